"""Human 3.6M, Physics 101 and SynPick without a GPU: the restatement (tests/video_ref.py) against the fixture drawn from the upstream
Human36MDataset and SynpickMovingDataset (tests/golden/video_windows.npz, tools/gen_golden_video.py), DATASET_CLASSES["H36M"] / ["P101"]
/ ["SPM"] on an exported tree of the fixture's names and lengths, the registry's four tiers, every refusal of the classes and of
ops.check_clips_var_table, both new C entry points in a dry run, and the host side of a mixed-shape ClipVPDataset with positions."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import video_ref as V
from golden_util import GOLDEN_DIR
from vp_suite_amd import DATASET_CLASSES
from vp_suite_amd._lib import VpxError
from vp_suite_amd.datasets import ClipVPDataset, Human36MDataset, Physics101Dataset, SynpickMovingDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_video_like as X  # noqa: E402

CONFIGS = [(4, 1), (5, 2), (7, 3)]                     # (seq_len, seq_step): 4, 3 and 3 frames
SPLITS = ("train", "val", "test")
HW = (4, 6)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "video_windows.npz"))


def _frames(seq_len, seq_step):
    return (seq_len - 1) // seq_step + 1


def test_fixture_holds_names_integers_and_small_float_arrays(golden):
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "video_windows.npz")) <= 200_000
    for k in golden.files:
        assert golden[k].dtype.kind in ("U", "i", "f") and golden[k].size <= 720, k
    assert golden["h36m_names"].tolist() == X.h36m_names(16) and golden["h36m_scenarios"].tolist() == ["WalkingDog"]
    assert (golden["h36m_lengths"] < 4 + 25).any()                                          # one video too short for any window
    assert {n.split("/")[-1].split(" ")[0] for n in golden["h36m_names"].tolist()} == {"Directions", "WalkingDog"}


def test_h36m_restatement_equals_the_upstream_fixture(golden):
    names, lengths = golden["h36m_names"].tolist(), golden["h36m_lengths"].tolist()
    n_windows = 0
    for split in SPLITS:
        seqs = V.h36m_split(names, split, ["WalkingDog"])
        assert [names.index(s) for s in seqs] == golden[f"h36m_{split}_seqs"].tolist(), split
        for seq_len, seq_step in CONFIGS:
            got = V.h36m_windows([lengths[names.index(s)] for s in seqs], seq_len, seq_step)
            assert got == [tuple(r) for r in golden[f"h36m_{split}_win_{seq_len}_{seq_step}"].tolist()], (split, seq_len, seq_step)
            n_windows += len(got)
    assert n_windows > 40 and V.h36m_windows([28, 29, 33], 4, 1) == [(1, 25), (2, 25), (2, 29)]


def test_h36m_class_equals_the_upstream_fixture_on_an_exported_tree(golden, tmp_path):
    names, lengths = golden["h36m_names"].tolist(), golden["h36m_lengths"].tolist()
    sizes = [(HW[0] + 2 * (k % 3 == 2), HW[1]) for k in range(len(names))]                 # every third video two rows taller
    files = X.export("h36m", str(tmp_path), names, lengths, HW, seed=5, sizes=sizes)
    assert np.load(files[2]).shape == (lengths[2], HW[0] + 2, HW[1], 3)
    root = os.path.realpath(str(tmp_path))
    for split in SPLITS:
        ds = Human36MDataset(split, data_dir=str(tmp_path), scenarios=["WalkingDog"], img_size=(5, 7))
        rel = [os.path.relpath(p, root)[:-len(".npy")] for p in ds.sequences]
        want_seqs = golden[f"h36m_{split}_seqs"].tolist()
        assert [names.index(r) for r in rel] == want_seqs and list(ds.sequences.values()) == [lengths[i] for i in want_seqs] == ds.clip_lengths
        assert ds.clip_hw == [sizes[i] for i in want_seqs] and ds.img_shape == (3, 5, 7) and len(ds) == 0
        for seq_len, seq_step in CONFIGS:
            ds.set_seq_len(1, _frames(seq_len, seq_step) - 1, seq_step)
            want = [tuple(r) for r in golden[f"h36m_{split}_win_{seq_len}_{seq_step}"].tolist()]
            assert ds.windows == want and [(list(ds.sequences).index(p), s) for p, s in ds.sequences_with_frame_index] == want
        assert ds.origin(0) == f"{list(ds.sequences)[0]}, start frame: 25"
        assert "sequences" not in ds.config and ds.config["action_size"] == 0 and "supports_actions" not in ds.config
    train = Human36MDataset("train", data_dir=str(tmp_path), scenarios=["WalkingDog"], img_size=(5, 7))
    assert train.mixed_shapes
    with pytest.raises(ValueError, match="need img_size="):
        Human36MDataset("train", data_dir=str(tmp_path), scenarios=["WalkingDog"])
    with pytest.raises(ValueError, match="acceptable choices"):
        Human36MDataset("train", data_dir=str(tmp_path), scenarios=["Dancing"])
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        Human36MDataset("train", data_dir=str(tmp_path / "absent"))
    tr, va = Human36MDataset.get_train_val(data_dir=str(tmp_path), img_size=(5, 7))
    assert (tr.split, va.split) == ("train", "val") and len(tr.sequences) == int(12 * 0.96) and len(va.sequences) == 1


def test_class_constants_are_the_references():
    h, p, s = Human36MDataset, Physics101Dataset, SynpickMovingDataset
    assert (h.NAME, h.MIN_SEQ_LEN, h.DATASET_FRAME_SHAPE, h.FPS, h.SKIP_FIRST_N, h.VALID_SPLITS, h.ACTION_SIZE, h.train_to_val_ratio) == \
        ("Human 3.6M", 994, (1000, 1000, 3), 50, 25, ["train", "val", "test"], 0, 0.96)
    assert len(h.ALL_SCENARIOS) == 17 and h.ALL_SCENARIOS[0] == "Directions" and h.ALL_SCENARIOS[-1] == "WalkingDog"
    assert (p.NAME, p.MIN_SEQ_LEN, p.DATASET_FRAME_SHAPE, p.VALID_SPLITS, p.ACTION_SIZE) == ("Physics 101", 16, (1080, 1920, 3), ["train", "test"], 0)
    assert (p.camera, p.subseq, p.trainval_to_test_ratio, p.trainval_test_seed) == ("Kinect_RGB_1", "middle", 0.8, 1612)
    assert p.AVAILABLE_CAMERAS == ["Camera_1", "Camera_2", "Kinect_RGB_1"] and p.AVAILABLE_SUBSEQ == ["start", "middle", "end"]
    assert (s.NAME, s.MIN_SEQ_LEN, s.DATASET_FRAME_SHAPE, s.SKIP_FIRST_N, s.VALID_SPLITS, s.ACTION_SIZE, s.train_to_val_ratio) == \
        ("SynPick - Moving", 90, (135, 240, 3), 72, ["train", "val", "test"], 3, 0.9)


def test_registry_has_four_stored_tiers_and_lists_none_of_them():
    assert DATASET_CLASSES["H36M"] is Human36MDataset and DATASET_CLASSES["P101"] is Physics101Dataset and DATASET_CLASSES["SPM"] is SynpickMovingDataset
    for key in ("H36M", "P101", "SPM"):
        assert key in DATASET_CLASSES and DATASET_CLASSES.get(key) is DATASET_CLASSES[key] and key not in list(DATASET_CLASSES)
        assert issubclass(DATASET_CLASSES[key], ClipVPDataset)
    assert list(DATASET_CLASSES) == ["MMF"] and list(DATASET_CLASSES.stored) == ["MM"] and list(DATASET_CLASSES.stored_with_actions) == ["BAIR"]
    assert list(DATASET_CLASSES.stored_clips) == ["KITTI", "CP"] and list(DATASET_CLASSES.stored_video) == ["H36M", "P101", "SPM"]
    assert "KTH" not in DATASET_CLASSES and DATASET_CLASSES.get("KTH") is None
    with pytest.raises(KeyError):
        DATASET_CLASSES["KTH"]
    assert type(DATASET_CLASSES)({"a": 1}, {"b": 2}).stored_video == {}                       # the new argument is optional


def test_spm_restatement_and_class_equal_the_upstream_fixture(golden, tmp_path):
    lengths = golden["spm_lengths"].tolist()
    for split in SPLITS:
        track = golden[f"spm_{split}_gripper"]
        tracks = [track[:lengths[0]], track[lengths[0]:]]
        X.export("spm", str(tmp_path), X.spm_names(2, split), lengths, HW, seed=3, grippers=tracks)
        ds = SynpickMovingDataset(split, data_dir=str(tmp_path))
        assert ds.clip_lengths == lengths and ds.config["supports_actions"] is True and ds.config["action_size"] == 3 and not ds.mixed_shapes
        for seq_len, seq_step in CONFIGS:
            want = golden[f"spm_{split}_valid_{seq_len}_{seq_step}"].tolist()
            valid, wins, why = V.spm_windows(lengths, tracks, seq_len, seq_step)
            assert valid == want and all(why[k] for k in ("skip", "episode_end", "overlap"))
            n_frames = _frames(seq_len, seq_step)
            ds.set_seq_len(1, n_frames - 1, seq_step)
            assert ds.valid_idx == want and ds.windows == wins and len(ds) == len(want)
            assert [int(ds.clip_first[c]) + s for c, s in ds.windows] == want
            for tag, (c, s) in (("first", wins[0]), ("last", wins[-1])):
                upstream = golden[f"spm_{split}_diff_{tag}_{seq_len}_{seq_step}"]
                assert upstream.dtype == np.float64 and upstream.shape == (n_frames - 1, 3)
                assert np.array_equal(V.action_diffs(tracks[c], s, n_frames, seq_step), upstream.astype(np.float32))
        assert ds.origin(0).startswith(f"1st frame: {ds.episode_fps[0]}, frame 72")
    fired = set()
    for seq_len, seq_step in CONFIGS:
        fired |= {k for k, n in V.spm_windows(lengths, tracks, seq_len, seq_step)[2].items() if n}
    assert fired == {"skip", "episode_end", "overlap", "too_still", "too_far"}


def test_spm_refusals(tmp_path):
    still = [np.zeros((100, 3)), np.zeros((100, 3))]
    X.export("spm", str(tmp_path), X.spm_names(2), [100, 100], HW, grippers=still)
    ds = SynpickMovingDataset("train", data_dir=str(tmp_path))
    with pytest.raises(ValueError, match="No valid indices"):
        ds.set_seq_len(2, 2, 1)
    assert not ds.ready_for_usage
    with pytest.raises(ValueError, match="up to 90 frames"):
        ds.set_seq_len(50, 50, 1)
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        SynpickMovingDataset("val", data_dir=str(tmp_path))
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        SynpickMovingDataset("train")
    os.remove(os.path.join(str(tmp_path), "processed", "train", "000001_gripper.npy"))
    with pytest.raises(VpxError, match="000001_gripper.npy"):
        SynpickMovingDataset("train", data_dir=str(tmp_path))


def test_p101_splits_and_subseq_starts(tmp_path):
    names, lengths = X.p101_names(10), [9, 12, 7, 15, 10, 8, 11, 14, 13, 16]
    X.export("p101", str(tmp_path), names, lengths, HW, seed=2)
    X.export("p101", str(tmp_path), names[:2], [5, 5], HW, camera="Camera_1")
    root = os.path.realpath(str(tmp_path))
    for split in ("train", "test"):
        want = V.p101_split(names, split)
        for subseq in ("start", "middle", "end"):
            ds = Physics101Dataset(split, data_dir=str(tmp_path), subseq=subseq)
            assert [os.path.relpath(os.path.dirname(p), root) for p in ds.vid_filepaths] == want and len(ds) == len(want) == (8 if split == "train" else 2)
            ds.set_seq_len(2, 1, 3)                                                         # seq_len 7: 3 frames at step 3
            assert ds.seq_len == 7 and len(ds) == len(want)                                 # one sample per video
            T = [lengths[names.index(w)] for w in want]
            assert ds.windows == [(c, V.p101_start(t, 7, subseq)) for c, t in enumerate(T)]
            assert ds.windows == [(c, {"start": 0, "end": t - 7, "middle": (t - 7) // 2}[subseq]) for c, t in enumerate(T)]
            assert ds.origin(0) == f"{ds.vid_filepaths[0]}, subseq mode: {subseq}"
    ds = Physics101Dataset("train", data_dir=str(tmp_path))
    with pytest.raises(ValueError, match="fewer than the 9 of a window"):
        ds.set_seq_len(4, 5, 1)                                                             # the 7- and 8-frame videos are in this split
    assert not ds.ready_for_usage
    with pytest.raises(ValueError, match="up to 16 frames"):
        ds.set_seq_len(9, 9, 1)
    for kw in (dict(camera="Camera_3"), dict(subseq="late")):
        with pytest.raises(ValueError, match="acceptable choices"):
            Physics101Dataset("train", data_dir=str(tmp_path), **kw)
    with pytest.raises(ValueError, match="has to be one of"):
        Physics101Dataset("val", data_dir=str(tmp_path))
    assert len(Physics101Dataset("train", data_dir=str(tmp_path), camera="Camera_1").vid_filepaths) == 1
    train, val = Physics101Dataset.get_train_val(data_dir=str(tmp_path))                    # no "val" split: by index
    assert (len(train), len(val)) == (6, 2) and train.dataset is val.dataset and sorted(train.indices + val.indices) == list(range(8))


def test_mixed_shape_clip_dataset_host_side():
    clips = [np.zeros((7, 6, 10, 3), dtype=np.uint8), np.zeros((12, 7, 9, 3), dtype=np.uint8), np.zeros((5, 9, 6, 3), dtype=np.uint8)]
    with pytest.raises(ValueError, match="need img_size="):
        ClipVPDataset("train", clips=clips)
    with pytest.raises(ValueError, match="clip 1"):
        ClipVPDataset("train", clips=[clips[0], clips[1][..., :1]], img_size=4)
    with pytest.raises(ValueError, match="does not fit the 6x10 frames of clip 0"):
        ClipVPDataset("train", clips=clips, img_size=4, crop=("center", 7, 6))
    ds = ClipVPDataset("train", clips=clips, img_size=(5, 7), crop=("center", 4, 5))
    assert ds.mixed_shapes and ds.img_shape == (3, 5, 7) and ds.clip_hw == [(6, 10), (7, 9), (9, 6)] and ds.config["action_size"] == 0
    ds.set_seq_len(2, 2, 1)
    table, programs = ds.clips_var_table(ds.windows)
    assert ds.windows == [(0, 0), (1, 0), (1, 4), (1, 8), (2, 0)] and table.dtype == np.int32 and table.shape == (5, 8)
    assert table[:, 2:6].tolist() == [[1, 2, 4, 5], [2, 2, 4, 5], [2, 2, 4, 5], [2, 2, 4, 5], [2, 0, 4, 5]]   # centred in each clip's own frame
    whole = ClipVPDataset("train", clips=clips, img_size=(5, 7))
    whole.set_seq_len(2, 2, 1)
    assert whole.clips_var_table([(2, 0), (0, 1)])[0].tolist() == [[2, 0, 0, 0, 9, 6, 0, 0], [0, 1, 0, 0, 6, 10, 0, 0]]
    rnd = ClipVPDataset("train", clips=clips, img_size=(5, 7), crop=("random", 4, 5), augmentations=[("hflip", 0.5)], transform_seed=3)
    rnd.set_seq_len(2, 2, 1)
    a = rnd.clips_var_table(rnd.windows)[0]
    rnd.reset_rng()
    assert np.array_equal(rnd.clips_var_table(rnd.windows)[0], a)                           # one seeded draw per window, in index order
    assert (a[:, 2] + 4 <= [6, 7, 7, 7, 9]).all() and (a[:, 3] + 5 <= [10, 9, 9, 9, 6]).all() and set(a[:, 6].tolist()) <= {0, 1}
    rng = np.random.default_rng(3)                                                          # StoredVPDataset's order: box row, box column, flips
    for row, (c, _) in zip(a, rnd.windows):
        H, W = rnd.clip_hw[c]
        assert (row[2], row[3], row[6]) == (int(rng.integers(0, H - 4 + 1)), int(rng.integers(0, W - 5 + 1)), int(rng.random() < 0.5))
    # positions
    pos = [np.zeros((n, 3)) for n in (7, 12, 5)]
    ds = ClipVPDataset("train", clips=clips, positions=pos, img_size=(5, 7))
    assert ds.ACTION_SIZE == 3 and ds.config["supports_actions"] is True and ds.config["action_size"] == 3
    for bad, word in (([pos[0], pos[1][:11], pos[2]], "positions of clip 1"), (pos[:2], "one per clip"), ([p.astype(np.int64) for p in pos], "float32 or float64"),
                      ([pos[0], pos[1][:, :2], pos[2]], "positions of clip 1"), ([pos[0], pos[1].astype(np.float32), pos[2]], "positions of clip 1")):
        with pytest.raises(ValueError, match=word):
            ClipVPDataset("train", clips=clips, positions=bad, img_size=(5, 7))
    with pytest.raises(ValueError, match="clips= as well"):
        ClipVPDataset("train", positions=pos)

    class Every(ClipVPDataset):                                                             # the hook: a rule of its own
        def _window_starts(self, clip_index, frame_count):
            return range(clip_index, frame_count - self.seq_len + 1, 5)
    ds = Every("train", clips=clips, img_size=4)
    ds.set_seq_len(2, 2, 1)
    assert ds.windows == [(0, 0), (1, 1), (1, 6)]


def test_clips_var_table_is_checked_on_the_host():
    from vp_suite_amd.ops import check_clips_var_table
    geom = np.array([[0, 7, 6, 10], [1260, 12, 7, 9], [3528, 5, 9, 6]], dtype=np.int64)      # 3 channels: 7*180, 12*189, 5*162 elements
    total = 3528 + 810
    ok = np.array([[0, 3, 2, 5, 4, 5, 3, 0], [1, 8, 0, 0, 7, 9, 0, 0], [2, 1, 8, 5, 1, 1, 0, 0]], dtype=np.int64)   # windows and boxes touching every far edge
    g, t = check_clips_var_table(ok, geom, total, 3, 4, 1)
    assert g.dtype == np.int64 and t.dtype == np.int32 and np.array_equal(t, ok) and np.array_equal(g, geom)
    for row, col, bad, word in ((0, 0, 3, "clip index"), (0, 0, -1, "clip index"), (0, 1, 4, "leaves its clip"), (1, 1, 9, "leaves its clip"),
                                (0, 1, -1, "leaves its clip"), (0, 2, 3, "crop box"), (0, 3, 6, "crop box"), (0, 2, -1, "crop box"), (0, 3, -1, "crop box"),
                                (0, 4, 0, "crop box"), (0, 5, 0, "crop box"), (0, 4, 5, "crop box"), (2, 5, 2, "crop box"), (1, 4, 8, "crop box"),
                                (0, 6, 4, "flip bits"), (0, 6, -1, "flip bits"), (1, 7, 1, "reserved")):
        rows = ok.copy()
        rows[row, col] = bad
        with pytest.raises(ValueError, match=word):
            check_clips_var_table(rows, geom, total, 3, 4, 1)
    with pytest.raises(ValueError, match="leaves its clip"):                                # by one frame, through the step alone
        check_clips_var_table(ok, geom, total, 3, 3, 2)
    with pytest.raises(ValueError, match="a clip leaves the 4337 stored elements"):
        check_clips_var_table(ok, geom, total - 1, 3, 4, 1)
    with pytest.raises(ValueError, match="a clip leaves"):
        check_clips_var_table(ok, geom, total, 4, 4, 1)
    for row, col, bad in ((0, 0, -1), (1, 1, 0), (1, 2, 0), (2, 3, 0), (2, 3, 32769)):
        bad_geom = geom.copy()
        bad_geom[row, col] = bad
        with pytest.raises(ValueError, match="clip_geom"):
            check_clips_var_table(ok, bad_geom, 10 ** 12, 3, 4, 1)
    for bad in (np.zeros((2, 6), dtype=np.int32), np.zeros((0, 8), dtype=np.int32), np.zeros(8, dtype=np.int32), ok.astype(np.float32)):
        with pytest.raises(ValueError, match=re.escape("integer table [B, 8]")):
            check_clips_var_table(bad, geom, total, 3, 4, 1)
    for bad in (np.zeros((2, 3), dtype=np.int64), geom.astype(np.float64), geom[0]):
        with pytest.raises(ValueError, match=re.escape("integer table [n_clips, 4]")):
            check_clips_var_table(ok, bad, total, 3, 4, 1)


def test_ops_refuse_before_any_launch():
    import torch
    import vp_suite_amd as vpx
    with pytest.raises(VpxError, match="GPU tensor"):
        vpx.ops.clips_preprocess_var(torch.zeros(100, dtype=torch.uint8), [[0, 1, 10, 10]], [[0, 0, 0, 0, 10, 10, 0, 0]], 1, out_size=(4, 4))
    with pytest.raises(VpxError, match="GPU tensor"):
        vpx.ops.actions_diff_gather(torch.zeros((10, 3)), [0, 10], [[0, 0, 0, 0, 0, 0, 0, 0]], 2)


def test_abi_exports_are_in_the_header_the_library_and_the_table():
    from vp_suite_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vpx.h")).read()
    assert re.search(r"\bint vpx_clips_preprocess_var\(const void\* src, int dtype, long long total_elems, int Cs, const long long\* clip_geom,", hdr)
    assert re.search(r"\bint vpx_actions_diff_gather\(const void\* src, int dtype, long long total_frames, int A, const long long\* clip_first,", hdr)
    for name, n_args in (("vpx_clips_preprocess_var", 17), ("vpx_actions_diff_gather", 12)):
        assert name in _lib.SIGNATURES and name in _lib.EXPORTED_SYMBOLS
        fn = getattr(_lib.lib(), name)
        assert len(fn.argtypes) == n_args and fn.argtypes[2] is _lib.ll and fn.argtypes[4] is _lib.vp and fn.argtypes[5] is _lib.ll


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def pre(src=p(1), dtype=0, total=40000000000, Cs=3, geom=p(2), n_clips=120, table=p(3), B=128, F=20, step=1, oh=64, ow=64, C_out=3, lo=0.0, hi=1.0, out=p(4)):
    return L.vpx_clips_preprocess_var(src, dtype, total, Cs, geom, n_clips, table, B, F, step, oh, ow, C_out, lo, hi, out, None)
def diff(src=p(1), dtype=1, total=40000, A=3, first=p(2), n_clips=120, table=p(3), B=128, F=20, step=1, out=p(4)):
    return L.vpx_actions_diff_gather(src, dtype, total, A, first, n_clips, table, B, F, step, out, None)
def refused(fn, rc, word, **kw):
    got = fn(**kw)
    assert got == rc and word in L.vpx_last_error(), (fn.__name__, kw, got, L.vpx_last_error())
assert pre() == OK and pre(dtype=1, Cs=1, C_out=3, lo=-1.0) == OK and pre(dtype=2, Cs=1, C_out=1, oh=9, ow=10) == OK
assert pre(F=10, step=2) == OK and pre(total=1, Cs=1, C_out=1, n_clips=1, B=1, F=1, oh=1, ow=1) == OK
for bad in (-1, 3):
    refused(pre, E_ARG, b"unknown element type", dtype=bad)
for name in ("src", "geom", "table", "out"):
    refused(pre, E_ARG, b"NULL", **{name: None})
for name in ("total", "n_clips", "Cs", "B", "F", "step", "oh", "ow"):
    refused(pre, E_ARG, b">= 1", **{name: 0})
refused(pre, E_ARG, b"a clip holds at least one", total=300, n_clips=101)
refused(pre, E_ARG, b"stored elements", total=60, n_clips=1, F=11, step=2)   # (11 - 1) * 2 = 20 >= 60 / 3 pixels
refused(pre, E_ARG, b"output channels", C_out=1)
refused(pre, E_ARG, b"empty value range", lo=1.0)
refused(pre, E_UNSUPPORTED, b"stored channels", Cs=5, C_out=5)
refused(pre, E_UNSUPPORTED, b"a side beyond", ow=32769)
refused(pre, E_UNSUPPORTED, b"exceed one launch", B=2 ** 31 - 1, oh=4096, ow=4096)
assert diff() == OK and diff(dtype=0, A=1, F=2, step=3) == OK and diff(total=2, n_clips=1, B=1, F=2) == OK
for bad in (-1, 2):
    refused(diff, E_ARG, b"unknown element type", dtype=bad)
for name in ("src", "first", "table", "out"):
    refused(diff, E_ARG, b"NULL", **{name: None})
for name in ("total", "n_clips", "A", "B", "F", "step"):
    refused(diff, E_ARG, b">= 1", **{name: 0})
refused(diff, E_ARG, b"needs two frames", F=1)
refused(diff, E_ARG, b"a clip holds at least one", total=100, n_clips=101)
refused(diff, E_ARG, b"stored frames", total=20, n_clips=1, F=11, step=2)
refused(diff, E_UNSUPPORTED, b"exceed one launch", total=2 ** 40, B=2 ** 31 - 1, F=2 ** 20, A=2 ** 20)
print("dry run ok")
"""


def test_entry_points_in_a_dry_run():
    """vpx_clips_preprocess_var and vpx_actions_diff_gather under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide)
    on a machine without a GPU: valid calls with fake pointers pass every host-side check and launch nothing (a launch would fail
    here); each documented refusal returns its code and names its reason."""
    from vp_suite_amd import _lib
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_export_tool_writes_seeded_trees(tmp_path):
    assert "THIS IS NOT HUMAN 3.6M, PHYSICS 101 OR SYNPICK DATA" in X.__doc__
    a = X.export("spm", str(tmp_path / "a"), X.spm_names(2), [80, 90], HW, seed=2)
    b = X.export("spm", str(tmp_path / "b"), X.spm_names(2), [80, 90], HW, seed=2)
    assert all(np.array_equal(np.load(x), np.load(y)) for x, y in zip(a, b)) and np.load(a[0]).dtype == np.uint8
    ga, gb = np.load(a[1][:-4] + "_gripper.npy"), np.load(b[1][:-4] + "_gripper.npy")
    assert ga.shape == (90, 3) and ga.dtype == np.float64 and np.array_equal(ga, gb)
    with pytest.raises(FileExistsError):
        X.export("spm", str(tmp_path / "a"), X.spm_names(2), [80, 90], HW)
    with pytest.raises(ValueError, match="layout"):
        X.export("kth", str(tmp_path / "c"), ["x"], [3])
    for layout, cls, kw in (("h36m", Human36MDataset, dict(img_size=(4, 6))), ("p101", Physics101Dataset, {}), ("spm", SynpickMovingDataset, {})):
        out = tmp_path / layout
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_video_like.py"), layout, str(out), "--clips", "8", "--height", "4", "--width", "6"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "NOT the dataset" in r.stdout, r.stderr
        ds = cls("train", data_dir=str(out), **kw)
        ds.set_seq_len(2, 2, 1)
        assert len(ds) >= 1
