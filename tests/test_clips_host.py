"""Long-clip datasets without a GPU: the restatement (tests/clips_ref.py) against the fixture drawn from the upstream KITTIRawDataset and
CaltechPedestrianDataset (tests/golden/clips_windows.npz, tools/gen_golden_clips.py), DATASET_CLASSES["KITTI"] / ["CP"] on an exported
tree of the fixture's names and lengths, every refusal of ops.check_clips_table and of the two classes, the registry, the C entry point
in a dry run, and the host side of datasets.ClipVPDataset."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import clips_ref as C
from golden_util import GOLDEN_DIR
from vp_suite_amd import DATASET_CLASSES
from vp_suite_amd._lib import VpxError
from vp_suite_amd.datasets import CaltechPedestrianDataset, ClipVPDataset, KITTIRawDataset, StoredVPDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_clips_like as X  # noqa: E402

CONFIGS = [(4, 1), (5, 2), (7, 3)]                     # (seq_len, seq_step): 4, 3 and 3 frames
SPLITS = ("train", "val", "test")
HW = (4, 6)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "clips_windows.npz"))


def _frames(seq_len, seq_step):
    return (seq_len - 1) // seq_step + 1


def test_fixture_holds_names_and_integers_only(golden):
    assert len(golden.files) == 28 and os.path.getsize(os.path.join(GOLDEN_DIR, "clips_windows.npz")) < 16384
    for k in golden.files:
        assert golden[k].dtype.kind in ("U", "i"), k
    assert golden["kitti_names"].tolist() == X.kitti_names(7) and golden["cp_names"].tolist() == X.cp_names(9)
    for tag in ("kitti", "cp"):                          # the splits are a partition of the tree (KITTI) / of its sets (CP)
        seqs = sorted(sum((golden[f"{tag}_{s}_seqs"].tolist() for s in SPLITS), []))
        assert seqs == list(range(len(golden[f"{tag}_names"])))


@pytest.mark.parametrize("tag", ["kitti", "cp"])
def test_restatement_equals_the_upstream_fixture(golden, tag):
    names, lengths = golden[f"{tag}_names"].tolist(), golden[f"{tag}_lengths"].tolist()
    n_windows = 0
    for split in SPLITS:
        seqs = (C.kitti_split if tag == "kitti" else C.cp_split)(names, split)
        assert [names.index(s) for s in seqs] == golden[f"{tag}_{split}_seqs"].tolist(), split
        for seq_len, seq_step in CONFIGS:
            want = golden[f"{tag}_{split}_win_{seq_len}_{seq_step}"]
            got = C.windows([lengths[names.index(s)] for s in seqs], seq_len, seq_step)
            assert got == [tuple(r) for r in want.tolist()], (split, seq_len, seq_step)
            n_windows += len(got)
    assert n_windows > 40
    assert C.windows([3, 4, 5, 9], 4, 1) == [(1, 0), (2, 0), (3, 0), (3, 4)] and C.windows([6], 7, 3) == []   # ends on the last frame; too short


@pytest.mark.parametrize("tag", ["kitti", "cp"])
def test_dataset_classes_equal_the_upstream_fixture_on_an_exported_tree(golden, tag, tmp_path):
    names, lengths = golden[f"{tag}_names"].tolist(), golden[f"{tag}_lengths"].tolist()
    files = X.export(tag, str(tmp_path), names, lengths, HW, seed=5)
    assert len(files) == len(names) and np.load(files[1]).shape == (lengths[1],) + HW + (3,)
    (tmp_path / "notes.txt").write_text("not a directory: ignored")
    cls = DATASET_CLASSES["KITTI" if tag == "kitti" else "CP"]
    for split in SPLITS:
        ds = cls(split, data_dir=str(tmp_path))
        rel = [os.path.relpath(p, os.path.realpath(str(tmp_path))) for p, _ in ds.sequences]
        rel = [r[:-len(".npy")] for r in rel] if tag == "cp" else rel
        want_seqs = golden[f"{tag}_{split}_seqs"].tolist()
        assert [names.index(r) for r in rel] == want_seqs, split
        assert [n for _, n in ds.sequences] == [lengths[i] for i in want_seqs] == ds.clip_lengths
        assert len(ds) == 0 and ds.img_shape == (3,) + HW and ds.DATASET_FRAME_SHAPE == HW + (3,)
        for seq_len, seq_step in CONFIGS:
            ds.set_seq_len(1, _frames(seq_len, seq_step) - 1, seq_step)
            want = golden[f"{tag}_{split}_win_{seq_len}_{seq_step}"].tolist()
            assert (ds.seq_len, len(ds)) == (seq_len, len(want))
            assert [(ds.sequences.index((p, lengths[names.index(_rel(p, tmp_path, tag))])), s) for p, s in ds.sequences_with_frame_index] == [tuple(r) for r in want]
            assert ds.windows == [tuple(r) for r in want]                                 # built anew by every call
        assert ds.origin(0) == f"{ds.sequences[want[0][0]][0]}, start frame: 0"
        assert "sequences" not in ds.config and ds.config["action_size"] == 0 and "supports_actions" not in ds.config
    train, val = cls.get_train_val(data_dir=str(tmp_path))
    assert (train.split, val.split, cls.get_test(data_dir=str(tmp_path)).split) == SPLITS and train is not val


def _rel(path, root, tag):
    rel = os.path.relpath(path, os.path.realpath(str(root)))
    return rel[:-len(".npy")] if tag == "cp" else rel


def test_class_constants_are_the_references():
    k, c = KITTIRawDataset, CaltechPedestrianDataset
    assert (k.NAME, k.MIN_SEQ_LEN, k.DATASET_FRAME_SHAPE, k.FPS, k.VALID_SPLITS, k.ACTION_SIZE) == ("KITTI raw", 994, (375, 1242, 3), 10, ["train", "val", "test"], 0)
    assert (k.camera, k.trainval_to_test_ratio, k.train_to_val_ratio, k.trainval_test_seed, k.train_val_seed) == ("image_02", 0.8, 0.9, 1234, 1234)
    assert k.AVAILABLE_CAMERAS == ["image_00", "image_01", "image_02", "image_03"]
    assert (c.NAME, c.MIN_SEQ_LEN, c.DATASET_FRAME_SHAPE, c.FPS, c.VALID_SPLITS, c.ACTION_SIZE) == ("Caltech Pedestrian", 568, (480, 640, 3), 30, ["train", "val", "test"], 0)
    assert (c.train_to_val_ratio, c.train_val_seed, c.TRAIN_VAL_SETS[0], c.TRAIN_VAL_SETS[-1], c.TEST_SETS[0], c.TEST_SETS[-1]) == (0.9, 1234, "set00", "set05", "set06", "set10")


def test_registry_finds_the_clip_datasets_and_does_not_list_them():
    assert DATASET_CLASSES["KITTI"] is KITTIRawDataset and DATASET_CLASSES["CP"] is CaltechPedestrianDataset
    assert "KITTI" in DATASET_CLASSES and "CP" in DATASET_CLASSES and DATASET_CLASSES.get("CP") is CaltechPedestrianDataset
    assert "KITTI" not in list(DATASET_CLASSES) and "CP" not in list(DATASET_CLASSES) and list(DATASET_CLASSES) == ["MMF"]
    assert list(DATASET_CLASSES.stored_clips) == ["KITTI", "CP"]
    assert issubclass(KITTIRawDataset, ClipVPDataset) and issubclass(ClipVPDataset, StoredVPDataset)
    assert "KTH" not in DATASET_CLASSES and DATASET_CLASSES.get("KTH") is None
    with pytest.raises(KeyError):
        DATASET_CLASSES["KTH"]


def test_both_datasets_refuse_what_the_reference_refuses(tmp_path):
    for cls in (KITTIRawDataset, CaltechPedestrianDataset):
        with pytest.raises(VpxError, match="Nothing is downloaded"):
            cls("train")
        with pytest.raises(VpxError, match="Nothing is downloaded"):
            cls("train", data_dir=str(tmp_path / "absent"))
        with pytest.raises(ValueError, match="has to be one of"):
            cls("validation", data_dir=str(tmp_path))
    two = tmp_path / "two"
    X.export("kitti", str(two), X.kitti_names(2), [5, 6], HW)
    for split in SPLITS:
        with pytest.raises(ValueError, match="found less than 3 sequences"):
            KITTIRawDataset(split, data_dir=str(two))
    three = tmp_path / "three"
    X.export("kitti", str(three), X.kitti_names(3), [5, 6, 7], HW)
    assert [len(KITTIRawDataset(s, data_dir=str(three)).sequences) for s in SPLITS] == [1, 1, 1]
    with pytest.raises(VpxError, match="image_03.npy"):
        KITTIRawDataset("train", data_dir=str(three), camera="image_03")
    only_test = tmp_path / "only_test"
    X.export("cp", str(only_test), ["set06/V000", "set00/V001"], [5, 6], HW)
    assert len(CaltechPedestrianDataset("test", data_dir=str(only_test)).sequences) == 1
    for split in ("train", "val"):
        with pytest.raises(ValueError, match="didn't find enough train/val sequences"):
            CaltechPedestrianDataset(split, data_dir=str(only_test))
    only_train = tmp_path / "only_train"
    X.export("cp", str(only_train), ["set00/V000", "set05/V001", "set11/V002"], [5, 6, 7], HW)
    with pytest.raises(ValueError, match="didn't find enough test sequences"):
        CaltechPedestrianDataset("test", data_dir=str(only_train))
    ds = CaltechPedestrianDataset("train", data_dir=str(only_train))
    assert len(ds.sequences) == 1
    with pytest.raises(ValueError, match="no clip holds the 7 frames"):
        ds.set_seq_len(3, 4, 1)
    with pytest.raises(RuntimeError, match="set_seq_len"):
        ds.batch([0])
    with pytest.raises(ValueError, match="up to 568 frames"):
        ds.set_seq_len(300, 300, 1)


def test_clips_table_is_checked_on_the_host():
    from vp_suite_amd.ops import check_clips_table
    first = C.clip_first([7, 12, 5])
    assert first.tolist() == [0, 7, 19, 24]
    ok = np.array([[0, 3, 3, 4, 3, 0], [1, 8, 0, 0, 0, 0], [2, 1, 0, 0, 0, 0]], dtype=np.int64)   # windows of 4 frames ending on their clips' last frames
    f, t = check_clips_table(ok, first, 4, 1, (9, 10), (6, 6))
    assert f.dtype == np.int64 and t.dtype == np.int32 and np.array_equal(t, ok) and np.array_equal(C.table([(0, 3), (1, 8), (2, 1)], [(3, 4), (0, 0), (0, 0)], [3, 0, 0]), ok)
    assert check_clips_table(torch.from_numpy(ok), torch.from_numpy(first), 2, 3, (9, 10), (6, 6))[1].shape == (3, 6)   # span 4 as well
    for row, col, bad, word in ((0, 0, 3, "clip index"), (0, 0, -1, "clip index"), (0, 1, 4, "leaves its clip"), (1, 1, 9, "leaves its clip"),
                                (2, 1, 2, "leaves its clip"), (0, 1, -1, "leaves its clip"), (0, 2, 4, "crop box"), (0, 3, 5, "crop box"),
                                (0, 2, -1, "crop box"), (0, 3, -1, "crop box"), (0, 4, 4, "flip bits"), (0, 4, -1, "flip bits"), (1, 5, 1, "reserved")):
        rows = ok.copy()
        rows[row, col] = bad
        with pytest.raises(ValueError, match=word):
            check_clips_table(rows, first, 4, 1, (9, 10), (6, 6))
    with pytest.raises(ValueError, match="leaves its clip"):                               # by one frame, through the step alone
        check_clips_table(ok, first, 3, 2, (9, 10), (6, 6))
    for bad in (np.zeros((2, 4), dtype=np.int32), np.zeros((0, 6), dtype=np.int32), np.zeros(6, dtype=np.int32), ok.astype(np.float32)):
        with pytest.raises(ValueError, match=re.escape("integer table [B, 6]")):
            check_clips_table(bad, first, 4, 1, (9, 10), (6, 6))
    for bad, word in (([0, 7, 7, 24], "increase strictly"), ([0, 19, 7, 24], "increase strictly"), ([1, 7, 19, 24], "start at 0"),
                      (np.array([0.0, 7.0]), "integer vector"), ([[0, 7]], "integer vector"), ([0], "integer vector")):
        with pytest.raises(ValueError, match=word):
            check_clips_table(ok[:1], np.asarray(bad), 4, 1, (9, 10), (6, 6))


def test_ops_refuse_before_any_launch():
    import vp_suite_amd as vpx
    first, rows = C.clip_first([7, 12]), C.table([(0, 0)])
    with pytest.raises(VpxError, match="GPU tensor"):
        vpx.ops.clips_preprocess(torch.zeros((19, 9, 10), dtype=torch.uint8), first, rows, 4)
    with pytest.raises(VpxError, match="GPU tensor"):
        vpx.ops.clips_preprocess(np.zeros((19, 9, 10), dtype=np.uint8), first, rows, 4)


def test_abi_export_is_in_the_header_the_library_and_the_table():
    from vp_suite_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vpx.h")).read()
    assert re.search(r"\bint vpx_clips_preprocess\(const void\* src, int dtype, long long total_frames,", hdr)
    assert "vpx_clips_preprocess" in _lib.SIGNATURES and "vpx_clips_preprocess" in _lib.EXPORTED_SYMBOLS
    fn = _lib.lib().vpx_clips_preprocess
    assert len(fn.argtypes) == 21 and fn.argtypes[6] is _lib.vp and fn.argtypes[7] is _lib.ll


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def pre(src=p(1), dtype=0, total=40000000, H=375, W=1242, Cs=3, first=p(2), n_clips=120, table=p(3), B=128, F=20, step=1, ch=375, cw=1242, oh=64, ow=64, C_out=3,
        lo=0.0, hi=1.0, out=p(4)):
    return L.vpx_clips_preprocess(src, dtype, total, H, W, Cs, first, n_clips, table, B, F, step, ch, cw, oh, ow, C_out, lo, hi, out, None)
def refused(rc, word, **kw):
    got = pre(**kw)
    assert got == rc and word in L.vpx_last_error(), (kw, got, L.vpx_last_error())
assert pre() == OK and pre(dtype=1, Cs=1, C_out=3, lo=-1.0) == OK and pre(dtype=2, Cs=1, C_out=1, ch=9, cw=10, oh=9, ow=10) == OK
assert pre(F=10, step=2) == OK and pre(total=1, n_clips=1, H=1, W=1, B=1, F=1, ch=1, cw=1, oh=1, ow=1) == OK
for bad in (-1, 3):
    refused(E_ARG, b"unknown element type", dtype=bad)
for name in ("src", "first", "table", "out"):
    refused(E_ARG, b"NULL", **{name: None})
for name in ("total", "n_clips", "H", "W", "Cs", "B", "F", "step", "ch", "cw", "oh", "ow"):
    refused(E_ARG, b">= 1", **{name: 0})
refused(E_ARG, b"a clip holds at least one", total=100, n_clips=101)
refused(E_ARG, b"stored frames", total=20, n_clips=1, F=11, step=2)   # (11 - 1) * 2 = 20 >= the frames
refused(E_ARG, b"no padding", ch=376)
refused(E_ARG, b"no padding", cw=1243)
refused(E_ARG, b"output channels", C_out=1)
refused(E_ARG, b"empty value range", lo=1.0)
refused(E_UNSUPPORTED, b"stored channels", Cs=5, C_out=5)
refused(E_UNSUPPORTED, b"a side beyond", ow=32769)
refused(E_UNSUPPORTED, b"exceed one launch", B=2 ** 31 - 1, oh=4096, ow=4096)
print("dry run ok")
"""


def test_entry_point_in_a_dry_run():
    """vpx_clips_preprocess under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide) on a machine without a GPU: valid
    calls with fake pointers pass every host-side check and launch nothing (a launch would fail here); each documented refusal returns
    its code and names its reason."""
    from vp_suite_amd import _lib
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_clip_dataset_host_side():
    clips = [np.zeros((n, 9, 10, 3), dtype=np.uint8) for n in (7, 12, 5)]
    ds = ClipVPDataset("train", clips=clips, crop=("random", 6, 7), img_size=(12, 5), augmentations=[("hflip", 0.5), ("invert", 0.5)], transform_seed=3)
    assert (len(ds), ds.MIN_SEQ_LEN, ds.img_shape, ds.DATASET_FRAME_SHAPE, ds.clip_first.tolist()) == (0, 12, (3, 12, 5), (9, 10, 3), [0, 7, 19, 24])
    ds.set_seq_len(2, 2, 1)
    assert ds.windows == C.windows([7, 12, 5], 4, 1) == [(0, 0), (1, 0), (1, 4), (1, 8), (2, 0)]
    ds.set_seq_len(4, 3, 1)
    assert ds.windows == [(0, 0), (1, 0)] and len(ds) == 2                                  # the 5-frame clip contributes none at seq_len 7
    ds.set_seq_len(2, 1, 2)
    assert ds.windows == [(0, 0), (1, 0), (1, 6), (2, 0)] and ds.origin(2) == "stored clip 1, start frame: 6"
    table, programs = ds.clips_table(ds.windows)
    assert table.dtype == np.int32 and table.shape == (4, 6) and table[:, :2].tolist() == [list(w) for w in ds.windows] and not table[:, 5].any()
    assert table[:, 2].max() <= 3 and table[:, 3].max() <= 3 and set(table[:, 4].tolist()) <= {0, 1} and len(programs) == 4
    ds.reset_rng()
    again, _ = ds.clips_table(ds.windows)
    assert np.array_equal(again, table)                                                     # one seeded draw per window, in index order
    cfg = ds.config
    assert (cfg["img_c"], cfg["img_h"], cfg["img_w"], cfg["action_size"]) == (3, 12, 5, 0) and not {"windows", "clip_first", "clip_lengths"} & set(cfg)
    assert (len(ds.loader(3)), len(ds.loader(3, drop_last=False))) == (1, 2)
    with pytest.raises(ValueError, match="up to 12 frames"):
        ds.set_seq_len(7, 6, 1)
    for bad, word in (([], "at least one clip"), ([clips[0], clips[1][:, :8]], "clip 1"), ([clips[0], clips[1].astype(np.uint16)], "clip 1"),
                      ([clips[0].astype(np.int32)], "uint8, uint16 or float32"), ([np.zeros((9, 10), dtype=np.uint8)], r"\[T, H, W\]")):
        with pytest.raises(ValueError, match=word):
            ClipVPDataset("train", clips=bad)
    with pytest.raises(ValueError, match="clips="):
        ClipVPDataset("train", raw=np.zeros((2, 3, 4, 4), dtype=np.uint8))
    with pytest.raises(NotImplementedError, match="no 'val' split"):
        ClipVPDataset.get_train_val(clips=clips)
    with pytest.raises(VpxError, match="holds no clips"):
        ClipVPDataset("train")._stored()


def test_export_tool_writes_seeded_trees(tmp_path):
    assert "NOT KITTI OR CALTECH DATA" in X.__doc__
    a = X.export("cp", str(tmp_path / "a"), X.cp_names(3), [3, 4, 5], HW, seed=2)
    b = X.export("cp", str(tmp_path / "b"), X.cp_names(3), [3, 4, 5], HW, seed=2)
    assert [np.load(f).shape[0] for f in a] == [3, 4, 5] and all(np.array_equal(np.load(x), np.load(y)) for x, y in zip(a, b))
    assert not np.array_equal(np.load(a[0])[:3], np.load(a[1])[:3]) and np.load(a[0]).dtype == np.uint8
    with pytest.raises(FileExistsError):
        X.export("cp", str(tmp_path / "a"), X.cp_names(3), [3, 4, 5], HW)
    with pytest.raises(ValueError, match="layout"):
        X.export("kth", str(tmp_path / "c"), ["x"], [3])
    assert X.default_lengths(4, 12, 30) == [12, 19, 26, 14]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_clips_like.py"), "kitti", str(tmp_path / "k"), "--clips", "3", "--height", "4", "--width", "6"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "NOT the dataset" in r.stdout
    assert [len(KITTIRawDataset(s, data_dir=str(tmp_path / "k")).sequences) for s in SPLITS] == [1, 1, 1]
