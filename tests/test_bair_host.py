"""Stored sequences that carry actions, without a GPU: the numpy restatement (tests/bair_ref.py) against the fixture drawn from the
upstream BAIRPushingDataset (tests/golden/bair_stored.npz, tools/gen_golden_bair.py), the host side of DATASET_CLASSES["BAIR"] and of
StoredVPDataset(actions=...), the registry, and vpx_actions_gather in a dry run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bair_ref as R
import frames_ref
from golden_util import GOLDEN_DIR
from vp_suite_amd import DATASET_CLASSES, _lib
from vp_suite_amd._lib import VpxError
from vp_suite_amd.datasets import BAIRPushingDataset, StoredVPDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_bair_like  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "bair_stored.npz"))


@pytest.mark.parametrize("step", [1, 2])
def test_restatement_reproduces_the_stored_fixture(golden, step):
    obs, actions = golden["obs"], golden["actions"]
    assert obs.dtype == np.uint8 and actions.dtype == np.float64 and actions[0, 0, 0] == 1.0 + 2.0 ** -24
    got = R.gather(actions, [0, 1, 2], 5, step)
    assert got.dtype == np.float32 and got.shape == (3, 5, 4) and np.array_equal(got, golden[f"actions_s{step}"])
    assert got[0, 0].tolist() == [1.0, float(np.float32(-1.0 - 2.0 ** -22)), float(np.finfo(np.float32).max), float(np.float32(0.1))]
    for i in range(3):
        rows, _ = R.sample(obs[i], actions[i], 5, step)
        assert np.array_equal(rows, obs[i, 0:(4 * step + 1):step])
    frames = frames_ref.preprocess(obs, frames_ref.table([0, 1, 2]), 5, step)
    assert np.array_equal(frames, golden[f"frames_s{step}"])


def test_export_tool_writes_the_layout_and_says_what_it_is(tmp_path):
    assert "NOT BAIR DATA" in export_bair_like.__doc__
    assert export_bair_like.export(str(tmp_path), {"train": 3, "test": 2}, n_frames=5, img_size=4, seed=9) == 5
    names = sorted(os.listdir(tmp_path / "softmotion30_44k" / "train"))
    assert names == [f"seq_{i:05d}_{kind}.npy" for i in range(3) for kind in ("actions", "obs")]
    obs, actions = np.load(tmp_path / "softmotion30_44k" / "test" / "seq_00001_obs.npy"), np.load(tmp_path / "softmotion30_44k" / "test" / "seq_00001_actions.npy")
    assert (obs.dtype, obs.shape, actions.dtype, actions.shape) == (np.uint8, (5, 4, 4, 3), np.float32, (5, 4))
    again = export_bair_like.synthetic_split(2, 5, 4, seed=9, split="test")
    assert np.array_equal(again[0][1], obs) and np.array_equal(again[1][1], actions)                # seeded
    assert not np.array_equal(export_bair_like.synthetic_split(2, 5, 4, seed=9, split="train")[0], again[0])
    with pytest.raises(FileExistsError):
        export_bair_like.export(str(tmp_path), {"train": 1})


def test_bair_discovery_refusals_and_config(golden, tmp_path):
    cls = BAIRPushingDataset
    assert (cls.NAME, cls.REFERENCE, cls.MIN_SEQ_LEN, cls.ACTION_SIZE, cls.DATASET_FRAME_SHAPE, cls.train_to_val_ratio, cls.VALID_SPLITS) == \
        ("BAIR robot pushing", "https://arxiv.org/abs/1710.05268", 30, 4, (64, 64, 3), 0.96, ["train", "test"])
    assert issubclass(cls, StoredVPDataset) and not hasattr(cls, "download_and_prepare_dataset")
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        cls("train")
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        cls("train", data_dir=str(tmp_path))
    obs, actions = golden["obs"], golden["actions"]
    target = export_bair_like.write_split(str(tmp_path), "train", obs, actions)
    np.save(os.path.join(target, "notes.npy"), np.zeros(3))                              # neither *obs.npy nor *actions.npy: ignored
    ds = cls("train", data_dir=str(tmp_path), value_range_min=-1.0)
    assert ds.obs_ids == [f"seq_{i:05d}_obs.npy" for i in range(3)] and ds.actions_ids == [f"seq_{i:05d}_actions.npy" for i in range(3)]
    assert len(ds) == 3 and ds.origin(2) == os.path.join(os.path.realpath(target), "seq_00002_obs.npy") and ds.data_dir == os.path.realpath(target)
    assert np.array_equal(ds._raw_host, obs) and np.array_equal(ds._actions_host, actions) and ds._actions_host.dtype == np.float64
    assert (ds.MIN_SEQ_LEN, ds.ACTION_SIZE, ds.img_shape, ds.DATASET_FRAME_SHAPE) == (30, 4, (3, 8, 8), (8, 8, 3))
    cfg = ds.config
    assert cfg["action_size"] == 4 and cfg["supports_actions"] is True and cfg["tensor_value_range"] == [-1.0, 1.0] and cfg["NAME"] == cls.NAME
    assert not {"obs_fps", "actions_fps", "obs_ids", "actions_ids", "data_dir"} & set(cfg)
    ds.set_seq_len(10, 20, 1)
    assert ds.seq_len == 30 and list(ds.frame_offsets) == list(range(30))
    ds.set_seq_len(8, 7, 2)
    assert ds.seq_len == 29 and list(ds.frame_offsets) == list(range(0, 30, 2))
    with pytest.raises(ValueError, match="up to 30 frames"):
        ds.set_seq_len(10, 21, 1)
    with pytest.raises(ValueError, match="up to 30 frames"):
        ds.set_seq_len(8, 8, 2)
    assert cls("train", data_dir=str(tmp_path), img_size=16).img_shape == (3, 16, 16)
    # the reference's two ValueErrors
    os.remove(os.path.join(target, "seq_00001_actions.npy"))
    with pytest.raises(ValueError, match="Different number of obs and action files found"):
        cls("train", data_dir=str(tmp_path))
    os.makedirs(tmp_path / "softmotion30_44k" / "test")
    with pytest.raises(ValueError, match="No trajectory files"):
        cls("test", data_dir=str(tmp_path))


def test_bair_refuses_a_file_that_differs_from_the_first(golden, tmp_path):
    obs, actions = golden["obs"], golden["actions"]
    cases = {"obs_shape": ("seq_00002_obs.npy", obs[2][:, :, :6]), "obs_dtype": ("seq_00001_obs.npy", obs[1].astype(np.uint16)),
             "act_shape": ("seq_00002_actions.npy", actions[2][:29]), "act_dtype": ("seq_00001_actions.npy", actions[1].astype(np.float32))}
    for tag, (name, data) in cases.items():
        target = export_bair_like.write_split(str(tmp_path / tag), "train", obs, actions)
        np.save(os.path.join(target, name), data)
        with pytest.raises(ValueError, match=name):
            BAIRPushingDataset("train", data_dir=str(tmp_path / tag))
    target = export_bair_like.write_split(str(tmp_path / "five"), "train", obs, np.zeros((3, 30, 5)))
    with pytest.raises(ValueError, match=r"seq_00000_actions.npy: expected actions \[t, 4\]"):
        BAIRPushingDataset("train", data_dir=str(tmp_path / "five"))
    target = export_bair_like.write_split(str(tmp_path / "ints"), "train", obs, np.zeros((3, 30, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="float32 or float64"):
        BAIRPushingDataset("train", data_dir=str(tmp_path / "ints"))


@pytest.mark.parametrize("n", [25, 50])
def test_bair_train_val_split_sizes(tmp_path, n):
    export_bair_like.export(str(tmp_path), {"train": n, "test": 2}, n_frames=2, img_size=2)
    train, val = BAIRPushingDataset.get_train_val(data_dir=str(tmp_path))
    assert len(train) == int(n * 0.96) and len(val) == n - int(n * 0.96)
    assert train.indices == frames_ref.train_val_indices(n, 0.96)[0] and val.indices == frames_ref.train_val_indices(n, 0.96)[1]
    assert val.dataset is train.dataset and train.config["supports_actions"] is True and train.ACTION_SIZE == 4
    assert len(BAIRPushingDataset.get_test(data_dir=str(tmp_path))) == 2


def test_registry_finds_bair_by_key_and_does_not_list_it():
    assert DATASET_CLASSES["BAIR"] is BAIRPushingDataset and "BAIR" in DATASET_CLASSES and DATASET_CLASSES.get("BAIR") is BAIRPushingDataset
    assert "BAIR" not in list(DATASET_CLASSES) and "BAIR" not in list(DATASET_CLASSES.keys()) and "BAIR" not in [k for k, _ in DATASET_CLASSES.items()]
    assert list(DATASET_CLASSES.stored_with_actions) == ["BAIR"] and len(DATASET_CLASSES) == 1
    with pytest.raises(KeyError):
        DATASET_CLASSES["KTH"]


def test_stored_actions_argument_refusals_and_config():
    raw = np.zeros((4, 6, 9, 10, 3), dtype=np.uint8)
    good = np.zeros((4, 6, 5), dtype=np.float32)
    for bad in (np.zeros((3, 6, 5)), np.zeros((4, 5, 5)), np.zeros((4, 6)), np.zeros((4, 6, 5, 1)), np.zeros((4, 6, 0))):
        with pytest.raises(ValueError, match=r"stored actions must be \[N, T', A\]"):
            StoredVPDataset("train", raw=raw, actions=bad.astype(np.float32))
    for dtype in (np.float16, np.int32, np.uint8):
        with pytest.raises(ValueError, match="float32 or float64"):
            StoredVPDataset("train", raw=raw, actions=good.astype(dtype))
    with pytest.raises(ValueError, match="give raw= as well"):
        StoredVPDataset("train", actions=good)
    for dtype in (np.float32, np.float64):
        ds = StoredVPDataset("train", raw=raw, actions=good.astype(dtype), storage="pinned")
        assert ds.ACTION_SIZE == 5 and ds.config["action_size"] == 5 and ds.config["supports_actions"] is True and StoredVPDataset.ACTION_SIZE == 0
        assert ds._actions_host.dtype == dtype and not {"actions"} & set(ds.config)
    plain = StoredVPDataset("train", raw=raw)
    assert plain.ACTION_SIZE == 0 and plain.config["action_size"] == 0 and "supports_actions" not in plain.config


def test_draws_without_actions_are_the_parent_commits():
    """Two calls of table() on a dataset without actions, and on one with them: the rows this class drew before actions existed."""
    raw = np.zeros((10, 6, 9, 10, 3), dtype=np.uint8)
    kw = dict(raw=raw, crop=("random", 6, 7), augmentations=[("hflip", 0.5), ("vflip", 0.5)], transform_seed=3)
    for extra in ({}, {"actions": np.zeros((10, 6, 4), dtype=np.float64)}):
        ds = StoredVPDataset("train", **kw, **extra)
        assert ds.table([7, 2, 9, 0]).tolist() == [[7, 3, 0, 1], [2, 3, 2, 3], [9, 2, 1, 1], [0, 0, 0, 1]]
        assert ds.table([1, 1]).tolist() == [[1, 1, 1, 0], [1, 3, 3, 1]]
    assert sorted(StoredVPDataset("train", **kw).config) == [
        "NAME", "action_size", "augmentations", "crop", "device", "img_c", "img_h", "img_shape", "img_size", "img_w", "photometric", "seq_step", "split",
        "storage", "tensor_value_range", "train_to_val_ratio", "train_val_seed", "transform_seed", "value_range_max", "value_range_min"]


def test_workbench_leaves_use_actions_open_only_for_datasets_with_actions(vpx):
    from vp_suite_amd.vpsuite import VPSuite

    class Model:
        def __init__(self, can, ac):
            self.CAN_HANDLE_ACTIONS, self.config = can, {"action_conditional": ac}

    class Data:
        def __init__(self, **extra):
            self.config = {"action_size": 0, **extra}

    run = {"use_actions": False, "epochs": 1}
    pick = VPSuite._open_use_actions
    assert pick(run, {}, Model(True, True), [Data(), Data(supports_actions=True)])["use_actions"] is True and run["use_actions"] is False
    assert pick(run, {}, Model(True, True), [Data()]) is run and pick(run, {}, Model(True, True), [Data(supports_actions=False)]) is run
    assert pick(run, {}, Model(True, False), [Data(supports_actions=True)]) is run and pick(run, {}, Model(False, True), [Data(supports_actions=True)]) is run
    assert pick(run, {"use_actions": False}, Model(True, True), [Data(supports_actions=True)]) is run
    doc = vpx.vpsuite.__doc__
    assert "supports_actions" in doc and "use_actions" in doc
    assert "supports_actions" in vpx.datasets.bair.__doc__ and "supports_actions" in vpx.datasets.base.__doc__


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def gather(src=p(1), dtype=0, N=44000, Tp=30, A=4, table=p(2), B=128, F=30, step=1, out=p(3)):
    return L.vpx_actions_gather(src, dtype, N, Tp, A, table, B, F, step, out, None)
def refused(rc, word, **kw):
    got = gather(**kw)
    assert got == rc and word in L.vpx_last_error(), (kw, got, L.vpx_last_error())
assert (_lib.ACTIONS_F32, _lib.ACTIONS_F64) == (0, 1)
assert gather() == OK and gather(dtype=1) == OK and gather(F=15, step=2) == OK and gather(F=10, step=3) == OK and gather(F=1, step=29) == OK
assert gather(N=1, Tp=1, A=1, B=1, F=1) == OK and gather(A=5, B=3) == OK
for bad in (-1, 2, 3):
    refused(E_ARG, b"unknown element type", dtype=bad)
for name in ("src", "table", "out"):
    refused(E_ARG, b"NULL", **{name: None})
for name in ("N", "Tp", "A", "B", "F", "step"):
    refused(E_ARG, b">= 1", **{name: 0})
    refused(E_ARG, b">= 1", **{name: -3})
refused(E_ARG, b"stored frames", F=31)                              # (31 - 1) * 1 + 1 > 30
refused(E_ARG, b"stored frames", F=16, step=2)                      # (16 - 1) * 2 + 1 = 31 > 30
refused(E_ARG, b"stored frames", F=2, step=30)
refused(E_UNSUPPORTED, b"exceed one launch", B=2 ** 31 - 1, Tp=2 ** 20, F=2 ** 20, A=2 ** 10)
print("dry run ok")
"""


def test_entry_point_in_a_dry_run():
    """vpx_actions_gather under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide): valid calls with fake pointers pass
    every host-side check and launch nothing; each documented refusal returns its code and names its reason."""
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_abi_lists_the_entry_point():
    assert "vpx_actions_gather" in _lib.SIGNATURES and "vpx_actions_gather" in _lib.EXPORTED_SYMBOLS
    fn = getattr(_lib.lib(), "vpx_actions_gather")
    assert fn is not None and len(fn.argtypes) == 11
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "vpx_actions_gather" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "vpx.h")) as fh:
        header = fh.read()
    assert "int vpx_actions_gather(const void* src, int dtype, long long N, int Tp, int A, const int* table, int B, int n_frames, int seq_step," in header
    assert "vpx_actions_gather " in header.split("#ifndef")[0] and "enum { VPX_ACTIONS_F32 = 0, VPX_ACTIONS_F64 = 1 };" in header
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert "vpx_actions_gather" in fh.read()


def test_ops_refuses_host_tensors_and_bad_shapes(vpx):
    import torch
    table = np.array([[0, 0, 0, 0]], dtype=np.int32)
    with pytest.raises(VpxError, match="GPU tensor"):
        vpx.ops.actions_gather(torch.zeros(2, 3, 4), table, 3, 1)
    with pytest.raises(VpxError, match="GPU tensor"):
        vpx.ops.actions_gather(np.zeros((2, 3, 4), dtype=np.float32), table, 3, 1)
