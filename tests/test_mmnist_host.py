"""Moving MNIST on the fly without a GPU: the numpy restatement (tests/mmnist_ref.py) against the fixture drawn from the upstream class
(tests/golden/mmnist_otf.npz, tools/gen_golden_mmnist.py), the package's host sampler against both, the trajectory rule at its corners,
the idx reader, the refusals, the registry, and the C entry point in a dry run."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import mmnist_ref as R
from golden_util import GOLDEN_DIR
from vp_suite_amd import AVAILABLE_DATASETS, DATASET_CLASSES
from vp_suite_amd._lib import VpxError
from vp_suite_amd.datasets import MovingMNISTOnTheFly, VPDataset, procedural_digits, read_idx_images
from vp_suite_amd.datasets.mmnist_on_the_fly import check_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"test": ("test", (0.0, 1.0), {}), "train": ("train", (-1.0, 1.0), {"value_range_min": -1.0})}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "mmnist_otf.npz"))


@pytest.fixture(scope="module")
def small_glyphs():
    return procedural_digits(n=12, size=7)


def test_procedural_digits_are_the_fixture_glyphs(golden):
    g = procedural_digits()
    assert g.dtype == np.uint8 and g.shape == (16, 28, 28)
    assert np.array_equal(g, golden["glyphs"])
    assert g.max() == 255 and g.min() == 0 and len(np.unique(g)) > 64          # values spread over the byte range
    assert all((g[i] > 0).any() for i in range(len(g))) and not np.array_equal(g[0], g[10])
    assert procedural_digits(n=3, size=9).shape == (3, 9, 9)


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_restatement_reproduces_the_reference_fixture(golden, tag):
    split, value_range, _ = CONFIGS[tag]
    glyphs, want = golden["glyphs"], golden[f"frames_{tag}"]
    params = R.Sampler(split, len(glyphs), glyphs.shape[1]).params(len(want))
    assert np.array_equal(params, golden[f"params_{tag}"])
    got = R.render(glyphs, params, want.shape[1], 3, 64, value_range)
    assert got.dtype == np.float32 and got.shape == (len(want), want.shape[1], 3, 64, 64)
    for c in range(3):
        assert np.array_equal(got[:, :, c], want)
    assert want.min() == value_range[0] and want.max() == value_range[1]


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_host_sampler_yields_the_fixture_rows(golden, tag):
    split, _, kwargs = CONFIGS[tag]
    ds = MovingMNISTOnTheFly(split, digits=golden["glyphs"], **kwargs)
    rows = ds.sample_params(3)
    assert rows.dtype == np.int32 and np.array_equal(rows, golden[f"params_{tag}"])


@pytest.mark.parametrize("num_digits", [1, 3])
@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_host_sampler_equals_the_restatement(small_glyphs, split, num_digits):
    kw = dict(img_size=16, num_digits=num_digits, max_speed=4, rng_seed=77)
    ds = MovingMNISTOnTheFly(split, digits=small_glyphs, **kw)
    ref = R.Sampler(split, len(small_glyphs), 7, **kw)
    rows = ds.sample_params(5)
    assert rows.shape == (5, num_digits, 5) and np.array_equal(rows, ref.params(5))
    assert (np.abs(rows[..., 3:]) >= 2).all() and (np.abs(rows[..., 3:]) <= 4).all()
    assert rows[..., 1:3].min() >= 0 and rows[..., 1:3].max() < 16 - 7 and rows[..., 0].max() < len(small_glyphs)


def test_batch_rows_equal_single_draws_and_reset_restarts(small_glyphs):
    a, b = (MovingMNISTOnTheFly("val", digits=small_glyphs, img_size=16) for _ in range(2))
    batch = a.sample_params(4)
    singles = np.concatenate([b.sample_params(1) for _ in range(4)])
    assert np.array_equal(batch, singles)
    nxt = a.sample_params(4)
    assert not np.array_equal(nxt, batch)
    a.reset_rng()
    assert np.array_equal(a.sample_params(4), batch)


def test_the_three_splits_differ(small_glyphs):
    rows = {s: MovingMNISTOnTheFly(s, digits=small_glyphs, img_size=16).sample_params(4) for s in ("train", "val", "test")}
    assert not np.array_equal(rows["train"], rows["val"]) and not np.array_equal(rows["val"], rows["test"]) and not np.array_equal(rows["train"], rows["test"])
    assert [len(MovingMNISTOnTheFly(s, digits=small_glyphs, img_size=16)) for s in ("train", "val", "test")] == [9600, 400, 1000]
    assert len(MovingMNISTOnTheFly("val", digits=small_glyphs, img_size=16, n_seqs=6)) == 6


def test_trajectory_rule():
    S, s = 16, 7   # positions 0 .. 9
    assert R.trajectory(5, 4, 1, S, s) == [9] and R.move(5, 4, S, s) == (9, 4)                 # ends exactly on the wall: no bounce
    assert R.move(9, 4, S, s) == (9, -4)                                                       # ... the next move overshoots: lands on the wall, turns
    assert R.move(6, 4, S, s) == (9, -4)                                                       # overshoot by 1
    assert R.move(9, 5, S, s) == (9, -5)                                                       # overshoot by max_speed
    assert R.move(0, -3, S, s) == (3, 3) and R.trajectory(0, -3, 3, S, s) == [3, 6, 9]          # start at 0, negative speed: mirrored
    assert R.move(2, -2, S, s) == (0, -2) and R.move(0, -2, S, s) == (2, 2)                     # reaching 0 exactly is no bounce either
    assert R.trajectory(4, 5, 5, S, s) == [9, 9, 4, 1, 6]                                       # two bounces (far wall, then 0: -1 mirrored to 1)
    assert R.trajectory(1, -4, 4, S, s) == [3, 7, 9, 5]                                         # ... (0, then the far wall)
    assert R.trajectory(3, 9, 3, S, s) == [9, 0, 9]                                             # the largest speed the wrapper admits: S - s


def _write_idx(path, images):
    with open(path, "wb") as fh:
        fh.write(b"\x00\x00\x08\x03" + struct.pack(">III", *images.shape) + images.tobytes())


def test_idx_reader_and_data_dir(tmp_path):
    images = (np.arange(3 * 5 * 5) * 7 % 256).astype(np.uint8).reshape(3, 5, 5)
    raw = tmp_path / "MNIST" / "raw"
    raw.mkdir(parents=True)
    _write_idx(raw / "t10k-images-idx3-ubyte", images)
    assert np.array_equal(read_idx_images(str(raw / "t10k-images-idx3-ubyte")), images)
    for split in ("val", "test"):
        assert np.array_equal(MovingMNISTOnTheFly(split, data_dir=str(tmp_path), img_size=12).digits, images)
    with pytest.raises(VpxError, match="train-images-idx3-ubyte"):   # the train split reads the other file
        MovingMNISTOnTheFly("train", data_dir=str(tmp_path), img_size=12)
    _write_idx(tmp_path / "train-images-idx3-ubyte", images[::-1].copy())   # ... also found at the top level of data_dir
    assert np.array_equal(MovingMNISTOnTheFly("train", data_dir=str(tmp_path), img_size=12).digits, images[::-1])
    (tmp_path / "bad").write_bytes(b"\x00\x00\x08\x03" + struct.pack(">III", 3, 5, 5) + b"\x00" * 10)
    with pytest.raises(VpxError, match="header says"):
        read_idx_images(str(tmp_path / "bad"))
    (tmp_path / "worse").write_bytes(b"\x00\x00\x0d\x03" + b"\x00" * 12)
    with pytest.raises(VpxError, match="not an idx file"):
        read_idx_images(str(tmp_path / "worse"))


def test_refusals(small_glyphs, tmp_path):
    with pytest.raises(VpxError, match="t10k-images-idx3-ubyte"):
        MovingMNISTOnTheFly("test")
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        MovingMNISTOnTheFly("test", data_dir=str(tmp_path))
    with pytest.raises(ValueError, match="num_channels"):
        MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=16, num_channels=2)
    for size in (7, 6):                                             # s >= S
        with pytest.raises(ValueError, match="do not move inside"):
            MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=size)
    with pytest.raises(ValueError, match="max_speed"):              # max_speed > S - s
        MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=11)
    MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=12)   # (max_speed == S - s is fine)
    with pytest.raises(ValueError, match="has to be one of"):
        MovingMNISTOnTheFly("validation", digits=small_glyphs, img_size=16)
    with pytest.raises(ValueError):
        MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=(16, 16))
    with pytest.raises(ValueError, match="uint8"):
        MovingMNISTOnTheFly("test", digits=small_glyphs.astype(np.float32), img_size=16)
    for kw in ({"crop": object()}, {"augmentations": [object()]}):
        with pytest.raises(NotImplementedError):
            MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=16, **kw)
    ds = MovingMNISTOnTheFly("test", digits=small_glyphs, img_size=16)
    assert not ds.ready_for_usage
    for use in (lambda: ds[0], lambda: ds.batch(2), lambda: next(iter(ds.loader(2)))):
        with pytest.raises(RuntimeError, match="set_seq_len"):
            use()


def test_launch_table_is_checked_on_the_host():
    ok = np.array([[[0, 0, 9, 9, -9]]], dtype=np.int32)
    assert check_params(ok, 12, 7, 16).dtype == np.int32
    for col, bad, word in ((0, 12, "glyph index"), (0, -1, "glyph index"), (1, 10, "start position"), (2, -1, "start position"), (3, 10, "speed"), (4, -10, "speed")):
        rows = ok.copy()
        rows[0, 0, col] = bad
        with pytest.raises(ValueError, match=word):
            check_params(rows, 12, 7, 16)
    with pytest.raises(ValueError, match="integer table"):
        check_params(np.zeros((2, 5), dtype=np.int32), 12, 7, 16)
    with pytest.raises(ValueError, match="integer table"):
        check_params(ok.astype(np.float32), 12, 7, 16)


def test_registry_and_config(small_glyphs):
    assert list(DATASET_CLASSES) == ["MMF"] and list(AVAILABLE_DATASETS) == ["MMF"] and DATASET_CLASSES["MMF"] is MovingMNISTOnTheFly
    assert issubclass(MovingMNISTOnTheFly, VPDataset) and MovingMNISTOnTheFly.VALID_SPLITS == ["train", "val", "test"]
    cls = MovingMNISTOnTheFly
    assert (cls.min_speed, cls.max_speed, cls.min_acc, cls.max_acc, cls.num_digits, cls.rng_seed, cls.num_channels, cls.img_size) == (2, 5, 0, 0, 2, 4115, 3, 64)
    assert cls.SPLIT_SEED_OFFSETS["test"](cls.rng_seed) == 12345 and cls.ON_THE_FLY and cls.ACTION_SIZE == 0
    ds = cls("train", digits=small_glyphs, img_size=16, num_channels=1, value_range_min=-1.0)
    ds.set_seq_len(4, 3, 2)
    assert (ds.total_frames, ds.seq_len, ds.seq_step, list(ds.frame_offsets)) == (7, 13, 2, [0, 2, 4, 6, 8, 10, 12]) and ds.ready_for_usage
    cfg = ds.config
    assert (cfg["img_c"], cfg["img_h"], cfg["img_w"], cfg["action_size"], cfg["tensor_value_range"], cfg["NAME"]) == (1, 16, 16, 0, [-1.0, 1.0], cls.NAME)
    assert cfg["split"] == "train" and cfg["num_digits"] == 2 and cfg["max_speed"] == 5 and cfg["img_shape"] == (1, 16, 16) and cfg["seq_step"] == 2
    assert not {"digits", "seq_len", "total_frames", "ready_for_usage", "pos_rng", "data_dir"} & set(cfg)
    assert len(ds.loader(128)) == 75 and len(ds.loader(1000, drop_last=False)) == 10 and ds.loader(1000, drop_last=False).sizes[-1] == 600


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def call(digits=p(1), N=16, s=28, params=p(2), B=128, D=2, F=20, C=1, S=64, lo=0.0, hi=1.0, out=p(3)):
    return L.vpx_mmnist_frames(digits, N, s, params, B, D, F, C, S, lo, hi, out, None)
def refused(rc, word, **kw):
    got = call(**kw)
    assert got == rc and word in L.vpx_last_error(), (kw, got, L.vpx_last_error())
assert call() == OK and call(C=3, lo=-1.0) == OK and call(B=1, D=1, F=1, S=29) == OK and call(D=16, S=33, s=12) == OK
refused(E_ARG, b"channels", C=2)
refused(E_ARG, b"channels", C=0)
refused(E_ARG, b"does not move inside", s=64)
refused(E_ARG, b"does not move inside", s=65)
refused(E_ARG, b"at least one digit", D=0)
refused(E_ARG, b"NULL", digits=None)
refused(E_ARG, b"NULL", params=None)
refused(E_ARG, b"NULL", out=None)
refused(E_ARG, b">= 1", B=0)
refused(E_ARG, b">= 1", F=0)
refused(E_ARG, b">= 1", N=0)
refused(E_UNSUPPORTED, b"digits per sample", D=17)
refused(E_UNSUPPORTED, b"bytes of LDS", D=16, s=56)
refused(E_UNSUPPORTED, b"image side", S=16385)
refused(E_UNSUPPORTED, b"frames per sample", F=65537)
refused(E_UNSUPPORTED, b"exceed one launch", B=2 ** 31 - 1, F=8)     # more workgroups than a grid holds
print("dry run ok")
"""


def test_entry_point_in_a_dry_run():
    """vpx_mmnist_frames under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide): a valid call with fake pointers
    passes every host-side check and launches nothing; each documented refusal returns its code and names its reason."""
    from vp_suite_amd import _lib
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
