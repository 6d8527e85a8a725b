"""Stored frames without a GPU: the numpy restatement (tests/frames_ref.py) against the fixture drawn from the upstream file-backed class
(tests/golden/mm_stored.npz, tools/gen_golden_mm.py) and against torch's own bilinear interpolate on the CPU, the byte-level facts the
design rests on, the C entry points in a dry run, and the host side of datasets.StoredVPDataset / DATASET_CLASSES["MM"]."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frames_ref as R
from golden_util import GOLDEN_DIR
from vp_suite_amd import DATASET_CLASSES
from vp_suite_amd._lib import VpxError
from vp_suite_amd.datasets import MovingMNISTDataset, MovingMNISTOnTheFly, StoredVPDataset, procedural_digits
from vp_suite_amd.datasets.base import center_offset, parse_augmentations, parse_crop, parse_img_size
from vp_suite_amd.ops import check_frames_table

RESIZES = [((8, 8), (16, 16)), ((16, 16), (8, 8)), ((7, 10), (10, 7)), ((5, 6), (1, 1)), ((1, 6), (3, 12)), ((9, 10), (4, 33)), ((64, 64), (128, 128))]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "mm_stored.npz"))


@pytest.mark.parametrize("tag,value_range", [("01", (0.0, 1.0)), ("11", (-1.0, 1.0))])
def test_restatement_reproduces_the_stored_fixture(golden, tag, value_range):
    raw, want = golden["raw"], golden[f"frames_{tag}"]
    got = R.preprocess(raw, R.table([0, 1, 2]), 3, 2, c_out=3, value_range=value_range)
    assert got.dtype == np.float32 and got.shape == (3, 3, 3, 12, 10)
    for c in range(3):
        assert np.array_equal(got[:, :, c], want)
    assert want.min() == value_range[0] and want.max() == value_range[1]


def test_restatement_reproduces_the_fixture_postprocess_and_split(golden):
    x = golden["post_in"]
    assert x.min() < -1.0 and x.max() > 1.0
    for tag, value_range in (("01", (0.0, 1.0)), ("11", (-1.0, 1.0))):
        assert np.array_equal(R.postprocess(x, value_range), golden[f"post_{tag}"])
    train, val = R.train_val_indices(25, 0.96)
    assert train == golden["split_train"].tolist() and val == golden["split_val"].tolist()


@pytest.mark.parametrize("in_hw,out_hw", RESIZES)
def test_restatement_resize_against_torch_interpolate(in_hw, out_hw):
    """Bound 2e-6 on values in [-1, 1]: torch's CPU kernel computes the same coordinates and rounds its own interpolation in float32."""
    rng = np.random.default_rng(in_hw[0] * 1000 + out_hw[1])
    v = rng.uniform(-1.0, 1.0, size=(2, 3) + in_hw).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(v), size=out_hw, mode="bilinear", align_corners=False).numpy().astype(np.float64)
    got = R.resize(v, out_hw)
    assert got.shape == want.shape and got.dtype == np.float64
    err = np.abs(got - want).max()
    print(f"resize {in_hw} -> {out_hw}: max |restatement - torch| = {err:.3e}")
    assert err <= 2e-6


def test_byte_facts():
    b = np.arange(256, dtype=np.uint8)
    unit = R.scale(b)
    a = b.astype(np.float64) / 255.0                                   # the MMF kernel's expression for one glyph on a pixel
    a = np.minimum(np.maximum(a, 0.0), 1.0) * 255.0 / 255.0
    assert np.array_equal(a.astype(np.float32), unit)
    assert np.array_equal(R.postprocess(unit.reshape(1, 16, 16)).ravel(), b)          # range (0, 1): every byte survives the round trip
    back = R.postprocess(R.scale(b, (-1.0, 1.0)).reshape(1, 16, 16), (-1.0, 1.0)).ravel().astype(np.int64)
    drop = b.astype(np.int64) - back
    assert set(drop.tolist()) <= {0, 1} and int(drop.sum()) == 63                       # range (-1, 1): 63 bytes come back one lower
    assert drop[0] == 0 and drop[255] == 0


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def pre(src=p(1), dtype=0, N=60000, Tp=20, H=64, W=64, Cs=1, table=p(2), B=128, F=20, step=1, ch=64, cw=64, oh=64, ow=64, C_out=3, lo=0.0, hi=1.0, out=p(3)):
    return L.vpx_frames_preprocess(src, dtype, N, Tp, H, W, Cs, table, B, F, step, ch, cw, oh, ow, C_out, lo, hi, out, None)
def post(x=p(1), N=8, C=3, h=64, w=64, lo=0.0, hi=1.0, out=p(2)):
    return L.vpx_frames_postprocess(x, N, C, h, w, lo, hi, out, None)
def refused(fn, rc, word, **kw):
    got = fn(**kw)
    assert got == rc and word in L.vpx_last_error(), (kw, got, L.vpx_last_error())
assert pre() == OK and pre(oh=128, ow=128, lo=-1.0) == OK and pre(dtype=1, C_out=1) == OK and pre(dtype=2, Cs=3, C_out=3, ch=9, cw=10, oh=9, ow=10) == OK
assert pre(F=10, step=2) == OK and pre(N=1, Tp=1, H=1, W=1, B=1, F=1, ch=1, cw=1, oh=1, ow=1) == OK
for bad in (-1, 3, 7):
    refused(pre, E_ARG, b"unknown element type", dtype=bad)
refused(pre, E_ARG, b"NULL", src=None)
refused(pre, E_ARG, b"NULL", table=None)
refused(pre, E_ARG, b"NULL", out=None)
for name in ("N", "Tp", "H", "W", "Cs", "B", "F", "step", "ch", "cw", "oh", "ow"):
    refused(pre, E_ARG, b">= 1", **{name: 0})
refused(pre, E_ARG, b"stored frames", F=11, step=2)                 # (11 - 1) * 2 = 20 >= T'
refused(pre, E_ARG, b"stored frames", F=21)
refused(pre, E_ARG, b"no padding", ch=65)
refused(pre, E_ARG, b"no padding", cw=65)
refused(pre, E_ARG, b"output channels", C_out=2)
refused(pre, E_ARG, b"output channels", Cs=3, C_out=1)
refused(pre, E_ARG, b"output channels", Cs=2, C_out=3)
refused(pre, E_ARG, b"empty value range", lo=1.0)
refused(pre, E_UNSUPPORTED, b"stored channels", Cs=5, C_out=5)
refused(pre, E_UNSUPPORTED, b"a side beyond", oh=32769)
refused(pre, E_UNSUPPORTED, b"exceed one launch", B=2 ** 31 - 1, oh=4096, ow=4096)
assert post() == OK and post(C=1, w=7, lo=-1.0) == OK and post(N=1, C=5, h=1, w=1) == OK
refused(post, E_ARG, b"NULL", x=None)
refused(post, E_ARG, b"NULL", out=None)
for name in ("N", "C", "h", "w"):
    refused(post, E_ARG, b">= 1", **{name: 0})
refused(post, E_ARG, b"empty value range", lo=0.5, hi=0.5)
refused(post, E_UNSUPPORTED, b"a side beyond", w=32769)
refused(post, E_UNSUPPORTED, b"exceed one launch", N=2 ** 40, h=1024, w=1024)
print("dry run ok")
"""


def test_entry_points_in_a_dry_run():
    """vpx_frames_preprocess / _postprocess under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide): valid calls with
    fake pointers pass every host-side check and launch nothing; each documented refusal returns its code and names its reason."""
    from vp_suite_amd import _lib
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_launch_table_is_checked_on_the_host():
    ok = np.array([[2, 3, 4, 3], [0, 0, 0, 0]], dtype=np.int64)
    assert check_frames_table(ok, 3, (9, 10), (6, 6)).dtype == np.int32
    for col, bad, word in ((0, 3, "sequence index"), (0, -1, "sequence index"), (1, 4, "crop box"), (2, 5, "crop box"), (1, -1, "crop box"),
                           (2, -1, "crop box"), (3, 4, "flip bits"), (3, -1, "flip bits")):
        rows = ok.copy()
        rows[0, col] = bad
        with pytest.raises(ValueError, match=word):
            check_frames_table(rows, 3, (9, 10), (6, 6))
    with pytest.raises(ValueError, match="integer table"):
        check_frames_table(np.zeros((2, 5), dtype=np.int32), 3, (9, 10), (6, 6))
    with pytest.raises(ValueError, match="integer table"):
        check_frames_table(ok.astype(np.float32), 3, (9, 10), (6, 6))
    assert np.array_equal(R.table([2, 0], [(3, 4), (0, 0)], [3, 0]), ok)


class CenterCrop:
    def __init__(self, size):
        self.size = size


class RandomCrop(CenterCrop):
    pass


class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        self.p = p


class RandomVerticalFlip(RandomHorizontalFlip):
    pass


class ColorJitter:
    pass


def test_argument_parsing_and_refusals():
    assert parse_img_size(None, (9, 10)) == (9, 10) and parse_img_size(7, (9, 10)) == (7, 7) and parse_img_size([4, 5], (9, 10)) == (4, 5)
    for bad in ("64", (1, 2, 3), 0, (4, 0), 4.0, (4.0, 4)):
        with pytest.raises(ValueError, match="img size"):
            parse_img_size(bad, (9, 10))
    assert parse_crop(None) is None and parse_crop(("center", 4, 5)) == ("center", 4, 5) and parse_crop(["random", 3, 3]) == ("random", 3, 3)
    assert parse_crop(("box", 1, 2, 3, 4)) == ("box", 1, 2, 3, 4)
    assert parse_crop(CenterCrop(4)) == ("center", 4, 4) and parse_crop(RandomCrop((3, 5))) == ("random", 3, 5) and parse_crop(CenterCrop([6])) == ("center", 6, 6)
    for bad in ("center", ("center", 4), ("middle", 4, 4), ("box", 1, 2, 3), ("box", -1, 0, 2, 2), ("center", 0, 4), ColorJitter(), object()):
        with pytest.raises(ValueError):
            parse_crop(bad)
    assert parse_augmentations(None) == [] and parse_augmentations([("hflip", 0.5), ("vflip", 1)]) == [(1, 0.5), (2, 1.0)]
    assert parse_augmentations([RandomHorizontalFlip(), RandomVerticalFlip(0.25)]) == [(1, 0.5), (2, 0.25)]
    with pytest.raises(NotImplementedError, match="ColorJitter"):
        parse_augmentations([("hflip", 0.5), ColorJitter()])
    with pytest.raises(NotImplementedError, match="rotate"):
        parse_augmentations([("rotate", 0.5)])
    with pytest.raises(ValueError, match="probability"):
        parse_augmentations([("hflip", 1.5)])
    raw = np.zeros((4, 6, 9, 10), dtype=np.uint8)
    with pytest.raises(ValueError, match="does not fit"):
        StoredVPDataset("train", raw=raw, crop=("center", 10, 10))
    with pytest.raises(ValueError, match="leaves the"):
        StoredVPDataset("train", raw=raw, crop=("box", 6, 0, 4, 4))
    with pytest.raises(ValueError, match="uint8, uint16 or float32"):
        StoredVPDataset("train", raw=raw.astype(np.int32))
    with pytest.raises(ValueError, match="empty value range"):
        StoredVPDataset("train", raw=raw, value_range_min=1.0)
    with pytest.raises(ValueError, match="storage"):
        StoredVPDataset("train", raw=raw, storage="disk")
    with pytest.raises(ValueError, match="img size"):
        StoredVPDataset("train", raw=raw, img_size="big")
    ds = StoredVPDataset("train", raw=raw)
    for use in (lambda: ds[0], lambda: ds.batch([0]), lambda: next(iter(ds.loader(2)))):
        with pytest.raises(RuntimeError, match="set_seq_len"):
            use()
    with pytest.raises(ValueError, match="up to 6 frames"):
        ds.set_seq_len(4, 3, 1)


def test_center_offsets_at_odd_remainders():
    """torchvision's int(round((H - h) / 2.0)) with Python's round: halves go to the even neighbour."""
    assert [center_offset(10, 5), center_offset(9, 4), center_offset(8, 5), center_offset(12, 5), center_offset(9, 9), center_offset(10, 9)] == [2, 2, 2, 4, 0, 0]
    assert center_offset(7, 4) == 2 and center_offset(5, 4) == 0 and R.center_offset(10, 5) == 2 and R.center_offset(12, 5) == 4
    ds = StoredVPDataset("train", raw=np.zeros((2, 2, 9, 10), dtype=np.uint8), crop=("center", 4, 5))
    assert ds.table([1, 0]).tolist() == [[1, 2, 2, 0], [0, 2, 2, 0]] and ds.img_shape == (1, 4, 5)


def test_shapes_draws_and_loader_lengths():
    raw = np.zeros((10, 6, 9, 10, 3), dtype=np.uint8)
    ds = StoredVPDataset("train", raw=raw, crop=("random", 6, 7), img_size=(12, 5), augmentations=[("hflip", 0.5), ("vflip", 0.5)], transform_seed=3)
    ds.set_seq_len(2, 1, 2)
    assert (ds.img_shape, ds.MIN_SEQ_LEN, ds.DATASET_FRAME_SHAPE, ds.total_frames, ds.seq_len, len(ds)) == ((3, 12, 5), 6, (9, 10, 3), 3, 5, 10)
    cfg = ds.config
    assert (cfg["img_c"], cfg["img_h"], cfg["img_w"], cfg["action_size"], cfg["tensor_value_range"]) == (3, 12, 5, 0, [0.0, 1.0])
    assert cfg["crop"] == ("random", 6, 7) and cfg["storage"] == "device" and not {"transform_rng", "seq_len", "data_dir"} & set(cfg)
    rows = ds.table(list(range(10)))
    assert rows.dtype == np.int32 and rows[:, 0].tolist() == list(range(10))
    assert rows[:, 1].min() >= 0 and rows[:, 1].max() <= 3 and rows[:, 2].min() >= 0 and rows[:, 2].max() <= 3 and set(rows[:, 3].tolist()) <= {0, 1, 2, 3}
    assert len({tuple(r[1:]) for r in rows.tolist()}) > 3                               # boxes and flips differ per sequence
    assert not np.array_equal(ds.table(list(range(10)))[:, 1:], rows[:, 1:])
    ds.reset_rng()
    assert np.array_equal(ds.table(list(range(10))), rows)
    assert np.array_equal(ds.table([4, 5], transform=False), [[4, 0, 0, 0], [5, 0, 0, 0]])
    assert StoredVPDataset("train", raw=raw, img_size=(9, 10), crop=("center", 4, 4)).img_shape == (3, 4, 4)   # the stored size: no resize
    assert StoredVPDataset("train", raw=raw[..., :1], img_size=16).img_shape == (1, 16, 16)
    assert (len(ds.loader(3)), len(ds.loader(3, drop_last=False)), ds.loader(3, drop_last=False).sizes[-1], len(ds.loader(10)), len(ds.loader(11))) == (3, 4, 1, 1, 0)
    with pytest.raises(ValueError, match="batch_size"):
        ds.loader(0)


def _write_split(root, split, raw):
    os.makedirs(os.path.join(root, split))
    for i, seq in enumerate(raw):
        np.save(os.path.join(root, split, f"seq_{i:05d}.npy"), seq)


def test_file_backed_moving_mnist(golden, tmp_path):
    assert DATASET_CLASSES["MM"] is MovingMNISTDataset and DATASET_CLASSES["MMF"] is MovingMNISTOnTheFly and issubclass(MovingMNISTDataset, StoredVPDataset)
    assert "MM" in DATASET_CLASSES and DATASET_CLASSES.get("MM") is MovingMNISTDataset and DATASET_CLASSES.get("KTH") is None and "KTH" not in DATASET_CLASSES
    assert list(DATASET_CLASSES.stored) == ["MM"] and "MM" not in list(DATASET_CLASSES)   # registered, not listed: it needs files a user brings
    with pytest.raises(KeyError):
        DATASET_CLASSES["KTH"]
    cls = MovingMNISTDataset
    assert (cls.NAME, cls.ACTION_SIZE, cls.DATASET_FRAME_SHAPE, cls.train_to_val_ratio, cls.train_val_seed, cls.VALID_SPLITS) == \
        ("Moving MNIST", 0, (64, 64, 3), 0.96, 1234, ["train", "test"])
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        cls("train")
    with pytest.raises(VpxError, match="Nothing is downloaded"):
        cls("train", data_dir=str(tmp_path))
    raw = golden["raw"]
    _write_split(str(tmp_path), "train", raw)
    np.save(str(tmp_path / "train" / "notes.npy"), np.zeros(3))                      # not seq_NNNNN.npy: ignored
    ds = cls("train", data_dir=str(tmp_path), value_range_min=-1.0)
    ds.set_seq_len(2, 1, 2)
    assert (len(ds), ds.MIN_SEQ_LEN, ds.img_shape, ds.DATASET_FRAME_SHAPE) == (3, 6, (3, 12, 10), (12, 10, 3))
    assert np.array_equal(ds._raw_host, raw) and ds.origin(1).endswith(os.path.join("train", "seq_00001.npy"))
    assert ds.config["img_c"] == 3 and "data_fps" not in ds.config
    _write_split(str(tmp_path), "test", raw[:, :, :, :8])
    np.save(str(tmp_path / "test" / "seq_00002.npy"), raw[2])
    with pytest.raises(ValueError, match="seq_00002.npy"):
        cls("test", data_dir=str(tmp_path))
    os.makedirs(str(tmp_path / "many"))
    _write_split(str(tmp_path / "many"), "train", np.zeros((25, 2, 4, 4), dtype=np.uint8))
    train, val = cls.get_train_val(data_dir=str(tmp_path / "many"))
    assert train.indices == golden["split_train"].tolist() and val.indices == golden["split_val"].tolist()
    assert (len(train), len(val), train.MIN_SEQ_LEN, val.img_shape, len(train.loader(5)), len(val.loader(1))) == (24, 1, 2, (3, 4, 4), 4, 1)
    train.set_seq_len(1, 1, 1)
    assert val.ready_for_usage and val.dataset is train.dataset


def test_generated_dataset_still_refuses_transforms():
    glyphs = procedural_digits(n=12, size=7)
    for kw in ({"crop": ("center", 8, 8)}, {"augmentations": [("hflip", 0.5)]}):
        with pytest.raises(NotImplementedError, match="not part of this build"):
            DATASET_CLASSES["MMF"]("test", digits=glyphs, img_size=16, **kw)
    assert not MovingMNISTOnTheFly.SUPPORTS_TRANSFORMS and StoredVPDataset.SUPPORTS_TRANSFORMS
