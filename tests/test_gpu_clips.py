"""vpx_clips_preprocess on the GPU: windows of long clips to batches, against the restatement (tests/clips_ref.py: the clip sliced, then
the stored-frame arithmetic of tests/frames_ref.py) run in the test.

The shapes are the smallest at which the launch can go wrong: clips of 7, 12 and 5 frames of 9 x 10 pixels (ow % 4 = 2: element stores
and a partial last group per row), stored as uint8 RGB, uint16 gray and float32 gray; 4 frames at step 1 and 3 frames at step 2. The
windows cover: one ending on the last frame of its clip; one starting at frame 0 of the clip AFTER a longer clip (a wrong offset table
shows there); B = 1 and B = 5 with a repeated row; the 5-frame clip contributing no window at seq_len 7.

EXACT cases (torch.equal): without resize a value is one float32 division and, for a range other than (0, 1), one multiply and one add.
BOUNDED cases (resize): |kernel - float64 restatement| <= 10 * 2^-24 * max(1, |dst|) per element, the bar of the stored-sequence launch
(tests/test_gpu_frames.py derives it: 9 float32 roundings to first order, the tenth for the second-order terms); the per-pixel device
code is the same function, so the same expression bounds it.
CONSISTENCY: with equal-length clips and every start 0 the launch equals vpx_frames_preprocess bit for bit, resize and flips included."""
import os
import sys

import numpy as np
import pytest
import torch

import clips_ref as C
import frames_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_clips_like as X  # noqa: E402

LENGTHS = (7, 12, 5)
KINDS = {"u8_rgb": (np.uint8, 3), "u16_gray": (np.uint16, 1), "f32_gray": (np.float32, 1)}
# (n_frames, seq_step, windows of B = 5, window of B = 1): each set ends on the last frame of clips 0 and 1, starts at frame 0 of clip 2
# (the clip after the longer one) and repeats a row; the single window ends on the last frame of the 5-frame clip
SETS = {"4x1": (4, 1, [(0, 3), (2, 0), (1, 8), (1, 0), (0, 3)], [(2, 1)]),
        "3x2": (3, 2, [(0, 2), (2, 0), (1, 7), (1, 1), (0, 2)], [(2, 0)])}


def _clips(kind, lengths=LENGTHS, hw=(9, 10), seed=0):
    dtype, channels = KINDS[kind]
    rng = np.random.default_rng([seed, len(kind)])
    shape = hw + ((channels,) if channels > 1 else ())
    if dtype == np.float32:
        return [rng.uniform(-0.25, 1.25, size=(n,) + shape).astype(np.float32) for n in lengths]
    clips = [rng.integers(0, np.iinfo(dtype).max + 1, size=(n,) + shape).astype(dtype) for n in lengths]
    clips[0].reshape(-1)[:2] = (0, np.iinfo(dtype).max)
    return clips


def _run(vpx, clips, rows, n_frames, **kw):
    src = torch.from_numpy(np.concatenate(clips)).cuda()
    return vpx.ops.clips_preprocess(src, C.clip_first([c.shape[0] for c in clips]), rows, n_frames, **kw)


def _exact(parity_log, name, got, ref):
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert got.is_cuda and got.dtype == ref.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    parity_log(name, got.float(), ref.float(), 0.0)
    assert torch.equal(got.cpu(), ref), f"{name}: {int((got.cpu() != ref).sum())} of {ref.numel()} values differ"


def _bounded(parity_log, name, got, ref):
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == ref.shape and ref.dtype == np.float64
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    bound = 10.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))
    worst = float((err / bound).max())
    print(f"{name}: max |kernel - restatement| = {err.max():.3e}, worst share of the per-element bound 10 * 2^-24 * max(1, |dst|) = {worst:.3f}")
    parity_log(name, got.double(), torch.from_numpy(ref), float(bound.min()) / max(float(np.abs(ref).max()), 1e-30))
    assert (err <= bound).all(), (name, float(err.max()), worst)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("tag", list(SETS))
def test_windows_without_resize_are_bit_exact(vpx, parity_log, kind, tag):
    n_frames, step, five, one = SETS[tag]
    clips = _clips(kind)
    span = (n_frames - 1) * step + 1
    assert any(s + span == LENGTHS[c] for c, s in five) and (2, 0) in five and len(set(five)) == 4 and one[0][1] + span == LENGTHS[2]
    boxes5, flips5 = [(0, 0), (3, 4), (1, 2), (3, 0), (0, 4)], [0, 1, 2, 3, 0]
    cases = [("identity", {}, None, None),
             ("crop", dict(crop_size=(6, 6)), boxes5, None),                                       # (3, 4): touches the bottom-right corner
             ("hflip_vflip", {}, None, flips5),
             ("crop_flips", dict(crop_size=(6, 6)), boxes5, flips5),
             ("range_11", dict(value_range=(-1.0, 1.0)), None, flips5)]
    if KINDS[kind][1] == 1:
        cases.append(("gray_to_3", dict(c_out=3), None, None))
        cases.append(("gray_to_3_crop_flips_11", dict(c_out=3, crop_size=(6, 6), value_range=(-1.0, 1.0)), boxes5, flips5))
    for name, kw, boxes, flips in cases:
        rows = C.table(five, boxes, flips)
        got = _run(vpx, clips, rows, n_frames, seq_step=step, **kw)
        _exact(parity_log, f"{kind}_{tag}_{name}_B5", got, C.preprocess(clips, rows, n_frames, step, **kw))
        rows = C.table(one, boxes and boxes[1:2], flips and flips[3:4])
        _exact(parity_log, f"{kind}_{tag}_{name}_B1", _run(vpx, clips, rows, n_frames, seq_step=step, **kw), C.preprocess(clips, rows, n_frames, step, **kw))
    got = _run(vpx, clips, C.table(five), n_frames, seq_step=step)
    assert torch.equal(got[0], got[4]) and not torch.equal(got[0], got[1])                        # the repeated row; different windows differ


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("out_hw", [(11, 7), (3, 4)])
def test_windows_with_resize_hold_the_frames_bound(vpx, parity_log, kind, out_hw):
    clips = _clips(kind, seed=1)
    for tag, (n_frames, step, five, one) in SETS.items():
        for vr in ((0.0, 1.0), (-1.0, 1.0)):
            rows = C.table(five, [(0, 0), (3, 4), (1, 2), (3, 0), (0, 4)], [0, 1, 2, 3, 0])
            kw = dict(crop_size=(6, 6), out_size=out_hw, value_range=vr, c_out=3 if KINDS[kind][1] == 1 else None)
            got = _run(vpx, clips, rows, n_frames, seq_step=step, **kw)
            assert tuple(got.shape) == (5, n_frames, 3) + out_hw
            _bounded(parity_log, f"{kind}_{tag}_to_{out_hw[0]}x{out_hw[1]}_{vr[0]:g}", got, C.preprocess(clips, rows, n_frames, step, **kw))
    rows = C.table(SETS["4x1"][3], [(3, 4)], [3])
    _bounded(parity_log, f"{kind}_B1_to_{out_hw[0]}x{out_hw[1]}", _run(vpx, clips, rows, 4, crop_size=(6, 6), out_size=out_hw),
             C.preprocess(clips, rows, 4, 1, crop_size=(6, 6), out_size=out_hw))


@pytest.mark.parametrize("kind", list(KINDS))
def test_equal_clips_from_frame_zero_equal_the_stored_sequence_launch(vpx, kind):
    clips = _clips(kind, lengths=(6, 6, 6), seed=2)
    src = torch.from_numpy(np.stack(clips)).cuda()                                                # [3, 6, 9, 10(, 3)]
    seqs, boxes, flips = [2, 0, 1, 2], [(0, 0), (3, 4), (1, 2), (3, 0)], [0, 1, 2, 3]
    for n_frames, step in ((4, 1), (3, 2), (6, 1)):
        for kw in ({}, dict(crop_size=(6, 6)), dict(crop_size=(6, 6), out_size=(11, 7), value_range=(-1.0, 1.0)), dict(crop_size=(6, 6), out_size=(3, 4))):
            use_boxes = boxes if kw else None
            want = vpx.ops.frames_preprocess(src, R.table(seqs, use_boxes, flips), n_frames, seq_step=step, **kw)
            got = _run(vpx, clips, C.table([(s, 0) for s in seqs], use_boxes, flips), n_frames, seq_step=step, **kw)
            assert got.shape == want.shape and torch.equal(got, want), (kind, n_frames, step, kw)


def test_refusals_come_before_any_launch(vpx):
    clips = _clips("u8_rgb")
    src = torch.from_numpy(np.concatenate(clips)).cuda()
    first = C.clip_first(LENGTHS)
    for rows, n_frames, kw, word in ((C.table([(0, 4)]), 4, {}, "leaves its clip"), (C.table([(2, 1)]), 3, dict(seq_step=2), "leaves its clip"),
                                     (C.table([(3, 0)]), 4, {}, "clip index"), (C.table([(0, 0)], [(4, 0)]), 4, dict(crop_size=(6, 6)), "crop box"),
                                     (C.table([(0, 0)], flips=[4]), 4, {}, "flip bits"), (C.table([(0, 0)]), 0, {}, ">= 1"),
                                     (C.table([(0, 0)]), 4, dict(c_out=2), "output channels"), (C.table([(0, 0)]), 4, dict(value_range=(1.0, 1.0)), "empty value range")):
        with pytest.raises(ValueError, match=word):
            vpx.ops.clips_preprocess(src, first, rows, n_frames, **kw)
    with pytest.raises(ValueError, match="src holds 24 frames"):
        vpx.ops.clips_preprocess(src, C.clip_first((7, 12)), C.table([(0, 0)]), 4)
    with pytest.raises(ValueError, match="unknown"):
        vpx.ops.clips_preprocess(src.to(torch.int32), first, C.table([(0, 0)]), 4)
    with pytest.raises(ValueError, match="out must be"):
        vpx.ops.clips_preprocess(src, first, C.table([(0, 0)]), 4, out=torch.empty((1, 4, 3, 9, 9), device="cuda"))
    out = torch.empty((1, 4, 3, 9, 10), device="cuda")
    assert vpx.ops.clips_preprocess(src, first, C.table([(0, 0)]), 4, out=out) is out


@pytest.mark.parametrize("out_hw", [(6, 6), (11, 7)], ids=["copy", "resize"])
def test_unchecked_rows_yield_zeros(vpx, out_hw):
    """Rows that the host check refuses, handed to vpx_frames_preprocess and vpx_clips_preprocess as device tables (ops always checks a
    host table, so the calls go through the library): every pointer and size of the call is valid, the kernel reads nothing for such a
    row and writes zeros, and the rows beside it are computed. The suite's guard bands around `src` and `out` are checked after the test."""
    L, lib, ops = vpx._lib, vpx._lib.lib(), vpx.ops
    stream = torch.cuda.current_stream().cuda_stream
    corners = [(4, 0), (0, 5), (-1, 0)]                                                            # below, right of, above the 9 x 10 frame

    def launch(fn, name, src, args, rows):
        out = torch.full((len(rows), 4, 3) + out_hw, 7.0, device="cuda")
        dev = torch.tensor(rows, dtype=torch.int32).cuda()
        L.check(fn(L.ptr(src), L.FRAMES_U8, *args, L.ptr(dev), len(rows), 4, 1, 6, 6, *out_hw, 3, 0.0, 1.0, L.ptr(out), stream), name)
        return out

    def judge(got, want, n_bad):
        assert want.abs().sum() > 0 and torch.equal(got[0], want[0]) and torch.equal(got[-1], want[0]) and len(got) == n_bad + 2
        for k in range(1, n_bad + 1):
            assert not got[k].any(), k

    # stored sequences
    seqs = torch.from_numpy(np.stack(_clips("u8_rgb", lengths=(6, 6, 6), seed=2))).cuda()         # [3, 6, 9, 10, 3]
    good = (2, 3, 4, 3)
    bad = [(3, 0, 0, 0), (-1, 0, 0, 0)] + [(0, y, x, 0) for y, x in corners]
    for row in bad:
        with pytest.raises(ValueError):
            ops.check_frames_table(np.array([row]), 3, (9, 10), (6, 6))
    want = ops.frames_preprocess(seqs, np.array([good]), 4, crop_size=(6, 6), out_size=out_hw)
    judge(launch(lib.vpx_frames_preprocess, "vpx_frames_preprocess", seqs, (3, 6, 9, 10, 3), [good] + bad + [good]), want, len(bad))
    # clips back to back
    src = torch.from_numpy(np.concatenate(_clips("u8_rgb"))).cuda()                               # [24, 9, 10, 3]
    first = C.clip_first(LENGTHS)
    good = (1, 8, 3, 4, 3, 0)
    bad = [(3, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (0, 4, 0, 0, 0, 0), (1, -1, 0, 0, 0, 0)] + [(0, 0, y, x, 0, 0) for y, x in corners]
    for row in bad:
        with pytest.raises(ValueError):
            ops.check_clips_table(np.array([row]), first, 4, 1, (9, 10), (6, 6))
    want = ops.clips_preprocess(src, first, np.array([good]), 4, crop_size=(6, 6), out_size=out_hw)
    dev_first = torch.from_numpy(first).cuda()
    judge(launch(lib.vpx_clips_preprocess, "vpx_clips_preprocess", src, (24, 9, 10, 3, L.ptr(dev_first), 3), [good] + bad + [good]), want, len(bad))
    # an offset table whose last clip leaves src: that clip's row yields zeros, the other clips' rows are computed
    late = torch.tensor([0, 7, 19, 25], dtype=torch.int64).cuda()
    got = launch(lib.vpx_clips_preprocess, "vpx_clips_preprocess", src, (24, 9, 10, 3, L.ptr(late), 3), [good, (2, 0, 0, 0, 0, 0), good])
    judge(got, want, 1)


def test_a_clip_beyond_two_to_the_31_bytes(vpx, parity_log):
    """64-bit frame offsets: a 12-frame clip at the end of a buffer of 8 150 000 uint8 RGB frames of 9 x 10 (2.2 GB, allocated but only
    written at the two clips that are read); its first byte lies at 2 200 496 760 > 2^31. A 32-bit offset would read the unwritten
    middle (or fault), and cannot return these values."""
    clips = _clips("u8_rgb", lengths=(7, 12), seed=3)
    total, frame = 8_150_000, 9 * 10 * 3
    buf = torch.empty(total * frame, dtype=torch.uint8, device="cuda")
    src = buf.view(total, 9, 10, 3)
    src[:7].copy_(torch.from_numpy(clips[0]))
    src[total - 12:].copy_(torch.from_numpy(clips[1]))
    first = np.array([0, 7, total - 12, total], dtype=np.int64)
    assert int(first[2]) * frame > 2 ** 31 and src.data_ptr() == buf.data_ptr()
    rows = C.table([(2, 8), (0, 3), (2, 0)], [(0, 0), (1, 2), (3, 4)], [0, 3, 1])
    got = vpx.ops.clips_preprocess(src, first, rows, 4, crop_size=(6, 6))
    filler = np.zeros((1, 9, 10, 3), dtype=np.uint8)                                              # never indexed by these rows
    _exact(parity_log, "beyond_2^31_bytes", got, C.preprocess([clips[0], filler, clips[1]], rows, 4, 1, crop_size=(6, 6)))
    rows = C.table([(2, 7)], [(1, 2)], [2])                                                       # frames 7, 9 and 11: ends on the buffer's last frame
    got = vpx.ops.clips_preprocess(src, first, rows, 3, seq_step=2, crop_size=(6, 6), out_size=(3, 4))
    _bounded(parity_log, "beyond_2^31_bytes_resize", got, C.preprocess([clips[0], filler, clips[1]], rows, 3, 2, crop_size=(6, 6), out_size=(3, 4)))


AUGS = [("hflip", 0.5), ("invert", 0.5), ("vflip", 0.5), ("color_jitter", 0.3, 0.2, 0.3, 0.05), ("erase", 1.0, (0.05, 0.3), (0.5, 2.0), (0.0, 0.5, 1.0))]


def test_dataset_batches_and_pinned_storage_equal_device_storage(vpx, parity_log):
    clips = _clips("u8_rgb", seed=4)
    made = {}
    for storage in ("device", "pinned"):
        ds = vpx.datasets.ClipVPDataset("train", clips=clips, storage=storage, crop=("random", 6, 7), img_size=(8, 5), augmentations=AUGS, transform_seed=7,
                                        value_range_min=-1.0)
        ds.set_seq_len(2, 1, 2)
        assert ds.windows == [(0, 0), (1, 0), (1, 6), (2, 0)]
        made[storage] = (ds, ds.batch([3, 0, 2, 2]), ds.batch([1]), ds[2])
    dev, pin = made["device"], made["pinned"]
    assert pin[0]._stored().is_pinned() and not pin[0]._stored().is_cuda and dev[0]._stored().is_cuda
    assert tuple(pin[0]._staging.buffer.shape) == (4, 5, 9, 10, 3)                                # seq_len frames per window, nothing else, crossed
    for a, b in zip(dev[1:], pin[1:]):
        assert a["frames"].is_cuda and a["frames"].dtype == torch.float32 and torch.equal(a["frames"], b["frames"]) and a["origin"] == b["origin"]
        assert torch.equal(a["actions"], b["actions"]) and not a["actions"].any()
    assert tuple(dev[1]["frames"].shape) == (4, 3, 3, 8, 5) and tuple(dev[1]["actions"].shape) == (4, 3, 1) and tuple(dev[3]["frames"].shape) == (3, 3, 8, 5)
    assert dev[1]["origin"][0] == "stored clip 2, start frame: 0" and not torch.equal(dev[1]["frames"][2], dev[1]["frames"][3])   # one draw per window
    # without photometric entries the batch is the restatement of its own table, bit for bit (a crop, both flips, no resize)
    ds = vpx.datasets.ClipVPDataset("train", clips=clips, crop=("random", 6, 7), augmentations=[("hflip", 0.5), ("vflip", 0.5)], transform_seed=7)
    ds.set_seq_len(2, 2, 1)
    windows = [ds.windows[i] for i in (4, 1, 3)]
    assert windows == [(2, 0), (1, 0), (1, 8)]
    table, _ = ds.clips_table(windows)
    ds.reset_rng()
    got = ds.batch([4, 1, 3])["frames"]
    _exact(parity_log, "dataset_batch", got, C.preprocess(clips, table, 4, 1, crop_size=(6, 7)))
    ds.reset_rng()
    singles = torch.stack([ds[i]["frames"] for i in (4, 1, 3)])
    assert torch.equal(singles, got)


def test_workbench_trains_and_tests_on_an_exported_kitti_tree(vpx, tmp_path):
    import golden_cases as gc
    tiny = {k: v for k, v in gc.EF_TINY3_KW.items() if k not in ("img_shape", "action_size", "tensor_value_range")}
    X.export("kitti", str(tmp_path / "data"), X.kitti_names(7), [7, 12, 5, 23, 9, 31, 16], (16, 24), seed=1)
    suite = vpx.VPSuite()
    suite.load_dataset("KITTI", data_dir=str(tmp_path / "data"))
    train = suite.training_sets[-1]
    assert type(train.train_data) is vpx.datasets.KITTIRawDataset and train.img_shape == (3, 16, 24) and train.val_data is not train.train_data
    suite.create_model("convlstm-shi", **tiny)
    run = dict(context_frames=3, pred_frames=2, seq_step=1)
    loss = suite.train(epochs=1, batch_size=2, out_dir=str(tmp_path / "run"), **run)
    assert np.isfinite(loss) and len(train.train_data) == 10 and len(train.val_data) == 1           # windows of 5 frames every 5 frames
    suite.load_dataset("KITTI", split="test", data_dir=str(tmp_path / "data"))
    assert len(suite.test_sets[-1].test_data.sequences) == 2
    results = suite.test(**run)
    (models,) = results.values()
    assert len(models) >= 1
    for name, rows in models.items():
        assert len(rows) >= 1 and all(np.isfinite(v) for row in rows for v in row.values()), (name, rows)
