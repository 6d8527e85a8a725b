"""vpx_clips_preprocess_var and vpx_actions_diff_gather on the GPU: windows of clips of mixed frame sizes to batches, and the position
differences that go with them, against the restatement (tests/video_ref.py: the clip sliced, then the stored-frame arithmetic of
tests/frames_ref.py with the row's own box) run in the test.

The shapes are the smallest at which the launches can go wrong: clips of 7, 12 and 5 frames of 6 x 10, 7 x 9 and 9 x 6 pixels (different
row strides and frame sizes, so a wrong per-clip offset or stride shows), boxes of 4 x 5 (ow % 4 = 1: element stores, a partial last
group) and outputs of 5 x 7 and 8 x 12 (ow % 4 = 0: vector stores).

EXACT cases (equality): a box of the output's size is copied; a value is one float32 division and, for a range other than (0, 1), one
multiply and one add. The action rows are one subtraction in the stored precision and one rounding.
BOUNDED cases (resize): |kernel - float64 restatement| <= 10 * 2^-24 * max(1, |dst|) per element, the bar of the stored-sequence launch
(tests/test_gpu_frames.py derives it); the per-pixel device code is the same function.
CONSISTENCY: with equal shapes the launch equals vpx_clips_preprocess bit for bit, resize and flips included."""
import os
import sys

import numpy as np
import pytest
import torch

import clips_ref as C
import video_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_video_like as X  # noqa: E402

LENGTHS, SIZES = (7, 12, 5), ((6, 10), (7, 9), (9, 6))
KINDS = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
# (n_frames, seq_step, windows of B = 5, window of B = 1): windows ending on the last frame of clips 0 and 1, starting at frame 0 of the
# clip after the longer one, a repeated row; the single window ends on the last frame of the 5-frame clip
SETS = {"4x1": (4, 1, [(0, 3), (2, 0), (1, 8), (1, 0), (0, 3)], [(2, 1)]),
        "2x3": (2, 3, [(0, 3), (2, 0), (1, 8), (1, 1), (0, 3)], [(2, 1)])}


def _clips(kind, channels, lengths=LENGTHS, sizes=SIZES, seed=0):
    dtype = KINDS[kind]
    rng = np.random.default_rng([seed, channels, len(kind)])
    shapes = [(n,) + hw + ((channels,) if channels > 1 else ()) for n, hw in zip(lengths, sizes)]
    if dtype == np.float32:
        return [rng.uniform(-0.25, 1.25, size=s).astype(np.float32) for s in shapes]
    clips = [rng.integers(0, np.iinfo(dtype).max + 1, size=s).astype(dtype) for s in shapes]
    clips[0].reshape(-1)[:2] = (0, np.iinfo(dtype).max)
    return clips


def _run(vpx, clips, rows, n_frames, seq_step, out_size, **kw):
    buf, geom = V.flat(clips)
    channels = clips[0].shape[3] if clips[0].ndim == 4 else 1
    return vpx.ops.clips_preprocess_var(torch.from_numpy(buf).cuda(), geom, rows, n_frames, seq_step, out_size, channels, **kw)


def _exact(parity_log, name, got, ref):
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == ref.shape, (got.shape, ref.shape)
    want = torch.from_numpy(ref.astype(np.float32))
    assert np.array_equal(want.numpy().astype(np.float64), ref)                                   # the reference itself is float32 values
    parity_log(name, got.float(), want, 0.0)
    assert torch.equal(got.cpu(), want), f"{name}: {int((got.cpu() != want).sum())} of {want.numel()} values differ"


def _bounded(parity_log, name, got, ref):
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == ref.shape and ref.dtype == np.float64
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    bound = 10.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))
    worst = float((err / bound).max())
    print(f"{name}: max |kernel - restatement| = {err.max():.3e}, worst share of the per-element bound 10 * 2^-24 * max(1, |dst|) = {worst:.3f}")
    parity_log(name, got.double(), torch.from_numpy(ref), float(bound.min()) / max(float(np.abs(ref).max()), 1e-30))
    assert (err <= bound).all(), (name, float(err.max()), worst)


@pytest.mark.parametrize("kind", ["u8_rgb", "u16_gray", "f32_gray"])
def test_equal_shapes_equal_the_clips_launch_bit_for_bit(vpx, kind):
    dtype, channels = {"u8_rgb": ("u8", 3), "u16_gray": ("u16", 1), "f32_gray": ("f32", 1)}[kind]
    clips = _clips(dtype, channels, lengths=(7, 3, 5, 4), sizes=((6, 10),) * 4, seed=2)
    src = torch.from_numpy(np.concatenate(clips)).cuda()
    first = C.clip_first([7, 3, 5, 4])
    wins, corners, flips = [(0, 3), (1, 0), (2, 1), (3, 0), (0, 0)], [(0, 0), (1, 3), (2, 2), (0, 5), (1, 1)], [0, 1, 2, 3, 0]
    if kind == "u8_rgb":
        assert [c.shape for c in clips] == [(7, 6, 10, 3), (3, 6, 10, 3), (5, 6, 10, 3), (4, 6, 10, 3)]
    for n_frames, step in ((3, 1), (2, 2)):
        for box, out_hw in (((6, 10), None), ((6, 10), (5, 7)), ((4, 5), None), ((4, 5), (5, 7))):
            for use_flips in (None, flips):
                use = corners if box != (6, 10) else [(0, 0)] * 5
                kw = dict(value_range=(-1.0, 1.0)) if use_flips else {}
                want = vpx.ops.clips_preprocess(src, first, C.table(wins, use, use_flips), n_frames, step, box, out_hw, **kw)
                rows = V.table(wins, [(y, x) + box for y, x in use], use_flips)
                got = _run(vpx, clips, rows, n_frames, step, out_hw or box, **kw)
                assert got.shape == want.shape and torch.equal(got, want), (kind, n_frames, step, box, out_hw, use_flips)


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("kind", list(KINDS))
def test_mixed_shapes_without_resize_are_bit_exact(vpx, parity_log, kind, channels):
    clips = _clips(kind, channels)
    center = {c: (V.R.center_offset(h, 4), V.R.center_offset(w, 5)) for c, (h, w) in enumerate(SIZES)}
    rng = np.random.default_rng(5)
    for tag, (n_frames, step, five, one) in SETS.items():
        span = (n_frames - 1) * step + 1
        assert any(s + span == LENGTHS[c] for c, s in five) and len(set(five)) == 4 and one[0][1] + span == LENGTHS[2]
        for crop in ("center", "random"):
            def boxes(wins):
                return [(center[c] if crop == "center" else (int(rng.integers(0, SIZES[c][0] - 3)), int(rng.integers(0, SIZES[c][1] - 4)))) + (4, 5) for c, _ in wins]
            for wins, flips in ((five, [0, 1, 2, 3, 0]), (one, [3])):
                b = boxes(wins)
                if len(wins) == 5:
                    b[4] = b[0]                                                                    # the repeated window, box and all
                for kw in ({}, dict(value_range=(-1.0, 1.0)), *([dict(c_out=3)] if channels == 1 else [])):
                    rows = V.table(wins, b, flips)
                    got = _run(vpx, clips, rows, n_frames, step, (4, 5), **kw)
                    assert got.shape[2] == kw.get("c_out", channels)
                    _exact(parity_log, f"{kind}_c{channels}_{tag}_{crop}_B{len(wins)}_{'_'.join(kw) or 'plain'}", got, V.preprocess(clips, rows, n_frames, step, (4, 5), **kw))
                    if len(wins) == 5:
                        assert torch.equal(got[0], got[4]) and not torch.equal(got[0], got[1])
    # the far corner of every clip's own frame: a wrong row stride or frame size reads the neighbour
    wins = [(0, 3), (1, 8), (2, 1)]
    rows = V.table(wins, [(h - 4, w - 5, 4, 5) for h, w in SIZES])
    _exact(parity_log, f"{kind}_c{channels}_far_corners", _run(vpx, clips, rows, 4, 1, (4, 5)), V.preprocess(clips, rows, 4, 1, (4, 5)))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("out_hw", [(5, 7), (8, 12)])
def test_mixed_shapes_with_resize_hold_the_frames_bound(vpx, parity_log, kind, out_hw):
    clips = _clips(kind, 3, lengths=(7, 12, 5), sizes=((6, 10), (7, 9), (1, 1)), seed=1)
    wins = [(0, 3), (2, 0), (1, 8), (1, 0), (2, 1)]
    for vr in ((0.0, 1.0), (-1.0, 1.0)):
        rows = V.table(wins, V.whole(clips, wins), [0, 1, 2, 3, 0])                               # whole frames: up and down in one batch
        got = _run(vpx, clips, rows, 4, 1, out_hw, value_range=vr)
        assert tuple(got.shape) == (5, 4, 3) + out_hw
        _bounded(parity_log, f"{kind}_whole_to_{out_hw[0]}x{out_hw[1]}_{vr[0]:g}", got, V.preprocess(clips, rows, 4, 1, out_hw, value_range=vr))
    wins = [(0, 0), (1, 5), (1, 2), (0, 2)]
    rows = V.table(wins, [(2, 9, 4, 1), (6, 1, 1, 7), (3, 4, 1, 1), (0, 0, 5, 7)], [1, 2, 3, 0])  # width 1 (last column), height 1 (last row), one pixel, the output's size
    got = _run(vpx, clips, rows, 2, 3, (5, 7))
    ref = V.preprocess(clips, rows, 2, 3, (5, 7))
    _bounded(parity_log, f"{kind}_thin_boxes", got, ref)
    assert np.array_equal(got[3].cpu().numpy().astype(np.float64), ref[3])                        # the box of the output's size is copied: exact


def test_unchecked_rows_yield_zeros(vpx):
    """Rows and clip geometry that the host check refuses, handed over as device tables (which the launch cannot check on the host):
    every pointer and size of the call is valid, the kernel reads nothing for such a row and writes zeros, and the rows beside it are
    computed. The suite's guard bands around `src` and `out` are checked after the test."""
    clips = _clips("u8", 3)
    buf, geom = V.flat(clips)
    src = torch.from_numpy(buf).cuda()
    good = (1, 8, 2, 3, 4, 5, 3, 0)
    bad_rows = {"clip index": (3, 0, 0, 0, 4, 5, 0, 0), "negative clip": (-1, 0, 0, 0, 4, 5, 0, 0), "window leaves its clip": (0, 4, 0, 0, 4, 5, 0, 0),
                "negative start": (1, -1, 0, 0, 4, 5, 0, 0), "box below": (0, 0, 3, 0, 4, 5, 0, 0), "box right": (2, 0, 0, 2, 4, 5, 0, 0),
                "negative corner": (0, 0, -1, 0, 4, 5, 0, 0), "empty box": (0, 0, 0, 0, 0, 5, 0, 0), "huge box": (0, 0, 0, 0, 2 ** 30, 5, 0, 0)}
    rows = np.array([good] + list(bad_rows.values()) + [good], dtype=np.int32)
    for name, row in bad_rows.items():
        with pytest.raises(ValueError):
            vpx.ops.check_clips_var_table(np.array([row]), geom, buf.size, 3, 4, 1)
    want = _run(vpx, clips, np.array([good], dtype=np.int32), 4, 1, (4, 5))
    got = vpx.ops.clips_preprocess_var(src, torch.from_numpy(geom).cuda(), torch.from_numpy(rows).cuda(), 4, 1, (4, 5), 3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[-1], want[0]) and want.abs().sum() > 0
    for k, name in enumerate(bad_rows, start=1):
        assert not got[k].any(), name
    # with a resize the same
    got = vpx.ops.clips_preprocess_var(src, torch.from_numpy(geom).cuda(), torch.from_numpy(rows).cuda(), 4, 1, (8, 12), 3)
    assert got[0].abs().sum() > 0 and not got[1:-1].any()
    # a clip that leaves src (or is not a clip at all): its rows yield zeros, the other clips' rows are computed
    rows = torch.from_numpy(V.table([(0, 0), (1, 0), (2, 0)], [(0, 0, 4, 5)] * 3)).cuda()
    for clip, col, value in ((2, 1, 6), (2, 0, buf.size), (1, 0, -1), (1, 1, 0), (1, 2, 2 ** 40), (0, 3, 0), (0, 1, 2 ** 62)):
        bad = geom.copy()
        bad[clip, col] = value
        if (clip, col) == (2, 1):                                                                 # 6 frames of 9 x 6 x 3 from the last clip's offset: 162 elements past the end
            with pytest.raises(ValueError, match="a clip leaves"):
                vpx.ops.check_clips_var_table(rows.cpu(), bad, buf.size, 3, 4, 1)
        got = vpx.ops.clips_preprocess_var(src, torch.from_numpy(bad).cuda(), rows, 4, 1, (4, 5), 3)
        for k in range(3):
            assert bool(got[k].any()) == (k != clip), (clip, col, value, k)
    # the action rows: the same convention
    pos = torch.from_numpy(np.random.default_rng(0).normal(size=(24, 3))).cuda()
    first = torch.from_numpy(C.clip_first(LENGTHS)).cuda()
    rows = torch.tensor([[1, 8, 0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0], [0, 4, 0, 0, 0, 0, 0, 0], [2, -1, 0, 0, 0, 0, 0, 0]], dtype=torch.int32).cuda()
    got = vpx.ops.actions_diff_gather(pos, first, rows, 4, 1)
    assert got[0].any() and not got[1:].any()
    bad_first = torch.tensor([0, 7, 19, 25], dtype=torch.int64).cuda()                           # the last clip leaves src
    got = vpx.ops.actions_diff_gather(pos, bad_first, torch.tensor([[2, 1, 0, 0, 0, 0, 0, 0], [1, 8, 0, 0, 0, 0, 0, 0]], dtype=torch.int32).cuda(), 4, 1)
    assert not got[0].any() and got[1].any()


def test_a_clip_beyond_two_to_the_31_elements(vpx, parity_log):
    """64-bit element offsets: the size and the time of the clips test of this kind (a 2.2 GB uint8 buffer, allocated but written only at
    the two clips that are read). The second clip, 12 frames of 7 x 9 RGB, ends the buffer; its first element lies at 2 200 497 732 >
    2^31. A 32-bit offset would read the unwritten middle (or fault), and cannot return these values."""
    clips = _clips("u8", 3, lengths=(7, 12), sizes=((6, 10), (7, 9)), seed=3)
    total = 8_150_000 * 270
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf[:clips[0].size].copy_(torch.from_numpy(clips[0].reshape(-1)))
    buf[total - clips[1].size:].copy_(torch.from_numpy(clips[1].reshape(-1)))
    geom = np.array([[0, 7, 6, 10], [total - clips[1].size, 12, 7, 9]], dtype=np.int64)
    assert int(geom[1, 0]) > 2 ** 31
    rows = V.table([(1, 8), (0, 3), (1, 0)], [(3, 4, 4, 5), (1, 2, 4, 5), (0, 0, 4, 5)], [0, 3, 1])  # one window from each side, one ending on the buffer's last frame
    got = vpx.ops.clips_preprocess_var(buf, geom, rows, 4, 1, (4, 5), 3)
    _exact(parity_log, "beyond_2^31_elements", got, V.preprocess(clips, rows, 4, 1, (4, 5)))
    rows = V.table([(1, 7), (0, 2)], [(0, 0, 7, 9), (0, 0, 6, 10)], [2, 1])
    got = vpx.ops.clips_preprocess_var(buf, geom, rows, 3, 2, (5, 7), 3)
    _bounded(parity_log, "beyond_2^31_elements_resize", got, V.preprocess(clips, rows, 3, 2, (5, 7)))


AUGS = [("hflip", 0.5), ("invert", 0.5), ("vflip", 0.5), ("color_jitter", 0.3, 0.2, 0.3, 0.05), ("erase", 1.0, (0.05, 0.3), (0.5, 2.0), (0.0, 0.5, 1.0))]


def test_mixed_dataset_pinned_storage_equals_device_storage(vpx, parity_log):
    clips = _clips("u8", 3, seed=4)
    pos = [np.random.default_rng(k).normal(size=(n, 3)) * 5 for k, n in enumerate(LENGTHS)]
    made = {}
    for storage in ("device", "pinned"):
        ds = vpx.datasets.ClipVPDataset("train", clips=clips, positions=pos, storage=storage, crop=("random", 4, 5), img_size=(8, 5), augmentations=AUGS,
                                        transform_seed=7, value_range_min=-1.0)
        ds.set_seq_len(2, 1, 2)
        assert ds.windows == [(0, 0), (1, 0), (1, 6), (2, 0)] and ds.mixed_shapes
        made[storage] = (ds, ds.batch([3, 0, 2, 2]), ds.batch([1]), ds[2])
    dev, pin = made["device"], made["pinned"]
    assert pin[0]._stored().is_pinned() and not pin[0]._stored().is_cuda and dev[0]._stored().is_cuda and dev[0]._stored().ndim == 1
    assert pin[0]._flat_staging.buffer.numel() == 5 * 3 * (9 * 6 + 6 * 10 + 7 * 9 + 7 * 9)          # seq_len frames per window, each of its own size, nothing else
    for a, b in zip(dev[1:], pin[1:]):
        assert a["frames"].is_cuda and a["frames"].dtype == torch.float32 and torch.equal(a["frames"], b["frames"]) and a["origin"] == b["origin"]
        assert torch.equal(a["actions"], b["actions"]) and a["actions"].any()
    assert tuple(dev[1]["frames"].shape) == (4, 3, 3, 8, 5) and tuple(dev[1]["actions"].shape) == (4, 2, 3) and tuple(dev[3]["actions"].shape) == (2, 3)
    assert not torch.equal(dev[1]["frames"][2], dev[1]["frames"][3])                               # one draw per window
    want = np.stack([V.action_diffs(pos[c], s, 3, 2) for c, s in [(2, 0), (0, 0), (1, 6), (1, 6)]])
    assert np.array_equal(dev[1]["actions"].cpu().numpy(), want)
    # without photometric entries the batch is the restatement of its own table
    ds = vpx.datasets.ClipVPDataset("train", clips=clips, crop=("random", 4, 5), img_size=(4, 5), augmentations=[("hflip", 0.5), ("vflip", 0.5)], transform_seed=7)
    ds.set_seq_len(2, 2, 1)
    windows = [ds.windows[i] for i in (4, 1, 3)]
    table, _ = ds.clips_var_table(windows)
    ds.reset_rng()
    got = ds.batch([4, 1, 3])
    _exact(parity_log, "mixed_dataset_batch", got["frames"], V.preprocess(clips, table, 4, 1, (4, 5)))
    assert tuple(got["actions"].shape) == (3, 4, 1) and not got["actions"].any()                   # no positions: the reference's zeros


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_action_differences_are_bit_exact(vpx, dtype):
    rng = np.random.default_rng(9)
    lengths = (30, 41)
    first = C.clip_first(lengths)
    for A in (1, 3, 7):
        # near 1e7 with steps of about 1e-3: float32 cannot hold the positions (its spacing there is 1), only their differences
        pos = [(1e7 + np.cumsum(rng.normal(0.0, 1e-3, size=(n, A)), axis=0)).astype(np.float64) for n in lengths]
        pos = [p.astype(dtype) for p in pos] if dtype == np.float32 else pos
        if dtype == np.float32:
            pos = [p + rng.normal(0.0, 3.0, size=p.shape).astype(np.float32) for p in pos]         # (float32 storage: differences of representable values)
        src = torch.from_numpy(np.concatenate(pos)).cuda()
        for n_frames, step in ((2, 1), (9, 1), (2, 3), (9, 3)):
            span = (n_frames - 1) * step + 1
            for B in (1, 130):
                wins = [(1, lengths[1] - span)] if B == 1 else [(k % 2, int(rng.integers(0, lengths[k % 2] - span + 1))) for k in range(B)]
                wins[-1] = (1, lengths[1] - span)                                                  # ends on the last stored row
                wins[0] = (0, lengths[0] - span) if B > 1 else wins[0]                             # ends on the first clip's last row
                rows = np.zeros((B, 8), dtype=np.int32)
                rows[:, :2] = wins
                got = vpx.ops.actions_diff_gather(src, first, rows, n_frames, step)
                want = np.stack([V.action_diffs(pos[c], s, n_frames, step) for c, s in wins])
                assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, n_frames - 1, A)
                assert np.array_equal(got.cpu().numpy(), want), (A, n_frames, step, B)
                if dtype == np.float64:                                                            # rounding the difference is not differencing the roundings
                    other = np.stack([V.diffs_of_roundings(pos[c], s, n_frames, step) for c, s in wins])
                    assert not np.array_equal(other, want) and np.abs(want).max() < 0.1 and np.abs(want).max() > 0
    with pytest.raises(ValueError, match=">= 2"):
        vpx.ops.actions_diff_gather(src, first, np.zeros((1, 8), dtype=np.int32), 1, 1)
    for rows, word in (([[2, 0]], "clip index"), ([[0, 22]], "leaves its clip"), ([[1, -1]], "leaves its clip")):
        with pytest.raises(ValueError, match=word):
            vpx.ops.actions_diff_gather(src, first, np.array(rows), 9, 1)
    with pytest.raises(ValueError, match="end at the 71 stored rows"):
        vpx.ops.actions_diff_gather(src, C.clip_first((30, 40)), np.zeros((1, 8), dtype=np.int32), 2, 1)


TINY_AC = dict(patch_size=1, num_layers=2, num_hidden=[8, 8], filter_size=5)   # 16 x 16 patches -> 4 x 4 maps after the two stride-2 convolutions
RUN = dict(context_frames=2, pred_frames=2, seq_step=2)


def test_workbench_trains_and_tests_an_action_model_on_an_exported_synpick_tree(vpx, tmp_path, monkeypatch):
    data = str(tmp_path / "data")
    for split, n in (("train", 3), ("val", 1), ("test", 1)):
        X.export("spm", data, X.spm_names(n, split), [100, 96, 90][:n], (12, 20), seed=6)
    suite = vpx.VPSuite()
    suite.load_dataset("SPM", data_dir=data, img_size=(16, 16))
    suite.create_model("predrnn-pp", action_conditional=True, **TINY_AC)
    model = suite.models[-1]
    assert model.action_conditional and model.action_size == 3 and model.img_shape == (3, 16, 16)
    batches, received = [], []
    cls, ds_cls = type(model), vpx.datasets.SynpickMovingDataset
    forward, batch = cls.forward, ds_cls.batch

    def recording_forward(self, x, pred_frames=1, **kwargs):
        acts = kwargs.get("actions")
        received.append(None if acts is None else acts.detach().cpu().numpy().copy())
        return forward(self, x, pred_frames=pred_frames, **kwargs)

    def recording_batch(self, indices):
        batches.append((self, list(indices)))
        return batch(self, indices)

    monkeypatch.setattr(cls, "forward", recording_forward)
    monkeypatch.setattr(ds_cls, "batch", recording_batch)
    best = suite.train(epochs=1, batch_size=2, out_dir=str(tmp_path / "run"), **RUN)
    assert np.isfinite(best)
    train = suite.training_sets[-1].train_data
    assert len(train) >= 2 and all(s >= 72 for _, s in train.windows)
    n_train = len(batches)
    suite.load_dataset("SPM", split="test", data_dir=data, img_size=(16, 16))
    results = suite.test(**RUN)
    monkeypatch.undo()
    (models,) = results.values()
    for name, rows in models.items():
        assert len(rows) >= 1 and all(np.isfinite(v) for row in rows for v in row.values()), (name, rows)
    # every forward call received the t - 1 action rows of the batch drawn just before it, bit for bit: position differences
    assert len(batches) == len(received) > n_train >= 2 and all(r is not None for r in received)
    for (ds, indices), got in zip(batches, received):
        want = np.stack([V.action_diffs(ds.gripper_pos[c], s, 4, 2) for c, s in (ds.windows[i] for i in indices)])
        if got.shape[0] == 2 * len(indices):                                                         # training: the sequence and its reversal as one batch
            want = np.concatenate([want, want])
        assert got.dtype == np.float32 and got.shape == want.shape and want.shape[1:] == (3, 3) and np.array_equal(got, want) and np.abs(want).max() > 0
