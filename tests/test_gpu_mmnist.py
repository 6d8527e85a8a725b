"""csrc/mmnist.hip on the GPU: Moving MNIST batches against the numpy restatement (tests/mmnist_ref.py), run in the test.

Every comparison is BIT-EXACT (torch.equal; the parity record shows 0): each step of the pixel contract is one correctly rounded IEEE
operation in a fixed order — float64 adds of double(g) / 255 in digit order, a clip, * 255, / 255, one conversion to float32, and for
a value range other than (0, 1) a float32 multiply and a float32 add. A difference in the last bit is a contraction or a reordering
in the kernel, not noise."""
import functools
import os

import numpy as np
import pytest
import torch

import mmnist_ref as R
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# (S, glyph s, C, B, (context, pred, seq_step) -> frames, value range, D)
CASES = {
    "16x16_bounces": (16, 7, 1, 3, (5, 4, 1), (0.0, 1.0), 2),        # 9 frames: a workgroup draws a chunk of two, the last chunk holds one
    "18x18_scalar_tail": (18, 5, 3, 2, (3, 3, 1), (-1.0, 1.0), 2),   # S % 4 = 2: element stores, a partial last group per row; scaled range
    "64x64_fixture_shape": (64, 28, 3, 2, (3, 2, 1), (0.0, 1.0), 2),
    "33x33_odd": (33, 12, 1, 1, (6, 6, 1), (0.0, 1.0), 2),           # odd side, 12 frames: six chunks
    "16x16_one_digit": (16, 7, 1, 2, (5, 4, 1), (0.0, 1.0), 1),
    "16x16_three_digits": (16, 7, 1, 2, (5, 4, 1), (0.0, 1.0), 3),
    "16x16_seq_step_2": (16, 7, 1, 2, (3, 2, 2), (0.0, 1.0), 2),     # seq_len = (5 - 1) * 2 + 1 = 9 frames are returned
}
FRAMES = {"16x16_bounces": 9, "18x18_scalar_tail": 6, "64x64_fixture_shape": 5, "33x33_odd": 12, "16x16_one_digit": 9, "16x16_three_digits": 9,
          "16x16_seq_step_2": 9}


@functools.lru_cache(maxsize=None)
def _glyphs(size):
    from vp_suite_amd.datasets import procedural_digits
    return procedural_digits(n=12, size=size)


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN_DIR, "mmnist_otf.npz"))


def _dataset(split, glyphs, S, C, D, value_range, **kw):
    from vp_suite_amd.datasets import DATASET_CLASSES
    return DATASET_CLASSES["MMF"](split, digits=glyphs, img_size=S, num_channels=C, num_digits=D, value_range_min=value_range[0],
                                  value_range_max=value_range[1], **kw)


def _exact(parity_log, name, got, ref):
    ref = torch.from_numpy(ref)
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(ref.shape)
    parity_log(name, got, ref, 0.0)
    assert torch.equal(got.cpu(), ref), f"{name}: {int((got.cpu() != ref).sum())} of {ref.numel()} values differ"


def _turns(p, v, n, S, s):
    count = 0
    for _ in range(n):
        p, w = R.move(p, v, S, s)
        count += w != v
        v = w
    return count


@pytest.mark.parametrize("case", list(CASES))
def test_batches_equal_the_restatement(vpx, parity_log, case):
    S, s, C, B, seq, value_range, D = CASES[case]
    ds = _dataset("val", _glyphs(s), S, C, D, value_range)
    ds.set_seq_len(*seq)
    assert ds.seq_len == FRAMES[case]
    params = R.Sampler("val", 12, s, img_size=S, num_digits=D).params(B)
    if case == "16x16_bounces":   # several bounces per axis within the sequence (shown on the host side)
        assert max(_turns(int(r[1 + ax]), int(r[3 + ax]), 9, S, s) for r in params.reshape(-1, 5) for ax in (0, 1)) >= 2
    data = ds.batch(B)
    _exact(parity_log, case, data["frames"], R.render(_glyphs(s), params, ds.seq_len, C, S, value_range))
    assert tuple(data["actions"].shape) == (B, ds.total_frames, 1) and not data["actions"].any() and len(data["origin"]) == B


def test_overlapping_glyphs_are_clipped(vpx, parity_log):
    """Two glyphs on the same pixels: the sum passes 1 where both strokes are bright and stays below it on their soft edges."""
    from vp_suite_amd.datasets import generate_frames
    S, s, F = 16, 7, 5
    glyphs = _glyphs(s)
    params = np.array([[[8, 3, 2, 2, 3], [0, 3, 2, 2, 3]], [[8, 4, 4, -2, 2], [3, 5, 4, -2, 2]]], dtype=np.int32)
    ref = R.render(glyphs, params, F, 1, S)
    parts = [R.render(glyphs, params[:, d:d + 1], F, 1, S).astype(np.float64) for d in (0, 1)]   # each digit alone: exact in float64
    both = (parts[0] > 0) & (parts[1] > 0)
    total = parts[0] + parts[1]
    assert (both & (total > 1.0) & (ref == 1.0)).any(), "no pixel is clipped to 1"
    assert (both & (total < 1.0) & (ref > np.maximum(parts[0], parts[1]))).any(), "no overlapping pixel stays an unclipped sum"
    for value_range in ((0.0, 1.0), (-1.0, 1.0)):
        got = generate_frames(torch.from_numpy(glyphs).cuda(), params, F, 1, S, value_range)
        _exact(parity_log, f"overlap{value_range}", got, R.render(glyphs, params, F, 1, S, value_range))


def test_walls_and_corners(vpx, parity_log):
    """One glyph per sample walked into each wall and each corner (room = S - s = 9, speed 3 or 0 per axis, 6 frames: into the wall, back
    across the image and off the opposite one)."""
    from vp_suite_amd.datasets import generate_frames
    S, s, F = 16, 7, 6
    starts = {"right": (4, 8, 0, 3), "left": (4, 1, 0, -3), "top": (1, 4, -3, 0), "bottom": (8, 4, 3, 0),
              "bottom_right": (8, 8, 3, 3), "top_left": (1, 1, -3, -3), "top_right": (1, 8, -3, 3), "bottom_left": (8, 1, 3, -3)}
    params = np.array([[[i % 12, *row]] for i, row in enumerate(starts.values())], dtype=np.int32)
    for (y, x, vy, vx) in starts.values():   # every moving axis turns, on the far wall or mirrored off 0; a resting one never does
        assert all(_turns(p, v, F, S, s) >= 1 if v else _turns(p, v, F, S, s) == 0 for p, v in ((y, vy), (x, vx)))
        assert (vy <= 0 or S - s in R.trajectory(y, vy, F, S, s)) and (vx <= 0 or S - s in R.trajectory(x, vx, F, S, s))
    for C in (1, 3):
        got = generate_frames(torch.from_numpy(_glyphs(s)).cuda(), params, F, C, S)
        _exact(parity_log, f"walls_c{C}", got, R.render(_glyphs(s), params, F, C, S))


def test_batch_equals_single_items(vpx, parity_log):
    a, b = (_dataset("train", _glyphs(7), 16, 1, 2, (0.0, 1.0)) for _ in range(2))
    for ds in (a, b):
        ds.set_seq_len(3, 3, 1)
    batch = a.batch(4)["frames"]
    items = [b[i] for i in range(4)]
    assert all(tuple(it["frames"].shape) == (6, 1, 16, 16) and tuple(it["actions"].shape) == (6, 1) and it["origin"] == "generated on-the-fly" for it in items)
    singles = torch.stack([it["frames"] for it in items])
    parity_log("batch_vs_items", batch, singles.cpu(), 0.0)
    assert torch.equal(batch, singles)
    assert not torch.equal(batch[0], batch[1])


@pytest.mark.parametrize("tag,split,kwargs", [("test", "test", {}), ("train", "train", {"value_range_min": -1.0})])
def test_reference_fixture_is_reproduced(vpx, parity_log, tag, split, kwargs):
    """The sequences the upstream class drew (tests/golden/mmnist_otf.npz) from its glyph table and seed, at its defaults (3 x 64 x 64)."""
    from vp_suite_amd.datasets import DATASET_CLASSES
    g = _golden()
    ds = DATASET_CLASSES["MMF"](split, digits=g["glyphs"], **kwargs)
    ds.set_seq_len(3, 2, 1)
    frames = ds.batch(3)["frames"]
    _exact(parity_log, f"fixture_{tag}", frames, np.ascontiguousarray(np.repeat(g[f"frames_{tag}"][:, :, None], 3, axis=2)))


def test_convlstm_trains_on_generated_batches(vpx):
    """End to end: two train_iter steps of convlstm-shi at 1 x 64 x 64 over loader(2); the loss is finite and the parameters move."""
    from vp_suite_amd.datasets import DATASET_CLASSES, procedural_digits
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.models import MODEL_CLASSES
    ds = DATASET_CLASSES["MMF"]("train", digits=procedural_digits(), num_channels=1, n_seqs=4)
    ds.set_seq_len(3, 2, 1)
    cfg = ds.config
    torch.manual_seed(0)
    m = MODEL_CLASSES["convlstm-shi"]("cuda", img_shape=(cfg["img_c"], cfg["img_h"], cfg["img_w"]), action_size=cfg["action_size"],
                                      tensor_value_range=cfg["tensor_value_range"]).to("cuda")
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    run = {"device": "cuda", "context_frames": 3, "pred_frames": 2, "val_rec_criterion": "mse"}
    losses, total_loss = [], m._total_loss

    def recording(*args):   # the loss train_iter itself differentiates, batch by batch
        value = total_loss(*args)
        losses.append(value.detach())
        return value
    m._total_loss = recording
    before = torch.cat([p.detach().flatten().clone() for p in m.parameters()])
    loader = ds.loader(2)
    assert len(loader) == 2
    m.train_iter(run, loader, torch.optim.Adam(m.parameters(), lr=1e-3), lp, epoch=0)
    after = torch.cat([p.detach().flatten() for p in m.parameters()])
    assert len(losses) == 2 and all(bool(torch.isfinite(v)) and float(v) > 0 for v in losses), losses
    assert torch.isfinite(after).all() and (after != before).float().mean() > 0.5
