"""The frame adapter kernel (csrc/adapt.hip, ops.frames_adapt) against the float64 restatement of tests/adapt_ref.py at the sizes where it
can go wrong (adapt_ref.SHAPES), for 1 and 3 channels, 1 and 5 frames, the three range pairs, and 5-D inputs that are the non-contiguous
halves VPModel.unpack_data splits."""
import numpy as np
import pytest
import torch

import adapt_ref

pytestmark = pytest.mark.gpu


def _check(vpx, x, out_hw, src, dst, tag):
    """x: a float32 GPU tensor [..., C, H, W] (any strides). Bound: adapt_ref.bound(dst) for inputs inside the source range."""
    hw = tuple(x.shape[-2:])
    host = x.cpu().numpy()                                             # (dense copy of what the kernel is asked to read)
    before = x.clone()
    got = vpx.ops.frames_adapt(x, None if out_hw == hw else out_hw, src, dst)
    assert got.is_contiguous() and got.dtype == torch.float32 and tuple(got.shape) == tuple(x.shape[:-2]) + out_hw
    assert torch.equal(x, before), f"{tag}: the input was written"
    ref = adapt_ref.adapt(host, out_hw, src, dst)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    bound = adapt_ref.bound(dst)
    print(f"{tag}: max |kernel - restatement| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (tag, err, bound)
    if src == dst and out_hw == hw:
        assert torch.equal(got, x), f"{tag}: equal ranges and sizes must return the input's bits"
    return got


@pytest.mark.parametrize("hw,out_hw", adapt_ref.SHAPES)
def test_adapt_matches_restatement(vpx, hw, out_hw):
    seed = 0
    for C in adapt_ref.CHANNELS:
        for N in adapt_ref.FRAMES:
            for src, dst in adapt_ref.RANGES:
                seed += 1
                x = torch.from_numpy(adapt_ref.frames((N, C) + hw, src, seed)).cuda()
                _check(vpx, x, out_hw, src, dst, f"{hw}->{out_hw} C={C} N={N} {src}->{dst}")


@pytest.mark.parametrize("hw,out_hw", adapt_ref.SHAPES)
def test_adapt_reads_non_contiguous_split_halves(vpx, hw, out_hw):
    """[b, t, c, h, w] halves of torch.split along t (what unpack_data returns): views with the batch stride of the whole sequence."""
    for C in adapt_ref.CHANNELS:
        for k, (src, dst) in enumerate(adapt_ref.RANGES):
            frames = torch.from_numpy(adapt_ref.frames((2, 5, C) + hw, src, 100 + k)).cuda()
            inp, target = torch.split(frames, [3, 2], dim=1)
            assert not inp.is_contiguous() and not target.is_contiguous()
            for name, half in (("context", inp), ("target", target)):
                got = _check(vpx, half, out_hw, src, dst, f"{hw}->{out_hw} C={C} {name} half {src}->{dst}")
                assert got.ndim == 5 and got.shape[:3] == half.shape[:3]


def test_adapt_unaligned_views_take_the_scalar_paths(vpx):
    """A dense input and output that start 4 bytes off a 16-byte boundary: the affine kernel must not use 16-byte accesses on them."""
    src, dst = (0.0, 1.0), (-1.0, 1.0)
    base = torch.from_numpy(adapt_ref.frames((1 + 2 * 3 * 8 * 8,), src, 7)).cuda()
    x = base[1:].view(2, 3, 8, 8)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    _check(vpx, x, (8, 8), src, dst, "affine, input 4 bytes off")
    _check(vpx, x, (4, 4), src, dst, "resize, input 4 bytes off")


def test_adapt_refuses_gradients_and_bad_inputs(vpx):
    x = torch.rand(1, 1, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(vpx.VpxError, match="forward only"):
        vpx.ops.frames_adapt(x, (2, 2))
    with torch.no_grad():                                              # testing runs under no_grad: nothing is differentiated
        assert vpx.ops.frames_adapt(x, (2, 2)).shape == (1, 1, 2, 2)
    y = torch.rand(1, 1, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="empty source value range"):
        vpx.ops.frames_adapt(y, None, (1.0, 1.0), (0.0, 1.0))
    with pytest.raises(ValueError):
        vpx.ops.frames_adapt(y, (0, 4))
    with pytest.raises(ValueError, match="float32"):
        vpx.ops.frames_adapt(y.double())
    with pytest.raises(ValueError):
        vpx.ops.frames_adapt(y[0, 0])
