"""CPU-side tests of the frame adapter (csrc/adapt.hip): the float64 restatement of tests/adapt_ref.py against torch's own chain, the
library's export and the refusals the entry point makes before any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adapt_ref


@pytest.mark.parametrize("src,dst", adapt_ref.RANGES)
@pytest.mark.parametrize("hw,out_hw", adapt_ref.SHAPES)
def test_restatement_agrees_with_torch_chain(hw, out_hw, src, dst):
    """adapt_ref.adapt against the reference's chain on the CPU in float32: the ScaleToModel expression (utils/models.py:62-63), then
    F.interpolate(mode="bilinear", align_corners=False, antialias=False). 1e-6 on float32 inputs, in units of the destination's
    magnitude max(1, |dst_lo|, |dst_hi|): torch's float32 result itself carries a few roundoffs of 6e-8 RELATIVE to the values (one unit
    in the last place of 255 is 1.5e-5), so an absolute 1e-6 is only defined for values of unit size.
    The source coordinate s * (d + 0.5) - 0.5 is rounded per operation by the kernels (csrc/frames_coord.h, pinned bit for bit by
    tests/test_gpu_frames.py), while ATen's CPU kernel rounds it per operation or once, depending on whether its build contracts the
    expression into a fused multiply-add (the AVX-512 build does). Where the two coordinates differ (64 -> 63 and 64 -> 65 of the table: one
    unit in the last place of a coordinate near 60, 3.8e-6, times the difference of two neighbouring pixels) torch agrees to 1e-6 with
    the restatement on ITS coordinates only; so the restatement is held to 1e-6 with the coordinates rounded one way or the other, and
    both figures are printed."""
    x = adapt_ref.frames((2, 3) + hw, src, seed=(hw[0] * 131 + hw[1] * 17 + out_hw[0] * 5 + out_hw[1]) % 1000)
    img = torch.from_numpy(x)
    if src != dst:
        img = (img - src[0]) / (src[1] - src[0])
        img = img * (dst[1] - dst[0]) + dst[0]
    if out_hw != hw:
        img = F.interpolate(img, size=out_hw, mode="bilinear", align_corners=False, antialias=False)
    got = img.numpy().astype(np.float64)
    errs = []
    for fused in (False, True):
        ref = adapt_ref.adapt(x, out_hw, src, dst, fused_coords=fused)
        assert ref.dtype == np.float64 and ref.shape == (2, 3) + out_hw
        errs.append(np.abs(got - ref).max() / max(1.0, abs(dst[0]), abs(dst[1])))
    print(f"{hw} -> {out_hw}, {src} -> {dst}: |torch - restatement| = {errs[0]:.3e} (coordinates rounded per operation), {errs[1]:.3e} (rounded once)")
    assert min(errs) <= 1e-6, errs


def test_library_exports_frames_adapt(vpx):
    L = vpx._lib.lib()
    assert hasattr(L, "vpx_frames_adapt") and "vpx_frames_adapt" in vpx._lib.EXPORTED_SYMBOLS
    assert len(L.vpx_frames_adapt.argtypes) == 13


def test_refusals_before_any_launch(vpx):
    """NULL pointers, non-positive sizes and an empty source range are refused on the host (VPX_ERR_ARG = -1), without a GPU."""
    L = vpx._lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x=p, N=1, C=1, H=2, W=2, oh=4, ow=4, slo=0.0, shi=1.0, dlo=-1.0, dhi=1.0, out=p)

    def call(**kw):
        a = {**ok, **kw}
        return L.vpx_frames_adapt(a["x"], a["N"], a["C"], a["H"], a["W"], a["oh"], a["ow"], a["slo"], a["shi"], a["dlo"], a["dhi"], a["out"], None)

    for kw, word in [(dict(x=None), b"NULL"), (dict(out=None), b"NULL"), (dict(N=0), b">= 1"), (dict(C=0), b">= 1"), (dict(H=0), b">= 1"),
                     (dict(W=-1), b">= 1"), (dict(oh=0), b">= 1"), (dict(ow=-3), b">= 1"), (dict(slo=0.5, shi=0.5), b"empty source value range")]:
        assert call(**kw) == -1, kw
        assert word in L.vpx_last_error(), (kw, L.vpx_last_error())
    assert call(H=40000) == -4 and b"side" in L.vpx_last_error()


def test_op_refuses_host_tensors_and_bad_arguments(vpx):
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        vpx.ops.frames_adapt(torch.zeros(1, 1, 2, 2))
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        vpx.ops.frames_adapt(np.zeros((1, 1, 2, 2), dtype=np.float32))
