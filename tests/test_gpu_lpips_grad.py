"""LPIPS as a training loss on the GPU (csrc/lpips.hip's backward) against float64 autograd through tests/lpips_ref.py: end to end
(ops.lpips_frames_diff), tap by tap, the three new kernels on their own at their edges, and the public path of measure.py once the
weights are registered with differentiable=True. References, cases and bounds: tests/lpips_grad_ref.py; the conditions on the inputs
are checked on the CPU in tests/test_lpips_grad_host.py.

Bounds. End to end and per tap: lpips_ref.E2E_MARGIN (4) x the max-normalised error of plain float32 CPU autograd over the same chain,
measured in the case builder, never from the library's result. Head: 2^-23 (double arithmetic, a float32 result) plus 4 x the distance between two float64
evaluations of the reference (autograd and the closed form), which is not small at C = 1, where the expression cancels. Pool: the float32
sum of at most four window gradients. Stem: 1e-5, the project's bar for fp32 convolution outputs.

With VPX_LPIPS_GRAD_PARITY_OUT=FILE the figures of every case and tap are written there (the `gradient` section of
profiles/lpips_parity.json was made from it)."""
import functools
import json
import os

import pytest
import torch

import lpips_grad_ref as gref
import lpips_ref
import test_gpu_lpips as base   # the device weights are shared with the forward's tests

pytestmark = pytest.mark.gpu

PARITY_OUT = os.environ.get("VPX_LPIPS_GRAD_PARITY_OUT")
_FIGURES = {}


def _record(case, tap, **figures):
    _FIGURES.setdefault(str(case), {})["whole" if tap is None else f"tap {tap}"] = figures
    if PARITY_OUT:
        with open(PARITY_OUT, "w") as fh:
            json.dump({"what": "d(sum(cotangent * ops.lpips_frames_diff)) / d pred on the GPU against float64 autograd through tests/lpips_ref.py, "
                               "max|got-ref| / max|ref| over the gradient; reference_error: plain float32 CPU autograd over the same chain; "
                               "bound = margin x reference_error; `tap k`: on weights with every lin but lin{k} zeroed",
                       "margin": lpips_ref.E2E_MARGIN, "cases (B, T, H, W)": _FIGURES}, fh, indent=1)


@functools.lru_cache(maxsize=None)
def _device_weights(tap=None):
    return base._device_weights() if tap is None else lpips_ref.isolated(base._device_weights(), tap)


def _grad(p, t, cot, w):
    from vp_suite_amd import ops
    p = p.detach().requires_grad_()
    table = ops.lpips_frames_diff(p, t, w)
    table.backward(cot)
    return table.detach(), p.grad


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gref.E2E_GRAD_CASES)
def test_lpips_frames_diff_vs_fp64(vpx, parity_log, case):
    from vp_suite_amd import ops
    pred, target, cot, ref, ref_err, bound = gref.grad_case(case)
    w = _device_weights()
    p, t, c = pred.cuda(), target.cuda(), cot.cuda()
    table, g = _grad(p, t, c, w)
    assert table.dtype == torch.float64 and tuple(table.shape) == tuple(cot.shape) and g.dtype == torch.float32 and g.shape == p.shape
    assert torch.equal(table, ops.lpips_frames(p, t, w))          # the training forward's table is the evaluation's, bit for bit
    e = parity_log("lpips.grad", g, ref, bound)
    print(f"lpips_frames_diff {case}: kernel {e:.3e}, reference-side {ref_err:.3e}, bound {bound:.3e}")
    _record(case, None, kernel_error=e, reference_error=ref_err, bound=bound)
    table2, g2 = _grad(p, t, c, w)
    assert torch.equal(table2, table) and torch.equal(g2, g)     # bit-reproducible
    _, g0 = _grad(p, t, torch.zeros_like(c), w)
    assert bool((g0 == 0).all())                                  # a zero cotangent: exactly zero
    assert e <= bound, (e, bound)


def test_lpips_frames_diff_on_sliced_inputs(vpx):
    pred, target, cot, ref, _, bound = gref.grad_case((2, 3, 35, 47))
    wide = torch.zeros(2, 4, 3, 37, 50)
    wide[:, 1:, :, 2:, 3:] = pred
    held = wide.cuda().requires_grad_()
    p = held[:, 1:, :, 2:, 3:]
    assert not p.is_contiguous()
    from vp_suite_amd import ops
    ops.lpips_frames_diff(p, target.cuda(), _device_weights()).backward(cot.cuda())
    assert lpips_ref.relmax(held.grad[:, 1:, :, 2:, 3:], ref) <= bound
    outside = held.grad.clone()
    outside[:, 1:, :, 2:, 3:] = 0
    assert bool((outside == 0).all())


def test_lpips_frames_diff_contract(vpx):
    from vp_suite_amd import ops
    pred, target, cot, _, _, _ = gref.grad_case((1, 1, 31, 31))
    w = {k: v.clone().requires_grad_() for k, v in _device_weights().items()}
    p, t = pred.cuda().requires_grad_(), target.cuda()
    table = ops.lpips_frames_diff(p, t, w)
    table.backward(cot.cuda())
    assert p.grad is not None and all(v.grad is None for v in w.values())    # the weights never receive a gradient
    with pytest.raises(NotImplementedError, match="target"):
        ops.lpips_frames_diff(p, t.clone().requires_grad_(), _device_weights())
    with torch.no_grad():                                                     # no grad wanted: the evaluation call
        assert torch.equal(ops.lpips_frames_diff(p, t, _device_weights()), table.detach())


# ---- per tap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gref.TAP_GRAD_CASES)
def test_one_tap_gradient_vs_fp64(vpx, parity_log, case):
    """With every lin{k} zeroed but one the gradient is that tap's share: a wrong slot, map size or layer index in the backward's schedule
    moves one share by its own size. The five shares add up to the whole within float32 summation noise: the float64 shares add up to
    the float64 whole exactly (test_lpips_grad_host), so the distance is at most the sum of the six bounds, each at its reference's size."""
    pred, target, cot, ref_whole, _, _ = gref.grad_case(case)
    p, t, c = pred.cuda(), target.cuda(), cot.cuda()
    _, whole = _grad(p, t, c, _device_weights())
    total, noise, worst = torch.zeros_like(whole, dtype=torch.float64), gref.grad_case(case)[5] * float(ref_whole.abs().max()), []
    for tap in range(1, 6):
        _, _, _, ref, ref_err, bound = gref.grad_case(case, tap)
        _, g = _grad(p, t, c, _device_weights(tap))
        e = parity_log(f"lpips.grad.tap{tap}", g, ref, bound)
        print(f"lpips gradient tap {tap} {case}: kernel {e:.3e}, reference-side {ref_err:.3e}, bound {bound:.3e}")
        _record(case, tap, kernel_error=e, reference_error=ref_err, bound=bound)
        worst.append((tap, e, bound))
        total += g.double()
        noise += bound * float(ref.abs().max())
    assert float((total - whole.double()).abs().max()) <= noise
    for tap, e, bound in worst:
        assert e <= bound, (tap, e, bound)


# ---- head backward -----------------------------------------------------------------------------------------------------------------------
def _head_bwd(C, h, w, scale, with_incoming):
    from vp_suite_amd import ops
    fx, fy, lin, _ = lpips_ref.head_edge_case(C, h, w, scale)
    g = torch.Generator().manual_seed(C * 100 + h * 10 + w)
    dtable = torch.randn(fx.shape[0], generator=g, dtype=torch.float64)
    incoming = torch.randn(fx.shape, generator=g) * float(gref.head_bwd_ref(fx, fy, lin, dtable).abs().max()) if with_incoming else None
    ref, bound = gref.head_bwd_bound(fx, fy, lin, dtable, incoming)
    got = ops.lpips_head_bwd(lpips_ref.nhwc(fx).cuda(), lpips_ref.nhwc(fy).cuda(), lin.cuda(), dtable.cuda(),
                             None if incoming is None else lpips_ref.nhwc(incoming).cuda())
    return fx, lpips_ref.nchw(got.cpu()), ref, bound


@pytest.mark.parametrize("with_incoming", [False, True])
@pytest.mark.parametrize("h,w", lpips_ref.HEAD_EDGE_MAPS)
@pytest.mark.parametrize("C", lpips_ref.HEAD_EDGE_C)
def test_head_bwd_edges_vs_fp64(vpx, parity_log, C, h, w, with_incoming):
    fx, got, ref, bound = _head_bwd(C, h, w, 1.0, with_incoming)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    zero = (fx == 0)
    assert bool(zero.all(dim=1).any()) and bool((got[zero] == 0).all())   # an all-zero vector (and every masked element): 0, not NaN
    e = parity_log("lpips.head_bwd", got, ref, bound)
    print(f"head backward C={C} {h}x{w} incoming={with_incoming}: {e:.3e}, bound {bound:.3e}")
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("with_incoming", [False, True])
@pytest.mark.parametrize("scale,C,h,w", lpips_ref.HEAD_SCALED)
def test_head_bwd_scaled_features(vpx, parity_log, scale, C, h, w, with_incoming):
    fx, got, ref, bound = _head_bwd(C, h, w, scale, with_incoming)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert bool((got[fx == 0] == 0).all())
    e = parity_log("lpips.head_bwd.scaled", got, ref, bound)
    print(f"head backward scale={scale} C={C} {h}x{w} incoming={with_incoming}: {e:.3e}, bound {bound:.3e}")
    assert e <= bound, (scale, e, bound)


def test_head_bwd_in_place_and_refusal(vpx):
    from vp_suite_amd import _lib, ops
    fx, fy, lin, _ = lpips_ref.head_edge_case(100, 5, 13)
    dfx, dfy, dl = lpips_ref.nhwc(fx).cuda(), lpips_ref.nhwc(fy).cuda(), lin.cuda()
    dtable = torch.ones(fx.shape[0], dtype=torch.float64, device="cuda")
    incoming = torch.randn(dfx.shape, device="cuda")
    want = ops.lpips_head_bwd(dfx, dfy, dl, dtable, incoming)
    held = incoming.clone()   # dz may be `incoming` itself: what the whole backward does
    _lib.check(_lib.lib().vpx_lpips_head_bwd(_lib.ptr(dfx), _lib.ptr(dfy), _lib.ptr(dl), _lib.ptr(dtable), _lib.ptr(held), fx.shape[0], 5 * 13, 100,
                                             _lib.ptr(held), ops.stream()), "vpx_lpips_head_bwd")
    assert torch.equal(held, want)
    wide = torch.zeros(1, 1, 1, 513, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.lpips_head_bwd(wide, wide, torch.ones(513, device="cuda"), dtable[:1])


# ---- pool backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gref.POOL_BWD_KINDS)
@pytest.mark.parametrize("C", lpips_ref.POOL_EDGE_C)
@pytest.mark.parametrize("h,w", lpips_ref.POOL_EDGE_MAPS)
def test_maxpool_bwd_edges(vpx, h, w, C, kind):
    from vp_suite_amd import ops
    x, dy = gref.pool_bwd_case(C, h, w, kind)
    ref = gref.pool_bwd_autograd(x, dy)
    got = lpips_ref.nchw(ops.lpips_maxpool_bwd(lpips_ref.nhwc(x).cuda(), lpips_ref.nhwc(dy).cuda()).cpu())
    assert got.shape == x.shape and got.dtype == torch.float32
    assert float((got.double() - ref).abs().max()) <= gref.POOL_BWD_ULPS * 2.0 ** -24 * float(dy.abs().max())
    assert torch.equal(got == 0, ref == 0)          # the same elements take a gradient: the tie rule, window by window
    if h % 2 == 0:                                  # the row / column floor mode drops
        assert bool((got[:, :, -1] == 0).all())
    if w % 2 == 0:
        assert bool((got[:, :, :, -1] == 0).all())
    if kind == "equal":                             # every window tied nine ways: its first element takes all of it
        assert torch.equal(got[:, :, 0:2 * dy.shape[2]:2, 0:2 * dy.shape[3]:2], dy)


# ---- stem backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "bounds"])
@pytest.mark.parametrize("H,W", lpips_ref.STEM_EDGE_SIZES)
def test_stem_bwd_edges_vs_fp64(vpx, parity_log, H, W, kind):
    """noise: pixels inside [-1, 1], beyond it (gradient 0) and, pinned, exactly on -1 and +1 (gradient passes); bounds: every pixel
    exactly -1 or +1, every one passes."""
    from vp_suite_amd import ops
    N = 2
    x, tap1 = lpips_ref.stem_edge_case(N, H, W, kind)
    w = lpips_ref.weights()["conv1.weight"]
    dz = torch.randn(tap1.shape, generator=torch.Generator().manual_seed(H * 100 + W))
    ref = gref.stem_bwd_ref(x, w, dz)
    got = ops.lpips_stem_bwd(x.cuda(), w.cuda(), lpips_ref.nhwc(dz).cuda()).cpu()
    assert got.shape == x.shape and got.dtype == torch.float32
    e = parity_log("lpips.stem_bwd", got, ref, gref.STEM_BWD_TOL)
    print(f"stem backward {H}x{W} {kind}: {e:.3e}")
    assert e <= gref.STEM_BWD_TOL, e
    r0, c0 = gref.stem_uncovered(H, W)
    assert bool((got[:, :, r0:] == 0).all()) and bool((got[:, :, :, c0:] == 0).all())   # no window covers them: exactly 0
    covered = got[:, :, :r0, :c0]
    if kind == "bounds":
        assert bool((covered != 0).all())
    else:
        assert bool((got[x.abs() > 1] == 0).all()) and bool((covered[x[:, :, :r0, :c0].abs() <= 1] != 0).all())
        for y, xx, v in lpips_ref.STEM_PINNED:   # exactly on a bound: the gradient passes
            if y % H < r0 and xx % W < c0:
                assert bool((x[:, :, y, xx] == v).all()) and bool((got[:, :, y, xx] != 0).all())


# ---- the public path ------------------------------------------------------------------------------------------------------------------
def test_provider_trains_through_lpips(vpx):
    from vp_suite_amd import measure as M
    case = (2, 3, 35, 47)
    pred, target, _, _, _, bound = gref.grad_case(case)
    B, T = case[:2]
    M.register_lpips_weights(lpips_ref.weights(), differentiable=True)
    try:
        provider = M.PredictionLossProvider({"device": "cuda", "losses_and_scales": {"l1": 1.0, "lpips": 0.5}})
        p, t = pred.cuda().requires_grad_(), target.cuda()
        disp, total = provider.get_losses(p, t)
        total.backward()
        with torch.no_grad():
            disp0, total0 = provider.get_losses(p, t)
        assert float(total0) == float(total.detach()) and float(disp0["lpips"]) == float(disp["lpips"].detach())   # the value is the no-grad call's
        p64 = pred.double().requires_grad_()
        w64 = {k: v.double() for k, v in lpips_ref.weights().items()}
        lp = M._lpips_host(p64, target.double(), w64).mean(dim=1).mean(dim=0)                     # the float64 host path under autograd
        (g_lp,) = torch.autograd.grad(0.5 * lp, p64)
        g_l1 = torch.sign(pred.double() - target.double()) / (B * T)
        got = p.grad.cpu().double()
        # the LPIPS share is held to the end-to-end bound; the sum with the (far larger) L1 share costs one float32 rounding at the sum's size
        tol = bound * float(g_lp.abs().max()) + 2.0 ** -23 * float((g_l1 + g_lp).abs().max())
        assert float((got - g_l1 - g_lp).abs().max()) <= tol, (float((got - g_l1 - g_lp).abs().max()), tol)
        assert float(g_lp.abs().max()) > 100 * tol   # the check sees the LPIPS share
    finally:
        M.clear_lpips_weights()
    with pytest.raises(NotImplementedError):          # cleared: LPIPS is gone again
        M.PredictionLossProvider({"device": "cuda", "losses_and_scales": {"lpips": 1.0}})
