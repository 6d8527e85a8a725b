"""The LPIPS gradient without a GPU: the two rules the backward kernels state (which tied element of a pool window takes the gradient,
what the clamp does at its bounds) against torch's CPU autograd in float64, the opt-in of measure.register_lpips_weights, the new C
entry points of csrc/lpips.hip in a dry run, and the conditions on the inputs of tests/test_gpu_lpips_grad.py."""
import ctypes

import pytest
import torch

import lpips_grad_ref as gref
import lpips_ref
from test_workspace_contract import E_ARG, E_UNSUPPORTED, E_WS, OK, WS_BASE, WS_BASE_ODD, L, _fake, _ok  # noqa: F401  (L: the dry-run fixture)
from vp_suite_amd import measure as M
from vp_suite_amd import ops

RES_BASE = 0x7E0000000000   # a fake reserve, away from the fake workspace


# ---- the two rules -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ties", "equal"])
@pytest.mark.parametrize("h,w", lpips_ref.POOL_EDGE_MAPS)
def test_pool_tie_rule_is_torchs(h, w, kind):
    """csrc/lpips.hip's lpips_maxpool_bwd_kernel hands a window's gradient to the FIRST maximal element in row-major order. torch's CPU
    max_pool2d backward, float64, on inputs full of ties, does the same — in both memory formats."""
    x, dy = gref.pool_bwd_case(5, h, w, kind)
    want = gref.first_max_pool_bwd(x, dy)
    if kind == "ties":
        win = torch.nn.functional.unfold(x, 3, stride=2).view(x.shape[0], x.shape[1], 9, -1)
        assert bool(((win == win.max(dim=2, keepdim=True).values).sum(dim=2) > 1).float().mean() > 0.5)   # most windows are tied
    assert torch.equal(gref.pool_bwd_autograd(x, dy), want)
    v = x.double().contiguous(memory_format=torch.channels_last).requires_grad_()
    (lpips_ref.maxpool(v) * dy.double()).sum().backward()
    assert torch.equal(v.grad, want)
    if h % 2 == 0:   # floor mode drops the last row: no gradient there
        assert bool((want[:, :, -1] == 0).all())
    if w % 2 == 0:
        assert bool((want[:, :, :, -1] == 0).all())


def test_clamp_mask_at_the_bounds_is_torchs():
    """lpips_stem_bwd_kernel passes the gradient where 0 <= (v + 1) / 2 <= 1, bounds included: torch's clamp does at v = -1 and v = +1,
    and blocks it on the first float32 beyond either."""
    beyond = torch.nextafter(torch.tensor([1.0, -1.0]), torch.tensor([2.0, -2.0]))
    v = torch.tensor([-1.0, 1.0, 0.25, float(beyond[0]), float(beyond[1])], dtype=torch.float64).view(1, 1, 1, 5).repeat(1, 3, 1, 1).requires_grad_()
    lpips_ref.normalise(v).sum().backward()
    for c in range(3):
        slope = 0.5 / lpips_ref.STD[c]
        assert v.grad[0, c, 0].tolist() == [slope, slope, slope, 0.0, 0.0]
    # the kernel evaluates the mask on the forward's own float32 (v + 1) / 2: exact at the bounds, and still beyond them one float32 on
    u = (torch.tensor([-1.0, 1.0]) + 1.0) * 0.5
    assert u.tolist() == [0.0, 1.0]
    assert float((beyond[1] + 1.0) * 0.5) < 0.0
    # one float32 above +1 the sum v + 1 rounds back to 2: this side needs the margin that test_grad_case_conditions asks of the inputs
    assert float((beyond[0] + 1.0) * 0.5) == 1.0


# ---- the opt-in ---------------------------------------------------------------------------------------------------------------------
def test_differentiable_flag_is_reset_by_clear(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "lpips_frames_diff", lambda *a: calls.append("diff"), raising=True)
    M.register_lpips_weights(lpips_ref.weights(), differentiable=True)
    assert M._lpips_differentiable is True
    M.clear_lpips_weights()
    assert M._lpips_differentiable is False
    M.register_lpips_weights(lpips_ref.weights())   # the default: the refusal path
    try:
        assert M._lpips_differentiable is False
    finally:
        M.clear_lpips_weights()
    assert calls == []


class _OnGpu:
    """What frame_lpips asks of a prediction before it hands it to ops: a 5-D shape, is_cuda, device, requires_grad."""

    def __init__(self, requires_grad):
        self.shape, self.ndim, self.is_cuda, self.device, self.requires_grad = torch.Size((1, 1, 3, 31, 31)), 5, True, "cpu", requires_grad


@pytest.mark.parametrize("differentiable,requires_grad,want", [(False, True, "frames"), (False, False, "frames"), (True, False, "frames"), (True, True, "diff")])
def test_frame_lpips_routing(monkeypatch, differentiable, requires_grad, want):
    """Default registration: ops.lpips_frames whatever the prediction (which refuses one that requires grad); differentiable=True: a
    prediction that requires grad goes to ops.lpips_frames_diff, every other one stays on ops.lpips_frames."""
    calls = []

    class _Table:
        def float(self):
            return self

    monkeypatch.setattr(ops, "lpips_frames", lambda *a: calls.append("frames") or _Table())
    monkeypatch.setattr(ops, "lpips_frames_diff", lambda *a: calls.append("diff") or _Table())
    monkeypatch.setattr(ops, "needs_grad", lambda *ts: torch.is_grad_enabled() and any(t.requires_grad for t in ts))
    if differentiable:
        M.register_lpips_weights(lpips_ref.weights(), differentiable=True)
    else:
        M.register_lpips_weights(lpips_ref.weights())
    try:
        p = _OnGpu(requires_grad)
        M.frame_lpips(p, _OnGpu(False))
        assert calls == [want]
        with torch.no_grad():
            M.frame_lpips(p, _OnGpu(False))
        assert calls == [want, "frames"]
    finally:
        M.clear_lpips_weights()


def test_diff_refuses_a_target_that_requires_grad():
    p, t = torch.zeros(1, 1, 3, 31, 31), torch.zeros(1, 1, 3, 31, 31, requires_grad=True)
    with pytest.raises(NotImplementedError, match="target"):
        ops.lpips_frames_diff(p, t, lpips_ref.weights())
    with pytest.raises(ValueError, match="31x31"):
        ops.lpips_frames_diff(p[..., :30], p[..., :30], lpips_ref.weights())


# ---- C ABI in a dry run ---------------------------------------------------------------------------------------------------------------
def test_training_entry_points_dry_run(L):
    params = (ctypes.c_void_p * 15)(*[0x200000000000 + i * (1 << 30) for i in range(15)])
    for B, T, H, W in lpips_ref.GEOMETRY_CASES:
        n = B * T
        sizes = lpips_ref.tap_sizes(H, W)
        nb, rb, bb = L.vpx_lpips_workspace_bytes(n, H, W), L.vpx_lpips_reserve_bytes(n, H, W), L.vpx_lpips_bwd_workspace_bytes(n, H, W)
        assert nb > 0 and bb > 0
        align = lambda v: (v + 255) // 256 * 256   # noqa: E731
        assert rb == sum(align(2 * n * h * w * c * 4) for (h, w), c in zip(sizes, (64, 192, 384, 256, 256))) + 256   # the documented formula
        for base, res in ((WS_BASE, RES_BASE), (WS_BASE_ODD, RES_BASE + 0x40)):
            for det in (0, 1):
                L.vpx_set_deterministic(det)
                _ok(L, L.vpx_lpips_fwd_train(_fake(1), _fake(2), n, 3, H, W, params, _fake(3), ctypes.c_void_p(res), rb, ctypes.c_void_p(base), nb, None),
                    f"lpips fwd_train {(B, T, H, W)}", False)
                _ok(L, L.vpx_lpips_bwd(_fake(1), params, ctypes.c_void_p(res), _fake(3), n, 3, H, W, _fake(4), ctypes.c_void_p(base), bb, None),
                    f"lpips bwd {(B, T, H, W)}", False)
        L.vpx_set_deterministic(0)
        args = (_fake(1), _fake(2), n, 3, H, W, params, _fake(3))
        assert L.vpx_lpips_fwd_train(*args, ctypes.c_void_p(RES_BASE), rb - 1, ctypes.c_void_p(WS_BASE), nb, None) == E_WS
        assert L.vpx_lpips_fwd_train(*args, ctypes.c_void_p(RES_BASE), rb, ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
        assert L.vpx_lpips_fwd_train(*args, None, rb, ctypes.c_void_p(WS_BASE), nb, None) == E_WS
        assert L.vpx_lpips_bwd(_fake(1), params, ctypes.c_void_p(RES_BASE), _fake(3), n, 3, H, W, _fake(4), ctypes.c_void_p(WS_BASE), bb - 1, None) == E_WS
        assert L.vpx_lpips_bwd(_fake(1), params, None, _fake(3), n, 3, H, W, _fake(4), ctypes.c_void_p(WS_BASE), bb, None) == E_ARG
    assert L.vpx_lpips_reserve_bytes(1, 30, 31) == 0 and L.vpx_lpips_bwd_workspace_bytes(0, 31, 31) == 0
    assert L.vpx_lpips_bwd(_fake(1), params, ctypes.c_void_p(RES_BASE), _fake(3), 1, 1, 31, 31, _fake(4), ctypes.c_void_p(WS_BASE), 1 << 30, None) == E_ARG


def test_piece_entry_points_dry_run(L):
    nb = L.vpx_lpips_stem_workspace_bytes()
    for H, W in lpips_ref.STEM_EDGE_SIZES:
        _ok(L, L.vpx_lpips_stem_bwd(_fake(1), _fake(2), _fake(3), 2, H, W, _fake(4), ctypes.c_void_p(WS_BASE_ODD), nb, None), f"stem bwd {(H, W)}", False)
    assert L.vpx_lpips_stem_bwd(_fake(1), _fake(2), _fake(3), 1, 6, 7, _fake(4), ctypes.c_void_p(WS_BASE), nb, None) == E_ARG
    assert L.vpx_lpips_stem_bwd(_fake(1), _fake(2), _fake(3), 1, 7, 7, _fake(4), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
    for h, w in lpips_ref.POOL_EDGE_MAPS:
        for C in lpips_ref.POOL_EDGE_C:
            _ok(L, L.vpx_lpips_maxpool_bwd(_fake(1), _fake(2), _fake(3), 2, h, w, C, None), f"pool bwd {(h, w, C)}", False)
    assert L.vpx_lpips_maxpool_bwd(_fake(1), _fake(2), _fake(3), 2, 2, 5, 4, None) == E_ARG
    for C in lpips_ref.HEAD_EDGE_C:
        for h, w in lpips_ref.HEAD_EDGE_MAPS:
            for incoming in (None, _fake(5)):
                _ok(L, L.vpx_lpips_head_bwd(_fake(1), _fake(2), _fake(3), _fake(4), incoming, 3, h * w, C, _fake(6), None), f"head bwd {(C, h, w)}", False)
    assert L.vpx_lpips_head_bwd(_fake(1), _fake(2), _fake(3), _fake(4), None, 3, 9, 513, _fake(6), None) == E_UNSUPPORTED
    assert L.vpx_lpips_head_bwd(_fake(1), _fake(2), _fake(3), None, None, 3, 9, 64, _fake(6), None) == E_ARG


# ---- conditions on the inputs of the GPU tests --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gref.E2E_GRAD_CASES)
def test_grad_case_conditions(case):
    """The bound (E2E_MARGIN x the float32 CPU autograd's error) stays under the ceiling, and the prediction's chain keeps away from its
    kinks: no ReLU pre-activation, no runner-up of a pool window and no clamp argument within ten times the float32 chain's own error
    of the point where the gradient jumps (there a float32 chain and the float64 one may take different branches, and the gradient
    is off by a whole term, not by rounding)."""
    assert case in lpips_ref.GEOMETRY_CASES[:3] + (lpips_ref.E2E_CASES[1],)
    pred, target, cot, ref, ref_err, bound = gref.grad_case(case)
    assert tuple(ref.shape) == tuple(pred.shape) and float(ref.abs().max()) > 0 and bool(torch.isfinite(ref).all())
    assert float(pred.abs().max()) > 1.0   # the clamp acts
    assert 0 < bound <= gref.GRAD_CEILING, bound
    for name, (margin, err) in gref.kink_margins(case).items():
        print(f"{case} {name}: margin {margin:.3e}, float32 error {err:.3e}")
        assert margin > gref.KINK_FACTOR * err, (name, margin, err)


@pytest.mark.parametrize("case", gref.TAP_GRAD_CASES)
def test_tap_grad_case_conditions(case):
    whole = gref.grad_case(case)[3]
    total = torch.zeros_like(whole)
    for tap in range(1, 6):
        _, _, _, ref, ref_err, bound = gref.grad_case(case, tap)
        assert float(ref.abs().max()) > 0 and 0 < bound <= gref.GRAD_CEILING, (tap, bound)
        total = total + ref
    assert lpips_ref.relmax(total, whole) < 1e-12   # the measure is linear in the lin weights: the shares are the whole


def test_piece_references():
    for C in (1, 5):   # the head reference: zero at an all-zero vector, finite everywhere
        fx, fy, lin, _ = lpips_ref.head_edge_case(C, 5, 13)
        g = gref.head_bwd_ref(fx, fy, lin, torch.ones(fx.shape[0], dtype=torch.float64))
        assert bool(torch.isfinite(g).all()) and bool((g[fx == 0] == 0).all()) and float(g.abs().max()) > 0
    assert gref.stem_uncovered(10, 7) == (9, 7) and gref.stem_uncovered(7, 10) == (7, 9) and gref.stem_uncovered(67, 38) == (67, 37)
    x, _ = lpips_ref.stem_edge_case(2, 10, 7, "noise")
    dz = torch.randn(2, 64, 1, 1, generator=torch.Generator().manual_seed(1))
    g = gref.stem_bwd_ref(x, lpips_ref.weights()["conv1.weight"], dz)
    assert bool((g[:, :, 9:] == 0).all()) and bool((g[x.abs() > 1] == 0).all()) and bool((g[:, :, 0, 0] != 0).all())   # (0, 0) is pinned at -1: it passes
