"""The two normalisation kernels against an fp64 restatement, at the shapes and statistics where they can go wrong: LayerNorm([C,H,W])
(csrc/layernorm.hip through `ops.layer_norm_chw`, the public form of vpx_layernorm_fwd/_bwd) and GroupNorm + LeakyReLU + residual
(csrc/groupnorm.hip through `phy_ops.group_norm`).

Reference: F.layer_norm / F.group_norm on the CPU in float64 with autograd, on the same float32 inputs cast up. Bounds, in the suite's
metric max|Δ| / max|ref|: forward 1e-5, every gradient 5e-5. Every case first holds the same CPU restatement in float32 to a quarter of
those bars against fp64: a condition on the inputs (the regime is well enough conditioned to judge a kernel by), with room left for an
equally valid fp32 summation order.

Input regimes: `centred` randn * 2 + 0.5; `offset` randn + 30 (mean 30 standard deviations out: a one-pass E[x²] - E[x]² variance or a
carelessly summed mean shows); `below_eps` randn * 1e-4 (variance 1e-8 against eps = 1e-5, y ~ x / sqrt(eps): a misplaced eps shows).

LeakyReLU: an element whose fp64 pre-activation has |z| < 1e-5 may take either slope. Such elements (at most 0.1 % of a case) are left
out of the dx comparison; what their choice moves elsewhere — dγ / dβ of their channel, and dx of their group through the two group
means of the backward — is bounded from the fp64 quantities and subtracted from the difference before it is measured (`_allowances`)."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from golden_util import name_seed, seeded_randn

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 5e-5
EPS = 1e-5
SLOPE = 0.2
KINK = 1e-5            # |z| below which either LeakyReLU slope is accepted
MAX_LEFT_OUT = 1e-3    # share of a case's elements that may be that close to the kink

REGIMES = {"centred": lambda z: z * 2.0 + 0.5, "offset": lambda z: z + 30.0, "below_eps": lambda z: z * 1e-4}

LN_SHAPES = [(3, 28, 6, 7),      # n = 1176: 64 does not divide it, ragged last chunk
             (2, 3, 1, 5),       # n = 15: fewer elements than chunks
             (1, 1, 1, 1),       # n = 1: y = beta, dx = 0
             (130, 4, 2, 3),     # batch past two 64-thread blocks of the finalise kernels
             (2, 64, 16, 16)]    # a model-sized sample
GN_SHAPES = [(3, 49, 16, 16, 7),     # PhyCell: 7 channels per group, 4 threads idle
             (2, 16, 5, 7, 16),      # 1 channel per group: 256 pixel rows, HW = 35 < 256
             (2, 256, 3, 3, 1),      # 256 channels per group (the limit): one pixel row
             (1, 130, 2, 3, 1),      # 130 per group: one row, 126 idle threads in both block sums; a single sample
             (2, 32, 1, 1, 16),      # HW = 1: two values per group
             (4, 64, 16, 16, 16)]    # the DCGAN layer
GN_VARIANTS = ["plain", "leaky", "leaky_residual"]
# Every regime at every shape but one: two-value groups at a mean of 30. There the group with the smallest spread, which has to carry
# max|dx| for dx to be resolved at all (see _gn_case), has rstd ~ 100, and F.group_norm in fp32 (y = x · rstd γ + (β - mean · rstd γ))
# loses 30 · 6e-8 · rstd in y: none of 3000 draws per variant holds the condition (the best: 3.6 to 9.8 times it; typical: y 1e-5 to
# 6e-5, dx 7e-4 to 2e-2, dγ 1e-5 to 8e-5 of the fp32 restatement against fp64), also not with inputs on a grid that makes every pair's
# mean exact. By the rule that keeps `randn + 1000` out, the combination would measure conditioning, not the kernel.
GN_CASES = [(s, r) for s in GN_SHAPES for r in REGIMES if not (s == (2, 32, 1, 1, 16) and r == "offset")]
_ids = lambda s: "x".join(map(str, s))


# ---- shared plumbing -----------------------------------------------------------------------------------------------------------------
def _measure(parity_log, name, got, ref, bound, allow=None):
    """The recorded max|got - ref| / max|ref|. `allow` (same shape, >= 0, inf where an element is left out): what the free slope choice
    of the elements at the LeakyReLU kink may move, taken off |got - ref| element by element first."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if allow is not None:
        d = got - ref
        got = ref + torch.sign(d) * (d.abs() - allow).clamp(min=0.0)
    return parity_log(name, got, ref, bound)


def _check(parity_log, tag, got, ref, allow=None, share=1.0):
    """Forward and every gradient of `got` (name -> tensor) against `ref` at `share` of the bars; returns the figures."""
    errs = {}
    for k, r in ref.items():
        bound = (FWD_TOL if k == "y" else GRAD_TOL) * share
        errs[k] = _measure(parity_log, f"{tag}.{k if k == 'y' else 'grad.' + k}", got[k], r, bound, None if allow is None else allow.get(k))
        assert errs[k] <= bound if share < 1.0 else errs[k] < bound, (tag, k, errs[k], bound)
    return errs


@contextlib.contextmanager
def _spy(L, name):
    """Records the arguments of every call of one library entry point (the op wrappers look it up on the loaded library per call)."""
    real, calls = getattr(L, name), []

    def wrapped(*args):
        calls.append(args)
        return real(*args)
    setattr(L, name, wrapped)
    try:
        yield calls
    finally:
        setattr(L, name, real)


def _inputs(tag, shape, pshape, regime, residual=False, base=0):
    seed = name_seed(tag, base)
    t = {"x": REGIMES[regime](seeded_randn(shape, seed)), "w": 1.0 + 0.3 * seeded_randn(pshape, seed + 1),
         "b": 0.3 * seeded_randn(pshape, seed + 2), "dy": seeded_randn(shape, seed + 4)}
    if residual:
        t["r"] = seeded_randn(shape, seed + 3)
    return t   # float32: the regime is applied in float32, the fp64 run casts these up


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
def _ln_cpu(t, dtype):
    x, w, b = (t[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x", "w", "b"))
    y = F.layer_norm(x, list(w.shape), w, b, EPS)
    y.backward(t["dy"].to(dtype))
    return {"y": y.detach(), "dx": x.grad, "dgamma": w.grad, "dbeta": b.grad}


@functools.lru_cache(maxsize=None)
def _ln_case(shape, regime):
    """Inputs, the fp64 reference and the fp32 CPU restatement of one case: computed once, shared, never written.
    A sample of one element has x̂ = 0, so dx = dγ = 0 exactly, where autograd leaves the rounding error of the terms that cancel
    (fp64: 1e-14; the fp32 restatement: 1e-5, no figure to set a condition by). There the reference is the exact zero, which the
    metric max|Δ| / max|ref| holds the kernel to bit for bit, and the fp32 restatement is asked for y and dβ alone."""
    t = _inputs(f"norms.ln.{shape}.{regime}", shape, shape[1:], regime)
    ref, cpu32 = _ln_cpu(t, torch.float64), _ln_cpu(t, torch.float32)
    if shape[1:] == (1, 1, 1):
        for k in ("dx", "dgamma"):
            assert float(ref[k].abs().max()) < 1e-10   # (fp64 rounding of terms of order 30)
            ref[k] = torch.zeros_like(ref[k])
            cpu32[k] = torch.zeros_like(cpu32[k])
    return t, ref, cpu32


def _ln_gpu(vpx, t, channels_last=False, backward=True):
    x = t["x"].cuda()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x, w, b = x.requires_grad_(True), t["w"].cuda().requires_grad_(True), t["b"].cuda().requires_grad_(True)
    y = vpx.ops.layer_norm_chw(x, w, b)
    if not backward:
        return {"y": y.detach()}
    y.backward(t["dy"].cuda())
    return {"y": y.detach(), "dx": x.grad, "dgamma": w.grad, "dbeta": b.grad}


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("shape", LN_SHAPES, ids=_ids)
def test_layernorm_parity_vs_fp64(vpx, parity_log, shape, regime):
    """Forward, dx, dγ, dβ of `ops.layer_norm_chw` against fp64, input given as contiguous NCHW; the same input channels-last gives
    the same bits."""
    t, ref, cpu32 = _ln_case(shape, regime)
    _check(parity_log, "ln.cpu_fp32", cpu32, ref, share=0.25)
    got = _ln_gpu(vpx, t)
    errs = _check(parity_log, "ln", got, ref)
    print(f"layernorm {shape} {regime}: {errs}")
    if shape[1:] == (1, 1, 1):   # one element per sample: y = β, dβ = dy, and (through the zero reference above) dx = dγ = 0
        assert torch.equal(got["y"].cpu(), t["b"].expand(shape)) and torch.equal(got["dbeta"].cpu(), t["dy"].sum(0))
        assert not got["dx"].any() and not got["dgamma"].any()
    got_cl = _ln_gpu(vpx, t, channels_last=True)
    for k in got:
        assert torch.equal(got[k], got_cl[k]), k


@pytest.mark.parametrize("shape", LN_SHAPES, ids=_ids)
def test_layernorm_inference_forward_writes_no_xhat_same_bits(vpx, shape):
    """Under torch.no_grad() (parameters that require a gradient all the same) the forward runs in its `xhat == NULL` form, and gives
    the bits of the grad-mode forward."""
    t, _, _ = _ln_case(shape, "centred")
    x, w, b = t["x"].cuda(), t["w"].cuda().requires_grad_(True), t["b"].cuda().requires_grad_(True)
    with _spy(vpx._lib.lib(), "vpx_layernorm_fwd") as calls:
        y_train = vpx.ops.layer_norm_chw(x, w, b)
        with torch.no_grad():
            y_eval = vpx.ops.layer_norm_chw(x, w, b)
    assert len(calls) == 2 and calls[0][4] is not None and calls[1][4] is None   # (argument 4: xhat)
    assert y_train.requires_grad and not y_eval.requires_grad
    assert torch.equal(y_train.detach(), y_eval)


@pytest.mark.parametrize("shape", [(3, 28, 6, 7), (130, 4, 2, 3)], ids=_ids)
def test_layernorm_repeated_backward_same_bits(vpx, shape):
    """Two backward passes through one graph, and two whole runs in deterministic mode: the same bits."""
    t, _, _ = _ln_case(shape, "centred")
    x, w, b = (t[k].cuda().requires_grad_(True) for k in ("x", "w", "b"))
    y = vpx.ops.layer_norm_chw(x, w, b)
    dy = t["dy"].cuda()
    first = torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)
    second = torch.autograd.grad(y, (x, w, b), dy)
    for a, c in zip(first, second):
        assert torch.equal(a, c)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = [_ln_gpu(vpx, t) for _ in range(2)]
    finally:
        torch.use_deterministic_algorithms(prev)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
        assert torch.equal(runs[0][k], {"y": y.detach(), "dx": first[0], "dgamma": first[1], "dbeta": first[2]}[k]), k


def test_layernorm_parity_after_inplace_parameter_update(vpx, parity_log):
    """The wrapper keeps a channels-last copy of each parameter, keyed on (the tensor, its version, its address): an in-place update
    must be seen by the next call."""
    shape = (3, 28, 6, 7)
    t, _, _ = _ln_case(shape, "centred")
    x, w, b = t["x"].cuda(), t["w"].cuda().requires_grad_(True), t["b"].cuda().requires_grad_(True)
    w_cpu, b_cpu = t["w"].clone(), t["b"].clone()

    def fp64():
        return F.layer_norm(t["x"].double(), list(shape[1:]), w_cpu.double(), b_cpu.double(), EPS)

    y0 = vpx.ops.layer_norm_chw(x, w, b).detach()   # fills the cache
    assert _measure(parity_log, "ln.update.y_before", y0, fp64(), FWD_TOL) < FWD_TOL
    with torch.no_grad():
        w.mul_(1.5)
        w_cpu.mul_(1.5)
        y1 = vpx.ops.layer_norm_chw(x, w, b)
    assert not torch.equal(y0, y1)
    assert _measure(parity_log, "ln.update.y_after_weight", y1, fp64(), FWD_TOL) < FWD_TOL
    with torch.no_grad():
        b.add_(0.25)
        b_cpu.add_(0.25)
    y2 = vpx.ops.layer_norm_chw(x, w, b)   # grad mode: the backward must read the updated weight too
    assert _measure(parity_log, "ln.update.y_after_bias", y2, fp64(), FWD_TOL) < FWD_TOL
    xg = x.clone().requires_grad_(True)
    vpx.ops.layer_norm_chw(xg, w, b).backward(t["dy"].cuda())
    x64 = t["x"].double().requires_grad_(True)
    F.layer_norm(x64, list(shape[1:]), w_cpu.double(), b_cpu.double(), EPS).backward(t["dy"].double())
    assert _measure(parity_log, "ln.update.grad.dx", xg.grad, x64.grad, GRAD_TOL) < GRAD_TOL


def test_layernorm_other_eps_raises(vpx):
    x = torch.zeros(2, 3, 4, 5, device="cuda")
    w, b = torch.ones(3, 4, 5, device="cuda"), torch.zeros(3, 4, 5, device="cuda")
    with _spy(vpx._lib.lib(), "vpx_layernorm_fwd") as calls:
        with pytest.raises(ValueError):
            vpx.ops.layer_norm_chw(x, w, b, eps=1e-6)
    assert not calls


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------------
def _gn_cpu(t, G, slope, dtype):
    names = [k for k in ("x", "w", "b", "r") if k in t]
    leaves = {k: t[k].detach().clone().to(dtype).requires_grad_(True) for k in names}
    z = F.group_norm(leaves["x"], G, leaves["w"], leaves["b"], eps=EPS)
    y = z if slope is None else F.leaky_relu(z, slope)
    if "r" in leaves:
        y = y + leaves["r"]
    y.backward(t["dy"].to(dtype))
    out = {"y": y.detach(), "dx": leaves["x"].grad, "dgamma": leaves["w"].grad, "dbeta": leaves["b"].grad}
    if "r" in leaves:
        out["dr"] = leaves["r"].grad
    return out, z.detach()


def _allowances(t, z, G, slope):
    """(share of elements at the kink, name -> allowance or None). With |z| < KINK at element i, LeakyReLU' may be 1 or `slope`: dz_i
    moves by J_i = (1 - slope) |dy_i|. That moves y_i by at most (1 - slope) |z_i|, dβ_c by J_i, dγ_c by J_i |x̂_i|, and — through the
    group means m1 = mean(dz γ), m2 = mean(dz γ x̂) of dx = rstd (dz γ - m1 - x̂ m2) — dx_j of the same group by at most
    rstd (J_i |γ_c| + |x̂_j| J_i |γ_c| |x̂_i|) / m. dx_i itself is left out."""
    kink = z.abs() < KINK
    if slope is None or not bool(kink.any()):
        return 0.0, None
    x, w, dy = t["x"].double(), t["w"].double(), t["dy"].double()
    N, C, H, W = x.shape
    m = (C // G) * H * W
    xg = x.reshape(N, G, m)
    rstd = (xg.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xh = ((xg - xg.mean(-1, keepdim=True)) * rstd).abs()
    J = (1.0 - slope) * dy.abs() * kink
    Jg = (J * w.abs().view(1, C, 1, 1)).reshape(N, G, m)
    dx = (rstd * (Jg.sum(-1, keepdim=True) + xh * (Jg * xh).sum(-1, keepdim=True)) / m).reshape(x.shape)
    dx[kink] = float("inf")
    xh = xh.reshape(x.shape)
    return float(kink.double().mean()), {"y": (1.0 - slope) * z.abs() * kink, "dx": dx, "dgamma": (J * xh).sum((0, 2, 3)), "dbeta": J.sum((0, 2, 3))}


def _holds(cpu32, ref, allow, share=0.25):
    """The condition on the inputs: the fp32 CPU restatement within `share` of the bars of fp64."""
    unrecorded = lambda name, g, r, bound: float((g - r).abs().max() / (r.abs().max() + 1e-30))   # (parity.record's figure)
    return all(_measure(unrecorded, k, cpu32[k], r, None, None if allow is None else allow.get(k)) <= (FWD_TOL if k == "y" else GRAD_TOL) * share
               for k, r in ref.items())


@functools.lru_cache(maxsize=None)
def _gn_case(shape, regime, variant):
    """Inputs, the fp64 reference, the fp32 CPU restatement and the kink allowances of one case: computed once, shared, never written.

    Groups of two values (HW = 1, two channels per group) with a spread of order 1 have x̂ = ±(1 - eps / 2d²) (d: half the difference)
    and dx = rstd (dz₁γ₁ - dz₂γ₂) / 2 · eps / (d² + eps): 1e-5 of its own terms, which no fp32 evaluation through x̂ resolves (the CPU
    restatement: 1e-3 to 2e-2 of max|dx| at most draws). A draw is well conditioned only when one group with a small spread carries
    max|dx|. So every case takes the first draw, base = 0, 1, ... of its seed, at which the fp32 CPU restatement holds the condition:
    base 0 everywhere but at that shape in the `centred` regime. The choice never looks at the kernel, and the test asserts the
    condition on what was chosen. In the `offset` regime that shape has no such draw (GN_CASES)."""
    N, C, H, W, G = shape
    slope = None if variant == "plain" else SLOPE
    for base in range(64):
        t = _inputs(f"norms.gn.{shape}.{regime}.{variant}", (N, C, H, W), (C,), regime, residual=variant == "leaky_residual", base=base)
        ref, z = _gn_cpu(t, G, slope, torch.float64)
        cpu32, _ = _gn_cpu(t, G, slope, torch.float32)
        left_out, allow = _allowances(t, z, G, slope)
        if left_out <= MAX_LEFT_OUT and _holds(cpu32, ref, allow):
            break
    return t, ref, cpu32, left_out, allow, base


def _gn_gpu(t, G, slope, train_params=True):
    from vp_suite_amd import phy_ops
    x = t["x"].cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w, b = t["w"].cuda().requires_grad_(train_params), t["b"].cuda().requires_grad_(train_params)
    r = t["r"].cuda().requires_grad_(True) if "r" in t else None
    y = phy_ops.group_norm(x, G, w, b, leaky_slope=slope, residual=r)
    y.backward(t["dy"].cuda())
    out = {"y": y.detach(), "dx": x.grad, "dgamma": w.grad, "dbeta": b.grad}
    if r is not None:
        out["dr"] = r.grad
    return out


@pytest.mark.parametrize("variant", GN_VARIANTS)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: f"{_ids(c[0])}-{c[1]}")
def test_phydnet_groupnorm_parity_vs_fp64(vpx, parity_log, case, variant):
    """Forward, dx, dγ, dβ (and the residual's gradient) of `phy_ops.group_norm` against fp64."""
    shape, regime = case
    t, ref, cpu32, left_out, allow, base = _gn_case(shape, regime, variant)
    assert left_out <= MAX_LEFT_OUT, left_out
    _check(parity_log, "gn.cpu_fp32", cpu32, ref, allow, share=0.25)
    got = _gn_gpu(t, shape[4], None if variant == "plain" else SLOPE)
    errs = _check(parity_log, "gn", got, ref, allow)
    print(f"groupnorm {shape} {regime} {variant}: draw {base}, left out {left_out:.1e} {errs}")
    if "dr" in got:
        assert torch.equal(got["dr"].cpu(), t["dy"])


@pytest.mark.parametrize("variant", ["plain", "leaky_residual"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=_ids)
def test_phydnet_groupnorm_frozen_parameters_same_dx_bits(vpx, shape, variant):
    """weight and bias frozen: the backward runs in its `dgamma == dbeta == NULL` form (no partials, no reduce launch) and gives the
    dx bits of the run in which they train."""
    t = _gn_case(shape, "centred", variant)[0]
    slope = None if variant == "plain" else SLOPE
    with _spy(vpx._lib.lib(), "vpx_groupnorm_bwd") as calls:
        trained = _gn_gpu(t, shape[4], slope)
        frozen = _gn_gpu(t, shape[4], slope, train_params=False)
    assert len(calls) == 2
    assert calls[0][6] is not None and calls[0][7] is not None and calls[1][6] is None and calls[1][7] is None   # (dgamma, dbeta)
    assert frozen["dgamma"] is None and frozen["dbeta"] is None
    assert torch.equal(frozen["y"], trained["y"]) and torch.equal(frozen["dx"], trained["dx"])
    if "dr" in trained:
        assert torch.equal(frozen["dr"], trained["dr"])


def test_phydnet_groupnorm_too_many_channels_per_group_raises(vpx):
    """257 channels per group: refused in the wrapper, before any launch."""
    from vp_suite_amd import phy_ops
    x = torch.zeros(1, 257, 2, 2, device="cuda")
    w, b = torch.ones(257, device="cuda"), torch.zeros(257, device="cuda")
    with _spy(vpx._lib.lib(), "vpx_groupnorm_fwd") as calls:
        with pytest.raises(ValueError):
            phy_ops.group_norm(x, 1, w, b)
        with pytest.raises(ValueError):
            phy_ops.group_norm(torch.zeros(1, 514, 2, 2, device="cuda"), 2, torch.ones(514, device="cuda"), torch.zeros(514, device="cuda"))
    assert not calls
