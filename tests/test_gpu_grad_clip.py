"""Gradient clipping and the non-finite step guard fused into the flat Adam update (csrc/train_tail.hip: grad_stats_*_kernel,
adam_kernel<1|2>; `ops.grad_stats`, `ops.adam_step_clipped`, `train.FlatAdam(max_grad_norm=, clip_grad_value=, skip_nonfinite=)`,
`train.DataParallelTrainer(...)`) against tests/clip_ref.py, which tests/test_grad_clip_host.py pins against torch on the CPU.

Statistics: max and non-finite count exact; the norm within (n + 4) 2^-53 relative, counted from the roundings (see _check_stats).
Update: the bounds of test_flat_adam_kernel_vs_oracle_and_torch (|dp| < 3e-7, relmax m, v < 1e-6 against oracle.torch_ref.adam_step_ref)
widened by the ONE rounding this change adds — the factor s = (float)(grad_scale c) — and none for the clamp (see _check_update).
Where clipping does nothing (c = 1, no clamp, nothing skipped) the three buckets have the bits `ops.adam_step` leaves."""
import functools

import numpy as np
import pytest
import torch

import clip_ref as C
import golden_cases as gc
from golden_util import name_seed, seeded_rand, seeded_randn

pytestmark = pytest.mark.gpu

LR, B1, B2 = 1e-3, 0.9, 0.999
GS_MAX_BLOCKS = C.kernel_constant("GS_MAX_BLOCKS")
GS_BLOCK_ELEMS = C.kernel_constant("GS_THREADS") * 4
N_TWO_TRIPS = GS_MAX_BLOCKS * GS_BLOCK_ELEMS + 1027        # past the block cap: a second grid-stride trip that ends on the scalar tail
STATS_SIZES = (1, 3, 4, 5, 1023, 100_003, N_TWO_TRIPS)
SCALES = (1.0, 0.5, 1.0 / 3.0)


def _dev(t):
    """A guarded device copy (torch.empty goes through tests/canary.py)."""
    t = torch.from_numpy(np.array(t)) if isinstance(t, np.ndarray) else t   # (a copy: the shared gradients are read-only arrays)
    return torch.empty(tuple(t.shape), dtype=t.dtype, device="cuda").copy_(t)


@functools.lru_cache(maxsize=None)
def _grad(n, tag="g"):
    """float32 gradient of n elements, magnitudes from 1e-2 to 1e1 (read-only: shared between the tests)."""
    seed = name_seed(f"clip.{tag}.{n}")
    g = (seeded_randn((n,), seed) * 10.0 ** (-2.0 + 3.0 * seeded_rand((n,), seed + 1))).numpy()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _stats_ref(n, tag, scale):
    return C.grad_stats_ref(_grad(n, tag), scale)


def _check_stats(parity_log, name, got, ref, n):
    """got: the kernel's float64[4] on the host. Max and count are exact: |g| of a float is exact, the scale's product with the maximum
    is the one rounding both sides make (rounding is monotone: max fl(s |g_i|) = fl(s max |g_i|)), the count is an integer.
    Norm: the squares are exact in double on both sides. Kernel: n - 1 additions of non-negative terms in whatever order, each
    within 2^-53 relative -> the sum within (n - 1) 2^-53; grad_scale^2 and its product with the sum: 2 more; the square root halves
    the relative error and rounds once: ((n + 1) / 2 + 1) 2^-53. Reference (clip_ref.grad_stats_ref): math.fsum rounds once, the same
    2 + sqrt: (3 / 2 + 1) 2^-53. Together n / 2 + 4 <= n + 4 roundings of 2^-53 relative."""
    assert got[2] == ref[2] and got[1] == ref[1], (name, got, ref)
    if ref[2] > 0:
        assert not np.isfinite(got[0]), (name, got)
        return
    assert np.isfinite(got[0])
    fig = parity_log(f"{name}.norm", got[:1], ref[:1], (n + 4) * C.U53)
    assert abs(got[0] - ref[0]) <= (n + 4) * C.U53 * ref[0], (name, fig / C.U53)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STATS_SIZES)
def test_grad_stats_sizes_and_scales_vs_fp64(vpx, parity_log, n):
    g = _dev(_grad(n))
    assert g.data_ptr() % 16 == 0
    out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    for scale in SCALES:
        ret = vpx.ops.grad_stats(g, scale, out=out)
        assert ret is out
        got = out.cpu().numpy()
        assert got[3] == -7.0                                    # (the skipped-step count is not this kernel's)
        _check_stats(parity_log, f"stats.n{n}.s{scale:.3g}", got, _stats_ref(n, "g", scale), n)
    fresh = vpx.ops.grad_stats(g, 0.5)
    assert fresh.dtype == torch.float64 and fresh.shape == (4,) and float(fresh[3]) == 0.0
    assert torch.equal(fresh, vpx.ops.grad_stats(g, 0.5))     # two runs: the same bits


@pytest.mark.parametrize("n", [5, 1023, 100_003, N_TWO_TRIPS])
def test_grad_stats_unaligned_view_takes_the_scalar_path(vpx, parity_log, n):
    buf = torch.empty(n + 8, device="cuda")
    g = buf[1:n + 1].copy_(torch.from_numpy(_grad(n)))
    assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    a = vpx.ops.grad_stats(g, 1.0 / 3.0)
    _check_stats(parity_log, f"stats.unaligned.n{n}", a.cpu().numpy(), _stats_ref(n, "g", 1.0 / 3.0), n)
    assert torch.equal(a, vpx.ops.grad_stats(g, 1.0 / 3.0))


@pytest.mark.parametrize("lo,hi", [(-20.0, 18.5), (-25.0, -23.0), (15.0, 18.5)], ids=["1e-20..3e18", "tiny", "huge"])
def test_grad_stats_beyond_the_float_range_of_the_squares(vpx, parity_log, lo, hi):
    """Squares from 1e-50 to 1e37 and their sum: float32 flushes the small ones to zero and overflows on the sum of the large ones."""
    n = 100_003
    seed = name_seed(f"clip.range.{lo}.{hi}")
    g = (torch.sign(seeded_randn((n,), seed)) * 10.0 ** (lo + (hi - lo) * seeded_rand((n,), seed + 1).double())).float().numpy()
    with np.errstate(all="ignore"):
        sq32 = g.astype(np.float32) ** 2
    with np.errstate(all="ignore"):
        assert (hi < 0 and not sq32.any()) or (hi > 0 and not np.isfinite(sq32.sum(dtype=np.float32)))
    ref = C.grad_stats_ref(g, 0.5)
    assert np.isfinite(ref[0]) and ref[0] > 0.0
    _check_stats(parity_log, f"stats.range.{lo:g}.{hi:g}", vpx.ops.grad_stats(_dev(g), 0.5).cpu().numpy(), ref, n)


def test_grad_stats_counts_non_finite_elements(vpx, parity_log):
    n = 5000
    for vec in (True, False):
        for bad in ({n - 1: np.nan}, {0: np.inf}, {0: -np.inf, 1: np.nan, 2047: np.inf, n - 1: np.nan}):
            g = _grad(n).copy()
            for i, val in bad.items():
                g[i] = val
            d = _dev(g) if vec else torch.empty(n + 8, device="cuda")[1:n + 1].copy_(torch.from_numpy(g))
            got = vpx.ops.grad_stats(d, 0.5).cpu().numpy()
            assert got[2] == len(bad)
            _check_stats(parity_log, "stats.nonfinite", got, C.grad_stats_ref(g, 0.5), n)
    only = vpx.ops.grad_stats(_dev(np.full(7, np.nan, dtype=np.float32))).cpu().numpy()
    assert np.isnan(only[0]) and only[1] == 0.0 and only[2] == 7


def test_grad_stats_refusals(vpx):
    g = torch.zeros(16, device="cuda")
    with pytest.raises(ValueError):
        vpx.ops.grad_stats(g[::2])
    with pytest.raises(ValueError):
        vpx.ops.grad_stats(g, -1.0)
    with pytest.raises(ValueError):
        vpx.ops.grad_stats(g, float("nan"))
    with pytest.raises(ValueError):
        vpx.ops.grad_stats(g, out=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        vpx.ops.grad_stats(g.double())


# ---- update --------------------------------------------------------------------------------------------------------------------------
def _check_update(parity_log, name, got, ref, before, ge):
    """got / ref / before: (p, m, v) after the kernel, after clip_ref.adam_clipped_ref, and before the step (numpy); ge: the reference's
    clipped gradient. The bounds of test_flat_adam_kernel_vs_oracle_and_torch, widened by the one rounding added: the kernel multiplies
    by (float)(grad_scale c) where the reference multiplies by the double — 2^-24 relative on every g. That is 2^-24 on the gradient
    term (1 - b1) g of m, 2 * 2^-24 on the term (1 - b2) g^2 of v, and on the update at most 2^-24 through m plus 2^-24 through
    sqrt(v) (half of v's two): 2 * 2^-24 |update|. The clamp adds nothing: min / max round nothing and move two values no further apart."""
    (p, m, v), (rp, rm, rv) = got, ref
    finite = np.isfinite(rp)
    assert np.array_equal(np.isfinite(p), finite) and np.array_equal(np.isfinite(m), np.isfinite(rm)) and np.array_equal(np.isfinite(v), np.isfinite(rv))
    if not finite.any():
        return
    p, m, v, rp, rm, rv, ge = (np.where(finite, t, 0.0).astype(np.float64) for t in (p, m, v, rp, rm, rv, ge))
    upd = np.abs(rp - np.where(finite, before[0], 0.0))
    bp = 3e-7 + 2 * C.U24 * float(upd.max())
    bm = 1e-6 + C.U24 * float(np.abs((1 - B1) * ge).max()) / float(np.abs(rm).max())
    bv = 1e-6 + 2 * C.U24 * float(((1 - B2) * ge * ge).max()) / float(np.abs(rv).max())
    parity_log(f"{name}.p", p, rp, None)
    assert float(np.abs(p - rp).max()) < bp, (name, float(np.abs(p - rp).max()), bp)
    assert parity_log(f"{name}.m", m, rm, bm) < bm and parity_log(f"{name}.v", v, rv, bv) < bv, name


@functools.lru_cache(maxsize=None)
def _settings(n):
    """max_norm / clip_value of the four settings, chosen from the reference's statistics of the three gradients (never from a kernel):
    (a) half the smallest norm, (b) a thousand times the largest, (c) the 0.9 quantile of |grad_scale g| of step 1, (d) (a) with the
    same quantile of the norm-clipped gradient. The clamp values are rounded to float32, what the kernel compares with."""
    norms = [float(C.grad_stats_ref(_grad(n, f"u{s}"), 0.5)[0]) for s in (1, 2, 3)]
    a = 0.5 * min(norms)
    q = float(np.float32(np.quantile(np.abs(_grad(n, "u1").astype(np.float64) * 0.5), 0.9)))
    qd = float(np.float32(q * C.clip_coefficient(norms[0], a)))
    return {"a": dict(max_norm=a), "b": dict(max_norm=1e3 * max(norms)), "c": dict(clip_value=q), "d": dict(max_norm=a, clip_value=qd)}


@pytest.mark.parametrize("setting", ["a", "b", "c", "d"])
@pytest.mark.parametrize("n", [100_003, 5])
def test_adam_clipped_three_steps_vs_reference(vpx, parity_log, n, setting):
    ops, kw = vpx.ops, _settings(n)[setting]
    p = seeded_randn((n,), name_seed(f"clip.p.{n}")).numpy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    dp, dm, dv = _dev(p), _dev(m), _dev(v)
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    for step in (1, 2, 3):
        g = _grad(n, f"u{step}")
        dg = _dev(g)
        before = (p, m, v)
        p, m, v, info = C.adam_clipped_ref(p, g, m, v, step, LR, grad_scale=0.5, **kw)
        if "max_norm" in kw:
            assert (info["c"] < 1.0) == (setting != "b") and (setting == "b" or info["c"] <= 0.5 + 1e-6)   # (a), (d): really clipping
        if "clip_value" in kw and n > 5:       # about a tenth of the elements, in every step
            assert 0.05 < info["clamped"] < 0.15, info["clamped"]
        elif "clip_value" in kw and step == 1:   # five elements: the largest of step 1 (the quantile lies between it and the next)
            assert info["clamped"] == 0.2
        use_stats = ops.grad_stats(dg, 0.5, out=stats) if "max_norm" in kw else None
        ops.adam_step_clipped(dp, dg, dm, dv, step, LR, grad_scale=0.5, stats=use_stats, **kw)
        assert torch.equal(dg.cpu(), torch.from_numpy(g))
        ge = C.clipped_gradient(g, 0.5, kw.get("max_norm", 0.0), kw.get("clip_value", 0.0))[0]
        _check_update(parity_log, f"clipped.{setting}.n{n}.step{step}", tuple(t.cpu().numpy() for t in (dp, dm, dv)), (p, m, v), before, ge)
    assert float(stats[3]) == 0.0


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [100_003, 5])
def test_adam_clipped_without_effect_has_the_bits_of_adam_step(vpx, n, wd):
    """c = 1 (max_norm far above the norm), or nothing asked for at all: s == (float)grad_scale, and param / exp_avg / exp_avg_sq come out
    bit for bit as from ops.adam_step — three steps on the same inputs, with and without weight decay, with and without statistics."""
    ops = vpx.ops
    p0 = seeded_randn((n,), name_seed(f"clip.p.{n}"))
    runs = {"plain": None, "far": dict(max_norm=_settings(n)["b"]["max_norm"]), "far+guard": dict(max_norm=_settings(n)["b"]["max_norm"], skip_nonfinite=True),
            "off": dict(), "off+stats": dict(stats=True)}
    out = {}
    for key, kw in runs.items():
        dp, dm, dv = _dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        for step in (1, 2, 3):
            dg = _dev(_grad(n, f"u{step}"))
            if kw is None:
                ops.adam_step(dp, dg, dm, dv, step, LR, weight_decay=wd, grad_scale=0.5)
            else:
                kw2 = {k: val for k, val in kw.items() if k != "stats"}
                stats = ops.grad_stats(dg, 0.5) if (kw.get("stats") or "max_norm" in kw) else None
                ops.adam_step_clipped(dp, dg, dm, dv, step, LR, weight_decay=wd, grad_scale=0.5, stats=stats, **kw2)
        out[key] = (dp, dm, dv)
    assert not torch.equal(out["plain"][0].cpu(), p0)
    for key in runs:
        for a, b in zip(out[key], out["plain"]):
            assert torch.equal(a, b), key


def test_adam_clipped_refusals_leave_the_buckets_unchanged(vpx):
    n = 1024
    bufs = [_dev(seeded_randn((n + 1,), name_seed(f"clip.refusal.{i}")).abs()) for i in range(4)]
    before = [t.clone() for t in bufs]
    stats = vpx.ops.grad_stats(bufs[1])
    E = vpx._lib.VpxError
    for exc, args, kw in ((E, [t[1:] for t in bufs], dict(clip_value=1.0)), (E, bufs, dict(clip_value=1.0, step=0)),
                          (ValueError, [t[::2] for t in bufs], dict(clip_value=1.0)), (ValueError, bufs, dict(max_norm=1.0)),
                          (ValueError, bufs, dict(skip_nonfinite=True)), (ValueError, bufs, dict(max_norm=-1.0, stats=stats)),
                          (ValueError, bufs, dict(clip_value=float("nan"))), (ValueError, bufs, dict(grad_scale=-1.0, clip_value=1.0)),
                          (ValueError, bufs, dict(max_norm=1.0, stats=stats.float())), (ValueError, bufs, dict(max_norm=1.0, stats=stats[:3]))):
        kw = dict(kw)
        with pytest.raises(exc):
            vpx.ops.adam_step_clipped(*args, kw.pop("step", 1), LR, **kw)
    for t, b in zip(bufs, before):
        assert torch.equal(t, b)


# ---- guard ---------------------------------------------------------------------------------------------------------------------------
def _poisoned(n, where):
    g = _grad(n, "guard.bad").copy()
    if where == "nan_last":
        g[-1] = np.nan        # (n % 4 = 3: the scalar tail of both kernels)
    else:
        g[0] = np.inf
    return g


@pytest.mark.parametrize("where", ["nan_last", "inf_first"])
def test_skip_nonfinite_leaves_the_buckets_alone_and_counts(vpx, parity_log, where):
    """Non-finite NUMBERS through plain arithmetic. bad, clean, bad: the buckets keep their bits over a bad step, stats[3] goes 0 -> 1 ->
    1 -> 2, and the clean step in between runs with the ADVANCED step count (2): held to the reference called with that count."""
    n, ops = 1027, vpx.ops
    seed = name_seed("clip.guard.state")
    state = tuple(t.numpy() for t in (seeded_randn((n,), seed), 0.1 * seeded_randn((n,), seed + 1), (0.1 * seeded_randn((n,), seed + 2)).pow(2)))
    dp, dm, dv = (_dev(t) for t in state)
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    bad, clean = _poisoned(n, where), _grad(n, "guard.clean")
    max_norm = 0.5 * float(C.grad_stats_ref(clean, 0.5)[0])
    kw = dict(grad_scale=0.5, max_norm=max_norm, clip_value=0.0, skip_nonfinite=True)

    def step(g, k):
        dg = _dev(g)
        ops.adam_step_clipped(dp, dg, dm, dv, k, LR, stats=ops.grad_stats(dg, 0.5, out=stats), **kw)
        return stats.cpu().numpy()

    s = step(bad, 1)
    _check_stats(parity_log, "guard.stats", s, C.grad_stats_ref(bad, 0.5), n)
    assert s[2] == 1 and s[3] == 1
    assert all(torch.equal(d.cpu(), torch.from_numpy(t)) for d, t in zip((dp, dm, dv), state))
    s = step(clean, 2)
    assert s[2] == 0 and s[3] == 1
    rp, rm, rv, info = C.adam_clipped_ref(*[state[0], clean, state[1], state[2]], 2, LR, **kw)
    assert info["c"] < 1.0 and not info["skipped"]
    ge = C.clipped_gradient(clean, 0.5, max_norm)[0]
    _check_update(parity_log, f"guard.{where}.clean_step", tuple(t.cpu().numpy() for t in (dp, dm, dv)), (rp, rm, rv), state, ge)
    wrong = C.adam_clipped_ref(*[state[0], clean, state[1], state[2]], 1, LR, **kw)[0]   # (the count held back: told apart)
    assert float(np.abs(wrong - rp).max()) > 1e-5
    after = tuple(t.clone() for t in (dp, dm, dv))
    s = step(bad, 3)
    assert s[2] == 1 and s[3] == 2
    assert all(torch.equal(a, b) for a, b in zip((dp, dm, dv), after))
    # the guard without norm clipping, and with the clamp: the same
    for extra in (dict(max_norm=0.0), dict(clip_value=0.25)):
        kw2 = {**kw, **extra}
        dg = _dev(bad)
        ops.adam_step_clipped(dp, dg, dm, dv, 4, LR, stats=ops.grad_stats(dg, 0.5, out=stats), **kw2)
    assert float(stats[3]) == 4.0 and all(torch.equal(a, b) for a, b in zip((dp, dm, dv), after))


@pytest.mark.parametrize("where", ["nan_last", "inf_first"])
def test_without_the_guard_nan_reaches_the_parameters_as_in_torch(vpx, parity_log, where):
    """clip_grad_norm_ with a NaN norm multiplies every gradient by NaN, with an infinite norm by 0 (inf * 0 = NaN at the element itself);
    clip_grad_value_ alone keeps the NaN where it is, an inf is clamped. The kernel does the same (clip_ref: pinned against torch)."""
    n, ops = 1027, vpx.ops
    seed = name_seed("clip.guard.state")
    state = tuple(t.numpy() for t in (seeded_randn((n,), seed), 0.1 * seeded_randn((n,), seed + 1), (0.1 * seeded_randn((n,), seed + 2)).pow(2)))
    bad = _poisoned(n, where)
    for kw in (dict(max_norm=1.0), dict(clip_value=0.25), dict(max_norm=1.0, clip_value=0.25)):
        dp, dm, dv = (_dev(t) for t in state)
        dg = _dev(bad)
        stats = ops.grad_stats(dg, 0.5)
        ops.adam_step_clipped(dp, dg, dm, dv, 1, LR, grad_scale=0.5, stats=stats, **kw)
        rp, rm, rv, info = C.adam_clipped_ref(state[0], bad, state[1], state[2], 1, LR, grad_scale=0.5, **kw)
        got = tuple(t.cpu().numpy() for t in (dp, dm, dv))
        if where == "nan_last":
            assert np.isnan(got[0][-1]) and (np.isnan(got[0]).all() if "max_norm" in kw else np.isnan(got[0]).sum() == 1)
        elif "max_norm" in kw:
            assert np.isnan(got[0][0]) and np.isnan(got[0]).sum() == 1
        else:
            assert np.isfinite(got[0]).all()
        assert float(stats[3]) == 0.0
        ge = C.clipped_gradient(bad, 0.5, kw.get("max_norm", 0.0), kw.get("clip_value", 0.0))[0]
        _check_update(parity_log, f"noguard.{where}", got, (rp, rm, rv), state, np.where(np.isfinite(ge), ge, 0.0))


# ---- optimizer -----------------------------------------------------------------------------------------------------------------------
def _flat(m):
    named = dict(m.named_parameters())
    return torch.cat([named[k].detach().reshape(-1) for k in sorted(named)]).cpu().numpy()


def _tiny_batch():
    kw, B, T, P = gc.EF_TINY_KW, 2, 3, 2
    c, h, w = kw["img_shape"]
    frames = seeded_rand((B, T + P, c, h, w), name_seed("ef.tiny.frames")).cuda()
    return frames, T, P


def _torch_clipped_run(vpx, max_norm=None, clip_value=None, steps=3):
    """The same model under torch.optim.Adam with clip_grad_norm_ / clip_grad_value_ in a hand-written loop on the GPU (train_iter's
    order: loss, zero_grad, backward, clip, step). Returns the parameters, the norms clip_grad_norm_ reported, step 1's gradient."""
    from test_gpu_models import _ef
    from vp_suite_amd.measure import PredictionLossProvider
    frames, T, P = _tiny_batch()
    m = _ef(vpx, "tiny", gc.EF_TINY_KW)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3)
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    norms, first = [], None
    for _ in range(steps):
        total = m.training_loss(frames[:, :T], frames[:, T:], P, lp, actions=torch.zeros(2, T + P - 1, 0, device="cuda"))
        opt.zero_grad()
        total.backward()
        if first is None:
            first = torch.cat([p.grad.reshape(-1) for p in params]).abs().cpu().numpy()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm if max_norm else float("inf"))))
        if clip_value:
            torch.nn.utils.clip_grad_value_(params, clip_value)
        opt.step()
    return _flat(m), norms, first


@pytest.mark.parametrize("which", ["max_grad_norm", "clip_grad_value"])
def test_flat_adam_clips_inside_train_iter_like_torch(vpx, parity_log, which):
    from test_gpu_models import _ef
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.train import FlatAdam
    _, norms0, first = _torch_clipped_run(vpx)
    if which == "max_grad_norm":
        kw = {which: 0.5 * min(norms0)}                       # half the smallest norm of the unclipped run
        want, norms, _ = _torch_clipped_run(vpx, max_norm=kw[which])
        assert all(nrm > kw[which] for nrm in norms)          # every step is clipped
    else:
        kw = {which: float(np.quantile(first, 0.9))}          # clamps about a tenth of step 1's gradient
        want, norms, _ = _torch_clipped_run(vpx, clip_value=kw[which])
    frames, T, P = _tiny_batch()
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    cfg = {"device": "cuda", "context_frames": T, "pred_frames": P, "val_rec_criterion": "mse"}
    data = {"frames": frames, "actions": torch.zeros(2, T + P - 1, 0)}
    m = _ef(vpx, "tiny", gc.EF_TINY_KW)
    opt = FlatAdam.from_module(m, lr=1e-3, **kw)
    seen = []
    for _ in range(3):
        m.train_iter(cfg, [data], opt, lp, epoch=0)
        seen.append(opt.last_grad_norm)
    got = _flat(m)
    parity_log(f"flat_adam.{which}.params_after3", got, want, None)
    assert np.abs(got - want).max() < 2e-5                    # (test_flat_adam_drives_train_iter_like_torch_adam's bound for the unclipped pair)
    assert opt.skipped_steps == 0 and opt.steps == 3
    if which == "max_grad_norm":
        # step 1 starts from the same parameters: the two norms differ by float32 summation order only; later steps start from
        # parameters that agree to 2e-5, compared above — their norms are only held to belong to the same trajectory
        assert abs(seen[0] - norms[0]) < 1e-5 * norms[0] and all(abs(a - b) < 1e-2 * b for a, b in zip(seen, norms)), (seen, norms)
        # one more step with host synchronisation forbidden: the optimizer reads the statistics on the device only
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        norm = float(opt.flat_grad.double().pow(2).sum().sqrt())
        assert abs(float(opt.grad_stats[0]) - norm) < 1e-12 * norm and opt.last_grad_norm == float(opt.grad_stats[0])
        assert float(opt.grad_stats[1]) == float(opt.flat_grad.abs().max()) and float(opt.grad_stats[2]) == 0.0
    else:
        assert seen == [0.0] * 3                              # value clipping alone runs no reduction


def test_dp_trainer_clips_the_averaged_gradient(vpx, parity_log):
    """World-2 arithmetic on one device: the injected all-reduce doubles the bucket (two ranks with the same shard), grad_scale = 1/2
    is folded into the update — and into the statistics: the norm is the averaged gradient's, and two steps match the single-process
    torch run clipped at the same max_grad_norm."""
    from test_gpu_models import _ef
    from vp_suite_amd.train import DataParallelTrainer
    _, norms0, _ = _torch_clipped_run(vpx, steps=2)
    max_norm = 0.5 * min(norms0)
    want, norms, _ = _torch_clipped_run(vpx, max_norm=max_norm, steps=2)
    assert all(nrm > max_norm for nrm in norms)
    frames, T, P = _tiny_batch()
    m = _ef(vpx, "tiny", gc.EF_TINY_KW)

    def doubling(t):
        t.mul_(2.0)

    tr = DataParallelTrainer(m, lr=1e-3, world_size=2, all_reduce=doubling, broadcast=lambda t, src: None, max_grad_norm=max_norm,
                             skip_nonfinite=True)
    assert tr.fused and tr.collectives
    for k in range(2):
        tr.step(frames[:, :T], frames[:, T:], P)
        assert tr.optimizer.grad_scale == 0.5
        avg = float((0.5 * tr.flat_grad.double()).pow(2).sum().sqrt())
        assert abs(tr.optimizer.last_grad_norm - avg) < 1e-12 * avg and abs(avg - norms[k]) < (1e-5, 1e-2)[k] * norms[k], (k, avg, norms[k])
    got = _flat(m)
    parity_log("dp.max_grad_norm.params_after2", got, want, None)
    assert np.abs(got - want).max() < 2e-5
    assert tr.optimizer.skipped_steps == 0
