"""The fused training tail against plain float64 (tests/train_tail_ref.py): the decoupling term (`ops.decouple_term`,
`ops.decouple_term_batched`: csrc/pointwise.hip behind the adapter contractions csrc/decouple_api.hip chooses), the MSE value and gradient
(`ops.mse_loss`) and the flat-bucket Adam update (`ops.adam_step`), both csrc/train_tail.hip — at the sizes where their unrolled loops,
remainders, block caps, alignment paths and launch choices change.

Decoupling term. Reference: oracle.torch_ref.decouple_term's expression on the CPU in float64 with autograd, on the same float32 inputs
cast up, under an upstream gradient of 0.37. Bounds (test_single_tile_weight_gradients_with_many_k_slices): value |v - ref| < 1e-5 |ref|,
every gradient max|d| / max|ref| < 2e-5 in f32 and 1e-4 in bf16x3. tests/test_train_tail_host.py holds every case to its conditions on the
CPU: the float32 CPU restatement within a quarter of the f32 bars of fp64 (measured over all shapes and regimes: value 1.6e-7 at worst,
gradients 5.9e-7), min|cos| >= 0.04 in the prescribed regimes and >= 1e-4 in `random` (measured: 1.3e-4 to 4.8e-3 at seed revision 0
everywhere), no row left out. On a one-pixel map the value is 1 (held to 1e-6) and the gradients are exactly 0; the kernel leaves the
rounding residue of two cancelling terms, held to k 2^-24 max|T|, T one of the terms pulled through the adapter's adjoint with its
signs (see test_decouple_one_pixel_map_leaves_rounding_residue_only).

MSE and Adam. The bounds are element-wise and derived from the kernels' operation counts (written next to each), in units of
2^-24; nothing is measured from the kernels. Adam is compared one step at a time: every step's reference starts from the float32 state
the kernel held before it. Its bounds take no credit for cancellation: they are stated against |g gs| + |wd p| in place of the effective
gradient, which is the issue's |v_ref| and |update| wherever the two do not cancel; where they do, the update's count grows from 18 to
13 + 5 V / v_ref, and every Adam bound carries a factor 1 + 2^-18 for the second-order terms (tests/train_tail_ref.py)."""
import contextlib

import numpy as np
import pytest
import torch

import train_tail_ref as R

pytestmark = pytest.mark.gpu

_ids = lambda s: "x".join(map(str, s))
GRADS = ("d_delta_c", "d_delta_m", "d_adapter")
DECOUPLE_CASES = [(s, r, "f32") for s, r in R.decouple_cases() if s[2] * s[3] > 1] + \
                 [(s, r, "bf16x3") for s in R.BF16X3_SHAPES for r in R.REGIME_SCALE]


# ---- shared plumbing -----------------------------------------------------------------------------------------------------------------
def _dev(t):
    """A guarded device copy (torch.empty goes through tests/canary.py)."""
    return torch.empty(tuple(t.shape), device="cuda").copy_(t)


@contextlib.contextmanager
def _deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


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


def _decouple_gpu(vpx, dc, dm, A, prec, need=(True, True, True), upstream=R.UPSTREAM):
    leaves = [_dev(t).requires_grad_(n) for t, n in zip((dc, dm, A), need)]
    v = vpx.ops.decouple_term(*leaves, prec)
    (upstream * v).backward()
    return {"value": v.detach(), **{k: t.grad for k, t in zip(GRADS, leaves)}}


def _check_decouple(parity_log, tag, got, ref, prec, names=GRADS):
    figs = {"value": parity_log(f"{tag}.value", got["value"], ref["value"], R.VALUE_TOL)}
    assert figs["value"] < R.VALUE_TOL, (tag, figs)
    for k in names:
        assert got[k].shape == ref[k].shape
        figs[k] = parity_log(f"{tag}.grad.{k}", got[k], ref[k], R.GRAD_TOL[prec])
        assert figs[k] < R.GRAD_TOL[prec], (tag, k, figs)
    return figs


def _elementwise(parity_log, name, got, ref, bound, k):
    """|got - ref| <= bound element by element; recorded with k 2^-24, the bound as a relative figure."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
    parity_log(name, got, ref, k * R.U)
    over = (got - ref).abs() - bound
    assert float(over.max()) <= 0.0, (name, int((over > 0).sum()), float(((got - ref).abs() / bound.clamp(min=1e-300)).max()))


# ---- decoupling term -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DECOUPLE_CASES, ids=lambda c: f"{_ids(c[0])}-{c[1]}-{c[2]}")
def test_decouple_parity_vs_fp64(vpx, parity_log, case):
    shape, regime, prec = case
    (dc, dm, A), ref, _, base = R.decouple_case(shape, regime)
    got = _decouple_gpu(vpx, dc, dm, A, prec)
    figs = _check_decouple(parity_log, f"decouple.{prec}", got, ref, prec)
    print(f"decouple {shape} {regime} {prec}: seed revision {base} {figs}")


@pytest.mark.parametrize("regime", ["prescribed", "small", "large"])
def test_decouple_one_pixel_map_leaves_rounding_residue_only(vpx, parity_log, regime):
    """HW = 1: |cos| = 1 whatever the inputs, so the reference is the value 1 and the exact zero gradient. Of
    g (y_m / (nc nm) - c y_c / scc) the kernel leaves the roundings of its two equal terms, none of which is credited as shared:
      y_m / (nc nm):  nc, nm = sqrt(fl(y^2)): 1.5 each; their product 1; the quotient 1                       ->  5
      c y_c / scc:    c = fl(y_c y_m) / (nc nm): 1 + 4 + 1 = 6; the product 1; scc 1; the quotient 1           ->  9
    -> 14 roundings of 2^-24 relative to T = g y_m / (|y_c||y_m|), g = 0.37 / (B Ch) (g itself carries three more, relative to the
    residue: nothing at this level); the adapter's adjoint (fp32 sums of Ch terms) and the weight gradient add less than one more:
    k = 15, asserted against the signed A^T T (for the adapter: T_c^T x_c + T_m^T x_m). The same figure against |A|^T |T| — what the
    count bounds rigorously, since the channels' rounding errors need not cancel where the terms do — is recorded beside it."""
    K_RESIDUE = 15
    shape = (3, 5, 1, 1)
    (dc, dm, A), ref, _, _ = R.decouple_case(shape, regime)
    got = _decouple_gpu(vpx, dc, dm, A, "f32")
    err = parity_log("decouple.hw1.value", got["value"], ref["value"], 1e-6)
    assert float(ref["value"]) == 1.0 and err <= 1e-6, err
    T = R.cancelling_terms(dc, dm, A)
    for k in GRADS:
        assert not ref[k].any() and bool(torch.isfinite(got[k]).all())
        # (recorded as T + residue against T: max|residue| / max|T| in the suite's metric)
        Ts = T["signed." + k]
        fig = parity_log(f"decouple.hw1.residue_over_T.{k}", Ts + got[k].cpu().double(), Ts, K_RESIDUE * R.U)
        fig_abs = parity_log(f"decouple.hw1.residue_over_absT.{k}", T[k] + got[k].cpu().double(), T[k], None)
        assert float(got[k].abs().max()) <= K_RESIDUE * R.U * float(Ts.abs().max()), (k, fig / R.U)
        print(f"one-pixel map {regime} {k}: max|grad| = {fig / R.U:.2f} * 2^-24 * max|A^T T| = {fig_abs / R.U:.2f} * 2^-24 * max(|A|^T |T|)")


@pytest.mark.parametrize("prec,shape", [("f32", R.SMALL_SHAPE), ("bf16x3", R.C1_SHAPE)], ids=["f32", "bf16x3-streaming"])
def test_decouple_gradient_subsets(vpx, parity_log, prec, shape):
    """Only delta_c, only delta_m, only the adapter, both deltas under a frozen adapter: each gradient produced holds the bars, the
    others are None. In deterministic mode (no K-split atomics) a subset's gradient has the bits of the all-gradients run wherever the
    same launches produce it: always for the adapter and for the pair of deltas, for a single delta where the pair runs as two
    convolutions anyway (slots not adjacent, no streaming kernel)."""
    (dc, dm, A), ref, _, _ = R.decouple_case(shape, "prescribed")
    subsets = [(True, False, False), (False, True, False), (False, False, True), (True, True, False)]
    with _spy(vpx._lib.lib(), "vpx_decouple_bwd") as calls:
        for need in subsets:
            got = _decouple_gpu(vpx, dc, dm, A, prec, need)
            names = [k for k, n in zip(GRADS, need) if n]
            _check_decouple(parity_log, f"decouple.subset.{''.join('cma'[i] for i in range(3) if need[i])}.{prec}", got, ref, prec, names)
            for k, n in zip(GRADS, need):
                assert (got[k] is not None) == n, (need, k)
    assert len(calls) == len(subsets)
    for args, need in zip(calls, subsets):   # (arguments 4, 5, 6: d_delta_c, d_delta_m, d_adapter)
        assert [args[i] is not None for i in (4, 5, 6)] == list(need)
    with _deterministic():
        full = _decouple_gpu(vpx, dc, dm, A, prec)
        _check_decouple(parity_log, f"decouple.subset.all.deterministic.{prec}", full, ref, prec)
        single_same = R.DECOUPLE_SHAPES[shape] != 0 and shape != R.C1_SHAPE
        for need in subsets:
            got = _decouple_gpu(vpx, dc, dm, A, prec, need)
            assert torch.equal(got["value"], full["value"])
            for k, n in zip(GRADS, need):
                if n and (k == "d_adapter" or need[:2] == (True, True) or single_same):
                    assert torch.equal(got[k], full[k]), (need, k)


def test_decouple_all_zero_sample(vpx, parity_log):
    """delta_c[0] = 0: its rows add 0 to the mean and take no gradient (the reference: sign(0) = 0), everything stays finite."""
    (dc, dm, A), _, _, _ = R.decouple_case(R.SMALL_SHAPE, "prescribed")
    dc2, dm2 = torch.cat([torch.zeros_like(dc), dc]), torch.cat([dm, dm])
    ref = R.decouple_run(dc2, dm2, A)
    for prec in ("f32", "bf16x3"):
        got = _decouple_gpu(vpx, dc2, dm2, A, prec)
        assert all(bool(torch.isfinite(t).all()) for t in got.values())
        _check_decouple(parity_log, f"decouple.zero_sample.{prec}", got, ref, prec)
        assert not got["d_delta_c"][0].any() and not got["d_delta_m"][0].any()


@pytest.mark.parametrize("shape", R.ADJACENT_SHAPES, ids=_ids)
def test_decouple_adjacent_operands_run_as_one_convolution(vpx, parity_log, shape):
    """delta_c | delta_m as the two halves of one channels-last buffer, at shapes whose workspace slots are adjacent too: the forward's
    adapter pair is ONE f32 convolution over 2B images (as are the recomputation and the adjoint in the backward), the weight gradient
    one launch. The operands are used where they lie."""
    assert R.DECOUPLE_SHAPES[shape] == 0
    B = shape[0]
    for regime in ("random", "prescribed"):
        (dc, dm, A), ref, _, _ = R.decouple_case(shape, regime)
        pair = vpx.ops.new_channels_last((2 * B, *shape[1:]), "cuda")
        pair[:B].copy_(dc)
        pair[B:].copy_(dm)
        leaves = [pair[:B].detach().requires_grad_(True), pair[B:].detach().requires_grad_(True), _dev(A).requires_grad_(True)]
        assert leaves[1].data_ptr() == leaves[0].data_ptr() + 4 * dc.numel()
        with _spy(vpx._lib.lib(), "vpx_decouple_fwd") as calls:
            v = vpx.ops.decouple_term(*leaves, "f32")
        assert len(calls) == 1 and calls[0][0].value == leaves[0].data_ptr() and calls[0][1].value == leaves[1].data_ptr()
        (R.UPSTREAM * v).backward()
        got = {"value": v.detach(), **{k: t.grad for k, t in zip(GRADS, leaves)}}
        figs = _check_decouple(parity_log, f"decouple.adjacent.{regime}", got, ref, "f32")
        print(f"adjacent operands {shape} {regime}: {figs}")


@pytest.mark.parametrize("key", list(R.BATCHED))
def test_decouple_batched_slab_vs_fp64(vpx, parity_log, key):
    """`decouple_term_batched` on a [2, K B, Ch, H, W] channels-last slab, the steps' tensors views of their slots: the mean of the K
    per-step terms, every step's two gradients, the adapter's. The slab's delta_c | delta_m halves are adjacent in memory; what the
    library makes of that depends on the workspace slots (R.BATCHED): "f32" two convolutions each way, two weight gradients and the add;
    "f32-joint" one f32 convolution over 2 K B images each way and one weight-gradient launch; "bf16x3" the streaming 1x1 kernel."""
    prec = key.split("-")[0]
    (K, B, Ch, H, W), rem = R.BATCHED[key]
    assert K * B * Ch * H * W % 64 == rem
    steps, A, ref = R.batched_case(key)
    ops = vpx.ops
    slab = ops.new_channels_last((2, K * B, Ch, H, W), "cuda")
    deltas = []
    for k, (c, m) in enumerate(steps):
        slab[0, k * B:(k + 1) * B].copy_(c.cuda())
        slab[1, k * B:(k + 1) * B].copy_(m.cuda())
        deltas += [slab[0, k * B:(k + 1) * B].detach().requires_grad_(True), slab[1, k * B:(k + 1) * B].detach().requires_grad_(True)]
    assert slab[1].data_ptr() == slab[0].data_ptr() + 4 * K * B * Ch * H * W
    Ad = _dev(A).requires_grad_(True)
    v = ops.decouple_term_batched(slab, Ad, prec, K, B, deltas)
    (R.UPSTREAM * v).backward()
    got = {"value": v.detach(), "d_adapter": Ad.grad}
    for k in range(K):
        got[f"d_delta_c{k}"], got[f"d_delta_m{k}"] = deltas[2 * k].grad, deltas[2 * k + 1].grad
    figs = _check_decouple(parity_log, f"decouple.batched.{key}", got, ref, prec, [k for k in ref if k != "value"])
    print(f"batched {key}: {figs}")
    with pytest.raises(ValueError):   # a step's tensor that is not its slot
        ops.decouple_term_batched(slab, Ad, prec, K, B, [deltas[1], deltas[0]] + deltas[2:])


@pytest.mark.parametrize("prec,shape", [("f32", R.SMALL_SHAPE), ("f32", (2, 64, 4, 32)), ("bf16x3", R.C1_SHAPE)], ids=["f32", "f32-adjacent", "bf16x3-streaming"])
def test_decouple_reproducible_in_deterministic_mode(vpx, prec, shape):
    (dc, dm, A), _, _, _ = R.decouple_case(shape, "random")
    with _deterministic():
        a, b = (_decouple_gpu(vpx, dc, dm, A, prec) for _ in range(2))
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- MSE -----------------------------------------------------------------------------------------------------------------------------
def _check_mse(parity_log, ops, tag, pred, target, p_cpu, t_cpu, scale):
    """Loss, the gradient under upstream 1 and — a second backward through the same graph — under upstream 3."""
    pred = pred.requires_grad_(True)
    loss = ops.mse_loss(pred, target, scale)
    (g1,) = torch.autograd.grad(loss, pred, retain_graph=True)
    (g3,) = torch.autograd.grad(loss, pred, torch.tensor(3.0, device="cuda"), retain_graph=True)
    (g3b,) = torch.autograd.grad(loss, pred, torch.tensor(3.0, device="cuda"))
    assert torch.equal(g3, g3b)
    ref_loss, ref_g1 = R.mse_ref(p_cpu, t_cpu, scale)
    _, ref_g3 = R.mse_ref(p_cpu, t_cpu, scale, 3.0)
    # R.MSE_LOSS_K = 4: fl(p - t) once, doubled by the square; double accumulation; one rounding to float
    _elementwise(parity_log, f"{tag}.loss", loss, ref_loss, R.MSE_LOSS_K * R.U * ref_loss.abs(), R.MSE_LOSS_K)
    # R.MSE_GRAD_R = 3 roundings (p - t, gscale, their product), 4 with the upstream product; (r + 1) 2^-24 |ref| element-wise
    _elementwise(parity_log, f"{tag}.grad", g1, ref_g1, (R.MSE_GRAD_R + 1) * R.U * ref_g1.abs(), R.MSE_GRAD_R + 1)
    _elementwise(parity_log, f"{tag}.grad_upstream3", g3, ref_g3, (R.MSE_GRAD_R + 2) * R.U * ref_g3.abs(), R.MSE_GRAD_R + 2)
    return loss.detach(), g1


@pytest.mark.parametrize("shape", R.MSE_SMALL, ids=_ids)
def test_mse_small_sizes_every_regime_and_scale(vpx, parity_log, shape):
    for regime in R.MSE_REGIMES:
        p, t = R.mse_inputs(shape, regime)
        for scale in R.MSE_SCALES:
            loss, g = _check_mse(parity_log, vpx.ops, f"mse.{regime}.{scale:g}", _dev(p), _dev(t), p, t, scale)
            if regime == "identical":
                assert float(loss) == 0.0 and not g.any()


@pytest.mark.parametrize("shape,regime,scale", [(R.MSE_TWO_TRIPS, "uniform", 0.25), (R.MSE_TWO_TRIPS, "offset", 1e3), (R.MSE_FULL_TRIPS, "uniform", 1e3),
                                                (R.MSE_FULL_TRIPS, "identical", 1.0)], ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_mse_past_the_block_cap(vpx, parity_log, shape, regime, scale):
    """More than 1024 blocks' worth of elements: the grid-stride loop makes a second (and third) trip."""
    p, t = R.mse_inputs(shape, regime)
    loss, g = _check_mse(parity_log, vpx.ops, f"mse.{regime}.{scale:g}", _dev(p), _dev(t), p, t, scale)
    if regime == "identical":
        assert float(loss) == 0.0 and not g.any()


@pytest.mark.parametrize("which", ["prediction", "target", "both"])
def test_mse_unaligned_views_take_the_scalar_path(vpx, parity_log, which):
    """Dense views 1, 2 and 3 floats into a larger buffer: not 16-byte aligned, so the kernel may not move four floats at a time."""
    shape = R.MSE_OFFSET_SHAPE
    n = int(np.prod(shape))
    p, t = R.mse_inputs(shape, "uniform")
    for off in (1, 2, 3):
        bufs = [torch.empty(n + 8, device="cuda") for _ in range(2)]
        pd = bufs[0][off:off + n].view(shape).copy_(p) if which != "target" else _dev(p)
        td = bufs[1][off:off + n].view(shape).copy_(t) if which != "prediction" else _dev(t)
        assert (pd.data_ptr() % 16 != 0) == (which != "target") and (td.data_ptr() % 16 != 0) == (which != "prediction")
        with _spy(vpx._lib.lib(), "vpx_mse_loss") as calls:
            _check_mse(parity_log, vpx.ops, f"mse.unaligned.{which}.{off}", pd.detach(), td, p, t, 0.25)
        assert len(calls) == 1 and calls[0][0].value == pd.data_ptr() and calls[0][1].value == td.data_ptr()   # (used in place, no copy)


def test_mse_channels_last_prediction(vpx, parity_log):
    shape = (2, 3, 3, 9, 7)
    p, t = R.mse_inputs(shape, "uniform")
    pd = vpx.ops.to_channels_last(_dev(p).flatten(0, 1)).unflatten(0, shape[:2])
    assert not pd.is_contiguous()
    _check_mse(parity_log, vpx.ops, "mse.channels_last", pd, _dev(t), p, t, 1.0)


def test_mse_value_only_when_prediction_takes_no_gradient(vpx, parity_log):
    for shape in ((3, 7, 3, 9, 7), R.MSE_TWO_TRIPS):
        p, t = R.mse_inputs(shape, "uniform")
        with _spy(vpx._lib.lib(), "vpx_mse_loss") as calls:
            loss = vpx.ops.mse_loss(_dev(p), _dev(t), 0.25)
        assert len(calls) == 1 and calls[0][6] is None and not loss.requires_grad   # (argument 6: dpred)
        ref_loss, _ = R.mse_ref(p, t, 0.25)
        _elementwise(parity_log, "mse.value_only.loss", loss, ref_loss, R.MSE_LOSS_K * R.U * ref_loss.abs(), R.MSE_LOSS_K)   # as in _check_mse


def test_mse_refusals(vpx):
    z = lambda *s: torch.zeros(*s, device="cuda")
    with _spy(vpx._lib.lib(), "vpx_mse_loss") as calls:
        with pytest.raises(ValueError, match="expects 5-D inputs"):
            vpx.ops.mse_loss(z(2, 3, 4, 5), z(2, 3, 4, 5))
        with pytest.raises(ValueError, match="different shape"):
            vpx.ops.mse_loss(z(2, 3, 1, 4, 5), z(2, 3, 1, 4, 6))
    assert not calls


# ---- flat Adam -----------------------------------------------------------------------------------------------------------------------
def _adam_step(parity_log, ops, tag, state, g, step, **kw):
    """One step of the kernel on device copies of the float32 `state` = (p, m, v), held element-wise to R.adam_ref's bounds (K_M = 6,
    K_V = 10, K_P = 18 roundings of 2^-24: counted in tests/train_tail_ref.py); returns the kernel's new float32 state."""
    p, m, v = state
    dp, dg, dm, dv = (_dev(t) for t in (p, g, m, v))
    ops.adam_step(dp, dg, dm, dv, step, R.LR, **kw)
    assert torch.equal(dg.cpu(), g)
    (p2, m2, v2), (bp, bm, bv) = R.adam_ref(p, g, m, v, step, **kw)
    _elementwise(parity_log, f"{tag}.step{step}.m", dm, m2, bm, R.K_M)      # |dm| <= K_M 2^-24 (|b1 m| + |(1 - b1) g|)
    _elementwise(parity_log, f"{tag}.step{step}.v", dv, v2, bv, R.K_V)      # |dv| <= K_V 2^-24 |v_ref|
    _elementwise(parity_log, f"{tag}.step{step}.p", dp, p2, bp, R.K_P)      # |dp| <= 2^-24 |p_ref| + K_P 2^-24 |update|
    return dp.cpu(), dm.cpu(), dv.cpu()


def _adam_run(parity_log, ops, n, tag, zero_steps=(1, 2, 3), late_steps=(1000, 100_000), **kw):
    p, g, m, v = R.adam_state(n, tag, zero_state=True)
    state = (p, m, v)
    for step in zero_steps:
        g = R.adam_state(n, f"{tag}.g{step}", zero_state=True)[1]
        state = _adam_step(parity_log, ops, f"adam.{tag}", state, g, step, **kw)
    for step in late_steps:
        p, g, m, v = R.adam_state(n, f"{tag}.late{step}", zero_state=False)
        assert float(v.min()) >= 0.0
        _adam_step(parity_log, ops, f"adam.{tag}", (p, m, v), g, step, **kw)


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_sizes_vs_fp64(vpx, parity_log, n):
    """Below one vector, around one block, an odd tail, past the cap of 2048 blocks — defaults, and weight_decay = 0.01."""
    capped = n == R.ADAM_CAPPED
    for wd in ((0.01,) if capped else (0.0, 0.01)):
        _adam_run(parity_log, vpx.ops, n, f"n{n}.wd{wd:g}", zero_steps=(1, 2) if capped else (1, 2, 3), late_steps=() if capped else (1000,),
                  weight_decay=wd)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=lambda b: f"b{b[0]:g}-{b[1]:g}")
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_every_setting_at_1025(vpx, parity_log, wd, betas):
    for gs in (1.0, 0.5):
        for eps in (1e-8, 1e-3):
            _adam_run(parity_log, vpx.ops, R.ADAM_ALL_SETTINGS_N, f"wd{wd:g}.b{betas[0]:g}.gs{gs:g}.eps{eps:g}", weight_decay=wd, betas=betas,
                      grad_scale=gs, eps=eps)


def test_adam_zero_gradient_on_zero_state_moves_nothing(vpx):
    """g = 0 on m = v = 0 without weight decay: 0 / (0 + eps), the parameter keeps its bits and no NaN appears — in the vector path and
    in the tail."""
    n = 1027
    p, g, m, v = R.adam_state(n, "zero_block", zero_state=False)
    idle = torch.zeros(n, dtype=torch.bool)
    idle[256:777] = True
    idle[-3:] = True
    g[idle], m[idle], v[idle] = 0.0, 0.0, 0.0
    for eps in (1e-8, 1e-3):
        dp, dg, dm, dv = (_dev(t) for t in (p, g, m, v))
        vpx.ops.adam_step(dp, dg, dm, dv, 5, R.LR, eps=eps)
        for t in (dp, dm, dv):
            assert bool(torch.isfinite(t).all())
        assert torch.equal(dp.cpu()[idle], p[idle]) and not dm.cpu()[idle].any() and not dv.cpu()[idle].any()
        assert not torch.equal(dp.cpu()[~idle], p[~idle])


def test_adam_refusals_leave_the_buckets_unchanged(vpx):
    n = 1024
    p, g, m, v = R.adam_state(n + 1, "refusals", zero_state=False)
    bufs = [_dev(t) for t in (p, g, m, v)]
    before = [t.clone() for t in bufs]
    with _spy(vpx._lib.lib(), "vpx_adam_step") as calls:
        with pytest.raises(vpx._lib.VpxError):   # a view at an odd float offset
            vpx.ops.adam_step(bufs[0][1:], bufs[1][1:], bufs[2][1:], bufs[3][1:], 1, R.LR)
        with pytest.raises(vpx._lib.VpxError):   # ... of one bucket alone
            vpx.ops.adam_step(bufs[0][:n], bufs[1][:n], bufs[2][1:], bufs[3][:n], 1, R.LR)
        assert not calls
        with pytest.raises(ValueError):   # not contiguous
            vpx.ops.adam_step(bufs[0][::2], bufs[1][::2], bufs[2][::2], bufs[3][::2], 1, R.LR)
        with pytest.raises(vpx._lib.VpxError):
            vpx.ops.adam_step(*bufs, 0, R.LR)
        assert not calls
    for t, b in zip(bufs, before):
        assert torch.equal(t, b)
