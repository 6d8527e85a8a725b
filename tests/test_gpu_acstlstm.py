"""The action-conditional ST-LSTM cell (csrc/acst.hip: vpx_acstlstm_step_fwd / _bwd through `ops.acstlstm_step`) against an fp64
restatement, across the shapes at which its launches change path, both operand modes, both K-split settings, missing incoming gradients,
`forget_bias`, two chained steps and input layouts.

Reference: `oracle.torch_ref.acstlstm_cell` on the CPU in float64 with autograd, on the same float32 inputs and parameters cast up.
Bounds, in the suite's metric max|Δ| / max|ref|: f32 outputs 1e-5, gradients 5e-5 (the two golden tests of this cell); bf16x3 outputs
1e-4 (`test_action_conditional_cell_inference_and_frozen_parameters`), gradients 2e-4 (`test_random_stlstm_steps_vs_oracle`); plain bf16
outputs 3e-2, forward only (`test_convlstm_shi_at_bench_batch_vs_oracle`). The cell has no kinks (sigmoid, tanh, products): no element
is left out of any comparison. A gradient that the loss does not reach (conv_o / conv_last under a loss on c_new and delta_m alone) has
the exact zero for its reference, which the metric holds the kernel to bit for bit.

Input condition: every case first holds the same restatement run in float32 on the CPU to half the f32 bars against fp64 (outputs 5e-6,
gradients 2.5e-5): the inputs are well enough conditioned to judge a kernel by. `host_conditions()` asserts it for every case of every
test without touching the GPU.

Inputs (`seeded_randn`): weights randn / sqrt(fan_in), biases 0.1 randn, LayerNorm weight 1 + 0.3 randn and bias 0.3 randn ([C,H,W]),
x ~ randn, h, c, m, a ~ 0.5 randn, incoming gradients ~ randn."""
import contextlib
import functools

import pytest
import torch

from golden_util import fan_in_scale, name_seed, seeded_randn
from oracle import torch_ref

pytestmark = pytest.mark.gpu

TOL = {"f32": (1e-5, 5e-5), "bf16x3": (1e-4, 2e-4)}   # (outputs, gradients)
COND = (5e-6, 2.5e-5)                                 # the fp32 CPU restatement against fp64: half the f32 bars
BF16_FWD_TOL = 3e-2

# (Cin, Ch, H, W, k, layer_norm, B). Pixel tiles are 8 x 16 (TILE_H x TILE_W). A convolution with Co outputs runs plain_groups(Co) = ng
# groups of 32 channels per N tile (the ng of 4..1 that minimises tiles * (2 + ng), ties to the wider): 56 -> one 64-wide tile, 140 ->
# two 96-wide, 144 -> two 96-wide, 252 -> two 128-wide, 448 -> four 128-wide, 130 -> two 96-wide. A weight gradient with Co rows over C
# activation channels has ceil(Co / 64) row tiles and, from wgrad_make_ctiles, ceil(C / 32) column halves paired into 64-wide column
# tiles. The contraction runs in channel stages of 8 .. 64 channels (pick_stage_channels). Every case has fewer than 256 workgroups per
# convolution, so pick_ksplit splits K over float atomics, into at most as many ranges as a layer has stages, wherever a layer has more
# than one, unless deterministic mode is on (then it returns 1: the unsplit path the B = 128 workload takes).
CASES = {
    # 2 x 2 pixel tiles, ragged on both axes (9 = 8 + 1 rows, 17 = 16 + 1 columns); wgrad_slices = 2 * 2 * 2 = 8 K slices
    "A": (5, 8, 9, 17, 3, False, 2),
    # exactly one full 8 x 16 tile, B = 1 (one wgrad slice). 7 * Ch = 140: two 96-wide N tiles, the last with 44 channels; 4 * Ch = 80 one
    # 96-wide tile, 3 * Ch = 60 one 64-wide. Weight gradients: 3 / 2 / 1 row tiles. LayerNorm over 140 * 128 .. 20 * 128 elements
    "B": (3, 20, 8, 16, 3, True, 1),
    # 7 * Ch = 252: two 128-wide N tiles (last: 124); 4 * Ch = 144: two 96-wide (last: 48); 3 * Ch = 108: one 128-wide; the conv_o / conv_last
    # adjoints (2 * Ch = 72 outputs): one 96-wide. 2 * Ch = 72 activation channels in the conv_o / conv_last weight gradients: three
    # column halves (32, 32, 8) = two column tiles, the second half-empty. Cin = 16: exactly one 16-channel k-step of the bf16 modes.
    # k = 5 on a 5 x 7 map
    "C": (16, 36, 5, 7, 5, False, 3),
    # 1 x 1 map, k = 1 (one tap), Cin = 1, Ch = 5 (not a multiple of 4: every staging and weight-gradient load takes its scalar path).
    # LayerNorm over 35, 20, 20, 15 and 5 elements (fewer than the 64 chunks of its statistics)
    "D": (1, 5, 1, 1, 1, True, 2),
    # k = 7 (reach 3) on a map 3 rows tall: every output row sees the top and the bottom padding at once. Three tiles along W (33 = 2 * 16
    # + 1), the last one a single column
    "E": (7, 6, 3, 33, 7, False, 2),
    # the model's own width: 7 * Ch = 448 (four 128-wide N tiles, the last with 64), 4 * Ch = 256 (two), 3 * Ch = 192 (two 96-wide),
    # 2 * Ch = 128 (one 128-wide; two full column tiles of the conv_o / conv_last weight gradients), 7 / 4 / 3 / 1 row tiles. 2 x 1 pixel tiles
    "F": (16, 64, 16, 16, 5, True, 2),
    # Cin = 130 = 2 * 64 + 2: conv_x contracts over at least three channel stages (a stage holds at most 64); its weight gradient has
    # five column halves (three column tiles, the last half-empty, its first half 2 channels wide); the dx adjoint has 130 outputs: two
    # 96-wide N tiles (last: 34)
    "G": (130, 8, 6, 6, 3, False, 1),
    # odd batch with LayerNorm on a map ragged on both axes (2 x 1 pixel tiles of 9 x 10); Ch = 12: 84 / 48 / 36 output channels
    "H": (4, 12, 9, 10, 3, True, 3),
}
SEED_BASE = {}   # case -> draw of its seeds, where draw 0 misses the input condition (none does)

CONVS = ("conv_x", "conv_h", "conv_a", "conv_m", "conv_o")
PARAM_KEYS = [f"{c}.0.{p}" for c in CONVS for p in ("weight", "bias")] + ["conv_last.weight", "conv_last.bias"]
LN_KEYS = [f"{c}.1.{p}" for c in CONVS for p in ("weight", "bias")]
INS = ("x", "h", "c", "m", "a")
OUTS = ("h_new", "c_new", "m_new", "delta_c", "delta_m")
LOSSES = {"full": OUTS, "h_only": ("h_new",), "c_dm": ("c_new", "delta_m"), "two_step": ("h_new", "delta_c", "delta_m")}


# ---- inputs, the fp64 reference, the fp32 restatement: computed once per case, shared, never written ---------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(case):
    """name -> float32 CPU tensor: the five inputs, x2 / a2 of a second step, the parameters, the cotangents g.<out> and g2.<out>."""
    Cin, Ch, H, W, k, ln, B = CASES[case]
    rn = lambda name, shape: seeded_randn(shape, name_seed(f"acstlstm.{case}.{name}", SEED_BASE.get(case, 0)))
    t = {"x": rn("x", (B, Cin, H, W)), "x2": rn("x2", (B, Cin, H, W)), "a2": 0.5 * rn("a2", (B, Ch, H, W))}
    for n in ("h", "c", "m", "a"):
        t[n] = 0.5 * rn(n, (B, Ch, H, W))
    for conv, ci, mult in (("conv_x", Cin, 7), ("conv_h", Ch, 4), ("conv_a", Ch, 4), ("conv_m", Ch, 3), ("conv_o", 2 * Ch, 1)):
        shape = (mult * Ch, ci, k, k)
        t[f"{conv}.0.weight"] = rn(f"{conv}.0.weight", shape) * fan_in_scale(shape)
        t[f"{conv}.0.bias"] = 0.1 * rn(f"{conv}.0.bias", (mult * Ch,))
        if ln:
            t[f"{conv}.1.weight"] = 1.0 + 0.3 * rn(f"{conv}.1.weight", (mult * Ch, H, W))
            t[f"{conv}.1.bias"] = 0.3 * rn(f"{conv}.1.bias", (mult * Ch, H, W))
    t["conv_last.weight"] = rn("conv_last.weight", (Ch, 2 * Ch, 1, 1)) * fan_in_scale((Ch, 2 * Ch, 1, 1))
    t["conv_last.bias"] = 0.1 * rn("conv_last.bias", (Ch,))
    for o in OUTS:
        t["g." + o] = rn("g." + o, (B, Ch, H, W))
        t["g2." + o] = rn("g2." + o, (B, Ch, H, W))
    return t


def _evaluate(step, t, loss):
    """Outputs and every gradient of one loss. `step(x, h, c, m, a, leaves)` -> the five outputs; `t` as from _inputs, on the device, in
    the dtype and in the layouts of the run. Losses: the sum of the named outputs times their fixed cotangents (LOSSES); `two_step`: a
    second step on (h_new, c_new, m_new) of the first with x2 and a2, the loss over h_new, delta_c, delta_m of both (the shape of the
    model's decoupling loss). A leaf that the loss does not reach has the zero gradient."""
    names = [n for n in t if not n.startswith("g") and (loss == "two_step" or n not in ("x2", "a2"))]
    lv = {n: t[n].detach().requires_grad_(True) for n in names}
    outs = step(*(lv[n] for n in INS), lv)
    res = {n: o.detach() for n, o in zip(OUTS, outs)}
    total = sum((o * t["g." + n]).sum() for n, o in zip(OUTS, outs) if n in LOSSES[loss])
    if loss == "two_step":
        outs2 = step(lv["x2"], outs[0], outs[1], outs[2], lv["a2"], lv)
        res.update({"step2." + n: o.detach() for n, o in zip(OUTS, outs2)})
        total = total + sum((o * t["g2." + n]).sum() for n, o in zip(OUTS, outs2) if n in LOSSES[loss])
    total.backward()
    for n in names:
        res["grad." + n] = torch.zeros_like(lv[n]) if lv[n].grad is None else lv[n].grad
    return res


def _cpu(case, loss, forget_bias, dtype):
    ln = CASES[case][5]
    t = {n: v.to(dtype) for n, v in _inputs(case).items()}
    return _evaluate(lambda x, h, c, m, a, p: torch_ref.acstlstm_cell(x, h, c, m, a, p, layer_norm=ln, forget_bias=forget_bias), t, loss)


@functools.lru_cache(maxsize=None)
def _case(case, loss="full", forget_bias=1.0):
    """(inputs, fp64 reference, fp32 CPU restatement) of one case under one loss."""
    return _inputs(case), _cpu(case, loss, forget_bias, torch.float64), _cpu(case, loss, forget_bias, torch.float32)


def _relmax(name, got, ref, bound):   # (parity.record's figure, unrecorded: for the host run)
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def _check(log, tag, got, ref, tol, inclusive=False):
    """Every entry of `ref` against `got` at tol = (outputs, gradients); all figures are measured and printed before any is judged."""
    assert set(got) == set(ref), (tag, sorted(set(got) ^ set(ref)))
    errs, bad = {}, []
    for k, r in ref.items():
        g = got[k].detach().cpu()
        assert g.shape == r.shape, (tag, k, tuple(g.shape), tuple(r.shape))
        bound = tol[1] if k.startswith("grad.") else tol[0]
        errs[k] = log(f"{tag}.{k}", g, r, bound)
        if not (errs[k] <= bound if inclusive else errs[k] < bound):
            bad.append((k, errs[k], bound))
    worst = lambda pre: max((v for k, v in errs.items() if k.startswith("grad.") == pre), default=0.0)
    print(f"{tag}: worst output {worst(False):.2e}, worst gradient {worst(True):.2e}")
    assert not bad, (tag, bad)
    return errs


def _condition(log, case, loss="full", forget_bias=1.0):
    """The input condition of one case; returns (inputs, fp64 reference)."""
    t, ref, cpu32 = _case(case, loss, forget_bias)
    _check(log, f"acst.cpu_fp32.{case}.{loss}.fb{forget_bias:g}", cpu32, ref, COND, inclusive=True)
    return t, ref


MISSING = [(c, l) for c in ("A", "H") for l in ("h_only", "c_dm")]
FORGET = [(c, fb) for c in ("A", "B") for fb in (0.0, 2.5)]


def host_conditions():
    """The CPU half of every case of every test below (inputs, fp64 reference, fp32 restatement, the condition): no GPU."""
    for case in CASES:
        _condition(_relmax, case)
    for case, loss in MISSING:
        _condition(_relmax, case, loss)
    for case, fb in FORGET:
        _condition(_relmax, case, "full", fb)
    for case in ("A", "H"):
        _condition(_relmax, case, "two_step")


# ---- the GPU side --------------------------------------------------------------------------------------------------------------------
def _gpu(vpx, case, loss="full", forget_bias=1.0, mode="f32", layout="nchw"):
    """`layout`: the five inputs as contiguous NCHW tensors (`nchw`), already channels-last (`channels_last`), or x as a channel slice
    of a wider NCHW tensor, non-contiguous (`sliced_x`)."""
    ln = CASES[case][5]
    t = {n: v.cuda() for n, v in _inputs(case).items()}
    if layout == "channels_last":
        for n in INS + ("x2", "a2"):
            t[n] = t[n].contiguous(memory_format=torch.channels_last)
    elif layout == "sliced_x":
        for n in ("x", "x2"):
            B, Cin, H, W = t[n].shape
            wide = torch.full((B, Cin + 5, H, W), 7.0, device="cuda")
            wide[:, 2:2 + Cin] = t[n]
            t[n] = wide[:, 2:2 + Cin]
            assert not t[n].is_contiguous()

    def step(x, h, c, m, a, p):
        return vpx.ops.acstlstm_step(x, h, c, m, a, [p[k] for k in PARAM_KEYS], [p[k] for k in LN_KEYS] if ln else (), precision=mode,
                                     forget_bias=forget_bias)
    return _evaluate(step, t, loss)


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


def _same_bits(a, b, what):
    assert set(a) == set(b)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, (what, differ)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", list(CASES))
def test_acstlstm_parity_vs_fp64(vpx, parity_log, case, mode):
    """The five outputs, dx, dh, dc, dm, da, the 12 convolution and (LayerNorm cases) the 10 LayerNorm parameter gradients under a loss
    over all five outputs. At these sizes every layer with more than one stage runs K-split."""
    _, ref = _condition(parity_log, case)
    assert len(ref) == 5 + 5 + 12 + (10 if CASES[case][5] else 0)
    _check(parity_log, f"acst.{case}.{mode}", _gpu(vpx, case, mode=mode), ref, TOL[mode])


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", ["A", "C", "F", "H"])
def test_acstlstm_parity_unsplit_path_and_same_bits(vpx, parity_log, case, mode):
    """Deterministic mode: pick_ksplit returns 1, so every convolution of the cell runs unsplit (no memset, no atomics; the `accumulate`
    epilogue adds conv_last's adjoint into dmem and conv_m's into dm in place) — the path of the B = 128 workload. The same bars, and
    two runs give the same bits in every output and every gradient."""
    _, ref = _condition(parity_log, case)
    with _deterministic():
        runs = [_gpu(vpx, case, mode=mode) for _ in range(2)]
    _check(parity_log, f"acst.det.{case}.{mode}", runs[0], ref, TOL[mode])
    _same_bits(runs[0], runs[1], "two deterministic runs")


@pytest.mark.parametrize("case,loss", MISSING)
def test_acstlstm_parity_missing_incoming_gradients(vpx, parity_log, case, loss):
    """`h_only`: the four state cotangents reach the library as NULL; `c_dm`: dh_new is missing (the binding substitutes zeros) and so
    are dm_new and d(delta_c); conv_o and conv_last get the exact zero gradient."""
    _, ref = _condition(parity_log, case, loss)
    with _spy(vpx._lib.lib(), "vpx_acstlstm_step_bwd") as calls:
        got = _gpu(vpx, case, loss)
    assert len(calls) == 1
    given = [g is not None for g in calls[0][10:15]]   # (dh_new, dc_new, dm_new, ddc, ddm)
    assert given == ([True, False, False, False, False] if loss == "h_only" else [True, True, False, False, True]), given
    _check(parity_log, f"acst.{loss}.{case}", got, ref, TOL["f32"])


@pytest.mark.parametrize("case,forget_bias", FORGET)
def test_acstlstm_parity_forget_bias(vpx, parity_log, case, forget_bias):
    _, ref = _condition(parity_log, case, "full", forget_bias)
    _check(parity_log, f"acst.fb{forget_bias:g}.{case}", _gpu(vpx, case, forget_bias=forget_bias), ref, TOL["f32"])


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", ["A", "H"])
def test_acstlstm_parity_two_chained_steps(vpx, parity_log, case, mode):
    """Step 2 runs on (h_new, c_new, m_new) of step 1: its dh, dc, dm arrive as step 1's dh_new, dc_new, dm_new next to the loss's own
    d(h_new), d(delta_c), d(delta_m), and every parameter gradient is the sum of two backward calls."""
    _, ref = _condition(parity_log, case, "two_step")
    _check(parity_log, f"acst.two_step.{case}.{mode}", _gpu(vpx, case, "two_step", mode=mode), ref, TOL[mode])


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_acstlstm_layouts_same_bits(vpx, mode):
    """Inputs that are already channels-last, and an x that is a channel slice of a wider tensor, give the bits of contiguous NCHW
    inputs (deterministic mode: no atomics)."""
    with _deterministic():
        base = _gpu(vpx, "A", mode=mode)
        for layout in ("channels_last", "sliced_x"):
            _same_bits(_gpu(vpx, "A", mode=mode, layout=layout), base, layout)


def test_acstlstm_parity_plain_bf16_forward(vpx, parity_log):
    _, ref = _condition(parity_log, "C")
    ln = CASES["C"][5]
    t = {n: v.cuda() for n, v in _inputs("C").items()}
    with torch.no_grad():
        outs = vpx.ops.acstlstm_step(*(t[n] for n in INS), [t[k] for k in PARAM_KEYS], [t[k] for k in LN_KEYS] if ln else (), precision="bf16")
    _check(parity_log, "acst.C.bf16", dict(zip(OUTS, outs)), {n: ref[n] for n in OUTS}, (BF16_FWD_TOL, None))


def test_acstlstm_refusals_before_any_launch(vpx):
    """Even or too wide kernels are refused by the workspace query; a wrong count of parameter or LayerNorm tensors by the binding."""
    Cin, Ch, H, W, B = 3, 4, 6, 6, 2
    z = lambda *shape: torch.zeros(*shape, device="cuda")

    def args(k, n_params=12, n_ln=0):
        params = []
        for ci, mult in ((Cin, 7), (Ch, 4), (Ch, 4), (Ch, 3), (2 * Ch, 1)):
            params += [z(mult * Ch, ci, k, k), z(mult * Ch)]
        params += [z(Ch, 2 * Ch, 1, 1), z(Ch)]
        ln = [z(mult * Ch, H, W) for mult in (7, 7, 4, 4, 4, 4, 3, 3, 1, 1)]
        return (z(B, Cin, H, W), *(z(B, Ch, H, W) for _ in range(4)), params[:n_params], ln[:n_ln])

    with _spy(vpx._lib.lib(), "vpx_acstlstm_step_fwd") as calls:
        for k in (4, 9):
            with pytest.raises(ValueError):
                vpx.ops.acstlstm_step(*args(k))
        with pytest.raises(ValueError):
            vpx.ops.acstlstm_step(*args(3, n_params=11))
        with pytest.raises(ValueError):
            vpx.ops.acstlstm_step(*args(3, n_ln=9))
        assert not calls
        vpx.ops.acstlstm_step(*args(3))   # (the same arguments, complete, are accepted)
        vpx.ops.acstlstm_step(*args(3, n_ln=10))
    assert len(calls) == 2
