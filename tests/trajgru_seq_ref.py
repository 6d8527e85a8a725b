"""The TrajGRU sequence (vpx_trajgru_seq_fwd / _bwd behind `traj_ops.trajgru_seq`; csrc/trajgru.hip) in plain float64, with the case table of
tests/test_gpu_trajgru_routes.py (GPU parity) and tests/test_trajgru_seq_cases.py (validity of every case, on the CPU). Nothing here touches
the GPU or imports the package.

The statement: `oracle.torch_ref.trajgru_seq(..., i2h_pad=k // 2)` on the CPU in float64 under autograd, on the float32 inputs cast up. A
case names B, T, Cin, C, H, W, L, k_i2h, the operands present ("x+h0"; "x": the zero-state form, h0 NULL; "h0": the forecaster form, x NULL),
the leaves whose gradient the call is asked for ("all", "params", "inputs", "none": the inference route under no_grad), the loss (the sum of
the named outputs times fixed random cotangents: "out", "hT", "out_hT"), the deterministic setting and a seed revision. Every case runs in
exact-fp32 ("f32") and in split-bf16 ("bf16x3") mode.

Inputs, seeded as in tests/test_gpu_fuzz.py under the names "trajgru.seq.<tag>.r<rev>.*": weights randn / sqrt(fan_in), biases 0.1 randn, x
uniform [0, 1), h0 0.5 randn, cotangents randn. `flows_conv` alone differs: its weight and bias are multiplied by FLOW_GAIN = 3, so that the
flows the generator itself produces are real displacements — every case on a map with H, W > 1 has 2 <= max|flow| <= 6 pixels in the
float64 reference (measured over the table: 2.2 to 4.7), which puts taps off every side of a 5x7 map and sends a full-size gradient down
the flow branch (df1, d_h2f_w, d_i2f_w, the flow branch's share of dx and dh).

Kinks. The block has two LeakyReLUs (the flow features, the candidate memory) and the bilinear sampler's cell boundaries. A case is
compared to a tight bar only if none of them is within reach of the arithmetic's noise; these are conditions on the inputs, checked on the
CPU (violations()), never exclusions — no element and no case is left out of a comparison, a case inside a margin gets the next seed
revision (REJECTED):
  COORD_MARGIN   1e-4 px   every sampling coordinate of the float64 reference is at least this far from every integer (the padding
                           borders -1 and W - 1 / H - 1 are integers; coordinates beyond the map's reach are held to it all the same)
  PREACT_MARGIN  1e-5      every pre-activation of either LeakyReLU is at least this far from 0 (trajgru_warp_ref.PREACT_MARGIN)
  DEVIATION      1/10      in both restatements below, the sampling coordinates (pixels: the flows times W / (W - 1)) and the
                           pre-activations deviate from float64 by at most a tenth of the distance the case itself keeps from the
                           nearest integer / from 0
The third condition is the binding one. The two margins are floors: the bf16x3 restatement moves coordinates by 1.4e-5 to 3.4e-5 px and
pre-activations by 4e-6 to 2.3e-5 on every seed of a multi-pixel map (the f32 restatement: up to 3.3e-6 px and 1.6e-6), which is more
than a tenth of either floor — so a case must keep its kinks ten times its own restatements' deviation away, further than the floors ask.
In the table: the nearest coordinate is 2.4e-4 px from an integer, the nearest pre-activation at 8.5e-5.
A gradient whose reference is exactly zero (a one-step call without h0 warps a zero state: nothing flows back into the flow generator, the
gradients of h2f_conv1, i2f_conv1 and flows_conv are all zero) must be zero bit for bit.

Restatements, on the same inputs; they only set bars and margins and never touch the code under test:
  f32      the same function in float32
  bf16x3   float64 throughout, but each operand of the five convolutions — activations and weights in the forward, the incoming gradient
           with the weights (data gradient) and with the activations (weight gradient) in the backward — is first rounded to float32 and
           split as the library splits it: hi = the bf16 rounding of v, lo = the bf16 rounding of v - hi, both ROUND TO NEAREST EVEN
           (split_bf16 in csrc/conv_gemm.hip, c2_split in csrc/cell2_dev.h behind split_convert_kernel: `(__bf16)v`, v_cvt_pk_bf16_f32;
           not truncation). hi*hi + hi*lo + lo*hi are summed in float64, lo*lo is dropped. Bias sums are plain.

Bars, max-normalised (parity.relmax), per case, tensor and mode. Base: forward 2e-5 (f32) / 1e-4 (bf16x3), TrajGRU's present bounds
(test_trajgru_block_vs_golden, test_random_trajgru_blocks_vs_oracle); gradients 1e-4 (f32, trajgru_warp_ref.GRAD_F32) / 2e-4 (bf16x3,
stlstm_ref.BARS, convlstm_ref.BARS). A bar becomes 3 x the matching restatement's own error against float64 where that error exceeds a
third of the base (the factor covers an equally valid summation order: bar_from in tests/test_gpu_unet3d.py, bars in trajgru_warp_ref.py).
CEILING: a derived bar above 4 x its base is not given; the case gets the next seed revision.

MEASURED over the table (tests/test_trajgru_seq_cases.py prints the figures per case and holds the table to these ceilings):
  f32 restatement     worst output error 1.0e-6 (k3, out), worst gradient error 2.2e-6 (k5_9x6, ret.weight)
  bf16x3 restatement  worst output error 1.5e-5 (params_only, out), worst gradient error 4.2e-5 (k5_9x6, ret.weight)
Both are under a third of every base bar (6.7e-6 / 3.3e-5 forward, 3.3e-5 / 6.7e-5 gradients): NO bar is raised in either mode, every
tensor of every case is held to its base bar.
  max|flow|           2.2 to 4.7 px over the cases with H, W > 1
  fp64 reference      0.7 s for the whole table on the CPU, both restatements included
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import name_seed, seeded_rand, seeded_randn

NAMES = ("i2h", "i2f_conv1", "h2f_conv1", "flows_conv", "ret")
PARAM_KEYS = tuple(f"{n}.{kind}" for n in NAMES for kind in ("weight", "bias"))
INPUT_SIDE = PARAM_KEYS[:4]          # i2h and i2f_conv1: without x the library neither reads nor writes their gradients
SLOPE = 0.2
FLOW_FEATURES = 32
FLOW_GAIN = 3.0
FLOW_RANGE = (2.0, 6.0)              # max|flow| in pixels of every case with H, W > 1 (float64 reference)
COORD_MARGIN, PREACT_MARGIN, DEVIATION = 1e-4, 1e-5, 0.1
MODES = ("f32", "bf16x3")
FWD = {"f32": 2e-5, "bf16x3": 1e-4}
GRAD = {"f32": 1e-4, "bf16x3": 2e-4}
CEILING = 4.0
LOSSES = {"out": ("out",), "hT": ("hT",), "out_hT": ("out", "hT")}

Case = collections.namedtuple("Case", "tag B T Cin C H W L k ops grads loss det rev")

# Seed revisions that were turned down (revision: why); tests/test_trajgru_seq_cases.py holds the revision in use to every condition.
REJECTED = {
    "k3": {0: "a sampling coordinate 1.2e-05 px from an integer"},
    "k5_9x6": {0: "bf16x3 coordinates deviate by 3.6e-05 px, the nearest integer is 1.2e-04 px away", 1: "bf16x3 coordinates deviate by 2.8e-05 px, the nearest integer is 2.1e-04 px away", 2: "a sampling coordinate 6.7e-05 px from an integer"},
    "k7_8x8": {0: "bf16x3 pre-activations deviate by 2.1e-05, the nearest is at 5.2e-05", 1: "bf16x3 pre-activations deviate by 2.3e-05, the nearest is at 1.3e-04", 2: "bf16x3 pre-activations deviate by 1.3e-05, the nearest is at 4.2e-05"},
    "t3_l5": {0: "bf16x3 pre-activations deviate by 1.2e-05, the nearest is at 4.2e-05"},
    "t4_cin1_l1": {0: "bf16x3 pre-activations deviate by 1.3e-05, the nearest is at 9.9e-05", 1: "bf16x3 pre-activations deviate by 3.1e-05, the nearest is at 2.5e-04"},
    "c32_cin8_8x8": {0: "a pre-activation at 8.6e-06", 1: "bf16x3 pre-activations deviate by 2.0e-05, the nearest is at 4.5e-05", 2: "bf16x3 pre-activations deviate by 1.7e-05, the nearest is at 1.7e-04", 3: "a sampling coordinate 9.6e-05 px from an integer", 4: "bf16x3 pre-activations deviate by 2.6e-05, the nearest is at 4.8e-05"},
    "c12_cin4": {0: "bf16x3 pre-activations deviate by 1.4e-05, the nearest is at 8.4e-05"},
    "fc": {0: "max|flow| 1.95 px", 1: "bf16x3 pre-activations deviate by 1.0e-05, the nearest is at 7.3e-05", 2: "bf16x3 pre-activations deviate by 1.1e-05, the nearest is at 3.5e-05", 3: "bf16x3 pre-activations deviate by 1.2e-05, the nearest is at 1.8e-05", 4: "bf16x3 pre-activations deviate by 1.1e-05, the nearest is at 8.6e-05", 5: "bf16x3 pre-activations deviate by 9.1e-06, the nearest is at 7.1e-05", 6: "bf16x3 pre-activations deviate by 6.7e-06, the nearest is at 1.1e-05", 7: "bf16x3 pre-activations deviate by 6.3e-06, the nearest is at 2.6e-05"},
    "fc_t3_det": {0: "max|flow| 1.83 px", 1: "a sampling coordinate 3.5e-05 px from an integer", 2: "bf16x3 pre-activations deviate by 9.6e-06, the nearest is at 6.0e-05", 3: "bf16x3 pre-activations deviate by 9.2e-06, the nearest is at 2.0e-05"},
    "fc_t1_hT": {0: "bf16x3 pre-activations deviate by 1.0e-05, the nearest is at 1.7e-05"},
    "fc_params": {0: "bf16x3 pre-activations deviate by 1.0e-05, the nearest is at 5.6e-05"},
    "zs_t1": {0: "max|flow| 1.80 px"},
    "zs_k5_hT": {0: "bf16x3 pre-activations deviate by 7.5e-06, the nearest is at 1.4e-05", 1: "bf16x3 coordinates deviate by 2.4e-05 px, the nearest integer is 1.3e-04 px away", 2: "a sampling coordinate 4.8e-05 px from an integer", 3: "bf16x3 pre-activations deviate by 8.5e-06, the nearest is at 1.8e-05", 4: "a sampling coordinate 4.8e-05 px from an integer", 5: "bf16x3 pre-activations deviate by 1.0e-05, the nearest is at 4.6e-05", 6: "a sampling coordinate 4.9e-05 px from an integer"},
    "zs_inputs": {0: "a sampling coordinate 7.6e-05 px from an integer"},
    "inputs_only": {0: "bf16x3 coordinates deviate by 2.4e-05 px, the nearest integer is 1.6e-04 px away"},
    "loss_out_t3": {0: "bf16x3 pre-activations deviate by 1.5e-05, the nearest is at 6.7e-05", 1: "max|flow| 6.22 px"},
    "loss_hT_t3": {0: "bf16x3 pre-activations deviate by 1.8e-05, the nearest is at 6.4e-05", 1: "bf16x3 pre-activations deviate by 1.7e-05, the nearest is at 2.5e-05"},
    "det_t3": {0: "bf16x3 pre-activations deviate by 1.6e-05, the nearest is at 2.9e-05", 1: "bf16x3 pre-activations deviate by 1.1e-05, the nearest is at 1.0e-04", 2: "a sampling coordinate 2.9e-05 px from an integer"},
    "infer_t3": {0: "bf16x3 coordinates deviate by 3.0e-05 px, the nearest integer is 2.9e-04 px away", 1: "bf16x3 coordinates deviate by 2.4e-05 px, the nearest integer is 2.0e-04 px away", 2: "bf16x3 pre-activations deviate by 1.5e-05, the nearest is at 2.6e-05", 3: "bf16x3 pre-activations deviate by 1.8e-05, the nearest is at 1.6e-05", 4: "bf16x3 coordinates deviate by 2.9e-05 px, the nearest integer is 1.2e-04 px away", 5: "bf16x3 coordinates deviate by 2.4e-05 px, the nearest integer is 2.2e-04 px away"},
    "infer_zs_k7_l13": {0: "a sampling coordinate 4.1e-05 px from an integer", 1: "bf16x3 pre-activations deviate by 8.1e-06, the nearest is at 4.4e-05"},
}


def _rev(tag):
    return 1 + max(REJECTED.get(tag, {-1: ""}))


def _c(tag, B, T, Cin, C, H, W, L, k=3, ops="x+h0", grads="all", loss="out_hT", det=0):
    assert ops in ("x+h0", "x", "h0") and grads in ("all", "params", "inputs", "none") and loss in LOSSES and k in (1, 3, 5, 7) and C % 4 == 0
    return Case(tag, B, T, Cin, C, H, W, L, k, ops, grads, loss, det, _rev(tag))


_TABLE = (
    # ---- the input projection's kernel ----------------------------------------------------------------------------------------------
    _c("k1", 1, 2, 3, 8, 5, 7, 3, k=1),
    _c("k3", 1, 2, 3, 8, 5, 7, 3),
    _c("k5_9x6", 1, 2, 4, 8, 9, 6, 3, k=5),                    # also run as the TrajGRU module (i2h_kernel=(5, 5), i2h_pad=(2, 2))
    _c("k7_8x8", 1, 2, 3, 4, 8, 8, 3, k=7),
    # ---- steps: T = 1 has no carry swap and no recurrent share of dh; T = 3, 4 swap carry / dprev two and three times ---------------------
    _c("t1", 2, 1, 3, 8, 5, 7, 3),
    _c("t3_l5", 1, 3, 3, 8, 5, 7, 5),
    _c("t4_cin1_l1", 1, 4, 1, 4, 5, 7, 1, loss="out"),
    # ---- channel and field counts: the default model's first encoder block has L = 13 ------------------------------------------------------
    _c("l13_c4", 1, 2, 3, 4, 5, 7, 13),
    _c("c32_cin8_8x8", 1, 2, 8, 32, 8, 8, 3),
    _c("c12_cin4", 1, 2, 4, 12, 5, 7, 3),
    # ---- the forecaster form (x NULL): LeakyReLU in h2f's own epilogue, no i2h term in the gates, dparams[0..3] absent -------------------------
    _c("fc", 1, 2, 3, 8, 5, 7, 3, ops="h0"),
    _c("fc_t3_det", 1, 3, 3, 8, 5, 7, 3, ops="h0", loss="out", det=1),
    _c("fc_t1_hT", 2, 1, 3, 8, 5, 7, 3, ops="h0", loss="hT"),
    _c("fc_params", 1, 2, 3, 8, 5, 7, 3, ops="h0", grads="params"),
    # ---- the zero-state form (h0 NULL); at T = 1 the gradient of h2f_conv1.weight is exactly zero ------------------------------------------
    _c("zs_t1", 2, 1, 3, 8, 5, 7, 3, ops="x"),
    _c("zs_t3", 1, 3, 3, 8, 5, 7, 3, ops="x"),
    _c("zs_k5_hT", 2, 2, 3, 8, 5, 7, 3, k=5, ops="x", loss="hT"),
    _c("zs_inputs", 1, 2, 3, 8, 5, 7, 3, ops="x", grads="inputs", loss="out"),
    # ---- subsets of the leaves: the library is handed NULL for dx / dh0 -----------------------------------------------------------------
    _c("params_only", 1, 2, 3, 8, 5, 7, 3, grads="params"),
    _c("inputs_only", 1, 2, 3, 8, 5, 7, 3, grads="inputs"),
    # ---- losses that leave a cotangent out: once more through the raw C ABI with NULL dhT / NULL dout ------------------------------------
    _c("loss_out_t3", 1, 3, 3, 8, 5, 7, 3, loss="out"),
    _c("loss_hT_t3", 2, 3, 3, 8, 5, 7, 3, loss="hT"),
    # ---- deterministic mode: the fixed-point scatter ------------------------------------------------------------------------------------
    _c("det_t3", 1, 3, 3, 8, 5, 7, 3, det=1),
    _c("det_1x1_b3", 3, 2, 3, 8, 1, 1, 3, det=1),
    # ---- 1-wide maps --------------------------------------------------------------------------------------------------------------------
    _c("map_1x7_b3", 3, 2, 3, 8, 1, 7, 3),
    _c("map_6x1_k5", 1, 2, 3, 8, 6, 1, 3, k=5),
    # ---- the inference route (no VPX_FLAG_SAVE_FOR_BWD): workspace buffers instead of the reserve ----------------------------------------------
    _c("infer_t3", 1, 3, 3, 8, 5, 7, 3, grads="none"),
    _c("infer_fc_det", 1, 2, 3, 8, 5, 7, 3, ops="h0", grads="none", det=1),
    _c("infer_zs_k7_l13", 1, 2, 4, 4, 5, 7, 13, k=7, ops="x", grads="none"),
)
CASES = collections.OrderedDict((c.tag, c) for c in _TABLE)
assert len(CASES) == len(_TABLE)
MODULE_CASE = "k5_9x6"

# What the table must cover; each value at a case where a gradient is taken (tests/test_trajgru_seq_cases.py asserts each list).
REQUIRED = {
    "k": {1, 3, 5, 7}, "T": {1, 2, 3, 4}, "L": {1, 3, 5, 13}, "C": {4, 8, 12, 32}, "Cin": {1, 3, 4, 8}, "B": {1, 2, 3},
    "map": {(1, 1), (1, 7), (6, 1), (5, 7), (8, 8), (9, 6)}, "ops": {"x+h0", "x", "h0"}, "loss": {"out", "hT", "out_hT"},
}


def has_x(case):
    return "x" in case.ops


def has_h0(case):
    return "h0" in case.ops


def used_params(case):
    return PARAM_KEYS if has_x(case) else PARAM_KEYS[4:]


def leaves(case):
    """The leaves whose gradient the case compares, in the order x, h0, parameters."""
    inp = tuple(n for n, on in (("x", has_x(case)), ("h0", has_h0(case))) if on)
    return {"all": inp + used_params(case), "params": used_params(case), "inputs": inp, "none": ()}[case.grads]


def shapes(case):
    C, Cin, L, k = case.C, case.Cin, case.L, case.k
    return {"i2h": (3 * C, Cin, k, k), "i2f_conv1": (FLOW_FEATURES, Cin, 5, 5), "h2f_conv1": (FLOW_FEATURES, C, 5, 5),
            "flows_conv": (2 * L, FLOW_FEATURES, 5, 5), "ret": (3 * C, L * C, 1, 1)}


@functools.lru_cache(maxsize=None)
def _inputs(tag):
    case = CASES[tag]
    seed = f"trajgru.seq.{tag}.r{case.rev}"
    t = {}
    for n, s_ in shapes(case).items():
        t[n + ".weight"] = seeded_randn(s_, name_seed(f"{seed}.{n}.w"), 1.0 / np.sqrt(s_[1] * s_[2] * s_[3]))
        t[n + ".bias"] = seeded_randn((s_[0],), name_seed(f"{seed}.{n}.b"), 0.1)
    t["flows_conv.weight"] = t["flows_conv.weight"] * FLOW_GAIN
    t["flows_conv.bias"] = t["flows_conv.bias"] * FLOW_GAIN
    t["x"] = seeded_rand((case.B, case.T, case.Cin, case.H, case.W), name_seed(seed + ".x"))
    t["h0"] = seeded_randn((case.B, case.C, case.H, case.W), name_seed(seed + ".h"), 0.5)
    t["g.out"] = seeded_randn((case.B, case.T, case.C, case.H, case.W), name_seed(seed + ".g"))
    t["g.hT"] = seeded_randn((case.B, case.C, case.H, case.W), name_seed(seed + ".ghT"))
    return t


def inputs(tag):
    """name -> float32 CPU tensor: the ten parameters (PARAM_KEYS), x, h0 (a case uses the operands it has) and the cotangents g.out,
    g.hT. Nobody writes them."""
    return _inputs(tag)


def evaluate(seq, t, case):
    """`seq(x, h0, P)` -> (out, hT) with x / h0 None where the case has none and P the ten parameters by name; `t` as from inputs(), on
    the device and in the dtype of the run. All ten parameters are handed over; the leaves of the case (and, with them, the unused
    input-side parameters of a forecaster call) require a gradient. Returns ({"out", "hT", "grad.<leaf>"...}, the leaf tensors)."""
    want = leaves(case)
    ask = set(want) | (set(INPUT_SIDE) if case.grads in ("all", "params") else set())
    lv = {n: t[n].detach().clone().requires_grad_(n in ask) for n in PARAM_KEYS + ("x", "h0")}
    with torch.enable_grad() if want else torch.no_grad():
        out, hT = seq(lv["x"] if has_x(case) else None, lv["h0"] if has_h0(case) else None, {k: lv[k] for k in PARAM_KEYS})
        res = {"out": out.detach(), "hT": hT.detach()}
        if want:
            sum((o * t["g." + n]).sum() for n, o in (("out", out), ("hT", hT)) if n in LOSSES[case.loss]).backward()
    for n in want:
        assert lv[n].grad is not None, (case.tag, n, "no gradient")
        res["grad." + n] = lv[n].grad.detach()
    return res, lv


def _split(v):
    """hi, lo of the float32 rounding of v, both bf16 by round to nearest even (torch's conversion), as float64."""
    f = v.detach().float()
    hi = f.bfloat16().float()
    lo = (f - hi).bfloat16().float()
    return hi.double(), lo.double()


class _SplitConv(torch.autograd.Function):
    """conv2d whose three contractions (forward, data gradient, weight gradient) run on split operands, products and sums in float64."""
    @staticmethod
    def forward(ctx, x, w, b, pad):
        ctx.save_for_backward(x, w)
        ctx.pad = pad
        (xh, xl), (wh, wl) = _split(x), _split(w)
        conv = lambda a, c: torch.conv2d(a, c, None, 1, pad)
        return conv(xh, wh) + conv(xh, wl) + conv(xl, wh) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        (xh, xl), (wh, wl), (gh, gl) = _split(x), _split(w), _split(dy)
        di = lambda g, c: torch.nn.grad.conv2d_input(x.shape, c, g, padding=ctx.pad)
        dw = lambda a, g: torch.nn.grad.conv2d_weight(a, w.shape, g, padding=ctx.pad)
        return di(gh, wh) + di(gh, wl) + di(gl, wh), dw(xh, gh) + dw(xh, gl) + dw(xl, gh), dy.sum((0, 2, 3)), None


def _split_conv2d(t, w, b=None, stride=1, padding=0):
    assert stride == 1 and b is not None
    return _SplitConv.apply(t, w, b, padding)


Run = collections.namedtuple("Run", "tensors coords preacts max_flow")


@functools.lru_cache(maxsize=None)
def run(tag, how="f64"):
    """The case on the CPU. how: "f64" (the reference), "f32", "bf16x3" (the restatements). Returns the tensors of evaluate(), every
    sampling coordinate in pixels ([calls, 2, B, H, W]: x then y, one call per step and field), every pre-activation of the two
    LeakyReLUs (flat) and max|flow|. Computed once; callers must not modify it."""
    from oracle import torch_ref as tr
    case = CASES[tag]
    dtype = torch.float32 if how == "f32" else torch.float64
    t = {n: v.to(dtype) for n, v in inputs(tag).items()}
    coords, pre = [], []
    plain = F.grid_sample, F.leaky_relu, F.conv2d

    def watching_sample(inp, grid, **kw):
        Hs, Ws = inp.shape[-2:]
        g = grid.detach().double()
        coords.append(torch.stack((((g[..., 0] + 1) * Ws - 1) / 2, ((g[..., 1] + 1) * Hs - 1) / 2)))
        return plain[0](inp, grid, **kw)

    def watching_leaky(v, *a, **kw):
        pre.append(v.detach().double().reshape(-1))
        return plain[1](v, *a, **kw)

    def seq(x, h0, P):
        return tr.trajgru_seq(x, h0, case.T, P, case.L, SLOPE, i2h_pad=case.k // 2)

    F.grid_sample, F.leaky_relu = watching_sample, watching_leaky
    if how == "bf16x3":
        F.conv2d = _split_conv2d
    try:
        res, _ = evaluate(seq, t, case)
    finally:
        F.grid_sample, F.leaky_relu, F.conv2d = plain
    coords = torch.stack(coords)
    # sx = (x - fx) * kx - 0.5: the flow back out of the coordinate
    kx, ky = case.W / max(case.W - 1, 1), case.H / max(case.H - 1, 1)
    gx = torch.arange(case.W, dtype=torch.float64).view(1, 1, 1, case.W)
    gy = torch.arange(case.H, dtype=torch.float64).view(1, 1, case.H, 1)
    fx, fy = gx - (coords[:, 0] + 0.5) / kx, gy - (coords[:, 1] + 0.5) / ky
    return Run(res, coords, torch.cat(pre), float(torch.maximum(fx.abs(), fy.abs()).max()))


Reference = collections.namedtuple("Reference", "tensors coord_dist preact_dist max_flow coords preacts")


def reference(tag):
    """The float64 reference of a case: out, hT and "grad.<leaf>" of every leaf it asks for; the smallest distance of a sampling
    coordinate from an integer, the smallest |pre-activation| of both LeakyReLUs, max|flow|, and the coordinates and pre-activations
    themselves."""
    r = run(tag, "f64")
    return Reference(r.tensors, float((r.coords - r.coords.round()).abs().min()), float(r.preacts.abs().min()), r.max_flow, r.coords, r.preacts)


def relmax(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def base_bar(name, mode):
    return (GRAD if name.startswith("grad.") else FWD)[mode]


def bars(tag, mode):
    """name -> (bound, the restatement's own error against float64): the base bar, or 3 x that error where it exceeds a third of the base."""
    ref, rst = run(tag, "f64").tensors, run(tag, mode).tensors
    res = {}
    for name, r in ref.items():
        err, base = relmax(rst[name], r), base_bar(name, mode)
        res[name] = (base if err <= base / 3 else 3 * err, err)
    return res


def deviation(tag, mode):
    """(coordinates in pixels, pre-activations): the largest deviation of the restatement from the float64 reference."""
    ref, rst = run(tag, "f64"), run(tag, mode)
    return float((rst.coords - ref.coords).abs().max()), float((rst.preacts - ref.preacts).abs().max())


def violations(tag):
    """Why the case's seed revision may not be used (empty: it may), in the order the conditions are stated in the module docstring."""
    case, ref, why = CASES[tag], reference(tag), []
    if ref.coord_dist < COORD_MARGIN:
        why.append(f"a sampling coordinate {ref.coord_dist:.1e} px from an integer")
    if ref.preact_dist < PREACT_MARGIN:
        why.append(f"a pre-activation at {ref.preact_dist:.1e}")
    if case.H > 1 and case.W > 1 and not FLOW_RANGE[0] <= ref.max_flow <= FLOW_RANGE[1]:
        why.append(f"max|flow| {ref.max_flow:.2f} px")
    if why:
        return why
    for mode in MODES:
        dc, dp = deviation(tag, mode)
        if dc > DEVIATION * ref.coord_dist:
            why.append(f"{mode} coordinates deviate by {dc:.1e} px, the nearest integer is {ref.coord_dist:.1e} px away")
        if dp > DEVIATION * ref.preact_dist:
            why.append(f"{mode} pre-activations deviate by {dp:.1e}, the nearest is at {ref.preact_dist:.1e}")
        for name, (bound, err) in bars(tag, mode).items():
            if bound > CEILING * base_bar(name, mode):
                why.append(f"{mode} {name}: the restatement's error {err:.1e} puts the bar above its ceiling")
    return why
