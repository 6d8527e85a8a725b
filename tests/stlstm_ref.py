"""The plain ST-LSTM cell step (vpx_stlstm_step_fwd_ex / _bwd_ex behind `ops.stlstm_step`; csrc/stlstm_api.hip, csrc/stlstm_bwd_api.hip,
csrc/stlstm_ln_api.hip) in plain float64, with the case table of tests/test_gpu_stlstm_routes.py (GPU parity) and tests/test_stlstm_host.py
(the plan every case takes, the workspace contract in a dry run, the condition of the inputs, on the CPU). Nothing here touches the GPU or
imports the package.

The statement: `oracle.torch_ref.stlstm_cell` on the CPU under autograd, on the float32 inputs cast up. Inputs (`seeded_randn`): weights
randn / sqrt(fan_in), x and the states 0.5 randn, cotangents randn, LayerNorm weight 1 + 0.1 randn and bias 0.1 randn ([C,H,W]). The cell
has no kinks (sigmoid, tanh, products): nothing is left out of a comparison.

A case is a shape (Cin, Ch, H, W, k, layer_norm, B), an operand mode, experiment bits (names of _lib.Exp joined by '|'), the deterministic
setting, the leaves whose gradients the call is asked for, a loss, a layout of the inputs — and the plan it is there to reach: the fields of
vpx_stlstm_plan_info (include/vpx.h) it must show, written next to the shape. tests/test_stlstm_host.py holds the table to the library's
own answer. Pixel tiles: 8 x 16 for the first-generation kernels (their grid rules count B * ceil(H/8) * ceil(W/16)), 16 x 16 for c5 (the
forward runs unsplit from 48 of them, the backward from 96; at most 16: the `ks_small` chunking, between: `ks_mid`). Narrow maps (17 x 1,
1 x 17) buy many tiles for few pixels."""
import collections
import functools

import torch

from golden_util import fan_in_scale, name_seed, seeded_randn
from oracle import torch_ref

BARS = {"f32": (1e-5, 5e-5), "bf16x3": (6e-5, 2e-4), "bf16": (3e-2, None)}   # (outputs, gradients) in max|d| / max|ref|; plain bf16: forward only
COND = (5e-6, 2.5e-5)                                                        # the fp32 CPU run against fp64: half the f32 bars

LN, GEN1, C5, C5K = 0, 1, 2, 3                                               # vpx_stlstm_plan_info.route (VPX_ST_ROUTE_*)
STATES = ("x", "h", "c", "m")
WEIGHTS = ("Wx", "Wh", "Wm", "Wo", "Wlast")
LN_NAMES = tuple(f"ln.{c}.{p}" for c in ("x", "h", "m", "o") for p in ("weight", "bias"))
OUTS = ("h_new", "c_new", "m_new", "delta_c", "delta_m")
LOSSES = {"full": OUTS, "h_only": ("h_new",), "c_dm": ("c_new", "delta_m"), "two_step": OUTS}
ALL = STATES + WEIGHTS

Case = collections.namedtuple("Case", "shape prec plan exp det grads loss layout")


def _c(shape, prec, plan, exp="0", det=0, grads=ALL, loss="full", layout="nchw"):
    return Case(tuple(shape), prec, dict(plan), exp, det, tuple(grads), loss, layout)


_S17x49 = (8, 32, 17, 49, 5, 0)        # 2 x 4 c5 tiles per image, ragged on both axes (17 = 16 + 1, 49 = 48 + 1)
_S17x17 = (8, 32, 17, 17, 5, 0)        # 2 x 2 c5 tiles per image
_S9x33 = (8, 32, 9, 33, 5, 0)          # 1 x 3 c5 tiles per image, ragged on both axes; Cin + Ch = 40 < 64: one gate chunk
_KS_MID_32 = (1, 1, 4, 2, 2)           # ks_mid (2, 2, 4, 2, 2) under the K / 32 cap at Ch = 32: conv_o's adjoints get 1
_KS_SMALL_32 = (1, 1, 6, 3, 3)         # ks_small (4, 4, 6, 3, 3) under the same cap

CASES = {
    # ---- forward C5 (unsplit) ------------------------------------------------------------------------------------------------------
    # 48 tiles: the smallest grid on C5; nt_o = 2 (48 * 1 < 384). Backward: 48 tiles -> ks_mid
    "c5_nt2_ragged": _c(_S17x49 + (6,), "bf16x3", dict(route=C5, nt_o=2, ks_g=0, last_c1=0, stw=1, c5=1, c5_ks=_KS_MID_32, n_slices=32, stw_ns=15)),
    # 96 tiles: the backward's c5 launches unsplit as well
    "c5_bwd_unsplit": _c(_S17x49 + (12,), "bf16x3", dict(route=C5, nt_o=2, stw=1, c5=1, c5_ks=(1, 1, 1, 1, 1), n_slices=32, stw_ns=30)),
    # 384 tiles of a 17 x 1 map: nt_o = 4
    "c5_nt4": _c((8, 32, 17, 1, 5, 0, 192), "bf16x3", dict(route=C5, nt_o=4, stw=1, c5=1, c5_ks=(1, 1, 1, 1, 1), ksplit_l=1, stw_ns=8)),
    # Ch = 96: conv_o's N tiles are 32 wide here (nt_o = 2: three full ones); the gate groups' 7 * 96 = 672 columns: five 128-wide + a 32-wide one
    "c5_ch96": _c((8, 96, 17, 1, 5, 0, 24), "bf16x3", dict(route=C5, nt_o=2, stw=1, c5=1, c5_ks=(2, 2, 4, 2, 2))),
    # ... and with 64-wide N tiles (nt_o = 4 from 192 tiles on): a full tile and a half-empty one
    "c5_ch96_nt4": _c((8, 96, 17, 1, 5, 0, 96), "bf16x3", dict(route=C5, nt_o=4, stw=1, c5=1, c5_ks=(1, 1, 1, 1, 1))),
    "c5_det": _c(_S17x49 + (6,), "bf16x3", dict(route=C5, nt_o=2, ksplit_l=1, stw=1, c5=1, c5_ks=_KS_MID_32), det=1),
    # ---- forward C5K (K-split jobs) ------------------------------------------------------------------------------------------------
    # 6 tiles: ks_small, the K / 32 cap bites
    "c5k_ks1_ragged": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K, nt_o=2, ks_g=1, ks_o=2, stw=1, c5=1, c5_ks=_KS_SMALL_32, n_slices=12, stw_ns=2)),
    "c5k_ks3": _c((32, 64, 16, 16, 5, 0, 2), "bf16x3", dict(route=C5K, nt_o=2, ks_g=3, ks_o=4, last_c1=0, stw=1, c5=1, c5_ks=(2, 2, 6, 3, 3), n_slices=4, stw_ns=1)),
    # the model's width at B = 2: six chunks each; conv_last on the streaming 1x1 kernel
    "c5k_ks6_c1": _c((64, 128, 16, 16, 5, 0, 2), "bf16x3", dict(route=C5K, nt_o=2, ks_g=6, ks_o=6, last_c1=1, stw=1, c5=1, c5_ks=(4, 4, 6, 3, 3))),
    # 28 tiles of a 1 x 17 map at Ch = 128: 28 * 2 * 6 >= 320 -> nt_o = 4
    "c5k_nt4": _c((8, 128, 1, 17, 5, 0, 14), "bf16x3", dict(route=C5K, nt_o=4, ks_g=2, ks_o=6, last_c1=1, stw=1, c5=1, c5_ks=(2, 2, 4, 2, 2))),
    "c5k_det": _c(_S17x17 + (5,), "bf16x3", dict(route=C5K, ks_g=1, ks_o=2, ksplit_l=1, stw=1, c5=1, c5_ks=_KS_MID_32, n_slices=30, stw_ns=6), det=1),
    # ---- forward GEN1 --------------------------------------------------------------------------------------------------------------
    "gen1_f32_k5": _c((8, 32, 9, 17, 5, 0, 2), "f32", dict(route=GEN1, o_split=8, mw_g=1, ksplit_l=8, stw=0, c5=0, n_slices=8)),
    "gen1_k3": _c((8, 16, 9, 17, 3, 0, 2), "bf16x3", dict(route=GEN1, o_split=2, ksplit_l=2, stw=0, c5=0)),
    "gen1_k7": _c((8, 16, 9, 17, 7, 0, 2), "bf16x3", dict(route=GEN1, o_split=2, stw=0, c5=0)),
    # Ch = 24 (in 8s, not in 32s): the forward stays on the first generation, the backward takes stw + K-split c5 — the mixed path
    "gen1_ch24_mixed": _c((8, 24, 17, 17, 5, 0, 5), "bf16x3", dict(route=GEN1, o_split=4, stw=1, c5=1, c5_ks=(1, 1, 4, 2, 2), stw_ns=6)),
    "gen1_cin1": _c((1, 8, 9, 17, 3, 0, 2), "f32", dict(route=GEN1, o_split=2, stw=0, c5=0)),
    "gen1_cin3": _c((3, 8, 9, 17, 5, 0, 2), "bf16x3", dict(route=GEN1, o_split=2, stw=0, c5=0)),
    "gen1_ch5": _c((3, 5, 9, 17, 3, 0, 2), "f32", dict(route=GEN1, o_split=2, stw=0, c5=0)),           # scalar staging and weight-gradient loads
    "gen1_1x1_map": _c((4, 8, 1, 1, 3, 0, 3), "f32", dict(route=GEN1, o_split=2, n_slices=3)),
    # 384 tiles of 8 x 16: conv_o fused with the gate by grid size, the gate launch in its 8-wave form, conv_last unsplit
    "gen1_fused_grid_8wave": _c((8, 32, 1, 17, 3, 0, 192), "bf16x3", dict(route=GEN1, o_split=0, mw_g=2, mw_o=1, ksplit_l=1, dg_ksplit=(1, 1, 1, 1, 1))),
    # ... and by deterministic mode on a grid that would split
    "gen1_fused_det": _c((8, 16, 9, 17, 3, 0, 2), "bf16x3", dict(route=GEN1, o_split=0, ksplit_l=1, dg_ksplit=(1, 1, 1, 1, 1)), det=1),
    # the c5 shape held on the first generation in both directions: what a failure of a c5 case is compared with
    "gen1_forced": _c(_S9x33 + (2,), "bf16x3", dict(route=GEN1, o_split=4, stw=0, c5=0), exp="ST_FWD_GEN1|ST_DGRAD_GEN1|ST_WGRAD_GEN1"),
    # ---- LayerNorm variant: ragged maps, odd batch ---------------------------------------------------------------------------------
    "k5_ln": _c((5, 12, 9, 17, 5, 1, 3), "f32", dict(route=LN, stw=0, c5=0), grads=ALL + LN_NAMES),
    "k3_ln": _c((4, 8, 9, 17, 3, 1, 3), "bf16x3", dict(route=LN, stw=0, c5=0), grads=ALL + LN_NAMES),
    # ---- plain bf16, forward only. c5 takes bf16x3 alone (c5_shape_ok): both run the first generation, one at a C5 case's shape (conv_o fused with
    #      the gate), one on a small grid with conv_o K-split ------------------------------------------------------------------------------------------
    "plain_bf16_c5_shape": _c((8, 32, 17, 1, 5, 0, 192), "bf16", dict(route=GEN1, o_split=0, mw_g=2), grads=()),
    "plain_bf16_small": _c((8, 16, 9, 17, 3, 0, 2), "bf16", dict(route=GEN1, o_split=2), grads=()),
    # ---- backward with a frozen weight: no stw, hence no c5 — the first generation behind a C5 / C5K forward (fine-tuning) ----------
    "frozen_wlast_c5": _c(_S17x49 + (6,), "bf16x3", dict(route=C5, stw=0, c5=0, c5_ks=(0,) * 5, dg_ksplit=(1, 1, 4, 4, 4)), grads=STATES + WEIGHTS[:4]),
    "only_wx_c5k": _c(_S17x17 + (5,), "bf16x3", dict(route=C5K, stw=0, c5=0, n_slices=30, dg_ksplit=(1, 1, 9, 8, 6)), grads=STATES + ("Wx",)),
    # ---- data gradients as subsets (all weights wanted: stw + c5) ------------------------------------------------------------------
    "dx_only": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K, stw=1, c5=1), grads=("x",) + WEIGHTS),
    "dh_dc_dm": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K, stw=1, c5=1), grads=("h", "c", "m") + WEIGHTS),
    "dx_only_gen1": _c((8, 16, 9, 17, 3, 0, 2), "f32", dict(route=GEN1, stw=0), grads=("x",) + WEIGHTS),
    "dh_dc_dm_gen1": _c((8, 16, 9, 17, 3, 0, 2), "f32", dict(route=GEN1, stw=0), grads=("h", "c", "m") + WEIGHTS),
    # ---- missing incoming gradients: conv_o / conv_last get the exact zero under c_dm ----------------------------------------------
    "h_only_c5k": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K, stw=1, c5=1), loss="h_only"),
    "c_dm_c5k": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K, stw=1, c5=1), loss="c_dm"),
    "h_only_gen1": _c((8, 16, 9, 17, 3, 0, 2), "f32", dict(route=GEN1), loss="h_only"),
    "c_dm_gen1": _c((8, 16, 9, 17, 3, 0, 2), "f32", dict(route=GEN1), loss="c_dm"),
    # ---- two chained steps on split-format shadows (Cin == Ch: h_new is the second step's x and h) ---------------------------------
    "two_step_shadows_c5k": _c((32, 32, 9, 33, 5, 0, 2), "bf16x3", dict(route=C5K, stw=1, c5=1), loss="two_step"),
    "two_step_shadows_c5": _c((32, 32, 17, 1, 5, 0, 24), "bf16x3", dict(route=C5, stw=1, c5=1, c5_ks=_KS_MID_32), loss="two_step"),
    # ---- input layouts ------------------------------------------------------------------------------------------------------------
    "channels_last_c5k": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K), layout="channels_last"),
    "sliced_c5k": _c(_S9x33 + (2,), "bf16x3", dict(route=C5K), layout="sliced"),
    "sliced_gen1": _c((3, 8, 9, 17, 5, 0, 2), "f32", dict(route=GEN1), layout="sliced"),
}

# What the table must reach (tests/test_stlstm_host.py asserts the sets themselves): (field, value) pairs, plan fields under conditions.
REQUIRED = {
    "routes": {LN, GEN1, C5, C5K},
    "c5_nt_o": {2, 4}, "c5k_nt_o": {2, 4}, "c5k_ks_g": {1, 2, 3, 6}, "c5k_ks_o": {2, 4, 6},
    "gen1_o_split": {0, 2, 4, 8}, "gen1_mw_g": {1, 2}, "ksplit_l": {1, 2, 4, 8}, "last_c1": {0, 1},
    "bwd": {(1, 1), (0, 0)},                                                   # (stw, c5); c5 never runs without stw
    "c5_ks": {(1, 1, 1, 1, 1), _KS_MID_32, _KS_SMALL_32, (2, 2, 4, 2, 2), (2, 2, 6, 3, 3), (4, 4, 6, 3, 3), (0, 0, 0, 0, 0)},
    "n_slices": {3, 4, 8, 12, 28, 30, 32}, "stw_ns": {0, 1, 2, 3, 6, 8, 15, 30},
}


def reached(plans):
    """The sets of REQUIRED, from {case: full plan dict} as the library answers."""
    P = list(plans.values())
    on = lambda r: [p for p in P if p["route"] == r]
    return {
        "routes": {p["route"] for p in P},
        "c5_nt_o": {p["nt_o"] for p in on(C5)}, "c5k_nt_o": {p["nt_o"] for p in on(C5K)},
        "c5k_ks_g": {p["ks_g"] for p in on(C5K)}, "c5k_ks_o": {p["ks_o"] for p in on(C5K)},
        "gen1_o_split": {p["o_split"] for p in on(GEN1)}, "gen1_mw_g": {p["mw_g"] for p in on(GEN1)},
        "ksplit_l": {p["ksplit_l"] for p in P if not p["last_c1"]}, "last_c1": {p["last_c1"] for p in P},
        "bwd": {(p["stw"], p["c5"]) for p in P if p["route"] != LN},
        "c5_ks": {tuple(p["c5_ks"]) for p in P if p["route"] != LN},
        "n_slices": {p["n_slices"] for p in P if p["route"] != LN}, "stw_ns": {p["stw_ns"] for p in P if p["route"] != LN},
    }


def all_weight_grads(case):
    return int(all(w in CASES[case].grads for w in WEIGHTS))


def _dims(shape):
    Cin, Ch, H, W, k, ln, B = shape
    return Cin, Ch, H, W, k, bool(ln), B


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    Cin, Ch, H, W, k, ln, B = _dims(shape)
    rn = lambda name, sh, scale=1.0: seeded_randn(sh, name_seed(f"stlstm.{shape}.{name}"), scale)
    t = {"x": rn("x", (B, Cin, H, W), 0.5)}
    for n in ("h", "c", "m"):
        t[n] = rn(n, (B, Ch, H, W), 0.5)
    for n, sh in (("Wx", (7 * Ch, Cin, k, k)), ("Wh", (4 * Ch, Ch, k, k)), ("Wm", (3 * Ch, Ch, k, k)), ("Wo", (Ch, 2 * Ch, k, k)), ("Wlast", (Ch, 2 * Ch, 1, 1))):
        t[n] = rn(n, sh, fan_in_scale(sh))
    if ln:
        for c, mult in (("x", 7), ("h", 4), ("m", 3), ("o", 1)):
            t[f"ln.{c}.weight"] = 1.0 + rn(f"ln.{c}.weight", (mult * Ch, H, W), 0.1)
            t[f"ln.{c}.bias"] = rn(f"ln.{c}.bias", (mult * Ch, H, W), 0.1)
    for o in OUTS:
        t["g." + o] = rn("g." + o, (B, Ch, H, W))
        t["g2." + o] = rn("g2." + o, (B, Ch, H, W))
    return t


def inputs(case):
    """name -> float32 CPU tensor: x, h, c, m, the five weights, the LayerNorm tensors (LayerNorm cases), the cotangents g.<out> and, for
    the second of two chained steps, g2.<out>. Cases of one shape share their draws; nobody writes them."""
    return _inputs(CASES[case].shape)


def leaves_of(shape):
    return ALL + (LN_NAMES if shape[5] else ())


def evaluate(step, t, shape, grads, loss):
    """Outputs and the gradients of the leaves `grads`. `step(x, h, c, m, lv)` -> the five outputs (lv: name -> leaf); `t` as from inputs(),
    on the device, in the dtype and the layouts of the run. The loss is the sum of the named outputs times their fixed cotangents;
    `two_step` runs a second step of the same cell on (x, h, c, m) = (h_new, h_new, c_new, m_new) of the first and sums both steps' losses.
    Only the leaves of `grads` require a gradient (none: a forward under no_grad); one that the loss does not reach has the zero gradient."""
    lv = {n: t[n].detach().requires_grad_(n in grads) for n in leaves_of(shape)}
    with torch.enable_grad() if grads else torch.no_grad():
        outs = step(lv["x"], lv["h"], lv["c"], lv["m"], lv)
        res = {n: o.detach() for n, o in zip(OUTS, outs)}
        if not grads:
            return res
        total = sum((o * t["g." + n]).sum() for n, o in zip(OUTS, outs) if n in LOSSES[loss])
        if loss == "two_step":
            outs2 = step(outs[0], outs[0], outs[1], outs[2], lv)
            res.update({"step2." + n: o.detach() for n, o in zip(OUTS, outs2)})
            total = total + sum((o * t["g2." + n]).sum() for n, o in zip(OUTS, outs2))
        total.backward()
    for n in grads:
        res["grad." + n] = torch.zeros_like(lv[n]) if lv[n].grad is None else lv[n].grad.detach()
    return res


def ref_step(shape):
    ln = bool(shape[5])

    def step(x, h, c, m, lv):
        p = {"conv_x.0.weight": lv["Wx"], "conv_h.0.weight": lv["Wh"], "conv_m.0.weight": lv["Wm"], "conv_o.0.weight": lv["Wo"], "conv_last.weight": lv["Wlast"]}
        if ln:
            for cname in ("x", "h", "m", "o"):
                p[f"conv_{cname}.1.weight"], p[f"conv_{cname}.1.bias"] = lv[f"ln.{cname}.weight"], lv[f"ln.{cname}.bias"]
        return torch_ref.stlstm_cell(x, h, c, m, p, layer_norm=ln)
    return step


@functools.lru_cache(maxsize=None)
def _cpu_all(shape, with_grads, loss, dtype):
    """Every gradient of a (shape, loss) on the CPU in `dtype`: computed once, shared by the cases of that shape, never written."""
    t = {n: v.to(dtype) for n, v in _inputs(shape).items()}
    return evaluate(ref_step(shape), t, shape, leaves_of(shape) if with_grads else (), loss)


def cpu(case, dtype=torch.float64):
    """The reference of one case: the five outputs (of both steps for `two_step`) and the gradients of the leaves it asks for."""
    C = CASES[case]
    every = _cpu_all(C.shape, bool(C.grads), C.loss, dtype)
    return {n: v for n, v in every.items() if not n.startswith("grad.") or n[5:] in C.grads}


def relmax(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))
