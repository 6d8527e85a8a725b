"""The ConvLSTM sequence (vpx_convlstm_seq_fwd / _bwd behind `ops.convlstm_seq`; csrc/convlstm_fwd_api.hip, csrc/convlstm_bwd_api.hip) in plain
float64, with the case table of tests/test_gpu_convlstm_routes.py (GPU parity) and tests/test_convlstm_host.py (the plan every case takes, the
workspace contract in a dry run, the condition of the inputs, on the CPU). Nothing here touches the GPU or imports the package.

The statement: `oracle.torch_ref.convlstm_hzzone_seq` on the CPU under autograd, on the float32 inputs cast up; gate order 1 (rows i, f, o, g)
by the row permutation of tests/test_gpu_cell2.py. Inputs as there: W randn / sqrt((Cin + Ch) k^2), bias 0.1 randn, x uniform [0, 1), h0 / c0
0.5 randn, peepholes 0.1 randn [1, Ch, H, W], cotangents randn. The operator has no kinks (sigmoid, tanh, products): no element and no case is
left out of a comparison.

A case is a shape (Cin, Ch, H, W, k, B, T), a precision, the present operands (letters of "xspb": x, initial state, peepholes, bias), the gate
order, option settings (names of _lib.OPT_*), experiment bits (names of _lib.Exp joined by '|'), the deterministic setting, the leaves whose
gradients the call is asked for (none: inference under no_grad), a loss — and the plan it is there to reach: the fields of
vpx_convlstm_plan_info (include/vpx.h) it must show, written next to the shape. tests/test_convlstm_host.py holds the table to the library's
own answer.

How the shapes follow from convlstm_layout (csrc/vpx_host.h). First-generation pixel tiles are 8 x 16: m = B ceil(H/8) ceil(W/16), n =
ceil(Ch/32). m n >= 256: the fused launch (8 waves from B ceil(H/16) ceil(W/16) n >= 512, bf16 modes). Below: cell3 where it applies (bf16x3,
3x3, Ch in 16s up to 96, maps in whole 16x16 tiles); else the K split, pick_ksplit = min(ceil(256 / (m N tiles)), K stages, 16), stages of 32
channels per operand; with T > 1 and x the projection is hoisted and the step splits over the h stages alone. The deterministic mode has no K
split: the fused launch again. cell2 (bf16x3 or plain bf16, 3x3, Cin and Ch in 16s, H >= 16) takes what is left of m n >= 256 from
B ceil(H/32) ceil(W/16) n >= 64 workgroups on (OPT_CELL2 = 2: everywhere): its q form on maps in whole 16x16 tiles with Ch in 32s, and an
inference call of at most 256 half-tile workgroups runs as c3. Narrow maps (1 x 17, 17 x 1) buy two or three tiles for 17 pixels."""
import collections
import functools

import numpy as np
import torch

from golden_util import name_seed, seeded_rand, seeded_randn
from oracle import torch_ref

BARS = {"f32": (1e-5, 5e-5), "bf16x3": (6e-5, 2e-4), "bf16": (1e-2, None)}   # (outputs, gradients) in max|d| / max|ref|; plain bf16: forward only
COND = (5e-6, 2.5e-5)                                                        # the fp32 CPU run against fp64: half the f32 bars

FUSED, KSPLIT, HOIST, CELL3, CELL2, C3 = range(6)                            # vpx_convlstm_plan_info.route (VPX_CL_ROUTE_*)
GEN1 = (FUSED, KSPLIT, HOIST)
LEAVES = ("x", "h0", "c0", "W", "b", "Wci", "Wcf", "Wco")
OUTS = ("out", "hT", "cT")
LOSSES = {"out_cT": ("out", "cT"), "out": ("out",), "hT_cT": ("hT", "cT")}
GEN1_OPTS = {"OPT_CELL2": 0, "OPT_CELL3": 0}
FORCE2 = {"OPT_CELL2": 2}

Case = collections.namedtuple("Case", "shape prec ops order opts exp det grads loss plan")


def present(ops):
    """The leaves a call with these operands has."""
    return tuple(n for n in LEAVES if n == "W" or {"x": "x", "h0": "s", "c0": "s", "b": "b"}.get(n, "p") in ops)


def _c(shape, prec, plan, ops="xspb", order=0, opts=None, exp="0", det=0, grads=None, drop=(), loss="out_cT"):
    """grads: None = every present leaf, () = inference; drop: leaves of the default set that do not require a gradient."""
    g = tuple(n for n in (present(ops) if grads is None else grads) if n not in drop)
    assert all(n in present(ops) for n in g) and not (prec == "bf16" and g)
    return Case(tuple(shape), prec, ops, order, dict(opts or {}), exp, det, g, loss, dict(plan))


_Q = (16, 32, 32, 16, 3, 2, 2)            # q-form shape: 2 x 1 half tiles per image, one 32-channel N tile; forced onto cell2 at B = 2
_Q64 = (16, 32, 32, 16, 3, 64, 2)         # ... at B = 64: m n = 64 * 4 = 256 and 64 cell2 workgroups — the product's own choice; 128 half tiles: c3
_RAG = (16, 32, 24, 20, 3, 2, 3)          # ragged on both axes (24 = 16 + 8, 20 = 16 + 4): no q form, no cell3
_N17 = (16, 32, 17, 1, 3, 86, 2)          # 17 x 1 map: m = 86 * 3 = 258, 86 cell2 workgroups, 1462 pixels
_C3S = (16, 16, 16, 16, 3, 2, 3)          # cell3's smallest: one 16x16 tile per image, Ch = 16
_CH48 = (16, 48, 32, 16, 3, 2, 2)         # Ch = 48: whole 16-channel stages, no whole 32-channel N tiles
_H16 = (16, 32, 16, 32, 3, 2, 2)          # 16-row maps: cell2 on its q form only
_C3T1 = (16, 32, 16, 16, 3, 2, 1)         # cell3, one step
_QT1 = (16, 32, 32, 16, 3, 2, 1)          # the q shape, one step
_QT3 = (16, 32, 32, 16, 3, 2, 3)          # the q shape, three steps (plain bf16)
_C96 = (3, 96, 16, 32, 3, 2, 2)           # cell3's widest on a 16x32 map, Cin = 3
_HST = (16, 64, 9, 17, 3, 2, 3)           # small ragged grid (m = 8), two 32-channel h stages: the hoist with hh_split = 2
_BWD_Q = dict(dgrad=1, dgrad_qform=1, d_mw=0, wgrad=1, dG_f32=0)          # behind a q-form cell2 forward: conv2 + wgrad2 on the reserve
_BWD_G1 = dict(dgrad=0, dgrad_qform=0, dG_f32=1)                          # first-generation data gradient on fp32 dG

CASES = {
    # ---- FUSED ---------------------------------------------------------------------------------------------------------------------
    # by grid size in f32: m = 128 * 1 * 2 = 256. Cin = 1; eight gate-backward batch slices: the peephole gradients take the sliced reduce
    "fused_f32_grid": _c((1, 8, 1, 17, 3, 128, 3), "f32", dict(route=FUSED, mw=1, ksplit=0, wgrad=0, gate_slices=8, dgrad_cols=9, **_BWD_G1)),
    # by deterministic mode on a grid that would split (m = 8); Cin = 3, k = 5: launch_wgrad behind a bf16x3 forward
    "fused_det_k5": _c((3, 8, 9, 17, 5, 2, 3), "bf16x3", dict(route=FUSED, mw=1, ksplit=0, wgrad=0, gate_slices=2, **_BWD_G1), det=1),
    # the 8-wave form: 256 * 1 * 2 * 1 = 512 double tiles; Cin = 8 keeps cell2 away, and in 8s: wgrad2 on operands the backward converts
    "fused_8wave": _c((8, 32, 1, 17, 3, 256, 2), "bf16x3", dict(route=FUSED, mw=2, wgrad=2, gate_slices=8, **_BWD_G1)),
    # a 1x1 map, k = 1, in deterministic mode (m = 3)
    "fused_det_1x1_k1": _c((3, 8, 1, 1, 1, 3, 3), "f32", dict(route=FUSED, mw=1, wgrad=0, gate_slices=3, **_BWD_G1), det=1),
    # ---- KSPLIT --------------------------------------------------------------------------------------------------------------------
    # T = 1: nothing to hoist. One stage per operand: two K ranges. B = 1: one gate-backward slice
    "ksplit_t1": _c((8, 16, 9, 17, 3, 1, 1), "f32", dict(route=KSPLIT, ksplit=2, hh_split=0, wgrad=0, gate_slices=1, **_BWD_G1)),
    # T > 1 without x, the hoist's x-less twin: four stages (2 + 2) and 16 workgroups: four K ranges, of which the call has the h stages only
    "ksplit_nox": _c((64, 64, 9, 17, 3, 2, 3), "bf16x3", dict(route=KSPLIT, ksplit=4, hoist_convq=0, wgrad=2, dgrad_cols=64, **_BWD_G1), ops="spb"),
    "ksplit_nox_f32_k7": _c((3, 5, 9, 17, 7, 2, 2), "f32", dict(route=KSPLIT, ksplit=2, wgrad=0, **_BWD_G1), ops="spb"),
    # ---- HOIST ---------------------------------------------------------------------------------------------------------------------
    # the projection on convq: bf16x3, Cin in 16s, a ragged map keeps cell3 away
    "hoist_convq": _c(_HST, "bf16x3", dict(route=HOIST, ksplit=0, hh_split=2, hoist_convq=1, wgrad=2, **_BWD_G1)),
    "hoist_gen1_on_convq_shape": _c(_HST, "bf16x3", dict(route=HOIST, hh_split=2, hoist_convq=0), exp="HOIST_GEN1"),
    "hoist_f32": _c((8, 64, 9, 17, 3, 2, 3), "f32", dict(route=HOIST, hh_split=2, hoist_convq=0, wgrad=0, **_BWD_G1)),
    # without an initial state: step 0 is the pointwise kernel alone
    "hoist_no_state": _c(_HST, "bf16x3", dict(route=HOIST, hh_split=2, hoist_convq=1), ops="xpb"),
    "hoist_f32_k7_ch5": _c((3, 5, 9, 17, 7, 2, 2), "f32", dict(route=HOIST, ksplit=0, hh_split=1, hoist_convq=0, wgrad=0, **_BWD_G1)),
    # ---- CELL3 ---------------------------------------------------------------------------------------------------------------------
    "cell3_ch16": _c(_C3S, "bf16x3", dict(route=CELL3, hoist_convq=1, ksplit=0), grads=()),
    # Ch = 96 on a 16x32 map, Cin = 3: the projection on the first generation; a saving call
    "cell3_ch96_cin3_train": _c(_C96, "bf16x3", dict(route=CELL3, hoist_convq=0, wgrad=0, **_BWD_G1)),
    "cell3_train": _c(_C3S, "bf16x3", dict(route=CELL3, hoist_convq=1, wgrad=2, **_BWD_G1)),
    "cell3_nox": _c(_C3S, "bf16x3", dict(route=CELL3, hoist_convq=0), ops="spb", grads=()),
    "cell3_t1": _c(_C3T1, "bf16x3", dict(route=CELL3, hoist_convq=1), grads=()),
    # ---- CELL2, the product's own choice -------------------------------------------------------------------------------------------
    "cell2_nonq_default": _c(_N17, "bf16x3", dict(route=CELL2, qform=0, dgrad=1, dgrad_qform=1, wgrad=1, dG_f32=0, dgrad_cols=48)),
    "cell2_q_default_train": _c(_Q64, "bf16x3", dict(route=CELL2, qform=1, cell2x=0, gate_slices=8, **_BWD_Q)),
    # ---- C3 ------------------------------------------------------------------------------------------------------------------------
    "c3_default": _c(_Q64, "bf16x3", dict(route=C3, qform=1, c3nt=4), grads=()),
    "c3_narrow_no_state": _c(_Q, "bf16x3", dict(route=C3, qform=1, c3nt=2), ops="xpb", opts=FORCE2, exp="C3_NARROW", grads=()),
    "c3_no_state": _c(_Q, "bf16x3", dict(route=C3, c3nt=4), ops="xpb", opts=FORCE2, grads=()),
    "c3_narrow": _c(_Q, "bf16x3", dict(route=C3, c3nt=2), opts=FORCE2, exp="C3_NARROW", grads=()),
    # its twin on the half tile
    "no_c3_half_tile": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, c3nt=0), opts=FORCE2, exp="NO_C3", grads=()),
    # ---- CELL2 forced onto B = 2 ---------------------------------------------------------------------------------------------------
    "cell2_nonq_ragged": _c(_RAG, "bf16x3", dict(route=CELL2, qform=0, dgrad=1, dgrad_qform=1, wgrad=1, dG_f32=0), opts=FORCE2),
    # Ch = 48: whole 16-channel stages, no whole 32-channel N tiles; gate order 1, no peepholes
    "cell2_nonq_ch48_ifog": _c(_CH48, "bf16x3", dict(route=CELL2, qform=0, wgrad=1), ops="xsb", order=1, opts=FORCE2),
    # the 16-row special case
    "cell2_q_h16": _c(_H16, "bf16x3", dict(route=CELL2, qform=1, **_BWD_Q), opts=FORCE2),
    # operand sets of the q form: x only, T >= 2 (two packs); x only, T = 1 (c_0 = 0: the gradients of Wci and Wcf are exactly zero); state only
    "cell2_q_x_only_two_packs": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, **_BWD_Q), ops="xpb", opts=FORCE2),
    "cell2_q_x_only_t1": _c(_QT1, "bf16x3", dict(route=CELL2, qform=1, **_BWD_Q), ops="xpb", opts=FORCE2),
    "cell2_q_state_only": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, dgrad_cols=32, **_BWD_Q), ops="spb", opts=FORCE2),
    "cell2_q_ifog_no_bias": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, **_BWD_Q), ops="xs", order=1, opts=FORCE2),
    "cell2_full_tile": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, cell2x=0, **_BWD_Q), opts=FORCE2, exp="CELL2_FULL_TILE"),
    "cell2x": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, cell2x=1, **_BWD_Q), opts=FORCE2, exp="CELL2X"),
    "cell2x_colsplit": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, cell2x=1, **_BWD_Q), opts=FORCE2, exp="CELL2X|CELL2X_COLSPLIT"),
    # the 32x32x16 MFMA form on the q shape, both directions
    "cell2_mfma0": _c(_Q, "bf16x3", dict(route=CELL2, qform=0, dgrad=1, dgrad_qform=0, wgrad=1, dG_f32=0), opts={"OPT_CELL2": 2, "OPT_MFMA_SHAPE": 0}),
    "cell2_plain_bf16": _c(_QT3, "bf16", dict(route=CELL2, qform=1), opts=FORCE2, grads=()),
    "cell2_q_infer_no_c3": _c(_Q, "bf16x3", dict(route=CELL2, qform=1), ops="spb", opts=FORCE2, exp="NO_C3", grads=()),
    # ---- backward: subsets of the leaves, losses, deterministic mode ------------------------------------------------------------------
    # x given but not requiring a gradient: the data gradient writes the h columns only
    "cell2_no_dx": _c(_Q, "bf16x3", dict(route=CELL2, dgrad_cols=32, **_BWD_Q), opts=FORCE2, drop=("x",)),
    "cell2_no_dstate": _c(_Q, "bf16x3", dict(route=CELL2, dgrad_cols=48, **_BWD_Q), opts=FORCE2, drop=("h0", "c0")),
    "cell2_w_frozen": _c(_Q, "bf16x3", dict(route=CELL2, dgrad=1, wgrad=0, n_slices=0, dG_f32=0), opts=FORCE2, drop=("W",)),
    "cell2_only_w": _c(_Q, "bf16x3", dict(route=CELL2, dgrad_cols=32, **_BWD_Q), opts=FORCE2, grads=("W",)),
    "cell2_loss_out": _c(_Q, "bf16x3", dict(route=CELL2, **_BWD_Q), opts=FORCE2, loss="out"),
    "cell2_loss_hT_cT": _c(_Q, "bf16x3", dict(route=CELL2, **_BWD_Q), opts=FORCE2, loss="hT_cT"),
    "cell2_q_det": _c(_Q, "bf16x3", dict(route=CELL2, qform=1, **_BWD_Q), opts=FORCE2, det=1),
    "gen1_no_dx": _c((8, 16, 9, 17, 3, 2, 3), "f32", dict(route=HOIST, dgrad_cols=16, wgrad=0, **_BWD_G1), drop=("x",)),
    "gen1_w_frozen": _c((8, 16, 9, 17, 3, 2, 3), "f32", dict(route=HOIST, wgrad=0, n_slices=0, **_BWD_G1), drop=("W",)),
    "gen1_only_w": _c((8, 16, 9, 17, 3, 2, 3), "f32", dict(route=HOIST, dgrad_cols=16, wgrad=0, **_BWD_G1), grads=("W",)),
    "gen1_loss_hT_cT": _c((8, 16, 9, 17, 3, 2, 3), "f32", dict(route=HOIST, wgrad=0, **_BWD_G1), loss="hT_cT"),
    "gen1_loss_out": _c((8, 16, 9, 17, 3, 2, 3), "f32", dict(route=HOIST, wgrad=0, **_BWD_G1), loss="out"),
    # ---- first-generation twins: the shape of each second / third generation family with OPT_CELL2 = 0, OPT_CELL3 = 0 ----------------------
    "twin_q": _c(_Q, "bf16x3", dict(route=HOIST, hoist_convq=1, wgrad=2, **_BWD_G1), opts=GEN1_OPTS),
    "twin_q_infer_no_state": _c(_Q, "bf16x3", dict(route=HOIST), ops="xpb", opts=GEN1_OPTS, grads=()),
    "twin_ragged": _c(_RAG, "bf16x3", dict(route=HOIST, wgrad=2, **_BWD_G1), opts=GEN1_OPTS),
    "twin_n17": _c(_N17, "bf16x3", dict(route=FUSED, mw=1, wgrad=2, **_BWD_G1), opts=GEN1_OPTS),
    "twin_cell3": _c(_C3S, "bf16x3", dict(route=HOIST, hoist_convq=1, wgrad=2, **_BWD_G1), opts=GEN1_OPTS),
    "twin_cell3_ch96_cin3": _c(_C96, "bf16x3", dict(route=HOIST, hoist_convq=0, wgrad=0, **_BWD_G1), opts=GEN1_OPTS),
    "twin_q_det": _c(_Q, "bf16x3", dict(route=FUSED, wgrad=2, **_BWD_G1), opts=GEN1_OPTS, det=1),
    "twin_q_state_only": _c(_Q, "bf16x3", dict(route=KSPLIT, wgrad=2, dgrad_cols=32, **_BWD_G1), ops="spb", opts=GEN1_OPTS),
    "twin_q64": _c(_Q64, "bf16x3", dict(route=FUSED, mw=1, wgrad=2, gate_slices=8, **_BWD_G1), opts=GEN1_OPTS),
    "twin_ch48_ifog": _c(_CH48, "bf16x3", dict(route=HOIST, wgrad=2, **_BWD_G1), ops="xsb", order=1, opts=GEN1_OPTS),
    "twin_h16": _c(_H16, "bf16x3", dict(route=HOIST, wgrad=2, **_BWD_G1), opts=GEN1_OPTS),
    "twin_cell3_t1": _c(_C3T1, "bf16x3", dict(route=KSPLIT, ksplit=2), opts=GEN1_OPTS, grads=()),
    "twin_q_x_only_t1": _c(_QT1, "bf16x3", dict(route=KSPLIT, ksplit=2, wgrad=2, **_BWD_G1), ops="xpb", opts=GEN1_OPTS),
    "twin_plain_bf16": _c(_QT3, "bf16", dict(route=HOIST, hoist_convq=0), opts=GEN1_OPTS, grads=()),
}

# What the table must reach (tests/test_convlstm_host.py asserts the sets themselves, from the library's answers: reached()).
REQUIRED = {
    "routes": {FUSED, KSPLIT, HOIST, CELL3, CELL2, C3},
    "default_options": {CELL2, C3},                                        # routes of the second generation reached without OPT_CELL2
    "fused": {("grid", "f32", 1), ("grid", "bf16x3", 2), ("grid", "bf16x3", 1), ("det", "f32", 1), ("det", "bf16x3", 1)},   # (why, precision, mw)
    "gen1_k": {1, 3, 5, 7}, "gen1_small_cin": {1, 3}, "odd_ch": {5}, "map_1x1": {True},
    "ksplit": {("t1", 2), ("no_x", 2), ("no_x", 4)},
    "hoist": {(1, "bf16x3", "0", 1), (0, "bf16x3", "HOIST_GEN1", 1), (0, "f32", "0", 1), (1, "bf16x3", "0", 0)},   # (hoist_convq, precision, exp, state) at hh_split > 1
    "cell3": {(16, (16, 16), 1, 1, 3, 0), (16, (16, 16), 1, 1, 3, 1), (96, (16, 32), 0, 1, 2, 1), (16, (16, 16), 0, 0, 3, 0), (32, (16, 16), 1, 1, 1, 0)},
    #         (Ch, map, hoist_convq, x present, T, saving)
    "cell2_qform": {0, 1}, "cell2_nonq": {"ragged", "ch48", "mfma0"}, "cell2_h16": {1},
    "cell2_q_operands": {("xs", 2), ("x", 2), ("x", 1), ("s", 2)},         # (operands, T) on the q form
    "cell2_order": {0, 1}, "cell2_peepholes": {0, 1}, "cell2_bias": {0, 1},
    "cell2_exp": {"0", "CELL2_FULL_TILE", "CELL2X", "CELL2X|CELL2X_COLSPLIT", "NO_C3"}, "cell2x": {0, 1},
    "cell2_prec": {"bf16x3", "bf16"},
    "c3": {(4, 1), (4, 0), (2, 1), (2, 0)},                                # (c3nt, state)
    "dgrad": {(0, 0), (1, 0), (1, 1)},                                     # (dgrad, dgrad_qform)
    "wgrad": {0, 1, 2}, "wgrad0_behind": {"f32", "bf16x3_cin3", "k5"},
    "gate_slices": {"1", ">1"}, "peepholes_sliced": {True}, "dG_f32": {0, 1},
    "dropped_leaves": {(), ("x",), ("h0", "c0"), ("W",), ("x", "h0", "c0", "b", "Wci", "Wcf", "Wco")},
    "losses": {"out", "hT_cT", "out_cT"},
    "det_routes": {FUSED, CELL2},
    # every (shape, precision) that a case takes to the second or third generation, each with a forced first-generation case beside it
    "twins": {(_Q, "bf16x3"), (_Q64, "bf16x3"), (_RAG, "bf16x3"), (_N17, "bf16x3"), (_C3S, "bf16x3"), (_C96, "bf16x3"), (_CH48, "bf16x3"), (_H16, "bf16x3"),
              (_C3T1, "bf16x3"), (_QT1, "bf16x3"), (_QT3, "bf16")},
}


REQUIRED["families"] = REQUIRED["twins"]   # ... and no family without its twin: a miss is laid at the route's or at the mode's door by comparing the two


def reached(plans):
    """The sets of REQUIRED, from {case: full plan dict} as the library answers."""
    C = CASES
    on = lambda *routes: [c for c in C if plans[c]["route"] in routes]
    saving = [c for c in C if C[c].grads]
    q = [c for c in on(CELL2) if plans[c]["qform"]]
    why_nonq = lambda s, o: "mfma0" if o.get("OPT_MFMA_SHAPE") == 0 else ("ch48" if s[1] % 32 else "ragged")
    return {
        "routes": {plans[c]["route"] for c in C},
        "default_options": {plans[c]["route"] for c in on(CELL2, C3) if "OPT_CELL2" not in C[c].opts},
        "fused": {("det" if C[c].det else "grid", C[c].prec, plans[c]["mw"]) for c in on(FUSED)},
        "gen1_k": {C[c].shape[4] for c in on(*GEN1)}, "gen1_small_cin": {C[c].shape[0] for c in on(*GEN1)} & {1, 3},
        "odd_ch": {C[c].shape[1] for c in on(*GEN1) if C[c].shape[1] % 8}, "map_1x1": {C[c].shape[2:4] == (1, 1) for c in C} - {False},
        "ksplit": {("t1" if C[c].shape[6] == 1 else "no_x" if "x" not in C[c].ops else "?", plans[c]["ksplit"]) for c in on(KSPLIT)},
        "hoist": {(plans[c]["hoist_convq"], C[c].prec, C[c].exp, int("s" in C[c].ops)) for c in on(HOIST) if plans[c]["hh_split"] > 1 and not C[c].opts},
        "cell3": {(C[c].shape[1], C[c].shape[2:4], plans[c]["hoist_convq"], int("x" in C[c].ops), C[c].shape[6], int(bool(C[c].grads))) for c in on(CELL3)},
        "cell2_qform": {plans[c]["qform"] for c in on(CELL2)},
        "cell2_nonq": {why_nonq(C[c].shape, C[c].opts) for c in on(CELL2) if not plans[c]["qform"]},
        "cell2_h16": {int(C[c].shape[2] == 16) for c in q} - {0},
        "cell2_q_operands": {("".join(o for o in "xs" if o in C[c].ops), C[c].shape[6]) for c in q if C[c].grads},
        "cell2_order": {C[c].order for c in on(CELL2)}, "cell2_peepholes": {int("p" in C[c].ops) for c in on(CELL2)},
        "cell2_bias": {int("b" in C[c].ops) for c in on(CELL2)},
        "cell2_exp": {C[c].exp for c in q}, "cell2x": {plans[c]["cell2x"] for c in q},
        "cell2_prec": {C[c].prec for c in on(CELL2)},
        "c3": {(plans[c]["c3nt"], int("s" in C[c].ops)) for c in on(C3)},
        "dgrad": {(plans[c]["dgrad"], plans[c]["dgrad_qform"]) for c in saving},
        "wgrad": {plans[c]["wgrad"] for c in saving if "W" in C[c].grads},
        "wgrad0_behind": {tag for c in saving if "W" in C[c].grads and plans[c]["wgrad"] == 0
                          for tag, hit in (("f32", C[c].prec == "f32"), ("bf16x3_cin3", C[c].prec == "bf16x3" and C[c].shape[0] == 3), ("k5", C[c].shape[4] == 5)) if hit},
        "gate_slices": {"1" if plans[c]["gate_slices"] == 1 else ">1" for c in saving},
        "peepholes_sliced": {plans[c]["gate_slices"] > 1 and "Wci" in C[c].grads for c in saving} - {False},
        "dG_f32": {plans[c]["dG_f32"] for c in saving},
        "dropped_leaves": {tuple(n for n in present(C[c].ops) if n not in C[c].grads) for c in saving if C[c].ops == "xspb"},
        "losses": {C[c].loss for c in saving},
        "det_routes": {plans[c]["route"] for c in C if C[c].det},
        "twins": {(C[c].shape, C[c].prec) for c in C if C[c].opts == GEN1_OPTS and plans[c]["route"] in GEN1},
        "families": {(C[c].shape, C[c].prec) for c in on(CELL3, CELL2, C3)},
    }


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    Cin, Ch, H, W, k, B, T = shape
    rn = lambda name, sh, scale=1.0: seeded_randn(sh, name_seed(f"convlstm.{shape}.{name}"), scale)
    t = {"W": rn("W", (4 * Ch, Cin + Ch, k, k), 1.0 / np.sqrt((Cin + Ch) * k * k)), "b": rn("b", (4 * Ch,), 0.1),
         "x": seeded_rand((B, T, Cin, H, W), name_seed(f"convlstm.{shape}.x")),
         "h0": rn("h0", (B, Ch, H, W), 0.5), "c0": rn("c0", (B, Ch, H, W), 0.5),
         "g.out": rn("g.out", (B, T, Ch, H, W)), "g.hT": rn("g.hT", (B, Ch, H, W)), "g.cT": rn("g.cT", (B, Ch, H, W))}
    for n in ("Wci", "Wcf", "Wco"):
        t[n] = rn(n, (1, Ch, H, W), 0.1)
    return t


def inputs(case):
    """name -> float32 CPU tensor: the eight leaves (a case uses the ones it has: present()) and the cotangents g.out, g.hT, g.cT. Cases of
    one shape share their draws; nobody writes them."""
    return _inputs(CASES[case].shape)


def evaluate(seq, t, ops, grads, loss):
    """out, hT, cT and the gradients of the leaves `grads`. `seq(x, h0, c0, W, b, Wci, Wcf, Wco)` -> (out, hT, cT), absent operands None;
    `t` as from inputs(), on the device and in the dtype of the run. The loss is the sum of the named outputs times their fixed
    cotangents. Only the leaves of `grads` require a gradient (none: a forward under no_grad)."""
    lv = {n: t[n].detach().requires_grad_(n in grads) for n in present(ops)}
    with torch.enable_grad() if grads else torch.no_grad():
        outs = seq(*(lv.get(n) for n in LEAVES))
        res = {n: o.detach() for n, o in zip(OUTS, outs)}
        if not grads:
            return res
        sum((o * t["g." + n]).sum() for n, o in zip(OUTS, outs) if n in LOSSES[loss]).backward()
    for n in grads:
        res["grad." + n] = torch.zeros_like(lv[n]) if lv[n].grad is None else lv[n].grad.detach()
    return res


def ref_seq(shape, order):
    Cin, Ch, H, W, k, B, T = shape

    def seq(x, h0, c0, Wt, b, Wci, Wcf, Wco):
        if order == 1:   # reference rows are (i, f, o, g): the hzzone restatement wants (i, f, g, o)
            perm = torch.cat([torch.arange(0, 2 * Ch), torch.arange(3 * Ch, 4 * Ch), torch.arange(2 * Ch, 3 * Ch)])
            Wt, b = Wt[perm], None if b is None else b[perm]
        z = torch.zeros(1, Ch, H, W, dtype=Wt.dtype)
        out, (hT, cT) = torch_ref.convlstm_hzzone_seq(x, None if h0 is None else (h0, c0), T, Wt, b, z if Wci is None else Wci, z if Wcf is None else Wcf,
                                                      z if Wco is None else Wco, padding=k // 2)
        return out, hT, cT
    return seq


@functools.lru_cache(maxsize=None)
def _cpu_all(shape, ops, order, with_grads, loss, dtype):
    """Every gradient of a (shape, operands, gate order, loss) on the CPU in `dtype`: computed once, shared by its cases, never written."""
    t = {n: v.to(dtype) for n, v in _inputs(shape).items()}
    return evaluate(ref_seq(shape, order), t, ops, present(ops) if with_grads else (), loss)


def cpu(case, dtype=torch.float64):
    """The reference of one case: out, hT, cT and the gradients of the leaves it asks for."""
    C = CASES[case]
    every = _cpu_all(C.shape, C.ops, C.order, bool(C.grads), C.loss, dtype)
    return {n: v for n, v in every.items() if not n.startswith("grad.") or n[5:] in C.grads}


def relmax(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))
