"""The stage-glue family on the CPU: the fp64 statement of tests/glue_ref.py checked against closed forms; the routes of
csrc/glue_fwd_api.hip / glue_bwd_api.hip restated in Python, checked against the library's own answers (vpx_conv2d_ex_takes_split, vpx_conv2d_ex_bwd_uses_split)
and against the tables — every route has a case, every neighbour falls outside its gate; the conditions under which
tests/test_gpu_glue.py may hold the kernels to the project's bars (the reference's own fp32 run stays inside a fifth of them; next to
nothing sits on the activation's kink); and — in a dry run (VPX_OPT_DRY_RUN, as tests/test_workspace_contract.py) — every case through
every entry point with a workspace of exactly the queried size, and the refusals with their documented codes."""
import ctypes

import pytest
import torch

import glue_ref as R
from vp_suite_amd import _lib
from vp_suite_amd._lib import ConvDesc, Exp

OK, E_ARG, E_WS, E_UNSUPPORTED = 0, -1, -2, -4
WS_BASE = 0x7F0000000000            # fake workspace address (256-byte aligned; never dereferenced in a dry run)
WS_BASE_ODD = WS_BASE + 0x40        # ... and one that is not 256-byte aligned
PRECS = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3}
CASES = R.all_cases()
IDS = [R.case_id(t, i) for t, i in CASES]
TILE_H, TILE_W = 8, 16              # csrc/vpx_internal.h


def _fake(i):                        # distinct fake tensor addresses far away from the workspace
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


def _desc(c, prec, slope=0.0):
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    return ConvDesc(N, H, W, Ci, Co, kh, kw, s, p, tr, slope, PRECS.get(prec, prec), oph, opw)


# ---- the reference against closed forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
def test_one_hot_weight_is_a_strided_gather_or_scatter_with_zero_fill(s):
    """w = 1 at tap (ky, kx) of a 3 x 4 kernel, pad 1. Convolution: y[o, q] = x[s o - 1 + ky, s q - 1 + kx], zero outside the map.
    Transposed: x[i, j] lands at y[s i - 1 + ky, s j - 1 + kx], everything else is zero."""
    H, W, kh, kw, p = 4, 6, 3, 4, 1
    x = torch.arange(2 * H * W, dtype=torch.float32).reshape(2, 1, H, W) + 1.0
    for tr in (0, 1):
        c = (tr, 2, 1, 1, kh, kw, s, p, 0, 0, H, W)
        Ho, Wo = R.out_shape(c)
        for ky in range(kh):
            for kx in range(kw):
                w = torch.zeros(1, 1, kh, kw)
                w[0, 0, ky, kx] = 1.0
                y = R.reference(c, x, w, None, torch.ones(2, 1, Ho, Wo))["y"]
                want = torch.zeros(2, 1, Ho, Wo, dtype=torch.float64)
                if tr:
                    for i in range(H):
                        for j in range(W):
                            o, q = s * i - p + ky, s * j - p + kx
                            if 0 <= o < Ho and 0 <= q < Wo:
                                want[:, 0, o, q] = x[:, 0, i, j].double()
                else:
                    for o in range(Ho):
                        for q in range(Wo):
                            i, j = s * o - p + ky, s * q - p + kx
                            if 0 <= i < H and 0 <= j < W:
                                want[:, 0, o, q] = x[:, 0, i, j].double()
                assert torch.equal(y, want), (tr, ky, kx)


def test_output_padding_adds_rows_and_columns_that_hold_the_bias_only():
    """Transposed, stride 2, pad 0: the output-padding row / column lies past every tap; the rest equals the unpadded layer."""
    x, w, b = torch.randn(2, 3, 4, 5), torch.randn(3, 2, 3, 4), torch.tensor([0.25, -1.5])
    base = R.reference((1, 2, 3, 2, 3, 4, 2, 0, 0, 0, 4, 5), x, w, b, torch.ones(2, 2, 9, 12))["y"]
    for oph, opw in ((1, 0), (0, 1), (1, 1)):
        y = R.reference((1, 2, 3, 2, 3, 4, 2, 0, oph, opw, 4, 5), x, w, b, torch.ones(2, 2, 9 + oph, 12 + opw))["y"]
        assert y.shape == (2, 2, 9 + oph, 12 + opw) and torch.equal(y[:, :, :9, :12], base)
        for co in range(2):
            if oph:
                assert bool((y[:, co, 9] == float(b[co])).all())
            if opw:
                assert bool((y[:, co, :, 12] == float(b[co])).all())
    assert R.has_bias_only_outputs((1, 2, 3, 2, 3, 4, 2, 0, 1, 0, 4, 5)) and not R.has_bias_only_outputs((1, 2, 3, 2, 3, 4, 2, 1, 1, 1, 4, 5))


def test_bias_gradient_is_the_column_sum_of_the_masked_gy():
    for table, i, relu in (("PHASES", 6, False), ("STRIDED", 5, True), ("FLIP", 2, False), ("SMALL", 0, False)):
        v = R.variant(table, i)
        assert v["bias"] and (relu or v["slope"] != 0.0)
        t, ref, share = R.case(table, i, relu)
        d = torch.where(ref["pre"] > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.0 if relu else v["slope"], dtype=torch.float64))
        assert R.relmax(ref["db"], (t["gy"].double() * d).sum(dim=(0, 2, 3))) < 1e-14
        assert bool((t["gy"][~R.off_kink(ref["pre"], ref["y"])] == 0).all())


# ---- the routes of csrc/glue_fwd_api.hip (glue_route) and csrc/glue_bwd_api.hip (glue_bwd_plan), restated ---------------------------------------------------------------------------------------
def conv_small_kind(c):                                   # csrc/conv_small.hip
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    if s != 1 or kh != kw:
        return 0
    if not tr and kh == 3 and p == 1 and Ci in (1, 3) and Co % 8 == 0 and Co <= 64:
        return 1
    if not tr and kh == 1 and p == 0 and Ci % 4 == 0 and Ci <= 64 and Co in (1, 3):
        return 2
    if tr and kh == 1 and p == 0 and Ci in (1, 3) and Co % 8 == 0 and Co <= 64:
        return 3
    return 0


def wgrad_small_applicable(c):                            # csrc/lstm_bwd.hip (plain convolutions only: glue_wgrad_rule)
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    if tr or s != 1 or kh != kw:
        return None
    if kh == 3 and p == 1 and Ci == 1 and Co % 16 == 0 and Co <= 64:
        return "<16,1,3>"
    if kh == 3 and p == 1 and Ci == 3 and Co % 4 == 0 and Co <= 64:
        return "<4,3,3>"
    if kh == 1 and p == 0 and Ci == 16 and Co in (1, 3):
        return f"<{Co},16,1>"
    return None


def c16_applicable(c, prec, exp=0):                       # csrc/conv16.hip
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    return (not exp & Exp.NO_C16 and prec == "bf16x3" and (kh, kw, s, p) == (3, 3, 1, 1) and Co == 16 and Ci % 16 == 0 and 16 <= Ci <= 64)


def ex_wgrad_split(c, prec, exp=0):                       # csrc/glue_bwd_api.hip: glue_wgrad_rule (at the default MFMA shape)
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    return (not exp & Exp.GLUE_WGRAD_TAPGROUP and prec == "bf16x3" and Ci % 8 == 0 and Co % 8 == 0 and kh <= 2 * s + 1 and kw <= 2 * s + 1
            and kh * kw > 1 and wgrad_small_applicable(c) is None)


def exq_problem(c, prec):
    """exq_problem's (H, W, phases) of the tile space, or None where convq does not take the layer."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    if prec != "bf16x3" or Ci % 16 or Ci < 16 or Ci // 16 > 60 or kh * kw > 25:
        return None
    Ho, Wo = R.out_shape(c)
    if not tr:
        per = [0] * (s * s)
        for ky in range(kh):
            for kx in range(kw):
                sy, sx = (ky - p) % s, (kx - p) % s
                if abs((ky - p - sy) // s) > 1 or abs((kx - p - sx) // s) > 1:
                    return None
                per[sy * s + sx] += 1
        return None if 0 in per else (Ho, Wo, 0)
    for py in range(s):
        for px in range(s):
            n = 0
            for ky in range((py + p) % s, kh, s):
                for kx in range((px + p) % s, kw, s):
                    if abs((ky - py - p) // s) > 1 or abs((kx - px - p) // s) > 1:
                        return None
                    n += 1
            if n == 0:
                return None
    return ((Ho + s - 1) // s, (Wo + s - 1) // s, int(s == 2))


def exq_workgroups(c, prec):
    Hq, Wq, _ = exq_problem(c, prec)
    return c[1] * ((Wq + 15) // 16) * ((Hq + 15) // 16) * (((c[3] + 31) // 32 + 3) // 4)


def exq_preferred(c, prec):                               # the grid rule: >= 64 output channels; the phase form, or >= 256 workgroups
    q = exq_problem(c, prec)
    return q is not None and c[3] >= 64 and (q[2] == 1 or exq_workgroups(c, prec) >= 256)


def takes_split(c, prec, exp=0):                          # vpx_conv2d_ex_takes_split: 2 = convq / c16, 1 = first generation, 0 = no
    if exq_preferred(c, prec) or c16_applicable(c, prec, exp):
        return 2
    return 1 if prec != "f32" and c[2] % 8 == 0 else 0


def plain_tiles(Co):                                      # csrc/conv_gemm.hip: plain_groups' cost rule, ties to more groups
    best = min(range(4, 0, -1), key=lambda ng: (-(-Co // (32 * ng)) * (2 + ng), -ng))
    return -(-Co // (32 * best))


def pick_mw(N, Ht, Wt, Co, prec):                         # 8-wave workgroups: bf16 modes, >= 512 of them
    return 2 if prec != "f32" and N * (-(-Ht // (2 * TILE_H))) * (-(-Wt // TILE_W)) * plain_tiles(Co) >= 512 else 1


def gen1_launches(c):
    """(name, Ht, Wt, input step) of the first generation's launches."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    Ho, Wo = R.out_shape(c)
    if not tr:
        return [(f"conv.s{s}", Ho, Wo, s)]
    if s == 1:
        return [("flip", Ho, Wo, 1)]
    return [("phases", (Ho - py + 1) // 2, (Wo - px + 1) // 2, 1) for py in (0, 1) for px in (0, 1) if Ho - py >= 1 and Wo - px >= 1]


def adjoint(c):
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    Ho, Wo = R.out_shape(c)
    return (1 - tr, N, Co, Ci, kh, kw, s, p) + R.adjoint_out_pad(c) + (Ho, Wo)


def residues(c):
    """Taps (nty, ntx) of the weight gradient's launches, one per stride residue (strided_wgrad)."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    out = []
    for ry in range(s):
        for rx in range(s):
            ky0, kx0 = (p + ry) % s, (p + rx) % s
            nty = (kh - ky0 + s - 1) // s if ky0 < kh else 0
            ntx = (kw - kx0 + s - 1) // s if kx0 < kw else 0
            if nty >= 1 and ntx >= 1:
                out.append((nty, ntx))
    return out


def _gen1(c, prec, names, pre):
    for name, Ht, Wt, sd in gen1_launches(c):
        names.add(f"{pre}gen1.{name}")
        if sd == 1 and pick_mw(c[1], Ht, Wt, c[3], prec) == 2:
            names.add(f"{pre}gen1.{name}.8waves")
            if Ht % 16 and Ht % 16 <= 8:
                names.add(f"{pre}gen1.{name}.8waves.ragged")


def routes(c, prec, v, relu=False, exp=0, training=True, from_split=False):
    """What a training call of ops.conv2d_ex (relu: stphy_ops.conv2d_act; from_split: a forward handed split input) on case c launches."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    names = set()
    wsp = ex_wgrad_split(c, prec, exp)
    if from_split or (training and not relu and (oph, opw) == (0, 0) and wsp and takes_split(c, prec, exp)):
        if c16_applicable(c, prec, exp):
            names.add("fwd.split.c16")
        elif exq_preferred(c, prec):
            names.add("fwd.split.convq")
        else:
            _gen1(c, prec, names, "fwd.split.")
    elif not relu and conv_small_kind(c):
        k = conv_small_kind(c)
        names.add("fwd.small2" if k == 2 else f"fwd.small{k}." + ("to16" if Co == 16 else "many"))
    else:
        _gen1(c, prec, names, "fwd.")
    if not training:
        return names
    dq = not exp & Exp.GLUE_DGRAD_GEN1 and Co % 8 == 0 and exq_preferred(adjoint(c), prec)
    act = relu or v["slope"] != 0.0
    if act or v["bias"]:
        names.add("colsum." + ("v4" if Co % 4 == 0 else "scalar") + (".split_copy" if act and (dq or wsp) and Co % 4 == 0 else ""))
    a = adjoint(c)
    op = "" if a[8:10] == (0, 0) else f".op{a[8]}{a[9]}"
    if dq:
        names.add("dx.convq" + op)
    elif conv_small_kind(a):
        names.add(f"dx.small{conv_small_kind(a)}")
    else:
        _gen1(a, prec, names, "dx.")
        if op:
            names.add("dx.gen1" + op)
    small = wgrad_small_applicable(c)
    if small:
        names.add("dw.small" + small)
    else:
        for nty, ntx in residues(c):
            names.add("dw.wgrad2g" if wsp and nty * ntx >= 2 and nty <= 3 and ntx <= 3 else "dw.launch_wgrad")
    return names


REQUIRED = ["fwd.small1.to16", "fwd.small1.many", "fwd.small2", "fwd.small3.to16", "fwd.small3.many",
            "fwd.gen1.conv.s1", "fwd.gen1.conv.s2", "fwd.gen1.flip", "fwd.gen1.phases", "fwd.gen1.flip.8waves.ragged", "fwd.gen1.phases.8waves.ragged",
            "fwd.split.c16", "fwd.split.convq", "fwd.split.gen1.conv.s1", "fwd.split.gen1.conv.s2", "fwd.split.gen1.phases",
            "colsum.v4", "colsum.scalar", "colsum.v4.split_copy",
            "dx.gen1.conv.s2", "dx.gen1.phases", "dx.gen1.flip", "dx.gen1.conv.s1", "dx.small3", "dx.gen1.op10", "dx.gen1.op01", "dx.gen1.op11",
            "dx.convq", "dx.convq.op10", "dx.convq.op01", "dx.convq.op11",
            "dw.small<16,1,3>", "dw.small<4,3,3>", "dw.small<1,16,1>", "dw.small<3,16,1>", "dw.launch_wgrad", "dw.wgrad2g"]


def test_tables_are_what_the_kernels_need():
    L = _lib.lib()
    seen = {}
    for table, i in CASES:
        c, v = R.TABLES[table][i], R.variant(table, i)
        for prec in PRECS:
            # the restatements against the library's own answers
            d = _desc(c, prec, v["slope"])
            assert L.vpx_conv2d_ex_takes_split(ctypes.byref(d)) == takes_split(c, prec), (R.case_id(table, i), prec)
            assert L.vpx_conv2d_ex_bwd_uses_split(ctypes.byref(d)) == int(ex_wgrad_split(c, prec)), (R.case_id(table, i), prec)
            ho, wo = ctypes.c_int(0), ctypes.c_int(0)
            assert L.vpx_conv2d_ex_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == OK
            assert (ho.value, wo.value) == R.out_shape(c)
            if prec == "bf16x3" or table in R.BOTH_MODES:
                for training in ((True, False) if table == "WAVES8" else (table != "CONVQ_FWD",)):   # (WAVES8: an inference call as well)
                    for r in routes(c, prec, v, training=training, from_split=table == "CONVQ_FWD"):
                        seen.setdefault(r, []).append(R.case_id(table, i))
        for bit, restated in ((Exp.NO_C16, takes_split(c, "bf16x3", Exp.NO_C16)), (Exp.GLUE_WGRAD_TAPGROUP, None)):
            d = _desc(c, "bf16x3", v["slope"])
            with _lib.experiment(bit):
                if restated is not None:
                    assert L.vpx_conv2d_ex_takes_split(ctypes.byref(d)) == restated, R.case_id(table, i)
                else:
                    assert L.vpx_conv2d_ex_bwd_uses_split(ctypes.byref(d)) == 0, R.case_id(table, i)
        N, Co = c[1], c[3]
        assert N * Co * R.out_shape(c)[0] * R.out_shape(c)[1] <= 5e5 or (table, i) == ("WAVES8", 1), R.case_id(table, i)
    for table, i in R.ACT:
        for r in routes(R.TABLES[table][i], "bf16x3", R.variant(table, i), relu=True):
            seen.setdefault("act." + r, []).append(R.case_id(table, i))
    for r in REQUIRED:
        assert r in seen, f"no case reaches {r}: {sorted(seen)}"
    print({r: len(s) for r, s in sorted(seen.items())})

    # PHASES: square and rectangular kernels, 1 ... 16 taps per phase, every output padding, the small maps
    ks = {(c[4], c[5]) for c in R.PHASES}
    assert ks >= {(k, k) for k in range(2, 8)} | {(3, 4), (4, 3), (2, 5), (7, 2)}
    for k in range(2, 8):
        assert {c[7] for c in R.PHASES if (c[4], c[5]) == (k, k) and (c[10], c[11]) == (7, 9)} == {0, 1, k // 2}
    assert {(c[8], c[9]) for c in R.PHASES} == set(R._OPS) and {(c[10], c[11]) for c in R.PHASES} == {(1, 1), (1, 5), (5, 1), (7, 9)}
    assert all(c[0] == 1 and c[6] == 2 and (c[2], c[3]) == (5, 6) for c in R.PHASES)
    assert {n for c in R.PHASES for n in residues(c)} >= {(1, 1), (2, 2), (3, 3), (3, 4), (4, 3), (4, 4), (1, 3), (4, 1)}
    assert any(len(gen1_launches(c)) < 4 for c in R.PHASES)                                   # an empty phase
    assert any(len({(h, w) for _, h, w, _ in gen1_launches(c)}) == 4 for c in R.PHASES)       # four unequal phases
    # STRIDED: every kernel with p = 0 ... 3 and all four output paddings of the adjoint
    for k in ((2, 2), (3, 3), (4, 4), (5, 5), (7, 7), (3, 5), (4, 2)):
        sel = [c for c in R.STRIDED if (c[4], c[5]) == k and c[10] > 1]
        assert {c[7] for c in sel} == {0, 1, 2, 3} and {R.adjoint_out_pad(c) for c in sel} == set(R._OPS), k
    assert any(c[10] == 1 and c[4] == 3 and c[7] == 1 for c in R.STRIDED)
    assert all((c[0], c[6], c[2], c[3]) == (0, 2, 12, 20) for c in R.STRIDED)
    # FLIP
    assert {(c[4], c[5]) for c in R.FLIP} == {(1, 1), (3, 3), (5, 5), (7, 7), (3, 5), (1, 7)} and {(c[10], c[11]) for c in R.FLIP} == {(4, 6), (9, 17)}
    for k in (3, 5, 7):
        assert {c[7] for c in R.FLIP if (c[4], c[5]) == (k, k)} == {0, k // 2, k - 1}
    assert all((c[0], c[6], c[2], c[3]) == (1, 1, 17, 9) for c in R.FLIP)
    # SMALL: the gates, and the neighbours just outside them
    assert all(conv_small_kind(c) == 1 for c in R.SMALL_KIND1) and {(c[2], c[3]) for c in R.SMALL_KIND1} == {(a, b) for a in (1, 3) for b in (8, 16, 24, 64)}
    assert all(conv_small_kind(c) == 2 for c in R.SMALL_KIND2) and {(c[2], c[3]) for c in R.SMALL_KIND2} == {(a, b) for a in (4, 16, 60, 64) for b in (1, 3)}
    assert all(conv_small_kind(c) == 3 for c in R.SMALL_KIND3) and {(c[2], c[3]) for c in R.SMALL_KIND3} == {(a, b) for a in (1, 3) for b in (8, 16, 64)}
    assert all(conv_small_kind(c) == 0 for c in R.SMALL_OUTSIDE) and {(c[2], c[3]) for c in R.SMALL_OUTSIDE} >= {(2, 16), (1, 12), (3, 72), (68, 3)}
    assert conv_small_kind(R.SMALL_WGRAD[0]) == 1 and conv_small_kind(R.SMALL_WGRAD[1]) == 0
    got = {(c[2], c[3]): wgrad_small_applicable(c) for c in R.SMALL if wgrad_small_applicable(c)}
    assert set(got) >= {(1, 16), (1, 32), (1, 64), (3, 4), (3, 8), (3, 64), (16, 1), (16, 3)}
    assert all(wgrad_small_applicable(c) is None for c in R.SMALL_OUTSIDE + R.SMALL_KIND3)
    assert all(c[1] * c[10] * c[11] == 306 for c in R.SMALL)
    for kind, rows in ((1, R.SMALL_KIND1), (2, R.SMALL_KIND2), (3, R.SMALL_KIND3)):   # with a slope, without one, without a bias
        vs = [R.variant("SMALL", R.SMALL.index(c)) for c in rows]
        assert {a["slope"] != 0.0 for a in vs} == {True, False} and {a["bias"] for a in vs} == {True, False}, kind
    # SPLIT: every channel pair on every layer; k7 s2 falls back
    for c in R.SPLIT:
        assert takes_split(c, "bf16x3") == 1 and ex_wgrad_split(c, "bf16x3") == (c[4] != 7), c
    assert {(c[2], c[3]) for c in R.SPLIT} == set(R._SPLIT_CH) and {(c[10], c[11]) for c in R.SPLIT} == {(19, 21), (9, 7)}
    assert {(c[0], c[4], c[6], c[7]) for c in R.SPLIT} == set(R._SPLIT_LAYERS) and len(R.SPLIT) == 24
    assert all(c16_applicable(c, "bf16x3") and not c16_applicable(c, "bf16x3", Exp.NO_C16) for c in R.C16)
    assert {(c[0], c[2]) for c in R.C16} == {(tr, ci) for tr in (0, 1) for ci in (16, 32, 48, 64)}
    # CONVQ: the smallest plain-conv grid exq_preferred takes — 256 workgroups, one frame fewer is refused
    c = R.CONVQ_FWD[0]
    assert exq_workgroups(c, "bf16x3") == 256 and not exq_preferred((c[0], 255) + c[2:], "bf16x3")
    assert all(takes_split(c, "bf16x3") == 2 and exq_preferred(c, "bf16x3") for c in R.CONVQ_FWD)
    assert [(c[8], c[9]) for c in R.CONVQ_FWD] == [(0, 0), (0, 0), (1, 1), (1, 0), (0, 1)]
    assert [R.adjoint_out_pad(c) for c in R.CONVQ_BWD] == [(0, 1), (1, 0), (0, 0), (1, 1), (1, 0)]
    assert all(exq_preferred(adjoint(c), "bf16x3") and not exq_preferred(adjoint(c), "f32") for c in R.CONVQ_BWD)
    # WAVES8: every launch (for stride 2, every phase) gets the 8-wave form on a ragged second half tile
    for c in R.WAVES8:
        for name, Ht, Wt, sd in gen1_launches(c):
            wgs = c[1] * (-(-Ht // 16)) * (-(-Wt // 16)) * plain_tiles(c[3])
            assert sd == 1 and wgs >= 512 and pick_mw(c[1], Ht, Wt, c[3], "bf16x3") == 2 and pick_mw(c[1], Ht, Wt, c[3], "f32") == 1, (c, name, wgs)
            assert Ht % 16 == 1 and Wt % 16 == 1
    assert pick_mw(22, 17, 33, 8, "bf16x3") == 1            # (the issue's N = 22 misses the rule: 132 workgroups per phase)
    # ACT: one case per table, ReLU through conv2d_act (no output padding there), both colsum forms, the streaming kernels bypassed
    assert [t for t, _ in R.ACT] == ["PHASES", "STRIDED", "FLIP", "SMALL"]
    assert all(R.TABLES[t][i][8:10] == (0, 0) for t, i in R.ACT) and {R.TABLES[t][i][3] % 4 == 0 for t, i in R.ACT} == {True, False}
    t, i = R.ACT[3]
    assert conv_small_kind(R.TABLES[t][i]) == 1 and "act.fwd.gen1.conv.s1" in seen and not any(r.startswith("act.fwd.small") for r in seen)
    for table in R.TABLES:
        vt = [R.variant(table, i) for i in range(len(R.TABLES[table]))]
        assert {a["channels_last"] for a in vt} == {True, False} and (len(vt) < 3 or {a["bias"] for a in vt} == {True, False})
    for table, i in R.ACT + R.DETERMINISTIC:
        assert i < len(R.TABLES[table])


# ---- the reference alone stays inside the bars ---------------------------------------------------------------------------------------
RELU_CASES = [(t, i, True) for t, i in R.ACT]


def _fp32_run(c, t, slope, relu, chunk=4):
    """The reference in fp32, at most 4 images at a time, the chunks' dw and db added in fp32. How long a sum over the batch torch's CPU
    kernels run in one piece depends on the machine's thread count, which is no property of the case: WAVES8's N = 86 in one piece gives
    dw 1.4e-6 on 8 threads and 7.4e-6 on one, db 4.5e-6 on both; 4 images at a time 4.5e-7 / 1.0e-6 and 4.2e-7."""
    out = None
    for n0 in range(0, c[1], chunk):
        r = R.reference((c[0], min(chunk, c[1] - n0)) + c[2:], t["x"][n0:n0 + chunk], t["w"], t["b"], t["gy"][n0:n0 + chunk], slope, relu, dtype=torch.float32)
        if out is None:
            out = {k: [a] for k, a in r.items()}
        else:
            for k, a in r.items():
                out[k].append(a)
    return {"y": torch.cat(out["y"]), "dx": torch.cat(out["dx"]), "dw": sum(out["dw"][1:], out["dw"][0]),
            "db": None if t["b"] is None else sum(out["db"][1:], out["db"][0])}


@pytest.mark.parametrize("table,i,relu", [(t, i, False) for t, i in CASES] + RELU_CASES, ids=IDS + [R.case_id(t, i) + "-relu" for t, i, _ in RELU_CASES])
def test_fp32_reference_holds_a_fifth_of_the_f32_bars_and_next_to_nothing_sits_on_the_kink(table, i, relu):
    c, v = R.TABLES[table][i], R.variant(table, i)
    t, ref, share = R.case(table, i, relu)
    r32 = _fp32_run(c, t, 0.0 if relu else v["slope"], relu)
    fwd, grad = R.BARS["f32"]
    errs = {k: R.relmax(r32[k], ref[k]) for k in ("y", "dx", "dw", "db") if ref[k] is not None}
    print(R.case_id(table, i), {k: f"{e:.2e}" for k, e in errs.items()}, f"zeroed {share:.2e} of {ref['y'].numel()}")
    assert share <= R.KINK_SHARE, share
    assert errs["y"] < R.HOST_SHARE * fwd, errs
    for k in ("dx", "dw", "db"):
        assert k not in errs or errs[k] < R.HOST_SHARE * grad, errs


# ---- dry run -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    lib = _lib.lib()
    with _lib.option(_lib.OPT_DRY_RUN, 1):
        yield lib
    lib.vpx_set_deterministic(0)


def _must(L, rc, what, want=OK):
    assert rc == want, f"{what}: rc={rc}, expected {want}: {L.vpx_last_error().decode()}"


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", list(PRECS))
def test_every_case_carves_exactly_the_queried_workspace(L, prec, det):
    """No case of any table is refused by any entry point: rc == 0 throughout, at an aligned and an unaligned workspace base."""
    L.vpx_set_deterministic(det)
    for table, i in CASES:
        c, v = R.TABLES[table][i], R.variant(table, i)
        d, plain = _desc(c, prec, v["slope"]), _desc(c, prec)
        dp, pp = ctypes.byref(d), ctypes.byref(plain)
        tag = f"{R.case_id(table, i)} {prec} det={det}"
        nb, nbw = L.vpx_conv2d_ex_workspace_bytes(dp), L.vpx_conv2d_ex_bwd_workspace_bytes(dp)
        nba, nbwa = L.vpx_conv2d_act_workspace_bytes(pp, _lib.ACT_RELU), L.vpx_conv2d_act_bwd_workspace_bytes(pp, _lib.ACT_RELU)
        nbs = L.vpx_conv2d_ex_split_workspace_bytes(dp)
        assert nb > 0 and nbw > 0 and nba > 0 and nbwa > 0 and (nbs > 0) == (takes_split(c, prec) != 0), tag
        for base in (WS_BASE, WS_BASE_ODD):
            ws = ctypes.c_void_p(base)
            _must(L, L.vpx_conv2d_ex_fwd(dp, _fake(1), _fake(2), _fake(3), _fake(4), ws, nb, None), tag + " fwd")
            if c[3] % 8 == 0:
                _must(L, L.vpx_conv2d_ex_fwd_split(dp, _fake(1), _fake(2), _fake(3), None, _fake(9), ws, nb, None), tag + " fwd_split")
            if nbs:
                for packed in (0, 1):
                    _must(L, L.vpx_conv2d_ex_fwd_from_split(dp, _fake(8), 0, 0, 1, _fake(2), _fake(3), _fake(4), _fake(9) if c[3] % 8 == 0 else None,
                                                            packed, ws, nbs, None), tag + f" fwd_from_split packed={packed}")
            _must(L, L.vpx_conv2d_ex_bwd(dp, _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(10), ws, nbw, None), tag + " bwd")
            _must(L, L.vpx_conv2d_ex_bwd_ex(dp, _fake(1), _fake(8) if ex_wgrad_split(c, prec) else None, _fake(2), _fake(4), _fake(5), _fake(6),
                                            _fake(7), None, ws, nbw, None), tag + " bwd_ex")
            _must(L, L.vpx_conv2d_act_fwd(pp, _lib.ACT_RELU, _fake(1), _fake(2), _fake(3), _fake(4), ws, nba, None), tag + " act_fwd")
            _must(L, L.vpx_conv2d_act_bwd(pp, _lib.ACT_RELU, _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(10), ws, nbwa, None),
                  tag + " act_bwd")
        _must(L, L.vpx_conv2d_ex_fwd(dp, _fake(1), _fake(2), _fake(3), _fake(4), ctypes.c_void_p(WS_BASE), nb - 1, None), tag + " fwd, short", E_WS)
        _must(L, L.vpx_conv2d_ex_bwd(dp, _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(10), ctypes.c_void_p(WS_BASE), nbw - 1, None),
              tag + " bwd, short", E_WS)


def test_refusals(L):
    """Each documented refusal (include/vpx.h) returns its code and leaves a message; the size queries answer 0."""
    L.vpx_set_deterministic(0)
    ws = ctypes.c_void_p(WS_BASE)

    def fwd(d, want, words):
        assert L.vpx_conv2d_ex_workspace_bytes(ctypes.byref(d)) == 0
        rc = L.vpx_conv2d_ex_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), ws, 1 << 30, None)
        assert rc == want and words in L.vpx_last_error(), (rc, L.vpx_last_error())
        assert L.vpx_conv2d_ex_bwd_workspace_bytes(ctypes.byref(d)) == 0
        rc = L.vpx_conv2d_ex_bwd(ctypes.byref(d), _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(10), ws, 1 << 30, None)
        assert rc == want and words in L.vpx_last_error(), (rc, L.vpx_last_error())

    fwd(ConvDesc(2, 9, 17, 8, 8, 3, 3, 3, 1, 0, 0.0, 0, 0, 0), E_UNSUPPORTED, b"stride 3")
    fwd(ConvDesc(2, 9, 17, 8, 8, 8, 8, 1, 1, 0, 0.0, 0, 0, 0), E_UNSUPPORTED, b"larger than 7")
    fwd(ConvDesc(2, 9, 17, 8, 8, 3, 8, 2, 1, 1, 0.0, 0, 0, 0), E_UNSUPPORTED, b"larger than 7")
    for s, oph, opw in ((2, 2, 0), (2, 0, 2), (1, 1, 0), (1, 0, 1), (2, -1, 0)):          # output padding >= stride
        fwd(ConvDesc(2, 9, 17, 8, 8, 4, 4, s, 1, 1, 0.0, 0, oph, opw), E_ARG, b"output padding")
    fwd(ConvDesc(2, 9, 17, 8, 8, 3, 3, 1, 3, 1, 0.0, 0, 0, 0), E_UNSUPPORTED, b"padding larger than kernel-1")
    fwd(ConvDesc(2, 9, 17, 8, 8, 3, 5, 1, 3, 1, 0.0, 0, 0, 0), E_UNSUPPORTED, b"padding larger than kernel-1")
    fwd(ConvDesc(2, 9, 17, 8, 8, 3, 3, 1, 1, 0, 0.0, 3, 0, 0), E_UNSUPPORTED, b"precision")
    # ReLU beside a LeakyReLU slope in the descriptor
    leaky = ConvDesc(2, 9, 17, 8, 8, 3, 3, 2, 1, 0, 0.2, 0, 0, 0)
    assert L.vpx_conv2d_act_workspace_bytes(ctypes.byref(leaky), _lib.ACT_RELU) == 0 and L.vpx_conv2d_act_bwd_workspace_bytes(ctypes.byref(leaky), _lib.ACT_RELU) == 0
    assert L.vpx_conv2d_act_fwd(ctypes.byref(leaky), _lib.ACT_RELU, _fake(1), _fake(2), _fake(3), _fake(4), ws, 1 << 30, None) == E_ARG
    assert L.vpx_conv2d_act_bwd(ctypes.byref(leaky), _lib.ACT_RELU, _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(10), ws, 1 << 30, None) == E_ARG
    assert b"VPX_ACT_RELU" in L.vpx_last_error()
    # a backward with a kernel smaller than the stride (the forward runs)
    for tr in (0, 1):
        for kh, kw in ((1, 1), (1, 3), (3, 1)):
            d = ConvDesc(2, 9, 17, 8, 8, kh, kw, 2, 0, tr, 0.0, 0, 0, 0)
            if not tr:
                _must(L, L.vpx_conv2d_ex_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), ws, L.vpx_conv2d_ex_workspace_bytes(ctypes.byref(d)), None), "k < s fwd")
            rc = L.vpx_conv2d_ex_bwd(ctypes.byref(d), _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(10), ws, 1 << 30, None)
            assert rc == E_UNSUPPORTED and L.vpx_last_error(), (tr, kh, kw, rc, L.vpx_last_error())
    # a split output needs whole groups of 8 channels
    d = ConvDesc(2, 9, 17, 8, 12, 3, 3, 1, 1, 0, 0.0, 1, 0, 0)
    nb = L.vpx_conv2d_ex_workspace_bytes(ctypes.byref(d))
    assert L.vpx_conv2d_ex_fwd_split(ctypes.byref(d), _fake(1), _fake(2), _fake(3), None, _fake(9), ws, nb, None) == E_UNSUPPORTED
    assert b"multiple of 8" in L.vpx_last_error()
    nbs = L.vpx_conv2d_ex_split_workspace_bytes(ctypes.byref(d))
    assert L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), _fake(8), 0, 0, 1, _fake(2), _fake(3), None, _fake(9), 0, ws, nbs, None) == E_UNSUPPORTED
    _must(L, L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), _fake(8), 0, 0, 1, _fake(2), _fake(3), _fake(4), None, 0, ws, nbs, None), "fp32 output, Co = 12")
    # a layer with no route on split input (f32 operands), NULL tensors
    d = ConvDesc(2, 9, 17, 8, 8, 3, 3, 1, 1, 0, 0.0, 0, 0, 0)
    assert L.vpx_conv2d_ex_split_workspace_bytes(ctypes.byref(d)) == 0
    assert L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), _fake(8), 0, 0, 1, _fake(2), _fake(3), _fake(4), None, 0, ws, 1 << 30, None) == E_UNSUPPORTED
    nb = L.vpx_conv2d_ex_workspace_bytes(ctypes.byref(d))
    assert L.vpx_conv2d_ex_fwd(ctypes.byref(d), None, _fake(2), _fake(3), _fake(4), ws, nb, None) == E_ARG
    assert L.vpx_conv2d_ex_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), None, nb, None) == E_WS
    _must(L, L.vpx_conv2d_ex_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), ws, nb, None), "the next valid call")
