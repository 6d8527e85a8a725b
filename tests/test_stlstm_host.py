"""The plain ST-LSTM step on the CPU: every case of tests/stlstm_ref.py is on the plan the table states (vpx_stlstm_plan: filled by the
functions that decide the real calls), the union of the plans covers every route value the table is there for, each case's forward and
backward accept exactly the queried workspace and reserve in a dry run (VPX_OPT_DRY_RUN, as tests/test_workspace_contract.py) and refuse
one byte less, the inputs are well enough conditioned to judge a kernel by (the reference's own fp32 run against fp64), and the query
refuses what the size query refuses."""
import ctypes

import pytest
import torch

import stlstm_ref as R
from vp_suite_amd import _lib
from vp_suite_amd._lib import STLSTMDesc, STLSTMPlanInfo

OK, E_ARG, E_WS, E_UNSUPPORTED = 0, -1, -2, -4
WS_BASE = 0x7F0000000000            # fake workspace address (256-byte aligned; never dereferenced in a dry run)
PRECS = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}
ARRAYS = ("c5_ks", "dg_ksplit", "dg_mw")


def _fake(i):                        # distinct fake tensor addresses far away from the workspace
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


def _desc(case, save=None):
    C = R.CASES[case]
    Cin, Ch, H, W, k, ln, B = C.shape
    save = bool(C.grads) if save is None else save
    return STLSTMDesc(B, Cin, Ch, H, W, k, ln, _lib.LAYOUT_NHWC, PRECS[C.prec], _lib.FLAG_SAVE_FOR_BWD if save else 0)


def plan_of(L, case, det=None):
    """(plan as a dict, vpx_stlstm_uses_split, vpx_stlstm_defers_wgrad) under the case's experiment bits and deterministic setting."""
    C = R.CASES[case]
    prev = L.vpx_set_deterministic(C.det if det is None else det)
    try:
        with _lib.experiment(_lib.exp_bits(C.exp)):
            d, info = _desc(case), STLSTMPlanInfo()
            rc = L.vpx_stlstm_plan(ctypes.byref(d), R.all_weight_grads(case), ctypes.byref(info))
            assert rc == OK, (case, rc, L.vpx_last_error())
            uses, defers = L.vpx_stlstm_uses_split(ctypes.byref(d)), L.vpx_stlstm_defers_wgrad(ctypes.byref(d))
    finally:
        L.vpx_set_deterministic(prev)
    return {n: (tuple(getattr(info, n)) if n in ARRAYS else getattr(info, n)) for n, _ in STLSTMPlanInfo._fields_}, uses, defers


@pytest.mark.parametrize("case", list(R.CASES))
def test_case_is_on_the_plan_the_table_states(case):
    L = _lib.lib()
    C = R.CASES[case]
    plan, uses, defers = plan_of(L, case)
    stated = {k: (tuple(v) if k in ARRAYS else v) for k, v in C.plan.items()}
    assert {k: plan[k] for k in stated} == stated, (case, plan)
    assert uses == int(plan["route"] in (R.C5, R.C5K)), (case, plan)
    # stw runs only when all five weight gradients are wanted; asked for all of them, it runs exactly where the gradients can be deferred
    if R.all_weight_grads(case):
        assert defers == plan["stw"], (case, plan)
    else:
        assert plan["stw"] == 0 and plan["c5"] == 0, (case, plan)
    assert plan["c5"] <= plan["stw"] and (plan["c5_ks"] == (0,) * 5) == (plan["c5"] == 0), (case, plan)


def test_table_covers_every_route_value():
    L = _lib.lib()
    plans = {case: plan_of(L, case)[0] for case in R.CASES}
    got = R.reached(plans)
    print({k: sorted(v) for k, v in got.items()})
    assert got == R.REQUIRED
    C = R.CASES
    # the table's other axes
    assert {C[c].prec for c in C} == {"f32", "bf16x3", "bf16"} and all((C[c].prec == "bf16") == (C[c].grads == ()) for c in C)
    assert {(C[c].prec, C[c].shape[4]) for c in C if plans[c]["route"] == R.GEN1} >= {("f32", 5), ("bf16x3", 3), ("bf16x3", 7), ("bf16x3", 5)}
    assert {C[c].shape[0] for c in C if plans[c]["route"] == R.GEN1} >= {1, 3} and any(C[c].shape[1] == 5 for c in C)
    assert any(C[c].shape[2:4] == (1, 1) for c in C)
    assert {(C[c].shape[4], C[c].shape[6] % 2) for c in C if plans[c]["route"] == R.LN} == {(5, 1), (3, 1)}
    ragged = lambda s: s[2] > 1 and s[3] > 1 and (s[2] % 8 or s[2] % 16) and s[3] % 16
    assert {plans[c]["route"] for c in C if ragged(C[c].shape)} == {R.LN, R.GEN1, R.C5, R.C5K}
    assert any(C[c].shape[1] == 96 and plans[c]["nt_o"] == 4 for c in C)                       # conv_o: a 64-wide tile and a half-empty one
    # fused conv_o by grid size and by deterministic mode
    assert {C[c].det for c in C if plans[c]["route"] == R.GEN1 and plans[c]["o_split"] == 0} == {0, 1}
    assert {plans[c]["route"] for c in C if C[c].det} == {R.GEN1, R.C5, R.C5K}
    # frozen weights behind a c5 forward; subsets of the data gradients; missing incoming gradients; chained steps; layouts
    frozen = [c for c in C if C[c].grads and not R.all_weight_grads(c)]
    assert {plans[c]["route"] for c in frozen} == {R.C5, R.C5K}
    assert {tuple(w for w in R.WEIGHTS if w in C[c].grads) for c in frozen} == {R.WEIGHTS[:4], ("Wx",)}
    assert {tuple(s for s in R.STATES if s in C[c].grads) for c in C if C[c].grads} == {R.STATES, ("x",), ("h", "c", "m")}
    assert {C[c].loss for c in C} == set(R.LOSSES) and {C[c].layout for c in C} == {"nchw", "channels_last", "sliced"}
    assert {plans[c]["route"] for c in C if C[c].loss == "two_step"} == {R.C5, R.C5K}
    assert all(C[c].shape[0] == C[c].shape[1] for c in C if C[c].loss == "two_step")
    # the mixed path: a first-generation forward in front of stw + K-split c5
    assert plans["gen1_ch24_mixed"]["route"] == R.GEN1 and plans["gen1_ch24_mixed"]["c5"] == 1 and max(plans["gen1_ch24_mixed"]["c5_ks"]) > 1


# ---- dry run ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    lib = _lib.lib()
    with _lib.option(_lib.OPT_DRY_RUN, 1):
        yield lib
    lib.vpx_set_deterministic(0)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("case", list(R.CASES))
def test_case_carves_exactly_the_queried_workspace_and_reserve(L, case, det):
    C = R.CASES[case]
    ln = C.shape[5]
    lnarr = (ctypes.c_void_p * 8)(*[0x200000000000 + i * (1 << 30) for i in range(8)]) if ln else None
    dlnarr = (ctypes.c_void_p * 8)(*[0x300000000000 + i * (1 << 30) for i in range(8)]) if ln else None
    want = lambda n, i: _fake(i) if n in C.grads else None
    L.vpx_set_deterministic(det)
    try:
        with _lib.experiment(_lib.exp_bits(C.exp)):
            d = _desc(case)
            save = bool(C.grads)
            nb, rs = L.vpx_stlstm_workspace_bytes(ctypes.byref(d)), L.vpx_stlstm_reserve_bytes(ctypes.byref(d))
            assert nb > 256 and (rs > 0) == save, (case, nb, rs)

            def fwd(rs_, nb_):
                return L.vpx_stlstm_step_fwd_ex(ctypes.byref(d), *[_fake(i) for i in range(1, 10)], lnarr, *[_fake(i) for i in range(10, 15)],
                                                _fake(15), rs_, ctypes.c_void_p(WS_BASE), nb_, None, None)

            def bwd(rs_, nb_):
                gin = [_fake(16 + i) if o in R.LOSSES[C.loss] or C.loss == "two_step" else None for i, o in enumerate(R.OUTS)]
                return L.vpx_stlstm_step_bwd_ex(ctypes.byref(d), *[_fake(i) for i in range(1, 12)], lnarr, _fake(15), rs_, *gin,
                                                *[want(n, 21 + i) for i, n in enumerate(R.STATES)], *[want(n, 25 + i) for i, n in enumerate(R.WEIGHTS)],
                                                dlnarr, ctypes.c_void_p(WS_BASE), nb_, None, None)
            for call in ((fwd, bwd) if save else (fwd,)):
                tag = f"{case} det={det} {call.__name__}"
                assert call(rs, nb) == OK, (tag, L.vpx_last_error())
                assert call(rs, nb - 1) == E_WS, (tag, "workspace one byte short")
                if save:
                    assert call(rs - 1, nb) == E_WS, (tag, "reserve one byte short")
    finally:
        L.vpx_set_deterministic(0)


# ---- the inputs' condition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_fp32_reference_holds_half_the_f32_bars(case):
    """The COND of tests/test_gpu_acstlstm.py: the reference's own fp32 CPU run against its fp64 run, outputs 5e-6, gradients 2.5e-5."""
    ref, r32 = R.cpu(case), R.cpu(case, torch.float32)
    assert set(ref) == set(r32)
    errs = {k: R.relmax(r32[k], ref[k]) for k in ref}
    worst = lambda pre: max((v for k, v in errs.items() if k.startswith("grad.") == pre), default=0.0)
    print(f"{case}: worst output {worst(False):.2e}, worst gradient {worst(True):.2e}")
    assert worst(False) <= R.COND[0] and worst(True) <= R.COND[1], {k: f"{v:.2e}" for k, v in errs.items()}
    C = R.CASES[case]
    if C.loss == "c_dm":   # conv_o and conv_last lie behind h_new alone: the loss does not reach them
        assert not ref["grad.Wo"].any() and not ref["grad.Wlast"].any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_plan_query_refuses_what_the_size_query_refuses():
    L = _lib.lib()
    info = STLSTMPlanInfo()
    good = dict(B=2, Cin=8, Ch=16, H=9, W=17, k=3, layer_norm=0, layout=0, precision=1, flags=1)

    def rc_of(**kw):
        d = STLSTMDesc(**{**good, **kw})
        rc = L.vpx_stlstm_plan(ctypes.byref(d), 1, ctypes.byref(info))
        assert (L.vpx_stlstm_workspace_bytes(ctypes.byref(d)) == 0) == (rc != OK), kw
        return rc
    assert rc_of() == OK
    for k in (2, 4, 0, 9, -1):                                # even, or larger than 7
        assert rc_of(k=k) == E_ARG and b"odd" in L.vpx_last_error(), k
    for dim in ("B", "Cin", "Ch", "H", "W"):
        for v in (0, -3):
            assert rc_of(**{dim: v}) == E_ARG and b"non-positive" in L.vpx_last_error(), (dim, v)
    for prec in (-1, 3):
        assert rc_of(precision=prec) == E_UNSUPPORTED and b"precision" in L.vpx_last_error(), prec
    assert rc_of(layout=2) == E_ARG
    d = STLSTMDesc(**good)
    assert L.vpx_stlstm_plan(ctypes.byref(d), 1, None) == E_ARG and L.vpx_stlstm_plan(None, 1, ctypes.byref(info)) == E_ARG
    assert rc_of() == OK                                      # (the next valid query)
