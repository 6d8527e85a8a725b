"""The ConvLSTM sequence on the CPU: every case of tests/convlstm_ref.py is on the plan the table states (vpx_convlstm_plan: filled by the
functions that decide the real calls), the union of the plans covers every route and form the table is there for, each case's forward and
backward accept the queried workspace and reserve in a dry run (VPX_OPT_DRY_RUN, as tests/test_workspace_contract.py) and refuse less,
the inputs are well enough conditioned to judge a kernel by (the reference's own fp32 run against fp64), and the query refuses what the
size query refuses. Every case runs under its own options, which are put back after it."""
import contextlib
import ctypes

import pytest
import torch

import convlstm_ref as R
from vp_suite_amd import _lib
from vp_suite_amd._lib import ConvLSTMDesc, ConvLSTMPlanInfo

OK, E_ARG, E_WS, E_UNSUPPORTED = 0, -1, -2, -4
WS_BASE = 0x7F0000000000            # fake workspace address (256-byte aligned; never dereferenced in a dry run)
PRECS = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}
DEFAULTS = {"OPT_CELL2": 1, "OPT_CELL3": 1, "OPT_MFMA_SHAPE": 1, "OPT_EXPERIMENT": 0}


def _fake(i):                        # distinct fake tensor addresses far away from the workspace
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


def _desc(case):
    C = R.CASES[case]
    Cin, Ch, H, W, k, B, T = C.shape
    return ConvLSTMDesc(B, T, Cin, Ch, H, W, k, k, C.order, _lib.LAYOUT_NHWC, PRECS[C.prec], _lib.FLAG_SAVE_FOR_BWD if C.grads else 0)


@contextlib.contextmanager
def settings(L, case):
    """The case's options, experiment bits and deterministic setting for a block; what was set before comes back on the way out."""
    C = R.CASES[case]
    prev = L.vpx_set_deterministic(C.det)
    try:
        with contextlib.ExitStack() as stack:
            for name, value in C.opts.items():
                stack.enter_context(_lib.option(getattr(_lib, name), value))
            stack.enter_context(_lib.experiment(_lib.exp_bits(C.exp)))
            yield
    finally:
        L.vpx_set_deterministic(prev)


def plan_of(L, case):
    """The library's plan of the case as a dict, under the case's settings."""
    C = R.CASES[case]
    with settings(L, case):
        d, info = _desc(case), ConvLSTMPlanInfo()
        rc = L.vpx_convlstm_plan(ctypes.byref(d), int("x" in C.ops), int("x" in C.grads), int("W" in C.grads), ctypes.byref(info))
        assert rc == OK, (case, rc, L.vpx_last_error())
    return {n: getattr(info, n) for n, _ in ConvLSTMPlanInfo._fields_}


def _options_now(L):
    """(option values, deterministic setting), read by setting each to its default and putting the answer back."""
    now = {}
    for name, default in DEFAULTS.items():
        now[name] = L.vpx_set_option(getattr(_lib, name), default)
        L.vpx_set_option(getattr(_lib, name), now[name])
    det = L.vpx_set_deterministic(0)
    L.vpx_set_deterministic(det)
    return now, det


@pytest.mark.parametrize("case", list(R.CASES))
def test_case_is_on_the_plan_the_table_states(case):
    L = _lib.lib()
    C = R.CASES[case]
    before = _options_now(L)
    plan = plan_of(L, case)
    assert _options_now(L) == before == (DEFAULTS, 0), (case, before)
    assert {k: plan[k] for k in C.plan} == C.plan, (case, plan)
    bwd = ("dgrad", "dgrad_qform", "d_mw", "dgrad_cols", "wgrad", "n_slices", "dG_f32", "gate_slices")
    if not C.grads:
        assert not any(plan[k] for k in bwd), (case, plan)
        return
    Cin, Ch = C.shape[:2]
    assert plan["dgrad_cols"] == (Cin + Ch if "x" in C.grads else Ch), (case, plan)
    assert (plan["wgrad"] == 0 and plan["n_slices"] == 0) if "W" not in C.grads else plan["n_slices"] >= 1, (case, plan)
    assert plan["dgrad"] == int(plan["route"] in (R.CELL2, R.C3)) and (plan["d_mw"] >= 1) == (plan["dgrad"] == 0), (case, plan)
    # fp32 dG has a reader unless conv2 takes the data gradient and the weight gradient is wgrad2 on the reserve (or not wanted)
    assert plan["dG_f32"] == int(plan["dgrad"] == 0 or ("W" in C.grads and plan["wgrad"] != 1)), (case, plan)


def test_table_covers_every_route_and_form():
    L = _lib.lib()
    plans = {case: plan_of(L, case) for case in R.CASES}
    got = R.reached(plans)
    print({k: sorted(v, key=repr) for k, v in got.items()})
    assert set(got) == set(R.REQUIRED)
    for k in R.REQUIRED:
        assert got[k] == R.REQUIRED[k], (k, sorted(got[k], key=repr), sorted(R.REQUIRED[k], key=repr))
    C = R.CASES
    assert {C[c].prec for c in C} == {"f32", "bf16x3", "bf16"} and all(C[c].shape[6] <= 3 for c in C)
    assert all(plans[c]["hh_split"] > 1 for c in ("hoist_convq", "hoist_gen1_on_convq_shape", "hoist_f32", "hoist_no_state"))
    # twins and families in both directions: every twin has a second / third generation case of its shape and precision beside it, and
    # every such case has a forced first-generation twin
    assert got["twins"] == got["families"]
    # the fuzz sweep's cap on the statement's cost
    for c in C:
        Cin, Ch, H, W, k, B, T = C[c].shape
        assert B * T * H * W * (Cin + Ch) * Ch * k * k <= 3e9, c


# ---- dry run ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_case_runs_inside_the_queried_workspace_and_reserve(case):
    L = _lib.lib()
    C = R.CASES[case]
    has = lambda n, i: _fake(i) if n in R.present(C.ops) else None
    want = lambda n, i: _fake(i) if n in C.grads else None
    save = bool(C.grads)
    with settings(L, case), _lib.option(_lib.OPT_DRY_RUN, 1):
        d = _desc(case)
        nb, rs = L.vpx_convlstm_workspace_bytes(ctypes.byref(d)), L.vpx_convlstm_reserve_bytes(ctypes.byref(d))
        assert nb > 256 and (rs > 0) == save, (case, nb, rs)

        def fwd(rs_, nb_):
            return L.vpx_convlstm_seq_fwd(ctypes.byref(d), *[has(n, i) for i, n in enumerate(R.LEAVES, 1)], _fake(9), _fake(10), _fake(11),
                                          _fake(12) if save else None, rs_, ctypes.c_void_p(WS_BASE), nb_, None)

        def bwd(rs_, nb_, null_unreached):
            # the incoming gradients: all three as `ops.convlstm_seq` passes them (autograd hands its backward zeros for an output the loss
            # does not reach), or NULL for those, as the raw call of tests/test_gpu_convlstm_routes.py passes them
            gin = [_fake(13 + i) if o in R.LOSSES[C.loss] or not null_unreached else None for i, o in enumerate(R.OUTS)]
            return L.vpx_convlstm_seq_bwd(ctypes.byref(d), *[has(n, i) for i, n in enumerate(R.LEAVES, 1) if n != "b"], _fake(9), _fake(12), rs_, *gin,
                                          *[want(n, 16 + i) for i, n in enumerate(R.LEAVES)], ctypes.c_void_p(WS_BASE), nb_, None)
        bwd_zeros, bwd_null = (lambda r, n: bwd(r, n, False)), (lambda r, n: bwd(r, n, True))
        for name, call in ((("fwd", fwd), ("bwd", bwd_zeros), ("bwd, NULL cotangents", bwd_null)) if save else (("fwd", fwd),)):
            tag = f"{case} {name}"
            assert call(rs, nb) == OK, (tag, L.vpx_last_error())
            assert call(rs, nb - 256) == E_WS, (tag, "workspace 256 bytes short")
            if save:
                assert call(rs - 1, nb) == E_WS, (tag, "reserve one byte short")


# ---- the inputs' condition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_fp32_reference_holds_half_the_f32_bars(case):
    """The reference's own fp32 CPU run against its fp64 run, outputs 5e-6, gradients 2.5e-5: measured from the reference alone."""
    ref, r32 = R.cpu(case), R.cpu(case, torch.float32)
    C = R.CASES[case]
    assert set(ref) == set(r32) == set(R.OUTS) | {"grad." + n for n in C.grads}
    errs = {k: R.relmax(r32[k], ref[k]) for k in ref}
    worst = lambda pre: max((v for k, v in errs.items() if k.startswith("grad.") == pre), default=0.0)
    print(f"{case}: worst output {worst(False):.2e}, worst gradient {worst(True):.2e}")
    assert worst(False) <= R.COND[0] and worst(True) <= R.COND[1], {k: f"{v:.2e}" for k, v in errs.items()}
    if case == "cell2_q_x_only_t1":   # c_0 = 0 and one step: the loss does not reach the input and forget peepholes
        assert not ref["grad.Wci"].any() and not ref["grad.Wcf"].any() and ref["grad.Wco"].any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_plan_query_refuses_what_the_size_query_refuses():
    L = _lib.lib()
    info = ConvLSTMPlanInfo()
    good = dict(B=2, T=3, Cin=8, Ch=16, H=9, W=17, kh=3, kw=3, gate_order=0, layout=0, precision=1, flags=1)

    def rc_of(**kw):
        d = ConvLSTMDesc(**{**good, **kw})
        rc = L.vpx_convlstm_plan(ctypes.byref(d), 1, 1, 1, ctypes.byref(info))
        assert (L.vpx_convlstm_workspace_bytes(ctypes.byref(d)) == 0) == (rc != OK), kw
        return rc
    assert rc_of() == OK
    for dim in ("B", "T", "Cin", "Ch", "H", "W"):
        for v in (0, -3):
            assert rc_of(**{dim: v}) in (E_ARG, E_UNSUPPORTED), (dim, v)
    for kw in (dict(kh=2), dict(kw=4), dict(kh=0), dict(precision=-1), dict(precision=3), dict(layout=2), dict(gate_order=2)):
        assert rc_of(**kw) in (E_ARG, E_UNSUPPORTED), kw
    d = ConvLSTMDesc(**good)
    assert L.vpx_convlstm_plan(ctypes.byref(d), 1, 1, 1, None) == E_ARG and L.vpx_convlstm_plan(None, 1, 1, 1, ctypes.byref(info)) == E_ARG
    assert rc_of() == OK                                      # (the next valid query)
    # without VPX_FLAG_SAVE_FOR_BWD the backward half is zero
    assert rc_of(flags=0) == OK and not any(getattr(info, n) for n in ("dgrad", "dgrad_qform", "d_mw", "dgrad_cols", "wgrad", "n_slices", "dG_f32", "gate_slices"))
