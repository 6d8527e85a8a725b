"""The plain ST-LSTM step (vpx_stlstm_step_fwd_ex / _bwd_ex through `ops.stlstm_step`) against float64 on every route of both directions:
one test per case of tests/stlstm_ref.py. Each case first asserts, through vpx_stlstm_plan under its own experiment bits and deterministic
setting, that it is on the plan it was written for (tests/test_stlstm_host.py holds the whole table and its coverage on the CPU), then
compares all five outputs and every requested gradient with `oracle.torch_ref.stlstm_cell` run on the CPU in float64 under autograd on the
same float32 inputs.

Bars, in max|d| / max|ref| (stlstm_ref.BARS): f32 outputs 1e-5, gradients 5e-5 (RTOL / GRTOL of test_gpu_stlstm.py); bf16x3 outputs 6e-5,
gradients 2e-4 (test_random_stlstm_steps_vs_oracle); plain bf16 outputs 3e-2, forward only. A gradient whose reference is exactly zero
(conv_o / conv_last under a loss on c_new and delta_m) must be zero bit for bit: the metric divides by max|ref| + 1e-30. No element and no
case is left out. A deterministic case runs twice and must give the same bits. Every figure goes through `parity_log` into the session's
parity record as `stlstm.<case>.<tensor>`; profiles/parity_stlstm_routes.json holds the worst output and gradient error per case from it."""
import contextlib

import pytest
import torch

import stlstm_ref as R
import test_stlstm_host as H

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _deterministic(on):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(bool(on))
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _device_inputs(case):
    """The case's inputs on the GPU in its layout: contiguous NCHW; channels-last; or (`sliced`) x a channel slice and h, c, m column
    slices of wider tensors, all four non-contiguous."""
    C = R.CASES[case]
    t = {n: v.cuda() for n, v in R.inputs(case).items()}
    if C.layout == "channels_last":
        for n in R.STATES:
            t[n] = t[n].contiguous(memory_format=torch.channels_last)
    elif C.layout == "sliced":
        B, Cin, H_, W = t["x"].shape
        wide = torch.full((B, Cin + 5, H_, W), 7.0, device="cuda")
        wide[:, 2:2 + Cin] = t["x"]
        t["x"] = wide[:, 2:2 + Cin]
        for n in ("h", "c", "m"):
            wide = torch.full(tuple(t[n].shape[:3]) + (W + 3,), -7.0, device="cuda")
            wide[..., 1:1 + W] = t[n]
            t[n] = wide[..., 1:1 + W]
        assert not any(t[n].is_contiguous() for n in R.STATES)
    return t


def _gpu(vpx, case):
    C = R.CASES[case]
    ln = bool(C.shape[5])

    def step(x, h, c, m, lv):
        return vpx.ops.stlstm_step(x, h, c, m, *(lv[w] for w in R.WEIGHTS), precision=C.prec, ln=[lv[n] for n in R.LN_NAMES] if ln else (),
                                   use_shadows=C.loss == "two_step")
    with _deterministic(C.det), vpx._lib.experiment(vpx._lib.exp_bits(C.exp)):
        return {k: v.cpu() for k, v in R.evaluate(step, _device_inputs(case), C.shape, C.grads, C.loss).items()}


def _check(log, tag, got, ref, tol):
    """Every entry of `ref` against `got` at tol = (outputs, gradients); all figures are measured and printed before any is judged."""
    assert set(got) == set(ref), (tag, sorted(set(got) ^ set(ref)))
    errs, bad = {}, []
    for k, r in ref.items():
        assert got[k].shape == r.shape, (tag, k, tuple(got[k].shape), tuple(r.shape))
        bound = tol[1] if k.startswith("grad.") else tol[0]
        errs[k] = log(f"{tag}.{k}", got[k], r, bound)
        if not errs[k] < bound:
            bad.append((k, errs[k], bound))
    worst = lambda pre: max((v for k, v in errs.items() if k.startswith("grad.") == pre), default=0.0)
    print(f"{tag}: worst output {worst(False):.2e}, worst gradient {worst(True):.2e}")
    return bad


def _run(vpx, parity_log, case):
    C = R.CASES[case]
    plan = H.plan_of(vpx._lib.lib(), case)[0]
    stated = {k: (tuple(v) if k in H.ARRAYS else v) for k, v in C.plan.items()}
    assert {k: plan[k] for k in stated} == stated, (case, plan)
    ref = R.cpu(case)
    assert len(ref) == (10 if C.loss == "two_step" else 5) + len(C.grads)
    got = _gpu(vpx, case)
    bad = _check(parity_log, f"stlstm.{case}", got, ref, R.BARS[C.prec])
    assert not bad, (case, bad)
    if C.loss == "c_dm":
        assert not got["grad.Wo"].any() and not got["grad.Wlast"].any()
    if C.det:
        again = _gpu(vpx, case)
        differ = [k for k in got if not torch.equal(got[k], again[k])]
        assert not differ, (case, "two deterministic runs", differ)


_LN = [c for c in R.CASES if R.CASES[c].shape[5]]
_BF16 = [c for c in R.CASES if R.CASES[c].prec == "bf16"]
_REST = [c for c in R.CASES if c not in _LN and c not in _BF16]


@pytest.mark.parametrize("case", _REST)
def test_stlstm_route_vs_oracle_fp64(vpx, parity_log, case):
    _run(vpx, parity_log, case)


@pytest.mark.parametrize("case", _LN)
def test_stlstm_route_vs_oracle_fp64_ln(vpx, parity_log, case):
    _run(vpx, parity_log, case)


@pytest.mark.parametrize("case", _BF16)
def test_stlstm_route_vs_oracle_fp64_plain_bf16(vpx, parity_log, case):
    _run(vpx, parity_log, case)
