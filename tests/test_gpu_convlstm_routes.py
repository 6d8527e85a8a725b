"""The ConvLSTM sequence (vpx_convlstm_seq_fwd / _bwd through `ops.convlstm_seq`) against float64 on every route of both directions: one
test per case of tests/convlstm_ref.py. Each case first asserts, through vpx_convlstm_plan under its own options, experiment bits and
deterministic setting, that it is on the plan it was written for (tests/test_convlstm_host.py holds the whole table and its coverage on
the CPU), then compares out, hT, cT and every requested gradient with `oracle.torch_ref.convlstm_hzzone_seq` run on the CPU in float64
under autograd on the same float32 inputs.

Bars, in max|d| / max|ref| (convlstm_ref.BARS): f32 outputs 1e-5, gradients 5e-5; bf16x3 outputs 6e-5, gradients 2e-4 (stlstm_ref.BARS);
plain bf16 outputs 1e-2, forward only (test_plain_bf16_on_the_q_kernel...). A gradient whose reference is exactly zero (the input and forget
peepholes of a one-step call without an initial state) must be zero bit for bit: the metric divides by max|ref| + 1e-30. No element and
no case is left out. A deterministic case runs twice and must give the same bits. Every figure goes through `parity_log` into the
session's parity record as `convlstm.<case>.<tensor>`; profiles/parity_convlstm_routes.json holds the worst output and gradient error per
case from it.

Incoming gradients. `ops.convlstm_seq` never hands the library a NULL cotangent: autograd gives its backward zeros for an output the loss
does not reach. The cases whose loss leaves an output out (`out` alone: no dhT, no dcT; `hT` and `cT` alone: no dout) therefore run a
second time through the raw C ABI (vpx_convlstm_seq_fwd / _bwd on NHWC buffers) with NULL in those places, which is what reaches the gate
backward's branches for a missing dout / dhT / dcT, and are held to the same float64 reference under `convlstm.<case>.abi.<tensor>`."""
import contextlib
import ctypes

import pytest
import torch

import convlstm_ref as R
import test_convlstm_host as H

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _settings(vpx, case):
    """The case's options and experiment bits; the deterministic setting through torch's switch, which the op mirrors into the library."""
    C = R.CASES[case]
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(bool(C.det))
    try:
        with contextlib.ExitStack() as stack:
            for name, value in C.opts.items():
                stack.enter_context(vpx._lib.option(getattr(vpx._lib, name), value))
            stack.enter_context(vpx._lib.experiment(vpx._lib.exp_bits(C.exp)))
            yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _gpu(vpx, case):
    C = R.CASES[case]
    Cin, T = C.shape[0], C.shape[6]

    def seq(x, h0, c0, W, b, Wci, Wcf, Wco):
        return vpx.ops.convlstm_seq(x, h0, c0, W, b, Wci, Wcf, Wco, seq_len=T, in_channels=Cin, gate_order=C.order, precision=C.prec)
    t = {n: v.cuda() for n, v in R.inputs(case).items()}
    with _settings(vpx, case):
        return {k: v.cpu() for k, v in R.evaluate(seq, t, C.ops, C.grads, C.loss).items()}


def _gpu_abi(vpx, case):
    """The case through the raw C ABI, NHWC: NULL for absent operands, for gradients not asked for and for every cotangent the loss
    leaves out. Returns what _gpu returns."""
    C = R.CASES[case]
    Cin, Ch, Hh, W, k, B, T = C.shape
    L, p, ops = vpx._lib.lib(), vpx._lib.ptr, vpx.ops
    has = R.present(C.ops)
    t = {n: v.cuda() for n, v in R.inputs(case).items()}
    op = {n: (ops.to_channels_last(t[n]) if n in has and n not in ("W", "b") else (t[n].contiguous() if n in has else None)) for n in R.LEAVES}
    cot = {o: (ops.to_channels_last(t["g." + o]) if o in R.LOSSES[C.loss] else None) for o in R.OUTS}
    out, hT, cT = (ops.new_channels_last(sh, "cuda") for sh in ((B, T, Ch, Hh, W), (B, Ch, Hh, W), (B, Ch, Hh, W)))
    grad = {n: (ops.new_channels_last(tuple(t[n].shape), "cuda") if t[n].dim() >= 4 and n != "W" else torch.empty_like(t[n])) if n in C.grads else None
            for n in R.LEAVES}
    with _settings(vpx, case):
        ops.sync_determinism()
        d = H._desc(case)
        nb, rs = L.vpx_convlstm_workspace_bytes(ctypes.byref(d)), L.vpx_convlstm_reserve_bytes(ctypes.byref(d))
        assert nb > 0 and rs > 0, (case, L.vpx_last_error())
        ws, res = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(rs, dtype=torch.uint8, device="cuda")
        rc = L.vpx_convlstm_seq_fwd(ctypes.byref(d), *[p(op[n]) for n in R.LEAVES], p(out), p(hT), p(cT), p(res), rs, p(ws), nb, ops.stream())
        assert rc == 0, (case, L.vpx_last_error())
        rc = L.vpx_convlstm_seq_bwd(ctypes.byref(d), *[p(op[n]) for n in R.LEAVES if n != "b"], p(out), p(res), rs, *[p(cot[o]) for o in R.OUTS],
                                    *[p(grad[n]) for n in R.LEAVES], p(ws), nb, ops.stream())
        assert rc == 0, (case, L.vpx_last_error())
        torch.cuda.synchronize()
    got = {"out": out.cpu(), "hT": hT.cpu(), "cT": cT.cpu()}
    got.update({"grad." + n: grad[n].cpu() for n in C.grads})
    return got


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


@pytest.mark.parametrize("case", list(R.CASES))
def test_convlstm_route_vs_oracle_fp64(vpx, parity_log, case):
    C = R.CASES[case]
    plan = H.plan_of(vpx._lib.lib(), case)
    assert {k: plan[k] for k in C.plan} == C.plan, (case, plan)
    ref = R.cpu(case)
    assert len(ref) == 3 + len(C.grads)
    got = _gpu(vpx, case)
    bad = _check(parity_log, f"convlstm.{case}", got, ref, R.BARS[C.prec])
    assert not bad, (case, bad)
    for k, r in ref.items():
        if not r.any():
            assert not got[k].any(), (case, k, "the reference is exactly zero")
    if C.grads and C.loss != "out_cT":   # a loss that leaves out dout, or dhT and dcT: once more with NULL in their places
        raw = _gpu_abi(vpx, case)
        bad = _check(parity_log, f"convlstm.{case}.abi", raw, ref, R.BARS[C.prec])
        assert not bad, (case, "raw C ABI, NULL cotangents", bad)
    if C.det:
        again = _gpu(vpx, case)
        differ = [k for k in got if not torch.equal(got[k], again[k])]
        assert not differ, (case, "two deterministic runs", differ)
