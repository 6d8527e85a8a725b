"""The TrajGRU sequence (vpx_trajgru_seq_fwd / _bwd through `traj_ops.trajgru_seq`; csrc/trajgru.hip) against float64 on every route of
both directions: one test per case of tests/trajgru_seq_ref.py and operand mode (f32, bf16x3). A case goes through the public op with its
leaves requiring a gradient and its loss; out, hT and every requested gradient are compared with `oracle.torch_ref.trajgru_seq(...,
i2h_pad=k // 2)` run on the CPU in float64 under autograd on the same float32 inputs. tests/test_trajgru_seq_cases.py shows on the CPU
that no case sits on a kink (sampling coordinates at least 1e-4 px from every integer, LeakyReLU pre-activations at least 1e-5 from 0,
and both at least ten times what the f32 and the bf16x3 arithmetic move them), that the flow generator's own flows reach 2.2 to 4.7 px,
and that the table covers k_i2h 1/3/5/7, T 1..4, L 1/3/5/13, C 4/8/12/32, Cin 1/3/4/8, B 1..3, maps 1x1 to 9x6, the forecaster (x NULL) and
zero-state (h0 NULL) forms, three losses, four gradient sets, deterministic mode. No element and no case is left out.

Bars, in max|d| / max|ref| (trajgru_seq_ref.bars): outputs 2e-5 (f32) / 1e-4 (bf16x3), gradients 1e-4 (f32) / 2e-4 (bf16x3); a bar
would become 3 x the matching CPU restatement's own error against float64 where that exceeds a third of it, and none does (measured worst:
f32 1.0e-6 outputs / 2.2e-6 gradients, bf16x3 1.5e-5 / 4.2e-5), so every tensor is held to the base bar. REJECTED seeds: the table in
trajgru_seq_ref.py, with the reason for each. A gradient whose reference is exactly zero (the whole flow generator's, in a one-step call
without h0: the warps sample zeros) must be zero bit for bit. A leaf that did not ask for a gradient has none; in the forecaster form
the four input-side parameters have none. A deterministic case runs twice and must give the same bits. Every figure goes through
`parity_log` as `trajgru.<case>.<prec>.<tensor>`; all figures of a run are measured and printed before any is judged.
profiles/parity_trajgru_routes.json holds the worst output and gradient error per case and mode.

Incoming gradients. Autograd hands the op's backward zeros for an output the loss does not reach, never NULL. The cases whose loss is
`out` alone or `hT` alone therefore run once more through the raw C ABI on time-major NHWC buffers, as traj_ops builds them, with NULL
for the missing cotangent, for dx / dh0 where not asked for and for the four input-side parameter gradients of a forecaster call (the
other parameter gradients are mandatory in the ABI: include/vpx.h), and are held to the same reference under
`trajgru.<case>.abi.<prec>.<tensor>`.

The "none" gradient set is the inference route (no VPX_FLAG_SAVE_FOR_BWD: workspace buffers instead of the reserve) under no_grad; in
a deterministic case its outputs must equal the training call's bit for bit."""
import ctypes

import pytest
import torch

import trajgru_seq_ref as R

pytestmark = pytest.mark.gpu


class _deterministic:
    """Torch's switch, which the op mirrors into the library, for the duration of a case; restored on the way out."""
    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        self.prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.prev)


def _op_seq(case, prec):
    from vp_suite_amd import traj_ops

    def seq(x, h0, P):
        return traj_ops.trajgru_seq(x, h0, [P[k] for k in R.PARAM_KEYS], seq_len=case.T, L=case.L, slope=R.SLOPE, state_hw=(case.H, case.W),
                                    precision=prec)
    return seq


def _gpu(tag, prec, seq=None, grads=None):
    """The case through `seq` (default: the public op). Returns (tensors on the CPU, leaves). grads: another gradient set than the case's."""
    case = R.CASES[tag] if grads is None else R.CASES[tag]._replace(grads=grads)
    t = {n: v.cuda() for n, v in R.inputs(tag).items()}
    with _deterministic(case.det):
        res, lv = R.evaluate(seq or _op_seq(case, prec), t, case)
        res = {k: v.cpu() for k, v in res.items()}
    return res, lv


def _nhwc(t):
    nd = t.dim()
    return t.permute(*range(nd - 3), nd - 2, nd - 1, nd - 3).contiguous()


def _nchw(t):
    nd = t.dim()
    return t.permute(*range(nd - 3), nd - 1, nd - 3, nd - 2)


def _gpu_abi(vpx, tag, prec):
    """The case through vpx_trajgru_seq_fwd / _bwd: x [T][B][HW][Cin], h0 [B][HW][C], hs / dout [T][B][HW][C], dhT / dh0 [B][HW][C], dx like x;
    NULL for absent operands, for the cotangent the loss leaves out and for every gradient the ABI lets a caller leave out. Returns what
    _gpu returns first."""
    case = R.CASES[tag]
    L, p, pa, ops = vpx._lib.lib(), vpx._lib.ptr, vpx._lib.ptr_array, vpx.ops
    B, T, Cin, C, H, W = case.B, case.T, case.Cin, case.C, case.H, case.W
    want = R.leaves(case)
    t = {n: v.cuda() for n, v in R.inputs(tag).items()}
    x = _nhwc(t["x"].transpose(0, 1)) if R.has_x(case) else None
    h0 = _nhwc(t["h0"]) if R.has_h0(case) else None
    params = [t[k].contiguous() for k in R.PARAM_KEYS]
    dout = t["g.out"].permute(1, 0, 3, 4, 2).contiguous() if "out" in R.LOSSES[case.loss] else None
    dhT = _nhwc(t["g.hT"]) if "hT" in R.LOSSES[case.loss] else None
    hs = torch.empty(T, B, H, W, C, device="cuda")
    dx = torch.empty(T, B, H, W, Cin, device="cuda") if "x" in want else None
    dh0 = torch.empty(B, H, W, C, device="cuda") if "h0" in want else None
    dparams = [torch.empty_like(q) if (R.has_x(case) or i >= 4) else None for i, q in enumerate(params)]
    with _deterministic(case.det):
        ops.sync_determinism()
        d = vpx._lib.TrajGRUDesc(B, T, Cin, C, H, W, case.L, case.k, ops.PRECISIONS[prec], vpx._lib.FLAG_SAVE_FOR_BWD, R.SLOPE)
        nb, rs = L.vpx_trajgru_workspace_bytes(ctypes.byref(d)), L.vpx_trajgru_reserve_bytes(ctypes.byref(d))
        assert nb > 0 and rs > 0, (tag, L.vpx_last_error())
        ws, res = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(rs, dtype=torch.uint8, device="cuda")
        rc = L.vpx_trajgru_seq_fwd(ctypes.byref(d), p(x), p(h0), pa(params), p(hs), p(res), rs, p(ws), nb, ops.stream())
        assert rc == 0, (tag, L.vpx_last_error())
        rc = L.vpx_trajgru_seq_bwd(ctypes.byref(d), p(x), p(h0), pa(params), p(hs), p(res), rs, p(dout), p(dhT), p(dx), p(dh0), pa(dparams), p(ws), nb,
                                   ops.stream())
        assert rc == 0, (tag, L.vpx_last_error())
        torch.cuda.synchronize()
    got = {"out": hs.permute(1, 0, 4, 2, 3).cpu(), "hT": _nchw(hs[T - 1]).cpu()}
    grad = dict(zip(R.PARAM_KEYS, dparams))
    grad.update(x=None if dx is None else dx.permute(1, 0, 4, 2, 3), h0=None if dh0 is None else _nchw(dh0))
    got.update({"grad." + n: grad[n].cpu() for n in want})
    return got


def _check(log, tag, prec, got, ref, label=None):
    """Every entry of `ref` against `got` at the case's bars; all figures are measured and printed before any is judged."""
    assert set(got) == set(ref), (tag, sorted(set(got) ^ set(ref)))
    bars, errs, bad = R.bars(tag, prec), {}, []
    name = f"trajgru.{tag}.{label + '.' if label else ''}{prec}"
    for k, r in ref.items():
        assert got[k].shape == r.shape, (tag, k, tuple(got[k].shape), tuple(r.shape))
        errs[k] = log(f"{name}.{k}", got[k], r, bars[k][0])
        if not errs[k] < bars[k][0]:
            bad.append((k, errs[k], bars[k][0]))
    worst = lambda pre: max((v for k, v in errs.items() if k.startswith("grad.") == pre), default=0.0)
    print(f"{name}: worst output {worst(False):.2e}, worst gradient {worst(True):.2e}")
    for k, r in ref.items():
        if not r.any():
            assert not got[k].any(), (tag, prec, label, k, "the reference is exactly zero")
    return bad


def _check_absent_grads(case, lv):
    want = R.leaves(case)
    for n, leaf in lv.items():
        if n not in want:   # did not ask, or (the input-side parameters of a forecaster call) asked and is not part of the call
            assert leaf.grad is None, (case.tag, n, "has a gradient")
    if not R.has_x(case) and case.grads in ("all", "params"):
        assert all(lv[n].requires_grad and lv[n].grad is None for n in R.INPUT_SIDE), case.tag


@pytest.mark.parametrize("prec", R.MODES)
@pytest.mark.parametrize("case", list(R.CASES))
def test_trajgru_route_vs_oracle_fp64(vpx, parity_log, case, prec):
    tag, case = case, R.CASES[case]
    ref = R.reference(tag).tensors
    assert len(ref) == 2 + len(R.leaves(case))
    got, lv = _gpu(tag, prec)
    bad = _check(parity_log, tag, prec, got, ref)
    assert not bad, (tag, prec, bad)
    _check_absent_grads(case, lv)
    if case.grads != "none" and case.loss != "out_hT":   # a loss that leaves out dhT, or dout: once more with NULL in its place
        raw = _gpu_abi(vpx, tag, prec)
        bad = _check(parity_log, tag, prec, raw, ref, "abi")
        assert not bad, (tag, prec, "raw C ABI, NULL cotangent", bad)
    if case.det:
        again, _ = _gpu(tag, prec)
        differ = [k for k in got if not torch.equal(got[k], again[k])]
        assert not differ, (tag, prec, "two deterministic runs", differ)
        if case.grads == "none":   # the inference route against the saving one: other buffers, the same launches
            train, _ = _gpu(tag, prec, grads="all")
            differ = [k for k in ("out", "hT") if not torch.equal(got[k], train[k])]
            assert not differ, (tag, prec, "inference against the training call", differ)


@pytest.mark.parametrize("prec", R.MODES)
def test_trajgru_module_passes_its_i2h_kernel_through(vpx, parity_log, prec):
    """TrajGRU(i2h_kernel=(5, 5), i2h_pad=(2, 2)) as a module on the table's 5x5 case: the same reference, the same bars."""
    from vp_suite_amd.model_blocks.traj_gru import TrajGRU
    tag = R.MODULE_CASE
    case = R.CASES[tag]
    block = TrajGRU("cuda", case.Cin, case.C, case.H, case.W, L=case.L, i2h_kernel=(case.k, case.k), i2h_pad=(case.k // 2, case.k // 2)).cuda()
    block.precision = prec
    assert tuple(block.i2h.weight.shape) == R.shapes(case)["i2h"]

    def seq(x, h0, P):
        mods = dict(block.named_parameters())
        assert set(mods) == set(R.PARAM_KEYS)
        for k in R.PARAM_KEYS:   # the leaves of evaluate() in the module's slots
            n, kind = k.split(".")
            delattr(getattr(block, n), kind)
            setattr(getattr(block, n), kind, P[k])
        return block(x, h0, case.T)
    got, _ = _gpu(tag, prec, seq=seq)
    bad = _check(parity_log, tag, prec, got, R.reference(tag).tensors, "module")
    assert not bad, (tag, prec, bad)
