"""The stage glue on the GPU — vpx_conv2d_ex_fwd / _fwd_from_split / _bwd_ex (behind ops.conv2d_ex and ops.conv2d_ex_from_split) and
vpx_conv2d_act_fwd / _bwd (behind stphy_ops.conv2d_act) — against the fp64 statement of tests/glue_ref.py, whose tables walk every route
of csrc/glue_fwd_api.hip / glue_bwd_api.hip: the streaming kernels of conv_small.hip in both forms, the first-generation implicit GEMM (stride 1 and 2, flipped
taps, the four phase launches with their tap map, 4-wave and 8-wave workgroups), conv16.hip and convq.hip on split input, launch_colsum
in its vector and scalar form with and without a split copy, the data gradient as the adjoint layer with every output padding on the
first generation and on convq, and the weight gradient on wgrad_small_kernel, on launch_wgrad per stride residue and on wgrad2_kernel's
glue form. tests/test_glue_host.py holds which case takes which route.

Every comparison is max|got - ref| / max|ref| against the fp64 run and goes through the parity record (parity_log; parity.relmax for the
comparisons of two launches with each other). Bars (conv_same_ref.BARS), forward / gradients: f32 1e-5 / 2e-5, bf16x3 5e-5 / 1e-4; two
launches of the same products 2e-5. The upstream gradient is zero on the activation's kink (glue_ref), so LeakyReLU' / ReLU' on the
reference's side comes from its own fp64 pre-activation. Destinations come from torch.empty: the guard bands of tests/canary.py stand
around every one of them and around every workspace.

Measured, one MI355X run of this file (every figure below is in that run's parity record — the parity_r06.json that tests/conftest.py
writes at the end of a `-m gpu` session — under this file's test names); worst over the cases:
  test_conv2d_ex_vs_fp64                f32:    y 1.0e-6 (FLIP 7x7 p3), dx 1.0e-6, dw 5.6e-7, db 5.4e-7
                                        bf16x3: y 1.1e-5 (PHASES 2x2 p1 op 1,0), dx 1.1e-5 (FLIP 1x1), dw 1.4e-5 (SMALL 4 -> 1), db 5.4e-7
  test_conv2d_act_relu_vs_fp64          f32: y 3.0e-7, gradients 2.7e-7; bf16x3: y 5.4e-6, gradients 7.8e-6 (STRIDED 3x3 p1, dw)
  test_eight_wave_workgroups_...        y 7.2e-6 (stride 2, both calls), dx 5.3e-6, dw 4.5e-6, db 9.9e-8
  test_split_training_call_...          y 6.6e-6, dx 7.1e-6, dw 6.8e-6 (8 -> 8 5x5 s2), db 2.3e-7; GLUE_WGRAD_TAPGROUP off against on 2.7e-7 (bar 2e-5)
  test_c16_gate_...                     y 6.9e-6, dx 6.8e-6, dw 5.2e-6; NO_C16 off against on 4.0e-7
  test_forward_from_split_input_...     y 6.9e-6 (C16 32 -> 16), before and after the weight update
  test_convq_forward_with_output_...    y 5.6e-6
  test_data_gradient_on_convq_...       y 7.5e-6, dx 7.6e-6 (4x4 s2 on 9x12), dw 6.5e-6; GLUE_DGRAD_GEN1 off against on 2.0e-7
  test_deterministic_mode_...           dx 7.6e-6, dw 6.1e-6; the second run equal bit for bit
  test_backward_that_wants_dx_or_dw_... y 4.8e-6, dx 7.6e-6, dw 6.1e-6, db 1.0e-7 (the calls for dx or dw alone give the full call's figures);
                                        in deterministic mode equal to the full call bit for bit
No case needed a bar other than the table's. Not measured: nothing — every test of the file ran. 298 tests; the file takes 4.8 s."""
import ctypes

import pytest
import torch

import glue_ref as R
from parity import relmax as _relmax

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [R.case_id(c[0], c[1]) + "".join(f"-{e}" for e in c[2:]) for c in cases]


def _hold(parity_log, name, got, ref, bar):
    e = parity_log(name, got, ref, bar)
    print(f"  {name}: {e:.3e} (bar {bar:.0e})")
    assert e < bar, (name, e, bar)
    return e


def _run(vpx, table, i, prec, relu=False, grads=True, need=(True, True)):
    """Case i through ops.conv2d_ex (relu: stphy_ops.conv2d_act) under its variant: (y, dx, dw, db or None). need: whether x / w require a
    gradient (a bias always does); what is not wanted comes back as None."""
    c, v = R.TABLES[table][i], R.variant(table, i)
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    t, ref, _ = R.case(table, i, relu)
    x = t["x"].cuda()
    if v["channels_last"]:
        x = x.contiguous(memory_format=torch.channels_last)
    leaves = [x.requires_grad_(grads and need[0]), t["w"].cuda().requires_grad_(grads and need[1])] + ([t["b"].cuda().requires_grad_(grads)] if v["bias"] else [])
    b = leaves[2] if v["bias"] else None
    with torch.set_grad_enabled(grads):
        if relu:
            from vp_suite_amd import stphy_ops
            y = stphy_ops.conv2d_act(leaves[0], leaves[1], b, s, p, bool(tr), "relu", prec)
        else:
            y = vpx.ops.conv2d_ex(leaves[0], leaves[1], b, s, p, bool(tr), v["slope"], prec, (oph, opw))
    assert y.shape == (N, Co) + R.out_shape(c) and y.permute(0, 2, 3, 1).is_contiguous()
    if not grads:
        return y, None, None, None
    # torch.autograd.grad hands out what the backward returned (a leaf's .grad would be restrided to the leaf's own layout)
    wanted = [k for k, leaf in enumerate(leaves) if leaf.requires_grad]
    g = dict(zip(wanted, torch.autograd.grad(y, [leaves[k] for k in wanted], t["gy"].cuda())))
    assert 0 not in g or (g[0].shape == x.shape and g[0].permute(0, 2, 3, 1).is_contiguous())
    assert 1 not in g or g[1].shape == t["w"].shape
    return y, g.get(0), g.get(1), g.get(2)


def _hold_all(parity_log, out, ref, prec, tag=""):
    fwd, grad = R.BARS[prec]
    _hold(parity_log, "y" + tag, out[0], ref["y"], fwd)
    for k, g in zip(("dx", "dw", "db"), out[1:]):
        if g is not None:
            assert not bool(torch.isnan(g).any()), k
            _hold(parity_log, k + tag, g, ref[k], grad)
    assert (out[3] is None) == (ref["db"] is None)


def _deterministic(vpx, fn):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        return fn()
    finally:
        torch.use_deterministic_algorithms(prev)
        vpx.ops.sync_determinism()


# ---- ops.conv2d_ex in both operand modes: phases, strides, flipped taps, the few-channel layers ------------------------------------------
EX_CASES = [(t, i, p) for t in R.BOTH_MODES for i in range(len(R.TABLES[t])) for p in ("f32", "bf16x3")]


@pytest.mark.parametrize("table,i,prec", EX_CASES, ids=_ids(EX_CASES))
def test_conv2d_ex_vs_fp64(vpx, parity_log, table, i, prec):
    print(R.case_id(table, i), prec, R.variant(table, i))
    _hold_all(parity_log, _run(vpx, table, i, prec), R.case(table, i)[1], prec)


ACT_CASES = [(t, i, p) for t, i in R.ACT for p in ("f32", "bf16x3")]


@pytest.mark.parametrize("table,i,prec", ACT_CASES, ids=_ids(ACT_CASES))
def test_conv2d_act_relu_vs_fp64(vpx, parity_log, table, i, prec):
    """ReLU in the epilogue, ReLU' read off the saved output in launch_colsum (Co % 4 == 0: the vector form; else the scalar one). The
    SMALL shape runs on the implicit GEMM: the streaming kernels know LeakyReLU only."""
    _hold_all(parity_log, _run(vpx, table, i, prec, relu=True), R.case(table, i, True)[1], prec)
    ref = R.case(table, i, True)[1]
    assert float(ref["y"].min()) == 0.0 and float((ref["y"] == 0).double().mean()) > 0.2     # (ReLU is at work)


@pytest.mark.parametrize("i", range(len(R.WAVES8)), ids=_ids([("WAVES8", i) for i in range(len(R.WAVES8))]))
def test_eight_wave_workgroups_on_ragged_maps_vs_fp64(vpx, parity_log, i):
    """17 x 33 maps: the second half of every 16-row tile of the 8-wave form holds one row. An inference call (fp32 input) and a training
    call (x converted once, the forward from split input), each against fp64."""
    ref = R.case("WAVES8", i)[1]
    y, _, _, _ = _run(vpx, "WAVES8", i, "bf16x3", grads=False)
    _hold(parity_log, "y.inference", y, ref["y"], R.BARS["bf16x3"][0])
    _hold_all(parity_log, _run(vpx, "WAVES8", i, "bf16x3"), ref, "bf16x3")


# ---- bf16x3 training calls on split operands ------------------------------------------------------------------------------------------
def _ab(vpx, parity_log, table, i, bit, same=("y", "dx", "dw", "db")):
    """Case i with the option bit off and on: each against fp64, and against each other to SAME_PRODUCTS."""
    ref = R.case(table, i)[1]
    outs = {}
    for bits in (0, bit):
        with vpx._lib.experiment(bits):
            outs[bits] = _run(vpx, table, i, "bf16x3")
        _hold_all(parity_log, outs[bits], ref, "bf16x3", f".bit{bits.bit_length() - 1 if bits else 'off'}")
    for k, a, b in zip(("y", "dx", "dw", "db"), outs[0], outs[bit]):
        if a is not None and k in same:
            e = _relmax(a, b)
            print(f"  {k}: bit off against on {e:.3e}")
            assert e <= R.SAME_PRODUCTS, (k, e)
    return outs


@pytest.mark.parametrize("i", range(len(R.SPLIT)), ids=_ids([("SPLIT", i) for i in range(len(R.SPLIT))]))
def test_split_training_call_vs_fp64_and_tap_group_kernel(vpx, parity_log, i):
    """x converted once, the forward from split input, the weight gradient per stride residue on wgrad2_kernel's glue form (k7 s2 and
    single-tap residues: launch_wgrad) — and with VPX_EXP_GLUE_WGRAD_TAPGROUP the fp32-operand tap-group weight gradient behind the plain
    forward. The same bf16x3 products both ways."""
    _ab(vpx, parity_log, "SPLIT", i, vpx._lib.Exp.GLUE_WGRAD_TAPGROUP)


@pytest.mark.parametrize("i", range(len(R.C16)), ids=_ids([("C16", i) for i in range(len(R.C16))]))
def test_c16_gate_vs_fp64_and_first_generation(vpx, parity_log, i):
    """conv16.hip behind a training call (VPX_EXP_NO_C16: the first generation on the same split input)."""
    _ab(vpx, parity_log, "C16", i, vpx._lib.Exp.NO_C16)


FROM_SPLIT = [("SPLIT", i) for i in range(len(R.SPLIT))] + [("C16", i) for i in range(len(R.C16))] + [("CONVQ_FWD", i) for i in R.CONVQ_FWD_PYTHON]


@pytest.mark.parametrize("table,i", FROM_SPLIT, ids=_ids(FROM_SPLIT))
def test_forward_from_split_input_vs_fp64(vpx, parity_log, table, i):
    """ops.conv2d_ex_from_split: y against fp64; the split output decodes bit for bit to split_convert(y); a second call, on the packed
    weights its workspace kept, is equal bit for bit; an in-place weight update is followed."""
    c, v = R.TABLES[table][i], R.variant(table, i)
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    t, ref, _ = R.case(table, i)
    x, w, b = t["x"].cuda(), t["w"].cuda(), (t["b"].cuda() if v["bias"] else None)
    assert vpx.ops.conv2d_ex_takes_split(N, H, W, Ci, Co, kh, kw, s, p, bool(tr))
    xbuf, _ = vpx.ops.split_convert(x)
    bar = R.BARS["bf16x3"][0]
    y, ybuf, shp = vpx.ops.conv2d_ex_from_split(xbuf, (N, Ci, H, W), w, b, s, p, bool(tr), v["slope"], "bf16x3", out_split=True)
    assert shp == tuple(ref["y"].shape)
    _hold(parity_log, "y", y, ref["y"], bar)
    sb, _ = vpx.ops.split_convert(y)
    assert torch.equal(sb.view(torch.int32), ybuf.view(torch.int32))
    y2, _, _ = vpx.ops.conv2d_ex_from_split(xbuf, (N, Ci, H, W), w, b, s, p, bool(tr), v["slope"], "bf16x3")
    assert torch.equal(y, y2)
    w.mul_(0.5)
    y3, _, _ = vpx.ops.conv2d_ex_from_split(xbuf, (N, Ci, H, W), w, b, s, p, bool(tr), v["slope"], "bf16x3")
    with torch.no_grad():
        ref3 = R.activate(R.conv(c, t["x"].double(), t["w"].double() * 0.5, None if t["b"] is None else t["b"].double()), v["slope"])
    _hold(parity_log, "y.after_update", y3, ref3, bar)


CONVQ_CTYPES = [("CONVQ_FWD", i) for i in range(len(R.CONVQ_FWD)) if i not in R.CONVQ_FWD_PYTHON]


@pytest.mark.parametrize("table,i", CONVQ_CTYPES, ids=_ids(CONVQ_CTYPES))
def test_convq_forward_with_output_padding_through_the_c_abi(vpx, parity_log, table, i):
    """vpx_conv2d_ex_fwd_from_split with an output padding in the descriptor (the Python wrapper passes none): convq's phase form on
    pr.H = (Ho + 1) / 2 phase rows, the last one ragged. The destination starts as NaN."""
    c, v = R.TABLES[table][i], R.variant(table, i)
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    t, ref, _ = R.case(table, i)
    L, ptr = vpx._lib.lib(), vpx._lib.ptr
    vpx.ops.sync_determinism()
    d = vpx._lib.ConvDesc(N, H, W, Ci, Co, kh, kw, s, p, tr, v["slope"], vpx._lib.PREC_BF16X3, oph, opw)
    assert L.vpx_conv2d_ex_takes_split(ctypes.byref(d)) == 2
    xbuf, _ = vpx.ops.split_convert(t["x"].cuda())
    w, b = t["w"].cuda(), (t["b"].cuda() if v["bias"] else None)
    Ho, Wo = R.out_shape(c)
    y = torch.empty(N, Ho, Wo, Co, device="cuda").fill_(float("nan"))
    ybuf = torch.empty(N * Ho * Wo * Co, device="cuda")
    nb = L.vpx_conv2d_ex_split_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), ptr(xbuf), 0, 0, 1, ptr(w), ptr(b), ptr(y), ptr(ybuf), 0, ptr(ws), nb, vpx.ops.stream())
    assert rc == 0, L.vpx_last_error().decode()
    got = y.permute(0, 3, 1, 2)
    assert not bool(torch.isnan(got).any())
    _hold(parity_log, "y", got, ref["y"], R.BARS["bf16x3"][0])
    sb, _ = vpx.ops.split_convert(got)
    assert torch.equal(sb.view(torch.int32), ybuf.view(torch.int32))


@pytest.mark.parametrize("i", range(len(R.CONVQ_BWD)), ids=_ids([("CONVQ_BWD", i) for i in range(len(R.CONVQ_BWD))]))
def test_data_gradient_on_convq_with_a_padded_adjoint_vs_fp64_and_first_generation(vpx, parity_log, i):
    """64 -> 16 stride-2 layers whose adjoint (16 -> 64, transposed) convq takes, with the output padding made from the rows / columns the
    forward dropped; VPX_EXP_GLUE_DGRAD_GEN1 keeps the first-generation data gradient."""
    _ab(vpx, parity_log, "CONVQ_BWD", i, vpx._lib.Exp.GLUE_DGRAD_GEN1)


@pytest.mark.parametrize("table,i", R.DETERMINISTIC, ids=_ids(R.DETERMINISTIC))
def test_deterministic_mode_gives_bit_equal_gradients(vpx, parity_log, table, i):
    ref = R.case(table, i)[1]
    a, b = _deterministic(vpx, lambda: (_run(vpx, table, i, "bf16x3"), _run(vpx, table, i, "bf16x3")))
    _hold_all(parity_log, a, ref, "bf16x3")
    for k, g, h in zip(("y", "dx", "dw", "db"), a, b):
        assert (g is None and h is None) or torch.equal(g, h), k


PARTIAL = [("CONVQ_BWD", 0), ("SPLIT", 1)]


@pytest.mark.parametrize("table,i", PARTIAL, ids=_ids(PARTIAL))
def test_backward_that_wants_dx_or_dw_alone_vs_fp64_and_the_full_call(vpx, parity_log, table, i):
    """The backward's workspace carve depends on what is wanted (csrc/glue_bwd_api.hip: the split copy of dy and the adjoint's convq pack
    for dx, the split copies of dy and x for dw). (x, w) requiring gradients as (1, 1), (1, 0) and (0, 1), on the layer whose data gradient
    runs on convq and on the one whose weight gradient alone reads split operands: every gradient a call produces holds the fp64 bars,
    and in deterministic mode equals the full call's bit for bit."""
    ref = R.case(table, i)[1]
    for need in ((True, True), (True, False), (False, True)):
        out = _run(vpx, table, i, "bf16x3", need=need)
        assert (out[1] is not None, out[2] is not None) == need
        fwd, grad = R.BARS["bf16x3"]
        _hold(parity_log, f"y.need{need[0]:d}{need[1]:d}", out[0], ref["y"], fwd)
        for k, g in zip(("dx", "dw", "db"), out[1:]):
            if g is not None:
                assert not bool(torch.isnan(g).any()), k
                _hold(parity_log, f"{k}.need{need[0]:d}{need[1]:d}", g, ref[k], grad)
    full, only_dx, only_dw = _deterministic(vpx, lambda: [_run(vpx, table, i, "bf16x3", need=n) for n in ((True, True), (True, False), (False, True))])
    assert torch.equal(only_dx[1], full[1]) and torch.equal(only_dw[2], full[2])
    for part in (only_dx, only_dw):
        assert (part[3] is None and full[3] is None) or torch.equal(part[3], full[3])
