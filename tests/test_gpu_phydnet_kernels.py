"""PhyDNet's own kernels (csrc/phydnet.hip through phy_ops) and the PhyCell block against fp64 on the CPU, on the same fp32 inputs, at
the shapes where they can go wrong: the 256-thread block edge, odd and non-square maps, several frames and channels through the
head's index transposition, even / non-square / 8-tap moment kernels, pair counts around the moment loss's 1024-thread loop.

Every comparison is max|got - ref| / max|ref| (parity.relmax's figure; `parity_log` is that measure with a name and its bar, so
every figure below lands in the parity record). The bars and where they come from:

  * forward values 1e-5 (BLOCK_TOL): the block-level bar of test_gpu_phydnet.py. The correction and the head are a handful of fp32
    operations per element (a few 6e-8 roundings, against 1e-5).
  * gradients 5e-5 (GRAD_TOL): the suite's gradient bar (test_gpu_phydnet.py, test_gpu_more.py).
  * the sigmoid head under saturation 1e-5 ABSOLUTE: the output's range is 1.
  * moment loss and its gradient 1e-6 relative (MOMENT_TOL), as in test_phydnet_moment_loss_vs_fp64: the kernel works in fp64 and
    rounds its results to fp32 once (6e-8), and takes the scale as an fp32 number (0.7f is 1.7e-8 off 0.7).
  * PhyCell block outputs 1e-5. Block gradients lie behind a GroupNorm, where the error is not derivable in advance: each bar is
    max(5e-5, 3 x the error of the fp32 run of tests/phydnet_ref.py against its own fp64 run on the same inputs), measured from the
    restatement alone before the library's result is read (as in test_gpu_unet3d.py), printed and recorded as `*.ref32` entries. A
    derived bar above 5e-4 (BAR_CAP) fails the case. Measured on the CPU for the seeds used here, worst fp32-restatement error per
    case: 8x14 k3 5x7 B1: 1.08e-5 on one host, 5.2e-6 on another (F.conv1.bias; torch's fp32 CPU convolution sums in a host-dependent
    order); 16x49 k7 6x10 B2, two cells: 6.7e-7 (cell 1 convgate.bias); 16x9 k3 8x8 a5 B2: 2.4e-6 (F.conv1.bias); 64x49 k7 16x16 B1:
    6.6e-7 (F.conv1.bias) -- three times the worst is 3.2e-5, so every derived bar is the 5e-5 floor, far under the cap.

Bit-equality is asked wherever two paths must run the same arithmetic: NCHW-contiguous against channels-last inputs (the wrapper
converts, the kernel is the same), a subset of the correction's gradients against the full call, dh against dFh, two calls of the
moment loss (one workgroup, fixed reduction order).

The moment loss at its optimum: w[o, b] = M0^-1 C_o M1^-T solved in fp64 and rounded to fp32 leaves D as pure rounding residue. Both
sides evaluate it in fp64 from the same fp32 numbers; the test first asserts on the CPU that the reference's two evaluation orders
(the einsum as written, the kernel's two matrix products) agree to 1e-7 relative there, in the loss and in the gradient, so the 1e-6
bar means something. They do for both shapes, so no perturbation of w is applied. Measured: 7x7: loss 1.1e-13, max|dW| 3.2e-8, the
orders 5.6e-12 (loss) and 4.2e-9 (gradient) apart. 3x3: the optimum's entries (0, +-1/2, 1, -2) and M's are exact in fp32 and every
product and sum is exact in fp64, so loss and gradient are exactly 0 in both orders, and the library must return exactly 0 too."""
import pytest
import torch

import phydnet_ref
from golden_util import name_seed, seeded_randn
from test_phydnet_host import phy_fill_

pytestmark = pytest.mark.gpu

BLOCK_TOL = 1e-5
GRAD_TOL = 5e-5
MOMENT_TOL = 1e-6
BAR_CAP = 5e-4
FORMATS = {"nchw": torch.contiguous_format, "nhwc": torch.channels_last}


def _hold(parity_log, name, got, ref, bar):
    """Records the figure, prints it, then asserts it."""
    err = parity_log("phyk." + name, got, ref, bar)
    print(f"phyk.{name}: {err:.3e} (bar {bar:.1e})")
    assert err < bar, (name, err, bar)
    return err


def _ids(case):
    return "x".join(map(str, case))


# ---- 1. PhyCell correction -------------------------------------------------------------------------------------------------------
CORRECT_SHAPES = [(1, 1, 1, 1), (1, 3, 5, 17), (1, 4, 8, 8), (1, 1, 257, 1), (2, 7, 5, 9), (2, 64, 16, 16)]
CORRECT_NAMES = ("dG", "dFh", "dh", "dE")


def _correct_inputs(shape, tag):
    """G, F(h), h, E and the cotangent (one value per element), fp32 on the CPU."""
    seed = name_seed(f"phyk.correct.{tag}.{shape}")
    return [seeded_randn(shape, seed + i, s) for i, s in enumerate((1.5, 0.5, 1.0, 1.0, 1.0))]


def _correct_fp64(G, Fh, h, E, dn):
    leaves = [t.double().requires_grad_(True) for t in (G, Fh, h, E)]
    g, fh, hh, e = leaves
    ht = hh + fh
    out = ht + torch.sigmoid(g) * (e - ht)
    out.backward(dn.double())
    return out.detach(), [t.grad for t in leaves]


def _correct_gpu(inputs, dn, layout, req=(True, True, True, True)):
    from vp_suite_amd import phy_ops
    fmt = FORMATS[layout]
    leaves = [t.cuda().contiguous(memory_format=fmt).requires_grad_(r) for t, r in zip(inputs, req)]
    out = phy_ops.phycell_correct(*leaves)
    assert tuple(out.shape) == tuple(inputs[0].shape)
    if any(req):
        out.backward(dn.cuda().contiguous(memory_format=fmt))
    return out.detach(), [t.grad for t in leaves]


def _correct_both_layouts(parity_log, tag, inputs, dn):
    """Runs both input layouts, holds each to fp64 and the two to each other bit for bit. Returns the channels-last result."""
    out64, g64 = _correct_fp64(*inputs, dn)
    runs = {}
    for layout in FORMATS:
        out, grads = _correct_gpu(inputs, dn, layout)
        assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads)
        _hold(parity_log, f"correct.{tag}.{layout}.fwd", out, out64, BLOCK_TOL)
        for name, g, r in zip(CORRECT_NAMES, grads, g64):
            assert g.shape == r.shape
            _hold(parity_log, f"correct.{tag}.{layout}.grad.{name}", g, r, GRAD_TOL)
        assert torch.equal(grads[1], grads[2]), "dh and dFh are the same number"
        runs[layout] = (out, grads)
    assert torch.equal(runs["nchw"][0], runs["nhwc"][0])
    for a, b in zip(runs["nchw"][1], runs["nhwc"][1]):
        assert torch.equal(a, b)
    return runs["nhwc"]


@pytest.mark.parametrize("shape", CORRECT_SHAPES, ids=_ids)
def test_phydnet_correct_vs_fp64(vpx, shape, parity_log):
    """n = 1, 255, 256, 257, 630 and the default latent: output and all four gradients, both input layouts."""
    *inputs, dn = _correct_inputs(shape, "plain")
    _correct_both_layouts(parity_log, _ids(shape), inputs, dn)


@pytest.mark.parametrize("req", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1)], ids=lambda r: "".join(map(str, r)))
def test_phydnet_correct_gradient_subsets(vpx, req):
    """The backward's outputs are optional one by one: a subset's gradients are the all-four call's, bit for bit."""
    *inputs, dn = _correct_inputs((2, 7, 5, 9), "subset")
    out_full, g_full = _correct_gpu(inputs, dn, "nhwc")
    out, grads = _correct_gpu(inputs, dn, "nhwc", req=tuple(bool(r) for r in req))
    assert torch.equal(out, out_full)
    for r, g, gf in zip(req, grads, g_full):
        if r:
            assert torch.equal(g, gf)
        else:
            assert g is None


@pytest.mark.parametrize("shape", [(2, 7, 5, 9), (2, 64, 16, 16)], ids=_ids)
def test_phydnet_correct_saturated_gates(vpx, shape, parity_log):
    """G = +-30, +-100 in a quarter of the elements: sigmoid is 0 or 1 in fp32 there; everything stays finite and inside the bars (dG
    max-normalised over the whole tensor: at a saturated element it is ~1e-13 of that scale in fp64 and 0 in fp32)."""
    *inputs, dn = _correct_inputs(shape, "saturated")
    G = inputs[0].reshape(-1)
    idx = torch.arange(0, G.numel(), 4)
    G[idx] = torch.tensor([30.0, -30.0, 100.0, -100.0])[(idx // 4) % 4]
    _correct_both_layouts(parity_log, "sat." + _ids(shape), inputs, dn)


@pytest.mark.parametrize("which", [3, 0], ids=["E", "G"])
def test_phydnet_correct_nan_stays_in_place(vpx, which):
    """A NaN in E or in G reaches exactly its own output elements."""
    shape = (2, 7, 5, 9)
    *inputs, dn = _correct_inputs(shape, "nan")
    mask = torch.zeros(shape, dtype=torch.bool)
    for pos in ((0, 0, 0, 0), (1, 3, 2, 8), (1, 6, 4, 8)):
        mask[pos] = True
    inputs[which][mask] = float("nan")
    for layout in FORMATS:
        with torch.no_grad():
            out, _ = _correct_gpu(inputs, dn, layout, req=(False,) * 4)
        assert torch.equal(torch.isnan(out).cpu(), mask), layout
        assert torch.isfinite(out.cpu()[~mask]).all()


# ---- 2. sigmoid head -------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 1, 4, 6), (2, 3, 16, 24)]     # (B, C, H, W)
HEAD_SLOTS = [(1, 0, 1), (4, 0, 1), (4, 3, 1), (5, 1, 3), (3, 0, 3)]         # (T, t0, nT)


def _head_logits(B, C, H, W, nT, tag):
    """[nT*B, C, H, W] frame-major, every element a value of its own (an even grid over [-4, 4] in a seeded order): any exchange of
    strides moves numbers."""
    n = nT * B * C * H * W
    order = seeded_randn((n,), name_seed(f"phyk.head.{tag}.{(B, C, H, W, nT)}")).argsort()
    x = torch.linspace(-4.0, 4.0, n)[order].reshape(nT * B, C, H, W).contiguous()
    assert x.unique().numel() == n
    return x


def _head_frames_fp64(t, nT):
    """[nT*B, C, H, W] -> [B, nT, C, H, W]."""
    NB, C, H, W = t.shape
    return t.view(nT, NB // nT, C, H, W).transpose(0, 1)


@pytest.mark.parametrize("slots", HEAD_SLOTS, ids=_ids)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=_ids)
def test_phydnet_head_writes_its_slots_only(vpx, shape, slots, parity_log):
    """The `out=` path under no_grad: frames t0 .. t0+nT-1 of a sentinel-filled [B, T, C, H, W] buffer take sigmoid(x), rearranged from
    x's [k][b][p][c] memory; every other slot keeps the sentinel; the returned view is that part of the buffer."""
    from vp_suite_amd import phy_ops
    (B, C, H, W), (T, t0, nT) = shape, slots
    x = _head_logits(B, C, H, W, nT, "direct")
    ref = _head_frames_fp64(torch.sigmoid(x.double()), nT)
    others = [t for t in range(T) if not t0 <= t < t0 + nT]
    results = []
    for layout, fmt in FORMATS.items():
        out = torch.full((B, T, C, H, W), 7.5, device="cuda")
        with torch.no_grad():
            ret = phy_ops.sigmoid_head(x.cuda().contiguous(memory_format=fmt), nT, out=out, t0=t0)
        want = out[:, t0:t0 + nT]
        assert ret.data_ptr() == want.data_ptr() and ret.shape == want.shape and ret.stride() == want.stride()
        assert ret.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()
        assert torch.equal(out[:, others], torch.full((B, len(others), C, H, W), 7.5, device="cuda")), layout
        _hold(parity_log, f"head.direct.{_ids(shape)}.{_ids(slots)}.{layout}", ret, ref, BLOCK_TOL)
        results.append(out.clone())
    assert torch.equal(results[0], results[1])


@pytest.mark.parametrize("nT", [1, 3])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=_ids)
def test_phydnet_head_differentiable_vs_fp64(vpx, shape, nT, parity_log):
    from vp_suite_amd import phy_ops
    B, C, H, W = shape
    x = _head_logits(B, C, H, W, nT, "grad")
    dout = seeded_randn((B, nT, C, H, W), name_seed(f"phyk.head.dout.{shape}.{nT}"))
    x64 = x.double().requires_grad_(True)
    ref = _head_frames_fp64(torch.sigmoid(x64), nT)
    ref.backward(dout.double())
    results = []
    for layout, fmt in FORMATS.items():
        xg = x.cuda().contiguous(memory_format=fmt).requires_grad_(True)
        out = phy_ops.sigmoid_head(xg, nT)
        assert tuple(out.shape) == (B, nT, C, H, W)
        _hold(parity_log, f"head.fn.{_ids(shape)}.nT{nT}.{layout}.fwd", out, ref.detach(), BLOCK_TOL)
        out.backward(dout.cuda())
        assert xg.grad.shape == xg.shape and xg.grad.is_contiguous(memory_format=fmt), (xg.grad.shape, xg.grad.stride())
        _hold(parity_log, f"head.fn.{_ids(shape)}.nT{nT}.{layout}.grad.dx", xg.grad, x64.grad, GRAD_TOL)
        results.append((out.detach(), xg.grad))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_phydnet_head_backward_into_later_slots(vpx, parity_log):
    """The backward at t0 > 0 (reachable over the C ABI only): `out` and `dout` are whole [B, T, C, H, W] buffers, the frames sit in slots
    t0 .. t0+nT-1, dx comes back in x's [k][b][p][c] memory."""
    from vp_suite_amd import _lib, ops, phy_ops
    B, T, t0, nT, C, H, W = 2, 5, 1, 3, 3, 5, 7
    x = _head_logits(B, C, H, W, nT, "abi")
    dout = seeded_randn((B, T, C, H, W), name_seed("phyk.head.abi.dout"))
    out = torch.full((B, T, C, H, W), 7.5, device="cuda")
    with torch.no_grad():
        phy_ops.sigmoid_head(x.cuda().contiguous(memory_format=torch.channels_last), nT, out=out, t0=t0)
    dout_g = dout.cuda()
    dx = ops.new_channels_last((nT * B, C, H, W), "cuda").fill_(7.5)
    _lib.check(_lib.lib().vpx_sigmoid_head_bwd(_lib.ptr(out), _lib.ptr(dout_g), _lib.ptr(dx), B, T, t0, nT, C, H, W, ops.stream()),
               "vpx_sigmoid_head_bwd")
    y = _head_frames_fp64(torch.sigmoid(x.double()), nT)                    # [B, nT, C, H, W]
    ref = (dout[:, t0:t0 + nT].double() * y * (1.0 - y)).transpose(0, 1).reshape(nT * B, C, H, W)
    _hold(parity_log, "head.abi.t0.grad.dx", dx, ref, GRAD_TOL)


def test_phydnet_head_saturation_and_nan(vpx, parity_log):
    """Logits +-20, +-89 (exp overflows fp32 at 88.7), +-100 and NaN at fixed places among ordinary ones: a NaN logit gives a NaN output and a
    NaN gradient in its own element only; everything else is finite, in [0, 1], within 1e-5 absolute of fp64 (gradients GRAD_TOL)."""
    from vp_suite_amd import phy_ops
    B, C, H, W, nT = 2, 3, 5, 7, 3
    x = _head_logits(B, C, H, W, nT, "saturated")
    flat = x.view(-1)
    places = torch.tensor([0, 5, 37, 101, 200, 333, 417, flat.numel() - 1])
    flat[places] = torch.tensor([20.0, -20.0, 89.0, -89.0, 100.0, -100.0, float("nan"), float("nan")])
    dout = seeded_randn((B, nT, C, H, W), name_seed("phyk.head.saturated.dout"))
    x64 = x.double().requires_grad_(True)
    ref = _head_frames_fp64(torch.sigmoid(x64), nT)
    ref.backward(dout.double())
    ref = ref.detach()
    nan_out, nan_x = torch.isnan(ref), torch.isnan(x)
    assert int(nan_out.sum()) == 2 and torch.equal(torch.isnan(x64.grad), nan_x)
    for layout, fmt in FORMATS.items():
        xg = x.cuda().contiguous(memory_format=fmt).requires_grad_(True)
        out = phy_ops.sigmoid_head(xg, nT)
        out.backward(dout.cuda())
        got, dx = out.detach().cpu(), xg.grad.cpu()
        assert torch.equal(torch.isnan(got), nan_out) and torch.equal(torch.isnan(dx), nan_x), layout
        assert torch.isfinite(got[~nan_out]).all() and torch.isfinite(dx[~nan_x]).all()
        assert float(got[~nan_out].min()) >= 0.0 and float(got[~nan_out].max()) <= 1.0
        err = parity_log(f"phyk.head.saturated.{layout}.fwd", got[~nan_out], ref[~nan_out], BLOCK_TOL)
        absolute = float((got[~nan_out].double() - ref[~nan_out]).abs().max())
        print(f"phyk.head.saturated.{layout}.fwd: {absolute:.3e} absolute, {err:.3e} max-normalised (bar 1e-5 absolute)")
        assert absolute < 1e-5
        _hold(parity_log, f"head.saturated.{layout}.grad.dx", dx[~nan_x], x64.grad[~nan_x], GRAD_TOL)


# ---- 3. moment loss --------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1, 1, 1), (6, 2, 2, 3), (12, 3, 4, 3), (5, 3, 3, 3), (20, 2, 3, 3), (64, 1, 8, 8), (32, 32, 3, 3), (41, 25, 3, 3),
                 (7, 3, 5, 7)]                                               # (hidden, Cin, kh, kw)
MOMENT_SCALE = 0.7


def _moment_reference(W, scale, factor):
    """fp64 loss and d(factor * loss)/dW of the fp32 filter bank W."""
    W64 = W.double().requires_grad_(True)
    ref = phydnet_ref._moment_loss_fp64(W64, scale)
    (ref * factor).backward()
    return ref.detach(), W64.grad


def _hold_moment(parity_log, tag, loss, grad, ref, gref):
    assert loss.dim() == 0 and loss.dtype == torch.float32 and torch.isfinite(loss) and torch.isfinite(grad).all()
    assert grad.shape == gref.shape
    _hold(parity_log, f"moment.{tag}.loss", loss.detach().reshape(1), ref.reshape(1), MOMENT_TOL)
    _hold(parity_log, f"moment.{tag}.grad.dW", grad, gref, MOMENT_TOL)


@pytest.mark.parametrize("factor", [1.0, -2.5], ids=["unit", "scaled"])
@pytest.mark.parametrize("shape", MOMENT_SHAPES, ids=_ids)
def test_phydnet_moment_loss_edge_shapes_vs_fp64(vpx, shape, factor, parity_log):
    """Non-square, even, 1x1 and 8-tap kernels, hidden below / at / above kh*kw, 1 / 1024 / 1025 (o, b) pairs. `scaled` multiplies the loss by
    -2.5 inside the graph, so the backward kernel reads an incoming gradient other than 1 from device memory."""
    from vp_suite_amd import phy_ops
    W = seeded_randn(shape, name_seed(f"phyk.moment.{shape}"), 0.3)
    ref, gref = _moment_reference(W, MOMENT_SCALE, factor)
    Wg = W.cuda().requires_grad_(True)
    loss = phy_ops.moment_loss(Wg, MOMENT_SCALE)
    (loss if factor == 1.0 else loss * factor).backward()
    _hold_moment(parity_log, f"{_ids(shape)}.{factor}", loss, Wg.grad, ref, gref)


@pytest.mark.parametrize("shape", [(6, 2, 2, 3), (41, 25, 3, 3), (7, 3, 5, 7)], ids=_ids)
def test_phydnet_moment_loss_non_contiguous_filter_bank(vpx, shape, parity_log):
    """W handed over as a view: the parameter is stored [Cin, hidden, kw, kh] and permuted back."""
    from vp_suite_amd import phy_ops
    W = seeded_randn(shape, name_seed(f"phyk.moment.view.{shape}"), 0.3)
    ref, gref = _moment_reference(W, MOMENT_SCALE, 1.0)
    stored = W.permute(1, 0, 3, 2).contiguous().cuda().requires_grad_(True)
    view = stored.permute(1, 0, 3, 2)
    assert tuple(view.shape) == shape and not view.is_contiguous()
    loss = phy_ops.moment_loss(view, MOMENT_SCALE)
    loss.backward()
    _hold_moment(parity_log, f"view.{_ids(shape)}", loss, stored.grad.permute(1, 0, 3, 2), ref, gref)


@pytest.mark.parametrize("shape", [(9, 4, 3, 3), (49, 2, 7, 7)], ids=_ids)
def test_phydnet_moment_loss_at_its_optimum(vpx, shape, parity_log):
    """D ~ 0 by cancellation (module docstring). No perturbation of w is applied: the reference's two evaluation orders agree to 1e-7 here,
    which the test asserts first."""
    from vp_suite_amd import phy_ops
    W = phydnet_ref.moment_optimum(*shape).float()
    ref, gref = _moment_reference(W, MOMENT_SCALE, 1.0)
    W64 = W.double().requires_grad_(True)
    ref2 = phydnet_ref.moment_loss_fp64_two_products(W64, MOMENT_SCALE)
    ref2.backward()
    assert 0.0 <= float(ref) < 1e-10, float(ref)
    order_loss, order_grad = abs(float(ref2.detach()) - float(ref)), float((W64.grad - gref).abs().max())
    print(f"phyk.moment.optimum.{_ids(shape)}: loss {float(ref):.3e}, max|dW| {float(gref.abs().max()):.3e}; the two fp64 orders differ by "
          f"{order_loss:.2e} (loss), {order_grad:.2e} (gradient), absolute")
    assert order_loss <= 1e-7 * float(ref) and order_grad <= 1e-7 * float(gref.abs().max())
    Wg = W.cuda().requires_grad_(True)
    loss = phy_ops.moment_loss(Wg, MOMENT_SCALE)
    loss.backward()
    _hold_moment(parity_log, f"optimum.{_ids(shape)}", loss, Wg.grad, ref, gref)


def test_phydnet_moment_loss_is_bit_reproducible(vpx):
    from vp_suite_amd import phy_ops
    shape = (41, 25, 3, 3)
    W = seeded_randn(shape, name_seed(f"phyk.moment.repeat.{shape}"), 0.3)
    runs = []
    for _ in range(2):
        Wg = W.cuda().requires_grad_(True)
        loss = phy_ops.moment_loss(Wg, MOMENT_SCALE)
        loss.backward()
        runs.append((loss.detach().clone(), Wg.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_phydnet_moment_loss_refuses_nine_taps(vpx):
    from vp_suite_amd import phy_ops
    with pytest.raises(ValueError):
        phy_ops.moment_loss(torch.zeros(4, 2, 9, 3, device="cuda"))
    with pytest.raises(ValueError):
        phy_ops.moment_loss(torch.zeros(4, 2, 3, 9, device="cuda"))


# ---- 4. PhyCell block against the fp64 restatement -------------------------------------------------------------------------------
# (input_dim, hidden, k, H, W, action_size, B, n_layers)
BLOCK_CASES = [(8, 14, 3, 5, 7, 0, 1, 1), (16, 49, 7, 6, 10, 0, 2, 2), (16, 9, 3, 8, 8, 5, 2, 1), (64, 49, 7, 16, 16, 0, 1, 1)]
BLOCK_STEPS = 3


def _block_inputs(case):
    idim, hid, k, H, W, asz, B, L = case
    tag = f"phyk.block.{case}"
    frames = seeded_randn((B, BLOCK_STEPS, idim, H, W), name_seed(tag + ".frames"))
    actions = seeded_randn((B, BLOCK_STEPS, max(asz, 1)), name_seed(tag + ".actions"))[:, :, :asz]
    cots = [seeded_randn((B, idim, H, W), name_seed(f"{tag}.g{t}")) for t in range(BLOCK_STEPS)]
    return frames, actions, cots


def _block_module(case, device):
    from vp_suite_amd.model_blocks import PhyCell
    idim, hid, k, H, W, asz, B, L = case
    blk = PhyCell((H, W), idim, [hid] * L, L, (k, k), asz > 0, asz, device)
    return phy_fill_(blk, name_seed(f"phyk.block.{case}"))


def block_restatement(case, dtype):
    """tests/phydnet_ref.py on the CPU in `dtype`, on the fp32 inputs: {"out{t}", "dframes", "dactions", "grad.<parameter>"}."""
    idim, hid, k, H, W, asz, B, L = case
    frames, actions, cots = _block_inputs(case)
    blk = _block_module(case, "cpu")
    sd = {key: v.detach().to(dtype).requires_grad_(True) for key, v in blk.state_dict().items()}
    fr = frames.to(dtype).requires_grad_(True)
    ac = actions.to(dtype).requires_grad_(asz > 0)
    outs, _ = phydnet_ref.phycell_stack(sd, L, fr, ac)
    sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots)).backward()
    res = {f"out{t}": o.detach() for t, o in enumerate(outs)}
    res["dframes"] = fr.grad
    if asz:
        res["dactions"] = ac.grad
    res.update({"grad." + key: sd[key].grad for key, _ in blk.named_parameters()})
    return res


def block_bars(r32, r64):
    """{name: (bar, the fp32 restatement's error)} for every gradient: max(GRAD_TOL, 3 x that error)."""
    bars = {}
    for key, ref in r64.items():
        if not key.startswith("out"):
            err = float((r32[key].double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
            bars[key] = (max(GRAD_TOL, 3.0 * err), err)
    return bars


@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids)
def test_phydnet_block_vs_fp64_restatement(vpx, case, parity_log):
    """PhyCell at f32, three steps from first_timestep=True, a cotangent of its own on every step's output: H != W, odd maps, B = 1, k = 3,
    a second stacked cell, five actions, the default latent. Outputs to 1e-5; frame / action / parameter gradients to bars measured
    from the restatement alone (module docstring)."""
    idim, hid, k, H, W, asz, B, L = case
    r64 = block_restatement(case, torch.float64)
    r32 = block_restatement(case, torch.float32)
    bars = block_bars(r32, r64)
    tag = "block." + _ids(case)
    for key, (bar, err) in bars.items():
        parity_log(f"phyk.{tag}.ref32.{key}", r32[key], r64[key], None)
    worst = max(bars, key=lambda key: bars[key][1])
    print(f"phyk.{tag}: fp32 restatement against fp64, worst {bars[worst][1]:.3e} ({worst}); largest bar {max(b for b, _ in bars.values()):.2e}")
    assert all(bar <= BAR_CAP for bar, _ in bars.values()), {key: b for key, b in bars.items() if b[0] > BAR_CAP}
    # only now the library
    frames, actions, cots = _block_inputs(case)
    blk = _block_module(case, "cuda").cuda()
    fr = frames.cuda().requires_grad_(True)
    ac = actions.cuda().requires_grad_(asz > 0)
    loss = 0.0
    for t in range(BLOCK_STEPS):
        Hs, out = blk(fr[:, t], ac[:, t], first_timestep=(t == 0))
        assert len(Hs) == L and tuple(out[-1].shape) == (B, idim, H, W)
        _hold(parity_log, f"{tag}.out{t}", out[-1], r64[f"out{t}"], BLOCK_TOL)
        loss = loss + (out[-1] * cots[t].cuda()).sum()
    loss.backward()
    got = {"dframes": fr.grad}
    if asz:
        got["dactions"] = ac.grad
    got.update({"grad." + key: p.grad for key, p in blk.named_parameters()})
    assert sorted(got) == sorted(bars)
    for key, (bar, _) in bars.items():
        assert got[key] is not None and got[key].shape == r64[key].shape, key
        _hold(parity_log, f"{tag}.{key}", got[key], r64[key], bar)
