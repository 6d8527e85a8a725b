"""PhyDNet ("phy") on the GPU: the GroupNorm kernel against torch, the moment loss against its fp64 formula, the PhyCell block and the
tiny / action-conditional / default models against the reference's fixtures (tools/gen_golden.py gen_phydnet), and a training
iteration through the model's own train_iter.

Bounds: forward values max|Δ|/max|ref| < 1e-4 (the north-star bar; the block and the GroupNorm comparisons hold 1e-5), gradients
5e-5 as in the existing block gradient tests (test_gpu_more.py phy_ssc). The model's gradient summaries (per-tensor sum, sum of squares,
the elements kept: all of a small tensor, a strided slice of a large one) are held to the same 5e-5, the sum measured against the
tensor's L1 norm; bf16x3 gradients of the whole model are held relative to a same-sized forward perturbation of the f32 model
(see PERTURB), every figure recorded in the parity log."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import checksum, load_golden, name_seed, seeded_rand, seeded_randn
from parity import relmax as _relmax
from phydnet_ref import _moment_loss_fp64
from test_phydnet_host import (PHY_CELL_CASES, PHY_DEFAULT_B, PHY_DEFAULT_CTX, PHY_DEFAULT_KW, PHY_DEFAULT_PRED,
                               PHY_TINY_AC_KW, PHY_TINY_B, PHY_TINY_CTX, PHY_TINY_KW, PHY_TINY_PRED, PHY_TRAIN_CTX, PHY_TRAIN_PRED,
                               grad_kept, phy_fill_)

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
GRAD_TOL = 5e-5
# bf16x3 gradients of the whole model. Every layer PhyDNet runs holds the existing per-layer bound in bf16x3 (5e-5 against fp64:
# test_phydnet_layers_vs_fp64, measured <= 1e-5), and the forward of the model holds the 1e-4 bar (measured 5e-5). Its training
# gradients, though, are ill-conditioned with respect to the forward: the same f32 model with every weight multiplied by
# (1 + PERTURB * randn) -- a perturbation that moves the forward by as much as bf16x3 does (measured 8e-5 against bf16x3's 5e-5) --
# moves the parameter gradients by 2.2e-2 / 1.9e-2 of their maximum (teacher forcing off / on), where bf16x3 moves them by
# 2.5e-2 / 6e-3 (f32 unperturbed: < 1e-5). So bf16x3 gradients are held to BF16X3_VS_PERTURBED times what that perturbation does to
# the f32 gradients, measured in the same test (the bound of every bf16x3 entry in the parity log). A precision defect in a bf16x3
# path (plain-bf16 products: relative 4e-3 per product, ~1000x the perturbation) lands far above it.
PERTURB = 5e-6
BF16X3_VS_PERTURBED = 2.0


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
GN_CASES = [(4, 32, 32, 32, 16), (4, 64, 16, 16, 16), (3, 49, 16, 16, 7), (3, 6, 5, 7, 3)]   # (N, C, H, W, G)


def _gn_torch(x, G, w, b, slope, r):
    y = F.group_norm(x, G, w, b, eps=1e-5)
    if slope is not None:
        y = F.leaky_relu(y, slope)
    return y if r is None else y + r


@pytest.mark.parametrize("variant", ["plain", "leaky", "leaky_residual"])
@pytest.mark.parametrize("shape", GN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_phydnet_groupnorm_vs_torch(vpx, shape, variant):
    from vp_suite_amd import phy_ops
    N, C, H, W, G = shape
    seed = name_seed(f"gn.{shape}.{variant}")
    x = seeded_randn((N, C, H, W), seed).cuda() * 2.0 + 0.5
    w = (1.0 + 0.3 * seeded_randn((C,), seed + 1)).cuda()
    b = (0.3 * seeded_randn((C,), seed + 2)).cuda()
    r = seeded_randn((N, C, H, W), seed + 3).cuda() if variant == "leaky_residual" else None
    dy = seeded_randn((N, C, H, W), seed + 4).cuda()
    slope = None if variant == "plain" else 0.2
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)] + ([r.clone().requires_grad_(True)] if r is not None else [None])
    y = phy_ops.group_norm(leaves[0].contiguous(memory_format=torch.channels_last), G, leaves[1], leaves[2], leaky_slope=slope,
                           residual=leaves[3])
    ref_leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, b, r)]
    y_ref = _gn_torch(ref_leaves[0], G, ref_leaves[1], ref_leaves[2], slope, ref_leaves[3])
    assert _relmax(y, y_ref) < 1e-5
    y.backward(dy)
    y_ref.backward(dy)
    for got, ref in zip(leaves, ref_leaves):
        if got is not None:
            assert _relmax(got.grad, ref.grad) < GRAD_TOL


def test_phydnet_groupnorm_param_grads_bit_reproducible(vpx):
    from vp_suite_amd import phy_ops
    N, C, H, W, G = 64, 64, 16, 16, 16
    x = seeded_randn((N, C, H, W), 11).cuda().contiguous(memory_format=torch.channels_last)
    dy = seeded_randn((N, C, H, W), 12).cuda()
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            w = torch.ones(C, device="cuda", requires_grad=True)
            b = torch.zeros(C, device="cuda", requires_grad=True)
            phy_ops.group_norm(x, G, w, b, leaky_slope=0.2).backward(dy)
            runs.append((w.grad.clone(), b.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(prev)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_phydnet_ops_check_every_tensor(vpx):
    """weight, bias, residual and the caller's result buffer are checked like the input: device first, then dtype."""
    from vp_suite_amd import phy_ops
    from vp_suite_amd._lib import VpxError
    x = torch.rand(2, 32, 4, 4, device="cuda")
    w, b = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    with pytest.raises(VpxError):
        phy_ops.group_norm(x, 16, w.cpu(), b)
    with pytest.raises(ValueError):
        phy_ops.group_norm(x, 16, w, b, residual=x.double())
    logits = torch.rand(2, 1, 8, 8, device="cuda")
    with torch.no_grad():
        with pytest.raises(VpxError):
            phy_ops.sigmoid_head(logits, 1, out=torch.empty(2, 3, 1, 8, 8), t0=0)
        with pytest.raises(ValueError):
            phy_ops.sigmoid_head(logits, 1, out=torch.empty(2, 3, 1, 8, 8, device="cuda", dtype=torch.float64), t0=0)


# ---- moment loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(49, 64, 7, 7), (49, 16, 7, 7), (9, 5, 3, 3)])
def test_phydnet_moment_loss_vs_fp64(vpx, shape):
    from vp_suite_amd import phy_ops
    W = seeded_randn(shape, name_seed(f"moment.{shape}"), 0.05)
    Wg = W.cuda().requires_grad_(True)
    loss = phy_ops.moment_loss(Wg, 0.7)
    W64 = W.double().requires_grad_(True)
    ref = _moment_loss_fp64(W64, 0.7)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    (loss * 1.5).backward()
    assert _relmax(Wg.grad, W64.grad.float() * 1.5) < 1e-6


# ---- every convolution / ConvLSTM layer PhyDNet runs, both operand modes, against fp64 ------------------------------------------
# (name, N, H, W, Ci, Co, k, stride, pad, transposed, output_padding) at the tiny (32x32) and default (64x64) model's shapes
PHY_LAYERS = [("E.c1", 2, 32, 32, 1, 32, 3, 2, 1, 0, 0), ("E.c1_64", 2, 64, 64, 1, 32, 3, 2, 1, 0, 0), ("E.c1_rgb", 2, 64, 64, 3, 32, 3, 2, 1, 0, 0),
              ("E.c2", 16, 32, 32, 32, 32, 3, 1, 1, 0, 0), ("E.c3", 2, 32, 32, 32, 64, 3, 2, 1, 0, 0),
              ("split", 2, 16, 16, 64, 64, 3, 1, 1, 0, 0), ("splitT", 2, 16, 16, 64, 64, 3, 1, 1, 1, 0),
              ("D.upc1", 2, 16, 16, 64, 32, 3, 2, 1, 1, 1), ("D.upc2", 2, 32, 32, 32, 32, 3, 1, 1, 1, 0),
              ("D.upc3", 2, 32, 32, 32, 1, 3, 2, 1, 1, 1), ("D.upc3_rgb", 2, 32, 32, 32, 3, 3, 2, 1, 1, 1),
              ("F.conv1", 16, 16, 16, 64, 49, 7, 1, 3, 0, 0), ("F.conv2", 2, 16, 16, 49, 64, 1, 1, 0, 0, 0),
              ("convgate", 2, 16, 16, 128, 64, 3, 1, 1, 0, 0), ("action_1x1", 2, 16, 16, 67, 64, 1, 1, 0, 0, 0)]
PHY_CELLS = [(64, 16, 8, 2), (16, 64, 8, 2), (64, 128, 16, 16), (128, 64, 16, 2), (67, 128, 16, 2)]   # (Cin, Ch, H=W, B)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("layer", PHY_LAYERS, ids=lambda l: l[0])
def test_phydnet_layers_vs_fp64(vpx, layer, precision):
    from vp_suite_amd import ops
    name, N, H, W, Ci, Co, k, s, p, tr, op = layer
    seed = name_seed(f"phydnet.layer.{name}")
    x = seeded_randn((N, Ci, H, W), seed)
    w = seeded_randn(((Ci, Co) if tr else (Co, Ci)) + (k, k), seed + 1, 1.0 / (Ci * k * k) ** 0.5)
    b = seeded_randn((Co,), seed + 2, 0.1)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv_transpose2d(x64, w64, b64, s, p, op) if tr else F.conv2d(x64, w64, b64, s, p)
    dy = seeded_randn(tuple(y64.shape), seed + 3)
    y64.backward(dy.double())
    xs, ws, bs = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = ops.conv2d_ex(xs, ws, bs, s, p, transposed=bool(tr), precision=precision, output_padding=(op, op))
    y.backward(dy.cuda())
    for got, ref in ((y, y64), (xs.grad, x64.grad), (ws.grad, w64.grad), (bs.grad, b64.grad)):
        assert _relmax(got, ref.detach()) < GRAD_TOL


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape", PHY_CELLS, ids=lambda c: "x".join(map(str, c)))
def test_phydnet_convlstm_cells_vs_fp64(vpx, shape, precision):
    """One ConvLSTMCell step (gate order i,f,o,g) at the widths of PhyDNet's ConvLSTM stack, all gradients, against fp64 autograd."""
    from vp_suite_amd.model_blocks.conv_lstm_ndrplz import ConvLSTMCell
    cin, ch, H, B = shape
    seed = name_seed(f"phydnet.cell.{shape}")
    W = seeded_randn((4 * ch, cin + ch, 3, 3), seed, 1.0 / (9 * (cin + ch)) ** 0.5)
    bias = seeded_randn((4 * ch,), seed + 1, 0.1)
    x, h, c = (seeded_randn((B, n, H, H), seed + 2 + i, 1.0 if i == 0 else 0.5) for i, n in enumerate((cin, ch, ch)))
    gh, gc = seeded_randn((B, ch, H, H), seed + 5), seeded_randn((B, ch, H, H), seed + 6)
    W64, b64, x64, h64, c64 = (t.double().requires_grad_(True) for t in (W, bias, x, h, c))
    i_, f_, o_, g_ = torch.split(F.conv2d(torch.cat([x64, h64], 1), W64, b64, padding=1), ch, 1)
    c_ref = torch.sigmoid(f_) * c64 + torch.sigmoid(i_) * torch.tanh(g_)
    h_ref = torch.sigmoid(o_) * torch.tanh(c_ref)
    ((h_ref * gh.double()).sum() + (c_ref * gc.double()).sum()).backward()
    cell = ConvLSTMCell(cin, ch, (3, 3), True).cuda()
    cell.precision = precision
    with torch.no_grad():
        cell.conv.weight.copy_(W)
        cell.conv.bias.copy_(bias)
    xs, hs, cs = (t.cuda().requires_grad_(True) for t in (x, h, c))
    h_new, c_new = cell(xs, (hs, cs))
    ((h_new * gh.cuda()).sum() + (c_new * gc.cuda()).sum()).backward()
    for got, ref in ((h_new, h_ref), (c_new, c_ref), (xs.grad, x64.grad), (hs.grad, h64.grad), (cs.grad, c64.grad),
                     (cell.conv.weight.grad, W64.grad), (cell.conv.bias.grad, b64.grad)):
        assert _relmax(got, ref.detach()) < GRAD_TOL


# ---- PhyCell block --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(PHY_CELL_CASES))
def test_phydnet_cell_vs_golden(vpx, tag):
    from vp_suite_amd.model_blocks import PhyCell
    idim, hid, k, H, W, asz, B, steps = PHY_CELL_CASES[tag]
    g = load_golden(f"phydnet_cell_{tag}")
    blk = PhyCell((H, W), idim, [hid], 1, (k, k), asz > 0, asz, "cuda")
    phy_fill_(blk, name_seed("phydnet_cell." + tag))
    blk = blk.cuda()
    frames = seeded_randn((B, steps, idim, H, W), name_seed(f"phydnet_cell.{tag}.frames")).cuda().requires_grad_(True)
    actions = seeded_randn((B, steps, max(asz, 1)), name_seed(f"phydnet_cell.{tag}.actions"))[:, :, :asz].cuda()
    loss = 0.0
    for t in range(steps):
        Hs, out = blk(frames[:, t], actions[:, t], first_timestep=(t == 0))
        assert _relmax(out[-1], g[f"out{t}"]) < 1e-5, t
        loss = loss + (out[-1] * seeded_randn(out[-1].shape, name_seed(f"phydnet_cell.{tag}.g{t}")).cuda()).sum()
    assert _relmax(Hs[0], g["H0"]) < 1e-5
    loss.backward()
    assert _relmax(frames.grad, g["dframes"]) < GRAD_TOL
    for key, prm in blk.named_parameters():
        assert _relmax(prm.grad, g["grad." + key]) < GRAD_TOL, key


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _model(kw, tag, precision):
    from vp_suite_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES["phy"]("cuda", cell_precision=precision, **kw)
    phy_fill_(m, name_seed(f"phydnet.{tag}"))
    return m.cuda()


def _check_grad_summaries(m, g, k, parity_log, tol):
    """Per parameter: the sum (error relative to the tensor's L1 norm: a sum that cancels keeps only the rounding of its terms), the sum of
    squares, and the kept elements (all of a small tensor, a strided slice of a large one) with max|Δ| / max|ref| over the whole tensor.
    Every parameter is checked and recorded before the assertion, which names all that miss the bound."""
    bad = []
    for name, p in m.named_parameters():
        a = p.grad.detach().double().cpu().numpy().reshape(-1)
        l1 = float(np.abs(a).sum())
        gs, gq, gmax = (float(g[f"{k}.{s}.{name}"]) for s in ("gsum", "gsq", "gmax"))
        errs = (parity_log(f"{k}.gsum.{name}", np.array([a.sum(), l1]), np.array([gs, l1]), tol),    # = |Δ sum| / L1
                parity_log(f"{k}.gsq.{name}", np.array([(a * a).sum()]), np.array([gq]), 2 * tol),
                parity_log(f"{k}.grad.{name}", np.append(grad_kept(a), gmax), np.append(g[f"{k}.gkept.{name}"], gmax), tol))
        if errs[0] >= tol or errs[1] >= 2 * tol or errs[2] >= tol:
            bad.append((name, errs))
    assert not bad, bad


def _elem_grad_error(m, g, k):
    """max over parameters of max|Δ| / max|ref| over the kept elements of the gradient (the fixture's primary gradient figure)."""
    worst = 0.0
    for name, p in m.named_parameters():
        a = grad_kept(p.grad.detach().double().cpu().numpy().reshape(-1))
        worst = max(worst, float(np.abs(a - g[f"{k}.gkept.{name}"]).max()) / float(g[f"{k}.gmax.{name}"]))
    return worst


def _train_step(m, xt, tkw, lp, tf):
    m.zero_grad()
    out, ml = m(xt, pred_frames=PHY_TRAIN_PRED, train=True, teacher_forcing=tf, **tkw)
    moment = ml["moment regularization loss"]
    _, total = lp.get_losses(out, xt[:, 1:])
    total = total + moment
    total.backward()
    return out, moment, total


def _perturbed_f32(kw, tag):
    m = _model(kw, tag, "f32")
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.mul_(1.0 + PERTURB * seeded_randn(p.shape, name_seed(f"phydnet.perturb.{name}")).cuda())
    return m


def _run_model_case(kw, tag, precision, parity_log, ac):
    from vp_suite_amd.measure import PredictionLossProvider
    g = load_golden(f"phydnet_{tag}")
    m = _model(kw, tag, precision)
    c, h, w = kw["img_shape"]
    a = kw["action_size"] if ac else 0
    x = seeded_rand((PHY_TINY_B, PHY_TINY_CTX, c, h, w), name_seed(f"phydnet.{tag}.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9 * max(1.0, abs(float(g["chk_x"])))
    fkw = {}
    if a:
        fkw["actions"] = seeded_randn((PHY_TINY_B, PHY_TINY_CTX + PHY_TINY_PRED - 1, a), name_seed(f"phydnet.{tag}.actions")).cuda()
    with torch.no_grad():
        pred, ml = m(x.cuda(), pred_frames=PHY_TINY_PRED, **fkw)
        assert ml is None and pred.shape == (PHY_TINY_B, PHY_TINY_PRED, c, h, w)
        assert _relmax(pred, g["eval"]) < FWD_TOL
        if not a:
            assert _relmax(m.pred_1(x.cuda()), g["pred1"]) < FWD_TOL
    xt = seeded_rand((PHY_TINY_B, PHY_TRAIN_CTX + PHY_TRAIN_PRED, c, h, w), name_seed(f"phydnet.{tag}.xt")).cuda()
    tkw = {}
    if a:
        tkw["actions"] = seeded_randn((PHY_TINY_B, PHY_TRAIN_CTX + PHY_TRAIN_PRED - 1, a), name_seed(f"phydnet.{tag}.actions_t")).cuda()
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    for tf in ((False, True) if not a else (False,)):
        k = f"tf{int(tf)}"
        out, moment, total = _train_step(m, xt, tkw, lp, tf)
        fwd_err = _relmax(out, g[f"{k}.frames"])
        assert fwd_err < FWD_TOL
        assert abs(moment.item() - float(g[f"{k}.moment"])) <= 1e-5 * abs(float(g[f"{k}.moment"]))
        assert abs(total.item() - float(g[f"{k}.total"])) <= FWD_TOL * abs(float(g[f"{k}.total"]))
        if precision == "f32":
            _check_grad_summaries(m, g, k, parity_log, GRAD_TOL)
            continue
        # bf16x3: against the same f32 model under a forward perturbation of the same size (see PERTURB)
        mp = _perturbed_f32(kw, tag)
        out_p, _, _ = _train_step(mp, xt, tkw, lp, tf)
        fwd_err_p = parity_log(f"{k}.perturbed_f32.frames", out_p, g[f"{k}.frames"], None)
        assert fwd_err <= 2.0 * fwd_err_p, (fwd_err, fwd_err_p)          # the perturbation is at least as large as bf16x3's
        tol = BF16X3_VS_PERTURBED * _elem_grad_error(mp, g, k)
        _check_grad_summaries(m, g, k, parity_log, tol)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_phydnet_tiny_model_vs_golden(vpx, precision, parity_log):
    _run_model_case(PHY_TINY_KW, "tiny", precision, parity_log, ac=False)


def test_phydnet_tiny_action_conditional_vs_golden(vpx, parity_log):
    _run_model_case(PHY_TINY_AC_KW, "tiny_ac", "f32", parity_log, ac=True)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_phydnet_default_model_vs_golden(vpx, precision):
    """The default model's prediction against the golden's strided slice (FWD_TOL) and its checksum over all 40 960 elements.
    Measured, 8 fresh models per operand mode and library build in one process, MI355X: no two predictions are bit-equal (the small-map
    convolutions add their K-split partial sums with atomics). f32: slice 2.9e-6 .. 4.0e-6, checksum error 5e-6 .. 9.9e-5 against its
    bound of 1.05e-3. bf16x3: slice 3.1e-5 .. 4.5e-5, checksum error 3.5e-4 .. 1.31e-3 — the bound lies INSIDE that spread (4 of 16 runs
    above it), so the bf16x3 case fails now and then with unchanged kernels. The bound stays as it is; the prediction needs to become
    reproducible (or more exact in bf16x3) for this case to hold on every run."""
    g = load_golden("phydnet_default")
    m = _model(PHY_DEFAULT_KW, "default", precision)
    assert sum(p.numel() for p in m.parameters()) == int(g["n_params"])
    x = seeded_rand((PHY_DEFAULT_B, PHY_DEFAULT_CTX, 1, 64, 64), name_seed("phydnet.default.x"))
    with torch.no_grad():
        pred, _ = m(x.cuda(), pred_frames=PHY_DEFAULT_PRED)
    assert _relmax(pred[:, :, :, ::4, ::4], g["pred_slice"]) < FWD_TOL
    assert abs(checksum(pred) - float(g["pred_chk"])) <= 1e-4 * max(1.0, abs(float(g["pred_chk"])))


def test_phydnet_train_iter_with_flat_adam(vpx):
    """Two batches through the model's own train_iter (epoch 0: teacher forcing ratio 1) with the package's fused Adam: the loss is finite,
    the parameters move, and the moment loss falls from one step to the next."""
    from vp_suite_amd import phy_ops
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.train import FlatAdam, _link_views
    m = _model(PHY_TINY_KW, "tiny", "f32")
    params = list(m.parameters())
    total = sum(p.numel() for p in params)
    flat_p = torch.empty(total, device="cuda")
    flat_g = torch.zeros(total, device="cuda")
    _link_views(params, flat_p, "data")
    _link_views(params, flat_g, "grad")
    opt = FlatAdam(params, flat_p, flat_g, lr=1e-3)
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    T = PHY_TRAIN_CTX + PHY_TRAIN_PRED
    loader = [{"frames": seeded_rand((2, T, 1, 32, 32), name_seed(f"phydnet.train_iter.{i}")).cuda(), "actions": torch.zeros(2, T - 1, 0)}
              for i in range(2)]
    cfg = {"device": "cuda", "context_frames": PHY_TRAIN_CTX, "pred_frames": PHY_TRAIN_PRED}
    fr = loader[0]["frames"]
    loss0 = m.training_loss(fr[:, :PHY_TRAIN_CTX], fr[:, PHY_TRAIN_CTX:], PHY_TRAIN_PRED, lp, teacher_forcing=True)
    assert torch.isfinite(loss0)
    w1 = m.phycell.cell_list[0].F.conv1.weight
    with torch.no_grad():
        moments = [float(phy_ops.moment_loss(w1))]
    before = flat_p.clone()
    for step in range(2):
        m.train_iter(cfg, loader[step:step + 1], opt, lp, epoch=0)
        with torch.no_grad():
            moments.append(float(phy_ops.moment_loss(w1)))
    assert torch.isfinite(flat_p).all() and not torch.equal(before, flat_p)
    assert moments[2] < moments[1] < moments[0], moments
