"""ST-Phy ("st-phy") on the GPU: the three new operators against torch in fp64 on the same inputs (forward and every gradient, both
operand modes, odd sizes, the eps branch of the row normalisation, W != H, one output channel, bit-reproducible parameter
gradients), the Autoencoder and the model against the reference's fixtures (tools/gen_golden_stphy.py), and one train_iter pass.

Bars (the project's own, tests/test_gpu_phydnet.py): forward relmax < 1e-4, block-level forwards < 1e-5, gradients < 5e-5; bf16x3
whole-model gradients are held to BF16X3_VS_PERTURBED times what a PERTURB weight perturbation does to the f32 gradients, measured
in the same test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import checksum, load_golden, name_seed, seeded_rand, seeded_randn
from parity import relmax as _relmax
from test_gpu_phydnet import BF16X3_VS_PERTURBED, PERTURB
from test_stphy_host import (STPHY_AE_B, STPHY_AE_ENC_C, STPHY_AE_SHAPE, STPHY_DEFAULT_B, STPHY_DEFAULT_CTX, STPHY_DEFAULT_KW,
                             STPHY_DEFAULT_PRED, STPHY_DEFAULT_SLICES, STPHY_TINY3_KW, STPHY_TINY_B, STPHY_TINY_CTX, STPHY_TINY_KW, STPHY_TINY_PRED,
                             STPHY_TRAIN_CTX, STPHY_TRAIN_PRED, grad_kept, stphy_fill_)

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
BLOCK_TOL = 1e-5
GRAD_TOL = 5e-5
# Ceiling of every gradient tolerance DERIVED from a perturbed run: half of the relative error of one plain-bf16 product (4e-3, the
# precision defect these bf16x3 tests exist to catch, tests/test_gpu_phydnet.py). A derived tolerance above it -- e.g. because one ReLU
# unit flipped in the perturbed run -- would let that defect through, so the test fails instead of using it.
BF16X3_GRAD_CEILING = 2e-3


def _p(name, shape, scale=1.0):
    return seeded_randn(shape, name_seed("stphy.gpu." + name), scale)


# ---- item 1: convolution + ReLU -------------------------------------------------------------------------------------------------
# (tag, N, H, W, Ci, Co, k, stride, transposed, act): the autoencoder's layers at 64x64 (30x30 -> 14x14 and 28x28 -> 60x60 among them),
# W != H, and the one-channel head
CONV_ACT_CASES = [("enc.conv1", 2, 64, 64, 1, 32, 5, 2, 0, "relu"), ("enc.conv2", 2, 30, 30, 32, 64, 3, 2, 0, "relu"),
                  ("enc.mean", 2, 14, 14, 64, 64, 3, 1, 0, None), ("dec.fc1", 2, 12, 12, 64, 64, 1, 1, 0, "relu"),
                  ("dec.conv1", 2, 12, 12, 64, 64, 6, 2, 1, "relu"), ("dec.conv2", 2, 28, 28, 64, 32, 6, 2, 1, "relu"),
                  ("dec.conv3", 2, 60, 60, 32, 1, 5, 1, 1, None), ("enc.conv2_wide", 3, 14, 18, 32, 64, 3, 2, 0, "relu"),
                  ("dec.conv2_wide", 3, 12, 16, 16, 32, 6, 2, 1, "relu"), ("head_relu", 2, 36, 44, 32, 1, 5, 1, 1, "relu"),
                  ("enc.conv1_rgb", 2, 40, 32, 3, 32, 5, 2, 0, "relu")]


def _conv_ref(x, w, b, stride, tr, act):
    y = (F.conv_transpose2d if tr else F.conv2d)(x, w, b, stride=stride)
    return F.relu(y) if act == "relu" else y


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", CONV_ACT_CASES, ids=lambda c: c[0])
def test_conv2d_act_vs_fp64(vpx, case, precision, parity_log):
    from vp_suite_amd import stphy_ops
    tag, N, H, W, Ci, Co, k, s, tr, act = case
    wshape = (Ci, Co, k, k) if tr else (Co, Ci, k, k)
    x = _p(tag + ".x", (N, Ci, H, W))
    w = _p(tag + ".w", wshape, 1.0 / np.sqrt(Ci * k * k))
    b = _p(tag + ".b", (Co,), 0.1)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = _conv_ref(xr, wr, br, s, tr, act)
    gy = _p(tag + ".gy", tuple(yr.shape))
    if act == "relu":
        # ReLU' jumps at 0: two outputs that both hold the forward bar may disagree on the sign of a pre-activation that lies within that
        # bar of the kink, and then differ by the whole cotangent there. Those elements (decided on the fp64 reference alone) get a zero
        # cotangent; everywhere else the derivative is unambiguous and the gradients are compared in full.
        pre = _conv_ref(xr.detach(), wr.detach(), br.detach(), s, tr, None)
        gy = gy * (pre.abs() >= BLOCK_TOL * float(yr.detach().abs().max())).float()
    (yr * gy.double()).sum().backward()
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = stphy_ops.conv2d_act(xg, wg, bg, s, 0, transposed=bool(tr), act=act, precision=precision)
    assert tuple(y.shape) == tuple(yr.shape)
    (y * gy.cuda()).sum().backward()
    errs = {"y": parity_log(f"{tag}.y", y, yr, BLOCK_TOL), "dx": parity_log(f"{tag}.dx", xg.grad, xr.grad, GRAD_TOL),
            "dw": parity_log(f"{tag}.dw", wg.grad, wr.grad, GRAD_TOL), "db": parity_log(f"{tag}.db", bg.grad, br.grad, GRAD_TOL)}
    assert errs["y"] < BLOCK_TOL and max(errs["dx"], errs["dw"], errs["db"]) < GRAD_TOL, errs
    if act == "relu":   # exact zeros where the reference has them, and no gradient through them
        assert bool(((y == 0) == (yr == 0).cuda()).float().mean() > 0.999)


def test_conv2d_act_relu_gradient_is_zero_at_zero(vpx):
    """ReLU' comes from the saved output: y > 0, so zero AT zero (torch's convention). A layer whose pre-activation is exactly 0 everywhere
    (zero weights, zero bias) passes no gradient."""
    from vp_suite_amd import stphy_ops
    x = _p("z.x", (2, 8, 10, 12)).cuda().requires_grad_(True)
    w = torch.zeros(16, 8, 3, 3, device="cuda", requires_grad=True)
    b = torch.zeros(16, device="cuda", requires_grad=True)
    y = stphy_ops.conv2d_act(x, w, b, 1, 0, act="relu")
    y.sum().backward()
    assert float(y.abs().max()) == 0.0
    assert float(x.grad.abs().max()) == 0.0 and float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0


# ---- item 2: encoder tail ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 12, 12), (3, 16, 4, 6), (2, 7, 5, 9), (2, 16, 6, 4)], ids=lambda s: "x".join(map(str, s)))
def test_relu_rownorm_vs_fp64(vpx, shape, parity_log):
    from vp_suite_amd import stphy_ops
    x = _p("rn.x" + str(shape), shape)
    x[0, 0, 1, :] = -x[0, 0, 1, :].abs() - 0.1          # a row that is all < 0 before ReLU: the eps branch
    x[1, 1, 0, :] = 0.0                                 # ... and one that is exactly 0
    x[1, 2, 2, 1:] = -1.0                               # a single survivor
    xr = x.double().requires_grad_(True)
    yr = F.normalize(F.relu(xr), p=2, dim=-1, eps=1e-8)
    gy = _p("rn.gy" + str(shape), shape)
    (yr * gy.double()).sum().backward()
    xg = x.cuda().requires_grad_(True)
    y = stphy_ops.relu_rownorm(xg, eps=1e-8)
    (y * gy.cuda()).sum().backward()
    assert torch.isfinite(y).all() and torch.isfinite(xg.grad).all()
    assert float(y[0, 0, 1].abs().max()) == 0.0 and float(xg.grad[0, 0, 1].abs().max()) == 0.0
    ey, ex = parity_log("rownorm.y", y, yr, BLOCK_TOL), parity_log("rownorm.dx", xg.grad, xr.grad, GRAD_TOL)
    assert ey < BLOCK_TOL and ex < GRAD_TOL, (ey, ex)
    # along W, not H: a transposed input gives the transposed result only for the other axis
    yt = stphy_ops.relu_rownorm(x.transpose(2, 3).contiguous().cuda())
    ytr = F.normalize(F.relu(x.double().transpose(2, 3)), p=2, dim=-1, eps=1e-8)
    assert _relmax(yt, ytr) < BLOCK_TOL


def test_relu_rownorm_eps_branch_gradient(vpx, parity_log):
    """Rows with 0 < ||r|| < eps: y = r / eps and dx = dy / eps masked by ReLU' (the clamp's derivative is zero there)."""
    from vp_suite_amd import stphy_ops
    x = torch.full((1, 4, 2, 6), -1.0)
    x[0, :, 0, 2] = 3e-10
    x[0, :, 1, :] = torch.tensor([1.0, -2.0, 3.0, 0.5, -0.1, 2.0])
    xr = x.double().requires_grad_(True)
    yr = F.normalize(F.relu(xr), p=2, dim=-1, eps=1e-8)
    gy = _p("rn.eps.gy", x.shape)
    (yr * gy.double()).sum().backward()
    xg = x.cuda().requires_grad_(True)
    y = stphy_ops.relu_rownorm(xg)
    (y * gy.cuda()).sum().backward()
    assert abs(float(y[0, 0, 0, 2]) - 3e-2) < 1e-8
    assert parity_log("rownorm.eps.y", y, yr, BLOCK_TOL) < BLOCK_TOL
    assert parity_log("rownorm.eps.dx", xg.grad, xr.grad, GRAD_TOL) < GRAD_TOL


# ---- item 3: merge -----------------------------------------------------------------------------------------------------------------
MERGE_CASES = [(2, 16, 16, 16, 4, 6, True), (2, 64, 64, 64, 12, 12, False), (16, 64, 64, 64, 12, 12, True), (3, 48, 16, 24, 5, 7, True)]


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", MERGE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_merge1x1_vs_fp64(vpx, case, precision, parity_log):
    from vp_suite_amd import stphy_ops
    N, Cs, Cp, Co, H, W, has_bias = case
    a, b = _p(f"mg.a{case}", (N, Cs, H, W)), _p(f"mg.b{case}", (N, Cp, H, W))
    w = _p(f"mg.w{case}", (Co, Cs + Cp, 1, 1), 1.0 / np.sqrt(Cs + Cp))
    bias = _p(f"mg.bias{case}", (Co,), 0.1) if has_bias else None
    ref_in = [t.double().requires_grad_(True) for t in (a, b, w)] + ([bias.double().requires_grad_(True)] if has_bias else [])
    yr = F.conv2d(torch.cat([ref_in[0], ref_in[1]], dim=1), ref_in[2], ref_in[3] if has_bias else None)
    gy = _p(f"mg.gy{case}", tuple(yr.shape))
    (yr * gy.double()).sum().backward()
    gpu_in = [t.cuda().requires_grad_(True) for t in (a, b, w)] + ([bias.cuda().requires_grad_(True)] if has_bias else [])
    y = stphy_ops.merge1x1(gpu_in[0], gpu_in[1], gpu_in[2], gpu_in[3] if has_bias else None, precision=precision)
    (y * gy.cuda()).sum().backward()
    errs = [parity_log("merge.y", y, yr, BLOCK_TOL)]
    errs += [parity_log(f"merge.d{n}", g.grad, r.grad, GRAD_TOL) for n, g, r in zip(("a", "b", "w", "bias"), gpu_in, ref_in)]
    assert errs[0] < BLOCK_TOL and max(errs[1:]) < GRAD_TOL, errs


def test_stphy_param_grads_bit_reproducible(vpx):
    """Parameter-gradient sums run in a fixed order with no float atomics: two runs under deterministic algorithms agree bit for bit."""
    from vp_suite_amd import stphy_ops
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            x = _p("det.x", (16, 32, 30, 30)).cuda()
            w = _p("det.w", (64, 32, 3, 3), 0.06).cuda().requires_grad_(True)
            b = _p("det.b", (64,), 0.1).cuda().requires_grad_(True)
            y = stphy_ops.conv2d_act(x, w, b, 2, 0, act="relu", precision="bf16x3")
            a2 = _p("det.a", (16, 64, 12, 12)).cuda()
            wm = _p("det.wm", (64, 128, 1, 1), 0.09).cuda().requires_grad_(True)
            bm = _p("det.bm", (64,), 0.1).cuda().requires_grad_(True)
            z = stphy_ops.merge1x1(a2, a2 * 0.5, wm, bm, precision="bf16x3")
            (y.square().sum() + z.square().sum()).backward()
            runs.append([t.grad.clone() for t in (w, b, wm, bm)])
        for g0, g1 in zip(*runs):
            assert torch.equal(g0, g1)
    finally:
        torch.use_deterministic_algorithms(prev)


# ---- Autoencoder against the reference -----------------------------------------------------------------------------------------------
def _grad_table(g, k):
    """{name: (sum, sumsq, max, kept)} of a fixture pass written by tools/gen_golden_stphy.py (_put_grads)."""
    names = [str(n) for n in g[f"{k}.gnames"]]
    off = np.concatenate([[0], np.cumsum(g[f"{k}.gkept_n"])])
    return {n: (*g[f"{k}.gstats"][i], g[f"{k}.gkept"][off[i]:off[i + 1]]) for i, n in enumerate(names)}


def _none_names(g, k):
    return {str(n) for n in g[f"{k}.none"] if str(n)}


def _check_grad_table(named_grads, g, k, parity_log, tol):
    """Per parameter with a reference gradient: the sum (relative to the L1 norm), the sum of squares, and the kept elements with
    max|delta| / max|ref| over the whole tensor; every figure is recorded before the assertion, which names all that miss the bound.
    A parameter whose reference gradient is None must have None or an all-zero gradient."""
    table, none, bad = _grad_table(g, k), _none_names(g, k), []
    assert set(named_grads) == set(table) | none, set(named_grads) ^ (set(table) | none)
    for name in sorted(none):
        gr = named_grads[name]
        assert gr is None or float(gr.abs().max()) == 0.0, name
    for name, (gs, gq, gmax, gkept) in table.items():
        assert named_grads[name] is not None, name
        a = named_grads[name].detach().double().cpu().numpy().reshape(-1)
        l1 = float(np.abs(a).sum())
        errs = (parity_log(f"{k}.gsum.{name}", np.array([a.sum(), l1]), np.array([gs, l1]), tol),
                parity_log(f"{k}.gsq.{name}", np.array([(a * a).sum()]), np.array([gq]), 2 * tol),
                parity_log(f"{k}.grad.{name}", np.append(grad_kept(a), gmax), np.append(gkept, gmax), tol))
        if errs[0] >= tol or errs[1] >= 2 * tol or errs[2] >= tol:
            bad.append((name, errs))
    assert not bad, bad


def _elem_grad_error(named_grads, g, k):
    worst = 0.0
    for name, (_, _, gmax, gkept) in _grad_table(g, k).items():
        a = grad_kept(named_grads[name].detach().double().cpu().numpy().reshape(-1))
        worst = max(worst, float(np.abs(a - gkept).max()) / float(gmax))
    return worst


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_autoencoder_vs_golden(vpx, precision, parity_log):
    from vp_suite_amd.model_blocks import Autoencoder
    g = load_golden("stphy_ae")
    ae = Autoencoder(STPHY_AE_SHAPE, STPHY_AE_ENC_C, "cuda")
    stphy_fill_(ae, name_seed("stphy.ae"))
    ae.encoder.precision = ae.decoder.precision = precision
    c, h, w = STPHY_AE_SHAPE
    x = seeded_rand((STPHY_AE_B, c, h, w), name_seed("stphy.ae.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9 * max(1.0, abs(float(g["chk_x"])))
    xg = x.cuda().requires_grad_(True)
    z = ae.encode(xg)
    out = ae.decode(z)
    assert tuple(z.shape) == tuple(g["z"].shape) and tuple(out.shape) == tuple(g["out"].shape)
    # f32: the block-level bar. bf16x3: a chain of seven layers, each held to the project's per-layer bf16x3 bound (5e-5 against fp64,
    # tests/test_gpu_phydnet.py), is a forward of a composite: the forward bar
    tol = BLOCK_TOL if precision == "f32" else FWD_TOL
    ez, eo = parity_log("ae.z", z, g["z"], tol), parity_log("ae.out", out, g["out"], tol)
    assert ez < tol and eo < tol, (ez, eo)
    gz = seeded_randn(z.shape, name_seed("stphy.ae.gz")).cuda()
    go = seeded_randn(out.shape, name_seed("stphy.ae.go")).cuda()
    ((z * gz).sum() + (out * go).sum()).backward()
    grads = {n: p.grad for n, p in ae.named_parameters()}
    grads["__x__"] = xg.grad
    tol = GRAD_TOL
    if precision != "f32":
        # bf16x3 gradients of a composite (seven layers, six ReLU kinks, a normalisation by row norms that can be small) are held the way
        # the whole model's are: to BF16X3_VS_PERTURBED times what a PERTURB weight perturbation does to the f32 gradients, measured here
        ap = Autoencoder(STPHY_AE_SHAPE, STPHY_AE_ENC_C, "cuda")
        stphy_fill_(ap, name_seed("stphy.ae"))
        with torch.no_grad():
            for name, p in ap.named_parameters():
                p.mul_(1.0 + PERTURB * seeded_randn(p.shape, name_seed(f"stphy.perturb.{name}")).cuda())
        xp = x.cuda().requires_grad_(True)
        zp = ap.encode(xp)
        op = ap.decode(zp)
        # The perturbation must stay a small one: its own forward holds the forward bar. (Here it moves the forward by LESS than half of
        # what bf16x3 does -- measured 2.6e-5 against 5.9e-5 on z -- so unlike in the model test the inequality fwd_err <= 2 * fwd_err_p
        # does not hold and is not asserted: a smaller perturbation only makes the gradient bound stricter.) What keeps the bound from
        # being inflated by an accident of the perturbed run (one flipped ReLU unit) is the ceiling below.
        fwd_err_p = max(parity_log("g.perturbed_f32.z", zp, g["z"], None), parity_log("g.perturbed_f32.out", op, g["out"], None))
        assert fwd_err_p < FWD_TOL, fwd_err_p
        ((zp * gz).sum() + (op * go).sum()).backward()
        gp = {n: p.grad for n, p in ap.named_parameters()}
        gp["__x__"] = xp.grad
        tol = BF16X3_VS_PERTURBED * _elem_grad_error(gp, g, "g")
        parity_log("g.perturbed_f32.grad_bound", np.array([tol]), np.array([tol]), None)
        assert tol <= BF16X3_GRAD_CEILING, tol
    _check_grad_table(grads, g, "g", parity_log, tol)


# ---- the model against the reference ------------------------------------------------------------------------------------------------
def _model(kw, tag, precision):
    from vp_suite_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES["st-phy"]("cuda", cell_precision=precision, **kw)
    stphy_fill_(m, name_seed(f"stphy.{tag}"))
    return m.cuda()


def _train_step(m, xt, lp, tf):
    m.zero_grad(set_to_none=True)
    out, ml = m(xt, pred_frames=STPHY_TRAIN_PRED, train=True, teacher_forcing=tf)
    _, total = lp.get_losses(out, xt[:, 1:])
    for v in ml.values():
        total = total + v
    total.backward()
    return out, ml, total


def _perturbed_f32(kw, tag):
    m = _model(kw, tag, "f32")
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.mul_(1.0 + PERTURB * seeded_randn(p.shape, name_seed(f"stphy.perturb.{name}")).cuda())
    return m


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_stphy_tiny_model_vs_golden(vpx, precision, parity_log):
    from vp_suite_amd.measure import PredictionLossProvider
    kw, tag = STPHY_TINY_KW, "tiny"
    g = load_golden("stphy_tiny")
    m = _model(kw, tag, precision)
    c, h, w = kw["img_shape"]
    x = seeded_rand((STPHY_TINY_B, STPHY_TINY_CTX, c, h, w), name_seed("stphy.tiny.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9 * max(1.0, abs(float(g["chk_x"])))
    with torch.no_grad():
        pred, ml = m(x.cuda(), pred_frames=STPHY_TINY_PRED)
        assert ml is None and pred.shape == (STPHY_TINY_B, STPHY_TINY_PRED, c, h, w)
        e1 = parity_log("eval", pred, g["eval"], FWD_TOL)
        e2 = parity_log("pred1", m.pred_1(x.cuda()), g["pred1"], FWD_TOL)
        assert e1 < FWD_TOL and e2 < FWD_TOL, (e1, e2)
    xt = seeded_rand((STPHY_TINY_B, STPHY_TRAIN_CTX + STPHY_TRAIN_PRED, c, h, w), name_seed("stphy.tiny.xt")).cuda()
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    for tf in (False, True):
        k = f"tf{int(tf)}"
        out, ml, total = _train_step(m, xt, lp, tf)
        assert out.shape[1] == STPHY_TRAIN_CTX + STPHY_TRAIN_PRED - 1
        fwd_err = parity_log(f"{k}.frames", out, g[f"{k}.frames"], FWD_TOL)
        assert fwd_err < FWD_TOL
        moment, dec = ml["moment regularization loss"], ml["memory decoupling loss"]
        assert abs(moment.item() - float(g[f"{k}.moment"])) <= 1e-5 * abs(float(g[f"{k}.moment"]))
        assert abs(dec.item() - float(g[f"{k}.decouple"])) <= FWD_TOL * abs(float(g[f"{k}.decouple"]))
        assert abs(total.item() - float(g[f"{k}.total"])) <= FWD_TOL * abs(float(g[f"{k}.total"]))
        grads = {n: p.grad for n, p in m.named_parameters()}
        if precision == "f32":
            _check_grad_table(grads, g, k, parity_log, GRAD_TOL)
            continue
        # bf16x3: against the same f32 model under a weight perturbation (test_gpu_phydnet.py: PERTURB, BF16X3_VS_PERTURBED)
        mp = _perturbed_f32(kw, tag)
        out_p, _, _ = _train_step(mp, xt, lp, tf)
        fwd_err_p = parity_log(f"{k}.perturbed_f32.frames", out_p, g[f"{k}.frames"], None)
        assert fwd_err <= 2.0 * fwd_err_p, (fwd_err, fwd_err_p)          # the perturbation is at least as large as bf16x3's
        tol = BF16X3_VS_PERTURBED * _elem_grad_error({n: p.grad for n, p in mp.named_parameters()}, g, k)
        parity_log(f"{k}.perturbed_f32.grad_bound", np.array([tol]), np.array([tol]), None)
        assert tol <= BF16X3_GRAD_CEILING, tol
        _check_grad_table(grads, g, k, parity_log, tol)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_stphy_tiny3_model_vs_golden(vpx, precision, parity_log):
    kw = STPHY_TINY3_KW
    g = load_golden("stphy_tiny3")
    m = _model(kw, "tiny3", precision)
    c, h, w = kw["img_shape"]
    x = seeded_rand((STPHY_TINY_B, STPHY_TINY_CTX, c, h, w), name_seed("stphy.tiny3.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9 * max(1.0, abs(float(g["chk_x"])))
    with torch.no_grad():
        pred, ml = m(x.cuda(), pred_frames=STPHY_TINY_PRED)
    assert ml is None
    assert parity_log("eval", pred, g["eval"], FWD_TOL) < FWD_TOL


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_stphy_default_model_vs_golden(vpx, precision, parity_log):
    g = load_golden("stphy_default")
    m = _model(STPHY_DEFAULT_KW, "default", precision)
    assert sum(p.numel() for p in m.parameters()) == int(g["n_params"])
    x = seeded_rand((STPHY_DEFAULT_B, STPHY_DEFAULT_CTX, 1, 64, 64), name_seed("stphy.default.x"))
    with torch.no_grad():
        pred, _ = m(x.cuda(), pred_frames=STPHY_DEFAULT_PRED)
    assert pred.shape == (STPHY_DEFAULT_B, STPHY_DEFAULT_PRED, 1, 64, 64)
    errs = [parity_log("pred_slice", pred[:, :, :, ::4, ::4], g["pred_slice"], FWD_TOL)]
    # three more offset slices: with the first one a quarter of every frame is held element-wise to the forward bar
    for oy, ox in STPHY_DEFAULT_SLICES:
        errs.append(parity_log(f"pred_slice_{oy}{ox}", pred[:, :, :, oy::4, ox::4], g[f"pred_slice_{oy}{ox}"], FWD_TOL))
    assert max(errs) < FWD_TOL, errs
    # The checksum sums all n elements with weights cos(0.37 i): it covers the pixels the slices skip. f32 holds the bound the PhyDNet
    # fixture uses (1e-4 of the checksum). That bound is relative to a sum that cancels (|chk| = 50 over 40960 elements of magnitude up
    # to 5), so it asks more of each element than the forward bar does; bf16x3 is held to what the bar implies for elements whose errors
    # do not conspire: each within eps = FWD_TOL * max|ref|, weights of mean square 1/2, hence a deviation of eps * sqrt(n / 2), at 3
    # deviations. (A 1 % error of random sign on the unsliced pixels is ~20 of these bounds.)
    chk_tol = 1e-4 * max(1.0, abs(float(g["pred_chk"])))
    if precision != "f32":
        ref_max = max(float(np.abs(g[k]).max()) for k in g if k.startswith("pred_slice"))
        chk_tol = 3.0 * FWD_TOL * ref_max * np.sqrt(pred.numel() / 2.0)
    chk_err = abs(checksum(pred) - float(g["pred_chk"]))
    parity_log("pred_chk", np.array([checksum(pred), chk_tol]), np.array([float(g["pred_chk"]), chk_tol]), None)
    assert chk_err <= chk_tol, (chk_err, chk_tol)


def test_stphy_train_iter_with_flat_adam(vpx):
    """One pass of the model's own train_iter over two batches with the package's fused Adam: every loss it computes is finite, every live parameter
    changes, and every dead one (reference gradient None) stays as it was."""
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.train import FlatAdam, _link_views
    g = load_golden("stphy_tiny")
    dead = _none_names(g, "tf1") & _none_names(g, "tf0")
    assert dead
    m = _model(STPHY_TINY_KW, "tiny", "f32")
    params = list(m.parameters())
    total = sum(p.numel() for p in params)
    flat_p = torch.empty(total, device="cuda")
    flat_g = torch.zeros(total, device="cuda")
    _link_views(params, flat_p, "data")
    _link_views(params, flat_g, "grad")
    opt = FlatAdam(params, flat_p, flat_g, lr=1e-3)
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    T = STPHY_TRAIN_CTX + STPHY_TRAIN_PRED
    loader = [{"frames": seeded_rand((2, T, 1, 32, 40), name_seed(f"stphy.train_iter.{i}")).cuda(), "actions": torch.zeros(2, T - 1, 0)}
              for i in range(2)]
    cfg = {"device": "cuda", "context_frames": STPHY_TRAIN_CTX, "pred_frames": STPHY_TRAIN_PRED}
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    losses, total_loss = [], m._total_loss

    def recording(*args):          # the loss train_iter itself differentiates, batch by batch
        value = total_loss(*args)
        losses.append(value.detach())
        return value
    m._total_loss = recording
    m.train_iter(cfg, loader, opt, lp, epoch=0)     # ONE pass over the two batches
    assert len(losses) == 2 and all(bool(torch.isfinite(v)) for v in losses), losses
    assert torch.isfinite(flat_p).all()
    for n, p in m.named_parameters():
        if n in dead:
            assert torch.equal(p, before[n]), n
        else:
            assert not torch.equal(p, before[n]), n
