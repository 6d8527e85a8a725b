"""UNet-3D on the GPU: the replicate-border convolution (forward, both data gradients, weight gradient; one and two sources; the eval
epilogue), BatchNorm + ReLU (+ pool) forward / backward with the running-statistic update, the time collapse, and the model against the
reference's fixtures (tests/golden/unet3d_*.npz, tools/gen_golden_unet3d.py).

References are torch's own ops with autograd on the same inputs, on the CPU in fp64 (tests/unet3d_ref.py states the layers).
Tolerances (max-normalised, max|got - ref| / max|ref|): 1e-4 on every forward output and eval frame; 5e-5 on the gradients of the plain
convolution and of the time collapse (fixed sums of fp32 products, the suite's existing gradient bar). Behind a BatchNorm the gradient
error is not derivable in advance (division by a batch standard deviation): there each bar is 3 x the error of the fp32 restatement
against its own fp64 run on the same inputs (the kernels add in another order), never below 5e-5 — measured in the test from the
reference alone, before the library's result is looked at. On the fixture inputs this measures 6.6e-7 for the blocks (bar 5e-5) and
1.92e-5 for the tiny model's worst parameter (bar 5.8e-5). Parameters whose exact gradient is zero (a bias in front of a BatchNorm:
time3ds.*.bias, the transposed convolutions' biases) are held to the same bar relative to their layer's weight gradient."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet3d_ref
from golden_util import checksum, load_golden, name_seed, seeded_rand, seeded_randn
from parity import relmax as _relmax
from test_unet3d_host import (UNET_BLOCKS, UNET_DEFAULT_B, UNET_DEFAULT_CTX, UNET_DEFAULT_KW, UNET_DEFAULT_PRED, UNET_DEFAULT_SLICES, UNET_TINY3_KW,
                              UNET_TINY_B, UNET_TINY_CTX, UNET_TINY_KW, UNET_TINY_PRED, buffers_of, fixture_grads, grad_kept, tiny_inputs, unet3d_fill_)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, GRAD_TOL = 1e-4, 5e-5


def frames(t):
    """[B,C,T,H,W] or [B,C,H,W] (the reference's layouts) -> the library's [B,T,H,W,C] on the GPU."""
    if t.dim() == 4:
        t = t.unsqueeze(2)
    return t.permute(0, 2, 3, 4, 1).contiguous().float().to(DEV)


def unframes(t, dims=3):
    t = t.detach().cpu().permute(0, 4, 1, 2, 3)
    return t.squeeze(2) if dims == 2 else t


def bar_from(ref32, ref64):
    """3 x the fp32 restatement's own error against its fp64 run, never below the suite's 5e-5."""
    err = float((ref32.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))
    return max(3.0 * err, GRAD_TOL)


# ---- replicate-border convolution ----------------------------------------------------------------------------------------------------
MAPS = [(1, 1), (2, 3), (5, 7), (18, 34)]
TIMES = [(1, 1), (1, 3), (2, 3), (3, 3)]          # (T, time taps)


def _conv_case(T, kt, H, W, Ca, Cb, Co, seed):
    x = seeded_randn((2, Ca + Cb, T, H, W), seed).double().requires_grad_(True)
    w = seeded_randn((Co, Ca + Cb, kt, 3, 3), seed + 1, 0.2).double().requires_grad_(True)
    go = seeded_randn((2, Co, T, H, W), seed + 2).double()
    ref = F.conv3d(F.pad(x, (1, 1, 1, 1, kt // 2, kt // 2), mode="replicate"), w)
    ref.backward(go)
    return x, w, go, ref.detach()


@pytest.mark.parametrize("T,kt", TIMES)
@pytest.mark.parametrize("H,W", MAPS)
def test_replicate_conv_vs_torch(vpx, H, W, T, kt):
    from vp_suite_amd import unet_ops
    for Ci, Co in [(1, 4), (3, 8), (8, 24), (20, 4), (1, 24), (3, 4), (8, 8), (20, 24), (20, 8)]:
        x, w, go, ref = _conv_case(T, kt, H, W, Ci, 0, Co, name_seed(f"rconv.{H}.{W}.{T}.{kt}.{Ci}.{Co}"))
        xs = frames(x.detach()).requires_grad_(True)
        wd = (w.detach().float() if kt == 3 else w.detach().float()[:, :, 0]).to(DEV).requires_grad_(True)     # kt = 1: a Conv2d weight
        y = unet_ops.replicate_conv(xs, wd)
        y.backward(frames(go))
        tag = (H, W, T, kt, Ci, Co)
        assert _relmax(unframes(y), ref) < FWD_TOL, tag
        assert _relmax(unframes(xs.grad), x.grad) < GRAD_TOL, tag
        assert _relmax(wd.grad.cpu().reshape(w.shape), w.grad) < GRAD_TOL, tag


@pytest.mark.parametrize("Ca,Cb", [(4, 4), (8, 20)])
@pytest.mark.parametrize("H,W", MAPS)
def test_replicate_conv_two_sources_vs_torch(vpx, H, W, Ca, Cb):
    from vp_suite_amd import unet_ops
    for (T, kt), Co in [((1, 1), 4), ((1, 1), 24), ((3, 3), 8)]:
        x, w, go, ref = _conv_case(T, kt, H, W, Ca, Cb, Co, name_seed(f"rconv2.{H}.{W}.{T}.{Ca}.{Cb}.{Co}"))
        a = frames(x.detach()[:, :Ca]).requires_grad_(True)
        b = frames(x.detach()[:, Ca:]).requires_grad_(True)
        wd = (w.detach().float() if kt == 3 else w.detach().float()[:, :, 0]).to(DEV).requires_grad_(True)
        y = unet_ops.replicate_conv(a, wd, b=b)
        y.backward(frames(go))
        tag = (H, W, T, kt, Ca, Cb, Co)
        assert _relmax(unframes(y), ref) < FWD_TOL, tag
        assert _relmax(unframes(a.grad), x.grad[:, :Ca]) < GRAD_TOL, tag
        assert _relmax(unframes(b.grad), x.grad[:, Ca:]) < GRAD_TOL, tag
        assert _relmax(wd.grad.cpu().reshape(w.shape), w.grad) < GRAD_TOL, tag


def _bn(C, dims, seed, train):
    bn = (torch.nn.BatchNorm3d if dims == 3 else torch.nn.BatchNorm2d)(C)
    with torch.no_grad():
        bn.weight.copy_(1.0 + seeded_randn((C,), seed, 0.1))
        bn.bias.copy_(seeded_randn((C,), seed + 1, 0.1))
        bn.running_mean.copy_(seeded_randn((C,), seed + 2, 0.1))
        bn.running_var.copy_(0.5 + 5.0 * seeded_randn((C,), seed + 3, 0.1).abs())
    return bn.train(train)


@pytest.mark.parametrize("H,W", MAPS)
def test_replicate_conv_eval_epilogue_vs_torch(vpx, H, W):
    """Folded BatchNorm (running statistics) + ReLU in the convolution's epilogue, one and two sources, with the eval path's pool."""
    from vp_suite_amd import unet_ops
    for (T, kt), (Ca, Cb), Co in [((1, 1), (3, 0), 4), ((3, 3), (8, 0), 24), ((1, 1), (8, 20), 8), ((2, 3), (1, 0), 8)]:
        seed = name_seed(f"rconv.eval.{H}.{W}.{T}.{Ca}.{Cb}.{Co}")
        x, w, _, raw = _conv_case(T, kt, H, W, Ca, Cb, Co, seed)
        bn = _bn(Co, 3, seed + 10, train=False)
        ref = F.relu(bn.double()(raw))
        bn = bn.float().to(DEV)
        a = frames(x.detach()[:, :Ca])
        b = frames(x.detach()[:, Ca:]) if Cb else None
        wd = (w.detach().float() if kt == 3 else w.detach().float()[:, :, 0]).to(DEV)
        pool = H % 2 == 0 and W % 2 == 0
        with torch.no_grad():
            out = unet_ops.conv_bn_relu(a, wd, bn, b=b, pool=pool)
        y = out[0] if pool else out
        assert _relmax(unframes(y), ref.detach()) < FWD_TOL, (H, W, T, kt, Ca, Cb, Co)
        if pool:
            assert torch.equal(unframes(out[1]), F.max_pool3d(unframes(y), (1, 2, 2), (1, 2, 2)))
        assert int(bn.num_batches_tracked) == 0
        with pytest.raises(vpx._lib.VpxError):        # the eval epilogue has no backward
            unet_ops.conv_bn_relu(a, wd.clone().requires_grad_(True), bn, b=b)


# ---- BatchNorm + ReLU (+ pool), training ---------------------------------------------------------------------------------------------
BN_CASES = [  # (B, T, H, W, pool): 2 values per channel; 2*3*5*7; an even map for the pooled output
    (2, 1, 1, 1, False), (2, 3, 5, 7, False), (2, 3, 6, 8, True), (2, 1, 2, 2, True)]


@pytest.mark.parametrize("C", [4, 24])
@pytest.mark.parametrize("B,T,H,W,pool", BN_CASES)
def test_conv_bn_relu_training_vs_torch(vpx, B, T, H, W, pool, C):
    """conv (training epilogue: batch statistics) -> BatchNorm + ReLU (+ pool): outputs, every gradient (the pooled output's routed to
    the first maximum), and the running statistics after one and after three calls."""
    from vp_suite_amd import unet_ops
    Ci, seed = 3, name_seed(f"bn.{B}.{T}.{H}.{W}.{C}")
    x0 = seeded_randn((B, Ci, T, H, W), seed)
    if B * T * H * W == 2:
        # Two values y1, y2 per channel: x-hat = +-s with s^2 = var / (var + eps), and the data gradient is (g1 - g2) / 2 * (1 - s^2) *
        # gamma / std. At var >> eps that is eps / var of its terms, rounding noise no bar can be set against; inputs of this size
        # put the batch variances around eps (1e-5), where the gradient is a quantity of its terms' size.
        x0 = x0 * 3e-3
    w0 = seeded_randn((C, Ci, 3, 3, 3), seed + 1, 0.3)
    go = seeded_randn((B, C, T, H, W), seed + 2)
    gp = seeded_randn((B, C, T, H // 2, W // 2), seed + 3) if pool else None

    def reference(dt, calls):
        bn = _bn(C, 3, seed + 10, train=True).to(dt)
        x, w = x0.clone().to(dt).requires_grad_(True), w0.clone().to(dt).requires_grad_(True)      # (fresh leaves: .to(float32) would hand back x0 itself)
        for _ in range(calls):
            act = F.relu(bn(F.conv3d(F.pad(x, (1,) * 6, mode="replicate"), w)))
        loss = (act * go.to(dt)).sum()
        pooled = None
        if pool:
            pooled = F.max_pool3d(act, (1, 2, 2), (1, 2, 2))
            loss = loss + (pooled * gp.to(dt)).sum()
        loss.backward()
        return dict(act=act.detach(), pooled=None if pooled is None else pooled.detach(), gx=x.grad, gw=w.grad, ggamma=bn.weight.grad, gbeta=bn.bias.grad,
                    rm=bn.running_mean.clone(), rv=bn.running_var.clone(), nbt=int(bn.num_batches_tracked))
    r32, r64 = reference(torch.float32, 1), reference(torch.float64, 1)
    bars = {k: bar_from(r32[k], r64[k]) for k in ("gx", "gw", "ggamma", "gbeta")}
    print("fp32-vs-fp64 reference bars:", {k: f"{v:.2e}" for k, v in bars.items()})

    bn = _bn(C, 3, seed + 10, train=True).to(DEV)
    xs, wd = frames(x0).requires_grad_(True), w0.to(DEV).requires_grad_(True)
    out = unet_ops.conv_bn_relu(xs, wd, bn, pool=pool)
    act, pooled = out if pool else (out, None)
    loss = (act * frames(go)).sum()
    if pool:
        loss = loss + (pooled * frames(gp)).sum()
    loss.backward()
    tag = (B, T, H, W, pool, C)
    assert _relmax(unframes(act), r64["act"]) < FWD_TOL, tag
    if pool:
        assert _relmax(unframes(pooled), r64["pooled"]) < FWD_TOL, tag
        assert torch.equal(unframes(pooled), F.max_pool3d(unframes(act), (1, 2, 2), (1, 2, 2)))
    assert _relmax(unframes(xs.grad), r64["gx"]) < bars["gx"], tag
    assert _relmax(wd.grad.cpu(), r64["gw"]) < bars["gw"], tag
    assert _relmax(bn.weight.grad.cpu(), r64["ggamma"]) < bars["ggamma"], tag
    assert _relmax(bn.bias.grad.cpu(), r64["gbeta"]) < bars["gbeta"], tag
    assert _relmax(bn.running_mean.cpu(), r64["rm"]) < FWD_TOL and _relmax(bn.running_var.cpu(), r64["rv"]) < FWD_TOL, tag
    assert int(bn.num_batches_tracked) == r64["nbt"] == 1
    with torch.no_grad():
        for _ in range(2):
            unet_ops.conv_bn_relu(xs, wd, bn, pool=pool)
    r3 = reference(torch.float64, 3)
    assert _relmax(bn.running_mean.cpu(), r3["rm"]) < FWD_TOL and _relmax(bn.running_var.cpu(), r3["rv"]) < FWD_TOL, tag
    assert int(bn.num_batches_tracked) == r3["nbt"] == 3


@pytest.mark.parametrize("C", [4, 24])
def test_batch_statistics_of_an_off_centre_output(vpx, C):
    """Convolution outputs whose channel means are up to ~65 standard deviations from 0 (inputs around 30), over 1800 pixels = 8
    workgroups: mean, 1/std, activation and running statistics against fp64. E[y^2] - mean^2 from fp32 sums loses 3e-4 to 6e-4 of the
    variance here (torch's own fp32 sums, on the CPU); the fp32 reference's activation is within 1.1e-5 of fp64."""
    from vp_suite_amd import unet_ops
    seed = name_seed(f"bn.offset.{C}")
    x0 = 30.0 + seeded_randn((2, 3, 3, 10, 30), seed)
    w0 = seeded_randn((C, 3, 3, 3, 3), seed + 1, 0.3)
    bn64 = torch.nn.BatchNorm3d(C).double().train()
    raw = F.conv3d(F.pad(x0.double(), (1,) * 6, mode="replicate"), w0.double())
    ref = F.relu(bn64(raw)).detach()
    mean, var = raw.mean((0, 2, 3, 4)), raw.var((0, 2, 3, 4), unbiased=False)
    assert float((mean.abs() / var.sqrt()).max()) > 50
    bn = torch.nn.BatchNorm3d(C).to(DEV).train()
    xs, wd = frames(x0), w0.to(DEV)
    with torch.no_grad():
        _, stats = unet_ops._RConvStatsFn.apply(xs, None, wd, unet_ops._desc(xs, None, wd, vpx._lib.RCONV_REPLICATE, "test"), None, None, False)
        act = unet_ops.conv_bn_relu(xs, wd, bn)
    assert _relmax(stats[0].cpu(), mean) < FWD_TOL
    assert float(((stats[1].cpu().double() - 1.0 / (var + 1e-5).sqrt()) * (var + 1e-5).sqrt()).abs().max()) < FWD_TOL      # per channel: each 1/std on its own scale
    assert _relmax(unframes(act), ref) < FWD_TOL
    assert _relmax(bn.running_mean.cpu(), bn64.running_mean) < FWD_TOL and _relmax(bn.running_var.cpu(), bn64.running_var) < FWD_TOL


def _tie_case(dt, C=4):
    """A [2,C,2,4,6] map of three values only (-1, 0.5, 2), so most 2x2 windows hold equal maxima; in every channel the first frame's top
    windows are: four equal live values, four equal dead ones, and a tie between the second and third element. BatchNorm (batch
    statistics) + ReLU + pool in torch, with a gradient of its own on every activation and pooled element."""
    seed = name_seed("bn.ties")
    x = torch.tensor([-1.0, 0.5, 2.0])[(seeded_rand((2, C, 2, 4, 6), seed) * 3).long().clamp(0, 2)]
    x[:, :, 0, :2, 0:2] = 2.0
    x[:, :, 0, :2, 2:4] = -1.0
    x[:, :, 0, :2, 4:6] = torch.tensor([[0.5, 2.0], [2.0, 0.5]])
    x = x.to(dt).requires_grad_(True)
    gamma = (1.0 + seeded_randn((C,), seed + 1, 0.1)).to(dt).requires_grad_(True)
    beta = seeded_randn((C,), seed + 2, 0.1).to(dt).requires_grad_(True)
    go, gp = seeded_randn(x.shape, seed + 3).to(dt), seeded_randn((2, C, 2, 2, 3), seed + 4).to(dt)
    act = F.relu(F.batch_norm(x, None, None, gamma, beta, training=True, eps=1e-5))
    pooled = F.max_pool3d(act, (1, 2, 2), (1, 2, 2))
    ((act * go).sum() + (pooled * gp).sum()).backward()
    return dict(x=x.detach(), gamma=gamma.detach(), beta=beta.detach(), go=go, gp=gp, act=act.detach(), pooled=pooled.detach(),
                gx=x.grad, ggamma=gamma.grad, gbeta=beta.grad)


def test_pool_gradient_goes_to_the_first_maximum(vpx):
    """Windows of equal activations: the pooled gradient goes to the window's first maximum in row-major order and is then gated by
    ReLU' (zero at 0), as torch's max_pool3d + relu backward do. The library's data gradient (the apply pass) and dgamma / dbeta (the
    reduce pass) against torch autograd on the same input; every element has a gradient of its own, so a gradient routed to another
    of the equal maxima shows in the data gradient by the size of the pooled gradient itself."""
    from vp_suite_amd import unet_ops
    r32, r64 = _tie_case(torch.float32), _tie_case(torch.float64)
    bars = {k: bar_from(r32[k], r64[k]) for k in ("gx", "ggamma", "gbeta")}
    print("fp32-vs-fp64 reference bars:", {k: f"{v:.2e}" for k, v in bars.items()})
    win = r64["act"][:, :, 0, :2]
    assert bool((win[..., 0:2].flatten(2).min(2).values > 0).any())            # four equal live maxima
    assert bool((win[..., 2:4].flatten(2).max(2).values == 0).all())           # four dead values
    assert bool(((win[..., 0, 5] == win[..., 1, 4]) & (win[..., 0, 5] > win[..., 0, 4])).any())     # a live tie that does not start the window
    # had the gradient gone to the LAST of the equal maxima instead, the data gradient would be off by far more than any bar
    live = win[..., 0, 0] > 0
    d = torch.where(live, r64["gp"][:, :, 0, 0, 0] * r64["gamma"].view(1, -1), torch.zeros(()).double())
    assert float(d.abs().max()) > 0.1 * float(r64["gx"].abs().max())

    xm = r64["x"].double()
    mean, var = xm.mean((0, 2, 3, 4)), xm.var((0, 2, 3, 4), unbiased=False)
    stats = torch.stack([mean, 1.0 / (var + 1e-5).sqrt()]).float().to(DEV)
    x = frames(r32["x"]).requires_grad_(True)
    gamma, beta = r32["gamma"].to(DEV).requires_grad_(True), r32["beta"].to(DEV).requires_grad_(True)
    act, pooled = unet_ops.bn_relu(x, stats, gamma, beta, pool=True)
    assert _relmax(unframes(act), r64["act"]) < FWD_TOL and _relmax(unframes(pooled), r64["pooled"]) < FWD_TOL
    ((act * frames(r32["go"])).sum() + (pooled * frames(r32["gp"])).sum()).backward()
    assert _relmax(unframes(x.grad), r64["gx"]) < bars["gx"]
    assert _relmax(gamma.grad.cpu(), r64["ggamma"]) < bars["ggamma"]
    assert _relmax(beta.grad.cpu(), r64["gbeta"]) < bars["gbeta"]
    # the pooled gradient alone (no gradient on the activation): the other input form of both backward passes
    x2 = frames(r32["x"]).requires_grad_(True)
    _, pooled2 = unet_ops.bn_relu(x2, stats, gamma.detach(), beta.detach(), pool=True)
    (pooled2 * frames(r32["gp"])).sum().backward()
    xr = r64["x"].clone().requires_grad_(True)
    (F.max_pool3d(F.relu(F.batch_norm(xr, None, None, r64["gamma"], r64["beta"], training=True, eps=1e-5)), (1, 2, 2), (1, 2, 2)) * r64["gp"]).sum().backward()
    assert _relmax(unframes(x2.grad), xr.grad) < bars["gx"]


def test_pool_and_relu_pass_nan_on(vpx):
    """A NaN in a window reaches the pooled map and the activation, as through torch's relu and max_pool3d."""
    from vp_suite_amd import unet_ops
    x = seeded_randn((1, 4, 1, 4, 6), name_seed("bn.nan"))
    x[0, 1, 0, 0, 0] = x[0, 2, 0, 1, 3] = x[0, 3, 0, 3, 4] = float("nan")       # first, last and an inner element of a window
    ref = F.max_pool3d(F.relu(x), (1, 2, 2), (1, 2, 2))
    assert int(ref.isnan().sum()) == 3
    with torch.no_grad():
        got = unet_ops.max_pool_2x2(frames(F.relu(x)))
        assert torch.equal(unframes(got).isnan(), ref.isnan()) and torch.equal(unframes(got).nan_to_num(7.0), ref.nan_to_num(7.0))
        stats = torch.tensor([[0.0] * 4, [1.0] * 4], device=DEV)
        act, pooled = unet_ops.bn_relu(frames(x), stats, torch.ones(4, device=DEV), torch.zeros(4, device=DEV), pool=True)
    assert torch.equal(unframes(act).isnan(), x.isnan()) and torch.equal(unframes(pooled).isnan(), ref.isnan())


# ---- time collapse -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 24])
@pytest.mark.parametrize("T", [2, 4])
def test_time_collapse_vs_torch(vpx, T, C):
    from vp_suite_amd import unet_ops
    for (H, W) in ((1, 1), (5, 7), (18, 34)):
        seed = name_seed(f"collapse.{T}.{C}.{H}.{W}")
        x = seeded_randn((2, C, T, H, W), seed).double().requires_grad_(True)
        w = seeded_randn((C, C, T, 1, 1), seed + 1, 0.3).double().requires_grad_(True)
        bias = seeded_randn((C,), seed + 2).double().requires_grad_(True)
        go = seeded_randn((2, C, 1, H, W), seed + 3).double()
        ref = F.conv3d(x, w, bias)
        ref.backward(go)
        xs = frames(x.detach()).requires_grad_(True)
        wd, bd = w.detach().float().to(DEV).requires_grad_(True), bias.detach().float().to(DEV).requires_grad_(True)
        y = unet_ops.time_collapse(xs, wd, bd)
        assert tuple(y.shape) == (2, 1, H, W, C)
        y.backward(frames(go))
        assert _relmax(unframes(y), ref.detach()) < FWD_TOL
        assert _relmax(unframes(xs.grad), x.grad) < GRAD_TOL
        assert _relmax(wd.grad.cpu(), w.grad) < GRAD_TOL
        assert _relmax(bd.grad.cpu(), bias.grad) < GRAD_TOL


# ---- blocks and model against the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["dc3", "dc2"])
def test_double_conv_blocks_vs_golden(vpx, tag):
    from vp_suite_amd.model_blocks import DoubleConv2d, DoubleConv3d
    g, case = load_golden("unet3d_blocks"), UNET_BLOCKS[tag]
    blk = (DoubleConv3d if case["dims"] == 3 else DoubleConv2d)(case["ci"], case["co"])
    unet3d_fill_(blk, name_seed(f"unet3d.{tag}"))
    x = seeded_randn(case["shape"], name_seed(f"unet3d.{tag}.x"))
    assert abs(checksum(x) - float(g[f"{tag}.chk_x"])) < 1e-6

    def ref_grads(dt):      # the restatement's gradients in dt, for the bars
        sd = {k: (v.detach().clone().to(dt).requires_grad_("running" not in k) if torch.is_floating_point(v) else v.clone()) for k, v in blk.state_dict().items()}
        xg = x.clone().to(dt).requires_grad_(True)
        out = unet3d_ref.double_conv(sd, "", xg, True)
        (out * seeded_randn(out.shape, name_seed(f"unet3d.{tag}.go")).to(dt)).sum().backward()
        return {**{k: v.grad for k, v in sd.items() if v.requires_grad}, "__x__": xg.grad}
    g32, g64 = ref_grads(torch.float32), ref_grads(torch.float64)
    bars = {k: bar_from(g32[k], g64[k]) for k in g64}
    print("fp32-vs-fp64 reference bars:", {k: f"{v:.2e}" for k, v in bars.items()})

    blk = blk.to(DEV).eval()
    with torch.no_grad():
        assert _relmax(unframes(blk(frames(x)), case["dims"]), g[f"{tag}.eval"]) < FWD_TOL
    blk.train()
    xs = frames(x).requires_grad_(True)
    out = blk(xs)
    go = seeded_randn(g[f"{tag}.train"].shape, name_seed(f"unet3d.{tag}.go"))
    out.backward(frames(go))
    assert _relmax(unframes(out, case["dims"]), g[f"{tag}.train"]) < FWD_TOL
    assert _relmax(unframes(xs.grad, case["dims"]), g[f"{tag}.g.__x__"]) < bars["__x__"]
    for n, p in blk.named_parameters():
        assert _relmax(p.grad.cpu(), g[f"{tag}.g.{n}"]) < bars[n], n
    for k, v in buffers_of(blk.state_dict()).items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(g[f"{tag}.buf.{k}"]) == 1
        else:
            assert _relmax(v.cpu(), g[f"{tag}.buf.{k}"]) < FWD_TOL, k


def _model(kw, seed_name, train=False):
    from vp_suite_amd.models import MODEL_CLASSES
    model = MODEL_CLASSES["unet-3d"](DEV, **kw)
    unet3d_fill_(model, name_seed(seed_name))
    return model.train(train)


def test_unet3d_tiny_eval_vs_golden(vpx):
    g = load_golden("unet3d_tiny")
    model = _model(UNET_TINY_KW, "unet3d.tiny")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    x = tiny_inputs().to(DEV)
    with torch.no_grad():
        pred, ml = model(x, pred_frames=UNET_TINY_PRED)
        assert ml is None and tuple(pred.shape) == (UNET_TINY_B, UNET_TINY_PRED, 1, 16, 24)
        assert _relmax(pred.cpu(), g["eval"]) < FWD_TOL
        assert _relmax(model.pred_1(x).cpu(), g["pred1"]) < FWD_TOL
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())      # eval() touches no buffer


def test_unet3d_tiny3_eval_vs_golden(vpx):
    g = load_golden("unet3d_tiny3")
    model = _model(UNET_TINY3_KW, "unet3d.tiny3")
    c, h, w = UNET_TINY3_KW["img_shape"]
    x = seeded_rand((UNET_TINY_B, UNET_TINY_CTX, c, h, w), name_seed("unet3d.tiny3.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-6
    with torch.no_grad():
        pred, _ = model(x.to(DEV), pred_frames=UNET_TINY_PRED)
    assert _relmax(pred.cpu(), g["eval"]) < FWD_TOL


def test_unet3d_default_eval_vs_golden(vpx):
    g = load_golden("unet3d_default")
    model = _model(UNET_DEFAULT_KW, "unet3d.default")
    x = seeded_rand((UNET_DEFAULT_B, UNET_DEFAULT_CTX, 1, 64, 64), name_seed("unet3d.default.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-6
    with torch.no_grad():
        pred, _ = model(x.to(DEV), pred_frames=UNET_DEFAULT_PRED)
    pred = pred.cpu()
    scale = float(g["pred_absmax"])
    for oy, ox in UNET_DEFAULT_SLICES:
        ref = g[f"pred_slice_{oy}{ox}"]
        _relmax(pred[:, :, :, oy::4, ox::4], ref)
        assert float((pred[:, :, :, oy::4, ox::4] - torch.from_numpy(ref)).abs().max()) < FWD_TOL * scale, (oy, ox)
    # the checksum is a cosine-weighted sum over every element: a per-element error of FWD_TOL * scale moves it by at most numel times that
    assert abs(checksum(pred) - float(g["pred_chk"])) < FWD_TOL * scale * pred.numel()


def test_unet3d_tiny_training_vs_golden(vpx):
    """Training-mode forward (batch statistics), loss sum(pred^2), every parameter gradient and every BatchNorm buffer against the
    reference; the gradient bars are measured from the restatement (module docstring)."""
    g = load_golden("unet3d_tiny")
    model = _model(UNET_TINY_KW, "unet3d.tiny", train=True)
    x = tiny_inputs()

    def ref_grads(dt):
        sd = {k: (v.detach().cpu().clone().to(dt).requires_grad_("running" not in k) if torch.is_floating_point(v) else v.cpu().clone())
              for k, v in model.state_dict().items()}
        pred, _ = unet3d_ref.forward(sd, x.to(dt), UNET_TINY_PRED, training=True)
        (pred * pred).sum().backward()
        return {k: v.grad for k, v in sd.items() if v.requires_grad}
    g32, g64 = ref_grads(torch.float32), ref_grads(torch.float64)
    zero = {k for k in g64 if k.endswith(".bias") and (k.startswith("time3ds.") or (k.startswith("ups.") and k.count(".") == 2))}
    bars = {k: bar_from(g32[k], g64[k]) for k in g64 if k not in zero}
    print("fp32-vs-fp64 reference bars, worst:", max(bars.values()))

    eval_model = _model(UNET_TINY_KW, "unet3d.tiny")
    with torch.no_grad():
        eval_pred, _ = eval_model(x.to(DEV), pred_frames=UNET_TINY_PRED)
    pred, ml = model(x.to(DEV), pred_frames=UNET_TINY_PRED)
    assert ml is None
    assert _relmax(pred.detach().cpu(), g["train.frames"]) < FWD_TOL
    assert float((pred.detach() - eval_pred).abs().max()) > 1e-2 * float(eval_pred.abs().max())      # train() is not eval()
    (pred * pred).sum().backward()
    table = fixture_grads(g, "train")
    assert sorted(table) == sorted(n for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        stats, kept = table[n]
        got = p.grad.detach().cpu().double().numpy().reshape(-1)
        if n in zero:       # exact gradient 0 (the BatchNorm behind it removes a constant): noise relative to the layer's weight gradient
            wmax = float(g64[n[:-4] + "weight"].abs().max())
            assert np.abs(got).max() <= GRAD_TOL * wmax, n
            continue
        assert _relmax(got, g64[n].numpy().reshape(-1)) < bars[n], n
        assert np.abs(grad_kept(got) - kept).max() <= bars[n] * stats[2], n
    for k, v in buffers_of(model.state_dict()).items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(g["buf." + k]) == UNET_TINY_PRED
        else:
            assert _relmax(v.cpu(), g["buf." + k]) < FWD_TOL, k


def test_unet3d_training_is_bit_reproducible(vpx):
    """Two identical training forwards + backwards under deterministic mode: frames, gradients and buffers bit-identical."""
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            model = _model(UNET_TINY_KW, "unet3d.tiny", train=True)
            pred, _ = model(tiny_inputs().to(DEV), pred_frames=2)
            (pred * pred).sum().backward()
            runs.append([pred.detach().clone()] + [p.grad.clone() for p in model.parameters()] + [v.clone() for v in buffers_of(model.state_dict()).values()])
        assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))
    finally:
        torch.use_deterministic_algorithms(prev)
