"""csrc/measure.hip on the GPU: per-frame pixel sums and SSIM with their gradients against the fp64 restatements of
tests/measure_ref.py, bit-reproducibility, and the two providers built on them.

Bounds. Pixel measures: 1e-6 relative on values, 1e-6 max-normalised on gradients (the bars of test_mse_loss_kernel_vs_oracle).
SSIM values: 1e-5 absolute (BLOCK_TOL on the measure's range of 1; near-zero SSIM values make a relative bar meaningless).
SSIM gradients: the fp32 torch restatement itself misses GRAD_TOL = 5e-5 against fp64 on smooth inputs (E[xx] - mu^2 cancels and
1 / C2 amplifies what is left), so each case measures that reference-side error on the CPU and holds the kernel to
max(GRAD_TOL, 4 x it) — 4 for an equally valid fp32 summation order (separable passes, fma contraction) — and a derived bound
above SSIM_GRAD_CEILING fails the case instead of being used: a dropped halo column, an unnormalised window or a tile-seam
off-by-one moves the gradient by 1e-2 or more."""
import functools

import pytest
import torch

import golden_cases as gc
import measure_ref
from golden_util import name_seed

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-6
PIXEL_GRAD_TOL = 1e-6
BLOCK_TOL = 1e-5
GRAD_TOL = 5e-5
SSIM_GRAD_CEILING = 5e-4


def _to_layout(t, channels_last):
    from vp_suite_amd import ops
    return ops.to_channels_last(t) if channels_last else t


# ---- pixel measures ----------------------------------------------------------------------------------------------------------------
PIXEL_SHAPES = [((3, 4, 1, 16, 16), False), ((2, 3, 3, 9, 7), True), ((1, 1, 1, 1, 1), False), ((4, 10, 1, 64, 64), False)]


@functools.lru_cache(maxsize=None)
def _pixel_case(shape):
    """(pred, target, coefficients, fp64 table, fp64 gradient of the coefficient mix) — |d| up to 2.6, a few d = 0 exactly."""
    g = torch.Generator().manual_seed(name_seed("measures.pixel" + str(shape)))
    pred, target = torch.rand(shape, generator=g) * 2.6 - 1.3, torch.rand(shape, generator=g) * 2.6 - 1.3
    if pred[0, 0].numel() > 4:
        pred[:, :, 0, 0, :3] = target[:, :, 0, 0, :3]
    coef = torch.rand(4, generator=g, dtype=torch.float64) + 0.5
    p64 = pred.double().requires_grad_(True)
    table = measure_ref.frame_sums(p64, target)
    _mix(table, coef, pred[0, 0].numel()).backward()
    return pred, target, coef, table.detach(), p64.grad


def _mix(table, coef, frame_elems):
    """coef . (mse, l1, smooth_l1, psnr) from a [3,B,T] table, each with the reference's reduction."""
    terms = [table[0], table[1], table[2], 10 * torch.log10(table[0] / frame_elems)]
    return sum(c * t.mean(dim=1).mean(dim=0) for c, t in zip(coef.to(table.dtype).to(table.device), terms))


@pytest.mark.parametrize("shape,channels_last", PIXEL_SHAPES)
def test_pixel_measures_vs_fp64(vpx, parity_log, shape, channels_last):
    from vp_suite_amd import ops
    pred, target, coef, table64, grad64 = _pixel_case(shape)
    p = _to_layout(pred.cuda(), channels_last).requires_grad_(True)
    if channels_last:
        assert not p.is_contiguous() and p[0, 0].numel() % 4 != 0   # odd frame length: every frame but the first starts unaligned
    table = ops.pixel_measures(p, target.cuda())
    assert table.shape == (3, *shape[:2]) and table.dtype == torch.float64
    err = ((table.detach().cpu().double() - table64).abs() / table64.abs()).max()
    parity_log("pixel.table", table, table64, VALUE_TOL)
    assert err < VALUE_TOL, err
    _mix(table, coef, pred[0, 0].numel()).backward()
    assert p.grad.stride() == p.stride()
    e = parity_log("pixel.grad", p.grad, grad64, PIXEL_GRAD_TOL)
    assert e < PIXEL_GRAD_TOL, e
    zero = (pred == target)
    assert torch.equal(p.grad.cpu()[zero], torch.zeros(int(zero.sum())))   # sign(0) = 0: d = 0 gets no gradient from any term


def test_pixel_measure_classes_and_identical_frames(vpx):
    from vp_suite_amd import measure as M
    pred, target, _, _, _ = _pixel_case((3, 4, 1, 16, 16))
    ref = measure_ref.measures(pred, target, keys=("mse", "l1", "smooth_l1", "psnr"))
    for key, want in ref.items():
        got = float(M.LOSS_CLASSES[key]("cuda")(pred.cuda(), target.cuda()))
        assert abs(got - float(want)) < VALUE_TOL * abs(float(want)), key
    same = pred.cuda()
    table = vpx.ops.pixel_measures(same, same.clone())
    assert torch.equal(table, torch.zeros_like(table))
    assert float(M.PSNR("cuda")(same, same.clone())) == -float("inf")   # as in the reference; forward value only


# ---- SSIM --------------------------------------------------------------------------------------------------------------------------
SSIM_SHAPES = [(1, 3, 3, 11, 11), (1, 2, 3, 12, 29), (2, 1, 3, 37, 45), (1, 1, 3, 64, 64)]   # 37x45, 64x64: several 16x32 tiles, ragged last ones
SSIM_KINDS = ["noise", "smooth", "mnist"]


@functools.lru_cache(maxsize=None)
def _ssim_case(kind, shape):
    """(pred, target, cotangent, fp64 values, fp64 gradient, relmax of the fp32 restatement's gradient against it)."""
    seed = name_seed(f"measures.ssim.{kind}{shape}")
    pred, target = measure_ref.ssim_inputs(kind, shape, seed)
    pred[0, 0, :, 1, 1], pred[0, 0, :, 5, 7] = 1.0, -1.0      # exactly on the clamp bounds: inside, by torch's rule
    pred[0, 0, :, 2, 3], pred[0, 0, :, 7, 4] = 1.25, -1.25    # beyond them
    w = torch.rand(shape[:2], generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64) + 0.25
    out = {}
    for dt in (torch.float64, torch.float32):
        p = pred.clone().requires_grad_(True)
        s = measure_ref.ssim_frames(p, target, dt)
        (s * w.to(dt)).sum().backward()
        out[dt] = (s.detach(), p.grad.double())
    ref_err = float((out[torch.float32][1] - out[torch.float64][1]).abs().max() / out[torch.float64][1].abs().max())
    return pred, target, w, out[torch.float64][0], out[torch.float64][1], ref_err


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", SSIM_KINDS)
def test_ssim_frames_vs_fp64(vpx, parity_log, kind, shape, channels_last):
    from vp_suite_amd import ops
    pred, target, w, s64, grad64, ref_err = _ssim_case(kind, shape)
    p = _to_layout(pred.cuda(), channels_last).requires_grad_(True)
    s = ops.ssim_frames(p, target.cuda())
    assert s.shape == shape[:2]
    parity_log("ssim.value", s, s64, BLOCK_TOL)
    err = float((s.detach().cpu().double() - s64).abs().max())
    assert err < BLOCK_TOL, err
    (s * w.float().cuda()).sum().backward()
    tol = max(GRAD_TOL, 4 * ref_err)
    parity_log("ssim.grad.fp32_restatement", torch.tensor([1.0 + ref_err], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64), GRAD_TOL)   # reference-side error, as a record
    e = parity_log("ssim.grad", p.grad, grad64, tol)
    assert tol <= SSIM_GRAD_CEILING, (tol, ref_err)
    assert e < tol, (e, tol, ref_err)
    assert p.grad.stride() == p.stride()
    g = p.grad.cpu()
    assert torch.equal(g[pred.abs() > 1], torch.zeros(int((pred.abs() > 1).sum())))   # outside the clamp: exactly zero
    assert (g[0, 0, :, 1, 1] != 0).all() and (g[0, 0, :, 5, 7] != 0).all()   # pred = +-1 exactly: inside


def test_ssim_measure_class(vpx):
    from vp_suite_amd import measure as M
    pred, target, _, s64, _, _ = _ssim_case("smooth", (2, 1, 3, 37, 45))
    got = M.SSIM("cuda")(pred.cuda(), target.cuda())
    assert abs(float(got) - float(1 - s64.mean())) < BLOCK_TOL
    with pytest.raises(ValueError, match="3-channel"):
        M.SSIM("cuda")(pred.cuda()[:, :, :1], target.cuda()[:, :, :1])
    with pytest.raises(ValueError, match="3-channel"):
        vpx.ops.ssim_frames(pred.cuda()[:, :, :2].contiguous(), target.cuda()[:, :, :2].contiguous())


def test_operators_are_bit_reproducible(vpx):
    from vp_suite_amd import ops
    pred, target, _, _, _, _ = _ssim_case("noise", (2, 1, 3, 37, 45))
    runs = []
    for _ in range(2):
        p = pred.cuda().requires_grad_(True)
        table, s = ops.pixel_measures(p, target.cuda()), ops.ssim_frames(p, target.cuda())
        (table.sum() + 100 * s.sum()).backward(retain_graph=True)
        g1 = p.grad.clone()
        p.grad = None
        (table.sum() + 100 * s.sum()).backward()   # the backward is out of place: a second pass through the same graph
        assert torch.equal(g1, p.grad)
        runs.append((table.detach(), s.detach(), g1))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- providers ---------------------------------------------------------------------------------------------------------------------
SCALES = {"mse": 1, "l1": .5, "smooth_l1": .25, "psnr": .01, "ssim": 2}


@functools.lru_cache(maxsize=None)
def _provider_case():
    shape = (2, 3, 3, 20, 24)
    return measure_ref.ssim_inputs("noise", shape, name_seed("measures.provider"))


def test_loss_provider_mix_vs_fp64(vpx, parity_log):
    from vp_suite_amd.measure import PredictionLossProvider
    pred, target = _provider_case()
    p64 = pred.double().requires_grad_(True)
    ref = measure_ref.measures(p64, target)
    total64 = sum(s * ref[k] for k, s in SCALES.items())
    total64.backward()
    p = pred.cuda().requires_grad_(True)
    disp, total = PredictionLossProvider({"device": "cuda", "losses_and_scales": dict(SCALES)}).get_losses(p, target.cuda())
    total.backward()
    # pixel terms to VALUE_TOL relative each, the SSIM term to BLOCK_TOL absolute times its scale
    bound = VALUE_TOL * sum(s * abs(float(ref[k].detach())) for k, s in SCALES.items() if k != "ssim") + SCALES["ssim"] * BLOCK_TOL
    assert abs(float(total.detach()) - float(total64.detach())) < bound
    for k in SCALES:
        want = float(measure_ref.display(k, ref[k].detach()))
        assert abs(float(disp[k].detach()) - want) < (BLOCK_TOL if k == "ssim" else VALUE_TOL * abs(want)), k
    e = parity_log("provider.grad", p.grad, p64.grad, GRAD_TOL)
    assert e < GRAD_TOL, e


def test_metric_provider_horizons_vs_fp64(vpx):
    from vp_suite_amd.measure import PredictionMetricProvider
    pred, target = _provider_case()
    mp = PredictionMetricProvider({"device": "cuda", "metrics": "all"})
    every = mp.get_metrics(pred.cuda(), target.cuda(), all_frame_cnts=True)
    assert len(every) == pred.shape[1]
    def check(row, n):   # pixel measures to 2 x VALUE_TOL relative (the prefix mean is an fp32 cumsum), SSIM to BLOCK_TOL absolute
        ref = measure_ref.measures(pred[:, :n], target[:, :n], keys=tuple(mp.metrics))
        assert list(row) == [f"{k} ({'↑' if k in ('psnr', 'ssim') else '↓'})" for k in mp.metrics]
        for (label, got), k in zip(row.items(), mp.metrics):
            want = float(measure_ref.display(k, ref[k]))
            assert abs(got - want) < (BLOCK_TOL if k == "ssim" else 2 * VALUE_TOL * abs(want)), (n, k, got, want)
    for n, row in enumerate(every, start=1):
        check(row, n)
    (last,) = mp.get_metrics(pred.cuda(), target.cuda())
    check(last, pred.shape[1])
    (two,) = mp.get_metrics(pred.cuda(), target.cuda(), frames=2)
    check(two, 2)


def test_train_iter_with_a_loss_mix(vpx):
    """One train_iter of the tiny convlstm-shi with an {"mse", "l1"} mix: runs through the fused pixel passes and moves the parameters."""
    from test_gpu_models import _ef
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.train import FlatAdam
    kw, B, T, P = gc.EF_TINY_KW, 2, 3, 2
    c, h, w = kw["img_shape"]
    frames = torch.rand((B, T + P, c, h, w), generator=torch.Generator().manual_seed(3)).cuda()
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0, "l1": 1.0}})
    cfg = {"device": "cuda", "context_frames": T, "pred_frames": P, "val_rec_criterion": "mse"}
    data = {"frames": frames, "actions": torch.zeros(B, T + P - 1, 0)}
    m = _ef(vpx, "tiny", kw)
    before = torch.cat([p.detach().flatten().clone() for p in m.parameters()])
    m.train_iter(cfg, [data], FlatAdam.from_module(m, lr=1e-3), lp, epoch=0)
    after = torch.cat([p.detach().flatten() for p in m.parameters()])
    assert torch.isfinite(after).all() and (after != before).float().mean() > 0.5
