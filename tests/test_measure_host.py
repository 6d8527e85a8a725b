"""The measure package without a GPU: registry and display conventions, the reference's error cases, the host (CPU tensor) values
of the five measures against independent expressions, the horizon logic of the metric provider, and the six C entry points of
csrc/measure.hip in a dry run (argument checks, workspace contract)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import measure_ref
from test_workspace_contract import E_ARG, E_WS, OK, WS_BASE, WS_BASE_ODD, L, _fake, _ok  # noqa: F401  (L: the dry-run fixture)
from vp_suite_amd import measure as M

NCHW, NHWC = 1, 0


def _pair(shape=(2, 4, 3, 13, 15), seed=0, scale=1.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale, (torch.rand(shape, generator=g) * 2 - 1) * scale


def test_registry_and_display_conventions():
    keys = ["mse", "l1", "smooth_l1", "lpips", "ssim", "psnr", "fvd"]
    assert list(M.LOSS_CLASSES) == keys and list(M.METRIC_CLASSES) == keys
    assert list(M.AVAILABLE_LOSSES) == keys and list(M.AVAILABLE_METRICS) == keys
    for key in measure_ref.KEYS:
        cls = M.LOSS_CLASSES[key]
        assert isinstance(cls.NAME, str) and cls("cpu").device == "cpu"
        assert cls.BIGGER_IS_BETTER == (key in ("psnr", "ssim"))
    assert M.MSE.OPT_VALUE == 0 and M.L1.OPT_VALUE == 0 and M.SmoothL1.OPT_VALUE == 0
    assert M.PSNR.OPT_VALUE == float("inf") and M.SSIM.OPT_VALUE == 1
    assert M.SSIM.REFERENCE and M.MSE.REFERENCE is None
    assert M.MSE.to_display(2.0) == 2.0 and M.PSNR.to_display(-30.0) == 30.0 and M.SSIM.to_display(0.25) == 0.75
    for key in ("lpips", "fvd"):
        with pytest.raises(NotImplementedError):
            M.LOSS_CLASSES[key]("cpu")
        with pytest.raises(NotImplementedError):
            M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {key: 1.0}})
        with pytest.raises(NotImplementedError):
            M.PredictionMetricProvider({"device": "cpu", "metrics": [key]})
    assert list(M.PredictionMetricProvider({"device": "cpu", "metrics": "all"}).metrics) == list(M.IMPLEMENTED)


def test_error_cases_follow_the_reference():
    a, b = _pair()
    for key in measure_ref.KEYS:
        m = M.LOSS_CLASSES[key]("cpu")
        with pytest.raises(ValueError, match="5-D"):
            m(a[0], b[0])
    ssim = M.SSIM("cpu")
    with pytest.raises(ValueError, match="3-channel"):
        ssim(a[:, :, :1], b[:, :, :1])
    with pytest.raises(ValueError, match="11x11"):
        ssim(a[:, :, :, :10], b[:, :, :, :10])
    lp = M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"l1": 1.0, "ssim": 1.0}})
    with pytest.raises(ValueError, match="different shape"):
        lp.get_losses(a, b[:, :3])
    mp = M.PredictionMetricProvider({"device": "cpu", "metrics": "all"})
    with pytest.raises(ValueError, match="different shape"):
        mp.get_metrics(a, b[:, :3])
    with pytest.raises(ValueError, match="5-dimensional"):
        mp.get_metrics(a[0], b[0])


def test_host_pixel_measures_against_torch_functional():
    a, b = _pair()
    want = {"mse": F.mse_loss(a, b, reduction="none"), "l1": F.l1_loss(a, b, reduction="none"), "smooth_l1": F.smooth_l1_loss(a, b, reduction="none")}
    for key, crit in want.items():
        got = M.LOSS_CLASSES[key]("cpu")(a, b)
        assert torch.allclose(got, crit.sum(dim=(4, 3, 2)).mean(dim=1).mean(dim=0), rtol=1e-6), key
        assert torch.allclose(got.double(), measure_ref.measures(a, b)[key], rtol=1e-5), key
    psnr = M.PSNR("cpu")(a, b)
    assert torch.allclose(psnr, (10 * torch.log10(F.mse_loss(a, b, reduction="none").mean(dim=(-1, -2, -3)))).mean(dim=1).mean(dim=0), rtol=1e-6)
    assert M.PSNR("cpu")(a, a) == -float("inf")   # identical frames, as in the reference


def test_host_ssim_properties():
    ssim = M.SSIM("cpu")
    a, b = _pair((1, 2, 3, 17, 14), scale=1.0)
    assert abs(float(ssim(a, a))) < 1e-6                       # SSIM(x, x) = 1, returned as 1 - SSIM
    assert abs(float(ssim(a, b)) - float(ssim(b, a))) < 1e-6   # symmetric
    # one 11x11 window over constant images u, v (in [0, 1] after the mapping): variances and covariance vanish, SSIM = (2uv + C1) / (u^2 + v^2 + C1).
    # On fp64 tensors: in fp32 the window sums to 1 only within ~1e-7, which E[yy] - mu_y^2 divides by C2 = 9e-4.
    for pu, pv in ((-0.4, 0.6), (0.2, 0.2), (-1.5, 0.0)):
        u, v = min(max((pu + 1) / 2, 0.0), 1.0), min(max((pv + 1) / 2, 0.0), 1.0)
        want = (2 * u * v + 1e-4) / (u * u + v * v + 1e-4)
        x, y = torch.full((1, 1, 3, 11, 11), pu, dtype=torch.float64), torch.full((1, 1, 3, 11, 11), pv, dtype=torch.float64)
        assert abs(M.SSIM.to_display(float(ssim(x, y))) - want) < 1e-9, (pu, pv)
        assert abs(float(measure_ref.ssim_frames(x, y)) - want) < 1e-9
    # the product's host expression and the tests' restatement are written separately: they agree
    for kind in ("noise", "smooth", "mnist"):
        p, t = measure_ref.ssim_inputs(kind, (1, 2, 3, 23, 19), 7)
        assert (M.frame_ssim(p, t).double() - measure_ref.ssim_frames(p, t)).abs().max() < 1e-5, kind


def test_loss_provider_mix_on_host():
    a, b = _pair()
    scales = {"mse": 1.0, "l1": 0.5, "smooth_l1": 0.25, "psnr": 0.01, "ssim": 2.0}
    a.requires_grad_(True)
    disp, total = M.PredictionLossProvider({"device": "cpu", "losses_and_scales": scales}).get_losses(a, b)
    ref = measure_ref.measures(a.detach(), b)
    assert abs(float(total.detach()) - sum(s * float(ref[k]) for k, s in scales.items())) < 1e-5 * abs(float(total.detach()))
    for k in scales:
        assert abs(float(disp[k].detach()) - float(measure_ref.display(k, ref[k]))) < 1e-5 * max(1.0, abs(float(ref[k]))), k
    total.backward()
    assert a.grad is not None and a.grad.abs().max() > 0


@pytest.mark.parametrize("metrics", ["all", ["ssim", "mse"], ["psnr"]])
def test_horizons_equal_separate_calls(metrics):
    a, b = _pair((3, 5, 3, 12, 16))
    mp = M.PredictionMetricProvider({"device": "cpu", "metrics": metrics})
    every = mp.get_metrics(a, b, all_frame_cnts=True)
    assert len(every) == 5
    for k in range(1, 6):
        (one,) = mp.get_metrics(a[:, :k], b[:, :k])
        (cut,) = mp.get_metrics(a, b, frames=k)
        assert list(one) == list(every[k - 1]) == list(cut)
        ref = measure_ref.measures(a[:, :k], b[:, :k], keys=tuple(mp.metrics))
        for (label, v), key in zip(every[k - 1].items(), mp.metrics):
            assert label == f"{key} ({'↑' if key in ('psnr', 'ssim') else '↓'})"
            assert isinstance(v, float) and math.isclose(v, one[label], rel_tol=1e-5, abs_tol=1e-6) and math.isclose(v, cut[label], rel_tol=1e-5, abs_tol=1e-6)
            assert math.isclose(v, float(measure_ref.display(key, ref[key])), rel_tol=1e-5, abs_tol=1e-5), (k, key)
    assert len(mp.get_metrics(a, b, frames=3, all_frame_cnts=True)) == 3


class _Echo(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((), 0.5))

    def forward(self, x, pred_frames):
        return x[:, -pred_frames:] * self.w, None


@pytest.mark.parametrize("losses", [{"l1": 1.0}, {"mse": 1.0, "l1": 1.0}, None])
def test_trainer_validate_without_mse_term(losses):
    """Trainer.validate reports the MSE also when the configured losses do not contain it."""
    from vp_suite_amd.train import DataParallelTrainer as Trainer
    x, y = _pair((2, 4, 1, 6, 5))
    tr = Trainer(_Echo(), losses_and_scales=losses, device="cpu", world_size=1)
    v = tr.validate([(x, y[:, :2])], pred_frames=2)
    assert torch.allclose(v, ((0.5 * x[:, -2:] - y[:, :2]) ** 2).sum(dim=(4, 3, 2)).mean(), rtol=1e-5)


# ---- C ABI in a dry run ------------------------------------------------------------------------------------------------------------
SHAPES = [(1280, 1, 64, 64), (1280, 3, 128, 128), (1, 3, 11, 11), (6, 3, 9 + 11, 7 + 11), (1, 1, 1, 1)]


def test_entry_points_dry_run(L):
    for n, C, H, W in SHAPES:
        fe = C * H * W
        nb = L.vpx_pixel_measures_workspace_bytes(n, fe)
        assert nb > 0
        for base in (WS_BASE, WS_BASE_ODD):
            _ok(L, L.vpx_pixel_measures_fwd(_fake(1), _fake(2), n, fe, _fake(3), ctypes.c_void_p(base), nb, None), f"pixel fwd {(n, fe)}", False)
        assert L.vpx_pixel_measures_fwd(_fake(1), _fake(2), n, fe, _fake(3), ctypes.c_void_p(WS_BASE), nb - 256, None) == E_WS
        _ok(L, L.vpx_pixel_measures_bwd(_fake(1), _fake(2), _fake(3), n, fe, _fake(4), None), f"pixel bwd {(n, fe)}", False)
        if C != 3:
            continue
        nb = L.vpx_ssim_workspace_bytes(n, H, W)
        assert nb > 0
        for layout, base in ((NCHW, WS_BASE), (NHWC, WS_BASE_ODD)):
            _ok(L, L.vpx_ssim_fwd(_fake(1), _fake(2), n, 3, H, W, layout, _fake(3), ctypes.c_void_p(base), nb, None), f"ssim fwd {(n, H, W)}", False)
            _ok(L, L.vpx_ssim_bwd(_fake(1), _fake(2), _fake(3), n, 3, H, W, layout, _fake(4), None), f"ssim bwd {(n, H, W)}", False)
        assert L.vpx_ssim_fwd(_fake(1), _fake(2), n, 3, H, W, NCHW, _fake(3), ctypes.c_void_p(WS_BASE), nb - 256, None) == E_WS
        assert L.vpx_ssim_fwd(_fake(1), _fake(2), n, 3, H, W, NCHW, _fake(3), None, nb, None) == E_WS


def test_entry_points_refuse_bad_arguments(L):
    ws, nb = ctypes.c_void_p(WS_BASE), 1 << 20
    assert L.vpx_pixel_measures_workspace_bytes(0, 16) == 0 and L.vpx_pixel_measures_workspace_bytes(4, 0) == 0
    assert L.vpx_pixel_measures_fwd(None, _fake(2), 4, 16, _fake(3), ws, nb, None) == E_ARG
    assert L.vpx_pixel_measures_fwd(_fake(1), _fake(2), 4, 16, None, ws, nb, None) == E_ARG
    assert L.vpx_pixel_measures_fwd(_fake(1), _fake(2), 0, 16, _fake(3), ws, nb, None) == E_ARG
    assert L.vpx_pixel_measures_fwd(_fake(1), _fake(2), 4, 0, _fake(3), ws, nb, None) == E_ARG
    assert L.vpx_pixel_measures_bwd(_fake(1), _fake(2), None, 4, 16, _fake(4), None) == E_ARG
    assert L.vpx_pixel_measures_bwd(_fake(1), _fake(2), _fake(3), 4, 16, None, None) == E_ARG
    assert L.vpx_ssim_workspace_bytes(4, 10, 64) == 0 and L.vpx_ssim_workspace_bytes(4, 64, 10) == 0 and L.vpx_ssim_workspace_bytes(0, 64, 64) == 0
    for (C, H, W, layout), word in (((1, 64, 64, NCHW), b"3-channel"), ((3, 10, 64, NCHW), b"11x11"), ((3, 64, 10, NHWC), b"11x11"), ((3, 64, 64, 2), b"layout")):
        assert L.vpx_ssim_fwd(_fake(1), _fake(2), 4, C, H, W, layout, _fake(3), ws, nb, None) == E_ARG
        assert word in L.vpx_last_error()
        assert L.vpx_ssim_bwd(_fake(1), _fake(2), _fake(3), 4, C, H, W, layout, _fake(4), None) == E_ARG
    assert L.vpx_ssim_fwd(_fake(1), None, 4, 3, 64, 64, NCHW, _fake(3), ws, nb, None) == E_ARG
    assert L.vpx_ssim_bwd(_fake(1), _fake(2), _fake(3), 0, 3, 64, 64, NCHW, _fake(4), None) == E_ARG
    assert L.vpx_ssim_fwd(_fake(1), _fake(2), 4, 3, 64, 64, NCHW, _fake(3), ws, nb, None) == OK
