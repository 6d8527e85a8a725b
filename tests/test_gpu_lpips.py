"""csrc/lpips.hip on the GPU against the float64 restatement of tests/lpips_ref.py: the stem, the max-pool and the layer head one by
one, then the whole measure through ops.lpips_frames, the measure class, both providers and the workbench.

Bounds. Per kernel: max|got - ref| / max|ref| <= 1e-5, the project's bar for fp32 convolution outputs (the pool moves values, the
head's identical-input and repeat results are exact). End to end: per case, 4 x the max-normalised error of the plain float32 torch
chain against the float64 restatement at the same inputs and weights, measured on the CPU (lpips_ref.e2e_case) — 4 for an equally
valid fp32 summation order in each of five chained layers. Every end-to-end case prints its figures and records them through parity_log;
with VPX_LPIPS_PARITY_OUT=FILE in the environment they are also written there (how profiles/lpips_parity.json was made). Every tap on
its own, the trunk layers alone and the edges of the three kernels: tests/test_gpu_lpips_taps.py (its per-tap figures go into the same file)."""
import functools
import json
import os

import pytest
import torch

import lpips_ref

pytestmark = pytest.mark.gpu

KERNEL_TOL = 1e-5
PARITY_OUT = os.environ.get("VPX_LPIPS_PARITY_OUT")
_PARITY, _PER_TAP = {}, {}


@pytest.fixture
def registered():
    from vp_suite_amd import measure as M
    M.register_lpips_weights(lpips_ref.weights())
    yield lpips_ref.weights()
    M.clear_lpips_weights()


@functools.lru_cache(maxsize=None)
def _device_weights():
    return {k: v.cuda() for k, v in lpips_ref.weights().items()}


# ---- stem --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_case(N, H, W, kind):
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + N)
    x = torch.full((N, 3, H, W), -1.0) if kind == "constant" else (torch.rand((N, 3, H, W), generator=g) * 2 - 1) * 1.4   # beyond [-1, 1]: the clamp acts
    w = lpips_ref.weights()
    return x, lpips_ref.stem(x, w["conv1.weight"], w["conv1.bias"])


@pytest.mark.parametrize("N,H,W,kind", [(1, 11, 11, "noise"), (5, 31, 31, "noise"), (1, 35, 47, "noise"), (5, 64, 64, "noise"), (1, 31, 31, "constant"),
                                        (5, 35, 47, "constant")])
def test_stem_vs_fp64(vpx, parity_log, N, H, W, kind):
    from vp_suite_amd import ops
    x, ref = _stem_case(N, H, W, kind)
    if kind == "noise":
        assert float(x.min()) < -1.05 and float(x.max()) > 1.05
    else:   # the interior sees the normalised value of 0, the ring a zero: the border outputs differ from the interior ones
        assert not torch.allclose(ref[:, :, 0, 0], ref[:, :, ref.shape[2] // 2, ref.shape[3] // 2])
    w = _device_weights()
    y = ops.lpips_stem(x.cuda(), w["conv1.weight"], w["conv1.bias"])
    assert y.shape == (N, ref.shape[2], ref.shape[3], 64) and float(ref.max()) > 0
    e = parity_log("lpips.stem", lpips_ref.nchw(y.cpu()), ref, KERNEL_TOL)
    print(f"stem {(N, H, W, kind)}: {e:.3e}")
    assert e <= KERNEL_TOL, e


def test_stem_two_sources_are_one_batch(vpx):
    from vp_suite_amd import ops
    x, _ = _stem_case(5, 35, 47, "noise")
    w = _device_weights()
    xd = x.cuda()
    whole = ops.lpips_stem(xd, w["conv1.weight"], w["conv1.bias"])
    halves = ops.lpips_stem(xd[:2], w["conv1.weight"], w["conv1.bias"], xd[2:])
    assert torch.equal(whole, halves)


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,h,w,out", [(2, 64, 3, 3, (1, 1)), (1, 192, 7, 7, (3, 3)), (3, 5, 8, 7, (3, 3)), (2, 64, 15, 15, (7, 7))])
def test_maxpool_vs_reference(vpx, N, C, h, w, out):
    from vp_suite_amd import ops
    g = torch.Generator().manual_seed(h * 100 + w)
    x = -torch.rand((N, C, h, w), generator=g) - 0.5   # negative only: a zero-initialised maximum would show
    ref = lpips_ref.maxpool(x)
    assert ref.shape[2:] == out and float(ref.max()) < 0
    y = ops.lpips_maxpool(lpips_ref.nhwc(x).cuda())
    assert y.shape == (N, *out, C)
    assert torch.equal(lpips_ref.nchw(y.cpu()).double(), ref)   # a pool moves values


# ---- head --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_case(N, C, h, w):
    g = torch.Generator().manual_seed(C * 100 + h * 10 + w)
    fx, fy = torch.relu(torch.randn((N, C, h, w), generator=g)), torch.relu(torch.randn((N, C, h, w), generator=g))
    fx[0, :, 0, 0] = 0.0          # one all-zero feature vector on each side
    fy[-1, :, -1, -1] = 0.0
    lin = torch.randn(C, generator=g).abs()
    return fx, fy, lin, lpips_ref.head(fx, fy, lin)


@pytest.mark.parametrize("C", [64, 192, 384, 256])
@pytest.mark.parametrize("N,h,w", [(3, 1, 1), (2, 3, 5), (2, 15, 15)])
def test_head_vs_fp64(vpx, parity_log, N, C, h, w):
    from vp_suite_amd import ops
    fx, fy, lin, ref = _head_case(N, C, h, w)
    dx, dy, dl = lpips_ref.nhwc(fx).cuda(), lpips_ref.nhwc(fy).cuda(), lin.cuda()
    got = ops.lpips_head(dx, dy, dl)
    assert got.dtype == torch.float64 and got.shape == (N,) and bool(torch.isfinite(got).all())
    e = parity_log("lpips.head", got, ref, KERNEL_TOL)
    print(f"head {(N, C, h, w)}: {e:.3e}")
    assert e <= KERNEL_TOL, e
    assert torch.equal(ops.lpips_head(dx, dy, dl), got)                                  # bit-reproducible
    assert torch.equal(ops.lpips_head(dx, dx, dl).cpu(), torch.zeros(N, dtype=torch.float64))   # identical maps: exactly 0
    twice = ops.lpips_head(dx, dy, dl, table=got.clone())                                # the head ADDS into its table
    assert lpips_ref.relmax(twice, 2 * ref) <= KERNEL_TOL


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _record(case, tap=None, **figures):
    """End to end (tap None) or one tap of a geometry case (tests/test_gpu_lpips_taps.py); the file is rewritten with everything so far."""
    if tap is None:
        _PARITY[str(case)] = figures
    else:
        _PER_TAP.setdefault(str(case), {})[f"tap {tap}"] = figures
    if not PARITY_OUT:
        return
    with open(PARITY_OUT, "w") as fh:
        json.dump({"what": "ops.lpips_frames on the GPU against the float64 restatement (tests/lpips_ref.py), max|got-ref| / max|ref| over the [B,T] table; "
                           "reference_error: the plain float32 torch chain on the CPU against the same restatement; bound = margin x reference_error",
                   "margin": lpips_ref.E2E_MARGIN, "cases (B, T, H, W)": _PARITY,
                   "per_tap": {"what": "the same three figures for one tap's share of the table alone (every lin{k}.weight zeroed but the tap's), over lpips_ref.GEOMETRY_CASES; "
                                       "bound = max(margin x reference_error, floor), a bound above the ceiling fails its case",
                               "floor": lpips_ref.TAP_FLOOR, "ceiling": lpips_ref.TAP_CEILING, "tap map sizes (h, w)": {str(c): [list(m) for m in t] for c, t in lpips_ref.GEOMETRY_TAPS.items()},
                               "cases (B, T, H, W)": _PER_TAP}}, fh, indent=1)


@pytest.mark.parametrize("case", lpips_ref.E2E_CASES)
def test_lpips_frames_vs_fp64(vpx, parity_log, case):
    from vp_suite_amd import ops
    pred, target, ref, ref_err, bound = lpips_ref.e2e_case(case)
    w = _device_weights()
    p, t = pred.cuda(), target.cuda()
    got = ops.lpips_frames(p, t, w)
    assert got.shape == ref.shape and got.dtype == torch.float64
    e = parity_log("lpips.frames", got, ref, bound)
    print(f"lpips_frames {case}: kernel {e:.3e}, reference-side {ref_err:.3e}, bound {bound:.3e}")
    _record(case, kernel_error=e, reference_error=ref_err, bound=bound)
    assert torch.equal(ops.lpips_frames(p, t, w), got)                                                   # bit-reproducible
    assert torch.equal(ops.lpips_frames(p, p, w).cpu(), torch.zeros(ref.shape, dtype=torch.float64))   # pred == target: exactly 0
    assert e <= bound, (e, bound)


def test_lpips_frames_on_sliced_inputs(vpx):
    from vp_suite_amd import ops
    pred, target, ref, _, bound = lpips_ref.e2e_case((2, 3, 35, 47))
    w = _device_weights()
    wide_p, wide_t = torch.zeros(2, 4, 3, 37, 50), torch.zeros(2, 6, 3, 35, 47)
    wide_p[:, 1:, :, 2:, 3:] = pred
    wide_t[:, ::2] = target
    p, t = wide_p.cuda()[:, 1:, :, 2:, 3:], wide_t.cuda()[:, ::2]
    assert not p.is_contiguous() and not t.is_contiguous()
    assert lpips_ref.relmax(ops.lpips_frames(p, t, w), ref) <= bound


def test_grad_mode_is_refused(vpx):
    from vp_suite_amd import ops
    pred, target, _, _, _ = lpips_ref.e2e_case((1, 1, 31, 31))
    p = pred.cuda().requires_grad_()
    with pytest.raises(NotImplementedError, match="backward"):
        ops.lpips_frames(p, target.cuda(), _device_weights())
    with torch.no_grad():
        assert ops.lpips_frames(p, target.cuda(), _device_weights()).shape == (1, 1)


def test_measure_and_providers_agree_with_the_host_path(vpx, registered):
    from vp_suite_amd import measure as M
    pred, target, ref, _, bound = lpips_ref.e2e_case((2, 3, 35, 47))
    host = M.frame_lpips(pred.double(), target.double())       # the host path in float64
    assert lpips_ref.relmax(host, ref) < 1e-12
    p, t = pred.cuda(), target.cuda()
    tol = bound * float(host.max()) + 1.2e-7 * float(host.max())   # the providers hand out float32 values: one rounding on top
    value = M.LPIPS("cuda")(p, t)
    assert value.is_cuda and abs(float(value) - float(host.mean(dim=1).mean(dim=0))) <= tol
    disp, total = M.PredictionLossProvider({"device": "cuda", "losses_and_scales": {"l1": 1.0, "lpips": 0.5, "ssim": 2.0}}).get_losses(p, t)
    assert abs(float(disp["lpips"]) - float(host.mean(dim=1).mean(dim=0))) <= tol
    assert abs(float(total) - (float(disp["l1"]) + 0.5 * float(disp["lpips"]) + 2.0 * (1.0 - float(disp["ssim"])))) < 1e-5 * abs(float(total))
    with pytest.raises(NotImplementedError, match="backward"):
        M.PredictionLossProvider({"device": "cuda", "losses_and_scales": {"lpips": 1.0}}).get_losses(pred.cuda().requires_grad_(), t)
    every = M.PredictionMetricProvider({"device": "cuda", "metrics": ["mse", "lpips", "psnr", "ssim"]}).get_metrics(p, t, all_frame_cnts=True)
    assert len(every) == 3
    for n in range(1, 4):
        assert abs(every[n - 1]["lpips (↓)"] - float(host[:, :n].mean(dim=1).mean(dim=0))) <= tol, n
    with pytest.raises(ValueError, match="3-channel"):
        M.LPIPS("cuda")(p[:, :, :1], t[:, :, :1])
    with pytest.raises(ValueError, match="31x31"):
        M.LPIPS("cuda")(p[..., :30], t[..., :30])


def test_workbench_reports_lpips(vpx, registered):
    import golden_cases as gc
    tiny = {k: v for k, v in gc.EF_TINY_KW.items() if k not in ("img_shape", "action_size", "tensor_value_range")}   # those come from the dataset
    suite = vpx.VPSuite()
    digits = vpx.datasets.procedural_digits(n=10, size=12)
    suite.load_dataset("MMF", split="test", digits=digits, n_seqs=3, img_size=32, num_channels=3)
    suite.create_model("convlstm-shi", **tiny)   # (test() wants a model; the copy baseline is evaluated beside it)
    results = suite.test(metrics=["mse", "lpips"], test_batch_size=2, context_frames=3, pred_frames=3)
    (per_model,) = results.values()
    assert "CopyLastFrame" in per_model
    for horizons in per_model.values():
        assert len(horizons) == 3
        for h in horizons:
            assert list(h) == ["mse (↓)", "lpips (↓)"] and 0 <= h["lpips (↓)"] < float("inf")
    # one-channel data: the measure's ValueError, not a crash
    grey = vpx.VPSuite()
    grey.load_dataset("MMF", split="test", digits=digits, n_seqs=2, img_size=32, num_channels=1)
    grey.create_model("convlstm-shi", **tiny)
    with pytest.raises(ValueError, match="3-channel"):
        grey.test(metrics=["mse", "lpips"], context_frames=3, pred_frames=3)
