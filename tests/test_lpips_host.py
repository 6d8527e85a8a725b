"""LPIPS without a GPU: the weight loader (three key layouts, one or two sources, shape refusals), registration and what returns after
clear_lpips_weights(), the host (CPU tensor) values against the float64 restatement of tests/lpips_ref.py, the reference's error cases,
the providers' table sharing and horizons, and the new C entry points of csrc/lpips.hip in a dry run."""
import ctypes
import math

import numpy as np
import pytest
import torch

import lpips_ref
from test_workspace_contract import E_ARG, E_UNSUPPORTED, E_WS, OK, WS_BASE, WS_BASE_ODD, L, _fake, _ok  # noqa: F401  (L: the dry-run fixture)
from vp_suite_amd import measure as M
from vp_suite_amd import ops

KEYS = ["mse", "l1", "smooth_l1", "lpips", "ssim", "psnr", "fvd"]


@pytest.fixture
def registered():
    M.register_lpips_weights(lpips_ref.weights())
    yield lpips_ref.weights()
    M.clear_lpips_weights()


def _torchvision_layout(w):
    return {f"features.{j}.{p}": w[f"conv{i}.{p}"] for i, j in enumerate(lpips_ref.TORCHVISION_INDEX, 1) for p in ("weight", "bias")}


def _lpips_package_layout(w):
    return {f"lin{i - 1}.model.1.weight": w[f"lin{i}.weight"].view(1, -1, 1, 1) for i in range(1, 6)}


def _stored():
    return {k: v.clone() for k, v in M.lpips_weights("cpu").items()}


# ---- weight maker ------------------------------------------------------------------------------------------------------------------
def test_weight_maker_fires_about_half_of_the_relus():
    w = lpips_ref.weights()
    x, _ = lpips_ref.frames((2, 1, 3, 64, 64), seed=3)
    for i, f in enumerate(lpips_ref.taps(x[:, 0], w), 1):
        fired = float((f > 0).double().mean())
        assert 0.35 < fired < 0.65, (i, fired)
        assert f.shape[1] == lpips_ref.CONV_SHAPES[i - 1][0]
    assert all(bool((w[f"lin{i}.weight"] >= 0).all()) for i in range(1, 6))


# ---- loader ------------------------------------------------------------------------------------------------------------------------
def test_loader_layouts_and_sources_give_equal_tensors(tmp_path):
    w = lpips_ref.weights()
    try:
        M.register_lpips_weights(w)
        canonical = _stored()
        assert list(canonical) == list(ops.LPIPS_KEYS)
        for k in ops.LPIPS_KEYS:
            assert torch.equal(canonical[k], w[k]) and canonical[k].data_ptr() != w[k].data_ptr()
        trunk, lin = _torchvision_layout(w), _lpips_package_layout(w)
        trunk["classifier.1.weight"] = torch.zeros(3)                     # keys of no layout are ignored
        np.savez(tmp_path / "trunk.npz", **{k: v.numpy() for k, v in trunk.items()})
        torch.save(lin, tmp_path / "lin.pth")
        torch.save({**trunk, **lin}, tmp_path / "all.pth")
        for args in ((trunk, lin), ({**trunk, **lin},), (str(tmp_path / "trunk.npz"), str(tmp_path / "lin.pth")), (tmp_path / "all.pth",),
                     ({**w, **{f"lin{i}.weight": w[f"lin{i}.weight"].view(1, -1, 1, 1) for i in range(1, 6)}},)):
            M.clear_lpips_weights()
            M.register_lpips_weights(*args)
            got = _stored()
            assert list(got) == list(canonical)
            for k in canonical:
                assert got[k].shape == canonical[k].shape and torch.equal(got[k], canonical[k]), k
    finally:
        M.clear_lpips_weights()


def test_loader_refuses_shapes_and_names_the_key():
    w = lpips_ref.weights()
    try:
        for key in ops.LPIPS_KEYS:
            bad = dict(w)
            bad[key] = torch.zeros(*w[key].shape[:-1], w[key].shape[-1] + 1)
            with pytest.raises(ValueError) as e:
                M.register_lpips_weights(bad)
            msg = str(e.value)
            assert repr(key) in msg and str(tuple(bad[key].shape)) in msg and str(tuple(w[key].shape)) in msg, msg
            with pytest.raises(NotImplementedError):    # nothing was stored
                M.LPIPS("cpu")
        bad = _torchvision_layout(w)
        bad["features.6.weight"] = torch.zeros(384, 192, 5, 5)
        with pytest.raises(ValueError, match=r"'features\.6\.weight'.*\(384, 192, 5, 5\).*\(384, 192, 3, 3\)"):
            M.register_lpips_weights(bad, _lpips_package_layout(w))
        bad = _lpips_package_layout(w)
        bad["lin2.model.1.weight"] = torch.zeros(1, 384, 2, 1)
        with pytest.raises(ValueError, match=r"'lin2\.model\.1\.weight'.*\(1, 384, 2, 1\).*\(384,\)"):
            M.register_lpips_weights(_torchvision_layout(w), bad)
        with pytest.raises(ValueError, match=r"lin3\.weight"):       # a missing tensor is named too
            M.register_lpips_weights({k: v for k, v in w.items() if k != "lin3.weight"})
        with pytest.raises(ValueError, match="neither"):
            M.register_lpips_weights("weights.bin")
        with pytest.raises(NotImplementedError):
            M.LPIPS("cpu")
    finally:
        M.clear_lpips_weights()


def test_registration_and_clear():
    def unavailable():
        with pytest.raises(NotImplementedError):
            M.LPIPS("cpu")
        with pytest.raises(NotImplementedError):
            M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"lpips": 1.0}})
        with pytest.raises(NotImplementedError):
            M.PredictionMetricProvider({"device": "cpu", "metrics": ["lpips"]})

    unavailable()
    M.register_lpips_weights(lpips_ref.weights())
    try:
        m = M.LPIPS("cpu")
        assert m.device == "cpu" and m.TABLE == "lpips" and not m.BIGGER_IS_BETTER and m.OPT_VALUE == 0 and m.to_display(0.25) == 0.25
        assert list(M.PredictionMetricProvider({"device": "cpu", "metrics": ["mse", "lpips", "psnr", "ssim"]}).metrics) == ["mse", "lpips", "psnr", "ssim"]
        assert "lpips" in M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"lpips": 1.0}}).losses
        # what must not change, registered or not
        assert list(M.LOSS_CLASSES) == KEYS and list(M.METRIC_CLASSES) == KEYS
        assert M.IMPLEMENTED == ("mse", "l1", "smooth_l1", "ssim", "psnr")
        assert list(M.PredictionMetricProvider({"device": "cpu", "metrics": "all"}).metrics) == list(M.IMPLEMENTED)
        with pytest.raises(NotImplementedError):
            M.FrechetVideoDistance("cpu")
    finally:
        M.clear_lpips_weights()
    unavailable()
    assert list(M.LOSS_CLASSES) == KEYS and M.IMPLEMENTED == ("mse", "l1", "smooth_l1", "ssim", "psnr")
    from vp_suite_amd import vpsuite
    assert vpsuite.DEFAULT_RUN_CONFIG["metrics"] == ["mse", "psnr", "ssim"] and "lpips" in vpsuite.__doc__


# ---- host values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lpips_ref.E2E_CASES)
def test_host_values_against_the_restatement(registered, case):
    pred, target, ref, ref_err, bound = lpips_ref.e2e_case(case)
    m = M.LPIPS("cpu")
    got64 = M.frame_lpips(pred.double(), target.double())
    assert got64.dtype == torch.float64 and got64.shape == ref.shape
    assert lpips_ref.relmax(got64, ref) < 1e-12
    assert abs(float(m(pred.double(), target.double())) - float(ref.mean(dim=1).mean(dim=0))) < 1e-12 * float(ref.max())
    got32 = M.frame_lpips(pred, target)
    print(f"host float32 {case}: reference-side error {ref_err:.3e}, bound {bound:.3e}, host path {lpips_ref.relmax(got32, ref):.3e}")
    assert got32.dtype == torch.float32 and 0 < ref_err < 1e-4    # the bound is a float32-sized number, never a loose one
    assert lpips_ref.relmax(got32, ref) <= bound
    assert bool((got64 > 0).all())


def test_host_identical_and_symmetric(registered):
    pred, target, _, _, _ = lpips_ref.e2e_case((2, 3, 35, 47))
    assert torch.equal(M.frame_lpips(pred, pred), torch.zeros(2, 3))
    a, b = M.frame_lpips(pred.double(), target.double()), M.frame_lpips(target.double(), pred.double())
    assert lpips_ref.relmax(a, b) < 1e-12
    zero = torch.full((1, 1, 3, 31, 31), -1.0)           # constant frames: finite, and 0 against themselves
    assert torch.isfinite(M.frame_lpips(zero, -zero)).all() and float(M.frame_lpips(zero, zero)) == 0.0


def test_error_cases(registered):
    m = M.LPIPS("cpu")
    a, b = lpips_ref.frames((2, 2, 3, 31, 33), seed=5)
    with pytest.raises(ValueError, match="5-D"):
        m(a[0], b[0])
    with pytest.raises(ValueError, match="different shape"):
        m(a, b[:, :1])
    with pytest.raises(ValueError, match="3-channel"):
        m(a[:, :, :1], b[:, :, :1])
    with pytest.raises(ValueError, match="31x31"):
        m(a[:, :, :, :30], b[:, :, :, :30])
    with pytest.raises(ValueError, match="31x31"):
        m(a[..., :30], b[..., :30])
    mp = M.PredictionMetricProvider({"device": "cpu", "metrics": ["mse", "lpips"]})
    with pytest.raises(ValueError, match="3-channel"):
        mp.get_metrics(a[:, :, :1], b[:, :, :1])
    for fn, args in ((ops.lpips_frames, (a, b, lpips_ref.weights())), (ops.lpips_stem, (a[0], lpips_ref.weights()["conv1.weight"], lpips_ref.weights()["conv1.bias"])),
                     (ops.lpips_maxpool, (torch.zeros(1, 3, 3, 4),)), (ops.lpips_head, (torch.zeros(1, 1, 1, 4), torch.zeros(1, 1, 1, 4), torch.ones(4)))):
        with pytest.raises(Exception, match="GPU"):      # no CPU fallback behind the ops
            fn(*args)


# ---- providers ---------------------------------------------------------------------------------------------------------------------
def test_providers_compute_each_table_once(registered, monkeypatch):
    calls = {"sums": 0, "ssim": 0, "lpips": 0}
    for name, fn in (("sums", "frame_sums"), ("ssim", "frame_ssim"), ("lpips", "frame_lpips")):
        def counted(*a, _orig=getattr(M, fn), _name=name, **kw):
            calls[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(M, fn, counted)
    pred, target, ref, _, bound = lpips_ref.e2e_case((2, 3, 35, 47))
    disp, total = M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"l1": 1.0, "lpips": 0.5, "ssim": 2.0, "smooth_l1": 1.0}}).get_losses(pred, target)
    assert calls == {"sums": 1, "ssim": 1, "lpips": 1}
    want = float(ref.mean(dim=1).mean(dim=0))
    assert abs(float(disp["lpips"]) - want) <= bound * float(ref.max()) + 1e-7 * want
    assert math.isclose(float(total), float(disp["l1"]) + 0.5 * float(disp["lpips"]) + 2.0 * (1 - float(disp["ssim"])) + float(disp["smooth_l1"]), rel_tol=1e-5)
    M.PredictionMetricProvider({"device": "cpu", "metrics": ["l1", "lpips", "ssim", "mse", "psnr"]}).get_metrics(pred, target, all_frame_cnts=True)
    assert calls == {"sums": 2, "ssim": 2, "lpips": 2}


def test_metric_provider_horizons(registered):
    pred, target, ref, _, bound = lpips_ref.e2e_case((2, 3, 35, 47))
    mp = M.PredictionMetricProvider({"device": "cpu", "metrics": ["mse", "lpips", "psnr", "ssim"]})
    every = mp.get_metrics(pred, target, all_frame_cnts=True)
    assert len(every) == 3 and list(every[0]) == ["mse (↓)", "lpips (↓)", "psnr (↑)", "ssim (↑)"]
    m = M.LPIPS("cpu")
    for n in range(1, 4):
        want = float(ref[:, :n].mean(dim=1).mean(dim=0))
        assert abs(every[n - 1]["lpips (↓)"] - want) <= bound * float(ref.max()) + 1e-7 * want
        assert math.isclose(every[n - 1]["lpips (↓)"], float(m(pred[:, :n], target[:, :n])), rel_tol=1e-5)
        (cut,) = mp.get_metrics(pred, target, frames=n)
        assert math.isclose(cut["lpips (↓)"], every[n - 1]["lpips (↓)"], rel_tol=1e-5)


# ---- C ABI in a dry run ------------------------------------------------------------------------------------------------------------
TRUNK_SHAPES = [(1, 31, 31), (6, 35, 47), (4, 64, 64), (2560, 64, 64), (3, 31, 200), (2, 128, 160), (1, 256, 256)]


def test_entry_points_dry_run(L):
    params = (ctypes.c_void_p * 15)(*[0x200000000000 + i * (1 << 30) for i in range(15)])
    for n, H, W in TRUNK_SHAPES:
        nb = L.vpx_lpips_workspace_bytes(n, H, W)
        assert nb > 0
        for base in (WS_BASE, WS_BASE_ODD):
            for det in (0, 1):
                L.vpx_set_deterministic(det)
                _ok(L, L.vpx_lpips_fwd(_fake(1), _fake(2), n, 3, H, W, params, _fake(3), ctypes.c_void_p(base), nb, None), f"lpips fwd {(n, H, W)}", False)
        L.vpx_set_deterministic(0)
        assert L.vpx_lpips_fwd(_fake(1), _fake(2), n, 3, H, W, params, _fake(3), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
        assert L.vpx_lpips_fwd(_fake(1), _fake(2), n, 3, H, W, params, _fake(3), None, nb, None) == E_WS
    nb = L.vpx_lpips_stem_workspace_bytes()
    assert nb > 3 * 121 * 64 * 4
    for n0, n1, H, W in ((1, 0, 11, 11), (5, 5, 35, 47), (2, 3, 7, 64), (1280, 1280, 64, 64)):
        for base in (WS_BASE, WS_BASE_ODD):
            _ok(L, L.vpx_lpips_stem_fwd(_fake(1), _fake(2) if n1 else None, n0, n1, H, W, _fake(3), _fake(4), _fake(5), ctypes.c_void_p(base), nb, None), f"stem {(n0, n1, H, W)}", False)
        assert L.vpx_lpips_stem_fwd(_fake(1), _fake(2), n0, n1, H, W, _fake(3), _fake(4), _fake(5), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
    for N, H, W, C in ((1, 3, 3, 64), (5, 8, 7, 192), (2560, 15, 15, 64), (1, 63, 63, 1)):
        _ok(L, L.vpx_lpips_maxpool_fwd(_fake(1), _fake(2), N, H, W, C, None), f"maxpool {(N, H, W, C)}", False)
    for n, HW, C in ((1, 1, 64), (5, 15, 192), (2560, 225, 64), (3, 3969, 384), (2, 9, 256), (1, 7, 512), (1, 7, 5)):
        nb = L.vpx_lpips_head_workspace_bytes(n, HW)
        assert nb > 0
        for base in (WS_BASE, WS_BASE_ODD):
            _ok(L, L.vpx_lpips_head_fwd(_fake(1), _fake(2), _fake(3), n, HW, C, _fake(4), ctypes.c_void_p(base), nb, None), f"head {(n, HW, C)}", False)
        assert L.vpx_lpips_head_fwd(_fake(1), _fake(2), _fake(3), n, HW, C, _fake(4), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS


def test_entry_points_refuse_bad_arguments(L):
    ws, nb = ctypes.c_void_p(WS_BASE), 1 << 30
    params = (ctypes.c_void_p * 15)(*[0x200000000000 + i * (1 << 30) for i in range(15)])
    assert L.vpx_lpips_workspace_bytes(0, 64, 64) == 0 and L.vpx_lpips_workspace_bytes(4, 30, 64) == 0 and L.vpx_lpips_workspace_bytes(4, 64, 30) == 0
    for args, word in (((None, _fake(2), 4, 3, 64, 64, params, _fake(3)), b"NULL"), ((_fake(1), None, 4, 3, 64, 64, params, _fake(3)), b"NULL"),
                       ((_fake(1), _fake(2), 4, 3, 64, 64, None, _fake(3)), b"NULL"), ((_fake(1), _fake(2), 4, 3, 64, 64, params, None), b"NULL"),
                       ((_fake(1), _fake(2), 0, 3, 64, 64, params, _fake(3)), b"n_frames"), ((_fake(1), _fake(2), 4, 1, 64, 64, params, _fake(3)), b"3-channel"),
                       ((_fake(1), _fake(2), 4, 3, 30, 64, params, _fake(3)), b"31x31"), ((_fake(1), _fake(2), 4, 3, 64, 30, params, _fake(3)), b"31x31")):
        assert L.vpx_lpips_fwd(*args, ws, nb, None) == E_ARG, args
        assert word in L.vpx_last_error()
    assert L.vpx_lpips_fwd(_fake(1), _fake(2), 4, 3, 64, 64, params, _fake(3), ws, nb, None) == OK
    snb = L.vpx_lpips_stem_workspace_bytes()
    good = [_fake(1), _fake(2), 2, 2, 35, 47, _fake(3), _fake(4), _fake(5)]
    assert L.vpx_lpips_stem_fwd(*good, ws, snb, None) == OK
    for i, v in ((0, None), (1, None), (6, None), (7, None), (8, None), (2, 0), (3, -1), (4, 6), (5, 6)):
        bad = list(good)
        bad[i] = v
        assert L.vpx_lpips_stem_fwd(*bad, ws, snb, None) == E_ARG, (i, v)
    assert L.vpx_lpips_stem_fwd(*good, None, snb, None) == E_WS
    good = [_fake(1), _fake(2), 4, 8, 7, 192]
    assert L.vpx_lpips_maxpool_fwd(*good, None) == OK
    for i, v in ((0, None), (1, None), (2, 0), (3, 2), (4, 2), (5, 0)):
        bad = list(good)
        bad[i] = v
        assert L.vpx_lpips_maxpool_fwd(*bad, None) == E_ARG, (i, v)
    assert L.vpx_lpips_head_workspace_bytes(0, 9) == 0 and L.vpx_lpips_head_workspace_bytes(4, 0) == 0
    good = [_fake(1), _fake(2), _fake(3), 4, 15, 192, _fake(4)]
    assert L.vpx_lpips_head_fwd(*good, ws, nb, None) == OK
    for i, v in ((0, None), (1, None), (2, None), (6, None), (3, 0), (4, 0), (5, 0)):
        bad = list(good)
        bad[i] = v
        assert L.vpx_lpips_head_fwd(*bad, ws, nb, None) == E_ARG, (i, v)
    bad = list(good)
    bad[5] = 513
    assert L.vpx_lpips_head_fwd(*bad, ws, nb, None) == E_UNSUPPORTED and b"512" in L.vpx_last_error()
    assert L.vpx_lpips_head_fwd(*good, None, nb, None) == E_WS
