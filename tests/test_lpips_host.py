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


# ---- the per-tap geometry table and the edge cases of tests/test_gpu_lpips_taps.py: conditions on the inputs ------------------------------
def test_geometry_table_reaches_the_seams():
    assert set(lpips_ref.GEOMETRY_TAPS) == set(lpips_ref.GEOMETRY_CASES)
    assert {(31, 31), (39, 71), (67, 38), (128, 96)} <= {c[2:] for c in lpips_ref.GEOMETRY_CASES}
    sides = set()
    for case in lpips_ref.GEOMETRY_CASES:
        B, T, H, W = case
        assert B * T <= 4 and (B * T == 2 or H * W < 128 * 96), case
        stated = lpips_ref.GEOMETRY_TAPS[case]
        assert stated == lpips_ref.tap_sizes(H, W), case
        x, _ = lpips_ref.frames((1, 1, 3, H, W), seed=1)
        assert stated == tuple(tuple(f.shape[2:]) for f in lpips_ref.taps(x[0], lpips_ref.weights())), case
        sides |= set(stated[0])
    assert lpips_ref.GEOMETRY_TAPS[(2, 2, 39, 71)] == ((9, 17), (4, 8), (1, 3), (1, 3), (1, 3))
    assert lpips_ref.GEOMETRY_TAPS[(2, 2, 67, 38)] == ((16, 8), (7, 3), (3, 1), (3, 1), (3, 1))
    assert lpips_ref.GEOMETRY_TAPS[(1, 2, 128, 96)][2:] == ((7, 5),) * 3
    # around the stem's 8x8 tile: on the seam, one before, one past, two tiles + 1, and four tiles per side
    assert sides >= {7, 8, 9, 16, 17} and max(sides) > 24, sides
    assert any(h > w for (h, w), *_ in lpips_ref.GEOMETRY_TAPS.values()) and any(h < w for (h, w), *_ in lpips_ref.GEOMETRY_TAPS.values())


@pytest.mark.parametrize("case", lpips_ref.GEOMETRY_CASES)
def test_geometry_case_conditions(case):
    pred, target, ref, errs, bounds = lpips_ref.geometry_case(case)
    w = lpips_ref.weights()
    assert len(ref) == len(errs) == len(bounds) == 5
    total = 0
    for l in range(1, 6):
        table, err, bound = ref[l - 1], errs[l - 1], bounds[l - 1]
        print(f"geometry {case} tap {l}: values {float(table.min()):.3e} .. {float(table.max()):.3e}, reference-side {err:.3e}, bound {bound:.3e}")
        assert table.shape == case[:2] and table.dtype == torch.float64
        assert bool((table > 0).all()), (case, l)                       # no degenerate tap, at 1x1 maps either
        assert float(table.min()) > 1e-3 * float(table.max()), (case, l)   # every frame carries weight in the max-normalised figure
        assert 0 < err and bound == max(lpips_ref.E2E_MARGIN * err, lpips_ref.TAP_FLOOR)
        assert bound <= lpips_ref.TAP_CEILING, (case, l, bound)         # (a miss: next seed revision, lpips_ref.REJECTED_SEEDS)
        # the isolating weights give exactly this tap's table in the restatement, and nothing of another tap
        iso = lpips_ref.isolated(w, l)
        assert all(torch.equal(iso[k], w[k]) for k in w if not k.startswith("lin") or k == f"lin{l}.weight")
        assert all(not bool(iso[f"lin{k}.weight"].any()) for k in range(1, 6) if k != l)
        assert torch.equal(lpips_ref.lpips_frames(pred, target, iso), table)
        total = total + table
    assert lpips_ref.relmax(total, lpips_ref.lpips_frames(pred, target, w)) < 1e-14
    f32 = lpips_ref.tap_tables_f32(pred, target, w)
    assert torch.equal(sum(f32[1:], f32[0]), lpips_ref.lpips_frames_f32(pred, target, w))
    rev = 1 + max(lpips_ref.REJECTED_SEEDS.get(case, {-1: ""}))
    assert all(r < rev for r in lpips_ref.REJECTED_SEEDS.get(case, {}))


def test_split_float32_chain_keeps_the_end_to_end_figures():
    """profiles/lpips_parity.json's reference-side errors were measured with the unsplit chain: the split one gives the same numbers."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lpips_parity.json")) as fh:
        rec = json.load(fh)["cases (B, T, H, W)"]
    for case in lpips_ref.E2E_CASES:
        assert lpips_ref.e2e_case(case)[3] == pytest.approx(rec[str(case)]["reference_error"], rel=1e-9), case


def test_trunk_layer_cases():
    """The 20 (layer, map) cases: the ReLU is at work, some outputs are clearly off, and none of them is a case of tests/glue_ref.py."""
    import glue_ref
    ours = set()
    for layer, (Ci, Co, k, pad) in enumerate(lpips_ref.TRUNK_LAYERS):
        assert lpips_ref.CONV_SHAPES[layer + 1] == (Co, Ci, k, k) and lpips_ref.STRIDE_PAD[layer + 1] == (1, pad)
        for h, w in lpips_ref.TRUNK_MAPS:
            x, wt, b, pre = lpips_ref.trunk_case(layer, h, w)
            assert x.shape == (lpips_ref.TRUNK_N, Ci, h, w) and float(x.min()) >= 0 and pre.shape == (lpips_ref.TRUNK_N, Co, h, w)
            scale = float(pre.clamp_min(0).max())
            off = float((pre < -lpips_ref.TRUNK_TOL * scale).double().mean())
            assert scale > 0 and 0.2 < off < 0.8, (layer, h, w, off)
            ours.add((0, lpips_ref.TRUNK_N, Ci, Co, k, k, 1, pad, 0, 0, h, w))
    assert {m for c in lpips_ref.GEOMETRY_TAPS.values() for m in c[2:]} <= set(lpips_ref.TRUNK_MAPS)
    theirs = {tuple(c) for t in glue_ref.TABLES.values() for c in t}
    assert not {c[2:8] for c in ours} & {c[2:8] for c in theirs}     # no (Ci, Co, kh, kw, s, p) of the trunk is in the glue tables at any map


def test_edge_case_conditions():
    for H, W in lpips_ref.STEM_EDGE_SIZES:
        for kind in lpips_ref.STEM_EDGE_KINDS:
            x, ref = lpips_ref.stem_edge_case(2, H, W, kind)
            assert ref.shape[2:] == lpips_ref.tap_sizes(H, W)[0] and float(ref.max()) > 0
            if kind == "noise":
                assert float(x.min()) < -1.05 and float(x.max()) > 1.05
                assert all(bool((x[:, :, y, xx] == v).all()) for y, xx, v in lpips_ref.STEM_PINNED)
            elif kind == "bounds":
                assert set(x.unique().tolist()) == {-1.0, 1.0}
            else:
                assert set(x.unique().tolist()) == {-1.0}
    for C in lpips_ref.HEAD_EDGE_C:
        for h, w in lpips_ref.HEAD_EDGE_MAPS:
            fx, fy, lin, ref = lpips_ref.head_edge_case(C, h, w)
            assert ref.shape == (lpips_ref.HEAD_EDGE_N,) and float(ref.max()) > 0, (C, h, w)
            assert bool((fx.pow(2).sum(dim=1) == 0).any()) and bool((fy.pow(2).sum(dim=1) == 0).any()) or C == 1, (C, h, w)
    assert sorted(h * w for h, w in lpips_ref.HEAD_EDGE_MAPS) == [1, 63, 64, 65, 129]
    for scale, C, h, w in lpips_ref.HEAD_SCALED:
        fx, fy, lin, ref = lpips_ref.head_edge_case(C, h, w, scale)
        assert bool(torch.isfinite(fx).all()) and bool(torch.isfinite(ref).all()) and float(ref.min()) > 0
        norms = fx.double().pow(2).sum(dim=1).sqrt()
        if scale < 1:   # the 1e-10 of the norm dominates: the value is far below the unscaled one
            assert float(norms.max()) < 1e-10 and float(ref.max()) < 0.1 * float(lpips_ref.head_edge_case(C, h, w)[3].max())
        else:           # the squares leave the fp32 range
            assert float(fx.max()) ** 2 > 3.5e38 and not bool(torch.isfinite(fx.pow(2).sum(dim=1)).all())
            assert lpips_ref.relmax(ref, lpips_ref.head_edge_case(C, h, w)[3]) < 1e-6   # (and in float64 the value is the unscaled one)


def test_new_shapes_dry_run(L):
    params = (ctypes.c_void_p * 15)(*[0x200000000000 + i * (1 << 30) for i in range(15)])
    for B, T, H, W in lpips_ref.GEOMETRY_CASES:
        nb = L.vpx_lpips_workspace_bytes(B * T, H, W)
        assert nb > 0
        for base in (WS_BASE, WS_BASE_ODD):
            _ok(L, L.vpx_lpips_fwd(_fake(1), _fake(2), B * T, 3, H, W, params, _fake(3), ctypes.c_void_p(base), nb, None), f"lpips fwd {(B, T, H, W)}", False)
        assert L.vpx_lpips_fwd(_fake(1), _fake(2), B * T, 3, H, W, params, _fake(3), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
    nb = L.vpx_lpips_stem_workspace_bytes()
    for H, W in lpips_ref.STEM_EDGE_SIZES:
        for n0, n1 in ((2, 0), (1, 0), (1, 4), (4, 1)):
            _ok(L, L.vpx_lpips_stem_fwd(_fake(1), _fake(2) if n1 else None, n0, n1, H, W, _fake(3), _fake(4), _fake(5), ctypes.c_void_p(WS_BASE_ODD), nb, None), f"stem {(n0, n1, H, W)}", False)
    assert L.vpx_lpips_stem_fwd(_fake(1), None, 1, 0, 6, 7, _fake(3), _fake(4), _fake(5), ctypes.c_void_p(WS_BASE), nb, None) == E_ARG
    assert L.vpx_lpips_stem_fwd(_fake(1), None, 1, 0, 7, 6, _fake(3), _fake(4), _fake(5), ctypes.c_void_p(WS_BASE), nb, None) == E_ARG
    for h, w in lpips_ref.POOL_EDGE_MAPS:
        for C in lpips_ref.POOL_EDGE_C:
            _ok(L, L.vpx_lpips_maxpool_fwd(_fake(1), _fake(2), 2, h, w, C, None), f"maxpool {(h, w, C)}", False)
    for C in lpips_ref.HEAD_EDGE_C:
        for h, w in lpips_ref.HEAD_EDGE_MAPS:
            nb = L.vpx_lpips_head_workspace_bytes(lpips_ref.HEAD_EDGE_N, h * w)
            _ok(L, L.vpx_lpips_head_fwd(_fake(1), _fake(2), _fake(3), lpips_ref.HEAD_EDGE_N, h * w, C, _fake(4), ctypes.c_void_p(WS_BASE_ODD), nb, None), f"head {(h * w, C)}", False)
    from vp_suite_amd._lib import ACT_RELU, PREC_F32, ConvDesc
    for Ci, Co, k, pad in lpips_ref.TRUNK_LAYERS:
        for h, w in lpips_ref.TRUNK_MAPS:
            d = ConvDesc(lpips_ref.TRUNK_N, h, w, Ci, Co, k, k, 1, pad, 0, 0.0, PREC_F32, 0, 0)
            nb = L.vpx_conv2d_act_workspace_bytes(ctypes.byref(d), ACT_RELU)
            assert nb > 0, L.vpx_last_error()
            _ok(L, L.vpx_conv2d_act_fwd(ctypes.byref(d), ACT_RELU, _fake(1), _fake(2), _fake(3), _fake(4), ctypes.c_void_p(WS_BASE_ODD), nb, None), f"trunk {(Ci, Co, k, h, w)}", False)
