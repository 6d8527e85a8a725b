"""FVD without a GPU: the weight loader (key parsing, widths read from the tensors, shape refusals), registration and what returns after
clear_fvd_weights(), the "SAME" padding rule, the chunk table and the host restatement against values recorded from the reference
(tools/gen_golden_fvd.py), the providers, and the C entry points of csrc/fvd.hip in a dry run."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import fvd_ref
from test_workspace_contract import E_ARG, E_UNSUPPORTED, E_WS, OK, WS_BASE, WS_BASE_ODD, L, _fake, _ok  # noqa: F401  (L: the dry-run fixture)
from vp_suite_amd import measure as M
from vp_suite_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def registered():
    M.register_fvd_weights(fvd_ref.state_dict())
    yield
    M.clear_fvd_weights()


def _golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


# ---- loader ------------------------------------------------------------------------------------------------------------------------
def test_loader_reads_the_widths_from_the_tensors(tmp_path):
    try:
        for div, ci in ((8, 3), (8, 2), (16, 3)):
            sd = fvd_ref.state_dict(div, ci)
            M.register_fvd_weights(sd)
            w = M.fvd_weights("cpu", torch.float64)
            assert list(w) == list(M.FVD_UNITS) + ["logits"] and M.fvd_in_channels() == ci
            assert w["Conv3d_1a_7x7"][0].shape == (64 // div, ci, 7, 7, 7) and w["Mixed_5c.b1b"][0].shape == (384 // div, 192 // div, 3, 3, 3)
            assert w["logits"][0].shape == (400 // div, 1024 // div) and w["logits"][1].shape == (400 // div,)
            fw, fb = fvd_ref.folded(sd, "Mixed_4b.b2a")                      # BatchNorm is folded at registration, in float64
            assert torch.equal(w["Mixed_4b.b2a"][0], fw) and torch.equal(w["Mixed_4b.b2a"][1], fb)
            assert M.fvd_weights("cpu", torch.float64) is w                  # built once per device and dtype
        sd = fvd_ref.state_dict()
        np.savez(tmp_path / "i3d.npz", **{k: v.numpy() for k, v in sd.items()})
        torch.save(dict(sd), tmp_path / "i3d.pth")
        M.register_fvd_weights(sd)
        want = M.fvd_weights("cpu", torch.float64)
        for source in (str(tmp_path / "i3d.npz"), tmp_path / "i3d.pth", {**sd, "Predictions.weight": torch.zeros(3)}):
            M.clear_fvd_weights()
            M.register_fvd_weights(source)
            got = M.fvd_weights("cpu", torch.float64)
            assert all(torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]) for k in want)
    finally:
        M.clear_fvd_weights()


def test_loader_refuses_inconsistent_shapes_and_names_the_key():
    sd = fvd_ref.state_dict()

    def refused(key, tensor, *words):
        bad = dict(sd)
        bad[key] = tensor
        with pytest.raises(ValueError) as e:
            M.register_fvd_weights(bad)
        msg = str(e.value)
        assert all(w in msg for w in words), msg
        with pytest.raises(NotImplementedError):    # nothing was stored
            M.FrechetVideoDistance("cpu")

    try:
        refused("Conv3d_1a_7x7.conv3d.weight", torch.zeros(8, 4, 7, 7, 7), "'Conv3d_1a_7x7.conv3d.weight'", "(8, 4, 7, 7, 7)", "2 or 3")
        refused("Conv3d_2b_1x1.conv3d.weight", torch.zeros(8, 9, 1, 1, 1), "'Conv3d_2b_1x1.conv3d.weight'", "(8, 9, 1, 1, 1)", "(8, 8, 1, 1, 1)", "'Conv3d_1a_7x7.conv3d.weight'", "(8, 3, 7, 7, 7)")
        refused("Conv3d_2c_3x3.conv3d.weight", torch.zeros(24, 8, 3, 3, 1), "'Conv3d_2c_3x3.conv3d.weight'", "(24, 8, 3, 3, 1)", "3, 3, 3")
        refused("Mixed_3b.b1b.conv3d.weight", torch.zeros(16, 11, 3, 3, 3), "'Mixed_3b.b1b.conv3d.weight'", "(16, 11, 3, 3, 3)", "(16, 12, 3, 3, 3)", "'Mixed_3b.b1a.conv3d.weight'")
        # a block's four branches must sum to the next block's input channels
        refused("Mixed_3c.b0.conv3d.weight", torch.zeros(16, 31, 1, 1, 1), "'Mixed_3c.b0.conv3d.weight'", "(16, 31, 1, 1, 1)", "(16, 32, 1, 1, 1)", "Mixed_3b", "8 + 16 + 4 + 4 = 32")
        refused("Mixed_4b.b3b.bn.running_var", torch.zeros(9), "'Mixed_4b.b3b.bn.running_var'", "(9,)", "(8,)")
        refused("logits.conv3d.weight", torch.zeros(50, 127, 1, 1, 1), "'logits.conv3d.weight'", "(50, 127, 1, 1, 1)", "128", "Mixed_5c")
        refused("logits.conv3d.bias", torch.zeros(49), "'logits.conv3d.bias'", "(49,)", "(50,)")
        refused("Mixed_5b.b0.bn.weight", torch.zeros(32, dtype=torch.int64), "'Mixed_5b.b0.bn.weight'", "int64")
        with pytest.raises(ValueError, match=r"'Mixed_4e\.b2b\.bn\.bias'"):   # a missing tensor is named too
            M.register_fvd_weights({k: v for k, v in sd.items() if k != "Mixed_4e.b2b.bn.bias"})
        with pytest.raises(ValueError, match="neither"):
            M.register_fvd_weights("weights.bin")
    finally:
        M.clear_fvd_weights()


def test_registration_and_clear():
    keys = ["mse", "l1", "smooth_l1", "lpips", "ssim", "psnr", "fvd"]

    def unavailable():
        with pytest.raises(NotImplementedError):
            M.FrechetVideoDistance("cpu")
        with pytest.raises(NotImplementedError):
            M.fvd_weights("cpu")
        with pytest.raises(NotImplementedError):
            M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"fvd": 1.0}})
        with pytest.raises(NotImplementedError):
            M.PredictionMetricProvider({"device": "cpu", "metrics": ["mse", "fvd"]})

    unavailable()
    M.register_fvd_weights(fvd_ref.state_dict())
    try:
        m = M.FrechetVideoDistance("cpu")
        assert m.device == "cpu" and m.TABLE is None and not m.BIGGER_IS_BETTER and m.OPT_VALUE == 0 and m.to_display(0.25) == 0.25
        assert list(M.PredictionMetricProvider({"device": "cpu", "metrics": ["mse", "fvd"]}).metrics) == ["mse", "fvd"]
        assert "fvd" in M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"fvd": 1.0}}).losses
        # what must not change, registered or not
        assert list(M.LOSS_CLASSES) == keys and list(M.METRIC_CLASSES) == keys
        assert M.IMPLEMENTED == ("mse", "l1", "smooth_l1", "ssim", "psnr")
        assert list(M.PredictionMetricProvider({"device": "cpu", "metrics": "all"}).metrics) == list(M.IMPLEMENTED)
        with pytest.raises(NotImplementedError):
            M.LPIPS("cpu")
    finally:
        M.clear_fvd_weights()
    unavailable()
    from vp_suite_amd import vpsuite
    assert vpsuite.DEFAULT_RUN_CONFIG["metrics"] == ["mse", "psnr", "ssim"]


# ---- the "SAME" rule ---------------------------------------------------------------------------------------------------------------
SAME_ROWS = {(9, 7, 2): (3, 3, 5), (16, 7, 2): (2, 3, 8), (13, 7, 2): (3, 3, 7), (12, 3, 2): (0, 1, 6), (13, 3, 2): (1, 1, 7), (7, 3, 1): (1, 1, 7),
             (7, 2, 2): (0, 1, 4), (4, 2, 2): (0, 0, 2), (1, 7, 2): (3, 3, 1), (1, 3, 1): (1, 1, 1), (5, 1, 2): (0, 0, 3), (17, 7, 1): (3, 3, 17)}


def test_same_padding_rule_against_the_table(L):
    """Sizes 1 .. 17, k in {1, 2, 3, 7}, s in {1, 2}: the package's rule and the library's against TensorFlow's statement of SAME
    (out = ceil(size / s), total padding max((out - 1) s + k - size, 0), the smaller half in front) and against rows written out by hand."""
    for size in range(1, 18):
        for k in (1, 2, 3, 7):
            for s in (1, 2):
                out = math.ceil(size / s)
                pad = max((out - 1) * s + k - size, 0)
                want = (pad // 2, pad - pad // 2, out)
                assert M.same_pad(size, k, s) == want and ops.same_padding(size, k, s) == want, (size, k, s)
                if (size, k, s) in SAME_ROWS:
                    assert want == SAME_ROWS[(size, k, s)], (size, k, s)
    front, out = ctypes.c_int(), ctypes.c_int()
    assert L.vpx_same_padding(0, 3, 1, ctypes.byref(front), ctypes.byref(out)) == E_ARG and L.vpx_same_padding(5, 3, 1, None, ctypes.byref(out)) == E_ARG


def test_written_out_rule_equals_the_package(L):
    """fvd_ref.same_rule, which the GPU edge tests build their expected maps from, against measure.same_pad and the library."""
    for size in range(1, 21):
        for k in range(1, 8):
            for s in range(1, 5):
                front, back, out = M.same_pad(size, k, s)
                assert fvd_ref.same_rule(size, k, s) == (front, out) and ops.same_padding(size, k, s) == (front, back, out), (size, k, s)


# ---- the case tables of tests/test_gpu_fvd_edges.py -----------------------------------------------------------------------------------
def _tap_by_conv(x, tap, kernel, stride, co_count=fvd_ref.TAP_CO):
    w = torch.zeros(co_count, x.shape[1], *kernel, dtype=torch.float64)
    w[tap] = 1.0
    return torch.nn.functional.conv3d(M._fvd_pad(x.double(), kernel, stride), w, stride=stride)


def _shift_by(x, tap, outs, strides, fronts):
    """x[:, ci] read at o * stride - front + d per axis, 0 outside the map: unit_tap_expected's arithmetic with the strides and front pads
    handed in, to restate what a kernel with a mistake in them would write."""
    y, keep = x[:, tap[1]], None
    for axis, (out, s, f, d) in enumerate(zip(outs, strides, fronts, tap[2:])):
        i = torch.arange(out) * s - f + d
        ok = ((i >= 0) & (i < x.shape[2 + axis])).view([-1 if a == axis else 1 for a in range(3)])
        keep = ok if keep is None else keep & ok
        y = y.index_select(1 + axis, i.clamp(0, x.shape[2 + axis] - 1))
    return torch.where(keep, y, torch.zeros(()))


def test_unit_tap_expectation_is_a_shift():
    """The index arithmetic of fvd_ref.unit_tap_expected against float64 F.conv3d with a one-hot weight (exact: one product by 1.0 per
    output), the taps' reach over the channels, and what the table can tell apart: on the forms with sh != sw the expected maps differ from
    those of a kernel that swapped the two strides, and on the forms with an odd total pad on some axis from those of one that put the
    larger half of it in front."""
    told_swap = told_front = 0
    for form in fvd_ref.EDGE_FORMS:
        kernel, stride, shape = form
        assert kernel[1] != kernel[2] and len(set(kernel)) > 1
        fronts, outs = zip(*(fvd_ref.same_rule(n, k, s) for n, k, s in zip(shape, kernel, stride)))
        pads = [sum(M.same_pad(n, k, s)[:2]) for n, k, s in zip(shape, kernel, stride)]
        swap_differs = front_differs = False
        for ci_count in (3, 4):
            taps = fvd_ref.unit_taps(kernel, ci_count)
            assert len(taps) == 9 and {t[0] for t in taps} == set(range(fvd_ref.TAP_CO)) and {t[1] for t in taps} == set(range(ci_count))
            assert all(0 <= d < k for t in taps for d, k in zip(t[2:], kernel))
            x = fvd_ref.edge_conv_case(form, ci_count, fvd_ref.TAP_CO, 2)[0]
            for tap in taps:
                want, keep = fvd_ref.unit_tap_expected(x, fvd_ref.TAP_CO, tap, kernel, stride)
                ref = _tap_by_conv(x, tap, kernel, stride)
                assert want.shape == ref.shape and torch.equal(want.double(), ref), (form, tap)
                assert int((want != 0).sum()) == 2 * int(keep.sum()) and torch.equal(_shift_by(x, tap, outs, stride, fronts), want[:, tap[0]])
                swap_differs |= not torch.equal(_shift_by(x, tap, outs, (stride[0], stride[2], stride[1]), fronts), want[:, tap[0]])
                front_differs |= not torch.equal(_shift_by(x, tap, outs, stride, [(p + 1) // 2 for p in pads]), want[:, tap[0]])
        assert front_differs == any(p % 2 for p in pads) and swap_differs == (stride[1] != stride[2]), form
        told_swap, told_front = told_swap + swap_differs, told_front + front_differs
    assert told_swap >= 2 and told_front >= 2


def test_edge_case_tables():
    for form in fvd_ref.EDGE_FORMS + fvd_ref.ADJACENT_FORMS:
        n = fvd_ref.ragged_batch(form)
        m = fvd_ref.out_positions(form, n)
        assert n in (3, 4) and m > 64 and m % 64 != 0, (form, n, m)
    assert [fvd_ref.ragged_batch(f) for f in fvd_ref.EDGE_FORMS] == [3, 3, 4, 3]     # 2x7x5 under stride (1, 3, 2) has 18 outputs: 54 at N = 3
    kernel, stride, shape = fvd_ref.EDGE_FORMS[1]
    assert shape[2] < kernel[2] and fvd_ref.same_rule(shape[2], kernel[2], stride[2]) == (3, 3)   # every column: taps before AND behind the map
    assert all(s > k for k, s in zip(*fvd_ref.EDGE_FORMS[3][:2])) and not any(s > k for k, s in zip(*fvd_ref.EDGE_FORMS[2][:2]))
    counts = {}
    for kernel, stride, shape, spots in fvd_ref.POOL_NAN_CASES:
        for what, at in spots.items():
            counts[(kernel, stride, what)] = int(fvd_ref.window_mask(shape, kernel, stride, at).sum())
    assert counts[((3, 3, 3), (3, 3, 3), "first of a window")] == counts[((3, 3, 3), (3, 3, 3), "inner")] == counts[((3, 3, 3), (3, 3, 3), "last of a window")] == 1
    assert counts[((3, 3, 3), (2, 2, 2), "shared by eight windows")] == 8 and counts[((3, 3, 3), (2, 2, 2), "shared by two")] == 2
    assert counts[((3, 3, 3), (2, 2, 2), "inner of one")] == 1 and counts[((3, 3, 3), (2, 2, 2), "in a border window that holds padding")] == 1
    assert counts[((3, 3, 3), (1, 1, 1), "shared by 27 windows")] == 27 and counts[((3, 3, 3), (1, 1, 1), "in border windows that hold padding")] == 8
    assert counts[((3, 3, 3), (1, 1, 1), "last element of the map")] == 8 and counts[((1, 3, 3), (1, 2, 2), "shared by four windows")] == 4
    assert counts[((1, 3, 3), (1, 2, 2), "last of the last window, next to padding")] == 1


def test_frechet_edge_tables_and_what_the_reference_supports():
    """The new kinds are what they claim to be, the old kinds' tables are untouched by them, and the float64 reference alone is good for
    the bound the GPU test uses: permuting the rows of both tables (the same distance) moves it by less than a tenth of frechet_bound, and
    the distance of the kinds that are not near zero by construction is more than 100 bounds away from zero."""
    g = torch.Generator().manual_seed(3000 + 17 * 8 + 7)   # "shifted" restated: the existing kinds draw as they always did
    p = torch.randn(8, 7, generator=g) * (torch.rand(1, 7, generator=g) * 2 + 0.5) + torch.randn(1, 7, generator=g)
    assert torch.equal(fvd_ref.feature_tables(8, 7, "shifted")[0], p) and fvd_ref.FRECHET_KINDS == ("shifted", "identical", "rank1")
    assert len(fvd_ref.FRECHET_EDGE_CASES) == 21 + 24
    for b, n, kind in fvd_ref.FRECHET_EDGE_CASES:
        p, t = fvd_ref.feature_tables(b, n, kind)
        assert p.dtype == t.dtype == torch.float32 and p.shape == t.shape == (b, n) and bool(torch.isfinite(p).all() and torch.isfinite(t).all())
        if kind in ("scaled_up", "scaled_down"):
            f = 2.0 ** 20 if kind == "scaled_up" else 2.0 ** -6
            p0, t0 = fvd_ref.feature_tables(b, n, "shifted")
            assert torch.equal(p / f, p0) and torch.equal(t / f, t0)                  # exact in float32
        if kind in ("equal_sigma", "graded"):
            for table in (p, t):
                s = fvd_ref.centred_sigma(table)
                assert int((s > s[0] * 400 * 2.3e-16).sum()) == b - 1, (b, kind, s)   # rank b - 1: centring takes one, nothing else is lost
                if kind == "equal_sigma":
                    assert float(s[0] / s[b - 2]) < 1 + 1e-5
                elif b > 2:
                    assert float(s[0] / s[b - 2]) > 1e6 and float(s[b // 2] / s[0]) < 1e-3
            if kind == "equal_sigma":
                sg = torch.linalg.svdvals((p.double() - p.double().mean(0)) @ (t.double() - t.double().mean(0)).t())
                assert float(sg[0] / sg[b - 2]) < 1 + 1e-5 and float(sg[b - 1]) < 1e-12 * float(sg[0])
        ref = float(M.frechet_distance_host(p, t))
        gp = torch.Generator().manual_seed(b + n)
        moved = float(M.frechet_distance_host(p[torch.randperm(b, generator=gp)], t[torch.randperm(b, generator=gp)]))
        bound = fvd_ref.frechet_bound(p, t)
        assert abs(moved - ref) < 0.1 * bound, (b, n, kind, ref, moved, bound)
        if kind in ("shifted", "scaled_up", "graded"):
            assert abs(ref) > 100 * bound, (b, n, kind, ref, bound)


# ---- the chunk rule ----------------------------------------------------------------------------------------------------------------
def test_chunk_table_against_the_reference():
    table = _golden("fvd_chunks.npz")["table"]
    assert table.shape == (fvd_ref.CHUNK_MAX_T, 4) and list(table[:, 0]) == list(range(1, fvd_ref.CHUNK_MAX_T + 1))
    raised = [int(T) for T, _, _, r in table if r]
    assert raised == [17, 18, 112]                       # the reference's lossy branch divides by a tuple: TypeError
    for T, n, drop, r in table.tolist():
        got = M.fvd_chunks(T)
        if T < 9:
            assert n == -1 and got is None
            continue
        assert got[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:]))          # consecutive from frame 0
        assert all(M.FVD_MIN_T <= length <= M.FVD_MAX_T for _, length in got), (T, got)
        if r:       # the departure: the chunk length with the largest remainder, the last chunk dropped
            rem = {l: T % l for l in range(16, 8, -1)}
            best = max(rem.values())
            assert max(rem.values()) < 9 and len(got) == T // [l for l in rem if rem[l] == best][-1]
            assert sum(length for _, length in got) < T
        else:       # the reference's count and torch.chunk's sizes; it never drops a chunk where it does not raise
            assert drop == 0 and len(got) == n
            assert [length for _, length in got] == [c.numel() for c in torch.chunk(torch.arange(T), n)]
    assert M.fvd_chunks(17) == [(0, 9)] and M.fvd_chunks(20) == [(0, 10), (10, 10)] and len(M.fvd_chunks(112)) == 8


# ---- the host restatement against the reference's blocks -----------------------------------------------------------------------------
BLOCK_TOL = 1e-12   # float64 on both sides; the fold moves roundings of 1e-16 around


def test_host_units_pools_and_blocks_against_the_reference():
    rec = _golden("fvd_blocks.npz")
    assert len(rec) == len(fvd_ref.UNIT_CASES) + len(fvd_ref.POOL_CASES) + len(fvd_ref.BLOCK_CASES)
    for case in fvd_ref.UNIT_CASES:
        x, tensors = fvd_ref.unit_case(case)
        got = M._fvd_unit_host(x.double(), fvd_ref.folded(tensors, "u"), case[2], case[3])
        want = torch.from_numpy(rec["unit_" + fvd_ref.case_id(case)])
        assert got.shape == want.shape and fvd_ref.relmax(got, want) < BLOCK_TOL, case
        assert tuple(got.shape[2:]) == tuple(M.same_pad(n, k, s)[2] for n, k, s in zip(case[4], case[2], case[3]))
    for case in fvd_ref.POOL_CASES:
        got = M._fvd_pool_host(fvd_ref.pool_case(case).double(), case[0], case[1])
        want = torch.from_numpy(rec["pool_" + fvd_ref.case_id(case)])
        assert torch.equal(got, want), case
        if case[3] == "negative":    # the reference pads with zeros before it pools: border windows give 0, never less
            assert float(want.max()) == 0.0 and float(want.min()) < 0.0 or case[0] == (2, 2, 2)
    for case in fvd_ref.BLOCK_CASES:
        x, tensors = fvd_ref.block_case(case)
        weights = {f"m.{b}": fvd_ref.folded(tensors, f"m.{b}") for b, _ in M.FVD_BRANCHES}
        got = M._fvd_block_host(x.double(), weights, "m")
        want = torch.from_numpy(rec["block_" + fvd_ref.case_id(case)])
        assert got.shape == want.shape and got.shape[1] == case[1][0] + case[1][2] + case[1][4] + case[1][5]
        assert fvd_ref.relmax(got, want) < BLOCK_TOL, case


def test_host_network_against_the_reference():
    """The whole restated network — the sequence, the widths, the fold, the head — against InceptionI3d.extract_features at the real widths
    on one seeded 9-frame clip, both in float64 (weights and clip regenerated from seeds, 400 recorded features)."""
    want = torch.from_numpy(_golden("fvd_network.npz")["features"])
    M.register_fvd_weights(fvd_ref.state_dict(1))
    try:
        got = M._fvd_features_host(fvd_ref.network_case().double(), M.fvd_weights("cpu", torch.float64))
    finally:
        M.clear_fvd_weights()
    assert got.shape == want.shape == (1, fvd_ref.N_FEATURES) and float(want.abs().max()) >= 1.0
    assert fvd_ref.relmax(got, want) < 1e-11      # 22 layers of float64 roundings moved around by the fold


def test_wasserstein_distance_against_the_reference():
    """calculate_2_wasserstein_dist as recorded, next to its own deviation from the singular-value form (measured when it was recorded: its
    non-symmetric eigvals is noisy, and it returns float32). The restatement is held to 2 x that deviation plus the float64 bound of the
    form itself (tests/fvd_ref.py: frechet_bound)."""
    rec = _golden("fvd_wasserstein.npz")
    assert len(rec) == len(fvd_ref.WASSERSTEIN_CASES)
    for b, n, kind in fvd_ref.WASSERSTEIN_CASES:
        p, t = fvd_ref.feature_tables(b, n, kind)
        ref, dev = rec[f"{b}_{n}_{kind}"]
        got = M.frechet_distance_host(p, t)
        assert got.dtype == torch.float64 and abs(float(got) - ref) <= 2 * dev + fvd_ref.frechet_bound(p, t), (b, n, kind)
        assert dev <= 1e-6 * fvd_ref.frechet_scale(p, t) + 1e-7                       # a float32-sized deviation, never a loose one
        if kind == "identical":
            assert abs(float(got)) <= 2 * b * 1e-15 ** 0.5 + 1e-10 * fvd_ref.frechet_scale(p, t)
    with pytest.raises(ValueError, match="equal shapes"):
        M.frechet_distance_host(torch.zeros(3, 4), torch.zeros(3, 5))


# ---- the measure and the providers on host tensors --------------------------------------------------------------------------------------
def test_measure_and_providers_on_the_host(registered):
    pred, target = fvd_ref.clips((2, 10, 3, 20, 28), seed=1)
    m = M.FrechetVideoDistance("cpu")
    assert m(pred[:, :8], target[:, :8]) is None
    with pytest.raises(ValueError, match="not equal"):
        m(pred, target[:, :9])
    with pytest.raises(ValueError, match="channels"):
        m(pred[:, :, :2], target[:, :, :2])
    value = m(pred, target)
    feats = M._fvd_features_host(torch.cat([pred, target]), M.fvd_weights("cpu"))
    assert float(feats.abs().max()) >= 1.0
    assert value.dtype == torch.float32 and float(value) == float(M.frechet_distance_host(feats[:2], feats[2:]).float()) and float(value) > 0
    grad = pred.clone().requires_grad_(True)           # forward only, on the host too: no term without a gradient passes for a loss
    with pytest.raises(NotImplementedError, match="forward only"):
        m(grad, target)
    with pytest.raises(NotImplementedError, match="forward only"):
        M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"mse": 1.0, "fvd": 0.5}}).get_losses(grad, target)
    with torch.no_grad():
        assert float(m(grad, target)) == float(value)
    assert abs(float(m(pred, pred))) <= 2 * 2 * 1e-15 ** 0.5 + 1e-10 * fvd_ref.frechet_scale(feats[:2], feats[:2])
    mp = M.PredictionMetricProvider({"device": "cpu", "metrics": ["mse", "fvd"]})
    every = mp.get_metrics(pred, target, all_frame_cnts=True)
    assert len(every) == 10 and [("fvd (↓)" in d) for d in every] == [False] * 8 + [True, True] and all("mse (↓)" in d for d in every)
    assert math.isclose(every[9]["fvd (↓)"], float(value), rel_tol=1e-6) and math.isclose(every[8]["fvd (↓)"], float(m(pred[:, :9], target[:, :9])), rel_tol=1e-6)
    (last,) = mp.get_metrics(pred, target)
    assert math.isclose(last["fvd (↓)"], float(value), rel_tol=1e-6)
    with pytest.warns(UserWarning, match="dropped"):      # other channel counts: the metric is dropped, the rest is computed
        (mono,) = mp.get_metrics(pred[:, :, :1], target[:, :, :1])
    assert list(mono) == ["mse (↓)"]
    disp, total = M.PredictionLossProvider({"device": "cpu", "losses_and_scales": {"mse": 1.0, "fvd": 0.5}}).get_losses(pred, target)
    assert math.isclose(float(disp["fvd"]), float(value), rel_tol=1e-6) and math.isclose(float(total), float(disp["mse"]) + 0.5 * float(value), rel_tol=1e-5)
    for fn, args in ((ops.conv3d_same, (torch.zeros(1, 2, 3, 3, 4), torch.zeros(5, 4, 1, 1, 1), torch.zeros(5))), (ops.maxpool3d_same, (torch.zeros(1, 2, 3, 3, 4), 3, 1)),
                     (ops.fvd_head, (torch.zeros(1, 2, 7, 7, 4), torch.zeros(5, 4), torch.zeros(5))), (ops.frechet_distance, (torch.zeros(3, 4), torch.zeros(3, 4)))):
        with pytest.raises(Exception, match="GPU"):      # no CPU fallback behind the ops
            fn(*args)


# ---- C ABI in a dry run ------------------------------------------------------------------------------------------------------------
def _fake_params(n):
    return (ctypes.c_void_p * n)(*[0x200000000000 + i * (1 << 30) for i in range(n)])


def test_entry_points_dry_run(L, registered):
    trunk = M._fvd_trunk("cpu")
    table, rows, n_params = trunk["table"], trunk["n_rows"], len(trunk["params"])
    assert rows == 5 + 9 * 7 + 2 + 1 and n_params == 2 * (len(M.FVD_UNITS) + 1) and trunk["ci"] == 3 and trunk["n_features"] == 50
    params = _fake_params(n_params)
    for n0, n1, T, h, w in ((1, 0, 9, 20, 28), (2, 2, 12, 64, 64), (16, 16, 16, 64, 64), (1, 1, 10, 224, 224), (3, 0, 16, 300, 7)):
        nb = L.vpx_fvd_features_workspace_bytes(n0 + n1, T, 3, h, w, table, rows)
        assert nb > (n0 + n1) * T * 224 * 224 * 3 * 4, L.vpx_last_error()
        for base in (WS_BASE, WS_BASE_ODD):
            _ok(L, L.vpx_fvd_features(_fake(1), _fake(2) if n1 else None, n0, n1, T, 3, h, w, table, rows, params, n_params, _fake(3), ctypes.c_void_p(base), nb, None),
                f"fvd_features {(n0, n1, T, h, w)}", False)
        assert L.vpx_fvd_features(_fake(1), _fake(2), n0, n1, T, 3, h, w, table, rows, params, n_params, _fake(3), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
        assert L.vpx_fvd_features(_fake(1), _fake(2), n0, n1, T, 3, h, w, table, rows, params, n_params, _fake(3), None, nb, None) == E_WS
    for T in (1, 8, 17, 32):      # the final map is not 2x7x7: refused by the query and by the call
        assert L.vpx_fvd_features_workspace_bytes(2, T, 3, 64, 64, table, rows) == 0 and b"2x7x7" in L.vpx_last_error()
        assert L.vpx_fvd_features(_fake(1), None, 2, 0, T, 3, 64, 64, table, rows, params, n_params, _fake(3), ctypes.c_void_p(WS_BASE), 1 << 40, None) == E_ARG
    assert L.vpx_fvd_features(_fake(1), None, 2, 0, 9, 2, 64, 64, table, rows, params, n_params, _fake(3), ctypes.c_void_p(WS_BASE), 1 << 40, None) == E_ARG
    assert b"input channels" in L.vpx_last_error()
    assert L.vpx_fvd_features(_fake(1), None, 2, 0, 9, 3, 64, 64, table, rows, params, n_params - 1, _fake(3), ctypes.c_void_p(WS_BASE), 1 << 40, None) == E_ARG
    for args in ((None, None, 2, 0), (_fake(1), None, 2, 1), (_fake(1), None, 0, 0)):
        assert L.vpx_fvd_features(*args, 9, 3, 64, 64, table, rows, params, n_params, _fake(3), ctypes.c_void_p(WS_BASE), 1 << 40, None) == E_ARG
    assert L.vpx_conv3d_same_workspace_bytes() == 0 and L.vpx_maxpool3d_same_workspace_bytes() == 0 and L.vpx_fvd_head_workspace_bytes() == 0
    good = [_fake(1), _fake(2), _fake(3), _fake(4), 3, 9, 13, 10, 3, 64, 7, 7, 7, 2, 2, 2, 1, 64, 0]
    assert L.vpx_conv3d_same(*good, None) == OK
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (8, 0), (9, 0), (10, 0), (13, 0), (17, 63), (18, 1), (18, -1)):
        bad = list(good)
        bad[i] = v
        assert L.vpx_conv3d_same(*bad, None) == E_ARG, (i, v)
    bad = list(good)
    bad[10] = 16
    assert L.vpx_conv3d_same(*bad, None) == E_UNSUPPORTED and b"15" in L.vpx_last_error()
    good = [_fake(1), _fake(2), 3, 9, 13, 10, 5, 3, 3, 3, 2, 2, 2]
    assert L.vpx_maxpool3d_same(*good, None) == OK
    for i, v in ((0, None), (1, None), (2, 0), (3, 0), (6, 0), (7, 0), (10, 0)):
        bad = list(good)
        bad[i] = v
        assert L.vpx_maxpool3d_same(*bad, None) == E_ARG, (i, v)
    good = [_fake(1), _fake(2), _fake(3), _fake(4), 5, 2, 7, 7, 1024, 400]
    assert L.vpx_fvd_head(*good, None) == OK
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 1), (6, 6), (7, 8), (8, 0), (9, 0)):
        bad = list(good)
        bad[i] = v
        assert L.vpx_fvd_head(*bad, None) == E_ARG, (i, v)
    bad = list(good)
    bad[8] = 4097
    assert L.vpx_fvd_head(*bad, None) == E_UNSUPPORTED and b"4096" in L.vpx_last_error()
    for b, n in ((1, 7), (2, 400), (33, 400), (ops.FVD_MAX_B, 400), (ops.FVD_MAX_B, 1)):
        nb = L.vpx_frechet_distance_workspace_bytes(b, n)
        assert nb >= 8 * (2 * b * n + b * b + 3 * n)
        for base in (WS_BASE, WS_BASE_ODD):
            _ok(L, L.vpx_frechet_distance(_fake(1), _fake(2), b, n, _fake(3), ctypes.c_void_p(base), nb, None), f"frechet {(b, n)}", False)
        assert L.vpx_frechet_distance(_fake(1), _fake(2), b, n, _fake(3), ctypes.c_void_p(WS_BASE), nb - 1, None) == E_WS
        assert L.vpx_frechet_distance(_fake(1), _fake(2), b, n, _fake(3), None, nb, None) == E_WS
    assert L.vpx_frechet_distance_workspace_bytes(ops.FVD_MAX_B + 1, 7) == 0 and L.vpx_frechet_distance_workspace_bytes(0, 7) == 0
    assert L.vpx_frechet_distance(_fake(1), _fake(2), ops.FVD_MAX_B + 1, 7, _fake(3), ctypes.c_void_p(WS_BASE), 1 << 30, None) == E_UNSUPPORTED
    assert str(ops.FVD_MAX_B).encode() in L.vpx_last_error()
    for args in ((None, _fake(2), 3, 7, _fake(3)), (_fake(1), None, 3, 7, _fake(3)), (_fake(1), _fake(2), 3, 7, None), (_fake(1), _fake(2), 0, 7, _fake(3)), (_fake(1), _fake(2), 3, 0, _fake(3))):
        assert L.vpx_frechet_distance(*args, ctypes.c_void_p(WS_BASE), 1 << 30, None) == E_ARG
