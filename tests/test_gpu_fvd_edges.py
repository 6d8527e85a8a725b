"""csrc/fvd.hip where its first tests do not reach: the convolution tap by tap (exact) and against float64 at anisotropic kernels and
strides, even kernels, strides above the kernel, maps narrower than the kernel, ragged M tiles and misaligned operands; non-finite values
through the ReLU, the pool, the trunk and the distance; the pool and the head at further forms and widths; the staging kernel at
downscales, one-pixel frames and two channels; the Jacobi iteration at its lane boundaries, at equal and at graded singular values and at
tables far from unit scale. Case tables and references: tests/fvd_ref.py (checked on the host in tests/test_fvd_host.py)."""
import pytest
import torch
import torch.nn.functional as F

import fvd_ref
from vp_suite_amd import measure as M
from vp_suite_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONV_BAR = 1e-5            # exact fp32 operands: the bar of tests/test_gpu_fvd_kernels.py
MARGIN, FLOOR = 4.0, 1e-6  # the trunk's rule of tests/test_gpu_fvd.py
NAN, INF = float("nan"), float("inf")
_form_ids = dict(ids=fvd_ref.form_id)


def _cl(x):   # [N, C, T, H, W] -> channels-last [N, T, H, W, C] on the GPU
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def _cf(y):   # back, on the host
    return y.cpu().permute(0, 4, 1, 2, 3)


@pytest.fixture
def thin():
    M.register_fvd_weights(fvd_ref.state_dict())
    yield M.fvd_weights(DEV)
    M.clear_fvd_weights()


# ---- 1. unit taps: a strided shift of one zero-padded channel, exactly --------------------------------------------------------------------
@pytest.mark.parametrize("ci", (3, 4))
@pytest.mark.parametrize("form", fvd_ref.EDGE_FORMS, **_form_ids)
def test_conv3d_unit_taps_are_exact_shifts(vpx, form, ci):
    kernel, stride, _ = form
    x = fvd_ref.edge_conv_case(form, ci, fvd_ref.TAP_CO, 2)[0]
    xd, zero = _cl(x), torch.zeros(fvd_ref.TAP_CO, device=DEV)
    for tap in fvd_ref.unit_taps(kernel, ci):
        w = torch.zeros(fvd_ref.TAP_CO, ci, *kernel)
        w[tap] = 1.0
        want, keep = fvd_ref.unit_tap_expected(x, fvd_ref.TAP_CO, tap, kernel, stride)
        got = _cf(vpx.ops.conv3d_same(xd, w.to(DEV), zero, stride=stride, relu=False))
        assert got.shape == want.shape and torch.equal(got, want), (form, ci, tap)
        others = [c for c in range(fvd_ref.TAP_CO) if c != tap[0]]
        assert bool((got[:, others] == 0).all()) and bool((got[:, tap[0]][:, ~keep] == 0).all())   # other channels, taps in the padding
        assert bool((got[:, tap[0]][:, keep] != 0).all())   # (a tap that no output reaches inside the map gives an all-zero map)


# ---- 2. float64 parity at anisotropic forms and tile seams --------------------------------------------------------------------------------
PARITY_CASES = ([(form, ci, co) for form in fvd_ref.EDGE_FORMS for ci, co in fvd_ref.EDGE_WIDTHS]
                + [(form, ci, co) for form in fvd_ref.ADJACENT_FORMS for ci, co in ((12, 70), (16, 64))])


@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: f"{fvd_ref.form_id(c[0])}-ci{c[1]}-co{c[2]}")
def test_conv3d_same_edge_forms_against_float64(case, parity_log):
    """N is the smallest batch from 3 on at which M spans several 64-position tiles with a ragged last one: 3 everywhere but on the
    2x7x5 map under stride (1, 3, 2), whose 18 outputs per map need 4."""
    form, ci, co = case
    kernel, stride, (T, H, W) = form
    n = fvd_ref.ragged_batch(form)
    x, w, bias = fvd_ref.edge_conv_case(form, ci, co, n)
    xd, wd, bd = _cl(x), w.to(DEV), bias.to(DEV)
    for relu in (False, True):
        ref = fvd_ref.conv3d_same_ref(x, w, bias, stride, relu)
        m_rows = ref.numel() // co
        assert m_rows % 64 != 0 and m_rows > 64 and m_rows == fvd_ref.out_positions(form, n)
        assert float(ref.abs().max()) > 0.1 and (not relu or ref.numel() < 16 or bool((ref == 0).any()))   # (the ReLU is at work)
        got = ops.conv3d_same(xd, wd, bd, stride=stride, relu=relu)
        assert tuple(got.shape) == (n, *ref.shape[2:], co)
        err = parity_log(f"conv3d_same edge relu={relu}", _cf(got), ref, CONV_BAR)
        print(f"conv3d_same {fvd_ref.form_id(form)} Ci={ci} Co={co} N={n} relu={relu}: {err:.3e}")
        fvd_ref.record(f"conv3d_same edge {fvd_ref.form_id(form)} Ci={ci} Co={co} N={n} relu={relu}", hip=err, bound=CONV_BAR)
        assert err <= CONV_BAR


@pytest.mark.parametrize("form", fvd_ref.EDGE_FORMS + fvd_ref.ADJACENT_FORMS, **_form_ids)
def test_conv3d_same_batch_of_four_is_its_two_halves(form):
    """The kernel header's claim: every output's sum runs over K in one order, whatever tile it lies in."""
    x, w, bias = fvd_ref.edge_conv_case(form, 12, 70, 4, seed=1)
    xd, wd, bd = _cl(x), w.to(DEV), bias.to(DEV)
    whole = ops.conv3d_same(xd, wd, bd, stride=form[1], relu=True)
    halves = [ops.conv3d_same(xd[i:i + 2].contiguous(), wd, bd, stride=form[1], relu=True) for i in (0, 2)]
    assert torch.equal(whole, torch.cat(halves))


# ---- 3. the scalar loads chosen by pointer alignment --------------------------------------------------------------------------------------
def _one_float_in(t):
    """An equal-valued contiguous view that starts one float into a larger flat buffer: 4 bytes off a 16-byte boundary."""
    flat = torch.empty(t.numel() + 8, device=t.device)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()   # (the wrapper does not copy it)
    return view


def test_conv3d_same_misaligned_operands_give_the_same_bits():
    """Ci % 4 == 0 and Co % 4 == 0 with the map, then the packed weights, then both at 4 bytes off a 16-byte boundary: the scalar loads
    the kernel falls back to fill the same tiles, so the bits are those of the vector path."""
    form = ((3, 3, 3), (1, 1, 1), (3, 5, 6))
    x, w, bias = fvd_ref.edge_conv_case(form, 16, 64, 2, seed=2)
    xd, wp, bd = _cl(x), ops.conv3d_pack(w.to(DEV)), bias.to(DEV)
    assert xd.data_ptr() % 16 == 0 and wp.data_ptr() % 16 == 0
    base = ops.conv3d_same(xd, wp, bd, relu=True, packed=True)
    ref = fvd_ref.conv3d_same_ref(x, w, bias, (1, 1, 1), True)
    assert fvd_ref.relmax(_cf(base), ref) <= CONV_BAR
    x_off, w_off = _one_float_in(xd), _one_float_in(wp)
    assert torch.equal(x_off, xd) and torch.equal(w_off, wp)
    assert torch.equal(ops.conv3d_same(x_off, wp, bd, relu=True, packed=True), base)
    assert torch.equal(ops.conv3d_same(xd, w_off, bd, relu=True, packed=True), base)
    assert torch.equal(ops.conv3d_same(x_off, w_off, bd, relu=True, packed=True), base)


# ---- 4. non-finite values are kept -----------------------------------------------------------------------------------------------------------
def _held_where_finite(got, ref, what):
    """NaN where the reference is NaN and nowhere else, the reference's infinities with their signs, the rest within CONV_BAR."""
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN at {int(torch.isnan(got).sum())} outputs, the float64 reference at {int(torch.isnan(ref).sum())}"
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf].double(), ref[inf]), what
    finite = torch.isfinite(ref)
    err = float((got.double() - ref)[finite].abs().max() / ref[finite].abs().max())
    assert err <= CONV_BAR, (what, err)
    return err


@pytest.mark.parametrize("ci,co", ((3, 5), (16, 64)))
def test_conv3d_same_relu_keeps_nan_and_inf(ci, co):
    form = ((3, 3, 3), (1, 1, 1), (3, 5, 6))
    x, w, bias = fvd_ref.edge_conv_case(form, ci, co, 2, seed=3)
    wd, bd = w.to(DEV), bias.to(DEV)
    spot = (1, ci - 1, 1, 2, 3)
    for value in (NAN, INF, -INF):
        xv, wv = x.clone(), w.clone()
        xv[spot] = value
        if value != value:
            wdv = wd
        else:   # weights of one sign on that channel: an infinity never meets one of the other sign in a sum
            wv[:, spot[1]] = wv[:, spot[1]].abs() + 0.01
            wdv = wv.to(DEV)
        ref = fvd_ref.conv3d_same_ref(xv, wv, bias, (1, 1, 1), True)
        hit = 27 * co   # an inner element of the second map: in 27 windows, in every output channel
        assert int((torch.isnan(ref) if value != value else (torch.isinf(ref) if value > 0 else ref == 0)).sum()) >= hit and not bool(torch.isnan(ref[0]).any())
        got = _cf(ops.conv3d_same(_cl(xv), wdv, bd, relu=True))
        err = _held_where_finite(got, ref, f"conv3d_same relu=True with {value} in the map")
        fvd_ref.record(f"conv3d_same Ci={ci} Co={co} relu=True, {value} at one input", hip_on_finite_outputs=err, bound=CONV_BAR,
                       nan_outputs=int(torch.isnan(got).sum()), inf_outputs=int(torch.isinf(got).sum()))


@pytest.mark.parametrize("case", fvd_ref.POOL_NAN_CASES, ids=lambda c: fvd_ref.form_id(c[:3]))
def test_maxpool3d_same_nan_wins(case):
    """One NaN per channel: the first, an inner and the last element of a window, elements that overlapping windows share, elements of
    border windows that also hold padding. The outputs that are NaN are those of the windows that hold the element (fvd_ref.window_mask,
    index arithmetic) and those of F.max_pool3d on the zero-padded map; every other output equals torch's bits."""
    kernel, stride, shape, spots = case
    g = torch.Generator().manual_seed(sum(shape) + sum(kernel))
    x = torch.randn(2, len(spots), *shape, generator=g)
    want = torch.zeros(2, len(spots), *(fvd_ref.same_rule(n, k, s)[1] for n, k, s in zip(shape, kernel, stride)), dtype=torch.bool)
    for c, at in enumerate(spots.values()):
        x[(c % 2, c) + tuple(at)] = NAN
        want[c % 2, c] = fvd_ref.window_mask(shape, kernel, stride, at)
    ref = fvd_ref.maxpool3d_same_ref(x, kernel, stride)
    got = _cf(ops.maxpool3d_same(_cl(x), kernel, stride))
    assert torch.equal(torch.isnan(ref), want)
    assert torch.equal(torch.isnan(got), want), {what: int(torch.isnan(got[:, c]).sum()) for c, what in enumerate(spots)}
    assert torch.equal(got.nan_to_num(nan=-77.0), ref.nan_to_num(nan=-77.0))


def _nan_clips():
    """(two clips [2, 9, 3, 20, 28]: one NaN pixel in the first, the second clean; the float64 host chain's features)."""
    clips = fvd_ref.clips((2, 9, 3, 20, 28), seed=9)[0].clone()
    clips[0, 4, 1, 7, 11] = NAN
    return clips, M._fvd_features_host(clips.double(), M.fvd_weights("cpu", torch.float64))


def test_thin_trunk_keeps_nan(thin):
    """A NaN pixel makes NaN features of its own clip, as the float64 host chain has it, and leaves the clip next to it alone."""
    clips, ref = _nan_clips()
    assert bool(torch.isnan(ref[0]).all()) and bool(torch.isfinite(ref[1]).all())
    got = ops.fvd_features(clips.to(DEV), thin)
    assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref)), f"NaN features per clip: HIP {torch.isnan(got).sum(dim=1).tolist()}, float64 host chain {torch.isnan(ref).sum(dim=1).tolist()}"
    alone = ops.fvd_features(clips[1:].to(DEV), thin)
    assert torch.equal(got[1:], alone) and bool(torch.isfinite(alone).all())
    target = fvd_ref.clips((2, 9, 3, 20, 28), seed=9)[1]
    value = M.FrechetVideoDistance(DEV)(clips.to(DEV), target.to(DEV))
    assert bool(torch.isnan(value)), float(value)                       # a model that predicts NaN frames has no finite FVD
    assert bool(torch.isfinite(M.FrechetVideoDistance(DEV)(clips[1:].to(DEV), target[1:].to(DEV))))


@pytest.mark.parametrize("b", (2, 33))
def test_frechet_distance_of_non_finite_tables_is_nan(b):
    for value in (NAN, INF, -INF):
        for which in (0, 1):
            tables = [t.clone() for t in fvd_ref.feature_tables(b, 7, "shifted")]
            tables[which][b - 1, 3] = value
            got = ops.frechet_distance(tables[0].to(DEV), tables[1].to(DEV))
            assert bool(torch.isnan(got)), (b, value, which, float(got))
    p, t = fvd_ref.feature_tables(b, 7, "shifted")
    assert bool(torch.isfinite(ops.frechet_distance(p.to(DEV), t.to(DEV))))


# ---- 5. pool and head ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", fvd_ref.POOL_EDGE_FORMS, ids=lambda f: "k" + "".join(map(str, f[0])) + "s" + "".join(map(str, f[1])))
def test_maxpool3d_same_anisotropic_forms_bit_for_bit(form):
    kernel, stride = form
    C = fvd_ref.POOL_EDGE_C
    for T, H, W in fvd_ref.POOL_EDGE_MAPS:
        g = torch.Generator().manual_seed(T * 100 + H * 10 + W + sum(kernel))
        mixed = torch.randn(2, C, T, H, W, generator=g)
        negative = -torch.rand(2, C, T, H, W, generator=g) - 0.25
        for name, x in (("mixed", mixed), ("negative", negative)):
            ref = fvd_ref.maxpool3d_same_ref(x, kernel, stride)
            got = _cf(ops.maxpool3d_same(_cl(x), kernel, stride))
            assert got.shape == ref.shape and torch.equal(got, ref), (name, T, H, W)
            assert tuple(ref.shape[2:]) == tuple(fvd_ref.same_rule(n, k, s)[1] for n, k, s in zip((T, H, W), kernel, stride))
        padded = any(max((fvd_ref.same_rule(n, k, s)[1] - 1) * s + k - n, 0) > 0 for n, k, s in zip((T, H, W), kernel, stride))
        assert float(ref.max()) <= 0 and bool((ref == 0).any()) == padded   # (ref: the all-negative map's)


@pytest.mark.parametrize("n_features", (1, 5))
@pytest.mark.parametrize("C", (1, 65, 130))
def test_head_at_narrow_and_odd_widths(C, n_features, parity_log):
    N = 3
    g = torch.Generator().manual_seed(7 * C + n_features)
    x = torch.randn(N, 2, 7, 7, C, generator=g).abs()
    w = torch.randn(n_features, C, generator=g) / C ** 0.5
    b = torch.randn(n_features, generator=g)
    ref = x.double().mean(dim=(1, 2, 3)) @ w.double().t() + b.double()
    got = ops.fvd_head(x.to(DEV), w.view(n_features, C, 1, 1, 1).to(DEV), b.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, n_features)
    bound = 2.0 ** -22
    err = parity_log("fvd_head", got.cpu(), ref, bound)
    fvd_ref.record(f"fvd_head C={C} features={n_features} N={N}", hip=err, bound=bound)
    assert err <= bound


# ---- 6. staging and trunk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", fvd_ref.STAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_staging_is_frames_adapt_at_every_size(thin, size):
    """Downscales, one axis already at 224, one-pixel frames: the trunk on the frames equals, bit for bit, the trunk on frames that
    ops.frames_adapt (held to float64 in tests/test_gpu_adapt.py) resized beforehand and the staging kernel then only copies."""
    x = fvd_ref.clips((1, 9, 3, *size), seed=size[0] + size[1])[0].to(DEV)
    staged = ops.frames_adapt(x, (224, 224))
    assert tuple(staged.shape) == (1, 9, 3, 224, 224)
    got = ops.fvd_features(x, thin)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.1
    assert torch.equal(got, ops.fvd_features(staged, thin))


def test_unequal_clip_counts(thin):
    pred, target = fvd_ref.clips((3, 9, 3, 20, 28), seed=31)
    p, t = pred[:1].to(DEV), target.to(DEV)
    got = ops.fvd_features(p, thin, t)
    assert tuple(got.shape) == (4, 50)
    assert torch.equal(got[:1], ops.fvd_features(p, thin)) and torch.equal(got[1:], ops.fvd_features(t, thin))


def test_two_channel_stem_against_float64(parity_log):
    M.register_fvd_weights(fvd_ref.state_dict(fvd_ref.THIN, in_channels=2))
    try:
        pred, target = fvd_ref.clips((1, 9, 2, 20, 28), seed=41)
        both = torch.cat([pred, target])
        ref = M._fvd_features_host(both.double(), M.fvd_weights("cpu", torch.float64))
        err32 = fvd_ref.relmax(M._fvd_features_host(both, M.fvd_weights("cpu")), ref)   # measured before the GPU result is looked at
        bound = max(MARGIN * err32, FLOOR)
        assert float(ref.abs().max()) >= 1.0
        trunk = M.fvd_weights(DEV)
        assert trunk["ci"] == 2
        got = ops.fvd_features(pred.to(DEV), trunk, target.to(DEV))
        assert tuple(got.shape) == (2, 50)
        err = parity_log("fvd_features thin two channels T=9", got.cpu(), ref, bound)
        print(f"two-channel thin trunk: max|ref| {float(ref.abs().max()):.3f}, float32 CPU chain {err32:.3e}, bound {bound:.3e}, HIP {err:.3e}")
        fvd_ref.record("thin two channels T=9", reference_error=err32, bound=bound, hip=err, max_ref=float(ref.abs().max()))
        assert err <= bound
    finally:
        M.clear_fvd_weights()


# ---- 7. Frechet distance: lane boundaries, equal and graded singular values, scales far from 1 -------------------------------------------------
def _frechet_held(b, n, kind):
    p, t = fvd_ref.feature_tables(b, n, kind)
    ref = float(M.frechet_distance_host(p, t))
    got = ops.frechet_distance(p.to(DEV), t.to(DEV))
    again = ops.frechet_distance(p.to(DEV), t.to(DEV))
    bound = fvd_ref.frechet_bound(p, t)
    print(f"frechet b={b} n={n} {kind}: value {ref:.6e}, |delta| {abs(float(got) - ref):.3e}, bound {bound:.3e}")
    fvd_ref.record(f"frechet_distance b={b} n={n} {kind}", svdvals_form=ref, abs_delta=abs(float(got) - ref), bound=bound)
    assert got.dtype == torch.float64 and bool(torch.isfinite(got)), (b, n, kind, float(got))   # NaN: no convergence within the sweeps
    assert abs(float(got) - ref) <= bound, (b, n, kind, float(got), ref)
    assert float(got) == float(again)
    return float(got)


@pytest.mark.parametrize("n", (1, 7, 400))
@pytest.mark.parametrize("b", (63, 64, 65, 127, 128, 129, 255))
def test_frechet_distance_at_lane_boundaries(b, n):
    assert (b, n, "shifted") in fvd_ref.FRECHET_LANE_CASES
    _frechet_held(b, n, "shifted")


@pytest.mark.parametrize("b", (2, 3, 33, 64, 65, 256))
@pytest.mark.parametrize("kind", fvd_ref.FRECHET_EDGE_KINDS)
def test_frechet_distance_at_equal_graded_and_scaled_values(kind, b):
    assert (b, 400, kind) in fvd_ref.FRECHET_KIND_CASES
    got = _frechet_held(b, 400, kind)
    if kind in ("scaled_up", "scaled_down"):   # the tables times f exactly: the distance times f^2, up to the constant under the root
        f = 2.0 ** 20 if kind == "scaled_up" else 2.0 ** -6
        p, t = fvd_ref.feature_tables(b, 400, "shifted")
        plain = float(ops.frechet_distance(p.to(DEV), t.to(DEV)))
        assert abs(got - f * f * plain) <= (1 + f * f) * fvd_ref.frechet_bound(p, t) + fvd_ref.frechet_bound(p * f, t * f)
