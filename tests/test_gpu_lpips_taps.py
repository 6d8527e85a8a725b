"""csrc/lpips.hip tap by tap: the cases of tests/test_gpu_lpips.py check the sum of the five taps at three sizes; here every tap is held
on its own over lpips_ref.GEOMETRY_CASES (tap-1 maps around the stem's 8x8 tile seams, H > W and H < W, deep maps of 1x1, 1x3, 3x1 and
7x5), the four trunk convolutions run alone as the measure calls them, and the stem, the pool and the head meet their edges. The
conditions on the inputs (tap sizes, no degenerate tap, the derived bounds) are checked on the CPU in tests/test_lpips_host.py.

One tap alone. ops.lpips_frames takes the weight dictionary: with every lin{k}.weight zeroed but lin{l}.weight (lpips_ref.isolated) each
other head adds an exact 0.0 and the table is tap l's share. A wrong map size, a head on the wrong workspace slot or a wrong lin / conv
index moves one tap's table by its own size, where the five-tap sum hides it behind tap 1 (about 1.0 against 0.05 - 0.25 for the others).

Bounds. Per tap: max(4 x the max-normalised error of the float32 CPU chain's tap table against the float64 one, 1e-6), from
lpips_ref.geometry_case, fixed before the library's table is looked at; 4 is lpips_ref.E2E_MARGIN, 1e-6 the two-rounding noise of a table
of double sums over fp32 features. Per kernel: 1e-5 max-normalised, the project's bar for fp32 convolution outputs; the pool moves values
(torch.equal). Figures of every (case, tap) go through parity_log and, with VPX_LPIPS_PARITY_OUT=FILE, into the `per_tap` section of
profiles/lpips_parity.json.

The reference-side error is that of the HOST's float32 convolutions (their blocking depends on the CPU and the thread count), so a
bound is a property of the host the test runs on: tap 5 of 31x31 gives 3.5e-7 (bound 1.4e-6) on the MI355X host and 5.0e-7 (2.0e-6)
on another. The kernel's figures do not depend on it.

Measured on an MI355X (worst over the four cases; kernel / bound): tap 1 1.2e-8 / 1.0e-6, tap 2 1.1e-7 / 1.0e-6, tap 3 6.0e-7 / 1.0e-6
(39x71, a 1x3 map), tap 4 1.0e-6 / 1.4e-6 (39x71), tap 5 1.1e-6 / 1.4e-6 (31x31, a single pixel: nothing averages). Trunk layers alone
2.6e-7 (64->192 at 1x1) ... 2.5e-6 (256->256 at 7x5) against 1e-5; stem edges <= 2.8e-7."""
import functools

import pytest
import torch
import torch.nn.functional as F

import lpips_ref
import test_gpu_lpips as base   # the parity record (_record) and the device weights are shared with the end-to-end tests

pytestmark = pytest.mark.gpu

KERNEL_TOL = base.KERNEL_TOL
ULP64 = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _device_case(case):
    pred, target, _, _, _ = lpips_ref.geometry_case(case)
    return pred.cuda(), target.cuda()


@functools.lru_cache(maxsize=None)
def _isolated_weights(tap):
    return lpips_ref.isolated(base._device_weights(), tap)


# ---- every tap on its own ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", lpips_ref.GEOMETRY_CASES)
def test_one_tap_vs_fp64(vpx, parity_log, case, tap):
    from vp_suite_amd import ops
    _, _, ref, errs, bounds = lpips_ref.geometry_case(case)
    ref, ref_err, bound = ref[tap - 1], errs[tap - 1], bounds[tap - 1]
    assert lpips_ref.TAP_FLOOR <= bound <= lpips_ref.TAP_CEILING, bound
    p, t = _device_case(case)
    w = _isolated_weights(tap)
    got = ops.lpips_frames(p, t, w)
    assert got.shape == ref.shape and got.dtype == torch.float64
    e = parity_log(f"lpips.tap{tap}", got, ref, bound)
    print(f"lpips tap {tap} {case} {lpips_ref.GEOMETRY_TAPS[case][tap - 1]}: kernel {e:.3e}, reference-side {ref_err:.3e}, bound {bound:.3e}")
    base._record(case, tap=tap, kernel_error=e, reference_error=ref_err, bound=bound)
    assert torch.equal(ops.lpips_frames(p, t, w), got)                                                   # bit-reproducible
    assert torch.equal(ops.lpips_frames(p, p, w).cpu(), torch.zeros(ref.shape, dtype=torch.float64))   # pred == target: exactly 0
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("case", lpips_ref.GEOMETRY_CASES)
def test_taps_add_up_to_the_table(vpx, case):
    """Each head adds into the same double table in a fixed order: the five isolated tables, added in that order, are the whole table."""
    from vp_suite_amd import ops
    p, t = _device_case(case)
    whole = ops.lpips_frames(p, t, base._device_weights()).cpu()
    total = torch.zeros_like(whole)
    for tap in range(1, 6):
        total = total + ops.lpips_frames(p, t, _isolated_weights(tap)).cpu()
    assert bool((whole > 0).all())
    assert bool(((total - whole).abs() <= 5 * ULP64 * whole.abs()).all()), float(((total - whole).abs() / whole.abs()).max())


# ---- the trunk layers as the measure calls them ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", lpips_ref.TRUNK_MAPS)
@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_trunk_layer_vs_fp64(vpx, parity_log, layer, h, w):
    """vpx_lpips_fwd runs taps 2 .. 5 through glue_forward with VPX_ACT_RELU on exact fp32 operands; stphy_ops.conv2d_act(act="relu",
    precision="f32") is the Python entry to the same call. N = 4 non-negative maps of 1x1 .. 7x5, where the 5x5 / 3x3 window is mostly
    padding. tests/glue_ref.py holds no case of these (Ci, Co, k) at any map (test_lpips_host.test_trunk_layer_cases asserts it): nothing
    here repeats a case of tests/test_gpu_glue.py."""
    from vp_suite_amd import stphy_ops
    Ci, Co, k, pad = lpips_ref.TRUNK_LAYERS[layer]
    x, wt, b, pre = lpips_ref.trunk_case(layer, h, w)
    ref = F.relu(pre)
    y = stphy_ops.conv2d_act(x.cuda(), wt.cuda(), b.cuda(), 1, pad, False, "relu", "f32")
    assert tuple(y.shape) == tuple(ref.shape) and y.dtype == torch.float32
    e = parity_log("lpips.trunk", y, ref, lpips_ref.TRUNK_TOL)
    print(f"trunk {Ci}->{Co} k{k} {h}x{w}: {e:.3e}")
    assert e <= lpips_ref.TRUNK_TOL, e
    off = pre < -lpips_ref.TRUNK_TOL * float(ref.max())
    assert bool(off.any()) and bool((y.cpu()[off] == 0).all())   # clearly negative pre-activations: exact zeros
    assert float(y.min()) >= 0.0


# ---- stem --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lpips_ref.STEM_EDGE_KINDS)
@pytest.mark.parametrize("H,W", lpips_ref.STEM_EDGE_SIZES)
def test_stem_edges_vs_fp64(vpx, parity_log, H, W, kind):
    """7x7: every tap of the 11x11 window but the centre 7x7 is padding; 7x10 / 10x7: one output, a window that is cut on three sides;
    39x71 / 67x38: tap-1 maps of 9x17 and 16x8, one row / column past a tile seam and exactly on it."""
    from vp_suite_amd import ops
    N = 2
    x, ref = lpips_ref.stem_edge_case(N, H, W, kind)
    wts = lpips_ref.weights()
    if kind == "constant":
        if ref.shape[2] > 2 and ref.shape[3] > 2:   # the interior sees one constant, the ring a zero: the border outputs differ from the interior ones
            assert not torch.allclose(ref[:, :, 0, 0], ref[:, :, ref.shape[2] // 2, ref.shape[3] // 2])
        else:                                       # a single output: it differs from the value of a window that lies wholly inside the constant
            inside = wts["conv1.bias"].double() + (wts["conv1.weight"].double() * lpips_ref.normalise(x[:1, :, :1, :1])).sum(dim=(1, 2, 3))
            assert not torch.allclose(ref[0, :, 0, 0], F.relu(inside))
    w = base._device_weights()
    y = ops.lpips_stem(x.cuda(), w["conv1.weight"], w["conv1.bias"])
    assert y.shape == (N, ref.shape[2], ref.shape[3], 64)
    e = parity_log("lpips.stem", lpips_ref.nchw(y.cpu()), ref, KERNEL_TOL)
    print(f"stem {(N, H, W, kind)}: {e:.3e}")
    assert e <= KERNEL_TOL, e


@pytest.mark.parametrize("H,W", [(39, 71), (7, 10)])
def test_stem_source_splits_are_one_batch(vpx, H, W):
    from vp_suite_amd import ops
    x, _ = lpips_ref.stem_edge_case(5, H, W, "noise")
    w = base._device_weights()
    xd = x.cuda()
    whole = ops.lpips_stem(xd, w["conv1.weight"], w["conv1.bias"])
    for n0 in (1, 4):                                                   # (n0, n1) = (1, 4), (4, 1)
        assert torch.equal(ops.lpips_stem(xd[:n0], w["conv1.weight"], w["conv1.bias"], xd[n0:]), whole), n0
    assert torch.equal(ops.lpips_stem(xd[:1], w["conv1.weight"], w["conv1.bias"]), whole[:1])            # (1, 0): x1 = None
    assert torch.equal(ops.lpips_stem(xd[:1], w["conv1.weight"], w["conv1.bias"], xd[:0]), whole[:1])    # (1, 0): a source of no image


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------
def _pool_equal(x):
    """ops.lpips_maxpool against F.max_pool2d on x [N,C,h,w]: the NaN masks and every other value (infinities included) are equal."""
    from vp_suite_amd import ops
    ref = F.max_pool2d(x, kernel_size=3, stride=2)
    y = lpips_ref.nchw(ops.lpips_maxpool(lpips_ref.nhwc(x).cuda()).cpu())
    assert y.shape == ref.shape
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(y, nan=0.0, posinf=float("inf"), neginf=float("-inf")), torch.nan_to_num(ref, nan=0.0, posinf=float("inf"), neginf=float("-inf")))
    return y


@pytest.mark.parametrize("C", lpips_ref.POOL_EDGE_C)
@pytest.mark.parametrize("h,w", lpips_ref.POOL_EDGE_MAPS)
def test_maxpool_mixed_signs(vpx, h, w, C):
    """4x4, 6x9, 9x6: floor mode drops the last row and / or column; 5x5: two overlapping windows per axis."""
    x = lpips_ref.pool_edge_case(C, h, w)
    assert float(x.min()) < 0 < float(x.max())
    y = _pool_equal(x)
    assert y.shape[2:] == ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
    if h % 2 == 0:   # the dropped row holds the map's maximum: it must not show
        x = x.clone()
        x[:, :, -1, :] = 100.0
        assert float(_pool_equal(x).max()) < 100.0
    if w % 2 == 0:
        x = x.clone()
        x[:, :, :, -1] = 100.0
        assert float(_pool_equal(x).max()) < 100.0


def test_maxpool_infinities(vpx):
    x = lpips_ref.pool_edge_case(5, 5, 5).clone()
    x[0, 0, 0:3, 0:3] = float("-inf")           # window (0, 0) of channel 0 holds nothing else
    x[0, 1, 2:5, 2:5] = float("-inf")           # window (1, 1) of channel 1: -inf but one finite value, its last element
    x[0, 1, 4, 4] = -7.0
    x[1, 2, 1, 1] = float("inf")
    y = _pool_equal(x)
    assert float(y[0, 0, 0, 0]) == float("-inf") and float(y[0, 1, 1, 1]) == -7.0 and float(y[1, 2, 0, 0]) == float("inf")
    assert bool(torch.isfinite(y[0, 0, 1, 1]))   # (the windows beside it see finite values)


def test_maxpool_nan_wins(vpx):
    """NaN as the first, an inner and the last element of a window; a NaN that two or four overlapping windows share shows in each of them;
    a NaN in the row floor mode drops shows nowhere."""
    nan = float("nan")
    x = lpips_ref.pool_edge_case(5, 5, 5).clone()        # 5x5 -> 2x2 windows over rows / columns 0-2 and 2-4
    x[0, 0, 0, 0] = nan                                  # first element of window (0, 0)
    x[0, 1, 1, 1] = nan                                  # inner element of window (0, 0)
    x[0, 2, 2, 2] = nan                                  # last element of window (0, 0), first of (1, 1): shared by all four
    x[0, 3, 2, 0] = nan                                  # shared by windows (0, 0) and (1, 0)
    x[1, 0, 4, 4] = nan                                  # last element of window (1, 1)
    x[1, 1, 0, 2] = nan                                  # shared by windows (0, 0) and (0, 1)
    y = _pool_equal(x)
    mask = torch.isnan(y)
    want = torch.zeros_like(mask)
    want[0, 0, 0, 0] = want[0, 1, 0, 0] = True
    want[0, 2] = True
    want[0, 3, :, 0] = True
    want[1, 0, 1, 1] = True
    want[1, 1, 0, :] = True
    assert torch.equal(mask, want)
    x = lpips_ref.pool_edge_case(5, 6, 9).clone()        # 6x9 -> 2x4: row 5 is dropped
    x[:, :, 5, :] = nan
    assert not bool(torch.isnan(_pool_equal(x)).any())
    x[0, 4, 4, 8] = nan                                  # the last element of the last window
    y = _pool_equal(x)
    assert bool(torch.isnan(y[0, 4, 1, 3])) and int(torch.isnan(y).sum()) == 1


# ---- head --------------------------------------------------------------------------------------------------------------------------
def _head_checks(parity_log, C, h, w, scale=1.0):
    from vp_suite_amd import ops
    fx, fy, lin, ref = lpips_ref.head_edge_case(C, h, w, scale)
    N = lpips_ref.HEAD_EDGE_N
    dx, dy, dl = lpips_ref.nhwc(fx).cuda(), lpips_ref.nhwc(fy).cuda(), lin.cuda()
    got = ops.lpips_head(dx, dy, dl)
    assert got.dtype == torch.float64 and got.shape == (N,) and bool(torch.isfinite(got).all())
    e = parity_log("lpips.head", got, ref, KERNEL_TOL)
    print(f"head {(N, C, h, w, scale)}: {e:.3e}")
    assert e <= KERNEL_TOL, e
    assert torch.equal(ops.lpips_head(dx, dy, dl), got)                                         # bit-reproducible
    assert torch.equal(ops.lpips_head(dx, dx, dl).cpu(), torch.zeros(N, dtype=torch.float64))   # identical maps: exactly 0
    twice = ops.lpips_head(dx, dy, dl, table=got.clone())                                       # the head ADDS into its table
    assert lpips_ref.relmax(twice, 2 * ref) <= KERNEL_TOL
    return e


@pytest.mark.parametrize("h,w", lpips_ref.HEAD_EDGE_MAPS)
@pytest.mark.parametrize("C", lpips_ref.HEAD_EDGE_C)
def test_head_widths_and_chunk_seams(vpx, parity_log, C, h, w):
    """C = 1 .. 512: lanes beyond C (and, at 65 and 100, lanes beyond C in the second register only) hold no channel; 63 / 64 / 65 pixels
    around the chunk of 64, 129 = two chunks + 1."""
    _head_checks(parity_log, C, h, w)


@pytest.mark.parametrize("scale,C,h,w", lpips_ref.HEAD_SCALED)
def test_head_norm_term_and_range(vpx, parity_log, scale, C, h, w):
    """1e-12: norms of about 1e-11, the 1e-10 of the denominator dominates; 1e25: the squares leave the fp32 range, the kernel's double
    arithmetic must not overflow. Both held to the float64 formula on the scaled float32 features."""
    _head_checks(parity_log, C, h, w, scale)


def test_head_refuses_more_than_512_channels(vpx):
    from vp_suite_amd import ops
    g = torch.Generator().manual_seed(513)
    fx, fy = torch.rand((2, 3, 3, 513), generator=g).cuda(), torch.rand((2, 3, 3, 513), generator=g).cuda()
    table = torch.tensor([3.25, -1.5], dtype=torch.float64).cuda()
    with pytest.raises(NotImplementedError, match="at most 512"):
        ops.lpips_head(fx, fy, torch.ones(513).cuda(), table=table)
    torch.cuda.synchronize()
    assert table.cpu().tolist() == [3.25, -1.5]
    assert bool(torch.isfinite(ops.lpips_head(fx[..., :512].contiguous(), fy[..., :512].contiguous(), torch.ones(512).cuda(), table=table)).all())
    assert table.cpu().tolist() != [3.25, -1.5]   # (the same call one channel narrower runs, and adds)
