"""The kernels of csrc/fvd.hip one by one on the GPU: the "SAME" 3-D convolution against float64 F.pad + F.conv3d, the zero-padded max-pool
against torch bit for bit, the head against float64, the Frechet distance against the float64 svdvals restatement on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import fvd_ref
from vp_suite_amd import measure as M
from vp_suite_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONV_BAR = 1e-5   # exact fp32 operands: the forward bar of tests/test_gpu_conv_same.py for that form

STEM_MAPS = ((9, 13, 10), (16, 12, 9))          # both parities of the padding rule on every axis
MID_MAPS = ((2, 7, 7), (3, 5, 6), (1, 1, 1))
CONV_CASES = ([("stem", (7, 7, 7), (2, 2, 2), ci, 16, m, n) for ci in (2, 3) for m in STEM_MAPS for n in (1, 3)]
              + [("3x3x3", (3, 3, 3), (1, 1, 1), ci, co, m, n) for ci, co in ((16, 32), (24, 64), (96, 208)) for m in MID_MAPS for n in (1, 3)]
              + [("1x1x1", (1, 1, 1), (1, 1, 1), ci, co, (2, 7, 7), n) for ci in (832, 1024) for co in (1, 16, 130) for n in (1, 3)])


def _cl(x):   # [N, C, T, H, W] -> channels-last [N, T, H, W, C] on the GPU
    return x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def _cf(y):   # back, on the host
    return y.cpu().permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}-ci{c[3]}-co{c[4]}-{'x'.join(map(str, c[5]))}-n{c[6]}")
def test_conv3d_same_against_float64(case, parity_log):
    _, k, s, ci, co, (T, H, W), n = case
    g = torch.Generator().manual_seed(ci * 131 + co * 7 + T * H * W + n)
    x = torch.randn(n, ci, T, H, W, generator=g)
    w = torch.randn(co, ci, *k, generator=g) / (ci * k[0] * k[1] * k[2]) ** 0.5
    bias = torch.randn(co, generator=g) * 0.3
    xd, wd, bd = _cl(x), w.to(DEV), bias.to(DEV)
    for relu in (False, True):
        ref = fvd_ref.conv3d_same_ref(x, w, bias, s, relu)
        assert float(ref.abs().max()) > 0.1 and (not relu or ref.numel() < 16 or bool((ref == 0).any()))   # (the ReLU is at work)
        got = ops.conv3d_same(xd, wd, bd, stride=s, relu=relu)
        assert tuple(got.shape) == (n, *ref.shape[2:], co)
        err = parity_log(f"conv3d_same relu={relu}", _cf(got), ref, CONV_BAR)
        print(f"conv3d_same {case} relu={relu}: {err:.3e}")
        fvd_ref.record(f"conv3d_same {case[0]} Ci={ci} Co={co} map={T}x{H}x{W} N={n} relu={relu}", hip=err, bound=CONV_BAR)
        assert err <= CONV_BAR
        # the same call at a channel offset of a wider map: its channels equal the dense call's bits, the others stay as they were
        wide = torch.full((n, *ref.shape[2:], co + 11), -7.25, device=DEV)
        back = ops.conv3d_same(xd, wd, bd, stride=s, relu=relu, out=wide, channel_offset=5)
        assert back is wide and torch.equal(wide[..., 5:5 + co], got)
        assert bool((wide[..., :5] == -7.25).all()) and bool((wide[..., 5 + co:] == -7.25).all())
    packed = ops.conv3d_same(xd, ops.conv3d_pack(wd), bd, stride=s, relu=True, packed=True)
    assert torch.equal(packed, got)


def test_conv3d_same_refusals():
    x, w, b = torch.zeros(1, 2, 3, 3, 4, device=DEV), torch.zeros(5, 4, 1, 1, 1, device=DEV), torch.zeros(5, device=DEV)
    with pytest.raises(ValueError, match="input channels"):
        ops.conv3d_same(x, torch.zeros(5, 3, 1, 1, 1, device=DEV), b)
    with pytest.raises(ValueError, match="do not fit"):
        ops.conv3d_same(x, w, b, out=torch.zeros(1, 2, 3, 3, 6, device=DEV), channel_offset=2)
    with pytest.raises(Exception, match="GPU"):
        ops.conv3d_same(x.cpu(), w.cpu(), b.cpu())
    with pytest.raises(NotImplementedError, match="up to 15"):
        ops.conv3d_same(torch.zeros(1, 20, 3, 3, 4, device=DEV), torch.zeros(5, 4, 17, 1, 1, device=DEV), b)


POOL_FORMS = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)))


@pytest.mark.parametrize("form", POOL_FORMS, ids=lambda f: "k" + "".join(map(str, f[0])) + "s" + "".join(map(str, f[1])))
def test_maxpool3d_same_equals_torch_bit_for_bit(form):
    kernel, stride = form
    for T, H, W in STEM_MAPS + MID_MAPS:
        g = torch.Generator().manual_seed(T * 100 + H * 10 + W)
        mixed = torch.randn(2, 5, T, H, W, generator=g)
        negative = -torch.rand(2, 5, T, H, W, generator=g) - 0.25
        for name, x in (("mixed", mixed), ("negative", negative)):
            ref = fvd_ref.maxpool3d_same_ref(x, kernel, stride)
            got = _cf(ops.maxpool3d_same(_cl(x), kernel, stride))
            assert got.shape == ref.shape and torch.equal(got, ref), (name, T, H, W)
        # a window that touches the zero border returns 0 on an all-negative map, never the map's own values
        ref = fvd_ref.maxpool3d_same_ref(negative, kernel, stride)
        padded = any(sum(M.same_pad(n, k, s)[:2]) > 0 for n, k, s in zip((T, H, W), kernel, stride))
        assert float(ref.max()) <= 0 and bool((ref == 0).any()) == padded


@pytest.mark.parametrize("C,n_features", ((128, 7), (1024, 400)))
@pytest.mark.parametrize("N", (1, 5))
def test_head_against_float64(C, n_features, N, parity_log):
    g = torch.Generator().manual_seed(C + N)
    x = torch.randn(N, 2, 7, 7, C, generator=g).abs()
    w = torch.randn(n_features, C, generator=g) / C ** 0.5
    b = torch.randn(n_features, generator=g)
    ref = x.double().mean(dim=(1, 2, 3)) @ w.double().t() + b.double()
    got = ops.fvd_head(x.to(DEV), w.view(n_features, C, 1, 1, 1).to(DEV), b.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, n_features)
    bound = 2.0 ** -22   # double arithmetic, rounded once to float32 (half an ulp: 2^-24 of the value), with a factor of 4 in hand
    err = parity_log("fvd_head", got.cpu(), ref, bound)
    fvd_ref.record(f"fvd_head C={C} features={n_features} N={N}", hip=err, bound=bound)
    assert err <= bound
    for shape in ((N, 2, 7, 6, C), (N, 1, 7, 7, C), (N, 3, 7, 7, C)):
        with pytest.raises(ValueError, match="2x7x7"):
            ops.fvd_head(torch.zeros(shape, device=DEV), w.to(DEV), b.to(DEV))


@pytest.mark.parametrize("n", (7, 400))
@pytest.mark.parametrize("b", (1, 2, 3, 8, 33, ops.FVD_MAX_B))
def test_frechet_distance_against_float64_svdvals(b, n):
    for kind in fvd_ref.FRECHET_KINDS:
        p, t = fvd_ref.feature_tables(b, n, kind)
        ref = float(M.frechet_distance_host(p, t))
        got = ops.frechet_distance(p.to(DEV), t.to(DEV))
        assert got.dtype == torch.float64 and got.is_cuda and got.ndim == 0
        again = ops.frechet_distance(p.to(DEV), t.to(DEV))
        bound = fvd_ref.frechet_bound(p, t)
        print(f"frechet b={b} n={n} {kind}: value {ref:.6e}, |delta| {abs(float(got) - ref):.3e}, bound {bound:.3e}")
        fvd_ref.record(f"frechet_distance b={b} n={n} {kind}", svdvals_form=ref, abs_delta=abs(float(got) - ref), bound=bound)
        assert abs(float(got) - ref) <= bound, (kind, float(got), ref)
        assert float(got) == float(again)
        if kind == "identical":
            assert abs(float(got)) <= 2 * b * 1e-15 ** 0.5 + 1e-10 * fvd_ref.frechet_scale(p, t)


def test_frechet_distance_refuses_more_than_its_cap():
    p = torch.zeros(ops.FVD_MAX_B + 1, 7, device=DEV)
    with pytest.raises(ops.VpxError, match=str(ops.FVD_MAX_B)):
        ops.frechet_distance(p, p)
    with pytest.raises(ValueError, match="one shape"):
        ops.frechet_distance(p[:4], p[:5])
