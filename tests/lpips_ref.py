"""Float64 plain-torch restatement of LPIPS on an AlexNet trunk, piece by piece as csrc/lpips.hip computes it, and a seeded weight maker.

Restated from the LPIPS paper (https://arxiv.org/abs/1801.03924) and the public descriptions of the `lpips` / `piqa` packages; the project
depends on neither, so no upstream fixture pins these values (as with SSIM, tests/measure_ref.py). Written separately from
the product's host expression (measure._lpips_host): prediction and target go through the trunk on their own here, and the head is the
per-pixel formula.

    x      = clamp((v + 1) / 2, 0, 1), then (x - mean_c) / std_c (ImageNet)
    tap 1  = relu(conv 3->64 k11 s4 p2)            tap 2 = relu(conv 64->192 k5 p2 (maxpool 3/2 (tap 1)))
    tap 3  = relu(conv 192->384 k3 p1 (maxpool 3/2 (tap 2)))   tap 4 = relu(conv 384->256 k3 p1 (tap 3))   tap 5 = relu(conv 256->256 k3 p1 (tap 4))
    d_l    = mean over pixels of sum_c w_l[c] (fx / (|fx| + 1e-10) - fy / (|fy| + 1e-10))^2,   value = sum_l d_l

Feature maps are [N, C, h, w] here; the kernels keep them channels-last ([N, h, w, C]): `nhwc` / `nchw` convert."""
import functools

import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
STRIDE_PAD = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))
POOL_BEFORE = (False, True, True, False, False)
TORCHVISION_INDEX = (0, 3, 6, 8, 10)


def make_weights(seed=0):
    """{canonical key: float32 tensor}. Convolution weights are zero-mean normal with He scaling and the biases small, so that about half
    of the ReLUs fire at every tap whatever the (non-negative) input of a layer is (test_lpips_host asserts it); linear weights |randn|."""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for i, shape in enumerate(CONV_SHAPES, 1):
        fan_in = shape[1] * shape[2] * shape[3]
        w[f"conv{i}.weight"] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        w[f"conv{i}.bias"] = torch.randn(shape[0], generator=g) * 0.05
        w[f"lin{i}.weight"] = torch.randn(shape[0], generator=g).abs()
    return w


@functools.lru_cache(maxsize=None)
def weights(seed=0):
    """The seeded weights, made once and shared (never modified by a test)."""
    return make_weights(seed)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def normalise(x):
    """[N,3,H,W] in the model's range -> ImageNet-normalised, float64."""
    x = ((x.double() + 1) / 2).clamp(0.0, 1.0)
    return (x - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)


def stem(x, w, b):
    """Tap 1 [N,64,h,w]: the padding ring of the convolution is zero in normalised space."""
    return F.relu(F.conv2d(normalise(x), w.double(), b.double(), stride=4, padding=2))


def maxpool(x):
    return F.max_pool2d(x.double(), kernel_size=3, stride=2, padding=0, ceil_mode=False)


def taps(x, wts):
    """The five taps [N,C_l,h_l,w_l] (float64) of images x [N,3,H,W]."""
    f, out = normalise(x), []
    for i in range(5):
        if POOL_BEFORE[i]:
            f = maxpool(f)
        s, p = STRIDE_PAD[i]
        f = F.relu(F.conv2d(f, wts[f"conv{i + 1}.weight"].double(), wts[f"conv{i + 1}.bias"].double(), stride=s, padding=p))
        out.append(f)
    return out


def head(fx, fy, w):
    """[N]: mean over the pixels of sum_c w[c] (fx_hat - fy_hat)^2 for maps [N,C,h,w]."""
    fx, fy = fx.double(), fy.double()
    nx = fx / (fx.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
    ny = fy / (fy.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
    return ((nx - ny).pow(2) * w.double().view(1, -1, 1, 1)).sum(dim=1).flatten(1).mean(dim=1)


def lpips_frames(pred, target, wts):
    """[B, T] float64."""
    b, t = pred.shape[:2]
    tx, ty = taps(pred.reshape(-1, *pred.shape[2:]), wts), taps(target.reshape(-1, *target.shape[2:]), wts)
    return sum(head(fx, fy, wts[f"lin{i + 1}.weight"]) for i, (fx, fy) in enumerate(zip(tx, ty))).view(b, t)


def tap_tables(pred, target, wts):
    """The five [B, T] float64 tables, one per tap: lpips_frames is their sum."""
    b, t = pred.shape[:2]
    tx, ty = taps(pred.reshape(-1, *pred.shape[2:]), wts), taps(target.reshape(-1, *target.shape[2:]), wts)
    return [head(fx, fy, wts[f"lin{i + 1}.weight"]).view(b, t) for i, (fx, fy) in enumerate(zip(tx, ty))]


def tap_tables_f32(pred, target, wts):
    """The five per-tap [B, T] tables of the same chain in plain float32 torch on the CPU."""
    b, t = pred.shape[:2]
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)

    def run(x):
        f, out = (((x.float() + 1) / 2).clamp(0.0, 1.0) - mean) / std, []
        for i in range(5):
            if POOL_BEFORE[i]:
                f = F.max_pool2d(f, 3, 2)
            s, p = STRIDE_PAD[i]
            f = F.relu(F.conv2d(f, wts[f"conv{i + 1}.weight"], wts[f"conv{i + 1}.bias"], stride=s, padding=p))
            out.append(f)
        return out

    terms = []
    for i, (fx, fy) in enumerate(zip(run(pred.reshape(-1, *pred.shape[2:])), run(target.reshape(-1, *target.shape[2:])))):
        nx = fx / (fx.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        ny = fy / (fy.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        terms.append(((nx - ny).pow(2) * wts[f"lin{i + 1}.weight"].view(1, -1, 1, 1)).sum(dim=1).flatten(1).mean(dim=1).view(b, t))
    return terms


def lpips_frames_f32(pred, target, wts):
    """The same chain in plain float32 torch on the CPU: its distance from the float64 restatement is the reference-side error that the
    end-to-end bound of the GPU tests is derived from."""
    total = 0
    for term in tap_tables_f32(pred, target, wts):
        total = total + term
    return total


def relmax(got, ref):
    """max|got - ref| / max|ref| (the metric every tolerance in tests/ is stated in)."""
    return float((got.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def frames(shape, seed, scale=1.3):
    """(pred, target) in [-scale, scale]: beyond [-1, 1] the clamp acts."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale, (torch.rand(shape, generator=g) * 2 - 1) * scale


E2E_CASES = ((1, 1, 31, 31), (2, 3, 35, 47), (2, 2, 64, 64))   # (B, T, H, W)
E2E_MARGIN = 4.0   # an equally valid fp32 summation order in each of five chained layers


@functools.lru_cache(maxsize=None)
def e2e_case(case):
    """(pred, target, float64 table, reference-side error, bound) of an end-to-end case: bound = E2E_MARGIN x the max-normalised error
    of the plain float32 chain against the float64 restatement, same inputs, same weights, measured here on the CPU."""
    B, T, H, W = case
    pred, target = frames((B, T, 3, H, W), seed=1000 + H * W + B)
    ref = lpips_frames(pred, target, weights())
    ref_err = relmax(lpips_frames_f32(pred, target, weights()), ref)
    return pred, target, ref, ref_err, E2E_MARGIN * ref_err


# ---- per-tap geometry table ----------------------------------------------------------------------------------------------------------
# (B, T, H, W) -> the (h, w) of taps 1 .. 5 the case must reach, STATED here (tests/test_lpips_host.py holds them to the formula
# tap 1 = (n - 7) // 4 + 1, each pool (n - 3) // 2 + 1, and to the shapes taps() returns). The stem works in 8x8 output tiles and the
# head in chunks of 64 pixels:
#   31x31    7x7   -> 3x3   -> 1x1    the minimum: one stem tile, every deep map one pixel
#   39x71    9x17  -> 4x8   -> 1x3    one output row / column past a stem seam on each axis, two seams in W; even pool inputs (floor mode
#                                     drops a row and a column); a non-square deep map; 153 pixels at tap 1: two head chunks + 25
#   67x38    16x8  -> 7x3   -> 3x1    exactly on the seam in H, one tile in W, H > W
#   128x96   31x23 -> 15x11 -> 7x5    four tiles per side in H, three in W; deep maps larger than the 3x3 window; 713 pixels at tap 1
GEOMETRY_CASES = ((1, 1, 31, 31), (2, 2, 39, 71), (2, 2, 67, 38), (1, 2, 128, 96))
GEOMETRY_TAPS = {(1, 1, 31, 31): ((7, 7), (3, 3), (1, 1), (1, 1), (1, 1)),
                 (2, 2, 39, 71): ((9, 17), (4, 8), (1, 3), (1, 3), (1, 3)),
                 (2, 2, 67, 38): ((16, 8), (7, 3), (3, 1), (3, 1), (3, 1)),
                 (1, 2, 128, 96): ((31, 23), (15, 11), (7, 5), (7, 5), (7, 5))}
TAP_FLOOR = 1e-6     # the two-rounding noise of a [B,T] table of double sums over fp32 features
TAP_CEILING = 1e-4   # a derived bound above it fails the case (a condition on the inputs, tests/test_lpips_host.py), it is never used
# Seed revisions that were turned down, {case: {revision: why}}; a case runs on the first revision that is not listed.
REJECTED_SEEDS = {}


def tap_sizes(H, W):
    """((h, w) of taps 1 .. 5) by the formula."""
    h, w = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    deep = ((h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1)
    return ((h, w), (h2, w2), deep, deep, deep)


def isolated(wts, tap):
    """The weights with every lin{k}.weight zeroed but lin{tap}.weight: the measure's table is then tap `tap`'s share alone."""
    return {k: (torch.zeros_like(v) if k.startswith("lin") and k != f"lin{tap}.weight" else v) for k, v in wts.items()}


@functools.lru_cache(maxsize=None)
def geometry_case(case):
    """(pred, target, the five float64 tap tables, the five reference-side errors, the five bounds) of a geometry case. Per tap:
    bound = max(E2E_MARGIN x the max-normalised error of the float32 CPU chain's tap table against the float64 one, TAP_FLOOR), measured
    from the two references alone."""
    B, T, H, W = case
    rev = 1 + max(REJECTED_SEEDS.get(case, {-1: ""}))
    pred, target = frames((B, T, 3, H, W), seed=2000 + H * W + B + 100000 * rev)
    ref = tap_tables(pred, target, weights())
    errs = tuple(relmax(g, r) for g, r in zip(tap_tables_f32(pred, target, weights()), ref))
    return pred, target, ref, errs, tuple(max(E2E_MARGIN * e, TAP_FLOOR) for e in errs)


# ---- the four trunk convolutions as the measure calls them: ReLU(conv) in exact fp32, N = 4, on the deep maps of the table above ------
TRUNK_LAYERS = ((64, 192, 5, 2), (192, 384, 3, 1), (384, 256, 3, 1), (256, 256, 3, 1))   # (Ci, Co, k, pad) of taps 2 .. 5
TRUNK_MAPS = ((1, 1), (1, 3), (3, 1), (3, 3), (7, 5))
TRUNK_N = 4
TRUNK_TOL = 1e-5     # the project's bar for fp32 convolution outputs


@functools.lru_cache(maxsize=None)
def trunk_case(layer, h, w):
    """(x [N,Ci,h,w] >= 0, weight, bias, float64 pre-activation) of trunk layer `layer` (0 .. 3) on the seeded AlexNet weights: the input is
    non-negative, as after a ReLU and a pool."""
    Ci, Co, k, pad = TRUNK_LAYERS[layer]
    g = torch.Generator().manual_seed(7000 + layer * 100 + h * 10 + w)
    x = torch.rand((TRUNK_N, Ci, h, w), generator=g) * 1.5
    wt, b = weights()[f"conv{layer + 2}.weight"], weights()[f"conv{layer + 2}.bias"]
    return x, wt, b, F.conv2d(x.double(), wt.double(), b.double(), stride=1, padding=pad)


# ---- stem, pool and head edges -------------------------------------------------------------------------------------------------------
STEM_EDGE_SIZES = ((7, 7), (7, 10), (10, 7), (39, 71), (67, 38))
STEM_EDGE_KINDS = ("noise", "constant", "bounds")
STEM_PINNED = ((0, 0, -1.0), (3, 3, 1.0), (-1, -1, 1.0), (0, -1, -1.0), (-1, 0, 1.0))   # (y, x, value): the clamp's own bounds, all channels


@functools.lru_cache(maxsize=None)
def stem_edge_case(N, H, W, kind):
    """(x, float64 tap 1). noise: uniform in [-1.4, 1.4] with the pixels of STEM_PINNED held at exactly -1.0 / +1.0; constant: -1 everywhere;
    bounds: every value exactly -1.0 or +1.0."""
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + N + 500000)
    if kind == "constant":
        x = torch.full((N, 3, H, W), -1.0)
    elif kind == "bounds":
        x = (torch.rand((N, 3, H, W), generator=g) < 0.5).float() * 2 - 1
    else:
        x = (torch.rand((N, 3, H, W), generator=g) * 2 - 1) * 1.4
        for y, xx, v in STEM_PINNED:
            x[:, :, y, xx] = v
    w = weights()
    return x, stem(x, w["conv1.weight"], w["conv1.bias"])


POOL_EDGE_MAPS = ((4, 4), (5, 5), (6, 9), (9, 6))
POOL_EDGE_C = (1, 5, 64)


def pool_edge_case(C, h, w, N=2):
    """Mixed signs [N,C,h,w]."""
    return torch.randn((N, C, h, w), generator=torch.Generator().manual_seed(C * 1000 + h * 10 + w))


HEAD_EDGE_C = (1, 5, 63, 65, 100, 512)
HEAD_EDGE_MAPS = ((1, 1), (7, 9), (8, 8), (5, 13), (3, 43))   # 1, 63, 64, 65 and 129 pixels: around the chunk of 64, two chunks + 1
HEAD_EDGE_N = 3
HEAD_SCALED = ((1e-12, 100, 5, 13), (1e-12, 256, 3, 3), (1e25, 100, 5, 13), (1e25, 256, 3, 3))   # (scale, C, h, w)


@functools.lru_cache(maxsize=None)
def head_edge_case(C, h, w, scale=1.0):
    """(fx, fy, lin, float64 [N]) with fx, fy = scale * relu(randn) in float32 and one all-zero feature vector on each side (where the map has
    more than one pixel; at 1x1 the first and the last image hold one). The reference reads the SCALED float32 features."""
    g = torch.Generator().manual_seed(90000 + C * 100 + h * 10 + w)
    fx, fy = torch.relu(torch.randn((HEAD_EDGE_N, C, h, w), generator=g)), torch.relu(torch.randn((HEAD_EDGE_N, C, h, w), generator=g))
    if C > 1:   # (at C = 1 the ReLU has left zero vectors already)
        fx[0, :, 0, 0] = 0.0
        fy[-1, :, -1, -1] = 0.0
    fx, fy = fx * scale, fy * scale
    lin = torch.randn(C, generator=g).abs()
    return fx, fy, lin, head(fx, fy, lin)
