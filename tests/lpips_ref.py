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


def lpips_frames_f32(pred, target, wts):
    """The same chain in plain float32 torch on the CPU: its distance from the float64 restatement is the reference-side error that the
    end-to-end bound of the GPU tests is derived from."""
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

    total = 0
    for i, (fx, fy) in enumerate(zip(run(pred.reshape(-1, *pred.shape[2:])), run(target.reshape(-1, *target.shape[2:])))):
        nx = fx / (fx.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        ny = fy / (fy.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        total = total + ((nx - ny).pow(2) * wts[f"lin{i + 1}.weight"].view(1, -1, 1, 1)).sum(dim=1).flatten(1).mean(dim=1)
    return total.view(b, t)


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
