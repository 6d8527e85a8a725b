"""Plain-torch restatements of the five image-wise measures (vp_suite/measure/image_wise.py with the reductions of
base/base_measure.py), in whatever dtype the caller asks for: fp64 is what the HIP kernels are held against, fp32 gives the
reference-side error that bounds the SSIM gradient test, and tools/bench_measures.py times the fp32 form on the GPU.

SSIM: piqa is not available where this project is built and tested, so NO value here comes from piqa itself. The restatement is
written from piqa's documented SSIM() defaults (window 11, sigma 1.5, k1 = 0.01, k2 = 0.03, value range 1, Gaussian window
normalised to sum 1 and applied per channel without padding, mean over channels and positions) and Wang et al. 2004,
"Image quality assessment: from error visibility to structural similarity", eq. 13. tests/test_measure_host.py checks it against
properties that hold for any correct SSIM (identity, symmetry, the closed form on constant images)."""
import torch
import torch.nn.functional as F

KEYS = ("mse", "l1", "smooth_l1", "psnr", "ssim")
C1, C2 = 0.01 ** 2, 0.03 ** 2


def frame_sums(pred, target, dtype=torch.float64):
    """[3, B, T]: per-frame sums of d^2, |d|, smooth-L1(d) with beta = 1."""
    d = pred.to(dtype) - target.to(dtype)
    ad = d.abs()
    return torch.stack([(d * d).sum(dim=(4, 3, 2)), ad.sum(dim=(4, 3, 2)), torch.where(ad < 1, 0.5 * d * d, ad - 0.5).sum(dim=(4, 3, 2))])


def ssim_frames(pred, target, dtype=torch.float64):
    """[B, T]: SSIM of each frame; inputs in [-1, 1] mapped by clamp((x + 1) / 2, 0, 1) (base_measure.py:71-74)."""
    b, t, c = pred.shape[:3]
    x = ((pred.to(dtype).flatten(0, 1) + 1) / 2).clamp(0, 1)
    y = ((target.to(dtype).flatten(0, 1) + 1) / 2).clamp(0, 1)
    k = torch.arange(11, dtype=dtype, device=pred.device) - 5
    k = torch.exp(-k ** 2 / (2 * 1.5 ** 2))
    k = k / k.sum()
    wv, wh = k.view(1, 1, 11, 1).repeat(c, 1, 1, 1), k.view(1, 1, 1, 11).repeat(c, 1, 1, 1)

    def blur(z):
        return F.conv2d(F.conv2d(z, wv, groups=c), wh, groups=c)

    mx, my = blur(x), blur(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = blur(x * x) - mxx, blur(y * y) - myy, blur(x * y) - mxy
    ss = (2 * mxy + C1) / (mxx + myy + C1) * ((2 * sxy + C2) / (sxx + syy + C2))
    return ss.flatten(1).mean(dim=-1).view(b, t)


def frame_values(pred, target, dtype=torch.float64, keys=KEYS):
    """{key: [B, T]} per-frame values in the lower-is-better representation the measures return."""
    out = {}
    if any(k != "ssim" for k in keys):
        s = frame_sums(pred, target, dtype)
        out.update(mse=s[0], l1=s[1], smooth_l1=s[2], psnr=10 * torch.log10(s[0] / pred[0, 0].numel()))
    if "ssim" in keys:
        out["ssim"] = 1 - ssim_frames(pred, target, dtype)
    return {k: out[k] for k in keys}


def measures(pred, target, dtype=torch.float64, keys=KEYS):
    """{key: scalar}: mean over t, then over b (base_measure.py:57; image_wise.py:71, :117)."""
    return {k: v.mean(dim=1).mean(dim=0) for k, v in frame_values(pred, target, dtype, keys).items()}


def display(key, value):
    """to_display of image_wise.py: PSNR is negated back, SSIM is 1 - value."""
    return -value if key == "psnr" else (1 - value if key == "ssim" else value)


def ssim_inputs(kind, shape, seed):
    """(pred, target) fp32 [B,T,3,H,W]: 'noise' uniform in [-1.2, 1.2] (crosses both clamp bounds), 'smooth' a smooth pattern plus
    noise, 'mnist' a flat -1 background with a textured block."""
    g = torch.Generator().manual_seed(seed)
    B, T, C, H, W = shape
    if kind == "noise":
        return torch.rand(shape, generator=g) * 2.4 - 1.2, torch.rand(shape, generator=g) * 2.4 - 1.2
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 3, W), indexing="ij")
        t = (torch.sin(xx * 2 + torch.arange(C).view(C, 1, 1)) * torch.cos(yy * 1.5)).expand(B, T, C, H, W) * 1.1
        t = t * (1 + 0.1 * torch.arange(B * T).view(B, T, 1, 1, 1))
        return t + 0.2 * torch.randn(shape, generator=g), t.contiguous()
    t = -torch.ones(shape)
    t[..., H // 3:2 * H // 3, W // 3:2 * W // 3] = torch.rand(B, T, C, 2 * H // 3 - H // 3, 2 * W // 3 - W // 3, generator=g) * 2 - 1
    return (t + 0.1 * torch.randn(shape, generator=g)).clamp(-1.3, 1.3), t
