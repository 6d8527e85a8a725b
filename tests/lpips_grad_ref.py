"""Float64 references for the LPIPS gradient (csrc/lpips.hip's backward): autograd through tests/lpips_ref.py, whose pieces are plain
torch. Nothing here looks at the library.

A case is (B, T, H, W) with seeded frames of its own (GRAD_REJECTED_SEEDS lists the seed revisions that were turned down, as
lpips_ref.REJECTED_SEEDS does) and a seeded float64 cotangent over [B, T]. Its bound is lpips_ref.E2E_MARGIN times the max-normalised
error of plain float32 CPU autograd over the same chain against the float64 gradient, measured here; tests/test_lpips_grad_host.py
holds the conditions on the inputs (bound under the ceiling, nothing near a kink)."""
import functools

import torch
import torch.nn.functional as F

import lpips_ref

E2E_GRAD_CASES = ((1, 1, 31, 31), (2, 2, 39, 71), (2, 2, 67, 38), (2, 3, 35, 47))   # GEOMETRY_CASES 31x31, 39x71, 67x38 and E2E_CASES (2, 3, 35, 47)
TAP_GRAD_CASES = E2E_GRAD_CASES[:3]
GRAD_CEILING = 1e-4
KINK_FACTOR = 10.0
# {case: {revision: why}}; a case runs on the first revision that is not listed
GRAD_REJECTED_SEEDS = {
    (1, 1, 31, 31): {0: "relu 1: margin 1.8e-05 within ten times the float32 error 6.4e-06"},
    (2, 2, 39, 71): {0: "pool 1: margin 3.5e-05 within ten times the float32 error 7.3e-06",
                     1: "relu 1: margin 2.1e-05 within ten times the float32 error 5.9e-06"},
    (2, 3, 35, 47): {0: "relu 1: margin 3.9e-05 within ten times the float32 error 5.8e-06"},
}


def case_inputs(case):
    """(pred, target, cotangent [B,T] float64) of a case."""
    B, T, H, W = case
    rev = 1 + max(GRAD_REJECTED_SEEDS.get(case, {-1: ""}))
    pred, target = lpips_ref.frames((B, T, 3, H, W), seed=3000 + H * W + B + 100000 * rev)
    cot = torch.randn((B, T), generator=torch.Generator().manual_seed(77 + H * W + B), dtype=torch.float64)
    return pred, target, cot


def grad64(pred, target, cot, wts):
    p = pred.detach().double().clone().requires_grad_()
    (lpips_ref.lpips_frames(p, target, wts) * cot).sum().backward()
    return p.grad


def grad32(pred, target, cot, wts):
    p = pred.detach().float().clone().requires_grad_()
    (lpips_ref.lpips_frames_f32(p, target, wts) * cot.float()).sum().backward()
    return p.grad


@functools.lru_cache(maxsize=None)
def grad_case(case, tap=None):
    """(pred, target, cotangent, float64 gradient, reference-side error, bound); tap 1 .. 5: on lpips_ref.isolated weights, that tap's
    share alone."""
    pred, target, cot = case_inputs(case)
    wts = lpips_ref.weights() if tap is None else lpips_ref.isolated(lpips_ref.weights(), tap)
    ref = grad64(pred, target, cot, wts)
    ref_err = lpips_ref.relmax(grad32(pred, target, cot, wts), ref)
    return pred, target, cot, ref, ref_err, lpips_ref.E2E_MARGIN * ref_err


def kink_margins(case):
    """The distances of the prediction's chain from its kinks, each next to the float32 chain's own error there:
    {"relu k": (min |pre-activation| of tap k, max |float32 - float64| of it), "pool k": (min gap between a window's maximum and its
    runner-up over the windows with a positive maximum, max |float32 - float64| of the tap), "clamp": (min distance of a pixel from
    -1 and +1, the spacing of float32 at 2: what (v + 1) / 2 can be off by)}."""
    pred, _, _ = case_inputs(case)
    x = pred.reshape(-1, *pred.shape[2:])
    wts = lpips_ref.weights()
    out = {"clamp": (float(torch.minimum((x.double() - 1).abs(), (x.double() + 1).abs()).min()), 2.0 ** -22)}
    mean, std = torch.tensor(lpips_ref.MEAN).view(1, 3, 1, 1), torch.tensor(lpips_ref.STD).view(1, 3, 1, 1)
    f64, f32 = lpips_ref.normalise(x), (((x.float() + 1) / 2).clamp(0.0, 1.0) - mean) / std
    for i in range(5):
        if lpips_ref.POOL_BEFORE[i]:
            err = float((f32.double() - f64).abs().max())
            win = F.unfold(f64, kernel_size=3, stride=2).view(f64.shape[0], f64.shape[1], 9, -1)   # [N, C, 9, windows]
            top = win.topk(2, dim=2).values
            live = top[:, :, 0] > 0   # an all-zero window hands its gradient to an element the ReLU mask removes, whichever it is
            out[f"pool {i}"] = (float((top[:, :, 0] - top[:, :, 1])[live].min()), err)
            f64, f32 = lpips_ref.maxpool(f64), F.max_pool2d(f32, 3, 2)
        s, p = lpips_ref.STRIDE_PAD[i]
        w, b = wts[f"conv{i + 1}.weight"], wts[f"conv{i + 1}.bias"]
        pre64, pre32 = F.conv2d(f64, w.double(), b.double(), stride=s, padding=p), F.conv2d(f32, w, b, stride=s, padding=p)
        out[f"relu {i + 1}"] = (float(pre64.abs().min()), float((pre32.double() - pre64).abs().max()))
        f64, f32 = F.relu(pre64), F.relu(pre32)
    return out


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
HEAD_BWD_TOL = 2.0 ** -23    # the arithmetic is double on float32 features: what is left is the rounding of the float32 result, doubled;
#                              head_bwd_bound adds the float64 reference's own error, which is not small where the expression cancels
STEM_BWD_TOL = 1e-5          # the project's bar for fp32 convolution outputs (lpips_ref.TRUNK_TOL): sums of up to 576 products
POOL_BWD_ULPS = 3 * 4        # at most four window gradients meet in an element: three float32 additions of sums of at most 4 max|dy|


def head_bwd_ref(fx, fy, lin, dtable, incoming=None):
    """[N,C,h,w] float64: where(fx > 0, incoming + d(sum_i dtable[i] head(fx, fy, lin)[i]) / d fx, 0). (At an all-zero vector autograd's
    own derivative of the norm is NaN; the mask, a select, drops it.)"""
    f = fx.double().requires_grad_()
    (lpips_ref.head(f, fy, lin) * dtable).sum().backward()
    g = f.grad if incoming is None else f.grad + incoming.double()
    return torch.where(fx > 0, g, torch.zeros_like(g))


def head_bwd_formula(fx, fy, lin, dtable, incoming=None):
    """The same gradient from the closed form, in float64: with s = |fx|, r = 1 / (s + 1e-10), u_c = 2 w_c (fx_c r - fy_c / (|fy| + 1e-10)):
    (dtable[i] / HW) (r u_c - fx_c r^2 (sum_k u_k fx_k) / s). Where the expression cancels (one channel: fx r is 1 - 1e-10 / s, and so is
    the other side) two float64 evaluations agree to a few digits only: their distance is the reference's own error there."""
    x, y = fx.double(), fy.double()
    s = x.pow(2).sum(dim=1, keepdim=True).sqrt()
    r, q = 1.0 / (s + 1e-10), 1.0 / (y.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
    u = 2.0 * lin.double().view(1, -1, 1, 1) * (x * r - y * q)
    k = torch.where(s > 0, r * r * (u * x).sum(dim=1, keepdim=True) / s.clamp_min(1e-300), torch.zeros_like(s))
    g = dtable.view(-1, 1, 1, 1) / (fx.shape[2] * fx.shape[3]) * (r * u - x * k)
    if incoming is not None:
        g = g + incoming.double()
    return torch.where(fx > 0, g, torch.zeros_like(g))


def head_bwd_bound(fx, fy, lin, dtable, incoming=None):
    """(float64 gradient by autograd, bound): HEAD_BWD_TOL plus lpips_ref.E2E_MARGIN x the distance between the two float64 evaluations."""
    ref = head_bwd_ref(fx, fy, lin, dtable, incoming)
    return ref, HEAD_BWD_TOL + lpips_ref.E2E_MARGIN * lpips_ref.relmax(head_bwd_formula(fx, fy, lin, dtable, incoming), ref)


def first_max_pool_bwd(x, dy):
    """The tie rule written out: every 3x3 stride-2 window hands its gradient to the FIRST of its maximal elements in row-major order.
    x [N,C,h,w], dy [N,C,ho,wo] -> [N,C,h,w] float64."""
    x, dy = x.double(), dy.double()
    dx = torch.zeros_like(x)
    for oy in range(dy.shape[2]):
        for ox in range(dy.shape[3]):
            win = x[:, :, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3].reshape(x.shape[0], x.shape[1], 9)
            first = (win == win.max(dim=2, keepdim=True).values).float().argmax(dim=2)   # argmax of a 0 / 1 mask: its first 1
            for k in range(9):
                dx[:, :, 2 * oy + k // 3, 2 * ox + k % 3] += torch.where(first == k, dy[:, :, oy, ox], torch.zeros_like(dy[:, :, oy, ox]))
    return dx


def pool_bwd_autograd(x, dy):
    """torch's CPU max_pool2d backward in float64."""
    v = x.double().requires_grad_()
    (lpips_ref.maxpool(v) * dy.double()).sum().backward()
    return v.grad


POOL_BWD_KINDS = ("noise", "ties", "equal")


def pool_bwd_case(C, h, w, kind, N=2):
    """(x [N,C,h,w], dy): noise = lpips_ref.pool_edge_case; ties = values in {-1, 0, 1}, so that most windows hold their maximum more
    than once; equal = one constant, every window tied nine ways."""
    g = torch.Generator().manual_seed(31000 + C * 1000 + h * 10 + w)
    if kind == "noise":
        x = lpips_ref.pool_edge_case(C, h, w, N)
    elif kind == "ties":
        x = torch.randint(-1, 2, (N, C, h, w), generator=g).float()
    else:
        x = torch.full((N, C, h, w), 0.75)
    return x, torch.randn((N, C, (h - 3) // 2 + 1, (w - 3) // 2 + 1), generator=g)


def stem_bwd_ref(x, w, dz):
    """[N,3,H,W] float64: the gradient at x of sum(dz * pre-activation of tap 1), through clamp and normalisation; dz [N,64,Ho,Wo]."""
    v = x.double().requires_grad_()
    (F.conv2d(lpips_ref.normalise(v), w.double(), None, stride=4, padding=2) * dz.double()).sum().backward()
    return v.grad


def stem_uncovered(H, W):
    """(first row, first column) that no window of the stem covers (== H, W when every one is covered)."""
    return tuple(min(n, 4 * ((n - 7) // 4 + 1) + 5) for n in (H, W))
