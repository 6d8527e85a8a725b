"""Image-wise measures and their providers (vp_suite/measure/image_wise.py, loss_provider.py, metric_provider.py).

Every measure here is a mean over frames of a PER-FRAME value, so two HIP passes serve all of them (csrc/measure.hip): one yields the
per-frame sums of d^2, |d| and smooth-L1(d) (MSE, L1, SmoothL1, PSNR), one the per-frame SSIM. A loss provider with any mix of
terms runs each pass once (and one gradient pass each); a metric provider derives every prediction horizon from the same two tables
by prefix means and transfers the results once. Host (CPU) tensors take the plain-torch expression of the same definitions.

The MSE with the reference's reduction (sum over c,h,w -> mean over t -> mean over b; base_measure.py:57, image_wise.py:19-27) keeps
its own kernel, which writes d/dpred in the same pass: `mse_measure`, and a provider configured with "mse" alone.

LPIPS runs on AlexNet weights the USER registers (register_lpips_weights: a dict, an .npz or a .pth file; nothing is ever downloaded):
a third per-frame table, from csrc/lpips.hip on the GPU (a training loss too once registered with differentiable=True). Until weights
are registered its registry entry raises NotImplementedError: this build ships no pretrained network.

FVD likewise runs on Inception-I3D weights the USER registers (register_fvd_weights; channel widths read from the tensors, BatchNorm folded
at registration): not a per-frame table but one distance per clip chunk, from csrc/fvd.hip on the GPU (forward only), computed by the
providers beside the tables. Until weights are registered "fvd" raises NotImplementedError everywhere."""
import os
import warnings

import torch
import torch.nn.functional as F
from torch import nn


def _check_5d(name, pred, target):
    if pred.ndim != 5 or target.ndim != 5:
        raise ValueError(f"{name} expects 5-D inputs!")
    if pred.shape != target.shape:
        raise ValueError("Output images and target images are of different shape!")


def mse_measure(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    if pred.ndim != 5 or target.ndim != 5:
        raise ValueError("Mean Squared Error (MSE) / L2 Loss expects 5-D inputs!")
    if pred.is_cuda:  # one HIP pass producing the value and d/dpred (train_tail.hip)
        from . import ops
        return ops.mse_loss(pred, target)
    # host tensors (data-pipeline side checks, gloo tests): the reference's own expression
    return ((pred - target) ** 2).sum(dim=(4, 3, 2)).mean(dim=1).mean(dim=0)


# ---- per-frame tables ----------------------------------------------------------------------------------------------------------
SSIM_WINDOW, SSIM_SIGMA, SSIM_C1, SSIM_C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2   # piqa.ssim.SSIM() defaults, value range 1


def frame_sums(pred, target):
    """[3, B, T]: sums over (c,h,w) of d^2, |d| and smooth-L1(d) (beta = 1), d = pred - target (float64 from the kernel)."""
    _check_5d("frame_sums", pred, target)
    if pred.is_cuda:
        from . import ops
        return ops.pixel_measures(pred, target)
    return torch.stack([F.mse_loss(pred, target, reduction="none").sum(dim=(4, 3, 2)), F.l1_loss(pred, target, reduction="none").sum(dim=(4, 3, 2)),
                        F.smooth_l1_loss(pred, target, reduction="none").sum(dim=(4, 3, 2))])


def _ssim_host(pred, target):
    """[B, T] on host tensors: piqa's SSIM() defaults restated (Gaussian window applied separably per channel without padding)."""
    b, t, c, _, _ = pred.shape
    x = ((pred.reshape(-1, *pred.shape[2:]) + 1) / 2).clamp(min=0.0, max=1.0)   # base_measure.py:71-74
    y = ((target.reshape(-1, *target.shape[2:]) + 1) / 2).clamp(min=0.0, max=1.0)
    k = torch.arange(SSIM_WINDOW, dtype=x.dtype) - SSIM_WINDOW // 2
    k = torch.exp(-(k / SSIM_SIGMA) ** 2 / 2)
    k = k / k.sum()

    def blur(z):
        z = F.conv2d(z, k.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
        return F.conv2d(z, k.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)

    mx, my = blur(x), blur(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = blur(x * x) - mxx, blur(y * y) - myy, blur(x * y) - mxy
    ss = (2 * mxy + SSIM_C1) / (mxx + myy + SSIM_C1) * ((2 * sxy + SSIM_C2) / (sxx + syy + SSIM_C2))
    return ss.flatten(1).mean(dim=-1).view(b, t)


def frame_ssim(pred, target, name="Structural Similarity (SSIM)"):
    """[B, T]: SSIM of every frame (3-channel frames, channels at dim 2, at least 11x11)."""
    _check_5d(name, pred, target)
    if pred.shape[2] != 3:
        raise ValueError(f"{name} needs 3-channel images with the channels at dim 2")
    if pred.shape[3] < SSIM_WINDOW or pred.shape[4] < SSIM_WINDOW:
        raise ValueError(f"{name} needs images of at least {SSIM_WINDOW}x{SSIM_WINDOW} pixels (the window is applied without padding)")
    if pred.is_cuda:
        from . import ops
        return ops.ssim_frames(pred, target)
    return _ssim_host(pred, target)


# ---- LPIPS: weights a user brings, the host expression, the per-frame table ---------------------------------------------------------
# Restated from the LPIPS paper (https://arxiv.org/abs/1801.03924) and the public descriptions of the `lpips` / `piqa` packages, neither
# of which this project depends on: no upstream fixture pins these values (as with SSIM).
LPIPS_NAME = "Learned Perceptual Image Patch Similarity (LPIPS)"
LPIPS_MEAN, LPIPS_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                  # ImageNet normalisation
LPIPS_CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))   # torchvision's AlexNet.features
LPIPS_MIN_SIDE = 31                                                                   # below it the third tap has no pixel
_TORCHVISION_FEATURES = (0, 3, 6, 8, 10)                                              # features.{i}: the five convolutions
_lpips_weights = None   # canonical {key: host tensor} once registered
_lpips_on_device = {}   # (device, dtype) -> the same on a device
_lpips_differentiable = False   # register_lpips_weights(differentiable=True): a GPU prediction that requires grad runs the training call


def _lpips_canonical_key(key):
    """The canonical name of a key of one of the accepted layouts, or None."""
    parts = key.split(".")
    if len(parts) == 2 and parts[1] in ("weight", "bias") and parts[0][:4] == "conv" and parts[0][4:] in tuple("12345"):
        return key
    if len(parts) == 2 and parts[1] == "weight" and parts[0][:3] == "lin" and parts[0][3:] in tuple("12345"):
        return key
    if len(parts) == 3 and parts[0] == "features" and parts[2] in ("weight", "bias") and parts[1].isdigit() and int(parts[1]) in _TORCHVISION_FEATURES:
        return f"conv{_TORCHVISION_FEATURES.index(int(parts[1])) + 1}.{parts[2]}"
    if len(parts) == 4 and parts[1:] == ["model", "1", "weight"] and parts[0][:3] == "lin" and parts[0][3:] in tuple("01234"):   # the `lpips` package
        return f"lin{int(parts[0][3:]) + 1}.weight"
    return None


def _lpips_load(source):
    if isinstance(source, dict):
        return source
    path = os.fspath(source)
    if path.endswith(".npz"):
        import numpy as np
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    if path.endswith(".pth"):
        return torch.load(path, map_location="cpu", weights_only=True)
    raise ValueError(f"LPIPS weights: {path!r} is neither a dict, an .npz nor a .pth file")


def register_lpips_weights(source, linear_source=None, differentiable=False):
    """Registers the AlexNet trunk and the five linear layers LPIPS runs on; from then on "lpips" works wherever a measure key is accepted.
    source (and, where the linear layers live in a file of their own, as upstream keeps them, linear_source): a dict, an .npz file or a
    .pth file (read with torch.load(weights_only=True)). Accepted keys: conv{1..5}.weight / .bias and lin{1..5}.weight ([C] or [1,C,1,1]);
    torchvision's features.{0,3,6,8,10}.weight / .bias; the `lpips` package's lin{0..4}.model.1.weight. Other keys are ignored. Every shape
    is checked before anything is stored (ValueError naming the key and both shapes). Nothing is ever downloaded.
    differentiable=True makes LPIPS a training loss on the GPU: a prediction that requires grad under grad mode then runs
    ops.lpips_frames_diff, which keeps the five taps of prediction and target until its backward has run (memory an evaluation call does
    not hold) and hands the gradient to the prediction alone. With the default, and for every prediction without grad, the call and its
    bits are the evaluation's, and a prediction that requires grad is refused."""
    global _lpips_weights, _lpips_differentiable
    found = {}
    for src in (source, linear_source):
        if src is None:
            continue
        for key, value in _lpips_load(src).items():
            name = _lpips_canonical_key(key) if isinstance(key, str) else None
            if name is None:
                continue
            t = torch.as_tensor(value).detach().cpu()
            i = int(name[name.index(".") - 1]) - 1
            want = LPIPS_CONV_SHAPES[i] if name.startswith("conv") and name.endswith("weight") else (LPIPS_CONV_SHAPES[i][0],)
            if name.startswith("lin") and tuple(t.shape) == (1, want[0], 1, 1):
                t = t.reshape(want)
            if tuple(t.shape) != want:
                raise ValueError(f"LPIPS weights: {key!r} has shape {tuple(t.shape)}, expected {want}" + (f" or {(1, want[0], 1, 1)}" if name.startswith("lin") else ""))
            if not t.is_floating_point():
                raise ValueError(f"LPIPS weights: {key!r} has dtype {t.dtype}, expected a floating-point tensor")
            found[name] = t.clone().contiguous()
    from .ops import LPIPS_KEYS
    missing = [k for k in LPIPS_KEYS if k not in found]
    if missing:
        raise ValueError(f"LPIPS weights: no tensor for {missing} (accepted key layouts: see register_lpips_weights)")
    _lpips_weights = {k: found[k] for k in LPIPS_KEYS}
    _lpips_differentiable = bool(differentiable)
    _lpips_on_device.clear()


def clear_lpips_weights():
    """Forgets the registered weights and the differentiable flag: "lpips" raises NotImplementedError again."""
    global _lpips_weights, _lpips_differentiable
    _lpips_weights = None
    _lpips_differentiable = False
    _lpips_on_device.clear()


def lpips_weights(device="cpu", dtype=torch.float32):
    """The registered weights {canonical key: tensor} on `device` in `dtype` (moved once per device and dtype)."""
    if _lpips_weights is None:
        raise NotImplementedError(f"{LPIPS_NAME} needs pretrained weights that this build does not ship (register_lpips_weights)")
    slot = (str(torch.device(device)), dtype)
    if slot not in _lpips_on_device:
        _lpips_on_device[slot] = {k: v.to(device=device, dtype=dtype) for k, v in _lpips_weights.items()}
    return _lpips_on_device[slot]


def _lpips_host(pred, target, weights):
    """[B, T] on host tensors: the definition in plain torch, in the inputs' dtype."""
    b, t = pred.shape[:2]
    mean, std = pred.new_tensor(LPIPS_MEAN).view(1, 3, 1, 1), pred.new_tensor(LPIPS_STD).view(1, 3, 1, 1)
    f = torch.cat([pred.reshape(-1, *pred.shape[2:]), target.reshape(-1, *target.shape[2:])])   # one batch of 2 B T images
    f = (((f + 1) / 2).clamp(min=0.0, max=1.0) - mean) / std                                 # base_measure.py:71-74, then ImageNet
    out = 0
    for i in range(5):
        k = LPIPS_CONV_SHAPES[i][2]
        if i in (1, 2):
            f = F.max_pool2d(f, 3, 2)
        f = F.relu(F.conv2d(f, weights[f"conv{i + 1}.weight"], weights[f"conv{i + 1}.bias"], stride=4 if i == 0 else 1, padding=k // 2 if i else 2))
        n = f / (f.square().sum(dim=1, keepdim=True).sqrt() + 1e-10)
        d = (n[:b * t] - n[b * t:]).square() * weights[f"lin{i + 1}.weight"].view(1, -1, 1, 1)
        out = out + d.sum(dim=1).mean(dim=(1, 2))
    return out.view(b, t)


def frame_lpips(pred, target, name=LPIPS_NAME):
    """[B, T]: LPIPS of every frame on the registered weights (3-channel frames, channels at dim 2, at least 31x31). On the GPU a
    prediction that requires grad under grad mode is refused (NotImplementedError) unless the weights were registered with
    differentiable=True: then it runs ops.lpips_frames_diff, same values, gradient to the prediction."""
    _check_5d(name, pred, target)
    if pred.shape[2] != 3:
        raise ValueError(f"{name} needs 3-channel images with the channels at dim 2")
    if pred.shape[3] < LPIPS_MIN_SIDE or pred.shape[4] < LPIPS_MIN_SIDE:
        raise ValueError(f"{name} needs images of at least {LPIPS_MIN_SIDE}x{LPIPS_MIN_SIDE} pixels (below that the third tap has no pixel)")
    if pred.is_cuda:
        from . import ops
        if _lpips_differentiable and ops.needs_grad(pred):
            return ops.lpips_frames_diff(pred, target, lpips_weights(pred.device)).float()
        return ops.lpips_frames(pred, target, lpips_weights(pred.device)).float()   # (the kernel's table is float64)
    return _lpips_host(pred, target, lpips_weights("cpu", pred.dtype))


def _frame_table(kind, pred, target, name):
    if kind == "ssim":
        return frame_ssim(pred, target, name)
    if kind == "lpips":
        return frame_lpips(pred, target, name)
    return frame_sums(pred, target)


# ---- measures --------------------------------------------------------------------------------------------------------------------
class VPMeasure(nn.Module):
    """base_measure.py: a measure returns lower-is-better values; to_display() converts to the measure's usual representation.
    Every measure is the mean over b of the mean over t of `frame_values` — which is what the providers share between measures."""
    NAME: str = NotImplemented
    REFERENCE: str = None
    BIGGER_IS_BETTER = False
    OPT_VALUE = 0.
    TABLE = "sums"   # the per-frame table the measure is derived from: "sums" (frame_sums), "ssim" (frame_ssim) or "lpips" (frame_lpips)
    ROW = 0          # row of the sums table

    def __init__(self, device):
        super().__init__()
        self.device = device

    def frame_values(self, table, frame_elems):
        """[B, T] per-frame values (lower is better) from the measure's table."""
        return table[self.ROW].float()

    def forward(self, pred, target):
        _check_5d(self.NAME, pred, target)
        table = _frame_table(self.TABLE, pred, target, self.NAME)
        return self.frame_values(table, pred[0, 0].numel()).mean(dim=1).mean(dim=0)

    @classmethod
    def to_display(cls, x):
        return x


class MSE(VPMeasure):
    NAME = "Mean Squared Error (MSE) / L2 Loss"

    def forward(self, pred, target):
        _check_5d(self.NAME, pred, target)
        return mse_measure(pred, target)   # value and gradient in one pass


class L1(VPMeasure):
    NAME = "Mean Absolute Error (MAE) / L1 Loss"
    ROW = 1


class SmoothL1(VPMeasure):
    NAME = "Smooth L1 Loss"
    ROW = 2


class PSNR(VPMeasure):
    """image_wise.py:65-71: mean over frames of 10 log10(per-frame mean squared error); display value is its negative."""
    NAME = "Peak Signal to Noise Ratio (PSNR)"
    BIGGER_IS_BETTER = True
    OPT_VALUE = float("inf")

    def frame_values(self, table, frame_elems):
        return (torch.log10(table[0] / frame_elems) * 10).float()

    @classmethod
    def to_display(cls, x):
        return -x


class SSIM(VPMeasure):
    """image_wise.py:113-117: 1 - mean over all frames of the SSIM; display value is the SSIM itself."""
    NAME = "Structural Similarity (SSIM)"
    REFERENCE = "https://ieeexplore.ieee.org/document/1284395"
    BIGGER_IS_BETTER = True
    OPT_VALUE = 1
    TABLE = "ssim"

    def frame_values(self, table, frame_elems):
        return 1.0 - table

    @classmethod
    def to_display(cls, x):
        return 1.0 - x


class LPIPS(VPMeasure):
    """image_wise.py's LPIPS: the mean over all frames of the AlexNet LPIPS value, on weights the user registered (register_lpips_weights);
    without them the constructor raises NotImplementedError, as it always did."""
    NAME = LPIPS_NAME
    REFERENCE = "https://arxiv.org/abs/1801.03924"
    TABLE = "lpips"

    def __init__(self, device):
        lpips_weights()   # NotImplementedError until weights are registered
        super().__init__(device)

    def frame_values(self, table, frame_elems):
        return table


# ---- FVD: I3D weights a user brings, the host expression, the chunk rule ------------------------------------------------------------------
FVD_NAME = "Frechet Video Distance (FVD)"
FVD_MIN_T, FVD_MAX_T, FVD_SIDE, FVD_BN_EPS = 9, 16, 224, 1e-3
FVD_BLOCKS = ("Mixed_3b", "Mixed_3c", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "Mixed_5b", "Mixed_5c")
FVD_BRANCHES = (("b0", 1), ("b1a", 1), ("b1b", 3), ("b2a", 1), ("b2b", 3), ("b3b", 1))   # the units of an Inception block and their kernel side
# InceptionI3d up to its logits: ("unit", name, kernel, stride) | ("pool", kernel, stride) | ("block", name). The topology is fixed, the
# channel widths are read from the registered tensors.
FVD_SEQUENCE = ((("unit", "Conv3d_1a_7x7", (7, 7, 7), (2, 2, 2)), ("pool", (1, 3, 3), (1, 2, 2)), ("unit", "Conv3d_2b_1x1", (1, 1, 1), (1, 1, 1)),
                 ("unit", "Conv3d_2c_3x3", (3, 3, 3), (1, 1, 1)), ("pool", (1, 3, 3), (1, 2, 2)))
                + tuple(("block", n) for n in FVD_BLOCKS[:2]) + (("pool", (3, 3, 3), (2, 2, 2)),)
                + tuple(("block", n) for n in FVD_BLOCKS[2:7]) + (("pool", (2, 2, 2), (2, 2, 2)),) + tuple(("block", n) for n in FVD_BLOCKS[7:]))
FVD_UNITS = tuple(u for step in FVD_SEQUENCE if step[0] != "pool" for u in ((step[1],) if step[0] == "unit" else tuple(f"{step[1]}.{b}" for b, _ in FVD_BRANCHES)))
_fvd_weights = None    # {unit: (folded weight, bias) float64 on the host, "logits": (weight [F, C], bias)} once registered
_fvd_on_device = {}    # device -> what the trunk reads there


def _fvd_unit_kernel(unit):
    for step in FVD_SEQUENCE:
        if step[0] == "unit" and step[1] == unit:
            return step[2]
    return (dict(FVD_BRANCHES)[unit.split(".")[1]],) * 3


def fvd_fold(w, gamma, beta, mean, var):
    """(weight, bias) of a Unit3D with its eval-mode BatchNorm (eps 1e-3) folded in, in float64: scale = gamma / sqrt(var + eps) goes into
    the weights, beta - mean * scale becomes the bias."""
    w, gamma, beta, mean, var = (t.double() for t in (w, gamma, beta, mean, var))
    scale = gamma / torch.sqrt(var + FVD_BN_EPS)
    return (w * scale.view(-1, 1, 1, 1, 1)).contiguous(), (beta - mean * scale).contiguous()


def register_fvd_weights(source):
    """Registers the Inception-I3D network FVD runs on; from then on "fvd" works wherever a measure key is accepted. source: a dict, an
    .npz file or a .pth file (read with torch.load(weights_only=True)) keyed as InceptionI3d.state_dict(): {unit}.conv3d.weight and
    {unit}.bn.weight / .bias / .running_mean / .running_var for Conv3d_1a_7x7, Conv3d_2b_1x1, Conv3d_2c_3x3 and Mixed_3b.b0 ... Mixed_5c.b3b,
    logits.conv3d.weight / .bias; num_batches_tracked and other keys are ignored. The topology is I3D's; the channel WIDTHS are read from the
    tensors (a thin network registers like the real one; the stem takes 2 or 3 channels) and checked for consistency before anything is
    stored: every layer's input channels against its producer's outputs, a block's four branches against the next layer's inputs (ValueError
    naming the key and both shapes). BatchNorm (eps 1e-3, running statistics) is folded here, in float64: scale = gamma / sqrt(var + eps)
    goes into the weights, beta - mean * scale becomes a bias. Nothing is ever downloaded."""
    global _fvd_weights
    raw = {k: torch.as_tensor(v).detach().cpu() for k, v in _lpips_load(source).items() if isinstance(k, str)}

    def need(key, shape=None):
        if key not in raw:
            raise ValueError(f"FVD weights: no tensor for {key!r} (expected the keys of InceptionI3d.state_dict())")
        t = raw[key]
        if not t.is_floating_point():
            raise ValueError(f"FVD weights: {key!r} has dtype {t.dtype}, expected a floating-point tensor")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"FVD weights: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t.double()

    def unit(name, c_in, producer):
        key = f"{name}.conv3d.weight"
        w = need(key)
        k = _fvd_unit_kernel(name)
        if w.ndim != 5 or tuple(w.shape[2:]) != k:
            raise ValueError(f"FVD weights: {key!r} has shape {tuple(w.shape)}, expected (Co, Ci, {k[0]}, {k[1]}, {k[2]})")
        if c_in is None:
            if w.shape[1] not in (2, 3):
                raise ValueError(f"FVD weights: {key!r} has shape {tuple(w.shape)}, expected (Co, 2 or 3, 7, 7, 7): the stem takes 2 or 3 channels")
        elif w.shape[1] != c_in:
            raise ValueError(f"FVD weights: {key!r} has shape {tuple(w.shape)}, expected ({w.shape[0]}, {c_in}, {k[0]}, {k[1]}, {k[2]}): its producer {producer}")
        co = w.shape[0]
        return fvd_fold(w, *(need(f"{name}.bn.{p}", (co,)) for p in ("weight", "bias", "running_mean", "running_var")))

    found, c, producer = {}, None, None
    for step in FVD_SEQUENCE:
        if step[0] == "unit":
            found[step[1]] = unit(step[1], c, producer)
            c, producer = found[step[1]][0].shape[0], f"{step[1] + '.conv3d.weight'!r} has shape {tuple(found[step[1]][0].shape)}"
        elif step[0] == "block":
            name, widths = step[1], {}
            for b, _ in FVD_BRANCHES:
                c_b, prod_b = (c, producer) if b in ("b0", "b1a", "b2a", "b3b") else (widths[b[:2] + "a"], f"{name + '.' + b[:2] + 'a.conv3d.weight'!r} has {widths[b[:2] + 'a']} output channels")
                found[f"{name}.{b}"] = unit(f"{name}.{b}", c_b, prod_b)
                widths[b] = found[f"{name}.{b}"][0].shape[0]
            outs = tuple(widths[b] for b in ("b0", "b1b", "b2b", "b3b"))
            c, producer = sum(outs), f"{name} ends in {outs[0]} + {outs[1]} + {outs[2]} + {outs[3]} = {sum(outs)} channels"
    w = need("logits.conv3d.weight")
    if w.ndim != 5 or tuple(w.shape[1:]) != (c, 1, 1, 1):
        raise ValueError(f"FVD weights: 'logits.conv3d.weight' has shape {tuple(w.shape)}, expected (n_features, {c}, 1, 1, 1): its producer {producer}")
    found["logits"] = (w.reshape(w.shape[0], c).contiguous(), need("logits.conv3d.bias", (w.shape[0],)).contiguous())
    _fvd_weights = found
    _fvd_on_device.clear()


def clear_fvd_weights():
    """Forgets the registered network: "fvd" raises NotImplementedError again."""
    global _fvd_weights
    _fvd_weights = None
    _fvd_on_device.clear()


def _fvd_trunk(device):
    """What ops.fvd_features reads on a GPU: the folded weights packed [kt, kh, kw, Ci, Co] and the biases as float32 tensors, and the layer
    table over four buffers (0: the staged clips; two that the maps alternate between; one for what a block's 1x1x1 units and its pool
    hand to the next unit). A block's branches write their channel ranges of ONE map: no cat."""
    from . import ops
    params, rows = [], []

    def conv(name, src, dst, k, s, coff, ld):
        w, b = _fvd_weights[name]
        rows.append((ops.FVD_CONV, src, dst, w.shape[1], w.shape[0], k, s, True, coff, w.shape[0] if ld is None else ld, len(params)))
        params.extend([ops.conv3d_pack(w.float()).to(device), b.float().to(device)])

    cur, c = 0, _fvd_weights["Conv3d_1a_7x7"][0].shape[1]
    for step in FVD_SEQUENCE:
        dst = 2 if cur == 1 else 1
        if step[0] == "unit":
            conv(step[1], cur, dst, step[2], step[3], 0, None)
            c = _fvd_weights[step[1]][0].shape[0]
        elif step[0] == "pool":
            rows.append((ops.FVD_POOL, cur, dst, c, c, step[1], step[2], False, 0, c, 0))
        else:
            name = step[1]
            co = {b: _fvd_weights[f"{name}.{b}"][0].shape[0] for b, _ in FVD_BRANCHES}
            ld, one, three = co["b0"] + co["b1b"] + co["b2b"] + co["b3b"], (1, 1, 1), (3, 3, 3)
            conv(f"{name}.b0", cur, dst, one, one, 0, ld)
            conv(f"{name}.b1a", cur, 3, one, one, 0, None)
            conv(f"{name}.b1b", 3, dst, three, one, co["b0"], ld)
            conv(f"{name}.b2a", cur, 3, one, one, 0, None)
            conv(f"{name}.b2b", 3, dst, three, one, co["b0"] + co["b1b"], ld)
            rows.append((ops.FVD_POOL, cur, 3, c, c, three, one, False, 0, c, 0))
            conv(f"{name}.b3b", 3, dst, one, one, co["b0"] + co["b1b"] + co["b2b"], ld)
            c = ld
        cur = dst
    w, b = _fvd_weights["logits"]
    rows.append((ops.FVD_HEAD, cur, cur, c, w.shape[0], (1, 1, 1), (1, 1, 1), False, 0, w.shape[0], len(params)))
    params.extend([w.float().to(device), b.float().to(device)])
    table, n_rows = ops.fvd_table(rows)
    return {"table": table, "n_rows": n_rows, "params": params, "rows": rows, "ci": _fvd_weights["Conv3d_1a_7x7"][0].shape[1], "n_features": w.shape[0]}


def fvd_weights(device="cpu", dtype=torch.float32):
    """The registered network on `device`, built once per device: on a GPU what ops.fvd_features takes (float32, weights packed for the
    kernel, the layer table); on the host {unit: (folded weight, bias), "logits": (weight [F, C], bias)} in `dtype`."""
    if _fvd_weights is None:
        raise NotImplementedError(f"{FVD_NAME} needs pretrained weights that this build does not ship (register_fvd_weights)")
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:   # "cuda" and "cuda:0" are one device: one pack
        dev = torch.device("cuda", torch.cuda.current_device())
    slot = (str(dev), dtype if dev.type == "cpu" else torch.float32)
    if slot not in _fvd_on_device:
        _fvd_on_device[slot] = {k: (w.to(dtype), b.to(dtype)) for k, (w, b) in _fvd_weights.items()} if dev.type == "cpu" else _fvd_trunk(dev)
    return _fvd_on_device[slot]


def fvd_in_channels():
    """The channel count the registered stem takes (2 or 3)."""
    fvd_weights()
    return _fvd_weights["Conv3d_1a_7x7"][0].shape[1]


def same_pad(size, k, s):
    """(front, back, out) of one axis: the reference's "SAME" rule (Unit3D.compute_pad, MaxPool3dSamePadding.compute_pad)."""
    pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return pad // 2, pad - pad // 2, -(-size // s)


def _fvd_pad(x, k, s):
    pads = [same_pad(n, kk, ss) for n, kk, ss in zip(x.shape[2:], k, s)]
    return F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))


def _fvd_unit_host(x, wb, k, s=(1, 1, 1)):
    return F.relu(F.conv3d(_fvd_pad(x, k, s), wb[0], wb[1], stride=s))


def _fvd_pool_host(x, k, s):
    return F.max_pool3d(_fvd_pad(x, k, s), k, s)   # the padding is ZERO, and part of the pooled map


def _fvd_block_host(x, weights, name):
    one, three = (1, 1, 1), (3, 3, 3)
    u = lambda b, z: _fvd_unit_host(z, weights[f"{name}.{b}"], dict(FVD_BRANCHES)[b] == 1 and one or three)
    return torch.cat([u("b0", x), u("b1b", u("b1a", x)), u("b2b", u("b2a", x)), u("b3b", _fvd_pool_host(x, three, one))], dim=1)


def _fvd_features_host(clips, weights):
    """[N, n_features] on host tensors: the trunk in plain torch on the folded weights, in the clips' dtype. clips: [N, T, C, h, w]."""
    n, t, c, h, w = clips.shape
    x = clips.reshape(n * t, c, h, w)
    if (h, w) != (FVD_SIDE, FVD_SIDE):
        x = F.interpolate(x, size=(FVD_SIDE, FVD_SIDE), mode="bilinear", align_corners=False, antialias=False)
    x = x.reshape(n, t, c, FVD_SIDE, FVD_SIDE).permute(0, 2, 1, 3, 4)
    for step in FVD_SEQUENCE:
        if step[0] == "unit":
            x = _fvd_unit_host(x, weights[step[1]], step[2], step[3])
        elif step[0] == "pool":
            x = _fvd_pool_host(x, step[1], step[2])
        else:
            x = _fvd_block_host(x, weights, step[1])
    if tuple(x.shape[2:]) != (2, 7, 7):
        raise ValueError(f"{FVD_NAME}: the final map must be 2x7x7 (got {tuple(x.shape[2:])}): clips of {FVD_MIN_T} .. {FVD_MAX_T} frames give it")
    return x.mean(dim=(2, 3, 4)) @ weights["logits"][0].t() + weights["logits"][1]


def frechet_distance_host(pred, target):
    """A float64 scalar: the reference's calculate_2_wasserstein_dist on two [b, n] tables, restated. With E the centred tables and
    fact = 1 / (b - 1) (1 for b = 1): fact sum Ep^2 + fact sum Et^2 - 2 sum_i sqrt(sigma_i^2 + 1e-15) + |mu_p - mu_t|^2, sigma_i the singular
    values of the b x b matrix fact Ep Et^T (the reference's M = M_l M_l^T is symmetric positive semidefinite with eigenvalues sigma_i^2).
    The n x n covariances are never formed."""
    if pred.ndim != 2 or pred.shape != target.shape:
        raise ValueError("Expecting equal shapes for pred and target!")
    p, t = pred.double(), target.double()
    b = p.shape[0]
    fact = 1.0 if b < 2 else 1.0 / (b - 1)
    mp, mt = p.mean(dim=0), t.mean(dim=0)
    ep, et = p - mp, t - mt
    sigma = torch.linalg.svdvals(fact * (ep @ et.t()))
    return fact * ep.square().sum() + fact * et.square().sum() - 2.0 * torch.sqrt(sigma.square() + 1e-15).sum() + (mp - mt).square().sum()


def fvd_chunks(num_frames):
    """The chunks FVD runs on for a clip length, [(first frame, length), ...], or None below 9 frames (fvd.py: calculate_n_chunks, then
    torch.chunk's sizes). Up to 16 frames: one chunk. Beyond: the number of chunks of the LAST chunk length L in 16 .. 9 whose remainder
    num_frames % L is at least 9 (num_frames // L + 1 chunks, none dropped). Where no length leaves such a remainder (17, 18 and 112 frames up
    to 128) the reference divides by a tuple and raises TypeError; this restates its evident intent: the chunk length with the largest
    remainder (the last of them among equals, as its sort orders them), num_frames // L + 1 chunks, the last one dropped."""
    if num_frames < FVD_MIN_T:
        return None
    n_chunks, drop_last = 1, False
    if num_frames > FVD_MAX_T:
        lengths = range(FVD_MAX_T, FVD_MIN_T - 1, -1)
        fitting = [l for l in lengths if num_frames % l >= FVD_MIN_T]
        if fitting:
            n_chunks = num_frames // fitting[-1] + 1
        else:
            best = sorted(((l, num_frames % l) for l in lengths), key=lambda lm: lm[1])[-1][0]
            n_chunks, drop_last = num_frames // best + 1, True
    size = -(-num_frames // n_chunks)                                   # torch.chunk: pieces of ceil(T / n), the last one shorter
    pieces = [(s, min(size, num_frames - s)) for s in range(0, num_frames, size)]
    return pieces[:n_chunks - 1 if drop_last else n_chunks]


class FrechetVideoDistance(VPMeasure):
    """fvd.py's measure on an I3D network the user registered (register_fvd_weights); without one the constructor raises NotImplementedError,
    as it always did. Not a mean over frames: prediction and target clips go through the trunk as ONE batch of 2B, the distance is taken
    between the two sets of B feature vectors, per chunk of 9 .. 16 frames (fvd_chunks), and the chunks' distances are averaged. Clips below
    9 frames give None. Forward only: a prediction that requires grad under grad mode raises NotImplementedError, on either device."""
    NAME = FVD_NAME
    REFERENCE = "https://arxiv.org/abs/1812.01717"
    TABLE = None   # no per-frame table: the providers compute it beside the tables

    def __init__(self, device):
        fvd_weights()   # NotImplementedError until weights are registered
        super().__init__(device)

    def forward(self, pred, target):
        if pred.shape != target.shape:
            raise ValueError("FrechetVideoDistance: vid shapes not equal!")
        if pred.ndim != 5:
            raise ValueError(f"{self.NAME} expects 5-D inputs!")
        chunks = fvd_chunks(pred.shape[1])
        if chunks is None:
            return None
        if pred.shape[2] != fvd_in_channels():
            raise ValueError(f"{self.NAME}: the frames have {pred.shape[2]} channels, the registered network takes {fvd_in_channels()}")
        b = pred.shape[0]
        values = []
        if torch.is_grad_enabled() and pred.requires_grad:   # on either device: a term without a gradient must not pass for a loss
            raise NotImplementedError(f"{self.NAME}: the backward is not implemented in this build (forward only): evaluate it under "
                                      f"torch.no_grad() or on detached tensors")
        if pred.is_cuda:
            from . import ops
            trunk = fvd_weights(pred.device)
            for first, length in chunks:
                feats = ops.fvd_features(pred[:, first:first + length].detach(), trunk, target[:, first:first + length].detach())
                values.append(ops.frechet_distance(feats[:b], feats[b:]))
        else:
            weights = fvd_weights("cpu", pred.dtype)
            with torch.no_grad():
                for first, length in chunks:
                    feats = _fvd_features_host(torch.cat([pred[:, first:first + length], target[:, first:first + length]]), weights)
                    values.append(frechet_distance_host(feats[:b], feats[b:]))
        return (sum(values) / len(values)).float()


LOSS_CLASSES = {"mse": MSE, "l1": L1, "smooth_l1": SmoothL1, "lpips": LPIPS, "ssim": SSIM, "psnr": PSNR, "fvd": FrechetVideoDistance}
AVAILABLE_LOSSES = LOSS_CLASSES.keys()
METRIC_CLASSES = dict(LOSS_CLASSES)
AVAILABLE_METRICS = METRIC_CLASSES.keys()
IMPLEMENTED = ("mse", "l1", "smooth_l1", "ssim", "psnr")   # what "all" means in this build


def _frame_values(measures, pred, target):
    """{key: [B, T] per-frame values}: each table the measures need is computed once."""
    tables = {}
    out = {}
    for key, m in measures.items():
        if m.TABLE not in tables:
            tables[m.TABLE] = _frame_table(m.TABLE, pred, target, m.NAME)
        out[key] = m.frame_values(tables[m.TABLE], pred[0, 0].numel())
    return out


class PredictionLossProvider:
    """config: {"device": ..., "losses_and_scales": {key: scale}} over any mix of "mse", "l1", "smooth_l1", "psnr" and "ssim"
    (loss_provider.py). All pixel-wise terms together cost one sums pass and one gradient pass, SSIM one of each. "lpips" joins them once
    weights are registered: on the GPU as a value only (a prediction that requires grad raises) unless they were registered with
    differentiable=True, which makes it a loss term with a HIP backward. "fvd" joins them once its weights are registered, as a value for
    inputs without grad (forward only); clips below 9 frames have none and add no term."""

    def __init__(self, config: dict):
        self.device = config["device"]
        scales = dict(config.get("losses_and_scales", {"mse": 1.0}))
        unknown = [k for k in scales if k not in LOSS_CLASSES]
        if unknown:
            raise NotImplementedError(f"losses {unknown} are not part of this build (available: {list(IMPLEMENTED)})")
        self.losses = {k: (LOSS_CLASSES[k](device=self.device), s) for k, s in scales.items()}

    def get_losses(self, pred, target):
        if pred.shape != target.shape:
            raise ValueError("Output images and target images are of different shape!")
        display, total = {}, torch.zeros((), device=pred.device)
        if list(self.losses) == ["mse"]:   # the fused value + gradient kernel
            values = {"mse": self.losses["mse"][0](pred, target)}
        else:
            frames = _frame_values({k: m for k, (m, _) in self.losses.items() if m.TABLE is not None}, pred, target)
            values = {k: v.mean(dim=1).mean(dim=0) for k, v in frames.items()}
            values.update({k: m(pred, target) for k, (m, _) in self.losses.items() if m.TABLE is None})   # FVD: not a per-frame table
        for key, (m, scale) in self.losses.items():
            if values[key] is None:   # FVD below 9 frames: no value, no term
                continue
            total = total + scale * values[key]
            display[key] = m.to_display(values[key])
        return display, total


class PredictionMetricProvider:
    """config: {"device": ..., "metrics": "all" | [keys]} (metric_provider.py). get_metrics returns one dict per evaluated frame count,
    keyed "mse (↓)", "ssim (↑)", ... with display values. The per-frame tables are computed once; every horizon is a prefix mean of
    them on the device, and all results reach the host in one transfer."""

    def __init__(self, config: dict):
        self.device = config["device"]
        keys = IMPLEMENTED if config["metrics"] == "all" else list(config["metrics"])
        unknown = [k for k in keys if k not in METRIC_CLASSES]
        if unknown:
            raise NotImplementedError(f"metrics {unknown} are not part of this build (available: {list(IMPLEMENTED)})")
        self.available_metrics = {k: METRIC_CLASSES[k] for k in keys}
        self.metrics = {k: metric(device=self.device) for k, metric in self.available_metrics.items()}

    @torch.no_grad()
    def get_metrics(self, pred, target, frames: int = None, all_frame_cnts: bool = False):
        if pred.ndim != 5 or target.ndim != 5:
            raise ValueError("Input tensors expected to be 5-dimensional!")
        if pred.shape != target.shape:
            raise ValueError("Output images and target images are of different shape!")
        frames = frames or pred.shape[1]
        horizons = list(range(1, frames + 1)) if all_frame_cnts else [frames]
        framewise = {k: m for k, m in self.metrics.items() if m.TABLE is not None}
        out = [{} for _ in horizons]
        if framewise:
            values = _frame_values(framewise, pred[:, :frames], target[:, :frames])
            table = torch.stack([values[k] for k in framewise])                      # [K, B, frames]
            if all_frame_cnts:   # horizon n = mean over b of the mean over the first n frames
                counts = torch.arange(1, frames + 1, device=table.device, dtype=table.dtype)
                table = (table.cumsum(dim=2) / counts).mean(dim=1)                   # [K, frames]
            else:
                table = table.mean(dim=2).mean(dim=1, keepdim=True)                  # [K, 1]
            host = table.cpu().tolist()                                              # the one transfer
            out = [{f"{k} ({'↑' if m.BIGGER_IS_BETTER else '↓'})": m.to_display(host[i][n]) for i, (k, m) in enumerate(framewise.items())}
                   for n in range(len(host[0]))]
        # FVD is no per-frame table: one value per requested horizon, present in that horizon's dict only from 9 frames on
        for k, m in self.metrics.items():
            if m.TABLE is not None:
                continue
            if pred.shape[2] != fvd_in_channels():   # (the reference drops it for frames its network cannot take)
                warnings.warn(f"metric {k!r} dropped: the frames have {pred.shape[2]} channels, the registered network takes {fvd_in_channels()}")
                continue
            computed = [(i, m(pred[:, :n], target[:, :n])) for i, n in enumerate(horizons) if n >= FVD_MIN_T]
            if computed:
                host = torch.stack([v.double() for _, v in computed]).cpu().tolist()
                for (i, _), v in zip(computed, host):
                    out[i][f"{k} ({'↑' if m.BIGGER_IS_BETTER else '↓'})"] = m.to_display(v)
        return out
