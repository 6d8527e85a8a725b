"""Image-wise measures and their providers (vp_suite/measure/image_wise.py, loss_provider.py, metric_provider.py).

Every measure here is a mean over frames of a PER-FRAME value, so two HIP passes serve all of them (csrc/measure.hip): one yields the
per-frame sums of d^2, |d| and smooth-L1(d) (MSE, L1, SmoothL1, PSNR), one the per-frame SSIM. A loss provider with any mix of
terms runs each pass once (and one gradient pass each); a metric provider derives every prediction horizon from the same two tables
by prefix means and transfers the results once. Host (CPU) tensors take the plain-torch expression of the same definitions.

The MSE with the reference's reduction (sum over c,h,w -> mean over t -> mean over b; base_measure.py:57, image_wise.py:19-27) keeps
its own kernel, which writes d/dpred in the same pass: `mse_measure`, and a provider configured with "mse" alone.

LPIPS runs on AlexNet weights the USER registers (register_lpips_weights: a dict, an .npz or a .pth file; nothing is ever downloaded):
a third per-frame table, from csrc/lpips.hip on the GPU (a training loss too once registered with differentiable=True). Until weights
are registered its registry entry raises NotImplementedError, as FVD's always does: this build ships no pretrained network."""
import os

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


class _Unavailable(VPMeasure):
    def __init__(self, device):
        raise NotImplementedError(f"{self.NAME} needs pretrained weights that this build does not ship")


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


class FrechetVideoDistance(_Unavailable):
    NAME = "Frechet Video Distance (FVD)"
    REFERENCE = "https://arxiv.org/abs/1812.01717"


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
    differentiable=True, which makes it a loss term with a HIP backward."""

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
            frames = _frame_values({k: m for k, (m, _) in self.losses.items()}, pred, target)
            values = {k: v.mean(dim=1).mean(dim=0) for k, v in frames.items()}
        for key, (m, scale) in self.losses.items():
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
        if not self.metrics:
            return [{} for _ in range(frames if all_frame_cnts else 1)]
        values = _frame_values(self.metrics, pred[:, :frames], target[:, :frames])
        table = torch.stack([values[k] for k in self.metrics])                       # [K, B, frames]
        if all_frame_cnts:   # horizon n = mean over b of the mean over the first n frames
            counts = torch.arange(1, frames + 1, device=table.device, dtype=table.dtype)
            table = (table.cumsum(dim=2) / counts).mean(dim=1)                       # [K, frames]
        else:
            table = table.mean(dim=2).mean(dim=1, keepdim=True)                      # [K, 1]
        host = table.cpu().tolist()                                                  # the one transfer
        return [{f"{k} ({'↑' if m.BIGGER_IS_BETTER else '↓'})": m.to_display(host[i][n]) for i, (k, m) in enumerate(self.metrics.items())}
                for n in range(len(host[0]))]
