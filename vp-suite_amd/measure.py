"""Image-wise measures and their providers (vp_suite/measure/image_wise.py, loss_provider.py, metric_provider.py).

Every measure here is a mean over frames of a PER-FRAME value, so two HIP passes serve all of them (csrc/measure.hip): one yields the
per-frame sums of d^2, |d| and smooth-L1(d) (MSE, L1, SmoothL1, PSNR), one the per-frame SSIM. A loss provider with any mix of
terms runs each pass once (and one gradient pass each); a metric provider derives every prediction horizon from the same two tables
by prefix means and transfers the results once. Host (CPU) tensors take the plain-torch expression of the same definitions.

The MSE with the reference's reduction (sum over c,h,w -> mean over t -> mean over b; base_measure.py:57, image_wise.py:19-27) keeps
its own kernel, which writes d/dpred in the same pass: `mse_measure`, and a provider configured with "mse" alone.

LPIPS and FVD need pretrained networks this build does not ship: their registry entries raise NotImplementedError."""
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


# ---- measures --------------------------------------------------------------------------------------------------------------------
class VPMeasure(nn.Module):
    """base_measure.py: a measure returns lower-is-better values; to_display() converts to the measure's usual representation.
    Every measure is the mean over b of the mean over t of `frame_values` — which is what the providers share between measures."""
    NAME: str = NotImplemented
    REFERENCE: str = None
    BIGGER_IS_BETTER = False
    OPT_VALUE = 0.
    TABLE = "sums"   # the per-frame table the measure is derived from: "sums" (frame_sums) or "ssim" (frame_ssim)
    ROW = 0          # row of the sums table

    def __init__(self, device):
        super().__init__()
        self.device = device

    def frame_values(self, table, frame_elems):
        """[B, T] per-frame values (lower is better) from the measure's table."""
        return table[self.ROW].float()

    def forward(self, pred, target):
        _check_5d(self.NAME, pred, target)
        table = frame_ssim(pred, target, self.NAME) if self.TABLE == "ssim" else frame_sums(pred, target)
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


class LPIPS(_Unavailable):
    NAME = "Learned Perceptual Image Patch Similarity (LPIPS)"
    REFERENCE = "https://arxiv.org/abs/1801.03924"


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
            tables[m.TABLE] = frame_ssim(pred, target, m.NAME) if m.TABLE == "ssim" else frame_sums(pred, target)
        out[key] = m.frame_values(tables[m.TABLE], pred[0, 0].numel())
    return out


class PredictionLossProvider:
    """config: {"device": ..., "losses_and_scales": {key: scale}} over any mix of "mse", "l1", "smooth_l1", "psnr" and "ssim"
    (loss_provider.py). All pixel-wise terms together cost one sums pass and one gradient pass, SSIM one of each."""

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
