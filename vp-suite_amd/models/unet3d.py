"""UNet-3D ("unet-3d") — drop-in for vp_suite/models/unet3d.py: the reference's class constants, hyper-parameters (`features`,
`temporal_dim`), `state_dict` (128 entries, 671 185 parameters at 1x64x64 with temporal_dim 4; BatchNorm buffers included) and
`forward(x, pred_frames) -> (pred [b,p,c,h,w], None)`, which slides a window of `temporal_dim` frames autoregressively, on the library's
kernels: replicate-border convolutions with BatchNorm + ReLU (unet_ops / csrc/unet3d.hip), the time collapse of the skip connections, and
`ops.conv2d_ex` for the 2x2 stride-2 transposed convolutions and the final 1x1 layer. No ATen convolution, normalisation, pooling or
activation runs over activations; the up path's `cat(skip, x)` is never materialised.

BatchNorm is the reference's (nn.BatchNorm2d / 3d defaults): in train() mode batch statistics (biased variance), with the running mean /
unbiased variance updated with momentum 0.1 and `num_batches_tracked` incremented once per `pred_1`, i.e. `pred_frames` times per
forward; in eval() mode the running statistics, applied in the convolutions' epilogues.

Divergences, stated loudly:
  * `action_conditional=True` raises NotImplementedError and `CAN_HANDLE_ACTIONS = False` (the reference: True);
  * a frame height or width that is not a multiple of 2**len(features) raises ValueError at construction (the reference resizes the
    up-sampled map with torchvision there);
  * `temporal_dim < 1` raises ValueError at construction, fewer context frames than `temporal_dim` in `pred_1`;
  * arithmetic is exact fp32 only: `precision = "f32"`, anything else raises ValueError;
  * an eval()-mode call that needs gradients raises VpxError (the eval epilogue has no backward);
  * one value per channel in training raises ValueError, as torch does."""
import torch
from torch import nn

from .. import ops, unet_ops
from ..base import VPModel
from ..model_blocks.conv import DoubleConv2d, DoubleConv3d


class UNet3D(VPModel):
    NAME = "UNet-3D"
    REQUIRED_ARGS = ["img_shape", "action_size", "tensor_value_range", "temporal_dim"]
    CAN_HANDLE_ACTIONS = False   # (the reference: True — see the module docstring)

    features = [8, 16, 32, 64]  #: Channel dimensionality per encoding/decoding stage
    temporal_dim = None  #: Number of consecutive frames used for 3D convolution
    precision = "f32"  #: arithmetic of the convolutions (exact fp32 only)

    def __init__(self, device, **model_kwargs):
        super().__init__(device, **model_kwargs)
        if self.precision != "f32":
            raise ValueError(f"UNet3D: precision must be 'f32', got {self.precision!r}")
        if self.action_conditional:
            raise NotImplementedError("UNet3D: the action-conditional variant is not implemented")
        if not isinstance(self.temporal_dim, int) or self.temporal_dim < 1:
            raise ValueError(f"UNet3D: temporal_dim must be a positive integer, got {self.temporal_dim!r}")
        self.features = [int(f) for f in self.features]
        if not self.features or min(self.features) < 1:
            raise ValueError(f"UNet3D: features must be a non-empty list of positive channel counts, got {self.features}")
        step = 2 ** len(self.features)
        if self.img_h % step or self.img_w % step:
            raise ValueError(f"UNet3D: frame size {self.img_h}x{self.img_w} is not a multiple of {step} (2**len(features)); the reference "
                             f"would resize the up-sampled maps there, which this port does not do")
        self.MIN_CONTEXT_FRAMES = self.temporal_dim
        self.downs = nn.ModuleList()
        self.ups = nn.ModuleList()
        self.time3ds = nn.ModuleList()
        self.pool = nn.MaxPool3d(kernel_size=(1, 2, 2), stride=(1, 2, 2))   # (the reference's attribute; the pooled maps come from bn_relu)

        cur_in_channels = self.img_c
        for feature in self.features:
            self.downs.append(DoubleConv3d(in_channels=cur_in_channels, out_channels=feature))
            self.time3ds.append(nn.Conv3d(in_channels=feature, out_channels=feature, kernel_size=(self.temporal_dim, 1, 1)))
            cur_in_channels = feature
        bn_feat = self.features[-1]
        self.time3ds.append(nn.Conv3d(in_channels=bn_feat, out_channels=bn_feat, kernel_size=(self.temporal_dim, 1, 1)))
        self.bottleneck = DoubleConv2d(in_channels=bn_feat, out_channels=bn_feat * 2)
        for feature in reversed(self.features):
            self.ups.append(nn.ConvTranspose2d(in_channels=feature * 2, out_channels=feature, kernel_size=(2, 2), stride=(2, 2)))
            self.ups.append(DoubleConv2d(in_channels=feature * 2, out_channels=feature))
        self.final_conv = nn.Conv2d(in_channels=self.features[0], out_channels=self.img_c, kernel_size=(1, 1))
        self.to(self.device)

    def pred_1(self, x, **kwargs):
        if x.dim() != 5 or tuple(x.shape[2:]) != (self.img_c, self.img_h, self.img_w):
            raise ValueError(f"UNet3D: expected frames [b,t,{self.img_c},{self.img_h},{self.img_w}], got {tuple(x.shape)}")
        if x.shape[1] < self.temporal_dim:
            raise ValueError(f"UNet3D: {x.shape[1]} context frames, temporal_dim={self.temporal_dim} needs at least as many")
        ops.require_gpu(x, "UNet3D")
        x = x[:, -self.temporal_dim:].permute(0, 1, 3, 4, 2).contiguous()   # [b, temporal_dim, h, w, c]: channels-last frames

        skips = []
        for down, t3d in zip(self.downs, self.time3ds):
            full, x = down(x, pool=True)
            skips.append(unet_ops.time_collapse(full, t3d.weight, t3d.bias))   # [b, 1, h, w, f]
        x = unet_ops.time_collapse(x, self.time3ds[-1].weight, self.time3ds[-1].bias)
        x = self.bottleneck(x)

        for i in range(0, len(self.ups), 2):
            up, skip = self.ups[i], skips[-1 - i // 2]
            # [b,1,h,w,C] frames are the memory of a channels-last [b,C,h,w] tensor: views both ways, no copy
            y = ops.conv2d_ex(x.squeeze(1).permute(0, 3, 1, 2), up.weight, up.bias, 2, 0, transposed=True)
            x = self.ups[i + 1](skip, y.permute(0, 2, 3, 1).unsqueeze(1))
        return ops.conv2d_ex(x.squeeze(1).permute(0, 3, 1, 2), self.final_conv.weight, self.final_conv.bias, 1, 0)

    def forward(self, x, pred_frames=1, **kwargs):
        preds = []
        for _ in range(pred_frames):
            pred = self.pred_1(x).unsqueeze(dim=1)
            preds.append(pred)
            x = torch.cat([x[:, 1:], pred], dim=1)
        return torch.cat(preds, dim=1), None
