"""UNet double-conv blocks and DCGAN convolution layers.

DoubleConv2d / DoubleConv3d — drop-in for vp_suite/model_blocks/conv.py:9-55: the reference's constructor signatures and module tree
(`conv.0` / `conv.3` the bias-free replicate-border convolutions, `conv.1` / `conv.4` the BatchNorms with their buffers). A block is two
`unet_ops.conv_bn_relu` calls on channels-last frames [B,T,H,W,C] (a 2-D block: T = 1); it can take two channel-concatenated sources
and hand out the 2x2 max-pooled map beside its result. BatchNorm follows `self.training` exactly as nn.BatchNorm does.

DCGAN convolution layers — drop-in for vp_suite/model_blocks/conv.py DCGANConv / DCGANConvTranspose: same constructor signatures and
`state_dict` keys (`main.0.*` the convolution, `main.1.*` the GroupNorm). A layer is two library calls: the convolution
(`ops.conv2d_ex`, no activation) and the fused GroupNorm(16) + LeakyReLU(0.2) (`phy_ops.group_norm`), which can also add a residual
after the activation (PhyDNet folds `decoded_phys + decoded_conv` into it). Activations stay channels-last."""
from torch import nn

from .. import ops, phy_ops, unet_ops
from ..base import VPModelBlock

GN_GROUPS = 16
LEAKY_SLOPE = 0.2


class _DoubleConv(VPModelBlock):
    PAPER_REFERENCE = "arxiv.org/abs/1505.04597"

    def forward(self, x, x2=None, pool=False):
        """x (, x2): [B,T,H,W,C] frames, read as one channel-concatenated input. Returns the block's result, or (result, pooled)."""
        c = self.conv
        h = unet_ops.conv_bn_relu(x, c[0].weight, c[1], b=x2)
        return unet_ops.conv_bn_relu(h, c[3].weight, c[4], pool=pool)


class DoubleConv2d(_DoubleConv):
    NAME = "DoubleConv2d"

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=(3, 3), stride=(1, 1), padding=1,
                      padding_mode='replicate', bias=False),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(in_channels=out_channels, out_channels=out_channels, kernel_size=(3, 3), stride=(1, 1), padding=1,
                      padding_mode='replicate', bias=False),
            nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
        )


class DoubleConv3d(_DoubleConv):
    NAME = "DoubleConv3d"

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv3d(in_channels=in_channels, out_channels=out_channels, kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=1,
                      padding_mode='replicate', bias=False),
            nn.BatchNorm3d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv3d(in_channels=out_channels, out_channels=out_channels, kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=1,
                      padding_mode='replicate', bias=False),
            nn.BatchNorm3d(out_channels),
            nn.ReLU(inplace=True),
        )


class DCGANConv(VPModelBlock):
    NAME = "DCGAN - Conv"
    PAPER_REFERENCE = "arxiv.org/abs/1511.06434"
    precision = "f32"   #: arithmetic of the convolution ("f32" | "bf16x3")

    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        self.stride = stride
        self.main = nn.Sequential(
            nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=(3, 3), stride=stride, padding=1),
            nn.GroupNorm(GN_GROUPS, out_channels),
            nn.LeakyReLU(LEAKY_SLOPE, inplace=True),
        )

    def forward(self, x, residual=None):
        conv, gn = self.main[0], self.main[1]
        y = ops.conv2d_ex(x, conv.weight, conv.bias, self.stride, 1, precision=self.precision)
        return phy_ops.group_norm(y, gn.num_groups, gn.weight, gn.bias, leaky_slope=LEAKY_SLOPE, residual=residual)


class DCGANConvTranspose(VPModelBlock):
    NAME = "DCGAN - ConvTranspose"
    PAPER_REFERENCE = "arxiv.org/abs/1511.06434"
    precision = "f32"

    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        self.stride = stride
        self.output_pad = int(stride == 2)
        self.main = nn.Sequential(
            nn.ConvTranspose2d(in_channels=in_channels, out_channels=out_channels, kernel_size=(3, 3), stride=stride, padding=1,
                               output_padding=(self.output_pad, self.output_pad)),
            nn.GroupNorm(GN_GROUPS, out_channels),
            nn.LeakyReLU(LEAKY_SLOPE, inplace=True),
        )

    def forward(self, x, residual=None):
        conv, gn = self.main[0], self.main[1]
        y = ops.conv2d_ex(x, conv.weight, conv.bias, self.stride, 1, transposed=True, precision=self.precision,
                          output_padding=(self.output_pad, self.output_pad))
        return phy_ops.group_norm(y, gn.num_groups, gn.weight, gn.bias, leaky_slope=LEAKY_SLOPE, residual=residual)
