"""DCGAN encoder / decoder — drop-in for vp_suite/model_blocks/enc.py DCGANEncoder / DCGANDecoder (same constructor signatures,
`state_dict` keys `c1.main.0.weight`, ..., `upc3.weight`), on the library's convolution and GroupNorm kernels.

Restriction: the reference ends the decoder with `Resize(out_size)`. That is the identity exactly when the frame's height and width are
divisible by 4 (two stride-2 layers down, two up), and only that case is supported: any other `out_size` raises ValueError at
construction instead of resampling."""
from torch import nn

from .. import ops
from ..base import VPModelBlock
from .conv import DCGANConv, DCGANConvTranspose


class DCGANEncoder(VPModelBlock):
    NAME = "DCGAN Encoder"
    PAPER_REFERENCE = "arxiv.org/abs/1511.06434"

    def __init__(self, img_channels=1, enc_channels=32):
        super().__init__()
        self.c1 = DCGANConv(img_channels, enc_channels, stride=2)
        self.c2 = DCGANConv(enc_channels, enc_channels, stride=1)
        self.c3 = DCGANConv(enc_channels, 2 * enc_channels, stride=2)

    def forward(self, x):
        return self.c3(self.c2(self.c1(x)))


class DCGANDecoder(VPModelBlock):
    NAME = "DCGAN Decoder"
    PAPER_REFERENCE = "arxiv.org/abs/1511.06434"
    precision = "f32"

    def __init__(self, out_size, img_channels=1, enc_channels=32):
        super().__init__()
        out_size = tuple(int(s) for s in out_size)
        if len(out_size) != 2 or out_size[0] % 4 or out_size[1] % 4:
            raise ValueError(f"DCGANDecoder: output size {out_size} is not divisible by 4; the reference's Resize path for such "
                             f"sizes is not supported")
        self.out_size = out_size
        self.upc1 = DCGANConvTranspose(2 * enc_channels, enc_channels, stride=2)
        self.upc2 = DCGANConvTranspose(enc_channels, enc_channels, stride=1)
        self.upc3 = nn.ConvTranspose2d(in_channels=enc_channels, out_channels=img_channels, kernel_size=(3, 3), stride=2, padding=1,
                                       output_padding=1)

    def forward(self, x):
        """The decoder's output before the model's sigmoid (channels-last)."""
        if tuple(x.shape[-2:]) != (self.out_size[0] // 4, self.out_size[1] // 4):
            raise ValueError(f"DCGANDecoder: input {tuple(x.shape)} does not decode to {self.out_size}")
        d = self.upc2(self.upc1(x))
        return ops.conv2d_ex(d, self.upc3.weight, self.upc3.bias, 2, 1, transposed=True, precision=self.precision, output_padding=(1, 1))
