"""DCGAN encoder / decoder — drop-in for vp_suite/model_blocks/enc.py DCGANEncoder / DCGANDecoder (same constructor signatures,
`state_dict` keys `c1.main.0.weight`, ..., `upc3.weight`), on the library's convolution and GroupNorm kernels.

Restriction: the reference ends the decoder with `Resize(out_size)`. That is the identity exactly when the frame's height and width are
divisible by 4 (two stride-2 layers down, two up), and only that case is supported: any other `out_size` raises ValueError at
construction instead of resampling.

`Autoencoder`, `Encoder`, `Decoder` (ST-Phy's, enc.py:14-97): the same constructor signatures, `encoded_shape`, `encoded_numel`,
`encode` / `decode` and state-dict keys. Every layer is one library convolution with ReLU in its epilogue (`stphy_ops.conv2d_act`);
`mean_layer` runs without activation and hands its output to the encoder-tail kernel (`stphy_ops.relu_rownorm`: relu + L2
normalisation of every image row, along W). `encoded_shape` is the closed form of the three unpadded layers, so the block builds
on "cpu". The reference's `Resize` at the decoder's end is the identity exactly when 4 * h3 + 16 == H (every multiple of 4 from 20
up); `Decoder` raises ValueError for any other size."""
import torch
from torch import nn

from .. import ops, stphy_ops
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


def _encoded_hw(n):
    """Side length after Encoder's three unpadded layers (5x5 stride 2, 3x3 stride 2, 3x3 stride 1)."""
    return ((((n - 5) // 2 + 1) - 3) // 2 + 1) - 2


class Encoder(VPModelBlock):
    NAME = "Encoder"
    precision = "f32"

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.conv1 = nn.Conv2d(in_channels=self.in_channels, out_channels=32, kernel_size=5, stride=2)
        self.conv2 = nn.Conv2d(in_channels=32, out_channels=64, kernel_size=3, stride=2)
        self.mean_layer = nn.Conv2d(in_channels=64, out_channels=self.out_channels, kernel_size=3, stride=1)

    def forward(self, x):
        x = stphy_ops.conv2d_act(x, self.conv1.weight, self.conv1.bias, 2, 0, act="relu", precision=self.precision)
        x = stphy_ops.conv2d_act(x, self.conv2.weight, self.conv2.bias, 2, 0, act="relu", precision=self.precision)
        x = stphy_ops.conv2d_act(x, self.mean_layer.weight, self.mean_layer.bias, 1, 0, act=None, precision=self.precision)
        return stphy_ops.relu_rownorm(x, eps=1e-8)


class Decoder(VPModelBlock):
    NAME = "Decoder"
    precision = "f32"

    def __init__(self, in_channels, out_shape):
        super().__init__()
        self.in_channels = in_channels
        self.out_c, self.out_h, self.out_w = (int(s) for s in out_shape)
        for name, n in (("height", self.out_h), ("width", self.out_w)):
            if n < 20 or 4 * _encoded_hw(n) + 16 != n:
                raise ValueError(f"Decoder: output {name} {n} is not reproduced by the three transposed layers (4 * h3 + 16, every "
                                 f"multiple of 4 from 20 up); the reference's Resize path for such sizes is not supported")
        self.fc1 = nn.Conv2d(self.in_channels, self.in_channels, kernel_size=1, stride=1)
        self.conv1 = nn.ConvTranspose2d(self.in_channels, 64, kernel_size=6, stride=2, padding=0)
        self.conv2 = nn.ConvTranspose2d(64, 32, kernel_size=6, stride=2, padding=0)
        self.conv3 = nn.ConvTranspose2d(32, self.out_c, kernel_size=5, stride=1, padding=0)

    def forward(self, x):
        if tuple(x.shape[-2:]) != (_encoded_hw(self.out_h), _encoded_hw(self.out_w)):
            raise ValueError(f"Decoder: input {tuple(x.shape)} does not decode to {(self.out_h, self.out_w)}")
        x = stphy_ops.conv2d_act(x, self.fc1.weight, self.fc1.bias, 1, 0, act="relu", precision=self.precision)
        x = stphy_ops.conv2d_act(x, self.conv1.weight, self.conv1.bias, 2, 0, transposed=True, act="relu", precision=self.precision)
        x = stphy_ops.conv2d_act(x, self.conv2.weight, self.conv2.bias, 2, 0, transposed=True, act="relu", precision=self.precision)
        return stphy_ops.conv2d_act(x, self.conv3.weight, self.conv3.bias, 1, 0, transposed=True, act=None, precision=self.precision)


class Autoencoder(VPModelBlock):
    NAME = "Autoencoder"

    def __init__(self, img_shape, encoded_channels, device):
        super().__init__()
        self.img_shape = img_shape
        self.img_c, self.img_h, self.img_w = img_shape
        self.enc_c = encoded_channels
        self.device = device
        self.build_models()
        self.to(self.device)
        self.encoded_shape = torch.Size((1, self.enc_c, _encoded_hw(self.img_h), _encoded_hw(self.img_w)))
        self.encoded_numel = self.encoded_shape.numel()

    def build_models(self):
        self.encoder = Encoder(in_channels=self.img_c, out_channels=self.enc_c)
        self.decoder = Decoder(in_channels=self.enc_c, out_shape=self.img_shape)

    def encode(self, x):
        return self.encoder(x)

    def decode(self, x):
        return self.decoder(x)
