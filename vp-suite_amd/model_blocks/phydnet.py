"""PhyDNet's ConvLSTM branch — drop-in for `SingleStepConvLSTM` (vp_suite/model_blocks/phydnet.py:117-175): a stack of
`ConvLSTMCell`s (conv_lstm_ndrplz.py:7-48, bias=True) that consumes ONE frame per call and keeps its (H, C) lists
between calls. The constructor signature, the public attributes (`H`, `C`, `cell_list`, ...) and the return convention
`((H, C), H)` are the reference's contract; the body is this package's:

  * a layer step is one fused cell launch of the library (`vpx_convlstm_seq_fwd`, T = 1, gate order i,f,o,g);
  * the step right after `init_hidden` passes NO state to the library (NULL = zeros): the kernel then skips the whole
    recurrent half of the contraction instead of multiplying a zero tensor, and nothing is read for c;
  * the action plane is written into the channel tail of one preallocated channels-last input buffer (no expand + cat pair).

The rest of PhyDNet's blocks follow (`PhyCell_Cell`, `PhyCell`, `EncoderSplit`, `DecoderSplit`): the reference's attributes and
`state_dict` keys on the library's convolution (`ops.conv2d_ex`), GroupNorm and PhyCell-correction kernels (`phy_ops`)."""
import math

import torch
from torch import nn

from .. import ops, phy_ops
from ..base import VPModelBlock
from .conv import DCGANConv, DCGANConvTranspose
from .conv_lstm_ndrplz import ConvLSTMCell


class SingleStepConvLSTM(nn.Module):
    def __init__(self, input_size, input_dim, hidden_dims, n_layers, kernel_size, action_conditional, action_size, device):
        super().__init__()
        self.input_size, self.input_dim, self.hidden_dims = input_size, input_dim, hidden_dims
        self.n_layers, self.kernel_size = n_layers, kernel_size
        self.action_conditional, self.action_size, self.device = action_conditional, action_size, device
        widths = [input_dim + (action_size if action_conditional else 0)] + list(hidden_dims[:n_layers])
        self.cell_list = nn.ModuleList(ConvLSTMCell(input_dim=cin, hidden_dim=ch, kernel_size=kernel_size, bias=True)
                                       for cin, ch in zip(widths[:-1], widths[1:]))
        self.H, self.C = [], []
        self._pristine = []   # the zero tensors handed out by init_hidden, while nobody has replaced or written them

    def _is_untouched_zero(self, j):
        """True while layer j's state still is the zero pair of init_hidden (same objects, never written in place)."""
        return (j < len(self._pristine) and self.H[j] is self._pristine[j][0] and self.C[j] is self._pristine[j][1]
                and self.H[j]._version == 0 and self.C[j]._version == 0)

    def _bottom_input(self, frame, action):
        if not self.action_conditional:
            return frame
        b, (hh, ww) = frame.size(0), self.input_size
        buf = ops.new_channels_last((b, self.input_dim + self.action_size, hh, ww), frame.device)
        buf[:, :self.input_dim].copy_(frame)
        buf[:, self.input_dim:].copy_(action[:, :, None, None].expand(b, self.action_size, hh, ww))
        return buf

    def forward(self, frame, action, first_timestep=False):
        if first_timestep:
            self.init_hidden(frame.size(0))
        below = self._bottom_input(frame, action)
        for j, cell in enumerate(self.cell_list):
            h, c = (None, None) if self._is_untouched_zero(j) else (self.H[j], self.C[j])
            _, self.H[j], self.C[j] = cell._run(below.unsqueeze(1), h, c, 1)
            below = self.H[j]
        self._pristine = []
        return (self.H, self.C), self.H

    def init_hidden(self, batch_size):
        hh, ww = self.input_size
        self._pristine = [(torch.zeros(batch_size, ch, hh, ww, device=self.device),
                           torch.zeros(batch_size, ch, hh, ww, device=self.device)) for ch in self.hidden_dims[:self.n_layers]]
        self.H, self.C = [p[0] for p in self._pristine], [p[1] for p in self._pristine]

    def set_hidden(self, hidden):
        self.H, self.C = hidden
        self._pristine = []


def find_divisor_for_group_norm(x: int):
    """The reference's group count for GroupNorm(?, x): the largest divisor of x not above sqrt(x), as x // that divisor
    (phydnet.py find_divisor_for_group_norm)."""
    sq = math.floor(math.sqrt(x))
    while True:
        if x // sq == x / sq:
            return x // sq
        sq -= 1


def _with_action_tail(t, action, action_size):
    """[B,C,H,W] -> channels-last [B,C+a,H,W] with the action broadcast into the channel tail."""
    b, c, hh, ww = t.shape
    buf = ops.new_channels_last((b, c + action_size, hh, ww), t.device)
    buf[:, :c].copy_(t)
    buf[:, c:].copy_(action[:, :, None, None].expand(b, action_size, hh, ww))
    return buf


def _cat_channels(a, b):
    n, ca, hh, ww = a.shape
    buf = ops.new_channels_last((n, ca + b.shape[1], hh, ww), a.device)
    buf[:, :ca].copy_(a)
    buf[:, ca:].copy_(b)
    return buf


class PhyCell_Cell(VPModelBlock):
    """One PhyCell (phydnet.py PhyCell_Cell): prediction h + F(h), F = conv kxk (input_dim -> hidden) + GroupNorm + conv 1x1 back,
    corrected towards the encoded frame with the gate sigmoid(convgate([frame, h])). Five library calls per step (seven with
    actions): the three convolutions, the GroupNorm and the correction."""
    NAME = "PhyCell - Cell"
    PAPER_REFERENCE = "https://arxiv.org/abs/2003.01460"
    CODE_REFERENCE = "https://github.com/vincent-leguen/PhyDNet"
    MATCHES_REFERENCE = "Not Yet"
    precision = "f32"

    def __init__(self, input_dim, action_conditional, action_size, hidden_dim, kernel_size, bias=True):
        super().__init__()
        self.input_dim = input_dim
        self.action_size = action_size
        self.action_conditional = action_conditional
        self.F_hidden_dim = hidden_dim
        self.kernel_size = kernel_size
        self.padding = kernel_size[0] // 2, kernel_size[1] // 2
        self.bias = bias
        if kernel_size[0] != kernel_size[1] or kernel_size[0] % 2 == 0:
            raise ValueError(f"PhyCell_Cell: kernel {tuple(kernel_size)} must be square and odd")
        self.F = nn.Sequential()
        self.F.add_module('conv1', nn.Conv2d(in_channels=input_dim, out_channels=hidden_dim, kernel_size=self.kernel_size, stride=(1, 1),
                                             padding=self.padding))
        self.F.add_module('bn1', nn.GroupNorm(find_divisor_for_group_norm(hidden_dim), hidden_dim))
        self.F.add_module('conv2', nn.Conv2d(in_channels=hidden_dim, out_channels=input_dim, kernel_size=(1, 1), stride=(1, 1),
                                             padding=(0, 0)))
        self.convgate = nn.Conv2d(in_channels=2 * self.input_dim, out_channels=self.input_dim, kernel_size=(3, 3), padding=(1, 1),
                                  bias=self.bias)
        if self.action_conditional:
            self.frame_action_conv = nn.Conv2d(in_channels=self.input_dim + self.action_size, out_channels=self.input_dim,
                                               kernel_size=(1, 1))
            self.hidden_action_conv = nn.Conv2d(in_channels=self.input_dim + self.action_size, out_channels=self.input_dim,
                                                kernel_size=(1, 1))

    def _conv(self, x, conv, padding):
        return ops.conv2d_ex(x, conv.weight, conv.bias, 1, padding, precision=self.precision)

    def forward(self, frame, action, hidden):
        if self.action_conditional:
            frame = self._conv(_with_action_tail(frame, action, self.action_size), self.frame_action_conv, 0)
            hidden = self._conv(_with_action_tail(hidden, action, self.action_size), self.hidden_action_conv, 0)
        gate = self._conv(_cat_channels(frame, hidden), self.convgate, 1)
        bn = self.F.bn1
        f = self._conv(hidden, self.F.conv1, self.padding[0])
        f = phy_ops.group_norm(f, bn.num_groups, bn.weight, bn.bias)
        f = self._conv(f, self.F.conv2, 0)
        return phy_ops.phycell_correct(gate, f, hidden, frame)


class PhyCell(VPModelBlock):
    """The stack of PhyCells (phydnet.py PhyCell); keeps its state list `H` between calls like the reference."""
    NAME = "PhyCell"
    PAPER_REFERENCE = "https://arxiv.org/abs/2003.01460"
    CODE_REFERENCE = "https://github.com/vincent-leguen/PhyDNet"
    MATCHES_REFERENCE = "Not Yet"

    def __init__(self, input_size, input_dim, hidden_dims, n_layers, kernel_size, action_conditional, action_size, device):
        super().__init__()
        self.input_size = input_size
        self.input_dim = input_dim
        self.hidden_dims = hidden_dims
        self.n_layers = n_layers
        self.kernel_size = kernel_size
        self.H = []
        self.device = device
        self.cell_list = nn.ModuleList(PhyCell_Cell(input_dim=self.input_dim, action_conditional=action_conditional,
                                                    action_size=action_size, hidden_dim=self.hidden_dims[i], kernel_size=self.kernel_size)
                                       for i in range(self.n_layers))

    def forward(self, frame, action, first_timestep=False):
        if first_timestep:
            self.init_hidden(frame.size(0))
        for j, cell in enumerate(self.cell_list):
            self.H[j] = cell(frame if j == 0 else self.H[j - 1], action, self.H[j])
        return self.H, self.H

    def init_hidden(self, batch_size):
        # a real zero state: F(0) = conv2(GN(bias of conv1)) is not zero, so there is no shortcut for the first step
        self.H = [ops.new_channels_last((batch_size, self.input_dim, *self.input_size), self.cell_list[0].convgate.weight.device).zero_()
                  for _ in range(self.n_layers)]

    def _set_hidden(self, H):
        self.H = H


class EncoderSplit(nn.Module):
    """phydnet.py EncoderSplit: two stride-1 DCGAN conv layers (64 -> 64 at the latent resolution)."""

    def __init__(self, in_channels=64, enc_channels=64):
        super().__init__()
        self.c1 = DCGANConv(in_channels, enc_channels, stride=1)
        self.c2 = DCGANConv(enc_channels, enc_channels, stride=1)

    def forward(self, x):
        return self.c2(self.c1(x))


class DecoderSplit(nn.Module):
    """phydnet.py DecoderSplit: two stride-1 DCGAN transposed-conv layers. `residual` is added after the last layer's activation
    inside its GroupNorm kernel (PhyDNet's `decoded_phys + decoded_conv`)."""

    def __init__(self, out_channels=64, enc_channels=64):
        super().__init__()
        self.upc1 = DCGANConvTranspose(enc_channels, enc_channels, stride=1)
        self.upc2 = DCGANConvTranspose(enc_channels, out_channels, stride=1)

    def forward(self, x, residual=None):
        return self.upc2(self.upc1(x), residual=residual)
