"""NonConvLSTM ("nc-lstm") — the model the docstring of vp_suite/models/lstm.py describes: a strided-convolution encoder, a Linear to
a `bottleneck_dim`-wide latent, a stack of LSTM layers whose state is carried from step to step, a Linear back and a
transposed-convolution decoder that ends in a bilinear Resize. The reference's class constants, hyper-parameters, errors, `pred_1` and
`(preds [b, p, c, h, w], None)` return, on the library's kernels: the convolutions with ReLU in their epilogue (stphy_ops / ops), and
the dense layer, the LSTM cell, the replicate padding and the differentiable resize of lstm_ops. No ATen convolution, padding, linear,
LSTM, activation, cat or interpolation runs over activations. fp32 only: any other `cell_precision` raises ValueError.

Divergences, stated loudly:
  * THE REFERENCE'S RECURRENCE IS DEAD. In lstm.py:94-95 and 107-108 `hidden = lstm_cell(encoded, hidden)` only rebinds a loop variable:
    `hiddens` stays all zeros, so the reference's forward returns decode(zeros) for every predicted frame, whatever the input. Its
    `rnn_layers` is a plain Python list, so the cells are absent from `state_dict()` and `parameters()` and are never trained. Every
    cell is built with `input_size=bottleneck_dim`, so feeding layer l-1's state to layer l would only work because both sizes default
    to 1024. The class says MATCHES_REFERENCE = "Not Yet".
  * `carry_state=True` (the default) is OUR model: per step, layer 0 reads the encoded frame (with the inflated action appended when
    action-conditional), layer l > 0 reads layer l-1's new h, every layer's (h, c) persists over all context and prediction steps, and
    the prediction is decode(h of the last layer). `rnn_layers` is an nn.ModuleList of holders with nn.LSTMCell's parameter names,
    shapes and default initialisation; layer 0 has input size `bottleneck_dim` (+ `bottleneck_dim // 10` when action-conditional), the
    layers above it `lstm_hidden_dim`. These parameters are in `state_dict()` and are trained.
  * `carry_state=False` is the reference's literal result: every predicted frame is decode(zeros). Work nothing can observe is skipped
    (the encoder, the cells, re-encoding the predictions); the skipped parameters get no gradient (`.grad` stays None), as in the
    reference, where the encoder's and to_linear's gradients are None too.
  * The registry key is "nc-lstm"; the reference's key "lstm" stays invalid (it would promise the reference's output).

Kept as the reference has them: every key and shape of its `state_dict`, including the duplicates it produces by registering
`enc1 ... dec3` both directly and inside `encoder` / `decoder` (a reference checkpoint loads with strict=False: only `rnn_layers.*` is
missing); prediction step t takes `actions[:, t - T_in]` exactly as lstm.py:105 indexes it (a negative index from the end for
t < T_in); `self.bottleneck_dim` grows by the inflated action size when action-conditional.

The step schedule differs from the reference's only in work nothing can observe: all context frames are encoded as one batch of T * B
rows, and the encoded frame and the inflated action are written side by side into one buffer by the dense layer (no cat).
The flatten between the channels-last maps and the Linear layers' [C, H, W] feature order is a layout copy."""
import math

import torch
from torch import nn

from .. import lstm_ops, ops, stphy_ops
from ..base import VPModel


class _LSTMCellParams(nn.Module):
    """The parameters of one torch.nn.LSTMCell: names, shapes and default initialisation (uniform in +-1 / sqrt(hidden_size))."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.weight_ih = nn.Parameter(torch.empty(4 * hidden_size, input_size))
        self.weight_hh = nn.Parameter(torch.empty(4 * hidden_size, hidden_size))
        self.bias_ih = nn.Parameter(torch.empty(4 * hidden_size))
        self.bias_hh = nn.Parameter(torch.empty(4 * hidden_size))
        bound = 1.0 / math.sqrt(hidden_size) if hidden_size > 0 else 0.0
        for p in self.parameters():
            nn.init.uniform_(p, -bound, bound)

    def forward(self, x, hc):
        return lstm_ops.lstm_cell(x, hc, self.weight_ih, self.weight_hh, self.bias_ih, self.bias_hh)


class _Resize(nn.Module):
    """Stands where the reference has TF.Resize((img_h, img_w)): the bilinear resize of a float tensor that is enlarged."""

    def __init__(self, size):
        super().__init__()
        self.size = tuple(int(s) for s in size)

    def forward(self, x):
        return lstm_ops.resize_bilinear(x, self.size)


def _down(n, k, pad):
    return (n + 2 * pad - k) // 2 + 1


class LSTM(VPModel):
    NAME = "NonConvLSTM"
    PAPER_REFERENCE = None
    CODE_REFERENCE = None
    MATCHES_REFERENCE: str = "Not Yet"
    CAN_HANDLE_ACTIONS = True

    bottleneck_dim = 1024  #: The dimensionality of the linearized latent space.
    lstm_hidden_dim = 1024  #: The hidden dimensionality of the LSTM cells.
    lstm_num_layers = 3  #: The number of LSTM cell layers.
    carry_state = True  #: True: the LSTM layers run and carry their state; False: the reference's literal output, decode(zeros)
    cell_precision = "f32"  #: arithmetic of every layer; only "f32" exists for this model

    def __init__(self, device, **model_kwargs):
        super().__init__(device, **model_kwargs)
        if self.cell_precision != "f32":
            raise ValueError(f"LSTM: cell_precision must be 'f32' (the dense layer and the LSTM cell are fp32 only), got {self.cell_precision!r}")
        if min(int(self.bottleneck_dim), int(self.lstm_hidden_dim), int(self.lstm_num_layers)) < 1:
            raise ValueError(f"LSTM: bottleneck_dim, lstm_hidden_dim and lstm_num_layers must be at least 1, got {self.bottleneck_dim}, "
                             f"{self.lstm_hidden_dim}, {self.lstm_num_layers}")
        self.act_fn = nn.ReLU(inplace=True)
        self.pool = nn.MaxPool2d(2, 2)
        self.enc1 = nn.Conv2d(self.img_c, 64, kernel_size=7, stride=2, padding=3)
        self.enc2 = nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1, padding_mode="replicate")
        self.enc3 = nn.Conv2d(128, 256, kernel_size=3, stride=2, padding=1, padding_mode="replicate")
        self.encoder = nn.Sequential(self.enc1, self.act_fn, self.enc2, self.act_fn, self.enc3, self.act_fn)
        eh, ew = (_down(_down(_down(n, 7, 3), 3, 1), 3, 1) for n in (self.img_h, self.img_w))   # (the reference runs its encoder on zeros)
        if eh < 1 or ew < 1:
            raise ValueError(f"LSTM: frames of {self.img_h}x{self.img_w} leave no encoded map")
        self.encoded_shape = torch.Size((256, eh, ew))
        self.encoded_numel = 256 * eh * ew
        self.to_linear = nn.Linear(self.encoded_numel, self.bottleneck_dim)
        self._encoded_dim = self.bottleneck_dim
        if self.action_conditional:
            inflated_action_size = self.bottleneck_dim // 10
            if self.action_size < 1 or inflated_action_size < 1:
                raise ValueError(f"LSTM: action-conditional needs action_size >= 1 and bottleneck_dim >= 10, got {self.action_size} and {self.bottleneck_dim}")
            self.bottleneck_dim += inflated_action_size
            self.action_inflate = nn.Linear(self.action_size, inflated_action_size)
        self.rnn_layers = nn.ModuleList([_LSTMCellParams(self.bottleneck_dim if i == 0 else self.lstm_hidden_dim, self.lstm_hidden_dim)
                                         for i in range(self.lstm_num_layers)])
        self.from_linear = nn.Linear(self.lstm_hidden_dim, self.encoded_numel)
        self.dec1 = nn.ConvTranspose2d(256, 128, kernel_size=3, stride=2, padding=1)
        self.dec2 = nn.ConvTranspose2d(128, 64, kernel_size=3, stride=2, padding=1)
        self.dec3 = nn.ConvTranspose2d(64, self.img_c, kernel_size=7, stride=2, padding=3)
        self.decoder = nn.Sequential(self.dec1, self.act_fn, self.dec2, self.act_fn, self.dec3, _Resize((self.img_h, self.img_w)))
        self.to(self.device)

    # ---- the layers on the library ----------------------------------------------------------------------------------------------------
    def _conv_encoder(self, x):
        x = stphy_ops.conv2d_act(x, self.enc1.weight, self.enc1.bias, 2, 3, act="relu")
        x = lstm_ops.conv2d_replicate(x, self.enc2.weight, self.enc2.bias, stride=2, relu=True)
        return lstm_ops.conv2d_replicate(x, self.enc3.weight, self.enc3.bias, stride=2, relu=True)

    def encode(self, x, out=None):
        """to_linear(encoder(x).flatten(1, -1)) for x [n, c, h, w]; `out`: a [n, bottleneck] column slice to write into."""
        maps = self._conv_encoder(x)
        return lstm_ops.dense(maps.reshape(maps.shape[0], -1), self.to_linear.weight, self.to_linear.bias, out=out)

    def decode(self, z):
        """decoder(from_linear(z).reshape(n, 256, eh, ew)) for z [n, lstm_hidden_dim]: [n, c, img_h, img_w]."""
        x = lstm_ops.dense(z, self.from_linear.weight, self.from_linear.bias).reshape(z.shape[0], *self.encoded_shape)
        x = stphy_ops.conv2d_act(x, self.dec1.weight, self.dec1.bias, 2, 1, transposed=True, act="relu")
        x = stphy_ops.conv2d_act(x, self.dec2.weight, self.dec2.bias, 2, 1, transposed=True, act="relu")
        x = ops.conv2d_ex(x, self.dec3.weight, self.dec3.bias, 2, 3, transposed=True)
        return lstm_ops.resize_bilinear(x, (self.img_h, self.img_w))

    def pred_1(self, x, **kwargs):
        return self(x, pred_frames=1, **kwargs)[0].squeeze(dim=1)

    def _cell_input(self, encode_into, action, b, dev):
        """[encoded | inflated action] of one step, both halves written in place by their dense layers. encode_into(out) fills the
        encoded half (out None: returns a fresh tensor)."""
        if not self.action_conditional:
            return encode_into(None)
        buf = torch.empty(b, self.bottleneck_dim, device=dev)
        encode_into(buf[:, :self._encoded_dim])
        lstm_ops.dense(action.flatten(1, -1), self.action_inflate.weight, self.action_inflate.bias, out=buf[:, self._encoded_dim:])
        return buf

    def forward(self, x, pred_frames=1, **kwargs):
        x = x.transpose(0, 1)  # imgs: [t, b, c, h, w]
        T_in, b, c, h, w = x.shape
        if tuple(self.img_shape) != (c, h, w):
            raise ValueError(f"input image does not match specified size "
                             f"(input image shape: {x.shape[2:]}, required: {self.img_shape})")
        actions = kwargs.get("actions", None)
        if self.action_conditional:
            if actions is None or actions.shape[-1] != self.action_size:
                raise ValueError("Given actions are None or of the wrong size!")
        if type(actions) == torch.Tensor:
            actions = actions.transpose(0, 1)  # [T_in+pred, b, ...]
        dev = x.device

        if not self.carry_state:
            # the reference's literal result: the state it decodes never leaves zero, so every frame is decode(zeros)
            frame = self.decode(torch.zeros(b, self.lstm_hidden_dim, device=dev))
            return torch.stack([frame] * pred_frames, dim=1), None

        # every context frame in one batch, frame-major rows; with actions, both halves of [encoded | inflated action] land in one buffer
        frames = x.reshape(T_in * b, c, h, w)
        if self.action_conditional:
            if actions.shape[0] < T_in:
                raise IndexError(f"index {actions.shape[0]} is out of bounds: {T_in} context frames need as many actions")
            ctx = torch.empty(T_in * b, self.bottleneck_dim, device=dev)
            self.encode(frames, out=ctx[:, :self._encoded_dim])
            lstm_ops.dense(actions[:T_in].reshape(T_in * b, -1), self.action_inflate.weight, self.action_inflate.bias, out=ctx[:, self._encoded_dim:])
        else:
            ctx = self.encode(frames)
        hiddens = [None] * len(self.rnn_layers)

        def step(inp):
            for i, cell in enumerate(self.rnn_layers):
                hiddens[i] = cell(inp, hiddens[i])
                inp = hiddens[i][0]
            return inp

        for t in range(T_in):
            output = step(ctx[t * b:(t + 1) * b])
        preds = [self.decode(output)]
        for t in range(pred_frames - 1):
            last = preds[-1]
            inp = self._cell_input(lambda out: self.encode(last, out=out), actions[t - T_in] if self.action_conditional else None, b, dev)
            output = step(inp)
            preds.append(self.decode(output))
        return torch.stack(preds, dim=1), None  # output is [b, t, c, h, w] again
