"""Oracle of the NonConvLSTM model ("nc-lstm") for what the reference cannot supply, in plain torch on any device and dtype (the tests use
float64 on the CPU; tools/bench_lstm.py uses it as the fp32 twin on the GPU):

  * the dense layer and the LSTM cell as explicit formulas (tests/test_lstm_host.py pins the cell to torch.nn.LSTMCell in double);
  * the replicate padding and the bilinear resize as index arithmetic: the resize takes its source coordinates in float32 exactly as
    csrc/frames_coord.h forms them and does the tap arithmetic in the tensor's dtype, so in float64 it is the restatement the kernel is
    held to; gradients of everything come from autograd over these formulas;
  * `RefLSTM`: the model built from the same layers, with the carried state (`carry_state=True`) or the reference's literal
    decode(zeros) (`carry_state=False`, pinned to the reference's own output in tests/golden/lstm_tiny*.npz).

Also the case table of the fixtures, shared by tests/test_lstm_host.py, tests/test_gpu_lstm.py and tools/gen_golden_lstm.py."""
import numpy as np
import torch
import torch.nn.functional as F

# ---- fixture cases (tools/gen_golden_lstm.py) -----------------------------------------------------------------------------------------
LSTM_TINY_KW = dict(img_shape=(1, 16, 24), action_size=0, tensor_value_range=[0.0, 1.0], bottleneck_dim=24, lstm_hidden_dim=24, lstm_num_layers=2)
LSTM_TINY3_KW = dict(img_shape=(3, 20, 12), action_size=3, action_conditional=True, tensor_value_range=[0.0, 1.0], bottleneck_dim=24,
                     lstm_hidden_dim=24, lstm_num_layers=2)
LSTM_DEFAULT_KW = dict(img_shape=(1, 64, 64), action_size=0, tensor_value_range=[0.0, 1.0])
LSTM_TINY_B, LSTM_TINY_CTX, LSTM_TINY_PRED = 2, 5, 3        # 5 -> 3
LSTM_TINY3_CTX, LSTM_TINY3_PRED = 4, 2                       # action-conditional: 4 -> 2
LSTM_DEFAULT_B = 1
GRAD_SLICE, GRAD_FULL_MAX = 97, 64                          # gradient summaries keep every 97th element (at most 64) of larger tensors


def grad_kept(a):
    return a if a.size <= GRAD_FULL_MAX else a[::GRAD_SLICE][:64]


def grad_summary(named_grads):
    """{name: (sum, sum of squares, max |g|, the elements kept)} of fp64 numpy copies."""
    out = {}
    for k, g in named_grads.items():
        a = g.detach().cpu().double().numpy().reshape(-1)
        out[k] = (a.sum(), (a * a).sum(), np.abs(a).max(), grad_kept(a))
    return out


# ---- formulas -------------------------------------------------------------------------------------------------------------------------
def dense_ref(x, w, bias=None, relu=False):
    y = x @ w.t()
    if bias is not None:
        y = y + bias
    return torch.clamp_min(y, 0) if relu else y


def cell_ref(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """(h', c') of an LSTM cell in torch's gate order i, f, g, o; h or c None: zeros."""
    H = w_hh.shape[1]
    gates = x @ w_ih.t()
    if h is not None:
        gates = gates + h @ w_hh.t()
    for b in (b_ih, b_hh):
        if b is not None:
            gates = gates + b
    i, f, g, o = (gates[:, k * H:(k + 1) * H] for k in range(4))
    i, f, g, o = 1 / (1 + torch.exp(-i)), 1 / (1 + torch.exp(-f)), torch.tanh(g), 1 / (1 + torch.exp(-o))
    c_new = i * g if c is None else f * c + i * g
    return o * torch.tanh(c_new), c_new


def replicate_pad_ref(x, pad):
    """x [N,C,H,W] -> [N,C,H+2p,W+2p] by clamped indices."""
    H, W = x.shape[-2:]
    iy = torch.arange(-pad, H + pad, device=x.device).clamp(0, H - 1)
    ix = torch.arange(-pad, W + pad, device=x.device).clamp(0, W - 1)
    return x[:, :, iy][:, :, :, ix]


def _coords(n_in, n_out, device):
    """(i0, i1, l) per output index, formed in float32 as csrc/frames_coord.h does."""
    s = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    src = np.maximum(s * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0).to(device), torch.from_numpy(i1).to(device), torch.from_numpy(lam.astype(np.float64)).to(device)


def resize_ref(x, out_hw):
    """Bilinear, align_corners=False, no antialiasing: horizontally first, r = v0 * (1 - l) + v1 * l, then vertically."""
    H, W = x.shape[-2:]
    oh, ow = out_hw
    y0, y1, ly = _coords(H, oh, x.device)
    x0, x1, lx = _coords(W, ow, x.device)
    ly, lx = ly.to(x.dtype).view(-1, 1), lx.to(x.dtype)
    rows = x[..., x0] * (1 - lx) + x[..., x1] * lx
    return rows[..., y0, :] * (1 - ly) + rows[..., y1, :] * ly


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class RefLSTM:
    """The NonConvLSTM model on plain torch from a state dict with the model's keys (`enc1.weight`, ..., `rnn_layers.0.weight_ih`, ...)."""

    def __init__(self, state_dict, img_shape, action_conditional=False, carry_state=True, dtype=torch.float64, device="cpu", requires_grad=False):
        self.p = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(requires_grad) for k, v in state_dict.items()
                  if not k.startswith(("encoder.", "decoder."))}
        self.img_shape, self.ac, self.carry = tuple(img_shape), action_conditional, carry_state
        self.n_layers = len({k.split(".")[1] for k in self.p if k.startswith("rnn_layers.")})
        self.hidden = self.p["from_linear.weight"].shape[1]
        self.dtype, self.device = dtype, device

    def conv_encoder(self, x):
        p = self.p
        x = F.relu(F.conv2d(x, p["enc1.weight"], p["enc1.bias"], stride=2, padding=3))
        x = F.relu(F.conv2d(replicate_pad_ref(x, 1), p["enc2.weight"], p["enc2.bias"], stride=2))
        return F.relu(F.conv2d(replicate_pad_ref(x, 1), p["enc3.weight"], p["enc3.bias"], stride=2))

    def encode(self, x):
        m = self.conv_encoder(x)
        self.encoded_shape = m.shape[1:]
        return m.flatten(1) @ self.p["to_linear.weight"].t() + self.p["to_linear.bias"]

    def encoded_map_shape(self):
        c, h, w = self.img_shape
        d = lambda n, k, pad: (n + 2 * pad - k) // 2 + 1  # noqa: E731
        return (256, d(d(d(h, 7, 3), 3, 1), 3, 1), d(d(d(w, 7, 3), 3, 1), 3, 1))

    def decode(self, z):
        p = self.p
        x = (z @ p["from_linear.weight"].t() + p["from_linear.bias"]).reshape(z.shape[0], *self.encoded_map_shape())
        x = F.relu(F.conv_transpose2d(x, p["dec1.weight"], p["dec1.bias"], stride=2, padding=1))
        x = F.relu(F.conv_transpose2d(x, p["dec2.weight"], p["dec2.bias"], stride=2, padding=1))
        x = F.conv_transpose2d(x, p["dec3.weight"], p["dec3.bias"], stride=2, padding=3)
        return resize_ref(x, self.img_shape[1:])

    def action_inflate(self, a):
        return a.flatten(1) @ self.p["action_inflate.weight"].t() + self.p["action_inflate.bias"]

    def forward(self, x, pred_frames=1, actions=None):
        x = x.transpose(0, 1)
        T_in, b = x.shape[:2]
        if not self.carry:
            frame = self.decode(torch.zeros(b, self.hidden, dtype=self.dtype, device=self.device))
            return torch.stack([frame] * pred_frames, dim=1)
        if actions is not None:
            actions = actions.transpose(0, 1)
        hiddens = [(None, None)] * self.n_layers

        def step(inp):
            for i in range(self.n_layers):
                q = f"rnn_layers.{i}."
                hiddens[i] = cell_ref(inp, *hiddens[i], self.p[q + "weight_ih"], self.p[q + "weight_hh"], self.p[q + "bias_ih"], self.p[q + "bias_hh"])
                inp = hiddens[i][0]
            return inp

        def cell_input(frame, action):
            e = self.encode(frame)
            return torch.cat([e, self.action_inflate(action)], dim=-1) if self.ac else e

        for t in range(T_in):
            out = step(cell_input(x[t], actions[t] if self.ac else None))
        preds = [self.decode(out)]
        for t in range(pred_frames - 1):
            out = step(cell_input(preds[-1], actions[t - T_in] if self.ac else None))
            preds.append(self.decode(out))
        return torch.stack(preds, dim=1)
