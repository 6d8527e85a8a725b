"""ST-Phy restated in plain torch ops over a state_dict (any device, any float dtype): what tools/bench_stphy.py times beside the
library path, and a second witness for the fixtures (tests/test_stphy_host.py runs it on the CPU against stphy_tiny.npz).

It follows the model's step order literally, without the library's schedule: one frame encoded per step, every layer's PhyCell and
merge computed (the lower layers' results are overwritten, as in the original), every produced frame decoded on the spot, the
decoupling term per layer and step. The ST-LSTM cell and the decoupling term are the oracle's (oracle/torch_ref.py)."""
import math

import torch
import torch.nn.functional as F

from oracle import torch_ref


def encode(sd, x, p="autoencoder.encoder."):
    x = F.relu(F.conv2d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], stride=2))
    x = F.relu(F.conv2d(x, sd[p + "conv2.weight"], sd[p + "conv2.bias"], stride=2))
    x = F.relu(F.conv2d(x, sd[p + "mean_layer.weight"], sd[p + "mean_layer.bias"]))
    return F.normalize(x, p=2, dim=-1, eps=1e-8)


def decode(sd, x, p="autoencoder.decoder."):
    x = F.relu(F.conv2d(x, sd[p + "fc1.weight"], sd[p + "fc1.bias"]))
    x = F.relu(F.conv_transpose2d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], stride=2))
    x = F.relu(F.conv_transpose2d(x, sd[p + "conv2.weight"], sd[p + "conv2.bias"], stride=2))
    return F.conv_transpose2d(x, sd[p + "conv3.weight"], sd[p + "conv3.bias"])


def _groups(c):
    sq = math.floor(math.sqrt(c))
    while c % sq:
        sq -= 1
    return c // sq


def phycell(sd, p, frame, hidden):
    k = sd[p + "F.conv1.weight"].shape[-1]
    f = F.conv2d(hidden, sd[p + "F.conv1.weight"], sd[p + "F.conv1.bias"], padding=k // 2)
    f = F.group_norm(f, _groups(f.shape[1]), sd[p + "F.bn1.weight"], sd[p + "F.bn1.bias"])
    f = F.conv2d(f, sd[p + "F.conv2.weight"], sd[p + "F.conv2.bias"])
    gate = torch.sigmoid(F.conv2d(torch.cat([frame, hidden], dim=1), sd[p + "convgate.weight"], sd[p + "convgate.bias"], padding=1))
    pred = hidden + f
    return pred + gate * (frame - pred)


def moment_loss(w, scale):
    """scale^2 * sum_b mean((M0 w[:, b] M1^T - C)^2) in fp64 (the scale enters inside the mean and once more outside it)."""
    hidden, cin, kh, kw = w.shape

    def mat(k):
        u = torch.arange(k, dtype=torch.float64, device=w.device) - (k - 1) // 2
        return torch.stack([u ** i / math.factorial(i) for i in range(k)])
    m0, m1 = mat(kh), mat(kw)
    mom = torch.einsum("iu,obuv,jv->boij", m0, w.double(), m1)
    target = torch.zeros(hidden, kh, kw, dtype=torch.float64, device=w.device)
    for o in range(min(hidden, kh * kw)):
        target[o, o // kw, o % kw] = 1.0
    return (scale * scale * ((mom - target) ** 2).mean(dim=(1, 2, 3)).sum()).to(w.dtype)


def forward(sd, x, pred_frames, *, num_layers, train=False, teacher_forcing=False, moment_loss_scale=1.0, decoupling_loss_scale=100.0):
    b, ctx = x.shape[0], x.shape[1] - (pred_frames if train else 0)
    teacher_forcing = teacher_forcing and train
    c = sd["adapter.weight"].shape[0]
    eh, ew = sd["st_cell_list.0.conv_x.1.weight"].shape[1:]
    z = x.new_zeros(b, c, eh, ew)
    st_h, st_c, phy_h = [z] * num_layers, [z] * num_layers, [z] * num_layers
    memory, x_gen, frames, dec = z, None, [], []
    for t in range(ctx + pred_frames - 1):
        inp = encode(sd, x[:, t]) if (t < ctx or teacher_forcing) else x_gen
        for i in range(num_layers):
            phy_h[i] = phycell(sd, f"phycell_list.{i}.", inp, phy_h[i])
            st_h[i], st_c[i], memory, d_c, d_m = torch_ref.stlstm_cell(inp, st_h[i], st_c[i], memory, sd, prefix=f"st_cell_list.{i}.",
                                                                       layer_norm=True)
            if train:
                dec.append(torch_ref.decouple_term(d_c, d_m, sd["adapter.weight"]))
            x_gen = F.conv2d(torch.cat([st_h[i], phy_h[i]], dim=1), sd[f"hidden_conv_list.{i}.weight"], sd.get(f"hidden_conv_list.{i}.bias"))
        if train or t >= ctx - 1:
            frames.append(decode(sd, x_gen))
    out = torch.stack(frames, dim=1)
    if not train:
        return out, None
    return out, {"moment regularization loss": moment_loss(sd["phycell_list.0.F.conv1.weight"], moment_loss_scale),
                 "memory decoupling loss": decoupling_loss_scale * torch.stack(dec).mean()}
