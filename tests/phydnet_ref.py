"""PhyDNet's own pieces restated in plain torch ops (any device, any float dtype): the PhyCell block over a state_dict, stated from
`PhyCell_Cell.forward` / `PhyCell.forward` (vp_suite/model_blocks/phydnet.py), and the moment regularisation loss in fp64. A second
witness beside the recorded fixtures: tests/test_phydnet_host.py runs the block on the CPU in fp64 against phydnet_cell_plain.npz and
phydnet_cell_ac.npz, and tests/test_gpu_phydnet_kernels.py holds the library to it at shapes no fixture has.

Nothing of the library's schedule is in here: no channels-last buffers, no fused correction, one torch op per line of the model."""
import math

import torch
import torch.nn.functional as F


def groups(c):
    """find_divisor_for_group_norm: c // (the largest divisor of c not above sqrt(c))."""
    sq = math.floor(math.sqrt(c))
    while c % sq:
        sq -= 1
    return c // sq


def phycell_cell(sd, prefix, frame, action, hidden):
    """One PhyCell_Cell step. The cell is action-conditional when `sd` holds its two action convolutions."""
    p = prefix
    if p + "frame_action_conv.weight" in sd:
        inflated = action[:, :, None, None].expand(-1, -1, *frame.shape[-2:])
        frame = F.conv2d(torch.cat([frame, inflated], dim=1), sd[p + "frame_action_conv.weight"], sd[p + "frame_action_conv.bias"])
        hidden = F.conv2d(torch.cat([hidden, inflated], dim=1), sd[p + "hidden_action_conv.weight"], sd[p + "hidden_action_conv.bias"])
    gate = torch.sigmoid(F.conv2d(torch.cat([frame, hidden], dim=1), sd[p + "convgate.weight"], sd.get(p + "convgate.bias"), padding=1))
    w1 = sd[p + "F.conv1.weight"]
    f = F.conv2d(hidden, w1, sd[p + "F.conv1.bias"], padding=(w1.shape[-2] // 2, w1.shape[-1] // 2))
    f = F.group_norm(f, groups(f.shape[1]), sd[p + "F.bn1.weight"], sd[p + "F.bn1.bias"], eps=1e-5)
    f = F.conv2d(f, sd[p + "F.conv2.weight"], sd[p + "F.conv2.bias"])
    pred = hidden + f
    return pred + gate * (frame - pred)


def phycell_stack(sd, n_layers, frames, actions):
    """PhyCell from a zero state (`first_timestep=True` at step 0). frames: [B, T, C, H, W]; actions: [B, T, a] (read only by
    action-conditional cells). Returns (the top layer's state after every step, the final state list)."""
    b, steps = frames.shape[:2]
    H = [frames.new_zeros(b, *frames.shape[2:]) for _ in range(n_layers)]
    outs = []
    for t in range(steps):
        act = None if actions is None else actions[:, t]
        for j in range(n_layers):
            H[j] = phycell_cell(sd, f"cell_list.{j}.", frames[:, t] if j == 0 else H[j - 1], act, H[j])
        outs.append(H[-1])
    return outs, H


def moment_matrix(k):
    """K2M's M[i][u] = (u - (k-1)//2)^i / i! in fp64."""
    return torch.tensor([[((u - (k - 1) // 2) ** i) / math.factorial(i) for u in range(k)] for i in range(k)], dtype=torch.float64)


def moment_target(hid, kh, kw):
    C = torch.zeros(hid, kh, kw, dtype=torch.float64)
    for o in range(min(hid, kh * kw)):
        C[o, o // kw, o % kw] = 1.0
    return C


def _moment_loss_fp64(W, scale):
    hid, cin, kh, kw = W.shape
    M0, M1 = moment_matrix(kh), moment_matrix(kw)
    C = moment_target(hid, kh, kw)
    moment = torch.einsum("iu,obuv,jv->obij", M0, W, M1)
    return scale * ((moment - C[:, None]) ** 2).mean(dim=(0, 2, 3)).sum()


def moment_loss_fp64_two_products(W, scale):
    """The same loss in the kernel's evaluation order: tmp = w M1^T first, then M0 tmp, the squares summed per (o, b) pair."""
    hid, cin, kh, kw = W.shape
    M0, M1 = moment_matrix(kh), moment_matrix(kw)
    D = torch.matmul(M0, torch.matmul(W, M1.t())) - moment_target(hid, kh, kw)[:, None]
    return (D * D).sum(dim=(2, 3)).sum() * (scale / (hid * kh * kw))


def moment_optimum(hid, cin, kh, kw):
    """The filter bank at which the loss vanishes, w[o, b] = M0^-1 C_o M1^-T, solved in fp64."""
    M0, M1 = moment_matrix(kh), moment_matrix(kw)
    C = moment_target(hid, kh, kw)
    left = torch.linalg.solve(M0, C)                                   # M0^-1 C_o
    w = torch.linalg.solve(M1, left.transpose(1, 2)).transpose(1, 2)   # (M1^-1 (M0^-1 C_o)^T)^T = M0^-1 C_o M1^-T
    return w[:, None].expand(hid, cin, kh, kw).contiguous()
