"""UNet-3D restated in plain torch ops over a state_dict (any device, any float dtype): what tools/bench_unet3d.py times beside the
library path, and a second witness for the fixtures (tests/test_unet3d_host.py runs it on the CPU against unet3d_tiny.npz).

`training=True` uses batch statistics and updates the BatchNorm buffers of `sd` IN PLACE (running mean / unbiased variance with momentum
0.1, num_batches_tracked + 1), once per pred_1, as the modules of the original do."""
import torch
import torch.nn.functional as F


def replicate_conv(x, w):
    nd = w.dim() - 2
    x = F.pad(x, (1, 1) * nd, mode="replicate")
    return F.conv3d(x, w) if nd == 3 else F.conv2d(x, w)


def batch_norm_relu(sd, p, x, training):
    y = F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], training, 0.1, 1e-5)
    if training:
        sd[p + "num_batches_tracked"] += 1
    return F.relu(y)


def double_conv(sd, p, x, training):
    x = batch_norm_relu(sd, p + "conv.1.", replicate_conv(x, sd[p + "conv.0.weight"]), training)
    return batch_norm_relu(sd, p + "conv.4.", replicate_conv(x, sd[p + "conv.3.weight"]), training)


def pred_1(sd, x, training=False):
    n = sum(1 for k in sd if k.startswith("downs.") and k.endswith(".conv.0.weight"))
    td = sd["time3ds.0.weight"].shape[2]
    x = x[:, -td:].permute(0, 2, 1, 3, 4)   # [b, c, temporal_dim, h, w]
    skips = []
    for i in range(n):
        x = double_conv(sd, f"downs.{i}.", x, training)
        skips.append(F.conv3d(x, sd[f"time3ds.{i}.weight"], sd[f"time3ds.{i}.bias"]).squeeze(2))
        x = F.max_pool3d(x, (1, 2, 2), (1, 2, 2))
    x = F.conv3d(x, sd[f"time3ds.{n}.weight"], sd[f"time3ds.{n}.bias"]).squeeze(2)
    x = double_conv(sd, "bottleneck.", x, training)
    for i in range(n):
        x = F.conv_transpose2d(x, sd[f"ups.{2 * i}.weight"], sd[f"ups.{2 * i}.bias"], stride=2)
        x = double_conv(sd, f"ups.{2 * i + 1}.", torch.cat((skips[n - 1 - i], x), dim=1), training)
    return F.conv2d(x, sd["final_conv.weight"], sd["final_conv.bias"])


def forward(sd, x, pred_frames, training=False):
    preds = []
    for _ in range(pred_frames):
        pred = pred_1(sd, x, training).unsqueeze(1)
        preds.append(pred)
        x = torch.cat([x[:, 1:], pred], dim=1)
    return torch.cat(preds, dim=1), None
