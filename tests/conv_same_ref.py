"""The stride-1 'same' convolution in plain float64 — vpx_conv2d_nhwc_fwd, vpx_conv2d_nhwc_fwd_ex and vpx_conv2d_nhwc_bwd (csrc/vpx_api.hip,
csrc/conv_same_api.hip; plain_conv / plain_wgrad / launch_colsum in csrc/vpx_host.h) — with the case tables of tests/test_gpu_conv_same.py (GPU parity)
and tests/test_conv_same_host.py (the conditions on the inputs, the dry run and the refusals, on the CPU). Nothing here touches the GPU or imports
the package.

The statement: y = leaky_relu(F.conv2d(x, w, b, padding=(kh // 2, kw // 2)) [+ acc0], slope), the activation on the SUM, and the autograd
gradients of (y * gy).sum() with respect to x, w and b. Inputs are seeded randn; weights are scaled 1 / sqrt(Ci kh kw) (outputs of unit
variance), the bias by 0.1. Nothing is symmetric: a missing tap flip or a kh / kw swap moves a result by its own size.

A case is (N, Ci, Co, kh, kw, H, W). Pixel tiles are 8 x 16 (TILE_H x TILE_W); an N tile holds ng = plain_groups(Co) groups of 32 output
channels; a contraction stage holds at most 64 channels (CS_MAX), in k-steps of 8 (f32) or 16 (the bf16 modes)."""
import functools

import torch
import torch.nn.functional as F

from golden_util import name_seed, seeded_randn

# max|got - ref| / max|ref| (tests/parity.py), forward and gradients, per operand mode
BARS = {"f32": (1e-5, 2e-5),       # RTOL / GRTOL of tests/test_gpu_convlstm.py
        "bf16x3": (5e-5, 1e-4),    # _conv2d_ex_cases (tests/test_gpu_more.py); train_tail_ref.GRAD_TOL
        "bf16": (2e-2, 2e-2)}      # test_plain_bf16_mode_has_its_own_tolerance
HOST_SHARE = 0.2                   # the fp32 CPU run of `reference` holds this share of the f32 bars against its fp64 run
SAME_PRODUCTS = 2e-5               # two launches with the same products in another fp32 summation order (tests/test_gpu_more.py)
KINK_SHARE = 1e-3                  # at most this share of the elements may lie within a forward bar of LeakyReLU's kink
SLOPE = 0.2

_MAP = (9, 17)                     # one past the 8 x 16 tile both ways: four pixel tiles, three of them ragged

# ng = 1, 2, 3, 4 at Co <= 32, <= 64, <= 96, <= 128; Co = 130: ng = 3 again, a 96-channel tile and a 34-channel tail tile
TILING = [(2, 12, Co, 3, 3) + _MAP for Co in (1, 5, 32, 33, 64, 70, 96, 97, 128, 130)] + [(2, 130, 33, 3, 3) + _MAP, (2, 130, 130, 3, 3) + _MAP]
# channel padding up to the k-step (8 / 16) and more than one 64-channel stage
CHANNELS = [(2, Ci, 24, 3, 3) + _MAP for Ci in (1, 3, 7, 8, 9, 16, 17, 40, 65, 130)]
# rectangular kernels: the tap flip of the data gradient, the tap groups of 9 of the weight gradient
KERNELS = [(2, 17, 40, kh, kw) + _MAP for kh, kw in ((1, 1), (3, 3), (5, 5), (7, 7), (3, 5), (5, 3), (1, 7), (7, 1))]
# one pixel, one row, one column, a map smaller than the kernel, exactly the tile, one past it, two tiles + one column
MAPS = [(N, 9, 33, k, k, H, W) for k in (3, 7) for (H, W) in ((1, 1), (1, 17), (9, 1), (2, 3), (8, 16), (9, 17), (16, 33)) for N in (1, 3)]
# more than 64 contraction channels on few tiles: pick_ksplit splits K over workgroups (below 256 workgroups, at least 2 stages, not in
# deterministic mode, no activation). The data gradient contracts over Co.
KSPLIT_FWD = [(1, 130, 33, 3, 3, 9, 17), (2, 65, 97, 7, 7, 2, 3)]
KSPLIT_BWD = [(1, 9, 130, 3, 3, 9, 17), (3, 17, 97, 5, 5, 8, 16)]
# wgrad_slices_for: up to 256 slices where all of dW is one output tile (Co, Ci <= 64, at most 9 taps), else 32; 40 work items tell them apart
SLICES = [(40, 64, 64, 3, 3, 8, 16),     # the 256-slice cap
          (40, 65, 64, 3, 3, 8, 16),     # the 32-slice cap: a second channel tile
          (40, 64, 64, 5, 5, 8, 16),     # the 32-slice cap: three tap groups
          (3, 130, 70, 3, 3, 16, 33)]    # ragged 64-row and 64-channel tiles
TABLES = {"TILING": TILING, "CHANNELS": CHANNELS, "KERNELS": KERNELS, "MAPS": MAPS, "KSPLIT_FWD": KSPLIT_FWD, "KSPLIT_BWD": KSPLIT_BWD,
          "SLICES": SLICES}
SAME_TABLES = ("TILING", "CHANNELS", "KERNELS", "MAPS")          # through ops.conv2d_same
# vpx_conv2d_nhwc_fwd_ex with its options: (table, index)
FWD_EX = [("KSPLIT_FWD", 0), ("KSPLIT_FWD", 1), ("MAPS", 6), ("MAPS", 26), ("TILING", 3), ("TILING", 9)]
# the plain-bf16 operand mode: one case of each table
PLAIN_BF16 = [("TILING", 11), ("CHANNELS", 6), ("KERNELS", 4), ("MAPS", 12)]
EXPANDED = ("CHANNELS", 5)         # its upstream gradient is the expanded zero-stride tensor of y.sum().backward()


def all_cases():
    return [(t, i) for t in TABLES for i in range(len(TABLES[t]))]


def case_id(table, i):
    N, Ci, Co, kh, kw, H, W = TABLES[table][i]
    return f"{table}-n{N}ci{Ci}co{Co}k{kh}x{kw}m{H}x{W}"


def variant(table, i):
    """How ops.conv2d_same is handed case i: with a bias or None, x channels-last or plain NCHW, the upstream gradient dense or expanded."""
    return {"bias": i % 3 != 1, "channels_last": i % 2 == 0, "expanded": (table, i) == EXPANDED}


def inputs(table, i):
    """x [N, Ci, H, W], w [Co, Ci, kh, kw], b [Co], gy and acc0 [N, Co, H, W] in float32."""
    N, Ci, Co, kh, kw, H, W = TABLES[table][i]
    tag = f"conv_same.{table}.{TABLES[table][i]}."
    return {"x": seeded_randn((N, Ci, H, W), name_seed(tag + "x")),
            "w": seeded_randn((Co, Ci, kh, kw), name_seed(tag + "w"), 1.0 / float(Ci * kh * kw) ** 0.5),
            "b": seeded_randn((Co,), name_seed(tag + "b"), 0.1),
            "gy": seeded_randn((N, Co, H, W), name_seed(tag + "gy")),
            "acc0": seeded_randn((N, Co, H, W), name_seed(tag + "acc0"))}


def reference(x, w, b, gy, acc0=None, slope=0.0, dtype=torch.float64):
    """On the CPU in `dtype`: y, the autograd gradients of (y * gy).sum() with respect to x, w and b (None without a bias), and the
    pre-activation sum."""
    lv = [None if t is None else t.detach().clone().to(dtype).requires_grad_(True) for t in (x, w, b)]
    kh, kw = w.shape[2:]
    pre = F.conv2d(lv[0], lv[1], lv[2], padding=(kh // 2, kw // 2))
    if acc0 is not None:
        pre = pre + acc0.to(dtype)
    y = F.leaky_relu(pre, slope) if slope != 0.0 else pre
    (y * gy.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": lv[0].grad, "dw": lv[1].grad, "db": None if b is None else lv[2].grad, "pre": pre.detach()}


@functools.lru_cache(maxsize=None)
def case(table, i, bias=True, ones=False, acc=False, slope=0.0):
    """(inputs, fp64 reference) of one case: computed once, shared among the tests, never written. `ones`: gy = 1 (y.sum())."""
    t = inputs(table, i)
    if ones:
        t["gy"] = torch.ones_like(t["gy"])
    return t, reference(t["x"], t["w"], t["b"] if bias else None, t["gy"], t["acc0"] if acc else None, slope)


def relmax(got, ref):
    """The suite's metric (tests/parity.py)."""
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def off_kink(ref, bar):
    """Elements whose fp64 pre-activation is farther than bar * max|ref| from LeakyReLU's kink."""
    return ref["pre"].abs() > bar * float(ref["y"].abs().max())
