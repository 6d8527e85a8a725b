"""The stage glue in plain float64 — vpx_conv2d_ex_fwd / _fwd_split / _fwd_from_split / _bwd / _bwd_ex and vpx_conv2d_act_fwd / _bwd
(csrc/glue_fwd_api.hip, csrc/glue_bwd_api.hip: stride-1/2 convolution and transposed convolution + bias + LeakyReLU / ReLU, forward and backward) — with the case
tables of tests/test_gpu_glue.py (GPU parity) and tests/test_glue_host.py (the conditions on the inputs, the routes each case takes, the
dry run and the refusals, on the CPU). Nothing here touches the GPU or imports the package.

The statement: y = act(F.conv2d | F.conv_transpose2d(x, w, b, stride, pad[, output_padding])) and the autograd gradients of
(y * gy).sum() with respect to x, w and b. Inputs are seeded as in conv_same_ref: randn, weights scaled 1 / sqrt(Ci kh kw), the bias by
0.1. Nothing is symmetric: a missing tap flip, a kh / kw swap or a dropped output-padding row moves a result by its own size.

The kink: gy is ZERO wherever the fp64 pre-activation lies within BARS["bf16x3"][0] * max|y| of 0 (in both operand modes). Neither side's
derivative there then matters, and the reference's LeakyReLU' / ReLU' comes from its OWN fp64 pre-activation, never from the library's
output. At most KINK_SHARE of a case's elements may be zeroed (tests/test_glue_host.py). The forward y is compared everywhere: it is
continuous at the kink.

A case is (tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W); weights have the reference's layouts, [Co, Ci, kh, kw] and, transposed,
[Ci, Co, kh, kw]."""
import functools

import torch
import torch.nn.functional as F

from conv_same_ref import BARS, HOST_SHARE, KINK_SHARE, SAME_PRODUCTS, SLOPE, relmax   # the project's figures: imported, not restated
from golden_util import name_seed, seeded_randn

__all__ = ["BARS", "HOST_SHARE", "KINK_SHARE", "SAME_PRODUCTS", "SLOPE", "relmax"]

KINK_BAR = BARS["bf16x3"][0]
_OPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def _c(tr, N, Ci, Co, k, s, p, H, W, op=(0, 0)):
    kh, kw = (k, k) if isinstance(k, int) else k
    return (int(tr), N, Ci, Co, kh, kw, s, p, op[0], op[1], H, W)


# ---- PHASES: transposed, stride 2 — four phase launches with a tap map; 1x1 ... 4x4 taps per phase; the output padding per axis ----------
_SQUARE = [(k, p) for k in range(2, 8) for p in sorted({0, 1, k // 2})]
PHASES = ([_c(1, 2, 5, 6, k, 2, p, 7, 9, _OPS[n % 4]) for n, (k, p) in enumerate(_SQUARE)] +
          [_c(1, 2, 5, 6, k, 2, 1, 7, 9, _OPS[(n + 1) % 4]) for n, k in enumerate(((3, 4), (4, 3), (2, 5), (7, 2)))] +
          # maps of one pixel, one row, one column: phases of unequal size, a phase that is empty along one axis (Ho or Wo == 1)
          [_c(1, 2, 5, 6, 3, 2, 1, 1, 1), _c(1, 2, 5, 6, 4, 2, 1, 1, 1, (1, 1)), _c(1, 2, 5, 6, 2, 2, 0, 1, 1, (1, 0)),
           _c(1, 2, 5, 6, 3, 2, 1, 1, 5, (0, 1)), _c(1, 2, 5, 6, 4, 2, 1, 1, 5), _c(1, 2, 5, 6, (3, 4), 2, 1, 5, 1, (1, 0)),
           _c(1, 2, 5, 6, 3, 2, 1, 5, 1)])


# ---- STRIDED: convolution, stride 2; its adjoint gets the output padding ((H + 2p - kh) % 2, (W + 2p - kw) % 2): all four per kernel -------
def _strided():
    out = []
    for ik, k in enumerate((2, 3, 4, 5, 7, (3, 5), (4, 2))):
        kh, kw = (k, k) if isinstance(k, int) else k
        for p in range(4):
            a, b = divmod((ik + p) % 4, 2)
            H = 10 + ((10 + 2 * p - kh) % 2 != a)
            W = 12 + ((12 + 2 * p - kw) % 2 != b)
            out.append(_c(0, 2, 12, 20, k, 2, p, H, W))
    return out + [_c(0, 2, 12, 20, 3, 2, 1, 1, 5)]     # a map smaller than the kernel


STRIDED = _strided()

# ---- FLIP: transposed, stride 1 — the flipped taps; p = 0 (the output grows by k - 1), k // 2, k - 1 (it shrinks) ----------------------------
_FLIP_KP = [(1, 0), (3, 0), (3, 1), (3, 2), (5, 0), (5, 2), (5, 4), (7, 0), (7, 3), (7, 6), ((3, 5), 0), ((3, 5), 1), ((3, 5), 2), ((1, 7), 0)]
FLIP = ([_c(1, 2, 17, 9, k, 1, p, 9, 17) for k, p in _FLIP_KP] +
        [_c(1, 2, 17, 9, k, 1, p, 4, 6) for k, p in ((3, 0), (3, 2), (5, 2), (7, 0), ((3, 5), 1), ((1, 7), 0))])

# ---- SMALL: the conv_small_kind gates (csrc/conv_small.hip) with their neighbours, wgrad_small_applicable; 306 pixels: a ragged last block ----
_SM = (2, 9, 17)
SMALL_KIND1 = [(0, _SM[0], Ci, Co, 3, 3, 1, 1, 0, 0) + _SM[1:] for Ci in (1, 3) for Co in (8, 16, 24, 64)]
SMALL_KIND2 = [(0, _SM[0], Ci, Co, 1, 1, 1, 0, 0, 0) + _SM[1:] for Ci in (4, 16, 60, 64) for Co in (1, 3)]
SMALL_KIND3 = [(1, _SM[0], Ci, Co, 1, 1, 1, 0, 0, 0) + _SM[1:] for Ci in (1, 3) for Co in (8, 16, 64)]
SMALL_OUTSIDE = [_c(0, 2, 2, 16, 3, 1, 1, 9, 17), _c(0, 2, 1, 12, 3, 1, 1, 9, 17), _c(0, 2, 3, 72, 3, 1, 1, 9, 17), _c(0, 2, 68, 3, 1, 1, 0, 9, 17),
                 _c(1, 2, 2, 16, 1, 1, 0, 9, 17)]
SMALL_WGRAD = [_c(0, 2, 1, 32, 3, 1, 1, 9, 17), _c(0, 2, 3, 4, 3, 1, 1, 9, 17)]    # (with 1 -> 16 / 64, 3 -> 8 / 64, 16 -> 1 / 3 above)
SMALL = SMALL_KIND1 + SMALL_KIND2 + SMALL_KIND3 + SMALL_OUTSIDE + SMALL_WGRAD

# ---- SPLIT: bf16x3 training calls: x converted once, forward from split, the weight gradient on wgrad2_kernel's glue form -----------------
# (8, 136): two 128-row tiles; (72, 8): a second column tile with a half-empty tail; k7 s2 falls back to launch_wgrad
_SPLIT_CH = ((8, 8), (24, 40), (8, 136), (72, 8))
_SPLIT_LAYERS = ((0, 3, 1, 1), (0, 3, 2, 1), (0, 2, 2, 0), (0, 5, 2, 2), (1, 4, 2, 1), (0, 7, 2, 3))   # (tr, k, s, p)
SPLIT = [_c(tr, 2, Ci, Co, k, s, p, *((19, 21) if (a + b) % 2 == 0 else (9, 7)))
         for a, (Ci, Co) in enumerate(_SPLIT_CH) for b, (tr, k, s, p) in enumerate(_SPLIT_LAYERS)]
C16 = [_c(tr, 2, Ci, 16, 3, 1, 1, 9, 17) for Ci in (16, 32, 48, 64) for tr in (0, 1)]                # the c16 gate (csrc/conv16.hip)

# ---- CONVQ: the schedule-driven kernel, forward (the smallest grid exq_preferred takes; the phase form; output padding) and as the
#      data gradient's adjoint layer with the output padding made from the rows / columns the forward dropped ----------------------------------
CONVQ_FWD = [_c(0, 256, 16, 64, 3, 2, 1, 9, 9), _c(1, 1, 16, 64, 4, 2, 1, 3, 5)] + [_c(1, 1, 16, 64, 4, 2, 1, 3, 5, op) for op in ((1, 1), (1, 0), (0, 1))]
CONVQ_FWD_PYTHON = (0, 1)          # through ops.conv2d_ex_from_split; the rest through ctypes (the wrapper passes no output padding)
CONVQ_BWD = [_c(0, 2, 64, 16, 3, 2, 1, H, W) for H, W in ((7, 10), (8, 9), (7, 9), (8, 10))] + [_c(0, 2, 64, 16, 4, 2, 1, 9, 12)]

# ---- WAVES8: the 8-wave workgroup of the glue (ex_mw: bf16x3, input step 1, >= 512 workgroups) with a ragged second half tile.
#      The stride-2 case needs N = 86 (at N = 22 its phases have 132 workgroups each): 1.5e6 output elements, the one case above 5e5 ----------
WAVES8 = [_c(1, 86, 8, 8, 3, 1, 1, 17, 33), _c(1, 86, 8, 8, 4, 2, 1, 17, 33)]

TABLES = {"PHASES": PHASES, "STRIDED": STRIDED, "FLIP": FLIP, "SMALL": SMALL, "SPLIT": SPLIT, "C16": C16, "CONVQ_FWD": CONVQ_FWD,
          "CONVQ_BWD": CONVQ_BWD, "WAVES8": WAVES8}
BOTH_MODES = ("PHASES", "STRIDED", "FLIP", "SMALL")       # through ops.conv2d_ex in f32 and bf16x3; the other tables are bf16x3 routes
# vpx_conv2d_act_fwd / _bwd with ReLU: (table, index) — Co = 6, 20, 9 and 16 (colsum's scalar and vector form); the SMALL shape (3 -> 16,
# conv_small kind 1) must bypass the streaming kernels
ACT = [("PHASES", 8), ("STRIDED", 5), ("FLIP", 2), ("SMALL", 5)]
DETERMINISTIC = [("SPLIT", 7), ("CONVQ_BWD", 0)]
# (table, index) -> n: another seed for a case that missed a condition of tests/test_glue_host.py (both: two elements on the kink)
RESEED = {("PHASES", 23): 1, ("FLIP", 6): 1}


def all_cases():
    return [(t, i) for t in TABLES for i in range(len(TABLES[t]))]


def case_id(table, i):
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = TABLES[table][i]
    return f"{table}{i}-{'t' if tr else 'c'}n{N}ci{Ci}co{Co}k{kh}x{kw}s{s}p{p}op{oph}{opw}m{H}x{W}"


def out_shape(c):
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    if tr:
        return (H - 1) * s - 2 * p + kh + oph, (W - 1) * s - 2 * p + kw + opw
    return (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1


def adjoint_out_pad(c):
    """The output padding of the data gradient's adjoint layer: the rows / columns a convolution dropped."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    return (0, 0) if tr else ((H + 2 * p - kh) % s, (W + 2 * p - kw) % s)


def has_bias_only_outputs(c):
    """Output rows / columns no input pixel reaches (a convolution padded past its kernel; output padding past the padding): without a
    bias their pre-activation is exactly 0, on the kink."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    return (oph > p or opw > p) if tr else (p >= kh or p >= kw)


def variant(table, i):
    """How the entry point is handed case i: with a bias or None, x channels-last or plain NCHW, with LeakyReLU(0.2) or without an
    activation — cycled as conv_same_ref.variant. A case with bias-only outputs keeps its bias (see has_bias_only_outputs)."""
    return {"bias": i % 3 != 1 or has_bias_only_outputs(TABLES[table][i]), "channels_last": i % 2 == 0, "slope": 0.0 if i % 4 == 1 else SLOPE}


def inputs(table, i):
    """x [N, Ci, H, W], w in the reference's layout, b [Co] and gy [N, Co, Ho, Wo] in float32 (gy before the kink's zeros)."""
    c = TABLES[table][i]
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    tag = f"glue.{table}.{c}.{RESEED.get((table, i), 0)}."
    return {"x": seeded_randn((N, Ci, H, W), name_seed(tag + "x")),
            "w": seeded_randn((Ci, Co, kh, kw) if tr else (Co, Ci, kh, kw), name_seed(tag + "w"), 1.0 / float(Ci * kh * kw) ** 0.5),
            "b": seeded_randn((Co,), name_seed(tag + "b"), 0.1),
            "gy": seeded_randn((N, Co) + out_shape(c), name_seed(tag + "gy"))}


def conv(c, x, w, b):
    """The pre-activation."""
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    if tr:
        return F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=(oph, opw))
    return F.conv2d(x, w, b, stride=s, padding=p)


def activate(pre, slope=0.0, relu=False):
    return F.relu(pre) if relu else (F.leaky_relu(pre, slope) if slope != 0.0 else pre)


def reference(c, x, w, b, gy, slope=0.0, relu=False, dtype=torch.float64):
    """On the CPU in `dtype`: y, the autograd gradients of (y * gy).sum() with respect to x, w and b (None without a bias), and the
    pre-activation."""
    lv = [None if t is None else t.detach().clone().to(dtype).requires_grad_(True) for t in (x, w, b)]
    pre = conv(c, *lv)
    y = activate(pre, slope, relu)
    (y * gy.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": lv[0].grad, "dw": lv[1].grad, "db": None if b is None else lv[2].grad, "pre": pre.detach()}


def off_kink(pre, y):
    """Elements whose fp64 pre-activation is farther than KINK_BAR * max|y| from the activation's kink."""
    return pre.abs() > KINK_BAR * float(y.abs().max())


@functools.lru_cache(maxsize=None)
def case(table, i, relu=False):
    """(inputs, fp64 reference, zeroed share) of one case under its variant: computed once, shared among the tests, never written. With
    an activation gy is zero on the kink."""
    c, v = TABLES[table][i], variant(table, i)
    slope = 0.0 if relu else v["slope"]
    t = inputs(table, i)
    if not v["bias"]:
        t["b"] = None
    share = 0.0
    if relu or slope != 0.0:
        with torch.no_grad():
            pre = conv(c, *[None if a is None else a.double() for a in (t["x"], t["w"], t["b"])])
            keep = off_kink(pre, activate(pre, slope, relu))
        t["gy"] = t["gy"] * keep
        share = 1.0 - float(keep.double().mean())
    return t, reference(c, t["x"], t["w"], t["b"], t["gy"], slope, relu), share
