"""Shared inputs of the FVD tests: a seeded Inception-I3D state dict at any width divisor (keyed as InceptionI3d.state_dict()), seeded clips and
feature tables, the float64 restatements the GPU kernels are held against. Everything here is regenerated from seeds; nothing is stored."""
import atexit
import functools
import json
import os

import torch
import torch.nn.functional as F

from vp_suite_amd import measure as M

# out_channels of InceptionModule: (b0, b1a, b1b, b2a, b2b, b3b)
BLOCK_WIDTHS = {"Mixed_3b": (64, 96, 128, 16, 32, 32), "Mixed_3c": (128, 128, 192, 32, 96, 64), "Mixed_4b": (192, 96, 208, 16, 48, 64),
                "Mixed_4c": (160, 112, 224, 24, 64, 64), "Mixed_4d": (128, 128, 256, 24, 64, 64), "Mixed_4e": (112, 144, 288, 32, 64, 64),
                "Mixed_4f": (256, 160, 320, 32, 128, 128), "Mixed_5b": (256, 160, 320, 32, 128, 128), "Mixed_5c": (384, 192, 384, 48, 128, 128)}
STEM_WIDTHS = {"Conv3d_1a_7x7": 64, "Conv3d_2b_1x1": 64, "Conv3d_2c_3x3": 192}
N_FEATURES = 400
THIN = 8   # the thin network of the tests: every width of the real one divided by 8


def unit_tensors(g, name, ci, co, k, gain=1.0):
    """conv3d.weight (He-scaled, so that activations keep their size through the ReLUs) and BatchNorm tensors of one Unit3D."""
    fan_in = ci * k[0] * k[1] * k[2]
    return {f"{name}.conv3d.weight": torch.randn(co, ci, *k, generator=g) * (gain * (2.0 / fan_in) ** 0.5),
            f"{name}.bn.weight": torch.rand(co, generator=g) + 0.5, f"{name}.bn.bias": torch.randn(co, generator=g) * 0.2,
            f"{name}.bn.running_mean": torch.randn(co, generator=g) * 0.1, f"{name}.bn.running_var": torch.rand(co, generator=g) + 0.5,
            f"{name}.bn.num_batches_tracked": torch.tensor(7)}


@functools.lru_cache(maxsize=None)
def state_dict(div=THIN, in_channels=3, seed=0):
    """A seeded network keyed as InceptionI3d.state_dict(), every width the real one's divided by `div` (float32)."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd, c = {}, in_channels
    for step in M.FVD_SEQUENCE:
        if step[0] == "unit":
            sd.update(unit_tensors(g, step[1], c, STEM_WIDTHS[step[1]] // div, step[2]))
            c = STEM_WIDTHS[step[1]] // div
        elif step[0] == "block":
            w = [v // div for v in BLOCK_WIDTHS[step[1]]]
            for (b, k), ci, co in zip(M.FVD_BRANCHES, (c, c, w[1], c, w[3], c), w):
                sd.update(unit_tensors(g, f"{step[1]}.{b}", ci, co, (k, k, k)))
            c = w[0] + w[2] + w[4] + w[5]
    f = N_FEATURES // div
    sd["logits.conv3d.weight"] = torch.randn(f, c, 1, 1, 1, generator=g) * (8.0 / c ** 0.5)   # features that reach well beyond 1
    sd["logits.conv3d.bias"] = torch.randn(f, generator=g) * 0.5
    return sd


def clips(shape, seed):
    """Two seeded clip batches [B, T, C, h, w] in [-1, 1]: smooth structure plus noise, the second a perturbed copy of the first."""
    g = torch.Generator().manual_seed(2000 + seed)
    B, T, C, h, w = shape
    coarse = torch.rand(B, T, C, max(h // 4, 1), max(w // 4, 1), generator=g) * 2 - 1
    a = F.interpolate(coarse.flatten(0, 1), size=(h, w), mode="bilinear", align_corners=False).view(shape)
    a = (a + 0.3 * (torch.rand(shape, generator=g) * 2 - 1)).clamp(-1, 1)
    b = (a + 0.4 * (torch.rand(shape, generator=g) * 2 - 1)).clamp(-1, 1)
    return a.contiguous(), b.contiguous()


# ---- the parity record: with VPX_FVD_PARITY_OUT=FILE in the environment every figure the GPU tests of the three FVD modules hand to record() is
#      written there ONCE, when the process ends (how profiles/fvd_parity.json is made) -------------------------------------------------------
_FIGURES = {}


def _write_figures():
    out = os.environ.get("VPX_FVD_PARITY_OUT")
    if out and _FIGURES:
        with open(out, "w") as fh:
            json.dump({"what": "FVD on one MI355X against float64 on the CPU, from tests/test_gpu_fvd_kernels.py, tests/test_gpu_fvd_edges.py and tests/test_gpu_fvd.py",
                       "metric": "kernels and trunk: max|got - ref| / max|ref|; the trunk's bound is max(4 x the float32 CPU chain's own error, 1e-6); distances: "
                                 "|got - ref| in absolute terms against the stated bound",
                       "cases": _FIGURES}, fh, indent=1)


atexit.register(_write_figures)


def record(name, **figures):
    _FIGURES[name] = figures


def relmax(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ---- Frechet distance inputs -----------------------------------------------------------------------------------------------------------
FRECHET_KINDS = ("shifted", "identical", "rank1")


def feature_tables(b, n, kind, seed=0):
    """Two float32 tables [b, n]: "shifted" (different spreads and means), "identical", "rank1" (every centred table of rank <= 1); the
    kinds of FRECHET_EDGE_KINDS are built by edge_feature_tables() below."""
    if kind in FRECHET_EDGE_KINDS:
        return edge_feature_tables(b, n, kind, seed)
    g = torch.Generator().manual_seed(3000 + 17 * b + n + seed)
    if kind == "rank1":
        p = torch.randn(b, 1, generator=g) * torch.randn(1, n, generator=g) + torch.randn(1, n, generator=g)
        t = torch.randn(b, 1, generator=g) * torch.randn(1, n, generator=g) * 1.5 - 0.5
        return p.contiguous(), t.contiguous()
    p = torch.randn(b, n, generator=g) * (torch.rand(1, n, generator=g) * 2 + 0.5) + torch.randn(1, n, generator=g)
    if kind == "identical":
        return p, p.clone()
    t = torch.randn(b, n, generator=g) * (torch.rand(1, n, generator=g) * 3 + 0.25) + torch.randn(1, n, generator=g) * 2
    return p, t


def frechet_scale(pred, target):
    """fact sum Ep^2 + fact sum Et^2 + |mu_p - mu_t|^2: the positive terms the tolerance of the distance is stated in."""
    p, t = pred.double(), target.double()
    b = p.shape[0]
    fact = 1.0 if b < 2 else 1.0 / (b - 1)
    ep, et = p - p.mean(dim=0), t - t.mean(dim=0)
    return float(fact * ep.square().sum() + fact * et.square().sum() + (p.mean(dim=0) - t.mean(dim=0)).square().sum())


def frechet_bound(pred, target):
    """1e-10 of the positive terms (float64 rounding over at most n b ~ 1e5 terms is about 1e-11 of them) + 2 b sqrt(1e-15), the epsilon's own
    contribution at singular values that are zero."""
    return 1e-10 * frechet_scale(pred, target) + 2 * pred.shape[0] * 1e-15 ** 0.5


# ---- the cases recorded from the reference (tools/gen_golden_fvd.py -> tests/golden/fvd_*.npz) ----------------------------------------------
CHUNK_MAX_T = 128
WASSERSTEIN_CASES = tuple((b, n, kind) for b in (1, 2, 3, 8) for n in (7, 400) for kind in FRECHET_KINDS)
ODD_MAP, EVEN_MAP = (9, 13, 10), (16, 12, 9)   # both parities of the padding rule on every axis
# (Ci, Co, kernel, stride, map): the stem at thin width on both maps, a 3x3x3 and a 1x1x1 layer
UNIT_CASES = ((3, 8, (7, 7, 7), (2, 2, 2), ODD_MAP), (2, 8, (7, 7, 7), (2, 2, 2), EVEN_MAP), (12, 16, (3, 3, 3), (1, 1, 1), (3, 5, 6)),
              (24, 8, (1, 1, 1), (1, 1, 1), (2, 7, 7)))
POOL_FORMS = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)))
POOL_CASES = tuple((k, s, m, kind) for k, s in POOL_FORMS for m in (ODD_MAP, EVEN_MAP) for kind in ("mixed", "negative"))
BLOCK_CASES = ((24, (8, 12, 16, 2, 4, 4), (3, 5, 6)), (32, (16, 16, 24, 4, 12, 8), (2, 7, 7)))   # Mixed_3b and Mixed_3c at 1/8 width


def case_id(case):
    return "_".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)


def _case_generator(case):
    return torch.Generator().manual_seed(4000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(case))) % 100003)


def unit_case(case):
    """(x [2, Ci, T, H, W], the unit's tensors keyed "u....")."""
    ci, co, k, _, shape = case
    g = _case_generator(case)
    return torch.randn(2, ci, *shape, generator=g), unit_tensors(g, "u", ci, co, k)


def pool_case(case):
    _, _, shape, kind = case
    g = _case_generator(case)
    return torch.randn(1, 2, *shape, generator=g) if kind == "mixed" else -torch.rand(1, 2, *shape, generator=g) - 0.25


def block_case(case):
    """(x [2, Ci, T, H, W], the block's tensors keyed "m.{branch}....")."""
    ci, w, shape = case
    g = _case_generator(case)
    x = torch.randn(2, ci, *shape, generator=g)
    tensors = {}
    for (b, k), c_in, c_out in zip(M.FVD_BRANCHES, (ci, ci, w[1], ci, w[3], ci), w):
        tensors.update(unit_tensors(g, f"m.{b}", c_in, c_out, (k, k, k)))
    return x, tensors


def network_case():
    """One 9-frame clip [1, 9, 3, 224, 224] (already at the I3D size: no resize on either side) for the whole network at the real widths,
    state_dict(1): what InceptionI3d.extract_features is recorded on."""
    return clips((1, 9, 3, 224, 224), seed=77)[0]


def folded(tensors, name):
    """(weight, bias) float64 of the unit `name` with its BatchNorm folded in, by the package's own rule."""
    return M.fvd_fold(tensors[f"{name}.conv3d.weight"], *(tensors[f"{name}.bn.{p}"] for p in ("weight", "bias", "running_mean", "running_var")))


# ---- kernel references in float64, channels-first as torch takes them ---------------------------------------------------------------------
def conv3d_same_ref(x, w, bias, stride, relu):
    """x [N, Ci, T, H, W] -> float64 [N, Co, To, Ho, Wo]: F.pad with the SAME rule, F.conv3d, bias, optional ReLU."""
    k = tuple(w.shape[2:])
    y = F.conv3d(M._fvd_pad(x.double(), k, stride), w.double(), bias.double(), stride=stride)
    return F.relu(y) if relu else y


def maxpool3d_same_ref(x, kernel, stride):
    return F.max_pool3d(M._fvd_pad(x, kernel, stride), kernel, stride)


# ---- edge cases (tests/test_gpu_fvd_edges.py; host checks of these tables in tests/test_fvd_host.py) ---------------------------------------
def same_rule(size, k, s):
    """(front, out) of one axis, the SAME rule written out on its own (not measure.same_pad, not the library's)."""
    pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return pad // 2, -(-size // s)


# (kernel, stride, map T x H x W): anisotropic on every axis; narrower than the kernel on W; even kernels; stride above the kernel on every axis
EDGE_FORMS = (((2, 3, 5), (1, 2, 3), (4, 6, 9)), ((3, 1, 7), (2, 1, 1), (5, 3, 3)), ((1, 4, 2), (1, 3, 2), (2, 7, 5)), ((1, 1, 2), (2, 3, 3), (5, 7, 8)))
ADJACENT_FORMS = tuple((k, s, m) for k, s in (((1, 3, 3), (1, 2, 2)), ((3, 1, 1), (2, 1, 1))) for m in (ODD_MAP, EVEN_MAP))   # pool-adjacent
EDGE_WIDTHS = ((3, 5), (4, 64), (12, 70), (16, 130))   # (Ci, Co): run below, at and above one K step; one, two and three N tiles
TAP_CO = 5


def form_id(form):
    return "k" + "".join(map(str, form[0])) + "s" + "".join(map(str, form[1])) + "-" + "x".join(map(str, form[2]))


def out_positions(form, n):
    """M of the implicit GEMM: output positions of n maps."""
    m = n
    for size, k, s in zip(form[2], form[0], form[1]):
        m *= same_rule(size, k, s)[1]
    return m


def ragged_batch(form):
    """The smallest N >= 3 at which M spans several 64-position tiles with a ragged last one."""
    n = 3
    while out_positions(form, n) <= 64 or out_positions(form, n) % 64 == 0:
        n += 1
    return n


def unit_taps(kernel, ci_count, co_count=TAP_CO):
    """(co, ci, dt, dh, dw) of the eight corners of the kernel and its centre (corners coincide where a side is 1: they stay, on other
    channels); tap i sits on input channel i % Ci and output channel i % Co, so nine taps reach every channel of both."""
    corners = [(a, b, c) for a in (0, kernel[0] - 1) for b in (0, kernel[1] - 1) for c in (0, kernel[2] - 1)]
    taps = corners + [tuple(k // 2 for k in kernel)]
    return tuple((i % co_count, i % ci_count, *t) for i, t in enumerate(taps))


def unit_tap_expected(x, co_count, tap, kernel, stride):
    """float32 [N, Co, To, Ho, Wo]: what a convolution whose only non-zero weight is 1.0 at `tap` gives on x [N, Ci, T, H, W] — output
    (ot, oh, ow) of channel co is x[ci, ot st - front_t + dt, ...] where that index lies in the map, 0 where it lies in the padding and in
    every other channel. Index arithmetic only."""
    co, ci, *d = tap
    index, inside = [], []
    for size, k, s, dd in zip(x.shape[2:], kernel, stride, d):
        front, out = same_rule(size, k, s)
        i = torch.arange(out) * s - front + dd
        inside.append((i >= 0) & (i < size))
        index.append(i.clamp(0, size - 1))
    y = torch.zeros(x.shape[0], co_count, *(len(i) for i in index))
    picked = x[:, ci][:, index[0]][:, :, index[1]][:, :, :, index[2]]
    keep = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
    y[:, co] = torch.where(keep, picked, torch.zeros(()))
    return y, keep


def edge_conv_case(form, ci, co, n, seed=0):
    """(x [n, Ci, T, H, W], w [Co, Ci, kt, kh, kw] scaled to unit-size outputs, bias)."""
    k, _, shape = form
    g = torch.Generator().manual_seed(5000 + seed + ci * 131 + co * 7 + sum(v * (i + 1) for i, v in enumerate(k + shape)))
    x = torch.randn(n, ci, *shape, generator=g)
    w = torch.randn(co, ci, *k, generator=g) / (ci * k[0] * k[1] * k[2]) ** 0.5
    return x, w, torch.randn(co, generator=g) * 0.3


def window_mask(shape, kernel, stride, at):
    """bool [To, Ho, Wo]: the pooling windows that hold the element `at` of a map of `shape` (same_rule again)."""
    axes = []
    for size, k, s, a in zip(shape, kernel, stride, at):
        front, out = same_rule(size, k, s)
        first = torch.arange(out) * s - front
        axes.append((first <= a) & (a < first + k))
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


# (kernel, stride, map, {what the element is: its index}): one NaN per channel, in the order of the dict
POOL_NAN_CASES = (
    ((3, 3, 3), (3, 3, 3), (6, 6, 6), {"first of a window": (3, 3, 3), "inner": (4, 1, 4), "last of a window": (2, 5, 2)}),
    ((3, 3, 3), (2, 2, 2), (5, 5, 5), {"shared by eight windows": (1, 1, 1), "shared by two": (2, 3, 2), "inner of one": (2, 2, 2),
                                       "in a border window that holds padding": (0, 4, 0)}),
    ((3, 3, 3), (1, 1, 1), (4, 4, 4), {"shared by 27 windows": (1, 2, 1), "in border windows that hold padding": (0, 0, 3), "last element of the map": (3, 3, 3)}),
    ((1, 3, 3), (1, 2, 2), (2, 5, 6), {"shared by four windows": (1, 1, 2), "last of the last window, next to padding": (0, 4, 5)}),
)
POOL_EDGE_FORMS = (((1, 2, 2), (1, 2, 2)), ((3, 1, 1), (2, 1, 1)), ((2, 3, 1), (1, 3, 2)))
POOL_EDGE_MAPS = (ODD_MAP, EVEN_MAP, (1, 1, 1))
POOL_EDGE_C = 70   # an output row of channels crosses a 256-thread block

STAGE_SIZES = ((1, 1), (224, 100), (100, 224), (225, 223), (300, 448), (7, 500))   # one-pixel, one scale 1, down, up, both at once

FRECHET_EDGE_KINDS = ("equal_sigma", "graded", "scaled_up", "scaled_down")
FRECHET_LANE_CASES = tuple((b, n, "shifted") for b in (63, 64, 65, 127, 128, 129, 255) for n in (1, 7, 400))
FRECHET_KIND_CASES = tuple((b, 400, kind) for kind in FRECHET_EDGE_KINDS for b in (2, 3, 33, 64, 65, 256))
FRECHET_EDGE_CASES = FRECHET_LANE_CASES + FRECHET_KIND_CASES
GRADED_SPAN = 1e-9


def _centred_factors(g, b, n):
    """(U [b, b - 1] with orthonormal columns that sum to zero, Q [b - 1, n] with orthonormal rows), float64: U S Q is a centred table of
    rank b - 1 whose singular values are the diagonal of S."""
    a = torch.randn(b, b - 1, generator=g, dtype=torch.float64)
    u = torch.linalg.qr(a - a.mean(dim=0))[0]
    q = torch.linalg.qr(torch.randn(n, b - 1, generator=g, dtype=torch.float64))[0].t()
    return u, q


def edge_feature_tables(b, n, kind, seed=0):
    """The kinds feature_tables() hands over to: "equal_sigma" (both centred tables multiples of one U Q: G = c (I - 1 1^T / b), b - 1 equal
    singular values and the zero centring forces), "graded" (centred tables U S Q with S falling geometrically from 1 to 1e-9, own factors per
    table; float32 storage lifts the smallest values to its rounding, about 1e-8), "scaled_up" / "scaled_down" ("shifted" times 2^20 / 2^-6)."""
    if kind in ("scaled_up", "scaled_down"):
        p, t = feature_tables(b, n, "shifted", seed)
        f = 2.0 ** 20 if kind == "scaled_up" else 2.0 ** -6
        return p * f, t * f
    if b - 1 > n:
        raise ValueError(f"{kind}: b - 1 <= n (got b={b}, n={n})")
    g = torch.Generator().manual_seed(6000 + 17 * b + n + seed)
    if kind == "equal_sigma":
        u, q = _centred_factors(g, b, n)
        e = u @ q
        mp, mt = torch.randn(1, n, generator=g, dtype=torch.float64), torch.randn(1, n, generator=g, dtype=torch.float64)
        return (3.0 * e + mp).float().contiguous(), (2.0 * e + mt).float().contiguous()
    if kind == "graded":
        s = torch.logspace(0, -9, b - 1, dtype=torch.float64) if b > 2 else torch.ones(1, dtype=torch.float64)
        tables = []
        for scale in (1.0, 1.5):
            u, q = _centred_factors(g, b, n)
            tables.append((scale * (u * s) @ q).float().contiguous())
        return tuple(tables)
    raise ValueError(f"unknown kind {kind!r}")


def centred_sigma(table):
    """Singular values (float64, descending) of the centred table."""
    t = table.double()
    return torch.linalg.svdvals(t - t.mean(dim=0))
