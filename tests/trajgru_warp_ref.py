"""TrajGRU blocks with PRESCRIBED flows: the case table and the fp64 reference runner of tests/test_gpu_trajgru_warp.py (GPU parity)
and tests/test_trajgru_warp_cases.py (validity of every case, on the CPU).

`flows_conv.weight = 0` and `flows_conv.bias = (fx_0, fy_0, ..., fx_{L-1}, fy_{L-1})` make every flow field a known constant, in pixels,
through the public op (`traj_ops.trajgru_seq`); the "jitter" variant puts 1e-2 of the usual `flows_conv.weight` on top, so that the
fractional parts of the sampling coordinates differ from pixel to pixel. Every other parameter, the input, the initial state and the
cotangent are seeded as in tests/test_gpu_fuzz.py. The reference is oracle.torch_ref.trajgru_seq on the CPU with autograd; for its
duration F.grid_sample and F.leaky_relu are wrapped, which yields the two figures that decide whether a case may be compared to a tight
bar at all: the distance of the sampling coordinates from the bilinear sampler's cell boundaries and of the LeakyReLU pre-activations
from 0 (the block's kinks: tests/test_gpu_fuzz.py explains what they do to a gradient).

Sampling coordinate of the reference (traj_gru.py:148-162 with grid_sample's default alignment): sx = (x - fx) * W / (W - 1) - 0.5
(W / max(W - 1, 1) on a 1-wide map). Zero flow is a resample by W / (W - 1), not the identity — and on an ODD side the centre pixel then
sits exactly on a cell boundary (sx = (W - 1) / 2): clear_of_boundaries() below moves such components, and says by how much."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import name_seed, seeded_rand, seeded_randn

NAMES = ("i2h", "i2f_conv1", "h2f_conv1", "flows_conv", "ret")
PARAM_KEYS = tuple(f"{n}.{kind}" for n in NAMES for kind in ("weight", "bias"))
SLOPE = 0.2
B, CIN, C = 2, 3, 8
COORD_MARGIN = 1e-3     # every sampling coordinate within reach of the map is at least this far from an integer ...
PREACT_MARGIN = 1e-5    # ... and every LeakyReLU pre-activation at least this far from 0 (both in the fp64 reference alone)

# max-normalised bounds (parity.relmax) of test_trajgru_block_vs_golden / test_random_trajgru_blocks_vs_oracle
FWD_F32, FWD_BF16X3, GRAD_F32 = 2e-5, 1e-4, 1e-4

# tag: H, W, T, fields ((fx, fy) in pixels), out (indices of the fields that sample nothing but padding), jitter, rev (seed revision)
Case = collections.namedtuple("Case", "tag H W T fields out jitter rev")


def side_clearance(f, n):
    """Smallest distance from an integer of s = (i - f) * n / (n - 1) - 0.5 over the pixels i of a side of n whose s is within reach of
    the map (-1 <= s <= n); None when there is none."""
    s = (np.arange(n) - f) * (n / max(n - 1, 1)) - 0.5
    s = s[(s >= -1 - COORD_MARGIN) & (s <= n + COORD_MARGIN)]
    return float(np.abs(s - np.round(s)).min()) if s.size else None


def clear_of_boundaries(f, n):
    """The flow table's fractional parts are adjusted where a side breaks them: a component that brings a coordinate of that side within
    0.03 px of a cell boundary moves by 0.07 px towards zero flow (a zero component by +0.1 px), until it does not. On an odd side every
    multiple of (n - 1) / 2n does that, zero first: zero flow is a resample by n / (n - 1) whose centre pixel sits exactly on a boundary."""
    for _ in range(4):
        d = side_clearance(f, n)
        if d is None or d >= 0.03:
            return round(f, 2)
        f = f + 0.1 if f == 0.0 else f - float(np.copysign(0.07, f))
    raise AssertionError((f, n))


def _fields(H, W, table):
    return tuple((clear_of_boundaries(fx, W), clear_of_boundaries(fy, H)) for fx, fy in table)


def near_fields(H, W):
    """Zero flow; one, two and four taps out on each of the four sides; only the last column / the first row in."""
    return _fields(H, W, ((0.0, 0.0), (2.3, -1.6), (-3.4, 2.7), (W - 0.6, 0.0), (0.0, -(H - 0.6))))


def far_fields(H, W):
    """One field inside (the state still reaches the gates through the warp), then fields that are out entirely: just, far (inside the
    int range) and beyond it."""
    return _fields(H, W, ((0.3, -0.4),)) + ((W + 3.25, 0.4), (0.4, -(H + 3.25)), (1e6, -1e6), (3e9, 3e9))


def narrow_fields(H, W):
    return _fields(H, W, ((0.0, 0.0), (0.3, -0.4))) + ((W + 3.25, 0.4),)


# Seed revisions: a case whose seeded tensors put a coordinate or a pre-activation inside a margin gets the next revision (the seed
# names are "warp.<tag>.r<rev>.*"); tests/test_trajgru_warp_cases.py holds every case below to both margins. Rejected (revision: what
# was too close):
#   6x7.far.T2.jitter  r0: a pre-activation at 3.1e-6; r1: one at 7.2e-7
REJECTED = {"6x7.far.T2.jitter": (0, 1)}


def _rev(tag):
    return 1 + max(REJECTED.get(tag, (-1,)))


def _make_cases():
    out = []
    for (H, W) in ((6, 7), (5, 8)):
        for T in (1, 2):
            for jitter in (False, True):
                for grp, fields, oidx in (("near", near_fields(H, W), ()), ("far", far_fields(H, W), (1, 2, 3, 4))):
                    tag = f"{H}x{W}.{grp}.T{T}.{'jitter' if jitter else 'bias'}"
                    out.append(Case(tag, H, W, T, fields, oidx, jitter, _rev(tag)))
    for (H, W) in ((1, 7), (6, 1), (1, 1), (2, 2)):
        tag = f"{H}x{W}.narrow.T2.bias"
        out.append(Case(tag, H, W, 2, narrow_fields(H, W), (2,), False, _rev(tag)))
    return collections.OrderedDict((c.tag, c) for c in out)


CASES = _make_cases()
MAIN = [t for t in CASES if ".narrow." not in t]
NARROW = [t for t in CASES if ".narrow." in t]
PARENT_HASH_CASE = "6x7.near.T2.bias"   # in-range and just-out flows only: defined in every build of the kernel


def tensors(case):
    """The block's ten parameters (reference names), x, h0 and the cotangent of `out`, float32 on the CPU."""
    L = len(case.fields)
    seed = f"warp.{case.tag}.r{case.rev}"
    shapes = {"i2h": (3 * C, CIN, 3, 3), "i2f_conv1": (32, CIN, 5, 5), "h2f_conv1": (32, C, 5, 5), "flows_conv": (2 * L, 32, 5, 5), "ret": (3 * C, L * C, 1, 1)}
    P = {}
    for n in NAMES:
        s_ = shapes[n]
        P[n + ".weight"] = seeded_randn(s_, name_seed(f"{seed}.{n}.w"), 1.0 / np.sqrt(s_[1] * s_[2] * s_[3]))
        P[n + ".bias"] = seeded_randn((s_[0],), name_seed(f"{seed}.{n}.b"), 0.1)
    P["flows_conv.weight"] = P["flows_conv.weight"] * (1e-2 if case.jitter else 0.0)
    P["flows_conv.bias"] = torch.tensor([v for f in case.fields for v in f], dtype=torch.float32)
    x = seeded_rand((B, case.T, CIN, case.H, case.W), name_seed(seed + ".x"))
    h0 = seeded_randn((B, C, case.H, case.W), name_seed(seed + ".h"), 0.5)
    g = seeded_randn((B, case.T, C, case.H, case.W), name_seed(seed + ".g"))
    return P, x, h0, g


def loss_of(out, hT, g):
    return (out * g).sum() + 0.5 * (hT * hT).sum()


Reference = collections.namedtuple("Reference", "out hT grads coord_dist preact_dist reach")


@functools.lru_cache(maxsize=None)
def reference(tag, dtype=torch.float64):
    """oracle.torch_ref.trajgru_seq in `dtype` on the CPU: outputs, every gradient (keys "x", "h0" and PARAM_KEYS), the smallest
    distance of a sampling coordinate within reach of the map from an integer, the smallest |pre-activation| of the two LeakyReLUs,
    and per field whether any of its samples is within reach. Computed once per (case, dtype); callers must not modify it."""
    from oracle import torch_ref as tr
    case = CASES[tag]
    P, x, h0, g = tensors(case)
    P = {k: v.to(dtype).requires_grad_(True) for k, v in P.items()}
    x, h0, g = x.to(dtype).requires_grad_(True), h0.to(dtype).requires_grad_(True), g.to(dtype)
    seen = {"coord": float("inf"), "pre": float("inf"), "reach": []}
    plain_sample, plain_leaky = F.grid_sample, F.leaky_relu

    def watching_sample(inp, grid, **kw):
        with torch.no_grad():
            Hs, Ws = inp.shape[-2:]
            sx, sy = ((grid[..., 0] + 1) * Ws - 1) / 2, ((grid[..., 1] + 1) * Hs - 1) / 2
            reach = (sx >= -1 - COORD_MARGIN) & (sx <= Ws + COORD_MARGIN) & (sy >= -1 - COORD_MARGIN) & (sy <= Hs + COORD_MARGIN)
            seen["reach"].append(bool(reach.any()))
            if reach.any():
                d = torch.minimum((sx - sx.round()).abs(), (sy - sy.round()).abs())[reach]
                seen["coord"] = min(seen["coord"], float(d.min()))
        return plain_sample(inp, grid, **kw)

    def watching_leaky(t, *a, **kw):
        seen["pre"] = min(seen["pre"], float(t.detach().abs().min()))
        return plain_leaky(t, *a, **kw)

    F.grid_sample, F.leaky_relu = watching_sample, watching_leaky
    try:
        out, hT = tr.trajgru_seq(x, h0, case.T, P, len(case.fields), SLOPE)
    finally:
        F.grid_sample, F.leaky_relu = plain_sample, plain_leaky
    loss_of(out, hT, g).backward()
    grads = {"x": x.grad, "h0": h0.grad}
    grads.update({k: P[k].grad for k in PARAM_KEYS})
    L = len(case.fields)
    reach = [any(seen["reach"][l::L]) for l in range(L)]
    return Reference(out.detach(), hT.detach(), grads, seen["coord"], seen["pre"], reach)


def bars(tag):
    """name -> (bound, reference-side error): the suite's bound, or 3 x the error of the fp32 oracle against its own fp64 run where
    that error exceeds a third of the bound (the rule of bar_from in tests/test_gpu_unet3d.py). "out" / "hT" carry the f32 bound."""
    r64, r32 = reference(tag, torch.float64), reference(tag, torch.float32)
    res = {}
    pairs = [("out", r32.out, r64.out, FWD_F32), ("hT", r32.hT, r64.hT, FWD_F32)] + [(k, r32.grads[k], r64.grads[k], GRAD_F32) for k in r64.grads]
    for name, a, b, base in pairs:
        err = float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))
        res[name] = (base if err <= base / 3 else 3 * err, err)
    return res
