"""Float64 numpy restatement of what `vpx_grad_stats` and `vpx_adam_step_clipped` (include/vpx.h) compute: the statistics of the flat
gradient, torch.nn.utils.clip_grad_norm_'s coefficient, clip_grad_value_'s clamp, the optional skip of a non-finite step — and then the
Adam update exactly as oracle.torch_ref.adam_step_ref states it (imported, not restated). tests/test_grad_clip_host.py pins this file
against torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam in float64 on the CPU; nothing here looks at a kernel."""
import math
import os
import re

import numpy as np

from oracle.torch_ref import adam_step_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
U24 = 2.0 ** -24


def kernel_constant(name):
    """An integer `constexpr int NAME = value;` of csrc/train_tail.hip (the tests read the block cap from the code)."""
    src = open(os.path.join(ROOT, "vp-suite_amd", "csrc", "train_tail.hip")).read()
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert m, name
    return int(m.group(1))


def grad_stats_ref(g, grad_scale=1.0):
    """[|| grad_scale g ||_2, max |grad_scale g| over the finite elements (0 without any), number of non-finite elements] in float64.
    The squares of float32 values are exact in float64 and math.fsum adds them with ONE rounding, so the norm carries three roundings
    in all (the scale's square, its product with the sum, the square root). With a non-finite element the norm is not finite (inf or
    NaN: which of the two is not part of the contract)."""
    g64 = np.asarray(g, dtype=np.float64).reshape(-1)
    finite = np.isfinite(g64)
    bad = int((~finite).sum())
    gs = float(grad_scale)
    if bad:
        norm = float("nan") if np.isnan(g64).any() else float("inf")
    else:
        norm = math.sqrt(math.fsum((g64 * g64).tolist()) * (gs * gs))
    mx = gs * float(np.abs(g64[finite]).max()) if finite.any() else 0.0
    return np.array([norm, mx, float(bad)], dtype=np.float64)


def clip_coefficient(norm, max_norm):
    """clip_grad_norm_'s factor: min(1, max_norm / (norm + 1e-6)), NaN for a NaN norm (torch.clamp(max=1) keeps it); 1 without max_norm."""
    if not max_norm > 0.0:
        return 1.0
    with np.errstate(all="ignore"):
        r = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return float(r) if not r > 1.0 else 1.0


def clipped_gradient(g, grad_scale=1.0, max_norm=0.0, clip_value=0.0):
    """(float64 gradient the update sees, c, statistics): g * (grad_scale * c), then clamped to +-clip_value (NaN stays NaN)."""
    stats = grad_stats_ref(g, grad_scale)
    c = clip_coefficient(stats[0], max_norm)
    with np.errstate(all="ignore"):
        ge = np.asarray(g, dtype=np.float64) * (float(grad_scale) * c)
        if clip_value > 0.0:
            ge = np.where(ge > clip_value, clip_value, np.where(ge < -clip_value, -clip_value, ge))
    return ge, c, stats


def adam_clipped_ref(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=0.0,
                     clip_value=0.0, skip_nonfinite=False):
    """One clipped step from float32 numpy p, g, m, v: returns (p, m, v, info). The clipped gradient is formed in float64 and handed
    to adam_step_ref with grad_scale = 1, which rounds it to float32 once and runs torch.optim.Adam's update in float32 as PyTorch does
    — against the kernel's g * (float)(grad_scale c) that is ONE rounding less (the factor's). A skipped step returns its inputs.
    info: c, stats (grad_stats_ref), skipped, clamped (share of elements the clamp changed)."""
    ge, c, stats = clipped_gradient(g, grad_scale, max_norm, clip_value)
    info = {"c": c, "stats": stats, "skipped": bool(skip_nonfinite and stats[2] > 0), "clamped": 0.0}
    if clip_value > 0.0:
        with np.errstate(all="ignore"):
            info["clamped"] = float((np.abs(np.asarray(g, dtype=np.float64) * (float(grad_scale) * c)) > clip_value).mean())
    if info["skipped"]:
        return p.copy(), m.copy(), v.copy(), info
    with np.errstate(all="ignore"):
        p2, m2, v2 = adam_step_ref(p, ge, m, v, step, lr, beta1, beta2, eps, weight_decay, 1.0)
    return p2, m2, v2, info
