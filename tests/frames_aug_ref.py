"""Plain numpy restatement of the photometric augmentations and erasing as csrc/frames_aug.hip computes them (include/vpx.h lists the
operations), and of the host draws of datasets.StoredVPDataset: the reference side of tests/test_frames_aug_host.py and
tests/test_gpu_frames_aug.py. torchvision is not imported anywhere; the pixel formulas are those its pinned version (0.11.2) applies to
float tensors, cited by function name: functional_tensor.invert, solarize, autocontrast, rgb_to_grayscale, _blend, adjust_brightness,
adjust_contrast, adjust_saturation, adjust_hue (_rgb2hsv, _hsv2rgb), functional.normalize, functional.erase, and the parameter draws of
transforms.ColorJitter.get_params and transforms.RandomErasing.get_params.

apply(v, rows): every operation ONE float32 rounding at a time, in the kernel's order; the contrast mean is a float64 sum rounded to
float32 once. apply(v, rows, twin=True): the float64 twin — identical up to the first contrast or hue row, float64 from there on, on the
same float32 inputs, parameters and constants (the gray weights are the float32 ones), the mean kept in float64.

CONTRAST bound (contrast_bound(), counted from the expression, u = 2^-24). The kernel forms K = clamp(fl(fl(f v) + fl(g m))), the twin
T = clamp(f v + g M) with M the float64 mean and m = fl(M') the kernel's, M' a float64 sum in another order (|M' - M| ~ 1e-16 |M|, which
can flip the rounding): |m - M| <= 2 u |M| (one float32 ulp).
    fl(f v)            u |f| |v|
    fl(g m) - g M      |g| |m - M| + u |g| |m|   <=  3 u |g| |M|
    the sum            u |f v + g m|             <=  u (|f| |v| + |g| |M|)
    the clamp          1-Lipschitz
With A >= |v| over the frame (so |M| <= A: the gray weights sum to 0.9999) that is (2 |f| + 4 |g|) A u, to first order; the factor
1 + 2^-10 covers the second order. It contains the issue's starting point 2 |g| |M| u + 2 max(1, |v|) u term by term except that the
final rounding is counted on the unclamped sum (|f| |v| + |g| |M| instead of max(1, |v|)). Operations that follow in the test chains are
Lipschitz and add their own float32 roundings (the twin runs them in float64): with e the error and a the magnitude so far,
    brightness (f)     e' = |f| e + u |f| a,                       a' = min(|f| a + e', 1)
    invert             e' = e + u (1 + a),                          a' = 1 + a
    normalize (m, s)   e' = (e + u (a + |m|)) / |s| + u (a + |m|) / |s|,   a' = (a + |m|) / |s|     (the worst channel)

HUE tolerance. Measured on the CPU: the largest |apply(x, rows) - apply(x, rows, twin=True)| over the inputs and chains of
tests/test_gpu_frames_aug.py::HUE_CASES (hue_cases() below builds them; neither side is the code under test) is HUE_F32_VS_F64; the
GPU test allows HUE_FACTOR = 4 times that: the factor covers a different rounding of the divisions and of floor at a sector boundary,
where the map stays continuous. tests/test_frames_aug_host.py recomputes the figure and holds it to the constant.
That continuity holds for values in [0, 1] only. On negative values (frames in a (-1, 1) range that no clamping operation has touched)
torchvision's formulas, and so the kernel's, are not continuous — the clamps of p, q, t cut a negative v's sectors apart, s = cr / maxc
is unbounded for a small maxc and 0 * inf = NaN at maxc == 0 — and two precisions differ there by whole values (0.19 and NaN were
measured on such inputs), so no tolerance compares them. Under the (-1, 1) range the hue chains therefore begin with a brightness row,
whose clamp brings the values into [0, 1] first; under (0, 1) hue also acts on the raw values."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24

INVERT, SOLARIZE, AUTOCONTRAST, GRAY, NORMALIZE, BRIGHTNESS, CONTRAST, SATURATION, HUE, ERASE = range(1, 11)
ROW = 9

HUE_F32_VS_F64 = 1.03e-6     # measured by measure_hue_deviation() on the CPU (float32 restatement against the float64 twin): 1.0282e-6
HUE_FACTOR = 4.0


def row(op, *params):
    """One program row as the host builds it: parameters rounded to float32 once."""
    return (float(op),) + tuple(float(F32(p)) for p in params) + (0.0,) * (ROW - 1 - len(params))


def blend_row(op, f):
    return row(op, f, 1.0 - f)                       # f and 1 - f formed in double, each rounded once


def pack(programs, max_ops=16):
    out = np.zeros((len(programs), max(max_ops, max(len(p) for p in programs)), ROW), dtype=F32)
    for k, rows in enumerate(programs):
        if rows:
            out[k, :len(rows)] = np.array(rows, dtype=F32)
    return out


def _clamp(v):
    one, zero = v.dtype.type(1.0), v.dtype.type(0.0)
    return np.where(v < zero, zero, np.where(v > one, one, v))


def _gray(v):
    """rgb_to_grayscale: (0.2989 r + 0.587 g) + 0.114 b, the weights float32 in either precision."""
    t = v.dtype.type
    return (t(F32(0.2989)) * v[..., 0, :, :] + t(F32(0.587)) * v[..., 1, :, :]) + t(F32(0.114)) * v[..., 2, :, :]


def _blend(v, other, f, g):
    t = v.dtype.type
    return _clamp(t(f) * v + t(g) * other)


def _frac(v):
    return v - np.trunc(v)


def _hue(v, d):
    """adjust_hue on [..., 3, h, w]: _rgb2hsv, (h + d) % 1.0, _hsv2rgb, in v's precision."""
    t = v.dtype.type
    r, g, b = v[..., 0, :, :], v[..., 1, :, :], v[..., 2, :, :]
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, t(1.0), maxc)
    div = np.where(eqc, t(1.0), cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, (t(2.0) + rc) - bc, (t(4.0) + gc) - rc))
    h = _frac(h / t(6.0) + t(1.0))
    h = _frac(h + t(d))
    h = np.where(h < 0, h + t(1.0), h)
    h6 = h * t(6.0)
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int64) % 6
    p = _clamp(maxc * (t(1.0) - s))
    q = _clamp(maxc * (t(1.0) - f * s))
    k = _clamp(maxc * (t(1.0) - (t(1.0) - f) * s))
    pick = lambda six: np.choose(i, six)
    out = np.stack([pick([maxc, q, p, p, k, maxc]), pick([k, maxc, maxc, q, p, p]), pick([p, p, k, maxc, maxc, q])], axis=-3)
    assert out.dtype == v.dtype
    return out


def apply(v, rows, twin=False):
    """One sample v [F, C, h, w] (float32) through a program (rows as row() builds them); float32, or float64 with twin=True from the
    first contrast / hue row on. Statistics are per frame (and channel, for autocontrast)."""
    v = np.array(v, dtype=np.float64 if (twin and np.asarray(v).dtype == np.float64) else F32)    # a twin already in float64 stays there
    assert v.ndim == 4
    C, h, w = v.shape[1:]
    for r in rows:
        op = int(r[0])
        if op == 0:
            break
        if twin and op in (CONTRAST, HUE):
            v = v.astype(np.float64)
        t = v.dtype.type
        p = [t(F32(x)) for x in r[1:]]
        if op == INVERT:
            v = t(1.0) - v
        elif op == SOLARIZE:
            v = np.where(v >= p[0], t(1.0) - v, v)
        elif op == AUTOCONTRAST:
            lo, hi = v.min(axis=(-2, -1), keepdims=True), v.max(axis=(-2, -1), keepdims=True)
            const = hi == lo
            scale = t(1.0) / np.where(const, t(1.0), hi - lo)
            v = np.where(const, v, _clamp((v - lo) * scale))
        elif op == GRAY:
            assert C == 3
            v = np.repeat(_gray(v)[:, None], 3, axis=1)
        elif op == NORMALIZE:
            mean, std = np.array(p[0:C], dtype=v.dtype).reshape(1, C, 1, 1), np.array(p[4:4 + C], dtype=v.dtype).reshape(1, C, 1, 1)
            v = (v - mean) / std
        elif op == BRIGHTNESS:
            v = _blend(v, t(0.0), p[0], p[1])
        elif op == CONTRAST:
            assert C in (1, 3)
            g = _gray(v) if C == 3 else v[:, 0]
            m = g.astype(np.float64).sum(axis=(-2, -1)) / float(h * w)                 # float64 sum of the float32 values
            m = m if v.dtype == np.float64 else m.astype(F32)                         # ... rounded to float32 once
            v = _blend(v, m.reshape(-1, 1, 1, 1), p[0], p[1])
        elif op == SATURATION:
            if C == 3:
                v = _blend(v, _gray(v)[:, None], p[0], p[1])
        elif op == HUE:
            if C == 3:
                v = _hue(v, p[0])
        elif op == ERASE:
            y0, x0, eh, ew = (int(x) for x in r[1:5])
            v = v.copy()
            v[:, :, max(y0, 0):max(min(y0 + eh, h), 0), max(x0, 0):max(min(x0 + ew, w), 0)] = np.array(p[4:4 + C], dtype=v.dtype).reshape(1, C, 1, 1)
        else:
            raise ValueError(f"unknown opcode {op}")
        assert v.dtype == (np.float64 if twin and v.dtype == np.float64 else F32)
    return v


def apply_batch(x, programs, twin=False):
    """x [B, F, C, h, w] through per-sample programs."""
    return np.stack([apply(x[b], programs[b], twin) for b in range(x.shape[0])])


def contrast_bound(rows, A):
    """Bound of |kernel - twin| after a chain whose ONE contrast row is followed by brightness / invert / normalize rows only; A >= |v|
    at the contrast row's input (see the module docstring)."""
    k = [int(r[0]) for r in rows].index(CONTRAST)
    f, g = abs(rows[k][1]), abs(rows[k][2])
    e = (2.0 * f + 4.0 * g) * A * U * (1.0 + 2.0 ** -10)
    a = min(f * A + g * A, 1.0)
    for r in rows[k + 1:]:
        op = int(r[0])
        if op == 0:
            break
        if op == BRIGHTNESS:
            e = abs(r[1]) * e + U * abs(r[1]) * a
            a = min(abs(r[1]) * a + e, 1.0)
        elif op == INVERT:
            e, a = e + U * (1.0 + a), 1.0 + a
        elif op == NORMALIZE:
            worst = max((a + abs(m)) / abs(s) for m, s in zip(r[1:5], r[5:9]) if s != 0.0)
            inv = max(1.0 / abs(s) for s in r[5:9] if s != 0.0)
            e, a = e * inv + 2.0 * U * worst * (1.0 + 2.0 ** -10), worst
        else:
            raise ValueError("only brightness, invert and normalize may follow a contrast row in these chains")
    return e


# ---- inputs shared by the GPU tests and the hue measurement ----
SIZES = [(1, 1), (1, 5), (3, 7), (17, 19), (33, 40)]
RANGES = {"01": (0.0, 1.0), "11": (-1.0, 1.0)}


def raw_bytes(hw, C, seed, B=3, F=2):
    """Random bytes [B, F, h, w, C] with both ends of the type present; the frames of a sample differ."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(B, F) + tuple(hw) + (C,), dtype=np.uint8)
    flat = raw.reshape(-1)
    flat[0], flat[-1] = 0, 255
    return raw


def scaled(raw, value_range):
    """What the preprocess launch makes of raw bytes [B, F, h, w, C] without crop, resize or flip: float32 [B, F, C, h, w]."""
    v = raw.astype(F32) / F32(255.0)
    lo, hi = float(value_range[0]), float(value_range[1])
    if lo != 0.0 or hi != 1.0:
        v = v * F32(hi - lo)
        v = v + F32(lo)
    return np.ascontiguousarray(v.transpose(0, 1, 4, 2, 3))


def hue_programs():
    """Per-sample programs of the hue cases: hue last; one sample's program is empty."""
    return [[row(HUE, 0.1)],
            [],
            [blend_row(SATURATION, 1.3), row(INVERT), blend_row(BRIGHTNESS, 0.8), row(HUE, -0.37)]], \
           [[row(HUE, -0.5)], [blend_row(BRIGHTNESS, 1.2), row(HUE, 0.5)], [row(SOLARIZE, F32(128.0) / F32(255.0)), row(HUE, 0.25)]]


def hue_cases():
    """(name, x float32 [3, 2, 3, h, w], programs) of every hue case the GPU test runs."""
    for hw in SIZES:
        for tag, vr in RANGES.items():
            x = scaled(raw_bytes(hw, 3, seed=hw[0] * 100 + hw[1]), vr)
            for k, programs in enumerate(hue_programs()):
                if tag == "11":                                    # hue is compared where it is continuous: on values in [0, 1] (see above)
                    programs = [([blend_row(BRIGHTNESS, 1.1)] + rows) if rows else rows for rows in programs]
                yield f"hue_{hw[0]}x{hw[1]}_{tag}_{k}", x, programs


def measure_hue_deviation():
    """max |float32 restatement - float64 twin| over hue_cases()."""
    worst = 0.0
    for _, x, programs in hue_cases():
        worst = max(worst, float(np.abs(apply_batch(x, programs).astype(np.float64) - apply_batch(x, programs, twin=True)).max()))
    return worst


# ---- the host draws, restated: same generator, same order ----
def erase_box(rng, frame_hw, scale, ratio):
    """RandomErasing.get_params: ten attempts, None when none fits."""
    H, W = frame_hw
    for _ in range(10):
        area = H * W * float(rng.uniform(scale[0], scale[1]))
        aspect = math.exp(float(rng.uniform(math.log(ratio[0]), math.log(ratio[1]))))
        eh, ew = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if not (eh < H and ew < W):
            continue
        return int(rng.integers(0, H - eh + 1)), int(rng.integers(0, W - ew + 1)), eh, ew
    return None


def _range(x, center, clip=True):
    if x is None:
        return None
    lo, hi = (x if isinstance(x, (tuple, list)) else ((max(center - x, 0.0) if clip else center - x), center + x))
    return None if lo == hi == center else (float(lo), float(hi))


def draw_sequence(rng, augmentations, frame_hw, crop, out_chw):
    """One sequence's draws from tuple-form `augmentations`: (crop y0, crop x0, steps). `steps` is the user's list in ITS order with what
    was drawn: ("hflip",) / ("vflip",) or program rows; an erase row holds the box as drawn (not mirrored). Draw order: box row, box
    column, every flip, then the other entries in list order."""
    H, W = frame_hw
    C, h, w = out_chw
    y0 = x0 = 0
    if crop is not None and crop[0] == "random":
        y0, x0 = int(rng.integers(0, H - crop[1] + 1)), int(rng.integers(0, W - crop[2] + 1))
    elif crop is not None and crop[0] == "center":
        y0, x0 = int(round((H - crop[1]) / 2.0)), int(round((W - crop[2]) / 2.0))
    elif crop is not None:
        y0, x0 = crop[1], crop[2]
    flips = {k: bool(rng.random() < aug[1]) for k, aug in enumerate(augmentations) if aug[0] in ("hflip", "vflip")}
    per = lambda vals, fill: (tuple(vals) * C if len(vals) == 1 else tuple(vals)) + (fill,) * (4 - (C if len(vals) == 1 else len(vals)))
    seq = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x,)
    steps = []
    for k, aug in enumerate(augmentations):
        kind = aug[0]
        if kind in ("hflip", "vflip"):
            if flips[k]:
                steps.append((kind,))
        elif kind in ("invert", "autocontrast", "grayscale"):
            if rng.random() < aug[1]:
                steps.append(row({"invert": INVERT, "autocontrast": AUTOCONTRAST, "grayscale": GRAY}[kind]))
        elif kind == "solarize":
            if rng.random() < aug[2]:
                steps.append(row(SOLARIZE, aug[1]))
        elif kind == "normalize":
            steps.append(row(NORMALIZE, *per(seq(aug[1]), 0.0), *per(seq(aug[2]), 1.0)))
        elif kind == "color_jitter":
            order = [int(i) for i in rng.permutation(4)]
            ranges = [_range(aug[1], 1.0), _range(aug[2], 1.0), _range(aug[3], 1.0), _range(aug[4], 0.0, clip=False)]
            factors = [None if r is None else float(rng.uniform(r[0], r[1])) for r in ranges]
            for i in order:
                if factors[i] is not None:
                    steps.append(row(HUE, factors[i]) if i == 3 else blend_row((BRIGHTNESS, CONTRAST, SATURATION)[i], factors[i]))
        elif kind == "erase":
            if rng.random() < aug[1]:
                box = erase_box(rng, (h, w), aug[2], aug[3])
                if box is not None:
                    steps.append(row(ERASE, *box, *per(seq(aug[4]), 0.0)))
        else:
            raise ValueError(kind)
    return y0, x0, steps


def apply_in_order(v, steps, twin=False):
    """One sample [F, C, h, w] through `steps` in list order (float32, or the float64 twin), flips as explicit array flips."""
    for st in steps:
        if st[0] == "hflip":
            v = v[..., ::-1]
        elif st[0] == "vflip":
            v = v[..., ::-1, :]
        else:
            v = apply(v, [st], twin)
    return np.ascontiguousarray(v)


def flip_bits(steps):
    """The table's flip bits of what was drawn: two drawn flips of one kind cancel."""
    bits = 0
    for st in steps:
        if st[0] in ("hflip", "vflip"):
            bits ^= {"hflip": 1, "vflip": 2}[st[0]]
    return bits
