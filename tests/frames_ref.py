"""Plain numpy restatement of the stored-frame chain (vp_suite/base/base_dataset.py preprocess :233-273, postprocess :286-297, the gray
repeat of datasets/mmnist.py:56) as csrc/frames.hip computes it: the reference side of tests/test_frames_host.py (against the fixture
drawn from the upstream class and against torch's interpolate) and of tests/test_gpu_frames.py.

Exact paths: every step is one float32 operation, as in the kernel. Resize: the SAME float32 source coordinates and weights as the
kernel (ATen's expressions), the interpolation itself accumulated in float64."""
import random

import numpy as np

F32 = np.float32


def scale(raw, value_range=(0.0, 1.0)):
    """float32 values of raw uint8 / uint16 / float32 elements: / 255 (/ 65535; float32 passes), then only for a range other than
    (0, 1) `* float32(hi - lo)` and `+ float32(lo)`, the difference formed in double."""
    raw = np.asarray(raw)
    if raw.dtype == np.uint8:
        v = raw.astype(F32) / F32(255.0)
    elif raw.dtype == np.uint16:
        v = raw.astype(F32) / F32(65535.0)
    elif raw.dtype == np.float32:
        v = raw.copy()
    else:
        raise ValueError(f"unknown element type {raw.dtype}")
    lo, hi = float(value_range[0]), float(value_range[1])
    if lo != 0.0 or hi != 1.0:
        v = v * F32(hi - lo)
        v = v + F32(lo)
    assert v.dtype == F32
    return v


def coords(n_in, n_out):
    """(i0, i1, lambda) per destination index, in float32: s = f(in) / f(out); src = max(s * (d + 0.5) - 0.5, 0); i0 = int(src);
    i1 = min(i0 + 1, in - 1); lambda = src - i0."""
    s = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32)
    src = s * (d + F32(0.5)) - F32(0.5)
    assert src.dtype == F32
    src = np.maximum(src, F32(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = src - i0.astype(F32)
    assert lam.dtype == F32
    return i0, i1, lam


def resize(v, out_hw):
    """float64 bilinear resize (align_corners=False, no antialiasing) of float32 taps v [..., h, w]: horizontally, then vertically."""
    h, w = v.shape[-2:]
    oh, ow = out_hw
    y0, y1, ly = coords(h, oh)
    x0, x1, lx = coords(w, ow)
    v = v.astype(np.float64)
    lx, ly = lx.astype(np.float64), ly.astype(np.float64)
    rows = v[..., :, x0] * (1.0 - lx) + v[..., :, x1] * lx
    return rows[..., y0, :] * (1.0 - ly)[:, None] + rows[..., y1, :] * ly[:, None]


def center_offset(full, size):
    return int(round((full - size) / 2.0))


def table(seqs, boxes=None, flips=None):
    """int32 [n, 4] rows (sequence index, crop y0, crop x0, flip bits)."""
    n = len(seqs)
    boxes = boxes or [(0, 0)] * n
    flips = flips or [0] * n
    return np.array([(s, y, x, f) for s, (y, x), f in zip(seqs, boxes, flips)], dtype=np.int32).reshape(n, 4)


def preprocess(src, rows, n_frames, seq_step=1, crop_size=None, out_size=None, c_out=None, value_range=(0.0, 1.0)):
    """[B, n_frames, C_out, oh, ow] from src [N, T', H, W(, Cs)]: float32 and bit-exact without resize, float64 with it. The order is the
    reference's: scale, crop, resize, flip."""
    src = np.asarray(src)
    if src.ndim == 4:
        src = src[..., None]
    N, Tp, H, W, Cs = src.shape
    ch, cw = crop_size or (H, W)
    oh, ow = out_size or (ch, cw)
    c_out = c_out or Cs
    assert c_out == Cs or (Cs == 1 and c_out == 3)
    out = []
    for s, y0, x0, bits in np.asarray(rows):
        assert 0 <= s < N and 0 <= y0 and y0 + ch <= H and 0 <= x0 and x0 + cw <= W
        seq = src[s, 0:(n_frames - 1) * seq_step + 1:seq_step, y0:y0 + ch, x0:x0 + cw]   # [F, ch, cw, Cs]
        assert seq.shape[0] == n_frames
        v = scale(seq, value_range).transpose(0, 3, 1, 2)
        if (oh, ow) != (ch, cw):
            v = resize(v, (oh, ow))
        if bits & 1:
            v = v[..., ::-1]
        if bits & 2:
            v = v[..., ::-1, :]
        if c_out != Cs:
            v = np.repeat(v, 3, axis=1)
        out.append(v)
    return np.ascontiguousarray(np.stack(out))


def postprocess(x, value_range=(0.0, 1.0)):
    """uint8 [..., h, w, c] from float32 [..., c, h, w]: ((x - lo) / (hi - lo)) * 255 in float32, clamp, truncate; NaN gives 0."""
    x = np.asarray(x)
    assert x.dtype == F32
    lo, hi = float(value_range[0]), float(value_range[1])
    v = x - F32(lo)
    v = v / F32(hi - lo)
    v = v * F32(255.0)
    assert v.dtype == F32
    v = np.where(np.isnan(v), F32(0.0), np.clip(v, F32(0.0), F32(255.0)))
    nd = x.ndim
    return np.ascontiguousarray(v.astype(np.uint8).transpose(list(range(nd - 3)) + [nd - 2, nd - 1, nd - 3]))


def train_val_indices(n, ratio, seed=1234):
    """Both halves of the reference's _random_split (base_dataset.py:377-400)."""
    n_train = int(n * ratio)
    idx = list(range(n))
    random.Random(seed).shuffle(idx)
    return idx[:n_train], idx[n_train:]


def resize_bound(value_range=(0.0, 1.0)):
    """Bound of |kernel - resize()| (see tests/test_gpu_frames.py): 10 float32 unit roundoffs times max(|lo|, |hi|, 1)."""
    return 10.0 * 2.0 ** -24 * max(abs(value_range[0]), abs(value_range[1]), 1.0)
