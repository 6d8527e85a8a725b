"""float64 restatement of the frame adapter (csrc/adapt.hip; vp_suite/utils/compatibility.py: ScaleToModel / ScaleToTest of
utils/models.py:7-64, then TF.Resize) and the case table of tests/test_adapt_host.py and tests/test_gpu_adapt.py.

The two affine steps are the reference's expressions in float64; the resize is frames_ref.resize: the SAME float32 source coordinates
and weights as the kernels (ATen's expressions), the interpolation itself accumulated in float64."""
import numpy as np

import frames_ref


def coords(n_in, n_out, fused=False):
    """frames_ref.coords — the kernels' float32 source coordinates, every operation rounded on its own. fused=True: s * (d + 0.5) - 0.5
    rounded ONCE, as a build of ATen whose compiler contracts the expression into a fused multiply-add computes it (the product of two
    float32 values is exact in float64); the two differ by at most one unit in the last place of the coordinate."""
    if not fused:
        return frames_ref.coords(n_in, n_out)
    s = np.float64(np.float32(n_in) / np.float32(n_out))
    src = np.maximum((s * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(np.float32), np.float32(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0.astype(np.float32)


def adapt(x, out_hw=None, src_range=(0.0, 1.0), dst_range=(0.0, 1.0), fused_coords=False):
    """float64 [..., oh, ow] from float32 frames x [..., h, w]: scale first, then resize; equal ranges / equal sizes skip their step.
    fused_coords: see coords(); the kernels' contract is False."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    v = x.astype(np.float64)
    (s_lo, s_hi), (d_lo, d_hi) = (float(a) for a in src_range), (float(a) for a in dst_range)
    if (s_lo, s_hi) != (d_lo, d_hi):
        v = (v - s_lo) / (s_hi - s_lo)          # [0., 1.]
        v = v * (d_hi - d_lo) + d_lo            # [dst_lo, dst_hi]
    if out_hw is not None and tuple(out_hw) != tuple(x.shape[-2:]):
        # frames_ref.resize takes float32 taps; the scaled taps are float64 here, so the same expressions are restated on them
        h, w = x.shape[-2:]
        y0, y1, ly = coords(h, out_hw[0], fused_coords)
        x0, x1, lx = coords(w, out_hw[1], fused_coords)
        lx, ly = lx.astype(np.float64), ly.astype(np.float64)
        rows = v[..., :, x0] * (1.0 - lx) + v[..., :, x1] * lx
        v = rows[..., y0, :] * (1.0 - ly)[:, None] + rows[..., y1, :] * ly[:, None]
    return v


def bound(dst_range):
    """Bound of |kernel - adapt()| for inputs inside the source range: 10 float32 unit roundoffs times max(1, |dst_lo|, |dst_hi|) — the
    bound of the dataset resize (frames_ref.resize_bound)."""
    return 10.0 * 2.0 ** -24 * max(1.0, abs(dst_range[0]), abs(dst_range[1]))


# (H, W) -> (oh, ow): the sizes at which the kernels can go wrong — single pixels, up and down, the affine-only path with an element
# count that is no multiple of 4, odd sizes, exact halving, and rows around the 64-pixel mark on either side (16-byte stores: ow % 4 == 0)
SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((2, 2), (1, 1)), ((5, 7), (5, 7)), ((5, 7), (8, 12)), ((9, 10), (4, 3)), ((8, 8), (4, 4)),
          ((6, 63), (5, 64)), ((6, 64), (5, 64)), ((6, 65), (5, 64)), ((5, 64), (6, 63)), ((5, 64), (6, 65))]
CHANNELS = [1, 3]
FRAMES = [1, 5]
RANGES = [((0.0, 1.0), (-1.0, 1.0)), ((-1.0, 1.0), (0.0, 255.0)), ((0.0, 1.0), (0.0, 1.0))]


def frames(shape, src_range, seed):
    """float32 frames inside src_range (both ends present)."""
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=np.float32) * np.float32(src_range[1] - src_range[0]) + np.float32(src_range[0])
    x = np.clip(x, np.float32(src_range[0]), np.float32(src_range[1]))
    x.reshape(-1)[0] = src_range[0]
    x.reshape(-1)[-1] = src_range[1]
    return x
