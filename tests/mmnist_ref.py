"""Plain numpy restatement of Moving MNIST generated on the fly (vp_suite/datasets/mmnist_on_the_fly.py with base_dataset.py's
preprocess()): the sampling order, the trajectory rule and the pixel arithmetic, each written down from its description. It is the
reference side of tests/test_mmnist_host.py (against the fixture drawn from the upstream class) and of tests/test_gpu_mmnist.py
(bit for bit against csrc/mmnist.hip).

Sampling: four default_rng(seed) generators — glyph index, speed, acceleration, position — on the split's seed (train 3x+2, val 3x+1,
test 3x). Per digit: the index; two positions in [0, S - s), the first drawn is x; speed x then speed y from [-max, max], each redrawn
while |v| < min_speed; the acceleration, drawn and never used.
Trajectory, per axis, integers: p += v; if p + s > S: p = S - s, v = -v; elif p < 0: p = -p, v = -v. The move comes before the draw.
Pixel, float64: frame[y:y+s, x:x+s] += glyph / 255 per digit in order; clip to [0, 1]; * 255; / 255; to float32; then only if
(lo, hi) != (0, 1): * float32(hi - lo), + float32(lo), two float32 operations. All channels equal."""
import numpy as np

SPLIT_SEED = {"train": lambda x: 3 * x + 2, "val": lambda x: 3 * x + 1, "test": lambda x: 3 * x}
RNG_SEED = 4115


class Sampler:
    def __init__(self, split, n_glyphs, glyph_size, img_size=64, num_digits=2, min_speed=2, max_speed=5, min_acc=0, max_acc=0, rng_seed=RNG_SEED):
        seed = SPLIT_SEED[split](rng_seed)
        self.r_index, self.r_speed, self.r_acc, self.r_pos = (np.random.default_rng(seed) for _ in range(4))
        self.n_glyphs, self.room, self.num_digits = n_glyphs, img_size - glyph_size, num_digits
        self.min_speed, self.max_speed, self.min_acc, self.max_acc = min_speed, max_speed, min_acc, max_acc

    def _redraw(self, rng, bound, least):
        while True:
            v = rng.integers(-bound, bound + 1)
            if abs(v) >= least:
                return v

    def digit(self):
        index = self.r_index.integers(self.n_glyphs)
        x = self.r_pos.integers(0, self.room)
        y = self.r_pos.integers(0, self.room)
        vx = self._redraw(self.r_speed, self.max_speed, self.min_speed)
        vy = self._redraw(self.r_speed, self.max_speed, self.min_speed)
        self._redraw(self.r_acc, self.max_acc, self.min_acc)
        return [index, y, x, vy, vx]

    def params(self, n):
        """int32 [n, num_digits, 5] rows (glyph index, y0, x0, vy, vx) of the next n sequences."""
        return np.array([[self.digit() for _ in range(self.num_digits)] for _ in range(n)], dtype=np.int32)


def move(p, v, img_size, glyph_size):
    """One move of one axis -> (p, v)."""
    p = p + v
    if p + glyph_size > img_size:
        return img_size - glyph_size, -v
    if p < 0:
        return -p, -v
    return p, v


def trajectory(p, v, n_frames, img_size, glyph_size):
    """Positions of one axis in frames 0 .. n_frames-1 (frame i: after i + 1 moves)."""
    out = []
    for _ in range(n_frames):
        p, v = move(p, v, img_size, glyph_size)
        out.append(p)
    return out


def render(digits, params, n_frames, channels, img_size, value_range=(0.0, 1.0)):
    """float32 [B, n_frames, channels, img_size, img_size] from digits uint8 [N, s, s] and params [B, D, 5]."""
    digits, params = np.asarray(digits), np.asarray(params)
    s = digits.shape[1]
    B, D = params.shape[:2]
    canvas = np.zeros((B, n_frames, img_size, img_size), dtype=np.float64)
    for b in range(B):
        for d in range(D):
            index, y0, x0, vy, vx = (int(v) for v in params[b, d])
            ys, xs = trajectory(y0, vy, n_frames, img_size, s), trajectory(x0, vx, n_frames, img_size, s)
            glyph = digits[index].astype(np.float64) / 255.0
            for f in range(n_frames):
                canvas[b, f, ys[f]:ys[f] + s, xs[f]:xs[f] + s] += glyph
    canvas = np.clip(canvas, 0.0, 1.0)
    canvas = canvas * 255.0
    canvas = canvas / 255.0
    x = canvas.astype(np.float32)
    lo, hi = float(value_range[0]), float(value_range[1])
    if lo != 0.0 or hi != 1.0:
        x = x * np.float32(hi - lo)
        x = x + np.float32(lo)
    assert x.dtype == np.float32
    return np.ascontiguousarray(np.repeat(x[:, :, None], channels, axis=2))
