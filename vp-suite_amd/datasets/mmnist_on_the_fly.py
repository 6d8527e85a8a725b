"""Moving MNIST generated on the fly (vp_suite/datasets/mmnist_on_the_fly.py, registry key "MMF"), drawn on the GPU.

The host keeps what must stay the reference's: the four numpy generators of a split and their draw order, so that equal glyphs and seed
give the reference's sequences. One int32 row (glyph index, y0, x0, vy, vx) per sample and digit goes to the device in one copy, and ONE
launch of csrc/mmnist.hip writes the [B, seq_len, C, S, S] batch where the model reads it. There is no host rendering path.

Glyphs: `digits=` a uint8 [N, s, s] table, or `data_dir=` with MNIST's raw idx files. Nothing is ever downloaded. procedural_digits()
draws a stand-in table (NOT MNIST) for tests and benchmarks."""
import os
import struct

import numpy as np
import torch

from .. import _lib
from .._lib import VpxError, check, ptr
from ..utils import set_from_kwarg
from .base import VPDataset

IDX_FILES = {"train": "train-images-idx3-ubyte", "test": "t10k-images-idx3-ubyte"}   # every split but "train" reads the t10k file


def read_idx_images(path):
    """uint8 [n, h, w] from an idx3-ubyte file (big-endian header: 0, 0, type 0x08, 3 dimensions, then the three sizes)."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < 16 or data[:4] != b"\x00\x00\x08\x03":
        raise VpxError(f"{path}: not an idx file of unsigned bytes with 3 dimensions")
    n, h, w = struct.unpack(">III", data[4:16])
    if len(data) != 16 + n * h * w:
        raise VpxError(f"{path}: header says {n}x{h}x{w} bytes, the file holds {len(data) - 16}")
    return np.frombuffer(data, dtype=np.uint8, offset=16).reshape(n, h, w).copy()


# seven-segment strokes in the unit square, (x0, y0, x1, y1), and the segments of the ten digits
_XL, _XR, _YT, _YM, _YB = 0.30, 0.70, 0.16, 0.50, 0.84
_SEGMENTS = {"A": (_XL, _YT, _XR, _YT), "B": (_XR, _YT, _XR, _YM), "C": (_XR, _YM, _XR, _YB), "D": (_XL, _YB, _XR, _YB),
             "E": (_XL, _YM, _XL, _YB), "F": (_XL, _YT, _XL, _YM), "G": (_XL, _YM, _XR, _YM)}
_DIGIT_SEGMENTS = ["ABCDEF", "BC", "ABGED", "ABGCD", "FGBC", "AFGCD", "AFGECD", "ABC", "ABCDEFG", "ABCDFG"]


def procedural_digits(n=16, size=28):
    """uint8 [n, size, size]: a deterministic glyph table drawn here — seven-segment digits (glyph i shows i % 10; every further ten is
    slanted and thickened differently) with a soft edge, so that the values spread over 0 ... 255. A stand-in for tests and benchmarks
    on machines without the MNIST files; it is not MNIST. Only +, -, *, /, sqrt, min and max in float64: the same bytes everywhere."""
    c = (np.arange(size, dtype=np.float64) + 0.5) / size
    y, x = np.meshgrid(c, c, indexing="ij")
    soft = 1.5 / size
    out = np.zeros((n, size, size), dtype=np.uint8)
    for i in range(n):
        shear = (0.0, 0.18, -0.18)[(i // 10) % 3]
        half = 0.055 + 0.012 * ((i // 10) % 4)
        val = np.zeros((size, size))
        for name in _DIGIT_SEGMENTS[i % 10]:
            x0, y0, x1, y1 = _SEGMENTS[name]
            x0, x1 = x0 + shear * (0.5 - y0), x1 + shear * (0.5 - y1)
            dx, dy = x1 - x0, y1 - y0
            t = np.minimum(np.maximum(((x - x0) * dx + (y - y0) * dy) / (dx * dx + dy * dy), 0.0), 1.0)
            ex, ey = x - (x0 + t * dx), y - (y0 + t * dy)
            dist = np.sqrt(ex * ex + ey * ey)
            val = np.maximum(val, np.minimum(np.maximum((half - dist) / soft + 0.5, 0.0), 1.0))
        out[i] = np.floor(val * 255.0 + 0.5).astype(np.uint8)
    return out


def check_params(params, n_glyphs, glyph_size, img_size):
    """The table a launch is handed, checked where it can be read: [B, D, 5] rows (glyph index, y0, x0, vy, vx) with the index inside
    the glyph table, the start inside the image and a speed that ONE reflection brings back inside (|v| <= img_size - glyph_size)."""
    p = np.asarray(params)
    if p.ndim != 3 or p.shape[2] != 5 or p.shape[0] < 1 or p.shape[1] < 1 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"params must be an integer table [B, D, 5] (got {p.dtype} {p.shape})")
    room = img_size - glyph_size
    if p[..., 0].min() < 0 or p[..., 0].max() >= n_glyphs:
        raise ValueError(f"glyph index outside [0, {n_glyphs})")
    if p[..., 1:3].min() < 0 or p[..., 1:3].max() > room:
        raise ValueError(f"start position outside [0, {room}]")
    if np.abs(p[..., 3:5]).max() > room:
        raise ValueError(f"speed beyond {room} pixels per frame: one reflection would not bring the glyph back inside")
    return np.ascontiguousarray(p, dtype=np.int32)


def generate_frames(digits, params, n_frames, num_channels, img_size, value_range=(0.0, 1.0)):
    """float32 [B, n_frames, num_channels, img_size, img_size] on the device of `digits` (a uint8 GPU tensor [N, s, s]) from the host
    table `params` [B, D, 5]: one host-to-device copy of the table, one launch (csrc/mmnist.hip)."""
    if not (torch.is_tensor(digits) and digits.is_cuda and digits.dtype == torch.uint8 and digits.ndim == 3 and digits.shape[1] == digits.shape[2]):
        raise VpxError("generate_frames: digits must be a uint8 GPU tensor [N, s, s]; frames are generated by a HIP kernel, there is no CPU fallback")
    n_glyphs, s = digits.shape[0], digits.shape[1]
    if s >= img_size:   # (before the table is read against img_size - s)
        raise ValueError(f"the {s}x{s} glyphs do not move inside a {img_size}x{img_size} image")
    table = check_params(params.cpu().numpy() if torch.is_tensor(params) else params, n_glyphs, s, img_size)
    B, D = table.shape[:2]
    digits = digits.contiguous()
    dev_table = torch.from_numpy(table).to(digits.device)
    out = torch.empty((B, n_frames, num_channels, img_size, img_size), dtype=torch.float32, device=digits.device)
    with torch.cuda.device(digits.device):
        rc = _lib.lib().vpx_mmnist_frames(ptr(digits), n_glyphs, s, ptr(dev_table), B, D, n_frames, num_channels, img_size,
                                          float(value_range[0]), float(value_range[1]), ptr(out),
                                          torch.cuda.current_stream().cuda_stream)
    check(rc, "vpx_mmnist_frames")
    return out


class _BatchLoader:
    """len(dataset) // batch_size batches (one more, smaller one without drop_last), each from one launch."""

    def __init__(self, dataset, batch_size, drop_last):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        full, rest = divmod(len(dataset), batch_size)
        self.dataset = dataset
        self.sizes = [batch_size] * full + ([rest] if rest and not drop_last else [])

    def __len__(self):
        return len(self.sizes)

    def __iter__(self):
        for n in self.sizes:
            yield self.dataset.batch(n)


class MovingMNISTOnTheFly(VPDataset):
    """Two (num_digits) glyphs moving linearly over a black image, bouncing off the walls and overlapping each other; digits, start
    positions and speeds are drawn per sequence. The index passed to __getitem__ is ignored, as in the reference."""
    NAME = "Moving MNIST - On the fly"
    REFERENCE = "https://arxiv.org/abs/1502.04681"
    IS_DOWNLOADABLE = "No (bring MNIST's raw idx files, or a glyph table)"
    ON_THE_FLY = True
    VALID_SPLITS = ["train", "val", "test"]
    MIN_SEQ_LEN = 1e8   # unbounded: depends on the requested sequence length only
    ACTION_SIZE = 0
    DATASET_FRAME_SHAPE = (64, 64, 3)
    DEFAULT_N_SEQS = {"train": 9600, "val": 400, "test": 1000}
    SPLIT_SEED_OFFSETS = {"train": lambda x: 3 * x + 2, "val": lambda x: 3 * x + 1, "test": lambda x: 3 * x}   # one RNG stream per split

    min_speed = 2
    max_speed = 5
    min_acc = 0
    max_acc = 0
    num_channels = 3
    num_digits = 2
    rng_seed = 4115   # the test split's seed becomes 12345
    n_seqs = None
    img_size = 64
    device = "cuda"

    def __init__(self, split, digits=None, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["digits", "digit_id_rng", "speed_rng", "acc_rng", "pos_rng"]
        for name in ("min_speed", "max_speed", "min_acc", "max_acc", "num_channels", "num_digits", "rng_seed", "img_size"):
            set_from_kwarg(self, dataset_kwargs, name)
        self.device = dataset_kwargs.get("device", self.device)
        if self.num_channels not in [1, 3]:
            raise ValueError("num_channels for dataset needs to be in [1, 3].")
        self.img_shape = (self.num_channels, self.img_size, self.img_size)   # (square: img_size is one int)
        self.DATASET_FRAME_SHAPE = (self.img_size, self.img_size, self.num_channels)
        self.digits = self._load_digits(digits)
        self.digit_size = int(self.digits.shape[1])
        room = self.img_size - self.digit_size
        if room < 1:
            raise ValueError(f"the {self.digit_size}x{self.digit_size} glyphs do not move inside a {self.img_size}x{self.img_size} image")
        if self.num_digits < 1 or not 0 <= self.min_speed <= self.max_speed or not 0 <= self.min_acc <= self.max_acc:
            raise ValueError("num_digits must be >= 1, and 0 <= min_speed <= max_speed, 0 <= min_acc <= max_acc")
        if self.max_speed > room:
            raise ValueError(f"max_speed {self.max_speed} exceeds img_size - glyph size = {room}: one reflection would not bring the glyph back inside")
        self.n_seqs = dataset_kwargs.get("n_seqs") or self.DEFAULT_N_SEQS[self.split]
        self._digits_dev = None
        self.reset_rng()

    def _load_digits(self, digits):
        if digits is None:
            name = IDX_FILES["train" if self.split == "train" else "test"]
            tried = [] if self.data_dir is None else [os.path.join(str(self.data_dir), "MNIST", "raw", name), os.path.join(str(self.data_dir), name)]
            found = [p for p in tried if os.path.isfile(p)]
            if not found:
                raise VpxError(f"'{self.NAME}' needs a glyph table: pass digits= (uint8 [N, s, s]) or data_dir= holding MNIST's raw file "
                               f"'{name}' (looked for: {tried or 'no data_dir given'}). Nothing is downloaded.")
            digits = read_idx_images(found[0])
        digits = digits.detach().cpu().numpy() if torch.is_tensor(digits) else np.asarray(digits)
        if digits.dtype != np.uint8 or digits.ndim != 3 or digits.shape[0] < 1 or digits.shape[1] != digits.shape[2]:
            raise ValueError(f"digits must be a uint8 table [N, s, s] (got {digits.dtype} {digits.shape})")
        return np.ascontiguousarray(digits)

    def __len__(self):
        return self.n_seqs

    def reset_rng(self):
        """Four generators on the split's seed — glyph index, speed, acceleration, position — each drawn from for its own purpose only."""
        seed = self.SPLIT_SEED_OFFSETS[self.split](self.rng_seed)
        self.digit_id_rng, self.speed_rng, self.acc_rng, self.pos_rng = (np.random.default_rng(seed) for _ in range(4))

    def _sample_digit(self):
        """(glyph index, y0, x0, vy, vx) in the reference's draw order (mmnist_on_the_fly.py:106-131): the index; two positions below
        img_size - glyph size, x first; speed x, then speed y, each redrawn while slower than min_speed; the acceleration, drawn and unused."""
        index = self.digit_id_rng.integers(len(self.digits))
        room = self.img_size - self.digit_size
        x0, y0 = self.pos_rng.integers(0, room), self.pos_rng.integers(0, room)
        speed = []
        for _ in range(2):
            v = None
            while v is None or abs(v) < self.min_speed:
                v = self.speed_rng.integers(-self.max_speed, self.max_speed + 1)
            speed.append(v)
        acc = None
        while acc is None or abs(acc) < self.min_acc:
            acc = self.acc_rng.integers(-self.max_acc, self.max_acc + 1)
        return index, y0, x0, speed[1], speed[0]

    def sample_params(self, n):
        """int32 [n, num_digits, 5]: the draws of the next n sequences (host only: advances the generators, touches no GPU)."""
        return np.array([[self._sample_digit() for _ in range(self.num_digits)] for _ in range(n)], dtype=np.int32).reshape(n, self.num_digits, 5)

    def batch(self, n):
        """The reference's dict for n consecutive samples from ONE launch: frames [n, seq_len, C, S, S] on the GPU, actions zeros
        [n, total_frames, 1], origin. Equal to n __getitem__ calls, in the same RNG order."""
        if not self.ready_for_usage:
            raise RuntimeError("Dataset is not yet ready for usage (maybe you forgot to call set_seq_len()).")
        if n < 1:
            raise ValueError("batch(n) needs n >= 1")
        if self._digits_dev is None:
            self._digits_dev = torch.from_numpy(self.digits).to(self.device)
        frames = generate_frames(self._digits_dev, self.sample_params(n), self.seq_len, self.num_channels, self.img_size,
                                 (self.value_range_min, self.value_range_max))
        actions = torch.zeros((n, self.total_frames, 1), device=frames.device)   # [b, t, a]: to be disregarded by the training logic
        return {"frames": frames, "actions": actions, "origin": ["generated on-the-fly"] * n}

    def __getitem__(self, i):
        data = self.batch(1)
        return {"frames": data["frames"][0], "actions": data["actions"][0], "origin": data["origin"][0]}

    def loader(self, batch_size, drop_last=True, shuffle=False, seed=None):
        """An iterable of len(self) // batch_size batches: what VPModel.train_iter / eval_iter take as `loader`. `shuffle` and `seed` are
        taken for the stored datasets' signature and change nothing: every sample is drawn when it is asked for, whatever its index."""
        return _BatchLoader(self, batch_size, drop_last)
