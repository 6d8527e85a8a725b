"""Dataset base classes with the reference's surface (vp_suite/base/base_dataset.py).

VPDataset: split handling, set_seq_len() and its sequence-length rule, the value range, `config`. A dataset that is generated on the GPU
produces its frames at their final size and value range in the generating kernel, so it has no preprocess() chain and refuses `crop` and
`augmentations` (SUPPORTS_TRANSFORMS = False).

StoredVPDataset: sequences held as ONE raw tensor [N, T', H, W(, C)] — on the GPU, or in pinned host memory — and the reference's
preprocess() / postprocess() chain (convert, permute, scale, crop, resize, flip) as one launch of csrc/frames.hip per batch and
direction. No ATen op touches a pixel between the stored bytes and the batch a model reads. The colour and erasing augmentations of the
reference's list run as per-sample programs in at most one further launch (csrc/frames_aug.hip), in place on the batch.

Stored actions (`actions=` [N, T', A]) are kept where the frames are and a batch's rows are gathered by one more launch of csrc/frames.hip
(vpx_actions_gather) from the table of the frames launch. WHAT DIFFERS FROM THE REFERENCE: a stored dataset with actions puts
`supports_actions = True` into its `config`. No dataset of the reference sets that key, although its compatibility check reads it, so
there an action-conditional model is accepted by no dataset at all; here it is accepted by the datasets that really carry actions."""
import math
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import ops
from .._lib import VpxError
from ..utils import get_public_attrs, set_from_kwarg


class VPDataset(Dataset):
    """Not usable directly after creation: set_seq_len() fixes the sequence length first (base_dataset.py:47-51)."""
    NON_CONFIG_VARS = ["functions", "ready_for_usage", "total_frames", "seq_len", "frame_offsets", "data_dir"]

    NAME: str = NotImplemented
    REFERENCE: str = None
    IS_DOWNLOADABLE: str = None
    ON_THE_FLY: bool = False
    SUPPORTS_TRANSFORMS: bool = False      # True: the class has the preprocess() chain and takes `crop` / `augmentations` / `img_size`
    VALID_SPLITS = ["train", "test"]
    MIN_SEQ_LEN: int = NotImplemented
    ACTION_SIZE: int = NotImplemented
    DATASET_FRAME_SHAPE = NotImplemented   # (h, w, c)

    img_shape = NotImplemented             # (c, h, w) of a returned frame
    split: str = None
    seq_step: int = 1
    data_dir: str = None
    value_range_min: float = 0.0
    value_range_max: float = 1.0

    def __init__(self, split: str, **dataset_kwargs):
        super().__init__()
        if split not in self.VALID_SPLITS:
            raise ValueError(f"parameter '{split}' has to be one of the following: {self.VALID_SPLITS}")
        self.split = split
        set_from_kwarg(self, dataset_kwargs, "seq_step")
        self.data_dir = dataset_kwargs.get("data_dir", self.data_dir)
        set_from_kwarg(self, dataset_kwargs, "value_range_min")
        set_from_kwarg(self, dataset_kwargs, "value_range_max")
        if not self.SUPPORTS_TRANSFORMS and (dataset_kwargs.get("crop") is not None or dataset_kwargs.get("augmentations")):
            raise NotImplementedError("'crop' and 'augmentations' are not part of this build: frames are generated at their final size")
        self.ready_for_usage = False   # True once the sequence length has been set

    @property
    def config(self) -> dict:
        """The dataset's configuration: its public attributes plus the keys every model reads (base_dataset.py:147-163)."""
        attrs = get_public_attrs(self, "config", non_config_vars=self.NON_CONFIG_VARS)
        img_c, img_h, img_w = self.img_shape
        return {**attrs, "img_h": img_h, "img_w": img_w, "img_c": img_c, "action_size": self.ACTION_SIZE,
                "tensor_value_range": [self.value_range_min, self.value_range_max], "NAME": self.NAME}

    def set_seq_len(self, context_frames: int, pred_frames: int, seq_step: int):
        """seq_len = (context_frames + pred_frames - 1) * seq_step + 1 (base_dataset.py:165-187)."""
        total_frames = context_frames + pred_frames
        seq_len = (total_frames - 1) * seq_step + 1
        if self.MIN_SEQ_LEN < seq_len:
            raise ValueError(f"Dataset '{self.NAME}' supports videos with up to {self.MIN_SEQ_LEN} frames, which is exceeded by your configuration: "
                             f"{{context frames: {context_frames}, pred frames: {pred_frames}, seq step: {seq_step}}}")
        self.total_frames = total_frames
        self.seq_len = seq_len
        self.seq_step = seq_step
        self.frame_offsets = range(0, total_frames * seq_step, seq_step)
        self.ready_for_usage = True

    def reset_rng(self):
        pass

    @classmethod
    def get_train_val(cls, **dataset_kwargs):
        """(training, validation) datasets of a class with a split of its own for each (base_dataset.py:333-358). A class with
        ["train", "test"] only splits its training samples by index: StoredVPDataset does."""
        if cls.VALID_SPLITS != ["train", "val", "test"]:
            raise NotImplementedError(f"dataset class '{cls.__name__}' has no 'val' split and no samples that could be split by index")
        return cls("train", **dataset_kwargs), cls("val", **dataset_kwargs)

    @classmethod
    def get_test(cls, **dataset_kwargs):
        return cls("test", **dataset_kwargs)

    def __len__(self) -> int:
        raise NotImplementedError

    def __getitem__(self, i):
        raise NotImplementedError


def parse_img_size(img_size, frame_hw):
    """(h, w) of a returned frame from `img_size`: None, an int or a two-element list / tuple (base_dataset.py:121-133)."""
    if img_size is None:
        return tuple(frame_hw)
    if isinstance(img_size, int) and not isinstance(img_size, bool):
        h, w = img_size, img_size
    elif isinstance(img_size, (list, tuple)) and len(img_size) == 2:
        h, w = img_size
    else:
        raise ValueError("invalid img size provided, expected either None, int or a two-element list/tuple")
    if not all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in (h, w)):
        raise ValueError(f"invalid img size provided: {img_size} (positive integers)")
    return h, w


def _pair(size, what):
    if isinstance(size, int) and not isinstance(size, bool):
        size = (size, size)
    size = tuple(size)
    if len(size) == 1:
        size = size * 2
    if len(size) != 2 or not all(isinstance(v, (int, np.integer)) and v >= 1 for v in size):
        raise ValueError(f"{what}: size must be one or two positive integers (got {size})")
    return int(size[0]), int(size[1])


def parse_crop(crop):
    """None, ("center", h, w), ("random", h, w) or ("box", y, x, h, w) from the `crop` argument: such a tuple, or an object whose type is
    named CenterCrop / RandomCrop and carries `.size` (torchvision's transforms, read by name: torchvision is never imported)."""
    if crop is None:
        return None
    kind = type(crop).__name__
    if kind in ("CenterCrop", "RandomCrop") and hasattr(crop, "size"):
        return ("center" if kind == "CenterCrop" else "random",) + _pair(crop.size, kind)
    if isinstance(crop, (tuple, list)) and crop and crop[0] in ("center", "random") and len(crop) == 3:
        return (crop[0],) + _pair(crop[1:], f"crop {crop[0]!r}")
    if isinstance(crop, (tuple, list)) and crop and crop[0] == "box" and len(crop) == 5:
        y, x = crop[1:3]
        if not all(isinstance(v, (int, np.integer)) and v >= 0 for v in (y, x)):
            raise ValueError(f"crop 'box': the corner must be two non-negative integers (got {(y, x)})")
        return ("box", int(y), int(x)) + _pair(crop[3:], "crop 'box'")
    raise ValueError(f"for the parameter 'crop', only ('center', h, w), ('random', h, w), ('box', y, x, h, w) and CenterCrop / RandomCrop "
                     f"objects are allowed (got {crop!r})")


_FLIPS = {"hflip": 1, "vflip": 2, "RandomHorizontalFlip": 1, "RandomVerticalFlip": 2}


def parse_augmentations(augmentations):
    """[(flip bit, p), ...] from a list of ("hflip", p) / ("vflip", p) or of objects named RandomHorizontalFlip / RandomVerticalFlip
    with `.p`. Every other entry of the reference's list of shape-preserving augmentations is not part of this build."""
    out = []
    for aug in augmentations or []:
        if isinstance(aug, (tuple, list)) and len(aug) == 2 and aug[0] in ("hflip", "vflip"):
            bit, p = _FLIPS[aug[0]], aug[1]
        elif type(aug).__name__ in ("RandomHorizontalFlip", "RandomVerticalFlip") and hasattr(aug, "p"):
            bit, p = _FLIPS[type(aug).__name__], aug.p
        else:
            raise NotImplementedError(f"augmentation {aug!r} is not part of this build: horizontal and vertical flips are")
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"augmentation {aug!r}: probability outside [0, 1]")
        out.append((bit, float(p)))
    return out


def is_flip(aug):
    """True for the entries parse_augmentations() takes: they stay in the preprocess launch."""
    return (isinstance(aug, (tuple, list)) and len(aug) > 0 and aug[0] in ("hflip", "vflip")) or type(aug).__name__ in ("RandomHorizontalFlip", "RandomVerticalFlip")


# opcodes of a program row (csrc/frames_aug.hip, include/vpx.h)
OP_INVERT, OP_SOLARIZE, OP_AUTOCONTRAST, OP_GRAY, OP_NORMALIZE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_ERASE = range(1, 11)
PROGRAM_ROW, PROGRAM_MIN_OPS, PROGRAM_MAX_OPS = 9, 16, 64

_BYTE_ONLY = {"RandomPosterize": "posterize", "RandomEqualize": "equalize"}
_OTHER_KERNEL = {"GaussianBlur": "blur", "RandomAdjustSharpness": "sharpness", "RandomRotation": "rotate"}
_P_ONLY = {"RandomInvert": "invert", "RandomAutocontrast": "autocontrast", "RandomGrayscale": "grayscale"}


def _probability(p, aug):
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"augmentation {aug!r}: probability outside [0, 1]")
    return float(p)


def _numbers(v, aug, what):
    """A tuple of floats from one number or a sequence of numbers."""
    seq = list(v) if isinstance(v, (tuple, list, np.ndarray)) else [v]
    if not seq or not all(isinstance(e, (int, float, np.integer, np.floating)) and not isinstance(e, bool) and math.isfinite(float(e)) for e in seq):
        raise ValueError(f"augmentation {aug!r}: {what} must be a number or a sequence of numbers")
    return tuple(float(e) for e in seq)


def _jitter_range(value, name, center, bound, aug, clip_first_on_zero=True):
    """torchvision's ColorJitter._check_input: None, or the (min, max) a factor is drawn from; None when that is (center, center)."""
    if value is None:
        return None
    if isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"augmentation {aug!r}: if {name} is a single number, it must be non negative")
        lo, hi = center - float(value), center + float(value)
        if clip_first_on_zero:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = _numbers(value, aug, name)
    else:
        raise ValueError(f"augmentation {aug!r}: {name} should be None, a single number or a (min, max) pair")
    if not bound[0] <= lo <= hi <= bound[1]:
        raise ValueError(f"augmentation {aug!r}: {name} values should be between {bound} and ordered (got {(lo, hi)}; negative factors and a hue outside [-0.5, 0.5] are refused)")
    return None if lo == hi == center else (lo, hi)


def parse_photometric(augmentations):
    """The colour and erasing entries of an `augmentations` list in canonical form, in their order:
    ("invert", p) | ("solarize", threshold, p) | ("autocontrast", p) | ("grayscale", p) | ("normalize", means, stds) |
    ("color_jitter", brightness, contrast, saturation, hue) with each None or the (min, max) its factor is drawn from |
    ("erase", p, (scale min, max), (ratio min, max), values). Accepts those tuples (color_jitter with torchvision's argument forms: None,
    a number x for [max(0, 1 - x), 1 + x] / [-x, x], or a pair) and objects named RandomInvert, RandomSolarize, RandomAutocontrast,
    RandomGrayscale, Grayscale, Normalize, ColorJitter, RandomErasing carrying torchvision's attributes (read by name: torchvision is
    never imported). What needs the frame shape is checked by check_photometric()."""
    out = []
    for aug in augmentations or []:
        kind = type(aug).__name__
        is_seq = isinstance(aug, (tuple, list)) and len(aug) > 0 and isinstance(aug[0], str)
        tag = aug[0] if is_seq else None
        if kind in _BYTE_ONLY or tag in _BYTE_ONLY.values():
            raise NotImplementedError(f"augmentation {aug!r} is not part of this build: torchvision's posterize and equalize accept byte tensors only, "
                                      f"and the reference's own chain raises on its float frames")
        if kind in _OTHER_KERNEL or tag in _OTHER_KERNEL.values():
            raise NotImplementedError(f"augmentation {aug!r} is not part of this build: blur, sharpness and rotation are neighbourhood and geometric "
                                      f"operations (a different kernel), not the element-wise ones the augment launch runs")
        if kind in _P_ONLY and hasattr(aug, "p"):
            out.append((_P_ONLY[kind], _probability(aug.p, aug)))
        elif is_seq and tag in _P_ONLY.values() and len(aug) == 2:
            out.append((tag, _probability(aug[1], aug)))
        elif kind == "Grayscale" and hasattr(aug, "num_output_channels"):
            if aug.num_output_channels != 3:
                raise NotImplementedError(f"augmentation {aug!r}: Grayscale(num_output_channels={aug.num_output_channels}) changes the frame shape; only 3 is part of this build")
            out.append(("grayscale", 1.0))
        elif (kind == "RandomSolarize" and hasattr(aug, "threshold") and hasattr(aug, "p")) or (is_seq and tag == "solarize" and len(aug) == 3):
            thr, p = (aug.threshold, aug.p) if not is_seq else aug[1:]
            out.append(("solarize", _numbers(thr, aug, "threshold")[0], _probability(p, aug)))
        elif (kind == "Normalize" and hasattr(aug, "mean") and hasattr(aug, "std")) or (is_seq and tag == "normalize" and len(aug) == 3):
            mean, std = (aug.mean, aug.std) if not is_seq else aug[1:]
            mean, std = _numbers(mean, aug, "mean"), _numbers(std, aug, "std")
            if any(np.float32(v) == 0 for v in std):
                raise ValueError(f"augmentation {aug!r}: a zero std (the division would give infinities)")
            out.append(("normalize", mean, std))
        elif (kind == "ColorJitter" and all(hasattr(aug, a) for a in ("brightness", "contrast", "saturation", "hue"))) or (is_seq and tag == "color_jitter" and len(aug) == 5):
            b, c, sat, hue = (aug.brightness, aug.contrast, aug.saturation, aug.hue) if not is_seq else aug[1:]
            inf = float("inf")
            out.append(("color_jitter", _jitter_range(b, "brightness", 1.0, (0.0, inf), aug), _jitter_range(c, "contrast", 1.0, (0.0, inf), aug),
                        _jitter_range(sat, "saturation", 1.0, (0.0, inf), aug), _jitter_range(hue, "hue", 0.0, (-0.5, 0.5), aug, clip_first_on_zero=False)))
        elif (kind == "RandomErasing" and all(hasattr(aug, a) for a in ("p", "scale", "ratio", "value"))) or (is_seq and tag == "erase" and len(aug) == 5):
            p, scale, ratio, value = (aug.p, aug.scale, aug.ratio, aug.value) if not is_seq else aug[1:]
            if value is None or isinstance(value, str):
                raise NotImplementedError(f"augmentation {aug!r}: erasing with value='random' (noise from torch's generator) is not part of this build; give a number or one per channel")
            scale, ratio = _numbers(scale, aug, "scale"), _numbers(ratio, aug, "ratio")
            if len(scale) != 2 or len(ratio) != 2 or not 0.0 <= scale[0] <= scale[1] <= 1.0 or not 0.0 < ratio[0] <= ratio[1]:
                raise ValueError(f"augmentation {aug!r}: scale must be an ordered pair in [0, 1] and ratio an ordered pair of positive numbers")
            out.append(("erase", _probability(p, aug), scale, ratio, _numbers(value, aug, "value")))
        else:
            raise NotImplementedError(f"augmentation {aug!r} is not part of this build: flips, invert, solarize, autocontrast, grayscale, normalize, "
                                      f"color_jitter and erase are")
    return out


def check_photometric(photometric, channels):
    """The refusals of parse_photometric()'s result that need the channel count of a returned frame."""
    for entry in photometric:
        kind = entry[0]
        if kind == "grayscale" and channels != 3:
            raise ValueError(f"augmentation {entry!r}: grayscale needs 3-channel frames (got {channels}; on one channel there is nothing to do, "
                             f"and torchvision refuses it)")
        if kind == "color_jitter" and channels not in (1, 3) and any(r is not None for r in entry[2:]):
            raise ValueError(f"augmentation {entry!r}: contrast, saturation and hue need 1 or 3 channels (got {channels})")
        for what, values in (("mean", entry[1]), ("std", entry[2])) if kind == "normalize" else ((("value", entry[4]),) if kind == "erase" else ()):
            if len(values) not in (1, channels):
                raise ValueError(f"augmentation {entry!r}: {len(values)} {what} entries for {channels} channels (one, or one per channel)")


def _row(op, *params):
    return (float(op),) + tuple(float(np.float32(p)) for p in params) + (0.0,) * (PROGRAM_ROW - 1 - len(params))


def _per_channel(values, channels, fill):
    values = tuple(values) * channels if len(values) == 1 else tuple(values)
    return values + (fill,) * (4 - len(values))


def draw_erase_box(rng, frame_hw, scale, ratio):
    """torchvision's RandomErasing.get_params: (y0, x0, rows, columns), or None after ten attempts that did not fit."""
    H, W = frame_hw
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        erase_area = area * float(rng.uniform(scale[0], scale[1]))
        aspect = math.exp(float(rng.uniform(log_ratio[0], log_ratio[1])))
        eh = int(round(math.sqrt(erase_area * aspect)))
        ew = int(round(math.sqrt(erase_area / aspect)))
        if not (eh < H and ew < W):
            continue
        y0 = int(rng.integers(0, H - eh + 1))
        x0 = int(rng.integers(0, W - ew + 1))
        return y0, x0, eh, ew
    return None


def pack_programs(programs):
    """float32 [n, max_ops, PROGRAM_ROW] from per-sample lists of rows: max_ops = the longest program, at least PROGRAM_MIN_OPS; opcode 0 ends one."""
    longest = max(len(rows) for rows in programs)
    if longest > PROGRAM_MAX_OPS:
        raise ValueError(f"an augmentation program of {longest} operations exceeds the launch's {PROGRAM_MAX_OPS}")
    out = np.zeros((len(programs), max(longest, PROGRAM_MIN_OPS), PROGRAM_ROW), dtype=np.float32)
    for k, rows in enumerate(programs):
        if rows:
            out[k, :len(rows)] = np.array(rows, dtype=np.float32)
    return out


def center_offset(full, size):
    """torchvision's CenterCrop offset: int(round((full - size) / 2.0)) with Python's round (half to even)."""
    return int(round((full - size) / 2.0))


class _IndexLoader:
    """Batches of a stored dataset in index order, or in an order shuffled anew by one seeded generator at every pass."""

    def __init__(self, dataset, batch_size, shuffle, drop_last, seed):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        full, rest = divmod(len(dataset), batch_size)
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle
        self.sizes = [batch_size] * full + ([rest] if rest and not drop_last else [])
        self.rng = random.Random(seed)

    def __len__(self):
        return len(self.sizes)

    def __iter__(self):
        order = list(range(len(self.dataset)))
        if self.shuffle:
            self.rng.shuffle(order)
        start = 0
        for n in self.sizes:
            yield self.dataset.batch(order[start:start + n])
            start += n


class _PinnedStage:
    """A pinned staging buffer: a batch's rows (their first `steps` entries along T') are gathered into it and copied to the GPU once.
    It is reused while it fits; the event tells when the previous batch's copy has left it."""

    def __init__(self):
        self.buffer = self.event = None

    def to_device(self, raw, indices, steps, device):
        return self._stage([raw[i, :steps] for i in indices], device)

    def spans_to_device(self, flat, firsts, steps, device):
        """The same for long clips stored back to back, flat [frames, ...]: row k of the staged block is flat[firsts[k]:firsts[k] + steps]."""
        return self._stage([flat[f:f + steps] for f in firsts], device)

    def _stage(self, pieces, device):
        n, steps = len(pieces), pieces[0].shape[0]
        if self.buffer is None or self.buffer.shape[0] < n or self.buffer.shape[1] != steps:
            self.buffer = torch.empty((n,) + tuple(pieces[0].shape), dtype=pieces[0].dtype).pin_memory()
        elif self.event is not None:
            self.event.synchronize()                              # the previous batch's copy has left the buffer
        for k, piece in enumerate(pieces):
            self.buffer[k].copy_(piece)
        dev = self.buffer[:n].to(device, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return dev


class StoredSubset:
    """Some samples of a stored dataset (the reference's VPSubset): forwards every other attribute to the dataset, keeps batch() / loader()."""

    def __init__(self, dataset, indices):
        self.dataset, self.indices = dataset, list(indices)

    def __getattr__(self, item):
        return getattr(self.__dict__["dataset"], item)

    def __len__(self):
        return len(self.indices)

    def batch(self, indices):
        return self.dataset.batch([self.indices[i] for i in indices])

    def __getitem__(self, i):
        return self.dataset[self.indices[i]]

    def loader(self, batch_size, shuffle=False, drop_last=True, seed=None):
        return _IndexLoader(self, batch_size, shuffle, drop_last, seed)


class StoredVPDataset(VPDataset):
    """Sequences stored as one raw tensor [N, T', H, W(, C)] of uint8, uint16 or float32 (float32 is taken as already in [0, 1]).

    storage="device": the tensor lives on the GPU and a batch is one launch over it. storage="pinned": it lives in pinned host memory; a
    batch's rows (their first seq_len frames) are gathered into a pinned staging buffer, copied once, then one launch.
    img_size: None, an int or a pair (base_dataset.py:121-133); as in the reference a resize takes place when it differs from the stored
    frame size, and then follows the crop. `img_shape` is the shape a returned frame really has (the reference reports the stored size
    even when a crop without resize returns less). The resize is bilinear with align_corners=False and NO antialiasing: what the
    reference's pinned torchvision does to tensors; newer torchvision antialiases by default.
    crop: ("center", h, w) | ("random", h, w) | ("box", y, x, h, w), or a CenterCrop / RandomCrop object. augmentations: a list of
    ("hflip", p) | ("vflip", p) and the colour and erasing entries parse_photometric() lists — ("invert", p), ("solarize", threshold, p),
    ("autocontrast", p), ("grayscale", p), ("normalize", mean, std), ("color_jitter", brightness, contrast, saturation, hue),
    ("erase", p, scale, ratio, value) — or the torchvision objects of those names. Random boxes, flips and every photometric parameter
    are drawn ONCE per sequence (the reference transforms the whole [t, c, h, w] tensor at once) from a host generator seeded with
    transform_seed: per sequence box row, box column, flips, then the photometric entries in list order (one random() per probability;
    colour jitter a permutation of its four adjustments, then one uniform per configured one; erasing torchvision's ten attempts).
    Operations act after scale, crop, resize and flips, in list order; an erasing rectangle is mirrored through the flips that follow it
    in the list and were drawn, so the result is the list applied in order. The flips land in `augmentations`, the rest in `photometric`.
    The clamps of colour jitter and autocontrast are to [0, 1] literally, also under a value range such as (-1, 1): the reference
    scales before it transforms and torchvision clamps float tensors to [0, 1], so it behaves the same way. A channel that is constant
    over a frame is left unchanged by autocontrast.
    actions: None, or the stored actions [N, T', A] as numpy float32 / float64 with the leading two sizes of `raw`. They live where
    `storage` keeps the frames (on the GPU, or pinned and staged per batch like the frames); ACTION_SIZE becomes A, `config` gains
    supports_actions = True, and batch() / __getitem__ return actions[i, :seq_len:seq_step] as float32 (float64 rounded to nearest even,
    what torch's .float() and numpy's astype do) from one further launch instead of zeros. Crops, flips and photometric entries never
    touch them (the reference's do not either). Without `actions` nothing changes: the same zeros, launches and draws."""
    NAME = "Stored sequences"
    ACTION_SIZE = 0
    SUPPORTS_TRANSFORMS = True
    OUT_CHANNELS = None   # channels of a returned frame: None = the stored ones; 3 with gray storage repeats the channel

    train_to_val_ratio: float = 0.8
    train_val_seed = 1234
    storage = "device"
    transform_seed = 0
    device = "cuda"
    img_size = None
    crop = None
    augmentations = None   # the flips [(bit, p)]
    photometric = None     # every other entry, parse_photometric()'s form

    def __init__(self, split, raw=None, actions=None, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["transform_rng"]
        self.storage = dataset_kwargs.get("storage", self.storage)
        if self.storage not in ("device", "pinned"):
            raise ValueError(f"storage '{self.storage}' has to be one of the following: ['device', 'pinned']")
        self.device = dataset_kwargs.get("device", self.device)
        set_from_kwarg(self, dataset_kwargs, "transform_seed")
        if self.value_range_max == self.value_range_min:
            raise ValueError(f"empty value range [{self.value_range_min}, {self.value_range_max}]")
        self.img_size = dataset_kwargs.get("img_size", None)
        parse_img_size(self.img_size, (1, 1))                     # (refused now; the size itself needs the stored frame shape)
        self.crop = parse_crop(dataset_kwargs.get("crop", None))
        given = list(dataset_kwargs.get("augmentations", None) or [])
        self.augmentations = parse_augmentations([aug for aug in given if is_flip(aug)])
        self.photometric = parse_photometric([aug for aug in given if not is_flip(aug)])
        flips_before = np.cumsum([is_flip(aug) for aug in given]).tolist()
        self._flips_before = [n for n, aug in zip(flips_before, given) if not is_flip(aug)]   # per photometric entry: flips ahead of it in the list
        self._raw = self._raw_host = self._actions = self._actions_host = None
        self._staging, self._actions_staging = _PinnedStage(), _PinnedStage()
        self.reset_rng()
        if raw is not None:
            self._set_raw(raw)
        if actions is not None:
            self._set_actions(actions)

    # ---- storage ----
    def _set_raw(self, raw):
        """Takes the raw sequences [N, T', H, W(, C)] (numpy or torch, on the host) and fixes everything that depends on their shape."""
        raw = raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
        if raw.dtype not in (np.uint8, np.uint16, np.float32):
            raise ValueError(f"stored sequences must be uint8, uint16 or float32 (got {raw.dtype})")
        if raw.ndim not in (4, 5) or min(raw.shape) < 1:
            raise ValueError(f"stored sequences must be [N, T', H, W] or [N, T', H, W, C], nothing empty (got {raw.shape})")
        self._raw_host = np.ascontiguousarray(raw)
        N, Tp, H, W = raw.shape[:4]
        self.MIN_SEQ_LEN = int(Tp)
        self._set_frame_geometry(H, W, raw.shape[4] if raw.ndim == 5 else 1)

    def _set_frame_geometry(self, H, W, Cs):
        """Everything that depends on the stored frame shape [H, W, Cs]: the returned channels, the crop box and the returned size."""
        c_out = self.OUT_CHANNELS or Cs
        if c_out != Cs and not (Cs == 1 and c_out == 3):
            raise ValueError(f"{c_out} channels cannot be returned from {Cs} stored ones (equal, or 3 from 1)")
        self.DATASET_FRAME_SHAPE = (int(H), int(W), int(c_out))
        self._crop_hw = (H, W) if self.crop is None else tuple(self.crop[-2:])
        if self._crop_hw[0] > H or self._crop_hw[1] > W:
            raise ValueError(f"the {self._crop_hw[0]}x{self._crop_hw[1]} crop does not fit the {H}x{W} frames (there is no padding)")
        if self.crop is not None and self.crop[0] == "box" and (self.crop[1] + self._crop_hw[0] > H or self.crop[2] + self._crop_hw[1] > W):
            raise ValueError(f"the crop box {self.crop[1:]} leaves the {H}x{W} frames (there is no padding)")
        want = parse_img_size(self.img_size, (H, W))
        self._out_hw = tuple(int(v) for v in (want if want != (H, W) else self._crop_hw))   # the reference appends Resize only then
        self.img_shape = (int(c_out),) + self._out_hw
        check_photometric(self.photometric, int(c_out))

    def _set_actions(self, actions):
        """Takes the stored actions [N, T', A] (numpy float32 / float64, or such a torch tensor on the host) of the sequences set before."""
        if self._raw_host is None:
            raise ValueError("actions need the sequences they belong to: give raw= as well")
        actions = actions.detach().cpu().numpy() if torch.is_tensor(actions) else np.asarray(actions)
        if actions.dtype not in (np.float32, np.float64):
            raise ValueError(f"stored actions must be float32 or float64 (got {actions.dtype})")
        if actions.ndim != 3 or actions.shape[2] < 1 or tuple(actions.shape[:2]) != tuple(self._raw_host.shape[:2]):
            raise ValueError(f"stored actions must be [N, T', A] with the sequences' N = {self._raw_host.shape[0]} and T' = {self._raw_host.shape[1]} "
                             f"(got {actions.shape})")
        self._actions_host = np.ascontiguousarray(actions)
        self.ACTION_SIZE = int(actions.shape[2])

    def _place(self, host):
        t = torch.from_numpy(host)
        return t.to(self.device) if self.storage == "device" else t.pin_memory()

    def _stored(self):
        """The raw tensor where the storage mode keeps it (made at the first use: building a dataset needs no GPU)."""
        if self._raw is None:
            if self._raw_host is None:
                raise VpxError(f"'{self.NAME}' holds no sequences")
            self._raw = self._place(self._raw_host)
        return self._raw

    def _stored_actions(self):
        if self._actions is None:
            self._actions = self._place(self._actions_host)
        return self._actions

    def _on_device(self, indices):
        """(raw tensor on the GPU, sequence index of every sample in it)."""
        raw = self._stored()
        if self.storage == "device":
            return raw, list(indices)
        dev = self._staging.to_device(raw, indices, min(self.seq_len, raw.shape[1]), self.device)
        return dev, list(range(len(indices)))

    def _actions_on_device(self, indices):
        """The stored actions on the GPU, laid out as _on_device() lays out the frames: the table of the frames launch indexes both."""
        raw = self._stored_actions()
        if self.storage == "device":
            return raw
        return self._actions_staging.to_device(raw, indices, min(self.seq_len, raw.shape[1]), self.device)

    # ---- transforms ----
    def reset_rng(self):
        self.transform_rng = np.random.default_rng(self.transform_seed)

    def _draw_geometry(self, frame_hw, crop, transform=True):
        """(crop y0, crop x0, flip bits, the flips' draws) of one sequence; random boxes and flips advance the host generator, box rows first."""
        H, W = frame_hw
        if not transform or crop is None:
            y0 = x0 = 0
        elif crop[0] == "center":
            y0, x0 = center_offset(H, crop[1]), center_offset(W, crop[2])
        elif crop[0] == "random":
            y0 = int(self.transform_rng.integers(0, H - crop[1] + 1))
            x0 = int(self.transform_rng.integers(0, W - crop[2] + 1))
        else:
            y0, x0 = crop[1], crop[2]
        bits, drawn = 0, []
        for bit, p in (self.augmentations if transform else []):
            drawn.append(bool(self.transform_rng.random() < p))
            if drawn[-1]:
                bits ^= bit
        return y0, x0, bits, drawn

    def _draw_transform(self, frame_hw, crop, transform=True):
        """(crop y0, crop x0, flip bits) of one sequence."""
        return self._draw_geometry(frame_hw, crop, transform)[:3]

    def _draw_program(self, out_chw, flips_drawn, transform=True):
        """The photometric program of one sequence, rows (opcode, 8 parameters) in the order they act; an operation that was not drawn
        is absent. Advances the host generator after the sequence's box and flip draws, in list order."""
        rows = []
        if not transform:
            return rows
        C, h, w = out_chw
        rng = self.transform_rng
        for entry, n_before in zip(self.photometric, self._flips_before):
            kind = entry[0]
            if kind in ("invert", "autocontrast", "grayscale", "solarize"):
                if rng.random() < entry[-1]:
                    rows.append(_row({"invert": OP_INVERT, "autocontrast": OP_AUTOCONTRAST, "grayscale": OP_GRAY, "solarize": OP_SOLARIZE}[kind],
                                     *((entry[1],) if kind == "solarize" else ())))
            elif kind == "normalize":
                rows.append(_row(OP_NORMALIZE, *_per_channel(entry[1], C, 0.0), *_per_channel(entry[2], C, 1.0)))
            elif kind == "color_jitter":
                order = [int(i) for i in rng.permutation(4)]
                factors = [None if r is None else float(rng.uniform(r[0], r[1])) for r in entry[1:]]
                for i in order:
                    if factors[i] is None:
                        continue
                    if i == 3:
                        rows.append(_row(OP_HUE, factors[i]))
                    else:                                             # f and 1 - f, formed in double, each rounded to float32 once
                        rows.append(_row((OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION)[i], factors[i], 1.0 - factors[i]))
            else:                                                     # erase
                if rng.random() < entry[1]:
                    box = draw_erase_box(rng, (h, w), entry[2], entry[3])
                    if box is not None:
                        y0, x0, eh, ew = box
                        for (bit, _), on in list(zip(self.augmentations, flips_drawn))[n_before:]:   # the flips that follow it mirror the box
                            if on and bit == 1:
                                x0 = w - x0 - ew
                            elif on:
                                y0 = h - y0 - eh
                        rows.append(_row(OP_ERASE, y0, x0, eh, ew, *_per_channel(entry[4], C, 0.0)))
        return rows

    def draws(self, seqs, transform=True, frame_hw=None, crop="own", out_chw=None):
        """(int32 [n, 4] rows (sequence index, crop y0, crop x0, flip bits), the n photometric programs) for the launches: one draw per
        sequence, its box and flips first, its photometric parameters after them."""
        frame_hw = tuple(self._raw_host.shape[2:4]) if frame_hw is None else frame_hw
        crop = self.crop if isinstance(crop, str) else crop
        out_chw = tuple(self.img_shape) if out_chw is None else out_chw
        rows, programs = [], []
        for s in seqs:
            y0, x0, bits, drawn = self._draw_geometry(frame_hw, crop, transform)
            rows.append((s, y0, x0, bits))
            programs.append(self._draw_program(out_chw, drawn, transform))
        return np.array(rows, dtype=np.int32).reshape(len(seqs), 4), programs

    def table(self, seqs, transform=True):
        """int32 [n, 4] rows (sequence index, crop y0, crop x0, flip bits) for the launch: one draw per sequence (draws() without its programs)."""
        return self.draws(seqs, transform)[0]

    def _augment(self, frames, programs):
        """The second launch, on the same stream and without a host sync; none when every program is empty."""
        if any(programs):
            ops.frames_augment(frames, pack_programs(programs))
        return frames

    def preprocess(self, x, transform=True):
        """The reference's preprocess() for one tensor [..., h, w(, c)] (2-D: one gray image), from one launch: float32 [..., c, h', w'] on
        the GPU, scaled to the value range, then (transform=True) cropped, resized, flipped and run through the photometric entries with
        ONE draw for the whole tensor. dtype
        rules as the reference's where the kernel has the element type: numpy uint8 / uint16 and torch uint8 are divided by their
        maximum; torch float32 passes through and torch double is converted to it (the reference's message names torch.float, its
        code refuses it); everything else raises its ValueError."""
        if isinstance(x, np.ndarray):
            if x.dtype not in (np.uint8, np.uint16):
                raise ValueError(f"if providing numpy arrays, only dtypes np.uint8 and np.uint16 are supported by this build (given: {x.dtype})")
            x = torch.from_numpy(np.ascontiguousarray(x))
        elif torch.is_tensor(x):
            if x.dtype == torch.double:
                x = x.float()
            elif x.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"if providing pytorch tensors, only dtypes torch.uint8, torch.float and torch.double are supported (given: {x.dtype})")
        else:
            raise ValueError("expected input to be either a numpy array or a PyTorch tensor")
        if x.ndim < 2:
            raise ValueError("expected at least two dimensions for input image")
        if x.ndim == 2:
            x = x[:, :, None]                                      # one gray image: [h, w] -> [1, h', w']
        lead = tuple(x.shape[:-3])
        H, W, C = (int(s) for s in x.shape[-3:])
        T = int(np.prod(lead)) if lead else 1
        crop = self.crop if transform else None
        ch, cw = (H, W) if crop is None else crop[-2:]
        if ch > H or cw > W or (crop is not None and crop[0] == "box" and (crop[1] + ch > H or crop[2] + cw > W)):
            raise ValueError(f"the crop {crop} does not fit the {H}x{W} frames (there is no padding)")
        want = parse_img_size(self.img_size, (H, W))
        oh, ow = want if (transform and want != tuple(self.DATASET_FRAME_SHAPE[:2])) else (ch, cw)
        if transform:
            check_photometric(self.photometric, C)
        row, programs = self.draws([0], transform, (H, W), crop, (C, oh, ow))
        out = ops.frames_preprocess(x.reshape(1, T, H, W, C).to(self.device), row, T, 1, (ch, cw), (oh, ow), C,
                                    (self.value_range_min, self.value_range_max))
        return self._augment(out, programs).reshape(lead + (C, oh, ow))

    def postprocess(self, x):
        """uint8 numpy [..., h, w, c] in [0, 255] from a tensor [..., c, h, w] in (about) the value range (base_dataset.py:275-298), one
        launch; unlike the reference's in-place arithmetic it leaves `x` as it is."""
        if x.ndim < 3:
            raise ValueError("expected at least three dimensions for input image")
        if not x.is_cuda:
            x = x.to(self.device)
        return ops.frames_postprocess(x.float(), self.value_range_min, self.value_range_max).cpu().numpy()

    # ---- samples ----
    def __len__(self):
        return 0 if self._raw_host is None else int(self._raw_host.shape[0])

    def origin(self, i):
        return f"stored sequence {i}"

    @property
    def config(self) -> dict:
        cfg = super().config
        if self._actions_host is not None:
            cfg["supports_actions"] = True                        # (no dataset of the reference sets the key: see the module docstring)
        return cfg

    def batch(self, indices):
        """The reference's dict for these samples from ONE launch (two when a photometric program was drawn): frames [n, total_frames, C, h, w] on the GPU, actions zeros
        [n, total_frames, max(ACTION_SIZE, 1)], origin. Equal to the __getitem__ calls in the same order. With stored actions: one more
        launch, directly after the frames launch and from its table, gathers them as float32 [n, total_frames, ACTION_SIZE]."""
        if not self.ready_for_usage:
            raise RuntimeError("Dataset is not yet ready for usage (maybe you forgot to call set_seq_len()).")
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("batch(indices) needs at least one index")
        if min(indices) < 0 or max(indices) >= len(self):
            raise IndexError(f"sample index outside [0, {len(self)})")
        raw, seqs = self._on_device(indices)
        table, programs = self.draws(seqs)
        frames = ops.frames_preprocess(raw, table, self.total_frames, self.seq_step, self._crop_hw, self._out_hw, self.img_shape[0],
                                       (self.value_range_min, self.value_range_max))
        if self._actions_host is not None:                        # directly after the frames launch, from its table
            actions = ops.actions_gather(self._actions_on_device(indices), table, self.total_frames, self.seq_step)
        self._augment(frames, programs)
        if self._actions_host is None:
            actions = torch.zeros((len(indices), self.total_frames, max(self.ACTION_SIZE, 1)), device=frames.device)
        return {"frames": frames, "actions": actions, "origin": [self.origin(i) for i in indices]}

    def __getitem__(self, i):
        data = self.batch([i])
        return {"frames": data["frames"][0], "actions": data["actions"][0], "origin": data["origin"][0]}

    def loader(self, batch_size, shuffle=False, drop_last=True, seed=None):
        """An iterable of batches: what VPModel.train_iter / eval_iter take as `loader`."""
        return _IndexLoader(self, batch_size, shuffle, drop_last, seed)

    @classmethod
    def get_train_val(cls, **dataset_kwargs):
        """(training, validation) halves of the "train" split, the reference's way (base_dataset.py:333-400): indices shuffled by
        random.Random(train_val_seed), the first int(len * train_to_val_ratio) are training samples."""
        if cls.VALID_SPLITS == ["train", "val", "test"]:
            return cls("train", **dataset_kwargs), cls("val", **dataset_kwargs)
        assert cls.VALID_SPLITS == ["train", "test"], f"parameter 'VALID_SPLITS' of dataset class '{cls.__name__}' is ill-configured"
        main = cls("train", **dataset_kwargs)
        n_train = int(len(main) * cls.train_to_val_ratio)
        indices = list(range(len(main)))
        random.Random(cls.train_val_seed).shuffle(indices)
        return StoredSubset(main, indices[:n_train]), StoredSubset(main, indices[n_train:])

    @classmethod
    def get_test(cls, **dataset_kwargs):
        return cls("test", **dataset_kwargs)
