"""Dataset base classes with the reference's surface (vp_suite/base/base_dataset.py).

VPDataset: split handling, set_seq_len() and its sequence-length rule, the value range, `config`. A dataset that is generated on the GPU
produces its frames at their final size and value range in the generating kernel, so it has no preprocess() chain and refuses `crop` and
`augmentations` (SUPPORTS_TRANSFORMS = False).

StoredVPDataset: sequences held as ONE raw tensor [N, T', H, W(, C)] — on the GPU, or in pinned host memory — and the reference's
preprocess() / postprocess() chain (convert, permute, scale, crop, resize, flip) as one launch of csrc/frames.hip per batch and
direction. No ATen op touches a pixel between the stored bytes and the batch a model reads."""
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
    ("hflip", p) | ("vflip", p), or RandomHorizontalFlip / RandomVerticalFlip objects. Random boxes and flips are drawn ONCE per sequence
    (the reference transforms the whole [t, c, h, w] tensor at once) from a host generator seeded with transform_seed."""
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
    augmentations = None

    def __init__(self, split, raw=None, **dataset_kwargs):
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
        self.augmentations = parse_augmentations(dataset_kwargs.get("augmentations", []))
        self._raw = self._raw_host = self._staging = self._staging_event = None
        self.reset_rng()
        if raw is not None:
            self._set_raw(raw)

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
        Cs = raw.shape[4] if raw.ndim == 5 else 1
        c_out = self.OUT_CHANNELS or Cs
        if c_out != Cs and not (Cs == 1 and c_out == 3):
            raise ValueError(f"{c_out} channels cannot be returned from {Cs} stored ones (equal, or 3 from 1)")
        self.MIN_SEQ_LEN = int(Tp)
        self.DATASET_FRAME_SHAPE = (int(H), int(W), int(c_out))
        self._crop_hw = (H, W) if self.crop is None else tuple(self.crop[-2:])
        if self._crop_hw[0] > H or self._crop_hw[1] > W:
            raise ValueError(f"the {self._crop_hw[0]}x{self._crop_hw[1]} crop does not fit the {H}x{W} frames (there is no padding)")
        if self.crop is not None and self.crop[0] == "box" and (self.crop[1] + self._crop_hw[0] > H or self.crop[2] + self._crop_hw[1] > W):
            raise ValueError(f"the crop box {self.crop[1:]} leaves the {H}x{W} frames (there is no padding)")
        want = parse_img_size(self.img_size, (H, W))
        self._out_hw = tuple(int(v) for v in (want if want != (H, W) else self._crop_hw))   # the reference appends Resize only then
        self.img_shape = (int(c_out),) + self._out_hw

    def _stored(self):
        """The raw tensor where the storage mode keeps it (made at the first use: building a dataset needs no GPU)."""
        if self._raw is None:
            if self._raw_host is None:
                raise VpxError(f"'{self.NAME}' holds no sequences")
            t = torch.from_numpy(self._raw_host)
            self._raw = t.to(self.device) if self.storage == "device" else t.pin_memory()
        return self._raw

    def _on_device(self, indices):
        """(raw tensor on the GPU, sequence index of every sample in it)."""
        raw = self._stored()
        if self.storage == "device":
            return raw, list(indices)
        n, frames = len(indices), min(self.seq_len, raw.shape[1])
        if self._staging is None or self._staging.shape[0] < n or self._staging.shape[1] != frames:
            self._staging = torch.empty((n, frames) + tuple(raw.shape[2:]), dtype=raw.dtype).pin_memory()
        elif self._staging_event is not None:
            self._staging_event.synchronize()                     # the previous batch's copy has left the buffer
        for k, i in enumerate(indices):
            self._staging[k].copy_(raw[i, :frames])
        dev = self._staging[:n].to(self.device, non_blocking=True)
        self._staging_event = torch.cuda.Event()
        self._staging_event.record()
        return dev, list(range(n))

    # ---- transforms ----
    def reset_rng(self):
        self.transform_rng = np.random.default_rng(self.transform_seed)

    def _draw_transform(self, frame_hw, crop, transform=True):
        """(crop y0, crop x0, flip bits) of one sequence; random boxes and flips advance the host generator, box rows first."""
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
        bits = 0
        for bit, p in (self.augmentations if transform else []):
            if self.transform_rng.random() < p:
                bits ^= bit
        return y0, x0, bits

    def table(self, seqs, transform=True):
        """int32 [n, 4] rows (sequence index, crop y0, crop x0, flip bits) for the launch: one draw per sequence."""
        H, W = self._raw_host.shape[2:4]
        return np.array([(s,) + self._draw_transform((H, W), self.crop, transform) for s in seqs], dtype=np.int32).reshape(len(seqs), 4)

    def preprocess(self, x, transform=True):
        """The reference's preprocess() for one tensor [..., h, w(, c)] (2-D: one gray image), from one launch: float32 [..., c, h', w'] on
        the GPU, scaled to the value range, then (transform=True) cropped, resized and flipped with ONE draw for the whole tensor. dtype
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
        row = np.array([(0,) + self._draw_transform((H, W), crop, transform)], dtype=np.int32)
        out = ops.frames_preprocess(x.reshape(1, T, H, W, C).to(self.device), row, T, 1, (ch, cw), (oh, ow), C,
                                    (self.value_range_min, self.value_range_max))
        return out.reshape(lead + (C, oh, ow))

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

    def batch(self, indices):
        """The reference's dict for these samples from ONE launch: frames [n, total_frames, C, h, w] on the GPU, actions zeros
        [n, total_frames, max(ACTION_SIZE, 1)], origin. Equal to the __getitem__ calls in the same order."""
        if not self.ready_for_usage:
            raise RuntimeError("Dataset is not yet ready for usage (maybe you forgot to call set_seq_len()).")
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("batch(indices) needs at least one index")
        if min(indices) < 0 or max(indices) >= len(self):
            raise IndexError(f"sample index outside [0, {len(self)})")
        raw, seqs = self._on_device(indices)
        frames = ops.frames_preprocess(raw, self.table(seqs), self.total_frames, self.seq_step, self._crop_hw, self._out_hw, self.img_shape[0],
                                       (self.value_range_min, self.value_range_max))
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
