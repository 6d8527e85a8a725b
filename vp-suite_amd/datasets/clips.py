"""Long clips of different lengths, each yielding many windows: the storage model of the reference's KITTI raw, Caltech Pedestrian, KTH,
Penn Action, Human 3.6M and SynPick classes (vp_suite/datasets/kitti_raw.py:77-95, caltech_pedestrian.py:69-86).

ClipVPDataset: the clips of a split are held back to back as ONE raw buffer [frames, H, W(, C)] — on the GPU, or in pinned host memory —
with the first frame of every clip beside it. set_seq_len() lists the windows by the reference's rule,
    for every clip: start in range(0, frame_count - seq_len + 1, seq_len + seq_step - 1),
and sample i is window i: frames start, start + seq_step, ... of its clip through ONE launch of vpx_clips_preprocess per batch
(csrc/frames.hip: the per-pixel code of the stored-sequence launch behind a 64-bit frame offset looked up per sample). Crops, flips,
photometric programs, preprocess() / postprocess(), loader() and `config` are StoredVPDataset's; the draws are per window.

WHAT DIFFERS FROM THE REFERENCE: set_seq_len() builds the window list anew (the reference appends to the list of an earlier call); a
configuration that yields no window at all raises ValueError (the reference returns an empty dataset)."""
import numpy as np
import torch

from .. import ops
from .._lib import VpxError
from .base import StoredVPDataset


def window_starts(frame_count, seq_len, seq_step):
    """The start frames of a clip's windows (kitti_raw.py:80-81): none when the clip is shorter than seq_len."""
    return range(0, frame_count - seq_len + 1, seq_len + seq_step - 1)


class ClipVPDataset(StoredVPDataset):
    """clips: a list of arrays [T_i, H, W(, C)] of one dtype (uint8, uint16 or float32) and one frame shape; the lengths T_i may differ.
    Memory-mapped arrays are read once, when the buffer is first placed. storage="device": the buffer lives on the GPU and a batch is one
    launch over it. storage="pinned": it lives in pinned host memory and only the seq_len frames of each window of a batch are gathered
    into a pinned staging block and copied; the launch then runs over that block, its offsets and table relative to it.
    `actions` is a [t, 1] zero tensor per sample, as in the reference; there are no stored actions."""
    NAME = "Stored clips"

    def __init__(self, split, clips=None, **dataset_kwargs):
        if dataset_kwargs.get("raw") is not None or dataset_kwargs.get("actions") is not None:
            raise ValueError("a clip dataset takes clips=[...]; raw= and actions= belong to StoredVPDataset")
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["clip_lengths", "clip_first", "windows"]
        self._clips_host = None
        self.clip_lengths, self.clip_first, self.windows = [], np.zeros(1, dtype=np.int64), []
        if clips is not None:
            self._set_clips(clips)

    # ---- storage ----
    def _set_clips(self, clips):
        """Takes the clips [T_i, H, W(, C)] (numpy, memory-mapped or not) and fixes everything that depends on their shape."""
        clips = [c.detach().cpu().numpy() if torch.is_tensor(c) else np.asanyarray(c) for c in clips]
        if not clips:
            raise ValueError("a clip dataset needs at least one clip")
        first = clips[0]
        if first.dtype not in (np.uint8, np.uint16, np.float32):
            raise ValueError(f"stored clips must be uint8, uint16 or float32 (got {first.dtype})")
        if first.ndim not in (3, 4) or min(first.shape) < 1:
            raise ValueError(f"a stored clip must be [T, H, W] or [T, H, W, C], nothing empty (got {first.shape})")
        for k, c in enumerate(clips):
            if c.dtype != first.dtype or c.shape[1:] != first.shape[1:] or c.ndim != first.ndim or c.shape[0] < 1:
                raise ValueError(f"clip {k}: {c.dtype} {c.shape} differs from the first clip's element type or frame shape ({first.dtype} {first.shape[1:]})")
        self._clips_host = clips
        self.clip_lengths = [int(c.shape[0]) for c in clips]
        self.clip_first = np.concatenate([[0], np.cumsum(self.clip_lengths)]).astype(np.int64)
        if type(self).MIN_SEQ_LEN is NotImplemented:
            self.MIN_SEQ_LEN = max(self.clip_lengths)                 # a window fits the longest clip at the most
        self._frame_hw = (int(first.shape[1]), int(first.shape[2]))
        self._set_frame_geometry(self._frame_hw[0], self._frame_hw[1], int(first.shape[3]) if first.ndim == 4 else 1)

    def _set_raw(self, raw):
        raise ValueError("a clip dataset takes clips=[...], not raw=")

    def _set_actions(self, actions):
        raise ValueError("a clip dataset stores no actions")

    def _stored(self):
        """The buffer [frames, H, W(, C)] where the storage mode keeps it (made at the first use: building a dataset needs no GPU)."""
        if self._raw is None:
            if self._clips_host is None:
                raise VpxError(f"'{self.NAME}' holds no clips")
            dtype = torch.from_numpy(np.empty(0, dtype=self._clips_host[0].dtype)).dtype
            flat = torch.empty((int(self.clip_first[-1]),) + tuple(self._clips_host[0].shape[1:]), dtype=dtype)
            if self.storage == "pinned":
                flat = flat.pin_memory()
            for first, clip in zip(self.clip_first[:-1].tolist(), self._clips_host):
                flat[first:first + clip.shape[0]].copy_(torch.from_numpy(np.array(clip)))   # (a copy: a memory-mapped file is read here, once)
            self._raw = flat.to(self.device) if self.storage == "device" else flat
        return self._raw

    # ---- windows ----
    def set_seq_len(self, context_frames, pred_frames, seq_step):
        """The parent's rule for seq_len, then the window list (clip index, start frame) in clip order (kitti_raw.py:77-83)."""
        super().set_seq_len(context_frames, pred_frames, seq_step)
        self.windows = [(c, s) for c, n in enumerate(self.clip_lengths) for s in window_starts(n, self.seq_len, self.seq_step)]
        if not self.windows:
            self.ready_for_usage = False
            raise ValueError(f"Dataset '{self.NAME}': no clip holds the {self.seq_len} frames of a window (the longest has "
                             f"{max(self.clip_lengths, default=0)})")

    def draws(self, seqs, transform=True, frame_hw=None, crop="own", out_chw=None):
        return super().draws(seqs, transform, self._frame_hw if frame_hw is None else frame_hw, crop, out_chw)

    def clips_table(self, windows, transform=True):
        """(int32 [n, 6] rows (clip index, start frame, crop y0, crop x0, flip bits, 0), the n photometric programs) for these windows
        [(clip, start), ...]: one draw per window, in their order."""
        rows, programs = self.draws(list(range(len(windows))), transform)
        table = np.zeros((len(windows), 6), dtype=np.int32)
        table[:, :2] = np.asarray(windows, dtype=np.int64).reshape(len(windows), 2)
        table[:, 2:5] = rows[:, 1:]
        return table, programs

    # ---- samples ----
    def __len__(self):
        return len(self.windows)

    def origin(self, i):
        clip, start = self.windows[i]
        return f"stored clip {clip}, start frame: {start}"

    def batch(self, indices):
        """The reference's dict for these windows from ONE launch (two when a photometric program was drawn): frames
        [n, total_frames, C, h, w] on the GPU, actions zeros [n, total_frames, 1], origin. Equal to the __getitem__ calls in the same order."""
        if not self.ready_for_usage:
            raise RuntimeError("Dataset is not yet ready for usage (maybe you forgot to call set_seq_len()).")
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("batch(indices) needs at least one index")
        if min(indices) < 0 or max(indices) >= len(self):
            raise IndexError(f"sample index outside [0, {len(self)})")
        windows = [self.windows[i] for i in indices]
        table, programs = self.clips_table(windows)
        flat = self._stored()
        if self.storage == "device":
            clip_first = self.clip_first
        else:                                                         # only the windows' frames cross: one staged clip of seq_len frames per sample
            firsts = [int(self.clip_first[c]) + s for c, s in windows]
            staged = self._staging.spans_to_device(flat, firsts, self.seq_len, self.device)
            flat = staged.reshape((len(windows) * self.seq_len,) + tuple(staged.shape[2:]))
            clip_first = np.arange(len(windows) + 1, dtype=np.int64) * self.seq_len
            table[:, 0], table[:, 1] = np.arange(len(windows)), 0
        frames = ops.clips_preprocess(flat, clip_first, table, self.total_frames, self.seq_step, self._crop_hw, self._out_hw, self.img_shape[0],
                                      (self.value_range_min, self.value_range_max))
        self._augment(frames, programs)
        actions = torch.zeros((len(indices), self.total_frames, 1), device=frames.device)
        return {"frames": frames, "actions": actions, "origin": [self.origin(i) for i in indices]}

    @classmethod
    def get_train_val(cls, **dataset_kwargs):
        """(training, validation) datasets of a class with a split of its own for each. Windows exist only once the sequence length is
        set, so a class without a "val" split has no samples that could be split by index here."""
        if cls.VALID_SPLITS != ["train", "val", "test"]:
            raise NotImplementedError(f"dataset class '{cls.__name__}' has no 'val' split; its windows exist only after set_seq_len(), "
                                      f"so divide the clips and build two datasets")
        return cls("train", **dataset_kwargs), cls("val", **dataset_kwargs)
