"""Long clips of different lengths, each yielding many windows: the storage model of the reference's KITTI raw, Caltech Pedestrian, KTH,
Human 3.6M, Physics 101 and SynPick classes (vp_suite/datasets/kitti_raw.py:77-95, caltech_pedestrian.py:69-86, human36m.py:71-78,
physics101.py:53-70, synpick.py:58-113).

ClipVPDataset: the clips of a split are held back to back as ONE raw buffer [frames, H, W(, C)] — on the GPU, or in pinned host memory —
with the first frame of every clip beside it. set_seq_len() lists the windows by the reference's rule,
    for every clip: start in range(0, frame_count - seq_len + 1, seq_len + seq_step - 1),
(a subclass with a rule of its own overrides _window_starts()) and sample i is window i: frames start, start + seq_step, ... of its clip
through ONE launch of vpx_clips_preprocess per batch (csrc/frames.hip: the per-pixel code of the stored-sequence launch behind a 64-bit
frame offset looked up per sample). Crops, flips, photometric programs, preprocess() / postprocess(), loader() and `config` are
StoredVPDataset's; the draws are per window.

MIXED FRAME SIZES: the clips may differ in H_i x W_i (Human 3.6M holds 1002 x 1000 videos among 1000 x 1000 ones). Then the buffer is one
run of elements, `img_size` is required, a batch is ONE launch of vpx_clips_preprocess_var, and every window's box — the whole frame, or
the crop drawn in the clip's own coordinates — is resized to img_size in that launch. With equal sizes nothing changes: the launch, the
draws and the bits are those of vpx_clips_preprocess.

POSITIONS: `positions=[...]`, one [T_i, A] float32 / float64 array per clip, are kept where the frames are; `actions` of a sample is then
the [total_frames - 1, A] differences of the positions of consecutive returned frames (synpick.py:135-137) from one launch of
vpx_actions_diff_gather, and `config` carries supports_actions = True (see datasets/base.py).

WHAT DIFFERS FROM THE REFERENCE: set_seq_len() builds the window list anew (the reference appends to the list of an earlier call); a
configuration that yields no window at all raises ValueError (the reference returns an empty dataset); with mixed sizes a box of the
STORED frame is resized once, where the reference resizes every frame to the model's size while it loads and crops afterwards."""
import numpy as np
import torch

from .. import ops
from .._lib import VpxError
from .base import StoredVPDataset, check_photometric, parse_img_size


def window_starts(frame_count, seq_len, seq_step):
    """The start frames of a clip's windows (kitti_raw.py:80-81): none when the clip is shorter than seq_len."""
    return range(0, frame_count - seq_len + 1, seq_len + seq_step - 1)


class _PinnedFlatStage:
    """The pinned staging buffer of a mixed-shape dataset: runs of elements of different lengths are gathered into it back to back and
    copied to the GPU once (datasets/base.py's _PinnedStage for pieces of one shape)."""

    def __init__(self):
        self.buffer = self.event = None

    def to_device(self, flat, spans, device):
        """(the staged elements on the GPU, the offset of every span in them) for spans [(first element, count), ...] of flat."""
        total = sum(n for _, n in spans)
        if self.buffer is None or self.buffer.numel() < total or self.buffer.dtype != flat.dtype:
            self.buffer = torch.empty(total, dtype=flat.dtype).pin_memory()
        elif self.event is not None:
            self.event.synchronize()                              # the previous batch's copy has left the buffer
        offsets, at = [], 0
        for first, n in spans:
            self.buffer[at:at + n].copy_(flat[first:first + n])
            offsets.append(at)
            at += n
        dev = self.buffer[:total].to(device, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return dev, offsets


class ClipVPDataset(StoredVPDataset):
    """clips: a list of arrays [T_i, H_i, W_i(, C)] of one dtype (uint8, uint16 or float32) and one channel count; the lengths T_i may
    differ, and so may the frame sizes (then img_size= is required: see the module docstring).
    Memory-mapped arrays are read once, when the buffer is first placed. storage="device": the buffer lives on the GPU and a batch is one
    launch over it. storage="pinned": it lives in pinned host memory and only the seq_len frames of each window of a batch are gathered
    into a pinned staging block and copied; the launch then runs over that block, its offsets and table relative to it.
    positions: None, or one [T_i, A] float32 / float64 array per clip. Without them `actions` is a [t, 1] zero tensor per sample, as in
    the reference; with them it is the [t - 1, A] differences of consecutive returned frames' positions."""
    NAME = "Stored clips"

    def __init__(self, split, clips=None, positions=None, **dataset_kwargs):
        if dataset_kwargs.get("raw") is not None or dataset_kwargs.get("actions") is not None:
            raise ValueError("a clip dataset takes clips=[...]; raw= and actions= belong to StoredVPDataset")
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["clip_lengths", "clip_first", "windows", "clip_hw", "mixed_shapes"]
        self._clips_host = self._positions_host = self._positions = None
        self._flat_staging = _PinnedFlatStage()
        self.clip_lengths, self.clip_first, self.windows, self.clip_hw, self.mixed_shapes = [], np.zeros(1, dtype=np.int64), [], [], False
        if clips is not None:
            self._set_clips(clips)
        if positions is not None:
            self._set_positions(positions)

    # ---- storage ----
    def _set_clips(self, clips):
        """Takes the clips [T_i, H_i, W_i(, C)] (numpy, memory-mapped or not) and fixes everything that depends on their shape."""
        clips = [c.detach().cpu().numpy() if torch.is_tensor(c) else np.asanyarray(c) for c in clips]
        if not clips:
            raise ValueError("a clip dataset needs at least one clip")
        first = clips[0]
        if first.dtype not in (np.uint8, np.uint16, np.float32):
            raise ValueError(f"stored clips must be uint8, uint16 or float32 (got {first.dtype})")
        if first.ndim not in (3, 4) or min(first.shape) < 1:
            raise ValueError(f"a stored clip must be [T, H, W] or [T, H, W, C], nothing empty (got {first.shape})")
        for k, c in enumerate(clips):
            if c.dtype != first.dtype or c.ndim != first.ndim or min(c.shape) < 1 or c.shape[3:] != first.shape[3:]:
                raise ValueError(f"clip {k}: {c.dtype} {c.shape} differs from the first clip's element type or channel count ({first.dtype} {first.shape[1:]})")
        self.clip_hw = [(int(c.shape[1]), int(c.shape[2])) for c in clips]
        self.mixed_shapes = any(hw != self.clip_hw[0] for hw in self.clip_hw)
        if self.mixed_shapes and self.img_size is None:
            k = next(k for k, hw in enumerate(self.clip_hw) if hw != self.clip_hw[0])
            raise ValueError(f"clip {k}: {clips[k].dtype} {clips[k].shape} differs from the first clip's frame shape ({first.dtype} {first.shape[1:]}); "
                             f"clips of mixed frame sizes need img_size=, the size every window is resized to")
        self._clips_host = clips
        self.clip_lengths = [int(c.shape[0]) for c in clips]
        self.clip_first = np.concatenate([[0], np.cumsum(self.clip_lengths)]).astype(np.int64)
        if type(self).MIN_SEQ_LEN is NotImplemented:
            self.MIN_SEQ_LEN = max(self.clip_lengths)                 # a window fits the longest clip at the most
        self._frame_hw = self.clip_hw[0]
        channels = int(first.shape[3]) if first.ndim == 4 else 1
        if not self.mixed_shapes:
            self._set_frame_geometry(self._frame_hw[0], self._frame_hw[1], channels)
            return
        # mixed sizes: the box is the crop (it has to fit every clip) or each clip's whole frame, and it is always resized to img_size
        self._channels = channels
        sizes = [n * h * w * channels for n, (h, w) in zip(self.clip_lengths, self.clip_hw)]
        self._elem_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        c_out = self.OUT_CHANNELS or channels
        if c_out != channels and not (channels == 1 and c_out == 3):
            raise ValueError(f"{c_out} channels cannot be returned from {channels} stored ones (equal, or 3 from 1)")
        self.DATASET_FRAME_SHAPE = self._frame_hw + (int(c_out),)
        self._crop_hw = None if self.crop is None else tuple(self.crop[-2:])
        for k, (h, w) in enumerate(self.clip_hw):
            if self.crop is not None and (self._crop_hw[0] > h or self._crop_hw[1] > w):
                raise ValueError(f"the {self._crop_hw[0]}x{self._crop_hw[1]} crop does not fit the {h}x{w} frames of clip {k} (there is no padding)")
            if self.crop is not None and self.crop[0] == "box" and (self.crop[1] + self._crop_hw[0] > h or self.crop[2] + self._crop_hw[1] > w):
                raise ValueError(f"the crop box {self.crop[1:]} leaves the {h}x{w} frames of clip {k} (there is no padding)")
        self._out_hw = tuple(int(v) for v in parse_img_size(self.img_size, self._frame_hw))
        self.img_shape = (int(c_out),) + self._out_hw
        check_photometric(self.photometric, int(c_out))

    def _set_positions(self, positions):
        """Takes one position array [T_i, A] (numpy float32 / float64) per clip set before."""
        if self._clips_host is None:
            raise ValueError("positions need the clips they belong to: give clips= as well")
        positions = [p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p) for p in positions]
        if len(positions) != len(self._clips_host):
            raise ValueError(f"{len(positions)} position arrays for {len(self._clips_host)} clips (one per clip)")
        first = positions[0]
        if first.dtype not in (np.float32, np.float64):
            raise ValueError(f"stored positions must be float32 or float64 (got {first.dtype})")
        for k, (p, n) in enumerate(zip(positions, self.clip_lengths)):
            if p.dtype != first.dtype or p.ndim != 2 or p.shape[1] < 1 or p.shape[1:] != first.shape[1:] or p.shape[0] != n:
                raise ValueError(f"positions of clip {k}: {p.dtype} {p.shape} must be {first.dtype} [{n}, A], one row per frame of the clip")
        self._positions_host = np.ascontiguousarray(np.concatenate(positions))
        self.ACTION_SIZE = int(first.shape[1])

    def _set_raw(self, raw):
        raise ValueError("a clip dataset takes clips=[...], not raw=")

    def _set_actions(self, actions):
        raise ValueError("a clip dataset stores no actions")

    def _stored(self):
        """The buffer [frames, H, W(, C)] (mixed frame sizes: the elements of every clip, back to back) where the storage mode keeps it
        (made at the first use: building a dataset needs no GPU)."""
        if self._raw is None:
            if self._clips_host is None:
                raise VpxError(f"'{self.NAME}' holds no clips")
            dtype = torch.from_numpy(np.empty(0, dtype=self._clips_host[0].dtype)).dtype
            if self.mixed_shapes:
                flat = torch.empty(int(self._elem_first[-1]), dtype=dtype)
            else:
                flat = torch.empty((int(self.clip_first[-1]),) + tuple(self._clips_host[0].shape[1:]), dtype=dtype)
            if self.storage == "pinned":
                flat = flat.pin_memory()
            firsts = self._elem_first if self.mixed_shapes else self.clip_first
            for first, clip in zip(firsts[:-1].tolist(), self._clips_host):
                piece = torch.from_numpy(np.array(clip))              # (a copy: a memory-mapped file is read here, once)
                if self.mixed_shapes:
                    flat[first:first + piece.numel()].copy_(piece.reshape(-1))
                else:
                    flat[first:first + clip.shape[0]].copy_(piece)
            self._raw = flat.to(self.device) if self.storage == "device" else flat
        return self._raw

    def _stored_positions(self):
        if self._positions is None:
            self._positions = self._place(self._positions_host)
        return self._positions

    # ---- windows ----
    def _window_starts(self, clip_index, frame_count):
        """The start frames of this clip's windows at the present seq_len / seq_step: the hook of a dataset with a rule of its own. It is
        called once per clip, in clip order, by every set_seq_len()."""
        return window_starts(frame_count, self.seq_len, self.seq_step)

    def _no_window_error(self):
        return ValueError(f"Dataset '{self.NAME}': no clip holds the {self.seq_len} frames of a window (the longest has "
                          f"{max(self.clip_lengths, default=0)})")

    def set_seq_len(self, context_frames, pred_frames, seq_step):
        """The parent's rule for seq_len, then the window list (clip index, start frame) in clip order (kitti_raw.py:77-83)."""
        super().set_seq_len(context_frames, pred_frames, seq_step)
        self.windows = [(c, int(s)) for c, n in enumerate(self.clip_lengths) for s in self._window_starts(c, n)]
        if not self.windows:
            self.ready_for_usage = False
            raise self._no_window_error()

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

    def clips_var_table(self, windows, transform=True):
        """The same for clips of mixed frame sizes: int32 [n, 8] rows (clip index, start frame, box y0, box x0, box h, box w, flip bits,
        0). The box is the crop, placed in the clip's OWN H_i x W_i frame ("center" and "random" use it), or the whole frame; the draws
        per window and their order are StoredVPDataset's (box row, box column, flips, then the photometric entries)."""
        table, programs = np.zeros((len(windows), 8), dtype=np.int32), []
        for k, (c, s) in enumerate(windows):
            hw = self.clip_hw[c]
            y0, x0, bits, drawn = self._draw_geometry(hw, self.crop, transform)
            bh, bw = hw if (self.crop is None or not transform) else self._crop_hw
            table[k] = (c, s, y0, x0, bh, bw, bits, 0)
            programs.append(self._draw_program(tuple(self.img_shape), drawn, transform))
        return table, programs

    # ---- samples ----
    def __len__(self):
        return len(self.windows)

    def origin(self, i):
        clip, start = self.windows[i]
        return f"stored clip {clip}, start frame: {start}"

    @property
    def config(self) -> dict:
        cfg = super().config
        if self._positions_host is not None:
            cfg["supports_actions"] = True                        # as a stored dataset with actions does (datasets/base.py)
        return cfg

    def _frames_equal(self, windows, table):
        flat = self._stored()
        if self.storage == "device":
            clip_first = self.clip_first
        else:                                                         # only the windows' frames cross: one staged clip of seq_len frames per sample
            firsts = [int(self.clip_first[c]) + s for c, s in windows]
            staged = self._staging.spans_to_device(flat, firsts, self.seq_len, self.device)
            flat = staged.reshape((len(windows) * self.seq_len,) + tuple(staged.shape[2:]))
            clip_first = np.arange(len(windows) + 1, dtype=np.int64) * self.seq_len
            table[:, 0], table[:, 1] = np.arange(len(windows)), 0
        return ops.clips_preprocess(flat, clip_first, table, self.total_frames, self.seq_step, self._crop_hw, self._out_hw, self.img_shape[0],
                                    (self.value_range_min, self.value_range_max))

    def _frames_mixed(self, windows, table):
        flat = self._stored()
        per_frame = [h * w * self._channels for h, w in self.clip_hw]
        if self.storage == "device":
            geom = np.array([(int(self._elem_first[c]), n, h, w) for c, (n, (h, w)) in enumerate(zip(self.clip_lengths, self.clip_hw))], dtype=np.int64)
        else:                                                         # as above, with each window's own frame bytes
            spans = [(int(self._elem_first[c]) + s * per_frame[c], self.seq_len * per_frame[c]) for c, s in windows]
            flat, offsets = self._flat_staging.to_device(flat, spans, self.device)
            geom = np.array([(off, self.seq_len) + self.clip_hw[c] for off, (c, _) in zip(offsets, windows)], dtype=np.int64)
            table[:, 0], table[:, 1] = np.arange(len(windows)), 0
        return ops.clips_preprocess_var(flat, geom, table, self.total_frames, self.seq_step, self._out_hw, self._channels, self.img_shape[0],
                                        (self.value_range_min, self.value_range_max))

    def _position_diffs(self, windows):
        rows = self._stored_positions()
        table = np.zeros((len(windows), 8), dtype=np.int32)
        if self.storage == "device":
            clip_first = self.clip_first
            table[:, :2] = np.asarray(windows, dtype=np.int64).reshape(len(windows), 2)
        else:                                                         # staged like the frames: seq_len rows per window
            firsts = [int(self.clip_first[c]) + s for c, s in windows]
            staged = self._actions_staging.spans_to_device(rows, firsts, self.seq_len, self.device)
            rows = staged.reshape(len(windows) * self.seq_len, staged.shape[2])
            clip_first = np.arange(len(windows) + 1, dtype=np.int64) * self.seq_len
            table[:, 0] = np.arange(len(windows))
        return ops.actions_diff_gather(rows, clip_first, table, self.total_frames, self.seq_step)

    def batch(self, indices):
        """The reference's dict for these windows from ONE launch (two when a photometric program was drawn): frames
        [n, total_frames, C, h, w] on the GPU, actions zeros [n, total_frames, 1], origin. Equal to the __getitem__ calls in the same order.
        With positions: one more launch, directly after the frames launch, yields actions [n, total_frames - 1, ACTION_SIZE]."""
        if not self.ready_for_usage:
            raise RuntimeError("Dataset is not yet ready for usage (maybe you forgot to call set_seq_len()).")
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("batch(indices) needs at least one index")
        if min(indices) < 0 or max(indices) >= len(self):
            raise IndexError(f"sample index outside [0, {len(self)})")
        windows = [self.windows[i] for i in indices]
        if self.mixed_shapes:
            table, programs = self.clips_var_table(windows)
            frames = self._frames_mixed(windows, table)
        else:
            table, programs = self.clips_table(windows)
            frames = self._frames_equal(windows, table)
        if self._positions_host is not None:
            if self.total_frames < 2:
                raise ValueError(f"Dataset '{self.NAME}': position differences need at least two frames per sample")
            actions = self._position_diffs(windows)
        self._augment(frames, programs)
        if self._positions_host is None:
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
