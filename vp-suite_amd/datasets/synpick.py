"""SynPick - Moving stored as files (vp_suite/datasets/synpick.py, registry key "SPM"): episodes of a suction gripper moving through a bin,
with the gripper's position per frame; the actions of a sample are the position differences between its consecutive frames
(datasets/clips.py: clips with `positions`).

ON-DISK LAYOUT, A DEPARTURE FROM THE REFERENCE: data_dir/processed/<split>/<episode>.npy, one array [T, 135, 240, 3] per episode (uint8,
uint16 or float32), and <episode>_gripper.npy [T, 3] (float32 or float64) beside it: row f is `cam_t_m2c` of the LAST object of frame f
in the episode's scene_gt json (synpick.py:50-56), frame number = row. The reference reads rgb/<episode>_<frame>.jpg|png files with
OpenCV and the json files. No decoder is part of this build; the files are opened with np.load(mmap_mode="r"). Nothing is downloaded or
decoded. tools/export_video_like.py writes a synthetic tree of this layout.

Carried literally: the constants and splits, and the window rule of _set_seq_len (synpick.py:58-94), restated per episode in
_window_starts(): the reference walks ONE index over the images of all episodes in sorted order; a start is valid when its frame number
is >= SKIP_FIRST_N, the window's last frame lies in the same episode, it does not overlap the last valid window (global index >= last
valid index + seq_len, counted over the concatenated episodes), and the xy distances between consecutive RETURNED frames satisfy
most(> 1.0) (at least 0.67 of them) and all(< 30.0). No valid window raises the reference's ValueError. The actions are
positions[frame j + 1] - positions[frame j] over the returned frames, total_frames - 1 rows (the reference's "sequence length is one
less"), subtracted in the stored precision and rounded to float32 once, as numpy's difference followed by .float() is.

WHAT DIFFERS: `config` carries supports_actions = True (see datasets/base.py)."""
import math
import os

import numpy as np

from .._lib import VpxError
from .clips import ClipVPDataset


def most(flags, factor=0.67):
    """True if at least `factor` of the entries are true (vp_suite/utils/utils.py:15-25)."""
    return sum(flags) >= factor * len(flags)


class SynpickMovingDataset(ClipVPDataset):
    """Each sequence depicts a robotic suction cap gripper that moves around in a red bin filled with objects, approaching 4 waypoints
    randomly chosen from the 4 corners and pushing the objects around on its way."""
    NAME = "SynPick - Moving"
    REFERENCE = "https://arxiv.org/abs/2107.04852"
    IS_DOWNLOADABLE = "No (bring each episode as <episode>.npy and <episode>_gripper.npy; tools/export_video_like.py writes a synthetic stand-in)"
    VALID_SPLITS = ["train", "val", "test"]
    SKIP_FIRST_N = 72                      # the gripper is still descending into the bin
    MIN_SEQ_LEN = 90
    ACTION_SIZE = 3
    DATASET_FRAME_SHAPE = (135, 240, 3)
    GRIPPER_SUFFIX = "_gripper.npy"

    train_to_val_ratio = 0.9

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["episode_fps", "gripper_pos", "valid_idx"]
        if self.data_dir is None:
            raise VpxError(f"'{self.NAME}' needs data_dir= holding processed/<split>/<episode>.npy and <episode>_gripper.npy files. "
                           f"Nothing is downloaded or decoded.")
        self.data_dir = os.path.realpath(os.path.join(str(self.data_dir), "processed", split))
        if not os.path.isdir(self.data_dir):
            raise VpxError(f"'{self.NAME}': no directory {self.data_dir}. Nothing is downloaded or decoded.")
        names = sorted(fn for fn in os.listdir(self.data_dir) if fn.endswith(".npy") and not fn.endswith(self.GRIPPER_SUFFIX))
        if not names:
            raise ValueError(f"Dataset '{self.NAME}': no episode file (.npy) in {self.data_dir}")
        self.episode_fps = [os.path.join(self.data_dir, fn) for fn in names]
        clips, self.gripper_pos = [], []
        for fp in self.episode_fps:
            gripper_fp = fp[:-len(".npy")] + self.GRIPPER_SUFFIX
            if not os.path.isfile(gripper_fp):
                raise VpxError(f"'{self.NAME}': no file {gripper_fp}. Nothing is downloaded or decoded.")
            clip, pos = np.load(fp, mmap_mode="r"), np.load(gripper_fp)
            if clip.ndim != 4:
                raise ValueError(f"{fp}: expected an episode [t, h, w, c], got {clip.shape}")
            if pos.ndim != 2 or pos.shape[1] != type(self).ACTION_SIZE:
                raise ValueError(f"{gripper_fp}: expected gripper positions [t, {type(self).ACTION_SIZE}], got {pos.shape}")
            clips.append(clip)
            self.gripper_pos.append(pos)
        self.valid_idx = []                    # the reference's global indices; filled by set_seq_len()
        self._set_clips(clips)
        self._set_positions(self.gripper_pos)

    def _window_starts(self, clip_index, frame_count):
        if clip_index == 0:                                           # a new walk over the concatenated episodes (synpick.py:60-61)
            self._last_valid_idx, self.valid_idx = -1 * self.seq_len, []
        base, pos, starts = int(self.clip_first[clip_index]), self.gripper_pos[clip_index], []
        for start in range(self.SKIP_FIRST_N, frame_count - self.seq_len + 1):   # first frames discarded; the window stays in its episode
            idx = base + start
            if idx < self._last_valid_idx + self.seq_len:             # sequences should not overlap
                continue
            xy = [(float(pos[start + off][0]), float(pos[start + off][1])) for off in self.frame_offsets]
            deltas = [math.sqrt((new[0] - old[0]) * (new[0] - old[0]) + (new[1] - old[1]) * (new[1] - old[1])) for old, new in zip(xy, xy[1:])]
            if not (most([d > 1.0 for d in deltas]) and all(d < 30.0 for d in deltas)):   # no considerable, or implausible, gripper movement
                continue
            starts.append(start)
            self.valid_idx.append(idx)
            self._last_valid_idx = idx
        return starts

    def _no_window_error(self):
        return ValueError("No valid indices in generated dataset! Perhaps the calculated sequence length is longer than the trajectories of the data?")

    def origin(self, i):
        clip, start = self.windows[i]
        return f"1st frame: {self.episode_fps[clip]}, frame {start}, frames: {self.total_frames}, step: {self.seq_step}"
