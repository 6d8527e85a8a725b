"""The videos of Physics 101 stored as files (vp_suite/datasets/physics101.py, registry key "P101"): ONE sample per video, taken from its
start, middle or end (datasets/clips.py holds the videos; each contributes one window).

ON-DISK LAYOUT, A DEPARTURE FROM THE REFERENCE: data_dir/**/<camera>.npy, one array [T, H, W, 3] per video (uint8, uint16 or float32),
where the reference reads <camera>.mp4 files. No decoder is part of this build; the files are opened with np.load(mmap_mode="r").
Nothing is downloaded or decoded. tools/export_video_like.py writes a synthetic tree of this layout.

Carried literally (physics101.py:21-52): the constants, the `camera` and `subseq` choices, the sorted file list shuffled by
random.Random(trainval_test_seed) and cut at int(n * trainval_to_test_ratio) into "train" and "test"; VALID_SPLITS has no "val", so
get_train_val() splits the training samples by index (datasets/base.py), which works because a video is a sample before any sequence
length is set.

WHAT DIFFERS: the reference reads only the first total_frames frames of a video and applies seq_step and `subseq` to those, so its
"start", "middle" and "end" coincide and seq_step > 1 returns fewer frames than asked for. Here the window is total_frames frames at
seq_step (seq_len stored frames) taken from the WHOLE video: "start" begins at frame 0, "end" at T - seq_len, "middle" at
(T - seq_len) // 2. A video shorter than seq_len raises ValueError at set_seq_len()."""
import os
import random

import numpy as np

from .._lib import VpxError
from ..utils import set_from_kwarg
from .base import StoredVPDataset
from .clips import ClipVPDataset
from .human36m import list_npy


class Physics101Dataset(ClipVPDataset):
    """Each sequence depicts object-centered physical properties by showing objects of various materials and appearances in different
    physical scenarios such as sliding down a ramp or bouncing off a flat surface."""
    NAME = "Physics 101"
    REFERENCE = "http://phys101.csail.mit.edu/"
    IS_DOWNLOADABLE = "No (bring each video as <camera>.npy; tools/export_video_like.py writes a synthetic stand-in)"
    AVAILABLE_CAMERAS = ["Camera_1", "Camera_2", "Kinect_RGB_1"]
    AVAILABLE_SUBSEQ = ["start", "middle", "end"]
    MIN_SEQ_LEN = 16
    ACTION_SIZE = 0
    DATASET_FRAME_SHAPE = (1080, 1920, 3)

    camera = "Kinect_RGB_1"
    subseq = "middle"
    trainval_to_test_ratio = 0.8
    trainval_test_seed = 1612              # the value of the 'Noether Networks' code

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["vid_filepaths", "AVAILABLE_CAMERAS", "AVAILABLE_SUBSEQ"]
        set_from_kwarg(self, dataset_kwargs, "camera", choices=self.AVAILABLE_CAMERAS)
        set_from_kwarg(self, dataset_kwargs, "subseq", choices=self.AVAILABLE_SUBSEQ)
        set_from_kwarg(self, dataset_kwargs, "trainval_test_seed")
        if self.data_dir is None or not os.path.isdir(str(self.data_dir)):
            raise VpxError(f"'{self.NAME}' needs data_dir= holding <camera>.npy files (got {self.data_dir!r}). Nothing is downloaded or decoded.")
        self.data_dir = os.path.realpath(str(self.data_dir))
        self.vid_filepaths = list_npy(self.data_dir, f"{self.camera}.npy")
        slice_idx = int(len(self.vid_filepaths) * self.trainval_to_test_ratio)
        random.Random(self.trainval_test_seed).shuffle(self.vid_filepaths)
        self.vid_filepaths = self.vid_filepaths[:slice_idx] if split == "train" else self.vid_filepaths[slice_idx:]
        if not self.vid_filepaths:
            raise ValueError(f"Dataset '{self.NAME}': no {self.camera}.npy file for split '{split}' below {self.data_dir}")
        clips = [np.load(fp, mmap_mode="r") for fp in self.vid_filepaths]
        for fp, clip in zip(self.vid_filepaths, clips):
            if clip.ndim != 4:
                raise ValueError(f"{fp}: expected a video [t, h, w, c], got {clip.shape}")
        self._set_clips(clips)
        self.windows = [(c, 0) for c in range(len(clips))]           # a video is a sample; set_seq_len() places its window

    def _window_starts(self, clip_index, frame_count):
        if frame_count < self.seq_len:
            self.ready_for_usage = False
            raise ValueError(f"Dataset '{self.NAME}': {self.vid_filepaths[clip_index]} holds {frame_count} frames, fewer than the {self.seq_len} of a window")
        return [{"start": 0, "end": frame_count - self.seq_len, "middle": (frame_count - self.seq_len) // 2}[self.subseq]]

    def origin(self, i):
        return f"{self.vid_filepaths[self.windows[i][0]]}, subseq mode: {self.subseq}"

    @classmethod
    def get_train_val(cls, **dataset_kwargs):
        return StoredVPDataset.get_train_val.__func__(cls, **dataset_kwargs)
