"""Caltech Pedestrian stored as files (vp_suite/datasets/caltech_pedestrian.py, registry key "CP"): long drives of different lengths,
each yielding many windows (datasets/clips.py).

ON-DISK LAYOUT, A DEPARTURE FROM THE REFERENCE: data_dir/<setNN>/<Vxxx>.npy, one array [T, H, W, 3] per video (uint8, uint16 or
float32), where the reference reads data_dir/<setNN>/<Vxxx>.seq with OpenCV and their lengths from a frame_counts.json its preparation
step writes. No video decoder is part of this build, so the user brings each video as one array; the files are opened with
np.load(mmap_mode="r") and a length is the array's own. Nothing is downloaded or decoded. tools/export_clips_like.py writes a synthetic
tree of this layout for tests and examples.

The split is the reference's (caltech_pedestrian.py:49-64): set06 ... set10 are the test videos; the videos of set00 ... set05, in the
sorted order of their paths (the order the reference's frame_counts.json lists them in) and shuffled by random.Random(train_val_seed),
are cut at max(1, int(n * train_to_val_ratio)) into training and validation videos."""
import os
import random

import numpy as np

from .._lib import VpxError
from ..utils import set_from_kwarg
from .clips import ClipVPDataset


class CaltechPedestrianDataset(ClipVPDataset):
    """Each sequence shows a short clip of 'driving through regular traffic in an urban environment'."""
    NAME = "Caltech Pedestrian"
    REFERENCE = "http://www.vision.caltech.edu/Image_Datasets/CaltechPedestrians/"
    IS_DOWNLOADABLE = "No (bring each video as <setNN>/<Vxxx>.npy; tools/export_clips_like.py writes a synthetic stand-in)"
    VALID_SPLITS = ["train", "val", "test"]
    MIN_SEQ_LEN = 568                      # minimum number of frames across all sequences (1322 in the 2nd-shortest, 2175 in the longest)
    ACTION_SIZE = 0
    DATASET_FRAME_SHAPE = (480, 640, 3)
    FPS = 30
    TRAIN_VAL_SETS = [f"set{i:02d}" for i in range(6)]       # the official training sets (here: training and validation)
    TEST_SETS = [f"set{i:02d}" for i in range(6, 11)]        # the official test sets

    train_to_val_ratio = 0.9

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["sequences", "sequences_with_frame_index", "TRAIN_VAL_SETS", "TEST_SETS"]
        set_from_kwarg(self, dataset_kwargs, "train_to_val_ratio")
        set_from_kwarg(self, dataset_kwargs, "train_val_seed")
        if self.data_dir is None or not os.path.isdir(str(self.data_dir)):
            raise VpxError(f"'{self.NAME}' needs data_dir= holding <setNN>/<Vxxx>.npy files (got {self.data_dir!r}). Nothing is downloaded or decoded.")
        self.data_dir = os.path.realpath(str(self.data_dir))
        videos = split_videos(list_videos(self.data_dir), split, self.NAME, self.train_to_val_ratio, self.train_val_seed)
        self.sequences, clips = [], []
        for rel in videos:
            fp = os.path.join(self.data_dir, rel)
            clip = np.load(fp, mmap_mode="r")
            if clip.ndim != 4:
                raise ValueError(f"{fp}: expected a video [t, h, w, c], got {clip.shape}")
            clips.append(clip)
            self.sequences.append((fp, int(clip.shape[0])))
        self.sequences_with_frame_index = []   # filled by set_seq_len()
        self._set_clips(clips)

    def set_seq_len(self, context_frames, pred_frames, seq_step):
        super().set_seq_len(context_frames, pred_frames, seq_step)
        self.sequences_with_frame_index = [(self.sequences[c][0], s) for c, s in self.windows]

    def origin(self, i):
        path, start = self.sequences_with_frame_index[i]
        return f"{path}, start frame: {start}"


def list_videos(data_dir):
    """The video files <setNN>/<Vxxx>.npy below data_dir, relative, in the sorted order of their paths."""
    sets = sorted(d for d in os.listdir(data_dir) if os.path.isdir(os.path.join(data_dir, d)))
    return [os.path.join(d, fn) for d in sets for fn in sorted(os.listdir(os.path.join(data_dir, d))) if fn.endswith(".npy")]


def split_videos(videos, split, name, train_to_val_ratio=0.9, train_val_seed=1234):
    """The videos of `split` (caltech_pedestrian.py:49-64), in the order the reference keeps them: the shuffled one for train / val."""
    test_sets, train_val_sets = CaltechPedestrianDataset.TEST_SETS, CaltechPedestrianDataset.TRAIN_VAL_SETS
    if split == "test":
        videos = [v for v in videos if os.path.basename(os.path.dirname(v)) in test_sets]
        if len(videos) < 1:
            raise ValueError(f"Dataset {name}: didn't find enough test sequences -> can't use dataset")
        return videos
    videos = [v for v in videos if os.path.basename(os.path.dirname(v)) in train_val_sets]
    if len(videos) < 2:
        raise ValueError(f"Dataset {name}: didn't find enough train/val sequences -> can't use dataset")
    slice_idx = max(1, int(len(videos) * train_to_val_ratio))
    random.Random(train_val_seed).shuffle(videos)
    return videos[:slice_idx] if split == "train" else videos[slice_idx:]
