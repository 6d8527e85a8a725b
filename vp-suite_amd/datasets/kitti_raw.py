"""The "raw data" regime of the KITTI Vision Benchmark Suite stored as files (vp_suite/datasets/kitti_raw.py, registry key "KITTI"):
long drives of different lengths, each yielding many windows (datasets/clips.py).

ON-DISK LAYOUT, A DEPARTURE FROM THE REFERENCE: data_dir/<date>/<drive>/<camera>.npy, one array [T, H, W, 3] per drive and camera
(uint8, uint16 or float32), where the reference reads data_dir/<date>/<drive>/<camera>/data/*.png with OpenCV. No image decoder is part
of this build, so the user brings each drive's frames as one array; the files are opened with np.load(mmap_mode="r"). Nothing is
downloaded or decoded. tools/export_clips_like.py writes a synthetic tree of this layout for tests and examples.

The split is the reference's (kitti_raw.py:49-67): the drive directories, shuffled by random.Random(trainval_test_seed), are cut at
max(1, int(n * trainval_to_test_ratio)) into training / validation and test drives, and the former, shuffled by
random.Random(train_val_seed), at max(1, int(n * train_to_val_ratio)) into training and validation drives. WHAT DIFFERS: the reference
shuffles the directories in the order the file system lists them, which no rule fixes; here they are sorted by path first, so a tree
gives the same split on every machine."""
import os
import random

import numpy as np

from .._lib import VpxError
from ..utils import set_from_kwarg
from .clips import ClipVPDataset


class KITTIRawDataset(ClipVPDataset):
    """Each sequence shows a short clip of 'driving around the mid-size city of Karlsruhe, in rural areas and on highways'."""
    NAME = "KITTI raw"
    REFERENCE = "http://www.cvlibs.net/datasets/kitti/raw_data.php"
    IS_DOWNLOADABLE = "No (bring each drive as <date>/<drive>/<camera>.npy; tools/export_clips_like.py writes a synthetic stand-in)"
    VALID_SPLITS = ["train", "val", "test"]
    MIN_SEQ_LEN = 994                      # minimum number of frames across all sequences (6349 in the longest)
    ACTION_SIZE = 0
    DATASET_FRAME_SHAPE = (375, 1242, 3)
    FPS = 10
    AVAILABLE_CAMERAS = [f"image_{i:02d}" for i in range(4)]   # greyscale left / right, colour left / right

    camera = "image_02"
    trainval_to_test_ratio = 0.8
    train_to_val_ratio = 0.9
    trainval_test_seed = 1234

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["sequences", "sequences_with_frame_index", "AVAILABLE_CAMERAS"]
        for name in ("camera", "trainval_to_test_ratio", "train_to_val_ratio", "trainval_test_seed", "train_val_seed"):
            set_from_kwarg(self, dataset_kwargs, name)
        if self.data_dir is None or not os.path.isdir(str(self.data_dir)):
            raise VpxError(f"'{self.NAME}' needs data_dir= holding <date>/<drive>/<camera>.npy files (got {self.data_dir!r}). "
                           f"Nothing is downloaded or decoded.")
        self.data_dir = os.path.realpath(str(self.data_dir))
        sequence_dirs = split_drives(list_drives(self.data_dir), split, self.NAME, self.trainval_to_test_ratio, self.trainval_test_seed,
                                     self.train_to_val_ratio, self.train_val_seed)
        self.sequences, clips = [], []
        for rel in sorted(sequence_dirs, key=lambda r: r.split(os.sep)):   # (pathlib's order: by components)
            fp = os.path.join(self.data_dir, rel, f"{self.camera}.npy")
            if not os.path.isfile(fp):
                raise VpxError(f"'{self.NAME}': no file {fp}. Nothing is downloaded or decoded.")
            clip = np.load(fp, mmap_mode="r")
            if clip.ndim != 4:
                raise ValueError(f"{fp}: expected a drive [t, h, w, c], got {clip.shape}")
            clips.append(clip)
            self.sequences.append((os.path.join(self.data_dir, rel), int(clip.shape[0])))
        self.sequences_with_frame_index = []   # filled by set_seq_len()
        self._set_clips(clips)

    def set_seq_len(self, context_frames, pred_frames, seq_step):
        super().set_seq_len(context_frames, pred_frames, seq_step)
        self.sequences_with_frame_index = [(self.sequences[c][0], s) for c, s in self.windows]

    def origin(self, i):
        path, start = self.sequences_with_frame_index[i]
        return f"{path}, start frame: {start}"


def list_drives(data_dir):
    """The drive directories <date>/<drive> below data_dir, relative and sorted (kitti_raw.py:50, in a fixed order)."""
    dates = sorted(d for d in os.listdir(data_dir) if os.path.isdir(os.path.join(data_dir, d)))
    return [os.path.join(d, sub) for d in dates for sub in sorted(os.listdir(os.path.join(data_dir, d))) if os.path.isdir(os.path.join(data_dir, d, sub))]


def split_drives(sequence_dirs, split, name, trainval_to_test_ratio=0.8, trainval_test_seed=1234, train_to_val_ratio=0.9, train_val_seed=1234):
    """The drives of `split` (kitti_raw.py:51-67), unsorted: two seeded shuffles and two max(1, int(...)) cuts."""
    sequence_dirs = list(sequence_dirs)
    if len(sequence_dirs) < 3:
        raise ValueError(f"Dataset {name}: found less than 3 sequences -> can't split dataset -> can't use it")
    slice_idx = max(1, int(len(sequence_dirs) * trainval_to_test_ratio))
    random.Random(trainval_test_seed).shuffle(sequence_dirs)
    if split == "test":
        return sequence_dirs[slice_idx:]
    sequence_dirs = sequence_dirs[:slice_idx]
    slice_idx = max(1, int(len(sequence_dirs) * train_to_val_ratio))
    random.Random(train_val_seed).shuffle(sequence_dirs)
    return sequence_dirs[:slice_idx] if split == "train" else sequence_dirs[slice_idx:]
