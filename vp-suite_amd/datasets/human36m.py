"""The videos of Human 3.6M stored as files (vp_suite/datasets/human36m.py, registry key "H36M"): long videos of different lengths AND,
for some, different frame sizes (1002 x 1000 among 1000 x 1000), each yielding many windows (datasets/clips.py).

ON-DISK LAYOUT, A DEPARTURE FROM THE REFERENCE: data_dir/{training,testing}/**/<Scenario ...>.npy, one array [T, H, W, 3] per video (uint8,
uint16 or float32), where the reference reads .mp4 files with OpenCV. No decoder is part of this build; the files are opened with
np.load(mmap_mode="r"). Nothing is downloaded or decoded. tools/export_video_like.py writes a synthetic tree of this layout.

Carried literally (human36m.py:26-78): the constants, the scenario filter (the first word of the file stem), the seeded train / val
shuffle cut at int(n * train_to_val_ratio), and the windows range(SKIP_FIRST_N, frame_count - seq_len + 1, seq_len + seq_step - 1).

WHAT DIFFERS: (1) the reference resizes every frame to the model's frame size with OpenCV while it loads it and crops afterwards; here a
box of the STORED frame (the whole frame, or the crop in the video's own coordinates) is resized once, in the preprocess launch, by the
library's bilinear rule (align_corners=False, no antialiasing). With videos of one size and no img_size nothing is resized. (2) The
reference shuffles the videos in the order of its frame_counts.json, which its preparation step writes in the order the file system
lists them; here the files are sorted by path first."""
import os
import random

import numpy as np

from .._lib import VpxError
from ..utils import set_from_kwarg
from .clips import ClipVPDataset


class Human36MDataset(ClipVPDataset):
    """Each sequence depicts a human actor in a room equipped with different cameras and sensors, in one of several scenarios such as
    "Discussion", "Sitting" or "Smoking"."""
    NAME = "Human 3.6M"
    REFERENCE = "http://vision.imar.ro/human3.6m/description.php"
    IS_DOWNLOADABLE = "No (bring each video as <Scenario ...>.npy; tools/export_video_like.py writes a synthetic stand-in)"
    VALID_SPLITS = ["train", "val", "test"]
    MIN_SEQ_LEN = 994                      # minimum number of frames across all sequences (6349 in the longest)
    ACTION_SIZE = 0
    DATASET_FRAME_SHAPE = (1000, 1000, 3)  # some videos come as (1002, 1000, 3)
    FPS = 50
    SKIP_FIRST_N = 25                      # the actor idles at the start of some videos: the first frames are discarded
    ALL_SCENARIOS = ['Directions', 'Discussion', 'Eating', 'Greeting', 'Phoning', 'Photo', 'Posing', 'Purchases', 'Sitting', 'SittingDown',
                     'Smoking', 'TakingPhoto', 'Waiting', 'WalkDog', 'WalkTogether', 'Walking', 'WalkingDog']

    train_to_val_ratio = 0.96
    scenarios = None                       # the scenarios of this instance (defaults to ALL_SCENARIOS)

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["sequences", "sequences_with_frame_index", "ALL_SCENARIOS"]
        set_from_kwarg(self, dataset_kwargs, "scenarios", default=self.ALL_SCENARIOS, choices=self.ALL_SCENARIOS)
        set_from_kwarg(self, dataset_kwargs, "train_val_seed")
        if self.data_dir is None or not os.path.isdir(os.path.join(str(self.data_dir), "testing" if split == "test" else "training")):
            raise VpxError(f"'{self.NAME}' needs data_dir= holding training/ and testing/ with <Scenario ...>.npy files (got {self.data_dir!r}). "
                           f"Nothing is downloaded or decoded.")
        self.data_dir = os.path.realpath(os.path.join(str(self.data_dir), "testing" if split == "test" else "training"))
        files = [fp for fp in list_npy(self.data_dir) if os.path.basename(fp).split(".")[0].split(" ")[0] in self.scenarios]
        if split in ("train", "val"):
            slice_idx = int(len(files) * self.train_to_val_ratio)
            random.Random(self.train_val_seed).shuffle(files)
            files = files[:slice_idx] if split == "train" else files[slice_idx:]
        if not files:
            raise ValueError(f"Dataset '{self.NAME}': no video of the scenarios {self.scenarios} in split '{split}' of {self.data_dir}")
        clips = [np.load(fp, mmap_mode="r") for fp in files]
        for fp, clip in zip(files, clips):
            if clip.ndim != 4:
                raise ValueError(f"{fp}: expected a video [t, h, w, c], got {clip.shape}")
        self.sequences = {fp: int(clip.shape[0]) for fp, clip in zip(files, clips)}   # (the reference's dict: path -> frame count)
        self.sequences_with_frame_index = []   # filled by set_seq_len()
        self._set_clips(clips)

    def _window_starts(self, clip_index, frame_count):
        return range(self.SKIP_FIRST_N, frame_count - self.seq_len + 1, self.seq_len + self.seq_step - 1)

    def set_seq_len(self, context_frames, pred_frames, seq_step):
        super().set_seq_len(context_frames, pred_frames, seq_step)
        paths = list(self.sequences)
        self.sequences_with_frame_index = [(paths[c], s) for c, s in self.windows]

    def origin(self, i):
        path, start = self.sequences_with_frame_index[i]
        return f"{path}, start frame: {start}"


def list_npy(root, name=None):
    """Every .npy file below root (of that file name, if one is given), as sorted absolute paths."""
    found = []
    for d, _, names in os.walk(root):
        found += [os.path.join(d, n) for n in names if n.endswith(".npy") and (name is None or n == name)]
    return sorted(found, key=lambda fp: fp.split(os.sep))
