"""Moving MNIST stored as files (vp_suite/datasets/mmnist.py, registry key "MM"): data_dir/<split>/seq_NNNNN.npy, one gray sequence
[T', H, W] each, as the reference's preparation step and tools/export_mmnist.py write them. The files of a split become ONE raw tensor;
the gray channel is repeated to three (mmnist.py:56) inside the preprocess launch, not on the host. Nothing is downloaded or generated."""
import os
import re

import numpy as np

from .._lib import VpxError
from .base import StoredVPDataset


class MovingMNISTDataset(StoredVPDataset):
    """Two MNIST digits moving linearly in front of a black background, bouncing off the walls and overlapping each other."""
    NAME = "Moving MNIST"
    REFERENCE = "https://arxiv.org/abs/1502.04681v3"
    IS_DOWNLOADABLE = "No (prepare the files with the reference's scripts, or write them with tools/export_mmnist.py)"
    ACTION_SIZE = 0
    DATASET_FRAME_SHAPE = (64, 64, 3)
    OUT_CHANNELS = 3

    train_to_val_ratio = 0.96

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["data_ids", "data_fps"]
        if self.data_dir is None:
            raise VpxError(f"'{self.NAME}' needs data_dir= holding <split>/seq_NNNNN.npy files. Nothing is downloaded or generated.")
        self.data_dir = os.path.realpath(os.path.join(str(self.data_dir), split))
        if not os.path.isdir(self.data_dir):
            raise VpxError(f"'{self.NAME}': no directory {self.data_dir}. Nothing is downloaded or generated.")
        self.data_ids = sorted(fn for fn in os.listdir(self.data_dir) if re.match(r"seq_[0-9]+\.npy", fn))
        self.data_fps = [os.path.join(self.data_dir, fn) for fn in self.data_ids]
        if not self.data_fps:
            raise VpxError(f"'{self.NAME}': no seq_NNNNN.npy file in {self.data_dir}. Nothing is downloaded or generated.")
        first = np.load(self.data_fps[0])
        if first.ndim != 3:
            raise ValueError(f"{self.data_fps[0]}: expected a gray sequence [t, h, w], got {first.shape}")
        raw = np.empty((len(self.data_fps),) + first.shape, dtype=first.dtype)
        for i, fp in enumerate(self.data_fps):
            seq = first if i == 0 else np.load(fp)
            if seq.shape != first.shape or seq.dtype != first.dtype:
                raise ValueError(f"{fp}: {seq.dtype} {seq.shape} differs from the split's first file ({first.dtype} {first.shape})")
            raw[i] = seq
        self._set_raw(raw)   # MIN_SEQ_LEN = the stored sequence length (mmnist.py:45)

    def origin(self, i):
        return self.data_fps[i]
