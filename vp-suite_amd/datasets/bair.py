"""BAIR robot pushing stored as files (vp_suite/datasets/bair.py, registry key "BAIR"): data_dir/softmotion30_44k/<split>/ holds per
sequence seq_NNNNN_obs.npy (uint8 [30, 64, 64, 3]) and seq_NNNNN_actions.npy ([30, 4]), as the reference's preparation step writes
them. The obs files of a split become ONE raw tensor and the action files one [N, T', 4] array beside it (datasets/base.py); sample i is
obs[:seq_len:seq_step] through the preprocess launch and actions[:seq_len:seq_step] as float32 through the gather launch. Nothing is
downloaded or prepared: the reference's download_and_prepare_dataset (tfrecord) is not part of this build. tools/export_bair_like.py
writes a synthetic directory of this layout for tests and examples.

WHAT DIFFERS FROM THE REFERENCE: `config` carries supports_actions = True (see datasets/base.py), so that an action-conditional model is
accepted on this dataset; the reference's class never sets the key its own compatibility check reads."""
import os

import numpy as np

from .._lib import VpxError
from .base import StoredVPDataset


class BAIRPushingDataset(StoredVPDataset):
    """A robotic gripper arm that randomly moves its end effector inside a bin filled with objects: RGB frames of 64x64 and a 4-D action
    vector per frame."""
    NAME = "BAIR robot pushing"
    REFERENCE = "https://arxiv.org/abs/1710.05268"
    IS_DOWNLOADABLE = "No (prepare the files with the reference's scripts; tools/export_bair_like.py writes a synthetic stand-in)"
    MIN_SEQ_LEN = 30
    ACTION_SIZE = 4
    DATASET_FRAME_SHAPE = (64, 64, 3)

    train_to_val_ratio = 0.96

    def __init__(self, split, **dataset_kwargs):
        super().__init__(split, **dataset_kwargs)
        self.NON_CONFIG_VARS = self.NON_CONFIG_VARS + ["obs_ids", "actions_ids", "obs_fps", "actions_fps"]
        if self.data_dir is None:
            raise VpxError(f"'{self.NAME}' needs data_dir= holding softmotion30_44k/<split>/seq_NNNNN_obs.npy and _actions.npy files. "
                           f"Nothing is downloaded or prepared.")
        self.data_dir = os.path.realpath(os.path.join(str(self.data_dir), "softmotion30_44k", split))
        if not os.path.isdir(self.data_dir):
            raise VpxError(f"'{self.NAME}': no directory {self.data_dir}. Nothing is downloaded or prepared.")
        names = sorted(os.listdir(self.data_dir))
        self.obs_ids = [fn for fn in names if fn.endswith("obs.npy")]
        self.actions_ids = [fn for fn in names if fn.endswith("actions.npy")]
        if len(self.obs_ids) != len(self.actions_ids):
            raise ValueError("Different number of obs and action files found -> Delete dataset and prepare again!")
        elif len(self.obs_ids) == 0:
            raise ValueError("No trajectory files (.npy) found! Maybe you forgot to prepare the dataset?")
        self.obs_fps = [os.path.join(self.data_dir, fn) for fn in self.obs_ids]
        self.actions_fps = [os.path.join(self.data_dir, fn) for fn in self.actions_ids]
        obs, actions = self._read(self.obs_fps), self._read(self.actions_fps)
        if obs.ndim != 5:
            raise ValueError(f"{self.obs_fps[0]}: expected a colour sequence [t, h, w, c], got {obs.shape[1:]}")
        if actions.ndim != 3 or actions.shape[2] != type(self).ACTION_SIZE:
            raise ValueError(f"{self.actions_fps[0]}: expected actions [t, {type(self).ACTION_SIZE}], got {actions.shape[1:]}")
        self._set_raw(obs)
        self._set_actions(actions)
        self.MIN_SEQ_LEN = min(type(self).MIN_SEQ_LEN, int(obs.shape[1]))   # (bair.py:26; never beyond what the files hold)

    @staticmethod
    def _read(paths):
        """The files stacked into one array; one whose shape or dtype differs from the first is refused by name."""
        first = np.load(paths[0])
        out = np.empty((len(paths),) + first.shape, dtype=first.dtype)
        for i, fp in enumerate(paths):
            seq = first if i == 0 else np.load(fp)
            if seq.shape != first.shape or seq.dtype != first.dtype:
                raise ValueError(f"{fp}: {seq.dtype} {seq.shape} differs from the split's first file ({first.dtype} {first.shape})")
            out[i] = seq
        return out

    def origin(self, i):
        return self.obs_fps[i]
