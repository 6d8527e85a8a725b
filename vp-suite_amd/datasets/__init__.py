"""Dataset registry with the reference's keys (vp_suite/datasets/__init__.py) for the datasets this build generates or reads."""
from .bair import BAIRPushingDataset  # noqa: F401
from .base import StoredSubset, StoredVPDataset, VPDataset  # noqa: F401
from .caltech_pedestrian import CaltechPedestrianDataset  # noqa: F401
from .clips import ClipVPDataset  # noqa: F401
from .human36m import Human36MDataset  # noqa: F401
from .kitti_raw import KITTIRawDataset  # noqa: F401
from .mmnist import MovingMNISTDataset  # noqa: F401
from .physics101 import Physics101Dataset  # noqa: F401
from .synpick import SynpickMovingDataset  # noqa: F401
from .mmnist_on_the_fly import MovingMNISTOnTheFly, generate_frames, procedural_digits, read_idx_images  # noqa: F401


class DatasetRegistry(dict):
    """The registry in tiers. LISTED datasets — what iteration, len() and AVAILABLE_DATASETS show — are the ones that produce their
    own frames and so run without a prepared directory. STORED datasets read files a user has to bring (data_dir=); they exist only
    then, so they are not listed, but they are registered: DATASET_CLASSES[key], `key in DATASET_CLASSES` and .get(key) find them.
    `stored` holds the ones whose files carry equal-length sequences of frames only, `stored_with_actions` the ones that carry actions
    beside them, `stored_clips` the ones whose files are long clips that yield many windows each, `stored_video` the clip datasets that need more
    than windowing (frame sizes that differ between videos, one sample per video, actions from stored positions: Human 3.6M, Physics 101,
    SynPick); all are found the same way."""

    def __init__(self, listed, stored, stored_with_actions=(), stored_clips=(), stored_video=()):
        super().__init__(listed)
        self.stored = dict(stored)
        self.stored_with_actions = dict(stored_with_actions)
        self.stored_clips = dict(stored_clips)
        self.stored_video = dict(stored_video)

    def _stored_tiers(self):
        return (self.stored, self.stored_with_actions, self.stored_clips, self.stored_video)

    def __missing__(self, key):
        for tier in self._stored_tiers():
            if key in tier:
                return tier[key]
        raise KeyError(key)

    def __contains__(self, key):
        return super().__contains__(key) or any(key in tier for tier in self._stored_tiers())

    def get(self, key, default=None):
        return self[key] if key in self else default


GENERATED_DATASET_CLASSES = {
    "MMF": MovingMNISTOnTheFly,
}
STORED_DATASET_CLASSES = {
    "MM": MovingMNISTDataset,
}
STORED_ACTION_DATASET_CLASSES = {
    "BAIR": BAIRPushingDataset,
}
STORED_CLIP_DATASET_CLASSES = {
    "KITTI": KITTIRawDataset,
    "CP": CaltechPedestrianDataset,
}
STORED_VIDEO_DATASET_CLASSES = {
    "H36M": Human36MDataset,
    "P101": Physics101Dataset,
    "SPM": SynpickMovingDataset,
}
DATASET_CLASSES = DatasetRegistry(GENERATED_DATASET_CLASSES, STORED_DATASET_CLASSES, STORED_ACTION_DATASET_CLASSES, STORED_CLIP_DATASET_CLASSES,
                                  STORED_VIDEO_DATASET_CLASSES)
AVAILABLE_DATASETS = DATASET_CLASSES.keys()
