"""Dataset registry with the reference's keys (vp_suite/datasets/__init__.py) for the datasets this build generates or reads."""
from .base import VPDataset  # noqa: F401
from .mmnist_on_the_fly import MovingMNISTOnTheFly, generate_frames, procedural_digits, read_idx_images  # noqa: F401

DATASET_CLASSES = {
    "MMF": MovingMNISTOnTheFly,
}
AVAILABLE_DATASETS = DATASET_CLASSES.keys()
