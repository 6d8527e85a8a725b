"""Dataset base class with the reference's surface (vp_suite/base/base_dataset.py), as far as a dataset that is generated on the GPU
uses it: split handling, set_seq_len() and its sequence-length rule, the value range, `config`. Frames are produced at their final size
and value range by the generating kernel, so there is no preprocess() chain: `crop` and `augmentations` are refused."""
from torch.utils.data import Dataset

from ..utils import get_public_attrs, set_from_kwarg


class VPDataset(Dataset):
    """Not usable directly after creation: set_seq_len() fixes the sequence length first (base_dataset.py:47-51)."""
    NON_CONFIG_VARS = ["functions", "ready_for_usage", "total_frames", "seq_len", "frame_offsets", "data_dir"]

    NAME: str = NotImplemented
    REFERENCE: str = None
    IS_DOWNLOADABLE: str = None
    ON_THE_FLY: bool = False
    VALID_SPLITS = ["train", "test"]
    MIN_SEQ_LEN: int = NotImplemented
    ACTION_SIZE: int = NotImplemented
    DATASET_FRAME_SHAPE = NotImplemented   # (h, w, c)

    img_shape = NotImplemented             # (c, h, w) of a returned frame
    split: str = None
    seq_step: int = 1
    data_dir: str = None
    value_range_min: float = 0.0
    value_range_max: float = 1.0

    def __init__(self, split: str, **dataset_kwargs):
        super().__init__()
        if split not in self.VALID_SPLITS:
            raise ValueError(f"parameter '{split}' has to be one of the following: {self.VALID_SPLITS}")
        self.split = split
        set_from_kwarg(self, dataset_kwargs, "seq_step")
        self.data_dir = dataset_kwargs.get("data_dir", self.data_dir)
        set_from_kwarg(self, dataset_kwargs, "value_range_min")
        set_from_kwarg(self, dataset_kwargs, "value_range_max")
        if dataset_kwargs.get("crop") is not None or dataset_kwargs.get("augmentations"):
            raise NotImplementedError("'crop' and 'augmentations' are not part of this build: frames are generated at their final size")
        self.ready_for_usage = False   # True once the sequence length has been set

    @property
    def config(self) -> dict:
        """The dataset's configuration: its public attributes plus the keys every model reads (base_dataset.py:147-163)."""
        attrs = get_public_attrs(self, "config", non_config_vars=self.NON_CONFIG_VARS)
        img_c, img_h, img_w = self.img_shape
        return {**attrs, "img_h": img_h, "img_w": img_w, "img_c": img_c, "action_size": self.ACTION_SIZE,
                "tensor_value_range": [self.value_range_min, self.value_range_max], "NAME": self.NAME}

    def set_seq_len(self, context_frames: int, pred_frames: int, seq_step: int):
        """seq_len = (context_frames + pred_frames - 1) * seq_step + 1 (base_dataset.py:165-187)."""
        total_frames = context_frames + pred_frames
        seq_len = (total_frames - 1) * seq_step + 1
        if self.MIN_SEQ_LEN < seq_len:
            raise ValueError(f"Dataset '{self.NAME}' supports videos with up to {self.MIN_SEQ_LEN} frames, which is exceeded by your configuration: "
                             f"{{context frames: {context_frames}, pred frames: {pred_frames}, seq step: {seq_step}}}")
        self.total_frames = total_frames
        self.seq_len = seq_len
        self.seq_step = seq_step
        self.frame_offsets = range(0, total_frames * seq_step, seq_step)
        self.ready_for_usage = True

    def reset_rng(self):
        pass

    def __len__(self) -> int:
        raise NotImplementedError

    def __getitem__(self, i):
        raise NotImplementedError
