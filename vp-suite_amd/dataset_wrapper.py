"""VPDatasetWrapper (vp_suite/utils/dataset_wrapper.py): handles training / validation data and test data in the same way."""
from .datasets.base import StoredSubset


class VPDatasetWrapper:
    ALLOWED_SPLITS = ["train", "test"]

    def __init__(self, dataset_class, split, **dataset_kwargs):
        if split == "train":
            train_data, val_data = dataset_class.get_train_val(**dataset_kwargs)
            main_data = train_data.dataset if isinstance(train_data, StoredSubset) else train_data
            self.datasets = {"main": main_data, "train": train_data, "val": val_data}
        elif split == "test":
            test_data = dataset_class.get_test(**dataset_kwargs)
            self.datasets = {"main": test_data, "test": test_data}
        else:
            raise ValueError(f"parameter {split} needs to be one of the following: {self.ALLOWED_SPLITS}")
        self.is_ready = False  # set to true after seq_len has been set (pre-requisite for training)

    def __repr__(self):
        return self.__str__()

    def __str__(self):
        return f"DatasetWrapper[{self.NAME}](datasets={self.datasets}, is_ready={self.is_ready})"

    def is_training_set(self):
        return "train" in self.datasets and "val" in self.datasets

    def is_test_set(self):
        return "test" in self.datasets

    def _data(self, key, what):
        data = self.datasets.get(key, None)
        if data is None:
            raise KeyError(f"dataset '{self.NAME}' does not contain {what} data")
        return data

    @property
    def train_data(self):
        return self._data("train", "training")

    @property
    def val_data(self):
        return self._data("val", "validation")

    @property
    def test_data(self):
        return self._data("test", "test")

    @property
    def NAME(self):
        return self.datasets["main"].NAME

    @property
    def data_dir(self):
        return self.datasets["main"].data_dir

    @property
    def action_size(self):
        return self.datasets["main"].ACTION_SIZE

    @property
    def img_shape(self):
        return self.datasets["main"].img_shape

    @property
    def config(self):
        return self.datasets["main"].config

    def _separate_val(self):
        return self.is_training_set() and not isinstance(self.val_data, StoredSubset)

    def set_seq_len(self, context_frames, pred_frames, seq_step):
        """Sets the sequence length of all wrapped datasets (of the validation data too where it is a dataset of its own)."""
        self.datasets["main"].set_seq_len(context_frames, pred_frames, seq_step)
        if self._separate_val():
            self.val_data.set_seq_len(context_frames, pred_frames, seq_step)
        self.is_ready = True

    def reset_rng(self):
        self.datasets["main"].reset_rng()
        if self._separate_val():
            self.val_data.reset_rng()
