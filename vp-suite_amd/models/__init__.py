"""Model registry with the reference's keys (vp_suite/models/__init__.py:14-26) for the models on the hot path, the copy baseline, and "nc-lstm":
the NonConvLSTM model under a key of its own (the reference's "lstm" computes decode(zeros); see models/lstm.py)."""
from .copy_last_frame import CopyLastFrame  # noqa: F401
from .ef_conv_lstm import EF_ConvLSTM, Encoder_Forecaster  # noqa: F401
from .ef_traj_gru import EF_TrajGRU  # noqa: F401
from .lstm import LSTM  # noqa: F401
from .phydnet import PhyDNet  # noqa: F401
from .predrnn_v2 import PredRNN_V2  # noqa: F401
from .st_phy import STPhy  # noqa: F401
from .unet3d import UNet3D  # noqa: F401

MODEL_CLASSES = {
    "convlstm-shi": EF_ConvLSTM,
    "predrnn-pp": PredRNN_V2,
    "trajgru": EF_TrajGRU,
    "phy": PhyDNet,
    "st-phy": STPhy,
    "unet-3d": UNet3D,
    "nc-lstm": LSTM,   # (the reference's key "lstm" stays invalid: models/lstm.py)
    "copy": CopyLastFrame,
}
AVAILABLE_MODELS = MODEL_CLASSES.keys()
