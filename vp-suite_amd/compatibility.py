"""Compatibility checks between a model, a dataset and a run configuration (vp_suite/utils/compatibility.py), restated literally, and the
adapter that bridges a model and a test set which differ in value range or frame size.

Where the reference chains ScaleToModel / ScaleToTest (utils/models.py:7-64) and TF.Resize inside an nn.Sequential — up to four ATen passes
over every frame on the way into and out of every model — this build returns ONE FrameAdapter per direction, whose forward is one
ops.frames_adapt call (csrc/adapt.hip: scale first, then resize, fused in one launch). When nothing differs both are nn.Identity(): no
launch at all.

The resize is bilinear with align_corners=False and NO antialiasing: what the reference's pinned torchvision does to tensors (newer
torchvision antialiases by default), and what the dataset resize of this build does (datasets/base.py)."""
import warnings

from torch import nn

from . import ops


class FrameAdapter(nn.Module):
    """Maps frames [..., c, h, w] from src_range to dst_range and, if out_hw is not None, resizes them to it: one HIP launch."""

    def __init__(self, src_range, dst_range, out_hw=None):
        super().__init__()
        self.src_range = tuple(float(v) for v in src_range)
        self.dst_range = tuple(float(v) for v in dst_range)
        self.out_hw = None if out_hw is None else tuple(int(v) for v in out_hw)

    def extra_repr(self):
        return f"src_range={self.src_range}, dst_range={self.dst_range}, out_hw={self.out_hw}"

    def forward(self, img):
        return ops.frames_adapt(img, self.out_hw, self.src_range, self.dst_range)


def check_model_and_data_compat(model, dataset, strict_mode=False):
    """Checks a model against a dataset (a VPDataset or a VPDatasetWrapper). Returns (preprocessing, postprocessing): modules that bridge a
    differing value range and / or frame size — preprocessing maps test frames to the model's format, postprocessing maps predictions
    back — or two nn.Identity() when nothing differs. In strict mode (training) such a difference raises ValueError instead. A channel
    mismatch, an action-conditional model on a dataset without actions and unequal action sizes always raise ValueError."""
    model_config = model.config
    dataset_config = dataset.config
    model_dir_str = f"(location: {model.model_dir})"

    # tensor value range
    model_value_range = list(model_config["tensor_value_range"])
    test_value_range = list(dataset_config["tensor_value_range"])
    ranges_differ = model_value_range != test_value_range
    if ranges_differ and strict_mode:
        raise ValueError("Model and run value ranges differ")

    # img_shape
    model_c, model_h, model_w = model_config["img_shape"]
    test_c, test_h, test_w = dataset_config["img_shape"]
    sizes_differ = False
    if model_c != test_c:
        raise ValueError(f"Test dataset provides {test_c}-channel images but "
                         f"Model '{model.NAME}' {model_dir_str} expects {model_c} channels")
    elif model_h != test_h or model_w != test_w:
        if strict_mode:
            raise ValueError("Model and run img sizes differ")
        sizes_differ = True

    # actions
    if model.CAN_HANDLE_ACTIONS and model_config["action_conditional"]:
        if not dataset_config.get("supports_actions", False):   # (no dataset of the reference sets the key: read as "no actions")
            raise ValueError("Can't train action-conditional model on a dataset that doesn't provide actions.")
        if model_config["action_size"] != dataset_config["action_size"]:
            raise ValueError("Action size of action-conditional model and dataset must be equal")

    # finalize pre-/postprocessing modules: scale and resize fused, one module (one launch) per direction
    if not (ranges_differ or sizes_differ):
        return nn.Identity(), nn.Identity()
    model_preprocessing = FrameAdapter(test_value_range, model_value_range, (model_h, model_w) if sizes_differ else None)
    model_postprocessing = FrameAdapter(model_value_range, test_value_range, (test_h, test_w) if sizes_differ else None)
    return model_preprocessing, model_postprocessing


def check_run_and_model_compat(model, run_config: dict):
    """Checks a model's configuration against the run configuration; raises ValueError on a critical inconsistency.

    Restated literally, including the reference's `elif` chain (compatibility.py:79-95): the MIN_CONTEXT_FRAMES check is the LAST branch of
    the chain that starts with `if model.CAN_HANDLE_ACTIONS`, so it is made only for models that cannot handle actions, and only when the
    run does not use actions (with use_actions=True such a model gets the warning instead)."""
    model_config = model.config
    model_dir_str = f"(location: {model.model_dir})"

    # action conditioning
    mdl_ac, run_ac = model_config["action_conditional"], run_config["use_actions"]
    if model.CAN_HANDLE_ACTIONS:
        if mdl_ac:
            if not run_ac:
                raise ValueError(f"Action-conditioned model '{model.NAME}' {model_dir_str}"
                                 f"can't be invoked without using actions -> set 'use_actions' to True in test cfg!")
        elif run_ac:
            raise ValueError(f"Action-conditionable model '{model.NAME}' {model_dir_str}"
                             f"was trained without using actions -> set 'use_actions' to False in test cfg!")
    elif run_ac:
        warnings.warn(f"Model '{model.NAME}' {model_dir_str} can't handle actions "
                      f"-> Testing it without using the actions provided by the dataset")

    # context frames and pred. horizon
    elif run_config["context_frames"] < model.MIN_CONTEXT_FRAMES:
        raise ValueError(f"Model '{model.NAME}' {model_dir_str} needs at least "
                         f"{model.MIN_CONTEXT_FRAMES} context frames as it uses temporal convolution "
                         f"with said number as kernel size")
