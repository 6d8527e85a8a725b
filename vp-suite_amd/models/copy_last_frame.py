"""CopyLastFrame (vp_suite/models/copy_last_frame.py, registry key "copy"): the non-trainable baseline VPSuite.test() appends to every
test set. Pure indexing, so it has no kernel and runs on host tensors too."""
from ..base import VPModel
from ..utils import get_public_attrs


class CopyLastFrame(VPModel):
    """Returns the latest frame as the next predicted frame."""
    NAME = "CopyLastFrame"
    REQUIRED_ARGS = []
    TRAINABLE = False

    def __init__(self, device=None, **model_kwargs):
        super().__init__(device, **model_kwargs)

    @property
    def config(self):
        """As VPModel.config, for a model that may have been given no img_shape (REQUIRED_ARGS is empty): img_h / img_w / img_c are None then."""
        attrs = get_public_attrs(self, "config", non_config_vars=self.NON_CONFIG_VARS, model_mode=True)
        c, h, w = self.img_shape if self.img_shape is not None else (None, None, None)
        attrs.update({"img_h": h, "img_w": w, "img_c": c, "NAME": self.NAME})
        return attrs

    def pred_1(self, x, **kwargs):
        return x[:, -1, :, :, :]

    def forward(self, x, pred_frames: int = 1, **kwargs):
        """pred_frames copies of the last frame: the values the base class's pred_1 loop yields (each prediction becomes the last frame
        of the next input), without its chain of concatenations."""
        last = self.pred_1(x, **kwargs).unsqueeze(dim=1)
        return last.expand(-1, pred_frames, -1, -1, -1).contiguous(), None
