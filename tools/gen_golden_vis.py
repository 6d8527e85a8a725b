"""Writes tests/golden/vis_layout.npz from the upstream reference's own visualization functions on the CPU (tools/ref_shim.py; build
container only, never imported by a test).

The inputs are the seeded byte sequences of tests/vis_ref.py (fixture_inputs: GT, Pred, seg_x, uint8 [5, 16, 24, 3], context 2), which
the tests regenerate; the npz holds the reference's OUTPUTS only:
  bordered_GT / bordered_Pred / bordered_seg_x   uint8 [5, 20, 28, 3]: add_borders() of the three sequences
  sheet                                          uint8 [52, 130, 3]: the image save_frame_compare_img() hands to cv2.imwrite, for the
                                                 ground truth GT, the predictions Pred and seg_x and vis_context_frame_idx = [0, 1]
cv2 is not installed: it is replaced by an object whose cvtColor flips the channel order and whose imwrite records the array with the
flip undone, so what is recorded is the RGB image the reference composed. matplotlib is stubbed when it cannot be imported.

    python tools/gen_golden_vis.py"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
import vis_ref  # noqa: E402
from golden_util import GOLDEN_DIR  # noqa: E402


class RecordingCV2:
    """Stands in for cv2: records what imwrite is handed, in RGB order."""
    COLOR_RGB2BGR = "rgb2bgr"

    def __init__(self):
        self.written = {}

    def cvtColor(self, img, code):
        assert code == self.COLOR_RGB2BGR
        return img[..., ::-1]

    def imwrite(self, filename, img):
        self.written[filename] = np.ascontiguousarray(np.asarray(img)[..., ::-1])
        return True


def main():
    cv2 = RecordingCV2()
    sys.modules["cv2"] = cv2
    for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.animation"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = MagicMock(name=name)
    ref_shim.load_reference()
    from vp_suite.utils import visualization as ref_vis
    inputs = vis_ref.fixture_inputs()
    arrays = {}
    out = ref_vis.add_borders({k: v.copy() for k, v in inputs.items()}, vis_ref.FIXTURE_CONTEXT)
    for name, vid in out.items():
        assert vid.dtype == np.uint8 and vid.shape == (5, 20, 28, 3), (name, vid.dtype, vid.shape)
        arrays[f"bordered_{name}"] = vid
    ref_vis.save_frame_compare_img("sheet.png", vis_ref.FIXTURE_CONTEXT, inputs["GT"].copy(), [inputs["Pred"].copy(), inputs["seg_x"].copy()],
                                   vis_ref.FIXTURE_SHEET_IDX)
    (arrays["sheet"],) = cv2.written.values()
    assert arrays["sheet"].dtype == np.uint8 and arrays["sheet"].shape == (52, 130, 3), arrays["sheet"].shape
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    path = os.path.join(GOLDEN_DIR, "vis_layout.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  wrote vis_layout.npz  ({size / 1024:.1f} KiB)")
    assert size <= 200 * 1024


if __name__ == "__main__":
    main()
