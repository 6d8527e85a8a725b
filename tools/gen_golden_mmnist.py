"""Writes tests/golden/mmnist_otf.npz from the upstream reference's MovingMNISTOnTheFly on the CPU (tools/ref_shim.py; build container
only, never imported by a test).

Under the shim torchvision is a mock, so the name `MNIST` inside the reference's mmnist_on_the_fly module is replaced by a stub that
serves procedural_digits() — the reference class itself runs unchanged, at its defaults (3 x 64 x 64), with an explicit data_dir.
After set_seq_len(3, 2, 1), three samples each of
  test    the `test` split, value range (0, 1)
  train   the `train` split, value_range_min = -1.0
The three channels are asserted equal and channel 0 is kept: frames_<cfg> float32 [3, 5, 64, 64]. params_<cfg> int32 [3, 2, 5] holds the
rows (glyph index, y0, x0, vy, vx) the class drew, recorded at its own sampling calls; glyphs uint8 [16, 28, 28] is the table served.

    python tools/gen_golden_mmnist.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from golden_util import GOLDEN_DIR  # noqa: E402

N_SAMPLES = 3
CONFIGS = {"test": ("test", {}), "train": ("train", {"value_range_min": -1.0})}


def main():
    from vp_suite_amd.datasets import procedural_digits
    glyphs = procedural_digits()

    class StubMNIST:   # what the reference uses of torchvision.datasets.MNIST: len() and [i][0], an image np.array() accepts
        def __init__(self, root, train, download):
            assert download is False

        def __len__(self):
            return len(glyphs)

        def __getitem__(self, i):
            return glyphs[i], 0

    ref_shim.load_reference()
    import vp_suite.datasets.mmnist_on_the_fly as ref_mod
    ref_mod.MNIST = StubMNIST
    arrays = {"glyphs": glyphs}
    for tag, (split, kwargs) in CONFIGS.items():
        ds = ref_mod.MovingMNISTOnTheFly(split, data_dir="unused", **kwargs)
        assert ds.img_shape == (3, 64, 64) and ds.num_digits == 2
        ds.set_seq_len(3, 2, 1)
        rows, indices = [], []
        draw_index, sample = ds.get_digit_id, ds._sample_digit

        def get_digit_id():
            indices.append(int(draw_index()))
            return indices[-1]

        def sample_digit():
            digit, pos, speed, size = sample()
            assert size == glyphs.shape[1]
            rows.append([indices[-1], int(pos[0]), int(pos[1]), int(speed[0]), int(speed[1])])   # pos, speed: (y, x)
            return digit, pos, speed, size
        ds.get_digit_id, ds._sample_digit = get_digit_id, sample_digit
        frames = []
        for i in range(N_SAMPLES):
            data = ds[i]
            f = data["frames"].numpy()
            assert f.dtype == np.float32 and f.shape == (5, 3, 64, 64) and tuple(data["actions"].shape) == (5, 1)
            assert np.array_equal(f[:, 0], f[:, 1]) and np.array_equal(f[:, 0], f[:, 2])
            frames.append(f[:, 0].copy())
        arrays[f"frames_{tag}"] = np.stack(frames)
        arrays[f"params_{tag}"] = np.array(rows, dtype=np.int32).reshape(N_SAMPLES, 2, 5)
        print(f"  {tag}: value range [{arrays[f'frames_{tag}'].min()}, {arrays[f'frames_{tag}'].max()}], rows\n{arrays[f'params_{tag}']}")
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    path = os.path.join(GOLDEN_DIR, "mmnist_otf.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  wrote mmnist_otf.npz  ({size / 1024:.1f} KiB)")
    assert size <= 400 * 1024


if __name__ == "__main__":
    main()
