"""Writes tests/golden/mm_stored.npz from the upstream reference's file-backed MovingMNISTDataset on the CPU (tools/ref_shim.py; build
container only, never imported by a test).

Three gray sequences [6, 12, 10] of seeded bytes (0 and 255 among them) are written as seq_NNNNN.npy into a temporary directory; the
reference class reads them unchanged, with an explicit data_dir. After set_seq_len(2, 1, 2) — frames 0, 2, 4 — the npz holds
  raw              uint8 [3, 6, 12, 10], the bytes of the files
  frames_01        float32 [3, 3, 12, 10]: channel 0 of the three samples at value range (0, 1) (the three channels are asserted equal)
  frames_11        the same at value_range_min = -1.0
  post_in          float32 [2, 3, 5, 7] that leaves the range (-1, 1) on both sides
  post_01/post_11  uint8 [2, 5, 7, 3]: the reference's postprocess() of post_in at either range
  split_train / split_val   the `indices` of both halves of get_train_val() over 25 files
Under the shim torchvision is a mock, so the reference cannot run its Resize: the resize path has no fixture from it
(tests/test_frames_host.py pins it to torch.nn.functional.interpolate instead).

    python tools/gen_golden_mm.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from golden_util import GOLDEN_DIR  # noqa: E402


def write_split(root, split, raw):
    os.makedirs(os.path.join(root, split))
    for i, seq in enumerate(raw):
        np.save(os.path.join(root, split, f"seq_{i:05d}.npy"), seq)


def main():
    import torch
    ref_shim.load_reference()
    from vp_suite.datasets.mmnist import MovingMNISTDataset
    rng = np.random.default_rng(20240607)
    raw = rng.integers(0, 256, size=(3, 6, 12, 10), dtype=np.uint8)
    raw[0, 0, 0, :4] = (0, 255, 1, 254)
    arrays = {"raw": raw}
    post_in = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(2, 3, 5, 7)).astype(np.float32))
    arrays["post_in"] = post_in.numpy().copy()
    with tempfile.TemporaryDirectory() as tmp:
        write_split(tmp, "train", raw)
        for tag, kwargs in (("01", {}), ("11", {"value_range_min": -1.0})):
            ds = MovingMNISTDataset("train", data_dir=tmp, **kwargs)
            assert len(ds) == 3 and ds.MIN_SEQ_LEN == 6
            ds.set_seq_len(2, 1, 2)
            frames = []
            for i in range(3):
                data = ds[i]
                f = data["frames"].numpy()
                assert f.dtype == np.float32 and f.shape == (3, 3, 12, 10) and tuple(data["actions"].shape) == (3, 1)
                assert np.array_equal(f[:, 0], f[:, 1]) and np.array_equal(f[:, 0], f[:, 2])
                frames.append(f[:, 0].copy())
            arrays[f"frames_{tag}"] = np.stack(frames)
            arrays[f"post_{tag}"] = ds.postprocess(post_in.clone())
            assert arrays[f"post_{tag}"].dtype == np.uint8 and arrays[f"post_{tag}"].shape == (2, 5, 7, 3)
    with tempfile.TemporaryDirectory() as tmp:
        write_split(tmp, "train", np.zeros((25, 2, 4, 4), dtype=np.uint8))
        train, val = MovingMNISTDataset.get_train_val(data_dir=tmp)
        arrays["split_train"], arrays["split_val"] = np.array(train.indices, dtype=np.int64), np.array(val.indices, dtype=np.int64)
        assert len(train) == 24 and len(val) == 1
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    path = os.path.join(GOLDEN_DIR, "mm_stored.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  wrote mm_stored.npz  ({size / 1024:.1f} KiB)")
    assert size <= 200 * 1024


if __name__ == "__main__":
    main()
