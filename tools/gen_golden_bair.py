"""Writes tests/golden/bair_stored.npz from the upstream reference's BAIRPushingDataset on the CPU (tools/ref_shim.py, which also stands in
for the `tfrecord` modules the reference's bair.py imports at its top; build container only, never imported by a test).

Three synthetic sequences from tools/export_bair_like.py — 30 frames of 8 x 8 x 3 noise bytes, float64 actions, NOT BAIR data — are
written in BAIR's layout into a temporary directory; the first action row is replaced by values float32 cannot hold (a tie, a value next
to the largest float32). The reference class reads them unchanged, with an explicit data_dir. The npz holds
  obs             uint8 [3, 30, 8, 8, 3], the bytes of the obs files
  actions         float64 [3, 30, 4], the action files
  frames_s1 / actions_s1   float32 [3, 5, 3, 8, 8] / [3, 5, 4]: the three samples after set_seq_len(3, 2, 1)
  frames_s2 / actions_s2   the same after set_seq_len(3, 2, 2): stored rows 0, 2, 4, 6, 8

    python tools/gen_golden_bair.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import export_bair_like  # noqa: E402
import ref_shim  # noqa: E402
from golden_util import GOLDEN_DIR  # noqa: E402

F32_MAX = float(np.finfo(np.float32).max)
SPECIAL = [1.0 + 2.0 ** -24, -(1.0 + 3.0 * 2.0 ** -24), F32_MAX * (1.0 - 2.0 ** -26), 0.1]   # tie to even (down), tie to even (up), rounds to max, inexact


def main():
    ref_shim.load_reference()
    from vp_suite.datasets.bair import BAIRPushingDataset
    obs, actions = export_bair_like.synthetic_split(3, 30, 8, seed=20241019, split="train", actions_dtype=np.float64)
    actions[0, 0] = SPECIAL
    arrays = {"obs": obs, "actions": actions}
    with tempfile.TemporaryDirectory() as tmp:
        target = export_bair_like.write_split(tmp, "train", obs, actions)
        ds = BAIRPushingDataset("train", data_dir=tmp)
        assert len(ds) == 3 and (ds.MIN_SEQ_LEN, ds.ACTION_SIZE, ds.NAME) == (30, 4, "BAIR robot pushing")
        for step in (1, 2):
            ds.set_seq_len(3, 2, step)
            frames, acts = [], []
            for i in range(3):
                data = ds[i]
                f, a = data["frames"].numpy(), data["actions"].numpy()
                assert f.dtype == np.float32 and f.shape == (5, 3, 8, 8) and a.dtype == np.float32 and a.shape == (5, 4)
                assert data["origin"] == os.path.join(os.path.realpath(target), f"seq_{i:05d}_obs.npy")
                frames.append(f.copy())
                acts.append(a.copy())
            arrays[f"frames_s{step}"], arrays[f"actions_s{step}"] = np.stack(frames), np.stack(acts)
    print(f"  special row as float32: {arrays['actions_s1'][0, 0].tolist()}")
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    path = os.path.join(GOLDEN_DIR, "bair_stored.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  wrote bair_stored.npz  ({size / 1024:.1f} KiB)")
    assert size <= 100 * 1024


if __name__ == "__main__":
    main()
