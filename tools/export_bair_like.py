"""Writes a small SYNTHETIC directory in the layout of the prepared BAIR robot pushing dataset
(out_dir/softmotion30_44k/<split>/seq_NNNNN_obs.npy, uint8 [frames, h, w, 3], and seq_NNNNN_actions.npy, [frames, 4]: what
vp_suite/datasets/bair.py split_bair_traj_files leaves behind) for tests and examples. DATASET_CLASSES["BAIR"] reads such a directory.

THIS IS NOT BAIR DATA: the frames are seeded uniform noise bytes and the actions seeded normal draws. Nothing here shows a robot, and a
model trained on it learns nothing. It needs numpy only, no GPU.

    python tools/export_bair_like.py OUT_DIR [--train 24] [--test 6] [--frames 30] [--img-size 64] [--seed 0] [--actions-dtype float32]"""
import argparse
import os

import numpy as np

ACTION_SIZE = 4
SPLIT_SEEDS = {"train": 0, "test": 1}


def synthetic_split(n_seqs, n_frames=30, img_size=64, seed=0, split="train", actions_dtype=np.float32):
    """(obs uint8 [n, frames, h, w, 3], actions [n, frames, 4]) of one split: seeded noise, a stream of its own per (seed, split)."""
    rng = np.random.default_rng([int(seed), SPLIT_SEEDS[split]])
    h, w = (img_size, img_size) if isinstance(img_size, int) else img_size
    obs = rng.integers(0, 256, size=(n_seqs, n_frames, h, w, 3), dtype=np.uint8)
    actions = rng.standard_normal(size=(n_seqs, n_frames, ACTION_SIZE)).astype(actions_dtype)
    return obs, actions


def write_split(out_dir, split, obs, actions):
    """One file pair per sequence below out_dir/softmotion30_44k/<split>, which must not exist yet. Returns that directory."""
    target = os.path.join(out_dir, "softmotion30_44k", split)
    os.makedirs(target)
    for i in range(len(obs)):
        np.save(os.path.join(target, f"seq_{i:05d}_obs.npy"), obs[i])
        np.save(os.path.join(target, f"seq_{i:05d}_actions.npy"), actions[i])
    return target


def export(out_dir, counts, n_frames=30, img_size=64, seed=0, actions_dtype=np.float32):
    """counts: {"train": n, "test": m}. Returns the number of sequences written. A split directory that exists already is refused."""
    written = 0
    for split, n_seqs in counts.items():
        if n_seqs < 1:
            continue
        write_split(out_dir, split, *synthetic_split(n_seqs, n_frames, img_size, seed, split, actions_dtype))
        written += n_seqs
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out_dir")
    ap.add_argument("--train", type=int, default=24)
    ap.add_argument("--test", type=int, default=6)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--actions-dtype", choices=["float32", "float64"], default="float32")
    args = ap.parse_args()
    n = export(args.out_dir, {"train": args.train, "test": args.test}, args.frames, args.img_size, args.seed, np.dtype(args.actions_dtype))
    print(f"wrote {n} synthetic sequences of {args.frames} frames to {args.out_dir} — seeded noise in BAIR's layout, this is NOT BAIR data")


if __name__ == "__main__":
    main()
