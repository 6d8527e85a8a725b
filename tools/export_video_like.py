"""Writes a small SYNTHETIC tree in one of the three video layouts this build reads, for tests and examples:

    h36m    OUT_DIR/{training,testing}/<subject>/Videos/<Scenario ...>.npy   [frames, h, w, 3] uint8   DATASET_CLASSES["H36M"] (datasets/human36m.py)
    p101    OUT_DIR/<scenario>/<object>/<trial>/<camera>.npy                 [frames, h, w, 3] uint8   DATASET_CLASSES["P101"] (datasets/physics101.py)
    spm     OUT_DIR/processed/<split>/<episode>.npy                          [frames, h, w, 3] uint8   DATASET_CLASSES["SPM"]  (datasets/synpick.py)
            OUT_DIR/processed/<split>/<episode>_gripper.npy                  [frames, 3] float64

THIS IS NOT HUMAN 3.6M, PHYSICS 101 OR SYNPICK DATA: every frame is seeded uniform noise bytes and every gripper track a seeded random
walk; a model trained on it learns nothing. Videos of one tree may differ in length and, for h36m, in frame size (every third video is
two rows taller, as the real 1002 x 1000 videos are). It needs numpy only, no GPU.

    python tools/export_video_like.py {h36m,p101,spm} OUT_DIR [--clips 6] [--min-frames 40] [--max-frames 60] [--height 16] [--width 24] [--seed 0]"""
import argparse
import os

import numpy as np

CAMERA = "Kinect_RGB_1"
SCENARIOS = ["Directions", "WalkingDog"]


def h36m_names(n):
    """n videos <split dir>/<subject>/Videos/<Scenario k.camera>, every fourth one a test video and the scenario changing every four, in sorted
    order (by path components)."""
    return sorted(os.path.join("testing" if k % 4 == 3 else "training", f"S{1 + k % 3}", "Videos", f"{SCENARIOS[(k // 4) % len(SCENARIOS)]} {k}.5501{k:04d}")
                  for k in range(n))   # (no name is a prefix of a directory name here: string order is component order)


def p101_names(n):
    """n trial directories <scenario>/<object>/<trial>, in sorted order."""
    return sorted(os.path.join(("ramp", "spring", "fall")[k % 3], f"object_{k % 2}", f"trial_{k:02d}") for k in range(n))


def spm_names(n, split="train"):
    """n episodes <split>/<6-digit episode number>, in sorted order."""
    return [os.path.join(split, f"{k:06d}") for k in range(n)]


def default_lengths(n, min_frames, max_frames):
    return [min_frames + (k * 7) % (max_frames - min_frames + 1) for k in range(n)]


def synthetic_clip(name, n_frames, hw=(16, 24), seed=0):
    """uint8 [n_frames, h, w, 3] seeded noise: a stream of its own per (seed, clip name)."""
    rng = np.random.default_rng([int(seed)] + [ord(ch) for ch in name])
    return rng.integers(0, 256, size=(n_frames,) + tuple(hw) + (3,), dtype=np.uint8)


def synthetic_gripper(name, n_frames, seed=0, step=4.0):
    """float64 [n_frames, 3]: a seeded random walk whose xy steps are `step` long on average (the window rule wants most of them above
    1.0 and all below 30.0) and whose height drifts slowly."""
    rng = np.random.default_rng([int(seed), 1] + [ord(ch) for ch in name])
    angle = rng.uniform(0.0, 2.0 * np.pi, size=n_frames)
    length = rng.uniform(0.5 * step, 1.5 * step, size=n_frames)
    steps = np.stack([length * np.cos(angle), length * np.sin(angle), rng.normal(0.0, 0.1, size=n_frames)], axis=1)
    return np.cumsum(steps, axis=0) + np.array([0.0, 0.0, 1000.0])


def export(layout, out_dir, names, lengths, hw=(16, 24), seed=0, camera=CAMERA, sizes=None, grippers=None):
    """One file per clip, names[k] holding lengths[k] frames of sizes[k] (default: hw) pixels; for spm also the gripper file, from
    grippers[k] if given. Returns the clip files written. A file that exists already is refused."""
    if layout not in ("h36m", "p101", "spm"):
        raise ValueError(f"layout '{layout}' has to be one of the following: ['h36m', 'p101', 'spm']")
    written = []
    for k, (name, n_frames) in enumerate(zip(names, lengths)):
        fp = {"h36m": os.path.join(out_dir, name + ".npy"), "p101": os.path.join(out_dir, name, f"{camera}.npy"),
              "spm": os.path.join(out_dir, "processed", name + ".npy")}[layout]
        if os.path.exists(fp):
            raise FileExistsError(fp)
        os.makedirs(os.path.dirname(fp), exist_ok=True)
        np.save(fp, synthetic_clip(name, int(n_frames), hw if sizes is None else sizes[k], seed))
        if layout == "spm":
            gripper = synthetic_gripper(name, int(n_frames), seed) if grippers is None else np.asarray(grippers[k])
            assert gripper.shape == (int(n_frames), 3), gripper.shape
            np.save(fp[:-len(".npy")] + "_gripper.npy", gripper)
        written.append(fp)
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("layout", choices=["h36m", "p101", "spm"])
    ap.add_argument("out_dir")
    ap.add_argument("--clips", type=int, default=6)
    ap.add_argument("--min-frames", type=int, default=40)
    ap.add_argument("--max-frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=16)
    ap.add_argument("--width", type=int, default=24)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    hw = (args.height, args.width)
    lengths = default_lengths(args.clips, args.min_frames, args.max_frames)
    if args.layout == "h36m":
        files = export("h36m", args.out_dir, h36m_names(args.clips), lengths, hw, args.seed,
                       sizes=[(hw[0] + 2 * (k % 3 == 2), hw[1]) for k in range(args.clips)])
    elif args.layout == "p101":
        files = export("p101", args.out_dir, p101_names(args.clips), lengths, hw, args.seed)
    else:
        files = []
        for split in ("train", "val", "test"):
            files += export("spm", args.out_dir, spm_names(args.clips, split), [72 + n for n in lengths], hw, args.seed)
    print(f"wrote {len(files)} synthetic clips to {args.out_dir} — seeded noise in the '{args.layout}' layout, this is NOT the dataset")


if __name__ == "__main__":
    main()
