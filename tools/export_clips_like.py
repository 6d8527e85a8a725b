"""Writes a small SYNTHETIC tree in one of the two long-clip layouts this build reads, for tests and examples:

    kitti   OUT_DIR/<date>/<drive>/<camera>.npy    [frames, h, w, 3] uint8    DATASET_CLASSES["KITTI"] (datasets/kitti_raw.py)
    cp      OUT_DIR/<setNN>/<Vxxx>.npy             [frames, h, w, 3] uint8    DATASET_CLASSES["CP"]    (datasets/caltech_pedestrian.py)

THIS IS NOT KITTI OR CALTECH DATA: every frame is seeded uniform noise bytes, and a model trained on it learns nothing. The clips differ
in length on purpose (that is what these datasets are about): clip k of n holds min_frames + (k * 7) % (max_frames - min_frames + 1)
frames unless lengths are given. It needs numpy only, no GPU.

    python tools/export_clips_like.py {kitti,cp} OUT_DIR [--clips 6] [--min-frames 12] [--max-frames 30] [--height 16] [--width 24] [--seed 0]"""
import argparse
import os

import numpy as np

CAMERA = "image_02"


def kitti_names(n):
    """n drive directories <date>/<drive> over two dates, in sorted order."""
    return [os.path.join(f"2011_09_{26 + k % 2}", f"2011_09_{26 + k % 2}_drive_{k + 1:04d}_sync") for k in sorted(range(n), key=lambda k: (k % 2, k))]


def cp_names(n):
    """n videos <setNN>/<Vxxx> alternating between the training / validation sets (set00 ...) and the test sets (set06 ...), two thirds
    of them in the former, in sorted order."""
    names = []
    for k in range(n):
        group = k % 3 == 2                                            # every third video is a test video
        idx = k // 3
        names.append(os.path.join(f"set{(6 if group else 0) + idx % (5 if group else 6):02d}", f"V{k:03d}"))
    return sorted(names)


def default_lengths(n, min_frames, max_frames):
    return [min_frames + (k * 7) % (max_frames - min_frames + 1) for k in range(n)]


def synthetic_clip(name, n_frames, hw=(16, 24), seed=0):
    """uint8 [n_frames, h, w, 3] seeded noise: a stream of its own per (seed, clip name)."""
    rng = np.random.default_rng([int(seed)] + [ord(ch) for ch in name])
    return rng.integers(0, 256, size=(n_frames,) + tuple(hw) + (3,), dtype=np.uint8)


def export(layout, out_dir, names, lengths, hw=(16, 24), seed=0, camera=CAMERA):
    """One file per clip, names[k] holding lengths[k] frames. Returns the files written. A file that exists already is refused."""
    if layout not in ("kitti", "cp"):
        raise ValueError(f"layout '{layout}' has to be one of the following: ['kitti', 'cp']")
    written = []
    for name, n_frames in zip(names, lengths):
        fp = os.path.join(out_dir, name, f"{camera}.npy") if layout == "kitti" else os.path.join(out_dir, name + ".npy")
        if os.path.exists(fp):
            raise FileExistsError(fp)
        os.makedirs(os.path.dirname(fp), exist_ok=True)
        np.save(fp, synthetic_clip(name, int(n_frames), hw, seed))
        written.append(fp)
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("layout", choices=["kitti", "cp"])
    ap.add_argument("out_dir")
    ap.add_argument("--clips", type=int, default=6)
    ap.add_argument("--min-frames", type=int, default=12)
    ap.add_argument("--max-frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=16)
    ap.add_argument("--width", type=int, default=24)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    names = kitti_names(args.clips) if args.layout == "kitti" else cp_names(args.clips)
    files = export(args.layout, args.out_dir, names, default_lengths(args.clips, args.min_frames, args.max_frames), (args.height, args.width), args.seed)
    print(f"wrote {len(files)} synthetic clips to {args.out_dir} — seeded noise in the '{args.layout}' layout, this is NOT the dataset")


if __name__ == "__main__":
    main()
