"""Writes a Moving MNIST directory in the reference's file format (data_dir/<split>/seq_NNNNN.npy, one gray uint8 sequence [t, h, w]
each: vp_suite/datasets/mmnist.py save_generated_mmnist) from the generator this package already has: batches of
DATASET_CLASSES["MMF"] at one channel and value range (0, 1), turned into bytes by ops.frames_postprocess on the GPU.
DATASET_CLASSES["MM"] reads such a directory. The trajectories are the on-the-fly generator's (integer speeds, its bounce rule), not
those of the reference's preparation script.

Glyphs: --mnist-dir with MNIST's raw idx files (train-images-idx3-ubyte for "train", t10k-images-idx3-ubyte for "test"). Without it
procedural_digits() is drawn — seven-segment stand-ins, NOT MNIST — and the tool says so.

    python tools/export_mmnist.py OUT_DIR [--train 9600] [--test 1000] [--frames 20] [--img-size 64] [--mnist-dir DIR] [--batch 256]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def export(out_dir, counts, n_frames=20, glyphs=None, mnist_dir=None, img_size=64, batch_size=256):
    """counts: {"train": n, "test": m}. Returns the number of files written. A split directory that exists already is refused."""
    import vp_suite_amd
    from vp_suite_amd import ops
    from vp_suite_amd.datasets import DATASET_CLASSES
    written = 0
    for split, n_seqs in counts.items():
        if n_seqs < 1:
            continue
        kw = {"digits": glyphs} if glyphs is not None else {"data_dir": mnist_dir}
        gen = DATASET_CLASSES["MMF"](split, img_size=img_size, num_channels=1, n_seqs=n_seqs, **kw)
        gen.set_seq_len(n_frames, 0, 1)
        target = os.path.join(out_dir, split)
        os.makedirs(target)
        for start in range(0, n_seqs, batch_size):
            frames = gen.batch(min(batch_size, n_seqs - start))["frames"]             # [n, t, 1, h, w] in (0, 1)
            data = ops.frames_postprocess(frames, 0.0, 1.0).cpu().numpy()[..., 0]      # [n, t, h, w] bytes
            for k, seq in enumerate(data):
                np.save(os.path.join(target, f"seq_{start + k:05d}.npy"), seq)
            written += len(data)
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out_dir")
    ap.add_argument("--train", type=int, default=9600)
    ap.add_argument("--test", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--mnist-dir", default=None)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    glyphs = None
    if args.mnist_dir is None:
        from vp_suite_amd.datasets import procedural_digits
        glyphs = procedural_digits()
        print("no --mnist-dir given: drawing procedural_digits() — seven-segment stand-ins, this is NOT MNIST")
    n = export(args.out_dir, {"train": args.train, "test": args.test}, args.frames, glyphs, args.mnist_dir, args.img_size, args.batch)
    print(f"wrote {n} sequences of {args.frames} frames to {args.out_dir}")


if __name__ == "__main__":
    main()
