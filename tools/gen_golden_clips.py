"""Writes tests/golden/clips_windows.npz: the splits and window tables of the UPSTREAM KITTIRawDataset and CaltechPedestrianDataset on a
synthetic tree (build container only, CPU, through tools/ref_shim.py; the fixture is committed, this tool is how it was made).

The upstream classes only COUNT files when they are built, so the tree holds no pixels: KITTI gets <date>/<drive>/image_02/data/NNNN.png
files of zero bytes, Caltech Pedestrian a frame_counts.json whose keys are <root>/<setNN>/<Vxxx>.seq paths in sorted order (the order its
preparation step writes them in). cv2 is a stub of the shim and is never called. The names are tools/export_clips_like.py's, so a test
can export a readable tree of the same names and lengths.

One normalisation: upstream shuffles KITTI's drive directories in the order pathlib's iterdir() lists them, which the file system
decides. Here iterdir() is wrapped to list sorted, the order datasets/kitti_raw.py fixes (its docstring says so).

Per dataset D in (kitti, cp): D_names [n] / D_lengths [n] (the whole tree, sorted) and per split S in (train, val, test): D_S_seqs [m]
(indices into D_names, in the order of upstream's `sequences`), D_S_win_L_P [k, 2] = upstream's sequences_with_frame_index as (index
into D_S_seqs, start frame) for (seq_len L, seq_step P) in (4, 1), (5, 2), (7, 3). Names and integers only.

    python tools/gen_golden_clips.py"""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import export_clips_like as X  # noqa: E402
from ref_shim import load_reference  # noqa: E402

CONFIGS = [(4, 1), (5, 2), (7, 3)]                    # (seq_len, seq_step)
KITTI_LENGTHS = [7, 12, 5, 23, 9, 31, 16]
CP_LENGTHS = [7, 12, 5, 23, 9, 31, 16, 4, 14]


def frames_for(seq_len, seq_step):
    total, rest = divmod(seq_len - 1, seq_step)
    assert rest == 0
    return total + 1


def record(out, tag, cls, data_dir, names, rel_of):
    for split in ("train", "val", "test"):
        ds = cls(split, data_dir=data_dir)
        seqs = [rel_of(path) for path, _ in ds.sequences]
        out[f"{tag}_{split}_seqs"] = np.array([names.index(s) for s in seqs], dtype=np.int64)
        for seq_len, seq_step in CONFIGS:
            ds.sequences_with_frame_index = []        # (upstream appends to the list of an earlier call)
            total = frames_for(seq_len, seq_step)
            ds.set_seq_len(1, total - 1, seq_step)
            assert ds.seq_len == seq_len
            rows = [(seqs.index(rel_of(path)), start) for path, start in ds.sequences_with_frame_index]
            out[f"{tag}_{split}_win_{seq_len}_{seq_step}"] = np.array(rows, dtype=np.int64).reshape(len(rows), 2)


def main():
    load_reference()
    from vp_suite.datasets.caltech_pedestrian import CaltechPedestrianDataset
    from vp_suite.datasets.kitti_raw import KITTIRawDataset
    plain_iterdir = pathlib.Path.iterdir
    pathlib.Path.iterdir = lambda self: iter(sorted(plain_iterdir(self)))
    out = {}
    tmp = tempfile.mkdtemp(prefix="clips_golden_")

    kitti_dir = os.path.join(tmp, "kitti")
    names = X.kitti_names(len(KITTI_LENGTHS))
    for name, n in zip(names, KITTI_LENGTHS):
        data = os.path.join(kitti_dir, name, X.CAMERA, "data")
        os.makedirs(data)
        for k in range(n):
            open(os.path.join(data, f"{k:010d}.png"), "w").close()
    out["kitti_names"], out["kitti_lengths"] = np.array(names), np.array(KITTI_LENGTHS, dtype=np.int64)
    record(out, "kitti", KITTIRawDataset, kitti_dir, names, lambda p: os.path.relpath(str(p), kitti_dir))

    cp_dir = os.path.join(tmp, "cp")
    os.makedirs(cp_dir)
    names = X.cp_names(len(CP_LENGTHS))
    with open(os.path.join(cp_dir, "frame_counts.json"), "w") as fh:
        json.dump({os.path.join(cp_dir, name + ".seq"): n for name, n in zip(names, CP_LENGTHS)}, fh)
    out["cp_names"], out["cp_lengths"] = np.array(names), np.array(CP_LENGTHS, dtype=np.int64)
    record(out, "cp", CaltechPedestrianDataset, cp_dir, names, lambda p: os.path.relpath(str(p), cp_dir)[:-len(".seq")])

    target = os.path.join(ROOT, "tests", "golden", "clips_windows.npz")
    np.savez_compressed(target, **out)
    print(f"wrote {target}: {len(out)} arrays, {os.path.getsize(target)} bytes")
    for k in sorted(out):
        print(k, out[k].tolist())


if __name__ == "__main__":
    main()
