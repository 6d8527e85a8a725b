"""Moving MNIST batches generated on the GPU (csrc/mmnist.hip through datasets.MovingMNISTOnTheFly.batch) against the host path they
replace — the numpy restatement of tests/mmnist_ref.py plus the .cuda() copy of its result — on the same machine; prints ONE JSON line
and writes it to profiles/mmnist_bench.json.

B = 32 and 128 sequences of 20 frames, 1x64x64 and 3x64x64, procedural_digits() as the glyph table. Per case:
  * batch_ms        host wall clock around batch(B) + a device synchronise: host sampling, the table's copy, the launch, the kernel;
  * sample_ms       the host sampling alone (sample_params(B)), the part of batch_ms that is numpy scalar draws;
  * kernel_ms       HIP events around KERNEL_REPS back-to-back calls of vpx_mmnist_frames on a table already on the device, per call
                    (no sampling, no copy, no allocation; launch gaps included — a kernel trace gives the kernel alone);
  * host_ms         the restatement's render() of the same rows + .cuda() + synchronise (what feeding the model from the host costs);
  * store_TBps      output bytes (B * 20 * C * 64 * 64 * 4, the only real traffic) over kernel_ms, against the 6.3 TB/s HBM roofline.
The two paths are timed interleaved in one process (one step of each in turn) after `--warmup` steps of both; medians of `--steps`.
The host path is the slow one, so its step count is capped by --host-steps.

    python tools/bench_mmnist.py [--steps 20] [--warmup 3] [--host-steps 3] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, SIDE = 20, 64
CASES = [(32, 1), (128, 1), (32, 3), (128, 3)]   # (B, C)
KERNEL_REPS = 20
HBM_ROOFLINE_TBPS = 6.3                          # achievable HBM bandwidth the project's rooflines use


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    import mmnist_ref
    from vp_suite_amd import _lib
    from vp_suite_amd.datasets import DATASET_CLASSES, procedural_digits
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmnist_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    glyphs = procedural_digits()
    glyphs_dev = torch.from_numpy(glyphs).cuda()
    out = {"what": "MovingMNISTOnTheFly.batch(B) (csrc/mmnist.hip) vs tests/mmnist_ref.py render() + .cuda(), same machine, interleaved; medians; "
                   "ratio = host_ms / batch_ms; store_TBps = output bytes / kernel_ms",
           "frames": FRAMES, "side": SIDE, "steps": args.steps, "host_steps": args.host_steps, "warmup": args.warmup,
           "hbm_roofline_TBps": HBM_ROOFLINE_TBPS, "cases": {}}
    for B, C in CASES:
        ds = DATASET_CLASSES["MMF"]("train", digits=glyphs, num_channels=C)
        ds.set_seq_len(10, 10, 1)
        assert ds.seq_len == FRAMES
        rows = ds.sample_params(B)
        rows_dev, frames = torch.from_numpy(rows).cuda(), torch.empty((B, FRAMES, C, SIDE, SIDE), device="cuda")

        def launches():
            for _ in range(KERNEL_REPS):
                _lib.check(_lib.lib().vpx_mmnist_frames(_lib.ptr(glyphs_dev), len(glyphs), glyphs.shape[1], _lib.ptr(rows_dev), B, 2, FRAMES, C, SIDE, 0.0, 1.0,
                                                        _lib.ptr(frames), torch.cuda.current_stream().cuda_stream), "vpx_mmnist_frames")

        def host():
            return torch.from_numpy(mmnist_ref.render(glyphs, rows, FRAMES, C, SIDE)).cuda()
        ms = {"batch": [], "sample": [], "kernel": [], "host": []}
        for step in range(args.warmup + args.steps):
            keep = step >= args.warmup
            t = _wall_ms(lambda: ds.batch(B))
            t0 = time.perf_counter()
            ds.sample_params(B)
            ts = (time.perf_counter() - t0) * 1e3
            tk = _event_ms(launches) / KERNEL_REPS
            if keep:
                ms["batch"].append(t), ms["sample"].append(ts), ms["kernel"].append(tk)
            if step < min(args.warmup, 1) or (keep and len(ms["host"]) < args.host_steps):
                th = _wall_ms(host)
                if keep:
                    ms["host"].append(th)
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = B * FRAMES * C * SIDE * SIDE * 4
        tbps = nbytes / (med["kernel"] * 1e-3) / 1e12
        out["cases"][f"B{B}_C{C}"] = {"batch_ms": round(med["batch"], 4), "sample_ms": round(med["sample"], 4), "kernel_ms": round(med["kernel"], 4),
                                      "host_ms": round(med["host"], 3), "ratio": round(med["host"] / med["batch"], 1), "output_bytes": nbytes,
                                      "store_TBps": round(tbps, 3), "share_of_hbm_roofline": round(tbps / HBM_ROOFLINE_TBPS, 3),
                                      "sampling_share_of_batch": round(med["sample"] / med["batch"], 3)}
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
