"""Batches of stored Moving MNIST frames (csrc/frames.hip through datasets.StoredVPDataset.batch) against the plain-torch chain they
replace on the same GPU — index, .float() / 255, permute, expand, F.interpolate — interleaved; prints ONE JSON line and writes it to
profiles/frames_bench.json.

batch(128) of 20 stored 64x64 gray frames out of 1024 stored sequences (uint8, on the device), to 3x64x64 and to 3x128x128. Per case:
  * batch_ms    wall time of ds.batch(indices): host table, its copy, one launch, zero actions, synchronised
  * kernel_ms   HIP events around KERNEL_REPS back-to-back calls of vpx_frames_preprocess on a table already on the device, per call
  * torch_ms    HIP events around KERNEL_REPS runs of the torch chain on the same indices (already on the device), per run
  * GBps        algorithmic bytes (source bytes read once + output bytes written once) / kernel_ms, and the same for the torch chain
Medians over --steps measured passes after --warmup; the library and the torch chain alternate inside every pass.

    python tools/bench_frames.py [--steps 20] [--warmup 3] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SEQS, FRAMES, SIDE, B = 1024, 20, 64, 128
CASES = [64, 128]          # output side
KERNEL_REPS = 20
HBM_ROOFLINE_TBPS = 6.3    # achievable HBM bandwidth the project's rooflines use


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
    from vp_suite_amd import _lib
    from vp_suite_amd.datasets import StoredVPDataset
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 256, size=(N_SEQS, FRAMES, SIDE, SIDE), dtype=np.uint8)
    out = {"what": "StoredVPDataset.batch(128) (csrc/frames.hip, one launch) vs the torch chain index / .float() / 255 / permute / expand / "
                   "F.interpolate on the same GPU, interleaved; medians; GBps over source bytes read once + output bytes written once",
           "stored": [N_SEQS, FRAMES, SIDE, SIDE], "batch": B, "steps": args.steps, "warmup": args.warmup, "hbm_roofline_TBps": HBM_ROOFLINE_TBPS, "cases": {}}
    for side in CASES:
        class Gray3(StoredVPDataset):
            OUT_CHANNELS = 3
        ds = Gray3("train", raw=raw, img_size=side)
        ds.set_seq_len(10, 10, 1)
        indices = rng.permutation(N_SEQS)[:B].tolist()
        src = ds._stored()
        table_dev = torch.from_numpy(ds.table(indices)).cuda()
        index_dev = torch.tensor(indices, device="cuda")
        frames = torch.empty((B, FRAMES, 3, side, side), device="cuda")

        def launches():
            for _ in range(KERNEL_REPS):
                _lib.check(_lib.lib().vpx_frames_preprocess(_lib.ptr(src), _lib.FRAMES_U8, N_SEQS, FRAMES, SIDE, SIDE, 1, _lib.ptr(table_dev), B, FRAMES, 1,
                                                            SIDE, SIDE, side, side, 3, 0.0, 1.0, _lib.ptr(frames), torch.cuda.current_stream().cuda_stream),
                           "vpx_frames_preprocess")

        def chain():
            x = src[index_dev].float() / 255                                   # [B, T, H, W]
            x = x.unsqueeze(-1).permute(0, 1, 4, 2, 3).expand(-1, -1, 3, -1, -1)
            if side != SIDE:
                x = torch.nn.functional.interpolate(x.reshape(B * FRAMES, 3, SIDE, SIDE), size=(side, side), mode="bilinear", align_corners=False)
                return x.reshape(B, FRAMES, 3, side, side)
            return x.contiguous()

        def chains():
            for _ in range(KERNEL_REPS):
                chain()
        launches()
        want = chain()
        torch.cuda.synchronize()
        max_diff = float((frames - want).abs().max())
        ms = {"batch": [], "kernel": [], "torch": []}
        for step in range(args.warmup + args.steps):
            tb = _wall_ms(lambda: ds.batch(indices))
            tk = _event_ms(launches) / KERNEL_REPS
            tt = _event_ms(chains) / KERNEL_REPS
            if step >= args.warmup:
                ms["batch"].append(tb), ms["kernel"].append(tk), ms["torch"].append(tt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = B * FRAMES * SIDE * SIDE + B * FRAMES * 3 * side * side * 4
        gbps = nbytes / (med["kernel"] * 1e-3) / 1e9
        out["cases"][f"to_3x{side}x{side}"] = {"batch_ms": round(med["batch"], 4), "kernel_ms": round(med["kernel"], 4), "torch_ms": round(med["torch"], 4),
                                               "torch_over_kernel": round(med["torch"] / med["kernel"], 2), "algorithmic_bytes": nbytes,
                                               "kernel_GBps": round(gbps, 1), "torch_GBps": round(nbytes / (med["torch"] * 1e-3) / 1e9, 1),
                                               "share_of_hbm_roofline": round(gbps / 1e3 / HBM_ROOFLINE_TBPS, 3), "max_abs_diff_vs_torch": max_diff}
    with open(_lib.LIB_PATH, "rb") as fh:
        out["lib_sha16"] = hashlib.sha256(fh.read()).hexdigest()[:16]
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
