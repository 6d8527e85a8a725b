"""Batches of windows of long stored clips (vpx_clips_preprocess through datasets.ClipVPDataset.batch) against the plain-torch chain they
replace on the same GPU — index the frames, permute, .float() / 255, F.interpolate — and against vpx_frames_preprocess at equal shapes
in the same run; prints ONE JSON line and writes it to profiles/clips_bench.json.

batch(128) of 20 uint8 RGB frames (seq_step 1) out of clips of different lengths held back to back on the device:
  * 64x64     stored 64 x 64, returned 3 x 64 x 64 (no resize)
  * kitti     stored 375 x 1242, returned 3 x 64 x 64 (bilinear resize)
Per case:
  * batch_ms          wall time of ds.batch(indices): host table, its copies, one launch, zero actions, synchronised
  * kernel_ms         HIP events around `reps` back-to-back calls of vpx_clips_preprocess on tables already on the device, per call
  * frames_kernel_ms  the same for vpx_frames_preprocess over the SAME buffer seen as equal-length sequences of 20 frames, as many
                      samples, frames and pixels: the same per-pixel work without the offset lookup. clips_over_frames is the ratio.
  * torch_ms          HIP events around `reps` runs of the torch chain on the same windows (frame indices already on the device)
Every call of a repetition reads other windows and writes another destination than the one before it: ROTATE tables and destinations
are cycled, sized so that a cycle's sources and destinations exceed the 256 MiB last-level cache (bytes_per_cycle in the result).
Medians over --steps measured passes after --warmup; the three contenders alternate inside every pass.

    python tools/bench_clips.py [--steps 10] [--warmup 2] [--cases 64x64,kitti] [--out FILE]"""
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

B, FRAMES, OUT = 128, 20, 64
ROTATE = 4
LLC_BYTES = 256 << 20
CASES = {"64x64": dict(hw=(64, 64), clips=64, min_len=200, max_len=400, reps=8),
         "kitti": dict(hw=(375, 1242), clips=8, min_len=300, max_len=500, reps=2)}


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


def run_case(name, cfg, steps, warmup):
    from vp_suite_amd import _lib
    from vp_suite_amd.datasets import ClipVPDataset
    H, W = cfg["hw"]
    rng = np.random.default_rng(0)
    lengths = rng.integers(cfg["min_len"], cfg["max_len"] + 1, size=cfg["clips"]).tolist()
    total = int(sum(lengths))
    shapes_only = [np.broadcast_to(np.zeros((), dtype=np.uint8), (n, H, W, 3)) for n in lengths]   # no host pixels: the buffer is made on the device
    ds = ClipVPDataset("train", clips=shapes_only, img_size=OUT if (H, W) != (OUT, OUT) else None)
    gen = torch.Generator(device="cuda").manual_seed(0)
    flat = torch.empty((total, H, W, 3), dtype=torch.uint8, device="cuda")
    for k in range(0, total, 256):                                       # seeded noise bytes, made on the device in slabs
        flat[k:k + 256] = torch.randint(0, 256, flat[k:k + 256].shape, dtype=torch.uint8, device="cuda", generator=gen)
    ds._raw = flat
    ds.set_seq_len(FRAMES // 2, FRAMES // 2, 1)
    assert len(ds) >= B and ds.img_shape == (3, OUT, OUT)
    stream = lambda: torch.cuda.current_stream().cuda_stream             # noqa: E731
    first_dev = torch.from_numpy(ds.clip_first).cuda()
    n_seqs = total // FRAMES                                             # the same buffer as equal-length sequences
    picks = [rng.permutation(len(ds))[:B].tolist() for _ in range(ROTATE)]
    clip_tables = [torch.from_numpy(ds.clips_table([ds.windows[i] for i in p])[0]).cuda() for p in picks]
    seq_tables = [torch.from_numpy(np.stack([rng.permutation(n_seqs)[:B], np.zeros(B), np.zeros(B), np.zeros(B)], axis=1).astype(np.int32)).cuda() for _ in range(ROTATE)]
    frame_idx = [torch.from_numpy(np.array([[int(ds.clip_first[c]) + s + t for t in range(FRAMES)] for c, s in (ds.windows[i] for i in p)])).cuda() for p in picks]
    outs = [torch.empty((B, FRAMES, 3, OUT, OUT), device="cuda") for _ in range(ROTATE)]
    reps = cfg["reps"]

    def clips_launches():
        for r in range(reps):
            _lib.check(_lib.lib().vpx_clips_preprocess(_lib.ptr(flat), _lib.FRAMES_U8, total, H, W, 3, _lib.ptr(first_dev), len(lengths), _lib.ptr(clip_tables[r % ROTATE]),
                                                       B, FRAMES, 1, H, W, OUT, OUT, 3, 0.0, 1.0, _lib.ptr(outs[r % ROTATE]), stream()), "vpx_clips_preprocess")

    def frames_launches():
        for r in range(reps):
            _lib.check(_lib.lib().vpx_frames_preprocess(_lib.ptr(flat), _lib.FRAMES_U8, n_seqs, FRAMES, H, W, 3, _lib.ptr(seq_tables[r % ROTATE]), B, FRAMES, 1,
                                                        H, W, OUT, OUT, 3, 0.0, 1.0, _lib.ptr(outs[r % ROTATE]), stream()), "vpx_frames_preprocess")

    def chain(r):
        x = flat[frame_idx[r % ROTATE]]                                  # [B, T, H, W, 3]
        x = x.permute(0, 1, 4, 2, 3).float() / 255
        if (H, W) != (OUT, OUT):
            x = torch.nn.functional.interpolate(x.reshape(B * FRAMES, 3, H, W), size=(OUT, OUT), mode="bilinear", align_corners=False)
            return x.reshape(B, FRAMES, 3, OUT, OUT)
        return x.contiguous()

    def chains():
        for r in range(reps):
            chain(r)

    clips_launches()
    torch.cuda.synchronize()
    max_diff = float((outs[0] - chain(0)).abs().max())
    ms = {"batch": [], "kernel": [], "frames_kernel": [], "torch": []}
    for step in range(warmup + steps):
        tb = _wall_ms(lambda: ds.batch(picks[step % ROTATE]))
        tk = _event_ms(clips_launches) / reps
        tf = _event_ms(frames_launches) / reps
        tt = _event_ms(chains) / reps
        if step >= warmup:
            ms["batch"].append(tb), ms["kernel"].append(tk), ms["frames_kernel"].append(tf), ms["torch"].append(tt)
    med = {k: statistics.median(v) for k, v in ms.items()}
    resize = (H, W) != (OUT, OUT)
    src_bytes = B * FRAMES * (OUT * OUT * 4 * 3 if resize else H * W * 3)   # with resize: four taps per returned pixel and channel, at the most
    out_bytes = B * FRAMES * 3 * OUT * OUT * 4
    cycle = ROTATE * (out_bytes + B * FRAMES * H * W * 3)
    assert cycle > LLC_BYTES
    return {"stored_hw": [H, W], "clip_lengths": lengths, "windows": len(ds), "reps": reps, "batch_ms": round(med["batch"], 4), "kernel_ms": round(med["kernel"], 4),
            "frames_kernel_ms": round(med["frames_kernel"], 4), "clips_over_frames": round(med["kernel"] / med["frames_kernel"], 3),
            "torch_ms": round(med["torch"], 4), "torch_over_kernel": round(med["torch"] / med["kernel"], 2),
            "algorithmic_bytes": src_bytes + out_bytes, "kernel_GBps": round((src_bytes + out_bytes) / (med["kernel"] * 1e-3) / 1e9, 1),
            "bytes_per_cycle": cycle, "max_abs_diff_vs_torch": max_diff}


def main():
    from vp_suite_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"what": "ClipVPDataset.batch(128) of 20 uint8 RGB frames (vpx_clips_preprocess, one launch) vs vpx_frames_preprocess at equal shapes and vs the torch "
                   "chain index / permute / .float() / 255 / F.interpolate on the same GPU, interleaved; tables and destinations rotated past the "
                   "last-level cache; medians", "batch": B, "frames": FRAMES, "returned": [3, OUT, OUT], "rotate": ROTATE, "steps": args.steps,
           "warmup": args.warmup, "cases": {}}
    for name in args.cases.split(","):
        out["cases"][name] = run_case(name, CASES[name], args.steps, args.warmup)
        torch.cuda.empty_cache()
    with open(_lib.LIB_PATH, "rb") as fh:
        out["lib_sha16"] = hashlib.sha256(fh.read()).hexdigest()[:16]
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
