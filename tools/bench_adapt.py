"""The frame adapter (csrc/adapt.hip through ops.frames_adapt, one launch) against the plain-torch chain it replaces on the same GPU —
the reference's two ScaleTo... expressions (utils/models.py:32-33, 62-63) plus F.interpolate — interleaved; prints ONE JSON line and
writes it to profiles/adapt_bench.json.

1280 planar float32 frames (128 sequences of 10): 3x64x64 -> 3x128x128 with [0, 1] -> [-1, 1] (into a larger model), the reverse
(3x128x128 -> 3x64x64, [-1, 1] -> [0, 1]: its predictions back), and the affine-only case at 3x64x64. Per case:
  * kernel_ms   HIP events around KERNEL_REPS back-to-back ops.frames_adapt calls, per call
  * torch_ms    HIP events around KERNEL_REPS runs of the torch chain on the same tensor, per run
  * TBps        algorithmic bytes 4 N C (H W + oh ow) — the input read once, the output written once — over the time
Medians over --steps measured passes after --warmup; the library and the torch chain alternate inside every pass. Both sides allocate
their output in every call (the caching allocator serves it), as a model's adapter does.

    python tools/bench_adapt.py [--steps 20] [--warmup 3] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C = 1280, 3
CASES = {   # name: ((H, W), (oh, ow), src range, dst range)
    "up_3x64x64_to_3x128x128": ((64, 64), (128, 128), (0.0, 1.0), (-1.0, 1.0)),
    "down_3x128x128_to_3x64x64": ((128, 128), (64, 64), (-1.0, 1.0), (0.0, 1.0)),
    "affine_3x64x64": ((64, 64), (64, 64), (0.0, 1.0), (-1.0, 1.0)),
}
KERNEL_REPS = 20
HBM_ROOFLINE_TBPS = 6.3    # achievable HBM bandwidth the project's rooflines use


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    from vp_suite_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"what": "ops.frames_adapt (csrc/adapt.hip, one launch) vs the torch chain (img - lo) / (hi - lo), * (hi' - lo') + lo', F.interpolate on the "
                   "same GPU, interleaved; medians; TBps over 4 N C (H W + oh ow) bytes",
           "frames": N, "channels": C, "steps": args.steps, "warmup": args.warmup, "hbm_roofline_TBps": HBM_ROOFLINE_TBPS, "cases": {}}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, ((H, W), (oh, ow), src, dst) in CASES.items():
        x = torch.rand((N, C, H, W), device="cuda", generator=gen) * (src[1] - src[0]) + src[0]
        size = None if (oh, ow) == (H, W) else (oh, ow)

        def launch():
            return ops.frames_adapt(x, size, src, dst)

        def chain():
            img = (x - src[0]) / (src[1] - src[0])
            img = img * (dst[1] - dst[0]) + dst[0]
            return img if size is None else F.interpolate(img, size=size, mode="bilinear", align_corners=False, antialias=False)

        def launches():
            for _ in range(KERNEL_REPS):
                launch()

        def chains():
            for _ in range(KERNEL_REPS):
                chain()
        max_diff = float((launch() - chain()).abs().max())
        torch.cuda.synchronize()
        ms = {"kernel": [], "torch": []}
        for step in range(args.warmup + args.steps):
            tk = _event_ms(launches) / KERNEL_REPS
            tt = _event_ms(chains) / KERNEL_REPS
            if step >= args.warmup:
                ms["kernel"].append(tk), ms["torch"].append(tt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = 4 * N * C * (H * W + oh * ow)
        tbps = nbytes / (med["kernel"] * 1e-3) / 1e12
        out["cases"][name] = {"kernel_ms": round(med["kernel"], 4), "torch_ms": round(med["torch"], 4), "torch_over_kernel": round(med["torch"] / med["kernel"], 2),
                              "kernel_ms_min_max": [round(min(ms["kernel"]), 4), round(max(ms["kernel"]), 4)], "algorithmic_bytes": nbytes,
                              "kernel_TBps": round(tbps, 3), "torch_TBps": round(nbytes / (med["torch"] * 1e-3) / 1e12, 3),
                              "share_of_hbm_roofline": round(tbps / HBM_ROOFLINE_TBPS, 3), "max_abs_diff_vs_torch": max_diff}
    with open(_lib.LIB_PATH, "rb") as fh:
        out["lib_sha16"] = hashlib.sha256(fh.read()).hexdigest()[:16]
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
