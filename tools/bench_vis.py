"""The side-by-side video canvas of a visualization (vpx_vis_compose: one launch from the model's float frames to bordered bytes) against
the plain-torch chain it replaces on the same GPU — ops.frames_postprocess, then torch.cat of colour bars per border and of the bordered
sequences — in the same run; prints ONE JSON line and writes it to profiles/vis_bench.json.

S = 4 sequences (GT and three predictions) of 20 RGB frames, context 10, composed into uint8 [20, h + 2b, 4 (w + 2b), 3]:
  * 64x64     b = 8:  src 3.9 MB, canvas 1.5 MB
  * 128x128   b = 16: src 15.7 MB, canvas 6.1 MB
Per case:
  * op_ms       wall time of visualization.compose_video on sequences already on the device: stack, host table and its check, the copy of the
                table, one launch, synchronised
  * kernel_ms   HIP events around `reps` back-to-back calls of vpx_vis_compose on a table already on the device, per call
  * torch_ms    HIP events around `reps` runs of the torch chain on the same sources (colour bars already on the device)
Every call of a repetition reads another source and writes another canvas than the one before it: ROTATE sources and canvases are cycled,
sized so that a cycle exceeds the 256 MiB last-level cache (bytes_per_cycle in the result). Medians over --steps measured passes after
--warmup; the contenders alternate inside every pass. The launch moves a few megabytes: no ratio is promised, the figures are what they are.

    python tools/bench_vis.py [--steps 10] [--warmup 2] [--cases 64x64,128x128] [--out FILE]"""
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

S, FRAMES, CONTEXT = 4, 20, 10
NAMES = ["GT", "Pred_a", "Pred_b", "Pred_c"]
LLC_BYTES = 256 << 20
CASES = {"64x64": dict(hw=(64, 64), rotate=52, reps=52), "128x128": dict(hw=(128, 128), rotate=13, reps=13)}


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
    from vp_suite_amd import _lib, ops
    from vp_suite_amd import visualization as V
    h, w = cfg["hw"]
    rotate, reps = cfg["rotate"], cfg["reps"]
    gen = torch.Generator(device="cuda").manual_seed(0)
    srcs = [torch.rand((S, FRAMES, 3, h, w), device="cuda", generator=gen) * 1.2 - 0.1 for _ in range(rotate)]
    tiles, shape, b = V.video_tiles(NAMES, FRAMES, (h, w), CONTEXT)
    host, bmax, covered = ops.check_vis_tiles(tiles, S, FRAMES, (h, w), shape)
    assert covered and bmax == b
    table = torch.from_numpy(host).cuda()
    canvases = [torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(rotate)]
    colours = [torch.tensor([V.COLORS[c] for c in V.border_colors(n, FRAMES, CONTEXT)], dtype=torch.uint8, device="cuda").view(FRAMES, 1, 1, 3) for n in NAMES]
    stream = lambda: torch.cuda.current_stream().cuda_stream             # noqa: E731
    F, Hc, Wc = shape[:3]

    def launches():
        for r in range(reps):
            _lib.check(_lib.lib().vpx_vis_compose(_lib.ptr(srcs[r % rotate]), S, FRAMES, 3, h, w, 0.0, 1.0, _lib.ptr(table), int(table.shape[0]), bmax,
                                                  _lib.ptr(canvases[r % rotate]), F, Hc, Wc, -1, stream()), "vpx_vis_compose")

    def chain(r):
        vids = ops.frames_postprocess(srcs[r % rotate], 0.0, 1.0)        # [S, T, h, w, 3]
        out = []
        for s in range(S):
            cbv = colours[s].expand(FRAMES, h, b, 3)
            cbh = colours[s].expand(FRAMES, b, w + 2 * b, 3)
            vid = torch.cat([cbv, vids[s], cbv], dim=2)
            out.append(torch.cat([cbh, vid, cbh], dim=1))
        return torch.cat(out, dim=2)

    def chains():
        for r in range(reps):
            chain(r)

    launches()
    torch.cuda.synchronize()
    equal = bool(torch.equal(canvases[0], chain(0))) and bool(torch.equal(V.compose_video(list(srcs[0]), CONTEXT, NAMES), canvases[0]))
    ms = {"op": [], "kernel": [], "torch": []}
    for step in range(warmup + steps):
        to = _wall_ms(lambda: V.compose_video(list(srcs[step % rotate]), CONTEXT, NAMES))
        tk = _event_ms(launches) / reps
        tt = _event_ms(chains) / reps
        if step >= warmup:
            ms["op"].append(to), ms["kernel"].append(tk), ms["torch"].append(tt)
    med = {k: statistics.median(v) for k, v in ms.items()}
    src_bytes, out_bytes = S * FRAMES * 3 * h * w * 4, int(np.prod(shape))
    cycle = rotate * (src_bytes + out_bytes)
    assert cycle > LLC_BYTES
    return {"frame_hw": [h, w], "border": b, "canvas": list(shape), "tiles": int(table.shape[0]), "reps": reps, "rotate": rotate,
            "op_ms": round(med["op"], 4), "kernel_ms": round(med["kernel"], 4), "torch_ms": round(med["torch"], 4),
            "torch_over_kernel": round(med["torch"] / med["kernel"], 2), "algorithmic_bytes": src_bytes + out_bytes,
            "kernel_GBps": round((src_bytes + out_bytes) / (med["kernel"] * 1e-3) / 1e9, 1), "bytes_per_cycle": cycle, "equal_bytes_vs_torch": equal}


def main():
    from vp_suite_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"what": "the video canvas of S = 4 sequences of 20 RGB frames (vpx_vis_compose, one launch, float frames to bordered bytes) vs ops.frames_postprocess + "
                   "torch.cat per border and per sequence on the same GPU, interleaved; sources and canvases rotated past the last-level cache; medians",
           "sequences": S, "frames": FRAMES, "context": CONTEXT, "steps": args.steps, "warmup": args.warmup, "cases": {}}
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
