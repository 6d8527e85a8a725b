"""Measure kernels (csrc/measure.hip) against the plain-torch expressions of tests/measure_ref.py on the same GPU in fp32; prints
ONE JSON line and writes it to profiles/measures_bench.json.

For B*T = 160 frames of 3x128x128 and B*T = 1280 frames of 1x64x64 (SSIM needs 3 channels: 3x128x128 only), T = 10:
  * pixel: the per-frame sums of d^2, |d|, smooth-L1 — forward, and forward + backward of an mse + l1 + smooth_l1 + psnr mix;
           achieved bytes/s against the floor of two tensor reads (forward) resp. four reads and one write (forward + backward);
  * ssim:  per-frame SSIM — forward, and forward + backward;
  * metrics: PredictionMetricProvider.get_metrics(all_frame_cnts=True) against the reference's loop (every measure re-evaluated for
           every horizon 1..T, one .item() per value).
Library and torch calls are timed interleaved in one process (one step of each in turn), HIP events around each step after
`--warmup` steps of both, the median of `--steps` reported; ratio = torch ms / library ms.

    python tools/bench_measures.py [--steps 20] [--warmup 5] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"160x3x128x128": (16, 10, 3, 128, 128), "1280x1x64x64": (128, 10, 1, 64, 64)}
F32 = torch.float32


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _time_pair(fn, ref, steps, warmup):
    """(median ms of fn, median ms of ref), one step of each in turn."""
    for _ in range(warmup):
        fn()
        ref()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(steps):
        for f, acc in ((fn, ms[0]), (ref, ms[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return statistics.median(ms[0]), statistics.median(ms[1])


def _entry(lib_ms, ref_ms, floor_bytes=None):
    e = {"ms": round(lib_ms, 4), "torch_ms": round(ref_ms, 4), "ratio": round(ref_ms / lib_ms, 2)}
    if floor_bytes is not None:
        e["floor_bytes"] = floor_bytes
        e["achieved_TBps"] = round(floor_bytes / (lib_ms * 1e-3) / 1e12, 3)
    return e


def _mix(table, frame_elems):
    return (table[0] + table[1] + table[2] + 10 * torch.log10(table[0] / frame_elems)).mean()


def main():
    import measure_ref
    from vp_suite_amd import ops
    from vp_suite_amd.measure import PredictionMetricProvider
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measures_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"what": "csrc/measure.hip vs tests/measure_ref.py (plain torch, fp32, same GPU), interleaved; ratio = torch ms / library ms",
           "steps": args.steps, "warmup": args.warmup, "cases": {}}
    for name, shape in CASES.items():
        pred = (torch.rand(shape, device="cuda") * 2.4 - 1.2).requires_grad_(True)
        target = torch.rand(shape, device="cuda") * 2.4 - 1.2
        fe, nbytes = pred[0, 0].numel(), pred.numel() * 4
        res = {}

        def fwd(f, **kw):
            def run():
                with torch.no_grad():
                    f(pred, target, **kw)
            return run

        def fwd_bwd(f, reduce, **kw):
            def run():
                pred.grad = None
                reduce(f(pred, target, **kw)).backward()
            return run
        res["pixel_fwd"] = _entry(*_time_pair(fwd(ops.pixel_measures), fwd(measure_ref.frame_sums, dtype=F32), args.steps, args.warmup), 2 * nbytes)
        res["pixel_fwd_bwd"] = _entry(*_time_pair(fwd_bwd(ops.pixel_measures, lambda t: _mix(t, fe)), fwd_bwd(measure_ref.frame_sums, lambda t: _mix(t, fe), dtype=F32),
                                                  args.steps, args.warmup), 5 * nbytes)
        keys = ("mse", "l1", "smooth_l1", "psnr")
        if shape[2] == 3:
            res["ssim_fwd"] = _entry(*_time_pair(fwd(ops.ssim_frames), fwd(measure_ref.ssim_frames, dtype=F32), args.steps, args.warmup))
            res["ssim_fwd_bwd"] = _entry(*_time_pair(fwd_bwd(ops.ssim_frames, torch.mean), fwd_bwd(measure_ref.ssim_frames, torch.mean, dtype=F32), args.steps, args.warmup))
            keys = measure_ref.KEYS
        mp = PredictionMetricProvider({"device": "cuda", "metrics": list(keys)})

        def metrics_ref():   # metric_provider.py:58-71: every horizon re-evaluates every measure, one host sync per value
            with torch.no_grad():
                return [{k: float(measure_ref.display(k, v).item()) for k, v in measure_ref.measures(pred[:, :n], target[:, :n], F32, keys).items()}
                        for n in range(1, shape[1] + 1)]
        res["metrics_all_frame_cnts"] = _entry(*_time_pair(lambda: mp.get_metrics(pred, target, all_frame_cnts=True), metrics_ref, args.steps, args.warmup))
        res["metrics"] = list(keys)
        out["cases"][name] = res
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
