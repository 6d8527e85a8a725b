"""Gradient clipping around the flat Adam update (csrc/train_tail.hip), on the flat buckets of the default `convlstm-shi` and `predrnn-pp`
models; prints ONE JSON line and writes it to profiles/clip_bench.json.

Three variants of one optimizer step on the same (param, grad, exp_avg, exp_avg_sq) buckets, max_norm = half the gradient's norm:
  * plain:   ops.adam_step alone (no clipping: the step before this feature);                                28 B per element
  * fused:   ops.grad_stats + ops.adam_step_clipped (norm read on the device, no host sync);                 28 + 4 B per element
  * torch:   torch.nn.utils.clip_grad_norm_ on the parameters' views of the gradient bucket + ops.adam_step;  28 + 12 B per element
             (norm: one read; scaling: one read, one write — and a string of small launches per parameter)
The three are timed interleaved in one process (one step of each in turn), HIP events around each step after `--warmup` steps of all,
the median of `--steps` reported. Bytes are the algorithmic floor of each variant (what it must move), not a counter.

    python tools/bench_clip.py [--steps 50] [--warmup 10] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = ("convlstm-shi", "predrnn-pp")
BYTES_PER_ELEM = {"plain": 28, "fused": 32, "torch": 40}


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _time_interleaved(fns, steps, warmup):
    """{name: median ms}, one step of each variant in turn."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    from vp_suite_amd import ops
    from vp_suite_amd.models import MODEL_CLASSES
    from vp_suite_amd.train import FlatAdam
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"what": "one optimizer step on the model's flat buckets: ops.adam_step | ops.grad_stats + ops.adam_step_clipped | "
                   "clip_grad_norm_ on the views + ops.adam_step; interleaved, median ms; bytes = algorithmic floor",
           "steps": args.steps, "warmup": args.warmup, "models": {}}
    for name in MODELS:
        torch.manual_seed(0)
        model = MODEL_CLASSES[name]("cuda", img_shape=(1, 64, 64), action_size=0, tensor_value_range=[0.0, 1.0]).to("cuda")
        opt = FlatAdam.from_module(model, lr=1e-4)
        params = opt.param_groups[0]["params"]
        n = opt.flat_param.numel()
        grad0 = torch.randn(n, device="cuda") * 1e-2
        max_norm = 0.5 * float(grad0.norm())
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        state = {"step": 0}

        def begin():
            opt.flat_grad.copy_(grad0)   # (the torch variant scales the bucket in place: every step starts from the same gradient)
            state["step"] += 1
            return state["step"]

        def plain():
            ops.adam_step(opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, begin(), 1e-4)

        def fused():
            k = begin()
            ops.grad_stats(opt.flat_grad, 1.0, out=stats)
            ops.adam_step_clipped(opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, k, 1e-4, stats=stats, max_norm=max_norm)

        def torch_clip():
            k = begin()
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            ops.adam_step(opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq, k, 1e-4)

        def copy_only():   # what begin() costs inside every variant: reported, and subtracted in `net_ms`
            begin()

        ms = _time_interleaved({"plain": plain, "fused": fused, "torch": torch_clip, "copy_only": copy_only}, args.steps, args.warmup)
        res = {"elements": n, "parameters": len(params), "copy_only_ms": round(ms["copy_only"], 4)}
        for k, b in BYTES_PER_ELEM.items():
            net = max(ms[k] - ms["copy_only"], 1e-6)
            res[k] = {"ms": round(ms[k], 4), "net_ms": round(net, 4), "bytes": b * n, "achieved_TBps": round(b * n / (net * 1e-3) / 1e12, 3)}
        res["fused_over_plain"] = round(res["fused"]["net_ms"] / res["plain"]["net_ms"], 3)
        res["torch_over_plain"] = round(res["torch"]["net_ms"] / res["plain"]["net_ms"], 3)
        out["models"][name] = res
        del model, opt
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
