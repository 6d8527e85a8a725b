"""LPIPS (csrc/lpips.hip through ops.lpips_frames) against the plain-torch float32 chain of tests/lpips_ref.py on the same GPU, on the
seeded weights of that module; prints ONE JSON line and writes it to profiles/lpips_bench.json. Not part of bench.py.

For B*T = 160 frames of 3x64x64 and of 3x128x128 (T = 10): the whole measure forward, the stem, the first max-pool and the first head on
their own against the matching torch expressions, and forward + backward (ops.lpips_frames_diff and its gradient with respect to the
prediction against the torch chain under autograd, cotangent of ones).
Library and torch calls are timed interleaved in one process (one step of each in turn), HIP events around each step after `--warmup`
steps of both, the median of `--steps` reported; ratio = torch ms / library ms. Every step reads the next of a ring of input pairs
that together exceed the last-level cache (256 MiB), so no step finds its inputs cached by the one before.

    python tools/bench_lpips.py [--steps 20] [--warmup 5] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"160x3x64x64": (16, 10, 3, 64, 64), "160x3x128x128": (16, 10, 3, 128, 128)}
LAST_LEVEL_CACHE = 256 << 20


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


class _Ring:
    """Input sets handed out in turn; together larger than the last-level cache."""

    def __init__(self, make, set_bytes):
        self.sets = [make() for _ in range(LAST_LEVEL_CACHE // set_bytes + 2)]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def _time_pair(fn, ref, ring, steps, warmup):
    """(median ms of fn, median ms of ref), one step of each in turn, each on the ring's next input set."""
    for _ in range(warmup):
        fn(*ring.next())
        ref(*ring.next())
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(steps):
        for f, acc in ((fn, ms[0]), (ref, ms[1])):
            args = ring.next()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f(*args)
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return statistics.median(ms[0]), statistics.median(ms[1])


def _entry(lib_ms, ref_ms):
    return {"ms": round(lib_ms, 4), "torch_ms": round(ref_ms, 4), "ratio": round(ref_ms / lib_ms, 2)}


def main():
    import lpips_ref
    from vp_suite_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    w = {k: v.cuda() for k, v in lpips_ref.weights().items()}
    mean, std = torch.tensor(lpips_ref.MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(lpips_ref.STD, device="cuda").view(1, 3, 1, 1)
    out = {"what": "csrc/lpips.hip vs the plain-torch float32 chain (same GPU, same weights), forward (and forward + backward to the prediction), interleaved, inputs rotated through a ring larger "
                   "than the last-level cache; ratio = torch ms / library ms", "steps": args.steps, "warmup": args.warmup, "cases": {}}

    def torch_norm(x):
        return (((x + 1) / 2).clamp(0.0, 1.0) - mean) / std

    def torch_chain(pred, target):
        b, t = pred.shape[:2]
        f = torch_norm(torch.cat([pred.flatten(0, 1), target.flatten(0, 1)]))
        total = 0
        for i in range(5):
            if lpips_ref.POOL_BEFORE[i]:
                f = F.max_pool2d(f, 3, 2)
            s, p = lpips_ref.STRIDE_PAD[i]
            f = F.relu(F.conv2d(f, w[f"conv{i + 1}.weight"], w[f"conv{i + 1}.bias"], stride=s, padding=p))
            n = f / (f.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            total = total + ((n[:b * t] - n[b * t:]).pow(2) * w[f"lin{i + 1}.weight"].view(1, -1, 1, 1)).sum(dim=1).flatten(1).mean(dim=1)
        return total.view(b, t)

    def torch_head(fx, fy):
        nx, ny = fx / (fx.pow(2).sum(dim=3, keepdim=True).sqrt() + 1e-10), fy / (fy.pow(2).sum(dim=3, keepdim=True).sqrt() + 1e-10)
        return ((nx - ny).pow(2) * w["lin1.weight"]).sum(dim=3).flatten(1).mean(dim=1)

    def train_step(fn):
        def run(pred, target):
            p = pred.detach().requires_grad_()
            fn(p, target).sum().backward()
            return p.grad
        return run

    with torch.no_grad():
        for name, shape in CASES.items():
            frames = _Ring(lambda: (torch.rand(shape, device="cuda") * 2.6 - 1.3, torch.rand(shape, device="cuda") * 2.6 - 1.3), 2 * 4 * torch.Size(shape).numel())
            res = {"lpips_frames": _entry(*_time_pair(lambda p, t: ops.lpips_frames(p, t, w), torch_chain, frames, args.steps, args.warmup))}
            res["stem"] = _entry(*_time_pair(lambda p, t: ops.lpips_stem(p.flatten(0, 1), w["conv1.weight"], w["conv1.bias"], t.flatten(0, 1)),
                                             lambda p, t: F.relu(F.conv2d(torch_norm(torch.cat([p.flatten(0, 1), t.flatten(0, 1)])), w["conv1.weight"], w["conv1.bias"], stride=4, padding=2)),
                                             frames, args.steps, args.warmup))
            n2, h1 = 2 * shape[0] * shape[1], (shape[3] + 4 - 11) // 4 + 1
            maps = _Ring(lambda: (torch.rand(n2 // 2, h1, h1, 64, device="cuda"), torch.rand(n2 // 2, h1, h1, 64, device="cuda")), 4 * n2 * h1 * h1 * 64)
            res["maxpool1"] = _entry(*_time_pair(lambda a, b: ops.lpips_maxpool(a), lambda a, b: F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2), maps, args.steps, args.warmup))
            res["head1"] = _entry(*_time_pair(lambda a, b: ops.lpips_head(a, b, w["lin1.weight"]), torch_head, maps, args.steps, args.warmup))
            with torch.enable_grad():
                res["lpips_frames_diff fwd+bwd"] = _entry(*_time_pair(train_step(lambda p, t: ops.lpips_frames_diff(p, t, w)), train_step(torch_chain),
                                                                      frames, args.steps, args.warmup))
            out["cases"][name] = res
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
