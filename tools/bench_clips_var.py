"""Batches of windows of clips of MIXED frame sizes (vpx_clips_preprocess_var, one launch) against vpx_clips_preprocess at equal shapes in
the same run, and against the plain-torch chain at mixed shapes; prints ONE JSON line and writes it to profiles/clips_var_bench.json.

batch(128) of 20 uint8 RGB frames (seq_step 1) out of clips held back to back on the device:
  * A  equal    every clip 64 x 64, returned 3 x 64 x 64 (no resize): the new launch against vpx_clips_preprocess over the SAME buffer,
                windows and destinations — the same per-pixel work plus one geometry lookup. var_over_clips is the ratio.
  * B  h36m     clips of 1000 x 1000 and 1002 x 1000, whole frames resized to 3 x 64 x 64: the new launch against the torch chain, which
                has to treat each frame size on its own (per size: index the frames, permute, .float() / 255, F.interpolate, then
                index_copy_ into the batch).
Per case kernel_ms / other_ms: HIP events around `reps` back-to-back calls on tables already on the device, per call. Every call of a
repetition reads other windows and writes another destination than the one before it: ROTATE tables and destinations are cycled, sized so
that a cycle's sources and destinations exceed the 256 MiB last-level cache (bytes_per_cycle in the result). Medians over --steps
measured passes after --warmup; the contenders alternate inside every pass.

    python tools/bench_clips_var.py [--steps 10] [--warmup 2] [--cases equal,h36m] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, FRAMES, OUT = 128, 20, 64
ROTATE = 4
LLC_BYTES = 256 << 20
CASES = {"equal": dict(sizes=[(64, 64)], clips=64, min_len=200, max_len=400, reps=8),
         "h36m": dict(sizes=[(1000, 1000), (1002, 1000)], clips=8, min_len=40, max_len=60, reps=2)}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_case(name, cfg, steps, warmup):
    from vp_suite_amd import _lib
    rng = np.random.default_rng(0)
    lengths = rng.integers(cfg["min_len"], cfg["max_len"] + 1, size=cfg["clips"]).tolist()
    sizes = [cfg["sizes"][k % len(cfg["sizes"])] for k in range(cfg["clips"])]
    elems = [n * h * w * 3 for n, (h, w) in zip(lengths, sizes)]
    first = np.concatenate([[0], np.cumsum(elems)]).astype(np.int64)
    total = int(first[-1])
    gen = torch.Generator(device="cuda").manual_seed(0)
    flat = torch.empty(total, dtype=torch.uint8, device="cuda")
    for k in range(0, total, 1 << 26):                                   # seeded noise bytes, made on the device in slabs
        flat[k:k + (1 << 26)] = torch.randint(0, 256, flat[k:k + (1 << 26)].shape, dtype=torch.uint8, device="cuda", generator=gen)
    geom = np.array([(o, n, h, w) for o, n, (h, w) in zip(first[:-1].tolist(), lengths, sizes)], dtype=np.int64)
    geom_dev = torch.from_numpy(geom).cuda()
    windows = [(c, s) for c, n in enumerate(lengths) for s in range(0, n - FRAMES + 1)]
    picks = [[windows[i] for i in rng.permutation(len(windows))[:B]] for _ in range(ROTATE)]
    var_tables = [torch.tensor([(c, s, 0, 0) + sizes[c] + (0, 0) for c, s in p], dtype=torch.int32).cuda() for p in picks]
    outs = [torch.empty((B, FRAMES, 3, OUT, OUT), device="cuda") for _ in range(ROTATE)]
    stream = lambda: torch.cuda.current_stream().cuda_stream             # noqa: E731
    reps, equal = cfg["reps"], len(cfg["sizes"]) == 1

    def var_launches():
        for r in range(reps):
            _lib.check(_lib.lib().vpx_clips_preprocess_var(_lib.ptr(flat), _lib.FRAMES_U8, total, 3, _lib.ptr(geom_dev), len(lengths), _lib.ptr(var_tables[r % ROTATE]),
                                                           B, FRAMES, 1, OUT, OUT, 3, 0.0, 1.0, _lib.ptr(outs[r % ROTATE]), stream()), "vpx_clips_preprocess_var")

    if equal:
        H, W = sizes[0]
        frames_first = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).cuda()
        clip_tables = [torch.tensor([(c, s, 0, 0, 0, 0) for c, s in p], dtype=torch.int32).cuda() for p in picks]

        def other_launches():
            for r in range(reps):
                _lib.check(_lib.lib().vpx_clips_preprocess(_lib.ptr(flat), _lib.FRAMES_U8, int(sum(lengths)), H, W, 3, _lib.ptr(frames_first), len(lengths),
                                                           _lib.ptr(clip_tables[r % ROTATE]), B, FRAMES, 1, H, W, OUT, OUT, 3, 0.0, 1.0, _lib.ptr(outs[r % ROTATE]), stream()),
                           "vpx_clips_preprocess")
        other_name = "vpx_clips_preprocess"
    else:
        # the torch chain: per frame size one view [frames, H, W, 3] per clip is not indexable at once, so per size the clips' frames are
        # gathered through one index over a per-size concatenation made ONCE here (not timed), then resized and scattered into the batch
        groups = {}
        for hw in cfg["sizes"]:
            members = [c for c in range(len(lengths)) if sizes[c] == hw]
            cat = torch.cat([flat[int(first[c]):int(first[c + 1])].view(lengths[c], hw[0], hw[1], 3) for c in members])
            base = dict(zip(members, np.concatenate([[0], np.cumsum([lengths[c] for c in members])]).tolist()))
            groups[hw] = (cat, base)
        plans = []
        for p in picks:
            plan = []
            for hw, (cat, base) in groups.items():
                rows = [b for b, (c, _) in enumerate(p) if sizes[c] == hw]
                idx = torch.tensor([[base[p[b][0]] + p[b][1] + t for t in range(FRAMES)] for b in rows]).cuda()
                plan.append((hw, torch.tensor(rows).cuda(), idx))
            plans.append(plan)

        def chain(r):
            out = torch.empty((B, FRAMES, 3, OUT, OUT), device="cuda")
            for hw, rows, idx in plans[r % ROTATE]:
                x = groups[hw][0][idx].permute(0, 1, 4, 2, 3).float() / 255
                x = torch.nn.functional.interpolate(x.reshape(-1, 3, hw[0], hw[1]), size=(OUT, OUT), mode="bilinear", align_corners=False)
                out.index_copy_(0, rows, x.reshape(len(rows), FRAMES, 3, OUT, OUT))
            return out

        def other_launches():
            for r in range(reps):
                chain(r)
        other_name = "torch chain"

    var_launches()
    torch.cuda.synchronize()
    got = outs[0].clone()
    if equal:
        other_launches()
        torch.cuda.synchronize()
        max_diff = float((outs[0] - got).abs().max())                    # the same destination, written by the other launch: equal bits
    else:
        max_diff = float((got - chain(0)).abs().max())
    ms = {"kernel": [], "other": []}
    for step in range(warmup + steps):
        order = (var_launches, other_launches) if step % 2 == 0 else (other_launches, var_launches)
        t = {fn: _event_ms(fn) / reps for fn in order}
        if step >= warmup:
            ms["kernel"].append(t[var_launches]), ms["other"].append(t[other_launches])
    med = {k: statistics.median(v) for k, v in ms.items()}
    frame_bytes = max(h * w * 3 for h, w in sizes)
    cycle = ROTATE * (B * FRAMES * 3 * OUT * OUT * 4 + B * FRAMES * frame_bytes)
    assert cycle > LLC_BYTES
    res = {"stored_hw": [list(s) for s in cfg["sizes"]], "clip_lengths": lengths, "windows": len(windows), "reps": reps, "against": other_name,
           "kernel_ms": round(med["kernel"], 4), "other_ms": round(med["other"], 4), "bytes_per_cycle": cycle, "max_abs_diff": max_diff}
    res["var_over_clips" if equal else "torch_over_kernel"] = round(med["kernel"] / med["other"], 3) if equal else round(med["other"] / med["kernel"], 2)
    return res


def main():
    from vp_suite_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_var_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"what": "batch(128) of 20 uint8 RGB frames: vpx_clips_preprocess_var (one launch) vs vpx_clips_preprocess at equal 64x64 shapes, and vs the torch chain "
                   "(per frame size: index / permute / .float() / 255 / F.interpolate / index_copy_) on clips of 1000x1000 and 1002x1000 resized to 64x64, same GPU, "
                   "alternating; tables and destinations rotated past the last-level cache; medians", "batch": B, "frames": FRAMES, "returned": [3, OUT, OUT],
           "rotate": ROTATE, "steps": args.steps, "warmup": args.warmup, "cases": {}}
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
