"""FVD: the library against the plain-torch chain on the same GPU -> profiles/fvd_bench.json.

Both sides run the same folded I3D weights (a seeded network at the real widths, tests/fvd_ref.py) on 64x64x3 clips of 10 and 16 frames at
B = 1, 16, 64, prediction and target as one batch of 2B. Trunk and distance are timed separately. The two sides alternate call by call
(interleaved), and every trunk call takes the next of a ring of clip batches of more than 512 MiB in all (rotated), beyond the last-level
cache, so neither side profits from what the other left there. The distance's inputs are feature tables of a few hundred KB: its ring of 16
only keeps the two sides off each other's buffers and stays cache-resident, as the tables are in use. Medians over the steps after a warm-up.
Usage: python tools/bench_fvd.py [--steps 10] [--warmup 3] [--out profiles/fvd_bench.json]"""
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

import fvd_ref  # noqa: E402
from vp_suite_amd import _lib, measure as M, ops  # noqa: E402

DEV = "cuda:0"
RING_BYTES = 512 << 20


def torch_features(clips, weights):
    return M._fvd_features_host(clips, weights)   # plain torch (F.conv3d / F.max_pool3d on the folded weights), here on GPU tensors


def timed(fn_pairs, ring, steps, warmup):
    """fn_pairs: {name: fn(input)}; the sides alternate, each call on the ring's next entry. Returns {name: median ms}."""
    times = {k: [] for k in fn_pairs}
    i = 0
    for step in range(warmup + steps):
        for name, fn in fn_pairs.items():
            x = ring[i % len(ring)]
            i += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(x)
            e1.record()
            e1.synchronize()
            if step >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fvd_bench.json"))
    args = ap.parse_args()
    M.register_fvd_weights(fvd_ref.state_dict(1))
    trunk = M.fvd_weights(DEV)
    host = {k: (w.float().to(DEV), b.float().to(DEV)) for k, (w, b) in M.fvd_weights("cpu", torch.float64).items()}
    with open(_lib.LIB_PATH, "rb") as fh:
        lib_id = hashlib.sha256(fh.read()).hexdigest()[:16]
    rows = []
    with torch.no_grad():
        for T in (10, 16):
            for B in (1, 16, 64):
                clip_bytes = 2 * B * T * 3 * 64 * 64 * 4
                n_ring = max(2, RING_BYTES // clip_bytes + 1)   # more than 512 MiB of clips: beyond the 256 MB last-level cache at every B
                ring = [torch.rand(2 * B, T, 3, 64, 64, device=DEV) * 2 - 1 for _ in range(n_ring)]
                t = timed({"library": lambda x: ops.fvd_features(x[:B], trunk, x[B:]), "torch": lambda x: torch_features(x, host)}, ring, args.steps, args.warmup)
                feats = [torch.randn(2 * B, trunk["n_features"], device=DEV) for _ in range(16)]
                d = timed({"library": lambda f: ops.frechet_distance(f[:B], f[B:]), "torch": lambda f: M.frechet_distance_host(f[:B], f[B:])}, feats, args.steps, args.warmup)
                rows.append({"T": T, "B": B, "trunk_ms": t, "distance_ms": d, "ring": n_ring})
                print(rows[-1], flush=True)
                del ring
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"what": "FVD on one MI355X: ops.fvd_features / ops.frechet_distance against the plain-torch chain on the same GPU, interleaved; clip batches rotated through a ring of more than 512 MiB, feature tables (cache-resident) through a ring of 16; "
                           "64x64x3 clips, real I3D widths, seeded weights, prediction and target as one batch of 2B; medians in ms",
                   "library": lib_id, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
