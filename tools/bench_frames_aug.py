"""Photometric augmentations and erasing of stored Moving MNIST batches (csrc/frames_aug.hip through datasets.StoredVPDataset.batch)
against the plain-torch expression chain on the same GPU, interleaved; prints ONE JSON line and writes it to
profiles/frames_aug_bench.json.

batch(128) of 20 stored 64x64 gray frames out of 1024 stored sequences (uint8, on the device) to 3x64x64, three configurations:
  * none        no augmentation: the preprocess launch alone (no second launch)
  * pointwise   invert, brightness, normalize: one sweep
  * full        colour jitter (brightness, contrast, saturation, hue) + autocontrast + erasing: three sweeps (two statistics)
Per configuration:
  * batch_ms    wall time of ds.batch(indices): host draws, table and program copies, the launches, zero actions, synchronised
  * kernel_ms   HIP events around one vpx_frames_augment call per buffer over ROTATE preprocessed batches (programs already on the device),
                per call; the buffers (ROTATE x 126 MB) exceed the L2 and most of the Infinity Cache, so a call does not find its frames cached
  * torch_ms    the same programs as plain-torch expressions (per-sample parameters as broadcast tensors) over the same rotated buffers
  * GBps        algorithmic bytes = 8 B per element per sweep (one read, one write) / kernel_ms, and its share of the HBM roofline
The torch chain computes the same formulas (its hue through the same _rgb2hsv / _hsv2rgb expressions); max_abs_diff_vs_torch says how
close. Medians over --steps measured passes after --warmup; the library and the torch chain alternate inside every pass.

    python tools/bench_frames_aug.py [--steps 20] [--warmup 3] [--out FILE]"""
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
ROTATE = 4
HBM_ROOFLINE_TBPS = 6.3    # achievable HBM bandwidth the project's rooflines use
CONFIGS = {"none": [],
           "pointwise": [("invert", 1.0), ("color_jitter", 0.4, 0, 0, 0), ("normalize", (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))],
           "full": [("color_jitter", 0.4, 0.4, 0.4, 0.1), ("autocontrast", 1.0), ("erase", 1.0, (0.02, 0.33), (0.3, 3.3), 0.0)]}


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


def _gray(x):
    return (0.2989 * x[:, :, 0] + 0.587 * x[:, :, 1] + 0.114 * x[:, :, 2]).unsqueeze(2)


def _hue(x, d):
    r, g, b = x.unbind(2)
    maxc, minc = x.max(2).values, x.min(2).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = (maxc == r) * (bc - gc) + ((maxc == g) & (maxc != r)) * (2.0 + rc - bc) + ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod(h / 6.0 + 1.0, 1.0)
    h = (h + d) % 1.0
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (maxc * (1.0 - s)).clamp(0.0, 1.0)
    q = (maxc * (1.0 - f * s)).clamp(0.0, 1.0)
    t = (maxc * (1.0 - (1.0 - f) * s)).clamp(0.0, 1.0)
    pick = lambda six: torch.gather(torch.stack(six, 0), 0, i.unsqueeze(0)).squeeze(0)
    return torch.stack([pick([maxc, q, p, p, t, maxc]), pick([t, maxc, maxc, q, p, p]), pick([p, p, t, maxc, maxc, q])], 2)


def torch_chain(x, programs, side):
    """The programs of one batch as plain-torch expressions over x [B, F, 3, h, w] (per-sample parameters as [B, 1, 1, 1, 1] tensors; every
    sample of a benchmark batch runs the same operations in its own drawn order, so the chain follows sample 0's order per group of equal orders)."""
    from vp_suite_amd.datasets import base as D
    out = torch.empty_like(x)
    orders = {}
    for k, rows in enumerate(programs):
        orders.setdefault(tuple(int(r[0]) for r in rows), []).append(k)
    for order, members in orders.items():
        idx = torch.tensor(members, device=x.device)
        v = x[idx]
        for j, op in enumerate(order):
            par = torch.tensor([programs[k][j][1:] for k in members], dtype=torch.float32, device=x.device)
            col = lambda c: par[:, c].view(-1, 1, 1, 1, 1)
            if op == D.OP_INVERT:
                v = 1.0 - v
            elif op == D.OP_NORMALIZE:
                v = (v - par[:, 0:3].view(-1, 1, 3, 1, 1)) / par[:, 4:7].view(-1, 1, 3, 1, 1)
            elif op == D.OP_BRIGHTNESS:
                v = (col(0) * v).clamp(0.0, 1.0)
            elif op == D.OP_CONTRAST:
                v = (col(0) * v + col(1) * _gray(v).mean(dim=(2, 3, 4), keepdim=True)).clamp(0.0, 1.0)
            elif op == D.OP_SATURATION:
                v = (col(0) * v + col(1) * _gray(v)).clamp(0.0, 1.0)
            elif op == D.OP_HUE:
                v = _hue(v, col(0).view(-1, 1, 1, 1))
            elif op == D.OP_AUTOCONTRAST:
                lo, hi = v.amin(dim=(3, 4), keepdim=True), v.amax(dim=(3, 4), keepdim=True)
                const = hi == lo
                v = torch.where(const, v, ((v - lo) * (1.0 / torch.where(const, torch.ones_like(hi), hi - lo))).clamp(0.0, 1.0))
            elif op == D.OP_ERASE:
                ys = torch.arange(side, device=x.device).view(1, 1, 1, side, 1)
                xs = torch.arange(side, device=x.device).view(1, 1, 1, 1, side)
                inside = (ys >= col(0)) & (ys < col(0) + col(2)) & (xs >= col(1)) & (xs < col(1) + col(3))
                v = torch.where(inside, par[:, 4:7].view(-1, 1, 3, 1, 1), v)
            else:
                raise ValueError(op)
        out[idx] = v
    return out


def main():
    from vp_suite_amd import _lib
    from vp_suite_amd.datasets import StoredVPDataset
    from vp_suite_amd.datasets.base import pack_programs
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_aug_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 256, size=(N_SEQS, FRAMES, SIDE, SIDE), dtype=np.uint8)
    elements = B * FRAMES * 3 * SIDE * SIDE
    out = {"what": "StoredVPDataset.batch(128) with photometric programs (csrc/frames_aug.hip, one launch after the preprocess launch) vs the same programs as "
                   "plain-torch expressions on the same GPU, interleaved, over rotated buffers; medians; GBps over 8 B per element per sweep",
           "stored": [N_SEQS, FRAMES, SIDE, SIDE], "batch": B, "frames": [FRAMES, 3, SIDE, SIDE], "rotate": ROTATE, "steps": args.steps, "warmup": args.warmup,
           "hbm_roofline_TBps": HBM_ROOFLINE_TBPS, "cases": {}}
    for name, augs in CONFIGS.items():
        class Gray3(StoredVPDataset):
            OUT_CHANNELS = 3
        ds = Gray3("train", raw=raw, augmentations=augs)
        ds.set_seq_len(10, 10, 1)
        indices = rng.permutation(N_SEQS)[:B].tolist()
        _, programs = ds.draws(indices)
        ds.reset_rng()
        case = {"operations": [a[0] for a in augs]}
        if not any(programs):
            ms = [_wall_ms(lambda: ds.batch(indices)) for _ in range(args.warmup + args.steps)][args.warmup:]
            case.update({"batch_ms": round(statistics.median(ms), 4), "sweeps": 0, "second_launch": False})
            out["cases"][name] = case
            continue
        sweeps = 1 + max(sum(int(r[0]) in (3, 7) for r in rows) for rows in programs)
        table = torch.from_numpy(pack_programs(programs)).cuda()
        ds.photometric, keep = [], ds.photometric
        base = ds.batch(indices)["frames"]                                     # the preprocess output the programs act on
        ds.photometric = keep
        bufs = [base.clone() for _ in range(ROTATE)]

        def launches():
            for buf in bufs:
                _lib.check(_lib.lib().vpx_frames_augment(_lib.ptr(buf), _lib.ptr(table), B, FRAMES, 3, SIDE, SIDE, int(table.shape[1]),
                                                         torch.cuda.current_stream().cuda_stream), "vpx_frames_augment")

        def chains():
            for buf in bufs:
                torch_chain(buf, programs, SIDE)

        def refill():
            for buf in bufs:
                buf.copy_(base)
        launches()
        got = bufs[0].clone()
        refill()
        want = torch_chain(bufs[0], programs, SIDE)
        torch.cuda.synchronize()
        diff = (got - want).abs()
        max_diff = float(diff[torch.isfinite(diff)].max())
        ms = {"batch": [], "kernel": [], "torch": []}
        for step in range(args.warmup + args.steps):
            tb = _wall_ms(lambda: ds.batch(indices))
            refill()
            tk = _event_ms(launches) / ROTATE
            refill()
            tt = _event_ms(chains) / ROTATE
            if step >= args.warmup:
                ms["batch"].append(tb), ms["kernel"].append(tk), ms["torch"].append(tt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = 8 * elements * sweeps
        gbps = nbytes / (med["kernel"] * 1e-3) / 1e9
        case.update({"batch_ms": round(med["batch"], 4), "kernel_ms": round(med["kernel"], 4), "torch_ms": round(med["torch"], 4),
                     "torch_over_kernel": round(med["torch"] / med["kernel"], 2), "sweeps": sweeps, "algorithmic_bytes": nbytes,
                     "kernel_GBps": round(gbps, 1), "share_of_hbm_roofline": round(gbps / 1e3 / HBM_ROOFLINE_TBPS, 3),
                     "single_pass_GBps": round(8 * elements / (med["kernel"] * 1e-3) / 1e9, 1), "max_abs_diff_vs_torch": max_diff, "second_launch": True})
        out["cases"][name] = case
    with open(_lib.LIB_PATH, "rb") as fh:
        out["lib_sha16"] = hashlib.sha256(fh.read()).hexdigest()[:16]
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
