"""NonConvLSTM ("nc-lstm") numbers on one GPU; prints ONE JSON line and writes it to profiles/lstm_bench.json.

  * dense: `lstm_ops.dense` against `torch.nn.functional.linear` at M in {16, 64, 128} for (K, N) = (16384, 1024) and (1024, 16384);
  * cell: `lstm_ops.lstm_cell` against `torch.nn.LSTMCell` at those M with Kx = H = 1024;
    both op benchmarks rotate over enough copies of the weights (and inputs) that a pass touches more than 512 MiB, past the 256 MiB
    last-level cache, so every call streams its weights from HBM; the contenders alternate call by call inside one pass, the per-call
    times are HIP events, and the median over `--steps` passes is reported with the algorithmic bytes (weights + activations, once each)
    per second and that as a fraction of the 8 TB/s HBM peak;
  * eval: predicted frames/s of the default model at 1x64x64, 10 -> 10, for B in {16, 64}, and a training step (forward + MSE + backward
    + torch.optim.Adam) at B = 16, 10 + 10 frames — beside the same step of the plain-torch twin `tests/lstm_ref.py` (fp32, same weights,
    same GPU), interleaved;
  * lib_sha16: sha256[:16] of the library the process loaded.

No figure is a pass / fail condition.

    python tools/bench_lstm.py [--steps 10] [--warmup 3] [--no-write]"""
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

KW = dict(img_shape=(1, 64, 64), action_size=0, tensor_value_range=[0.0, 1.0])
HBM_PEAK = 8.0e12          # bytes/s, MI355X
ROTATE_BYTES = 512 << 20   # a pass over the rotated buffers touches at least this much


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _interleaved(fns, n_sets, steps, warmup):
    """Median ms per call of each contender: per pass every contender runs once on every buffer set, alternating call by call."""
    per = [[] for _ in fns]
    for p in range(warmup + steps):
        acc = [0.0] * len(fns)
        for s in range(n_sets):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(s)
                b.record()
                b.synchronize()
                acc[i] += a.elapsed_time(b)
        if p >= warmup:
            for i in range(len(fns)):
                per[i].append(acc[i] / n_sets)
    return [statistics.median(v) for v in per]


def bench_dense(M, K, N, steps, warmup):
    from vp_suite_amd import lstm_ops
    n_sets = max(2, -(-ROTATE_BYTES // (N * K * 4)))
    ws = [torch.randn(N, K, device="cuda") / K ** 0.5 for _ in range(n_sets)]
    xs = [torch.randn(M, K, device="cuda") for _ in range(n_sets)]
    b = torch.randn(N, device="cuda")
    with torch.no_grad():
        ours, ref = _interleaved([lambda s: lstm_ops.dense(xs[s], ws[s], b), lambda s: torch.nn.functional.linear(xs[s], ws[s], b)], n_sets, steps, warmup)
    nbytes = 4 * (N * K + M * K + M * N + N)
    return dict(M=M, K=K, N=N, sets=n_sets, plan=lstm_ops.dense_plan(M, N, K), ms=ours, torch_ms=ref, ratio=ref / ours, bytes=nbytes,
                hbm_fraction=nbytes / (ours * 1e-3) / HBM_PEAK, torch_hbm_fraction=nbytes / (ref * 1e-3) / HBM_PEAK)


def bench_cell(M, H, steps, warmup):
    from vp_suite_amd import lstm_ops
    n_sets = max(2, -(-ROTATE_BYTES // (8 * H * H * 4)))
    cells = [torch.nn.LSTMCell(H, H).cuda() for _ in range(n_sets)]
    x, h, c = (torch.randn(M, H, device="cuda") for _ in range(3))
    with torch.no_grad():
        ours, ref = _interleaved([lambda s: lstm_ops.lstm_cell(x, (h, c), cells[s].weight_ih, cells[s].weight_hh, cells[s].bias_ih, cells[s].bias_hh),
                                  lambda s: cells[s](x, (h, c))], n_sets, steps, warmup)
    nbytes = 4 * (8 * H * H + 8 * H + 5 * M * H)
    return dict(M=M, H=H, sets=n_sets, ms=ours, torch_ms=ref, ratio=ref / ours, bytes=nbytes, hbm_fraction=nbytes / (ours * 1e-3) / HBM_PEAK,
                torch_hbm_fraction=nbytes / (ref * 1e-3) / HBM_PEAK)


def bench_model(steps, warmup):
    import lstm_ref
    from vp_suite_amd.models import MODEL_CLASSES
    torch.manual_seed(0)
    m = MODEL_CLASSES["nc-lstm"]("cuda", **KW).to("cuda")
    twin = lstm_ref.RefLSTM(m.state_dict(), KW["img_shape"], dtype=torch.float32, device="cuda", requires_grad=True)
    out = {}
    for B in (16, 64):
        x = torch.rand(B, 10, 1, 64, 64, device="cuda")
        with torch.no_grad():
            ours, ref = _interleaved([lambda s: m(x, pred_frames=10), lambda s: twin.forward(x, 10)], 1, steps, warmup)
        out[f"eval_b{B}"] = dict(ms=ours, torch_ms=ref, frames_per_s=B * 10 / (ours * 1e-3), torch_frames_per_s=B * 10 / (ref * 1e-3), ratio=ref / ours)
    x, y = torch.rand(16, 10, 1, 64, 64, device="cuda"), torch.rand(16, 10, 1, 64, 64, device="cuda")
    opt_a, opt_b = torch.optim.Adam(m.parameters(), lr=1e-4), torch.optim.Adam(list(twin.p.values()), lr=1e-4)

    def train(fwd, opt):
        opt.zero_grad(set_to_none=True)
        ((fwd(x) - y) ** 2).mean().backward()
        opt.step()
    ours, ref = _interleaved([lambda s: train(lambda v: m(v, pred_frames=10)[0], opt_a), lambda s: train(lambda v: twin.forward(v, 10), opt_b)], 1, steps, warmup)
    out["train_b16"] = dict(ms=ours, torch_ms=ref, ratio=ref / ours)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    res = dict(lib_sha16=_lib_sha16(), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, precision="f32")
    res["dense"] = [bench_dense(M, K, N, args.steps, args.warmup) for (K, N) in ((16384, 1024), (1024, 16384)) for M in (16, 64, 128)]
    res["cell"] = [bench_cell(M, 1024, args.steps, args.warmup) for M in (16, 64, 128)]
    res["model"] = bench_model(args.steps, args.warmup)
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, "profiles", "lstm_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
