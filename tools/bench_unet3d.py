"""UNet-3D ("unet-3d") throughput on one GPU; prints ONE JSON line and writes it to profiles/unet3d_bench.json.

  * eval: predicted frames/s of the default model at 1x64x64, temporal_dim 4, 6 -> 4, for B in {16, 64};
  * train: ms per training step (train()-mode forward + sum(pred^2)-style MSE + backward + torch.optim.Adam) at B = 16;
  * beside each, the same step of tests/unet3d_ref.py (plain torch ops on the same GPU, fp32, the same weights), timed by the same
    function, library and reference INTERLEAVED call by call so that both see the same clocks;
  * launches_per_pred_1: kernel launches of one pred_1 of the library path in eval() and in train() mode, both under no_grad (the
    train() count leaves out what a call that keeps state for its backward would add); torch profiler, its own run;
  * lib_sha16: sha256[:16] of the library the process loaded.

Timing: HIP events around `--steps` calls after `--warmup` calls, the median step reported (see bench.py for the same conventions).

    python tools/bench_unet3d.py [--steps 10] [--warmup 3] [--no-write]"""
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

KW = dict(img_shape=(1, 64, 64), action_size=0, tensor_value_range=[0.0, 1.0], temporal_dim=4)
CTX, PRED = 6, 4


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _model():
    from vp_suite_amd.models import MODEL_CLASSES
    torch.manual_seed(0)
    return MODEL_CLASSES["unet-3d"]("cuda", **KW)


def _time_pair(fa, fb, steps, warmup):
    """Median ms of fa and of fb, their calls interleaved."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(steps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return statistics.median(ms[0]), statistics.median(ms[1])


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import unet3d_ref
    out = {"model": "unet-3d", "img": [1, 64, 64], "temporal_dim": 4, "context": CTX, "pred": PRED, "eval": {}, "eval_torch_ref": {}, "train_ms": {},
           "train_ms_torch_ref": {}, "steps": args.steps, "warmup": args.warmup}
    m = _model().eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for B in (16, 64):
        x = torch.rand(B, CTX, 1, 64, 64, device="cuda")

        def fwd():
            with torch.no_grad():
                m(x, pred_frames=PRED)

        def fwd_ref():
            with torch.no_grad():
                unet3d_ref.forward(sd, x, PRED)
        ms, ms_ref = _time_pair(fwd, fwd_ref, args.steps, args.warmup)
        out["eval"][f"f32_B{B}"] = {"ms": round(ms, 3), "frames_per_s": round(B * PRED / ms * 1e3, 1)}
        out["eval_torch_ref"][f"f32_B{B}"] = {"ms": round(ms_ref, 3), "frames_per_s": round(B * PRED / ms_ref * 1e3, 1)}

    x = torch.rand(16, CTX + PRED, 1, 64, 64, device="cuda")
    m = _model().train()
    opt = torch.optim.Adam(list(m.parameters()), lr=1e-4)
    m_ref = _model()
    sd_ref = {**dict(m_ref.named_buffers()), **dict(m_ref.named_parameters())}
    opt_ref = torch.optim.Adam(list(m_ref.parameters()), lr=1e-4)

    def step():
        pred, _ = m(x[:, :CTX], pred_frames=PRED)
        loss = ((pred - x[:, CTX:]) ** 2).sum(dim=(2, 3, 4)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()

    def step_ref():
        pred, _ = unet3d_ref.forward(sd_ref, x[:, :CTX], PRED, training=True)
        loss = ((pred - x[:, CTX:]) ** 2).sum(dim=(2, 3, 4)).mean()
        opt_ref.zero_grad()
        loss.backward()
        opt_ref.step()
    ms, ms_ref = _time_pair(step, step_ref, args.steps, args.warmup)
    out["train_ms"]["f32_B16"], out["train_ms_torch_ref"]["f32_B16"] = round(ms, 3), round(ms_ref, 3)

    x1 = torch.rand(16, CTX, 1, 64, 64, device="cuda")

    def one_pred():
        with torch.no_grad():
            m.pred_1(x1)
    m.eval()
    n_eval = _launches(one_pred)
    m.train()
    out["launches_per_pred_1"] = {"eval": n_eval, "train_forward_no_grad": _launches(one_pred)}     # (train() mode's batch statistics, nothing kept for a backward)
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, "profiles", "unet3d_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
