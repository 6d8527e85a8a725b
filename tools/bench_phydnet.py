"""PhyDNet ("phy") throughput on one GPU; prints ONE JSON line.

  * eval: predicted frames/s of the default model at 1x64x64, 10 -> 10, for B in {16, 64}, in f32 and bf16x3;
  * train: ms per training step (forward + moment loss + MSE + backward + fused Adam) at B = 16, 10 + 10 frames, teacher forcing on / off;
  * lib_sha16: sha256[:16] of the library the process loaded.

Timing: HIP events around `--steps` calls after `--warmup` calls, the median step reported (see bench.py for the same conventions).

    python tools/bench_phydnet.py [--steps 10] [--warmup 3] [--profile-step eval|train]

--profile-step runs ONE eval forward (B = 16) or ONE training step and nothing else (for a kernel trace)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _model(precision, device="cuda"):
    from vp_suite_amd.models import MODEL_CLASSES
    torch.manual_seed(0)
    return MODEL_CLASSES["phy"](device, img_shape=(1, 64, 64), action_size=0, tensor_value_range=[0.0, 1.0],
                                cell_precision=precision).to(device)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def _trainer(m, B, teacher_forcing):
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.train import FlatAdam, _link_views
    params = list(m.parameters())
    total = sum(p.numel() for p in params)
    flat_p = torch.empty(total, device="cuda")
    flat_g = torch.zeros(total, device="cuda")
    _link_views(params, flat_p, "data")
    _link_views(params, flat_g, "grad")
    opt = FlatAdam(params, flat_p, flat_g, lr=1e-4)
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    x = torch.rand(B, 20, 1, 64, 64, device="cuda")

    def step():
        loss = m.training_loss(x[:, :10], x[:, 10:], 10, lp, teacher_forcing=teacher_forcing)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-step", choices=["eval", "train"], default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if args.profile_step == "eval":
        m = _model("f32")
        x = torch.rand(16, 10, 1, 64, 64, device="cuda")
        with torch.no_grad():
            m(x, pred_frames=10)
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "eval", "B": 16, "lib_sha16": _lib_sha16()}))
        return
    if args.profile_step == "train":
        _trainer(_model("f32"), 16, False)()
        torch.cuda.synchronize()
        print(json.dumps({"profiled": "train", "B": 16, "lib_sha16": _lib_sha16()}))
        return
    out = {"model": "phy", "img": [1, 64, 64], "context": 10, "pred": 10, "eval": {}, "train_ms": {}, "steps": args.steps,
           "warmup": args.warmup}
    for precision in ("f32", "bf16x3"):
        m = _model(precision)
        for B in (16, 64):
            x = torch.rand(B, 10, 1, 64, 64, device="cuda")

            def fwd():
                with torch.no_grad():
                    m(x, pred_frames=10)
            ms = _time(fwd, args.steps, args.warmup)
            out["eval"][f"{precision}_B{B}"] = {"ms": round(ms, 3), "frames_per_s": round(B * 10 / ms * 1e3, 1)}
        del m
    for tf in (True, False):
        m = _model("f32")
        ms = _time(_trainer(m, 16, tf), args.steps, args.warmup)
        out["train_ms"][f"f32_B16_tf{int(tf)}"] = round(ms, 3)
        del m
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
