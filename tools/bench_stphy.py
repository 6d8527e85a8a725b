"""ST-Phy ("st-phy") throughput on one GPU; prints ONE JSON line and writes it to profiles/stphy_bench.json.

  * eval: predicted frames/s of the default model at 1x64x64, 10 -> 10, for B in {16, 64}, in f32 and bf16x3;
  * train: ms per training step (forward + both model losses + MSE + backward + fused Adam) at B = 16, 10 + 10 frames, teacher forcing
    on / off;
  * beside each, the same step of tests/stphy_ref.py (plain torch ops on the same GPU, fp32, the same weights; its training step uses
    torch.optim.Adam), timed by the same function;
  * lib_sha16: sha256[:16] of the library the process loaded.

Timing: HIP events around `--steps` calls after `--warmup` calls, the median step reported (see bench.py for the same conventions).

    python tools/bench_stphy.py [--steps 10] [--warmup 3] [--profile-step eval|train] [--no-write]

--profile-step runs ONE eval forward (B = 16) or ONE training step of the library path and nothing else (for a kernel trace; timing and
tracing are separate runs)."""
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


def _lib_sha16():
    from vp_suite_amd import _lib
    with open(_lib.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def _model(precision, device="cuda"):
    from vp_suite_amd.models import MODEL_CLASSES
    torch.manual_seed(0)
    return MODEL_CLASSES["st-phy"](device, cell_precision=precision, **KW).to(device)


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


def _ref_trainer(m, B, teacher_forcing):
    """The same training step in plain torch ops: tests/stphy_ref.py over the model's own parameters, MSE as the loss provider sums it
    (per-frame sum, mean over frames), torch.optim.Adam."""
    import stphy_ref
    sd = dict(m.named_parameters())
    opt = torch.optim.Adam(list(m.parameters()), lr=1e-4)
    x = torch.rand(B, 20, 1, 64, 64, device="cuda")

    def step():
        out, ml = stphy_ref.forward(sd, x, 10, num_layers=m.num_layers, train=True, teacher_forcing=teacher_forcing,
                                    moment_loss_scale=m.moment_loss_scale, decoupling_loss_scale=m.decoupling_loss_scale)
        loss = ((out - x[:, 1:]) ** 2).sum(dim=(2, 3, 4)).mean() + sum(ml.values())
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-step", choices=["eval", "train"], default=None)
    ap.add_argument("--no-write", action="store_true")
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
    import stphy_ref
    out = {"model": "st-phy", "img": [1, 64, 64], "context": 10, "pred": 10, "eval": {}, "eval_torch_ref": {}, "train_ms": {},
           "train_ms_torch_ref": {}, "steps": args.steps, "warmup": args.warmup}
    for precision in ("f32", "bf16x3"):
        m = _model(precision)
        sd = {k: v.detach() for k, v in m.state_dict().items()}
        for B in (16, 64):
            x = torch.rand(B, 10, 1, 64, 64, device="cuda")

            def fwd():
                with torch.no_grad():
                    m(x, pred_frames=10)

            def fwd_ref():
                with torch.no_grad():
                    stphy_ref.forward(sd, x, 10, num_layers=m.num_layers)
            ms = _time(fwd, args.steps, args.warmup)
            out["eval"][f"{precision}_B{B}"] = {"ms": round(ms, 3), "frames_per_s": round(B * 10 / ms * 1e3, 1)}
            if precision == "f32":
                ms = _time(fwd_ref, args.steps, args.warmup)
                out["eval_torch_ref"][f"f32_B{B}"] = {"ms": round(ms, 3), "frames_per_s": round(B * 10 / ms * 1e3, 1)}
        del m
    for tf in (True, False):
        m = _model("f32")
        out["train_ms"][f"f32_B16_tf{int(tf)}"] = round(_time(_trainer(m, 16, tf), args.steps, args.warmup), 3)
        m = _model("f32")
        out["train_ms_torch_ref"][f"f32_B16_tf{int(tf)}"] = round(_time(_ref_trainer(m, 16, tf), args.steps, args.warmup), 3)
        del m
    out["lib_sha16"] = _lib_sha16()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, "profiles", "stphy_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
