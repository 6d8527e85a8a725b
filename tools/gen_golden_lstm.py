"""Writes the NonConvLSTM fixtures under tests/golden/ from the upstream reference on the CPU (tools/ref_shim.py; build container only):

  lstm_tiny.npz      img_shape (1, 16, 24), bottleneck_dim 24, lstm_hidden_dim 24, 2 layers, B = 2: model.encode(x) and model.decode(z)
                     with the gradients of every encoder / decoder / linear parameter and of the inputs under seeded cotangents, the
                     reference's forward (5 -> 3) and pred_1, per-parameter gradient summaries for sum(pred^2) (parameters whose
                     gradient is None by name), the state_dict key / shape table
  lstm_tiny3.npz     (3, 20, 12), action_conditional, action_size 3 (odd 5x3 and 3x2 maps: replicate taps on the bottom / right edges
                     too): encode, decode, action_inflate and the literal forward (4 -> 2)
  lstm_default.npz   defaults at 1x64x64, B = 1: [::4, ::4] slices and a checksum of decode(encode(x)), n_params, the key table

The reference's forward never advances its LSTM state (vp_suite/models/lstm.py:94-95), so `fwd` is decode(zeros) per frame: the
fixtures pin that literal output, the encoder, the decoder and the parameter table; the carried-state model is held to tests/lstm_ref.py.

torchvision is a MagicMock here and nn.Sequential rejects it, so `vp_suite.models.lstm.TF.Resize` is replaced by a small nn.Module that
calls F.interpolate(x, size, mode="bilinear", align_corners=False). That is what torchvision's Resize does to a float tensor when it
enlarges (antialiasing only ever changes a reduction), and the decoder only enlarges: three transposed layers produce h - 7.

Inputs and parameters are regenerated from seeds by the tests (tests/golden_util.py); the fixtures hold the reference's outputs and
names only. A separate script so that running it cannot touch any other fixture.

    python tools/gen_golden_lstm.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from golden_util import GOLDEN_DIR, checksum, fill_state_dict_, name_seed, seeded_rand, seeded_randn  # noqa: E402
from lstm_ref import (LSTM_DEFAULT_B, LSTM_DEFAULT_KW, LSTM_TINY3_CTX, LSTM_TINY3_KW, LSTM_TINY3_PRED, LSTM_TINY_B, LSTM_TINY_CTX,  # noqa: E402
                      LSTM_TINY_KW, LSTM_TINY_PRED, grad_summary)

torch.set_num_threads(4)
torch.use_deterministic_algorithms(True)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def _save(name, **arrays):
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  wrote {name}.npz  ({size / 1024:.1f} KiB)")
    assert size <= 200 * 1024, f"{name}.npz is larger than 200 KB"


def _sd_meta(module):
    sd = module.state_dict()
    return dict(sd_keys=np.array(sorted(sd.keys())), sd_shapes=np.array(json.dumps({k: list(v.shape) for k, v in sd.items()})))


def _reference():
    ref_shim.load_reference()
    import vp_suite.models.lstm as ref_lstm

    class _Resize(torch.nn.Module):
        def __init__(self, size):
            super().__init__()
            self.size = tuple(size)

        def forward(self, x):
            return torch.nn.functional.interpolate(x, self.size, mode="bilinear", align_corners=False)
    ref_lstm.TF.Resize = _Resize
    return ref_lstm.LSTM


KINK_MARGIN = 2e-6   # ~10x the fp32 rounding of these sums (<= 2304 terms of size <= 0.1: about 2e-7)


def _kink_guard(model):
    """No ReLU input of a pass whose gradients are pinned may sit within fp32 rounding of zero: there ReLU' depends on the accumulation
    order, and a gradient pinned to one side would fail every other correct implementation. While `model.kink_guard` is True a ReLU
    input that close raises; the seed that trips it is changed (tiny3's first latent seed had a dec2 input of 2.6e-8)."""
    def check(_module, args):
        if model.kink_guard:
            smallest = float(args[0].detach().abs().min())
            assert smallest > KINK_MARGIN, f"a ReLU input of {smallest:.2e} is too close to the kink: choose another seed"
    model.kink_guard = False
    model.act_fn.register_forward_pre_hook(check)
    return model


def _put_grads(arrays, prefix, named_grads):
    none = sorted(n for n, g in named_grads.items() if g is None)
    arrays[f"{prefix}.none"] = np.array(none if none else [""])
    summ = grad_summary({n: g for n, g in named_grads.items() if g is not None})
    names = sorted(summ)
    arrays[f"{prefix}.gnames"] = np.array(names)
    arrays[f"{prefix}.gstats"] = np.array([[summ[n][0], summ[n][1], summ[n][2]] for n in names], dtype=np.float64)
    arrays[f"{prefix}.gkept_n"] = np.array([summ[n][3].size for n in names], dtype=np.int64)
    arrays[f"{prefix}.gkept"] = np.concatenate([summ[n][3] for n in names]).astype(np.float32)


def _enc_dec(model, tag, B, arrays):
    """encode / decode of the first frame batch and a seeded latent, with gradients under seeded cotangents."""
    c, h, w = model.img_shape
    x0 = seeded_rand((B, c, h, w), name_seed(f"lstm.{tag}.x0")).requires_grad_(True)
    z = seeded_randn((B, model.lstm_hidden_dim), name_seed(f"lstm.{tag}.latent")).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    model.kink_guard = True
    enc, dec = model.encode(x0), model.decode(z)
    model.kink_guard = False
    ge, gd = seeded_randn(enc.shape, name_seed(f"lstm.{tag}.ge")), seeded_randn(dec.shape, name_seed(f"lstm.{tag}.gd"))
    ((enc * ge).sum() + (dec * gd).sum()).backward()
    arrays.update(enc=_np(enc), dec=_np(dec), chk_x0=checksum(x0), chk_z=checksum(z))
    grads = {n: p.grad for n, p in model.named_parameters()}
    grads["__x0__"], grads["__z__"] = x0.grad, z.grad
    _put_grads(arrays, "ed", grads)


def gen_tiny(LSTM):
    kw, B = LSTM_TINY_KW, LSTM_TINY_B
    model = _kink_guard(LSTM("cpu", **kw))
    fill_state_dict_(model, name_seed("lstm.tiny"))
    c, h, w = kw["img_shape"]
    arrays = {}
    _enc_dec(model, "tiny", B, arrays)
    x = seeded_rand((B, LSTM_TINY_CTX, c, h, w), name_seed("lstm.tiny.x"))
    model.zero_grad(set_to_none=True)
    model.kink_guard = True            # (the forward's gradients all come through decode(zeros))
    model.decode(torch.zeros(B, model.lstm_hidden_dim))
    model.kink_guard = False
    pred, ml = model(x, pred_frames=LSTM_TINY_PRED)
    assert ml is None
    (pred * pred).sum().backward()
    arrays["fwd"] = _np(pred)
    _put_grads(arrays, "fwd", {n: p.grad for n, p in model.named_parameters()})
    with torch.no_grad():
        arrays["pred1"] = _np(model.pred_1(x))
    arrays.update(chk_x=checksum(x), n_params=np.array(sum(p.numel() for p in model.parameters())), **_sd_meta(model))
    _save("lstm_tiny", **arrays)


def gen_tiny3(LSTM):
    kw, B = LSTM_TINY3_KW, LSTM_TINY_B
    model = _kink_guard(LSTM("cpu", **kw))
    fill_state_dict_(model, name_seed("lstm.tiny3"))
    c, h, w = kw["img_shape"]
    arrays = {}
    _enc_dec(model, "tiny3", B, arrays)
    x = seeded_rand((B, LSTM_TINY3_CTX, c, h, w), name_seed("lstm.tiny3.x"))
    actions = seeded_randn((B, LSTM_TINY3_CTX + LSTM_TINY3_PRED, kw["action_size"]), name_seed("lstm.tiny3.actions"))
    with torch.no_grad():
        pred, _ = model(x, pred_frames=LSTM_TINY3_PRED, actions=actions)
        arrays["fwd"] = _np(pred)
        arrays["inflate"] = _np(model.action_inflate(actions[:, 0].flatten(1, -1)))
    arrays.update(chk_x=checksum(x), chk_actions=checksum(actions), n_params=np.array(sum(p.numel() for p in model.parameters())), **_sd_meta(model))
    _save("lstm_tiny3", **arrays)


def gen_default(LSTM):
    model = _kink_guard(LSTM("cpu", **LSTM_DEFAULT_KW))
    fill_state_dict_(model, name_seed("lstm.default"))
    x = seeded_rand((LSTM_DEFAULT_B, 1, 64, 64), name_seed("lstm.default.x"))
    with torch.no_grad():
        z = model.encode(x)
        out = model.decode(z)
    _save("lstm_default", z_slice=_np(z[:, ::4]), out_slice=_np(out[:, :, ::4, ::4]), out_chk=np.float64(checksum(out)), z_chk=np.float64(checksum(z)),
          chk_x=checksum(x), n_params=np.array(sum(p.numel() for p in model.parameters())), **_sd_meta(model))


if __name__ == "__main__":
    LSTM = _reference()
    gen_tiny(LSTM)
    gen_tiny3(LSTM)
    gen_default(LSTM)
