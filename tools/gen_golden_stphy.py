"""Writes the ST-Phy fixtures under tests/golden/ from the upstream reference on the CPU (tools/ref_shim.py; build container only):

  stphy_ae.npz        Autoencoder at (1, 32, 40), enc_c = 16: encode, decode, gradient summaries of every parameter and of the input
  stphy_tiny.npz      img_shape (1, 32, 40), 2 layers, 16 channels, moment_loss_scale 0.5, B = 2: eval 4 -> 3, pred_1, training forwards
                      (3 + 3 frames, teacher forcing off / on) with frames, both model losses, the total and per-parameter gradient
                      summaries; parameters whose gradient is None are recorded by name
  stphy_tiny3.npz     (3, 40, 32), 3 layers, 16 channels: eval only
  stphy_default.npz   default model, B = 1, 10 -> 10 eval: pred[..., ::4, ::4] and three offset slices, checksum, state_dict table, n_params

Inputs and parameters are regenerated from seeds by the tests (tests/golden_util.py); the fixtures hold the reference's outputs and
names only. A separate script from tools/gen_golden.py so that running it cannot touch any other fixture.

    python tools/gen_golden_stphy.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from golden_util import GOLDEN_DIR, checksum, name_seed, seeded_rand, seeded_randn  # noqa: E402
from test_stphy_host import (STPHY_AE_B, STPHY_AE_ENC_C, STPHY_AE_SHAPE, STPHY_DEFAULT_B, STPHY_DEFAULT_CTX, STPHY_DEFAULT_KW,  # noqa: E402
                             STPHY_DEFAULT_PRED, STPHY_DEFAULT_SLICES, STPHY_TINY3_KW, STPHY_TINY_B, STPHY_TINY_CTX, STPHY_TINY_KW, STPHY_TINY_PRED,
                             STPHY_TRAIN_CTX, STPHY_TRAIN_PRED, grad_summary, stphy_fill_)

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
    import json
    sd = module.state_dict()
    return dict(sd_keys=np.array(sorted(sd.keys())), sd_shapes=np.array(json.dumps({k: list(v.shape) for k, v in sd.items()})))


def _reference():
    """The reference's model registry and Autoencoder with the decoder's `TF.Resize` replaced by a size-asserting identity (torchvision is
    a stub here; at the sizes used Resize is the identity)."""
    ref_shim.load_reference()
    import vp_suite.model_blocks.enc as ref_enc
    from vp_suite.models import MODEL_CLASSES

    class _SameSize(torch.nn.Module):
        def __init__(self, size):
            super().__init__()
            self.size = tuple(size)

        def forward(self, x):
            assert tuple(x.shape[-2:]) == self.size, (tuple(x.shape), self.size)
            return x
    ref_enc.TF.Resize = _SameSize
    return MODEL_CLASSES, ref_enc.Autoencoder


def _loss_provider(img_c):
    from vp_suite.measure.loss_provider import PredictionLossProvider
    return PredictionLossProvider({"device": "cpu", "losses_and_scales": {"mse": 1.0}, "img_c": img_c})


def _put_grads(arrays, prefix, named_grads):
    """One table per pass (an .npz entry costs ~250 bytes of headers): names of the parameters with a gradient, their (sum, sum of
    squares, max |g|) rows, the kept elements back to back with their counts; the parameters whose gradient is None by name."""
    none = sorted(n for n, g in named_grads.items() if g is None)
    arrays[f"{prefix}.none"] = np.array(none if none else [""])
    summ = grad_summary({n: g for n, g in named_grads.items() if g is not None})
    names = sorted(summ)
    arrays[f"{prefix}.gnames"] = np.array(names)
    arrays[f"{prefix}.gstats"] = np.array([[summ[n][0], summ[n][1], summ[n][2]] for n in names], dtype=np.float64)
    arrays[f"{prefix}.gkept_n"] = np.array([summ[n][3].size for n in names], dtype=np.int64)
    arrays[f"{prefix}.gkept"] = np.concatenate([summ[n][3] for n in names]).astype(np.float32)


def gen_ae(AE):
    c, h, w = STPHY_AE_SHAPE
    ae = AE(STPHY_AE_SHAPE, STPHY_AE_ENC_C, "cpu")
    stphy_fill_(ae, name_seed("stphy.ae"))
    x = seeded_rand((STPHY_AE_B, c, h, w), name_seed("stphy.ae.x")).requires_grad_(True)
    z = ae.encode(x)
    out = ae.decode(z)
    gz = seeded_randn(z.shape, name_seed("stphy.ae.gz"))
    go = seeded_randn(out.shape, name_seed("stphy.ae.go"))
    ((z * gz).sum() + (out * go).sum()).backward()
    arrays = dict(z=_np(z), out=_np(out), chk_x=checksum(x), encoded_shape=np.array(list(ae.encoded_shape)))
    grads = {n: p.grad for n, p in ae.named_parameters()}
    grads["__x__"] = x.grad
    _put_grads(arrays, "g", grads)
    arrays.update(_sd_meta(ae))
    _save("stphy_ae", **arrays)


def gen_tiny(MC):
    kw, B = STPHY_TINY_KW, STPHY_TINY_B
    model = MC["st-phy"]("cpu", **kw)
    stphy_fill_(model, name_seed("stphy.tiny"))
    c, h, w = kw["img_shape"]
    arrays = {}
    x = seeded_rand((B, STPHY_TINY_CTX, c, h, w), name_seed("stphy.tiny.x"))
    with torch.no_grad():
        pred, ml = model(x, pred_frames=STPHY_TINY_PRED)
        assert ml is None
        arrays["eval"] = _np(pred)
        arrays["pred1"] = _np(model.pred_1(x))
    xt = seeded_rand((B, STPHY_TRAIN_CTX + STPHY_TRAIN_PRED, c, h, w), name_seed("stphy.tiny.xt"))
    lp = _loss_provider(c)
    for tf in (False, True):
        model.zero_grad(set_to_none=True)
        out, ml = model(xt, pred_frames=STPHY_TRAIN_PRED, train=True, teacher_forcing=tf)
        _, total = lp.get_losses(out, xt[:, 1:])
        for v in ml.values():
            total = total + v
        total.backward()
        k = f"tf{int(tf)}"
        arrays[f"{k}.frames"] = _np(out)
        arrays[f"{k}.moment"] = np.float64(ml["moment regularization loss"].item())
        arrays[f"{k}.decouple"] = np.float64(ml["memory decoupling loss"].item())
        arrays[f"{k}.total"] = np.float64(total.item())
        _put_grads(arrays, k, {n: p.grad for n, p in model.named_parameters()})
    arrays.update(chk_x=checksum(x), chk_xt=checksum(xt))
    arrays.update(_sd_meta(model))
    _save("stphy_tiny", **arrays)


def gen_tiny3(MC):
    kw, B = STPHY_TINY3_KW, STPHY_TINY_B
    model = MC["st-phy"]("cpu", **kw)
    stphy_fill_(model, name_seed("stphy.tiny3"))
    c, h, w = kw["img_shape"]
    x = seeded_rand((B, STPHY_TINY_CTX, c, h, w), name_seed("stphy.tiny3.x"))
    with torch.no_grad():
        pred, _ = model(x, pred_frames=STPHY_TINY_PRED)
    _save("stphy_tiny3", eval=_np(pred), chk_x=checksum(x), **_sd_meta(model))


def gen_default(MC):
    model = MC["st-phy"]("cpu", **STPHY_DEFAULT_KW)
    stphy_fill_(model, name_seed("stphy.default"))
    x = seeded_rand((STPHY_DEFAULT_B, STPHY_DEFAULT_CTX, 1, 64, 64), name_seed("stphy.default.x"))
    with torch.no_grad():
        pred, _ = model(x, pred_frames=STPHY_DEFAULT_PRED)
    more = {f"pred_slice_{oy}{ox}": _np(pred[:, :, :, oy::4, ox::4]) for oy, ox in STPHY_DEFAULT_SLICES}
    _save("stphy_default", pred_slice=_np(pred[:, :, :, ::4, ::4]), **more, pred_chk=np.float64(checksum(pred)), chk_x=checksum(x),
          n_params=np.array(sum(p.numel() for p in model.parameters())), **_sd_meta(model))


if __name__ == "__main__":
    MC, AE = _reference()
    gen_ae(AE)
    gen_tiny(MC)
    gen_tiny3(MC)
    gen_default(MC)
