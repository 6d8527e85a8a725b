"""Writes the UNet-3D fixtures under tests/golden/ from the upstream reference on the CPU (tools/ref_shim.py; build container only):

  unet3d_blocks.npz    DoubleConv3d (3 -> 4, B 2, T 3, 5x7) and DoubleConv2d (6 -> 4, B 2, 2x3): eval output; training output, the
                       gradients of every parameter and of the input under a seeded cotangent, the BatchNorm buffers after the call
  unet3d_tiny.npz      img_shape (1, 16, 24), features [4, 8], temporal_dim 3, B 2, 5 context -> 3: eval forward and pred_1; a training
                       forward with the loss sum(pred^2), per-parameter gradient summaries, every BatchNorm buffer after it
  unet3d_tiny3.npz     (3, 20, 12), features [4, 8], temporal_dim 2: eval only
  unet3d_default.npz   default model at 1x64x64, temporal_dim 4, B 1, 6 -> 4, eval with seeded running statistics: four offset
                       [::4, ::4] slices, checksum, n_params
Every fixture holds the state_dict table. `TF.resize` is replaced by a function that fails: no case may reach it.

Inputs and parameters are regenerated from seeds by the tests (tests/golden_util.py, tests/test_unet3d_host.py unet3d_fill_).

    python tools/gen_golden_unet3d.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
from golden_util import GOLDEN_DIR, checksum, name_seed, seeded_rand, seeded_randn  # noqa: E402
from test_unet3d_host import (UNET_BLOCKS, UNET_DEFAULT_B, UNET_DEFAULT_CTX, UNET_DEFAULT_KW, UNET_DEFAULT_PRED, UNET_DEFAULT_SLICES,  # noqa: E402
                              UNET_TINY3_KW, UNET_TINY_B, UNET_TINY_CTX, UNET_TINY_KW, UNET_TINY_PRED, buffers_of, grad_summary, tiny_inputs,
                              unet3d_fill_)

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


def _sd_meta(module, prefix=""):
    sd = module.state_dict()
    return {prefix + "sd_keys": np.array(sorted(sd.keys())), prefix + "sd_shapes": np.array(json.dumps({k: list(v.shape) for k, v in sd.items()}))}


def _reference():
    ref_shim.load_reference()
    import vp_suite.models.unet3d as ref_unet
    from vp_suite.model_blocks import DoubleConv2d, DoubleConv3d
    from vp_suite.models import MODEL_CLASSES

    def _never(*a, **k):
        raise AssertionError("TF.resize reached: the fixture sizes must not need it")
    ref_unet.TF.resize = _never
    return MODEL_CLASSES, {"dc3": DoubleConv3d, "dc2": DoubleConv2d}


def _put_grads(arrays, prefix, named_grads):
    summ = grad_summary(named_grads)
    names = sorted(summ)
    arrays[f"{prefix}.gnames"] = np.array(names)
    arrays[f"{prefix}.gstats"] = np.array([[summ[n][0], summ[n][1], summ[n][2]] for n in names], dtype=np.float64)
    arrays[f"{prefix}.gkept_n"] = np.array([summ[n][3].size for n in names], dtype=np.int64)
    arrays[f"{prefix}.gkept"] = np.concatenate([summ[n][3] for n in names]).astype(np.float32)


def _put_buffers(arrays, prefix, module):
    for k, v in buffers_of(module.state_dict()).items():
        arrays[prefix + k] = v.detach().cpu().numpy().copy()


def gen_blocks(blocks):
    arrays = {}
    for tag, case in UNET_BLOCKS.items():
        blk = blocks[tag](in_channels=case["ci"], out_channels=case["co"])
        unet3d_fill_(blk, name_seed(f"unet3d.{tag}"))
        x = seeded_randn(case["shape"], name_seed(f"unet3d.{tag}.x"))
        blk.eval()
        with torch.no_grad():
            arrays[f"{tag}.eval"] = _np(blk(x))
        blk.train()
        xg = x.clone().requires_grad_(True)
        out = blk(xg)
        (out * seeded_randn(out.shape, name_seed(f"unet3d.{tag}.go"))).sum().backward()
        arrays[f"{tag}.train"] = _np(out)
        for n, p in blk.named_parameters():
            arrays[f"{tag}.g.{n}"] = _np(p.grad)
        arrays[f"{tag}.g.__x__"] = _np(xg.grad)
        _put_buffers(arrays, f"{tag}.buf.", blk)
        arrays[f"{tag}.chk_x"] = checksum(x)
        arrays.update(_sd_meta(blk, f"{tag}."))
    _save("unet3d_blocks", **arrays)


def gen_tiny(MC):
    model = MC["unet-3d"]("cpu", **UNET_TINY_KW)
    unet3d_fill_(model, name_seed("unet3d.tiny"))
    x = tiny_inputs()
    arrays = {}
    model.eval()
    with torch.no_grad():
        pred, ml = model(x, pred_frames=UNET_TINY_PRED)
        assert ml is None
        arrays["eval"] = _np(pred)
        arrays["pred1"] = _np(model.pred_1(x))
    model.train()
    pred, _ = model(x, pred_frames=UNET_TINY_PRED)
    (pred * pred).sum().backward()
    arrays["train.frames"] = _np(pred)
    _put_grads(arrays, "train", {n: p.grad for n, p in model.named_parameters()})
    _put_buffers(arrays, "buf.", model)
    assert all(int(v) == UNET_TINY_PRED for k, v in arrays.items() if k.endswith("num_batches_tracked"))
    arrays.update(chk_x=checksum(x), **_sd_meta(model))
    _save("unet3d_tiny", **arrays)


def gen_tiny3(MC):
    model = MC["unet-3d"]("cpu", **UNET_TINY3_KW)
    unet3d_fill_(model, name_seed("unet3d.tiny3")).eval()
    c, h, w = UNET_TINY3_KW["img_shape"]
    x = seeded_rand((UNET_TINY_B, UNET_TINY_CTX, c, h, w), name_seed("unet3d.tiny3.x"))
    with torch.no_grad():
        pred, _ = model(x, pred_frames=UNET_TINY_PRED)
    _save("unet3d_tiny3", eval=_np(pred), chk_x=checksum(x), **_sd_meta(model))


def gen_default(MC):
    model = MC["unet-3d"]("cpu", **UNET_DEFAULT_KW)
    unet3d_fill_(model, name_seed("unet3d.default")).eval()
    x = seeded_rand((UNET_DEFAULT_B, UNET_DEFAULT_CTX, 1, 64, 64), name_seed("unet3d.default.x"))
    with torch.no_grad():
        pred, _ = model(x, pred_frames=UNET_DEFAULT_PRED)
    slices = {f"pred_slice_{oy}{ox}": _np(pred[:, :, :, oy::4, ox::4]) for oy, ox in UNET_DEFAULT_SLICES}
    _save("unet3d_default", **slices, pred_chk=np.float64(checksum(pred)), pred_absmax=np.float64(pred.abs().max()), chk_x=checksum(x),
          n_params=np.array(sum(p.numel() for p in model.parameters())), **_sd_meta(model))


if __name__ == "__main__":
    MC, blocks = _reference()
    gen_blocks(blocks)
    gen_tiny(MC)
    gen_tiny3(MC)
    gen_default(MC)
