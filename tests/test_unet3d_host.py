"""UNet-3D ("unet-3d") on the host, no GPU: registry, constructor contract (state_dict keys / shapes / n_params against the reference's,
pinned in tests/golden/unet3d_*.npz), pickling, the errors the port raises, the plain-torch restatement (tests/unet3d_ref.py) against
the reference's fixture, and the dry-run workspace contract (VPX_OPT_DRY_RUN, see test_workspace_contract.py) of the new entry points.

Also the case table of the UNet-3D fixtures, shared with test_gpu_unet3d.py and tools/gen_golden_unet3d.py."""
import ctypes
import itertools
import json
import pickle

import numpy as np
import pytest
import torch

from golden_util import checksum, fill_state_dict_, load_golden, name_seed, seeded_rand

# ---- fixture cases (tools/gen_golden_unet3d.py) -------------------------------------------------------------------------------------
_BASE = dict(action_size=0, tensor_value_range=[0.0, 1.0])
UNET_TINY_KW = dict(img_shape=(1, 16, 24), features=[4, 8], temporal_dim=3, **_BASE)
UNET_TINY3_KW = dict(img_shape=(3, 20, 12), features=[4, 8], temporal_dim=2, **_BASE)
UNET_DEFAULT_KW = dict(img_shape=(1, 64, 64), temporal_dim=4, **_BASE)
UNET_TINY_B, UNET_TINY_CTX, UNET_TINY_PRED = 2, 5, 3
UNET_DEFAULT_B, UNET_DEFAULT_CTX, UNET_DEFAULT_PRED = 1, 6, 4
UNET_DEFAULT_SLICES = ((0, 0), (2, 2), (1, 3), (3, 1))        # offsets of the default fixture's [oy::4, ox::4] slices
UNET_BLOCKS = {"dc3": dict(dims=3, ci=3, co=4, shape=(2, 3, 3, 5, 7)),      # DoubleConv3d on [B, Ci, T, H, W]
               "dc2": dict(dims=2, ci=6, co=4, shape=(2, 6, 2, 3))}         # DoubleConv2d on [B, Ci, H, W]
GRAD_SLICE, GRAD_FULL_MAX = 97, 64      # gradient summaries keep every 97th element (at most 64) of tensors larger than 64 elements


def unet3d_fill_(module, seed):
    """fill_state_dict_, then every BatchNorm scale moved to 1 + 0.1 N(0,1) (away from 0) and every running variance to
    0.5 + 5 |0.1 N(0,1)| (positive, of the order of the activations' variance): non-trivial running statistics."""
    fill_state_dict_(module, seed)
    with torch.no_grad():
        for k, t in module.state_dict().items():
            if k.endswith("running_var"):
                t.copy_(0.5 + 5.0 * t.abs())
            elif k.endswith(".weight") and t.dim() == 1:
                t.add_(1.0)
    return module


def grad_kept(a):
    return a if a.size <= GRAD_FULL_MAX else a[::GRAD_SLICE][:64]


def grad_summary(named_grads):
    """{name: (sum, sum of squares, max |g|, the elements kept)} of fp64 numpy copies."""
    out = {}
    for k, g in named_grads.items():
        a = g.detach().cpu().double().numpy().reshape(-1)
        out[k] = (a.sum(), (a * a).sum(), np.abs(a).max(), grad_kept(a))
    return out


def fixture_grads(g, prefix):
    """{name: (stats row, kept elements)} of a gradient table written by tools/gen_golden_unet3d.py."""
    names = [str(n) for n in g[f"{prefix}.gnames"]]
    offs = np.concatenate([[0], np.cumsum(g[f"{prefix}.gkept_n"])])
    return {n: (g[f"{prefix}.gstats"][i], g[f"{prefix}.gkept"][offs[i]:offs[i + 1]]) for i, n in enumerate(names)}


def tiny_inputs():
    c, h, w = UNET_TINY_KW["img_shape"]
    return seeded_rand((UNET_TINY_B, UNET_TINY_CTX, c, h, w), name_seed("unet3d.tiny.x"))


def buffers_of(sd):
    return {k: v for k, v in sd.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


# ---- host tests -------------------------------------------------------------------------------------------------------------------
def test_unet3d_is_registered(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    assert "unet-3d" in MODEL_CLASSES
    M = MODEL_CLASSES["unet-3d"]
    assert M.NAME == "UNet-3D" and not M.CAN_HANDLE_ACTIONS and "temporal_dim" in M.REQUIRED_ARGS
    assert M("cpu", **UNET_TINY_KW).MIN_CONTEXT_FRAMES == 3


@pytest.mark.parametrize("tag,kw", [("unet3d_tiny", UNET_TINY_KW), ("unet3d_tiny3", UNET_TINY3_KW), ("unet3d_default", UNET_DEFAULT_KW)])
def test_unet3d_state_dict_matches_reference_on_cpu(vpx, tag, kw):
    from vp_suite_amd.models import MODEL_CLASSES
    g = load_golden(tag)
    model = MODEL_CLASSES["unet-3d"]("cpu", **kw)
    sd = model.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert {k: list(v.shape) for k, v in sd.items()} == json.loads(str(g["sd_shapes"]))
    if tag == "unet3d_default":
        assert len(sd) == 128
        assert sum(p.numel() for p in model.parameters()) == int(g["n_params"]) == 671185


def test_double_conv_blocks_have_the_reference_trees(vpx):
    from vp_suite_amd.model_blocks import DoubleConv2d, DoubleConv3d
    g = load_golden("unet3d_blocks")
    for tag, cls in (("dc3", DoubleConv3d), ("dc2", DoubleConv2d)):
        blk = cls(in_channels=UNET_BLOCKS[tag]["ci"], out_channels=UNET_BLOCKS[tag]["co"])
        sd = blk.state_dict()
        assert {k: list(v.shape) for k, v in sd.items()} == json.loads(str(g[f"{tag}.sd_shapes"]))
        assert blk.conv[0].padding_mode == "replicate" and blk.conv[0].bias is None


def test_unet3d_pickles(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    model = MODEL_CLASSES["unet-3d"]("cpu", **UNET_TINY_KW)
    unet3d_fill_(model, 3)
    clone = pickle.loads(pickle.dumps(model))
    for (k, a), (k2, b) in zip(sorted(model.state_dict().items()), sorted(clone.state_dict().items())):
        assert k == k2 and torch.equal(a, b)
    assert clone.precision == "f32" and clone.temporal_dim == 3 and clone.features == [4, 8]


def test_unet3d_refuses_what_it_cannot_run(vpx):
    from vp_suite_amd._lib import VpxError
    from vp_suite_amd.models import MODEL_CLASSES
    M = MODEL_CLASSES["unet-3d"]
    with pytest.raises(NotImplementedError):
        M("cpu", img_shape=(1, 64, 64), action_size=3, action_conditional=True, tensor_value_range=[0.0, 1.0], temporal_dim=4)
    for shape in ((1, 60, 64), (1, 64, 72), (3, 20, 20)):            # not multiples of 2**4
        with pytest.raises(ValueError):
            M("cpu", img_shape=shape, temporal_dim=4, **_BASE)
    with pytest.raises(ValueError):
        M("cpu", img_shape=(1, 16, 18), features=[4, 8], temporal_dim=3, **_BASE)
    for td in (0, -1):
        with pytest.raises(ValueError):
            M("cpu", img_shape=(1, 64, 64), temporal_dim=td, **_BASE)
    for prec in ("bf16x3", "bf16"):
        with pytest.raises(ValueError):
            M("cpu", precision=prec, **UNET_TINY_KW)
    model = M("cpu", **UNET_TINY_KW)
    with pytest.raises(ValueError):                                  # fewer context frames than temporal_dim
        model(torch.rand(2, 2, 1, 16, 24), pred_frames=1)
    with pytest.raises(VpxError):                                    # no CPU fallback
        model(torch.rand(2, 3, 1, 16, 24), pred_frames=1)


def test_unet_ops_refuse_bad_arguments(vpx):
    from vp_suite_amd import unet_ops
    from vp_suite_amd._lib import VpxError
    with pytest.raises(VpxError):
        unet_ops.replicate_conv(torch.rand(2, 1, 5, 7, 3), torch.rand(4, 3, 3, 3))
    with pytest.raises(VpxError):
        unet_ops.time_collapse(torch.rand(2, 2, 5, 7, 4), torch.rand(4, 4, 2, 1, 1))
    with pytest.raises(VpxError):
        unet_ops.bn_relu(torch.rand(2, 1, 4, 4, 4), torch.rand(2, 4), torch.rand(4), torch.rand(4))
    bn = torch.nn.BatchNorm2d(4, eps=1e-3)
    with pytest.raises((ValueError, VpxError)):
        unet_ops.conv_bn_relu(torch.rand(2, 1, 5, 7, 3), torch.rand(4, 3, 3, 3), bn)


# ---- the plain-torch restatement (tests/unet3d_ref.py) against the reference's fixture, on the CPU ------------------------------------
def test_unet3d_ref_matches_fixture_on_cpu(vpx):
    """unet3d_ref is what tools/bench_unet3d.py times beside the library and what the GPU tests' gradient bars are measured with: it must
    compute the reference's model. f32 on the CPU against the f32 CPU fixture: 1e-5 max-normalised on frames and buffers, 1e-4 on
    gradients (two fp32 orders of summation through the BatchNorms)."""
    import unet3d_ref
    from vp_suite_amd.models import MODEL_CLASSES
    g = load_golden("unet3d_tiny")
    model = MODEL_CLASSES["unet-3d"]("cpu", **UNET_TINY_KW)
    unet3d_fill_(model, name_seed("unet3d.tiny"))
    x = tiny_inputs()
    assert abs(float(g["chk_x"]) - checksum(x)) < 1e-6

    def relmax(a, b):
        b = torch.as_tensor(np.asarray(b)).double()
        return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))
    with torch.no_grad():
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        pred, ml = unet3d_ref.forward(sd, x, UNET_TINY_PRED)
        assert ml is None and relmax(pred, g["eval"]) < 1e-5
        assert relmax(unet3d_ref.pred_1(sd, x), g["pred1"]) < 1e-5
        assert all(torch.equal(sd[k], v) for k, v in model.state_dict().items())       # eval touches no buffer
    sd = {k: v.clone().requires_grad_(torch.is_floating_point(v) and "running" not in k) for k, v in model.state_dict().items()}
    pred, _ = unet3d_ref.forward(sd, x, UNET_TINY_PRED, training=True)
    assert relmax(pred.detach(), g["train.frames"]) < 1e-5
    (pred * pred).sum().backward()
    table = fixture_grads(g, "train")
    assert sorted(table) == sorted(k for k, v in sd.items() if v.requires_grad)
    for k, (stats, kept) in table.items():
        a = sd[k].grad.double().numpy().reshape(-1)
        assert np.abs(grad_kept(a) - kept).max() <= 1e-4 * stats[2], k
        assert abs(a.sum() - stats[0]) <= 1e-4 * max(np.sqrt(stats[1] * a.size), 1e-30), k
    for k, v in buffers_of(sd).items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(g["buf." + k]) == 3
        else:
            assert relmax(v.detach(), g["buf." + k]) < 1e-5, k


# ---- dry-run workspace contract -----------------------------------------------------------------------------------------------------
OK, E_ARG, E_WS, E_UNSUP = 0, -1, -2, -4
WS_BASE = 0x7F0000000000
WS_BASE_ODD = WS_BASE + 0x40
REPLICATE, COLLAPSE = 0, 1
EPI_PLAIN, EPI_EVAL, EPI_STATS = 0, 1, 2


def _fake(i):
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


@pytest.fixture(scope="module")
def L():
    from vp_suite_amd import _lib
    lib = _lib.lib()
    with _lib.option(_lib.OPT_DRY_RUN, 1):
        yield lib
    lib.vpx_set_deterministic(0)


def unet_layers(c, h, w, features, td):
    """(T, H, W, Ca, Cb, Co, kt, mode) of every rconv layer of UNet3D(img_shape=(c, h, w), features, temporal_dim=td)."""
    out, ci = [], c
    for f in features:
        out += [(td, h, w, ci, 0, f, 3, REPLICATE), (td, h, w, f, 0, f, 3, REPLICATE), (td, h, w, f, 0, f, td, COLLAPSE)]
        ci, h, w = f, h // 2, w // 2
    f = features[-1]
    out += [(td, h, w, f, 0, f, td, COLLAPSE), (1, h, w, f, 0, 2 * f, 1, REPLICATE), (1, h, w, 2 * f, 0, 2 * f, 1, REPLICATE)]
    for f in reversed(features):
        h, w = 2 * h, 2 * w
        out += [(1, h, w, f, f, f, 1, REPLICATE), (1, h, w, f, 0, f, 1, REPLICATE)]
    return out


UNET_GEOMETRIES = [(1, 16, 24, [4, 8], 3), (3, 20, 12, [4, 8], 2), (1, 64, 64, [8, 16, 32, 64], 4), (3, 128, 128, [8, 16, 32, 64], 4)]
OP_SHAPES = [(1, 1, 1, 1, 0, 4, 1, REPLICATE), (2, 3, 2, 3, 0, 8, 3, REPLICATE), (3, 18, 34, 20, 0, 24, 3, REPLICATE), (1, 5, 7, 8, 20, 24, 1, REPLICATE),
             (2, 5, 7, 4, 0, 4, 2, COLLAPSE), (4, 5, 7, 24, 0, 24, 4, COLLAPSE)]


@pytest.mark.parametrize("det", [0, 1])
def test_rconv_entry_points(L, det):
    from vp_suite_amd._lib import RConvDesc
    L.vpx_set_deterministic(det)
    cases = [(lay, N) for (c, h, w, feats, td), N in itertools.product(UNET_GEOMETRIES, (1, 2, 16, 64)) for lay in unet_layers(c, h, w, feats, td)]
    cases += [(lay, 2) for lay in OP_SHAPES]
    for (T, H, W, Ca, Cb, Co, kt, mode), N in cases:
        d = RConvDesc(N, T, H, W, Ca, Cb, Co, kt, mode)
        b = _fake(2) if Cb else None
        for epi in (EPI_PLAIN, EPI_EVAL, EPI_STATS):
            if epi == EPI_STATS and N * (1 if mode == COLLAPSE else T) * H * W < 2:
                continue
            nb = L.vpx_rconv_workspace_bytes(ctypes.byref(d), epi)
            assert nb > 0, L.vpx_last_error()
            for base in (WS_BASE, WS_BASE_ODD):
                rc = L.vpx_rconv_fwd(ctypes.byref(d), epi, _fake(1), b, _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), 1e-5, 0.1, _fake(8), _fake(9),
                                     ctypes.c_void_p(base), nb, None)
                assert rc == OK, ((T, H, W, Ca, Cb, Co, kt, mode), epi, L.vpx_last_error())
            assert L.vpx_rconv_fwd(ctypes.byref(d), epi, _fake(1), b, _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), 1e-5, 0.1, _fake(8), _fake(9),
                                   ctypes.c_void_p(WS_BASE), nb - 256 - 4, None) == E_WS
        nbw = L.vpx_rconv_bwd_workspace_bytes(ctypes.byref(d))
        assert nbw > 0, L.vpx_last_error()
        for base in (WS_BASE, WS_BASE_ODD):
            rc = L.vpx_rconv_bwd(ctypes.byref(d), _fake(1), b, _fake(3), _fake(10), _fake(11), _fake(12) if Cb else None, _fake(13), _fake(14),
                                 ctypes.c_void_p(base), nbw, None)
            assert rc == OK, ((T, H, W, Ca, Cb, Co, kt, mode), L.vpx_last_error())
        assert L.vpx_rconv_bwd(ctypes.byref(d), _fake(1), b, _fake(3), _fake(10), None, None, _fake(13), None, ctypes.c_void_p(WS_BASE), nbw, None) == OK
        assert L.vpx_rconv_bwd(ctypes.byref(d), _fake(1), b, _fake(3), _fake(10), _fake(11), None, _fake(13), None, ctypes.c_void_p(WS_BASE), nbw - 256 - 4,
                               None) == E_WS


def test_bn_relu_entry_points(L):
    cases = {(N * T, H, W, Co) for (c, h, w, feats, td), N in itertools.product(UNET_GEOMETRIES, (1, 2, 16, 64))
             for (T, H, W, Ca, Cb, Co, kt, mode) in unet_layers(c, h, w, feats, td) if mode == REPLICATE}
    cases |= {(2, 1, 1, 4), (2, 1, 1, 24), (6, 5, 7, 24), (6, 6, 8, 4), (2, 2, 2, 300)}
    for (N, H, W, C) in sorted(cases):
        even = H % 2 == 0 and W % 2 == 0
        assert L.vpx_bn_relu_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), None, N, H, W, C, None) == OK, L.vpx_last_error()
        assert L.vpx_bn_relu_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), N, H, W, C, None) == (OK if even else E_ARG)
        nb = L.vpx_bn_relu_bwd_workspace_bytes(N, H, W, C)
        assert nb > 0
        for base in (WS_BASE, WS_BASE_ODD):
            rc = L.vpx_bn_relu_bwd(_fake(1), _fake(5), _fake(2), _fake(3), _fake(7), _fake(8) if even else None, _fake(9), _fake(10), _fake(11), N, H, W, C,
                                   ctypes.c_void_p(base), nb, None)
            assert rc == OK, ((N, H, W, C), L.vpx_last_error())
        assert L.vpx_bn_relu_bwd(_fake(1), _fake(5), _fake(2), _fake(3), _fake(7), None, _fake(9), None, None, N, H, W, C, ctypes.c_void_p(WS_BASE),
                                 nb - 256 - 4, None) == E_WS
    assert L.vpx_bn_relu_fwd(_fake(1), None, None, None, None, _fake(6), 2, 4, 6, 8, None) == OK          # the eval path's pool
    assert L.vpx_bn_relu_fwd(_fake(1), None, None, None, _fake(5), _fake(6), 2, 4, 6, 8, None) == E_ARG
    assert L.vpx_bn_relu_fwd(_fake(1), _fake(2), _fake(3), _fake(4), None, None, 2, 4, 6, 8, None) == E_ARG


def test_rconv_rejects_bad_arguments(L):
    from vp_suite_amd._lib import RConvDesc
    good = RConvDesc(2, 3, 5, 7, 3, 0, 4, 3, REPLICATE)
    nb = L.vpx_rconv_workspace_bytes(ctypes.byref(good), EPI_STATS)
    args = (_fake(1), None, _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), 1e-5, 0.1, _fake(8), _fake(9), ctypes.c_void_p(WS_BASE), nb, None)
    assert L.vpx_rconv_fwd(ctypes.byref(good), EPI_STATS, *args) == OK
    assert L.vpx_rconv_fwd(ctypes.byref(good), 7, *args) == E_ARG
    for bad in (RConvDesc(2, 3, 5, 7, 3, 0, 4, 2, REPLICATE), RConvDesc(2, 3, 5, 7, 3, 0, 4, 2, COLLAPSE), RConvDesc(2, 3, 0, 7, 3, 0, 4, 3, REPLICATE),
                RConvDesc(2, 3, 5, 7, 3, 0, 4, 3, 5)):
        assert L.vpx_rconv_workspace_bytes(ctypes.byref(bad), EPI_PLAIN) == 0
        assert L.vpx_rconv_bwd_workspace_bytes(ctypes.byref(bad)) == 0
        assert L.vpx_rconv_fwd(ctypes.byref(bad), EPI_PLAIN, *args) == E_ARG
    one = RConvDesc(1, 1, 1, 1, 3, 0, 4, 1, REPLICATE)                 # one value per channel: no batch statistics
    assert L.vpx_rconv_fwd(ctypes.byref(one), EPI_STATS, *args) == E_ARG and b"more than one value" in L.vpx_last_error()
    two = RConvDesc(2, 3, 5, 7, 3, 2, 4, 3, REPLICATE)                 # a second source that is not there
    assert L.vpx_rconv_fwd(ctypes.byref(two), EPI_PLAIN, *args) == E_ARG
    eps0 = args[:7] + (0.0,) + args[8:]
    assert L.vpx_rconv_fwd(ctypes.byref(good), EPI_EVAL, *eps0) == E_ARG


def test_unet_entry_points_refuse_what_a_launch_cannot_cover(L):
    """2^38 elements or more, or more than 65 536 channels: refused, not launched on a truncated grid (Limits)."""
    from vp_suite_amd._lib import RConvDesc
    big = 1 << 15
    for d in (RConvDesc(4, 4, big, big, 8, 0, 8, 3, REPLICATE),                       # 2^34 pixels x 16 channels = 2^38
              RConvDesc(big, big, big, big, 8, 0, 8, 3, REPLICATE),                   # a pixel count past 2^63
              RConvDesc(1, 1, 4, 4, 8, 0, (1 << 16) + 4, 1, REPLICATE)):              # channel groups past grid.y
        assert L.vpx_rconv_workspace_bytes(ctypes.byref(d), EPI_PLAIN) == 0 and b"too large" in L.vpx_last_error()
        assert L.vpx_rconv_bwd_workspace_bytes(ctypes.byref(d)) == 0
    assert L.vpx_rconv_workspace_bytes(ctypes.byref(RConvDesc(4, 4, big, big >> 1, 8, 0, 8, 3, REPLICATE)), EPI_PLAIN) > 0      # 2^37: served
    for (N, H, W, C) in ((1 << 8, big, big, 1), (1 << 62, 2, 2, 4), (1 << 40, big, big, 4), (2, 2, 2, (1 << 16) + 1)):
        assert L.vpx_bn_relu_bwd_workspace_bytes(N, H, W, C) == 0
        assert L.vpx_bn_relu_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), None, N, H, W, C, None) == E_ARG
    assert L.vpx_bn_relu_bwd_workspace_bytes(1 << 7, big, big, 1) > 0
