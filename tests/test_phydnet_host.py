"""PhyDNet ("phy") on the host, no GPU: registry, constructor contract (state_dict keys / shapes / n_params against the reference's, pinned
in tests/golden/phydnet_default.npz), pickling, the errors the port raises, and the dry-run workspace contract (VPX_OPT_DRY_RUN, see
test_workspace_contract.py) of the new library entry points and of the convolution layers PhyDNet runs.

Also the case table of the PhyDNet fixtures, shared with test_gpu_phydnet.py and tools/gen_golden.py (gen_phydnet)."""
import ctypes
import itertools
import json
import pickle

import numpy as np
import pytest
import torch

from golden_util import fill_state_dict_, load_golden

# ---- fixture cases (tools/gen_golden.py gen_phydnet) ----------------------------------------------------------------------------
# PhyCell block: (input_dim, hidden, k, H, W, action_size (0: plain), B, steps)
PHY_CELL_CASES = {"plain": (16, 49, 7, 8, 8, 0, 2, 3), "ac": (16, 49, 7, 8, 8, 3, 2, 3)}
# tiny model. The last ConvLSTM width stays 64: the reference's DecoderSplit takes 64 channels, and with a narrower last layer its
# forward fails (a [16, 16, 8] stack raises in decoder_Dr.upc1).
PHY_TINY_KW = dict(img_shape=(1, 32, 32), action_size=0, tensor_value_range=[0.0, 1.0], convlstm_hidden_dims=[16, 16, 64])
PHY_TINY_AC_KW = dict(img_shape=(1, 32, 32), action_size=3, action_conditional=True, tensor_value_range=[0.0, 1.0],
                      convlstm_hidden_dims=[16, 16, 64])
PHY_DEFAULT_KW = dict(img_shape=(1, 64, 64), action_size=0, tensor_value_range=[0.0, 1.0])
PHY_TINY_B, PHY_TINY_CTX, PHY_TINY_PRED = 2, 4, 3          # eval: 4 -> 3
PHY_TRAIN_CTX, PHY_TRAIN_PRED = 3, 3                       # train: 6 frames, 3 of them predicted
PHY_DEFAULT_B, PHY_DEFAULT_CTX, PHY_DEFAULT_PRED = 1, 10, 10
GRAD_SLICE = 97                                            # the gradient summaries keep every 97th element (at most 64 of them) ...
GRAD_FULL_MAX = 4096                                       # ... of tensors larger than this; smaller ones (biases, GroupNorm) in full


def phy_fill_(module, seed):
    """fill_state_dict_ plus 1 on every GroupNorm scale (the seeded 0.1-scale values would squash every normalised activation)."""
    fill_state_dict_(module, seed)
    with torch.no_grad():
        for name, m in module.named_modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.add_(1.0)
    return module


def grad_summary(named_grads):
    """{name: (sum, sum of squares, max |g|, the elements kept)} of fp64 numpy copies; the elements kept are all of them for tensors of at
    most GRAD_FULL_MAX elements, else every GRAD_SLICE-th (at most 64)."""
    out = {}
    for k, g in named_grads.items():
        a = g.detach().cpu().double().numpy().reshape(-1)
        out[k] = (a.sum(), (a * a).sum(), np.abs(a).max(), grad_kept(a))
    return out


def grad_kept(a):
    return a if a.size <= GRAD_FULL_MAX else a[::GRAD_SLICE][:64]


# ---- host tests -------------------------------------------------------------------------------------------------------------------
def test_phy_is_registered(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    assert "phy" in MODEL_CLASSES
    assert MODEL_CLASSES["phy"].CAN_HANDLE_ACTIONS


def test_phydnet_state_dict_matches_reference_on_cpu(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    g = load_golden("phydnet_default")
    m = MODEL_CLASSES["phy"]("cpu", **PHY_DEFAULT_KW)
    sd = m.state_dict()
    assert sorted(sd.keys()) == list(g["sd_keys"])
    shapes = json.loads(str(g["sd_shapes"]))
    assert {k: list(v.shape) for k, v in sd.items()} == shapes
    assert len(sd) == 68
    assert sum(p.numel() for p in m.parameters()) == int(g["n_params"]) == 3_091_732
    assert m.shape_Ep == torch.Size((64, 16, 16)) and m.shape_Er == torch.Size((64, 16, 16))


def test_phydnet_pickles(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    for kw in (PHY_TINY_KW, PHY_TINY_AC_KW):
        m = MODEL_CLASSES["phy"]("cpu", **kw)
        m2 = pickle.loads(pickle.dumps(m))
        sd, sd2 = m.state_dict(), m2.state_dict()
        assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_phydnet_rejects_sizes_not_divisible_by_4(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    for shape in ((1, 30, 32), (1, 32, 34), (3, 62, 64)):
        with pytest.raises(ValueError):
            MODEL_CLASSES["phy"]("cpu", img_shape=shape, action_size=0, tensor_value_range=[0.0, 1.0])


def test_phydnet_action_conditional_needs_actions(vpx):
    """The reference's check (phydnet.py forward) runs before any launch, so it needs no GPU."""
    from vp_suite_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES["phy"]("cpu", **PHY_TINY_AC_KW)
    x = torch.rand(2, 3, 1, 32, 32)
    with pytest.raises(ValueError, match="actions"):
        m(x, pred_frames=2)
    with pytest.raises(ValueError, match="actions"):
        m(x, pred_frames=2, actions=torch.rand(2, 4, 2))


def test_phydnet_training_loss_contract(vpx):
    """training_loss takes the context frames and the pred_frames frames after them (unpack_data's split, what the data-parallel trainer
    passes); anything else is refused before any launch. The teacher-forcing draw follows the reference's schedule at training_epoch."""
    from vp_suite_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES["phy"]("cpu", **PHY_TINY_KW)
    ctx = torch.rand(2, 3, 1, 32, 32)
    for bad in (None, torch.rand(2, 2, 1, 32, 32), torch.rand(1, 3, 1, 32, 32)):
        with pytest.raises(ValueError, match="targets"):
            m.training_loss(ctx, bad, 3, None)
    assert "training_epoch" not in m.config
    m.training_epoch = 0
    assert all(m._teacher_forcing_draw() for _ in range(20))          # ratio 1 at epoch 0
    m.training_epoch = int(1 / m.teacher_forcing_decay) + 1
    assert not any(m._teacher_forcing_draw() for _ in range(20))      # ratio 0 past 1 / decay


def test_phydnet_rejects_non_square_phycell_kernel(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    for ks in ((7, 5), (6, 6)):
        with pytest.raises(ValueError):
            MODEL_CLASSES["phy"]("cpu", phycell_kernel_size=ks, **PHY_TINY_KW)


def test_phycell_cell_rejects_non_square_or_even_kernel(vpx):
    """The block's own check (the model's is above): the moment matrices and the 'same' padding are stated for square odd kernels."""
    from vp_suite_amd.model_blocks.phydnet import PhyCell_Cell
    for ks in ((3, 5), (4, 4)):
        with pytest.raises(ValueError):
            PhyCell_Cell(input_dim=16, action_conditional=False, action_size=0, hidden_dim=9, kernel_size=ks)
    PhyCell_Cell(input_dim=16, action_conditional=False, action_size=0, hidden_dim=9, kernel_size=(3, 3))


def test_phy_ops_refuse_cpu_tensors(vpx):
    """No CPU fallback: every op raises on host tensors before anything else."""
    from vp_suite_amd import phy_ops
    from vp_suite_amd._lib import VpxError
    with pytest.raises(VpxError):                         # no CPU fallback
        phy_ops.group_norm(torch.rand(2, 32, 4, 4), 16, torch.ones(32), torch.zeros(32))
    with pytest.raises(VpxError):
        phy_ops.moment_loss(torch.rand(49, 4, 7, 7))


# ---- dry-run workspace contract -----------------------------------------------------------------------------------------------------
OK, E_ARG, E_WS = 0, -1, -2
WS_BASE = 0x7F0000000000
WS_BASE_ODD = WS_BASE + 0x40


def _fake(i):
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


@pytest.fixture(scope="module")
def L():
    from vp_suite_amd import _lib
    lib = _lib.lib()
    with _lib.option(_lib.OPT_DRY_RUN, 1):
        yield lib
    lib.vpx_set_deterministic(0)


# (HW, C, G) of PhyDNet: DCGAN layers at 32x32x32 and 16x16x64 with 16 groups, the PhyCell's GroupNorm(7, 49) at 16x16; a grid around them
GN_SHAPES = [(32 * 32, 32, 16), (16 * 16, 64, 16), (16 * 16, 49, 7), (8 * 8, 49, 7), (64 * 64, 32, 16), (16 * 16, 128, 32), (5 * 7, 6, 3),
             (1, 256, 1), (17 * 13, 96, 16), (4, 3, 3)]


@pytest.mark.parametrize("det", [0, 1])
def test_groupnorm_entry_points(L, det):
    L.vpx_set_deterministic(det)
    for (HW, C, G), N, act in itertools.product(GN_SHAPES, (1, 2, 16, 64, 640), (0, 1)):
        rc = L.vpx_groupnorm_fwd(_fake(1), _fake(2), _fake(3), None, _fake(4), _fake(5), N, HW, C, G, act, 0.2, None)
        assert rc == OK, L.vpx_last_error()
        rc = L.vpx_groupnorm_fwd(_fake(1), _fake(2), _fake(3), _fake(6), _fake(4), _fake(5), N, HW, C, G, act, 0.2, None)
        assert rc == OK, L.vpx_last_error()
        nb = L.vpx_groupnorm_bwd_workspace_bytes(N, C)
        assert nb >= 2 * N * C * 4
        for base in (WS_BASE, WS_BASE_ODD):
            rc = L.vpx_groupnorm_bwd(_fake(1), _fake(5), _fake(2), _fake(3), _fake(7), _fake(8), _fake(9), _fake(10), N, HW, C, G, act, 0.2,
                                     ctypes.c_void_p(base), nb, None)
            assert rc == OK, L.vpx_last_error()
        rc = L.vpx_groupnorm_bwd(_fake(1), _fake(5), _fake(2), _fake(3), _fake(7), _fake(8), None, None, N, HW, C, G, act, 0.2, None, 0, None)
        assert rc == OK, L.vpx_last_error()          # no parameter gradients: no workspace
        rc = L.vpx_groupnorm_bwd(_fake(1), _fake(5), _fake(2), _fake(3), _fake(7), _fake(8), _fake(9), _fake(10), N, HW, C, G, act, 0.2,
                                 ctypes.c_void_p(WS_BASE), nb - 256 - 4, None)
        assert rc == E_WS


def test_groupnorm_rejects_bad_groups(L):
    for (C, G) in ((32, 5), (49, 0), (600, 2)):
        assert L.vpx_groupnorm_fwd(_fake(1), _fake(2), _fake(3), None, _fake(4), _fake(5), 2, 16, C, G, 1, 0.2, None) == E_ARG
    assert L.vpx_groupnorm_bwd_workspace_bytes(0, 32) == 0


def test_phydnet_small_entry_points(L):
    for n in (1, 2 * 16 * 16 * 64, 64 * 16 * 16 * 64):
        assert L.vpx_phycell_correct_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), n, None) == OK
        assert L.vpx_phycell_correct_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), None, _fake(8), None, n, None) == OK
    for (hid, cin, k) in ((49, 64, 7), (49, 16, 7), (9, 3, 3), (64, 64, 8)):
        assert L.vpx_moment_loss_fwd(_fake(1), _fake(2), hid, cin, k, k, 1.0, None) == OK
        assert L.vpx_moment_loss_bwd(_fake(1), _fake(2), _fake(3), hid, cin, k, k, 1.0, None) == OK
    assert L.vpx_moment_loss_fwd(_fake(1), _fake(2), 81, 4, 9, 9, 1.0, None) == E_ARG
    for (B, T, t0, nT, C, H, W) in ((1, 10, 0, 10, 1, 64, 64), (64, 10, 9, 1, 3, 64, 64), (2, 5, 1, 4, 1, 32, 32)):
        assert L.vpx_sigmoid_head_fwd(_fake(1), _fake(2), B, T, t0, nT, C, H, W, None) == OK
        assert L.vpx_sigmoid_head_bwd(_fake(1), _fake(2), _fake(3), B, T, t0, nT, C, H, W, None) == OK
    assert L.vpx_sigmoid_head_fwd(_fake(1), _fake(2), 2, 5, 3, 3, 1, 8, 8, None) == E_ARG   # slots past T


# the 13 distinct convolution layers of PhyDNet at 64x64 (ConvDesc fields after N, H, W: Ci, Co, k, stride, pad, transposed, out_pad)
PHY_CONV_LAYERS = [(64, 64, 1, 32, 3, 2, 1, 0, 0), (32, 32, 32, 32, 3, 1, 1, 0, 0), (32, 32, 32, 64, 3, 2, 1, 0, 0),
                   (16, 16, 64, 64, 3, 1, 1, 0, 0), (16, 16, 64, 64, 3, 1, 1, 1, 0), (16, 16, 64, 49, 7, 1, 3, 0, 0),
                   (16, 16, 49, 64, 1, 1, 0, 0, 0), (16, 16, 128, 64, 3, 1, 1, 0, 0), (16, 16, 64, 32, 3, 2, 1, 1, 1),
                   (32, 32, 32, 32, 3, 1, 1, 1, 0), (32, 32, 32, 1, 3, 2, 1, 1, 1), (64, 64, 3, 32, 3, 2, 1, 0, 0),
                   (32, 32, 32, 3, 3, 2, 1, 1, 1), (16, 16, 67, 64, 1, 1, 0, 0, 0)]


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", [0, 1])
def test_phydnet_conv_layers(L, det, prec):
    from vp_suite_amd._lib import ConvDesc
    L.vpx_set_deterministic(det)
    for (H, W, Ci, Co, k, s, p, tr, op), N in itertools.product(PHY_CONV_LAYERS, (1, 2, 16, 64, 640)):
        d = ConvDesc(N, H, W, Ci, Co, k, k, s, p, tr, 0.0, prec, op, op)
        ho, wo = ctypes.c_int(0), ctypes.c_int(0)
        assert L.vpx_conv2d_ex_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == OK, L.vpx_last_error()
        nb = L.vpx_conv2d_ex_workspace_bytes(ctypes.byref(d))
        assert nb > 0, L.vpx_last_error()
        rc = L.vpx_conv2d_ex_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), ctypes.c_void_p(WS_BASE_ODD), nb, None)
        assert rc == OK, (H, W, Ci, Co, k, s, tr, L.vpx_last_error())
        nbw = L.vpx_conv2d_ex_bwd_workspace_bytes(ctypes.byref(d))
        assert nbw > 0, L.vpx_last_error()
        rc = L.vpx_conv2d_ex_bwd(ctypes.byref(d), _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8),
                                 ctypes.c_void_p(WS_BASE), nbw, None)
        assert rc == OK, (H, W, Ci, Co, k, s, tr, L.vpx_last_error())


# ---- the plain-torch restatement (tests/phydnet_ref.py) against the reference's PhyCell fixtures, on the CPU -------------------------
@pytest.mark.parametrize("tag", list(PHY_CELL_CASES))
def test_phydnet_ref_matches_cell_fixtures_on_cpu(vpx, tag):
    """phydnet_ref's PhyCell block, run in fp64 on the inputs of the recorded f32 fixture, must be the reference's block: every step's
    output and the final state to 1e-5, the frame gradient and every parameter gradient to 5e-5 (max-normalised, the block's bars).
    test_gpu_phydnet_kernels.py holds the library to this restatement at shapes no fixture has; this case is what entitles it to."""
    import phydnet_ref
    from golden_util import name_seed, seeded_randn
    from vp_suite_amd.model_blocks import PhyCell
    idim, hid, k, H, W, asz, B, steps = PHY_CELL_CASES[tag]
    g = load_golden(f"phydnet_cell_{tag}")
    blk = phy_fill_(PhyCell((H, W), idim, [hid], 1, (k, k), asz > 0, asz, "cpu"), name_seed("phydnet_cell." + tag))
    sd = {key: v.detach().double().requires_grad_(True) for key, v in blk.state_dict().items()}
    assert (asz > 0) == ("cell_list.0.frame_action_conv.weight" in sd)
    frames = seeded_randn((B, steps, idim, H, W), name_seed(f"phydnet_cell.{tag}.frames")).double().requires_grad_(True)
    actions = seeded_randn((B, steps, max(asz, 1)), name_seed(f"phydnet_cell.{tag}.actions"))[:, :, :asz].double()
    outs, Hs = phydnet_ref.phycell_stack(sd, 1, frames, actions)

    def err(got, ref):
        return float(np.abs(got.detach().numpy() - ref).max()) / float(np.abs(ref).max())
    loss = 0.0
    for t, out in enumerate(outs):
        assert err(out, g[f"out{t}"]) < 1e-5, t
        loss = loss + (out * seeded_randn(out.shape, name_seed(f"phydnet_cell.{tag}.g{t}")).double()).sum()
    assert err(Hs[0], g["H0"]) < 1e-5
    loss.backward()
    assert err(frames.grad, g["dframes"]) < 5e-5
    names = [key for key, _ in blk.named_parameters()]
    assert sorted("grad." + key for key in names) == sorted(key for key in g if key.startswith("grad."))
    for key in names:
        assert err(sd[key].grad, g["grad." + key]) < 5e-5, key
