"""NonConvLSTM ("nc-lstm") on the host, no GPU: registry (and the key "lstm" still invalid), class constants, the state_dict against the
reference's key table (tests/golden/lstm_*.npz), constructor and forward errors, the oracle of tests/lstm_ref.py pinned to
torch.nn.LSTMCell / F.interpolate in double and to the reference's outputs in the fixtures, the dry-run workspace contract
(VPX_OPT_DRY_RUN, see test_workspace_contract.py) of the new entry points, and vpx_dense_plan over the GPU tests' case table.

Also that case table, shared with test_gpu_lstm.py."""
import ctypes
import itertools
import json

import numpy as np
import pytest
import torch

import lstm_ref
from golden_util import checksum, fill_state_dict_, load_golden, name_seed, seeded_rand, seeded_randn
from lstm_ref import LSTM_DEFAULT_KW, LSTM_TINY3_CTX, LSTM_TINY3_KW, LSTM_TINY3_PRED, LSTM_TINY_B, LSTM_TINY_CTX, LSTM_TINY_KW, LSTM_TINY_PRED

# ---- the dense layer's GPU cases: (M, N, K) ------------------------------------------------------------------------------------------------
DENSE_MS, DENSE_NS, DENSE_KS = (1, 2, 5, 17, 130), (1, 7, 33, 130), (1, 7, 33, 130)
DENSE_DEFAULT = (2, 1024, 16384)   # (M, N, K) of to_linear at the default sizes, B = 2
CELL_CASES = ((1, 3, 1), (3, 40, 5), (2, 7, 8), (17, 130, 36), (3, 33, 130))   # (M, Kx, H)


def _plan(M, N, K):
    from vp_suite_amd import lstm_ops
    return lstm_ops.dense_plan(M, N, K)


def smallest_k(M, N, chunks, ragged):
    """The smallest K whose plan for (M, N, K) has `chunks` K chunks (ragged: with a last chunk shorter than the others)."""
    for K in range(1, 1 << 14):
        p = _plan(M, N, K)
        if p["chunks"] == chunks and (not ragged or K % p["chunk_len"] != 0):
            return K
    raise AssertionError(f"no K below 16384 gives {chunks} chunks for M={M} N={N}")


def dense_split_cases():
    """Split routes on each tile form: two even chunks and three chunks with a ragged last one."""
    return [(2, 7, smallest_k(2, 7, 2, False)), (2, 7, smallest_k(2, 7, 3, True)), (5, 130, smallest_k(5, 130, 3, True)),
            (17, 33, smallest_k(17, 33, 2, False)), (130, 33, smallest_k(130, 33, 3, True))]


def dense_cases():
    return list(itertools.product(DENSE_MS, DENSE_NS, DENSE_KS)) + dense_split_cases()


def _model(kw, **extra):
    from vp_suite_amd.models import MODEL_CLASSES
    return MODEL_CLASSES["nc-lstm"]("cpu", **{**kw, **extra})


# ---- registry and constructor contract ------------------------------------------------------------------------------------------------------
def test_nc_lstm_is_registered_and_lstm_is_not(vpx):
    from vp_suite_amd.models import MODEL_CLASSES
    from vp_suite_amd.models.lstm import LSTM
    assert MODEL_CLASSES["nc-lstm"] is LSTM and "lstm" not in MODEL_CLASSES
    suite = vpx.VPSuite(device="cpu")
    with pytest.raises(ValueError, match="invalid model type"):
        suite.create_model("lstm")


def test_class_constants_are_the_references(vpx):
    from vp_suite_amd.models.lstm import LSTM
    assert LSTM.NAME == "NonConvLSTM" and LSTM.CAN_HANDLE_ACTIONS is True and LSTM.MATCHES_REFERENCE == "Not Yet"
    assert LSTM.PAPER_REFERENCE is None and LSTM.CODE_REFERENCE is None
    assert (LSTM.bottleneck_dim, LSTM.lstm_hidden_dim, LSTM.lstm_num_layers, LSTM.carry_state) == (1024, 1024, 3, True)
    assert LSTM.TRAINABLE and not LSTM.NEEDS_COMPLETE_INPUT and LSTM.MIN_CONTEXT_FRAMES == 1


@pytest.mark.parametrize("tag,kw", [("tiny", LSTM_TINY_KW), ("tiny3", LSTM_TINY3_KW), ("default", LSTM_DEFAULT_KW)])
def test_state_dict_holds_the_references_table(vpx, tag, kw):
    """state_dict >= the reference's keys with equal shapes (duplicates `encoder.*` / `decoder.*` included); the rest is exactly
    rnn_layers.* with nn.LSTMCell's names and shapes; the reference's part has the reference's parameter count."""
    g = load_golden(f"lstm_{tag}")
    model = _model(kw)
    sd = model.state_dict()
    ref_shapes = json.loads(str(g["sd_shapes"]))
    assert sorted(ref_shapes) == [str(k) for k in g["sd_keys"]]
    for k, shape in ref_shapes.items():
        assert k in sd and list(sd[k].shape) == shape, k
    extra = sorted(set(sd) - set(ref_shapes))
    H, L = model.lstm_hidden_dim, model.lstm_num_layers
    want = {}
    for i in range(L):
        k_in = model.bottleneck_dim if i == 0 else H
        want.update({f"rnn_layers.{i}.weight_ih": [4 * H, k_in], f"rnn_layers.{i}.weight_hh": [4 * H, H], f"rnn_layers.{i}.bias_ih": [4 * H],
                     f"rnn_layers.{i}.bias_hh": [4 * H]})
    assert extra == sorted(want) and all(list(sd[k].shape) == want[k] for k in want)
    assert isinstance(model.rnn_layers, torch.nn.ModuleList)
    n_ref = sum(p.numel() for n, p in model.named_parameters() if not n.startswith("rnn_layers."))
    assert n_ref == int(g["n_params"])
    if kw.get("action_conditional"):
        assert model.bottleneck_dim == 24 + 2 and list(sd["rnn_layers.0.weight_ih"].shape) == [96, 26]
    # a reference checkpoint loads with strict=False: only the cells are missing
    ref_sd = {k: torch.zeros(v) for k, v in ref_shapes.items()}
    res = model.load_state_dict(ref_sd, strict=False)
    assert sorted(res.missing_keys) == sorted(want) and not res.unexpected_keys


def test_cell_parameters_have_lstmcells_default_initialisation(vpx):
    model = _model(LSTM_TINY_KW, lstm_hidden_dim=16)
    bound = 1.0 / np.sqrt(16)
    for p in model.rnn_layers.parameters():
        assert 0.5 * bound < float(p.detach().abs().max()) <= bound


def test_constructor_and_forward_errors(vpx):
    with pytest.raises(ValueError, match="cell_precision"):
        _model(LSTM_TINY_KW, cell_precision="bf16x3")
    with pytest.raises(ValueError, match="at least 1"):
        _model(LSTM_TINY_KW, lstm_num_layers=0)
    with pytest.raises(ValueError, match="tensor_value_range"):
        _model({**LSTM_TINY_KW, "tensor_value_range": 1.0})
    m = _model(LSTM_TINY_KW)
    with pytest.raises(ValueError, match="input image does not match specified size"):
        m(torch.zeros(2, 3, 1, 16, 16), pred_frames=1)
    ac = _model(LSTM_TINY3_KW)
    with pytest.raises(ValueError, match="Given actions are None or of the wrong size"):
        ac(torch.zeros(2, 3, 3, 20, 12), pred_frames=1)
    with pytest.raises(ValueError, match="Given actions are None or of the wrong size"):
        ac(torch.zeros(2, 3, 3, 20, 12), pred_frames=1, actions=torch.zeros(2, 4, 2))
    # past the checks the hot path needs the GPU: no CPU fallback
    with pytest.raises(vpx._lib.VpxError, match="GPU"):
        m(torch.zeros(2, 3, 1, 16, 24), pred_frames=1)


def test_ops_refuse_cpu_tensors_and_bad_shapes(vpx):
    from vp_suite_amd import lstm_ops
    x, w = torch.zeros(2, 3), torch.zeros(4, 3)
    with pytest.raises(vpx._lib.VpxError, match="GPU"):
        lstm_ops.dense(x, w)
    with pytest.raises(vpx._lib.VpxError, match="GPU"):
        lstm_ops.lstm_cell(x, None, torch.zeros(8, 3), torch.zeros(8, 2), torch.zeros(8), torch.zeros(8))
    with pytest.raises(vpx._lib.VpxError, match="GPU"):
        lstm_ops.conv2d_replicate(torch.zeros(1, 1, 4, 4), torch.zeros(2, 1, 3, 3), None)
    with pytest.raises(vpx._lib.VpxError, match="GPU"):
        lstm_ops.resize_bilinear(torch.zeros(1, 1, 4, 4), (8, 8))


# ---- the oracle, pinned ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Kx,H", CELL_CASES)
def test_cell_formulas_match_torch_lstmcell_in_double(M, Kx, H):
    cell = torch.nn.LSTMCell(Kx, H).double()
    fill_state_dict_(cell, name_seed(f"lstm.cellpin.{M}.{Kx}.{H}"))
    x, h, c = (seeded_randn(s, name_seed(f"lstm.cellpin.{n}.{M}.{Kx}.{H}")).double().requires_grad_(True) for n, s in (("x", (M, Kx)), ("h", (M, H)), ("c", (M, H))))
    gh, gc = seeded_randn((M, H), 11).double(), seeded_randn((M, H), 12).double()
    params = [cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh]
    h1, c1 = cell(x, (h, c))
    want = torch.autograd.grad((h1 * gh).sum() + (c1 * gc).sum(), [x, h, c] + params)
    h2, c2 = lstm_ref.cell_ref(x, h, c, *params)
    got = torch.autograd.grad((h2 * gh).sum() + (c2 * gc).sum(), [x, h, c] + params)
    assert torch.allclose(h1, h2, rtol=0, atol=1e-13) and torch.allclose(c1, c2, rtol=0, atol=1e-13)
    for a, b in zip(want, got):
        assert torch.allclose(a, b, rtol=0, atol=1e-12)
    # zero state through None
    h3, c3 = lstm_ref.cell_ref(x, None, None, *params)
    h4, c4 = cell(x)
    assert torch.allclose(h3, h4, rtol=0, atol=1e-13) and torch.allclose(c3, c4, rtol=0, atol=1e-13)


@pytest.mark.parametrize("src,dst", [((1, 1), (16, 24)), ((2, 3), (16, 24)), ((9, 17), (16, 24)), ((9, 17), (20, 12)), ((2, 3), (20, 12)), ((57, 57), (64, 64))])
def test_resize_and_pad_restatements_match_torch_in_double(src, dst):
    x = seeded_randn((2, 3, *src), name_seed(f"lstm.resizepin.{src}.{dst}")).double()
    want = torch.nn.functional.interpolate(x, dst, mode="bilinear", align_corners=False)
    got = lstm_ref.resize_ref(x, dst)
    # (the source coordinates are float32 on purpose: their distance from torch's double ones bounds the difference)
    assert float((want - got).abs().max()) <= 4 * 2.0 ** -24 * max(dst) * float(x.abs().max())
    want_p = torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate")
    assert torch.equal(want_p, lstm_ref.replicate_pad_ref(x, 1))


def _ref_model(tag, kw, **extra):
    """RefLSTM in double with the parameters the generator gave the reference (the cells: seeded by name as well)."""
    model = _model(kw)
    fill_state_dict_(model, name_seed(f"lstm.{tag}"))
    return model, lstm_ref.RefLSTM(model.state_dict(), kw["img_shape"], action_conditional=kw.get("action_conditional", False), **extra)


def _check_grads(g, prefix, named, rel):
    names = [str(n) for n in g[f"{prefix}.gnames"]]
    stats, kept_n, kept = g[f"{prefix}.gstats"], g[f"{prefix}.gkept_n"], g[f"{prefix}.gkept"]
    summ = lstm_ref.grad_summary({n: named[n] for n in names})
    off = 0
    for i, n in enumerate(names):
        scale = max(float(stats[i][2]), 1e-30)
        assert abs(summ[n][2] - stats[i][2]) <= rel * scale, n
        assert np.abs(summ[n][3] - kept[off:off + kept_n[i]]).max() <= rel * scale, n
        off += int(kept_n[i])


@pytest.mark.parametrize("tag,kw", [("tiny", LSTM_TINY_KW), ("tiny3", LSTM_TINY3_KW)])
def test_oracle_matches_the_reference_fixture(vpx, tag, kw):
    """encode / decode with gradients and the literal (carry_state=False) forward of tests/lstm_ref.py against the reference's own output."""
    g = load_golden(f"lstm_{tag}")
    B = LSTM_TINY_B
    c, h, w = kw["img_shape"]
    _, ref = _ref_model(tag, kw, carry_state=False, requires_grad=True)
    x0 = seeded_rand((B, c, h, w), name_seed(f"lstm.{tag}.x0"))
    z = seeded_randn((B, kw["lstm_hidden_dim"]), name_seed(f"lstm.{tag}.latent"))
    assert abs(checksum(x0) - float(g["chk_x0"])) < 1e-9 and abs(checksum(z) - float(g["chk_z"])) < 1e-9
    x0d, zd = x0.double().requires_grad_(True), z.double().requires_grad_(True)
    enc, dec = ref.encode(x0d), ref.decode(zd)
    assert np.abs(enc.detach().numpy() - g["enc"]).max() <= 2e-6 * np.abs(g["enc"]).max()
    assert np.abs(dec.detach().numpy() - g["dec"]).max() <= 2e-6 * np.abs(g["dec"]).max()
    ge, gd = seeded_randn(enc.shape, name_seed(f"lstm.{tag}.ge")).double(), seeded_randn(dec.shape, name_seed(f"lstm.{tag}.gd")).double()
    ((enc * ge).sum() + (dec * gd).sum()).backward()
    named = {k: v.grad for k, v in ref.p.items()}
    named["__x0__"], named["__z__"] = x0d.grad, zd.grad
    _check_grads(g, "ed", named, 2e-5)
    assert sorted(str(n) for n in g["ed.none"] if str(n)) == (["action_inflate.bias", "action_inflate.weight"] if tag == "tiny3" else [])
    # the literal forward
    ctx, pred = (LSTM_TINY_CTX, LSTM_TINY_PRED) if tag == "tiny" else (LSTM_TINY3_CTX, LSTM_TINY3_PRED)
    x = seeded_rand((B, ctx, c, h, w), name_seed(f"lstm.{tag}.x")).double()
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9
    out = ref.forward(x, pred_frames=pred)
    assert tuple(out.shape) == tuple(g["fwd"].shape)
    assert np.abs(out.detach().numpy() - g["fwd"]).max() <= 2e-6 * np.abs(g["fwd"]).max()
    if tag == "tiny":
        assert np.abs(ref.forward(x, 1)[:, 0].detach().numpy() - g["pred1"]).max() <= 2e-6 * np.abs(g["pred1"]).max()
        for v in ref.p.values():
            v.grad = None
        (out * out).sum().backward()
        _check_grads(g, "fwd", {k: v.grad for k, v in ref.p.items()}, 2e-5)
        none = sorted(str(n) for n in g["fwd.none"] if str(n))
        assert none == sorted(k for k, v in ref.p.items() if v.grad is None and not k.startswith("rnn_layers."))
        assert all(k.startswith(("enc", "to_linear")) for k in none) and none
    else:
        a0 = seeded_randn((B, ctx + pred, kw["action_size"]), name_seed("lstm.tiny3.actions"))
        assert abs(checksum(a0) - float(g["chk_actions"])) < 1e-9
        assert np.abs(ref.action_inflate(a0[:, 0].double()).detach().numpy() - g["inflate"]).max() <= 2e-6 * np.abs(g["inflate"]).max()


def test_carried_state_oracle_depends_on_the_context(vpx):
    """What the literal model cannot do: with the state carried, a changed context frame changes the prediction."""
    _, ref = _ref_model("tiny", LSTM_TINY_KW, carry_state=True)
    x = seeded_rand((LSTM_TINY_B, 3, 1, 16, 24), name_seed("lstm.tiny.x")).double()
    a = ref.forward(x, 2)
    x2 = x.clone()
    x2[:, 0] = 1 - x2[:, 0]
    assert float((ref.forward(x2, 2) - a).abs().max()) > 1e-6
    _, lit = _ref_model("tiny", LSTM_TINY_KW, carry_state=False)
    assert torch.equal(lit.forward(x, 2), lit.forward(x2, 2))


# ---- dry-run workspace contract -------------------------------------------------------------------------------------------------------------
OK, E_ARG, E_WS, E_UNSUPPORTED = 0, -1, -2, -4
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


def _ok(L, rc, what):
    assert rc == OK, f"{what}: rc={rc}: {L.vpx_last_error().decode()}"


def _dense_calls(L, M, N, K, base, nb, relu):
    rc = L.vpx_dense_fwd(_fake(1), K + 3, _fake(2), _fake(3), _fake(4), N + 5, M, N, K, relu, ctypes.c_void_p(base), nb, None)
    rc2 = L.vpx_dense_bwd(_fake(1), K + 3, _fake(2), _fake(4), N + 5, _fake(5), N, _fake(6), K, _fake(7), _fake(8), M, N, K, relu, 1,
                          ctypes.c_void_p(base), nb, None)
    return rc, rc2


def test_dense_entry_points_fit_their_workspace(L):
    """vpx_dense_fwd / _bwd with a workspace of exactly the query's size: the GPU case table, the model's layers at B = 1 ... 128 and at
    T * B rows, and a grid around the split thresholds."""
    model_layers = [(M, 1024, 16384) for M in (1, 2, 8, 9, 16, 32, 33, 64, 128, 129, 640, 1280)] + [(M, 16384, 1024) for M in (1, 2, 16, 64, 128)] + \
                   [(M, 102, 3) for M in (2, 128, 1280)] + [(2, 24, 1536), (10, 24, 1536), (2, 1536, 24), (2, 2, 3)]
    grid = [(M, N, K) for M in (1, 8, 9, 32, 33, 128, 129, 300) for N in (1, 31, 32, 33, 127, 128, 129, 1000) for K in (1, 255, 256, 511, 512, 767, 769, 4097)]
    n = 0
    for (M, N, K) in dense_cases() + model_layers + grid:
        nb = L.vpx_dense_workspace_bytes(M, N, K)
        assert nb > 0
        for base, relu in ((WS_BASE, 0), (WS_BASE_ODD, 1)):
            rc, rc2 = _dense_calls(L, M, N, K, base, nb, relu)
            _ok(L, rc, f"dense fwd {(M, N, K)}")
            _ok(L, rc2, f"dense bwd {(M, N, K)}")
        rc, rc2 = _dense_calls(L, M, N, K, WS_BASE, nb - 1, 0)
        assert rc == E_WS and rc2 == E_WS
        n += 1
    assert n > 600


def test_cell_entry_points_fit_their_workspace(L):
    cases = list(CELL_CASES) + [(M, Kx, H) for M in (1, 2, 16, 64, 128, 130) for (Kx, H) in ((1024, 1024), (1126, 1024), (24, 24), (26, 24), (300, 700), (2048, 64))]
    for (M, Kx, H) in cases:
        nb = L.vpx_lstm_cell_workspace_bytes(M, Kx, H)
        assert nb > 0
        for base in (WS_BASE, WS_BASE_ODD):
            for h in (_fake(2), None):
                rc = L.vpx_lstm_cell_fwd(_fake(1), Kx, h, _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8), _fake(9), _fake(10), M, Kx, H,
                                         ctypes.c_void_p(base), nb, None)
                _ok(L, rc, f"cell fwd {(M, Kx, H)} h={h is not None}")
                rc = L.vpx_lstm_cell_bwd(_fake(1), Kx, h, _fake(3), _fake(4), _fake(5), _fake(10), _fake(11), _fake(12), _fake(13), _fake(14), _fake(15),
                                         _fake(16), _fake(17), _fake(18), _fake(19), _fake(20), M, Kx, H, 0, ctypes.c_void_p(base), nb, None)
                _ok(L, rc, f"cell bwd {(M, Kx, H)} h={h is not None}")
        rc = L.vpx_lstm_cell_fwd(_fake(1), Kx, _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8), _fake(9), _fake(10), M, Kx, H,
                                 ctypes.c_void_p(WS_BASE), nb - 1, None)
        assert rc == E_WS


def test_new_entry_points_reject_bad_arguments(L):
    nb = L.vpx_dense_workspace_bytes(2, 3, 4)
    ws = ctypes.c_void_p(WS_BASE)
    assert L.vpx_dense_workspace_bytes(0, 3, 4) == 0 and L.vpx_lstm_cell_workspace_bytes(1, 0, 4) == 0
    assert L.vpx_dense_fwd(_fake(1), 3, _fake(2), None, _fake(4), 3, 2, 3, 4, 0, ws, nb, None) == E_ARG          # ldx < K
    assert L.vpx_dense_fwd(_fake(1), 4, _fake(2), None, _fake(4), 2, 2, 3, 4, 0, ws, nb, None) == E_ARG          # ldy < N
    assert L.vpx_dense_fwd(None, 4, _fake(2), None, _fake(4), 3, 2, 3, 4, 0, ws, nb, None) == E_ARG
    assert L.vpx_dense_fwd(_fake(1), 4, _fake(2), None, _fake(4), 3, 2, 3, 4, 0, None, nb, None) == E_WS
    assert L.vpx_dense_bwd(_fake(1), 4, _fake(2), None, 3, _fake(5), 3, _fake(6), 4, None, None, 2, 3, 4, 1, 0, ws, nb, None) == E_ARG   # relu without y
    assert L.vpx_dense_plan(2, 3, 4, None) == E_ARG
    assert L.vpx_replicate_pad_fwd(_fake(1), _fake(2), 1, 4, 4, 3, -1, None) == E_ARG
    assert L.vpx_replicate_pad_bwd(_fake(1), None, 1, 4, 4, 3, 1, None) == E_ARG
    assert L.vpx_replicate_pad_fwd(_fake(1), _fake(2), 2, 5, 3, 64, 1, None) == OK
    assert L.vpx_resize_bilinear_fwd(_fake(1), _fake(2), 2, 3, 9, 17, 16, 24, None) == OK
    assert L.vpx_resize_bilinear_bwd(_fake(1), _fake(2), 2, 3, 9, 17, 20, 12, None) == OK
    assert L.vpx_resize_bilinear_bwd(_fake(1), _fake(2), 2, 3, 9, 17, 40000, 12, None) == E_UNSUPPORTED
    assert L.vpx_resize_bilinear_fwd(_fake(1), _fake(2), 0, 3, 9, 17, 16, 24, None) == E_ARG


def test_model_conv_layers_fit_their_workspaces(L):
    """The convolution layers the model sends through vpx_conv2d_act_fwd / _bwd and vpx_conv2d_ex_fwd / _bwd (replicate-padded inputs with
    padding 0 among them), dry."""
    from vp_suite_amd._lib import ACT_NONE, ACT_RELU
    from vp_suite_amd.ops import conv_desc, conv_out_shape
    for (c, h, w, N) in ((1, 16, 24, 2), (3, 20, 12, 2), (1, 64, 64, 16), (3, 64, 64, 2)):
        hh, ww, layers = h, w, []
        layers.append(((N, c, hh, ww), (64, c, 7, 7), 3, False, ACT_RELU))
        hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        for ci, co in ((64, 128), (128, 256)):
            layers.append(((N, ci, hh + 2, ww + 2), (co, ci, 3, 3), 0, False, ACT_RELU))
            hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        for ci, co, k, p, act in ((256, 128, 3, 1, ACT_RELU), (128, 64, 3, 1, ACT_RELU), (64, c, 7, 3, ACT_NONE)):
            layers.append(((N, ci, hh, ww), (ci, co, k, k), p, True, act))
            hh, ww = (hh - 1) * 2 - 2 * p + k, (ww - 1) * 2 - 2 * p + k
        assert (hh, ww) == (h - 7 if h % 8 == 0 else hh, w - 7 if w % 8 == 0 else ww)
        for xs, wsz, p, tr, act in layers:
            d = conv_desc(xs, wsz, 2, p, tr, 0.0, 0)
            conv_out_shape(d)
            nb = L.vpx_conv2d_act_workspace_bytes(ctypes.byref(d), act)
            _ok(L, L.vpx_conv2d_act_fwd(ctypes.byref(d), act, _fake(1), _fake(2), _fake(3), _fake(4), ctypes.c_void_p(WS_BASE_ODD), nb, None), f"fwd {xs} {wsz}")
            nbb = L.vpx_conv2d_act_bwd_workspace_bytes(ctypes.byref(d), act)
            _ok(L, L.vpx_conv2d_act_bwd(ctypes.byref(d), act, _fake(1), _fake(2), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8),
                                        ctypes.c_void_p(WS_BASE), nbb, None), f"bwd {xs} {wsz}")


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def test_dense_plan_over_the_gpu_case_table(vpx):
    """Every case's plan is consistent (chunks cover K, a multiple of 32 per chunk, no empty chunk, tiles cover M and N) and every route
    — tile form x {single pass, K split} — has a case; the design target's shapes fill the chip."""
    routes = set()
    for (M, N, K) in dense_cases() + [DENSE_DEFAULT]:
        p = _plan(M, N, K)
        assert p["split"] == int(p["chunks"] > 1) and p["chunk_len"] % 32 == 0
        assert (p["chunks"] - 1) * p["chunk_len"] < K <= p["chunks"] * p["chunk_len"]
        assert p["m_tiles"] * p["tile_m"] >= M > (p["m_tiles"] - 1) * p["tile_m"] and p["n_tiles"] * p["tile_n"] >= N > (p["n_tiles"] - 1) * p["tile_n"]
        assert p["form"] == (0 if M <= 8 else 1 if M <= 32 else 2) and (p["tile_m"], p["tile_n"]) == ((8, 128), (32, 32), (128, 32))[p["form"]]
        routes.add((p["form"], p["split"]))
    assert routes == {(f, s) for f in (0, 1, 2) for s in (0, 1)}
    ks = dense_split_cases()
    assert _plan(*ks[0])["chunks"] == 2 and ks[0][2] % _plan(*ks[0])["chunk_len"] == 0
    assert _plan(*ks[1])["chunks"] == 3 and ks[1][2] % _plan(*ks[1])["chunk_len"] != 0
    assert _plan(2, 7, ks[0][2] - 1)["chunks"] == 1
    for M in (2, 16, 64, 128):   # N = 1024, K = 16384: one M tile (each weight element read by one workgroup) and >= 256 workgroups
        p = _plan(M, 1024, 16384)
        assert p["m_tiles"] == 1 and p["n_tiles"] * p["chunks"] >= 256
        p = _plan(M, 16384, 1024)
        assert p["m_tiles"] == 1 and p["n_tiles"] * p["chunks"] >= 256
