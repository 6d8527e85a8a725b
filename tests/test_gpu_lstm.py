"""NonConvLSTM ("nc-lstm") on the GPU: the dense layer, the LSTM cell, the replicate-padded stride-2 convolution, the differentiable
resize and the model against float64 references (tests/lstm_ref.py) and the reference's fixtures (tests/golden/lstm_*.npz).

Bars: max|d| / max|ref| against float64, the project's fp32 bars: 1e-5 for outputs, 5e-5 for gradients."""
import os

import numpy as np
import pytest
import torch

import lstm_ref
from golden_util import checksum, fill_state_dict_, load_golden, name_seed, seeded_rand, seeded_randn
from lstm_ref import (LSTM_DEFAULT_KW, LSTM_TINY3_CTX, LSTM_TINY3_KW, LSTM_TINY3_PRED, LSTM_TINY_B, LSTM_TINY_CTX, LSTM_TINY_KW, LSTM_TINY_PRED)
from test_lstm_host import CELL_CASES, DENSE_DEFAULT, DENSE_KS, DENSE_NS, _check_grads, dense_split_cases

pytestmark = pytest.mark.gpu
OUT_BAR, GRAD_BAR = 1e-5, 5e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _rn(shape, name, scale=1.0):
    return seeded_randn(shape, name_seed(name), scale)


# ---- dense ----------------------------------------------------------------------------------------------------------------------------
def _dense_case(ops, M, N, K, relu, tag):
    """Forward and the three gradients of one case against float64; returns the forward's relative error."""
    x, w, b, gy = _rn((M, K), f"{tag}.x"), _rn((N, K), f"{tag}.w", 1 / np.sqrt(K)), _rn((N,), f"{tag}.b"), _rn((M, N), f"{tag}.gy")
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    want = lstm_ref.dense_ref(xd, wd, bd, relu)
    gw = torch.autograd.grad((want * gy.double()).sum(), [xd, wd, bd])
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    got = ops.dense(xg, wg, bg, relu=relu)
    gg = torch.autograd.grad((got * gy.cuda()).sum(), [xg, wg, bg])
    err = rel(got, want)
    assert err < OUT_BAR, (M, N, K, relu, err)
    for name, a, r in zip("xwb", gg, gw):
        assert rel(a, r) < GRAD_BAR or float(r.abs().max()) == 0.0, (M, N, K, relu, name, rel(a, r))
    return err


@pytest.mark.parametrize("M", (1, 2, 5, 17, 130))
def test_dense_forward_and_gradients(vpx, M):
    from vp_suite_amd import lstm_ops
    for N in DENSE_NS:
        for K in DENSE_KS:
            p = lstm_ops.dense_plan(M, N, K)
            assert p["split"] == 0 and p["form"] == (0 if M <= 8 else 1 if M <= 32 else 2)
            _dense_case(lstm_ops, M, N, K, relu=(N + K) % 2 == 0, tag=f"lstm.dense.{M}.{N}.{K}")


@pytest.mark.parametrize("i", range(5))
def test_dense_k_split_routes(vpx, i):
    """Two even chunks and three chunks with a ragged last one, on each tile form; N past a tile boundary among them."""
    from vp_suite_amd import lstm_ops
    M, N, K = dense_split_cases()[i]
    p = lstm_ops.dense_plan(M, N, K)
    assert p["split"] == 1 and p["chunks"] == (2 if i in (0, 3) else 3) and (K % p["chunk_len"] != 0) == (i not in (0, 3))
    assert lstm_ops.dense_plan(M, K, N)["split"] == 0      # (the data gradient of these cases is single pass; the next test splits it)
    for relu in (False, True):
        _dense_case(lstm_ops, M, N, K, relu, tag=f"lstm.dense.split.{i}.{relu}")


def test_dense_data_gradient_k_split(vpx):
    """dx = dy * w with the contraction over N split (N = 769: three ragged chunks)."""
    from vp_suite_amd import lstm_ops
    M, N, K = 5, dense_split_cases()[1][2], 33
    assert lstm_ops.dense_plan(M, K, N)["chunks"] == 3
    _dense_case(lstm_ops, M, N, K, False, tag="lstm.dense.dxsplit")


def test_dense_strided_rows_subsets_accumulate_and_repeats(vpx):
    from vp_suite_amd import _lib, lstm_ops
    import ctypes
    M, N, K = 5, 33, dense_split_cases()[1][2]
    x, w, b = _rn((M, K + 9), "lstm.dense.ld.x"), _rn((N, K), "lstm.dense.ld.w", 1 / np.sqrt(K)), _rn((N,), "lstm.dense.ld.b")
    want = lstm_ref.dense_ref(x[:, 4:4 + K].double(), w.double(), b.double())
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    for (m, n, k) in ((M, N, K), (M, N, 33)):     # split and single pass
        buf = torch.full((m, n + 11), 7.5, device="cuda")
        out = lstm_ops.dense(xg[:, 4:4 + k], wg[:, :k], bg, out=buf[:, 3:3 + n])
        assert out.data_ptr() == buf[:, 3:].data_ptr()
        ref = lstm_ref.dense_ref(x[:, 4:4 + k].double(), w[:, :k].double(), b.double())
        assert rel(buf[:, 3:3 + n], ref) < OUT_BAR
        assert bool((buf[:, :3] == 7.5).all()) and bool((buf[:, 3 + n:] == 7.5).all())          # the bytes between the rows: untouched
    # out= inside autograd: two layers write side by side into one buffer, gradients reach both
    a, wa = _rn((M, 3), "lstm.dense.ld.a"), _rn((4, 3), "lstm.dense.ld.wa")
    gy = _rn((M, N + 4), "lstm.dense.ld.gy")
    leaves = [t.cuda().requires_grad_(True) for t in (x[:, 4:4 + K].contiguous(), w, b, a, wa)]
    buf = torch.empty(M, N + 4, device="cuda")
    lstm_ops.dense(leaves[0], leaves[1], leaves[2], out=buf[:, :N])
    lstm_ops.dense(leaves[3], leaves[4], None, out=buf[:, N:])
    got = torch.autograd.grad((buf * gy.cuda()).sum(), leaves)
    dl = [t.detach().cpu().double().requires_grad_(True) for t in leaves]
    cat = torch.cat([lstm_ref.dense_ref(dl[0], dl[1], dl[2]), lstm_ref.dense_ref(dl[3], dl[4])], dim=1)
    assert rel(buf, cat) < OUT_BAR
    for g_, r_ in zip(got, torch.autograd.grad((cat * gy.double()).sum(), dl)):
        assert rel(g_, r_) < GRAD_BAR
    # gradient subsets: only what requires grad is computed, and equals the full call's
    full = torch.autograd.grad((lstm_ops.dense(leaves[0], leaves[1], leaves[2]) * gy[:, :N].cuda()).sum(), leaves[:3])
    for keep in ((0,), (1,), (2,), (0, 2)):
        ins = [t.detach().clone().requires_grad_(i in keep) for i, t in enumerate(leaves[:3])]
        sub = torch.autograd.grad((lstm_ops.dense(*ins) * gy[:, :N].cuda()).sum(), [ins[i] for i in keep])
        for i, s in zip(keep, sub):
            assert torch.equal(s, full[i])
    # accumulate and bit-equal repeats, on the C ABI
    L = _lib.lib()
    xs, dy = leaves[0].detach(), gy[:, :N].cuda().contiguous()
    nb = L.vpx_dense_workspace_bytes(M, N, K)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def bwd(dw, db, acc):
        dx = torch.empty(M, K, device="cuda")
        rc = L.vpx_dense_bwd(p(xs), K, p(wg), None, N, p(dy), N, p(dx), K, p(dw), p(db), M, N, K, 0, acc, p(ws), nb, None)
        assert rc == 0, L.vpx_last_error()
        return dx
    dw0, db0 = torch.full((N, K), 2.0, device="cuda"), torch.full((N,), -1.0, device="cuda")
    dx0 = bwd(dw0, db0, 1)
    assert torch.equal(dx0, full[0]) and rel(dw0 - 2.0, full[1]) < GRAD_BAR and rel(db0 + 1.0, full[2]) < GRAD_BAR
    dw1, db1 = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
    assert torch.equal(bwd(dw1, db1, 0), dx0) and torch.equal(dw1, full[1]) and torch.equal(db1, full[2])
    y1, y2 = lstm_ops.dense(xs, wg, bg), lstm_ops.dense(xs, wg, bg)
    assert torch.equal(y1, y2)


def test_dense_default_size_long_k(vpx):
    """(M, K, N) = (2, 16384, 1024): accumulation over a long K on the 64-chunk route. The bar is max(1e-5, 4 x the error of torch's own
    CPU float32 F.linear on the same operands against float64): any correct fp32 accumulation order passes, a dropped chunk does not."""
    from vp_suite_amd import lstm_ops
    M, N, K = DENSE_DEFAULT
    assert lstm_ops.dense_plan(M, N, K)["chunks"] == 64
    x, w, b = _rn((M, K), "lstm.dense.default.x"), _rn((N, K), "lstm.dense.default.w", 1 / np.sqrt(K)), _rn((N,), "lstm.dense.default.b")
    want = torch.nn.functional.linear(x.double(), w.double(), b.double())
    cpu32 = rel(torch.nn.functional.linear(x, w, b), want)
    bar = max(1e-5, 4 * cpu32)
    y1 = lstm_ops.dense(x.cuda(), w.cuda(), b.cuda())
    err = rel(y1, want)
    print(f"dense default: err {err:.3e}, cpu fp32 err {cpu32:.3e}, bar {bar:.3e}")   # (recorded in profiles/lstm_parity.json)
    assert err < bar
    assert torch.equal(y1, lstm_ops.dense(x.cuda(), w.cuda(), b.cuda()))


# ---- cell -----------------------------------------------------------------------------------------------------------------------------
def _cell_inputs(M, Kx, H, tag, scale=1.0):
    shapes = dict(x=(M, Kx), h=(M, H), c=(M, H), w_ih=(4 * H, Kx), w_hh=(4 * H, H), b_ih=(4 * H,), b_hh=(4 * H,))
    t = {k: _rn(s, f"{tag}.{k}") for k, s in shapes.items()}
    t["w_ih"], t["w_hh"] = t["w_ih"] * scale / np.sqrt(Kx), t["w_hh"] * scale / np.sqrt(H)
    return t


ORDER = ("x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh")


def _cell_both(ops, t, gh, gc, zero_state=False):
    d = {k: v.double().requires_grad_(True) for k, v in t.items()}
    g = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
    names = [k for k in ORDER if not (zero_state and k in ("h", "c"))]
    hw, cw = lstm_ref.cell_ref(d["x"], None if zero_state else d["h"], None if zero_state else d["c"], d["w_ih"], d["w_hh"], d["b_ih"], d["b_hh"])
    hg, cg = ops.lstm_cell(g["x"], None if zero_state else (g["h"], g["c"]), g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"])
    lw = (0 if gh is None else (hw * gh.double()).sum()) + (0 if gc is None else (cw * gc.double()).sum())
    lg = (0 if gh is None else (hg * gh.cuda()).sum()) + (0 if gc is None else (cg * gc.cuda()).sum())
    want = torch.autograd.grad(lw, [d[k] for k in names], allow_unused=True)
    got = torch.autograd.grad(lg, [g[k] for k in names], allow_unused=True)
    return (hg, cg), (hw, cw), dict(zip(names, got)), dict(zip(names, want))


@pytest.mark.parametrize("M,Kx,H", CELL_CASES)
def test_cell_forward_and_gradients(vpx, M, Kx, H):
    from vp_suite_amd import lstm_ops
    tag = f"lstm.cell.{M}.{Kx}.{H}"
    t = _cell_inputs(M, Kx, H, tag)
    gh, gc = _rn((M, H), tag + ".gh"), _rn((M, H), tag + ".gc")
    for use_h, use_c in ((gh, gc), (gh, None), (None, gc)):       # dh' or dc' missing
        (hg, cg), (hw, cw), got, want = _cell_both(lstm_ops, t, use_h, use_c)
        assert rel(hg, hw) < OUT_BAR and rel(cg, cw) < OUT_BAR
        for k in got:
            assert rel(got[k], want[k]) < GRAD_BAR, (k, rel(got[k], want[k]))
    # zero state through null pointers against explicit zeros: equal bits; and against float64
    z = {**t, "h": torch.zeros(M, H), "c": torch.zeros(M, H)}
    (h0, c0), (hw, cw), got0, want0 = _cell_both(lstm_ops, t, gh, gc, zero_state=True)
    (h1, c1), _, got1, _ = _cell_both(lstm_ops, z, gh, gc)
    assert torch.equal(h0, h1) and torch.equal(c0, c1) and rel(h0, hw) < OUT_BAR and rel(c0, cw) < OUT_BAR
    for k in got0:
        if k == "w_hh":
            assert float(got0[k].abs().max()) == 0.0 and float(got1[k].abs().max()) == 0.0
        else:
            assert torch.equal(got0[k], got1[k]) and rel(got0[k], want0[k]) < GRAD_BAR, k


def test_cell_chained_steps_saturation_and_layouts(vpx):
    from vp_suite_amd import lstm_ops
    M, Kx, H = 3, 33, 130
    t = _cell_inputs(M, Kx, H, "lstm.cell.chain")
    x2, gh = _rn((M, Kx), "lstm.cell.chain.x2"), _rn((M, H), "lstm.cell.chain.gh")
    d = {k: v.double().requires_grad_(True) for k, v in t.items()}
    g = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
    wp = ("w_ih", "w_hh", "b_ih", "b_hh")
    hw, cw = lstm_ref.cell_ref(x2.double(), *lstm_ref.cell_ref(d["x"], d["h"], d["c"], *(d[k] for k in wp)), *(d[k] for k in wp))
    hg, cg = lstm_ops.lstm_cell(x2.cuda(), lstm_ops.lstm_cell(g["x"], (g["h"], g["c"]), *(g[k] for k in wp)), *(g[k] for k in wp))
    assert rel(hg, hw) < OUT_BAR and rel(cg, cw) < OUT_BAR
    want = torch.autograd.grad((hw * gh.double()).sum(), [d[k] for k in ORDER])
    got = torch.autograd.grad((hg * gh.cuda()).sum(), [g[k] for k in ORDER])
    for k, a, r in zip(ORDER, got, want):
        assert rel(a, r) < GRAD_BAR, k
    # pre-activations scaled to +-30: saturated gates stay finite and within the bar
    ts = _cell_inputs(M, Kx, H, "lstm.cell.sat", scale=30.0)
    (hg, cg), (hw, cw), got, want = _cell_both(lstm_ops, ts, gh, gh)
    assert bool(torch.isfinite(hg).all()) and bool(torch.isfinite(cg).all()) and rel(hg, hw) < OUT_BAR and rel(cg, cw) < OUT_BAR
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and rel(got[k], want[k]) < GRAD_BAR, k
    # non-contiguous inputs are copied
    tc = {k: v.cuda() for k, v in t.items()}
    ref = lstm_ops.lstm_cell(tc["x"], (tc["h"], tc["c"]), *(tc[k] for k in wp))
    xt, ht = tc["x"].t().contiguous().t(), tc["h"].t().contiguous().t()
    wt = tc["w_ih"].t().contiguous().t()
    assert not xt.is_contiguous() and not wt.is_contiguous()
    out = lstm_ops.lstm_cell(xt, (ht, tc["c"]), wt, tc["w_hh"], tc["b_ih"], tc["b_hh"])
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


# ---- replicate stride-2 convolution and resize ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", ((1, 1), (2, 2), (5, 3), (8, 12), (16, 33)))
@pytest.mark.parametrize("ci,co", ((1, 1), (3, 3), (64, 5)))
def test_conv2d_replicate_forward_and_gradients(vpx, hw, ci, co):
    from vp_suite_amd import lstm_ops
    tag = f"lstm.rconv.{hw}.{ci}.{co}"
    x, w, b = _rn((2, ci, *hw), tag + ".x"), _rn((co, ci, 3, 3), tag + ".w", 1 / np.sqrt(9 * ci)), _rn((co,), tag + ".b")
    for relu in (True, False):
        d = [t.double().requires_grad_(True) for t in (x, w, b)]
        conv = torch.nn.functional.conv2d(torch.nn.functional.pad(d[0], (1, 1, 1, 1), mode="replicate"), d[1], d[2], stride=2)
        want = torch.relu(conv) if relu else conv
        gy = _rn(want.shape, tag + ".gy")
        g = [t.cuda().requires_grad_(True) for t in (x, w, b)]
        got = lstm_ops.conv2d_replicate(g[0], g[1], g[2], stride=2, relu=relu)
        assert tuple(got.shape) == tuple(want.shape) and rel(got, want) < OUT_BAR
        gw = torch.autograd.grad((want * gy.double()).sum(), d)
        gg = torch.autograd.grad((got * gy.cuda()).sum(), g)
        gg2 = torch.autograd.grad((lstm_ops.conv2d_replicate(g[0], g[1], g[2], stride=2, relu=relu) * gy.cuda()).sum(), g)
        for a, a2, r in zip(gg, gg2, gw):
            assert rel(a, r) < GRAD_BAR or float(r.abs().max()) == 0.0
    # the padding's adjoint alone: bit-reproducible
    xp = x.cuda().requires_grad_(True)
    gp = _rn((2, ci, hw[0] + 2, hw[1] + 2), tag + ".gp").cuda()
    r1 = torch.autograd.grad((lstm_ops.replicate_pad(xp, 1) * gp).sum(), xp)[0]
    r2 = torch.autograd.grad((lstm_ops.replicate_pad(xp, 1) * gp).sum(), xp)[0]
    xd = x.double().requires_grad_(True)
    rw = torch.autograd.grad((lstm_ref.replicate_pad_ref(xd, 1) * gp.cpu().double()).sum(), xd)[0]
    assert torch.equal(r1, r2) and rel(r1, rw) < GRAD_BAR
    assert torch.equal(lstm_ops.replicate_pad(xp, 1).detach().cpu(), lstm_ref.replicate_pad_ref(x, 1))


@pytest.mark.parametrize("src", ((1, 1), (2, 3), (9, 17)))
@pytest.mark.parametrize("dst", ((16, 24), (20, 12)))
def test_resize_bilinear_forward_and_adjoint(vpx, src, dst):
    from vp_suite_amd import lstm_ops
    tag = f"lstm.resize.{src}.{dst}"
    for C in (1, 3):
        x = _rn((2, C, *src), tag + f".{C}")
        xd = x.double().requires_grad_(True)
        want = lstm_ref.resize_ref(xd, dst)
        xg = x.cuda().requires_grad_(True)
        got = lstm_ops.resize_bilinear(xg, dst)
        assert got.is_contiguous() and tuple(got.shape) == (2, C, *dst)
        bound = 10 * 2.0 ** -24 * torch.clamp_min(want.detach().abs(), 1.0)
        assert bool(((got.detach().cpu().double() - want.detach()).abs() <= bound).all())
        gy = _rn(want.shape, tag + f".gy{C}")
        gw = torch.autograd.grad((want * gy.double()).sum(), xd)[0]
        g1 = torch.autograd.grad((got * gy.cuda()).sum(), xg)[0]
        g2 = torch.autograd.grad((lstm_ops.resize_bilinear(xg, dst) * gy.cuda()).sum(), xg)[0]
        assert torch.equal(g1, g2) and rel(g1, gw) < GRAD_BAR


# ---- model ----------------------------------------------------------------------------------------------------------------------------
def _models(tag, kw, **extra):
    from vp_suite_amd.models import MODEL_CLASSES
    m = MODEL_CLASSES["nc-lstm"]("cpu", **{**kw, **extra})
    fill_state_dict_(m, name_seed(f"lstm.{tag}"))
    return m.to("cuda"), m.state_dict()


def _named_grads(m):
    return {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("tag,kw", [("tiny", LSTM_TINY_KW), ("tiny3", LSTM_TINY3_KW)])
def test_model_encode_decode_and_literal_forward_vs_reference_fixture(vpx, tag, kw):
    g = load_golden(f"lstm_{tag}")
    m, _ = _models(tag, kw, carry_state=False)
    B = LSTM_TINY_B
    c, h, w = kw["img_shape"]
    x0 = seeded_rand((B, c, h, w), name_seed(f"lstm.{tag}.x0")).cuda().requires_grad_(True)
    z = seeded_randn((B, kw["lstm_hidden_dim"]), name_seed(f"lstm.{tag}.latent")).cuda().requires_grad_(True)
    enc, dec = m.encode(x0), m.decode(z)
    assert rel(enc, torch.from_numpy(g["enc"])) < OUT_BAR and rel(dec, torch.from_numpy(g["dec"])) < OUT_BAR
    ge, gd = seeded_randn(enc.shape, name_seed(f"lstm.{tag}.ge")).cuda(), seeded_randn(dec.shape, name_seed(f"lstm.{tag}.gd")).cuda()
    ((enc * ge).sum() + (dec * gd).sum()).backward()
    named = {n: p for n, p in _named_grads(m).items() if not n.startswith("rnn_layers.")}
    assert all(p.grad is None for p in m.rnn_layers.parameters())
    named["__x0__"], named["__z__"] = x0.grad, z.grad
    _check_grads(g, "ed", {k: v for k, v in named.items() if v is not None}, GRAD_BAR)
    # the literal forward, pred_1, gradient summaries and where .grad is None
    ctx, pred = (LSTM_TINY_CTX, LSTM_TINY_PRED) if tag == "tiny" else (LSTM_TINY3_CTX, LSTM_TINY3_PRED)
    x = seeded_rand((B, ctx, c, h, w), name_seed(f"lstm.{tag}.x")).cuda()
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9
    actions = seeded_randn((B, ctx + pred, 3), name_seed("lstm.tiny3.actions")).cuda() if tag == "tiny3" else None
    m.zero_grad(set_to_none=True)
    out, ml = m(x, pred_frames=pred, actions=actions)
    assert ml is None and tuple(out.shape) == (B, pred, c, h, w) and rel(out, torch.from_numpy(g["fwd"])) < OUT_BAR
    if tag == "tiny":
        assert rel(m.pred_1(x), torch.from_numpy(g["pred1"])) < OUT_BAR
        (out * out).sum().backward()
        grads = _named_grads(m)
        none = sorted(str(n) for n in g["fwd.none"] if str(n))
        assert sorted(n for n, v in grads.items() if v is None and not n.startswith("rnn_layers.")) == none
        assert all(v is None for n, v in grads.items() if n.startswith("rnn_layers."))
        _check_grads(g, "fwd", {k: v for k, v in grads.items() if v is not None}, GRAD_BAR)
    else:
        got = __import__("vp_suite_amd").lstm_ops.dense(actions[:, 0].flatten(1), m.action_inflate.weight, m.action_inflate.bias)
        assert rel(got, torch.from_numpy(g["inflate"])) < OUT_BAR


def test_model_default_encode_decode_vs_reference_fixture(vpx):
    g = load_golden("lstm_default")
    m, _ = _models("default", LSTM_DEFAULT_KW)
    x = seeded_rand((1, 1, 64, 64), name_seed("lstm.default.x"))
    assert abs(checksum(x) - float(g["chk_x"])) < 1e-9
    with torch.no_grad():
        z = m.encode(x.cuda())
        out = m.decode(z)
    assert rel(z[:, ::4], torch.from_numpy(g["z_slice"])) < OUT_BAR and rel(out[:, :, ::4, ::4], torch.from_numpy(g["out_slice"])) < OUT_BAR
    assert abs(checksum(out) - float(g["out_chk"])) < 1e-3 * max(1.0, abs(float(g["out_chk"])))


@pytest.mark.parametrize("tag,kw,ctx,pred", [("tiny", LSTM_TINY_KW, LSTM_TINY_CTX, LSTM_TINY_PRED), ("tiny3", LSTM_TINY3_KW, LSTM_TINY3_CTX, LSTM_TINY3_PRED)])
def test_model_carried_state_forward_and_gradients_vs_oracle(vpx, tag, kw, ctx, pred):
    m, sd = _models(tag, kw)
    ref = lstm_ref.RefLSTM(sd, kw["img_shape"], action_conditional=kw.get("action_conditional", False), requires_grad=True)
    B = LSTM_TINY_B
    c, h, w = kw["img_shape"]
    x = seeded_rand((B, ctx, c, h, w), name_seed(f"lstm.{tag}.x"))
    actions = seeded_randn((B, ctx + pred, 3), name_seed("lstm.tiny3.actions")) if tag == "tiny3" else None
    want = ref.forward(x.double(), pred, None if actions is None else actions.double())
    got, ml = m(x.cuda(), pred_frames=pred, actions=None if actions is None else actions.cuda())
    assert ml is None and rel(got, want) < OUT_BAR
    (want * want).sum().backward()
    (got * got).sum().backward()
    grads = _named_grads(m)
    assert all(v is not None for v in grads.values())
    for n, v in grads.items():
        assert rel(v, ref.p[n].grad) < GRAD_BAR, (n, rel(v, ref.p[n].grad))
    # a prediction that changes when a context frame changes (the literal model's cannot)
    x2 = x.clone()
    x2[:, 0] = 1 - x2[:, 0]
    with torch.no_grad():
        moved = m(x2.cuda(), pred_frames=pred, actions=None if actions is None else actions.cuda())[0]
    assert float((moved - got).abs().max()) > 1e-6


def test_model_train_and_eval_iter(vpx):
    from vp_suite_amd.measure import PredictionLossProvider
    m, _ = _models("tiny", LSTM_TINY_KW)
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    cfg = {"device": "cuda", "context_frames": 3, "pred_frames": 2, "val_rec_criterion": "mse"}
    data = {"frames": seeded_rand((2, 5, 1, 16, 24), name_seed("lstm.tiny.frames")), "actions": torch.zeros(2, 4, 0)}
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    m0 = m.eval_iter(cfg, [data], lp)[0]["mse"]
    for _ in range(3):
        m.train_iter(cfg, [data], opt, lp, epoch=0)
    assert all(not torch.equal(p, before[n]) for n, p in m.named_parameters())
    assert m.eval_iter(cfg, [data], lp)[0]["mse"] < m0 and m.training


def test_suite_trains_and_tests_nc_lstm_on_mmf(vpx, tmp_path):
    run = dict(context_frames=3, pred_frames=2)
    digits = vpx.datasets.procedural_digits(n=10, size=12)
    suite = vpx.VPSuite()
    suite.load_dataset("MMF", split="train", digits=digits, n_seqs=4, img_size=32, num_channels=3)
    suite.create_model("nc-lstm", bottleneck_dim=32, lstm_hidden_dim=24, lstm_num_layers=2)
    model = suite.models[-1]
    assert model.NAME == "NonConvLSTM" and (model.bottleneck_dim, model.lstm_hidden_dim) == (32, 24) and model.img_shape == (3, 32, 32)
    best = suite.train(epochs=1, batch_size=2, out_dir=str(tmp_path / "run"), **run)
    assert np.isfinite(best) and os.path.isfile(tmp_path / "run" / "best_model.pth")
    suite.load_dataset("MMF", split="test", digits=digits, n_seqs=3, img_size=32, num_channels=3)
    (models,) = suite.test(**run).values()
    assert model.NAME in models and all(np.isfinite(v) for row in models[model.NAME] for v in row.values())


def test_action_conditional_model_receives_bair_actions(vpx, tmp_path, monkeypatch):
    """On a synthetic "BAIR" directory the action-conditional model is handed the dataset's actions, and its prediction depends on them."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_bair_like
    export_bair_like.export(str(tmp_path / "data"), {"train": 4, "test": 2}, seed=3)
    run = dict(context_frames=2, pred_frames=2, seq_step=2)
    suite = vpx.VPSuite()
    suite.load_dataset("BAIR", data_dir=str(tmp_path / "data"), img_size=16)
    suite.create_model("nc-lstm", action_conditional=True, bottleneck_dim=30, lstm_hidden_dim=16, lstm_num_layers=2)
    model = suite.models[-1]
    assert model.action_conditional and model.action_size == 4 and model.bottleneck_dim == 33
    received = []
    forward = type(model).forward

    def recording_forward(self, x, pred_frames=1, **kwargs):
        acts = kwargs.get("actions")
        received.append(None if acts is None else tuple(acts.shape))
        return forward(self, x, pred_frames=pred_frames, **kwargs)
    monkeypatch.setattr(type(model), "forward", recording_forward)
    best = suite.train(epochs=1, batch_size=2, out_dir=str(tmp_path / "run"), **run)
    monkeypatch.undo()
    assert np.isfinite(best) and received and all(r is not None and r[-1] == 4 for r in received)
    suite.load_dataset("BAIR", split="test", data_dir=str(tmp_path / "data"), img_size=16)
    (models,) = suite.test(**run).values()
    assert all(np.isfinite(v) for row in models[model.NAME] for v in row.values())
    data = suite.test_sets[-1].test_data.batch([0, 1])
    model.eval()
    with torch.no_grad():
        pred, _ = model(data["frames"][:, :2], pred_frames=2, actions=data["actions"])
        negated, _ = model(data["frames"][:, :2], pred_frames=2, actions=-data["actions"])
    assert torch.isfinite(pred).all() and float((pred - negated).abs().max()) > 0
