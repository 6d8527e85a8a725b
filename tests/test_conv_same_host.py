"""The stride-1 'same' convolution family on the CPU: the fp64 statement of tests/conv_same_ref.py checked against closed forms, the
conditions under which tests/test_gpu_conv_same.py may hold the kernels to the project's bars (the reference's own fp32 run stays inside a
fifth of them; next to nothing sits on LeakyReLU's kink), and — in a dry run (VPX_OPT_DRY_RUN, as tests/test_workspace_contract.py) —
every case of every table through vpx_conv2d_nhwc_fwd / _fwd_ex / _bwd with a workspace of exactly the queried size, and the refusals
with their documented codes."""
import ctypes

import pytest
import torch

import conv_same_ref as R
from vp_suite_amd import _lib

OK, E_ARG, E_WS, E_UNSUPPORTED = 0, -1, -2, -4
WS_BASE = 0x7F0000000000            # fake workspace address (256-byte aligned; never dereferenced in a dry run)
WS_BASE_ODD = WS_BASE + 0x40        # ... and one that is not 256-byte aligned
PRECS = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}
CASES = R.all_cases()
IDS = [R.case_id(t, i) for t, i in CASES]


def _fake(i):                        # distinct fake tensor addresses far away from the workspace
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


# ---- the reference against closed forms ----------------------------------------------------------------------------------------------
def test_one_hot_weight_is_a_shift_with_zero_fill():
    """w = 1 at tap (ky, kx) of a 3 x 5 kernel: y[i, j] = x[i + ky - 1, j + kx - 2], zero outside the map."""
    x = torch.arange(2 * 1 * 4 * 6, dtype=torch.float32).reshape(2, 1, 4, 6) + 1.0
    kh, kw = 3, 5
    for ky in range(kh):
        for kx in range(kw):
            w = torch.zeros(1, 1, kh, kw)
            w[0, 0, ky, kx] = 1.0
            y = R.reference(x, w, None, torch.ones(2, 1, 4, 6))["y"]
            dy, dx = ky - kh // 2, kx - kw // 2
            want = torch.zeros(2, 1, 4, 6, dtype=torch.float64)
            for i in range(4):
                for j in range(6):
                    if 0 <= i + dy < 4 and 0 <= j + dx < 6:
                        want[:, 0, i, j] = x[:, 0, i + dy, j + dx].double()
            assert torch.equal(y, want), (ky, kx)


def test_accumulate_then_leaky_on_the_sum():
    """1 x 1, one channel: conv = 3 * (-2) + 0.5 = -5.5. With acc0 = 10 the sum is 4.5 and passes LeakyReLU(0.2) unchanged (activating
    the convolution first would give -1.1 + 10 = 8.9); with acc0 = 1 the sum is -4.5 and y = -0.9 (the other order: -0.1)."""
    x, w, b = torch.full((1, 1, 1, 1), 3.0), torch.full((1, 1, 1, 1), -2.0), torch.tensor([0.5])
    gy = torch.full((1, 1, 1, 1), 4.0)
    r = R.reference(x, w, b, gy, torch.full((1, 1, 1, 1), 10.0), 0.2)
    assert abs(float(r["y"]) - 4.5) < 1e-15 and abs(float(r["pre"]) - 4.5) < 1e-15
    assert abs(float(r["dx"]) - 4.0 * -2.0) < 1e-15 and abs(float(r["dw"]) - 4.0 * 3.0) < 1e-15 and abs(float(r["db"]) - 4.0) < 1e-15
    r = R.reference(x, w, b, gy, torch.full((1, 1, 1, 1), 1.0), 0.2)
    assert abs(float(r["y"]) - (-0.9)) < 1e-15 and abs(float(r["pre"]) - (-4.5)) < 1e-15
    # d/dx = gy * slope * w, d/dw = gy * slope * x, d/db = gy * slope
    assert abs(float(r["dx"]) - 4.0 * 0.2 * -2.0) < 1e-15 and abs(float(r["dw"]) - 4.0 * 0.2 * 3.0) < 1e-15 and abs(float(r["db"]) - 0.8) < 1e-15
    assert float(R.reference(x, w, b, gy)["y"]) == -5.5                     # no accumulate, no activation


def test_bias_gradient_is_the_column_sum_of_gy():
    for table, i in (("MAPS", 6), ("KERNELS", 4), ("TILING", 9)):
        t, ref = R.case(table, i)
        assert R.relmax(ref["db"], t["gy"].double().sum(dim=(0, 2, 3))) < 1e-14
    t, ref = R.case(*R.EXPANDED, bias=True, ones=True)
    N, _, Co, _, _, H, W = R.TABLES[R.EXPANDED[0]][R.EXPANDED[1]]
    assert torch.equal(ref["db"], torch.full((Co,), float(N * H * W), dtype=torch.float64))


def test_tables_are_what_the_kernels_need():
    assert sorted({c[2] for c in R.TILING}) == [1, 5, 32, 33, 64, 70, 96, 97, 128, 130]
    assert {(c[1], c[2]) for c in R.TILING if c[1] == 130} == {(130, 33), (130, 130)}
    assert [c[1] for c in R.CHANNELS] == [1, 3, 7, 8, 9, 16, 17, 40, 65, 130]
    assert {(c[3], c[4]) for c in R.KERNELS} == {(1, 1), (3, 3), (5, 5), (7, 7), (3, 5), (5, 3), (1, 7), (7, 1)}
    assert {(c[5], c[6]) for c in R.MAPS} == {(1, 1), (1, 17), (9, 1), (2, 3), (8, 16), (9, 17), (16, 33)}
    assert {c[0] for c in R.MAPS} == {1, 3} and {c[3] for c in R.MAPS} == {3, 7} and len(R.MAPS) == 28
    for c in R.KSPLIT_FWD:
        assert c[1] > 64            # contraction over Ci: at least two stages
    for c in R.KSPLIT_BWD:
        assert c[2] > 64            # the data gradient contracts over Co
    for table, i in CASES:
        N, Ci, Co, kh, kw, H, W = R.TABLES[table][i]
        assert N * Co * H * W <= 2e5 or table == "SLICES", R.case_id(table, i)    # (40 work items are what tells the slice caps apart)
    for table, i in R.FWD_EX + R.PLAIN_BF16 + [R.EXPANDED]:
        assert i < len(R.TABLES[table])
    v = [R.variant(t, i) for t in R.SAME_TABLES for i in range(len(R.TABLES[t]))]
    assert sum(a["expanded"] for a in v) == 1
    for t in R.SAME_TABLES:
        vt = [R.variant(t, i) for i in range(len(R.TABLES[t]))]
        assert {a["bias"] for a in vt} == {True, False} and {a["channels_last"] for a in vt} == {True, False}


# ---- the reference alone stays inside the bars ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,i", CASES, ids=IDS)
def test_fp32_reference_holds_a_fifth_of_the_f32_bars(table, i):
    t, ref = R.case(table, i)
    r32 = R.reference(t["x"], t["w"], t["b"], t["gy"], dtype=torch.float32)
    fwd, grad = R.BARS["f32"]
    errs = {k: R.relmax(r32[k], ref[k]) for k in ("y", "dx", "dw", "db")}
    print(R.case_id(table, i), {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["y"] < R.HOST_SHARE * fwd, errs
    for k in ("dx", "dw", "db"):
        assert errs[k] < R.HOST_SHARE * grad, errs


@pytest.mark.parametrize("table,i", R.FWD_EX, ids=[R.case_id(t, i) for t, i in R.FWD_EX])
def test_next_to_nothing_sits_on_the_kink(table, i):
    """The inputs of test_conv2d_fwd_ex_accumulate_and_leaky_vs_fp64: at most 0.1 % of the fp64 pre-activations lie within a forward bar
    (times max|ref|) of zero, with and without the accumulate, in every operand mode the test runs."""
    for acc in (False, True):
        _, ref = R.case(table, i, acc=acc, slope=R.SLOPE)
        for prec in ("f32", "bf16x3"):
            keep = R.off_kink(ref, R.BARS[prec][0])
            share = 1.0 - float(keep.double().mean())
            print(R.case_id(table, i), f"acc={acc} {prec}: {share:.2e} of {keep.numel()} excluded")
            assert share <= R.KINK_SHARE, (acc, prec, share)


# ---- dry run -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    lib = _lib.lib()
    with _lib.option(_lib.OPT_DRY_RUN, 1):
        yield lib
    lib.vpx_set_deterministic(0)


def _must(L, rc, what, want=OK):
    assert rc == want, f"{what}: rc={rc}, expected {want}: {L.vpx_last_error().decode()}"


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", list(PRECS))
def test_every_case_carves_exactly_the_queried_workspace(L, prec, det):
    """No case of any table is refused: rc == 0 throughout."""
    L.vpx_set_deterministic(det)
    p = PRECS[prec]
    for table, i in CASES:
        N, Ci, Co, kh, kw, H, W = R.TABLES[table][i]
        tag = f"{R.case_id(table, i)} {prec} det={det}"
        nb = L.vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)
        nbw = L.vpx_conv2d_bwd_workspace_bytes(N, H, W, Ci, Co, kh, kw)
        assert nb > 0 and nbw > 0, tag
        for base in (WS_BASE, WS_BASE_ODD):
            ws = ctypes.c_void_p(base)
            _must(L, L.vpx_conv2d_nhwc_fwd(_fake(1), _fake(2), _fake(3), _fake(4), N, H, W, Ci, Co, kh, kw, p, ws, nb, None), tag + " fwd")
            _must(L, L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), N, H, W, Ci, Co, kh, kw, p, 0, 0.0, ws, nb, None), tag + " fwd_ex")
            _must(L, L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), None, _fake(4), N, H, W, Ci, Co, kh, kw, p, 1, 0.2, ws, nb, None),
                  tag + " fwd_ex(accumulate, leaky)")
            _must(L, L.vpx_conv2d_nhwc_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), N, H, W, Ci, Co, kh, kw, p, ws, nbw, None),
                  tag + " bwd")


def _calls(L, N, H, W, Ci, Co, kh, kw, prec=0, slope=0.0, x=_fake(1), w=_fake(2), y=_fake(4), short=0):
    """(name, rc, message) of the three entry points on one problem; `short`: bytes taken off the queried workspace."""
    nb = L.vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)
    nbw = L.vpx_conv2d_bwd_workspace_bytes(N, H, W, Ci, Co, kh, kw)
    ws = ctypes.c_void_p(WS_BASE)
    out = []
    for name, call in (
            ("fwd", lambda: L.vpx_conv2d_nhwc_fwd(x, w, _fake(3), y, N, H, W, Ci, Co, kh, kw, prec, ws, max(nb - short, 0), None)),
            ("fwd_ex", lambda: L.vpx_conv2d_nhwc_fwd_ex(x, w, _fake(3), y, N, H, W, Ci, Co, kh, kw, prec, 0, slope, ws, max(nb - short, 0), None)),
            ("bwd", lambda: L.vpx_conv2d_nhwc_bwd(x, w, y, _fake(5), _fake(6), _fake(7), N, H, W, Ci, Co, kh, kw, prec, ws, max(nbw - short, 0), None))):
        rc = call()
        out.append((name, rc, L.vpx_last_error().decode()))
    return out


def test_refusals(L):
    """Each refusal returns its documented code (include/vpx.h) and leaves a message."""
    L.vpx_set_deterministic(0)
    geo = (2, 9, 17, 8, 8)
    for kh, kw in ((2, 2), (3, 4), (9, 9), (3, 9)):                       # even kernels, kernels past 7
        for name, rc, msg in _calls(L, *geo, kh, kw):
            assert rc == E_ARG and msg, (name, kh, kw, rc, msg)
    assert L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), *geo, 3, 3, 0, 0, -0.1, ctypes.c_void_p(WS_BASE),
                                    L.vpx_conv2d_workspace_bytes(8, 8, 3, 3), None) == E_ARG and L.vpx_last_error()
    for name, rc, msg in _calls(L, *geo, 3, 3, prec=3):
        assert rc == E_UNSUPPORTED and "not implemented" in msg, (name, rc, msg)
    for null in ("x", "w", "y"):                                         # (bwd: y stands for dy)
        for name, rc, msg in _calls(L, *geo, 3, 3, **{null: None}):
            assert rc == E_ARG and msg, (null, name, rc, msg)
    for bad in ((0, 9, 17, 8, 8), (2, 0, 17, 8, 8), (2, 9, 0, 8, 8), (2, 9, 17, 0, 8), (2, 9, 17, 8, 0)):
        for name, rc, msg in _calls(L, *bad, 3, 3):
            assert rc == E_ARG and msg, (bad, name, rc, msg)
    # more channel stages than a plan holds
    assert L.vpx_conv2d_workspace_bytes(2049, 8, 1, 1) == 0
    ws = ctypes.c_void_p(WS_BASE)
    rc = L.vpx_conv2d_nhwc_fwd(_fake(1), _fake(2), _fake(3), _fake(4), 1, 1, 1, 2049, 8, 1, 1, 0, ws, 1 << 20, None)
    assert rc == E_UNSUPPORTED and b"too many channel stages" in L.vpx_last_error()
    rc = L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), 1, 1, 1, 2049, 8, 1, 1, 0, 0, 0.0, ws, 1 << 20, None)
    assert rc == E_UNSUPPORTED and b"too many channel stages" in L.vpx_last_error()
    assert L.vpx_conv2d_workspace_bytes(2048, 8, 1, 1) > 0               # (the last count it takes)
    # a workspace one byte short, and none at all
    for name, rc, msg in _calls(L, *geo, 3, 3, short=1):
        assert rc == E_WS and "workspace" in msg, (name, rc, msg)
    rc = L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), *geo, 3, 3, 0, 0, 0.0, None, 1 << 20, None)
    assert rc == E_WS
    for name, rc, msg in _calls(L, *geo, 3, 3):                          # the next valid call succeeds
        assert rc == OK, (name, rc, msg)
