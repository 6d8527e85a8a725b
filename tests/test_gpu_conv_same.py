"""The stride-1 'same' convolution family on the GPU — vpx_conv2d_nhwc_fwd (behind ops.conv2d_same), vpx_conv2d_nhwc_fwd_ex and
vpx_conv2d_nhwc_bwd — against the fp64 statement of tests/conv_same_ref.py, whose tables walk the N tilings (EpiPlain<1..4>, the partly
filled tail tile), the channel padding, contractions of several stages, the K split over workgroups, accumulate + LeakyReLU, rectangular
kernels (the transposed, tap-flipped pack of the data gradient; the tap groups of the weight gradient), both slice caps of the weight
gradient, and maps from one pixel to two tiles and a column.

Every comparison is max|got - ref| / max|ref| against the fp64 run and goes through the parity record (parity_log; parity.relmax for the
comparisons of two launches with each other). Bars (conv_same_ref.BARS), forward / gradients: f32 1e-5 / 2e-5, bf16x3 5e-5 / 1e-4,
bf16 2e-2 / 2e-2 — the project's own figures; the fp32 CPU run of the reference holds a fifth of the f32 ones on every case
(tests/test_conv_same_host.py). A dropped tap, halo column, tail channel or stage moves a result by 1e-2 or more.

Destinations come from torch.empty: the guard bands of tests/canary.py stand around every one of them and around every workspace, each
of exactly the queried size.

Measured, one MI355X run of this file (every figure below is in that run's parity record — the parity_r06.json that
tests/conftest.py writes at the end of a `-m gpu` session — under this file's test names; profiles/parity_r06.json is the record of an earlier
run and does not hold them yet); worst over the cases:
  test_conv2d_same_vs_fp64              f32:    y 1.2e-6 (TILING Ci=130 Co=33), dx 6.9e-7, dw 4.5e-7, db 2.5e-7
                                        bf16x3: y 8.7e-6 (MAPS 7x7 on 1x17), dx 7.1e-6, dw 1.2e-5 (MAPS 3x3 on 2x3), db 2.5e-7
  test_conv2d_fwd_ex_accumulate_and_... f32 1.2e-6, bf16x3 5.4e-6
  test_k_split_and_single_pass_...      f32: y 9.4e-7, dx 1.7e-6; bf16x3: y 5.1e-6, dx 6.1e-6; split against single pass 1.8e-6 (bar 2e-5)
  test_weight_gradient_slices_...       f32: dw 3.6e-7, db 1.9e-7; bf16x3: dw 5.4e-6
  test_plain_bf16_mode_...              y 2.6e-3, dx 2.7e-3, dw 3.1e-3
No case needed a bar other than the table's: none was derived from the reference's fp32 error. Not measured: nothing — every test of the
file ran. The file takes 4 s."""
import ctypes

import pytest
import torch

import conv_same_ref as R
from parity import relmax as _relmax

pytestmark = pytest.mark.gpu

PRECS = ("f32", "bf16x3")
SENTINEL = -7.0e30
SAME_CASES = [(t, i, p) for t in R.SAME_TABLES for i in range(len(R.TABLES[t])) for p in PRECS]


def _ids(cases):
    return [R.case_id(c[0], c[1]) + "".join(f"-{e}" for e in c[2:]) for c in cases]


def _hold(parity_log, name, got, ref, bar):
    e = parity_log(name, got, ref, bar)
    print(f"  {name}: {e:.3e} (bar {bar:.0e})")
    assert e < bar, (name, e, bar)
    return e


def _nhwc(t):
    """[N, C, H, W] on the CPU -> the library's dense [N, H, W, C] on the GPU."""
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def _filled(shape, value):
    return torch.empty(shape, device="cuda").fill_(value)


class _Lib:
    """The three entry points through ctypes on dense NHWC buffers, each call with a fresh workspace of exactly the queried size."""

    def __init__(self, vpx):
        self.vpx, self.L, self.p = vpx, vpx._lib.lib(), vpx._lib.ptr

    def fwd_ex(self, geo, prec, x, w, b, y, accumulate=0, slope=0.0, ws_short=0, fn="fwd_ex"):
        N, Ci, Co, kh, kw, H, W = geo
        nb = self.L.vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
        p = self.p
        if fn == "fwd":
            return self.L.vpx_conv2d_nhwc_fwd(p(x), p(w), p(b), p(y), N, H, W, Ci, Co, kh, kw, self.vpx.ops.PRECISIONS.get(prec, prec),
                                              p(ws), max(nb - ws_short, 0), self.vpx.ops.stream())
        return self.L.vpx_conv2d_nhwc_fwd_ex(p(x), p(w), p(b), p(y), N, H, W, Ci, Co, kh, kw, self.vpx.ops.PRECISIONS.get(prec, prec),
                                             accumulate, slope, p(ws), max(nb - ws_short, 0), self.vpx.ops.stream())

    def bwd(self, geo, prec, x, w, dy, dx, dw, db, ws_short=0):
        N, Ci, Co, kh, kw, H, W = geo
        nb = self.L.vpx_conv2d_bwd_workspace_bytes(N, H, W, Ci, Co, kh, kw)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
        p = self.p
        return self.L.vpx_conv2d_nhwc_bwd(p(x), p(w), p(dy), p(dx), p(dw), p(db), N, H, W, Ci, Co, kh, kw, self.vpx.ops.PRECISIONS.get(prec, prec),
                                          p(ws), max(nb - ws_short, 0), self.vpx.ops.stream())

    def ok(self, rc, what):
        assert rc == 0, f"{what}: rc={rc}: {self.L.vpx_last_error().decode()}"


@pytest.fixture
def lib(vpx):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    vpx.ops.sync_determinism()
    return _Lib(vpx)


# ---- ops.conv2d_same: forward and the three gradients ---------------------------------------------------------------------------------
@pytest.mark.parametrize("table,i,prec", SAME_CASES, ids=_ids(SAME_CASES))
def test_conv2d_same_vs_fp64(vpx, parity_log, table, i, prec):
    v = R.variant(table, i)
    N, Ci, Co, kh, kw, H, W = R.TABLES[table][i]
    t, ref = R.case(table, i, bias=v["bias"], ones=v["expanded"])
    print(R.case_id(table, i), prec, v)
    x = t["x"].cuda()
    if v["channels_last"]:
        x = x.contiguous(memory_format=torch.channels_last)
    leaves = [x.requires_grad_(True), t["w"].cuda().requires_grad_(True)] + ([t["b"].cuda().requires_grad_(True)] if v["bias"] else [])
    y = vpx.ops.conv2d_same(leaves[0], leaves[1], leaves[2] if v["bias"] else None, precision=prec)
    assert y.shape == (N, Co, H, W) and y.permute(0, 2, 3, 1).is_contiguous()
    # torch.autograd.grad hands out what the backward returned (a leaf's .grad would be restrided to the leaf's own layout)
    grads = torch.autograd.grad(y.sum(), leaves) if v["expanded"] else torch.autograd.grad(y, leaves, t["gy"].cuda())
    dx, dw = grads[0], grads[1]
    assert dx.shape == (N, Ci, H, W) and dx.permute(0, 2, 3, 1).is_contiguous()
    assert dw.shape == (Co, Ci, kh, kw) and dw.stride() == leaves[1].stride()
    fwd, grad = R.BARS[prec]
    _hold(parity_log, "y", y, ref["y"], fwd)
    _hold(parity_log, "dx", dx, ref["dx"], grad)
    _hold(parity_log, "dw", dw, ref["dw"], grad)
    if v["bias"]:
        assert grads[2].shape == (Co,)
        _hold(parity_log, "db", grads[2], ref["db"], grad)


PLAIN_BF16 = list(R.PLAIN_BF16)


@pytest.mark.parametrize("table,i", PLAIN_BF16, ids=_ids(PLAIN_BF16))
def test_plain_bf16_mode_through_conv2d_same(vpx, parity_log, table, i):
    """VPX_PREC_BF16 (bf16 operands, fp32 accumulate) through this entry: its own bar, forward and gradients."""
    t, ref = R.case(table, i)
    leaves = [t[k].cuda().requires_grad_(True) for k in ("x", "w", "b")]
    y = vpx.ops.conv2d_same(*leaves, precision="bf16")
    grads = torch.autograd.grad(y, leaves, t["gy"].cuda())
    fwd, grad = R.BARS["bf16"]
    _hold(parity_log, "y", y, ref["y"], fwd)
    for k, g in zip(("dx", "dw", "db"), grads):
        _hold(parity_log, k, g, ref[k], grad)


# ---- vpx_conv2d_nhwc_fwd_ex: accumulate and LeakyReLU -----------------------------------------------------------------------------------
FWD_EX = [(t, i, p) for t, i in R.FWD_EX for p in PRECS]


@pytest.mark.parametrize("table,i,prec", FWD_EX, ids=_ids(FWD_EX))
def test_conv2d_fwd_ex_accumulate_and_leaky_vs_fp64(lib, parity_log, table, i, prec):
    """Plain, accumulate onto a seeded destination, LeakyReLU(0.2), and both. Without the accumulate the destination starts as NaN: a K
    split without its clear, or any pixel or channel left unwritten, stays NaN. With a slope, elements whose fp64 pre-activation lies
    within the forward bar (times max|ref|) of zero are left out of the comparison (at most 0.1 % of them: tests/test_conv_same_host.py)."""
    geo = R.TABLES[table][i]
    bar = R.BARS[prec][0]
    for accumulate, slope in ((0, 0.0), (1, 0.0), (0, R.SLOPE), (1, R.SLOPE)):
        t, ref = R.case(table, i, acc=bool(accumulate), slope=slope)
        x, w, b = _nhwc(t["x"]), t["w"].cuda(), t["b"].cuda()
        y = torch.empty(geo[0], geo[5], geo[6], geo[2], device="cuda")
        if accumulate:
            y.copy_(_nhwc(t["acc0"]))
        else:
            y.fill_(float("nan"))
        lib.ok(lib.fwd_ex(geo, prec, x, w, b, y, accumulate, slope), f"fwd_ex accumulate={accumulate} slope={slope}")
        got = _nchw(y)
        assert not bool(torch.isnan(got).any()), (accumulate, slope, int(torch.isnan(got).sum()))
        name = f"y.acc{accumulate}.slope{slope}"
        if slope == 0.0:
            _hold(parity_log, name, got, ref["y"], bar)
        else:
            keep = R.off_kink(ref, bar)
            assert 1.0 - float(keep.double().mean()) <= R.KINK_SHARE
            _hold(parity_log, name, got[keep], ref["y"][keep], bar)


# ---- the K split ----------------------------------------------------------------------------------------------------------------------
KSPLIT = [("KSPLIT_FWD", i, p) for i in range(len(R.KSPLIT_FWD)) for p in PRECS] + [("KSPLIT_BWD", i, p) for i in range(len(R.KSPLIT_BWD)) for p in PRECS]


@pytest.mark.parametrize("table,i,prec", KSPLIT, ids=_ids(KSPLIT))
def test_k_split_and_single_pass_agree_and_meet_fp64(lib, parity_log, table, i, prec):
    """Once with the K split allowed (vpx_set_deterministic(0): a clear of the destination, atomic partial sums, the bias from the first
    split only) and twice without (1): all three meet fp64, the two single-pass runs are equal bit for bit, split and single pass differ in
    fp32 summation order only."""
    geo = R.TABLES[table][i]
    N, Ci, Co, kh, kw, H, W = geo
    t, ref = R.case(table, i)
    x, w, b, gy = _nhwc(t["x"]), t["w"].cuda(), t["b"].cuda(), _nhwc(t["gy"])
    fwd, grad = R.BARS[prec]
    runs = []
    prev = lib.L.vpx_set_deterministic(0)
    try:
        for det in (0, 1, 1):
            lib.L.vpx_set_deterministic(det)
            if table == "KSPLIT_FWD":
                y = _filled((N, H, W, Co), float("nan"))
                lib.ok(lib.fwd_ex(geo, prec, x, w, b, y), f"fwd_ex det={det}")
                runs.append(y)
                _hold(parity_log, f"y.det{det}.{len(runs)}", _nchw(y), ref["y"], fwd)
            else:
                dx, dw, db = _filled((N, H, W, Ci), float("nan")), _filled((Co, Ci, kh, kw), float("nan")), _filled((Co,), float("nan"))
                lib.ok(lib.bwd(geo, prec, x, w, gy, dx, dw, db), f"bwd det={det}")
                runs.append(dx)
                _hold(parity_log, f"dx.det{det}.{len(runs)}", _nchw(dx), ref["dx"], grad)
                _hold(parity_log, f"dw.det{det}.{len(runs)}", dw, ref["dw"], grad)
                _hold(parity_log, f"db.det{det}.{len(runs)}", db, ref["db"], grad)
    finally:
        lib.L.vpx_set_deterministic(prev)
    assert torch.equal(runs[1], runs[2])
    e = _relmax(runs[0], runs[1])
    print(f"  split vs single pass: {e:.3e}")
    assert e <= R.SAME_PRODUCTS, e


# ---- the weight gradient's slices -----------------------------------------------------------------------------------------------------
SLICES = [("SLICES", i, p) for i in range(len(R.SLICES)) for p in PRECS]


@pytest.mark.parametrize("table,i,prec", SLICES, ids=_ids(SLICES))
def test_weight_gradient_slices_and_ragged_tiles_vs_fp64(lib, parity_log, table, i, prec):
    """Both sides of wgrad_slices_for and ragged 64-row / 64-channel tiles; dw and db are equal bit for bit between two runs in every
    mode: slabs and column sums add in a fixed order."""
    geo = R.TABLES[table][i]
    N, Ci, Co, kh, kw, H, W = geo
    t, ref = R.case(table, i)
    x, w, gy = _nhwc(t["x"]), t["w"].cuda(), _nhwc(t["gy"])
    grad = R.BARS[prec][1]
    runs = []
    for n in (1, 2):
        dw, db = _filled((Co, Ci, kh, kw), float("nan")), _filled((Co,), float("nan"))
        lib.ok(lib.bwd(geo, prec, x, w, gy, None, dw, db), "bwd (dw, db)")
        _hold(parity_log, f"dw.run{n}", dw, ref["dw"], grad)
        _hold(parity_log, f"db.run{n}", db, ref["db"], grad)
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- gradient subsets -----------------------------------------------------------------------------------------------------------------
SUBSET_CASES = [("KERNELS", 4), ("KSPLIT_BWD", 0)]


@pytest.mark.parametrize("table,i", SUBSET_CASES, ids=_ids(SUBSET_CASES))
def test_gradient_subsets(lib, parity_log, table, i):
    """vpx_conv2d_nhwc_bwd with every subset of (dx, dw, db): what is asked for equals the all-outputs call bit for bit (single-pass
    mode for dx), what is passed as NULL — its slot lies between the others in one buffer — keeps its sentinel, as do the gaps."""
    geo = R.TABLES[table][i]
    N, Ci, Co, kh, kw, H, W = geo
    t, ref = R.case(table, i)
    x, w, gy = _nhwc(t["x"]), t["w"].cuda(), _nhwc(t["gy"])
    sizes = {"dx": N * H * W * Ci, "dw": Co * Ci * kh * kw, "db": Co}
    off, pos = {}, 64
    for k in ("dx", "dw", "db"):
        off[k] = pos
        pos += (sizes[k] + 63) // 64 * 64 + 64
    prev = lib.L.vpx_set_deterministic(1)
    try:
        results = {}
        for mask in (7, 6, 5, 3, 1, 2, 4):
            want = {k: bool(mask >> n & 1) for n, k in enumerate(("dx", "dw", "db"))}
            buf = _filled((pos,), SENTINEL)
            seg = {k: buf[off[k]:off[k] + sizes[k]] for k in sizes}
            lib.ok(lib.bwd(geo, "f32", x, w, gy, *[seg[k] if want[k] else None for k in ("dx", "dw", "db")]), f"bwd {want}")
            untouched = torch.ones(pos, dtype=torch.bool, device="cuda")
            for k in sizes:
                if want[k]:
                    untouched[off[k]:off[k] + sizes[k]] = False
            assert bool((buf[untouched] == SENTINEL).all()), want
            for k in sizes:
                if want[k]:
                    if mask == 7:
                        results[k] = seg[k].clone()
                    else:
                        assert torch.equal(seg[k], results[k]), (want, k)
        grad = R.BARS["f32"][1]
        _hold(parity_log, "dx", _nchw(results["dx"].view(N, H, W, Ci)), ref["dx"], grad)
        _hold(parity_log, "dw", results["dw"].view(Co, Ci, kh, kw), ref["dw"], grad)
        _hold(parity_log, "db", results["db"], ref["db"], grad)
    finally:
        lib.L.vpx_set_deterministic(prev)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(lib, parity_log):
    """The refusals of tests/test_conv_same_host.py on real buffers: the documented code, a message, every destination as it was, and the
    next valid call succeeds."""
    E_ARG, E_WS, E_UNSUPPORTED = -1, -2, -4
    table, i = "CHANNELS", 3
    geo = R.TABLES[table][i]
    N, Ci, Co, kh, kw, H, W = geo
    t, ref = R.case(table, i)
    x, gy = _nhwc(t["x"]), _nhwc(t["gy"])
    w = torch.randn(Co * Ci * 81, device="cuda")                       # room for every kernel size named below
    y, dx, dw, db = (_filled(s, SENTINEL) for s in ((N, H, W, Co), (N, H, W, Ci), (Co * Ci * 81,), (Co,)))

    def refused(rc, code, what):
        msg = lib.L.vpx_last_error().decode()
        assert rc == code and msg, (what, rc, msg)
        for d in (y, dx, dw, db):
            assert bool((d == SENTINEL).all()), what

    def all_three(g, prec, code, what, x=x, w=w, y=y, dy=gy, **kw):
        refused(lib.fwd_ex(g, prec, x, w, None, y, fn="fwd", **kw), code, what + " fwd")
        refused(lib.fwd_ex(g, prec, x, w, None, y, **kw), code, what + " fwd_ex")
        refused(lib.bwd(g, prec, x, w, dy, dx, dw, db, **kw), code, what + " bwd")

    for k2 in ((2, 2), (3, 4), (9, 9)):
        all_three((N, Ci, Co) + k2 + (H, W), "f32", E_ARG, f"kernel {k2}")
    refused(lib.fwd_ex(geo, "f32", x, w, None, y, 0, -0.1), E_ARG, "negative slope")
    all_three(geo, 3, E_UNSUPPORTED, "precision 3")
    all_three(geo, "f32", E_ARG, "NULL x", x=None)
    all_three(geo, "f32", E_ARG, "NULL w", w=None)
    all_three(geo, "f32", E_ARG, "NULL y / dy", y=None, dy=None)
    all_three(geo, "f32", E_WS, "workspace one byte short", ws_short=1)
    wide = (1, 2049, 8, 1, 1, 1, 1)                                     # more channel stages than a plan holds
    assert lib.L.vpx_conv2d_workspace_bytes(2049, 8, 1, 1) == 0
    xw, ww = torch.randn(1, 1, 1, 2049, device="cuda"), torch.randn(8, 2049, 1, 1, device="cuda")
    for fn in ("fwd", "fwd_ex"):
        refused(lib.fwd_ex(wide, "f32", xw, ww, None, y, fn=fn), E_UNSUPPORTED, "2049 channels " + fn)
        assert "too many channel stages" in lib.L.vpx_last_error().decode()
    # the next valid call
    w, b = t["w"].cuda(), t["b"].cuda()
    lib.ok(lib.fwd_ex(geo, "f32", x, w, b, y), "fwd_ex after the refusals")
    _hold(parity_log, "y", _nchw(y), ref["y"], R.BARS["f32"][0])
    dwv = dw[:Co * Ci * kh * kw].view(Co, Ci, kh, kw)
    lib.ok(lib.bwd(geo, "f32", x, w, gy, dx, dwv, db), "bwd after the refusals")
    _hold(parity_log, "dx", _nchw(dx), ref["dx"], R.BARS["f32"][1])
    _hold(parity_log, "dw", dwv, ref["dw"], R.BARS["f32"][1])
    _hold(parity_log, "db", db, ref["db"], R.BARS["f32"][1])
    assert bool((dw[Co * Ci * kh * kw:] == SENTINEL).all())
