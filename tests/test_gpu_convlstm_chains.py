"""vpx_convlstm_seq_fwd with the batch as two launch chains (vpx_set_option(VPX_OPT_SEQ_CHAINS, 2): samples [0, (B + 1) / 2) on the caller's
stream, the rest on the library's side stream, from B = 2 on) against the single chain (value 0), through the raw C ABI on NHWC buffers.

What is asserted. Each chain launches the kernel chosen for the whole call on its own samples, so every output must be the single chain's
BIT FOR BIT: out, hT, cT, the split-format output under VPX_FLAG_OUT_SPLIT, and the whole reserve of a saving forward (compared as
integers: the split format holds bf16 pairs, whose bit patterns need not be numbers). The two-chain result is also held to the float64
reference of tests/convlstm_ref.py (`ref_seq`, the CPU restatement of the reference module) at the bar of the existing route tests,
convlstm_ref.BARS["bf16x3"][0] = 6e-5 in max|d| / max|ref|. Before it runs, a case asserts through vpx_convlstm_plan and
vpx_convlstm_seq_chains that it is on the route it names and that the library would run two chains there.

Shapes (Cin, Ch, H, W) = (16, 32, 16, 16) and (16, 32, 32, 16), bf16x3: one and two 16x16 half tiles per image, one 32-channel N tile.
VPX_OPT_CELL2 = 2 puts them on the second-generation cell, where the small grid selects the C3 route by itself; VPX_EXP_NO_C3 keeps the
q-form half-tile kernel (CELL2). B = 2, 3, 5: an even split, an odd one (2 + 1: a one-sample chain) and 3 + 2; T = 1 and 3 (T = 1: no
step reads a chain's own h_t). Inputs are drawn once per shape and never written; the float64 reference is computed once per operand set."""
import contextlib
import ctypes
import functools

import pytest
import torch

import convlstm_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {"16x16": (16, 32, 16, 16), "32x16": (16, 32, 32, 16)}
ROUTES = ("cell2", "c3")
BAR = R.BARS["bf16x3"][0]
# operand sets: x, s = (h0, c0), p = peepholes, b = bias; then the flags of the call
SETS = {"full": "xspb", "no_x": "spb", "no_state": "xpb", "no_peepholes": "xsb", "bare": "x"}


@functools.lru_cache(maxsize=None)
def _inputs(shape, B, T):
    Cin, Ch, H, W = SHAPES[shape]
    return R._inputs((Cin, Ch, H, W, 3, B, T))


@functools.lru_cache(maxsize=None)
def _reference(shape, B, T, ops):
    """out, hT, cT of the operand set in float64 on the CPU."""
    Cin, Ch, H, W = SHAPES[shape]
    t = {n: v.double() for n, v in _inputs(shape, B, T).items()}
    has = R.present(ops)
    out, hT, cT = R.ref_seq((Cin, Ch, H, W, 3, B, T), 0)(*(t[n] if n in has else None for n in R.LEAVES))
    return {"out": out, "hT": hT, "cT": cT}


@contextlib.contextmanager
def _route(vpx, route, chains):
    _lib = vpx._lib
    value = {1: 0, 2: 2}[chains]   # 0: never; 2: from B = 2 on (the default, 1, starts at the batch floor)
    with _lib.option(_lib.OPT_CELL2, 2), _lib.experiment(_lib.Exp.NO_C3 if route == "cell2" else 0), _lib.option(_lib.OPT_SEQ_CHAINS, value):
        yield


def _desc(vpx, shape, B, T, flags=0):
    Cin, Ch, H, W = SHAPES[shape]
    return vpx._lib.ConvLSTMDesc(B, T, Cin, Ch, H, W, 3, 3, vpx._lib.GATE_IFGO, vpx._lib.LAYOUT_NHWC, vpx.ops.PRECISIONS["bf16x3"], flags)


class _Call:
    """The device buffers of one call (allocated on the current stream) and the call itself."""

    def __init__(self, vpx, shape, B, T, ops="xspb", flags=0, h0=None, c0=None):
        _lib, o = vpx._lib, vpx.ops
        Cin, Ch, H, W = SHAPES[shape]
        self.vpx, self.shape, self.B, self.T, self.flags = vpx, shape, B, T, flags
        has = R.present(ops)
        t = _inputs(shape, B, T)
        self.op = {n: ((o.to_channels_last(t[n].cuda()) if t[n].dim() >= 4 and n != "W" else t[n].cuda().contiguous()) if n in has else None)
                   for n in R.LEAVES}
        if h0 is not None:
            self.op["h0"], self.op["c0"] = h0, c0
        self.x_present = self.op["x"] is not None
        if flags & _lib.FLAG_X_SPLIT:   # the sequence as its producer would hand it over: [B][T][HW][Cin] in operand format
            self.op["x"] = o.split_convert(self.op["x"].reshape(B * T, Cin, H, W))[0]
        d = self.desc = _desc(vpx, shape, B, T, flags)
        L = _lib.lib()
        self.nb, self.rs = L.vpx_convlstm_workspace_bytes(ctypes.byref(d)), L.vpx_convlstm_reserve_bytes(ctypes.byref(d))
        assert self.nb > 0, L.vpx_last_error()
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device="cuda")
        self.res = torch.zeros(self.rs, dtype=torch.uint8, device="cuda") if self.rs else None   # (zeros: the slots' alignment gaps are compared too)
        if flags & _lib.FLAG_OUT_SPLIT:
            self.out = torch.zeros(B * T * H * W * Ch, dtype=torch.float32, device="cuda")
        else:
            self.out = o.new_channels_last((B, T, Ch, H, W), "cuda").zero_()
        self.hT, self.cT = (o.new_channels_last((B, Ch, H, W), "cuda").zero_() for _ in range(2))

    def plan(self):
        L, info = self.vpx._lib.lib(), self.vpx._lib.ConvLSTMPlanInfo()
        assert L.vpx_convlstm_plan(ctypes.byref(self.desc), int(self.x_present), 0, 0, ctypes.byref(info)) == 0, L.vpx_last_error()
        return info.route, info.qform

    def chains(self):
        return self.vpx._lib.lib().vpx_convlstm_seq_chains(ctypes.byref(self.desc), int(self.x_present), self.vpx.ops.stream())

    def run(self):
        L, p = self.vpx._lib.lib(), self.vpx._lib.ptr
        rc = L.vpx_convlstm_seq_fwd(ctypes.byref(self.desc), *[p(self.op[n]) for n in R.LEAVES], p(self.out), p(self.hT), p(self.cT), p(self.res), self.rs,
                                    p(self.ws), self.nb, self.vpx.ops.stream())
        assert rc == 0, L.vpx_last_error()
        return self

    def results(self):
        """name -> CPU tensor; bit-compared, so everything that may hold operand-format data goes as integers."""
        torch.cuda.synchronize()
        as_bits = bool(self.flags & self.vpx._lib.FLAG_OUT_SPLIT)
        got = {"out": (self.out.view(torch.int32) if as_bits else self.out).cpu(), "hT": self.hT.cpu(), "cT": self.cT.cpu()}
        if self.res is not None:
            got["reserve"] = self.res.cpu()
        return got


def _on_route(vpx, call, route):
    _lib = vpx._lib
    want = (_lib.CL_ROUTE_CELL2, 1) if route == "cell2" else (_lib.CL_ROUTE_C3, 1)
    assert call.plan() == want, (route, call.plan())


def _both(vpx, shape, B, T, route, ops="xspb", flags=0):
    """The call on one chain and on two: (single, double) result dicts, after the route and chain-count assertions."""
    with _route(vpx, route, 1):
        c1 = _Call(vpx, shape, B, T, ops, flags)
        _on_route(vpx, c1, route)
        assert c1.chains() == 1
        single = c1.run().results()
    with _route(vpx, route, 2):
        c2 = _Call(vpx, shape, B, T, ops, flags)
        _on_route(vpx, c2, route)
        assert c2.chains() == 2, "the library would not run two chains here"
        double = c2.run().results()
    return single, double


def _assert_same_bits(single, double, tag):
    assert set(single) == set(double)
    differ = [k for k in single if not torch.equal(single[k], double[k])]
    assert not differ, (tag, "two chains differ from the single chain in", differ)


def _assert_fp64(got, shape, B, T, ops, tag, names=("out", "hT", "cT")):
    ref = _reference(shape, B, T, ops)
    errs = {k: R.relmax(got[k], ref[k]) for k in names}
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bar {BAR:.0e})")
    bad = {k: v for k, v in errs.items() if not v < BAR}
    assert not bad, (tag, bad, BAR)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_chains_equal_the_single_chain(vpx, shape, route, B, T):
    single, double = _both(vpx, shape, B, T, route)
    tag = f"chains.{shape}.{route}.B{B}.T{T}"
    _assert_same_bits(single, double, tag)
    _assert_fp64(double, shape, B, T, "xspb", tag)


@pytest.mark.parametrize("ops", [k for k in SETS if k != "full"])
@pytest.mark.parametrize("route", ROUTES)
def test_operand_sets(vpx, route, ops):
    """Without an input tensor (the forecaster's first block: every step runs on the h-only pack), without an initial state (step 0 runs
    on the other pack), without peepholes, with nothing but x and W: B = 3 (2 + 1), T = 3, the two-tile shape."""
    single, double = _both(vpx, "32x16", 3, 3, route, SETS[ops])
    tag = f"chains.32x16.{route}.{ops}"
    _assert_same_bits(single, double, tag)
    _assert_fp64(double, "32x16", 3, 3, SETS[ops], tag)


@pytest.mark.parametrize("flags", ["x_split", "out_split", "x_split_out_split"])
@pytest.mark.parametrize("route", ROUTES)
def test_split_hand_over(vpx, route, flags):
    """The sequence taken and handed on in operand format, as the model's stages do: `out` [B][T][HW][Ch] then holds bf16 pairs (and is
    where step t + 1 reads h_t: the chains' strides through it), h_T still comes out in fp32."""
    _lib = vpx._lib
    f = (_lib.FLAG_X_SPLIT if "x_split" in flags else 0) | (_lib.FLAG_OUT_SPLIT if "out_split" in flags else 0)
    single, double = _both(vpx, "32x16", 5, 3, route, "xspb", f)
    tag = f"chains.32x16.{route}.{flags}"
    _assert_same_bits(single, double, tag)
    _assert_fp64(double, "32x16", 5, 3, "xspb", tag, names=("hT", "cT") if f & _lib.FLAG_OUT_SPLIT else ("out", "hT", "cT"))


@pytest.mark.parametrize("B,T", [(2, 1), (3, 3), (5, 3)])
def test_saving_forward(vpx, B, T):
    """VPX_FLAG_SAVE_FOR_BWD (CELL2: C3 is inference only): gates, cell states and the split operands of every step land in the reserve's
    per-step planes at the chain's samples — the whole reserve must be the single chain's."""
    single, double = _both(vpx, "32x16", B, T, "cell2", "xspb", vpx._lib.FLAG_SAVE_FOR_BWD)
    assert "reserve" in double and double["reserve"].numel() > 0
    tag = f"chains.32x16.cell2.save.B{B}.T{T}"
    _assert_same_bits(single, double, tag)
    _assert_fp64(double, "32x16", B, T, "xspb", tag)


@pytest.mark.parametrize("route", ROUTES)
def test_non_default_stream(vpx, route):
    """The caller's stream is a torch side stream: chain 0 runs there, the fork and the join order chain 1 against it."""
    with _route(vpx, route, 1):
        single = _Call(vpx, "32x16", 5, 3).run().results()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with _route(vpx, route, 2), torch.cuda.stream(s):
        c = _Call(vpx, "32x16", 5, 3)
        assert c.chains() == 2
        c.run()
        follow = c.out * 2.0   # on `s`, behind the join
    double = c.results()
    _assert_same_bits(single, double, f"chains.stream.{route}")
    assert torch.equal(follow.cpu(), single["out"] * 2.0)


@pytest.mark.parametrize("route", ROUTES)
def test_back_to_back_calls_and_a_consumer(vpx, route):
    """Two calls without a synchronize in between, the second continuing from the first one's h_T, c_T (read by BOTH of its chains, so the
    second fork must lie behind the first join), then a torch op on the caller's stream that reads the second result at once. The side
    stream and the events are reused. A missing or misplaced fork / join shows as a wrong answer."""
    def two_calls(chains):
        with _route(vpx, route, chains):
            a = _Call(vpx, "32x16", 5, 3)
            b = _Call(vpx, "32x16", 5, 3, h0=a.hT, c0=a.cT)
            a.run()
            b.run()
            total = b.out.sum(dim=1) + b.cT   # consumed immediately
            got = b.results()
            got["total"], got["first"] = total.cpu(), a.out.cpu()
            return got
    single, double = two_calls(1), two_calls(2)
    _assert_same_bits(single, double, f"chains.back_to_back.{route}")
    ref = _reference("32x16", 5, 3, "xspb")
    assert R.relmax(double["first"], ref["out"]) < BAR


def test_a_capturing_stream_takes_the_single_chain(vpx):
    """While the caller's stream captures, the call runs one chain (the graph holds no stream of the library's): vpx_convlstm_seq_chains
    says so during the capture, and the replayed graph gives the single chain's bits."""
    with _route(vpx, "cell2", 2):
        eager = _Call(vpx, "32x16", 5, 3)
        assert eager.chains() == 2
        want = eager.run().results()
        c = _Call(vpx, "32x16", 5, 3)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            during = c.chains()
            c.run()
        assert during == 1
        assert c.chains() == 2   # the capture is over
        g.replay()
        got = c.results()
    _assert_same_bits(want, got, "chains.capture")


def test_one_sample_and_other_routes_stay_on_one_chain(vpx):
    _lib = vpx._lib
    with _route(vpx, "cell2", 2):
        assert _Call(vpx, "32x16", 1, 3).chains() == 1
    with _lib.option(_lib.OPT_CELL2, 2), _lib.option(_lib.OPT_SEQ_CHAINS, 1):   # the default rule: nothing below its batch floor
        assert _Call(vpx, "32x16", 5, 3).chains() == 1
    with _lib.option(_lib.OPT_SEQ_CHAINS, 2):   # B = 4 at 16x16: a small grid off the second-generation routes
        c = _Call(vpx, "16x16", 4, 3)
        assert c.plan()[0] not in (_lib.CL_ROUTE_CELL2, _lib.CL_ROUTE_C3) and c.chains() == 1
        got = c.run().results()
    _assert_fp64(got, "16x16", 4, 3, "xspb", "chains.other_route")
