"""The launch chains of vpx_convlstm_seq_fwd (VPX_OPT_SEQ_CHAINS) on the CPU, in a dry run: the option itself, the rule that decides the
number of chains (vpx_convlstm_seq_chains), the sizes the option must not move, and the two chains' host-side work (plans, pointer
offsets, carve checks) through the entry point. Whether a capturing stream takes the single chain needs a stream that captures:
tests/test_gpu_convlstm_chains.py."""
import contextlib
import ctypes

import pytest

OK = 0
# (Cin, Ch, H, W, B, T, flags) with OPT_CELL2 = 2: the q-form cell (NO_C3) / the C3 route, a saving forward, the benchmark's three block shapes
SHAPES = [(16, 32, 16, 16, 2, 1, 0), (16, 32, 32, 16, 3, 3, 0), (16, 32, 32, 16, 5, 3, 1), (64, 64, 64, 64, 128, 10, 0), (96, 96, 32, 32, 128, 10, 0),
          (96, 96, 16, 16, 128, 10, 0), (64, 64, 64, 64, 128, 10, 1)]


def _desc(_lib, Cin, Ch, H, W, B, T, flags):
    return _lib.ConvLSTMDesc(B, T, Cin, Ch, H, W, 3, 3, _lib.GATE_IFGO, _lib.LAYOUT_NHWC, _lib.PREC_BF16X3, flags)


@contextlib.contextmanager
def _dry(_lib, chains, exp=0):
    value = {1: 0, 2: 2}[chains]   # 0: one chain; 2: two from B = 2 on
    with _lib.option(_lib.OPT_DRY_RUN, 1), _lib.option(_lib.OPT_CELL2, 2), _lib.experiment(exp), _lib.option(_lib.OPT_SEQ_CHAINS, value):
        yield


def test_option_is_stored_clamped_and_restored(vpx):
    _lib = vpx._lib
    L = _lib.lib()
    default = L.vpx_set_option(_lib.OPT_SEQ_CHAINS, 0)
    assert default == 1                                       # two chains from the batch floor on
    assert L.vpx_set_option(_lib.OPT_SEQ_CHAINS, 7) == 0      # beyond the table: 2
    assert L.vpx_set_option(_lib.OPT_SEQ_CHAINS, -3) == 2     # below it: 0
    assert L.vpx_set_option(_lib.OPT_SEQ_CHAINS, default) == 0
    with _lib.option(_lib.OPT_SEQ_CHAINS, 2) as prev:
        assert prev == default
    assert L.vpx_set_option(_lib.OPT_SEQ_CHAINS, default) == default


@pytest.mark.parametrize("shape", SHAPES)
def test_sizes_do_not_depend_on_the_chains(vpx, shape):
    """vpx_convlstm_workspace_bytes / vpx_convlstm_reserve_bytes and the plan of the call: the same on one chain and on two."""
    _lib = vpx._lib
    L, d = _lib.lib(), _desc(_lib, *shape)
    seen = []
    for chains in (1, 2):
        for exp in (0, _lib.Exp.NO_C3):
            with _dry(_lib, chains, exp):
                info = _lib.ConvLSTMPlanInfo()
                assert L.vpx_convlstm_plan(ctypes.byref(d), 1, 0, 0, ctypes.byref(info)) == OK
                seen.append((exp, L.vpx_convlstm_workspace_bytes(ctypes.byref(d)), L.vpx_convlstm_reserve_bytes(ctypes.byref(d)),
                             tuple(getattr(info, n) for n, _ in _lib.ConvLSTMPlanInfo._fields_)))
    assert seen[0][1] > 0 and seen[:2] == seen[2:], seen


def test_the_chain_rule(vpx):
    """Option 2: two chains on CELL2 and C3 from B = 2 on; option 1, the default: from B = 8 on; one chain for B = 1, off those routes, and
    under option 0."""
    _lib = vpx._lib
    L = _lib.lib()

    def chains(shape, opt, exp=0, cell2=2, x_present=1):
        d = _desc(_lib, *shape)
        with _lib.option(_lib.OPT_DRY_RUN, 1), _lib.option(_lib.OPT_CELL2, cell2), _lib.experiment(exp), _lib.option(_lib.OPT_SEQ_CHAINS, opt):
            info = _lib.ConvLSTMPlanInfo()
            assert L.vpx_convlstm_plan(ctypes.byref(d), x_present, 0, 0, ctypes.byref(info)) == OK
            return info.route, L.vpx_convlstm_seq_chains(ctypes.byref(d), x_present, None)
    small = (16, 32, 32, 16, 3, 3, 0)
    assert chains(small, 2) == (_lib.CL_ROUTE_C3, 2) and chains(small, 0) == (_lib.CL_ROUTE_C3, 1) and chains(small, 1) == (_lib.CL_ROUTE_C3, 1)
    assert chains(small, 2, _lib.Exp.NO_C3) == (_lib.CL_ROUTE_CELL2, 2) and chains(small, 0, _lib.Exp.NO_C3) == (_lib.CL_ROUTE_CELL2, 1)
    assert chains(small, 2, x_present=0) == (_lib.CL_ROUTE_C3, 2)
    assert chains((16, 32, 32, 16, 1, 3, 0), 2, _lib.Exp.NO_C3) == (_lib.CL_ROUTE_CELL2, 1)          # one sample
    assert chains((16, 32, 32, 16, 2, 3, 1), 2) == (_lib.CL_ROUTE_CELL2, 2)                          # a saving forward (never on C3)
    for shape in SHAPES[3:]:                                                                       # the benchmark's blocks, as they select themselves
        assert chains(shape, 1, cell2=1) == (_lib.CL_ROUTE_CELL2, 2) and chains(shape, 0, cell2=1) == (_lib.CL_ROUTE_CELL2, 1), shape
    for B, n in ((7, 1), (8, 2)):                                                                  # the default's batch floor
        assert chains((64, 64, 64, 64, B, 10, 0), 1, cell2=1)[1] == n and chains((64, 64, 64, 64, B, 10, 0), 2, cell2=1)[1] == 2, B
    route, n = chains((16, 32, 16, 16, 4, 3, 0), 2, cell2=1)                                         # a small grid: the first generation or cell3
    assert route not in (_lib.CL_ROUTE_CELL2, _lib.CL_ROUTE_C3) and n == 1
    bad = _desc(_lib, 16, 32, 16, 16, 0, 3, 0)
    assert L.vpx_convlstm_seq_chains(ctypes.byref(bad), 1, None) == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("exp", ["0", "NO_C3"])
def test_dry_run_of_the_two_chains(vpx, shape, exp):
    """The entry point's host-side work on two chains (and on one) inside a workspace of exactly the queried size: no carve, bounds or
    argument check objects, with and without x / initial state."""
    _lib = vpx._lib
    L, d = _lib.lib(), _desc(_lib, *shape)
    fake = lambda: ctypes.c_void_p(1 << 20)   # a dry run touches no pointer
    for chains in (2, 1):
        with _dry(_lib, chains, _lib.exp_bits(exp)):
            nb, rs = L.vpx_convlstm_workspace_bytes(ctypes.byref(d)), L.vpx_convlstm_reserve_bytes(ctypes.byref(d))
            for x, h0 in ((fake(), fake()), (None, fake()), (fake(), None)):
                rc = L.vpx_convlstm_seq_fwd(ctypes.byref(d), x, h0, h0, fake(), fake(), fake(), fake(), fake(), fake(), fake(), fake(),
                                            fake() if rs else None, rs, fake(), nb, None)
                assert rc == OK, (chains, L.vpx_last_error())
