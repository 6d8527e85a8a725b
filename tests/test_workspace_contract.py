"""Workspace contract of the C ABI, checked WITHOUT a GPU (VPX_OPT_DRY_RUN, include/vpx.h).

Every entry point that is handed a workspace is called with fake (never dereferenced) pointers and a workspace of EXACTLY the
size its `*_workspace_bytes` query returns. In a dry run the library does all of its host-side work — kernel selection, carving,
and the bounds check of everything it would write into the workspace (weight packs, K-slice slabs, operand conversions, partial
sums) — and issues no HIP call. A sizing rule that disagrees with the launch code returns VPX_ERR_WORKSPACE (-2) here instead of
writing past the caller's buffer on the GPU box.

Regression: round 4's intermittent abort of the GPU suite (GPUTEST_r04: SIGABRT inside the default-size `trajgru` forward).
`vpx_conv2d_workspace_bytes` sized the weight pack with the stage size of a 4-group N tile (32 channels for 5x5 taps: 25 chunks per
32 input channels) while `vpx_conv2d_nhwc_fwd_ex` packs with the stage size of the tiling it actually picks (1 group for Co <= 32:
16-channel stages, 13 chunks each = 26 per 32 channels): the flow generator's 5x5 layers (h2f_conv1 64|96 -> 32, flows_conv
32 -> 26) wrote 4-12 KB past a torch allocation. `test_trajgru_flow_generator_layers` pins exactly those layers."""
import contextlib
import ctypes
import itertools

import pytest

from vp_suite_amd import _lib
from vp_suite_amd._lib import ConvDesc, ConvLSTMDesc, STLSTMDesc

OK, E_ARG, E_WS, E_LAUNCH, E_UNSUPPORTED = 0, -1, -2, -3, -4
WS_BASE = 0x7F0000000000            # fake workspace address (256-byte aligned; never dereferenced in a dry run)
WS_BASE_ODD = WS_BASE + 0x40        # ... and one that is not 256-byte aligned (the carver rounds up; the query's slack covers it)


def _fake(i):                        # distinct fake tensor addresses far away from the workspace
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36))


@pytest.fixture(scope="module")
def L():
    lib = _lib.lib()
    with _lib.option(_lib.OPT_DRY_RUN, 1):
        yield lib
    lib.vpx_set_deterministic(0)


def _ok(L, rc, what, allow_unsupported=True):
    if rc == OK or (allow_unsupported and rc == E_UNSUPPORTED):
        return
    raise AssertionError(f"{what}: rc={rc}: {L.vpx_last_error().decode()}")


GEOS = [(1, 16, 16), (6, 64, 64), (8, 16, 16), (6, 32, 32), (128, 16, 16), (2, 67, 83), (40, 32, 32), (4, 128, 128)]


@pytest.mark.parametrize("det", [0, 1])
def test_plain_conv_entry_points(L, det):
    """vpx_conv2d_nhwc_fwd / _fwd_ex / _bwd on every (Ci, Co, k) the models produce and a grid around them."""
    L.vpx_set_deterministic(det)
    cis = [1, 3, 8, 13, 16, 26, 32, 48, 64, 96, 128, 192, 256, 288, 13 * 64, 13 * 96]
    cos = [1, 3, 16, 26, 32, 33, 64, 96, 97, 128, 192, 288, 384]
    n = 0
    for Ci, Co, k, prec in itertools.product(cis, cos, (1, 3, 5, 7), (0, 1, 2)):
        if Ci * k * k > 13 * 96 * 9:      # (outside anything the models build; keeps the sweep short)
            continue
        nb = L.vpx_conv2d_workspace_bytes(Ci, Co, k, k)
        assert nb > 0
        for (N, H, W) in GEOS[:6]:
            for base in (WS_BASE, WS_BASE_ODD):
                rc = L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), N, H, W, Ci, Co, k, k, prec, 0, 0.0,
                                              ctypes.c_void_p(base), nb, None)
                _ok(L, rc, f"fwd_ex Ci={Ci} Co={Co} k={k} prec={prec} geo={(N, H, W)}")
            rc = L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), N, H, W, Ci, Co, k, k, prec, 1, 0.2,
                                          ctypes.c_void_p(WS_BASE), nb, None)
            _ok(L, rc, f"fwd_ex(acc, leaky) Ci={Ci} Co={Co} k={k} prec={prec} geo={(N, H, W)}")
            rc = L.vpx_conv2d_nhwc_fwd(_fake(1), _fake(2), _fake(3), _fake(4), N, H, W, Ci, Co, k, k, prec, ctypes.c_void_p(WS_BASE), nb, None)
            _ok(L, rc, f"fwd Ci={Ci} Co={Co} k={k} prec={prec} geo={(N, H, W)}")
            nbw = L.vpx_conv2d_bwd_workspace_bytes(N, H, W, Ci, Co, k, k)
            rc = L.vpx_conv2d_nhwc_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), N, H, W, Ci, Co, k, k, prec,
                                       ctypes.c_void_p(WS_BASE_ODD), nbw, None)
            _ok(L, rc, f"bwd Ci={Ci} Co={Co} k={k} prec={prec} geo={(N, H, W)}")
            n += 1
    assert n > 5000


def test_trajgru_flow_generator_layers(L):
    """The layers behind GPUTEST_r04's abort (default EF-TrajGRU: traj_gru.py:108-132 with ef_traj_gru.py:31-75), every operand mode."""
    L.vpx_set_deterministic(0)
    for (C, H) in ((64, 64), (96, 32), (96, 16)):
        for (Ci, Co, k) in ((C, 32, 5), (32, 26, 5), (13 * C, 3 * C, 1), (C, 3 * C, 3)):
            for prec in (0, 1, 2):
                nb = L.vpx_conv2d_workspace_bytes(Ci, Co, k, k)
                rc = L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), 2, H, H, Ci, Co, k, k, prec, 0, 0.0,
                                              ctypes.c_void_p(WS_BASE), nb, None)
                _ok(L, rc, f"Ci={Ci} Co={Co} k={k} prec={prec}", allow_unsupported=False)


def test_undersized_workspace_is_refused_not_overrun(L):
    nb = L.vpx_conv2d_workspace_bytes(96, 32, 5, 5)
    rc = L.vpx_conv2d_nhwc_fwd_ex(_fake(1), _fake(2), _fake(3), _fake(4), 2, 32, 32, 96, 32, 5, 5, 1, 0, 0.0, ctypes.c_void_p(WS_BASE), nb - 4096, None)
    assert rc == E_WS


CLSTM_BLOCKS = [(16, 64, 64, 64), (64, 96, 32, 32), (96, 96, 16, 16), (96, 96, 32, 32), (96, 64, 64, 64), (64, 64, 64, 64),
                (16, 64, 128, 128), (64, 96, 64, 64), (3, 8, 12, 10), (3, 64, 67, 83), (4, 8, 16, 16), (8, 8, 8, 8), (12, 12, 4, 4)]


# Options of the ConvLSTM sweep, one at a time (inference calls of B <= 32, T > 1). The experiment bits change the route at these shapes:
# NO_C3 / C3_NARROW where the half-tile grid has at most 256 workgroups (B <= 8 on the 64x64 blocks), HOIST_GEN1 on the small grids,
# CELL2_FULL_TILE / CELL2X (both wave splits) where cell2_kernel_q takes the step: B = 32 on the 32x32 and 64x64 blocks whose Ch is in 32s.
E = _lib.Exp
CLSTM_EXPERIMENTS = (E.NO_C3, E.C3_NARROW, E.HOIST_GEN1, E.CELL2_FULL_TILE, E.CELL2X, E.CELL2X | E.CELL2X_COLSPLIT)
CLSTM_OPTIONS = ((None, (_lib.OPT_CELL2, 0), (_lib.OPT_CELL2, 2), (_lib.OPT_CELL3, 0), (_lib.OPT_MFMA_SHAPE, 0)) +
                 tuple((_lib.OPT_EXPERIMENT, e) for e in CLSTM_EXPERIMENTS))
# ... and with the saved-for-backward reserve as well (the tile form also decides the data gradient's launch; the x form fills the reserve)
CLSTM_OPTIONS_TRAINING = tuple((_lib.OPT_EXPERIMENT, e) for e in CLSTM_EXPERIMENTS[3:])


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_convlstm_seq(L, det, prec):
    L.vpx_set_deterministic(det)
    for (Cin, Ch, H, W), B, T, k, layout, gate in itertools.product(CLSTM_BLOCKS, (1, 2, 4, 32, 128), (1, 10), (3, 5), (0, 1), (0, 1)):
        if B * H * W > 128 * 64 * 64 or (layout == 1 and B > 4) or (k == 5 and B > 4):
            continue
        for save in (0, 1):
            for opt in CLSTM_OPTIONS:
                if opt is not None and (B > 32 or T == 1 or (save and opt not in CLSTM_OPTIONS_TRAINING)):
                    continue
                with _lib.option(*opt) if opt else contextlib.nullcontext():
                    d = ConvLSTMDesc(B, T, Cin, Ch, H, W, k, k, gate, layout, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0)
                    nb = L.vpx_convlstm_workspace_bytes(ctypes.byref(d))
                    if nb == 0:
                        continue
                    rs = L.vpx_convlstm_reserve_bytes(ctypes.byref(d))
                    tag = f"convlstm {(Cin, Ch, H, W)} B={B} T={T} k={k} layout={layout} prec={prec} save={save} opt={opt}"
                    for (x, h0) in ((_fake(1), _fake(2)), (None, _fake(2)), (_fake(1), None)):
                        rc = L.vpx_convlstm_seq_fwd(ctypes.byref(d), x, h0, None if h0 is None else _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8),
                                                    _fake(9), _fake(10), _fake(11), _fake(12), rs, ctypes.c_void_p(WS_BASE), nb, None)
                        _ok(L, rc, tag + f" fwd x={x is not None} h0={h0 is not None}")
                        if save:
                            rc = L.vpx_convlstm_seq_bwd(ctypes.byref(d), x, h0, None if h0 is None else _fake(3), _fake(4), _fake(6), _fake(7), _fake(8),
                                                        _fake(9), _fake(12), rs, _fake(13), _fake(14), _fake(15),
                                                        None if x is None else _fake(16), None if h0 is None else _fake(17), None if h0 is None else _fake(18),
                                                        _fake(19), _fake(20), _fake(21), _fake(22), _fake(23), ctypes.c_void_p(WS_BASE_ODD), nb, None)
                            _ok(L, rc, tag + f" bwd x={x is not None} h0={h0 is not None}")
                    if not save and L.vpx_convlstm_takes_split_input(ctypes.byref(d)):
                        d.flags |= _lib.FLAG_X_SPLIT
                        if L.vpx_convlstm_writes_split_output(ctypes.byref(d)):
                            d.flags |= _lib.FLAG_OUT_SPLIT
                        rc = L.vpx_convlstm_seq_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8),
                                                    _fake(9), _fake(10), _fake(11), None, 0, ctypes.c_void_p(WS_BASE), nb, None)
                        _ok(L, rc, tag + " fwd (split in/out)")


# One descriptor per route of the ConvLSTM forward (csrc/convlstm_fwd_api.hip: Route), as its dry-run launches show; inference calls with x.
# The saving variant of the same descriptor may take another route (c3 is inference only: the q form of cell2 takes the saving call).
CLSTM_ROUTES = [  # ((Cin, Ch, H, W), B, T, prec, options)
    ((16, 64, 64, 64), 4, 10, 0, ()),                                              # fused first generation (256 workgroups: not below the bar)
    ((96, 96, 16, 16), 4, 1, 0, ()),                                               # K split, T = 1: nothing to hoist
    ((96, 96, 16, 16), 4, 10, 0, ()),                                              # hoist (fp32: cell3 does not apply)
    ((96, 96, 16, 16), 4, 10, 1, ()),                                              # cell3, its projection on convq
    ((64, 96, 32, 32), 4, 10, 1, ((_lib.OPT_CELL2, 2), (_lib.OPT_MFMA_SHAPE, 0))),  # cell2 without the q form (32x32x16 MFMAs), forced onto a small grid
    ((64, 64, 64, 64), 32, 10, 1, ()),                                             # cell2, q form (1024 half-tile workgroups)
    ((64, 64, 64, 64), 4, 10, 1, ()),                                              # c3 (128 half-tile workgroups)
]


@pytest.mark.parametrize("case", CLSTM_ROUTES, ids=["fused", "ksplit", "hoist", "cell3", "cell2", "cell2q", "c3"])
def test_convlstm_routes_refuse_short_buffers_and_accept_exact_ones(L, case):
    """Every route, both directions: the sizes the queries return are accepted at an aligned and at an odd base; a workspace 256 bytes
    short, and (saving call) a reserve one byte short, are refused with VPX_ERR_WORKSPACE before anything is carved or launched."""
    (Cin, Ch, H, W), B, T, prec, options = case
    L.vpx_set_deterministic(0)

    def fwd(d, rs, base, nb):
        return L.vpx_convlstm_seq_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), _fake(8),
                                      _fake(9), _fake(10), _fake(11), _fake(12), rs, ctypes.c_void_p(base), nb, None)

    def bwd(d, rs, base, nb):
        return L.vpx_convlstm_seq_bwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), _fake(6), _fake(7), _fake(8), _fake(9), _fake(12), rs,
                                      _fake(13), _fake(14), _fake(15), _fake(16), _fake(17), _fake(18), _fake(19), _fake(20), _fake(21), _fake(22),
                                      _fake(23), ctypes.c_void_p(base), nb, None)
    with contextlib.ExitStack() as stack:
        for opt in options:
            stack.enter_context(_lib.option(*opt))
        for save in (0, 1):
            d = ConvLSTMDesc(B, T, Cin, Ch, H, W, 3, 3, 0, 0, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0)
            nb, rs = L.vpx_convlstm_workspace_bytes(ctypes.byref(d)), L.vpx_convlstm_reserve_bytes(ctypes.byref(d))
            assert nb > 256 and (rs > 0) == bool(save)
            calls = (fwd, bwd) if save else (fwd,)
            for call in calls:
                assert call(d, rs, WS_BASE, nb - 256) == E_WS, (call.__name__, save)
                if save:
                    assert call(d, rs - 1, WS_BASE, nb) == E_WS, (call.__name__, "reserve")
                for base in (WS_BASE, WS_BASE_ODD):
                    _ok(L, call(d, rs, base, nb), f"{call.__name__} save={save} base={base:#x}", allow_unsupported=False)


ST_CELLS = [(16, 128, 16, 16, 5), (128, 128, 16, 16, 5), (48, 128, 32, 32, 5), (128, 128, 32, 32, 5), (16, 16, 8, 8, 5), (3, 8, 12, 10, 3),
            (16, 64, 16, 16, 3), (64, 64, 16, 16, 5), (16, 128, 16, 16, 3)]
# (ST_LAST_FP32 changes the route wherever c5 takes the forward: k = 5, Ch in 32s, no LayerNorm)
ST_EXPERIMENTS = (0, E.ST_WGRAD_GEN1, E.ST_DGRAD_GEN1, E.ST_FWD_GEN1, E.C1_GEN1, E.C5_UNSPLIT, E.C5_NO_KSPLIT,
                  E.ST_WGRAD_GEN1 | E.ST_DGRAD_GEN1 | E.ST_FWD_GEN1 | E.C1_GEN1, E.ST_LAST_FP32, E.C5_UNSPLIT | E.ST_LAST_FP32)
DECOUPLE_EXPERIMENTS = (0, E.C1_GEN1)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_stlstm_step(L, det, prec):
    L.vpx_set_deterministic(det)
    for (Cin, Ch, H, W, k), B, ln, layout, exp in itertools.product(ST_CELLS, (1, 2, 4, 8, 16, 128, 256), (0, 1), (0, 1), ST_EXPERIMENTS):
        if (layout == 1 or ln == 1 or exp) and B > 8:
            continue
        with _lib.experiment(exp):
            for save in (0, 1):
                for packed in (0, 1):
                    d = STLSTMDesc(B, Cin, Ch, H, W, k, ln, layout, prec, (_lib.FLAG_SAVE_FOR_BWD if save else 0) | (_lib.FLAG_WEIGHTS_PACKED if packed else 0))
                    nb = L.vpx_stlstm_workspace_bytes(ctypes.byref(d))
                    if nb == 0:
                        continue
                    rs = L.vpx_stlstm_reserve_bytes(ctypes.byref(d))
                    lnarr = (ctypes.c_void_p * 8)(*[0x200000000000 + i * (1 << 30) for i in range(8)]) if ln else None
                    tag = f"stlstm {(Cin, Ch, H, W, k)} B={B} ln={ln} layout={layout} prec={prec} exp={exp} save={save} packed={packed}"
                    rc = L.vpx_stlstm_step_fwd(ctypes.byref(d), *[_fake(i) for i in range(1, 10)], lnarr, *[_fake(i) for i in range(10, 15)],
                                               _fake(15), rs, ctypes.c_void_p(WS_BASE), nb, None)
                    _ok(L, rc, tag + " fwd")
                    if save:
                        dlnarr = (ctypes.c_void_p * 8)(*[0x300000000000 + i * (1 << 30) for i in range(8)]) if ln else None
                        for (wantx, wanth) in ((1, 1), (0, 1), (1, 0)):
                            rc = L.vpx_stlstm_step_bwd(ctypes.byref(d), *[_fake(i) for i in range(1, 12)], lnarr, _fake(15), rs,
                                                       *[_fake(i) for i in range(16, 21)],
                                                       _fake(21) if wantx else None, _fake(22) if wanth else None, _fake(23), _fake(24),
                                                       *[_fake(i) for i in range(25, 30)], dlnarr, ctypes.c_void_p(WS_BASE_ODD), nb, None)
                            _ok(L, rc, tag + f" bwd dx={wantx} dh={wanth}")
                        if not ln and layout == 0 and L.vpx_stlstm_defers_wgrad(ctypes.byref(d)):
                            # deferred weight gradients: the step writes dG8 to the caller's slot; the batch call takes T*B images
                            sh = _lib.STLSTMShadows((ctypes.c_void_p * 5)(*[0x400000000000 + i * (1 << 34) for i in range(5)]), (ctypes.c_void_p * 3)(),
                                                    0x500000000000)
                            rc = L.vpx_stlstm_step_bwd_ex(ctypes.byref(d), *[_fake(i) for i in range(1, 12)], lnarr, _fake(15), rs,
                                                          *[_fake(i) for i in range(16, 21)], _fake(21), _fake(22), _fake(23), _fake(24),
                                                          None, None, None, None, None, dlnarr, ctypes.c_void_p(WS_BASE), nb, None, ctypes.byref(sh))
                            _ok(L, rc, tag + " bwd (deferred weight gradients)", allow_unsupported=False)
                            for T in (1, 19, 39):
                                dT = STLSTMDesc(T * B, Cin, Ch, H, W, k, 0, 0, prec, _lib.FLAG_SAVE_FOR_BWD)
                                nbb = L.vpx_stlstm_wgrad_batch_workspace_bytes(ctypes.byref(dT))
                                assert nbb > 0
                                rc = L.vpx_stlstm_wgrad_batch(ctypes.byref(dT), _fake(1), (ctypes.c_void_p * 5)(*[0x400000000000 + i * (1 << 34) for i in range(5)]),
                                                              *[_fake(i) for i in range(25, 30)], ctypes.c_void_p(WS_BASE_ODD), nbb, None)
                                _ok(L, rc, tag + f" wgrad_batch T={T}", allow_unsupported=False)


# One descriptor per route of the ST-LSTM step (csrc/stlstm_api.hip: STRoute, its conv_o sub-forms; csrc/stlstm_bwd_api.hip: STBwdChoice), as
# the dry-run launches show; B = 2 unless given, bf16x3 unless given.
ST_ROUTES = [  # ((Cin, Ch, H, W, k), B, layer_norm, layout, prec, experiment, deferred)
    ((8, 32, 16, 16, 5), 2, 0, 0, 1, 0, False),                                   # C5K forward (2 pixel tiles); stw + K-split c5 backward
    ((8, 32, 16, 16, 5), 2, 0, 0, 1, E.C5_UNSPLIT, False),                        # C5 forward; stw + unsplit c5 backward
    ((8, 32, 16, 16, 5), 2, 0, 0, 1, E.ST_FWD_GEN1, False),                       # GEN1, conv_o K-split + pointwise gate (4 tiles * 1 < 384)
    ((8, 128, 32, 48, 3), 8, 0, 0, 1, 0, False),                                  # GEN1, conv_o fused with the gate (96 tiles * 4 = 384)
    ((3, 8, 12, 10, 3), 2, 1, 0, 0, 0, False),                                    # LN
    ((3, 8, 12, 10, 3), 2, 1, 1, 0, 0, False),                                    # LN, reference layout (staging inside its carve)
    ((8, 32, 16, 16, 5), 2, 0, 0, 1, E.ST_DGRAD_GEN1 | E.ST_WGRAD_GEN1, False),   # first-generation backward (fp32 dG7, five weight-gradient launches)
    ((8, 32, 16, 16, 5), 2, 0, 0, 1, 0, True),                                    # deferred weight gradients (vpx_stlstm_defers_wgrad = 1)
]


@pytest.mark.parametrize("case", ST_ROUTES, ids=["c5k", "c5", "gen1_osplit", "gen1_fused", "ln", "ln_nchw", "bwd_gen1", "deferred"])
def test_stlstm_routes_refuse_short_buffers_and_accept_exact_ones(L, case):
    """Every route of the ST-LSTM step, both directions: the sizes the queries return are accepted at an aligned and at an odd base; a
    workspace 256 bytes short, and (saving call) a reserve one byte short, are refused with VPX_ERR_WORKSPACE. The queries tell the split
    routes from GEN1 / LN and C5 from C5K (asserted); which conv_o form a GEN1 descriptor takes shows in no query: that rests on the
    dry-run launch log the descriptors were picked from (`st_ln_out_kernel` after conv_o: K-split)."""
    (Cin, Ch, H, W, k), B, ln, layout, prec, exp, deferred = case
    L.vpx_set_deterministic(0)
    lnarr = (ctypes.c_void_p * 8)(*[0x200000000000 + i * (1 << 30) for i in range(8)]) if ln else None
    dlnarr = (ctypes.c_void_p * 8)(*[0x300000000000 + i * (1 << 30) for i in range(8)]) if ln else None
    sh = _lib.STLSTMShadows((ctypes.c_void_p * 5)(*[0x400000000000 + i * (1 << 34) for i in range(5)]), (ctypes.c_void_p * 3)(), 0x500000000000)

    def fwd(d, rs, base, nb):
        return L.vpx_stlstm_step_fwd(ctypes.byref(d), *[_fake(i) for i in range(1, 10)], lnarr, *[_fake(i) for i in range(10, 15)],
                                     _fake(15), rs, ctypes.c_void_p(base), nb, None)

    def bwd(d, rs, base, nb):
        dWs = [None] * 5 if deferred else [_fake(i) for i in range(25, 30)]
        return L.vpx_stlstm_step_bwd_ex(ctypes.byref(d), *[_fake(i) for i in range(1, 12)], lnarr, _fake(15), rs, *[_fake(i) for i in range(16, 21)],
                                        _fake(21), _fake(22), _fake(23), _fake(24), *dWs, dlnarr, ctypes.c_void_p(base), nb, None,
                                        ctypes.byref(sh) if deferred else None)
    with _lib.experiment(exp):
        for save in (0, 1):
            d = STLSTMDesc(B, Cin, Ch, H, W, k, ln, layout, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0)
            nb, rs = L.vpx_stlstm_workspace_bytes(ctypes.byref(d)), L.vpx_stlstm_reserve_bytes(ctypes.byref(d))
            assert nb > 256 and (rs > 0) == bool(save)
            assert not deferred or L.vpx_stlstm_defers_wgrad(ctypes.byref(d)) == 1
            # the forward's c5 routes are the ones on split operands; the first generation and LayerNorm are not
            assert L.vpx_stlstm_uses_split(ctypes.byref(d)) == int(not ln and k == 5 and not (exp & E.ST_FWD_GEN1))
            if not save and not ln and k == 5 and not (exp & ~E.C5_UNSPLIT):   # C5 against C5K: the K-split form alone carves partial sums
                with _lib.experiment(exp ^ E.C5_UNSPLIT):
                    other = L.vpx_stlstm_workspace_bytes(ctypes.byref(d))
                assert (nb < other) == bool(exp & E.C5_UNSPLIT) and nb != other
            for call in ((fwd, bwd) if save else (fwd,)):
                assert call(d, rs, WS_BASE, nb - 256) == E_WS, (call.__name__, save)
                if save:
                    assert call(d, rs - 1, WS_BASE, nb) == E_WS, (call.__name__, "reserve")
                for base in (WS_BASE, WS_BASE_ODD):
                    _ok(L, call(d, rs, base, nb), f"{call.__name__} save={save} base={base:#x}", allow_unsupported=False)


def test_decouple_tail(L):
    for det in (0, 1):
        L.vpx_set_deterministic(det)
        for (B, Ch, H, W), prec, exp in itertools.product(((1, 16, 8, 8), (2, 128, 16, 16), (8, 128, 32, 32), (128, 128, 16, 16), (2, 8, 12, 10)), (0, 1, 2), DECOUPLE_EXPERIMENTS):
            with _lib.experiment(exp):
                nb = L.vpx_decouple_workspace_bytes(B, Ch, H, W)
                rc = L.vpx_decouple_fwd(_fake(1), _fake(2), _fake(3), _fake(4), B, Ch, H, W, prec, ctypes.c_void_p(WS_BASE), nb, None)
                _ok(L, rc, f"decouple fwd {(B, Ch, H, W)} prec={prec}")
                for adjacent in (0, 1):
                    dc = _fake(1)
                    dm = ctypes.c_void_p(dc.value + B * H * W * Ch * 4) if adjacent else _fake(2)
                    gc = _fake(5)
                    gm = ctypes.c_void_p(gc.value + B * H * W * Ch * 4) if adjacent else _fake(6)
                    rc = L.vpx_decouple_bwd(dc, dm, _fake(3), _fake(4), gc, gm, _fake(7), B, Ch, H, W, prec, ctypes.c_void_p(WS_BASE_ODD), nb, None)
                    _ok(L, rc, f"decouple bwd {(B, Ch, H, W)} prec={prec} adjacent={adjacent}")


# the stage glue of EF-ConvLSTM / EF-TrajGRU (ef_conv_lstm.py:36-65, ef_traj_gru.py:37-44) and PredRNN's action / frame convolutions
GLUE = [  # (Ci, Co, k, stride, pad, transposed)
    (1, 16, 3, 1, 1, 0), (3, 16, 3, 1, 1, 0), (64, 64, 3, 2, 1, 0), (96, 96, 3, 2, 1, 0), (64, 96, 3, 2, 1, 0), (96, 96, 4, 2, 1, 1), (64, 64, 4, 2, 1, 1),
    (96, 64, 4, 2, 1, 1), (64, 16, 3, 1, 1, 1), (64, 16, 3, 1, 1, 0), (16, 16, 3, 1, 1, 0), (16, 1, 1, 1, 0, 0), (16, 3, 1, 1, 0, 0), (4, 8, 3, 2, 1, 0),
    (12, 12, 4, 2, 1, 1), (8, 4, 3, 1, 1, 1), (16, 128, 5, 1, 2, 0), (128, 16, 1, 1, 0, 0), (2, 16, 5, 2, 2, 0), (16, 16, 5, 2, 2, 1), (32, 48, 7, 2, 3, 0),
]


# CONVQ_FULL_TILE: the 3x3-halo layers convq takes; GLUE_WGRAD_TAPGROUP: bf16x3 layers with channels in 8s; GLUE_DGRAD_GEN1: layers whose
# adjoint convq takes (64 -> 64 / 96 -> 96 stride 2 and their transposes on the large batches); NO_C16: the 3x3 stride-1 layers onto 16 channels
GLUE_EXPERIMENTS = (0, E.CONVQ_FULL_TILE, E.GLUE_WGRAD_TAPGROUP, E.GLUE_DGRAD_GEN1, E.NO_C16)
# what the sweeps of this file switch on, per family of entry points (tests/test_host_logic.py holds it against the name table)
SWEPT_EXPERIMENTS = {"convlstm": CLSTM_EXPERIMENTS, "stlstm": ST_EXPERIMENTS, "decouple": DECOUPLE_EXPERIMENTS, "glue": GLUE_EXPERIMENTS}


@pytest.mark.parametrize("det", [0, 1])
def test_stage_glue(L, det):
    L.vpx_set_deterministic(det)
    for (Ci, Co, k, s, p, tr), (N, H, W), prec, slope, exp in itertools.product(GLUE, GEOS + [(1280, 16, 16), (40, 64, 64)], (0, 1, 2), (0.0, 0.2), GLUE_EXPERIMENTS):
        if N * H * W * max(Ci, Co) > 1 << 31 or (exp and prec != 1):
            continue
        with _lib.experiment(exp):
            d = ConvDesc(N, H, W, Ci, Co, k, k, s, p, tr, slope, prec, 0, 0)
            ho, wo = ctypes.c_int(0), ctypes.c_int(0)
            if L.vpx_conv2d_ex_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) != OK:
                continue
            tag = f"glue {(Ci, Co, k, s, p, tr)} geo={(N, H, W)} prec={prec} slope={slope} exp={exp}"
            nb = L.vpx_conv2d_ex_workspace_bytes(ctypes.byref(d))
            rc = L.vpx_conv2d_ex_fwd(ctypes.byref(d), _fake(1), _fake(2), _fake(3), _fake(4), ctypes.c_void_p(WS_BASE), nb, None)
            _ok(L, rc, tag + " fwd")
            if Co % 8 == 0:
                rc = L.vpx_conv2d_ex_fwd_split(ctypes.byref(d), _fake(1), _fake(2), _fake(3), None, _fake(5), ctypes.c_void_p(WS_BASE_ODD), nb, None)
                _ok(L, rc, tag + " fwd_split")
            if L.vpx_conv2d_ex_takes_split(ctypes.byref(d)):
                nbs = L.vpx_conv2d_ex_split_workspace_bytes(ctypes.byref(d))
                for packed in (0, 1):
                    rc = L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), _fake(1), 0, 0, 1, _fake(2), _fake(3), _fake(4), _fake(5) if Co % 8 == 0 else None, packed,
                                                        ctypes.c_void_p(WS_BASE), nbs, None)
                    _ok(L, rc, tag + f" fwd_from_split packed={packed}")
            nbb = L.vpx_conv2d_ex_bwd_workspace_bytes(ctypes.byref(d))
            if nbb:
                rc = L.vpx_conv2d_ex_bwd(ctypes.byref(d), _fake(1), _fake(2), _fake(4), _fake(6), _fake(7), _fake(8), _fake(9), ctypes.c_void_p(WS_BASE_ODD), nbb, None)
                _ok(L, rc, tag + " bwd")
                if L.vpx_conv2d_ex_bwd_uses_split(ctypes.byref(d)):   # the weight gradient on split operands, the forward's copy of x handed back
                    rc = L.vpx_conv2d_ex_bwd_ex(ctypes.byref(d), _fake(1), _fake(10), _fake(2), _fake(4), _fake(6), _fake(7), _fake(8), _fake(9),
                                                ctypes.c_void_p(WS_BASE), nbb, None)
                    _ok(L, rc, tag + " bwd_ex")
                    rc = L.vpx_conv2d_ex_bwd_ex(ctypes.byref(d), _fake(1), _fake(10), _fake(2), _fake(4), _fake(6), None, _fake(8), None,
                                                ctypes.c_void_p(WS_BASE_ODD), nbb, None)
                    _ok(L, rc, tag + " bwd_ex (dw only)")


# One descriptor per route of the stage glue (csrc/glue_fwd_api.hip: GlueRoute; csrc/glue_bwd_api.hip: glue_bwd_plan), from the tables of
# tests/glue_ref.py: (table, index, precision, what is called, takes_split, bwd_uses_split, names tests/test_glue_host.py::routes must give)
GLUE_ROUTES = [
    ("C16", 0, "bf16x3", "from_split", 2, 1, {"fwd.split.c16"}),
    ("CONVQ_FWD", 0, "bf16x3", "from_split", 2, 1, {"fwd.split.convq"}),                 # convq, plain
    ("CONVQ_FWD", 1, "bf16x3", "from_split", 2, 1, {"fwd.split.convq"}),                 # convq, phase form
    ("SPLIT", 0, "bf16x3", "from_split", 1, 1, {"fwd.split.gen1.conv.s1"}),              # first generation, one launch
    ("SPLIT", 4, "bf16x3", "from_split", 1, 1, {"fwd.split.gen1.phases"}),               # first generation, four phase launches
    ("SMALL_KIND1", 0, "bf16x3", "fwd", 0, 0, {"fwd.small1.many"}),
    ("SMALL_KIND2", 0, "bf16x3", "fwd", 0, 0, {"fwd.small2"}),
    ("SMALL_KIND3", 0, "bf16x3", "fwd", 0, 0, {"fwd.small3.many"}),
    ("FLIP", 0, "bf16x3", "fwd", 0, 0, {"fwd.gen1.flip"}),
    ("PHASES", 0, "bf16x3", "fwd", 0, 0, {"fwd.gen1.phases"}),
    ("CONVQ_BWD", 0, "bf16x3", "bwd", 1, 1, {"dx.convq.op01", "dw.wgrad2g", "colsum.v4.split_copy"}),   # convq data gradient
    ("SPLIT", 1, "bf16x3", "bwd", 1, 1, {"dx.gen1.phases", "dw.wgrad2g"}),                              # split weight gradient, gen1 data gradient
    ("SMALL_WGRAD", 0, "bf16x3", "bwd", 0, 0, {"dx.gen1.flip", "dw.small<16,1,3>"}),                    # small weight gradient
    ("PHASES", 0, "f32", "bwd", 0, 0, {"dx.gen1.conv.s2", "dw.launch_wgrad"}),                          # neither
]


@pytest.mark.parametrize("case", GLUE_ROUTES, ids=[f"{c[0]}{c[1]}-{c[2]}-{c[3]}" for c in GLUE_ROUTES])
def test_glue_routes_refuse_short_buffers_and_accept_exact_ones(L, case):
    """Every route of the stage glue: the size its query returns is accepted at an aligned and at an odd base, one byte less is refused
    with VPX_ERR_WORKSPACE — the backward also with dx, dw or db absent (its carve depends on what is wanted, its size test does not).
    The queries show the route as far as they can (vpx_conv2d_ex_takes_split, vpx_conv2d_ex_bwd_uses_split: asserted); the rest is held
    against the restatement of the routes in tests/test_glue_host.py."""
    import glue_ref as R
    import test_glue_host as GH
    table, i, prec, call, takes, uses, names = case
    c = getattr(R, table)[i] if table not in R.TABLES else R.TABLES[table][i]
    tab, idx = (table, i) if table in R.TABLES else ("SMALL", R.SMALL.index(c))
    v = R.variant(tab, idx)
    tr, N, Ci, Co, kh, kw, s, p, oph, opw, H, W = c
    L.vpx_set_deterministic(0)
    d = ConvDesc(N, H, W, Ci, Co, kh, kw, s, p, tr, v["slope"], GH.PRECS[prec], oph, opw)
    dp = ctypes.byref(d)
    assert L.vpx_conv2d_ex_takes_split(dp) == takes and L.vpx_conv2d_ex_bwd_uses_split(dp) == uses
    assert names <= GH.routes(c, prec, v, training=call == "bwd", from_split=call == "from_split"), GH.routes(c, prec, v, training=call == "bwd")

    def run(base, nb, absent=None):
        ws = ctypes.c_void_p(base)
        if call == "fwd":
            return [L.vpx_conv2d_ex_fwd(dp, _fake(1), _fake(2), _fake(3), _fake(4), ws, nb, None)]
        if call == "from_split":
            return [L.vpx_conv2d_ex_fwd_from_split(dp, _fake(8), 0, 0, 1, _fake(2), _fake(3), _fake(4), _fake(9) if Co % 8 == 0 else None, packed, ws, nb, None)
                    for packed in (0, 1)]
        g = {"dx": _fake(6), "dw": _fake(7), "db": _fake(10)}
        g[absent] = None
        return [L.vpx_conv2d_ex_bwd_ex(dp, _fake(1), x_sp, _fake(2), _fake(4), _fake(5), g["dx"], g["dw"], g["db"], ws, nb, None)
                for x_sp in ((None, _fake(8)) if uses else (None,))]
    query = {"fwd": L.vpx_conv2d_ex_workspace_bytes, "from_split": L.vpx_conv2d_ex_split_workspace_bytes, "bwd": L.vpx_conv2d_ex_bwd_workspace_bytes}[call]
    nb = query(dp)
    assert nb > 256
    for absent in ((None, "dx", "dw", "db") if call == "bwd" else (None,)):
        for base in (WS_BASE, WS_BASE_ODD):
            for rc in run(base, nb, absent):
                _ok(L, rc, f"{call} base={base:#x} absent={absent}", allow_unsupported=False)
        assert run(WS_BASE, nb - 1, absent) == [E_WS] * len(run(WS_BASE, nb, absent)), (call, absent)


def test_trajgru_sequence(L):
    """vpx_trajgru_seq_fwd / _bwd over the default EF-TrajGRU blocks (ef_traj_gru.py:31-75) and small / ragged shapes, every operand mode."""
    from vp_suite_amd._lib import TrajGRUDesc
    blocks = [(16, 64, 64, 64, 13), (64, 96, 32, 32, 13), (96, 96, 16, 16, 13), (96, 96, 32, 32, 13), (96, 64, 64, 64, 13), (4, 8, 16, 16, 3), (6, 12, 9, 11, 5)]
    # 1-wide and tiny maps (tests/test_gpu_trajgru_warp.py runs these on the GPU: here first, every launch's writes against its slot)
    narrow = [(3, 8, 1, 7, 3), (3, 8, 6, 1, 3), (3, 8, 1, 1, 3), (3, 8, 2, 2, 3)]
    for det in (0, 1):
        L.vpx_set_deterministic(det)
        for (Cin, C, H, W, nl), B, T, prec, save in itertools.chain(itertools.product(blocks, (1, 2, 8), (1, 4), (0, 1, 2), (0, 1)),
                                                                    itertools.product(narrow, (2,), (2,), (0, 1), (0, 1))):
            d = TrajGRUDesc(B, T, Cin, C, H, W, nl, 3, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0, 0.2)
            nb, rs = L.vpx_trajgru_workspace_bytes(ctypes.byref(d)), L.vpx_trajgru_reserve_bytes(ctypes.byref(d))
            assert nb > 0 and (rs > 0) == bool(save)
            params = (ctypes.c_void_p * 10)(*[0x200000000000 + i * (1 << 32) for i in range(10)])
            dparams = (ctypes.c_void_p * 10)(*[0x300000000000 + i * (1 << 32) for i in range(10)])
            tag = f"trajgru {(Cin, C, H, W, nl)} B={B} T={T} prec={prec} save={save} det={det}"
            for (x, h0) in ((_fake(1), _fake(2)), (None, _fake(2)), (_fake(1), None)):
                rc = L.vpx_trajgru_seq_fwd(ctypes.byref(d), x, h0, params, _fake(3), _fake(4), rs, ctypes.c_void_p(WS_BASE), nb, None)
                _ok(L, rc, tag + " fwd", allow_unsupported=False)
                if save:
                    rc = L.vpx_trajgru_seq_bwd(ctypes.byref(d), x, h0, params, _fake(3), _fake(4), rs, _fake(5), _fake(6), None if x is None else _fake(7),
                                               None if h0 is None else _fake(8), dparams, ctypes.c_void_p(WS_BASE_ODD), nb, None)
                    _ok(L, rc, tag + " bwd", allow_unsupported=False)
    d = TrajGRUDesc(2, 3, 4, 6, 8, 8, 3, 3, 0, 0, 0.2)   # C % 4 != 0
    assert L.vpx_trajgru_workspace_bytes(ctypes.byref(d)) == 0


def test_trajgru_refuses_short_buffers_and_accepts_exact_ones(L):
    """vpx_trajgru_seq_fwd / _bwd, every i2h kernel size, operand mode and operand form, with and without the fixed-point scatter's slot in
    use: the sizes the queries return (each direction's own carve, measured) are accepted at an aligned and at an odd base; a workspace 256
    bytes short, and (saving descriptor) a reserve one byte short, are refused with VPX_ERR_WORKSPACE. Only a saving descriptor has a reserve."""
    from vp_suite_amd._lib import TrajGRUDesc
    descs = [(3, 8, 1, 1, 3), (6, 12, 9, 11, 5), (16, 64, 64, 64, 13)]
    params = (ctypes.c_void_p * 10)(*[0x200000000000 + i * (1 << 32) for i in range(10)])
    dparams = (ctypes.c_void_p * 10)(*[0x300000000000 + i * (1 << 32) for i in range(10)])
    for det in (0, 1):
        L.vpx_set_deterministic(det)
        for (Cin, C, H, W, nl), k, B, T, prec, save in itertools.product(descs, (1, 3, 5, 7), (1, 2), (1, 4), (0, 1, 2), (0, 1)):
            d = TrajGRUDesc(B, T, Cin, C, H, W, nl, k, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0, 0.2)
            nb, rs = L.vpx_trajgru_workspace_bytes(ctypes.byref(d)), L.vpx_trajgru_reserve_bytes(ctypes.byref(d))
            assert nb > 256 and (rs > 0) == bool(save)
            for (x, h0) in ((_fake(1), _fake(2)), (None, _fake(2)), (_fake(1), None)):
                def fwd(rs_, base, nb_):
                    return L.vpx_trajgru_seq_fwd(ctypes.byref(d), x, h0, params, _fake(3), _fake(4), rs_, ctypes.c_void_p(base), nb_, None)

                def bwd(rs_, base, nb_):
                    return L.vpx_trajgru_seq_bwd(ctypes.byref(d), x, h0, params, _fake(3), _fake(4), rs_, _fake(5), _fake(6), None if x is None else _fake(7),
                                                 None if h0 is None else _fake(8), dparams, ctypes.c_void_p(base), nb_, None)
                tag = f"trajgru {(Cin, C, H, W, nl)} k={k} B={B} T={T} prec={prec} save={save} det={det} x={x is not None} h0={h0 is not None}"
                for call in ((fwd, bwd) if save else (fwd,)):
                    assert call(rs, WS_BASE, nb - 256) == E_WS, (tag, call.__name__)
                    if save:
                        assert call(rs - 1, WS_BASE, nb) == E_WS, (tag, call.__name__, "reserve")
                    for base in (WS_BASE, WS_BASE_ODD):
                        _ok(L, call(rs, base, nb), f"{tag} {call.__name__} base={base:#x}", allow_unsupported=False)


def test_acstlstm_refuses_short_buffers_and_accepts_exact_ones(L):
    """vpx_acstlstm_step_fwd / _bwd, with and without LayerNorm, every operand mode, all gradients wanted and the frozen pattern of
    `test_acstlstm_step`: the sizes the queries return (each direction's own carve, measured) are accepted at an aligned and at an odd base; a
    workspace 256 bytes short, and (saving descriptor) a reserve one byte short, are refused with VPX_ERR_WORKSPACE. Only a saving
    descriptor has a reserve. Each call is handed its own descriptor's sizes: no order between the saving and the non-saving query is
    assumed. They do differ where there is no LayerNorm — the non-saving forward takes conv_h / conv_a / mem from its workspace and pays for
    no backward, the saving one takes them from the reserve and is sized for the backward's carve; a formula that ignores the flag (as the
    hand count did) returns one number for both."""
    from vp_suite_amd._lib import ACSTLSTMDesc
    descs = [(1, 4, 7, 5, 1), (3, 6, 9, 11, 3), (12, 20, 33, 17, 7)]
    params = (ctypes.c_void_p * 12)(*[0x200000000000 + i * (1 << 32) for i in range(12)])
    L.vpx_set_deterministic(0)
    for (Cin, Ch, H, W, k), B, ln, prec in itertools.product(descs, (1, 8), (0, 1), (0, 1, 2)):
        lnp = (ctypes.c_void_p * 10)(*[0x280000000000 + i * (1 << 32) for i in range(10)]) if ln else None
        sizes = {}
        for save in (0, 1):
            d = ACSTLSTMDesc(B, Cin, Ch, H, W, k, ln, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0, 1.0)
            nb, rs = L.vpx_acstlstm_workspace_bytes(ctypes.byref(d)), L.vpx_acstlstm_reserve_bytes(ctypes.byref(d))
            assert nb > 256 and (rs > 0) == bool(save)
            sizes[save] = nb

            def fwd(rs_, base, nb_):
                return L.vpx_acstlstm_step_fwd(ctypes.byref(d), *[_fake(i) for i in range(1, 6)], params, lnp, *[_fake(i) for i in range(6, 11)], _fake(11), rs_,
                                               ctypes.c_void_p(base), nb_, None)

            def bwd(frozen):
                dparams = (ctypes.c_void_p * 12)(*[None if (frozen and i % 3 == 0) else 0x300000000000 + i * (1 << 32) for i in range(12)])
                dln = (ctypes.c_void_p * 10)(*[None if (frozen and i % 4 == 1) else 0x380000000000 + i * (1 << 32) for i in range(10)]) if ln else None
                douts = [_fake(12)] + [None if frozen else _fake(13 + i) for i in range(4)]
                dins = [None if (frozen and i in (0, 3)) else _fake(20 + i) for i in range(5)]

                def call(rs_, base, nb_):
                    return L.vpx_acstlstm_step_bwd(ctypes.byref(d), *[_fake(i) for i in range(1, 6)], params, lnp, _fake(11), rs_, *douts, *dins, dparams, dln,
                                                   ctypes.c_void_p(base), nb_, None)
                return call
            tag = f"acstlstm {(Cin, Ch, H, W, k)} B={B} ln={ln} prec={prec} save={save}"
            for name, call in ((("fwd", fwd), ("bwd", bwd(False)), ("bwd frozen", bwd(True))) if save else (("fwd", fwd),)):
                assert call(rs, WS_BASE, nb - 256) == E_WS, (tag, name)
                if save:
                    assert call(rs - 1, WS_BASE, nb) == E_WS, (tag, name, "reserve")
                for base in (WS_BASE, WS_BASE_ODD):
                    _ok(L, call(rs, base, nb), f"{tag} {name} base={base:#x}", allow_unsupported=False)
        if not ln:
            assert sizes[0] != sizes[1], (Cin, Ch, H, W, k, B, prec, sizes)


def test_acstlstm_step(L):
    """vpx_acstlstm_step_fwd / _bwd (action-conditional ST-LSTM cell, predrnn.py:86-169): with / without LayerNorm, every operand mode, odd
    map sizes, frozen parameters and unwanted data gradients."""
    from vp_suite_amd._lib import ACSTLSTMDesc
    shapes = [(4, 8, 16, 16, 3), (16, 32, 32, 32, 5), (3, 6, 9, 11, 3), (64, 64, 16, 16, 5), (1, 4, 7, 5, 1), (12, 20, 33, 17, 7)]
    for det in (0, 1):
        L.vpx_set_deterministic(det)
        for (Cin, Ch, H, W, k), B, ln, prec, save in itertools.product(shapes, (1, 2, 8), (0, 1), (0, 1, 2), (0, 1)):
            d = ACSTLSTMDesc(B, Cin, Ch, H, W, k, ln, prec, _lib.FLAG_SAVE_FOR_BWD if save else 0, 1.0)
            nb, rs = L.vpx_acstlstm_workspace_bytes(ctypes.byref(d)), L.vpx_acstlstm_reserve_bytes(ctypes.byref(d))
            assert nb > 0 and (rs > 0) == bool(save)
            params = (ctypes.c_void_p * 12)(*[0x200000000000 + i * (1 << 32) for i in range(12)])
            lnp = (ctypes.c_void_p * 10)(*[0x280000000000 + i * (1 << 32) for i in range(10)]) if ln else None
            tag = f"acstlstm {(Cin, Ch, H, W, k)} B={B} ln={ln} prec={prec} save={save} det={det}"
            for base in (WS_BASE, WS_BASE_ODD):
                rc = L.vpx_acstlstm_step_fwd(ctypes.byref(d), *[_fake(i) for i in range(1, 6)], params, lnp, *[_fake(i) for i in range(6, 11)], _fake(11), rs,
                                             ctypes.c_void_p(base), nb, None)
                _ok(L, rc, tag + " fwd", allow_unsupported=False)
            if save:
                for frozen in (False, True):
                    dparams = (ctypes.c_void_p * 12)(*[None if (frozen and i % 3 == 0) else 0x300000000000 + i * (1 << 32) for i in range(12)])
                    dln = (ctypes.c_void_p * 10)(*[None if (frozen and i % 4 == 1) else 0x380000000000 + i * (1 << 32) for i in range(10)]) if ln else None
                    douts = [_fake(12)] + [None if frozen else _fake(13 + i) for i in range(4)]
                    dins = [None if (frozen and i in (0, 3)) else _fake(20 + i) for i in range(5)]
                    rc = L.vpx_acstlstm_step_bwd(ctypes.byref(d), *[_fake(i) for i in range(1, 6)], params, lnp, _fake(11), rs, *douts, *dins, dparams, dln,
                                                 ctypes.c_void_p(WS_BASE_ODD), nb, None)
                    _ok(L, rc, tag + f" bwd frozen={frozen}", allow_unsupported=False)
                assert L.vpx_acstlstm_step_bwd(ctypes.byref(d), *[_fake(i) for i in range(1, 6)], params, lnp, _fake(11), rs, *douts, *dins, dparams, dln,
                                               ctypes.c_void_p(WS_BASE), nb - 4096, None) == E_WS
    d = ACSTLSTMDesc(2, 4, 8, 8, 8, 4, 0, 0, 0, 1.0)   # even kernel size
    assert L.vpx_acstlstm_workspace_bytes(ctypes.byref(d)) == 0


def test_small_workspaces(L):
    """LayerNorm, MSE."""
    for B in (1, 2, 8, 128):
        nb = L.vpx_layernorm_workspace_bytes(B)
        _ok(L, L.vpx_layernorm_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), B, 128 * 16 * 16, ctypes.c_void_p(WS_BASE), nb, None), "ln fwd", False)
        _ok(L, L.vpx_layernorm_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), B, 256, 128, ctypes.c_void_p(WS_BASE), nb, None), "ln bwd", False)
    nb = L.vpx_mse_loss_workspace_bytes()
    _ok(L, L.vpx_mse_loss(_fake(1), _fake(2), 128 * 10 * 64 * 64, 1280, 1.0, _fake(3), _fake(4), ctypes.c_void_p(WS_BASE), nb, None), "mse", False)


# ---- the small operators: each query measures the carve its call runs (csrc: carve_rconv_fwd, carve_merge_bwd, carve_ssim, ...) ----------
def _exact(L, what, nb, call):
    """The queried size is accepted at an aligned and at an odd base; one byte less is refused with VPX_ERR_WORKSPACE."""
    assert nb > 0, (what, L.vpx_last_error())
    for base in (WS_BASE, WS_BASE_ODD):
        _ok(L, call(ctypes.c_void_p(base), nb), f"{what} base={base:#x}", allow_unsupported=False)
    assert call(ctypes.c_void_p(WS_BASE), nb - 1) == E_WS, what


RC_PIX, RC_VEC, RC_SLAB_FLOATS = 256, 4, 4 << 20          # csrc/unet3d.hip
# (B, T, H, W, Ca, Cb, Co, kt, mode): one and two sources, kt 1 / 3 and the collapse, Co off RC_VEC, npix = 2, 127, 128, 129 (the slice
# rule's /128), more than one RC_PIX block, and weights whose size caps the slices: 37 of 40 wanted (64 -> 64, 27 taps), 1 of 2 (512 -> 256)
RCONV_DESCS = ([(1, 1, 1, npix, Ca, Cb, Co, 1, 0) for npix in (2, 127, 128, 129) for (Ca, Cb, Co) in ((3, 0, 5), (4, 6, 8))] +
               [(2, 1, 9, 15, 8, 0, 7, 1, 0), (1, 4, 9, 15, 6, 3, 10, 3, 0), (2, 4, 9, 15, 5, 0, 5, 4, 1), (1, 3, 1, 2, 4, 4, 6, 3, 1),
                (1, 5, 32, 32, 64, 0, 64, 3, 0), (1, 1, 3, 43, 256, 256, 256, 3, 0)])


def _rconv_slices(B, T, H, W, Ca, Cb, Co, kt, mode):      # the slice rule, written out: (wanted, the weight's cap)
    npix = B * (1 if mode else T) * H * W
    nel = kt * (1 if mode else 9) * Co * (Ca + Cb) + Co
    return min((npix + 127) // 128, 256), RC_SLAB_FLOATS // nel


def test_rconv_and_bn_relu(L):
    from vp_suite_amd._lib import RConvDesc
    assert [c for c in RCONV_DESCS if _rconv_slices(*c)[1] < _rconv_slices(*c)[0]] == RCONV_DESCS[-2:]
    assert any(c[6] % RC_VEC for c in RCONV_DESCS) and any(c[0] * c[1] * c[2] * c[3] > RC_PIX for c in RCONV_DESCS)
    for c in RCONV_DESCS:
        d = RConvDesc(*c)
        b = _fake(2) if c[5] else None
        for epi in (_lib.RCONV_EPI_PLAIN, _lib.RCONV_EPI_EVAL, _lib.RCONV_EPI_STATS):
            _exact(L, f"rconv fwd {c} epilogue={epi}", L.vpx_rconv_workspace_bytes(ctypes.byref(d), epi),
                   lambda ws, nb: L.vpx_rconv_fwd(ctypes.byref(d), epi, _fake(1), b, _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), 1e-5, 0.1,
                                                  _fake(8), _fake(9), ws, nb, None))
        for (da, db, dw, dbias) in ((1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
            _exact(L, f"rconv bwd {c} wanted={(da, db, dw, dbias)}", L.vpx_rconv_bwd_workspace_bytes(ctypes.byref(d)),
                   lambda ws, nb: L.vpx_rconv_bwd(ctypes.byref(d), _fake(1), b, _fake(3), _fake(4), _fake(5) if da else None,
                                                  _fake(6) if db and c[5] else None, _fake(7) if dw else None, _fake(8) if dbias else None, ws, nb, None))
    # N*H*W = 1, one below / at / one above a multiple of RC_PIX, several blocks
    for (N, H, W), C in itertools.product(((1, 1, 1), (3, 5, 17), (1, 16, 16), (1, 1, 257), (2, 2, 128), (5, 33, 31)), (1, 6, 64)):
        for (dact, dpool) in ((1, 0), (1, 1), (0, 1)):
            if dpool and (H & 1 or W & 1):
                continue
            _exact(L, f"bn_relu bwd {(N, H, W, C)} dact={dact} dpool={dpool}", L.vpx_bn_relu_bwd_workspace_bytes(N, H, W, C),
                   lambda ws, nb: L.vpx_bn_relu_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5) if dact else None, _fake(6) if dpool else None,
                                                    _fake(7), _fake(8), _fake(9), N, H, W, C, ws, nb, None))


MERGE_SHAPES = [(8, 24, 16), (24, 8, 16), (16, 16, 16), (32, 96, 64), (96, 32, 64), (64, 64, 64), (64, 160, 96), (3, 5, 7)]   # (Cs, Cp, Co)


def test_merge1x1(L):
    """Cs < Cp, Cs > Cp and Cs == Cp, on both sides of the 64-channel bar of the weight gradient's slice cap; 1x1 and 67x83 maps."""
    for (Cs, Cp, Co), (N, H, W), prec in itertools.product(MERGE_SHAPES, ((1, 1, 1), (2, 67, 83), (128, 16, 16)), (0, 1)):
        tag = f"merge1x1 {(Cs, Cp, Co)} geo={(N, H, W)} prec={prec}"
        _exact(L, tag + " fwd", L.vpx_merge1x1_workspace_bytes(Cs, Cp, Co),
               lambda ws, nb: L.vpx_merge1x1_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), N, H, W, Cs, Cp, Co, prec, ws, nb, None))
        for (da, db, dw, dbias) in ((1, 1, 1, 1), (0, 0, 1, 0), (1, 1, 0, 0), (0, 0, 0, 1)):
            _exact(L, tag + f" bwd wanted={(da, db, dw, dbias)}", L.vpx_merge1x1_bwd_workspace_bytes(N, H, W, Cs, Cp, Co),
                   lambda ws, nb: L.vpx_merge1x1_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5) if da else None, _fake(6) if db else None,
                                                     _fake(7) if dw else None, _fake(8) if dbias else None, N, H, W, Cs, Cp, Co, prec, ws, nb, None))


PM_CHUNK, SS_TAPS, SS_TH, SS_TW = 256 * 16, 11, 16, 32     # csrc/measure.hip
# the SSIM map is (H - 10) x (W - 10): one entry, one tile exactly, one entry more than a tile in either direction and in both, non-square maps
SSIM_SIZES = [(SS_TAPS, SS_TAPS), (SS_TH + 10, SS_TW + 10), (SS_TH + 11, SS_TW + 10), (SS_TH + 10, SS_TW + 11), (SS_TH + 11, SS_TW + 11),
              (SS_TAPS, 100), (75, 13), (64, 64), (67, 83)]


def test_pixel_measures_and_ssim(L):
    for n_frames, elems in itertools.product((1, 3, 40), (1, PM_CHUNK - 1, PM_CHUNK, PM_CHUNK + 1, 3 * 67 * 83)):
        _exact(L, f"pixel_measures {(n_frames, elems)}", L.vpx_pixel_measures_workspace_bytes(n_frames, elems),
               lambda ws, nb: L.vpx_pixel_measures_fwd(_fake(1), _fake(2), n_frames, elems, _fake(3), ws, nb, None))
    for n_frames, (H, W), layout in itertools.product((1, 3, 40), SSIM_SIZES, (0, 1)):
        _exact(L, f"ssim {(n_frames, H, W)} layout={layout}", L.vpx_ssim_workspace_bytes(n_frames, H, W),
               lambda ws, nb: L.vpx_ssim_fwd(_fake(1), _fake(2), n_frames, 3, H, W, layout, _fake(3), ws, nb, None))
    assert L.vpx_ssim_workspace_bytes(1, SS_TAPS - 1, 64) == 0 and L.vpx_ssim_workspace_bytes(1, 64, SS_TAPS - 1) == 0


def test_groupnorm_bwd(L):
    """With dgamma / dbeta the partial sums need the queried size; without them there is nothing to carve and a NULL workspace is accepted."""
    for (N, HW, C, G), act in itertools.product(((1, 1, 1, 1), (2, 64, 16, 4), (3, 67 * 83, 24, 3), (128, 256, 64, 16), (5, 7, 256, 1)), (0, 1)):
        def call(ws, nb, params=True):
            return L.vpx_groupnorm_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), _fake(7) if params else None,
                                       _fake(8) if params else None, N, HW, C, G, act, 0.2, ws, nb, None)
        _exact(L, f"groupnorm bwd {(N, HW, C, G)} act={act}", L.vpx_groupnorm_bwd_workspace_bytes(N, C), call)
        assert call(None, L.vpx_groupnorm_bwd_workspace_bytes(N, C)) == E_WS
        _ok(L, call(None, 0, params=False), f"groupnorm bwd {(N, HW, C, G)} without dgamma / dbeta", allow_unsupported=False)


MSE_BLOCK, MSE_MAX_BLOCKS, GS_BLOCK, GS_MAX_BLOCKS = 256 * 4, 1024, 256 * 4, 1024     # csrc/train_tail.hip: elements per block, block cap


def test_mse_and_grad_stats(L):
    """One element, the last n whose blocks are all launched, the first beyond the block cap, and far beyond it."""
    for n in (1, MSE_BLOCK * MSE_MAX_BLOCKS, MSE_BLOCK * MSE_MAX_BLOCKS + 1, 1 << 33):
        for dpred in (_fake(4), None):
            _exact(L, f"mse n={n}", L.vpx_mse_loss_workspace_bytes(),
                   lambda ws, nb: L.vpx_mse_loss(_fake(1), _fake(2), n, 1 + n % 7, 1.0, _fake(3), dpred, ws, nb, None))
    for n in (1, GS_BLOCK * GS_MAX_BLOCKS, GS_BLOCK * GS_MAX_BLOCKS + 1, 1 << 33):
        _exact(L, f"grad_stats n={n}", L.vpx_grad_stats_workspace_bytes(),
               lambda ws, nb: L.vpx_grad_stats(_fake(1), n, 1.0, _fake(2), ws, nb, None))


def test_layernorm(L):
    """One query for both directions: the larger carve (the backward's); each direction carves its own slots out of it."""
    for B, (HW, C) in itertools.product((1, 2, 63, 64, 65, 128), ((1, 1), (35, 20), (256, 128))):
        nb = L.vpx_layernorm_workspace_bytes(B)
        _exact(L, f"layernorm fwd B={B} n={HW * C}", nb,
               lambda ws, nb: L.vpx_layernorm_fwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), B, HW * C, ws, nb, None))
        _exact(L, f"layernorm bwd B={B} {(HW, C)}", nb,
               lambda ws, nb: L.vpx_layernorm_bwd(_fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6), _fake(7), B, HW, C, ws, nb, None))


HD_PIX = 64     # csrc/lpips.hip: pixels per workgroup of the head


def test_lpips_stem_and_head(L):
    for (n0, n1), (H, W) in itertools.product(((1, 0), (2, 2), (16, 16)), ((7, 7), (31, 33), (64, 64), (67, 83))):
        _exact(L, f"lpips stem fwd {(n0, n1, H, W)}", L.vpx_lpips_stem_workspace_bytes(),
               lambda ws, nb: L.vpx_lpips_stem_fwd(_fake(1), _fake(2) if n1 else None, n0, n1, H, W, _fake(3), _fake(4), _fake(5), ws, nb, None))
        _exact(L, f"lpips stem bwd {(n0, H, W)}", L.vpx_lpips_stem_workspace_bytes(),
               lambda ws, nb: L.vpx_lpips_stem_bwd(_fake(1), _fake(2), _fake(3), n0, H, W, _fake(4), ws, nb, None))
    for n, HW, C in itertools.product((1, 3, 40), (1, HD_PIX - 1, HD_PIX, HD_PIX + 1, 3 * HD_PIX - 1, 3 * HD_PIX, 3 * HD_PIX + 1, 15 * 15), (1, 64, 384)):
        _exact(L, f"lpips head {(n, HW, C)}", L.vpx_lpips_head_workspace_bytes(n, HW),
               lambda ws, nb: L.vpx_lpips_head_fwd(_fake(1), _fake(2), _fake(3), n, HW, C, _fake(4), ws, nb, None))


def test_fvd_features(L):
    """The table tests/test_fvd_host.py builds, one and two clip sets (its own dry run holds the refusals)."""
    import fvd_ref
    from vp_suite_amd import measure as M
    M.register_fvd_weights(fvd_ref.state_dict())
    try:
        trunk = M._fvd_trunk("cpu")
        table, rows, n_params = trunk["table"], trunk["n_rows"], len(trunk["params"])
        params = (ctypes.c_void_p * n_params)(*[0x200000000000 + i * (1 << 30) for i in range(n_params)])
        for (n0, n1), (T, h, w) in itertools.product(((1, 0), (3, 0), (1, 1), (2, 5)), ((9, 20, 28), (16, 64, 64), (12, 224, 224), (10, 67, 83))):
            _exact(L, f"fvd_features {(n0, n1, T, h, w)}", L.vpx_fvd_features_workspace_bytes(n0 + n1, T, 3, h, w, table, rows),
                   lambda ws, nb: L.vpx_fvd_features(_fake(1), _fake(2) if n1 else None, n0, n1, T, 3, h, w, table, rows, params, n_params, _fake(3), ws, nb, None))
    finally:
        M.clear_fvd_weights()


def test_random_shapes_fuzz():
    """tools/fuzz_contract.py: 4 000 random descriptors (odd map sizes, channel counts that are multiples of nothing, every kernel size,
    layout, operand mode and option bit) through every entry point that takes a workspace, in its own process (it switches the library
    into a dry run). Round 5: its first run found a 7x7 ConvLSTM data gradient over 4 * 288 gate channels whose 8-wave form needs 168 KB
    of LDS — refused at the launch with an 'invalid argument'; the layouts now fall back to the 4-wave form (conv_fits_lds)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for seed in (1, 2):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_contract.py"), "2000", str(seed)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
