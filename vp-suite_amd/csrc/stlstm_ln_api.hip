// stlstm_ln_api.hip — LayerNorm variant of the ST-LSTM cell (predrnn.py:24-40 + 57-83): conv_x / conv_h / conv_m /
// conv_o are each followed by LayerNorm([C,H,W]) before the gates add them, so they run as separate plain convolutions
// (same implicit-GEMM kernel), LayerNorm kernels and pointwise gate kernels. Called from vpx_stlstm_step_fwd/_bwd when
// desc.layer_norm != 0. LN parameters arrive in the reference's [C,H,W] layout and are transposed to [HW,C] per call.
#include "vpx_host.h"

namespace vpx {

struct STLN {  // sizes
    size_t n_state, n_x, HW;
    int B, Cin, Ch, H, W, k;
    size_t wpk_max;      // floats
    size_t slab_floats;
    int slices;
};

static STLN stln_sizes(const vpx_stlstm_desc* d) {
    STLN s{};
    s.B = d->B; s.Cin = d->Cin; s.Ch = d->Ch; s.H = d->H; s.W = d->W; s.k = d->k;
    s.HW = (size_t)d->H * d->W;
    s.n_state = (size_t)d->B * s.HW * d->Ch;
    s.n_x = (size_t)d->B * s.HW * d->Cin;
    const int Ch = d->Ch, Cin = d->Cin, k = d->k;
    size_t m = plain_conv_wpk_floats(Cin, 7 * Ch, k, k);
    auto mx = [&](size_t v) { if (v > m) m = v; };
    mx(plain_conv_wpk_floats(Ch, 4 * Ch, k, k)); mx(plain_conv_wpk_floats(Ch, 3 * Ch, k, k));
    mx(plain_conv_wpk_floats(2 * Ch, Ch, k, k)); mx(plain_conv_wpk_floats(2 * Ch, Ch, 1, 1));
    mx(plain_conv_wpk_floats(7 * Ch, Cin, k, k)); mx(plain_conv_wpk_floats(4 * Ch, Ch, k, k));
    mx(plain_conv_wpk_floats(3 * Ch, Ch, k, k)); mx(plain_conv_wpk_floats(Ch, 2 * Ch, k, k));
    mx(plain_conv_wpk_floats(Ch, 2 * Ch, 1, 1));
    s.wpk_max = m;
    s.slices = wgrad_slices(d->B, d->H, d->W);
    size_t w = (size_t)7 * Ch * Cin * k * k;
    if ((size_t)4 * Ch * Ch * k * k > w) w = (size_t)4 * Ch * Ch * k * k;
    if ((size_t)2 * Ch * Ch * k * k > w) w = (size_t)2 * Ch * Ch * k * k;
    s.slab_floats = w * s.slices;
    return s;
}

// The reserve of the LayerNorm variant: xhat_x(7) xhat_h(4) xhat_m(3) xhat_o(1) gates_c(3) gates_m(3) o tl mem(2) = 25 state-sized planes, then
// 4 x stats[B][2]. base == nullptr: the size alone. A descriptor that does not save has none (all null, 0 bytes).
struct LNReserve {
    float *xhat_x, *xhat_h, *xhat_m, *xhat_o, *gates_c, *gates_m, *o, *tl, *mem, *st_x, *st_h, *st_m, *st_o;
    size_t bytes;
};
static LNReserve stlstm_ln_reserve(const vpx_stlstm_desc* d, const STLN& s, const void* base) {
    LNReserve R{};
    if (!(d->flags & VPX_FLAG_SAVE_FOR_BWD)) return R;
    const size_t plane = align256(s.n_state * 4);
    auto take = [&](int planes) { float* p = base ? (float*)((char*)base + R.bytes) : nullptr; R.bytes += planes * plane; return p; };
    R.xhat_x = take(7); R.xhat_h = take(4); R.xhat_m = take(3); R.xhat_o = take(1);
    R.gates_c = take(3); R.gates_m = take(3); R.o = take(1); R.tl = take(1); R.mem = take(2);
    if (float* st = base ? (float*)((char*)base + R.bytes) : nullptr) { R.st_x = st; R.st_h = st + 2 * s.B; R.st_m = st + 4 * s.B; R.st_o = st + 6 * s.B; }
    R.bytes += align256((size_t)8 * d->B * 4) + 256;
    return R;
}
size_t stlstm_ln_reserve_bytes(const vpx_stlstm_desc* d) { return stlstm_ln_reserve(d, stln_sizes(d), nullptr).bytes; }

// ---- the workspaces: each direction's slots in the order they are taken (see CarveMeasure, vpx_host.h) ----
constexpr int LN_MULT[4] = {7, 4, 3, 1};   // channels of the LayerNorms of conv_x / conv_h / conv_m / conv_o, in units of Ch
// the 8 LN parameter tensors transposed ([C,H,W] -> [HW,C]) or their gradients; order x_g,x_b,h_g,h_b,m_g,m_b,o_g,o_b
template <class WS>
static void carve_ln_params(WS& ws, const STLN& s, float* dst[8]) {
    for (int i = 0; i < 8; ++i) dst[i] = ws.take(s.HW * LN_MULT[i / 2] * s.Ch);
}
// VPX_FLAG_WEIGHTS_PACKED (forward): the caller kept this workspace since a call with the same weights, LayerNorm parameters and desc —
// the five weight packs (one region each) and the transposed LayerNorm parameters are still in it (first carves after the staging: fixed offsets)
struct LNFwdSlots {
    STStage nchw;   // h, c, m and the five outputs
    float *wpk5[5], *lnp[8], *partial, *st_tmp, *xc, *hc, *mc, *o_pre, *oc, *lc, *mem;   // partial: doubles, taken as floats
};
template <class WS>
static void carve_ln_fwd(WS& ws, const vpx_stlstm_desc* d, const STLN& s, LNFwdSlots& w) {
    carve_st_stage(ws, d, s.n_x, s.n_state, false, 8, w.nchw);   // 3 inputs + 5 outputs listed for st_stage_in
    for (auto& p : w.wpk5) p = ws.take(s.wpk_max);
    carve_ln_params(ws, s, w.lnp);
    w.partial = ws.take((size_t)s.B * 64 * 2 * 2);
    w.st_tmp = ws.take((size_t)8 * s.B);
    w.xc = ws.take(7 * s.n_state); w.hc = ws.take(4 * s.n_state); w.mc = ws.take(3 * s.n_state);
    for (float** p : {&w.o_pre, &w.oc, &w.lc}) *p = ws.take(s.n_state);
    w.mem = ws.take(2 * s.n_state);
}
struct LNBwdSlots {
    STStage nchw;   // h, c, m and the five incoming gradients, dh, dc, dm (the last is spare)
    float *wpk, *partial, *sums, *dG7, *dlc, *du_o, *dcn, *dmn, *dm_scratch, *du_x, *du_h, *du_m, *dmem, *slabs, *lnp[8], *dlnp[8];
};
template <class WS>
static void carve_ln_bwd(WS& ws, const vpx_stlstm_desc* d, const STLN& s, LNBwdSlots& w) {
    carve_st_stage(ws, d, s.n_x, s.n_state, true, 12, w.nchw);   // 8 inputs + 3 outputs listed for st_stage_in, + the spare
    w.wpk = ws.take(s.wpk_max);
    w.partial = ws.take((size_t)s.B * 64 * 2 * 2);
    w.sums = ws.take((size_t)2 * s.B);
    w.dG7 = ws.take(7 * s.n_state);
    for (float** p : {&w.dlc, &w.du_o, &w.dcn, &w.dmn, &w.dm_scratch}) *p = ws.take(s.n_state);
    w.du_x = ws.take(7 * s.n_state); w.du_h = ws.take(4 * s.n_state); w.du_m = ws.take(3 * s.n_state);
    w.dmem = ws.take(2 * s.n_state);
    w.slabs = ws.take(s.slab_floats);
    carve_ln_params(ws, s, w.lnp);
    carve_ln_params(ws, s, w.dlnp);
}
size_t stlstm_ln_workspace_bytes(const vpx_stlstm_desc* d) {
    const STLN s = stln_sizes(d);
    CarveMeasure f, b;
    LNFwdSlots wf{}; LNBwdSlots wb{};
    carve_ln_fwd(f, d, s, wf);
    if (d->flags & VPX_FLAG_SAVE_FOR_BWD) carve_ln_bwd(b, d, s, wb);   // (only a saving call is followed by a backward)
    return f.off > b.off ? f.off : b.off;
}

// transposes the 8 LN parameter tensors ([C,H,W] -> [HW,C]) into their slots
static int ln_params_nhwc(const float* const* ln, float* const dst[8], const STLN& s, hipStream_t stream, bool cached = false) {
    for (int i = 0; i < 8; ++i) {
        if (!ln[i]) { set_error("stlstm (layer_norm): LayerNorm parameter %d is NULL", i); return VPX_ERR_ARG; }
        if (!cached) VPX_CHECK_HIP(launch_nchw_to_nhwc(ln[i], dst[i], 1, LN_MULT[i / 2] * s.Ch, s.H, s.W, stream));
    }
    return VPX_OK;
}

int stlstm_ln_fwd(const vpx_stlstm_desc* d, STFwdTensors t, void* reserve, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const STLN s = stln_sizes(d);
    const int B = s.B, Cin = s.Cin, Ch = s.Ch, k = s.k, prec = d->precision;
    const ConvGeo g{B, s.H, s.W};
    const bool save = (d->flags & VPX_FLAG_SAVE_FOR_BWD) != 0, packed = (d->flags & VPX_FLAG_WEIGHTS_PACKED) != 0;
    const LNReserve R = stlstm_ln_reserve(d, s, reserve);
    Carver ws(workspace, workspace_bytes);
    LNFwdSlots w{};
    carve_ln_fwd(ws, d, s, w);
    VPX_CHECK_CARVE(ws, "vpx_stlstm_step_fwd (LayerNorm)");
    int rc;
    if ((rc = st_stage_in(d, w.nchw, &t.x, {&t.h, &t.c, &t.m}, 3, {&t.out[0], &t.out[1], &t.out[2], &t.out[3], &t.out[4]}, nullptr, stream))) return rc;
    if ((rc = ln_params_nhwc(t.ln, w.lnp, s, stream, packed))) return rc;
    double* partial = (double*)w.partial;
    float* mem = save ? R.mem : w.mem;
    const long long n1 = (long long)s.HW * Ch;
    // conv_x / conv_h / conv_m, each followed by its own LayerNorm (predrnn.py:58-60 with :24-36)
    if ((rc = plain_conv(stream, prec, g, t.x, Cin, Cin, t.Wx, (long long)Cin * k * k, k * k, k, k, 7 * Ch, false, nullptr, w.xc, 7 * Ch, false, w.wpk5[0], 0.0f, packed))) return rc;
    VPX_CHECK_HIP(launch_layernorm_fwd(w.xc, w.lnp[0], w.lnp[1], w.xc, R.xhat_x, save ? R.st_x : w.st_tmp, partial, B, 7 * n1, stream));
    if ((rc = plain_conv(stream, prec, g, t.h, Ch, Ch, t.Wh, (long long)Ch * k * k, k * k, k, k, 4 * Ch, false, nullptr, w.hc, 4 * Ch, false, w.wpk5[1], 0.0f, packed))) return rc;
    VPX_CHECK_HIP(launch_layernorm_fwd(w.hc, w.lnp[2], w.lnp[3], w.hc, R.xhat_h, save ? R.st_h : w.st_tmp + 2 * B, partial, B, 4 * n1, stream));
    if ((rc = plain_conv(stream, prec, g, t.m, Ch, Ch, t.Wm, (long long)Ch * k * k, k * k, k, k, 3 * Ch, false, nullptr, w.mc, 3 * Ch, false, w.wpk5[2], 0.0f, packed))) return rc;
    VPX_CHECK_HIP(launch_layernorm_fwd(w.mc, w.lnp[4], w.lnp[5], w.mc, R.xhat_m, save ? R.st_m : w.st_tmp + 4 * B, partial, B, 3 * n1, stream));
    STLNGateArgs ga{};
    ga.npix = (long long)B * s.HW; ga.Ch = Ch; ga.xc = w.xc; ga.hc = w.hc; ga.mc = w.mc; ga.c = t.c; ga.m = t.m;
    ga.c_new = t.out[1]; ga.m_new = t.out[2]; ga.delta_c = t.out[3]; ga.delta_m = t.out[4]; ga.o_pre = w.o_pre; ga.mem = mem;
    ga.gates_c = R.gates_c; ga.gates_m = R.gates_m;
    VPX_CHECK_HIP(launch_st_ln_gates(ga, stream));
    // conv_o(mem) + LayerNorm, conv_last(mem)   (predrnn.py:80-81)
    if ((rc = plain_conv(stream, prec, g, mem, 2 * Ch, 2 * Ch, t.Wo, (long long)2 * Ch * k * k, k * k, k, k, Ch, false, nullptr, w.oc, Ch, false, w.wpk5[3], 0.0f, packed))) return rc;
    VPX_CHECK_HIP(launch_layernorm_fwd(w.oc, w.lnp[6], w.lnp[7], w.oc, R.xhat_o, save ? R.st_o : w.st_tmp + 6 * B, partial, B, n1, stream));
    if ((rc = plain_conv(stream, prec, g, mem, 2 * Ch, 2 * Ch, t.Wlast, (long long)2 * Ch, 1, 1, 1, Ch, false, nullptr, w.lc, Ch, false, w.wpk5[4], 0.0f, packed))) return rc;
    VPX_CHECK_HIP(launch_st_ln_out(w.o_pre, w.oc, w.lc, t.out[0], R.o, R.tl, (long long)s.n_state, stream));
    return st_stage_out(d, w.nchw, stream);
}

int stlstm_ln_bwd(const vpx_stlstm_desc* d, STBwdTensors t, const void* reserve, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const STLN s = stln_sizes(d);
    const int B = s.B, Cin = s.Cin, Ch = s.Ch, k = s.k, prec = d->precision;
    const int HW = (int)s.HW, ldG = 7 * Ch;
    const ConvGeo g{B, s.H, s.W};
    const LNReserve R = stlstm_ln_reserve(d, s, reserve);
    Carver ws(workspace, workspace_bytes);
    LNBwdSlots w{};
    carve_ln_bwd(ws, d, s, w);
    VPX_CHECK_CARVE(ws, "vpx_stlstm_step_bwd (LayerNorm)");
    int rc;
    // (the LayerNorm parameters and their gradients keep the reference's [C,H,W] layout in either layout of the activations)
    if ((rc = st_stage_in(d, w.nchw, &t.x, {&t.h, &t.c, &t.m, &t.g[0], &t.g[1], &t.g[2], &t.g[3], &t.g[4]}, 8, {&t.dh, &t.dc, &t.dm}, &t.dx, stream))) return rc;
    if ((rc = ln_params_nhwc(t.ln, w.lnp, s, stream))) return rc;
    double* partial = (double*)w.partial;
    float* dm_out = t.dm ? t.dm : w.dm_scratch;

    // A: through h_new = o * tanh(lc): d(o pre-activation) -> dG7 block 3, d conv_last
    {
        STBwdOutArgs a{(long long)s.n_state, Ch, ldG, 3 * Ch, -1, t.g[0], R.o, R.tl, w.dG7, w.dlc, 0};
        VPX_CHECK_HIP(launch_st_bwd_out(a, stream));
    }
    // B: LayerNorm of conv_o backward (dy = dG7 block 3), then grads of mem through conv_o and conv_last
    const int blk_o[8] = {3, 0, 0, 0, 0, 0, 0, 0};
    VPX_CHECK_HIP(launch_layernorm_bwd(w.dG7, ldG, Ch, blk_o, R.xhat_o, R.st_o, w.lnp[6], B, HW, Ch, partial, w.sums, w.du_o, w.dlnp[6], w.dlnp[7], stream));
    if ((rc = plain_conv(stream, prec, g, w.du_o, Ch, Ch, t.Wo, (long long)2 * Ch * k * k, k * k, k, k, 2 * Ch, true, nullptr, w.dmem, 2 * Ch, false, w.wpk))) return rc;
    if ((rc = plain_conv(stream, prec, g, w.dlc, Ch, Ch, t.Wlast, (long long)2 * Ch, 1, 1, 1, 2 * Ch, true, nullptr, w.dmem, 2 * Ch, true, w.wpk))) return rc;
    // split dmem [B,HW,2Ch] into the two state gradients the gate stage expects
    VPX_CHECK_HIP(vpx_memcpy2d_async(w.dcn, (size_t)Ch * 4, w.dmem, (size_t)2 * Ch * 4, (size_t)Ch * 4, (size_t)B * HW, hipMemcpyDeviceToDevice, stream));
    VPX_CHECK_HIP(vpx_memcpy2d_async(w.dmn, (size_t)Ch * 4, w.dmem + Ch, (size_t)2 * Ch * 4, (size_t)Ch * 4, (size_t)B * HW, hipMemcpyDeviceToDevice, stream));
    // C: gate groups -> dG7 blocks (i,f,g | o | i',f',g') w.r.t. the SUMS of normalised conv outputs
    {
        STBwdGateArgs a{};
        a.npix = (long long)B * HW; a.Ch = Ch; a.ldG = ldG;
        a.gates_c = R.gates_c; a.gates_m = R.gates_m; a.c = t.c; a.m = t.m;
        a.dcn_ext = t.g[1]; a.dmn_ext = t.g[2]; a.ddc_ext = t.g[3]; a.ddm_ext = t.g[4];
        a.dcn_conv = w.dcn; a.dmn_conv = w.dmn; a.dG7 = w.dG7; a.dc = t.dc; a.dm = dm_out;
        VPX_CHECK_HIP(launch_st_bwd_gates(a, stream));
    }
    // D: LayerNorm backward of conv_x (Wx row order i,f,g,i',f',g',o), conv_h (i,f,g,o), conv_m (i,f,g)
    const int blk_x[8] = {0, 1, 2, 4, 5, 6, 3, 0}, blk_h[8] = {0, 1, 2, 3, 0, 0, 0, 0}, blk_m[8] = {4, 5, 6, 0, 0, 0, 0, 0};
    VPX_CHECK_HIP(launch_layernorm_bwd(w.dG7, ldG, Ch, blk_x, R.xhat_x, R.st_x, w.lnp[0], B, HW, 7 * Ch, partial, w.sums, w.du_x, w.dlnp[0], w.dlnp[1], stream));
    VPX_CHECK_HIP(launch_layernorm_bwd(w.dG7, ldG, Ch, blk_h, R.xhat_h, R.st_h, w.lnp[2], B, HW, 4 * Ch, partial, w.sums, w.du_h, w.dlnp[2], w.dlnp[3], stream));
    VPX_CHECK_HIP(launch_layernorm_bwd(w.dG7, ldG, Ch, blk_m, R.xhat_m, R.st_m, w.lnp[4], B, HW, 3 * Ch, partial, w.sums, w.du_m, w.dlnp[4], w.dlnp[5], stream));
    // E: data gradients
    if (t.dx && (rc = plain_conv(stream, prec, g, w.du_x, 7 * Ch, 7 * Ch, t.Wx, (long long)Cin * k * k, k * k, k, k, Cin, true, nullptr, t.dx, Cin, false, w.wpk))) return rc;
    if (t.dh && (rc = plain_conv(stream, prec, g, w.du_h, 4 * Ch, 4 * Ch, t.Wh, (long long)Ch * k * k, k * k, k, k, Ch, true, nullptr, t.dh, Ch, false, w.wpk))) return rc;
    if (t.dm && (rc = plain_conv(stream, prec, g, w.du_m, 3 * Ch, 3 * Ch, t.Wm, (long long)Ch * k * k, k * k, k, k, Ch, true, nullptr, t.dm, Ch, true, w.wpk))) return rc;
    // F: weight gradients (dW: Wx, Wh, Wm, Wo, Wlast)
    if (t.dW[0] && (rc = plain_wgrad(stream, prec, g, w.du_x, 7 * Ch, t.x, Cin, k, k, w.slabs, t.dW[0]))) return rc;
    if (t.dW[1] && (rc = plain_wgrad(stream, prec, g, w.du_h, 4 * Ch, t.h, Ch, k, k, w.slabs, t.dW[1]))) return rc;
    if (t.dW[2] && (rc = plain_wgrad(stream, prec, g, w.du_m, 3 * Ch, t.m, Ch, k, k, w.slabs, t.dW[2]))) return rc;
    if (t.dW[3] && (rc = plain_wgrad(stream, prec, g, w.du_o, Ch, R.mem, 2 * Ch, k, k, w.slabs, t.dW[3]))) return rc;
    if (t.dW[4] && (rc = plain_wgrad(stream, prec, g, w.dlc, Ch, R.mem, 2 * Ch, 1, 1, w.slabs, t.dW[4]))) return rc;
    // G: LayerNorm parameter gradients back to the reference's [C,H,W]
    if (t.dln)
        for (int i = 0; i < 8; ++i)
            if (t.dln[i]) VPX_CHECK_HIP(launch_nhwc_to_nchw(w.dlnp[i], t.dln[i], 1, LN_MULT[i / 2] * Ch, s.H, s.W, stream));
    return st_stage_out(d, w.nchw, stream);
}

}  // namespace vpx
