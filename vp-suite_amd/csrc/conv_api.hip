// conv_api.hip — plain NHWC stride-1 "same" convolution backward and the decoupling-loss tail, built from the same
// implicit-GEMM / weight-gradient kernels as the recurrent cells.
//   vpx_conv2d_nhwc_bwd   dx = conv^T(dy, w) (transposed + tap-flipped packing), dw = wgrad(dy, x), db = colsum(dy)
//   vpx_decouple_fwd/_bwd adapter 1x1 conv on delta_c / delta_m, per-(b, channel) cosine over H*W, |.|, mean
//                         (vp_suite/models/predrnn_v2.py:197-198, 209-211)
#include "vpx_host.h"

using namespace vpx;

extern "C" {

size_t vpx_conv2d_bwd_workspace_bytes(int N, int H, int W, int Ci, int Co, int kh, int kw) {
    if (N < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1) return 0;
    return align256(plain_conv_wpk_floats(Co, Ci, kh, kw) * 4) +
           align256((size_t)wgrad_slices_for(N, H, W, Co, Ci, kh, kw) * kh * kw * Co * Ci * 4) + align256((size_t)COLSUM_BLOCKS * Co * 4) + 512;
}

int vpx_conv2d_nhwc_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int N, int H,
                        int W, int Ci, int Co, int kh, int kw, int precision, void* workspace, size_t workspace_bytes,
                        void* stream_) {
    if (!x || !w || !dy || N < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1 || !(kh & 1) || !(kw & 1) || kh > 7 || kw > 7) {
        set_error("vpx_conv2d_nhwc_bwd: bad argument");
        return VPX_ERR_ARG;
    }
    if ((precision < VPX_PREC_F32 || precision > VPX_PREC_BF16)) { set_error("vpx_conv2d_nhwc_bwd: precision %d not implemented", precision); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < vpx_conv2d_bwd_workspace_bytes(N, H, W, Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(plain_conv_wpk_floats(Co, Ci, kh, kw));
    const int slice_cap = wgrad_slices_for(N, H, W, Co, Ci, kh, kw);
    float* slabs = ws.take((size_t)slice_cap * kh * kw * Co * Ci);
    float* db_part = ws.take((size_t)COLSUM_BLOCKS * Co);
    VPX_CHECK_CARVE(ws, "vpx_conv2d_nhwc_bwd");
    const ConvGeo g{N, H, W};
    int rc;
    if (dx && (rc = plain_conv(stream, precision, g, dy, Co, Co, w, (long long)Ci * kh * kw, kh * kw, kh, kw, Ci, true,
                               nullptr, dx, Ci, false, wpk))) return rc;
    if (dw && (rc = plain_wgrad(stream, precision, g, dy, Co, x, Ci, kh, kw, slabs, dw, nullptr, slice_cap))) return rc;
    if (db) VPX_CHECK_HIP(launch_colsum(dy, nullptr, 0.f, nullptr, db, db_part, (long long)N * H * W, Co, stream));
    return VPX_OK;
}

/* y = act(conv(x, w) + bias [+ y]): stride-1 "same" convolution with an optional accumulate into the destination (a second
 * convolution summed into the same output, e.g. TrajGRU's i2f + h2f, traj_gru.py:134-142) and LeakyReLU on the sum. */
int vpx_conv2d_nhwc_fwd_ex(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Ci, int Co,
                           int kh, int kw, int precision, int accumulate, float leaky_slope, void* workspace,
                           size_t workspace_bytes, void* stream_) {
    if (!x || !w || !y || N < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1 || !(kh & 1) || !(kw & 1) || kh > 7 || kw > 7 || leaky_slope < 0.0f) {
        set_error("vpx_conv2d_nhwc_fwd_ex: bad argument");
        return VPX_ERR_ARG;
    }
    if ((precision < VPX_PREC_F32 || precision > VPX_PREC_BF16)) { set_error("vpx_conv2d_nhwc_fwd_ex: precision %d not implemented", precision); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_fwd_ex: workspace too small"); return VPX_ERR_WORKSPACE; }
    const ConvGeo g{N, H, W};
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(plain_conv_pack_floats(precision, g, Ci, kh, kw, Co));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_nhwc_fwd_ex");
    return plain_conv((hipStream_t)stream_, precision, g, x, Ci, Ci, w, (long long)Ci * kh * kw, kh * kw, kh, kw, Co, false, bias, y, Co,
                      accumulate != 0, wpk, leaky_slope);
}

/* ---- decoupling-loss tail ---------------------------------------------------------------------------------- */
}  // extern "C"
// Arithmetic of the tail's three 1x1 contractions (adapter forward, its adjoint, its weight gradient) = the caller's `precision`
// argument (the model's operand mode). bf16x3: fp32-level accuracy (4e-6; the loss value and its gradients hold the goldens'
// 1e-4 / 5e-5 bars) at a third of the exact-fp32 MFMA cycles — the fp32 forms cost PredRNN's bf16x3 training step 34 of 493 ms.
// The adapter (1x1, Ch -> Ch; transposed = its adjoint) applied to the c and the m operand. When both the sources and the
// destinations are adjacent in memory ([2, B, HW, Ch]: the cell step hands out delta_c | delta_m as one block, the
// workspace slots are adjacent) the pair is ONE convolution over 2B images — these launches are latency-bound (K = Ch).
static int decouple_adapter_pair(hipStream_t stream, int prec, ConvGeo g, const float* sc, const float* sm, const float* adapter,
                                 float* oc, float* om, size_t n, int Ch, bool transposed, float* wpk) {
    int rc;
    {   // streaming 1x1 kernel (conv1.hip): weights resident in registers, fp32 in and out
        C1Args c{};
        c.x[0] = sc; c.xld[0] = Ch; c.xc[0] = Ch; c.x[1] = nullptr; c.xld[1] = 0; c.xc[1] = 0;
        c.npix = (long long)g.N * g.H * g.W;
        c.w = adapter; c.w_sn = transposed ? 1 : Ch; c.w_sc = transposed ? Ch : 1;
        c.y[0] = oc; c.y[1] = nullptr; c.yld[0] = Ch; c.yld[1] = 0; c.ysplit = Ch; c.Co = Ch; c.accumulate = 0;
        if (c1_applicable(c, prec)) {
            if (sm == sc + n && om == oc + n) { c.npix *= 2; VPX_CHECK_HIP(launch_c1(c, stream)); return VPX_OK; }
            VPX_CHECK_HIP(launch_c1(c, stream));
            c.x[0] = sm; c.y[0] = om;
            VPX_CHECK_HIP(launch_c1(c, stream));
            return VPX_OK;
        }
    }
    if (sm == sc + n && om == oc + n) {
        const ConvGeo g2{2 * g.N, g.H, g.W};
        return plain_conv(stream, prec, g2, sc, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, transposed, nullptr, oc, Ch, false, wpk);
    }
    if ((rc = plain_conv(stream, prec, g, sc, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, transposed, nullptr, oc, Ch, false, wpk))) return rc;
    return plain_conv(stream, prec, g, sm, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, transposed, nullptr, om, Ch, false, wpk);
}
extern "C" {
size_t vpx_decouple_workspace_bytes(int B, int Ch, int H, int W) {
    if (B < 1 || Ch < 1 || H < 1 || W < 1) return 0;
    const size_t n = (size_t)B * H * W * Ch;
    return 4 * align256(n * 4) + align256((size_t)B * Ch * 4 * 4) + align256(plain_conv_wpk_floats(Ch, Ch, 1, 1) * 4) +
           align256((size_t)wgrad_slices_1x1(B, H, W) * Ch * Ch * 4) + align256((size_t)Ch * Ch * 4) + 1024;
}

static bool decouple_prec_ok(int prec, const char* who) {
    if (prec == VPX_PREC_F32 || prec == VPX_PREC_BF16X3 || prec == VPX_PREC_BF16) return true;
    set_error("%s: unknown precision %d", who, prec); return false;
}
int vpx_decouple_fwd(const float* delta_c, const float* delta_m, const float* adapter, float* value, int B, int Ch,
                     int H, int W, int prec, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!delta_c || !delta_m || !adapter || !value || B < 1 || Ch < 1 || H < 1 || W < 1) { set_error("vpx_decouple_fwd: bad argument"); return VPX_ERR_ARG; }
    if (!decouple_prec_ok(prec, "vpx_decouple_fwd")) return VPX_ERR_ARG;
    if (!workspace || workspace_bytes < vpx_decouple_workspace_bytes(B, Ch, H, W)) { set_error("vpx_decouple_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)B * H * W * Ch;
    Carver ws(workspace, workspace_bytes);
    float* yc = ws.take(n);
    float* ym = ws.take(n);
    ws.take(n); ws.take(n);  // (backward's dYc / dYm slots)
    float* stats = ws.take((size_t)B * Ch * 4);
    float* wpk = ws.take(plain_conv_wpk_floats(Ch, Ch, 1, 1));
    VPX_CHECK_CARVE(ws, "vpx_decouple_fwd");
    const ConvGeo g{B, H, W};
    int rc;
    if ((rc = decouple_adapter_pair(stream, prec, g, delta_c, delta_m, adapter, yc, ym, n, Ch, false, wpk))) return rc;
    VPX_CHECK_HIP(launch_decouple_stats(yc, ym, stats, B, H * W, Ch, stream));
    VPX_CHECK_HIP(launch_decouple_mean(stats, value, B * Ch, stream));
    return VPX_OK;
}

int vpx_decouple_bwd(const float* delta_c, const float* delta_m, const float* adapter, const float* dvalue,
                     float* d_delta_c, float* d_delta_m, float* d_adapter, int B, int Ch, int H, int W, int prec,
                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (!delta_c || !delta_m || !adapter || !dvalue || B < 1 || Ch < 1 || H < 1 || W < 1) { set_error("vpx_decouple_bwd: bad argument"); return VPX_ERR_ARG; }
    if (!decouple_prec_ok(prec, "vpx_decouple_bwd")) return VPX_ERR_ARG;
    if (!workspace || workspace_bytes < vpx_decouple_workspace_bytes(B, Ch, H, W)) { set_error("vpx_decouple_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)B * H * W * Ch;
    Carver ws(workspace, workspace_bytes);
    float* yc = ws.take(n);
    float* ym = ws.take(n);
    float* dyc = ws.take(n);
    float* dym = ws.take(n);
    float* stats = ws.take((size_t)B * Ch * 4);
    float* wpk = ws.take(plain_conv_wpk_floats(Ch, Ch, 1, 1));
    const int slice_cap = wgrad_slices_1x1(B, H, W);
    float* slabs = ws.take((size_t)slice_cap * Ch * Ch);
    float* dA2 = ws.take((size_t)Ch * Ch);
    VPX_CHECK_CARVE(ws, "vpx_decouple_bwd");
    const ConvGeo g{B, H, W};
    int rc;
    // recompute the adapter outputs (cheaper than keeping them alive between forward and backward)
    if ((rc = decouple_adapter_pair(stream, prec, g, delta_c, delta_m, adapter, yc, ym, n, Ch, false, wpk))) return rc;
    VPX_CHECK_HIP(launch_decouple_stats(yc, ym, stats, B, H * W, Ch, stream));
    VPX_CHECK_HIP(launch_decouple_bwd_pointwise(yc, ym, stats, dvalue, dyc, dym, B, H * W, Ch, stream));
    if (d_delta_c && d_delta_m) {
        if ((rc = decouple_adapter_pair(stream, prec, g, dyc, dym, adapter, d_delta_c, d_delta_m, n, Ch, true, wpk))) return rc;
    } else {
        if (d_delta_c && (rc = plain_conv(stream, prec, g, dyc, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, true, nullptr, d_delta_c, Ch, false, wpk))) return rc;
        if (d_delta_m && (rc = plain_conv(stream, prec, g, dym, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, true, nullptr, d_delta_m, Ch, false, wpk))) return rc;
    }
    if (d_adapter) {
        if (dym == dyc + n && (((uintptr_t)delta_c ^ (uintptr_t)delta_m) & 15) == 0) {
            // both pairs in ONE launch (the c and m halves are two "time steps"): one weight gradient + reduce instead of two + an add
            if ((rc = plain_wgrad(stream, prec, g, dyc, Ch, delta_c, Ch, 1, 1, slabs, d_adapter, delta_m, slice_cap))) return rc;
        } else {
            if ((rc = plain_wgrad(stream, prec, g, dyc, Ch, delta_c, Ch, 1, 1, slabs, d_adapter, nullptr, slice_cap))) return rc;
            if ((rc = plain_wgrad(stream, prec, g, dym, Ch, delta_m, Ch, 1, 1, slabs, dA2, nullptr, slice_cap))) return rc;
            VPX_CHECK_HIP(launch_axpy(d_adapter, dA2, (long long)Ch * Ch, stream));
        }
    }
    return VPX_OK;
}

}  // extern "C"

/* ---- general conv / transposed conv + bias + LeakyReLU (EF stage glue) -------------------------------------------- */
namespace {

struct ExGeo { int Ho, Wo; };

int ex_check(const vpx_conv_desc* d, ExGeo& g) {
    if (!d) { set_error("conv desc is NULL"); return VPX_ERR_ARG; }
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->Ci < 1 || d->Co < 1 || d->kh < 1 || d->kw < 1 || d->pad < 0) { set_error("conv desc: bad dimension"); return VPX_ERR_ARG; }
    if (d->stride != 1 && d->stride != 2) { set_error("conv desc: stride %d not implemented (1 or 2)", d->stride); return VPX_ERR_UNSUPPORTED; }
    if (d->kh > 7 || d->kw > 7) { set_error("conv desc: kernel larger than 7 not implemented"); return VPX_ERR_UNSUPPORTED; }
    if (d->precision < VPX_PREC_F32 || d->precision > VPX_PREC_BF16) { set_error("conv desc: unknown precision %d", d->precision); return VPX_ERR_UNSUPPORTED; }
    if (!d->transposed) {
        g.Ho = (d->H + 2 * d->pad - d->kh) / d->stride + 1;
        g.Wo = (d->W + 2 * d->pad - d->kw) / d->stride + 1;
    } else {
        if (d->out_pad_h < 0 || d->out_pad_w < 0 || d->out_pad_h >= d->stride || d->out_pad_w >= d->stride) { set_error("conv desc: output padding must be in [0, stride)"); return VPX_ERR_ARG; }
        g.Ho = (d->H - 1) * d->stride - 2 * d->pad + d->kh + d->out_pad_h;
        g.Wo = (d->W - 1) * d->stride - 2 * d->pad + d->kw + d->out_pad_w;
        if (d->stride == 1 && (d->kh - 1 - d->pad < 0 || d->kw - 1 - d->pad < 0)) { set_error("conv desc: padding larger than kernel-1 in a transposed conv"); return VPX_ERR_UNSUPPORTED; }
    }
    if (g.Ho < 1 || g.Wo < 1) { set_error("conv desc: empty output"); return VPX_ERR_ARG; }
    return VPX_OK;
}

// workgroup form of a glue launch: the 8-wave / 16x16-pixel tile when the grid stays large (pick_mw's rule) and the
// stride-1 halo keeps two such workgroups per CU
static int ex_mw(const vpx_conv_desc* d, int Ht, int Wt, int sd) {
    if (d->precision == VPX_PREC_F32 || sd != 1) return 1;
    const int mw = pick_mw(d->N, Ht, Wt, plain_tiles(d->Co), d->precision);
    const int segC[1] = {d->Ci};
    return (mw > 1 && !conv_fits_lds(segC, 1, d->kh, d->kw, plain_groups(d->Co), d->precision, mw, sd)) ? 1 : mw;
}

// one launch: tile space Ht x Wt, kernel taps th x tw, halo origin (oy, ox), input step `sd`
int ex_launch(hipStream_t stream, const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
              const ExGeo& g, int Ht, int Wt, int th, int tw, int sd, int oy, int ox, const int* tapmap, bool flip,
              int omap, int oys, int oyo, int oxs, int oxo, float* wpk, char* y_split = nullptr, bool x_split = false, bool packed = false,
              int act = 0) {
    const int prec = d->precision;
    ConvPlan P{};
    int chunks = 0;
    const int segC[1] = {d->Ci};
    P.prec = prec;
    const int ng = plain_groups(d->Co);
    const int mw = ex_mw(d, Ht, Wt, sd);
    P.nstage = build_stages(P.stage, &chunks, segC, 1, th * tw, pick_stage_channels(segC, 1, th, tw, ng, prec, mw, sd), prec);
    if (P.nstage < 0) { set_error("conv: too many channel stages (Ci=%d)", d->Ci); return VPX_ERR_UNSUPPORTED; }
    PackDesc pd{};
    const int src_taps = d->kh * d->kw;
    if (!d->transposed) pd.seg[0] = PackSeg{w, (long long)d->Ci * src_taps, src_taps, 0, d->Ci};
    else pd.seg[0] = PackSeg{w, (long long)d->Co * src_taps, src_taps, 0, d->Ci};
    memcpy(pd.stage, P.stage, sizeof(ConvStage) * P.nstage);
    pd.nstage = P.nstage; pd.chunks_total = chunks; pd.prec = prec; pd.taps = th * tw;
    fill_plain_pack(pd, d->Co, 0);
    pd.transposed = d->transposed ? 1 : 0;
    pd.flip = flip ? 1 : 0;
    if (tapmap) { pd.src_taps = src_taps; for (int i = 0; i < th * tw; ++i) pd.tapmap[i] = tapmap[i]; }
    if (!packed) VPX_CHECK_HIP(launch_pack_weights(pd, wpk, stream));   // (packed: the caller's workspace still holds this launch's pack)
    P.B = d->N; P.H = Ht; P.W = Wt; P.kh = th; P.kw = tw;
    set_plan_tiles(P, mw);
    P.stride = sd; P.use_org = 1; P.org_y = oy; P.org_x = ox; P.Hin = d->H; P.Win = d->W;
    P.nseg = 1;
    P.seg[0] = ConvSeg{x, (long long)d->H * d->W * d->Ci, d->Ci, d->Ci, x_split ? 1 : 0, 0};
    P.chunks_total = chunks;
    P.a_bytes = conv_a_bytes(P.stage, P.nstage, th, tw, mw, sd);
    P.wpk = wpk;
    PlainEpiArgs ea{};
    ea.bias = bias; ea.Co = d->Co; ea.split = d->Co; ea.ng = ng;
    ea.out0 = y; ea.bstride0 = (long long)g.Ho * g.Wo * d->Co; ea.ld0 = d->Co;
    ea.leaky = d->leaky_slope;
    ea.relu = act == VPX_ACT_RELU ? 1 : 0;
    ea.omap = omap; ea.oys = oys; ea.oyo = oyo; ea.oxs = oxs; ea.oxo = oxo; ea.Wmem = g.Wo;
    ea.sp_out = y_split; ea.sp_bstride = (long long)g.Ho * g.Wo * d->Co * 4;
    VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, pd.n_tiles, stream));
    return VPX_OK;
}

int ex_forward(const vpx_conv_desc* d, const ExGeo& g, const float* x, const float* w, const float* bias, float* y, float* wpk,
               hipStream_t stream, char* y_split = nullptr, bool x_split = false, bool packed = false, int act = 0);
bool exq_problem(const vpx_conv_desc* d, const ExGeo& g, ConvQProblem& pr);
int ex_forward_q(const vpx_conv_desc* d, const ExGeo& g, const char* x_sp, long long x_bstride, long long x_tstride, int x_nT,
                 const float* w, const float* bias, float* y, char* y_sp, char* wpk, bool weights_packed, hipStream_t stream);

size_t ex_wpk_floats(const vpx_conv_desc* d) {
    // upper bound over the launches this descriptor can produce (full tap set, stride as given)
    ConvStage st[MAX_STAGE];
    int chunks = 0;
    const int segC[1] = {d->Ci};
    const int ng = plain_groups(d->Co);
    const int sd = d->transposed ? 1 : d->stride;
    size_t best = 0;
    for (int mw = 1; mw <= 2; ++mw) {  // upper bound over both workgroup forms (their stage sizes differ)
        if (build_stages(st, &chunks, segC, 1, d->kh * d->kw, pick_stage_channels(segC, 1, d->kh, d->kw, ng, d->precision, mw, sd), d->precision) < 0) return 0;
        const size_t b = packed_weight_bytes(plain_tiles(d->Co), chunks, ng, d->precision) / 4 + 1024;
        if (b > best) best = b;
    }
    return best;
}

}  // namespace

extern "C" {

int vpx_conv2d_ex_out_shape(const vpx_conv_desc* d, int* Ho, int* Wo) {
    ExGeo g;
    int rc = ex_check(d, g);
    if (rc != VPX_OK) return rc;
    if (Ho) *Ho = g.Ho;
    if (Wo) *Wo = g.Wo;
    return VPX_OK;
}

size_t vpx_conv2d_ex_workspace_bytes(const vpx_conv_desc* d) {
    ExGeo g;
    if (ex_check(d, g) != VPX_OK) return 0;
    return align256(ex_wpk_floats(d) * 4) + 512;
}

int vpx_conv2d_ex_fwd(const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                      void* workspace, size_t workspace_bytes, void* stream_) {
    ExGeo g;
    int rc = ex_check(d, g);
    if (rc != VPX_OK) return rc;
    if (!x || !w || !y) { set_error("vpx_conv2d_ex_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_conv2d_ex_workspace_bytes(d)) { set_error("vpx_conv2d_ex_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(ex_wpk_floats(d));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_ex_fwd");
    return ex_forward(d, g, x, w, bias, y, wpk, (hipStream_t)stream_);
}

// activation codes beyond the descriptor's LeakyReLU: leaky_slope == 0 means "no activation" there, so ReLU travels beside it
static int ex_act_check(const vpx_conv_desc* d, int act, const char* who) {
    if (act != VPX_ACT_NONE && act != VPX_ACT_RELU) { set_error("%s: unknown activation code %d", who, act); return VPX_ERR_ARG; }
    if (d && act == VPX_ACT_RELU && d->leaky_slope != 0.0f) { set_error("%s: VPX_ACT_RELU with a LeakyReLU slope in the descriptor", who); return VPX_ERR_ARG; }
    return VPX_OK;
}

size_t vpx_conv2d_act_workspace_bytes(const vpx_conv_desc* d, int act) {
    if (ex_act_check(d, act, "vpx_conv2d_act_workspace_bytes") != VPX_OK) return 0;
    return vpx_conv2d_ex_workspace_bytes(d);
}

int vpx_conv2d_act_fwd(const vpx_conv_desc* d, int act, const float* x, const float* w, const float* bias, float* y, void* workspace,
                       size_t workspace_bytes, void* stream_) {
    ExGeo g;
    int rc = ex_check(d, g);
    if (rc != VPX_OK) return rc;
    if ((rc = ex_act_check(d, act, "vpx_conv2d_act_fwd")) != VPX_OK) return rc;
    if (!x || !w || !y) { set_error("vpx_conv2d_act_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_conv2d_ex_workspace_bytes(d)) { set_error("vpx_conv2d_act_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(ex_wpk_floats(d));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_act_fwd");
    return ex_forward(d, g, x, w, bias, y, wpk, (hipStream_t)stream_, nullptr, false, false, act);
}

int vpx_conv2d_ex_fwd_split(const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* y_split,
                            void* workspace, size_t workspace_bytes, void* stream_) {
    ExGeo g;
    int rc = ex_check(d, g);
    if (rc != VPX_OK) return rc;
    if (!x || !w || !y_split) { set_error("vpx_conv2d_ex_fwd_split: NULL tensor argument"); return VPX_ERR_ARG; }
    if (d->Co & 7) { set_error("vpx_conv2d_ex_fwd_split: the split format needs Co to be a multiple of 8 (got %d)", d->Co); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < vpx_conv2d_ex_workspace_bytes(d)) { set_error("vpx_conv2d_ex_fwd_split: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(ex_wpk_floats(d));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_ex_fwd_split");
    return ex_forward(d, g, x, w, bias, y, wpk, (hipStream_t)stream_, reinterpret_cast<char*>(y_split));
}

// Which kernel takes a layer on split input (measured, tools/ab_glue.py, ms per 1280 frames, first generation on split input ->
// convq on half tiles): layers with >= 64 output channels — stride-2 convolutions 64 -> 64 at 64x64 0.72 -> 0.60 and 96 -> 96 at
// 32x32 0.32 -> 0.25, stride-2 transposed 4x4 96 -> 96 at 16x16 0.48 -> 0.38 and at 32x32 1.79 -> 1.47 (at 40 frames 0.12 -> 0.04 /
// 0.15 -> 0.06: the phase form is one launch) — but plain convolutions only on grids of >= 256 workgroups (40 frames: 0.045 -> 0.049).
// 3x3 stride-1 layers with 16 output channels (64 -> 16: 0.83 first generation, 1.22 convq) have their own kernel (conv16.hip: 0.41).
static bool exq_preferred(const vpx_conv_desc* d, const ExGeo& g, ConvQProblem& pr) {
    if (!exq_problem(d, g, pr) || convq_wpk_bytes(pr) == 0) return false;
    if (d->Co < 64) return false;
    if (pr.phases) return true;
    const long long wgs = (long long)pr.N * ((pr.W + 15) / 16) * ((pr.H + 15) / 16) * (((d->Co + 31) / 32 + 3) / 4);
    return wgs >= 256;
}
static bool ex_split_gen1_ok(const vpx_conv_desc* d) {
    return d->precision != VPX_PREC_F32 && (d->Ci & 7) == 0;
}

int vpx_conv2d_ex_takes_split(const vpx_conv_desc* d) {
    ExGeo g;
    static thread_local ConvQProblem pr;
    if (ex_check(d, g) != VPX_OK) return 0;
    if (exq_preferred(d, g, pr) || c16_applicable(d)) return 2;
    return ex_split_gen1_ok(d) ? 1 : 0;
}

size_t vpx_conv2d_ex_split_workspace_bytes(const vpx_conv_desc* d) {
    ExGeo g;
    static thread_local ConvQProblem pr;
    if (ex_check(d, g) != VPX_OK) return 0;
    size_t b = 0;
    if (exq_preferred(d, g, pr)) b = align256(convq_wpk_bytes(pr)) + 512;
    if (ex_split_gen1_ok(d)) { const size_t b1 = align256(ex_wpk_floats(d) * 4) + 512; if (b1 > b) b = b1; }
    if (c16_applicable(d)) { const size_t b1 = align256(c16_wpk_bytes(d)) + 512; if (b1 > b) b = b1; }
    return b;
}

int vpx_conv2d_ex_fwd_from_split(const vpx_conv_desc* d, const void* x_split, long long x_bstride, long long x_tstride, int x_nT,
                                 const float* w, const float* bias, float* y, void* y_split, int weights_packed, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
    ExGeo g;
    int rc = ex_check(d, g);
    if (rc != VPX_OK) return rc;
    if (!x_split || !w || (!y && !y_split)) { set_error("vpx_conv2d_ex_fwd_from_split: NULL tensor argument"); return VPX_ERR_ARG; }
    if (y_split && (d->Co & 7)) { set_error("vpx_conv2d_ex_fwd_from_split: the split format needs Co to be a multiple of 8 (got %d)", d->Co); return VPX_ERR_UNSUPPORTED; }
    const size_t need = vpx_conv2d_ex_split_workspace_bytes(d);
    if (!need) { set_error("vpx_conv2d_ex_fwd_from_split: layer not implemented on split input (vpx_conv2d_ex_takes_split)"); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < need) { set_error("vpx_conv2d_ex_fwd_from_split: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    char* wpk = reinterpret_cast<char*>(ws.take((need - 512) / 4));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_ex_fwd_from_split");
    const long long dense = (long long)d->H * d->W * d->Ci * 4;
    if (x_bstride == 0) x_bstride = dense;
    static thread_local ConvQProblem pr;
    if (c16_applicable(d))   // 16 output channels: the whole K of a tile resident (conv16.hip)
        return c16_forward(d, reinterpret_cast<const char*>(x_split), x_bstride, x_tstride, x_nT, w, bias, y, reinterpret_cast<char*>(y_split),
                           wpk, weights_packed != 0, (hipStream_t)stream_);
    if (exq_preferred(d, g, pr))
        return ex_forward_q(d, g, reinterpret_cast<const char*>(x_split), x_bstride, x_tstride, x_nT, w, bias, y, reinterpret_cast<char*>(y_split),
                            wpk, weights_packed != 0, (hipStream_t)stream_);
    if (x_nT > 1 || x_bstride != dense) { set_error("vpx_conv2d_ex_fwd_from_split: this layer needs a dense batch of split images"); return VPX_ERR_UNSUPPORTED; }
    return ex_forward(d, g, reinterpret_cast<const float*>(x_split), w, bias, y, reinterpret_cast<float*>(wpk), (hipStream_t)stream_,
                      reinterpret_cast<char*>(y_split), true, weights_packed != 0);
}

}  // extern "C"

namespace {

// packed: the workspace still holds the layer's packed weights — honoured by the single-launch forms (the four phase launches of a
// stride-2 transposed layer pack into the same space one after the other)
int ex_forward(const vpx_conv_desc* d, const ExGeo& g, const float* x, const float* w, const float* bias, float* y, float* wpk,
               hipStream_t stream, char* y_split, bool x_split, bool packed, int act) {
    int rc;
    const int small_kind = (x_split || act) ? 0 : conv_small_kind(d);   // (the streaming kernels read fp32 and know LeakyReLU only)
    if (const int kind = small_kind) {   // few-channel layers: streaming kernels (conv_small.hip)
        if (kind != 2 || !y_split) {
            VPX_CHECK_HIP(launch_conv_small(d, kind, x, w, bias, y, y_split, stream));
            return VPX_OK;
        }
    }
    if (!d->transposed)  // y[o] = sum_k x[o*s - pad + k] w[k]
        return ex_launch(stream, d, x, w, bias, y, g, g.Ho, g.Wo, d->kh, d->kw, d->stride, -d->pad, -d->pad, nullptr, false,
                         0, 1, 0, 1, 0, wpk, y_split, x_split, packed, act);
    if (d->stride == 1)  // y[o] = sum_k x[o + pad - k] w[k]  ==  correlation with the flipped kernel, origin -(k-1-pad)
        return ex_launch(stream, d, x, w, bias, y, g, g.Ho, g.Wo, d->kh, d->kw, 1, -(d->kh - 1 - d->pad), -(d->kw - 1 - d->pad),
                         nullptr, true, 0, 1, 0, 1, 0, wpk, y_split, x_split, packed, act);
    // stride 2: output phase (py, px) is a stride-1 correlation of x with the taps k == (p + pad) mod 2 of that axis
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const int Ht = (g.Ho - py + 1) / 2, Wt = (g.Wo - px + 1) / 2;
            if (Ht < 1 || Wt < 1) continue;
            const int ky0 = (py + d->pad) & 1, kx0 = (px + d->pad) & 1;
            const int nty = (d->kh - ky0 + 1) / 2, ntx = (d->kw - kx0 + 1) / 2;
            if (nty < 1 || ntx < 1) {  // no tap feeds this phase: bias (+activation) only — not reachable for k >= 2
                set_error("vpx_conv2d_ex_fwd: kernel too small for stride 2");
                return VPX_ERR_UNSUPPORTED;
            }
            if (nty * ntx > 16) { set_error("vpx_conv2d_ex_fwd: too many taps per phase"); return VPX_ERR_UNSUPPORTED; }
            const int basey = (py + d->pad - ky0) / 2, basex = (px + d->pad - kx0) / 2;
            int tapmap[16];
            for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx)
                    tapmap[ty * ntx + tx] = (ky0 + 2 * (nty - 1 - ty)) * d->kw + (kx0 + 2 * (ntx - 1 - tx));
            rc = ex_launch(stream, d, x, w, bias, y, g, Ht, Wt, nty, ntx, 1, basey - (nty - 1), basex - (ntx - 1), tapmap, false,
                           1, 2, py, 2, px, wpk, y_split, x_split, false, act);
            if (rc != VPX_OK) return rc;
        }
    return VPX_OK;
}

// ---- the same layers on SPLIT-format input through the schedule-driven K = 32 kernel (convq.hip) -----------------------
// Terms of a layer (see convq.hip): a convolution with stride s reads the s x s sub-images x[s*i + sy, s*j + sx] of its input,
// tap ky of row residue sy = (ky - pad) mod s lands at da = (ky - pad - sy) / s; a transposed convolution computes output phase
// (py, px) = (oy mod s, ox mod s) as a stride-1 correlation over x with the taps ky = (py + pad) mod s (+ s, ...) at
// da = -(ky - py - pad) / s. Sub-positions with a single tap get a zero-weight filler so that their stages span a whole step.
bool exq_problem(const vpx_conv_desc* d, const ExGeo& g, ConvQProblem& pr) {
    memset(&pr, 0, sizeof(pr));
    if (d->precision != VPX_PREC_BF16X3 || (d->Ci & 15) || d->Ci < 16 || d->Ci / 16 > 60) return false;
    const int s = d->stride, p = d->pad;
    const int nst = d->Ci / 16;
    const int row = d->W * d->Ci * 4, pix = d->Ci * 4;
    pr.N = d->N; pr.halo = 2;
    pr.Co = d->Co; pr.col0 = 0;
    const int taps = d->kh * d->kw;
    if (taps > 25) return false;
    auto fmod_ = [](int a, int b) { return ((a % b) + b) % b; };
    if (!d->transposed) {
        pr.s_oc = (long long)d->Ci * taps; pr.s_ic = taps;
        pr.H = g.Ho; pr.W = g.Wo;
        pr.nseg = s * s; pr.ngs = 1; pr.phases = 0;
        if (pr.nseg > 4) return false;
        ConvQGroupSet& gs = pr.gs[0];
        gs.nt0 = 0; gs.ntn = 8; gs.nterm = 0;
        int per_seg[4] = {0, 0, 0, 0};
        for (int sy = 0; sy < s; ++sy)
            for (int sx = 0; sx < s; ++sx) {
                const int si = sy * s + sx;
                CQSeg& sg = pr.seg[si];
                sg.sp = nullptr; sg.nT = 1;
                sg.rowpitch = s * row; sg.colpitch = s * pix; sg.org = (sy * d->W + sx) * pix;
                sg.Hs = (d->H - sy + s - 1) / s; sg.Ws = (d->W - sx + s - 1) / s;
                sg.nstage = nst; sg.c0 = 0; pr.seg_wc0[si] = 0;
            }
        for (int ky = 0; ky < d->kh; ++ky)
            for (int kx = 0; kx < d->kw; ++kx) {
                const int sy = fmod_(ky - p, s), sx = fmod_(kx - p, s);
                const int da = (ky - p - sy) / s, db = (kx - p - sx) / s;
                if (da < -1 || da > 1 || db < -1 || db > 1 || gs.nterm >= 30) return false;
                gs.term[gs.nterm++] = ConvQTerm{sy * s + sx, da, db, ky * d->kw + kx};
                ++per_seg[sy * s + sx];
            }
        for (int si = 0; si < pr.nseg; ++si) {
            if (per_seg[si] == 0) return false;   // a sub-image nobody reads (kernel smaller than the stride)
            if (per_seg[si] == 1 && s > 1) {      // filler: the same tap again with zero weights
                for (int k = 0; k < gs.nterm; ++k)
                    if (gs.term[k].seg == si) { ConvQTerm f = gs.term[k]; f.wtap = -1; gs.term[gs.nterm++] = f; break; }
            }
        }
        pr.periodic = s == 1 ? 1 : 0;
    } else {
        pr.s_oc = taps; pr.s_ic = (long long)d->Co * taps;
        pr.nseg = 1;
        CQSeg& sg = pr.seg[0];
        sg.sp = nullptr; sg.nT = 1; sg.rowpitch = row; sg.colpitch = pix; sg.org = 0; sg.Hs = d->H; sg.Ws = d->W; sg.nstage = nst; sg.c0 = 0;
        pr.seg_wc0[0] = 0;
        pr.H = (g.Ho + s - 1) / s; pr.W = (g.Wo + s - 1) / s;
        pr.phases = s == 2 ? 1 : 0;
        pr.ngs = s * s;
        for (int py = 0; py < s; ++py)
            for (int px = 0; px < s; ++px) {
                ConvQGroupSet& gs = pr.gs[py * s + px];
                gs.nt0 = s == 2 ? 2 * (py * 2 + px) : 0; gs.ntn = s == 2 ? 2 : 8; gs.nterm = 0;
                for (int ky = fmod_(py + p, s); ky < d->kh; ky += s)
                    for (int kx = fmod_(px + p, s); kx < d->kw; kx += s) {
                        const int da = -(ky - py - p) / s, db = -(kx - px - p) / s;
                        if (da < -1 || da > 1 || db < -1 || db > 1 || gs.nterm >= 30) return false;
                        gs.term[gs.nterm++] = ConvQTerm{0, da, db, ky * d->kw + kx};
                    }
                if (gs.nterm == 0) return false;
            }
        pr.periodic = s == 1 ? 1 : 0;
    }
    return true;
}

int ex_forward_q(const vpx_conv_desc* d, const ExGeo& g, const char* x_sp, long long x_bstride, long long x_tstride, int x_nT,
                 const float* w, const float* bias, float* y, char* y_sp, char* wpk, bool weights_packed, hipStream_t stream) {
    static thread_local ConvQProblem pr;
    if (!exq_problem(d, g, pr)) { set_error("vpx_conv2d_ex_fwd_from_split: layer not implemented on split input"); return VPX_ERR_UNSUPPORTED; }
    for (int i = 0; i < pr.nseg; ++i) { pr.seg[i].sp = x_sp; pr.seg[i].bstride = x_bstride; pr.seg[i].tstride = x_tstride; pr.seg[i].nT = x_nT > 0 ? x_nT : 1; }
    pr.w = w;
    ConvQEpiArgs ea{};
    ea.bias = bias; ea.leaky = d->leaky_slope; ea.Co = d->Co; ea.split = d->Co;
    const int s = d->transposed ? d->stride : 1;
    ea.oys = s; ea.oxs = s; ea.oyo = 0; ea.oxo = 0; ea.Hmem = g.Ho; ea.Wmem = g.Wo;
    ea.out0 = y; ea.bstride0 = (long long)g.Ho * g.Wo * d->Co; ea.ld0 = d->Co;
    ea.sp_out = y_sp; ea.sp_bstride = (long long)g.Ho * g.Wo * d->Co * 4;
    return convq_run(pr, ea, wpk, weights_packed, stream);
}

constexpr long long GLUE_SLAB_FLOATS = 4ll << 20;  // K-slice slab budget of the glue weight gradients (16 MB)

// dW[r][c][ky][kx] = sum_{b,y,x} G[b,y,x,r] * A[b, s*y + ky - p, s*x + kx - p, c]   (G: [N,Hg,Wg,Rg], A: [N,Ha,Wa,Ca], NHWC).
// ky - p = s*a + ry: the taps of one residue (ry, rx) slide over the sub-image A[s*i + ry, s*j + rx] with offsets a —
// one stride-1 weight-gradient launch per residue on the MFMA kernel, its taps scattered into dW by the reduce.
// G_sp / A_sp (round 6): both operands once more in the split format — residues with >= 2 taps then run on wgrad2_kernel's glue form
// (LDS-DMA staging, no conversion work in the loop; wgrad2.hip), `slab_floats` = what `slabs` holds.
int strided_wgrad(hipStream_t stream, int prec, int N, int Hg, int Wg, const float* G, int Rg, int Ha, int Wa, const float* A,
                  int Ca, int kh, int kw, int s, int p, float* slabs, float* dW, const char* G_sp = nullptr, const char* A_sp = nullptr,
                  size_t slab_floats = 0) {
    auto fdiv = [](int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); };
    for (int ry = 0; ry < s; ++ry)
        for (int rx = 0; rx < s; ++rx) {
            // taps of this residue: ky = ky0, ky0 + s, ...
            int ky0 = ((p + ry) % s + s) % s, kx0 = ((p + rx) % s + s) % s;
            const int nty = ky0 < kh ? (kh - ky0 + s - 1) / s : 0, ntx = kx0 < kw ? (kw - kx0 + s - 1) / s : 0;
            if (nty < 1 || ntx < 1) continue;
            if (nty * ntx > 16 && s != 1) { set_error("conv wgrad: too many taps per residue"); return VPX_ERR_UNSUPPORTED; }
            WgradArgs wa{};
            wa.T = 1; wa.B = N; wa.H = Hg; wa.W = Wg; wa.HW = Hg * Wg; wa.kh = nty; wa.kw = ntx;
            wa.tiles_x = (Wg + TILE_W - 1) / TILE_W; wa.tiles_y = (Hg + TILE_H - 1) / TILE_H;
            wa.N4 = Rg; wa.Cin = Ca; wa.Ch = 1; wa.Ct = Ca; wa.ldG = Rg; wa.n_out = Rg; wa.prec = prec;
            wa.dG = G; wa.x = A; wa.x_bstride = (long long)Ha * Wa * Ca;
            wa.a_sub = 1; wa.a_sy = s; wa.a_sx = s; wa.a_oy = ry; wa.a_ox = rx;
            wa.a_Hs = (Ha - ry + s - 1) / s; wa.a_Ws = (Wa - rx + s - 1) / s; wa.a_Wfull = Wa;
            wa.use_org = 1; wa.org_y = fdiv(ky0 - p - ry, s); wa.org_x = fdiv(kx0 - p - rx, s);
            wa.n_ctiles = wgrad_make_ctiles(wa.ct, WG_MAX_CTILES, Ca, 0, 0);
            if (wa.n_ctiles < 0) { set_error("conv wgrad: too many channels (%d)", Ca); return VPX_ERR_UNSUPPORTED; }
            wa.slabs = slabs;
            const int taps = nty * ntx;
            // K slices: ~1024 workgroups, bounded by the work items and by the slab budget (GLUE_SLAB_FLOATS, or 32 slices
            // when one slice alone is that large). Layers with few rows x channels (1->16, 16->1) get all their
            // parallelism from the slices.
            const long long items = (long long)N * wa.tiles_x * wa.tiles_y;
            const long long per_slice = (long long)taps * Rg * Ca;
            long long cap = GLUE_SLAB_FLOATS / per_slice;
            if (cap < 32) cap = 32;
            int ns = wgrad_pick_slices((int)(cap < items ? cap : items), Rg, wa.n_ctiles, taps);
            WgradArgs wq = wa;
            wq.g_sp = G_sp; wq.x_sp = A_sp; wq.x_sp_bstride = (long long)Ha * Wa * Ca * 4; wq.a_split = 1;
            if (G_sp && A_sp && wgrad2g_applicable(wq)) {
                const long long room = (long long)(slab_floats / (size_t)per_slice);
                VPX_CHECK_HIP(launch_wgrad2g(wq, (int)(room < 1 ? 1 : (room > 4096 ? 4096 : room)), &ns, stream));
            } else
            VPX_CHECK_HIP(launch_wgrad(wa, ns, stream));
            if (s == 1) {
                VPX_CHECK_HIP(launch_wgrad_reduce(slabs, dW, ns, taps, Rg, Ca, stream));
            } else {
                int tapmap[16];
                for (int ty = 0; ty < nty; ++ty)
                    for (int tx = 0; tx < ntx; ++tx) tapmap[ty * ntx + tx] = (ky0 + s * ty) * kw + (kx0 + s * tx);
                VPX_CHECK_HIP(launch_wgrad_reduce_map(slabs, dW, ns, taps, Rg, Ca, kh * kw, tapmap, stream));
            }
        }
    return VPX_OK;
}

// the adjoint layer of d (what maps dy to dx), as a forward descriptor
int ex_adjoint(const vpx_conv_desc* d, const ExGeo& g, vpx_conv_desc& a) {
    a = *d;
    a.H = g.Ho; a.W = g.Wo; a.Ci = d->Co; a.Co = d->Ci; a.leaky_slope = 0.0f;
    a.out_pad_h = a.out_pad_w = 0;
    if (!d->transposed) {  // dx = conv_transpose2d(dy, w, stride, pad, output_padding = the rows/cols the forward conv dropped)
        a.transposed = 1;
        a.out_pad_h = (d->H + 2 * d->pad - d->kh) % d->stride;
        a.out_pad_w = (d->W + 2 * d->pad - d->kw) % d->stride;
    } else {               // dx = conv2d(dy, w, stride, pad)
        a.transposed = 0;
    }
    ExGeo ga;
    if (ex_check(&a, ga) != VPX_OK) return VPX_ERR_UNSUPPORTED;
    if (ga.Ho != d->H || ga.Wo != d->W) { set_error("conv bwd: adjoint shape %dx%d != input %dx%d", ga.Ho, ga.Wo, d->H, d->W); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

// weight gradient on split copies of x and dy (wgrad2_kernel's glue form): bf16x3 on the 16x16x32 shape, channel counts in whole groups of 8
static bool ex_wgrad_split(const vpx_conv_desc* d) {
    return !exp_on(VPX_EXP_GLUE_WGRAD_TAPGROUP) && d->precision == VPX_PREC_BF16X3 && g_mfma_shape == 1 && (d->Ci & 7) == 0 && (d->Co & 7) == 0 &&
           d->kh <= 2 * d->stride + 1 && d->kw <= 2 * d->stride + 1 && d->kh * d->kw > 1 &&
           !(!d->transposed && wgrad_small_applicable(d->Co, d->Ci, d->kh, d->kw, d->stride, d->pad));
}

size_t ex_bwd_slab_floats(const vpx_conv_desc* d, const ExGeo& g) {
    // a residue launch uses <= max(32 slices, GLUE_SLAB_FLOATS / slice) slices of <= kh*kw*Ci*Co floats
    (void)g;
    const size_t full = (size_t)32 * d->kh * d->kw * d->Ci * d->Co;
    size_t b = full > (size_t)GLUE_SLAB_FLOATS ? full : (size_t)GLUE_SLAB_FLOATS;
    // the glue form of wgrad2_kernel: up to WGRAD2_TARGET_WGS workgroups = that many slices of ONE row x column tile pair
    // (a residue's slab is at most kh * kw * Ci * Co / stride^2 floats)
    if (ex_wgrad_split(d)) {
        const int rows = ((d->transposed ? d->Ci : d->Co) + 127) / 128, cols = ((d->transposed ? d->Co : d->Ci) + 63) / 64;
        const size_t per = (size_t)((d->kh + d->stride - 1) / d->stride) * ((d->kw + d->stride - 1) / d->stride) * d->Ci * d->Co;
        const size_t need = (size_t)(WGRAD2_TARGET_WGS / (rows * cols) + 1) * per;
        if (need > b) b = need;
    }
    return b;
}

}  // namespace

extern "C" {

// Round 5: the data gradient of a glue layer = its adjoint layer on dy. Where that adjoint is a layer the schedule-driven K = 32 kernel
// (convq) takes — the same rule as in the forward: bf16x3, >= 64 output channels, a grid that fills the chip — it runs THERE: the pass
// that scales dy by LeakyReLU' (and sums the bias gradient) writes the scaled gradient once more in the split operand format.
// VPX_EXP_GLUE_DGRAD_GEN1 keeps the first-generation launch (A/B runs, tests).
static bool ex_bwd_q(const vpx_conv_desc* d, const vpx_conv_desc* a, ConvQProblem& pr) {
    if (exp_on(VPX_EXP_GLUE_DGRAD_GEN1) || (d->Co & 7)) return false;
    const ExGeo ga{d->H, d->W};
    return exq_preferred(a, ga, pr) && convq_wpk_bytes(pr) != 0;
}

size_t vpx_conv2d_ex_bwd_workspace_bytes(const vpx_conv_desc* d) {
    ExGeo g;
    vpx_conv_desc a;
    if (ex_check(d, g) != VPX_OK || ex_adjoint(d, g, a) != VPX_OK) return 0;
    // + the LeakyReLU'-scaled copy of dy and the bias-gradient partials
    const size_t n_dy = (size_t)d->N * g.Ho * g.Wo * d->Co;
    size_t b = align256(ex_wpk_floats(&a) * 4) + align256(ex_bwd_slab_floats(d, g) * 4) + align256(n_dy * 4) +
               align256((size_t)COLSUM_BLOCKS * d->Co * 4) + 1024;
    static thread_local ConvQProblem pr;
    if (ex_bwd_q(d, &a, pr)) b += align256(n_dy * 4) + align256(convq_wpk_bytes(pr));   // dy in the split format + the adjoint's convq pack
    if (ex_wgrad_split(d)) b += align256(n_dy * 4) + align256((size_t)d->N * d->H * d->W * d->Ci * 4);   // dy and x in the split format
    return b;
}

int vpx_conv2d_ex_bwd_uses_split(const vpx_conv_desc* d) {
    ExGeo g;
    if (!d || ex_check(d, g) != VPX_OK) return 0;
    return ex_wgrad_split(d) ? 1 : 0;
}

int vpx_conv2d_ex_bwd(const vpx_conv_desc* d, const float* x, const float* w, const float* y, const float* dy, float* dx,
                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    return vpx_conv2d_ex_bwd_ex(d, x, nullptr, w, y, dy, dx, dw, db, workspace, workspace_bytes, stream_);
}

static int ex_bwd_impl(const char* who, const vpx_conv_desc* d, int act, const float* x, const void* x_split, const float* w, const float* y,
                       const float* dy, float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_);

int vpx_conv2d_ex_bwd_ex(const vpx_conv_desc* d, const float* x, const void* x_split, const float* w, const float* y, const float* dy, float* dx,
                         float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    return ex_bwd_impl("vpx_conv2d_ex_bwd", d, VPX_ACT_NONE, x, x_split, w, y, dy, dx, dw, db, workspace, workspace_bytes, stream_);
}

size_t vpx_conv2d_act_bwd_workspace_bytes(const vpx_conv_desc* d, int act) {
    if (ex_act_check(d, act, "vpx_conv2d_act_bwd_workspace_bytes") != VPX_OK) return 0;
    return vpx_conv2d_ex_bwd_workspace_bytes(d);
}

/* ReLU' is read off the saved output (y > 0: zero at y == 0, as torch's threshold backward for finite dy) in the pass that sums the bias
 * gradient. That pass multiplies dy by the 0 / 1 derivative (launch_colsum, shared with LeakyReLU): a non-finite dy at a dead unit
 * gives NaN where torch's select gives 0. */
int vpx_conv2d_act_bwd(const vpx_conv_desc* d, int act, const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw,
                       float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = ex_act_check(d, act, "vpx_conv2d_act_bwd")) return rc;
    return ex_bwd_impl("vpx_conv2d_act_bwd", d, act, x, nullptr, w, y, dy, dx, dw, db, workspace, workspace_bytes, stream_);
}

static int ex_bwd_impl(const char* who, const vpx_conv_desc* d, int act, const float* x, const void* x_split, const float* w, const float* y,
                       const float* dy, float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    ExGeo g;
    int rc = ex_check(d, g);
    if (rc != VPX_OK) return rc;
    vpx_conv_desc a;
    if ((rc = ex_adjoint(d, g, a)) != VPX_OK) return rc;
    if (d->kh < d->stride || d->kw < d->stride) { set_error("%s: kernel smaller than the stride", who); return VPX_ERR_UNSUPPORTED; }
    if (!x || !w || !dy) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_conv2d_ex_bwd_workspace_bytes(d)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(ex_wpk_floats(&a));
    float* slabs = ws.take(ex_bwd_slab_floats(d, g));
    const size_t n_dy = (size_t)d->N * g.Ho * g.Wo * d->Co;
    float* dys = ws.take(n_dy);
    float* db_part = ws.take((size_t)COLSUM_BLOCKS * d->Co);
    static thread_local ConvQProblem prq;
    const bool dq = dx && ex_bwd_q(d, &a, prq);
    char *dy_sp = nullptr, *wpkq = nullptr;
    if (dq) { dy_sp = (char*)ws.take(n_dy); wpkq = (char*)ws.take(align256(convq_wpk_bytes(prq)) / 4); }
    const bool wsp = dw && ex_wgrad_split(d);
    char* x_sp = nullptr;
    if (wsp) { if (!dy_sp) dy_sp = (char*)ws.take(n_dy); x_sp = (char*)ws.take((size_t)d->N * d->H * d->W * d->Ci); }
    VPX_CHECK_CARVE(ws, who);
    const bool v4 = (d->Co & 3) == 0 && (((uintptr_t)dy | (uintptr_t)y) & 15) == 0;   // (launch_colsum's vector form: the split copy needs it)
    bool have_sp = false;
    if (d->leaky_slope != 0.0f || act == VPX_ACT_RELU) {
        // d(pre-activation) = dy * LeakyReLU'(.), the derivative read off the sign of the forward OUTPUT (same sign as the
        // pre-activation for a positive slope) — one pass that also yields the bias gradient
        if (!y) { set_error("%s: y (forward output) is required when the layer has an activation", who); return VPX_ERR_ARG; }
        if (d->leaky_slope < 0.0f) { set_error("%s: negative leaky_slope is not implemented", who); return VPX_ERR_UNSUPPORTED; }
        have_sp = (dq || wsp) && v4;
        VPX_CHECK_HIP(launch_colsum(dy, y, d->leaky_slope, dys, db, db_part, (long long)d->N * g.Ho * g.Wo, d->Co, stream, have_sp ? dy_sp : nullptr));
        dy = dys;
    } else if (db) {
        VPX_CHECK_HIP(launch_colsum(dy, nullptr, 0.f, nullptr, db, db_part, (long long)d->N * g.Ho * g.Wo, d->Co, stream));
    }
    if (dx) {
        ExGeo ga{d->H, d->W};
        if (dq) {
            if (!have_sp) { VPX_CHECK_HIP(launch_split_convert(dy, dy_sp, (long long)d->N * g.Ho * g.Wo, d->Co, stream)); have_sp = true; }
            if ((rc = ex_forward_q(&a, ga, dy_sp, (long long)g.Ho * g.Wo * d->Co * 4, 0, 1, w, nullptr, dx, nullptr, wpkq, false, stream)) != VPX_OK) return rc;
        } else if ((rc = ex_forward(&a, ga, dy, w, nullptr, dx, wpk, stream)) != VPX_OK) return rc;
    }
    if (dw && !d->transposed && wgrad_small_applicable(d->Co, d->Ci, d->kh, d->kw, d->stride, d->pad) &&
        (size_t)WGRAD_SMALL_BLOCKS * d->Co * d->Ci * d->kh * d->kw <= ex_bwd_slab_floats(d, g)) {
        VPX_CHECK_HIP(launch_wgrad_small(dy, x, d->N, d->H, d->W, d->Co, d->Ci, d->kh, d->pad, slabs, dw, stream));
    } else if (dw) {
        if (wsp) {   // both operands once more in the split format (dy: unless the LeakyReLU' pass or the data gradient already wrote it)
            if (!have_sp) { VPX_CHECK_HIP(launch_split_convert(dy, dy_sp, (long long)d->N * g.Ho * g.Wo, d->Co, stream)); have_sp = true; }
            if (x_split) x_sp = reinterpret_cast<char*>(const_cast<void*>(x_split));   // the caller kept the forward's copy
            else VPX_CHECK_HIP(launch_split_convert(x, x_sp, (long long)d->N * d->H * d->W, d->Ci, stream));
        }
        const size_t slab_floats = ex_bwd_slab_floats(d, g);
        if (!d->transposed)  // dW[co][ci][ky][kx] = sum dy[b,oy,ox,co] x[b, s*oy + ky - p, s*ox + kx - p, ci]
            rc = strided_wgrad(stream, d->precision, d->N, g.Ho, g.Wo, dy, d->Co, d->H, d->W, x, d->Ci, d->kh, d->kw, d->stride, d->pad, slabs, dw,
                               wsp ? dy_sp : nullptr, x_sp, slab_floats);
        else                 // dW[ci][co][ky][kx] = sum x[b,i,j,ci] dy[b, s*i + ky - p, s*j + kx - p, co]
            rc = strided_wgrad(stream, d->precision, d->N, d->H, d->W, x, d->Ci, g.Ho, g.Wo, dy, d->Co, d->kh, d->kw, d->stride, d->pad, slabs, dw,
                               x_sp, wsp ? dy_sp : nullptr, slab_floats);
        if (rc != VPX_OK) return rc;
    }
    return VPX_OK;
}

}  // extern "C"
