// conv_same_api.hip — plain NHWC stride-1 "same" convolution (include/vpx.h), built from the same implicit-GEMM / weight-gradient
// kernels as the recurrent cells. Host code only.
//   vpx_conv2d_nhwc_fwd / _fwd_ex   y = act(conv(x, w) + bias [+ y])
//   vpx_conv2d_nhwc_bwd             dx = conv^T(dy, w) (transposed + tap-flipped packing), dw = wgrad(dy, x), db = colsum(dy)
#include "vpx_host.h"
using namespace vpx;

namespace {
bool same_args_ok(const void* x, const void* w, const void* y, int N, int H, int W, int Ci, int Co, int kh, int kw) {
    return x && w && y && N >= 1 && H >= 1 && W >= 1 && Ci >= 1 && Co >= 1 && (kh & 1) && (kw & 1) && kh <= 7 && kw <= 7;
}
bool same_prec_ok(int precision) { return precision >= VPX_PREC_F32 && precision <= VPX_PREC_BF16; }

// the backward's workspace: ONE list of slots, taken by the call's Carver and by the size query's CarveMeasure
struct SameBwdSlots { float *wpk, *slabs, *db_part; int slice_cap; };
template <class WS>
void carve_same_bwd(WS& ws, int N, int H, int W, int Ci, int Co, int kh, int kw, SameBwdSlots& s) {
    s.wpk = ws.take(plain_conv_wpk_floats(Co, Ci, kh, kw));
    s.slice_cap = wgrad_slices_for(N, H, W, Co, Ci, kh, kw);
    s.slabs = ws.take((size_t)s.slice_cap * kh * kw * Co * Ci);
    s.db_part = ws.take((size_t)COLSUM_BLOCKS * Co);
}
}  // namespace

extern "C" {
size_t vpx_conv2d_workspace_bytes(int Ci, int Co, int kh, int kw) {
    if (Ci < 1 || Co < 1 || kh < 1 || kw < 1) return 0;
    ConvStage st[MAX_STAGE];
    int chunks = 0;
    const int segC[1] = {Ci};
    // one query serves vpx_conv2d_nhwc_fwd (stage size of the 4-group tile) and vpx_conv2d_nhwc_fwd_ex (plain_conv: stage size of
    // the tiling it picks) in every operand mode: the larger of the two packs. (Round 4 sized only the first — the 5x5 layers
    // with <= 32 outputs of the TrajGRU flow generator then packed 4 % more than the workspace held.)
    size_t best = plain_conv_wpk_floats(Ci, Co, kh, kw) * 4;
    for (int prec = VPX_PREC_F32; prec <= VPX_PREC_BF16; ++prec) {
        if (build_stages(st, &chunks, segC, 1, kh * kw, pick_stage_channels(segC, 1, kh, kw, 4, prec), prec) < 0) return 0;
        const size_t b = packed_weight_bytes(plain_tiles(Co), chunks, plain_groups(Co), prec);
        if (b > best) best = b;
    }
    return align256(best) + 256;
}
int vpx_conv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Ci, int Co, int kh, int kw, int precision,
                        void* workspace, size_t workspace_bytes, void* stream_) {
    if (!same_args_ok(x, w, y, N, H, W, Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_fwd: bad argument"); return VPX_ERR_ARG; }
    if (!same_prec_ok(precision)) { set_error("vpx_conv2d_nhwc_fwd: precision %d not implemented", precision); return VPX_ERR_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)stream_;
    ConvPlan P{};
    int chunks = 0;
    const int segC[1] = {Ci}, n_tiles = plain_tiles(Co);
    P.nstage = build_stages(P.stage, &chunks, segC, 1, kh * kw, pick_stage_channels(segC, 1, kh, kw, 4, precision), precision);
    if (P.nstage < 0) { set_error("vpx_conv2d_nhwc_fwd: too many channel stages"); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(packed_weight_bytes(n_tiles, chunks, plain_groups(Co), precision) / sizeof(float));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_nhwc_fwd");
    PackDesc pd{};
    pd.seg[0] = PackSeg{w, (long long)Ci * kh * kw, kh * kw, 0, Ci};
    memcpy(pd.stage, P.stage, sizeof(ConvStage) * P.nstage);
    pd.nstage = P.nstage; pd.chunks_total = chunks; pd.prec = precision; pd.taps = kh * kw;
    fill_plain_pack(pd, Co, 0);
    VPX_CHECK_HIP(launch_pack_weights(pd, wpk, stream));
    P.B = N; P.H = H; P.W = W; P.kh = kh; P.kw = kw;
    P.tiles_x = (W + TILE_W - 1) / TILE_W; P.tiles_y = (H + TILE_H - 1) / TILE_H;
    P.nseg = 1; P.seg[0] = ConvSeg{x, (long long)H * W * Ci, Ci, 0};
    P.chunks_total = chunks; P.prec = precision; P.a_bytes = conv_a_bytes(P.stage, P.nstage, kh, kw); P.wpk = wpk;
    PlainEpiArgs ea{};
    ea.bias = bias; ea.Co = Co; ea.split = Co; ea.ng = plain_groups(Co);
    ea.out0 = y; ea.bstride0 = (long long)H * W * Co; ea.ld0 = Co;
    VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, n_tiles, stream));
    return VPX_OK;
}
/* y = act(conv(x, w) + bias [+ y]): stride-1 "same" convolution with an optional accumulate into the destination (a second
 * convolution summed into the same output, e.g. TrajGRU's i2f + h2f, traj_gru.py:134-142) and LeakyReLU on the sum. */
int vpx_conv2d_nhwc_fwd_ex(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Ci, int Co, int kh, int kw, int precision,
                           int accumulate, float leaky_slope, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!same_args_ok(x, w, y, N, H, W, Ci, Co, kh, kw) || leaky_slope < 0.0f) { set_error("vpx_conv2d_nhwc_fwd_ex: bad argument"); return VPX_ERR_ARG; }
    if (!same_prec_ok(precision)) { set_error("vpx_conv2d_nhwc_fwd_ex: precision %d not implemented", precision); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_fwd_ex: workspace too small"); return VPX_ERR_WORKSPACE; }
    const ConvGeo g{N, H, W};
    Carver ws(workspace, workspace_bytes);
    float* wpk = ws.take(plain_conv_pack_floats(precision, g, Ci, kh, kw, Co));
    VPX_CHECK_CARVE(ws, "vpx_conv2d_nhwc_fwd_ex");
    return plain_conv((hipStream_t)stream_, precision, g, x, Ci, Ci, w, (long long)Ci * kh * kw, kh * kw, kh, kw, Co, false, bias, y, Co,
                      accumulate != 0, wpk, leaky_slope);
}
size_t vpx_conv2d_bwd_workspace_bytes(int N, int H, int W, int Ci, int Co, int kh, int kw) {
    if (N < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1) return 0;
    CarveMeasure m; SameBwdSlots s{};
    carve_same_bwd(m, N, H, W, Ci, Co, kh, kw, s);
    return m.off + 512;
}
int vpx_conv2d_nhwc_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int N, int H, int W, int Ci, int Co, int kh, int kw,
                        int precision, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!same_args_ok(x, w, dy, N, H, W, Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_bwd: bad argument"); return VPX_ERR_ARG; }
    if (!same_prec_ok(precision)) { set_error("vpx_conv2d_nhwc_bwd: precision %d not implemented", precision); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < vpx_conv2d_bwd_workspace_bytes(N, H, W, Ci, Co, kh, kw)) { set_error("vpx_conv2d_nhwc_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    SameBwdSlots s{};
    carve_same_bwd(ws, N, H, W, Ci, Co, kh, kw, s);
    VPX_CHECK_CARVE(ws, "vpx_conv2d_nhwc_bwd");
    const ConvGeo g{N, H, W};
    int rc;
    if (dx && (rc = plain_conv(stream, precision, g, dy, Co, Co, w, (long long)Ci * kh * kw, kh * kw, kh, kw, Ci, true, nullptr, dx, Ci, false, s.wpk))) return rc;
    if (dw && (rc = plain_wgrad(stream, precision, g, dy, Co, x, Ci, kh, kw, s.slabs, dw, nullptr, s.slice_cap))) return rc;
    if (db) VPX_CHECK_HIP(launch_colsum(dy, nullptr, 0.f, nullptr, db, s.db_part, (long long)N * H * W, Co, stream));
    return VPX_OK;
}
}  // extern "C"
