// vpx_api.hip — the extern "C" boundary of libvpx_hip.so (declared in include/vpx.h).
// Host-side orchestration only: plan building, workspace carving, per-timestep launches on the caller's stream.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "vpx_host.h"

namespace vpx {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- workspace accounting (vpx_internal.h) ----
static thread_local Carver* g_carver = nullptr;
static thread_local char g_ws_violation[256] = "";

Carver::Carver(void* workspace, size_t bytes)
    : base((char*)workspace), off((256 - ((uintptr_t)workspace & 255)) & 255), cap(bytes), nslot(0), over(false), prev(g_carver) {
    if (off > cap) over = true;
    if (!prev) c5_drop_pending_packs();   // (outermost carver of a call: nothing queued by an earlier call survives)
    g_carver = this;
    g_ws_violation[0] = 0;
}
Carver::~Carver() { g_carver = prev; }

const char* ws_violation() { return g_ws_violation; }
void ws_violation_clear() { g_ws_violation[0] = 0; }

bool ws_write_ok(const void* dst_, size_t bytes, const char* what) {
    const char* dst = (const char*)dst_;
    for (const Carver* c = g_carver; c; c = c->prev) {
        if (dst < c->base || dst >= c->base + c->cap) continue;   // not in this call's workspace: the caller's own tensor
        const char* end = c->base + c->cap;
        size_t room = (size_t)(end - dst);
        for (int i = 0; i < c->nslot; ++i)
            if (dst >= c->slot[i].p && dst < c->slot[i].p + c->slot[i].n) { room = (size_t)(c->slot[i].p + c->slot[i].n - dst); break; }
        if (bytes <= room) return true;
        snprintf(g_ws_violation, sizeof(g_ws_violation), "%s: %zu bytes do not fit the %zu bytes carved for them (workspace sizing rule and launch disagree)",
                 what, bytes, room);
        return false;
    }
    return true;
}

int g_dry_run = 0;
int g_deterministic = 0;
// the kernel-selection options at their defaults; vpx_set_option is their only writer
int g_cell3_mode = 1;
int g_cell2_mode = 1;
int g_experiment = 0;
int g_mfma_shape = 1;   // measured (tools/ab_shape.py, B=128, one process, interleaved): 1.05-1.11x per fused step, every block shape

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_version(void) { return VPX_VERSION; }
static int g_option_epoch = 0;
int vpx_option_epoch(void) { return g_option_epoch; }
int vpx_set_deterministic(int on) { const int prev = vpx::g_deterministic; vpx::g_deterministic = on ? 1 : 0; ++g_option_epoch; return prev; }
const char* vpx_last_error(void) { return g_err; }
int vpx_set_option(int option, int value) {
    ++g_option_epoch;
    if (option == VPX_OPT_CELL2) {
        const int prev = g_cell2_mode;
        vpx::g_cell2_mode = value < 0 ? 0 : (value > 2 ? 2 : value);
        return prev;
    }
    if (option == VPX_OPT_EXPERIMENT) {
        const int prev = vpx::g_experiment;
        vpx::g_experiment = value;
        return prev;
    }
    if (option == VPX_OPT_MFMA_SHAPE) {
        const int prev = g_mfma_shape;
        vpx::g_mfma_shape = value ? 1 : 0;
        return prev;
    }
    if (option == VPX_OPT_DRY_RUN) {
        const int prev = vpx::g_dry_run;
        vpx::g_dry_run = value ? 1 : 0;
        return prev;
    }
    if (option == VPX_OPT_CELL3) {
        const int prev = g_cell3_mode;
        vpx::g_cell3_mode = value ? 1 : 0;
        return prev;
    }
    set_error("vpx_set_option: unknown option %d", option);
    return VPX_ERR_ARG;
}

int vpx_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst || N < 1 || C < 1 || H < 1 || W < 1) { set_error("vpx_nchw_to_nhwc: bad argument"); return VPX_ERR_ARG; }
    VPX_CHECK_HIP(launch_nchw_to_nhwc(src, dst, N, C, H, W, (hipStream_t)stream));
    return VPX_OK;
}
int vpx_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst || N < 1 || C < 1 || H < 1 || W < 1) { set_error("vpx_nhwc_to_nchw: bad argument"); return VPX_ERR_ARG; }
    VPX_CHECK_HIP(launch_nhwc_to_nchw(src, dst, N, C, H, W, (hipStream_t)stream));
    return VPX_OK;
}

int vpx_split_convert(const float* x, void* x_split, long long n_pixels, int C, void* stream) {
    if (!x || !x_split || n_pixels < 0 || C < 8 || (C & 7)) { set_error("vpx_split_convert: NULL tensor or channel count %d not a multiple of 8", C); return VPX_ERR_ARG; }
    VPX_CHECK_HIP(launch_split_convert(x, x_split, n_pixels, C, (hipStream_t)stream));
    return VPX_OK;
}

/* ---- plain conv ------------------------------------------------------------------------------------------------ */
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

int vpx_conv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Ci,
                        int Co, int kh, int kw, int precision, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!x || !w || !y || N < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1 || !(kh & 1) || !(kw & 1) || kh > 7 || kw > 7) {
        set_error("vpx_conv2d_nhwc_fwd: bad argument");
        return VPX_ERR_ARG;
    }
    if ((precision < VPX_PREC_F32 || precision > VPX_PREC_BF16)) { set_error("vpx_conv2d_nhwc_fwd: precision %d not implemented", precision); return VPX_ERR_UNSUPPORTED; }
    hipStream_t stream = (hipStream_t)stream_;
    ConvPlan P{};
    int chunks = 0;
    const int segC[1] = {Ci};
    P.nstage = build_stages(P.stage, &chunks, segC, 1, kh * kw, pick_stage_channels(segC, 1, kh, kw, 4, precision), precision);
    if (P.nstage < 0) { set_error("vpx_conv2d_nhwc_fwd: too many channel stages"); return VPX_ERR_UNSUPPORTED; }
    const int n_tiles = plain_tiles(Co);
    if (!workspace || workspace_bytes < vpx_conv2d_workspace_bytes(Ci, Co, kh, kw)) {
        set_error("vpx_conv2d_nhwc_fwd: workspace too small");
        return VPX_ERR_WORKSPACE;
    }
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
    P.nseg = 1;
    P.seg[0] = ConvSeg{x, (long long)H * W * Ci, Ci, 0};
    P.chunks_total = chunks; P.prec = precision;
    P.a_bytes = conv_a_bytes(P.stage, P.nstage, kh, kw);
    P.wpk = wpk;
    PlainEpiArgs ea{};
    ea.bias = bias; ea.Co = Co; ea.split = Co; ea.ng = plain_groups(Co);
    ea.out0 = y; ea.bstride0 = (long long)H * W * Co; ea.ld0 = Co;
    VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, n_tiles, stream));
    return VPX_OK;
}

}  // extern "C"
