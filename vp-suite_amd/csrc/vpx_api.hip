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
int g_seq_chains = 1;   // (convlstm_fwd_api.hip, seq_chains; the measurements behind the default and its batch floor: DESIGN.md §4)
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
    if (option == VPX_OPT_SEQ_CHAINS) {
        const int prev = g_seq_chains;
        vpx::g_seq_chains = value < 0 ? 0 : (value > 2 ? 2 : value);
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

}  // extern "C"
