// groupnorm.hip — GroupNorm(G, C) with per-channel affine, optional LeakyReLU and optional residual, forward and backward, on NHWC
// fp32 (DCGANConv / DCGANConvTranspose of vp_suite/model_blocks/conv.py: GroupNorm(16, C) + LeakyReLU(0.2); the PhyCell's
// GroupNorm(7, 49) in vp_suite/model_blocks/phydnet.py, no activation).
//
// A group of one sample is HW * cpg floats, cpg = C / G contiguous channels per pixel: 64-128 KB per sample at the PhyDNet shapes,
// so the op is bound by launch count and latency, not by HBM. One workgroup per (sample, group) does the whole forward in one
// launch: thread t owns channel t % cpg of the group and every R-th pixel (R = 256 / cpg rows), sums run per thread in a fixed pixel
// order and then as an LDS tree (deterministic), the variance is the exact two-pass one. The backward recomputes x̂ from x and the
// saved (mean, 1/std); dγ / dβ go through per-sample partials in the workspace and a fixed-order reduce over the batch (no atomics).
#include "vpx_host.h"

namespace vpx {

constexpr int GN_THREADS = 256;
constexpr float GN_EPS = 1e-5f;

struct GNArgs {
    const float* x; const float* gamma; const float* beta; const float* r;
    float* y; float* stats;
    const float* dy; float* dx; float* part;   // backward: part [2][N][C] (dγ partials, then dβ partials) or null
    int N, HW, C, G, act;
    float slope;
};

// sum of v over the workgroup; every thread gets the result. `red` is reused: the trailing barrier frees it for the next call
__device__ __forceinline__ float gn_block_sum(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = GN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(GN_THREADS) void gn_fwd_kernel(const GNArgs a) {
    __shared__ float red[GN_THREADS];
    const int n = blockIdx.x / a.G, g = blockIdx.x - n * a.G;
    const int cpg = a.C / a.G, R = GN_THREADS / cpg, t = threadIdx.x;
    const bool on = t < R * cpg;
    const int c = g * cpg + t % cpg, row = t / cpg;
    const size_t base = (size_t)n * a.HW * a.C + c;
    const float inv_m = 1.0f / (float)(a.HW * cpg);
    float s = 0.f;
    if (on) for (int p = row; p < a.HW; p += R) s += a.x[base + (size_t)p * a.C];
    const float mean = gn_block_sum(s, red) * inv_m;
    float q = 0.f;
    if (on) for (int p = row; p < a.HW; p += R) { const float d = a.x[base + (size_t)p * a.C] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(gn_block_sum(q, red) * inv_m + GN_EPS);
    if (t == 0) { a.stats[2 * blockIdx.x] = mean; a.stats[2 * blockIdx.x + 1] = rstd; }
    if (!on) return;
    const float gm = a.gamma[c], bt = a.beta[c];
    for (int p = row; p < a.HW; p += R) {
        const size_t e = base + (size_t)p * a.C;
        float z = (a.x[e] - mean) * rstd * gm + bt;
        if (a.act) z = z > 0.f ? z : z * a.slope;
        a.y[e] = a.r ? z + a.r[e] : z;
    }
}

__global__ __launch_bounds__(GN_THREADS) void gn_bwd_kernel(const GNArgs a) {
    __shared__ float red[GN_THREADS];
    const int n = blockIdx.x / a.G, g = blockIdx.x - n * a.G;
    const int cpg = a.C / a.G, R = GN_THREADS / cpg, t = threadIdx.x;
    const bool on = t < R * cpg;
    const int c = g * cpg + t % cpg, row = t / cpg;
    const size_t base = (size_t)n * a.HW * a.C + c;
    const float mean = a.stats[2 * blockIdx.x], rstd = a.stats[2 * blockIdx.x + 1];
    const float gm = on ? a.gamma[c] : 0.f, bt = on ? a.beta[c] : 0.f;
    float s1 = 0.f, s2 = 0.f, pg = 0.f, pb = 0.f;
    if (on) {
        for (int p = row; p < a.HW; p += R) {
            const size_t e = base + (size_t)p * a.C;
            const float xh = (a.x[e] - mean) * rstd;
            float dz = a.dy[e];
            if (a.act && !(xh * gm + bt > 0.f)) dz *= a.slope;   // LeakyReLU' from the sign of the (recomputed) pre-activation
            const float dxh = dz * gm;
            s1 += dxh; s2 += dxh * xh; pg += dz * xh; pb += dz;
        }
    }
    const float inv_m = 1.0f / (float)(a.HW * cpg);
    const float m1 = gn_block_sum(s1, red) * inv_m;
    const float m2 = gn_block_sum(s2, red) * inv_m;
    if (a.part) {   // per-channel partials of this sample: thread c of the group sums its channel's R rows in row order
        for (int k = 0; k < 2; ++k) {
            red[t] = k ? pb : pg;
            __syncthreads();
            if (t < cpg) {
                float acc = 0.f;
                for (int r = 0; r < R; ++r) acc += red[r * cpg + t];
                a.part[(size_t)k * a.N * a.C + (size_t)n * a.C + g * cpg + t] = acc;
            }
            __syncthreads();
        }
    }
    if (!on) return;
    for (int p = row; p < a.HW; p += R) {
        const size_t e = base + (size_t)p * a.C;
        const float xh = (a.x[e] - mean) * rstd;
        float dz = a.dy[e];
        if (a.act && !(xh * gm + bt > 0.f)) dz *= a.slope;
        a.dx[e] = rstd * (dz * gm - m1 - xh * m2);
    }
}

// dγ[c] = Σ_n part[0][n][c], dβ[c] = Σ_n part[1][n][c], n ascending
__global__ void gn_param_reduce_kernel(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int n = 0; n < N; ++n) { sg += part[(size_t)n * C + c]; sb += part[(size_t)N * C + (size_t)n * C + c]; }
    dgamma[c] = sg;
    dbeta[c] = sb;
}

static int gn_check_shape(const char* who, int N, int HW, int C, int G) {
    if (N < 1 || HW < 1 || C < 1 || G < 1 || C % G != 0 || C / G > GN_THREADS) {
        set_error("%s: bad shape (N=%d HW=%d C=%d G=%d; C must be a multiple of G with at most %d channels per group)", who, N, HW, C, G,
                  GN_THREADS);
        return VPX_ERR_ARG;
    }
    if ((long long)N * G > 0x7fffffffLL) { set_error("%s: N*G too large", who); return VPX_ERR_ARG; }
    return VPX_OK;
}

// The backward's workspace (only a call that wants dgamma / dbeta has one): their per-image partial sums, [2][N][C]
struct GnBwdSlots { float* part; size_t part_floats; };
template <class WS>
static void carve_groupnorm_bwd(WS& ws, int N, int C, GnBwdSlots& s) {
    s.part_floats = (size_t)2 * N * C;
    s.part = ws.take(s.part_floats);
}

}  // namespace vpx

extern "C" {

int vpx_groupnorm_fwd(const float* x, const float* gamma, const float* beta, const float* r, float* y, float* stats, int N, int HW, int C,
                      int G, int act, float slope, void* stream) {
    using namespace vpx;
    if (!x || !gamma || !beta || !y || !stats) { set_error("vpx_groupnorm_fwd: NULL argument"); return VPX_ERR_ARG; }
    if (int rc = gn_check_shape("vpx_groupnorm_fwd", N, HW, C, G)) return rc;
    GNArgs a{};
    a.x = x; a.gamma = gamma; a.beta = beta; a.r = r; a.y = y; a.stats = stats;
    a.N = N; a.HW = HW; a.C = C; a.G = G; a.act = act ? 1 : 0; a.slope = slope;
    VPX_LAUNCH(gn_fwd_kernel, dim3((unsigned)(N * G)), dim3(GN_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

size_t vpx_groupnorm_bwd_workspace_bytes(int N, int C) {
    if (N < 1 || C < 1) return 0;
    vpx::CarveMeasure m; vpx::GnBwdSlots s{};
    vpx::carve_groupnorm_bwd(m, N, C, s);
    return m.off + 256;
}

int vpx_groupnorm_bwd(const float* x, const float* stats, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                      float* dbeta, int N, int HW, int C, int G, int act, float slope, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace vpx;
    if (!x || !stats || !gamma || !beta || !dy || !dx || (!dgamma) != (!dbeta)) {
        set_error("vpx_groupnorm_bwd: NULL argument (dgamma and dbeta: both or neither)");
        return VPX_ERR_ARG;
    }
    if (int rc = gn_check_shape("vpx_groupnorm_bwd", N, HW, C, G)) return rc;
    GNArgs a{};
    a.x = x; a.gamma = gamma; a.beta = beta; a.dy = dy; a.dx = dx;
    a.stats = const_cast<float*>(stats);   // (only read by the backward kernel)
    a.N = N; a.HW = HW; a.C = C; a.G = G; a.act = act ? 1 : 0; a.slope = slope;
    if (dgamma) {
        if (!workspace || workspace_bytes < vpx_groupnorm_bwd_workspace_bytes(N, C)) {
            set_error("vpx_groupnorm_bwd: workspace too small");
            return VPX_ERR_WORKSPACE;
        }
        Carver ws(workspace, workspace_bytes);
        GnBwdSlots sl{};
        carve_groupnorm_bwd(ws, N, C, sl);
        VPX_CHECK_CARVE(ws, "vpx_groupnorm_bwd");
        a.part = sl.part;
        if (!ws_write_ok(a.part, sl.part_floats * sizeof(float), "vpx_groupnorm_bwd partials")) {
            set_error("%s", ws_violation());
            ws_violation_clear();
            return VPX_ERR_WORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    VPX_LAUNCH(gn_bwd_kernel, dim3((unsigned)(N * G)), dim3(GN_THREADS), 0, s, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    if (dgamma) {
        VPX_LAUNCH(gn_param_reduce_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, s, a.part, dgamma, dbeta, N, C);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

}  // extern "C"
