// Training tail of the hot path's caller: the prediction loss with its gradient in one pass, and
// one Adam update over the flat parameter / gradient buckets. Both are streaming, HBM-bound kernels.
//   vpx_mse_loss      MSE summed over (c,h,w), averaged over frames (t) then samples (b):
//                     vp_suite/base/base_measure.py:55-57 with nn.MSELoss(reduction="none") (measure/image_wise.py:25),
//                     scaled and summed by PredictionLossProvider.get_losses (measure/loss_provider.py:48-51)
//   vpx_adam_step     torch.optim.Adam(params, lr) as constructed in vp_suite/vpsuite.py:353 (betas 0.9/0.999, eps 1e-8,
//                     no weight decay, no amsgrad), called once per iteration at base_model.py:176
//   vpx_grad_stats / vpx_adam_step_clipped   no counterpart in the reference: norm / max / non-finite count of the flat gradient in
//                     one deterministic pass, and the same Adam update reading that result on the device — norm clipping
//                     (torch.nn.utils.clip_grad_norm_'s coefficient), value clipping (clip_grad_value_) and an optional skip of a
//                     non-finite step, without a host round trip or another pass over the gradient. A skipped step still
//                     advances the caller's step count: the bias corrections are host scalars of that count.
#include <hip/hip_runtime.h>
#include <math.h>
#include "vpx_internal.h"
#include "vpx_host.h"

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MSE_THREADS = 256;
constexpr int MSE_MAX_BLOCKS = 1024;

// grad (optional) = 2 * scale / n_frames * (pred - target); partial[block] = sum (pred - target)^2 in double
__global__ __launch_bounds__(MSE_THREADS) void mse_partial_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ target, long long n,
                                                                  float gscale, float* __restrict__ grad,
                                                                  double* __restrict__ partial) {
    __shared__ double red[MSE_THREADS / 64];
    double acc = 0.0;
    const long long stride = (long long)gridDim.x * MSE_THREADS * 4;
    const bool vec = (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad) & 15) == 0;
    for (long long e = ((long long)blockIdx.x * MSE_THREADS + threadIdx.x) * 4; e < n; e += stride) {
        if (vec && e + 3 < n) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(pred + e);
            const f32x4 t = *reinterpret_cast<const f32x4*>(target + e);
            f32x4 d;
#pragma unroll
            for (int k = 0; k < 4; ++k) { d[k] = p[k] - t[k]; acc += (double)d[k] * d[k]; d[k] *= gscale; }
            if (grad) *reinterpret_cast<f32x4*>(grad + e) = d;
        } else {
            for (long long k = e; k < n && k < e + 4; ++k) {
                const float d = pred[k] - target[k];
                acc += (double)d * d;
                if (grad) grad[k] = d * gscale;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < MSE_THREADS / 64; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

// loss = scale / n_frames * sum(partial): one wave, fixed summation order (deterministic)
__global__ void mse_final_kernel(const double* __restrict__ partial, int nblocks, double mult, float* __restrict__ loss) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64) acc += partial[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) *loss = (float)(acc * mult);
}

constexpr int GS_THREADS = 256;
constexpr int GS_MAX_BLOCKS = 1024;

static __device__ __forceinline__ bool gs_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// partial[3 b .. 3 b + 2] = sum g^2 (a float x float product is exact in double), max |g| over the finite elements, number of
// non-finite elements — of block b's share of grad. A non-finite element goes into the sum as it is: the sum is then inf or NaN.
__global__ __launch_bounds__(GS_THREADS) void grad_stats_partial_kernel(const float* __restrict__ grad, long long n,
                                                                        double* __restrict__ partial) {
    __shared__ double red[3][GS_THREADS / 64];
    double acc = 0.0, bad = 0.0;
    float mx = 0.0f;
    const long long stride = (long long)gridDim.x * GS_THREADS * 4;
    const bool vec = ((uintptr_t)grad & 15) == 0;
    for (long long e = ((long long)blockIdx.x * GS_THREADS + threadIdx.x) * 4; e < n; e += stride) {
        if (vec && e + 3 < n) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(grad + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc += (double)g[k] * g[k];
                if (gs_finite(g[k])) mx = fmaxf(mx, fabsf(g[k])); else bad += 1.0;
            }
        } else {
            for (long long k = e; k < n && k < e + 4; ++k) {
                const float g = grad[k];
                acc += (double)g * g;
                if (gs_finite(g)) mx = fmaxf(mx, fabsf(g)); else bad += 1.0;
            }
        }
    }
    double dmx = (double)mx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        bad += __shfl_down(bad, off, 64);
        dmx = fmax(dmx, __shfl_down(dmx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = acc; red[1][threadIdx.x >> 6] = dmx; red[2][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, m = 0.0, c = 0.0;
        for (int w = 0; w < GS_THREADS / 64; ++w) { s += red[0][w]; m = fmax(m, red[1][w]); c += red[2][w]; }
        partial[3 * blockIdx.x] = s; partial[3 * blockIdx.x + 1] = m; partial[3 * blockIdx.x + 2] = c;
    }
}

// stats[0] = sqrt(grad_scale^2 * sum), stats[1] = grad_scale * max, stats[2] = count: one wave, fixed order (deterministic).
// stats[3] (the skipped-step count of adam_kernel) is left alone.
__global__ void grad_stats_final_kernel(const double* __restrict__ partial, int nblocks, double grad_scale, double* __restrict__ stats) {
    double acc = 0.0, mx = 0.0, bad = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64) { acc += partial[3 * i]; mx = fmax(mx, partial[3 * i + 1]); bad += partial[3 * i + 2]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        bad += __shfl_down(bad, off, 64);
        mx = fmax(mx, __shfl_down(mx, off, 64));
    }
    if (threadIdx.x == 0) { stats[0] = sqrt(acc * (grad_scale * grad_scale)); stats[1] = grad_scale * mx; stats[2] = bad; }
}

struct AdamArgs {
    float* p; const float* g; float* m; float* v;
    long long n;
    // scalars are prepared in double on the host exactly as torch/optim/adam.py does in Python floats, then rounded once
    float beta1, beta2, omb1, omb2;      // beta, 1 - beta
    float step_size, bc2_sqrt, eps;      // lr / (1 - beta1^t), sqrt(1 - beta2^t)
    float weight_decay, grad_scale;
};

// What vpx_adam_step_clipped adds to the update; read on the device, so the caller never waits for the statistics.
struct ClipArgs {
    double* stats;            // vpx_grad_stats's result (nullable: value clipping alone needs none); [3] counts the skipped steps
    double grad_scale, max_norm;
    float clip_value;
    int skip_nonfinite;
};

// torch.optim.Adam single-tensor update (torch/optim/adam.py _single_tensor_adam, amsgrad = False, maximize = False):
//   g += wd * p ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// MODE 0: vpx_adam_step, g = grad * grad_scale. MODE 1: the factor is s = (float)(grad_scale * c) with clip_grad_norm_'s coefficient
// c = min(1, max_norm / (stats[0] + 1e-6)) formed in double from the device value (1 without max_norm), and a step whose gradient
// holds a non-finite element (stats[2] > 0) is left out on request: every thread returns before its first store and one thread
// counts the step in stats[3]. MODE 2: additionally g is clamped to +-clip_value (NaN stays NaN, as torch.clamp) before the weight
// decay. With c = 1 and nothing skipped, s == (float)grad_scale and MODE 1 runs MODE 0's arithmetic on MODE 0's values: same bits.
template <int MODE>
__global__ __launch_bounds__(256) void adam_kernel(const AdamArgs a, const ClipArgs c) {
    const long long stride = (long long)gridDim.x * 256 * 4;
    const float step_size = a.step_size;
    float gs = a.grad_scale;
    if constexpr (MODE != 0) {
        if (c.stats) {
            if (c.skip_nonfinite && c.stats[2] > 0.0) {
                if (blockIdx.x == 0 && threadIdx.x == 0) c.stats[3] = c.stats[3] + 1.0;
                return;
            }
            if (c.max_norm > 0.0) {
                const double r = c.max_norm / (c.stats[0] + 1e-6);
                gs = (float)(c.grad_scale * (r > 1.0 ? 1.0 : r));   // (a NaN norm gives a NaN factor, as torch.clamp(max=1) does)
            }
        }
    }
    auto clamp = [&](float g) -> float {
        if constexpr (MODE == 2) return g > c.clip_value ? c.clip_value : (g < -c.clip_value ? -c.clip_value : g);
        else return g;
    };
    for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < a.n; e += stride) {
        if (e + 3 < a.n) {  // the buckets are 256-byte aligned allocations: vector path
            f32x4 p = *reinterpret_cast<const f32x4*>(a.p + e);
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.g + e);
            f32x4 m = *reinterpret_cast<const f32x4*>(a.m + e);
            f32x4 v = *reinterpret_cast<const f32x4*>(a.v + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float g = clamp(g4[k] * gs);
                if (a.weight_decay != 0.0f) g += a.weight_decay * p[k];
                m[k] = a.beta1 * m[k] + a.omb1 * g;
                v[k] = a.beta2 * v[k] + a.omb2 * g * g;
                const float denom = sqrtf(v[k]) / a.bc2_sqrt + a.eps;
                p[k] -= step_size * (m[k] / denom);
            }
            *reinterpret_cast<f32x4*>(a.p + e) = p;
            *reinterpret_cast<f32x4*>(a.m + e) = m;
            *reinterpret_cast<f32x4*>(a.v + e) = v;
        } else {
            for (long long k = e; k < a.n; ++k) {
                float g = clamp(a.g[k] * gs);
                if (a.weight_decay != 0.0f) g += a.weight_decay * a.p[k];
                const float m = a.beta1 * a.m[k] + a.omb1 * g;
                const float v = a.beta2 * a.v[k] + a.omb2 * g * g;
                a.m[k] = m; a.v[k] = v;
                a.p[k] -= step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
            }
        }
    }
}

// the arguments both Adam entry points refuse, and the scalars of the update as torch forms them
static int adam_prepare(const char* who, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale, AdamArgs& a) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n < 1 || step < 1) { set_error("%s: bad argument", who); return VPX_ERR_ARG; }
    if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) {
        set_error("%s: buckets must be 16-byte aligned", who);
        return VPX_ERR_ARG;
    }
    a = AdamArgs{param, grad, exp_avg, exp_avg_sq, n, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                 (float)(lr / (1.0 - pow(beta1, step))), (float)sqrt(1.0 - pow(beta2, step)), (float)eps,
                 (float)weight_decay, (float)grad_scale};
    return VPX_OK;
}

static unsigned adam_blocks(long long n) {
    long long blocks = (n + 1023) / 1024;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

// The reductions' workspaces: per-workgroup partial sums in double (take() counts floats: a double is two). The queries have no size
// argument, so the slot holds the block cap's worth whatever n is; `blocks` is what this n launches.
struct TailSlots { double* partial; long long blocks; };
template <class WS>
static void carve_mse(WS& ws, long long n, TailSlots& s) {
    s.blocks = std::min<long long>((n + MSE_THREADS * 4 - 1) / (MSE_THREADS * 4), MSE_MAX_BLOCKS);
    s.partial = reinterpret_cast<double*>(ws.take((size_t)MSE_MAX_BLOCKS * 2));
}
template <class WS>
static void carve_grad_stats(WS& ws, long long n, TailSlots& s) {
    s.blocks = std::min<long long>((n + GS_THREADS * 4 - 1) / (GS_THREADS * 4), GS_MAX_BLOCKS);
    s.partial = reinterpret_cast<double*>(ws.take((size_t)GS_MAX_BLOCKS * 3 * 2));
}

}  // namespace vpx

using namespace vpx;

extern "C" {

size_t vpx_mse_loss_workspace_bytes(void) {
    CarveMeasure m; TailSlots s{};
    carve_mse(m, 1, s);
    return m.off + 256;
}

int vpx_mse_loss(const float* pred, const float* target, long long n_elements, long long n_frames, float scale, float* loss,
                 float* dpred, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!pred || !target || !loss || n_elements < 1 || n_frames < 1) { set_error("vpx_mse_loss: bad argument"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_mse_loss_workspace_bytes()) { set_error("vpx_mse_loss: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    TailSlots s{};
    carve_mse(ws, n_elements, s);
    VPX_CHECK_CARVE(ws, "vpx_mse_loss");
    const double mult = (double)scale / (double)n_frames;
    VPX_LAUNCH(mse_partial_kernel, dim3((unsigned)s.blocks), dim3(MSE_THREADS), 0, stream, pred, target, n_elements,
                       (float)(2.0 * mult), dpred, s.partial);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(mse_final_kernel, dim3(1), dim3(64), 0, stream, s.partial, (int)s.blocks, mult, loss);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream_) {
    AdamArgs a;
    if (int rc = adam_prepare("vpx_adam_step", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, a)) return rc;
    VPX_LAUNCH(adam_kernel<0>, dim3(adam_blocks(n)), dim3(256), 0, (hipStream_t)stream_, a, ClipArgs{});
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

size_t vpx_grad_stats_workspace_bytes(void) {
    CarveMeasure m; TailSlots s{};
    carve_grad_stats(m, 1, s);
    return m.off + 256;
}

int vpx_grad_stats(const float* grad, long long n, double grad_scale, double* stats, void* workspace, size_t workspace_bytes,
                   void* stream_) {
    if (!grad || !stats || n < 1) { set_error("vpx_grad_stats: bad argument"); return VPX_ERR_ARG; }
    if (((uintptr_t)grad & 3) != 0 || ((uintptr_t)stats & 7) != 0) { set_error("vpx_grad_stats: grad must be 4-byte, stats 8-byte aligned"); return VPX_ERR_ARG; }
    if (!(grad_scale >= 0.0)) { set_error("vpx_grad_stats: grad_scale must not be negative or NaN"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_grad_stats_workspace_bytes()) { set_error("vpx_grad_stats: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    TailSlots s{};
    carve_grad_stats(ws, n, s);
    VPX_CHECK_CARVE(ws, "vpx_grad_stats");
    VPX_LAUNCH(grad_stats_partial_kernel, dim3((unsigned)s.blocks), dim3(GS_THREADS), 0, stream, grad, n, s.partial);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(grad_stats_final_kernel, dim3(1), dim3(64), 0, stream, s.partial, (int)s.blocks, grad_scale, stats);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_adam_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1,
                          double beta2, double eps, double weight_decay, int step, double grad_scale, const double* stats,
                          double max_norm, double clip_value, int skip_nonfinite, void* stream_) {
    AdamArgs a;
    if (int rc = adam_prepare("vpx_adam_step_clipped", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, a)) return rc;
    if (!(grad_scale >= 0.0) || !(max_norm >= 0.0) || !(clip_value >= 0.0)) {
        set_error("vpx_adam_step_clipped: grad_scale, max_norm and clip_value must not be negative or NaN");
        return VPX_ERR_ARG;
    }
    if (!stats && (max_norm > 0.0 || skip_nonfinite)) { set_error("vpx_adam_step_clipped: max_norm and skip_nonfinite need stats"); return VPX_ERR_ARG; }
    if (((uintptr_t)stats & 7) != 0) { set_error("vpx_adam_step_clipped: stats must be 8-byte aligned"); return VPX_ERR_ARG; }
    // (stats is const for the caller's reading of it: the one element the update writes is its own skipped-step count)
    const ClipArgs c{const_cast<double*>(stats), grad_scale, max_norm, (float)clip_value, skip_nonfinite};
    if (clip_value > 0.0) VPX_LAUNCH(adam_kernel<2>, dim3(adam_blocks(n)), dim3(256), 0, (hipStream_t)stream_, a, c);
    else VPX_LAUNCH(adam_kernel<1>, dim3(adam_blocks(n)), dim3(256), 0, (hipStream_t)stream_, a, c);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
