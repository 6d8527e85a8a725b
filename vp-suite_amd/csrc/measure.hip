// Image-wise measures of vp_suite/measure/image_wise.py as streaming kernels whose PER-FRAME results serve every reduction the
// package needs (loss terms, metrics, every prediction horizon of get_metrics(all_frame_cnts=True)):
//   vpx_pixel_measures_fwd / _bwd   per-frame sums of d^2, |d| and smooth-L1(d), d = pred - target: the criteria of MSE, L1, SmoothL1
//                                   (nn.*Loss(reduction="none"), summed over c,h,w by base_measure.py:57) and of PSNR (image_wise.py:69-70)
//   vpx_ssim_fwd / _bwd             per-frame SSIM with piqa's SSIM() defaults (image_wise.py:111-117, base_measure.py:71-74): inputs
//                                   clamp((x+1)/2, 0, 1), 11-tap Gaussian (sigma 1.5), no padding, C1 = 0.01^2, C2 = 0.03^2
// As in train_tail.hip: double partial sums, a fixed-order final reduction, no floating-point atomics — bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include "vpx_internal.h"
#include "vpx_host.h"

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- pixel measures ------------------------------------------------------------------------------------------------------------
constexpr int PM_THREADS = 256;
constexpr int PM_CHUNK = PM_THREADS * 16;   // elements of one frame per workgroup

// the differences are formed in double (exact for fp32 operands); the kernel stays bound by its two reads
__device__ __forceinline__ void pm_accumulate(float p, float t, double& s2, double& s1, double& sh) {
    const double d = (double)p - (double)t, ad = fabs(d);
    s2 += d * d;
    s1 += ad;
    sh += ad < 1.0 ? 0.5 * d * d : ad - 0.5;   // nn.SmoothL1Loss, beta = 1
}

__device__ __forceinline__ double block_sum(double v, double* red) {   // result valid in thread 0; red: PM_THREADS / 64 doubles
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();   // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < PM_THREADS / 64; ++w) s += red[w];
    return s;
}

// workgroup (frame, chunk) -> partial[(frame * chunks + chunk) * 3 + {0: d^2, 1: |d|, 2: smooth-L1}]
__global__ __launch_bounds__(PM_THREADS) void pixel_measures_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                            long long frame_elems, int chunks, double* __restrict__ partial) {
    __shared__ double red[PM_THREADS / 64];
    const long long f = blockIdx.x / chunks;
    const long long start = (long long)(blockIdx.x % chunks) * PM_CHUNK;
    const int n = (int)(frame_elems - start < PM_CHUNK ? frame_elems - start : PM_CHUNK);
    const float* p = pred + f * frame_elems + start;
    const float* t = target + f * frame_elems + start;
    const bool vec = (((uintptr_t)p | (uintptr_t)t) & 15) == 0;   // frames of odd length start unaligned: scalar path
    double s2 = 0.0, s1 = 0.0, sh = 0.0;
    for (int e = threadIdx.x * 4; e < n; e += PM_THREADS * 4) {
        if (vec && e + 3 < n) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + e);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(t + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) pm_accumulate(pv[k], tv[k], s2, s1, sh);
        } else {
            for (int k = e; k < n && k < e + 4; ++k) pm_accumulate(p[k], t[k], s2, s1, sh);
        }
    }
    s2 = block_sum(s2, red);
    s1 = block_sum(s1, red);
    sh = block_sum(sh, red);
    if (threadIdx.x == 0) {
        double* o = partial + (size_t)blockIdx.x * 3;
        o[0] = s2; o[1] = s1; o[2] = sh;
    }
}

// one wave per frame, fixed order: sums[k * n_frames + frame] = sum over the frame's chunks
__global__ void pixel_measures_final_kernel(const double* __restrict__ partial, int chunks, long long n_frames, double* __restrict__ sums) {
    const long long f = blockIdx.x;
    for (int k = 0; k < 3; ++k) {
        double acc = 0.0;
        for (int c = threadIdx.x; c < chunks; c += 64) acc += partial[((size_t)f * chunks + c) * 3 + k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (threadIdx.x == 0) sums[k * n_frames + f] = acc;
    }
}

// dpred = 2 g0[f] d + g1[f] sign(d) + g2[f] clamp(d, -1, 1), g = the cotangents of the three per-frame sums (device memory)
__device__ __forceinline__ float pm_grad(float p, float t, float a, float b, float c) {
    const float d = p - t;
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    return a * d + b * sg + c * fminf(fmaxf(d, -1.0f), 1.0f);
}

__global__ __launch_bounds__(PM_THREADS) void pixel_measures_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                        const float* __restrict__ dsums, long long frame_elems, int chunks,
                                                                        long long n_frames, float* __restrict__ dpred) {
    const long long f = blockIdx.x / chunks;
    const long long start = (long long)(blockIdx.x % chunks) * PM_CHUNK;
    const int n = (int)(frame_elems - start < PM_CHUNK ? frame_elems - start : PM_CHUNK);
    const float* p = pred + f * frame_elems + start;
    const float* t = target + f * frame_elems + start;
    float* g = dpred + f * frame_elems + start;
    const float a = 2.0f * dsums[f], b = dsums[n_frames + f], c = dsums[2 * n_frames + f];
    const bool vec = (((uintptr_t)p | (uintptr_t)t | (uintptr_t)g) & 15) == 0;
    for (int e = threadIdx.x * 4; e < n; e += PM_THREADS * 4) {
        if (vec && e + 3 < n) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + e);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(t + e);
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = pm_grad(pv[k], tv[k], a, b, c);
            *reinterpret_cast<f32x4*>(g + e) = o;
        } else {
            for (int k = e; k < n && k < e + 4; ++k) g[k] = pm_grad(p[k], t[k], a, b, c);
        }
    }
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------
// Tiles are 32 wide: the 32 lanes an LDS read is serviced in read 32 consecutive floats of one row in the vertical passes (rows are
// stored without padding and walked by a flat index, so a lane group that wraps to the next row still reads consecutive words).
constexpr int SS_TAPS = 11, SS_HALO = SS_TAPS - 1;
constexpr int SS_THREADS = 256;
constexpr int SS_TW = 32, SS_TH = 16;                                 // tile: map entries (forward), input pixels (backward)
constexpr int SF_IW = SS_TW + SS_HALO, SF_IH = SS_TH + SS_HALO;       // forward: input tile 42 x 26
constexpr int SB_QW = SS_TW + SS_HALO, SB_QH = SS_TH + SS_HALO;       // backward: map entries whose window holds a pixel of the tile, 42 x 26
constexpr int SB_IW = SB_QW + SS_HALO, SB_IH = SB_QH + SS_HALO;       // ... and the inputs under those windows, 52 x 36
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

struct SsimArgs {
    const float* pred;
    const float* target;
    int H, W, layout, tiles_x, tiles;
    float w[SS_TAPS];
};

__device__ __forceinline__ float ssim_unit(float v) { return fminf(fmaxf((v + 1.0f) * 0.5f, 0.0f), 1.0f); }   // reshape_clamp
__device__ __forceinline__ long long ssim_index(int layout, int H, int W, int c, int y, int x) {           // inside one 3-channel frame
    return layout == VPX_LAYOUT_NCHW ? ((long long)c * H + y) * W + x : ((long long)y * W + x) * 3 + c;
}

// haloed tile of both mapped images; positions outside the image read as 0 (no valid map entry uses them)
__device__ __forceinline__ void ssim_stage(const SsimArgs& a, long long frame, int c, int y0, int x0, int rows, int cols, float* sx, float* sy) {
    const float* p = a.pred + frame * 3 * a.H * a.W;
    const float* t = a.target + frame * 3 * a.H * a.W;
    for (int i = threadIdx.x; i < rows * cols; i += SS_THREADS) {
        const int y = y0 + i / cols, x = x0 + i % cols;
        float xv = 0.0f, yv = 0.0f;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const long long e = ssim_index(a.layout, a.H, a.W, c, y, x);
            xv = ssim_unit(p[e]);
            yv = ssim_unit(t[e]);
        }
        sx[i] = xv;
        sy[i] = yv;
    }
}

// horizontal pass over x, y, xx, yy, xy: hb[k][r * ocols + c] = sum_j w[j] * product_k(r, c + j)
__device__ __forceinline__ void ssim_rows(const SsimArgs& a, const float* sx, const float* sy, int rows, int icols, int ocols, float* hb) {
    const int plane = rows * ocols;
    for (int i = threadIdx.x; i < plane; i += SS_THREADS) {
        const float* rx = sx + (i / ocols) * icols + i % ocols;
        const float* ry = sy + (i / ocols) * icols + i % ocols;
        float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
        for (int j = 0; j < SS_TAPS; ++j) {
            const float xv = rx[j], yv = ry[j], wx = a.w[j] * xv, wy = a.w[j] * yv;
            m0 += wx; m1 += wy;
            m2 = fmaf(wx, xv, m2); m3 = fmaf(wy, yv, m3); m4 = fmaf(wx, yv, m4);
        }
        hb[i] = m0; hb[plane + i] = m1; hb[2 * plane + i] = m2; hb[3 * plane + i] = m3; hb[4 * plane + i] = m4;
    }
}

// vertical pass at flat position i of a `cols`-wide plane: s[k] = sum_j w[j] * hb[k][i + j * cols]
__device__ __forceinline__ void ssim_cols(const SsimArgs& a, const float* hb, int plane, int cols, int i, float s[5]) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = 0.0f;
#pragma unroll
    for (int j = 0; j < SS_TAPS; ++j)
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = fmaf(a.w[j], hb[k * plane + i + j * cols], s[k]);
}

// workgroup (frame, tile): partial[(frame * tiles + tile) * 3 + c] = sum of the SSIM map over the tile's valid entries of channel c
__global__ __launch_bounds__(SS_THREADS) void ssim_fwd_kernel(const SsimArgs a, double* __restrict__ partial) {
    __shared__ float sx[SF_IH * SF_IW], sy[SF_IH * SF_IW];
    __shared__ float hb[5 * SF_IH * SS_TW];
    __shared__ double red[SS_THREADS / 64];
    const long long frame = blockIdx.x / a.tiles;
    const int tile = blockIdx.x % a.tiles;
    const int oy0 = (tile / a.tiles_x) * SS_TH, ox0 = (tile % a.tiles_x) * SS_TW;
    const int Hm = a.H - SS_HALO, Wm = a.W - SS_HALO;
    double acc[3];
    for (int c = 0; c < 3; ++c) {
        ssim_stage(a, frame, c, oy0, ox0, SF_IH, SF_IW, sx, sy);
        __syncthreads();
        ssim_rows(a, sx, sy, SF_IH, SF_IW, SS_TW, hb);
        __syncthreads();
        acc[c] = 0.0;
        for (int i = threadIdx.x; i < SS_TH * SS_TW; i += SS_THREADS) {
            if (oy0 + i / SS_TW >= Hm || ox0 + i % SS_TW >= Wm) continue;
            float s[5];
            ssim_cols(a, hb, SF_IH * SS_TW, SS_TW, i, s);
            const float mxx = s[0] * s[0], myy = s[1] * s[1], mxy = s[0] * s[1];
            const float sxx = s[2] - mxx, syy = s[3] - myy, sxy = s[4] - mxy;
            acc[c] += (double)(((2.0f * mxy + SS_C1) / (mxx + myy + SS_C1)) * ((2.0f * sxy + SS_C2) / (sxx + syy + SS_C2)));
        }
        // (the next channel's stage writes sx / sy, last read before the barrier above; its row pass writes hb behind its own barrier)
    }
    for (int c = 0; c < 3; ++c) {
        const double s = block_sum(acc[c], red);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 3 + c] = s;
    }
}

// one wave per frame, fixed order: ssim[frame] = mean of the map over 3 (H-10) (W-10) entries
__global__ void ssim_final_kernel(const double* __restrict__ partial, int per_frame, double inv_count, float* __restrict__ ssim) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < per_frame; i += 64) acc += partial[(size_t)blockIdx.x * per_frame + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) ssim[blockIdx.x] = (float)(acc * inv_count);
}

// d ssim[frame] / d pred for a 16 x 32 tile of input pixels p, nothing saved by the forward:
//   dS/dx(p) = sum_q w(p - q) [dS/dmu_x(q) + 2 x(p) dS/dE[xx](q) + y(p) dS/dE[xy](q)]   over the map entries q whose window holds p.
// The three derivative maps are recomputed on the tile plus a 10-entry halo towards the origin (zero outside the valid map) and
// correlated back separably; the result is scaled by dssim[frame] / count and by the clamp's derivative (0.5 on -1 <= pred <= 1).
__global__ __launch_bounds__(SS_THREADS) void ssim_bwd_kernel(const SsimArgs a, const float* __restrict__ dssim, float inv_count,
                                                              float* __restrict__ dpred) {
    __shared__ float in[2 * SB_IH * SB_IW];        // mapped inputs; later the three derivative maps (3 * 26 * 42 <= 2 * 36 * 52)
    __shared__ float hb[5 * SB_IH * SB_QW];        // row pass of the five products; later the row pass of the derivative maps
    static_assert(3 * SB_QH * SB_QW <= 2 * SB_IH * SB_IW && 3 * SB_QH * SS_TW <= 5 * SB_IH * SB_QW, "aliased LDS planes");
    float* sx = in;
    float* sy = in + SB_IH * SB_IW;
    float* dm = in;
    const long long frame = blockIdx.x / a.tiles;
    const int tile = blockIdx.x % a.tiles;
    const int py0 = (tile / a.tiles_x) * SS_TH, px0 = (tile % a.tiles_x) * SS_TW;
    const int Hm = a.H - SS_HALO, Wm = a.W - SS_HALO;
    const int qy0 = py0 - SS_HALO, qx0 = px0 - SS_HALO;   // first map entry (also the first input pixel) of the haloed region
    const float scale = dssim[frame] * inv_count;
    const float* pf = a.pred + frame * 3 * a.H * a.W;
    const float* tf = a.target + frame * 3 * a.H * a.W;
    float* gf = dpred + frame * 3 * a.H * a.W;
    constexpr int QP = SB_QH * SB_QW, RP = SB_QH * SS_TW;
    for (int c = 0; c < 3; ++c) {
        ssim_stage(a, frame, c, qy0, qx0, SB_IH, SB_IW, sx, sy);
        __syncthreads();
        ssim_rows(a, sx, sy, SB_IH, SB_IW, SB_QW, hb);
        __syncthreads();
        // the derivative maps go where sx / sy were (last read before the barrier above); zero outside the valid map
        for (int i = threadIdx.x; i < QP; i += SS_THREADS) {
            const int qy = qy0 + i / SB_QW, qx = qx0 + i % SB_QW;
            float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
            if (qy >= 0 && qy < Hm && qx >= 0 && qx < Wm) {
                float s[5];
                ssim_cols(a, hb, SB_IH * SB_QW, SB_QW, i, s);
                const float mx = s[0], my = s[1];
                const float a1 = 2.0f * mx * my + SS_C1, a2 = 2.0f * (s[4] - mx * my) + SS_C2;
                const float r1 = 1.0f / (mx * mx + my * my + SS_C1), r2 = 1.0f / ((s[2] - mx * mx) + (s[3] - my * my) + SS_C2);
                const float S = a1 * a2 * r1 * r2;
                d0 = 2.0f * my * (a2 - a1) * r1 * r2 - 2.0f * mx * S * (r1 - r2);   // dS/dmu_x   (E[xx], E[xy] held fixed)
                d1 = -S * r2;                                                        // dS/dE[xx]
                d2 = 2.0f * a1 * r1 * r2;                                            // dS/dE[xy]
            }
            dm[i] = d0; dm[QP + i] = d1; dm[2 * QP + i] = d2;
        }
        __syncthreads();   // derivative maps complete, every read of hb done
        for (int i = threadIdx.x; i < RP; i += SS_THREADS) {   // rows: h2[k][r][pc] = sum_j w[j] * dm[k][r][pc + 10 - j]
            const float* src = dm + (i / SS_TW) * SB_QW + i % SS_TW + SS_HALO;
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
#pragma unroll
            for (int j = 0; j < SS_TAPS; ++j) {
                g0 = fmaf(a.w[j], src[-j], g0);
                g1 = fmaf(a.w[j], src[QP - j], g1);
                g2 = fmaf(a.w[j], src[2 * QP - j], g2);
            }
            hb[i] = g0; hb[RP + i] = g1; hb[2 * RP + i] = g2;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < SS_TH * SS_TW; i += SS_THREADS) {   // columns: G[k](p) = sum_j w[j] * h2[k][pr + 10 - j][pc]
            const int py = py0 + i / SS_TW, px = px0 + i % SS_TW;
            if (py >= a.H || px >= a.W) continue;
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
#pragma unroll
            for (int j = 0; j < SS_TAPS; ++j) {
                const int r = i + (SS_HALO - j) * SS_TW;
                g0 = fmaf(a.w[j], hb[r], g0);
                g1 = fmaf(a.w[j], hb[RP + r], g1);
                g2 = fmaf(a.w[j], hb[2 * RP + r], g2);
            }
            const long long e = ssim_index(a.layout, a.H, a.W, c, py, px);
            const float pv = pf[e];
            const float dclamp = (pv >= -1.0f && pv <= 1.0f) ? 0.5f : 0.0f;   // torch's clamp rule, decided on pred itself
            gf[e] = scale * dclamp * (g0 + 2.0f * ssim_unit(pv) * g1 + ssim_unit(tf[e]) * g2);
        }
        __syncthreads();   // the next channel's stage overwrites dm's planes and its row pass hb
    }
}

static inline int pm_chunks(long long frame_elems) { return (int)((frame_elems + PM_CHUNK - 1) / PM_CHUNK); }
// SS_TH x SS_TW tiles over a tile_h x tile_w area of one frame (forward: the valid SSIM map; backward: the image)
static inline int ssim_tiles(int tile_h, int tile_w, int* tiles_x) {
    *tiles_x = (tile_w + SS_TW - 1) / SS_TW;
    return *tiles_x * ((tile_h + SS_TH - 1) / SS_TH);
}

// The forward workspaces: per-workgroup partial sums in double (take() counts floats: a double is two)
struct PmSlots { double* partial; int chunks; };
template <class WS>
static void carve_pixel_measures(WS& ws, long long n_frames, long long frame_elems, PmSlots& s) {
    s.chunks = pm_chunks(frame_elems);
    s.partial = reinterpret_cast<double*>(ws.take((size_t)n_frames * s.chunks * 3 * 2));
}
struct SsimSlots { double* partial; int tiles; };
template <class WS>
static void carve_ssim(WS& ws, long long n_frames, int H, int W, SsimSlots& s) {
    int tiles_x;
    s.tiles = ssim_tiles(H - SS_HALO, W - SS_HALO, &tiles_x);
    s.partial = reinterpret_cast<double*>(ws.take((size_t)n_frames * s.tiles * 3 * 2));
}

static int pixel_measures_check(const char* who, const void* pred, const void* target, const void* io0, const void* io1, long long n_frames,
                                long long frame_elems) {
    if (!pred || !target || !io0 || !io1) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (n_frames < 1 || frame_elems < 1) { set_error("%s: n_frames and frame_elems must be >= 1 (got %lld, %lld)", who, n_frames, frame_elems); return VPX_ERR_ARG; }
    if ((frame_elems + PM_CHUNK - 1) / PM_CHUNK * n_frames > 0x7fffffffLL) { set_error("%s: %lld frames of %lld elements exceed one launch", who, n_frames, frame_elems); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

static int ssim_check(const char* who, const void* pred, const void* target, const void* io0, const void* io1, long long n_frames, int C, int H,
                      int W, int layout, SsimArgs& a, int tile_h, int tile_w) {
    if (!pred || !target || !io0 || !io1) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (n_frames < 1) { set_error("%s: n_frames must be >= 1 (got %lld)", who, n_frames); return VPX_ERR_ARG; }
    if (C != 3) { set_error("%s: SSIM needs 3-channel images (got %d channels)", who, C); return VPX_ERR_ARG; }
    if (H < SS_TAPS || W < SS_TAPS) { set_error("%s: images must be at least %dx%d for the %d-tap window (got %dx%d)", who, SS_TAPS, SS_TAPS, SS_TAPS, H, W); return VPX_ERR_ARG; }
    if (layout != VPX_LAYOUT_NHWC && layout != VPX_LAYOUT_NCHW) { set_error("%s: unknown layout %d", who, layout); return VPX_ERR_ARG; }
    a.pred = (const float*)pred; a.target = (const float*)target;
    a.H = H; a.W = W; a.layout = layout;
    a.tiles = ssim_tiles(tile_h, tile_w, &a.tiles_x);
    if ((long long)a.tiles * n_frames > 0x7fffffffLL) { set_error("%s: %lld frames of %dx%d exceed one launch", who, n_frames, H, W); return VPX_ERR_UNSUPPORTED; }
    double g[SS_TAPS], sum = 0.0;   // piqa's gaussian_kernel(11, sigma = 1.5), normalised to sum 1
    for (int j = 0; j < SS_TAPS; ++j) { const double x = (j - SS_TAPS / 2) / 1.5; g[j] = exp(-0.5 * x * x); sum += g[j]; }
    for (int j = 0; j < SS_TAPS; ++j) a.w[j] = (float)(g[j] / sum);
    return VPX_OK;
}

}  // namespace vpx

using namespace vpx;

extern "C" {

size_t vpx_pixel_measures_workspace_bytes(long long n_frames, long long frame_elems) {
    if (n_frames < 1 || frame_elems < 1) return 0;
    CarveMeasure m; PmSlots s{};
    carve_pixel_measures(m, n_frames, frame_elems, s);
    return m.off + 256;
}

int vpx_pixel_measures_fwd(const float* pred, const float* target, long long n_frames, long long frame_elems, double* sums,
                           void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = pixel_measures_check("vpx_pixel_measures_fwd", pred, target, sums, sums, n_frames, frame_elems)) return rc;
    if (!workspace || workspace_bytes < vpx_pixel_measures_workspace_bytes(n_frames, frame_elems)) { set_error("vpx_pixel_measures_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    PmSlots s{};
    carve_pixel_measures(ws, n_frames, frame_elems, s);
    VPX_CHECK_CARVE(ws, "vpx_pixel_measures_fwd");
    VPX_LAUNCH(pixel_measures_partial_kernel, dim3((unsigned)(n_frames * s.chunks)), dim3(PM_THREADS), 0, stream, pred, target, frame_elems, s.chunks, s.partial);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(pixel_measures_final_kernel, dim3((unsigned)n_frames), dim3(64), 0, stream, s.partial, s.chunks, n_frames, sums);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_pixel_measures_bwd(const float* pred, const float* target, const float* dsums, long long n_frames, long long frame_elems,
                           float* dpred, void* stream_) {
    if (int rc = pixel_measures_check("vpx_pixel_measures_bwd", pred, target, dsums, dpred, n_frames, frame_elems)) return rc;
    const int chunks = pm_chunks(frame_elems);
    VPX_LAUNCH(pixel_measures_bwd_kernel, dim3((unsigned)(n_frames * chunks)), dim3(PM_THREADS), 0, (hipStream_t)stream_, pred, target, dsums, frame_elems,
               chunks, n_frames, dpred);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

size_t vpx_ssim_workspace_bytes(long long n_frames, int H, int W) {
    if (n_frames < 1 || H < SS_TAPS || W < SS_TAPS) return 0;
    CarveMeasure m; SsimSlots s{};
    carve_ssim(m, n_frames, H, W, s);
    return m.off + 256;
}

int vpx_ssim_fwd(const float* pred, const float* target, long long n_frames, int C, int H, int W, int layout, float* ssim,
                 void* workspace, size_t workspace_bytes, void* stream_) {
    SsimArgs a;
    if (int rc = ssim_check("vpx_ssim_fwd", pred, target, ssim, ssim, n_frames, C, H, W, layout, a, H - SS_HALO, W - SS_HALO)) return rc;
    if (!workspace || workspace_bytes < vpx_ssim_workspace_bytes(n_frames, H, W)) { set_error("vpx_ssim_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    SsimSlots s{};
    carve_ssim(ws, n_frames, H, W, s);   // (s.tiles == a.tiles: ssim_check counted the same area with the same function)
    VPX_CHECK_CARVE(ws, "vpx_ssim_fwd");
    VPX_LAUNCH(ssim_fwd_kernel, dim3((unsigned)(n_frames * s.tiles)), dim3(SS_THREADS), 0, stream, a, s.partial);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(ssim_final_kernel, dim3((unsigned)n_frames), dim3(64), 0, stream, s.partial, 3 * s.tiles, 1.0 / (3.0 * (H - SS_HALO) * (double)(W - SS_HALO)), ssim);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_ssim_bwd(const float* pred, const float* target, const float* dssim, long long n_frames, int C, int H, int W, int layout,
                 float* dpred, void* stream_) {
    SsimArgs a;
    if (int rc = ssim_check("vpx_ssim_bwd", pred, target, dssim, dpred, n_frames, C, H, W, layout, a, H, W)) return rc;
    VPX_LAUNCH(ssim_bwd_kernel, dim3((unsigned)(n_frames * a.tiles)), dim3(SS_THREADS), 0, (hipStream_t)stream_, a, dssim,
               (float)(1.0 / (3.0 * (H - SS_HALO) * (double)(W - SS_HALO))), dpred);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
