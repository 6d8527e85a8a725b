// LPIPS on an AlexNet trunk (https://arxiv.org/abs/1801.03924; vp_suite/measure/image_wise.py's LPIPS through piqa), forward and the
// gradient with respect to the prediction (the trunk's weights are frozen), fp32, no floating-point atomics — bit-reproducible. The
// trunk runs channels-last (NHWC), the layout of the library's convolutions:
//   vpx_lpips_stem_fwd      clamp((v+1)/2, 0, 1) and the ImageNet normalisation fused into the operand load of the 11x11 stride-4 pad-2
//                           convolution 3 -> 64, bias, ReLU. The padding ring is zero in NORMALISED space.
//   vpx_lpips_maxpool_fwd   3x3 stride-2 max-pool, floor mode, no padding
//   vpx_lpips_head_fwd      per pixel: both channel norms, sum_c w[c] (fx/(|fx|+1e-10) - fy/(|fy|+1e-10))^2; per image: the pixel mean,
//                           ADDED into a float64 table. Every feature element is read once; the normalised maps never exist in memory.
//   vpx_lpips_fwd           the whole measure: prediction and target as ONE batch of 2n images through stem, pools and the four stride-1
//                           "same" convolutions + ReLU (the library's implicit-GEMM kernel with ReLU in its epilogue: glue_forward with
//                           VPX_ACT_RELU, exact fp32 operands), one head launch per tap.
//   vpx_lpips_fwd_train     the same launches, with the five taps kept in a reserve for the backward
//   vpx_lpips_head_bwd      the head's gradient with respect to fx, plus the gradient arriving from the next layer, times the ReLU mask
//   vpx_lpips_maxpool_bwd   a gather: one thread per input element, the window maxima found again in the tap
//   vpx_lpips_stem_bwd      the stem's data gradient as a gather by input phase, times 0.5 / std_c and the clamp's mask
//   vpx_lpips_bwd           the whole backward over the n prediction images: heads from tap 5 down, the four stride-1 data gradients on
//                           the library's glue backward (vpx_conv2d_ex_bwd, dw not requested), pools, stem
#include <hip/hip_runtime.h>
#include <math.h>
#include "vpx_internal.h"
#include "vpx_host.h"

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- stem ----------------------------------------------------------------------------------------------------------------------
// A workgroup computes an 8x8 tile of output pixels for all 64 channels: wave g holds channels 16g .. 16g+15 of the 64 pixels (one
// per lane). The haloed input patch (39x39 per channel, mapped and normalised while it is staged) lies in LDS with the columns
// de-interleaved by x mod 4, so that the 8 lanes of a tile row read consecutive words although the convolution strides by 4; the
// row pitch of 42 puts the 8 tile rows (4 patch rows apart) on banks 8 apart. The weights of one input channel ([121 taps][64 outputs],
// transposed once per call by lpips_stem_pack_kernel) are staged per channel and read as wave-wide broadcasts.
constexpr int LP_K = 11, LP_STRIDE = 4, LP_PAD = 2, LP_CO = 64, LP_TAPS = LP_K * LP_K;
constexpr int ST_TILE = 8;
constexpr int ST_IN = (ST_TILE - 1) * LP_STRIDE + LP_K;   // 39 input rows / columns under a tile
constexpr int ST_PHASE = (ST_IN + 3) / 4;                 // 10 columns of each x mod 4
constexpr int ST_PITCH = 42;
constexpr int ST_THREADS = 256;
constexpr int ST_PACK_FLOATS = 3 * LP_TAPS * LP_CO;
static_assert(4 * ST_PHASE <= ST_PITCH && ST_TILE * ST_TILE == 64 && ST_THREADS / 64 * 16 == LP_CO, "stem tiling");

// wT[c][tap][co] = w[co][c][tap]
__global__ void lpips_stem_pack_kernel(const float* __restrict__ w, float* __restrict__ wT) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ST_PACK_FLOATS) return;
    const int co = i % LP_CO, tap = (i / LP_CO) % LP_TAPS, c = i / (LP_CO * LP_TAPS);
    wT[i] = w[(co * 3 + c) * LP_TAPS + tap];
}

__global__ __launch_bounds__(ST_THREADS) void lpips_stem_kernel(const float* __restrict__ x0, const float* __restrict__ x1, long long n0, int H, int W,
                                                                int Ho, int Wo, int tiles_x, int tiles, const float* __restrict__ wT,
                                                                const float* __restrict__ bias, float* __restrict__ y) {
    __shared__ float patch[3 * ST_IN * ST_PITCH];
    __shared__ __attribute__((aligned(16))) float wl[LP_TAPS * LP_CO];
    const long long n = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int oy0 = (tile / tiles_x) * ST_TILE, ox0 = (tile % tiles_x) * ST_TILE;
    const float* img = n < n0 ? x0 + n * 3 * H * W : x1 + (n - n0) * 3 * H * W;
    const int iy0 = oy0 * LP_STRIDE - LP_PAD, ix0 = ox0 * LP_STRIDE - LP_PAD;
    for (int i = threadIdx.x; i < 3 * ST_IN * ST_IN; i += ST_THREADS) {
        const int c = i / (ST_IN * ST_IN), r = (i / ST_IN) % ST_IN, xx = i % ST_IN;
        const int iy = iy0 + r, ix = ix0 + xx;
        float v = 0.0f;   // the padding ring and everything beyond the image: zero AFTER the normalisation
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const float u = fminf(fmaxf((img[((long long)c * H + iy) * W + ix] + 1.0f) * 0.5f, 0.0f), 1.0f);   // reshape_clamp
            const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
            v = (u - mean) / sd;
        }
        patch[(c * ST_IN + r) * ST_PITCH + (xx & 3) * ST_PHASE + (xx >> 2)] = v;
    }
    const int p = threadIdx.x & 63, g = threadIdx.x >> 6, py = p >> 3, px = p & 7;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = bias[g * 16 + j];
    for (int c = 0; c < 3; ++c) {
        __syncthreads();   // the patch is staged (c == 0); every read of the previous channel's weights is done
        for (int i = threadIdx.x; i < LP_TAPS * LP_CO / 4; i += ST_THREADS)
            reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(wT + c * LP_TAPS * LP_CO)[i];
        __syncthreads();
        const float* pr = patch + (c * ST_IN + py * LP_STRIDE) * ST_PITCH + px;
        for (int ky = 0; ky < LP_K; ++ky) {
            float row[16];   // blocked summation: the 11 products of a kernel row first, then one add into the running sum of 363
#pragma unroll
            for (int j = 0; j < 16; ++j) row[j] = 0.0f;
#pragma unroll
            for (int kx = 0; kx < LP_K; ++kx) {
                const float xv = pr[ky * ST_PITCH + (kx & 3) * ST_PHASE + (kx >> 2)];
                const f32x4* wv = reinterpret_cast<const f32x4*>(wl + (ky * LP_K + kx) * LP_CO + g * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w4 = wv[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) row[q * 4 + k] = fmaf(xv, w4[k], row[q * 4 + k]);
                }
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += row[j];
        }
    }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy >= Ho || ox >= Wo) return;
    f32x4* o = reinterpret_cast<f32x4*>(y + ((n * Ho + oy) * Wo + ox) * LP_CO + g * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaxf(acc[q * 4 + k], 0.0f);
        o[q] = v;
    }
}

// ---- max-pool 3x3 / 2, floor mode, NHWC: one thread per output element, channels fastest ------------------------------------------
constexpr int MP_THREADS = 256;
__global__ __launch_bounds__(MP_THREADS) void lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int W,
                                                                   int C, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long long p = i / C;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const long long n = p / Ho;
    const float* s = x + ((n * H + oy * 2) * W + ox * 2) * C + c;   // rows 2 oy .. 2 oy + 2 <= H - 1 by Ho = (H - 3) / 2 + 1
    float m = s[0];                                                  // (the window's own first element: no initial value to leak)
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float v = s[((long long)dy * W + dx) * C];
            m = (v > m || v != v) ? v : m;   // NaN wins, as in torch
        }
    y[i] = m;
}

// ---- layer head ----------------------------------------------------------------------------------------------------------------------
// A wave takes one pixel at a time: lane l holds channels l, l + 64, ... of both feature vectors in registers (C <= 512), the two
// squared norms are wave reductions, the weighted squared difference of the normalised vectors is summed per lane over the wave's
// pixels; all of it in double on the fp32 features. Workgroup (image, chunk of 64 pixels) -> partial[image * chunks + chunk]; a second launch adds the pixel mean of
// every image into the table in a fixed order.
constexpr int HD_THREADS = 256, HD_WAVES = HD_THREADS / 64, HD_PIX = 64, HD_MAX_C = 512, HD_PER_LANE = HD_MAX_C / 64;

static __device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(HD_THREADS) void lpips_head_kernel(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ w,
                                                                long long HW, int C, int chunks, double* __restrict__ partial) {
    __shared__ double red[HD_WAVES];
    const long long n = blockIdx.x / chunks;
    const long long first = (long long)(blockIdx.x % chunks) * HD_PIX;
    const long long last = first + HD_PIX < HW ? first + HD_PIX : HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wv[HD_PER_LANE];
#pragma unroll
    for (int j = 0; j < HD_PER_LANE; ++j) wv[j] = lane + 64 * j < C ? w[lane + 64 * j] : 0.0f;
    double acc = 0.0;
    for (long long pix = first + wave; pix < last; pix += HD_WAVES) {
        const float* a = fx + (n * HW + pix) * C;
        const float* b = fy + (n * HW + pix) * C;
        float va[HD_PER_LANE], vb[HD_PER_LANE];
        double sa = 0.0, sb = 0.0;   // the arithmetic on the fp32 features is double, as in measure.hip: the kernel stays bound by its two reads
#pragma unroll
        for (int j = 0; j < HD_PER_LANE; ++j) {
            const bool in = lane + 64 * j < C;
            va[j] = in ? a[lane + 64 * j] : 0.0f;
            vb[j] = in ? b[lane + 64 * j] : 0.0f;
            sa = fma((double)va[j], (double)va[j], sa);
            sb = fma((double)vb[j], (double)vb[j], sb);
        }
        const double ia = 1.0 / (sqrt(lp_wave_sum(sa)) + 1e-10), ib = 1.0 / (sqrt(lp_wave_sum(sb)) + 1e-10);   // an all-zero vector: 0 * 1e10 = 0
#pragma unroll
        for (int j = 0; j < HD_PER_LANE; ++j) {
            double t;
            {   // both products rounded, never contracted into an fma (which would keep one of them exact): identical maps give exactly 0
#pragma clang fp contract(off)
                const double pa = (double)va[j] * ia, pb = (double)vb[j] * ib;
                t = pa - pb;
            }
            acc = fma((double)wv[j] * t, t, acc);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < HD_WAVES; ++k) s += red[k];
        partial[blockIdx.x] = s;
    }
}

// one wave per image, fixed order: table[image] += mean over the pixels
__global__ void lpips_head_final_kernel(const double* __restrict__ partial, int chunks, double inv_pixels, double* __restrict__ table) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < chunks; i += 64) acc += partial[(size_t)blockIdx.x * chunks + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) table[blockIdx.x] += acc * inv_pixels;
}

// ---- layer head, backward -------------------------------------------------------------------------------------------------------------
// The forward's lane layout, one wave per pixel, double arithmetic. With s = |fx|, r = 1 / (s + 1e-10), t_c = fx_c r - fy_c / (|fy| + 1e-10)
// and u_c = 2 w_c t_c:   d fx_c = (dtable[image] / HW) (r u_c - fx_c r^2 (sum_k u_k fx_k) / s),  plus the gradient that arrives from the next
// layer, times the ReLU mask fx_c > 0: the result is the gradient of the tap's PRE-activation. An all-zero vector has s = 0: the second
// term is left out (every fx_c is 0, the mask removes the element anyway), so nothing divides by 0. dz may be `incoming` itself: an
// element is read and written by one lane only.
__global__ __launch_bounds__(HD_THREADS) void lpips_head_bwd_kernel(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ w,
                                                                    const double* __restrict__ dtable, const float* incoming, long long HW, int C,
                                                                    int chunks, float* dz) {
    const long long n = blockIdx.x / chunks;
    const long long first = (long long)(blockIdx.x % chunks) * HD_PIX;
    const long long last = first + HD_PIX < HW ? first + HD_PIX : HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double scale = dtable[n] / (double)HW;
    float wv[HD_PER_LANE];
#pragma unroll
    for (int j = 0; j < HD_PER_LANE; ++j) wv[j] = lane + 64 * j < C ? w[lane + 64 * j] : 0.0f;
    for (long long pix = first + wave; pix < last; pix += HD_WAVES) {
        const long long at = (n * HW + pix) * C;
        float va[HD_PER_LANE], vb[HD_PER_LANE];
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < HD_PER_LANE; ++j) {
            const bool in = lane + 64 * j < C;
            va[j] = in ? fx[at + lane + 64 * j] : 0.0f;
            vb[j] = in ? fy[at + lane + 64 * j] : 0.0f;
            sa = fma((double)va[j], (double)va[j], sa);
            sb = fma((double)vb[j], (double)vb[j], sb);
        }
        const double s = sqrt(lp_wave_sum(sa)), ia = 1.0 / (s + 1e-10), ib = 1.0 / (sqrt(lp_wave_sum(sb)) + 1e-10);
        double u[HD_PER_LANE], dot = 0.0;
#pragma unroll
        for (int j = 0; j < HD_PER_LANE; ++j) {
            double t;
            {   // as in the forward: both products rounded, so that identical maps give a gradient of exactly 0
#pragma clang fp contract(off)
                const double pa = (double)va[j] * ia, pb = (double)vb[j] * ib;
                t = pa - pb;
            }
            u[j] = 2.0 * (double)wv[j] * t;
            dot = fma(u[j], (double)va[j], dot);
        }
        dot = lp_wave_sum(dot);
        const double k = s > 0.0 ? ia * ia * dot / s : 0.0;
#pragma unroll
        for (int j = 0; j < HD_PER_LANE; ++j) {
            if (lane + 64 * j >= C) continue;
            double g = scale * (ia * u[j] - (double)va[j] * k);
            if (incoming) g += (double)incoming[at + lane + 64 * j];
            dz[at + lane + 64 * j] = va[j] > 0.0f ? (float)g : 0.0f;
        }
    }
}

// ---- max-pool 3x3 / 2, backward: a gather, one thread per INPUT element ---------------------------------------------------------------
// An element lies in at most 2 x 2 windows. Each window's maximum is found again from x, by the forward's own scan (rows, then columns;
// a later element replaces the running maximum only when it is GREATER, or NaN): among tied elements the FIRST in that order takes the
// window's gradient, the element torch's CPU max_pool2d backward picks (tests/test_lpips_grad_host.py). Rows and columns that floor mode
// drops lie in no window and get 0.
__global__ __launch_bounds__(MP_THREADS) void lpips_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                                       long long total, int H, int W, int C, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long long p = i / C;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H);
    const long long n = p / H;
    const int oy0 = iy < 2 ? 0 : (iy - 1) / 2, oy1 = iy / 2 < Ho - 1 ? iy / 2 : Ho - 1;   // windows 2 o .. 2 o + 2 that hold the element
    const int ox0 = ix < 2 ? 0 : (ix - 1) / 2, ox1 = ix / 2 < Wo - 1 ? ix / 2 : Wo - 1;
    float acc = 0.0f;
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const float* s = x + ((n * H + oy * 2) * W + ox * 2) * C + c;
            float m = s[0];
            int arg = 0;
#pragma unroll
            for (int k = 1; k < 9; ++k) {
                const float v = s[((long long)(k / 3) * W + k % 3) * C];
                if (v > m || v != v) { m = v; arg = k; }
            }
            if (arg == (iy - oy * 2) * 3 + (ix - ox * 2)) acc += dy[((n * Ho + oy) * Wo + ox) * C + c];
        }
    dx[i] = acc;
}

// ---- stem, backward: the data gradient of the 11x11 stride-4 pad-2 convolution, as a gather ---------------------------------------------
// Input row iy = 4 q + p - 2 (cell q, phase p = (iy + 2) mod 4) meets kernel row ky = p + 4 a at output row q - a, a = 0, 1, 2 with ky < 11:
// the taps of a pixel depend on its phase alone. A workgroup takes 8 x 8 cells (32 x 32 input pixels, 3 colours) and stages the 10 x 10
// output pixels x 64 channels of dz under them once. Wave g computes the pixels of row phase g, one cell per lane, column phase after
// column phase: per tap the 64 channels of one dz pixel (ds_read_b128 per lane) against the weights of the three colours (wave-wide
// broadcasts, staged per column phase from the forward's transposed pack). A dz pixel takes 68 floats and a tile row 736, which spreads
// the 16 lanes that share a ds_read_b128 cycle over all banks. The sums go through LDS (over the dz tile, which is dead by then) so that
// x is read and dx written in whole rows; the epilogue multiplies by 0.5 / std_c and by the clamp's mask, evaluated on the forward's own
// fp32 (v + 1) / 2: the gradient passes where 0 <= u <= 1, bounds included (torch's clamp).
constexpr int SB_CELLS = 8, SB_DZ = SB_CELLS + 2, SB_SIDE = SB_CELLS * 4;
constexpr int SB_PIX = 68, SB_ROW = 736, SB_OUT_PITCH = 40;
constexpr int SB_THREADS = 256;
static_assert(SB_DZ * SB_PIX <= SB_ROW && SB_ROW % 64 == 32 && SB_PIX % 4 == 0 && SB_PIX >= LP_CO, "stem backward: dz tile pitches");
static_assert(3 * SB_SIDE * SB_OUT_PITCH <= SB_DZ * SB_ROW && SB_THREADS / 64 == 4 && SB_CELLS * SB_CELLS == 64, "stem backward tiling");

__global__ __launch_bounds__(SB_THREADS) void lpips_stem_bwd_kernel(const float* __restrict__ x, const float* __restrict__ wT, const float* __restrict__ dz,
                                                                    int H, int W, int Ho, int Wo, int tiles_x, int tiles, float* __restrict__ dx) {
    __shared__ __attribute__((aligned(16))) float dzt[SB_DZ * SB_ROW];
    __shared__ __attribute__((aligned(16))) float wl[4 * 3 * 9 * LP_CO];   // [row phase][colour][a * 3 + b][channel]
    const long long n = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int qy0 = (tile / tiles_x) * SB_CELLS, qx0 = (tile % tiles_x) * SB_CELLS;
    for (int i = threadIdx.x; i < SB_DZ * SB_DZ * (LP_CO / 4); i += SB_THREADS) {
        const int q = i % (LP_CO / 4), col = (i / (LP_CO / 4)) % SB_DZ, r = i / ((LP_CO / 4) * SB_DZ);
        const int oy = qy0 - 2 + r, ox = qx0 - 2 + col;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};   // beyond the output map: no window there
        if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) v = reinterpret_cast<const f32x4*>(dz + ((n * Ho + oy) * Wo + ox) * LP_CO)[q];
        reinterpret_cast<f32x4*>(dzt + r * SB_ROW + col * SB_PIX)[q] = v;
    }
    const int lane = threadIdx.x & 63, py = threadIdx.x >> 6, cy = lane >> 3, cx = lane & 7;
    const int na = py + 8 < LP_K ? 3 : 2;
    float res[4][3];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        __syncthreads();   // the dz tile is staged (px == 0); every read of the previous column phase's weights is done
        for (int i = threadIdx.x; i < 4 * 3 * 9 * (LP_CO / 4); i += SB_THREADS) {
            const int q = i % (LP_CO / 4), t = (i / (LP_CO / 4)) % 9, c = (i / (LP_CO / 4 * 9)) % 3, p = i / (LP_CO / 4 * 27);
            const int ky = p + 4 * (t / 3), kx = px + 4 * (t % 3);
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (ky < LP_K && kx < LP_K) v = reinterpret_cast<const f32x4*>(wT + ((size_t)c * LP_TAPS + ky * LP_K + kx) * LP_CO)[q];
            reinterpret_cast<f32x4*>(wl)[i] = v;
        }
        __syncthreads();
        const int nb = px + 8 < LP_K ? 3 : 2;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int a = 0; a < na; ++a)
            for (int b = 0; b < nb; ++b) {
                const f32x4* dp = reinterpret_cast<const f32x4*>(dzt + (cy + 2 - a) * SB_ROW + (cx + 2 - b) * SB_PIX);
                const f32x4* wp = reinterpret_cast<const f32x4*>(wl + ((py * 3) * 9 + a * 3 + b) * LP_CO);
                float row[3] = {0.0f, 0.0f, 0.0f};   // blocked summation: the 64 channels of a tap first, then one add into the running sum
#pragma unroll
                for (int q = 0; q < LP_CO / 4; ++q) {
                    const f32x4 d4 = dp[q];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const f32x4 w4 = wp[c * 9 * (LP_CO / 4) + q];
#pragma unroll
                        for (int k = 0; k < 4; ++k) row[c] = fmaf(d4[k], w4[k], row[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += row[c];
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) res[px][c] = acc[c];
    }
    __syncthreads();   // every wave is done with the dz tile: the sums take its place
    float* out = dzt;
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(c * SB_SIDE + cy * 4 + py) * SB_OUT_PITCH + cx * 4 + px] = res[px][c];
    __syncthreads();
    const int iy0 = qy0 * 4 - LP_PAD, ix0 = qx0 * 4 - LP_PAD;
    for (int i = threadIdx.x; i < 3 * SB_SIDE * SB_SIDE; i += SB_THREADS) {
        const int col = i % SB_SIDE, r = (i / SB_SIDE) % SB_SIDE, c = i / (SB_SIDE * SB_SIDE);
        const int iy = iy0 + r, ix = ix0 + col;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const long long at = ((n * 3 + c) * H + iy) * W + ix;
        const float u = (x[at] + 1.0f) * 0.5f;   // the forward's own argument of the clamp
        const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        dx[at] = (u >= 0.0f && u <= 1.0f) ? out[(c * SB_SIDE + r) * SB_OUT_PITCH + col] * (0.5f / sd) : 0.0f;
    }
}

// ---- host side: the launchers, shared by their own entry points and the trunk ----------------------------------------------------------
constexpr long long LP_MAX_GRID = 0x7fffffffLL;
constexpr int LP_MIN_SIDE = 31;   // below it the third tap has no pixel
static inline int lp_stem_out(int n) { return (n + 2 * LP_PAD - LP_K) / LP_STRIDE + 1; }
static inline int lp_pool_out(int n) { return (n - 3) / 2 + 1; }
static inline int lp_head_chunks(long long HW) { return (int)((HW + HD_PIX - 1) / HD_PIX); }

static int lp_stem(const char* who, const float* x0, const float* x1, long long n0, long long n1, int H, int W, const float* w, const float* bias,
                   float* y, float* wT, hipStream_t stream) {
    const int Ho = lp_stem_out(H), Wo = lp_stem_out(W);
    const int tiles_x = (Wo + ST_TILE - 1) / ST_TILE, tiles = tiles_x * ((Ho + ST_TILE - 1) / ST_TILE);
    if ((n0 + n1) * tiles > LP_MAX_GRID) { set_error("%s: %lld images of %dx%d exceed one launch", who, n0 + n1, H, W); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(wT, ST_PACK_FLOATS * sizeof(float), "stem weights (lpips_stem_pack_kernel)") ||
        !ws_write_ok(y, (size_t)(n0 + n1) * Ho * Wo * LP_CO * sizeof(float), "tap 1 (lpips_stem_kernel)"))
        VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(lpips_stem_pack_kernel, dim3((ST_PACK_FLOATS + 255) / 256), dim3(256), 0, stream, w, wT);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(lpips_stem_kernel, dim3((unsigned)((n0 + n1) * tiles)), dim3(ST_THREADS), 0, stream, x0, x1, n0, H, W, Ho, Wo, tiles_x, tiles, wT, bias, y);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int lp_pool(const char* who, const float* x, float* y, long long N, int H, int W, int C, hipStream_t stream) {
    const int Ho = lp_pool_out(H), Wo = lp_pool_out(W);
    const long long total = N * Ho * Wo * C;
    if ((total + MP_THREADS - 1) / MP_THREADS > LP_MAX_GRID) { set_error("%s: %lld maps of %dx%dx%d exceed one launch", who, N, H, W, C); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(y, (size_t)total * sizeof(float), "pooled map (lpips_maxpool_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(lpips_maxpool_kernel, dim3((unsigned)((total + MP_THREADS - 1) / MP_THREADS)), dim3(MP_THREADS), 0, stream, x, y, total, H, W, C, Ho, Wo);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int lp_head(const char* who, const float* fx, const float* fy, const float* w, long long n, long long HW, int C, double* table, double* partial,
                   hipStream_t stream) {
    const int chunks = lp_head_chunks(HW);
    if (C > HD_MAX_C) { set_error("%s: %d channels, the head holds at most %d per pixel", who, C, HD_MAX_C); return VPX_ERR_UNSUPPORTED; }
    if (n * chunks > LP_MAX_GRID) { set_error("%s: %lld images of %lld pixels exceed one launch", who, n, HW); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(partial, (size_t)n * chunks * sizeof(double), "head partial sums (lpips_head_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(lpips_head_kernel, dim3((unsigned)(n * chunks)), dim3(HD_THREADS), 0, stream, fx, fy, w, HW, C, chunks, partial);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(lpips_head_final_kernel, dim3((unsigned)n), dim3(64), 0, stream, partial, chunks, 1.0 / (double)HW, table);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int lp_head_bwd(const char* who, const float* fx, const float* fy, const float* w, const double* dtable, const float* incoming, long long n,
                       long long HW, int C, float* dz, hipStream_t stream) {
    const int chunks = lp_head_chunks(HW);
    if (C > HD_MAX_C) { set_error("%s: %d channels, the head holds at most %d per pixel", who, C, HD_MAX_C); return VPX_ERR_UNSUPPORTED; }
    if (n * chunks > LP_MAX_GRID) { set_error("%s: %lld images of %lld pixels exceed one launch", who, n, HW); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(dz, (size_t)n * HW * C * sizeof(float), "tap gradient (lpips_head_bwd_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(lpips_head_bwd_kernel, dim3((unsigned)(n * chunks)), dim3(HD_THREADS), 0, stream, fx, fy, w, dtable, incoming, HW, C, chunks, dz);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int lp_pool_bwd(const char* who, const float* x, const float* dy, float* dx, long long N, int H, int W, int C, hipStream_t stream) {
    const long long total = N * H * W * C;
    if ((total + MP_THREADS - 1) / MP_THREADS > LP_MAX_GRID) { set_error("%s: %lld maps of %dx%dx%d exceed one launch", who, N, H, W, C); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(dx, (size_t)total * sizeof(float), "pool input gradient (lpips_maxpool_bwd_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(lpips_maxpool_bwd_kernel, dim3((unsigned)((total + MP_THREADS - 1) / MP_THREADS)), dim3(MP_THREADS), 0, stream, x, dy, dx, total, H, W, C,
               lp_pool_out(H), lp_pool_out(W));
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int lp_stem_bwd(const char* who, const float* x, const float* w, const float* dz, long long n, int H, int W, float* dx, float* wT, hipStream_t stream) {
    const int cells_y = (H + 1) / 4 + 1, cells_x = (W + 1) / 4 + 1;   // input row iy lies in cell (iy + 2) / 4
    const int tiles_x = (cells_x + SB_CELLS - 1) / SB_CELLS, tiles = tiles_x * ((cells_y + SB_CELLS - 1) / SB_CELLS);
    if (n * tiles > LP_MAX_GRID) { set_error("%s: %lld images of %dx%d exceed one launch", who, n, H, W); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(wT, ST_PACK_FLOATS * sizeof(float), "stem weights (lpips_stem_pack_kernel)") ||
        !ws_write_ok(dx, (size_t)n * 3 * H * W * sizeof(float), "image gradient (lpips_stem_bwd_kernel)"))
        VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(lpips_stem_pack_kernel, dim3((ST_PACK_FLOATS + 255) / 256), dim3(256), 0, stream, w, wT);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(lpips_stem_bwd_kernel, dim3((unsigned)(n * tiles)), dim3(SB_THREADS), 0, stream, x, wT, dz, H, W, lp_stem_out(H), lp_stem_out(W), tiles_x,
               tiles, dx);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

// ---- the trunk: AlexNet's features in torchvision's layout -------------------------------------------------------------------------
struct LpLayer { int Ci, Co, k; };
constexpr LpLayer LP_LAYER[4] = {{64, 192, 5}, {192, 384, 3}, {384, 256, 3}, {256, 256, 3}};   // taps 2 .. 5, stride 1, "same"
struct LpGeo { int h[3], w[3]; };   // maps of tap 1, of tap 2 (after the first pool), of taps 3-5 (after the second)
static inline void lp_geo(int H, int W, LpGeo& g) {
    g.h[0] = lp_stem_out(H); g.w[0] = lp_stem_out(W);
    for (int i = 1; i < 3; ++i) { g.h[i] = lp_pool_out(g.h[i - 1]); g.w[i] = lp_pool_out(g.w[i - 1]); }
}
static inline vpx_conv_desc lp_desc(int layer, long long n2, const LpGeo& g) {
    const int s = layer == 0 ? 1 : 2;
    vpx_conv_desc d{};
    d.N = (int)n2; d.H = g.h[s]; d.W = g.w[s]; d.Ci = LP_LAYER[layer].Ci; d.Co = LP_LAYER[layer].Co;
    d.kh = d.kw = LP_LAYER[layer].k; d.stride = 1; d.pad = LP_LAYER[layer].k / 2; d.precision = VPX_PREC_F32;
    return d;
}
// The workspace: ONE list of slots, taken by the call's Carver and by the size query's CarveMeasure. The maps ping-pong between two
// slots (a tap is read by its head and by the next layer only): A holds taps 1, 2, 3 and 5, B the two pooled maps and tap 4.
struct LpSlots { float *wT, *A, *B, *wpk[4], *partial; size_t pack_bytes[4]; };
template <class WS>
static int carve_lpips(WS& ws, long long n, const LpGeo& g, LpSlots& s) {
    const size_t n2 = (size_t)2 * n, px0 = (size_t)g.h[0] * g.w[0], px1 = (size_t)g.h[1] * g.w[1], px2 = (size_t)g.h[2] * g.w[2];
    size_t a = px0 * 64, b = px1 * 64;
    if (px1 * 192 > a) a = px1 * 192;
    if (px2 * 384 > a) a = px2 * 384;
    if (px2 * 192 > b) b = px2 * 192;
    if (px2 * 256 > b) b = px2 * 256;
    s.wT = ws.take(ST_PACK_FLOATS);
    s.A = ws.take(n2 * a);
    s.B = ws.take(n2 * b);
    for (int l = 0; l < 4; ++l) {
        const vpx_conv_desc d = lp_desc(l, (long long)n2, g);
        GlueGeo gg;
        GlueChoice c;
        if (int rc = glue_check(&d, gg)) return rc;
        glue_route(&d, gg, false, VPX_ACT_RELU, false, c);
        s.pack_bytes[l] = c.pack_bytes;
        s.wpk[l] = ws.take(c.pack_bytes / sizeof(float));
    }
    s.partial = ws.take((size_t)n * lp_head_chunks((long long)px0) * 2);   // doubles; tap 1 has the most pixels
    return VPX_OK;
}

static int lpips_check(const char* who, long long n, int C, int H, int W) {
    if (n < 1) { set_error("%s: n_frames must be >= 1 (got %lld)", who, n); return VPX_ERR_ARG; }
    if (C != 3) { set_error("%s: LPIPS needs 3-channel images (got %d channels)", who, C); return VPX_ERR_ARG; }
    if (H < LP_MIN_SIDE || W < LP_MIN_SIDE) { set_error("%s: images must be at least %dx%d, below that the third tap has no pixel (got %dx%d)", who, LP_MIN_SIDE, LP_MIN_SIDE, H, W); return VPX_ERR_ARG; }
    if (2 * n > 0x7fffffffLL) { set_error("%s: %lld frames exceed one call", who, n); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

// What a training call keeps for its backward: the five taps of the 2n images (prediction first), ONE list of slots for the call's
// Carver and the size query's CarveMeasure. The pooled maps are not kept: the pool's backward finds the window maxima again in the tap.
constexpr int LP_TAP_C[5] = {64, 192, 384, 256, 256}, LP_TAP_STAGE[5] = {0, 1, 2, 2, 2};
struct LpReserve { float* tap[5]; };
struct CarveRead {   // the backward's walk over the reserve: the Carver's addresses, nothing registered (the reserve is only read)
    char* base; size_t off;
    explicit CarveRead(const void* p) : base(const_cast<char*>(static_cast<const char*>(p))), off((256 - ((uintptr_t)p & 255)) & 255) {}
    float* take(size_t nfloat) { float* p = reinterpret_cast<float*>(base + off); off += align256(nfloat * sizeof(float)); return p; }
};
template <class WS>
static void carve_lpips_reserve(WS& ws, long long n, const LpGeo& g, LpReserve& r) {
    for (int k = 0; k < 5; ++k) r.tap[k] = ws.take((size_t)2 * n * g.h[LP_TAP_STAGE[k]] * g.w[LP_TAP_STAGE[k]] * LP_TAP_C[k]);
}

// The backward's workspace, over the n prediction images. The gradients alternate between two slots: P holds the gradients of taps 5, 3,
// 2 and 1 (a head works in place on what the layer behind it left there), Q that of tap 4 and those of the two pooled maps. `conv` is
// handed to the public data-gradient call of the stride-1 layers, one after the other, sized by that call's own query.
struct LpBwdSlots { float *wT, *P, *Q, *conv; size_t conv_bytes; };
template <class WS>
static int carve_lpips_bwd(WS& ws, long long n, const LpGeo& g, LpBwdSlots& s) {
    const size_t px0 = (size_t)g.h[0] * g.w[0], px1 = (size_t)g.h[1] * g.w[1], px2 = (size_t)g.h[2] * g.w[2];
    size_t p = px0 * 64, q = px1 * 64;
    if (px1 * 192 > p) p = px1 * 192;
    if (px2 * 384 > p) p = px2 * 384;
    if (px2 * 256 > q) q = px2 * 256;
    s.wT = ws.take(ST_PACK_FLOATS);
    s.P = ws.take((size_t)n * p);
    s.Q = ws.take((size_t)n * q);
    s.conv_bytes = 0;
    for (int l = 0; l < 4; ++l) {
        const vpx_conv_desc d = lp_desc(l, n, g);
        const size_t b = vpx_conv2d_ex_bwd_workspace_bytes(&d);
        if (!b) return VPX_ERR_UNSUPPORTED;
        if (b > s.conv_bytes) s.conv_bytes = b;
    }
    s.conv = ws.take((s.conv_bytes + sizeof(float) - 1) / sizeof(float));
    return VPX_OK;
}

// The forward of both entry points: the same launches in the same order; `tap` and `pooled` say where the maps go (vpx_lpips_fwd: the two
// slots in turn; vpx_lpips_fwd_train: the taps into the reserve).
static int lpips_forward(const char* who, const float* pred, const float* target, long long n, int H, int W, const float* const* params, double* table,
                         const LpGeo& g, const LpSlots& s, float* const tap[5], float* const pooled[2], hipStream_t stream) {
    const float* const* cw = params;        // conv1 .. conv5 weights [Co, Ci, k, k]
    const float* const* cb = params + 5;    // their biases
    const float* const* lin = params + 10;  // lin1 .. lin5 [C]
    const long long n2 = 2 * n;
    double* partial = reinterpret_cast<double*>(s.partial);
    VPX_CHECK_HIP(vpx_memset_async(table, 0, (size_t)n * sizeof(double), stream));
    auto head = [&](int k) {   // prediction: images 0 .. n-1 of the batch, target: n .. 2n-1
        const long long HW = (long long)g.h[LP_TAP_STAGE[k]] * g.w[LP_TAP_STAGE[k]];
        return lp_head(who, tap[k], tap[k] + n * HW * LP_TAP_C[k], g_dry_run ? nullptr : lin[k], n, HW, LP_TAP_C[k], table, partial, stream);
    };
    auto conv = [&](int l, const float* x, float* y) {
        const vpx_conv_desc d = lp_desc(l, n2, g);
        GlueGeo gg;
        GlueChoice c;
        if (int rc = glue_check(&d, gg)) return rc;
        glue_route(&d, gg, false, VPX_ACT_RELU, false, c);
        if (!ws_write_ok(y, (size_t)n2 * gg.Ho * gg.Wo * d.Co * sizeof(float), "feature map (convolution)")) { set_error("%s: %s", who, ws_violation()); ws_violation_clear(); return (int)VPX_ERR_WORKSPACE; }
        if (c.pack_bytes > s.pack_bytes[l]) { set_error("%s: weight pack of layer %d outgrew its slot", who, l + 2); return (int)VPX_ERR_WORKSPACE; }
        GlueIO io{};
        io.x = x; io.x_bstride = (long long)d.H * d.W * d.Ci * 4; io.w = g_dry_run ? nullptr : cw[l + 1]; io.bias = g_dry_run ? nullptr : cb[l + 1];
        io.y = y; io.wpk = reinterpret_cast<char*>(s.wpk[l]); io.act = VPX_ACT_RELU;
        return glue_forward(&d, gg, c, io, stream);
    };
    int rc;
    if ((rc = lp_stem(who, pred, target, n, n, H, W, g_dry_run ? nullptr : cw[0], g_dry_run ? nullptr : cb[0], tap[0], s.wT, stream))) return rc;
    if ((rc = head(0))) return rc;
    if ((rc = lp_pool(who, tap[0], pooled[0], n2, g.h[0], g.w[0], 64, stream))) return rc;
    if ((rc = conv(0, pooled[0], tap[1]))) return rc;
    if ((rc = head(1))) return rc;
    if ((rc = lp_pool(who, tap[1], pooled[1], n2, g.h[1], g.w[1], 192, stream))) return rc;
    if ((rc = conv(1, pooled[1], tap[2]))) return rc;
    if ((rc = head(2))) return rc;
    if ((rc = conv(2, tap[2], tap[3]))) return rc;
    if ((rc = head(3))) return rc;
    if ((rc = conv(3, tap[3], tap[4]))) return rc;
    return head(4);
}

// The stand-alone stem (either direction) and head: one slot each
template <class WS>
static void carve_lpips_stem(WS& ws, float*& wT) { wT = ws.take(ST_PACK_FLOATS); }
template <class WS>
static void carve_lpips_head(WS& ws, long long n, long long HW, double*& partial) {   // (take() counts floats: a double is two)
    partial = reinterpret_cast<double*>(ws.take((size_t)n * lp_head_chunks(HW) * 2));
}

static int lpips_params_check(const char* who, const float* const* params) {
    if (!g_dry_run)   // (a dry run hands over an address it never reads)
        for (int i = 0; i < 15; ++i)
            if (!params[i]) { set_error("%s: params[%d] is NULL", who, i); return VPX_ERR_ARG; }
    return VPX_OK;
}

}  // namespace vpx

using namespace vpx;

extern "C" {

size_t vpx_lpips_stem_workspace_bytes(void) {
    CarveMeasure m; float* wT;
    carve_lpips_stem(m, wT);
    return m.off + 256;
}

int vpx_lpips_stem_fwd(const float* x0, const float* x1, long long n0, long long n1, int H, int W, const float* w, const float* bias, float* y,
                       void* workspace, size_t workspace_bytes, void* stream_) {
    if (!x0 || !w || !bias || !y || (n1 > 0 && !x1)) { set_error("vpx_lpips_stem_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (n0 < 1 || n1 < 0) { set_error("vpx_lpips_stem_fwd: image counts must be >= 1 and >= 0 (got %lld, %lld)", n0, n1); return VPX_ERR_ARG; }
    if (H < LP_K - 2 * LP_PAD || W < LP_K - 2 * LP_PAD) { set_error("vpx_lpips_stem_fwd: images must be at least 7x7 for the padded 11x11 window (got %dx%d)", H, W); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lpips_stem_workspace_bytes()) { set_error("vpx_lpips_stem_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wT;
    carve_lpips_stem(ws, wT);
    VPX_CHECK_CARVE(ws, "vpx_lpips_stem_fwd");
    return lp_stem("vpx_lpips_stem_fwd", x0, x1, n0, n1, H, W, w, bias, y, wT, (hipStream_t)stream_);
}

int vpx_lpips_maxpool_fwd(const float* x, float* y, long long N, int H, int W, int C, void* stream_) {
    if (!x || !y) { set_error("vpx_lpips_maxpool_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (N < 1 || C < 1 || H < 3 || W < 3) { set_error("vpx_lpips_maxpool_fwd: N, C must be >= 1 and the map at least 3x3 (got N=%lld C=%d %dx%d)", N, C, H, W); return VPX_ERR_ARG; }
    return lp_pool("vpx_lpips_maxpool_fwd", x, y, N, H, W, C, (hipStream_t)stream_);
}

size_t vpx_lpips_head_workspace_bytes(long long n, long long HW) {
    if (n < 1 || HW < 1) return 0;
    CarveMeasure m; double* partial;
    carve_lpips_head(m, n, HW, partial);
    return m.off + 256;
}

int vpx_lpips_head_fwd(const float* fx, const float* fy, const float* w, long long n, long long HW, int C, double* table, void* workspace,
                       size_t workspace_bytes, void* stream_) {
    if (!fx || !fy || !w || !table) { set_error("vpx_lpips_head_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (n < 1 || HW < 1 || C < 1) { set_error("vpx_lpips_head_fwd: n, HW and C must be >= 1 (got %lld, %lld, %d)", n, HW, C); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lpips_head_workspace_bytes(n, HW)) { set_error("vpx_lpips_head_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    double* partial;
    carve_lpips_head(ws, n, HW, partial);
    VPX_CHECK_CARVE(ws, "vpx_lpips_head_fwd");
    return lp_head("vpx_lpips_head_fwd", fx, fy, w, n, HW, C, table, partial, (hipStream_t)stream_);
}

size_t vpx_lpips_workspace_bytes(long long n_frames, int H, int W) {
    if (lpips_check("vpx_lpips_workspace_bytes", n_frames, 3, H, W) != VPX_OK) return 0;
    LpGeo g;
    lp_geo(H, W, g);
    CarveMeasure m;
    LpSlots s{};
    if (carve_lpips(m, n_frames, g, s) != VPX_OK) return 0;
    return m.off + 256;
}

int vpx_lpips_fwd(const float* pred, const float* target, long long n_frames, int C, int H, int W, const float* const* params, double* table,
                  void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_lpips_fwd";
    if (!pred || !target || !params || !table) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (int rc = lpips_check(who, n_frames, C, H, W)) return rc;
    if (int rc = lpips_params_check(who, params)) return rc;
    if (!workspace || workspace_bytes < vpx_lpips_workspace_bytes(n_frames, H, W)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    LpGeo g;
    lp_geo(H, W, g);
    Carver ws(workspace, workspace_bytes);
    LpSlots s{};
    if (int rc = carve_lpips(ws, n_frames, g, s)) return rc;
    VPX_CHECK_CARVE(ws, who);
    float* const tap[5] = {s.A, s.A, s.A, s.B, s.A};   // a tap is read by its head and by the next layer only
    float* const pooled[2] = {s.B, s.B};
    return lpips_forward(who, pred, target, n_frames, H, W, params, table, g, s, tap, pooled, (hipStream_t)stream_);
}

size_t vpx_lpips_reserve_bytes(long long n_frames, int H, int W) {
    if (lpips_check("vpx_lpips_reserve_bytes", n_frames, 3, H, W) != VPX_OK) return 0;
    LpGeo g;
    lp_geo(H, W, g);
    CarveMeasure m;
    LpReserve r{};
    carve_lpips_reserve(m, n_frames, g, r);
    return m.off + 256;
}

int vpx_lpips_fwd_train(const float* pred, const float* target, long long n_frames, int C, int H, int W, const float* const* params, double* table,
                        void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_lpips_fwd_train";
    if (!pred || !target || !params || !table) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (int rc = lpips_check(who, n_frames, C, H, W)) return rc;
    if (int rc = lpips_params_check(who, params)) return rc;
    if (!workspace || workspace_bytes < vpx_lpips_workspace_bytes(n_frames, H, W)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    if (!reserve || reserve_bytes < vpx_lpips_reserve_bytes(n_frames, H, W)) { set_error("%s: reserve too small", who); return VPX_ERR_WORKSPACE; }
    LpGeo g;
    lp_geo(H, W, g);
    Carver ws(workspace, workspace_bytes);
    LpSlots s{};
    if (int rc = carve_lpips(ws, n_frames, g, s)) return rc;
    VPX_CHECK_CARVE(ws, who);
    Carver keep(reserve, reserve_bytes);   // (registered like the workspace: a tap that outgrew its slot is an error, not a write)
    LpReserve r{};
    carve_lpips_reserve(keep, n_frames, g, r);
    VPX_CHECK_CARVE(keep, who);
    float* const pooled[2] = {s.B, s.B};
    return lpips_forward(who, pred, target, n_frames, H, W, params, table, g, s, r.tap, pooled, (hipStream_t)stream_);
}

int vpx_lpips_head_bwd(const float* fx, const float* fy, const float* w, const double* dtable, const float* incoming, long long n, long long HW, int C,
                       float* dz, void* stream_) {
    if (!fx || !fy || !w || !dtable || !dz) { set_error("vpx_lpips_head_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (n < 1 || HW < 1 || C < 1) { set_error("vpx_lpips_head_bwd: n, HW and C must be >= 1 (got %lld, %lld, %d)", n, HW, C); return VPX_ERR_ARG; }
    return lp_head_bwd("vpx_lpips_head_bwd", fx, fy, w, dtable, incoming, n, HW, C, dz, (hipStream_t)stream_);
}

int vpx_lpips_maxpool_bwd(const float* x, const float* dy, float* dx, long long N, int H, int W, int C, void* stream_) {
    if (!x || !dy || !dx) { set_error("vpx_lpips_maxpool_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (N < 1 || C < 1 || H < 3 || W < 3) { set_error("vpx_lpips_maxpool_bwd: N, C must be >= 1 and the map at least 3x3 (got N=%lld C=%d %dx%d)", N, C, H, W); return VPX_ERR_ARG; }
    return lp_pool_bwd("vpx_lpips_maxpool_bwd", x, dy, dx, N, H, W, C, (hipStream_t)stream_);
}

int vpx_lpips_stem_bwd(const float* x, const float* w, const float* dz, long long n, int H, int W, float* dx, void* workspace, size_t workspace_bytes,
                       void* stream_) {
    if (!x || !w || !dz || !dx) { set_error("vpx_lpips_stem_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (n < 1) { set_error("vpx_lpips_stem_bwd: the image count must be >= 1 (got %lld)", n); return VPX_ERR_ARG; }
    if (H < LP_K - 2 * LP_PAD || W < LP_K - 2 * LP_PAD) { set_error("vpx_lpips_stem_bwd: images must be at least 7x7 for the padded 11x11 window (got %dx%d)", H, W); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lpips_stem_workspace_bytes()) { set_error("vpx_lpips_stem_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wT;
    carve_lpips_stem(ws, wT);
    VPX_CHECK_CARVE(ws, "vpx_lpips_stem_bwd");
    return lp_stem_bwd("vpx_lpips_stem_bwd", x, w, dz, n, H, W, dx, wT, (hipStream_t)stream_);
}

size_t vpx_lpips_bwd_workspace_bytes(long long n_frames, int H, int W) {
    if (lpips_check("vpx_lpips_bwd_workspace_bytes", n_frames, 3, H, W) != VPX_OK) return 0;
    LpGeo g;
    lp_geo(H, W, g);
    CarveMeasure m;
    LpBwdSlots s{};
    if (carve_lpips_bwd(m, n_frames, g, s) != VPX_OK) return 0;
    return m.off + 256;
}

int vpx_lpips_bwd(const float* pred, const float* const* params, const void* reserve, const double* dtable, long long n_frames, int C, int H, int W,
                  float* dpred, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_lpips_bwd";
    if (!pred || !params || !reserve || !dtable || !dpred) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (int rc = lpips_check(who, n_frames, C, H, W)) return rc;
    if (int rc = lpips_params_check(who, params)) return rc;
    if (!workspace || workspace_bytes < vpx_lpips_bwd_workspace_bytes(n_frames, H, W)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    LpGeo g;
    lp_geo(H, W, g);
    Carver ws(workspace, workspace_bytes);
    LpBwdSlots s{};
    if (int rc = carve_lpips_bwd(ws, n_frames, g, s)) return rc;
    VPX_CHECK_CARVE(ws, who);
    LpReserve r{};
    CarveRead keep(reserve);
    carve_lpips_reserve(keep, n_frames, g, r);
    const long long n = n_frames;
    const float* const* cw = params;
    const float* const* lin = params + 10;
    auto head = [&](int k, const float* incoming, float* dz) {   // the target half of a tap serves as fy
        const long long HW = (long long)g.h[LP_TAP_STAGE[k]] * g.w[LP_TAP_STAGE[k]];
        return lp_head_bwd(who, r.tap[k], r.tap[k] + n * HW * LP_TAP_C[k], g_dry_run ? nullptr : lin[k], dtable, incoming, n, HW, LP_TAP_C[k], dz, stream);
    };
    // The data gradient of stride-1 layer l (taps 2 .. 5) on the public glue backward: exact fp32 operands, no activation (the head has
    // applied the mask), dw and db not requested. Without dw the call never reads the layer's input: it is handed dz as a placeholder.
    auto dgrad = [&](int l, const float* dz, float* dx) {
        const vpx_conv_desc d = lp_desc(l, n, g);
        if (!ws_write_ok(dx, (size_t)n * d.H * d.W * d.Ci * sizeof(float), "layer input gradient (convolution)")) { set_error("%s: %s", who, ws_violation()); ws_violation_clear(); return (int)VPX_ERR_WORKSPACE; }
        const float* wt = g_dry_run ? dz : cw[l + 1];
        return vpx_conv2d_ex_bwd(&d, dz, wt, nullptr, dz, dx, nullptr, nullptr, s.conv, s.conv_bytes, stream_);
    };
    int rc;
    if ((rc = head(4, nullptr, s.P))) return rc;
    if ((rc = dgrad(3, s.P, s.Q))) return rc;
    if ((rc = head(3, s.Q, s.Q))) return rc;
    if ((rc = dgrad(2, s.Q, s.P))) return rc;
    if ((rc = head(2, s.P, s.P))) return rc;
    if ((rc = dgrad(1, s.P, s.Q))) return rc;
    if ((rc = lp_pool_bwd(who, r.tap[1], s.Q, s.P, n, g.h[1], g.w[1], 192, stream))) return rc;
    if ((rc = head(1, s.P, s.P))) return rc;
    if ((rc = dgrad(0, s.P, s.Q))) return rc;
    if ((rc = lp_pool_bwd(who, r.tap[0], s.Q, s.P, n, g.h[0], g.w[0], 64, stream))) return rc;
    if ((rc = head(0, s.P, s.P))) return rc;
    return lp_stem_bwd(who, pred, g_dry_run ? nullptr : cw[0], s.P, n, H, W, dpred, s.wT, stream);
}

}  // extern "C"
