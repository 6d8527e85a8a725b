// LPIPS on an AlexNet trunk (https://arxiv.org/abs/1801.03924; vp_suite/measure/image_wise.py's LPIPS through piqa), forward only, fp32,
// no floating-point atomics — bit-reproducible. The trunk runs channels-last (NHWC), the layout of the library's convolutions:
//   vpx_lpips_stem_fwd      clamp((v+1)/2, 0, 1) and the ImageNet normalisation fused into the operand load of the 11x11 stride-4 pad-2
//                           convolution 3 -> 64, bias, ReLU. The padding ring is zero in NORMALISED space.
//   vpx_lpips_maxpool_fwd   3x3 stride-2 max-pool, floor mode, no padding
//   vpx_lpips_head_fwd      per pixel: both channel norms, sum_c w[c] (fx/(|fx|+1e-10) - fy/(|fy|+1e-10))^2; per image: the pixel mean,
//                           ADDED into a float64 table. Every feature element is read once; the normalised maps never exist in memory.
//   vpx_lpips_fwd           the whole measure: prediction and target as ONE batch of 2n images through stem, pools and the four stride-1
//                           "same" convolutions + ReLU (the library's implicit-GEMM kernel with ReLU in its epilogue: glue_forward with
//                           VPX_ACT_RELU, exact fp32 operands), one head launch per tap.
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

// ---- host side: the three launchers, shared by their own entry points and the trunk --------------------------------------------------
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

}  // namespace vpx

using namespace vpx;

extern "C" {

size_t vpx_lpips_stem_workspace_bytes(void) { return align256(ST_PACK_FLOATS * sizeof(float)) + 256; }

int vpx_lpips_stem_fwd(const float* x0, const float* x1, long long n0, long long n1, int H, int W, const float* w, const float* bias, float* y,
                       void* workspace, size_t workspace_bytes, void* stream_) {
    if (!x0 || !w || !bias || !y || (n1 > 0 && !x1)) { set_error("vpx_lpips_stem_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (n0 < 1 || n1 < 0) { set_error("vpx_lpips_stem_fwd: image counts must be >= 1 and >= 0 (got %lld, %lld)", n0, n1); return VPX_ERR_ARG; }
    if (H < LP_K - 2 * LP_PAD || W < LP_K - 2 * LP_PAD) { set_error("vpx_lpips_stem_fwd: images must be at least 7x7 for the padded 11x11 window (got %dx%d)", H, W); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lpips_stem_workspace_bytes()) { set_error("vpx_lpips_stem_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* wT = ws.take(ST_PACK_FLOATS);
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
    return align256((size_t)n * lp_head_chunks(HW) * sizeof(double)) + 256;
}

int vpx_lpips_head_fwd(const float* fx, const float* fy, const float* w, long long n, long long HW, int C, double* table, void* workspace,
                       size_t workspace_bytes, void* stream_) {
    if (!fx || !fy || !w || !table) { set_error("vpx_lpips_head_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (n < 1 || HW < 1 || C < 1) { set_error("vpx_lpips_head_fwd: n, HW and C must be >= 1 (got %lld, %lld, %d)", n, HW, C); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lpips_head_workspace_bytes(n, HW)) { set_error("vpx_lpips_head_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    double* partial = reinterpret_cast<double*>(ws.take((size_t)n * lp_head_chunks(HW) * 2));
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
    const float* const* cw = params;        // conv1 .. conv5 weights [Co, Ci, k, k]
    const float* const* cb = params + 5;    // their biases
    const float* const* lin = params + 10;  // lin1 .. lin5 [C]
    if (!g_dry_run)   // (a dry run hands over an address it never reads)
        for (int i = 0; i < 15; ++i)
            if (!params[i]) { set_error("%s: params[%d] is NULL", who, i); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lpips_workspace_bytes(n_frames, H, W)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    LpGeo g;
    lp_geo(H, W, g);
    Carver ws(workspace, workspace_bytes);
    LpSlots s{};
    if (int rc = carve_lpips(ws, n_frames, g, s)) return rc;
    VPX_CHECK_CARVE(ws, who);
    const long long n = n_frames, n2 = 2 * n_frames;
    double* partial = reinterpret_cast<double*>(s.partial);
    VPX_CHECK_HIP(vpx_memset_async(table, 0, (size_t)n * sizeof(double), stream));
    auto head = [&](const float* f, int stage, int Cf, int tap) {   // prediction: images 0 .. n-1 of the batch, target: n .. 2n-1
        const long long HW = (long long)g.h[stage] * g.w[stage];
        return lp_head(who, f, f + n * HW * Cf, g_dry_run ? nullptr : lin[tap], n, HW, Cf, table, partial, stream);
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
    if ((rc = lp_stem(who, pred, target, n, n, H, W, g_dry_run ? nullptr : cw[0], g_dry_run ? nullptr : cb[0], s.A, s.wT, stream))) return rc;
    if ((rc = head(s.A, 0, 64, 0))) return rc;
    if ((rc = lp_pool(who, s.A, s.B, n2, g.h[0], g.w[0], 64, stream))) return rc;
    if ((rc = conv(0, s.B, s.A))) return rc;
    if ((rc = head(s.A, 1, 192, 1))) return rc;
    if ((rc = lp_pool(who, s.A, s.B, n2, g.h[1], g.w[1], 192, stream))) return rc;
    if ((rc = conv(1, s.B, s.A))) return rc;
    if ((rc = head(s.A, 2, 384, 2))) return rc;
    if ((rc = conv(2, s.A, s.B))) return rc;
    if ((rc = head(s.B, 2, 256, 3))) return rc;
    if ((rc = conv(3, s.B, s.A))) return rc;
    return head(s.A, 2, 256, 4);
}

}  // extern "C"
