// Frechet Video Distance on an Inception-I3D trunk (https://arxiv.org/abs/1812.01717; vp_suite/measure/fvd), forward only, fp32
// activations, no floating-point atomics — bit-reproducible. Activations are channels-last [N, T, H, W, C].
//   vpx_conv3d_same      Unit3D: zero-padded 3-D convolution with TensorFlow "SAME" padding, any kernel and stride, bias and optional ReLU,
//                        written at a channel offset into a buffer of a larger channel stride (the four branches of an Inception block
//                        land in one tensor). Implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): M = output positions,
//                        N = output channels, K = (kt, kh) rows of kw * Ci CONTIGUOUS input elements each — so the 7x7x7 stem over 2 or 3
//                        channels fills its K steps with 14 or 21 elements per row instead of 2 or 3.
//   vpx_maxpool3d_same   max-pool over the ZERO-padded map ("SAME" padding, as the reference pads before it pools): a window on the
//                        border never returns less than 0.
//   vpx_fvd_head         mean over the final 2x7x7 map, then the 1x1x1 logits layer with bias: [N, n_features]
//   vpx_fvd_features     the whole trunk over a layer table: bilinear resize of [B, T, C, h, w] frames to 224x224 straight into the stem's
//                        layout (frames_coord.h: bit-equal to vpx_frames_adapt's resize), then the table's rows, then the head
//   vpx_frechet_distance the 2-Wasserstein distance of two [b, n] feature tables in float64: centring, the b x b matrix fact * Ep Et^T, its
//                        singular values by a one-sided Jacobi iteration with a FIXED maximum of sweeps, one float64 scalar on the device
#include <hip/hip_runtime.h>
#include <math.h>
#include "vpx_internal.h"
#include "vpx_host.h"

// (frames_coord.h asks for it: every operation of the resize is rounded on its own)
#pragma clang fp contract(off)

#include "frames_coord.h"

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr long long FV_MAX_GRID = 0x7fffffffLL;
constexpr int FV_SIDE = 224;        // the I3D input
constexpr int FV_MAX_SIDE = 32768;
constexpr int FV_MAX_K = 15;        // kernel sides
constexpr int FV_MAX_C = 65536;     // channel counts and strides

// ---- "SAME" padding: pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0); front = pad / 2; out = ceil(size / s) -----------
static inline void fv_same(int size, int k, int s, int& front, int& out) {
    const int pad = size % s == 0 ? (k - s > 0 ? k - s : 0) : (k - size % s > 0 ? k - size % s : 0);
    front = pad / 2;
    out = (size + s - 1) / s;
}

// ---- Unit3D --------------------------------------------------------------------------------------------------------------------------
// A workgroup of four waves computes 64 output positions x 64 output channels, a wave 32 x 32 of them. Per (kt, kh) row and per 16
// elements of the row's kw * Ci run: the A tile [64 positions][16] (zero where the row or the element lies in the padding) and the B tile
// [16][64 channels] of the packed weights [kt][kh][kw * Ci][Co] go through LDS; eight 32x32x2 MFMAs per wave consume them. Every output's
// sum runs over K in one fixed order, whatever tile the output lies in: a batch of 2B gives the bits of two batches of B.
constexpr int FC_THREADS = 256, FC_M = 64, FC_N = 64, FC_K = 16, FC_APITCH = FC_K + 1;

struct FvConv {
    const float* x;      // [N, T, H, W, Ci] dense
    const float* wp;     // [kt][kh][kw * Ci][Co]
    const float* bias;   // [Co]
    float* y;            // [N, To, Ho, Wo, ldy], written at channels coff .. coff + Co - 1
    long long M;         // N * To * Ho * Wo
    int T, H, W, Ci, To, Ho, Wo, Co;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
    int run;             // kw * Ci
    int ldy, coff, relu;
    int vecA, vecB;      // 16-byte loads: Ci % 4 == 0 and x aligned; Co % 4 == 0 and wp aligned
};

__global__ __launch_bounds__(FC_THREADS) void fvd_conv3d_kernel(FvConv a) {
    __shared__ float As[FC_M * FC_APITCH];
    __shared__ __attribute__((aligned(16))) float Bs[FC_K * FC_N];
    const int tid = threadIdx.x;
    // ---- the thread's share of the A tile: position m_l, elements 4 q .. 4 q + 3 of the 16 ----
    const int m_l = tid >> 2, q = tid & 3;
    const long long m = (long long)blockIdx.x * FC_M + m_l;
    const bool mvalid = m < a.M;
    long long r = mvalid ? m : 0;
    const int ow = (int)(r % a.Wo); r /= a.Wo;
    const int oh = (int)(r % a.Ho); r /= a.Ho;
    const int ot = (int)(r % a.To);
    const long long n = r / a.To;
    const int it0 = ot * a.st - a.pt, ih0 = oh * a.sh - a.ph, iw0 = ow * a.sw - a.pw;
    const int lo_e = (iw0 < 0 ? -iw0 : 0) * a.Ci;                                   // elements of the run inside the map: [lo_e, hi_e)
    const int hi_e = mvalid ? (a.W - iw0 < a.kw ? a.W - iw0 : a.kw) * a.Ci : 0;
    // ---- the thread's share of the B tile: row kb, channels co0 .. co0 + 3 ----
    const int kb = tid >> 4, nb = (tid & 15) * 4;
    const int co0 = blockIdx.y * FC_N + nb;
    const int lane = tid & 63, wave = tid >> 6, hh = lane >> 5, li = lane & 31;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
    for (int dt = 0; dt < a.kt; ++dt)
        for (int dh = 0; dh < a.kh; ++dh) {
            const int it = it0 + dt, ih = ih0 + dh;
            const bool rowvalid = mvalid && it >= 0 && it < a.T && ih >= 0 && ih < a.H;
            // (the address of element 0 of the run: it may lie before the row where iw0 < 0 — only elements in [lo_e, hi_e) are read)
            const long long xoff = rowvalid ? (((n * a.T + it) * a.H + ih) * (long long)a.W + iw0) * a.Ci : 0;
            const float* wrow = a.wp + (size_t)(dt * a.kh + dh) * a.run * a.Co;
            for (int e0 = 0; e0 < a.run; e0 += FC_K) {
                const int e = e0 + 4 * q;
                float av[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (rowvalid) {
                    if (a.vecA) {   // lo_e, hi_e and e are multiples of 4: a group is inside or outside as a whole
                        if (e >= lo_e && e + 4 <= hi_e) {
                            const f32x4 v4 = *reinterpret_cast<const f32x4*>(a.x + xoff + e);
#pragma unroll
                            for (int j = 0; j < 4; ++j) av[j] = v4[j];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (e + j >= lo_e && e + j < hi_e) av[j] = a.x[xoff + e + j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) As[m_l * FC_APITCH + 4 * q + j] = av[j];
                const int ek = e0 + kb;
                float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (ek < a.run) {
                    if (a.vecB) {   // Co and co0 are multiples of 4
                        if (co0 < a.Co) {
                            const f32x4 v4 = *reinterpret_cast<const f32x4*>(wrow + (size_t)ek * a.Co + co0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) bv[j] = v4[j];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (co0 + j < a.Co) bv[j] = wrow[(size_t)ek * a.Co + co0 + j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) Bs[kb * FC_N + nb + j] = bv[j];
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < FC_K; kk += 2)   // lanes 0-31 supply k = kk, lanes 32-63 k = kk + 1, for both operands
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(wm + li) * FC_APITCH + kk + hh], Bs[(kk + hh) * FC_N + wn + li], acc, 0, 0, 0);
                __syncthreads();
            }
        }
    // ---- bias, ReLU, store: acc[v] is position wm + (v & 3) + 8 (v >> 2) + 4 hh, channel wn + li ----
    const int co = blockIdx.y * FC_N + wn + li;
    if (co >= a.Co) return;
    const float b = a.bias[co];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const long long mo = (long long)blockIdx.x * FC_M + wm + (v & 3) + 8 * (v >> 2) + 4 * hh;
        if (mo >= a.M) continue;
        float o = acc[v] + b;
        if (a.relu) o = (o > 0.0f || o != o) ? o : 0.0f;   // NaN stays NaN, as in torch; every other value as before, -0 included
        a.y[mo * a.ldy + a.coff + co] = o;
    }
}

// ---- max-pool over the zero-padded map: one thread per output element, channels fastest ----------------------------------------------
constexpr int FP_THREADS = 256;
struct FvPool {
    const float* x;   // [N, T, H, W, C]
    float* y;         // [N, To, Ho, Wo, C]
    long long total;
    int T, H, W, C, To, Ho, Wo;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
};

__global__ __launch_bounds__(FP_THREADS) void fvd_maxpool3d_kernel(FvPool a) {
    const long long i = (long long)blockIdx.x * FP_THREADS + threadIdx.x;
    if (i >= a.total) return;
    const int c = (int)(i % a.C);
    long long p = i / a.C;
    const int ow = (int)(p % a.Wo); p /= a.Wo;
    const int oh = (int)(p % a.Ho); p /= a.Ho;
    const int ot = (int)(p % a.To);
    const long long n = p / a.To;
    float m = 0.0f;
    bool first = true;
    for (int dt = 0; dt < a.kt; ++dt)
        for (int dh = 0; dh < a.kh; ++dh)
            for (int dw = 0; dw < a.kw; ++dw) {
                const int it = ot * a.st - a.pt + dt, ih = oh * a.sh - a.ph + dh, iw = ow * a.sw - a.pw + dw;
                float v = 0.0f;   // the padding is part of the pooled map
                if (it >= 0 && it < a.T && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) v = a.x[(((n * a.T + it) * a.H + ih) * (long long)a.W + iw) * a.C + c];
                if (first) { m = v; first = false; }
                else m = (v > m || v != v) ? v : m;   // NaN wins, as in torch
            }
    a.y[i] = m;
}

// ---- head: the mean over the map's positions (double), then out[n][f] = bias[f] + sum_c w[f][c] mean[c] (double, rounded once) ------
constexpr int FH_THREADS = 256, FH_MAX_C = 4096, FH_T = 2, FH_S = 7;
__global__ __launch_bounds__(FH_THREADS) void fvd_head_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                              int P, int C, int F, float* __restrict__ out) {
    __shared__ double mean[FH_MAX_C];
    const long long n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += FH_THREADS) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += (double)x[(n * P + p) * C + c];
        mean[c] = s / (double)P;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int f = wave; f < F; f += FH_THREADS / 64) {
        double s = 0.0;
        for (int c = lane; c < C; c += 64) s = fma((double)w[(size_t)f * C + c], mean[c], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) out[n * F + f] = (float)(s + (double)bias[f]);
    }
}

// ---- input staging: [B, T, C, h, w] planar frames (two sources, one behind the other) -> [N, T, S, S, C] ----------------------------------
// The taps and weights of frames_coord.h and the arithmetic of adapt.hip's resize, operation for operation: horizontally first,
// v0 * (1 - l) + v1 * l, then the same vertically. Equal sizes: a copy.
constexpr int FS_THREADS = 256;
struct FvStage {
    const float *x0, *x1;   // frames of the first n0 and of the following videos
    float* y;
    long long n0, total;    // total = N * T * S * S output pixels
    int T, C, h, w, S, resize;
    float sy, sx;
};

__global__ __launch_bounds__(FS_THREADS) void fvd_stage_kernel(FvStage a) {
    const long long i = (long long)blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= a.total) return;
    const int x = (int)(i % a.S);
    long long p = i / a.S;
    const int y = (int)(p % a.S); p /= a.S;
    const int t = (int)(p % a.T);
    const long long n = p / a.T;
    const size_t plane = (size_t)a.h * a.w;
    const float* src = (n < a.n0 ? a.x0 + (size_t)n * a.T * a.C * plane : a.x1 + (size_t)(n - a.n0) * a.T * a.C * plane) + (size_t)t * a.C * plane;
    float* dst = a.y + (size_t)i * a.C;
    if (!a.resize) {
        for (int c = 0; c < a.C; ++c) dst[c] = src[c * plane + (size_t)y * a.w + x];
        return;
    }
    int iy0, iy1, ix0, ix1;
    float ly, lx;
    fr_coord(a.sy, y, a.h, iy0, iy1, ly);
    fr_coord(a.sx, x, a.w, ix0, ix1, lx);
    const float wy = 1.0f - ly, wx = 1.0f - lx;
    for (int c = 0; c < a.C; ++c) {
        const float* top = src + c * plane + (size_t)iy0 * a.w;
        const float* bot = src + c * plane + (size_t)iy1 * a.w;
        const float tv = top[ix0] * wx + top[ix1] * lx;
        const float uv = bot[ix0] * wx + bot[ix1] * lx;
        dst[c] = tv * wy + uv * ly;
    }
}

// ---- Frechet distance ------------------------------------------------------------------------------------------------------------------
// d = fact sum Ep^2 + fact sum Et^2 - 2 sum_i sqrt(sigma_i^2 + 1e-15) + |mu_p - mu_t|^2, sigma_i the singular values of G = fact Ep Et^T
// (b x b; E the centred tables, fact = 1 / (b - 1), 1 for b = 1). All of it in float64, every sum in one fixed order.
constexpr int FD_MAX_B = 256;       // the cap on b: rows of a pair are held four elements per lane
// the fixed maximum of Jacobi sweeps (a sweep without a rotation ends the iteration; none within the maximum: NaN). Well-conditioned tables
// end within 15 sweeps at b = 256; tables whose singular values fall over nine decades (G's over eighteen) need 28 at b = 64, 36 at 129 and
// 44 .. 47 at 256 in this pair order, so the maximum leaves those a factor of 1.7
constexpr int FD_SWEEPS = 80;
constexpr int FD_THREADS = 1024, FD_WAVES = FD_THREADS / 64, FD_PER_LANE = FD_MAX_B / 64;
constexpr double FD_EPS = 1e-15;    // the reference's constant under the square root
constexpr double FD_TOL = 1e-13;    // rows count as orthogonal below this cosine: the error left in sum sigma is of its square

// one thread per feature k: both means, both centred columns, the feature's share of the three sums
__global__ void fvd_centre_kernel(const float* __restrict__ P, const float* __restrict__ Tg, int b, int n, double* __restrict__ Ep, double* __restrict__ Et,
                                  double* __restrict__ part) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double mp = 0.0, mt = 0.0;
    for (int i = 0; i < b; ++i) { mp += (double)P[(size_t)i * n + k]; mt += (double)Tg[(size_t)i * n + k]; }
    mp = mp / (double)b;
    mt = mt / (double)b;
    double sp = 0.0, st = 0.0;
    for (int i = 0; i < b; ++i) {
        const double ep = (double)P[(size_t)i * n + k] - mp, et = (double)Tg[(size_t)i * n + k] - mt;
        Ep[(size_t)i * n + k] = ep;
        Et[(size_t)i * n + k] = et;
        sp = fma(ep, ep, sp);
        st = fma(et, et, st);
    }
    part[k] = sp;
    part[n + k] = st;
    part[2 * n + k] = (mt - mp) * (mt - mp);
}

// one thread per element of G
__global__ void fvd_gram_kernel(const double* __restrict__ Ep, const double* __restrict__ Et, int b, int n, double fact, double* __restrict__ G) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= b * b) return;
    const int i = idx / b, j = idx % b;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s = fma(Ep[(size_t)i * n + k], Et[(size_t)j * n + k], s);
    G[idx] = fact * s;
}

static __device__ __forceinline__ double fd_wave_sum(double v) {   // every lane ends with the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One workgroup. One-sided Jacobi on the ROWS of G (the singular values of G and of its transpose are the same): a sweep is bp - 1
// rounds of bp / 2 disjoint row pairs (round-robin: player bp - 1 stays, the others rotate; bp = b rounded up to even, the extra player
// sits out), a wave per pair, the rows held in registers. After the last sweep the row norms are the singular values.
__global__ __launch_bounds__(FD_THREADS) void fvd_jacobi_kernel(double* G, int b, int n, double fact, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ int rotated;
    __shared__ double sig2[FD_MAX_B];
    __shared__ double sums[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bp = (b + 1) & ~1, rounds = bp - 1, pairs = bp / 2;
    bool converged = false;   // a sweep went by without a rotation (uniform over the workgroup)
    for (int sweep = 0; sweep < FD_SWEEPS; ++sweep) {
        if (threadIdx.x == 0) rotated = 0;
        __syncthreads();
        for (int r = 0; r < rounds; ++r) {
            for (int k = wave; k < pairs; k += FD_WAVES) {
                const int p = k == 0 ? bp - 1 : (r + k) % rounds, q = (r + rounds - k) % rounds;
                if (p >= b || q >= b) continue;
                double* gp = G + (size_t)p * b;
                double* gq = G + (size_t)q * b;
                double vp[FD_PER_LANE], vq[FD_PER_LANE], aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
                for (int j = 0; j < FD_PER_LANE; ++j) {
                    const int col = lane + 64 * j;
                    vp[j] = col < b ? gp[col] : 0.0;
                    vq[j] = col < b ? gq[col] : 0.0;
                    aa = fma(vp[j], vp[j], aa);
                    bb = fma(vq[j], vq[j], bb);
                    ab = fma(vp[j], vq[j], ab);
                }
                aa = fd_wave_sum(aa); bb = fd_wave_sum(bb); ab = fd_wave_sum(ab);
                if (ab == 0.0 || fabs(ab) <= FD_TOL * sqrt(aa) * sqrt(bb)) continue;   // (wave-uniform: the sums are)
                const double zeta = (bb - aa) / (2.0 * ab);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int j = 0; j < FD_PER_LANE; ++j) {
                    const int col = lane + 64 * j;
                    if (col < b) {
                        gp[col] = cs * vp[j] - sn * vq[j];
                        gq[col] = sn * vp[j] + cs * vq[j];
                    }
                }
                if (lane == 0) rotated = 1;
            }
            __syncthreads();   // the round's pairs are disjoint; the next round reads what this one wrote
        }
        const int any = rotated;
        __syncthreads();
        if (!any) { converged = true; break; }
    }
    for (int i = wave; i < b; i += FD_WAVES) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < FD_PER_LANE; ++j) {
            const int col = lane + 64 * j;
            const double v = col < b ? G[(size_t)i * b + col] : 0.0;
            s = fma(v, v, s);
        }
        s = fd_wave_sum(s);
        if (lane == 0) sig2[i] = s;
    }
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += part[threadIdx.x * n + k];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double root = 0.0;
        for (int i = 0; i < b; ++i) root += sqrt(sig2[i] + FD_EPS);
        // rows still rotating after the last sweep: the row norms are not singular values yet — NaN, never a number that looks like a distance
        out[0] = converged ? fact * sums[0] + fact * sums[1] - 2.0 * root + sums[2] : __longlong_as_double(0x7ff8000000000000LL);
    }
}

// ---- host side: the launchers, shared by their own entry points and the trunk ----------------------------------------------------------
struct FvGeo { int T, H, W, C; };   // a map [N, T, H, W, C]

static int fv_conv_check(const char* who, long long N, const FvGeo& g, int Co, const int k[3], const int s[3], int ldy, int coff) {
    if (N < 1 || g.T < 1 || g.H < 1 || g.W < 1 || g.C < 1 || Co < 1) { set_error("%s: every size must be >= 1 (got N=%lld map %dx%dx%d Ci=%d Co=%d)", who, N, g.T, g.H, g.W, g.C, Co); return VPX_ERR_ARG; }
    for (int i = 0; i < 3; ++i)
        if (k[i] < 1 || s[i] < 1) { set_error("%s: kernel and stride must be >= 1 (got kernel %dx%dx%d stride %dx%dx%d)", who, k[0], k[1], k[2], s[0], s[1], s[2]); return VPX_ERR_ARG; }
    if (coff < 0 || ldy < 1 || coff + (long long)Co > ldy) { set_error("%s: channels %d .. %d do not fit a channel stride of %d", who, coff, coff + Co - 1, ldy); return VPX_ERR_ARG; }
    for (int i = 0; i < 3; ++i)
        if (k[i] > FV_MAX_K || s[i] > FV_MAX_K) { set_error("%s: kernel and stride sides up to %d (got kernel %dx%dx%d stride %dx%dx%d)", who, FV_MAX_K, k[0], k[1], k[2], s[0], s[1], s[2]); return VPX_ERR_UNSUPPORTED; }
    if (g.T > FV_MAX_SIDE || g.H > FV_MAX_SIDE || g.W > FV_MAX_SIDE || g.C > FV_MAX_C || Co > FV_MAX_C || ldy > FV_MAX_C) { set_error("%s: a side beyond %d or a channel count beyond %d", who, FV_MAX_SIDE, FV_MAX_C); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

// y = act(conv(x) + bias) at channels coff.. of a map of channel stride ldy; `out` receives the output map's geometry (C = ldy)
static int fv_conv(const char* who, const float* x, const float* wp, const float* bias, float* y, long long N, const FvGeo& g, int Co, const int k[3],
                   const int s[3], int relu, int ldy, int coff, FvGeo& out, hipStream_t stream) {
    if (int rc = fv_conv_check(who, N, g, Co, k, s, ldy, coff)) return rc;
    FvConv a{};
    a.x = x; a.wp = wp; a.bias = bias; a.y = y;
    a.T = g.T; a.H = g.H; a.W = g.W; a.Ci = g.C; a.Co = Co;
    a.kt = k[0]; a.kh = k[1]; a.kw = k[2]; a.st = s[0]; a.sh = s[1]; a.sw = s[2];
    fv_same(g.T, k[0], s[0], a.pt, a.To);
    fv_same(g.H, k[1], s[1], a.ph, a.Ho);
    fv_same(g.W, k[2], s[2], a.pw, a.Wo);
    a.M = N * a.To * a.Ho * a.Wo;
    a.run = a.kw * a.Ci;
    a.ldy = ldy; a.coff = coff; a.relu = relu ? 1 : 0;
    a.vecA = (a.Ci % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
    a.vecB = (a.Co % 4 == 0 && ((uintptr_t)wp & 15) == 0) ? 1 : 0;
    out = FvGeo{a.To, a.Ho, a.Wo, ldy};
    const long long mt = (a.M + FC_M - 1) / FC_M;
    if (mt > FV_MAX_GRID || (double)N * g.T * g.H * g.W * g.C > 4.0e18 || (double)a.M * ldy > 4.0e18) { set_error("%s: %lld maps of %dx%dx%dx%d exceed one launch", who, N, g.T, g.H, g.W, g.C); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(y, (size_t)a.M * ldy * sizeof(float), "feature map (fvd_conv3d_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(fvd_conv3d_kernel, dim3((unsigned)mt, (unsigned)((Co + FC_N - 1) / FC_N)), dim3(FC_THREADS), 0, stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int fv_pool(const char* who, const float* x, float* y, long long N, const FvGeo& g, const int k[3], const int s[3], FvGeo& out, hipStream_t stream) {
    if (int rc = fv_conv_check(who, N, g, g.C, k, s, g.C, 0)) return rc;
    FvPool a{};
    a.x = x; a.y = y; a.T = g.T; a.H = g.H; a.W = g.W; a.C = g.C;
    a.kt = k[0]; a.kh = k[1]; a.kw = k[2]; a.st = s[0]; a.sh = s[1]; a.sw = s[2];
    fv_same(g.T, k[0], s[0], a.pt, a.To);
    fv_same(g.H, k[1], s[1], a.ph, a.Ho);
    fv_same(g.W, k[2], s[2], a.pw, a.Wo);
    out = FvGeo{a.To, a.Ho, a.Wo, g.C};
    if ((double)N * g.T * g.H * g.W * g.C > 4.0e18) { set_error("%s: %lld maps of %dx%dx%dx%d exceed one launch", who, N, g.T, g.H, g.W, g.C); return VPX_ERR_UNSUPPORTED; }
    a.total = N * a.To * a.Ho * a.Wo * g.C;
    const long long blocks = (a.total + FP_THREADS - 1) / FP_THREADS;
    if (blocks > FV_MAX_GRID) { set_error("%s: %lld maps of %dx%dx%dx%d exceed one launch", who, N, g.T, g.H, g.W, g.C); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(y, (size_t)a.total * sizeof(float), "pooled map (fvd_maxpool3d_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(fvd_maxpool3d_kernel, dim3((unsigned)blocks), dim3(FP_THREADS), 0, stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int fv_head(const char* who, const float* x, const float* w, const float* bias, float* out, long long N, const FvGeo& g, int F, hipStream_t stream) {
    if (N < 1 || g.C < 1 || F < 1) { set_error("%s: N, C and n_features must be >= 1 (got %lld, %d, %d)", who, N, g.C, F); return VPX_ERR_ARG; }
    if (g.T != FH_T || g.H != FH_S || g.W != FH_S) { set_error("%s: the final map must be %dx%dx%d (got %dx%dx%d): clips of 9 .. 16 frames give it", who, FH_T, FH_S, FH_S, g.T, g.H, g.W); return VPX_ERR_ARG; }
    if (g.C > FH_MAX_C) { set_error("%s: %d channels, the head holds at most %d", who, g.C, FH_MAX_C); return VPX_ERR_UNSUPPORTED; }
    if (N > FV_MAX_GRID || F > FV_MAX_C) { set_error("%s: %lld maps or %d features exceed one launch", who, N, F); return VPX_ERR_UNSUPPORTED; }
    VPX_LAUNCH(fvd_head_kernel, dim3((unsigned)N), dim3(FH_THREADS), 0, stream, x, w, bias, g.T * g.H * g.W, g.C, F, out);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

static int fv_stage(const char* who, const float* x0, const float* x1, long long n0, long long n1, int T, int C, int h, int w, float* y, hipStream_t stream) {
    FvStage a{};
    a.x0 = x0; a.x1 = x1; a.y = y; a.n0 = n0; a.T = T; a.C = C; a.h = h; a.w = w; a.S = FV_SIDE;
    a.resize = (h != FV_SIDE || w != FV_SIDE) ? 1 : 0;
    a.sy = (float)h / (float)FV_SIDE;
    a.sx = (float)w / (float)FV_SIDE;
    a.total = (n0 + n1) * T * FV_SIDE * FV_SIDE;
    const long long blocks = (a.total + FS_THREADS - 1) / FS_THREADS;
    if (blocks > FV_MAX_GRID) { set_error("%s: %lld clips of %d frames exceed one launch", who, n0 + n1, T); return VPX_ERR_UNSUPPORTED; }
    if (!ws_write_ok(y, (size_t)a.total * C * sizeof(float), "staged clips (fvd_stage_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
    VPX_LAUNCH(fvd_stage_kernel, dim3((unsigned)blocks), dim3(FS_THREADS), 0, stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

// ---- the trunk: a walk over the caller's layer table -----------------------------------------------------------------------------------
// A row: VPX_FVD_ROW ints (op, src, dst, Ci, Co, kt, kh, kw, st, sh, sw, relu, coff, ld, param, 0). op VPX_FVD_CONV / _POOL / _HEAD; src, dst: two
// different ones of the FV_BUFS buffers (buffer 0 holds the staged clips; the head's dst is unused); a convolution writes channels coff ..
// coff + Co - 1 of a map of channel stride ld and reads params[param] (packed weights) and params[param + 1] (bias); the head reads
// params[param] ([Co, Ci]) and params[param + 1]. The walk tracks every buffer's geometry; with `buf` == nullptr it only measures: floats[]
// receives what every buffer must hold — the size query and the call run the same walk, so neither can outgrow the other.
constexpr int FV_BUFS = 4, FV_MAX_ROWS = 256;
static int fv_walk(const char* who, long long N, int T, int C, const int* table, int n_rows, const float* const* params, int n_params, float* const* buf,
                   float* out, size_t floats[FV_BUFS], int* n_features, hipStream_t stream) {
    if (n_rows < 1 || n_rows > FV_MAX_ROWS) { set_error("%s: the layer table must have 1 .. %d rows (got %d)", who, FV_MAX_ROWS, n_rows); return VPX_ERR_ARG; }
    FvGeo geo[FV_BUFS] = {};
    geo[0] = FvGeo{T, FV_SIDE, FV_SIDE, C};
    for (int i = 0; i < FV_BUFS; ++i) floats[i] = 0;
    floats[0] = (size_t)N * T * FV_SIDE * FV_SIDE * C;
    bool headed = false;
    for (int r = 0; r < n_rows; ++r) {
        const int* row = table + (size_t)r * VPX_FVD_ROW;
        const int op = row[0], src = row[1], dst = row[2], Ci = row[3], Co = row[4], relu = row[11], coff = row[12], ld = row[13], param = row[14];
        const int k[3] = {row[5], row[6], row[7]}, s[3] = {row[8], row[9], row[10]};
        if (headed) { set_error("%s: row %d follows the head", who, r); return VPX_ERR_ARG; }
        if (src < 0 || src >= FV_BUFS || dst < 0 || dst >= FV_BUFS || (src == dst && op != VPX_FVD_HEAD)) { set_error("%s: row %d: buffers %d -> %d (two different ones of 0 .. %d)", who, r, src, dst, FV_BUFS - 1); return VPX_ERR_ARG; }
        if (geo[src].C < 1) { set_error("%s: row %d reads buffer %d before anything wrote it", who, r, src); return VPX_ERR_ARG; }
        if (Ci != geo[src].C) { set_error("%s: row %d expects %d input channels, buffer %d holds %d", who, r, Ci, src, geo[src].C); return VPX_ERR_ARG; }
        const bool reads = op != VPX_FVD_POOL && params && !g_dry_run;   // (the size query has no parameters, a dry run never reads them)
        if (op != VPX_FVD_POOL && params && (param < 0 || param + 2 > n_params)) { set_error("%s: row %d: params[%d], [%d] of %d", who, r, param, param + 1, n_params); return VPX_ERR_ARG; }
        if (reads && (!params[param] || !params[param + 1])) { set_error("%s: row %d: params[%d] or [%d] is NULL", who, r, param, param + 1); return VPX_ERR_ARG; }
        const float* p0 = reads ? params[param] : nullptr;
        const float* p1 = reads ? params[param + 1] : nullptr;
        FvGeo og{};
        if (op == VPX_FVD_CONV) {
            if (buf) { if (int rc = fv_conv(who, buf[src], p0, p1, buf[dst], N, geo[src], Co, k, s, relu, ld, coff, og, stream)) return rc; }
            else {
                if (int rc = fv_conv_check(who, N, geo[src], Co, k, s, ld, coff)) return rc;
                int f;
                fv_same(geo[src].T, k[0], s[0], f, og.T); fv_same(geo[src].H, k[1], s[1], f, og.H); fv_same(geo[src].W, k[2], s[2], f, og.W);
                og.C = ld;
            }
        } else if (op == VPX_FVD_POOL) {
            if (buf) { if (int rc = fv_pool(who, buf[src], buf[dst], N, geo[src], k, s, og, stream)) return rc; }
            else {
                if (int rc = fv_conv_check(who, N, geo[src], Ci, k, s, Ci, 0)) return rc;
                int f;
                fv_same(geo[src].T, k[0], s[0], f, og.T); fv_same(geo[src].H, k[1], s[1], f, og.H); fv_same(geo[src].W, k[2], s[2], f, og.W);
                og.C = Ci;
            }
        } else if (op == VPX_FVD_HEAD) {
            if (buf) { if (int rc = fv_head(who, buf[src], p0, p1, out, N, geo[src], Co, stream)) return rc; }
            else {
                if (geo[src].T != FH_T || geo[src].H != FH_S || geo[src].W != FH_S) { set_error("%s: the final map must be %dx%dx%d (got %dx%dx%d): clips of 9 .. 16 frames give it", who, FH_T, FH_S, FH_S, geo[src].T, geo[src].H, geo[src].W); return VPX_ERR_ARG; }
                if (Ci > FH_MAX_C || Co < 1 || Co > FV_MAX_C) { set_error("%s: a head of %d channels and %d features (at most %d, 1 .. %d)", who, Ci, Co, FH_MAX_C, FV_MAX_C); return VPX_ERR_UNSUPPORTED; }
            }
            *n_features = Co;
            headed = true;
            continue;
        } else { set_error("%s: row %d: unknown op %d", who, r, op); return VPX_ERR_ARG; }
        geo[dst] = og;
        const size_t need = (size_t)N * og.T * og.H * og.W * og.C;
        if (need > floats[dst]) floats[dst] = need;
    }
    if (!headed) { set_error("%s: the layer table has no head", who); return VPX_ERR_ARG; }
    return VPX_OK;
}

static int fv_features_check(const char* who, long long n0, long long n1, int T, int C, int h, int w, const int* table) {
    if (!table) { set_error("%s: NULL layer table", who); return VPX_ERR_ARG; }
    if (n0 < 1 || n1 < 0 || T < 1 || C < 1 || h < 1 || w < 1) { set_error("%s: clip counts must be >= 1 and >= 0, every size >= 1 (got %lld, %lld clips of %d frames %dx%dx%d)", who, n0, n1, T, C, h, w); return VPX_ERR_ARG; }
    if (h > FV_MAX_SIDE || w > FV_MAX_SIDE || T > FV_MAX_SIDE || C > 4 || n0 + n1 > FV_MAX_GRID) { set_error("%s: a side beyond %d, more than 4 frame channels or too many clips", who, FV_MAX_SIDE); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

// the trunk's buffers, each as large as the walk found its largest map
template <class WS>
static void carve_fvd(WS& ws, const size_t floats[FV_BUFS], float* buf[FV_BUFS]) {
    for (int i = 0; i < FV_BUFS; ++i) buf[i] = ws.take(floats[i]);
}

static int fd_check(const char* who, int b, int n) {
    if (b < 1 || n < 1) { set_error("%s: b and n must be >= 1 (got %d, %d)", who, b, n); return VPX_ERR_ARG; }
    if (b > FD_MAX_B) { set_error("%s: %d feature vectors per set, this build supports at most %d", who, b, FD_MAX_B); return VPX_ERR_UNSUPPORTED; }
    if (n > (1 << 20)) { set_error("%s: %d features exceed one launch", who, n); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

struct FdSlots { double *Ep, *Et, *G, *part; };
template <class WS>
static void carve_frechet(WS& ws, int b, int n, FdSlots& s) {   // (take() counts floats: a double is two)
    s.Ep = reinterpret_cast<double*>(ws.take((size_t)2 * b * n));
    s.Et = reinterpret_cast<double*>(ws.take((size_t)2 * b * n));
    s.G = reinterpret_cast<double*>(ws.take((size_t)2 * b * b));
    s.part = reinterpret_cast<double*>(ws.take((size_t)2 * 3 * n));
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_same_padding(int size, int k, int s, int* front, int* out) {
    if (size < 1 || k < 1 || s < 1 || !front || !out) { set_error("vpx_same_padding: sizes must be >= 1 and the outputs not NULL"); return VPX_ERR_ARG; }
    fv_same(size, k, s, *front, *out);
    return VPX_OK;
}

size_t vpx_conv3d_same_workspace_bytes(void) { return 0; }

int vpx_conv3d_same(const float* x, const float* wp, const float* bias, float* y, long long N, int T, int H, int W, int Ci, int Co, int kt, int kh, int kw,
                    int st, int sh, int sw, int relu, int ldy, int coff, void* stream_) {
    const char* who = "vpx_conv3d_same";
    if (!x || !wp || !bias || !y) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    const int k[3] = {kt, kh, kw}, s[3] = {st, sh, sw};
    FvGeo og;
    return fv_conv(who, x, wp, bias, y, N, FvGeo{T, H, W, Ci}, Co, k, s, relu, ldy, coff, og, (hipStream_t)stream_);
}

size_t vpx_maxpool3d_same_workspace_bytes(void) { return 0; }

int vpx_maxpool3d_same(const float* x, float* y, long long N, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw, void* stream_) {
    const char* who = "vpx_maxpool3d_same";
    if (!x || !y) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    const int k[3] = {kt, kh, kw}, s[3] = {st, sh, sw};
    FvGeo og;
    return fv_pool(who, x, y, N, FvGeo{T, H, W, C}, k, s, og, (hipStream_t)stream_);
}

size_t vpx_fvd_head_workspace_bytes(void) { return 0; }

int vpx_fvd_head(const float* x, const float* w, const float* bias, float* out, long long N, int T, int H, int W, int C, int n_features, void* stream_) {
    const char* who = "vpx_fvd_head";
    if (!x || !w || !bias || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    return fv_head(who, x, w, bias, out, N, FvGeo{T, H, W, C}, n_features, (hipStream_t)stream_);
}

size_t vpx_fvd_features_workspace_bytes(long long n_clips, int T, int C, int h, int w, const int* table, int n_rows) {
    const char* who = "vpx_fvd_features_workspace_bytes";
    if (fv_features_check(who, n_clips, 0, T, C, h, w, table) != VPX_OK) return 0;
    size_t floats[FV_BUFS];
    int F = 0;
    if (fv_walk(who, n_clips, T, C, table, n_rows, nullptr, 0, nullptr, nullptr, floats, &F, nullptr) != VPX_OK) return 0;
    CarveMeasure m; float* buf[FV_BUFS];
    carve_fvd(m, floats, buf);
    return m.off + 256;
}

int vpx_fvd_features(const float* x0, const float* x1, long long n0, long long n1, int T, int C, int h, int w, const int* table, int n_rows,
                     const float* const* params, int n_params, float* out, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_fvd_features";
    if (!x0 || (n1 > 0 && !x1) || !params || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (int rc = fv_features_check(who, n0, n1, T, C, h, w, table)) return rc;
    const long long N = n0 + n1;
    size_t floats[FV_BUFS];
    int F = 0;
    if (int rc = fv_walk(who, N, T, C, table, n_rows, params, n_params, nullptr, nullptr, floats, &F, nullptr)) return rc;
    const size_t need = vpx_fvd_features_workspace_bytes(N, T, C, h, w, table, n_rows);
    if (!workspace || !need || workspace_bytes < need) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    float* buf[FV_BUFS];
    carve_fvd(ws, floats, buf);
    VPX_CHECK_CARVE(ws, who);
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = fv_stage(who, x0, x1, n0, n1, T, C, h, w, buf[0], stream)) return rc;
    return fv_walk(who, N, T, C, table, n_rows, params, n_params, buf, out, floats, &F, stream);
}

size_t vpx_frechet_distance_workspace_bytes(int b, int n) {
    if (fd_check("vpx_frechet_distance_workspace_bytes", b, n) != VPX_OK) return 0;
    CarveMeasure m;
    FdSlots s{};
    carve_frechet(m, b, n, s);
    return m.off + 256;
}

int vpx_frechet_distance(const float* pred, const float* target, int b, int n, double* out, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_frechet_distance";
    if (!pred || !target || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (int rc = fd_check(who, b, n)) return rc;
    if (!workspace || workspace_bytes < vpx_frechet_distance_workspace_bytes(b, n)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    FdSlots s{};
    carve_frechet(ws, b, n, s);
    VPX_CHECK_CARVE(ws, who);
    hipStream_t stream = (hipStream_t)stream_;
    const double fact = b < 2 ? 1.0 : 1.0 / (double)(b - 1);
    VPX_LAUNCH(fvd_centre_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, pred, target, b, n, s.Ep, s.Et, s.part);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(fvd_gram_kernel, dim3((unsigned)((b * b + 255) / 256)), dim3(256), 0, stream, s.Ep, s.Et, b, n, fact, s.G);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(fvd_jacobi_kernel, dim3(1), dim3(FD_THREADS), 0, stream, s.G, b, n, fact, s.part, out);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
