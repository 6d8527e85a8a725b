// unet3d.hip — what UNet-3D (vp_suite/models/unet3d.py, blocks in model_blocks/conv.py DoubleConv2d / DoubleConv3d) needs and the
// library did not have: a convolution with REPLICATE borders, BatchNorm with batch statistics, and a 2x2 max-pool.
// Activations are channels-last per frame, [B][T][H][W][C]; a 2-D layer is T = 1 with one time tap. Weights stay in the reference's
// parameter layout ([Co][Ci][kt][ks][ks]; a Conv2d weight [Co][Ci][3][3] is the kt = 1 case of the same memory).
//   * rconv: kt x ks x ks taps (ks = 3 with kt in {1, 3}: frame and pixel index both CLAMPED = padding 1, padding_mode 'replicate';
//     or the time collapse Conv3d(C -> C, (T,1,1)): kt = T, ks = 1, one output frame, no border at all). The input may be two
//     channel-concatenated sources (the up path's cat(skip, x) is never materialised). fp32 FMA. Three epilogues: plain (+ bias), eval
//     (BatchNorm's running statistics and ReLU applied in place), and training (raw output + per-workgroup partial sums of y and of its squared deviations from the
//     workgroup's mean, per channel; a one-thread-per-channel finalise adds them in launch order in double: no atomics, no pass over the output).
//   * The data gradient of a clamped read is NOT a convolution with a border mode: taps that fell outside land on the edge pixel /
//     frame. rconv_dgrad gathers: per axis, input coordinate h receives exactly three (output, tap) pairs — (h - d, d) for d in
//     {-1, 0, 1}, where a pair whose output would lie outside [0, H) is the folded ring: (0, -1) at the low edge, (H-1, +1) at the
//     high edge. Fixed loop order, so bit-reproducible. The weight gradient runs over fixed pixel slices into slabs that a second
//     kernel adds in slice order (the bias gradient of the time collapse rides along as Co extra slab entries).
//   * bn_relu: y = relu(xhat * gamma + beta) from the raw convolution output and the finalised statistics, optionally also the 2x2
//     max-pooled activation in the same pass (the down path needs both). Backward: a reduction pass (sum dy relu', sum dy relu' xhat;
//     per-block partials, added in block order), and an apply pass. The pooled output's gradient is folded in: it goes to the FIRST
//     maximum of its window in row-major order (torch's max_pool backward); ReLU' is read off the saved activation (zero at 0).
#include "vpx_host.h"

namespace vpx {

constexpr int RC_VEC = 4;            // channels per thread of the convolution kernels
constexpr int RC_PIX = 256;          // pixels per workgroup
constexpr size_t RC_SLAB_FLOATS = (size_t)4 << 20;   // cap of the weight-gradient slabs (16 MB)
// Refused beyond these: every launch below covers its elements 256 to a workgroup on grid.x (< 2^31 workgroups) and its channels
// RC_VEC to a workgroup on grid.y (< 65536).
constexpr long long RC_MAX_ELEMS = 1LL << 38;
constexpr int RC_MAX_CH = 1 << 16;

struct RcArgs {
    const float *a, *b, *w;          // sources [B][T][H][W][Ca], [..][Cb] (Cb may be 0), weight [Co][Ca+Cb][kt][ks][ks]
    int B, T, To, H, W, Ca, Cb, Co, kt, ks, collapse;
    long long npix;                  // output pixels B*To*H*W
};

__device__ __forceinline__ int rc_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// sum over the 256 threads of a workgroup, in a fixed order; every thread must call it
__device__ __forceinline__ float rc_block_sum(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(RC_PIX) void rconv_fwd_kernel(RcArgs A, int epi, const float* __restrict__ p0, const float* __restrict__ p1,
                                                           const float* __restrict__ p2, const float* __restrict__ p3, float eps,
                                                           float* __restrict__ y, float* __restrict__ part) {
    __shared__ float sh[4];
    const long long p = blockIdx.x * (long long)RC_PIX + threadIdx.x;
    const int co0 = blockIdx.y * RC_VEC;
    const int nj = A.Co - co0 < RC_VEC ? A.Co - co0 : RC_VEC;
    const int Ci = A.Ca + A.Cb, taps = A.kt * A.ks * A.ks;
    const bool live = p < A.npix;
    float acc[RC_VEC];
#pragma unroll
    for (int j = 0; j < RC_VEC; ++j) acc[j] = 0.f;
    if (live) {
        const int x0 = (int)(p % A.W);
        const int y0 = (int)((p / A.W) % A.H);
        const int t0 = (int)((p / ((long long)A.W * A.H)) % A.To);
        const long long b = p / ((long long)A.W * A.H * A.To);
        for (int dt = 0; dt < A.kt; ++dt) {
            const int ts = A.collapse ? dt : rc_clamp(t0 + dt - A.kt / 2, A.T);
            for (int dy = 0; dy < A.ks; ++dy) {
                const int ys = rc_clamp(y0 + dy - A.ks / 2, A.H);
                for (int dx = 0; dx < A.ks; ++dx) {
                    const int xs = rc_clamp(x0 + dx - A.ks / 2, A.W);
                    const long long src = ((b * A.T + ts) * A.H + ys) * A.W + xs;
                    const float* wp = A.w + (size_t)co0 * Ci * taps + (dt * A.ks + dy) * A.ks + dx;
                    const float* ap = A.a + src * A.Ca;
                    for (int ci = 0; ci < A.Ca; ++ci) {
                        const float xv = ap[ci];
#pragma unroll
                        for (int j = 0; j < RC_VEC; ++j)
                            if (j < nj) acc[j] += xv * wp[(size_t)(j * Ci + ci) * taps];
                    }
                    if (A.Cb) {
                        const float* bp = A.b + src * A.Cb;
                        for (int ci = 0; ci < A.Cb; ++ci) {
                            const float xv = bp[ci];
#pragma unroll
                            for (int j = 0; j < RC_VEC; ++j)
                                if (j < nj) acc[j] += xv * wp[(size_t)(j * Ci + A.Ca + ci) * taps];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RC_VEC; ++j) {
            if (j >= nj) continue;
            const int co = co0 + j;
            float v = acc[j];
            if (epi == VPX_RCONV_EPI_PLAIN) {
                if (p0) v += p0[co];
            } else if (epi == VPX_RCONV_EPI_EVAL) {   // (x - running_mean) / sqrt(running_var + eps) * gamma + beta, then ReLU
                v = (v - p2[co]) * (1.0f / sqrtf(p3[co] + eps)) * p0[co] + p1[co];
                v = v < 0.f ? 0.f : v;          // (a NaN passes, as through torch's relu)
            }
            y[p * A.Co + co] = v;
        }
    }
    if (epi == VPX_RCONV_EPI_STATS) {   // (uniform branch: every thread of the workgroup takes it)
        const long long left = A.npix - blockIdx.x * (long long)RC_PIX;
        const int cnt = left < RC_PIX ? (int)left : RC_PIX;          // this workgroup's pixels (>= 1)
#pragma unroll
        for (int j = 0; j < RC_VEC; ++j) {
            const bool on = live && j < nj;
            const float s = rc_block_sum(on ? acc[j] : 0.f, sh);
            const float dv = on ? acc[j] - s / (float)cnt : 0.f;     // centred on the workgroup's own mean: no cancellation at |mean| >> std
            const float q = rc_block_sum(dv * dv, sh);
            if (threadIdx.x == 0 && j < nj) {
                part[((size_t)blockIdx.x * 2) * A.Co + co0 + j] = s;
                part[((size_t)blockIdx.x * 2 + 1) * A.Co + co0 + j] = q;
            }
        }
    }
}

// stats [2][C] = (mean, 1/sqrt(biased var + eps)); the running statistics (optional) take the batch mean and the UNBIASED variance
__global__ void bn_stats_finalize_kernel(const float* __restrict__ part, int nblk, int C, long long n, float eps, float momentum,
                                         float* __restrict__ stats, float* __restrict__ rmean, float* __restrict__ rvar) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int i = 0; i < nblk; ++i) s += (double)part[((size_t)i * 2) * C + c];
    const double mean = s / (double)n;
    for (int i = 0; i < nblk; ++i) {     // workgroup i: cnt values with sum part[2i] and squared deviations from their own mean part[2i+1]
        const double cnt = (double)(i + 1 < nblk ? RC_PIX : n - (long long)(nblk - 1) * RC_PIX);
        const double dm = (double)part[((size_t)i * 2) * C + c] / cnt - mean;
        q += (double)part[((size_t)i * 2 + 1) * C + c] + cnt * dm * dm;
    }
    const double var = q / (double)n;
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean) {
        rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mean);
        rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * var * ((double)n / (double)(n - 1)));
    }
}

// (output coordinate, tap index) pairs of one axis whose clamped read lands on input coordinate h: see the file comment
__device__ __forceinline__ int rc_pairs(int h, int H, int k, int* o, int* d) {
    if (k == 1) { o[0] = h; d[0] = 0; return 1; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int dd = i - 1, oo = h - dd;
        if (oo < 0) { oo = 0; dd = -1; }
        else if (oo >= H) { oo = H - 1; dd = 1; }
        o[i] = oo;
        d[i] = dd + 1;
    }
    return 3;
}

// dsrc [B][T][H][W][Cd] = the gradient of source channels [ci_off, ci_off + Cd) of the Ci = Ca + Cb the weight spans
__global__ __launch_bounds__(RC_PIX) void rconv_dgrad_kernel(RcArgs A, const float* __restrict__ dy, float* __restrict__ dsrc, int ci_off, int Cd) {
    const long long p = blockIdx.x * (long long)RC_PIX + threadIdx.x;   // input pixel (b, t, h, w)
    const long long npix_in = (long long)A.B * A.T * A.H * A.W;
    if (p >= npix_in) return;
    const int c0 = blockIdx.y * RC_VEC;
    const int nj = Cd - c0 < RC_VEC ? Cd - c0 : RC_VEC;
    const int Ci = A.Ca + A.Cb, taps = A.kt * A.ks * A.ks;
    const int x0 = (int)(p % A.W);
    const int y0 = (int)((p / A.W) % A.H);
    const int t0 = (int)((p / ((long long)A.W * A.H)) % A.T);
    const long long b = p / ((long long)A.W * A.H * A.T);
    int ot[3], dt[3], oy[3], dyi[3], ox[3], dxi[3];
    int nt;
    if (A.collapse) { ot[0] = 0; dt[0] = t0; nt = 1; }
    else nt = rc_pairs(t0, A.T, A.kt, ot, dt);
    const int ny = rc_pairs(y0, A.H, A.ks, oy, dyi), nx = rc_pairs(x0, A.W, A.ks, ox, dxi);
    float acc[RC_VEC];
#pragma unroll
    for (int j = 0; j < RC_VEC; ++j) acc[j] = 0.f;
    for (int it = 0; it < nt; ++it)
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) {
                const long long op = ((b * A.To + ot[it]) * A.H + oy[iy]) * A.W + ox[ix];
                const int tap = (dt[it] * A.ks + dyi[iy]) * A.ks + dxi[ix];
                const float* gp = dy + op * A.Co;
                const float* wp = A.w + (size_t)(ci_off + c0) * taps + tap;
                for (int co = 0; co < A.Co; ++co) {
                    const float g = gp[co];
#pragma unroll
                    for (int j = 0; j < RC_VEC; ++j)
                        if (j < nj) acc[j] += g * wp[((size_t)co * Ci + j) * taps];
                }
            }
#pragma unroll
    for (int j = 0; j < RC_VEC; ++j)
        if (j < nj) dsrc[p * Cd + c0 + j] = acc[j];
}

// slab [slice][Co*Ci*taps (+ Co)]: thread e owns one weight (ci fastest, so a wave reads a run of input channels) or, past the
// weights, one bias entry; it walks its slice's output pixels in order
__global__ __launch_bounds__(256) void rconv_wgrad_kernel(RcArgs A, const float* __restrict__ dy, float* __restrict__ slab, long long chunk, int with_bias) {
    const int Ci = A.Ca + A.Cb, taps = A.kt * A.ks * A.ks;
    const long long nw = (long long)taps * A.Co * Ci, nel = nw + (with_bias ? A.Co : 0);
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (e >= nel) return;
    const long long p_lo = blockIdx.y * chunk;
    long long p_hi = p_lo + chunk;
    if (p_hi > A.npix) p_hi = A.npix;
    float acc = 0.f;
    long long out;
    if (e >= nw) {
        const int co = (int)(e - nw);
        for (long long p = p_lo; p < p_hi; ++p) acc += dy[p * A.Co + co];
        out = nw + co;
    } else {
        const int ci = (int)(e % Ci), co = (int)((e / Ci) % A.Co), tap = (int)(e / ((long long)Ci * A.Co));
        const int dx = tap % A.ks, dyy = (tap / A.ks) % A.ks, dt = tap / (A.ks * A.ks);
        const bool from_a = ci < A.Ca;
        const float* src = from_a ? A.a : A.b;
        const int Cs = from_a ? A.Ca : A.Cb, cs = from_a ? ci : ci - A.Ca;
        for (long long p = p_lo; p < p_hi; ++p) {
            const int x0 = (int)(p % A.W);
            const int y0 = (int)((p / A.W) % A.H);
            const int t0 = (int)((p / ((long long)A.W * A.H)) % A.To);
            const long long b = p / ((long long)A.W * A.H * A.To);
            const int ts = A.collapse ? dt : rc_clamp(t0 + dt - A.kt / 2, A.T);
            const int ys = rc_clamp(y0 + dyy - A.ks / 2, A.H), xs = rc_clamp(x0 + dx - A.ks / 2, A.W);
            acc += dy[p * A.Co + co] * src[(((b * A.T + ts) * A.H + ys) * A.W + xs) * Cs + cs];
        }
        out = ((long long)co * Ci + ci) * taps + tap;
    }
    slab[(size_t)blockIdx.y * nel + out] = acc;
}

__global__ void rconv_wgrad_reduce_kernel(const float* __restrict__ slab, int nslice, long long nw, long long nel, float* __restrict__ dw, float* __restrict__ dbias) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= nel) return;
    double s = 0.0;
    for (int i = 0; i < nslice; ++i) s += (double)slab[(size_t)i * nel + e];
    if (e < nw) { if (dw) dw[e] = (float)s; }
    else if (dbias) dbias[e - nw] = (float)s;
}

// ---- BatchNorm + ReLU (+ 2x2 max-pool) -----------------------------------------------------------------------------------------------
// stats == NULL: x already is the activation (the eval path's pool); act == NULL: only the pooled output is written
__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ act, float* __restrict__ pooled,
                                                          long long N, int H, int W, int C) {
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (pooled) {
        const int Hq = H / 2, Wq = W / 2;
        if (e >= N * Hq * Wq * C) return;
        const int c = (int)(e % C);
        const long long q = e / C;
        const int wq = (int)(q % Wq), hq = (int)((q / Wq) % Hq);
        const long long n = q / ((long long)Wq * Hq);
        const long long base = (n * H + 2 * hq) * W + 2 * wq;
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = (base + (k >> 1) * W + (k & 1)) * C + c;
            float v = x[i];
            if (stats) {
                v = (v - stats[c]) * stats[C + c] * gamma[c] + beta[c];
                v = v < 0.f ? 0.f : v;
            }
            if (act) act[i] = v;
            if (k == 0 || v > m || v != v) m = v;   // (a NaN wins, as in torch's max_pool)
        }
        pooled[e] = m;
    } else {
        if (e >= N * H * W * C) return;
        const int c = (int)(e % C);
        float v = (x[e] - stats[c]) * stats[C + c] * gamma[c] + beta[c];
        act[e] = v < 0.f ? 0.f : v;
    }
}

// gradient reaching the pre-ReLU value of (pixel p, channel c): ReLU' * (dact + the pooled gradient if this element is the first
// maximum of its 2x2 window)
__device__ __forceinline__ float bn_g(const float* __restrict__ act, const float* __restrict__ dact, const float* __restrict__ dpool,
                                      long long p, int c, int H, int W, int C) {
    if (!(act[p * C + c] > 0.f)) return 0.f;
    float g = dact ? dact[p * C + c] : 0.f;
    if (dpool) {
        const int w = (int)(p % W), h = (int)((p / W) % H);
        const long long n = p / ((long long)W * H);
        const long long base = ((n * H + (h & ~1)) * W + (w & ~1));
        int idx = 0;
        float m = act[base * C + c];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float v = act[(base + (k >> 1) * W + (k & 1)) * C + c];
            if (v > m || v != v) { m = v; idx = k; }
        }
        if (idx == (h & 1) * 2 + (w & 1)) g += dpool[((n * (H / 2) + h / 2) * (W / 2) + w / 2) * C + c];
    }
    return g;
}

// part [block][2][C]: sums of g and g * xhat over the block's RC_PIX pixels. Threads are (pixel lane, channel) with the channel fastest
// (coalesced rows); the pixel lanes of a channel are added in lane order by lane 0.
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ act, const float* __restrict__ stats,
                                                            const float* __restrict__ dact, const float* __restrict__ dpool, float* __restrict__ part,
                                                            long long npix, int H, int W, int C) {
    __shared__ float s1[256], s2[256];
    const int Cb = C < 256 ? C : 256, npl = 256 / Cb;
    const int pl = threadIdx.x / Cb, cl = threadIdx.x % Cb;
    const long long p_lo = blockIdx.x * (long long)RC_PIX;
    long long p_hi = p_lo + RC_PIX;
    if (p_hi > npix) p_hi = npix;
    for (int cbase = 0; cbase < C; cbase += Cb) {   // (uniform trip count)
        const int c = cbase + cl;
        float a1 = 0.f, a2 = 0.f;
        if (pl < npl && c < C) {
            const float mean = stats[c], inv = stats[C + c];
            for (long long p = p_lo + pl; p < p_hi; p += npl) {
                const float g = bn_g(act, dact, dpool, p, c, H, W, C);
                a1 += g;
                a2 += g * ((x[p * C + c] - mean) * inv);
            }
        }
        __syncthreads();
        s1[threadIdx.x] = a1;
        s2[threadIdx.x] = a2;
        __syncthreads();
        if (pl == 0 && c < C) {
            float t1 = 0.f, t2 = 0.f;
            for (int k = 0; k < npl; ++k) { t1 += s1[k * Cb + cl]; t2 += s2[k * Cb + cl]; }
            part[((size_t)blockIdx.x * 2) * C + c] = t1;
            part[((size_t)blockIdx.x * 2 + 1) * C + c] = t2;
        }
    }
}

// sums [2][C] = (sum g, sum g xhat) = (dbeta, dgamma)
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int i = 0; i < nblk; ++i) {
        a += (double)part[((size_t)i * 2) * C + c];
        b += (double)part[((size_t)i * 2 + 1) * C + c];
    }
    sums[c] = (float)a;
    sums[C + c] = (float)b;
    if (dbeta) dbeta[c] = (float)a;
    if (dgamma) dgamma[c] = (float)b;
}

// dx = gamma / std * (g - mean(g) - xhat * mean(g xhat))
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ act, const float* __restrict__ stats,
                                                           const float* __restrict__ gamma, const float* __restrict__ dact, const float* __restrict__ dpool,
                                                           const float* __restrict__ sums, float* __restrict__ dx, long long npix, int H, int W, int C) {
    const long long e = blockIdx.x * 256LL + threadIdx.x;
    if (e >= npix * C) return;
    const int c = (int)(e % C);
    const long long p = e / C;
    const float inv = stats[C + c], rn = 1.0f / (float)npix;
    const float xh = (x[e] - stats[c]) * inv;
    const float g = bn_g(act, dact, dpool, p, c, H, W, C);
    dx[e] = gamma[c] * inv * (g - sums[c] * rn - xh * (sums[C + c] * rn));
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// prod(v[0..n)) * c < RC_MAX_ELEMS, without overflowing on the way (all factors >= 1, c <= 3 * RC_MAX_CH)
static bool rc_fits(const long long* v, int n, long long c) {
    long long room = (RC_MAX_ELEMS - 1) / c;
    for (int i = 0; i < n; ++i) room /= v[i];
    return room >= 1;
}

static int rc_check(const char* who, const vpx_rconv_desc* d, RcArgs& A) {
    if (!d) { set_error("%s: desc is NULL", who); return VPX_ERR_ARG; }
    if (d->B < 1 || d->T < 1 || d->H < 1 || d->W < 1 || d->Ca < 1 || d->Cb < 0 || d->Co < 1) {
        set_error("%s: bad shape (B=%d T=%d H=%d W=%d Ca=%d Cb=%d Co=%d)", who, d->B, d->T, d->H, d->W, d->Ca, d->Cb, d->Co);
        return VPX_ERR_ARG;
    }
    if (d->mode == VPX_RCONV_REPLICATE) {
        if (d->kt != 1 && d->kt != 3) { set_error("%s: a replicate-border layer has 1 or 3 taps in time, got %d", who, d->kt); return VPX_ERR_ARG; }
    } else if (d->mode == VPX_RCONV_COLLAPSE) {
        if (d->kt != d->T) { set_error("%s: the time collapse spans all %d frames, got kt=%d", who, d->T, d->kt); return VPX_ERR_ARG; }
    } else { set_error("%s: unknown mode %d", who, d->mode); return VPX_ERR_ARG; }
    const long long dims[4] = {d->B, d->T, d->H, d->W};
    if (d->Ca > RC_MAX_CH || d->Cb > RC_MAX_CH || d->Co > RC_MAX_CH || !rc_fits(dims, 4, (long long)d->Ca + d->Cb + d->Co) ||
        (long long)d->kt * d->Co * ((long long)d->Ca + d->Cb) >= RC_MAX_ELEMS) {     // (the weight gradient's grid; only a collapse of very many frames gets here)
        set_error("%s: tensor too large", who);
        return VPX_ERR_UNSUPPORTED;
    }
    const bool col = d->mode == VPX_RCONV_COLLAPSE;
    A = RcArgs{nullptr, nullptr, nullptr, d->B, d->T, col ? 1 : d->T, d->H, d->W, d->Ca, d->Cb, d->Co, d->kt, col ? 1 : 3, col ? 1 : 0, 0};
    A.npix = (long long)d->B * A.To * d->H * d->W;
    return VPX_OK;
}
static inline long long rc_blocks(long long n) { return (n + RC_PIX - 1) / RC_PIX; }
static inline int rc_slices(const RcArgs& A, long long nel) {
    long long s = (A.npix + 127) / 128;
    if (s > 256) s = 256;
    const long long cap = (long long)(RC_SLAB_FLOATS / (size_t)nel);
    if (s > cap) s = cap;
    return (int)(s < 1 ? 1 : s);
}
static inline long long rc_nel(const RcArgs& A, bool bias) { return (long long)A.kt * A.ks * A.ks * A.Co * (A.Ca + A.Cb) + (bias ? A.Co : 0); }

// The workspaces: every slot in the order the call takes it, and the counts the launches are sized by.
struct RcFwdSlots { float* part; long long nblk; };   // per-workgroup statistics of the training epilogue (else one unused float)
template <class WS>
static void carve_rconv_fwd(WS& ws, const RcArgs& A, int epilogue, RcFwdSlots& s) {
    s.nblk = rc_blocks(A.npix);
    s.part = ws.take(epilogue == VPX_RCONV_EPI_STATS ? (size_t)s.nblk * 2 * A.Co : 1);
}
struct RcBwdSlots { float* slab; int ns; };   // ns K slices of [dw | dbias], sized with the bias whether or not the call wants it
template <class WS>
static void carve_rconv_bwd(WS& ws, const RcArgs& A, RcBwdSlots& s) {
    const long long nel = rc_nel(A, true);
    s.ns = rc_slices(A, nel);
    s.slab = ws.take((size_t)s.ns * nel);
}
struct BnBwdSlots { float *part, *sums; long long nblk; };
template <class WS>
static void carve_bn_relu_bwd(WS& ws, long long npix, int C, BnBwdSlots& s) {
    s.nblk = rc_blocks(npix);
    s.part = ws.take((size_t)s.nblk * 2 * C);
    s.sums = ws.take((size_t)2 * C);
}

static int bn_check(const char* who, long long N, int H, int W, int C, bool pool) {
    const long long dims[3] = {N, H, W};
    if (N < 1 || H < 1 || W < 1 || C < 1 || C > RC_MAX_CH || !rc_fits(dims, 3, C)) { set_error("%s: bad shape (N=%lld H=%d W=%d C=%d)", who, N, H, W, C); return VPX_ERR_ARG; }
    if (pool && ((H & 1) || (W & 1))) { set_error("%s: the 2x2 pool needs an even map, got %dx%d", who, H, W); return VPX_ERR_ARG; }
    return VPX_OK;
}

}  // namespace vpx

using namespace vpx;

extern "C" {

size_t vpx_rconv_workspace_bytes(const vpx_rconv_desc* d, int epilogue) {
    RcArgs A;
    if (rc_check("vpx_rconv_workspace_bytes", d, A)) return 0;
    if (epilogue < VPX_RCONV_EPI_PLAIN || epilogue > VPX_RCONV_EPI_STATS) { set_error("vpx_rconv_workspace_bytes: unknown epilogue %d", epilogue); return 0; }
    CarveMeasure m; RcFwdSlots s{};
    carve_rconv_fwd(m, A, epilogue, s);
    return m.off + 512;
}

int vpx_rconv_fwd(const vpx_rconv_desc* d, int epilogue, const float* a, const float* b, const float* w, const float* gamma_or_bias,
                  const float* beta, float* running_mean, float* running_var, float eps, float momentum, float* y, float* stats,
                  void* workspace, size_t workspace_bytes, void* stream_) {
    RcArgs A;
    if (int rc = rc_check("vpx_rconv_fwd", d, A)) return rc;
    if (epilogue < VPX_RCONV_EPI_PLAIN || epilogue > VPX_RCONV_EPI_STATS) { set_error("vpx_rconv_fwd: unknown epilogue %d", epilogue); return VPX_ERR_ARG; }
    if (!a || !w || !y || (d->Cb > 0 && !b)) { set_error("vpx_rconv_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (epilogue == VPX_RCONV_EPI_EVAL && (!gamma_or_bias || !beta || !running_mean || !running_var)) { set_error("vpx_rconv_fwd: the eval epilogue needs gamma, beta and both running statistics"); return VPX_ERR_ARG; }
    if (epilogue != VPX_RCONV_EPI_PLAIN && !(eps > 0.f)) { set_error("vpx_rconv_fwd: eps must be positive"); return VPX_ERR_ARG; }
    if (epilogue == VPX_RCONV_EPI_STATS) {
        if (!stats || (!running_mean) != (!running_var)) { set_error("vpx_rconv_fwd: the training epilogue needs stats, and both running statistics or neither"); return VPX_ERR_ARG; }
        if (A.npix < 2) { set_error("vpx_rconv_fwd: batch statistics need more than one value per channel"); return VPX_ERR_ARG; }
    }
    if (!workspace || workspace_bytes < vpx_rconv_workspace_bytes(d, epilogue)) { set_error("vpx_rconv_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    RcFwdSlots s{};
    carve_rconv_fwd(ws, A, epilogue, s);
    VPX_CHECK_CARVE(ws, "vpx_rconv_fwd");
    A.a = a; A.b = b; A.w = w;
    VPX_LAUNCH(rconv_fwd_kernel, dim3((unsigned)s.nblk, (unsigned)((A.Co + RC_VEC - 1) / RC_VEC)), dim3(RC_PIX), 0, stream, A, epilogue, gamma_or_bias, beta,
               (const float*)running_mean, (const float*)running_var, eps, y, s.part);
    VPX_CHECK_HIP(vpx_hip_last_error());
    if (epilogue == VPX_RCONV_EPI_STATS) {
        VPX_LAUNCH(bn_stats_finalize_kernel, dim3((unsigned)((A.Co + 63) / 64)), dim3(64), 0, stream, (const float*)s.part, (int)s.nblk, A.Co, A.npix, eps, momentum,
                   stats, running_mean, running_var);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

size_t vpx_rconv_bwd_workspace_bytes(const vpx_rconv_desc* d) {
    RcArgs A;
    if (rc_check("vpx_rconv_bwd_workspace_bytes", d, A)) return 0;
    CarveMeasure m; RcBwdSlots s{};
    carve_rconv_bwd(m, A, s);
    return m.off + 512;
}

int vpx_rconv_bwd(const vpx_rconv_desc* d, const float* a, const float* b, const float* w, const float* dy, float* da, float* db, float* dw,
                  float* dbias, void* workspace, size_t workspace_bytes, void* stream_) {
    RcArgs A;
    if (int rc = rc_check("vpx_rconv_bwd", d, A)) return rc;
    if (!a || !w || !dy || (d->Cb > 0 && !b)) { set_error("vpx_rconv_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (db && d->Cb == 0) { set_error("vpx_rconv_bwd: db without a second source"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_rconv_bwd_workspace_bytes(d)) { set_error("vpx_rconv_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    RcBwdSlots s{};
    carve_rconv_bwd(ws, A, s);
    VPX_CHECK_CARVE(ws, "vpx_rconv_bwd");
    A.a = a; A.b = b; A.w = w;
    const long long nblk_in = rc_blocks((long long)A.B * A.T * A.H * A.W);
    if (da) {
        VPX_LAUNCH(rconv_dgrad_kernel, dim3((unsigned)nblk_in, (unsigned)((A.Ca + RC_VEC - 1) / RC_VEC)), dim3(RC_PIX), 0, stream, A, dy, da, 0, A.Ca);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    if (db) {
        VPX_LAUNCH(rconv_dgrad_kernel, dim3((unsigned)nblk_in, (unsigned)((A.Cb + RC_VEC - 1) / RC_VEC)), dim3(RC_PIX), 0, stream, A, dy, db, A.Ca, A.Cb);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    if (dw || dbias) {
        const bool with_bias = dbias != nullptr;
        const long long nel = rc_nel(A, with_bias), nw = rc_nel(A, false);
        const int ns = s.ns;
        const long long chunk = (A.npix + ns - 1) / ns;
        VPX_LAUNCH(rconv_wgrad_kernel, dim3((unsigned)((nel + 255) / 256), (unsigned)ns), dim3(256), 0, stream, A, dy, s.slab, chunk, with_bias ? 1 : 0);
        VPX_CHECK_HIP(vpx_hip_last_error());
        VPX_LAUNCH(rconv_wgrad_reduce_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, stream, (const float*)s.slab, ns, nw, nel, dw, dbias);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

int vpx_bn_relu_fwd(const float* x, const float* stats, const float* gamma, const float* beta, float* act, float* pooled, long long N, int H,
                    int W, int C, void* stream) {
    if (int rc = bn_check("vpx_bn_relu_fwd", N, H, W, C, pooled != nullptr)) return rc;
    if (!x || (!act && !pooled) || (stats && (!gamma || !beta || !act))) { set_error("vpx_bn_relu_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (!stats && (act || !pooled)) { set_error("vpx_bn_relu_fwd: without statistics only the pooled output is written"); return VPX_ERR_ARG; }
    const long long n = pooled ? N * (H / 2) * (W / 2) * C : N * H * W * C;
    VPX_LAUNCH(bn_relu_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, stats, gamma, beta, act, pooled, N, H, W, C);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

size_t vpx_bn_relu_bwd_workspace_bytes(long long N, int H, int W, int C) {
    if (bn_check("vpx_bn_relu_bwd_workspace_bytes", N, H, W, C, false)) return 0;
    CarveMeasure m; BnBwdSlots s{};
    carve_bn_relu_bwd(m, N * H * W, C, s);
    return m.off + 512;
}

int vpx_bn_relu_bwd(const float* x, const float* act, const float* stats, const float* gamma, const float* dact, const float* dpool, float* dx,
                    float* dgamma, float* dbeta, long long N, int H, int W, int C, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = bn_check("vpx_bn_relu_bwd", N, H, W, C, dpool != nullptr)) return rc;
    if (!x || !act || !stats || !gamma || !dx || (!dact && !dpool)) { set_error("vpx_bn_relu_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_bn_relu_bwd_workspace_bytes(N, H, W, C)) { set_error("vpx_bn_relu_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    const long long npix = N * H * W;
    Carver ws(workspace, workspace_bytes);
    BnBwdSlots s{};
    carve_bn_relu_bwd(ws, npix, C, s);
    VPX_CHECK_CARVE(ws, "vpx_bn_relu_bwd");
    VPX_LAUNCH(bn_bwd_reduce_kernel, dim3((unsigned)s.nblk), dim3(256), 0, stream, x, act, stats, dact, dpool, s.part, npix, H, W, C);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(bn_bwd_finalize_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, stream, (const float*)s.part, (int)s.nblk, C, s.sums, dgamma, dbeta);
    VPX_CHECK_HIP(vpx_hip_last_error());
    VPX_LAUNCH(bn_bwd_apply_kernel, dim3((unsigned)((npix * C + 255) / 256)), dim3(256), 0, stream, x, act, stats, gamma, dact, dpool, (const float*)s.sums, dx,
               npix, H, W, C);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
