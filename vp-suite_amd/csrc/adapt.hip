// Frame adapter between a model and a test set that differ in value range or frame size (vp_suite/utils/compatibility.py:31-50: ScaleToModel /
// ScaleToTest of utils/models.py:7-64, then TF.Resize), one launch:
//   vpx_frames_adapt    x float32 [N][C][H][W] (planar, only read) -> out float32 [N][C][oh][ow]
// Pixel contract (tests/adapt_ref.py restates it), every step ONE correctly rounded float32 operation, in the reference's order — scale
// first, then resize:
//   only if (src_lo, src_hi) != (dst_lo, dst_hi):  v = v - float(src_lo);  v = v / float(src_hi - src_lo);  v = v * float(dst_hi - dst_lo);
//   v = v + float(dst_lo)   (the differences formed in double by the caller's language);
//   only if (oh, ow) != (H, W): bilinear, align_corners = False, no antialiasing, with the source coordinates of frames_coord.h (the ones the
//   dataset resize of frames.hip uses); the taps are the scaled values v; horizontally first, r = v0 * (1 - l) + v1 * l, then the same
//   vertically. Held to a bound, not to bits.
// Equal sizes: the pure affine map over the flat tensor. Equal ranges: no arithmetic on the taps; with equal sizes too, a copy.
// Streaming kernels, no LDS, no atomics. Resize: a thread owns four neighbouring output pixels of one row in EVERY channel of one frame, so
// the row's and the four columns' taps and weights are computed once per thread and serve all 16 * C taps, and a channel plane receives one
// 16-byte store per thread where the rows allow it (ow % 4 == 0, `out` 16-byte aligned), single stores otherwise. Affine: a thread owns four
// consecutive elements, one 16-byte load and store where both pointers are 16-byte aligned, and the last 1-3 elements leave singly.
#include <hip/hip_runtime.h>
#include "vpx_internal.h"
#include "vpx_host.h"

// Every operation of this file is rounded on its own (see frames.hip): no a * b + c becomes a fused multiply-add.
#pragma clang fp contract(off)

#include "frames_coord.h"

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AD_THREADS = 256;
constexpr int AD_MAX_SIDE = 32768;    // frame and output sides: coordinates and their float32 images stay exact (as in frames.hip)

struct AdaptArgs {
    const float* x;                    // [N][C][H][W]
    float* out;                        // [N][C][oh][ow]
    long long items;                   // resize: N * oh * Q threads; affine: groups of four elements
    long long total;                   // affine: N * C * H * W elements
    int C, H, W, oh, ow;
    int Q;                             // groups of four pixels per output row (the last one partial if ow % 4)
    int vec;                           // 1: every full group is one 16-byte store (resize) / load and store (affine)
    int scaled;                        // 1: (src_lo, src_hi) != (dst_lo, dst_hi)
    float slo, sden, dscale, dlo;      // float(src_lo), float(src_hi - src_lo), float(dst_hi - dst_lo), float(dst_lo)
    float sy, sx;                      // float(H) / float(oh), float(W) / float(ow)
};

__device__ __forceinline__ float ad_value(const AdaptArgs& a, float v) {
    if (a.scaled) {
        v = v - a.slo;
        v = v / a.sden;
        v = v * a.dscale;
        v = v + a.dlo;
    }
    return v;
}

// thread = (frame n, output row y, group of four output pixels); loops over the frame's channels
__global__ __launch_bounds__(AD_THREADS) void adapt_resize_kernel(AdaptArgs a) {
    const long long item = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int q = (int)(item % a.Q);
    const long long r = item / a.Q;
    const int y = (int)(r % a.oh);
    const long long n = r / a.oh;
    const int x0 = q << 2;
    int iy0, iy1;
    float ly;
    fr_coord(a.sy, y, a.H, iy0, iy1, ly);
    const float wy = 1.0f - ly;
    int ix0[4], ix1[4];
    float lx[4], wx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k < a.ow ? x0 + k : a.ow - 1;               // (a partial group repeats the row's last pixel; it is not stored)
        fr_coord(a.sx, x, a.W, ix0[k], ix1[k], lx[k]);
        wx[k] = 1.0f - lx[k];
    }
    const size_t in_plane = (size_t)a.H * a.W, out_plane = (size_t)a.oh * a.ow;   // 64-bit offsets throughout
    const float* src = a.x + (size_t)n * a.C * in_plane;
    float* dst = a.out + (size_t)n * a.C * out_plane + (size_t)y * a.ow + x0;
    for (int c = 0; c < a.C; ++c) {
        const float* top = src + (size_t)iy0 * a.W;
        const float* bot = src + (size_t)iy1 * a.W;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = ad_value(a, top[ix0[k]]) * wx[k] + ad_value(a, top[ix1[k]]) * lx[k];
            const float u = ad_value(a, bot[ix0[k]]) * wx[k] + ad_value(a, bot[ix1[k]]) * lx[k];
            o[k] = t * wy + u * ly;
        }
        if (a.vec) *reinterpret_cast<f32x4*>(dst) = o;
        else
            for (int k = 0; k < 4 && x0 + k < a.ow; ++k) dst[k] = o[k];
        src += in_plane;
        dst += out_plane;
    }
}

// thread = four consecutive elements of the flat tensor (equal sizes: no taps, the affine map alone)
__global__ __launch_bounds__(AD_THREADS) void adapt_affine_kernel(AdaptArgs a) {
    const long long item = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const long long e0 = item << 2;
    if (a.vec && e0 + 4 <= a.total) {
        f32x4 v = *reinterpret_cast<const f32x4*>(a.x + e0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ad_value(a, v[k]);
        *reinterpret_cast<f32x4*>(a.out + e0) = v;
    } else {
        for (int k = 0; k < 4 && e0 + k < a.total; ++k) a.out[e0 + k] = ad_value(a, a.x[e0 + k]);
    }
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_frames_adapt(const float* x, long long N, int C, int H, int W, int oh, int ow, double src_lo, double src_hi, double dst_lo,
                     double dst_hi, float* out, void* stream) {
    const char* who = "vpx_frames_adapt";
    if (!x || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (N < 1 || C < 1 || H < 1 || W < 1 || oh < 1 || ow < 1) { set_error("%s: every size must be >= 1 (got N=%lld C=%d H=%d W=%d, output %dx%d)", who, N, C, H, W, oh, ow); return VPX_ERR_ARG; }
    if (src_hi == src_lo || (float)(src_hi - src_lo) == 0.0f) { set_error("%s: empty source value range [%g, %g]", who, src_lo, src_hi); return VPX_ERR_ARG; }
    if (H > AD_MAX_SIDE || W > AD_MAX_SIDE || oh > AD_MAX_SIDE || ow > AD_MAX_SIDE) { set_error("%s: a side beyond %d (frame %dx%d, output %dx%d)", who, AD_MAX_SIDE, H, W, oh, ow); return VPX_ERR_UNSUPPORTED; }
    const int resize = (oh != H || ow != W) ? 1 : 0;
    const int Q = (ow + 3) / 4;
    const double in_elems = (double)N * C * H * W, out_elems = (double)N * C * oh * ow;
    const double items_d = resize ? (double)N * oh * Q : (in_elems + 3.0) / 4.0;
    if (in_elems > 4.0e18 || out_elems > 4.0e18 || items_d / AD_THREADS + 1.0 > 2147483647.0) { set_error("%s: %lld frames of %dx%dx%d -> %dx%d exceed one launch", who, N, C, H, W, oh, ow); return VPX_ERR_UNSUPPORTED; }
    AdaptArgs a;
    a.x = x; a.out = out; a.C = C; a.H = H; a.W = W; a.oh = oh; a.ow = ow; a.Q = Q;
    a.total = N * C * H * W;
    a.items = resize ? N * oh * Q : (a.total + 3) / 4;
    a.vec = resize ? ((ow % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0) : ((((uintptr_t)out | (uintptr_t)x) & 15) == 0 ? 1 : 0);
    a.scaled = (src_lo != dst_lo || src_hi != dst_hi) ? 1 : 0;
    a.slo = (float)src_lo;
    a.sden = (float)(src_hi - src_lo);
    a.dscale = (float)(dst_hi - dst_lo);
    a.dlo = (float)dst_lo;
    a.sy = (float)H / (float)oh;
    a.sx = (float)W / (float)ow;
    const unsigned blocks = (unsigned)((a.items + AD_THREADS - 1) / AD_THREADS);
    if (resize) VPX_LAUNCH(adapt_resize_kernel, dim3(blocks), dim3(AD_THREADS), 0, (hipStream_t)stream, a);
    else VPX_LAUNCH(adapt_affine_kernel, dim3(blocks), dim3(AD_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
