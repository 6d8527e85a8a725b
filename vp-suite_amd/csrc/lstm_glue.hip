// lstm_glue.hip — the encoder / decoder pieces of the NonConvLSTM model (vp_suite/models/lstm.py) that the convolution layers lack:
//   * replicate padding with its adjoint on channels-last maps. enc2 / enc3 are Conv2d(3x3, stride 2, padding 1, padding_mode =
//     "replicate"): the padded map [N][H + 2p][W + 2p][C] goes to the library's strided convolution with padding 0. The adjoint is a
//     gather per source pixel (an edge pixel sums the border cells that copied it, row by row), so it is bit-reproducible.
//   * a differentiable bilinear resize (the decoder's final Resize((img_h, img_w)), which only ever enlarges; a side that shrinks is
//     sampled the same way, without antialiasing, as F.interpolate does): x channels-last
//     [N][H][W][C] -> y planar [N][C][oh][ow], align_corners = False, no antialiasing, on the source coordinate of frames_coord.h —
//     horizontally first, r = v0 * (1 - l) + v1 * l, then vertically, every operation rounded on its own (as vpx_frames_adapt does).
//     The backward is a gather too: a source pixel visits the output pixels whose taps can name it (a window from the inverse of the
//     coordinate map, widened by one, every candidate decided by fr_coord itself) in row-major order.
// Streaming kernels, no LDS, no atomics, 64-bit element offsets.
#include "vpx_host.h"

#pragma clang fp contract(off)

#include "frames_coord.h"

namespace vpx {

constexpr int LG_THREADS = 256;
constexpr int LG_MAX_SIDE = 32768;   // coordinates and their float32 images stay exact (as in adapt.hip)

__global__ __launch_bounds__(LG_THREADS) void replicate_pad_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H,
                                                                       int W, int C, int pad) {
    const long long e = (long long)blockIdx.x * LG_THREADS + threadIdx.x;
    if (e >= total) return;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int c = (int)(e % C);
    long long r = e / C;
    const int xx = (int)(r % Wp); r /= Wp;
    const int yy = (int)(r % Hp);
    const long long n = r / Hp;
    int sy = yy - pad, sx = xx - pad;
    sy = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);
    sx = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx);
    y[e] = x[((n * H + sy) * W + sx) * C + c];
}

__global__ __launch_bounds__(LG_THREADS) void replicate_pad_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long total, int H,
                                                                       int W, int C, int pad) {
    const long long e = (long long)blockIdx.x * LG_THREADS + threadIdx.x;
    if (e >= total) return;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int c = (int)(e % C);
    long long r = e / C;
    const int sx = (int)(r % W); r /= W;
    const int sy = (int)(r % H);
    const long long n = r / H;
    const int ylo = sy == 0 ? 0 : sy + pad, yhi = sy == H - 1 ? Hp - 1 : sy + pad;
    const int xlo = sx == 0 ? 0 : sx + pad, xhi = sx == W - 1 ? Wp - 1 : sx + pad;
    float s = 0.f;
    for (int yy = ylo; yy <= yhi; ++yy)
        for (int xx = xlo; xx <= xhi; ++xx) s += dy[((n * Hp + yy) * Wp + xx) * C + c];
    dx[e] = s;
}

struct ResizeArgs {
    long long total;
    int C, H, W, oh, ow;
    float sy, sx;   // float(H) / float(oh), float(W) / float(ow)
};

// thread = one output element of y [N][C][oh][ow]
__global__ __launch_bounds__(LG_THREADS) void resize_bilinear_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, ResizeArgs a) {
    const long long e = (long long)blockIdx.x * LG_THREADS + threadIdx.x;
    if (e >= a.total) return;
    const int ox = (int)(e % a.ow);
    long long r = e / a.ow;
    const int oy = (int)(r % a.oh); r /= a.oh;
    const int c = (int)(r % a.C);
    const long long n = r / a.C;
    int iy0, iy1, ix0, ix1;
    float ly, lx;
    fr_coord(a.sy, oy, a.H, iy0, iy1, ly);
    fr_coord(a.sx, ox, a.W, ix0, ix1, lx);
    const float wy = 1.0f - ly, wx = 1.0f - lx;
    const float* top = x + ((n * a.H + iy0) * a.W) * a.C + c;
    const float* bot = x + ((n * a.H + iy1) * a.W) * a.C + c;
    const float t = top[(long long)ix0 * a.C] * wx + top[(long long)ix1 * a.C] * lx;
    const float u = bot[(long long)ix0 * a.C] * wx + bot[(long long)ix1 * a.C] * lx;
    y[e] = t * wy + u * ly;
}

// output indices whose source coordinate can fall into (i - 1, i + 1): the inverse of src = s * (d + 0.5) - 0.5, one index wider each way
__device__ __forceinline__ void rs_window(float s, int i, int out, int& lo, int& hi) {
    const float a = ((float)i - 0.5f) / s - 0.5f, b = ((float)i + 1.5f) / s - 0.5f;
    lo = a < 0.0f ? 0 : (a > (float)out ? out : (int)a);
    lo = lo > 1 ? lo - 2 : 0;
    hi = b < 0.0f ? 0 : (b > (float)out ? out : (int)b);
    hi = hi + 2 > out - 1 ? out - 1 : hi + 2;
}

// thread = one source element of dx [N][H][W][C]
__global__ __launch_bounds__(LG_THREADS) void resize_bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, ResizeArgs a) {
    const long long e = (long long)blockIdx.x * LG_THREADS + threadIdx.x;
    if (e >= a.total) return;
    const int c = (int)(e % a.C);
    long long r = e / a.C;
    const int ix = (int)(r % a.W); r /= a.W;
    const int iy = (int)(r % a.H);
    const long long n = r / a.H;
    int ylo, yhi, xlo, xhi;
    rs_window(a.sy, iy, a.oh, ylo, yhi);
    rs_window(a.sx, ix, a.ow, xlo, xhi);
    const float* g = dy + (n * a.C + c) * (long long)a.oh * a.ow;
    float s = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        int i0, i1;
        float l;
        fr_coord(a.sy, oy, a.H, i0, i1, l);
        const float wyv = (i0 == iy ? 1.0f - l : 0.0f) + (i1 == iy ? l : 0.0f);
        if (i0 != iy && i1 != iy) continue;
        float row = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            int j0, j1;
            float m;
            fr_coord(a.sx, ox, a.W, j0, j1, m);
            if (j0 != ix && j1 != ix) continue;
            const float wxv = (j0 == ix ? 1.0f - m : 0.0f) + (j1 == ix ? m : 0.0f);
            row += g[(long long)oy * a.ow + ox] * wxv;
        }
        s += row * wyv;
    }
    dx[e] = s;
}

static int lg_pad_check(const char* who, const void* a, const void* b, long long N, int H, int W, int C, int pad) {
    if (!a || !b) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (N < 1 || H < 1 || W < 1 || C < 1 || pad < 0) { set_error("%s: bad argument (N=%lld H=%d W=%d C=%d pad=%d)", who, N, H, W, C, pad); return VPX_ERR_ARG; }
    if (H > LG_MAX_SIDE || W > LG_MAX_SIDE || pad > LG_MAX_SIDE || (double)N * (H + 2.0 * pad) * (W + 2.0 * pad) * C / LG_THREADS + 1.0 > 2147483647.0) {
        set_error("%s: %lld maps of %dx%dx%d with padding %d exceed one launch", who, N, H, W, C, pad);
        return VPX_ERR_UNSUPPORTED;
    }
    return VPX_OK;
}

static int lg_resize_check(const char* who, const void* a, const void* b, long long N, int C, int H, int W, int oh, int ow, ResizeArgs& ra) {
    if (!a || !b) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (N < 1 || C < 1 || H < 1 || W < 1 || oh < 1 || ow < 1) { set_error("%s: every size must be >= 1 (N=%lld C=%d H=%d W=%d, output %dx%d)", who, N, C, H, W, oh, ow); return VPX_ERR_ARG; }
    if (H > LG_MAX_SIDE || W > LG_MAX_SIDE || oh > LG_MAX_SIDE || ow > LG_MAX_SIDE || (double)N * C * H * W / LG_THREADS + 1.0 > 2147483647.0 || (double)N * C * oh * ow / LG_THREADS + 1.0 > 2147483647.0) {
        set_error("%s: not implemented: %lld frames of %dx%dx%d -> %dx%d exceed one launch", who, N, C, H, W, oh, ow);
        return VPX_ERR_UNSUPPORTED;
    }
    ra.C = C; ra.H = H; ra.W = W; ra.oh = oh; ra.ow = ow;
    ra.sy = (float)H / (float)oh;
    ra.sx = (float)W / (float)ow;
    return VPX_OK;
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_replicate_pad_fwd(const float* x, float* y, long long N, int H, int W, int C, int pad, void* stream) {
    if (int rc = lg_pad_check("vpx_replicate_pad_fwd", x, y, N, H, W, C, pad)) return rc;
    const long long total = N * (H + 2 * pad) * (long long)(W + 2 * pad) * C;
    VPX_LAUNCH(replicate_pad_fwd_kernel, dim3((unsigned)((total + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0, (hipStream_t)stream, x, y, total, H, W, C, pad);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_replicate_pad_bwd(const float* dy, float* dx, long long N, int H, int W, int C, int pad, void* stream) {
    if (int rc = lg_pad_check("vpx_replicate_pad_bwd", dy, dx, N, H, W, C, pad)) return rc;
    const long long total = N * H * (long long)W * C;
    VPX_LAUNCH(replicate_pad_bwd_kernel, dim3((unsigned)((total + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0, (hipStream_t)stream, dy, dx, total, H, W, C, pad);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_resize_bilinear_fwd(const float* x, float* y, long long N, int C, int H, int W, int oh, int ow, void* stream) {
    ResizeArgs a{};
    if (int rc = lg_resize_check("vpx_resize_bilinear_fwd", x, y, N, C, H, W, oh, ow, a)) return rc;
    a.total = N * C * (long long)oh * ow;
    VPX_LAUNCH(resize_bilinear_fwd_kernel, dim3((unsigned)((a.total + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0, (hipStream_t)stream, x, y, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_resize_bilinear_bwd(const float* dy, float* dx, long long N, int C, int H, int W, int oh, int ow, void* stream) {
    ResizeArgs a{};
    if (int rc = lg_resize_check("vpx_resize_bilinear_bwd", dy, dx, N, C, H, W, oh, ow, a)) return rc;
    a.total = N * C * (long long)H * W;
    VPX_LAUNCH(resize_bilinear_bwd_kernel, dim3((unsigned)((a.total + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0, (hipStream_t)stream, dy, dx, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
