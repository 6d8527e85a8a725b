// Photometric augmentations and erasing of a preprocessed batch (the colour and erasing entries of vp_suite/base/base_dataset.py:19-23),
// in place, one launch.
//   vpx_frames_augment   x float32 [B][F][C][h][w] and a device table of programs float32 [B][max_ops][VPX_FRAMES_AUG_ROW]
// A program is a list of rows (opcode, 8 parameters), ended by opcode 0 (or by max_ops); every frame of sample b runs program b. The
// parameters were drawn on the host, once per sequence. Pixel contract (tests/frames_aug_ref.py restates it), every step ONE correctly
// rounded float32 operation; clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v), literal whatever the value range; gray(r, g, b) =
// (0.2989f * r + 0.587f * g) + 0.114f * b (torchvision's rgb_to_grayscale); blend(a, b) = clamp(f * a + g * b) with f and g = 1 - f both
// given by the row (torchvision's _blend):
//   1 invert          v = 1 - v
//   2 solarize        p0 = threshold:  v >= p0 ? 1 - v : v
//   3 autocontrast    per channel lo / hi = min / max over the frame; hi == lo: unchanged; else s = 1 / (hi - lo), v = clamp((v - lo) * s)
//   4 grayscale       C = 3: every plane = gray(r, g, b)
//   5 normalize       p0..3 = mean, p4..7 = std:  v = (v - mean[c]) / std[c]
//   6 brightness      p0 = f, p1 = g:  v = blend(v, 0)
//   7 contrast        v = blend(v, m), m = float(sum / n) of gray (C = 3) or of v (C = 1) over the frame, the sum formed in float64
//   8 saturation      C = 3: v = blend(v, gray); C = 1: identity
//   9 hue             p0 = d; C = 3: torchvision's _rgb2hsv, h = (h + d) mod 1, _hsv2rgb; C = 1: identity
//  10 erase           p0..3 = y0, x0, rows, columns (whole numbers), p4..7 = value per channel: the rectangle, clipped to the frame, = value
// One workgroup per (sample, frame); a thread owns the pixel groups g, g + 256, ... in every channel (the planes are separate, so a
// wave's loads of one plane are contiguous). The workgroup sweeps the frame: in one sweep it applies consecutive operations until it
// meets one that needs a statistic of the whole frame (3, 7), gathers that statistic from the values it has just computed, writes them
// back, reduces across the workgroup (lanes by shuffles, waves through LDS, a fixed tree), and carries on from that operation. Sweeps =
// 1 + number of statistic operations (a program that BEGINS with one reads the frame once more without writing it). A thread only ever
// reads back what it wrote itself. No atomics, nothing depends on the launch order: two runs give equal bits.
// The table lives on the device, so the caller checks it; a row the kernel cannot run (an unknown opcode, an operation the channel
// count does not allow) ends the program there, and a rectangle is clipped: nothing is read or written outside the frame.
#include <hip/hip_runtime.h>
#include "vpx_internal.h"
#include "vpx_host.h"

// Every operation of this file is rounded on its own (see frames.hip): no a * b + c becomes a fused multiply-add.
#pragma clang fp contract(off)

namespace vpx {

typedef float fa_f32x4 __attribute__((ext_vector_type(4)));

constexpr int FA_THREADS = 256;
constexpr int FA_WAVES = FA_THREADS / 64;
constexpr int FA_ROW = VPX_FRAMES_AUG_ROW;
constexpr int FA_MIN_OPS = 16;
constexpr int FA_MAX_OPS = 64;
constexpr int FA_MAX_C = 4;
constexpr int FA_MAX_SIDE = 32768;    // FR_MAX_SIDE of frames.hip: pixel coordinates and their float32 images stay exact

enum { FA_END = 0, FA_INVERT, FA_SOLARIZE, FA_AUTOCONTRAST, FA_GRAY, FA_NORMALIZE, FA_BRIGHTNESS, FA_CONTRAST, FA_SATURATION, FA_HUE, FA_ERASE, FA_NOPS };

struct AugArgs {
    float* x;                          // [B][F][C][h][w]
    const float* programs;             // [B][max_ops][FA_ROW]
    int F, C, h, w, max_ops;
    int npix;                          // h * w (<= 2^30)
};

struct FaStat {                        // the statistic of the running statistic operation, valid for every thread after fa_reduce()
    float mean;                        // contrast
    float lo[FA_MAX_C], scale[FA_MAX_C];   // autocontrast: scale 0 marks a constant channel (1 / (hi - lo) is never 0)
};

__device__ __forceinline__ float fa_clamp(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
__device__ __forceinline__ float fa_gray(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }
__device__ __forceinline__ float fa_blend(float f, float g, float a, float b) { return fa_clamp(f * a + g * b); }
__device__ __forceinline__ float fa_frac(float v) { return v - truncf(v); }          // fmod(v, 1): exact
__device__ __forceinline__ int fa_whole(float v) { return !(v >= 0.0f) ? 0 : (v > (float)FA_MAX_SIDE ? FA_MAX_SIDE : (int)v); }

// torchvision's adjust_hue on one pixel (functional_tensor.py: _rgb2hsv, (h + d) % 1.0, _hsv2rgb)
__device__ __forceinline__ void fa_hue(float* v, float d) {
    const float r = v[0], g = v[1], b = v[2];
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float div = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float hh;
    if (maxc == r) hh = bc - gc;
    else if (maxc == g) hh = (2.0f + rc) - bc;
    else hh = (4.0f + gc) - rc;
    hh = fa_frac(hh / 6.0f + 1.0f);
    hh = hh + d;
    hh = fa_frac(hh);                                                  // Python's %: the remainder takes the divisor's sign
    if (hh < 0.0f) hh = hh + 1.0f;
    const float h6 = hh * 6.0f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    int i = (int)fl % 6;
    if (i < 0) i += 6;
    const float p = fa_clamp(maxc * (1.0f - s));
    const float q = fa_clamp(maxc * (1.0f - f * s));
    const float t = fa_clamp(maxc * (1.0f - (1.0f - f) * s));
    v[0] = i == 0 ? maxc : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : maxc))));
    v[1] = i == 0 ? t : (i == 1 ? maxc : (i == 2 ? maxc : (i == 3 ? q : (i == 4 ? p : p))));
    v[2] = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? maxc : (i == 4 ? maxc : q))));
}

// operation `op` with parameter row `r` on the C channels of pixel `pix`; the statistic operations read `st`
__device__ __forceinline__ void fa_apply(int op, const float* r, const FaStat& st, float* v, int C, int pix, int h, int w) {
    switch (op) {
    case FA_INVERT:
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c) v[c] = 1.0f - v[c];
        break;
    case FA_SOLARIZE: {
        const float thr = r[1];
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c) v[c] = v[c] >= thr ? 1.0f - v[c] : v[c];
        break;
    }
    case FA_AUTOCONTRAST:
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c)
            if (st.scale[c] != 0.0f) v[c] = fa_clamp((v[c] - st.lo[c]) * st.scale[c]);
        break;
    case FA_GRAY: {
        const float g = fa_gray(v[0], v[1], v[2]);
        v[0] = v[1] = v[2] = g;
        break;
    }
    case FA_NORMALIZE:
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c) v[c] = (v[c] - r[1 + c]) / r[5 + c];
        break;
    case FA_BRIGHTNESS:
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c) v[c] = fa_blend(r[1], r[2], v[c], 0.0f);
        break;
    case FA_CONTRAST:
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c) v[c] = fa_blend(r[1], r[2], v[c], st.mean);
        break;
    case FA_SATURATION:
        if (C == 3) {
            const float g = fa_gray(v[0], v[1], v[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = fa_blend(r[1], r[2], v[c], g);
        }
        break;
    case FA_HUE:
        if (C == 3) fa_hue(v, r[1]);
        break;
    case FA_ERASE: {
        const int y = pix / w, x = pix - y * w;
        const int y0 = fa_whole(r[1]), x0 = fa_whole(r[2]);
        const int y1 = min(y0 + fa_whole(r[3]), h), x1 = min(x0 + fa_whole(r[4]), w);   // clipped: sums stay below 2^17
        if (y >= y0 && y < y1 && x >= x0 && x < x1) {
#pragma unroll
            for (int c = 0; c < FA_MAX_C; ++c) v[c] = r[5 + c];
        }
        break;
    }
    default:
        break;
    }
}

// channels past C carry zeros through every operation and are never stored; a normalize row holds std = 1 there (a zero would only
// make a NaN that nobody reads)

// VEC = 4: h * w % 4 == 0 and x 16-byte aligned, so every plane of every frame starts on a 16-byte boundary and a thread's four
// neighbouring pixels of a plane move as one 16-byte access; VEC = 1: element accesses
template <int VEC>
__global__ __launch_bounds__(FA_THREADS) void frames_augment_kernel(AugArgs a) {
    __shared__ float s_prog[FA_MAX_OPS * FA_ROW];
    __shared__ int s_n;
    __shared__ double s_sum[FA_WAVES];
    __shared__ float s_lo[FA_WAVES][FA_MAX_C], s_hi[FA_WAVES][FA_MAX_C];
    __shared__ FaStat s_stat;
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.F);
    const int C = a.C;
    const float* prog = a.programs + (size_t)b * a.max_ops * FA_ROW;
    for (int i = tid; i < a.max_ops * FA_ROW; i += FA_THREADS) s_prog[i] = prog[i];
    __syncthreads();
    if (tid == 0) {
        // the program's length: up to the first row that is not an operation this frame can run
        int n = 0;
        for (; n < a.max_ops; ++n) {
            const float o = s_prog[n * FA_ROW];
            if (!(o >= 1.0f && o < (float)FA_NOPS) || o != truncf(o)) break;
            const int op = (int)o;
            if (op == FA_GRAY && C != 3) break;
            if ((op == FA_CONTRAST || op == FA_SATURATION || op == FA_HUE) && C != 1 && C != 3) break;
        }
        s_n = n;
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) return;                                                // an empty program: the frame is not touched
    const size_t plane = (size_t)a.npix;
    float* frame = a.x + (size_t)blockIdx.x * C * plane;               // 64-bit offsets throughout
    const int groups = a.npix / VEC;
    int pc = 0;
    bool have = false;                                                 // row pc is a statistic operation whose statistic sits in s_stat
    while (pc < n) {
        int stop = pc + (have ? 1 : 0);
        int next = FA_END;
        for (; stop < n; ++stop) {
            const int op = (int)s_prog[stop * FA_ROW];
            if (op == FA_AUTOCONTRAST || op == FA_CONTRAST) { next = op; break; }
        }
        const bool write = stop > pc;                                  // at least one operation applies in this sweep
        double sum = 0.0;
        float lo[FA_MAX_C], hi[FA_MAX_C];
#pragma unroll
        for (int c = 0; c < FA_MAX_C; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
        const FaStat st = s_stat;                                      // (read by an operation only when `have`)
        for (int g = tid; g < groups; g += FA_THREADS) {
            float v[VEC][FA_MAX_C];
            float* px = frame + (size_t)g * VEC;
#pragma unroll
            for (int c = 0; c < FA_MAX_C; ++c) {
                if (c < C) {
                    if (VEC == 4) {
                        const fa_f32x4 t = *reinterpret_cast<const fa_f32x4*>(px + (size_t)c * plane);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) v[k][c] = t[k];
                    } else {
                        v[0][c] = px[(size_t)c * plane];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) v[k][c] = 0.0f;
                }
            }
            for (int i = pc; i < stop; ++i) {
                const float* r = s_prog + i * FA_ROW;
                const int op = (int)r[0];
#pragma unroll
                for (int k = 0; k < VEC; ++k) fa_apply(op, r, st, v[k], C, g * VEC + k, a.h, a.w);
            }
            if (next == FA_CONTRAST) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) sum += (double)(C == 3 ? fa_gray(v[k][0], v[k][1], v[k][2]) : v[k][0]);
            } else if (next == FA_AUTOCONTRAST) {
#pragma unroll
                for (int k = 0; k < VEC; ++k)
#pragma unroll
                    for (int c = 0; c < FA_MAX_C; ++c) { lo[c] = fminf(lo[c], v[k][c]); hi[c] = fmaxf(hi[c], v[k][c]); }
            }
            if (write) {
#pragma unroll
                for (int c = 0; c < FA_MAX_C; ++c) {
                    if (c < C) {
                        if (VEC == 4) {
                            fa_f32x4 t;
#pragma unroll
                            for (int k = 0; k < VEC; ++k) t[k] = v[k][c];
                            *reinterpret_cast<fa_f32x4*>(px + (size_t)c * plane) = t;
                        } else {
                            px[(size_t)c * plane] = v[0][c];
                        }
                    }
                }
            }
        }
        if (next == FA_END) break;
        // the statistic: lanes by shuffles, waves through LDS, thread 0 combines the waves — one fixed tree
        if (next == FA_CONTRAST) {
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
        } else {
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int c = 0; c < FA_MAX_C; ++c) {
                    lo[c] = fminf(lo[c], __shfl_down(lo[c], off, 64));
                    hi[c] = fmaxf(hi[c], __shfl_down(hi[c], off, 64));
                }
            }
        }
        if ((tid & 63) == 0) {
            s_sum[tid >> 6] = sum;
#pragma unroll
            for (int c = 0; c < FA_MAX_C; ++c) { s_lo[tid >> 6][c] = lo[c]; s_hi[tid >> 6][c] = hi[c]; }
        }
        __syncthreads();
        if (tid == 0) {
            const double total = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
            s_stat.mean = (float)(total / (double)a.npix);
#pragma unroll
            for (int c = 0; c < FA_MAX_C; ++c) {
                const float l = fminf(fminf(s_lo[0][c], s_lo[1][c]), fminf(s_lo[2][c], s_lo[3][c]));
                const float u = fmaxf(fmaxf(s_hi[0][c], s_hi[1][c]), fmaxf(s_hi[2][c], s_hi[3][c]));
                s_stat.lo[c] = l;
                s_stat.scale[c] = (c < C && u != l) ? 1.0f / (u - l) : 0.0f;
            }
        }
        __syncthreads();
        pc = stop;
        have = true;
    }
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_frames_augment(float* x, const float* programs, int B, int n_frames, int C, int h, int w, int max_ops, void* stream) {
    const char* who = "vpx_frames_augment";
    if (!x || !programs) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || C < 1 || h < 1 || w < 1) { set_error("%s: every size must be >= 1 (got B=%d F=%d C=%d h=%d w=%d)", who, B, n_frames, C, h, w); return VPX_ERR_ARG; }
    if (max_ops < FA_MIN_OPS || max_ops > FA_MAX_OPS) { set_error("%s: max_ops %d outside [%d, %d]", who, max_ops, FA_MIN_OPS, FA_MAX_OPS); return VPX_ERR_ARG; }
    if (C > FA_MAX_C) { set_error("%s: %d channels exceed the kernel's %d", who, C, FA_MAX_C); return VPX_ERR_UNSUPPORTED; }
    if (h > FA_MAX_SIDE || w > FA_MAX_SIDE) { set_error("%s: a side beyond %d (%dx%d)", who, FA_MAX_SIDE, h, w); return VPX_ERR_UNSUPPORTED; }
    if ((long long)B * n_frames > 2147483647LL) { set_error("%s: %d samples of %d frames exceed one launch", who, B, n_frames); return VPX_ERR_UNSUPPORTED; }
    AugArgs a;
    a.x = x; a.programs = programs; a.F = n_frames; a.C = C; a.h = h; a.w = w; a.max_ops = max_ops;
    a.npix = h * w;
    const unsigned blocks = (unsigned)((long long)B * n_frames);
    const bool vec = a.npix % 4 == 0 && ((uintptr_t)x & 15) == 0;
    if (vec) VPX_LAUNCH((frames_augment_kernel<4>), dim3(blocks), dim3(FA_THREADS), 0, (hipStream_t)stream, a);
    else VPX_LAUNCH((frames_augment_kernel<1>), dim3(blocks), dim3(FA_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
