// Stored frames to a model-ready batch and back (vp_suite/base/base_dataset.py:233-273 preprocess, :293-297 postprocess; the gray
// repeat of vp_suite/datasets/mmnist.py:56), one launch each.
//   vpx_frames_preprocess    src [N][T'][H][W][Cs] (uint8 / uint16 / float32, channels last as the files hold them) and a device table
//                            int32 [B][4] = (sequence, crop y0, crop x0, flip bits) -> out float32 [B][F][C_out][oh][ow]
//   vpx_clips_preprocess     src [frames][H][W][Cs]: every clip of a split back to back, clip_first int64 [n_clips + 1] (on the device) and a
//                            device table int32 [B][6] = (clip, start frame within it, crop y0, crop x0, flip bits, 0) -> the same output,
//                            out[b][t] from frame clip_first[clip] + start + t * step; the SAME per-pixel code (fr_group)
//   vpx_clips_preprocess_var src: ONE element buffer, clips of DIFFERENT frame sizes back to back; clip_geom int64 [n_clips][4] = (element
//                            offset, frames, H_i, W_i) and a device table int32 [B][8] = (clip, start frame, box y0, box x0, box h, box w,
//                            flip bits, 0) -> the same output: each sample's box through fr_group with that sample's sizes
//   vpx_actions_diff_gather  src [frames][A] (float32 / float64) per-frame positions, clip_first and the table of the launch above ->
//                            out float32 [B][F - 1][A] = float(src[g(j + 1)] - src[g(j)]), the subtraction in the stored precision
//   vpx_frames_postprocess   x float32 [N][C][h][w] -> out uint8 [N][h][w][C]; x is only read
//   vpx_actions_gather       src [N][T'][A] (float32 / float64) and the same device table -> out float32 [B][F][A]: the action rows that go
//                            with the frames of a batch, out[b][t][:] = float(src[table[b].seq][t * step][:]); a conversion, no arithmetic
// Streaming kernels: a thread owns four neighbouring output pixels of one row in every channel, so a channel plane receives one 16-byte
// store per thread where the rows allow it, and on the path without resize every source element is read exactly once (for Cs = 3 the
// thread's four pixels are 12 contiguous bytes). The resize path gathers four taps per pixel and channel from the same family.
//
// Pixel contract of the preprocess (tests/frames_ref.py restates it), every step ONE correctly rounded float32 operation:
//   v = float(raw) / 255.0f (uint16: / 65535.0f; float32 passes through);
//   only if (lo, hi) != (0, 1):  v = v * float(hi - lo), then v = v + float(lo)   (the difference formed in double by the caller's language);
//   without resize (crop size == output size) that is the output: bit-exact against numpy and the reference.
//   With resize (bilinear, align_corners = False, no antialiasing — ATen's upsample_bilinear2d), per axis, in float32:
//     s = float(in) / float(out);  src = max(s * (d + 0.5f) - 0.5f, 0);  i0 = int(src);  i1 = min(i0 + 1, in - 1);  l = src - i0;
//   the taps are the scaled values v; horizontally first, r = v0 * (1 - l) + v1 * l, then the same vertically. Held to a bound, not bits.
//   Flips act on the OUTPUT index, after the resize: out[y][x] = r[oh - 1 - y if bit 1 else y][ow - 1 - x if bit 0 else x].
// Postprocess, in float32: v = ((x - float(lo)) / float(hi - lo)) * 255.0f, clamped to [0, 255], truncated toward zero; NaN gives 0.
#include <hip/hip_runtime.h>
#include "vpx_internal.h"
#include "vpx_host.h"

// Every operation of this file is rounded on its own (see mmnist.hip): no a * b + c becomes a fused multiply-add.
#pragma clang fp contract(off)

#include "frames_coord.h"
#include "frames_byte.h"   // fr_byte: the float -> byte rule of the postprocess, shared with vis.hip

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FR_THREADS = 256;
constexpr int FR_MAX_CS = 4;          // source channels a thread keeps in registers (gray, gray + alpha, RGB, RGBA)
constexpr int FR_MAX_SIDE = 32768;    // frame, crop and output sides: coordinates and their float32 images stay exact

struct FramesArgs {
    const void* src;                   // [N][Tp][H][W][Cs]
    const int* table;                  // [B][4] = (sequence, crop y0, crop x0, flip bits)
    float* out;                        // [B][F][C_out][oh][ow]
    long long N;
    long long items;                   // B * F * oh * Q: one thread each
    int Tp, H, W, Cs, B, F, step, ch, cw, oh, ow, Cout;
    int Q;                             // groups of four pixels per output row (the last one partial if ow % 4)
    int vec;                           // 1: ow % 4 == 0 and `out` 16-byte aligned — every group is one 16-byte store per plane
    int scaled;                        // 1: (lo, hi) != (0, 1)
    float scale, lo;                   // float(hi - lo), float(lo)
    float sy, sx;                      // float(ch) / float(oh), float(cw) / float(ow)
};

template <typename T> __device__ __forceinline__ float fr_unit(T raw);
template <> __device__ __forceinline__ float fr_unit<unsigned char>(unsigned char raw) { return (float)raw / 255.0f; }
template <> __device__ __forceinline__ float fr_unit<unsigned short>(unsigned short raw) { return (float)raw / 65535.0f; }
template <> __device__ __forceinline__ float fr_unit<float>(float raw) { return raw; }

template <typename T> __device__ __forceinline__ float fr_value(const FramesArgs& a, T raw) {
    float v = fr_unit<T>(raw);
    if (a.scaled) {
        v = v * a.scale;
        v = v + a.lo;
    }
    return v;
}

// fr_coord(): ATen's source coordinate of destination index d (area_pixel_compute_source_index, align_corners = False) — frames_coord.h,
// shared with adapt.hip.

// The four neighbouring output pixels (row y, columns x0 .. x0 + 3) of output frame (b, f) in every channel, from the stored frame
// `frame` [H][W][Cs] and the row's box and flips: the pixel contract above, once, for every kernel that gathers stored frames
// (frames_preprocess_kernel: equal-length sequences; clips_preprocess_kernel: windows of long clips; clips_var_kernel: clips of mixed
// frame sizes). The row stride W, the box ch x cw and its scales sy, sx are arguments: the first two kernels hand over the launch's,
// the third its sample's. !valid: zeros, nothing is read.
template <typename T, int RESIZE>
__device__ __forceinline__ void fr_group(const FramesArgs& a, const T* frame, bool valid, int W, int ch, int cw, float sy, float sx, int cy, int cx, int flip,
                                         int b, int f, int y, int x0) {
    const int yr = (flip & 2) ? a.oh - 1 - y : y;
    float v[FR_MAX_CS][4];
#pragma unroll
    for (int c = 0; c < FR_MAX_CS; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = 0.0f;
    if (valid) {
        if (!RESIZE) {
            const T* line = frame + (size_t)(cy + yr) * W * a.Cs;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                if (x >= a.ow) break;
                const int xr = (flip & 1) ? a.ow - 1 - x : x;
                const T* px = line + (size_t)(cx + xr) * a.Cs;
#pragma unroll
                for (int c = 0; c < FR_MAX_CS; ++c)
                    if (c < a.Cs) v[c][k] = fr_value<T>(a, px[c]);
            }
        } else {
            int iy0, iy1;
            float ly;
            fr_coord(sy, yr, ch, iy0, iy1, ly);
            const T* top = frame + (size_t)(cy + iy0) * W * a.Cs;
            const T* bot = frame + (size_t)(cy + iy1) * W * a.Cs;
            const float wy = 1.0f - ly;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                if (x >= a.ow) break;
                const int xr = (flip & 1) ? a.ow - 1 - x : x;
                int ix0, ix1;
                float lx;
                fr_coord(sx, xr, cw, ix0, ix1, lx);
                const float wx = 1.0f - lx;
                const size_t o0 = (size_t)(cx + ix0) * a.Cs, o1 = (size_t)(cx + ix1) * a.Cs;
#pragma unroll
                for (int c = 0; c < FR_MAX_CS; ++c) {
                    if (c < a.Cs) {
                        const float t = fr_value<T>(a, top[o0 + c]) * wx + fr_value<T>(a, top[o1 + c]) * lx;
                        const float u = fr_value<T>(a, bot[o0 + c]) * wx + fr_value<T>(a, bot[o1 + c]) * lx;
                        v[c][k] = t * wy + u * ly;
                    }
                }
            }
        }
    }
    const size_t plane = (size_t)a.oh * a.ow;
    float* dst = a.out + ((size_t)b * a.F + f) * a.Cout * plane + (size_t)y * a.ow + x0;
#pragma unroll
    for (int c = 0; c < FR_MAX_CS; ++c) {
        if (c >= a.Cout) break;
        const int cs = a.Cs == 1 ? 0 : c;                              // the gray repeat: every plane carries channel 0
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = cs == 0 ? v[0][k] : (cs == 1 ? v[1][k] : (cs == 2 ? v[2][k] : v[3][k]));
        if (a.vec) *reinterpret_cast<f32x4*>(dst) = o;
        else
            for (int k = 0; k < 4 && x0 + k < a.ow; ++k) dst[k] = o[k];
        dst += plane;
    }
}

// thread = (sample b, frame f, output row y, group of four output pixels). RESIZE = 0: crop size == output size.
template <typename T, int RESIZE>
__global__ __launch_bounds__(FR_THREADS) void frames_preprocess_kernel(FramesArgs a) {
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int q = (int)(item % a.Q);
    long long r = item / a.Q;
    const int y = (int)(r % a.oh);
    r /= a.oh;
    const int f = (int)(r % a.F);
    const int b = (int)(r / a.F);
    const int* row = a.table + (size_t)b * 4;
    const long long seq = row[0];
    const int cy = row[1], cx = row[2], flip = row[3];
    // a row the caller did not check (the table lives on the device) reads nothing out of bounds: it yields zeros
    const bool valid = seq >= 0 && seq < a.N && cy >= 0 && cx >= 0 && (long long)cy + a.ch <= a.H && (long long)cx + a.cw <= a.W;
    const T* frame = (const T*)a.src + ((size_t)(valid ? seq : 0) * a.Tp + (size_t)f * a.step) * ((size_t)a.H * a.W * a.Cs);   // 64-bit offsets throughout
    fr_group<T, RESIZE>(a, frame, valid, a.W, a.ch, a.cw, a.sy, a.sx, cy, cx, flip, b, f, y, q << 2);
}

// Windows of long clips: src holds every clip of a split back to back, clip c being frames clip_first[c] .. clip_first[c + 1] - 1;
// a table row is (clip, start frame within the clip, crop y0, crop x0, flip bits, 0) and output frame f of sample b is stored frame
// clip_first[clip] + start + f * step. Everything after the frame pointer is fr_group(), so the pixels are those of the kernel above.
struct ClipsArgs {
    FramesArgs fr;                     // src, out and the geometry; table, N and Tp are not used
    const long long* clip_first;       // [n_clips + 1], on the device; the last entry is the number of frames in src
    const int* table;                  // [B][6]
    long long n_clips, total;          // total: frames in src
};

template <typename T, int RESIZE>
__global__ __launch_bounds__(FR_THREADS) void clips_preprocess_kernel(ClipsArgs c) {
    const FramesArgs& a = c.fr;
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int q = (int)(item % a.Q);
    long long r = item / a.Q;
    const int y = (int)(r % a.oh);
    r /= a.oh;
    const int f = (int)(r % a.F);
    const int b = (int)(r / a.F);
    const int* row = c.table + (size_t)b * 6;
    const long long clip = row[0], start = row[1];
    const int cy = row[2], cx = row[3], flip = row[4];
    // as above: a row (or an offset table) the caller did not check yields zeros and reads nothing outside src
    bool valid = clip >= 0 && clip < c.n_clips && start >= 0 && cy >= 0 && cx >= 0 && (long long)cy + a.ch <= a.H && (long long)cx + a.cw <= a.W;
    long long first = 0;
    if (valid) {
        first = c.clip_first[clip];
        const long long end = c.clip_first[clip + 1];
        valid = first >= 0 && end <= c.total && first + start + (long long)(a.F - 1) * a.step < end;
    }
    const T* frame = (const T*)a.src + (size_t)(valid ? first + start + (long long)f * a.step : 0) * ((size_t)a.H * a.W * a.Cs);   // 64-bit offsets throughout
    fr_group<T, RESIZE>(a, frame, valid, a.W, a.ch, a.cw, a.sy, a.sx, cy, cx, flip, b, f, y, q << 2);
}

// Windows of clips whose frame sizes differ: src is ONE element buffer holding every clip back to back and clip_geom [n_clips][4] =
// (element offset of the clip's first frame, frame count, H_i, W_i) says where each lies. A table row is (clip, start frame, box y0,
// box x0, box h, box w, flip bits, 0): the box of stored frame start + f * step goes to oh x ow through fr_group(), with the sample's row
// stride, box and scales where the kernels above hand over the launch's. A box of the output's size takes the path without resize, so
// equal shapes give the bits of clips_preprocess_kernel; the choice is per sample (uniform over a sample's threads).
struct ClipsVarArgs {
    FramesArgs fr;                     // src, out, Cs, F, step, oh, ow, Cout and the value map; H, W, ch, cw, sy, sx are not used
    const long long* geom;             // [n_clips][4], on the device
    const int* table;                  // [B][8]
    long long n_clips, total;          // total: elements in src
};

template <typename T>
__global__ __launch_bounds__(FR_THREADS) void clips_var_kernel(ClipsVarArgs c) {
    const FramesArgs& a = c.fr;
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int q = (int)(item % a.Q);
    long long r = item / a.Q;
    const int y = (int)(r % a.oh);
    r /= a.oh;
    const int f = (int)(r % a.F);
    const int b = (int)(r / a.F);
    const int* row = c.table + (size_t)b * 8;
    const long long clip = row[0], start = row[1];
    const int cy = row[2], cx = row[3], bh = row[4], bw = row[5], flip = row[6];
    // as above: a row (or a geometry table) the caller did not check yields zeros and reads nothing outside src
    bool valid = clip >= 0 && clip < c.n_clips && start >= 0 && cy >= 0 && cx >= 0 && bh >= 1 && bw >= 1;
    long long first = 0, frame_elems = 0;
    int W = 1;
    if (valid) {
        const long long* g = c.geom + (size_t)clip * 4;
        const long long count = g[1], H = g[2], Wl = g[3];
        first = g[0];
        valid = first >= 0 && first <= c.total && count >= 1 && H >= 1 && Wl >= 1 && H <= FR_MAX_SIDE && Wl <= FR_MAX_SIDE &&
                (long long)cy + bh <= H && (long long)cx + bw <= Wl && start + (long long)(a.F - 1) * a.step < count;
        if (valid) {
            frame_elems = H * Wl * a.Cs;                                                              // <= 2^32: no overflow
            valid = count <= (c.total - first) / frame_elems;                                         // the whole clip lies inside src
            W = (int)Wl;
        }
    }
    const T* frame = (const T*)a.src + (size_t)(valid ? first + (start + (long long)f * a.step) * frame_elems : 0);   // 64-bit offsets throughout
    if (valid && (bh != a.oh || bw != a.ow))
        fr_group<T, 1>(a, frame, true, W, bh, bw, (float)bh / (float)a.oh, (float)bw / (float)a.ow, cy, cx, flip, b, f, y, q << 2);
    else
        fr_group<T, 0>(a, frame, valid, W, bh, bw, 1.0f, 1.0f, cy, cx, flip, b, f, y, q << 2);
}

struct PostArgs {
    const float* x;                    // [N][C][h][w]
    unsigned char* out;                // [N][h][w][C]
    long long items;                   // N * h * Q
    int C, h, w, Q;
    int vec;                           // 1: w % 4 == 0, C <= 4 and `out` 4-byte aligned — a thread's 4 * C bytes leave as C 32-bit stores
    float scale, lo;                   // float(hi - lo), float(lo)
};

// thread = (image n, row y, group of four pixels): reads its four pixels of every plane, writes their 4 * C interleaved bytes
__global__ __launch_bounds__(FR_THREADS) void frames_postprocess_kernel(PostArgs a) {
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int q = (int)(item % a.Q);
    const long long r = item / a.Q;
    const int y = (int)(r % a.h);
    const long long n = r / a.h;
    const int x0 = q << 2;
    const size_t plane = (size_t)a.h * a.w;
    const float* src = a.x + (size_t)n * a.C * plane + (size_t)y * a.w + x0;
    unsigned char* dst = a.out + ((size_t)n * plane + (size_t)y * a.w + x0) * a.C;
    if (a.vec) {
        unsigned words[4] = {0u, 0u, 0u, 0u};                          // 4 * C <= 16 bytes, little endian: byte j = pixel j / C, channel j % C
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= a.C) break;
            const f32x4 p = *reinterpret_cast<const f32x4*>(src + (size_t)c * plane);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = k * a.C + c;
                const unsigned byte = fr_byte(a.lo, a.scale, p[k]) << ((j & 3) * 8);
#pragma unroll
                for (int wd = 0; wd < 4; ++wd)
                    if ((j >> 2) == wd) words[wd] |= byte;
            }
        }
#pragma unroll
        for (int wd = 0; wd < 4; ++wd)
            if (wd < a.C) reinterpret_cast<unsigned*>(dst)[wd] = words[wd];
    } else {
        for (int k = 0; k < 4 && x0 + k < a.w; ++k)
            for (int c = 0; c < a.C; ++c) dst[k * a.C + c] = (unsigned char)fr_byte(a.lo, a.scale, src[(size_t)c * plane + k]);
    }
}

struct ActionsArgs {
    const void* src;                   // [N][Tp][A]
    const int* table;                  // [B][4]: column 0, the sequence index, is all that is read
    float* out;                        // [B][F][A]
    long long N;
    long long items;                   // B * F * A: one thread each
    int Tp, A, F, step;
};

// thread = one output element (sample b, frame t, component a). float64 storage: the conversion rounds to nearest even (the default
// mode), as numpy's astype(float32) does; float32 storage is copied.
template <typename T>
__global__ __launch_bounds__(FR_THREADS) void actions_gather_kernel(ActionsArgs a) {
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int c = (int)(item % a.A);
    const long long r = item / a.A;
    const int t = (int)(r % a.F);
    const long long b = r / a.F;
    const long long seq = a.table[(size_t)b * 4];
    float v = 0.0f;                                                    // a row the caller did not check reads nothing out of bounds: zeros
    if (seq >= 0 && seq < a.N) v = (float)((const T*)a.src)[((size_t)seq * a.Tp + (size_t)t * a.step) * a.A + c];
    a.out[item] = v;
}

struct ActionsDiffArgs {
    const void* src;                   // [total][A]: per-frame positions, every clip back to back
    const long long* clip_first;       // [n_clips + 1], on the device
    const int* table;                  // [B][8], the table of clips_var_kernel: columns 0 (clip) and 1 (start frame) are all that is read
    float* out;                        // [B][F - 1][A]
    long long n_clips, total;          // total: rows in src
    long long items;                   // B * (F - 1) * A: one thread each
    int A, F, step;
};

// thread = one output element (sample b, step j, component a): the difference of the rows of frames j + 1 and j of the window, formed
// in the STORED precision and rounded to float32 once (float64: to nearest even) — numpy's (new - old), then .float().
template <typename T>
__global__ __launch_bounds__(FR_THREADS) void actions_diff_kernel(ActionsDiffArgs a) {
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int c = (int)(item % a.A);
    const long long r = item / a.A;
    const int j = (int)(r % (a.F - 1));
    const long long b = r / (a.F - 1);
    const int* row = a.table + (size_t)b * 8;
    const long long clip = row[0], start = row[1];
    float v = 0.0f;                                                    // a row the caller did not check reads nothing out of bounds: zeros
    if (clip >= 0 && clip < a.n_clips && start >= 0) {
        const long long first = a.clip_first[clip], end = a.clip_first[clip + 1];
        if (first >= 0 && end <= a.total && first + start + (long long)(a.F - 1) * a.step < end) {
            const T* old_row = (const T*)a.src + (size_t)(first + start + (long long)j * a.step) * a.A;
            const T* new_row = old_row + (size_t)a.step * a.A;
            const T d = new_row[c] - old_row[c];
            v = (float)d;
        }
    }
    a.out[item] = v;
}

template <typename T>
static void launch_preprocess(const FramesArgs& a, int resize, unsigned blocks, hipStream_t stream) {
    if (resize) VPX_LAUNCH((frames_preprocess_kernel<T, 1>), dim3(blocks), dim3(FR_THREADS), 0, stream, a);
    else VPX_LAUNCH((frames_preprocess_kernel<T, 0>), dim3(blocks), dim3(FR_THREADS), 0, stream, a);
}

template <typename T>
static void launch_clips(const ClipsArgs& c, int resize, unsigned blocks, hipStream_t stream) {
    if (resize) VPX_LAUNCH((clips_preprocess_kernel<T, 1>), dim3(blocks), dim3(FR_THREADS), 0, stream, c);
    else VPX_LAUNCH((clips_preprocess_kernel<T, 0>), dim3(blocks), dim3(FR_THREADS), 0, stream, c);
}

// What both gathers hand fr_group(): the geometry, the value map and the destination (checked by the entry points).
static FramesArgs frames_args(const void* src, float* out, int H, int W, int Cs, int B, int n_frames, int seq_step, int ch, int cw, int oh, int ow,
                              int C_out, double lo, double hi) {
    FramesArgs a;
    a.src = src; a.table = nullptr; a.out = out;
    a.N = 0; a.Tp = 0; a.H = H; a.W = W; a.Cs = Cs; a.B = B; a.F = n_frames; a.step = seq_step;
    a.ch = ch; a.cw = cw; a.oh = oh; a.ow = ow; a.Cout = C_out; a.Q = (ow + 3) / 4;
    a.items = (long long)B * n_frames * oh * a.Q;
    a.vec = (ow % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    a.scaled = (lo != 0.0 || hi != 1.0) ? 1 : 0;
    a.scale = (float)(hi - lo);
    a.lo = (float)lo;
    a.sy = (float)ch / (float)oh;
    a.sx = (float)cw / (float)ow;
    return a;
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_frames_preprocess(const void* src, int dtype, long long N, int Tp, int H, int W, int Cs, const int* table, int B, int n_frames,
                          int seq_step, int ch, int cw, int oh, int ow, int C_out, double lo, double hi, float* out, void* stream) {
    const char* who = "vpx_frames_preprocess";
    if (!src || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (dtype != VPX_FRAMES_U8 && dtype != VPX_FRAMES_U16 && dtype != VPX_FRAMES_F32) { set_error("%s: unknown element type %d (uint8, uint16 and float32 are stored)", who, dtype); return VPX_ERR_ARG; }
    if (N < 1 || Tp < 1 || H < 1 || W < 1 || Cs < 1) { set_error("%s: every source size must be >= 1 (got N=%lld T'=%d H=%d W=%d Cs=%d)", who, N, Tp, H, W, Cs); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || seq_step < 1) { set_error("%s: B, n_frames and seq_step must be >= 1 (got %d, %d, %d)", who, B, n_frames, seq_step); return VPX_ERR_ARG; }
    if (ch < 1 || cw < 1 || oh < 1 || ow < 1) { set_error("%s: crop and output sizes must be >= 1 (got crop %dx%d, output %dx%d)", who, ch, cw, oh, ow); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step >= Tp) { set_error("%s: frame %d at step %d lies past the %d stored frames", who, n_frames - 1, seq_step, Tp); return VPX_ERR_ARG; }
    if (ch > H || cw > W) { set_error("%s: the %dx%d crop box lies outside the %dx%d frame (there is no padding)", who, ch, cw, H, W); return VPX_ERR_ARG; }
    if (C_out != Cs && !(Cs == 1 && C_out == 3)) { set_error("%s: %d output channels from %d stored ones (equal, or 3 from 1)", who, C_out, Cs); return VPX_ERR_ARG; }
    if (hi == lo) { set_error("%s: empty value range [%g, %g]", who, lo, hi); return VPX_ERR_ARG; }
    if (Cs > FR_MAX_CS) { set_error("%s: %d stored channels exceed the kernel's %d", who, Cs, FR_MAX_CS); return VPX_ERR_UNSUPPORTED; }
    if (H > FR_MAX_SIDE || W > FR_MAX_SIDE || oh > FR_MAX_SIDE || ow > FR_MAX_SIDE) { set_error("%s: a side beyond %d (frame %dx%d, output %dx%d)", who, FR_MAX_SIDE, H, W, oh, ow); return VPX_ERR_UNSUPPORTED; }
    const int Q = (ow + 3) / 4;
    const double items_d = (double)B * n_frames * oh * Q;
    if (items_d / FR_THREADS + 1.0 > 2147483647.0) { set_error("%s: %d samples of %d %dx%d frames exceed one launch", who, B, n_frames, oh, ow); return VPX_ERR_UNSUPPORTED; }
    FramesArgs a = frames_args(src, out, H, W, Cs, B, n_frames, seq_step, ch, cw, oh, ow, C_out, lo, hi);
    a.table = table; a.N = N; a.Tp = Tp;
    const int resize = (ch != oh || cw != ow) ? 1 : 0;
    const unsigned blocks = (unsigned)((a.items + FR_THREADS - 1) / FR_THREADS);
    if (dtype == VPX_FRAMES_U8) launch_preprocess<unsigned char>(a, resize, blocks, (hipStream_t)stream);
    else if (dtype == VPX_FRAMES_U16) launch_preprocess<unsigned short>(a, resize, blocks, (hipStream_t)stream);
    else launch_preprocess<float>(a, resize, blocks, (hipStream_t)stream);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_clips_preprocess(const void* src, int dtype, long long total_frames, int H, int W, int Cs, const long long* clip_first, long long n_clips,
                         const int* table, int B, int n_frames, int seq_step, int ch, int cw, int oh, int ow, int C_out, double lo, double hi,
                         float* out, void* stream) {
    const char* who = "vpx_clips_preprocess";
    if (!src || !clip_first || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (dtype != VPX_FRAMES_U8 && dtype != VPX_FRAMES_U16 && dtype != VPX_FRAMES_F32) { set_error("%s: unknown element type %d (uint8, uint16 and float32 are stored)", who, dtype); return VPX_ERR_ARG; }
    if (total_frames < 1 || n_clips < 1 || H < 1 || W < 1 || Cs < 1) { set_error("%s: every source size must be >= 1 (got frames=%lld clips=%lld H=%d W=%d Cs=%d)", who, total_frames, n_clips, H, W, Cs); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || seq_step < 1) { set_error("%s: B, n_frames and seq_step must be >= 1 (got %d, %d, %d)", who, B, n_frames, seq_step); return VPX_ERR_ARG; }
    if (ch < 1 || cw < 1 || oh < 1 || ow < 1) { set_error("%s: crop and output sizes must be >= 1 (got crop %dx%d, output %dx%d)", who, ch, cw, oh, ow); return VPX_ERR_ARG; }
    if (n_clips > total_frames) { set_error("%s: %lld clips in %lld stored frames (a clip holds at least one)", who, n_clips, total_frames); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step >= total_frames) { set_error("%s: frame %d at step %d lies past the %lld stored frames", who, n_frames - 1, seq_step, total_frames); return VPX_ERR_ARG; }
    if (ch > H || cw > W) { set_error("%s: the %dx%d crop box lies outside the %dx%d frame (there is no padding)", who, ch, cw, H, W); return VPX_ERR_ARG; }
    if (C_out != Cs && !(Cs == 1 && C_out == 3)) { set_error("%s: %d output channels from %d stored ones (equal, or 3 from 1)", who, C_out, Cs); return VPX_ERR_ARG; }
    if (hi == lo) { set_error("%s: empty value range [%g, %g]", who, lo, hi); return VPX_ERR_ARG; }
    if (Cs > FR_MAX_CS) { set_error("%s: %d stored channels exceed the kernel's %d", who, Cs, FR_MAX_CS); return VPX_ERR_UNSUPPORTED; }
    if (H > FR_MAX_SIDE || W > FR_MAX_SIDE || oh > FR_MAX_SIDE || ow > FR_MAX_SIDE) { set_error("%s: a side beyond %d (frame %dx%d, output %dx%d)", who, FR_MAX_SIDE, H, W, oh, ow); return VPX_ERR_UNSUPPORTED; }
    const double items_d = (double)B * n_frames * oh * ((ow + 3) / 4);
    if (items_d / FR_THREADS + 1.0 > 2147483647.0) { set_error("%s: %d samples of %d %dx%d frames exceed one launch", who, B, n_frames, oh, ow); return VPX_ERR_UNSUPPORTED; }
    ClipsArgs c;
    c.fr = frames_args(src, out, H, W, Cs, B, n_frames, seq_step, ch, cw, oh, ow, C_out, lo, hi);
    c.clip_first = clip_first; c.table = table; c.n_clips = n_clips; c.total = total_frames;
    const int resize = (ch != oh || cw != ow) ? 1 : 0;
    const unsigned blocks = (unsigned)((c.fr.items + FR_THREADS - 1) / FR_THREADS);
    if (dtype == VPX_FRAMES_U8) launch_clips<unsigned char>(c, resize, blocks, (hipStream_t)stream);
    else if (dtype == VPX_FRAMES_U16) launch_clips<unsigned short>(c, resize, blocks, (hipStream_t)stream);
    else launch_clips<float>(c, resize, blocks, (hipStream_t)stream);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_clips_preprocess_var(const void* src, int dtype, long long total_elems, int Cs, const long long* clip_geom, long long n_clips, const int* table,
                             int B, int n_frames, int seq_step, int oh, int ow, int C_out, double lo, double hi, float* out, void* stream) {
    const char* who = "vpx_clips_preprocess_var";
    if (!src || !clip_geom || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (dtype != VPX_FRAMES_U8 && dtype != VPX_FRAMES_U16 && dtype != VPX_FRAMES_F32) { set_error("%s: unknown element type %d (uint8, uint16 and float32 are stored)", who, dtype); return VPX_ERR_ARG; }
    if (total_elems < 1 || n_clips < 1 || Cs < 1) { set_error("%s: every source size must be >= 1 (got elements=%lld clips=%lld Cs=%d)", who, total_elems, n_clips, Cs); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || seq_step < 1) { set_error("%s: B, n_frames and seq_step must be >= 1 (got %d, %d, %d)", who, B, n_frames, seq_step); return VPX_ERR_ARG; }
    if (oh < 1 || ow < 1) { set_error("%s: output sizes must be >= 1 (got output %dx%d)", who, oh, ow); return VPX_ERR_ARG; }
    if (n_clips > total_elems / Cs) { set_error("%s: %lld clips in %lld stored elements of %d channels (a clip holds at least one frame of one pixel)", who, n_clips, total_elems, Cs); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step >= total_elems / Cs) { set_error("%s: frame %d at step %d lies past the %lld stored elements", who, n_frames - 1, seq_step, total_elems); return VPX_ERR_ARG; }
    if (C_out != Cs && !(Cs == 1 && C_out == 3)) { set_error("%s: %d output channels from %d stored ones (equal, or 3 from 1)", who, C_out, Cs); return VPX_ERR_ARG; }
    if (hi == lo) { set_error("%s: empty value range [%g, %g]", who, lo, hi); return VPX_ERR_ARG; }
    if (Cs > FR_MAX_CS) { set_error("%s: %d stored channels exceed the kernel's %d", who, Cs, FR_MAX_CS); return VPX_ERR_UNSUPPORTED; }
    if (oh > FR_MAX_SIDE || ow > FR_MAX_SIDE) { set_error("%s: a side beyond %d (output %dx%d)", who, FR_MAX_SIDE, oh, ow); return VPX_ERR_UNSUPPORTED; }
    const double items_d = (double)B * n_frames * oh * ((ow + 3) / 4);
    if (items_d / FR_THREADS + 1.0 > 2147483647.0) { set_error("%s: %d samples of %d %dx%d frames exceed one launch", who, B, n_frames, oh, ow); return VPX_ERR_UNSUPPORTED; }
    ClipsVarArgs c;
    c.fr = frames_args(src, out, 0, 0, Cs, B, n_frames, seq_step, oh, ow, oh, ow, C_out, lo, hi);   // (frame and box sizes come per sample)
    c.geom = clip_geom; c.table = table; c.n_clips = n_clips; c.total = total_elems;
    const unsigned blocks = (unsigned)((c.fr.items + FR_THREADS - 1) / FR_THREADS);
    if (dtype == VPX_FRAMES_U8) VPX_LAUNCH(clips_var_kernel<unsigned char>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, c);
    else if (dtype == VPX_FRAMES_U16) VPX_LAUNCH(clips_var_kernel<unsigned short>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, c);
    else VPX_LAUNCH(clips_var_kernel<float>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, c);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_actions_diff_gather(const void* src, int dtype, long long total_frames, int A, const long long* clip_first, long long n_clips, const int* table,
                            int B, int n_frames, int seq_step, float* out, void* stream) {
    const char* who = "vpx_actions_diff_gather";
    if (!src || !clip_first || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (dtype != VPX_ACTIONS_F32 && dtype != VPX_ACTIONS_F64) { set_error("%s: unknown element type %d (float32 and float64 are stored)", who, dtype); return VPX_ERR_ARG; }
    if (total_frames < 1 || n_clips < 1 || A < 1) { set_error("%s: every source size must be >= 1 (got frames=%lld clips=%lld A=%d)", who, total_frames, n_clips, A); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || seq_step < 1) { set_error("%s: B, n_frames and seq_step must be >= 1 (got %d, %d, %d)", who, B, n_frames, seq_step); return VPX_ERR_ARG; }
    if (n_frames < 2) { set_error("%s: a difference needs two frames (n_frames = %d)", who, n_frames); return VPX_ERR_ARG; }
    if (n_clips > total_frames) { set_error("%s: %lld clips in %lld stored frames (a clip holds at least one)", who, n_clips, total_frames); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step >= total_frames) { set_error("%s: frame %d at step %d lies past the %lld stored frames", who, n_frames - 1, seq_step, total_frames); return VPX_ERR_ARG; }
    const double items_d = (double)B * (n_frames - 1) * A;
    if (items_d / FR_THREADS + 1.0 > 2147483647.0) { set_error("%s: %d samples of %d rows of %d exceed one launch", who, B, n_frames - 1, A); return VPX_ERR_UNSUPPORTED; }
    ActionsDiffArgs a;
    a.src = src; a.clip_first = clip_first; a.table = table; a.out = out;
    a.n_clips = n_clips; a.total = total_frames; a.A = A; a.F = n_frames; a.step = seq_step;
    a.items = (long long)B * (n_frames - 1) * A;
    const unsigned blocks = (unsigned)((a.items + FR_THREADS - 1) / FR_THREADS);
    if (dtype == VPX_ACTIONS_F32) VPX_LAUNCH(actions_diff_kernel<float>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
    else VPX_LAUNCH(actions_diff_kernel<double>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_frames_postprocess(const float* x, long long N, int C, int h, int w, double lo, double hi, unsigned char* out, void* stream) {
    const char* who = "vpx_frames_postprocess";
    if (!x || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (N < 1 || C < 1 || h < 1 || w < 1) { set_error("%s: every size must be >= 1 (got N=%lld C=%d h=%d w=%d)", who, N, C, h, w); return VPX_ERR_ARG; }
    if (hi == lo) { set_error("%s: empty value range [%g, %g]", who, lo, hi); return VPX_ERR_ARG; }
    if (h > FR_MAX_SIDE || w > FR_MAX_SIDE) { set_error("%s: a side beyond %d (%dx%d)", who, FR_MAX_SIDE, h, w); return VPX_ERR_UNSUPPORTED; }
    const int Q = (w + 3) / 4;
    const double items_d = (double)N * h * Q;
    if (items_d / FR_THREADS + 1.0 > 2147483647.0) { set_error("%s: %lld images of %dx%d exceed one launch", who, N, h, w); return VPX_ERR_UNSUPPORTED; }
    PostArgs a;
    a.x = x; a.out = out; a.C = C; a.h = h; a.w = w; a.Q = Q;
    a.items = N * h * Q;
    a.vec = (w % 4 == 0 && C <= 4 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
    a.scale = (float)(hi - lo);
    a.lo = (float)lo;
    const unsigned blocks = (unsigned)((a.items + FR_THREADS - 1) / FR_THREADS);
    VPX_LAUNCH(frames_postprocess_kernel, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_actions_gather(const void* src, int dtype, long long N, int Tp, int A, const int* table, int B, int n_frames, int seq_step,
                       float* out, void* stream) {
    const char* who = "vpx_actions_gather";
    if (!src || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (dtype != VPX_ACTIONS_F32 && dtype != VPX_ACTIONS_F64) { set_error("%s: unknown element type %d (float32 and float64 are stored)", who, dtype); return VPX_ERR_ARG; }
    if (N < 1 || Tp < 1 || A < 1) { set_error("%s: every source size must be >= 1 (got N=%lld T'=%d A=%d)", who, N, Tp, A); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || seq_step < 1) { set_error("%s: B, n_frames and seq_step must be >= 1 (got %d, %d, %d)", who, B, n_frames, seq_step); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step + 1 > Tp) { set_error("%s: frame %d at step %d lies past the %d stored frames", who, n_frames - 1, seq_step, Tp); return VPX_ERR_ARG; }
    const double items_d = (double)B * n_frames * A;
    if (items_d / FR_THREADS + 1.0 > 2147483647.0) { set_error("%s: %d samples of %d rows of %d exceed one launch", who, B, n_frames, A); return VPX_ERR_UNSUPPORTED; }
    ActionsArgs a;
    a.src = src; a.table = table; a.out = out;
    a.N = N; a.Tp = Tp; a.A = A; a.F = n_frames; a.step = seq_step;
    a.items = (long long)B * n_frames * A;
    const unsigned blocks = (unsigned)((a.items + FR_THREADS - 1) / FR_THREADS);
    if (dtype == VPX_ACTIONS_F32) VPX_LAUNCH(actions_gather_kernel<float>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
    else VPX_LAUNCH(actions_gather_kernel<double>, dim3(blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
