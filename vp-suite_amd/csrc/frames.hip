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

// What every gather hands fr_group(): the stored elements, the destination and the value map. Where a frame lies in src, and which box of
// it is taken, is the business of the launch's locator (below).
struct FramesArgs {
    const void* src;                   // stored frames [H][W][Cs], channels last
    float* out;                        // [B][F][C_out][oh][ow]
    long long items;                   // B * F * oh * Q: one thread each
    int Cs, F, step, oh, ow, Cout;
    int Q;                             // groups of four pixels per output row (the last one partial if ow % 4)
    int vec;                           // 1: ow % 4 == 0 and `out` 16-byte aligned — every group is one 16-byte store per plane
    int scaled;                        // 1: (lo, hi) != (0, 1)
    float scale, lo;                   // float(hi - lo), float(lo)
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
// `frame` [H][W][Cs] and the row's box and flips: the pixel contract above, once, for every launch that gathers stored frames
// (SeqSource: equal-length sequences; ClipSource: windows of long clips; VarClipSource: clips of mixed frame sizes). The row stride W,
// the box ch x cw and its scales sy, sx are arguments: the first two locators hand over the launch's, the third its sample's.
// !valid: zeros, nothing is read.
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

// A locator says where the frames of a launch lie: locate(a, b, f) yields, for output frame (b, f), the arguments of fr_group().
// PER_SAMPLE: the locator, not the launch, chooses between copy and resize (FrSample::resize; otherwise not read).
template <typename T>
struct FrSample { const T* frame; int W, ch, cw; float sy, sx; int cy, cx, flip; bool valid, resize; };

// Stored sequences of equal length: src [N][Tp][H][W][Cs], a table row is (sequence, crop y0, crop x0, flip bits) and output frame f of
// sample b is stored frame f * step of that sequence. The crop box and its scales are the launch's.
struct SeqSource {
    static constexpr bool PER_SAMPLE = false;
    const int* table;                  // [B][4]
    long long N;
    int Tp, H, W, ch, cw;
    float sy, sx;                      // float(ch) / float(oh), float(cw) / float(ow)

    template <typename T> __device__ __forceinline__ FrSample<T> locate(const FramesArgs& a, int b, int f) const {
        const int* row = table + (size_t)b * 4;
        const long long seq = row[0];
        const int cy = row[1], cx = row[2], flip = row[3];
        // a row the caller did not check (the table lives on the device) reads nothing out of bounds: it yields zeros
        const bool valid = seq >= 0 && seq < N && cy >= 0 && cx >= 0 && (long long)cy + ch <= H && (long long)cx + cw <= W;
        const T* frame = (const T*)a.src + ((size_t)(valid ? seq : 0) * Tp + (size_t)f * a.step) * ((size_t)H * W * a.Cs);   // 64-bit offsets throughout
        return {frame, W, ch, cw, sy, sx, cy, cx, flip, valid, false};
    }
};

// Windows of long clips: src holds every clip of a split back to back, clip c being frames clip_first[c] .. clip_first[c + 1] - 1;
// a table row is (clip, start frame within the clip, crop y0, crop x0, flip bits, 0) and output frame f of sample b is stored frame
// clip_first[clip] + start + f * step. Everything after the frame pointer is fr_group(), so the pixels are those of the locator above.
struct ClipSource {
    static constexpr bool PER_SAMPLE = false;
    const long long* clip_first;       // [n_clips + 1], on the device; the last entry is the number of frames in src
    const int* table;                  // [B][6]
    long long n_clips, total;          // total: frames in src
    int H, W, ch, cw;
    float sy, sx;                      // float(ch) / float(oh), float(cw) / float(ow)

    template <typename T> __device__ __forceinline__ FrSample<T> locate(const FramesArgs& a, int b, int f) const {
        const int* row = table + (size_t)b * 6;
        const long long clip = row[0], start = row[1];
        const int cy = row[2], cx = row[3], flip = row[4];
        // as above: a row (or an offset table) the caller did not check yields zeros and reads nothing outside src
        bool valid = clip >= 0 && clip < n_clips && start >= 0 && cy >= 0 && cx >= 0 && (long long)cy + ch <= H && (long long)cx + cw <= W;
        long long first = 0;
        if (valid) {
            first = clip_first[clip];
            const long long end = clip_first[clip + 1];
            valid = first >= 0 && end <= total && first + start + (long long)(a.F - 1) * a.step < end;
        }
        const T* frame = (const T*)a.src + (size_t)(valid ? first + start + (long long)f * a.step : 0) * ((size_t)H * W * a.Cs);   // 64-bit offsets throughout
        return {frame, W, ch, cw, sy, sx, cy, cx, flip, valid, false};
    }
};

// Windows of clips whose frame sizes differ: src is ONE element buffer holding every clip back to back and clip_geom [n_clips][4] =
// (element offset of the clip's first frame, frame count, H_i, W_i) says where each lies. A table row is (clip, start frame, box y0,
// box x0, box h, box w, flip bits, 0): the box of stored frame start + f * step goes to oh x ow through fr_group(), with the sample's row
// stride, box and scales where the locators above hand over the launch's. A box of the output's size takes the path without resize, so
// equal shapes give the bits of ClipSource; the choice is per sample (uniform over a sample's threads).
struct VarClipSource {
    static constexpr bool PER_SAMPLE = true;
    const long long* geom;             // [n_clips][4], on the device
    const int* table;                  // [B][8]
    long long n_clips, total;          // total: elements in src

    template <typename T> __device__ __forceinline__ FrSample<T> locate(const FramesArgs& a, int b, int f) const {
        const int* row = table + (size_t)b * 8;
        const long long clip = row[0], start = row[1];
        const int cy = row[2], cx = row[3], bh = row[4], bw = row[5], flip = row[6];
        // as above: a row (or a geometry table) the caller did not check yields zeros and reads nothing outside src
        bool valid = clip >= 0 && clip < n_clips && start >= 0 && cy >= 0 && cx >= 0 && bh >= 1 && bw >= 1;
        long long first = 0, frame_elems = 0;
        int W = 1;
        if (valid) {
            const long long* g = geom + (size_t)clip * 4;
            const long long count = g[1], H = g[2], Wl = g[3];
            first = g[0];
            valid = first >= 0 && first <= total && count >= 1 && H >= 1 && Wl >= 1 && H <= FR_MAX_SIDE && Wl <= FR_MAX_SIDE &&
                    (long long)cy + bh <= H && (long long)cx + bw <= Wl && start + (long long)(a.F - 1) * a.step < count;
            if (valid) {
                frame_elems = H * Wl * a.Cs;                                                          // <= 2^32: no overflow
                valid = count <= (total - first) / frame_elems;                                       // the whole clip lies inside src
                W = (int)Wl;
            }
        }
        const T* frame = (const T*)a.src + (size_t)(valid ? first + (start + (long long)f * a.step) * frame_elems : 0);   // 64-bit offsets throughout
        const bool resize = valid && (bh != a.oh || bw != a.ow);
        return {frame, W, bh, bw, resize ? (float)bh / (float)a.oh : 1.0f, resize ? (float)bw / (float)a.ow : 1.0f, cy, cx, flip, valid, resize};
    }
};

// thread = (sample b, frame f, output row y, group of four output pixels). RESIZE = 0: crop size == output size; 1: bilinear resize;
// FR_PER_SAMPLE: the locator says which, sample by sample.
constexpr int FR_PER_SAMPLE = 2;

template <typename T, typename Source, int RESIZE>
__global__ __launch_bounds__(FR_THREADS) void frames_gather_kernel(FramesArgs a, Source s) {
    const long long item = (long long)blockIdx.x * FR_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const int q = (int)(item % a.Q);
    long long r = item / a.Q;
    const int y = (int)(r % a.oh);
    r /= a.oh;
    const int f = (int)(r % a.F);
    const int b = (int)(r / a.F);
    const FrSample<T> p = s.template locate<T>(a, b, f);
    if (RESIZE == FR_PER_SAMPLE ? p.resize : RESIZE != 0)
        fr_group<T, 1>(a, p.frame, p.valid, p.W, p.ch, p.cw, p.sy, p.sx, p.cy, p.cx, p.flip, b, f, y, q << 2);
    else
        fr_group<T, 0>(a, p.frame, p.valid, p.W, p.ch, p.cw, p.sy, p.sx, p.cy, p.cx, p.flip, b, f, y, q << 2);
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
    const int* table;                  // [B][8], the table of VarClipSource: columns 0 (clip) and 1 (start frame) are all that is read
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

static unsigned fr_blocks(long long items) { return (unsigned)((items + FR_THREADS - 1) / FR_THREADS); }

// RESIZE of frames_gather_kernel for one element type: the launch's `resize` (crop size != output size), or the locator's own choice.
template <typename T, typename Source>
static void launch_gather(const FramesArgs& a, const Source& s, bool resize, hipStream_t stream) {
    const dim3 grid(fr_blocks(a.items)), block(FR_THREADS);
    if constexpr (Source::PER_SAMPLE) VPX_LAUNCH((frames_gather_kernel<T, Source, FR_PER_SAMPLE>), grid, block, 0, stream, a, s);
    else if (resize) VPX_LAUNCH((frames_gather_kernel<T, Source, 1>), grid, block, 0, stream, a, s);
    else VPX_LAUNCH((frames_gather_kernel<T, Source, 0>), grid, block, 0, stream, a, s);
}

// The launch of every frame gather, its arguments checked by the entry point: what fr_group() reads, then the element type by RESIZE
// dispatch over the locator `s`.
template <typename Source>
static int gather_frames(const void* src, int dtype, int Cs, const Source& s, int B, int n_frames, int seq_step, bool resize, int oh, int ow, int C_out,
                         double lo, double hi, float* out, void* stream) {
    FramesArgs a;
    a.src = src; a.out = out;
    a.Cs = Cs; a.F = n_frames; a.step = seq_step; a.oh = oh; a.ow = ow; a.Cout = C_out; a.Q = (ow + 3) / 4;
    a.items = (long long)B * n_frames * oh * a.Q;
    a.vec = (ow % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    a.scaled = (lo != 0.0 || hi != 1.0) ? 1 : 0;
    a.scale = (float)(hi - lo);
    a.lo = (float)lo;
    if (dtype == VPX_FRAMES_U8) launch_gather<unsigned char>(a, s, resize, (hipStream_t)stream);
    else if (dtype == VPX_FRAMES_U16) launch_gather<unsigned short>(a, s, resize, (hipStream_t)stream);
    else launch_gather<float>(a, s, resize, (hipStream_t)stream);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

// ---- the refusals several entry points share, once: VPX_OK, or the code after set_error() ----
#define FR_TRY(check) do { const int rc__ = (check); if (rc__ != VPX_OK) return rc__; } while (0)

static int check_dtype(const char* who, int dtype, bool known, const char* stored) {
    if (!known) { set_error("%s: unknown element type %d (%s are stored)", who, dtype, stored); return VPX_ERR_ARG; }
    return VPX_OK;
}
static int check_frame_dtype(const char* who, int dtype) { return check_dtype(who, dtype, dtype == VPX_FRAMES_U8 || dtype == VPX_FRAMES_U16 || dtype == VPX_FRAMES_F32, "uint8, uint16 and float32"); }
static int check_action_dtype(const char* who, int dtype) { return check_dtype(who, dtype, dtype == VPX_ACTIONS_F32 || dtype == VPX_ACTIONS_F64, "float32 and float64"); }
static int check_counts(const char* who, int B, int n_frames, int seq_step) {
    if (B < 1 || n_frames < 1 || seq_step < 1) { set_error("%s: B, n_frames and seq_step must be >= 1 (got %d, %d, %d)", who, B, n_frames, seq_step); return VPX_ERR_ARG; }
    return VPX_OK;
}
static int check_clips_in_frames(const char* who, long long n_clips, long long total_frames, int n_frames, int seq_step) {
    if (n_clips > total_frames) { set_error("%s: %lld clips in %lld stored frames (a clip holds at least one)", who, n_clips, total_frames); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step >= total_frames) { set_error("%s: frame %d at step %d lies past the %lld stored frames", who, n_frames - 1, seq_step, total_frames); return VPX_ERR_ARG; }
    return VPX_OK;
}
static int check_value_range(const char* who, double lo, double hi) {
    if (hi == lo) { set_error("%s: empty value range [%g, %g]", who, lo, hi); return VPX_ERR_ARG; }
    return VPX_OK;
}
// one thread per item, FR_THREADS per block: the block count must fit a grid's 31 bits (the product in double: it may pass 2^63)
static bool fits_one_launch(double items) { return items / FR_THREADS + 1.0 <= 2147483647.0; }
static int check_rows_launch(const char* who, int B, int rows, int A) {
    if (!fits_one_launch((double)B * rows * A)) { set_error("%s: %d samples of %d rows of %d exceed one launch", who, B, rows, A); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}
static int check_crop_sizes(const char* who, int ch, int cw, int oh, int ow) {
    if (ch < 1 || cw < 1 || oh < 1 || ow < 1) { set_error("%s: crop and output sizes must be >= 1 (got crop %dx%d, output %dx%d)", who, ch, cw, oh, ow); return VPX_ERR_ARG; }
    return VPX_OK;
}
static int check_value_map(const char* who, int Cs, int C_out, double lo, double hi) {
    if (C_out != Cs && !(Cs == 1 && C_out == 3)) { set_error("%s: %d output channels from %d stored ones (equal, or 3 from 1)", who, C_out, Cs); return VPX_ERR_ARG; }
    FR_TRY(check_value_range(who, lo, hi));
    if (Cs > FR_MAX_CS) { set_error("%s: %d stored channels exceed the kernel's %d", who, Cs, FR_MAX_CS); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}
static int check_frames_launch(const char* who, int B, int n_frames, int oh, int ow) {
    if (!fits_one_launch((double)B * n_frames * oh * ((ow + 3) / 4))) { set_error("%s: %d samples of %d %dx%d frames exceed one launch", who, B, n_frames, oh, ow); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}
// a launch with one crop box (sequences, clips back to back): the box inside the frame, the value map, the sides, the launch size
static int check_boxed_gather(const char* who, int H, int W, int Cs, int B, int n_frames, int ch, int cw, int oh, int ow, int C_out, double lo, double hi) {
    if (ch > H || cw > W) { set_error("%s: the %dx%d crop box lies outside the %dx%d frame (there is no padding)", who, ch, cw, H, W); return VPX_ERR_ARG; }
    FR_TRY(check_value_map(who, Cs, C_out, lo, hi));
    if (H > FR_MAX_SIDE || W > FR_MAX_SIDE || oh > FR_MAX_SIDE || ow > FR_MAX_SIDE) { set_error("%s: a side beyond %d (frame %dx%d, output %dx%d)", who, FR_MAX_SIDE, H, W, oh, ow); return VPX_ERR_UNSUPPORTED; }
    return check_frames_launch(who, B, n_frames, oh, ow);
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_frames_preprocess(const void* src, int dtype, long long N, int Tp, int H, int W, int Cs, const int* table, int B, int n_frames,
                          int seq_step, int ch, int cw, int oh, int ow, int C_out, double lo, double hi, float* out, void* stream) {
    const char* who = "vpx_frames_preprocess";
    if (!src || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    FR_TRY(check_frame_dtype(who, dtype));
    if (N < 1 || Tp < 1 || H < 1 || W < 1 || Cs < 1) { set_error("%s: every source size must be >= 1 (got N=%lld T'=%d H=%d W=%d Cs=%d)", who, N, Tp, H, W, Cs); return VPX_ERR_ARG; }
    FR_TRY(check_counts(who, B, n_frames, seq_step));
    FR_TRY(check_crop_sizes(who, ch, cw, oh, ow));
    if ((long long)(n_frames - 1) * seq_step >= Tp) { set_error("%s: frame %d at step %d lies past the %d stored frames", who, n_frames - 1, seq_step, Tp); return VPX_ERR_ARG; }
    FR_TRY(check_boxed_gather(who, H, W, Cs, B, n_frames, ch, cw, oh, ow, C_out, lo, hi));
    const SeqSource s{table, N, Tp, H, W, ch, cw, (float)ch / (float)oh, (float)cw / (float)ow};
    return gather_frames(src, dtype, Cs, s, B, n_frames, seq_step, ch != oh || cw != ow, oh, ow, C_out, lo, hi, out, stream);
}

int vpx_clips_preprocess(const void* src, int dtype, long long total_frames, int H, int W, int Cs, const long long* clip_first, long long n_clips,
                         const int* table, int B, int n_frames, int seq_step, int ch, int cw, int oh, int ow, int C_out, double lo, double hi,
                         float* out, void* stream) {
    const char* who = "vpx_clips_preprocess";
    if (!src || !clip_first || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    FR_TRY(check_frame_dtype(who, dtype));
    if (total_frames < 1 || n_clips < 1 || H < 1 || W < 1 || Cs < 1) { set_error("%s: every source size must be >= 1 (got frames=%lld clips=%lld H=%d W=%d Cs=%d)", who, total_frames, n_clips, H, W, Cs); return VPX_ERR_ARG; }
    FR_TRY(check_counts(who, B, n_frames, seq_step));
    FR_TRY(check_crop_sizes(who, ch, cw, oh, ow));
    FR_TRY(check_clips_in_frames(who, n_clips, total_frames, n_frames, seq_step));
    FR_TRY(check_boxed_gather(who, H, W, Cs, B, n_frames, ch, cw, oh, ow, C_out, lo, hi));
    const ClipSource s{clip_first, table, n_clips, total_frames, H, W, ch, cw, (float)ch / (float)oh, (float)cw / (float)ow};
    return gather_frames(src, dtype, Cs, s, B, n_frames, seq_step, ch != oh || cw != ow, oh, ow, C_out, lo, hi, out, stream);
}

int vpx_clips_preprocess_var(const void* src, int dtype, long long total_elems, int Cs, const long long* clip_geom, long long n_clips, const int* table,
                             int B, int n_frames, int seq_step, int oh, int ow, int C_out, double lo, double hi, float* out, void* stream) {
    const char* who = "vpx_clips_preprocess_var";
    if (!src || !clip_geom || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    FR_TRY(check_frame_dtype(who, dtype));
    if (total_elems < 1 || n_clips < 1 || Cs < 1) { set_error("%s: every source size must be >= 1 (got elements=%lld clips=%lld Cs=%d)", who, total_elems, n_clips, Cs); return VPX_ERR_ARG; }
    FR_TRY(check_counts(who, B, n_frames, seq_step));
    if (oh < 1 || ow < 1) { set_error("%s: output sizes must be >= 1 (got output %dx%d)", who, oh, ow); return VPX_ERR_ARG; }
    if (n_clips > total_elems / Cs) { set_error("%s: %lld clips in %lld stored elements of %d channels (a clip holds at least one frame of one pixel)", who, n_clips, total_elems, Cs); return VPX_ERR_ARG; }
    if ((long long)(n_frames - 1) * seq_step >= total_elems / Cs) { set_error("%s: frame %d at step %d lies past the %lld stored elements", who, n_frames - 1, seq_step, total_elems); return VPX_ERR_ARG; }
    FR_TRY(check_value_map(who, Cs, C_out, lo, hi));
    if (oh > FR_MAX_SIDE || ow > FR_MAX_SIDE) { set_error("%s: a side beyond %d (output %dx%d)", who, FR_MAX_SIDE, oh, ow); return VPX_ERR_UNSUPPORTED; }
    FR_TRY(check_frames_launch(who, B, n_frames, oh, ow));
    const VarClipSource s{clip_geom, table, n_clips, total_elems};   // frame and box sizes come per sample, and with them the choice to resize (not the launch's `false`)
    return gather_frames(src, dtype, Cs, s, B, n_frames, seq_step, false, oh, ow, C_out, lo, hi, out, stream);
}

int vpx_actions_diff_gather(const void* src, int dtype, long long total_frames, int A, const long long* clip_first, long long n_clips, const int* table,
                            int B, int n_frames, int seq_step, float* out, void* stream) {
    const char* who = "vpx_actions_diff_gather";
    if (!src || !clip_first || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    FR_TRY(check_action_dtype(who, dtype));
    if (total_frames < 1 || n_clips < 1 || A < 1) { set_error("%s: every source size must be >= 1 (got frames=%lld clips=%lld A=%d)", who, total_frames, n_clips, A); return VPX_ERR_ARG; }
    FR_TRY(check_counts(who, B, n_frames, seq_step));
    if (n_frames < 2) { set_error("%s: a difference needs two frames (n_frames = %d)", who, n_frames); return VPX_ERR_ARG; }
    FR_TRY(check_clips_in_frames(who, n_clips, total_frames, n_frames, seq_step));
    FR_TRY(check_rows_launch(who, B, n_frames - 1, A));
    ActionsDiffArgs a;
    a.src = src; a.clip_first = clip_first; a.table = table; a.out = out;
    a.n_clips = n_clips; a.total = total_frames; a.A = A; a.F = n_frames; a.step = seq_step;
    a.items = (long long)B * (n_frames - 1) * A;
    const dim3 grid(fr_blocks(a.items)), block(FR_THREADS);
    if (dtype == VPX_ACTIONS_F32) VPX_LAUNCH(actions_diff_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
    else VPX_LAUNCH(actions_diff_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_frames_postprocess(const float* x, long long N, int C, int h, int w, double lo, double hi, unsigned char* out, void* stream) {
    const char* who = "vpx_frames_postprocess";
    if (!x || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (N < 1 || C < 1 || h < 1 || w < 1) { set_error("%s: every size must be >= 1 (got N=%lld C=%d h=%d w=%d)", who, N, C, h, w); return VPX_ERR_ARG; }
    FR_TRY(check_value_range(who, lo, hi));
    if (h > FR_MAX_SIDE || w > FR_MAX_SIDE) { set_error("%s: a side beyond %d (%dx%d)", who, FR_MAX_SIDE, h, w); return VPX_ERR_UNSUPPORTED; }
    const int Q = (w + 3) / 4;
    if (!fits_one_launch((double)N * h * Q)) { set_error("%s: %lld images of %dx%d exceed one launch", who, N, h, w); return VPX_ERR_UNSUPPORTED; }
    PostArgs a;
    a.x = x; a.out = out; a.C = C; a.h = h; a.w = w; a.Q = Q;
    a.items = N * h * Q;
    a.vec = (w % 4 == 0 && C <= 4 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
    a.scale = (float)(hi - lo);
    a.lo = (float)lo;
    VPX_LAUNCH(frames_postprocess_kernel, dim3(fr_blocks(a.items)), dim3(FR_THREADS), 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_actions_gather(const void* src, int dtype, long long N, int Tp, int A, const int* table, int B, int n_frames, int seq_step,
                       float* out, void* stream) {
    const char* who = "vpx_actions_gather";
    if (!src || !table || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    FR_TRY(check_action_dtype(who, dtype));
    if (N < 1 || Tp < 1 || A < 1) { set_error("%s: every source size must be >= 1 (got N=%lld T'=%d A=%d)", who, N, Tp, A); return VPX_ERR_ARG; }
    FR_TRY(check_counts(who, B, n_frames, seq_step));
    if ((long long)(n_frames - 1) * seq_step + 1 > Tp) { set_error("%s: frame %d at step %d lies past the %d stored frames", who, n_frames - 1, seq_step, Tp); return VPX_ERR_ARG; }
    FR_TRY(check_rows_launch(who, B, n_frames, A));
    ActionsArgs a;
    a.src = src; a.table = table; a.out = out;
    a.N = N; a.Tp = Tp; a.A = A; a.F = n_frames; a.step = seq_step;
    a.items = (long long)B * n_frames * A;
    const dim3 grid(fr_blocks(a.items)), block(FR_THREADS);
    if (dtype == VPX_ACTIONS_F32) VPX_LAUNCH(actions_gather_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
    else VPX_LAUNCH(actions_gather_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
