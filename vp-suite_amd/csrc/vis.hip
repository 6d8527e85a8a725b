// Prediction visualizations (vp_suite/utils/visualization.py: add_borders + the side-by-side concatenation of save_vid_vis, and the sheet of
// save_frame_compare_img), one launch per canvas:
//   vpx_vis_compose     src float32 [S][T][C][h][w] (planar, only read, C = 1 or 3) and a device table int32 [n_tiles][8] =
//                       (s, t, f, y0, x0, b, colour 0xRRGGBB, 0) -> canvas uint8 [F][Hc][Wc][3]
// A tile paints the (h + 2b) x (w + 2b) rectangle at (y0, x0) of canvas frame f: the outer ring of width b in the colour, the inner h x w
// with frame (s, t) as bytes — fr_byte of frames_byte.h, the device function of vpx_frames_postprocess, so the inner rectangle IS
// postprocess(src[s][t]); a one-channel source goes to all three channels. Bytes no tile covers hold the background: one asynchronous fill
// of the canvas before the launch, skipped when the caller says the tiles cover it (background < 0).
//
// Streaming kernel, no LDS, no atomics, no workspace. A tile row is 3 * (w + 2b) bytes that start at any byte of the canvas, so the unit of
// work is one 4-byte-ALIGNED word of canvas memory that a tile row overlaps (alignment taken on the address itself, whatever the canvas
// pointer is): neighbouring lanes own neighbouring words, a word that lies inside the row leaves as one 32-bit store, and the one or two
// words a row shares with its neighbours (another tile, the background) leave as single byte stores of this row's bytes only — nothing is
// read back, nothing outside a tile's rectangle is written. Each byte costs one float load of its plane. item = (tile, row, word) over the
// largest tile the table may hold (b <= max_border); the grid is capped and strides.
//
// The table lives on the device, so the CALLER checks it (ops.check_vis_tiles). A row the kernel cannot run — s, t or f out of range, b
// outside [0, max_border], a rectangle that leaves the canvas — is skipped as a whole: nothing of it is read, nothing written. Two tiles
// of one canvas frame that overlap are in bounds, and which of them a shared byte shows is not defined. Offsets are 64-bit.
#include <hip/hip_runtime.h>
#include "vpx_internal.h"
#include "vpx_host.h"

// Every operation of this file is rounded on its own (see frames.hip): no a * b + c becomes a fused multiply-add.
#pragma clang fp contract(off)

#include "frames_byte.h"

namespace vpx {

constexpr int VIS_THREADS = 256;
constexpr int VIS_MAX_BLOCKS = 2048;     // 256 CUs x 8 workgroups: a larger canvas is walked in strides of the grid
constexpr int VIS_MAX_SIDE = 32768;      // frame and canvas sides (as in frames.hip)
constexpr int VIS_ROW = 8;               // table columns

struct VisArgs {
    const float* src;                    // [S][T][C][h][w]
    const int* tiles;                    // [n_tiles][8] = (s, t, f, y0, x0, b, colour, 0)
    unsigned char* canvas;               // [F][Hc][Wc][3]
    long long items;                     // n_tiles * R * NW
    int S, T, C, h, w, F, Hc, Wc;
    int bmax;                            // the largest border the table may hold
    int R, NW;                           // rows and aligned words per row of the largest tile: h + 2 bmax, (3 (w + 2 bmax) + 6) / 4
    float scale, lo;                     // float(hi - lo), float(lo)
};

__global__ __launch_bounds__(VIS_THREADS) void vis_compose_kernel(VisArgs a) {
    const long long stride = (long long)gridDim.x * VIS_THREADS;
    for (long long item = (long long)blockIdx.x * VIS_THREADS + threadIdx.x; item < a.items; item += stride) {
        const int k = (int)(item % a.NW);
        const long long q = item / a.NW;
        const int r = (int)(q % a.R);
        const int* row = a.tiles + (q / a.R) * VIS_ROW;
        const int s = row[0], t = row[1], f = row[2], y0 = row[3], x0 = row[4], b = row[5];
        const unsigned colour = (unsigned)row[6];
        if (s < 0 || s >= a.S || t < 0 || t >= a.T || f < 0 || f >= a.F || b < 0 || b > a.bmax || y0 < 0 || x0 < 0) continue;
        const int th = a.h + 2 * b, tw = a.w + 2 * b;                          // (b <= bmax <= 32768: no overflow)
        if ((long long)y0 + th > a.Hc || (long long)x0 + tw > a.Wc) continue;   // the rectangle leaves the canvas: the whole row is skipped
        if (r >= th) continue;
        const int L = 3 * tw;                                                  // bytes of this tile row
        unsigned char* seg = a.canvas + (((size_t)f * a.Hc + (size_t)(y0 + r)) * a.Wc + (size_t)x0) * 3;
        const int head = (int)((uintptr_t)seg & 3);                            // bytes of the first aligned word that lie before the row
        const int p0 = 4 * k - head;                                           // row byte of this word's byte 0 (negative in the first word)
        if (p0 >= L) continue;
        const bool ring_row = r < b || r >= b + a.h;
        const size_t plane = (size_t)a.h * a.w;
        const float* frame = a.src + ((size_t)s * a.T + (size_t)t) * a.C * plane + (ring_row ? (size_t)0 : (size_t)(r - b) * a.w);
        unsigned word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = p0 + j;
            if (p < 0 || p >= L) continue;
            const int px = p / 3, c = p - 3 * px;
            unsigned v;
            if (ring_row || px < b || px >= b + a.w) v = (colour >> (8 * (2 - c))) & 0xffu;   // 0xRRGGBB: red is channel 0
            else v = fr_byte(a.lo, a.scale, frame[(a.C == 3 ? (size_t)c * plane : (size_t)0) + (size_t)(px - b)]);
            word |= v << (8 * j);                                              // little endian: byte j of the word
        }
        if (p0 >= 0 && p0 + 4 <= L) {
            *reinterpret_cast<unsigned*>(seg + p0) = word;                     // seg + p0 is 4-byte aligned by construction
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j >= 0 && p0 + j < L) seg[p0 + j] = (unsigned char)(word >> (8 * j));
        }
    }
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_vis_compose(const float* src, int S, int T, int C, int h, int w, double lo, double hi, const int* tiles, int n_tiles, int max_border,
                    unsigned char* canvas, int F, int Hc, int Wc, int background, void* stream) {
    const char* who = "vpx_vis_compose";
    if (!src || !tiles || !canvas) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (C != 1 && C != 3) { set_error("%s: %d source channels (1 and 3 are drawn)", who, C); return VPX_ERR_ARG; }
    if (!(hi > lo) || !((float)(hi - lo) > 0.0f)) { set_error("%s: empty value range [%g, %g] (hi must exceed lo)", who, lo, hi); return VPX_ERR_ARG; }
    if (n_tiles < 0 || max_border < 0) { set_error("%s: n_tiles and max_border must be >= 0 (got %d, %d)", who, n_tiles, max_border); return VPX_ERR_ARG; }
    if (background < -1 || background > 255) { set_error("%s: background %d is neither a grey level 0 ... 255 nor -1 (no fill)", who, background); return VPX_ERR_ARG; }
    if (n_tiles > 0 && (S < 1 || T < 1 || h < 1 || w < 1 || F < 1 || Hc < 1 || Wc < 1)) {
        set_error("%s: every size must be >= 1 (got S=%d T=%d h=%d w=%d, canvas F=%d %dx%d)", who, S, T, h, w, F, Hc, Wc);
        return VPX_ERR_ARG;
    }
    if (h > VIS_MAX_SIDE || w > VIS_MAX_SIDE || Hc > VIS_MAX_SIDE || Wc > VIS_MAX_SIDE || max_border > VIS_MAX_SIDE) {
        set_error("%s: a side or border beyond %d (frame %dx%d, border %d, canvas %dx%d)", who, VIS_MAX_SIDE, h, w, max_border, Hc, Wc);
        return VPX_ERR_UNSUPPORTED;
    }
    const bool canvas_empty = F < 1 || Hc < 1 || Wc < 1;
    VisArgs a;
    a.src = src; a.tiles = tiles; a.canvas = canvas;
    a.S = S; a.T = T; a.C = C; a.h = h; a.w = w; a.F = F; a.Hc = Hc; a.Wc = Wc; a.bmax = max_border;
    a.R = h + 2 * max_border;
    a.NW = (3 * (w + 2 * max_border) + 6) / 4;      // aligned words a row of 3 (w + 2b) bytes can overlap, wherever it starts
    const double items_d = (double)n_tiles * a.R * a.NW;
    if (items_d > 4.0e18 || (double)F * Hc * Wc * 3.0 > 4.0e18) { set_error("%s: %d tiles of up to %dx%d words exceed one launch", who, n_tiles, a.R, a.NW); return VPX_ERR_UNSUPPORTED; }
    a.items = (long long)n_tiles * a.R * a.NW;
    a.scale = (float)(hi - lo);
    a.lo = (float)lo;
    if (background >= 0 && !canvas_empty) VPX_CHECK_HIP(vpx_memset_async(canvas, background, (size_t)F * Hc * Wc * 3, (hipStream_t)stream));
    if (a.items > 0) {
        const long long need = (a.items + VIS_THREADS - 1) / VIS_THREADS;
        const unsigned blocks = (unsigned)(need < VIS_MAX_BLOCKS ? need : VIS_MAX_BLOCKS);
        VPX_LAUNCH(vis_compose_kernel, dim3(blocks), dim3(VIS_THREADS), 0, (hipStream_t)stream, a);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

}  // extern "C"
