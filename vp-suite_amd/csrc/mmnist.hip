// Moving MNIST generated on the device (vp_suite/datasets/mmnist_on_the_fly.py:78-104, 133-147): one launch writes a whole
// [B, F, C, S, S] batch from a table of glyphs and one row of five integers per sample and digit.
//   vpx_mmnist_frames   D glyphs of s x s bytes per sample move over an S x S canvas, bounce off its walls, are summed and clipped
// A gather: every thread owns output pixels and tests the D glyph boxes of its frame, so there is no atomic, no ordering between
// workgroups, and the sum over the digits runs in digit order in every pixel — the result is the same in every mode, bit for bit.
//
// Bit-exact contract (the reference computes in float64 and converts once; tests/mmnist_ref.py restates it):
//   a = 0.0;  a += double(g) / 255.0 for each digit, in order, whose box holds the pixel;  a = min(max(a, 0), 1);
//   a = a * 255.0 / 255.0 (two operations: the reference's `frames * 255`, then preprocess()'s `/ 255`);  x = float(a);
//   only if (lo, hi) != (0, 1):  x = x * float(hi - lo), then x = x + float(lo) — two fp32 roundings, never a fused multiply-add (the pragma below).
// double(g) / 255.0 has 256 possible values: the workgroup's 256 threads divide once each into an LDS table.
#include <hip/hip_runtime.h>
#include "vpx_internal.h"
#include "vpx_host.h"

// Every operation of this file is rounded on its own: HIP contracts a * b + c into one fused multiply-add by default, and its
// __fmul_rn / __fadd_rn are the plain operators, which the contraction sees through.
#pragma clang fp contract(off)

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MM_THREADS = 256;       // = entries of the value table: one division per thread
constexpr int MM_FRAMES = 2;          // frames of one sample per workgroup
constexpr int MM_MAX_DIGITS = 16;     // glyphs per sample (the positions of a frame chunk live in LDS)
constexpr int MM_MAX_GLYPH_BYTES = 48 * 1024;   // D * s * s: the sample's glyphs live in LDS too (MNIST's 28 x 28: 784 bytes each)
constexpr int MM_MAX_SIDE = 16384;    // canvas side: a workgroup's pixel-group count stays far below 2^31
constexpr int MM_MAX_FRAMES = 65536;  // frames per sample: every workgroup walks the rule from the start of the sequence

struct MMArgs {
    const unsigned char* digits;   // [N][s][s]
    const int* params;             // [B][D][5] = (glyph index, y0, x0, vy, vx)
    float* out;                    // [B][F][C][S][S]
    int N, s, B, D, F, C, S;
    int chunks;                    // ceil(F / MM_FRAMES)
    int vec;                       // 1: S % 4 == 0 and `out` 16-byte aligned — every group of four pixels is one 16-byte store
    int scaled;                    // 1: (lo, hi) != (0, 1)
    float scale, lo;               // float(hi - lo), float(lo)
};

// one move of one axis (mmnist_on_the_fly.py:137-146): past the far wall -> exactly on it, past 0 -> mirrored; either turns the speed round
__device__ __forceinline__ void mm_move(long long& p, long long& v, int S, int s) {
    p += v;
    if (p + s > S) { p = S - s; v = -v; }
    else if (p < 0) { p = -p; v = -v; }
}

// workgroup (sample b, chunk of MM_FRAMES frames). Lanes 0 .. 2D-1 walk one (digit, axis) each from the start of the sequence — frame i
// shows the position after i + 1 moves — and leave the chunk's positions in LDS; nobody walks the rule per pixel. The sample's D glyphs
// are copied to LDS once, so the pixel loop waits for no global load: its only traffic is the store stream.
__global__ __launch_bounds__(MM_THREADS) void mmnist_frames_kernel(MMArgs a) {
    extern __shared__ unsigned char glyphs[];                  // [D][s][s]: this sample's glyphs; zeros for an index outside [0, N)
    __shared__ double lut[256];                                // double(g) / 255.0
    __shared__ int pos[MM_FRAMES][MM_MAX_DIGITS][2];           // (y, x) of the glyph's corner
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.chunks;
    const int f0 = (blockIdx.x % a.chunks) * MM_FRAMES;
    const int nf = a.F - f0 < MM_FRAMES ? a.F - f0 : MM_FRAMES;
    const int* rows = a.params + (size_t)b * a.D * 5;
    lut[tid] = (double)tid / 255.0;
    if (tid < 2 * a.D) {
        const int d = tid >> 1, axis = tid & 1;                // axis 0 = y
        long long p = rows[d * 5 + 1 + axis], v = rows[d * 5 + 3 + axis];   // (64-bit: no table, however wrong, overflows the walk)
        for (int i = 0; i < f0 + nf; ++i) {
            mm_move(p, v, a.S, a.s);
            if (i >= f0) pos[i - f0][d][axis] = (int)(p < -a.s ? -a.s : (p > a.S ? a.S : p));   // (clamped positions are off the canvas)
        }
    }
    const int ss = a.s * a.s;
    for (int i = tid; i < a.D * ss; i += MM_THREADS) {
        const int d = i / ss, index = rows[d * 5];
        glyphs[i] = (index >= 0 && index < a.N) ? a.digits[(size_t)index * ss + (i - d * ss)] : 0;
    }
    __syncthreads();

    const int Q = (a.S + 3) >> 2;                              // groups of four pixels per row (the last one partial if S % 4)
    const int per_frame = a.S * Q;
    const size_t plane = (size_t)a.S * a.S;
    for (int f = 0; f < nf; ++f) {
        float* frame = a.out + ((size_t)b * a.F + f0 + f) * a.C * plane;
        for (int r = tid; r < per_frame; r += MM_THREADS) {
            const int y = r / Q, x0 = (r - y * Q) << 2;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int d = 0; d < a.D; ++d) {
                const int dy = y - pos[f][d][0], dx0 = x0 - pos[f][d][1];
                if (dy < 0 || dy >= a.s || dx0 <= -4 || dx0 >= a.s) continue;
                const unsigned char* g = glyphs + (d * a.s + dy) * a.s;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int dx = dx0 + k;
                    if (dx >= 0 && dx < a.s) acc[k] += lut[g[dx]];
                }
            }
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double v = acc[k];
                if (v != 0.0) {                                // (0 * 255 / 255 is 0: the background skips the division)
                    v = fmin(fmax(v, 0.0), 1.0);
                    v = v * 255.0;
                    v = v / 255.0;
                }
                float x = (float)v;
                if (a.scaled) {
                    x = x * a.scale;
                    x = x + a.lo;
                }
                o[k] = x;
            }
            float* dst = frame + (size_t)y * a.S + x0;
            for (int c = 0; c < a.C; ++c, dst += plane) {      // every channel carries the same value
                if (a.vec) *reinterpret_cast<f32x4*>(dst) = o;
                else
                    for (int k = 0; k < 4 && x0 + k < a.S; ++k) dst[k] = o[k];
            }
        }
    }
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_mmnist_frames(const unsigned char* digits, int n_glyphs, int glyph_size, const int* params, int B, int D, int n_frames, int C, int S,
                      double lo, double hi, float* out, void* stream) {
    const char* who = "vpx_mmnist_frames";
    if (!digits || !params || !out) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (B < 1 || n_frames < 1 || n_glyphs < 1 || glyph_size < 1) { set_error("%s: B, n_frames, n_glyphs and glyph_size must be >= 1 (got %d, %d, %d, %d)", who, B, n_frames, n_glyphs, glyph_size); return VPX_ERR_ARG; }
    if (D < 1) { set_error("%s: at least one digit per sample (got %d)", who, D); return VPX_ERR_ARG; }
    if (C != 1 && C != 3) { set_error("%s: 1 or 3 channels (got %d)", who, C); return VPX_ERR_ARG; }
    if (glyph_size >= S) { set_error("%s: the %dx%d glyph does not move inside a %dx%d image", who, glyph_size, glyph_size, S, S); return VPX_ERR_ARG; }
    if (D > MM_MAX_DIGITS) { set_error("%s: %d digits per sample exceed the kernel's %d", who, D, MM_MAX_DIGITS); return VPX_ERR_UNSUPPORTED; }
    if ((long long)D * glyph_size * glyph_size > MM_MAX_GLYPH_BYTES) { set_error("%s: %d glyphs of %dx%d bytes exceed the %d bytes of LDS they are staged in", who, D, glyph_size, glyph_size, MM_MAX_GLYPH_BYTES); return VPX_ERR_UNSUPPORTED; }
    if (S > MM_MAX_SIDE) { set_error("%s: image side %d exceeds %d", who, S, MM_MAX_SIDE); return VPX_ERR_UNSUPPORTED; }
    if (n_frames > MM_MAX_FRAMES) { set_error("%s: %d frames per sample exceed %d", who, n_frames, MM_MAX_FRAMES); return VPX_ERR_UNSUPPORTED; }
    const int chunks = (n_frames + MM_FRAMES - 1) / MM_FRAMES;
    if ((long long)B * chunks > 0x7fffffffLL) { set_error("%s: %d samples of %d frames exceed one launch", who, B, n_frames); return VPX_ERR_UNSUPPORTED; }
    MMArgs a;
    a.digits = digits; a.params = params; a.out = out;
    a.N = n_glyphs; a.s = glyph_size; a.B = B; a.D = D; a.F = n_frames; a.C = C; a.S = S;
    a.chunks = chunks;
    a.vec = (S % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
    a.scaled = (lo != 0.0 || hi != 1.0) ? 1 : 0;
    a.scale = (float)(hi - lo);
    a.lo = (float)lo;
    VPX_LAUNCH(mmnist_frames_kernel, dim3((unsigned)(B * chunks)), dim3(MM_THREADS), (unsigned)(D * glyph_size * glyph_size), (hipStream_t)stream, a);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
