// dense.hip — the dense layer and the LSTM cell of the NonConvLSTM model (vp_suite/models/lstm.py: nn.Linear 16384 <-> 1024 and a stack
// of nn.LSTMCell(1024, 1024)). Both are skinny matrix products that stream weights: M = 2 ... 128 rows against 16-67 MB of fp32 weights.
//   * gemm_kernel: out[M][N] = A[M][K] * B, fp32 FMA. A may be two row-major sources side by side along K ([x | h]); B is either the
//     weight as it is stored ([N][K], rows along K: the forward, again two sources [W_ih | W_hh]) or read the other way round ([K][N]:
//     the data gradient dy * w). A workgroup owns one (M tile, N tile, K chunk); three tile forms (8 x 128, 32 x 32, 128 x 32) keep all
//     rows of M <= 128 in ONE workgroup, so a weight element is read from HBM by exactly one workgroup of a launch.
//   * K split: with few tiles (N = 1024: 8 ... 32 of them) the K axis is cut into chunks, one workgroup each, until about two workgroups
//     per CU exist. Partial sums go to the workspace [chunk][M][N] and a second kernel adds them in chunk order: no float atomics, equal
//     bits run to run in every mode.
//   * LSTM cell: the N axis is walked gate-interleaved (column 4 j + g reads weight row g H + j), so the four accumulators of a thread
//     are the gates i, f, g, o of one hidden unit and the gate arithmetic is the epilogue of the launch (single pass) or of the
//     reduction (K split).
//   * weight gradient dw[N][K] (+)= dy^T x: the output is the large side (one 64 x 64 tile per workgroup), the contraction over M runs
//     inside the workgroup in row order. Bias gradient: column sums in row order.
#include "vpx_host.h"

namespace vpx {

constexpr int DN_THREADS = 256;
constexpr int DN_KT = 32;            // K elements staged per round
constexpr int DN_MIN_CHUNK = 256;    // a K chunk is never shorter (below, the reduction costs more than the idle CUs)
constexpr int DN_TARGET_WGS = 512;   // two workgroups per CU
constexpr int DN_MAX_CHUNKS = 64;

struct DensePlan { int form, tm, tn, m_tiles, n_tiles, chunks, chunk_len; };

// The launch of out[M][N] with a contraction of length K: tile form from M, K chunks from the tile count. The one place that decides.
static DensePlan dense_plan_of(long long M, long long N, long long K) {
    DensePlan p{};
    p.form = M <= 8 ? 0 : (M <= 32 ? 1 : 2);
    p.tm = p.form == 0 ? 8 : (p.form == 1 ? 32 : 128);
    p.tn = p.form == 0 ? 128 : 32;
    p.m_tiles = (int)((M + p.tm - 1) / p.tm);
    p.n_tiles = (int)((N + p.tn - 1) / p.tn);
    const long long tiles = (long long)p.m_tiles * p.n_tiles;
    long long want = (DN_TARGET_WGS + tiles - 1) / tiles;
    const long long by_k = K / DN_MIN_CHUNK;
    if (want > by_k) want = by_k;
    if (want > DN_MAX_CHUNKS) want = DN_MAX_CHUNKS;
    if (want < 1) want = 1;
    long long len = (K + want - 1) / want;
    len = (len + DN_KT - 1) / DN_KT * DN_KT;
    p.chunk_len = (int)len;
    p.chunks = (int)((K + len - 1) / len);
    return p;
}

struct GemmArgs {
    const float *a0, *a1;        // A: [M][K0] and [M][K1] side by side along K (a1 == nullptr: K1 = 0)
    long long lda0, lda1;
    const float *b0, *b1;        // B as stored: [N][K0], [N][K1] (row strides ldb0, ldb1); read the other way round: b0 [K][N] alone
    long long ldb0, ldb1;
    int M, N, K0, K1;
    int chunk_len;
    int cell_H;                  // > 0: gate-interleaved columns, N == 4 * cell_H
    float* part;                 // K split: [chunk][M][N] (columns as the launch walks them)
    float* y; long long ldy;     // dense epilogue
    const float *bias0, *bias1;  // (bias1: the cell's second bias)
    int relu;
    const float* c;              // cell epilogue: c [M][H] (nullptr: zero), outputs [M][H], activated gates [M][4H] in torch's order (nullable)
    float *h_new, *c_new, *gates;
};

__device__ __forceinline__ float dn_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// pre: the four pre-activations i, f, g, o of one hidden unit (biases added)
__device__ __forceinline__ void cell_point(const float pre[4], float c_prev, float* h_new, float* c_new, float* gates, long long m, int j, int H) {
    const float i = dn_sigmoid(pre[0]), f = dn_sigmoid(pre[1]), g = tanhf(pre[2]), o = dn_sigmoid(pre[3]);
    const float cn = f * c_prev + i * g;
    c_new[m * H + j] = cn;
    h_new[m * H + j] = o * tanhf(cn);
    if (gates) {
        float* gp = gates + m * 4 * H + j;
        gp[0] = i; gp[H] = f; gp[2 * (long long)H] = g; gp[3 * (long long)H] = o;
    }
}

template <int TGM, int RM, bool NN>
__global__ __launch_bounds__(DN_THREADS) void gemm_kernel(GemmArgs a) {
    constexpr int RN = 4, TGN = DN_THREADS / TGM, TM = TGM * RM, TN = TGN * RN;
    __shared__ float As[DN_KT][TM + 1];
    __shared__ float Bs[DN_KT][TN + 1];
    const int tid = threadIdx.x;
    const int tng = tid % TGN, tmg = tid / TGN;
    const long long m0 = (long long)blockIdx.y * TM;
    const long long n0 = (long long)blockIdx.x * TN;
    const int K = a.K0 + a.K1;
    const int k_begin = blockIdx.z * a.chunk_len;
    const int k_end = k_begin + a.chunk_len < K ? k_begin + a.chunk_len : K;
    float acc[RM][RN];
#pragma unroll
    for (int r = 0; r < RM; ++r)
#pragma unroll
        for (int j = 0; j < RN; ++j) acc[r][j] = 0.f;

    for (int kt = k_begin; kt < k_end; kt += DN_KT) {
        for (int e = tid; e < TM * DN_KT; e += DN_THREADS) {
            const int mm = e / DN_KT, kk = e % DN_KT;
            const long long m = m0 + mm;
            const int k = kt + kk;
            float v = 0.f;
            if (m < a.M && k < k_end) v = k < a.K0 ? a.a0[m * a.lda0 + k] : a.a1[m * a.lda1 + (k - a.K0)];
            As[kk][mm] = v;
        }
        if (NN) {
            for (int e = tid; e < TN * DN_KT; e += DN_THREADS) {
                const int kk = e / TN, nn = e % TN;
                const long long n = n0 + nn;
                const int k = kt + kk;
                Bs[kk][nn] = (n < a.N && k < k_end) ? a.b0[(long long)k * a.ldb0 + n] : 0.f;
            }
        } else {
            for (int e = tid; e < TN * DN_KT; e += DN_THREADS) {
                const int nn = e / DN_KT, kk = e % DN_KT;
                const long long n = n0 + nn;
                const int k = kt + kk;
                float v = 0.f;
                if (n < a.N && k < k_end) {
                    const long long row = a.cell_H > 0 ? (n & 3) * a.cell_H + (n >> 2) : n;
                    v = k < a.K0 ? a.b0[row * a.ldb0 + k] : a.b1[row * a.ldb1 + (k - a.K0)];
                }
                Bs[kk][nn] = v;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < DN_KT; ++kk) {
            float av[RM], bv[RN];
#pragma unroll
            for (int r = 0; r < RM; ++r) av[r] = As[kk][tmg * RM + r];
#pragma unroll
            for (int j = 0; j < RN; ++j) bv[j] = Bs[kk][tng * RN + j];
#pragma unroll
            for (int r = 0; r < RM; ++r)
#pragma unroll
                for (int j = 0; j < RN; ++j) acc[r][j] += av[r] * bv[j];
        }
        __syncthreads();
    }

    const long long nb = n0 + tng * RN;
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        const long long m = m0 + tmg * RM + r;
        if (m >= a.M) continue;
        if (a.part) {
            float* p = a.part + ((long long)blockIdx.z * a.M + m) * a.N;
#pragma unroll
            for (int j = 0; j < RN; ++j) if (nb + j < a.N) p[nb + j] = acc[r][j];
        } else if (a.cell_H > 0) {
            if (nb < a.N) {   // (N == 4 H and nb % 4 == 0: a thread's four columns are one unit's gates)
                const int H = a.cell_H, u = (int)(nb >> 2);
                float pre[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = acc[r][g] + (a.bias0 ? a.bias0[g * H + u] : 0.f) + (a.bias1 ? a.bias1[g * H + u] : 0.f);
                cell_point(pre, a.c ? a.c[m * H + u] : 0.f, a.h_new, a.c_new, a.gates, m, u, H);
            }
        } else {
#pragma unroll
            for (int j = 0; j < RN; ++j) {
                if (nb + j >= a.N) continue;
                float v = acc[r][j] + (a.bias0 ? a.bias0[nb + j] : 0.f);
                if (a.relu) v = v > 0.f ? v : 0.f;
                a.y[m * a.ldy + nb + j] = v;
            }
        }
    }
}

// y[m][n] = act(sum over chunks, in chunk order, of part[chunk][m][n] + bias[n])
__global__ __launch_bounds__(DN_THREADS) void dense_reduce_kernel(const float* __restrict__ part, int chunks, long long M, long long N,
                                                                  const float* __restrict__ bias, int relu, float* __restrict__ y, long long ldy) {
    const long long e = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= M * N) return;
    const long long m = e / N, n = e - m * N;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(long long)c * M * N + e];
    if (bias) s += bias[n];
    if (relu) s = s > 0.f ? s : 0.f;
    y[m * ldy + n] = s;
}

// the cell's gate arithmetic after a K split: one thread per (row, hidden unit)
__global__ __launch_bounds__(DN_THREADS) void cell_reduce_kernel(const float* __restrict__ part, int chunks, long long M, int H,
                                                                 const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                                 const float* __restrict__ c, float* h_new, float* c_new, float* gates) {
    const long long e = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= M * H) return;
    const long long m = e / H;
    const int u = (int)(e - m * H);
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float s = 0.f;
        for (int ch = 0; ch < chunks; ++ch) s += part[((long long)ch * M + m) * 4 * H + 4 * u + g];
        pre[g] = s + (b_ih ? b_ih[g * H + u] : 0.f) + (b_hh ? b_hh[g * H + u] : 0.f);
    }
    cell_point(pre, c ? c[e] : 0.f, h_new, c_new, gates, m, u, H);
}

// out[m][n] = y[m][n] > 0 ? dy[m][n] : 0 (the ReLU of a dense layer, read off its output)
__global__ __launch_bounds__(DN_THREADS) void dense_relu_mask_kernel(const float* __restrict__ y, long long ldy, const float* __restrict__ dy,
                                                                     long long lddy, float* __restrict__ out, long long M, long long N) {
    const long long e = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= M * N) return;
    const long long m = e / N, n = e - m * N;
    out[e] = y[m * ldy + n] > 0.f ? dy[m * lddy + n] : 0.f;
}

// dw[n][k] (+)= sum over m, in row order, of dy[m][n] * x[m][k]: a 64 x 64 tile per workgroup, 4 x 4 per thread
constexpr int DW_T = 64, DW_MT = 16;
__global__ __launch_bounds__(DN_THREADS) void dense_dw_kernel(const float* __restrict__ dy, long long lddy, const float* __restrict__ x, long long ldx,
                                                              float* __restrict__ dw, long long M, long long N, long long K, int accumulate) {
    __shared__ float Ds[DW_MT][DW_T + 1];
    __shared__ float Xs[DW_MT][DW_T + 1];
    const int tid = threadIdx.x, tk = tid % 16, tn = tid / 16;
    const long long k0 = (long long)blockIdx.x * DW_T, n0 = (long long)blockIdx.y * DW_T;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (long long mt = 0; mt < M; mt += DW_MT) {
        for (int e = tid; e < DW_MT * DW_T; e += DN_THREADS) {
            const int mm = e / DW_T, cc = e % DW_T;
            const long long m = mt + mm;
            Ds[mm][cc] = (m < M && n0 + cc < N) ? dy[m * lddy + n0 + cc] : 0.f;
            Xs[mm][cc] = (m < M && k0 + cc < K) ? x[m * ldx + k0 + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int mm = 0; mm < DW_MT; ++mm) {
            float dv[4], xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { dv[i] = Ds[mm][tn * 4 + i]; xv[i] = Xs[mm][tk * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += dv[i] * xv[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long n = n0 + tn * 4 + i;
        if (n >= N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long k = k0 + tk * 4 + j;
            if (k >= K) continue;
            float* p = dw + n * K + k;
            *p = accumulate ? *p + acc[i][j] : acc[i][j];
        }
    }
}

// out0[n], out1[n] (+)= sum over m, in row order, of dy[m][n]
__global__ __launch_bounds__(DN_THREADS) void dense_db_kernel(const float* __restrict__ dy, long long lddy, float* out0, float* out1, long long M,
                                                              long long N, int accumulate) {
    const long long n = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (long long m = 0; m < M; ++m) s += dy[m * lddy + n];
    if (out0) out0[n] = accumulate ? out0[n] + s : s;
    if (out1) out1[n] = accumulate ? out1[n] + s : s;
}

// The cell's pointwise backward: from the activated gates, c and the incoming gradients to the gate gradient [M][4H] (torch's order) and dc.
__global__ __launch_bounds__(DN_THREADS) void cell_bwd_point_kernel(const float* __restrict__ gates, const float* __restrict__ c,
                                                                    const float* __restrict__ dh_new, const float* __restrict__ dc_new,
                                                                    float* __restrict__ dgates, float* __restrict__ dc, long long M, int H) {
    const long long e = (long long)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= M * H) return;
    const long long m = e / H;
    const int u = (int)(e - m * H);
    const float* gp = gates + m * 4 * H + u;
    const float i = gp[0], f = gp[H], g = gp[2 * (long long)H], o = gp[3 * (long long)H];
    const float cp = c ? c[e] : 0.f;
    const float t = tanhf(f * cp + i * g);
    const float dhn = dh_new ? dh_new[e] : 0.f;
    const float dct = (dc_new ? dc_new[e] : 0.f) + dhn * o * (1.0f - t * t);
    float* dp = dgates + m * 4 * H + u;
    dp[0] = dct * g * i * (1.0f - i);
    dp[H] = dct * cp * f * (1.0f - f);
    dp[2 * (long long)H] = dct * i * (1.0f - g * g);
    dp[3 * (long long)H] = dhn * t * o * (1.0f - o);
    if (dc) dc[e] = dct * f;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static inline unsigned dn_blocks(long long n) { return (unsigned)((n + DN_THREADS - 1) / DN_THREADS); }

static int dn_check_sizes(const char* who, long long M, long long N, long long K) {
    if (M < 1 || N < 1 || K < 1) { set_error("%s: every size must be >= 1 (M=%lld N=%lld K=%lld)", who, M, N, K); return VPX_ERR_ARG; }
    // int columns inside the kernels, 16-bit grid rows, element counts of one launch below 2^31 blocks
    if (N > (1 << 30) || K > (1 << 30) || M > 65535LL * 8 || (double)M * (double)N > 2.0e11 || (double)M * (double)K > 2.0e11 || (double)N * (double)K > 1.0e12) {
        set_error("%s: M=%lld N=%lld K=%lld exceed one launch", who, M, N, K);
        return VPX_ERR_UNSUPPORTED;
    }
    return VPX_OK;
}

// partial sums of a planned launch (0 floats without a split)
static inline size_t dn_part_floats(const DensePlan& p, long long M, long long N) { return p.chunks > 1 ? (size_t)p.chunks * M * N : 0; }

static hipError_t launch_gemm(GemmArgs& a, const DensePlan& p, bool nn, hipStream_t stream) {
    if (a.part && !ws_write_ok(a.part, (size_t)p.chunks * a.M * a.N * sizeof(float), "K-split partial sums (gemm_kernel)")) return hipErrorInvalidValue;
    a.chunk_len = p.chunk_len;
    const dim3 grid((unsigned)p.n_tiles, (unsigned)p.m_tiles, (unsigned)p.chunks), block(DN_THREADS);
    if (nn) {
        if (p.form == 0) VPX_LAUNCH((gemm_kernel<8, 1, true>), grid, block, 0, stream, a);
        else if (p.form == 1) VPX_LAUNCH((gemm_kernel<32, 1, true>), grid, block, 0, stream, a);
        else VPX_LAUNCH((gemm_kernel<32, 4, true>), grid, block, 0, stream, a);
    } else {
        if (p.form == 0) VPX_LAUNCH((gemm_kernel<8, 1, false>), grid, block, 0, stream, a);
        else if (p.form == 1) VPX_LAUNCH((gemm_kernel<32, 1, false>), grid, block, 0, stream, a);
        else VPX_LAUNCH((gemm_kernel<32, 4, false>), grid, block, 0, stream, a);
    }
    return vpx_hip_last_error();
}

// out[M][Nout] (ldo) = A[M][Kc] (lda) * w, w [Kc][Nout] as stored (row stride ldw): the data gradient of a dense layer
static int dense_dgrad(hipStream_t stream, const float* A, long long lda, const float* w, long long ldw, float* out, long long ldo, long long M,
                       long long Nout, long long Kc, float* part) {
    const DensePlan p = dense_plan_of(M, Nout, Kc);
    GemmArgs a{};
    a.a0 = A; a.lda0 = lda; a.K0 = (int)Kc; a.b0 = w; a.ldb0 = ldw; a.M = (int)M; a.N = (int)Nout;
    a.y = out; a.ldy = ldo;
    a.part = p.chunks > 1 ? part : nullptr;
    VPX_CHECK_HIP(launch_gemm(a, p, true, stream));
    if (p.chunks > 1) {
        VPX_LAUNCH(dense_reduce_kernel, dim3(dn_blocks(M * Nout)), dim3(DN_THREADS), 0, stream, part, p.chunks, M, Nout, (const float*)nullptr, 0, out, ldo);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

static int dense_wgrad(hipStream_t stream, const float* dy, long long lddy, const float* x, long long ldx, float* dw, long long M, long long N,
                       long long K, int accumulate) {
    const long long gy = (N + DW_T - 1) / DW_T;
    if (gy > 65535) { set_error("dense weight gradient: N=%lld exceeds one launch", N); return VPX_ERR_UNSUPPORTED; }
    VPX_LAUNCH(dense_dw_kernel, dim3((unsigned)((K + DW_T - 1) / DW_T), (unsigned)gy), dim3(DN_THREADS), 0, stream, dy, lddy, x, ldx, dw, M, N, K, accumulate);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

template <class WS> static void carve_dense_fwd(WS& ws, long long M, long long N, long long K, float** part) {
    *part = ws.take(dn_part_floats(dense_plan_of(M, N, K), M, N));
}
template <class WS> static void carve_dense_bwd(WS& ws, long long M, long long N, long long K, float** masked, float** part) {
    *masked = ws.take((size_t)M * N);
    *part = ws.take(dn_part_floats(dense_plan_of(M, K, N), M, K));
}
// the two-source launch and the zero-state launch (x alone) plan on their own: a slot each
template <class WS> static void carve_cell_fwd(WS& ws, long long M, long long Kx, long long H, float** part_xh, float** part_x) {
    *part_xh = ws.take(dn_part_floats(dense_plan_of(M, 4 * H, Kx + H), M, 4 * H));
    *part_x = ws.take(dn_part_floats(dense_plan_of(M, 4 * H, Kx), M, 4 * H));
}
template <class WS> static void carve_cell_bwd(WS& ws, long long M, long long Kx, long long H, float** part_x, float** part_h) {
    *part_x = ws.take(dn_part_floats(dense_plan_of(M, Kx, 4 * H), M, Kx));
    *part_h = ws.take(dn_part_floats(dense_plan_of(M, H, 4 * H), M, H));
}

static int cell_check(const char* who, long long M, long long Kx, long long H) {
    if (M < 1 || Kx < 1 || H < 1) { set_error("%s: every size must be >= 1 (M=%lld Kx=%lld H=%lld)", who, M, Kx, H); return VPX_ERR_ARG; }
    if (int rc = dn_check_sizes(who, M, 4 * H, Kx + H)) return rc;
    if (H > (1 << 28)) { set_error("%s: H=%lld exceeds one launch", who, H); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_dense_plan(long long M, long long N, long long K, vpx_dense_plan_info* out) {
    if (!out) { set_error("vpx_dense_plan: out is NULL"); return VPX_ERR_ARG; }
    if (int rc = dn_check_sizes("vpx_dense_plan", M, N, K)) return rc;
    const DensePlan p = dense_plan_of(M, N, K);
    out->split = p.chunks > 1 ? 1 : 0;
    out->chunks = p.chunks; out->chunk_len = p.chunk_len;
    out->form = p.form; out->tile_m = p.tm; out->tile_n = p.tn; out->m_tiles = p.m_tiles; out->n_tiles = p.n_tiles;
    return VPX_OK;
}

size_t vpx_dense_workspace_bytes(long long M, long long N, long long K) {
    if (dn_check_sizes("vpx_dense_workspace_bytes", M, N, K)) return 0;
    CarveMeasure f, b;
    float *p0, *p1;
    carve_dense_fwd(f, M, N, K, &p0);
    carve_dense_bwd(b, M, N, K, &p0, &p1);
    return (f.off > b.off ? f.off : b.off) + 256;
}

int vpx_dense_fwd(const float* x, long long ldx, const float* w, const float* bias, float* y, long long ldy, long long M, long long N, long long K,
                  int relu, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_dense_fwd";
    if (int rc = dn_check_sizes(who, M, N, K)) return rc;
    if (!x || !w || !y) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (ldx < K || ldy < N) { set_error("%s: row strides must cover a row (ldx=%lld < K=%lld or ldy=%lld < N=%lld)", who, ldx, K, ldy, N); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_dense_workspace_bytes(M, N, K)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    float* part;
    carve_dense_fwd(ws, M, N, K, &part);
    VPX_CHECK_CARVE(ws, who);
    const DensePlan p = dense_plan_of(M, N, K);
    GemmArgs a{};
    a.a0 = x; a.lda0 = ldx; a.K0 = (int)K; a.b0 = w; a.ldb0 = K; a.M = (int)M; a.N = (int)N;
    a.y = y; a.ldy = ldy; a.bias0 = bias; a.relu = relu ? 1 : 0;
    a.part = p.chunks > 1 ? part : nullptr;
    VPX_CHECK_HIP(launch_gemm(a, p, false, stream));
    if (p.chunks > 1) {
        VPX_LAUNCH(dense_reduce_kernel, dim3(dn_blocks(M * N)), dim3(DN_THREADS), 0, stream, part, p.chunks, M, N, bias, relu ? 1 : 0, y, ldy);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

int vpx_dense_bwd(const float* x, long long ldx, const float* w, const float* y, long long ldy, const float* dy, long long lddy, float* dx,
                  long long lddx, float* dw, float* db, long long M, long long N, long long K, int relu, int accumulate, void* workspace,
                  size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_dense_bwd";
    if (int rc = dn_check_sizes(who, M, N, K)) return rc;
    if (!dy || (dx && !w) || (dw && !x) || (relu && !y)) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (lddy < N || (dw && ldx < K) || (dx && lddx < K) || (relu && ldy < N)) { set_error("%s: a row stride does not cover its row", who); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_dense_workspace_bytes(M, N, K)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    float *masked, *part;
    carve_dense_bwd(ws, M, N, K, &masked, &part);
    VPX_CHECK_CARVE(ws, who);
    if (relu) {
        if (!ws_write_ok(masked, (size_t)M * N * sizeof(float), "masked gradient (dense_relu_mask_kernel)")) VPX_CHECK_HIP(hipErrorInvalidValue);
        VPX_LAUNCH(dense_relu_mask_kernel, dim3(dn_blocks(M * N)), dim3(DN_THREADS), 0, stream, y, ldy, dy, lddy, masked, M, N);
        VPX_CHECK_HIP(vpx_hip_last_error());
        dy = masked; lddy = N;
    }
    if (dx) if (int rc = dense_dgrad(stream, dy, lddy, w, K, dx, lddx, M, K, N, part)) return rc;
    if (dw) if (int rc = dense_wgrad(stream, dy, lddy, x, ldx, dw, M, N, K, accumulate ? 1 : 0)) return rc;
    if (db) {
        VPX_LAUNCH(dense_db_kernel, dim3(dn_blocks(N)), dim3(DN_THREADS), 0, stream, dy, lddy, db, (float*)nullptr, M, N, accumulate ? 1 : 0);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

size_t vpx_lstm_cell_workspace_bytes(long long M, long long Kx, long long H) {
    if (cell_check("vpx_lstm_cell_workspace_bytes", M, Kx, H)) return 0;
    CarveMeasure f, b;
    float *p0, *p1;
    carve_cell_fwd(f, M, Kx, H, &p0, &p1);
    carve_cell_bwd(b, M, Kx, H, &p0, &p1);
    return (f.off > b.off ? f.off : b.off) + 256;
}

int vpx_lstm_cell_fwd(const float* x, long long ldx, const float* h, const float* c, const float* w_ih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* h_new, float* c_new, float* gates, long long M, long long Kx, long long H, void* workspace,
                      size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_lstm_cell_fwd";
    if (int rc = cell_check(who, M, Kx, H)) return rc;
    if (!x || !w_ih || !h_new || !c_new || (h && !w_hh)) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (ldx < Kx) { set_error("%s: ldx=%lld does not cover a row of %lld", who, ldx, Kx); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lstm_cell_workspace_bytes(M, Kx, H)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    float *part_xh, *part_x;
    carve_cell_fwd(ws, M, Kx, H, &part_xh, &part_x);
    VPX_CHECK_CARVE(ws, who);
    const long long Kh = h ? H : 0;                      // zero state: the h * W_hh^T half is skipped
    const DensePlan p = dense_plan_of(M, 4 * H, Kx + Kh);
    float* part = h ? part_xh : part_x;
    GemmArgs a{};
    a.a0 = x; a.lda0 = ldx; a.K0 = (int)Kx; a.a1 = h; a.lda1 = H; a.K1 = (int)Kh;
    a.b0 = w_ih; a.ldb0 = Kx; a.b1 = w_hh; a.ldb1 = H;
    a.M = (int)M; a.N = (int)(4 * H); a.cell_H = (int)H;
    a.bias0 = b_ih; a.bias1 = b_hh; a.c = c; a.h_new = h_new; a.c_new = c_new; a.gates = gates;
    a.part = p.chunks > 1 ? part : nullptr;
    VPX_CHECK_HIP(launch_gemm(a, p, false, stream));
    if (p.chunks > 1) {
        VPX_LAUNCH(cell_reduce_kernel, dim3(dn_blocks(M * H)), dim3(DN_THREADS), 0, stream, part, p.chunks, M, (int)H, b_ih, b_hh, c, h_new, c_new, gates);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

int vpx_lstm_cell_bwd(const float* x, long long ldx, const float* h, const float* c, const float* w_ih, const float* w_hh, const float* gates,
                      const float* dh_new, const float* dc_new, float* dx, float* dh, float* dc, float* dw_ih, float* dw_hh, float* db_ih,
                      float* db_hh, float* dgates, long long M, long long Kx, long long H, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream_) {
    const char* who = "vpx_lstm_cell_bwd";
    if (int rc = cell_check(who, M, Kx, H)) return rc;
    if (!gates || !dgates || (dx && !w_ih) || (dh && !w_hh) || (dw_ih && !x)) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (dw_ih && ldx < Kx) { set_error("%s: ldx=%lld does not cover a row of %lld", who, ldx, Kx); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_lstm_cell_workspace_bytes(M, Kx, H)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    float *part_x, *part_h;
    carve_cell_bwd(ws, M, Kx, H, &part_x, &part_h);
    VPX_CHECK_CARVE(ws, who);
    accumulate = accumulate ? 1 : 0;
    VPX_LAUNCH(cell_bwd_point_kernel, dim3(dn_blocks(M * H)), dim3(DN_THREADS), 0, stream, gates, c, dh_new, dc_new, dgates, dc, M, (int)H);
    VPX_CHECK_HIP(vpx_hip_last_error());
    const long long N4 = 4 * H;
    if (dx) if (int rc = dense_dgrad(stream, dgates, N4, w_ih, Kx, dx, Kx, M, Kx, N4, part_x)) return rc;
    if (dh) if (int rc = dense_dgrad(stream, dgates, N4, w_hh, H, dh, H, M, H, N4, part_h)) return rc;
    if (dw_ih) if (int rc = dense_wgrad(stream, dgates, N4, x, ldx, dw_ih, M, N4, Kx, accumulate)) return rc;
    if (dw_hh) {
        if (h) { if (int rc = dense_wgrad(stream, dgates, N4, h, H, dw_hh, M, N4, H, accumulate)) return rc; }
        else if (!accumulate) VPX_CHECK_HIP(vpx_memset_async(dw_hh, 0, (size_t)N4 * H * sizeof(float), stream));   // zero state: no contribution
    }
    if (db_ih || db_hh) {
        VPX_LAUNCH(dense_db_kernel, dim3(dn_blocks(N4)), dim3(DN_THREADS), 0, stream, (const float*)dgates, N4, db_ih, db_hh, M, N4, accumulate);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    return VPX_OK;
}

}  // extern "C"
