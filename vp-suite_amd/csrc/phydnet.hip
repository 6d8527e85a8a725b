// phydnet.hip — the three small kernels of PhyDNet (vp_suite/models/phydnet.py, vp_suite/model_blocks/phydnet.py) that are not
// convolutions, GroupNorm (groupnorm.hip) or the ConvLSTM cell:
//   * the PhyCell's prediction-correction update  next = ht + σ(G)·(E − ht), ht = h + F(h)      (PhyCell_Cell.forward)
//   * the moment regularisation loss over the first filter bank of F (K2M + the loss of PhyDNet.forward), in fp64
//   * the sigmoid output head, written straight into frame slots of the [B, T, C, H, W] result (torch.sigmoid + torch.stack)
#include "vpx_host.h"

namespace vpx {

__device__ __forceinline__ float pd_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ void phycell_correct_fwd_kernel(const float* __restrict__ G, const float* __restrict__ Fh, const float* __restrict__ h,
                                           const float* __restrict__ E, float* __restrict__ next, long long n) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float ht = h[e] + Fh[e];
    next[e] = ht + pd_sigmoid(G[e]) * (E[e] - ht);
}

__global__ void phycell_correct_bwd_kernel(const float* __restrict__ G, const float* __restrict__ Fh, const float* __restrict__ h,
                                           const float* __restrict__ E, const float* __restrict__ dn, float* __restrict__ dG,
                                           float* __restrict__ dh, float* __restrict__ dFh, float* __restrict__ dE, long long n) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float k = pd_sigmoid(G[e]), d = dn[e];
    const float dht = d - k * d;   // d · (1 − k)
    if (dG) dG[e] = d * (E[e] - (h[e] + Fh[e])) * k * (1.0f - k);
    if (dh) dh[e] = dht;
    if (dFh) dFh[e] = dht;
    if (dE) dE[e] = k * d;
}

// ---- moment loss ------------------------------------------------------------------------------------------------------------
constexpr int ML_MAXK = 8;
constexpr int ML_THREADS = 1024;

// M[i][u] = (u − (k−1)/2)^i / i!  (K2M's moment matrix; exact small integers over exact factorials, divided once in fp64),
// built by the first 2·ML_MAXK² threads of the workgroup into LDS
__device__ __forceinline__ void ml_matrices(double M0[ML_MAXK][ML_MAXK], double M1[ML_MAXK][ML_MAXK], int kh, int kw) {
    const int t = threadIdx.x;
    if (t < 2 * ML_MAXK * ML_MAXK) {
        const int which = t / (ML_MAXK * ML_MAXK), i = (t / ML_MAXK) % ML_MAXK, u = t % ML_MAXK, k = which ? kw : kh;
        double f = 1.0, p = 1.0;
        for (int q = 2; q <= i; ++q) f *= q;
        for (int q = 0; q < i; ++q) p *= (double)(u - (k - 1) / 2);
        (which ? M1 : M0)[i][u] = (i < k && u < k) ? p / f : 0.0;
    }
    __syncthreads();
}

// D = M0 · w · M1^T − C for one (o, b) filter w [kh][kw]
__device__ __forceinline__ void ml_residual(const float* __restrict__ w, int o, int kh, int kw, const double M0[ML_MAXK][ML_MAXK],
                                            const double M1[ML_MAXK][ML_MAXK], double D[ML_MAXK][ML_MAXK]) {
    double tmp[ML_MAXK][ML_MAXK];   // tmp[u][j] = Σ_v w[u][v] M1[j][v]
    for (int u = 0; u < kh; ++u)
        for (int j = 0; j < kw; ++j) {
            double acc = 0.0;
            for (int v = 0; v < kw; ++v) acc += (double)w[u * kw + v] * M1[j][v];
            tmp[u][j] = acc;
        }
    for (int i = 0; i < kh; ++i)
        for (int j = 0; j < kw; ++j) {
            double acc = 0.0;
            for (int u = 0; u < kh; ++u) acc += M0[i][u] * tmp[u][j];
            D[i][j] = acc - (o == i * kw + j ? 1.0 : 0.0);
        }
}

// one workgroup; thread t takes the (o, b) pairs t, t + 1024, ... in order, then an fp64 LDS tree: fixed order
__global__ __launch_bounds__(ML_THREADS) void moment_loss_fwd_kernel(const float* __restrict__ W, float* __restrict__ loss, int hidden,
                                                                     int Cin, int kh, int kw, double coef) {
    __shared__ double red[ML_THREADS];
    __shared__ double M0[ML_MAXK][ML_MAXK], M1[ML_MAXK][ML_MAXK];
    double D[ML_MAXK][ML_MAXK];
    ml_matrices(M0, M1, kh, kw);
    double acc = 0.0;
    for (int pr = threadIdx.x; pr < hidden * Cin; pr += ML_THREADS) {
        const int o = pr / Cin, b = pr - o * Cin;
        ml_residual(W + ((size_t)o * Cin + b) * kh * kw, o, kh, kw, M0, M1, D);
        for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j) acc += D[i][j] * D[i][j];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = ML_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] * coef);
}

// dW[o][b] = dloss · 2·coef · M0^T D M1, one thread per (o, b)
__global__ void moment_loss_bwd_kernel(const float* __restrict__ W, const float* __restrict__ dloss, float* __restrict__ dW, int hidden,
                                       int Cin, int kh, int kw, double coef) {
    __shared__ double M0[ML_MAXK][ML_MAXK], M1[ML_MAXK][ML_MAXK];
    ml_matrices(M0, M1, kh, kw);   // (before the range check: every thread reaches the barrier)
    const int pr = blockIdx.x * blockDim.x + threadIdx.x;
    if (pr >= hidden * Cin) return;
    const int o = pr / Cin, b = pr - o * Cin;
    double D[ML_MAXK][ML_MAXK], tmp[ML_MAXK][ML_MAXK];
    const size_t off = ((size_t)o * Cin + b) * kh * kw;
    ml_residual(W + off, o, kh, kw, M0, M1, D);
    const double g = 2.0 * coef * (double)dloss[0];
    for (int u = 0; u < kh; ++u)   // tmp[u][j] = Σ_i M0[i][u] D[i][j]
        for (int j = 0; j < kw; ++j) {
            double acc = 0.0;
            for (int i = 0; i < kh; ++i) acc += M0[i][u] * D[i][j];
            tmp[u][j] = acc;
        }
    for (int u = 0; u < kh; ++u)
        for (int v = 0; v < kw; ++v) {
            double acc = 0.0;
            for (int j = 0; j < kw; ++j) acc += tmp[u][j] * M1[j][v];
            dW[off + u * kw + v] = (float)(g * acc);
        }
}

// ---- sigmoid output head ------------------------------------------------------------------------------------------------------
// element e enumerates out's slots t0 .. t0+nT−1 in out's order [b][k][c][p]; x is [k][b][p][c]
struct SHIdx { size_t xo, oo; };
__device__ __forceinline__ SHIdx sh_index(long long e, int B, int T, int t0, int nT, int C, int HW) {
    const int p = (int)(e % HW);
    long long r = e / HW;
    const int c = (int)(r % C); r /= C;
    const int k = (int)(r % nT);
    const int b = (int)(r / nT);
    SHIdx s;
    s.xo = (((size_t)k * B + b) * HW + p) * C + c;
    s.oo = (((size_t)b * T + t0 + k) * C + c) * HW + p;
    return s;
}

__global__ void sigmoid_head_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int T, int t0, int nT, int C, int HW) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= (long long)B * nT * C * HW) return;
    const SHIdx s = sh_index(e, B, T, t0, nT, C, HW);
    out[s.oo] = pd_sigmoid(x[s.xo]);
}

__global__ void sigmoid_head_bwd_kernel(const float* __restrict__ out, const float* __restrict__ dout, float* __restrict__ dx, int B, int T,
                                        int t0, int nT, int C, int HW) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= (long long)B * nT * C * HW) return;
    const SHIdx s = sh_index(e, B, T, t0, nT, C, HW);
    const float y = out[s.oo];
    dx[s.xo] = dout[s.oo] * y * (1.0f - y);
}

static inline unsigned pd_blocks(long long n) { return (unsigned)((n + 255) / 256); }

static int sh_check(const char* who, int B, int T, int t0, int nT, int C, int H, int W) {
    if (B < 1 || T < 1 || nT < 1 || t0 < 0 || t0 + nT > T || C < 1 || H < 1 || W < 1) {
        set_error("%s: bad shape (B=%d T=%d t0=%d nT=%d C=%d H=%d W=%d)", who, B, T, t0, nT, C, H, W);
        return VPX_ERR_ARG;
    }
    return VPX_OK;
}

static int ml_check(const char* who, int hidden, int Cin, int kh, int kw) {
    if (hidden < 1 || Cin < 1 || kh < 1 || kw < 1 || kh > ML_MAXK || kw > ML_MAXK) {
        set_error("%s: bad shape (hidden=%d Cin=%d kernel %dx%d; at most %d taps per side)", who, hidden, Cin, kh, kw, ML_MAXK);
        return VPX_ERR_ARG;
    }
    return VPX_OK;
}

}  // namespace vpx

extern "C" {

int vpx_phycell_correct_fwd(const float* G, const float* Fh, const float* h, const float* E, float* next, long long n, void* stream) {
    using namespace vpx;
    if (!G || !Fh || !h || !E || !next || n < 1) { set_error("vpx_phycell_correct_fwd: bad argument"); return VPX_ERR_ARG; }
    VPX_LAUNCH(phycell_correct_fwd_kernel, dim3(pd_blocks(n)), dim3(256), 0, (hipStream_t)stream, G, Fh, h, E, next, n);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_phycell_correct_bwd(const float* G, const float* Fh, const float* h, const float* E, const float* dnext, float* dG, float* dh,
                            float* dFh, float* dE, long long n, void* stream) {
    using namespace vpx;
    if (!G || !Fh || !h || !E || !dnext || n < 1) { set_error("vpx_phycell_correct_bwd: bad argument"); return VPX_ERR_ARG; }
    VPX_LAUNCH(phycell_correct_bwd_kernel, dim3(pd_blocks(n)), dim3(256), 0, (hipStream_t)stream, G, Fh, h, E, dnext, dG, dh, dFh, dE, n);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_moment_loss_fwd(const float* W, float* loss, int hidden, int Cin, int kh, int kw, float scale, void* stream) {
    using namespace vpx;
    if (!W || !loss) { set_error("vpx_moment_loss_fwd: NULL argument"); return VPX_ERR_ARG; }
    if (int rc = ml_check("vpx_moment_loss_fwd", hidden, Cin, kh, kw)) return rc;
    const double coef = (double)scale / ((double)hidden * kh * kw);
    VPX_LAUNCH(moment_loss_fwd_kernel, dim3(1), dim3(ML_THREADS), 0, (hipStream_t)stream, W, loss, hidden, Cin, kh, kw, coef);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_moment_loss_bwd(const float* W, const float* dloss, float* dW, int hidden, int Cin, int kh, int kw, float scale, void* stream) {
    using namespace vpx;
    if (!W || !dloss || !dW) { set_error("vpx_moment_loss_bwd: NULL argument"); return VPX_ERR_ARG; }
    if (int rc = ml_check("vpx_moment_loss_bwd", hidden, Cin, kh, kw)) return rc;
    const double coef = (double)scale / ((double)hidden * kh * kw);
    VPX_LAUNCH(moment_loss_bwd_kernel, dim3(pd_blocks((long long)hidden * Cin)), dim3(256), 0, (hipStream_t)stream, W, dloss, dW, hidden,
               Cin, kh, kw, coef);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_sigmoid_head_fwd(const float* x, float* out, int B, int T, int t0, int nT, int C, int H, int W, void* stream) {
    using namespace vpx;
    if (!x || !out) { set_error("vpx_sigmoid_head_fwd: NULL argument"); return VPX_ERR_ARG; }
    if (int rc = sh_check("vpx_sigmoid_head_fwd", B, T, t0, nT, C, H, W)) return rc;
    VPX_LAUNCH(sigmoid_head_fwd_kernel, dim3(pd_blocks((long long)B * nT * C * H * W)), dim3(256), 0, (hipStream_t)stream, x, out, B, T, t0,
               nT, C, H * W);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_sigmoid_head_bwd(const float* out, const float* dout, float* dx, int B, int T, int t0, int nT, int C, int H, int W, void* stream) {
    using namespace vpx;
    if (!out || !dout || !dx) { set_error("vpx_sigmoid_head_bwd: NULL argument"); return VPX_ERR_ARG; }
    if (int rc = sh_check("vpx_sigmoid_head_bwd", B, T, t0, nT, C, H, W)) return rc;
    VPX_LAUNCH(sigmoid_head_bwd_kernel, dim3(pd_blocks((long long)B * nT * C * H * W)), dim3(256), 0, (hipStream_t)stream, out, dout, dx, B,
               T, t0, nT, C, H * W);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

}  // extern "C"
