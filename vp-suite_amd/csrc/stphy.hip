// stphy.hip — what ST-Phy (vp_suite/models/st_phy.py) needs beyond the cells: the encoder tail of its autoencoder
// (vp_suite/model_blocks/enc.py Encoder.forward: F.normalize(relu(.), p=2, dim=-1, eps=1e-8)) and the per-layer merge
// hidden_conv(cat([st_h, phy_h], dim=1)) (st_phy.py:152) over two sources.
//   * relu_rownorm: y = r / max(||r||_2 over W, eps), r = relu(x), on channels-last [N][H][W][C]. One thread owns the W pixels of
//     one (sample, row, 4-channel group): lanes run along C, so every load and store of a wave is one contiguous run of 16-byte
//     accesses; W is short (12 at 64x64 frames), the second pass over the row hits L2. The row norm is saved for the backward.
//   * merge: a biased 1x1 convolution whose K axis is split over two tensors. The two halves run on the implicit-GEMM kernel
//     (f32 / bf16x3 like every other 1x1 layer), the second accumulating into the first's output: no concatenated copy exists.
//     c1_kernel (conv1.hip) has a two-source form, but only for bf16x3 at (Co, K) in {(128, 256), (256, 128), (128, 128)} and without
//     a bias; the merge is (64, 128) at the default width and must run in f32 too.
//     Backward: da / db = the adjoint 1x1 layers on dy, dW = the two weight gradients written side by side, dbias = column sums —
//     all fixed-order reductions (no float atomics under vpx_set_deterministic(1)).
// (ReLU on the convolution path — vpx_conv2d_act_fwd / _bwd — lives with the layer launchers in glue_fwd_api.hip / glue_bwd_api.hip.)
#include "vpx_host.h"

namespace vpx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int V> struct RnVec;
template <> struct RnVec<1> { typedef float t; };
template <> struct RnVec<4> { typedef f32x4 t; };
__device__ __forceinline__ float rn_get(float v, int) { return v; }
__device__ __forceinline__ float rn_get(const f32x4& v, int i) { return v[i]; }
__device__ __forceinline__ void rn_set(float& v, int, float x) { v = x; }
__device__ __forceinline__ void rn_set(f32x4& v, int i, float x) { v[i] = x; }

template <int V>   // V = 4: 16-byte accesses (C % 4 == 0, aligned tensors); V = 1: scalar
__global__ __launch_bounds__(256) void relu_rownorm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ norm,
                                                               long long rows, int W, int C, float eps) {
    typedef typename RnVec<V>::t vec;
    const int vc = C / V;
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= rows * vc) return;
    const long long row = e / vc;
    const int cg = (int)(e - row * vc);
    const vec* xp = reinterpret_cast<const vec*>(x) + row * W * vc + cg;
    vec* yp = reinterpret_cast<vec*>(y) + row * W * vc + cg;
    float ss[V], s[V];
#pragma unroll
    for (int i = 0; i < V; ++i) ss[i] = 0.f;
    for (int w = 0; w < W; ++w) {
        const vec v = xp[(long long)w * vc];
#pragma unroll
        for (int i = 0; i < V; ++i) { const float r = rn_get(v, i) > 0.f ? rn_get(v, i) : 0.f; ss[i] += r * r; }
    }
    vec n;
#pragma unroll
    for (int i = 0; i < V; ++i) { const float nv = sqrtf(ss[i]); rn_set(n, i, nv); s[i] = 1.0f / (nv > eps ? nv : eps); }
    if (norm) reinterpret_cast<vec*>(norm)[e] = n;
    for (int w = 0; w < W; ++w) {
        const vec v = xp[(long long)w * vc];
        vec o;
#pragma unroll
        for (int i = 0; i < V; ++i) rn_set(o, i, rn_get(v, i) > 0.f ? rn_get(v, i) * s[i] : 0.f);
        yp[(long long)w * vc] = o;
    }
}

// dr = (dy - y * <dy, y>) / n  where n >= eps (F.normalize's clamp passes the gradient there), dy / eps below it (the clamp's
// derivative is zero: y = r / eps); dx = dr where x > 0. y is recomputed from x and n. A select per case, never 0 * inf.
template <int V>
__global__ __launch_bounds__(256) void relu_rownorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ norm,
                                                               const float* __restrict__ dy, float* __restrict__ dx, long long rows, int W,
                                                               int C, float eps) {
    typedef typename RnVec<V>::t vec;
    const int vc = C / V;
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= rows * vc) return;
    const long long row = e / vc;
    const int cg = (int)(e - row * vc);
    const long long base = row * W * vc + cg;
    const vec* xp = reinterpret_cast<const vec*>(x) + base;
    const vec* gp = reinterpret_cast<const vec*>(dy) + base;
    vec* dp = reinterpret_cast<vec*>(dx) + base;
    const vec n = reinterpret_cast<const vec*>(norm)[e];
    float s[V], dot[V];
    bool big[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float nv = rn_get(n, i);
        big[i] = nv >= eps;
        s[i] = 1.0f / (big[i] ? nv : eps);
        dot[i] = 0.f;
    }
    for (int w = 0; w < W; ++w) {
        const vec v = xp[(long long)w * vc], g = gp[(long long)w * vc];
#pragma unroll
        for (int i = 0; i < V; ++i) dot[i] += rn_get(v, i) > 0.f ? rn_get(g, i) * (rn_get(v, i) * s[i]) : 0.f;
    }
    for (int w = 0; w < W; ++w) {
        const vec v = xp[(long long)w * vc], g = gp[(long long)w * vc];
        vec o;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float vi = rn_get(v, i), gi = rn_get(g, i);
            const float dr = big[i] ? (gi - vi * s[i] * dot[i]) * s[i] : gi * s[i];
            rn_set(o, i, vi > 0.f ? dr : 0.f);
        }
        dp[(long long)w * vc] = o;
    }
}

// dW [Co][Cs + Cp] = [dWa [Co][Cs] | dWb [Co][Cp]]
__global__ void merge_dw_kernel(const float* __restrict__ dWa, const float* __restrict__ dWb, float* __restrict__ dW, int Co, int Cs, int Cp) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int K = Cs + Cp;
    if (e >= Co * K) return;
    const int o = e / K, k = e - o * K;
    dW[e] = k < Cs ? dWa[o * Cs + k] : dWb[o * Cp + (k - Cs)];
}

static int rn_check(const char* who, int N, int H, int W, int C, float eps) {
    if (N < 1 || H < 1 || W < 1 || C < 1 || !(eps > 0.0f)) {
        set_error("%s: bad argument (N=%d H=%d W=%d C=%d eps=%g)", who, N, H, W, C, (double)eps);
        return VPX_ERR_ARG;
    }
    return VPX_OK;
}

static inline bool rn_vec4(int C, const void* a, const void* b, const void* c, const void* d) {
    return (C & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

static int merge_check(const char* who, int N, int H, int W, int Cs, int Cp, int Co, int prec) {
    if (N < 1 || H < 1 || W < 1 || Cs < 1 || Cp < 1 || Co < 1) {
        set_error("%s: bad shape (N=%d H=%d W=%d Cs=%d Cp=%d Co=%d)", who, N, H, W, Cs, Cp, Co);
        return VPX_ERR_ARG;
    }
    if (prec != VPX_PREC_F32 && prec != VPX_PREC_BF16X3) { set_error("%s: precision %d not implemented (f32, bf16x3)", who, prec); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

// The workspaces: every slot in the order the call takes it. One weight pack serves both halves, so it holds the larger one.
struct MergeFwdSlots { float* wpk; };
template <class WS>
static void carve_merge_fwd(WS& ws, int Cs, int Cp, int Co, MergeFwdSlots& s) {
    const size_t a = plain_conv_wpk_floats(Cs, Co, 1, 1), b = plain_conv_wpk_floats(Cp, Co, 1, 1);
    s.wpk = ws.take(a > b ? a : b);
}
// ... and one slab slot both weight gradients, sized for the wider half (Cm channels); cap_a, cap_b: the slice cap each half's launch gets
// (its own geometry's, within what the slot was sized for)
struct MergeBwdSlots { float *wpk, *slabs, *db_part, *dWa, *dWb; int Cm, cap_a, cap_b; };
template <class WS>
static void carve_merge_bwd(WS& ws, int N, int H, int W, int Cs, int Cp, int Co, MergeBwdSlots& s) {
    const size_t a = plain_conv_wpk_floats(Co, Cs, 1, 1), b = plain_conv_wpk_floats(Co, Cp, 1, 1);
    s.Cm = Cs > Cp ? Cs : Cp;
    const int cap_m = wgrad_slices_for(N, H, W, Co, s.Cm, 1, 1);
    s.cap_a = std::min(wgrad_slices_for(N, H, W, Co, Cs, 1, 1), cap_m);
    s.cap_b = std::min(wgrad_slices_for(N, H, W, Co, Cp, 1, 1), cap_m);
    s.wpk = ws.take(a > b ? a : b);
    s.slabs = ws.take((size_t)cap_m * Co * s.Cm);
    s.db_part = ws.take((size_t)COLSUM_BLOCKS * Co);
    s.dWa = ws.take((size_t)Co * Cs);
    s.dWb = ws.take((size_t)Co * Cp);
}

}  // namespace vpx

using namespace vpx;

extern "C" {

int vpx_relu_rownorm_fwd(const float* x, float* y, float* norm, int N, int H, int W, int C, float eps, void* stream) {
    if (!x || !y) { set_error("vpx_relu_rownorm_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (int rc = rn_check("vpx_relu_rownorm_fwd", N, H, W, C, eps)) return rc;
    const long long rows = (long long)N * H;
    if (rn_vec4(C, x, y, norm, nullptr))
        VPX_LAUNCH(relu_rownorm_fwd_kernel<4>, dim3((unsigned)((rows * (C / 4) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, norm, rows, W, C, eps);
    else
        VPX_LAUNCH(relu_rownorm_fwd_kernel<1>, dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, norm, rows, W, C, eps);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

int vpx_relu_rownorm_bwd(const float* x, const float* norm, const float* dy, float* dx, int N, int H, int W, int C, float eps, void* stream) {
    if (!x || !norm || !dy || !dx) { set_error("vpx_relu_rownorm_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (int rc = rn_check("vpx_relu_rownorm_bwd", N, H, W, C, eps)) return rc;
    const long long rows = (long long)N * H;
    if (rn_vec4(C, x, norm, dy, dx))
        VPX_LAUNCH(relu_rownorm_bwd_kernel<4>, dim3((unsigned)((rows * (C / 4) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, norm, dy, dx, rows, W, C, eps);
    else
        VPX_LAUNCH(relu_rownorm_bwd_kernel<1>, dim3((unsigned)((rows * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, norm, dy, dx, rows, W, C, eps);
    VPX_CHECK_HIP(vpx_hip_last_error());
    return VPX_OK;
}

size_t vpx_merge1x1_workspace_bytes(int Cs, int Cp, int Co) {
    if (Cs < 1 || Cp < 1 || Co < 1) return 0;
    CarveMeasure m; MergeFwdSlots s{};
    carve_merge_fwd(m, Cs, Cp, Co, s);
    return m.off + 512;
}

int vpx_merge1x1_fwd(const float* a, const float* b, const float* w, const float* bias, float* y, int N, int H, int W, int Cs, int Cp,
                     int Co, int precision, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = merge_check("vpx_merge1x1_fwd", N, H, W, Cs, Cp, Co, precision)) return rc;
    if (!a || !b || !w || !y) { set_error("vpx_merge1x1_fwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_merge1x1_workspace_bytes(Cs, Cp, Co)) { set_error("vpx_merge1x1_fwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    MergeFwdSlots s{};
    carve_merge_fwd(ws, Cs, Cp, Co, s);
    VPX_CHECK_CARVE(ws, "vpx_merge1x1_fwd");
    const ConvGeo g{N, H, W};
    const long long K = (long long)Cs + Cp;
    int rc;
    if ((rc = plain_conv(stream, precision, g, a, Cs, Cs, w, K, 1, 1, 1, Co, false, bias, y, Co, false, s.wpk))) return rc;
    return plain_conv(stream, precision, g, b, Cp, Cp, w + Cs, K, 1, 1, 1, Co, false, nullptr, y, Co, true, s.wpk);
}

size_t vpx_merge1x1_bwd_workspace_bytes(int N, int H, int W, int Cs, int Cp, int Co) {
    if (N < 1 || H < 1 || W < 1 || Cs < 1 || Cp < 1 || Co < 1) return 0;
    CarveMeasure m; MergeBwdSlots s{};
    carve_merge_bwd(m, N, H, W, Cs, Cp, Co, s);
    return m.off + 1024;
}

int vpx_merge1x1_bwd(const float* a, const float* b, const float* w, const float* dy, float* da, float* db, float* dw, float* dbias, int N,
                     int H, int W, int Cs, int Cp, int Co, int precision, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = merge_check("vpx_merge1x1_bwd", N, H, W, Cs, Cp, Co, precision)) return rc;
    if (!a || !b || !w || !dy) { set_error("vpx_merge1x1_bwd: NULL tensor argument"); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_merge1x1_bwd_workspace_bytes(N, H, W, Cs, Cp, Co)) { set_error("vpx_merge1x1_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    MergeBwdSlots s{};
    carve_merge_bwd(ws, N, H, W, Cs, Cp, Co, s);
    VPX_CHECK_CARVE(ws, "vpx_merge1x1_bwd");
    const ConvGeo g{N, H, W};
    const long long K = (long long)Cs + Cp;
    int rc;
    if (da && (rc = plain_conv(stream, precision, g, dy, Co, Co, w, K, 1, 1, 1, Cs, true, nullptr, da, Cs, false, s.wpk))) return rc;
    if (db && (rc = plain_conv(stream, precision, g, dy, Co, Co, w + Cs, K, 1, 1, 1, Cp, true, nullptr, db, Cp, false, s.wpk))) return rc;
    if (dw) {
        if ((rc = plain_wgrad(stream, precision, g, dy, Co, a, Cs, 1, 1, s.slabs, s.dWa, nullptr, s.cap_a))) return rc;
        if ((rc = plain_wgrad(stream, precision, g, dy, Co, b, Cp, 1, 1, s.slabs, s.dWb, nullptr, s.cap_b))) return rc;
        VPX_LAUNCH(merge_dw_kernel, dim3((unsigned)((Co * K + 255) / 256)), dim3(256), 0, stream, s.dWa, s.dWb, dw, Co, Cs, Cp);
        VPX_CHECK_HIP(vpx_hip_last_error());
    }
    if (dbias) VPX_CHECK_HIP(launch_colsum(dy, nullptr, 0.f, nullptr, dbias, s.db_part, (long long)N * H * W, Co, stream));
    return VPX_OK;
}

}  // extern "C"
