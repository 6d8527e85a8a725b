// decouple_api.hip — the decoupling-loss tail (include/vpx.h; vp_suite/models/predrnn_v2.py:197-198, 209-211). Host code only.
//   vpx_decouple_fwd / _bwd   adapter 1x1 conv on delta_c / delta_m, per-(b, channel) cosine over H*W, |.|, mean
// Arithmetic of the tail's three 1x1 contractions (adapter forward, its adjoint, its weight gradient) = the caller's `precision`
// argument (the model's operand mode). bf16x3: fp32-level accuracy (4e-6; the loss value and its gradients hold the goldens'
// 1e-4 / 5e-5 bars) at a third of the exact-fp32 MFMA cycles — the fp32 forms cost PredRNN's bf16x3 training step 34 of 493 ms.
#include "vpx_host.h"
using namespace vpx;

namespace {
// The adapter (1x1, Ch -> Ch; transposed = its adjoint) applied to the c and the m operand. When both the sources and the
// destinations are adjacent in memory ([2, B, HW, Ch]: the cell step hands out delta_c | delta_m as one block, the
// workspace slots are adjacent) the pair is ONE convolution over 2B images — these launches are latency-bound (K = Ch).
int decouple_adapter_pair(hipStream_t stream, int prec, ConvGeo g, const float* sc, const float* sm, const float* adapter,
                          float* oc, float* om, size_t n, int Ch, bool transposed, float* wpk) {
    int rc;
    {   // streaming 1x1 kernel (conv1.hip): weights resident in registers, fp32 in and out
        C1Args c{};
        c.x[0] = sc; c.xld[0] = Ch; c.xc[0] = Ch; c.x[1] = nullptr; c.xld[1] = 0; c.xc[1] = 0;
        c.npix = (long long)g.N * g.H * g.W;
        c.w = adapter; c.w_sn = transposed ? 1 : Ch; c.w_sc = transposed ? Ch : 1;
        c.y[0] = oc; c.y[1] = nullptr; c.yld[0] = Ch; c.yld[1] = 0; c.ysplit = Ch; c.Co = Ch; c.accumulate = 0;
        if (c1_applicable(c, prec)) {
            if (sm == sc + n && om == oc + n) { c.npix *= 2; VPX_CHECK_HIP(launch_c1(c, stream)); return VPX_OK; }
            VPX_CHECK_HIP(launch_c1(c, stream));
            c.x[0] = sm; c.y[0] = om;
            VPX_CHECK_HIP(launch_c1(c, stream));
            return VPX_OK;
        }
    }
    if (sm == sc + n && om == oc + n) {
        const ConvGeo g2{2 * g.N, g.H, g.W};
        return plain_conv(stream, prec, g2, sc, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, transposed, nullptr, oc, Ch, false, wpk);
    }
    if ((rc = plain_conv(stream, prec, g, sc, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, transposed, nullptr, oc, Ch, false, wpk))) return rc;
    return plain_conv(stream, prec, g, sm, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, transposed, nullptr, om, Ch, false, wpk);
}

// The workspace: ONE list of slots. The forward takes its own (the adapter outputs, the statistics, the weight pack); the backward
// adds their gradients, the weight gradient's slabs and the second pair's dA. The one size query measures the backward's list.
struct DecoupleSlots { float *yc, *ym, *dyc, *dym, *stats, *wpk, *slabs, *dA2; int slice_cap; };
template <class WS>
void carve_decouple(WS& ws, int B, int Ch, int H, int W, bool bwd, DecoupleSlots& s) {
    const size_t n = (size_t)B * H * W * Ch;
    s.yc = ws.take(n);
    s.ym = ws.take(n);
    if (bwd) { s.dyc = ws.take(n); s.dym = ws.take(n); }
    s.stats = ws.take((size_t)B * Ch * 4);
    s.wpk = ws.take(plain_conv_wpk_floats(Ch, Ch, 1, 1));
    if (!bwd) return;
    s.slice_cap = wgrad_slices_1x1(B, H, W);
    s.slabs = ws.take((size_t)s.slice_cap * Ch * Ch);
    s.dA2 = ws.take((size_t)Ch * Ch);
}

// what both directions refuse, in their order: bad argument, unknown precision, workspace
int decouple_check(const char* who, bool args_ok, int B, int Ch, int H, int W, int prec, const void* workspace, size_t workspace_bytes) {
    if (!args_ok || B < 1 || Ch < 1 || H < 1 || W < 1) { set_error("%s: bad argument", who); return VPX_ERR_ARG; }
    if (prec != VPX_PREC_F32 && prec != VPX_PREC_BF16X3 && prec != VPX_PREC_BF16) { set_error("%s: unknown precision %d", who, prec); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_decouple_workspace_bytes(B, Ch, H, W)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    return VPX_OK;
}
}  // namespace

extern "C" {
size_t vpx_decouple_workspace_bytes(int B, int Ch, int H, int W) {
    if (B < 1 || Ch < 1 || H < 1 || W < 1) return 0;
    CarveMeasure m; DecoupleSlots s{};
    carve_decouple(m, B, Ch, H, W, true, s);
    return m.off + 1024;
}
int vpx_decouple_fwd(const float* delta_c, const float* delta_m, const float* adapter, float* value, int B, int Ch, int H, int W, int prec,
                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = decouple_check("vpx_decouple_fwd", delta_c && delta_m && adapter && value, B, Ch, H, W, prec, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)B * H * W * Ch;
    Carver ws(workspace, workspace_bytes);
    DecoupleSlots s{};
    carve_decouple(ws, B, Ch, H, W, false, s);
    VPX_CHECK_CARVE(ws, "vpx_decouple_fwd");
    const ConvGeo g{B, H, W};
    if (int rc = decouple_adapter_pair(stream, prec, g, delta_c, delta_m, adapter, s.yc, s.ym, n, Ch, false, s.wpk)) return rc;
    VPX_CHECK_HIP(launch_decouple_stats(s.yc, s.ym, s.stats, B, H * W, Ch, stream));
    VPX_CHECK_HIP(launch_decouple_mean(s.stats, value, B * Ch, stream));
    return VPX_OK;
}
int vpx_decouple_bwd(const float* delta_c, const float* delta_m, const float* adapter, const float* dvalue, float* d_delta_c, float* d_delta_m,
                     float* d_adapter, int B, int Ch, int H, int W, int prec, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = decouple_check("vpx_decouple_bwd", delta_c && delta_m && adapter && dvalue, B, Ch, H, W, prec, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)B * H * W * Ch;
    Carver ws(workspace, workspace_bytes);
    DecoupleSlots s{};
    carve_decouple(ws, B, Ch, H, W, true, s);
    VPX_CHECK_CARVE(ws, "vpx_decouple_bwd");
    const ConvGeo g{B, H, W};
    int rc;   // recompute the adapter outputs (cheaper than keeping them alive between forward and backward)
    if ((rc = decouple_adapter_pair(stream, prec, g, delta_c, delta_m, adapter, s.yc, s.ym, n, Ch, false, s.wpk))) return rc;
    VPX_CHECK_HIP(launch_decouple_stats(s.yc, s.ym, s.stats, B, H * W, Ch, stream));
    VPX_CHECK_HIP(launch_decouple_bwd_pointwise(s.yc, s.ym, s.stats, dvalue, s.dyc, s.dym, B, H * W, Ch, stream));
    if (d_delta_c && d_delta_m) {
        if ((rc = decouple_adapter_pair(stream, prec, g, s.dyc, s.dym, adapter, d_delta_c, d_delta_m, n, Ch, true, s.wpk))) return rc;
    } else {
        if (d_delta_c && (rc = plain_conv(stream, prec, g, s.dyc, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, true, nullptr, d_delta_c, Ch, false, s.wpk))) return rc;
        if (d_delta_m && (rc = plain_conv(stream, prec, g, s.dym, Ch, Ch, adapter, Ch, 1, 1, 1, Ch, true, nullptr, d_delta_m, Ch, false, s.wpk))) return rc;
    }
    if (d_adapter) {
        if (s.dym == s.dyc + n && (((uintptr_t)delta_c ^ (uintptr_t)delta_m) & 15) == 0) {
            // both pairs in ONE launch (the c and m halves are two "time steps"): one weight gradient + reduce instead of two + an add
            if ((rc = plain_wgrad(stream, prec, g, s.dyc, Ch, delta_c, Ch, 1, 1, s.slabs, d_adapter, delta_m, s.slice_cap))) return rc;
        } else {
            if ((rc = plain_wgrad(stream, prec, g, s.dyc, Ch, delta_c, Ch, 1, 1, s.slabs, d_adapter, nullptr, s.slice_cap))) return rc;
            if ((rc = plain_wgrad(stream, prec, g, s.dym, Ch, delta_m, Ch, 1, 1, s.slabs, s.dA2, nullptr, s.slice_cap))) return rc;
            VPX_CHECK_HIP(launch_axpy(d_adapter, s.dA2, (long long)Ch * Ch, stream));
        }
    }
    return VPX_OK;
}
}  // extern "C"
