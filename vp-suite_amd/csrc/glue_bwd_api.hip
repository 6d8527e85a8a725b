// glue_bwd_api.hip — the EF stage glue backward and its queries (include/vpx.h). Host code only: one function plans a call (glue_bwd_plan:
// the data gradient's route, the weight gradient's kernel, who writes the split copy of dy), one lists the workspace slots (carve_glue_bwd)
// for the call's Carver and for the size query's CarveMeasure. d(pre-activation) = dy * act'(y) and db in one pass (launch_colsum); dx = the
// adjoint layer on dy through glue_forward (glue_fwd_api.hip); dw per stride residue (strided_wgrad) or on wgrad_small_kernel.
#include "vpx_host.h"
using namespace vpx;

namespace {
constexpr long long GLUE_SLAB_FLOATS = 4ll << 20;  // K-slice slab budget of the glue weight gradients (16 MB)

// dW[r][c][ky][kx] = sum_{b,y,x} G[b,y,x,r] * A[b, s*y + ky - p, s*x + kx - p, c]   (G: [N,Hg,Wg,Rg], A: [N,Ha,Wa,Ca], NHWC).
// ky - p = s*a + ry: the taps of one residue (ry, rx) slide over the sub-image A[s*i + ry, s*j + rx] with offsets a —
// one stride-1 weight-gradient launch per residue on the MFMA kernel, its taps scattered into dW by the reduce.
// G_sp / A_sp (round 6): both operands once more in the split format — residues with >= 2 taps then run on wgrad2_kernel's glue form
// (LDS-DMA staging, no conversion work in the loop; wgrad2.hip), `slab_floats` = what `slabs` holds.
int strided_wgrad(hipStream_t stream, int prec, int N, int Hg, int Wg, const float* G, int Rg, int Ha, int Wa, const float* A,
                  int Ca, int kh, int kw, int s, int p, float* slabs, float* dW, const char* G_sp, const char* A_sp, size_t slab_floats) {
    auto fdiv = [](int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); };
    for (int ry = 0; ry < s; ++ry)
        for (int rx = 0; rx < s; ++rx) {
            // taps of this residue: ky = ky0, ky0 + s, ...
            int ky0 = ((p + ry) % s + s) % s, kx0 = ((p + rx) % s + s) % s;
            const int nty = ky0 < kh ? (kh - ky0 + s - 1) / s : 0, ntx = kx0 < kw ? (kw - kx0 + s - 1) / s : 0;
            if (nty < 1 || ntx < 1) continue;
            if (nty * ntx > 16 && s != 1) { set_error("conv wgrad: too many taps per residue"); return VPX_ERR_UNSUPPORTED; }
            WgradArgs wa{};
            wa.T = 1; wa.B = N; wa.H = Hg; wa.W = Wg; wa.HW = Hg * Wg; wa.kh = nty; wa.kw = ntx;
            wa.tiles_x = (Wg + TILE_W - 1) / TILE_W; wa.tiles_y = (Hg + TILE_H - 1) / TILE_H;
            wa.N4 = Rg; wa.Cin = Ca; wa.Ch = 1; wa.Ct = Ca; wa.ldG = Rg; wa.n_out = Rg; wa.prec = prec;
            wa.dG = G; wa.x = A; wa.x_bstride = (long long)Ha * Wa * Ca;
            wa.a_sub = 1; wa.a_sy = s; wa.a_sx = s; wa.a_oy = ry; wa.a_ox = rx;
            wa.a_Hs = (Ha - ry + s - 1) / s; wa.a_Ws = (Wa - rx + s - 1) / s; wa.a_Wfull = Wa;
            wa.use_org = 1; wa.org_y = fdiv(ky0 - p - ry, s); wa.org_x = fdiv(kx0 - p - rx, s);
            wa.n_ctiles = wgrad_make_ctiles(wa.ct, WG_MAX_CTILES, Ca, 0, 0);
            if (wa.n_ctiles < 0) { set_error("conv wgrad: too many channels (%d)", Ca); return VPX_ERR_UNSUPPORTED; }
            wa.slabs = slabs;
            const int taps = nty * ntx;
            // K slices: ~1024 workgroups, bounded by the work items and by the slab budget (GLUE_SLAB_FLOATS, or 32 slices
            // when one slice alone is that large). Layers with few rows x channels (1->16, 16->1) get all their
            // parallelism from the slices.
            const long long items = (long long)N * wa.tiles_x * wa.tiles_y;
            const long long per_slice = (long long)taps * Rg * Ca;
            long long cap = GLUE_SLAB_FLOATS / per_slice;
            if (cap < 32) cap = 32;
            int ns = wgrad_pick_slices((int)(cap < items ? cap : items), Rg, wa.n_ctiles, taps);
            WgradArgs wq = wa;
            wq.g_sp = G_sp; wq.x_sp = A_sp; wq.x_sp_bstride = (long long)Ha * Wa * Ca * 4; wq.a_split = 1;
            if (G_sp && A_sp && wgrad2g_applicable(wq)) {
                const long long room = (long long)(slab_floats / (size_t)per_slice);
                VPX_CHECK_HIP(launch_wgrad2g(wq, (int)(room < 1 ? 1 : (room > 4096 ? 4096 : room)), &ns, stream));
            } else
            VPX_CHECK_HIP(launch_wgrad(wa, ns, stream));
            if (s == 1) {
                VPX_CHECK_HIP(launch_wgrad_reduce(slabs, dW, ns, taps, Rg, Ca, stream));
            } else {
                int tapmap[16];
                for (int ty = 0; ty < nty; ++ty)
                    for (int tx = 0; tx < ntx; ++tx) tapmap[ty * ntx + tx] = (ky0 + s * ty) * kw + (kx0 + s * tx);
                VPX_CHECK_HIP(launch_wgrad_reduce_map(slabs, dW, ns, taps, Rg, Ca, kh * kw, tapmap, stream));
            }
        }
    return VPX_OK;
}

// the adjoint layer of d (what maps dy to dx), as a forward descriptor, and its output shape (= d's input)
int ex_adjoint(const vpx_conv_desc* d, const GlueGeo& g, vpx_conv_desc& a, GlueGeo& ga) {
    a = *d;
    a.H = g.Ho; a.W = g.Wo; a.Ci = d->Co; a.Co = d->Ci; a.leaky_slope = 0.0f;
    a.out_pad_h = a.out_pad_w = 0;
    if (!d->transposed) {  // dx = conv_transpose2d(dy, w, stride, pad, output_padding = the rows/cols the forward conv dropped)
        a.transposed = 1;
        a.out_pad_h = (d->H + 2 * d->pad - d->kh) % d->stride;
        a.out_pad_w = (d->W + 2 * d->pad - d->kw) % d->stride;
    } else {               // dx = conv2d(dy, w, stride, pad)
        a.transposed = 0;
    }
    if (glue_check(&a, ga) != VPX_OK) return VPX_ERR_UNSUPPORTED;
    if (ga.Ho != d->H || ga.Wo != d->W) { set_error("conv bwd: adjoint shape %dx%d != input %dx%d", ga.Ho, ga.Wo, d->H, d->W); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

// ---- the plan of a call ------------------------------------------------------------------------------------------------------------------
// The weight gradient's kernel and the K-slice slab space beside it.
//   SMALL     few-channel plain convolutions on wgrad_small_kernel (lstm_bwd.hip), where its partial sums fit the slabs
//   SPLIT     both operands once more in the split format: residues with >= 2 taps on wgrad2_kernel's glue form, the rest on the tap-group
//             kernel — bf16x3 on the 16x16x32 shape, channel counts in whole groups of 8 (VPX_EXP_GLUE_WGRAD_TAPGROUP: never)
//   TAPGROUP  launch_wgrad per residue on fp32 operands
enum class GlueWgrad { SMALL, SPLIT, TAPGROUP };
struct WgradRule { GlueWgrad kernel; size_t slab_floats; };
WgradRule glue_wgrad_rule(const vpx_conv_desc* d) {
    const bool small_shape = !d->transposed && wgrad_small_applicable(d->Co, d->Ci, d->kh, d->kw, d->stride, d->pad);
    const bool split = !exp_on(VPX_EXP_GLUE_WGRAD_TAPGROUP) && d->precision == VPX_PREC_BF16X3 && g_mfma_shape == 1 && (d->Ci & 7) == 0 && (d->Co & 7) == 0 &&
                       d->kh <= 2 * d->stride + 1 && d->kw <= 2 * d->stride + 1 && d->kh * d->kw > 1 && !small_shape;
    // a residue launch uses <= max(32 slices, GLUE_SLAB_FLOATS / slice) slices of <= kh*kw*Ci*Co floats
    const size_t full = (size_t)32 * d->kh * d->kw * d->Ci * d->Co;
    size_t slab = full > (size_t)GLUE_SLAB_FLOATS ? full : (size_t)GLUE_SLAB_FLOATS;
    // the glue form of wgrad2_kernel: up to WGRAD2_TARGET_WGS workgroups = that many slices of ONE row x column tile pair (a residue's slab is
    if (split) {   // at most kh * kw * Ci * Co / stride^2 floats)
        const int rows = ((d->transposed ? d->Ci : d->Co) + 127) / 128, cols = ((d->transposed ? d->Co : d->Ci) + 63) / 64;
        const size_t per = (size_t)((d->kh + d->stride - 1) / d->stride) * ((d->kw + d->stride - 1) / d->stride) * d->Ci * d->Co;
        const size_t need = (size_t)(WGRAD2_TARGET_WGS / (rows * cols) + 1) * per;
        if (need > slab) slab = need;
    }
    const bool small = small_shape && (size_t)WGRAD_SMALL_BLOCKS * d->Co * d->Ci * d->kh * d->kw <= slab;
    return {small ? GlueWgrad::SMALL : (split ? GlueWgrad::SPLIT : GlueWgrad::TAPGROUP), slab};
}

// Round 5: the data gradient of a glue layer = its adjoint layer on dy. Where that adjoint is a layer the schedule-driven K = 32 kernel
// (convq) takes — the forward's rule on split input — it runs THERE, on a split copy of dy (Co in whole groups of 8); else on the adjoint's
// fp32 route. VPX_EXP_GLUE_DGRAD_GEN1 keeps the latter (A/B runs, tests). The split copy of dy, which the SPLIT weight gradient reads as
// well, is written by the pass that scales dy by act' and sums the bias gradient — in launch_colsum's vector form (`vec4`: Co % 4 == 0,
// dy and y 16-byte aligned) — else by one conversion launch before its first reader.
struct GlueBwdPlan {
    vpx_conv_desc a; GlueGeo ga;           // the adjoint layer
    GlueChoice dgrad; size_t wpk_bytes;    // its route; the first generation's pack (carved on every route)
    WgradRule wgrad;
    bool dq, wsp;                          // wanted and on split operands: the data gradient on CONVQ, the weight gradient SPLIT
    bool scale, scale_splits;              // an activation: the scaling pass runs; ... and writes the split copy of dy
    size_t n_dy, n_x;
};
int glue_bwd_plan(const vpx_conv_desc* d, const GlueGeo& g, int act, bool want_dx, bool want_dw, bool vec4, GlueBwdPlan& p) {
    if (int rc = ex_adjoint(d, g, p.a, p.ga)) return rc;
    glue_route(&p.a, p.ga, false, VPX_ACT_NONE, false, p.dgrad);
    p.wpk_bytes = p.dgrad.pack_bytes;
    p.dq = false;
    if (want_dx && !exp_on(VPX_EXP_GLUE_DGRAD_GEN1) && !(d->Co & 7)) {
        GlueChoice q;
        glue_route(&p.a, p.ga, true, VPX_ACT_NONE, false, q);
        if (q.route == GlueRoute::CONVQ) { p.dgrad = q; p.dq = true; }
    }
    p.wgrad = glue_wgrad_rule(d);
    p.wsp = want_dw && p.wgrad.kernel == GlueWgrad::SPLIT;
    p.scale = d->leaky_slope != 0.0f || act == VPX_ACT_RELU;
    p.scale_splits = p.scale && (p.dq || p.wsp) && vec4;
    p.n_dy = (size_t)d->N * g.Ho * g.Wo * d->Co;
    p.n_x = (size_t)d->N * d->H * d->W * d->Ci;
    return VPX_OK;
}

// the workspace: ONE list of slots (a call that wants everything takes them all: what the size query measures)
struct GlueBwdSlots {
    float *wpk, *slabs, *dys, *db_part;   // the adjoint's first-generation pack; K-slice slabs; dy * act'(y); the bias gradient's partial sums
    char *dy_sp, *wpkq, *x_sp;            // dy in the split format; the adjoint's convq pack; x in the split format (unless the caller kept one)
};
template <class WS>
void carve_glue_bwd(WS& ws, const vpx_conv_desc* d, const GlueBwdPlan& p, GlueBwdSlots& s) {
    s.wpk = ws.take(p.wpk_bytes / sizeof(float));
    s.slabs = ws.take(p.wgrad.slab_floats);
    s.dys = ws.take(p.n_dy);
    s.db_part = ws.take((size_t)COLSUM_BLOCKS * d->Co);
    if (p.dq || p.wsp) s.dy_sp = (char*)ws.take(p.n_dy);
    if (p.dq) s.wpkq = (char*)ws.take(p.dgrad.pack_bytes / sizeof(float));
    if (p.wsp) s.x_sp = (char*)ws.take(p.n_x);
}
constexpr size_t GLUE_BWD_SLACK = 1024;

int ex_bwd_impl(const char* who, const vpx_conv_desc* d, int act, const float* x, const void* x_split, const float* w, const float* y,
                const float* dy, float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    GlueGeo g;
    int rc = glue_check(d, g);
    if (rc != VPX_OK) return rc;
    GlueBwdPlan p;
    if ((rc = glue_bwd_plan(d, g, act, dx != nullptr, dw != nullptr, (d->Co & 3) == 0 && (((uintptr_t)dy | (uintptr_t)y) & 15) == 0, p)) != VPX_OK) return rc;
    if (d->kh < d->stride || d->kw < d->stride) { set_error("%s: kernel smaller than the stride", who); return VPX_ERR_UNSUPPORTED; }
    if (!x || !w || !dy) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (!workspace || workspace_bytes < vpx_conv2d_ex_bwd_workspace_bytes(d)) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    hipStream_t stream = (hipStream_t)stream_;
    Carver ws(workspace, workspace_bytes);
    GlueBwdSlots s{};
    carve_glue_bwd(ws, d, p, s);
    VPX_CHECK_CARVE(ws, who);
    const long long npix_dy = (long long)d->N * g.Ho * g.Wo;
    if (p.scale) {
        // d(pre-activation) = dy * act'(.), the derivative read off the sign of the forward OUTPUT (same sign as the
        // pre-activation for a positive slope) — one pass that also yields the bias gradient
        if (!y) { set_error("%s: y (forward output) is required when the layer has an activation", who); return VPX_ERR_ARG; }
        if (d->leaky_slope < 0.0f) { set_error("%s: negative leaky_slope is not implemented", who); return VPX_ERR_UNSUPPORTED; }
        VPX_CHECK_HIP(launch_colsum(dy, y, d->leaky_slope, s.dys, db, s.db_part, npix_dy, d->Co, stream, p.scale_splits ? s.dy_sp : nullptr));
        dy = s.dys;
    } else if (db) VPX_CHECK_HIP(launch_colsum(dy, nullptr, 0.f, nullptr, db, s.db_part, npix_dy, d->Co, stream));
    bool have_sp = p.scale_splits;
    auto split_dy = [&]() { if (have_sp) return hipSuccess; have_sp = true; return launch_split_convert(dy, s.dy_sp, npix_dy, d->Co, stream); };
    if (dx) {
        GlueIO io{};
        io.x = dy; io.w = w; io.y = dx; io.wpk = reinterpret_cast<char*>(s.wpk);
        if (p.dq) {
            VPX_CHECK_HIP(split_dy());
            io.x = s.dy_sp; io.x_split = true; io.x_bstride = (long long)g.Ho * g.Wo * d->Co * 4; io.x_nT = 1; io.wpk = s.wpkq;
        }
        if ((rc = glue_forward(&p.a, p.ga, p.dgrad, io, stream)) != VPX_OK) return rc;
    }
    if (dw && p.wgrad.kernel == GlueWgrad::SMALL) {
        VPX_CHECK_HIP(launch_wgrad_small(dy, x, d->N, d->H, d->W, d->Co, d->Ci, d->kh, d->pad, s.slabs, dw, stream));
    } else if (dw) {
        const char* x_sp = nullptr;
        if (p.wsp) {
            VPX_CHECK_HIP(split_dy());
            if (x_split) x_sp = reinterpret_cast<const char*>(x_split);   // the caller kept the forward's copy
            else { VPX_CHECK_HIP(launch_split_convert(x, s.x_sp, (long long)d->N * d->H * d->W, d->Ci, stream)); x_sp = s.x_sp; }
        }
        const char* dy_sp = p.wsp ? s.dy_sp : nullptr;
        if (!d->transposed)  // dW[co][ci][ky][kx] = sum dy[b,oy,ox,co] x[b, s*oy + ky - p, s*ox + kx - p, ci]
            rc = strided_wgrad(stream, d->precision, d->N, g.Ho, g.Wo, dy, d->Co, d->H, d->W, x, d->Ci, d->kh, d->kw, d->stride, d->pad, s.slabs, dw,
                               dy_sp, x_sp, p.wgrad.slab_floats);
        else                 // dW[ci][co][ky][kx] = sum x[b,i,j,ci] dy[b, s*i + ky - p, s*j + kx - p, co]
            rc = strided_wgrad(stream, d->precision, d->N, d->H, d->W, x, d->Ci, g.Ho, g.Wo, dy, d->Co, d->kh, d->kw, d->stride, d->pad, s.slabs, dw,
                               x_sp, dy_sp, p.wgrad.slab_floats);
        if (rc != VPX_OK) return rc;
    }
    return VPX_OK;
}
}  // namespace

extern "C" {
size_t vpx_conv2d_ex_bwd_workspace_bytes(const vpx_conv_desc* d) {
    GlueGeo g; GlueBwdPlan p;
    if (glue_check(d, g) != VPX_OK || glue_bwd_plan(d, g, VPX_ACT_NONE, true, true, true, p) != VPX_OK) return 0;
    CarveMeasure m; GlueBwdSlots s{};
    carve_glue_bwd(m, d, p, s);
    return m.off + GLUE_BWD_SLACK;
}
size_t vpx_conv2d_act_bwd_workspace_bytes(const vpx_conv_desc* d, int act) {
    if (glue_act_check(d, act, "vpx_conv2d_act_bwd_workspace_bytes") != VPX_OK) return 0;
    return vpx_conv2d_ex_bwd_workspace_bytes(d);
}
int vpx_conv2d_ex_bwd_uses_split(const vpx_conv_desc* d) {
    GlueGeo g;
    if (!d || glue_check(d, g) != VPX_OK) return 0;
    return glue_wgrad_rule(d).kernel == GlueWgrad::SPLIT ? 1 : 0;
}
int vpx_conv2d_ex_bwd(const vpx_conv_desc* d, const float* x, const float* w, const float* y, const float* dy, float* dx,
                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    return ex_bwd_impl("vpx_conv2d_ex_bwd", d, VPX_ACT_NONE, x, nullptr, w, y, dy, dx, dw, db, workspace, workspace_bytes, stream_);
}
int vpx_conv2d_ex_bwd_ex(const vpx_conv_desc* d, const float* x, const void* x_split, const float* w, const float* y, const float* dy, float* dx,
                         float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    return ex_bwd_impl("vpx_conv2d_ex_bwd", d, VPX_ACT_NONE, x, x_split, w, y, dy, dx, dw, db, workspace, workspace_bytes, stream_);
}
/* ReLU' is read off the saved output (y > 0: zero at y == 0, as torch's threshold backward for finite dy) in the pass that sums the bias
 * gradient. That pass multiplies dy by the 0 / 1 derivative (launch_colsum, shared with LeakyReLU): a non-finite dy at a dead unit
 * gives NaN where torch's select gives 0. */
int vpx_conv2d_act_bwd(const vpx_conv_desc* d, int act, const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw,
                       float* db, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = glue_act_check(d, act, "vpx_conv2d_act_bwd")) return rc;
    return ex_bwd_impl("vpx_conv2d_act_bwd", d, act, x, nullptr, w, y, dy, dx, dw, db, workspace, workspace_bytes, stream_);
}
}  // extern "C"
