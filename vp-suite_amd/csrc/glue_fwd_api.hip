// glue_fwd_api.hip — the EF stage glue forward: general conv / transposed conv (stride 1 or 2) + bias + LeakyReLU / ReLU, and its queries
// (include/vpx.h). Host code only: the route of a call is decided once (glue_route); the one workspace slot, the weight pack, has the size
// the route names, in the call and in the size queries; every forward, the backward's adjoint launch included, runs through glue_forward.
#include "vpx_host.h"
using namespace vpx;

namespace {
// ---- first generation: the implicit-GEMM kernel, fp32 or split input -------------------------------------------------------------------
// workgroup form of a glue launch: the 8-wave / 16x16-pixel tile when the grid stays large (pick_mw's rule) and the
// stride-1 halo keeps two such workgroups per CU
int ex_mw(const vpx_conv_desc* d, int Ht, int Wt, int sd) {
    if (d->precision == VPX_PREC_F32 || sd != 1) return 1;
    const int mw = pick_mw(d->N, Ht, Wt, plain_tiles(d->Co), d->precision), segC[1] = {d->Ci};
    return (mw > 1 && !conv_fits_lds(segC, 1, d->kh, d->kw, plain_groups(d->Co), d->precision, mw, sd)) ? 1 : mw;
}

struct Gen1Launch {
    int Ht, Wt, th, tw, sd, oy, ox;   // tile space, kernel taps, input step, halo origin
    const int* tapmap; bool flip;     // the launch's taps in the layer's kernel (null: all of them, in order); flipped taps
    int omap, oys, oyo, oxs, oxo;     // omap: tile (ty, tx) is output pixel (oys * ty + oyo, oxs * tx + oxo)
};
int ex_launch(hipStream_t stream, const vpx_conv_desc* d, const GlueGeo& g, const Gen1Launch& l, const GlueIO& io) {
    const int prec = d->precision, segC[1] = {d->Ci}, ng = plain_groups(d->Co), mw = ex_mw(d, l.Ht, l.Wt, l.sd), src_taps = d->kh * d->kw;
    float* wpk = reinterpret_cast<float*>(io.wpk);
    ConvPlan P{};
    int chunks = 0;
    P.prec = prec;
    P.nstage = build_stages(P.stage, &chunks, segC, 1, l.th * l.tw, pick_stage_channels(segC, 1, l.th, l.tw, ng, prec, mw, l.sd), prec);
    if (P.nstage < 0) { set_error("conv: too many channel stages (Ci=%d)", d->Ci); return VPX_ERR_UNSUPPORTED; }
    PackDesc pd{};
    pd.seg[0] = PackSeg{io.w, (long long)(d->transposed ? d->Co : d->Ci) * src_taps, src_taps, 0, d->Ci};
    memcpy(pd.stage, P.stage, sizeof(ConvStage) * P.nstage);
    pd.nstage = P.nstage; pd.chunks_total = chunks; pd.prec = prec; pd.taps = l.th * l.tw;
    fill_plain_pack(pd, d->Co, 0);
    pd.transposed = d->transposed ? 1 : 0; pd.flip = l.flip ? 1 : 0;
    if (l.tapmap) { pd.src_taps = src_taps; for (int i = 0; i < l.th * l.tw; ++i) pd.tapmap[i] = l.tapmap[i]; }
    if (!io.packed) VPX_CHECK_HIP(launch_pack_weights(pd, wpk, stream));
    P.B = d->N; P.H = l.Ht; P.W = l.Wt; P.kh = l.th; P.kw = l.tw;
    set_plan_tiles(P, mw);
    P.stride = l.sd; P.use_org = 1; P.org_y = l.oy; P.org_x = l.ox; P.Hin = d->H; P.Win = d->W;
    P.nseg = 1;
    P.seg[0] = ConvSeg{reinterpret_cast<const float*>(io.x), (long long)d->H * d->W * d->Ci, d->Ci, d->Ci, io.x_split ? 1 : 0, 0};
    P.chunks_total = chunks; P.a_bytes = conv_a_bytes(P.stage, P.nstage, l.th, l.tw, mw, l.sd); P.wpk = wpk;
    PlainEpiArgs ea{};
    ea.bias = io.bias; ea.Co = d->Co; ea.split = d->Co; ea.ng = ng;
    ea.out0 = io.y; ea.bstride0 = (long long)g.Ho * g.Wo * d->Co; ea.ld0 = d->Co;
    ea.leaky = d->leaky_slope; ea.relu = io.act == VPX_ACT_RELU ? 1 : 0;
    ea.omap = l.omap; ea.oys = l.oys; ea.oyo = l.oyo; ea.oxs = l.oxs; ea.oxo = l.oxo; ea.Wmem = g.Wo;
    ea.sp_out = io.y_split; ea.sp_bstride = (long long)g.Ho * g.Wo * d->Co * 4;
    VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, pd.n_tiles, stream));
    return VPX_OK;
}

int gen1_forward(const vpx_conv_desc* d, const GlueGeo& g, GlueRoute route, const GlueIO& io, hipStream_t stream) {
    Gen1Launch l{};
    l.Ht = g.Ho; l.Wt = g.Wo; l.th = d->kh; l.tw = d->kw; l.oys = l.oxs = 1;
    if (route == GlueRoute::GEN1) { l.sd = d->stride; l.oy = l.ox = -d->pad; return ex_launch(stream, d, g, l, io); }
    l.sd = 1;
    if (route == GlueRoute::GEN1_FLIP) { l.oy = -(d->kh - 1 - d->pad); l.ox = -(d->kw - 1 - d->pad); l.flip = true; return ex_launch(stream, d, g, l, io); }
    GlueIO ph = io; ph.packed = false;   // (each phase packs its own taps)
    l.omap = 1; l.oys = l.oxs = 2;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            const int Ht = (g.Ho - py + 1) / 2, Wt = (g.Wo - px + 1) / 2;
            if (Ht < 1 || Wt < 1) continue;
            const int ky0 = (py + d->pad) & 1, kx0 = (px + d->pad) & 1;
            const int nty = (d->kh - ky0 + 1) / 2, ntx = (d->kw - kx0 + 1) / 2;
            // (no tap feeds this phase: bias (+activation) only — not reachable for k >= 2)
            if (nty < 1 || ntx < 1) { set_error("vpx_conv2d_ex_fwd: kernel too small for stride 2"); return VPX_ERR_UNSUPPORTED; }
            if (nty * ntx > 16) { set_error("vpx_conv2d_ex_fwd: too many taps per phase"); return VPX_ERR_UNSUPPORTED; }
            const int basey = (py + d->pad - ky0) / 2, basex = (px + d->pad - kx0) / 2;
            int tapmap[16];
            for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx)
                    tapmap[ty * ntx + tx] = (ky0 + 2 * (nty - 1 - ty)) * d->kw + (kx0 + 2 * (ntx - 1 - tx));
            l.Ht = Ht; l.Wt = Wt; l.th = nty; l.tw = ntx; l.oy = basey - (nty - 1); l.ox = basex - (ntx - 1); l.tapmap = tapmap; l.oyo = py; l.oxo = px;
            const int rc = ex_launch(stream, d, g, l, ph);
            if (rc != VPX_OK) return rc;
        }
    return VPX_OK;
}

size_t ex_wpk_floats(const vpx_conv_desc* d) {
    // upper bound over the launches this descriptor can produce (full tap set, stride as given)
    ConvStage st[MAX_STAGE];
    int chunks = 0;
    const int segC[1] = {d->Ci}, ng = plain_groups(d->Co), sd = d->transposed ? 1 : d->stride;
    size_t best = 0;
    for (int mw = 1; mw <= 2; ++mw) {  // upper bound over both workgroup forms (their stage sizes differ)
        if (build_stages(st, &chunks, segC, 1, d->kh * d->kw, pick_stage_channels(segC, 1, d->kh, d->kw, ng, d->precision, mw, sd), d->precision) < 0) return 0;
        const size_t b = packed_weight_bytes(plain_tiles(d->Co), chunks, ng, d->precision) / 4 + 1024;
        if (b > best) best = b;
    }
    return best;
}

// ---- the same layers on SPLIT-format input through the schedule-driven K = 32 kernel (convq.hip) -----------------------
// Terms of a layer (see convq.hip): a convolution with stride s reads the s x s sub-images x[s*i + sy, s*j + sx] of its input,
// tap ky of row residue sy = (ky - pad) mod s lands at da = (ky - pad - sy) / s; a transposed convolution computes output phase
// (py, px) = (oy mod s, ox mod s) as a stride-1 correlation over x with the taps ky = (py + pad) mod s (+ s, ...) at
// da = -(ky - py - pad) / s. Sub-positions with a single tap get a zero-weight filler so that their stages span a whole step.
bool exq_problem(const vpx_conv_desc* d, const GlueGeo& g, ConvQProblem& pr) {
    memset(&pr, 0, sizeof(pr));
    if (d->precision != VPX_PREC_BF16X3 || (d->Ci & 15) || d->Ci < 16 || d->Ci / 16 > 60) return false;
    const int s = d->stride, p = d->pad, nst = d->Ci / 16, row = d->W * d->Ci * 4, pix = d->Ci * 4, taps = d->kh * d->kw;
    pr.N = d->N; pr.halo = 2; pr.Co = d->Co; pr.col0 = 0;
    if (taps > 25) return false;
    auto fmod_ = [](int a, int b) { return ((a % b) + b) % b; };
    if (!d->transposed) {
        pr.s_oc = (long long)d->Ci * taps; pr.s_ic = taps;
        pr.H = g.Ho; pr.W = g.Wo;
        pr.nseg = s * s; pr.ngs = 1; pr.phases = 0;
        if (pr.nseg > 4) return false;
        ConvQGroupSet& gs = pr.gs[0];
        gs.nt0 = 0; gs.ntn = 8; gs.nterm = 0;
        int per_seg[4] = {0, 0, 0, 0};
        for (int sy = 0; sy < s; ++sy)
            for (int sx = 0; sx < s; ++sx) {
                const int si = sy * s + sx;
                CQSeg& sg = pr.seg[si];
                sg.sp = nullptr; sg.nT = 1;
                sg.rowpitch = s * row; sg.colpitch = s * pix; sg.org = (sy * d->W + sx) * pix;
                sg.Hs = (d->H - sy + s - 1) / s; sg.Ws = (d->W - sx + s - 1) / s;
                sg.nstage = nst; sg.c0 = 0; pr.seg_wc0[si] = 0;
            }
        for (int ky = 0; ky < d->kh; ++ky)
            for (int kx = 0; kx < d->kw; ++kx) {
                const int sy = fmod_(ky - p, s), sx = fmod_(kx - p, s);
                const int da = (ky - p - sy) / s, db = (kx - p - sx) / s;
                if (da < -1 || da > 1 || db < -1 || db > 1 || gs.nterm >= 30) return false;
                gs.term[gs.nterm++] = ConvQTerm{sy * s + sx, da, db, ky * d->kw + kx};
                ++per_seg[sy * s + sx];
            }
        for (int si = 0; si < pr.nseg; ++si) {
            if (per_seg[si] == 0) return false;   // a sub-image nobody reads (kernel smaller than the stride)
            if (per_seg[si] == 1 && s > 1) {      // filler: the same tap again with zero weights
                for (int k = 0; k < gs.nterm; ++k)
                    if (gs.term[k].seg == si) { ConvQTerm f = gs.term[k]; f.wtap = -1; gs.term[gs.nterm++] = f; break; }
            }
        }
        pr.periodic = s == 1 ? 1 : 0;
    } else {
        pr.s_oc = taps; pr.s_ic = (long long)d->Co * taps;
        pr.nseg = 1;
        CQSeg& sg = pr.seg[0];
        sg.sp = nullptr; sg.nT = 1; sg.rowpitch = row; sg.colpitch = pix; sg.org = 0; sg.Hs = d->H; sg.Ws = d->W; sg.nstage = nst; sg.c0 = 0;
        pr.seg_wc0[0] = 0;
        pr.H = (g.Ho + s - 1) / s; pr.W = (g.Wo + s - 1) / s;
        pr.phases = s == 2 ? 1 : 0;
        pr.ngs = s * s;
        for (int py = 0; py < s; ++py)
            for (int px = 0; px < s; ++px) {
                ConvQGroupSet& gs = pr.gs[py * s + px];
                gs.nt0 = s == 2 ? 2 * (py * 2 + px) : 0; gs.ntn = s == 2 ? 2 : 8; gs.nterm = 0;
                for (int ky = fmod_(py + p, s); ky < d->kh; ky += s)
                    for (int kx = fmod_(px + p, s); kx < d->kw; kx += s) {
                        const int da = -(ky - py - p) / s, db = -(kx - px - p) / s;
                        if (da < -1 || da > 1 || db < -1 || db > 1 || gs.nterm >= 30) return false;
                        gs.term[gs.nterm++] = ConvQTerm{0, da, db, ky * d->kw + kx};
                    }
                if (gs.nterm == 0) return false;
            }
        pr.periodic = s == 1 ? 1 : 0;
    }
    return true;
}

// Which kernel takes a layer on split input (measured, tools/ab_glue.py, ms per 1280 frames, first generation on split input ->
// convq on half tiles): layers with >= 64 output channels — stride-2 convolutions 64 -> 64 at 64x64 0.72 -> 0.60 and 96 -> 96 at
// 32x32 0.32 -> 0.25, stride-2 transposed 4x4 96 -> 96 at 16x16 0.48 -> 0.38 and at 32x32 1.79 -> 1.47 (at 40 frames 0.12 -> 0.04 /
// 0.15 -> 0.06: the phase form is one launch) — but plain convolutions only on grids of >= 256 workgroups (40 frames: 0.045 -> 0.049).
// 3x3 stride-1 layers with 16 output channels (64 -> 16: 0.83 first generation, 1.22 convq) have their own kernel (conv16.hip: 0.41).
bool exq_preferred(const vpx_conv_desc* d, const ConvQProblem& pr) {   // pr: the layer's problem (exq_problem)
    if (convq_wpk_bytes(pr) == 0 || d->Co < 64) return false;
    if (pr.phases) return true;
    const long long wgs = (long long)pr.N * ((pr.W + 15) / 16) * ((pr.H + 15) / 16) * (((d->Co + 31) / 32 + 3) / 4);
    return wgs >= 256;
}

int convq_forward(const vpx_conv_desc* d, const GlueGeo& g, ConvQProblem& pr, const GlueIO& io, hipStream_t stream) {
    for (CQSeg* sg = pr.seg; sg < pr.seg + pr.nseg; ++sg) { sg->sp = reinterpret_cast<const char*>(io.x); sg->bstride = io.x_bstride; sg->tstride = io.x_tstride; sg->nT = io.x_nT > 0 ? io.x_nT : 1; }
    pr.w = io.w;
    ConvQEpiArgs ea{};
    ea.bias = io.bias; ea.leaky = d->leaky_slope; ea.Co = d->Co; ea.split = d->Co;
    const int s = d->transposed ? d->stride : 1;
    ea.oys = s; ea.oxs = s; ea.oyo = 0; ea.oxo = 0; ea.Hmem = g.Ho; ea.Wmem = g.Wo;
    ea.out0 = io.y; ea.bstride0 = (long long)g.Ho * g.Wo * d->Co; ea.ld0 = d->Co;
    ea.sp_out = io.y_split; ea.sp_bstride = (long long)g.Ho * g.Wo * d->Co * 4;
    return convq_run(pr, ea, io.wpk, io.packed, stream);
}

constexpr size_t GLUE_FWD_SLACK = 512;   // beside the pack in every forward query: the carver's start at a 256-byte boundary

// the queries: the route of a layer on the given input form (false: refused, or no route)
bool query_route(const vpx_conv_desc* d, bool x_split, int act, GlueChoice& c) {
    GlueGeo g;
    if (glue_check(d, g) != VPX_OK) return false;
    glue_route(d, g, x_split, act, false, c);
    return c.route != GlueRoute::NONE;
}

// every forward entry point: check, route, size test, carve, run. null_tensor: the caller's own test of the tensors it needs
int glue_fwd_entry(const char* who, const vpx_conv_desc* d, bool null_tensor, GlueIO io, void* workspace, size_t workspace_bytes, void* stream_) {
    GlueGeo g;
    if (int rc = glue_check(d, g)) return rc;
    if (int rc = glue_act_check(d, io.act, who)) return rc;
    if (null_tensor) { set_error("%s: NULL tensor argument", who); return VPX_ERR_ARG; }
    if (io.y_split && (d->Co & 7)) { set_error("%s: the split format needs Co to be a multiple of 8 (got %d)", who, d->Co); return VPX_ERR_UNSUPPORTED; }
    GlueChoice c;
    glue_route(d, g, io.x_split, io.act, io.y_split != nullptr, c);
    if (c.route == GlueRoute::NONE) { set_error("%s: layer not implemented on split input (vpx_conv2d_ex_takes_split)", who); return VPX_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < c.pack_bytes + GLUE_FWD_SLACK) { set_error("%s: workspace too small", who); return VPX_ERR_WORKSPACE; }
    Carver ws(workspace, workspace_bytes);
    io.wpk = reinterpret_cast<char*>(ws.take(c.pack_bytes / sizeof(float)));
    VPX_CHECK_CARVE(ws, who);
    const long long dense = (long long)d->H * d->W * d->Ci * 4;
    if (io.x_bstride == 0) io.x_bstride = dense;
    if (io.x_split && glue_on_gen1(c.route) && (io.x_nT > 1 || io.x_bstride != dense)) { set_error("%s: this layer needs a dense batch of split images", who); return VPX_ERR_UNSUPPORTED; }
    return glue_forward(d, g, c, io, (hipStream_t)stream_);
}
}  // namespace

namespace vpx {
int glue_check(const vpx_conv_desc* d, GlueGeo& g) {
    if (!d) { set_error("conv desc is NULL"); return VPX_ERR_ARG; }
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->Ci < 1 || d->Co < 1 || d->kh < 1 || d->kw < 1 || d->pad < 0) { set_error("conv desc: bad dimension"); return VPX_ERR_ARG; }
    if (d->stride != 1 && d->stride != 2) { set_error("conv desc: stride %d not implemented (1 or 2)", d->stride); return VPX_ERR_UNSUPPORTED; }
    if (d->kh > 7 || d->kw > 7) { set_error("conv desc: kernel larger than 7 not implemented"); return VPX_ERR_UNSUPPORTED; }
    if (d->precision < VPX_PREC_F32 || d->precision > VPX_PREC_BF16) { set_error("conv desc: unknown precision %d", d->precision); return VPX_ERR_UNSUPPORTED; }
    if (!d->transposed) {
        g.Ho = (d->H + 2 * d->pad - d->kh) / d->stride + 1;
        g.Wo = (d->W + 2 * d->pad - d->kw) / d->stride + 1;
    } else {
        if (d->out_pad_h < 0 || d->out_pad_w < 0 || d->out_pad_h >= d->stride || d->out_pad_w >= d->stride) { set_error("conv desc: output padding must be in [0, stride)"); return VPX_ERR_ARG; }
        g.Ho = (d->H - 1) * d->stride - 2 * d->pad + d->kh + d->out_pad_h;
        g.Wo = (d->W - 1) * d->stride - 2 * d->pad + d->kw + d->out_pad_w;
        if (d->stride == 1 && (d->kh - 1 - d->pad < 0 || d->kw - 1 - d->pad < 0)) { set_error("conv desc: padding larger than kernel-1 in a transposed conv"); return VPX_ERR_UNSUPPORTED; }
    }
    if (g.Ho < 1 || g.Wo < 1) { set_error("conv desc: empty output"); return VPX_ERR_ARG; }
    return VPX_OK;
}

// leaky_slope == 0 means "no activation" in the descriptor, so ReLU travels beside it
int glue_act_check(const vpx_conv_desc* d, int act, const char* who) {
    if (act != VPX_ACT_NONE && act != VPX_ACT_RELU) { set_error("%s: unknown activation code %d", who, act); return VPX_ERR_ARG; }
    if (d && act == VPX_ACT_RELU && d->leaky_slope != 0.0f) { set_error("%s: VPX_ACT_RELU with a LeakyReLU slope in the descriptor", who); return VPX_ERR_ARG; }
    return VPX_OK;
}

// The only place that asks the kernels' gates. The streaming kernels read fp32 and know LeakyReLU only (no split input, no activation
// code); kind 2 writes no split output. The first generation reads split input in its bf16 modes, channels in whole groups of 8.
void glue_route(const vpx_conv_desc* d, const GlueGeo& g, bool x_split, int act, bool y_split, GlueChoice& c) {
    c.route = !d->transposed ? GlueRoute::GEN1 : (d->stride == 1 ? GlueRoute::GEN1_FLIP : GlueRoute::GEN1_PHASES);
    c.kind = 0;
    c.pack_bytes = align256(ex_wpk_floats(d) * sizeof(float));
    if (!x_split) {
        c.kind = act ? 0 : conv_small_kind(d);
        if (c.kind && (c.kind != 2 || !y_split)) c.route = GlueRoute::SMALL;
    } else if (c16_applicable(d)) {
        c.route = GlueRoute::C16; c.pack_bytes = align256(c16_wpk_bytes(d));
    } else if (exq_problem(d, g, c.q) && exq_preferred(d, c.q)) {
        c.route = GlueRoute::CONVQ; c.pack_bytes = align256(convq_wpk_bytes(c.q));
    } else if (d->precision == VPX_PREC_F32 || (d->Ci & 7)) {
        c.route = GlueRoute::NONE; c.pack_bytes = 0;
    }
}

int glue_forward(const vpx_conv_desc* d, const GlueGeo& g, GlueChoice& c, const GlueIO& io, hipStream_t stream) {
    switch (c.route) {
    case GlueRoute::SMALL: VPX_CHECK_HIP(launch_conv_small(d, c.kind, reinterpret_cast<const float*>(io.x), io.w, io.bias, io.y, io.y_split, stream)); return VPX_OK;
    case GlueRoute::C16: return c16_forward(d, reinterpret_cast<const char*>(io.x), io.x_bstride, io.x_tstride, io.x_nT, io.w, io.bias, io.y, io.y_split, io.wpk, io.packed, stream);
    case GlueRoute::CONVQ: return convq_forward(d, g, c.q, io, stream);
    case GlueRoute::NONE: set_error("conv: layer not implemented on split input"); return VPX_ERR_UNSUPPORTED;
    default: return gen1_forward(d, g, c.route, io, stream);
    }
}
}  // namespace vpx

extern "C" {
int vpx_conv2d_ex_out_shape(const vpx_conv_desc* d, int* Ho, int* Wo) {
    GlueGeo g;
    if (int rc = glue_check(d, g)) return rc;
    if (Ho) *Ho = g.Ho;
    if (Wo) *Wo = g.Wo;
    return VPX_OK;
}
size_t vpx_conv2d_ex_workspace_bytes(const vpx_conv_desc* d) {
    GlueChoice c;
    return query_route(d, false, VPX_ACT_NONE, c) ? c.pack_bytes + GLUE_FWD_SLACK : 0;
}
size_t vpx_conv2d_act_workspace_bytes(const vpx_conv_desc* d, int act) {
    if (glue_act_check(d, act, "vpx_conv2d_act_workspace_bytes") != VPX_OK) return 0;
    return vpx_conv2d_ex_workspace_bytes(d);
}
// 2: C16 or CONVQ (worth converting an fp32 input for), 1: the first generation, 0: no route on split input
int vpx_conv2d_ex_takes_split(const vpx_conv_desc* d) {
    GlueChoice c;
    if (!query_route(d, true, VPX_ACT_NONE, c)) return 0;
    return glue_on_gen1(c.route) ? 1 : 2;
}
size_t vpx_conv2d_ex_split_workspace_bytes(const vpx_conv_desc* d) {
    GlueChoice c;
    return query_route(d, true, VPX_ACT_NONE, c) ? c.pack_bytes + GLUE_FWD_SLACK : 0;
}
int vpx_conv2d_ex_fwd(const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                      void* workspace, size_t workspace_bytes, void* stream_) {
    GlueIO io{}; io.x = x; io.w = w; io.bias = bias; io.y = y;
    return glue_fwd_entry("vpx_conv2d_ex_fwd", d, !x || !w || !y, io, workspace, workspace_bytes, stream_);
}
int vpx_conv2d_act_fwd(const vpx_conv_desc* d, int act, const float* x, const float* w, const float* bias, float* y, void* workspace,
                       size_t workspace_bytes, void* stream_) {
    GlueIO io{}; io.x = x; io.w = w; io.bias = bias; io.y = y; io.act = act;
    return glue_fwd_entry("vpx_conv2d_act_fwd", d, !x || !w || !y, io, workspace, workspace_bytes, stream_);
}
int vpx_conv2d_ex_fwd_split(const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* y_split,
                            void* workspace, size_t workspace_bytes, void* stream_) {
    GlueIO io{}; io.x = x; io.w = w; io.bias = bias; io.y = y; io.y_split = reinterpret_cast<char*>(y_split);
    return glue_fwd_entry("vpx_conv2d_ex_fwd_split", d, !x || !w || !y_split, io, workspace, workspace_bytes, stream_);
}
int vpx_conv2d_ex_fwd_from_split(const vpx_conv_desc* d, const void* x_split, long long x_bstride, long long x_tstride, int x_nT,
                                 const float* w, const float* bias, float* y, void* y_split, int weights_packed, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
    GlueIO io{}; io.x = x_split; io.x_bstride = x_bstride; io.x_tstride = x_tstride; io.x_nT = x_nT; io.x_split = true;
    io.w = w; io.bias = bias; io.y = y; io.y_split = reinterpret_cast<char*>(y_split); io.packed = weights_packed != 0;
    return glue_fwd_entry("vpx_conv2d_ex_fwd_from_split", d, !x_split || !w || (!y && !y_split), io, workspace, workspace_bytes, stream_);
}
}  // extern "C"
