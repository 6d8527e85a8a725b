// stlstm_api.hip — vpx_stlstm_step_fwd / _bwd: one Spatio-Temporal LSTM cell step (predrnn.py:57-83) as four launches of
// the implicit-GEMM kernel:
//   c group   conv([x|h]; Wx rows i,f,g,o + Wh rows i,f,g,o)  -> c_new, delta_c, o_pre           (fused gates)
//   m group   conv([x|m]; Wx rows i',f',g' + Wm rows i,f,g)   -> m_new, delta_m                  (fused gates)
//   conv_last 1x1 over mem = [c_new|m_new]                    -> lc
//   conv_o    kxk over mem, epilogue h_new = sigmoid(o_pre + conv_o) * tanh(lc)
// The LayerNorm variant (predrnn.py:24-40) runs unfused, on plain convolutions and LayerNorm kernels (stlstm_ln_api.hip).
// Host code only: the route of a call is decided once (st_route, st_choice), one function carves the workspace for the call and for the
// size query (carve_st_fwd), the reserve has one layout (stlstm_reserve, vpx_host.h), each route has its own functions.
#include "vpx_host.h"

using namespace vpx;

namespace {

// ---- the route of a call: which kernels take the four launches ----
enum class STRoute {
    LN,     // LayerNorm variant: separate plain convolutions, LayerNorm and pointwise gate kernels (stlstm_ln_api.hip)
    GEN1,   // first generation: dual gate launch, conv_last, conv_o fused with the output gate or K-split + pointwise
    C5,     // gate groups and conv_o on the 16x16-tile kernel over split-format operands (convq.hip)
    C5K,    // ... K-split on small grids: every K chunk a job writing partial sums, pointwise kernels add them and apply the gates
};

struct STLayout {
    int taps, tiles32, tiles128, ng_l, ksplit_l;
    int mw_g, mw_o;               // workgroup form of the dual gate launch / the conv_o launch (2: 8 waves, 16x16 pixels)
    int o_split, o_ng, o_tiles;   // conv_o as a K-split plain conv accumulating into o_pre (small maps) instead of the fused launch
    int nstage_g, chunks_g;            // gate groups: segments (x: Cin, recurrent: Ch), k x k
    ConvStage stage_g[MAX_STAGE];
    int nstage_o, chunks_o;            // conv_o: segments (c_new: Ch, m_new: Ch), k x k
    ConvStage stage_o[MAX_STAGE];
    int nstage_l, chunks_l;            // conv_last: same segments, 1 x 1
    ConvStage stage_l[MAX_STAGE];
    size_t n_state, n_x;
    size_t wpk_c, wpk_m, wpk_o, wpk_l;  // float counts
    STRoute route; size_t c5_wc, c5_wm, c5_wo;   // C5: bytes of its weight packs
    int ks_g, ks_o, nt_o; size_t k_wc[6], k_wm[6], k_wo[6];   // C5K: chunks of the gate groups / of conv_o, conv_o's N-tile width, bytes of the chunk packs
};
// conv_o on c5: 64-column N tiles, or 32-column ones when those would leave the chip half empty (B = 128 on 16x16 maps, Ch = 128: 256
// workgroups of four waves = one wave per SIMD; 512 at 32 columns)
static inline int c5f_nt_o(const vpx_stlstm_desc* d) {
    const long long mt = (long long)d->B * ((d->H + 15) / 16) * ((d->W + 15) / 16);
    return mt * ((d->Ch + 63) / 64) < 384 ? 2 : 4;
}

// VPX_EXP_ST_FWD_GEN1 keeps the first-generation forward launches (A/B runs, tests)
// Grid rule (measured, tools/ab_predrnn.py, predrnn-pp inference, ms per forward c5 vs first generation): 16x16 maps B = 8 / 16 / 32 / 64 /
// 128: 23.5 / 23.7 / 24.4 / 30.5 / 53.8 vs 13.7 / 14.1 / 17.1 / 26.9 / 58.5; 32x32 maps (128x128x3, 4 layers, 10 -> 30) B = 4 / 8 / 16:
// 72.5 / 78.1 / 90.9 vs 45.0 / 53.0 / 83.5 — a c5 workgroup runs its whole K (200 steps of 96 MFMAs) on one CU, the first generation
// splits K over workgroups when the pixel tiles do not fill the chip. c5 from 96 pixel tiles of 16x16 on — first pass of round 4. After the
// K loop's diet (convq.hip) the unsplit form wins from 48 tiles on against its own K-split job forms (ab_c5_min.sh, removed with the developer build; 16x16 maps,
// ms per forward unsplit vs K-split: B = 40 30.2 vs 28.9, 48 30.7 vs 33.2, 56 32.1 vs 34.7, 64 33.5 vs 36.2, 80 47.1 vs 50.4); the backward
// launches keep 96 (training step B = 48 221 vs 211 ms, 64 246 vs 242, 80 309.5 vs 309.1).
static bool c5_shape_ok(const vpx_stlstm_desc* d) {
    return d->k == 5 && d->precision == VPX_PREC_BF16X3 && !(d->Ch & 31) && !(d->Cin & 7) && !d->layer_norm && !exp_on(VPX_EXP_ST_FWD_GEN1);
}
constexpr int C5_MIN_TILES = 48;
bool c5_fwd_applicable(const vpx_stlstm_desc* d) {
    const long long mt = (long long)d->B * ((d->H + 15) / 16) * ((d->W + 15) / 16);
    return c5_shape_ok(d) && (mt >= C5_MIN_TILES || exp_on(VPX_EXP_C5_UNSPLIT));   // (VPX_EXP_C5_UNSPLIT forces the unsplit form on small grids: tests)
}
// below the bar: K-split jobs (VPX_EXP_C5_NO_KSPLIT keeps the first-generation launches there)
bool c5k_fwd_applicable(const vpx_stlstm_desc* d) { return c5_shape_ok(d) && !c5_fwd_applicable(d) && !exp_on(VPX_EXP_C5_NO_KSPLIT); }
// K chunks so that the launch has about 448 workgroups, every chunk at least four 8-channel stages (25 steps), at most six chunks
static int c5k_chunks(long long wgs1, int S8) {
    constexpr long long C5K_TARGET = 448;   // workgroups the chunked launch aims at
    int ks = (int)((C5K_TARGET + wgs1 / 2) / (wgs1 > 0 ? wgs1 : 1));
    if (ks > S8 / 4) ks = S8 / 4;
    if (ks > 6) ks = 6;
    return ks < 1 ? 1 : ks;
}
// The only reader of the applicability predicates.
static STRoute st_route(const vpx_stlstm_desc* d) {
    if (d->layer_norm) return STRoute::LN;
    if (c5_fwd_applicable(d)) return STRoute::C5;
    return c5k_fwd_applicable(d) ? STRoute::C5K : STRoute::GEN1;
}

int check_st_desc(const vpx_stlstm_desc* d) {
    if (!d) { set_error("stlstm desc is NULL"); return VPX_ERR_ARG; }
    if (d->B < 1 || d->Cin < 1 || d->Ch < 1 || d->H < 1 || d->W < 1) { set_error("stlstm desc: non-positive dimension"); return VPX_ERR_ARG; }
    if (d->k < 1 || !(d->k & 1) || d->k > 7) { set_error("stlstm desc: filter size must be odd and <= 7 (got %d)", d->k); return VPX_ERR_ARG; }
    if (d->layout != VPX_LAYOUT_NHWC && d->layout != VPX_LAYOUT_NCHW) { set_error("stlstm desc: unknown layout %d", d->layout); return VPX_ERR_ARG; }
    if ((d->precision < VPX_PREC_F32 || d->precision > VPX_PREC_BF16)) { set_error("stlstm: precision %d not implemented", d->precision); return VPX_ERR_UNSUPPORTED; }
    return VPX_OK;
}

int st_layout(const vpx_stlstm_desc* d, STLayout& L) {
    L.taps = d->k * d->k;
    L.tiles32 = (d->Ch + 31) / 32;
    L.ng_l = plain_groups(d->Ch, (long long)d->B * ((d->H + TILE_H - 1) / TILE_H) * ((d->W + TILE_W - 1) / TILE_W));
    L.tiles128 = plain_tiles_ng(d->Ch, L.ng_l);
    const int segG[2] = {d->Cin, d->Ch};
    const int segO[2] = {d->Ch, d->Ch};
    L.mw_g = d->layer_norm ? 1 : pick_mw(d->B, d->H, d->W, 2 * L.tiles32, d->precision);
    if (L.mw_g > 1 && !conv_fits_lds(segG, 2, d->k, d->k, 4, d->precision, L.mw_g)) L.mw_g = 1;   // (8-wave form too large for LDS)
    L.nstage_g = build_stages(L.stage_g, &L.chunks_g, segG, 2, L.taps, pick_stage_channels(segG, 2, d->k, d->k, 4, d->precision, L.mw_g), d->precision);
    const long long m_tiles = (long long)d->B * ((d->H + TILE_H - 1) / TILE_H) * ((d->W + TILE_W - 1) / TILE_W);
    // conv_o: fused with the output gate (32 channels per workgroup) when that fills the chip; on small maps a 128-wide
    // K-split plain convolution adds conv_o(mem) into o_pre and a pointwise kernel applies the gate
    L.o_ng = 1; L.o_tiles = L.tiles32; L.o_split = 0;
    if (m_tiles * L.tiles32 < 384 && !d->layer_norm) {
        const int ng = plain_groups(d->Ch);
        ConvStage st[MAX_STAGE];
        int ch = 0;
        const int ns = build_stages(st, &ch, segO, 2, L.taps, pick_stage_channels(segO, 2, d->k, d->k, ng, d->precision), d->precision);
        const int ks = ns > 0 ? pick_ksplit(m_tiles * plain_tiles_ng(d->Ch, ng), ns) : 1;
        if (ks > 1) { L.o_split = ks; L.o_ng = ng; L.o_tiles = plain_tiles_ng(d->Ch, ng); }
    }
    L.mw_o = d->layer_norm ? 1 : pick_mw(d->B, d->H, d->W, L.o_tiles, d->precision);
    if (L.mw_o > 1 && !conv_fits_lds(segO, 2, d->k, d->k, L.o_ng, d->precision, L.mw_o)) L.mw_o = 1;
    if (!conv_fits_lds(segG, 2, d->k, d->k, 4, d->precision, L.mw_g) || !conv_fits_lds(segO, 2, d->k, d->k, L.o_ng, d->precision, L.mw_o)) {
        set_error("stlstm: %dx%d kernel over %d+%d channels does not fit the kernel's LDS stages", d->k, d->k, d->Cin, d->Ch);
        return VPX_ERR_UNSUPPORTED;
    }
    L.nstage_o = build_stages(L.stage_o, &L.chunks_o, segO, 2, L.taps, pick_stage_channels(segO, 2, d->k, d->k, L.o_ng, d->precision, L.mw_o), d->precision);
    L.nstage_l = build_stages(L.stage_l, &L.chunks_l, segO, 2, 1, pick_stage_channels(segO, 2, 1, 1, L.ng_l, d->precision), d->precision);
    if (L.nstage_g < 0 || L.nstage_o < 0 || L.nstage_l < 0) { set_error("stlstm: too many channel stages"); return VPX_ERR_UNSUPPORTED; }
    L.n_state = (size_t)d->B * d->H * d->W * d->Ch;
    L.n_x = (size_t)d->B * d->H * d->W * d->Cin;
    L.wpk_c = packed_weight_bytes(L.tiles32, L.chunks_g, 4, d->precision) / 4;
    L.wpk_m = packed_weight_bytes(L.tiles32, L.chunks_g, 3, d->precision) / 4;
    L.wpk_o = packed_weight_bytes(L.o_tiles, L.chunks_o, L.o_ng, d->precision) / 4;
    L.wpk_l = packed_weight_bytes(L.tiles128, L.chunks_l, L.ng_l, d->precision) / 4;
    L.ksplit_l = pick_ksplit(m_tiles * L.tiles128, L.nstage_l);
    L.route = st_route(d);
    L.ks_g = L.ks_o = L.nt_o = 0;   // (C5K only)
    if (L.route == STRoute::C5) {
        L.c5_wc = align256(c5_wpk_bytes(d->Cin + d->Ch, d->Ch, 8, 4));
        L.c5_wm = align256(c5_wpk_bytes(d->Cin + d->Ch, d->Ch, 8, 3));
        L.c5_wo = align256(c5_wpk_bytes(2 * d->Ch, d->Ch, c5f_nt_o(d)));
    }
    if (L.route == STRoute::C5K) {
        const long long mt = (long long)d->B * ((d->H + 15) / 16) * ((d->W + 15) / 16);
        L.ks_g = c5k_chunks(mt * ((7 * d->Ch + 127) / 128), (d->Cin + d->Ch) / 8);
        L.nt_o = mt * ((d->Ch + 63) / 64) * 6 < 320 ? 2 : 4;
        L.ks_o = c5k_chunks(mt * ((d->Ch + L.nt_o * 16 - 1) / (L.nt_o * 16)), 2 * d->Ch / 8);
        for (int k = 0; k < L.ks_g; ++k) {
            L.k_wc[k] = align256(c5_chunk_wpk_bytes(d->Cin + d->Ch, k, L.ks_g, 4 * d->Ch, 8));
            L.k_wm[k] = align256(c5_chunk_wpk_bytes(d->Cin + d->Ch, k, L.ks_g, 3 * d->Ch, 8));
        }
        for (int k = 0; k < L.ks_o; ++k) L.k_wo[k] = align256(c5_chunk_wpk_bytes(2 * d->Ch, k, L.ks_o, d->Ch, L.nt_o));
    }
    return VPX_OK;
}

ConvPlan base_plan(const vpx_stlstm_desc* d, int k) {
    ConvPlan P{};
    P.prec = d->precision;
    P.B = d->B; P.H = d->H; P.W = d->W; P.kh = k; P.kw = k;
    P.tiles_x = (d->W + TILE_W - 1) / TILE_W;
    P.tiles_y = (d->H + TILE_H - 1) / TILE_H;
    return P;
}

}  // namespace

namespace vpx {
STSplitShadows st_shadows_of(const vpx_stlstm_shadows* p) {
    STSplitShadows s{};
    if (!p) return s;
    for (int i = 0; i < 5; ++i) s.in[i] = reinterpret_cast<const char*>(p->in[i]);
    for (int i = 0; i < 3; ++i) s.out[i] = reinterpret_cast<char*>(p->out[i]);
    s.dg8 = reinterpret_cast<char*>(p->dg8_out);
    s.set = 1;
    return s;
}
}  // namespace vpx

namespace {

// o_split: GEN1's conv_o as a K-split plain convolution + pointwise gate (0: fused with the gate); last_split: conv_last reads the split
// copies of c_new / m_new the gate stage left (VPX_EXP_ST_LAST_FP32 keeps the fp32 sources: tests, A/B); nt_o: conv_o's N-tile width on C5 / C5K
struct STRouteChoice { STRoute route; int o_split; bool last_split; int nt_o; };
bool on_c5(STRoute r) { return r == STRoute::C5 || r == STRoute::C5K; }
STRouteChoice st_choice(const vpx_stlstm_desc* d, const STLayout& L) {
    if (on_c5(L.route)) return {L.route, 0, !exp_on(VPX_EXP_ST_LAST_FP32), L.route == STRoute::C5 ? c5f_nt_o(d) : L.nt_o};
    return {L.route, L.route == STRoute::GEN1 ? L.o_split : 0, false, 0};
}

// ---- the forward workspace: its slots in the order they are taken (see CarveMeasure, vpx_host.h) ----
struct STFwdSlots {
    float *wpk_c, *wpk_m, *wpk_o, *wpk_l, *o_pre, *lc;   // first-generation packs (conv_last's serves every route); o pre-activation, conv_last
    char *c5wc, *c5wm, *c5wo;                            // C5: packs of the two gate groups and of conv_o
    char *kwc[6], *kwm[6], *kwo[6];                      // C5K: their chunk packs
    char *x_sp, *h_sp, *m_sp, *cn_sp, *mn_sp;            // C5, C5K: operands in the split format (a shadow of the caller's replaces its slot)
    float *part_g, *part_o;                              // C5K: partial sums of the gate groups (7Ch per chunk) / of conv_o (Ch per chunk)
    STStage nchw;                                        // h, c, m and the five outputs
};
template <class WS>
void carve_st_fwd(WS& ws, const vpx_stlstm_desc* d, const STLayout& L, const STRouteChoice& r, STFwdSlots& s) {
    s.wpk_c = ws.take(L.wpk_c); s.wpk_m = ws.take(L.wpk_m); s.wpk_o = ws.take(L.wpk_o); s.wpk_l = ws.take(L.wpk_l);
    s.o_pre = ws.take(L.n_state); s.lc = ws.take(L.n_state);
    if (r.route == STRoute::C5) {
        s.c5wc = (char*)ws.take(L.c5_wc / 4); s.c5wm = (char*)ws.take(L.c5_wm / 4); s.c5wo = (char*)ws.take(L.c5_wo / 4);
    }
    if (r.route == STRoute::C5K) {
        for (int k = 0; k < L.ks_g; ++k) { s.kwc[k] = (char*)ws.take(L.k_wc[k] / 4); s.kwm[k] = (char*)ws.take(L.k_wm[k] / 4); }
        for (int k = 0; k < L.ks_o; ++k) s.kwo[k] = (char*)ws.take(L.k_wo[k] / 4);
    }
    if (on_c5(r.route)) {
        s.x_sp = (char*)ws.take(L.n_x);
        for (char** p : {&s.h_sp, &s.m_sp, &s.cn_sp, &s.mn_sp}) *p = (char*)ws.take(L.n_state);
    }
    if (r.route == STRoute::C5K) { s.part_g = ws.take((size_t)L.ks_g * 7 * L.n_state); s.part_o = ws.take((size_t)L.ks_o * L.n_state); }
    carve_st_stage(ws, d, L.n_x, L.n_state, false, 8, s.nchw);   // 8 = the 3 inputs + 5 outputs the entry point lists for st_stage_in
}
// ---- what every route's functions see of a call ----
struct STFwdCtx {
    const vpx_stlstm_desc* d; const STLayout* L; STRouteChoice r;
    STFwdTensors t;       // native layout (NHWC): the caller's tensors or their staged copies
    STFwdSlots ws;
    STReserve res;        // all null unless the call saves for the backward
    STSplitShadows sh;    // an argument of THIS call (NHWC only): nothing survives it, nothing precedes it
    hipStream_t stream; size_t HW; long long npix;
    bool packed;          // the caller vouches the workspace still holds every weight pack
};

// ---- pieces shared by the routes ----
// conv_last's first-generation pack: Wlast [Ch, 2Ch, 1, 1] (used when the streaming form does not apply)
int pack_conv_last(const STFwdCtx& c) {
    if (c.packed) return VPX_OK;
    const STLayout& L = *c.L; const int Ch = c.d->Ch;
    PackDesc pl{};
    pl.seg[0] = PackSeg{c.t.Wlast, (long long)2 * Ch, 1, 0, Ch};
    pl.seg[1] = PackSeg{c.t.Wlast, (long long)2 * Ch, 1, Ch, Ch};
    memcpy(pl.stage, L.stage_l, sizeof(ConvStage) * L.nstage_l);
    pl.nstage = L.nstage_l; pl.chunks_total = L.chunks_l; pl.prec = c.d->precision; pl.taps = 1;
    fill_plain_pack(pl, Ch, 0, L.ng_l);
    VPX_CHECK_HIP(launch_pack_weights(pl, c.ws.wpk_l, c.stream));
    return VPX_OK;
}
// C5, C5K: operands a previous call left in the split format come back as shadows; the others are converted here. cp: a plan over x | h | m
int split_operands(STFwdCtx& c, C5Plan& cp) {
    STFwdSlots& s = c.ws; const int Cin = c.d->Cin, Ch = c.d->Ch;
    if (c.sh.in[0]) s.x_sp = const_cast<char*>(c.sh.in[0]); else VPX_CHECK_HIP(launch_split_convert(c.t.x, s.x_sp, c.npix, Cin, c.stream));
    if (c.sh.in[1]) s.h_sp = const_cast<char*>(c.sh.in[1]); else VPX_CHECK_HIP(launch_split_convert(c.t.h, s.h_sp, c.npix, Ch, c.stream));
    if (c.sh.in[2]) s.m_sp = const_cast<char*>(c.sh.in[2]); else VPX_CHECK_HIP(launch_split_convert(c.t.m, s.m_sp, c.npix, Ch, c.stream));
    if (c.sh.out[1]) s.cn_sp = c.sh.out[1];
    if (c.sh.out[2]) s.mn_sp = c.sh.out[2];
    cp = c5_plan_of(c.d->B, c.d->H, c.d->W);
    cp.src[0] = C5Src{s.x_sp, (long long)c.HW * Cin * 4, Cin * 4, 0};
    cp.src[1] = C5Src{s.h_sp, (long long)c.HW * Ch * 4, Ch * 4, 0};
    cp.src[2] = C5Src{s.m_sp, (long long)c.HW * Ch * 4, Ch * 4, 0};
    return VPX_OK;
}
// the K ranges of gate group grp (0: c group (i,f,g,o_pre) from [x | h]; 1: m group (i',f',g') from [x | m]) and the weight rows they multiply
void gate_group_job(const STFwdCtx& c, int grp, C5Job& j, C5PackRange pr[2]) {
    const int Cin = c.d->Cin, Ch = c.d->Ch, taps = c.L->taps;
    const long long ws_x = (long long)Cin * taps, ws_h = (long long)Ch * taps;   // weight strides of one output channel
    j = C5Job{};
    j.nrange = 2;
    j.r_src[0] = 0; j.r_c0[0] = 0; j.r_n[0] = Cin;
    j.r_src[1] = grp ? 2 : 1; j.r_c0[1] = 0; j.r_n[1] = Ch;
    // x rows: (i,f,g,o) = blocks 0,1,2,6 of Wx, (i',f',g') = blocks 3,4,5 (predrnn.py:61); recurrent rows: blocks 0.. of Wh / Wm (:62-63)
    if (grp == 0) pr[0] = C5PackRange{c.t.Wx, ws_x, (long long)taps, 0, {0, Ch, 2 * Ch, 6 * Ch}};
    else pr[0] = C5PackRange{c.t.Wx, ws_x, (long long)taps, 0, {3 * Ch, 4 * Ch, 5 * Ch, 0}};
    pr[1] = C5PackRange{grp ? c.t.Wm : c.t.Wh, ws_h, (long long)taps, 0, {0, Ch, 2 * Ch, 3 * Ch}};
}
// conv_o over mem = [c_new | m_new] in the split format: the plan's sources, the job's K ranges and Wo's columns
void conv_o_job(const STFwdCtx& c, C5Plan& cp, C5Job& j, C5PackRange pr[2]) {
    const int Ch = c.d->Ch, taps = c.L->taps;
    cp = c5_plan_of(c.d->B, c.d->H, c.d->W);
    cp.src[0] = C5Src{c.ws.cn_sp, (long long)c.HW * Ch * 4, Ch * 4, 0};
    cp.src[1] = C5Src{c.ws.mn_sp, (long long)c.HW * Ch * 4, Ch * 4, 0};
    j = C5Job{};
    j.nrange = 2;
    j.r_src[0] = 0; j.r_c0[0] = 0; j.r_n[0] = Ch;
    j.r_src[1] = 1; j.r_c0[1] = 0; j.r_n[1] = Ch;
    const long long so = (long long)2 * Ch * taps;
    pr[0] = C5PackRange{c.t.Wo, so, (long long)taps, 0, {0, 0, 0, 0}};
    pr[1] = C5PackRange{c.t.Wo, so, (long long)taps, Ch, {0, 0, 0, 0}};
}
// a first-generation plan over mem = [c_new | m_new] in fp32
ConvPlan mem_plan(const STFwdCtx& c, int k) {
    const int Ch = c.d->Ch;
    ConvPlan P = base_plan(c.d, k);
    P.nseg = 2;
    P.seg[0] = ConvSeg{c.t.out[1], (long long)(c.HW * Ch), Ch, 0};
    P.seg[1] = ConvSeg{c.t.out[2], (long long)(c.HW * Ch), Ch, 0};
    return P;
}

// ---- C5 and C5K: launches 1 + 2 (the two gate groups as the jobs of one launch) and 4 (conv_o + output gate). C5K: every job K-split into
// ks_g / ks_o chunk jobs writing partial sums, then the pointwise kernel that adds them and applies the gates ----
int c5_gates(STFwdCtx& c) {
    const STFwdSlots& s = c.ws; const STLayout& L = *c.L; const int Ch = c.d->Ch; const bool ks = c.r.route == STRoute::C5K;
    C5Plan cp;
    int rc = split_operands(c, cp);
    for (int grp = 0; grp < 2 && !rc; ++grp) {
        C5Job full;
        C5PackRange prf[2], pr[3];
        gate_group_job(c, grp, full, prf);
        if (!ks) {
            full.epi = 1; full.Co = Ch; full.Ch = Ch; full.ng = grp ? 3 : 4; full.fbias = 1.0f;
            full.wpk = grp ? s.c5wm : s.c5wc;
            full.e_in0 = grp ? c.t.m : c.t.c;
            full.e_out[0] = c.t.out[grp ? 2 : 1]; full.e_out[1] = c.t.out[grp ? 4 : 3]; full.e_out[2] = grp ? nullptr : s.o_pre; full.e_out[3] = grp ? c.res.gates_m : c.res.gates_c;
            full.e_sp = grp ? s.mn_sp : s.cn_sp;
            rc = c5_prepare_job(cp.job[cp.njobs++] = full, 8, prf, grp ? 3 : 4, 0, c.packed, c.stream);
            continue;
        }
        full.epi = 0; full.Co = (grp ? 3 : 4) * Ch; full.ld = 7 * Ch; full.accumulate = 0;
        full.out_bstride = (long long)c.HW * 7 * Ch;
        for (int kk = 0; kk < L.ks_g && !rc; ++kk) {
            C5Job& j = cp.job[cp.njobs++];
            c5_chunk_job(full, prf, kk, L.ks_g, j, pr);
            j.wpk = grp ? s.kwm[kk] : s.kwc[kk];
            j.out = s.part_g + (size_t)kk * 7 * L.n_state + (grp ? 4 * Ch : 0);
            rc = c5_prepare_job(j, 8, pr, grp ? 3 : 4, 0, c.packed, c.stream, 1);
        }
    }
    if (rc) return rc;
    VPX_CHECK_HIP(launch_c5(cp, 8, c.stream));
    if (ks) {
        STGatesKSArgs ga{};
        ga.npix = c.npix; ga.Ch = Ch; ga.ks = L.ks_g; ga.pstride = (long long)(7 * L.n_state); ga.fbias = 1.0f;
        ga.part = s.part_g; ga.c = c.t.c; ga.m = c.t.m;
        ga.c_new = c.t.out[1]; ga.m_new = c.t.out[2]; ga.delta_c = c.t.out[3]; ga.delta_m = c.t.out[4]; ga.o_pre = s.o_pre;
        ga.gates_c = c.res.gates_c; ga.gates_m = c.res.gates_m; ga.cn_sp = s.cn_sp; ga.mn_sp = s.mn_sp;
        VPX_CHECK_HIP(launch_st_gates_ks(ga, c.stream));
    }
    return pack_conv_last(c);
}
int c5_out(const STFwdCtx& c) {
    const STFwdSlots& s = c.ws; const STLayout& L = *c.L; const int Ch = c.d->Ch; const bool ks = c.r.route == STRoute::C5K;
    C5Plan cp;
    C5Job full;
    C5PackRange prf[2], pr[3];
    conv_o_job(c, cp, full, prf);
    int rc = VPX_OK;
    if (!ks) {
        full.epi = 2; full.Co = Ch; full.Ch = Ch; full.wpk = s.c5wo;
        full.e_in0 = s.o_pre; full.e_in1 = s.lc;
        full.e_out[0] = c.t.out[0]; full.e_out[1] = c.res.o; full.e_out[2] = c.res.tl;
        full.e_sp = c.sh.out[0];
        rc = c5_prepare_job(cp.job[cp.njobs++] = full, c.r.nt_o, prf, 0, 0, c.packed, c.stream);
    } else {
        full.epi = 0; full.Co = Ch; full.ld = Ch; full.accumulate = 0; full.out_bstride = (long long)c.HW * Ch;
        for (int kk = 0; kk < L.ks_o && !rc; ++kk) {
            C5Job& j = cp.job[cp.njobs++];
            c5_chunk_job(full, prf, kk, L.ks_o, j, pr);
            j.wpk = s.kwo[kk];
            j.out = s.part_o + (size_t)kk * L.n_state;
            rc = c5_prepare_job(j, c.r.nt_o, pr, 0, 0, c.packed, c.stream);
        }
    }
    if (rc) return rc;
    VPX_CHECK_HIP(launch_c5(cp, c.r.nt_o, c.stream));
    if (!ks) return VPX_OK;
    STOutKSArgs oa{};
    oa.n = (long long)L.n_state; oa.ks = L.ks_o; oa.pstride = (long long)L.n_state; oa.part = s.part_o;
    oa.o_pre = s.o_pre; oa.lc = s.lc; oa.h_new = c.t.out[0]; oa.o_save = c.res.o; oa.tl_save = c.res.tl; oa.h_sp = c.sh.out[0]; oa.Ch = Ch;
    VPX_CHECK_HIP(launch_st_out_ks(oa, c.stream));
    return VPX_OK;
}

// ---- GEN1 ----
// weight repack (skipped when the caller vouches the workspace still holds it)
int gen1_pack(const STFwdCtx& c) {
    if (c.packed) return VPX_OK;
    const STLayout& L = *c.L; const STFwdTensors& t = c.t; const int Cin = c.d->Cin, Ch = c.d->Ch;
    PackDesc pd{};
    // c group: x rows (i,f,g,o) = blocks 0,1,2,6 of Wx (predrnn.py:61); h rows (i,f,g,o) = blocks 0..3 of Wh (:62)
    pd.seg[0] = PackSeg{t.Wx, (long long)Cin * L.taps, L.taps, 0, Cin};
    pd.seg[1] = PackSeg{t.Wh, (long long)Ch * L.taps, L.taps, 0, Ch};
    memcpy(pd.stage, L.stage_g, sizeof(ConvStage) * L.nstage_g);
    pd.nstage = L.nstage_g; pd.chunks_total = L.chunks_g; pd.prec = c.d->precision; pd.n_tiles = L.tiles32; pd.taps = L.taps; pd.NG = 4;
    const int xr[4] = {0, 1, 2, 6};
    for (int g = 0; g < 4; ++g) { pd.rowbase[0][g] = xr[g] * Ch; pd.rowbase[1][g] = g * Ch; pd.goff[g] = 0; }
    pd.tile_stride = 32; pd.nch = Ch;
    VPX_CHECK_HIP(launch_pack_weights(pd, c.ws.wpk_c, c.stream));
    // m group: x rows (i',f',g') = blocks 3,4,5 of Wx; m rows (i,f,g) = blocks 0..2 of Wm (:63)
    pd.seg[1] = PackSeg{t.Wm, (long long)Ch * L.taps, L.taps, 0, Ch};
    pd.NG = 3;
    for (int g = 0; g < 3; ++g) { pd.rowbase[0][g] = (3 + g) * Ch; pd.rowbase[1][g] = g * Ch; }
    pd.rowbase[0][3] = pd.rowbase[1][3] = -1;
    VPX_CHECK_HIP(launch_pack_weights(pd, c.ws.wpk_m, c.stream));
    // conv_o over mem = [c_new | m_new]: Wo [Ch, 2Ch, k, k]
    PackDesc po{};
    po.seg[0] = PackSeg{t.Wo, (long long)2 * Ch * L.taps, L.taps, 0, Ch};
    po.seg[1] = PackSeg{t.Wo, (long long)2 * Ch * L.taps, L.taps, Ch, Ch};
    memcpy(po.stage, L.stage_o, sizeof(ConvStage) * L.nstage_o);
    po.nstage = L.nstage_o; po.chunks_total = L.chunks_o; po.prec = c.d->precision; po.taps = L.taps;
    fill_plain_pack(po, Ch, 0, L.o_ng);  // ng = 1: 32 output channels per N tile (the fused launch's layout)
    VPX_CHECK_HIP(launch_pack_weights(po, c.ws.wpk_o, c.stream));
    return pack_conv_last(c);
}
// launches 1 + 2: the c group and the m group are independent and run as ONE dual launch
int gen1_gates(const STFwdCtx& c) {
    const STLayout& L = *c.L; const STFwdTensors& t = c.t; const int Cin = c.d->Cin, Ch = c.d->Ch, k = c.d->k;
    ConvPlan P = base_plan(c.d, k);
    set_plan_tiles(P, L.mw_g);
    P.nseg = 2;
    P.seg[0] = ConvSeg{t.x, (long long)(c.HW * Cin), Cin, 0};
    P.seg[1] = ConvSeg{t.h, (long long)(c.HW * Ch), Ch, 0};
    P.nstage = L.nstage_g; memcpy(P.stage, L.stage_g, sizeof(ConvStage) * L.nstage_g);
    P.chunks_total = L.chunks_g; P.a_bytes = conv_a_bytes(L.stage_g, L.nstage_g, k, k, L.mw_g); P.wpk = c.ws.wpk_c;
    STGateArgs ea{Ch, 1.0f, t.c, t.out[1], t.out[3], c.ws.o_pre, c.res.gates_c};
    ConvPlan Pm = P;
    Pm.seg[1] = ConvSeg{t.m, (long long)(c.HW * Ch), Ch, 0};
    Pm.wpk = c.ws.wpk_m;
    STGateArgs em{Ch, 1.0f, t.m, t.out[2], t.out[4], nullptr, c.res.gates_m};
    VPX_CHECK_HIP(launch_st_gates_dual(P, ea, Pm, em, L.tiles32, c.stream));
    return VPX_OK;
}
// launch 4: conv_o(mem) fused with the output gate, or (o_split) K-split into o_pre and the pointwise gate
int gen1_out(const STFwdCtx& c) {
    const STLayout& L = *c.L; const STFwdSlots& s = c.ws; const int Ch = c.d->Ch, k = c.d->k;
    ConvPlan P = mem_plan(c, k);
    set_plan_tiles(P, L.mw_o);
    P.nstage = L.nstage_o; memcpy(P.stage, L.stage_o, sizeof(ConvStage) * L.nstage_o);
    P.chunks_total = L.chunks_o; P.a_bytes = conv_a_bytes(L.stage_o, L.nstage_o, k, k, L.mw_o); P.wpk = s.wpk_o;
    if (c.r.o_split > 1) {
        PlainEpiArgs pa{};
        pa.Co = Ch; pa.split = Ch; pa.out0 = s.o_pre; pa.bstride0 = (long long)(c.HW * Ch); pa.ld0 = Ch; pa.ng = L.o_ng;
        pa.accumulate = 1;  // o_pre already holds o_x + o_h (c-group launch)
        P.ksplit = c.r.o_split;
        VPX_CHECK_HIP(launch_conv_plain_f32(P, pa, L.o_tiles, c.stream));
        VPX_CHECK_HIP(launch_st_ln_out(s.o_pre, nullptr, s.lc, c.t.out[0], c.res.o, c.res.tl, (long long)L.n_state, c.stream));
    } else {
        STOutArgs ea{Ch, s.o_pre, s.lc, c.t.out[0], c.res.o, c.res.tl};
        VPX_CHECK_HIP(launch_st_out_f32(P, ea, L.tiles32, c.stream));
    }
    return VPX_OK;
}

// ---- every route's launch 3: conv_last(mem) 1x1 -> lc ----
// the streaming kernel's view of it (conv1.hip): what c1_applicable is asked about, by the call and by the plan query
C1Args conv_last_c1(const vpx_stlstm_desc* d, const float* c_new, const float* m_new, const float* Wlast, float* lc) {
    const int Ch = d->Ch;
    C1Args c1{};
    c1.x[0] = c_new; c1.x[1] = m_new; c1.xld[0] = c1.xld[1] = Ch; c1.xc[0] = c1.xc[1] = Ch;
    c1.npix = (long long)d->B * d->H * d->W;
    c1.w = Wlast; c1.w_sn = 2 * Ch; c1.w_sc = 1;
    c1.y[0] = lc; c1.yld[0] = Ch; c1.ysplit = Ch; c1.Co = Ch;
    return c1;
}
int conv_last(const STFwdCtx& c) {
    const STLayout& L = *c.L; const STFwdSlots& s = c.ws; const int Ch = c.d->Ch;
    C1Args c1 = conv_last_c1(c.d, c.t.out[1], c.t.out[2], c.t.Wlast, s.lc);
    if (c.r.last_split) {
        // the gate stage left c_new / m_new in the operand format as well: read THOSE (no fp32 -> (hi, lo) conversion in the kernel; round 6)
        c1.x[0] = reinterpret_cast<const float*>(s.cn_sp); c1.x[1] = reinterpret_cast<const float*>(s.mn_sp); c1.x_split = 1;
    }
    if (c1_applicable(c1, c.d->precision)) {
        VPX_CHECK_HIP(launch_c1(c1, c.stream));   // streaming form (conv1.hip): no weight pack, no LDS
        return VPX_OK;
    }
    ConvPlan P = mem_plan(c, 1);
    if (on_c5(c.r.route)) {   // the gate stage left c_new / m_new in the split format as well: staged without conversion
        P.seg[0] = ConvSeg{reinterpret_cast<const float*>(s.cn_sp), (long long)(c.HW * Ch), Ch, 0, 1};
        P.seg[1] = ConvSeg{reinterpret_cast<const float*>(s.mn_sp), (long long)(c.HW * Ch), Ch, 0, 1};
    }
    P.nstage = L.nstage_l; memcpy(P.stage, L.stage_l, sizeof(ConvStage) * L.nstage_l);
    P.chunks_total = L.chunks_l; P.a_bytes = conv_a_bytes(L.stage_l, L.nstage_l, 1, 1); P.wpk = s.wpk_l;
    PlainEpiArgs ea{};
    ea.Co = Ch; ea.split = Ch; ea.out0 = s.lc; ea.bstride0 = (long long)(c.HW * Ch); ea.ld0 = Ch; ea.ng = L.ng_l;
    P.ksplit = L.ksplit_l;
    if (P.ksplit > 1) VPX_CHECK_HIP(vpx_memset_async(s.lc, 0, L.n_state * sizeof(float), c.stream));
    VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, L.tiles128, c.stream));
    return VPX_OK;
}

}  // namespace

extern "C" {

int vpx_stlstm_uses_split(const vpx_stlstm_desc* d) {
    if (check_st_desc(d) != VPX_OK || d->layout != VPX_LAYOUT_NHWC) return 0;
    return on_c5(st_route(d)) ? 1 : 0;
}

int vpx_stlstm_plan(const vpx_stlstm_desc* d, int all_weight_grads, vpx_stlstm_plan_info* out) {
    int rc = check_st_desc(d);
    if (rc != VPX_OK) return rc;
    if (!out) { set_error("vpx_stlstm_plan: out is NULL"); return VPX_ERR_ARG; }
    STLayout L;
    if ((rc = st_layout(d, L)) != VPX_OK) return rc;
    const STRouteChoice r = st_choice(d, L);
    *out = vpx_stlstm_plan_info{};
    out->route = (int)r.route; out->o_split = r.o_split; out->nt_o = r.nt_o; out->ks_g = L.ks_g; out->ks_o = L.ks_o;
    out->mw_g = L.mw_g; out->mw_o = L.mw_o; out->ksplit_l = L.ksplit_l;
    out->last_c1 = r.route != STRoute::LN && c1_applicable(conv_last_c1(d, nullptr, nullptr, nullptr, nullptr), d->precision) ? 1 : 0;
    if (r.route == STRoute::LN) return VPX_OK;   // (the LayerNorm variant's backward has no forms to choose from)
    rc = stlstm_bwd_plan(d, all_weight_grads != 0, out);
    return (d->flags & VPX_FLAG_SAVE_FOR_BWD) ? rc : VPX_OK;   // (a descriptor that does not save is followed by no backward)
}

size_t vpx_stlstm_reserve_bytes(const vpx_stlstm_desc* d) {
    STLayout L;
    if (check_st_desc(d) != VPX_OK || st_layout(d, L) != VPX_OK) return 0;
    return d->layer_norm ? stlstm_ln_reserve_bytes(d) : stlstm_reserve(d, L, nullptr).bytes;   // (a descriptor that does not save has none)
}

// the larger of the two directions' carves, each measured by the function that carves it, + the base-alignment slack
size_t vpx_stlstm_workspace_bytes(const vpx_stlstm_desc* d) {
    STLayout L;
    if (check_st_desc(d) != VPX_OK || st_layout(d, L) != VPX_OK) return 0;
    CarveMeasure m; STFwdSlots s{};
    if (!d->layer_norm) carve_st_fwd(m, d, L, st_choice(d, L), s);
    const size_t fwd = d->layer_norm ? stlstm_ln_workspace_bytes(d) : m.off;
    const size_t bwd = (d->flags & VPX_FLAG_SAVE_FOR_BWD) && !d->layer_norm ? stlstm_bwd_workspace_bytes(d) : 0;   // (only a saving call is followed by one)
    return (fwd > bwd ? fwd : bwd) + 256;
}

int vpx_stlstm_step_fwd(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m, const float* Wx, const float* Wh,
                        const float* Wm, const float* Wo, const float* Wlast, const float* const* ln, float* h_new, float* c_new, float* m_new,
                        float* delta_c, float* delta_m, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    return vpx_stlstm_step_fwd_ex(d, x, h, c, m, Wx, Wh, Wm, Wo, Wlast, ln, h_new, c_new, m_new, delta_c, delta_m, reserve, reserve_bytes,
                                  workspace, workspace_bytes, stream_, nullptr);
}

int vpx_stlstm_step_fwd_ex(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m, const float* Wx, const float* Wh,
                           const float* Wm, const float* Wo, const float* Wlast, const float* const* ln, float* h_new, float* c_new, float* m_new,
                           float* delta_c, float* delta_m, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream_,
                           const vpx_stlstm_shadows* shadows) {
    int rc = check_st_desc(d);
    if (rc != VPX_OK) return rc;
    STLayout L;
    if ((rc = st_layout(d, L)) != VPX_OK) return rc;
    if (!x || !h || !c || !m || !Wx || !Wh || !Wm || !Wo || !Wlast || !h_new || !c_new || !m_new || !delta_c || !delta_m) {
        set_error("vpx_stlstm_step_fwd: NULL tensor argument");
        return VPX_ERR_ARG;
    }
    const bool save = (d->flags & VPX_FLAG_SAVE_FOR_BWD) != 0;
    if (save && (!reserve || reserve_bytes < vpx_stlstm_reserve_bytes(d))) { set_error("vpx_stlstm_step_fwd: reserve too small"); return VPX_ERR_WORKSPACE; }
    if (!workspace || workspace_bytes < vpx_stlstm_workspace_bytes(d)) {
        set_error("vpx_stlstm_step_fwd: workspace too small (%zu < %zu)", workspace_bytes, vpx_stlstm_workspace_bytes(d));
        return VPX_ERR_WORKSPACE;
    }
    STFwdCtx f{};
    f.d = d; f.L = &L; f.r = st_choice(d, L); f.stream = (hipStream_t)stream_;
    f.HW = (size_t)d->H * d->W; f.npix = (long long)d->B * (long long)f.HW; f.packed = (d->flags & VPX_FLAG_WEIGHTS_PACKED) != 0;
    f.t = STFwdTensors{x, h, c, m, Wx, Wh, Wm, Wo, Wlast, ln, {h_new, c_new, m_new, delta_c, delta_m}};
    if (f.r.route == STRoute::LN) {   // unfused LayerNorm path (stlstm_ln_api.hip), the layout adaptation inside it
        if (!ln) { set_error("vpx_stlstm_step_fwd: layer_norm set but ln is NULL"); return VPX_ERR_ARG; }
        return stlstm_ln_fwd(d, f.t, reserve, workspace, workspace_bytes, f.stream);
    }
    if (d->layout == VPX_LAYOUT_NHWC) f.sh = st_shadows_of(shadows);
    f.res = stlstm_reserve(d, L, reserve);
    Carver ws(workspace, workspace_bytes);
    carve_st_fwd(ws, d, L, f.r, f.ws);
    VPX_CHECK_CARVE(ws, "vpx_stlstm_step_fwd");
    STFwdTensors& t = f.t;
    if ((rc = st_stage_in(d, f.ws.nchw, &t.x, {&t.h, &t.c, &t.m}, 3, {&t.out[0], &t.out[1], &t.out[2], &t.out[3], &t.out[4]}, nullptr, f.stream))) return rc;
    switch (f.r.route) {   // launches 1 + 2 behind the route's weight packs (skipped where the caller's workspace still holds them)
        case STRoute::C5: case STRoute::C5K: rc = c5_gates(f); break;
        default: if ((rc = gen1_pack(f)) == VPX_OK) rc = gen1_gates(f); break;
    }
    if (rc != VPX_OK || (rc = conv_last(f)) != VPX_OK) return rc;
    switch (f.r.route) {   // launch 4: conv_o(mem) + output gate
        case STRoute::C5: case STRoute::C5K: rc = c5_out(f); break;
        default: rc = gen1_out(f); break;
    }
    return rc != VPX_OK ? rc : st_stage_out(d, f.ws.nchw, f.stream);
}

}  // extern "C"
