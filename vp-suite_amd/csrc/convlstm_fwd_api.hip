// convlstm_fwd_api.hip — vpx_convlstm_seq_fwd and its queries (include/vpx.h). Host code only: the route of a call is decided once
// (convlstm_route), one function carves the workspace for the call and for the size query (carve_fwd), each route has its own functions.
#include "vpx_host.h"

#include <mutex>
using namespace vpx;

// c3 (convq.hip: c5_kernel<NT, 3>, round 4): the fused step on 16x16-pixel tiles x (4 gates x NT * 4 channels) with 8-channel stages, for the
// launches in which the half tile of cell2_kernel_q leaves most of the chip empty (B = 4 on 64x64 maps: 128 workgroups of four waves,
// one wave per SIMD on half the CUs, each running 36 steps of 96 MFMAs plus a 25 k-cycle epilogue alone). Halving / quartering the N
// tile doubles / quadruples the waves and shortens each wave's critical path. Inference only (it does not write the saved gates).
// VPX_EXP_NO_C3 keeps the half tile there (A/B runs, tests).
static int c3_nt(const vpx_convlstm_desc* d, const ConvLSTMLayout& L) {   // 0: not applicable; else column tiles per N tile (4 | 2)
    if (!L.v2 || !cell2_q_applicable(d) || d->precision != VPX_PREC_BF16X3 || (d->flags & VPX_FLAG_SAVE_FOR_BWD) || exp_on(VPX_EXP_NO_C3)) return 0;
    if ((d->Cin & 7) || (d->Ch & 15)) return 0;
    const long long mt = (long long)d->B * ((d->H + 15) / 16) * ((d->W + 15) / 16);
    // Measured (round 4, B = 4, 64x64 maps, Ch = 64: 128 half-tile workgroups of 39 us). First pass: 32-column tiles (512 workgroups) 34 us,
    // 64-column tiles (256) 36 us — the narrow tiles were bound by their K loop's bookkeeping. With that gone (convq.hip, "the K loop's
    // diet") the 64-column tiles win: cell (64,64,64^2) B = 4 0.309 vs 0.336 ms per 10 steps, inference step 1.60 vs 1.63 ms
    // — half the stage copies per MFMA. With 192 half-tile workgroups (64x64 maps, Ch = 96: configs[3]'s shard) the
    // 64-column c3 tiles are 1.4 % ahead on the whole model (5.70 vs 5.78 ms per step, the (64,96,64^2) cell alone 2 %), equal at B = 8 / 16 on
    // 64x64 maps with Ch = 64 (256 / 512 half-tile workgroups) — and behind once the 128x128 maps' 512 workgroups join (5.88 vs 5.72):
    // c3 up to 256 half-tile workgroups (128 in the first pass of the round, for the 32-column tiles).
    constexpr int C3_MAX = 256;
    if (mt * L.n_tiles > C3_MAX) return 0;
    return exp_on(VPX_EXP_C3_NARROW) ? 2 : 4;   // VPX_EXP_C3_NARROW: the 32-column tiles (tests, A/B runs)
}

// ---- the route of a call: which kernels take the steps --------------------------------------------------------------
enum class Route {
    FUSED,    // first generation: one fused conv + gate + state-update launch per step
    KSPLIT,   // small grids: the pre-activations by a K-split plain convolution (atomics) into a gate buffer, then the pointwise kernel
    HOIST,    // ... with W_x (*) x_t of all frames hoisted into one launch: a step contracts h_{t-1} only and accumulates into its slice
    CELL3,    // small grids where cell3.hip applies: hoisted projection, no K split, no atomics
    CELL2,    // the second-generation cell on pre-split operands (qform: its 16x16x32 MFMA form)
    C3,       // ... its small-grid form on the c5 machinery (c5_kernel<c3nt, 3>): cell2's operand sets in cell2's pack slots
};
struct RouteChoice { Route route; int qform, c3nt; };   // qform: CELL2 and C3 (c3 implies it); c3nt: C3, column tiles per N tile
// The only reader of the layout's route flags. `hoist` implies `split`; without an input tensor nothing is hoisted: the K split takes the steps.
static RouteChoice convlstm_route(const vpx_convlstm_desc* d, const ConvLSTMLayout& L, bool x_present) {
    if (L.v3) return {Route::CELL3, 0, 0};
    if (L.v2) { const int nt = c3_nt(d, L); return {nt ? Route::C3 : Route::CELL2, cell2_q_applicable(d) ? 1 : 0, nt}; }
    if (L.hoist && x_present) return {Route::HOIST, 0, 0};
    return {L.split ? Route::KSPLIT : Route::FUSED, 0, 0};
}
static bool on_cell2(const RouteChoice& r) { return r.route == Route::CELL2 || r.route == Route::C3; }
static bool on_ksplit(const RouteChoice& r) { return r.route == Route::KSPLIT || r.route == Route::HOIST; }
static bool inference_nhwc(const vpx_convlstm_desc* d) { return d->layout == VPX_LAYOUT_NHWC && !(d->flags & VPX_FLAG_SAVE_FOR_BWD); }

// one cell2 weight pack: an upper bound over both MFMA forms (the q form rounds an odd stage count up by half a stage)
static size_t cell2_wpk_bytes(const vpx_convlstm_desc* d, const ConvLSTMLayout& L) {
    const int S = (d->Cin + d->Ch) / 16;
    const size_t a = cell2_packed_bytes(L.n_tiles, 3 * S), b = cell2_packed_bytes_q(L.n_tiles, S);
    size_t m = a > b ? a : b;
    for (int nt = 2; nt <= 4; nt += 2) { const size_t c = c5_wpk_bytes(d->Cin + d->Ch, d->Ch, nt, 4, 3); if (c > m) m = c; }
    return m;
}
static size_t convlstm_wpk_bytes(const vpx_convlstm_desc* d, const ConvLSTMLayout& L, bool ksplit) {
    return ksplit ? packed_weight_bytes(L.s_tiles, L.s_chunks, L.s_ng, d->precision)
                  : packed_weight_bytes(L.n_tiles, L.chunks_total, 4, d->precision, L.qpc);
}

// The hoisted input projection W_x (*) x_t of all B*T frames (small-grid paths) as ONE launch of the schedule-driven K = 32 kernel
// (convq.hip): a plain 3x3 'same' convolution whose output channel is the reference row of W (gate-major), on operand-format input.
// 40 frames 64 -> 4x96 channels at 32x32: 84 -> ~25 us against the first-generation launch.
static bool hoist_q_problem(const vpx_convlstm_desc* d, ConvQProblem& pr) {
    memset(&pr, 0, sizeof(pr));
    if (exp_on(VPX_EXP_HOIST_GEN1)) return false;   // VPX_EXP_HOIST_GEN1: the first-generation launch (tests, A/B)
    if (d->precision != VPX_PREC_BF16X3 || d->kh != 3 || d->kw != 3 || (d->Cin & 15) || d->Cin < 16 || d->layout != VPX_LAYOUT_NHWC) return false;
    pr.N = d->B * d->T; pr.H = d->H; pr.W = d->W; pr.halo = 2;
    pr.nseg = 1;
    CQSeg& sg = pr.seg[0];
    sg.nT = 1; sg.bstride = (long long)d->H * d->W * d->Cin * 4;
    sg.rowpitch = d->W * d->Cin * 4; sg.colpitch = d->Cin * 4; sg.org = 0; sg.Hs = d->H; sg.Ws = d->W; sg.nstage = d->Cin / 16; sg.c0 = 0;
    pr.ngs = 1;
    ConvQGroupSet& gs = pr.gs[0];
    gs.nt0 = 0; gs.ntn = 8; gs.nterm = 0;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) gs.term[gs.nterm++] = ConvQTerm{0, ky - 1, kx - 1, ky * 3 + kx};
    pr.periodic = 1;
    pr.s_oc = (long long)(d->Cin + d->Ch) * 9; pr.s_ic = 9;
    pr.Co = 4 * d->Ch; pr.col0 = 0; pr.phases = 0;
    return convq_wpk_bytes(pr) != 0;
}
// (the routes with a hoisted projection run it on convq where hoist_q_problem() describes it)
static bool route_hoists_on_convq(const vpx_convlstm_desc* d, const RouteChoice& r, ConvQProblem& pr) {
    return (r.route == Route::HOIST || r.route == Route::CELL3) && hoist_q_problem(d, pr);
}

// ---- the forward workspace: ONE list of slots, taken in this order by a call's Carver and by the size query's CarveMeasure ----
struct FwdSlots {
    float *wpk, *c_scratch, *pre_scratch;            // first-generation weight pack; c_t between steps; K split: gate pre-activations of one step
    float *pre_all, *wpk_hx, *wpk_hh;                // hoisted projection of all steps [B,T,HW,4Ch] + the packs of W's x columns / h columns
    char *wpk3, *h0_sp3, *h_ring3[2];                // cell3: slice-major recurrent weights, split h0, a two-slot ring of h_t
    char *wpk_hq, *x_sp_hq;                          // the hoisted projection on convq: its weight pack + x in operand format
    char *wpk2, *wpk2b, *x_sp, *h0_sp, *h_ring[2];   // cell2 (q form: up to two packs, one per set of present operands), split x, h0, ring of h_t
    float *bx, *bout, *bh0, *bc0, *bhT, *bcT, *bpeep[3];   // NCHW staging
};
// hq: the hoisted projection's convq problem, or null where the route has none. A saving call on cell2 carves x_sp, h0_sp and the ring as
// well, although its copies live in the reserve: the size, and with it the Python workspace cache's exact-size test, stays what it was.
template <class WS>
static void carve_fwd(WS& ws, const vpx_convlstm_desc* d, const ConvLSTMLayout& L, const RouteChoice& r, const ConvQProblem* hq, FwdSlots& s) {
    s.wpk = ws.take(convlstm_wpk_bytes(d, L, on_ksplit(r)) / sizeof(float));
    s.c_scratch = ws.take(L.n_state);
    if (on_ksplit(r)) s.pre_scratch = ws.take(4 * L.n_state);
    if (r.route == Route::HOIST || r.route == Route::CELL3) {
        s.pre_all = ws.take(4 * L.n_out);
        s.wpk_hx = ws.take(packed_weight_bytes(L.s_tiles, L.hx_chunks, L.s_ng, d->precision) / sizeof(float));
    }
    if (r.route == Route::HOIST) s.wpk_hh = ws.take(packed_weight_bytes(L.s_tiles, L.hh_chunks, L.s_ng, d->precision) / sizeof(float));
    if (r.route == Route::CELL3) {
        s.wpk3 = (char*)ws.take(cell3_packed_bytes(d->Ch) / sizeof(float));
        for (char** p : {&s.h0_sp3, &s.h_ring3[0], &s.h_ring3[1]}) *p = (char*)ws.take(L.n_state);
    }
    if (hq) {
        s.wpk_hq = (char*)ws.take(align256(convq_wpk_bytes(*hq)) / sizeof(float));
        s.x_sp_hq = (char*)ws.take(L.n_x);
    }
    if (on_cell2(r)) {
        for (char** p : {&s.wpk2, &s.wpk2b}) *p = (char*)ws.take(cell2_wpk_bytes(d, L) / sizeof(float));
        s.x_sp = (char*)ws.take(L.n_x);
        for (char** p : {&s.h0_sp, &s.h_ring[0], &s.h_ring[1]}) *p = (char*)ws.take(L.n_state);
    }
    if (d->layout == VPX_LAYOUT_NCHW) {
        s.bx = ws.take(L.n_x);
        s.bout = ws.take(L.n_out);
        for (float** p : {&s.bh0, &s.bc0, &s.bhT, &s.bcT}) *p = ws.take(L.n_state);
        for (auto& p : s.bpeep) p = ws.take(L.n_peep);
    }
}

// 1: the inference forward (NHWC) takes x (input) / writes h_t (output) in the split operand format. The second-generation cell does both
// anyway; cell3 keeps h_t in operand format for its own recurrence, and x only feeds its hoisted projection W_x (*) x_t of all frames: where
// that runs on the schedule-driven kernel it reads the operand format — the producing stage then writes it directly (no fp32 copy, no
// conversion launch)
static int split_format(const vpx_convlstm_desc* d, bool input) {
    ConvLSTMLayout L;
    if (check_convlstm_desc(d) != VPX_OK || convlstm_layout(d, L) != VPX_OK || !inference_nhwc(d)) return 0;
    const RouteChoice r = convlstm_route(d, L, true);
    ConvQProblem pr;
    return on_cell2(r) || (r.route == Route::CELL3 && (!input || hoist_q_problem(d, pr))) ? 1 : 0;
}

extern "C" {
size_t vpx_convlstm_reserve_bytes(const vpx_convlstm_desc* d) {
    ConvLSTMLayout L;
    if (check_convlstm_desc(d) != VPX_OK || convlstm_layout(d, L) != VPX_OK) return 0;
    return convlstm_reserve(d, L, nullptr).bytes;
}
int vpx_convlstm_takes_split_input(const vpx_convlstm_desc* d) { return split_format(d, true); }
int vpx_convlstm_writes_split_output(const vpx_convlstm_desc* d) { return split_format(d, false); }

// the larger of the two directions' carves, each measured by the function that carves it (x taken as present), + the alignment slack
size_t vpx_convlstm_workspace_bytes(const vpx_convlstm_desc* d) {
    ConvLSTMLayout L;
    if (check_convlstm_desc(d) != VPX_OK || convlstm_layout(d, L) != VPX_OK) return 0;
    const RouteChoice r = convlstm_route(d, L, true);
    ConvQProblem hq; CarveMeasure m; FwdSlots s{};
    carve_fwd(m, d, L, r, route_hoists_on_convq(d, r, hq) ? &hq : nullptr, s);
    const size_t bwd = (d->flags & VPX_FLAG_SAVE_FOR_BWD) ? convlstm_bwd_workspace_bytes(d, L) : 0;   // (only a saving call is followed by one)
    return (m.off > bwd ? m.off : bwd) + 256;
}
}  // extern "C"

// ---- what every route's functions see of a call ----
struct FwdCtx {
    const vpx_convlstm_desc* d; const ConvLSTMLayout* L; RouteChoice r;
    const float *x, *h0, *c0, *W, *bias, *wci, *wcf, *wco;   // native layout (NHWC): the caller's tensors or their staged copies
    float *out, *hT, *cT;
    FwdSlots ws;           // (cell2 routes: x_sp / h0_sp are redirected to the reserve by a saving call, x_sp to the caller's x under X_SPLIT)
    ConvLSTMReserve res;   // all null unless the call saves for the backward
    int gp[4]; hipStream_t stream; size_t HW;
    bool save, wp, x_split, out_split;   // wp: the caller's workspace still holds every weight pack of an earlier call with the same descriptor, weights and operand set
    bool hoist_q; ConvQProblem hq;       // the hoisted projection runs on convq: `hq` is its problem
};

// A launch chain of the time loop: the samples [b0, b0 + B) of the call, step after step on one stream. Every operand of a step carries a
// batch stride, so a chain is the call's base pointers advanced by b0 strides and a launch over B samples — of the kernel the route chose
// for the WHOLE call (c.r, c.L: a chain never re-decides them from its own grid).
struct Chain { int b0, B; hipStream_t stream; };

// ---- layout adaptation (reference NCHW -> native NHWC) ----
static int stage_in_nchw(FwdCtx& c) {
    const FwdSlots& s = c.ws;
    const int B = c.d->B, T = c.d->T, Cin = c.d->Cin, Ch = c.d->Ch, H = c.d->H, Wd = c.d->W;
    if (c.x) { VPX_CHECK_HIP(launch_nchw_to_nhwc(c.x, s.bx, B * T, Cin, H, Wd, c.stream)); c.x = s.bx; }
    if (c.h0) { VPX_CHECK_HIP(launch_nchw_to_nhwc(c.h0, s.bh0, B, Ch, H, Wd, c.stream)); c.h0 = s.bh0; }
    if (c.c0) { VPX_CHECK_HIP(launch_nchw_to_nhwc(c.c0, s.bc0, B, Ch, H, Wd, c.stream)); c.c0 = s.bc0; }
    const float** peep[3] = {&c.wci, &c.wcf, &c.wco};
    for (int i = 0; i < 3 && c.wci; ++i) { VPX_CHECK_HIP(launch_nchw_to_nhwc(*peep[i], s.bpeep[i], 1, Ch, H, Wd, c.stream)); *peep[i] = s.bpeep[i]; }
    c.out = s.bout; c.hT = c.hT ? s.bhT : nullptr; c.cT = c.cT ? s.bcT : nullptr;
    return VPX_OK;
}
// h_{t-1} in fp32 as an operand: the initial state (or none), then the output sequence
static ConvSeg h_prev(const FwdCtx& c, int t) {
    const size_t n = c.HW * c.d->Ch;
    return t == 0 ? ConvSeg{c.h0, (long long)n, c.d->Ch, 0} : ConvSeg{c.out + (size_t)(t - 1) * n, (long long)(c.d->T * n), c.d->Ch, 0};
}

// ---- first generation: FUSED, KSPLIT (and the pack HOIST keeps for its x-less twin) ----
// weight repack: OIHW [4Ch, Cin+Ch, kh, kw] -> per-tile K-chunk stream
static int gen1_pack(const FwdCtx& c) {
    const vpx_convlstm_desc* d = c.d; const ConvLSTMLayout& L = *c.L;
    PackDesc pd{};
    const long long ld_o = (long long)(d->Cin + d->Ch) * L.taps;
    pd.seg[0] = PackSeg{c.W, ld_o, L.taps, 0, d->Cin};
    pd.seg[1] = PackSeg{c.W, ld_o, L.taps, d->Cin, d->Ch};
    pd.prec = d->precision; pd.taps = L.taps;
    if (on_ksplit(c.r)) {  // plain layout: output channel n = reference row n of W (gate-major), s_ng * 32 rows per N tile
        memcpy(pd.stage, L.s_stage, sizeof(ConvStage) * L.s_nstage);
        pd.nstage = L.s_nstage; pd.chunks_total = L.s_chunks;
        fill_plain_pack(pd, 4 * d->Ch, 0, L.s_ng);
    } else {
        memcpy(pd.stage, L.stage, sizeof(ConvStage) * L.nstage);
        pd.nstage = L.nstage; pd.chunks_total = L.chunks_total; pd.qpc = L.qpc; pd.n_tiles = L.n_tiles; pd.NG = 4;
        for (int g = 0; g < 4; ++g) { pd.rowbase[0][g] = pd.rowbase[1][g] = c.gp[g] * d->Ch; pd.goff[g] = 0; }
        pd.tile_stride = 32; pd.nch = d->Ch;
    }
    if (!c.wp) VPX_CHECK_HIP(launch_pack_weights(pd, c.ws.wpk, c.stream));
    return VPX_OK;
}
// the launch plan of step t over [x_t | h_{t-1}]: the fused kernel's tiling, or the plain convolution's when K is split
static ConvPlan gen1_plan(const FwdCtx& c, int t) {
    const vpx_convlstm_desc* d = c.d; const ConvLSTMLayout& L = *c.L;
    const bool ks = on_ksplit(c.r);
    ConvPlan P{};
    P.B = d->B; P.H = d->H; P.W = d->W; P.kh = d->kh; P.kw = d->kw;
    set_plan_tiles(P, ks ? 1 : L.mw);
    P.nseg = 2;
    P.seg[0] = ConvSeg{c.x ? c.x + (size_t)t * c.HW * d->Cin : nullptr, (long long)((size_t)d->T * c.HW * d->Cin), d->Cin, 0};
    P.seg[1] = h_prev(c, t);
    const ConvStage* stages = ks ? L.s_stage : L.stage; const int nstages = ks ? L.s_nstage : L.nstage;
    for (int s = 0; s < nstages; ++s)
        if (P.seg[stages[s].seg].ptr) P.stage[P.nstage++] = stages[s];  // absent source == all-zero operand: its K range is skipped
    P.chunks_total = ks ? L.s_chunks : L.chunks_total; P.prec = d->precision; P.qpc = ks ? 0 : L.qpc;
    P.a_bytes = conv_a_bytes(stages, nstages, d->kh, d->kw, ks ? 1 : L.mw); P.wpk = c.ws.wpk;
    return P;
}
static int fused_step(const FwdCtx& c, int t, const ConvLSTMStepArgs& ea) {
    VPX_CHECK_HIP(launch_convlstm_step_f32(gen1_plan(c, t), ea, c.L->n_tiles, c.stream));
    return VPX_OK;
}
// the 4Ch gate pre-activations (reference row order) of a plain convolution go to a gate buffer
static PlainEpiArgs gate_buffer_epi(const FwdCtx& c, float* out, long long bstride) {
    PlainEpiArgs pa{};
    pa.Co = 4 * c.d->Ch; pa.split = 4 * c.d->Ch; pa.ng = c.L->s_ng;
    pa.out0 = out; pa.bstride0 = bstride; pa.ld0 = 4 * c.d->Ch;
    return pa;
}
// pre-activations of all four gates by a K-split plain convolution (atomic partial sums), then the gates
static int ksplit_step(const FwdCtx& c, int t, const ConvLSTMStepArgs& ea) {
    const ConvLSTMLayout& L = *c.L;
    ConvPlan P = gen1_plan(c, t);
    float* pre = ea.gates ? ea.gates : c.ws.pre_scratch;  // with SAVE_FOR_BWD the reserve slot doubles as scratch
    VPX_CHECK_HIP(vpx_memset_async(pre, 0, 4 * L.n_state * sizeof(float), c.stream));
    P.ksplit = P.nstage ? L.split : 0;
    if (P.nstage > 0) VPX_CHECK_HIP(launch_conv_plain_f32(P, gate_buffer_epi(c, pre, (long long)(c.HW * 4 * c.d->Ch)), L.s_tiles, c.stream));
    VPX_CHECK_HIP(launch_convlstm_pointwise(ea, pre, c.d->B, (long long)c.HW, c.stream));
    return VPX_OK;
}

// ---- HOIST and CELL3: the hoisted projection; HOIST's step ----
// the pack of W's columns [coff, coff + C) and the launch plan of a plain convolution over them (reference row order, one operand)
static int plain_pack(const FwdCtx& c, int coff, int C, const ConvStage* st, int nst, int chunks, float* dst) {
    PackDesc p{};
    p.seg[0] = PackSeg{c.W, (long long)(c.d->Cin + c.d->Ch) * c.L->taps, c.L->taps, coff, C};
    memcpy(p.stage, st, sizeof(ConvStage) * nst);
    p.nstage = nst; p.chunks_total = chunks; p.prec = c.d->precision; p.taps = c.L->taps;
    fill_plain_pack(p, 4 * c.d->Ch, 0, c.L->s_ng);
    VPX_CHECK_HIP(launch_pack_weights(p, dst, c.stream));
    return VPX_OK;
}
static ConvPlan plain_plan(const FwdCtx& c, int N, ConvSeg seg, const ConvStage* st, int nst, int chunks, const float* wpk) {
    ConvPlan P{};
    P.B = N; P.H = c.d->H; P.W = c.d->W; P.kh = c.d->kh; P.kw = c.d->kw;
    set_plan_tiles(P, 1);
    P.nseg = 1; P.seg[0] = seg; P.nstage = nst;
    memcpy(P.stage, st, sizeof(ConvStage) * nst);
    P.chunks_total = chunks; P.prec = c.d->precision; P.wpk = wpk;
    P.a_bytes = conv_a_bytes(st, nst, c.d->kh, c.d->kw, 1);
    return P;
}
// two packs (x columns / h columns of W, reference row order), then W_x * x for all B*T frames in one launch
static int hoisted_projection(FwdCtx& c) {
    const vpx_convlstm_desc* d = c.d; const ConvLSTMLayout& L = *c.L;
    const int BT = d->B * d->T, Cin = d->Cin, Ch = d->Ch;
    const long long pre_bs = (long long)(c.HW * 4 * Ch);
    int rc;
    if (!c.wp && !c.hoist_q && (rc = plain_pack(c, 0, Cin, L.hx_stage, L.hx_nstage, L.hx_chunks, c.ws.wpk_hx)) != VPX_OK) return rc;
    if (!c.wp && c.r.route == Route::HOIST && (rc = plain_pack(c, Cin, Ch, L.hh_stage, L.hh_nstage, L.hh_chunks, c.ws.wpk_hh)) != VPX_OK) return rc;
    if (c.hoist_q) {
        const char* xs = reinterpret_cast<const char*>(c.x);
        if (!c.x_split) { VPX_CHECK_HIP(launch_split_convert(c.x, c.ws.x_sp_hq, (long long)BT * (long long)c.HW, Cin, c.stream)); xs = c.ws.x_sp_hq; }
        c.hq.seg[0].sp = xs; c.hq.w = c.W;
        ConvQEpiArgs ea{};
        ea.Co = 4 * Ch; ea.split = 4 * Ch; ea.oys = 1; ea.oxs = 1; ea.Hmem = d->H; ea.Wmem = d->W;
        ea.out0 = c.ws.pre_all; ea.bstride0 = pre_bs; ea.ld0 = 4 * Ch;
        return convq_run(c.hq, ea, c.ws.wpk_hq, c.wp, c.stream);
    }
    const ConvSeg xseg{c.x, (long long)(c.HW * Cin), Cin, 0};   // x is [B][T][HW][Cin]: B*T dense images
    const ConvPlan PX = plain_plan(c, BT, xseg, L.hx_stage, L.hx_nstage, L.hx_chunks, c.ws.wpk_hx);
    VPX_CHECK_HIP(launch_conv_plain_f32(PX, gate_buffer_epi(c, c.ws.pre_all, pre_bs), L.s_tiles, c.stream));
    return VPX_OK;
}
// the step contracts only h_{t-1} and accumulates (atomics when K is split) into its slice of the hoisted input
// projection; the pointwise kernel reads that slice (batch stride T*HW*4Ch) and writes gates / c / h
static int hoist_step(const FwdCtx& c, int t, const ConvLSTMStepArgs& ea) {
    const ConvLSTMLayout& L = *c.L;
    float* pre_t = c.ws.pre_all + (size_t)t * c.HW * 4 * c.d->Ch;
    const long long pre_bs = (long long)((size_t)c.d->T * c.HW * 4 * c.d->Ch);
    const ConvSeg hprev = h_prev(c, t);
    if (hprev.ptr) {
        ConvPlan PH = plain_plan(c, c.d->B, hprev, L.hh_stage, L.hh_nstage, L.hh_chunks, c.ws.wpk_hh);
        PH.ksplit = L.hh_split;
        PlainEpiArgs pa = gate_buffer_epi(c, pre_t, pre_bs);
        pa.accumulate = 1;
        VPX_CHECK_HIP(launch_conv_plain_f32(PH, pa, L.s_tiles, c.stream));
    }
    VPX_CHECK_HIP(launch_convlstm_pointwise(ea, pre_t, c.d->B, (long long)c.HW, c.stream, pre_bs));
    return VPX_OK;
}

// ---- CELL3 ----
static int cell3_pack(const FwdCtx& c) {
    const vpx_convlstm_desc* d = c.d;
    Cell3Pack pk{c.W, d->Cin, d->Ch, d->Cin + d->Ch, d->Ch / 8, 9 * d->Ch / 16, {c.gp[0], c.gp[1], c.gp[2], c.gp[3]}};
    if (!c.wp) VPX_CHECK_HIP(launch_cell3_pack(pk, c.ws.wpk3, c.stream));
    if (c.h0) VPX_CHECK_HIP(launch_split_convert(c.h0, c.ws.h0_sp3, (long long)d->B * (long long)c.HW, d->Ch, c.stream));
    return VPX_OK;
}
static int cell3_step(const FwdCtx& c, int t, const ConvLSTMStepArgs& ea) {
    const int T = c.d->T, Ch = c.d->Ch; const size_t HW = c.HW;
    Cell3Args c3{};
    c3.B = c.d->B; c3.H = c.d->H; c3.W = c.d->W; c3.wpk = c.ws.wpk3;
    c3.h_sp = (t == 0) ? (c.h0 ? c.ws.h0_sp3 : nullptr) : c.ws.h_ring3[(t - 1) & 1];
    c3.h_sp_out = (t + 1 < T) ? c.ws.h_ring3[t & 1] : nullptr;
    c3.h_bstride = c3.h_sp_out_bstride = (long long)(HW * Ch * 4);
    c3.pre = c.x ? c.ws.pre_all + (size_t)t * HW * 4 * Ch : nullptr;
    c3.pre_bstride = (long long)((size_t)T * HW * 4 * Ch);
    c3.ea = ea;
    if (c.out_split) {
        // the caller's `out` [B][T][HW][Ch] takes the steps' operand-format h_t (it is also where step t + 1 reads h_t); no fp32
        // sequence — the last step still hands h_T out in fp32 where the caller wants it
        const long long seq_bs = (long long)((size_t)T * HW * Ch * 4);
        char* const out_sp = reinterpret_cast<char*>(c.out);
        if (t > 0) { c3.h_sp = out_sp + (size_t)(t - 1) * HW * Ch * 4; c3.h_bstride = seq_bs; }
        c3.h_sp_out = out_sp + (size_t)t * HW * Ch * 4; c3.h_sp_out_bstride = seq_bs;
        c3.ea.h_out = (t == T - 1) ? c.hT : nullptr; c3.ea.h_bstride = (long long)(HW * Ch);
    }
    VPX_CHECK_HIP(launch_cell3(c3, c.stream));
    return VPX_OK;
}

// ---- CELL2 and C3 ----
// q form (16x16x32 MFMAs): the K = 32 steps pair taps over the sequence of PRESENT stages, so steps with different operand
// sets (t = 0 without an initial state: x only; no input tensor: h only) read different packs — at most two per call.
// An operand set is (x present ? 1 : 0) | (h present ? 2 : 0); the set of steps t >= 1 owns the first pack slot.
static char* cell2_pack_of(const FwdCtx& c, int combo) { return combo == ((c.x ? 1 : 0) | 2) ? c.ws.wpk2 : c.ws.wpk2b; }
// h_t in operand format: the reserve (training), the caller's `out` buffer laid out [B][T][HW][Ch] (OUT_SPLIT), or a two-slot ring
static char* cell2_h_slot(const FwdCtx& c, int tt) {
    if (c.out_split) return reinterpret_cast<char*>(c.out) + (size_t)tt * c.HW * c.d->Ch * 4;
    return c.res.h_sp ? c.res.h_sp + (size_t)tt * c.L->n_state * 4 : c.ws.h_ring[tt & 1];
}
// one operand set of the q form, packed for cell2_kernel_q (CELL2) or for c5_kernel<NT, 3> (C3)
static int cell2_pack_combo(const FwdCtx& c, Cell2Pack& pk, int combo) {
    const int Cin = c.d->Cin, Ch = c.d->Ch, *gp = c.gp;
    pk.qform = 1; pk.S = 0;
    if (combo & 1) for (int s = 0; s < Cin / 16; ++s) pk.stage_col[pk.S++] = 16 * s;
    if (combo & 2) for (int s = 0; s < Ch / 16; ++s) pk.stage_col[pk.S++] = Cin + 16 * s;
    pk.chunks_total = cell2_qchunks(pk.S);
    if (c.wp) return VPX_OK;
    if (!c.r.c3nt) { VPX_CHECK_HIP(launch_cell2_pack(pk, cell2_pack_of(c, combo), c.stream)); return VPX_OK; }
    C5Job j{};
    C5PackRange pr[2];
    const long long so = (long long)(Cin + Ch) * 9;
    if (combo & 1) { j.r_n[j.nrange] = Cin; pr[j.nrange] = C5PackRange{c.W, so, 9, 0, {gp[0] * Ch, gp[1] * Ch, gp[2] * Ch, gp[3] * Ch}}; ++j.nrange; }
    if (combo & 2) { j.r_n[j.nrange] = Ch; pr[j.nrange] = C5PackRange{c.W, so, 9, Cin, {gp[0] * Ch, gp[1] * Ch, gp[2] * Ch, gp[3] * Ch}}; ++j.nrange; }
    j.Co = Ch; j.wpk = cell2_pack_of(c, combo);
    return c5_prepare_job(j, c.r.c3nt, pr, 4, 0, false, c.stream, 0, 3);
}
// the packs of the call's operand sets, then the operands of the steps in split form
static int cell2_pack(FwdCtx& c) {
    const vpx_convlstm_desc* d = c.d; const int Cin = d->Cin, Ch = d->Ch;
    const int combo0 = (c.x ? 1 : 0) | (c.h0 ? 2 : 0), combo1 = (c.x ? 1 : 0) | 2;   // operand sets of step 0 / of steps t >= 1
    Cell2Pack pk{};
    pk.w = c.W; pk.Ch = Ch; pk.Ct = Cin + Ch; pk.n_tiles = c.L->n_tiles;
    memcpy(pk.gate_pos, c.gp, sizeof(c.gp));
    if (!c.r.qform) {
        pk.chunks_total = 3 * ((Cin + Ch) / 16);
        for (int s = 0; s < (Cin + Ch) / 16; ++s) pk.stage_col[s] = 16 * s;  // x stages first, then h: columns of [x | h] in order
        if (!c.wp) VPX_CHECK_HIP(launch_cell2_pack(pk, c.ws.wpk2, c.stream));
    } else {
        int rc;
        // combo1 serves steps t >= 1 (and step 0 when it has the same operands); combo0 only when it differs and is not empty
        if (!(d->T < 2 && combo0 != combo1) && (rc = cell2_pack_combo(c, pk, combo1)) != VPX_OK) return rc;
        if (combo0 != combo1 && combo0 != 0 && (rc = cell2_pack_combo(c, pk, combo0)) != VPX_OK) return rc;
    }
    // the whole input sequence and the initial hidden state, once. A saving call keeps them for the backward's weight gradient: in the reserve
    if (c.save) { c.ws.x_sp = c.res.x_sp; c.ws.h0_sp = c.res.h0_sp; }
    if (c.x && c.x_split) c.ws.x_sp = const_cast<char*>(reinterpret_cast<const char*>(c.x));   // the producer already wrote operands
    else if (c.x) VPX_CHECK_HIP(launch_split_convert(c.x, c.ws.x_sp, (long long)d->B * d->T * (long long)c.HW, Cin, c.stream));
    if (c.h0) VPX_CHECK_HIP(launch_split_convert(c.h0, c.ws.h0_sp, (long long)d->B * (long long)c.HW, Ch, c.stream));
    return VPX_OK;
}
static int cell2_step(const FwdCtx& c, int t, ConvLSTMStepArgs ea, const Chain& ch) {
    const vpx_convlstm_desc* d = c.d; const int T = d->T, Cin = d->Cin, Ch = d->Ch; const size_t HW = c.HW, b0 = (size_t)ch.b0;
    Cell2Plan P2{};
    P2.B = ch.B; P2.H = d->H; P2.W = d->W; P2.tiles_x = (d->W + 15) / 16; P2.tiles_y = (d->H + 31) / 32; P2.n_tiles = c.L->n_tiles;
    P2.chunks_total = 3 * ((Cin + Ch) / 16); P2.wpk = c.ws.wpk2;
    P2.qform = c.r.qform; P2.plain = d->precision == VPX_PREC_BF16 ? 1 : 0;
    const long long hsp_bs = c.out_split ? (long long)((size_t)T * HW * Ch * 4) : (long long)(HW * Ch * 4);
    // OUT_SPLIT: no fp32 sequence; the last step still hands h_T out in fp32 where the caller wants it
    if (c.out_split) { ea.h_out = (t == T - 1 && c.hT) ? c.hT + b0 * HW * Ch : nullptr; ea.h_bstride = (long long)(HW * Ch); }
    const char* hprev_sp = (t == 0) ? (c.h0 ? c.ws.h0_sp : nullptr) : cell2_h_slot(c, t - 1);
    P2.seg[0] = Cell2Seg{c.x ? c.ws.x_sp + (size_t)t * HW * Cin * 4 : nullptr, (long long)((size_t)T * HW * Cin * 4), Cin, 0};
    P2.seg[1] = Cell2Seg{hprev_sp, (t == 0) ? (long long)(HW * Ch * 4) : hsp_bs, Ch, 0};
    for (Cell2Seg& sg : P2.seg) if (sg.sp) sg.sp += b0 * (size_t)sg.bstride;   // the chain's first sample
    P2.nx = c.x ? Cin / 16 : 0; P2.nh = hprev_sp ? Ch / 16 : 0; P2.hs_off = Cin / 16;
    if (c.r.qform) {   // the pack of this step's operand set
        P2.chunks_total = cell2_qchunks(P2.nx + P2.nh);
        P2.wpk = cell2_pack_of(c, (P2.nx ? 1 : 0) | (P2.nh ? 2 : 0));
    }
    // the split copy of h_t feeds step t+1 only: the last step does not need it
    char* const hsp_t = (t + 1 < T || c.out_split) ? cell2_h_slot(c, t) + b0 * (size_t)hsp_bs : nullptr;
    if (c.r.route == Route::CELL2) { VPX_CHECK_HIP(launch_cell2(P2, ea, hsp_t, hsp_bs, ch.stream)); return VPX_OK; }
    C5Plan cp{};   // C3: the same step as one job of the c5 machinery
    cp.B = P2.B; cp.H = P2.H; cp.W = P2.W; cp.ks = 3;
    cp.src[0] = C5Src{P2.seg[0].sp, P2.seg[0].bstride, Cin * 4, 0};
    cp.src[1] = C5Src{P2.seg[1].sp, P2.seg[1].bstride, Ch * 4, 0};
    C5Job& j = cp.job[cp.njobs++] = C5Job{};
    if (P2.nx) { j.r_src[j.nrange] = 0; j.r_n[j.nrange] = Cin; ++j.nrange; }
    if (P2.nh) { j.r_src[j.nrange] = 1; j.r_n[j.nrange] = Ch; ++j.nrange; }
    j.epi = 3; j.Co = Ch; j.Ch = Ch; j.wpk = P2.wpk;
    j.e_in0 = ea.c_in; j.e_in1 = ea.wci; j.e_in2 = ea.wcf; j.e_in3 = ea.wco; j.bias = ea.bias;
    for (int g = 0; g < 4; ++g) j.gate_pos[g] = ea.gate_pos[g];
    j.e_out[0] = ea.h_out; j.e_out[1] = ea.c_out; j.h_bstride = ea.h_bstride;
    j.e_sp = hsp_t; j.sp_bstride = hsp_bs;
    const int rcj = c5_prepare_job(j, c.r.c3nt, nullptr, 4, 0, true, ch.stream, 0, 3);   // (derived fields only: the pack is in place)
    if (rcj) return rcj;
    VPX_CHECK_HIP(launch_c5(cp, c.r.c3nt, ch.stream));
    return VPX_OK;
}

// ---- the entry point: what every route's step is handed: bias, peepholes, where c and h of step t go, and the saved gates
// ... of the chain's samples: the per-sample tensors (c, gates, h) start at sample ch.b0, bias and peepholes are shared
static ConvLSTMStepArgs step_args(const FwdCtx& c, int t, const Chain& ch) {
    const size_t n = c.L->n_state, off = (size_t)ch.b0 * c.HW * c.d->Ch;   // off: sample b0 of a [B][HW][Ch] tensor
    ConvLSTMStepArgs ea{};
    ea.bias = c.bias; ea.Ch = c.d->Ch;
    memcpy(ea.gate_pos, c.gp, sizeof(c.gp));
    if (c.save) {   // c_t and the gates of every step stay in the reserve
        ea.c_in = (t == 0) ? c.c0 : c.res.cs + (size_t)(t - 1) * n;
        ea.c_out = c.res.cs + (size_t)t * n + off; ea.gates = c.res.gates + (size_t)t * n * 4 + 4 * off;
    } else {
        ea.c_in = (t == 0) ? c.c0 : c.ws.c_scratch;   // (updated in place per sample: each chain walks its own slice)
        ea.c_out = ((t == c.d->T - 1 && c.cT) ? c.cT : c.ws.c_scratch) + off;  // the last step writes c_T where the caller wants it
    }
    if (ea.c_in) ea.c_in += off;
    ea.wci = c.wci; ea.wcf = c.wcf; ea.wco = c.wco;
    ea.h_bstride = (long long)((size_t)c.d->T * c.HW * c.d->Ch);
    ea.h_out = c.out + (size_t)t * c.HW * c.d->Ch + (size_t)ch.b0 * (size_t)ea.h_bstride;
    return ea;
}

// ---- two launch chains ----
// One launch per step on one stream leaves holes nothing of the same call can fill: step t + 1 waits for the last workgroup of step t, so
// a launch's tail (CUs down to one workgroup), its cold-weights prologue and, on the 16x16 maps' 384 workgroups for 512 slots, a quarter
// of the chip are idle. The samples of a batch are independent through the whole sequence: the CELL2 and C3 routes run the two halves of
// the batch as two chains, chain 0 on the caller's stream, chain 1 on a stream of the library's, issued step by step in turn. Each chain
// launches the kernel the whole call chose, on its own samples: results are bit for bit those of the single chain, the workspace and the
// reserve are those of the whole call. vpx_set_option(VPX_OPT_SEQ_CHAINS, 0) keeps the single chain (A/B runs, tests); a capturing
// stream takes it too (the captured graph then holds no stream of the library's).
// The batch floor (convlstm-shi inference, ms per forward, one chain -> two, medians; DESIGN.md §4 has every run): B = 128 23.03 -> 22.67 and
// 22.85 -> 22.51 (two sessions), B = 64 11.72 -> 11.50, B = 32 6.34 -> 6.25, B = 16 3.59 -> 3.27, B = 8 2.366 -> 2.345, but B = 4 1.53 -> 1.67:
// there the chained launches are C3's, 128 workgroups that already leave half the chip empty, and twice the launches plus the fork and
// the join cost more than there is to fill. VPX_OPT_SEQ_CHAINS = 2 chains from B = 2 on (tests).
constexpr int SEQ_CHAINS_MIN_B = 8;
static int seq_chains(const vpx_convlstm_desc* d, const RouteChoice& r, hipStream_t stream) {
    if (!on_cell2(r) || g_seq_chains == 0 || d->B < (g_seq_chains == 2 ? 2 : SEQ_CHAINS_MIN_B)) return 1;
    if (g_dry_run) return 2;   // (no HIP call: the chains' host-side work runs, on the caller's stream handle)
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) { (void)hipGetLastError(); return 1; }
    return st == hipStreamCaptureStatusNone ? 2 : 1;
}
// The side stream of a device and the two events of a fork / join, created on first use and kept. Non-blocking: the caller's stream may be
// the null stream, which every blocking stream synchronises with launch by launch. The events are shared by every call on the device, so
// a record and the wait that belongs to it are issued under the lock (a wait takes the event's record as of that moment).
struct SeqSide { hipStream_t stream; hipEvent_t fork, join; bool made; };
static std::mutex g_side_mutex;
static SeqSide g_side[64];
static int seq_side(SeqSide*& out) {
    int dev = 0;
    VPX_CHECK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) { set_error("vpx_convlstm_seq_fwd: device %d beyond the side-stream table", dev); return VPX_ERR_UNSUPPORTED; }
    std::lock_guard<std::mutex> lock(g_side_mutex);
    SeqSide& sd = g_side[dev];
    if (!sd.made) {
        VPX_CHECK_HIP(hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking));
        VPX_CHECK_HIP(hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming));
        VPX_CHECK_HIP(hipEventCreateWithFlags(&sd.join, hipEventDisableTiming));
        sd.made = true;
    }
    out = &sd;
    return VPX_OK;
}
// `to` goes on only after everything issued to `from` so far
static hipError_t seq_order(hipEvent_t ev, hipStream_t from, hipStream_t to) {
    std::lock_guard<std::mutex> lock(g_side_mutex);
    const hipError_t e = hipEventRecord(ev, from);
    return e != hipSuccess ? e : hipStreamWaitEvent(to, ev, 0);
}
extern "C" int vpx_convlstm_seq_chains(const vpx_convlstm_desc* d, int x_present, void* stream) {
    ConvLSTMLayout L;
    if (check_convlstm_desc(d) != VPX_OK || convlstm_layout(d, L) != VPX_OK) return 0;
    return seq_chains(d, convlstm_route(d, L, x_present != 0), (hipStream_t)stream);
}
extern "C" int vpx_convlstm_seq_fwd(const vpx_convlstm_desc* d, const float* x, const float* h0, const float* c0,
                                    const float* W, const float* bias, const float* Wci, const float* Wcf, const float* Wco,
                                    float* out, float* hT, float* cT, void* reserve, size_t reserve_bytes, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
    int rc = check_convlstm_desc(d);
    if (rc != VPX_OK) return rc;
    ConvLSTMLayout L;
    if ((rc = convlstm_layout(d, L)) != VPX_OK) return rc;
    if (!W || !out) { set_error("vpx_convlstm_seq_fwd: W and out must not be NULL"); return VPX_ERR_ARG; }
    if ((Wci || Wcf || Wco) && !(Wci && Wcf && Wco)) { set_error("vpx_convlstm_seq_fwd: peephole tensors must be given together"); return VPX_ERR_ARG; }
    FwdCtx c{};
    c.d = d; c.L = &L; c.stream = (hipStream_t)stream_; c.HW = (size_t)d->H * d->W;
    c.x = x; c.h0 = h0; c.c0 = c0; c.W = W; c.bias = bias; c.wci = Wci; c.wcf = Wcf; c.wco = Wco;
    c.out = out; c.hT = hT; c.cT = cT;
    c.save = (d->flags & VPX_FLAG_SAVE_FOR_BWD) != 0; c.x_split = (d->flags & VPX_FLAG_X_SPLIT) != 0;
    c.wp = (d->flags & VPX_FLAG_WEIGHTS_PACKED) != 0; c.out_split = (d->flags & VPX_FLAG_OUT_SPLIT) != 0;
    if (c.out_split && !vpx_convlstm_writes_split_output(d)) {
        set_error("vpx_convlstm_seq_fwd: VPX_FLAG_OUT_SPLIT given, but this descriptor's forward writes fp32 only (vpx_convlstm_writes_split_output)"); return VPX_ERR_ARG;
    }
    if (c.x_split && !vpx_convlstm_takes_split_input(d)) {
        set_error("vpx_convlstm_seq_fwd: VPX_FLAG_X_SPLIT given, but this descriptor's forward takes fp32 input (vpx_convlstm_takes_split_input)"); return VPX_ERR_ARG;
    }
    c.res = convlstm_reserve(d, L, reserve);
    if (c.save && (!reserve || reserve_bytes < c.res.bytes)) { set_error("vpx_convlstm_seq_fwd: reserve too small (%zu < %zu)", reserve_bytes, c.res.bytes); return VPX_ERR_WORKSPACE; }
    if (!workspace || workspace_bytes < vpx_convlstm_workspace_bytes(d)) {
        set_error("vpx_convlstm_seq_fwd: workspace too small (%zu < %zu)", workspace_bytes, vpx_convlstm_workspace_bytes(d)); return VPX_ERR_WORKSPACE;
    }
    c.r = convlstm_route(d, L, x != nullptr);
    c.hoist_q = route_hoists_on_convq(d, c.r, c.hq);
    Carver ws(workspace, workspace_bytes);
    carve_fwd(ws, d, L, c.r, c.hoist_q ? &c.hq : nullptr, c.ws);
    VPX_CHECK_CARVE(ws, "vpx_convlstm_seq_fwd");
    if (d->layout == VPX_LAYOUT_NCHW && (rc = stage_in_nchw(c)) != VPX_OK) return rc;
    gate_positions(d->gate_order, c.gp);
    switch (c.r.route) {   // the route's weight packs (skipped where the caller's workspace still holds them) and operand conversions
        case Route::FUSED: case Route::KSPLIT: case Route::HOIST: rc = gen1_pack(c); break;
        case Route::CELL3: rc = cell3_pack(c); break;
        case Route::CELL2: case Route::C3: rc = cell2_pack(c); break;
    }
    if (rc != VPX_OK) return rc;
    if ((c.r.route == Route::HOIST || c.r.route == Route::CELL3) && c.x && (rc = hoisted_projection(c)) != VPX_OK) return rc;
    // ---- time loop: one fused conv + gate + state-update launch per step (KSPLIT, HOIST: a convolution and the pointwise kernel) ----
    // CELL2, C3: the batch as two chains of such launches (seq_chains), chain 1 forked from the caller's stream here and joined below
    Chain chain[2] = {{0, d->B, c.stream}, {0, 0, c.stream}};
    const int nchain = seq_chains(d, c.r, c.stream);
    SeqSide* side = nullptr;
    if (nchain == 2) {
        chain[0].B = (d->B + 1) / 2;
        chain[1].b0 = chain[0].B; chain[1].B = d->B - chain[0].B;
        if (!g_dry_run) {
            if ((rc = seq_side(side)) != VPX_OK) return rc;
            VPX_CHECK_HIP(c5_flush_packs(c.stream));   // (C3's packs wait for the first launch: chain 1 must find them behind the fork)
            VPX_CHECK_HIP(seq_order(side->fork, c.stream, side->stream));
            chain[1].stream = side->stream;
        }
    }
    for (int t = 0; t < d->T && rc == VPX_OK; ++t)
        for (int k = 0; k < nchain && rc == VPX_OK; ++k) {   // A(t), B(t), A(t + 1), ...: neither queue runs dry on the host side
            const Chain& ch = chain[k];
            const ConvLSTMStepArgs ea = step_args(c, t, ch);
            switch (c.r.route) {
                case Route::FUSED: rc = fused_step(c, t, ea); break;
                case Route::KSPLIT: rc = ksplit_step(c, t, ea); break;
                case Route::HOIST: rc = hoist_step(c, t, ea); break;
                case Route::CELL3: rc = cell3_step(c, t, ea); break;
                case Route::CELL2: case Route::C3: rc = cell2_step(c, t, ea, ch); break;
            }
        }
    if (side) {   // also after a failed launch: nothing of the call stays outstanding outside the caller's stream
        const hipError_t ej = seq_order(side->join, side->stream, c.stream);
        if (rc == VPX_OK) VPX_CHECK_HIP(ej);
    }
    if (rc != VPX_OK) return rc;
    // ---- final states ----
    const int B = d->B, T = d->T, Ch = d->Ch;
    if (c.cT && c.save)
        VPX_CHECK_HIP(vpx_memcpy_async(c.cT, c.res.cs + (size_t)(T - 1) * L.n_state, L.n_state * sizeof(float), hipMemcpyDeviceToDevice, c.stream));
    if (c.hT && !c.out_split)
        VPX_CHECK_HIP(vpx_memcpy2d_async(c.hT, c.HW * Ch * sizeof(float), c.out + (size_t)(T - 1) * c.HW * Ch,
                                       (size_t)T * c.HW * Ch * sizeof(float), c.HW * Ch * sizeof(float), B, hipMemcpyDeviceToDevice, c.stream));
    if (d->layout == VPX_LAYOUT_NCHW) {
        VPX_CHECK_HIP(launch_nhwc_to_nchw(c.out, out, B * T, Ch, d->H, d->W, c.stream));
        if (hT) VPX_CHECK_HIP(launch_nhwc_to_nchw(c.hT, hT, B, Ch, d->H, d->W, c.stream));
        if (cT) VPX_CHECK_HIP(launch_nhwc_to_nchw(c.cT, cT, B, Ch, d->H, d->W, c.stream));
    }
    return VPX_OK;
}

// The plan of a call (include/vpx.h): the layout, the route and the backward's choice as the calls compute them, nothing launched or carved
extern "C" int vpx_convlstm_plan(const vpx_convlstm_desc* d, int x_present, int want_dx, int want_dW, vpx_convlstm_plan_info* out) {
    int rc = check_convlstm_desc(d);
    if (rc != VPX_OK) return rc;
    if (!out) { set_error("vpx_convlstm_plan: out is NULL"); return VPX_ERR_ARG; }
    ConvLSTMLayout L;
    if ((rc = convlstm_layout(d, L)) != VPX_OK) return rc;
    const RouteChoice r = convlstm_route(d, L, x_present != 0);
    ConvQProblem hq;
    *out = vpx_convlstm_plan_info{};
    out->route = (int)r.route; out->qform = r.qform; out->c3nt = r.c3nt;
    out->mw = r.route == Route::FUSED ? L.mw : 0;
    out->ksplit = r.route == Route::KSPLIT ? L.split : 0;   // (HOIST launches nothing with L.split: its steps split by hh_split)
    out->hh_split = r.route == Route::HOIST ? L.hh_split : 0;
    out->hoist_convq = x_present && route_hoists_on_convq(d, r, hq) ? 1 : 0;   // (without x the entry point runs no projection)
    out->cell2x = r.route == Route::CELL2 && cell2_step_on_x(r.qform) ? 1 : 0;
    if (d->flags & VPX_FLAG_SAVE_FOR_BWD) convlstm_bwd_plan(d, L, x_present != 0, want_dx != 0, want_dW != 0, out);
    return VPX_OK;
}
