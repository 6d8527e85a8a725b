// stlstm_bwd_api.hip — vpx_stlstm_step_bwd: backward of one ST-LSTM cell step (predrnn.py:57-83), explicit instead of
// autograd. d(pre-activations) of all seven gate blocks live in ONE tensor dG7 [B,HW,7Ch] ordered
// (i,f,g | o | i',f',g') so that Wh's rows are its first 4Ch channels, Wm's rows its last 3Ch, and Wx's row blocks the
// permutation {0,1,2,6,3,4,5}; convolution sources are channel slices of it (ConvSeg.ld).
//   A  pointwise: dh_new -> d(o pre-act) [dG7 block 3], d conv_last
//   B  dgrad conv_o (k x k) + dgrad conv_last (1 x 1, accumulate) -> grads of c_new / m_new through mem
//   C  pointwise: gate groups -> dG7 blocks 0-2, 4-6; dc; direct part of dm
//   D  dgrad: dx (3 segments over Wx), dh (Wh), dm += (Wm)
//   E  wgrad x5 (K-slice slabs + reduce): Wo, Wlast, Wx (row-block map), Wh, Wm
#include "vpx_host.h"

using namespace vpx;

namespace {

struct STBwdLayout {
    int taps, Ch, Cin;
    size_t n_state, n_x, n_g7;
    // dgrad plans: stage tables + chunk counts + N tiles
    struct DG { int nstage, chunks, tiles, ng, ksplit, mw; ConvStage stage[MAX_STAGE]; size_t wpk; } o, l, x, h, m;
    int n_slices;
    size_t slab_floats;
    // stw (wgrad2.hip): the four k x k weight gradients in one launch on split operands — 5x5, bf16x3, channels in 8s
    bool stw; int stw_pairs, stw_ns;
    // c5 (convq.hip): the k x k data gradients on 16x16-pixel tiles over the split-format dG8, two launches (conv_o's adjoint; dx | dh | dm)
    // slots: conv_o -> c, conv_o -> m, dx, dh, dm. On small grids (< 96 pixel tiles) every slot's K is cut into c5_ks chunks that run
    // as separate jobs writing fp32 partial sums (no atomics), added by sum_partials_kernel (st_pointwise.hip)
    bool c5; int c5_ks[5]; size_t c5_wpk[5][6]; size_t c5_part[5];   // bytes of the chunk packs; floats of a slot's partial buffers (0: none)
};
constexpr int C5_NT = 4;   // 64-column N tiles: 6 jobs x 128 pixel tiles of unequal K balance over the chip (see convq.hip)

// VPX_EXP_ST_WGRAD_GEN1 keeps the first-generation weight-gradient launches (A/B runs, tests)
bool stw_applicable(const vpx_stlstm_desc* d) {
    return d->k == 5 && d->precision == VPX_PREC_BF16X3 && !(d->Ch & 7) && !(d->Cin & 7) && !d->layer_norm && !exp_on(VPX_EXP_ST_WGRAD_GEN1);
}

int mk_dg(STBwdLayout::DG& g, const int* segC, int nseg, int k, int n_out, int prec, long long m_tiles) {
    const int taps = k * k;
    g.ng = plain_groups(n_out, m_tiles);
    g.mw = pick_mw_tiles(m_tiles, plain_tiles_ng(n_out, g.ng), prec);  // 8-wave form when the grid stays large
    if (g.mw > 1 && !conv_fits_lds(segC, nseg, k, k, g.ng, prec, g.mw)) g.mw = 1;   // (... and fits LDS)
    if (!conv_fits_lds(segC, nseg, k, k, g.ng, prec, g.mw)) return -1;
    g.nstage = build_stages(g.stage, &g.chunks, segC, nseg, taps, pick_stage_channels(segC, nseg, k, k, g.ng, prec, g.mw), prec);
    if (g.nstage < 0) return -1;
    g.tiles = plain_tiles_ng(n_out, g.ng);
    g.ksplit = pick_ksplit(m_tiles * g.tiles, g.nstage, true);  // 16x16 maps: 64 pixel tiles per launch, K = gates*Ch*k*k is long
    g.wpk = packed_weight_bytes(g.tiles, g.chunks, g.ng, prec) / 4;
    return 0;
}

int st_bwd_layout(const vpx_stlstm_desc* d, STBwdLayout& L) {
    const int Ch = d->Ch, Cin = d->Cin;
    L.taps = d->k * d->k; L.Ch = Ch; L.Cin = Cin;
    L.n_state = (size_t)d->B * d->H * d->W * Ch;
    L.n_x = (size_t)d->B * d->H * d->W * Cin;
    L.n_g7 = L.n_state * (stw_applicable(d) ? 8 : 7);   // the one-launch weight gradient keeps d conv_last as an eighth block
    const int s1[1] = {Ch}, s3[3] = {3 * Ch, Ch, 3 * Ch}, s4[1] = {4 * Ch}, s3m[1] = {3 * Ch};
    const int pr = d->precision;
    const long long mt = (long long)d->B * ((d->W + TILE_W - 1) / TILE_W) * ((d->H + TILE_H - 1) / TILE_H);
    if (mk_dg(L.o, s1, 1, d->k, 2 * Ch, pr, mt) || mk_dg(L.l, s1, 1, 1, 2 * Ch, pr, mt) || mk_dg(L.x, s3, 3, d->k, Cin, pr, mt) ||
        mk_dg(L.h, s4, 1, d->k, Ch, pr, mt) || mk_dg(L.m, s3m, 1, d->k, Ch, pr, mt)) {
        set_error("stlstm bwd: too many channel stages (Ch=%d)", Ch);
        return VPX_ERR_UNSUPPORTED;
    }
    const int tiles = ((d->W + TILE_W - 1) / TILE_W) * ((d->H + TILE_H - 1) / TILE_H);
    long long items = (long long)d->B * tiles;
    L.n_slices = (int)(items < 32 ? items : 32);
    // largest weight-gradient tensor (elements) among Wx, Wh, Wm, Wo, Wlast
    size_t mx = (size_t)7 * Ch * Cin * L.taps;
    if ((size_t)4 * Ch * Ch * L.taps > mx) mx = (size_t)4 * Ch * Ch * L.taps;
    if ((size_t)2 * Ch * Ch * L.taps > mx) mx = (size_t)2 * Ch * Ch * L.taps;
    L.slab_floats = mx * L.n_slices;
    L.stw = stw_applicable(d); L.stw_pairs = 0; L.stw_ns = 0;
    if (L.stw) {
        static thread_local STWArgs sa; static thread_local STWOut so;
        L.stw_pairs = stw_build(sa, so, d->B, d->H, d->W, Cin, Ch);
        if (L.stw_pairs < 1) L.stw = false;
        else {
            L.stw_ns = stw_slices(sa.npairs5, (long long)d->B * ((d->W + 15) / 16) * ((d->H + 3) / 4));
            const size_t need = sa.slab_stride * L.stw_ns;
            if (need > L.slab_floats) L.slab_floats = need;
        }
    }
    // VPX_EXP_ST_DGRAD_GEN1 keeps the first-generation data-gradient launches (A/B runs, tests)
    // From 96 pixel tiles of 16x16 on, a job runs its whole K (the grid rule of the forward launches, stlstm_api.hip; measured training
    // step at 16x16 maps, unsplit c5 vs first-generation K-split data gradients: B = 8 130 vs 78 ms, B = 32 165 vs 136 ms, B = 128 361
    // vs ~405 ms); below, the K of every slot is cut into chunks (VPX_EXP_C5_NO_KSPLIT keeps the first generation there).
    const long long mt16 = (long long)d->B * ((d->H + 15) / 16) * ((d->W + 15) / 16);
    constexpr int C5B_MIN_TILES = 96;
    const bool big = mt16 >= C5B_MIN_TILES || exp_on(VPX_EXP_C5_UNSPLIT);
    L.c5 = L.stw && !exp_on(VPX_EXP_ST_DGRAD_GEN1) && (big || !exp_on(VPX_EXP_C5_NO_KSPLIT));
    if (L.c5) {
        const int K[5] = {Ch, Ch, 7 * Ch, 4 * Ch, 3 * Ch}, Co[5] = {Ch, Ch, Cin, Ch, Ch};
        const int ks_small[5] = {4, 4, 6, 3, 3}, ks_mid[5] = {2, 2, 4, 2, 2};
        for (int i = 0; i < 5; ++i) {
            int ks = big ? 1 : (mt16 <= 16 ? ks_small[i] : ks_mid[i]);
            if (ks > K[i] / 32) ks = K[i] / 32 > 0 ? K[i] / 32 : 1;   // at least four 8-channel stages per chunk
            L.c5_ks[i] = ks;
            for (int k = 0; k < ks; ++k) L.c5_wpk[i][k] = align256(c5_chunk_wpk_bytes(K[i], k, ks, Co[i], C5_NT));
            L.c5_part[i] = ks > 1 ? (size_t)ks * (i == 2 ? L.n_x : L.n_state) : 0;
        }
    }
    return VPX_OK;
}

// ---- the backward workspace: its slots in the order they are taken (see CarveMeasure, vpx_host.h) ----
struct STBwdSlots {
    float *dG7, *dlc, *dcn_conv, *dmn_conv, *dm_scratch;
    float *wpk_o, *wpk_l, *wpk_x, *wpk_h, *wpk_m;   // first generation: the five transposed weight packs
    float *slabs;
    char *x_sp, *st_sp[4];                          // stw: split copies of x; h, m, c_new, m_new
    char* c5w[5][6]; float* c5p[5];                 // c5: the slots' chunk packs and partial sums
    STStage nchw;                                   // h, c, m, c_new, m_new, the five incoming gradients, dh, dc, dm (the last is spare)
};
template <class WS>
void carve_st_bwd(WS& ws, const vpx_stlstm_desc* d, const STBwdLayout& L, STBwdSlots& s) {
    s.dG7 = ws.take(L.n_g7);
    for (float** p : {&s.dlc, &s.dcn_conv, &s.dmn_conv, &s.dm_scratch}) *p = ws.take(L.n_state);
    s.wpk_o = ws.take(L.o.wpk); s.wpk_l = ws.take(L.l.wpk); s.wpk_x = ws.take(L.x.wpk); s.wpk_h = ws.take(L.h.wpk); s.wpk_m = ws.take(L.m.wpk);
    s.slabs = ws.take(L.slab_floats);
    if (L.stw) {
        s.x_sp = (char*)ws.take(L.n_x);
        for (auto& q : s.st_sp) q = (char*)ws.take(L.n_state);
    }
    if (L.c5) for (int i = 0; i < 5; ++i) {
        for (int k = 0; k < L.c5_ks[i]; ++k) s.c5w[i][k] = (char*)ws.take(L.c5_wpk[i][k] / 4);
        if (L.c5_part[i]) s.c5p[i] = ws.take(L.c5_part[i]);
    }
    carve_st_stage(ws, d, L.n_x, L.n_state, true, 14, s.nchw);   // 10 inputs + 3 outputs listed for st_stage_in, + the spare the query always counted
}

}  // namespace

namespace vpx {
size_t stlstm_bwd_workspace_bytes(const vpx_stlstm_desc* d) {
    STBwdLayout L;
    if (st_bwd_layout(d, L) != VPX_OK) return 0;
    CarveMeasure m; STBwdSlots s{};
    carve_st_bwd(m, d, L, s);
    return m.off;
}
}  // namespace vpx

namespace {

// ---- the form of a call, decided once from the layout, the requested gradients and the shadows ----
// stw: dG7 in the split operand format with d conv_last as an eighth block, all k x k weight gradients in one launch (or deferred);
// c5: the k x k data gradients on the 16x16-tile kernel; defer: this step's dG8 goes to the caller's slab slot, no weight gradient here
struct STBwdChoice { bool stw, c5, defer; };
STBwdChoice st_bwd_choice(const STBwdLayout& L, bool defer, float* const dW[5]) {
    const bool stw = L.stw && (defer || (dW[0] && dW[1] && dW[2] && dW[3] && dW[4]));
    return {stw, L.c5 && stw, defer};
}

}  // namespace

namespace vpx {
// the backward half of vpx_stlstm_plan (stlstm_api.hip): the layout and the choice as a call computes them
int stlstm_bwd_plan(const vpx_stlstm_desc* d, bool all_weight_grads, vpx_stlstm_plan_info* out) {
    STBwdLayout L;
    const int rc = st_bwd_layout(d, L);
    if (rc != VPX_OK) return rc;
    float* const some = reinterpret_cast<float*>(out);   // (any non-NULL address: the choice asks which gradients are wanted, no more)
    float* const dW[5] = {some, some, some, some, all_weight_grads ? some : nullptr};
    const STBwdChoice r = st_bwd_choice(L, false, dW);
    out->stw = r.stw; out->c5 = r.c5; out->n_slices = L.n_slices; out->stw_ns = L.stw_ns;
    const STBwdLayout::DG* dg[5] = {&L.o, &L.l, &L.x, &L.h, &L.m};
    for (int i = 0; i < 5; ++i) { out->c5_ks[i] = r.c5 ? L.c5_ks[i] : 0; out->dg_ksplit[i] = dg[i]->ksplit; out->dg_mw[i] = dg[i]->mw; }
    return VPX_OK;
}
}  // namespace vpx

namespace {

// ---- what every stage's functions see of a call ----
struct STBwdCtx {
    const vpx_stlstm_desc* d; const STBwdLayout* L; STBwdChoice r;
    STBwdTensors t;      // native layout (NHWC): the caller's tensors or their staged copies
    STBwdSlots ws; STReserve res; STSplitShadows sh;
    hipStream_t stream; size_t HW;
    bool packed;         // `workspace` is the one a previous backward call of the SAME cell, weights, shape and set of requested data gradients left
                         // behind — its transposed weight packs are reused (PredRNN: 57 cell steps per training step share four cells' weights)
    float *dG7, *dmn;    // dG7 | dG8: the workspace's or (defer) the caller's slab slot; dm's accumulator: dm or scratch
    int g7s, ldG;        // stw: dG8 = the seven gate blocks + d conv_last (block 7), all in the split format
    C5Plan cp;           // c5: the jobs of the launch being assembled, and the slots whose partial sums it leaves to add
    struct Pending { float* out; const float* part; long long n; int ks, acc; } pend[5];
    int npend;
};

// ---- first-generation pieces ----
ConvPlan plan_for(const STBwdCtx& c, const STBwdLayout::DG& g, int kk, const float* wpk) {
    ConvPlan P{};
    P.prec = c.d->precision;
    P.B = c.d->B; P.H = c.d->H; P.W = c.d->W; P.kh = kk; P.kw = kk;
    set_plan_tiles(P, g.mw);
    P.nstage = g.nstage; memcpy(P.stage, g.stage, sizeof(ConvStage) * g.nstage);
    P.chunks_total = g.chunks; P.a_bytes = conv_a_bytes(g.stage, g.nstage, kk, kk, g.mw); P.wpk = wpk;
    return P;
}
void pack_plain_T(const STBwdCtx& c, PackDesc& pd, const STBwdLayout::DG& g, int taps, int n_out) {
    memcpy(pd.stage, g.stage, sizeof(ConvStage) * g.nstage);
    pd.nstage = g.nstage; pd.chunks_total = g.chunks; pd.prec = c.d->precision; pd.taps = taps;
    fill_plain_pack(pd, n_out, 0, g.ng);
    pd.transposed = 1; pd.flip = 1;
}
// K-split data gradients add their partial sums atomically: destinations that are not accumulated into start at zero
hipError_t split_plan(const STBwdCtx& c, ConvPlan& P, const STBwdLayout::DG& g, float* o0, float* o1, size_t n, bool accumulate) {
    P.ksplit = g.ksplit;
    if (g.ksplit > 1 && !accumulate) {
        hipError_t e = vpx_memset_async(o0, 0, n * sizeof(float), c.stream);
        if (e == hipSuccess && o1) e = vpx_memset_async(o1, 0, n * sizeof(float), c.stream);
        return e;
    }
    return hipSuccess;
}
int c5_job(STBwdCtx& c, int slot, int Co_, float* out, int ld_out, int acc, const float* w, long long s_row, int w_col0, int nrange, const int (*rng)[3]);
// one k x k data gradient: out [B,HW,Co] (+)= conv^T(dG7 ranges; rows of w). rng[i] = {dG7 channel 0, channels, weight row 0}. c5: a job of the
// launch being assembled (slot: its packs and partial sums); else a first-generation launch of its own
int data_grad(STBwdCtx& c, int slot, const STBwdLayout::DG& g, float* wpk, const float* w, int Co, float* out, size_t n, int nrange,
              const int (*rng)[3], bool accumulate) {
    const STBwdLayout& L = *c.L;
    if (c.r.c5) return c5_job(c, slot, Co, out, Co, accumulate ? 1 : 0, w, (long long)Co * L.taps, 0, nrange, rng);
    PackDesc pd{};
    for (int i = 0; i < nrange; ++i) pd.seg[i] = PackSeg{w, (long long)Co * L.taps, L.taps, rng[i][2], rng[i][1]};
    pack_plain_T(c, pd, g, L.taps, Co);
    if (!c.packed) VPX_CHECK_HIP(launch_pack_weights(pd, wpk, c.stream));
    ConvPlan P = plan_for(c, g, c.d->k, wpk);
    P.nseg = nrange;
    for (int i = 0; i < nrange; ++i) P.seg[i] = ConvSeg{c.dG7 + rng[i][0], (long long)(c.HW * c.ldG), rng[i][1], c.ldG, c.g7s};
    PlainEpiArgs ea{};
    ea.Co = Co; ea.split = Co; ea.ng = g.ng; ea.out0 = out; ea.bstride0 = (long long)(c.HW * Co); ea.ld0 = Co;
    ea.accumulate = accumulate ? 1 : 0;
    VPX_CHECK_HIP(split_plan(c, P, g, out, nullptr, n, accumulate));
    VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, g.tiles, c.stream));
    return VPX_OK;
}
// one weight gradient: dW[n_out, C0 + C1, kh, kw] from dG (channel slice [N] of a [.., ldG] tensor) and up to two sources
int run_wgrad(const vpx_stlstm_desc* d, const STBwdLayout& L, const float* dG, int N, int ldG, const float* src0, int C0,
              const float* src1, int C1, int k, const int* rowblk, int blk, int n_out, float* slabs, float* dW,
              hipStream_t stream) {
    WgradArgs wa{};
    wa.T = 1; wa.B = d->B; wa.H = d->H; wa.W = d->W; wa.HW = d->H * d->W; wa.kh = k; wa.kw = k;
    wa.tiles_x = (d->W + TILE_W - 1) / TILE_W; wa.tiles_y = (d->H + TILE_H - 1) / TILE_H;
    wa.N4 = N; wa.Cin = C0; wa.Ch = C1 > 0 ? C1 : 1; wa.Ct = C0 + C1;
    wa.ldG = ldG; wa.blk = blk; wa.n_out = n_out; wa.prec = d->precision;
    if (rowblk) for (int i = 0; i < 8; ++i) wa.rowblk[i] = rowblk[i];
    wa.dG = dG;
    wa.x = src0; wa.x_bstride = (long long)wa.HW * C0; wa.x_tstride = 0;
    wa.hseq = nullptr; wa.h0 = src1;
    wa.n_ctiles = wgrad_make_ctiles(wa.ct, WG_MAX_CTILES, C0, C1, C0);
    if (wa.n_ctiles < 0) { set_error("stlstm bwd: too many channels for the weight-gradient kernel"); return VPX_ERR_UNSUPPORTED; }
    wa.slabs = slabs;
    const int taps = k * k, ns = wgrad_pick_slices(L.n_slices, N, wa.n_ctiles, taps);
    // (no slab clear: every workgroup of every slice stores its full tile, so each slab element is written once)
    VPX_CHECK_HIP(launch_wgrad(wa, ns, stream));
    VPX_CHECK_HIP(launch_wgrad_reduce(slabs, dW, ns, taps, n_out, wa.Ct, stream));
    return VPX_OK;
}

// ---- c5: a data gradient as a job of the launch being assembled (or, K-split, as c5_ks[slot] jobs writing partial sums) ----
// rng[i] = {source channel 0, channels, weight row 0}: the job's K = channel ranges of dG8, each multiplying rows of `w`
int c5_job(STBwdCtx& c, int slot, int Co_, float* out, int ld_out, int acc, const float* w, long long s_row, int w_col0, int nrange,
           const int (*rng)[3]) {
    const STBwdLayout& L = *c.L;
    C5Job full{};
    full.nrange = nrange;
    C5PackRange prf[3] = {};
    for (int i = 0; i < nrange; ++i) {
        full.r_src[i] = 0; full.r_c0[i] = rng[i][0]; full.r_n[i] = rng[i][1];
        prf[i] = C5PackRange{w, (long long)L.taps, s_row, rng[i][2], {w_col0, 0, 0, 0}};   // data gradient: column = the weight's input channel
    }
    full.Co = Co_; full.ld = ld_out; full.accumulate = acc; full.out = out; full.out_bstride = (long long)c.HW * ld_out;
    const int ks = L.c5_ks[slot];
    if (ks == 1) {
        C5Job& j = c.cp.job[c.cp.njobs++];
        j = full; j.wpk = c.ws.c5w[slot][0];
        return c5_prepare_job(j, C5_NT, prf, 0, 1, c.packed, c.stream);
    }
    const long long n = (long long)c.d->B * (long long)c.HW * ld_out;
    for (int kk = 0; kk < ks; ++kk) {   // chunk jobs write partial sums; sum_partials_kernel adds them (onto `out` when acc)
        C5Job& j = c.cp.job[c.cp.njobs++];
        C5PackRange pr[3];
        c5_chunk_job(full, prf, kk, ks, j, pr);
        j.wpk = c.ws.c5w[slot][kk]; j.accumulate = 0; j.out = c.ws.c5p[slot] + (size_t)kk * n;
        const int rcj = c5_prepare_job(j, C5_NT, pr, 0, 1, c.packed, c.stream);
        if (rcj) return rcj;
    }
    c.pend[c.npend++] = STBwdCtx::Pending{out, c.ws.c5p[slot], n, ks, acc};
    return VPX_OK;
}
int c5_flush(STBwdCtx& c) {
    if (c.cp.njobs) VPX_CHECK_HIP(launch_c5(c.cp, C5_NT, c.stream));
    {   // the slots' partial sums in ONE launch (round 5: five 5 us launches per cell step on the small grids)
        float* po[5]; const float* pp[5]; long long pn[5]; int pk[5], pa[5];
        bool vec = true;
        for (int i = 0; i < c.npend; ++i) {
            const STBwdCtx::Pending& p = c.pend[i];
            po[i] = p.out; pp[i] = p.part; pn[i] = p.n; pk[i] = p.ks; pa[i] = p.acc; vec = vec && !(p.n & 3);
        }
        if (vec) VPX_CHECK_HIP(launch_sum_partials_multi(c.npend, po, pp, pn, pk, pa, c.stream));
        else for (int i = 0; i < c.npend; ++i) VPX_CHECK_HIP(launch_sum_partials(c.pend[i].out, c.pend[i].part, c.pend[i].n, c.pend[i].ks, c.pend[i].n, c.pend[i].acc, c.stream));
    }
    c.cp.njobs = 0; c.npend = 0;
    return VPX_OK;
}

// ---- A: through h_new = o * tanh(conv_last(mem)) ----
int stage_out_gate(const STBwdCtx& c) {
    const int Ch = c.d->Ch;
    // (stw: d conv_last goes to dG8 block 7 in the split format for the weight gradient AND to the fp32 tensor dlc for the streaming 1x1 adjoint)
    STBwdOutArgs a{(long long)c.L->n_state, Ch, c.ldG, 3 * Ch, c.r.stw ? 7 * Ch : -1, c.t.g[0], c.res.o, c.res.tl, c.dG7, c.ws.dlc, c.g7s};
    VPX_CHECK_HIP(launch_st_bwd_out(a, c.stream));
    return VPX_OK;
}
// ---- B: grads of mem = [c_new | m_new] through conv_o (k x k) and conv_last (1 x 1) ----
int stage_mem_grads(STBwdCtx& c) {
    const STBwdLayout& L = *c.L; const STBwdSlots& s = c.ws; const STBwdTensors& t = c.t;
    const int Ch = c.d->Ch, ldG = c.ldG; const size_t HW = c.HW;
    int rc;
    if (c.r.c5) {
        const int ro[1][3] = {{3 * Ch, Ch, 0}};
        if ((rc = c5_job(c, 0, Ch, s.dcn_conv, Ch, 0, t.Wo, (long long)2 * Ch * L.taps, 0, 1, ro))) return rc;
        if ((rc = c5_job(c, 1, Ch, s.dmn_conv, Ch, 0, t.Wo, (long long)2 * Ch * L.taps, Ch, 1, ro))) return rc;
        if ((rc = c5_flush(c))) return rc;
    }
    PlainEpiArgs ea{};
    ea.Co = 2 * Ch; ea.split = Ch; ea.ng = L.o.ng;
    ea.out0 = s.dcn_conv; ea.bstride0 = (long long)(HW * Ch); ea.ld0 = Ch;
    ea.out1 = s.dmn_conv; ea.bstride1 = (long long)(HW * Ch); ea.ld1 = Ch;
    if (!c.r.c5) {
        PackDesc pd{};
        pd.seg[0] = PackSeg{t.Wo, (long long)2 * Ch * L.taps, L.taps, 0, Ch};
        pack_plain_T(c, pd, L.o, L.taps, 2 * Ch);
        if (!c.packed) VPX_CHECK_HIP(launch_pack_weights(pd, s.wpk_o, c.stream));
        ConvPlan P = plan_for(c, L.o, c.d->k, s.wpk_o);
        P.nseg = 1; P.seg[0] = ConvSeg{c.dG7 + 3 * Ch, (long long)(HW * ldG), Ch, ldG, c.g7s};
        VPX_CHECK_HIP(split_plan(c, P, L.o, s.dcn_conv, s.dmn_conv, L.n_state, false));
        VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, L.o.tiles, c.stream));
    }
    C1Args c1{};   // conv_last's adjoint: [dc_new | dm_new] += Wlast^T d conv_last
    c1.x[0] = s.dlc; c1.xld[0] = Ch; c1.xc[0] = Ch;
    c1.npix = (long long)c.d->B * (long long)HW;
    c1.w = t.Wlast; c1.w_sn = 1; c1.w_sc = 2 * Ch;
    c1.y[0] = s.dcn_conv; c1.y[1] = s.dmn_conv; c1.yld[0] = c1.yld[1] = Ch; c1.ysplit = Ch; c1.Co = 2 * Ch; c1.accumulate = 1;
    if (c1_applicable(c1, c.d->precision)) {
        VPX_CHECK_HIP(launch_c1(c1, c.stream));   // streaming form (conv1.hip)
        return VPX_OK;
    }
    PackDesc pl{};
    pl.seg[0] = PackSeg{t.Wlast, (long long)2 * Ch, 1, 0, Ch};
    pack_plain_T(c, pl, L.l, 1, 2 * Ch);
    if (!c.packed) VPX_CHECK_HIP(launch_pack_weights(pl, s.wpk_l, c.stream));
    ConvPlan Q = plan_for(c, L.l, 1, s.wpk_l);
    Q.nseg = 1; Q.seg[0] = c.r.stw ? ConvSeg{c.dG7 + 7 * Ch, (long long)(HW * ldG), Ch, ldG, 1} : ConvSeg{s.dlc, (long long)(HW * Ch), Ch, 0};
    ea.accumulate = 1;
    VPX_CHECK_HIP(split_plan(c, Q, L.l, s.dcn_conv, s.dmn_conv, L.n_state, true));
    VPX_CHECK_HIP(launch_conv_plain_f32(Q, ea, L.l.tiles, c.stream));
    return VPX_OK;
}
// ---- C: gate groups ----
int stage_gates(const STBwdCtx& c) {
    const STBwdTensors& t = c.t;
    STBwdGateArgs a{};
    a.npix = (long long)c.d->B * c.HW; a.Ch = c.d->Ch; a.ldG = c.ldG;
    a.gates_c = c.res.gates_c; a.gates_m = c.res.gates_m; a.c = t.c; a.m = t.m;
    a.dcn_ext = t.g[1]; a.dmn_ext = t.g[2]; a.ddc_ext = t.g[3]; a.ddm_ext = t.g[4];
    a.dcn_conv = c.ws.dcn_conv; a.dmn_conv = c.ws.dmn_conv;
    a.dG7 = c.dG7; a.dc = t.dc; a.dm = c.dmn; a.split = c.g7s;
    VPX_CHECK_HIP(launch_st_bwd_gates(a, c.stream));
    return VPX_OK;
}
// ---- D: data gradients dx (three ranges over Wx), dh (Wh), dm += (Wm): c5 — the jobs of ONE launch, longest K first — or first generation ----
int stage_data_grads(STBwdCtx& c) {
    const STBwdLayout& L = *c.L; const STBwdSlots& s = c.ws; const STBwdTensors& t = c.t;
    const int Cin = c.d->Cin, Ch = c.d->Ch;
    // dG8 blocks (i,f,g | o | i',f',g') <-> Wx row blocks 0-2 | 6 | 3-5; Wh's rows are the first 4Ch channels, Wm's the last 3Ch
    const int rx[3][3] = {{0, 3 * Ch, 0}, {3 * Ch, Ch, 6 * Ch}, {4 * Ch, 3 * Ch, 3 * Ch}}, rh[1][3] = {{0, 4 * Ch, 0}}, rm[1][3] = {{4 * Ch, 3 * Ch, 0}};
    int rc;
    c.cp.njobs = 0;
    if (t.dx && (rc = data_grad(c, 2, L.x, s.wpk_x, t.Wx, Cin, t.dx, L.n_x, 3, rx, false))) return rc;
    if (t.dh && (rc = data_grad(c, 3, L.h, s.wpk_h, t.Wh, Ch, t.dh, L.n_state, 1, rh, false))) return rc;
    if (t.dm && (rc = data_grad(c, 4, L.m, s.wpk_m, t.Wm, Ch, c.dmn, L.n_state, 1, rm, true))) return rc;   // onto dm_new_total * f' written by stage C
    return c.r.c5 ? c5_flush(c) : VPX_OK;
}
// ---- E: weight gradients ----
// all four k x k tensors and Wlast in one launch (wgrad2.hip, stw): operands once more in the split format
int stw_wgrads(STBwdCtx& c) {
    const STBwdLayout& L = *c.L; STBwdSlots& s = c.ws; const STBwdTensors& t = c.t;
    const int Cin = c.d->Cin, Ch = c.d->Ch;
    static thread_local STWArgs sa; static thread_local STWOut so;
    if (stw_build(sa, so, c.d->B, c.d->H, c.d->W, Cin, Ch) != L.stw_pairs) { set_error("stlstm bwd: pair table changed"); return VPX_ERR_ARG; }
    const long long npix = (long long)c.d->B * (long long)c.HW;
    if (c.sh.in[0]) s.x_sp = const_cast<char*>(c.sh.in[0]); else VPX_CHECK_HIP(launch_split_convert(t.x, s.x_sp, npix, Cin, c.stream));
    const float* st_src[4] = {t.h, t.m, t.c_new, t.m_new};
    for (int i = 0; i < 4; ++i) {   // the forward's split shadows of h, m, c_new, m_new where the caller kept them
        if (c.sh.in[1 + i]) s.st_sp[i] = const_cast<char*>(c.sh.in[1 + i]);
        else VPX_CHECK_HIP(launch_split_convert(st_src[i], s.st_sp[i], npix, Ch, c.stream));
    }
    sa.g_sp = reinterpret_cast<const char*>(c.dG7);   // written in the split format by stages A and C
    sa.src[0] = STWSrc{s.x_sp, Cin};
    for (int i = 0; i < 4; ++i) sa.src[1 + i] = STWSrc{s.st_sp[i], Ch};
    sa.n_slices = L.stw_ns; sa.slabs = s.slabs;
    for (int i = 0; i < 5; ++i) so.dW[i] = t.dW[i];
    VPX_CHECK_HIP(launch_stw(sa, so, c.stream));
    return VPX_OK;
}
int gen1_wgrads(const STBwdCtx& c) {
    const STBwdTensors& t = c.t; const int Cin = c.d->Cin, Ch = c.d->Ch, k = c.d->k, ldG = c.ldG;
    const int rowblk[8] = {0, 1, 2, 6, 3, 4, 5, 0};
    const struct { float* dW; const float* dG; int N, ldG; const float* src0; int C0; const float* src1; int C1, k; const int* rowblk; int blk; } tab[5] = {
        {t.dW[3], c.dG7 + 3 * Ch, Ch, ldG, t.c_new, Ch, t.m_new, Ch, k, nullptr, 0},    // Wo
        {t.dW[4], c.ws.dlc, Ch, Ch, t.c_new, Ch, t.m_new, Ch, 1, nullptr, 0},           // Wlast
        {t.dW[0], c.dG7, 7 * Ch, ldG, t.x, Cin, nullptr, 0, k, rowblk, Ch},             // Wx (row-block map)
        {t.dW[1], c.dG7, 4 * Ch, ldG, t.h, Ch, nullptr, 0, k, nullptr, 0},              // Wh
        {t.dW[2], c.dG7 + 4 * Ch, 3 * Ch, ldG, t.m, Ch, nullptr, 0, k, nullptr, 0},     // Wm
    };
    for (const auto& w : tab) {
        if (!w.dW) continue;
        const int rc = run_wgrad(c.d, *c.L, w.dG, w.N, w.ldG, w.src0, w.C0, w.src1, w.C1, w.k, w.rowblk, w.blk, w.N, c.ws.slabs, w.dW, c.stream);
        if (rc) return rc;
    }
    return VPX_OK;
}

}  // namespace

extern "C" int vpx_stlstm_step_bwd(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m, const float* c_new,
                                   const float* m_new, const float* Wx, const float* Wh, const float* Wm, const float* Wo, const float* Wlast,
                                   const float* const* ln, const void* reserve, size_t reserve_bytes, const float* dh_new, const float* dc_new,
                                   const float* dm_new, const float* ddelta_c, const float* ddelta_m, float* dx, float* dh, float* dc, float* dm,
                                   float* dWx, float* dWh, float* dWm, float* dWo, float* dWlast, float* const* dln, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
    return vpx_stlstm_step_bwd_ex(d, x, h, c, m, c_new, m_new, Wx, Wh, Wm, Wo, Wlast, ln, reserve, reserve_bytes, dh_new, dc_new, dm_new,
                                  ddelta_c, ddelta_m, dx, dh, dc, dm, dWx, dWh, dWm, dWo, dWlast, dln, workspace, workspace_bytes, stream_, nullptr);
}

extern "C" int vpx_stlstm_step_bwd_ex(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m, const float* c_new,
                                      const float* m_new, const float* Wx, const float* Wh, const float* Wm, const float* Wo, const float* Wlast,
                                      const float* const* ln, const void* reserve, size_t reserve_bytes, const float* dh_new, const float* dc_new,
                                      const float* dm_new, const float* ddelta_c, const float* ddelta_m, float* dx, float* dh, float* dc, float* dm,
                                      float* dWx, float* dWh, float* dWm, float* dWo, float* dWlast, float* const* dln, void* workspace,
                                      size_t workspace_bytes, void* stream_, const vpx_stlstm_shadows* shadows) {
    if (!d) { set_error("stlstm desc is NULL"); return VPX_ERR_ARG; }
    // the split-format shadows (and the deferred weight gradient's dG8 slot with them) exist for NHWC callers only: a request for a
    // deferred weight gradient on reference-layout buffers is refused, not dropped (a caller who passed NULL dW pointers for it would
    // get VPX_OK and no weight gradient at all)
    if (d->layout != VPX_LAYOUT_NHWC && shadows && shadows->dg8_out) {
        set_error("vpx_stlstm_step_bwd_ex: dg8_out (deferred weight gradients) needs VPX_LAYOUT_NHWC"); return VPX_ERR_UNSUPPORTED;
    }
    if ((d->precision < VPX_PREC_F32 || d->precision > VPX_PREC_BF16)) { set_error("stlstm: precision %d not implemented", d->precision); return VPX_ERR_UNSUPPORTED; }
    if (!(d->flags & VPX_FLAG_SAVE_FOR_BWD)) { set_error("vpx_stlstm_step_bwd: desc lacks VPX_FLAG_SAVE_FOR_BWD"); return VPX_ERR_ARG; }
    if (!x || !h || !c || !m || !c_new || !m_new || !Wx || !Wh || !Wm || !Wo || !Wlast || !reserve) {
        set_error("vpx_stlstm_step_bwd: NULL tensor argument");
        return VPX_ERR_ARG;
    }
    STBwdLayout L;
    int rc = st_bwd_layout(d, L);
    if (rc != VPX_OK) return rc;
    if (reserve_bytes < vpx_stlstm_reserve_bytes(d)) { set_error("vpx_stlstm_step_bwd: reserve too small"); return VPX_ERR_WORKSPACE; }
    if (!workspace || workspace_bytes < vpx_stlstm_workspace_bytes(d)) { set_error("vpx_stlstm_step_bwd: workspace too small"); return VPX_ERR_WORKSPACE; }
    STBwdCtx b{};
    b.d = d; b.L = &L; b.stream = (hipStream_t)stream_; b.HW = (size_t)d->H * d->W; b.packed = (d->flags & VPX_FLAG_WEIGHTS_PACKED) != 0;
    b.t = STBwdTensors{x, h, c, m, c_new, m_new, Wx, Wh, Wm, Wo, Wlast, ln, {dh_new, dc_new, dm_new, ddelta_c, ddelta_m},
                       dx, dh, dc, dm, {dWx, dWh, dWm, dWo, dWlast}, dln};
    if (d->layer_norm) {   // unfused LayerNorm path (stlstm_ln_api.hip), the layout adaptation inside it
        if (!ln) { set_error("vpx_stlstm_step_bwd: layer_norm set but ln is NULL"); return VPX_ERR_ARG; }
        return stlstm_ln_bwd(d, b.t, reserve, workspace, workspace_bytes, b.stream);
    }
    if (d->layout == VPX_LAYOUT_NHWC) b.sh = st_shadows_of(shadows);   // an argument of THIS call
    b.r = st_bwd_choice(L, b.sh.dg8 != nullptr, b.t.dW);
    // deferred weight gradients (vpx_stlstm_shadows::dg8_out): this step's dG8 goes to the caller's slab slot in the split format and the
    // five weight gradients are left to ONE vpx_stlstm_wgrad_batch call over all the steps of the cell
    if (b.r.defer && !L.stw) { set_error("vpx_stlstm_step_bwd_ex: dg8_out given, but this descriptor's weight gradients cannot be deferred (vpx_stlstm_defers_wgrad)"); return VPX_ERR_UNSUPPORTED; }
    b.res = stlstm_reserve(d, L, reserve);
    Carver ws(workspace, workspace_bytes);
    carve_st_bwd(ws, d, L, b.ws);
    VPX_CHECK_CARVE(ws, "vpx_stlstm_step_bwd");
    STBwdTensors& t = b.t;
    if ((rc = st_stage_in(d, b.ws.nchw, &t.x, {&t.h, &t.c, &t.m, &t.c_new, &t.m_new, &t.g[0], &t.g[1], &t.g[2], &t.g[3], &t.g[4]}, 10,
                          {&t.dh, &t.dc, &t.dm}, &t.dx, b.stream))) return rc;
    // The one-launch weight gradient wants dG7 in the split operand format: the two pointwise stages then write that format ONLY
    // (the data-gradient convolutions read it without conversion, ConvSeg.split) — no fp32 dG7, no conversion pass.
    b.dG7 = b.r.defer ? reinterpret_cast<float*>(b.sh.dg8) : b.ws.dG7;
    b.dmn = b.t.dm ? b.t.dm : b.ws.dm_scratch;
    b.g7s = b.r.stw ? 1 : 0; b.ldG = (b.r.stw ? 8 : 7) * d->Ch;
    b.cp = c5_plan_of(d->B, d->H, d->W);
    b.cp.src[0] = C5Src{reinterpret_cast<const char*>(b.dG7), (long long)b.HW * b.ldG * 4, b.ldG * 4, 0};
    if ((rc = stage_out_gate(b)) || (rc = stage_mem_grads(b)) || (rc = stage_gates(b)) || (rc = stage_data_grads(b))) return rc;
    if (b.r.stw && !b.r.defer) rc = stw_wgrads(b);
    else if (!b.r.stw) rc = gen1_wgrads(b);
    return rc != VPX_OK ? rc : st_stage_out(d, b.ws.nchw, b.stream);
}

// ---- deferred weight gradients: all the steps of one cell in ONE launch ---------------------------------------------------------
// The one-launch kernel (stw, wgrad2.hip) walks items = (image, 4 x 16-pixel tile); a step's images are just more images. With every
// operand of the T steps in a dense slab [T][B][HW][C] (split format) the batch is the same launch over T * B images: one slab write
// and one slice reduction per cell and training step instead of one per cell STEP (at B = 2..4 per GPU those two were a third of the
// kernel's time, and the per-step results cost autograd one accumulation launch per weight tensor and step).
extern "C" int vpx_stlstm_defers_wgrad(const vpx_stlstm_desc* d) {
    if (!d || d->layout != VPX_LAYOUT_NHWC || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Ch < 1) return 0;
    if (!stw_applicable(d)) return 0;
    static thread_local STWArgs sa; static thread_local STWOut so;
    return stw_build(sa, so, d->B, d->H, d->W, d->Cin, d->Ch) >= 1 ? 1 : 0;
}

extern "C" size_t vpx_stlstm_wgrad_batch_workspace_bytes(const vpx_stlstm_desc* d) {
    if (!vpx_stlstm_defers_wgrad(d)) return 0;
    static thread_local STWArgs sa; static thread_local STWOut so;
    if (stw_build(sa, so, d->B, d->H, d->W, d->Cin, d->Ch) < 1) return 0;
    const int ns = stw_slices(sa.npairs5, (long long)d->B * ((d->W + 15) / 16) * ((d->H + 3) / 4));
    return align256(sa.slab_stride * (size_t)ns * 4) + 512;
}

extern "C" int vpx_stlstm_wgrad_batch(const vpx_stlstm_desc* d, const void* dg8_split, const void* const* src5_split, float* dWx, float* dWh,
                                      float* dWm, float* dWo, float* dWlast, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!vpx_stlstm_defers_wgrad(d)) { set_error("vpx_stlstm_wgrad_batch: not available for this descriptor (vpx_stlstm_defers_wgrad)"); return VPX_ERR_UNSUPPORTED; }
    if (!dg8_split || !src5_split || !dWx || !dWh || !dWm || !dWo || !dWlast) { set_error("vpx_stlstm_wgrad_batch: NULL tensor argument"); return VPX_ERR_ARG; }
    for (int i = 0; i < 5; ++i) if (!src5_split[i]) { set_error("vpx_stlstm_wgrad_batch: source %d is NULL", i); return VPX_ERR_ARG; }
    if ((long long)d->B * ((d->W + 15) / 16) * ((d->H + 3) / 4) > 0x7fffffffll) { set_error("vpx_stlstm_wgrad_batch: too many items"); return VPX_ERR_UNSUPPORTED; }
    const size_t need = vpx_stlstm_wgrad_batch_workspace_bytes(d);
    if (!workspace || workspace_bytes < need) { set_error("vpx_stlstm_wgrad_batch: workspace too small"); return VPX_ERR_WORKSPACE; }
    static thread_local STWArgs sa; static thread_local STWOut so;
    if (stw_build(sa, so, d->B, d->H, d->W, d->Cin, d->Ch) < 1) { set_error("vpx_stlstm_wgrad_batch: pair table"); return VPX_ERR_UNSUPPORTED; }
    const int ns = stw_slices(sa.npairs5, (long long)d->B * ((d->W + 15) / 16) * ((d->H + 3) / 4));
    Carver ws(workspace, workspace_bytes);
    float* slabs = ws.take(sa.slab_stride * (size_t)ns);
    VPX_CHECK_CARVE(ws, "vpx_stlstm_wgrad_batch");
    sa.g_sp = reinterpret_cast<const char*>(dg8_split);
    sa.src[0] = STWSrc{reinterpret_cast<const char*>(src5_split[0]), d->Cin};
    for (int i = 1; i < 5; ++i) sa.src[i] = STWSrc{reinterpret_cast<const char*>(src5_split[i]), d->Ch};
    sa.n_slices = ns; sa.slabs = slabs;
    so.dW[0] = dWx; so.dW[1] = dWh; so.dW[2] = dWm; so.dW[3] = dWo; so.dW[4] = dWlast;
    VPX_CHECK_HIP(launch_stw(sa, so, (hipStream_t)stream_));
    return VPX_OK;
}
