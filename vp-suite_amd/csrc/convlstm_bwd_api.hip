// convlstm_bwd_api.hip — vpx_convlstm_seq_bwd: BPTT through the fused ConvLSTM sequence (include/vpx.h).
// Per step (reverse time): gate-backward (pointwise) -> data-gradient conv (same implicit-GEMM kernel as the forward,
// weights packed transposed + tap-flipped); after the loop one weight-gradient launch over all (t, b) images, a
// K-slice reduction into the reference's OIHW layout, and a column sum for the bias gradient.
#include "vpx_host.h"

using namespace vpx;

// ---- the backward workspace: ONE list of slots, taken in this order by a call's Carver and by the size query's CarveMeasure ----
struct BwdSlots {
    float *wpk, *dG_all, *dh_buf, *dc_buf, *slabs;   // data-gradient weight pack (upper bound over both tilings), dG of all steps, dh / dc carries, wgrad K-slice slabs
    float *db_part, *db_part2, *peep_part[3];        // bias-gradient partials and their second level; per-batch-slice peephole-gradient partials
    char *dG_sp_all, *wpk2;                          // dG of all steps in split operand format; the conv2 weight pack of the data gradient
    char *xsp_w, *hsp_w, *h0sp_w;                    // wgrad2 after a forward on another kernel: split copies of x, the output sequence and h0
    float *bx, *bdx, *bout, *bdout, *st[6], *pp[6];  // NCHW staging: x, dx, out, dout, states (h0,c0,dhT,dcT,dh0,dc0), 6 peephole-sized buffers
};
template <class WS>
static void carve_bwd(WS& ws, const vpx_convlstm_desc* d, const ConvLSTMLayout& L, BwdSlots& s) {
    const int N4 = 4 * d->Ch, Ct = d->Cin + d->Ch, T = d->T;
    s.wpk = ws.take(packed_weight_bytes(L.d_tiles_full, L.d_chunks, 4, d->precision, L.d_qpc) / sizeof(float));
    s.dG_all = ws.take((size_t)T * L.n_state * 4);
    for (float** p : {&s.dh_buf, &s.dc_buf}) *p = ws.take(L.n_state);
    s.slabs = ws.take(L.slab_floats);
    s.db_part = ws.take((size_t)T * GATE_BWD_MAX_SLICES * gate_bwd_blocks(d->H * d->W, d->Ch) * N4);
    s.db_part2 = ws.take((size_t)COLSUM_BLOCKS * N4);
    for (auto& p : s.peep_part) p = ws.take((size_t)GATE_BWD_MAX_SLICES * L.n_peep);
    // forward on the second-generation cell: the gate-backward kernel also writes dG in split operand format and the data
    // gradient runs on the cell2 main loop with a plain epilogue (conv2)
    if (L.v2) {
        s.dG_sp_all = (char*)ws.take((size_t)T * L.n_state * 4);
        s.wpk2 = (char*)ws.take((cell2_packed_bytes(conv2_tiles(Ct), 3 * (N4 / 16)) + 16384 * conv2_tiles(Ct)) / sizeof(float));
    }
    if (wgrad2_wsp(d, L)) {
        s.dG_sp_all = (char*)ws.take((size_t)T * L.n_state * 4);
        s.xsp_w = (char*)ws.take(L.n_x);
        s.hsp_w = (char*)ws.take(L.n_out);
        s.h0sp_w = (char*)ws.take(L.n_state);
    }
    if (d->layout == VPX_LAYOUT_NCHW) {
        for (float** p : {&s.bx, &s.bdx}) *p = ws.take(L.n_x);
        for (float** p : {&s.bout, &s.bdout}) *p = ws.take(L.n_out);
        for (auto& p : s.st) p = ws.take(L.n_state);
        for (auto& p : s.pp) p = ws.take(L.n_peep);
    }
}
size_t vpx::convlstm_bwd_workspace_bytes(const vpx_convlstm_desc* d, const ConvLSTMLayout& L) {
    CarveMeasure m; BwdSlots s{};
    carve_bwd(m, d, L, s);
    return m.off;
}

// ---- the form of a call, decided once from the layout, the present operands and the requested gradients ----
// c2d: the data gradient on conv2 (dG in the split operand format) instead of the first-generation kernel; wsp: the forward ran on
// another kernel, the weight gradient on wgrad2 all the same, on operands this call converts; wgrad: 0 launch_wgrad, 1 wgrad2 on the
// reserve's operands, 2 wgrad2 behind wsp (0 without dW); need_dG_f32: a consumer still reads dG in fp32
struct BwdChoice {
    bool c2d, wsp, need_dx, need_dG_f32;
    int qform, col_start, n_out, wgrad, wgrad_slices, gb_slices;
};
static BwdChoice convlstm_bwd_choice(const vpx_convlstm_desc* d, const ConvLSTMLayout& L, bool x_present, bool want_dx, bool want_dW) {
    BwdChoice r{};
    const int N4 = 4 * d->Ch;
    r.gb_slices = gate_bwd_slices(d->H * d->W, d->Ch, d->B, false);
    r.c2d = L.v2;
    r.wsp = wgrad2_wsp(d, L) && want_dW;
    // data-gradient weights: contraction over the 4Ch gate rows, outputs over [x | h] (or only h) columns
    r.need_dx = want_dx && x_present;
    r.col_start = r.need_dx ? 0 : d->Cin;
    r.n_out = r.need_dx ? d->Cin + d->Ch : d->Ch;
    r.qform = g_mfma_shape == 1 ? 1 : 0;   // conv2's epilogue handles ragged tiles in both forms
    // the weight gradient: wgrad2 where its operands are in the split format (the reserve's after a cell2 forward, or this call's own)
    WgradArgs probe{};
    probe.T = d->T; probe.B = d->B; probe.H = d->H; probe.W = d->W; probe.kh = d->kh; probe.kw = d->kw; probe.N4 = N4; probe.Cin = d->Cin; probe.Ch = d->Ch;
    probe.prec = d->precision;
    probe.a_split = ((L.v2 && d->layout == VPX_LAYOUT_NHWC) || r.wsp) ? 1 : 0;
    probe.g_sp = (r.c2d || r.wsp) ? reinterpret_cast<const char*>(&L) : nullptr;   // (any non-NULL address: the probe asks whether dG comes split, no more)
    probe.n_ctiles = wgrad_make_ctiles(probe.ct, WG_MAX_CTILES, x_present ? d->Cin : 0, d->Ch, d->Cin);
    const bool w2 = want_dW && L.n_slices2 > 0 && wgrad2_applicable(probe);
    r.wgrad = !w2 ? 0 : (r.wsp ? 2 : 1);
    r.wgrad_slices = !want_dW ? 0 : (w2 ? wgrad2_used_slices(probe, L.n_slices2) : L.n_slices);
    // fp32 dG is only written for consumers that still read it (first-generation data- / weight-gradient kernels)
    r.need_dG_f32 = !r.c2d || (want_dW && r.wgrad != 1);
    return r;
}
void vpx::convlstm_bwd_plan(const vpx_convlstm_desc* d, const ConvLSTMLayout& L, bool x_present, bool want_dx, bool want_dW, vpx_convlstm_plan_info* out) {
    const BwdChoice r = convlstm_bwd_choice(d, L, x_present, want_dx, want_dW);
    out->dgrad = r.c2d ? 1 : 0; out->dgrad_qform = r.c2d ? r.qform : 0; out->d_mw = r.c2d ? 0 : L.d_mw; out->dgrad_cols = r.n_out;
    out->wgrad = r.wgrad; out->n_slices = r.wgrad_slices; out->dG_f32 = r.need_dG_f32 ? 1 : 0; out->gate_slices = r.gb_slices;
}

extern "C" int vpx_convlstm_seq_bwd(const vpx_convlstm_desc* d, const float* x, const float* h0, const float* c0,
                                    const float* W, const float* Wci, const float* Wcf, const float* Wco,
                                    const float* out, const void* reserve, size_t reserve_bytes, const float* dout,
                                    const float* dhT, const float* dcT, float* dx, float* dh0, float* dc0, float* dW,
                                    float* db, float* dWci, float* dWcf, float* dWco, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
    int rc = check_convlstm_desc(d);
    if (rc != VPX_OK) return rc;
    ConvLSTMLayout L;
    if ((rc = convlstm_layout(d, L)) != VPX_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (!(d->flags & VPX_FLAG_SAVE_FOR_BWD)) { set_error("vpx_convlstm_seq_bwd: desc lacks VPX_FLAG_SAVE_FOR_BWD"); return VPX_ERR_ARG; }
    if (!W || !out || !reserve) { set_error("vpx_convlstm_seq_bwd: W, out and reserve must not be NULL"); return VPX_ERR_ARG; }
    if (reserve_bytes < vpx_convlstm_reserve_bytes(d)) { set_error("vpx_convlstm_seq_bwd: reserve too small"); return VPX_ERR_WORKSPACE; }
    if (!workspace || workspace_bytes < vpx_convlstm_workspace_bytes(d)) {
        set_error("vpx_convlstm_seq_bwd: workspace too small (%zu < %zu)", workspace_bytes, vpx_convlstm_workspace_bytes(d));
        return VPX_ERR_WORKSPACE;
    }
    const bool peep = Wci || Wcf || Wco;
    if (peep && !(Wci && Wcf && Wco)) { set_error("vpx_convlstm_seq_bwd: peephole tensors must be given together"); return VPX_ERR_ARG; }
    const bool dpeep = dWci || dWcf || dWco;
    if (dpeep && !(dWci && dWcf && dWco && peep)) { set_error("vpx_convlstm_seq_bwd: peephole gradients must be requested together"); return VPX_ERR_ARG; }

    const int B = d->B, T = d->T, Cin = d->Cin, Ch = d->Ch, H = d->H, Wd = d->W;
    const int N4 = 4 * Ch, Ct = Cin + Ch;
    const size_t HW = (size_t)H * Wd;
    Carver ws(workspace, workspace_bytes); BwdSlots s{};
    carve_bwd(ws, d, L, s);
    VPX_CHECK_CARVE(ws, "vpx_convlstm_seq_bwd");
    // peephole gradients: a sum over the batch. With several batch slices every slice accumulates (over the time steps, single
    // owner per element) into its own partial tensor; launch_peep_reduce adds them in a fixed order after the loop
    const BwdChoice ch = convlstm_bwd_choice(d, L, x != nullptr, dx != nullptr, dW != nullptr);
    const int gb_slices = ch.gb_slices;
    const int gb_blocks = gate_bwd_blocks((int)HW, Ch) * gb_slices;  // partial rows per step
    const bool c2d = ch.c2d, wsp = ch.wsp;

    // ---- layout adaptation ----
    const float *xn = x, *h0n = h0, *c0n = c0, *outn = out, *doutn = dout, *dhTn = dhT, *dcTn = dcT;
    const float *wci = Wci, *wcf = Wcf, *wco = Wco;
    float *dxn = dx, *dh0n = dh0, *dc0n = dc0, *dwci = dWci, *dwcf = dWcf, *dwco = dWco;
    if (d->layout == VPX_LAYOUT_NCHW) {
        if (x) { VPX_CHECK_HIP(launch_nchw_to_nhwc(x, s.bx, B * T, Cin, H, Wd, stream)); xn = s.bx; }
        VPX_CHECK_HIP(launch_nchw_to_nhwc(out, s.bout, B * T, Ch, H, Wd, stream)); outn = s.bout;
        if (dout) { VPX_CHECK_HIP(launch_nchw_to_nhwc(dout, s.bdout, B * T, Ch, H, Wd, stream)); doutn = s.bdout; }
        if (h0) { VPX_CHECK_HIP(launch_nchw_to_nhwc(h0, s.st[0], B, Ch, H, Wd, stream)); h0n = s.st[0]; }
        if (c0) { VPX_CHECK_HIP(launch_nchw_to_nhwc(c0, s.st[1], B, Ch, H, Wd, stream)); c0n = s.st[1]; }
        if (dhT) { VPX_CHECK_HIP(launch_nchw_to_nhwc(dhT, s.st[2], B, Ch, H, Wd, stream)); dhTn = s.st[2]; }
        if (dcT) { VPX_CHECK_HIP(launch_nchw_to_nhwc(dcT, s.st[3], B, Ch, H, Wd, stream)); dcTn = s.st[3]; }
        if (dh0) dh0n = s.st[4];
        if (dc0) dc0n = s.st[5];
        if (dx) dxn = s.bdx;
        if (peep) {
            VPX_CHECK_HIP(launch_nchw_to_nhwc(Wci, s.pp[0], 1, Ch, H, Wd, stream));
            VPX_CHECK_HIP(launch_nchw_to_nhwc(Wcf, s.pp[1], 1, Ch, H, Wd, stream));
            VPX_CHECK_HIP(launch_nchw_to_nhwc(Wco, s.pp[2], 1, Ch, H, Wd, stream));
            wci = s.pp[0]; wcf = s.pp[1]; wco = s.pp[2];
        }
        if (dpeep) { dwci = s.pp[3]; dwcf = s.pp[4]; dwco = s.pp[5]; }
    }

    const ConvLSTMReserve res = convlstm_reserve(d, L, const_cast<void*>(reserve));   // (read only)
    const float *gates_all = res.gates, *cs_all = res.cs;
    int gp[4];
    gate_positions(d->gate_order, gp);

    const bool peep_sliced = dpeep && gb_slices > 1;
    if (peep_sliced) {
        for (auto pp_ : s.peep_part) VPX_CHECK_HIP(vpx_memset_async(pp_, 0, (size_t)gb_slices * L.n_peep * sizeof(float), stream));
    } else if (dpeep) {
        VPX_CHECK_HIP(vpx_memset_async(dwci, 0, L.n_peep * sizeof(float), stream));
        VPX_CHECK_HIP(vpx_memset_async(dwcf, 0, L.n_peep * sizeof(float), stream));
        VPX_CHECK_HIP(vpx_memset_async(dwco, 0, L.n_peep * sizeof(float), stream));
    }

    // ---- data-gradient weights: contraction over the 4Ch gate rows, outputs over [x | h] (or only h) columns ----
    const bool need_dx = ch.need_dx;
    const int col_start = ch.col_start, n_out = ch.n_out, qform = ch.qform;
    const int d_tiles = plain_tiles(n_out);
    if (c2d) {
        Conv2Pack pk{W, (long long)L.taps, (long long)Ct * L.taps, n_out, col_start, conv2_tiles(n_out), conv2_gpt(n_out),
                     qform ? cell2_qchunks(N4 / 16) : 3 * (N4 / 16), 1, qform, 0};
        VPX_CHECK_HIP(launch_conv2_pack(pk, s.wpk2, stream));
    } else {
        PackDesc pd{};
        pd.seg[0] = PackSeg{W, (long long)Ct * L.taps, L.taps, 0, N4};
        memcpy(pd.stage, L.d_stage, sizeof(ConvStage) * L.d_nstage);
        pd.nstage = L.d_nstage; pd.chunks_total = L.d_chunks; pd.prec = d->precision; pd.taps = L.taps; pd.qpc = L.d_qpc;
        fill_plain_pack(pd, n_out, col_start);
        pd.transposed = 1; pd.flip = 1;
        VPX_CHECK_HIP(launch_pack_weights(pd, s.wpk, stream));
    }

    const bool need_dG_f32 = ch.need_dG_f32;
    for (int t = T - 1; t >= 0; --t) {
        GateBwdArgs ga{};
        ga.B = B; ga.HW = (int)HW; ga.Ch = Ch;
        memcpy(ga.gate_pos, gp, sizeof(gp));
        ga.gates = gates_all + (size_t)t * L.n_state * 4;
        ga.c_t = cs_all + (size_t)t * L.n_state;
        ga.c_prev = (t > 0) ? cs_all + (size_t)(t - 1) * L.n_state : c0n;
        ga.dh_in = (t == T - 1) ? dhTn : s.dh_buf;
        ga.dout = doutn ? doutn + (size_t)t * HW * Ch : nullptr;
        ga.dout_bstride = (long long)((size_t)T * HW * Ch);
        ga.dc_in = (t == T - 1) ? dcTn : s.dc_buf;
        ga.dc_out = (t == 0 && dc0n) ? dc0n : s.dc_buf;
        ga.wci = wci; ga.wcf = wcf; ga.wco = wco;
        ga.dwci = dpeep ? dwci : nullptr; ga.dwcf = dpeep ? dwcf : nullptr; ga.dwco = dpeep ? dwco : nullptr;
        if (peep_sliced) { ga.dwci = s.peep_part[0]; ga.dwcf = s.peep_part[1]; ga.dwco = s.peep_part[2]; ga.peep_slice_stride = (long long)L.n_peep; }
        ga.dG = need_dG_f32 ? s.dG_all + (size_t)t * L.n_state * 4 : nullptr;
        ga.dG_sp = (c2d || wsp) ? s.dG_sp_all + (size_t)t * L.n_state * 16 : nullptr;
        ga.db_partial = db ? s.db_part + (size_t)t * gb_blocks * N4 : nullptr;
        VPX_CHECK_HIP(launch_gate_bwd(ga, stream));

        float* dh_target = (t > 0) ? s.dh_buf : dh0n;  // at t = 0 the recurrent gradient is dL/dh0 (if requested)
        if ((need_dx || dh_target) && c2d) {
            Conv2Args ca{};
            ca.B = B; ca.H = H; ca.W = Wd; ca.C = N4; ca.Co = n_out; ca.split = need_dx ? Cin : 0;
            ca.src_sp = ga.dG_sp; ca.src_bstride = (long long)(HW * N4 * 4);
            ca.wpk = s.wpk2; ca.qform = qform;
            ca.out0 = need_dx ? dxn + (size_t)t * HW * Cin : nullptr;
            ca.bstride0 = (long long)((size_t)T * HW * Cin); ca.ld0 = Cin;
            ca.out1 = dh_target; ca.bstride1 = (long long)(HW * Ch); ca.ld1 = Ch;
            VPX_CHECK_HIP(launch_conv2(ca, stream));
        } else if (need_dx || dh_target) {
            ConvPlan P{};
            P.B = B; P.H = H; P.W = Wd; P.kh = d->kh; P.kw = d->kw;
            set_plan_tiles(P, L.d_mw);
            P.nseg = 1;
            P.seg[0] = ConvSeg{ga.dG, (long long)(HW * N4), N4, 0};
            P.nstage = L.d_nstage;
            memcpy(P.stage, L.d_stage, sizeof(ConvStage) * L.d_nstage);
            P.chunks_total = L.d_chunks; P.prec = d->precision; P.qpc = L.d_qpc;
            P.a_bytes = conv_a_bytes(L.d_stage, L.d_nstage, d->kh, d->kw, L.d_mw);
            P.wpk = s.wpk;
            PlainEpiArgs ea{};
            ea.Co = n_out; ea.ng = plain_groups(n_out);
            ea.split = need_dx ? Cin : 0;
            ea.out0 = need_dx ? dxn + (size_t)t * HW * Cin : nullptr;
            ea.bstride0 = (long long)((size_t)T * HW * Cin); ea.ld0 = Cin;
            ea.out1 = dh_target; ea.bstride1 = (long long)(HW * Ch); ea.ld1 = Ch;
            VPX_CHECK_HIP(launch_conv_plain_f32(P, ea, d_tiles, stream));
        }
    }
    if (dxn && !xn) { set_error("vpx_convlstm_seq_bwd: dx requested but x is NULL"); return VPX_ERR_ARG; }
    if (peep_sliced)
        VPX_CHECK_HIP(launch_peep_reduce(s.peep_part[0], s.peep_part[1], s.peep_part[2], dwci, dwcf, dwco, gb_slices, (long long)L.n_peep, stream));

    // ---- weight gradient over all (t, b) images ----
    if (dW) {
        WgradArgs wa{};
        wa.T = T; wa.B = B; wa.H = H; wa.W = Wd; wa.HW = (int)HW; wa.kh = d->kh; wa.kw = d->kw;
        wa.tiles_x = (Wd + TILE_W - 1) / TILE_W; wa.tiles_y = (H + TILE_H - 1) / TILE_H;
        wa.N4 = N4; wa.Cin = Cin; wa.Ch = Ch; wa.Ct = Ct; wa.prec = d->precision;
        wa.dG = s.dG_all;
        wa.x = xn; wa.x_bstride = (long long)((size_t)T * HW * Cin); wa.x_tstride = (long long)(HW * Cin);
        wa.hseq = outn; wa.h_bstride = (long long)((size_t)T * HW * Ch); wa.h_tstride = (long long)(HW * Ch);
        wa.h0 = h0n;
        wa.n_ctiles = wgrad_make_ctiles(wa.ct, WG_MAX_CTILES, xn ? Cin : 0, Ch, Cin);  // no input tensor: its columns stay zero
        if (L.v2 && d->layout == VPX_LAYOUT_NHWC) {
            // the forward ran on the second-generation cell: x, h_0 and h_t sit in the reserve in split operand format
            wa.a_split = 1;
            wa.x_sp = xn ? res.x_sp : nullptr; wa.x_sp_bstride = (long long)((size_t)T * HW * Cin * 4); wa.x_sp_tstride = (long long)(HW * Cin * 4);
            wa.h0_sp = h0n ? res.h0_sp : nullptr;
            wa.h_sp = res.h_sp; wa.h_sp_bstride = (long long)(HW * Ch * 4); wa.h_sp_tstride = (long long)(L.n_state * 4);
        }
        if (wsp) {   // operands in split form, laid out like x / out ([B][T][HW][C]); conversions are one pass each over small tensors
            if (xn) VPX_CHECK_HIP(launch_split_convert(xn, s.xsp_w, (long long)B * T * (long long)HW, Cin, stream));
            VPX_CHECK_HIP(launch_split_convert(outn, s.hsp_w, (long long)B * T * (long long)HW, Ch, stream));
            if (h0n) VPX_CHECK_HIP(launch_split_convert(h0n, s.h0sp_w, (long long)B * (long long)HW, Ch, stream));
            wa.a_split = 1;
            wa.x_sp = xn ? s.xsp_w : nullptr; wa.x_sp_bstride = (long long)((size_t)T * HW * Cin * 4); wa.x_sp_tstride = (long long)(HW * Cin * 4);
            wa.h0_sp = h0n ? s.h0sp_w : nullptr;
            wa.h_sp = s.hsp_w; wa.h_sp_bstride = (long long)((size_t)T * HW * Ch * 4); wa.h_sp_tstride = (long long)(HW * Ch * 4);
        }
        wa.slabs = s.slabs;
        // every launched tile stores all of its slab elements; only the skipped x columns need a clear
        if (!xn) VPX_CHECK_HIP(vpx_memset_async(s.slabs, 0, L.slab_floats * sizeof(float), stream));
        wa.g_sp = (c2d || wsp) ? s.dG_sp_all : nullptr;
        int ns_used = L.n_slices, tail_col0 = Ct, tail_slices = L.n_slices;
        if (ch.wgrad) VPX_CHECK_HIP(launch_wgrad2(wa, L.n_slices2, &ns_used, &tail_col0, &tail_slices, stream));
        else VPX_CHECK_HIP(launch_wgrad(wa, L.n_slices, stream));
        VPX_CHECK_HIP(launch_wgrad_reduce_tail(s.slabs, dW, ns_used, L.taps, N4, Ct, tail_col0, tail_slices, stream));
    }
    if (db)  // block partials from the gate-backward kernel, summed in a fixed order
        VPX_CHECK_HIP(launch_colsum(s.db_part, nullptr, 0.f, nullptr, db, s.db_part2, (long long)T * gb_blocks, N4, stream));
    if (d->layout == VPX_LAYOUT_NCHW) {
        if (dx) VPX_CHECK_HIP(launch_nhwc_to_nchw(dxn, dx, B * T, Cin, H, Wd, stream));
        if (dh0) VPX_CHECK_HIP(launch_nhwc_to_nchw(dh0n, dh0, B, Ch, H, Wd, stream));
        if (dc0) VPX_CHECK_HIP(launch_nhwc_to_nchw(dc0n, dc0, B, Ch, H, Wd, stream));
        if (dpeep) {
            VPX_CHECK_HIP(launch_nhwc_to_nchw(dwci, dWci, 1, Ch, H, Wd, stream));
            VPX_CHECK_HIP(launch_nhwc_to_nchw(dwcf, dWcf, 1, Ch, H, Wd, stream));
            VPX_CHECK_HIP(launch_nhwc_to_nchw(dwco, dWco, 1, Ch, H, Wd, stream));
        }
    }
    return VPX_OK;
}
