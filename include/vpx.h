/*
 * vpx.h — C ABI of libvpx_hip.so: the MI355X (gfx950) implementation of vp-suite's spatiotemporal recurrent hot path.
 *
 * The reference (AIS-Bonn/vp-suite) has NO native/FFI layer: its hot path is a sequence of ATen calls issued from
 * Python. Each entry point below therefore replaces one Python-level callable of the reference; the
 * binding a maintainer adds is a ctypes stub. All pointers are DEVICE pointers (hipMalloc'd / torch
 * CUDA tensors), fp32 unless stated. The library never allocates, never synchronises and enqueues everything on the
 * `stream` argument (a hipStream_t passed as void*; NULL = default stream). The caller owns every buffer including
 * workspace and reserve. Return value: 0 = OK, negative = error (message via vpx_last_error(), thread-local).
 *
 * Entry point                      replaces (reference file:line)
 * -------------------------------  -----------------------------------------------------------------------------
 * vpx_convlstm_seq_fwd / _bwd      model_blocks.ConvLSTM.forward            vp_suite/model_blocks/conv_lstm_hzzone.py:38-70
 *                                  ConvLSTMCell.forward (T=1, IFOG)         vp_suite/model_blocks/conv_lstm_ndrplz.py:28-43
 *                                  ConvLSTM(ndrplz) per-layer time loop     vp_suite/model_blocks/conv_lstm_ndrplz.py:112-121
 * vpx_stlstm_step_fwd / _bwd       SpatioTemporalLSTMCell.forward           vp_suite/model_blocks/predrnn.py:57-83
 * vpx_acstlstm_step_fwd / _bwd     ActionConditionalSpatioTemporalLSTMCell.forward  vp_suite/model_blocks/predrnn.py:139-169
 * vpx_trajgru_seq_fwd / _bwd       TrajGRU.forward (time loop, warps, gates)        vp_suite/model_blocks/traj_gru.py:164-214
 * vpx_decouple_fwd / _bwd          adapter + normalize + |cos| + mean       vp_suite/models/predrnn_v2.py:197-198,209-211
 * vpx_conv2d_nhwc_fwd / _bwd       F.conv2d 1x1 / kxk "same", stride 1      vp_suite/models/predrnn_v2.py:223 (conv_last)
 * vpx_conv2d_ex_fwd / _bwd         Conv2d / ConvTranspose2d + LeakyReLU     vp_suite/models/precipitation_nowcasting/ef_blocks.py:15-49
 * vpx_mse_loss                     MSE measure + loss provider              vp_suite/base/base_measure.py:55-57, measure/loss_provider.py:48-51
 * vpx_adam_step                    torch.optim.Adam(model.parameters(), lr)  vp_suite/vpsuite.py:353, base/base_model.py:174-176
 * vpx_grad_stats                   total_norm of torch.nn.utils.clip_grad_norm_, max |g|, non-finite count   (new: the reference never clips)
 * vpx_adam_step_clipped            clip_grad_norm_ / clip_grad_value_ + Adam step, optional skip of a non-finite step   (new)
 * vpx_pixel_measures_fwd / _bwd    MSE, L1, SmoothL1, PSNR per frame         vp_suite/measure/image_wise.py:19-71
 * vpx_ssim_fwd / _bwd              SSIM per frame (piqa defaults)           vp_suite/measure/image_wise.py:99-117
 * vpx_lpips_fwd (+ stem, maxpool, head)  LPIPS per frame on AlexNet weights the caller brings  vp_suite/measure/image_wise.py (LPIPS)
 * vpx_lpips_fwd_train / _bwd (+ stem, maxpool, head _bwd)  the same as a training loss: gradient to the prediction
 * vpx_fvd_features (+ conv3d_same, maxpool3d_same, fvd_head) / vpx_frechet_distance  FVD on I3D weights the caller brings  vp_suite/measure/fvd/fvd.py
 * vpx_groupnorm_fwd / _bwd         GroupNorm + LeakyReLU (DCGAN layers)    vp_suite/model_blocks/conv.py, model_blocks/phydnet.py
 * vpx_phycell_correct_fwd / _bwd   PhyCell_Cell prediction-correction       vp_suite/model_blocks/phydnet.py (PhyCell_Cell.forward)
 * vpx_moment_loss_fwd / _bwd       K2M + moment regularisation loss         vp_suite/models/phydnet.py (PhyDNet.forward)
 * vpx_sigmoid_head_fwd / _bwd      sigmoid output + stack of frames         vp_suite/models/phydnet.py (encoder_fwd, forward)
 * vpx_rconv_fwd / _bwd             Conv2d / Conv3d, padding_mode='replicate'; time3ds  vp_suite/model_blocks/conv.py:9-55, models/unet3d.py:45
 * vpx_bn_relu_fwd / _bwd           BatchNorm + ReLU (+ MaxPool3d (1,2,2))   vp_suite/model_blocks/conv.py:22-27, models/unet3d.py:29
 * vpx_dense_fwd / _bwd             nn.Linear (+ ReLU), strided rows         vp_suite/models/lstm.py:41,45,50 (to_linear, action_inflate, from_linear)
 * vpx_lstm_cell_fwd / _bwd         nn.LSTMCell.forward                      vp_suite/models/lstm.py:46-49,95,108
 * vpx_replicate_pad_fwd / _bwd     padding_mode="replicate" of a strided Conv2d   vp_suite/models/lstm.py:30-31 (enc2, enc3)
 * vpx_resize_bilinear_fwd / _bwd   TF.Resize at the decoder's end, differentiable  vp_suite/models/lstm.py:57
 * vpx_mmnist_frames                MovingMNISTOnTheFly.__getitem__ (a batch) vp_suite/datasets/mmnist_on_the_fly.py:78-104,133-147
 * vpx_frames_preprocess            VPDataset.preprocess (a batch of stored sequences)  vp_suite/base/base_dataset.py:233-273, datasets/mmnist.py:56-57
 * vpx_clips_preprocess             the same for windows of long clips       vp_suite/datasets/kitti_raw.py:77-95, caltech_pedestrian.py:69-86
 * vpx_clips_preprocess_var         the same for clips of mixed frame sizes  vp_suite/datasets/human36m.py:30,80-83 (the resize at load), physics101.py, synpick.py
 * vpx_frames_postprocess           VPDataset.postprocess                   vp_suite/base/base_dataset.py:286-297
 * vpx_actions_gather               the action rows of a batch of stored sequences  vp_suite/datasets/bair.py:60-61
 * vpx_actions_diff_gather          action rows as differences of stored positions  vp_suite/datasets/synpick.py:110-113,135-137
 * vpx_frames_augment               the colour and erasing entries of VPDataset's augmentation list  vp_suite/base/base_dataset.py:19-23,135-141
 * vpx_frames_adapt                 ScaleToModel / ScaleToTest + TF.Resize   vp_suite/utils/compatibility.py:31-50, utils/models.py:7-64
 * vpx_vis_compose                  add_borders + side-by-side video, save_frame_compare_img  vp_suite/utils/visualization.py:37-79,133,220-258
 * vpx_nchw_to_nhwc / nhwc_to_nchw  (layout adaptors at the boundary; the reference is NCHW throughout)
 *
 * Layouts. VPX_LAYOUT_NHWC ("channels last", the library's native layout):
 *      x [B,T,H,W,Cin]   h/c states [B,H,W,Ch]   out [B,T,H,W,Ch]   peepholes [H,W,Ch]
 *    VPX_LAYOUT_NCHW (the reference's layout; the library transposes through the workspace):
 *      x [B,T,Cin,H,W]   h/c states [B,Ch,H,W]   out [B,T,Ch,H,W]   peepholes [1,Ch,H,W]
 *    Convolution weights / biases and their gradients are ALWAYS in the reference's parameter layout
 *    (OIHW, e.g. _conv.weight [4Ch, Cin+Ch, kh, kw]) so reference checkpoints are used unchanged.
 */
#ifndef VPX_H_
#define VPX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPX_VERSION 100

enum { VPX_OK = 0, VPX_ERR_ARG = -1, VPX_ERR_WORKSPACE = -2, VPX_ERR_LAUNCH = -3, VPX_ERR_UNSUPPORTED = -4 };

enum { VPX_GATE_IFGO = 0 /* chunk order (i,f,g,o): conv_lstm_hzzone.py:62 */,
       VPX_GATE_IFOG = 1 /* split order (i,f,o,g): conv_lstm_ndrplz.py:34 */ };
enum { VPX_LAYOUT_NHWC = 0, VPX_LAYOUT_NCHW = 1 };
enum { VPX_PREC_F32 = 0    /* exact fp32: v_mfma_f32_32x32x2_f32, fp32 operands + fp32 accumulate */,
       VPX_PREC_BF16X3 = 1 /* split bf16 (hi/lo) operands, 3 bf16 MFMAs per product, fp32 accumulate (~fp32 accuracy) */,
       VPX_PREC_BF16 = 2   /* bf16 operands, fp32 accumulate, fp32 state and I/O */ };
enum { VPX_FLAG_OUT_SPLIT = 8 /* ConvLSTM forward (inference): `out` receives the output sequence in the split-bf16 operand format
                                 ([B][T][H*W][Ch] split-encoded, the byte size of the fp32 tensor it replaces) and NO fp32 copy is written
                                 — for a consumer that reads the operand format (vpx_conv2d_ex_fwd_from_split); hT, if not NULL, is
                                 still fp32. Only where vpx_convlstm_writes_split_output() says so, and not with SAVE_FOR_BWD */,
       VPX_FLAG_X_SPLIT = 4 /* ConvLSTM forward: `x` holds the input sequence in the split-bf16 operand format (below) instead of
                              fp32 — only where vpx_convlstm_takes_split_input() says so; saves the conversion pass */,
       VPX_FLAG_SAVE_FOR_BWD = 1 /* forward fills `reserve` (gate activations + cell states per step) */,
       VPX_FLAG_WEIGHTS_PACKED = 2 /* ConvLSTM forward: `workspace` still holds the weight packs of a previous forward call with the SAME
                                      descriptor (flags aside), weight values and set of present operands (x / h0 NULL or not) — the caller
                                      keeps one workspace per block; saves the repack launches of a small-batch inference step.
                                      ST-LSTM: `workspace` still holds the repacked weights (LayerNorm variant, forward: and the
                                      transposed LayerNorm parameters) of a previous call with the SAME values and desc (caller keeps one workspace per cell per forward; the
                                      backward has its own workspace and additionally needs the same set of requested
                                      data gradients dx / dh / dm as the call that packed) */ };

typedef struct vpx_convlstm_desc {
    int32_t B, T, Cin, Ch, H, W, kh, kw; /* padding is kh/2, kw/2 ("same"), stride 1 — the only form the cells use */
    int32_t gate_order;                   /* VPX_GATE_* */
    int32_t layout;                       /* VPX_LAYOUT_* */
    int32_t precision;                    /* VPX_PREC_* */
    int32_t flags;                        /* VPX_FLAG_* */
} vpx_convlstm_desc;

typedef struct vpx_stlstm_desc {
    int32_t B, Cin, Ch, H, W, k; /* filter_size k (odd), stride 1, padding k/2: predrnn.py:22 */
    int32_t layer_norm;          /* 0/1: LayerNorm([C,H,W]) after conv_x/h/m/o (predrnn.py:24-40) */
    int32_t layout, precision, flags;
} vpx_stlstm_desc;

int vpx_version(void);
const char* vpx_last_error(void);
/* Run-to-run bit reproducibility (the counterpart of torch.use_deterministic_algorithms, which the reference inherits
 * from PyTorch). Default 0: convolutions on small feature maps split their contraction over workgroups and combine
 * partial sums with floating-point atomics (results equal up to fp32 summation order, ~1e-7 relative). 1: no atomics
 * anywhere (slower on 16x16 / 32x32 maps; TrajGRU's warp backward switches to integer atomics, whose sum is order-independent:
 * vpx_trajgru_warp_bwd_det). Process-wide; returns the previous setting. */
int vpx_set_deterministic(int on);
/* Kernel-selection switches for A/B measurements and parity tests inside one process (results never depend on them beyond
 * fp32 summation order). Returns the previous value, or a negative error code for an unknown option.
 *   VPX_OPT_CELL2        0 = the first-generation fused cell kernel everywhere; 1 (default) = the second-generation kernel
 *                        (pre-split operands, LDS-DMA staging) where it applies and fills the chip; 2 = wherever it applies */
#define VPX_OPT_CELL2 1
/*   VPX_OPT_CELL3        small grids (small batch and / or 16x16 - 32x32 maps): 1 (default) = the sliced fused step (8-channel
 *                        slices, weights resident in LDS, no atomics) where it applies; 0 = K-split convolution + gate kernel */
#define VPX_OPT_CELL3 2
/*   VPX_OPT_MFMA_SHAPE   bf16 MFMA shape of the second-generation kernels' main loop (fused cell step, its data gradient): 0 =
 *                        v_mfma_f32_32x32x16_bf16, 1 = v_mfma_f32_16x16x32_bf16 (K = 32 steps pair two taps of a 16-channel
 *                        stage; same wave tile, same LDS traffic, the chip holds a higher clock on it). Same products, same
 *                        operand split: results differ in fp32 summation order only */
#define VPX_OPT_MFMA_SHAPE 3
/*   VPX_OPT_EXPERIMENT   bits of kernel variants under measurement (A/B inside one process; 0 = the product's behaviour): an OR of
 *                        the VPX_EXP_* values below. Any value is stored; bits without a name select nothing. */
#define VPX_OPT_EXPERIMENT 4
/* Selection bits, read by the host code that chooses a launch. Each names the form it switches ON in place of the product's. */
#define VPX_EXP_CELL2_FULL_TILE 4         /* the 32x16 tile instead of the half tile (fused cell, data gradient) */
#define VPX_EXP_CONVQ_FULL_TILE 16        /* the 32x16 tile for the stage-glue kernel (convq) */
#define VPX_EXP_HOIST_GEN1 32             /* the hoisted input projection of the small-grid paths on the first-generation kernel */
#define VPX_EXP_ST_WGRAD_GEN1 64          /* the ST-LSTM step's k x k weight gradients on the first-generation launches instead of the
                                           * one-launch split-operand kernel (stw, wgrad2.hip) */
#define VPX_EXP_ST_DGRAD_GEN1 128         /* its k x k data gradients on the first-generation kernel instead of the 16x16-tile job-table
                                           * kernel (c5, convq.hip) */
#define VPX_EXP_ST_FWD_GEN1 256           /* the same for its forward launches (gate groups, conv_o + output gate) */
#define VPX_EXP_C1_GEN1 512               /* the 1x1 layers (conv_last, its adjoint, the decoupling tail's adapter) on the implicit-GEMM
                                           * kernel instead of the streaming one (c1, conv1.hip) */
#define VPX_EXP_C5_UNSPLIT 1024           /* the c5 launches unsplit on grids below their pixel-tile bar (48 tiles forward, 96 backward; tests) */
#define VPX_EXP_C5_NO_KSPLIT 2048         /* the first-generation launches instead of the K-split c5 jobs on those grids */
#define VPX_EXP_NO_C3 4096                /* the half tile of the fused ConvLSTM step instead of its narrow-tile form (c3: c5_kernel<4, 3>)
                                           * on grids of at most 256 half-tile workgroups */
#define VPX_EXP_C3_NARROW 8192            /* c3 with 32-column tiles (c5_kernel<2, 3>) instead of 64-column ones */
#define VPX_EXP_GLUE_DGRAD_GEN1 16384     /* the stage glue's data gradients on the first-generation kernel where the schedule-driven one
                                           * (convq) would take them */
#define VPX_EXP_CELL2X 32768              /* the fused ConvLSTM step on the eight-wave half tile (cell2_kernel_x: 64-register wave tiles,
                                           * four waves per SIMD) instead of the four-wave one */
#define VPX_EXP_CELL2X_COLSPLIT 65536     /* cell2_kernel_x's column split instead of its row split */
#define VPX_EXP_ST_LAST_FP32 (1 << 27)    /* the ST-LSTM step's conv_last (1x1) on the fp32 c_new / m_new (converted in the kernel) instead
                                           * of on the split copies its gate stage leaves */
#define VPX_EXP_NO_C16 (1 << 28)          /* 3x3 layers with 16 output channels on the first-generation kernel instead of the
                                           * resident-weights one (csrc/conv16.hip) */
#define VPX_EXP_GLUE_WGRAD_TAPGROUP (1 << 29) /* the stage glue's weight gradients on the tap-group kernel (fp32 operands) instead of
                                           * wgrad2_kernel's glue form on split copies */
/* Diagnostics of the 16x16x32-form cell kernel (cell2_kernel_q), read inside the kernel: the launch hands it the option word masked
 * with VPX_EXP_CELL2_DIAG_MASK and nothing else. */
#define VPX_EXP_CELL2_NO_STAGGER 1        /* no sync-point stagger between the wave halves of the 32x16-tile cell */
#define VPX_EXP_CELL2_PLACEMENT 8         /* the N tiles of a pixel tile D dispatch positions apart inside an XCD, D = bits 8-19 of the
                                           * option word (value | D << 8). That field lies on top of the selection bits 256 .. 65536:
                                           * never combine VPX_EXP_CELL2_PLACEMENT with one of them */
#define VPX_EXP_CELL2_DIAG_MASK (VPX_EXP_CELL2_NO_STAGGER | VPX_EXP_CELL2_PLACEMENT | (0xfff << 8))
/*   VPX_OPT_DRY_RUN      1 = every entry point does all of its host-side work (argument checks, kernel selection, workspace carving
 *                        and the bounds checks of everything it would write into the workspace) but issues no HIP call: needs no GPU
 *                        and touches none of the pointers (they only have to be non-NULL where the call requires a tensor). A sizing
 *                        rule of a `*_workspace_bytes` query that disagrees with the launch code returns VPX_ERR_WORKSPACE. For the
 *                        CPU test-suite (tests/test_workspace_contract.py). Leaves no state behind: switch it off again and launch. */
#define VPX_OPT_DRY_RUN 5
/*   VPX_OPT_SEQ_CHAINS   launch chains of vpx_convlstm_seq_fwd's time loop on the second-generation routes (CELL2, C3): 1 (default) = from
 *                        B = 8 on, the two halves of the batch ([0, (B + 1) / 2) and the rest) as two chains of step launches, one on
 *                        the caller's stream and one on a stream the library keeps per device, forked after the call's packs and joined
 *                        before its final copies, so that one half's next step fills the tail of the other's; 2 = the same from B = 2
 *                        on (tests, A/B runs); 0 = one chain on the caller's stream. All launch the kernel chosen for the whole call:
 *                        results are bit-identical, workspace and reserve sizes the same. A call with B = 1, on another route or on a
 *                        capturing stream runs one chain whatever the value (vpx_convlstm_seq_chains tells). */
#define VPX_OPT_SEQ_CHAINS 6
int vpx_set_option(int option, int value);
/* A counter that advances with every vpx_set_option / vpx_set_deterministic call: callers that cache anything kernel-selection
 * dependent (a workspace with weight packs, VPX_FLAG_WEIGHTS_PACKED) key it on this value. */
int vpx_option_epoch(void);

/* ---- ConvLSTM over a sequence ------------------------------------------------------------------------------ */
size_t vpx_convlstm_workspace_bytes(const vpx_convlstm_desc* d); /* scratch, contents undefined between calls */
/* Split-bf16 operand format ("split"): a [N,H,W,C] fp32 NHWC tensor re-encoded, same byte count, as per pixel, per group of 8
 * channels: 8 hi bf16 (round-to-nearest of the value) then 8 lo bf16 (round-to-nearest of value - hi) — what the bf16x3
 * kernels multiply. Producers: vpx_conv2d_ex_fwd_split (the stage glue feeding a recurrent block). 1 = this descriptor's
 * forward consumes x in that form when VPX_FLAG_X_SPLIT is set (inference: the second-generation cell kernel, and the small-grid
 * kernel where its hoisted input projection runs on the schedule-driven convolution), 0 = fp32 only. */
int vpx_convlstm_takes_split_input(const vpx_convlstm_desc* d);
int vpx_convlstm_writes_split_output(const vpx_convlstm_desc* d);   /* 1 = VPX_FLAG_OUT_SPLIT is available for this descriptor */
size_t vpx_convlstm_reserve_bytes(const vpx_convlstm_desc* d);   /* saved-for-backward, 0 without SAVE_FOR_BWD */

/* x may be NULL (all-zero input: conv_lstm_hzzone.py:54-56), h0/c0 may be NULL (zero state: :40-45), bias may be NULL,
 * Wci/Wcf/Wco may be NULL together (no peephole = the ndrplz cell). hT/cT may be NULL. */
int vpx_convlstm_seq_fwd(const vpx_convlstm_desc* d, const float* x, const float* h0, const float* c0,
                         const float* W, const float* bias, const float* Wci, const float* Wcf, const float* Wco,
                         float* out, float* hT, float* cT, void* reserve, size_t reserve_bytes, void* workspace,
                         size_t workspace_bytes, void* stream);

/* BPTT. `out`/`reserve` are the forward's. dout/dhT/dcT may be NULL (zero). Every gradient output may be NULL
 * (skipped). dW/db/dWc* are OVERWRITTEN (not accumulated). */
int vpx_convlstm_seq_bwd(const vpx_convlstm_desc* d, const float* x, const float* h0, const float* c0,
                         const float* W, const float* Wci, const float* Wcf, const float* Wco, const float* out,
                         const void* reserve, size_t reserve_bytes, const float* dout, const float* dhT,
                         const float* dcT, float* dx, float* dh0, float* dc0, float* dW, float* db, float* dWci,
                         float* dWcf, float* dWco, void* workspace, size_t workspace_bytes, void* stream);

/* The plan of a sequence call: which kernels vpx_convlstm_seq_fwd / _bwd with this descriptor take under the current
 * vpx_set_deterministic / vpx_set_option state, filled by the functions that decide it for the calls themselves. No launch, no
 * allocation. x_present: 0 = the call's `x` is NULL; want_dx / want_dW: the backward is asked for dx / dW (non-NULL pointers).
 *   forward   route (VPX_CL_ROUTE_*); qform: the 16x16x32 MFMA form on CELL2 / C3; c3nt: C3's column tiles per N tile (4 | 2, else 0);
 *             mw: FUSED's workgroup form (1: four waves, 2: eight waves; 0 off FUSED); ksplit: K ranges of the step's convolution on
 *             KSPLIT (else 0); hh_split: K ranges of HOIST's recurrent convolution, the only split of that route (else 0); hoist_convq: the hoisted projection of HOIST / CELL3 on the
 *             schedule-driven kernel; cell2x: CELL2's q form on the eight-wave half tile
 *   backward  (all zero without VPX_FLAG_SAVE_FOR_BWD) dgrad: the data gradient on 0 the first-generation kernel, 1 conv2;
 *             dgrad_qform: conv2's MFMA form; d_mw: the first-generation data gradient's workgroup form (0 on conv2); dgrad_cols: the
 *             columns of [x | h] it writes (Cin + Ch, or Ch without dx); wgrad (0 without want_dW): 0 launch_wgrad, 1 wgrad2 on the
 *             operands of the reserve, 2 wgrad2 on operands the backward converts itself; n_slices: K slices of the weight-gradient
 *             kernel that takes the launch; dG_f32: the gate backward writes dG in fp32; gate_slices: its batch slices (peephole
 *             gradients are reduced over them when > 1)
 * Returns what vpx_convlstm_workspace_bytes' checks refuse with (VPX_ERR_ARG, VPX_ERR_UNSUPPORTED), VPX_ERR_ARG for a NULL `out`. */
enum { VPX_CL_ROUTE_FUSED = 0, VPX_CL_ROUTE_KSPLIT = 1, VPX_CL_ROUTE_HOIST = 2, VPX_CL_ROUTE_CELL3 = 3, VPX_CL_ROUTE_CELL2 = 4,
       VPX_CL_ROUTE_C3 = 5 };
typedef struct vpx_convlstm_plan_info {
    int32_t route, qform, c3nt, mw, ksplit, hh_split, hoist_convq, cell2x;
    int32_t dgrad, dgrad_qform, d_mw, dgrad_cols, wgrad, n_slices, dG_f32, gate_slices;
} vpx_convlstm_plan_info;
int vpx_convlstm_plan(const vpx_convlstm_desc* d, int x_present, int want_dx, int want_dW, vpx_convlstm_plan_info* out);
/* Launch chains (VPX_OPT_SEQ_CHAINS) a vpx_convlstm_seq_fwd call with this descriptor on `stream` would run right now: 2 or 1; 0 for a
 * descriptor the call refuses. Asks the stream whether it is capturing (a dry run does not: it answers as for a stream that is not). */
int vpx_convlstm_seq_chains(const vpx_convlstm_desc* d, int x_present, void* stream);

/* ---- ST-LSTM cell step (PredRNN-V2) -------------------------------------------------------------------------- */
size_t vpx_stlstm_workspace_bytes(const vpx_stlstm_desc* d);
size_t vpx_stlstm_reserve_bytes(const vpx_stlstm_desc* d);
/* Split-format shadows. The bf16x3 5x5 kernels read every activation in the split operand format (above); a tensor that a
 * previous step produced — h_new is the next step's h and the next layer's x, m_new the next layer's m — need not be converted
 * again when the caller hands its split copy back. The shadows are an ARGUMENT of the step call they belong to
 * (vpx_stlstm_step_fwd_ex / _bwd_ex; round 4 passed them through a thread-local setter that a failed or skipped call could leave
 * armed for an unrelated one — removed):
 *   vpx_stlstm_uses_split(d)   1 when calls with this descriptor consume / produce shadows, else 0 (they are ignored)
 *   in[5]  = {x, h, m, c_new, m_new}: NULL or the tensor once more in the split format, B*H*W*C*4 bytes (forward reads the first
 *            three, backward all five; a NULL entry is converted by the library as before)
 *   out[3] = {h_new, c_new, m_new}: NULL or caller buffers of B*H*W*Ch*4 bytes the forward fills with these outputs in the split
 *            format (ignored by the backward)
 *   dg8_out (backward only; NULL = off): DEFERRED WEIGHT GRADIENTS. The step writes its d(pre-activations) dG8 [B][H*W][8Ch]
 *            (gate blocks i,f,g | o | i',f',g' + d conv_last; split format, B*H*W*8Ch*4 bytes) there, computes the data gradients as
 *            usual and leaves dWx .. dWlast alone (they may be NULL). The caller keeps the dG8 of the T steps of one cell and the five
 *            sources x, h, m, c_new, m_new (split format) in dense slabs [T][B][H*W][C] and calls vpx_stlstm_wgrad_batch ONCE with a
 *            descriptor whose B is T*B: the same kernel over all the steps' images — one launch, one slab reduction and no per-step
 *            accumulation of the results. Available where vpx_stlstm_defers_wgrad(d) says 1 (5x5, bf16x3, channels in 8s, no LayerNorm).
 *   NHWC layout only: on reference-layout (NCHW) descriptors in[] / out[] are ignored and a non-NULL dg8_out is refused with
 *   VPX_ERR_UNSUPPORTED (never silently dropped). Without dg8_out a NULL dW pointer means "this weight is frozen": that gradient is
 *   not computed.
 *   `shadows` may be NULL: vpx_stlstm_step_fwd / _bwd are exactly that. */
typedef struct vpx_stlstm_shadows { const void* in[5]; void* out[3]; void* dg8_out; } vpx_stlstm_shadows;
int vpx_stlstm_uses_split(const vpx_stlstm_desc* d);
int vpx_stlstm_defers_wgrad(const vpx_stlstm_desc* d);
size_t vpx_stlstm_wgrad_batch_workspace_bytes(const vpx_stlstm_desc* d);   /* d->B = all images of the batch (T*B) */
/* dg8_split [N][H*W][8Ch], src5_split = {x [N][H*W][Cin], h, m, c_new, m_new [N][H*W][Ch]} with N = d->B, all in the split format;
 * weight gradients in reference layout (as vpx_stlstm_step_bwd), OVERWRITTEN. */
int vpx_stlstm_wgrad_batch(const vpx_stlstm_desc* d, const void* dg8_split, const void* const* src5_split, float* dWx, float* dWh,
                           float* dWm, float* dWo, float* dWlast, void* workspace, size_t workspace_bytes, void* stream);

/* The plan of a step: which kernels a vpx_stlstm_step_fwd_ex / _bwd_ex call with this descriptor takes under the current
 * vpx_set_deterministic / vpx_set_option state, filled by the functions that decide it for the calls themselves. No launch, no
 * allocation. all_weight_grads: 1 = the backward is asked for all five weight gradients, 0 = at least one weight is frozen (a NULL dW).
 *   forward   route (VPX_ST_ROUTE_*); o_split: K ranges of GEN1's conv_o as a plain convolution + pointwise gate (0: fused with the gate);
 *             nt_o: conv_o's N-tile width in 16-column units on C5 / C5K (else 0); ks_g / ks_o: K chunks of the gate groups / of conv_o on
 *             C5K (else 0); mw_g / mw_o: workgroup form of GEN1's gate / conv_o launch (2: 8 waves); ksplit_l: K ranges of conv_last on the
 *             implicit-GEMM kernel; last_c1: conv_last on the streaming 1x1 kernel instead (operands 16-byte aligned)
 *   backward  (zero with layer_norm) stw: the five weight gradients in one launch; c5: the k x k data gradients on the 16x16-tile kernel,
 *             c5_ks[]: their K chunks (conv_o -> c_new, conv_o -> m_new, dx, dh, dm; 0 without c5); n_slices / stw_ns: K slices of the
 *             first-generation / the one-launch weight gradients; dg_ksplit[] / dg_mw[]: K ranges and workgroup form of the
 *             first-generation data gradients (conv_o's adjoint, conv_last's adjoint, dx, dh, dm)
 * Returns what vpx_stlstm_workspace_bytes' checks refuse with (VPX_ERR_ARG, VPX_ERR_UNSUPPORTED), VPX_ERR_ARG for a NULL `out`. */
enum { VPX_ST_ROUTE_LN = 0, VPX_ST_ROUTE_GEN1 = 1, VPX_ST_ROUTE_C5 = 2, VPX_ST_ROUTE_C5K = 3 };
typedef struct vpx_stlstm_plan_info {
    int32_t route, o_split, nt_o, ks_g, ks_o, mw_g, mw_o, ksplit_l, last_c1;
    int32_t stw, c5, c5_ks[5], n_slices, stw_ns, dg_ksplit[5], dg_mw[5];
} vpx_stlstm_plan_info;
int vpx_stlstm_plan(const vpx_stlstm_desc* d, int all_weight_grads, vpx_stlstm_plan_info* out);

/* Weights in reference layout: Wx [7Ch,Cin,k,k] Wh [4Ch,Ch,k,k] Wm [3Ch,Ch,k,k] Wo [Ch,2Ch,k,k] Wlast [Ch,2Ch,1,1].
 * ln: NULL or 8 pointers {x_gamma,x_beta,h_gamma,h_beta,m_gamma,m_beta,o_gamma,o_beta}, each in reference [C,H,W]. */
int vpx_stlstm_step_fwd(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m,
                        const float* Wx, const float* Wh, const float* Wm, const float* Wo, const float* Wlast,
                        const float* const* ln, float* h_new, float* c_new, float* m_new, float* delta_c,
                        float* delta_m, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                        void* stream);

/* c_new / m_new are the forward's outputs (the operands of conv_o / conv_last). Incoming gradients may be NULL (zero);
 * every gradient output may be NULL (skipped); weight gradients are OVERWRITTEN. ln / dln: the 8 LayerNorm parameter
 * tensors and their gradients (reference layout [C,H,W]); NULL unless desc.layer_norm. */
int vpx_stlstm_step_bwd(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m,
                        const float* c_new, const float* m_new,
                        const float* Wx, const float* Wh, const float* Wm, const float* Wo, const float* Wlast,
                        const float* const* ln, const void* reserve, size_t reserve_bytes, const float* dh_new,
                        const float* dc_new, const float* dm_new, const float* ddelta_c, const float* ddelta_m,
                        float* dx, float* dh, float* dc, float* dm, float* dWx, float* dWh, float* dWm, float* dWo,
                        float* dWlast, float* const* dln, void* workspace, size_t workspace_bytes, void* stream);
/* the same calls with split-format shadows (see above) */
int vpx_stlstm_step_fwd_ex(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m,
                           const float* Wx, const float* Wh, const float* Wm, const float* Wo, const float* Wlast,
                           const float* const* ln, float* h_new, float* c_new, float* m_new, float* delta_c,
                           float* delta_m, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                           void* stream, const vpx_stlstm_shadows* shadows);
int vpx_stlstm_step_bwd_ex(const vpx_stlstm_desc* d, const float* x, const float* h, const float* c, const float* m,
                           const float* c_new, const float* m_new,
                           const float* Wx, const float* Wh, const float* Wm, const float* Wo, const float* Wlast,
                           const float* const* ln, const void* reserve, size_t reserve_bytes, const float* dh_new,
                           const float* dc_new, const float* dm_new, const float* ddelta_c, const float* ddelta_m,
                           float* dx, float* dh, float* dc, float* dm, float* dWx, float* dWh, float* dWm, float* dWo,
                           float* dWlast, float* const* dln, void* workspace, size_t workspace_bytes, void* stream,
                           const vpx_stlstm_shadows* shadows);

/* ---- decoupling-loss term: mean_{b,ch} |cos(normalize(A*dc), normalize(A*dm))| over H*W ---------------------- */
/* delta_c/delta_m [B,H,W,Ch] (NHWC) ; adapter [Ch,Ch] ; value / dvalue: 1 float on device.
 * precision (vpx_precision): arithmetic of the tail's three 1x1 contractions (adapter, its adjoint, its weight gradient) —
 * the caller passes the model's own operand mode, so a VPX_PREC_F32 model gets exact fp32 here too (round 3 ran this tail in
 * bf16x3 for every caller). The normalisation / cosine / mean are fp32 with double partial sums in every mode. */
size_t vpx_decouple_workspace_bytes(int B, int Ch, int H, int W);
int vpx_decouple_fwd(const float* delta_c, const float* delta_m, const float* adapter, float* value, int B, int Ch,
                     int H, int W, int precision, void* workspace, size_t workspace_bytes, void* stream);
int vpx_decouple_bwd(const float* delta_c, const float* delta_m, const float* adapter, const float* dvalue,
                     float* d_delta_c, float* d_delta_m, float* d_adapter, int B, int Ch, int H, int W, int precision,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- training tail (the caller side of the path: base_model.py:168-176, vpsuite.py:353) ------------------------- */
/* loss = scale * mean_{b,t} sum_{c,h,w} (pred - target)^2   (base_measure.py:55-57, image_wise.py:25, loss_provider.py:48-51)
 * pred/target: n_elements = B*T*C*H*W floats in any (identical) layout, n_frames = B*T; loss: 1 float on device;
 * dpred (nullable): d loss / d pred, written in the same pass. Deterministic (fixed reduction order, double partials). */
size_t vpx_mse_loss_workspace_bytes(void);
int vpx_mse_loss(const float* pred, const float* target, long long n_elements, long long n_frames, float scale,
                 float* loss, float* dpred, void* workspace, size_t workspace_bytes, void* stream);
/* One torch.optim.Adam step (amsgrad off) over flat, 16-byte aligned buckets of n floats; step >= 1 is the iteration
 * count after this update; grad is multiplied by grad_scale first (1/world_size after a summing all-reduce).
 * Hyper-parameters are doubles: the derived scalars (1 - beta, lr / (1 - beta1^t), ...) are formed in double as PyTorch
 * forms them in Python floats, and rounded to fp32 once. */
int vpx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream);
/* Gradient clipping and a non-finite step guard, fused into the update (no host round trip, no further pass over the gradient).
 * vpx_grad_stats: one streaming pass over grad[n] (16-byte loads where grad is 16-byte aligned, scalar otherwise) into a
 * device-resident double stats[4] (8-byte aligned):
 *   stats[0] = || grad_scale * grad ||_2: the squares are summed exactly in double (a float x float product is exact there),
 *              grad_scale is applied in double to the sum, then one sqrt. Not finite (inf or NaN) when an element is not.
 *   stats[1] = max | grad_scale * grad | over the FINITE elements (0 if there are none)
 *   stats[2] = number of non-finite elements (NaN, +-inf)
 *   stats[3]   not touched here: the number of steps vpx_adam_step_clipped skipped (the caller zeroes it once).
 * Double per-thread accumulators, per-block partials in the workspace, a one-wave final kernel with a fixed summation order and no
 * floating-point atomics: bit-reproducible run to run whatever vpx_set_deterministic says.
 * VPX_ERR_ARG: grad or stats NULL, n < 1, stats not 8-byte aligned, grad_scale negative or NaN. VPX_ERR_WORKSPACE: workspace NULL or
 * smaller than vpx_grad_stats_workspace_bytes().
 *
 * vpx_adam_step_clipped: vpx_adam_step with, in this order,
 *   1. the per-launch factor s = (float)(grad_scale * c), c = max_norm > 0 ? min(1, max_norm / (stats[0] + 1e-6)) : 1 formed in
 *      double from the device value (torch.nn.utils.clip_grad_norm_'s coefficient; a NaN norm gives NaN, as there):
 *      g = grad[k] * s is the one float multiply vpx_adam_step spends on grad_scale;
 *   2. clip_value > 0: g = min(max(g, -clip_value), clip_value), NaN stays NaN (torch.clamp; clip_grad_value_);
 *   then weight decay and the update as in vpx_adam_step, from the same host-prepared scalars.
 *   3. skip_nonfinite != 0 and stats[2] > 0: nothing is written to param / exp_avg / exp_avg_sq (bit-unchanged) and stats[3] is
 *      incremented by one. A SKIPPED STEP STILL ADVANCES THE STEP COUNT: the bias corrections are host scalars of `step`, and
 *      holding the count back would take a host sync or a device-side pow; the caller passes step + 1 to the next call either way.
 * With c = 1 (max_norm = 0, or the norm below it), clip_value = 0 and nothing skipped, s == (float)grad_scale and param / exp_avg /
 * exp_avg_sq come out bit-identical to vpx_adam_step's. stats is read on the device when the kernel runs (enqueue vpx_grad_stats
 * on the same stream before it); stats == NULL is allowed with max_norm == 0 and skip_nonfinite == 0 (value clipping alone needs
 * no reduction).
 * VPX_ERR_ARG: what vpx_adam_step refuses (a NULL bucket, n < 1, step < 1, buckets not 16-byte aligned), stats not 8-byte aligned,
 * grad_scale / max_norm / clip_value negative or NaN, stats == NULL with max_norm > 0 or skip_nonfinite. */
size_t vpx_grad_stats_workspace_bytes(void);
int vpx_grad_stats(const float* grad, long long n, double grad_scale, double* stats, void* workspace, size_t workspace_bytes,
                   void* stream);
int vpx_adam_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                          double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale,
                          const double* stats, double max_norm, double clip_value, int skip_nonfinite, void* stream);

/* ---- image-wise measures (vp_suite/measure/image_wise.py): per-frame tables that serve every reduction ------------
 * All of them: double partial sums, fixed-order final reduction, no atomics (bit-reproducible in either determinism mode).
 * pred / target: n_frames = B*T dense frames of frame_elems = C*H*W floats, in any per-frame element order both share.
 * sums [3, n_frames] (doubles): per-frame sums of d^2, |d| and smooth-L1(d) (beta = 1), d = pred - target — the criteria of MSE, L1,
 * SmoothL1 and PSNR (nn.*Loss(reduction="none"); base_measure.py:57 and image_wise.py:69-71 reduce them further).
 * Backward: dsums [3, n_frames] (floats) = the cotangents of that table, read on the device (no host sync):
 *   dpred = 2 dsums[0][f] d + dsums[1][f] sign(d) + dsums[2][f] clamp(d, -1, 1), sign(0) = 0; written out of place.
 * A PSNR term reaches it through row 0: d/dSE_f of mean_f 10 log10(SE_f / frame_elems) is 10 / (ln10 n_frames SE_f). */
size_t vpx_pixel_measures_workspace_bytes(long long n_frames, long long frame_elems);
int vpx_pixel_measures_fwd(const float* pred, const float* target, long long n_frames, long long frame_elems, double* sums,
                           void* workspace, size_t workspace_bytes, void* stream);
int vpx_pixel_measures_bwd(const float* pred, const float* target, const float* dsums, long long n_frames,
                           long long frame_elems, float* dpred, void* stream);
/* ssim [n_frames]: SSIM of each frame with piqa's SSIM() defaults (image_wise.py:111-117 after base_measure.py:71-74): inputs
 * mapped by clamp((x+1)/2, 0, 1) inside the kernel, 11-tap Gaussian (sigma 1.5, sum 1) per channel without padding, C1 = 0.01^2,
 * C2 = 0.03^2, mean over the 3 (H-10) (W-10) map entries. Frames are [3,H,W] (VPX_LAYOUT_NCHW) or [H,W,3] (VPX_LAYOUT_NHWC);
 * C must be 3 and H, W >= 11 (VPX_ERR_ARG otherwise). Backward: dpred = dssim[f] * d ssim[f] / d pred, recomputed from the
 * inputs (the forward saves nothing), including the clamp's derivative: 0.5 where -1 <= pred <= 1, else 0. No workspace. */
size_t vpx_ssim_workspace_bytes(long long n_frames, int H, int W);
int vpx_ssim_fwd(const float* pred, const float* target, long long n_frames, int C, int H, int W, int layout, float* ssim,
                 void* workspace, size_t workspace_bytes, void* stream);
int vpx_ssim_bwd(const float* pred, const float* target, const float* dssim, long long n_frames, int C, int H, int W,
                 int layout, float* dpred, void* stream);
/* LPIPS on an AlexNet trunk (https://arxiv.org/abs/1801.03924; image_wise.py's LPIPS through piqa), fp32, no atomics
 * (bit-reproducible in either determinism mode); the training entry points and the backward follow below. The library ships no weights: the caller hands them in. Feature maps are
 * channels-last, [N, h, w, C], the layout of the library's convolutions.
 * vpx_lpips_fwd: pred / target: n_frames dense [3,H,W] frames in the model's range. Each is mapped by clamp((v+1)/2, 0, 1), then
 *   (u - mean_c) / std_c with ImageNet's mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225); both go through the trunk as ONE
 *   batch of 2 n_frames images: conv 3->64 k11 s4 p2 + ReLU (tap 1), max-pool 3/2, conv 64->192 k5 p2 + ReLU (tap 2), max-pool 3/2,
 *   conv 192->384 k3 p1 + ReLU (tap 3), conv 384->256 k3 p1 + ReLU (tap 4), conv 256->256 k3 p1 + ReLU (tap 5); the pools in floor mode
 *   without padding. table [n_frames] (doubles, OVERWRITTEN) = sum over the taps of the mean over a tap's pixels of
 *   sum_c lin[c] (fx[c] / (|fx| + 1e-10) - fy[c] / (|fy| + 1e-10))^2, |f| the channel norm at the pixel.
 *   params: 15 device pointers, conv1..conv5 weights [Co,Ci,k,k], conv1..conv5 biases [Co], lin1..lin5 [C] (the array itself on the host).
 *   VPX_ERR_ARG: a NULL pointer, n_frames < 1, C != 3, H or W < 31 (below that the third tap has no pixel). VPX_ERR_UNSUPPORTED: more
 *   work than one launch holds. VPX_ERR_WORKSPACE: workspace NULL or smaller than vpx_lpips_workspace_bytes(n_frames, H, W) (0 for
 *   sizes the call refuses), which holds the feature maps of the 2 n_frames images (two slots, used in turn), the weight packs of
 *   the four stride-1 convolutions, the transposed stem weights and the heads' partial sums.
 * The pieces, as the trunk runs them:
 * vpx_lpips_stem_fwd: y [n0 + n1, Ho, Wo, 64] = ReLU(conv(norm(x), w [64,3,11,11], stride 4, pad 2) + bias), Ho = (H + 4 - 11) / 4 + 1, over
 *   the n0 images [3,H,W] at x0 followed by the n1 at x1 (n1 = 0: x1 may be NULL); `norm` as above, fused into the operand load; the
 *   padding ring is zero in NORMALISED space, not the normalised value of 0. H, W >= 7. Workspace: vpx_lpips_stem_workspace_bytes().
 * vpx_lpips_maxpool_fwd: y [N, (H-3)/2+1, (W-3)/2+1, C] = 3x3 stride-2 max-pool of x [N,H,W,C], floor mode, no padding; H, W >= 3.
 * vpx_lpips_head_fwd: table[i] += mean over the HW pixels of the expression above for fx, fy [n, HW, C] and w [C]; C <= 512
 *   (VPX_ERR_UNSUPPORTED beyond). Every feature element is read once, the arithmetic on them is double; an all-zero feature vector
 *   contributes through the 1e-10, never as NaN. Workspace: vpx_lpips_head_workspace_bytes(n, HW). */
size_t vpx_lpips_workspace_bytes(long long n_frames, int H, int W);
int vpx_lpips_fwd(const float* pred, const float* target, long long n_frames, int C, int H, int W, const float* const* params,
                  double* table, void* workspace, size_t workspace_bytes, void* stream);
size_t vpx_lpips_stem_workspace_bytes(void);
int vpx_lpips_stem_fwd(const float* x0, const float* x1, long long n0, long long n1, int H, int W, const float* w, const float* bias,
                       float* y, void* workspace, size_t workspace_bytes, void* stream);
int vpx_lpips_maxpool_fwd(const float* x, float* y, long long N, int H, int W, int C, void* stream);
size_t vpx_lpips_head_workspace_bytes(long long n, long long HW);
int vpx_lpips_head_fwd(const float* fx, const float* fy, const float* w, long long n, long long HW, int C, double* table,
                       void* workspace, size_t workspace_bytes, void* stream);
/* LPIPS as a training loss: the gradient with respect to the PREDICTION (target and weights get none: the trunk is frozen). fp32 storage,
 * no atomics, bit-reproducible in either determinism mode.
 * vpx_lpips_fwd_train: vpx_lpips_fwd's launches in its order, so `table` is bit-equal to vpx_lpips_fwd's; the five taps of the 2 n_frames
 *   images (prediction first) are written into `reserve` instead of the two slots used in turn. Workspace: vpx_lpips_workspace_bytes.
 *   vpx_lpips_reserve_bytes(n_frames, H, W) = sum over the taps k of align256(2 n_frames h_k w_k C_k 4) + 256 bytes, (h_k, w_k) the map of
 *   tap k ((H-7)/4+1 at tap 1, (h-3)/2+1 per pool), C_k = 64, 192, 384, 256, 256; 0 for sizes the call refuses. The pooled maps are not
 *   kept. VPX_ERR_WORKSPACE also for a reserve that is NULL or smaller than that.
 * vpx_lpips_bwd: dpred [n_frames,3,H,W] (dense, every element OVERWRITTEN) = sum_i dtable[i] d table[i] / d pred, from the reserve that
 *   vpx_lpips_fwd_train filled for the same pred, params and sizes. dtable: n_frames doubles ON THE DEVICE (no host sync). Runs over the
 *   n_frames prediction images only, the target half of each tap serves as fy: head of tap 5; conv5 data gradient, head of tap 4 with it
 *   as `incoming`; conv4, head 3; conv3, pool, head 2; conv2, pool, head 1; stem. The four stride-1 data gradients are
 *   vpx_conv2d_ex_bwd calls (exact fp32 operands, dw and db not requested) on a slot of vpx_conv2d_ex_bwd_workspace_bytes, which counts
 *   weight-gradient slabs this call never touches. Workspace: vpx_lpips_bwd_workspace_bytes(n_frames, H, W). Errors as vpx_lpips_fwd.
 * The pieces:
 * vpx_lpips_head_bwd: dz [n, HW, C] (float32) = the gradient with respect to the tap's PRE-activation. With s = |fx|, r = 1 / (s + 1e-10),
 *   u_c = 2 w_c (fx_c r - fy_c / (|fy| + 1e-10)):  dz_c = [fx_c > 0] (incoming_c + (dtable[i] / HW) (r u_c - fx_c r^2 (sum_k u_k fx_k) / s)),
 *   in double. incoming [n, HW, C]: the gradient arriving from the next layer, or NULL; dz may be `incoming` itself. An all-zero feature
 *   vector gives exactly 0, never NaN. C <= 512 (VPX_ERR_UNSUPPORTED beyond). No workspace.
 * vpx_lpips_maxpool_bwd: dx [N,H,W,C] (every element written) from dy [N,(H-3)/2+1,(W-3)/2+1,C] and the pool's input x. Tie rule: a
 *   window hands its gradient to the FIRST of its maximal elements in row-major order (rows, then columns), the element torch's CPU
 *   max_pool2d picks; a NaN takes the window, the last one if there are several. Rows and columns that floor mode drops get exactly 0.
 * vpx_lpips_stem_bwd: dx [n,3,H,W] (dense, every element written) from dz [n,Ho,Wo,64] (the gradient of tap 1's pre-activation), the
 *   images x and w [64,3,11,11]: the data gradient of the stride-4 convolution times 0.5 / std_c times the clamp's mask. Clamp rule: the
 *   mask is evaluated on the forward's own fp32 u = (x + 1) / 2 and passes the gradient where 0 <= u <= 1, bounds INCLUDED (torch's
 *   clamp). Pixels no window covers (trailing rows / columns when (H + 4 - 11) % 4 != 0) get exactly 0. Workspace:
 *   vpx_lpips_stem_workspace_bytes(). */
size_t vpx_lpips_reserve_bytes(long long n_frames, int H, int W);
int vpx_lpips_fwd_train(const float* pred, const float* target, long long n_frames, int C, int H, int W, const float* const* params,
                        double* table, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t vpx_lpips_bwd_workspace_bytes(long long n_frames, int H, int W);
int vpx_lpips_bwd(const float* pred, const float* const* params, const void* reserve, const double* dtable, long long n_frames, int C,
                  int H, int W, float* dpred, void* workspace, size_t workspace_bytes, void* stream);
int vpx_lpips_head_bwd(const float* fx, const float* fy, const float* w, const double* dtable, const float* incoming, long long n,
                       long long HW, int C, float* dz, void* stream);
int vpx_lpips_maxpool_bwd(const float* x, const float* dy, float* dx, long long N, int H, int W, int C, void* stream);
int vpx_lpips_stem_bwd(const float* x, const float* w, const float* dz, long long n, int H, int W, float* dx, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- Frechet Video Distance on an Inception-I3D trunk (csrc/fvd.hip; vp_suite/measure/fvd), forward only. Activations are channels-last
 * [N, T, H, W, C] float32. "SAME" padding, per axis (the reference's Unit3D / MaxPool3dSamePadding rule): pad = max(k - s, 0) if
 * size % s == 0, else max(k - size % s, 0); front = pad / 2, the rest behind; output size ceil(size / s). vpx_same_padding answers it
 * (host only): *front and *out for one axis.
 *
 * vpx_conv3d_same: y[.., coff + o] = act(sum x * w + bias[o]) over the ZERO-padded map. x [N,T,H,W,Ci] dense; wp the weights PACKED as
 *   [kt][kh][kw][Ci][Co] (a permutation of the reference's [Co,Ci,kt,kh,kw]; BatchNorm, where a layer has one, folded in by the caller);
 *   bias [Co]; y [N,To,Ho,Wo,ldy], of which only channels coff .. coff + Co - 1 are written (the branches of an Inception block share one
 *   tensor). relu: 0 / 1. Operands are exact fp32 on the fp32 MFMA; every output sums K in one fixed order, whatever the batch size.
 *   Kernel and stride sides up to 15. No workspace (the query answers 0).
 * vpx_maxpool3d_same: the max over windows of the ZERO-padded map, as the reference pads before it pools: a window that touches the border
 *   never returns less than 0. NaN wins, as in torch. No workspace.
 * vpx_fvd_head: out [N, n_features] = bias + w [n_features, C] * (mean over the positions of x [N,2,7,7,C]); double arithmetic, rounded
 *   once. A map that is not 2x7x7 is VPX_ERR_ARG; C <= 4096. No workspace.
 * vpx_fvd_features: out [n0 + n1, n_features] of the clips x0 [n0,T,C,h,w] and, behind them, x1 [n1,T,C,h,w] (NULL with n1 = 0): planar
 *   frames, values as they are. They are resized to 224x224 (bilinear, align_corners = False, no antialiasing, the arithmetic of
 *   vpx_frames_adapt bit for bit; 224x224 frames are copied) straight into the channels-last stem input, then the rows of `table` run.
 *   A row has VPX_FVD_ROW ints: op, src, dst, Ci, Co, kt, kh, kw, st, sh, sw, relu, coff, ld, param, 0. src and dst are two different ones of
 *   four buffers, buffer 0 the staged clips. VPX_FVD_CONV writes channels coff .. coff + Co - 1 of a map of channel stride ld into dst from
 *   params[param] (packed weights, as above) and params[param + 1] (bias); VPX_FVD_POOL pools src into dst; VPX_FVD_HEAD, the last row,
 *   reads params[param] ([Co, Ci]) and params[param + 1] and writes `out`. `table` lives on the HOST, `params` is a host array of
 *   device pointers. VPX_ERR_ARG: a row whose Ci is not its source's channel count, a buffer read before it is written, a final map
 *   that is not 2x7x7 (clips of 9 .. 16 frames give it). Workspace: vpx_fvd_features_workspace_bytes(n0 + n1, ...), 0 for a refusal.
 * vpx_frechet_distance: *out (ONE double on the device) = fact sum Ep^2 + fact sum Et^2 - 2 sum_i sqrt(sigma_i^2 + 1e-15) + |mu_p - mu_t|^2
 *   for pred, target [b, n] float32, E the centred tables, fact = 1 / (b - 1) (1 for b = 1), sigma_i the singular values of the b x b
 *   matrix fact Ep Et^T: the reference's calculate_2_wasserstein_dist restated, in float64, every sum in one fixed order. The singular
 *   values come from a one-sided Jacobi iteration of at most 80 sweeps; input on which an 80th sweep still rotates gives NaN, never an
 *   unconverged number. b <= 256 (VPX_ERR_UNSUPPORTED beyond). */
#define VPX_FVD_ROW 16
enum { VPX_FVD_CONV = 0, VPX_FVD_POOL = 1, VPX_FVD_HEAD = 2 };
int vpx_same_padding(int size, int k, int s, int* front, int* out);
size_t vpx_conv3d_same_workspace_bytes(void);
int vpx_conv3d_same(const float* x, const float* wp, const float* bias, float* y, long long N, int T, int H, int W, int Ci, int Co,
                    int kt, int kh, int kw, int st, int sh, int sw, int relu, int ldy, int coff, void* stream);
size_t vpx_maxpool3d_same_workspace_bytes(void);
int vpx_maxpool3d_same(const float* x, float* y, long long N, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh, int sw,
                       void* stream);
size_t vpx_fvd_head_workspace_bytes(void);
int vpx_fvd_head(const float* x, const float* w, const float* bias, float* out, long long N, int T, int H, int W, int C, int n_features,
                 void* stream);
size_t vpx_fvd_features_workspace_bytes(long long n_clips, int T, int C, int h, int w, const int* table, int n_rows);
int vpx_fvd_features(const float* x0, const float* x1, long long n0, long long n1, int T, int C, int h, int w, const int* table, int n_rows,
                     const float* const* params, int n_params, float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t vpx_frechet_distance_workspace_bytes(int b, int n);
int vpx_frechet_distance(const float* pred, const float* target, int b, int n, double* out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- plain stride-1 "same" convolution, NHWC, optional bias; y [N,H,W,Co] = conv(x [N,H,W,Ci], w [Co,Ci,kh,kw]) --- */
size_t vpx_conv2d_workspace_bytes(int Ci, int Co, int kh, int kw);
int vpx_conv2d_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Ci,
                        int Co, int kh, int kw, int precision, void* workspace, size_t workspace_bytes, void* stream);

/* backward of the same convolution: dx [N,H,W,Ci], dw [Co,Ci,kh,kw], db [Co]; each may be NULL (skipped), all OVERWRITTEN */
size_t vpx_conv2d_bwd_workspace_bytes(int N, int H, int W, int Ci, int Co, int kh, int kw);
int vpx_conv2d_nhwc_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int N, int H,
                        int W, int Ci, int Co, int kh, int kw, int precision, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- general 2-D convolution / transposed convolution with fused bias + LeakyReLU (the EF "stage glue":
 *      vp_suite/models/precipitation_nowcasting/ef_blocks.py:15-49, layer table ef_conv_lstm.py:36-65) -------------- */
typedef struct vpx_conv_desc {
    int32_t N, H, W, Ci, Co;       /* input x [N,H,W,Ci] (NHWC) */
    int32_t kh, kw, stride, pad;   /* stride 1 or 2; any padding */
    int32_t transposed;            /* 0: nn.Conv2d weight [Co,Ci,kh,kw]; 1: nn.ConvTranspose2d weight [Ci,Co,kh,kw] */
    float leaky_slope;             /* LeakyReLU negative slope fused after the bias; 0 = no activation */
    int32_t precision;             /* VPX_PREC_* */
    int32_t out_pad_h, out_pad_w;  /* transposed only: nn.ConvTranspose2d output_padding (0 .. stride-1) */
} vpx_conv_desc;
int vpx_conv2d_ex_out_shape(const vpx_conv_desc* d, int* Ho, int* Wo);
size_t vpx_conv2d_ex_workspace_bytes(const vpx_conv_desc* d);
/* y [N,Ho,Wo,Co]. A stride-2 transposed convolution runs as 4 output-phase launches of the same kernel. */
int vpx_conv2d_ex_fwd(const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same layer with the output (also) in the split-bf16 operand format (see vpx_convlstm_takes_split_input): y_split
 * [N,Ho,Wo,Co] split-encoded, Co % 8 == 0; y may be NULL (inference: nobody reads the fp32 copy). */
int vpx_conv2d_ex_fwd_split(const vpx_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* y_split,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same layer on SPLIT-format input (x_split: [N,H,W,Ci] split-encoded; image n at (n / x_nT) * x_bstride + (n % x_nT) *
 * x_tstride bytes, x_bstride = 0: dense, x_nT <= 1: plain batch), on the schedule-driven K = 32 kernel (csrc/convq.hip): bf16x3,
 * Ci % 16 == 0, stride 1 or 2, taps within one pixel of the (sub-)image grid (3x3 pad 1, 4x4 stride 2 pad 1, plain or transposed)
 * — vpx_conv2d_ex_takes_split says whether a descriptor qualifies (0 no; 1 yes; 2 yes, and on the schedule-driven K = 32 kernel,
 *   which is worth a vpx_split_convert of an fp32 input for stride-2 transposed layers — or, for 3x3 stride-1 pad-1 layers with 16
 *   output channels and 16..64 input channels, on the resident-weights kernel of csrc/conv16.hip). y (fp32) and y_split may each be NULL, not both.
 * weights_packed: the workspace still holds this layer's packed weights (same values, same descriptor) — the pack launch is skipped
 *   (both kernels; on the first-generation kernel for the single-launch forms: a stride-2 transposed layer's four phase launches
 *   share the space and pack every time). */
int vpx_conv2d_ex_takes_split(const vpx_conv_desc* d);
/* fp32 channels-last pixels [n_pixels][C] -> the split-bf16 operand format (per pixel and 8 channels: 8 hi bf16, 8 lo bf16; the
 * same n_pixels * C * 4 bytes), C % 8 == 0: what the recurrent blocks and vpx_conv2d_ex_fwd_split write themselves. */
int vpx_split_convert(const float* x, void* x_split, long long n_pixels, int C, void* stream);
size_t vpx_conv2d_ex_split_workspace_bytes(const vpx_conv_desc* d);
int vpx_conv2d_ex_fwd_from_split(const vpx_conv_desc* d, const void* x_split, long long x_bstride, long long x_tstride, int x_nT,
                                 const float* w, const float* bias, float* y, void* y_split, int weights_packed, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* Backward of the same layer (the reference gets it from autograd over nn.Conv2d / nn.ConvTranspose2d (+ LeakyReLU),
 * ef_blocks.py:15-49): dy [N,Ho,Wo,Co] is the gradient w.r.t. the layer OUTPUT (after bias and activation); y is that
 * output as vpx_conv2d_ex_fwd produced it — needed (and only read) when d->leaky_slope != 0: the activation derivative is
 * taken from its sign. dx [N,H,W,Ci], dw (layout of w) and db [Co] are written; each may be NULL. db and the LeakyReLU'
 * scaling are one pass over dy, summed in a fixed order (bit-reproducible).
 * dx is the adjoint layer run forward (transposed <-> plain, through vpx_conv2d_ex_fwd's kernels); dw contracts dy with
 * the stride-decimated sub-images of x (or x with those of dy) on the MFMA weight-gradient kernel. Needs kh, kw >= stride. */
size_t vpx_conv2d_ex_bwd_workspace_bytes(const vpx_conv_desc* d);
int vpx_conv2d_ex_bwd(const vpx_conv_desc* d, const float* x, const float* w, const float* y, const float* dy, float* dx,
                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* Round 6: with bf16x3 operands and channel counts in groups of 8 (vpx_conv2d_ex_bwd_uses_split(d) != 0) the weight gradient runs
 * per stride residue on split copies of x and dy (csrc/wgrad2.hip, glue form). _bwd converts x itself; a caller that ran the forward
 * through vpx_conv2d_ex_fwd_from_split hands that x_split [N,H,W,Ci] back to _bwd_ex and saves the pass (x stays required: residues of a
 * single tap and the other operand modes read it). x_split == NULL: exactly vpx_conv2d_ex_bwd. */
int vpx_conv2d_ex_bwd_uses_split(const vpx_conv_desc* d);
int vpx_conv2d_ex_bwd_ex(const vpx_conv_desc* d, const float* x, const void* x_split, const float* w, const float* y, const float* dy,
                         float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* y = act(conv(x, w) + bias [+ y]): the stride-1 "same" convolution of vpx_conv2d_nhwc_fwd with an optional accumulate
 * into the destination (two convolutions summed into one output) and LeakyReLU (slope >= 0, 0 = none) applied to the sum.
 * Workspace: vpx_conv2d_workspace_bytes(Ci, Co, kh, kw). */
int vpx_conv2d_nhwc_fwd_ex(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Ci, int Co,
                           int kh, int kw, int precision, int accumulate, float leaky_slope, void* workspace,
                           size_t workspace_bytes, void* stream);
/* ---- TrajGRU over a sequence (vp_suite/model_blocks/traj_gru.py:164-214), time-major NHWC ---------------------------------- *
 * One call runs the block's whole time loop: the input projection i2h of all frames (one launch), then per step the flow generator
 * (two 5x5 convolutions summed + LeakyReLU, the 5x5 flow convolution, :134-146), the L bilinear warps of h_{t-1} along -flow with the
 * reference's normalisation (divide by W-1 / H-1, grid_sample align_corners=False, zero padding, :148-162), the 1x1 `ret`
 * convolution and the GRU gates r = s(i0+h0), u = s(i1+h1), m = leaky(i2 + r*h2), h_t = u*h_{t-1} + (1-u)*m (:190-203). The backward
 * is the explicit BPTT schedule of the same launches (the warped operand is recomputed per step, not stored).
 *   x  [T][B][H*W][Cin] or NULL (no input: zero projection)      h0 [B][H*W][C] or NULL (zero state); not both NULL
 *   params / dparams: 10 pointers in the order (i2h, i2f_conv1, h2f_conv1, flows_conv, ret) x (weight OIHW, bias); with x == NULL the
 *        first four gradients are not written (may be NULL). Parameter gradients are OVERWRITTEN.
 *   hs [T][B][H*W][C]: h_1 .. h_T (forward output, backward input)       dout [T][B][H*W][C] or NULL, dhT [B][H*W][C] or NULL
 *   reserve: vpx_trajgru_reserve_bytes (0 without VPX_FLAG_SAVE_FOR_BWD); workspace: vpx_trajgru_workspace_bytes
 * The warp backward scatters with float atomics (like torch's grid_sample backward: sum order depends on timing); under
 * vpx_set_deterministic(1) it scatters 2^40-scaled 64-bit integers instead (associative, hence bit-reproducible; resolution 9e-13,
 * range +-8.4e6 per element). Restrictions: C % 4 == 0, i2h a square odd stride-1 'same' convolution, slope > 0, zoneout = 0. */
typedef struct vpx_trajgru_desc {
    int32_t B, T, Cin, C, H, W;
    int32_t L;             /* flow fields / warps per step */
    int32_t k_i2h;         /* kernel size of the input projection */
    int32_t precision;     /* vpx_precision: arithmetic of the five convolutions */
    int32_t flags;         /* VPX_FLAG_SAVE_FOR_BWD */
    float slope;           /* LeakyReLU negative slope (> 0) */
} vpx_trajgru_desc;
size_t vpx_trajgru_workspace_bytes(const vpx_trajgru_desc* d);
size_t vpx_trajgru_reserve_bytes(const vpx_trajgru_desc* d);
int vpx_trajgru_seq_fwd(const vpx_trajgru_desc* d, const float* x, const float* h0, const float* const* params, float* hs, void* reserve,
                        size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream);
int vpx_trajgru_seq_bwd(const vpx_trajgru_desc* d, const float* x, const float* h0, const float* const* params, const float* hs,
                        const void* reserve, size_t reserve_bytes, const float* dout, const float* dhT, float* dx, float* dh0,
                        float* const* dparams, void* workspace, size_t workspace_bytes, void* stream);

/* ---- action-conditional ST-LSTM cell, one step (vp_suite/model_blocks/predrnn.py:86-169), NHWC ------------------------------ *
 * replaces ActionConditionalSpatioTemporalLSTMCell.forward (:139-169) and its autograd: x_concat = conv_x(x), h_concat = conv_h(h),
 * a_concat = conv_a(a), m_concat = conv_m(m) — Conv2d WITH bias, each followed by LayerNorm([C,H,W]) when layer_norm (:102-136) —
 * h_concat * a_concat (:144), both gate groups and the state updates (:146-164), conv_o / conv_last on mem = (c_new | m_new), the
 * output gate (:165-167). Tensors are [B][H*W][C] (x: Cin channels; h, c, m, a and all outputs: Ch).
 *   params / dparams: 12 pointers, (conv_x, conv_h, conv_a, conv_m, conv_o, conv_last) x (weight OIHW, bias); conv_x [7Ch,Cin,k,k],
 *        conv_h / conv_a [4Ch,Ch,k,k], conv_m [3Ch,Ch,k,k], conv_o [Ch,2Ch,k,k], conv_last [Ch,2Ch,1,1]. A NULL dparams entry is skipped
 *        (frozen parameter); gradients are OVERWRITTEN.
 *   ln / dln: 10 pointers, (x, h, a, m, o) x (weight, bias) in the reference's [C,H,W] layout; NULL unless layer_norm (eps = 1e-5).
 *   backward: dh_new is required; dc_new / dm_new / ddc / ddm (gradients of c_new, m_new, delta_c, delta_m) may be NULL = zero;
 *        dx / dh / dc / dm / da may be NULL (not wanted).
 *   reserve: vpx_acstlstm_reserve_bytes (0 without VPX_FLAG_SAVE_FOR_BWD), written by the forward, read by the backward.
 * First-generation convolution kernels in every precision; k odd, stride 1. */
typedef struct vpx_acstlstm_desc {
    int32_t B, Cin, Ch, H, W;
    int32_t k;             /* kernel size of conv_x / conv_h / conv_a / conv_m / conv_o ('same', stride 1) */
    int32_t layer_norm;    /* LayerNorm after those five convolutions */
    int32_t precision;     /* VPX_PREC_* of the six convolutions */
    int32_t flags;         /* VPX_FLAG_SAVE_FOR_BWD */
    float forget_bias;     /* added to both forget gates' pre-activations (the reference: 1.0) */
} vpx_acstlstm_desc;
size_t vpx_acstlstm_workspace_bytes(const vpx_acstlstm_desc* d);
size_t vpx_acstlstm_reserve_bytes(const vpx_acstlstm_desc* d);
int vpx_acstlstm_step_fwd(const vpx_acstlstm_desc* d, const float* x, const float* h, const float* c, const float* m, const float* a,
                          const float* const* params, const float* const* ln, float* h_new, float* c_new, float* m_new, float* delta_c,
                          float* delta_m, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, void* stream);
int vpx_acstlstm_step_bwd(const vpx_acstlstm_desc* d, const float* x, const float* h, const float* c, const float* m, const float* a,
                          const float* const* params, const float* const* ln, const void* reserve, size_t reserve_bytes, const float* dh_new,
                          const float* dc_new, const float* dm_new, const float* ddc, const float* ddm, float* dx, float* dh, float* dc, float* dm,
                          float* da, float* const* dparams, float* const* dln, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LayerNorm([C,H,W]) per sample on NHWC tensors (predrnn.py:27-40, 105-135; eps = 1e-5) ---------------------------------- *
 * x, y, xhat: [B][n = H*W*C]; gamma, beta (and dgamma, dbeta): [H*W][C], i.e. the reference's [C,H,W] parameters channels-last;
 * stats [B][2] = (mean, 1/std) and xhat (optional in the forward: NULL skips the store) feed the backward. Sums run in double over
 * fixed chunks (bit-reproducible); dgamma / dbeta are OVERWRITTEN. */
size_t vpx_layernorm_workspace_bytes(int B);
int vpx_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* xhat, float* stats, int B, long long n,
                      void* workspace, size_t workspace_bytes, void* stream);
int vpx_layernorm_bwd(const float* dy, const float* xhat, const float* stats, const float* gamma, float* dx, float* dgamma, float* dbeta,
                      int B, int HW, int C, void* workspace, size_t workspace_bytes, void* stream);

/* ---- GroupNorm(G, C) + optional LeakyReLU + optional residual on NHWC tensors (conv.py DCGANConv / DCGANConvTranspose,
 *      phydnet.py PhyCell_Cell.F; eps = 1e-5, biased variance) ----------------------------------------------------------------- *
 * x, y, r: [N][HW][C]; gamma, beta: [C]; stats [N][G][2] = (mean, 1/std) written by the forward for the backward.
 * y = act(x̂ * gamma + beta) + r, act = LeakyReLU(slope) when `act` != 0 else the identity, r optional (NULL: no residual; its gradient
 * is dy itself). One launch forward (one workgroup per (sample, group), exact two-pass variance in fp32 with fixed-order sums).
 * The backward recomputes x̂ from x and stats and takes the activation's derivative from the sign of the recomputed pre-activation;
 * dgamma / dbeta (OVERWRITTEN, optional: both or neither) are reduced through per-sample partials in the workspace in a fixed order
 * (no atomics: bit-reproducible in every mode). Two launches. */
int vpx_groupnorm_fwd(const float* x, const float* gamma, const float* beta, const float* r, float* y, float* stats, int N, int HW, int C,
                      int G, int act, float slope, void* stream);
size_t vpx_groupnorm_bwd_workspace_bytes(int N, int C);
int vpx_groupnorm_bwd(const float* x, const float* stats, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                      float* dbeta, int N, int HW, int C, int G, int act, float slope, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PhyDNet (models/phydnet.py, model_blocks/phydnet.py) ------------------------------------------------------------------------ *
 * PhyCell correction, n elements of one layout: next = (h + Fh) + sigmoid(G) * (E - (h + Fh)). The backward writes dG, dh (the direct
 * part; the convolution paths add to it), dFh and dE; any of the four may be NULL. */
int vpx_phycell_correct_fwd(const float* G, const float* Fh, const float* h, const float* E, float* next, long long n, void* stream);
int vpx_phycell_correct_bwd(const float* G, const float* Fh, const float* h, const float* E, const float* dnext, float* dG, float* dh,
                            float* dFh, float* dE, long long n, void* stream);
/* Moment loss of the PhyCell's first filter bank W [hidden][Cin][kh][kw] (kh, kw <= 8): for every input channel b,
 * moment[o] = M0 · W[o, b] · M1^T with M[i][u] = (u - (k-1)/2)^i / i! (K2M), loss = scale * sum_b mean((moment - C)^2) with
 * C[o][i][j] = (o == i*kw + j). Computed in fp64, written as fp32 to *loss (one launch). The backward reads dloss from device memory
 * and OVERWRITES dW = dloss * scale * 2/(hidden*kh*kw) * M0^T (moment - C) M1. */
int vpx_moment_loss_fwd(const float* W, float* loss, int hidden, int Cin, int kh, int kw, float scale, void* stream);
int vpx_moment_loss_bwd(const float* W, const float* dloss, float* dW, int hidden, int Cin, int kh, int kw, float scale, void* stream);
/* Sigmoid output head: x holds nT frames time-major NHWC [nT][B][H*W][C]; frame k lands in slot t0 + k of out [B][T][C][H][W].
 * The backward reads that slot of out (the saved sigmoid) and of dout and writes dx in x's layout. */
int vpx_sigmoid_head_fwd(const float* x, float* out, int B, int T, int t0, int nT, int C, int H, int W, void* stream);
int vpx_sigmoid_head_bwd(const float* out, const float* dout, float* dx, int B, int T, int t0, int nT, int C, int H, int W, void* stream);

/* ---- ST-Phy (models/st_phy.py, model_blocks/enc.py Autoencoder) ------------------------------------------------------------------- *
 * The layers of vpx_conv2d_ex_fwd / _bwd with an activation code beside the descriptor (whose leaky_slope == 0 means "none", so ReLU
 * cannot be said there). VPX_ACT_RELU needs leaky_slope == 0 and is applied in the epilogue of the implicit-GEMM launch(es) that run
 * the layer; VPX_ACT_NONE is exactly vpx_conv2d_ex_fwd / _bwd (y may be NULL in the backward). The backward reads ReLU' off the saved
 * output y (y > 0; zero at y == 0) in the pass that sums the bias gradient; that pass MULTIPLIES dy by the 0 / 1 derivative, so a
 * non-finite dy at a dead unit yields NaN (torch selects 0 there). Workspaces: the *_act_* queries (same sizes as the plain layer's). */
enum { VPX_ACT_NONE = 0, VPX_ACT_RELU = 1 };
size_t vpx_conv2d_act_workspace_bytes(const vpx_conv_desc* d, int act);
int vpx_conv2d_act_fwd(const vpx_conv_desc* d, int act, const float* x, const float* w, const float* bias, float* y, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t vpx_conv2d_act_bwd_workspace_bytes(const vpx_conv_desc* d, int act);
int vpx_conv2d_act_bwd(const vpx_conv_desc* d, int act, const float* x, const float* w, const float* y, const float* dy, float* dx,
                       float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* Encoder tail: y = r / max(||r||_2 over W, eps), r = relu(x), per (sample, row, channel) of x [N][H][W][C] (F.normalize(relu(x),
 * p=2, dim=-1, eps) on the reference's NCHW tensor). norm [N][H][C] (nullable in the forward) receives ||r||_2 for the backward, which
 * writes dx = relu'(x) * (dy - y <dy, y>) / norm where norm >= eps and relu'(x) * dy / eps below it. One launch each. */
int vpx_relu_rownorm_fwd(const float* x, float* y, float* norm, int N, int H, int W, int C, float eps, void* stream);
int vpx_relu_rownorm_bwd(const float* x, const float* norm, const float* dy, float* dx, int N, int H, int W, int C, float eps, void* stream);
/* Merge: y [N,H,W,Co] = w[:, :Cs] a + w[:, Cs:] b + bias for a [N,H,W,Cs], b [N,H,W,Cp], w [Co, Cs+Cp] (the 1x1 Conv2d over
 * cat([a, b], dim=1), never materialised); bias nullable. precision: VPX_PREC_F32 | VPX_PREC_BF16X3. The backward OVERWRITES
 * da, db, dw [Co, Cs+Cp], dbias [Co] (each nullable); parameter gradients are fixed-order sums (bit-reproducible). y, da and db come
 * from K-split launches with float atomics on small maps unless vpx_set_deterministic(1). */
size_t vpx_merge1x1_workspace_bytes(int Cs, int Cp, int Co);
int vpx_merge1x1_fwd(const float* a, const float* b, const float* w, const float* bias, float* y, int N, int H, int W, int Cs, int Cp,
                     int Co, int precision, void* workspace, size_t workspace_bytes, void* stream);
size_t vpx_merge1x1_bwd_workspace_bytes(int N, int H, int W, int Cs, int Cp, int Co);
int vpx_merge1x1_bwd(const float* a, const float* b, const float* w, const float* dy, float* da, float* db, float* dw, float* dbias, int N,
                     int H, int W, int Cs, int Cp, int Co, int precision, void* workspace, size_t workspace_bytes, void* stream);

/* ---- UNet-3D (models/unet3d.py, model_blocks/conv.py DoubleConv2d / DoubleConv3d) --------------------------------------------------- *
 * Activations are channels-last per frame: [B][T][H][W][C]; a 2-D layer is T = 1, kt = 1. Weights keep the reference's layout
 * [Co][Ca+Cb][kt][ks][ks]. VPX_RCONV_REPLICATE: 3x3 in space, kt in {1, 3} taps in time, frame and pixel index clamped (padding 1,
 * padding_mode 'replicate'), no bias. VPX_RCONV_COLLAPSE: Conv3d(C -> Co, (T,1,1)) + squeeze: kt == T, one output frame [B][1][H][W][Co].
 * The input may be two channel-concatenated sources a [..][Ca] and b [..][Cb] (Cb = 0, b = NULL: one source). fp32 FMA, every sum in a
 * fixed order (bit-reproducible in every mode).
 * Epilogues of the forward: PLAIN writes y (+ gamma_or_bias as a bias, nullable). EVAL writes relu((y - running_mean) / sqrt(running_var +
 * eps) * gamma + beta). STATS writes the raw y, stats [2][Co] = (batch mean, 1 / sqrt(biased batch variance + eps)) and, when the running
 * statistics are given, running = (1 - momentum) * running + momentum * (mean, UNBIASED variance); it needs more than one value per
 * channel. The backward is that of the PLAIN / raw output: da, db, dw, dbias (each nullable) are OVERWRITTEN. */
enum { VPX_RCONV_REPLICATE = 0, VPX_RCONV_COLLAPSE = 1 };
enum { VPX_RCONV_EPI_PLAIN = 0, VPX_RCONV_EPI_EVAL = 1, VPX_RCONV_EPI_STATS = 2 };
typedef struct vpx_rconv_desc {
    int32_t B, T, H, W, Ca, Cb, Co, kt, mode;
} vpx_rconv_desc;
size_t vpx_rconv_workspace_bytes(const vpx_rconv_desc* d, int epilogue);
int vpx_rconv_fwd(const vpx_rconv_desc* d, int epilogue, const float* a, const float* b, const float* w, const float* gamma_or_bias,
                  const float* beta, float* running_mean, float* running_var, float eps, float momentum, float* y, float* stats,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t vpx_rconv_bwd_workspace_bytes(const vpx_rconv_desc* d);
int vpx_rconv_bwd(const vpx_rconv_desc* d, const float* a, const float* b, const float* w, const float* dy, float* da, float* db, float* dw,
                  float* dbias, void* workspace, size_t workspace_bytes, void* stream);
/* BatchNorm + ReLU on the raw output x [N][H][W][C] (N = B*T) with the statistics of the STATS epilogue: act = relu((x - mean) / std *
 * gamma + beta); `pooled` (nullable; even H, W) also receives the 2x2 max-pool of act, [N][H/2][W/2][C], in the same pass. stats == NULL:
 * x already is an activation and only `pooled` is written (act == NULL). The backward takes the gradients of act and of pooled (either
 * nullable), routes the pooled one to the first maximum of its window in row-major order, reads ReLU' off act (zero at 0) and writes dx,
 * dgamma, dbeta (the last two nullable, OVERWRITTEN): a reduction pass over per-block partials added in block order, then an apply pass. */
int vpx_bn_relu_fwd(const float* x, const float* stats, const float* gamma, const float* beta, float* act, float* pooled, long long N, int H,
                    int W, int C, void* stream);
size_t vpx_bn_relu_bwd_workspace_bytes(long long N, int H, int W, int C);
int vpx_bn_relu_bwd(const float* x, const float* act, const float* stats, const float* gamma, const float* dact, const float* dpool, float* dx,
                    float* dgamma, float* dbeta, long long N, int H, int W, int C, void* workspace, size_t workspace_bytes, void* stream);

/* ---- NonConvLSTM (models/lstm.py): dense layer, LSTM cell, replicate padding, differentiable resize ------------------------------------ *
 * Everything is fp32 FMA. Every sum runs in a fixed order and no launch uses float atomics: equal bits run to run in every mode.
 *
 * Dense layer: y [M][N] = x [M][K] * w [N][K]^T + bias [N] (nullable), then ReLU when relu != 0. x and y have row strides ldx >= K and
 * ldy >= N in elements (a result may be a column slice of a wider buffer; the elements between the rows are never touched); w is the
 * Linear's weight as stored. The launch is planned from (M, N, K) alone: a tile form from M (8 x 128 for M <= 8, 32 x 32 for M <= 32,
 * else 128 x 32 rows x columns; all rows of M <= 128 are one workgroup's, so a weight element is read from memory by one workgroup) and
 * a K split where the tiles alone leave CUs idle: min(ceil(512 / tiles), K / 256, 64) chunks of a length rounded up to 32; the partial
 * sums [chunk][M][N] live in the workspace and a second launch adds them in chunk order, adds the bias and applies ReLU.
 * vpx_dense_plan answers the plan of a forward (for the data gradient call it with N and K exchanged): it is filled by the function
 * that plans the launches.
 * Backward: dx [M][K] (row stride lddx) = dy' * w, dw [N][K] = dy'^T * x, db [N] = column sums of dy', where dy' = dy (row stride lddy)
 * or, with relu != 0, dy masked by y > 0 (y: the forward's output, row stride ldy; otherwise y may be NULL). dx, dw, db are each nullable.
 * accumulate != 0 ADDS to dw and db (the parameter gradients) instead of overwriting them; dx is always overwritten.
 * One workspace query covers both directions. VPX_ERR_ARG: a size < 1, a NULL operand, a row stride shorter than its row.
 * VPX_ERR_UNSUPPORTED: sizes beyond one launch. VPX_ERR_WORKSPACE: workspace NULL or smaller than the query's answer. */
typedef struct vpx_dense_plan_info {
    int32_t split;       /* 0: single pass (bias / ReLU in the epilogue); 1: K split + reduction */
    int32_t chunks;      /* K chunks (1 without a split) */
    int32_t chunk_len;   /* elements of K per chunk, a multiple of 32; the last chunk may be shorter */
    int32_t form;        /* tile form 0 / 1 / 2 */
    int32_t tile_m, tile_n, m_tiles, n_tiles;
} vpx_dense_plan_info;
int vpx_dense_plan(long long M, long long N, long long K, vpx_dense_plan_info* out);
size_t vpx_dense_workspace_bytes(long long M, long long N, long long K);
int vpx_dense_fwd(const float* x, long long ldx, const float* w, const float* bias, float* y, long long ldy, long long M, long long N, long long K,
                  int relu, void* workspace, size_t workspace_bytes, void* stream);
int vpx_dense_bwd(const float* x, long long ldx, const float* w, const float* y, long long ldy, const float* dy, long long lddy, float* dx,
                  long long lddx, float* dw, float* db, long long M, long long N, long long K, int relu, int accumulate, void* workspace,
                  size_t workspace_bytes, void* stream);
/* LSTM cell (torch.nn.LSTMCell, gate order i, f, g, o): gates = x [M][Kx] * w_ih [4H][Kx]^T + h [M][H] * w_hh [4H][H]^T + b_ih + b_hh;
 * c_new = sigmoid(f) * c + sigmoid(i) * tanh(g); h_new = sigmoid(o) * tanh(c_new). One call per layer-step: the two products are ONE K loop
 * over [x | h] on the dense layer's launch, whose columns are walked gate-interleaved so that a thread holds the four gates of a hidden
 * unit; the gate arithmetic is that launch's epilogue, or the reduction's where the plan of (M, 4H, Kx + H) splits K.
 * x has a row stride ldx >= Kx; h, c, h_new, c_new are dense [M][H]. h == NULL means a zero hidden state: the h * w_hh^T half is skipped
 * (the plan is that of (M, 4H, Kx)); c == NULL a zero cell state. The biases are nullable. `gates` (nullable) receives the ACTIVATED gates
 * [M][4H] = [i | f | g | o]: the reserve the backward needs.
 * Backward: from dh_new and dc_new (either may be NULL = zero), the reserve and c, it writes the gate gradient dgates [M][4H] (required:
 * it is also the operand of everything below), dc = dc_total * f, dx = dgates * w_ih (dense [M][Kx]), dh = dgates * w_hh, dw_ih = dgates^T x,
 * dw_hh = dgates^T h (zero for h == NULL), db_ih = db_hh = column sums of dgates; every output but dgates is nullable. accumulate != 0 ADDS
 * to the four parameter gradients, so the steps of a pass can sum into one buffer. One workspace query covers both directions.
 * Error codes as for the dense layer. */
size_t vpx_lstm_cell_workspace_bytes(long long M, long long Kx, long long H);
int vpx_lstm_cell_fwd(const float* x, long long ldx, const float* h, const float* c, const float* w_ih, const float* w_hh, const float* b_ih,
                      const float* b_hh, float* h_new, float* c_new, float* gates, long long M, long long Kx, long long H, void* workspace,
                      size_t workspace_bytes, void* stream);
int vpx_lstm_cell_bwd(const float* x, long long ldx, const float* h, const float* c, const float* w_ih, const float* w_hh, const float* gates,
                      const float* dh_new, const float* dc_new, float* dx, float* dh, float* dc, float* dw_ih, float* dw_hh, float* db_ih,
                      float* db_hh, float* dgates, long long M, long long Kx, long long H, int accumulate, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Replicate padding of channels-last maps: y [N][H + 2 pad][W + 2 pad][C] with y[.., yy, xx, ..] = x[.., clamp(yy - pad), clamp(xx - pad), ..]
 * (F.pad(mode="replicate")); a Conv2d with padding_mode="replicate" is this followed by the unpadded convolution. The backward is the
 * adjoint as a gather: dx [N][H][W][C] sums, row by row, the padded cells that copied each pixel. One launch each, no workspace.
 * VPX_ERR_ARG: a NULL pointer, a size < 1, pad < 0. VPX_ERR_UNSUPPORTED: a side beyond 32768, more work than one launch holds. */
int vpx_replicate_pad_fwd(const float* x, float* y, long long N, int H, int W, int C, int pad, void* stream);
int vpx_replicate_pad_bwd(const float* dy, float* dx, long long N, int H, int W, int C, int pad, void* stream);
/* Differentiable bilinear resize: x channels-last [N][H][W][C] -> y planar [N][C][oh][ow], align_corners = False, no antialiasing (the model
 * only enlarges; a side that shrinks is point-sampled between two taps as F.interpolate does, not averaged), the fp32 source coordinates of vpx_frames_preprocess and vpx_frames_adapt, horizontally first, every operation
 * rounded on its own (held to a bound, not to bits). The backward takes dy planar and writes dx channels-last as a gather per source pixel
 * over the output pixels whose taps name it, in row-major order. One launch each, no workspace.
 * VPX_ERR_ARG: a NULL pointer, a size < 1. VPX_ERR_UNSUPPORTED: a side beyond 32768, more work than one launch holds. */
int vpx_resize_bilinear_fwd(const float* x, float* y, long long N, int C, int H, int W, int oh, int ow, void* stream);
int vpx_resize_bilinear_bwd(const float* dy, float* dx, long long N, int C, int H, int W, int oh, int ow, void* stream);

/* ---- Moving MNIST generated on the device (vp_suite/datasets/mmnist_on_the_fly.py) ------------------------------
 * out [B, n_frames, C, S, S] (dense fp32, the reference's layout) from digits [n_glyphs, glyph_size, glyph_size] (bytes) and
 * params [B, D, 5] (int32): per sample and digit (glyph index, y0, x0, vy, vx). Per axis and frame: p += v; if p + glyph_size > S then
 * p = S - glyph_size, v = -v; else if p < 0 then p = -p, v = -v. Frame i shows the positions after i + 1 moves. A pixel is, in float64,
 * a = sum over the digits in order of double(g) / 255.0 where the digit's box holds it; a = min(max(a, 0), 1); a = a * 255.0 / 255.0
 * (two operations); x = float(a); then only if (lo, hi) != (0, 1): x = x * float(hi - lo), x = x + float(lo), each rounded to fp32 on
 * its own. All C channels carry x. One launch, no workspace, no atomics: the same bits in either determinism mode.
 * VPX_ERR_ARG: a NULL pointer, C not 1 or 3, glyph_size >= S, D < 1, a size < 1. VPX_ERR_UNSUPPORTED: D > 16, D * glyph_size^2 > 48 KiB, S > 16384, n_frames > 65536,
 * more workgroups than one launch holds. `params` lives on the device, so the CALLER checks it: a glyph index outside [0, n_glyphs) draws
 * nothing and a position or speed that leaves the image is drawn clipped, but neither reads or writes out of bounds. */
int vpx_mmnist_frames(const unsigned char* digits, int n_glyphs, int glyph_size, const int* params, int B, int D, int n_frames, int C, int S,
                      double lo, double hi, float* out, void* stream);

/* ---- stored frames to a model-ready batch and back (vp_suite/base/base_dataset.py preprocess / postprocess) ----------------
 * Preprocess: src [N, T', H, W, Cs] holds raw stored sequences, channels last as the files hold them (a gray [T', H, W] file is Cs = 1),
 * of element type VPX_FRAMES_U8 / _U16 / _F32; table [B, 4] (int32, on the device) holds per output sample (sequence index, crop y0,
 * crop x0, flip bits: bit 0 horizontal, bit 1 vertical); out [B, n_frames, C_out, oh, ow] is dense fp32. Output frame f is stored frame
 * f * seq_step; the crop box is ch x cw at (y0, x0); C_out = Cs, or 3 from Cs = 1 (the gray repeat). One launch, no workspace, no
 * atomics; source offsets are 64-bit. Per element, each step one correctly rounded fp32 operation, never a fused multiply-add:
 *   v = float(raw) / 255.0f (U16: / 65535.0f, F32: v = raw); only if (lo, hi) != (0, 1): v = v * float(hi - lo), then v = v + float(lo).
 * ch == oh and cw == ow: that is the output, bit-exact against numpy. Otherwise a bilinear resize with align_corners = False and no
 * antialiasing follows, per axis in fp32: s = float(in) / float(out); src = max(s * (d + 0.5f) - 0.5f, 0); i0 = int(src);
 * i1 = min(i0 + 1, in - 1); l = src - i0; r = v0 * (1 - l) + v1 * l, horizontally first, then vertically (held to a bound, not to bits).
 * Flips act on the output index after the resize.
 * VPX_ERR_ARG: a NULL pointer, an unknown element type, a size < 1, (n_frames - 1) * seq_step >= T', a crop box larger than the frame,
 * C_out neither Cs nor 3 from 1, hi == lo. VPX_ERR_UNSUPPORTED: Cs > 4, a side beyond 32768, more workgroups than one launch holds.
 * `table` lives on the device, so the CALLER checks it: a row whose sequence index is outside [0, N) or whose box leaves the frame
 * yields zeros and reads nothing out of bounds.
 * Postprocess: x [N, C, h, w] fp32 (only read) -> out [N, h, w, C] bytes; in fp32 v = ((x - float(lo)) / float(hi - lo)) * 255.0f,
 * clamped to [0, 255], truncated toward zero; NaN gives 0. VPX_ERR_ARG: a NULL pointer, a size < 1, hi == lo. */
enum { VPX_FRAMES_U8 = 0, VPX_FRAMES_U16 = 1, VPX_FRAMES_F32 = 2 };
int vpx_frames_preprocess(const void* src, int dtype, long long N, int Tp, int H, int W, int Cs, const int* table, int B, int n_frames,
                          int seq_step, int ch, int cw, int oh, int ow, int C_out, double lo, double hi, float* out, void* stream);
int vpx_frames_postprocess(const float* x, long long N, int C, int h, int w, double lo, double hi, unsigned char* out, void* stream);
/* Windows of long clips (vp_suite/datasets/kitti_raw.py:77-95, caltech_pedestrian.py:69-86): src [total_frames, H, W, Cs] holds every clip
 * of a split back to back, element types as above; clip_first [n_clips + 1] (int64, on the device) holds the first frame of each clip,
 * its last entry total_frames; table [B, 6] (int32, on the device) holds per output sample (clip index, start frame within the clip,
 * crop y0, crop x0, flip bits, 0). out [B, n_frames, C_out, oh, ow] is dense fp32 and output frame f of sample b is stored frame
 * clip_first[clip] + start + f * seq_step. From the frame on, the pixels are those of vpx_frames_preprocess, computed by the same device
 * function: the same scale, crop, resize, flips and gray repeat, bit for bit. One launch, no workspace, no atomics, no host sync; frame
 * offsets are 64-bit (a split may hold tens of gigabytes). Return codes as vpx_frames_preprocess, with total_frames and n_clips among the
 * sizes, n_clips > total_frames and (n_frames - 1) * seq_step >= total_frames VPX_ERR_ARG. `clip_first` and `table` live on the device, so
 * the CALLER checks them: a row whose clip index is outside [0, n_clips), whose window leaves its clip (start < 0 or
 * start + (n_frames - 1) * seq_step >= the clip's length), whose clip leaves src or whose box leaves the frame yields zeros and reads
 * nothing out of bounds. */
int vpx_clips_preprocess(const void* src, int dtype, long long total_frames, int H, int W, int Cs, const long long* clip_first, long long n_clips,
                         const int* table, int B, int n_frames, int seq_step, int ch, int cw, int oh, int ow, int C_out, double lo, double hi,
                         float* out, void* stream);
/* Windows of clips whose FRAME SIZES differ (vp_suite/datasets/human36m.py: 1002 x 1000 videos among 1000 x 1000 ones, resized while
 * they load; here in the launch): src is one element buffer of total_elems elements (element types as above, Cs channels, channels last)
 * that holds every clip back to back; clip_geom [n_clips, 4] (int64, on the device) holds per clip (element offset of its first frame,
 * frame count, H_i, W_i); table [B, 8] (int32, on the device) holds per output sample (clip index, start frame within the clip, box y0,
 * box x0, box h, box w, flip bits, 0). out [B, n_frames, C_out, oh, ow] is dense fp32; output frame f of sample b is frame
 * start + f * seq_step of its clip, and the box of that frame goes to oh x ow through the device function of the two launches above
 * with the sample's sizes in place of the launch's: a box of the output's size is copied (the bits of vpx_clips_preprocess), any other
 * is resized by the same bilinear rule with s = float(box) / float(out) per axis; flips after the resize; the gray repeat. One launch,
 * no workspace, no atomics, no host sync; offsets are 64-bit.
 * VPX_ERR_ARG: a NULL pointer, an unknown element type, a size < 1, n_clips > total_elems / Cs, (n_frames - 1) * seq_step >=
 * total_elems / Cs, C_out neither Cs nor 3 from 1, hi == lo. VPX_ERR_UNSUPPORTED: Cs > 4, an output side beyond 32768, more workgroups
 * than one launch holds. Both tables live on the device, so the CALLER checks them: a row whose clip index is outside [0, n_clips), whose
 * window leaves its clip, whose box is empty or leaves the clip's H_i x W_i frame, or whose clip (a negative offset or a size < 1, a side
 * beyond 32768, offset + count * H_i * W_i * Cs > total_elems) leaves src yields zeros and reads nothing out of bounds. */
int vpx_clips_preprocess_var(const void* src, int dtype, long long total_elems, int Cs, const long long* clip_geom, long long n_clips,
                             const int* table, int B, int n_frames, int seq_step, int oh, int ow, int C_out, double lo, double hi, float* out,
                             void* stream);
/* The action rows that go with such a batch (vp_suite/datasets/bair.py:60-61): src [N, T', A] of element type VPX_ACTIONS_F32 / _F64,
 * the SAME device table [B, 4] as vpx_frames_preprocess of which only column 0 (the sequence index) is read; out [B, n_frames, A] dense
 * fp32, out[b, t, :] = float(src[table[b].seq, t * seq_step, :]). float64 is rounded to nearest even, as numpy's astype(float32) does;
 * float32 is copied; no other arithmetic. One launch on the caller's stream, no workspace, no atomics, no host sync, 64-bit source
 * offsets. VPX_ERR_ARG: a NULL pointer, an unknown element type, a size < 1, (n_frames - 1) * seq_step + 1 > T'. VPX_ERR_UNSUPPORTED: more
 * workgroups than one launch holds. The CALLER checks the table: a sequence index outside [0, N) yields zeros and reads nothing out of
 * bounds. */
enum { VPX_ACTIONS_F32 = 0, VPX_ACTIONS_F64 = 1 };
int vpx_actions_gather(const void* src, int dtype, long long N, int Tp, int A, const int* table, int B, int n_frames, int seq_step,
                       float* out, void* stream);
/* Action rows that are DIFFERENCES of stored positions (vp_suite/datasets/synpick.py:110-113, 135-137): src [total_frames, A] of element
 * type VPX_ACTIONS_F32 / _F64 holds one position row per stored frame, every clip back to back; clip_first [n_clips + 1] (int64, on the
 * device) the first row of each clip; table [B, 8] is the device table of vpx_clips_preprocess_var, of which columns 0 (clip) and 1
 * (start frame) are read. out [B, n_frames - 1, A] dense fp32, out[b, j, :] = float(src[g(j + 1), :] - src[g(j), :]) with
 * g(j) = clip_first[clip] + start + j * seq_step: the subtraction in the source's precision, then ONE rounding to fp32 (nearest even) —
 * numpy's (new - old) followed by .float(). One launch, no workspace, no atomics, no host sync, 64-bit offsets.
 * VPX_ERR_ARG: a NULL pointer, an unknown element type, a size < 1, n_frames == 1, n_clips > total_frames, (n_frames - 1) * seq_step >=
 * total_frames. VPX_ERR_UNSUPPORTED: more workgroups than one launch holds. The CALLER checks the tables: a clip index outside
 * [0, n_clips), a window that leaves its clip or a clip that leaves src yields zeros and reads nothing out of bounds. */
int vpx_actions_diff_gather(const void* src, int dtype, long long total_frames, int A, const long long* clip_first, long long n_clips,
                            const int* table, int B, int n_frames, int seq_step, float* out, void* stream);

/* ---- photometric augmentations and erasing of a preprocessed batch, in place (torchvision's tensor transforms, restated) ----
 * x [B, n_frames, C, h, w] dense fp32, changed in place by ONE launch; programs [B, max_ops, VPX_FRAMES_AUG_ROW] (fp32, on the device):
 * sample b runs rows (opcode, p0 .. p7) until opcode 0 or max_ops rows, the same program on each of its frames (parameters are drawn
 * once per sequence, on the host). Per element every step is one correctly rounded fp32 operation, never a fused multiply-add.
 * clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v), literally, whatever value range the frames are in; gray = (0.2989f r + 0.587f g) + 0.114f b;
 * blend(a, b) = clamp(p0 * a + p1 * b), the caller passing p0 = float(f), p1 = float(1 - f) (the difference formed in double).
 *   1 invert        v = 1 - v                                2 solarize     v >= p0 ? 1 - v : v
 *   3 autocontrast  per frame and channel lo / hi = min / max over h x w; hi == lo: unchanged; else clamp((v - lo) * (1 / (hi - lo)))
 *   4 grayscale     C = 3: all planes = gray                 5 normalize    (v - p[c]) / p[4 + c]
 *   6 brightness    blend(v, 0)                              7 contrast     blend(v, m), m = float(sum / (h w)) of gray (C = 3) or v (C = 1)
 *   8 saturation    C = 3: blend(v, gray); C = 1: identity      over the frame, the sum formed in fp64 in a fixed tree
 *   9 hue           C = 3: _rgb2hsv, h = (h + p0) mod 1, _hsv2rgb; C = 1: identity
 *  10 erase         rows [p0, p0 + p2) x columns [p1, p1 + p3), clipped to the frame, = p[4 + c]
 * One workgroup per (sample, frame) sweeps the frame 1 + (number of operations 3 and 7) times (once more, read only, when the program
 * begins with one). No workspace, no atomics: two runs give equal bits. 64-bit element offsets.
 * VPX_ERR_ARG: a NULL pointer, a size < 1, max_ops outside [16, 64]. VPX_ERR_UNSUPPORTED: C > 4, a side beyond 32768, B * n_frames
 * beyond one grid. `programs` lives on the device, so the CALLER checks it: a row the kernel cannot run (an unknown opcode; 4 without
 * three channels; 7, 8 or 9 with neither one nor three) ends the program there, and nothing is read or written outside the frames. */
#define VPX_FRAMES_AUG_ROW 9
int vpx_frames_augment(float* x, const float* programs, int B, int n_frames, int C, int h, int w, int max_ops, void* stream);

/* ---- frame adapter between a model and a test set (vp_suite/utils/compatibility.py: ScaleToModel / ScaleToTest, then TF.Resize) ----
 * x [N, C, H, W] planar fp32 (only read) -> out [N, C, oh, ow], one launch, no workspace, no atomics, 64-bit element offsets. Forward
 * only. Per element, each step one correctly rounded fp32 operation, never a fused multiply-add, scale first and resize second as in the
 * reference: only if (src_lo, src_hi) != (dst_lo, dst_hi): v = v - float(src_lo); v = v / float(src_hi - src_lo);
 * v = v * float(dst_hi - dst_lo); v = v + float(dst_lo) (the differences formed in double). Only if (oh, ow) != (H, W): the bilinear resize
 * of vpx_frames_preprocess over the scaled taps (align_corners = False, no antialiasing, the same fp32 source coordinates, horizontally
 * first; held to a bound, not to bits). Equal sizes: the affine map alone; equal ranges: no arithmetic on the taps; both: a copy.
 * VPX_ERR_ARG: a NULL pointer, a size < 1, src_hi == src_lo. VPX_ERR_UNSUPPORTED: a side beyond 32768, more workgroups than one launch holds. */
int vpx_frames_adapt(const float* x, long long N, int C, int H, int W, int oh, int ow, double src_lo, double src_hi, double dst_lo,
                     double dst_hi, float* out, void* stream);

/* ---- prediction visualizations: bordered tiles composed into a canvas (vp_suite/utils/visualization.py: add_borders, the side-by-side
 * video of save_vid_vis, the sheet of save_frame_compare_img) ----
 * src [S, T, C, h, w] planar fp32 (only read; C = 1 or 3) holds S sequences in the value range [lo, hi]; tiles [n_tiles, 8] (int32, on the
 * device) holds rows (s, t, f, y0, x0, b, colour 0xRRGGBB, 0); canvas [F, Hc, Wc, 3] is bytes. A tile paints the (h + 2b) x (w + 2b)
 * rectangle at (y0, x0) of canvas frame f: the outer ring of width b in the colour, the inner h x w with frame (s, t) turned into bytes by
 * the device function of vpx_frames_postprocess (the same bytes); a one-channel source goes to all three channels. Bytes that no tile covers
 * hold `background` (a grey level 0 ... 255: one asynchronous fill of the canvas before the launch), or are left as they are for
 * background = -1 (the caller knows that the tiles cover the canvas). max_border is the largest b of the table (it sizes the launch).
 * One launch over the tiles on the caller's stream, no workspace, no atomics, no host sync, 64-bit offsets: two runs give equal bytes.
 * VPX_ERR_ARG: a NULL pointer, C neither 1 nor 3, hi <= lo, n_tiles < 0, max_border < 0, background outside [-1, 255], with n_tiles > 0 a
 * size < 1. VPX_ERR_UNSUPPORTED: a side or border beyond 32768, more work than one launch holds. `tiles` lives on the device, so the CALLER
 * checks it: a row whose s, t or f is out of range, whose b is outside [0, max_border] or whose rectangle leaves the canvas is skipped as
 * a whole (nothing of it is read or written); two overlapping tiles of one canvas frame stay in bounds and show either. */
int vpx_vis_compose(const float* src, int S, int T, int C, int h, int w, double lo, double hi, const int* tiles, int n_tiles, int max_border,
                    unsigned char* canvas, int F, int Hc, int Wc, int background, void* stream);

/* ---- layout adaptors: src [N,C,H,W] <-> dst [N,H,W,C] -------------------------------------------------------- */
int vpx_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, void* stream);
int vpx_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPX_H_ */
