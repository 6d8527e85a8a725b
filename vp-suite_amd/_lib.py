"""ctypes binding of libvpx_hip.so (C ABI: include/vpx.h). No torch types cross the boundary: only raw device
pointers (tensor.data_ptr()), sizes and the current HIP stream handle.

There is NO CPU fallback: if the shared library is missing or fails to load, every op raises."""
import contextlib
import ctypes
import enum
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# VPX_LIB: developer override to A/B two builds of the library inside one GPU session (tools/ab_*); never a fallback
LIB_PATH = os.environ.get("VPX_LIB") or os.path.join(_HERE, "libvpx_hip.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

GATE_IFGO, GATE_IFOG = 0, 1
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1
PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 1
RCONV_REPLICATE, RCONV_COLLAPSE = 0, 1
RCONV_EPI_PLAIN, RCONV_EPI_EVAL, RCONV_EPI_STATS = 0, 1, 2
FLAG_SAVE_FOR_BWD = 1
FLAG_WEIGHTS_PACKED = 2
FLAG_X_SPLIT = 4
FLAG_OUT_SPLIT = 8
FRAMES_U8, FRAMES_U16, FRAMES_F32 = 0, 1, 2
ACTIONS_F32, ACTIONS_F64 = 0, 1
FRAMES_AUG_ROW, FRAMES_AUG_MIN_OPS, FRAMES_AUG_MAX_OPS = 9, 16, 64   # a program row: opcode + 8 parameters; rows per program
VIS_TILE_ROW = 8     # a visualization tile: (s, t, f, y0, x0, b, colour 0xRRGGBB, 0)

OPT_CELL2 = 1
OPT_CELL3 = 2
OPT_EXPERIMENT = 4
OPT_DRY_RUN = 5      # host-side work only, no HIP call (tests/test_workspace_contract.py)
OPT_SEQ_CHAINS = 6   # a ConvLSTM sequence forward on CELL2 / C3 runs the batch halves as two launch chains: 1 from B = 8 on, 2 from B = 2 on, 0 never
OPT_MFMA_SHAPE = 3   # 0: v_mfma_f32_32x32x16_bf16, 1: v_mfma_f32_16x16x32_bf16 in the second-generation kernels' main loop


class Exp(enum.IntFlag):
    """Values of OPT_EXPERIMENT: the VPX_EXP_* table of include/vpx.h, name for name (tests/test_host_logic.py holds the two together).
    Each bit switches one kernel form on in place of the product's; 0 is the product."""
    CELL2_FULL_TILE = 4
    CONVQ_FULL_TILE = 16
    HOIST_GEN1 = 32
    ST_WGRAD_GEN1 = 64
    ST_DGRAD_GEN1 = 128
    ST_FWD_GEN1 = 256
    C1_GEN1 = 512
    C5_UNSPLIT = 1024
    C5_NO_KSPLIT = 2048
    NO_C3 = 4096
    C3_NARROW = 8192
    GLUE_DGRAD_GEN1 = 16384
    CELL2X = 32768
    CELL2X_COLSPLIT = 65536
    ST_LAST_FP32 = 1 << 27
    NO_C16 = 1 << 28
    GLUE_WGRAD_TAPGROUP = 1 << 29
    # diagnostics inside cell2_kernel_q; PLACEMENT takes a distance in bits 8-19 (value | D << 8): never with a selection bit of that range
    CELL2_NO_STAGGER = 1
    CELL2_PLACEMENT = 8
    CELL2_DIAG_MASK = 1 | 8 | 0xfff << 8


class ConvLSTMDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "T", "Cin", "Ch", "H", "W", "kh", "kw", "gate_order", "layout",
                                              "precision", "flags")]


class STLSTMDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "Cin", "Ch", "H", "W", "k", "layer_norm", "layout", "precision",
                                              "flags")]


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "H", "W", "Ci", "Co", "kh", "kw", "stride", "pad", "transposed")] + \
               [("leaky_slope", ctypes.c_float), ("precision", ctypes.c_int32), ("out_pad_h", ctypes.c_int32),
                ("out_pad_w", ctypes.c_int32)]


class ACSTLSTMDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "Cin", "Ch", "H", "W", "k", "layer_norm", "precision", "flags")] + [("forget_bias", ctypes.c_float)]


class TrajGRUDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "T", "Cin", "C", "H", "W", "L", "k_i2h", "precision", "flags")] + [("slope", ctypes.c_float)]


class RConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "T", "H", "W", "Ca", "Cb", "Co", "kt", "mode")]


class STLSTMShadows(ctypes.Structure):
    """vpx_stlstm_shadows: split-format copies of (x, h, m, c_new, m_new) handed in, buffers for (h_new, c_new, m_new) handed out."""
    _fields_ = [("inp", ctypes.c_void_p * 5), ("out", ctypes.c_void_p * 3), ("dg8_out", ctypes.c_void_p)]


class STLSTMPlanInfo(ctypes.Structure):
    """vpx_stlstm_plan_info: the kernels a step with a descriptor takes (include/vpx.h), every field an int32."""
    _fields_ = ([(n, ctypes.c_int32) for n in ("route", "o_split", "nt_o", "ks_g", "ks_o", "mw_g", "mw_o", "ksplit_l", "last_c1", "stw", "c5")] +
                [("c5_ks", ctypes.c_int32 * 5), ("n_slices", ctypes.c_int32), ("stw_ns", ctypes.c_int32), ("dg_ksplit", ctypes.c_int32 * 5),
                 ("dg_mw", ctypes.c_int32 * 5)])


ST_ROUTE_LN, ST_ROUTE_GEN1, ST_ROUTE_C5, ST_ROUTE_C5K = 0, 1, 2, 3


class ConvLSTMPlanInfo(ctypes.Structure):
    """vpx_convlstm_plan_info: the kernels a sequence call with a descriptor takes (include/vpx.h), every field an int32."""
    _fields_ = [(n, ctypes.c_int32) for n in ("route", "qform", "c3nt", "mw", "ksplit", "hh_split", "hoist_convq", "cell2x", "dgrad", "dgrad_qform",
                                              "d_mw", "dgrad_cols", "wgrad", "n_slices", "dG_f32", "gate_slices")]


CL_ROUTE_FUSED, CL_ROUTE_KSPLIT, CL_ROUTE_HOIST, CL_ROUTE_CELL3, CL_ROUTE_CELL2, CL_ROUTE_C3 = range(6)


class DensePlanInfo(ctypes.Structure):
    """vpx_dense_plan_info: the launch a dense layer of (M, N, K) takes (include/vpx.h), every field an int32."""
    _fields_ = [(n, ctypes.c_int32) for n in ("split", "chunks", "chunk_len", "form", "tile_m", "tile_n", "m_tiles", "n_tiles")]


class VpxError(RuntimeError):
    pass


# ---- the C ABI, once: name -> (restype, argtypes), one entry per function of include/vpx.h, grouped and ordered as the header is.
#      tests/test_host_logic.py holds every entry's argument count against the header's prototype. ----
vp, sz, ci, ll, fl, dbl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
_clstm, _stlstm, _conv, _acst, _traj = (ctypes.POINTER(D) for D in (ConvLSTMDesc, STLSTMDesc, ConvDesc, ACSTLSTMDesc, TrajGRUDesc))
_rconv = ctypes.POINTER(RConvDesc)
_int_p = ctypes.POINTER(ci)
_ws = [vp, sz, vp]           # void* workspace, size_t workspace_bytes, void* stream
_rs_ws = [vp, sz] + _ws      # void* reserve, size_t reserve_bytes, then the workspace and the stream
_stlstm_fwd = [_stlstm] + [vp] * 4 + [vp] * 5 + [vp] + [vp] * 5 + _rs_ws                                  # x h c m | 5 weights | ln | 5 outputs
_stlstm_bwd = [_stlstm] + [vp] * 6 + [vp] * 5 + [vp] + [vp, sz] + [vp] * 5 + [vp] * 4 + [vp] * 5 + [vp] + _ws
#             x h c m c_new m_new | 5 weights | ln | reserve | 5 incoming gradients | dx dh dc dm | 5 weight gradients | dln

SIGNATURES = {
    "vpx_version": (ci, []),
    "vpx_last_error": (ctypes.c_char_p, []),
    "vpx_set_deterministic": (ci, [ci]),
    "vpx_set_option": (ci, [ci, ci]),
    "vpx_option_epoch": (ci, []),
    # ConvLSTM over a sequence
    "vpx_convlstm_workspace_bytes": (sz, [_clstm]),
    "vpx_convlstm_takes_split_input": (ci, [_clstm]),
    "vpx_convlstm_writes_split_output": (ci, [_clstm]),
    "vpx_convlstm_reserve_bytes": (sz, [_clstm]),
    "vpx_convlstm_seq_fwd": (ci, [_clstm] + [vp] * 8 + [vp] * 3 + _rs_ws),                     # x h0 c0 W bias Wci Wcf Wco | out hT cT
    "vpx_convlstm_seq_bwd": (ci, [_clstm] + [vp] * 8 + [vp, sz] + [vp] * 3 + [vp] * 8 + _ws),  # x h0 c0 W Wci Wcf Wco out | reserve | dout dhT dcT | 8 gradients
    "vpx_convlstm_plan": (ci, [_clstm, ci, ci, ci, vp]),
    "vpx_convlstm_seq_chains": (ci, [_clstm, ci, vp]),
    # ST-LSTM cell step
    "vpx_stlstm_workspace_bytes": (sz, [_stlstm]),
    "vpx_stlstm_reserve_bytes": (sz, [_stlstm]),
    "vpx_stlstm_uses_split": (ci, [_stlstm]),
    "vpx_stlstm_defers_wgrad": (ci, [_stlstm]),
    "vpx_stlstm_plan": (ci, [_stlstm, ci, vp]),
    "vpx_stlstm_wgrad_batch_workspace_bytes": (sz, [_stlstm]),
    "vpx_stlstm_wgrad_batch": (ci, [_stlstm, vp, vp] + [vp] * 5 + _ws),
    "vpx_stlstm_step_fwd": (ci, _stlstm_fwd),
    "vpx_stlstm_step_bwd": (ci, _stlstm_bwd),
    "vpx_stlstm_step_fwd_ex": (ci, _stlstm_fwd + [ctypes.POINTER(STLSTMShadows)]),
    "vpx_stlstm_step_bwd_ex": (ci, _stlstm_bwd + [ctypes.POINTER(STLSTMShadows)]),
    # decoupling-loss term
    "vpx_decouple_workspace_bytes": (sz, [ci] * 4),
    "vpx_decouple_fwd": (ci, [vp] * 4 + [ci] * 5 + _ws),
    "vpx_decouple_bwd": (ci, [vp] * 7 + [ci] * 5 + _ws),
    # training tail
    "vpx_mse_loss_workspace_bytes": (sz, []),
    "vpx_mse_loss": (ci, [vp, vp, ll, ll, fl, vp, vp] + _ws),
    "vpx_adam_step": (ci, [vp] * 4 + [ll] + [dbl] * 5 + [ci, dbl, vp]),
    "vpx_grad_stats_workspace_bytes": (sz, []),
    "vpx_grad_stats": (ci, [vp, ll, dbl, vp] + _ws),
    "vpx_adam_step_clipped": (ci, [vp] * 4 + [ll] + [dbl] * 5 + [ci, dbl, vp, dbl, dbl, ci, vp]),   # ... step grad_scale | stats max_norm clip_value skip_nonfinite
    # image-wise measures
    "vpx_pixel_measures_workspace_bytes": (sz, [ll, ll]),
    "vpx_pixel_measures_fwd": (ci, [vp, vp, ll, ll, vp] + _ws),
    "vpx_pixel_measures_bwd": (ci, [vp, vp, vp, ll, ll, vp, vp]),
    "vpx_ssim_workspace_bytes": (sz, [ll, ci, ci]),
    "vpx_ssim_fwd": (ci, [vp, vp, ll] + [ci] * 4 + [vp] + _ws),
    "vpx_ssim_bwd": (ci, [vp, vp, vp, ll] + [ci] * 4 + [vp, vp]),
    "vpx_lpips_workspace_bytes": (sz, [ll, ci, ci]),
    "vpx_lpips_fwd": (ci, [vp, vp, ll] + [ci] * 3 + [vp, vp] + _ws),                                  # pred target n C H W | params table
    "vpx_lpips_stem_workspace_bytes": (sz, []),
    "vpx_lpips_stem_fwd": (ci, [vp, vp, ll, ll, ci, ci, vp, vp, vp] + _ws),                           # x0 x1 n0 n1 H W | w bias y
    "vpx_lpips_maxpool_fwd": (ci, [vp, vp, ll] + [ci] * 3 + [vp]),
    "vpx_lpips_head_workspace_bytes": (sz, [ll, ll]),
    "vpx_lpips_head_fwd": (ci, [vp, vp, vp, ll, ll, ci, vp] + _ws),                                   # fx fy w n HW C | table
    "vpx_lpips_reserve_bytes": (sz, [ll, ci, ci]),
    "vpx_lpips_fwd_train": (ci, [vp, vp, ll] + [ci] * 3 + [vp, vp, vp, sz] + _ws),                    # pred target n C H W | params table reserve
    "vpx_lpips_bwd_workspace_bytes": (sz, [ll, ci, ci]),
    "vpx_lpips_bwd": (ci, [vp, vp, vp, vp, ll] + [ci] * 3 + [vp] + _ws),                              # pred params reserve dtable n C H W | dpred
    "vpx_lpips_head_bwd": (ci, [vp, vp, vp, vp, vp, ll, ll, ci, vp, vp]),                             # fx fy w dtable incoming n HW C | dz
    "vpx_lpips_maxpool_bwd": (ci, [vp, vp, vp, ll] + [ci] * 3 + [vp]),
    "vpx_lpips_stem_bwd": (ci, [vp, vp, vp, ll, ci, ci, vp] + _ws),                                   # x w dz n H W | dx
    # Frechet Video Distance on an I3D trunk
    "vpx_same_padding": (ci, [ci, ci, ci, _int_p, _int_p]),
    "vpx_conv3d_same_workspace_bytes": (sz, []),
    "vpx_conv3d_same": (ci, [vp] * 4 + [ll] + [ci] * 14 + [vp]),                                      # x wp bias y | N T H W Ci Co | kernel stride | relu ldy coff
    "vpx_maxpool3d_same_workspace_bytes": (sz, []),
    "vpx_maxpool3d_same": (ci, [vp, vp, ll] + [ci] * 10 + [vp]),                                      # x y | N T H W C | kernel stride
    "vpx_fvd_head_workspace_bytes": (sz, []),
    "vpx_fvd_head": (ci, [vp] * 4 + [ll] + [ci] * 5 + [vp]),                                          # x w bias out | N T H W C n_features
    "vpx_fvd_features_workspace_bytes": (sz, [ll] + [ci] * 4 + [_int_p, ci]),                         # n_clips T C h w | table n_rows
    "vpx_fvd_features": (ci, [vp, vp, ll, ll] + [ci] * 4 + [_int_p, ci, vp, ci, vp] + _ws),           # x0 x1 n0 n1 T C h w | table n_rows params n_params | out
    "vpx_frechet_distance_workspace_bytes": (sz, [ci, ci]),
    "vpx_frechet_distance": (ci, [vp, vp, ci, ci, vp] + _ws),                                         # pred target b n | out
    # plain stride-1 "same" convolution
    "vpx_conv2d_workspace_bytes": (sz, [ci] * 4),
    "vpx_conv2d_nhwc_fwd": (ci, [vp] * 4 + [ci] * 8 + _ws),
    "vpx_conv2d_bwd_workspace_bytes": (sz, [ci] * 7),
    "vpx_conv2d_nhwc_bwd": (ci, [vp] * 6 + [ci] * 8 + _ws),
    # general convolution / transposed convolution + bias + LeakyReLU (stage glue)
    "vpx_conv2d_ex_out_shape": (ci, [_conv, _int_p, _int_p]),
    "vpx_conv2d_ex_workspace_bytes": (sz, [_conv]),
    "vpx_conv2d_ex_fwd": (ci, [_conv] + [vp] * 4 + _ws),
    "vpx_conv2d_ex_fwd_split": (ci, [_conv] + [vp] * 5 + _ws),
    "vpx_conv2d_ex_takes_split": (ci, [_conv]),
    "vpx_split_convert": (ci, [vp, vp, ll, ci, vp]),
    "vpx_conv2d_ex_split_workspace_bytes": (sz, [_conv]),
    "vpx_conv2d_ex_fwd_from_split": (ci, [_conv, vp, ll, ll, ci, vp, vp, vp, vp, ci] + _ws),
    "vpx_conv2d_ex_bwd_workspace_bytes": (sz, [_conv]),
    "vpx_conv2d_ex_bwd": (ci, [_conv] + [vp] * 7 + _ws),
    "vpx_conv2d_ex_bwd_uses_split": (ci, [_conv]),
    "vpx_conv2d_ex_bwd_ex": (ci, [_conv] + [vp] * 8 + _ws),
    "vpx_conv2d_nhwc_fwd_ex": (ci, [vp] * 4 + [ci] * 9 + [fl] + _ws),
    # TrajGRU over a sequence
    "vpx_trajgru_workspace_bytes": (sz, [_traj]),
    "vpx_trajgru_reserve_bytes": (sz, [_traj]),
    "vpx_trajgru_seq_fwd": (ci, [_traj, vp, vp, vp, vp] + _rs_ws),
    "vpx_trajgru_seq_bwd": (ci, [_traj, vp, vp, vp, vp, vp, sz] + [vp] * 5 + _ws),
    # action-conditional ST-LSTM cell step
    "vpx_acstlstm_workspace_bytes": (sz, [_acst]),
    "vpx_acstlstm_reserve_bytes": (sz, [_acst]),
    "vpx_acstlstm_step_fwd": (ci, [_acst] + [vp] * 5 + [vp, vp] + [vp] * 5 + _rs_ws),                              # x h c m a | params ln | 5 outputs
    "vpx_acstlstm_step_bwd": (ci, [_acst] + [vp] * 5 + [vp, vp] + [vp, sz] + [vp] * 5 + [vp] * 5 + [vp, vp] + _ws),  # ... | reserve | 5 incoming | dx dh dc dm da | dparams dln
    # LayerNorm([C,H,W])
    "vpx_layernorm_workspace_bytes": (sz, [ci]),
    "vpx_layernorm_fwd": (ci, [vp] * 6 + [ci, ll] + _ws),
    "vpx_layernorm_bwd": (ci, [vp] * 7 + [ci, ci, ci] + _ws),
    # GroupNorm
    "vpx_groupnorm_fwd": (ci, [vp] * 6 + [ci] * 5 + [fl, vp]),
    "vpx_groupnorm_bwd_workspace_bytes": (sz, [ci, ci]),
    "vpx_groupnorm_bwd": (ci, [vp] * 8 + [ci] * 5 + [fl] + _ws),
    # PhyDNet
    "vpx_phycell_correct_fwd": (ci, [vp] * 5 + [ll, vp]),
    "vpx_phycell_correct_bwd": (ci, [vp] * 9 + [ll, vp]),
    "vpx_moment_loss_fwd": (ci, [vp, vp] + [ci] * 4 + [fl, vp]),
    "vpx_moment_loss_bwd": (ci, [vp, vp, vp] + [ci] * 4 + [fl, vp]),
    "vpx_sigmoid_head_fwd": (ci, [vp, vp] + [ci] * 7 + [vp]),
    "vpx_sigmoid_head_bwd": (ci, [vp, vp, vp] + [ci] * 7 + [vp]),
    # ST-Phy
    "vpx_conv2d_act_workspace_bytes": (sz, [_conv, ci]),
    "vpx_conv2d_act_fwd": (ci, [_conv, ci] + [vp] * 4 + _ws),
    "vpx_conv2d_act_bwd_workspace_bytes": (sz, [_conv, ci]),
    "vpx_conv2d_act_bwd": (ci, [_conv, ci] + [vp] * 7 + _ws),
    "vpx_relu_rownorm_fwd": (ci, [vp] * 3 + [ci] * 4 + [fl, vp]),
    "vpx_relu_rownorm_bwd": (ci, [vp] * 4 + [ci] * 4 + [fl, vp]),
    "vpx_merge1x1_workspace_bytes": (sz, [ci] * 3),
    "vpx_merge1x1_fwd": (ci, [vp] * 5 + [ci] * 7 + _ws),
    "vpx_merge1x1_bwd_workspace_bytes": (sz, [ci] * 6),
    "vpx_merge1x1_bwd": (ci, [vp] * 8 + [ci] * 7 + _ws),
    # UNet-3D
    "vpx_rconv_workspace_bytes": (sz, [_rconv, ci]),
    "vpx_rconv_fwd": (ci, [_rconv, ci] + [vp] * 7 + [fl, fl] + [vp, vp] + _ws),      # a b w gamma|bias beta rmean rvar | eps momentum | y stats
    "vpx_rconv_bwd_workspace_bytes": (sz, [_rconv]),
    "vpx_rconv_bwd": (ci, [_rconv] + [vp] * 8 + _ws),                                # a b w dy | da db dw dbias
    "vpx_bn_relu_fwd": (ci, [vp] * 6 + [ll, ci, ci, ci, vp]),
    "vpx_bn_relu_bwd_workspace_bytes": (sz, [ll, ci, ci, ci]),
    "vpx_bn_relu_bwd": (ci, [vp] * 9 + [ll, ci, ci, ci] + _ws),
    # NonConvLSTM: dense layer, LSTM cell, replicate padding, differentiable resize
    "vpx_dense_plan": (ci, [ll, ll, ll, vp]),
    "vpx_dense_workspace_bytes": (sz, [ll, ll, ll]),
    "vpx_dense_fwd": (ci, [vp, ll, vp, vp, vp, ll] + [ll] * 3 + [ci] + _ws),                          # x ldx w bias y ldy | M N K | relu
    "vpx_dense_bwd": (ci, [vp, ll, vp, vp, ll, vp, ll, vp, ll, vp, vp] + [ll] * 3 + [ci, ci] + _ws),  # x ldx w y ldy dy lddy dx lddx dw db | M N K | relu accumulate
    "vpx_lstm_cell_workspace_bytes": (sz, [ll, ll, ll]),
    "vpx_lstm_cell_fwd": (ci, [vp, ll] + [vp] * 6 + [vp] * 3 + [ll] * 3 + _ws),                       # x ldx h c w_ih w_hh b_ih b_hh | h_new c_new gates | M Kx H
    "vpx_lstm_cell_bwd": (ci, [vp, ll] + [vp] * 5 + [vp, vp] + [vp] * 8 + [ll] * 3 + [ci] + _ws),     # x ldx h c w_ih w_hh gates | dh_new dc_new | dx dh dc dw_ih dw_hh db_ih db_hh dgates | M Kx H | accumulate
    "vpx_replicate_pad_fwd": (ci, [vp, vp, ll] + [ci] * 4 + [vp]),
    "vpx_replicate_pad_bwd": (ci, [vp, vp, ll] + [ci] * 4 + [vp]),
    "vpx_resize_bilinear_fwd": (ci, [vp, vp, ll] + [ci] * 5 + [vp]),
    "vpx_resize_bilinear_bwd": (ci, [vp, vp, ll] + [ci] * 5 + [vp]),
    # Moving MNIST generated on the device
    "vpx_mmnist_frames": (ci, [vp, ci, ci, vp] + [ci] * 5 + [dbl, dbl, vp, vp]),     # digits N s | params B D F C S | lo hi | out
    # stored frames to a model-ready batch and back
    "vpx_frames_preprocess": (ci, [vp, ci, ll] + [ci] * 4 + [vp] + [ci] * 8 + [dbl, dbl, vp, vp]),   # src dtype N T' H W Cs | table B F step ch cw oh ow C_out | lo hi | out
    "vpx_clips_preprocess": (ci, [vp, ci, ll] + [ci] * 3 + [vp, ll, vp] + [ci] * 8 + [dbl, dbl, vp, vp]),  # src dtype frames H W Cs | clip_first n_clips table B F step ch cw oh ow C_out | lo hi | out
    "vpx_clips_preprocess_var": (ci, [vp, ci, ll, ci, vp, ll, vp] + [ci] * 6 + [dbl, dbl, vp, vp]),   # src dtype elems Cs | clip_geom n_clips table B F step oh ow C_out | lo hi | out
    "vpx_frames_postprocess": (ci, [vp, ll] + [ci] * 3 + [dbl, dbl, vp, vp]),                       # x N C h w | lo hi | out
    "vpx_actions_gather": (ci, [vp, ci, ll, ci, ci, vp] + [ci] * 3 + [vp, vp]),                     # src dtype N T' A | table B F step | out
    "vpx_actions_diff_gather": (ci, [vp, ci, ll, ci, vp, ll, vp] + [ci] * 3 + [vp, vp]),           # src dtype frames A | clip_first n_clips table B F step | out
    "vpx_frames_augment": (ci, [vp, vp] + [ci] * 6 + [vp]),                                           # x programs | B F C h w max_ops
    # frame adapter between a model and a test set
    "vpx_frames_adapt": (ci, [vp, ll] + [ci] * 5 + [dbl] * 4 + [vp, vp]),                            # x N C H W oh ow | src lo hi, dst lo hi | out
    # prediction visualizations
    "vpx_vis_compose": (ci, [vp] + [ci] * 5 + [dbl, dbl, vp, ci, ci, vp] + [ci] * 4 + [vp]),          # src S T C h w | lo hi | tiles n_tiles max_border | canvas F Hc Wc background
    # layout adaptors
    "vpx_nchw_to_nhwc": (ci, [vp, vp] + [ci] * 4 + [vp]),
    "vpx_nhwc_to_nchw": (ci, [vp, vp] + [ci] * 4 + [vp]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)

_lib = None


def build(force: bool = False, jobs: int = 4) -> str:
    """Compiles every HIP source under csrc/ for gfx950 into vp-suite_amd/libvpx_hip.so (hipcc cross-compiles
    without a GPU). No-op when the library is newer than all sources."""
    srcs = [os.path.join(CSRC_DIR, f) for f in os.listdir(CSRC_DIR) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "vpx.h"))
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", CSRC_DIR, "-s", f"-j{jobs}"] + (["-B"] if force else []))
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VpxError(f"HIP extension not built: {LIB_PATH} is missing (run `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` or `make -C {CSRC_DIR}`). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


@contextlib.contextmanager
def option(opt: int, value: int):
    """vpx_set_option(opt, value) for a block; the previous value comes back on the way out, exception or not."""
    prev = lib().vpx_set_option(opt, int(value))
    try:
        yield prev
    finally:
        lib().vpx_set_option(opt, prev)


def experiment(bits: int):
    """option(OPT_EXPERIMENT, bits): an OR of Exp members (0 = the product's kernels)."""
    return option(OPT_EXPERIMENT, bits)


def exp_bits(text: str) -> int:
    """An OPT_EXPERIMENT value as the tools take it from the command line: Exp names and / or numbers joined by '|'
    ("0", "CELL2X|CELL2X_COLSPLIT", "4096")."""
    bits = 0
    for t in text.split("|"):
        bits |= Exp[t.strip()] if t.strip() in Exp.__members__ else int(t, 0)
    return int(bits)


def convlstm_plan(d: ConvLSTMDesc, x_present=True, want_dx=True, want_dW=True) -> dict:
    """vpx_convlstm_plan as a dict (field -> int) under the current options; raises as check() does where the query refuses."""
    info = ConvLSTMPlanInfo()
    check(lib().vpx_convlstm_plan(ctypes.byref(d), int(bool(x_present)), int(bool(want_dx)), int(bool(want_dW)), ctypes.byref(info)), "vpx_convlstm_plan")
    return {n: getattr(info, n) for n, _ in ConvLSTMPlanInfo._fields_}


def check(rc: int, what: str):
    """Maps library error codes to the exception types the reference raises for the same misuse
    (ValueError for shape/argument problems, e.g. predrnn_v2.py:136-137; NotImplementedError conv_lstm_ndrplz.py:100)."""
    if rc == 0:
        return
    msg = lib().vpx_last_error().decode(errors="replace")
    if rc == -1:
        raise ValueError(f"{what}: {msg}")
    if rc == -4:
        raise NotImplementedError(f"{what}: {msg}")
    raise VpxError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a torch tensor or None."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptr_array(tensors):
    """C array of the device pointers of `tensors` (NULL for None): the `const float* const*` arguments."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
