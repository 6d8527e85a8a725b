"""ST-Phy's operators over the C ABI (include/vpx.h): a convolution layer with an activation code (ReLU in the epilogue of the launch
that runs the layer), the encoder tail relu + L2 row normalisation, and the two-source 1x1 merge; one autograd Function each,
forward and backward in libvpx_hip (csrc/glue_fwd_api.hip, csrc/glue_bwd_api.hip, csrc/stphy.hip).

As in phy_ops: activations keep the reference's logical shapes ([N,C,H,W]) and live channels-last in memory; whether a Function keeps
its backward state is decided in the wrapper, where grad mode is visible; shapes are checked here, before any launch. CPU tensors
raise VpxError: there is no fallback."""
import ctypes

import torch

from . import _lib
from ._lib import check, ptr
from .ops import (NOT_IMPLEMENTED, PRECISIONS, conv_desc, conv_out_shape, needs_grad, new_channels_last, require_gpu, stream, sync_determinism,
                  to_channels_last, workspace)

ACTIVATIONS = {None: _lib.ACT_NONE, "none": _lib.ACT_NONE, "relu": _lib.ACT_RELU}


# ---- convolution / transposed convolution + bias + activation ---------------------------------------------------------------------
class _ConvActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, d, act, need_grad):
        xs = to_channels_last(x)
        wc = w.contiguous()
        bc = None if bias is None else bias.contiguous()
        L = _lib.lib()
        y = new_channels_last((d.N, d.Co, *conv_out_shape(d)), x.device)
        ws, ws_bytes = workspace(x.device, L.vpx_conv2d_act_workspace_bytes, ctypes.byref(d), act)
        check(L.vpx_conv2d_act_fwd(ctypes.byref(d), act, ptr(xs), ptr(wc), ptr(bc), ptr(y), ptr(ws), ws_bytes, stream()), "vpx_conv2d_act_fwd")
        if need_grad:   # the output is kept only where the backward reads ReLU' off it
            ctx.save_for_backward(xs, wc, *([y] if act != _lib.ACT_NONE else []))
            ctx.cfg = (d, act, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        xs, wc, *ys = ctx.saved_tensors
        y = ys[0] if ys else None
        d, act, has_bias = ctx.cfg
        L = _lib.lib()
        dys = to_channels_last(dy)
        ws, ws_bytes = workspace(dy.device, L.vpx_conv2d_act_bwd_workspace_bytes, ctypes.byref(d), act, unsupported=NOT_IMPLEMENTED)
        dx = new_channels_last(tuple(xs.shape), dy.device) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(wc) if ctx.needs_input_grad[1] else None
        db = torch.empty(d.Co, device=dy.device) if (has_bias and ctx.needs_input_grad[2]) else None
        check(L.vpx_conv2d_act_bwd(ctypes.byref(d), act, ptr(xs), ptr(wc), ptr(y), ptr(dys), ptr(dx), ptr(dw), ptr(db), ptr(ws), ws_bytes,
                                   stream()), "vpx_conv2d_act_bwd")
        return dx, dw, db, None, None, None


def conv2d_act(x, w, bias, stride, padding, transposed=False, act="relu", precision="f32"):
    """act(Conv2d / ConvTranspose2d(x; w, bias)) with stride 1 or 2 and one padding for both axes; act = "relu" | None. x: [N,C,H,W]
    fp32 on the GPU, w in the reference's parameter layout. Differentiable; ReLU' is read off the saved output (zero at 0)."""
    for t in (x, w, bias):
        if t is not None:
            require_gpu(t, "conv2d_act")
    if act not in ACTIVATIONS:
        raise ValueError(f"conv2d_act: unknown activation {act!r} (one of {sorted(k for k in ACTIVATIONS if k)} or None)")
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(f"conv2d_act: expected a [N,C,H,W] input and a 4-d weight, got {tuple(x.shape)} and {tuple(w.shape)}")
    d = conv_desc(x.shape, w.shape, stride, padding, transposed, 0.0, PRECISIONS[precision])
    Ci, Co, kh, kw = d.Ci, d.Co, d.kh, d.kw
    if int(w.shape[0] if transposed else w.shape[1]) != Ci:
        raise ValueError(f"conv2d_act: weight {tuple(w.shape)} does not match {Ci} input channels")
    if bias is not None and tuple(bias.shape) != (Co,):
        raise ValueError(f"conv2d_act: bias {tuple(bias.shape)} does not match {Co} output channels")
    need_grad = needs_grad(x, w, bias)
    if need_grad and (kh < stride or kw < stride):
        raise _lib.VpxError(f"conv2d_act: a {kh}x{kw} kernel with stride {stride} has no backward in the library")
    return _ConvActFn.apply(x, w, bias, d, ACTIVATIONS[act], need_grad)


# ---- encoder tail: relu + L2 normalisation of every image row ------------------------------------------------------------------------
class _ReluRownormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, need_grad):
        xs = to_channels_last(x)
        N, C, H, W = (int(s) for s in xs.shape)
        y = new_channels_last((N, C, H, W), x.device)
        norm = torch.empty(N * H * C, device=x.device) if need_grad else None
        check(_lib.lib().vpx_relu_rownorm_fwd(ptr(xs), ptr(y), ptr(norm), N, H, W, C, float(eps), stream()), "vpx_relu_rownorm_fwd")
        if need_grad:
            ctx.save_for_backward(xs, norm)
            ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, norm = ctx.saved_tensors
        N, C, H, W = (int(s) for s in xs.shape)
        dys = to_channels_last(dy)
        dx = new_channels_last((N, C, H, W), dy.device)
        check(_lib.lib().vpx_relu_rownorm_bwd(ptr(xs), ptr(norm), ptr(dys), ptr(dx), N, H, W, C, ctx.eps, stream()), "vpx_relu_rownorm_bwd")
        return dx, None, None


def relu_rownorm(x, eps=1e-8):
    """F.normalize(relu(x), p=2, dim=-1, eps): every image row (along W, per sample, channel and row) of relu(x) divided by
    max(its L2 norm, eps). x: [N,C,H,W] fp32 on the GPU."""
    require_gpu(x, "relu_rownorm")
    if x.dim() != 4:
        raise ValueError(f"relu_rownorm: expected a [N,C,H,W] tensor, got shape {tuple(x.shape)}")
    if not eps > 0.0:
        raise ValueError("relu_rownorm: eps must be positive")
    return _ReluRownormFn.apply(x, float(eps), needs_grad(x))


# ---- merge: a biased 1x1 convolution over two sources ------------------------------------------------------------------------------
class _Merge1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, w, bias, precision, need_grad):
        As, Bs = to_channels_last(a), to_channels_last(b)
        N, Cs, H, W = (int(s) for s in As.shape)
        Cp, Co = int(Bs.shape[1]), int(w.shape[0])
        wc = w.contiguous()
        bc = None if bias is None else bias.contiguous()
        L = _lib.lib()
        y = new_channels_last((N, Co, H, W), a.device)
        ws, ws_bytes = workspace(a.device, L.vpx_merge1x1_workspace_bytes, Cs, Cp, Co)
        check(L.vpx_merge1x1_fwd(ptr(As), ptr(Bs), ptr(wc), ptr(bc), ptr(y), N, H, W, Cs, Cp, Co, precision, ptr(ws), ws_bytes, stream()),
              "vpx_merge1x1_fwd")
        if need_grad:
            ctx.save_for_backward(As, Bs, wc)
            ctx.cfg = (precision, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        As, Bs, wc = ctx.saved_tensors
        precision, has_bias = ctx.cfg
        N, Cs, H, W = (int(s) for s in As.shape)
        Cp, Co = int(Bs.shape[1]), int(wc.shape[0])
        L = _lib.lib()
        dys = to_channels_last(dy)
        needs = ctx.needs_input_grad
        da = new_channels_last(tuple(As.shape), dy.device) if needs[0] else None
        db = new_channels_last(tuple(Bs.shape), dy.device) if needs[1] else None
        dw = torch.empty_like(wc) if needs[2] else None
        dbias = torch.empty(Co, device=dy.device) if (has_bias and needs[3]) else None
        ws, ws_bytes = workspace(dy.device, L.vpx_merge1x1_bwd_workspace_bytes, N, H, W, Cs, Cp, Co)
        check(L.vpx_merge1x1_bwd(ptr(As), ptr(Bs), ptr(wc), ptr(dys), ptr(da), ptr(db), ptr(dw), ptr(dbias), N, H, W, Cs, Cp, Co, precision,
                                 ptr(ws), ws_bytes, stream()), "vpx_merge1x1_bwd")
        return da, db, dw, dbias, None, None


def merge1x1(a, b, w, bias=None, precision="f32"):
    """conv2d(cat([a, b], dim=1), w, bias) for a 1x1 weight [Co, Ca+Cb, 1, 1] without the concatenated copy. a, b: [N,C,H,W] fp32 on
    the GPU with equal N, H, W. precision "f32" | "bf16x3"."""
    for t in (a, b, w, bias):
        if t is not None:
            require_gpu(t, "merge1x1")
    if precision not in ("f32", "bf16x3"):
        raise ValueError(f"merge1x1: precision must be 'f32' or 'bf16x3', got {precision!r}")
    if a.dim() != 4 or b.dim() != 4 or a.shape[0] != b.shape[0] or tuple(a.shape[2:]) != tuple(b.shape[2:]):
        raise ValueError(f"merge1x1: sources {tuple(a.shape)} and {tuple(b.shape)} must be [N,C,H,W] tensors of one batch and map size")
    if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1) or int(w.shape[1]) != int(a.shape[1]) + int(b.shape[1]):
        raise ValueError(f"merge1x1: weight {tuple(w.shape)} is not a 1x1 kernel over {int(a.shape[1])}+{int(b.shape[1])} channels")
    if bias is not None and tuple(bias.shape) != (int(w.shape[0]),):
        raise ValueError(f"merge1x1: bias {tuple(bias.shape)} does not match {int(w.shape[0])} output channels")
    return _Merge1x1Fn.apply(a, b, w, bias, PRECISIONS[precision], needs_grad(a, b, w, bias))
