"""UNet-3D's operators over the C ABI (include/vpx.h, csrc/unet3d.hip): the replicate-border convolution (one or two channel-concatenated
sources; plain, eval and training epilogue), the time collapse, and BatchNorm + ReLU (+ 2x2 max-pool) with batch statistics; one
autograd Function each, forward and backward in libvpx_hip.

Unlike the other op modules, activations here are handed around in their MEMORY shape, channels-last per frame: [B, T, H, W, C]
contiguous (a 2-D layer is T = 1). Weights are the reference's parameters ([Co, Ci, 3, 3, 3], [Co, Ci, 3, 3], [Co, Ci, T, 1, 1]). As in
stphy_ops: whether a Function keeps its backward state is decided in the wrapper, where grad mode is visible; shapes are checked here,
before any launch; CPU tensors raise VpxError: there is no fallback."""
import ctypes

import torch

from . import _lib
from ._lib import RConvDesc, check, ptr
from .ops import needs_grad, require_gpu, stream, sync_determinism, workspace

BN_EPS = 1e-5        # nn.BatchNorm's default, the only value the model uses
BN_MOMENTUM = 0.1


def _frames(t, what):
    if t.dim() != 5 or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous [B,T,H,W,C] tensor, got shape {tuple(t.shape)} with strides {t.stride()}")


def _desc(a, b, w, mode, what):
    """RConvDesc of a layer with weight `w` on source(s) a (, b); every shape check of the convolution entry points."""
    for t in (a, b, w):
        if t is not None:
            require_gpu(t, what)
    _frames(a, what)
    B, T, H, W, Ca = (int(s) for s in a.shape)
    Cb = 0
    if b is not None:
        _frames(b, what)
        if tuple(b.shape[:4]) != (B, T, H, W):
            raise ValueError(f"{what}: sources {tuple(a.shape)} and {tuple(b.shape)} differ in more than their channels")
        Cb = int(b.shape[4])
    ws = tuple(int(s) for s in w.shape)
    if len(ws) == 4:
        ws = ws[:2] + (1,) + ws[2:]
    if len(ws) != 5 or ws[1] != Ca + Cb:
        raise ValueError(f"{what}: weight {tuple(w.shape)} does not span {Ca}+{Cb} input channels")
    if mode == _lib.RCONV_REPLICATE:
        if ws[3:] != (3, 3) or ws[2] not in (1, 3):
            raise ValueError(f"{what}: a replicate-border layer is 3x3 in space with 1 or 3 taps in time, got a weight of shape {tuple(w.shape)}")
    elif ws[2:] != (T, 1, 1):
        raise ValueError(f"{what}: the time collapse of {T} frames needs a [Co,Ci,{T},1,1] weight, got {tuple(w.shape)}")
    return RConvDesc(B, T, H, W, Ca, Cb, ws[0], ws[2], mode)


def _out(d, dev):
    return torch.empty(d.B, 1 if d.mode == _lib.RCONV_COLLAPSE else d.T, d.H, d.W, d.Co, device=dev)


def _rconv_backward(ctx, dy):
    sync_determinism()
    a, b, wc = ctx.saved_tensors if ctx.two else (*ctx.saved_tensors[:1], None, ctx.saved_tensors[1])
    d, has_bias = ctx.cfg
    L = _lib.lib()
    dyc = dy.contiguous()
    needs = ctx.needs_input_grad
    da = torch.empty_like(a) if needs[0] else None
    db = torch.empty_like(b) if (b is not None and needs[1]) else None
    dw = torch.empty_like(wc) if needs[2] else None
    dbias = torch.empty(d.Co, device=dy.device) if (has_bias and needs[3]) else None
    ws, ws_bytes = workspace(dy.device, L.vpx_rconv_bwd_workspace_bytes, ctypes.byref(d))
    check(L.vpx_rconv_bwd(ctypes.byref(d), ptr(a), ptr(b), ptr(wc), ptr(dyc), ptr(da), ptr(db), ptr(dw), ptr(dbias), ptr(ws), ws_bytes, stream()),
          "vpx_rconv_bwd")
    return da, db, dw, dbias


def _save(ctx, a, b, wc, d, has_bias):
    ctx.two = b is not None
    ctx.save_for_backward(*([a, b, wc] if b is not None else [a, wc]))
    ctx.cfg = (d, has_bias)


# ---- convolution, plain epilogue (+ bias): the time collapse, and the replicate-border layer on its own -------------------------------
class _RConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, w, bias, d, need_grad):
        wc = w.contiguous()
        bc = None if bias is None else bias.contiguous()
        L = _lib.lib()
        y = _out(d, a.device)
        ws, ws_bytes = workspace(a.device, L.vpx_rconv_workspace_bytes, ctypes.byref(d), _lib.RCONV_EPI_PLAIN)
        check(L.vpx_rconv_fwd(ctypes.byref(d), _lib.RCONV_EPI_PLAIN, ptr(a), ptr(b), ptr(wc), ptr(bc), None, None, None, 0.0, 0.0, ptr(y), None,
                              ptr(ws), ws_bytes, stream()), "vpx_rconv_fwd")
        if need_grad:
            _save(ctx, a, b, wc, d, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        return (*_rconv_backward(ctx, dy), None, None)


def replicate_conv(a, w, b=None):
    """conv(cat([a, b], channels); w) with padding 1, padding_mode 'replicate', no bias: w [Co,Ci,3,3] or [Co,Ci,{1,3},3,3] on
    [B,T,H,W,C] sources (b optional; the concatenation is never materialised). Differentiable in a, b and w."""
    d = _desc(a, b, w, _lib.RCONV_REPLICATE, "replicate_conv")
    return _RConvFn.apply(a, b, w, None, d, needs_grad(a, b, w))


def time_collapse(x, w, bias=None):
    """Conv3d(C -> Co, (T,1,1)) + bias + squeeze of the time axis: x [B,T,H,W,C], w [Co,C,T,1,1] -> [B,1,H,W,Co]."""
    d = _desc(x, None, w, _lib.RCONV_COLLAPSE, "time_collapse")
    if bias is not None:
        require_gpu(bias, "time_collapse")
        if tuple(bias.shape) != (d.Co,):
            raise ValueError(f"time_collapse: bias {tuple(bias.shape)} does not match {d.Co} output channels")
    return _RConvFn.apply(x, None, w, bias, d, needs_grad(x, w, bias))


# ---- convolution with the training epilogue: raw output + batch statistics (and the running-statistics update) --------------------------
class _RConvStatsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, w, d, running_mean, running_var, need_grad):
        wc = w.contiguous()
        L = _lib.lib()
        y = _out(d, a.device)
        stats = torch.empty(2, d.Co, device=a.device)
        ws, ws_bytes = workspace(a.device, L.vpx_rconv_workspace_bytes, ctypes.byref(d), _lib.RCONV_EPI_STATS)
        check(L.vpx_rconv_fwd(ctypes.byref(d), _lib.RCONV_EPI_STATS, ptr(a), ptr(b), ptr(wc), None, None, ptr(running_mean), ptr(running_var),
                              BN_EPS, BN_MOMENTUM, ptr(y), ptr(stats), ptr(ws), ws_bytes, stream()), "vpx_rconv_fwd")
        if need_grad:
            _save(ctx, a, b, wc, d, False)
        ctx.mark_non_differentiable(stats)   # (the BatchNorm backward carries the statistics' dependence on y itself)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        return (*_rconv_backward(ctx, dy)[:3], None, None, None, None)


class _BnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stats, gamma, beta, pool, need_grad):
        B, T, H, W, C = (int(s) for s in x.shape)
        gc, bc = gamma.contiguous(), beta.contiguous()
        act = torch.empty_like(x)
        pooled = torch.empty(B, T, H // 2, W // 2, C, device=x.device) if pool else None
        check(_lib.lib().vpx_bn_relu_fwd(ptr(x), ptr(stats), ptr(gc), ptr(bc), ptr(act), ptr(pooled), B * T, H, W, C, stream()), "vpx_bn_relu_fwd")
        if need_grad:
            ctx.save_for_backward(x, act, stats, gc)
        ctx.set_materialize_grads(False)   # (an unused output's gradient arrives as None, not as a tensor of zeros to read)
        return (act, pooled) if pool else act

    @staticmethod
    def backward(ctx, dact, dpool=None):
        sync_determinism()
        x, act, stats, gc = ctx.saved_tensors
        B, T, H, W, C = (int(s) for s in x.shape)
        L = _lib.lib()
        dact = None if dact is None else dact.contiguous()
        dpool = None if dpool is None else dpool.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, device=x.device) if ctx.needs_input_grad[2] else None
        dbeta = torch.empty(C, device=x.device) if ctx.needs_input_grad[3] else None
        ws, ws_bytes = workspace(x.device, L.vpx_bn_relu_bwd_workspace_bytes, B * T, H, W, C)
        check(L.vpx_bn_relu_bwd(ptr(x), ptr(act), ptr(stats), ptr(gc), ptr(dact), ptr(dpool), ptr(dx), ptr(dgamma), ptr(dbeta), B * T, H, W, C,
                                ptr(ws), ws_bytes, stream()), "vpx_bn_relu_bwd")
        return dx, None, dgamma, dbeta, None, None


def bn_relu(x, stats, gamma, beta, pool=False):
    """relu(BatchNorm(x)) with the batch statistics `stats` [2,C] = (mean, 1/std) of the training epilogue; x [B,T,H,W,C]. With `pool` also
    the (1,2,2) max-pool of the result: returns (act, pooled). The backward differentiates through the statistics."""
    for t in (x, stats, gamma, beta):
        require_gpu(t, "bn_relu")
    _frames(x, "bn_relu")
    C = int(x.shape[4])
    if tuple(stats.shape) != (2, C) or tuple(gamma.shape) != (C,) or tuple(beta.shape) != (C,):
        raise ValueError(f"bn_relu: statistics {tuple(stats.shape)} / gamma {tuple(gamma.shape)} / beta {tuple(beta.shape)} do not match {C} channels")
    if pool and (x.shape[2] % 2 or x.shape[3] % 2):
        raise ValueError(f"bn_relu: the 2x2 pool needs an even map, got {int(x.shape[2])}x{int(x.shape[3])}")
    return _BnReluFn.apply(x, stats, gamma, beta, bool(pool), needs_grad(x, gamma, beta))


def max_pool_2x2(x):
    """MaxPool3d((1,2,2)) of an activation [B,T,H,W,C]; inference only (in training bn_relu writes the pooled map in its own pass)."""
    require_gpu(x, "max_pool_2x2")
    _frames(x, "max_pool_2x2")
    if needs_grad(x):
        raise _lib.VpxError("max_pool_2x2: no backward in the library on its own (bn_relu(pool=True) has one)")
    B, T, H, W, C = (int(s) for s in x.shape)
    if H % 2 or W % 2:
        raise ValueError(f"max_pool_2x2: needs an even map, got {H}x{W}")
    pooled = torch.empty(B, T, H // 2, W // 2, C, device=x.device)
    check(_lib.lib().vpx_bn_relu_fwd(ptr(x), None, None, None, None, ptr(pooled), B * T, H, W, C, stream()), "vpx_bn_relu_fwd")
    return pooled


def conv_bn_relu(a, w, bn, b=None, pool=False):
    """One half of a DoubleConv block: relu(bn(replicate_conv(cat(a, b); w))), `bn` an nn.BatchNorm2d / 3d module.

    bn.training: the convolution's epilogue leaves the batch statistics (and updates bn's running statistics and
    num_batches_tracked, as nn.BatchNorm does with momentum 0.1); bn_relu normalises, with the pooled map in the same pass when `pool`.
    Otherwise ONE launch: the running statistics and the ReLU are applied in the convolution's epilogue (no backward: VpxError in a call
    that needs gradients). Returns act, or (act, pooled)."""
    d = _desc(a, b, w, _lib.RCONV_REPLICATE, "conv_bn_relu")
    params = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if any(p is None for p in params) or bn.eps != BN_EPS or bn.momentum != BN_MOMENTUM:
        raise ValueError("conv_bn_relu: needs an affine BatchNorm that tracks running statistics with eps 1e-5 and momentum 0.1")
    for p in params:
        require_gpu(p, "conv_bn_relu")
        if tuple(p.shape) != (d.Co,):
            raise ValueError(f"conv_bn_relu: BatchNorm over {tuple(p.shape)} channels after a convolution to {d.Co}")
    if bn.training:
        if d.B * d.T * d.H * d.W < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[d.B, d.Co, d.T, d.H, d.W]}")
        y, stats = _RConvStatsFn.apply(a, b, w, d, bn.running_mean, bn.running_var, needs_grad(a, b, w))
        bn.num_batches_tracked.add_(1)
        return bn_relu(y, stats, bn.weight, bn.bias, pool=pool)
    if needs_grad(a, b, w, bn.weight, bn.bias):
        raise _lib.VpxError("conv_bn_relu: the eval-mode layer (running statistics in the convolution's epilogue) has no backward in the library; "
                            "call it under torch.no_grad() or put the module in train() mode")
    wc = w.contiguous()
    L = _lib.lib()
    y = _out(d, a.device)
    ws, ws_bytes = workspace(a.device, L.vpx_rconv_workspace_bytes, ctypes.byref(d), _lib.RCONV_EPI_EVAL)
    check(L.vpx_rconv_fwd(ctypes.byref(d), _lib.RCONV_EPI_EVAL, ptr(a), ptr(b), ptr(wc), ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
                          ptr(bn.running_var), BN_EPS, 0.0, ptr(y), None, ptr(ws), ws_bytes, stream()), "vpx_rconv_fwd")
    return (y, max_pool_2x2(y)) if pool else y
