"""PhyDNet's operators over the C ABI (include/vpx.h): GroupNorm (+ LeakyReLU, + residual), the PhyCell correction, the moment
regularisation loss and the sigmoid output head, one autograd Function each, forward and backward in libvpx_hip
(csrc/groupnorm.hip, csrc/phydnet.hip).

Activations keep the reference's logical shapes ([N,C,H,W]) and live channels-last in memory, as everywhere in the package. Whether
a Function keeps its backward state is decided in the wrapper, where grad mode is visible (inside `Function.forward` grad mode is
off and `ctx.needs_input_grad` ignores `torch.no_grad()`). Shapes are checked here, before any launch."""

import torch

from . import _lib
from ._lib import check, ptr
from .ops import needs_grad, new_channels_last, require_gpu, stream, sync_determinism, to_channels_last, workspace


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
class _GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, r, G, act, slope, need_grad):
        xs = to_channels_last(x)
        N, C, H, W = xs.shape
        rs = None if r is None else to_channels_last(r)
        y = new_channels_last((N, C, H, W), x.device)
        stats = torch.empty(N * G * 2, device=x.device)
        gc, bc = gamma.contiguous(), beta.contiguous()
        check(_lib.lib().vpx_groupnorm_fwd(ptr(xs), ptr(gc), ptr(bc), ptr(rs), ptr(y), ptr(stats), N, H * W, C, G, int(act), float(slope),
                                           stream()), "vpx_groupnorm_fwd")
        if need_grad:
            ctx.save_for_backward(xs, stats, gc, bc)
            ctx.cfg = (G, int(act), float(slope), r is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        xs, stats, gc, bc = ctx.saved_tensors
        G, act, slope, has_r = ctx.cfg
        N, C, H, W = xs.shape
        L = _lib.lib()
        dys = to_channels_last(dy)
        dx = new_channels_last((N, C, H, W), dy.device)
        want_param = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dg = torch.empty(C, device=dy.device) if want_param else None
        db = torch.empty(C, device=dy.device) if want_param else None
        ws, ws_bytes = workspace(dy.device, L.vpx_groupnorm_bwd_workspace_bytes, N, C) if want_param else (None, 0)
        check(L.vpx_groupnorm_bwd(ptr(xs), ptr(stats), ptr(gc), ptr(bc), ptr(dys), ptr(dx), ptr(dg), ptr(db), N, H * W, C, G, act, slope,
                                  ptr(ws), ws_bytes, stream()), "vpx_groupnorm_bwd")
        dr = dy if (has_r and ctx.needs_input_grad[3]) else None
        return dx, dg, db, dr, None, None, None, None


def group_norm(x, num_groups, weight, bias, leaky_slope=None, residual=None):
    """act(GroupNorm(num_groups)(x)) + residual, act = LeakyReLU(leaky_slope) or the identity (leaky_slope None). x: [N,C,H,W] fp32 on the
    GPU (any memory layout; the output is channels-last)."""
    for t in (x, weight, bias, residual):
        if t is not None:
            require_gpu(t, "group_norm")
    if x.dim() != 4:
        raise ValueError(f"group_norm: expected a [N,C,H,W] tensor, got shape {tuple(x.shape)}")
    C = int(x.shape[1])
    if num_groups < 1 or C % num_groups:
        raise ValueError(f"group_norm: {C} channels are not divisible into {num_groups} groups")
    if C // num_groups > 256:
        raise ValueError(f"group_norm: {C // num_groups} channels per group (at most 256)")
    if tuple(weight.shape) != (C,) or tuple(bias.shape) != (C,):
        raise ValueError(f"group_norm: affine parameters {tuple(weight.shape)}, {tuple(bias.shape)} do not match {C} channels")
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError(f"group_norm: residual {tuple(residual.shape)} does not match the input {tuple(x.shape)}")
    act = leaky_slope is not None
    if act and leaky_slope < 0.0:
        raise ValueError("group_norm: the LeakyReLU slope must be non-negative (the backward reads its derivative from the sign)")
    return _GroupNormFn.apply(x, weight, bias, residual, int(num_groups), act, float(leaky_slope or 0.0),
                              needs_grad(x, weight, bias, residual))


# ---- PhyCell correction ----------------------------------------------------------------------------------------------------------
class _PhyCellCorrectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, Fh, h, E, need_grad):
        ts = [to_channels_last(t) for t in (G, Fh, h, E)]
        nxt = new_channels_last(tuple(G.shape), G.device)
        check(_lib.lib().vpx_phycell_correct_fwd(*[ptr(t) for t in ts], ptr(nxt), nxt.numel(), stream()), "vpx_phycell_correct_fwd")
        if need_grad:
            ctx.save_for_backward(*ts)
        return nxt

    @staticmethod
    def backward(ctx, dn):
        ts = ctx.saved_tensors
        dns = to_channels_last(dn)
        outs = [new_channels_last(tuple(ts[0].shape), dn.device) if ctx.needs_input_grad[i] else None for i in range(4)]
        check(_lib.lib().vpx_phycell_correct_bwd(*[ptr(t) for t in ts], ptr(dns), *[ptr(o) for o in outs], dns.numel(), stream()),
              "vpx_phycell_correct_bwd")
        return (*outs, None)


def phycell_correct(G, Fh, h, E):
    """PhyCell_Cell's update: ht = h + Fh, next = ht + sigmoid(G) * (E - ht). Four [B,C,H,W] tensors of one shape."""
    require_gpu(G, "phycell_correct")
    for name, t in (("F(h)", Fh), ("h", h), ("E", E)):
        if tuple(t.shape) != tuple(G.shape):
            raise ValueError(f"phycell_correct: {name} {tuple(t.shape)} does not match the gate {tuple(G.shape)}")
        require_gpu(t, "phycell_correct")
    if G.dim() != 4:
        raise ValueError(f"phycell_correct: expected [B,C,H,W] tensors, got shape {tuple(G.shape)}")
    return _PhyCellCorrectFn.apply(G, Fh, h, E, needs_grad(G, Fh, h, E))


# ---- moment loss -----------------------------------------------------------------------------------------------------------------
class _MomentLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, scale, need_grad):
        Wc = W.contiguous()
        hidden, Cin, kh, kw = (int(s) for s in Wc.shape)
        loss = torch.empty((), device=W.device)
        check(_lib.lib().vpx_moment_loss_fwd(ptr(Wc), ptr(loss), hidden, Cin, kh, kw, float(scale), stream()), "vpx_moment_loss_fwd")
        if need_grad:
            ctx.save_for_backward(Wc)
            ctx.scale = float(scale)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (Wc,) = ctx.saved_tensors
        hidden, Cin, kh, kw = (int(s) for s in Wc.shape)
        dl = dloss.detach().to(torch.float32).contiguous()
        dW = torch.empty_like(Wc)
        check(_lib.lib().vpx_moment_loss_bwd(ptr(Wc), ptr(dl), ptr(dW), hidden, Cin, kh, kw, ctx.scale, stream()), "vpx_moment_loss_bwd")
        return dW, None, None


def moment_loss(W, scale=1.0):
    """scale * sum_b mean((K2M(W[:, b]) - C)^2) for the PhyCell filter bank W [hidden, Cin, kh, kw] (phydnet.py PhyDNet.forward),
    evaluated in fp64 in one launch. C[o, i, j] = 1 where o == i * kw + j."""
    require_gpu(W, "moment_loss")
    if W.dim() != 4 or W.shape[2] > 8 or W.shape[3] > 8:
        raise ValueError(f"moment_loss: expected a [hidden, Cin, kh, kw] filter bank with kh, kw <= 8, got {tuple(W.shape)}")
    return _MomentLossFn.apply(W, float(scale), needs_grad(W))


# ---- sigmoid output head ---------------------------------------------------------------------------------------------------------
def _head_frames(x, nT):
    """x: [nT*B, C, H, W] (frame-major) -> its NHWC memory and (B, C, H, W)."""
    xs = to_channels_last(x)
    NB, C, H, W = xs.shape
    if NB % nT:
        raise ValueError(f"sigmoid_head: {NB} images are not {nT} frames of one batch")
    return xs, (NB // nT, C, H, W)


class _SigmoidHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nT, need_grad):
        xs, (B, C, H, W) = _head_frames(x, nT)
        out = torch.empty(B, nT, C, H, W, device=x.device)
        check(_lib.lib().vpx_sigmoid_head_fwd(ptr(xs), ptr(out), B, nT, 0, nT, C, H, W, stream()), "vpx_sigmoid_head_fwd")
        if need_grad:
            ctx.save_for_backward(out)
            ctx.xshape = tuple(xs.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        B, nT, C, H, W = out.shape
        dx = new_channels_last(ctx.xshape, dout.device)
        check(_lib.lib().vpx_sigmoid_head_bwd(ptr(out), ptr(dout.contiguous()), ptr(dx), B, nT, 0, nT, C, H, W, stream()),
              "vpx_sigmoid_head_bwd")
        return dx, None, None


def sigmoid_head(x, n_frames=1, out=None, t0=0):
    """sigmoid of the decoder's output. x: [n_frames*B, C, H, W], frame-major. With `out` ([B, T, C, H, W], contiguous) and no gradient
    needed, the frames are written straight into out[:, t0:t0+n_frames] and that view is returned; otherwise a new [B, n_frames, C, H, W]
    tensor is returned (differentiable)."""
    require_gpu(x, "sigmoid_head")
    if out is not None:
        require_gpu(out, "sigmoid_head")
    if x.dim() != 4:
        raise ValueError(f"sigmoid_head: expected a [N,C,H,W] tensor, got shape {tuple(x.shape)}")
    if out is not None and not needs_grad(x):
        xs, (B, C, H, W) = _head_frames(x, n_frames)
        if out.dim() != 5 or tuple(out.shape[:1]) + tuple(out.shape[2:]) != (B, C, H, W) or not out.is_contiguous() \
                or not 0 <= t0 <= out.shape[1] - n_frames:
            raise ValueError(f"sigmoid_head: result buffer {tuple(out.shape)} cannot take {n_frames} frames of {(B, C, H, W)} at slot {t0}")
        check(_lib.lib().vpx_sigmoid_head_fwd(ptr(xs), ptr(out), B, int(out.shape[1]), int(t0), int(n_frames), C, H, W, stream()),
              "vpx_sigmoid_head_fwd")
        return out[:, t0:t0 + n_frames]
    return _SigmoidHeadFn.apply(x, int(n_frames), needs_grad(x))
