"""The NonConvLSTM model's operators over the C ABI (include/vpx.h): the dense layer with strided rows, the LSTM cell, the stride-2
convolution with replicate padding and the differentiable bilinear resize; one autograd Function each, forward and backward in
libvpx_hip (csrc/dense.hip, csrc/lstm_glue.hip). Everything is fp32.

As in stphy_ops: whether a Function keeps its backward state is decided in the wrapper, where grad mode is visible; shapes are checked
here, before any launch; CPU tensors raise VpxError: there is no fallback. Matrices are row-major [rows, columns]; a dense layer reads
and writes rows with a stride (a column slice of a wider buffer), every other operand that is not contiguous is copied. Maps keep the
reference's logical shape [N,C,H,W] and live channels-last in memory; the resize hands back a plain contiguous [N,C,oh,ow] tensor."""
import ctypes

import torch

from . import _lib, stphy_ops
from ._lib import check, ptr
from .ops import needs_grad, new_channels_last, require_gpu, stream, sync_determinism, to_channels_last, workspace


def _rows(t):
    """(tensor, row stride) of a 2-d operand the library can read in place: unit column stride and rows that do not overlap; anything
    else is copied."""
    if t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1]):
        return t, (int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]))
    t = t.contiguous()
    return t, int(t.shape[1])


def dense_plan(M, N, K):
    """The launch a dense layer of (M, N, K) takes (vpx_dense_plan): {"split", "chunks", "chunk_len", "form", "tile_m", "tile_n",
    "m_tiles", "n_tiles"}. Needs no GPU."""
    info = _lib.DensePlanInfo()
    check(_lib.lib().vpx_dense_plan(int(M), int(N), int(K), ctypes.byref(info)), "vpx_dense_plan")
    return {n: int(getattr(info, n)) for n, _ in info._fields_}


# ---- dense layer ----------------------------------------------------------------------------------------------------------------------
class _DenseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, x, w, bias, relu, need_grad):   # (out first: autograd rebases a written view on input 0)
        xs, ldx = _rows(x)
        wc = w.contiguous()
        bc = None if bias is None else bias.contiguous()
        M, K = (int(s) for s in xs.shape)
        N = int(wc.shape[0])
        y = torch.empty(M, N, device=x.device) if out is None else out
        ldy = int(y.stride(0)) if M > 1 else N
        L = _lib.lib()
        ws, ws_bytes = workspace(x.device, L.vpx_dense_workspace_bytes, M, N, K)
        check(L.vpx_dense_fwd(ptr(xs), ldx, ptr(wc), ptr(bc), ptr(y), ldy, M, N, K, int(relu), ptr(ws), ws_bytes, stream()), "vpx_dense_fwd")
        if out is not None:
            ctx.mark_dirty(out)
        if need_grad:   # the output is kept only where the backward reads ReLU' off it (a copy when it lives in the caller's buffer)
            ctx.save_for_backward(xs, wc, *([y.detach().clone(memory_format=torch.contiguous_format) if out is not None else y] if relu else []))
            ctx.cfg = (bool(relu), bias is not None, ldx, out is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        xs, wc, *ys = ctx.saved_tensors
        relu, has_bias, ldx, has_out = ctx.cfg
        y = ys[0] if ys else None
        M, K = (int(s) for s in xs.shape)
        N = int(wc.shape[0])
        dys, lddy = _rows(dy)
        needs = ctx.needs_input_grad
        dx = torch.empty(M, K, device=dy.device) if needs[1] else None
        dw = torch.empty_like(wc) if needs[2] else None
        db = torch.empty(N, device=dy.device) if (has_bias and needs[3]) else None
        dout = torch.zeros_like(dy) if has_out else None   # what `out` held before is overwritten: no gradient reaches it
        if dx is None and dw is None and db is None:
            return dout, None, None, None, None, None
        L = _lib.lib()
        ws, ws_bytes = workspace(dy.device, L.vpx_dense_workspace_bytes, M, N, K)
        check(L.vpx_dense_bwd(ptr(xs), ldx, ptr(wc), ptr(y), N, ptr(dys), lddy, ptr(dx), K, ptr(dw), ptr(db), M, N, K, int(relu), 0, ptr(ws),
                              ws_bytes, stream()), "vpx_dense_bwd")
        return dout, dx, dw, db, None, None


def dense(x, w, bias=None, relu=False, out=None):
    """relu?(x @ w.T + bias): torch.nn.functional.linear for a 2-d x [M, K] and a Linear's weight [N, K], fp32 on the GPU. x may be a
    column slice of a wider matrix (unit column stride); `out`, a [M, N] tensor or column slice to write the result into (the bytes
    between its rows are not touched), is returned in place of a fresh tensor. Differentiable in x, w and bias."""
    for t in (x, w, bias, out):
        if t is not None:
            require_gpu(t, "dense")
    if x.dim() != 2 or w.dim() != 2 or int(x.shape[1]) != int(w.shape[1]) or x.shape[0] < 1 or w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError(f"dense: expected x [M, K] and w [N, K] with M, N, K >= 1, got {tuple(x.shape)} and {tuple(w.shape)}")
    if bias is not None and tuple(bias.shape) != (int(w.shape[0]),):
        raise ValueError(f"dense: bias {tuple(bias.shape)} does not match {int(w.shape[0])} output features")
    if out is not None:
        if tuple(out.shape) != (int(x.shape[0]), int(w.shape[0])) or _rows(out)[0] is not out:
            raise ValueError(f"dense: out must be a [{int(x.shape[0])}, {int(w.shape[0])}] tensor with unit column stride and rows that do not "
                             f"overlap, got shape {tuple(out.shape)} with strides {tuple(out.stride())}")
        if out.requires_grad and torch.is_grad_enabled() and out.is_leaf:
            raise ValueError("dense: out is a leaf that requires grad; it cannot be written in place")
    return _DenseFn.apply(out, x, w, bias, bool(relu), needs_grad(x, w, bias, out))


# ---- LSTM cell ------------------------------------------------------------------------------------------------------------------------
class _LSTMCellFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, c, w_ih, w_hh, b_ih, b_hh, need_grad):
        xs, ldx = _rows(x)
        hs = None if h is None else h.contiguous()
        cs = None if c is None else c.contiguous()
        wi, wh = w_ih.contiguous(), w_hh.contiguous()
        bi = None if b_ih is None else b_ih.contiguous()
        bh = None if b_hh is None else b_hh.contiguous()
        M, Kx = (int(s) for s in xs.shape)
        H = int(wh.shape[1])
        dev = x.device
        h_new, c_new = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
        gates = torch.empty(M, 4 * H, device=dev) if need_grad else None
        L = _lib.lib()
        ws, ws_bytes = workspace(dev, L.vpx_lstm_cell_workspace_bytes, M, Kx, H)
        check(L.vpx_lstm_cell_fwd(ptr(xs), ldx, ptr(hs), ptr(cs), ptr(wi), ptr(wh), ptr(bi), ptr(bh), ptr(h_new), ptr(c_new), ptr(gates), M, Kx, H,
                                  ptr(ws), ws_bytes, stream()), "vpx_lstm_cell_fwd")
        if need_grad:
            ctx.save_for_backward(xs, wi, wh, gates, *[t for t in (hs, cs) if t is not None])
            ctx.cfg = (ldx, hs is not None, cs is not None, bi is not None, bh is not None)
        return h_new, c_new

    @staticmethod
    def backward(ctx, dh_new, dc_new):
        sync_determinism()
        xs, wi, wh, gates, *state = ctx.saved_tensors
        ldx, has_h, has_c, has_bi, has_bh = ctx.cfg
        hs = state.pop(0) if has_h else None
        cs = state.pop(0) if has_c else None
        M, Kx = (int(s) for s in xs.shape)
        H = int(wh.shape[1])
        dev = gates.device
        needs = ctx.needs_input_grad
        dhn = None if dh_new is None else dh_new.contiguous()
        dcn = None if dc_new is None else dc_new.contiguous()
        dx = torch.empty(M, Kx, device=dev) if needs[0] else None
        dh = torch.empty(M, H, device=dev) if (has_h and needs[1]) else None
        dc = torch.empty(M, H, device=dev) if (has_c and needs[2]) else None
        dwi = torch.empty_like(wi) if needs[3] else None
        dwh = torch.empty_like(wh) if needs[4] else None
        dbi = torch.empty(4 * H, device=dev) if (has_bi and needs[5]) else None
        dbh = torch.empty(4 * H, device=dev) if (has_bh and needs[6]) else None
        dgates = torch.empty(M, 4 * H, device=dev)
        L = _lib.lib()
        ws, ws_bytes = workspace(dev, L.vpx_lstm_cell_workspace_bytes, M, Kx, H)
        check(L.vpx_lstm_cell_bwd(ptr(xs), ldx, ptr(hs), ptr(cs), ptr(wi), ptr(wh), ptr(gates), ptr(dhn), ptr(dcn), ptr(dx), ptr(dh), ptr(dc), ptr(dwi),
                                  ptr(dwh), ptr(dbi), ptr(dbh), ptr(dgates), M, Kx, H, 0, ptr(ws), ws_bytes, stream()), "vpx_lstm_cell_bwd")
        return dx, dh, dc, dwi, dwh, dbi, dbh, None


def lstm_cell(x, hc, w_ih, w_hh, b_ih=None, b_hh=None):
    """torch.nn.LSTMCell's forward, (h', c') = cell(x, (h, c)), one library call: x [M, Kx], h and c [M, H], w_ih [4H, Kx], w_hh [4H, H],
    biases [4H] (gate order i, f, g, o), fp32 on the GPU. `hc` None, or a None h or c, means a zero state: a zero h skips the h @ w_hh.T
    half of the product. Differentiable in every operand."""
    h, c = (None, None) if hc is None else hc
    for t in (x, h, c, w_ih, w_hh, b_ih, b_hh):
        if t is not None:
            require_gpu(t, "lstm_cell")
    if x.dim() != 2 or w_ih.dim() != 2 or w_hh.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1 or w_hh.shape[1] < 1:
        raise ValueError(f"lstm_cell: expected x [M, Kx], w_ih [4H, Kx] and w_hh [4H, H], got {tuple(x.shape)}, {tuple(w_ih.shape)}, {tuple(w_hh.shape)}")
    M, Kx, H = int(x.shape[0]), int(x.shape[1]), int(w_hh.shape[1])
    if tuple(w_ih.shape) != (4 * H, Kx) or tuple(w_hh.shape) != (4 * H, H):
        raise ValueError(f"lstm_cell: weights {tuple(w_ih.shape)} and {tuple(w_hh.shape)} do not fit an input of {Kx} features and {H} hidden units")
    for name, t in (("h", h), ("c", c)):
        if t is not None and tuple(t.shape) != (M, H):
            raise ValueError(f"lstm_cell: state {name} {tuple(t.shape)} is not [{M}, {H}]")
    for name, t in (("b_ih", b_ih), ("b_hh", b_hh)):
        if t is not None and tuple(t.shape) != (4 * H,):
            raise ValueError(f"lstm_cell: {name} {tuple(t.shape)} is not [{4 * H}]")
    return _LSTMCellFn.apply(x, h, c, w_ih, w_hh, b_ih, b_hh, needs_grad(x, h, c, w_ih, w_hh, b_ih, b_hh))


# ---- replicate padding + strided convolution ------------------------------------------------------------------------------------------------
class _ReplicatePadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad):
        xs = to_channels_last(x)
        N, C, H, W = (int(s) for s in xs.shape)
        y = new_channels_last((N, C, H + 2 * pad, W + 2 * pad), x.device)
        check(_lib.lib().vpx_replicate_pad_fwd(ptr(xs), ptr(y), N, H, W, C, pad, stream()), "vpx_replicate_pad_fwd")
        ctx.cfg = (N, C, H, W, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, pad = ctx.cfg
        dys = to_channels_last(dy)
        dx = new_channels_last((N, C, H, W), dy.device)
        check(_lib.lib().vpx_replicate_pad_bwd(ptr(dys), ptr(dx), N, H, W, C, pad, stream()), "vpx_replicate_pad_bwd")
        return dx, None


def replicate_pad(x, pad):
    """F.pad(x, (pad,) * 4, mode="replicate") for x [N,C,H,W] fp32 on the GPU (channels-last result). Differentiable."""
    require_gpu(x, "replicate_pad")
    if x.dim() != 4 or min(int(s) for s in x.shape) < 1 or int(pad) < 0:
        raise ValueError(f"replicate_pad: expected a non-empty [N,C,H,W] tensor and pad >= 0, got {tuple(x.shape)} and {pad}")
    return _ReplicatePadFn.apply(x, int(pad))


def conv2d_replicate(x, w, bias, stride=2, relu=True):
    """relu?(Conv2d(x; w, bias)) with padding_mode="replicate" and padding k // 2 for an odd square kernel and stride 1 or 2: the
    replicate-padded map through the library's convolution with padding 0. x [N,C,H,W] fp32 on the GPU, w [Co,Ci,k,k]."""
    for t in (x, w, bias):
        if t is not None:
            require_gpu(t, "conv2d_replicate")
    if x.dim() != 4 or w.dim() != 4 or w.shape[2] != w.shape[3] or not int(w.shape[2]) & 1:
        raise ValueError(f"conv2d_replicate: expected a [N,C,H,W] input and an odd square kernel, got {tuple(x.shape)} and {tuple(w.shape)}")
    xp = replicate_pad(x, int(w.shape[2]) // 2)
    return stphy_ops.conv2d_act(xp, w, bias, stride, 0, act="relu" if relu else None)


# ---- bilinear resize ------------------------------------------------------------------------------------------------------------------------
class _ResizeBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        xs = to_channels_last(x)
        N, C, H, W = (int(s) for s in xs.shape)
        y = torch.empty(N, C, oh, ow, device=x.device)
        check(_lib.lib().vpx_resize_bilinear_fwd(ptr(xs), ptr(y), N, C, H, W, oh, ow, stream()), "vpx_resize_bilinear_fwd")
        ctx.cfg = (N, C, H, W, oh, ow)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, oh, ow = ctx.cfg
        dyc = dy.contiguous()
        dx = new_channels_last((N, C, H, W), dy.device)
        check(_lib.lib().vpx_resize_bilinear_bwd(ptr(dyc), ptr(dx), N, C, H, W, oh, ow, stream()), "vpx_resize_bilinear_bwd")
        return dx, None, None


def resize_bilinear(x, out_hw):
    """F.interpolate(x, out_hw, mode="bilinear", align_corners=False), no antialiasing: what torchvision's Resize does to a float tensor
    that it enlarges (a side that shrinks is sampled, not averaged). x [N,C,H,W] fp32 on the GPU; a contiguous [N,C,oh,ow] result.
    Differentiable."""
    require_gpu(x, "resize_bilinear")
    oh, ow = (int(s) for s in out_hw)
    if x.dim() != 4 or min(int(s) for s in x.shape) < 1 or oh < 1 or ow < 1:
        raise ValueError(f"resize_bilinear: expected a non-empty [N,C,H,W] tensor and a positive output size, got {tuple(x.shape)} and {(oh, ow)}")
    return _ResizeBilinearFn.apply(x, oh, ow)
