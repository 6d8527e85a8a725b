"""torch-level operators over the C ABI (include/vpx.h). Tensors keep the reference's LOGICAL shapes
([B,T,C,H,W], [B,C,H,W]) but live channels-last in memory (NHWC) so that kernels get coalesced channel rows and the
glue convolutions of the models (HIP kernels of this library too, csrc/glue_fwd_api.hip) exchange activations with them without a copy."""
import collections
import contextlib
import ctypes
import weakref

import torch

from . import _lib
from ._lib import ConvDesc, ConvLSTMDesc, STLSTMDesc, check, ptr, ptr_array

VpxError = _lib.VpxError
PRECISIONS = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}


class KernelProfile:
    """Opt-in HIP-event bracket around every fused-cell library call (used by bench.py for the live roofline numbers).
    Events are recorded on the stream the kernels are launched on (torch's current stream)."""

    def __init__(self):
        self.records = []  # (start_event, end_event, algorithmic_flops, algorithmic_bytes, cell_launches, tag, wide_read_bytes)

    def summary(self):
        ms = sum(r[0].elapsed_time(r[1]) for r in self.records)
        # wide_read_bytes: the part of the algorithmic reads that reaches HBM as wide (128-byte, 16 B per lane) coalesced requests — the
        # epilogue's cell-state reads; the operand stages arrive as 64-byte segments by LDS-DMA. The two are tallied differently by
        # FETCH_SIZE on gfx950 (profiles/r06_fetch_calibration.md): the PMC summaries need the split to turn the counter into bytes.
        return dict(ms=ms, flops=sum(r[2] for r in self.records), bytes=sum(r[3] for r in self.records),
                    launches=sum(r[4] for r in self.records), wide_read_bytes=sum(r[6] for r in self.records if len(r) > 6))


PROFILE = None  # set to a KernelProfile() to collect
BWD_WEIGHT_PACK_REUSE = True   #: ST-LSTM backward: keep the transposed weight packs between the steps of one cell (tests switch it off)


@contextlib.contextmanager
def _profiled(tag, launches, work, wide_read_bytes=0.0):
    """The HIP-event bracket around one fused-cell library call while PROFILE collects (the call is the `with` body; a call that raises
    leaves no record). work() -> (algorithmic flops, algorithmic bytes), evaluated only then."""
    if PROFILE is None:
        yield
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    yield
    ev1.record()
    PROFILE.records.append((ev0, ev1, *work(), launches, tag, wide_read_bytes))


def require_gpu(t: torch.Tensor, what: str):
    sync_determinism()
    if not t.is_cuda:
        raise _lib.VpxError(f"{what}: tensors must live on the GPU (got device '{t.device}'). The hot path runs only as "
                            f"HIP kernels on MI355X; there is no CPU fallback.")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32 tensors, got {t.dtype}")


_det_state = None


def sync_determinism():
    """Mirrors torch.use_deterministic_algorithms() into the library (deterministic mode forbids the K-split
    convolutions' floating-point atomics, see include/vpx.h). Called at the start of every op, before any size query."""
    global _det_state
    det = torch.are_deterministic_algorithms_enabled()
    if det != _det_state:
        _lib.lib().vpx_set_deterministic(int(det))
        _det_state = det


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def needs_grad(*tensors):
    """True when a call on these tensors (None and non-tensor operands allowed) will need a backward. Asked in the wrappers: inside
    Function.forward grad mode is always off and ctx.needs_input_grad ignores torch.no_grad()."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


NOT_IMPLEMENTED = b"not implemented"


def workspace_bytes(query, *args, unsupported=None):
    """Answer of a `*_workspace_bytes` query. With `unsupported` — the words by which the query's message tells a problem the library
    does not implement (NotImplementedError) from a bad argument (ValueError) — an answer of 0, the query's refusal, raises through
    check(). Without it the answer is passed on as it is: those queries leave no message, the launch reports the error."""
    nbytes = query(*args)
    if nbytes == 0 and unsupported is not None:
        check(-4 if unsupported in _lib.lib().vpx_last_error() else -1, query.__name__)
    return nbytes


def workspace(dev, query, *args, unsupported=None):
    """(uint8 tensor, nbytes): the workspace a `*_workspace_bytes` query asks for (see workspace_bytes)."""
    nbytes = workspace_bytes(query, *args, unsupported=unsupported)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def reserve_buffer(dev, query, d):
    """(uint8 tensor, nbytes): the saved-for-backward buffer a `*_reserve_bytes` query asks for (0 bytes without SAVE_FOR_BWD: one byte,
    so that the library still gets a pointer)."""
    nbytes = query(ctypes.byref(d))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def conv_desc(xshape, wshape, stride, padding, transposed, slope, precision, out_pad=(0, 0)):
    """ConvDesc of a Conv2d / ConvTranspose2d layer with weight shape `wshape` (the reference's layout) on an input of logical shape
    `xshape` = (N, Ci, H, W). `precision`: a PREC_* code."""
    N, Ci, H, Wd = (int(s) for s in xshape)
    Co = int(wshape[1] if transposed else wshape[0])
    return ConvDesc(N, H, Wd, Ci, Co, int(wshape[2]), int(wshape[3]), int(stride), int(padding), int(bool(transposed)), float(slope), precision,
                    int(out_pad[0]), int(out_pad[1]))


def conv_out_shape(d):
    """(Ho, Wo) of the layer a ConvDesc describes; a descriptor the library refuses raises through check()."""
    ho, wo = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.lib().vpx_conv2d_ex_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)), "vpx_conv2d_ex_out_shape")
    return ho.value, wo.value


def to_channels_last(t: torch.Tensor) -> torch.Tensor:
    """Same logical tensor ([..., C, H, W]) with NHWC memory. No copy if it already is."""
    nd = t.dim()
    perm = list(range(nd - 3)) + [nd - 2, nd - 1, nd - 3]
    inv = list(range(nd - 3)) + [nd - 1, nd - 3, nd - 2]
    return t.permute(perm).contiguous().permute(inv)


def _unchanged(ref, version, addr, t=None, at=None):
    """The cache-entry test 'same tensor, still alive and unmodified': the weak reference still leads to a tensor (to `t` itself, when
    given) whose version counter is `version` and whose data is at `addr` (`at`: the address the caller is about to hand to the
    library instead of the tensor's own, i.e. that of its contiguous form)."""
    live = ref()
    if live is None or (t is not None and live is not t):
        return False
    return live._version == version and (live.data_ptr() if at is None else at) == addr


class _WorkspaceCache:
    """Workspaces (and with them packed weights) kept between inference calls while the owning weight tensor is unchanged.
    LRU with a byte budget; an entry whose weight tensor died, changed version or moved, or whose kernel-option epoch is
    stale, is dropped on the next insert — a ragged last batch, a varying horizon or an A/B option toggle cannot pin
    HBM beyond the budget."""

    def __init__(self, budget_bytes=4 << 30):
        self.budget, self.bytes, self.ents = budget_bytes, 0, collections.OrderedDict()

    def get(self, key, w, addr, need_bytes, dev, exact=True):
        ent = self.ents.get(key)
        if ent is None:
            return None
        ref, version, a, ws, _ = ent
        ok = _unchanged(ref, version, a, w, addr) and ws.device == dev and \
            (ws.numel() == need_bytes if exact else ws.numel() >= need_bytes)
        if not ok:
            self._drop(key)
            return None
        self.ents.move_to_end(key)
        return ws

    def put(self, key, w, addr, ws, epoch):
        self._drop(key)
        for k in [k for k, (ref, version, a, _, ep) in self.ents.items() if not _unchanged(ref, version, a) or ep != epoch]:
            self._drop(k)
        if ws.numel() > self.budget:   # larger than the whole budget: never kept (the caller re-packs every call)
            return
        while self.ents and self.bytes + ws.numel() > self.budget:
            self._drop(next(iter(self.ents)))
        try:
            self.ents[key] = (weakref.ref(w), w._version, addr, ws, epoch)
            self.bytes += ws.numel()
        except TypeError:
            pass

    def _drop(self, key):
        ent = self.ents.pop(key, None)
        if ent is not None:
            self.bytes -= ent[3].numel()

    def clear(self):
        self.ents.clear()
        self.bytes = 0

    def __len__(self):
        return len(self.ents)


_cl_cache = {}


def _cached_channels_last(p: torch.Tensor) -> torch.Tensor:
    """Channels-last copy of a parameter tensor, re-used while the SAME tensor object is unchanged (identity checked
    through a weak reference — a recycled address can never hit — plus (_version, data_ptr)): the peephole tensors
    [1,Ch,H,W] of a ConvLSTM block are converted once per optimizer step instead of once per call. Writes through
    `.data` do not bump `_version`; code doing that must call `ops.clear_layout_cache()`."""
    ent = _cl_cache.get(id(p))
    if ent is not None and _unchanged(*ent[:3], p):
        return ent[3]
    if len(_cl_cache) > 256:   # drop what died or went stale first; only a cache full of live entries is cleared
        for k in [k for k, ent in _cl_cache.items() if not _unchanged(*ent[:3])]:
            del _cl_cache[k]
        if len(_cl_cache) > 256:
            _cl_cache.clear()
    cl = to_channels_last(p.detach())
    try:
        _cl_cache[id(p)] = (weakref.ref(p), p._version, p.data_ptr(), cl)
    except TypeError:
        pass
    return cl


def clear_layout_cache():
    _cl_cache.clear()
    _clstm_ws.clear()
    _convq_ws.clear()


def is_channels_last(t: torch.Tensor) -> bool:
    nd = t.dim()
    perm = list(range(nd - 3)) + [nd - 2, nd - 1, nd - 3]
    return t.permute(perm).is_contiguous()


def new_channels_last(shape, device, dtype=torch.float32) -> torch.Tensor:
    """Uninitialised tensor of logical shape [..., C, H, W] with NHWC memory."""
    *lead, C, H, W = shape
    nd = len(shape)
    inv = list(range(nd - 3)) + [nd - 1, nd - 3, nd - 2]
    return torch.empty(*lead, H, W, C, device=device, dtype=dtype).permute(inv)


class SplitActivation:
    """An activation sequence in the library's split-bf16 operand format (include/vpx.h) — what a stage's last convolution
    hands to the recurrent block in inference so that no fp32 copy is written and no conversion pass runs. Not a tensor:
    only `ops.convlstm_seq` consumes it. `shape` is the logical [B, T, C, H, W]."""

    def __init__(self, buf, shape):
        self.buf, self.shape, self.device = buf, tuple(shape), buf.device


def convlstm_takes_split(B, T, Cin, Ch, H, W, k, gate_order, precision):
    """True when convlstm_seq on this problem (inference) consumes a SplitActivation input."""
    d = ConvLSTMDesc(B, T, Cin, Ch, H, W, k, k, gate_order, _lib.LAYOUT_NHWC, PRECISIONS[precision], 0)
    return bool(_lib.lib().vpx_convlstm_takes_split_input(ctypes.byref(d)))


_clstm_ws = _WorkspaceCache()
_CLSTM_WS_CACHE_LIMIT = 1 << 30   # bytes: larger workspaces (large batches) are not kept alive — there the repack is noise


def _kernel_options():
    """Epoch of the library's kernel-selection switches (they change which packs a workspace holds)."""
    return _lib.lib().vpx_option_epoch()


class _ConvLSTMSeqFn(torch.autograd.Function):
    """out, hT, cT = ConvLSTM over T steps. Replaces the python time loop of conv_lstm_hzzone.py:52-70 /
    conv_lstm_ndrplz.py:112-121 by ONE library call (T fused conv+gate launches on the current stream)."""

    @staticmethod
    def forward(ctx, x, h0, c0, W, b, Wci, Wcf, Wco, seq_len, gate_order, precision, in_channels, need_grad, out_split=False):
        ref = x.buf if isinstance(x, SplitActivation) else (x if x is not None else h0)
        require_gpu(ref, "convlstm_seq")
        dev = ref.device
        Ch = W.shape[0] // 4
        kh, kw = int(W.shape[2]), int(W.shape[3])
        Cin = int(in_channels)
        if W.shape[1] != Cin + Ch:
            raise ValueError(f"convlstm_seq: weight has {W.shape[1]} input channels, expected {Cin}+{Ch}")
        x_split = isinstance(x, SplitActivation)
        if x_split:
            B, T, cx, H, Wd = x.shape
            if cx != Cin or T != seq_len or need_grad:
                raise ValueError("convlstm_seq: a SplitActivation input must match (Cin, seq_len) exactly and is inference-only")
            x = x.buf
        elif x is not None:
            B, T, cx, H, Wd = x.shape
            if cx != Cin or T < seq_len:
                raise ValueError(f"convlstm_seq: input shape {tuple(x.shape)} does not match Cin={Cin}, T>={seq_len}")
            x = to_channels_last(x[:, :seq_len]) if T != seq_len else to_channels_last(x)
        else:
            B, _, H, Wd = h0.shape
        T = int(seq_len)
        h0c = None if h0 is None else to_channels_last(h0)
        c0c = None if c0 is None else to_channels_last(c0)
        peep = Wci is not None
        wci = _cached_channels_last(Wci) if peep else None
        wcf = _cached_channels_last(Wcf) if peep else None
        wco = _cached_channels_last(Wco) if peep else None
        Wc = W.contiguous()
        bc = None if b is None else b.contiguous()
        if out_split and need_grad:
            raise ValueError("convlstm_seq: out_split is inference-only")
        d = ConvLSTMDesc(B, T, Cin, Ch, H, Wd, kh, kw, gate_order, _lib.LAYOUT_NHWC, precision,
                         (_lib.FLAG_SAVE_FOR_BWD if need_grad else 0) | (_lib.FLAG_X_SPLIT if x_split else 0) |
                         (_lib.FLAG_OUT_SPLIT if out_split else 0))
        L = _lib.lib()
        ws_bytes = workspace_bytes(L.vpx_convlstm_workspace_bytes, ctypes.byref(d), unsupported=NOT_IMPLEMENTED)
        ws = None
        if not need_grad and ws_bytes <= _CLSTM_WS_CACHE_LIMIT:
            # inference: the block keeps its workspace, and with it the weight packs, while the weight tensor is unchanged
            # (identity by weak reference + version + address; kernel selection switches are part of the key)
            key = (id(W), B, T, Cin, Ch, H, Wd, kh, kw, gate_order, precision, x is None, h0 is None, x_split, out_split,
                   torch.are_deterministic_algorithms_enabled(), _kernel_options())
            ws = _clstm_ws.get(key, W, Wc.data_ptr(), ws_bytes, dev)
            if ws is not None:
                d.flags |= _lib.FLAG_WEIGHTS_PACKED
            else:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                _clstm_ws.put(key, W, Wc.data_ptr(), ws, _kernel_options())
        if ws is None:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        reserve, rs_bytes = reserve_buffer(dev, L.vpx_convlstm_reserve_bytes, d)
        if out_split:   # the sequence in operand format (no fp32 copy exists); h_T separately in fp32
            out = torch.empty(B * T * H * Wd * Ch, dtype=torch.float32, device=dev)
            hT = new_channels_last((B, Ch, H, Wd), dev)
        else:
            out = new_channels_last((B, T, Ch, H, Wd), dev)
            hT = out[:, T - 1]  # h_T IS the last slice of the output slab: a view, no copy
        cT = new_channels_last((B, Ch, H, Wd), dev)
        wide = 4.0 * H * Wd * Ch * B * (T if h0 is not None else T - 1)   # c_{t-1}, read by the fused step's epilogue in full lines
        with _profiled("convlstm_fwd", T, lambda: convlstm_algorithmic_work(B, T, Cin if x is not None else 0, Ch, H, Wd, kh, kw,
                                                                            h0 is not None, peep), wide):
            rc = L.vpx_convlstm_seq_fwd(ctypes.byref(d), ptr(x), ptr(h0c), ptr(c0c), ptr(Wc), ptr(bc), ptr(wci), ptr(wcf),
                                        ptr(wco), ptr(out), ptr(hT) if out_split else None, ptr(cT), ptr(reserve), rs_bytes, ptr(ws),
                                        ws_bytes, stream())
            check(rc, "vpx_convlstm_seq_fwd")
        if need_grad:
            ctx.save_for_backward(x, h0c, c0c, Wc, wci, wcf, wco, out, reserve)
            ctx.desc = d
            ctx.has_bias = b is not None
            ctx.rs_bytes = rs_bytes
        if out_split:
            return SplitActivation(out, (B, T, Ch, H, Wd)), hT, cT
        return out, hT, cT

    @staticmethod
    def backward(ctx, dout, dhT, dcT):
        sync_determinism()
        x, h0c, c0c, Wc, wci, wcf, wco, out, reserve = ctx.saved_tensors
        d = ctx.desc
        dev = out.device
        L = _lib.lib()
        B, T, Cin, Ch, H, Wd = d.B, d.T, d.Cin, d.Ch, d.H, d.W
        needs = ctx.needs_input_grad
        dout = None if dout is None else to_channels_last(dout)
        dhT = None if dhT is None else to_channels_last(dhT)
        dcT = None if dcT is None else to_channels_last(dcT)
        dx = new_channels_last((B, T, Cin, H, Wd), dev) if (x is not None and needs[0]) else None
        dh0 = new_channels_last((B, Ch, H, Wd), dev) if (h0c is not None and needs[1]) else None
        dc0 = new_channels_last((B, Ch, H, Wd), dev) if (c0c is not None and needs[2]) else None
        dW = torch.empty_like(Wc) if needs[3] else None
        db = torch.empty(4 * Ch, device=dev) if (ctx.has_bias and needs[4]) else None
        peep = wci is not None
        dwci = new_channels_last((1, Ch, H, Wd), dev) if (peep and needs[5]) else None
        dwcf = new_channels_last((1, Ch, H, Wd), dev) if (peep and needs[6]) else None
        dwco = new_channels_last((1, Ch, H, Wd), dev) if (peep and needs[7]) else None
        ws, ws_bytes = workspace(dev, L.vpx_convlstm_workspace_bytes, ctypes.byref(d))
        rc = L.vpx_convlstm_seq_bwd(ctypes.byref(d), ptr(x), ptr(h0c), ptr(c0c), ptr(Wc), ptr(wci), ptr(wcf), ptr(wco),
                                    ptr(out), ptr(reserve), ctx.rs_bytes, ptr(dout), ptr(dhT), ptr(dcT), ptr(dx),
                                    ptr(dh0), ptr(dc0), ptr(dW), ptr(db), ptr(dwci), ptr(dwcf), ptr(dwco), ptr(ws),
                                    ws_bytes, stream())
        check(rc, "vpx_convlstm_seq_bwd")
        return dx, dh0, dc0, dW, db, dwci, dwcf, dwco, None, None, None, None, None


def convlstm_algorithmic_work(B, T, Cin, Ch, H, W, kh, kw, has_h0=True, peephole=True, dt=4):
    """Algorithmic FLOPs and bytes of a ConvLSTM sequence call: per cell-step and sample
    flops = 2*4Ch*(Cin+Ch)*k^2*H*W over the operand ranges that are not identically zero;
    bytes = dt*H*W*(Cin + 2Ch + 2Ch) (read x,h,c; write h,c) + per-step shared weights/bias/peepholes."""
    flops = 0.0
    nbytes = 0.0
    for t in range(T):
        kc = Cin + (Ch if (t > 0 or has_h0) else 0)
        flops += 2.0 * 4 * Ch * kc * kh * kw * H * W * B
        nbytes += dt * H * W * (Cin + 4 * Ch) * B
        nbytes += dt * (4 * Ch * (Cin + Ch) * kh * kw + 4 * Ch + (3 * Ch * H * W if peephole else 0))
    return flops, nbytes


def convlstm_writes_split(B, T, Cin, Ch, H, W, k, gate_order, precision):
    """True when convlstm_seq on this problem (inference) can hand its output sequence out as a SplitActivation (out_split=True)."""
    d = ConvLSTMDesc(B, T, Cin, Ch, H, W, k, k, gate_order, _lib.LAYOUT_NHWC, PRECISIONS[precision], 0)
    return bool(_lib.lib().vpx_convlstm_writes_split_output(ctypes.byref(d)))


def convlstm_seq(x, h0, c0, W, b, Wci=None, Wcf=None, Wco=None, *, seq_len, in_channels, gate_order=_lib.GATE_IFGO,
                 precision="f32", out_split=False):
    """x: [B,T,Cin,H,W] or None; h0/c0: [B,Ch,H,W] or None (not both x and h0 None). Returns (out [B,T,Ch,H,W], hT, cT);
    out_split (inference, where convlstm_writes_split says so): `out` is a SplitActivation — the sequence in the library's operand
    format for a consumer that reads it (conv2d_ex_from_split); no fp32 copy of it is written."""
    if x is None and h0 is None:
        raise ValueError("convlstm_seq: inputs and states must not both be None")
    # grad mode is always off INSIDE Function.forward, so decide here whether the forward must fill the reserve
    need_grad = needs_grad(x, h0, c0, W, b, Wci, Wcf, Wco)
    if isinstance(x, SplitActivation) or out_split:   # autograd.Function.apply only takes / returns tensors: call the forward body directly
        if need_grad:
            raise ValueError("convlstm_seq: split-format input / output is inference-only")

        class _Ctx:   # (inference only: nothing is saved)
            needs_input_grad = (False,) * 13
        if x is not None and not isinstance(x, SplitActivation) and x.dim() == 5 and x.shape[1] > seq_len:
            x = x[:, :seq_len]
        return _ConvLSTMSeqFn.forward(_Ctx(), x, h0, c0, W, b, Wci, Wcf, Wco, int(seq_len), int(gate_order), PRECISIONS[precision],
                                      int(in_channels), False, bool(out_split))
    if x is not None and x.dim() == 5 and x.shape[1] > seq_len:
        x = x[:, :seq_len]  # sliced here, outside the Function: autograd pads dx back to x's shape
    return _ConvLSTMSeqFn.apply(x, h0, c0, W, b, Wci, Wcf, Wco, int(seq_len), int(gate_order), PRECISIONS[precision],
                                int(in_channels), need_grad)


class _Conv2dSameFn(torch.autograd.Function):
    """Stride-1 'same' convolution through the library's implicit-GEMM kernel, with explicit backward
    (data gradient = same kernel with transposed/flipped packing, weight gradient = MFMA wgrad kernel)."""

    @staticmethod
    def forward(ctx, x, w, bias, precision):
        require_gpu(x, "conv2d_same")
        xs = to_channels_last(x)
        N, Ci, H, Wd = xs.shape
        Co, ci_w, kh, kw = w.shape
        if ci_w != Ci:
            raise ValueError(f"conv2d_same: weight expects {ci_w} input channels, input has {Ci}")
        wc = w.contiguous()
        bc = None if bias is None else bias.contiguous()
        L = _lib.lib()
        ws, ws_bytes = workspace(x.device, L.vpx_conv2d_workspace_bytes, Ci, Co, kh, kw)
        y = new_channels_last((N, Co, H, Wd), x.device)
        rc = L.vpx_conv2d_nhwc_fwd(ptr(xs), ptr(wc), ptr(bc), ptr(y), N, H, Wd, Ci, Co, kh, kw, precision, ptr(ws),
                                   ws_bytes, stream())
        check(rc, "vpx_conv2d_nhwc_fwd")
        ctx.save_for_backward(xs, wc)
        ctx.has_bias = bias is not None
        ctx.precision = precision
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        xs, wc = ctx.saved_tensors
        N, Ci, H, Wd = xs.shape
        Co, _, kh, kw = wc.shape
        dys = to_channels_last(dy)
        needs = ctx.needs_input_grad
        dx = new_channels_last((N, Ci, H, Wd), xs.device) if needs[0] else None
        dw = torch.empty_like(wc) if needs[1] else None
        db = torch.empty(Co, device=xs.device) if (ctx.has_bias and needs[2]) else None
        L = _lib.lib()
        ws, ws_bytes = workspace(xs.device, L.vpx_conv2d_bwd_workspace_bytes, N, H, Wd, Ci, Co, kh, kw)
        rc = L.vpx_conv2d_nhwc_bwd(ptr(xs), ptr(wc), ptr(dys), ptr(dx), ptr(dw), ptr(db), N, H, Wd, Ci, Co, kh, kw,
                                   ctx.precision, ptr(ws), ws_bytes, stream())
        check(rc, "vpx_conv2d_nhwc_bwd")
        return dx, dw, db, None


def conv2d_same(x, w, bias=None, precision="f32"):
    """y = conv2d(x, w, bias, stride=1, padding=k//2) on a [N,C,H,W] tensor (PredRNN's 1x1 frame head,
    predrnn_v2.py:223, and any other stride-1 'same' convolution); differentiable."""
    return _Conv2dSameFn.apply(x, w, bias, PRECISIONS[precision])




class _ConvExFn(torch.autograd.Function):
    """Conv2d / ConvTranspose2d (stride 1 or 2) + bias + LeakyReLU in ONE library launch (4 for a stride-2 transposed
    conv) — the EF stage glue of ef_blocks.py:15-49. Forward and backward (LeakyReLU', bias / data / weight gradients)
    run in libvpx_hip. A layer whose backward the library does not implement (kernel smaller than its stride, negative slope)
    raises VpxError in the FORWARD of a call that will need gradients — not after a whole forward pass has been spent."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, transposed, slope, precision, out_pad=(0, 0)):
        require_gpu(x, "conv2d_ex")
        xs = to_channels_last(x)
        N, Ci, H, Wd = xs.shape
        if int(w.shape[0] if transposed else w.shape[1]) != Ci:
            raise ValueError(f"conv2d_ex: weight {tuple(w.shape)} does not match {Ci} input channels")
        wc = w.contiguous()
        bc = None if bias is None else bias.contiguous()
        d = conv_desc(xs.shape, w.shape, stride, padding, transposed, slope, precision, out_pad)
        L = _lib.lib()
        y = new_channels_last((N, d.Co, *conv_out_shape(d)), x.device)
        x_sp = None
        if (ctx.needs_input_grad[1] and tuple(out_pad) == (0, 0) and L.vpx_conv2d_ex_bwd_uses_split(ctypes.byref(d))
                and L.vpx_conv2d_ex_takes_split(ctypes.byref(d))):
            # a training call whose weight gradient will want x in the split operand format anyway (wgrad2.hip, glue form): convert once,
            # run the forward on the split-input kernels (convq / c16 / first generation without its in-kernel conversion) and keep the copy
            x_sp = torch.empty(xs.numel(), dtype=torch.float32, device=x.device)
            check(L.vpx_split_convert(ptr(xs), ptr(x_sp), N * H * Wd, Ci, stream()), "vpx_split_convert")
            ws, ws_bytes = workspace(x.device, L.vpx_conv2d_ex_split_workspace_bytes, ctypes.byref(d))
            check(L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), ptr(x_sp), 0, 0, 1, ptr(wc), ptr(bc), ptr(y), None, 0, ptr(ws), ws_bytes,
                                                 stream()), "vpx_conv2d_ex_fwd_from_split")
        else:
            ws, ws_bytes = workspace(x.device, L.vpx_conv2d_ex_workspace_bytes, ctypes.byref(d))
            check(L.vpx_conv2d_ex_fwd(ctypes.byref(d), ptr(xs), ptr(wc), ptr(bc), ptr(y), ptr(ws), ws_bytes, stream()),
                  "vpx_conv2d_ex_fwd")
        ctx.x_sp = x_sp
        ctx.save_for_backward(xs, wc, y)
        ctx.cfg = (float(slope), bias is not None)
        ctx.desc = d
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        xs, wc, y = ctx.saved_tensors
        slope, has_bias = ctx.cfg
        mask = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]]
        d = ctx.desc
        if d.kh >= d.stride and d.kw >= d.stride and slope >= 0.0:
            # library path: LeakyReLU' + bias gradient in one pass over dy, dx = the adjoint layer on the implicit-GEMM kernel,
            # dw on the MFMA weight-gradient kernel
            L = _lib.lib()
            dyc = to_channels_last(dy)
            ws, ws_bytes = workspace(dy.device, L.vpx_conv2d_ex_bwd_workspace_bytes, ctypes.byref(d), unsupported=NOT_IMPLEMENTED)
            dx = new_channels_last(tuple(xs.shape), dy.device) if mask[0] else None
            dw = torch.empty_like(wc) if mask[1] else None
            db = torch.empty(d.Co, device=dy.device) if mask[2] else None
            check(L.vpx_conv2d_ex_bwd_ex(ctypes.byref(d), ptr(xs), ptr(ctx.x_sp), ptr(wc), ptr(y), ptr(dyc), ptr(dx), ptr(dw), ptr(db), ptr(ws),
                                         ws_bytes, stream()), "vpx_conv2d_ex_bwd")
            ctx.x_sp = None
            return dx, dw, db, None, None, None, None, None, None
        # No second backend in the product path: a layer the library's glue backward does not implement fails loudly.
        raise _lib.VpxError(f"conv2d_ex backward: layer (k={d.kh}x{d.kw}, stride={d.stride}, transposed={bool(d.transposed)}, slope={slope}) "
                       f"is outside vpx_conv2d_ex_bwd (needs kernel >= stride and a non-negative LeakyReLU slope): unsupported")


def conv2d_ex(x, w, bias, stride, padding, transposed=False, leaky_slope=0.0, precision="f32", output_padding=(0, 0)):
    """Conv2d / ConvTranspose2d (stride 1 or 2; `output_padding` for transposed layers) + bias + LeakyReLU, differentiable."""
    kh, kw = int(w.shape[2]), int(w.shape[3])
    # (decided here: inside Function.forward grad mode is always off and needs_input_grad ignores torch.no_grad())
    if needs_grad(x, w, bias):
        ok = kh >= stride and kw >= stride and leaky_slope >= 0.0
        if ok and x.dim() == 4:   # ... and the adjoint layer must be one the library runs (the same query the backward makes)
            d = conv_desc(x.shape, w.shape, stride, padding, transposed, leaky_slope, PRECISIONS[precision], output_padding)
            L = _lib.lib()
            ho, wo = ctypes.c_int(0), ctypes.c_int(0)
            if L.vpx_conv2d_ex_out_shape(ctypes.byref(d), ctypes.byref(ho), ctypes.byref(wo)) == 0:
                ok = L.vpx_conv2d_ex_bwd_workspace_bytes(ctypes.byref(d)) != 0
        if not ok:
            raise _lib.VpxError(f"conv2d_ex: layer (k={kh}x{kw}, stride={stride}, padding={padding}, transposed={bool(transposed)}, slope={leaky_slope}) has no "
                                f"backward in the library (vpx_conv2d_ex_bwd needs kernel >= stride, a non-negative LeakyReLU slope and an adjoint layer "
                                f"it implements: padding <= kernel - 1): unsupported in a call that requires gradients")
    return _ConvExFn.apply(x, w, bias, stride, padding, transposed, leaky_slope, PRECISIONS[precision], tuple(output_padding))


def conv2d_ex_split(x, w, bias, stride, padding, transposed=False, leaky_slope=0.0, precision="f32"):
    """conv2d_ex in inference with the output ONLY in the split-bf16 operand format: returns (buffer, (N, Co, Ho, Wo)).
    The buffer has the byte size of the fp32 NHWC output it replaces."""
    require_gpu(x, "conv2d_ex_split")
    xs = to_channels_last(x)
    d = conv_desc(xs.shape, w.shape, stride, padding, transposed, leaky_slope, PRECISIONS[precision])
    L = _lib.lib()
    ho, wo = conv_out_shape(d)
    ws, ws_bytes = workspace(x.device, L.vpx_conv2d_ex_workspace_bytes, ctypes.byref(d))
    buf = torch.empty(d.N * ho * wo * d.Co, dtype=torch.float32, device=x.device)
    wc = w.contiguous()
    bc = None if bias is None else bias.contiguous()
    check(L.vpx_conv2d_ex_fwd_split(ctypes.byref(d), ptr(xs), ptr(wc), ptr(bc), None, ptr(buf), ptr(ws), ws_bytes, stream()),
          "vpx_conv2d_ex_fwd_split")
    return buf, (d.N, d.Co, ho, wo)


def split_convert(x, native=True):
    """fp32 [..., C, H, W] tensor -> SplitActivation-style buffer in the split-bf16 operand format (vpx_split_convert for a
    channels-last 4-D batch; otherwise — and with native=False, the tests' cross-check — the same rounding with torch ops).
    Returns (buffer, logical shape)."""
    require_gpu(x, "split_convert")
    xs = to_channels_last(x)
    C = xs.shape[-3]
    if C % 8:
        raise ValueError("split_convert: the channel count must be a multiple of 8")
    if native and xs.dim() == 4 and xs.dtype == torch.float32 and xs.is_contiguous(memory_format=torch.channels_last):
        buf = torch.empty(xs.numel(), device=xs.device, dtype=torch.float32)
        n, _, h, w = xs.shape
        check(_lib.lib().vpx_split_convert(ptr(xs), ptr(buf), n * h * w, C, stream()), "vpx_split_convert")
        return buf, tuple(x.shape)
    # fp32 hi/lo split on the GPU with torch ops (same rounding as the kernels: round-to-nearest-even to bf16, twice)
    flat = xs.permute(*range(xs.dim() - 3), xs.dim() - 2, xs.dim() - 1, xs.dim() - 3).contiguous()   # [..., H, W, C]
    hi = flat.to(torch.bfloat16)
    lo = (flat - hi.to(torch.float32)).to(torch.bfloat16)
    g = flat.shape[:-1] + (C // 8, 8)
    buf = torch.stack([hi.reshape(g), lo.reshape(g)], dim=-2).contiguous()   # [..., C/8, 2, 8] bf16
    return buf.view(torch.float32).reshape(-1), tuple(x.shape)


_convq_ws = _WorkspaceCache()


def conv2d_ex_takes_split(N, H, W, Ci, Co, kh, kw, stride, padding, transposed, precision="bf16x3"):
    d = conv_desc((N, Ci, H, W), (Ci, Co, kh, kw) if transposed else (Co, Ci, kh, kw), stride, padding, transposed, 0.0, PRECISIONS[precision])
    return bool(_lib.lib().vpx_conv2d_ex_takes_split(ctypes.byref(d)))


def conv2d_ex_prefers_split(N, H, W, Ci, Co, kh, kw, stride, padding, transposed, precision="bf16x3"):
    """True when the layer runs on the schedule-driven K = 32 kernel (convq) given split input — for stride-2 transposed layers
    that is worth converting an fp32 input first (all four output phases in one launch)."""
    d = conv_desc((N, Ci, H, W), (Ci, Co, kh, kw) if transposed else (Co, Ci, kh, kw), stride, padding, transposed, 0.0, PRECISIONS[precision])
    return _lib.lib().vpx_conv2d_ex_takes_split(ctypes.byref(d)) == 2


def conv2d_ex_from_split(xbuf, xshape, w, bias, stride, padding, transposed=False, leaky_slope=0.0, precision="bf16x3",
                         out_split=False, out_fp32=True):
    """The stage-glue layer on an input that already is in the split-bf16 operand format (inference): xbuf / xshape =
    (buffer, (N, Ci, H, W)). Returns (y or None, ybuf or None, (N, Co, Ho, Wo)). The packed weights stay in a per-layer
    workspace while the weight tensor is unchanged (keyed on the tensor object, its version and address)."""
    N, Ci, H, Wd = xshape
    d = conv_desc(xshape, w.shape, stride, padding, transposed, leaky_slope, PRECISIONS[precision])
    Co, kh, kw = d.Co, d.kh, d.kw
    L = _lib.lib()
    ho, wo = conv_out_shape(d)
    ws_bytes = L.vpx_conv2d_ex_split_workspace_bytes(ctypes.byref(d))
    if ws_bytes == 0:
        raise _lib.VpxError("conv2d_ex_from_split: layer not implemented on split input: " + L.vpx_last_error().decode())
    key = (id(w), N, H, Wd, Ci, Co, kh, kw, int(stride), int(padding), bool(transposed), precision, L.vpx_conv2d_ex_takes_split(ctypes.byref(d)),
           torch.are_deterministic_algorithms_enabled(), _kernel_options())
    packed = 0
    ws = _convq_ws.get(key, w, w.data_ptr(), ws_bytes, xbuf.device, exact=False)
    if ws is not None:
        packed = 1
    else:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xbuf.device)
        _convq_ws.put(key, w, w.data_ptr(), ws, _kernel_options())
    wc = w.contiguous()
    if wc.data_ptr() != w.data_ptr():
        packed = 0
    bc = None if bias is None else bias.contiguous()
    y = new_channels_last((N, Co, ho, wo), xbuf.device) if out_fp32 else None
    ybuf = torch.empty(N * ho * wo * Co, dtype=torch.float32, device=xbuf.device) if out_split else None
    check(L.vpx_conv2d_ex_fwd_from_split(ctypes.byref(d), ptr(xbuf), 0, 0, 1, ptr(wc), ptr(bc), ptr(y), ptr(ybuf), packed, ptr(ws),
                                         ws_bytes, stream()), "vpx_conv2d_ex_fwd_from_split")
    return y, ybuf, (N, Co, ho, wo)


def conv_transpose2d_to_size(x, w, stride, padding, out_hw, precision="f32"):
    """nn.ConvTranspose2d(...)(x, output_size=out_hw) without bias (predrnn_v2.py:213-218): the output padding is whatever
    makes the result exactly out_hw (it must lie in [0, stride))."""
    kh, kw = int(w.shape[2]), int(w.shape[3])
    base = ((x.shape[-2] - 1) * stride - 2 * padding + kh, (x.shape[-1] - 1) * stride - 2 * padding + kw)
    op = (int(out_hw[0]) - base[0], int(out_hw[1]) - base[1])
    if min(op) < 0 or max(op) >= max(stride, 1):
        raise ValueError(f"requested output size {tuple(out_hw)} is not reachable (needs output padding {op}, stride {stride})")
    return conv2d_ex(x, w, None, stride, padding, True, 0.0, precision, op)


def glue_supported(kh, kw, stride, padding, transposed) -> bool:
    """Configurations vpx_conv2d_ex_fwd implements. Anything else is refused when a model is built (models/ef_conv_lstm._validate_stage):
    the product has no second convolution backend."""
    if stride not in (1, 2) or kh > 7 or kw > 7 or padding < 0:
        return False
    if transposed and stride == 1:
        return kh - 1 - padding >= 0 and kw - 1 - padding >= 0
    if transposed and stride == 2:
        return kh >= 2 and kw >= 2
    return True


class _DecoupleFn(torch.autograd.Function):
    """mean_{b,ch} |cos(normalize(A*delta_c), normalize(A*delta_m))| over H*W  (predrnn_v2.py:197-198, 209-211)."""

    @staticmethod
    def forward(ctx, delta_c, delta_m, adapter_w, precision):
        require_gpu(delta_c, "decouple_term")
        dc, dm = to_channels_last(delta_c), to_channels_last(delta_m)
        B, Ch, H, Wd = dc.shape
        A = adapter_w.reshape(Ch, Ch).contiguous()
        L = _lib.lib()
        ws, ws_bytes = workspace(dc.device, L.vpx_decouple_workspace_bytes, B, Ch, H, Wd)
        value = torch.empty((), device=dc.device)
        rc = L.vpx_decouple_fwd(ptr(dc), ptr(dm), ptr(A), ptr(value), B, Ch, H, Wd, precision, ptr(ws), ws_bytes, stream())
        check(rc, "vpx_decouple_fwd")
        ctx.save_for_backward(dc, dm, A)
        ctx.precision = precision
        ctx.wshape = tuple(adapter_w.shape)
        return value

    @staticmethod
    def backward(ctx, dvalue):
        sync_determinism()
        dc, dm, A = ctx.saved_tensors
        B, Ch, H, Wd = dc.shape
        needs = ctx.needs_input_grad
        if needs[0] and needs[1]:
            gg = new_channels_last((2 * B, Ch, H, Wd), dc.device)  # adjacent: one adjoint conv for the pair
            g_dc, g_dm = gg[:B], gg[B:]
        else:
            g_dc = new_channels_last((B, Ch, H, Wd), dc.device) if needs[0] else None
            g_dm = new_channels_last((B, Ch, H, Wd), dc.device) if needs[1] else None
        g_A = torch.empty_like(A) if needs[2] else None
        L = _lib.lib()
        ws, ws_bytes = workspace(dc.device, L.vpx_decouple_workspace_bytes, B, Ch, H, Wd)
        dv = dvalue.contiguous().reshape(1)
        rc = L.vpx_decouple_bwd(ptr(dc), ptr(dm), ptr(A), ptr(dv), ptr(g_dc), ptr(g_dm), ptr(g_A), B, Ch, H, Wd,
                                ctx.precision, ptr(ws), ws_bytes, stream())
        check(rc, "vpx_decouple_bwd")
        return g_dc, g_dm, (None if g_A is None else g_A.reshape(ctx.wshape)), None


def decouple_term(delta_c, delta_m, adapter_w, precision="f32"):
    """`precision`: arithmetic of the adapter contractions — pass the model's operand mode (default: exact fp32)."""
    return _DecoupleFn.apply(delta_c, delta_m, adapter_w, PRECISIONS[precision])


class _DecoupleBatchFn(torch.autograd.Function):
    """The decoupling term of ALL K layer-steps of a pass in one library call each way. `slab` is [2, K*B, Ch, H, W] (channels-last):
    slab[0] holds the K steps' delta_c one after the other, slab[1] their delta_m; `deltas` = (dc_0, dm_0, dc_1, dm_1, ...) are the
    steps' own output tensors — views of those slots — passed so that autograd has an edge to every step; the data is read from the
    slab. mean over (K*B, channel) of |cos| = the mean over the K steps of the per-step means (equal B): predrnn_v2.py:197-211, 229."""

    @staticmethod
    def forward(ctx, adapter_w, precision, slab, K, B, *deltas):
        require_gpu(slab, "decouple_term_batched")
        _, KB, Ch, H, Wd = slab.shape
        if KB != K * B or len(deltas) != 2 * K:
            raise ValueError("decouple_term_batched: the slab does not hold K steps of B samples / 2K delta tensors")
        n = B * Ch * H * Wd
        for k in (0, K - 1):   # the steps wrote where the slab expects them (first and last: the rest follow the same arithmetic)
            if deltas[2 * k].data_ptr() != slab[0].data_ptr() + 4 * k * n or deltas[2 * k + 1].data_ptr() != slab[1].data_ptr() + 4 * k * n:
                raise ValueError("decouple_term_batched: a step's delta tensor is not its slot of the slab")
        dc, dm = slab[0], slab[1]
        if not (is_channels_last(dc) and dm.data_ptr() == dc.data_ptr() + 4 * K * n):
            raise ValueError("decouple_term_batched: slab must be one dense channels-last block")
        A = adapter_w.reshape(Ch, Ch).contiguous()
        L = _lib.lib()
        ws, ws_bytes = workspace(slab.device, L.vpx_decouple_workspace_bytes, KB, Ch, H, Wd)
        value = torch.empty((), device=slab.device)
        check(L.vpx_decouple_fwd(ptr(dc), ptr(dm), ptr(A), ptr(value), KB, Ch, H, Wd, precision, ptr(ws), ws_bytes, stream()), "vpx_decouple_fwd")
        ctx.save_for_backward(slab, A)
        ctx.geo = (K, B, precision, tuple(adapter_w.shape))
        return value

    @staticmethod
    def backward(ctx, dvalue):
        sync_determinism()
        slab, A = ctx.saved_tensors
        K, B, precision, wshape = ctx.geo
        _, KB, Ch, H, Wd = slab.shape
        gg = new_channels_last((2 * KB, Ch, H, Wd), slab.device)   # adjacent: one adjoint conv for the pair
        g_dc, g_dm = gg[:KB], gg[KB:]
        g_A = torch.empty_like(A) if ctx.needs_input_grad[0] else None
        L = _lib.lib()
        ws, ws_bytes = workspace(slab.device, L.vpx_decouple_workspace_bytes, KB, Ch, H, Wd)
        dv = dvalue.contiguous().reshape(1)
        check(L.vpx_decouple_bwd(ptr(slab[0]), ptr(slab[1]), ptr(A), ptr(dv), ptr(g_dc), ptr(g_dm), ptr(g_A), KB, Ch, H, Wd, precision,
                                 ptr(ws), ws_bytes, stream()), "vpx_decouple_bwd")
        per_step = []
        for k in range(K):   # every step's gradients are views of the two slabs: no copies
            per_step += [g_dc[k * B:(k + 1) * B], g_dm[k * B:(k + 1) * B]]
        return (None if g_A is None else g_A.reshape(wshape), None, None, None, None, *per_step)


def decouple_term_batched(slab, adapter_w, precision, K, B, deltas):
    """mean over the K layer-steps of decouple_term(delta_c_k, delta_m_k) in ONE call (see _DecoupleBatchFn)."""
    return _DecoupleBatchFn.apply(adapter_w, PRECISIONS[precision], slab, int(K), int(B), *deltas)


def _is_dense(t: torch.Tensor) -> bool:
    """True when the tensor's elements tile one memory block without gaps or overlap (any dimension order)."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s > 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


class _MSELossFn(torch.autograd.Function):
    """scale * mean_{b,t} sum_{c,h,w} (pred - target)^2 with d/dpred produced in the same pass
    (base_measure.py:55-57, image_wise.py:25, loss_provider.py:48-51)."""

    @staticmethod
    def forward(ctx, pred, target, scale):
        require_gpu(pred, "mse_loss")
        if pred.ndim != 5 or target.ndim != 5:
            raise ValueError("Mean Squared Error (MSE) / L2 Loss expects 5-D inputs!")
        if pred.shape != target.shape:
            raise ValueError("Output images and target images are of different shape!")
        p = pred if _is_dense(pred) else pred.contiguous()
        # the sum runs over memory order, so the target only has to share the prediction's memory layout
        tg = target if (target.stride() == p.stride() and target.dtype == p.dtype) else torch.empty_like(p).copy_(target)
        L = _lib.lib()
        ws, ws_bytes = workspace(p.device, L.vpx_mse_loss_workspace_bytes)
        loss = torch.empty((), device=p.device)
        need = ctx.needs_input_grad[0]
        g = torch.empty_like(p) if need else None
        rc = L.vpx_mse_loss(ptr(p), ptr(tg), p.numel(), p.shape[0] * p.shape[1], float(scale), ptr(loss), ptr(g),
                            ptr(ws), ws_bytes, stream())
        check(rc, "vpx_mse_loss")
        if need:
            ctx.save_for_backward(g)
        ctx.need = need
        return loss

    @staticmethod
    def backward(ctx, dloss):
        if not ctx.need:
            return None, None, None
        (g,) = ctx.saved_tensors  # out of place: a second backward through the same node (retain_graph) stays correct
        return g * dloss, None, None


def mse_loss(pred, target, scale: float = 1.0):
    return _MSELossFn.apply(pred, target, scale)


def _frame_operands(pred, target, what):
    """(pred, target, layout) for the per-frame measure kernels: [B,T] dense frames whose elements lie in the reference's order
    (LAYOUT_NCHW) or channels-last (LAYOUT_NHWC). A prediction in either form is used as it is, anything else is made contiguous;
    the target is brought to the prediction's strides, as in _MSELossFn."""
    require_gpu(pred, what)
    if pred.ndim != 5 or target.ndim != 5:
        raise ValueError(f"{what} expects 5-D inputs!")
    if pred.shape != target.shape:
        raise ValueError("Output images and target images are of different shape!")
    if pred.is_contiguous():
        p, layout = pred, _lib.LAYOUT_NCHW
    elif is_channels_last(pred):
        p, layout = pred, _lib.LAYOUT_NHWC
    else:
        p, layout = pred.contiguous(), _lib.LAYOUT_NCHW
    tg = target if (target.stride() == p.stride() and target.dtype == p.dtype and target.device == p.device) else torch.empty_like(p).copy_(target)
    return p, tg, layout


class _PixelMeasuresFn(torch.autograd.Function):
    """[3, B, T] per-frame sums of d^2, |d| and smooth-L1(d), d = pred - target (image_wise.py:19-71 before their reductions). The
    backward is ONE launch on the incoming cotangent table, whatever mix of MSE / L1 / SmoothL1 / PSNR terms produced it."""

    @staticmethod
    def forward(ctx, pred, target):
        p, tg, _ = _frame_operands(pred, target, "pixel_measures")
        B, T = p.shape[:2]
        L = _lib.lib()
        ws, ws_bytes = workspace(p.device, L.vpx_pixel_measures_workspace_bytes, B * T, p[0, 0].numel())
        sums = torch.empty(3, B, T, device=p.device, dtype=torch.float64)   # (a PSNR term takes the logarithm of these)
        check(L.vpx_pixel_measures_fwd(ptr(p), ptr(tg), B * T, p[0, 0].numel(), ptr(sums), ptr(ws), ws_bytes, stream()), "vpx_pixel_measures_fwd")
        ctx.save_for_backward(p, tg)
        return sums

    @staticmethod
    def backward(ctx, dsums):
        if not ctx.needs_input_grad[0]:
            return None, None
        p, tg = ctx.saved_tensors
        B, T = p.shape[:2]
        g = torch.empty_like(p)   # out of place: a second backward through the same node (retain_graph) stays correct
        dsums = dsums.float().contiguous()
        check(_lib.lib().vpx_pixel_measures_bwd(ptr(p), ptr(tg), ptr(dsums), B * T, p[0, 0].numel(), ptr(g), stream()), "vpx_pixel_measures_bwd")
        return g, None


def pixel_measures(pred, target):
    """[3, B, T] float64: per-frame sums over (c,h,w) of (pred - target)^2, |pred - target| and smooth-L1(pred - target)."""
    return _PixelMeasuresFn.apply(pred, target)


class _SSIMFramesFn(torch.autograd.Function):
    """[B, T] SSIM of every frame (piqa's SSIM() defaults on clamp((x+1)/2, 0, 1), image_wise.py:111-117); the backward recomputes
    the derivative maps from the inputs, nothing but the inputs is saved."""

    @staticmethod
    def forward(ctx, pred, target):
        p, tg, layout = _frame_operands(pred, target, "ssim_frames")
        B, T, C, H, W = p.shape
        L = _lib.lib()
        nbytes = workspace_bytes(L.vpx_ssim_workspace_bytes, B * T, H, W)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=p.device)   # (0: the launch reports the bad shape)
        out = torch.empty(B, T, device=p.device)
        check(L.vpx_ssim_fwd(ptr(p), ptr(tg), B * T, C, H, W, layout, ptr(out), ptr(ws), nbytes, stream()), "vpx_ssim_fwd")
        ctx.save_for_backward(p, tg)
        ctx.layout = layout
        return out

    @staticmethod
    def backward(ctx, dssim):
        if not ctx.needs_input_grad[0]:
            return None, None
        p, tg = ctx.saved_tensors
        B, T, C, H, W = p.shape
        g = torch.empty_like(p)
        dssim = dssim.contiguous()
        check(_lib.lib().vpx_ssim_bwd(ptr(p), ptr(tg), ptr(dssim), B * T, C, H, W, ctx.layout, ptr(g), stream()), "vpx_ssim_bwd")
        return g, None


def ssim_frames(pred, target):
    """[B, T]: SSIM of each predicted frame against its target frame (3-channel frames of at least 11x11)."""
    return _SSIMFramesFn.apply(pred, target)


# ---- LPIPS on an AlexNet trunk (csrc/lpips.hip); feature maps are channels-last [N, h, w, C]. lpips_frames is the evaluation call (forward
# only), lpips_frames_diff the training call (gradient to the prediction) ---------------------------------------------------------------
LPIPS_MIN_SIDE = 31   # below it the third tap has no pixel
LPIPS_CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))   # torchvision's AlexNet.features
LPIPS_KEYS = tuple(f"conv{i}.weight" for i in range(1, 6)) + tuple(f"conv{i}.bias" for i in range(1, 6)) + tuple(f"lin{i}.weight" for i in range(1, 6))
LPIPS_SHAPES = dict(zip(LPIPS_KEYS, LPIPS_CONV_SHAPES + tuple((s[0],) for s in LPIPS_CONV_SHAPES) * 2))


def _lpips_operand(t, what, name, shape=None):
    require_gpu(t, what)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.contiguous()


def lpips_stem(x, w, bias, x1=None):
    """[N, Ho, Wo, 64] channels-last: ReLU(conv(norm(x), w, stride 4, padding 2) + bias) of x [N,3,H,W] in the model's range (and of the
    images of x1 behind them), norm = ImageNet normalisation of clamp((x+1)/2, 0, 1); the padding ring is zero in normalised space."""
    what = "lpips_stem"
    if x.ndim != 4 or x.shape[1] != 3 or (x1 is not None and x1.shape[1:] != x.shape[1:]):
        raise ValueError(f"{what}: expected [N,3,H,W] images of one size")
    x = _lpips_operand(x, what, "x")
    x1 = None if x1 is None else _lpips_operand(x1, what, "x1")
    w, bias = _lpips_operand(w, what, "w", LPIPS_CONV_SHAPES[0]), _lpips_operand(bias, what, "bias", (64,))
    n0, n1, (H, W) = x.shape[0], 0 if x1 is None else x1.shape[0], x.shape[2:]
    L = _lib.lib()
    ws, ws_bytes = workspace(x.device, L.vpx_lpips_stem_workspace_bytes)
    y = torch.empty(n0 + n1, max((H + 4 - 11) // 4 + 1, 0), max((W + 4 - 11) // 4 + 1, 0), 64, device=x.device)
    check(L.vpx_lpips_stem_fwd(ptr(x), ptr(x1), n0, n1, H, W, ptr(w), ptr(bias), ptr(y), ptr(ws), ws_bytes, stream()), "vpx_lpips_stem_fwd")
    return y


def lpips_maxpool(x):
    """[N, (h-3)//2+1, (w-3)//2+1, C]: 3x3 stride-2 max-pool (floor mode, no padding) of a channels-last map [N, h, w, C]."""
    if x.ndim != 4:
        raise ValueError("lpips_maxpool: expected a channels-last map [N, h, w, C]")
    x = _lpips_operand(x, "lpips_maxpool", "x")
    N, h, w, C = x.shape
    y = torch.empty(N, max((h - 3) // 2 + 1, 0), max((w - 3) // 2 + 1, 0), C, device=x.device)
    check(_lib.lib().vpx_lpips_maxpool_fwd(ptr(x), ptr(y), N, h, w, C, stream()), "vpx_lpips_maxpool_fwd")
    return y


def lpips_head(fx, fy, w, table=None):
    """table [N] (float64; zeros when not given) += mean over the pixels of sum_c w[c] (fx / (|fx| + 1e-10) - fy / (|fy| + 1e-10))^2 for
    channels-last feature maps fx, fy [N, h, w, C], |f| the channel norm at a pixel."""
    what = "lpips_head"
    if fx.ndim != 4 or fx.shape != fy.shape:
        raise ValueError(f"{what}: expected two channels-last maps [N, h, w, C] of one shape")
    fx, fy = _lpips_operand(fx, what, "fx"), _lpips_operand(fy, what, "fy")
    N, h, wd, C = fx.shape
    w = _lpips_operand(w, what, "w", (C,))
    if table is None:
        table = torch.zeros(N, device=fx.device, dtype=torch.float64)
    elif table.dtype != torch.float64 or tuple(table.shape) != (N,) or not table.is_contiguous() or table.device != fx.device:
        raise ValueError(f"{what}: table must be a contiguous float64 tensor of shape ({N},) on the maps' device")
    L = _lib.lib()
    ws, ws_bytes = workspace(fx.device, L.vpx_lpips_head_workspace_bytes, N, h * wd)
    check(L.vpx_lpips_head_fwd(ptr(fx), ptr(fy), ptr(w), N, h * wd, C, ptr(table), ptr(ws), ws_bytes, stream()), "vpx_lpips_head_fwd")
    return table


def lpips_frames(pred, target, weights):
    """[B, T] float64: LPIPS of each predicted frame against its target frame on an AlexNet trunk. pred, target: [B, T, 3, H, W] in the
    model's range, H, W >= 31. weights: {key: device tensor} over LPIPS_KEYS (measure.register_lpips_weights builds it). Prediction and
    target run through the trunk as one batch. FORWARD ONLY: the backward is not implemented, a prediction that requires grad under grad
    mode raises NotImplementedError (use torch.no_grad() or detach)."""
    what = "lpips_frames"
    B, T, C, H, W = _lpips_frames_shape(what, pred, target)
    if needs_grad(pred, target):
        raise NotImplementedError(f"{what}: the backward of LPIPS is not implemented in this build (forward only): evaluate it under "
                                  f"torch.no_grad() or on detached tensors")
    p, tg, params = _lpips_frames_operands(what, pred, target, weights)
    L = _lib.lib()
    ws, ws_bytes = workspace(p.device, L.vpx_lpips_workspace_bytes, B * T, H, W)
    table = torch.empty(B, T, device=p.device, dtype=torch.float64)
    check(L.vpx_lpips_fwd(ptr(p), ptr(tg), B * T, C, H, W, ptr_array(params), ptr(table), ptr(ws), ws_bytes, stream()), "vpx_lpips_fwd")
    return table


def _lpips_frames_shape(what, pred, target):
    if pred.ndim != 5 or target.ndim != 5:
        raise ValueError(f"{what} expects 5-D inputs!")
    if pred.shape != target.shape:
        raise ValueError("Output images and target images are of different shape!")
    B, T, C, H, W = pred.shape
    if C != 3:
        raise ValueError(f"{what} needs 3-channel images with the channels at dim 2")
    if H < LPIPS_MIN_SIDE or W < LPIPS_MIN_SIDE:
        raise ValueError(f"{what} needs images of at least {LPIPS_MIN_SIDE}x{LPIPS_MIN_SIDE} pixels (below that the third tap has no pixel)")
    return B, T, C, H, W


def _lpips_frames_operands(what, pred, target, weights):
    p, tg = _lpips_operand(pred, what, "pred"), _lpips_operand(target, what, "target")
    params = [_lpips_operand(weights[k], what, k, LPIPS_SHAPES[k]) for k in LPIPS_KEYS]
    if any(t.device != p.device for t in params + [tg]):
        raise ValueError(f"{what}: prediction, target and weights must live on one device")
    return p, tg, params


class _LPIPSFramesFn(torch.autograd.Function):
    """lpips_frames_diff: the forward keeps the five taps of both halves of the batch in a reserve, the backward runs from them. The
    gradient goes to the prediction alone."""

    @staticmethod
    def forward(ctx, pred, target, weights):
        what = "lpips_frames_diff"
        p, tg, params = _lpips_frames_operands(what, pred, target, weights)
        B, T, C, H, W = p.shape
        L = _lib.lib()
        ws, ws_bytes = workspace(p.device, L.vpx_lpips_workspace_bytes, B * T, H, W)
        reserve, reserve_bytes = workspace(p.device, L.vpx_lpips_reserve_bytes, B * T, H, W)
        table = torch.empty(B, T, device=p.device, dtype=torch.float64)
        check(L.vpx_lpips_fwd_train(ptr(p), ptr(tg), B * T, C, H, W, ptr_array(params), ptr(table), ptr(reserve), reserve_bytes, ptr(ws), ws_bytes,
                                    stream()), "vpx_lpips_fwd_train")
        ctx.save_for_backward(p, reserve, *params)
        return table

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dtable):
        p, reserve, *params = ctx.saved_tensors
        B, T, C, H, W = p.shape
        L = _lib.lib()
        ws, ws_bytes = workspace(p.device, L.vpx_lpips_bwd_workspace_bytes, B * T, H, W)
        g = torch.empty_like(p)   # out of place: a second backward through the same node (retain_graph) stays correct
        dtable = dtable.to(torch.float64).contiguous()
        check(L.vpx_lpips_bwd(ptr(p), ptr_array(params), ptr(reserve), ptr(dtable), B * T, C, H, W, ptr(g), ptr(ws), ws_bytes, stream()),
              "vpx_lpips_bwd")
        return g, None, None


def lpips_frames_diff(pred, target, weights):
    """lpips_frames as a training loss: the same [B, T] float64 table, bit for bit, differentiable ONCE with respect to `pred`. The
    weights never receive a gradient (the trunk is frozen) and a target that requires grad raises NotImplementedError. A call whose
    prediction requires grad keeps the five taps of the 2 B T images until its backward has run; without grad it is lpips_frames."""
    what = "lpips_frames_diff"
    B, T, C, H, W = _lpips_frames_shape(what, pred, target)
    if needs_grad(target):
        raise NotImplementedError(f"{what}: the gradient with respect to the target is not implemented (the gradient goes to the prediction)")
    if not needs_grad(pred):
        return lpips_frames(pred, target, weights)
    return _LPIPSFramesFn.apply(pred, target, weights)


def lpips_head_bwd(fx, fy, w, dtable, incoming=None):
    """[N, h, w, C] float32: the gradient with respect to the PRE-activation of the tap fx (channels-last, as lpips_head takes it) of
    sum_i dtable[i] * lpips_head(fx, fy, w)[i], plus `incoming` (the gradient arriving from the next layer), times the mask fx > 0.
    dtable: [N] float64 on the maps' device."""
    what = "lpips_head_bwd"
    if fx.ndim != 4 or fx.shape != fy.shape or (incoming is not None and incoming.shape != fx.shape):
        raise ValueError(f"{what}: expected channels-last maps [N, h, w, C] of one shape")
    fx, fy = _lpips_operand(fx, what, "fx"), _lpips_operand(fy, what, "fy")
    incoming = None if incoming is None else _lpips_operand(incoming, what, "incoming")
    N, h, wd, C = fx.shape
    w = _lpips_operand(w, what, "w", (C,))
    if dtable.dtype != torch.float64 or tuple(dtable.shape) != (N,) or not dtable.is_contiguous() or dtable.device != fx.device:
        raise ValueError(f"{what}: dtable must be a contiguous float64 tensor of shape ({N},) on the maps' device")
    dz = torch.empty_like(fx)
    check(_lib.lib().vpx_lpips_head_bwd(ptr(fx), ptr(fy), ptr(w), ptr(dtable), ptr(incoming), N, h * wd, C, ptr(dz), stream()), "vpx_lpips_head_bwd")
    return dz


def lpips_maxpool_bwd(x, dy):
    """[N, h, w, C]: the gradient of lpips_maxpool at its input x from dy [N, (h-3)//2+1, (w-3)//2+1, C]. Among tied maxima of a window the
    first in row-major order takes the gradient (torch's CPU rule)."""
    what = "lpips_maxpool_bwd"
    if x.ndim != 4:
        raise ValueError(f"{what}: expected a channels-last map [N, h, w, C]")
    x = _lpips_operand(x, what, "x")
    N, h, w, C = x.shape
    dy = _lpips_operand(dy, what, "dy", (N, max((h - 3) // 2 + 1, 0), max((w - 3) // 2 + 1, 0), C))
    dx = torch.empty_like(x)
    check(_lib.lib().vpx_lpips_maxpool_bwd(ptr(x), ptr(dy), ptr(dx), N, h, w, C, stream()), "vpx_lpips_maxpool_bwd")
    return dx


def lpips_stem_bwd(x, w, dz):
    """[N, 3, H, W]: the gradient of lpips_stem at the images x from dz [N, Ho, Wo, 64], the gradient of tap 1's pre-activation; the clamp
    passes the gradient where 0 <= (x + 1) / 2 <= 1 in float32, bounds included."""
    what = "lpips_stem_bwd"
    if x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"{what}: expected [N,3,H,W] images of one size")
    x = _lpips_operand(x, what, "x")
    w = _lpips_operand(w, what, "w", LPIPS_CONV_SHAPES[0])
    N, (H, W) = x.shape[0], x.shape[2:]
    dz = _lpips_operand(dz, what, "dz", (N, max((H + 4 - 11) // 4 + 1, 0), max((W + 4 - 11) // 4 + 1, 0), 64))
    L = _lib.lib()
    ws, ws_bytes = workspace(x.device, L.vpx_lpips_stem_workspace_bytes)
    dx = torch.empty_like(x)
    check(L.vpx_lpips_stem_bwd(ptr(x), ptr(w), ptr(dz), N, H, W, ptr(dx), ptr(ws), ws_bytes, stream()), "vpx_lpips_stem_bwd")
    return dx


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """One torch.optim.Adam update of flat fp32 buckets, in place (vpsuite.py:353; torch/optim/adam.py semantics)."""
    require_gpu(param, "adam_step")
    for t in (param, grad, exp_avg, exp_avg_sq):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == param.numel()):
            raise ValueError("adam_step: buckets must be contiguous float32 GPU tensors of equal size")
    # The shapes and values are fine here (check() keeps ValueError for those, as the reference does): the caller broke the op's contract
    # — a view the kernel's four-float moves cannot address, a step counter that was never advanced — which this package reports as
    # VpxError (cf. require_gpu). Asked here so that the type does not depend on the library's one code for every bad argument; the
    # library keeps its own check for callers of the C ABI.
    if any(t.data_ptr() & 15 for t in (param, grad, exp_avg, exp_avg_sq)):
        raise _lib.VpxError("adam_step: buckets must be 16-byte aligned (the kernel moves four floats at a time)")
    if int(step) < 1:
        raise _lib.VpxError(f"adam_step: step counts from 1 (got {step}): the bias corrections divide by 1 - beta^step")
    rc = _lib.lib().vpx_adam_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
                                  float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                  float(grad_scale), stream())
    check(rc, "vpx_adam_step")


_grad_stats_ws = {}   # (device, stream) -> the partial sums' workspace: a few KB, kept so that a training step allocates nothing


def grad_stats(grad, grad_scale=1.0, out=None):
    """Norm, largest magnitude and non-finite count of `grad_scale * grad` in one deterministic pass: a float64 GPU tensor of 4
    elements (include/vpx.h: vpx_grad_stats), `out` if given (element 3, adam_step_clipped's skipped-step count, is left alone; a new
    tensor starts it at 0). Nothing is read back: looking at the result is the caller's host sync."""
    require_gpu(grad, "grad_stats")
    if not (grad.is_contiguous() and grad.numel() > 0):
        raise ValueError("grad_stats: the gradient must be a contiguous, non-empty float32 GPU tensor")
    if not float(grad_scale) >= 0.0:
        raise ValueError(f"grad_stats: grad_scale must not be negative or NaN (got {grad_scale})")
    if out is None:
        out = torch.zeros(4, dtype=torch.float64, device=grad.device)
    elif not (out.is_cuda and out.device == grad.device and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 4):
        raise ValueError("grad_stats: out must be a contiguous float64 tensor of 4 elements on the gradient's device")
    L = _lib.lib()
    s = stream()
    ws = _grad_stats_ws.get((grad.device, s.value))
    if ws is None:
        ws = _grad_stats_ws[(grad.device, s.value)] = workspace(grad.device, L.vpx_grad_stats_workspace_bytes)
    check(L.vpx_grad_stats(ptr(grad), grad.numel(), float(grad_scale), ptr(out), ptr(ws[0]), ws[1], s), "vpx_grad_stats")
    return out


def adam_step_clipped(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                      stats=None, max_norm=0.0, clip_value=0.0, skip_nonfinite=False):
    """adam_step with the gradient clipped on the way in: by norm (clip_grad_norm_'s coefficient from `stats`, grad_stats's result of
    the SAME grad_scale, read on the device), then by value (clip_grad_value_), and the whole step left out when `skip_nonfinite` and
    the statistics count a non-finite element (stats[3] counts those steps; the caller's step count advances all the same).
    `stats` may be None for value clipping alone. include/vpx.h: vpx_adam_step_clipped."""
    require_gpu(param, "adam_step_clipped")
    for t in (param, grad, exp_avg, exp_avg_sq):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == param.numel()):
            raise ValueError("adam_step_clipped: buckets must be contiguous float32 GPU tensors of equal size")
    for name, val in (("max_norm", max_norm), ("clip_value", clip_value), ("grad_scale", grad_scale)):
        if not float(val) >= 0.0:
            raise ValueError(f"adam_step_clipped: {name} must not be negative or NaN (got {val})")
    if stats is None:
        if float(max_norm) > 0.0 or skip_nonfinite:
            raise ValueError("adam_step_clipped: max_norm and skip_nonfinite read the gradient statistics: pass stats=grad_stats(grad, grad_scale)")
    elif not (stats.is_cuda and stats.device == param.device and stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 4):
        raise ValueError("adam_step_clipped: stats must be grad_stats's float64 tensor of 4 elements on the buckets' device")
    # (the contract breaches adam_step reports as VpxError, for the same reason)
    if any(t.data_ptr() & 15 for t in (param, grad, exp_avg, exp_avg_sq)):
        raise _lib.VpxError("adam_step_clipped: buckets must be 16-byte aligned (the kernel moves four floats at a time)")
    if int(step) < 1:
        raise _lib.VpxError(f"adam_step_clipped: step counts from 1 (got {step}): the bias corrections divide by 1 - beta^step")
    rc = _lib.lib().vpx_adam_step_clipped(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
                                          float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                          float(grad_scale), ptr(stats), float(max_norm), float(clip_value), int(bool(skip_nonfinite)),
                                          stream())
    check(rc, "vpx_adam_step_clipped")


class STWorkspace:
    """Per-cell workspace that lets consecutive steps of one forward pass skip the weight repack
    (VPX_FLAG_WEIGHTS_PACKED): valid while the weights' version counters and the problem shape are unchanged."""

    def __init__(self):
        self.buf = None
        self.key = None
        self.bwd = None  # the backward's own holder (different workspace layout, transposed packs)

    def backward_holder(self):
        if self.bwd is None:
            self.bwd = STWorkspace()
        return self.bwd

    def get(self, nbytes, device, key):
        """Returns (buffer, packed_valid)."""
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.key = None
        valid = self.key == key
        self.key = key
        return self.buf, valid


_shadow_epoch = 0


def new_shadow_epoch():
    """Ends the life of every split-format shadow attached so far. A model calls this at the start of each forward pass: a shadow then
    only ever describes a tensor produced earlier in the SAME pass, inside the model's own time loop — memory no user code gets
    to write through an alias the version counter cannot see (`.data`, dlpack, a raw-pointer kernel) while the shadow lives."""
    global _shadow_epoch
    _shadow_epoch += 1


def _attach_shadow(t, buf):
    """Records `buf` as the split-format copy of the tensor `t` a library call just wrote: (buffer, version, address, shape, epoch)."""
    t._vpx_sp = (buf, t._version, t.data_ptr(), tuple(t.shape), _shadow_epoch)


def invalidate_shadow(t):
    """Drops a tensor's split-format shadow. Code that writes into a tensor WITHOUT bumping its version counter — `.data.copy_()`,
    a raw-pointer kernel, dlpack aliases — must call this (or `ops.clear_layout_cache()` for everything)."""
    if getattr(t, "_vpx_sp", None) is not None:
        t._vpx_sp = None


def _shadow_of(t, tl, channels):
    """The split-format copy a previous library call attached to tensor `t`, if it still describes the memory `tl` that is about to
    be handed to the library as an operand with `channels` channels: same shadow epoch (new_shadow_epoch), same tensor version, same
    address, same device and the same logical shape [B, channels, H, W] as when it was attached. The attribute lives on the very
    object the library returned — views, clones and `.data` aliases never carry it."""
    sp = getattr(t, "_vpx_sp", None)
    if sp is None:
        return None
    buf, version, addr, shape, epoch = sp
    if epoch != _shadow_epoch or version != t._version or addr != tl.data_ptr() or buf.device != tl.device or shape != tuple(tl.shape) or shape[1] != channels \
            or buf.numel() != tl.numel():
        return None
    return buf


class STWeightBank:
    """Deferred weight gradients of ONE ST-LSTM cell over the T steps of one training forward (include/vpx.h: dg8_out,
    vpx_stlstm_wgrad_batch). The owner (PredRNN_V2.forward) lays the cell's operands out as dense time-major slabs in the split operand
    format and hands every step its slots explicitly:
        g       [T][B*HW*8Ch]   dG8 of step t — written by the step's backward
        sources five tensors, each the slot of step 0 of a slab whose slot t (stride = one slot) is that operand of step t:
                x, h, m (inputs of the step) and c_new, m_new (its outputs)
    `weights()` passes the five weight tensors through an identity autograd node; the steps take THOSE. Their backward deposits dG8 and
    returns no weight gradient; when autograd reaches the identity node — every step of the cell has run its backward by then — `run()`
    computes the five gradients of all T steps in one launch and returns them as the node's input gradients."""

    def __init__(self, weights5, B, Cin, Ch, H, W, k, T, precision):
        self.w5 = tuple(weights5)
        self.geo = (int(B), int(Cin), int(Ch), int(H), int(W), int(k), int(T), int(precision))
        dev = self.w5[0].device
        self.g = torch.empty(T, B * H * W * 8 * Ch, dtype=torch.float32, device=dev)
        self.sources = None
        self.deposited = set()

    @staticmethod
    def available(B, Cin, Ch, H, W, k, precision):
        d = STLSTMDesc(B, Cin, Ch, H, W, k, 0, _lib.LAYOUT_NHWC, PRECISIONS[precision], _lib.FLAG_SAVE_FOR_BWD)
        L = _lib.lib()
        return bool(L.vpx_stlstm_defers_wgrad(ctypes.byref(d))) and bool(L.vpx_stlstm_uses_split(ctypes.byref(d)))

    def set_sources(self, x, h, m, c_new, m_new):
        """Each argument: the slot-0 tensor (1-D, one slot long) of the operand's slab; slots t = 1 .. T-1 follow it in memory."""
        self.sources = (x, h, m, c_new, m_new)

    def weights(self):
        return _BankFn.apply(self, *self.w5)

    def run(self):
        B, Cin, Ch, H, W, k, T, prec = self.geo
        if self.sources is None:
            raise _lib.VpxError("STWeightBank: set_sources was never called")
        for t in range(T):
            if t not in self.deposited:     # a step whose outputs reached no loss: its dG8 is zero
                self.g[t].zero_()
        d = STLSTMDesc(T * B, Cin, Ch, H, W, k, 0, _lib.LAYOUT_NHWC, prec, _lib.FLAG_SAVE_FOR_BWD)
        L = _lib.lib()
        nb = L.vpx_stlstm_wgrad_batch_workspace_bytes(ctypes.byref(d))
        if nb == 0:
            raise _lib.VpxError("STWeightBank: vpx_stlstm_wgrad_batch is not available for this cell")
        ws = torch.empty(nb, dtype=torch.uint8, device=self.g.device)
        dWs = [torch.empty_like(w) for w in self.w5]
        check(L.vpx_stlstm_wgrad_batch(ctypes.byref(d), ptr(self.g), ptr_array(self.sources), *[ptr(g) for g in dWs], ptr(ws), nb, stream()), "vpx_stlstm_wgrad_batch")
        self.deposited.clear()
        return dWs


class _BankFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bank, *w5):
        ctx.bank = bank
        ctx.set_materialize_grads(False)
        return tuple(w.view_as(w) for w in w5)

    @staticmethod
    def backward(ctx, *grads):
        sync_determinism()
        dWs = ctx.bank.run()
        for i, g in enumerate(grads):       # (a consumer that did not defer — none today — adds its gradient the ordinary way)
            if g is not None:
                dWs[i] = dWs[i] + g
        return (None, *dWs)


class _STLSTMStepFn(torch.autograd.Function):
    """(h_new, c_new, m_new, delta_c, delta_m) = ST-LSTM cell step (predrnn.py:57-83) in one library call.
    `ln` = () or the 8 LayerNorm tensors (x_gamma, x_beta, h_gamma, h_beta, m_gamma, m_beta, o_gamma, o_beta)."""

    @staticmethod
    def forward(ctx, x, h, c, m, Wx, Wh, Wm, Wo, Wlast, precision, need_grad, wsholder, use_shadows, slots, delta_out, *ln):
        require_gpu(x, "stlstm_step")
        dev = x.device
        B, Cin, H, Wd = x.shape
        Ch = h.shape[1]
        k = int(Wx.shape[-1])
        xs, hs, cs, ms = (to_channels_last(t) for t in (x, h, c, m))
        W5 = [w.contiguous() for w in (Wx, Wh, Wm, Wo, Wlast)]
        lnc = [t.contiguous() for t in ln]
        use_ln = len(lnc) == 8
        flags = _lib.FLAG_SAVE_FOR_BWD if need_grad else 0
        d = STLSTMDesc(B, Cin, Ch, H, Wd, k, int(use_ln), _lib.LAYOUT_NHWC, precision, flags)
        L = _lib.lib()
        ws_bytes = workspace_bytes(L.vpx_stlstm_workspace_bytes, ctypes.byref(d), unsupported=NOT_IMPLEMENTED)
        key = (B, Cin, Ch, H, Wd, k, precision, flags, _det_state, _kernel_options(), tuple((w.data_ptr(), w._version) for w in W5),
               tuple((t.data_ptr(), t._version) for t in lnc))
        if wsholder is not None:
            ws, packed = wsholder.get(ws_bytes, dev, key)
        else:
            ws, packed = torch.empty(ws_bytes, dtype=torch.uint8, device=dev), False
        if packed:
            d.flags |= _lib.FLAG_WEIGHTS_PACKED
        reserve, rs_bytes = reserve_buffer(dev, L.vpx_stlstm_reserve_bytes, d)
        outs = [new_channels_last((B, Ch, H, Wd), dev) for _ in range(3)]
        if delta_out is not None:   # the caller's slab slots (decouple_term_batched: one decoupling tail over all the steps of a pass)
            for t in delta_out:
                if tuple(t.shape) != (B, Ch, H, Wd) or not is_channels_last(t) or t.dtype != torch.float32 or t.device != dev:
                    raise ValueError("stlstm_step: delta_out must hold two channels-last float32 [B, Ch, H, W] tensors on the step's device")
            outs += [delta_out[0], delta_out[1]]
        else:
            dd = new_channels_last((2 * B, Ch, H, Wd), dev)  # delta_c | delta_m adjacent: the decoupling tail runs the pair as one conv
            outs += [dd[:B], dd[B:]]
        ln_arr = ptr_array(lnc) if use_ln else None
        # split-format shadows (vpx.h): operands a previous step left in the kernels' operand format are handed back instead of being
        # converted again (h_new is the next step's h and the next layer's x, m_new the next layer's m), and this step's h_new / c_new /
        # m_new come back with shadows of their own
        sp_in, sp_out, shadows = [None] * 5, None, None
        bank = None
        if slots is not None:
            # explicit operand slots (STWeightBank mode): the owner's slabs hold x, h, m in the split format and receive h_new, c_new, m_new
            bank, bank_t, slot_in, slot_out, convert_x = slots
            if use_ln or not need_grad or not L.vpx_stlstm_uses_split(ctypes.byref(d)):
                raise _lib.VpxError("stlstm_step: operand slots need the split-operand kernels in a call that saves for the backward")
            sp_in[:3] = list(slot_in)
            if convert_x:   # an input without a split copy (the first layer's frame): converted into its slot of the owner's x slab
                check(L.vpx_split_convert(ptr(xs), ptr(sp_in[0]), B * H * Wd, Cin, stream()), "vpx_split_convert")
            sp_out = list(slot_out)
            for buf, n in zip(sp_in[:3] + sp_out, (Cin, Ch, Ch, Ch, Ch, Ch)):
                if buf.numel() != B * H * Wd * n or not buf.is_contiguous() or buf.dtype != torch.float32:
                    raise ValueError("stlstm_step: an operand slot does not hold B*H*W*C elements")
        elif use_shadows and not use_ln and L.vpx_stlstm_uses_split(ctypes.byref(d)):
            sp_in[:3] = [_shadow_of(x, xs, Cin), _shadow_of(h, hs, Ch), _shadow_of(m, ms, Ch)]
            sp_out = [torch.empty(B * H * Wd * Ch, dtype=torch.float32, device=dev) for _ in range(3)]
        if sp_out is not None:
            shadows = _lib.STLSTMShadows(ptr_array(sp_in), ptr_array(sp_out), None)
        with _profiled("stlstm_fwd", 4, lambda: stlstm_algorithmic_work(B, Cin, Ch, H, Wd, k)):
            rc = L.vpx_stlstm_step_fwd_ex(ctypes.byref(d), ptr(xs), ptr(hs), ptr(cs), ptr(ms), *[ptr(w) for w in W5], ln_arr,
                                          *[ptr(o) for o in outs], ptr(reserve), rs_bytes, ptr(ws), ws_bytes, stream(),
                                          None if shadows is None else ctypes.byref(shadows))
            check(rc, "vpx_stlstm_step_fwd")
        if sp_out is not None and bank is None:
            for t, buf in zip(outs[:3], sp_out):
                _attach_shadow(t, buf)
        if need_grad:
            ctx.sp = None if sp_out is None else (sp_in[0], sp_in[1], sp_in[2], sp_out[1], sp_out[2])   # x, h, m, c_new, m_new
            ctx.save_for_backward(xs, hs, cs, ms, outs[1], outs[2], *W5, reserve, *lnc)
            d.flags = flags
            ctx.desc = d
            ctx.rs_bytes = rs_bytes
            ctx.use_ln = use_ln
            ctx.bwd_holder = wsholder.backward_holder() if (wsholder is not None and not use_ln) else None
            ctx.wkey = key
            ctx.bank = None if bank is None else (bank, bank_t)
        return tuple(outs)

    @staticmethod
    def backward(ctx, dh_new, dc_new, dm_new, ddc, ddm):
        sync_determinism()
        saved = ctx.saved_tensors
        xs, hs, cs, ms, c_new, m_new, Wx, Wh, Wm, Wo, Wlast, reserve = saved[:12]
        lnc = list(saved[12:])
        d = ctx.desc
        dev = xs.device
        L = _lib.lib()
        gin = [None if g is None else to_channels_last(g) for g in (dh_new, dc_new, dm_new, ddc, ddm)]
        needs = ctx.needs_input_grad
        dx = new_channels_last(tuple(xs.shape), dev) if needs[0] else None
        dh = new_channels_last(tuple(hs.shape), dev) if needs[1] else None
        dc = new_channels_last(tuple(cs.shape), dev) if needs[2] else None
        dm = new_channels_last(tuple(ms.shape), dev) if needs[3] else None
        bank = getattr(ctx, "bank", None)
        dWs = [torch.empty_like(w) if (needs[4 + i] and bank is None) else None for i, w in enumerate((Wx, Wh, Wm, Wo, Wlast))]
        dln = [torch.empty_like(t) if needs[15 + i] else None for i, t in enumerate(lnc)]
        ln_arr = ptr_array(lnc) if ctx.use_ln else None
        dln_arr = ptr_array(dln) if ctx.use_ln else None
        ws_bytes = L.vpx_stlstm_workspace_bytes(ctypes.byref(d))
        flags0 = d.flags
        if ctx.bwd_holder is not None and BWD_WEIGHT_PACK_REUSE:
            # (which transposed packs a call makes depends on the data gradients it is asked for)
            ws, packed = ctx.bwd_holder.get(ws_bytes, dev, (ctx.wkey, dx is not None, dh is not None, dm is not None, bank is not None))
            if packed:
                d.flags = flags0 | _lib.FLAG_WEIGHTS_PACKED
        else:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        shadows = None
        if getattr(ctx, "sp", None) is not None:   # the forward's split shadows: the weight-gradient kernel stages them as they are
            shadows = _lib.STLSTMShadows(ptr_array(ctx.sp), ptr_array((None,) * 3),
                                         None if bank is None else bank[0].g[bank[1]].data_ptr())
        rc = L.vpx_stlstm_step_bwd_ex(ctypes.byref(d), ptr(xs), ptr(hs), ptr(cs), ptr(ms), ptr(c_new), ptr(m_new), ptr(Wx),
                                      ptr(Wh), ptr(Wm), ptr(Wo), ptr(Wlast), ln_arr, ptr(reserve), ctx.rs_bytes,
                                      *[ptr(g) for g in gin], ptr(dx), ptr(dh), ptr(dc), ptr(dm), *[ptr(g) for g in dWs],
                                      dln_arr, ptr(ws), ws_bytes, stream(), None if shadows is None else ctypes.byref(shadows))
        d.flags = flags0
        check(rc, "vpx_stlstm_step_bwd")
        if bank is not None:
            bank[0].deposited.add(bank[1])
        return (dx, dh, dc, dm, *dWs, None, None, None, None, None, None, *dln)


def stlstm_algorithmic_work(B, Cin, Ch, H, W, k, dt=4):
    """flops = 2*[(7Ch*Cin + 9Ch^2)*k^2 + 2Ch^2]*H*W per sample; bytes = dt*H*W*(Cin + 3Ch + 5Ch) per
    sample + the weights once per step."""
    flops = 2.0 * ((7 * Ch * Cin + 9 * Ch * Ch) * k * k + 2 * Ch * Ch) * H * W * B
    nbytes = dt * H * W * (Cin + 8 * Ch) * B + dt * ((7 * Ch * Cin + 9 * Ch * Ch) * k * k + 2 * Ch * Ch)
    return flops, nbytes


def stlstm_step(x, h, c, m, Wx, Wh, Wm, Wo, Wlast, precision="f32", wsholder=None, ln=(), use_shadows=False, slots=None, delta_out=None):
    """ln: () or the 8 LayerNorm parameter tensors [C,H,W] (x_gamma, x_beta, h_.., m_.., o_..) of the LayerNorm variant.
    use_shadows: hand h_new / c_new / m_new out with split-format shadows and take the shadows of x / h / m where a previous step of
    the same shadow epoch attached them (no second conversion). Opt-in: the caller vouches that nothing writes those tensors behind
    the version counter's back between the steps (PredRNN_V2.forward: the tensors never leave its loop).
    slots: (bank, t, (x_sp, h_sp, m_sp), (h_new_sp, c_new_sp, m_new_sp), convert_x) — STWeightBank mode: the weights must be
    `bank.weights()`, the operands' split copies live in the owner's slabs (convert_x: x has none yet — converted into x_sp here), the
    weight gradients of the cell's steps are computed together when autograd reaches the bank.
    delta_out: (delta_c, delta_m) — caller tensors [B, Ch, H, W] (channels-last) the step writes its two deltas into instead of
    allocating them (slots of the slab `decouple_term_batched` reads)."""
    ln = tuple(ln)
    if len(ln) not in (0, 8):
        raise ValueError("stlstm_step: ln must hold 0 or 8 tensors")
    need_grad = needs_grad(x, h, c, m, Wx, Wh, Wm, Wo, Wlast, *ln)
    return _STLSTMStepFn.apply(x, h, c, m, Wx, Wh, Wm, Wo, Wlast, PRECISIONS[precision], need_grad, wsholder, bool(use_shadows), slots, delta_out, *ln)


class _LayerNormCHWFn(torch.autograd.Function):
    """nn.LayerNorm([C,H,W]) on a [B,C,H,W] tensor (channels-last memory) through the library's LayerNorm kernels (double-precision
    statistics over fixed chunks, explicit backward) — the action-conditional ST-LSTM cell's per-convolution normalisation
    (predrnn.py:105-135)."""

    @staticmethod
    def forward(ctx, x, weight, bias, need):
        require_gpu(x, "layer_norm_chw")
        xs = to_channels_last(x)
        B, C, H, Wd = xs.shape
        # keyed on the parameter itself (a `weight[None]` temporary is a new object every call and can never hit)
        g = _cached_channels_last(weight)
        b = _cached_channels_last(bias)
        L = _lib.lib()
        ws, ws_bytes = workspace(x.device, L.vpx_layernorm_workspace_bytes, B)
        y = new_channels_last((B, C, H, Wd), x.device)
        xhat = new_channels_last((B, C, H, Wd), x.device) if need else None
        stats = torch.empty(B, 2, device=x.device)
        check(L.vpx_layernorm_fwd(ptr(xs), ptr(g), ptr(b), ptr(y), ptr(xhat), ptr(stats), B, C * H * Wd, ptr(ws), ws_bytes, stream()),
              "vpx_layernorm_fwd")
        if need:
            ctx.save_for_backward(xhat, stats, g)
            ctx.wshape = tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        sync_determinism()
        xhat, stats, g = ctx.saved_tensors
        B, C, H, Wd = xhat.shape
        dys = to_channels_last(dy)
        L = _lib.lib()
        ws, ws_bytes = workspace(dy.device, L.vpx_layernorm_workspace_bytes, B)
        dx = new_channels_last((B, C, H, Wd), dy.device)
        dg = new_channels_last((1, C, H, Wd), dy.device)
        db = new_channels_last((1, C, H, Wd), dy.device)
        check(L.vpx_layernorm_bwd(ptr(dys), ptr(xhat), ptr(stats), ptr(g), ptr(dx), ptr(dg), ptr(db), B, H * Wd, C, ptr(ws), ws_bytes,
                                  stream()), "vpx_layernorm_bwd")
        return dx, dg.reshape(ctx.wshape), db.reshape(ctx.wshape), None


def layer_norm_chw(x, weight, bias, eps=1e-5):
    """F.layer_norm(x, [C,H,W], weight, bias, eps) for a [B,C,H,W] tensor, on the library's kernels (eps is fixed at 1e-5). No model
    calls it (the cells normalise inside their own library calls): it is the public form of vpx_layernorm_fwd/_bwd, covered by
    tests/test_gpu_norms.py. Whether x̂ is kept for a backward is decided here, where grad mode is visible: under torch.no_grad(), or
    when no operand requires a gradient, the forward writes no x̂ (the library's `xhat == NULL` form)."""
    if abs(float(eps) - 1e-5) > 1e-12:
        raise ValueError("layer_norm_chw: the library's LayerNorm kernels use eps = 1e-5 (nn.LayerNorm's default)")
    return _LayerNormCHWFn.apply(x, weight, bias, needs_grad(x, weight, bias))


class _ACSTStepFn(torch.autograd.Function):
    """(h_new, c_new, m_new, delta_c, delta_m) = action-conditional ST-LSTM cell step (predrnn.py:139-169) in ONE library call each
    way (vpx_acstlstm_step_fwd / _bwd): six biased convolutions, optional LayerNorms, the conv_h(h) * conv_a(a) product, both gate
    groups, the state updates and the output gate. `tensors` = the 12 parameters (conv_x, conv_h, conv_a, conv_m, conv_o, conv_last)
    x (weight, bias), then — with layer_norm — the 10 LayerNorm tensors (x, h, a, m, o) x (weight, bias)."""

    @staticmethod
    def forward(ctx, x, h, c, m, a, precision, forget_bias, *tensors):
        require_gpu(x, "acstlstm_step")
        dev = x.device
        B, Cin, H, Wd = x.shape
        Ch = h.shape[1]
        prm = [t.contiguous() for t in tensors[:12]]
        lnc = [t.contiguous() for t in tensors[12:]]
        if len(prm) != 12 or len(lnc) not in (0, 10):
            raise ValueError("acstlstm_step: 12 parameters, then either no or ten LayerNorm tensors")
        k = int(prm[0].shape[-1])
        need = any(ctx.needs_input_grad)
        d = _lib.ACSTLSTMDesc(B, Cin, Ch, H, Wd, k, int(bool(lnc)), precision, _lib.FLAG_SAVE_FOR_BWD if need else 0, float(forget_bias))
        L = _lib.lib()
        ws, ws_bytes = workspace(dev, L.vpx_acstlstm_workspace_bytes, ctypes.byref(d), unsupported=NOT_IMPLEMENTED)   # (none of its messages says so: ValueError)
        reserve, rs_bytes = reserve_buffer(dev, L.vpx_acstlstm_reserve_bytes, d)
        xs, hs, cs, ms, as_ = (to_channels_last(t) for t in (x, h, c, m, a))
        outs = [new_channels_last((B, Ch, H, Wd), dev) for _ in range(5)]
        p_arr = ptr_array(prm)
        ln_arr = ptr_array(lnc) if lnc else None
        check(L.vpx_acstlstm_step_fwd(ctypes.byref(d), ptr(xs), ptr(hs), ptr(cs), ptr(ms), ptr(as_), p_arr, ln_arr, *[ptr(o) for o in outs],
                                      ptr(reserve), rs_bytes, ptr(ws), ws_bytes, stream()), "vpx_acstlstm_step_fwd")
        if need:
            ctx.save_for_backward(xs, hs, cs, ms, as_, reserve, *prm, *lnc)
            ctx.desc, ctx.rs_bytes = d, rs_bytes
            ctx.set_materialize_grads(False)   # (an output the loss does not reach hands the backward None: NULL to the library, no zeros to read)
        return tuple(outs)

    @staticmethod
    def backward(ctx, dh_new, dc_new, dm_new, ddc, ddm):
        sync_determinism()
        saved = ctx.saved_tensors
        xs, hs, cs, ms, as_, reserve = saved[:6]
        prm, lnc = list(saved[6:18]), list(saved[18:])
        d, dev, L = ctx.desc, xs.device, _lib.lib()
        gin = [None if g is None else to_channels_last(g) for g in (dh_new, dc_new, dm_new, ddc, ddm)]
        if gin[0] is None:
            gin[0] = torch.zeros_like(hs)
        needs = ctx.needs_input_grad
        dins = [new_channels_last(tuple(t.shape), dev) if needs[i] else None for i, t in enumerate((xs, hs, cs, ms, as_))]
        dprm = [torch.empty_like(t) if needs[7 + i] else None for i, t in enumerate(prm)]
        dln = [torch.empty_like(t) if needs[19 + i] else None for i, t in enumerate(lnc)]
        p_arr, dp_arr = ptr_array(prm), ptr_array(dprm)
        ln_arr = ptr_array(lnc) if lnc else None
        dln_arr = ptr_array(dln) if lnc else None
        ws, ws_bytes = workspace(dev, L.vpx_acstlstm_workspace_bytes, ctypes.byref(d))
        check(L.vpx_acstlstm_step_bwd(ctypes.byref(d), ptr(xs), ptr(hs), ptr(cs), ptr(ms), ptr(as_), p_arr, ln_arr, ptr(reserve), ctx.rs_bytes,
                                      *[ptr(g) for g in gin], *[ptr(t) for t in dins], dp_arr, dln_arr, ptr(ws), ws_bytes, stream()),
              "vpx_acstlstm_step_bwd")
        return (*dins, None, None, *dprm, *dln)


def acstlstm_step(x, h, c, m, a, params, ln=(), precision="f32", forget_bias=1.0):
    """One step of the action-conditional ST-LSTM cell; `params`: the 12 convolution tensors, `ln`: () or the 10 LayerNorm tensors."""
    return _ACSTStepFn.apply(x, h, c, m, a, PRECISIONS[precision], float(forget_bias), *params, *ln)


# ---- stored frames to a model-ready batch and back (csrc/frames.hip) ----
FRAME_DTYPES = {torch.uint8: _lib.FRAMES_U8, torch.uint16: _lib.FRAMES_U16, torch.float32: _lib.FRAMES_F32}


def _stored_source(who, name, t, dtypes, work):
    """`t`, the stored data of a gather, contiguous: a GPU tensor of one of the stored element types `dtypes`."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.VpxError(f"{who}: {name} must be a GPU tensor; {work} by a HIP kernel, there is no CPU fallback")
    if t.dtype not in dtypes:
        kinds = [str(d).split(".")[-1] for d in dtypes]
        raise ValueError(f"{who}: stored element type {t.dtype} is unknown ({', '.join(kinds[:-1])} and {kinds[-1]} are)")
    return t.contiguous()


def _boxed_sizes(who, frame_hw, Cs, crop_size, out_size, c_out, n_frames, seq_step):
    """(ch, cw, oh, ow, c_out) of a launch with one crop box: crop_size defaults to the frame, out_size to the crop, c_out to Cs."""
    ch, cw = frame_hw if crop_size is None else (int(s) for s in crop_size)
    oh, ow = (ch, cw) if out_size is None else (int(s) for s in out_size)
    c_out = Cs if c_out is None else int(c_out)
    if min(ch, cw, oh, ow, n_frames, seq_step) < 1:
        raise ValueError(f"{who}: every size must be >= 1 (crop {ch}x{cw}, output {oh}x{ow}, {n_frames} frames, step {seq_step})")
    return ch, cw, oh, ow, c_out


def _gather_out(who, out, shape, device):
    """The destination of a preprocess launch: `out` if it is a contiguous float32 GPU tensor of `shape`, a new one for None."""
    if out is None:
        if min(shape) < 1:
            raise ValueError(f"{who}: empty output {shape}")
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError(f"{who}: out must be a contiguous float32 GPU tensor {shape}")
    return out


def _host_table(table, cols, name="table", shape=None, min_cols=None):
    """An integer host table of at least one row and `cols` (or min_cols ... cols) columns, as an int64 array."""
    import numpy as np
    t = table.cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    if t.ndim != 2 or not (min_cols or cols) <= t.shape[1] <= cols or t.shape[0] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"{name} must be an integer table {shape or f'[B, {cols}]'} (got {t.dtype} {t.shape})")
    return t.astype(np.int64)


def _host_clip_first(clip_first, ends_at=None):
    """int64 clip_first [n_clips + 1] from host integers: it starts at 0, increases strictly and (ends_at given) ends there."""
    import numpy as np
    first = clip_first.cpu().numpy() if torch.is_tensor(clip_first) else np.asarray(clip_first)
    if first.ndim != 1 or first.shape[0] < 2 or not np.issubdtype(first.dtype, np.integer):
        raise ValueError(f"clip_first must be an integer vector [n_clips + 1] (got {first.dtype} {first.shape})")
    first = np.ascontiguousarray(first, dtype=np.int64)
    if first[0] != 0 or np.diff(first).min() < 1 or (ends_at is not None and int(first[-1]) != ends_at):
        raise ValueError("clip_first must start at 0 and increase strictly (every clip holds at least one frame)" if ends_at is None else
                         f"clip_first must start at 0, increase strictly and end at the {ends_at} stored rows")
    return first


# the checks of a table's rows, one each (t: _host_table's array, or columns of it)
def _check_index(index, n, what):
    if index.min() < 0 or index.max() >= n:
        raise ValueError(f"{what} index outside [0, {n})")


def _check_windows(t, lengths, n_frames, seq_step):
    """Columns 0 and 1 of a clips table: the clip index inside `lengths` (frames per clip), the window inside its clip."""
    _check_index(t[:, 0], len(lengths), "clip")
    if t[:, 1].min() < 0 or (t[:, 1] + (int(n_frames) - 1) * int(seq_step) >= lengths[t[:, 0]]).any():
        raise ValueError(f"a window of {n_frames} frames at step {seq_step} leaves its clip")


def _boxes_leave(y0, x0, h, w, H, W):
    return bool(y0.min() < 0 or x0.min() < 0 or (y0 + h > H).any() or (x0 + w > W).any())


def _check_flips(flips, reserved=None):
    if flips.min() < 0 or flips.max() > 3:
        raise ValueError("flip bits outside 0 ... 3 (bit 0 horizontal, bit 1 vertical)")
    if reserved is not None and (reserved != 0).any():
        raise ValueError("the last column of a clips table is reserved: zeros")


def _int32(t):
    import numpy as np
    return np.ascontiguousarray(t, dtype=np.int32)


def _on_device(who, src, whose, index, index_name, index_cols, table):
    """True: `index` (clip_geom [n_clips, 4] or clip_first [n_clips + 1]) and `table` [B, 8] are GPU tensors of the launch's types on
    src's GPU, which the caller has checked; False: both are host tables, to be checked here. One of each is refused."""
    on_device = [torch.is_tensor(t) and t.is_cuda for t in (index, table)]
    if all(on_device):
        tail, rows, shape = ((index_cols,), 1, f"[n_clips, {index_cols}]") if index_cols else ((), 2, "[n_clips + 1]")
        if (index.dtype != torch.int64 or index.ndim != 1 + len(tail) or tuple(index.shape[1:]) != tail or index.shape[0] < rows or not index.is_contiguous()
                or table.dtype != torch.int32 or table.ndim != 2 or table.shape[1] != 8 or table.shape[0] < 1 or not table.is_contiguous()
                or index.device != src.device or table.device != src.device):
            raise ValueError(f"{who}: device tables must be contiguous int64 {shape} and int32 [B, 8] on the {whose} GPU")
    elif any(on_device):
        raise ValueError(f"{who}: {index_name} and table must both be host tables or both be GPU tensors")
    return all(on_device)


def check_frames_table(table, n_seqs, frame_hw, crop_hw):
    """The table a preprocess launch is handed, checked where it can be read (the host): int32 [B, 4] rows (sequence index, crop y0,
    crop x0, flip bits) with the index inside [0, n_seqs), the box inside the frame (there is no padding) and flip bits in 0 ... 3."""
    t = _host_table(table, 4)
    (H, W), (ch, cw) = frame_hw, crop_hw
    _check_index(t[:, 0], n_seqs, "sequence")
    if _boxes_leave(t[:, 1], t[:, 2], ch, cw, H, W):
        raise ValueError(f"a {ch}x{cw} crop box leaves the {H}x{W} frame (there is no padding)")
    _check_flips(t[:, 3])
    return _int32(t)


def frames_preprocess(src, table, n_frames, seq_step=1, crop_size=None, out_size=None, c_out=None, value_range=(0.0, 1.0), out=None):
    """float32 [B, n_frames, C_out, oh, ow] from raw stored sequences `src` [N, T', H, W(, Cs)] (a uint8 / uint16 / float32 GPU tensor,
    channels last) in ONE launch: scale, crop, bilinear resize (align_corners=False, no antialiasing), flip — see include/vpx.h.
    `table`: host rows [B, 4] = (sequence index, crop y0, crop x0, flip bits), checked here, copied to the device once. crop_size defaults
    to the frame, out_size to the crop, c_out to Cs. `out`: an optional destination of that shape (any 4-byte alignment)."""
    src = _stored_source("frames_preprocess", "src", src, FRAME_DTYPES, "frames are converted")
    if src.ndim not in (4, 5):
        raise ValueError(f"frames_preprocess: src must be [N, T', H, W] or [N, T', H, W, C] (got {tuple(src.shape)})")
    N, Tp, H, W = (int(s) for s in src.shape[:4])
    Cs = int(src.shape[4]) if src.ndim == 5 else 1
    ch, cw, oh, ow, c_out = _boxed_sizes("frames_preprocess", (H, W), Cs, crop_size, out_size, c_out, n_frames, seq_step)
    host = check_frames_table(table, N, (H, W), (ch, cw))
    B = host.shape[0]
    lo, hi = float(value_range[0]), float(value_range[1])
    out = _gather_out("frames_preprocess", out, (B, int(n_frames), c_out, oh, ow), src.device)
    dev_table = torch.from_numpy(host).to(src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().vpx_frames_preprocess(ptr(src), FRAME_DTYPES[src.dtype], N, Tp, H, W, Cs, ptr(dev_table), B, int(n_frames), int(seq_step),
                                               ch, cw, oh, ow, c_out, lo, hi, ptr(out), stream()), "vpx_frames_preprocess")
    return out


def check_clips_table(table, clip_first, n_frames, seq_step, frame_hw, crop_hw):
    """The offsets and the table a clips launch is handed, checked where they can be read (the host). clip_first: integers
    [n_clips + 1], the first frame of every clip in the buffer, starting at 0 and strictly increasing (a clip holds at least one frame);
    its last entry is the number of frames. table: integer [B, 6] rows (clip index, start frame within the clip, crop y0, crop x0, flip
    bits, 0) with the index inside [0, n_clips), the window inside its clip (0 <= start, start + (n_frames - 1) * seq_step < the clip's
    length), the box inside the frame (there is no padding), flip bits in 0 ... 3 and a zero last column.
    Returns (int64 clip_first, int32 table), both contiguous."""
    first = _host_clip_first(clip_first)
    t = _host_table(table, 6)
    (H, W), (ch, cw) = frame_hw, crop_hw
    _check_windows(t, first[1:] - first[:-1], n_frames, seq_step)
    if _boxes_leave(t[:, 2], t[:, 3], ch, cw, H, W):
        raise ValueError(f"a {ch}x{cw} crop box leaves the {H}x{W} frame (there is no padding)")
    _check_flips(t[:, 4], reserved=t[:, 5])
    return first, _int32(t)


def clips_preprocess(src, clip_first, table, n_frames, seq_step=1, crop_size=None, out_size=None, c_out=None, value_range=(0.0, 1.0), out=None):
    """float32 [B, n_frames, C_out, oh, ow] from windows of long clips in ONE launch. `src` [frames, H, W(, Cs)] (a uint8 / uint16 /
    float32 GPU tensor, channels last) holds every clip back to back; `clip_first`: host integers [n_clips + 1], the first frame of each
    clip, the last entry = frames; `table`: host rows [B, 6] = (clip index, start frame within the clip, crop y0, crop x0, flip bits, 0).
    out[b, t] comes from frame clip_first[clip] + start + t * seq_step, through the pixel arithmetic of frames_preprocess (the same device
    function: scale, crop, bilinear resize, flips, gray repeat — see include/vpx.h). Both host arguments are checked here
    (check_clips_table) and copied to the device once. The defaults are those of frames_preprocess."""
    src = _stored_source("clips_preprocess", "src", src, FRAME_DTYPES, "frames are converted")
    if src.ndim not in (3, 4):
        raise ValueError(f"clips_preprocess: src must be [frames, H, W] or [frames, H, W, C] (got {tuple(src.shape)})")
    total, H, W = (int(s) for s in src.shape[:3])
    Cs = int(src.shape[3]) if src.ndim == 4 else 1
    n_frames, seq_step = int(n_frames), int(seq_step)
    ch, cw, oh, ow, c_out = _boxed_sizes("clips_preprocess", (H, W), Cs, crop_size, out_size, c_out, n_frames, seq_step)
    first, host = check_clips_table(table, clip_first, n_frames, seq_step, (H, W), (ch, cw))
    if int(first[-1]) != total:
        raise ValueError(f"clips_preprocess: clip_first ends at {int(first[-1])} but src holds {total} frames")
    B = host.shape[0]
    lo, hi = float(value_range[0]), float(value_range[1])
    out = _gather_out("clips_preprocess", out, (B, n_frames, c_out, oh, ow), src.device)
    dev_first = torch.from_numpy(first).to(src.device)
    dev_table = torch.from_numpy(host).to(src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().vpx_clips_preprocess(ptr(src), FRAME_DTYPES[src.dtype], total, H, W, Cs, ptr(dev_first), first.shape[0] - 1, ptr(dev_table), B,
                                              n_frames, seq_step, ch, cw, oh, ow, c_out, lo, hi, ptr(out), stream()), "vpx_clips_preprocess")
    return out


ACTION_DTYPES = {torch.float32: _lib.ACTIONS_F32, torch.float64: _lib.ACTIONS_F64}


def actions_gather(raw_actions, table, n_frames, seq_step=1):
    """float32 [B, n_frames, A] from stored actions `raw_actions` [N, T', A] (a float32 / float64 GPU tensor) in ONE launch:
    out[b, t] = float32(raw_actions[table[b, 0], t * seq_step]) — see include/vpx.h. `table`: the host rows [B, 4] a preprocess launch
    takes, or a GPU int32 tensor [B, 4] whose sequence indices the caller has checked (a dataset hands over the table of its frames
    launch); only column 0 is read. float64 is rounded to nearest even, as numpy's astype(float32) does."""
    src = _stored_source("actions_gather", "raw_actions", raw_actions, ACTION_DTYPES, "the rows are gathered")
    if src.ndim != 3 or min(src.shape) < 1:
        raise ValueError(f"actions_gather: raw_actions must be [N, T', A], nothing empty (got {tuple(src.shape)})")
    N, Tp, A = (int(s) for s in src.shape)
    n_frames, seq_step = int(n_frames), int(seq_step)
    if min(n_frames, seq_step) < 1:
        raise ValueError(f"actions_gather: n_frames and seq_step must be >= 1 (got {n_frames}, {seq_step})")
    if (n_frames - 1) * seq_step + 1 > Tp:
        raise ValueError(f"actions_gather: frame {n_frames - 1} at step {seq_step} lies past the {Tp} stored frames")
    if torch.is_tensor(table) and table.is_cuda:
        if table.dtype != torch.int32 or table.ndim != 2 or table.shape[1] != 4 or table.shape[0] < 1 or not table.is_contiguous() or table.device != src.device:
            raise ValueError(f"actions_gather: a device table must be a contiguous int32 [B, 4] on the actions' GPU (got {table.dtype} {tuple(table.shape)})")
        dev_table = table
    else:
        t = _host_table(table, 4)
        _check_index(t[:, 0], N, "sequence")
        dev_table = torch.from_numpy(_int32(t)).to(src.device)
    B = int(dev_table.shape[0])
    out = torch.empty((B, n_frames, A), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().vpx_actions_gather(ptr(src), ACTION_DTYPES[src.dtype], N, Tp, A, ptr(dev_table), B, n_frames, seq_step, ptr(out), stream()),
              "vpx_actions_gather")
    return out


def check_clips_var_table(table, clip_geom, total_elems, channels, n_frames, seq_step):
    """The tables a mixed-shape clips launch is handed, checked where they can be read (the host). clip_geom: integers [n_clips, 4] rows
    (element offset of the clip's first frame, frame count, H_i, W_i), every clip inside the total_elems elements of the buffer (offset
    >= 0, count, H_i, W_i >= 1, sides up to 32768, offset + count * H_i * W_i * channels <= total_elems). table: integer [B, 8] rows (clip
    index, start frame within the clip, box y0, box x0, box h, box w, flip bits, 0) with the index inside [0, n_clips), the window inside
    its clip, a box of at least one pixel inside the clip's own H_i x W_i frame (there is no padding), flip bits in 0 ... 3 and a zero
    last column. Returns (int64 clip_geom, int32 table), both contiguous."""
    import numpy as np
    geom = np.ascontiguousarray(_host_table(clip_geom, 4, "clip_geom", "[n_clips, 4]"))
    if geom[:, 0].min() < 0 or geom[:, 1:].min() < 1 or geom[:, 2:].max() > 32768:
        raise ValueError("clip_geom: an offset below 0, a frame count or a side below 1, or a side beyond 32768")
    if (geom[:, 0] + geom[:, 1] * geom[:, 2] * geom[:, 3] * int(channels) > int(total_elems)).any():
        raise ValueError(f"a clip leaves the {int(total_elems)} stored elements")
    t = _host_table(table, 8)
    _check_windows(t, geom[:, 1], n_frames, seq_step)
    if t[:, 4:6].min() < 1 or _boxes_leave(t[:, 2], t[:, 3], t[:, 4], t[:, 5], geom[t[:, 0], 2], geom[t[:, 0], 3]):
        raise ValueError("a crop box is empty or leaves its clip's frame (there is no padding)")
    _check_flips(t[:, 6], reserved=t[:, 7])
    return geom, _int32(t)


def clips_preprocess_var(src, clip_geom, table, n_frames, seq_step=1, out_size=None, channels=1, c_out=None, value_range=(0.0, 1.0), out=None):
    """float32 [B, n_frames, C_out, oh, ow] from windows of clips of MIXED frame sizes in ONE launch. `src`: a contiguous uint8 / uint16 /
    float32 GPU tensor (any shape; read as one element buffer) holding every clip [T_i, H_i, W_i, channels] back to back; `clip_geom`:
    host integers [n_clips, 4] = (element offset, frame count, H_i, W_i); `table`: host rows [B, 8] = (clip index, start frame within the
    clip, box y0, box x0, box h, box w, flip bits, 0). The box of frame start + t * seq_step goes to out_size = (oh, ow) through the pixel
    arithmetic of frames_preprocess (the same device function, with the sample's sizes): a box of that size is copied, any other resized
    (bilinear, align_corners=False, no antialiasing); flips after the resize; c_out = 3 repeats one stored channel. Host tables are
    checked here (check_clips_var_table) and copied to the device once. Both may also be GPU tensors (int64 [n_clips, 4], int32 [B, 8])
    that the caller has checked: the launch reads nothing outside `src` for any row, and a row that was not valid yields zeros."""
    src = _stored_source("clips_preprocess_var", "src", src, FRAME_DTYPES, "frames are converted")
    total, Cs = int(src.numel()), int(channels)
    n_frames, seq_step = int(n_frames), int(seq_step)
    if out_size is None:
        raise ValueError("clips_preprocess_var: out_size=(oh, ow) is required (the clips have no common frame size)")
    oh, ow = (int(s) for s in out_size)
    c_out = Cs if c_out is None else int(c_out)
    if min(oh, ow, n_frames, seq_step, Cs, total) < 1:
        raise ValueError(f"clips_preprocess_var: every size must be >= 1 (output {oh}x{ow}, {n_frames} frames, step {seq_step}, {Cs} channels, {total} elements)")
    if _on_device("clips_preprocess_var", src, "frames'", clip_geom, "clip_geom", 4, table):
        dev_geom, dev_table = clip_geom, table
    else:
        geom, host = check_clips_var_table(table, clip_geom, total, Cs, n_frames, seq_step)
        dev_geom, dev_table = torch.from_numpy(geom).to(src.device), torch.from_numpy(host).to(src.device)
    B, n_clips = int(dev_table.shape[0]), int(dev_geom.shape[0])
    lo, hi = float(value_range[0]), float(value_range[1])
    out = _gather_out("clips_preprocess_var", out, (B, n_frames, c_out, oh, ow), src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().vpx_clips_preprocess_var(ptr(src), FRAME_DTYPES[src.dtype], total, Cs, ptr(dev_geom), n_clips, ptr(dev_table), B, n_frames,
                                                  seq_step, oh, ow, c_out, lo, hi, ptr(out), stream()), "vpx_clips_preprocess_var")
    return out


def actions_diff_gather(positions, clip_first, table, n_frames, seq_step=1):
    """float32 [B, n_frames - 1, A] from per-frame positions `positions` [frames, A] (a float32 / float64 GPU tensor, every clip back to
    back) in ONE launch: out[b, j] = float32(positions[g(j + 1)] - positions[g(j)]) with g(j) = clip_first[clip] + start + j * seq_step,
    the subtraction in the stored precision — see include/vpx.h. `clip_first`: host integers [n_clips + 1]; `table`: host rows [B, 8] of a
    mixed-shape clips launch (or any integer [B, >= 2] rows: only the clip index and the start frame are read), checked here; or both as
    GPU tensors (int64 [n_clips + 1], int32 [B, 8]) that the caller has checked."""
    src = _stored_source("actions_diff_gather", "positions", positions, ACTION_DTYPES, "the rows are gathered")
    if src.ndim != 2 or min(src.shape) < 1:
        raise ValueError(f"actions_diff_gather: positions must be [frames, A], nothing empty (got {tuple(src.shape)})")
    total, A = (int(s) for s in src.shape)
    n_frames, seq_step = int(n_frames), int(seq_step)
    if n_frames < 2 or seq_step < 1:
        raise ValueError(f"actions_diff_gather: n_frames must be >= 2 (a difference needs two frames) and seq_step >= 1 (got {n_frames}, {seq_step})")
    if _on_device("actions_diff_gather", src, "positions'", clip_first, "clip_first", None, table):
        dev_first, dev_table = clip_first, table
    else:
        import numpy as np
        first = _host_clip_first(clip_first, ends_at=total)
        t = _host_table(table, 8, min_cols=2)
        _check_windows(t, first[1:] - first[:-1], n_frames, seq_step)
        host = np.zeros((t.shape[0], 8), dtype=np.int32)
        host[:, :2] = t[:, :2]
        dev_first, dev_table = torch.from_numpy(first).to(src.device), torch.from_numpy(host).to(src.device)
    B = int(dev_table.shape[0])
    out = torch.empty((B, n_frames - 1, A), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().vpx_actions_diff_gather(ptr(src), ACTION_DTYPES[src.dtype], total, A, ptr(dev_first), int(dev_first.shape[0]) - 1, ptr(dev_table), B,
                                                 n_frames, seq_step, ptr(out), stream()), "vpx_actions_diff_gather")
    return out


def frames_postprocess(x, lo=0.0, hi=1.0):
    """uint8 [..., h, w, C] on the GPU from float32 [..., C, h, w] in one launch: ((x - lo) / (hi - lo)) * 255 in float32, clamped to
    [0, 255], truncated; NaN gives 0. `x` is left as it is (the reference subtracts in place)."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.VpxError("frames_postprocess: x must be a GPU tensor; there is no CPU fallback")
    if x.dtype != torch.float32:
        raise ValueError(f"frames_postprocess: expected float32, got {x.dtype}")
    if x.ndim < 3:
        raise ValueError("expected at least three dimensions for input image")
    xc = x.contiguous()
    C, h, w = (int(s) for s in x.shape[-3:])
    lead = tuple(int(s) for s in x.shape[:-3])
    N = 1
    for s in lead:
        N *= s
    out = torch.empty(lead + (h, w, C), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vpx_frames_postprocess(ptr(xc), N, C, h, w, float(lo), float(hi), ptr(out), stream()), "vpx_frames_postprocess")
    return out


# ---- photometric augmentations and erasing of a preprocessed batch (csrc/frames_aug.hip) ----
def check_frames_programs(programs, n_samples):
    """The programs an augment launch is handed, checked where they can be read (the host): float32 [B, max_ops, FRAMES_AUG_ROW] with
    max_ops in [FRAMES_AUG_MIN_OPS, FRAMES_AUG_MAX_OPS], every opcode a whole number in 0 ... 10 and every parameter finite."""
    import numpy as np
    t = np.asarray(programs)
    if t.ndim != 3 or t.shape[0] != n_samples or t.shape[2] != _lib.FRAMES_AUG_ROW or t.dtype != np.float32:
        raise ValueError(f"programs must be a float32 table [{n_samples}, max_ops, {_lib.FRAMES_AUG_ROW}] (got {t.dtype} {t.shape})")
    if not _lib.FRAMES_AUG_MIN_OPS <= t.shape[1] <= _lib.FRAMES_AUG_MAX_OPS:
        raise ValueError(f"programs hold {t.shape[1]} rows per sample, outside [{_lib.FRAMES_AUG_MIN_OPS}, {_lib.FRAMES_AUG_MAX_OPS}]")
    op = t[:, :, 0]
    if not np.isfinite(t).all() or (op != np.floor(op)).any() or op.min() < 0 or op.max() > 10:
        raise ValueError("programs: an opcode outside 0 ... 10 or a parameter that is not finite")
    return np.ascontiguousarray(t)


def frames_augment(x, programs):
    """Runs per-sample programs of photometric operations and erasing over x [B, n_frames, C, h, w] (a contiguous float32 GPU tensor)
    IN PLACE, in one launch, and returns x — see include/vpx.h for the operations and their float32 forms. `programs`: rows
    [B, max_ops, 9] = (opcode, 8 parameters), opcode 0 ends a program; a host array is checked here and copied to the device once, a GPU
    tensor is taken as it is (the kernel ends a program at a row it cannot run and writes nothing outside the frames)."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.VpxError("frames_augment: x must be a GPU tensor; frames are augmented by a HIP kernel, there is no CPU fallback")
    if x.dtype != torch.float32:
        raise ValueError(f"frames_augment: expected float32, got {x.dtype}")
    if x.ndim != 5 or not x.is_contiguous():
        raise ValueError(f"frames_augment: x must be a contiguous [B, n_frames, C, h, w] tensor, changed in place (got {tuple(x.shape)})")
    B, F, C, h, w = (int(s) for s in x.shape)
    if min(B, F, C, h, w) < 1:
        raise ValueError(f"frames_augment: empty input {tuple(x.shape)}")
    if torch.is_tensor(programs) and programs.is_cuda:
        if programs.dtype != torch.float32 or programs.ndim != 3 or programs.shape[0] != B or programs.shape[2] != _lib.FRAMES_AUG_ROW or not programs.is_contiguous():
            raise ValueError(f"frames_augment: programs must be a contiguous float32 table [{B}, max_ops, {_lib.FRAMES_AUG_ROW}] (got {programs.dtype} {tuple(programs.shape)})")
        dev = programs
    else:
        dev = torch.from_numpy(check_frames_programs(programs.numpy() if torch.is_tensor(programs) else programs, B)).to(x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vpx_frames_augment(ptr(x), ptr(dev), B, F, C, h, w, int(dev.shape[1]), stream()), "vpx_frames_augment")
    return x


# ---- frame adapter between a model and a test set (csrc/adapt.hip) ----
def frames_adapt(x, out_hw=None, src_range=(0.0, 1.0), dst_range=(0.0, 1.0)):
    """float32 [..., C, oh, ow] on the GPU from planar float32 frames x [N, C, H, W] or [b, t, C, H, W] in ONE launch: every value mapped
    from src_range to dst_range (((v - src_lo) / (src_hi - src_lo)) * (dst_hi - dst_lo) + dst_lo; skipped for equal ranges), then resized
    bilinearly (align_corners=False, no antialiasing; skipped for out_hw None or (H, W)) — the reference's ScaleToModel / ScaleToTest and
    TF.Resize in their order, see include/vpx.h. Forward only: an input that needs a gradient is refused. A non-contiguous `x` (the halves
    VPModel.unpack_data splits) is read through one dense copy; `x` itself is left as it is."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.VpxError("frames_adapt: x must be a GPU tensor; frames are adapted by a HIP kernel, there is no CPU fallback")
    if x.dtype != torch.float32:
        raise ValueError(f"frames_adapt: expected float32, got {x.dtype}")
    if x.ndim not in (4, 5):
        raise ValueError(f"frames_adapt: x must be [N, C, H, W] or [b, t, C, H, W] (got {tuple(x.shape)})")
    if needs_grad(x):
        raise _lib.VpxError("frames_adapt: the adapter is forward only (testing runs under no_grad); x requires a gradient")
    if len(src_range) != 2 or len(dst_range) != 2:
        raise ValueError("frames_adapt: src_range and dst_range are (lo, hi) pairs")
    lead = tuple(int(s) for s in x.shape[:-3])
    C, H, W = (int(s) for s in x.shape[-3:])
    oh, ow = (H, W) if out_hw is None else (int(s) for s in out_hw)
    N = 1
    for s in lead:
        N *= s
    if min(N, C, H, W) < 1:
        raise ValueError(f"frames_adapt: empty input {tuple(x.shape)}")
    xc = x.detach().contiguous()
    out = torch.empty(lead + (C, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vpx_frames_adapt(ptr(xc), N, C, H, W, oh, ow, float(src_range[0]), float(src_range[1]), float(dst_range[0]),
                                          float(dst_range[1]), ptr(out), stream()), "vpx_frames_adapt")
    return out


# ---- prediction visualizations: bordered tiles composed into a canvas (csrc/vis.hip) ----
def check_vis_tiles(tiles, n_seqs, n_frames, frame_hw, canvas_shape):
    """The table a compose launch is handed, checked where it can be read (the host): int32 [n_tiles, 8] rows (s, t, f, y0, x0, b, colour
    0xRRGGBB, 0) with s inside [0, n_seqs), t inside [0, n_frames), f inside the canvas's frames, b >= 0, the (h + 2b) x (w + 2b) rectangle
    inside the canvas frame and no two rectangles of one canvas frame overlapping. Returns (the table as contiguous int32, the largest b,
    whether the tiles cover the canvas exactly)."""
    import numpy as np
    t = tiles.cpu().numpy() if torch.is_tensor(tiles) else np.asarray(tiles)
    if t.ndim != 2 or t.shape[1] != _lib.VIS_TILE_ROW or t.shape[0] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"tiles must be an integer table [n_tiles, {_lib.VIS_TILE_ROW}] (got {t.dtype} {t.shape})")
    if len(canvas_shape) != 4 or int(canvas_shape[3]) != 3 or min(int(v) for v in canvas_shape) < 1:
        raise ValueError(f"the canvas is [F, Hc, Wc, 3] with every size >= 1 (got {tuple(canvas_shape)})")
    t = t.astype(np.int64)
    (h, w), (F, Hc, Wc) = frame_hw, (int(v) for v in canvas_shape[:3])
    s, tt, f, y0, x0, b, colour, rest = (t[:, i] for i in range(8))
    if s.min() < 0 or s.max() >= n_seqs:
        raise ValueError(f"sequence index s outside [0, {n_seqs})")
    if tt.min() < 0 or tt.max() >= n_frames:
        raise ValueError(f"frame index t outside [0, {n_frames})")
    if f.min() < 0 or f.max() >= F:
        raise ValueError(f"canvas frame f outside [0, {F})")
    if b.min() < 0:
        raise ValueError("negative border width b")
    y1, x1 = y0 + h + 2 * b, x0 + w + 2 * b
    if y0.min() < 0 or x0.min() < 0 or (y1 > Hc).any() or (x1 > Wc).any():
        raise ValueError(f"a tile leaves the {Hc}x{Wc} canvas")
    if colour.min() < 0 or colour.max() > 0xFFFFFF:
        raise ValueError("border colour outside 0x000000 ... 0xFFFFFF")
    if rest.any():
        raise ValueError("column 7 is reserved and must be 0")
    for frame in np.unique(f):
        i = np.nonzero(f == frame)[0]
        if i.size > 1:
            meet = (np.minimum(y1[i, None], y1[None, i]) > np.maximum(y0[i, None], y0[None, i])) & \
                   (np.minimum(x1[i, None], x1[None, i]) > np.maximum(x0[i, None], x0[None, i]))
            np.fill_diagonal(meet, False)
            if meet.any():
                a, c = (int(v[0]) for v in np.nonzero(meet))
                raise ValueError(f"tiles {int(i[a])} and {int(i[c])} of canvas frame {int(frame)} overlap")
    covered = int(((y1 - y0) * (x1 - x0)).sum()) == F * Hc * Wc           # (in bounds and disjoint: equal areas mean an exact cover)
    return np.ascontiguousarray(t, dtype=np.int32), int(b.max()), covered


def vis_compose(src, tiles, canvas_shape, lo=0.0, hi=1.0, background=255, *, max_border=None):
    """uint8 [F, Hc, Wc, 3] on the GPU, composed in ONE launch (csrc/vis.hip) from src [S, T, C, h, w] (a float32 GPU tensor in the value
    range [lo, hi], C = 1 or 3) and the tile table [n_tiles, 8] = (s, t, f, y0, x0, b, colour 0xRRGGBB, 0): each tile is frame (s, t) as
    frames_postprocess's bytes inside a ring of width b in its colour, at (y0, x0) of canvas frame f; the rest is `background` (a grey
    level). A host table is checked here (check_vis_tiles) and copied to the device once, and the canvas fill is skipped when its tiles
    cover the canvas exactly. A GPU tensor (int32, contiguous) is taken as it is, with max_border = the largest b it holds given by the
    caller: the kernel skips a row it cannot run and writes nothing outside the canvas. A non-contiguous `src` is read through one dense copy."""
    if not (torch.is_tensor(src) and src.is_cuda):
        raise _lib.VpxError("vis_compose: src must be a GPU tensor; visualizations are composed by a HIP kernel, there is no CPU fallback")
    if src.dtype != torch.float32:
        raise ValueError(f"vis_compose: expected float32, got {src.dtype}")
    if src.ndim != 5:
        raise ValueError(f"vis_compose: src must be [S, T, C, h, w] (got {tuple(src.shape)})")
    S, T, C, h, w = (int(v) for v in src.shape)
    if min(S, T, C, h, w) < 1:
        raise ValueError(f"vis_compose: empty input {tuple(src.shape)}")
    if len(canvas_shape) != 4 or int(canvas_shape[3]) != 3 or min(int(v) for v in canvas_shape) < 1:
        raise ValueError(f"vis_compose: the canvas is [F, Hc, Wc, 3] with every size >= 1 (got {tuple(canvas_shape)})")
    if not 0 <= int(background) <= 255:
        raise ValueError(f"vis_compose: background {background} is not a grey level 0 ... 255")
    F, Hc, Wc = (int(v) for v in canvas_shape[:3])
    if torch.is_tensor(tiles) and tiles.is_cuda:
        if tiles.dtype != torch.int32 or tiles.ndim != 2 or tiles.shape[1] != _lib.VIS_TILE_ROW or tiles.shape[0] < 1 or not tiles.is_contiguous():
            raise ValueError(f"vis_compose: tiles must be a contiguous int32 table [n_tiles, {_lib.VIS_TILE_ROW}] (got {tiles.dtype} {tuple(tiles.shape)})")
        if max_border is None:
            raise ValueError("vis_compose: a table on the device needs max_border, the largest b it holds")
        dev, bmax, fill = tiles, int(max_border), int(background)
    else:
        host, bmax, covered = check_vis_tiles(tiles, S, T, (h, w), (F, Hc, Wc, 3))
        dev, fill = torch.from_numpy(host).to(src.device), (-1 if covered else int(background))
    xc = src.detach().contiguous()
    canvas = torch.empty((F, Hc, Wc, 3), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        check(_lib.lib().vpx_vis_compose(ptr(xc), S, T, C, h, w, float(lo), float(hi), ptr(dev), int(dev.shape[0]), bmax, ptr(canvas), F, Hc, Wc,
                                         fill, stream()), "vpx_vis_compose")
    return canvas


# ---- Frechet Video Distance on an Inception-I3D trunk (csrc/fvd.hip); maps are channels-last [N, T, H, W, C]; forward only ----------------
FVD_SIDE = 224       # the I3D input: frames are resized to it
FVD_MAX_B = 256      # the cap on feature vectors per set in frechet_distance
FVD_ROW, FVD_CONV, FVD_POOL, FVD_HEAD = 16, 0, 1, 2   # include/vpx.h: VPX_FVD_ROW, VPX_FVD_CONV / _POOL / _HEAD


def same_padding(size, k, s):
    """(front, back, out) of one axis under the reference's "SAME" rule: pad = max(k - s, 0) if size % s == 0 else max(k - size % s, 0),
    front = pad // 2, output size ceil(size / s). Answered by the library (host only), so that Python and the kernels share one rule."""
    front, out = ctypes.c_int(), ctypes.c_int()
    check(_lib.lib().vpx_same_padding(int(size), int(k), int(s), ctypes.byref(front), ctypes.byref(out)), "vpx_same_padding")
    back = max((out.value - 1) * s + k - size, 0) - front.value   # what the library's front and output size leave behind the map
    return front.value, back, out.value


def _fvd_operand(t, what, name, shape=None):
    require_gpu(t, what)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.contiguous()


def _triple(v, what, name):
    v = tuple(int(i) for i in ((v,) * 3 if isinstance(v, int) else v))
    if len(v) != 3 or min(v) < 1:
        raise ValueError(f"{what}: {name} must be three sizes >= 1 (got {v})")
    return v


def conv3d_pack(w):
    """[kt, kh, kw, Ci, Co] contiguous: the layout vpx_conv3d_same reads, from the reference's [Co, Ci, kt, kh, kw]."""
    return w.permute(2, 3, 4, 1, 0).contiguous()


def conv3d_same(x, w, bias, stride=(1, 1, 1), relu=False, out=None, channel_offset=0, packed=False):
    """Unit3D without its BatchNorm (fold it into w and bias): ReLU?(conv3d(zero-pad "SAME"(x), w) + bias) of a channels-last map
    x [N, T, H, W, Ci]. w: [Co, Ci, kt, kh, kw], packed here per call, or with packed=True the result of conv3d_pack (the trunk packs
    once, at registration). Returns [N, To, Ho, Wo, Co]; with `out` [N, To, Ho, Wo, ld] only its channels channel_offset ..
    channel_offset + Co - 1 are written. Exact fp32 operands."""
    what = "conv3d_same"
    if x.ndim != 5 or w.ndim != 5:
        raise ValueError(f"{what}: expected a channels-last map [N, T, H, W, Ci] and weights with five axes")
    x = _fvd_operand(x, what, "x")
    N, T, H, W, Ci = x.shape
    wp = _fvd_operand(w, what, "w") if packed else conv3d_pack(_fvd_operand(w, what, "w"))
    kt, kh, kw, wci, Co = wp.shape
    if wci != Ci:
        raise ValueError(f"{what}: w has {wci} input channels, x has {Ci}")
    bias = _fvd_operand(bias, what, "bias", (Co,))
    st, sh, sw = _triple(stride, what, "stride")
    To, Ho, Wo = same_padding(T, kt, st)[2], same_padding(H, kh, sh)[2], same_padding(W, kw, sw)[2]
    if out is None:
        out = torch.empty(N, To, Ho, Wo, Co, device=x.device)
        channel_offset = 0
    else:
        require_gpu(out, what)
        if out.ndim != 5 or tuple(out.shape[:4]) != (N, To, Ho, Wo) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"{what}: out must be a contiguous [N, To, Ho, Wo, ld] = [{N}, {To}, {Ho}, {Wo}, ld] map on x's device (got {tuple(out.shape)})")
        if channel_offset < 0 or channel_offset + Co > out.shape[4]:
            raise ValueError(f"{what}: channels {channel_offset} .. {channel_offset + Co - 1} do not fit out's {out.shape[4]}")
    with torch.cuda.device(x.device):
        check(_lib.lib().vpx_conv3d_same(ptr(x), ptr(wp), ptr(bias), ptr(out), N, T, H, W, Ci, Co, kt, kh, kw, st, sh, sw, int(bool(relu)), out.shape[4],
                                         int(channel_offset), stream()), "vpx_conv3d_same")
    return out


def maxpool3d_same(x, kernel, stride):
    """[N, To, Ho, Wo, C]: max-pool of a channels-last map [N, T, H, W, C] over its ZERO-padded extension ("SAME" padding: the reference
    pads with zeros before it pools, so a window on the border never returns less than 0)."""
    what = "maxpool3d_same"
    if x.ndim != 5:
        raise ValueError(f"{what}: expected a channels-last map [N, T, H, W, C]")
    x = _fvd_operand(x, what, "x")
    N, T, H, W, C = x.shape
    (kt, kh, kw), (st, sh, sw) = _triple(kernel, what, "kernel"), _triple(stride, what, "stride")
    y = torch.empty(N, same_padding(T, kt, st)[2], same_padding(H, kh, sh)[2], same_padding(W, kw, sw)[2], C, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vpx_maxpool3d_same(ptr(x), ptr(y), N, T, H, W, C, kt, kh, kw, st, sh, sw, stream()), "vpx_maxpool3d_same")
    return y


def fvd_head(x, w, bias):
    """[N, n_features] float32: the mean over the 2x7x7 positions of a channels-last map [N, 2, 7, 7, C], then the logits layer
    w [n_features, C] (or [n_features, C, 1, 1, 1]) with bias. Any other map is refused."""
    what = "fvd_head"
    if x.ndim != 5:
        raise ValueError(f"{what}: expected a channels-last map [N, 2, 7, 7, C]")
    x = _fvd_operand(x, what, "x")
    N, T, H, W, C = x.shape
    if w.ndim == 5 and tuple(w.shape[2:]) == (1, 1, 1):
        w = w.reshape(w.shape[0], w.shape[1])
    w = _fvd_operand(w, what, "w", (w.shape[0], C))
    bias = _fvd_operand(bias, what, "bias", (w.shape[0],))
    out = torch.empty(N, w.shape[0], device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vpx_fvd_head(ptr(x), ptr(w), ptr(bias), ptr(out), N, T, H, W, C, w.shape[0], stream()), "vpx_fvd_head")
    return out


def fvd_table(rows):
    """(C int array, n_rows) of layer-table rows (op, src, dst, Ci, Co, kernel, stride, relu, coff, ld, param): what vpx_fvd_features walks."""
    flat = []
    for op, src, dst, Ci, Co, k, s, relu, coff, ld, param in rows:
        flat += [op, src, dst, Ci, Co, *k, *s, int(relu), coff, ld, param, 0]
    assert len(flat) == FVD_ROW * len(rows)
    return (ctypes.c_int * len(flat))(*flat), len(rows)


def fvd_features(x, trunk, x1=None):
    """[N (+ N1), n_features] float32: the I3D logits of the clips x [N, T, C, h, w] (and of x1 behind them, as one batch), values as they
    are. The frames are resized to 224x224 (ops.frames_adapt's resize, bit for bit) inside the call. trunk: what
    measure.fvd_weights(device) returns: {"table", "n_rows", "params", "ci", "n_features"}. T must lead to a final 2x7x7 map: 9 .. 16."""
    what = "fvd_features"
    if x.ndim != 5 or (x1 is not None and x1.shape[1:] != x.shape[1:]):
        raise ValueError(f"{what}: expected clips [N, T, C, h, w] of one shape")
    if needs_grad(x, x1):
        raise NotImplementedError(f"{what}: the backward of FVD is not implemented in this build (forward only): evaluate it under torch.no_grad() "
                                  f"or on detached tensors")
    x = _fvd_operand(x, what, "x")
    x1 = None if x1 is None else _fvd_operand(x1, what, "x1")
    n0, T, C, h, w = x.shape
    n1 = 0 if x1 is None else x1.shape[0]
    if C != trunk["ci"]:
        raise ValueError(f"{what}: the frames have {C} channels, the registered stem takes {trunk['ci']}")
    if any(p.device != x.device for p in trunk["params"]) or (x1 is not None and x1.device != x.device):
        raise ValueError(f"{what}: clips and weights must live on one device")
    L = _lib.lib()
    with torch.cuda.device(x.device):
        ws, ws_bytes = workspace(x.device, L.vpx_fvd_features_workspace_bytes, n0 + n1, T, C, h, w, trunk["table"], trunk["n_rows"], unsupported=b"beyond")
        out = torch.empty(n0 + n1, trunk["n_features"], device=x.device)
        check(L.vpx_fvd_features(ptr(x), ptr(x1), n0, n1, T, C, h, w, trunk["table"], trunk["n_rows"], ptr_array(trunk["params"]), len(trunk["params"]),
                                 ptr(out), ptr(ws), ws_bytes, stream()), "vpx_fvd_features")
    return out


def frechet_distance(pred, target):
    """A float64 scalar on the device: fact sum Ep^2 + fact sum Et^2 - 2 sum_i sqrt(sigma_i^2 + 1e-15) + |mu_p - mu_t|^2 of two feature
    tables [b, n] float32 (the reference's calculate_2_wasserstein_dist restated: sigma_i the singular values of the b x b matrix
    fact Ep Et^T, by a Jacobi iteration of a fixed maximum of sweeps). b <= FVD_MAX_B: more raises VpxError."""
    what = "frechet_distance"
    if pred.ndim != 2 or pred.shape != target.shape:
        raise ValueError(f"{what}: expected two feature tables [b, n] of one shape")
    pred, target = _fvd_operand(pred, what, "pred"), _fvd_operand(target, what, "target")
    b, n = pred.shape
    if b > FVD_MAX_B:
        raise VpxError(f"{what}: {b} feature vectors per set, this build supports at most {FVD_MAX_B}")
    if target.device != pred.device:
        raise ValueError(f"{what}: both tables must live on one device")
    L = _lib.lib()
    with torch.cuda.device(pred.device):
        ws, ws_bytes = workspace(pred.device, L.vpx_frechet_distance_workspace_bytes, b, n)
        out = torch.empty((), device=pred.device, dtype=torch.float64)
        check(L.vpx_frechet_distance(ptr(pred), ptr(target), b, n, ptr(out), ptr(ws), ws_bytes, stream()), "vpx_frechet_distance")
    return out
