"""The TrajGRU bilinear warp (csrc/trajgru.hip: trajgru_warp_fwd_kernel, trajgru_warp_bwd_kernel<FIXED>) at PRESCRIBED flows, through
the public op: zero flow, one / two / four taps out on every side, a single column or row left in, whole fields out (just, far, beyond
the int range), 1-wide and tiny maps, the fixed-point deterministic scatter — forward and every gradient against the fp64 oracle
(tests/trajgru_warp_ref.py holds the case table and the reference runner; tests/test_trajgru_warp_cases.py shows on the CPU that no case
sits on a kink, so every element of every tensor is compared). The blocks of the other TrajGRU tests draw their flows from a randomly
initialised flow generator: a fraction of a pixel, which a warp that clamps instead of padding, or loses d_flow once two taps are out,
passes.

Bounds: the suite's own (test_trajgru_block_vs_golden, test_random_trajgru_blocks_vs_oracle) — forward 2e-5 in exact-fp32 mode and 1e-4
in bf16x3 mode, every gradient 1e-4 in exact-fp32 mode, max-normalised; a bound becomes 3 x the fp32 oracle's own error against its fp64
run where that error exceeds a third of it (measured: at most 6.3e-7 on any tensor of the table, so none does)."""
import hashlib

import pytest
import torch

import trajgru_warp_ref as wr
from parity import relmax as _relmax   # max|a - b| / max|b|, recorded (tests/parity.py)

pytestmark = pytest.mark.gpu

# sha256 of `out` (float32, [B,T,C,H,W] contiguous) of wr.PARENT_HASH_CASE in deterministic mode, taken from a build of the commit before
# the coordinate clamp in warp_coords
PARENT_OUT_SHA256 = "93649fe00d926e9a08cfc45cfc58cb4c8909039019f36ca3a60ed73619452131"


def _run(tag, precision="f32", grad=True, scale=1.0, edit=None):
    """The case through traj_ops.trajgru_seq. Returns (out, hT, grads or None), on the CPU. `scale` multiplies the loss (both cotangents);
    `edit(P)` may change the CPU parameters first."""
    from vp_suite_amd import traj_ops
    case = wr.CASES[tag]
    P, x, h0, g = wr.tensors(case)
    if edit is not None:
        edit(P)
    dev = {k: v.cuda().requires_grad_(grad) for k, v in P.items()}
    dx, dh = x.cuda().requires_grad_(grad), h0.cuda().requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        out, hT = traj_ops.trajgru_seq(dx, dh, [dev[k] for k in wr.PARAM_KEYS], seq_len=case.T, L=len(case.fields), slope=wr.SLOPE,
                                       state_hw=(case.H, case.W), precision=precision)
    if not grad:
        return out.cpu(), hT.cpu(), None
    (wr.loss_of(out, hT, g.cuda()) * scale).backward()
    grads = {"x": dx.grad.cpu(), "h0": dh.grad.cpu()}
    grads.update({k: dev[k].grad.cpu() for k in wr.PARAM_KEYS})
    return out.detach().cpu(), hT.detach().cpu(), grads


def _deterministic(fn):
    torch.use_deterministic_algorithms(True)
    try:
        return fn()
    finally:
        torch.use_deterministic_algorithms(False)


def _check_grads(tag, grads, scale=1.0):
    case, ref, bars = wr.CASES[tag], wr.reference(tag), wr.bars(tag)
    bad = {}
    for k, r in ref.grads.items():   # dx, dh0 and the ten parameter gradients, each on its own
        e = _relmax(grads[k] / scale, r)
        print(f"  {tag} grad {k}: {e:.2e} (bound {bars[k][0]:.1e})")
        if not e < bars[k][0]:
            bad[k] = e
    assert not bad, (tag, bad)
    db = grads["flows_conv.bias"]
    for l in case.out:   # a field that samples nothing but padding: d_flow is exactly 0 at every pixel
        assert torch.equal(db[2 * l:2 * l + 2], torch.zeros(2)), (tag, l, db)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("tag", wr.MAIN + wr.NARROW)
def test_trajgru_prescribed_flows_vs_fp64(vpx, tag, precision):
    """Forward (both operand modes) and, in exact-fp32 mode, dx, dh0 and all ten parameter gradients against the fp64 oracle.
    flows_conv.bias.grad is the sum of d_flow per component — the direct observable of the warp backward's d_flow branch — and
    flows_conv.weight.grad is non-zero although the weight itself is 0 in the "bias" variant."""
    ref, bars = wr.reference(tag), wr.bars(tag)
    f32 = precision == "f32"
    out, hT, grads = _run(tag, precision, grad=f32)
    for name, got, want in (("out", out, ref.out), ("hT", hT, ref.hT)):
        bound, err32 = bars[name]
        if not f32:
            bound = wr.FWD_BF16X3 if err32 <= wr.FWD_BF16X3 / 3 else 3 * err32
        e = _relmax(got, want)
        print(f"  {tag} {precision} {name}: {e:.2e} (bound {bound:.1e})")
        assert e < bound, (tag, precision, name, e)
    if f32:
        _check_grads(tag, grads)


@pytest.mark.parametrize("tag", [t for t in wr.CASES if wr.CASES[t].out])
def test_trajgru_field_out_of_the_map_contributes_nothing(vpx, tag):
    """`warped` of a field that is out entirely is exactly 0: another slice of ret.weight for that field leaves `out` bit-identical
    (no oracle needed), another slice for a field that is in does not. Deterministic mode: on maps this small the convolutions
    otherwise split K over workgroups, and float atomics alone would change the last bit from run to run."""
    case = wr.CASES[tag]

    def with_slices(fields):
        def edit(P):
            for l in fields:
                P["ret.weight"][:, l * wr.C:(l + 1) * wr.C] += 1.0
        return edit

    inside = [l for l in range(len(case.fields)) if l not in case.out]
    base, other, moved = _deterministic(lambda: [_run(tag, grad=False, edit=e)[0] for e in (None, with_slices(case.out), with_slices(inside))])
    assert torch.equal(base, other), tag
    assert not torch.equal(base, moved), tag


def _out_sha256(tag):
    out = _deterministic(lambda: _run(tag, grad=False)[0])
    return hashlib.sha256(out.contiguous().numpy().tobytes()).hexdigest()


def test_trajgru_clamped_coordinates_leave_in_range_results_unchanged(vpx):
    """warp_coords clamps floor(s) to [-2, W] x [-2, H] before the int conversion (defined for any finite flow; every clamped value
    still has both taps out). In-range results do not move by one bit: `out` of the 6x7 table with flows up to one map width hashes
    to what the build before the clamp produced."""
    assert _out_sha256(wr.PARENT_HASH_CASE) == PARENT_OUT_SHA256


@pytest.mark.parametrize("tag", [t for t in wr.MAIN if t.startswith("6x7.") and ".T2." in t])
def test_trajgru_deterministic_scatter_at_prescribed_flows(vpx, tag):
    """torch.use_deterministic_algorithms(True): the 2^40 fixed-point scatter at flows that leave the map — two runs bit-identical,
    every gradient within the same 1e-4 of the fp64 oracle (not only of the float-atomic path), and again with the loss, hence both
    cotangents and every scattered addend, scaled by 1e4 (sums far inside the documented +-8.4e6): the scale does not enter the result."""
    a, b, big = _deterministic(lambda: [_run(tag)[2], _run(tag)[2], _run(tag, scale=1e4)[2]])
    for k in a:
        assert torch.equal(a[k], b[k]), (tag, k)
    _check_grads(tag, a)
    _check_grads(tag, big, scale=1e4)


def test_trajgru_channel_count_off_a_multiple_of_4_is_refused(vpx):
    """C = 6: the library's size query refuses the descriptor — ahead of every allocation and launch of the forward — and the op
    raises VpxError with the library's message."""
    from vp_suite_amd import traj_ops
    Cb, L, H, W = 6, 3, 6, 7
    shapes = {"i2h": (3 * Cb, wr.CIN, 3, 3), "i2f_conv1": (32, wr.CIN, 5, 5), "h2f_conv1": (32, Cb, 5, 5), "flows_conv": (2 * L, 32, 5, 5), "ret": (3 * Cb, L * Cb, 1, 1)}
    params = [t for n in wr.NAMES for t in (torch.zeros(shapes[n], device="cuda"), torch.zeros(shapes[n][0], device="cuda"))]
    x, h0 = torch.zeros(wr.B, 2, wr.CIN, H, W, device="cuda"), torch.zeros(wr.B, Cb, H, W, device="cuda")
    with pytest.raises(vpx.VpxError, match="multiple of 4"):
        traj_ops.trajgru_seq(x, h0, params, seq_len=2, L=L, slope=wr.SLOPE, state_hw=(H, W))
