"""The fused training tail in plain float64: the decoupling term (csrc/pointwise.hip, csrc/decouple_api.hip), the MSE value and gradient
and the flat-bucket Adam update (csrc/train_tail.hip), with the case tables of tests/test_gpu_train_tail.py (GPU parity) and
tests/test_train_tail_host.py (the conditions on the inputs, on the CPU). Nothing here touches the GPU or imports the package.

Decoupling inputs. The adapter is A = Q diag(s): Q the orthogonal factor of a seeded randn matrix, s drawn from [0.5, 2] — its inverse
amplifies rounding by 4 at most (with randn / sqrt(Ch) + I the fp32 restatement itself drifts to 1e-5 in the gradients: conditioning,
not the kernel). `random`: independent randn operands. `prescribed`: the adapter OUTPUTS are built in fp64 so that row (b, ch) has
cosine rho, rho cycling through RHOS — y_c = |y_c| u, y_m = |y_m| (rho u + sqrt(1 - rho^2) z), z orthogonal to u, lengths from [0.5, 2]
— and pulled back through the inverse of the float32 adapter, then rounded to float32. `small` / `large`: those inputs times 1e-4 / 1e3.
On a one-pixel map (HW = 1) no z exists: every cosine is +-1 whatever the inputs are, the value is 1 and every gradient is 0."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from golden_util import name_seed, seeded_rand, seeded_randn

U = 2.0 ** -24           # unit roundoff of float32
UPSTREAM = 0.37          # the decoupling tests run (0.37 * v).backward()

# ---- decoupling term -----------------------------------------------------------------------------------------------------------------
VALUE_TOL = 1e-5                                   # |v - ref| < 1e-5 |ref|
GRAD_TOL = {"f32": 2e-5, "bf16x3": 1e-4}           # every gradient, max|d| / max|ref| (test_single_tile_weight_gradients_with_many_k_slices)
HOST_SHARE = 0.25                                  # the fp32 CPU restatement holds this share of the f32 bars against fp64
MIN_COS_PRESCRIBED = 0.04
MIN_COS_RANDOM = 1e-4
RHOS = (0.9, -0.9, 0.5, -0.5, 0.1, -0.1, 0.05)
REGIME_SCALE = {"random": 1.0, "prescribed": 1.0, "small": 1e-4, "large": 1e3}

# (B, Ch, H, W) -> B*H*W*Ch % 64. 0: the workspace slots of the two adapter outputs and of their gradients are adjacent — they are carved
# in steps of 256 bytes. The backward then runs the adjoint as one convolution over 2B images (the wrapper hands out adjacent gradients)
# and the weight gradient as one launch; the forward does so only when delta_c | delta_m are adjacent in memory too (ADJACENT_SHAPES:
# halves of one buffer; the batched slab). Otherwise: two convolutions, two weight gradients and the add.
DECOUPLE_SHAPES = collections.OrderedDict([
    ((2, 8, 6, 5), 32),        # the golden's shape: two convolutions, two weight gradients + the add
    ((3, 5, 1, 1), 15),        # HW = 1, odd Ch
    ((2, 33, 1, 7), 14),       # a second channel block with one live lane; HW = 7 < 32: most pixel slices are empty
    ((1, 40, 3, 11), 40),      # HW = 33, B = 1
    ((2, 64, 4, 32), 0),       # HW = 128: exactly one unrolled round, empty remainder
    ((1, 64, 1, 129), 0),      # HW = 129: one past the unrolled round
    ((3, 40, 11, 12), 32),     # HW = 132
    ((67, 40, 2, 3), 16),      # B*Ch = 2680: one unrolled round of the mean kernel + a 632-value remainder
    ((2, 128, 8, 8), 0),       # in bf16x3: the streaming 1x1 kernel
])
BF16X3_SHAPES = [(2, 8, 6, 5), (1, 40, 3, 11), (67, 40, 2, 3), (2, 128, 8, 8)]
SMALL_SHAPE = (1, 40, 3, 11)   # gradient subsets, the all-zero sample, reproducibility
C1_SHAPE = (2, 128, 8, 8)
ADJACENT_SHAPES = [(2, 64, 4, 32), (1, 64, 1, 129)]   # f32, delta_c | delta_m halves of one buffer: one forward convolution over 2B images
# (K, B, Ch, H, W) -> K*B*Ch*H*W % 64 (the slab's halves are always adjacent; the workspace slots only at 0). "f32": two convolutions each
# way, two weight gradients and the add; "f32-joint": one convolution over 2KB images each way, one weight-gradient launch; "bf16x3": the
# streaming 1x1 kernel over the pair. The key's first word is the operand mode.
BATCHED = collections.OrderedDict([("f32", ((3, 2, 40, 3, 11), 48)), ("f32-joint", ((3, 2, 40, 4, 8), 0)), ("bf16x3", ((3, 2, 128, 8, 8), 0))])


def decouple_cases():
    """(shape, regime) of every f32 case; `random` has nothing to say on a one-pixel map."""
    return [(s, r) for s in DECOUPLE_SHAPES for r in REGIME_SCALE if not (r == "random" and s[2] * s[3] == 1)]


def adapter(Ch, seed):
    """Q diag(s) as the float32 [Ch, Ch, 1, 1] weight."""
    q, r = torch.linalg.qr(seeded_randn((Ch, Ch), seed).double())
    q = q * torch.sign(torch.diagonal(r)).unsqueeze(0)   # (the sign convention of the factorisation does not reach the matrix)
    s = 0.5 + 1.5 * seeded_rand((Ch,), seed + 1).double()
    return (q * s.unsqueeze(0)).float().reshape(Ch, Ch, 1, 1)


def _prescribed(shape, A, seed):
    B, Ch, H, W = shape
    HW = H * W
    g = torch.Generator().manual_seed(int(seed))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = rn(B, Ch, HW)
    u = u / u.norm(dim=2, keepdim=True)
    rho = torch.tensor([RHOS[i % len(RHOS)] for i in range(B * Ch)], dtype=torch.float64).reshape(B, Ch, 1)
    if HW > 1:
        z = rn(B, Ch, HW)
        z = z - (z * u).sum(2, keepdim=True) * u
        z = z / z.norm(dim=2, keepdim=True)
        v = rho * u + torch.sqrt(1.0 - rho * rho) * z
    else:
        v = torch.sign(rho) * u
    len_c = 0.5 + 1.5 * torch.rand(B, Ch, 1, generator=g, dtype=torch.float64)
    len_m = 0.5 + 1.5 * torch.rand(B, Ch, 1, generator=g, dtype=torch.float64)
    Ainv = torch.linalg.inv(A.reshape(Ch, Ch).double())
    back = lambda y: torch.einsum("io,bop->bip", Ainv, y).reshape(B, Ch, H, W).float()
    return back(len_c * u), back(len_m * v)


def decouple_inputs(shape, regime, base=0):
    """(delta_c, delta_m, adapter) in float32."""
    B, Ch, H, W = shape
    seed = name_seed(f"train_tail.decouple.{shape}", base)
    A = adapter(Ch, seed)
    if regime == "random":
        return seeded_randn(shape, seed + 2), seeded_randn(shape, seed + 3), A
    dc, dm = _prescribed(shape, A, seed + 4)
    return dc * REGIME_SCALE[regime], dm * REGIME_SCALE[regime], A


def decouple_expr(dc, dm, A):
    """predrnn_v2.py:197-198, 209-211 as oracle.torch_ref.decouple_term states it; also returns the cosines [B, Ch]."""
    B, Ch = dc.shape[:2]
    a = F.normalize(F.conv2d(dc, A).view(B, Ch, -1), dim=2)
    b = F.normalize(F.conv2d(dm, A).view(B, Ch, -1), dim=2)
    cos = torch.cosine_similarity(a, b, dim=2)
    return torch.mean(torch.abs(cos)), cos


def decouple_run(dc, dm, A, dtype=torch.float64, upstream=UPSTREAM):
    """Value, the three gradients under `upstream` and the cosines, on the CPU in `dtype`."""
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in (dc, dm, A)]
    v, cos = decouple_expr(*leaves)
    (upstream * v).backward()
    return {"value": v.detach(), "d_delta_c": leaves[0].grad, "d_delta_m": leaves[1].grad, "d_adapter": leaves[2].grad, "cos": cos.detach()}


def relmax(got, ref):
    """The suite's metric (tests/parity.py)."""
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def cancelling_terms(dc, dm, A, upstream=UPSTREAM):
    """HW = 1. d|cos| / dY_c = g (y_m / (|y_c||y_m|) - cos y_c / |y_c|^2) is the difference of two equal terms; the kernel leaves their
    rounding residue. Returns, in fp64, the first term's magnitude pulled through the adapter's adjoint — |A|^T |T|, in absolute values
    since the rounding errors of the channels do not share the terms' signs — for delta_c and delta_m, and its outer-product sum with
    the inputs for the adapter — and under "signed.*" the same with the terms' own signs, A^T T (the tighter of the two: channels may
    cancel in it, which their rounding errors need not do). The kernel is held to the signed form; the other is recorded beside it."""
    B, Ch, H, W = dc.shape
    assert H * W == 1
    A2 = A.reshape(Ch, Ch).double()
    xc, xm = dc.reshape(B, Ch).double(), dm.reshape(B, Ch).double()
    yc, ym = xc @ A2.T, xm @ A2.T
    g = upstream / (B * Ch)
    sgn = torch.sign(yc * ym)                     # sign(cos)
    Tc = g * sgn * ym / (yc.abs() * ym.abs())     # g sign(cos) y_m / (|y_c||y_m|)
    Tm = g * sgn * yc / (yc.abs() * ym.abs())
    return {"d_delta_c": (Tc.abs() @ A2.abs()).reshape(dc.shape), "d_delta_m": (Tm.abs() @ A2.abs()).reshape(dc.shape),
            "d_adapter": (Tc.abs().T @ xc.abs() + Tm.abs().T @ xm.abs()).reshape(A.shape),
            "signed.d_delta_c": (Tc @ A2).reshape(dc.shape), "signed.d_delta_m": (Tm @ A2).reshape(dc.shape),
            "signed.d_adapter": (Tc.T @ xc + Tm.T @ xm).reshape(A.shape)}


@functools.lru_cache(maxsize=None)
def decouple_case(shape, regime):
    """Inputs, the fp64 reference, the fp32 CPU restatement and the seed revision of one case: computed once, shared, never written.
    `random` takes the first revision 0, 1, ... of its seed at which no cosine of the fp64 reference is within MIN_COS_RANDOM of the
    |.| kink (a row there may flip its sign in fp32); the choice never looks at a kernel."""
    for base in range(64):
        dc, dm, A = decouple_inputs(shape, regime, base)
        ref = decouple_run(dc, dm, A)
        if regime != "random" or float(ref["cos"].abs().min()) >= MIN_COS_RANDOM:
            break
    else:
        raise AssertionError(f"decouple_case{(shape, regime)}: no seed revision below 64 keeps every cosine {MIN_COS_RANDOM} off the kink")
    cpu32 = decouple_run(dc, dm, A, torch.float32)
    if shape[2] * shape[3] == 1:   # the exact zero is the reference; autograd leaves the fp64 residue of the cancelling terms
        for k in ("d_delta_c", "d_delta_m", "d_adapter"):
            assert float(ref[k].abs().max()) < 1e-12 / min(REGIME_SCALE[regime], 1.0), (k, float(ref[k].abs().max()))
            ref[k] = torch.zeros_like(ref[k])
        ref["value"] = torch.ones_like(ref["value"])
    return (dc, dm, A), ref, cpu32, base


@functools.lru_cache(maxsize=None)
def batched_case(key):
    """K steps of B samples: the per-step inputs (prescribed regime, one adapter) and the fp64 reference of the mean of the K terms."""
    K, B, Ch, H, W = BATCHED[key][0]
    seed = name_seed(f"train_tail.batched.{key}")
    A = adapter(Ch, seed)
    steps = [_prescribed((B, Ch, H, W), A, seed + 10 + k) for k in range(K)]
    leaves = [[t.double().requires_grad_(True) for t in st] for st in steps]
    A64 = A.double().requires_grad_(True)
    v = torch.stack([decouple_expr(c, m, A64)[0] for c, m in leaves]).mean()
    (UPSTREAM * v).backward()
    ref = {"value": v.detach(), "d_adapter": A64.grad}
    for k, (c, m) in enumerate(leaves):
        ref[f"d_delta_c{k}"], ref[f"d_delta_m{k}"] = c.grad, m.grad
    return steps, A, ref


# ---- MSE -----------------------------------------------------------------------------------------------------------------------------
MSE_MAX_BLOCKS, MSE_BLOCK_ELEMS = 1024, 256 * 4      # train_tail.hip: MSE_MAX_BLOCKS, MSE_THREADS * 4 floats per block and trip
MSE_TWO_TRIPS = (1, 1, 1, 1025, 1025)                # n = 1 050 625: the second grid-stride trip, with an odd tail
MSE_FULL_TRIPS = (3, 1, 1, 700, 1000)                # n = 2 100 000: two full trips
MSE_SMALL = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 3), (1, 3, 1, 1, 5), (3, 7, 3, 9, 7)]
MSE_OFFSET_SHAPE = (1, 1, 1, 1, 4099)                # the scalar path: dense views at 1, 2, 3 floats into a larger buffer
MSE_SCALES = (1.0, 0.25, 1e3)
MSE_REGIMES = ("uniform", "identical", "offset")
MSE_LOSS_K = 4        # fl(p - t): one rounding, doubled by the square; the sum and the scaling run in double; one rounding to float
MSE_GRAD_R = 3        # fl(p - t), gscale = fl(2 scale / n_frames), their product; + 1 for the product with an upstream gradient


def mse_inputs(shape, regime):
    seed = name_seed(f"train_tail.mse.{shape}.{regime}")
    if regime == "uniform":
        return seeded_rand(shape, seed), seeded_rand(shape, seed + 1)
    if regime == "identical":
        p = seeded_rand(shape, seed)
        return p, p.clone()
    t = 1000.0 + seeded_randn(shape, seed)      # `offset`: the fp32 difference of neighbours in [2^9, 2^10] is exact (Sterbenz)
    return t + 1e-3 * seeded_randn(shape, seed + 1), t


def mse_ref(pred, target, scale, upstream=1.0):
    """scale * mean_{b,t} sum_{c,h,w} (p - t)^2 and upstream * its gradient, in float64."""
    d = pred.double() - target.double()
    nf = pred.shape[0] * pred.shape[1]
    return scale * d.pow(2).sum() / nf, (upstream * 2.0 * scale / nf) * d


# ---- flat Adam -----------------------------------------------------------------------------------------------------------------------
ADAM_MAX_BLOCKS, ADAM_BLOCK_ELEMS = 2048, 1024       # vpx_adam_step: the block cap, 256 threads * 4 floats
ADAM_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 100_003, 2_098_179)
ADAM_CAPPED = 2_098_179                              # 2048 * 1024 + 1027: the cap and a ragged tail
ADAM_ALL_SETTINGS_N = 1025
LR = 1e-3
# Roundings of adam_kernel and of the scalars vpx_adam_step rounds to float, counted against magnitudes that take no credit for
# cancellation: G = |g gs| + |wd p| for the effective gradient, M = |b1 m| + (1 - b1) G, V = b2 v + (1 - b2) G^2.
#   g'  = g gs (1) + fl(wd) p (2), the sum (1)                         -> 3 G          (1 G without weight decay; 3 is used throughout)
#   m   : fl(b1) m (2), fl(1 - b1) g' (3 + 2), the sum (1)             -> K_M = 6      against M
#   v   : fl(b2) v (2) + 1; fl(1 - b2) g' g' (2 * 3 + 3) + 1           -> K_V = 10     against V
#   upd : m (6); denom = sqrt(v) (10 / 2 + 1) / fl(sqrt(bc2)) (2) + fl(eps) (1 on its part, 1 for the sum), the quotient (1),
#         fl(lr / bc1) (1) and the product (1)                         -> K_P = 6 + 5 + 7 = 18 against step_size M / denom
#   p   : p - upd, one rounding of the result                          -> 1 against |p_ref|
# Where nothing cancels (always without weight decay) G = |g'|, V = v_ref, and these are the bounds K_M 2^-24 (|b1 m| + |(1 - b1) g|),
# K_V 2^-24 |v_ref|, 2^-24 |p_ref| + K_P 2^-24 |update| (as far as b1 m and (1 - b1) g' do not cancel in the update). Two things are added
# in adam_ref, both written out there: where g gs and wd p cancel, v_ref's relative error grows by r_v = V / v_ref >= 1, and the 5 of
# K_P that come through sqrt(v) grow with it: K_P - 5 + 5 r_v; and every bound is multiplied by 1 + 2^-18, since the counts are first
# order in 2^-24 and up to 18 roundings compound ((1 + 2^-24)^18 - 1 = 18 * 2^-24 (1 + 5e-7): far inside that factor).
K_M, K_V, K_P = 6, 10, 18


def adam_ref(p, g, m, v, step, lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """One torch.optim.Adam step (_single_tensor_adam, amsgrad = False) in float64 from the float32 p, g, m, v cast up, the scalars in
    double. Returns (p, m, v) and the element-wise bounds (dp, dm, dv) of the comments above."""
    b1, b2 = betas
    p, g, m, v = (t.double() for t in (p, g, m, v))
    ge = g * grad_scale + weight_decay * p
    G = (g * grad_scale).abs() + (weight_decay * p).abs()
    m2 = b1 * m + (1.0 - b1) * ge
    v2 = b2 * v + (1.0 - b2) * ge * ge
    M = (b1 * m).abs() + (1.0 - b1) * G
    V = b2 * v + (1.0 - b2) * G * G
    denom = v2.sqrt() / np.sqrt(1.0 - b2 ** step) + eps
    step_size = lr / (1.0 - b1 ** step)
    p2 = p - step_size * m2 / denom
    second = 1.0 + 2.0 ** -18     # (the counts are first order; 18 roundings compound to less than this)
    r_v = torch.where(v2 > 0, V / v2.clamp(min=1e-300), torch.ones_like(V))   # 1 unless g gs and wd p cancel
    bound_m = K_M * U * M * second
    bound_v = K_V * U * V * second
    bound_p = (U * p2.abs() + (K_P - 5 + 5 * r_v) * U * step_size * M / denom) * second
    return (p2, m2, v2), (bound_p, bound_m, bound_v)


def adam_state(n, tag, zero_state):
    """p, g, m, v (float32). The gradient's magnitudes run from 1e-6 to 1e3 across the bucket; the non-zero state has v >= 0."""
    seed = name_seed(f"train_tail.adam.{n}.{tag}")
    p = seeded_randn((n,), seed)
    mag = 10.0 ** (-6.0 + 9.0 * seeded_rand((n,), seed + 1))
    g = seeded_randn((n,), seed + 2) * mag
    if zero_state:
        return p, g, torch.zeros(n), torch.zeros(n)
    return p, g, seeded_randn((n,), seed + 3) * mag * 0.5, (seeded_randn((n,), seed + 4) * mag).pow(2)
