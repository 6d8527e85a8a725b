"""The conditions on the inputs of tests/test_gpu_train_tail.py, checked on the CPU: every decoupling case is conditioned well enough to
judge a kernel by (so that a failing GPU test means the kernel), the fp64 restatements of tests/train_tail_ref.py agree with the
oracle's, and the case tables reach what they claim to reach."""
import numpy as np
import pytest
import torch

import train_tail_ref as R

_ids = lambda c: "x".join(map(str, c[0])) + "-" + c[1]


@pytest.mark.parametrize("case", R.decouple_cases(), ids=_ids)
def test_decouple_case_conditions(case):
    shape, regime = case
    (dc, dm, A), ref, cpu32, base = R.decouple_case(shape, regime)
    assert dc.dtype == dm.dtype == A.dtype == torch.float32
    for t in (dc, dm, A, *ref.values(), *cpu32.values()):
        assert bool(torch.isfinite(t).all())
    hw1 = shape[2] * shape[3] == 1
    # the fp32 CPU restatement holds a quarter of the f32 bars against fp64
    verr = abs(float(cpu32["value"]) - float(ref["value"])) / abs(float(ref["value"]))
    assert verr <= R.HOST_SHARE * R.VALUE_TOL, verr
    worst = 0.0
    if not hw1:   # (HW = 1: the reference is the exact zero, and the fp32 restatement's residue is what the GPU test bounds)
        for k in ("d_delta_c", "d_delta_m", "d_adapter"):
            worst = max(worst, R.relmax(cpu32[k], ref[k]))
        assert worst <= R.HOST_SHARE * R.GRAD_TOL["f32"], worst
    # no row near the |.| kink, none left out
    mincos = float(ref["cos"].abs().min())
    floor = R.MIN_COS_RANDOM if regime == "random" else R.MIN_COS_PRESCRIBED
    assert mincos >= floor, mincos
    assert float((ref["cos"].abs() < floor).double().mean()) == 0.0
    assert bool((torch.sign(cpu32["cos"]) == torch.sign(ref["cos"])).all())
    if regime != "random" and not hw1:   # the rows have the cosines they were given (the inputs were rounded to float32 on the way)
        rho = torch.tensor([R.RHOS[i % len(R.RHOS)] for i in range(shape[0] * shape[1])], dtype=torch.float64).reshape(shape[:2])
        assert float((ref["cos"] - rho).abs().max()) < 1e-5
    if hw1:
        assert float((ref["cos"].abs() - 1.0).abs().max()) < 1e-12
    print(f"decouple {shape} {regime}: seed revision {base}, min|cos| {mincos:.2e}, fp32 restatement value {verr:.1e} gradients {worst:.1e}")


@pytest.mark.parametrize("key", list(R.BATCHED))
def test_batched_case_is_the_mean_of_its_steps(key):
    steps, A, ref = R.batched_case(key)
    K = R.BATCHED[key][0][0]
    assert len(steps) == K
    per_step = [R.decouple_run(c, m, A) for c, m in steps]
    assert abs(float(ref["value"]) - np.mean([float(r["value"]) for r in per_step])) < 1e-14
    for k, r in enumerate(per_step):
        assert float(r["cos"].abs().min()) >= R.MIN_COS_PRESCRIBED
        assert R.relmax(ref[f"d_delta_c{k}"] * K, r["d_delta_c"]) < 1e-12
    assert R.relmax(ref["d_adapter"] * K, sum(r["d_adapter"] for r in per_step)) < 1e-12


def test_zero_sample_has_zero_gradients_in_the_reference():
    """delta_c[0] = 0: cos = 0 on those rows, sign(0) = 0, and everything stays finite."""
    (dc, dm, A), _, _, _ = R.decouple_case(R.SMALL_SHAPE, "prescribed")
    B, Ch = 2, R.SMALL_SHAPE[1]
    dc2 = torch.cat([torch.zeros_like(dc), dc])
    dm2 = torch.cat([dm, dm])
    ref = R.decouple_run(dc2, dm2, A)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    assert not ref["cos"][0].any() and not ref["d_delta_c"][0].any() and not ref["d_delta_m"][0].any()
    one = R.decouple_run(dc, dm, A)
    assert abs(float(ref["value"]) - float(one["value"]) / B) < 1e-15
    assert R.relmax(ref["d_adapter"] * B, one["d_adapter"]) < 1e-12


def test_restatements_agree_with_the_oracle():
    from oracle import torch_ref as tr
    dc, dm, A = R.decouple_inputs((2, 8, 6, 5), "random")
    assert float(R.decouple_expr(dc.double(), dm.double(), A.double())[0]) == float(tr.decouple_term(dc.double(), dm.double(), A.double()))
    shape = (3, 7, 3, 9, 7)
    p, t = R.mse_inputs(shape, "uniform")
    loss, grad = R.mse_ref(p, t, 1.0)
    p64 = p.double().requires_grad_(True)
    want = tr.mse_measure(p64, t.double())
    want.backward()
    assert abs(float(loss) - float(want.detach())) <= 1e-14 * float(loss) and R.relmax(grad, p64.grad) < 1e-14
    n = 1025
    p, g, m, v = R.adam_state(n, "host", zero_state=False)
    (p2, m2, v2), (bp, bm, bv) = R.adam_ref(p, g, m, v, 7, weight_decay=0.01, grad_scale=0.5)
    rp, rm, rv = tr.adam_step_ref(p.numpy(), g.numpy(), m.numpy(), v.numpy(), 7, R.LR, weight_decay=0.01, grad_scale=0.5)
    # the oracle's restatement runs in float32: it lies within the element-wise bounds the kernel is held to
    for got, want, bound in ((rp, p2, bp), (rm, m2, bm), (rv, v2, bv)):
        assert bool(((torch.from_numpy(got).double() - want).abs() <= bound).all())
    opt_p = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([opt_p], lr=R.LR, weight_decay=0.01)
    opt.state[opt_p] = {"step": torch.tensor(6.0), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    opt_p.grad = g.double() * 0.5
    opt.step()
    assert R.relmax(opt_p.detach(), p2) < 1e-13
    assert R.relmax(opt.state[opt_p]["exp_avg"], m2) < 1e-13 and R.relmax(opt.state[opt_p]["exp_avg_sq"], v2) < 1e-13


def test_case_tables_reach_what_they_claim():
    for (B, Ch, H, W), rem in R.DECOUPLE_SHAPES.items():
        assert B * H * W * Ch % 64 == rem, (B, Ch, H, W)
    adjacent = [s for s, rem in R.DECOUPLE_SHAPES.items() if rem == 0]
    assert adjacent == [(2, 64, 4, 32), (1, 64, 1, 129), (2, 128, 8, 8)]
    assert sorted(s[2] * s[3] for s in R.DECOUPLE_SHAPES) == [1, 6, 7, 30, 33, 64, 128, 129, 132]
    assert 67 * 40 == 2048 + 632 and set(R.BF16X3_SHAPES) <= set(R.DECOUPLE_SHAPES)
    assert set(R.ADJACENT_SHAPES) <= set(adjacent) and all(s[1] != 128 for s in R.ADJACENT_SHAPES)
    for key, ((K, B, Ch, H, W), rem) in R.BATCHED.items():
        assert (K, B) == (3, 2) and Ch == (40 if key.startswith("f32") else 128)
        assert K * B * Ch * H * W % 64 == rem, key
    assert [rem for _, rem in R.BATCHED.values()] == [48, 0, 0]   # f32: both forms of the adapter pair; bf16x3: the streaming kernel's
    # restated here: MSE_MAX_BLOCKS (1024) blocks of MSE_THREADS (256) * 4 floats in csrc/train_tail.hip::vpx_mse_loss; the cap of
    # 2048 blocks of 256 threads * 4 floats in vpx_adam_step
    MSE_ONE_TRIP, ADAM_ONE_TRIP = 1024 * 1024, 2048 * 1024
    assert (R.MSE_MAX_BLOCKS * R.MSE_BLOCK_ELEMS, R.ADAM_MAX_BLOCKS * R.ADAM_BLOCK_ELEMS) == (MSE_ONE_TRIP, ADAM_ONE_TRIP)
    n2 = int(np.prod(R.MSE_TWO_TRIPS))
    assert n2 == 1_050_625 and MSE_ONE_TRIP < n2 < 2 * MSE_ONE_TRIP and n2 % 4 == 1
    n3 = int(np.prod(R.MSE_FULL_TRIPS))
    assert n3 == 2_100_000 and n3 > 2 * MSE_ONE_TRIP
    assert R.ADAM_CAPPED == ADAM_ONE_TRIP + 1027 and max(R.ADAM_SIZES) == R.ADAM_CAPPED and R.ADAM_CAPPED % 4 == 3
    assert int(np.prod(R.MSE_OFFSET_SHAPE)) == 4099


def test_offset_regime_difference_is_exact_in_fp32():
    p, t = R.mse_inputs((3, 7, 3, 9, 7), "offset")
    assert torch.equal((p - t).double(), p.double() - t.double())
    assert float((p - t).abs().max()) > 1e-3
