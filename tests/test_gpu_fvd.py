"""FVD end to end on the GPU: the I3D trunk (ops.fvd_features) against the float64 host restatement at thin and at the real widths, the
measure and the providers. The trunk's bar is measured, not chosen: the float32 CPU chain's own error against float64 on the same inputs,
times 4, with a floor of 1e-6 of max|ref| (the rule of tests/test_gpu_lpips_taps.py). With VPX_FVD_PARITY_OUT=FILE in the environment
every figure of this module and of tests/test_gpu_fvd_kernels.py is written there when the run ends (tests/fvd_ref.py: record; how
profiles/fvd_parity.json was made)."""
import os

import pytest
import torch

import fvd_ref
from vp_suite_amd import measure as M
from vp_suite_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN, FLOOR = 4.0, 1e-6
_record = fvd_ref.record


@pytest.fixture
def thin():
    M.register_fvd_weights(fvd_ref.state_dict())
    yield M.fvd_weights(DEV)
    M.clear_fvd_weights()


def _host_chains(clips):
    """(float64 features, the float32 CPU chain's error against them, the bar) of a clip batch on the registered network."""
    ref = M._fvd_features_host(clips.double(), M.fvd_weights("cpu", torch.float64))
    err32 = fvd_ref.relmax(M._fvd_features_host(clips, M.fvd_weights("cpu")), ref)
    return ref, err32, max(MARGIN * err32, FLOOR)


@pytest.mark.parametrize("T", (9, 12, 16))
def test_thin_trunk_against_float64(thin, T, parity_log):
    pred, target = fvd_ref.clips((2, T, 3, 20, 28), seed=T)
    ref, err32, bound = _host_chains(torch.cat([pred, target]))
    assert float(ref.abs().max()) >= 1.0          # features of a size at which a relative figure means something
    p, t = pred.to(DEV), target.to(DEV)
    got = ops.fvd_features(p, thin, t)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 50)
    err = parity_log(f"fvd_features thin T={T}", got.cpu(), ref, bound)
    print(f"thin trunk T={T}: max|ref| {float(ref.abs().max()):.3f}, float32 CPU chain {err32:.3e}, bound {bound:.3e}, HIP {err:.3e}")
    _record(f"thin T={T}", reference_error=err32, bound=bound, hip=err, max_ref=float(ref.abs().max()))
    assert err <= bound
    assert torch.equal(ops.fvd_features(p, thin, t), got)                                       # repeat calls are bit-equal
    assert torch.equal(ops.fvd_features(p, thin), got[:2]) and torch.equal(ops.fvd_features(t, thin), got[2:])   # and so are the halves
    if T == 9:   # the staging resize is ops.frames_adapt's, bit for bit: clips resized beforehand (and then only copied) give the same bits
        assert torch.equal(ops.fvd_features(ops.frames_adapt(p, (224, 224)), thin, ops.frames_adapt(t, (224, 224))), got)
    for bad in (8, 17):
        with pytest.raises(ValueError, match="2x7x7"):
            ops.fvd_features(torch.zeros(1, bad, 3, 20, 28, device=DEV), thin)
    with pytest.raises(ValueError, match="channels"):
        ops.fvd_features(torch.zeros(1, 9, 2, 20, 28, device=DEV), thin)


def test_real_width_trunk_against_float64(parity_log):
    M.register_fvd_weights(fvd_ref.state_dict(1))
    try:
        clip, _ = fvd_ref.clips((1, 9, 3, 20, 28), seed=77)
        ref, err32, bound = _host_chains(clip)
        got = ops.fvd_features(clip.to(DEV), M.fvd_weights(DEV))
        assert tuple(got.shape) == (1, 400)
        err = parity_log("fvd_features real widths T=9", got.cpu(), ref, bound)
        print(f"real widths T=9: max|ref| {float(ref.abs().max()):.3f}, float32 CPU chain {err32:.3e}, bound {bound:.3e}, HIP {err:.3e}")
        _record("real widths T=9", reference_error=err32, bound=bound, hip=err, max_ref=float(ref.abs().max()))
        assert err <= bound
    finally:
        M.clear_fvd_weights()


def _carried(fp, ft, delta):
    """What an error of at most `delta` in every feature can move the distance by. With A^2 = fact sum Ep^2, B^2 = fact sum Et^2, m = |mu_p - mu_t|
    and a, m' the same figures of the error itself (a <= sqrt(fact b n) 2 delta: centring can double it; m' <= sqrt(n) 2 delta): A^2 and B^2 move by at
    most 2 A a + a^2 and 2 B a + a^2, m^2 by 2 m m' + m'^2, and twice the nuclear norm of fact Ep Et^T (at most A B) by 2 (a B + A a + a^2)."""
    b, n = fp.shape
    fact = 1.0 if b < 2 else 1.0 / (b - 1)
    p, t = fp.double(), ft.double()
    A, B = float((fact * (p - p.mean(0)).square().sum()).sqrt()), float((fact * (t - t.mean(0)).square().sum()).sqrt())
    m = float((p.mean(0) - t.mean(0)).norm())
    a, m1 = (fact * b * n) ** 0.5 * 2 * delta, n ** 0.5 * 2 * delta
    return 4 * a * (A + B) + 4 * a * a + 2 * m * m1 + m1 * m1 + fvd_ref.frechet_bound(fp, ft)


@pytest.mark.parametrize("T", (10, 20))
def test_measure_against_the_host_restatement(thin, T):
    pred, target = fvd_ref.clips((2, T, 3, 20, 28), seed=100 + T)
    m = M.FrechetVideoDistance(DEV)
    chunks = M.fvd_chunks(T)
    assert chunks == [(s, 10) for s in range(0, T, 10)]
    want, bound, same_bound = 0.0, 0.0, 0.0
    for first, length in chunks:
        ref, err32, bar = _host_chains(torch.cat([pred[:, first:first + length], target[:, first:first + length]]))
        want += float(M.frechet_distance_host(ref[:2], ref[2:])) / len(chunks)
        bound += _carried(ref[:2], ref[2:], bar * float(ref.abs().max())) / len(chunks)
        same_bound += fvd_ref.frechet_bound(ref[:2], ref[:2]) / len(chunks)
    got = m(pred.to(DEV), target.to(DEV))
    print(f"FVD T={T}: host float64 {want:.6e}, HIP {float(got):.6e}, |delta| {abs(float(got) - want):.3e}, carried bound {bound:.3e}")
    _record(f"measure T={T}", host=want, hip=float(got), bound=bound)
    assert got.dtype == torch.float32 and got.is_cuda and got.ndim == 0
    assert abs(float(got) - want) <= bound + 2.0 ** -23 * abs(want)                       # (the value is handed out in float32)
    same = m(pred.to(DEV), pred.to(DEV))   # identical sets: |d| <= 2 b sqrt(1e-15) plus the rounding of the positive terms
    assert abs(float(same)) <= same_bound, float(same)


def test_distance_against_the_recorded_reference():
    """calculate_2_wasserstein_dist as recorded (tests/golden/fvd_wasserstein.npz) next to its own deviation from the float64 singular-value
    form on the same inputs: its non-symmetric eigvals is noisy and it returns float32. The HIP value is held to 2 x that deviation plus
    its own float64 bound against the form (fvd_ref.frechet_bound)."""
    import numpy as np
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fvd_wasserstein.npz")) as z:
        rec = {k: z[k] for k in z.files}
    figures = {}
    for b, n, kind in fvd_ref.WASSERSTEIN_CASES:
        p, t = fvd_ref.feature_tables(b, n, kind)
        ref, dev = (float(v) for v in rec[f"{b}_{n}_{kind}"])
        got = float(ops.frechet_distance(p.to(DEV), t.to(DEV)))
        figures[f"b={b} n={n} {kind}"] = {"reference": ref, "reference_deviation": dev, "hip_minus_reference": got - ref}
        assert abs(got - ref) <= 2 * dev + fvd_ref.frechet_bound(p, t), (b, n, kind, got, ref, dev)
    _record("distance against the recorded reference", **figures)


def test_measure_and_providers(thin):
    pred, target = fvd_ref.clips((2, 10, 3, 20, 28), seed=5)
    p, t = pred.to(DEV), target.to(DEV)
    m = M.FrechetVideoDistance(DEV)
    assert m(p[:, :8], t[:, :8]) is None
    with pytest.raises(ValueError, match="not equal"):
        m(p, t[:, :9])
    every = M.PredictionMetricProvider({"device": DEV, "metrics": ["mse", "fvd"]}).get_metrics(p, t, all_frame_cnts=True)
    assert len(every) == 10 and [("fvd (↓)" in d) for d in every] == [False] * 8 + [True, True] and all("mse (↓)" in d for d in every)
    assert every[9]["fvd (↓)"] == pytest.approx(float(m(p, t)), rel=1e-6) and every[8]["fvd (↓)"] == pytest.approx(float(m(p[:, :9], t[:, :9])), rel=1e-6)
    disp, total = M.PredictionLossProvider({"device": DEV, "losses_and_scales": {"mse": 1.0, "fvd": 0.5}}).get_losses(p, t)
    assert float(disp["fvd"]) == pytest.approx(float(m(p, t)), rel=1e-6) and float(total) == pytest.approx(float(disp["mse"]) + 0.5 * float(disp["fvd"]), rel=1e-5)
    q = p.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="forward only"):
        m(q, t)
    with torch.no_grad():
        assert float(m(q, t)) == float(m(p, t))


def test_workbench_reports_fvd(vpx, thin):
    """suite.test(metrics=["mse", "fvd"]): every horizon keeps its own keys, "fvd" has a value from 9 predicted frames on."""
    import golden_cases as gc
    tiny = {k: v for k, v in gc.EF_TINY_KW.items() if k not in ("img_shape", "action_size", "tensor_value_range")}   # those come from the dataset
    suite = vpx.VPSuite()
    suite.load_dataset("MMF", split="test", digits=vpx.datasets.procedural_digits(n=10, size=12), n_seqs=3, img_size=32, num_channels=3)
    suite.create_model("convlstm-shi", **tiny)   # (test() wants a model; the copy baseline is evaluated beside it)
    results = suite.test(metrics=["mse", "fvd"], test_batch_size=2, context_frames=2, pred_frames=9)   # batches of 2 and 1 datapoints
    (per_model,) = results.values()
    assert "CopyLastFrame" in per_model
    for horizons in per_model.values():
        assert len(horizons) == 9 and all(list(h) == ["mse (↓)"] for h in horizons[:8])
        assert list(horizons[8]) == ["mse (↓)", "fvd (↓)"] and 0 <= horizons[8]["fvd (↓)"] < float("inf")
