"""bench.py's run forms: a plain run (the headline only), --full (roofline, CPU baseline, extras), --dump-outputs DIR."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod_forms", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _run(*args):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=400, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_plain_run_reports_the_headline_only():
    """A plain run times the headline and nothing else; --full brings the roofline of the same timed steps back."""
    plain = _run("--stub", "--steps", "5", "--warmup", "1")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 5 and plain["warmup"] == 1 and plain["higher_is_better"] is True
    assert not {"roofline", "cpu_baseline", "extras", "extras_file"} & set(plain)
    assert plain["value"] == pytest.approx(128 * 10 / (plain["ms_per_step"] * 1e-3), rel=1e-3)
    full = _run("--stub", "--steps", "5", "--warmup", "1", "--full")
    assert full["roofline"]["bound"] == "mfma" and full["steps"] == 5


def test_bench_dump_outputs_budget_and_fixed_sample(tmp_path):
    """Outputs fit in 64 MB: arrays below their share are written whole in their shape, a larger one as the same seeded 1-D
    sample every time; float64 stays float64, every other dtype becomes float32."""
    bench = _bench_module()
    g = torch.Generator().manual_seed(3)
    arrays = {"big": torch.randn(20_000_000, generator=g), "small": torch.arange(10.0).reshape(2, 5),
              "wide": torch.randn(7, dtype=torch.float64, generator=g), "model loss": torch.tensor(0.5, dtype=torch.bfloat16)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(arrays, str(a))
    bench.dump_outputs(arrays, str(b))
    files = sorted(os.listdir(a))
    assert files == ["big.npy", "model_loss.npy", "small.npy", "wide.npy"]
    assert sum(os.path.getsize(a / f) for f in files) <= 64 * 2 ** 20
    small, wide, big = np.load(a / "small.npy"), np.load(a / "wide.npy"), np.load(a / "big.npy")
    assert small.dtype == np.float32 and np.array_equal(small, np.arange(10.0, dtype=np.float32).reshape(2, 5))
    assert wide.dtype == np.float64 and np.array_equal(wide, arrays["wide"].numpy())
    assert np.load(a / "model_loss.npy").shape == () and float(np.load(a / "model_loss.npy")) == 0.5
    assert big.dtype == np.float32 and big.ndim == 1 and 1_000_000 < big.size < 20_000_000
    assert np.isin(big[:100], arrays["big"].numpy()).all()
    assert all(np.array_equal(np.load(a / f), np.load(b / f)) for f in files)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_dump_outputs_repeat_run_for_run(tmp_path):
    """Same arguments, same outputs: the inference step's predictions, and the training step's loss and parameters even when the
    clock-dependent prewarm ran a different number of steps before the timed ones."""
    common = ("--batch", "4", "--steps", "2", "--warmup", "1")
    for mode, prewarms in (("infer", ("0.2", "0.2")), ("train", ("0", "0.5"))):
        dirs = [tmp_path / f"{mode}_{i}" for i in range(2)]
        for d, pw in zip(dirs, prewarms):
            line = _run(*common, "--mode", mode, "--prewarm", pw, "--dump-outputs", str(d))
            assert line["steps"] == 2 and line["ms_per_step"] > 0 and "roofline" not in line
        names = sorted(os.listdir(dirs[0]))
        assert names == sorted(os.listdir(dirs[1]))
        assert names == (["loss.npy", "parameters.npy"] if mode == "train" else ["predictions.npy"])
        for n in names:
            x, y = np.load(dirs[0] / n), np.load(dirs[1] / n)
            assert x.dtype == np.float32 and np.isfinite(x).all()
            assert np.abs(x - y).max() <= 1e-6 * max(1.0, float(np.abs(y).max())), (mode, n)
        if mode == "infer":
            assert np.load(dirs[0] / "predictions.npy").shape == (4, 10, 1, 64, 64)
