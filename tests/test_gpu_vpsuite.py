"""The workbench on the GPU (vp_suite_amd.VPSuite): a training run on "MMF" with the tiny Encoder-Forecaster of tests/golden_cases.py, its
checkpoints, and test() over a trained model, a model of another value range and frame size (both adapters run), the copy baseline and an
incompatible model."""
import json
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import measure_ref

pytestmark = pytest.mark.gpu

TINY = {k: v for k, v in gc.EF_TINY_KW.items() if k not in ("img_shape", "action_size", "tensor_value_range")}   # those come from the dataset
RUN = dict(context_frames=3, pred_frames=2)
SIZE = 32          # frames 3 x 32 x 32: SSIM needs three channels and at least 11 x 11 pixels
N_TEST = 7         # not a multiple of the test batch size 3: the last batch is ragged
VALUE_TOL, BLOCK_TOL = 1e-6, 1e-5   # the bars of tests/test_gpu_measures.py: pixel measures relative (2 x for prefix means), SSIM absolute


def _digits(vpx):
    return vpx.datasets.procedural_digits(n=10, size=12)


def _mmf(suite, vpx, split, n_seqs, channels=3):
    suite.load_dataset("MMF", split=split, digits=_digits(vpx), n_seqs=n_seqs, img_size=SIZE, num_channels=channels)


@pytest.fixture(scope="module")
def trained(vpx, tmp_path_factory):
    """(suite, output directory, returned best validation loss) of ONE two-epoch training run, shared by the tests below."""
    out = tmp_path_factory.mktemp("vpsuite_run")
    suite = vpx.VPSuite()
    assert suite.device == "cuda"
    _mmf(suite, vpx, "train", 4)
    suite.create_model("convlstm-shi", **TINY)
    assert suite.models[0].img_shape == (3, SIZE, SIZE) and suite.models[0].action_size == 0
    best = suite.train(epochs=2, batch_size=2, out_dir=str(out), **RUN)
    return suite, str(out), best


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def test_train_writes_checkpoints_and_returns_the_best_models_loss(vpx, trained):
    from vp_suite_amd.measure import PredictionLossProvider
    suite, out, best = trained
    for name in ("best_model.pth", "final_model.pth", "run_cfg.json"):
        assert os.path.isfile(os.path.join(out, name)), name
    cfg = json.load(open(os.path.join(out, "run_cfg.json")))
    assert set(cfg) == {"run", "model", "dataset", "device"} and cfg["run"]["epochs"] == 2 and cfg["model"]["NAME"] == suite.models[0].NAME
    assert np.isfinite(best) and best > 0
    # the returned value is the validation loss of the model saved as best_model.pth, on the same validation data
    suite.load_model(out)
    loaded = suite.models.pop()
    assert loaded.model_dir == out and type(loaded) is type(suite.models[0])
    val = suite.training_sets[-1].val_data
    val.reset_rng()
    config = {**RUN, "device": "cuda", "val_rec_criterion": "mse"}
    _, indicator = loaded.eval_iter(config, val.loader(1), PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}}))
    print(f"train() returned {best!r}, best_model.pth validates at {indicator.item()!r}")
    assert abs(indicator.item() - best) <= 1e-5 * abs(best)


def test_no_train_leaves_the_parameters_and_flat_adam_runs(vpx, trained, tmp_path):
    suite, _, _ = trained
    model = suite.models[0]
    before = _params(model)
    val_loss = suite.train(model_idx=0, epochs=1, batch_size=2, no_train=True, out_dir=str(tmp_path / "no_train"), **RUN)
    assert all(torch.equal(a, b) for a, b in zip(before, _params(model)))
    assert np.isfinite(val_loss) and os.path.isfile(tmp_path / "no_train" / "best_model.pth")
    # FlatAdam re-homes the parameters into flat buckets: on a model of its own, so that the shared one stays as it is
    suite.create_model("convlstm-shi", **TINY)
    flat = suite.models[-1]
    start = _params(flat)
    loss = suite.train(model_idx=-1, epochs=1, batch_size=2, flat_adam=True, out_dir=str(tmp_path / "flat"), **RUN)
    suite.models.pop()
    assert np.isfinite(loss) and any(not torch.equal(a, b) for a, b in zip(start, _params(flat)))
    assert os.path.isfile(tmp_path / "flat" / "final_model.pth")
    with pytest.raises(ValueError, match="has to be one of the chosen losses"):
        suite.train(epochs=1, batch_size=2, val_rec_criterion="l1", out_dir=str(tmp_path / "bad"), **RUN)


@pytest.fixture(scope="module")
def tested(vpx, trained):
    """test() with batches of three and of one over the same 7 sequences: the trained model, a model of value range [-1, 1] at 16 x 16
    (both adapters run) and the copy baseline."""
    suite, _, _ = trained
    _mmf(suite, vpx, "test", N_TEST)
    suite.create_model("convlstm-shi", img_shape=(3, 16, 16), tensor_value_range=[-1.0, 1.0], **TINY)
    calls = []
    real = vpx.ops.frames_adapt

    def counting(x, out_hw=None, src_range=(0.0, 1.0), dst_range=(0.0, 1.0)):
        calls.append((tuple(x.shape), out_hw, tuple(src_range), tuple(dst_range)))
        return real(x, out_hw, src_range, dst_range)

    vpx.ops.frames_adapt = counting
    try:
        by3 = suite.test(test_batch_size=3, **RUN)
    finally:
        vpx.ops.frames_adapt = real
    by1 = suite.test(test_batch_size=1, **RUN)
    suite.models.pop()
    return suite, by3, by1, calls


def test_test_runs_both_adapters_once_per_batch_and_direction(vpx, tested):
    suite, by3, _, calls = tested
    name = suite.test_sets[0].NAME
    assert list(by3) == [name]
    ef = suite.models[0].NAME
    assert list(by3[name]) == [ef, f"{ef} #1", "CopyLastFrame"]
    assert all(len(rows) == RUN["pred_frames"] and list(rows[0]) == ["mse (↓)", "psnr (↑)", "ssim (↑)"] for rows in by3[name].values())
    # three batches (3 + 3 + 1), one launch into and one out of the second model each; the first model and the baseline need none
    pre = [c for c in calls if c[1] == (16, 16)]
    post = [c for c in calls if c[1] == (SIZE, SIZE)]
    assert len(calls) == 6 and len(pre) == 3 and len(post) == 3
    assert [c[0][0] for c in pre] == [3, 3, 1] and all(c[2:] == ((0.0, 1.0), (-1.0, 1.0)) and c[0][1:] == (3, 3, SIZE, SIZE) for c in pre)
    assert all(c[2:] == ((-1.0, 1.0), (0.0, 1.0)) and c[0][1:] == (2, 3, 16, 16) for c in post)


def test_copy_baseline_metrics_equal_the_plain_torch_expressions(vpx, tested):
    suite, by3, _, _ = tested
    ds = suite.test_sets[0].test_data
    ds.reset_rng()
    frames = ds.batch(N_TEST)["frames"].cpu()
    context, target = frames[:, :3], frames[:, 3:5]
    pred = context[:, -1:].expand(-1, 2, -1, -1, -1)
    rows = by3[ds.NAME]["CopyLastFrame"]
    for n, row in enumerate(rows, start=1):
        ref = measure_ref.measures(pred[:, :n], target[:, :n], keys=("mse", "psnr", "ssim"))
        for k, label in (("mse", "mse (↓)"), ("psnr", "psnr (↑)"), ("ssim", "ssim (↑)")):
            want = float(measure_ref.display(k, ref[k]))
            print(f"horizon {n} {k}: test() {row[label]!r}, plain torch {want!r}")
            assert abs(row[label] - want) < (BLOCK_TOL if k == "ssim" else 2 * VALUE_TOL * abs(want)), (n, k, row[label], want)


def test_batches_of_three_and_of_one_agree(vpx, tested):
    _, by3, by1, _ = tested
    (models3,), (models1,) = by3.values(), by1.values()
    assert list(models3) == list(models1)
    for name in models3:
        for n, (a, b) in enumerate(zip(models3[name], models1[name]), start=1):
            for k in a:
                print(f"{name} horizon {n} {k}: {a[k]!r} (batches of 3) {b[k]!r} (batches of 1)")
                assert abs(a[k] - b[k]) <= 1e-6 * abs(b[k]), (name, n, k, a[k], b[k])


def test_brief_test_and_an_incompatible_model_is_skipped(vpx, trained, capsys):
    """A 3-channel model against a 1-channel set is skipped with a message; the set is still tested with the copy baseline."""
    suite, _, _ = trained
    gray = vpx.VPSuite()
    gray.models.append(suite.models[0])
    gray.load_dataset("MMF", split="test", digits=_digits(vpx), n_seqs=12, img_size=SIZE, num_channels=1)
    out = gray.test(brief_test=True, test_batch_size=4, metrics=["mse", "psnr"], **RUN)
    said = capsys.readouterr().out
    assert "skipping test of model" in said and "1-channel images" in said
    (models,) = out.values()
    assert list(models) == ["CopyLastFrame"] and len(models["CopyLastFrame"]) == 2
    # brief: 10 of the 12 datapoints (4 + 4 + 2 of the third batch)
    ds = gray.test_sets[0].test_data
    ds.reset_rng()
    frames = ds.batch(12)["frames"][:10].cpu()
    ref = measure_ref.measures(frames[:, 2:3].expand(-1, 2, -1, -1, -1), frames[:, 3:5], keys=("mse",))
    assert abs(models["CopyLastFrame"][1]["mse (↓)"] - float(ref["mse"])) < 2 * VALUE_TOL * float(ref["mse"])
