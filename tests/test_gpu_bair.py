"""Stored sequences that carry actions, on the GPU: ops.actions_gather (csrc/frames.hip, vpx_actions_gather) against the numpy restatement
(tests/bair_ref.py) bit for bit, StoredVPDataset(actions=...) in both storage modes, DATASET_CLASSES["BAIR"] against the fixture drawn
from the upstream class (tests/golden/bair_stored.npz), and the workbench's quick-start sequence with an action-conditional PredRNN++
that must really receive the dataset's actions. No speed figure: the gather moves a few kilobytes."""
import os
import sys

import numpy as np
import pytest
import torch

import bair_ref as R
from golden_util import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_bair_like  # noqa: E402

pytestmark = pytest.mark.gpu

N, TP = 7, 30
F32_MAX = float(np.finfo(np.float32).max)
# float64 values float32 cannot hold: ties (to even: down, up), next to the largest float32 (rounds to it), inexact, the subnormal range
SPECIAL_F64 = [1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -(1.0 + 2.0 ** -24), F32_MAX * (1.0 - 2.0 ** -26), -F32_MAX * (1.0 - 2.0 ** -26), 0.1, 1e-40,
               -0.75 * 2.0 ** -149, 2.0 ** -150, -0.0]
SPECIAL_F32 = [-0.0, np.inf, -np.inf, np.nan, 1e-40, F32_MAX]


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _stored_actions(A, dtype, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(size=(N, TP, A)).astype(dtype)
    special = SPECIAL_F64 if dtype == np.float64 else SPECIAL_F32
    flat = a.reshape(-1)
    flat[:len(special) * 3:3] = np.array(special, dtype=dtype)        # scattered over the first rows of sequence 0, whatever A is
    return a


def _seq_lists(n_frames, A):
    many = -(-257 // (n_frames * A))                                  # B * n_frames * A passes one block of 256 threads
    descending = [N - 1 - (i % N) for i in range(max(many, N + 2))]   # descending, and repeated once it wraps
    return [[0], [N - 1], [4, 4, 1], [0] + descending]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_frames,seq_step", [(30, 1), (15, 2), (10, 3), (1, 1)])
@pytest.mark.parametrize("A", [1, 4, 5])
def test_actions_gather_equals_the_restatement_bit_for_bit(vpx, A, n_frames, seq_step, dtype):
    host = _stored_actions(A, dtype, 100 * A + n_frames)
    dev = torch.from_numpy(host).cuda()
    with np.errstate(over="ignore"):
        for seqs in _seq_lists(n_frames, A):
            want = R.gather(host, seqs, n_frames, seq_step)
            table = np.array([[s, 0, 0, 0] for s in seqs], dtype=np.int32)
            got = vpx.ops.actions_gather(dev, table, n_frames, seq_step)
            assert got.dtype == torch.float32 and tuple(got.shape) == (len(seqs), n_frames, A) and got.is_cuda
            got = got.cpu().numpy()
            differ = int((_bits(got) != _bits(want)).sum())
            print(f"A={A} F={n_frames} step={seq_step} {np.dtype(dtype).name} B={len(seqs)}: {differ} of {want.size} elements differ in their bits")
            assert differ == 0
    if len(_seq_lists(n_frames, A)[-1]) * n_frames * A <= 256:
        pytest.fail("the largest table does not pass one block")


def test_actions_gather_special_values_and_table_columns(vpx):
    """The float64 values that float32 cannot hold land on the float32 numpy's astype gives (ties to even, the largest float32, subnormals);
    float32 storage is copied bit for bit; columns 1-3 of the table (box, flips) are not read; a device table is taken as it is."""
    for dtype, special in ((np.float64, SPECIAL_F64), (np.float32, SPECIAL_F32)):
        host = np.zeros((2, 4, len(special)), dtype=dtype)
        host[1, 2] = special
        want = host[1, 2].astype(np.float32)
        table = np.array([[1, 7, 9, 3]], dtype=np.int32)
        got = vpx.ops.actions_gather(torch.from_numpy(host).cuda(), table, 2, 2).cpu().numpy()
        print(f"{np.dtype(dtype).name}: {got[0, 1].tolist()}")
        assert np.array_equal(_bits(got[0, 1]), _bits(want)) and not _bits(got[0, 0]).any()
        again = vpx.ops.actions_gather(torch.from_numpy(host).cuda(), torch.from_numpy(table).cuda(), 2, 2).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(got))
    tie = vpx.ops.actions_gather(torch.tensor([[[1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24]]], dtype=torch.float64).cuda(), np.zeros((1, 4), dtype=np.int32), 1, 1)
    assert tie.cpu().tolist() == [[[1.0, 1.0 + 2.0 ** -22]]]


def test_actions_gather_refusals(vpx):
    a = torch.zeros((3, 6, 4), dtype=torch.float32).cuda()
    table = np.array([[2, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    assert tuple(vpx.ops.actions_gather(a, table, 3, 2).shape) == (2, 3, 4)
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        vpx.ops.actions_gather(a.cpu(), table, 3, 2)
    for bad, word in ((a[0], r"\[N, T', A\]"), (a[..., None], r"\[N, T', A\]"), (a[:, :, :0], r"\[N, T', A\]"), (a.to(torch.float16), "float32 and float64"),
                      (a.to(torch.int32), "float32 and float64")):
        with pytest.raises(ValueError, match=word):
            vpx.ops.actions_gather(bad, table, 3, 2)
    for F, step in ((7, 1), (4, 2), (2, 6)):
        with pytest.raises(ValueError, match="stored frames"):
            vpx.ops.actions_gather(a, table, F, step)
    for F, step in ((0, 1), (1, 0)):
        with pytest.raises(ValueError, match=">= 1"):
            vpx.ops.actions_gather(a, table, F, step)
    for rows, word in (([[3, 0, 0, 0]], "sequence index"), ([[-1, 0, 0, 0]], "sequence index"), ([[0, 0, 0]], "integer table"), ([[0.0, 0, 0, 0]], "integer table")):
        with pytest.raises(ValueError, match=word):
            vpx.ops.actions_gather(a, np.array(rows), 3, 2)
    with pytest.raises(ValueError, match="device table"):
        vpx.ops.actions_gather(a, torch.zeros((2, 4), dtype=torch.int64).cuda(), 3, 2)


@pytest.mark.parametrize("storage", ["device", "pinned"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_stored_dataset_returns_its_actions_in_both_storage_modes(vpx, storage, dtype):
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, size=(N, TP, 9, 10, 3), dtype=np.uint8)
    actions = _stored_actions(5, dtype, 77)
    augs = [("hflip", 0.5), ("vflip", 0.5), ("invert", 0.5), ("erase", 1.0, (0.1, 0.3), (0.5, 2.0), 0.0)]
    kw = dict(raw=raw, storage=storage, crop=("random", 6, 7), augmentations=augs, transform_seed=11)
    ds = vpx.datasets.StoredVPDataset("train", actions=actions, **kw)
    plain = vpx.datasets.StoredVPDataset("train", **kw)
    for ctx, pred, step, batches in ((3, 2, 2, ([5, 0, 5], [1], [6, 5, 4, 3, 2])), (10, 20, 1, ([0, 6],)), (1, 0, 1, ([3],))):
        ds.set_seq_len(ctx, pred, step)
        plain.set_seq_len(ctx, pred, step)
        for indices in batches:
            data, bare = ds.batch(indices), plain.batch(indices)
            want = R.gather(actions, indices, ctx + pred, step)
            assert data["actions"].dtype == torch.float32 and data["actions"].is_cuda and data["origin"] == bare["origin"]
            assert np.array_equal(_bits(data["actions"].cpu().numpy()), _bits(want))
            # crops, flips and photometric entries never touch the actions, and the actions change neither the draws nor the frames
            assert torch.equal(data["frames"], bare["frames"])
            assert tuple(bare["actions"].shape) == (len(indices), ctx + pred, 1) and not bare["actions"].any()
    ds.set_seq_len(3, 2, 2)
    ds.reset_rng()
    whole = ds.batch([2, 6, 2])
    ds.reset_rng()
    singles = [ds[i] for i in (2, 6, 2)]
    assert torch.equal(whole["actions"], torch.stack([s["actions"] for s in singles])) and torch.equal(whole["frames"], torch.stack([s["frames"] for s in singles]))
    assert tuple(singles[0]["actions"].shape) == (5, 5) and whole["origin"] == [s["origin"] for s in singles]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "bair_stored.npz"))


@pytest.mark.parametrize("storage", ["device", "pinned"])
def test_bair_batches_against_the_upstream_fixture(vpx, golden, tmp_path, storage):
    obs, actions = golden["obs"], golden["actions"]
    export_bair_like.write_split(str(tmp_path), "train", obs, actions)
    ds = vpx.datasets.DATASET_CLASSES["BAIR"]("train", data_dir=str(tmp_path), storage=storage)
    plain = vpx.datasets.StoredVPDataset("train", raw=obs, storage=storage)
    for step in (1, 2):
        ds.set_seq_len(3, 2, step)
        plain.set_seq_len(3, 2, step)
        for indices in ([0, 1, 2], [2, 0], [1, 1, 0, 2]):
            data = ds.batch(indices)
            assert torch.equal(data["frames"], plain.batch(indices)["frames"])                      # bitwise: the same launch over the same bytes
            got = data["actions"].cpu().numpy()
            assert np.array_equal(_bits(got), _bits(R.gather(actions, indices, 5, step)))
            assert np.array_equal(_bits(got), _bits(golden[f"actions_s{step}"][indices]))
            assert np.array_equal(data["frames"].cpu().numpy(), golden[f"frames_s{step}"][indices])
            assert data["origin"] == [ds.obs_fps[i] for i in indices]
            singles = [ds[i] for i in indices]
            assert torch.equal(data["actions"], torch.stack([s["actions"] for s in singles])) and torch.equal(data["frames"], torch.stack([s["frames"] for s in singles]))
    assert float(golden["actions_s1"][0, 0, 0]) == 1.0 and golden["actions"][0, 0, 0] != 1.0       # the tie is in what was compared


RUN = dict(context_frames=2, pred_frames=2, seq_step=2)
TINY_AC = dict(patch_size=1, num_layers=2, num_hidden=[8, 8], filter_size=5)   # 16 x 16 patches -> 4 x 4 maps after the two stride-2 convolutions


def test_quick_start_trains_and_tests_an_action_conditional_model_on_the_datasets_actions(vpx, tmp_path, monkeypatch):
    export_bair_like.export(str(tmp_path / "data"), {"train": 6, "test": 2}, seed=3)
    suite = vpx.VPSuite()
    suite.load_dataset("BAIR", data_dir=str(tmp_path / "data"), img_size=16)
    suite.create_model("predrnn-pp", action_conditional=True, **TINY_AC)
    model = suite.models[-1]
    assert model.action_conditional and model.action_size == 4 and model.img_shape == (3, 16, 16) and (model.rnn_h, model.rnn_w) == (4, 4)

    batches, received = [], []
    cls, ds_cls = type(model), vpx.datasets.BAIRPushingDataset
    forward, batch = cls.forward, ds_cls.batch

    def recording_forward(self, x, pred_frames=1, **kwargs):
        acts = kwargs.get("actions")
        received.append(None if acts is None else acts.detach().cpu().numpy().copy())
        return forward(self, x, pred_frames=pred_frames, **kwargs)

    def recording_batch(self, indices):
        batches.append((self, [int(i) for i in indices]))
        return batch(self, indices)

    monkeypatch.setattr(cls, "forward", recording_forward)
    monkeypatch.setattr(ds_cls, "batch", recording_batch)
    best = suite.train(epochs=1, batch_size=2, out_dir=str(tmp_path / "run"), **RUN)
    print(f"train(epochs=1) returned {best!r}")
    assert np.isfinite(best) and os.path.isfile(tmp_path / "run" / "best_model.pth")
    n_train = len(batches)
    assert n_train == 3                                                                             # 5 training samples in batches of 2, 1 validation sample
    suite.load_dataset("BAIR", split="test", data_dir=str(tmp_path / "data"), img_size=16)
    results = suite.test(**RUN)
    monkeypatch.undo()
    (models,) = results.values()
    assert list(models) == [model.NAME, "CopyLastFrame"]
    for name, rows in models.items():
        assert len(rows) == 2 and all(np.isfinite(v) for row in rows for v in row.values()), (name, rows)
    # every forward call received the actions of the batch drawn just before it, bit for bit
    assert len(batches) == len(received) == n_train + 2 and all(r is not None for r in received)
    for k, ((ds, indices), got) in enumerate(zip(batches, received)):
        want = R.gather(ds._actions_host, indices, 4, 2)
        if got.shape[0] == 2 * len(indices):                                                         # training: the sequence and its reversal as one batch
            want = np.concatenate([want, want])
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (k, indices)
        assert np.abs(want).max() > 0
    assert {id(ds) for ds, _ in batches[:n_train]} != {id(ds) for ds, _ in batches[n_train:]}     # the training split, then the test split

    # the prediction depends on them
    data = suite.test_sets[-1].test_data.batch([0, 1])
    model.eval()
    with torch.no_grad():
        pred, _ = model(data["frames"], pred_frames=2, actions=data["actions"])
        negated, _ = model(data["frames"], pred_frames=2, actions=-data["actions"])
    delta = float((pred - negated).abs().max())
    print(f"max |forward(actions) - forward(-actions)| = {delta:.3e}")
    assert torch.isfinite(pred).all() and delta > 0


def test_an_explicit_use_actions_and_a_dataset_without_actions_keep_their_refusals(vpx, tmp_path):
    export_bair_like.export(str(tmp_path / "data"), {"train": 3}, n_frames=8, img_size=16, seed=4)
    suite = vpx.VPSuite()
    suite.load_dataset("BAIR", data_dir=str(tmp_path / "data"))
    suite.create_model("predrnn-pp", action_conditional=True, **TINY_AC)
    with pytest.raises(ValueError, match="can't be invoked without using actions"):
        suite.train(epochs=1, batch_size=1, use_actions=False, out_dir=str(tmp_path / "run"), **RUN)
    plain = vpx.VPSuite()
    plain.load_dataset("MMF", digits=vpx.datasets.procedural_digits(n=4, size=8), n_seqs=2, img_size=16, num_channels=3)
    plain.models.append(suite.models[-1])
    with pytest.raises(ValueError, match="can't be invoked without using actions"):                # as before: nothing opens use_actions here
        plain.train(epochs=1, batch_size=1, out_dir=str(tmp_path / "run2"), **RUN)
    with pytest.raises(ValueError, match="doesn't provide actions"):
        plain.train(epochs=1, batch_size=1, use_actions=True, out_dir=str(tmp_path / "run2"), **RUN)
