"""The fused data-parallel path (train.DataParallelTrainer on the GPU: flat parameter + gradient buckets, 1/W folded into
the Adam kernel) executed with world_size = 2 ARITHMETIC on one device: two replicas, one batch shard each, the
"all-reduce" a hand-written sum of the two shard gradients. The result must equal the single-process update on the
global batch (harness semantics base_model.py:162-179). RCCL itself refuses two ranks on one GPU, so
the collective is the only piece this test replaces; `bench.py --gpus N` runs it for real."""
import numpy as np
import pytest
import torch

import golden_cases as gc
from golden_util import name_seed, seeded_rand
from test_gpu_models import _ef

pytestmark = pytest.mark.gpu


class _FakeWorld:
    """Sum-all-reduce over the replicas living in this process: every replica deposits its buckets in launch order, the k-th
    reduction happens when every replica's k-th bucket has arrived, then all of them hold the sum (what ncclAllReduce(SUM)
    leaves). One callable per rank (`for_rank`), as every rank has its own communicator."""

    def __init__(self, n):
        self.n, self.queues, self.done = n, [[] for _ in range(n)], 0

    def for_rank(self, r):
        def all_reduce(t):
            self.queues[r].append(t)
            while all(len(q) > self.done for q in self.queues):
                parts = [q[self.done] for q in self.queues]
                assert len({p.numel() for p in parts}) == 1   # the ranks cut and launch their buckets alike
                total = torch.stack(parts).sum(dim=0)
                for p in parts:
                    p.copy_(total)
                self.done += 1
        return all_reduce

    def reset(self):
        assert all(len(q) == self.done for q in self.queues)
        self.queues, self.done = [[] for _ in range(self.n)], 0

    def broadcast(self, t, src):
        pass  # replicas are built from identical seeds


def _flat(m):
    named = dict(m.named_parameters())
    return torch.cat([named[k].detach().reshape(-1) for k in sorted(named)]).cpu().numpy()


@pytest.mark.parametrize("precision,bucketed", [("f32", True), ("bf16x3", True), ("bf16x3", False)])
def test_fused_dp_world2_equals_global_batch_update(vpx, precision, bucketed):
    from vp_suite_amd.train import DataParallelTrainer
    kw = dict(gc.EF_TINY_KW, cell_precision=precision)
    B, T, P = 4, 3, 2
    c, h, w = kw["img_shape"]
    frames = seeded_rand((B, T + P, c, h, w), name_seed("dp.frames")).cuda()

    ref = _ef(vpx, "tiny", kw)
    tr_ref = DataParallelTrainer(ref, lr=1e-3, world_size=1)
    world = _FakeWorld(2)
    reps = [_ef(vpx, "tiny", kw) for _ in range(2)]
    trs = [DataParallelTrainer(m, lr=1e-3, world_size=2, all_reduce=world.for_rank(r), broadcast=world.broadcast, bucketed=bucketed)
           for r, m in enumerate(reps)]
    assert all(t.fused and t.collectives for t in trs)
    # per-block buckets: the 6 recurrent blocks and the 6 stages of convlstm-shi, contiguous and complete
    assert [b[3] for b in trs[0].buckets] == [f"{half}.{kind}{i}" for half, order in (("encoder", (1, 2, 3)), ("forecaster", (3, 2, 1)))
                                               for i in order for kind in (("stage", "rnn") if half == "encoder" else ("rnn", "stage"))]
    assert sum(b[1] for b in trs[0].buckets) == trs[0].flat_grad.numel()
    for step in range(3):
        tr_ref.step(frames[:, :T], frames[:, T:], P)
        # ranks run concurrently in reality; here: both backward passes (bucketed: each block's bucket is deposited from inside
        # the backward pass, the sums complete during rank 1's), then the rest of the exchange, then both updates
        for r, t in enumerate(trs):
            t.backward_shard(frames[2 * r:2 * r + 2, :T], frames[2 * r:2 * r + 2, T:], P)
        if not bucketed:
            shard_sum = trs[0].flat_grad + trs[1].flat_grad
        for t in trs:
            t.reduce_gradients()
        world.reset()
        if not bucketed:
            assert torch.equal(trs[0].flat_grad, shard_sum)
        assert torch.equal(trs[0].flat_grad, trs[1].flat_grad)
        assert trs[0].optimizer.grad_scale == 0.5
        # mean over the global batch = (sum of shard means) / 2: the summed bucket is 2x the global-batch gradient
        g_ref = tr_ref.flat_grad
        err = float((trs[0].flat_grad * 0.5 - g_ref).abs().max() / g_ref.abs().max())
        assert err < (2e-5 if precision == "f32" else 1e-4), (step, err)
        for t in trs:
            t.optimizer.step()
    want = _flat(ref)
    for m in reps:
        # Adam's first steps move every weight by ~lr regardless of gradient scale; compare absolutely (lr = 1e-3)
        assert np.abs(_flat(m) - want).max() < 2e-5
    assert np.array_equal(_flat(reps[0]), _flat(reps[1]))


@pytest.mark.timeout(600)
def test_bench_launcher_path_runs_rccl_world1():
    """`bench.py --gpus 1` under a launcher (RANK set): one rank per GPU through RCCL, spawned as a CHILD `torch.distributed.run`
    before anything in the parent touches the GPU. Asserts the line's backend / n_gpus and that gradients went through RCCL
    (train mode, bucketed all-reduce on a world of one)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(bench.free_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", "8", "--mode", "train", "--full", "--no-extras", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.splitlines()[-1]
    # the driver parses the LAST stdout line out of a bounded capture: it must be the JSON line, and short (BENCH_r03: parsed null)
    assert last.startswith("{") and len(last) < bench.LINE_BUDGET and len(out.stdout) < 2 * bench.LINE_BUDGET, len(out.stdout)
    line = json.loads(last)
    assert line["n_gpus"] == 1 and line["config"]["backend"] == "nccl (RCCL)" and line["config"]["mode"] == "train"
    assert "traffic_source" in line["roofline"]
    assert line["value"] > 0 and line["steps"] == 2
    # the measurement contract's extra objects: roofline of the dominant kernel (live HIP-event timing) and the prewarm record
    assert line["roofline"]["bound"] == "mfma" and 0.0 < line["roofline"]["frac"] < 1.0 and line["roofline"]["achieved"] > 0
    assert line["config"]["prewarm"]["steps"] >= 2 and line["config"]["workload"].startswith("convlstm-shi")


def test_trainer_runs_predrnn_training_semantics(vpx):
    """DataParallelTrainer.step on PredRNN-V2 = the model's own train_iter (predrnn_v2.py:319-365): training-time mask,
    forward + reversed forward averaged, training_iteration bumped — same parameters as train_iter with FlatAdam."""
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.models import MODEL_CLASSES
    from vp_suite_amd.train import DataParallelTrainer, FlatAdam
    from golden_util import fill_state_dict_
    kw = dict(gc.PRED_TINY_KW, scheduled_sampling=False)
    B, T, P = 2, 3, 2
    c, h, w = kw["img_shape"]
    frames = seeded_rand((B, T + P, c, h, w), name_seed("dp.predrnn.frames")).cuda()

    def build():
        m = MODEL_CLASSES["predrnn-pp"]("cuda", **kw)
        fill_state_dict_(m, name_seed("dp.predrnn"))
        return m.to("cuda")
    a, b = build(), build()
    tr = DataParallelTrainer(a, lr=1e-3, world_size=1)
    opt = FlatAdam.from_module(b, lr=1e-3)
    lp = PredictionLossProvider({"device": "cuda", "losses_and_scales": {"mse": 1.0}})
    cfg = {"device": "cuda", "context_frames": T, "pred_frames": P, "val_rec_criterion": "mse"}
    data = {"frames": frames, "actions": torch.zeros(B, T + P - 1, 0)}
    torch.use_deterministic_algorithms(True)  # no K-split atomics: both runs sum in the same order
    try:
        for _ in range(2):
            tr.step(frames, frames[:, T:], P)
            b.train_iter(cfg, [data], opt, lp, epoch=0)
    finally:
        torch.use_deterministic_algorithms(False)
    assert a.training_iteration == b.training_iteration == 3
    # a semantic difference (no reversed pass, test-time mask) moves every weight by ~lr = 1e-3 per step
    assert np.abs(_flat(a) - _flat(b)).max() < 2e-5


def test_flat_adam_survives_set_to_none_and_keeps_state(vpx):
    """p.grad = None (torch's zero_grad default) must not make FlatAdam step on a stale bucket; state_dict
    carries the moments."""
    from vp_suite_amd.train import FlatAdam
    m = _ef(vpx, "tiny", gc.EF_TINY_KW)
    twin = _ef(vpx, "tiny", gc.EF_TINY_KW)
    opt, opt2 = FlatAdam.from_module(m, lr=1e-3), torch.optim.Adam(twin.parameters(), lr=1e-3)
    frames = seeded_rand((2, 5, 1, 16, 16), name_seed("ef.tiny.frames")).cuda()
    for _ in range(2):
        for model, o in ((m, opt), (twin, opt2)):
            for p in model.parameters():
                p.grad = None  # what nn.Module.zero_grad(set_to_none=True) does
            pred, _ = model(frames[:, :3], pred_frames=2)
            ((pred - frames[:, 3:]) ** 2).sum().backward()
            o.step()
    assert np.abs(_flat(m) - _flat(twin)).max() < 2e-6
    base = opt.flat_grad.untyped_storage().data_ptr()
    assert all(p.grad.untyped_storage().data_ptr() == base for p in m.parameters())
    sd = opt.state_dict()
    assert sd["flat_adam"]["steps"] == 2 and float(sd["flat_adam"]["exp_avg_sq"].abs().sum()) > 0
    fresh = FlatAdam.from_module(_ef(vpx, "tiny", gc.EF_TINY_KW), lr=1e-3)
    fresh.load_state_dict(sd)
    assert fresh.steps == 2 and torch.equal(fresh.exp_avg, opt.exp_avg)
    with pytest.raises(ValueError):
        FlatAdam([{"params": list(m.parameters())}], opt.flat_param, opt.flat_grad)


@pytest.mark.timeout(600)
def test_predrnn_deferred_weight_gradients_drive_the_bucket_hooks_under_rccl_world1():
    """a full predrnn-pp training step with DEFERRED weight gradients (ops.STWeightBank: a cell's five weight
    gradients reach autograd once per pass, from the bank's identity node, after every step's backward) under the bucketed
    post-accumulate hooks and real RCCL collectives (world 1, own process). The hooks of a cell's bucket then fire late and together —
    the launch order must still be strictly descending, every bucket must go out exactly once per step, and the reduced gradient must
    equal the gradient of the same step without collectives."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    script = r'''
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import torch, torch.distributed as dist
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
import vp_suite_amd
from vp_suite_amd.models import MODEL_CLASSES
from vp_suite_amd.train import DataParallelTrainer
from golden_util import fill_state_dict_, name_seed, seeded_rand
kw = dict(img_shape=(1, 32, 32), action_size=0, tensor_value_range=[0.0, 1.0], num_layers=2, num_hidden=[32, 32], cell_precision="bf16x3")
def build():   # (32 hidden channels: the split-operand ST-LSTM kernels — and with them the banks — want channels in 32s)
    m = MODEL_CLASSES["predrnn-pp"]("cuda", **kw)
    fill_state_dict_(m, name_seed("dp.predrnn.banks"))
    m = m.to("cuda"); m.sampling_eta = 0.5
    return m
frames = seeded_rand((4, 7, 1, 32, 32), name_seed("dp.predrnn.banks.frames")).cuda()
a, b = build(), build()
tr = DataParallelTrainer(a, lr=1e-3, world_size=1, force_collectives=True)      # RCCL at world 1, bucketed hooks
ref = DataParallelTrainer(b, lr=1e-3, world_size=1)                               # no collectives
assert tr.collectives and tr.bucketed and not ref.collectives
banks = a._weight_banks(8, 6) is not None
launched, fired = [], []
orig_launch, orig_ready = tr._launch_bucket, tr._grad_ready
def launch(i): launched[-1].append(i); return orig_launch(i)
def ready(p): fired[-1].append(tr._bucket_of[id(p)]); return orig_ready(p)
tr._launch_bucket = launch
for h in tr._hooks: h.remove()
tr._hooks = [p.register_post_accumulate_grad_hook(ready) for p in tr.params]
diffs = []
for step in range(2):
    launched.append([]); fired.append([])
    torch.manual_seed(100 + step); tr.backward_shard(frames, frames[:, 4:], 3); tr.reduce_gradients()
    torch.manual_seed(100 + step); ref.backward_shard(frames, frames[:, 4:], 3); ref.reduce_gradients()
    torch.cuda.synchronize()
    diffs.append(float((tr.flat_grad - ref.flat_grad).abs().max() / ref.flat_grad.abs().max()))
    tr.optimizer.step(); ref.optimizer.step()
print("RESULT " + json.dumps({"banks": banks, "names": [x[3] for x in tr.buckets], "launched": launched, "fired": fired, "diffs": diffs}))
dist.destroy_process_group()
''' % (root, root)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench.free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=500, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["banks"], "the deferred-weight-gradient banks were not built for this model"
    nb = len(res["names"])
    assert any(n.startswith("cell_list.") for n in res["names"])
    for step in range(2):
        assert res["launched"][step] == list(range(nb - 1, -1, -1)), res["launched"][step]   # every bucket once, strictly descending
        assert sorted(set(res["fired"][step])) == list(range(nb))                            # every bucket's hooks fired (banks included)
        # all-reduce over one rank = identity; the two replicas still differ in fp32 summation order (K-split atomics) and, from
        # step 1 on, in the parameters those gradients updated
        assert res["diffs"][step] < 2e-5, res["diffs"]
