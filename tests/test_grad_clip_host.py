"""Gradient clipping and the non-finite step guard of the training tail, as far as the CPU reaches: the float64 restatement
(tests/clip_ref.py) pinned against torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam, the three new symbols of the
C ABI (header, exports, ctypes table, refusals, dry runs inside the workspace the query asks for), FlatAdam's keywords and state dict on
CPU tensors, and DataParallelTrainer's CPU path."""
import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as C
from golden_util import name_seed, seeded_rand, seeded_randn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_WS = 0, -1, -2
NEW_SYMBOLS = ("vpx_grad_stats_workspace_bytes", "vpx_grad_stats", "vpx_adam_step_clipped")
NAN = float("nan")


def _fake(i, off=0):   # distinct fake device addresses (256-byte aligned + off): never dereferenced in a dry run
    return ctypes.c_void_p(0x100000000000 + i * (1 << 36) + off)


@pytest.fixture
def L(vpx):
    lib = vpx._lib.lib()
    with vpx._lib.option(vpx._lib.OPT_DRY_RUN, 1):
        yield lib


# ---- the yardstick: clip_ref against torch in float64 --------------------------------------------------------------------------------
def _torch64_step(p, g, m, v, step, lr, wd, grad_scale, max_norm, clip_value):
    """clip_grad_norm_ -> clip_grad_value_ -> torch.optim.Adam.step() on two float64 parameters that split the bucket."""
    cut = len(p) // 3
    params = [torch.from_numpy(p[:cut]).double().requires_grad_(True), torch.from_numpy(p[cut:]).double().requires_grad_(True)]
    opt = torch.optim.Adam(params, lr=lr, weight_decay=wd)
    for q, sl in zip(params, (slice(0, cut), slice(cut, None))):
        q.grad = torch.from_numpy(g[sl]).double() * grad_scale
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m[sl]).double(),
                        "exp_avg_sq": torch.from_numpy(v[sl]).double()}
    norm = None
    if max_norm > 0:
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    if clip_value > 0:
        torch.nn.utils.clip_grad_value_(params, clip_value)
    grad = torch.cat([q.grad for q in params]).numpy().copy()
    opt.step()
    cat = lambda key: torch.cat([opt.state[q][key] for q in params]).numpy()
    return torch.cat([q.detach() for q in params]).numpy(), cat("exp_avg"), cat("exp_avg_sq"), grad, norm


@pytest.mark.parametrize("n", [5, 1025])
@pytest.mark.parametrize("max_norm,clip_value", [(0.0, 0.0), (0.25, 0.0), (1e6, 0.0), (0.0, 0.125), (0.25, 2.0 ** -8)])
def test_clip_ref_agrees_with_torch_in_float64(n, max_norm, clip_value):
    seed = name_seed(f"clip.host.{n}")
    p, g = seeded_randn((n,), seed).numpy(), seeded_randn((n,), seed + 1).numpy()
    m, v = (0.1 * seeded_randn((n,), seed + 2)).numpy(), (0.1 * seeded_randn((n,), seed + 3)).pow(2).numpy()
    for step, wd, gs in ((1, 0.0, 1.0), (4, 0.01, 0.5)):
        tp, tm, tv, tgrad, tnorm = _torch64_step(p, g, m, v, step, 1e-3, wd, gs, max_norm, clip_value)
        ge, c, stats = C.clipped_gradient(g, gs, max_norm, clip_value)
        if tnorm is not None:
            assert abs(stats[0] - tnorm) <= 1e-14 * tnorm and (c < 1.0) == (max_norm < tnorm)
        assert stats[1] == gs * float(np.abs(g).max()) and stats[2] == 0
        # the clipped gradient is float64 on both sides
        assert float(np.abs(ge - tgrad).max()) <= 1e-15 * float(np.abs(tgrad).max())
        if clip_value > 0:
            share = float((np.abs(ge) == clip_value).mean())     # (some elements sit on the clamp; of 1025, not all of them)
            assert 0.0 < share and (share < 1.0 or n == 5)
        # the update runs in float32 in the restatement (adam_step_ref, as PyTorch on float32 tensors): the bounds of
        # test_flat_adam_kernel_vs_oracle_and_torch, which holds a float32 kernel against the same function
        rp, rm, rv, info = C.adam_clipped_ref(p, g, m, v, step, 1e-3, weight_decay=wd, grad_scale=gs, max_norm=max_norm, clip_value=clip_value)
        assert info["c"] == c and not info["skipped"]
        assert float(np.abs(rp - tp).max()) < 3e-7
        assert float(np.abs(rm - tm).max()) < 1e-6 * float(np.abs(tm).max()) and float(np.abs(rv - tv).max()) < 1e-6 * float(np.abs(tv).max())


def test_clip_ref_statistics_and_nonfinite_rules():
    g = np.array([3.0, -4.0, 0.0, 12.0], dtype=np.float32)
    assert C.grad_stats_ref(g, 1.0).tolist() == [13.0, 12.0, 0.0]
    assert C.grad_stats_ref(g, 0.5).tolist() == [6.5, 6.0, 0.0]
    # squares that would overflow or flush to zero in float32
    assert C.grad_stats_ref(np.array([1e-20, 1e-20], dtype=np.float32))[0] == pytest.approx(math.sqrt(2.0) * float(np.float32(1e-20)), rel=1e-15)
    assert C.grad_stats_ref(np.array([1e18, 1e-20], dtype=np.float32))[0] == pytest.approx(float(np.float32(1e18)), rel=1e-15)
    bad = np.array([1.0, NAN, -np.inf, 2.0], dtype=np.float32)
    s = C.grad_stats_ref(bad, 0.5)
    assert not np.isfinite(s[0]) and s[1] == 1.0 and s[2] == 2.0
    assert C.grad_stats_ref(np.array([NAN], dtype=np.float32)).tolist()[1:] == [0.0, 1.0]
    # torch's rules for a non-finite norm: inf -> coefficient 0, NaN -> NaN
    for val in (np.inf, NAN):
        q = [torch.ones(2).requires_grad_(True)]
        q[0].grad = torch.tensor([val, 1.0])
        torch.nn.utils.clip_grad_norm_(q, 1.0)
        ge, c, _ = C.clipped_gradient(np.array([val, 1.0], dtype=np.float32), 1.0, 1.0, 0.0)
        assert np.array_equal(np.isnan(ge), torch.isnan(q[0].grad).numpy()) and (np.isnan(c) if np.isnan(val) else c == 0.0)
        assert np.array_equal(ge[~np.isnan(ge)], q[0].grad.numpy()[~np.isnan(ge)].astype(np.float64))
    # clamp keeps NaN (torch.clamp)
    ge, _, _ = C.clipped_gradient(np.array([NAN, 3.0, -3.0], dtype=np.float32), 1.0, 0.0, 1.0)
    assert np.isnan(ge[0]) and ge[1:].tolist() == [1.0, -1.0]
    p = np.ones(3, dtype=np.float32)
    rp, rm, rv, info = C.adam_clipped_ref(p, np.array([NAN, 1.0, 1.0], dtype=np.float32), p, p, 1, 1e-3, max_norm=1.0, skip_nonfinite=True)
    assert info["skipped"] and all(np.array_equal(t, p) for t in (rp, rm, rv))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_argtypes_agree_for_the_new_symbols(vpx):
    hdr = open(os.path.join(ROOT, "include", "vpx.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(vpx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code))
    lib = vpx._lib.lib()
    ctype = {"double": ctypes.c_double, "int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
    for name in NEW_SYMBOLS:
        assert name in protos and name in vpx._lib.SIGNATURES and hasattr(lib, name)
        params = [] if protos[name].strip() == "void" else [q.strip() for q in protos[name].split(",")]
        want = [ctypes.c_void_p if "*" in q else ctype[q.rsplit(" ", 1)[0].replace("const ", "")] for q in params]
        assert getattr(lib, name).argtypes == want, name
    assert lib.vpx_grad_stats.restype == lib.vpx_adam_step_clipped.restype == ctypes.c_int
    assert lib.vpx_grad_stats_workspace_bytes.restype == ctypes.c_size_t
    # the header's table of entry points and INTEGRATION.md name them too
    assert "vpx_grad_stats " in hdr.split("#ifndef")[0] and "vpx_adam_step_clipped " in hdr.split("#ifndef")[0]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in NEW_SYMBOLS)


def _stats_call(L, grad=None, n=5, gs=1.0, stats=None, ws=None, nb=None):
    nbytes = L.vpx_grad_stats_workspace_bytes()
    return L.vpx_grad_stats(_fake(1) if grad is None else grad, n, gs, _fake(2) if stats is None else stats,
                            _fake(3) if ws is None else ws, nbytes if nb is None else nb, None)


def _adam_call(L, bufs=None, n=5, step=1, gs=1.0, stats=_fake(6), max_norm=0.0, clip_value=0.0, skip=0):
    bufs = bufs or [_fake(i) for i in (1, 2, 3, 4)]
    return L.vpx_adam_step_clipped(*bufs, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, gs, stats, max_norm, clip_value, skip, None)


def test_every_refusal_has_its_code_and_a_message(L):
    null = ctypes.c_void_p(None)
    nbytes = L.vpx_grad_stats_workspace_bytes()
    cases = [
        ("stats: grad NULL", lambda: _stats_call(L, grad=null), E_ARG),
        ("stats: stats NULL", lambda: _stats_call(L, stats=null), E_ARG),
        ("stats: n = 0", lambda: _stats_call(L, n=0), E_ARG),
        ("stats: stats not 8-byte aligned", lambda: _stats_call(L, stats=_fake(2, 4)), E_ARG),
        ("stats: grad_scale < 0", lambda: _stats_call(L, gs=-1.0), E_ARG),
        ("stats: grad_scale NaN", lambda: _stats_call(L, gs=NAN), E_ARG),
        ("stats: workspace NULL", lambda: _stats_call(L, ws=null), E_WS),
        ("stats: workspace one byte short", lambda: _stats_call(L, nb=nbytes - 1), E_WS),
        ("adam: n = 0", lambda: _adam_call(L, n=0), E_ARG),
        ("adam: step = 0", lambda: _adam_call(L, step=0), E_ARG),
        ("adam: stats not 8-byte aligned", lambda: _adam_call(L, stats=_fake(6, 4), max_norm=1.0), E_ARG),
        ("adam: max_norm < 0", lambda: _adam_call(L, max_norm=-1.0), E_ARG),
        ("adam: max_norm NaN", lambda: _adam_call(L, max_norm=NAN), E_ARG),
        ("adam: clip_value < 0", lambda: _adam_call(L, clip_value=-0.5), E_ARG),
        ("adam: clip_value NaN", lambda: _adam_call(L, clip_value=NAN), E_ARG),
        ("adam: grad_scale < 0", lambda: _adam_call(L, gs=-0.5), E_ARG),
        ("adam: grad_scale NaN", lambda: _adam_call(L, gs=NAN), E_ARG),
        ("adam: max_norm without stats", lambda: _adam_call(L, stats=null, max_norm=1.0), E_ARG),
        ("adam: skip_nonfinite without stats", lambda: _adam_call(L, stats=null, skip=1), E_ARG),
    ]
    for i in range(4):
        bufs = [_fake(k) for k in (1, 2, 3, 4)]
        bufs[i] = null
        cases.append((f"adam: bucket {i} NULL", lambda b=bufs: _adam_call(L, bufs=b), E_ARG))
        bufs = [_fake(k) for k in (1, 2, 3, 4)]
        bufs[i] = _fake(i + 1, 4)
        cases.append((f"adam: bucket {i} not 16-byte aligned", lambda b=bufs: _adam_call(L, bufs=b), E_ARG))
    for what, call, code in cases:
        # (the other entry point is refused first, so that the message found afterwards is this refusal's own)
        own, other = (b"vpx_grad_stats", b"vpx_adam_step_clipped") if what.startswith("stats") else (b"vpx_adam_step_clipped", b"vpx_grad_stats")
        assert (_adam_call(L, n=0) if what.startswith("stats") else _stats_call(L, n=0)) == E_ARG and other in L.vpx_last_error()
        rc = call()
        msg = L.vpx_last_error()
        assert rc == code, (what, rc, msg)
        assert msg.startswith(own + b":"), (what, msg)
    # value clipping alone needs no statistics
    assert _adam_call(L, stats=null, clip_value=0.5) == OK
    assert _adam_call(L, stats=null) == OK


@pytest.mark.parametrize("n", [1, 5, 2 ** 20 + 5])
def test_dry_runs_stay_inside_the_workspace(L, n):
    nbytes = L.vpx_grad_stats_workspace_bytes()
    cap = C.kernel_constant("GS_MAX_BLOCKS")
    assert nbytes >= cap * 3 * 8
    for off in (0, 0x40, 0xF8):         # (the carver rounds the base up to 256 bytes: the query's slack covers it)
        for grad_off in (0, 4):         # (an unaligned gradient takes the scalar path)
            rc = L.vpx_grad_stats(_fake(1, grad_off), n, 0.5, _fake(2), _fake(3, off), nbytes, None)
            assert rc == OK, (n, off, L.vpx_last_error())
    for kw in (dict(max_norm=1.0), dict(clip_value=0.5), dict(max_norm=1.0, clip_value=0.5, skip=1), dict()):
        assert _adam_call(L, n=n, step=3, gs=0.5, **kw) == OK, (n, kw, L.vpx_last_error())


# ---- FlatAdam on CPU tensors ---------------------------------------------------------------------------------------------------------
def test_flat_adam_keywords_are_validated_and_live_in_the_group(vpx):
    from vp_suite_amd.train import FlatAdam
    for kw in (dict(max_grad_norm=-1.0), dict(max_grad_norm=NAN), dict(clip_grad_value=-0.5), dict(clip_grad_value=NAN)):
        with pytest.raises(ValueError):
            FlatAdam.from_module(torch.nn.Linear(3, 2), **kw)
    opt = FlatAdam.from_module(torch.nn.Linear(3, 2), lr=1e-3, max_grad_norm=2.0, clip_grad_value=0.5, skip_nonfinite=True)
    g = opt.param_groups[0]
    assert (g["max_grad_norm"], g["clip_grad_value"], g["skip_nonfinite"]) == (2.0, 0.5, True)
    assert opt.grad_stats.dtype == torch.float64 and opt.grad_stats.shape == (4,) and opt.skipped_steps == 0 and opt.last_grad_norm == 0.0
    off = FlatAdam.from_module(torch.nn.Linear(3, 2))
    g = off.param_groups[0]
    assert (g["max_grad_norm"], g["clip_grad_value"], g["skip_nonfinite"]) == (None, None, False)


def test_flat_adam_state_dict_round_trip_and_old_format(vpx):
    from vp_suite_amd.train import FlatAdam
    a = FlatAdam.from_module(torch.nn.Linear(3, 2), lr=1e-3, max_grad_norm=2.0, skip_nonfinite=True)
    a.exp_avg.fill_(0.25)
    a.exp_avg_sq.fill_(0.5)
    a.steps = 7
    a.grad_stats[3] = 3.0
    sd = copy.deepcopy(a.state_dict())
    assert sd["flat_adam"]["skipped_steps"] == 3 and sd["param_groups"][0]["max_grad_norm"] == 2.0
    b = FlatAdam.from_module(torch.nn.Linear(3, 2), lr=1e-2)
    b.load_state_dict(sd)
    assert b.steps == 7 and b.skipped_steps == 3 and torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    g = b.param_groups[0]
    assert (g["lr"], g["max_grad_norm"], g["clip_grad_value"], g["skip_nonfinite"]) == (1e-3, 2.0, None, True)
    # a state dict saved before the settings existed: no such keys in the group, no skipped_steps in the entry
    old = copy.deepcopy(sd)
    for k in ("max_grad_norm", "clip_grad_value", "skip_nonfinite"):
        del old["param_groups"][0][k]
    del old["flat_adam"]["skipped_steps"]
    c = FlatAdam.from_module(torch.nn.Linear(3, 2), lr=1e-2, clip_grad_value=0.5)
    c.grad_stats[3] = 9.0
    c.load_state_dict(old)
    g = c.param_groups[0]
    assert c.steps == 7 and c.skipped_steps == 0 and torch.equal(c.exp_avg, a.exp_avg)
    assert (g["lr"], g["max_grad_norm"], g["clip_grad_value"], g["skip_nonfinite"]) == (1e-3, None, 0.5, False)


def test_flat_adam_step_picks_the_plain_kernel_when_everything_is_off(vpx, monkeypatch):
    from vp_suite_amd import ops
    from vp_suite_amd.train import FlatAdam
    calls = []
    monkeypatch.setattr(ops, "adam_step", lambda *a, **k: calls.append(("adam_step", a, k)))
    monkeypatch.setattr(ops, "adam_step_clipped", lambda *a, **k: calls.append(("adam_step_clipped", a, k)))
    monkeypatch.setattr(ops, "grad_stats", lambda g, s=1.0, out=None: (calls.append(("grad_stats", (g, s), {"out": out})), out)[1])

    def names(**kw):
        calls.clear()
        opt = FlatAdam.from_module(torch.nn.Linear(3, 2), lr=1e-3, **kw)
        opt.grad_scale = 0.5
        opt.step()
        return opt, [c[0] for c in calls]

    for kw in (dict(), dict(max_grad_norm=None, clip_grad_value=None, skip_nonfinite=False), dict(max_grad_norm=0.0, clip_grad_value=0.0)):
        opt, seen = names(**kw)
        assert seen == ["adam_step"]
        assert calls[0][1][:4] == (opt.flat_param, opt.flat_grad, opt.exp_avg, opt.exp_avg_sq) and calls[0][1][4] == 1 and calls[0][1][-1] == 0.5
    opt, seen = names(clip_grad_value=0.5)                       # value clipping alone: no reduction
    assert seen == ["adam_step_clipped"] and calls[0][2] == dict(stats=None, max_norm=0.0, clip_value=0.5, skip_nonfinite=False)
    for kw, want in ((dict(max_grad_norm=2.0), dict(max_norm=2.0, clip_value=0.0, skip_nonfinite=False)),
                     (dict(skip_nonfinite=True), dict(max_norm=0.0, clip_value=0.0, skip_nonfinite=True)),
                     (dict(max_grad_norm=2.0, clip_grad_value=0.5, skip_nonfinite=True), dict(max_norm=2.0, clip_value=0.5, skip_nonfinite=True))):
        opt, seen = names(**kw)
        assert seen == ["grad_stats", "adam_step_clipped"]
        assert calls[0][1][0] is opt.flat_grad and calls[0][1][1] == 0.5 and calls[0][2]["out"] is opt.grad_stats
        assert calls[1][2] == dict(stats=opt.grad_stats, **want) and calls[1][1][-1] == 0.5 and calls[1][1][4] == 1
    # the group is what step() reads, as for lr
    opt, _ = names()
    opt.param_groups[0]["max_grad_norm"] = 1.0
    calls.clear()
    opt.step()
    assert [c[0] for c in calls] == ["grad_stats", "adam_step_clipped"] and calls[1][1][4] == 2
    opt.param_groups[0]["max_grad_norm"] = -1.0
    with pytest.raises(ValueError):
        opt.step()


def test_ops_refuse_cpu_tensors_and_bad_values(vpx):
    from vp_suite_amd import ops
    t = torch.zeros(8)
    with pytest.raises(vpx._lib.VpxError, match="no CPU fallback"):
        ops.grad_stats(t)
    with pytest.raises(vpx._lib.VpxError, match="no CPU fallback"):
        ops.adam_step_clipped(t, t, t, t, 1, 1e-3, clip_value=0.5)


# ---- DataParallelTrainer, CPU path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(max_grad_norm="half"), dict(clip_grad_value=1e-3), dict(max_grad_norm="half", clip_grad_value=1e-3)],
                         ids=["norm", "value", "both"])
def test_dp_trainer_cpu_path_clips_the_averaged_gradient_like_torch(vpx, kw):
    from test_dp_gloo import _TinyPredictor
    from vp_suite_amd.measure import PredictionLossProvider
    from vp_suite_amd.train import DataParallelTrainer
    frames = seeded_rand((4, 5, 1, 8, 8), name_seed("clip.host.dp"))
    x, y = frames[:, :3], frames[:, 3:]
    torch.manual_seed(11)
    model = _TinyPredictor()
    twin = copy.deepcopy(model)
    lp = PredictionLossProvider({"device": "cpu", "losses_and_scales": {"mse": 1.0}})

    def torch_run(max_norm, clip_value, steps=2):
        m = copy.deepcopy(twin)
        params = [p for p in m.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-2)
        norms = []
        for _ in range(steps):
            opt.zero_grad()
            pred, reg = m(x, pred_frames=2)
            total = lp.get_losses(pred, y)[1] + reg["reg"]
            total.backward()
            with_grad = [p for p in params if p.grad is not None]
            norms.append(float(torch.nn.utils.clip_grad_norm_(with_grad, max_norm if max_norm else float("inf"))))
            if clip_value:
                torch.nn.utils.clip_grad_value_(with_grad, clip_value)
            opt.step()
        return torch.cat([p.detach().reshape(-1) for p in m.parameters()]), norms

    kw = dict(kw)
    if kw.get("max_grad_norm") == "half":   # half the smallest norm of the unclipped run: every step is clipped
        kw["max_grad_norm"] = 0.5 * min(torch_run(None, None)[1])
    want, norms = torch_run(kw.get("max_grad_norm"), kw.get("clip_grad_value"))
    if "max_grad_norm" in kw:
        assert all(nrm > kw["max_grad_norm"] for nrm in norms)
    tr = DataParallelTrainer(model, lr=1e-2, world_size=1, device="cpu", **kw)
    assert not tr.fused
    for _ in range(2):
        tr.step(x, y, pred_frames=2)
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-8), float((got - want).abs().max())
    if "clip_grad_value" in kw:   # (Adam's update barely notices a common factor; the clamp changes its direction: not vacuous)
        assert float((torch_run(None, None)[0] - want).abs().max()) > 1e-4


def test_dp_trainer_cpu_path_refuses_the_skip_guard_and_bad_values(vpx):
    from test_dp_gloo import _TinyPredictor
    from vp_suite_amd.train import DataParallelTrainer
    with pytest.raises(ValueError, match="skip_nonfinite"):
        DataParallelTrainer(_TinyPredictor(), world_size=1, device="cpu", skip_nonfinite=True)
    for kw in (dict(max_grad_norm=-1.0), dict(clip_grad_value=NAN)):
        with pytest.raises(ValueError):
            DataParallelTrainer(_TinyPredictor(), world_size=1, device="cpu", **kw)
