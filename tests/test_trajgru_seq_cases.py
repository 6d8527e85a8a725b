"""Validity of the TrajGRU sequence cases (tests/trajgru_seq_ref.py), on the CPU and without the package: a case is compared to its bars
on the GPU (tests/test_gpu_trajgru_routes.py) only if, in the float64 reference, no sampling coordinate and no LeakyReLU pre-activation
sits within reach of the arithmetic's noise, its flows are real displacements, and no bar derived for it exceeds its ceiling. The table's
coverage is asserted list by list. No element is ever excluded from a comparison there."""
import pytest
import torch

import trajgru_seq_ref as R

TAGS = list(R.CASES)
GRAD_TAGS = [t for t in TAGS if R.CASES[t].grads != "none"]


@pytest.mark.parametrize("tag", TAGS)
def test_trajgru_seq_case_is_clear_of_kinks(tag):
    """Both margins, in the float64 reference alone; integers include the padding borders -1 and W - 1 / H - 1."""
    ref = R.reference(tag)
    print(f"{tag}: min coordinate distance {ref.coord_dist:.3e} px, min |pre-activation| {ref.preact_dist:.3e}")
    assert ref.coord_dist >= R.COORD_MARGIN, (tag, ref.coord_dist)
    assert ref.preact_dist >= R.PREACT_MARGIN, (tag, ref.preact_dist)


@pytest.mark.parametrize("tag", TAGS)
def test_trajgru_seq_case_flows_are_real_displacements(tag):
    case, ref = R.CASES[tag], R.reference(tag)
    print(f"{tag}: max|flow| {ref.max_flow:.2f} px")
    if case.H > 1 and case.W > 1:
        assert R.FLOW_RANGE[0] <= ref.max_flow <= R.FLOW_RANGE[1], (tag, ref.max_flow)
    assert ref.coords.shape == (case.T * case.L, 2, case.B, case.H, case.W)
    assert ref.preacts.numel() == case.T * case.B * case.H * case.W * (R.FLOW_FEATURES + case.C)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("tag", TAGS)
def test_trajgru_seq_restatement_stays_a_tenth_inside_the_margins(tag, mode):
    """The restatement's coordinates and pre-activations deviate from float64 by at most a tenth of the distance the case keeps from its
    nearest kink (which is at least the margin): what ties the margins to the arithmetic's real noise."""
    ref, (dc, dp) = R.reference(tag), R.deviation(tag, mode)
    print(f"{tag} {mode}: coordinates deviate by {dc:.2e} px (nearest integer {ref.coord_dist:.2e}), pre-activations by {dp:.2e} (nearest {ref.preact_dist:.2e})")
    assert dc <= R.DEVIATION * ref.coord_dist, (tag, mode, dc, ref.coord_dist)
    assert dp <= R.DEVIATION * ref.preact_dist, (tag, mode, dp, ref.preact_dist)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("tag", TAGS)
def test_trajgru_seq_bars_are_under_their_ceiling(tag, mode):
    """Every derived bar is at most CEILING x its base; measured, none is raised at all (the module docstring's figures are ceilings here:
    f32 1.0e-6 / 2.3e-6, bf16x3 1.6e-5 / 4.2e-5 on outputs / gradients)."""
    case, b = R.CASES[tag], R.bars(tag, mode)
    assert set(b) == {"out", "hT"} | {"grad." + n for n in R.leaves(case)}, (tag, sorted(b))
    worst = max(b.items(), key=lambda kv: kv[1][1] / R.base_bar(kv[0], mode))
    print(f"{tag} {mode}: worst restatement error {worst[1][1]:.2e} ({worst[0]})")
    measured = {"f32": (1.05e-6, 2.3e-6), "bf16x3": (1.6e-5, 4.2e-5)}[mode]
    for name, (bound, err) in b.items():
        assert bound <= R.CEILING * R.base_bar(name, mode), (tag, mode, name, err)
        assert bound == R.base_bar(name, mode), (tag, mode, name, err, "a raised bar: state it in the module docstring")
        assert err <= measured[name.startswith("grad.")], (tag, mode, name, err, "above the module docstring's measured worst")


def test_trajgru_seq_seed_revisions():
    """The revision in use follows the rejected ones, and passes every condition at once."""
    for tag, case in R.CASES.items():
        assert case.rev == len(R.REJECTED.get(tag, ())) and sorted(R.REJECTED.get(tag, ())) == list(range(case.rev)), tag
        assert not R.violations(tag), (tag, R.violations(tag))
    assert set(R.REJECTED) <= set(R.CASES)


def test_trajgru_seq_table_covers_every_list():
    C = [R.CASES[t] for t in GRAD_TAGS]   # each value at a case where a gradient is taken
    assert 20 <= len(R.CASES) <= 30
    assert {c.k for c in C} == R.REQUIRED["k"] == {1, 3, 5, 7}
    assert {c.T for c in C} == R.REQUIRED["T"] == {1, 2, 3, 4}
    assert {c.L for c in C} == R.REQUIRED["L"] == {1, 3, 5, 13}
    assert {c.C for c in C} == R.REQUIRED["C"] == {4, 8, 12, 32}
    assert {c.Cin for c in C} == R.REQUIRED["Cin"] == {1, 3, 4, 8}
    assert {c.B for c in C} == R.REQUIRED["B"] == {1, 2, 3}
    assert {(c.H, c.W) for c in C} == R.REQUIRED["map"] == {(1, 1), (1, 7), (6, 1), (5, 7), (8, 8), (9, 6)}
    assert {c.ops for c in C} == R.REQUIRED["ops"] == {"x+h0", "x", "h0"}
    assert {c.loss for c in C} == R.REQUIRED["loss"] == {"out", "hT", "out_hT"}
    assert {c.grads for c in R.CASES.values()} == {"all", "params", "inputs", "none"}
    assert {c.ops for c in R.CASES.values() if c.grads == "none"} == {"x+h0", "x", "h0"}          # the inference route in all three forms
    det = [c for c in R.CASES.values() if c.det]
    assert len(det) >= 4 and any(c.ops == "h0" and c.grads != "none" for c in det) and any(c.T >= 3 and c.grads != "none" for c in det)
    assert any(c.det and c.grads == "none" for c in det)                                           # inference bits against the training call's
    assert any(c.L == 13 and c.C == 4 and (c.H, c.W) == (5, 7) for c in C) and any(c.C == 32 and (c.H, c.W) == (8, 8) for c in C)
    assert max(c.H * c.W for c in R.CASES.values()) <= 64                                          # nothing near the default model's 64x64
    # both "a loss that leaves a cotangent out" kinds exist with gradients: they run once more through the raw C ABI
    assert {c.loss for c in C if c.loss != "out_hT"} == {"out", "hT"}
    km = R.CASES[R.MODULE_CASE]
    assert km.k == 5 and km.grads == "all" and km.ops == "x+h0"


def test_trajgru_seq_exact_zero_gradient_is_in_the_table():
    """One step without h0: the warps sample a zero state, so nothing flows back into the flow generator — the gradients of h2f_conv1,
    i2f_conv1 and flows_conv are exactly zero in the reference (the GPU test asks for the same bits); those of i2h and ret.bias are not."""
    hit = [t for t in GRAD_TAGS if R.CASES[t].T == 1 and R.CASES[t].ops == "x" and R.CASES[t].grads == "all"]
    assert hit
    for tag in hit:
        g = R.reference(tag).tensors
        for n in ("h2f_conv1", "i2f_conv1", "flows_conv"):
            assert not g[f"grad.{n}.weight"].any() and not g[f"grad.{n}.bias"].any(), (tag, n)
        assert g["grad.i2h.weight"].any() and g["grad.ret.bias"].any() and g["grad.x"].any(), tag


def test_trajgru_seq_reference_equals_the_unchanged_oracle_call():
    """k = 3: reference() (i2h_pad = k // 2 = 1) against the oracle called as every earlier caller calls it, bit for bit."""
    from oracle import torch_ref as tr
    tag = "k3"
    case = R.CASES[tag]
    assert case.k == 3 and case.ops == "x+h0" and case.grads == "all" and case.loss == "out_hT"
    t = {n: v.double() for n, v in R.inputs(tag).items()}
    lv = {n: t[n].clone().requires_grad_(True) for n in R.PARAM_KEYS + ("x", "h0")}
    out, hT = tr.trajgru_seq(lv["x"], lv["h0"], case.T, {k: lv[k] for k in R.PARAM_KEYS}, case.L, R.SLOPE)
    ((out * t["g.out"]).sum() + (hT * t["g.hT"]).sum()).backward()
    ref = R.reference(tag).tensors
    assert torch.equal(out.detach(), ref["out"]) and torch.equal(hT.detach(), ref["hT"])
    for n in R.leaves(case):
        assert torch.equal(lv[n].grad, ref["grad." + n]), n
