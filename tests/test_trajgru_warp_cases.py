"""Validity of the prescribed-flow TrajGRU cases (tests/trajgru_warp_ref.py), in the fp64 reference alone and without a GPU: a case is
compared to a tight bar on the GPU (tests/test_gpu_trajgru_warp.py) only if none of its sampling coordinates and none of its LeakyReLU
pre-activations sits within rounding of a kink. No element is ever excluded from a comparison there."""
import pytest
import torch

import trajgru_warp_ref as wr


@pytest.mark.parametrize("tag", list(wr.CASES))
def test_trajgru_warp_case_is_clear_of_kinks(tag):
    case, ref = wr.CASES[tag], wr.reference(tag)
    print(f"{tag}: min coordinate distance {ref.coord_dist:.3e}, min |pre-activation| {ref.preact_dist:.3e}")
    assert ref.coord_dist >= wr.COORD_MARGIN, (tag, ref.coord_dist)
    assert ref.preact_dist >= wr.PREACT_MARGIN, (tag, ref.preact_dist)
    # the table's own claims: which fields sample nothing but padding, and what the reference makes of them
    assert [l for l, r in enumerate(ref.reach) if not r] == list(case.out), (tag, ref.reach)
    db = ref.grads["flows_conv.bias"]
    for l in range(len(case.fields)):
        if l in case.out:
            assert torch.equal(db[2 * l:2 * l + 2], torch.zeros(2, dtype=db.dtype)), (tag, l)
        else:
            assert float(db[2 * l:2 * l + 2].abs().min()) > 0.0, (tag, l)
    assert float(ref.grads["flows_conv.weight"].abs().max()) > 0.0


@pytest.mark.parametrize("tag", list(wr.CASES))
def test_trajgru_warp_reference_side_error(tag):
    """The fp32 oracle against its own fp64 run, per tensor: the figure that would widen a bound (3 x, where it exceeds a third of it).
    Measured over the whole table: at most 6.3e-7 on any tensor (h2f_conv1.weight of 6x7.near.T1.jitter), ten times below a third of the
    tightest bound — no tensor's bound moves."""
    b = wr.bars(tag)
    worst = max(b.items(), key=lambda kv: kv[1][1])
    print(f"{tag}: worst reference-side error {worst[1][1]:.2e} ({worst[0]})")
    for name, (bound, err) in b.items():
        assert bound == (wr.FWD_F32 if name in ("out", "hT") else wr.GRAD_F32), (tag, name, err)
