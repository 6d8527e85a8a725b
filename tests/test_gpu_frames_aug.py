"""csrc/frames_aug.hip on the GPU: photometric augmentations and erasing in place, against the numpy restatement
(tests/frames_aug_ref.py) run in the test.

EXACT cases (torch.equal; the parity record shows bound 0): invert, solarize, brightness, saturation, grayscale, normalize,
autocontrast and erasing are float32 operations rounded one at a time (min and max are exact by nature), singly and chained.
BOUNDED cases: contrast (the mean is a float64 sum in the kernel's own order) against the float64 twin with the bound counted in
frames_aug_ref.py from the expression; hue against the float64 twin with four times the deviation measured on the CPU between the
float32 and the float64 restatement over the same inputs (frames_aug_ref.HUE_F32_VS_F64). No element is excluded.

Inputs are random bytes through the preprocess launch under the value ranges (0, 1) and (-1, 1) (so that the clamps bite), B = 3 samples
with a different program each, one of them empty, F = 2 frames of differing content. Frame sizes: 1x1 and 1x5 (fewer pixels than lanes),
3x7, 17x19 (323 pixels: some threads own two, the tail is ragged; element accesses), 33x40 (1320 pixels: 16-byte accesses, 330 groups
over 256 threads)."""
import os

import numpy as np
import pytest
import torch

import frames_aug_ref as A
import frames_ref as R

pytestmark = pytest.mark.gpu

SIZES, RANGES = A.SIZES, A.RANGES
THR = float(np.float32(128.0) / np.float32(255.0))          # a byte value: the pixels that hold 128 sit exactly on the threshold


def _frames(vpx, raw, vr):
    """(GPU batch [B, F, C, h, w] from the preprocess launch, the same values from the restatement)."""
    B, F = raw.shape[:2]
    x = vpx.ops.frames_preprocess(torch.from_numpy(raw).cuda(), R.table(list(range(B))), F, value_range=vr)
    ref = A.scaled(raw, vr)
    assert torch.equal(x.cpu(), torch.from_numpy(ref))
    return x, ref


def _exact(parity_log, name, got, ref):
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert got.is_cuda and got.dtype == ref.dtype and got.is_contiguous() and tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    parity_log(name, got.float(), ref.float(), 0.0)
    assert torch.equal(got.cpu(), ref), f"{name}: {int((got.cpu() != ref).sum())} of {ref.numel()} values differ"


def _bounded(parity_log, name, got, ref, bound):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape and ref.dtype == np.float64
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"{name}: max |kernel - twin| = {err:.3e} (bound {bound:.3e})")
    parity_log(name, got.double(), torch.from_numpy(ref), bound / max(float(np.abs(ref).max()), 1e-30))
    assert err <= bound, (name, err, bound)


def _augment(vpx, x, programs):
    out = vpx.ops.frames_augment(x, A.pack(programs))
    assert out.data_ptr() == x.data_ptr()
    return out


def _means(C):
    return ([0.5, 0.4, 0.3, 0.2][:C] + [0.0] * (4 - C)), ([0.25, 0.5, 2.0, 0.75][:C] + [1.0] * (4 - C))


def _pointwise_programs(C):
    mean, std = _means(C)
    a = [A.row(A.INVERT), A.row(A.SOLARIZE, THR), A.row(A.NORMALIZE, *mean, *std)]
    c = [A.row(A.SOLARIZE, THR), A.blend_row(A.BRIGHTNESS, 1.3), A.row(A.INVERT), A.row(A.NORMALIZE, *([0.5] * C + [0.0] * (4 - C)), *([0.25] * C + [1.0] * (4 - C))),
         A.blend_row(A.BRIGHTNESS, 0.7)]
    if C in (1, 3):
        c = [A.blend_row(A.SATURATION, 1.4)] + c + [A.blend_row(A.SATURATION, 0.3)] + ([A.row(A.GRAY)] if C == 3 else [])
    c = (c + [A.row(A.INVERT), A.blend_row(A.BRIGHTNESS, 1.1), A.row(A.SOLARIZE, 0.25)] * 4)[:16]        # a chain 16 long
    assert len(c) == 16
    return [a, [], c]


@pytest.mark.parametrize("tag", list(RANGES))
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", SIZES)
def test_pointwise_operations_are_exact(vpx, parity_log, hw, C, tag):
    raw = A.raw_bytes(hw, C, seed=hw[1] * 10 + C)
    raw.reshape(-1)[1 % raw.size] = 128                                        # a pixel exactly on the solarize threshold
    x, ref = _frames(vpx, raw, RANGES[tag])
    singles = [[A.row(A.INVERT)], [A.row(A.SOLARIZE, THR)], [A.blend_row(A.BRIGHTNESS, 0.6)]]
    _exact(parity_log, f"singles_{hw}_{C}_{tag}", _augment(vpx, x.clone(), singles), A.apply_batch(ref, singles))
    if C == 3:
        singles = [[A.blend_row(A.SATURATION, 0.5)], [A.row(A.GRAY)], [A.row(A.NORMALIZE, 0.5, 0.5, 0.5, 0, 0.5, 0.5, 0.5, 1)]]
        _exact(parity_log, f"singles3_{hw}_{tag}", _augment(vpx, x.clone(), singles), A.apply_batch(ref, singles))
    programs = _pointwise_programs(C)
    got = _augment(vpx, x, programs)
    _exact(parity_log, f"pointwise_{hw}_{C}_{tag}", got, A.apply_batch(ref, programs))
    assert torch.equal(got[1].cpu(), torch.from_numpy(ref[1]))                 # the empty program left its sample alone


@pytest.mark.parametrize("tag", list(RANGES))
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", SIZES)
def test_autocontrast_is_exact(vpx, parity_log, hw, C, tag):
    raw = A.raw_bytes(hw, C, seed=hw[0] * 7 + C)
    raw[0, 0, :, :, 0] = 77                                                     # a constant channel: unchanged
    raw[0, 1] = np.maximum(raw[0, 1], 3)
    raw[0, 1, -1, -1, C - 1] = 1                                                # the minimum sits in the last, ragged pixel
    raw[2, 1] = np.minimum(raw[2, 1], 250)
    raw[2, 1, -1, -1, 0] = 254                                                  # ... and a maximum
    x, ref = _frames(vpx, raw, RANGES[tag])
    mean, std = _means(C)
    programs = [[A.row(A.AUTOCONTRAST)], [],
                [A.row(A.INVERT), A.row(A.AUTOCONTRAST), A.blend_row(A.BRIGHTNESS, 0.8), A.row(A.SOLARIZE, 0.5), A.row(A.AUTOCONTRAST), A.row(A.NORMALIZE, *mean, *std)]]
    want = A.apply_batch(ref, programs)
    assert np.array_equal(want[0, 0, 0], ref[0, 0, 0])
    if hw != (1, 1):
        assert not np.array_equal(want[0, 0], want[0, 1]) and want[0, 1, C - 1, -1, -1] == 0.0 and want[0, 1].max() == 1.0
    _exact(parity_log, f"autocontrast_{hw}_{C}_{tag}", _augment(vpx, x, programs), want)


def _boxes(h, w):
    return [(0, 0, max(h // 2, 1), max(w // 3, 1)), (0, w - max(w // 2, 1), 1, max(w // 2, 1)), (h - 1, 0, 1, 1), (h - max(h // 3, 1), w - 1, max(h // 3, 1), 1),
            (0, w // 2, h - 1, 1), (h // 2, w // 2, 1, 1)]            # the four corners, full height less one, 1 x 1


@pytest.mark.parametrize("tag", list(RANGES))
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", SIZES)
def test_erasing_is_exact(vpx, parity_log, hw, C, tag):
    h, w = hw
    x, ref = _frames(vpx, A.raw_bytes(hw, C, seed=hw[0] + hw[1] + C), RANGES[tag])
    value = [0.25, -0.5, 2.0, 0.125][:C] + [0.0] * (4 - C)
    boxes = _boxes(h, w)
    programs = [[A.row(A.ERASE, *box, *([0.5] * C + [0.0] * (4 - C))) for box in boxes[:3]], [],
                [A.row(A.AUTOCONTRAST), A.row(A.ERASE, *boxes[3], *value), A.row(A.INVERT), A.row(A.ERASE, *boxes[4], *value), A.row(A.ERASE, *boxes[5], *value)]]
    want = A.apply_batch(ref, programs)
    got = _augment(vpx, x, programs)
    _exact(parity_log, f"erase_{hw}_{C}_{tag}", got, want)
    y0, x0, eh, ew = boxes[4]
    if eh > 0:                                                                  # the same rectangle in both frames, a per-frame statistic around it
        assert bool((got[2, :, 0, y0:y0 + eh, x0:x0 + ew] == value[0]).all())


def test_bad_rows_read_and_write_nothing_out_of_bounds(vpx, parity_log):
    """A device table the host never saw: an unknown opcode ends the program, a rectangle is clipped, grayscale on two channels ends the
    program; the bands around the batch keep their values. The batch starts 4 bytes past a 16-byte boundary: element accesses."""
    h, w, C = 6, 8, 2
    raw = A.raw_bytes((h, w), C, seed=3)
    n = 3 * 2 * C * h * w
    flat = torch.full((n + 64,), -7.0, device="cuda")
    x = flat[33:33 + n].view(3, 2, C, h, w)
    assert x.data_ptr() % 16 == 4
    ref = A.scaled(raw, (0.0, 1.0))
    x.copy_(torch.from_numpy(ref))
    huge = [A.row(A.INVERT), A.row(A.ERASE, h - 2, w - 3, 30000, 40000, 0.5, 0.25, 0, 0), A.row(A.ERASE, 1e9, 0, 5, 5, 9, 9, 0, 0), A.row(A.ERASE, -4, -4, 6, 6, 3, 3, 0, 0)]
    programs = [huge + [(99.0,) + (1.0,) * 8, A.row(A.INVERT)], [A.row(A.INVERT), A.row(A.GRAY), A.row(A.INVERT)], [(float("nan"),) + (0.0,) * 8, A.row(A.INVERT)]]
    table = torch.from_numpy(A.pack(programs)).cuda()
    out = vpx.ops.frames_augment(x, table)
    # the restatement of the refusals: program 0 runs up to the unknown row, a negative corner counts as 0 with its own size
    want = A.apply_batch(ref, [huge[:3] + [A.row(A.ERASE, 0, 0, 6, 6, 3, 3, 0, 0)], [A.row(A.INVERT)], []])
    _exact(parity_log, "bad_rows", out.contiguous(), want)
    assert bool((flat[:33] == -7.0).all()) and bool((flat[33 + n:] == -7.0).all())
    with pytest.raises(ValueError, match="opcode"):
        vpx.ops.frames_augment(x, A.pack(programs))                             # the same table from the host is refused before any launch
    with pytest.raises(vpx._lib.VpxError, match="GPU tensor"):
        vpx.ops.frames_augment(x.cpu(), A.pack([[]] * 3))
    with pytest.raises(ValueError, match="contiguous"):
        vpx.ops.frames_augment(x.transpose(3, 4), A.pack([[]] * 3))
    with pytest.raises(ValueError, match="max_ops"):
        vpx.ops.frames_augment(x, torch.zeros((3, 8, 9), device="cuda"))


@pytest.mark.parametrize("tag", list(RANGES))
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw", SIZES)
def test_contrast_within_its_counted_bound(vpx, parity_log, hw, C, tag):
    x, ref = _frames(vpx, A.raw_bytes(hw, C, seed=hw[0] * 3 + hw[1] + C), RANGES[tag])
    mean, std = _means(C)
    programs = [[A.blend_row(A.CONTRAST, 1.3)], [],
                [A.row(A.SOLARIZE, THR), A.blend_row(A.CONTRAST, 0.6), A.blend_row(A.BRIGHTNESS, 1.2), A.row(A.INVERT), A.row(A.NORMALIZE, *mean, *std)]]
    assert float(np.abs(A.apply(ref[2], programs[2][:1])).max()) <= 1.0 and float(np.abs(ref).max()) <= 1.0      # A = 1 bounds the contrast rows' inputs
    got = _augment(vpx, x, programs)
    twin = A.apply_batch(ref, programs, twin=True)
    assert twin.dtype == np.float64
    _bounded(parity_log, f"contrast_{hw}_{C}_{tag}_single", got[0:1], twin[0:1], A.contrast_bound(programs[0], 1.0))
    _bounded(parity_log, f"contrast_{hw}_{C}_{tag}_chain", got[2:3], twin[2:3], A.contrast_bound(programs[2], 1.0))
    assert torch.equal(got[1].cpu(), torch.from_numpy(ref[1]))


HUE_CASES = {name: (x, programs) for name, x, programs in A.hue_cases()}


@pytest.mark.parametrize("name", list(HUE_CASES))
def test_hue_within_four_times_the_measured_deviation(vpx, parity_log, name):
    ref, programs = HUE_CASES[name]
    got = _augment(vpx, torch.from_numpy(ref).cuda(), programs)
    _bounded(parity_log, name, got, A.apply_batch(ref, programs, twin=True), A.HUE_FACTOR * A.HUE_F32_VS_F64)


def test_two_runs_give_equal_bits(vpx):
    x, ref = _frames(vpx, A.raw_bytes((33, 40), 3, seed=9), (-1.0, 1.0))
    programs = [[A.blend_row(A.CONTRAST, 1.3), A.row(A.AUTOCONTRAST), A.row(A.HUE, 0.2)], [A.row(A.AUTOCONTRAST), A.blend_row(A.CONTRAST, 0.5)], []]
    a = _augment(vpx, x.clone(), programs)
    b = _augment(vpx, x.clone(), programs)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, x)


# ---- datasets ----
AUGS = [("hflip", 0.5), ("erase", 1.0, (0.05, 0.3), (0.3, 3.3), (0.25, 0.5, 0.75)), ("vflip", 0.5), ("color_jitter", 0.4, 0.4, 0.4, 0.1),
        ("normalize", (0.5, 0.4, 0.3), 0.25)]


def _stored(vpx, **kw):
    raw = A.raw_bytes((9, 10), 3, seed=11, B=7, F=6)
    ds = vpx.datasets.StoredVPDataset("train", raw=raw, **kw)
    ds.set_seq_len(2, 1, 2)
    return raw, ds


def _restated(raw, augs, seed, indices, crop, twin=False):
    rng = np.random.default_rng(seed)
    out = []
    for i in indices:
        y0, x0, steps = A.draw_sequence(rng, augs, raw.shape[2:4], crop, (3,) + tuple(crop[1:]))
        v = R.preprocess(raw, R.table([i], [(y0, x0)]), 3, 2, crop_size=crop[1:])[0]
        out.append(A.apply_in_order(v, steps, twin))
    return np.stack(out)


def test_batch_equals_the_restatement_and_single_items(vpx, parity_log):
    """batch() against the restatement driven by the same seed: the user's list applied in order, flips as array flips. Colour jitter
    holds contrast and hue, so the comparison is bounded the way the hue cases are: four times the deviation between the float32 and the
    float64 restatement over these very inputs, measured here on the CPU (neither side is the code under test)."""
    crop = ("random", 6, 7)
    kw = dict(crop=crop, augmentations=AUGS, transform_seed=5)
    raw, a = _stored(vpx, **kw)
    _, b = _stored(vpx, **kw)
    order = [5, 2, 0, 6]
    want32, want64 = _restated(raw, AUGS, 5, order, crop), _restated(raw, AUGS, 5, order, crop, twin=True)
    deviation = float(np.abs(want32.astype(np.float64) - want64).max())
    print(f"max |float32 restatement - float64 twin| over the batch = {deviation:.3e}")
    assert 0 < deviation < 1e-4
    batch = a.batch(order)
    assert tuple(batch["frames"].shape) == (4, 3, 3, 6, 7)
    _bounded(parity_log, "batch_vs_restatement", batch["frames"], want64, A.HUE_FACTOR * deviation)
    items = [b[i] for i in order]
    _exact(parity_log, "batch_vs_items", batch["frames"], torch.stack([it["frames"] for it in items]).cpu().numpy())
    # without contrast and hue the same path is exact
    augs = [("hflip", 0.5), ("erase", 1.0, (0.05, 0.3), (0.3, 3.3), (0.25, 0.5, 0.75)), ("vflip", 0.5), ("color_jitter", 0.4, 0, 0.4, 0), ("autocontrast", 0.5),
            ("normalize", (0.5, 0.4, 0.3), 0.25)]
    _, c = _stored(vpx, crop=crop, augmentations=augs, transform_seed=8, value_range_min=-1.0)
    want = np.stack([A.apply_in_order(R.preprocess(raw, R.table([i], [(y0, x0)]), 3, 2, crop_size=crop[1:], value_range=(-1.0, 1.0))[0], steps)
                     for i, (y0, x0, steps) in zip(order, _draws(augs, 8, len(order), raw.shape[2:4], crop))])
    _exact(parity_log, "batch_exact_chain", c.batch(order)["frames"], want)


def _draws(augs, seed, n, frame_hw, crop):
    rng = np.random.default_rng(seed)
    return [A.draw_sequence(rng, augs, frame_hw, crop, (3,) + tuple(crop[1:])) for _ in range(n)]


def test_empty_programs_launch_nothing_and_change_nothing(vpx, parity_log):
    kw = dict(crop=("random", 6, 7), augmentations=[("hflip", 0.5), ("vflip", 0.5)], transform_seed=5, value_range_min=-1.0)
    raw, plain = _stored(vpx, **kw)
    never = [("hflip", 0.5), ("invert", 0.0), ("vflip", 0.5), ("solarize", 0.5, 0.0), ("erase", 0.0, (0.1, 0.2), (1, 2), 0), ("grayscale", 0.0)]
    _, ds = _stored(vpx, **{**kw, "augmentations": never})
    calls = []
    real = vpx.ops.frames_augment

    def counting(x, programs):
        calls.append(tuple(x.shape))
        return real(x, programs)

    vpx.ops.frames_augment = counting
    try:
        # the flip draws interleave with the unused probabilities' draws: compare against the restatement, and the launch count
        got = ds.batch([5, 2, 3])["frames"]
        off = ds.batch([1, 4])["frames"]
        ds.photometric, ds._flips_before = [("invert", 1.0)], [0]
        on = ds.batch([1])["frames"]
    finally:
        vpx.ops.frames_augment = real
    assert calls == [(1, 3, 3, 6, 7)]                                          # only the batch that drew a program launched
    rng = np.random.default_rng(5)
    want = []
    for i in (5, 2, 3):
        y0, x0, steps = A.draw_sequence(rng, never, (9, 10), ("random", 6, 7), (3, 6, 7))
        assert all(st[0] in ("hflip", "vflip") for st in steps)
        want.append(R.preprocess(raw, R.table([i], [(y0, x0)], [A.flip_bits(steps)]), 3, 2, crop_size=(6, 7), value_range=(-1.0, 1.0))[0])
    _exact(parity_log, "empty_programs", got, np.stack(want))
    assert tuple(off.shape) == (2, 3, 3, 6, 7) and tuple(on.shape) == (1, 3, 3, 6, 7)
    # a dataset without photometric entries is the existing path bit for bit
    rows = plain.table([5, 2])
    plain.reset_rng()
    _exact(parity_log, "flips_only", plain.batch([5, 2])["frames"], R.preprocess(raw, rows, 3, 2, crop_size=(6, 7), value_range=(-1.0, 1.0)))


def test_preprocess_makes_one_draw_for_the_whole_tensor(vpx, parity_log):
    augs = [("hflip", 0.5), ("erase", 1.0, (0.05, 0.3), (0.3, 3.3), 0.5), ("invert", 0.5), ("color_jitter", 0.4, 0, 0.4, 0), ("autocontrast", 0.5)]
    raw, ds = _stored(vpx, crop=("random", 6, 7), augmentations=augs, transform_seed=13)
    x = ds.preprocess(raw[3, :5])
    assert tuple(x.shape) == (5, 3, 6, 7)
    rng = np.random.default_rng(13)
    y0, x0, steps = A.draw_sequence(rng, augs, (9, 10), ("random", 6, 7), (3, 6, 7))
    want = A.apply_in_order(R.preprocess(raw[3:4], R.table([0], [(y0, x0)]), 5, crop_size=(6, 7))[0], steps)
    _exact(parity_log, "ds_preprocess_aug", x, want)
    state = ds.transform_rng.bit_generator.state
    assert state == rng.bit_generator.state                                    # ONE sequence's draws, whatever the number of frames
    plain = ds.preprocess(raw[3, 0], transform=False)
    _exact(parity_log, "ds_preprocess_plain_aug", plain, R.preprocess(raw[3:4], R.table([0]), 1)[0, 0])
    assert ds.transform_rng.bit_generator.state == state                       # transform=False: an empty program, no draw
    with pytest.raises(ValueError, match="1 or 3 channels"):
        ds.photometric = [("color_jitter", None, (0.6, 1.4), None, None)]
        ds.preprocess(np.zeros((2, 9, 10, 2), dtype=np.uint8))


def _write_split(root, split, raw):
    os.makedirs(os.path.join(root, split))
    for i, seq in enumerate(raw):
        np.save(os.path.join(root, split, f"seq_{i:05d}.npy"), seq)


def test_train_val_subsets_forward_the_programs(vpx, parity_log, tmp_path):
    raw = A.raw_bytes((8, 8), 1, seed=12, B=25, F=2)[..., 0]
    _write_split(str(tmp_path), "train", raw)
    augs = [("vflip", 0.5), ("invert", 0.5), ("erase", 1.0, (0.05, 0.3), (0.5, 2.0), (0.0, 0.5, 1.0)), ("color_jitter", 0.3, 0, 0.3, 0)]
    train, val = vpx.datasets.DATASET_CLASSES["MM"].get_train_val(data_dir=str(tmp_path), augmentations=augs, transform_seed=4)
    assert train.photometric == val.photometric == train.dataset.photometric and len(train.photometric) == 3 and train.config["photometric"] == train.photometric
    train.set_seq_len(1, 1, 1)
    files = [train.indices[i] for i in (0, 23, 7)] + [val.indices[0]]
    got = torch.cat([train.batch([0, 23, 7])["frames"], val[0]["frames"][None]])
    rng = np.random.default_rng(4)
    want = []
    for i in files:
        _, _, steps = A.draw_sequence(rng, augs, (8, 8), None, (3, 8, 8))
        want.append(A.apply_in_order(R.preprocess(raw, R.table([i]), 2, c_out=3)[0], steps))
    _exact(parity_log, "subsets_aug", got, np.stack(want))


def test_workbench_trains_on_augmented_stored_frames(vpx, tmp_path):
    import golden_cases as gc
    tiny = {k: v for k, v in gc.EF_TINY_KW.items() if k not in ("img_shape", "action_size", "tensor_value_range")}
    _write_split(str(tmp_path / "data"), "train", A.raw_bytes((16, 16), 1, seed=14, B=5, F=5)[..., 0])
    suite = vpx.VPSuite()
    suite.load_dataset("MM", split="train", data_dir=str(tmp_path / "data"), augmentations=AUGS)
    assert len(suite.training_sets[-1].train_data.photometric) == 3
    suite.create_model("convlstm-shi", **tiny)
    loss = suite.train(epochs=1, batch_size=2, context_frames=3, pred_frames=2, out_dir=str(tmp_path / "run"))
    assert np.isfinite(loss)
