"""Photometric augmentations and erasing without a GPU: parsing and refusals, the host draws of datasets.StoredVPDataset against the
restatement (tests/frames_aug_ref.py), the erasing draws and their mirroring through flips, vpx_frames_augment in a dry run, the ABI."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frames_aug_ref as A
from vp_suite_amd import DATASET_CLASSES, _lib
from vp_suite_amd.datasets import StoredVPDataset, procedural_digits
from vp_suite_amd.datasets.base import check_photometric, draw_erase_box, pack_programs, parse_augmentations, parse_photometric
from vp_suite_amd.ops import check_frames_programs


def _named(name, **attrs):
    return type(name, (), attrs)()


def test_every_tuple_and_object_form_parses():
    tuples = [("invert", 0.5), ("solarize", 0.5, 1), ("autocontrast", 0.25), ("grayscale", 0.1), ("normalize", 0.5, 0.25),
              ("normalize", (0.1, 0.2, 0.3), [1, 2, 3]), ("color_jitter", 0.4, 0.4, 0.4, 0.1), ("color_jitter", None, (0.5, 2), 0, (-0.2, 0.3)),
              ("erase", 0.5, (0.02, 0.33), (0.3, 3.3), 0), ("erase", 1, (0.1, 0.1), (1, 1), (0.1, 0.2, 0.3))]
    want = [("invert", 0.5), ("solarize", 0.5, 1.0), ("autocontrast", 0.25), ("grayscale", 0.1), ("normalize", (0.5,), (0.25,)),
            ("normalize", (0.1, 0.2, 0.3), (1.0, 2.0, 3.0)), ("color_jitter", (0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1)),
            ("color_jitter", None, (0.5, 2.0), None, (-0.2, 0.3)), ("erase", 0.5, (0.02, 0.33), (0.3, 3.3), (0.0,)),
            ("erase", 1.0, (0.1, 0.1), (1.0, 1.0), (0.1, 0.2, 0.3))]
    assert parse_photometric(tuples) == want and parse_photometric(None) == [] and parse_photometric([]) == []
    objects = [_named("RandomInvert", p=0.5), _named("RandomSolarize", threshold=0.5, p=1), _named("RandomAutocontrast", p=0.25),
               _named("RandomGrayscale", p=0.1), _named("Normalize", mean=0.5, std=0.25), _named("Normalize", mean=(0.1, 0.2, 0.3), std=[1, 2, 3]),
               _named("ColorJitter", brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1),
               _named("ColorJitter", brightness=None, contrast=(0.5, 2), saturation=0, hue=(-0.2, 0.3)),
               _named("RandomErasing", p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0),
               _named("RandomErasing", p=1, scale=(0.1, 0.1), ratio=(1, 1), value=(0.1, 0.2, 0.3))]
    assert parse_photometric(objects) == want
    assert parse_photometric([_named("Grayscale", num_output_channels=3)]) == [("grayscale", 1.0)]
    assert parse_photometric([("color_jitter", 2.0, None, None, None)]) == [("color_jitter", (0.0, 3.0), None, None, None)]    # max(0, 1 - x)


def test_refusals_before_any_launch():
    for bad, word in ((_named("RandomPosterize", bits=4, p=0.5), "byte tensors"), (("posterize", 4, 0.5), "byte tensors"),
                      (_named("RandomEqualize", p=0.5), "byte tensors"), (("equalize", 0.5), "byte tensors"),
                      (_named("GaussianBlur", kernel_size=3, sigma=1.0), "neighbourhood and geometric"), (("blur", 3, 1.0), "neighbourhood and geometric"),
                      (_named("RandomAdjustSharpness", sharpness_factor=2, p=0.5), "neighbourhood and geometric"),
                      (_named("RandomRotation", degrees=10), "neighbourhood and geometric"), (("rotate", 10), "neighbourhood and geometric"),
                      (_named("Grayscale", num_output_channels=1), "changes the frame shape"),
                      (("erase", 0.5, (0.02, 0.33), (0.3, 3.3), "random"), "random"),
                      (_named("RandomErasing", p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value="random"), "random"),
                      (_named("RandomPerspective"), "not part of this build"), (("invert",), "not part of this build"), (object(), "not part of this build")):
        with pytest.raises(NotImplementedError, match=word):
            parse_photometric([("invert", 0.5), bad])
    for bad, word in ((("invert", 1.5), "probability"), (("solarize", 0.5, -0.1), "probability"), (("autocontrast", 2), "probability"),
                      (("grayscale", -1), "probability"), (("erase", 1.01, (0.1, 0.2), (1, 2), 0), "probability"),
                      (("normalize", 0.5, 0.0), "zero std"), (("normalize", (0.1, 0.2, 0.3), (1, 0, 1)), "zero std"),
                      (("color_jitter", 0, 0, 0, 0.6), "hue"), (("color_jitter", 0, 0, 0, (-0.6, 0.1)), "hue"), (("color_jitter", 0, 0, 0, -0.1), "non negative"),
                      (("color_jitter", -0.1, 0, 0, 0), "non negative"), (("color_jitter", 0, (-0.5, 1.0), 0, 0), "negative factors"),
                      (("color_jitter", 0, 0, (1.5, 0.5), 0), "ordered"), (("erase", 0.5, (0.2, 1.2), (1, 2), 0), "scale"),
                      (("erase", 0.5, (0.1, 0.2), (0.0, 2), 0), "ratio")):
        with pytest.raises(ValueError, match=word):
            parse_photometric([bad])
    # what needs the channel count: checked when the stored frame shape is known
    gray, rgb, two = np.zeros((2, 3, 5, 6), dtype=np.uint8), np.zeros((2, 3, 5, 6, 3), dtype=np.uint8), np.zeros((2, 3, 5, 6, 2), dtype=np.uint8)
    for raw, bad, word in ((two, ("grayscale", 0.5), "3-channel"), (gray, ("grayscale", 0.5), "3-channel"), (two, ("color_jitter", 0, 0, 0.2, 0), "1 or 3 channels"),
                           (two, ("color_jitter", 0, 0, 0, 0.2), "1 or 3 channels"), (two, ("color_jitter", 0, 0.2, 0, 0), "1 or 3 channels"),
                           (rgb, ("normalize", (0.1, 0.2), 1.0), "mean entries"), (rgb, ("normalize", 0.5, (1, 2)), "std entries"),
                           (rgb, ("erase", 1.0, (0.1, 0.2), (1, 2), (0, 1)), "value entries"), (gray, ("erase", 1.0, (0.1, 0.2), (1, 2), (0, 1, 0)), "value entries")):
        with pytest.raises(ValueError, match=word):
            StoredVPDataset("train", raw=raw, augmentations=[("hflip", 0.5), bad])
    StoredVPDataset("train", raw=two, augmentations=[("color_jitter", 0.3, 0, 0, 0), ("invert", 0.5), ("normalize", (0.1, 0.2), 2.0), ("erase", 1.0, (0.1, 0.2), (1, 2), (0, 1))])
    StoredVPDataset("train", raw=gray, augmentations=[("color_jitter", 0.3, 0.3, 0.3, 0.3)])                  # saturation and hue: identity on one channel
    check_photometric(parse_photometric([("grayscale", 1.0)]), 3)


def test_flip_parser_keeps_its_contract_and_the_dataset_splits_the_list():
    jitter = _named("ColorJitter", brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1)
    with pytest.raises(NotImplementedError, match="ColorJitter"):
        parse_augmentations([("hflip", 0.5), jitter])
    with pytest.raises(NotImplementedError):
        parse_augmentations([("invert", 0.5)])
    raw = np.zeros((4, 3, 5, 6, 3), dtype=np.uint8)
    ds = StoredVPDataset("train", raw=raw, augmentations=[("hflip", 0.5), ("erase", 1.0, (0.1, 0.2), (1, 2), 0), _named("RandomVerticalFlip", p=0.25), jitter])
    assert ds.augmentations == [(1, 0.5), (2, 0.25)]
    assert ds.photometric == [("erase", 1.0, (0.1, 0.2), (1.0, 2.0), (0.0,)), ("color_jitter", (0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1))]
    assert ds._flips_before == [1, 2]
    cfg = ds.config
    assert cfg["photometric"] == ds.photometric and cfg["augmentations"] == ds.augmentations
    assert StoredVPDataset("train", raw=raw).photometric == [] and StoredVPDataset("train", raw=raw).config["photometric"] == []
    glyphs = procedural_digits(n=12, size=7)
    with pytest.raises(NotImplementedError, match="not part of this build"):
        DATASET_CLASSES["MMF"]("test", digits=glyphs, img_size=16, augmentations=[("invert", 0.5)])


def test_flips_only_draws_are_the_parent_commits():
    """Literal rows from the commit before photometric augmentations existed: the same seeds, the same table() rows."""
    raw = np.zeros((10, 6, 9, 10, 3), dtype=np.uint8)
    ds = StoredVPDataset("train", raw=raw, crop=("random", 6, 7), augmentations=[("hflip", 0.5), ("vflip", 0.5)], transform_seed=3)
    assert ds.table(list(range(6))).tolist() == [[0, 3, 0, 1], [1, 3, 2, 3], [2, 2, 1, 1], [3, 0, 0, 1], [4, 1, 1, 0], [5, 3, 3, 1]]
    ds = StoredVPDataset("train", raw=raw, augmentations=[("vflip", 0.3), ("hflip", 0.7)], transform_seed=11)
    rows, programs = ds.draws([4, 1, 7, 7, 0])
    assert rows.tolist() == [[4, 0, 0, 3], [1, 0, 0, 1], [7, 0, 0, 2], [7, 0, 0, 3], [0, 0, 0, 1]] and rows.dtype == np.int32 and programs == [[]] * 5
    assert ds.table([2, 3], transform=False).tolist() == [[2, 0, 0, 0], [3, 0, 0, 0]]


AUGS = [("hflip", 0.5), ("invert", 0.5), ("erase", 0.8, (0.05, 0.4), (0.3, 3.3), (0.25, 0.5, 0.75)), ("vflip", 0.5), ("solarize", 0.5, 0.5),
        ("color_jitter", 0.4, 0.4, 0.4, 0.1), ("autocontrast", 0.5), ("hflip", 0.5), ("grayscale", 0.3), ("normalize", (0.5, 0.4, 0.3), 0.25)]


def _mirrored(steps, hw):
    """The rows of `steps` with every erase box mirrored through the flips that follow it: what the launch is handed."""
    h, w = hw
    rows = []
    for k, st in enumerate(steps):
        if st[0] in ("hflip", "vflip"):
            continue
        if int(st[0]) == A.ERASE:
            y0, x0, eh, ew = st[1:5]
            for later in steps[k + 1:]:
                if later[0] == "hflip":
                    x0 = w - x0 - ew
                elif later[0] == "vflip":
                    y0 = h - y0 - eh
            st = (st[0], y0, x0, eh, ew) + st[5:]
        rows.append(st)
    return rows


def test_photometric_draws_follow_per_sequence_and_replay():
    raw = np.zeros((12, 3, 11, 13, 3), dtype=np.uint8)
    ds = StoredVPDataset("train", raw=raw, crop=("random", 8, 9), augmentations=AUGS, transform_seed=7)
    rows, programs = ds.draws(list(range(12)))
    rng = np.random.default_rng(7)
    kinds = set()
    for s in range(12):
        y0, x0, steps = A.draw_sequence(rng, AUGS, (11, 13), ("random", 8, 9), (3, 8, 9))
        assert rows[s].tolist() == [s, y0, x0, A.flip_bits(steps)]
        assert programs[s] == _mirrored(steps, (8, 9)), s
        kinds |= {int(r[0]) for r in programs[s]}
    assert kinds == set(range(1, 11))                                                  # every operation was drawn at least once
    assert len({len(p) for p in programs}) > 2 and all(int(p[-1][0]) == A.NORMALIZE for p in programs)
    again = ds.draws(list(range(12)))
    assert again[1] != programs
    ds.reset_rng()
    replay = ds.draws(list(range(12)))
    assert np.array_equal(replay[0], rows) and replay[1] == programs
    plain_rows, plain = ds.draws([3, 4], transform=False)
    assert plain == [[], []] and plain_rows.tolist() == [[3, 0, 0, 0], [4, 0, 0, 0]]
    packed = pack_programs(programs)
    assert packed.dtype == np.float32 and packed.shape == (12, 16, 9) and check_frames_programs(packed, 12) is not None
    for s in range(12):
        assert packed[s, len(programs[s]):, 0].max() == 0 and packed[s, :len(programs[s])].tolist() == [list(r) for r in programs[s]]
    assert pack_programs([[A.row(A.INVERT)] * 20, []]).shape == (2, 20, 9)
    with pytest.raises(ValueError, match="exceeds"):
        pack_programs([[A.row(A.INVERT)] * 65])


def test_double_hflip_bits():
    """Two flips of one kind that were both drawn cancel in the table's bits."""
    raw = np.zeros((40, 2, 4, 4), dtype=np.uint8)
    ds = StoredVPDataset("train", raw=raw, augmentations=[("hflip", 1.0), ("hflip", 1.0), ("vflip", 1.0)])
    assert set(ds.table(range(40))[:, 3].tolist()) == {2}


def test_erasing_draws():
    rng = np.random.default_rng(0)
    state = rng.bit_generator.state
    assert draw_erase_box(rng, (8, 8), (1.0, 1.0), (1.0, 1.0)) is None                   # a side of 8 is not < 8: ten attempts, no rectangle
    ten = np.random.default_rng(0)
    ten.bit_generator.state = state
    for _ in range(20):
        ten.uniform(0, 1)
    assert rng.bit_generator.state == ten.bit_generator.state                            # two uniforms per attempt, no corner
    seen = set()
    for hw in ((8, 8), (5, 9), (17, 19), (2, 2), (1, 1), (1, 5)):
        for _ in range(300):
            twin = np.random.default_rng(rng.integers(1 << 30))
            mine = np.random.default_rng()
            mine.bit_generator.state = twin.bit_generator.state
            box = draw_erase_box(mine, hw, (0.02, 0.6), (0.3, 3.3))
            assert box == A.erase_box(twin, hw, (0.02, 0.6), (0.3, 3.3))
            if box is not None:
                y0, x0, eh, ew = box
                assert 0 <= y0 and 0 <= x0 and 0 <= eh < hw[0] and 0 <= ew < hw[1] and y0 + eh <= hw[0] and x0 + ew <= hw[1]
                seen.add(hw)
    assert (8, 8) in seen and (17, 19) in seen and (1, 1) in seen                        # (1 x 1: only the empty 0 x 0 rectangle fits)
    ds = StoredVPDataset("train", raw=np.zeros((3, 2, 8, 8), dtype=np.uint8), augmentations=[("erase", 1.0, (1.0, 1.0), (1.0, 1.0), 0)])
    assert ds.draws([0, 1, 2])[1] == [[], [], []]                                        # the fallback: no rectangle, an empty program


@pytest.mark.parametrize("flips", [[("hflip", 1.0)], [("vflip", 1.0)], [("hflip", 1.0), ("vflip", 1.0)], [("hflip", 0.5), ("vflip", 0.5)]])
def test_rectangle_mirroring_equals_the_list_applied_in_order(flips):
    """flips everywhere first (the preprocess launch), then the mirrored rectangle == the user's list applied in order with array flips."""
    augs = [flips[0], ("erase", 1.0, (0.05, 0.3), (0.3, 3.3), (0.25, 0.5, 0.75))] + flips[1:] + [("invert", 1.0), ("erase", 1.0, (0.05, 0.2), (0.5, 2.0), 2.0)] \
        + [("hflip", 0.5)]
    raw = A.raw_bytes((7, 9), 3, seed=5, B=8, F=2)
    ds = StoredVPDataset("train", raw=raw, augmentations=augs, transform_seed=21)
    rows, programs = ds.draws(list(range(8)))
    rng = np.random.default_rng(21)
    x = A.scaled(raw, (0.0, 1.0))
    moved = 0
    for s in range(8):
        _, _, steps = A.draw_sequence(rng, augs, (7, 9), None, (3, 7, 9))
        want = A.apply_in_order(x[s], steps)
        v = x[s]
        if rows[s, 3] & 1:
            v = v[..., ::-1]
        if rows[s, 3] & 2:
            v = v[..., ::-1, :]
        got = A.apply(v, programs[s])
        assert np.array_equal(got, want), s
        moved += programs[s] != [st for st in steps if st[0] not in ("hflip", "vflip")]
    assert moved > 0                                                                     # some rectangle really was mirrored


def test_hue_tolerance_is_the_measured_one():
    got = A.measure_hue_deviation()
    print(f"max |float32 restatement - float64 twin| over the hue cases = {got:.4e} (recorded {A.HUE_F32_VS_F64:.4e}, factor {A.HUE_FACTOR})")
    assert 0.9 * A.HUE_F32_VS_F64 <= got <= A.HUE_F32_VS_F64


def test_restatement_facts():
    x = A.scaled(A.raw_bytes((3, 7), 3, seed=1), (0.0, 1.0))[0]
    assert np.array_equal(A.apply(A.apply(x, [A.row(A.INVERT)]), [A.row(A.INVERT)]) <= 1.0, np.ones_like(x, dtype=bool))
    gray = A.apply(x, [A.row(A.GRAY)])
    assert np.array_equal(gray[:, 0], gray[:, 1]) and np.array_equal(gray[:, 0], gray[:, 2]) and not np.array_equal(gray[:, 0], x[:, 0])
    assert np.array_equal(A.apply(x, [A.row(A.HUE, 0.0)]).round(5), x.round(5))          # hue 0 returns the colours (to rounding)
    const = np.full((1, 2, 3, 4), 0.25, dtype=np.float32)
    const[0, 1, 0, 0] = 0.5
    auto = A.apply(const, [A.row(A.AUTOCONTRAST)])
    assert np.array_equal(auto[0, 0], const[0, 0]) and auto[0, 1].max() == 1.0 and auto[0, 1].min() == 0.0
    one = A.scaled(A.raw_bytes((3, 7), 1, seed=2), (0.0, 1.0))[0]
    assert np.array_equal(A.apply(one, [A.blend_row(A.SATURATION, 0.3), A.row(A.HUE, 0.2)]), one)
    rows = [A.blend_row(A.CONTRAST, 1.3), A.row(A.INVERT), A.row(A.NORMALIZE, 0.5, 0.5, 0.5, 0, 0.25, 0.25, 0.25, 1)]
    err = np.abs(A.apply(x, rows).astype(np.float64) - A.apply(x, rows, twin=True)).max()
    assert A.apply(x, rows, twin=True).dtype == np.float64 and 0 < err <= A.contrast_bound(rows, 1.0) < 1e-5


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def aug(x=p(1), programs=p(2), B=128, F=20, C=3, h=64, w=64, max_ops=16):
    return L.vpx_frames_augment(x, programs, B, F, C, h, w, max_ops, None)
def refused(fn, rc, word, **kw):
    got = fn(**kw)
    assert got == rc and word in L.vpx_last_error(), (kw, got, L.vpx_last_error())
assert aug() == OK and aug(B=1, F=1, C=1, h=1, w=1) == OK and aug(C=4, h=17, w=19, max_ops=64) == OK and aug(C=2, h=32768, w=3) == OK
assert aug(x=ctypes.c_void_p(0x100000000004)) == OK              # any 4-byte alignment: element accesses
refused(aug, E_ARG, b"NULL", x=None)
refused(aug, E_ARG, b"NULL", programs=None)
for name in ("B", "F", "C", "h", "w"):
    refused(aug, E_ARG, b">= 1", **{name: 0})
    refused(aug, E_ARG, b">= 1", **{name: -3})
for bad in (0, 15, 65, -1):
    refused(aug, E_ARG, b"max_ops", max_ops=bad)
refused(aug, E_UNSUPPORTED, b"channels exceed", C=5)
refused(aug, E_UNSUPPORTED, b"a side beyond", h=32769)
refused(aug, E_UNSUPPORTED, b"a side beyond", w=32769)
refused(aug, E_UNSUPPORTED, b"exceed one launch", B=2 ** 31 - 1, F=2)
print("dry run ok")
"""


def test_entry_point_in_a_dry_run():
    """vpx_frames_augment under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide): valid calls with fake pointers pass
    every host-side check and launch nothing; each documented refusal returns its code and names its reason."""
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_abi_and_host_side_table_check():
    assert "vpx_frames_augment" in _lib.SIGNATURES and "vpx_frames_augment" in _lib.EXPORTED_SYMBOLS
    assert getattr(_lib.lib(), "vpx_frames_augment") is not None
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "vpx.h")) as fh:
        header = fh.read()
    assert "int vpx_frames_augment(float* x, const float* programs," in header and f"#define VPX_FRAMES_AUG_ROW {_lib.FRAMES_AUG_ROW}" in header
    assert (_lib.FRAMES_AUG_ROW, _lib.FRAMES_AUG_MIN_OPS, _lib.FRAMES_AUG_MAX_OPS) == (A.ROW, 16, 64)
    ok = A.pack([[A.row(A.INVERT)], []])
    assert check_frames_programs(ok, 2).shape == (2, 16, 9)
    for bad, word in ((ok[:1], "float32 table"), (ok.astype(np.float64), "float32 table"), (ok[:, :, :8], "float32 table"), (ok[:, :15], "rows per sample"),
                      (np.zeros((2, 65, 9), dtype=np.float32), "rows per sample")):
        with pytest.raises(ValueError, match=word):
            check_frames_programs(bad, 2)
    for value in (11.0, -1.0, 1.5, np.nan):
        bad = ok.copy()
        bad[1, 0, 0] = value
        with pytest.raises(ValueError, match="opcode"):
            check_frames_programs(bad, 2)
