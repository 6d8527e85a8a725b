"""CPU-side tests of the prediction visualizations (csrc/vis.hip, ops.vis_compose, vp_suite_amd/visualization.py): the numpy restatement
of tests/vis_ref.py against the fixture drawn from the upstream functions, the tile tables against the restatement, the table check, the
refusals the entry point makes before any launch, its dry run, and what the module does without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import vis_ref
from golden_util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_reference_fixture():
    """vis_ref.bordered / vis_ref.sheet on the regenerated inputs against add_borders / save_frame_compare_img of the reference, byte for byte."""
    g = load_golden("vis_layout")
    assert sorted(g) == ["bordered_GT", "bordered_Pred", "bordered_seg_x", "sheet"]
    inp = vis_ref.fixture_inputs()
    for name in vis_ref.FIXTURE_NAMES:
        got = vis_ref.bordered(inp[name], name, vis_ref.FIXTURE_CONTEXT)
        assert got.dtype == np.uint8 and got.shape == g[f"bordered_{name}"].shape == (5, 20, 28, 3)
        assert np.array_equal(got, g[f"bordered_{name}"]), name
    sheet = vis_ref.sheet(inp["GT"], [inp["Pred"], inp["seg_x"]], vis_ref.FIXTURE_CONTEXT, vis_ref.FIXTURE_SHEET_IDX)
    assert sheet.shape == g["sheet"].shape == (52, 130, 3) and np.array_equal(sheet, g["sheet"])
    video = vis_ref.video([inp[n] for n in vis_ref.FIXTURE_NAMES], vis_ref.FIXTURE_NAMES, vis_ref.FIXTURE_CONTEXT)
    assert np.array_equal(video, np.concatenate([g[f"bordered_{n}"] for n in vis_ref.FIXTURE_NAMES], axis=-2))
    # the three colour classes are all in the fixture: green throughout, green then red, yellow throughout
    assert [tuple(g[f"bordered_{n}"][t, 0, 0]) for n in vis_ref.FIXTURE_NAMES for t in (0, 4)] == \
        [(0, 200, 0), (0, 200, 0), (0, 200, 0), (150, 0, 0), (100, 100, 0), (100, 100, 0)]


def _paint(tiles, seqs, canvas_shape, background):
    """What the kernel is specified to do with a CHECKED table, in numpy, on byte sequences seqs [S][T, h, w, 3]."""
    canvas = np.full(canvas_shape, background, dtype=np.uint8)
    h, w = seqs[0].shape[1:3]
    for s, t, f, y0, x0, b, colour, _ in tiles:
        canvas[f, y0:y0 + h + 2 * b, x0:x0 + w + 2 * b] = ((colour >> 16) & 255, (colour >> 8) & 255, colour & 255)
        canvas[f, y0 + b:y0 + b + h, x0 + b:x0 + b + w] = seqs[s][t]
    return canvas


@pytest.mark.parametrize("hw", [(16, 24), (8, 8), (4, 6), (1, 1), (9, 7), (9, 13)])
def test_tile_tables_describe_the_reference_layouts(vpx, hw):
    """visualization.video_tiles / sheet_tiles, painted in numpy, equal the restatement; both pass check_vis_tiles; the video's tiles
    cover their canvas exactly (no fill) and the sheet's do not."""
    from vp_suite_amd import visualization as V
    names = ["GT", "pred_a", "Seg_b", "true_x", "other"]
    for S in (1, 2, 3, 5):
        for T, ctx in ((1, 0), (1, 1), (5, 0), (5, 2), (5, 5)):
            seqs = [vis_ref.seeded_bytes((T,) + hw + (3,), f"tab{S}{T}{i}") for i in range(S)]
            tiles, shape, b = V.video_tiles(names[:S], T, hw, ctx)
            assert b == min(hw) // 8 and tiles.dtype == np.int32 and tiles.shape == (S * T, 8)
            host, bmax, covered = vpx.ops.check_vis_tiles(tiles, S, T, hw, shape)
            assert bmax == b and covered and np.array_equal(host, tiles)
            assert np.array_equal(_paint(tiles, seqs, shape, 7), vis_ref.video(seqs, names[:S], ctx))
            for idx in ([], [0], [1, 1, 0], [-1]):
                if (not idx and T == ctx) or any(i >= T or i < -T for i in idx):
                    continue
                tiles, shape = V.sheet_tiles(S, T, hw, ctx, idx)
                _, bmax, covered = vpx.ops.check_vis_tiles(tiles, S, T, hw, shape)
                assert bmax == 0 and not covered                                   # (the gaps between the frames are background)
                assert np.array_equal(_paint(tiles, seqs, shape, 255)[0], vis_ref.sheet(seqs[0], seqs[1:], ctx, idx))
    with pytest.raises(ValueError, match="would be empty"):
        V.sheet_tiles(1, 3, hw, 3, [])


def test_border_colours_follow_the_reference_rules():
    from vp_suite_amd import visualization as V
    assert V.COLORS == {k: list(v) for k, v in vis_ref.COLORS.items()}
    assert V.get_color_array("red").shape == (1, 1, 1, 3) and V.get_color_array("red").dtype == np.uint8
    assert V.get_color_array("no such colour").ravel().tolist() == [255, 255, 255]
    for name in ("GT", "gt", "Gt", "TRUE_frames", "my_gt_seq", "seg", "pred_SEG_2", "Pred", "gtx", "true", "x"):
        for T, ctx in ((1, 0), (5, 2), (5, 5), (3, 7)):
            assert V.border_colors(name, T, ctx) == vis_ref.frame_colors(name, T, ctx), (name, T, ctx)
    assert V.border_colors("gt_seg", 2, 0) == ["green", "green"]            # the ground-truth rule comes first


def test_vis_table_is_checked_on_the_host(vpx):
    check = vpx.ops.check_vis_tiles
    ok = np.array([[0, 0, 0, 0, 0, 1, 0x00C800, 0], [1, 2, 0, 0, 8, 1, 0x960000, 0], [0, 1, 1, 4, 4, 0, 0, 0]], dtype=np.int64)   # 4 x 6 frames
    host, bmax, covered = check(ok, 2, 3, (4, 6), (2, 8, 16, 3))
    assert host.dtype == np.int32 and np.array_equal(host, ok) and bmax == 1 and not covered
    assert check(torch.from_numpy(ok), 2, 3, (4, 6), (2, 8, 16, 3))[0].shape == (3, 8)
    for row, col, bad, word in ((0, 0, 2, "sequence index"), (0, 0, -1, "sequence index"), (1, 1, 3, "frame index"), (1, 1, -1, "frame index"),
                                (2, 2, 2, "canvas frame"), (2, 2, -1, "canvas frame"), (0, 5, -1, "negative border"), (0, 3, 3, "leaves the"),
                                (0, 3, -1, "leaves the"), (1, 4, 9, "leaves the"), (1, 4, -1, "leaves the"), (0, 5, 3, "leaves the"), (0, 5, 2, "overlap"),
                                (2, 3, 5, "leaves the"), (1, 4, 7, "overlap"), (0, 6, 1 << 24, "colour"), (0, 6, -1, "colour"), (2, 7, 1, "reserved")):
        rows = ok.copy()
        rows[row, col] = bad
        with pytest.raises(ValueError, match=word):
            check(rows, 2, 3, (4, 6), (2, 8, 16, 3))
    both = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 3, 5, 0, 0, 0]])                    # one shared pixel
    with pytest.raises(ValueError, match="tiles 0 and 1 of canvas frame 0 overlap"):
        check(both, 2, 3, (4, 6), (1, 8, 16, 3))
    both[1, 2] = 1                                                                          # ... on different canvas frames: fine
    check(both, 2, 3, (4, 6), (2, 8, 16, 3))
    for bad in (np.zeros((2, 4), dtype=np.int32), np.zeros((0, 8), dtype=np.int32), np.zeros(8, dtype=np.int32), ok.astype(np.float32)):
        with pytest.raises(ValueError, match=re.escape("integer table [n_tiles, 8]")):
            check(bad, 2, 3, (4, 6), (2, 8, 16, 3))
    for shape in ((2, 8, 16), (2, 8, 16, 1), (0, 8, 16, 3)):
        with pytest.raises(ValueError, match="canvas"):
            check(ok, 2, 3, (4, 6), shape)


def test_abi_export_is_in_the_header_the_library_and_the_table():
    from vp_suite_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vpx.h")).read()
    assert re.search(r"\bint vpx_vis_compose\(const float\* src, int S, int T, int C, int h, int w, double lo, double hi, const int\* tiles,", hdr)
    assert "vpx_vis_compose" in _lib.SIGNATURES and "vpx_vis_compose" in _lib.EXPORTED_SYMBOLS
    fn = _lib.lib().vpx_vis_compose
    assert len(fn.argtypes) == 17 and fn.argtypes[0] is _lib.vp and fn.argtypes[6] is _lib.dbl and fn.argtypes[8] is _lib.vp and fn.argtypes[11] is _lib.vp
    assert "vpx_vis_compose" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(_lib.CSRC_DIR, "vis.hip")).read()
    # the float -> byte rule is the postprocess's device function, included, not restated
    assert '#include "frames_byte.h"' in src and "255.0f" not in src
    assert '#include "frames_byte.h"' in open(os.path.join(_lib.CSRC_DIR, "frames.hip")).read()


def test_refusals_before_any_launch(vpx):
    """NULL pointers, C not 1 or 3, hi <= lo, negative counts, a bad background and (with tiles) non-positive sizes are refused on the host
    (VPX_ERR_ARG = -1), without a GPU."""
    L = vpx._lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(src=p, S=1, T=1, C=3, h=2, w=2, lo=0.0, hi=1.0, tiles=p, n=1, bmax=0, canvas=p, F=1, Hc=2, Wc=2, bg=255)

    def call(**kw):
        a = {**ok, **kw}
        return L.vpx_vis_compose(a["src"], a["S"], a["T"], a["C"], a["h"], a["w"], a["lo"], a["hi"], a["tiles"], a["n"], a["bmax"], a["canvas"],
                                 a["F"], a["Hc"], a["Wc"], a["bg"], None)

    cases = [(dict(src=None), b"NULL"), (dict(tiles=None), b"NULL"), (dict(canvas=None), b"NULL"), (dict(C=2), b"source channels"),
             (dict(C=0), b"source channels"), (dict(C=4), b"source channels"), (dict(lo=0.5, hi=0.5), b"empty value range"),
             (dict(lo=1.0, hi=0.0), b"empty value range"), (dict(n=-1), b">= 0"), (dict(bmax=-1), b">= 0"), (dict(bg=256), b"background"),
             (dict(bg=-2), b"background")]
    cases += [({name: 0}, b">= 1") for name in ("S", "T", "h", "w", "F", "Hc", "Wc")] + [(dict(h=-3), b">= 1")]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in L.vpx_last_error(), (kw, L.vpx_last_error())
    assert call(Wc=40000) == -4 and b"side" in L.vpx_last_error()
    assert call(bmax=40000) == -4 and b"side" in L.vpx_last_error()


_DRY_RUN = r"""
import ctypes, importlib.util, sys
spec = importlib.util.spec_from_file_location("vpx_lib", sys.argv[1])   # the binding table alone: no torch in this process
_lib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_lib)
L = _lib.lib()
L.vpx_set_option(_lib.OPT_DRY_RUN, 1)
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
p = lambda i: ctypes.c_void_p(0x100000000000 + i * (1 << 36))   # fake device pointers: never dereferenced in a dry run
def compose(src=p(1), S=4, T=20, C=3, h=64, w=64, lo=0.0, hi=1.0, tiles=p(2), n=80, bmax=8, canvas=p(3), F=20, Hc=80, Wc=320, bg=-1):
    return L.vpx_vis_compose(src, S, T, C, h, w, lo, hi, tiles, n, bmax, canvas, F, Hc, Wc, bg, None)
def refused(rc, word, **kw):
    got = compose(**kw)
    assert got == rc and word in L.vpx_last_error(), (kw, got, L.vpx_last_error())
assert compose() == OK and compose(bg=255) == OK and compose(C=1, lo=-1.0) == OK and compose(bg=0, bmax=0) == OK
assert compose(S=1, T=1, h=1, w=1, n=1, bmax=0, F=1, Hc=1, Wc=1) == OK
assert compose(n=0, S=0, T=0, h=0, w=0, bg=255) == OK and compose(n=0, F=0, Hc=0, Wc=0, bg=255) == OK   # no tiles: the fill alone, or nothing
assert compose(n=2 ** 31 - 1, h=1, w=1, bmax=0) == OK            # a capped grid walks any table that one launch can count
for name in ("src", "tiles", "canvas"):
    refused(E_ARG, b"NULL", **{name: None})
for name in ("S", "T", "h", "w", "F", "Hc", "Wc"):
    refused(E_ARG, b">= 1", **{name: 0})
refused(E_ARG, b"source channels", C=2)
refused(E_ARG, b"empty value range", lo=1.0)
refused(E_ARG, b"empty value range", lo=2.0)
refused(E_ARG, b">= 0", n=-1)
refused(E_ARG, b">= 0", bmax=-1)
refused(E_ARG, b"background", bg=300)
refused(E_UNSUPPORTED, b"a side or border beyond", w=32769)
refused(E_UNSUPPORTED, b"a side or border beyond", Hc=32769)
refused(E_UNSUPPORTED, b"exceed one launch", n=2 ** 31 - 1, h=32768, w=32768, bmax=32768)
print("dry run ok")
"""


def test_entry_point_in_a_dry_run():
    """vpx_vis_compose under VPX_OPT_DRY_RUN, in a process of its own (the option is process-wide) on a machine without a GPU: valid
    calls with fake pointers pass every host-side check and neither fill nor launch (either would fail here); each documented refusal
    returns its code and names its reason."""
    from vp_suite_amd import _lib
    r = subprocess.run([sys.executable, "-c", _DRY_RUN, os.path.join(_lib._HERE, "_lib.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dry run ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_ops_and_module_refuse_host_tensors_and_bad_arguments(vpx):
    from vp_suite_amd import visualization as V
    tiles = np.array([[0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        vpx.ops.vis_compose(torch.zeros(1, 1, 3, 2, 2), tiles, (1, 2, 2, 3))
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        vpx.ops.vis_compose(np.zeros((1, 1, 3, 2, 2), dtype=np.float32), tiles, (1, 2, 2, 3))
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        V.compose_video([torch.zeros(2, 3, 4, 4)], 1, ["GT"])
    with pytest.raises(vpx.VpxError, match="GPU tensor"):
        V.compose_sheet(torch.zeros(2, 3, 4, 4), [], 1, [0])
    with pytest.raises(ValueError, match="cannot be mixed"):
        V.save_vid_vis("x.gif", 1, GT=np.zeros((2, 4, 4, 3), dtype=np.uint8), Pred=torch.zeros(2, 3, 4, 4))


def test_mp4_and_bad_vis_idx_raise_the_reference_errors(vpx, tmp_path):
    from vp_suite_amd import visualization as V
    with pytest.raises(NotImplementedError, match="gif-mode"):
        V.save_vid_vis(str(tmp_path / "x.mp4"), 2, mode="mp4", GT=np.zeros((3, 4, 4, 3), dtype=np.uint8))
    assert not os.listdir(tmp_path)

    class FiveSamples:
        NAME = "five"
        value_range_min, value_range_max = 0.0, 1.0

        def __len__(self):
            return 5

    for bad in (None, [5], [0, 7]):
        with pytest.raises(ValueError, match=re.escape(f"invalid vis_idx provided for visualization (dataset len = 5): {bad}")):
            V.visualize_sequences(FiveSamples(), 2, 2, [], "cuda", tmp_path, bad, None, "gif")
        with pytest.raises(ValueError, match=re.escape(f"invalid vis_idx provided for visualization (dataset len = 5): {bad}")):
            V.visualize_vid(FiveSamples(), 2, 2, None, "cuda", tmp_path, bad, "gif")
    assert not os.listdir(tmp_path)


def test_bytes_travel_through_the_float_rule_unchanged():
    """A postprocessed uint8 sequence reaches the kernel as byte + 0.5 in the range [0, 255] (visualization._stack): the float -> byte
    rule gives every byte back."""
    b = np.arange(256, dtype=np.float32).reshape(1, 1, 1, 256) + np.float32(0.5)
    assert np.array_equal(vis_ref.to_bytes(b, (0.0, 255.0))[0, 0, :, 0], np.arange(256, dtype=np.uint8))


def test_gif_and_png_are_written_through_pil(vpx, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vp_suite_amd import visualization as V
    inp = vis_ref.fixture_inputs()
    frames = vis_ref.video([inp[n] for n in vis_ref.FIXTURE_NAMES], vis_ref.FIXTURE_NAMES, vis_ref.FIXTURE_CONTEXT)   # [5, 20, 84, 3]
    V.write_gif(tmp_path / "v.gif", frames)
    with Image.open(tmp_path / "v.gif") as im:
        assert im.format == "GIF" and im.is_animated and im.n_frames == frames.shape[0] == 5 and im.size == (84, 20)
        durations = []
        for t in range(im.n_frames):
            im.seek(t)
            durations.append(im.info["duration"])
        assert durations == [V.GIF_FRAME_MS] * 5 == [500] * 5
    sheet = vis_ref.sheet(inp["GT"], [inp["Pred"], inp["seg_x"]], vis_ref.FIXTURE_CONTEXT, vis_ref.FIXTURE_SHEET_IDX)
    V.write_png(tmp_path / "s.png", torch.from_numpy(sheet))
    with Image.open(tmp_path / "s.png") as im:
        assert im.format == "PNG" and im.mode == "RGB" and np.array_equal(np.asarray(im), sheet)
    with pytest.raises(ValueError, match="uint8"):
        V.write_gif(tmp_path / "bad.gif", frames.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        V.write_png(tmp_path / "bad.png", sheet[..., :1])


def test_a_missing_pil_is_named(vpx, monkeypatch, tmp_path):
    from vp_suite_amd import visualization as V
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="please install pillow"):
        V.write_gif(tmp_path / "v.gif", np.zeros((1, 2, 2, 3), dtype=np.uint8))
    with pytest.raises(ImportError, match="please install pillow"):
        V.save_vid_vis(str(tmp_path / "v.gif"), 1, GT=np.zeros((1, 2, 2, 3), dtype=np.uint8))


def test_workbench_has_visualize_and_training_still_refuses_no_vis(vpx):
    import inspect
    sig = inspect.signature(vpx.VPSuite.visualize)
    assert list(sig.parameters)[:5] == ["self", "out_dir", "vis_idx", "vis_context_frame_idx", "vis_vid_mode"]
    assert sig.parameters["vis_context_frame_idx"].default is None and sig.parameters["vis_vid_mode"].default == "gif"
    suite = vpx.VPSuite(device="cpu")
    suite.models.append(object())
    suite.datasets.append(type("Set", (), {"is_training_set": lambda self: True, "is_test_set": lambda self: True})())
    with pytest.raises(NotImplementedError, match="no_vis=False"):
        suite.train(no_vis=False)
    with pytest.raises(NotImplementedError, match="no_vis=False"):
        suite.visualize("nowhere", [0], no_vis=False)
    with pytest.raises(NotImplementedError, match="gif-mode"):
        suite.visualize("nowhere", [0], vis_vid_mode="mp4")
    assert not os.path.exists("nowhere")
