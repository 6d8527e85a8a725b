"""csrc/vis.hip on the GPU (ops.vis_compose, vp_suite_amd/visualization.py): composed videos and comparison sheets against the numpy
restatement of tests/vis_ref.py, byte for byte.

Everything is EXACT (torch.equal): a border byte is a constant of the table, an inner byte is frames_postprocess's conversion (three
float32 operations, a clamp and a truncation, from the same device function), and a background byte is the fill. A differing byte is a
wrong address, a wrong tile or a drifted conversion, never noise.

The shapes are the smallest at which the kernel takes another path. A tile row is 3 (w + 2b) bytes, written as aligned 32-bit words with
single bytes at both ends: 16x24 (b = 2: 84 bytes, every row starts on a word), 8x8 (b = 1: 30 bytes, rows start at every phase of a
word), 4x6 and 1x1 (b = 0; 1x1: a row is ONE partial word), 9x7 (21 bytes: odd, b = 0) and 9x13 (b = 1: 45 bytes, odd with a border);
one and three channels; 1 to 3 sequences (the x offset of a tile moves its phase); 1 and 5 frames."""
import os

import numpy as np
import pytest
import torch

import vis_ref
from golden_util import load_golden

pytestmark = pytest.mark.gpu

SHAPES = [(16, 24), (8, 8), (4, 6), (1, 1), (9, 7), (9, 13)]
RANGES = [(0.0, 1.0), (-1.0, 1.0)]
NAMES = ["GT", "Pred", "seg_x"]        # green throughout; green then red; yellow throughout


def _frames(shape, value_range, seed):
    """float32 frames that leave the value range on both sides, with the special values at fixed places: below lo, above hi, exactly
    hi, exactly lo, NaN, +inf, -inf."""
    lo, hi = value_range
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), size=shape).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([lo - 1.0, hi + 1.0, hi, lo, np.nan, np.inf, -np.inf], dtype=np.float32)
    at = rng.permutation(flat.size)[:special.size]
    flat[at] = special[:at.size]
    return x


def _exact(parity_log, name, got, ref):
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    parity_log(name, got.float(), ref.float(), 0.0)
    assert torch.equal(got.cpu(), ref), f"{name}: {int((got.cpu() != ref).sum())} of {ref.numel()} bytes differ"


@pytest.mark.parametrize("hw", SHAPES)
def test_video_matches_restatement_and_postprocess(vpx, parity_log, hw):
    from vp_suite_amd import visualization as V
    b, seed = min(hw) // 8, 0
    for C in (3, 1):
        for S in (1, 2, 3):
            for T, contexts in ((1, (0, 1)), (5, (0, 2, 5))):
                for ctx in contexts:
                    seed += 1
                    vr = RANGES[seed % 2]
                    host = _frames((S, T, C) + hw, vr, 1000 * hw[0] + 10 * hw[1] + seed)
                    dev = torch.from_numpy(host).cuda()
                    tag = f"video {hw} C={C} S={S} T={T} ctx={ctx} {vr}"
                    got = V.compose_video(list(dev), ctx, NAMES[:S], *vr)
                    seqs = [vis_ref.to_bytes(host[s], vr) for s in range(S)]
                    _exact(parity_log, tag, got, vis_ref.video(seqs, NAMES[:S], ctx))
                    # the inner rectangles are frames_postprocess of the same tensor, byte for byte
                    post = vpx.ops.frames_postprocess(dev, *vr)                     # [S, T, h, w, C]
                    for s in range(S):
                        x0 = s * (hw[1] + 2 * b) + b
                        inner = got[:, b:b + hw[0], x0:x0 + hw[1], :]
                        assert torch.equal(inner, post[s].expand(-1, -1, -1, 3) if C == 1 else post[s]), (tag, s)


def test_video_equals_the_reference_fixture(vpx, parity_log):
    """The fixture's sequences (bytes, handed over as postprocessed uint8 arrays) through compose_video's own entry for them, against
    add_borders of the reference side by side."""
    from vp_suite_amd import visualization as V
    g = load_golden("vis_layout")
    inp = vis_ref.fixture_inputs()
    src, lo, hi = V._stack([inp[n] for n in vis_ref.FIXTURE_NAMES], 0.0, 1.0, "test")
    got = V.compose_video(src, vis_ref.FIXTURE_CONTEXT, vis_ref.FIXTURE_NAMES, lo, hi)
    _exact(parity_log, "video fixture", got, np.concatenate([g[f"bordered_{n}"] for n in vis_ref.FIXTURE_NAMES], axis=-2))
    sheet = V.compose_sheet(src[0], [src[1], src[2]], vis_ref.FIXTURE_CONTEXT, vis_ref.FIXTURE_SHEET_IDX, lo, hi)
    _exact(parity_log, "sheet fixture", sheet, g["sheet"])


@pytest.mark.parametrize("hw", SHAPES)
def test_sheet_matches_restatement(vpx, parity_log, hw):
    from vp_suite_amd import visualization as V
    seed = 0
    for C in (3, 1):
        for n_preds in (0, 2):
            for T, ctx in ((5, 2), (5, 0), (1, 0)):
                for idx in ([], [0], [1, 1, 0]):
                    if any(i >= T for i in idx):
                        continue
                    seed += 1
                    vr = RANGES[seed % 2]
                    host = _frames((1 + n_preds, T, C) + hw, vr, 77 * hw[0] + 3 * hw[1] + seed)
                    dev = torch.from_numpy(host).cuda()
                    got = V.compose_sheet(dev[0], list(dev[1:]), ctx, idx, *vr)
                    seqs = [vis_ref.to_bytes(host[s], vr) for s in range(1 + n_preds)]
                    _exact(parity_log, f"sheet {hw} C={C} preds={n_preds} T={T} ctx={ctx} idx={idx} {vr}", got, vis_ref.sheet(seqs[0], seqs[1:], ctx, idx))


def test_sliced_and_channels_last_sources(vpx, parity_log):
    """A src that is a view (every second frame of a longer sequence, a crop, channels-last strides) is read through one dense copy."""
    vr, hw = (0.0, 1.0), (9, 13)
    host = _frames((2, 10, 3, 11, 16), vr, 5)
    dev = torch.from_numpy(host).cuda()
    from vp_suite_amd import visualization as V
    views = {"every second frame": (dev[:, ::2], host[:, ::2]),
             "crop": (dev[:, :5, :, 1:10, 2:15], host[:, :5, :, 1:10, 2:15]),
             "channels last": (dev[:, :5, :, :9, :13].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3), host[:, :5, :, :9, :13])}
    for tag, (view, ref) in views.items():
        assert not view.is_contiguous(), tag
        before = view.clone()
        tiles, shape, _ = V.video_tiles(NAMES[:2], 5, tuple(view.shape[-2:]), 2)
        got = vpx.ops.vis_compose(view, tiles, shape, *vr)
        assert torch.equal(view, before), f"{tag}: the input was written"
        _exact(parity_log, f"view: {tag}", got, vis_ref.video([vis_ref.to_bytes(ref[s], vr) for s in range(2)], NAMES[:2], 2))


def test_unchecked_bad_rows_are_skipped_whole(vpx, parity_log):
    """A table handed over on the device is not checked: rows the kernel cannot run leave their canvas bytes at the background (and the
    guard bands around the canvas intact: conftest's canary), the good rows next to them are painted."""
    hw, vr = (4, 6), (0.0, 1.0)
    host = _frames((2, 3, 3) + hw, vr, 9)
    dev = torch.from_numpy(host).cuda()
    shape = (2, 8, 20, 3)
    good = [(0, 0, 0, 0, 0, 1, 0x00C800, 0), (1, 2, 1, 2, 13, 0, 0, 0)]
    bad = [(0, 1, 0, 3, 8, 1, 0x960000, 0),        # 6 x 8 at (3, 8): leaves the canvas at the bottom
           (0, 1, 1, 0, 13, 1, 0x960000, 0),       # ... at the right
           (2, 0, 0, 0, 10, 0, 0xFFFFFF, 0),       # s out of range
           (-1, 0, 0, 0, 10, 0, 0xFFFFFF, 0),
           (0, 3, 0, 0, 10, 0, 0xFFFFFF, 0),       # t out of range
           (0, 0, 2, 0, 10, 0, 0xFFFFFF, 0),       # f out of range
           (0, 0, -1, 0, 10, 0, 0xFFFFFF, 0),
           (0, 0, 0, 0, 10, -1, 0xFFFFFF, 0),      # negative border
           (0, 0, 0, 0, 10, 2, 0xFFFFFF, 0),       # border beyond max_border
           (0, 0, 0, -1, 10, 0, 0xFFFFFF, 0),      # negative origin
           (0, 0, 1, 0, -1, 0, 0xFFFFFF, 0),
           (0, 0, 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0xFFFFFF, 0)]
    table = torch.tensor(bad[:6] + good + bad[6:], dtype=torch.int32).cuda()
    got = vpx.ops.vis_compose(dev, table, shape, *vr, background=93, max_border=1)
    ref = np.full(shape, 93, dtype=np.uint8)
    ref[0, 0:6, 0:8] = (0, 200, 0)
    ref[0, 1:5, 1:7] = vis_ref.to_bytes(host[0, 0], vr)
    ref[1, 2:6, 13:19] = vis_ref.to_bytes(host[1, 2], vr)
    _exact(parity_log, "bad rows skipped", got, ref)
    with pytest.raises(ValueError, match="max_border"):
        vpx.ops.vis_compose(dev, table, shape, *vr)
    for row, word in ((bad[0], "leaves the"), (bad[2], "sequence index")):                    # the same rows from the host are refused
        with pytest.raises(ValueError, match=word):
            vpx.ops.vis_compose(dev, np.array(good + [row]), shape, *vr)


def test_two_calls_give_equal_bytes_and_arguments_are_checked(vpx):
    from vp_suite_amd import visualization as V
    vr, hw = (-1.0, 1.0), (9, 13)
    dev = torch.from_numpy(_frames((3, 5, 3) + hw, vr, 3)).cuda()
    a = V.compose_video(list(dev), 2, NAMES, *vr)
    b = V.compose_video(dev, 2, NAMES, *vr)                                  # (stacked already)
    assert torch.equal(a, b)
    s1, s2 = (V.compose_sheet(dev[0], [dev[1], dev[2]], 2, [0, 1], *vr) for _ in range(2))
    assert torch.equal(s1, s2)
    tiles, shape, _ = V.video_tiles(NAMES, 5, hw, 2)
    with pytest.raises(ValueError, match="float32"):
        vpx.ops.vis_compose(dev.double(), tiles, shape)
    with pytest.raises(ValueError, match=r"\[S, T, C, h, w\]"):
        vpx.ops.vis_compose(dev[0], tiles, shape)
    with pytest.raises(ValueError, match="source channels"):
        vpx.ops.vis_compose(dev[:, :, :2], tiles, shape)
    with pytest.raises(ValueError, match="empty value range"):
        vpx.ops.vis_compose(dev, tiles, shape, 1.0, 1.0)
    with pytest.raises(ValueError, match="grey level"):
        vpx.ops.vis_compose(dev, tiles, shape, background=256)
    with pytest.raises(ValueError, match="3 sequences, 2 names"):
        V.compose_video(dev, 2, NAMES[:2])


# ---- end to end: "MMF", an untrained convlstm-shi with a model_dir, visualize_sequences for two datapoints ----
def test_visualize_sequences_end_to_end(vpx, tmp_path):
    import golden_cases as gc
    from vp_suite_amd import visualization as V
    from vp_suite_amd.models import MODEL_CLASSES
    from vp_suite_amd.models.copy_last_frame import CopyLastFrame
    Image = pytest.importorskip("PIL.Image")
    ctx, n_pred, size = 3, 2, 32
    ds = vpx.DATASET_CLASSES["MMF"]("test", digits=vpx.datasets.procedural_digits(n=10, size=12), n_seqs=4, img_size=size, num_channels=3)
    ds.set_seq_len(ctx, n_pred, 1)
    torch.manual_seed(0)
    kw = {**gc.EF_TINY_KW, "img_shape": (3, size, size), "action_size": 0, "tensor_value_range": [0.0, 1.0]}
    model = MODEL_CLASSES["convlstm-shi"]("cuda", **kw).to("cuda")
    model.model_dir = str(tmp_path / "model")
    model.eval()                                                             # (the mode is to be left as it is found)
    baseline = CopyLastFrame().to("cuda")
    assert baseline.model_dir is None
    forwards = []
    hook = model.register_forward_hook(lambda m, args, out: forwards.append(out[0].detach().clone()))
    out = tmp_path / "vis"
    out.mkdir()
    ds.reset_rng()
    V.visualize_sequences(ds, ctx, n_pred, [baseline, model], "cuda", out, [1, 3], [0, 2], "gif")
    hook.remove()
    assert not model.training and len(forwards) == 2                         # one forward per (datapoint, model with a model_dir)
    assert sorted(os.listdir(out)) == ["vis_0.png", "vis_0_model_1.gif", "vis_1.png", "vis_1_model_1.gif", "vis_info.txt"]
    assert open(out / "vis_info.txt").read().splitlines() == [
        f"DATASET: {ds.NAME}", "chosen dataset idx: [1, 3]", "Displayed context frames: [0, 1, 2], ([0, 2] in seq_img)", "Displayed pred frames: [3, 4]",
        "Displayed rows (from top):", " - Ground Truth", f" - model 1: {model.NAME} (model dir: {model.model_dir})",
        "vis 0 (idx 1) origin: generated on-the-fly", "vis 1 (idx 3) origin: generated on-the-fly"]
    # the same two datapoints again (an on-the-fly set draws them in order, whatever the index): the composed arrays are vis_ref of the
    # ground truth and of the model's OWN prediction, as recorded by the hook
    ds.reset_rng()
    for i in range(2):
        frames = ds[i]["frames"]                                             # [5, 3, 32, 32]
        gt = vis_ref.to_bytes(frames.cpu().numpy())
        pred = vis_ref.to_bytes(torch.cat([frames[:ctx], forwards[i][0]], dim=0).cpu().numpy())
        video = vis_ref.video([gt, pred], ["GT", "Pred"], ctx)
        got = V.compose_video([frames, torch.cat([frames[:ctx], forwards[i][0]], dim=0)], ctx, ["GT", "Pred"]).cpu().numpy()
        assert np.array_equal(got, video)
        with Image.open(out / f"vis_{i}_model_1.gif") as im:
            assert im.n_frames == ctx + n_pred and im.size == (video.shape[2], video.shape[1])
        with Image.open(out / f"vis_{i}.png") as im:
            assert np.array_equal(np.asarray(im), vis_ref.sheet(gt, [pred], ctx, [0, 2]))
    model.train()
    V.get_vis_from_model(ds, ds[0], model, {"device": "cuda", "context_frames": ctx, "pred_frames": n_pred}, n_pred)
    assert model.training
