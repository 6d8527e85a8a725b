"""Plain numpy restatement of the visualization layouts (vp_suite/utils/visualization.py: add_borders, the side-by-side concatenation of
save_vid_vis's mp4 branch, save_frame_compare_img) as csrc/vis.hip composes them: the reference side of tests/test_vis_host.py (against
the fixture drawn from the upstream functions, tests/golden/vis_layout.npz) and of tests/test_gpu_vis.py.

Everything here works on BYTES [T, h, w, 3]; to_bytes() is the float -> byte rule of tests/frames_ref.py (postprocess), with the grey
repeat for one-channel frames. Written independently of vp_suite_amd/visualization.py: slices and loops, no tile tables."""
import numpy as np

import frames_ref
from golden_util import name_seed, seeded_rand

COLORS = {"green": (0, 200, 0), "red": (150, 0, 0), "yellow": (100, 100, 0), "black": (0, 0, 0), "white": (255, 255, 255)}

# the inputs of tests/golden/vis_layout.npz (tools/gen_golden_vis.py): seeded bytes, regenerated wherever they are needed
FIXTURE_NAMES = ("GT", "Pred", "seg_x")
FIXTURE_T, FIXTURE_HW, FIXTURE_CONTEXT = 5, (16, 24), 2
FIXTURE_SHEET_IDX = [0, 1]


def seeded_bytes(shape, tag):
    """uint8 array of `shape` from the seeded CPU generator of tests/golden_util.py (machine independent)."""
    return np.floor(seeded_rand(shape, name_seed(tag)).numpy().astype(np.float64) * 256.0).clip(0, 255).astype(np.uint8)


def fixture_inputs():
    """{name: uint8 [5, 16, 24, 3]} for the three sequences of the fixture (the sheet takes GT as ground truth and the other two as predictions)."""
    h, w = FIXTURE_HW
    return {n: seeded_bytes((FIXTURE_T, h, w, 3), f"vis_layout_{n}") for n in FIXTURE_NAMES}


def to_bytes(x, value_range=(0.0, 1.0)):
    """uint8 [..., h, w, 3] from float32 [..., c, h, w] (c = 1 or 3): frames_ref.postprocess, a single channel repeated three times."""
    out = frames_ref.postprocess(np.asarray(x, dtype=np.float32), value_range)
    return np.repeat(out, 3, axis=-1) if out.shape[-1] == 1 else out


def border_width(h, w):
    return min(h, w) // 8


def frame_colors(name, T, context_frames):
    key = name.lower()
    if key == "gt" or "true_" in key or "gt_" in key:
        return ["green"] * T
    if "seg" in key:
        return ["yellow"] * T
    return ["green"] * min(context_frames, T) + ["red"] * max(T - context_frames, 0)


def bordered(seq, name, context_frames):
    """uint8 [T, h + 2b, w + 2b, 3]: seq [T, h, w, 3] inside its per-frame border."""
    T, h, w, _ = seq.shape
    b = border_width(h, w)
    out = np.empty((T, h + 2 * b, w + 2 * b, 3), dtype=np.uint8)
    for t, color in enumerate(frame_colors(name, T, context_frames)):
        out[t] = np.array(COLORS[color], dtype=np.uint8)
        out[t, b:b + h, b:b + w] = seq[t]
    return out


def video(seqs, names, context_frames):
    """uint8 [T, h + 2b, S (w + 2b), 3]: the bordered sequences next to each other."""
    return np.concatenate([bordered(s, n, context_frames) for s, n in zip(seqs, names)], axis=2)


def sheet(gt, preds, context_frames, vis_context_frame_idx, border=2):
    """uint8 [H, W, 3]: the comparison image, white where no frame stands. Context column n at x = n (w + border); predicted frame t of row
    n at y = n (h + border), x = W_context + (t - context_frames) (w + border) + border."""
    seqs = [gt] + list(preds)
    T, h, w, _ = gt.shape
    hb, wb = h + border, w + border
    H, w_context = hb * len(seqs) - border, wb * len(vis_context_frame_idx)
    img = np.full((H, w_context + wb * (T - context_frames), 3), 255, dtype=np.uint8)
    for n, i in enumerate(vis_context_frame_idx):
        img[:h, n * wb:n * wb + w] = gt[i]
    for n, seq in enumerate(seqs):
        for t in range(context_frames, T):
            x = w_context + (t - context_frames) * wb + border
            img[n * hb:n * hb + h, x:x + w] = seq[t]
    return img
