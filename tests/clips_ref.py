"""Plain numpy / Python restatement of the long-clip storage model (vp_suite/datasets/kitti_raw.py, caltech_pedestrian.py) as
datasets/clips.py and vpx_clips_preprocess compute it: the window list, both split rules, and a window's frames — the clip sliced and
handed to the stored-frame arithmetic of tests/frames_ref.py, so there is ONE statement of the pixel contract on the reference side too.
The reference side of tests/test_clips_host.py (against tests/golden/clips_windows.npz, drawn from the upstream classes) and of
tests/test_gpu_clips.py."""
import random

import numpy as np

import frames_ref as R

TRAIN_VAL_SETS = [f"set{i:02d}" for i in range(6)]
TEST_SETS = [f"set{i:02d}" for i in range(6, 11)]


def windows(lengths, seq_len, seq_step):
    """[(clip, start), ...] in clip order: per clip range(0, frame_count - seq_len + 1, seq_len + seq_step - 1)."""
    return [(c, s) for c, n in enumerate(lengths) for s in range(0, n - seq_len + 1, seq_len + seq_step - 1)]


def kitti_split(names, split, trainval_to_test_ratio=0.8, train_to_val_ratio=0.9, trainval_test_seed=1234, train_val_seed=1234):
    """The drives of a split, sorted as upstream keeps them: names is the sorted list of <date>/<drive>."""
    names = list(names)
    if len(names) < 3:
        raise ValueError("found less than 3 sequences")
    cut = max(1, int(len(names) * trainval_to_test_ratio))
    random.Random(trainval_test_seed).shuffle(names)
    if split == "test":
        return sorted(names[cut:])
    names = names[:cut]
    cut = max(1, int(len(names) * train_to_val_ratio))
    random.Random(train_val_seed).shuffle(names)
    return sorted(names[:cut] if split == "train" else names[cut:])


def cp_split(names, split, train_to_val_ratio=0.9, train_val_seed=1234):
    """The videos of a split in upstream's order (shuffled for train / val): names is the sorted list of <setNN>/<Vxxx>."""
    if split == "test":
        names = [n for n in names if n.split("/")[-2] in TEST_SETS]
        if len(names) < 1:
            raise ValueError("didn't find enough test sequences")
        return names
    names = [n for n in names if n.split("/")[-2] in TRAIN_VAL_SETS]
    if len(names) < 2:
        raise ValueError("didn't find enough train/val sequences")
    cut = max(1, int(len(names) * train_to_val_ratio))
    random.Random(train_val_seed).shuffle(names)
    return names[:cut] if split == "train" else names[cut:]


def clip_first(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def table(wins, boxes=None, flips=None):
    """int32 [n, 6] rows (clip, start frame, crop y0, crop x0, flip bits, 0)."""
    n = len(wins)
    boxes = boxes or [(0, 0)] * n
    flips = flips or [0] * n
    return np.array([(c, s, y, x, f, 0) for (c, s), (y, x), f in zip(wins, boxes, flips)], dtype=np.int32).reshape(n, 6)


def preprocess(clips, rows, n_frames, seq_step=1, **kw):
    """[B, n_frames, C_out, oh, ow] from the clips [T_i, H, W(, Cs)] and rows of table(): per row the window
    clip[start : start + (n_frames - 1) * seq_step + 1] as a one-sequence source of frames_ref.preprocess (which applies the step)."""
    out = []
    for c, s, y0, x0, bits, _ in np.asarray(rows).tolist():
        span = (n_frames - 1) * seq_step + 1
        assert 0 <= c < len(clips) and 0 <= s and s + span <= clips[c].shape[0]
        out.append(R.preprocess(clips[c][s:s + span][None], R.table([0], [(y0, x0)], [bits]), n_frames, seq_step, **kw)[0])
    return np.ascontiguousarray(np.stack(out))
