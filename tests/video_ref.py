"""Plain numpy / Python restatement of the three video datasets (vp_suite/datasets/human36m.py, physics101.py, synpick.py) as
datasets/human36m.py, physics101.py and synpick.py compute them — splits, window rules, action rows — and of a mixed-shape window's
frames: the clip sliced and handed to the stored-frame arithmetic of tests/frames_ref.py with the row's own box, so there is ONE statement
of the pixel contract on the reference side. The reference side of tests/test_video_host.py (against tests/golden/video_windows.npz,
drawn from the upstream classes) and of tests/test_gpu_video.py."""
import collections
import math
import random

import numpy as np

import frames_ref as R

SKIP_H36M, SKIP_SPM = 25, 72


def h36m_split(names, split, scenarios, train_to_val_ratio=0.96, train_val_seed=1234):
    """The videos of a split in upstream's order: names is the sorted list of <training|testing>/.../<Scenario ...> (no extension)."""
    part = "testing" if split == "test" else "training"
    names = [n for n in names if n.split("/")[0] == part and n.split("/")[-1].split(".")[0].split(" ")[0] in scenarios]
    if split == "test":
        return names
    cut = int(len(names) * train_to_val_ratio)
    random.Random(train_val_seed).shuffle(names)
    return names[:cut] if split == "train" else names[cut:]


def h36m_windows(lengths, seq_len, seq_step):
    return [(c, s) for c, n in enumerate(lengths) for s in range(SKIP_H36M, n - seq_len + 1, seq_len + seq_step - 1)]


def p101_split(names, split, trainval_to_test_ratio=0.8, trainval_test_seed=1612):
    names = list(names)
    cut = int(len(names) * trainval_to_test_ratio)
    random.Random(trainval_test_seed).shuffle(names)
    return names[:cut] if split == "train" else names[cut:]


def p101_start(frame_count, seq_len, subseq):
    """The stated departure: the window is taken from the whole video."""
    assert frame_count >= seq_len
    return {"start": 0, "end": frame_count - seq_len, "middle": (frame_count - seq_len) // 2}[subseq]


def spm_windows(lengths, positions, seq_len, seq_step):
    """(upstream's valid_idx over the concatenated episodes, the same as (episode, start) pairs, how often each rule rejected a start):
    synpick.py:58-94 walked as upstream walks it, ONE index over all frames."""
    first = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    episode_of = [c for c, n in enumerate(lengths) for _ in range(n)]
    offsets = range(0, seq_len, seq_step)
    last_valid, valid, wins, why = -seq_len, [], [], collections.Counter()
    for idx in range(first[-1] - seq_len + 1):
        ep = episode_of[idx]
        frame = idx - first[ep]
        if frame < SKIP_SPM:
            why["skip"] += 1
            continue
        if episode_of[idx + offsets[-1]] != ep:
            why["episode_end"] += 1
            continue
        if idx < last_valid + seq_len:
            why["overlap"] += 1
            continue
        pos = [positions[ep][frame + o] for o in offsets]
        deltas = [math.sqrt((float(b[0]) - float(a[0])) ** 2 + (float(b[1]) - float(a[1])) ** 2) for a, b in zip(pos, pos[1:])]
        if not sum(d > 1.0 for d in deltas) >= 0.67 * len(deltas):
            why["too_still"] += 1
            continue
        if not all(d < 30.0 for d in deltas):
            why["too_far"] += 1
            continue
        valid.append(idx)
        wins.append((ep, frame))
        last_valid = idx
    return valid, wins, why


def action_diffs(positions, start, n_frames, seq_step):
    """float32 [n_frames - 1, A]: numpy's (new - old) in the stored precision, then one rounding."""
    rows = np.asarray(positions)[start:start + (n_frames - 1) * seq_step + 1:seq_step]
    assert rows.shape[0] == n_frames
    return (rows[1:] - rows[:-1]).astype(np.float32)


def diffs_of_roundings(positions, start, n_frames, seq_step):
    """What a gather that rounds first and subtracts afterwards would give: NOT the contract."""
    rows = np.asarray(positions)[start:start + (n_frames - 1) * seq_step + 1:seq_step].astype(np.float32)
    return rows[1:] - rows[:-1]


def flat(clips):
    """(every clip's elements back to back, int64 [n, 4] rows (element offset, frames, H_i, W_i))."""
    channels = clips[0].shape[3] if clips[0].ndim == 4 else 1
    sizes = [c.size for c in clips]
    firsts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    geom = np.array([(o, c.shape[0], c.shape[1], c.shape[2]) for o, c in zip(firsts, clips)], dtype=np.int64).reshape(len(clips), 4)
    assert all(c.size == c.shape[0] * c.shape[1] * c.shape[2] * channels for c in clips)
    return np.concatenate([np.ascontiguousarray(c).reshape(-1) for c in clips]), geom


def table(wins, boxes, flips=None):
    """int32 [n, 8] rows (clip, start frame, box y0, box x0, box h, box w, flip bits, 0)."""
    n = len(wins)
    flips = flips or [0] * n
    return np.array([(c, s, y, x, h, w, f, 0) for (c, s), (y, x, h, w), f in zip(wins, boxes, flips)], dtype=np.int32).reshape(n, 8)


def whole(clips, wins):
    """The whole-frame box of every window's clip."""
    return [(0, 0, clips[c].shape[1], clips[c].shape[2]) for c, _ in wins]


def preprocess(clips, rows, n_frames, seq_step, out_size, **kw):
    """[B, n_frames, C_out, oh, ow] from clips [T_i, H_i, W_i(, Cs)] and rows of table(): per row the window sliced from its clip as a
    one-sequence source of frames_ref.preprocess with the row's box as the crop (float32 and bit-exact where the box has the output's
    size, float64 where it is resized)."""
    out = []
    for c, s, y0, x0, bh, bw, bits, _ in np.asarray(rows).tolist():
        span = (n_frames - 1) * seq_step + 1
        assert 0 <= c < len(clips) and 0 <= s and s + span <= clips[c].shape[0]
        out.append(R.preprocess(clips[c][s:s + span][None], R.table([0], [(y0, x0)], [bits]), n_frames, seq_step, crop_size=(bh, bw),
                                out_size=tuple(out_size), **kw)[0].astype(np.float64))
    return np.ascontiguousarray(np.stack(out))
