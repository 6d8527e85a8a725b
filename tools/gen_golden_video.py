"""Writes tests/golden/video_windows.npz: the splits and window tables of the UPSTREAM Human36MDataset and SynpickMovingDataset on a
synthetic tree without pixels (build container only, CPU, through tools/ref_shim.py; the fixture is committed, this tool is how it was
made). Physics 101 gets no upstream fixture: its windows are a stated departure (datasets/physics101.py).

The upstream classes read no pixel when they are built or when set_seq_len() lists their windows. Human 3.6M gets
{training,testing}/frame_counts.json whose keys are <root>/<name>.mp4 paths in sorted order (the order datasets/human36m.py fixes; its
docstring says so) — one length below seq_len + 25, two scenarios of which `scenarios=` keeps one. SynPick gets, per split,
rgb/<episode>_<frame>.png files of zero bytes and scene_gt/<episode>_scene_gt.json files whose last object per frame carries the gripper
position: two episodes of 120 frames, a seeded random walk with a stretch at rest and one jump each, so that every rejection rule of
synpick.py:58-94 fires (asserted below through tests/video_ref.py). cv2 is a stub of the shim and is never called. The names are
tools/export_video_like.py's, so a test can export a readable tree of the same names and lengths.

h36m_names [n] / h36m_lengths [n] (the whole tree, sorted), h36m_scenarios, and per split S: h36m_S_seqs [m] (indices into h36m_names in
the order of upstream's `sequences`), h36m_S_win_L_P [k, 2] = upstream's sequences_with_frame_index as (index into h36m_S_seqs, start
frame) for (seq_len L, seq_step P) in (4, 1), (5, 2), (7, 3). spm_lengths [2], and per split S: spm_S_gripper [240, 3] float64 (both
episodes, back to back), spm_S_valid_L_P = upstream's valid_idx, spm_S_diff_first_L_P / _diff_last_L_P = upstream's
_get_gripper_pos_diff for the first and last valid window (float64, as upstream forms them before .float()).

    python tools/gen_golden_video.py"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import export_video_like as X  # noqa: E402
import video_ref as V  # noqa: E402
from ref_shim import load_reference  # noqa: E402

CONFIGS = [(4, 1), (5, 2), (7, 3)]                    # (seq_len, seq_step)
SPLITS = ("train", "val", "test")
H36M_LENGTHS = [31, 40, 27, 52, 33, 45, 29, 60, 36, 41, 30, 47, 28, 38, 55, 43]   # 27 < 4 + 25: no window at any configuration
H36M_SCENARIOS = ["WalkingDog"]                       # "Directions" is filtered out
SPM_LENGTHS = [120, 120]


def frames_for(seq_len, seq_step):
    total, rest = divmod(seq_len - 1, seq_step)
    assert rest == 0
    return total + 1


def spm_gripper(split):
    """Both episodes' tracks [120, 3]: the export tool's random walk with a stretch at rest and one jump."""
    tracks = []
    for k, name in enumerate(X.spm_names(len(SPM_LENGTHS), split)):
        steps = np.diff(X.synthetic_gripper(name, SPM_LENGTHS[k], seed=11), axis=0, prepend=0.0)
        steps[84 + 6 * k:96 + 6 * k, :2] *= 0.01      # at rest: most xy distances fall below 1.0
        steps[104 + 3 * k, :2] += 40.0                # a jump: one xy distance beyond 30.0
        tracks.append(np.cumsum(steps, axis=0))
    return tracks


def main():
    load_reference()
    from vp_suite.datasets.human36m import Human36MDataset
    from vp_suite.datasets.synpick import SynpickMovingDataset
    out = {}
    tmp = tempfile.mkdtemp(prefix="video_golden_")

    h_dir = os.path.join(tmp, "h36m")
    names = X.h36m_names(len(H36M_LENGTHS))
    for part in ("training", "testing"):
        os.makedirs(os.path.join(h_dir, part))
        with open(os.path.join(h_dir, part, "frame_counts.json"), "w") as fh:
            json.dump({os.path.join(h_dir, n + ".mp4"): c for n, c in zip(names, H36M_LENGTHS) if n.split(os.sep)[0] == part}, fh)
    out["h36m_names"], out["h36m_lengths"], out["h36m_scenarios"] = np.array(names), np.array(H36M_LENGTHS, dtype=np.int64), np.array(H36M_SCENARIOS)
    for split in SPLITS:
        ds = Human36MDataset(split, data_dir=h_dir, scenarios=list(H36M_SCENARIOS))
        seqs = [os.path.relpath(p, h_dir)[:-len(".mp4")] for p in ds.sequences]
        out[f"h36m_{split}_seqs"] = np.array([names.index(s) for s in seqs], dtype=np.int64)
        for seq_len, seq_step in CONFIGS:
            ds.sequences_with_frame_index = []        # (upstream appends to the list of an earlier call)
            ds.set_seq_len(1, frames_for(seq_len, seq_step) - 1, seq_step)
            assert ds.seq_len == seq_len
            rows = [(seqs.index(os.path.relpath(p, h_dir)[:-len(".mp4")]), start) for p, start in ds.sequences_with_frame_index]
            out[f"h36m_{split}_win_{seq_len}_{seq_step}"] = np.array(rows, dtype=np.int64).reshape(len(rows), 2)

    s_dir = os.path.join(tmp, "spm")
    out["spm_lengths"] = np.array(SPM_LENGTHS, dtype=np.int64)
    fired = set()
    for split in SPLITS:
        tracks = spm_gripper(split)
        rgb, gt = os.path.join(s_dir, "processed", split, "rgb"), os.path.join(s_dir, "processed", split, "scene_gt")
        os.makedirs(rgb)
        os.makedirs(gt)
        for ep, track in enumerate(tracks):
            for f in range(track.shape[0]):
                open(os.path.join(rgb, f"{ep:06d}_{f:06d}.png"), "w").close()
            with open(os.path.join(gt, f"{ep:06d}_scene_gt.json"), "w") as fh:   # two objects per frame: the LAST one is the gripper
                json.dump({str(f): [{"cam_t_m2c": [0.0, 0.0, 0.0]}, {"cam_t_m2c": [float(v) for v in track[f]]}] for f in range(track.shape[0])}, fh)
        out[f"spm_{split}_gripper"] = np.concatenate(tracks)
        ds = SynpickMovingDataset(split, data_dir=s_dir)
        for seq_len, seq_step in CONFIGS:
            ds.set_seq_len(1, frames_for(seq_len, seq_step) - 1, seq_step)
            assert ds.seq_len == seq_len and len(ds.valid_idx) >= 2
            out[f"spm_{split}_valid_{seq_len}_{seq_step}"] = np.array(ds.valid_idx, dtype=np.int64)
            for tag, i in (("first", ds.valid_idx[0]), ("last", ds.valid_idx[-1])):
                idx = range(i, i + ds.seq_len, ds.seq_step)                      # synpick.py:103-110
                ep_num = ds._ep_num_from_id(ds.image_ids[idx[0]])
                frame_nums = [ds._frame_num_from_id(ds.image_ids[id_]) for id_ in idx]
                out[f"spm_{split}_diff_{tag}_{seq_len}_{seq_step}"] = ds._get_gripper_pos_diff([ds.gripper_pos[ep_num][f] for f in frame_nums])
            valid, _, why = V.spm_windows(SPM_LENGTHS, tracks, seq_len, seq_step)
            assert valid == ds.valid_idx, (split, seq_len, seq_step)
            fired |= {k for k, n in why.items() if n}
    assert fired == {"skip", "episode_end", "overlap", "too_still", "too_far"}, fired

    target = os.path.join(ROOT, "tests", "golden", "video_windows.npz")
    np.savez_compressed(target, **out)
    print(f"wrote {target}: {len(out)} arrays, {os.path.getsize(target)} bytes")
    for k in sorted(out):
        if out[k].size <= 40:
            print(k, out[k].tolist())


if __name__ == "__main__":
    main()
