"""Prediction visualizations (vp_suite/utils/visualization.py), restated on ONE HIP launch per output: a bordered side-by-side video of
ground truth and prediction, and a sheet that shows the predictions of several models below the ground truth frame by frame.

The reference builds both with numpy on postprocessed frames: np.tile / np.concatenate per border, a Python loop per frame. Here the
frames stay where the model left them: the sequences of one output are stacked once, a small table says which frame goes where with which
border (video_tiles / sheet_tiles, host integers only), ops.vis_compose paints the whole canvas on the GPU — the inner rectangles are
ops.frames_postprocess's bytes, from the same device function — and the canvas comes to the host in one copy, where PIL writes it.

    compose_video(seqs, context_frames, names, lo, hi)        uint8 [T, h + 2b, S (w + 2b), 3]: add_borders + the side-by-side concatenation
    compose_sheet(gt, preds, context_frames, idx, lo, hi)     uint8 [H, W, 3]: save_frame_compare_img's image
    save_vid_vis / save_frame_compare_img / get_vis_from_model / visualize_vid / visualize_sequences: the reference's entry points.

WHAT DIFFERS FROM THE REFERENCE, all of it here:
  * A GIF holds the composed side-by-side frames themselves (the layout of the reference's mp4 branch), 500 ms per frame, written by
    PIL: no matplotlib figure, so no titles above the videos, and no imagemagick.
  * One-channel frames are shown as grey RGB (the reference's sheet would be one-channel, its videos need three channels).
  * mode="mp4" raises NotImplementedError: there is no encoder in this build.
  * get_vis_from_model returns the two sequences as float GPU tensors [T, c, h, w] in the dataset's value range, not as postprocessed
    numpy arrays: the bytes are made inside the compose launch. save_vid_vis and save_frame_compare_img take such tensors (with
    value_range=) as well as the reference's uint8 arrays [T, h, w, c].
  * A model may be given as (model, preprocessing, postprocessing): the frame adapters of compatibility.check_model_and_data_compat, so
    that a model of another value range or frame size is shown in the dataset's format (VPSuite.visualize does; the reference hands
    visualize_sequences the bare models).
  * Actions go to action-conditional models only, as in VPSuite.test()."""
from pathlib import Path

import numpy as np
import torch

from . import ops

COLORS = {
    "green": [0, 200, 0],
    "red": [150, 0, 0],
    "yellow": [100, 100, 0],
    "black": [0, 0, 0],
    "white": [255, 255, 255]
}  #: border colours of the video visualizations (r, g, b)

SHEET_BORDER = 2          # save_frame_compare_img: pixels between the frames of the sheet
SHEET_BACKGROUND = 255    # ... and their grey level
GIF_FRAME_MS = 500        # FuncAnimation(interval=500)


def get_color_array(color: str):
    """uint8 [1, 1, 1, 3]: the (r, g, b) of a COLORS key, white for any other string."""
    return np.array(COLORS.get(color, COLORS["white"]), dtype=np.uint8)[np.newaxis, np.newaxis, np.newaxis, ...]


def _rgb_word(color: str) -> int:
    r, g, b = COLORS.get(color, COLORS["white"])
    return (r << 16) | (g << 8) | b


def border_colors(name: str, n_frames: int, context_frames: int):
    """The colour name of every frame's border (add_borders): a sequence called `gt`, or with `true_` / `gt_` in its name, is green
    throughout; one with `seg` yellow; any other green for the context frames and red after. Case does not matter."""
    key = name.lower()
    if "true_" in key or "gt_" in key or key == "gt":
        return ["green"] * n_frames
    if "seg" in key:
        return ["yellow"] * n_frames
    return ["green" if t < context_frames else "red" for t in range(n_frames)]


def video_tiles(names, n_frames, frame_hw, context_frames):
    """(int32 table [S * T, 8], canvas shape, b) of the side-by-side video: sequence i of frame t at x = i (w + 2b) of canvas frame t, inside
    a border of b = min(h, w) // 8 pixels. The tiles cover the canvas exactly."""
    h, w = frame_hw
    b = min(h, w) // 8
    rows = []
    for i, name in enumerate(names):
        for t, color in enumerate(border_colors(name, n_frames, context_frames)):
            rows.append((i, t, t, 0, i * (w + 2 * b), b, _rgb_word(color), 0))
    return np.array(rows, dtype=np.int32).reshape(-1, 8), (n_frames, h + 2 * b, len(names) * (w + 2 * b), 3), b


def sheet_tiles(n_seqs, n_frames, frame_hw, context_frames, vis_context_frame_idx):
    """(int32 table, canvas shape) of save_frame_compare_img's image, its geometry kept as it is: sequence 0 is the ground truth, context
    column n shows its frame vis_context_frame_idx[n] at x = n (w + 2) in the top row; the predicted frames t >= context_frames of row n
    stand at y = n (h + 2), x = W_context + (t - context_frames) (w + 2) + 2 — the gap comes BEFORE a prediction column and AFTER a context
    column; H = (h + 2) rows - 2. No tile has a border of its own."""
    h, w = frame_hw
    hb, wb = h + SHEET_BORDER, w + SHEET_BORDER
    idx = [int(i) for i in vis_context_frame_idx]
    H = hb * n_seqs - SHEET_BORDER
    w_context = wb * len(idx)
    W = w_context + wb * (n_frames - context_frames)
    rows = [(0, i if i >= 0 else i + n_frames, 0, 0, n * wb, 0, 0, 0) for n, i in enumerate(idx)]   # (a negative index counts from the end, as numpy's)
    for n in range(n_seqs):
        for t in range(context_frames, n_frames):
            rows.append((n, t, 0, n * hb, w_context + (t - context_frames) * wb + SHEET_BORDER, 0, 0, 0))
    if not rows or H < 1 or W < 1:
        raise ValueError(f"the comparison image would be empty ({n_seqs} rows of {h}x{w} frames, {len(idx)} context and "
                         f"{n_frames - context_frames} predicted columns)")
    return np.array(rows, dtype=np.int32).reshape(-1, 8), (1, H, W, 3)


def _stack(seqs, lo, hi, what):
    """(float32 GPU tensor [S, T, c, h, w], lo, hi) from sequences that are float GPU tensors [T, c, h, w] in [lo, hi] or postprocessed
    uint8 arrays / tensors [T, h, w, c]. Bytes travel as byte + 0.5 in the range [0, 255]: ((v + 0.5) / 255) * 255 lies within 1e-4 of
    v + 0.5 in float32, so the truncation gives every byte back. Floats and bytes cannot be mixed (one launch has one value range)."""
    seqs = list(seqs)
    if not seqs:
        raise ValueError(f"{what}: no sequences given")
    as_bytes = [isinstance(s, np.ndarray) or (torch.is_tensor(s) and s.dtype == torch.uint8) for s in seqs]
    if any(as_bytes):
        if not all(as_bytes):
            raise ValueError(f"{what}: float tensors and uint8 arrays cannot be mixed in one visualization")
        if not torch.cuda.is_available():
            raise ops._lib.VpxError(f"{what}: visualizations are composed by a HIP kernel on the GPU, there is no CPU fallback")
        dev = []
        for s in seqs:
            s = torch.from_numpy(np.ascontiguousarray(s)) if isinstance(s, np.ndarray) else s
            if s.dtype != torch.uint8 or s.ndim != 4:
                raise ValueError(f"{what}: postprocessed sequences are uint8 [T, h, w, c] (got {s.dtype} {tuple(s.shape)})")
            dev.append(s.cuda().permute(0, 3, 1, 2).float() + 0.5)
        seqs, lo, hi = dev, 0.0, 255.0
    for s in seqs:
        if not (torch.is_tensor(s) and s.is_cuda):
            raise ops._lib.VpxError(f"{what}: sequences must be GPU tensors; visualizations are composed by a HIP kernel, there is no CPU fallback")
        if s.ndim != 4 or s.shape != seqs[0].shape:
            raise ValueError(f"{what}: every sequence is [T, c, h, w] of one shape (got {[tuple(x.shape) for x in seqs]})")
    return torch.stack([s.detach().float() for s in seqs]), float(lo), float(hi)


def compose_video(seqs, context_frames, names, lo=0.0, hi=1.0):
    """uint8 GPU tensor [T, h + 2b, S (w + 2b), 3]: the S sequences `seqs` (float GPU tensors [T, c, h, w] in [lo, hi], or one stacked
    tensor [S, T, c, h, w]) side by side, each inside its border — add_borders followed by np.concatenate(axis=-2). One launch."""
    names = list(names)
    src = seqs if torch.is_tensor(seqs) and seqs.ndim == 5 else _stack(seqs, lo, hi, "compose_video")[0]
    if src.shape[0] != len(names):
        raise ValueError(f"compose_video: {src.shape[0]} sequences, {len(names)} names")
    T, h, w = int(src.shape[1]), int(src.shape[3]), int(src.shape[4])
    tiles, canvas_shape, _ = video_tiles(names, T, (h, w), int(context_frames))
    return ops.vis_compose(src, tiles, canvas_shape, lo, hi)


def compose_sheet(gt, preds, context_frames, vis_context_frame_idx, lo=0.0, hi=1.0):
    """uint8 GPU tensor [H, W, 3]: save_frame_compare_img's image of the ground truth `gt` and the predictions `preds` (float GPU tensors
    [T, c, h, w] in [lo, hi]). One launch."""
    src = _stack([gt] + list(preds), lo, hi, "compose_sheet")[0]
    S, T, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[3]), int(src.shape[4])
    tiles, canvas_shape = sheet_tiles(S, T, (h, w), int(context_frames), vis_context_frame_idx)
    return ops.vis_compose(src, tiles, canvas_shape, lo, hi, background=SHEET_BACKGROUND)[0]


def _pil():
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("importing from PIL failed -> please install pillow; it writes the gif and png visualizations.")
    return Image


def write_gif(out_fp, frames, frame_ms=GIF_FRAME_MS):
    """Writes uint8 frames [T, H, W, 3] as an animated GIF that loops, frame_ms per frame."""
    Image = _pil()
    frames = np.ascontiguousarray(frames.cpu().numpy() if torch.is_tensor(frames) else frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError(f"write_gif: frames are uint8 [T, H, W, 3] (got {frames.dtype} {frames.shape})")
    images = [Image.fromarray(f, "RGB") for f in frames]
    images[0].save(str(out_fp), format="GIF", save_all=True, append_images=images[1:], duration=int(frame_ms), loop=0, optimize=False)


def write_png(out_fp, image):
    """Writes a uint8 image [H, W, 3] as a PNG."""
    Image = _pil()
    image = np.ascontiguousarray(image.cpu().numpy() if torch.is_tensor(image) else image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"write_png: the image is uint8 [H, W, 3] (got {image.dtype} {image.shape})")
    Image.fromarray(image, "RGB").save(str(out_fp), format="PNG")


def save_vid_vis(out_fp: str, context_frames: int, mode: str = "gif", value_range=(0.0, 1.0), **trajs):
    """Writes the videos `trajs` side by side, each inside a border that tells given from predicted frames (the keyword is the
    sequence's name: it picks the colours, see border_colors). trajs: float GPU tensors [T, c, h, w] in value_range, or postprocessed
    uint8 arrays [T, h, w, c]; None entries are left out. mode "gif" only. Returns the composed frames (uint8 [T, H, W, 3], host)."""
    if mode != "gif":
        raise NotImplementedError(f"vis mode '{mode}': this build has no video encoder -> use the gif-mode for visualization")
    _pil()   # (before any GPU work)
    trajs = {k: v for k, v in trajs.items() if v is not None}
    src, lo, hi = _stack(trajs.values(), value_range[0], value_range[1], "save_vid_vis")
    frames = compose_video(src, context_frames, list(trajs), lo, hi).cpu().numpy()
    write_gif(out_fp, frames)
    return frames


def save_frame_compare_img(out_filename: str, context_frames: int, ground_truth_vis, preds_vis, vis_context_frame_idx, value_range=(0.0, 1.0)):
    """Writes the comparison image as a PNG: the ground truth in the first row (of its context frames only those of
    vis_context_frame_idx), each prediction's predicted frames in a row below. Sequences as in save_vid_vis. Returns the image."""
    _pil()
    src, lo, hi = _stack([ground_truth_vis] + list(preds_vis), value_range[0], value_range[1], "save_frame_compare_img")
    image = compose_sheet(src[0], list(src[1:]), context_frames, vis_context_frame_idx, lo, hi).cpu().numpy()
    write_png(out_filename, image)
    return image


def _model_and_adapters(entry):
    """(model, preprocessing, postprocessing) of a bare model or of a tuple that starts with these three (VPSuite's model lists)."""
    if isinstance(entry, (tuple, list)):
        return entry[0], entry[1], entry[2]
    return entry, None, None


def get_vis_from_model(dataset, data, model, data_unpack_config: dict, pred_frames: int, preprocessing=None, postprocessing=None):
    """(ground truth, context frames + prediction): two float GPU tensors [T, c, h, w] in the dataset's value range, from ONE forward of
    `model` under no_grad on the datapoint `data`. The model's eval / train mode is restored afterwards."""
    was_training = model.training
    model.eval()
    try:
        inp, target, actions = model.unpack_data(data, data_unpack_config)
        full = inp.clone() if model.NEEDS_COMPLETE_INPUT else torch.cat([inp, target], dim=1)
        model_inp = inp if preprocessing is None else preprocessing(inp)
        with torch.no_grad():
            if model.CAN_HANDLE_ACTIONS and model.config["action_conditional"]:
                pred, _ = model(model_inp, pred_frames=pred_frames, actions=actions)
            else:
                pred, _ = model(model_inp, pred_frames=pred_frames)
        pred = pred if postprocessing is None else postprocessing(pred)   # [1, T_pred, c, h, w]
        if model.NEEDS_COMPLETE_INPUT:   # the predicted frames take the place of the input's last ones
            input_and_pred = full.clone()
            input_and_pred[:, -pred.shape[1]:] = pred
        else:
            input_and_pred = torch.cat([inp, pred], dim=1)
    finally:
        model.train(was_training)
    return full.squeeze(dim=0).detach(), input_and_pred.squeeze(dim=0).detach()


def _check_vis_idx(dataset, vis_idx):
    if vis_idx is None or any([x >= len(dataset) for x in vis_idx]):
        raise ValueError(f"invalid vis_idx provided for visualization "
                         f"(dataset len = {len(dataset)}): {vis_idx}")


def _value_range(dataset):
    return float(dataset.value_range_min), float(dataset.value_range_max)


def visualize_vid(dataset, context_frames: int, pred_frames: int, model, device: str, out_path: Path, vis_idx, vis_mode: str):
    """Saves vis_<i>.<vis_mode> for the datapoints vis_idx of `dataset`: ground truth and the model's prediction side by side."""
    data_unpack_config = {"device": device, "context_frames": context_frames, "pred_frames": pred_frames}
    _check_vis_idx(dataset, vis_idx)
    model, pre, post = _model_and_adapters(model)
    for i, n in enumerate(vis_idx):
        input_vis, pred_vis = get_vis_from_model(dataset, dataset[n], model, data_unpack_config, pred_frames, pre, post)
        save_vid_vis(out_fp=str(Path(out_path) / f"vis_{i}.{vis_mode}"), context_frames=context_frames, mode=vis_mode,
                     value_range=_value_range(dataset), GT=input_vis, Pred=pred_vis)


def visualize_sequences(dataset, context_frames, pred_frames, models, device, out_path, vis_idx, vis_context_frame_idx, vis_vid_mode):
    """For every datapoint of vis_idx: vis_<i>_model_<j>.<vis_vid_mode> per model that has a model_dir (baselines such as CopyLastFrame
    have none and are left out), and, if vis_context_frame_idx is given, the comparison image vis_<i>.png of all of them against the
    ground truth; vis_info.txt says what is shown. One forward per (datapoint, model)."""
    out_path = Path(out_path)
    data_unpack_config = {"device": device, "context_frames": context_frames, "pred_frames": pred_frames}
    info_file_lines = [f"DATASET: {dataset.NAME}", f"chosen dataset idx: {vis_idx}",
                       f"Displayed context frames: {list(range(context_frames))}, ({vis_context_frame_idx} in seq_img)",
                       f"Displayed pred frames: {list(range(context_frames, context_frames + pred_frames))}",
                       "Displayed rows (from top):", " - Ground Truth"]
    _check_vis_idx(dataset, vis_idx)
    value_range = _value_range(dataset)
    for i, n in enumerate(vis_idx):
        data = dataset[n]
        ground_truth_vis, preds_vis = None, []
        for j, entry in enumerate(models):
            model, pre, post = _model_and_adapters(entry)
            if model.model_dir is None:
                continue
            input_vis, pred_vis = get_vis_from_model(dataset, data, model, data_unpack_config, pred_frames, pre, post)
            if ground_truth_vis is None:
                ground_truth_vis = input_vis
            preds_vis.append(pred_vis)
            save_vid_vis(out_fp=str(out_path / f"vis_{i}_model_{j}.{vis_vid_mode}"), context_frames=context_frames, mode=vis_vid_mode,
                         value_range=value_range, GT=input_vis, Pred=pred_vis)
            if i == 0:
                info_file_lines.append(f" - model {j}: {model.NAME} (model dir: {model.model_dir})")
        if vis_context_frame_idx is not None:
            if ground_truth_vis is None:   # no model with a model_dir: the ground truth alone
                frames = data["frames"].to(device)
                ground_truth_vis = frames[:context_frames + pred_frames].detach()
            save_frame_compare_img(str((out_path / f"vis_{i}.png").resolve()), context_frames, ground_truth_vis, preds_vis,
                                   vis_context_frame_idx, value_range=value_range)
        info_file_lines.append(f"vis {i} (idx {n}) origin: {data['origin']}")
    with open(str((out_path / "vis_info.txt").resolve()), "w") as vis_info_file:
        vis_info_file.writelines(line + "\n" for line in info_file_lines)
