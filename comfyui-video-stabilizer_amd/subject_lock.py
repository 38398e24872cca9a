"""Subject lock: stabilize on a masked subject instead of the camera (beyond the reference, off by default).

Every other estimator of the package measures the camera.  This one takes a per-frame segmentation mask of a subject and
turns the subject's absolute position -- which a mask gives in every frame, with no drift -- into the per-pair transitions
the pipeline expects, so that trajectory, camera_lock, the framings, the warp, motion_meta and Motion Apply follow unchanged.
The device side is one pass, `native.Context.mask_moments_batch` (csrc/vstab_subject.hip; include/vstab.h states the rule
"vstab_mask_moments_batch"): count, coordinate sums and bounding box of the pixels with mask > 0.5, per frame, as exact
integers.  Everything here is host arithmetic in float64 on those 28 bytes per frame (NumPy, no GPU).
"""

from __future__ import annotations

from typing import Any, Dict, Tuple

import numpy as np

from . import native

ESTIMATOR = "subject"
TRANSFORM_MODES = ("translation", "similarity")


def check_request(subject_mask, transform_mode: str, estimator: str = ESTIMATOR, total_frames=None, size=None) -> bool:
    """The checks of a subject-lock request that need no GPU -> whether the estimator is the subject lock.
    subject_mask and estimator="subject" go together; transform_mode is "translation" or "similarity"; the mask is a float
    array or tensor [N,H,W].  With total_frames and size = (width, height) the shape is held against the clip as well."""
    if estimator != ESTIMATOR:
        if subject_mask is not None:
            raise ValueError(f"subject_mask needs estimator={ESTIMATOR!r}, got estimator={estimator!r}: the other estimators "
                             "measure the camera and have no use for a subject (estimation_mask keeps one out of their fit).")
        return False
    if subject_mask is None:
        raise ValueError(f"estimator={ESTIMATOR!r} needs subject_mask: a float mask [N,H,W] of the subject, one per frame.")
    if transform_mode == "perspective":
        raise ValueError("transform_mode='perspective' is not supported with estimator 'subject': a centroid and an area "
                         "determine no homography.  Use 'translation' or 'similarity'.")
    if transform_mode not in TRANSFORM_MODES:
        raise ValueError(f"transform_mode={transform_mode!r} is not supported with estimator 'subject': expected one of {TRANSFORM_MODES}.")
    if not (hasattr(subject_mask, "shape") and hasattr(subject_mask, "dtype")):
        raise ValueError(f"subject_mask must be a float array or tensor [N,H,W], got {type(subject_mask).__name__}")
    if "float" not in str(subject_mask.dtype):
        raise ValueError(f"subject_mask must be floating point (> 0.5 marks the subject), got dtype {subject_mask.dtype}")
    shape = tuple(int(v) for v in subject_mask.shape)
    if len(shape) != 3:
        raise ValueError(f"subject_mask of shape {shape} is not [N,H,W]: the subject lock needs one mask per frame"
                         + (" (one mask for the whole clip has no motion)" if len(shape) == 2 else ""))
    if total_frames is not None:
        width, height = size
        if shape[0] == 1 and total_frames != 1 and shape[1:] == (height, width):
            raise ValueError(f"subject_mask of shape {shape} holds one mask for a clip of {total_frames} frames: one mask has no "
                             f"motion, expected [{total_frames},{height},{width}]")
        if shape != (total_frames, height, width):
            raise ValueError(f"subject_mask of shape {shape} does not match the clip: expected [{total_frames},{height},{width}]")
    return True


def check_pipeline(temporal_fill: int = 0, scene_cuts=None, estimation_mask=None) -> None:
    """What a subject-lock call cannot be combined with, each with its reason.  scene_cuts: the caller's keyword, or a checked
    scene_cuts.Request."""
    if int(temporal_fill) > 0:
        raise ValueError(f"temporal_fill={int(temporal_fill)} is not supported with estimator 'subject': fill candidates register "
                         "the background through the transitions, and these transitions are the subject's.")
    if getattr(scene_cuts, "mode", scene_cuts) == "auto":
        raise ValueError("scene_cuts='auto' is not supported with estimator 'subject': the residual score is taken after the "
                         "pair's camera transition, which this estimator does not measure.  Pass the cuts as a list of frame indices.")
    if estimation_mask is not None:
        raise ValueError("estimation_mask is not supported with estimator 'subject': there is no camera-motion fit to keep a "
                         "subject out of.")


def centroids(sums, bbox, size) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The kernel's integers -> (c float64 [N,2] = (x, y), area float64 [N], measured bool [N]).
    c = (sum_x / count, sum_y / count) and area = count where the frame has a subject.  A frame without one takes the linear
    interpolation, in frame index, between the nearest frames that have one -- of the position and of log(area); in front of
    the first and behind the last such frame the value is held.  No frame with a subject: ValueError."""
    sums = np.asarray(sums, dtype=np.int64).reshape(-1, 3)
    bbox = np.asarray(bbox, dtype=np.int32).reshape(-1, 4)
    if sums.shape[0] != bbox.shape[0]:
        raise ValueError(f"subject lock: {sums.shape[0]} sums and {bbox.shape[0]} bounding boxes")
    n = sums.shape[0]
    count = sums[:, 0].astype(np.float64)
    measured = sums[:, 0] > 0
    if not measured.any():
        raise ValueError(f"subject_mask holds no subject pixel (> 0.5) in any of its {n} frames (frame size {tuple(size)}): "
                         "there is nothing to lock on.")
    idx = np.arange(n, dtype=np.float64)
    known = idx[measured]
    c = np.empty((n, 2), np.float64)
    c[:, 0] = np.interp(idx, known, sums[measured, 1].astype(np.float64) / count[measured])
    c[:, 1] = np.interp(idx, known, sums[measured, 2].astype(np.float64) / count[measured])
    area = np.exp(np.interp(idx, known, np.log(count[measured])))
    first, last = int(known[0]), int(known[-1])
    area[measured] = count[measured]      # (exp(log(x)) need not be x: measured and held values are the counts themselves)
    area[:first], area[last + 1:] = count[first], count[last]
    return c, area, measured


def transition_table(c, area, measured, size, working_size=None) -> np.ndarray:
    """-> the candidate fits [N-1,3] (native.FIT_DTYPE) at working resolution, as the other estimators report them:
    translation [[1,0,dx],[0,1,dy]] with d = (c[k+1] - c[k]) * working / full; similarity with s = sqrt(area[k+1] / area[k]),
    no rotation and t = c'[k+1] - s * c'[k] in working coordinates; perspective not computed.  Formed in float64, cast once.
    confidence = min(area) / max(area) of the pair where both frames were measured, 0.0 where one was interpolated (the
    transition is carried, but reported as not estimated); residual 0.0; valid_points = total_points = 1."""
    c = np.asarray(c, dtype=np.float64).reshape(-1, 2)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    measured = np.asarray(measured, dtype=bool).reshape(-1)
    pairs = max(c.shape[0] - 1, 0)
    work = size if working_size is None else working_size
    scale = np.array([work[0] / float(size[0]), work[1] / float(size[1])], np.float64)
    cw = c * scale
    table = np.zeros((pairs, 3), native.FIT_DTYPE)
    table["matrix"][:] = np.eye(3, dtype=np.float32).reshape(9)
    if pairs == 0:
        return table
    a0, a1 = area[:-1], area[1:]
    s = np.sqrt(a1 / a0)
    both = measured[:-1] & measured[1:]
    conf = np.where(both, np.minimum(a0, a1) / np.maximum(a0, a1), 0.0)
    mats = np.zeros((pairs, 2, 9), np.float64)
    mats[:, :, [0, 4, 8]] = 1.0
    mats[:, 0, [2, 5]] = cw[1:] - cw[:-1]
    mats[:, 1, 0] = mats[:, 1, 4] = s
    mats[:, 1, [2, 5]] = cw[1:] - s[:, None] * cw[:-1]
    for mi in (0, 1):
        rows = table[:, mi]
        rows["matrix"] = mats[:, mi].astype(np.float32)
        rows["confidence"] = conf
        rows["residual"] = 0.0
        rows["accepted"] = 1
        rows["computed"] = 1
        rows["valid_points"] = 1
        rows["total_points"] = 1
    return table


def meta_block(sums, bbox, c, measured, size) -> Dict[str, Any]:
    """meta["subject_lock"].  frames_touching_border: frames whose bounding box lies on row or column 0 or on the last one --
    the subject is clipped there and its centroid biased; reported, not corrected.  area_fraction_*: count / (W * H) over
    the frames that have a subject."""
    sums = np.asarray(sums, dtype=np.int64).reshape(-1, 3)
    bbox = np.asarray(bbox, dtype=np.int32).reshape(-1, 4)
    measured = np.asarray(measured, dtype=bool).reshape(-1)
    width, height = int(size[0]), int(size[1])
    touching = measured & ((bbox[:, 0] == 0) | (bbox[:, 1] == 0) | (bbox[:, 2] == width - 1) | (bbox[:, 3] == height - 1))
    fraction = sums[measured, 0].astype(np.float64) / float(width * height)
    return {
        "version": 1,
        "mask_frames": int(sums.shape[0]),
        "frames_without_subject": int((~measured).sum()),
        "frames_touching_border": int(touching.sum()),
        "area_fraction_min": float(fraction.min()),
        "area_fraction_mean": float(fraction.mean()),
        "area_fraction_max": float(fraction.max()),
        "centroid": np.asarray(c, dtype=np.float64).reshape(-1, 2).tolist(),
        "interpolated": np.nonzero(~measured)[0].tolist(),
    }


def mask_on_device(ctx, subject_mask):
    """The mask as a contiguous float32 [N,H,W] tensor on the context's device (a float32 host tensor goes through the
    pinned ring)."""
    torch = ctx.torch
    mask = subject_mask if isinstance(subject_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subject_mask, dtype=np.float32))
    if mask.device.type == "cpu" and mask.dtype == torch.float32:
        return ctx.upload(mask.contiguous())
    return mask.to(device=ctx.device, dtype=torch.float32).contiguous()


def estimate_on_device(ctx, mask_dev, size, working_size) -> Tuple[np.ndarray, Dict[str, Any]]:
    """One launch over the mask clip, a download of 28 bytes per frame -> (candidate fits [N-1,3], meta["subject_lock"])."""
    sums, bbox = ctx.mask_moments_batch(mask_dev)
    sums, bbox = sums.cpu().numpy(), bbox.cpu().numpy()
    c, area, measured = centroids(sums, bbox, size)
    return transition_table(c, area, measured, size, working_size), meta_block(sums, bbox, c, measured, size)
