"""Template track: the subject lock without a mask (beyond the reference, off by default).

The subject lock needs a segmentation mask per frame.  This estimator needs what an editor's "track motion" asks for: one
rectangle around the subject in one frame.  The box's content in frame `track_key` is the template; one device pass,
`native.Context.track_template_batch` (csrc/vstab_track.hip; include/vstab_track.h states the rule), follows it through the
clip by an exhaustive zero-mean SSD search in a window around the previous position, in exact integers, forwards and
backwards from the key frame, with no host round trip between frames.  Everything here is host arithmetic in float64 on what
the pass returns per frame -- position, best cost and the 3 x 3 costs around it (NumPy, no GPU): a parabola per axis refines
the position, 1 - sqrt(J_best / J_T) is the confidence, frames below LOST are interpolated as the subject lock interpolates
frames without a subject, and `subject_lock.transition_table` turns the centres into the transitions the pipeline expects.

DEFAULT_RADIUS = 24 working pixels and LOST = 0.3 are choices, not calibrations.  Out of scope: scale and rotation (one scale
is searched: translation only), template update, re-detection after loss, several subjects, the sharded path.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import native
from . import subject_lock

ESTIMATOR = "track"
DEFAULT_RADIUS = 24
LOST = 0.3
SENTINEL = native.TRACK_SENTINEL


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_request(track_box, track_key, track_radius, estimator: str, transform_mode: str) -> Optional[Tuple[Tuple[int, int, int, int], int, int]]:
    """The checks of a track request that need neither the clip nor a GPU -> (box, key, radius), or None where the estimator
    is another one.  track_box and estimator="track" go together; track_key and track_radius are read with them only."""
    if estimator != ESTIMATOR:
        for name, value, default in (("track_box", track_box, None), ("track_key", track_key, 0), ("track_radius", track_radius, None)):
            if value is not default and not (_is_int(value) and value == default):
                raise ValueError(f"{name}={value!r} needs estimator={ESTIMATOR!r}, got estimator={estimator!r}: the other estimators "
                                 "follow no box.")
        return None
    if track_box is None:
        raise ValueError(f"estimator={ESTIMATOR!r} needs track_box: (x, y, width, height) around the subject in frame track_key, "
                         "in full-resolution pixels.")
    if isinstance(track_box, (str, bytes)) or not hasattr(track_box, "__len__") or len(track_box) != 4 or not all(_is_int(v) for v in track_box):
        raise ValueError(f"track_box={track_box!r} is not (x, y, width, height), four integers in full-resolution pixels")
    box = tuple(int(v) for v in track_box)
    if box[0] < 0 or box[1] < 0 or box[2] < 1 or box[3] < 1:
        raise ValueError(f"track_box={box!r}: x and y must be >= 0, width and height >= 1")
    if not _is_int(track_key) or track_key < 0:
        raise ValueError(f"track_key={track_key!r} is not a frame index (an integer >= 0)")
    if track_radius is None:
        radius = DEFAULT_RADIUS
    elif not _is_int(track_radius) or not 1 <= track_radius <= native.TRACK_RADIUS_MAX:
        raise ValueError(f"track_radius={track_radius!r} is not None or an integer in 1..{native.TRACK_RADIUS_MAX} (working pixels)")
    else:
        radius = int(track_radius)
    if transform_mode != "translation":
        raise ValueError(f"transform_mode={transform_mode!r} is not supported with estimator 'track': the template is searched at "
                         "one scale and one orientation, which determines a translation.  Use 'translation'.")
    return box, int(track_key), radius


# what a track call cannot be combined with: (keyword, reason), refused in this order
_REFUSALS = (
    ("scene_cuts", "the box names one shot, and the template is not searched across a cut."),
    ("estimation_mask", "there is no camera-motion fit to keep a subject out of."),
    ("mesh_warp", "the track yields one position per frame: it has no dense grid of flow samples."),
    ("temporal_fill", "fill candidates register the background through the transitions, and these transitions are the subject's."),
    ("sharpness_transfer", "its transitions are the subject's, not the camera's, so they do not register a neighbour's background."),
    ("rolling_shutter", "its transitions are the subject's, not the camera's, and the readout shears with the camera's velocity."),
    ("drift_correction", "its transitions follow the subject, while the keyframe alignment registers whole estimation images."),
    ("deflicker", "its transitions register the subject, not the scene, so the pixels the measurement compares would not show the "
                  "same scene point."),
    ("horizon_level", "the chain of transitions is the subject's path, not the camera's roll."),
    ("plate_fill", "the frames are then registered on the subject, and the plate would be of the subject."),
)


def check_pipeline(requested: Dict[str, Any]) -> None:
    """requested: {keyword: its checked request, None / 0 / False where it is off}.  The first of _REFUSALS that is on raises."""
    for name, reason in _REFUSALS:
        value = requested.get(name)
        if value is None or value is False or (isinstance(value, int) and value == 0):
            continue
        raise ValueError(f"{name} is not supported with estimator 'track': {reason}")


def working_box(box, size, working_size) -> Tuple[int, int, int, int]:
    """The full-resolution box in working pixels: floor(v * working / full) per value, width and height at least 1.  A box
    below native.TRACK_MIN_BOX working pixels on an axis raises."""
    (W, H), (w, h) = (int(size[0]), int(size[1])), (int(working_size[0]), int(working_size[1]))
    x, y, bw, bh = box
    out = (x * w // W, y * h // H, max(bw * w // W, 1), max(bh * h // H, 1))
    for name, full, work in (("width", bw, out[2]), ("height", bh, out[3])):
        if work < native.TRACK_MIN_BOX:
            raise ValueError(f"track_box={tuple(box)!r}: its {name} of {full} px is {work} working pixels (estimation images of "
                             f"{w} x {h}), the minimum is {native.TRACK_MIN_BOX}")
    return out


def stride_of(bw: int, bh: int) -> int:
    return -(-max(int(bw), int(bh)) // 64)


def check_against_clip(box, key: int, total_frames: int, size) -> None:
    """The checks that need the clip: the key frame exists and the box lies inside it."""
    if key >= total_frames:
        raise ValueError(f"track_key={key} outside a clip of {total_frames} frames")
    x, y, bw, bh = box
    if x + bw > int(size[0]) or y + bh > int(size[1]):
        raise ValueError(f"track_box={tuple(box)!r} leaves the {int(size[0])} x {int(size[1])} frame")


def template_energy(tsums) -> int:
    """J_T = n * sum T^2 - (sum T)^2 as a Python int."""
    n, st, st2 = (int(v) for v in np.asarray(tsums).reshape(3))
    return n * st2 - st * st


def subpixel(near) -> np.ndarray:
    """near uint64 [N,9] -> float64 [N,2] = (dx, dy) of the parabola through the three costs of each axis:
    (J- - J+) / (2 (J- - 2 J0 + J+)), clipped to +-0.5; 0 where a neighbour is the sentinel or the denominator is not positive."""
    near = np.asarray(near).astype(np.uint64).reshape(-1, 9)
    out = np.zeros((near.shape[0], 2), np.float64)
    for axis, (lo, hi) in enumerate(((3, 5), (1, 7))):
        bad = (near[:, lo] == SENTINEL) | (near[:, hi] == SENTINEL) | (near[:, 4] == SENTINEL)
        jm, j0, jp = (np.where(bad, 0.0, near[:, i].astype(np.float64)) for i in (lo, 4, hi))
        den = jm - 2.0 * j0 + jp
        ok = ~bad & (den > 0.0)
        out[:, axis] = np.where(ok, np.clip((jm - jp) / (2.0 * np.where(ok, den, 1.0)), -0.5, 0.5), 0.0)
    return out


def confidence(best, energy: int) -> np.ndarray:
    """clip(1 - sqrt(J_best / J_T), 0, 1); 0 for a sentinel best."""
    best = np.asarray(best).astype(np.uint64).reshape(-1)
    sentinel = best == SENTINEL
    ratio = np.where(sentinel, 1.0, best.astype(np.float64)) / float(energy)
    return np.where(sentinel, 0.0, np.clip(1.0 - np.sqrt(ratio), 0.0, 1.0))


def centres(pos, delta, wbox, size, working_size, lost) -> np.ndarray:
    """The box's centre in full-resolution pixel coordinates, float64 [N,2]: (pos + delta + (b - 1) / 2) * full / working; a
    lost frame takes the linear interpolation, in frame index, between the nearest frames that are not (held at the ends), as
    subject_lock.centroids does for frames without a subject."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    lost = np.asarray(lost, dtype=bool).reshape(-1)
    half = np.array([(wbox[2] - 1) / 2.0, (wbox[3] - 1) / 2.0])
    scale = np.array([size[0] / float(working_size[0]), size[1] / float(working_size[1])])
    c = (pos + np.asarray(delta, dtype=np.float64) + half) * scale
    idx = np.arange(c.shape[0], dtype=np.float64)
    known = idx[~lost]
    return np.stack([np.interp(idx, known, c[~lost, 0]), np.interp(idx, known, c[~lost, 1])], axis=1)


def solve(tsums, pos, best, near, box, key: int, radius: int, wbox, size, working_size) -> Tuple[np.ndarray, Dict[str, Any]]:
    """What the device pass returned (host arrays) -> (candidate fits [N-1,3], meta["template_track"])."""
    energy = template_energy(tsums)
    if energy == 0:
        raise ValueError(f"track_box={tuple(box)!r} in frame {key}: the box holds no texture (its samples are all equal), so "
                         "there is nothing to follow.")
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 2)
    n = pos.shape[0]
    conf = confidence(best, energy)
    lost = conf < LOST                  # (never the key frame: its best is 0)
    c = centres(pos, subpixel(near), wbox, size, working_size, lost)
    table = subject_lock.transition_table(c, np.ones(n), ~lost, size, working_size)
    follows = np.arange(n) + np.sign(key - np.arange(n))       # the frame each frame starts from; the key frame itself
    step = np.abs(pos - pos[follows])
    block = {
        "version": 1,
        "box": [int(v) for v in box],
        "key": int(key),
        "radius": int(radius),
        "stride": stride_of(wbox[2], wbox[3]),
        "samples": int(np.asarray(tsums).reshape(3)[0]),
        "position": c.tolist(),
        "confidence": conf.tolist(),
        "lost": np.nonzero(lost)[0].tolist(),
        "frames_at_window_edge": int((step.max(axis=1) == radius).sum()),
    }
    return table, block


def estimate_on_device(ctx, gray, request, size, working_size) -> Tuple[np.ndarray, Dict[str, Any]]:
    """gray u8 [N,h,w] on the device (the estimator's own images), request = (box, key, radius) -> (candidate fits [N-1,3],
    meta["template_track"]).  One call into the library, one download of 92 bytes per frame."""
    box, key, radius = request
    work = (int(gray.shape[2]), int(gray.shape[1]))
    wbox = working_box(box, size, work)
    tsums, pos, best, near, _ = ctx.track_template_batch(gray, wbox, stride_of(wbox[2], wbox[3]), radius, key)
    host = [t.cpu().numpy() for t in (tsums, pos, best, near)]
    return solve(host[0], host[1], host[2].view(np.uint64), host[3].view(np.uint64), box, key, radius, wbox, size, work)
