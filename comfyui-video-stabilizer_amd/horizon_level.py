"""Horizon level: every shot is rolled so that its vertical and horizontal structure stands upright (Gyroflow's horizon lock,
from the picture instead of a gyro).

The device side is one pass, `native.Context.orientation_hist_batch` (csrc/vstab_level.hip; include/vstab.h states the rule
"vstab_orientation_hist_batch"): per estimation image the histogram of Scharr gradient orientations, folded modulo 90 degrees
and weighted by the squared gradient, as exact integers.  This module is the host side, all float64: the checks of a request,
the roll a histogram stands for, the roll of every frame relative to its shot's first frame from the chain of transitions,
the one slowly varying offset per shot that the picture content has to supply, and the levelling matrices.  Nothing here
needs a GPU.  Angles are in degrees throughout; positive is the rotation of the point matrix [[c, -s], [s, c]] in pixel
coordinates (x right, y down).

The levelling only changes each frame's final matrix (L_i @ F_i, a rotation about the canvas centre), in front of the mesh
warp's offsets and the dynamic zoom, so everything behind the plan follows by itself, as it does for the zoom.  For
`crop_and_pad` framing and translation / similarity.  Out of scope: rolls beyond 45 degrees (image structure gives the roll
modulo 90 only), perspective mode, `crop` and `expand` framing, rolling_shutter, the subject and sharded paths, the device
plan, line or vanishing-point detection, pitch and yaw, gyro data, a per-pixel mask for the histogram.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from .dynamic_zoom import _is_number, radius_frames

VERSION = 1
K = 256                          # VSTAB_ORIENTATION_K (include/vstab.h): bins -K .. K, bin k stands for atan(k / K)
# Both are choices, not calibrations.  They have been tried on synthetic material only (tests/horizon_level_restatement.py:
# rectangles with smooth edges, a horizon and weak sinusoids): there the confidence of a frame with structure is 0.6-0.8, of
# one with sinusoids of amplitude 0.02 on top 0.3-0.45, of sinusoids alone at most 0.05 -- 0.25 lies between the last two.
# 65536 is a Scharr gradient of 256, a step of 16 grey levels across a straight edge.
MIN_CONFIDENCE = 0.25            # a frame's roll counts only with at least this share of the mass within 1 degree of it
MIN_MAG2 = 65536                 # the histogram's min_mag2
DEFAULT_LIMIT_DEG = 20.0         # horizon_limit=None
LIMIT_MAX_DEG = 45.0             # exclusive: the roll is known modulo 90 degrees
WINDOW_MAX_S = 60.0
GRID_DEG = 0.25                  # the score's grid over the period
WINDOW_DEG = 1.0                 # half-width of the score's triangular window, and of the confidence
SHIFT_RADII_DEG = (1.0, 1.0, 0.5, 0.5, 0.5)   # the mean-shift steps behind the best grid point
MIN_MEASURED = 3                 # a shot with fewer measured frames than max(this, 10 %) is not observable

_FRAMING_LIMITS = {
    "crop": "the crop solver has already bounded the matrices it was given; a rotation behind it would uncover padding.",
    "expand": "an expand canvas is fixed by the plan's matrices; a rotation behind it would leave the canvas.",
}


@dataclass
class Request:
    """A checked horizon_level request.  window_s None: one offset per shot."""

    window_s: Optional[float]
    limit_deg: float


def check_request(horizon_level, horizon_limit=None) -> Optional[Request]:
    """The checks that need neither the clip nor a GPU.  horizon_level: None -> None (the feature is off), True -> one offset
    per shot, a finite number in (0, 60] -> the window in seconds over which the offset may vary.  horizon_limit: None ->
    DEFAULT_LIMIT_DEG, else a finite number in (0, 45); without horizon_level it is an error."""
    if horizon_level is None:
        if horizon_limit is not None:
            raise ValueError(f"horizon_limit={horizon_limit!r} needs horizon_level: without a levelling there is no correction to limit.")
        return None
    if horizon_level is True:
        window = None
    else:
        if not _is_number(horizon_level) or not np.isfinite(horizon_level) or not 0.0 < horizon_level <= WINDOW_MAX_S:
            raise ValueError(f"horizon_level={horizon_level!r}: expected None, True or a finite window in seconds in (0, {WINDOW_MAX_S:g}]")
        window = float(horizon_level)
    limit = DEFAULT_LIMIT_DEG
    if horizon_limit is not None:
        if not _is_number(horizon_limit) or not np.isfinite(horizon_limit) or not 0.0 < horizon_limit < LIMIT_MAX_DEG:
            raise ValueError(f"horizon_limit={horizon_limit!r}: expected None or a finite number of degrees in (0, {LIMIT_MAX_DEG:g})")
        limit = float(horizon_limit)
    return Request(window, limit)


def check_pipeline(framing_mode: str, transform_mode: str, estimator: str, rolling=None) -> None:
    """What the levelling does not go with, each with its reason."""
    if framing_mode in _FRAMING_LIMITS:
        raise ValueError(f"horizon_level is not supported with framing_mode {framing_mode!r}: {_FRAMING_LIMITS[framing_mode]} "
                         "Use framing_mode 'crop_and_pad'.")
    if transform_mode == "perspective":
        raise ValueError("horizon_level is not supported with transform_mode 'perspective': a homography has no single roll. "
                         "Use 'translation' or 'similarity'.")
    if estimator == "subject":
        raise ValueError("horizon_level is not supported with estimator 'subject': the subject lock never makes the estimation "
                         "images the roll is measured on.")
    if rolling is not None:
        raise ValueError(f"horizon_level is not supported with rolling_shutter={rolling!r}: the two have not been tried together.")


def wrap90(deg):
    """deg modulo 90 into [-45, 45)."""
    return np.mod(np.asarray(deg, dtype=np.float64) + 45.0, 90.0) - 45.0


def bin_angles() -> np.ndarray:
    """The orientation each of the 2K + 1 bins stands for, degrees: atan(k / K), k = -K .. K."""
    return np.degrees(np.arctan(np.arange(-K, K + 1, dtype=np.float64) / K))


@lru_cache(maxsize=1)
def _score_window() -> Tuple[np.ndarray, np.ndarray]:
    """(grid [G] = -45 + GRID_DEG * i over one period, weights [2K+1, G]: the triangular window of every grid point at every
    bin, over the circle of 90 degrees)."""
    grid = -45.0 + GRID_DEG * np.arange(int(round(90.0 / GRID_DEG)), dtype=np.float64)
    dist = np.abs(wrap90(bin_angles()[:, None] - grid[None, :]))
    return grid, np.maximum(0.0, 1.0 - dist / WINDOW_DEG)


def frame_roll(hist) -> Tuple[Optional[float], float]:
    """One histogram (2K + 1 non-negative masses) -> (roll in degrees in [-45, 45) or None, confidence in [0, 1]).  The score
    of a grid point is the mass under a triangular window of half-width WINDOW_DEG; from the best grid point (the first of
    equals) five mass-weighted mean-shift steps with the radii SHIFT_RADII_DEG; the confidence is the mass within WINDOW_DEG of
    the result over the total mass.  Everything lives on the circle of 90 degrees: bins -K and +K are one orientation.  An
    empty histogram gives (None, 0.0)."""
    mass = np.asarray(hist, dtype=np.float64).reshape(-1)
    if mass.shape[0] != 2 * K + 1:
        raise ValueError(f"frame_roll: a histogram of {mass.shape[0]} bins, expected {2 * K + 1}")
    total = mass.sum()
    if not total > 0.0:
        return None, 0.0
    grid, weights = _score_window()
    centre = float(grid[int(np.argmax(mass @ weights))])
    angles = bin_angles()
    for radius in SHIFT_RADII_DEG:
        d = wrap90(angles - centre)
        near = np.abs(d) <= radius
        m = mass[near].sum()
        if not m > 0.0:
            break
        centre = float(wrap90(centre + (mass[near] * d[near]).sum() / m))
    near = np.abs(wrap90(angles - centre)) <= WINDOW_DEG
    return centre, float(mass[near].sum() / total)


def frame_rolls(hist) -> Tuple[np.ndarray, np.ndarray]:
    """frame_roll of every row of hist [N, 2K+1] -> (roll f64 [N], NaN where there is none; confidence f64 [N])."""
    hist = np.asarray(hist)
    roll, conf = np.full(hist.shape[0], np.nan), np.zeros(hist.shape[0])
    for i, row in enumerate(hist):
        r, conf[i] = frame_roll(row)
        if r is not None:
            roll[i] = r
    return roll, conf


def _segments(segments, n: int):
    return [(int(s), int(e)) for s, e in segments] if segments is not None else [(0, n)]


def chain_roll(transitions, segments=None, confidences=None) -> np.ndarray:
    """r_i, degrees [N]: the roll of frame i relative to its shot's first frame, atan2(C_i[1, 0], C_i[0, 0]) of the
    full-resolution transitions [N-1, 3, 3] composed from that frame on (C_s = 1, C_{i+1} = T_i @ C_i, float64).  A pair with
    confidence 0 contributes the identity.  Translation transitions have no rotation, so r is 0 for them."""
    T = np.asarray(transitions, dtype=np.float64).reshape(-1, 3, 3)
    n = T.shape[0] + 1
    conf = np.ones(n - 1) if confidences is None else np.asarray(confidences, dtype=np.float64).reshape(-1)
    r = np.zeros(n, np.float64)
    for s, e in _segments(segments, n):
        C = np.eye(3)
        for i in range(s + 1, e):
            if conf[i - 1] > 0.0:
                C = T[i - 1] @ C
            r[i] = np.degrees(np.arctan2(C[1, 0], C[0, 0]))
    return r


def _circular_median(e: np.ndarray) -> float:
    """The sample (the first of equals) with the smallest sum of distances to the others on the circle of 90 degrees."""
    cost = np.abs(wrap90(e[:, None] - e[None, :])).sum(axis=1)
    return float(e[int(np.argmin(cost))])


def offsets(roll, confidence, r, request: Request, fps: float, segments=None) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (beta f64 [N], degrees, NaN through a shot that is not observable;  measured bool [N];  shots not observable).
    beta is what the picture content adds to the chain: the roll of the shot's first frame, as far as frame i knows it.  Per
    shot, over the frames with a roll and confidence >= MIN_CONFIDENCE: e_i = wrap90(roll_i - r_i), unwrapped about the shot's
    circular median.  window_s None: the median of the shot.  Else with R = radius_frames(window_s, fps): the median over the
    measured frames within R of frame i, frames without one interpolated linearly (ends held), then the box mean over
    [i - R, i + R], indices clamped to the shot.  A shot with fewer measured frames than max(MIN_MEASURED, 10 %) gets none."""
    roll = np.asarray(roll, dtype=np.float64).reshape(-1)
    conf = np.asarray(confidence, dtype=np.float64).reshape(-1)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    n = roll.shape[0]
    measured = np.isfinite(roll) & (conf >= MIN_CONFIDENCE)
    beta = np.full(n, np.nan)
    not_observable = 0
    radius = None if request.window_s is None else radius_frames(request.window_s, fps)
    for s, e in _segments(segments, n):
        if e <= s:
            continue
        idx = np.flatnonzero(measured[s:e])
        if idx.size < max(MIN_MEASURED, int(np.ceil(0.1 * (e - s)))):
            not_observable += 1
            continue
        err = wrap90(roll[s:e][idx] - r[s:e][idx])
        mid = _circular_median(err)
        err = mid + wrap90(err - mid)
        if radius is None:
            beta[s:e] = np.median(err)
            continue
        pos = np.arange(e - s)
        local = np.full(e - s, np.nan)
        for i in pos:
            near = np.abs(idx - i) <= radius
            if near.any():
                local[i] = np.median(err[near])
        have = np.isfinite(local)
        local = np.interp(pos, pos[have], local[have])
        window = np.clip(pos[:, None] + np.arange(-radius, radius + 1)[None, :], 0, e - s - 1)
        beta[s:e] = local[window].sum(axis=1) / np.float64(2 * radius + 1)
    return beta, measured, not_observable


def level_matrices(beta, r, final_matrices, out_size, limit: float) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (L float32 [N,3,3], the correction a f64 [N] in degrees, frames whose correction the limit cut).
    The output of frame i shows the content at beta_i + r_i + the rotation of its final matrix F_i; a_i is minus that, modulo
    90 into [-45, 45), clamped to +-limit; 0 where beta is NaN.  L_i rotates by a_i about the canvas centre
    cx = (W-1)/2, cy = (H-1)/2: formed in float64, cast once.  Applied as np.matmul(L, final) in float32, like the zoom."""
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    F = np.asarray(final_matrices, dtype=np.float64).reshape(-1, 3, 3)
    own = np.degrees(np.arctan2(F[:, 1, 0], F[:, 0, 0]))
    a = -wrap90(np.where(np.isfinite(beta), beta, 0.0) + np.asarray(r, dtype=np.float64).reshape(-1) + own)
    a = np.where(np.isfinite(beta), a, 0.0)
    limited = int(np.count_nonzero(np.abs(a) > limit))
    a = np.clip(a, -float(limit), float(limit))
    cx, cy = (int(out_size[0]) - 1) / 2.0, (int(out_size[1]) - 1) / 2.0
    c, s = np.cos(np.radians(a)), np.sin(np.radians(a))
    m = np.zeros((a.shape[0], 3, 3), np.float64)
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = c, -s, cx - c * cx + s * cy
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = s, c, cy - s * cx - c * cy
    m[:, 2, 2] = 1.0
    return m.astype(np.float32), a, limited


def _listed(values, valid) -> list:
    return [float(v) if ok else None for v, ok in zip(values, valid)]


def plan_level(request: Request, hist, transitions, confidences, final_matrices, out_size, fps_effective: float,
               segments: Optional[Sequence[Tuple[int, int]]] = None):
    """Histograms [N, 2K+1] and the plan's own full-resolution transitions, confidences and final matrices -> (the levelling
    matrices float32 [N,3,3] or None where no frame is corrected, meta["horizon_level"])."""
    roll, conf = frame_rolls(hist)
    r = chain_roll(transitions, segments, confidences)
    beta, measured, not_observable = offsets(roll, conf, r, request, fps_effective, segments)
    L, a, limited = level_matrices(beta, r, final_matrices, out_size, request.limit_deg)
    block: Dict[str, Any] = {
        "version": VERSION,
        "window_s": None if request.window_s is None else float(request.window_s),
        "limit_deg": float(request.limit_deg),
        "min_confidence": MIN_CONFIDENCE,
        "roll_deg": _listed(roll, np.isfinite(roll)),
        "confidence": conf.tolist(),
        "frames_measured": int(np.count_nonzero(measured)),
        "shots_not_observable": int(not_observable),
        "offset_deg": _listed(beta, np.isfinite(beta)),
        "correction_deg": a.tolist(),
        "correction_deg_max": float(np.max(np.abs(a))) if a.size else 0.0,
        "frames_limited": int(limited),
    }
    return (L if np.any(a != 0.0) else None), block
