"""Rolling shutter: the parametric correction of a row-by-row readout in the Flow warp (what Warp Stabilizer, Resolve and
Gyroflow call rolling-shutter repair).

A sensor that is read out row by row over the fraction `rho` of the frame interval (the readout; its sign says top to bottom
or bottom to top) shows a point that a global shutter would show at q at

    s = q + tau(s_y) * v(q),    tau(y) = rho * (y / (H - 1) - 1/2)   in frame intervals,

v(q) = V (q_x, q_y, 1) the image velocity in px per frame, a 2x3 V per frame.  The equation is linear in s_y:
tau = rho * (q_y / (H - 1) - 1/2) / (1 - rho * v_y / (H - 1)).  Once the global motion is taken out, that is the artefact
which remains: verticals lean left and right in time with the shake.

The device side: `native.Context.rolling_warp_batch` (csrc/vstab_rolling.hip) is the plain warp that samples the source at s
instead of q, `native.Context.row_residual_batch` reduces the stride-8 flow grid a Flow run already has to one residual per
grid row and pair (include/vstab.h states both rules).  This module is the host side: the checks of a request, the per-frame
velocities from the transitions, the least-squares estimate of the one physical unknown rho from the row residuals, and the
meta block.  All float64, pure functions; nothing here needs a GPU.

The round trip: `parse_block` reads the block back for Motion Apply (`apply_motion(rolling=True)`), which applies the row
correction again on the run's source frames (`rolling_warp_batch`) or undoes it on the stabilized ones
(`native.Context.rolling_unwarp_batch`, the closed-form inverse: tau is known from the output row).

The refit (`rolling_refit=True`): the warp corrects rows, but the pair transitions in front of it were fitted on samples that
the readout had sheared, and a similarity fit takes part of that shear for rotation and scale.  One pass between the first
plan and the final one rectifies both ends of every flow sample with the first pass's own per-frame velocities, at working
resolution (`native.Context.rectify_samples_batch`: the inverse's closed form at a point), fits the pairs again on them
(`native.Context.points_fit_batch`, unchanged) and forms the plan again; the warp's velocities and the meta's come from that
second plan.  `check_refit_request` and `refit_block` are its host side.

Out of scope: perspective mode, `crop` framing and dynamic zoom, the mesh, temporal-fill, sharpness-transfer, subject and
sharded paths, bicubic and motion-blur warps, a per-row homography mixture, readout tables per camera model; for the refit
also a second readout estimate from the rectified residuals (which would drop the `f_k` factor), Classic's tracked corners,
the images that drift correction registers, `plan_kernel`.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Union

import numpy as np

VERSION = 1
AUTO = "auto"
# Both are choices, not calibrations: they have been tried on synthetic material only -- analytic rolling flows over a
# procedural texture, no footage.
ROW_MIN_SAMPLES = 8        # VSTAB_ROW_MIN_SAMPLES (include/vstab.h): admitted samples a grid row needs for its median to count
ROW_MIN_RMS_PX = 0.05      # RMS of the predicted row signal below which the readout is not observable (working px)
D_MIN = 0.5                # the warp's clamp of 1 - rho * v_y / (H - 1) (the rule in include/vstab.h)

_ESTIMATOR_LIMITS = {
    "classic": "the Classic estimator tracks sparse corners: it has no grid of flow samples to estimate the readout from.",
    "flow_phase_correlate": "phase correlation yields one global shift per pair: it has no grid of flow samples to estimate the readout from.",
}


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def check_request(value) -> Union[None, str, float]:
    """The checks that need neither the clip nor a GPU.  None or 0 -> None (the feature is off); "auto" -> "auto" (the readout
    is estimated); a finite number in [-1, 1] -> that readout as a float.  Anything else, a bool included, is a ValueError."""
    if value is None:
        return None
    if isinstance(value, str) and value == AUTO:
        return AUTO
    if not _is_number(value) or not np.isfinite(value) or not -1.0 <= value <= 1.0:
        raise ValueError(f"rolling_shutter={value!r}: expected None, 0, 'auto' or a finite readout in [-1, 1] "
                         "(a fraction of the frame interval; negative: bottom to top)")
    return float(value) if value != 0 else None


def check_pipeline(request, transform_mode: str, framing_mode: str, estimator: str, mesh=None, temporal_fill: int = 0,
                   sharpness=None, zoom=None) -> None:
    """What a rolling-shutter call cannot be combined with, each with its reason.  request: check_request's answer, not None;
    mesh / sharpness / zoom: the checked requests of those features (None: off)."""
    if transform_mode == "perspective":
        raise ValueError("rolling_shutter is not supported with transform_mode 'perspective': the image velocity of a "
                         "perspective transition is not affine, and the row correction is a closed form of an affine one.")
    if framing_mode == "crop":
        raise ValueError("rolling_shutter is not supported with framing_mode 'crop': the crop solver bounds matrices only, so it "
                         "cannot keep a per-row displacement free of padding.")
    if mesh is not None:
        raise ValueError("rolling_shutter is not supported with mesh_warp: the warp takes one displacement, and the mesh's "
                         "vertex residuals already hold what they could measure of the skew.")
    if int(temporal_fill) > 0:
        raise ValueError(f"rolling_shutter is not supported with temporal_fill={int(temporal_fill)}: fill candidates are "
                         "neighbour frames that have not been corrected.")
    if sharpness is not None:
        raise ValueError("rolling_shutter is not supported with sharpness_transfer: its candidates are neighbour frames that "
                         "have not been corrected.")
    if zoom is not None:
        raise ValueError("rolling_shutter is not supported with dynamic_zoom: its coverage-extent kernel does not know the "
                         "per-row displacement.")
    if estimator == "subject":
        raise ValueError("rolling_shutter is not supported with estimator 'subject': its transitions are the subject's, not the "
                         "camera's, and the readout shears with the camera's velocity.")
    if request == AUTO and estimator in _ESTIMATOR_LIMITS:
        raise ValueError(f"rolling_shutter='auto' is not supported with estimator {estimator!r}: {_ESTIMATOR_LIMITS[estimator]} "
                         "Give the readout as a number.")


_REFIT_ESTIMATOR_LIMITS = {
    "classic": "the Classic estimator tracks sparse corners: it has no grid of flow samples to rectify.",
    "flow_phase_correlate": "phase correlation yields one global shift per pair: it has no grid of flow samples to rectify.",
}


def check_refit_request(value, request, estimator: str, drift=None) -> bool:
    """rolling_refit, checked without the clip or a GPU -> whether the transitions are fitted again on readout-corrected
    samples.  value: None or a bool; request: check_request's answer for rolling_shutter; drift: drift_correction's checked
    request (None: off).  None / False -> False."""
    if value is None:
        return False
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"rolling_refit={value!r}: expected None or a bool")
    if not value:
        return False
    if request is None:
        raise ValueError("rolling_refit=True needs rolling_shutter: without a readout there is nothing to correct the samples for.")
    if estimator in _REFIT_ESTIMATOR_LIMITS:
        raise ValueError(f"rolling_refit is not supported with estimator {estimator!r}: {_REFIT_ESTIMATOR_LIMITS[estimator]}")
    if drift is not None:
        raise ValueError("rolling_refit is not supported with drift_correction: the keyframe alignment registers images that "
                         "have not been corrected for the readout, and its poses overwrite the fit table.")
    return True


def transition_change_px(first, second, size) -> np.ndarray:
    """Per pair, the largest displacement of the four corners of a w x h frame between two affine transitions [P,3,3] -> [P] px."""
    A = np.asarray(first, dtype=np.float64).reshape(-1, 3, 3)
    B = np.asarray(second, dtype=np.float64).reshape(-1, 3, 3)
    w, h = int(size[0]), int(size[1])
    corners = np.array([[0.0, 0.0, 1.0], [w - 1.0, 0.0, 1.0], [0.0, h - 1.0, 1.0], [w - 1.0, h - 1.0, 1.0]]).T
    d = (np.matmul(A, corners) - np.matmul(B, corners))[:, :2]
    return np.sqrt((d * d).sum(axis=1)).max(axis=1) if A.shape[0] else np.zeros(0)


def refit_block(passes: int, first=None, second=None, confidences=None, segments=None, unsolved=None, size=None) -> Dict[str, Any]:
    """meta["rolling_shutter"]["refit"].  passes 0 (a readout of 0: nothing was launched): zeros.  Else first / second: the
    full-resolution transitions of the first pass and of the refit, confidences / segments: the refit plan's, unsolved: the
    rectifier's per-pair counts.  pairs_refit: the pairs whose refit transition carries a measured motion."""
    if not passes:
        return {"passes": 0, "pairs_refit": 0, "samples_unsolved_max": 0, "transition_change_px_mean": 0.0,
                "transition_change_px_max": 0.0}
    change = transition_change_px(first, second, size)
    unsolved = np.asarray(unsolved).reshape(-1)
    return {
        "passes": int(passes),
        "pairs_refit": int(_available(confidences, segments, change.shape[0]).sum()),
        "samples_unsolved_max": int(unsolved.max()) if unsolved.size else 0,
        "transition_change_px_mean": float(change.mean()) if change.size else 0.0,
        "transition_change_px_max": float(change.max()) if change.size else 0.0,
    }


def _available(confidences, segments, pairs: int) -> np.ndarray:
    """Which of the `pairs` transitions carry a measured motion: confidence != 0 and both frames in one shot."""
    ok = np.asarray(confidences, dtype=np.float64).reshape(-1) != 0.0
    if ok.shape[0] != pairs:
        raise ValueError(f"rolling_shutter: {ok.shape[0]} confidences for {pairs} transitions")
    if segments is not None:
        for s, _ in segments:
            if 1 <= int(s) <= pairs:
                ok[int(s) - 1] = False          # the pair (s - 1, s) crosses a shot boundary
    return ok


def _affine_transitions(transitions) -> np.ndarray:
    A = np.asarray(transitions, dtype=np.float64).reshape(-1, 3, 3)
    bad = np.nonzero((A[:, 2] != np.array([0.0, 0.0, 1.0])).any(axis=1))[0]
    if bad.size:
        raise ValueError(f"rolling_shutter: transition {int(bad[0])} has the last row {A[bad[0], 2].tolist()}, not (0, 0, 1): "
                         "the image velocity of a perspective transition is not affine")
    return A


def velocities(transitions, confidences, segments=None) -> np.ndarray:
    """Per-frame image velocity V [N,6] (v(q) = (V0 q_x + V1 q_y + V2, V3 q_x + V4 q_y + V5), px per frame interval) from the
    N-1 transitions A_i (x_{i+1} = A_i x_i): the mean of the forward difference A_i q - q and the backward difference
    q - A_{i-1}^-1 q, of those that are available.  A pair with confidence 0 or across a shot boundary (segments: the shots'
    frame ranges [s, e), or None) is not available; with neither, the row is zeros.  Transitions must be affine."""
    A = _affine_transitions(transitions)
    pairs = A.shape[0]
    ok = _available(confidences, segments, pairs)
    eye = np.eye(3, dtype=np.float64)
    V = np.zeros((pairs + 1, 6), np.float64)
    for i in range(pairs + 1):
        parts = []
        if i < pairs and ok[i]:
            parts.append((A[i] - eye)[:2])
        if i > 0 and ok[i - 1]:
            det = np.linalg.det(A[i - 1][:2, :2])
            if det != 0.0 and np.isfinite(det):
                parts.append((eye - np.linalg.inv(A[i - 1]))[:2])
        if parts:
            V[i] = (sum(parts) / float(len(parts))).reshape(6)
    return V


def _apply_velocity(V, x, y):
    return V[0] * x + V[1] * y + V[2], V[3] * x + V[4] * y + V[5]


def estimate_readout(row_residual, row_count, work_transitions, confidences, modes: Sequence[str], segments, work_size,
                     step: int) -> Dict[str, Any]:
    """The least-squares readout from the per-row medians of the global fits' residuals.
    row_residual [P,gh,2], row_count [P,gh] (native.Context.row_residual_batch), work_transitions [P,3,3] at working resolution,
    confidences [P], modes [P] ("translation" | "similarity": what the pair's fit was), segments (shots' frame ranges or None),
    work_size (w, h), step: the grid's stride.

    To first order the residual of pair k at row y is r = rho * (y/(h-1) - 1/2) * (v_{k+1}(A_k p) - v_k(p)): what the readout
    shears is the CHANGE of velocity between the two frames.  With p = ((w-1)/2, y) -- a row median sits at the central
    column -- and m the same expression without rho, over the usable pairs and the rows with count >= ROW_MIN_SAMPLES:
    num += f_k * (r . m), den += m . m, rho_raw = num / den.  f_k undoes what the pair's own fit absorbed of a row-linear field:
    nothing for a translation, the share h^2 / (w^2 + h^2) for a least-squares similarity (f_k = (w^2 + h^2) / w^2).
    If the RMS of |m| over the used rows is below ROW_MIN_RMS_PX the clip has no acceleration to speak of and the readout is
    not observable: readout 0.
    -> {"readout", "source": "estimated" | "not_observable", "readout_raw", "pairs_used", "rows_used", "signal_rms_px"}."""
    r = np.asarray(row_residual, dtype=np.float64)
    cnt = np.asarray(row_count)
    pairs, gh = cnt.shape
    w, h = int(work_size[0]), int(work_size[1])
    A = _affine_transitions(work_transitions)
    if A.shape[0] != pairs or r.shape != (pairs, gh, 2) or len(modes) != pairs:
        raise ValueError(f"rolling_shutter: row residuals {r.shape}, counts {cnt.shape}, {A.shape[0]} transitions and "
                         f"{len(modes)} modes do not describe the same pairs")
    ok = _available(confidences, segments, pairs)
    # usable: the pair and both of its neighbours are available, so that v_k and v_{k+1} are both two-sided means.  A
    # one-sided difference is the velocity half a frame away; the change of velocity formed with it is half as large, and
    # the two end pairs of every shot would pull rho_raw up by ~5 % on a 12-frame clip.
    usable = ok.copy()
    usable[1:] &= ok[:-1]
    usable[:-1] &= ok[1:]
    if pairs:
        usable[[0, -1]] = False
    V = velocities(A, confidences, segments)
    y = (np.arange(gh) * int(step)).astype(np.float64)
    x = np.full(gh, (w - 1) / 2.0)
    lever = y / float(h - 1) - 0.5
    num = den = 0.0
    pairs_used = rows_used = 0
    for k in range(pairs):
        rows = cnt[k] >= ROW_MIN_SAMPLES
        if not usable[k] or not rows.any():
            continue
        f = float(w * w + h * h) / float(w * w) if modes[k] == "similarity" else 1.0
        ax = A[k][0, 0] * x + A[k][0, 1] * y + A[k][0, 2]
        ay = A[k][1, 0] * x + A[k][1, 1] * y + A[k][1, 2]
        nx, ny = _apply_velocity(V[k + 1], ax, ay)
        px, py = _apply_velocity(V[k], x, y)
        mx, my = (lever * (nx - px))[rows], (lever * (ny - py))[rows]
        num += f * float((r[k, rows, 0] * mx).sum() + (r[k, rows, 1] * my).sum())
        den += float((mx * mx).sum() + (my * my).sum())
        pairs_used += 1
        rows_used += int(rows.sum())
    rms = float(np.sqrt(den / rows_used)) if rows_used else 0.0
    observable = rows_used > 0 and den > 0.0 and rms >= ROW_MIN_RMS_PX and np.isfinite(num) and np.isfinite(den)
    raw = float(num / den) if observable else 0.0
    return {"readout": float(np.clip(raw, -1.0, 1.0)) if observable else 0.0,
            "source": "estimated" if observable else "not_observable",
            "readout_raw": raw, "pairs_used": pairs_used, "rows_used": rows_used, "signal_rms_px": rms}


def corner_skew(velocity, readout: float, size) -> np.ndarray:
    """|tau| * |v| at the four corners of a w x h frame, per frame -> [N,4] px: the warp's own closed form (clamp included)."""
    V = np.asarray(velocity, dtype=np.float64).reshape(-1, 6)
    w, h = int(size[0]), int(size[1])
    out = np.zeros((V.shape[0], 4), np.float64)
    for c, (qx, qy) in enumerate(((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0))):
        vx = V[:, 0] * qx + V[:, 1] * qy + V[:, 2]
        vy = V[:, 3] * qx + V[:, 4] * qy + V[:, 5]
        D = 1.0 - readout * vy / float(h - 1)
        D = np.where(D >= D_MIN, D, D_MIN)
        tau = readout * (qy / float(h - 1) - 0.5) / D
        out[:, c] = np.abs(tau) * np.sqrt(vx * vx + vy * vy)
    return out


def meta_block(readout: float, source: str, estimate: Optional[Dict[str, Any]], velocity, size) -> Dict[str, Any]:
    """meta["rolling_shutter"].  source: "given" | "estimated" | "not_observable"; estimate: estimate_readout's answer or None
    (a given readout).  skew_px_mean / skew_px_max: over the frames, each frame's largest |tau| * |v| of its four corners.
    `velocity` is in the meta so that the correction can be replayed or undone from the meta alone."""
    V = np.asarray(velocity, dtype=np.float64).reshape(-1, 6)
    skew = corner_skew(V, float(readout), size).max(axis=1) if V.shape[0] else np.zeros(0)
    return {
        "version": VERSION,
        "readout": float(readout),
        "source": source,
        "estimate": None if estimate is None else {key: estimate[key] for key in ("readout_raw", "pairs_used", "rows_used", "signal_rms_px")},
        "skew_px_mean": float(skew.mean()) if skew.size else 0.0,
        "skew_px_max": float(skew.max()) if skew.size else 0.0,
        "velocity": V.tolist(),
    }


def parse_block(meta, frame_count: int):
    """meta["rolling_shutter"] as meta_block wrote it (possibly through JSON) -> (readout, velocity f64 [frame_count,6]): what
    Motion Apply needs to apply the row correction again or to undo it.  A ValueError names the key or shape that is wrong."""
    block = meta.get("rolling_shutter") if isinstance(meta, dict) else None
    if not isinstance(block, dict):
        raise ValueError("rolling=True needs meta['rolling_shutter'], the block a Flow run with rolling_shutter= writes; "
                         "this meta has none.")
    if block.get("version") != VERSION or isinstance(block.get("version"), bool):
        raise ValueError(f"meta['rolling_shutter']['version'] is {block.get('version')!r}, expected {VERSION}")
    readout = block.get("readout")
    if not _is_number(readout) or not -1.0 <= float(readout) <= 1.0:        # (a NaN fails it too)
        raise ValueError(f"meta['rolling_shutter']['readout'] is {readout!r}, expected a number in [-1, 1]")
    n = int(frame_count)
    try:
        V = np.asarray(block.get("velocity"), dtype=np.float64)
    except (TypeError, ValueError):
        V = None
    if V is not None and n == 0 and V.size == 0:
        V = V.reshape(0, 6)                    # an empty clip's [] has lost its second axis
    if V is None or V.shape != (n, 6) or not np.isfinite(V).all():
        shape = "not an array of numbers" if V is None else f"of shape {list(V.shape)}"
        raise ValueError(f"meta['rolling_shutter']['velocity'] is {shape}; expected [{n}][6] finite numbers, one row per frame")
    return float(readout), np.ascontiguousarray(V)
