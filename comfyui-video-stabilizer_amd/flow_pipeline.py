"""Whole-clip pipeline of the `Video Stabilizer Flow` node on one MI355X.

Same stages, meta keys and soft-failure rules as the reference's
nodes/video_stabilizer_flow.py:213-640 (`_stabilize_frames`), but batched over the clip:

    gray+downscale (HIP) -> DIS flow for all N-1 pairs (HIP) -> model fit for all pairs (HIP)
    -> sticky-mode selection + parameter deltas (host, sequential by definition)
    -> prefix sum / box smoothing / blend (HIP, fp64) -> framing geometry (host fp64)
    -> warp + padding mask + per-frame padding count for all N frames (HIP)

The host keeps only what is sequential or scalar in the reference (flow.py:324-346, 360-546,
596-640).  There is no CPU fallback for the pixel stages.
"""

from __future__ import annotations

import gc
import os
from dataclasses import dataclass, replace
from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np

from . import clean_plate as clean_plate_mod
from . import deflicker as deflicker_mod
from . import dynamic_zoom as dynamic_zoom_mod
from . import horizon_level as horizon_level_mod
from . import host_math as hm
from . import mesh_warp as mesh_warp_mod
from . import native
from . import scene_cuts as scene_cuts_mod
from . import mask_handoff as mask_handoff_mod
from . import rolling_shutter as rolling_shutter_mod
from . import drift_correction as drift_correction_mod
from . import sharpness_transfer as sharpness_transfer_mod
from . import spatial_fill as spatial_fill_mod
from . import stability as stability_mod
from . import subject_lock as subject_lock_mod
from . import template_track as template_track_mod
from . import temporal_fill as temporal_fill_mod
from .comfy_compat import ProgressBar, check_interrupt
from .meta_v2 import applied_motion_meta_from_arrays, applied_motion_meta_from_stabilization_warp

SAMPLE_STEP = 8  # flow.py:138


class _gc_paused:
    """The plan / meta builders create tens of thousands of small Python objects per clip; a generational GC
    pass landing in the middle costs more than the work itself.  Collection is only postponed, not skipped."""

    def __enter__(self):
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc):
        if self.was:
            gc.enable()
        return False


# The Classic node (nodes/video_stabilizer_classic.py) shares this pipeline; only the estimator and a few
# meta keys differ: no flow_backend / flow_fallback_reason (classic.py:189-208, 236-250, 336-360, 537-568),
# no per-transition residual (classic.py:549-557), source "estimated_classic" (classic.py:57-61).
#
# "flow_phase_correlate" is the Flow node running on its fallback estimator (flow.py:90-130).  The reference takes
# that branch when cv2.DISOpticalFlow cannot be created and cv2.optflow (TV-L1, contrib) is missing; here DIS
# always exists, so the branch is selected only by VSTAB_FLOW_BACKEND=phase_correlate (see resolve_flow_backend).
#
# "flow_tvl1" is the Flow node on its second dense backend, cv2.optflow.DualTVL1OpticalFlow (flow.py:76-80), which the
# reference picks when DIS cannot be created; here it is chosen by the caller (_stabilize_frames(estimator="flow_tvl1")).
#
# "subject" (subject_lock.py, beyond the reference) measures no camera at all: its transitions are those of a masked
# subject's centroid and area, so that everything behind the fit table holds the subject still instead of the background.
#
# "track" (template_track.py, beyond the reference) is the subject lock without a mask: the subject is one box in one frame,
# followed through the estimation images by a fixed-template search; its transitions are the subject's as well.
_META_SOURCE = {"flow": "estimated_flow", "flow_phase_correlate": "estimated_flow", "flow_tvl1": "estimated_flow",
                "classic": "estimated_classic", "subject": "estimated_subject", "track": "estimated_subject"}
_PHASE_REASON = "DIS unavailable (disabled by VSTAB_FLOW_BACKEND); cv2.optflow missing; using phase correlation."
_TVL1_REASON = "DIS unavailable (disabled by the caller); using TV-L1."


def resolve_flow_backend(estimator: str) -> str:
    """_select_flow_backend (flow.py:90-107) for this build: DIS unless the environment asks for the fallback."""
    if estimator != "flow":
        return estimator
    want = os.environ.get("VSTAB_FLOW_BACKEND", "DIS").strip()
    if want in ("", "DIS", "dis"):
        return "flow"
    if want == "phase_correlate":
        return "flow_phase_correlate"
    raise ValueError(f"VSTAB_FLOW_BACKEND={want!r}: expected 'DIS' or 'phase_correlate' (TV-L1 needs opencv-contrib in the "
                     "reference and is not provided).")


def _backend_fields(estimator: str) -> Dict[str, Any]:
    if estimator == "flow":
        return {"flow_backend": "DIS", "flow_fallback_reason": None}
    if estimator == "flow_phase_correlate":
        return {"flow_backend": "phase_correlate", "flow_fallback_reason": _PHASE_REASON}
    if estimator == "flow_tvl1":
        return {"flow_backend": "TVL1", "flow_fallback_reason": _TVL1_REASON}
    if estimator == "subject":
        return {"flow_backend": "subject_mask", "flow_fallback_reason": None}
    if estimator == "track":
        return {"flow_backend": "template_track", "flow_fallback_reason": None}
    return {}


def _attach_motion_meta(meta: Dict[str, Any], fps: float, estimator: str = "flow") -> Dict[str, Any]:
    """flow.py:62-73: a failure to derive motion_meta is swallowed, the rest of the meta survives."""
    try:
        meta["motion_meta"] = applied_motion_meta_from_stabilization_warp(
            meta["stabilization_warp"], fps=fps, source=_META_SOURCE[estimator])
    except (KeyError, TypeError, ValueError, np.linalg.LinAlgError):
        pass
    return meta


def _replay_progress(pbar, done: int, count: int, total: int, stride: int = 10) -> int:
    """Emit the update_absolute sequence the reference's per-item loop produces (flow.py:347-351, 589-593):
    one call per `stride` finished items and one for the remainder."""
    for upto in range(stride, count + 1, stride):
        pbar.update_absolute(done + upto, total)
    if count % stride:
        pbar.update_absolute(done + count, total)
    return done + count


_MODE_INDEX = {"translation": 0, "similarity": 1, "perspective": 2}
_MODE_NAME = ("translation", "similarity", "perspective")


def select_transitions(fit_records, requested_mode: str):
    """Sequential 'sticky active_mode' walk over the per-pair candidate fits (flow.py:324-339, 153-210).

    `fit_records`: structured table [P,3] (native.FIT_DTYPE) or the equivalent list of dicts.
    Returns (matrices f32 [P,3,3] @ working resolution, modes, confidences, residuals, final active mode)."""
    table = fit_records if isinstance(fit_records, np.ndarray) else native.fit_table_from_dicts(fit_records)
    pairs = table.shape[0]
    usable = (table["computed"] != 0) & (table["accepted"] != 0)   # [P,3], mode index 0..2
    active = _MODE_INDEX[requested_mode]
    if pairs and usable[:, active].all():   # the common case: the requested model was accepted for every pair
        rows = table[:, active]
        return (rows["matrix"].reshape(pairs, 3, 3).astype(np.float32), [requested_mode] * pairs, rows["confidence"].tolist(),
                rows["residual"].tolist(), requested_mode)
    chosen = np.empty(pairs, dtype=np.int64)
    p = 0
    while p < pairs:
        # the active mode keeps winning until the first pair whose fit at that mode was rejected
        ok = usable[p:, active]
        run = int(ok.size if ok.all() else np.argmin(ok))
        chosen[p:p + run] = active
        p += run
        if p >= pairs:
            break
        pick = -1
        for m in range(active - 1, -1, -1):   # perspective -> similarity -> translation
            if usable[p, m]:
                pick = m
                break
        chosen[p] = pick
        # no candidate at all (fewer than 12 finite samples, flow.py:153-154): identity, reported as "translation"
        active = pick if pick >= 0 else 0
        p += 1
    idx = chosen
    safe = np.where(idx >= 0, idx, 0)
    rows = table[np.arange(pairs), safe]
    mats = rows["matrix"].reshape(pairs, 3, 3).astype(np.float32)
    confs = rows["confidence"].astype(np.float64)
    resids = rows["residual"].astype(np.float64)
    missing = idx < 0
    if missing.any():
        mats[missing] = np.eye(3, dtype=np.float32)
        confs[missing] = 0.0
        resids[missing] = 0.0
    modes = [_MODE_NAME[m] if m >= 0 else "translation" for m in chosen.tolist()]
    return mats, modes, confs.tolist(), resids.tolist(), _MODE_NAME[active]


def _gray(ctx, device_frames, working_size, peaks_out, gray_out=None):
    """F2, plus the per-frame maxima of the same pass when the caller still owes the value-range sniff (F0).
    gray_out: a list that receives the estimation images themselves (the scene-cut score reads them after the fits)."""
    if peaks_out is None:
        gray = ctx.gray_downscale(device_frames, working_size)
    else:
        gray, peaks = ctx.gray_downscale(device_frames, working_size, want_range=True)
        peaks_out.append(hm.prefetch_peaks(peaks))
    if gray_out is not None:
        gray_out.append(gray)
    return gray


def estimate_transitions(ctx, device_frames, working_size, transform_mode: str, clip_start: bool = True, peaks_out=None,
                         blocked=None, gray_out=None, grid_out=None):
    """F2-F5 for frames [N,H,W,3] on the device -> per-pair candidate fits (structured table [N-1,3]).
    peaks_out: a list that receives the device tensor of per-frame maxima (see host_math.resolve_value_range).
    blocked: the estimation mask's block grid (u8 [N,gh,gw], Context.mask_block_grid); the flow itself is computed on the
    unmasked images.  grid_out: a list that receives the grid of flow samples itself (the mesh warp reads it after the fits)."""
    gray = _gray(ctx, device_frames, working_size, peaks_out, gray_out)
    _, grid = ctx.dis_flow_batch(gray, sample_step=SAMPLE_STEP, want_full=False, want_grid=True, clip_start=clip_start)
    if grid_out is not None:
        grid_out.append(grid)
    return ctx.sample_fit_batch(grid, SAMPLE_STEP, transform_mode, blocked=blocked)


def estimate_transitions_phase(ctx, device_frames, working_size, transform_mode: str, clip_start: bool = True, peaks_out=None,
                               gray_out=None):
    """Fallback estimator (flow.py:110-130, 325-330): phase correlation of consecutive estimation images.  Every pair
    is reported as a "translation" fit whatever `transform_mode` asks for; confidence = peak response, residual 0."""
    gray = _gray(ctx, device_frames, working_size, peaks_out, gray_out)
    table, _ = ctx.phase_correlate_batch(gray)
    return table


def estimate_transitions_tvl1(ctx, device_frames, working_size, transform_mode: str, clip_start: bool = True, peaks_out=None,
                              blocked=None, gray_out=None, grid_out=None):
    """Second dense estimator (flow.py:76-80, 140-147): Dual TV-L1 flow with OpenCV's default parameters on the
    estimation images, sampled and fitted exactly as the DIS flow is.  Pairs are independent (no initial flow), so
    clip_start does not matter."""
    gray = _gray(ctx, device_frames, working_size, peaks_out, gray_out)
    _, grid, _ = ctx.tvl1_flow_batch(gray, sample_step=SAMPLE_STEP, want_full=False, want_grid=True)
    if grid_out is not None:
        grid_out.append(grid)
    return ctx.sample_fit_batch(grid, SAMPLE_STEP, transform_mode, blocked=blocked)


_ESTIMATORS = {}   # filled below the four estimator functions


# classic.py:76-96: cv2.goodFeaturesToTrack / cv2.calcOpticalFlowPyrLK arguments of the Classic node
CLASSIC_GFTT = dict(max_corners=400, quality=0.01, min_distance=7.0, block_size=21)
CLASSIC_LK = dict(win=31, max_level=3, max_count=50, epsilon=0.01)


def estimate_transitions_classic(ctx, device_frames, working_size, transform_mode: str, clip_start: bool = True, peaks_out=None,
                                 gray_out=None):
    """Classic estimator (classic.py:69-160) for frames [N,H,W,3] on the device -> candidate fits [N-1,3]:
    corners of frame i (HIP) -> pyramidal LK into frame i+1 (HIP) -> model fits on the tracked pairs (HIP)."""
    gray = _gray(ctx, device_frames, working_size, peaks_out, gray_out)
    corners, counts = ctx.gftt_batch(gray[:-1], **CLASSIC_GFTT)
    pairs = ctx.lk_track_batch(gray, corners, counts, **CLASSIC_LK)
    return ctx.points_fit_batch(pairs, counts, transform_mode)


def estimate_transitions_subject(ctx, device_frames, working_size, transform_mode: str, clip_start: bool = True, peaks_out=None,
                                 subject=None):
    """Subject lock (subject_lock.py): one reduction over the mask clip (HIP), 28 bytes per frame to the host, the candidate
    fits from the subject's centroid and area.  subject: {"mask": device f32 [N,H,W]}; receives "block", meta["subject_lock"].
    The frames are never read, so where the caller still owes the value-range sniff (F0) their per-frame maxima come from a
    pass of their own, as in Motion Apply."""
    if peaks_out is not None:
        peaks_out.append(hm.prefetch_peaks(ctx.frame_range(device_frames)))
    size = (int(device_frames.shape[2]), int(device_frames.shape[1]))
    table, subject["block"] = subject_lock_mod.estimate_on_device(ctx, subject["mask"], size, working_size)
    return table


def estimate_transitions_track(ctx, device_frames, working_size, transform_mode: str, clip_start: bool = True, peaks_out=None,
                               gray_out=None, track=None):
    """Template track (template_track.py): the estimation images as every camera estimator makes them (the owed F0 peaks come
    from that pass, as for DIS), one call that follows the box through them on the device (HIP), 92 bytes per frame to the
    host, the candidate fits from the box's centres.  track: {"request": (box, key, radius)}; receives "block",
    meta["template_track"]."""
    gray = _gray(ctx, device_frames, working_size, peaks_out, gray_out)
    size = (int(device_frames.shape[2]), int(device_frames.shape[1]))
    table, track["block"] = template_track_mod.estimate_on_device(ctx, gray, track["request"], size, working_size)
    return table


_ESTIMATORS.update({"flow": estimate_transitions, "flow_phase_correlate": estimate_transitions_phase,
                    "flow_tvl1": estimate_transitions_tvl1, "classic": estimate_transitions_classic,
                    "subject": estimate_transitions_subject, "track": estimate_transitions_track})


def _fps_fields(context: hm.VideoContext, frame_rate) -> Tuple[float, Optional[float]]:
    cand = frame_rate
    if not isinstance(cand, (int, float)) or not np.isfinite(cand) or cand <= 0.0:
        cfps = context.fps
        cand = cfps if isinstance(cfps, (int, float)) and np.isfinite(cfps) and cfps > 0.0 else 16.0
    effective = float(max(1.0, cand))
    requested = float(frame_rate) if isinstance(frame_rate, (int, float)) and frame_rate > 0.0 else None
    return effective, requested


def _host_frames(context: hm.VideoContext) -> np.ndarray:
    if context.batch is not None:
        hm.resolve_value_range(context)
        return context.batch.detach().cpu().numpy()
    if context.batch_u8 is not None:
        arr = context.batch_u8.numpy().astype(np.float32)
        arr /= 255.0
        return arr
    return np.stack([hm._ensure_rgb(f) for f in context.frames], axis=0)


@dataclass
class FlowPlan:
    """Everything the warp stage and the meta need, derived on the host from the per-pair fits
    (replicated on every rank in multi-GPU runs: deterministic fp64 / integer logic only)."""

    final_matrices: np.ndarray         # float32 [N,3,3] (source -> output), stacked: indexable per frame, no list copies
    output_size: Tuple[int, int]
    meta_head: Dict[str, Any]          # keys of flow.py:598-611 that do not depend on the warp
    framing_meta: Dict[str, Any]
    estimated_motion: Dict[str, Any]
    framing_mode: str
    source_size: Tuple[int, int]
    fps_effective: float
    bypass_meta: Optional[Dict[str, Any]] = None
    estimator: str = "flow"


def plan_stabilization(*args, **kwargs) -> "FlowPlan":
    with _gc_paused():
        return _plan_stabilization(*args, **kwargs)


def _select_per_segment(fit_records, transform_mode: str, segments):
    """select_transitions run shot by shot: the sticky walk restarts at the requested mode in every segment, and the pair
    across each cut is reported in the "no candidate" form (identity, confidence 0, residual 0, "translation").
    -> the five values of select_transitions for the whole clip; the active mode is the last segment's."""
    table = fit_records if isinstance(fit_records, np.ndarray) else native.fit_table_from_dicts(fit_records)
    pairs = table.shape[0]
    work_mats = np.tile(np.eye(3, dtype=np.float32), (pairs, 1, 1))
    modes, confs, resids = ["translation"] * pairs, [0.0] * pairs, [0.0] * pairs
    active = transform_mode
    for s, e in segments:
        if e - s < 2:           # a one-frame shot has no transition of its own
            active = transform_mode
            continue
        m, md, cf, rs, active = select_transitions(table[s:e - 1], transform_mode)
        work_mats[s:e - 1] = m
        modes[s:e - 1], confs[s:e - 1], resids[s:e - 1] = md, cf, rs
    return work_mats, modes, confs, resids, active


def keep_fov_bypasses(framing_mode: str, keep_fov: float) -> bool:
    """flow.py:387: `crop` framing with keep_fov ~ 1 returns the original frames.  The plan decides it; what would only feed
    the plan (the drift correction) asks here too, so that the bypass launches nothing."""
    return framing_mode == "crop" and float(np.clip(keep_fov, 0.0, 1.0)) >= 0.9999


def _plan_stabilization(ctx, fit_records, size, total_frames, framing_mode, transform_mode, camera_lock, strength, smooth,
                       keep_fov, padding_rgb, fps_effective, fps_requested, estimator: str = "flow", segments=None,
                       path_deltas=None) -> FlowPlan:
    """flow.py:324-546 for a whole clip: sticky-mode selection, parameter deltas, trajectory (HIP fp64),
    framing geometry.  `fit_records` covers all N-1 transitions of the clip.
    segments (scene cuts; None: one continuous camera move, the reference's behaviour): frame ranges [s, e) of the shots.
    Selection and trajectory run per shot -- every shot's path starts at 0 -- and are concatenated; the framing below stays
    global, so there is one output geometry.
    path_deltas (drift correction; None: the reference's behaviour): float64 [N-1, P], the per-pair steps of a path formed
    elsewhere.  They replace the parameter deltas of the table's matrices in the trajectory, per shot as those; `matrices`,
    modes and confidences still come from the table."""
    width, height = size
    rgb_list = [int(c) for c in padding_rgb]
    base_mode = transform_mode
    working_size = hm._working_estimation_size(width, height)
    if segments is None:
        work_mats, modes_used, confidences, residuals, active_mode = select_transitions(fit_records, transform_mode)
    else:
        work_mats, modes_used, confidences, residuals, active_mode = _select_per_segment(fit_records, transform_mode, segments)
    # rescale to full resolution + parameter deltas (flow.py:340-346), one library call over the clip
    matrices, delta_params = native.transitions_to_params(work_mats, base_mode, size, working_size)
    if path_deltas is not None:
        path_deltas = np.ascontiguousarray(path_deltas, dtype=np.float64)
        if path_deltas.shape != delta_params.shape:
            raise ValueError(f"path_deltas of shape {path_deltas.shape} are not {delta_params.shape}")
        delta_params = path_deltas

    # ---- trajectory (F7-F8) --------------------------------------------------
    strength = float(np.clip(strength, 0.0, 1.0))
    smooth = float(np.clip(smooth, 0.0, 1.0))
    if segments is None:
        path, target_path = ctx.trajectory(delta_params, smooth, fps_effective, strength, bool(camera_lock))
    else:
        path = np.zeros((total_frames, delta_params.shape[1]), np.float64)
        target_path = np.zeros_like(path)
        for s, e in segments:
            if e - s >= 2:      # (the transitions are converted pair by pair, so a shot's deltas are its slice of the clip's)
                path[s:e], target_path[s:e] = ctx.trajectory(delta_params[s:e - 1], smooth, fps_effective, strength, bool(camera_lock))
    if camera_lock:
        smooth = max(smooth, 0.85)
    diffs = target_path - path

    keep_fov_clamped = float(np.clip(keep_fov, 0.0, 1.0))
    keep_fov_applied = framing_mode == "crop" and keep_fov_clamped > 1e-6
    stabilization_scale = 1.0

    if framing_mode == "crop":
        if keep_fov_bypasses(framing_mode, keep_fov):  # flow.py:387-429: return the original frames
            meta = {
                "frames": total_frames,
                "note": "keep_fov~=1.0 in crop mode; returning original frames.",
                "transform_mode_requested": transform_mode,
                "transform_mode_applied": "identity",
                "camera_lock": camera_lock,
                "strength": strength,
                "strength_effective": 0.0,
                "smooth": smooth,
                "fps_requested": fps_requested,
                "fps_effective": fps_effective,
                "framing": {
                    "mode": framing_mode,
                    "input_size": list(size),
                    "keep_fov_requested": keep_fov_clamped,
                    "keep_fov_effective": 1.0,
                    "min_content_ratio": 1.0,
                    "padding_color_rgb": rgb_list,
                    "stabilization_scale": 0.0,
                },
                "keep_fov_applied": False,
                **_backend_fields(estimator),
                "stabilization_warp": hm._build_stabilization_warp_meta(
                    source_size=size, output_size=size, framing_mode=framing_mode,
                    applied_matrices=[np.eye(3, dtype=np.float32) for _ in range(total_frames)]),
                "estimated_motion": {
                    "per_transition": [],
                    "path": path.tolist(),
                    "target_path": target_path.tolist(),
                    "target_path_effective": path.tolist(),
                },
                "padding_fraction_mean": 0.0,
                "padding_fraction_max": 0.0,
            }
            return FlowPlan(np.zeros((0, 3, 3), np.float32), size, {}, {}, {}, framing_mode, size, fps_effective, bypass_meta=meta,
                            estimator=estimator)
        # flow.py:431-470: keep_fov solver, then the padding-free refinement
        from .crop_solver import solve_crop

        sol = solve_crop(ctx, base_mode, list(diffs), width, height, keep_fov_clamped,
                         max(0.5, 0.02 * max(width, height)), interrupt_check=check_interrupt)
        crop_solution = sol
        apply_matrices = np.stack([np.asarray(m, dtype=np.float32) for m in sol["apply_matrices"]])
        stabilization_scale = sol["scale"]
    else:
        crop_solution = None
        apply_matrices = native.params_to_matrices(diffs, base_mode)
    output_size = size
    mins, maxs = native.bounding_boxes(apply_matrices, width, height)   # f32 matrices (params_to_matrices / crop solver)
    framing_meta: Dict[str, Any] = {
        "mode": framing_mode,
        "input_size": list(size),
        "padding_color_rgb": rgb_list,
        "min_content_ratio": hm._min_content_ratio(mins, maxs, width, height),
    }
    if framing_mode == "crop":  # flow.py:485-499
        final_matrices = np.stack([np.asarray(m, dtype=np.float32) for m in crop_solution["final_matrices"]])
        framing_meta.update({
            "keep_fov_status": crop_solution["status"],
            "keep_fov_effective": crop_solution["keep_fov_effective"],
            "crop_origin": crop_solution["crop_origin"],
            "crop_size": crop_solution["crop_size"],
            "actual_content_ratio": crop_solution["keep_fov_effective"],
            "stabilization_scale": float(stabilization_scale),
        })
        if keep_fov_applied:
            framing_meta["keep_fov_requested"] = keep_fov_clamped
        if crop_solution["note"]:
            framing_meta["keep_fov_note"] = crop_solution["note"]
    elif framing_mode == "crop_and_pad":  # flow.py:500-529
        x0, y0 = float(np.max(mins[:, 0])), float(np.max(mins[:, 1]))
        x1, y1 = float(np.min(maxs[:, 0])), float(np.min(maxs[:, 1]))
        inter_w, inter_h = max(1.0, x1 - x0), max(1.0, y1 - y0)
        off_x = width * 0.5 - (x0 + x1) * 0.5
        off_y = height * 0.5 - (y0 + y1) * 0.5
        shift = np.array([[1.0, 0.0, off_x], [0.0, 1.0, off_y], [0.0, 0.0, 1.0]], dtype=np.float32)
        final_matrices = np.matmul(shift, apply_matrices)
        framing_meta.update({
            "safe_region_origin": [x0, y0],
            "safe_region_size": [inter_w, inter_h],
            "actual_content_ratio": min(inter_w / width, inter_h / height),
            "center_offset": [off_x, off_y],
        })
    elif framing_mode == "expand":  # flow.py:530-533
        shift, output_size = hm._prepare_expand_transform(mins, maxs)
        final_matrices = np.matmul(shift, apply_matrices)
        framing_meta["expanded_size"] = list(output_size)
    else:
        raise ValueError(f"Unsupported framing_mode {framing_mode!r}; expected 'crop', 'crop_and_pad', or 'expand'.")

    effective_diffs = hm.matrices_to_params(apply_matrices, base_mode) if framing_mode == "crop" else diffs  # flow.py:535-539
    stabilization_scale = float(np.clip(stabilization_scale, 0.0, 1.0))
    effective_target_path = path + effective_diffs
    meta_head = {
        "frames": total_frames,
        "transform_mode_requested": transform_mode,
        "transform_mode_applied": active_mode,
        "camera_lock": camera_lock,
        "strength": strength,
        "strength_effective": strength * stabilization_scale,
        "smooth": smooth,
        "fps_requested": fps_requested,
        "fps_effective": fps_effective,
        "keep_fov_applied": keep_fov_applied,
        "padding_color_rgb": rgb_list,
        **_backend_fields(estimator),
    }
    estimated_motion = {   # arrays; turned into JSON lists by prepare_meta (off the critical path)
        "modes": modes_used, "confidences": confidences, "residuals": residuals, "matrices": matrices,
        "work_matrices": work_mats,   # (not a meta key: what the mesh warp measures its residual against)
        "path": path, "target_path": target_path, "target_path_effective": effective_target_path,
    }
    return FlowPlan(final_matrices, output_size, meta_head, framing_meta, estimated_motion, framing_mode, size, fps_effective,
                    estimator=estimator)


def prepare_meta(plan: FlowPlan) -> Dict[str, Any]:
    with _gc_paused():
        return _prepare_meta(plan)


def _prepare_meta(plan: FlowPlan) -> Dict[str, Any]:
    """Everything of flow.py:596-640 that does not depend on the warped pixels (the heavy JSON part:
    stabilization_warp + motion_meta).  Called while the warp kernel is still running."""
    h = plan.meta_head
    em = plan.estimated_motion
    final_stack = plan.final_matrices
    meta = {
        "frames": h["frames"],
        "transform_mode_requested": h["transform_mode_requested"],
        "transform_mode_applied": h["transform_mode_applied"],
        "camera_lock": h["camera_lock"],
        "strength": h["strength"],
        "strength_effective": h["strength_effective"],
        "smooth": h["smooth"],
        "fps_requested": h["fps_requested"],
        "fps_effective": h["fps_effective"],
        "framing": dict(plan.framing_meta),
        "keep_fov_applied": h["keep_fov_applied"],
        "padding_color_rgb": h["padding_color_rgb"],
        **_backend_fields(plan.estimator),
        "stabilization_warp": hm._build_stabilization_warp_meta(
            source_size=plan.source_size, output_size=plan.output_size, framing_mode=plan.framing_mode,
            applied_matrices=final_stack),
        "estimated_motion": {
            "per_transition": [
                {"index": i, "mode": mode, "confidence": conf, "residual": resid, "matrix": mat}
                for i, (mode, conf, resid, mat) in enumerate(zip(em["modes"], em["confidences"], em["residuals"],
                                                                 np.asarray(em["matrices"], dtype=np.float32).tolist()))
            ] if plan.estimator != "classic" else [
                {"index": i, "mode": mode, "confidence": conf, "matrix": mat}
                for i, (mode, conf, mat) in enumerate(zip(em["modes"], em["confidences"],
                                                          np.asarray(em["matrices"], dtype=np.float32).tolist()))
            ],
            "path": em["path"].tolist(),
            "target_path": em["target_path"].tolist(),
            "target_path_effective": em["target_path_effective"].tolist(),
        },
        "padding_fraction_mean": None,
        "padding_fraction_max": None,
    }
    fast = applied_motion_meta_from_arrays(final_stack, plan.source_size, plan.output_size, plan.fps_effective,
                                           _META_SOURCE[plan.estimator])
    if fast is not None:
        meta["motion_meta"] = fast
        return meta
    return _attach_motion_meta(meta, plan.fps_effective, plan.estimator)


def complete_meta(meta: Dict[str, Any], plan: FlowPlan, pad_counts) -> Dict[str, Any]:
    """flow.py:583-588, 596, 636-637: padding statistics from the per-frame padded-pixel counts."""
    counts = np.asarray(pad_counts, dtype=np.int64)
    pixels = np.float32(plan.output_size[0] * plan.output_size[1])
    padded_ratios = (counts.astype(np.float32) / pixels).astype(np.float64)  # mask.mean() in float32 (flow.py:587)
    meta["framing"]["padding_detected"] = bool((counts > 0).any())
    meta["padding_fraction_mean"] = float(np.mean(padded_ratios))
    meta["padding_fraction_max"] = float(np.max(padded_ratios))
    return meta


def finish_meta(plan: FlowPlan, pad_counts) -> Dict[str, Any]:
    return complete_meta(prepare_meta(plan), plan, pad_counts)


# ---- the plan formed on the device, speculatively (csrc/vstab_traj.hip: plan_kernel) ---------------------------------
# Between the last model fit and the first warp the reference runs its sequential host logic (flow.py:324-371, 472-521).
# Formed on the host that is a download of the fits, ~0.15 ms of arithmetic, an upload of the matrices and a launch: ~0.24 ms
# in which the GPU idles (3 % of a C2 step, more of a rank's step in a multi-GPU run).  For the common configuration --
# DIS estimator, crop_and_pad, translation / similarity -- the same logic runs as one small fp64 kernel behind the fit
# kernel and the warp is queued behind it at once.  The host still forms the plan, with the HOST's libm as the reference
# does (it needs the fits for the meta anyway), while the warp runs, then compares its float32 final matrices with the
# device's bit for bit: a frame whose matrix differs (the device's atan2 / log / exp / cos / sin may differ from glibc's in
# the last bit of a double, which survives the float32 cast about once in 1e8 entries) is warped again with the host's.
# What is returned is therefore always the host plan's result.  VSTAB_DEVICE_PLAN=0 switches the speculation off (A/B).
_DEVICE_PLAN_MAX_FRAMES = 4096          # plan_kernel keeps the path [frames, 4] fp64 in LDS (perspective: [frames, 8], half as many)
PLAN_PARAMS = {"translation": 2, "similarity": 4, "perspective": 8}   # parameters per frame of a model's path
_DEVICE_PLAN_MAX_SEGMENTS = 64          # plan_kernel's segment table (PLAN_MAX_SEG in csrc/vstab_traj.hip): ranks of a sharded run


def device_plan_applies(estimator: str, framing_mode: str, transform_mode: str, total_frames: int, segments: int = 1) -> bool:
    """Whether the speculative device plan covers this call.  `segments`: the ranks whose record blocks plan_kernel would
    read from an all-gather's receive buffer (a world beyond its segment table takes the host-plan form, which has no limit).
    What a call did is reported in its result (`StabilizationResult.device_plan`, `stats["device_plan"]` of a sharded call):
    {"used": bool, "mismatched_frames": int} -- there is no module-level record."""
    return (os.environ.get("VSTAB_DEVICE_PLAN", "1") not in ("0", "false", "False") and estimator == "flow"
            and framing_mode in ("crop_and_pad", "expand") and transform_mode in PLAN_PARAMS
            and 2 <= total_frames <= (_DEVICE_PLAN_MAX_FRAMES * 4) // max(PLAN_PARAMS[transform_mode], 4)
            and 1 <= segments <= _DEVICE_PLAN_MAX_SEGMENTS)


def _counts_to_host(counts, mirrored: bool = True) -> np.ndarray:
    """The warp's per-frame padded-pixel counts on the host: from the mirror the library keeps behind the warp kernel (no copy,
    no stream synchronisation of ours) where the tensor carries its fetch handle, else by a transfer."""
    fetch = getattr(counts, "_vstab_fetch", None) if mirrored else None
    return fetch() if fetch is not None else counts.cpu().numpy()


def _rewarp_mismatched(ctx, device_frames, plan, final_dev, dst, mask, counts, padding_rgb) -> int:
    """Frames whose device-plan matrix is not the host plan's, bit for bit, are warped again with the host's."""
    host = np.ascontiguousarray(plan.final_matrices, np.float32)
    bad = np.nonzero((host.view(np.uint32) != np.ascontiguousarray(final_dev).view(np.uint32)).reshape(len(host), -1).any(axis=1))[0]
    # runs of consecutive frames go in one launch each, straight into their slices of the outputs: the one situation with
    # MANY differing frames (an exactly constant rotation path after a sticky fallback) costs one more warp of those
    # frames, not a launch per frame
    if bad.size:
        cuts = np.nonzero(np.diff(bad) > 1)[0] + 1
        for run in np.split(bad, cuts):
            a, b = int(run[0]), int(run[-1]) + 1
            _, _, c2 = ctx.warp_batch(device_frames[a:b], host[a:b], plan.output_size, interp="bilinear",
                                      border=hm.border_value(padding_rgb), want_mask=True, want_count=True, out=dst[a:b],
                                      out_mask=mask[a:b])
            counts[a:b].copy_(c2)
    return int(bad.size)


def _temporal_fill(ctx, device_frames, dst, mask, plan, meta, radius: int, blend=(None, False)) -> None:
    """Fills the warp's padding from neighbouring frames in place (temporal_fill.py) and adds meta["temporal_fill"]; the
    other meta keys keep describing the warp.  `crop` framing has no padding: nothing to do.  blend = (feather px | None,
    exposure): temporal_fill.check_blend_request's answer; (None, False) is the plain fill."""
    if radius <= 0 or plan.framing_mode == "crop":
        return
    em = plan.estimated_motion
    meta["temporal_fill"] = temporal_fill_mod.fill_on_device(
        ctx, device_frames, dst, mask, plan.final_matrices, np.asarray(em["matrices"], dtype=np.float32), em["confidences"], radius,
        feather=blend[0], exposure=blend[1])


def _deflicker(ctx, device_frames, dst, mask, plan, meta, request, segments=None) -> None:
    """Takes the exposure steps between consecutive frames out of the warped frames in place (deflicker.py) and adds
    meta["deflicker"]; the mask and the other meta keys are unchanged.  request: deflicker.check_request's answer.  It measures
    on the SOURCE frames through the plan's own full-resolution transitions -- whatever estimator, refit or drift correction
    made them -- and applies to the frame's own pixels: padding keeps its colour.  `crop` framing has no mask: every pixel is
    own."""
    if request is None:
        return
    em = plan.estimated_motion
    meta["deflicker"] = deflicker_mod.deflicker_on_device(
        ctx, request, device_frames, dst, None if plan.framing_mode == "crop" else mask, np.asarray(em["matrices"], dtype=np.float32),
        em["confidences"], plan.fps_effective, segments)


def _sharpness_transfer(ctx, device_frames, dst, mask, plan, meta, sharp) -> None:
    """Pulls the own pixels of blurred frames towards what sharper neighbours show there, in place (sharpness_transfer.py), and
    adds meta["sharpness_transfer"]; mask and the other meta keys are unchanged.  sharp = (radius, alpha) or None:
    sharpness_transfer.check_request's answer.  It runs BEFORE the fills: a filled pixel gets mask 0 and would be taken for
    an own one.  `crop` framing has no padding: every pixel is own."""
    if sharp is None:
        return
    em = plan.estimated_motion
    meta["sharpness_transfer"] = sharpness_transfer_mod.transfer_on_device(
        ctx, device_frames, dst, None if plan.framing_mode == "crop" else mask, plan.final_matrices,
        np.asarray(em["matrices"], dtype=np.float32), em["confidences"], sharp[0], sharp[1])


def _plate(ctx, dst, mask, plan, min_count, segments):
    """-> (plate, count, sample table) of every shot, or None (clean_plate.py).  Formed from the frames as they stand behind the
    deflicker and the sharpness transfer, under the warp's TRUE mask, before any fill: a filled pixel gets mask 0 and would vote
    as an own one.  min_count: clean_plate.check_request's answer, None = off.  `crop` framing has no padding: nothing to do."""
    if min_count is None or plan.framing_mode == "crop":
        return None
    return clean_plate_mod.plate_on_device(ctx, dst, mask, segments)


def _plate_fill(ctx, dst, mask, meta, min_count, plate_state, segments) -> None:
    """Fills what is still padding behind the temporal fill from its shot's plate in place (clean_plate.py) and adds
    meta["plate_fill"]; a filled pixel's mask becomes 0 -- it was seen -- and the other meta keys keep describing the warp."""
    if plate_state is None:
        return
    plate, count, table = plate_state
    meta["plate_fill"] = clean_plate_mod.fill_and_report(ctx, dst, mask, plate, count, table, segments, min_count)


def _spatial_fill(ctx, dst, mask, plan, meta, enabled: bool) -> None:
    """Fills what is still padding from each frame's own valid pixels in place (spatial_fill.py), as the very last pass on
    the outputs, and adds meta["spatial_fill"]; the mask and the other meta keys are unchanged.  `crop` framing has no
    padding: nothing to do."""
    if not enabled or plan.framing_mode == "crop":
        return
    meta["spatial_fill"] = spatial_fill_mod.fill_on_device(ctx, dst, mask)


def _stability_report(ctx, device_frames, dst, mask, plan, meta, enabled: bool, segments=None) -> None:
    """Adds meta["stability"] (stability.py): the ITF of the source frames, without a mask, and of the outputs under their
    padding mask, measured behind every fill -- spatial fill leaves the mask as it is, so its invented pixels stay out.
    `crop` framing has no mask.  Pairs across a scene cut are in neither mean.  Reads only; the other meta keys are unchanged."""
    if not enabled:
        return
    cuts = None if segments is None else [s for s, _ in segments[1:]]
    meta["stability"] = stability_mod.report_on_device(ctx, device_frames, dst, None if plan.framing_mode == "crop" else mask, cuts)


def _mask_handoff(ctx, mask, plan, meta, request, segments=None):
    """-> the mask to return: held, grown and feathered for an outpainter (mask_handoff.py), with meta["mask_handoff"] added --
    or `mask` itself where nothing was asked for.  request: mask_handoff.check_request's answer.  It runs LAST, behind the
    sharpness transfer, the fills and the stability report, which all see the true mask; `padding_fraction_*` and every other
    block keep describing the warp.  `crop` framing has no mask: nothing to do."""
    if request is None or plan.framing_mode == "crop":
        return mask
    mask, meta["mask_handoff"] = mask_handoff_mod.handoff_on_device(ctx, mask, request, segments)
    return mask


# ---- estimation mask (beyond the reference; the rule is in include/vstab.h) --------------------------------------------
MASK_MARGIN_MAX = 64
_MASK_LIMITS = {
    "classic": "the Classic estimator fits tracked corners, not grid samples: it needs a masked corner detector, which does not exist yet.",
    "flow_phase_correlate": "phase correlation yields one global transform per pair: it has no samples to drop.",
    "subject": "the subject lock follows a mask's centroid: it has no camera-motion fit to keep a subject out of.",
}


def check_estimation_mask_request(estimator: str, mask_margin) -> int:
    """The checks of an estimation-mask request that need neither the clip nor a GPU -> the margin as an int."""
    margin = int(mask_margin)
    if not 0 <= margin <= MASK_MARGIN_MAX:
        raise ValueError(f"mask_margin={margin} outside [0, {MASK_MARGIN_MAX}] (working pixels)")
    if estimator in _MASK_LIMITS:
        raise ValueError(f"estimation_mask is not supported with estimator {estimator!r}: {_MASK_LIMITS[estimator]}")
    return margin


def check_estimation_mask_shape(estimation_mask, total_frames: int, size) -> None:
    """[N,H,W], [1,H,W] or [H,W] at the frames' full resolution, else a ValueError naming both shapes."""
    width, height = size
    shape = tuple(int(v) for v in estimation_mask.shape)
    ok = (shape == (height, width)) or (len(shape) == 3 and shape[1:] == (height, width) and shape[0] in (1, total_frames))
    if not ok:
        raise ValueError(f"estimation_mask of shape {shape} does not match the clip [{total_frames},{height},{width}]: expected "
                         f"[{total_frames},{height},{width}], [1,{height},{width}] or [{height},{width}]")


def _block_grid(ctx, estimation_mask, total_frames, working_size, margin):
    """The mask on the device (a float32 host tensor goes through the pinned ring) -> block grid u8 [N,gh,gw]."""
    torch = ctx.torch
    mask = estimation_mask if isinstance(estimation_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(estimation_mask, dtype=np.float32))
    if mask.device.type == "cpu" and mask.dtype == torch.float32:
        mask = ctx.upload(mask)
    return ctx.mask_block_grid(mask, total_frames, working_size, SAMPLE_STEP, margin), 1 if mask.dim() == 2 else int(mask.shape[0])


def estimation_mask_meta(fit_records, margin: int, mask_frames: int, grid_samples: int) -> Dict[str, Any]:
    """meta["estimation_mask"] from the fits' own counts (total_points = admitted samples of the pair)."""
    admitted = np.asarray(fit_records["total_points"][:, 0], dtype=np.int64)
    fraction = (grid_samples - admitted) / float(grid_samples)
    return {"margin": int(margin), "mask_frames": int(mask_frames), "blocked_fraction_mean": float(fraction.mean()),
            "blocked_fraction_max": float(fraction.max()), "admitted_points_min": int(admitted.min())}


# ---- scene cuts (beyond the reference; scene_cuts.py, the rule is in include/vstab.h) -----------------------------------
def _scene_segments(ctx, scene, fit_records, gray_out, transform_mode: str, total_frames: int):
    """-> (segments [s, e) of frames, meta["scene_cuts"]).  "auto": one launch of the residual kernel over the estimation
    images the estimator made, scored with each pair's own best candidate; "given": the caller's edit list."""
    if scene.mode == "given":
        return scene_cuts_mod.segments_from_cuts(scene.cuts, total_frames), scene_cuts_mod.meta_block(scene, scene.cuts)
    gray = gray_out[0]
    sum_abs, inside = ctx.pair_residual_batch(gray, scene_cuts_mod.scoring_transitions(fit_records, transform_mode))
    scores, overlap = scene_cuts_mod.scores_and_overlap(sum_abs, inside, int(gray.shape[1]), int(gray.shape[2]))
    cuts = scene_cuts_mod.cuts_from_pairs(scene_cuts_mod.is_cut(scores, overlap, scene.threshold))
    return scene_cuts_mod.segments_from_cuts(cuts, total_frames), scene_cuts_mod.meta_block(scene, cuts, scores, overlap)


# ---- mesh warp (beyond the reference; mesh_warp.py, the rules are in include/vstab.h) -----------------------------------
def _mesh_offsets(ctx, mesh, plan, grid, blocked, working_size, size, segments, args):
    """-> (the warp's vertex offsets f32 [N,mh,mw,2] in full-resolution px, meta["mesh_warp"]).  One launch of the residual
    kernel over the grid the estimator made, against the working-resolution transitions the plan itself used; the vertex
    paths go through the trajectory routine with the plan's own (clipped) smooth / strength.  args: the call's FlowArgs."""
    width, height = size
    work = working_size if working_size is not None else size
    mw, mh = mesh.vertices
    em = plan.estimated_motion
    residual, count = ctx.mesh_residual_batch(grid, SAMPLE_STEP, work, em["work_matrices"], mw, mh, blocked=blocked)
    residual, count = residual.cpu().numpy(), count.cpu().numpy()
    max_shift = mesh.max_shift_px(width)
    offsets, _ = mesh_warp_mod.plan_offsets(
        ctx.trajectory, residual, em["confidences"], segments, float(np.clip(args.smooth, 0.0, 1.0)), args.fps_effective,
        float(np.clip(args.strength, 0.0, 1.0)), bool(args.camera_lock), (1.0 / (work[0] / float(width)), 1.0 / (work[1] / float(height))), max_shift)   # the plan's own up-scale factors
    return offsets, mesh_warp_mod.meta_block(mesh, max_shift, residual, count, offsets, native.MESH_MIN_SAMPLES)


# ---- rolling shutter (beyond the reference; rolling_shutter.py, the rules are in include/vstab.h) -----------------------
def _rolling_shutter(ctx, rolling, plan, grid_out, blocked, working_size, size, segments, refit=None):
    """-> (the plan, the warp's per-frame velocities f64 [N,6] in full-resolution px per frame, the readout,
    meta["rolling_shutter"], the fit table of the refit or None).
    A given readout launches nothing here.  "auto": one launch of the row-residual kernel over the grid the estimator made,
    against the working-resolution transitions the plan itself used, then the least-squares readout on the host.
    refit (rolling_refit; None: off, and the plan comes back as it went in): plan -> the plan formed again on a fit table.  The
    readout is the first pass's either way; with a readout other than 0 the flow samples are corrected for it with the first
    plan's working-resolution velocities (one launch of the rectifier), the pairs are fitted again on them (one launch of the
    point fit) and the velocities of the warp and of the meta are the second plan's."""
    em = plan.estimated_motion
    work = working_size if working_size is not None else size
    estimate = None
    if rolling == rolling_shutter_mod.AUTO:
        residual, count = ctx.row_residual_batch(grid_out[0], SAMPLE_STEP, work, em["work_matrices"], blocked=blocked)
        estimate = rolling_shutter_mod.estimate_readout(residual.cpu().numpy(), count.cpu().numpy(), em["work_matrices"],
                                                        em["confidences"], em["modes"], segments, work, SAMPLE_STEP)
        readout, source = estimate["readout"], estimate["source"]
    else:
        readout, source = float(rolling), "given"
    table = refit_block = None
    if refit is not None and readout == 0.0:          # "not_observable": nothing to correct for, nothing is launched
        refit_block = rolling_shutter_mod.refit_block(0)
    elif refit is not None:
        work_velocity = rolling_shutter_mod.velocities(em["work_matrices"], em["confidences"], segments)
        point_pairs, counts, unsolved = ctx.rectify_samples_batch(grid_out[0], SAMPLE_STEP, work, work_velocity, readout, blocked=blocked)
        table = ctx.points_fit_batch(point_pairs, counts, plan.meta_head["transform_mode_requested"])
        first, plan = em["matrices"], refit(table)
        em = plan.estimated_motion
        refit_block = rolling_shutter_mod.refit_block(1, first, em["matrices"], em["confidences"], segments, unsolved.cpu().numpy(), size)
    velocity = rolling_shutter_mod.velocities(em["matrices"], em["confidences"], segments)
    block = rolling_shutter_mod.meta_block(readout, source, estimate, velocity, size)
    if refit_block is not None:
        block["refit"] = refit_block
    return plan, velocity, readout, block, table


# ---- drift correction (beyond the reference; drift_correction.py, the rule is in include/vstab.h) ------------------------
def _drift_correction(ctx, spacing, fit_records, gray, segments, total_frames, transform_mode, size, working_size,
                      exposure=False, blocked=None):
    """-> (the fit table with the registered poses' transitions, the path's per-pair steps, meta["drift_correction"]).  Runs
    on the selection the plan itself will make; every launch covers all frames of the clip that are still iterating.
    exposure (drift_exposure) or blocked (drift_mask: the estimation mask's block grid) switch to the second form of the rule;
    without them the first entry point is the one called."""
    table = fit_records if isinstance(fit_records, np.ndarray) else native.fit_table_from_dicts(fit_records)
    if segments is None:
        selection = select_transitions(table, transform_mode)
    else:
        selection = _select_per_segment(table, transform_mode, segments)

    second_form = exposure or blocked is not None

    def sums_fn(anchor, R, gain=None, offset=None, cap=drift_correction_mod.RESIDUAL_CAP):
        if second_form:
            return ctx.anchor_sums_ex_batch(gray, anchor, R, cap, gain, offset, blocked, SAMPLE_STEP)
        return ctx.anchor_sums_batch(gray, anchor, R, cap)       # the faster kernel

    return drift_correction_mod.correct(sums_fn, table, selection, segments, total_frames, transform_mode, size, working_size, spacing,
                                        exposure=exposure, masked=blocked is not None)


# ---- dynamic zoom (beyond the reference; dynamic_zoom.py, the rule is in include/vstab.h) -------------------------------
def _dynamic_zoom(ctx, zoom, plan, offsets, segments):
    """-> (the plan with its final matrices zoomed, meta["dynamic_zoom"] still without the warp's counts).  One launch of the
    coverage-extent kernel over the plan's final matrices -- and the mesh warp's vertex offsets, where there are any -- then
    the envelope on the host, per shot under scene cuts; Z @ final in float32, like the other framing shifts."""
    extent = ctx.cover_extent_batch(plan.final_matrices, plan.source_size, plan.output_size, offsets)
    Z, block = dynamic_zoom_mod.plan_zoom(zoom, extent, plan.output_size, plan.fps_effective, segments)
    return replace(plan, final_matrices=np.matmul(Z, np.asarray(plan.final_matrices, dtype=np.float32))), block


# ---- horizon level (beyond the reference; horizon_level.py, the rule is in include/vstab.h) -----------------------------
def _horizon_level(ctx, level, plan, gray, segments):
    """-> (the plan with its final matrices levelled, meta["horizon_level"]).  One launch of the orientation histogram over
    the estimation images the estimator made, then on the host: every frame's roll, the chain's roll from the plan's own
    full-resolution transitions, one offset per shot (or a slowly varying one); L @ final in float32, like the zoom.  A clip
    on which no frame is corrected (not observable) keeps its plan as it is."""
    hist = ctx.orientation_hist_batch(gray, horizon_level_mod.MIN_MAG2).cpu().numpy()
    em = plan.estimated_motion
    L, block = horizon_level_mod.plan_level(level, hist, em["matrices"], em["confidences"], plan.final_matrices, plan.output_size,
                                            plan.fps_effective, segments)
    if L is None:
        return plan, block
    return replace(plan, final_matrices=np.matmul(L, np.asarray(plan.final_matrices, dtype=np.float32))), block


# ---- the driver: one validated request, one record of the reference's arguments, one post-warp tail ----------------------
@dataclass(frozen=True)
class FlowRequest:
    """The keyword extras of one `_stabilize_frames` call, checked: every field is what its feature's check returned, and
    the object existing means the requests are valid and compatible with each other, with the framing and with the
    transform mode.  It carries no tensor and no per-call state (masks, clip, context travel beside it).  What each keyword
    means is in `_stabilize_frames`' docstring."""

    estimator: str                     # resolved (resolve_flow_backend)
    temporal_fill: int                 # radius, 0 = off
    fill_blend: Tuple[Optional[int], bool]   # temporal_fill.check_blend_request: (feather px | None, exposure)
    sharpness: Optional[Tuple[int, float]]   # sharpness_transfer.check_request: (radius, alpha) | None
    handoff: Any                       # mask_handoff.check_request: Request | None
    zoom: Any                          # dynamic_zoom.check_request | None
    scene: Any                         # scene_cuts.check_request | None
    mesh: Any                          # mesh_warp.check_request | None
    mesh_motion: bool
    subject: bool                      # the estimator is the subject lock (its mask travels beside the request)
    rolling: Any                       # rolling_shutter.check_request: readout | AUTO | None
    spatial_fill: bool
    stability_report: bool
    mask_margin: Optional[int]         # the estimation mask's margin; None: no estimation mask was given
    drift: Optional[int] = None        # drift_correction.check_request: the keyframe spacing | None
    drift_exposure: bool = False       # drift_correction.check_options: the keyframe alignment estimates a gain and an offset
    drift_mask: bool = False           # ... and leaves out what the estimation mask's block grid names
    deflicker: Any = None              # deflicker.check_request: Request | None
    level: Any = None                  # horizon_level.check_request: Request | None
    plate: Optional[int] = None        # clean_plate.check_request: the plate fill's min_count | None
    track: Any = None                  # template_track.check_request: (box, key, radius) | None
    refit: bool = False                # rolling_shutter.check_refit_request: the transitions are fitted again on rectified samples

    @property
    def needs_host_plan(self) -> bool:
        """Scene-aware calls form the plan on the host: plan_kernel knows one continuous camera move; so do mesh-warp calls:
        the vertex paths need the plan's own transitions before the warp can be queued; and dynamic-zoom calls: the zoom is
        formed from the plan's final matrices before the warp can be queued; and rolling-shutter calls: the velocities come
        from the plan's transitions before the warp can be queued; and drift-corrected calls: the keyframe alignment rewrites
        the transitions before there is a plan; and levelled calls: the roll is measured and the final matrices are turned
        before the warp can be queued."""
        return not (self.scene is None and self.mesh is None and self.zoom is None and self.rolling is None and self.drift is None
                    and self.level is None)

    @property
    def kept_by_products(self) -> Tuple[str, ...]:
        """The estimator's by-products that stay alive behind the fits (its `*_out` keywords): the estimation images for the
        scene-cut score, the keyframe alignment and the horizon level's histogram, the grid of flow samples for the vertex /
        row residuals.  (The estimation mask's block grid, which drift_mask reads behind the fits, is made before the estimator
        runs and is held by the call itself for all of its length: it is no by-product and needs no entry here.)"""
        auto_cuts = self.scene is not None and self.scene.mode == "auto"
        keep = ("gray_out",) if auto_cuts or self.drift is not None or self.level is not None else ()
        return keep + (("grid_out",) if self.mesh is not None or self.rolling == rolling_shutter_mod.AUTO or self.refit else ())


def check_flow_request(framing_mode: str, transform_mode: str, estimator: str, kw: Dict[str, Any]) -> FlowRequest:
    """Every check of `_stabilize_frames`' keyword extras `kw` (by name) that needs neither the clip nor a GPU, in one fixed
    order: a call that is wrong in several ways always raises the same message (tests/test_flow_request_cpu.py)."""
    handoff = mask_handoff_mod.check_request(kw["mask_grow"], kw["mask_feather"], kw["mask_hold"], kw["mask_tapered"])
    zoom = dynamic_zoom_mod.check_request(kw["dynamic_zoom"], kw["zoom_limit"])
    if zoom is not None:
        dynamic_zoom_mod.check_pipeline(framing_mode)
    spatial_fill = spatial_fill_mod.check_request(kw["spatial_fill"])
    stability_report = stability_mod.check_request(kw["stability_report"])
    scene = scene_cuts_mod.check_request(kw["scene_cuts"], kw["cut_threshold"])
    mesh = mesh_warp_mod.check_request(kw["mesh_warp"], kw["mesh_max_shift"])
    if kw["mesh_motion"] and mesh is None:
        raise ValueError("mesh_motion=True needs mesh_warp: without a mesh warp there are no per-vertex offsets to record.")
    if estimator not in _META_SOURCE:
        raise ValueError(f"Unknown estimator {estimator!r}; expected 'flow' or 'classic'.")
    subject = subject_lock_mod.check_request(kw["subject_mask"], transform_mode, estimator)
    track = template_track_mod.check_request(kw.get("track_box"), kw.get("track_key", 0), kw.get("track_radius"), estimator,
                                             transform_mode)
    temporal_fill = int(kw["temporal_fill"])
    if not 0 <= temporal_fill <= temporal_fill_mod.MAX_RADIUS:
        raise ValueError(f"temporal_fill={temporal_fill} outside [0, {temporal_fill_mod.MAX_RADIUS}]")
    fill_blend = temporal_fill_mod.check_blend_request(temporal_fill, kw["fill_feather"], kw["fill_exposure"])
    sharpness = sharpness_transfer_mod.check_request(kw["sharpness_transfer"], kw["sharpness_alpha"])
    if sharpness is not None:
        sharpness_transfer_mod.check_pipeline(estimator, mesh)
    estimator = resolve_flow_backend(estimator)
    mask_margin = None
    if kw["estimation_mask"] is not None:
        mask_margin = check_estimation_mask_request(estimator, kw["mask_margin"])
    if mesh is not None:
        mesh_warp_mod.check_pipeline(estimator, framing_mode, temporal_fill)
    if subject:
        subject_lock_mod.check_pipeline(temporal_fill, scene, kw["estimation_mask"])
    rolling = rolling_shutter_mod.check_request(kw["rolling_shutter"])
    if rolling is not None:
        rolling_shutter_mod.check_pipeline(rolling, transform_mode, framing_mode, estimator, mesh, temporal_fill, sharpness, zoom)
    drift = drift_correction_mod.check_request(kw["drift_correction"])
    if drift is not None:   # (drift_mask=True lifts the estimation_mask refusal; whether the keyword is well-formed comes next)
        drift_correction_mod.check_pipeline(transform_mode, bool(subject), kw["estimation_mask"], kw.get("drift_mask") is True)
    drift_exposure, drift_mask = drift_correction_mod.check_options(drift, kw.get("drift_exposure"), kw.get("drift_mask"),
                                                                    kw["estimation_mask"])
    refit = rolling_shutter_mod.check_refit_request(kw.get("rolling_refit"), rolling, estimator, drift)
    deflicker = deflicker_mod.check_request(kw.get("deflicker"), kw.get("deflicker_mode"))
    if deflicker is not None:
        deflicker_mod.check_pipeline(estimator, temporal_fill, fill_blend[1], sharpness)
    level = horizon_level_mod.check_request(kw.get("horizon_level"), kw.get("horizon_limit"))
    if level is not None:
        horizon_level_mod.check_pipeline(framing_mode, transform_mode, estimator, rolling)
    plate = clean_plate_mod.check_request(kw.get("plate_fill"))
    if plate is not None:
        clean_plate_mod.check_pipeline(kw.get("camera_lock"), kw.get("strength"), estimator, zoom, level)
    if track is not None:   # (behind every keyword's own check: a malformed value keeps its own message)
        template_track_mod.check_pipeline({
            "scene_cuts": scene, "estimation_mask": kw["estimation_mask"], "mesh_warp": mesh, "temporal_fill": temporal_fill,
            "sharpness_transfer": sharpness, "rolling_shutter": rolling, "drift_correction": drift, "deflicker": deflicker,
            "horizon_level": level, "plate_fill": plate})
    return FlowRequest(estimator, temporal_fill, fill_blend, sharpness, handoff, zoom, scene, mesh, bool(kw["mesh_motion"]),
                       bool(subject), rolling, spatial_fill, stability_report, mask_margin, drift, drift_exposure, drift_mask,
                       refit=refit, deflicker=deflicker, level=level, plate=plate, track=track)


def _check_request_against_clip(request: FlowRequest, kw: Dict[str, Any], transform_mode: str, total_frames: int, size) -> None:
    """The four checks that need the clip's length and size, run as soon as they are known."""
    if kw["estimation_mask"] is not None:
        check_estimation_mask_shape(kw["estimation_mask"], total_frames, size)
    if request.scene is not None and request.scene.mode == "given":
        scene_cuts_mod.check_given_cuts(request.scene.cuts, total_frames)
    if request.subject:
        subject_lock_mod.check_request(kw["subject_mask"], transform_mode, request.estimator, total_frames, size)
    if request.track is not None:
        box, key, _ = request.track
        template_track_mod.check_against_clip(box, key, total_frames, size)
        template_track_mod.working_box(box, size, hm._working_estimation_size(*size) or size)


class FlowArgs(NamedTuple):
    """The reference's arguments of one call behind the clip, in the order plan_stabilization takes them (`*args`)."""

    framing_mode: str
    transform_mode: str
    camera_lock: bool
    strength: float
    smooth: float
    keep_fov: float
    padding_rgb: Tuple[int, int, int]
    fps_effective: float
    fps_requested: Optional[float]


def _finish(ctx, request: FlowRequest, plan, device_frames, dst, mask, meta, segments, keep_on_device: bool, verdict):
    """Everything behind the warp, for either plan path: the six post-warp passes, then the result on the device or the host.
    The ORDER is a correctness rule.  The deflicker runs first: it scales a frame's OWN pixels (padding keeps its colour), so it
    has to see the warp's mask before a fill clears it, and the passes behind it -- the exposure match of the blended fill, the
    fills themselves, the stability report -- then work on deflickered frames (the sharpness transfer and a hard temporal
    fill, which would bring uncorrected neighbour pixels in, are refused with it).  The sharpness transfer runs before the
    fills: a filled pixel gets mask 0 and would be taken for an own one.  The clean plate is formed before any fill, for the same
    reason, and fills between the two: seen nearby in time (temporal fill), then seen anywhere in the shot (plate fill), then
    invented (spatial fill).  The stability report
    measures behind every fill; the spatial fill leaves the mask as it is, so its invented pixels stay out of it.  The mask
    hand-off runs last, so that every other pass has seen the true mask; it replaces only the mask that is returned.  Each
    pass adds its own meta block, in this order, and nothing else in the meta changes.
    segments: the shots under scene cuts, None for one continuous camera move (always on the device-plan path)."""
    _deflicker(ctx, device_frames, dst, mask, plan, meta, request.deflicker, segments)
    _sharpness_transfer(ctx, device_frames, dst, mask, plan, meta, request.sharpness)
    plate_state = _plate(ctx, dst, mask, plan, request.plate, segments)
    _temporal_fill(ctx, device_frames, dst, mask, plan, meta, request.temporal_fill, request.fill_blend)
    _plate_fill(ctx, dst, mask, meta, request.plate, plate_state, segments)
    _spatial_fill(ctx, dst, mask, plan, meta, request.spatial_fill)
    _stability_report(ctx, device_frames, dst, mask, plan, meta, request.stability_report, segments)
    mask = _mask_handoff(ctx, mask, plan, meta, request.handoff, segments)
    check_interrupt()
    if keep_on_device:
        return hm.StabilizationResult(dst, mask.unsqueeze(-1), meta, verdict)
    return hm.StabilizationResult(dst.cpu().numpy(), mask.cpu().numpy()[..., np.newaxis], meta, verdict)


def _stabilize_with_device_plan(ctx, context, device_frames, request: FlowRequest, args: FlowArgs, pbar, keep_on_device: bool,
                                blocked=None, mask_info=None):
    """F2-F14 with the plan formed on the device (see above).  Returns None when F0 found 0..255 float data: the
    speculative run used the unscaled frames and is discarded; the caller takes the regular path on the rescaled clip.
    Only for requests that do not need the host plan: there are no shots here, one continuous camera move."""
    size = (context.width, context.height)
    total_frames = len(context.frames)
    progress_total = (total_frames - 1) + total_frames
    working_size = hm._working_estimation_size(context.width, context.height)
    framing_mode, transform_mode, padding_rgb = args.framing_mode, args.transform_mode, args.padding_rgb
    peaks = [] if context.range_pending else None
    gray = _gray(ctx, device_frames, working_size, peaks)
    _, grid = ctx.dis_flow_batch(gray, sample_step=SAMPLE_STEP, want_full=False, want_grid=True)
    pairs = ctx.sample_fit_batch_begin(grid, SAMPLE_STEP, transform_mode, blocked=blocked)
    ctx.flow_plan_device(ctx.fit_records_device(), pairs, transform_mode, size, working_size, args.smooth, args.fps_effective,
                         args.strength, bool(args.camera_lock), warp_frames=total_frames, framing=framing_mode)
    out_size = size
    if framing_mode == "expand":
        # the canvas has to exist before the warp is queued: wait for the plan kernel's region (the plan's download, ~30 us
        # behind the fit kernel on the side stream -- not for the host's own plan, which runs under the warp as before)
        out_size = ctx.expand_canvas(ctx.flow_plan_result(total_frames, PLAN_PARAMS[transform_mode])[3])
        if out_size is None:           # a non-finite region: nothing to speculate on
            ctx.sample_fit_batch_end(pairs)
            return None
    dst, mask, counts = ctx.warp_batch_planned(device_frames, 0, out_size, border=hm.border_value(padding_rgb), want_mask=True,
                                               want_count=True)
    fit_records = ctx.sample_fit_batch_end(pairs)          # waits for the fits only; the plan kernel and the warp run on
    if peaks and hm.resolve_value_range(context, peaks[0], ctx):
        return None
    progress_done = _replay_progress(pbar, 0, total_frames - 1, progress_total)
    check_interrupt()
    plan = plan_stabilization(ctx, fit_records, size, total_frames, *args, estimator="flow")
    meta = prepare_meta(plan)                               # host JSON work overlaps the warp kernel
    final_dev = ctx.flow_plan_result(total_frames, PLAN_PARAMS[transform_mode])[0]
    if tuple(plan.output_size) != tuple(out_size):
        # expand: the host's canvas is a pixel wider / taller than the device's (an extent within one ulp of an integer): every
        # frame is warped again onto the host plan's canvas
        dst, mask, counts = ctx.warp_batch(device_frames, plan.final_matrices, plan.output_size, interp="bilinear",
                                           border=hm.border_value(padding_rgb), want_mask=True, want_count=True)
        verdict = {"used": True, "mismatched_frames": total_frames}
        mirror_ok = True               # (the counts of that one warp of all frames are what the library mirrored last)
    else:
        verdict = {"used": True, "mismatched_frames": _rewarp_mismatched(ctx, device_frames, plan, final_dev, dst, mask, counts, padding_rgb)}
        mirror_ok = verdict["mismatched_frames"] == 0
    _replay_progress(pbar, progress_done, total_frames, progress_total)   # (host work that needs no pixel: before the last wait)
    # the warp's counts: mirrored to the host behind the kernel (native.last_pad_counts) -- unless frames were warped again,
    # whose counts went into the device tensor only
    meta = complete_meta(meta, plan, _counts_to_host(counts, mirrored=mirror_ok))
    if mask_info is not None:
        meta["estimation_mask"] = estimation_mask_meta(fit_records, *mask_info)
    # the passes run on the host plan's verified matrices
    return _finish(ctx, request, plan, device_frames, dst, mask, meta, None, keep_on_device, verdict)


def _stabilize_frames(
    context: hm.VideoContext,
    framing_mode: str,
    transform_mode: str,
    camera_lock: bool,
    strength: float,
    smooth: float,
    keep_fov: float,
    padding_rgb: Tuple[int, int, int],
    frame_rate: float,
    *,
    ctx: Optional[native.Context] = None,
    keep_on_device: bool = False,
    estimator: str = "flow",
    temporal_fill: int = 0,
    estimation_mask=None,
    mask_margin: int = 16,
    scene_cuts=None,
    cut_threshold=None,
    mesh_warp=None,
    mesh_max_shift=None,
    mesh_motion: bool = False,
    spatial_fill: bool = False,
    stability_report: bool = False,
    dynamic_zoom=None,
    zoom_limit=None,
    subject_mask=None,
    fill_feather=None,
    fill_exposure: bool = False,
    sharpness_transfer=None,
    sharpness_alpha=None,
    mask_grow=None,
    mask_feather=None,
    mask_hold=None,
    mask_tapered=None,
    rolling_shutter=None,
    rolling_refit=None,
    deflicker=None,
    deflicker_mode=None,
    horizon_level=None,
    horizon_limit=None,
    plate_fill=None,
    track_box=None,
    track_key: int = 0,
    track_radius=None,
    drift_correction=None,
    drift_exposure=None,
    drift_mask=None,
) -> hm.StabilizationResult:
    """Positional signature of the reference (flow.py:213-223); keyword-only extras select the GPU
    context, keep outputs resident in HBM (multi-GPU sharding lives in distributed.py) or switch the
    motion estimator to the Classic node's sparse tracker (classic.py:163-173, same signature).
    temporal_fill = R > 0 (beyond the reference, off by default): after the final warp the padded pixels are filled from
    the up to R frames before and after that saw them (temporal_fill.py); `padding_mask` keeps what no frame saw and
    meta["temporal_fill"] describes the fill.  0: the reference's behaviour and meta.  Bypass paths ignore it.
    estimation_mask (beyond the reference, None by default): [N,H,W], [1,H,W] or [H,W] float at the frames' resolution, > 0.5
    or not finite where a moving subject (or a burnt-in logo) is; the DIS / TV-L1 flow samples within mask_margin working
    pixels of it in either frame of a pair stay out of that pair's fit (include/vstab.h states the rule) and
    meta["estimation_mask"] reports how many.  None: the reference's behaviour and meta.  Bypass paths ignore it.
    scene_cuts (beyond the reference, None by default): "auto" finds the hard cuts of the clip from the motion-compensated
    residual of every pair (scene_cuts.py; include/vstab.h states the rule; cut_threshold None: the calibrated default), a
    strictly increasing sequence of frame indices in 1..N-1 names the first frames of the shots instead.  Mode selection
    and trajectory then run per shot, the transition across a cut is reported as "no candidate", framing stays global and
    meta["scene_cuts"] reports cuts and scores.  None: the reference's behaviour and meta.  Bypass paths ignore it.
    mesh_warp (beyond the reference, None by default): True (16 x 9 cells) or a (cols, rows) pair, each in 2..64.  The
    residual of the pairs' global fits is measured per mesh vertex from the flow grid (mesh_warp.py; include/vstab.h states
    the rules), its vertex paths are smoothed as the global path is, and the final warp displaces the source by the
    per-vertex correction, clamped to mesh_max_shift full-resolution px per axis (None: 1/64 of the width).  For the DIS and
    TV-L1 estimators under crop_and_pad / expand framing, without temporal_fill; meta["mesh_warp"] reports residuals and
    corrections, motion_meta keeps describing the global part.  None: the reference's behaviour and meta.  Bypass paths
    ignore it.
    mesh_motion (with mesh_warp only, False by default): True adds the per-vertex offsets themselves as
    meta["mesh_warp"]["motion"] (mesh_warp.motion_block), which is what Motion Apply's mesh=True replays or undoes.  False:
    the meta without it, byte for byte.
    spatial_fill (beyond the reference, False by default): True fills the pixels that are still padding after the warp (plain
    or mesh) and after temporal_fill from each frame's own valid pixels by pyramid push-pull (spatial_fill.py; include/vstab.h
    states the rule), as the very last pass.  `padding_mask` and `padding_fraction_*` keep describing the warp -- the pixels
    are invented, not seen -- and meta["spatial_fill"] describes the fill.  False: the behaviour and meta without it, byte
    for byte, and nothing is launched.  `crop` framing has no padding; bypass paths ignore it.
    stability_report (beyond the reference, False by default): True adds meta["stability"], the inter-frame transformation
    fidelity (mean PSNR between consecutive frames over the pixels both show; stability.py, include/vstab.h states the rule)
    of the source frames and of the returned frames under the returned mask, behind every fill, and their difference
    gain_db; pairs across a scene cut are left out and counted.  Frames, mask and every other meta key are unchanged.
    False: the meta without it, byte for byte, and nothing is launched.  Bypass paths ignore it.
    dynamic_zoom (beyond the reference, None by default): True (a window of 2 s) or a window in seconds in (0, 60].  Every
    frame is zoomed about the canvas centre just enough to hide its own border: the coverage extent of the plan's final
    matrices (and of the mesh offsets, under mesh_warp) is measured per output pixel with the warp's own arithmetic
    (dynamic_zoom.py; include/vstab.h states the rule), the zoom each frame needs goes through a sliding maximum and a box
    mean over the window -- per shot under scene_cuts -- and is capped at zoom_limit (None: 2.0, else in [1, 16]); the
    plan's final matrices are replaced by the zoomed ones and the warp runs unchanged.  For crop_and_pad framing only;
    meta["dynamic_zoom"] reports the zoom per frame, stabilization_warp / motion_meta hold the zoomed matrices.  None: the
    behaviour and meta without it, byte for byte, and nothing is launched.  Bypass paths ignore it.
    subject_mask (beyond the reference, None by default; with estimator="subject" only, and required by it): [N,H,W] float
    at the frames' resolution, > 0.5 where the subject is (a NaN is not subject).  The transitions are then the subject's, not
    the camera's: count, coordinate sums and bounding box of every mask come from one reduction (subject_lock.py;
    include/vstab.h states the rule), translation follows the centroid, similarity also the square root of the area ratio,
    frames without a subject are interpolated and reported with confidence 0.  Everything behind the fit table is unchanged:
    camera_lock=True pins the subject where frame 0 shows it.  For translation / similarity, without temporal_fill,
    estimation_mask, mesh_warp or scene_cuts="auto"; meta["subject_lock"] reports centroids and gaps.  None: the behaviour and
    meta without it, byte for byte, and nothing is launched.  Bypass paths ignore it.
    fill_feather, fill_exposure (beyond the reference, None / False by default; with temporal_fill > 0 only): how the temporal
    fill writes its pixels (temporal_fill.py; include/vstab.h states both rules).  fill_exposure=True scales what a neighbour
    supplies by one gain per channel, the ratio of the two frames' sums over the lattice of pixels both see, so a clip shot
    with auto exposure leaves no brightness step at the filled border.  fill_feather = True (16 px) or an int in 0..64
    cross-fades the frame's own pixels within that many source pixels of its border into the neighbour's, which also
    replaces the ring of own pixels the padding colour was interpolated into.  Each works without the other;
    meta["temporal_fill"] gains feather_px, blended_fraction_* and exposure.  Not in sub-pixel mode 'exact'.  None / False:
    the behaviour and meta without them, byte for byte, and nothing new is launched.  `crop` framing and bypass paths
    ignore them.
    sharpness_transfer = R in 1..16, sharpness_alpha (beyond the reference, None by default): after the final warp and before
    any fill, the own pixels of a frame that a camera jolt blurred are pulled towards what the up to R frames before and
    after show there (sharpness_transfer.py; include/vstab.h states both rules).  Every source frame's gradient energy is
    measured as one exact integer; frame i borrows from neighbour j only where E_j / E_i >= 1.1, each sample weighted by
    ratio / (ratio + alpha * D), D the L1 colour distance to the pixel (sharpness_alpha None: 16.0, else in [0, 1024]), the
    pixel itself with weight 1.  Frames with no sharper neighbour, the mask and every other meta key are unchanged, bit for
    bit; meta["sharpness_transfer"] lists every frame's sharpness and what was transferred.  Not with mesh_warp, estimator
    "subject" or sub-pixel mode 'exact'.  0 / None / False: the behaviour and meta without it, byte for byte, and nothing new
    is launched.  Bypass paths ignore it.
    mask_grow, mask_feather, mask_hold, mask_tapered (beyond the reference, None by default): the hand-off of `padding_mask` to
    a generative outpainter (mask_handoff.py; include/vstab.h states the rules).  mask_hold = T in 0..16 takes the maximum of
    the mask over the frames within T of each frame, inside its shot under scene_cuts, so the repaint region stands still;
    mask_grow = g in -64..64 is ComfyUI's GrowMask (negative erodes), over the L1 ball (mask_tapered None / True: GrowMask's
    tapered corners) or the square one (False); mask_feather = f in 0..64 adds an outward linear ramp of f pixels.  Any of the
    first three switches the pass on, the others read as 0.  It runs last and replaces only the returned mask: the fills,
    the sharpness transfer and the stability report see the true mask, frames and every other meta key are unchanged, and
    meta["mask_handoff"] reports the request and the fraction of pixels above 0.5.  All None: the behaviour and meta without
    it, byte for byte, and nothing new is launched.  `crop` framing has no mask; bypass paths ignore them.
    rolling_shutter (beyond the reference, None by default): the readout time of the sensor as a fraction of the frame interval,
    a finite number in [-1, 1] (negative: read out bottom to top), or "auto" to estimate it.  A sensor read out row by row
    shears and bends every frame with the camera's velocity; the final warp then samples every source row where that readout
    showed it (rolling_shutter.py; include/vstab.h states both rules): the per-frame image velocity comes from the plan's own
    full-resolution transitions, and "auto" fits the one number to the per-row medians of the global fits' residuals over the
    flow grid (DIS / TV-L1 only), reporting "not_observable" and correcting nothing on a clip without acceleration.  For
    translation / similarity under crop_and_pad / expand, without mesh_warp, temporal_fill, sharpness_transfer, dynamic_zoom or
    estimator "subject"; everything behind the final warp follows unchanged.  meta["rolling_shutter"] reports the readout, the
    skew it amounts to and every frame's velocity.  None / 0: the behaviour and meta without it, byte for byte, and nothing new
    is launched.  Bypass paths ignore it.
    rolling_refit (beyond the reference, None by default; with rolling_shutter only): True fits the pair transitions again on
    flow samples that have been corrected for the readout.  The row correction acts on the final warp; the transitions in front
    of it were fitted on sheared samples, and a similarity fit takes part of the shear for rotation and scale.  Between the
    first plan and the final one, both ends of every admitted flow sample are rectified with the first pass's per-frame
    velocities at working resolution (include/vstab.h states the rule), the pairs are fitted again on them by the point fit,
    and the plan -- sticky modes included -- is formed again on that table; the readout ("auto": estimated on the first
    pass) is unchanged, the warp's velocities and the meta's are the second plan's, so Motion Apply's rolling=True replays and
    undoes the run as before.  One pass; a readout of 0 ("not_observable") launches nothing.  For the DIS and TV-L1 estimators,
    without drift_correction; meta["rolling_shutter"]["refit"] reports passes, pairs_refit, samples_unsolved_max and how far
    the transitions moved.  None / False: the behaviour and meta without it, byte for byte, and nothing new is launched.
    drift_correction (beyond the reference, None by default): True (a keyframe every 32 frames) or the keyframe spacing, an int
    in 2..4096.  Every estimator measures consecutive pairs, and the bias of a pair adds up along the chain: a locked picture
    creeps.  With the keyword every frame is registered directly against the latest keyframe before it, and every keyframe
    against the previous one, by Gauss-Newton on the estimation images (drift_correction.py; include/vstab.h states the rule
    of its sums), starting from the chained estimate; the transitions the plan reads are those of the registered poses, and
    the path is the poses' own parameter vector instead of the sum of the pairs', so that camera_lock at strength 1 applies
    the inverse pose exactly.  A frame whose alignment cannot be trusted keeps its chained estimate, counted by reason in
    meta["drift_correction"].  For translation / similarity, without estimation_mask or estimator "subject"; everything behind
    the fit table follows unchanged.  None / 0 / False: the behaviour and meta without it, byte for byte, and nothing new is
    launched.  Bypass paths ignore it.
    drift_exposure, drift_mask (beyond the reference, None by default; with drift_correction only): what real handheld footage
    adds to the keyframe alignment.  drift_exposure=True estimates a gain and an offset per frame against its keyframe next to
    the motion, so that auto-exposure between frames up to a whole spacing apart does not read as a residual; a frame whose
    gain leaves [0.5, 2] or whose offset exceeds 64 grey levels keeps its chained estimate under the reason "gain".
    drift_mask=True (needs estimation_mask) leaves the pixels the estimation mask's block grid names, in the keyframe or in the
    frame, out of the alignment, and with it drift_correction accepts estimation_mask.  Both use the second form of the rule
    (include/vstab.h); meta["drift_correction"] gains `exposure` (the gains and offsets), `masked_fraction_mean` and
    frames_kept["gain"].  None / False: the behaviour and meta without them, byte for byte, and nothing new is launched.
    deflicker, deflicker_mode (beyond the reference, None by default): True (a window of 1 s) or a window in seconds in (0, 60].
    Auto exposure and auto white balance hunt while the camera shakes, and once the picture stands still the brightness steps
    are what is left to see.  Every consecutive pair of SOURCE frames is compared through its own full-resolution transition on
    a lattice of well-exposed pixels: the histogram of the registered 16-bit level ratios gives a median no moving subject
    shifts while it owns less than half of the samples, the level sums inside a band around it give the pair's gain
    (deflicker.py; include/vstab.h states both rules).  The log-gains are chained per shot -- and no further than a pair with
    confidence 0 or too few samples --, the chain's box mean over the window is taken, and every frame's own pixels are
    multiplied by exp(mean - chain), at most one stop: the high-pass, so a deliberate exposure ramp survives.
    deflicker_mode None / "exposure" applies one gain to the three colours, "rgb" one per colour (white balance too).  It is
    the first pass behind the warp, so the blended fill's exposure match, the fills and the stability report see
    deflickered frames; padding keeps its colour.  Behind either plan path, with every camera estimator; not with estimator
    "subject", sharpness_transfer, or temporal_fill without fill_exposure=True.  meta["deflicker"] reports every pair's gain,
    every frame's correction and the chain's RMS step before and after.  None / False: the behaviour and meta without it, byte
    for byte, and nothing new is launched.  Bypass paths ignore it.
    horizon_level, horizon_limit (beyond the reference, None by default): True levels every shot with one roll offset, a window
    in seconds in (0, 60] lets that offset vary slowly (a camera that tips over).  Every other pass removes relative motion; a
    clip shot 5 degrees off level comes out steady and 5 degrees off level.  The estimation images' gradient orientations,
    folded modulo 90 degrees, are reduced to one histogram per frame (horizon_level.py; include/vstab.h states the rule); its
    peak is the frame's roll, the chain of transitions supplies every frame's roll relative to its shot's first frame, and the
    median of the differences -- per shot under scene_cuts -- is the one number taken from the picture content.  Every final
    matrix is then turned about the canvas centre by what is left, at most horizon_limit degrees (None: 20, else in (0, 45):
    structure gives the roll modulo 90 only), in front of the mesh warp and the dynamic zoom, and everything behind the plan
    follows.  A shot without enough measurable frames is reported as not observable and is left as it is.  For crop_and_pad
    framing and translation / similarity, not with estimator "subject" or rolling_shutter; meta["horizon_level"] reports every
    frame's roll, confidence, offset and correction.  None: the behaviour and meta without it, byte for byte, and nothing new
    is launched.  Bypass paths ignore it.
    plate_fill (beyond the reference, None by default): True, or the number of valid samples a plate pixel needs, an int in
    1..256 (True is 1).  A locked shot registers every output frame to its shot's first frame, so the per-pixel median over
    time of what the frames really show -- the samples under the warp's own mask, up to 256 frames per shot at the centres of
    equal strata -- is one still image of the background with everything that moves taken out (clean_plate.py; include/vstab.h
    states the rules).  It is formed before any fill, per shot under scene_cuts, and what is still padding behind
    temporal_fill is taken from it, with its mask set to 0 as the temporal fill does, before spatial_fill invents the rest: the
    border is one plate, not a patchwork that changes its donor from frame to frame.  Needs camera_lock=True at strength 1; not
    with dynamic_zoom, a horizon_level window or estimator "subject", whose frames are not registered to each other (or not
    on the background).  `padding_fraction_*` keep describing the warp; meta["plate_fill"] reports samples, what was filled,
    what is left and what no frame of a shot saw.  None / False: the behaviour and meta without it, byte for byte, and nothing
    new is launched.  `crop` framing has no padding; bypass paths ignore it.
    track_box, track_key, track_radius (beyond the reference, None / 0 / None by default; with estimator="track" only, and
    track_box required by it): the subject lock without a mask.  track_box = (x, y, width, height), ints in full-resolution
    pixels, is a rectangle around the subject in frame track_key; its content in the estimation image of that frame is the
    template, and one device pass follows it through the clip, forwards and backwards from the key frame, by an exhaustive
    zero-mean SSD search within track_radius working pixels (None: 24, else an int in 1..48) of the previous position, in
    exact integers (template_track.py; include/vstab_track.h states the rule).  A parabola through the costs beside the pick
    refines the position, 1 - sqrt(J_best / J_T) is the confidence, frames below 0.3 are lost: interpolated and reported with
    confidence 0.  The transitions are the subject's, and everything behind the fit table follows as for the subject lock:
    camera_lock=True pins the subject where frame 0 shows it.  For translation only, without scene_cuts, estimation_mask,
    subject_mask, mesh_warp, temporal_fill, sharpness_transfer, rolling_shutter, drift_correction, deflicker, horizon_level or
    plate_fill; meta["template_track"] reports positions, confidences and lost frames.  track_box=None with any other
    estimator: the behaviour and meta without it, byte for byte, and nothing new is launched.  Bypass paths ignore them."""
    kw = dict(locals())     # every argument by name (nothing else is local yet): the keyword extras are read from here
    request = check_flow_request(framing_mode, transform_mode, estimator, kw)
    estimator = request.estimator
    total_frames = len(context.frames)
    fps_effective, fps_requested = _fps_fields(context, frame_rate)
    args = FlowArgs(framing_mode, transform_mode, camera_lock, strength, smooth, keep_fov, padding_rgb, fps_effective, fps_requested)
    size = (context.width, context.height)
    rgb_list = [int(c) for c in padding_rgb]

    if total_frames == 0:  # unreachable through the node (flow.py:242-273)
        meta = {
            "frames": 0,
            "note": "Empty frame sequence; nothing to stabilise.",
            "transform_mode_requested": transform_mode,
            "transform_mode_applied": "identity",
            "camera_lock": camera_lock,
            "strength": strength,
            "strength_effective": 0.0,
            "smooth": smooth,
            "fps_requested": fps_requested,
            "fps_effective": fps_effective,
            "framing": {"mode": framing_mode, "input_size": list(size), "padding_color_rgb": rgb_list},
            "keep_fov_applied": False,
            "padding_color_rgb": rgb_list,
            **_backend_fields(estimator),
            "stabilization_warp": hm._build_stabilization_warp_meta(
                source_size=size, output_size=size, framing_mode=framing_mode, applied_matrices=[]),
            "estimated_motion": {"per_transition": [], "path": [], "target_path": [], "target_path_effective": []},
            "padding_fraction_mean": 0.0,
            "padding_fraction_max": 0.0,
        }
        return hm.StabilizationResult([], [], _attach_motion_meta(meta, fps_effective, estimator))

    progress_total = max(0, total_frames - 1) + total_frames
    pbar = ProgressBar(progress_total)

    if total_frames == 1:  # flow.py:289-310
        meta = {
            "frames": 1,
            "note": "Single-frame input; bypassed stabilization.",
            "transform_mode": transform_mode,
            "framing_mode": framing_mode,
            **({"keep_fov_applied": False} if estimator != "classic" else {}),   # flow.py:297 only; classic.py:236-250 has no such key
            **_backend_fields(estimator),
            "stabilization_warp": hm._build_stabilization_warp_meta(
                source_size=size, output_size=size, framing_mode=framing_mode,
                applied_matrices=[np.eye(3, dtype=np.float32)]),
            "fps_requested": fps_requested,
            "fps_effective": fps_effective,
        }
        pbar.update_absolute(progress_total, progress_total)
        frames_out = _host_frames(context)
        masks_out = np.zeros((1, context.height, context.width, 1), np.float32)
        return hm.StabilizationResult(frames_out, masks_out, _attach_motion_meta(meta, fps_effective, estimator))

    _check_request_against_clip(request, kw, transform_mode, total_frames, size)
    ctx = ctx or native.default_context()
    device_frames = context.device_batch(ctx)
    working_size = hm._working_estimation_size(context.width, context.height)
    blocked = mask_info = None
    if estimation_mask is not None:   # reduced once per call: the block grid serves every estimation pass below
        blocked, mask_frames = _block_grid(ctx, estimation_mask, total_frames, working_size, request.mask_margin)
        mask_info = (request.mask_margin, mask_frames, int(blocked.shape[1] * blocked.shape[2]))

    if not request.needs_host_plan and device_plan_applies(estimator, framing_mode, transform_mode, total_frames):
        done = _stabilize_with_device_plan(ctx, context, device_frames, request, args, pbar, keep_on_device, blocked, mask_info)
        if done is not None:
            return done
        device_frames = context.device_batch(ctx)   # F0 rescaled the clip: everything is redone on the rescaled frames below

    # ---- estimation (F2-F5) -------------------------------------------------
    # the estimator's keyword arguments, built here and nowhere else: the block grid or the subject's mask (never both: the
    # checks refuse it), and a fresh list for every by-product that has to stay alive behind the fits
    extras = {"subject": {"mask": subject_lock_mod.mask_on_device(ctx, subject_mask)}} if request.subject else {}
    if request.track is not None:
        extras["track"] = {"request": request.track}
    if blocked is not None:
        extras["blocked"] = blocked

    def estimate(frames, peaks_out=None):
        extras.update({name: [] for name in request.kept_by_products})
        return _ESTIMATORS[estimator](ctx, frames, working_size, transform_mode, peaks_out=peaks_out, **extras)

    peaks = [] if context.range_pending else None
    fit_records = estimate(device_frames, peaks)
    if peaks and hm.resolve_value_range(context, peaks[0], ctx):
        # F0 (stabilizer_utils.py:127-131): some frame turned out to be 0..255 float data.  The estimation above ran
        # optimistically on the tensor as given (the gray pass reported the per-frame maxima for free); the frames
        # have been rescaled now, so it is repeated on the rescaled clip.  0..1 input -- the ComfyUI IMAGE contract --
        # never takes this branch.
        device_frames = context.device_batch(ctx)
        fit_records = estimate(device_frames)
    progress_done = _replay_progress(pbar, 0, total_frames - 1, progress_total)
    check_interrupt()

    scene, mesh, zoom, rolling = request.scene, request.mesh, request.zoom, request.rolling
    segments = scene_block = None
    if scene is not None:
        segments, scene_block = _scene_segments(ctx, scene, fit_records, extras.get("gray_out"), transform_mode, total_frames)
    path_deltas = drift_block = None
    if request.drift is not None and not keep_fov_bypasses(framing_mode, keep_fov):   # (the plan returns the original frames)
        fit_records, path_deltas, drift_block = _drift_correction(ctx, request.drift, fit_records, extras["gray_out"][0], segments,
                                                                  total_frames, transform_mode, size, working_size,
                                                                  request.drift_exposure, blocked if request.drift_mask else None)
    plan = plan_stabilization(ctx, fit_records, size, total_frames, *args, estimator=estimator, segments=segments,
                              path_deltas=path_deltas)
    if plan.bypass_meta is not None:  # crop + keep_fov ~ 1 (flow.py:387-429): original frames
        pbar.update_absolute(progress_total, progress_total)
        frames_out = device_frames if keep_on_device else _host_frames(context)
        masks_out = (ctx.torch.zeros((total_frames, context.height, context.width, 1), device=ctx.device)
                     if keep_on_device else np.zeros((total_frames, context.height, context.width, 1), np.float32))
        return hm.StabilizationResult(frames_out, masks_out, _attach_motion_meta(plan.bypass_meta, fps_effective, estimator))

    # ---- warp (F13) ------------------------------------------------------------
    mesh_block = zoom_block = rolling_block = level_block = offsets = None
    if request.level is not None:
        plan, level_block = _horizon_level(ctx, request.level, plan, extras["gray_out"][0], segments)
    if mesh is not None:
        offsets, mesh_block = _mesh_offsets(ctx, mesh, plan, extras["grid_out"][0], blocked, working_size, size, segments, args)
    if zoom is not None:
        plan, zoom_block = _dynamic_zoom(ctx, zoom, plan, offsets, segments)
    if rolling is not None:
        def plan_again(table):
            return plan_stabilization(ctx, table, size, total_frames, *args, estimator=estimator, segments=segments)

        plan, velocity, readout, rolling_block, refit_table = _rolling_shutter(
            ctx, rolling, plan, extras.get("grid_out"), blocked, working_size, size, segments, plan_again if request.refit else None)
        if refit_table is not None:
            fit_records = refit_table          # what the meta's counts describe from here on
    warp_args = dict(border=hm.border_value(padding_rgb), want_mask=True, want_count=True)
    if mesh is not None:
        dst, mask, counts = ctx.mesh_warp_batch(device_frames, plan.final_matrices, plan.output_size, offsets, **warp_args)
        if request.mesh_motion:
            mesh_block["motion"] = mesh_warp_mod.motion_block(offsets, size)
    elif rolling is not None:
        dst, mask, counts = ctx.rolling_warp_batch(device_frames, plan.final_matrices, plan.output_size, velocity, readout, **warp_args)
    else:
        dst, mask, counts = ctx.warp_batch(device_frames, plan.final_matrices, plan.output_size, interp="bilinear", **warp_args)
    meta = prepare_meta(plan)  # host JSON work overlaps the warp kernel
    progress_done = _replay_progress(pbar, progress_done, total_frames, progress_total)
    pad_counts = _counts_to_host(counts)
    meta = complete_meta(meta, plan, pad_counts)
    blocks = {   # in the order the meta lists them
        "horizon_level": level_block,
        "dynamic_zoom": None if zoom_block is None else dynamic_zoom_mod.finish_meta(zoom_block, pad_counts),
        "estimation_mask": None if mask_info is None else estimation_mask_meta(fit_records, *mask_info),
        "scene_cuts": scene_block,
        "mesh_warp": mesh_block,
        "subject_lock": extras["subject"]["block"] if request.subject else None,
        "template_track": extras["track"]["block"] if request.track is not None else None,
        "rolling_shutter": rolling_block,
        "drift_correction": drift_block,
    }
    meta.update({key: block for key, block in blocks.items() if block is not None})
    return _finish(ctx, request, plan, device_frames, dst, mask, meta, segments, keep_on_device, {"used": False, "mismatched_frames": 0})
