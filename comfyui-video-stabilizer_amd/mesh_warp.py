"""Mesh warp: take out the residual motion that one global fit per frame pair leaves (parallax, rolling-shutter skew, lens
breathing), after MeshFlow (Liu et al., ECCV 2016: per-vertex motion profiles).

The device side: `native.Context.mesh_residual_batch` (csrc/vstab_mesh.hip) reduces the stride-8 flow grid a Flow run
already has to one residual per mesh vertex and pair, `native.Context.mesh_warp_batch` (csrc/vstab_warp.hip:
warp_kernel with MeshWarpArgs) is the plain warp with a per-vertex displacement of the source frame (include/vstab.h states both
rules). This module is the host side between the two: the checks of a request and the vertex paths. Nothing here needs
a GPU.

A vertex path is treated exactly as the global parameters are: P_0 = 0, P_{i+1} = P_i + r_i, sent through the same
trajectory routine with the plan's own smooth / fps / strength / camera_lock, so local and global smoothing agree by
construction.

The round trip: `motion_block` puts the per-vertex offsets of a run into meta["mesh_warp"]["motion"] (Flow's
`mesh_motion=True`), `parse_motion_block` reads and checks them, and Motion Apply's `mesh=True` replays them -- forward
through `mesh_warp_batch`, or restoring through `native.Context.mesh_unwarp_batch`, the per-pixel inverse of the
displacement (include/vstab.h states that rule too).  Out of scope of the round trip: bicubic interpolation, motion blur,
`crop` framing and the sharded path; of the mesh warp as a whole also the device plan and per-vertex adaptive smoothing.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, Dict, Optional, Sequence, Tuple

import numpy as np

DEFAULT_CELLS = (16, 9)          # mesh_warp=True: 16 x 9 cells, 17 x 10 vertices
CELLS_MIN, CELLS_MAX = 2, 64
# max_shift default: 1/64 of the frame's width, full-resolution px (30 px at 1920).  Tried on synthetic material only --
# procedural texture under a smooth differential shake, no footage -- which is why it is a parameter of every entry point.
DEFAULT_MAX_SHIFT_FRACTION = 1.0 / 64.0
MOTION_VERSION = 1               # meta["mesh_warp"]["motion"]["version"]
VERTS_MIN, VERTS_MAX = 2, 65     # vertices per axis (native.MESH_MAX_VERTS)

_ESTIMATOR_LIMITS = {
    "classic": "the Classic estimator tracks sparse corners: it has no dense grid of flow samples to take the residual from.",
    "flow_phase_correlate": "phase correlation yields one global shift per pair: it has no dense grid of flow samples.",
    "subject": "the subject lock reduces a mask to a centroid and an area: it has no dense grid of flow samples.",
}


@dataclass
class Request:
    """A checked mesh_warp request."""

    cols: int                       # cells per row; vertices per row = cols + 1
    rows: int
    max_shift: Optional[float]      # full-resolution px; None: DEFAULT_MAX_SHIFT_FRACTION of the frame's width

    @property
    def vertices(self) -> Tuple[int, int]:
        return self.cols + 1, self.rows + 1

    def max_shift_px(self, width: int) -> float:
        return float(width) * DEFAULT_MAX_SHIFT_FRACTION if self.max_shift is None else self.max_shift


def check_request(mesh_warp, mesh_max_shift=None) -> Optional[Request]:
    """The checks that need neither the clip nor a GPU.  None -> None (the feature is off); True -> DEFAULT_CELLS;
    (cols, rows) -> that many cells, each in 2..64.  mesh_max_shift: None or a finite number above 0."""
    if mesh_warp is None:
        return None
    if mesh_warp is True:
        cols, rows = DEFAULT_CELLS
    else:
        ok = (isinstance(mesh_warp, (tuple, list)) and len(mesh_warp) == 2
              and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in mesh_warp))
        if not ok:
            raise ValueError(f"mesh_warp={mesh_warp!r}: expected None, True or a (cols, rows) pair of integers")
        cols, rows = int(mesh_warp[0]), int(mesh_warp[1])
        if not (CELLS_MIN <= cols <= CELLS_MAX and CELLS_MIN <= rows <= CELLS_MAX):
            raise ValueError(f"mesh_warp={mesh_warp!r}: cols and rows must lie in [{CELLS_MIN}, {CELLS_MAX}]")
    shift = mesh_max_shift
    if shift is not None:
        if isinstance(shift, bool) or not isinstance(shift, (int, float, np.integer, np.floating)) or not np.isfinite(shift) or shift <= 0.0:
            raise ValueError(f"mesh_max_shift={mesh_max_shift!r}: expected a finite number above 0 (full-resolution px) or None")
        shift = float(shift)
    return Request(cols, rows, shift)


def check_pipeline(estimator: str, framing_mode: str, temporal_fill: int) -> None:
    """What a mesh-warp call cannot be combined with, each with its reason."""
    if estimator in _ESTIMATOR_LIMITS:
        raise ValueError(f"mesh_warp is not supported with estimator {estimator!r}: {_ESTIMATOR_LIMITS[estimator]}")
    if framing_mode == "crop":
        raise ValueError("mesh_warp is not supported with framing_mode 'crop': the crop solver bounds matrices only, so it "
                         "cannot keep a per-vertex displacement free of padding.")
    if int(temporal_fill) > 0:
        raise ValueError(f"mesh_warp is not supported with temporal_fill={int(temporal_fill)}: fill candidates are global "
                         "matrices, which do not describe a mesh-warped neighbour.")


def vertex_median3(residual: np.ndarray) -> np.ndarray:
    """MeshFlow's second filter: a 3x3 median over the vertices of every pair and axis ([P,mh,mw,2]; the border vertices
    see their own values repeated)."""
    r = np.asarray(residual)
    pad = np.pad(r, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    mh, mw = r.shape[1], r.shape[2]
    stack = np.stack([pad[:, dy:dy + mh, dx:dx + mw] for dy in range(3) for dx in range(3)], axis=0)
    return np.median(stack, axis=0).astype(r.dtype)


def plan_offsets(trajectory: Callable, residual, confidences: Sequence[float], segments, smooth: float, fps: float,
                 strength: float, camera_lock: bool, scale: Tuple[float, float], max_shift: float):
    """Vertex residuals -> the warp's per-frame vertex offsets.
    trajectory: native.Context.trajectory (deltas [n-1,p] -> path, target [n,p]); residual f32 [P,mh,mw,2] in working px;
    confidences [P] of the transitions the plan used (0: a failed fit or a scene cut -- that pair contributes nothing);
    segments: None or the shots' frame ranges [s, e) -- paths restart at 0 in every shot; scale = (x, y) working px ->
    full-resolution px; max_shift: per-axis clamp in full-resolution px.
    -> (offsets f32 [P+1,mh,mw,2] full-resolution px, paths f64 [P+1,mh,mw,2] working px)."""
    r = vertex_median3(np.asarray(residual, dtype=np.float32)).astype(np.float64)
    pairs, mh, mw, _ = r.shape
    conf = np.asarray(confidences, dtype=np.float64).reshape(pairs)
    r[conf == 0.0] = 0.0
    deltas = r.reshape(pairs, mh * mw * 2)
    n = pairs + 1
    path = np.zeros((n, deltas.shape[1]), np.float64)
    target = np.zeros_like(path)
    for s, e in ([(0, n)] if segments is None else segments):
        if e - s >= 2:
            path[s:e], target[s:e] = trajectory(deltas[s:e - 1], smooth, fps, strength, bool(camera_lock))
    correction = (target - path).reshape(n, mh, mw, 2)
    correction = correction * np.array([scale[0], scale[1]], np.float64)
    correction = np.clip(correction, -float(max_shift), float(max_shift))
    return correction.astype(np.float32), path.reshape(n, mh, mw, 2)


def meta_block(request: Request, max_shift: float, residual, count, offsets, min_samples: int) -> Dict[str, Any]:
    """meta["mesh_warp"]: residuals in working px (as measured, before the vertex median), corrections in full-resolution px."""
    res = np.abs(np.asarray(residual, dtype=np.float64))
    off = np.abs(np.asarray(offsets, dtype=np.float64))
    return {"cells": [int(request.cols), int(request.rows)], "max_shift": float(max_shift),
            "residual_px_mean": float(res.mean()), "residual_px_max": float(res.max()),
            "correction_px_mean": float(off.mean()), "correction_px_max": float(off.max()),
            "vertices_without_samples": int((np.asarray(count) < int(min_samples)).sum())}


# ---- the round trip: the offsets in the meta -----------------------------------------------------------------------------
@dataclass
class Motion:
    """A parsed meta["mesh_warp"]["motion"] block."""

    domain_size: Tuple[int, int]    # (w, h) of the canvas the mesh lies over: the source frames of the mesh-warped run
    vertices: Tuple[int, int]       # (mw, mh)
    offsets: np.ndarray             # f32 [N,mh,mw,2], px of the domain


def motion_block(offsets, domain_size) -> Dict[str, Any]:
    """meta["mesh_warp"]["motion"]: the warp's per-frame vertex offsets, f32 [N,mh,mw,2] in px of domain_size = (w, h), as JSON
    numbers.  A float32 widened to a Python float survives json.dumps / loads exactly (repr round-trips a double)."""
    off = np.asarray(offsets, dtype=np.float32)
    if off.ndim != 4 or off.shape[3] != 2:
        raise ValueError(f"mesh motion: offsets {off.shape} are not [N,mh,mw,2]")
    n, mh, mw, _ = off.shape
    return {"version": MOTION_VERSION, "domain_size": [int(domain_size[0]), int(domain_size[1])], "vertices": [int(mw), int(mh)],
            "frame_count": int(n), "offsets": off.astype(np.float64).tolist()}


def _int_pair(block, key) -> Tuple[int, int]:
    raw = block.get(key)
    ok = (isinstance(raw, (list, tuple)) and len(raw) == 2
          and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in raw))
    if not ok:
        raise ValueError(f"mesh_warp.motion.{key} must be a pair of integers, got {raw!r}.")
    return int(raw[0]), int(raw[1])


def parse_motion_block(meta, frame_count: Optional[int] = None, domain_size: Optional[Tuple[int, int]] = None) -> Motion:
    """meta["mesh_warp"]["motion"] -> Motion, or a ValueError that names the key or shape that is wrong.  frame_count /
    domain_size: what the motion the caller resolved expects (None: not checked)."""
    mesh = meta.get("mesh_warp") if isinstance(meta, dict) else None
    block = mesh.get("motion") if isinstance(mesh, dict) else None
    if not isinstance(block, dict):
        raise ValueError("meta has no mesh_warp.motion block: run Flow with mesh_warp and mesh_motion=True "
                         "(the Video Stabilizer Flow (Mesh Motion) node) to record the per-vertex offsets.")
    if block.get("version") != MOTION_VERSION:
        raise ValueError(f"mesh_warp.motion.version must be {MOTION_VERSION}, got {block.get('version')!r}.")
    domain = _int_pair(block, "domain_size")
    if domain[0] < 2 or domain[1] < 2:
        raise ValueError(f"mesh_warp.motion.domain_size {list(domain)} must be at least 2x2.")
    mw, mh = _int_pair(block, "vertices")
    if not (VERTS_MIN <= mw <= VERTS_MAX and VERTS_MIN <= mh <= VERTS_MAX):
        raise ValueError(f"mesh_warp.motion.vertices {[mw, mh]} outside {VERTS_MIN}..{VERTS_MAX} per axis.")
    count = block.get("frame_count")
    if not isinstance(count, (int, np.integer)) or isinstance(count, bool) or count < 0:
        raise ValueError(f"mesh_warp.motion.frame_count must be a non-negative integer, got {count!r}.")
    try:
        wide = np.asarray(block.get("offsets"), dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError("mesh_warp.motion.offsets must be a [frame_count][mh][mw][2] list of numbers.") from exc
    if wide.shape != (int(count), mh, mw, 2):
        raise ValueError(f"mesh_warp.motion.offsets has shape {list(wide.shape)}, expected {[int(count), mh, mw, 2]} "
                         "([frame_count][mh][mw][2]).")
    with np.errstate(over="ignore"):
        off = wide.astype(np.float32)
    if not np.isfinite(off).all():
        raise ValueError("mesh_warp.motion.offsets must contain finite float32 numbers.")
    if frame_count is not None and int(count) != int(frame_count):
        raise ValueError(f"mesh_warp.motion.frame_count is {int(count)}, the motion describes {int(frame_count)} frame(s).")
    if domain_size is not None and tuple(domain) != (int(domain_size[0]), int(domain_size[1])):
        raise ValueError(f"mesh_warp.motion.domain_size {list(domain)} does not match the motion's canvas "
                         f"{[int(domain_size[0]), int(domain_size[1])]}.")
    return Motion(domain, (mw, mh), np.ascontiguousarray(off))
