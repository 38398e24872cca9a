"""Dynamic zoom: every frame is zoomed about the canvas centre just enough to hide its own border, and the zoom factor is
smoothed over time so that it never pumps (vid.stab's adaptive `optzoom`, Gyroflow's dynamic zoom).

The device side is one pass, `native.Context.cover_extent_batch` (csrc/vstab_warp.hip: cover_extent_kernel; include/vstab.h
states the rule): per frame, how far the warp's own nearest-neighbour coverage reaches around the canvas centre, evaluated
per output pixel with the warp's own coordinate arithmetic, for the plain warp and for the mesh warp alike.  This module is
the host side: the checks of a request, the zoom a frame's extent asks for, its envelope over time and the zoom matrices.
Nothing here needs a GPU.

The zoom only changes each frame's final matrix (Z_i @ F_i), so everything behind the plan follows by itself: the warp or
mesh warp runs unchanged, `stabilization_warp` / `motion_meta` hold the zoomed matrices and Motion Apply replays or inverts
them, `padding_fraction_*` come from the zoomed warp's counts, temporal fill, spatial fill and the stability report see the
zoomed result.  For `crop_and_pad` framing only.  Out of scope: a non-centred or aspect-changing window, zoom driven by
anything but coverage, `crop` and `expand` framing, the sharded path and the device plan.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

VERSION = 1
# Both defaults are choices, not calibrations: they have been tried on synthetic material only -- procedural texture under
# a synthetic shake, no footage -- which is why both are parameters of every entry point.
DEFAULT_WINDOW_S = 2.0           # dynamic_zoom=True: the envelope's window in seconds
DEFAULT_ZOOM_LIMIT = 2.0         # zoom_limit=None
WINDOW_MAX_S = 60.0
ZOOM_LIMIT_MIN, ZOOM_LIMIT_MAX = 1.0, 16.0
MARGIN_PX = 2                    # VSTAB_ZOOM_MARGIN_PX (include/vstab.h)
SENTINEL = 0xFFFFFFFF            # extent of a frame without an uncovered pixel

_FRAMING_LIMITS = {
    "crop": "crop framing already has no padding: it removes it with one crop for the whole clip.",
    "expand": "an expand canvas has no frame to fill: it grows until it holds every frame.",
}


@dataclass
class Request:
    """A checked dynamic_zoom request."""

    window_s: float
    zoom_limit: float


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def check_request(dynamic_zoom, zoom_limit=None) -> Optional[Request]:
    """The checks that need neither the clip nor a GPU.  dynamic_zoom: None -> None (the feature is off), True -> a window
    of DEFAULT_WINDOW_S seconds, a finite number in (0, 60] -> that window in seconds.  zoom_limit: None ->
    DEFAULT_ZOOM_LIMIT, else a finite number in [1, 16]; without dynamic_zoom it is an error."""
    if dynamic_zoom is None:
        if zoom_limit is not None:
            raise ValueError(f"zoom_limit={zoom_limit!r} needs dynamic_zoom: without a dynamic zoom there is no zoom to limit.")
        return None
    if dynamic_zoom is True:
        window = DEFAULT_WINDOW_S
    else:
        if not _is_number(dynamic_zoom) or not np.isfinite(dynamic_zoom) or not 0.0 < dynamic_zoom <= WINDOW_MAX_S:
            raise ValueError(f"dynamic_zoom={dynamic_zoom!r}: expected None, True or a finite window in seconds in (0, {WINDOW_MAX_S:g}]")
        window = float(dynamic_zoom)
    limit = DEFAULT_ZOOM_LIMIT
    if zoom_limit is not None:
        if not _is_number(zoom_limit) or not np.isfinite(zoom_limit) or not ZOOM_LIMIT_MIN <= zoom_limit <= ZOOM_LIMIT_MAX:
            raise ValueError(f"zoom_limit={zoom_limit!r}: expected None or a finite number in [{ZOOM_LIMIT_MIN:g}, {ZOOM_LIMIT_MAX:g}]")
        limit = float(zoom_limit)
    return Request(window, limit)


def check_pipeline(framing_mode: str) -> None:
    """Dynamic zoom is a form of crop_and_pad framing: the other two raise, and say why."""
    if framing_mode in _FRAMING_LIMITS:
        raise ValueError(f"dynamic_zoom is not supported with framing_mode {framing_mode!r}: {_FRAMING_LIMITS[framing_mode]} "
                         "Use framing_mode 'crop_and_pad'.")


def radius_frames(window_s: float, fps_effective: float) -> int:
    """Half the window in frames: floor(window_s * fps_effective / 2 + 0.5)."""
    return int(np.floor(float(window_s) * float(fps_effective) / 2.0 + 0.5))


def required_zoom(extent, out_size) -> np.ndarray:
    """The zoom about the canvas centre that frame i needs, float64 [N], from its coverage extent (uint32, the rule of
    vstab_cover_extent_batch).  With E = (W-1)*(H-1) the canvas edge and m = 2 * MARGIN_PX * max(W-1, H-1) the margin in
    the extent's units: 1.0 for the sentinel, else max(1.0, E / max(extent - m, 1)).
    Two pixels of margin, not one: the covered integer rectangle ends up to one pixel (2 * (H-1) or 2 * (W-1) units) inside
    `extent`, so in the direction of the shorter side a one-pixel back-off leaves zero slack between the rectangle the zoomed
    warp samples and the integer rectangle known to be covered; two pixels leave at least one whole pixel, orders of
    magnitude above the float32 rounding of Z @ F."""
    w, h = int(out_size[0]), int(out_size[1])
    ext = np.asarray(extent).astype(np.int64).reshape(-1)
    if w < 2 or h < 2:
        raise ValueError(f"required_zoom: a {w}x{h} canvas has no centred extent")
    edge = np.float64((w - 1) * (h - 1))
    margin = 2 * MARGIN_PX * max(w - 1, h - 1)
    z = np.maximum(1.0, edge / np.maximum(ext - margin, 1).astype(np.float64))
    return np.where(ext == SENTINEL, 1.0, z).astype(np.float64)


def envelope(z_req, radius: int, limit: float, segments: Optional[Sequence[Tuple[int, int]]] = None) -> np.ndarray:
    """The zoom actually applied, float64 [N]: a sliding maximum of z_req over [i-r, i+r], then the box mean of that maximum
    over the same window, indices clamped to the clip -- or to the frame's segment [s, e): with scene cuts the envelope
    restarts in every shot, a zoom step across a cut is invisible -- and finally min(., limit).  Before the cap the result is
    >= z_req[i] everywhere and never above the largest z_req: every term of the mean is a maximum over a window that
    contains i (the closing clamp between z_req[i] and the largest term only takes the rounding of the mean's own sum and
    division out of those two statements).  r = 0 returns min(z_req, limit)."""
    z = np.asarray(z_req, dtype=np.float64).reshape(-1)
    n, r = z.shape[0], int(radius)
    if r < 0:
        raise ValueError(f"envelope: radius={radius} is negative")
    out = np.empty(n, np.float64)
    for s, e in (segments if segments is not None else [(0, n)]):
        if e <= s:
            continue
        seg = z[s:e]
        if r == 0:
            out[s:e] = seg
            continue
        idx = np.clip(np.arange(e - s)[:, None] + np.arange(-r, r + 1)[None, :], 0, e - s - 1)   # [len, 2r+1]
        top = seg[idx].max(axis=1)
        terms = top[idx]
        mean = terms.sum(axis=1) / np.float64(2 * r + 1)
        out[s:e] = np.maximum(np.minimum(mean, terms.max(axis=1)), seg)
    return np.minimum(out, np.float64(limit))


def zoom_matrices(z, out_size) -> np.ndarray:
    """Z_i = [[z, 0, (1-z) cx], [0, z, (1-z) cy], [0, 0, 1]] about the canvas centre cx = (W-1)/2, cy = (H-1)/2: formed in
    float64, cast once -> float32 [N,3,3].  Applied as np.matmul(Z, final) in float32, like the other framing shifts."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    cx, cy = (int(out_size[0]) - 1) / 2.0, (int(out_size[1]) - 1) / 2.0
    m = np.zeros((z.shape[0], 3, 3), np.float64)
    m[:, 0, 0] = z
    m[:, 1, 1] = z
    m[:, 0, 2] = (1.0 - z) * cx
    m[:, 1, 2] = (1.0 - z) * cy
    m[:, 2, 2] = 1.0
    return m.astype(np.float32)


def plan_zoom(request: Request, extent, out_size, fps_effective: float,
              segments: Optional[Sequence[Tuple[int, int]]] = None):
    """Extents -> (zoom matrices float32 [N,3,3], meta["dynamic_zoom"] without `frames_with_padding`, which the warp's
    counts complete: finish_meta)."""
    z_req = required_zoom(extent, out_size)
    radius = radius_frames(request.window_s, fps_effective)
    z = envelope(z_req, radius, request.zoom_limit, segments)
    block = {
        "version": VERSION,
        "window_s": float(request.window_s),
        "radius_frames": int(radius),
        "zoom_limit": float(request.zoom_limit),
        "margin_px": MARGIN_PX,
        "zoom_required": z_req.tolist(),
        "zoom": z.tolist(),
        "zoom_mean": float(np.mean(z)),
        "zoom_max": float(np.max(z)),
        "static_zoom": float(np.max(z_req)),       # what one crop for the whole clip would need
        "frames_capped": int(np.count_nonzero(z_req > request.zoom_limit)),   # the cap leaves these short of what they need
        "frames_with_padding": None,
    }
    return zoom_matrices(z, out_size), block


def finish_meta(block: Dict[str, Any], pad_counts) -> Dict[str, Any]:
    """frames_with_padding: frames whose (zoomed) warp reported a non-zero padded-pixel count.  Reported, never retried."""
    block["frames_with_padding"] = int(np.count_nonzero(np.asarray(pad_counts, dtype=np.int64) > 0))
    return block
