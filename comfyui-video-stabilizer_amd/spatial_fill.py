"""Spatial fill: the pixels of a stabilized frame that stay padding are filled from the frame's own valid pixels.

Pyramid push-pull (Gortler et al., "The Lumigraph", 1996): valid pixels are averaged down a pyramid, holes are filled back
up from the first level that knows something.  The kernels behind `native.Context.spatial_fill_batch`
(csrc/vstab_fill.hip) read only a frame and its mask -- see include/vstab.h for the exact rule -- so the pass composes with
everything that produces the two: Flow, Classic, temporal fill, mesh warp, Motion Apply in both directions.  The mask is not
changed: these pixels are invented, not seen, and a downstream in-painter still needs to know where they are.  Per frame,
deterministic, off by default.
"""

from __future__ import annotations

from typing import Any, Dict

import numpy as np

METHOD = "push_pull"
VERSION = 1


def check_request(spatial_fill) -> bool:
    """The keyword of the pipelines: a bool, anything else is a ValueError naming the value."""
    if not isinstance(spatial_fill, bool):
        raise ValueError(f"spatial_fill={spatial_fill!r} is not a bool (True fills the leftover padding, False leaves it)")
    return spatial_fill


def fill_meta(hole_counts, fill_counts, output_size) -> Dict[str, Any]:
    """The `spatial_fill` meta block from the kernel's per-frame counts (fractions formed like `padding_fraction_*`: float32
    count / float32 pixels).  frames_without_source: frames with holes and no valid pixel, which stay as they were."""
    holes = np.asarray(hole_counts, dtype=np.int64).reshape(-1)
    filled = np.asarray(fill_counts, dtype=np.int64).reshape(-1)
    if holes.shape != filled.shape:
        raise ValueError(f"spatial fill: {holes.shape[0]} hole counts and {filled.shape[0]} fill counts")
    pixels = np.float32(int(output_size[0]) * int(output_size[1]))
    fraction = (filled.astype(np.float32) / pixels).astype(np.float64)
    return {"method": METHOD, "version": VERSION,
            "filled_fraction_mean": float(np.mean(fraction)) if fraction.size else 0.0,
            "filled_fraction_max": float(np.max(fraction)) if fraction.size else 0.0,
            "frames_filled": int(np.count_nonzero(filled)),
            "frames_without_source": int(np.count_nonzero((holes > 0) & (filled == 0)))}


def fill_on_device(ctx, dst, mask) -> Dict[str, Any]:
    """Runs the fill over a whole clip in place (dst [N,h,w,3], mask [N,h,w] or [N,h,w,1], device) and returns the meta block."""
    hole_count, fill_count = ctx.spatial_fill_batch(dst, mask)
    counts = ctx.torch.stack([hole_count, fill_count]).cpu().numpy()
    return fill_meta(counts[0], counts[1], (dst.shape[2], dst.shape[1]))
