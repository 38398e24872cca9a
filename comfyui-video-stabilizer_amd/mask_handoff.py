"""Mask hand-off: hold, grow and feather the padding mask for a generative outpainter (not a feature of the reference).

The reference exists to feed an outpainter: its README hands `padding_mask` to VACE, and both workflows it ships put ComfyUI's
core GrowMask node (expand 5, tapered corners) between the stabilizer and WanVaceToVideo -- because the outermost ring of own
pixels has the padding colour interpolated into it while the mask is 0 there, so the repaint region has to be wider than
the mask.  GrowMask runs scipy's 3 x 3 grey dilation once per pixel of growth, per frame, on one CPU thread, on a mask that
was on the GPU a moment earlier.  Two more things outpainting users do by hand belong with it: a soft edge (a hard mask edge
shows as a seam when the generated border is composited back) and a steady region (in stabilized output the content stands
still and the padding border is what shakes; holding the mask over a few neighbouring frames gives the video model one
outline to repaint).

Three device passes, in this order (include/vstab.h states the rules; all are maxima, so the result equals a NumPy
restatement in bits):
  * hold     `native.Context.mask_hold_batch`: the maximum over the frames within `hold` of each frame, inside its shot;
  * grow     `native.Context.mask_grow_batch`: GrowMask's dilation (erosion for a negative value) over the L1 ball (tapered) or
             the square one, clipped to the frame;
  * feather  the same call: an outward linear ramp of `feather` pixels in the same norm, on 16-bit levels.

Off by default.  It replaces only the mask a pipeline RETURNS: the fills, the sharpness transfer and the stability report
keep seeing the true mask, and `padding_fraction_*` keeps describing the warp.
"""

from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional

import numpy as np

HOLD_MAX = 16
GROW_MAX = 64
FEATHER_MAX = 64


class Request(NamedTuple):
    hold: int
    grow: int
    tapered: bool
    feather: int


def _int_in(name: str, value, lo: int, hi: int) -> int:
    if value is None:
        return 0
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{name}={value!r} is not None or an integer in {lo}..{hi}")
    return int(value)


def check_request(mask_grow=None, mask_feather=None, mask_hold=None, mask_tapered=None) -> Optional[Request]:
    """-> the request, None = off (all four None).  Any of mask_grow (int in -64..64), mask_feather (int in 0..64) and
    mask_hold (int in 0..16) given switches the hand-off on, the others read as 0; mask_tapered (a bool, None reads as True)
    chooses GrowMask's tapered corners and needs one of the three.  Everything is checked here, before any GPU work."""
    grow = _int_in("mask_grow", mask_grow, -GROW_MAX, GROW_MAX)
    feather = _int_in("mask_feather", mask_feather, 0, FEATHER_MAX)
    hold = _int_in("mask_hold", mask_hold, 0, HOLD_MAX)
    if mask_tapered is not None and not isinstance(mask_tapered, (bool, np.bool_)):
        raise ValueError(f"mask_tapered={mask_tapered!r} is not None or a bool")
    if mask_grow is None and mask_feather is None and mask_hold is None:
        if mask_tapered is not None:
            raise ValueError(f"mask_tapered={mask_tapered!r} needs mask_grow, mask_feather or mask_hold: it chooses their footprint")
        return None
    return Request(hold, grow, True if mask_tapered is None else bool(mask_tapered), feather)


def shots_from_segments(segments, total_frames: int) -> Optional[np.ndarray]:
    """The pipelines' `segments` (frame ranges [s, e) of the shots, None: one shot) as the hold's shot number per frame."""
    if segments is None:
        return None
    shot = np.zeros((int(total_frames),), np.int32)
    for index, (s, e) in enumerate(segments):
        shot[int(s):int(e)] = index
    return shot


def meta_block(request: Request, counts, size) -> Dict[str, Any]:
    """meta["mask_handoff"].  The fractions are formed like `padding_fraction_*` (float32 count / float32 pixels) from the
    per-frame counts of returned mask pixels above 0.5; size = (h, w)."""
    pixels = np.float32(int(size[0]) * int(size[1]))
    frac = (np.asarray(counts, dtype=np.int64).reshape(-1).astype(np.float32) / pixels).astype(np.float64)
    return {"version": 1, "hold": request.hold, "grow": request.grow, "tapered": request.tapered, "feather": request.feather,
            "masked_fraction_mean": float(np.mean(frac)) if frac.size else 0.0,
            "masked_fraction_max": float(np.max(frac)) if frac.size else 0.0}


def handoff_on_device(ctx, mask, request: Request, segments=None):
    """mask [n,h,w] f32, device, contiguous (left as it is) -> (the mask to hand on, a new device tensor; the meta block).
    Hold, then grow, then feather; under scene cuts (`segments`) the hold stays inside a shot.  One small download (the
    counts) ends it."""
    held = mask
    if request.hold > 0:
        held = ctx.mask_hold_batch(mask, request.hold, shots_from_segments(segments, mask.shape[0]))
    out, counts = ctx.mask_grow_batch(held, request.grow, tapered=request.tapered, feather=request.feather, want_count=True)
    return out, meta_block(request, counts.cpu().numpy(), (mask.shape[1], mask.shape[2]))
