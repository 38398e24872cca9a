"""Clean plate: the per-pixel temporal median of a locked shot, the fill of leftover padding from it, and the difference
matte (not a feature of the reference).

`camera_lock=True` at `strength=1` registers every output frame to its shot's first frame, so one pixel position shows one
scene point all through the shot.  The median over time of what the frames really show there (the samples whose padding mask
is <= 0.5) is the background with everything that moves taken out: a clean plate.  Two uses follow from it:

  * plate fill  what is still padding after the temporal fill is taken from the plate: seen somewhere in the shot, the same
                still image in every frame, where the temporal fill changes its donor from frame to frame and the spatial
                fill invents;
  * matte       a frame's own pixel that differs from the plate by more than a threshold in some channel moves.

Three device passes (include/vstab.h states the rules; a selection on integers is the same in any order, so all results
equal a NumPy restatement in bits): `native.Context.plate_median_batch`, `plate_fill_batch`, `plate_matte_batch`.  This
module is host only: the request, what it cannot run with, which frames of a shot are sampled, and the meta block.

Off by default.  The plate is formed BEFORE the temporal fill, under the warp's true mask -- a temporally filled pixel must
not vote as an own one -- and the fill runs between the temporal and the spatial fill: seen nearby in time, then seen
anywhere in the shot, then invented.  `padding_fraction_*` keep describing the warp.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from . import mask_handoff

# Choices, not calibrations: 256 samples bound the median kernel's LDS tile (a longer shot is sampled at the centres of 256
# equal strata); a matte threshold of 0.1 is a tenth of the value range, well above sensor noise and compression, below most
# subject / background contrasts; a plate value needs 3 samples before a median can outvote anything.
SAMPLES_MAX = 256
DEFAULT_MATTE_THRESHOLD = 0.1
DEFAULT_MATTE_MIN_COUNT = 3


def check_request(plate_fill) -> Optional[int]:
    """-> min_count, None = off.  plate_fill: None / False is off, True is 1, an int in 1..256 is the number of valid
    samples a plate pixel needs before it fills anything.  Everything else raises, naming the value."""
    if plate_fill is None or plate_fill is False:
        return None
    if plate_fill is True:
        return 1
    if isinstance(plate_fill, (bool, np.bool_)) or not isinstance(plate_fill, (int, np.integer)) or not 1 <= int(plate_fill) <= SAMPLES_MAX:
        raise ValueError(f"plate_fill={plate_fill!r} is not None, False, True or an integer in 1..{SAMPLES_MAX}")
    return int(plate_fill)


def check_pipeline(camera_lock, strength, estimator: str, zoom=None, level=None) -> None:
    """What the plate cannot run with raises, and says why.  zoom: dynamic_zoom.check_request's answer; level:
    horizon_level.check_request's (one offset per shot keeps the frames of a shot registered, a window does not)."""
    if not bool(camera_lock) or not float(np.clip(strength, 0.0, 1.0)) == 1.0:      # (the plan clips the strength to [0, 1] too)
        raise ValueError(f"plate_fill needs camera_lock=True and strength=1 (got camera_lock={camera_lock!r}, strength={strength!r}): "
                         "only a locked shot registers its output frames to each other, and a median over frames that are not "
                         "registered is a smear.")
    if zoom is not None:
        raise ValueError("plate_fill is not supported with dynamic_zoom: the per-frame zoom unregisters the frames of a shot.")
    if level is not None and level.window_s is not None:
        raise ValueError("plate_fill is not supported with a horizon_level window: the per-frame turn unregisters the frames of a "
                         "shot.  horizon_level=True (one offset per shot) is allowed.")
    if estimator == "subject":
        raise ValueError("plate_fill is not supported with estimator 'subject': the frames are then registered on the subject, and "
                         "the plate would be of the subject.")


def _segments(segments, total_frames: int):
    return [(0, int(total_frames))] if segments is None else [(int(s), int(e)) for s, e in segments]


def sample_table(segments, total_frames: int) -> np.ndarray:
    """-> int32 [shots, S]: the frames of every shot [s, e) of length L the plate is formed from, S_s = min(L, 256) samples at
    s + ((2k + 1) * L) // (2 * S_s), the centres of S_s equal strata (every frame of a shot of up to 256), rows padded with -1
    to the widest.  segments None: one shot [0, total_frames)."""
    segs = _segments(segments, total_frames)
    rows = []
    for s, e in segs:
        length = e - s
        if length < 1 or s < 0 or e > total_frames:
            raise ValueError(f"clean plate: shot [{s}, {e}) is not a range of frames in 0..{total_frames}")
        count = min(length, SAMPLES_MAX)
        k = np.arange(count, dtype=np.int64)
        rows.append(s + ((2 * k + 1) * length) // (2 * count))
    width = max(len(r) for r in rows)
    table = np.full((len(rows), width), -1, np.int32)
    for i, r in enumerate(rows):
        table[i, :len(r)] = r
    return table


def plate_on_device(ctx, frames, mask, segments=None):
    """frames [n,h,w,3], mask [n,h,w] or None (device, read only) -> (plate [shots,h,w,3], count [shots,h,w], the sample table)."""
    table = sample_table(segments, int(frames.shape[0]))
    plate, count = ctx.plate_median_batch(frames, mask, table)
    return plate, count, table


def fill_on_device(ctx, dst, mask, plate, count, segments, min_count: int):
    """Fills dst / mask in place per shot -> filled_count i32 [n] (device)."""
    return ctx.plate_fill_batch(dst, mask, plate, count, mask_handoff.shots_from_segments(segments, int(dst.shape[0])), int(min_count))


def matte_on_device(ctx, frames, mask, plate, count, segments, threshold: float = DEFAULT_MATTE_THRESHOLD,
                    min_count: int = DEFAULT_MATTE_MIN_COUNT):
    """-> (matte f32 [n,h,w], matte_count i32 [n]), device tensors; nothing is written to the inputs."""
    return ctx.plate_matte_batch(frames, mask, plate, count, mask_handoff.shots_from_segments(segments, int(frames.shape[0])),
                                 threshold, int(min_count))


def meta_block(min_count: int, table, filled_counts, padded_after, unseen_counts, size: Tuple[int, int]) -> Dict[str, Any]:
    """meta["plate_fill"].  The fractions are formed like `padding_fraction_*` (float32 count / float32 pixels): filled_counts
    [n] the fill's per-frame counts, padded_after [n] the pixels with !(mask <= 0.5) behind it, unseen_counts [shots] the plate
    pixels with count < min_count; size = (h, w)."""
    pixels = np.float32(int(size[0]) * int(size[1]))

    def fraction(counts):
        return (np.asarray(counts, dtype=np.int64).reshape(-1).astype(np.float32) / pixels).astype(np.float64)

    filled, left = fraction(filled_counts), fraction(padded_after)
    table = np.asarray(table)
    return {"version": 1, "min_count": int(min_count), "shots": int(table.shape[0]),
            "samples_per_shot": [int(v) for v in (table >= 0).sum(axis=1)],
            "filled_fraction_mean": float(np.mean(filled)), "filled_fraction_max": float(np.max(filled)),
            "padding_fraction_mean_after": float(np.mean(left)), "padding_fraction_max_after": float(np.max(left)),
            "frames_with_padding_after": int((np.asarray(padded_after, dtype=np.int64) > 0).sum()),
            "unseen_fraction": [float(v) for v in fraction(unseen_counts)]}


def fill_and_report(ctx, dst, mask, plate, count, table, segments, min_count: int) -> Dict[str, Any]:
    """The pipelines' fill step: fills in place, then one small download (the fill's counts, what is still padding per frame,
    the plate pixels no min_count frames saw per shot) -> the meta block."""
    torch = ctx.torch
    filled = fill_on_device(ctx, dst, mask, plate, count, segments, min_count)
    left = torch.logical_not(mask <= 0.5).sum(dim=(1, 2), dtype=torch.int64)
    unseen = (count < int(min_count)).sum(dim=(1, 2), dtype=torch.int64)
    numbers = torch.cat([filled.to(torch.int64), left, unseen]).cpu().numpy()
    n = int(dst.shape[0])
    return meta_block(min_count, table, numbers[:n], numbers[n:2 * n], numbers[2 * n:], (int(dst.shape[1]), int(dst.shape[2])))
