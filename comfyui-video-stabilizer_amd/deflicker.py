"""Deflicker: the exposure (and, on request, white-balance) steps between consecutive frames are measured on registered
pixels, smoothed over time and taken out of the output frames.

Handheld footage is shot with auto exposure and auto white balance, and both hunt while the camera shakes.  Once the picture
stands still, a frame-to-frame brightness step is the most visible artefact left.  The stabilizer holds what a stand-alone
deflicker lacks: the transitions A_k that register frame k+1 against frame k, so the two can be compared pixel against the
same scene point and what differs is exposure, not content under camera motion.

The device side is three entries (csrc/vstab_deflicker.hip; include/vstab.h states both rules):
`native.Context.pair_gain_hist_batch` -- per pair, the histograms of the registered 16-bit level ratios on a lattice of
well-exposed pixels; `pair_gain_sums_batch` -- the level sums inside a band around each histogram's median; and
`apply_gain_batch` -- one float32 multiply per value of the output frames.  Everything between them is this module, in
float64 on the host, and needs no GPU: the median bin and its band, the gain of a pair, the running log-gain of a segment,
its box mean, the correction.

The correction is the HIGH-PASS of the log-gain chain: c_i = exp(mean(L) - L_i).  A slow measurement drift along the chain
cancels in it, and a deliberate exposure ramp survives.  Out of scope: an offset or gamma term, spatially varying flicker
(rolling light bands, vignetting), dropping samples under the estimation mask (the median already ignores a subject that
owns less than half of them), replaying or undoing the correction in Motion Apply, the sharded path and the device plan.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

VERSION = 1
# All of these are choices, not calibrations: they have been tried on synthetic material only -- procedural texture under a
# synthetic shake with synthetic gains, no footage.
STRIDE = 4                        # VSTAB_DEFLICKER_STRIDE: one pixel in 16 is compared
LEVEL_LO, LEVEL_HI = 2048, 63488  # VSTAB_DEFLICKER_LO / _HI: 1/32 from either end of the 16-bit range
BINS = 1024                       # VSTAB_DEFLICKER_BINS: ratios in units of 1/256, saturating at 1023 / 256
BAND_SHIFT = 3                    # the band reaches 1/8 of the median bin to either side
MIN_COUNT = 256                   # fewer samples in the band: the pair is unmeasured
CLAMP = (0.5, 2.0)                # the correction of a frame stays within one stop
DEFAULT_WINDOW_S = 1.0            # deflicker=True
WINDOW_MAX_S = 60.0
MODES = ("exposure", "rgb")


@dataclass(frozen=True)
class Request:
    """A checked deflicker request."""

    window_s: float
    mode: str


def _is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def check_request(deflicker, deflicker_mode=None) -> Optional[Request]:
    """The checks that need neither the clip nor a GPU.  deflicker: None / False -> None (the feature is off), True -> a
    window of DEFAULT_WINDOW_S seconds, a finite number in (0, 60] -> that window in seconds.  deflicker_mode: None /
    "exposure" (one gain for the three colours) or "rgb" (one per colour: white balance too); without deflicker it is an
    error."""
    if deflicker_mode is not None and not (isinstance(deflicker_mode, str) and deflicker_mode in MODES):
        raise ValueError(f"deflicker_mode={deflicker_mode!r}: expected None, 'exposure' or 'rgb'")
    if deflicker is None or deflicker is False:
        if deflicker_mode is not None:
            raise ValueError(f"deflicker_mode={deflicker_mode!r} needs deflicker: without a deflicker there are no gains to form.")
        return None
    if deflicker is True:
        window = DEFAULT_WINDOW_S
    else:
        if not _is_number(deflicker) or not np.isfinite(deflicker) or not 0.0 < deflicker <= WINDOW_MAX_S:
            raise ValueError(f"deflicker={deflicker!r}: expected None, False, True or a finite window in seconds in (0, {WINDOW_MAX_S:g}]")
        window = float(deflicker)
    return Request(window, deflicker_mode or "exposure")


def check_pipeline(estimator: str, temporal_fill: int, fill_exposure: bool, sharpness) -> None:
    """What the deflicker cannot run with raises, and says why."""
    if estimator == "subject":
        raise ValueError("deflicker is not supported with estimator 'subject': its transitions register the subject, not the "
                         "scene, so the pixels the measurement compares would not show the same scene point.")
    if temporal_fill > 0 and not fill_exposure:
        raise ValueError("deflicker with temporal_fill needs fill_exposure=True: a hard fill would paste the uncorrected pixels "
                         "of neighbouring frames next to corrected content.")
    if sharpness is not None:
        raise ValueError("deflicker is not supported with sharpness_transfer: the samples it blends in are the uncorrected "
                         "pixels of neighbouring frames.")


def radius_frames(window_s: float, fps_effective: float) -> int:
    """Half the window in frames, at least one: max(1, floor(window_s * fps_effective / 2 + 0.5))."""
    return max(1, int(np.floor(float(window_s) * float(fps_effective) / 2.0 + 0.5)))


def active_pairs(confidences, total_frames: int, segments: Optional[Sequence[Tuple[int, int]]] = None) -> np.ndarray:
    """bool [N-1]: the pairs worth measuring -- inside one shot and with a transition the estimator stands behind
    (confidence > 0; a NaN is not)."""
    conf = np.asarray(confidences, dtype=np.float64).reshape(-1)
    if conf.shape != (total_frames - 1,):
        raise ValueError(f"deflicker: {conf.size} confidences for {total_frames} frames")
    active = conf > 0.0
    for s, _ in (segments or [])[1:]:
        if 1 <= s <= total_frames - 1:
            active[s - 1] = False          # the pair across the cut
    return active


# ---- host arithmetic on the downloaded integers ------------------------------------------------------------------------
def bands_from_hist(hist) -> Tuple[np.ndarray, np.ndarray]:
    """hist int [P,4,1024] -> (band int32 [P,4,2], median int64 [P,4]).  m is the LOWER median bin: the smallest bin whose
    cumulative count reaches (total + 1) // 2.  The band is [m - (m >> 3), m + ((m + 7) >> 3)], both inclusive: 1/8 to either
    side, rounded outwards above.  An empty histogram gives m = -1 and the empty band [1, 0]."""
    hist = np.asarray(hist).astype(np.int64)
    if hist.ndim != 3 or hist.shape[1:] != (4, BINS):
        raise ValueError(f"bands_from_hist: histograms of shape {hist.shape} are not [P,4,{BINS}]")
    total = hist.sum(axis=2)
    need = (total + 1) // 2
    cum = np.cumsum(hist, axis=2)
    m = np.argmax(cum >= np.maximum(need, 1)[..., None], axis=2).astype(np.int64)
    lo = m - (m >> BAND_SHIFT)
    hi = m + ((m + (1 << BAND_SHIFT) - 1) >> BAND_SHIFT)
    empty = total == 0
    band = np.stack([np.where(empty, 1, lo), np.where(empty, 0, hi)], axis=2).astype(np.int32)
    return band, np.where(empty, -1, m)


def gains_from_sums(sums) -> Tuple[np.ndarray, np.ndarray]:
    """sums int [P,4,3] = {count, sum qa, sum qb} -> (gain float64 [P,4], measured bool [P,4]): g = sum_b / sum_a where count
    >= MIN_COUNT (sum_a >= count * LEVEL_LO > 0 then); an unmeasured entry reads 1.0."""
    sums = np.asarray(sums).astype(np.int64)
    if sums.ndim != 3 or sums.shape[1:] != (4, 3):
        raise ValueError(f"gains_from_sums: sums of shape {sums.shape} are not [P,4,3]")
    measured = sums[..., 0] >= MIN_COUNT
    g = np.ones(sums.shape[:2], np.float64)
    g[measured] = sums[..., 2][measured].astype(np.float64) / sums[..., 1][measured].astype(np.float64)
    return g, measured


def pair_gains(gain, measured, mode: str) -> Tuple[np.ndarray, np.ndarray]:
    """The per-colour gain of every pair from the four ratio channels -> (float64 [P,3], measured bool [P]).  "exposure": the
    sum channel for all three colours; "rgb": each colour's own channel, measured only where all three are."""
    gain, measured = np.asarray(gain, np.float64), np.asarray(measured, bool)
    if mode == "rgb":
        ok = measured[:, :3].all(axis=1)
        g = gain[:, :3].copy()
    else:
        ok = measured[:, 3].copy()
        g = np.repeat(gain[:, 3:4], 3, axis=1)
    g[~ok] = 1.0
    return g, ok


def chain_segments(total_frames: int, linked, segments: Optional[Sequence[Tuple[int, int]]] = None) -> List[Tuple[int, int]]:
    """The frame ranges [s, e) over which exposure is chained: the shots, split further behind every pair that is not
    `linked` (confidence 0, unmeasured).  Exposure across them is unknown, so nothing is carried over."""
    linked = np.asarray(linked, bool).reshape(-1)
    out = []
    for s, e in (segments if segments is not None else [(0, total_frames)]):
        start = s
        for k in range(s, e - 1):
            if not linked[k]:
                out.append((start, k + 1))
                start = k + 1
        if e > start:
            out.append((start, e))
    return out


def corrections(pair_gain, linked, total_frames: int, radius: int,
                segments: Optional[Sequence[Tuple[int, int]]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (c float64 [N,3], clamped bool [N], L float64 [N,3]).  Inside a chain segment (chain_segments) L_i is the running
    sum of log g, starting at 0; L~_i the box mean of L over [i - r, i + r] clipped to the segment; c_i = exp(L~_i - L_i),
    clamped to CLAMP.  A frame alone in its segment gets exactly 1."""
    g = np.asarray(pair_gain, np.float64).reshape(total_frames - 1, 3)
    L = np.zeros((total_frames, 3), np.float64)
    c = np.ones((total_frames, 3), np.float64)
    for s, e in chain_segments(total_frames, linked, segments):
        if e - s < 2:
            continue
        L[s + 1:e] = np.cumsum(np.log(g[s:e - 1]), axis=0)
        prefix = np.concatenate([np.zeros((1, 3)), np.cumsum(L[s:e], axis=0)])
        for i in range(s, e):
            a, b = max(s, i - radius), min(e, i + radius + 1)
            c[i] = np.exp((prefix[b - s] - prefix[a - s]) / (b - a) - L[i])
    clamped = ((c < CLAMP[0]) | (c > CLAMP[1])).any(axis=1)
    return np.clip(c, CLAMP[0], CLAMP[1]), clamped, L


def step_rms(pair_gain, linked, correction=None) -> float:
    """The RMS log-gain step over the linked pairs and the three colours: of the measured chain, or, with `correction`
    [N,3], of the chain times the corrections (log g_k + log c_{k+1} - log c_k).  0.0 without a linked pair."""
    g = np.asarray(pair_gain, np.float64)
    linked = np.asarray(linked, bool)
    if not linked.any():
        return 0.0
    step = np.log(g)
    if correction is not None:
        lc = np.log(np.asarray(correction, np.float64))
        step = step + lc[1:] - lc[:-1]
    return float(np.sqrt(np.mean(step[linked] ** 2)))


def meta_block(request: Request, radius: int, pair_gain, measured, active, stats, inlier, correction, frames_clamped, values_clamped,
               rms_before: float, rms_after: float) -> Dict[str, Any]:
    """meta["deflicker"].  pair_gain [P,3] with None for a pair that is not linked (inactive or unmeasured); pairs_unmeasured
    counts the ACTIVE pairs with fewer than MIN_COUNT samples in the band; the fractions are means over the active / the
    measured pairs (0.0 where there is none); frames_clamped counts the frames whose correction hit CLAMP, values_clamped the
    values the apply pass held at 1.0."""
    measured, active = np.asarray(measured, bool), np.asarray(active, bool)
    stats = np.asarray(stats, np.int64).reshape(-1, 2)
    linked = measured & active
    well = np.where(stats[:, 0] > 0, stats[:, 1] / np.maximum(stats[:, 0], 1), 0.0)
    inl = np.asarray(inlier, np.float64)[linked]
    corr = np.asarray(correction, np.float64)
    return {
        "version": VERSION,
        "mode": request.mode,
        "window_s": float(request.window_s),
        "radius_frames": int(radius),
        "stride": STRIDE,
        "pair_gain": [[float(v) for v in row] if ok else None for row, ok in zip(np.asarray(pair_gain, np.float64), linked)],
        "pairs_unmeasured": int((active & ~measured).sum()),
        "well_exposed_fraction_mean": float(well[active].mean()) if active.any() else 0.0,
        "inlier_fraction_mean": float(inl.mean()) if inl.size else 0.0,
        "inlier_fraction_min": float(inl.min()) if inl.size else 0.0,
        "correction": [[float(v) for v in row] for row in corr],
        "correction_min": float(corr.min()),
        "correction_max": float(corr.max()),
        "frames_clamped": int(frames_clamped),
        "values_clamped": int(values_clamped),
        "step_rms_before": float(rms_before),
        "step_rms_after": float(rms_after),
    }


def solve(request: Request, hist_fn, sums_fn, confidences, total_frames: int, fps_effective: float,
          segments: Optional[Sequence[Tuple[int, int]]] = None):
    """Everything between the measurement and the apply pass -> (gains float32 [N,3] for the apply pass, finish), finish(values
    clamped) -> meta["deflicker"].  hist_fn(active u8 [P]) -> (hist [P,4,1024], stats [P,2]); sums_fn(active, band int32
    [P,4,2]) -> sums [P,4,3], as integers on the host: the two device passes, or their restatement."""
    active = active_pairs(confidences, total_frames, segments)
    act = active.astype(np.uint8)
    hist, stats = hist_fn(act)
    band, _ = bands_from_hist(hist)
    sums = np.asarray(sums_fn(act, band)).astype(np.int64)
    gain, ok = gains_from_sums(sums)
    pair_gain, measured = pair_gains(gain, ok, request.mode)
    linked = measured & active
    pair_gain[~linked] = 1.0
    radius = radius_frames(request.window_s, fps_effective)
    corr, clamped, _ = corrections(pair_gain, linked, total_frames, radius, segments)
    stats = np.asarray(stats).astype(np.int64).reshape(-1, 2)
    well = np.maximum(stats[:, 1], 1).astype(np.float64)
    counts = sums[..., 0].astype(np.float64)
    inlier = (counts[:, :3].min(axis=1) if request.mode == "rgb" else counts[:, 3]) / well
    gains32 = corr.astype(np.float32)
    rms_before = step_rms(pair_gain, linked)
    rms_after = step_rms(pair_gain, linked, gains32.astype(np.float64))

    def finish(values_clamped: int) -> Dict[str, Any]:
        return meta_block(request, radius, pair_gain, measured, active, stats, inlier, gains32, int(clamped.sum()), values_clamped,
                          rms_before, rms_after)

    return gains32, finish


def deflicker_on_device(ctx, request: Request, device_frames, dst, mask, transitions, confidences, fps_effective: float,
                        segments: Optional[Sequence[Tuple[int, int]]] = None) -> Dict[str, Any]:
    """Measures on `device_frames` (the source clip, f32 [N,H,W,3] on the device) through `transitions` (f32 [N-1,3,3], full
    resolution), applies the corrections to `dst` in place under `mask` (None: every pixel is own) -> meta["deflicker"].
    Three launches and two small downloads; a clip whose corrections are all exactly 1 launches no apply kernel."""
    transitions = np.ascontiguousarray(transitions, dtype=np.float32).reshape(-1, 3, 3)
    total_frames = int(device_frames.shape[0])

    def hist_fn(active):
        hist, stats = ctx.pair_gain_hist_batch(device_frames, transitions, active)
        return hist.cpu().numpy(), stats.cpu().numpy()

    def sums_fn(active, band):
        return ctx.pair_gain_sums_batch(device_frames, transitions, band, active).cpu().numpy()

    gains, finish = solve(request, hist_fn, sums_fn, confidences, total_frames, fps_effective, segments)
    clamped = ctx.apply_gain_batch(dst, gains, mask)
    return finish(int(clamped.cpu().numpy().astype(np.int64).sum()))
