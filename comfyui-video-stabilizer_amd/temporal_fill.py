"""Temporal fill: padding pixels of a stabilized frame are taken from neighbouring frames that saw the missing content.

An output pixel p of frame i that is padding has a known position in every other source frame j: with the final matrices
F_i (source i -> output canvas) and the full-resolution transitions A_i (x_{i+1} = A_i x_i),

    x_j = A_{j-1} ... A_i F_i^-1 p   (j > i),        x_j = A_j^-1 ... A_{i-1}^-1 F_i^-1 p   (j < i),

i.e. source frame j reaches the canvas of frame i through the FORWARD matrix

    H_{i,j} = F_i (A_{j-1} ... A_i)^-1   (j > i),    H_{i,j} = F_i A_{i-1} ... A_j   (j < i).

`fill_candidates` forms these on the host (NumPy float64, one cast to float32); the kernel behind
`native.Context.temporal_fill_batch` (csrc/vstab_neighbour.hip: temporal_fill_kernel) warps the first candidate whose every
interpolation tap lies inside its frame into the pixel -- see include/vstab.h for the exact rule.  Off by default.

That fill is a hard cut: a neighbour's raw value next to the frame's own content.  Two options, each off by default and each
working without the other, go through `native.Context.temporal_fill_blend_batch` instead (temporal_fill_blend_kernel):
`exposure` scales what candidate j supplies to frame i by one gain per channel, the ratio of the two frames' sums over the
lattice of pixels both see (`native.Context.fill_gain_sums`, then `gains_from_sums`), and `feather` cross-fades the frame's own
pixels within that many source pixels of its border into the candidate, which also replaces the ring of own pixels the
padding colour was interpolated into.  include/vstab.h states both rules.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np

MAX_RADIUS = 32   # K = 2 * radius candidates per frame; the kernel takes K <= 64
MAX_FEATHER = 64          # VSTAB_FILL_FEATHER_MAX
DEFAULT_FEATHER = 16      # fill_feather=True
# Choices, not calibrations (like the lattice stride of 8, VSTAB_FILL_GAIN_STRIDE): a gain needs an overlap of at least
# GAIN_MIN_COUNT lattice pixels (a 45 x 45 px patch) and stays within one photographic stop either way.
GAIN_MIN_COUNT = 32
GAIN_CLAMP = (0.5, 2.0)


def _finite(m: np.ndarray) -> bool:
    return bool(np.isfinite(m).all())


def fill_candidates(final_matrices, transitions, confidences, radius: int, first: int = 0, count: Optional[int] = None,
                    min_confidence: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """-> (matrices float32 [n, K, 3, 3], cand_frame int32 [n, K]) for output frames [first, first + count), K = 2 * radius.

    final_matrices [N,3,3] float32, transitions [N-1,3,3] float32 (x_{i+1} = A_i x_i), confidences [N-1].
    Candidate order: temporal distance d = 1 .. radius, and for equal d the earlier frame (i - d) before the later (i + d)
    -- nearest in time first, because the chain's error grows with d.  cand_frame is -1 (and the matrix the identity) where
    j lies outside the clip, where the chain i -> j crosses a transition whose confidence is <= min_confidence (the
    "no estimate" identity records), or where a matrix on the way is singular or not finite.  Pure NumPy float64 from the
    float32 inputs, cast once to float32; no GPU."""
    radius = int(radius)
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"temporal fill radius {radius} outside [1, {MAX_RADIUS}]")
    F = np.asarray(final_matrices, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    total = F.shape[0]
    A = np.asarray(transitions, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    conf = np.asarray(confidences, dtype=np.float64).reshape(-1)
    if A.shape[0] != max(total - 1, 0) or conf.shape[0] != A.shape[0]:
        raise ValueError(f"temporal fill: {total} frames need {max(total - 1, 0)} transitions and confidences, "
                         f"got {A.shape[0]} and {conf.shape[0]}")
    count = total - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > total:
        raise ValueError(f"temporal fill: frames [{first}, {first + count}) outside a clip of {total}")
    usable = [bool(c > min_confidence) and _finite(a) for c, a in zip(conf, A)]   # NaN confidence compares false

    K = 2 * radius
    mats = np.tile(np.eye(3, dtype=np.float32), (count, K, 1, 1))
    cand = np.full((count, K), -1, dtype=np.int32)

    def put(f, k, j, h64):
        if not _finite(h64):
            return False
        h32 = h64.astype(np.float32)
        if not _finite(h32):
            return False
        mats[f, k] = h32
        cand[f, k] = j
        return True

    for f in range(count):
        i = first + f
        if not _finite(F[i]):
            continue
        # earlier frames j = i - d: H = F_i A_{i-1} ... A_j  (slot 2 (d - 1))
        chain = None
        for d in range(1, radius + 1):
            j = i - d
            if j < 0 or not usable[j]:
                break
            chain = A[j] if chain is None else chain @ A[j]
            if not _finite(chain) or np.linalg.det(chain) == 0.0:   # a singular chain maps frame j onto a line: no candidate
                break
            if not put(f, 2 * (d - 1), j, F[i] @ chain):
                break
        # later frames j = i + d: H = F_i (A_{j-1} ... A_i)^-1  (slot 2 (d - 1) + 1)
        chain = None
        for d in range(1, radius + 1):
            j = i + d
            if j >= total or not usable[j - 1]:
                break
            chain = A[j - 1] if chain is None else A[j - 1] @ chain
            try:
                inv = np.linalg.inv(chain)
            except np.linalg.LinAlgError:
                break
            if not put(f, 2 * (d - 1) + 1, j, F[i] @ inv):
                break
    return mats, cand


# ---- from a Flow / Classic meta ---------------------------------------------------------------------------------------
def plan_from_meta(meta: Any) -> Dict[str, Any]:
    """What the fill needs from a Flow / Classic node's meta JSON: final matrices (`stabilization_warp`), transitions and
    confidences (`estimated_motion.per_transition`), sizes.  A meta without them (Motion Apply's, bypass metas) raises a
    ValueError naming the missing key."""
    if not isinstance(meta, dict):
        raise ValueError("temporal fill: meta must be the JSON dictionary of a Flow / Classic stabilizer node")
    warp = meta.get("stabilization_warp")
    if not isinstance(warp, dict) or not isinstance(warp.get("per_frame"), list):
        raise ValueError("temporal fill: meta has no 'stabilization_warp' with 'per_frame' matrices")
    motion = meta.get("estimated_motion")
    if not isinstance(motion, dict) or not isinstance(motion.get("per_transition"), list):
        raise ValueError("temporal fill: meta has no 'estimated_motion' with 'per_transition' records "
                         "(Motion Apply and bypass metas carry no transitions)")
    try:
        final = np.array([e["applied_matrix"] for e in warp["per_frame"]], dtype=np.float32).reshape(-1, 3, 3)
    except KeyError as exc:
        raise ValueError(f"temporal fill: a 'stabilization_warp.per_frame' entry has no {exc.args[0]!r}") from None
    per = motion["per_transition"]
    try:
        trans = np.array([e["matrix"] for e in per], dtype=np.float32).reshape(-1, 3, 3)
        conf = np.array([e["confidence"] for e in per], dtype=np.float64)
    except KeyError as exc:
        raise ValueError(f"temporal fill: an 'estimated_motion.per_transition' entry has no {exc.args[0]!r}") from None
    if len(final) < 2 or len(trans) != len(final) - 1:
        raise ValueError(f"temporal fill: meta has {len(final)} frame matrices and {len(trans)} entries in "
                         "'estimated_motion.per_transition' (frames - 1 are needed)")
    for key in ("source_size", "output_size"):
        if key not in warp:
            raise ValueError(f"temporal fill: 'stabilization_warp' has no {key!r}")
    return {"final_matrices": final, "transitions": trans, "confidences": conf,
            "source_size": (int(warp["source_size"][0]), int(warp["source_size"][1])),
            "output_size": (int(warp["output_size"][0]), int(warp["output_size"][1]))}


def fill_meta(radius: int, fill_counts, pad_counts, output_size) -> Dict[str, Any]:
    """The `temporal_fill` meta block from the kernel's per-frame counts (fractions formed like `padding_fraction_*`:
    float32 count / float32 pixels)."""
    pixels = np.float32(int(output_size[0]) * int(output_size[1]))
    filled = (np.asarray(fill_counts, dtype=np.int64).astype(np.float32) / pixels).astype(np.float64)
    left = (np.asarray(pad_counts, dtype=np.int64).astype(np.float32) / pixels).astype(np.float64)
    return {"radius": int(radius),
            "filled_fraction_mean": float(np.mean(filled)), "filled_fraction_max": float(np.max(filled)),
            "padding_fraction_mean_after": float(np.mean(left)), "padding_fraction_max_after": float(np.max(left))}


def gains_from_sums(sums) -> np.ndarray:
    """sums [n,K,7] (count, own r g b, candidate r g b: vstab_fill_gain_sums) -> gains float32 [n,K,3], formed in float64:
    g_c = own_c / cand_c, clamped to GAIN_CLAMP, where count >= GAIN_MIN_COUNT and cand_c >= 1; 1.0 otherwise.  The gain
    relates candidate j to frame i directly, over their own overlap: nothing accumulates along a chain."""
    s = np.asarray(sums).astype(np.float64)
    if s.ndim != 3 or s.shape[2] != 7:
        raise ValueError(f"temporal fill: gain sums {s.shape} are not [n, K, 7]")
    own, cand = s[..., 1:4], s[..., 4:7]
    ok = (s[..., 0:1] >= GAIN_MIN_COUNT) & (cand >= 1.0)
    ratio = np.clip(own / np.where(ok, cand, 1.0), GAIN_CLAMP[0], GAIN_CLAMP[1])
    return np.where(ok, ratio, 1.0).astype(np.float32)


def check_blend_request(temporal_fill: int, fill_feather=None, fill_exposure=False, subpix=None):
    """-> (feather px | None, exposure bool) of a `fill_feather` / `fill_exposure` request; None, False = neither.
    fill_feather: None (or False) is off, True is DEFAULT_FEATHER px, an int in 0..MAX_FEATHER is that width.  Everything is
    checked here, before any GPU work: either option needs temporal_fill > 0 and the 'q5' sub-pixel mode."""
    if fill_feather is None or fill_feather is False:
        feather = None
    elif fill_feather is True:
        feather = DEFAULT_FEATHER
    elif isinstance(fill_feather, (int, np.integer)) and 0 <= int(fill_feather) <= MAX_FEATHER:
        feather = int(fill_feather)
    else:
        raise ValueError(f"fill_feather={fill_feather!r} is not None, True or an integer in 0..{MAX_FEATHER}")
    if not isinstance(fill_exposure, (bool, np.bool_)):
        raise ValueError(f"fill_exposure={fill_exposure!r} is not a bool")
    exposure = bool(fill_exposure)
    if feather is None and not exposure:
        return None, False
    if int(temporal_fill) <= 0:
        raise ValueError(f"fill_feather={fill_feather!r} / fill_exposure={fill_exposure!r} need temporal_fill > 0: they change how the "
                         "temporal fill writes its pixels")
    if subpix is None:
        from . import native
        subpix = native.DEFAULT_SUBPIX
    if subpix != "q5":
        raise ValueError(f"fill_feather / fill_exposure are not supported in sub-pixel mode {subpix!r}: the blended fill is stated on "
                         "the 1/32-px coordinates of 'q5'")
    return feather, exposure


def blend_meta(feather_px: int, blend_counts, output_size, matched: bool, gains, counted, cand_frame) -> Dict[str, Any]:
    """The keys the blended fill adds to the `temporal_fill` block.  gains [n,K,3]; counted [n,K] bool: the candidate's overlap
    reached GAIN_MIN_COUNT (None without exposure matching); gain_min / gain_max run over those candidates."""
    pixels = np.float32(int(output_size[0]) * int(output_size[1]))
    blended = (np.asarray(blend_counts, dtype=np.int64).astype(np.float32) / pixels).astype(np.float64)
    exposure = {"matched": bool(matched), "gain_min": 1.0, "gain_max": 1.0, "candidates_without_overlap": 0}
    if matched:
        present = np.asarray(cand_frame) >= 0
        used = present & np.asarray(counted, dtype=bool)
        if used.any():
            g = np.asarray(gains, dtype=np.float32)[used]
            exposure["gain_min"], exposure["gain_max"] = float(g.min()), float(g.max())
        exposure["candidates_without_overlap"] = int((present & ~used).sum())
    return {"feather_px": int(feather_px), "blended_fraction_mean": float(np.mean(blended)),
            "blended_fraction_max": float(np.max(blended)), "exposure": exposure}


def fill_on_device(ctx, device_frames, dst, mask, final_matrices, transitions, confidences, radius: int,
                   interp: str = "bilinear", subpix=None, feather=None, exposure=False) -> Dict[str, Any]:
    """Runs the fill over a whole clip in place (dst [N,h,w,3], mask [N,h,w], device) and returns the meta block.
    feather (px, None = off) or exposure=True switch to the blended entry; exposure off means gains of 1, exposure on the
    sums launch in front of the fill, one small download and `gains_from_sums`."""
    mats, cand = fill_candidates(final_matrices, transitions, confidences, radius)
    if feather is None and not exposure:
        _, fill_count, pad_count = ctx.temporal_fill_batch(device_frames, mats, cand, dst, mask, first=0, interp=interp, subpix=subpix)
        counts = ctx.torch.stack([fill_count, pad_count]).cpu().numpy()
        return fill_meta(radius, counts[0], counts[1], (dst.shape[2], dst.shape[1]))
    feather_px = 0 if feather is None else int(feather)
    own = np.asarray(final_matrices, dtype=np.float32).reshape(-1, 3, 3)
    gains, counted = np.ones(cand.shape + (3,), np.float32), None
    if exposure:
        sums = ctx.fill_gain_sums(device_frames, mats, cand, own, dst, first=0, interp=interp, subpix=subpix).cpu().numpy()
        gains, counted = gains_from_sums(sums), sums[..., 0] >= GAIN_MIN_COUNT
    _, fill_count, pad_count, blend_count = ctx.temporal_fill_blend_batch(
        device_frames, mats, cand, own, gains, dst, mask, feather_px=feather_px, first=0, interp=interp, subpix=subpix)
    counts = ctx.torch.stack([fill_count, pad_count, blend_count]).cpu().numpy()
    size = (dst.shape[2], dst.shape[1])
    block = fill_meta(radius, counts[0], counts[1], size)
    block.update(blend_meta(feather_px, counts[2], size, bool(exposure), gains, counted, cand))
    return block
