"""Drift correction (beyond the reference): register every frame directly against a keyframe, so that the absolute pose of
frame i is a chain of i / S keyframe alignments instead of i consecutive-pair estimates whose bias adds up.

The alignment is inverse-compositional Gauss-Newton on the estimation images the gray pass already made.  Its normal
equations are exact integer sums over pixels (csrc/vstab_anchor.hip; the rule and its two forms are stated once, in
include/vstab.h); everything here is float64 arithmetic on those numbers, driven by a `sums_fn` callable: the kernel in the
pipeline, the NumPy restatement in the CPU suite.  The plain rule gives 17 numbers per frame
(`native.Context.anchor_sums_batch`); exposure matching (`drift_exposure`) and the subject mask (`drift_mask`) use the second
form (`native.Context.anchor_sums_ex_batch`, 31 numbers).  The plain rule is the second form at unit gain without a mask, so
there is one loop, `refine_ex`, on the 31; `refine` puts the plain rule's 17 into their places among them.

The update.  T is the template (the anchor's image), I the frame's, R maps an anchor pixel into the frame, and W(d) moves a
template pixel p = (x, y) about the image centre c = ((w-1)/2, (h-1)/2):
    W(d): p -> p + (d0 + d2 xc - d3 yc,  d1 + d3 xc + d2 yc),   (xc, yc) = p - c.
The model is I(R p) = g T(W(d) p) + o; the plain rule holds g = 1, o = 0.  The kernel has the integers G = 1024 g and
O = 1024 o of the current estimate and forms r = v - G T - O with v = 1024 I(R p).  To first order T(W(d) p) = T(p) +
grad T . (dW/dd) d, and with the central differences grad T = (gx / 2, gy / 2) and xc = u / 2, yc = q / 2 the true Jacobian
is D J, D = diag(1/2, 1/2, 1/4, 1/4), of the rule's integer J: grad T . (dW/dd) d = J[0..3] . d' with d' = D d, hence
d = (2 d'0, 2 d'1, 4 d'2, 4 d'3).  With the gain off by dg and the offset by do, I - g T - o = dg T + do + (g + dg) J . d';
times 1024, r = dG T + dO + (G + dG) (J[0..3] . d'), dG = 1024 dg, dO = 1024 do.  That is linear in
theta = ((G + dG) d'_0..3, dG, dO) with the columns (J0, J1, J2, J3, T, 1): H6 theta = b6 and d'_k = theta_k / (G + dG).
Without exposure matching G = 1024 and dG = dO = 0 are held, and the first four rows are H d' = b / 1024.  Substituting
p' = W(d) p gives I(R W(d)^-1 p') = g T(p') + o: the update is R <- R W(d)^-1."""

from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

# Choices, not calibrations: they bound the work and say when to distrust a result; none was fitted to a clip.
DEFAULT_SPACING = 32         # frames between keyframes
MAX_ITERATIONS = 6           # launches that solve; one more evaluates the result
CONVERGED_PX = 0.005         # an update that moves no corner this far ends a frame's iterations
MIN_OVERLAP = 0.5            # of the (w-2)(h-2) template pixels that must still take part
MAX_CORRECTION_PX = 4.0      # working px a corner may move in total: more than that is not drift
RESIDUAL_CAP = 32            # grey levels; a pixel further off is a moving subject, not the camera
MIN_SPACING, MAX_SPACING = 2, 4096
MODES = ("translation", "similarity")
KEEP_REASONS = ("singular", "overlap", "cost", "step", "no_anchor")
SLOTS = 17
# The exposure-matched / masked form.  Choices as well: the gain range is the temporal fill's [0.5, 2] clamp, 64 grey levels is a
# quarter of the range (no auto-exposure step between two frames a spacing apart adds that much), and the first launch of an
# exposure-matched call runs uncapped because no gain has been estimated yet that the cap could be applied behind.
SLOTS_EX = 31
GAIN_UNIT = 1024             # G and O are integers in units of 1/1024 (of 1, of a grey level)
GAIN_MIN, GAIN_MAX = 512, 2048
MAX_OFFSET_LEVELS = 64
BOOTSTRAP_CAP = 255          # caps nothing at G = 1024, O = 0
KEEP_REASONS_EX = KEEP_REASONS + ("gain",)
# the 31 slots: count, capped, masked, sum|r|, b0..b5, then J_j J_k for j <= k row-major
_H_SLOT = {}
for _j in range(6):
    for _k in range(_j, 6):
        _H_SLOT[(_j, _k)] = 10 + len(_H_SLOT)
PLAIN_SLOTS = [0, 1, 3, 4, 5, 6, 7] + [_H_SLOT[(j, k)] for j in range(4) for k in range(j, 4)]   # the 17 of the plain rule


def check_request(value) -> Optional[int]:
    """The `drift_correction` keyword -> the keyframe spacing, or None for off (None / 0 / False)."""
    if value is None or value is False or (isinstance(value, (int, np.integer)) and not isinstance(value, bool) and int(value) == 0):
        return None
    if value is True:
        return DEFAULT_SPACING
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool) and MIN_SPACING <= int(value) <= MAX_SPACING:
        return int(value)
    raise ValueError(f"drift_correction={value!r}: expected None / False / 0 (off), True (a keyframe every {DEFAULT_SPACING} frames) "
                     f"or an int in {MIN_SPACING}..{MAX_SPACING}, the keyframe spacing.")


def check_options(drift, drift_exposure, drift_mask, estimation_mask):
    """The `drift_exposure` / `drift_mask` keywords -> (exposure, masked) as bools.  None / False: off."""
    for name, value in (("drift_exposure", drift_exposure), ("drift_mask", drift_mask)):
        if value is not None and not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{name}={value!r}: expected None / False (off) or True.")
    exposure, masked = bool(drift_exposure), bool(drift_mask)
    for name, on in (("drift_exposure", exposure), ("drift_mask", masked)):
        if on and drift is None:
            raise ValueError(f"{name}=True needs drift_correction: it changes how the keyframe alignment is solved, and without "
                             "drift_correction there is none.")
    if masked and estimation_mask is None:
        raise ValueError("drift_mask=True needs estimation_mask: the keyframe alignment leaves out the pixels that mask's block "
                         "grid names, and without estimation_mask there is no grid.")
    return exposure, masked


def check_pipeline(transform_mode: str, subject: bool, estimation_mask, drift_mask: bool = False) -> None:
    """What drift correction cannot be combined with; each refusal says why.  drift_mask: the alignment reads the estimation
    mask's block grid, so the mask is no obstacle."""
    if transform_mode == "perspective":
        raise ValueError("drift_correction does not support transform_mode='perspective': the keyframe alignment updates a "
                         "similarity (shift, zoom, rotation); use 'translation' or 'similarity'.")
    if subject:
        raise ValueError("drift_correction does not support estimator='subject': its transitions follow the subject, while the "
                         "estimation images the keyframe alignment reads show the background.")
    if estimation_mask is not None and not drift_mask:
        raise ValueError("drift_correction does not support estimation_mask: the keyframe alignment has no per-pixel exclusion "
                         "yet (its residual cap is the only guard against moving subjects).")


# ---------------------------------------------------------------------------------------------------------- schedule
@dataclass
class Schedule:
    anchor: np.ndarray           # int64 [N]: the frame each frame is registered against, -1 for none
    keyframes: List[int]         # every keyframe of the clip, ascending (each anchoring segment's first frame is one)
    shot_start: np.ndarray       # bool [N]: the pose restarts at the identity here
    spacing: int


def schedule(total_frames: int, segments, confidences, S: int) -> Schedule:
    """Anchoring segments are the shots, split further at every pair whose selected transition has confidence 0.  In a
    segment starting at s the keyframes are s, s+S, s+2S, ...; a keyframe's anchor is the previous keyframe, any other
    frame's the latest keyframe before it, the segment's first frame has none."""
    n = int(total_frames)
    conf = np.asarray(confidences, dtype=np.float64).reshape(-1)
    if conf.shape[0] != max(n - 1, 0):
        raise ValueError(f"schedule: {conf.shape[0]} confidences for {n} frames")
    shots = [(0, n)] if segments is None else [(int(s), int(e)) for s, e in segments]
    anchor = np.full(n, -1, np.int64)
    shot_start = np.zeros(n, bool)
    keyframes: List[int] = []
    for s, e in shots:
        if e <= s:
            continue
        shot_start[s] = True
        starts = [s] + [k + 1 for k in range(s, e - 1) if conf[k] == 0.0]
        for a, b in zip(starts, starts[1:] + [e]):
            for i in range(a, b):
                if (i - a) % S == 0:
                    keyframes.append(i)
                    anchor[i] = i - S if i > a else -1
                else:
                    anchor[i] = a + ((i - a) // S) * S
    return Schedule(anchor, keyframes, shot_start, int(S))


# ---------------------------------------------------------------------------------------------------------- refinement
def _affine3(m23: np.ndarray) -> np.ndarray:
    out = np.zeros(m23.shape[:-2] + (3, 3), np.float64)
    out[..., :2, :] = m23
    out[..., 2, 2] = 1.0
    return out


def chained(work_mats, sched: Schedule) -> np.ndarray:
    """R_i of the chain: the product of the selected working-resolution transitions from the anchor to i -> f64 [N,2,3]
    (the identity where there is no anchor)."""
    mats = np.asarray(work_mats, dtype=np.float64).reshape(-1, 3, 3)
    n = sched.anchor.shape[0]
    R = np.tile(np.eye(3)[:2], (n, 1, 1))
    for i in range(n):
        a = int(sched.anchor[i])
        if a < 0:
            continue
        # the anchor is at most S frames back: R_i = A_{i-1} R_{i-1} where i-1 shares the anchor, else the plain product
        if i - 1 > a and int(sched.anchor[i - 1]) == a:
            R[i] = (mats[i - 1] @ _affine3(R[i - 1]))[:2]
        else:
            acc = np.eye(3)
            for k in range(a, i):
                acc = mats[k] @ acc
            R[i] = acc[:2]
    return R


def warp_matrix(d, size) -> np.ndarray:
    """W(d) as a 3x3: p -> p + (d0 + d2 xc - d3 yc, d1 + d3 xc + d2 yc) about the image centre."""
    w, h = size
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    L = np.array([[1.0 + d[2], -d[3]], [d[3], 1.0 + d[2]]])
    t = np.array([d[0], d[1]]) + np.array([cx, cy]) - L @ np.array([cx, cy])
    out = np.eye(3)
    out[:2, :2], out[:2, 2] = L, t
    return out


def solve_update(sums, mode: str):
    """One frame's 17 numbers -> d (4 values; zoom and rotation 0 in translation mode), or None where H is not positive
    definite."""
    s = [float(int(v)) for v in sums]
    H = np.array([[s[7], s[8], s[9], s[10]], [s[8], s[11], s[12], s[13]], [s[9], s[12], s[14], s[15]], [s[10], s[13], s[15], s[16]]])
    b = np.array(s[3:7]) / 1024.0
    k = 2 if mode == "translation" else 4
    dp = _solve_scaled(H[:k, :k], b[:k])
    if dp is None:
        return None
    d = np.zeros(4)
    d[:2] = 2.0 * dp[:2]
    if k == 4:
        d[2:] = 4.0 * dp[2:]
    return d


def _solve_scaled(H: np.ndarray, b: np.ndarray):
    """H x = b for a symmetric H that must be positive definite -> x, or None where it is not.
    Scaled to a unit diagonal first: the zoom / rotation rows are ~1e5 times the shift rows, and the test is on the shape.
    Positive definite here means: the Cholesky factor exists and no pivot of the scaled matrix is below 1e-6 (a choice:
    below that the solution has no correct digit left in float64 after the two triangular solves' 1e-12 amplification)."""
    diag = np.diag(H)
    if not (diag > 0.0).all():
        return None
    e = 1.0 / np.sqrt(diag)
    Hs = H * e[:, None] * e[None, :]
    try:
        Lc = np.linalg.cholesky(Hs)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(Lc).all() or np.min(np.diag(Lc)) < 1e-6:
        return None
    return e * np.linalg.solve(Lc.T, np.linalg.solve(Lc, e * b))


def solve_update_ex(sums, mode: str, gain: int, exposure: bool):
    """One frame's 31 numbers, taken at the integer gain G -> (d, dG, dO), or None where H is not positive definite.
    exposure False (the mask alone): today's columns from the new slots; the sums were taken at G = 1024, O = 0, and dG = dO
    = 0.  exposure True: H6 theta = b6 over the columns (J0..J3, T, 1) -- (J0, J1, T, 1) in translation mode -- with
    theta = ((G + dG) d', dG, dO)."""
    if not exposure:
        d = solve_update([sums[k] for k in PLAIN_SLOTS], mode)
        return None if d is None else (d, 0.0, 0.0)
    s = [float(int(v)) for v in sums]
    cols = (0, 1, 4, 5) if mode == "translation" else (0, 1, 2, 3, 4, 5)
    H = np.array([[s[_H_SLOT[(min(j, k), max(j, k))]] for k in cols] for j in cols])
    b = np.array([s[4 + k] for k in cols])
    theta = _solve_scaled(H, b)
    if theta is None:
        return None
    dG, dO = float(theta[-2]), float(theta[-1])
    scale = float(gain) + dG
    if not scale > 0.0:
        return None
    dp = theta[:-2] / scale
    d = np.zeros(4)
    d[:2] = 2.0 * dp[:2]
    if len(cols) == 6:
        d[2:] = 4.0 * dp[2:]
    return d, dG, dO


ROUNDING_LATTICE = 8         # the mean rounding displacement is taken over every 8th template pixel per axis


def sampled_at(R23: np.ndarray, size) -> np.ndarray:
    """The matrix the sums were really taken at.  The rule rounds every sample position to 1/32 px, so a template pixel p
    is looked up at R p + e(p), |e| <= 1/64 px per axis.  Under a rotation or a zoom e differs from pixel to pixel and its
    mean is ~0; under a pure shift -- translation mode, or a similarity whose 2x2 part is within ~1e-5 of the identity --
    every pixel rounds alike and the sums are those of the shift moved by e.  The update the sums give starts from R plus
    the mean of e (the shift closest to the field e in the least-squares sense), taken over a lattice of the template's
    pixels.  Applied to R itself it would leave e in place, and the iterations would hop between two cells of the 1/32 grid
    without ever converging."""
    R23 = np.asarray(R23, dtype=np.float64)
    w, h = size
    y, x = np.meshgrid(np.arange(1, max(h - 1, 2), ROUNDING_LATTICE, dtype=np.float64),
                       np.arange(1, max(w - 1, 2), ROUNDING_LATTICE, dtype=np.float64), indexing="ij")
    out = R23.copy()
    with np.errstate(all="ignore"):
        for row in (0, 1):
            pos = (R23[row, 0] * x + R23[row, 1] * y) + R23[row, 2]          # the rule's association
            mean = float(np.mean(np.rint(32.0 * pos) / 32.0 - pos))
            if np.isfinite(mean):
                out[row, 2] += mean
    return out


def _corners(size) -> np.ndarray:
    w, h = size
    return np.array([[0.0, 0.0, 1.0], [w - 1.0, 0.0, 1.0], [0.0, h - 1.0, 1.0], [w - 1.0, h - 1.0, 1.0]]).T


def corner_distance(Ra, Rb, size) -> float:
    """The largest distance between the images of the four frame corners under two 2x3 matrices."""
    c = _corners(size)
    return float(np.max(np.hypot(*(np.asarray(Ra) @ c - np.asarray(Rb) @ c))))


@dataclass
class Refinement:
    R: np.ndarray                # f64 [N,2,3]: the matrices to use (the chained one where a frame was kept)
    R_chained: np.ndarray
    reason: List[Optional[str]]  # per frame: None = refined, else one of KEEP_REASONS
    launches: int
    iterations: int
    sums_first: np.ndarray       # int64 [N,17] (PLAIN_SLOTS) at the chained matrices: the launch the cost test starts from
    sums_final: np.ndarray       # int64 [N,17] at the refined ones (zeros where none was evaluated)
    # the exposure-matched / masked form only (None from `refine`)
    gain: Optional[np.ndarray] = None        # int64 [N]: G per frame, 1024 where the frame was kept or has no anchor
    offset: Optional[np.ndarray] = None      # int64 [N]: O per frame
    masked_first: Optional[np.ndarray] = None    # int64 [N]: the masked pixels of that launch
    before_launch: int = 1                   # which launch sums_first is, counted from 1


def refine(sums_fn, work_mats, sched: Schedule, mode: str, size) -> Refinement:
    """The plain rule: sums_fn(anchor, R) -> int64 [N,17], taken at RESIDUAL_CAP.  It is the second form at G = 1024, O = 0
    without a mask, so its 17 numbers go to their places among the 31 and `refine_ex` runs without exposure."""
    n = sched.anchor.shape[0]

    def sums_ex_fn(anchor, R, gain, offset, cap):
        sums = np.zeros((n, SLOTS_EX), np.int64)
        sums[:, PLAIN_SLOTS] = np.asarray(sums_fn(anchor, R), dtype=np.int64).reshape(n, SLOTS)
        return sums

    return replace(refine_ex(sums_ex_fn, work_mats, sched, mode, size, exposure=False), gain=None, offset=None, masked_first=None)


def refine_ex(sums_fn, work_mats, sched: Schedule, mode: str, size, exposure: bool) -> Refinement:
    """Gauss-Newton on every anchored frame at once, on the 31 numbers of the second form: sums_fn(anchor, R, gain, offset,
    cap) -> int64 [N,31], with or without a mask behind it.  At most MAX_ITERATIONS launches that solve, converged frames
    drop out (anchor -1), one more launch evaluates the result, then the tests that keep a frame's chained matrix.
    The kernel always sees the integers held here: G <- rint(G + dG), O <- rint(O + dO) after every solve.
    exposure: the first launch is the bootstrap.  At G = 1024 an exposure step pushes most pixels over the cap before any gain
    is known, so that launch runs with BOOTSTRAP_CAP (which caps nothing) and only its gain and offset are taken: uncapped sums
    hold every moving subject, so the motion they give is not applied, and R stays the chained matrix.  Every later launch and
    the evaluating one run with RESIDUAL_CAP.  The second launch is therefore the chained matrix under the estimated exposure,
    and the cost test compares it with the last launch, both under the same cap (`before_launch` = 2).  Without exposure the
    gain stays 1024 / 0, every launch runs with RESIDUAL_CAP and the cost test starts from the first launch."""
    if mode not in MODES:
        raise ValueError(f"drift correction: mode {mode!r} is not one of {MODES}")
    w, h = size
    anchor = sched.anchor
    n = anchor.shape[0]
    R0 = chained(work_mats, sched)
    R = R0.copy()
    G = np.full(n, GAIN_UNIT, np.int64)
    O = np.zeros(n, np.int64)
    reason: List[Optional[str]] = [None if a >= 0 else "no_anchor" for a in anchor.tolist()]
    active = anchor >= 0
    before_at = 1 if exposure else 0
    before = np.zeros((n, SLOTS_EX), np.int64)
    launches = iterations = 0

    def launch(rows, cap):
        return np.asarray(sums_fn(np.where(rows, anchor, -1), R.reshape(n, 6), G.copy(), O.copy(), cap), dtype=np.int64).reshape(n, SLOTS_EX)

    for it in range(MAX_ITERATIONS):
        if not active.any():
            break
        bootstrap = exposure and it == 0
        sums = launch(active, BOOTSTRAP_CAP if bootstrap else RESIDUAL_CAP)
        launches += 1
        iterations += 1
        if it == before_at:
            before = sums.copy()
        for i in np.nonzero(active)[0].tolist():
            solved = solve_update_ex(sums[i], mode, int(G[i]), exposure)
            if solved is None:
                reason[i], active[i] = "singular", False
                continue
            d, dG, dO = solved
            if exposure:
                g_new, o_new = float(np.rint(G[i] + dG)), float(np.rint(O[i] + dO))
                if not (GAIN_MIN <= g_new <= GAIN_MAX and abs(o_new) <= MAX_OFFSET_LEVELS * GAIN_UNIT):
                    reason[i], active[i] = "gain", False      # (NaN fails the comparisons too); G and O keep their last values
                    continue
                G[i], O[i] = int(g_new), int(o_new)
            if bootstrap:
                continue
            new = (_affine3(sampled_at(R[i], size)) @ np.linalg.inv(warp_matrix(d, size)))[:2]
            moved = corner_distance(new, R[i], size)
            R[i] = new
            if moved < CONVERGED_PX:
                active[i] = False
    final = np.zeros((n, SLOTS_EX), np.int64)
    evaluate = np.array([r is None for r in reason])
    if evaluate.any():
        final = launch(evaluate, RESIDUAL_CAP)
        launches += 1
    need = MIN_OVERLAP * (w - 2) * (h - 2)
    for i in np.nonzero(evaluate)[0].tolist():
        count0, sum0, count1, sum1 = int(before[i, 0]), int(before[i, 3]), int(final[i, 0]), int(final[i, 3])
        if count1 < need:
            reason[i] = "overlap"
        elif sum1 * count0 > sum0 * count1:          # the mean |r| went up: integers, no division
            reason[i] = "cost"
        elif corner_distance(R[i], R0[i], size) > MAX_CORRECTION_PX:
            reason[i] = "step"
    for i, r in enumerate(reason):
        if r is not None:
            R[i], G[i], O[i] = R0[i], GAIN_UNIT, 0
    return Refinement(R, R0, reason, launches, iterations, before[:, PLAIN_SLOTS], final[:, PLAIN_SLOTS], G, O, before[:, 2].copy(),
                      before_at + 1)


# ---------------------------------------------------------------------------------------------------------- poses
def poses(R, sched: Schedule) -> np.ndarray:
    """C_i = R_i C_anchor(i) along the keyframes -> f64 [N,3,3], working resolution.  Every shot starts at the identity;
    across a confidence-0 pair inside a shot the pose continues as under the identity."""
    n = sched.anchor.shape[0]
    C = np.tile(np.eye(3), (n, 1, 1))
    for i in range(n):
        a = int(sched.anchor[i])
        if a >= 0:
            C[i] = _affine3(np.asarray(R[i], dtype=np.float64)) @ C[a]
        elif not sched.shot_start[i]:
            C[i] = C[i - 1]
    return C


def transitions(C) -> np.ndarray:
    """A'_k = C_{k+1} C_k^-1 in float64 -> [N-1,3,3]."""
    C = np.asarray(C, dtype=np.float64)
    if C.shape[0] < 2:
        return np.zeros((0, 3, 3))
    return np.matmul(C[1:], np.linalg.inv(C[:-1]))


_MODE_INDEX = {"translation": 0, "similarity": 1, "perspective": 2}


def write_transitions(fit_records: np.ndarray, A, modes: Sequence[str], confidences, sched: Schedule) -> np.ndarray:
    """A copy of the fit table with float32(A'_k) in the `matrix` field of the row that selection picked for pair k.
    Confidence, residual and point counts stay the estimator's; a pair without an estimate, one of confidence 0 and the pair
    across a cut stay untouched."""
    table = fit_records.copy()
    conf = np.asarray(confidences, dtype=np.float64)
    for k in range(table.shape[0]):
        if conf[k] == 0.0 or sched.shot_start[k + 1]:
            continue
        table["matrix"][k, _MODE_INDEX[modes[k]]] = np.asarray(A[k], dtype=np.float32).reshape(9)
    return table


def rescale_to_full(C, size, working_size) -> np.ndarray:
    """S^-1 C S in float64: `host_math.rescale_transforms_to_full` without its float32 cast."""
    C = np.asarray(C, dtype=np.float64)
    if working_size is None:
        return C.copy()
    sx, sy = working_size[0] / float(size[0]), working_size[1] / float(size[1])
    up, down = np.array([1.0 / sx, 1.0 / sy, 1.0]), np.array([sx, sy, 1.0])
    return (up[None, :, None] * C) * down[None, None, :]


def path_params(C_full, mode: str) -> np.ndarray:
    """The parameter vector whose negation is the inverse's: params_to_matrix(-path_params(C)) = C^-1.  Translation:
    (tx, ty).  Similarity: (t'x, t'y, theta, log s) with t' = s^-1 R(-theta) t.  (The reference's path is the sum of the
    pairs' own parameters, rotation about the pixel origin: that sum is not the parameter vector of the composed matrix.)"""
    C = np.asarray(C_full, dtype=np.float64).reshape(-1, 3, 3)
    if mode == "translation":
        return np.stack([C[:, 0, 2], C[:, 1, 2]], axis=1)
    if mode != "similarity":
        raise ValueError(f"path_params: mode {mode!r} is not one of {MODES}")
    a, c = C[:, 0, 0], C[:, 1, 0]
    s = np.sqrt(a * a + c * c)
    theta = np.arctan2(c, a)
    ct, st = np.cos(theta), np.sin(theta)
    tx, ty = C[:, 0, 2], C[:, 1, 2]
    return np.stack([(ct * tx + st * ty) / s, (-st * tx + ct * ty) / s, theta, np.log(s)], axis=1)


def path_deltas(C_full, mode: str) -> np.ndarray:
    """d_k = path_params(C_{k+1}) - path_params(C_k), f64 [N-1,P]: what `_plan_stabilization(path_deltas=...)` takes."""
    p = path_params(C_full, mode)
    return p[1:] - p[:-1]


# ---------------------------------------------------------------------------------------------------------- the whole step
def correct(sums_fn, fit_records: np.ndarray, selection, segments, total_frames: int, mode: str, size, working_size, spacing: int,
            exposure: bool = False, masked: bool = False):
    """Everything between the estimator's fit table and the plan: schedule, refinement, poses.
    selection: (work_mats, modes, confidences, ...) as select_transitions returns them.
    sums_fn: the plain rule's, sums_fn(anchor, R) -> int64 [N,17]; with exposure or masked the second form's,
    sums_fn(anchor, R, gain, offset, cap) -> int64 [N,31].
    -> (the fit table with the corrected transitions, path_deltas f64 [N-1,P], meta["drift_correction"])."""
    work_mats, modes, confidences = selection[0], selection[1], selection[2]
    work = working_size if working_size is not None else size
    sched = schedule(total_frames, segments, confidences, spacing)
    extended = exposure or masked
    result = refine_ex(sums_fn, work_mats, sched, mode, work, exposure) if extended else refine(sums_fn, work_mats, sched, mode, work)
    C = poses(result.R, sched)
    table = write_transitions(fit_records, transitions(C), modes, confidences, sched)
    C_full = rescale_to_full(C, size, working_size)
    deltas = path_deltas(C_full, mode)
    for k in range(deltas.shape[0]):                  # every shot's path starts at 0: no delta across a cut
        if sched.shot_start[k + 1]:
            deltas[k] = 0.0
    chained_full = rescale_to_full(poses(result.R_chained, sched), size, working_size)
    block = meta_block(sched, result, C_full, chained_full, size)
    if extended:
        block.update(meta_block_ex(sched, result, exposure, masked))
    return table, deltas, block


def meta_block(sched: Schedule, result: Refinement, C_full, chained_full, size) -> Dict[str, Any]:
    refined = [i for i, r in enumerate(result.reason) if r is None]
    c = _corners(size)                                          # the corner PIXELS (0, 0) .. (w-1, h-1), as corner_distance
    diff = C_full[:, :2] @ c - chained_full[:, :2] @ c          # [N,2,4]: the four corners, full-resolution px
    moved = np.max(np.hypot(diff[:, 0], diff[:, 1]), axis=-1)
    anchored = sched.anchor >= 0

    def mean_residual(sums, rows):
        count = int(sums[rows, 0].sum())
        return float(int(sums[rows, 2].sum()) / (1024.0 * count)) if count else 0.0

    seen = result.sums_first[anchored, 0] + result.sums_first[anchored, 1]
    capped = result.sums_first[anchored, 1][seen > 0] / seen[seen > 0]
    return {
        "version": 1,
        "spacing": sched.spacing,
        "iterations": result.iterations,
        "residual_cap": RESIDUAL_CAP,
        "path_model": "anchored",
        "keyframes": [int(k) for k in sched.keyframes],
        "frames_refined": len(refined),
        "frames_kept": {name: sum(1 for r in result.reason if r == name) for name in KEEP_REASONS},
        "correction_px_mean": float(np.mean(moved)) if moved.size else 0.0,
        "correction_px_max": float(np.max(moved)) if moved.size else 0.0,
        "residual_before": mean_residual(result.sums_first, refined),
        "residual_after": mean_residual(result.sums_final, refined),
        "capped_fraction_mean": float(np.mean(capped)) if capped.size else 0.0,
    }


def meta_block_ex(sched: Schedule, result: Refinement, exposure: bool, masked: bool) -> Dict[str, Any]:
    """What the block gains (and, for frames_kept, replaces) under drift_exposure / drift_mask.  residual_before and
    capped_fraction_mean then describe launch `residual_before_launch`, the one the cost test starts from."""
    out: Dict[str, Any] = {"frames_kept": {name: sum(1 for r in result.reason if r == name) for name in KEEP_REASONS_EX}}
    if exposure:
        gain = result.gain.astype(np.float64) / GAIN_UNIT
        out["exposure"] = {"matched": True, "gain": [float(g) for g in gain],
                           "offset": [float(o) for o in result.offset.astype(np.float64) / GAIN_UNIT],
                           "gain_min": float(gain.min()), "gain_max": float(gain.max()),
                           "residual_before_launch": int(result.before_launch)}
    if masked:
        anchored = sched.anchor >= 0
        seen = result.sums_first[anchored, 0] + result.sums_first[anchored, 1] + result.masked_first[anchored]
        hidden = result.masked_first[anchored][seen > 0] / seen[seen > 0]
        out["masked_fraction_mean"] = float(np.mean(hidden)) if hidden.size else 0.0
    return out
