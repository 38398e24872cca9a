"""Scene cuts: find the hard cuts of a clip and split it into shots that are stabilized one by one.

The detector is the motion-compensated residual of every consecutive pair of estimation images: the mean absolute
difference of frame i and frame i+1 AFTER the pair's own fitted transition (include/vstab.h states the rule; the kernel
behind `native.Context.pair_residual_batch` is csrc/vstab_cut.hip).  Inside a shot the transition explains the pair and
the residual is interpolation noise; across a cut nothing explains it.  Uncompensated differences cannot tell violent
shake from a cut, and histograms miss cuts between similar scenes (profiles/r09_scene_cuts.md has the numbers).

This module is the host side: the decision, the segmentation and the checks of a request.  Nothing here needs a GPU.
Out of scope: fades, dissolves and flashes (a dissolve is many small residuals, not one large one) and per-shot framing.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

OVERLAP_MIN = 0.25   # below a quarter of common area there is no camera move to smooth across: a cut by definition

# sqrt(a * b) rounded to one decimal, a = the largest within-shot score and b = the smallest across-cut score of the
# calibration set (tools/scene_cuts_accuracy.py prints both; profiles/r09_scene_cuts.md).  The value below is from the NumPy
# form of that experiment with the clips' TRUE transitions (a = 4.1, b = 29.8 at 480x270); the tool repeats it with FITTED
# transitions on the GPU and reports the default that follows next to this one.  Calibrated on synthetic clips only --
# procedural texture under random-walk shake, no footage -- which is why it is a parameter of every entry point and not a
# constant of the rule.
DEFAULT_CUT_THRESHOLD = 11.1

_MODE_INDEX = {"translation": 0, "similarity": 1, "perspective": 2}


@dataclass
class Request:
    """A checked scene_cuts request: mode "auto" (detect) or "given" (an edit list of first frames of shots)."""

    mode: str
    threshold: Optional[float]      # auto only
    cuts: Optional[List[int]]       # given only, until detection fills it in


def check_request(scene_cuts, cut_threshold=None) -> Optional[Request]:
    """The checks that need neither the clip nor a GPU.  None -> None (the feature is off); "auto" -> detection with
    cut_threshold (None: DEFAULT_CUT_THRESHOLD); a sequence of frame indices -> those frames start a shot."""
    if scene_cuts is None:
        return None
    if isinstance(scene_cuts, str):
        if scene_cuts != "auto":
            raise ValueError(f"scene_cuts={scene_cuts!r}: expected None, 'auto' or a sequence of frame indices")
        threshold = DEFAULT_CUT_THRESHOLD if cut_threshold is None else cut_threshold
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not np.isfinite(threshold) or threshold <= 0.0:
            raise ValueError(f"cut_threshold={cut_threshold!r}: expected a finite number above 0 (mean absolute difference, 0..255) or None")
        return Request("auto", float(threshold), None)
    try:
        items = list(scene_cuts)
    except TypeError:
        raise ValueError(f"scene_cuts={scene_cuts!r}: expected None, 'auto' or a sequence of frame indices") from None
    cuts = []
    for v in items:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"scene_cuts entry {v!r} is not an integer frame index")
        if cuts and int(v) <= cuts[-1]:
            raise ValueError(f"scene_cuts entry {int(v)} does not increase (after {cuts[-1]}): the list must be strictly increasing")
        cuts.append(int(v))
    return Request("given", None, cuts)


def check_given_cuts(cuts: Sequence[int], total_frames: int) -> None:
    """A shot starts at a frame in 1 .. N-1."""
    for v in cuts:
        if not 1 <= v <= total_frames - 1:
            raise ValueError(f"scene_cuts entry {v} outside [1, {total_frames - 1}] for a clip of {total_frames} frames")


def scoring_transitions(fit_records: np.ndarray, requested_mode: str) -> np.ndarray:
    """The transition each pair is scored with, from that pair's records alone (no stickiness: detection must not depend on
    the segmentation it produces): the usable (computed and accepted) candidate of the highest mode at or below the
    requested one, the identity where there is none.  [P,3] records -> float32 [P,3,3] at working resolution."""
    pairs = fit_records.shape[0]
    usable = (fit_records["computed"] != 0) & (fit_records["accepted"] != 0)
    mats = np.tile(np.eye(3, dtype=np.float32), (pairs, 1, 1))
    taken = np.zeros(pairs, bool)
    for m in range(_MODE_INDEX[requested_mode], -1, -1):
        pick = usable[:, m] & ~taken
        mats[pick] = fit_records["matrix"][pick, m].reshape(-1, 3, 3)
        taken |= pick
    return mats


def scores_and_overlap(sum_abs, inside, height: int, width: int) -> Tuple[np.ndarray, np.ndarray]:
    """score = sum_abs / inside (float64, 0..255), overlap = inside / (h*w).  A pair with inside == 0 has nothing to
    average: its score is reported as 255.0 (it is a cut by its overlap) and nothing is divided."""
    s = np.asarray(sum_abs, dtype=np.int64)
    n = np.asarray(inside, dtype=np.int64)
    scores = np.full(s.shape, 255.0, np.float64)
    some = n > 0
    scores[some] = s[some].astype(np.float64) / n[some].astype(np.float64)
    return scores, n.astype(np.float64) / float(int(height) * int(width))


def is_cut(scores, overlap, threshold: float) -> np.ndarray:
    """Pair i is a cut iff overlap_i < OVERLAP_MIN or score_i >= threshold."""
    return (np.asarray(overlap, np.float64) < OVERLAP_MIN) | (np.asarray(scores, np.float64) >= float(threshold))


def cuts_from_pairs(cut_pairs) -> List[int]:
    """A cut at pair i (frames i, i+1) makes frame i+1 the first of a shot."""
    return [int(i) + 1 for i in np.nonzero(np.asarray(cut_pairs, bool))[0]]


def segments_from_cuts(cuts: Sequence[int], total_frames: int) -> List[Tuple[int, int]]:
    """First frames of shots -> [s_k, e_k) over the clip's frames, in order.  A one-frame segment is legal."""
    edges = [0] + [int(c) for c in cuts] + [int(total_frames)]
    return [(edges[k], edges[k + 1]) for k in range(len(edges) - 1)]


def meta_block(request: Request, cuts: Sequence[int], scores=None, overlap=None) -> Dict[str, Any]:
    return {"mode": request.mode, "threshold": request.threshold, "cuts": [int(c) for c in cuts], "segments": len(cuts) + 1,
            "scores": None if scores is None else [float(v) for v in scores],
            "overlap": None if overlap is None else [float(v) for v in overlap]}
