#!/usr/bin/env python3
"""Scene cuts: the calibration of the default threshold, and the cost of the residual kernel.

  calibration  The shots of tests/test_scene_cuts_gpu.py (bench.synth_clip, another texture seed per shot, under
               tests.util.shake_path, another path seed per shot; 12 frames each).  For every case the first shot is joined
               with each of the three others; the scores (mean absolute difference after the pair's FITTED transition) of
               the pairs inside the shots and of the pair across the cut are collected:
                 DIS       translation / similarity / perspective  x  amp 1 / 3  x  480x270 / 960x540
                 TV-L1     similarity, amp 1 / 3, 480x270
                 classic   similarity, amp 1 / 3, 480x270
                 bench     64 frames of the benchmark's own clip (1080p, working size 960x540): within-shot only
               a = the largest within-shot score, b = the smallest across-cut score, default = sqrt(a * b) rounded to one
               decimal (scene_cuts.DEFAULT_CUT_THRESHOLD); b / a < 3 is reported as "do not ship a default".
               One JSON object per case and one summary; they back profiles/r09_scene_cuts.md.
  --cost       C2 clip (256 x 1080p -> 255 pairs of 960x540): the "cut" kernel's time (vstab_set_timing), median of 5
               launches after one warm-up, next to the "gray" time of the same clip in the same run, bytes and rate.

    python tools/scene_cuts_accuracy.py [--cost] [--no-calibration]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import __graft_entry__ as graft  # noqa: E402
from tests.test_scene_cuts_gpu import joined  # noqa: E402


def pair_scores(fp, hm, sc, ctx, frames, mode, estimator):
    """The detector's numbers for a clip, through the pipeline's own pieces: estimator -> each pair's own best candidate ->
    residual kernel -> (scores, overlap)."""
    h, w = int(frames.shape[1]), int(frames.shape[2])
    gray_out = []
    records = fp._ESTIMATORS[estimator](ctx, frames, hm._working_estimation_size(w, h), mode, gray_out=gray_out)
    gray = gray_out[0]
    sum_abs, inside = ctx.pair_residual_batch(gray, sc.scoring_transitions(records, mode))
    return sc.scores_and_overlap(sum_abs, inside, int(gray.shape[1]), int(gray.shape[2]))


def calibration(fp, hm, sc, ctx, dev):
    cases = [((w, h), mode, amp, "flow") for (w, h) in ((480, 270), (960, 540)) for mode in ("translation", "similarity", "perspective")
             for amp in (1.0, 3.0)]
    cases += [((480, 270), "similarity", amp, est) for est in ("flow_tvl1", "classic") for amp in (1.0, 3.0)]
    within, across = [], []
    for (w, h), mode, amp, estimator in cases:
        row = {"case": f"{w}x{h} {mode} amp {amp} {estimator}", "within_max": 0.0, "across": [], "overlap_min": 1.0}
        for k in (1, 2, 3):
            frames, _, cuts = joined((0, k), w, h, mode, amp, dev)
            scores, overlap = pair_scores(fp, hm, sc, ctx, frames, mode, estimator)
            c = cuts[0] - 1
            row["across"].append(round(float(scores[c]), 3))
            row["within_max"] = round(max(row["within_max"], float(np.delete(scores, c).max())), 3)
            row["overlap_min"] = round(min(row["overlap_min"], float(np.delete(overlap, c).min())), 3)
            del frames
        within.append(row["within_max"])
        across.append(min(row["across"]))
        print(json.dumps(row), flush=True)
    frames = bench.synth_clip(64, 0, 1080, 1920, dev)
    scores, overlap = pair_scores(fp, hm, sc, ctx, frames, "similarity", "flow")
    row = {"case": "bench clip, 64 frames 1920x1080 similarity flow", "within_max": round(float(scores.max()), 3),
           "overlap_min": round(float(overlap.min()), 3)}
    within.append(row["within_max"])
    print(json.dumps(row), flush=True)
    a, b = max(within), min(across)
    out = {"within_max_a": a, "across_min_b": b, "ratio_b_over_a": round(b / a, 2), "default_sqrt_ab": round(float(np.sqrt(a * b)), 1),
           "shipped_default": sc.DEFAULT_CUT_THRESHOLD}
    if b / a < 3:
        out["verdict"] = "b / a < 3: the score does not separate on this set; do not ship a default"
    print(json.dumps(out), flush=True)


def cost(fp, hm, sc, ctx, dev, torch, n=256, reps=5):
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, dev)
    work = hm._working_estimation_size(w, h)
    gray_out = []
    records = fp.estimate_transitions(ctx, frames, work, "similarity", gray_out=gray_out)
    gray, mats = gray_out[0], sc.scoring_transitions(records, "similarity")
    ctx.set_timing(True)
    kinds = {"gray": [], "cut": []}
    for _ in range(reps + 1):   # the first of each is the warm-up
        ctx.gray_downscale(frames, work)
        torch.cuda.synchronize()
        kinds["gray"].append(ctx.last_kernel_ms("gray"))
        sum_abs, inside = ctx.pair_residual_batch(gray, mats)
        kinds["cut"].append(ctx.last_kernel_ms("cut"))
    ctx.set_timing(False)
    out = {"frames": n, "pairs": n - 1, "working_size": list(work), "launches": reps, "ms": {}}
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
    gray_bytes = n * h * w * 12 + n * work[0] * work[1]
    cut_bytes = (n - 1) * 2 * work[0] * work[1]
    out["gray_bytes"], out["cut_bytes"] = gray_bytes, cut_bytes
    out["gray_TBps"] = round(gray_bytes / (out["ms"]["gray"]["median"] * 1e-3) / 1e12, 3)
    out["cut_TBps"] = round(cut_bytes / (out["ms"]["cut"]["median"] * 1e-3) / 1e12, 3)
    scores, overlap = sc.scores_and_overlap(sum_abs, inside, work[1], work[0])
    out["score_max"], out["overlap_min"] = round(float(scores.max()), 3), round(float(overlap.min()), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    import torch

    graft.load_package()
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import native
    from vstab_amd import scene_cuts as sc

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    if not args.no_calibration:
        calibration(fp, hm, sc, ctx, dev)
    if args.cost:
        cost(fp, hm, sc, ctx, dev, torch)


if __name__ == "__main__":
    main()
