#!/usr/bin/env python3
"""Estimation mask: accuracy on a clip whose larger part is a moving subject, and the cost of the feature.

  accuracy   tests/test_estimation_mask_gpu.py::subject_clip (bench.synth_clip background under tests.util.shake_path, a
             second layer with its own motion inside a rectangle of 60 % of the frame): error of the reported
             displacement at the frame centre against the background's true transition (bench.transition_accuracy, px at
             working resolution), per pair, without a mask and with the exact rectangle masks at margins 0 / 8 / 16 / 32.
             One JSON object per case; the numbers back MASKED_BOUNDS of the test and profiles/r08_estimation_mask.md.
  --cost     C2 clip (256 x 1080p) with full-frame masks holding a 60 % rectangle: kernel times (vstab_set_timing) of
             "mask" and the masked "fit" next to the same clip's "gray" and unmasked "fit", several launches each.

    python tools/estimation_mask_accuracy.py [--frames 48] [--cost] [--no-accuracy]
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
from tests.test_estimation_mask_gpu import ARGS, centre_errors, subject_clip  # noqa: E402

MARGINS = (0, 8, 16, 32)


def spread(v):
    v = np.asarray(v, np.float64)
    return {"min": round(float(v.min()), 5), "mean": round(float(v.mean()), 5), "max": round(float(v.max()), 5)}


def accuracy(fp, hm, ctx, dev, n):
    cases = [((960, 540), m, "flow", n) for m in ("translation", "similarity", "perspective")]
    cases += [((1920, 1080), m, "flow", n) for m in ("translation", "similarity", "perspective")]
    cases += [((480, 270), "similarity", "flow_tvl1", n)]
    for (w, h), mode, estimator, frames_n in cases:
        frames, masks, cam = subject_clip(frames_n, w, h, mode, dev)
        work = hm._working_estimation_size(w, h)

        def run(**kw):
            res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", mode, *ARGS, ctx=ctx, keep_on_device=True,
                                       estimator=estimator, **kw)
            return centre_errors(res.meta, cam, (w, h), work), res.meta

        plain, _ = run()
        row = {"case": f"{w}x{h} {mode} {estimator}", "pairs": frames_n - 1, "unmasked_px": spread(plain)}
        for margin in MARGINS:
            err, meta = run(estimation_mask=masks, mask_margin=margin)
            row[f"margin_{margin}_px"] = spread(err)
            row[f"margin_{margin}_blocked_mean"] = round(meta["estimation_mask"]["blocked_fraction_mean"], 4)
            row[f"margin_{margin}_modes"] = sorted({t["mode"] for t in meta["estimated_motion"]["per_transition"]})
        print(json.dumps(row), flush=True)
        del frames, masks


def cost(fp, hm, ctx, dev, torch, n=256, reps=5):
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, dev)
    masks = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    side = np.sqrt(0.6)
    rw, rh = int(round(w * side)), int(round(h * side))
    for i in range(n):
        x0, y0 = (w - rw) // 2 + (i % 16) - 8, (h - rh) // 2 + (i % 8) - 4
        masks[i, y0:y0 + rh, x0:x0 + rw] = 1.0
    work = hm._working_estimation_size(w, h)
    gray = ctx.gray_downscale(frames, work)
    _, grid = ctx.dis_flow_batch(gray, sample_step=8, want_full=False, want_grid=True)
    ctx.set_timing(True)
    out = {"frames": n, "size": [w, h], "launches": reps, "ms": {}}
    kinds = {"gray": [], "mask": [], "mask_broadcast": [], "fit": [], "fit_masked": []}
    blocked = None
    for _ in range(reps + 1):   # the first of each is the warm-up
        ctx.gray_downscale(frames, work)
        torch.cuda.synchronize()
        kinds["gray"].append(ctx.last_kernel_ms("gray"))
        blocked = ctx.mask_block_grid(masks, n, work, 8, 16)
        torch.cuda.synchronize()
        kinds["mask"].append(ctx.last_kernel_ms("mask"))
        ctx.mask_block_grid(masks[:1], n, work, 8, 16)
        torch.cuda.synchronize()
        kinds["mask_broadcast"].append(ctx.last_kernel_ms("mask"))
        ctx.sample_fit_batch(grid, 8, "similarity")
        kinds["fit"].append(ctx.last_kernel_ms("fit"))
        ctx.sample_fit_batch(grid, 8, "similarity", blocked=blocked)
        kinds["fit_masked"].append(ctx.last_kernel_ms("fit"))
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
    gray_bytes, mask_bytes = n * h * w * 12 + n * work[0] * work[1], n * h * w * 4
    out["gray_TBps"] = round(gray_bytes / (out["ms"]["gray"]["median"] * 1e-3) / 1e12, 3)
    out["mask_TBps"] = round(mask_bytes / (out["ms"]["mask"]["median"] * 1e-3) / 1e12, 3)
    out["blocked_fraction"] = round(float(blocked.float().mean()), 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    args = ap.parse_args()
    import torch

    graft.load_package()
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import native

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    if not args.no_accuracy:
        accuracy(fp, hm, ctx, dev, args.frames)
    if args.cost:
        cost(fp, hm, ctx, dev, torch)


if __name__ == "__main__":
    main()
