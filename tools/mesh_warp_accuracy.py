#!/usr/bin/env python3
"""Mesh warp: what it recovers on non-rigid clips, what it leaves alone on rigid ones, and what its kernels cost.

  accuracy   The clips of tests/test_mesh_warp_gpu.py: the bench's texture sampled analytically at p - D_i(p),
             D_i(p) = g_i + a(p) e_i (tests/mesh_restatement.nonrigid_clip), 24 frames, camera_lock, strength 1 -- the ideal
             output is the static texture.  PSNR against it over the pixels at least max_shift inside the masks, for
             mesh_warp=None, mesh_warp=True and the mesh warp fed the analytic offsets (the ceiling of the representation),
             and the share of the None-to-ceiling gap that is recovered, in dB.  Then tests.util.shake_path clips
             (similarity, amp 1 / 3): PSNR with and without, correction_px_max.  One JSON object per clip.
  --cost     C2 clip (256 x 1080p): the "mesh_warp" kernel (zero offsets, 17 x 10 vertices) next to the "warp" kind in the
             same run, and "mesh_residual" on the clip's own grid; median of 5 launches after one warm-up (vstab_set_timing).

    python tools/mesh_warp_accuracy.py [--cost] [--no-accuracy]

They back profiles/r10_mesh_warp.md.
"""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import __graft_entry__ as graft  # noqa: E402
from tests import mesh_restatement as R  # noqa: E402
from tests import test_mesh_warp_gpu as T  # noqa: E402
from tests.util import shake_path  # noqa: E402


def accuracy(ctx, torch, dev):
    n = T.CLIP_FRAMES
    for (w, h), seed in (((480, 270), 5), ((480, 270), 11), ((960, 540), 5), ((960, 540), 11)):
        frames, g, e = R.nonrigid_clip(n, h, w, dev, seed=seed)
        none = T._stabilize(ctx, frames, args=T.LOCK_ARGS)
        mesh = T._stabilize(ctx, frames, args=T.LOCK_ARGS, mesh_warp=True)
        final = T._final_matrices(none.meta)
        shift = mesh.meta["mesh_warp"]["max_shift"]
        offsets = np.clip(T._analytic_offsets(final, g, e, w, h, 17, 10), -shift, shift)
        top, top_mask, _ = ctx.mesh_warp_batch(frames, final, (w, h), offsets, want_mask=True)
        ideal = T._static_ideal(final[0], n, h, w, dev)
        sel = T._interior(torch.maximum(torch.maximum(none.masks[..., 0], mesh.masks[..., 0]), top_mask), int(math.ceil(shift)))
        p = [T._psnr(x, ideal, sel) for x in (none.frames, mesh.frames, top)]
        print(json.dumps({"clip": f"nonrigid {w}x{h} seed {seed}", "psnr_none": round(p[0], 2), "psnr_mesh": round(p[1], 2),
                          "psnr_ceiling": round(p[2], 2), "gain_db": round(p[1] - p[0], 2), "gap_db": round(p[2] - p[0], 2),
                          "recovered": round((p[1] - p[0]) / (p[2] - p[0]), 3), "differential_px_max": round(float(np.abs(e).max()), 2),
                          "meta": mesh.meta["mesh_warp"]}), flush=True)
    for amp in (1.0, 3.0):
        w, h = 480, 270
        frames = bench.synth_clip(n, 0, h, w, dev, seed=1234, mats=shake_path(n, w, h, "similarity", seed=3, amp=amp))
        none = T._stabilize(ctx, frames, args=T.LOCK_ARGS)
        mesh = T._stabilize(ctx, frames, args=T.LOCK_ARGS, mesh_warp=True)
        ideal = T._static_ideal(T._final_matrices(none.meta)[0], n, h, w, dev)
        sel = T._interior(torch.maximum(none.masks[..., 0], mesh.masks[..., 0]), int(math.ceil(mesh.meta["mesh_warp"]["max_shift"])))
        print(json.dumps({"clip": f"rigid similarity amp {amp} {w}x{h}", "psnr_none": round(T._psnr(none.frames, ideal, sel), 2),
                          "psnr_mesh": round(T._psnr(mesh.frames, ideal, sel), 2), "meta": mesh.meta["mesh_warp"]}), flush=True)


def cost(ctx, torch, dev, fp, hm, n=256, reps=5):
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, dev)
    work = hm._working_estimation_size(w, h)
    grid_out = []
    records = fp.estimate_transitions(ctx, frames, work, "similarity", grid_out=grid_out)
    mats = fp.select_transitions(records, "similarity")[0]
    final = np.tile(np.array([[1, 0, 3.25], [0, 1, -2.5], [0, 0, 1]], np.float32), (n, 1, 1))
    zero = torch.zeros((n, 10, 17, 2), device=dev)
    ctx.set_timing(True)
    kinds = {"warp": [], "mesh_warp": [], "mesh_residual": []}
    for _ in range(reps + 1):   # the first of each is the warm-up
        ctx.warp_batch(frames, final, (w, h), want_mask=True, want_count=True)
        kinds["warp"].append(ctx.last_kernel_ms("warp"))
        ctx.mesh_warp_batch(frames, final, (w, h), zero, want_mask=True, want_count=True)
        kinds["mesh_warp"].append(ctx.last_kernel_ms("mesh_warp"))
        ctx.mesh_residual_batch(grid_out[0], fp.SAMPLE_STEP, work, mats, 17, 10)
        kinds["mesh_residual"].append(ctx.last_kernel_ms("mesh_residual"))
    ctx.set_timing(False)
    out = {"frames": n, "size": [w, h], "working_size": list(work), "vertices": [17, 10], "launches": reps, "ms": {}}
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
    out["mesh_warp_over_warp"] = round(out["ms"]["mesh_warp"]["median"] / out["ms"]["warp"]["median"], 3)
    out["warp_TBps"] = round(n * w * h * 28 / (out["ms"]["warp"]["median"] * 1e-3) / 1e12, 3)
    out["mesh_warp_TBps"] = round(n * w * h * 28 / (out["ms"]["mesh_warp"]["median"] * 1e-3) / 1e12, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
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
        accuracy(ctx, torch, dev)
    if args.cost:
        cost(ctx, torch, dev, fp, hm)


if __name__ == "__main__":
    main()
