#!/usr/bin/env python3
"""Mesh warp round trip: what restoring with the recorded mesh gains, and what the inverse kernel costs.

  accuracy   The non-rigid clips of tests/mesh_restatement.nonrigid_clip (24 frames, camera_lock, strength 1) at 480x270 and
             960x540, stabilized with mesh_warp=True and mesh_motion=True, then restored from the stabilized frames.  PSNR of
             restored against original frames over the pixels at least ceil(max_shift) + 2 inside every restore's mask, for
               mesh     the mesh run restored with apply_motion(mesh=True)              (the per-pixel inverse)
               today    the same run restored with mesh=False                           (the global matrices only)
               ceiling  a plain run (mesh_warp=None) restored plainly                   (two bilinear interpolations)
             One JSON object per clip.
  --cost     256 x 1080p: the "mesh_unwarp" kernel next to "mesh_warp" and the plain "warp" in the same run (a smooth field of
             amplitude w/64 on 17 x 10 vertices, and all-zero offsets); median of 5 launches after one warm-up.

    python tools/mesh_round_trip_accuracy.py [--cost] [--no-accuracy]

They back profiles/r12_mesh_round_trip.md.
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
from tests import test_mesh_round_trip_cpu as C  # noqa: E402
from tests import test_mesh_round_trip_gpu as T  # noqa: E402


def accuracy(ctx, torch, dev):
    n = T.CLIP_FRAMES
    for (w, h), seed in (((480, 270), 5), ((480, 270), 11), ((960, 540), 5), ((960, 540), 11)):
        frames, _, _ = R.nonrigid_clip(n, h, w, dev, seed=seed)
        run = T._stabilize(ctx, frames, "crop_and_pad", mesh_warp=True, mesh_motion=True)
        none = T._stabilize(ctx, frames, "crop_and_pad")
        back = {k: v for k, v in json.loads(json.dumps(run.meta)).items() if k != "motion_meta"}
        none_back = {k: v for k, v in none.meta.items() if k != "motion_meta"}
        mesh = T._apply(ctx, run.frames, back, mesh=True)
        today = T._apply(ctx, run.frames, back)
        ceiling = T._apply(ctx, none.frames, none_back)
        radius = int(math.ceil(run.meta["mesh_warp"]["max_shift"])) + 2
        masks = torch.maximum(torch.maximum(mesh.masks[..., 0], today.masks[..., 0]), ceiling.masks[..., 0])
        sel = T._interior(masks, radius)
        p = [T._psnr(x.frames, frames, sel) for x in (mesh, today, ceiling)]
        print(json.dumps({"clip": f"nonrigid {w}x{h} seed {seed}", "psnr_mesh": round(p[0], 2), "psnr_today": round(p[1], 2),
                          "psnr_ceiling": round(p[2], 2), "gain_db": round(p[0] - p[1], 2),
                          "unconverged_max": mesh.meta["motion_apply"]["mesh"]["unconverged_max"],
                          "interior": round(float(sel.float().mean()), 3),
                          "correction_px_max": round(run.meta["mesh_warp"]["correction_px_max"], 3)}), flush=True)


def cost(ctx, torch, dev, n=256, reps=5):
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, dev)
    final = np.tile(np.array([[1, 0, 3.25], [0, 1, -2.5], [0, 0, 1]], np.float32), (n, 1, 1))
    fields = {"zero": torch.zeros((n, 10, 17, 2), device=dev),
              "smooth": torch.from_numpy(np.stack([C.smooth_field(w, h, 17, 10, w / 64.0, phase=0.05 * i) for i in range(n)])).to(dev)}
    ctx.set_timing(True)
    kinds = {"warp": []}
    unconverged = {}
    for rep in range(reps + 1):   # the first of each is the warm-up
        ctx.warp_batch(frames, final, (w, h), want_mask=True, want_count=True)
        kinds["warp"].append(ctx.last_kernel_ms("warp"))
        for name, off in fields.items():
            ctx.mesh_warp_batch(frames, final, (w, h), off, want_mask=True, want_count=True)
            kinds.setdefault(f"mesh_warp {name}", []).append(ctx.last_kernel_ms("mesh_warp"))
            unc = ctx.mesh_unwarp_batch(frames, final, (w, h), off, want_mask=True, want_count=True, want_unconverged=True)[3]
            kinds.setdefault(f"mesh_unwarp {name}", []).append(ctx.last_kernel_ms("mesh_unwarp"))
            unconverged[name] = int(unc.max().item())
    ctx.set_timing(False)
    out = {"frames": n, "size": [w, h], "vertices": [17, 10], "launches": reps, "unconverged_max": unconverged, "ms": {}}
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
    base = out["ms"]["warp"]["median"]
    out["over_warp"] = {k: round(v["median"] / base, 3) for k, v in out["ms"].items() if k != "warp"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    args = ap.parse_args()
    import torch

    graft.load_package()
    from vstab_amd import native

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    if not args.no_accuracy:
        accuracy(ctx, torch, dev)
    if args.cost:
        cost(ctx, torch, dev)


if __name__ == "__main__":
    main()
