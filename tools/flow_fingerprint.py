#!/usr/bin/env python3
"""Fingerprint of the Flow step's driver: what five configurations return and which kernels they launch.

For a change of the Python that drives the kernels (flow_pipeline._stabilize_frames and what it calls) which must leave
behaviour alone: run this before and after, the lines must be identical.  The clip is the small one of
tests/test_device_plan_gpu.py (12 frames of 160 x 96, frame 5 blurred); the configurations are

  plain        crop_and_pad on the device plan
  expand       expand on the device plan
  scene_mesh   scene_cuts="auto" + mesh_warp + mesh_motion + dynamic_zoom (host plan)
  rolling      rolling_shutter="auto" (host plan)
  full_tail    estimation mask, sharpness transfer, blended temporal fill, spatial fill, stability report, mask hand-off

One JSON line per configuration: sha256 of the frames' and the masks' bytes, sha256 of the meta as canonical JSON (sorted
keys) and the order of its top-level keys, the device-plan verdict, and the launches per timed kind (kernel_ms_stats under
set_timing(True)).  --out FILE also writes the lines with the canonical meta itself, for a diff.

    python tools/flow_fingerprint.py [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/flow_fingerprint.py --marks
    python tools/flow_fingerprint.py --split-trace DIR/.../*_kernel_trace.csv

--marks launches one torch cumsum in front of every configuration (a scan kernel, which nothing else here launches), and --split-trace
cuts a kernel trace at those marks: the ordered kernel names per configuration and hardware queue, their count and sha256.  No
GPU needed for that.
"""
import argparse
import csv
import hashlib
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CONFIGS = ("plain", "expand", "scene_mesh", "rolling", "full_tail")
KINDS = ("range", "gray", "dis", "mask", "fit", "cut", "mesh_residual", "cover_extent", "row_residual", "warp", "rolling_warp",
         "sharpness", "sharp_transfer", "fill", "fill_gain", "fill_blend", "sfill", "stability", "mask_hold", "mask_grow")
MARK = "scan"       # what the mark's kernel is recognised by in a trace: torch's cumsum is a scan kernel, and nothing else here is


def sha(tensor) -> str:
    return hashlib.sha256(tensor.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def launches(ctx) -> dict:
    from vstab_amd import native

    out = {}
    for kind in KINDS:
        try:
            n = ctx.kernel_ms_stats(kind)[1]
        except native.VstabError:       # a kind this process has not timed yet
            n = 0
        if n:
            out[kind] = n
    return out


def run(marks: bool):
    import torch

    import __graft_entry__ as graft

    graft.load_package()
    from tests import test_device_plan_gpu as T
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import native

    ctx = native.default_context()
    frames = T.full_tail_clip(ctx.device)
    requests = {
        "plain": ("crop_and_pad", {}),
        "expand": ("expand", {}),
        "scene_mesh": ("crop_and_pad", dict(scene_cuts="auto", mesh_warp=True, mesh_motion=True, dynamic_zoom=True)),
        "rolling": ("crop_and_pad", dict(rolling_shutter="auto")),
        "full_tail": ("crop_and_pad", T.full_tail_requests(ctx.device)),
    }
    rows = []
    for name in CONFIGS:
        framing, extras = requests[name]
        if marks:
            torch.ones(64, device=ctx.device).cumsum(0)
        ctx.set_timing(True)            # also resets the counts
        res = fp._stabilize_frames(hm._normalize_video_input(frames), framing, "similarity", *T.TAIL_ARGS, ctx=ctx, keep_on_device=True,
                                   **extras)
        torch.cuda.synchronize()
        counts = launches(ctx)
        ctx.set_timing(False)
        meta = json.dumps(res.meta, sort_keys=True, default=float)
        rows.append({"config": name, "frames_sha256": sha(res.frames), "masks_sha256": sha(res.masks),
                     "meta_sha256": hashlib.sha256(meta.encode()).hexdigest(), "meta_keys": list(res.meta),
                     "device_plan": res.device_plan, "launches": counts, "meta": meta})
    return rows


def split_trace(path: str):
    with open(path, newline="") as fh:
        recs = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(recs) if MARK in r["Kernel_Name"].lower()]
    if len(cuts) != len(CONFIGS):
        raise SystemExit(f"{path}: {len(cuts)} marks for {len(CONFIGS)} configurations (was the trace taken with --marks?)")
    for k, name in enumerate(CONFIGS):
        part = recs[cuts[k] + 1:cuts[k + 1] if k + 1 < len(cuts) else len(recs)]
        # the order is taken per hardware queue: the downloads on the side stream run beside the kernels of the call's stream,
        # and which of two such neighbours starts first (they are ~0.2 us apart) is not a property of the code
        queues = {}
        for r in part:
            queues.setdefault(r["Queue_Id"], []).append(r["Kernel_Name"])
        full = "\n--\n".join("\n".join(names) for names in queues.values())
        short = [[re.split(r"[<(]", n.replace("void ", "", 1).replace("(anonymous namespace)::", ""))[0] for n in names]
                 for names in queues.values()]
        print(json.dumps({"config": name, "kernels": len(part), "sequence_sha256": hashlib.sha256(full.encode()).hexdigest(),
                          "sequence_per_queue": short}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines, with the canonical meta, to this file")
    ap.add_argument("--marks", action="store_true", help="launch a mark kernel in front of every configuration (for --split-trace)")
    ap.add_argument("--split-trace", default=None, metavar="CSV", help="cut a rocprofv3 kernel trace at the marks; runs nothing")
    args = ap.parse_args()
    if args.split_trace:
        split_trace(args.split_trace)
        return
    rows = run(args.marks)
    for row in rows:
        print(json.dumps({k: v for k, v in row.items() if k != "meta"}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(row) + "\n" for row in rows))


if __name__ == "__main__":
    main()
