"""What the padded-pixel count costs the plain warp: the bench shape (256 x 1080p -> same size, bilinear, q5, mask on)
through ctx.warp_batch with want_count=True and want_count=False, interleaved, HIP events around every launch.
The count is free if the difference of the medians is not larger than the spread (max - min) of one form's launches.
   python tools/warp_count_cost.py [--n 256] [--reps 9]          (VSTAB_LIB=... measures another build of the library)
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as graft

graft.load_package()
from vstab_amd import native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--h", type=int, default=1080)
ap.add_argument("--w", type=int, default=1920)
ap.add_argument("--reps", type=int, default=9, help="timed launches of each form (at least 7)")
args = ap.parse_args()
assert args.reps >= 7

ctx = native.default_context()
n, h, w = args.n, args.h, args.w
frames = torch.rand((n, h, w, 3), device="cuda", dtype=torch.float32)
rng = np.random.default_rng(0)
# a stabilizing clip's corrections: small rotation and zoom, a translation of some pixels (crop_and_pad pads the rim only)
mats = np.tile(np.eye(3), (n, 1, 1))
th, sc = rng.uniform(-0.01, 0.01, n), rng.uniform(0.99, 1.01, n)
mats[:, 0, 0] = sc * np.cos(th); mats[:, 0, 1] = -sc * np.sin(th)
mats[:, 1, 0] = sc * np.sin(th); mats[:, 1, 1] = sc * np.cos(th)
mats[:, 0, 2] = rng.uniform(-20, 20, n); mats[:, 1, 2] = rng.uniform(-12, 12, n)
mats = mats.astype(np.float32)
border = np.array([127, 127, 127], np.float32) / 255
dst = torch.empty((n, h, w, 3), device="cuda")
mask = torch.empty((n, h, w), device="cuda")


def launch(count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ctx.warp_batch(frames, mats, (w, h), interp="bilinear", border=border, subpix="q5", want_mask=True, want_count=count, out=dst, out_mask=mask)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for _ in range(2):
    launch(True), launch(False)
ms = {True: [], False: []}
for _ in range(args.reps):
    for count in (True, False):
        ms[count].append(launch(count))
med = {k: float(np.median(v)) for k, v in ms.items()}
spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
diff = med[True] - med[False]
print(json.dumps({
    "shape": [n, h, w], "launches_each": args.reps, "library": str(native.LIB_PATH),
    "count_ms": [round(v, 4) for v in ms[True]], "no_count_ms": [round(v, 4) for v in ms[False]],
    "median_count_ms": round(med[True], 4), "median_no_count_ms": round(med[False], 4), "median_difference_ms": round(diff, 4),
    "spread_count_ms": round(spread[True], 4), "spread_no_count_ms": round(spread[False], 4),
    "count_is_free": bool(diff <= max(spread.values())),
}))
