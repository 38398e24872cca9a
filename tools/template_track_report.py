"""What the template track costs; writes the next free profiles/rNN_template_track.md.

  1. kernel time (HIP events, timing kind "track_template", median of 7) of vstab_track_template_batch over the estimation
     images (960 x 540) of the bench's 256 x 1080p clip, for a box of 64 x 64 and of 256 x 256 working pixels at R = 24 and
     R = 48, keyed on frame 0, next to the plain warp of the same run;
  2. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` alternately in that tree and in this
     one, as child processes -- the default path launches nothing new, so the two must agree within the runs' own spread.

python tools/template_track_report.py [--frames N] [--parent DIR] [--out FILE]"""
import argparse
import json
import os
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench alternation")
ap.add_argument("--bench-rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="where to write the profile (default: the next free profiles/rNN_template_track.md)")
args = ap.parse_args()

import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from vstab_amd import native, template_track as tt

n, h, w, reps = args.frames, 1080, 1920, 7
dev = torch.device("cuda", 0)
ctx = native.Context(0)


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


frames = bench.synth_clip(n, 0, h, w, dev)
gray = ctx.gray_downscale(frames, (960, 540))
ctx.set_timing(True)
rows = []
for side in (64, 256):
    box = ((960 - side) // 2, (540 - side) // 2, side, side)
    for radius in (24, 48):
        ms, runs = timed("track_template", lambda: ctx.track_template_batch(gray, box, tt.stride_of(side, side), radius, 0))
        _, pos, best, _, _ = ctx.track_template_batch(gray, box, tt.stride_of(side, side), radius, 0)
        moved = int((pos.cpu().numpy() != np.array(box[:2])).any(axis=1).sum())
        rows.append((side, radius, ms, runs, moved))
eye = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
eye[:, 0, 2] = 3.25
warp_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, eye, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
ctx.set_timing(False)
del frames, gray
torch.cuda.empty_cache()

bench_rows = []
if args.parent:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-extras"]
    for r in range(args.bench_rounds):
        for name, tree in (("parent", Path(args.parent).resolve()), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "VSTAB_LIB"}
            out = subprocess.run(cmd, cwd=str(tree), env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("{") and '"ms_per_step"' in l]
            if out.returncode != 0 or not line:
                raise SystemExit(f"bench.py failed in {tree} ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            j = json.loads(line[-1])
            bench_rows.append((r, name, j["ms_per_step"], j["value"]))

fmt = lambda runs: ", ".join(f"{v:.3f}" for v in runs)
lines = ["# Template track: what following one box costs", "",
         f"`python tools/template_track_report.py --frames {n}`" + (" --parent ..." if args.parent else "")
         + f" on one MI355X; HIP-event times, median of {reps} after one warm-up run.", "",
         f"## `vstab_track_template_batch`, {n} estimation images of 960 x 540, key 0 (plain warp of {n} x {h}p in the same run: {warp_ms:.3f} ms)", "",
         f"One launch per frame and two more: {n + 1} dependent launches.", "",
         "| box | R | samples | ms | us per frame | / plain warp | frames that moved | runs ms |", "|---|---|---|---|---|---|---|---|"]
for side, radius, ms, runs, moved in rows:
    s = tt.stride_of(side, side)
    lines.append(f"| {side} x {side} | {radius} | {(side // s) ** 2} | {ms:.3f} | {ms / n * 1e3:.2f} | {ms / warp_ms:.3f} | {moved} | {fmt(runs)} |")
lines.append("")
if bench_rows:
    lines += ["## `bench.py --gpus 1 --steps 10 --warmup 3 --no-extras`, parent commit and this tree alternately on one box", "",
              "| round | tree | ms per step | frames/s |", "|---|---|---|---|"]
    for r, name, ms, value in bench_rows:
        lines.append(f"| {r} | {name} | {ms:.3f} | {value:.1f} |")
    for name in ("parent", "this"):
        v = [ms for _, nm, ms, _ in bench_rows if nm == name]
        lines += ["", f"{name}: median {np.median(v):.3f} ms per step, spread {min(v):.3f} .. {max(v):.3f}."]
    lines.append("")
else:
    lines += ["The bench alternation with the parent commit: not measured in this run (no --parent checkout given).", ""]

if args.out:
    target = Path(args.out)
else:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    target = ROOT / "profiles" / f"r{max(taken) + 1:02d}_template_track.md"
target.parent.mkdir(parents=True, exist_ok=True)
target.write_text("\n".join(lines))
print("\n".join(lines))
print("written:", target)
