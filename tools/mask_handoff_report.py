"""What the mask hand-off costs; writes the next free profiles/rNN_mask_handoff.md.

  1. kernel time (HIP events, timing kinds "mask_grow" and "mask_hold", median of 7) over the padding masks of the C2 clip
     (256 x 1080p, the masks of a Flow run of the bench's clip) of: grow 5 tapered, grow 5 square, grow 16 + feather 16,
     grow 64, hold 2 -- each next to the plain warp of the same run, and as TB/s against the algorithmic bytes: 8 B per pixel
     and pass (one read, one write) for the grow, 4 (2T + 2) B per pixel for the hold;
  2. in the same run, ComfyUI GrowMask's own loop (scipy grey_dilation, 3 x 3, once per pixel of growth) on 8 of those masks
     on the host, expand 5, both footprints -- per frame, and scaled to the clip -- and that its result equals the kernel's;
  3. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` alternately in that tree and in this
     one, as child processes -- the default path calls nothing new, so the two must agree within the runs' own spread.

python tools/mask_handoff_report.py [--frames N] [--parent DIR] [--out FILE]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench alternation")
ap.add_argument("--bench-rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="where to write the profile (default: the next free profiles/rNN_mask_handoff.md)")
args = ap.parse_args()

import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from vstab_amd import flow_pipeline as fp, host_math as hm, native, temporal_fill as tf

n, h, w, reps = args.frames, 1080, 1920, 7
dev = torch.device("cuda", 0)
ctx = native.Context(0)
STEPS = 16   # one-pixel steps per pass (csrc/vstab_handoff.hip: MH_MAX_STEPS)


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", *bench.FLOW_ARGS[2:], ctx=ctx, keep_on_device=True)
mask = res.masks[..., 0].contiguous()
final = tf.plan_from_meta(res.meta)["final_matrices"]
padding = float(res.meta["padding_fraction_mean"])
del res
ctx.set_timing(True)
warp_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
del frames
torch.cuda.empty_cache()

out = torch.empty_like(mask)
px = n * h * w
rows = []
for name, grow, tapered, feather in (("grow 5, tapered", 5, True, 0), ("grow 5, square", 5, False, 0), ("grow 16 + feather 16, tapered", 16, True, 16),
                                     ("grow 64, tapered", 64, True, 0), ("grow 64, square", 64, False, 0)):
    ms, runs = timed("mask_grow", lambda: ctx.mask_grow_batch(mask, grow, tapered=tapered, feather=feather, want_count=True, out=out))
    passes = max(1, -(-(abs(grow) + feather) // STEPS))
    rows.append((name, passes, 8 * passes, ms, runs))
hold_ms, hold_runs = timed("mask_hold", lambda: ctx.mask_hold_batch(mask, 2))
rows.append(("hold 2", 1, 4 * (2 * 2 + 2), hold_ms, hold_runs))
ctx.set_timing(False)

# GrowMask's own loop on the host, on 8 of the same masks
import scipy
import scipy.ndimage

pick = np.linspace(0, n - 1, 8).astype(int)
host = mask[torch.as_tensor(pick, device=dev)].cpu().numpy()
cpu_rows = []
for tapered in (True, False):
    c = 0 if tapered else 1
    kernel = np.array([[c, 1, c], [1, 1, 1], [c, 1, c]])
    t0 = time.perf_counter()
    grown = []
    for f in host:
        o = f
        for _ in range(5):
            o = scipy.ndimage.grey_dilation(o, footprint=kernel)
        grown.append(o)
    sec = (time.perf_counter() - t0) / len(host)
    same = bool(np.array_equal(np.stack(grown).view(np.uint32),
                               ctx.mask_grow_batch(torch.from_numpy(host).to(dev), 5, tapered=tapered).cpu().numpy().view(np.uint32)))
    cpu_rows.append(("tapered" if tapered else "square", sec, same))
del mask, out
torch.cuda.empty_cache()

bench_rows = []
if args.parent:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-extras"]
    for r in range(args.bench_rounds):
        for name, tree in (("parent", Path(args.parent).resolve()), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "VSTAB_LIB"}
            run = subprocess.run(cmd, cwd=str(tree), env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in run.stdout.splitlines() if l.startswith("{") and '"ms_per_step"' in l]
            if run.returncode != 0 or not line:
                raise SystemExit(f"bench.py failed in {tree} ({run.returncode}):\n{run.stdout[-2000:]}\n{run.stderr[-2000:]}")
            j = json.loads(line[-1])
            bench_rows.append((r, name, j["ms_per_step"], j["value"], j["config"]["stage_ms"]["warp"]))

fmt = lambda runs: ", ".join(f"{v:.3f}" for v in runs)
lines = ["# Mask hand-off: what hold, grow and feather cost", "",
         f"`python tools/mask_handoff_report.py --frames {n}`" + (" --parent ..." if args.parent else "")
         + f" on one MI355X; HIP-event times, median of {reps} after one warm-up run.", "",
         f"## The padding masks of a Flow run of the bench's clip, {n} x {h}p ({px * 4 / 1e9:.2f} GB, mean padding fraction {padding:.4f}; "
         f"plain warp of the same run: {warp_ms:.3f} ms)", "",
         "Algorithmic bytes: a grow / feather pass reads and writes every pixel once (8 B per pixel and pass; a pass is up to "
         f"{STEPS} one-pixel steps), the hold reads 2T + 1 frames and writes one (4 (2T + 2) B per pixel).  The stability and "
         "subject passes reach about 6 TB/s.", "",
         "| call | passes | B per pixel | ms | / plain warp | TB/s against those bytes | ms per pass | runs ms |", "|---|---|---|---|---|---|---|---|"]
for name, passes, bpp, ms, runs in rows:
    lines.append(f"| {name} | {passes} | {bpp} | {ms:.3f} | {ms / warp_ms:.3f} | {px * bpp / (ms * 1e-3) / 1e12:.2f} | {ms / passes:.3f} | {fmt(runs)} |")
lines += ["", f"## GrowMask's own loop on the host (scipy {scipy.__version__}, one thread), expand 5, 8 of the same masks", "",
          "| footprint | s per 1080p frame | scaled to the clip, s | kernel of the same footprint, ms | ratio | same bits as the kernel |", "|---|---|---|---|---|---|"]
for (name, sec, same), (_, _, _, ms, _) in zip(cpu_rows, rows[:2]):
    lines.append(f"| {name} | {sec:.4f} | {sec * n:.1f} | {ms:.3f} | {sec * n / (ms * 1e-3):.0f} | {'yes' if same else 'NO'} |")
lines.append("")
if bench_rows:
    lines += ["## `bench.py --gpus 1 --steps 10 --warmup 3 --no-extras`, parent commit and this tree alternately on one box", "",
              "| round | tree | ms per step | frames/s | warp ms |", "|---|---|---|---|---|"]
    for r, name, ms, value, warp in bench_rows:
        lines.append(f"| {r} | {name} | {ms:.3f} | {value:.1f} | {warp:.3f} |")
    for name in ("parent", "this"):
        v = [ms for _, nm, ms, _, _ in bench_rows if nm == name]
        lines.append("")
        lines.append(f"{name}: median {np.median(v):.3f} ms per step, spread {min(v):.3f} .. {max(v):.3f}.")
    lines.append("")
else:
    lines += ["The bench alternation with the parent commit: NOT MEASURED in this run (no --parent given).", ""]

if args.out:
    target = Path(args.out)
else:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    mine = sorted((ROOT / "profiles").glob("r*_mask_handoff.md"))
    target = mine[-1] if mine else ROOT / "profiles" / f"r{max(taken) + 1:02d}_mask_handoff.md"
target.parent.mkdir(parents=True, exist_ok=True)
target.write_text("\n".join(lines))
print("\n".join(lines))
print("written:", target)
