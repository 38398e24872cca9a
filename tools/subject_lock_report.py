"""What the subject lock's reduction costs; writes the next free profiles/rNN_subject_lock.md.

  1. kernel time (HIP events, timing kind "mask_moments", median of 7) of vstab_mask_moments_batch over the masks of a
     256 x 1080p clip -- a moving disc of 5 % of the frame, an empty clip and an all-subject clip -- next to the
     plain warp of the same run, and as TB/s against the algorithmic 4 B per pixel;
  2. the same three with a build of the library whose kernel loads plainly instead of non-temporally (--variant LIB: a
     build with EXTRA=-DVSTAB_MASK_MOMENTS_PLAIN, measured in a child process that loads it through VSTAB_LIB);
  3. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` alternately in that tree and in this
     one, as child processes -- the default path calls nothing new, so the two must agree within the runs' own spread.

python tools/subject_lock_report.py [--frames N] [--variant LIB] [--parent DIR] [--out FILE]"""
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
ap.add_argument("--variant", default=None, help="a build of libvstab.so with -DVSTAB_MASK_MOMENTS_PLAIN")
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench alternation")
ap.add_argument("--bench-rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="where to write the profile (default: the next free profiles/rNN_subject_lock.md)")
ap.add_argument("--kernel-only", action="store_true", help="print the kernel times as one JSON line and stop (the child of --variant)")
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


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


def disc_masks():
    """A disc of radius 190 px (5 % of the frame) on a slow zig-zag, built on the device."""
    yy = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    k = torch.arange(n, device=dev, dtype=torch.float32)[:, None, None]
    cx = w / 2 + 300.0 * torch.sin(k * 0.21)
    cy = h / 2 + 150.0 * torch.cos(k * 0.13)
    return (((xx - cx) ** 2 + (yy - cy) ** 2) <= 190.0 ** 2).to(torch.float32).contiguous()


def kernel_rows(mask):
    rows = []
    for name, m in (("a disc of 5 % of the frame", mask), ("no subject", torch.zeros_like(mask)), ("all subject", torch.ones_like(mask))):
        ms, runs = timed("mask_moments", lambda: ctx.mask_moments_batch(m))
        rows.append((name, ms, runs))
        del m
    return rows


mask = disc_masks()
ctx.set_timing(True)
rows = kernel_rows(mask)
if args.kernel_only:
    print("KERNEL_ROWS " + json.dumps(rows))
    sys.exit(0)

frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "translation", *bench.FLOW_ARGS[2:], ctx=ctx,
                           keep_on_device=True, estimator="subject", subject_mask=mask)
final = tf.plan_from_meta(res.meta)["final_matrices"]
block = res.meta["subject_lock"]
warp_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
ctx.set_timing(False)
del res, frames, mask
torch.cuda.empty_cache()

variant_rows = None
if args.variant:
    env = dict(os.environ, VSTAB_LIB=str(Path(args.variant).resolve()))
    out = subprocess.run([sys.executable, __file__, "--frames", str(n), "--kernel-only"], env=env, capture_output=True, text=True, timeout=600)
    line = [l for l in out.stdout.splitlines() if l.startswith("KERNEL_ROWS ")]
    if out.returncode != 0 or not line:
        raise SystemExit(f"the variant run failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    variant_rows = json.loads(line[0][len("KERNEL_ROWS "):])

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
            bench_rows.append((r, name, j["ms_per_step"], j["value"], j["config"]["stage_ms"]["warp"]))

px = n * h * w
fmt = lambda runs: ", ".join(f"{v:.3f}" for v in runs)
lines = ["# Subject lock: what the mask reduction costs", "",
         f"`python tools/subject_lock_report.py --frames {n}`" + (" --variant ..." if args.variant else "") + (" --parent ..." if args.parent else "")
         + f" on one MI355X; HIP-event times, median of {reps} after one warm-up run.", "",
         f"## `vstab_mask_moments_batch`, {n} masks of {h}p ({px * 4 / 1e9:.2f} GB; plain warp of the same run: {warp_ms:.3f} ms)", "",
         "4 B per pixel is all the kernel reads; at the 6.3 TB/s the chip's streams reach that is "
         f"{px * 4 / 6.3e12 * 1e3:.3f} ms.", "",
         "| mask | loads | ms | / plain warp | TB/s against 4 B per pixel | runs ms |", "|---|---|---|---|---|---|"]
for label, table in (("non-temporal (shipped)", rows), ("plain (variant build)", variant_rows)):
    if table is None:
        continue
    for name, ms, runs in table:
        lines.append(f"| {name} | {label} | {ms:.3f} | {ms / warp_ms:.3f} | {px * 4 / (ms * 1e-3) / 1e12:.2f} | {fmt(runs)} |")
if variant_rows is None:
    lines += ["", "Plain loads: not measured in this run (no --variant build given)."]
lines += ["", f"The run itself (estimator=\"subject\", translation, the bench's strength and smooth): {block['mask_frames']} mask frames, "
              f"{block['frames_without_subject']} without a subject, {block['frames_touching_border']} touching the border, "
              f"area fraction {block['area_fraction_min']:.4f} .. {block['area_fraction_max']:.4f}.", ""]
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

if args.out:
    target = Path(args.out)
else:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    mine = sorted((ROOT / "profiles").glob("r*_subject_lock.md"))
    target = mine[-1] if mine else ROOT / "profiles" / f"r{max(taken) + 1:02d}_subject_lock.md"
target.parent.mkdir(parents=True, exist_ok=True)
target.write_text("\n".join(lines))
print("\n".join(lines))
print("written:", target)
