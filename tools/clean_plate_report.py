"""What the clean plate costs; writes the next free profiles/rNN_clean_plate.md (or the one that exists).

  1. kernel times (HIP events, median of 7 after one warm-up) on the outputs of the C2 clip (256 frames of 1080p through the Flow
     pipeline, the warp's own padding masks) next to the plain warp OF THE SAME RUN: the median at S = 256 with and without the
     masks, against 16 B (12 B) per pixel and frame; the fill and the matte; short shots on either side of every sample count at
     which the median changes its kernel (native.PLATE_PATH_STEPS), as time per sample;
  2. the registers, LDS and scratch of the build (hipcc's own resource remarks for csrc/vstab_plate.hip);
  3. the quality figure of tests/test_clean_plate_gpu.py: PSNR of the plate and of the plain temporal mean against the rendered
     background, and the bound from the CPU restatement;
  4. with a directory as second argument: the `value` (frames/s) of the bench.py lines found there as bench_parent_<k>.log and
     bench_pr_<k>.log -- `bench.py --gpus 1 --steps 5 --warmup 2` run alternately in a checkout of the parent commit and in
     this tree.  Without it the section says NOT MEASURED.

python tools/clean_plate_report.py [frames] [directory of bench logs]"""
import json
import re
import subprocess
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from vstab_amd import clean_plate, flow_pipeline as fp, host_math as hm, native, temporal_fill

existing = sorted((ROOT / "profiles").glob("r*_clean_plate.md"))
numbers = [int(m.group(1)) for p in (ROOT / "profiles").glob("r*_*.md") if (m := re.match(r"r(\d+)_", p.name))]
PROFILE = existing[-1] if existing else ROOT / "profiles" / f"r{max(numbers, default=0) + 1:02d}_clean_plate.md"
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
logs = sys.argv[2] if len(sys.argv) > 2 else None
h, w, reps = 1080, 1920, 7
dev = torch.device("cuda", 0)
ctx = native.Context(0)
lines = ["# Clean plate: cost and quality", "",
         f"`python tools/clean_plate_report.py {n}` on one MI355X; HIP-event times, median of {reps} after one warm-up run.", ""]


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


def runs_text(runs):
    return ", ".join(f"{v:.3f}" for v in runs)


# ---- 1. cost --------------------------------------------------------------------------------------------------------------
frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", *bench.FLOW_ARGS[2:], ctx=ctx, keep_on_device=True)
final = temporal_fill.plan_from_meta(res.meta)["final_matrices"]
dst, mask = res.frames, res.masks[..., 0].contiguous()
del res
ctx.set_timing(True)
warp_ms, warp_runs = timed("warp", lambda: ctx.warp_batch(frames, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
px = n * h * w
lines += [f"## Kernel times, the outputs of {n} frames of {w} x {h} ({px * 12 / 1e9:.2f} GB of frames, {px * 4 / 1e9:.2f} GB of masks)", "",
          f"Plain warp of the same run: **{warp_ms:.3f} ms** ({runs_text(warp_runs)}).  Padded share of the clip: "
          f"{100 * float((mask > 0.5).float().mean()):.2f} %.", "",
          "| pass | ms | x warp | bytes counted | TB/s | runs ms |", "|---|---|---|---|---|---|"]
table = clean_plate.sample_table(None, n)
for name, m, per in (("median, S = %d, masks" % table.shape[1], mask, 16), ("median, S = %d, mask = NULL" % table.shape[1], None, 12)):
    ms, runs = timed("plate_median", lambda: ctx.plate_median_batch(dst, m, table))
    lines.append(f"| {name} | {ms:.3f} | {ms / warp_ms:.2f} | {per} B per pixel and sample + the plate | "
                 f"{(table.shape[1] * h * w * per + h * w * 16) / (ms * 1e-3) / 1e12:.3f} | {runs_text(runs)} |")
plate, count = ctx.plate_median_batch(dst, mask, table)
work, work_mask = dst.clone(), mask.clone()


def fill():
    work.copy_(dst)
    work_mask.copy_(mask)
    ctx.plate_fill_batch(work, work_mask, plate, count, None, 1)


ms, runs = timed("plate_fill", fill)
filled = int(ctx.plate_fill_batch(dst.clone(), mask.clone(), plate, count, None, 1).sum())
lines.append(f"| fill, min_count 1 ({100 * filled / px:.2f} % of the pixels filled) | {ms:.3f} | {ms / warp_ms:.2f} | 4 B per pixel (the mask) + 40 B per "
             f"pixel of a touched group | {(px * 4) / (ms * 1e-3) / 1e12:.3f} (the 4 B alone) | {runs_text(runs)} |")
ms, runs = timed("plate_matte", lambda: ctx.plate_matte_batch(dst, mask, plate, count, None, 0.1, 3))
lines.append(f"| matte, threshold 0.1, min_count 3 | {ms:.3f} | {ms / warp_ms:.2f} | 20 B per pixel and frame in, 4 B out (the plate and "
             f"its counts stay in cache) | {(px * 24) / (ms * 1e-3) / 1e12:.3f} | {runs_text(runs)} |")
del work, work_mask
lines += ["", "## Short shots: the median on either side of every change of kernel", "",
          "| S | kernel | ms | us per sample | TB/s at 16 B | runs ms |", "|---|---|---|---|---|---|"]
steps = native.PLATE_PATH_STEPS
for S in sorted(set([1, 2] + list(steps) + [s + 1 for s in steps] + [native.PLATE_SAMPLES_MAX])):
    if S > n:
        continue
    row = np.arange(S, dtype=np.int32)[None]
    ms, runs = timed("plate_median", lambda: ctx.plate_median_batch(dst, mask, row))
    form = ("registers, %d keys" % min(c for c in (4, 8, 16, 32, 64) if c >= S)) if S <= native.PLATE_REGISTER_MAX else \
        ("LDS, %d rows" % min(c for c in (128, 256) if c >= S))
    lines.append(f"| {S} | {form} | {ms:.3f} | {1e3 * ms / S:.2f} | {(S * h * w * 16 + h * w * 16) / (ms * 1e-3) / 1e12:.3f} | {runs_text(runs)} |")
ctx.set_timing(False)
lines.append("")
del frames, dst, mask, plate, count

# ---- 2. the build -----------------------------------------------------------------------------------------------------------
lines += ["## Build figures (`-Rpass-analysis=kernel-resource-usage`)", ""]
try:
    src = ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "vstab_plate.hip"
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-fno-slp-vectorize", "-fhip-fp32-correctly-rounded-divide-sqrt", "-c", str(src), "-o", "/dev/null",
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300).stderr
    fields = re.findall(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", out)
    lines += ["| kernel | VGPRs | SGPRs | scratch B/lane | waves/SIMD | LDS B/block |", "|---|---|---|---|---|---|"]
    columns = ("Function Name", "VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
    kernels = []
    for key, value in fields:
        if key == "Function Name":
            kernels.append({})
        kernels[-1][key] = value
    lines += ["| " + " | ".join(row[c] for c in columns) + " |" for row in kernels]
    lines.append("")
except Exception as exc:   # noqa: BLE001 -- a report without the compiler still has its other sections
    lines += [f"NOT MEASURED in this run ({type(exc).__name__}).", ""]

# ---- 3. quality -------------------------------------------------------------------------------------------------------------
lines += ["## Quality, the 12-frame 240 x 135 clip of tests/test_clean_plate_gpu.py", ""]
try:
    from oracle import oracle
    from tests import test_clean_plate_gpu as T
    from tests.drift_util import LOCK_ARGS, stabilize

    oracle.build()
    reference, ref_count, clip, bound, figures = T.quality_reference(oracle)
    base = stabilize(ctx, torch.from_numpy(clip).to(dev), "translation", LOCK_ARGS)
    p, c, _ = clean_plate.plate_on_device(ctx, base.frames, base.masks[..., 0].contiguous())
    p, c = p.cpu().numpy()[0], c.cpu().numpy()[0]
    where = (c >= 3) & (ref_count >= 3)
    mean = T.temporal_mean(base.frames.cpu().numpy(), base.masks.cpu().numpy()[..., 0])
    lines += [f"PSNR against the static background rendered through the true matrices with the oracle's warp, over the {int(where.sum())} of "
              f"{where.size} pixels with count >= 3: plate **{T.psnr_db(p, reference, where):.2f} dB**, plain temporal mean of the same frames "
              f"**{T.psnr_db(mean, reference, where):.2f} dB** (the subject stains it).  Bound, from the CPU restatement alone: the lowest of 8 "
              f"seeded runs with 0.05 px of error in every frame's true matrix, **{bound:.2f} dB** ({', '.join(f'{f:.2f}' for f in figures)}).", ""]
except Exception as exc:   # noqa: BLE001
    lines += [f"NOT MEASURED in this run ({type(exc).__name__}: {exc}).", ""]

# ---- 4. the default path ----------------------------------------------------------------------------------------------------
lines += ["## Default path: `bench.py --gpus 1 --steps 5 --warmup 2`, alternating parent / this tree", ""]
values = {}
for prefix in ("bench_parent", "bench_pr"):
    values[prefix] = []
    for path in sorted(Path(logs).glob(f"{prefix}_*.log")) if logs else []:
        rows = [ln for ln in path.read_text().splitlines() if ln.startswith("{")]
        if rows:
            values[prefix].append(float(json.loads(rows[-1])["value"]))
parent, pr = values["bench_parent"], values["bench_pr"]
if parent and pr:
    lines += ["| round | parent frames/s | this tree frames/s |", "|---|---|---|"]
    lines += [f"| {k + 1} | {a:.1f} | {b:.1f} |" for k, (a, b) in enumerate(zip(parent, pr))]
    lines += ["", f"Medians: parent {np.median(parent):.1f} ({min(parent):.1f} .. {max(parent):.1f}), this tree {np.median(pr):.1f} "
                  f"({min(pr):.1f} .. {max(pr):.1f}) frames/s ({100.0 * (np.median(pr) / np.median(parent) - 1.0):+.2f} %).  The default "
                  "path launches nothing new.", ""]
else:
    lines += ["NOT MEASURED in this run (no directory of bench logs was given).", ""]
PROFILE.write_text("\n".join(lines))
print("\n".join(lines))
