"""What the horizon level costs and how well it measures; writes the next free profiles/rNN_horizon_level.md (or the one
that exists).

  1. kernel time (HIP events, timing kind "orientation_hist", median of 7 after one warm-up) on the C2 working grid, 256
     estimation images of 540 x 960, for both content extremes -- the analytic structure upright (nearly every counted pixel
     in one bin) and random bytes (bins spread, every pixel counted) -- next to the scene-cut residual ("cut") OF THE SAME RUN,
     which has the same traffic of about one byte per working pixel;
  2. the registers, LDS and scratch of the build (hipcc's own resource remarks for csrc/vstab_level.hip);
  3. the accuracy figures of the tests: the restatement's worst single-frame error at 12 known rolls (CPU, true uint8 frames)
     and the roll of every output frame of the tilted test clip with and without horizon_level=True (HIP pipeline);
  4. with a directory as second argument: the `value` (frames/s) of the bench.py lines found there as bench_parent_<k>.log and
     bench_pr_<k>.log -- `bench.py --gpus 1 --steps 5 --warmup 2` run alternately in a checkout of the parent commit and in
     this tree.  Without it the section says NOT MEASURED.

python tools/horizon_level_report.py [frames] [directory of bench logs]"""
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
from tests import horizon_level_restatement as R
from vstab_amd import flow_pipeline as fp, horizon_level as hl, host_math as hm, native

existing = sorted((ROOT / "profiles").glob("r*_horizon_level.md"))
numbers = [int(m.group(1)) for p in (ROOT / "profiles").glob("r*_*.md") if (m := re.match(r"r(\d+)_", p.name))]
PROFILE = existing[-1] if existing else ROOT / "profiles" / f"r{max(numbers, default=0) + 1:02d}_horizon_level.md"
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
logs = sys.argv[2] if len(sys.argv) > 2 else None
h, w, reps = 540, 960, 7
dev = torch.device("cuda", 0)
ctx = native.Context(0)
lines = ["# Horizon level: cost and accuracy", "",
         f"`python tools/horizon_level_report.py {n}` on one MI355X; HIP-event times, median of {reps} after one warm-up run.", ""]


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


# ---- 1. cost --------------------------------------------------------------------------------------------------------------
upright = torch.from_numpy(R.Scene(size=(w, h)).render(0.0)).to(dev)
clips = {"analytic structure, upright (one hot bin)": upright[None].repeat(n, 1, 1).contiguous(),
         "random bytes (bins spread)": torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev,
                                                     generator=torch.Generator(device=dev).manual_seed(30))}
eye = np.tile(np.eye(3, dtype=np.float32), (n - 1, 1, 1))
ctx.set_timing(True)
lines += [f"## Kernel time, {n} estimation images of {w} x {h} ({n * h * w / 1e6:.1f} MB)", "",
          "| content | min_mag2 | counted pixels | fullest bin | orientation_hist ms | pair_residual ms (same run) | ratio | GB/s | runs ms |",
          "|---|---|---|---|---|---|---|---|---|"]
for name, gray in clips.items():
    cut_ms, _ = timed("cut", lambda: ctx.pair_residual_batch(gray, eye))
    for min_mag2 in (hl.MIN_MAG2, 0):
        ms, runs = timed("orientation_hist", lambda: ctx.orientation_hist_batch(gray, min_mag2))
        hist = ctx.orientation_hist_batch(gray[:1], min_mag2).cpu().numpy()[0]
        gx, gy, m2 = R.gradients(gray[0].cpu().numpy())
        counted = float(np.count_nonzero((m2 >= min_mag2) & (m2 > 0))) / m2.size
        lines.append(f"| {name} | {min_mag2} | {100 * counted:.1f} % | {100 * hist.max() / max(hist.sum(), 1):.1f} % of the mass | {ms:.3f} | "
                     f"{cut_ms:.3f} | {ms / cut_ms:.2f} | {n * h * w / (ms * 1e-3) / 1e9:.0f} | {', '.join(f'{v:.3f}' for v in runs)} |")
ctx.set_timing(False)
del clips
lines.append("")

# ---- 2. the build -----------------------------------------------------------------------------------------------------------
lines += ["## Build figures (`-Rpass-analysis=kernel-resource-usage`)", ""]
try:
    src = ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "vstab_level.hip"
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
    lines += ["", "(`ILb1E`: aligned 16-byte loads, `ILb0E`: byte loads.)", ""]
except Exception as exc:   # noqa: BLE001 -- a report without the compiler still has its other sections
    lines += [f"NOT MEASURED in this run ({type(exc).__name__}).", ""]

# ---- 3. accuracy ------------------------------------------------------------------------------------------------------------
scene = R.Scene()
rolls, conf = hl.frame_rolls(R.orientation_hist(np.stack([scene.render(r) for r in R.ACCURACY_ROLLS]), hl.MIN_MAG2))
err = hl.wrap90(rolls - np.asarray(R.ACCURACY_ROLLS))
gray, true = R.tilted_clip(scene, 7.0)
clip = torch.from_numpy(R.rgb_clip(gray)).to(dev)
args = ("crop_and_pad", "similarity", True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)
measured = {}
for name, kw in (("horizon_level=True", dict(horizon_level=True)), ("without the keyword", {})):
    run = fp._stabilize_frames(hm._normalize_video_input(clip), *args, ctx=ctx, keep_on_device=True, **kw)
    luma = R.luma_u8(run.frames.cpu().numpy())[:, 48:-48, 48:-48]
    measured[name] = np.array([hl.frame_roll(hist)[0] for hist in R.orientation_hist(luma, hl.MIN_MAG2)]), run.meta.get("horizon_level")
block = measured["horizon_level=True"][1]
lines += ["## Accuracy, the analytic clip (480 x 270: 40 rectangles with tanh edges, a horizon, weak sinusoids)", "",
          f"Restatement on uint8 frames rendered at the 12 rolls {list(R.ACCURACY_ROLLS)} (CPU): errors "
          f"{np.round(err, 4).tolist()} degrees, worst **{np.abs(err).max():.4f}**; confidence {conf.min():.2f} .. {conf.max():.2f}.  "
          f"tests/horizon_level_restatement.py holds MEASURED_WORST_DEG = {R.MEASURED_WORST_DEG}; the CPU test asserts 1.5 x, the GPU "
          "tests 2 x that figure.", "",
          "The tilted test clip (7 degrees, +-2 degrees of roll shake, 3 px of translation, similarity, camera_lock), every output "
          "frame's roll measured with the restatement on the interior of its luma:", "",
          "| run | rolls of the 12 output frames, degrees | worst distance from level |", "|---|---|---|"]
for name, (got, _) in measured.items():
    lines.append(f"| {name} | {np.round(got, 4).tolist()} | {np.abs(got).max():.4f} |")
lines += ["", f"Offset {block['offset_deg'][0]:.4f} degrees (true 7), confidence of the estimation images {min(block['confidence']):.3f} .. "
              f"{max(block['confidence']):.3f} -- these went through the RGB gray pass.", ""]

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
