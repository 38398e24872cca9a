"""What the blended temporal fill costs and what it buys; writes the next free profiles/rNN_fill_blend.md.

  1. C2 clip (256 x 1080p), R = 8: kernel time (HIP events, median of 7) of vstab_fill_gain_sums (timing kind "fill_gain")
     and of vstab_temporal_fill_blend_batch ("fill_blend") at feather 0, 16 and 64, next to the plain fill ("fill") and the
     plain warp ("warp") of the same run, and the blended fill's VGPR / scratch figures from the compiler's resource report;
  2. flicker clip (windows of one texture at integer offsets, frame j times 0.8 / 1.25): PSNR of the filled and blended
     pixels against a_i * texture for the hard fill, exposure only, and exposure plus feather 16;
  3. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` alternately in that tree and in this one,
     as child processes -- the default path launches nothing new, so the two must agree within the runs' own spread.

python tools/fill_blend_report.py [--frames N] [--parent DIR] [--resources FILE] [--out FILE]
python tools/fill_blend_report.py --resources-only     (needs no GPU: prints the resource figures as one JSON line)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--radius", type=int, default=8)
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench alternation")
ap.add_argument("--bench-rounds", type=int, default=3)
ap.add_argument("--resources", default=None, help="JSON written by --resources-only (default: compile csrc/vstab_neighbour.hip now)")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--out", default=None, help="where to write the profile (default: the next free profiles/rNN_fill_blend.md)")
args = ap.parse_args()


def resource_report():
    """{kernel instance: {vgprs, sgprs, scratch, occupancy, lds}} of the fill kernels, from hipcc's kernel-resource-usage
    remarks on csrc/vstab_neighbour.hip with the Makefile's flags."""
    csrc = ROOT / "comfyui-video-stabilizer_amd" / "csrc"
    flags = re.search(r"^CXXFLAGS = (.*?)\n(?!\s)", (csrc / "Makefile").read_text(), flags=re.S | re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-Rpass-analysis=kernel-resource-usage", "-c",
                              "vstab_neighbour.hip", "-o", str(Path(tmp) / "neighbour.o")], cwd=str(csrc), capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit(f"hipcc failed:\n{out.stderr[-3000:]}")
    table, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "LDS Size [bytes/block]": "lds"}
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            f = m.group(1)
            name = None
            for kern in ("temporal_fill_blend_kernel", "fill_gain_sums_kernel", "temporal_fill_kernel"):
                if kern in f:
                    params = re.search(kern + r"ILi(\d)E(?:Li(\d)E)?", f)
                    name = kern + "<" + ("bicubic" if params.group(1) == "1" else "bilinear") + (", exact" if params.group(2) == "1" else "") + ">"
                    table[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1) in keys:
            table[name][keys[m.group(1)]] = int(m.group(2))
    return table


if args.resources_only:
    print(json.dumps(resource_report()))
    sys.exit(0)

import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from tests import fill_blend_restatement as B
from vstab_amd import flow_pipeline as fp, host_math as hm, native, temporal_fill as tf

resources = json.loads(Path(args.resources).read_text()) if args.resources else resource_report()
n, h, w, reps, radius = args.frames, 1080, 1920, 7, args.radius
dev = torch.device("cuda", 0)
ctx = native.Context(0)


def timed(kind, call, prepare=lambda: None):
    ms = []
    for _ in range(reps + 1):
        prepare()
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


# ---- 1. the C2 clip ----------------------------------------------------------------------------------------------------
frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
plan = tf.plan_from_meta(res.meta)
final = plan["final_matrices"]
mats, cand = tf.fill_candidates(final, plan["transitions"], plan["confidences"], radius)
ones = np.ones(cand.shape + (3,), np.float32)
warped, mask0 = res.frames.clone(), res.masks[..., 0].contiguous().clone()
padded_share = float((mask0 == 1.0).float().mean())
del res
dst, mask = warped.clone(), mask0.clone()


def reset():
    dst.copy_(warped)
    mask.copy_(mask0)


ctx.set_timing(True)
rows = []
warp_ms, runs = timed("warp", lambda: ctx.warp_batch(frames, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
rows.append(("plain warp", warp_ms, runs, ""))
fill_ms, runs = timed("fill", lambda: ctx.temporal_fill_batch(frames, mats, cand, dst, mask), reset)
rows.append((f"plain fill, R = {radius}", fill_ms, runs, ""))
gain_ms, runs = timed("fill_gain", lambda: ctx.fill_gain_sums(frames, mats, cand, final, warped))
sums = ctx.fill_gain_sums(frames, mats, cand, final, warped).cpu().numpy()
gains = tf.gains_from_sums(sums)
rows.append(("gain sums", gain_ms, runs, f"{int((sums[..., 0] > 0).sum())} of {cand.size} pairs counted, {int(sums[..., 0].sum())} lattice pixels"))
for feather, g, label in ((0, ones, "gains 1"), (0, gains, "measured gains"), (16, gains, "measured gains"), (64, gains, "measured gains")):
    counts = {}

    def call():
        _, fc, pc, bc = ctx.temporal_fill_blend_batch(frames, mats, cand, final, g, dst, mask, feather_px=feather)
        counts["filled"], counts["blended"] = int(fc.sum()), int(bc.sum())

    ms, runs = timed("fill_blend", call, reset)
    rows.append((f"blended fill, feather {feather}, {label}", ms, runs,
                 f"{counts['filled']} filled, {counts['blended']} blended ({counts['blended'] / (n * h * w) * 100:.3f} % of the pixels)"))
ctx.set_timing(False)
del frames, warped, mask0, dst, mask
torch.cuda.empty_cache()

# ---- 2. the flicker clip ---------------------------------------------------------------------------------------------
clip = B.flicker_clip()
src = torch.from_numpy(clip["frames"]).to(dev)
fh, fw = clip["frames"].shape[1:3]
d0, m0, _ = ctx.warp_batch(src, clip["final"], (fw, fh), border=(0.5, 0.5, 0.5), want_mask=True)
fsums = ctx.fill_gain_sums(src, clip["matrices"], clip["cand_frame"], clip["final"], d0).cpu().numpy()
fgains = tf.gains_from_sums(fsums)
unit = np.ones_like(fgains)
d, m = d0.clone(), m0.clone()
ff, _, _, _ = ctx.temporal_fill_blend_batch(src, clip["matrices"], clip["cand_frame"], clip["final"], fgains, d, m, feather_px=16,
                                            want_filled_from=True)
region = ff.cpu().numpy() >= 0                      # the pixels exposure + feather 16 writes: filled and blended
filled_region = region & (m0.cpu().numpy() == 1.0)
truth = clip["truth"].astype(np.float64)


def psnr(err2):
    return float(10.0 * np.log10(1.0 / max(float(err2), 1e-20)))


quality = []
for label, g, feather in (("hard fill", unit, 0), ("exposure only", fgains, 0), ("exposure + feather 16", fgains, 16)):
    d, m = d0.clone(), m0.clone()
    ctx.temporal_fill_blend_batch(src, clip["matrices"], clip["cand_frame"], clip["final"], g, d, m, feather_px=feather)
    err2 = ((d.cpu().numpy().astype(np.float64) - truth) ** 2).mean(axis=-1)
    quality.append((label, psnr(err2[filled_region].mean()), psnr(err2[region & ~filled_region].mean()), psnr(err2[region].mean())))

# ---- 3. bench.py, parent and this tree alternately -------------------------------------------------------------------------
bench_rows = []
if args.parent:
    del ctx
    torch.cuda.empty_cache()
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

fmt = lambda runs: ", ".join(f"{v:.3f}" for v in runs)
lines = ["# Blended temporal fill: cost of the two kernels, quality on a flickering clip", "",
         f"`python tools/fill_blend_report.py --frames {n}`" + (" --parent ..." if args.parent else "")
         + f" on one MI355X; HIP-event times, median of {reps} after one warm-up run; dst and mask are restored in front of every fill.", "",
         f"## C2 clip, {n} x {h}p, R = {radius} (K = {2 * radius}), {padded_share * 100:.3f} % of the pixels padded after the warp", "",
         "| kernel | ms | / plain fill | / plain warp | | runs ms |", "|---|---|---|---|---|---|"]
for name, ms, runs, note in rows:
    lines.append(f"| {name} | {ms:.3f} | {ms / fill_ms:.2f} | {ms / warp_ms:.2f} | {note} | {fmt(runs)} |")
lines += ["", "Compiler's resource report (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
          "| kernel | VGPRs | SGPRs | scratch B/lane | waves/SIMD | LDS B |", "|---|---|---|---|---|---|"]
for name, r in sorted(resources.items()):
    lines.append(f"| `{name}` | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('scratch')} | {r.get('occupancy')} | {r.get('lds')} |")
lines += ["", f"## Flicker clip ({clip['frames'].shape[0]} frames of {fw} x {fh}, gains 0.8 / 1.25, radius 1): PSNR against a_i * texture", "",
          f"Over the pixels that exposure + feather 16 writes: {int(filled_region.sum())} filled, {int((region & ~filled_region).sum())} blended "
          "(own pixels within the feather; the hard fill and exposure only leave them as the warp wrote them, fringe ring included).", "",
          "| fill | filled pixels dB | feather pixels dB | both dB |", "|---|---|---|---|"]
for label, a, b, c in quality:
    lines.append(f"| {label} | {a:.2f} | {b:.2f} | {c:.2f} |")
lines += ["", "200.00 dB is the floor of the PSNR function: no error at all.  Under integer translations every bilinear weight is 1, 0, 0, 0, so "
          "the frame's own pixels are exact, fringe ring included: on this clip the feather can only show that it costs nothing.", ""]
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
    lines += ["`bench.py` against the parent commit: not measured in this run (no --parent tree given).", ""]

if args.out:
    target = Path(args.out)
else:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    mine = sorted((ROOT / "profiles").glob("r*_fill_blend.md"))
    target = mine[-1] if mine else ROOT / "profiles" / f"r{max(taken) + 1:02d}_fill_blend.md"
target.parent.mkdir(parents=True, exist_ok=True)
target.write_text("\n".join(lines))
print("\n".join(lines))
print("written:", target)
