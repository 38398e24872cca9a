"""What the sharpness transfer costs and what it buys; writes the next free profiles/rNN_sharpness_transfer.md.

  1. C2 clip (256 x 1080p): kernel time (HIP events, median of 7) of vstab_frame_sharpness_batch (timing kind "sharpness")
     and its TB/s against 12 B per pixel, and of vstab_sharp_transfer_batch ("sharp_transfer") at R = 1, 2 and 4 in two
     cases -- no frame blurred (no frame has a neighbour a tenth sharper: the cost of finding nothing to do) and every
     fourth frame blurred with a --blur x --blur box (31 by default: the clip's texture is band-limited to wavelengths of
     57 px and more, a 5 x 5 box takes 2 % of its gradient energy) -- next to the plain warp ("warp") of the same run, and the
     kernels' VGPR / scratch figures from the compiler's resource report; with --variant LIB (a build with
     EXTRA=-DVSTAB_SHARPNESS_PLAIN) the sharpness kernel with plain instead of non-temporal loads, measured in a child
     process that loads it through VSTAB_LIB, alternating with a child on the shipped library;
  2. the referee's clip (tests/sharpness_restatement.py: 9 frames of 160 x 120, frames 2 and 6 blurred, true matrices)
     through the two GPU entries at alpha 0, 4, 16 and 64: PSNR of the blurred frames against their sharp render;
  3. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` alternately in that tree and in this one,
     as child processes -- the default path launches nothing new, so the two must agree within the runs' own spread.

python tools/sharpness_transfer_report.py [--frames N] [--blur B] [--variant LIB] [--parent DIR] [--resources FILE] [--out FILE]
python tools/sharpness_transfer_report.py --resources-only     (needs no GPU: prints the resource figures as one JSON line)"""
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
ap.add_argument("--blur", type=int, default=31, help="odd side of the box that blurs every fourth frame of the C2 clip")
ap.add_argument("--variant", default=None, help="a build of libvstab.so with -DVSTAB_SHARPNESS_PLAIN")
ap.add_argument("--kernel-only", action="store_true", help="print the sharpness kernel's times as one JSON line and stop (the child of --variant)")
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the bench alternation")
ap.add_argument("--bench-rounds", type=int, default=3)
ap.add_argument("--resources", default=None, help="JSON written by --resources-only (default: compile the two sources now)")
ap.add_argument("--resources-only", action="store_true")
ap.add_argument("--out", default=None, help="where to write the profile (default: the next free profiles/rNN_sharpness_transfer.md)")
args = ap.parse_args()


def resource_report():
    """{kernel instance: {vgprs, sgprs, scratch, occupancy, lds}} of the two new kernels, from hipcc's kernel-resource-usage
    remarks with the Makefile's flags."""
    csrc = ROOT / "comfyui-video-stabilizer_amd" / "csrc"
    flags = re.search(r"^CXXFLAGS = (.*?)\n(?!\s)", (csrc / "Makefile").read_text(), flags=re.S | re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    table = {}
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "LDS Size [bytes/block]": "lds"}
    for source in ("vstab_sharp.hip", "vstab_neighbour.hip"):
        with tempfile.TemporaryDirectory() as tmp:
            out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-Rpass-analysis=kernel-resource-usage", "-c",
                                  source, "-o", str(Path(tmp) / "out.o")], cwd=str(csrc), capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit(f"hipcc failed:\n{out.stderr[-3000:]}")
        name = None
        for line in out.stderr.splitlines():
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                f, name = m.group(1), None
                if "frame_sharpness_kernel" in f:
                    name = "frame_sharpness_kernel"
                elif "sharp_transfer_kernel" in f:
                    name = "sharp_transfer_kernel<" + ("bicubic" if re.search(r"sharp_transfer_kernelILi(\d)E", f).group(1) == "1" else "bilinear") + ">"
                if name:
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
from tests import sharpness_restatement as S
from vstab_amd import flow_pipeline as fp, host_math as hm, native, sharpness_transfer as st, temporal_fill as tf

resources = json.loads(Path(args.resources).read_text()) if args.resources else resource_report()
n, h, w, reps = args.frames, 1080, 1920, 7
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
if args.kernel_only:
    ctx.set_timing(True)
    ms, runs = timed("sharpness", lambda: ctx.frame_sharpness_batch(frames))
    print("KERNEL_ROW " + json.dumps({"ms": ms, "runs": runs}))
    sys.exit(0)
res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
plan = tf.plan_from_meta(res.meta)
final = plan["final_matrices"]
mask = res.masks[..., 0].contiguous().clone()
del res
# the same clip with every fourth frame blurred by a box (border replicated); the motion, hence the plan, is the same
blurred = frames.clone()
idx = torch.arange(2, n, 4, device=dev)
for i in idx.tolist():
    f = blurred[i].permute(2, 0, 1)[None]
    blurred[i] = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(f, (args.blur // 2,) * 4, mode="replicate"), args.blur, stride=1)[0].permute(1, 2, 0)
torch.cuda.synchronize()

ctx.set_timing(True)
rows = []
warp_ms, runs = timed("warp", lambda: ctx.warp_batch(frames, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
rows.append(("plain warp", warp_ms, runs, ""))
sharp_ms, runs = timed("sharpness", lambda: ctx.frame_sharpness_batch(frames))
rows.append(("frame sharpness", sharp_ms, runs, f"{n * h * w * 12 / sharp_ms / 1e9:.2f} TB/s against 12 B per pixel"))
ratio_note = ""
for label, clip in (("no frame blurred", frames), ("every fourth frame blurred", blurred)):
    energy = ctx.frame_sharpness_batch(clip).cpu().numpy()
    if clip is blurred:
        q = energy[np.clip(idx.cpu().numpy() - 1, 0, n - 1)] / np.maximum(energy[idx.cpu().numpy()], 1)
        ratio_note = (f"Every fourth frame (i % 4 == 2) is blurred with a {args.blur} x {args.blur} box, border replicated; the energy of "
                      f"the frame before it is {q.min():.2f} .. {q.max():.2f} times its own.")
    warped = ctx.warp_batch(clip, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=False)[0]
    dst = warped.clone()
    for radius in (1, 2, 4):
        mats, cand = tf.fill_candidates(final, plan["transitions"], plan["confidences"], radius)
        ratios = st.ratios_from_energy(energy, cand)
        live = int((ratios > 0).any(axis=1).sum())
        counts = {}

        def call():
            counts["px"] = int(ctx.sharp_transfer_batch(clip, mats, cand, ratios, st.DEFAULT_ALPHA, dst, mask).sum())

        ms, runs = timed("sharp_transfer", call, lambda: dst.copy_(warped))
        rows.append((f"transfer, R = {radius}, {label}", ms, runs,
                     f"{live} of {n} frames borrow, {int((ratios > 0).sum())} candidates sampled, {counts['px']} pixels written "
                     f"({counts['px'] / (n * h * w) * 100:.2f} % of the clip)"))
    del warped, dst
ctx.set_timing(False)
del frames, blurred, mask
torch.cuda.empty_cache()

variant_rows = []
if args.variant:   # plain against non-temporal loads: two children per round, alternately, each a median of 7
    me = [sys.executable, str(Path(__file__).resolve()), "--kernel-only", "--frames", str(n)]
    for r in range(2):
        for name, lib in (("plain loads (variant build)", str(Path(args.variant).resolve())), ("non-temporal loads (shipped)", None)):
            env = {k: v for k, v in os.environ.items() if k != "VSTAB_LIB"}
            if lib:
                env["VSTAB_LIB"] = lib
            out = subprocess.run(me, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("KERNEL_ROW ")]
            if out.returncode != 0 or not line:
                raise SystemExit(f"the {name} run failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            j = json.loads(line[0][len("KERNEL_ROW "):])
            variant_rows.append((r, name, j["ms"], j["runs"]))

# ---- 2. the referee's clip, alpha sweep -----------------------------------------------------------------------------------
clip = S.referee_clip()
src = torch.from_numpy(clip["frames"]).to(dev)
fh, fw = clip["frames"].shape[1:3]
d0, m0, _ = ctx.warp_batch(src, clip["final"], (fw, fh), border=(0.5, 0.5, 0.5), want_mask=True)
truth = ctx.warp_batch(torch.from_numpy(clip["sharp"]).to(dev), clip["final"], (fw, fh), border=(0.5, 0.5, 0.5), want_mask=False)[0].cpu().numpy()
energy = ctx.frame_sharpness_batch(src).cpu().numpy()
ratios = st.ratios_from_energy(energy, clip["cand_frame"])
own = m0.cpu().numpy() == 0
before = [S.psnr(d0[i].cpu().numpy(), truth[i], own[i]) for i in clip["blurred"]]
sweep = []
for alpha in (0.0, 4.0, 16.0, 64.0):
    d = d0.clone()
    ctx.sharp_transfer_batch(src, clip["matrices"], clip["cand_frame"], ratios, alpha, d, m0)
    after = [S.psnr(d[i].cpu().numpy(), truth[i], own[i]) for i in clip["blurred"]]
    sweep.append((alpha, after, float(np.mean(np.subtract(after, before)))))

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
lines = ["# Sharpness transfer: cost of the two kernels, gain on the referee's clip", "",
         f"`python tools/sharpness_transfer_report.py --frames {n}`" + (" --parent ..." if args.parent else "")
         + f" on one MI355X; HIP-event times, median of {reps} after one warm-up run; dst is restored in front of every transfer.", "",
         f"## C2 clip, {n} x {h}p, alpha = {st.DEFAULT_ALPHA:g}, the stabilizer's own plan and padding mask", "",
         "| kernel | ms | / plain warp | | runs ms |", "|---|---|---|---|---|"]
for name, ms, runs, note in rows:
    lines.append(f"| {name} | {ms:.3f} | {ms / warp_ms:.2f} | {note} | {fmt(runs)} |")
lines += ["", ratio_note]
if variant_rows:
    lines += ["", "The sharpness kernel in child processes, plain against non-temporal pixel loads, alternately:", "",
              "| round | loads | ms | TB/s against 12 B per pixel | runs ms |", "|---|---|---|---|---|"]
    for r, name, ms, runs in variant_rows:
        lines.append(f"| {r} | {name} | {ms:.3f} | {n * h * w * 12 / ms / 1e9:.2f} | {fmt(runs)} |")
else:
    lines += ["", "Plain against non-temporal loads: not measured in this run (no --variant build given)."]
lines += ["", "Compiler's resource report (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
          "| kernel | VGPRs | SGPRs | scratch B/lane | waves/SIMD | LDS B |", "|---|---|---|---|---|---|"]
for name, r in sorted(resources.items()):
    lines.append(f"| `{name}` | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('scratch')} | {r.get('occupancy')} | {r.get('lds')} |")
lines += ["", f"## Referee's clip ({clip['frames'].shape[0]} frames of {fw} x {fh}, frames {clip['blurred']} blurred with a 5 x 5 box, noise "
          "sigma 0.005, true matrices, R = 2): PSNR against the sharp render", "",
          f"Energy ratio of a sharp neighbour to a blurred frame: {float(ratios[ratios > 0].min()):.2f} .. {float(ratios.max()):.2f}.  "
          "Before the transfer: " + ", ".join(f"{v:.2f}" for v in before) + " dB.", "",
          "| alpha | " + " | ".join(f"frame {i} dB" for i in clip["blurred"]) + " | mean gain dB |", "|---|" + "---|" * (len(clip["blurred"]) + 1)]
for alpha, after, gain in sweep:
    lines.append(f"| {alpha:g} | " + " | ".join(f"{v:.2f}" for v in after) + f" | {gain:.2f} |")
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
    lines += ["`bench.py` against the parent commit: not measured in this run (no --parent tree given).", ""]

if args.out:
    target = Path(args.out)
else:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    mine = sorted((ROOT / "profiles").glob("r*_sharpness_transfer.md"))
    target = mine[-1] if mine else ROOT / "profiles" / f"r{max(taken) + 1:02d}_sharpness_transfer.md"
target.parent.mkdir(parents=True, exist_ok=True)
target.write_text("\n".join(lines))
print("\n".join(lines))
print("written:", target)
