"""What the spatial fill costs and what it is worth; writes profiles/r13_spatial_fill.md.

  1. kernel time (HIP events, timing kind "sfill") on the C2 clip (256 x 1080p, bench.FLOW_ARGS) after the plain warp, after
     the warp + temporal_fill=8, and on a clip whose padded share is about 5 %, each next to the plain warp of the same run;
  2. PSNR of the filled pixels against the analytic texture on a camera-locked shaken clip, next to black and to the
     frame's mean colour.

  3. with a directory as second argument: the `value` (frames/s) of the bench.py lines found there as bench_parent_<k>.log and
     bench_pr_<k>.log -- `bench.py --gpus 1 --steps 5 --warmup 2` run alternately in a checkout of the parent commit and in
     this tree -- as a table with the parent's own spread.

python tools/spatial_fill_accuracy.py [frames [bench-log-directory]]   |   ... bench-table <bench-log-directory>"""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np


def bench_table(directory):
    """Section 3 from the bench.py lines in `directory` (needs no GPU)."""
    def values(prefix):
        out = []
        for path in sorted(Path(directory).glob(f"{prefix}_*.log")):
            last = [ln for ln in path.read_text().splitlines() if ln.startswith("{")][-1]
            out.append(float(json.loads(last)["value"]))
        return out
    parent, pr = values("bench_parent"), values("bench_pr")
    if not (parent and pr):
        return []
    out = ["", "## Default path: `bench.py --gpus 1 --steps 5 --warmup 2`, alternating parent / this tree", "",
           "| round | parent frames/s | this tree frames/s |", "|---|---|---|"]
    out += [f"| {k + 1} | {a:.1f} | {b:.1f} |" for k, (a, b) in enumerate(zip(parent, pr))]
    spread = (max(parent) - min(parent)) / float(np.median(parent))
    return out + ["", f"Medians: parent {np.median(parent):.1f}, this tree {np.median(pr):.1f} frames/s "
                      f"({100.0 * (np.median(pr) / np.median(parent) - 1.0):+.2f} %); the parent's own spread over its runs: "
                      f"{100.0 * spread:.2f} %.", ""]


PROFILE = ROOT / "profiles" / "r13_spatial_fill.md"
if len(sys.argv) > 2 and sys.argv[1] == "bench-table":   # add section 3 to a profile written earlier
    PROFILE.write_text(PROFILE.read_text().rstrip("\n") + "\n" + "\n".join(bench_table(sys.argv[2])))
    sys.exit(0)

import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from tests.util import shake_path, similarity
from vstab_amd import flow_pipeline as fp, host_math as hm, native, spatial_fill as sf, temporal_fill as tf

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
h, w, reps = 1080, 1920, 5
dev = torch.device("cuda", 0)
ctx = native.Context(0)
lines = ["# Spatial fill (push-pull): cost and quality", "",
         f"`python tools/spatial_fill_accuracy.py {n}` on one MI355X; HIP-event times, median of {reps} after one warm-up run.", ""]


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


def sfill_ms(dst0, mask0):
    """The fill works in place: every run gets a fresh copy of the warp's output."""
    ms, counts = [], None
    for _ in range(reps + 1):
        d = dst0.clone()
        counts = ctx.spatial_fill_batch(d, mask0)
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms("sfill"))
    block = sf.fill_meta(counts[0].cpu().numpy(), counts[1].cpu().numpy(), (dst0.shape[2], dst0.shape[1]))
    return float(np.median(ms[1:])), ms[1:], block


frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
plan = tf.plan_from_meta(res.meta)
ctx.set_timing(True)
rows = []

warp_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, plan["final_matrices"], plan["output_size"], border=(0.5, 0.5, 0.5),
                                                  want_mask=True, want_count=True))
mask0 = res.masks[..., 0].contiguous()
ms, runs, block = sfill_ms(res.frames, mask0)
rows.append(("C2 after the plain warp", res.meta["padding_fraction_mean"], warp_ms, ms, runs, block))

d8, m8 = res.frames.clone(), mask0.clone()
tblock = tf.fill_on_device(ctx, frames, d8, m8, plan["final_matrices"], plan["transitions"], plan["confidences"], 8)
ms, runs, block = sfill_ms(d8, m8)
rows.append(("C2 after the warp + temporal_fill=8", tblock["padding_fraction_mean_after"], warp_ms, ms, runs, block))

# a clip whose padded share is about 5 %: the same frames, shifted by 3 % of the width and 2 % of the height in alternating directions
shift = np.stack([similarity((1 if i % 2 else -1) * 0.03 * w, (1 if (i // 2) % 2 else -1) * 0.02 * h, 0.0, 1.0) for i in range(n)]).astype(np.float32)
warp5_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, shift, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
d5, m5, _ = ctx.warp_batch(frames, shift, (w, h), border=(0.5, 0.5, 0.5), want_mask=True, want_count=True)
ms, runs, block = sfill_ms(d5, m5)
rows.append(("about 5 % padded (shifted frames)", float((m5 > 0.5).float().mean().item()), warp5_ms, ms, runs, block))

# frames without any hole: the first pass alone
ms, runs, block = sfill_ms(frames, torch.zeros((n, h, w), device=dev))
rows.append(("no holes at all (first pass only)", 0.0, warp_ms, ms, runs, block))
ctx.set_timing(False)

lines += [f"## Kernel time, {n} x {h}p", "",
          "| clip | padded share (mean) | frames filled | plain warp ms | sfill ms | sfill / warp | sfill runs ms |", "|---|---|---|---|---|---|---|"]
for name, share, wms, ms, runs, block in rows:
    lines.append(f"| {name} | {share:.4f} | {block['frames_filled']} / {n} | {wms:.3f} | {ms:.3f} | {ms / wms:.2f} | "
                 f"{', '.join(f'{v:.3f}' for v in runs)} |")
del frames, res, d8, m8, d5, m5, mask0
torch.cuda.empty_cache()

# ---- quality: camera-locked shaken clip, the truth is the texture itself under the applied matrices -------------------------
qn, qh, qw = 24, 270, 480
lines += ["", f"## Quality, camera-locked shaken clip ({qn} x {qh} x {qw}, crop_and_pad)", "",
          "PSNR over the filled pixels against the analytic texture `T((F_i M_i)^-1 p)`, which exists under the padding too.", "",
          "| framing | filled px | push-pull dB | frame mean colour dB | black dB | padding colour dB |", "|---|---|---|---|---|---|"]
cam = shake_path(qn, qw, qh, "similarity", seed=3, amp=1.5)
clip = bench.synth_clip(qn, 0, qh, qw, dev, mats=cam)


def psnr(err2):
    return 10.0 * float(np.log10(1.0 / max(float(err2), 1e-20)))


for framing in ("crop_and_pad",):
    args = (framing, "similarity", True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)
    off = fp._stabilize_frames(hm._normalize_video_input(clip), *args, ctx=ctx, keep_on_device=True)
    on = fp._stabilize_frames(hm._normalize_video_input(clip), *args, ctx=ctx, keep_on_device=True, spatial_fill=True)
    final = np.array([e["applied_matrix"] for e in on.meta["stabilization_warp"]["per_frame"]], np.float64)
    truth = bench.synth_clip(qn, 0, qh, qw, dev, mats=final @ cam)   # (crop_and_pad: the output canvas is the source's)
    hole = on.masks[..., 0] > 0.5
    valid = ~hole
    mean = (off.frames * valid[..., None]).sum(dim=(1, 2)) / valid.sum(dim=(1, 2)).clamp(min=1)[:, None]
    def over_holes(img):
        return psnr(((img - truth) ** 2).mean(dim=-1)[hole].mean().item())
    lines.append(f"| {framing} | {int(hole.sum().item())} | {over_holes(on.frames):.2f} | "
                 f"{over_holes(mean[:, None, None, :].expand_as(truth)):.2f} | {over_holes(torch.zeros_like(truth)):.2f} | "
                 f"{over_holes(off.frames):.2f} |")

if len(sys.argv) > 2:
    lines += bench_table(sys.argv[2])

lines += ["", "The fill is per frame: invented borders may shimmer from frame to frame (no temporal coherence is attempted).", ""]
PROFILE.write_text("\n".join(lines))
print("\n".join(lines))
