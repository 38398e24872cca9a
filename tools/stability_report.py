"""What the stability report costs and what it says on the bench's C2 clip; writes profiles/r14_stability.md.

  1. kernel time (HIP events, timing kind "stability") of the consecutive form on the outputs of a default Flow run with
     their padding mask (32 B per pixel and pair) and on the source frames without a mask (24 B), next to the plain warp's
     kernel time of the same run, and the achieved bytes per second against those algorithmic byte counts;
  2. the same masked call with `b` in a separate copy of the clip, so that no frame is read twice: whether the consecutive
     form's second read of a frame is served by a cache shows as the difference;
  3. before / after / gain for default Flow, mesh_warp=True, temporal_fill=8 and spatial_fill=True.

python tools/stability_report.py [frames]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from vstab_amd import flow_pipeline as fp, host_math as hm, native, temporal_fill as tf

PROFILE = ROOT / "profiles" / "r14_stability.md"
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
h, w, reps = 1080, 1920, 7
dev = torch.device("cuda", 0)
ctx = native.Context(0)
lines = ["# Stability report (ITF): cost and figures", "",
         f"`python tools/stability_report.py {n}` on one MI355X; HIP-event times, median of {reps} after one warm-up run.", ""]


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
plan = tf.plan_from_meta(res.meta)
out, mask = res.frames, res.masks[..., 0].contiguous()
assert tuple(out.shape) == tuple(frames.shape)
ctx.set_timing(True)
warp_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, plan["final_matrices"], plan["output_size"], border=(0.5, 0.5, 0.5),
                                                  want_mask=True, want_count=True))
pairs, px = n - 1, h * w
rows = []
ms, runs = timed("stability", lambda: ctx.frame_sse_batch(out[:-1], out[1:], mask[:-1], mask[1:]))
rows.append(("consecutive form, outputs + padding mask", 32, ms, runs))
copy_f, copy_m = out.clone(), mask.clone()
ms, runs = timed("stability", lambda: ctx.frame_sse_batch(out[:-1], copy_f[1:], mask[:-1], copy_m[1:]))
rows.append(("the same with `b` and `mask_b` in a separate copy (no frame read twice)", 32, ms, runs))
same = [t.cpu().numpy() for t in ctx.frame_sse_batch(out[:-1], out[1:], mask[:-1], mask[1:])]
other = [t.cpu().numpy() for t in ctx.frame_sse_batch(out[:-1], copy_f[1:], mask[:-1], copy_m[1:])]
assert np.array_equal(same[0], other[0]) and np.array_equal(same[1], other[1])
del copy_m
ms, runs = timed("stability", lambda: ctx.frame_sse_batch(frames[:-1], frames[1:]))
rows.append(("consecutive form, source frames, no mask", 24, ms, runs))
ms, runs = timed("stability", lambda: ctx.frame_sse_batch(frames[:-1], copy_f[1:]))
rows.append(("source frames against a separate clip, no mask (no frame read twice)", 24, ms, runs))
ctx.set_timing(False)
del copy_f, out, mask, res
torch.cuda.empty_cache()

lines += [f"## Kernel time, {pairs} pairs of {h}p (plain warp of the same run: {warp_ms:.3f} ms)", "",
          "| call | B per pixel and pair | ms | / plain warp | TB/s against the algorithmic bytes | runs ms |", "|---|---|---|---|---|---|"]
for name, per_px, ms, runs in rows:
    tbs = pairs * px * per_px / (ms * 1e-3) / 1e12
    lines.append(f"| {name} | {per_px} | {ms:.3f} | {ms / warp_ms:.2f} | {tbs:.2f} | {', '.join(f'{v:.3f}' for v in runs)} |")
ratio32, ratio24 = rows[0][2] / rows[1][2], rows[2][2] / rows[3][2]
lines += ["", f"Consecutive form over separate copies: {ratio32:.2f} x the time with masks, {ratio24:.2f} x without.  The algorithmic byte "
              "count takes every frame as read twice; a ratio below 1 is what the caches serve of the second read.", ""]

lines += [f"## Figures, {n} x {h}p (bench.FLOW_ARGS)", "",
          "| configuration | before ITF dB | after ITF dB | gain dB | after min dB | after overlap (mean) | pairs without overlap |",
          "|---|---|---|---|---|---|---|"]
for name, kw in (("default Flow", {}), ("mesh_warp=True", dict(mesh_warp=True)), ("temporal_fill=8", dict(temporal_fill=8)),
                 ("spatial_fill=True", dict(spatial_fill=True))):
    run = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True,
                               stability_report=True, **kw)
    b = run.meta["stability"]
    fmt = lambda v: "none" if v is None else f"{v:.3f}"
    lines.append(f"| {name} | {fmt(b['before']['itf_db'])} | {fmt(b['after']['itf_db'])} | {fmt(b['gain_db'])} | "
                 f"{fmt(b['after']['psnr_db_min'])} | {b['after']['overlap_fraction_mean']:.4f} | {b['after']['pairs_without_overlap']} |")
    del run
    torch.cuda.empty_cache()
lines += ["", "Spatial fill leaves the mask as it is: its invented pixels are outside the measure, so its row equals the default's.", ""]
PROFILE.write_text("\n".join(lines))
print("\n".join(lines))
