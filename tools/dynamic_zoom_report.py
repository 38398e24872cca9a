"""What the dynamic zoom costs and what it keeps on the bench's C2 clip; writes the next free profiles/rNN_dynamic_zoom.md.

  1. kernel time (HIP events, timing kind "cover_extent") of vstab_cover_extent_batch on the clip's final matrices, plain
     and with the 17 x 10 mesh of a mesh_warp=True run, next to the plain warp and the mesh warp of the same run: a ratio
     to the warp each guards, and the time per pixel against the kernel's fp64 instruction count;
  2. field of view kept: the mean of 1 / zoom against 1 / static_zoom, and against `crop` framing's crop_size on the clip;
  3. the default path: bench.py result lines of this tree and of the parent commit, alternated on one box by the caller
     (--bench THIS.jsonl PARENT.jsonl, one JSON line per run); without the files that section says NOT MEASURED.  The tool
     only formats the two files -- it cannot tell which tree a line came from -- so they are made exactly like this, from
     the root of this tree, in one shell on one box:

       git worktree add ../vstab_parent HEAD~1
       (cd ../vstab_parent && python -c "import __graft_entry__ as g; g.build()")
       B="--gpus 1 --steps 5 --warmup 2 --cpu-frames 0 --cv2-frames 0 --no-extras --no-checks"
       for round in 1 2 3; do
         python bench.py $B | grep '^{' >> this.jsonl
         (cd ../vstab_parent && python bench.py $B | grep '^{') >> parent.jsonl
       done
       python tools/dynamic_zoom_report.py 256 --bench this.jsonl parent.jsonl

     (HEAD~1: the commit this feature was added on top of; the flags leave out the CPU baselines, extras and accuracy checks,
     which do not enter the timed value.)

python tools/dynamic_zoom_report.py [frames] [--bench THIS.jsonl PARENT.jsonl]"""
import json
import re
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from vstab_amd import dynamic_zoom as dz, flow_pipeline as fp, host_math as hm, native, temporal_fill as tf

argv = sys.argv[1:]
bench_files = None
if "--bench" in argv:
    k = argv.index("--bench")
    bench_files = (Path(argv[k + 1]), Path(argv[k + 2]))
    del argv[k:k + 3]
n = int(argv[0]) if argv else 256
h, w, reps = 1080, 1920, 7
taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
PROFILE = ROOT / "profiles" / f"r{max(taken, default=0) + 1:02d}_dynamic_zoom.md"
dev = torch.device("cuda", 0)
ctx = native.Context(0)
cmd = f"python tools/dynamic_zoom_report.py {n}" + (" --bench THIS.jsonl PARENT.jsonl" if bench_files else "")
lines = ["# Dynamic zoom: cost of the coverage extent, field of view kept, default path", "",
         f"`{cmd}` on one MI355X; HIP-event times, median of {reps} after one warm-up run.", ""]


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


def stabilize(framing="crop_and_pad", **kw):
    args = (framing,) + tuple(bench.FLOW_ARGS[1:])
    return fp._stabilize_frames(hm._normalize_video_input(frames), *args, ctx=ctx, keep_on_device=True, **kw)


frames = bench.synth_clip(n, 0, h, w, dev)
size = (w, h)
res = stabilize()
final = np.asarray(tf.plan_from_meta(res.meta)["final_matrices"], np.float32)
mesh_run = stabilize(mesh_warp=True, mesh_motion=True)
mesh_final = np.asarray(tf.plan_from_meta(mesh_run.meta)["final_matrices"], np.float32)
offsets = torch.from_numpy(np.asarray(mesh_run.meta["mesh_warp"]["motion"]["offsets"], np.float32)).to(dev)
del res, mesh_run
torch.cuda.empty_cache()

# ---- 1. kernel time ----
ctx.set_timing(True)
warp_ms, warp_runs = timed("warp", lambda: ctx.warp_batch(frames, final, size, border=(0.5, 0.5, 0.5), want_mask=True, want_count=True))
mwarp_ms, mwarp_runs = timed("mesh_warp", lambda: ctx.mesh_warp_batch(frames, mesh_final, size, offsets, border=(0.5, 0.5, 0.5),
                                                                      want_mask=True, want_count=True))
rows = []
for name, guard_ms, call in (
        ("plain, q5", warp_ms, lambda: ctx.cover_extent_batch(final, size, size)),
        ("plain, exact", warp_ms, lambda: ctx.cover_extent_batch(final, size, size, subpix="exact")),
        ("17 x 10 mesh, q5", mwarp_ms, lambda: ctx.cover_extent_batch(mesh_final, size, size, offsets)),
        ("17 x 10 mesh, exact", mwarp_ms, lambda: ctx.cover_extent_batch(mesh_final, size, size, offsets, subpix="exact"))):
    ms, runs = timed("cover_extent", call)
    rows.append((name, guard_ms, ms, runs))
ctx.set_timing(False)
px = n * h * w
lines += [f"## Kernel time, {n} frames of {h}p ({px / 1e6:.0f} Mpixel)", "",
          f"Plain warp of the same run: {warp_ms:.3f} ms ({', '.join(f'{v:.3f}' for v in warp_runs)}); mesh warp: {mwarp_ms:.3f} ms "
          f"({', '.join(f'{v:.3f}' for v in mwarp_runs)}).  The extent times include the preset kernel in front and the "
          "host-side staging of the matrices, as the warp's do.", "",
          "| vstab_cover_extent_batch | ms | / the warp it guards | ps per pixel | Gpixel/s | runs ms |", "|---|---|---|---|---|---|"]
for name, guard_ms, ms, runs in rows:
    lines.append(f"| {name} | {ms:.3f} | {ms / guard_ms:.2f} | {ms * 1e9 / px:.1f} | {px / (ms * 1e-3) / 1e9:.1f} | "
                 f"{', '.join(f'{v:.3f}' for v in runs)} |")
lines += ["", "No image memory is read or written, so HBM does not bound the pass; what it executes per pixel is the warp's fp64 "
              "coordinate arithmetic (and under a mesh the LDS vertex lookups and the fp64 bilinear blend).", ""]

# ---- 2. field of view ----
lines += [f"## Field of view kept, {n} x {h}p (bench.FLOW_ARGS)", "",
          "| run | zoom_mean | zoom_max | static_zoom | mean of 1 / zoom | 1 / static_zoom | frames_capped | frames_with_padding | padding_fraction_max |",
          "|---|---|---|---|---|---|---|---|---|"]
for name, kw in (("dynamic_zoom=True (2 s, limit 2)", dict(dynamic_zoom=True)), ("dynamic_zoom=0.5", dict(dynamic_zoom=0.5)),
                 ("dynamic_zoom=True, mesh_warp=True", dict(dynamic_zoom=True, mesh_warp=True))):
    run = stabilize(**kw)
    b = run.meta["dynamic_zoom"]
    lines.append(f"| {name} | {b['zoom_mean']:.4f} | {b['zoom_max']:.4f} | {b['static_zoom']:.4f} | {float(np.mean(1.0 / np.asarray(b['zoom']))):.4f} | "
                 f"{1.0 / b['static_zoom']:.4f} | {b['frames_capped']} | {b['frames_with_padding']} | {run.meta['padding_fraction_max']:.6f} |")
    del run
    torch.cuda.empty_cache()
crop = stabilize("crop")
fr = crop.meta["framing"]
cw, ch = fr.get("crop_size", size)
lines += ["", f"`crop` framing on the same clip: crop_size {int(cw)} x {int(ch)} of {w} x {h} = {cw / w:.4f} x {ch / h:.4f} of the frame per axis "
              f"(keep_fov_effective {fr.get('keep_fov_effective')}, status {fr.get('keep_fov_status')}).", ""]
del crop

# ---- 3. the default path ----
lines += ["## Default path (bench.py, this tree alternating with the parent commit on one box)", ""]
if bench_files is None:
    lines += ["NOT MEASURED in this run (no --bench files given).", ""]
else:
    for name, path in zip(("this tree", "parent commit"), bench_files):
        vals = [json.loads(l)["value"] for l in path.read_text().splitlines() if l.startswith("{") and '"value"' in l]
        lines.append(f"- {name}: {', '.join(f'{v:.2f}' for v in vals)} frames/s" + (f" (median {float(np.median(vals)):.2f})" if vals else ""))
    lines += ["", "The default path launches nothing new (`dynamic_zoom=None` returns before any of it)."]
PROFILE.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
print(f"wrote {PROFILE}")
