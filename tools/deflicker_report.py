"""What the deflicker costs and how well it measures; writes profiles/r27_deflicker.md.

  1. kernel times (HIP events, timing kinds "gain_hist", "gain_sums", "apply_gain", median of 7 after one warm-up) on the
     bench's C2 clip under a synthetic per-frame flicker, with the transitions of a default Flow run of that clip, next to
     the plain warp's kernel time OF THE SAME RUN; bytes per lattice sample / per pixel and the achieved rate;
  2. the accuracy figures of tests/test_deflicker_gpu.py's synthetic flicker clip: the restatement's own error with the true
     transitions (CPU), the pipeline's with estimated ones, the plain ratio of sums, the RMS step and the ITF;
  3. with a directory as second argument: the `value` (frames/s) of the bench.py lines found there as bench_parent_<k>.log and
     bench_pr_<k>.log -- `bench.py --gpus 1 --steps 5 --warmup 2` run alternately in a checkout of the parent commit and in
     this tree -- as a table with the parent's own spread.  Without it the section says NOT MEASURED.
  4. with a library as third argument -- the same sources built with -DVSTAB_DEFLICKER_NT_STORES -- the apply pass with
     non-temporal stores, measured by a child process that loads that library (VSTAB_LIB) and runs the same steps.

python tools/deflicker_report.py [frames] [directory of bench logs | -] [variant library]"""
import json
import os
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
from tests import deflicker_restatement as R
from vstab_amd import deflicker as D, flow_pipeline as fp, host_math as hm, native, temporal_fill as tf

PROFILE = ROOT / "profiles" / "r27_deflicker.md"
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
logs = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
variant = sys.argv[3] if len(sys.argv) > 3 else None
APPLY_ONLY = os.environ.get("DEFLICKER_REPORT_APPLY_ONLY") == "1"      # the child of section 4
h, w, reps = 1080, 1920, 7
dev = torch.device("cuda", 0)
ctx = native.Context(0)
lines = ["# Deflicker: cost and accuracy", "",
         f"`python tools/deflicker_report.py {n}` on one MI355X; HIP-event times, median of {reps} after one warm-up run.", ""]


def timed(kind, call):
    ms = []
    for _ in range(reps + 1):
        call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    return float(np.median(ms[1:])), ms[1:]


# ---- 1. cost --------------------------------------------------------------------------------------------------------------
frames = bench.synth_clip(n, 0, h, w, dev)
rng = np.random.default_rng(27)
flicker = np.exp(rng.normal(0.0, 0.08, n)).astype(np.float32)
frames *= torch.from_numpy(flicker).to(dev)[:, None, None, None]
res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
plan = tf.plan_from_meta(res.meta)
out, mask = res.frames, res.masks[..., 0].contiguous()
mats = plan["transitions"]
pairs, px = n - 1, h * w
lattice = len(R.lattice(h, w)[0])
ctx.set_timing(True)
warp_ms, _ = timed("warp", lambda: ctx.warp_batch(frames, plan["final_matrices"], plan["output_size"], border=(0.5, 0.5, 0.5),
                                                  want_mask=True, want_count=True))
hist_ms, hist_runs = timed("gain_hist", lambda: ctx.pair_gain_hist_batch(frames, mats))
hist, stats = (t.cpu().numpy() for t in ctx.pair_gain_hist_batch(frames, mats))
band, _ = D.bands_from_hist(hist)
sums_ms, sums_runs = timed("gain_sums", lambda: ctx.pair_gain_sums_batch(frames, mats, band))
gain, ok = D.gains_from_sums(ctx.pair_gain_sums_batch(frames, mats, band).cpu().numpy())
true = (flicker[1:] / flicker[:-1]).astype(np.float64)
c2_err = float(np.abs(gain[:, 3] / true - 1).max())
corr = np.exp(rng.normal(0.0, 0.05, (n, 3))).astype(np.float32)      # every frame takes part, none clamps the whole frame
work = out.clone()
apply_ms, apply_runs = timed("apply_gain", lambda: ctx.apply_gain_batch(work, corr, mask))
bare_ms, bare_runs = timed("apply_gain", lambda: ctx.apply_gain_batch(work, corr, None))
ctx.set_timing(False)
if APPLY_ONLY:
    print(json.dumps({"masked": [apply_ms, apply_runs], "bare": [bare_ms, bare_runs]}))
    sys.exit(0)
own = float((mask != 1.0).float().mean())
del work, out, mask, res
torch.cuda.empty_cache()

sample_b = 24                       # 12 B of frame a and 12 B of frame b per lattice sample
lines += [f"## Kernel time, {n} frames of {h}p ({pairs} pairs, {lattice} lattice samples per pair; plain warp of the same run: {warp_ms:.3f} ms)", "",
          "| kernel | unit | B per unit | ms | / plain warp | G units/s | TB/s against the algorithmic bytes | runs ms |", "|---|---|---|---|---|---|---|---|"]
for name, unit, per, count, ms, runs in (
        ("pair_gain_hist", "lattice sample", sample_b, pairs * lattice, hist_ms, hist_runs),
        ("pair_gain_sums", "lattice sample", sample_b, pairs * lattice, sums_ms, sums_runs),
        (f"apply_gain under the padding mask ({100 * own:.1f} % own pixels)", "pixel", 28, n * px, apply_ms, apply_runs),
        ("apply_gain, mask NULL", "pixel", 24, n * px, bare_ms, bare_runs)):
    lines.append(f"| {name} | {unit} | {per} | {ms:.3f} | {ms / warp_ms:.2f} | {count / (ms * 1e-3) / 1e9:.2f} | "
                 f"{count * per / (ms * 1e-3) / 1e12:.3f} | {', '.join(f'{v:.3f}' for v in runs)} |")
nt = None
if variant:
    child = subprocess.run([sys.executable, __file__, str(n)], env=dict(os.environ, VSTAB_LIB=variant, DEFLICKER_REPORT_APPLY_ONLY="1"),
                           capture_output=True, text=True, timeout=600)
    rows = [ln for ln in child.stdout.splitlines() if ln.startswith("{")]
    if child.returncode == 0 and rows:
        nt = json.loads(rows[-1])
        for key, name, per in (("masked", "apply_gain under the padding mask, non-temporal stores", 28),
                               ("bare", "apply_gain, mask NULL, non-temporal stores", 24)):
            ms, runs = nt[key]
            lines.append(f"| {name} | pixel | {per} | {ms:.3f} | {ms / warp_ms:.2f} | {n * px / (ms * 1e-3) / 1e9:.2f} | "
                         f"{n * px * per / (ms * 1e-3) / 1e12:.3f} | {', '.join(f'{v:.3f}' for v in runs)} |")
stores = ("Non-temporal stores: NOT MEASURED -- the passes behind it read the frames again at once, which is what the ordinary stores "
          "were chosen for." if nt is None else
          f"With non-temporal stores (a second build of the library, the same steps in a child process) it takes {nt['masked'][0]:.3f} ms "
          f"against {apply_ms:.3f} ms under the mask and {nt['bare'][0]:.3f} ms against {bare_ms:.3f} ms without; the shipped kernel "
          "uses ordinary stores.")
rows_tb = pairs * 2 * len(range(R.STRIDE // 2, h, R.STRIDE)) * w * 12 / 1e12      # every touched row in full, both frames of a pair
lines += ["", f"The two measuring kernels gather 12 B at a 48-B pitch, which leaves no 64-B sector of a lattice row untouched: what crosses "
              f"the memory system is every fourth row in full, {rows_tb * 1e3:.2f} GB per launch if both frames of every pair come from HBM "
              f"(half of that if frame b of a pair is still cached as frame a of the next), against {pairs * lattice * sample_b / 1e9:.2f} GB of "
              f"used bytes.  That is {rows_tb / (hist_ms * 1e-3):.2f} TB/s (hist) and {rows_tb / (sums_ms * 1e-3):.2f} TB/s (sums) counting both "
              "frames, the rate of a streaming pass: what bounds them is the memory traffic of rows of which a quarter of the bytes is "
              "used, not the fp64 mapping, the four LDS atomics per sample or the flush of the non-zero bins (the sums pass has neither "
              f"of the latter two and is {100.0 * (1.0 - sums_ms / hist_ms):.0f} % faster).  The apply pass is an in-place stream (read 12 B + 4 B of mask, write 12 B per "
              "pixel): it is bound by HBM bandwidth.  " + stores,
          f"On this clip (flicker sigma 8 %, no subject) every pair is measured: {bool(ok[:, 3].all())}; worst relative error of a pair "
          f"gain against the true ratio: {c2_err:.5f}; well-exposed share of the inside samples: {float((stats[:, 1] / np.maximum(stats[:, 0], 1)).mean()):.3f}.", ""]

# ---- 2. accuracy on the tests' clip ---------------------------------------------------------------------------------------
clip, gains, shifts, _ = R.flicker_clip()
true = gains[1:] / gains[:-1]
ref_gain, _, ref_inlier = R.measure(clip, R.true_transitions(shifts))
ref_plain, _, _ = R.measure(clip, R.true_transitions(shifts), band_override=[0, 1023])
small = torch.from_numpy(clip).to(dev)
args = ("crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
runs = {}
for name, kw in (("off", {}), ("window 1 s", dict(deflicker=True)), ("window 60 s", dict(deflicker=60))):
    runs[name] = fp._stabilize_frames(hm._normalize_video_input(small), *args, ctx=ctx, keep_on_device=True, stability_report=True, **kw)
block = runs["window 60 s"].meta["deflicker"]
got = np.asarray(block["pair_gain"], np.float64)
est = np.array([t["matrix"] for t in runs["off"].meta["estimated_motion"]["per_transition"]], np.float32)
plain = D.gains_from_sums(ctx.pair_gain_sums_batch(small, est, np.tile(np.array([0, 1023], np.int32), (len(est), 4, 1))).cpu().numpy())[0][:, 3]
rel = lambda g: float(np.abs(np.asarray(g) / true[:, :1].reshape(-1, *([1] * (np.ndim(g) - 1))) - 1).max())
lines += [f"## Accuracy, the synthetic flicker clip ({R.CLIP_N} frames of {R.CLIP_W} x {R.CLIP_H}, gains sigma 12 %, a subject of new content on "
          "at most 30 % of the frame, a clipped patch)", "",
          "| estimate | transitions | worst relative error of a pair gain |", "|---|---|---|",
          f"| restatement, median + band (CPU) | true | {rel(ref_gain):.5f} |",
          f"| restatement, plain ratio of sums (CPU) | true | {rel(ref_plain):.5f} |",
          f"| pipeline, deflicker=60 (HIP) | estimated | {rel(got):.5f} |",
          f"| plain ratio of sums, band [0, 1023] (HIP) | estimated | {rel(plain):.5f} |", "",
          f"The GPU test's bound is twice the first row ({2 * rel(ref_gain):.5f}), taken from the CPU run.  Inlier share of the "
          f"restatement: at least {float(ref_inlier.min()):.3f}; of the pipeline: at least {block['inlier_fraction_min']:.3f}.", "",
          "| run | step_rms_before | step_rms_after | after.itf_db | values_clamped |", "|---|---|---|---|---|"]
for name, run in runs.items():
    b = run.meta.get("deflicker")
    itf = run.meta["stability"]["after"]["itf_db"]
    lines.append(f"| {name} | {'' if b is None else format(b['step_rms_before'], '.4f')} | {'' if b is None else format(b['step_rms_after'], '.4f')} | "
                 f"{itf:.3f} | {'' if b is None else b['values_clamped']} |")
lines.append("")

# ---- 3. the default path ----------------------------------------------------------------------------------------------------
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
                  "path calls nothing new.", ""]
else:
    lines += ["NOT MEASURED in this run (no directory of bench logs was given).", ""]
PROFILE.write_text("\n".join(lines))
print("\n".join(lines))
