#!/usr/bin/env python3
"""Rolling shutter round trip: how well the pair restores, and what the inverse costs.

  always     No GPU needed.  The coordinate image of tests/test_rolling_round_trip_cpu.py (160 x 90, readout 0.7) through the
             NumPy restatements: the rolling round trip, the plain round trip of the same matrices, the plain inverse of the
             rolling forward.
  on a GPU   (not with --cpu) the end-to-end clip of tests/test_rolling_round_trip_gpu.py (12 frames, 480 x 270, readout 0.7,
             translation mode) through the package: forward replay against Flow, PSNR of the restore with and without
             rolling=True (the figures the GPU test pins); the kernel time of rolling_unwarp_batch next to rolling_warp_batch
             and warp_batch of the same run on the C2 clip (256 x 1080p), HIP events, median of 7 after one warm-up.
  --parent D also alternates `bench.py --gpus 1 --steps 20 --warmup 5` between this tree and a built checkout of the parent
             commit at D (child processes, 3 rounds, one box).

    python tools/rolling_round_trip_report.py [--cpu] [--parent DIR] [--out profiles/rNN_rolling_round_trip.md]

Writes the next free profiles/rNN_rolling_round_trip.md unless --out names a file.
"""
import argparse
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import __graft_entry__ as graft  # noqa: E402
from tests import rolling_shutter_restatement as R  # noqa: E402
from tests import test_rolling_round_trip_cpu as TC  # noqa: E402
from tests import test_rolling_round_trip_gpu as T  # noqa: E402


def cpu_round_trip(lines):
    from vstab_amd import rolling_shutter as rs

    skew = float(rs.corner_skew(TC.VELOCITY[None], TC.RHO, (TC.W, TC.H)).max())
    err, interior = TC.round_trip_errors(TC.coordinate_round_trip())
    lines.append(f"Coordinate image {TC.W} x {TC.H}, similarity 1.03 / 0.02 rad, readout {TC.RHO}, velocity {TC.VELOCITY.tolist()}: corner "
                 f"skew {skew:.3f} px.  Max |restored - original| over the pixels all three passes show, {TC.ERODE} px inside "
                 f"({interior:.2f} of the frame):\n")
    lines.append("| pass | max error (px) |")
    lines.append("|---|---|")
    for name, label in (("rolling", "rolling forward, rolling inverse"), ("plain", "plain forward, plain inverse (zero velocity)"),
                        ("plain_inverse", "rolling forward, plain inverse")):
        lines.append(f"| {label} | {err[name]:.4f} |")
    lines.append("")
    print(json.dumps({"coordinate_round_trip": {k: round(v, 4) for k, v in err.items()}, "corner_skew": round(skew, 3)}), flush=True)


def gpu_end_to_end(lines):
    """The clip of tests/test_rolling_round_trip_gpu.py through the package: what its assertions are pinned to."""
    import torch

    from vstab_amd import native

    ctx = native.default_context()
    e = T.E2E
    path = R.CameraPath(e["w"], e["h"], amp=e["amp"], omega=e["omega"], seed=e["seed"])
    frames = R.rolling_clip(path, e["n"], e["rho"], torch.device("cuda", 0))
    run = T._stabilize(ctx, frames, "crop_and_pad", rolling_shutter=e["rho"])
    meta = json.loads(json.dumps(run.meta))
    replay = T._apply(ctx, frames, meta, rolling=True)
    same = T._same(replay.frames, run.frames) and T._same(replay.masks, run.masks)
    back_meta = T._inverse_meta(meta)
    rolling, plain = T._apply(ctx, run.frames, back_meta, rolling=True), T._apply(ctx, run.frames, back_meta)
    sel = T._interior(torch.maximum(rolling.masks[..., 0], plain.masks[..., 0]), 4)
    p_rolling, p_plain = T._psnr(rolling.frames, frames, sel), T._psnr(plain.frames, frames, sel)
    info = rolling.meta["motion_apply"]["rolling_shutter"]
    lines.append(f"Clip: {e['n']} frames {e['w']} x {e['h']}, readout {e['rho']}, translation mode, camera lock, crop_and_pad; "
                 f"meta skew_px_max {meta['rolling_shutter']['skew_px_max']:.2f} px.\n")
    lines.append(f"Forward replay on the source frames (rolling=True) equals Flow's frames and mask in bits: {same}.\n")
    lines.append("| restore of the stabilized frames | PSNR against the source frames (dB) |")
    lines.append("|---|---|")
    lines.append(f"| rolling=True | {p_rolling:.2f} |")
    lines.append(f"| rolling=False | {p_plain:.2f} |")
    lines.append(f"\nOver the pixels both restores show, 4 px inside ({float(sel.float().mean()):.2f} of the frame); unsolved_max {info['unsolved_max']}.\n")
    print(json.dumps({"forward_replay_bits": same, "psnr_rolling": round(p_rolling, 2), "psnr_plain": round(p_plain, 2),
                      "unsolved_max": info["unsolved_max"]}), flush=True)


def gpu_cost(lines, n=256, reps=7):
    import torch

    import bench
    from vstab_amd import native

    ctx = native.default_context()
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, torch.device("cuda", 0))
    final = np.tile(np.array([[1, 0, 3.25], [0, 1, -2.5], [0, 0, 1]], np.float32), (n, 1, 1))
    velocity = np.tile([0.002, -0.003, 6.0, 0.003, 0.002, -4.0], (n, 1))
    ctx.set_timing(True)
    kinds = {"warp": [], "rolling_warp": [], "rolling_unwarp": []}
    for _ in range(reps + 1):   # the first of each is the warm-up
        ctx.warp_batch(frames, final, (w, h), want_mask=True, want_count=True)
        kinds["warp"].append(ctx.last_kernel_ms("warp"))
        ctx.rolling_warp_batch(frames, final, (w, h), velocity, 0.7, want_mask=True, want_count=True)
        kinds["rolling_warp"].append(ctx.last_kernel_ms("rolling_warp"))
        ctx.rolling_unwarp_batch(frames, final, (w, h), velocity, 0.7, want_mask=True, want_count=True, want_unsolved=True)
        kinds["rolling_unwarp"].append(ctx.last_kernel_ms("rolling_unwarp"))
    ctx.set_timing(False)
    out = {"frames": n, "size": [w, h], "launches": reps, "ms": {}}
    lines.append(f"C2 clip: {n} frames {w} x {h}; HIP events, median of {reps} launches after one warm-up.\n")
    lines.append("| kind | median (ms) | all launches (ms) |")
    lines.append("|---|---|---|")
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
        lines.append(f"| {k} | {out['ms'][k]['median']:.4f} | {', '.join(f'{x:.4f}' for x in v)} |")
    ratio = {k: round(out["ms"][k]["median"] / out["ms"]["warp"]["median"], 3) for k in ("rolling_warp", "rolling_unwarp")}
    out["over_warp"] = ratio
    lines.append(f"\nrolling_warp / warp = {ratio['rolling_warp']:.3f}, rolling_unwarp / warp = {ratio['rolling_unwarp']:.3f}; at 28 B per "
                 f"output pixel the inverse moves {n * w * h * 28 / (out['ms']['rolling_unwarp']['median'] * 1e-3) / 1e12:.2f} TB/s.\n")
    print(json.dumps(out), flush=True)


def bench_alternation(lines, parent: Path, rounds=3):
    """`bench.py --gpus 1 --steps 20 --warmup 5` in child processes, this tree and the parent's checkout in turn."""
    def one(tree: Path) -> float:
        proc = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=str(tree),
                              capture_output=True, text=True, timeout=600)
        if proc.returncode != 0:
            raise RuntimeError(f"bench.py failed in {tree}: {proc.stderr[-2000:]}")
        line = [json.loads(t) for t in proc.stdout.splitlines() if t.startswith("{")][-1]
        return float(line["value"])

    rows = []
    for r in range(rounds):
        rows.append((one(ROOT), one(parent)))
        print(json.dumps({"bench_round": r + 1, "this_tree_fps": rows[-1][0], "parent_fps": rows[-1][1]}), flush=True)
    lines.append("| round | this tree (frames/s) | parent (frames/s) |")
    lines.append("|---|---|---|")
    for r, (a, b) in enumerate(rows):
        lines.append(f"| {r + 1} | {a:.2f} | {b:.2f} |")
    mine, theirs = [a for a, _ in rows], [b for _, b in rows]
    lines.append(f"\nThis tree: median {np.median(mine):.2f} ({min(mine):.2f} .. {max(mine):.2f}); parent: median {np.median(theirs):.2f} "
                 f"({min(theirs):.2f} .. {max(theirs):.2f}).  The default path calls nothing new.\n")


def next_profile() -> Path:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    return ROOT / "profiles" / f"r{max(taken, default=0) + 1:02d}_rolling_round_trip.md"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="only the figures that need no GPU")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the bench.py alternation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    graft.load_package()
    import torch

    gpu = torch.cuda.is_available() and not args.cpu
    bench_lines = []
    if gpu and args.parent:   # first, while this process holds nothing on the device
        bench_alternation(bench_lines, Path(args.parent).resolve())
    lines = ["# Rolling shutter round trip: how well the pair restores, what the inverse costs", "",
             "Written by tools/rolling_round_trip_report.py" + (" --cpu" if args.cpu else "") + ".", ""]
    lines += ["## Round trip of a coordinate image (NumPy restatements)", ""]
    cpu_round_trip(lines)
    if gpu:
        lines += ["## End to end, on the MI355X (the package itself)", "",
                  "What tests/test_rolling_round_trip_gpu.py pins: half of the measured gain.", ""]
        gpu_end_to_end(lines)
        lines += ["## Kernel times (MI355X)", ""]
        gpu_cost(lines)
    else:
        lines += ["## End to end and kernel times", "", "NOT MEASURED: this run had no GPU.", ""]
    lines += ["## The default path (`bench.py --gpus 1 --steps 20 --warmup 5`, alternating with a checkout of the parent commit, one box)", ""]
    if bench_lines:
        lines += bench_lines
    else:
        lines += ["NOT MEASURED: " + ("no --parent checkout was given." if gpu else "this run had no GPU."), ""]
    out = Path(args.out) if args.out else next_profile()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
