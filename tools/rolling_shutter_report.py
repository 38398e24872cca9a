#!/usr/bin/env python3
"""Rolling shutter: what the correction recovers, how well the readout is found, and what the two kernels cost.

  always     No GPU needed.  The end-to-end clip of tests/test_rolling_shutter_gpu.py (12 frames, 480 x 270, readout 0.7)
             through the oracle's estimation chain (gray, DIS, fits), the package's host plan and the NumPy restatement of the warp: PSNR
             against the static texture without the keyword, with it, and of the global-shutter twin's run; the share of the
             gap that is recovered; the readout "auto" finds.  These are the figures the GPU test's assertions are derived from.
             Then the accuracy table: analytic rolling flows at 960 x 540 (and the other sizes of tests/test_rolling_shutter_cpu.py),
             least-squares fits, the readout estimate against the truth.
  on a GPU   (not with --cpu) the same clip through the package itself, and the kernel time of rolling_warp_batch next to
             warp_batch of the same run on the C2 clip (256 x 1080p), HIP events, median of 7 after one warm-up;
             row_residual_batch on the clip's own grid.

    python tools/rolling_shutter_report.py [--cpu] [--out profiles/rNN_rolling_shutter.md]

Writes the next free profiles/rNN_rolling_shutter.md unless --out names a file.
"""
import argparse
import itertools
import json
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import __graft_entry__ as graft  # noqa: E402
from tests import rolling_shutter_restatement as R  # noqa: E402
from tests import test_rolling_shutter_cpu as TC  # noqa: E402
from tests import test_rolling_shutter_gpu as T  # noqa: E402


def cpu_run(oracle, fp, hm, rs, frames, mode, rolling):
    """_stabilize_frames(camera_lock, strength 1, crop_and_pad, rolling_shutter=rolling) without a GPU: the oracle's estimation
    chain, the package's host plan, the restatement's warp -> (frames, mask, final matrices, meta["rolling_shutter"] | None)."""
    from tests.test_e2e_golden_cpu import OraclePlanCtx

    n, h, w, _ = frames.shape
    work = hm._working_estimation_size(w, h) or (w, h)
    gray = oracle.gray_for_estimation(frames, hm._working_estimation_size(w, h))
    flow = oracle.dis_flow_clip(gray)
    records = [oracle.fit_all_modes(flow[i], 8, mode)[0] for i in range(n - 1)]
    lock, strength, smooth, keep_fov, rgb, fps = T.LOCK_ARGS
    plan = fp.plan_stabilization(OraclePlanCtx(oracle), records, (w, h), n, "crop_and_pad", mode, lock, strength, smooth, keep_fov,
                                 rgb, fps, fps, estimator="flow")
    em = plan.estimated_motion
    final = np.asarray(plan.final_matrices, np.float32)
    border = hm.border_value(rgb)
    if rolling is None:
        out, mask, _ = R.rolling_warp(frames, final, plan.output_size, np.zeros((n, 6)), 0.0, border)
        return out, mask, final, None
    velocity = rs.velocities(em["matrices"], em["confidences"], None)
    estimate = None
    readout, source = rolling, "given"
    if rolling == "auto":
        grid = np.ascontiguousarray(np.asarray(flow)[:, ::8, ::8], np.float32)
        residual, count = R.row_residual(grid, 8, work, em["work_matrices"])
        estimate = rs.estimate_readout(residual, count, em["work_matrices"], em["confidences"], em["modes"], None, work, 8)
        readout, source = estimate["readout"], estimate["source"]
    out, mask, _ = R.rolling_warp(frames, final, plan.output_size, velocity, readout, border)
    return out, mask, final, rs.meta_block(readout, source, estimate, velocity, (w, h))


def cpu_end_to_end(lines):
    import torch

    from oracle import oracle
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import rolling_shutter as rs

    oracle.build()
    e = T.E2E
    dev = torch.device("cpu")
    path = T.e2e_path()
    skew = [path.corner_skew(i, e["rho"]) for i in range(e["n"])]
    lines.append(f"Clip: {e['n']} frames {e['w']} x {e['h']}, readout {e['rho']}, path amp {e['amp']}, omega {e['omega']}, seed {e['seed']}; "
                 f"analytic corner skew per frame (px): {[round(s, 2) for s in skew]} (max {max(skew):.2f}).\n")
    frames = R.rolling_clip(path, e["n"], e["rho"], dev).numpy()
    twin_frames = R.rolling_clip(path, e["n"], 0.0, dev).numpy()
    lines.append("| mode | PSNR none (dB) | PSNR rolling (dB) | PSNR twin (dB) | share of the gap | auto readout | auto error | meta skew_px_max |")
    lines.append("|---|---|---|---|---|---|---|---|")
    for mode in ("similarity", "translation"):
        runs = [cpu_run(oracle, fp, hm, rs, frames, mode, None), cpu_run(oracle, fp, hm, rs, frames, mode, e["rho"]),
                cpu_run(oracle, fp, hm, rs, twin_frames, mode, None)]
        auto = cpu_run(oracle, fp, hm, rs, frames, mode, "auto")[3]
        as_torch = [(torch.from_numpy(f), torch.from_numpy(m), final) for f, m, final, _ in runs]
        p, share = T.share_of_the_gap(as_torch, e["h"], e["w"], dev)
        row = {"mode": mode, "psnr_none": round(p[0], 2), "psnr_rolling": round(p[1], 2), "psnr_twin": round(p[2], 2),
               "share": round(share, 3), "auto_readout": round(auto["readout"], 4), "auto_error": round(abs(auto["readout"] - e["rho"]), 4),
               "auto": {k: v for k, v in auto.items() if k != "velocity"}, "skew_px_max": round(runs[1][3]["skew_px_max"], 2)}
        print(json.dumps(row), flush=True)
        lines.append(f"| {mode} | {p[0]:.2f} | {p[1]:.2f} | {p[2]:.2f} | {share:.3f} | {auto['readout']:.4f} | "
                     f"{abs(auto['readout'] - e['rho']):.4f} | {runs[1][3]['skew_px_max']:.2f} |")
    lines.append("")


def gpu_end_to_end(lines):
    """The same clip through the package on the GPU: what tests/test_rolling_shutter_gpu.py asserts on."""
    import torch

    from vstab_amd import native

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    e = T.E2E
    path = T.e2e_path()
    frames, twin_frames = R.rolling_clip(path, e["n"], e["rho"], dev), R.rolling_clip(path, e["n"], 0.0, dev)
    lines.append("| mode | PSNR none (dB) | PSNR rolling (dB) | PSNR twin (dB) | share of the gap | auto readout | auto error |")
    lines.append("|---|---|---|---|---|---|---|")
    for mode in ("similarity", "translation"):
        results = [T._stabilize(ctx, frames, mode), T._stabilize(ctx, frames, mode, rolling_shutter=e["rho"]), T._stabilize(ctx, twin_frames, mode)]
        auto = T._stabilize(ctx, frames, mode, rolling_shutter="auto").meta["rolling_shutter"]
        p, share = T.share_of_the_gap([(r.frames, r.masks[..., 0], T.final_matrices(r.meta)) for r in results], e["h"], e["w"], dev)
        print(json.dumps({"gpu_mode": mode, "psnr": [round(v, 2) for v in p], "share": round(share, 3),
                          "auto": {k: v for k, v in auto.items() if k != "velocity"}}), flush=True)
        lines.append(f"| {mode} | {p[0]:.2f} | {p[1]:.2f} | {p[2]:.2f} | {share:.3f} | {auto['readout']:.4f} | {abs(auto['readout'] - e['rho']):.4f} |")
    lines.append("")


def accuracy_table(lines):
    from vstab_amd import rolling_shutter as rs

    lines.append("| fit | readout | size | estimates (seeds 0, 1, 2) | worst error |")
    lines.append("|---|---|---|---|---|")
    worst = 0.0
    for mode, rho, size in itertools.product(TC.FIT_MODES, TC.READOUTS, TC.SIZES):
        got = [TC.estimate_case(rs, mode, rho, size, seed)["readout"] for seed in TC.SEEDS]
        err = max(abs(g - rho) for g in got)
        worst = max(worst, err)
        lines.append(f"| {mode} | {rho} | {size[0]} x {size[1]} | {', '.join(f'{g:.4f}' for g in got)} | {err:.4f} |")
    lines.append(f"\nWorst |rho_hat - rho| over the {len(TC.FIT_MODES) * len(TC.READOUTS) * len(TC.SIZES) * len(TC.SEEDS)} cases: {worst:.4f}.\n")
    print(json.dumps({"accuracy_worst_error": round(worst, 4)}), flush=True)


def gpu_cost(lines, n=256, reps=7):
    import torch

    import bench
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import native

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, dev)
    work = hm._working_estimation_size(w, h)
    grid_out = []
    records = fp.estimate_transitions(ctx, frames, work, "similarity", grid_out=grid_out)
    mats = fp.select_transitions(records, "similarity")[0]
    final = np.tile(np.array([[1, 0, 3.25], [0, 1, -2.5], [0, 0, 1]], np.float32), (n, 1, 1))
    velocity = np.tile([0.002, -0.003, 6.0, 0.003, 0.002, -4.0], (n, 1))
    ctx.set_timing(True)
    kinds = {"warp": [], "rolling_warp": [], "row_residual": []}
    for _ in range(reps + 1):   # the first of each is the warm-up
        ctx.warp_batch(frames, final, (w, h), want_mask=True, want_count=True)
        kinds["warp"].append(ctx.last_kernel_ms("warp"))
        ctx.rolling_warp_batch(frames, final, (w, h), velocity, 0.7, want_mask=True, want_count=True)
        kinds["rolling_warp"].append(ctx.last_kernel_ms("rolling_warp"))
        ctx.row_residual_batch(grid_out[0], fp.SAMPLE_STEP, work, mats)
        kinds["row_residual"].append(ctx.last_kernel_ms("row_residual"))
    ctx.set_timing(False)
    out = {"frames": n, "size": [w, h], "working_size": list(work), "launches": reps, "ms": {}}
    lines.append(f"C2 clip: {n} frames {w} x {h}, working size {work[0]} x {work[1]}; HIP events, median of {reps} launches after one warm-up.\n")
    lines.append("| kind | median (ms) | all launches (ms) |")
    lines.append("|---|---|---|")
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
        lines.append(f"| {k} | {out['ms'][k]['median']:.4f} | {', '.join(f'{x:.4f}' for x in v)} |")
    out["rolling_warp_over_warp"] = round(out["ms"]["rolling_warp"]["median"] / out["ms"]["warp"]["median"], 3)
    lines.append(f"\nrolling_warp / warp = {out['rolling_warp_over_warp']:.3f}; at 28 B per output pixel the two kernels move "
                 f"{n * w * h * 28 / (out['ms']['warp']['median'] * 1e-3) / 1e12:.2f} and "
                 f"{n * w * h * 28 / (out['ms']['rolling_warp']['median'] * 1e-3) / 1e12:.2f} TB/s.\n")
    print(json.dumps(out), flush=True)


def next_profile() -> Path:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    return ROOT / "profiles" / f"r{max(taken, default=0) + 1:02d}_rolling_shutter.md"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="only the figures that need no GPU")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    graft.load_package()
    import torch

    gpu = torch.cuda.is_available() and not args.cpu
    lines = ["# Rolling shutter: what the correction recovers, how well the readout is found, what it costs", "",
             "Written by tools/rolling_shutter_report.py" + (" --cpu" if args.cpu else "") + ".", ""]
    lines += ["## End to end, on the CPU (oracle estimation chain + host plan + the restatement's warp)", "",
              "What the assertions of tests/test_rolling_shutter_gpu.py are derived from: half of the share, twice the auto error.", ""]
    cpu_end_to_end(lines)
    lines += ["## Readout estimate on analytic rolling flows (least-squares fits, NumPy)", ""]
    accuracy_table(lines)
    if gpu:
        lines += ["## End to end, on the MI355X (the package itself)", ""]
        gpu_end_to_end(lines)
        lines += ["## Kernel times (MI355X)", ""]
        gpu_cost(lines)
    else:
        lines += ["## Kernel times", "", "NOT MEASURED: this run had no GPU.", ""]
    out = Path(args.out) if args.out else next_profile()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
