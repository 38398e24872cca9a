#!/usr/bin/env python3
"""Rolling-shutter refit: what fitting the pair transitions again on readout-corrected samples buys, and what it costs.

  always     No GPU needed.  The analytic cases of tests/test_rolling_refit_cpu.py (exact rolling flows, least-squares similarity
             fits, the NumPy restatement of the rectifier): pair and chain errors of the first pass, of one refit pass, of a
             second pass, and of one pass with the readout "auto" reports on that clip.
  on a GPU   (not with --cpu) the end-to-end clip of tests/test_rolling_refit_gpu.py through the package in both modes: PSNR
             against the static texture without the keywords, with rolling_shutter, with rolling_shutter + rolling_refit and of
             the global-shutter twin's run, over the pixels all four show, and the share of the gap each recovers -- the
             similarity share is the constant of the GPU test.  Then the kernel time of rectify_samples_batch for the 255 pairs
             of the C2 working grid next to row_residual_batch and one points_fit_batch launch of the same run (HIP events,
             median of 7 after one warm-up).
  --bench-logs DIR   the `value` (frames/s) of the bench.py lines found there as bench_parent_<k>.log and bench_pr_<k>.log --
             `bench.py --gpus 1` run alternately in a checkout of the parent commit and in this tree, a round's two runs on one
             box -- as a table
             with the parent's own spread.

    python tools/rolling_refit_report.py [--cpu] [--bench-logs DIR] [--out profiles/rNN_rolling_refit.md]

Writes the next free profiles/rNN_rolling_refit.md unless --out names a file.
"""
import argparse
import json
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import __graft_entry__ as graft  # noqa: E402
from tests import rolling_refit_restatement as RF  # noqa: E402
from tests import test_rolling_refit_gpu as T  # noqa: E402


def analytic_table(lines):
    from vstab_amd import rolling_shutter as rs

    def refit(case, flows, transitions, readout):
        size = (case["w"], case["h"])
        velocity = rs.velocities(transitions, np.ones(len(transitions)), None)
        pairs, counts, _ = RF.rectify_samples(flows, RF.STEP, size, velocity, readout)
        return np.stack([RF.similarity_from_pairs(pairs[k], counts[k]) for k in range(len(transitions))])

    for name, case in (("480 x 270, 12 frames", RF.BIG), ("61 x 45, 8 frames", RF.SMALL)):
        size = (case["w"], case["h"])
        flows, truth, first = RF.analytic_case(case)
        once = refit(case, flows, first, case["rho"])
        rows = [("first pass: fits on the raw samples", first), ("one refit on rectified samples (true readout)", once),
                ("a second refit pass", refit(case, flows, once, case["rho"]))]
        if case is RF.BIG:
            rows.append(("one refit with the readout \"auto\" finds (0.643)", refit(case, flows, first, 0.643)))
        lines += [f"{name}, amp {case['amp']}, omega {case['omega']}, seed {case['seed']}, readout {case['rho']}; corner errors in px.", "",
                  "| | pair error, mean | pair error, worst | chain (worst corner, all frames) |", "|---|---|---|---|"]
        for label, mats in rows:
            pair, chain = RF.corner_errors(mats, truth, size)
            lines.append(f"| {label} | {pair.mean():.4f} | {pair.max():.3f} | {chain:.3f} |")
            print(json.dumps({"analytic": name, "row": label, "pair_mean": round(float(pair.mean()), 4), "pair_worst": round(float(pair.max()), 3),
                              "chain": round(chain, 3)}), flush=True)
        lines.append("")


def gpu_end_to_end(lines):
    import torch

    from tests import rolling_shutter_restatement as R
    from vstab_amd import native

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    e = T.E2E
    path = R.CameraPath(e["w"], e["h"], amp=e["amp"], omega=e["omega"], seed=e["seed"])
    frames, twin = R.rolling_clip(path, e["n"], e["rho"], dev), R.rolling_clip(path, e["n"], 0.0, dev)
    lines += [f"Clip: {e['n']} frames {e['w']} x {e['h']}, readout {e['rho']}, camera_lock, strength 1; PSNR against the static "
              "texture over the pixels all four runs show, 4 px inside.", "",
              "| mode | PSNR none (dB) | rolling (dB) | rolling + refit (dB) | twin (dB) | share, rolling | share, rolling + refit | refit block |",
              "|---|---|---|---|---|---|---|---|"]
    for mode in ("similarity", "translation"):
        runs = [T._stabilize(ctx, frames, mode), T._stabilize(ctx, frames, mode, rolling_shutter=e["rho"]),
                T._stabilize(ctx, frames, mode, rolling_shutter=e["rho"], rolling_refit=True), T._stabilize(ctx, twin, mode)]
        p = T.psnr_of_runs(runs, e["h"], e["w"], dev)
        shares = [(p[1] - p[0]) / (p[3] - p[0]), (p[2] - p[0]) / (p[3] - p[0])]
        block = runs[2].meta["rolling_shutter"]["refit"]
        print(json.dumps({"gpu_mode": mode, "psnr": [round(v, 2) for v in p], "share_rolling": round(shares[0], 3),
                          "share_refit": round(shares[1], 3), "refit": block}), flush=True)
        lines.append(f"| {mode} | {p[0]:.2f} | {p[1]:.2f} | {p[2]:.2f} | {p[3]:.2f} | {shares[0]:.3f} | {shares[1]:.3f} | `{json.dumps(block)}` |")
    lines.append("")


def gpu_cost(lines, n=256, reps=7):
    import torch

    import bench
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import native
    from vstab_amd import rolling_shutter as rs

    ctx = native.default_context()
    dev = torch.device("cuda", 0)
    w, h = 1920, 1080
    frames = bench.synth_clip(n, 0, h, w, dev)
    work = hm._working_estimation_size(w, h)
    grid_out = []
    records = fp.estimate_transitions(ctx, frames, work, "similarity", grid_out=grid_out)
    mats, _, confidences, _, _ = fp.select_transitions(records, "similarity")
    velocity = rs.velocities(mats, confidences, None)
    grid = grid_out[0]
    ctx.set_timing(True)
    kinds = {"rectify": [], "row_residual": [], "fit": []}
    for _ in range(reps + 1):   # the first of each is the warm-up
        pairs, counts, _ = ctx.rectify_samples_batch(grid, fp.SAMPLE_STEP, work, velocity, 0.7)
        kinds["rectify"].append(ctx.last_kernel_ms("rectify"))
        ctx.row_residual_batch(grid, fp.SAMPLE_STEP, work, mats)
        kinds["row_residual"].append(ctx.last_kernel_ms("row_residual"))
        ctx.points_fit_batch(pairs, counts, "similarity")
        kinds["fit"].append(ctx.last_kernel_ms("fit"))
    ctx.set_timing(False)
    cells = int(grid.shape[1] * grid.shape[2])
    out = {"pairs": n - 1, "working_size": list(work), "grid": [int(grid.shape[2]), int(grid.shape[1])], "launches": reps, "ms": {}}
    lines += [f"C2 clip: {n} frames {w} x {h}, working size {work[0]} x {work[1]}, {n - 1} pairs of {cells} samples; HIP events, "
              f"median of {reps} launches after one warm-up.  `fit` is one points_fit_batch launch on the rectifier's output.", "",
              "| kind | median (ms) | all launches (ms) |", "|---|---|---|"]
    for k, v in kinds.items():
        out["ms"][k] = {"median": round(float(np.median(v[1:])), 4), "all": [round(x, 4) for x in v]}
        lines.append(f"| {k} | {out['ms'][k]['median']:.4f} | {', '.join(f'{x:.4f}' for x in v)} |")
    moved = (n - 1) * cells * (8 + 16)
    lines.append(f"\nThe rectifier reads 8 and writes 16 bytes per sample: {moved / (out['ms']['rectify']['median'] * 1e-3) / 1e9:.1f} GB/s "
                 "from one workgroup per pair.\n")
    print(json.dumps(out), flush=True)


def bench_table(folder: Path):
    def values(stem):
        found = []
        for p in sorted(folder.glob(stem + "_*.log")):
            last = [ln for ln in p.read_text().splitlines() if ln.startswith("{")][-1]      # the result line
            found.append(float(json.loads(last)["value"]))
        return found

    parent, pr = values("bench_parent"), values("bench_pr")
    if not (parent and pr):
        return ["## Default path: `bench.py --gpus 1`", "", f"NOT MEASURED: no bench logs in {folder.name}.", ""]
    out = ["## Default path: `bench.py --gpus 1 --steps 5 --warmup 2`, alternating parent / this tree, the two runs of a round on one box", "",
           "| round | parent frames/s | this tree frames/s |", "|---|---|---|"]
    out += [f"| {k + 1} | {a:.1f} | {b:.1f} |" for k, (a, b) in enumerate(zip(parent, pr))]
    spread = (max(parent) - min(parent)) / float(np.median(parent))
    print(json.dumps({"bench_parent": parent, "bench_pr": pr}), flush=True)
    return out + ["", f"Medians: parent {np.median(parent):.1f}, this tree {np.median(pr):.1f} frames/s "
                      f"({100.0 * (np.median(pr) / np.median(parent) - 1.0):+.2f} %); the parent's own spread over its runs: "
                      f"{100.0 * spread:.2f} %.  The default path launches nothing new.", ""]


def next_profile() -> Path:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)_", p.name))]
    return ROOT / "profiles" / f"r{max(taken, default=0) + 1:02d}_rolling_refit.md"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="only the figures that need no GPU")
    ap.add_argument("--bench-logs", default=None, help="a directory with bench_parent_<k>.log / bench_pr_<k>.log")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    graft.load_package()
    import torch

    gpu = torch.cuda.is_available() and not args.cpu
    lines = ["# Rolling-shutter refit: what one pass on readout-corrected samples buys, and what it costs", "",
             "Written by tools/rolling_refit_report.py" + (" --cpu" if args.cpu else "") + ".", "",
             "## Analytic rolling flows, least-squares similarity fits (NumPy)", ""]
    analytic_table(lines)
    if gpu:
        lines += ["## End to end, on the MI355X (the package itself)", ""]
        gpu_end_to_end(lines)
        lines += ["## Kernel times (MI355X)", ""]
        gpu_cost(lines)
    else:
        lines += ["## End to end and kernel times", "", "NOT MEASURED: this run had no GPU.", ""]
    if args.bench_logs:
        lines += bench_table(Path(args.bench_logs))
    out = Path(args.out) if args.out else next_profile()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
