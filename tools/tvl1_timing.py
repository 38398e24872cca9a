"""Times the Flow pipeline on its TV-L1 estimator (estimator="flow_tvl1") on the C2 clip (256 x 1080p, similarity,
crop_and_pad), and the estimator call alone with its inner-iteration table.

  python tools/tvl1_timing.py [--frames N] [--out result.json]
      ms per clip and per pair, mean inner iterations per scale (and per pair), the modelled bytes of the
      inner-iteration kernel: 64 B per pixel and iteration of an active pair (csrc/vstab_tvl1.hip).
  python tools/tvl1_timing.py --stats kernel_stats.csv --result result.json
      with the `rocprofv3 --kernel-trace --stats --output-format csv` table of a run of this tool: the inner kernel's total time and
      its achieved bandwidth on the modelled bytes (against the 8 TB/s HBM peak).
"""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BYTES_PER_PX_ITER = 64
HBM_PEAK = 8.0e12


def bandwidth(stats_csv, result_json):
    res = json.loads(Path(result_json).read_text())
    rows = list(csv.DictReader(open(stats_csv)))
    inner = [r for r in rows if "tvl1_inner_kernel" in r["Name"]]
    if not inner:
        raise SystemExit("no tvl1_inner_kernel row in " + str(stats_csv))
    total_ns = sum(float(r["TotalDurationNs"]) for r in inner)
    calls = sum(int(r["Calls"]) for r in inner)
    # the profiled run computes the clip's TV-L1 this many times (warm-up, timed pipeline passes, the estimator call)
    runs = res["inner_kernel_runs"]
    modelled = res["inner_modelled_bytes_per_call"] * runs
    bw = modelled / (total_ns * 1e-9)
    out = {"inner_kernel_ms_total": round(total_ns * 1e-6, 3), "inner_kernel_launches": calls,
           "inner_modelled_GB": round(modelled / 1e9, 3), "inner_achieved_TBps": round(bw / 1e12, 3),
           "fraction_of_8TBps": round(bw / HBM_PEAK, 3)}
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--result", default=None)
    args = ap.parse_args()
    if args.stats is not None:
        bandwidth(args.stats, args.result)
        return

    import numpy as np
    import torch

    import __graft_entry__ as graft
    import bench

    graft.load_package()
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import native

    n, h, w = args.frames, 1080, 1920
    dev = torch.device("cuda", 0)
    ctx = native.Context(0)
    frames = bench.synth_clip(n, 0, h, w, dev)
    torch.cuda.synchronize()

    def step():
        context = hm.VideoContext([None] * n, hm.FrameAdapter(np.dtype(np.float32), False, "0_1", "torch", False), w, h, 3, None,
                                  "sequence", {}, batch=frames)
        return fp._stabilize_frames(context, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0, ctx=ctx,
                                    keep_on_device=True, estimator="flow_tvl1")

    res = step()   # warm-up (workspace allocation)
    meta = res.meta
    del res
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.runs):
        res = step()
        del res
    torch.cuda.synchronize()
    clip_ms = (time.perf_counter() - t0) / args.runs * 1e3

    # the estimator alone on the clip's estimation images, with its iteration table
    ws = hm._working_estimation_size(w, h)
    gray = ctx.gray_downscale(frames, ws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, iters = ctx.tvl1_flow_batch(gray, want_grid=True, want_iterations=True)
    torch.cuda.synchronize()
    est_ms = (time.perf_counter() - t0) * 1e3
    it = iters.cpu().numpy().astype(np.int64)   # [pairs, scales, warps]
    gh, gw = gray.shape[1], gray.shape[2]
    from tests import tvl1_restatement as R

    sizes = R.pyramid_sizes(gh, gw, 5, 0.8)
    npx = np.array([hh * ww for hh, ww in sizes] + [0] * (5 - len(sizes)), np.int64)
    modelled = int(BYTES_PER_PX_ITER * (it.sum(axis=2) * npx[None, :]).sum())
    pairs = n - 1
    out = {
        "clip": f"{n} x {h}x{w}, estimation {gw}x{gh}", "backend": meta["flow_backend"],
        "ms_per_clip": round(clip_ms, 1), "ms_per_pair": round(clip_ms / pairs, 3),
        "estimator_ms": round(est_ms, 1), "estimator_ms_per_pair": round(est_ms / pairs, 3),
        "scales": [f"{ww}x{hh}" for hh, ww in sizes],
        "mean_inner_iterations_per_scale": [round(float(v), 1) for v in it.sum(axis=2).mean(axis=0)],
        "mean_inner_iterations_per_pair": round(float(it.sum(axis=(1, 2)).mean()), 1),
        "max_inner_iterations_per_scale": [int(v) for v in it.sum(axis=2).max(axis=0)],
        "inner_modelled_bytes_per_call": modelled,
        "inner_kernel_runs": args.runs + 2,   # warm-up + timed pipeline passes + the estimator call
        "modes": sorted(set(t["mode"] for t in meta["estimated_motion"]["per_transition"])),
    }
    print(json.dumps(out))
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
