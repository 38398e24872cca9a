#!/usr/bin/env python3
"""Drift correction: what it costs and what it recovers; writes the next free profiles/rNN_drift_exposure.md.

  1. kernel time per launch of anchor_sums_batch for 256 frames at 960x540 (every frame but the first anchored, keyframes
     every 32) next to pair_residual_batch of the same run: HIP events, median of 7 after one warm-up;
  2. the 64-frame 960x540 clips of tests/test_drift_correction_gpu.py through the pipeline, without and with the keyword:
     chain of the reported transitions against the analytic path (worst frame, centre / corner in working px), launches used,
     frames refined / kept -- also with sigma 0.03 noise added to the frames;
  3. camera lock on the similarity clip: PSNR against the static texture without and with;
  4. a clip whose exposure drifts by 20 % over its length, and one whose exposure flickers from frame to frame: the chain
     without and with drift_exposure; the same kernel timing for anchor_sums_ex, unmasked and masked, in section 1;
  5. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` alternating between the two trees.

    python tools/drift_correction_report.py [--out FILE] [--parent DIR] [--rounds 3] [--steps 20] [--warmup 5]

A section whose run did not happen says NOT MEASURED.
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


def next_profile() -> Path:
    taken = [int(m.group(1)) for p in (ROOT / "profiles").glob("r*") if (m := re.match(r"r(\d+)_", p.name))]
    return ROOT / "profiles" / f"r{max(taken, default=0) + 1:02d}_drift_exposure.md"


def bench_once(tree: Path, steps: int, warmup: int) -> float:
    """One `bench.py --gpus 1` in a child process of its own -> frames/s of its result line.  A child that fails, or ends
    without a result line, ends the tool: nothing more is started on a GPU that a process may just have faulted."""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=str(tree),
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"bench.py in {tree} ended with status {out.returncode}; nothing more is run\n"
                         + out.stdout[-2000:] + out.stderr[-2000:])
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and '"value"' in line:
            return float(json.loads(line)["value"])
    raise SystemExit(f"bench.py in {tree} printed no result line; nothing more is run\n" + out.stdout[-2000:] + out.stderr[-2000:])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    out_path = Path(args.out) if args.out else next_profile()
    given = " ".join(a for a in sys.argv[1:])
    lines = ["# Drift correction: cost and figures", "", f"`python tools/drift_correction_report.py {given}`".replace(" `", "`") + " on one MI355X.", ""]

    # the benchmark first, in child processes, before this process opens the GPU
    lines += ["## bench.py --gpus 1, alternating with the parent commit", ""]
    if args.parent:
        rows = {"this tree": [], "parent": []}
        for _ in range(args.rounds):
            for name, tree in (("this tree", ROOT), ("parent", Path(args.parent))):
                rows[name].append(bench_once(tree, args.steps, args.warmup))
                print(f"bench {name}: {rows[name][-1]}", flush=True)
        for name, vals in rows.items():
            lines.append(f"- {name}: median {np.median(vals):.1f} frames/s ({min(vals):.1f} .. {max(vals):.1f}), runs "
                         f"{', '.join(f'{v:.1f}' for v in vals)}")
        lines += ["", f"{args.rounds} rounds of `--steps {args.steps} --warmup {args.warmup}`, one child process per run.  The default "
                      "path calls nothing new.", ""]
    else:
        lines += ["NOT MEASURED (no --parent checkout given).", ""]

    import torch

    graft.load_package()
    import bench
    from tests import drift_util as T
    from tests.util import shake_path
    from vstab_amd import drift_correction as dc
    from vstab_amd import native

    dev = torch.device("cuda", 0)
    ctx = native.Context(0)
    reps = 7

    def timed(kind, call):
        ms = []
        for _ in range(reps + 1):
            call()
            torch.cuda.synchronize()
            ms.append(ctx.last_kernel_ms(kind))
        return float(np.median(ms[1:])), ms[1:]

    # ---- 1. kernel time ----------------------------------------------------------------------------------------------
    n, w, h = 256, 960, 540
    cam = shake_path(n, w, h, "similarity", seed=3, amp=1.0)
    gray = torch.cat([ctx.gray_downscale(bench.synth_clip(64, 0, h, w, dev, mats=cam[i:i + 64]), None) for i in range(0, n, 64)])
    true = np.stack([cam[i + 1] @ np.linalg.inv(cam[i]) for i in range(n - 1)])
    sched = dc.schedule(n, None, [0.9] * (n - 1), 32)
    Rm = dc.chained(true, sched).reshape(n, 6)
    ctx.set_timing(True)
    anchor_ms, anchor_runs = timed("anchor", lambda: ctx.anchor_sums_batch(gray, sched.anchor, Rm, dc.RESIDUAL_CAP))
    cut_ms, cut_runs = timed("cut", lambda: ctx.pair_residual_batch(gray, true.astype(np.float32)))
    step = 8
    blocked = (torch.rand((n, -(-h // step), -(-w // step)), device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.3).to(torch.uint8)
    gains = np.full(n, 900)
    ex_ms, ex_runs = timed("anchor_ex", lambda: ctx.anchor_sums_ex_batch(gray, sched.anchor, Rm, dc.RESIDUAL_CAP, gains))
    exm_ms, exm_runs = timed("anchor_ex", lambda: ctx.anchor_sums_ex_batch(gray, sched.anchor, Rm, dc.RESIDUAL_CAP, gains, None, blocked, step))
    ctx.set_timing(False)
    frames_bytes = 2.0 * h * w * (n - 1)
    lines += [f"## Kernel time, {n} frames of {w}x{h} (HIP events, median of {reps})", "",
              "| kernel | ms per launch | TB/s against 2 h w bytes per frame | runs ms |", "|---|---|---|---|",
              f"| anchor_sums ({n - 1} anchored frames) | {anchor_ms:.3f} | {frames_bytes / (anchor_ms * 1e-3) / 1e12:.2f} | {', '.join(f'{v:.3f}' for v in anchor_runs)} |",
              f"| anchor_sums_ex, unmasked | {ex_ms:.3f} | {frames_bytes / (ex_ms * 1e-3) / 1e12:.2f} | {', '.join(f'{v:.3f}' for v in ex_runs)} |",
              f"| anchor_sums_ex, 30 % of the grid blocked at random | {exm_ms:.3f} | {frames_bytes / (exm_ms * 1e-3) / 1e12:.2f} | {', '.join(f'{v:.3f}' for v in exm_runs)} |",
              f"| pair_residual ({n - 1} pairs) | {cut_ms:.3f} | {frames_bytes / (cut_ms * 1e-3) / 1e12:.2f} | {', '.join(f'{v:.3f}' for v in cut_runs)} |", "",
              f"anchor_sums / pair_residual = {anchor_ms / cut_ms:.2f}.  A corrected call launches it `iterations + 1` times.",
              f"anchor_sums_ex / anchor_sums = {ex_ms / anchor_ms:.2f} unmasked, {exm_ms / anchor_ms:.2f} masked (31 accumulators against 17: {31 / 17:.2f}).", ""]
    del gray, blocked
    torch.cuda.empty_cache()

    # ---- 2. accuracy -------------------------------------------------------------------------------------------------
    lines += ["## Chain of the reported transitions against the analytic path, 64 frames of 960x540 (working px, worst frame)", "",
              "| clip | noise sigma | spacing | centre without | corner without | centre with | corner with | launches | refined | kept |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    clips = {}
    for kind in ("similarity", "translation"):
        cam = shake_path(T.N, T.W, T.H, kind, seed=3, amp=1.0)
        clips[kind] = (cam, bench.synth_clip(T.N, 0, T.H, T.W, dev, mats=cam))
    gen = torch.Generator(device=dev).manual_seed(7)
    for kind, sigma, spacing in (("similarity", 0.0, 32), ("similarity", 0.0, 16), ("translation", 0.0, 32), ("similarity", 0.03, 32),
                                 ("translation", 0.03, 32)):
        cam, frames = clips[kind]
        if sigma:
            frames = (frames + sigma * torch.randn(frames.shape, device=dev, generator=gen)).clamp(0.0, 1.0)
        c0, k0 = T.chain_error(T.stabilize(ctx, frames, kind).meta, cam)
        block = T.stabilize(ctx, frames, kind, drift_correction=spacing).meta
        c1, k1 = T.chain_error(block, cam)
        b = block["drift_correction"]
        kept = {k: v for k, v in b["frames_kept"].items() if v}
        lines.append(f"| {kind} | {sigma} | {spacing} | {c0:.4f} | {k0:.4f} | {c1:.4f} | {k1:.4f} | {b['iterations'] + 1} | {b['frames_refined']} | {kept} |")
    lines.append("")

    # ---- 3. the lock -------------------------------------------------------------------------------------------------
    cam, frames = clips["similarity"]
    without = bench.static_texture_error(T.stabilize(ctx, frames, "similarity", args=T.LOCK_ARGS), cam, frames, dev)
    with_it = bench.static_texture_error(T.stabilize(ctx, frames, "similarity", args=T.LOCK_ARGS, drift_correction=True), cam, frames, dev)
    lines += ["## Camera lock, strength 1, crop_and_pad, similarity clip: error against the static texture", "",
              f"- without: {json.dumps(without)}", f"- with drift_correction=True: {json.dumps(with_it)}",
              f"- the test's gate is the PSNR with the keyword less 1 dB: {with_it['psnr_db'] - 1.0:.2f} dB", ""]

    # ---- 4. exposure: a ramp and per-frame flicker ---------------------------------------------------------------------
    ramp = frames * torch.linspace(1.0, 0.8, T.N, device=dev).view(-1, 1, 1, 1)
    rng = np.random.default_rng(11)                   # the flicker of tests/test_drift_exposure_gpu.py
    g, o = rng.uniform(0.75, 0.95, T.N), rng.uniform(0.0, 0.04, T.N)
    flicker = frames * torch.from_numpy(g).float().to(dev).view(-1, 1, 1, 1) + torch.from_numpy(o).float().to(dev).view(-1, 1, 1, 1)
    anchor = [-1] + [32 * ((i - 1) // 32) for i in range(1, T.N)]
    want = np.array([1.0] + [g[i] / g[anchor[i]] for i in range(1, T.N)])
    lines += ["## Exposure: falling by 20 % over the clip (ramp), and per-frame gains in [0.75, 0.95] with offsets in [0, 0.04] (flicker)", "",
              "| clip | call | centre | corner | launches | refined | kept | residual before -> after |", "|---|---|---|---|---|---|---|---|"]
    for name, clip in (("ramp", ramp), ("flicker", flicker)):
        c0, k0 = T.chain_error(T.stabilize(ctx, clip, "similarity").meta, cam)
        lines.append(f"| {name} | no drift_correction | {c0:.4f} | {k0:.4f} | | | | |")
        for label, kw in (("drift_correction=True", {}), ("+ drift_exposure=True", dict(drift_exposure=True))):
            meta = T.stabilize(ctx, clip, "similarity", drift_correction=True, **kw).meta
            c1, k1 = T.chain_error(meta, cam)
            b = meta["drift_correction"]
            kept = {k: v for k, v in b["frames_kept"].items() if v}
            lines.append(f"| {name} | {label} | {c1:.4f} | {k1:.4f} | {b['iterations'] + 1} | {b['frames_refined']} | {kept} | "
                         f"{b['residual_before']:.3f} -> {b['residual_after']:.3f} |")
            if kw and name == "flicker":
                worst = float(np.max(np.abs(np.array(b["exposure"]["gain"]) - want)))
    lines += ["", f"Flicker: the worst |reported gain - g_i / g_anchor(i)| over the clip is {worst:.5f}.  Under drift_exposure "
                  "`residual_before` is the second launch (the chained matrices under the estimated exposure).", ""]
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
