"""Per-launch device time of every kernel that ends in the block-level integer sum (BlockSums / block_count_add,
csrc/vstab_internal.h) and whose listing a change of that helper can move: one warm-up and `--launches` timed launches per
kind in this process, the device events of set_timing / last_kernel_ms, median and 10th-90th percentile in ms, and a checksum
of each kind's outputs (equal between two builds of the library: the sums are integers).

   python tools/block_sums_timing.py [--n 256] [--launches 40] [--kinds cut,anchor,...] [--label NAME]
   AB_LIB=... tools/ab_lib.sh python tools/block_sums_timing.py ...          (the other build, a fresh process each)

Shapes: the C2 clip, n x 1920x1080 float32 frames; the estimation-side kernels (cut, anchor, anchor_ex, rectify) at the
960x540 working size, step 8.  Synthetic content: a smooth pattern with a little noise, similarity matrices with some pixels
of shift, so that the warps pad a rim and every pass has pixels to count and pixels to skip.  Prints one JSON line.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import __graft_entry__ as graft

graft.load_package()
from vstab_amd import native  # noqa: E402

KINDS = ("cut", "anchor", "anchor_ex", "rectify", "sharpness", "stability", "gain_hist", "gain_sums", "apply_gain",
         "mesh_unwarp", "rolling_unwarp", "fill", "fill_gain", "fill_blend", "sfill")
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--launches", type=int, default=40)
ap.add_argument("--kinds", default=",".join(KINDS))
ap.add_argument("--label", default="")
args = ap.parse_args()
kinds = [k for k in args.kinds.split(",") if k]
assert all(k in KINDS for k in kinds), f"kinds are {KINDS}"

torch.manual_seed(0)
rng = np.random.default_rng(0)
dev = torch.device("cuda", 0)
ctx = native.Context(0)
n, h, w, wh, ww, step = args.n, 1080, 1920, 540, 960, 8
gh, gw = (wh + step - 1) // step, (ww + step - 1) // step


def pattern(rows, cols, scale):
    y = torch.arange(rows, device=dev, dtype=torch.float32)[:, None] * scale
    x = torch.arange(cols, device=dev, dtype=torch.float32)[None, :] * scale
    return 0.5 + 0.22 * torch.sin(x / 37.0) + 0.18 * torch.cos(y / 23.0) + 0.06 * torch.sin((x + y) / 11.0)


def similarity(count, shift):
    m = np.tile(np.eye(3), (count, 1, 1))
    th, sc = rng.uniform(-0.01, 0.01, count), rng.uniform(0.99, 1.01, count)
    m[:, 0, 0] = sc * np.cos(th); m[:, 0, 1] = -sc * np.sin(th)
    m[:, 1, 0] = sc * np.sin(th); m[:, 1, 1] = sc * np.cos(th)
    m[:, 0, 2] = rng.uniform(-shift, shift, count); m[:, 1, 2] = rng.uniform(-0.6 * shift, 0.6 * shift, count)
    return m


def checksum(*tensors):
    return [float(t.double().sum()) if t.is_floating_point() else int(t.long().sum()) for t in tensors if t is not None]


def timed(kind, call, prepare=lambda: None):
    ms, out = [], None
    for _ in range(args.launches + 1):
        prepare()
        out = call()
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms(kind))
    ms = np.array(ms[1:])
    out = out if isinstance(out, tuple) else (out,)
    return {"median": round(float(np.median(ms)), 4), "p10": round(float(np.percentile(ms, 10)), 4),
            "p90": round(float(np.percentile(ms, 90)), 4),
            "checksum": checksum(*[torch.as_tensor(o) for o in out if o is not None])}


ctx.set_timing(True)
res = {}

# ---- the estimation side: 960 x 540 gray images ----
if any(k in kinds for k in ("cut", "anchor", "anchor_ex", "rectify")):
    gray = (pattern(wh, ww, 2.0)[None] * 255.0 + torch.randint(-3, 4, (n, wh, ww), device=dev)).clamp(0, 255).to(torch.uint8)
    small = similarity(n, 4.0)
    if "cut" in kinds:
        res["cut"] = timed("cut", lambda: ctx.pair_residual_batch(gray, small[:-1].astype(np.float32)))
    anchor = (np.arange(n) // 32) * 32
    anchor[anchor == np.arange(n)] = -1                      # a keyframe has no anchor
    R = small[:, :2, :].reshape(n, 6)
    if "anchor" in kinds:
        res["anchor"] = timed("anchor", lambda: ctx.anchor_sums_batch(gray, anchor, R, 40))
    if "anchor_ex" in kinds:
        blocked = (torch.rand((n, gh, gw), device=dev) < 0.1).to(torch.uint8)
        gain, offset = rng.integers(900, 1150, n), rng.integers(-4096, 4096, n)
        res["anchor_ex"] = timed("anchor_ex", lambda: ctx.anchor_sums_ex_batch(gray, anchor, R, 40, gain, offset, blocked, step))
    if "rectify" in kinds:
        flow = torch.randn((n - 1, gh, gw, 2), device=dev) * 2.0
        vel = rng.uniform(-10, 10, (n, 6)) * np.array([0.001, 0.001, 1, 0.001, 0.001, 1])
        res["rectify"] = timed("rectify", lambda: ctx.rectify_samples_batch(flow, step, (ww, wh), vel, 0.5)[1:])
    del gray

# ---- the frame side: n x 1080p ----
frames = (pattern(h, w, 1.0)[None, :, :, None] + 0.04 * torch.randn((n, h, w, 3), device=dev)).clamp_(0, 1).contiguous()
final = similarity(n, 20.0).astype(np.float32)
if "sharpness" in kinds:
    res["sharpness"] = timed("sharpness", lambda: ctx.frame_sharpness_batch(frames))
if "gain_hist" in kinds:
    res["gain_hist"] = timed("gain_hist", lambda: ctx.pair_gain_hist_batch(frames, final[:-1]))
if "gain_sums" in kinds:
    band = np.tile(np.array([200, 320], np.int32), (n - 1, 4, 1))
    res["gain_sums"] = timed("gain_sums", lambda: ctx.pair_gain_sums_batch(frames, final[:-1], band))
if "mesh_unwarp" in kinds:
    offsets = torch.randn((n, 10, 17, 2), device=dev) * 3.0
    res["mesh_unwarp"] = timed("mesh_unwarp", lambda: ctx.mesh_unwarp_batch(frames, final, (w, h), offsets, want_mask=True, want_count=True,
                                                                           want_unconverged=True)[1:])
if "rolling_unwarp" in kinds:
    vel = rng.uniform(-20, 20, (n, 6)) * np.array([0.001, 0.001, 1, 0.001, 0.001, 1])
    res["rolling_unwarp"] = timed("rolling_unwarp", lambda: ctx.rolling_unwarp_batch(frames, final, (w, h), vel, 0.5, want_mask=True,
                                                                                    want_count=True, want_unsolved=True)[1:])

if any(k in kinds for k in ("stability", "apply_gain", "fill", "fill_gain", "fill_blend", "sfill")):
    warped, mask0, _ = ctx.warp_batch(frames, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True)
    dst, mask = warped.clone(), mask0.clone()

    def reset():
        dst.copy_(warped)
        mask.copy_(mask0)

    if "stability" in kinds:
        res["stability"] = timed("stability", lambda: ctx.frame_sse_batch(warped[:-1], warped[1:], mask0[:-1], mask0[1:]))
    if "apply_gain" in kinds:
        gains = rng.uniform(1.05, 1.3, (n, 3)).astype(np.float32)
        res["apply_gain"] = timed("apply_gain", lambda: ctx.apply_gain_batch(dst, gains, mask), reset)
    # two candidates per frame: the frame's own matrix moved by 15 px to either side, sampled from the neighbouring frames
    K = 2
    cand = np.stack([np.arange(n) - 1, np.arange(n) + 1], axis=1).astype(np.int32)
    cand[cand >= n] = -1
    mats = np.repeat(final[:, None], K, axis=1).copy()
    mats[:, 0, 0, 2] -= 15.0; mats[:, 1, 0, 2] += 15.0; mats[:, 0, 1, 2] -= 9.0; mats[:, 1, 1, 2] += 9.0
    if "fill" in kinds:
        res["fill"] = timed("fill", lambda: ctx.temporal_fill_batch(frames, mats, cand, dst, mask)[1:], reset)
    if "fill_gain" in kinds:
        res["fill_gain"] = timed("fill_gain", lambda: ctx.fill_gain_sums(frames, mats, cand, final, warped))
    if "fill_blend" in kinds:
        g = rng.uniform(0.95, 1.05, (n, K, 3)).astype(np.float32)
        res["fill_blend"] = timed("fill_blend", lambda: ctx.temporal_fill_blend_batch(frames, mats, cand, final, g, dst, mask, feather_px=16)[1:], reset)
    if "sfill" in kinds:
        res["sfill"] = timed("sfill", lambda: ctx.spatial_fill_batch(dst, mask), reset)

print(json.dumps({"label": args.label, "library": str(native.LIB_PATH), "n": n, "launches": args.launches, "kinds": res}))
