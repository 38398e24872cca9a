"""Kernel time of the temporal fill on the C2 clip (256 x 1080p, similarity, crop_and_pad), device-resident, HIP-event time
of the fill launch (timing kind "fill"), next to the warp's own time and to the naive composition (K plain warps + a
select per candidate):  python tools/temporal_fill_timing.py [frames] [radius ...]"""
import json, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import __graft_entry__ as graft
graft.load_package()
import bench
from vstab_amd import flow_pipeline as fp, host_math as hm, native, temporal_fill as tf

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
radii = [int(a) for a in sys.argv[2:]] or [2, 8, 16]
h, w, reps = 1080, 1920, 5
dev = torch.device("cuda", 0)
ctx = native.Context(0)
frames = bench.synth_clip(n, 0, h, w, dev)
res = fp._stabilize_frames(hm._normalize_video_input(frames), *bench.FLOW_ARGS, ctx=ctx, keep_on_device=True)
plan = tf.plan_from_meta(res.meta)
dst0, mask0 = res.frames, res.masks[..., 0].contiguous()
out = {"frames": n, "size": [w, h], "flow_args": [str(a) for a in bench.FLOW_ARGS], "padding_fraction_mean": res.meta["padding_fraction_mean"],
       "padding_fraction_max": res.meta["padding_fraction_max"], "rows": []}

ctx.set_timing(True)
warp_ms = []
for _ in range(reps + 1):   # the plain warp of the same clip, for scale
    ctx.warp_batch(frames, plan["final_matrices"], plan["output_size"], border=(0.5, 0.5, 0.5), want_mask=True, want_count=True)
    torch.cuda.synchronize()
    warp_ms.append(ctx.last_kernel_ms("warp"))
out["warp_ms"] = round(float(np.median(warp_ms[1:])), 4)

for radius in radii:
    mats, cand = tf.fill_candidates(plan["final_matrices"], plan["transitions"], plan["confidences"], radius)
    ms = []
    for _ in range(reps + 1):
        d, m = dst0.clone(), mask0.clone()
        _, fc, pc = ctx.temporal_fill_batch(frames, mats, cand, d, m)
        torch.cuda.synchronize()
        ms.append(ctx.last_kernel_ms("fill"))
    block = tf.fill_meta(radius, fc.cpu().numpy(), pc.cpu().numpy(), plan["output_size"])
    # the naive composition: one plain warp of the shifted clip per candidate slot, then a select
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    naive = []
    for _ in range(2):
        d, m = dst0.clone(), mask0.clone()
        torch.cuda.synchronize()
        start.record()
        for k in range(2 * radius):
            j = cand[:, k]
            ok = np.nonzero(j >= 0)[0]
            if not ok.size:
                continue
            a, b = int(ok[0]), int(ok[-1]) + 1          # the slot's frames are one run (clip edges cut its ends)
            cw, cm, _ = ctx.warp_batch(frames[int(j[a]):int(j[b - 1]) + 1], mats[a:b, k], plan["output_size"], want_mask=True)
            take = (m[a:b] == 1.0) & (cm == 0.0)
            d[a:b] = torch.where(take[..., None], cw, d[a:b])
            m[a:b] = torch.where(take, torch.zeros_like(cm), m[a:b])
        stop.record()
        torch.cuda.synchronize()
        naive.append(start.elapsed_time(stop))
    out["rows"].append({"radius": radius, "K": 2 * radius, "fill_ms": round(float(np.median(ms[1:])), 4),
                        "fill_ms_all": [round(v, 4) for v in ms], "naive_ms": round(min(naive), 3), **block})
print(json.dumps(out))
