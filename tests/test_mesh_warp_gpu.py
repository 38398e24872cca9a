"""Mesh warp on the GPU (include/vstab.h "mesh warp"; flow_pipeline._stabilize_frames(mesh_warp=...)).

  1. vstab_mesh_residual_batch against the NumPy restatement (tests/mesh_restatement.py): exact equality
  2. all-zero offsets: vstab_mesh_warp_batch == vstab_warp_batch in bits (dst, mask, pad_count)
  3. drawn offsets: == the restatement in bits; a known-answer integer shift
  4. it helps: camera-locked PSNR against the static texture on non-rigid clips, mesh vs plain vs the analytic ceiling
  5. it does no harm on rigid shake     6. None is the call without the keyword, no new kernel is launched
  7. composition: scene cuts, estimation mask, the refusals, the node

The clips of test 4: the bench's texture sampled analytically at p - D_i(p), D_i(p) = g_i + a(p) e_i, g and e random walks,
a(p) a smooth ramp from 0 to 1 across the frame (mesh_restatement.nonrigid_clip).  Measured figures: profiles/r10_mesh_warp.md.
"""

import json
import math

import numpy as np
import pytest

from tests import mesh_restatement as R
from tests import util
from tests.util import shake_path

pytestmark = pytest.mark.gpu

ARGS = (False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
LOCK_ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the target path is 0
PSNR_MARGIN_DB = 1.0          # "meaningfully different", as tests/test_scene_cuts_gpu.py uses it
CLIP_FRAMES = 24


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _stabilize(ctx, frames, mode="similarity", estimator="flow", framing="crop_and_pad", args=ARGS, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, *args, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


# ---- 1. residual kernel == restatement, exactly ----------------------------------------------------------------------------
def _draw_field(rng, pairs, w, h, step):
    gh, gw = -(-h // step), -(-w // step)
    x = (np.arange(gw) * step).astype(np.float64)[None, :].repeat(gh, 0)
    y = (np.arange(gh) * step).astype(np.float64)[:, None].repeat(gw, 1)
    kinds = ["translation", "similarity", "perspective"]
    mats = np.stack([util.test_matrices(1, w, h, kinds[i % 3], seed=int(rng.integers(0, 1 << 30)))[0] for i in range(pairs)]).astype(np.float32)
    flow = np.empty((pairs, gh, gw, 2), np.float32)
    for i in range(pairs):
        A = mats[i].astype(np.float64)
        W = A[2, 0] * x + A[2, 1] * y + A[2, 2]
        flow[i, ..., 0] = (A[0, 0] * x + A[0, 1] * y + A[0, 2]) / W - x + rng.normal(0, 0.7, (gh, gw)) + 1.5 * np.sin(x / 90.0 + i)
        flow[i, ..., 1] = (A[1, 0] * x + A[1, 1] * y + A[1, 2]) / W - y + rng.normal(0, 0.7, (gh, gw)) + 1.0 * np.cos(y / 70.0 - i)
    # equal values (ties in the rank), NaN / Inf samples
    flow[:, : gh // 2, : gw // 3] = np.round(flow[:, : gh // 2, : gw // 3] * 2) / 2
    bad = rng.random((pairs, gh, gw)) < 0.03
    flow[..., 0][bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    bad = rng.random((pairs, gh, gw)) < 0.02
    flow[..., 1][bad] = np.nan
    return flow, mats, gh, gw


@pytest.mark.parametrize("w,h,verts", [(960, 540, (17, 10)), (480, 270, (17, 10)), (333, 187, (9, 6)), (101, 67, (2, 2)),
                                       (960, 540, (3, 3)), (960, 540, (65, 33)), (960, 960, (3, 3))])
def test_residual_kernel_equals_the_restatement(pkg, ctx, w, h, verts):
    import torch

    rng = np.random.default_rng(w * 7 + h + verts[0])
    step, pairs = 8, 3
    mw, mh = verts
    flow, mats, gh, gw = _draw_field(rng, pairs, w, h, step)
    blocked = (rng.random((pairs + 1, gh, gw)) < 0.1).astype(np.uint8)
    blocked[:, : gh // (mh - 1) + 2, : gw // (mw - 1) + 2] = 1                # vertex (0, 0) loses all of its samples but one
    blocked[:, 0, 0] = 0
    flow[:, 0, 0] = (0.25, -0.25)
    seen = {}
    for blk in (None, blocked):
        want_res, want_cnt = R.mesh_residual(flow, step, (w, h), mats, mw, mh, blk)
        got_res, got_cnt = ctx.mesh_residual_batch(torch.from_numpy(flow).cuda(), step, (w, h), mats, mw, mh,
                                                   blocked=None if blk is None else torch.from_numpy(blk).cuda())
        assert got_cnt.dtype == torch.int32 and got_res.dtype == torch.float32
        assert np.array_equal(got_cnt.cpu().numpy(), want_cnt)
        assert np.array_equal(got_res.cpu().numpy(), want_res)
        assert np.isfinite(want_res).all()
        seen[blk is None] = (want_res, want_cnt)
    assert (seen[True][1] >= R.MIN_SAMPLES).any() and seen[True][0].any()
    res_b, cnt_b = seen[False]
    assert (cnt_b[:, 0, 0] == 1).all() and not res_b[:, 0, 0].any()          # the starved vertex reports 0 and its true count
    # (960x540 with 3 x 3 vertices fills 64 KB of LDS per workgroup, 960x960 with 3 x 3 takes 112.5 KB: both sides of the limit
    # the host has to raise)


def test_residual_kernel_argument_checks(pkg, ctx):
    import torch

    from vstab_amd import native

    g = torch.zeros((2, 5, 8, 2), device="cuda")
    eye = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    with pytest.raises(ValueError, match="vertices outside 2..65"):
        ctx.mesh_residual_batch(g, 8, (64, 40), eye, 1, 4)
    with pytest.raises(ValueError, match="is not a 64x48 image at step 8"):
        ctx.mesh_residual_batch(g, 8, (64, 48), eye, 3, 3)
    with pytest.raises(ValueError, match=r"are not \[2,3,3\]"):
        ctx.mesh_residual_batch(g, 8, (64, 40), eye[:1], 3, 3)
    with pytest.raises(ValueError, match="blocked"):
        ctx.mesh_residual_batch(g, 8, (64, 40), eye, 3, 3, blocked=torch.zeros((2, 5, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(native.VstabError, match="neighbourhood of 19044 grid positions exceeds 16384"):
        ctx.mesh_residual_batch(torch.zeros((1, 138, 138, 2), device="cuda"), 8, (1100, 1100), eye[:1], 3, 3)
    with pytest.raises(ValueError, match=r"offsets .* are not float32 \[2,mh,mw,2\]"):
        ctx.mesh_warp_batch(torch.zeros((2, 8, 8, 3), device="cuda"), eye, (8, 8), np.zeros((3, 4, 4, 2), np.float32))


# ---- 2. zero offsets: the plain warp, in bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("kind,size,out_size", [
    ("similarity", (1920, 1080), (1920, 1080)), ("perspective", (1920, 1080), (1920, 1080)),
    ("similarity", (480, 270), (523, 301)), ("perspective", (333, 187), (333, 187)), ("perspective", (960, 540), (1011, 577)),
    ("horizon", (160, 90), (160, 90)), ("far", (160, 90), (177, 95)), ("similarity", (61, 45), (1100, 20)),
    ("similarity", (61, 45), (333, 11))])   # 11 rows: column blocks of 1024 // 11 = 93 px, neither a power of two nor the whole row
def test_zero_offsets_are_the_plain_warp(pkg, ctx, subpix, kind, size, out_size):
    import torch

    w, h = size
    n = 2 if w >= 1920 else 3
    frames = torch.from_numpy(util.synth_frames(n, h, w, seed=w + h)).cuda()
    mats = util.test_matrices(n, w, h, kind, seed=5).astype(np.float32)
    border = (0.2, 0.4, 0.6)
    want, want_mask, want_cnt = ctx.warp_batch(frames, mats, out_size, interp="bilinear", border=border, subpix=subpix, want_mask=True,
                                               want_count=True)
    for verts in ((17, 10), (2, 2), (65, 65)):
        zero = np.zeros((n, verts[1], verts[0], 2), np.float32)
        got, got_mask, got_cnt = ctx.mesh_warp_batch(frames, mats, out_size, zero, border=border, subpix=subpix, want_mask=True,
                                                     want_count=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, subpix, verts)
        assert torch.equal(got_mask.view(torch.int32), want_mask.view(torch.int32))
        assert torch.equal(got_cnt, want_cnt)
    plain_no_mask = ctx.mesh_warp_batch(frames, mats, out_size, zero, border=border, subpix=subpix, want_mask=False)
    assert plain_no_mask[1] is None and torch.equal(plain_no_mask[0].view(torch.int32), want.view(torch.int32))


# ---- 3. drawn offsets: the restatement, in bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("kind,size,out_size,verts", [("similarity", (320, 180), (320, 180), (17, 10)),
                                                      ("perspective", (213, 121), (240, 140), (9, 6)),
                                                      ("translation", (96, 64), (1100, 24), (2, 2)),
                                                      ("horizon", (120, 80), (120, 80), (5, 4)),
                                                      ("perspective", (96, 64), (333, 11), (3, 3))])   # 93-px column blocks
def test_mesh_warp_equals_the_restatement(pkg, ctx, subpix, kind, size, out_size, verts):
    import torch

    w, h = size
    n = 2
    rng = np.random.default_rng(w + verts[0])
    max_shift = w / 64.0
    frames = util.synth_frames(n, h, w, seed=w)
    mats = util.test_matrices(n, w, h, kind, seed=9).astype(np.float32)
    offsets = rng.uniform(-max_shift, max_shift, (n, verts[1], verts[0], 2)).astype(np.float32)
    border = (0.2, 0.4, 0.6)
    want, want_mask, want_cnt = R.mesh_warp(frames, mats, out_size, offsets, border, subpix)
    got, got_mask, got_cnt = ctx.mesh_warp_batch(torch.from_numpy(frames).cuda(), mats, out_size, offsets, border=border, subpix=subpix,
                                                 want_mask=True, want_count=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (kind, subpix)
    assert np.array_equal(_bits(got_mask.cpu().numpy()), _bits(want_mask))
    assert got_cnt.cpu().numpy().tolist() == want_cnt.tolist()
    plain = ctx.warp_batch(torch.from_numpy(frames).cuda(), mats, out_size, interp="bilinear", border=border, subpix=subpix)[0]
    if kind not in ("horizon",):
        assert not torch.equal(plain, got)                 # the offsets did something


@pytest.mark.parametrize("subpix", ["q5", "exact"])
def test_integer_offset_shifts_the_source(pkg, ctx, subpix):
    import torch

    src = util.synth_frames(1, 40, 64, seed=2)
    off = np.tile(np.float32([5.0, -3.0]), (1, 10, 17, 1))
    got, mask, cnt = ctx.mesh_warp_batch(torch.from_numpy(src).cuda(), np.eye(3, dtype=np.float32)[None], (64, 40), off,
                                         border=(0.1, 0.2, 0.3), subpix=subpix, want_mask=True, want_count=True)
    got, mask = got.cpu().numpy()[0], mask.cpu().numpy()[0]
    assert np.array_equal(got[:37, 5:], src[0, 3:, :59]) and not mask[:37, 5:].any()
    edge = np.float32([0.1, 0.2, 0.3])
    assert (got[37:] == edge).all() and (got[:, :5] == edge).all() and (mask[37:] == 1).all() and (mask[:, :5] == 1).all()
    assert int(cnt[0]) == 64 * 40 - 37 * 59


# ---- 4. it helps -------------------------------------------------------------------------------------------------------
def _final_matrices(meta):
    return np.array([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)


def _interior(masks, radius):
    """Pixels at least `radius` inside mask == 0 (the frame's edge counts as padding): bool [N,H,W] on the device."""
    import torch
    import torch.nn.functional as F

    k = 2 * radius + 1
    padded = F.pad((masks > 0).float()[:, None], (radius,) * 4, value=1.0)
    return F.max_pool2d(padded, k, stride=1)[:, 0] == 0


def _psnr(out, ideal, sel):
    err = ((out - ideal) ** 2).sum(-1)[sel]
    return 10.0 * math.log10(1.0 / (float(err.mean()) / 3.0))


def _static_ideal(final0, n, h, w, device, seed=1234):
    """The locked camera shows frame 0's content, moved by frame 0's matrix (the recentring translation)."""
    import torch

    assert np.array_equal(final0[:2, :2], np.eye(2, dtype=np.float32)) and np.array_equal(final0[2], np.float32([0, 0, 1]))
    yy, xx = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32), torch.arange(w, device=device, dtype=torch.float32),
                            indexing="ij")
    return R.texture(xx - float(final0[0, 2]), yy - float(final0[1, 2]), h, w, seed)


def _analytic_offsets(final, g, e, w, h, mw, mh):
    """The ceiling of the representation: at every vertex v the offset that makes the mesh warp sample where the static
    texture's point lies.  Output p = M_i v shows T(p - t0) in the ideal; frame_i(s) = T(s - D_i(s)), so s solves
    s = (p - t0) + D_i(s) (fixed point, D is a contraction) and c(v) = v - s."""
    vx = np.arange(mw) * (w - 1) / (mw - 1)
    vy = np.arange(mh) * (h - 1) / (mh - 1)
    V = np.stack(np.meshgrid(vx, vy), -1)                       # [mh,mw,2]
    t0 = final[0].astype(np.float64)[:2, 2]
    out = np.empty((len(final), mh, mw, 2), np.float32)
    for i, M in enumerate(final.astype(np.float64)):
        den = M[2, 0] * V[..., 0] + M[2, 1] * V[..., 1] + M[2, 2]
        p = np.stack([(M[0, 0] * V[..., 0] + M[0, 1] * V[..., 1] + M[0, 2]) / den,
                      (M[1, 0] * V[..., 0] + M[1, 1] * V[..., 1] + M[1, 2]) / den], -1) - t0
        s = p.copy()
        for _ in range(8):
            s = p + g[i] + R.ramp(np.clip(s[..., :1], 0, w - 1), w) * e[i]
        out[i] = V - s
    return out


@pytest.mark.parametrize("w,h,seed", [(480, 270, 5), (480, 270, 11), (960, 540, 5)])
def test_it_helps_on_nonrigid_clips(pkg, ctx, w, h, seed):
    import torch

    dev = torch.device("cuda")
    frames, g, e = R.nonrigid_clip(CLIP_FRAMES, h, w, dev, seed=seed)
    none = _stabilize(ctx, frames, args=LOCK_ARGS, mesh_warp=None)
    mesh = _stabilize(ctx, frames, args=LOCK_ARGS, mesh_warp=True)
    final = _final_matrices(none.meta)
    assert np.array_equal(final, _final_matrices(mesh.meta))              # the global part is the same plan
    max_shift = mesh.meta["mesh_warp"]["max_shift"]
    assert max_shift == w / 64.0 and mesh.meta["mesh_warp"]["cells"] == [16, 9]
    ceiling_offsets = np.clip(_analytic_offsets(final, g, e, w, h, 17, 10), -max_shift, max_shift)
    top, top_mask, _ = ctx.mesh_warp_batch(frames, final, (w, h), ceiling_offsets, border=(0.5, 0.5, 0.5), want_mask=True)
    ideal = _static_ideal(final[0], CLIP_FRAMES, h, w, dev)
    sel = _interior(torch.maximum(torch.maximum(none.masks[..., 0], mesh.masks[..., 0]), top_mask), int(math.ceil(max_shift)))
    assert float(sel.float().mean()) > 0.5
    p_none, p_mesh, p_top = _psnr(none.frames, ideal, sel), _psnr(mesh.frames, ideal, sel), _psnr(top, ideal, sel)
    share = (p_mesh - p_none) / (p_top - p_none) if p_top > p_none else float("nan")
    print(f"\nmesh_warp it-helps {w}x{h} seed {seed}: PSNR none {p_none:.2f} dB, mesh {p_mesh:.2f} dB, analytic ceiling {p_top:.2f} dB; "
          f"recovered {p_mesh - p_none:.2f} of {p_top - p_none:.2f} dB ({100 * share:.0f} %); meta {json.dumps(mesh.meta['mesh_warp'])}")
    assert p_mesh > p_none + PSNR_MARGIN_DB, (p_none, p_mesh, p_top)


# ---- 5. it does no harm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [1.0, 3.0])
def test_it_does_no_harm_on_rigid_shake(pkg, ctx, amp):
    import bench
    import torch

    w, h = 480, 270
    dev = torch.device("cuda")
    cam = shake_path(CLIP_FRAMES, w, h, "similarity", seed=3, amp=amp)
    frames = bench.synth_clip(CLIP_FRAMES, 0, h, w, dev, seed=1234, mats=cam)
    none = _stabilize(ctx, frames, args=LOCK_ARGS)
    mesh = _stabilize(ctx, frames, args=LOCK_ARGS, mesh_warp=True)
    final = _final_matrices(none.meta)
    ideal = _static_ideal(final[0], CLIP_FRAMES, h, w, dev)
    sel = _interior(torch.maximum(none.masks[..., 0], mesh.masks[..., 0]), int(math.ceil(mesh.meta["mesh_warp"]["max_shift"])))
    p_none, p_mesh = _psnr(none.frames, ideal, sel), _psnr(mesh.frames, ideal, sel)
    print(f"\nmesh_warp no-harm amp {amp}: PSNR none {p_none:.2f} dB, mesh {p_mesh:.2f} dB, "
          f"correction_px_max {mesh.meta['mesh_warp']['correction_px_max']:.3f}, meta {json.dumps(mesh.meta['mesh_warp'])}")
    assert abs(p_mesh - p_none) <= PSNR_MARGIN_DB, (p_none, p_mesh)


# ---- 6. off means off -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator,framing,mode", [("flow", "crop_and_pad", "similarity"), ("flow", "crop", "similarity"),
                                                    ("flow_tvl1", "expand", "translation"), ("classic", "crop_and_pad", "similarity")])
def test_off_is_off(pkg, ctx, estimator, framing, mode):
    import bench
    import torch

    n = 6 if estimator == "flow_tvl1" else 12
    w, h = (240, 136) if estimator == "flow_tvl1" else (480, 270)
    frames = bench.synth_clip(n, 0, h, w, torch.device("cuda"), mats=shake_path(n, w, h, mode, seed=3))
    ctx.set_timing(True)
    try:
        # one launch of each new kernel, so that both timing kinds exist
        ctx.mesh_residual_batch(torch.zeros((1, 2, 2, 2), device="cuda"), 8, (16, 16), np.eye(3, dtype=np.float32)[None], 2, 2)
        ctx.mesh_warp_batch(torch.zeros((1, 8, 8, 3), device="cuda"), np.eye(3, dtype=np.float32)[None], (8, 8), np.zeros((1, 2, 2, 2), np.float32))
        ctx.set_timing(True)                                   # clears the totals: 0 launches of either kind from here on
        plain = _stabilize(ctx, frames, mode, estimator, framing)
        none = _stabilize(ctx, frames, mode, estimator, framing, mesh_warp=None, mesh_max_shift=None)
        assert ctx.kernel_ms_stats("mesh_residual")[1] == 0 and ctx.kernel_ms_stats("mesh_warp")[1] == 0
        if estimator != "classic" and framing != "crop":
            on = _stabilize(ctx, frames, mode, estimator, framing, mesh_warp=True)
            assert ctx.kernel_ms_stats("mesh_residual")[1] == 1 and ctx.kernel_ms_stats("mesh_warp")[1] == 1
            assert set(on.meta) - set(plain.meta) == {"mesh_warp"} and set(plain.meta) <= set(on.meta)
            assert tuple(on.frames.shape) == tuple(plain.frames.shape)
    finally:
        ctx.set_timing(False)
    assert np.array_equal(_bits(plain.frames.cpu().numpy()), _bits(none.frames.cpu().numpy()))
    assert np.array_equal(_bits(plain.masks.cpu().numpy()), _bits(none.masks.cpu().numpy()))
    assert json.dumps(plain.meta, sort_keys=True) == json.dumps(none.meta, sort_keys=True) and "mesh_warp" not in none.meta
    assert "work_matrices" not in none.meta.get("estimated_motion", {})       # the plan's hand-over to the mesh stays out of meta
    assert plain.device_plan == none.device_plan


# ---- 7. composition --------------------------------------------------------------------------------------------------------
def test_scene_cuts_restart_the_vertex_paths(pkg, ctx, monkeypatch):
    import torch

    from vstab_amd import mesh_warp as mw

    dev = torch.device("cuda")
    a, _, _ = R.nonrigid_clip(10, 270, 480, dev, seed=5)
    b, _, _ = R.nonrigid_clip(8, 270, 480, dev, seed=6, texture_seed=99)
    frames = torch.cat([a, b])
    seen = {}
    real = mw.plan_offsets

    def spy(*args, **kw):
        out = real(*args, **kw)
        seen["offsets"], seen["segments"] = out[0], args[3]
        return out

    monkeypatch.setattr(mw, "plan_offsets", spy)
    res = _stabilize(ctx, frames, args=LOCK_ARGS, scene_cuts=[10], mesh_warp=(8, 5), mesh_max_shift=6.0)
    assert seen["segments"] == [(0, 10), (10, 18)] and seen["offsets"].shape == (18, 6, 9, 2)
    assert not seen["offsets"][0].any() and not seen["offsets"][10].any()            # the first frame of each shot
    assert seen["offsets"][9].any() and seen["offsets"][17].any()
    assert res.meta["scene_cuts"]["cuts"] == [10] and res.meta["mesh_warp"]["cells"] == [8, 5]
    assert res.meta["mesh_warp"]["max_shift"] == 6.0 and res.meta["mesh_warp"]["correction_px_max"] <= 6.0


def test_estimation_mask_composes_and_the_refusals_raise(pkg, ctx):
    import torch

    from vstab_amd import distributed

    frames, _, _ = R.nonrigid_clip(8, 270, 480, torch.device("cuda"), seed=5)
    mask = torch.zeros((270, 480))
    mask[100:170, 200:300] = 1.0
    for estimator, clip in (("flow", frames), ("flow_tvl1", frames[:3, ::2, ::2].contiguous())):
        m = mask if estimator == "flow" else mask[::2, ::2].contiguous()
        res = _stabilize(ctx, clip, estimator=estimator, estimation_mask=m, mesh_warp=True, framing="expand")
        assert res.meta["estimation_mask"]["blocked_fraction_max"] > 0.0 and res.meta["mesh_warp"]["cells"] == [16, 9]
        counts = (res.masks[..., 0] > 0.5).reshape(len(clip), -1).sum(1).cpu().numpy()                   # the mesh warp's own counts
        pixels = np.float32(res.masks.shape[1] * res.masks.shape[2])
        assert res.meta["padding_fraction_max"] == float((counts.astype(np.float32) / pixels).astype(np.float64).max())
    for kw, text in ((dict(estimator="classic"), "no dense grid"), (dict(estimator="flow_phase_correlate"), "no dense grid"),
                     (dict(framing="crop"), "the crop solver bounds matrices only"),
                     (dict(temporal_fill=3), "fill candidates are global matrices")):
        with pytest.raises(ValueError, match=text):
            _stabilize(ctx, frames, mesh_warp=True, **kw)
    with pytest.raises(ValueError, match="the mesh warp is not sharded"):
        distributed.stabilize_sharded(ctx, frames, len(frames), "crop_and_pad", "similarity", *ARGS, mesh_warp=True)


def test_node_equals_the_keyword_call(pkg, ctx):
    import torch

    from vstab_amd import nodes

    frames, _, _ = R.nonrigid_clip(8, 270, 480, torch.device("cuda"), seed=5)
    for cols, rows, shift, kw in ((16, 9, 0.0, dict(mesh_warp=True)), (6, 4, 3.5, dict(mesh_warp=(6, 4), mesh_max_shift=3.5))):
        want = _stabilize(ctx, frames, **kw)
        out = nodes.VideoStabilizerFlowMesh.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F",
                                                    cols, rows, shift)
        node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
        assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
        assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
        assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True)
        assert node_meta["mesh_warp"]["cells"] == [cols, rows]
