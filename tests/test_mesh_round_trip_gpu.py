"""Mesh warp round trip on the GPU (include/vstab.h "vstab_mesh_unwarp_batch"; apply_pipeline.apply_motion(mesh=True)).

  1. all-zero offsets: vstab_mesh_unwarp_batch == vstab_warp_batch in bits (dst, mask, pad_count), nothing unconverged
  2. drawn offsets: == the restatement (tests/mesh_inverse_restatement.py) in bits, the unconverged counts included
  3. a known answer: a constant integer offset shifts the frame the opposite way to the forward mesh warp
  4. end to end, forward: Motion Apply with mesh=True on the source frames reproduces Flow's mesh-warped frames in bits
  5. end to end, inverse: restoring with mesh=True beats the plain restore of the same frames by PSNR_MARGIN_DB
  6. mesh=False on a meta that carries the block is today's result, and launches no mesh kernel

Measured figures: profiles/r12_mesh_round_trip.md.
"""

import json
import math

import numpy as np
import pytest

from tests import mesh_inverse_restatement as RI
from tests import mesh_restatement as R
from tests import util

pytestmark = pytest.mark.gpu

LOCK_ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the largest corrections
PSNR_MARGIN_DB = 1.0          # "meaningfully different", as tests/test_mesh_warp_gpu.py uses it
CLIP_FRAMES = 24
RGB = (127, 127, 127)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


# ---- 1. zero offsets: the plain warp, in bits ---------------------------------------------------------------------------
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
        if verts == (2, 2):
            zero = -zero                                           # zeros of the other sign
        got, got_mask, got_cnt, unconverged = ctx.mesh_unwarp_batch(frames, mats, out_size, zero, border=border, subpix=subpix,
                                                                    want_mask=True, want_count=True, want_unconverged=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, subpix, verts)
        assert torch.equal(got_mask.view(torch.int32), want_mask.view(torch.int32))
        assert torch.equal(got_cnt, want_cnt)
        assert unconverged.dtype == torch.int32 and not unconverged.any()
    no_mask = ctx.mesh_unwarp_batch(frames, mats, out_size, zero, border=border, subpix=subpix, want_mask=False)
    assert no_mask[1] is None and no_mask[2] is None and no_mask[3] is None
    assert torch.equal(no_mask[0].view(torch.int32), want.view(torch.int32))


# ---- 2. drawn offsets: the restatement, in bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("kind,size,out_size,verts", [("similarity", (320, 180), (320, 180), (17, 10)),
                                                      ("perspective", (213, 121), (240, 140), (9, 6)),
                                                      ("translation", (96, 64), (1100, 24), (2, 2)),
                                                      ("perspective", (96, 64), (333, 11), (3, 3)),   # 93-px column blocks
                                                      ("similarity", (160, 90), (160, 90), (65, 65))])
def test_mesh_unwarp_equals_the_restatement(pkg, ctx, subpix, kind, size, out_size, verts):
    """Independent uniform offsets of the full amplitude (1/64 of the canvas the mesh lies over).  At 65 x 65 vertices on
    160 x 90 a cell is 2.5 x 1.4 px wide and the offsets reach +-2.5 px: not a contraction, the restatement reports unconverged
    pixels, and the kernel's counts must equal them."""
    import torch

    w, h = size
    n = 2
    rng = np.random.default_rng(w + verts[0])
    max_shift = out_size[0] / 64.0
    frames = util.synth_frames(n, h, w, seed=w)
    mats = util.test_matrices(n, w, h, kind, seed=9).astype(np.float32)
    offsets = rng.uniform(-max_shift, max_shift, (n, verts[1], verts[0], 2)).astype(np.float32)
    border = (0.2, 0.4, 0.6)
    want, want_mask, want_cnt, want_unc = RI.mesh_unwarp(frames, mats, out_size, offsets, border, subpix)
    got, got_mask, got_cnt, got_unc = ctx.mesh_unwarp_batch(torch.from_numpy(frames).cuda(), mats, out_size, offsets, border=border,
                                                            subpix=subpix, want_mask=True, want_count=True, want_unconverged=True)
    print(f"\nmesh_unwarp {kind} {size}->{out_size} {verts} {subpix}: unconverged {want_unc.tolist()} (kernel {got_unc.cpu().numpy().tolist()})")
    assert got_unc.cpu().numpy().tolist() == want_unc.tolist()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (kind, subpix)
    assert np.array_equal(_bits(got_mask.cpu().numpy()), _bits(want_mask))
    assert got_cnt.cpu().numpy().tolist() == want_cnt.tolist()
    if verts == (65, 65):
        assert want_unc.min() > 0
    plain = ctx.warp_batch(torch.from_numpy(frames).cuda(), mats, out_size, interp="bilinear", border=border, subpix=subpix)[0]
    assert not torch.equal(plain, got)                     # the offsets did something
    # the counts are optional one by one
    only_unc = ctx.mesh_unwarp_batch(torch.from_numpy(frames).cuda(), mats, out_size, offsets, border=border, subpix=subpix,
                                     want_mask=False, want_unconverged=True)
    assert only_unc[3].cpu().numpy().tolist() == want_unc.tolist() and torch.equal(only_unc[0], got)


def test_argument_checks(pkg, ctx):
    import torch

    from vstab_amd import native

    eye = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    src = torch.zeros((2, 8, 8, 3), device="cuda")
    with pytest.raises(ValueError, match=r"mesh_unwarp_batch: offsets .* are not float32 \[2,mh,mw,2\]"):
        ctx.mesh_unwarp_batch(src, eye, (8, 8), np.zeros((3, 4, 4, 2), np.float32))
    with pytest.raises(ValueError, match=r"mesh_unwarp_batch: 66x4 vertices outside 2..65"):
        ctx.mesh_unwarp_batch(src, eye, (8, 8), np.zeros((2, 4, 66, 2), np.float32))
    with pytest.raises(native.VstabError, match=r"vstab_mesh_unwarp_batch: bad size .*the output must be at least 2x2"):
        ctx.mesh_unwarp_batch(src, eye, (8, 1), np.zeros((2, 2, 2, 2), np.float32))
    with pytest.raises(native.VstabError, match=r"vstab_mesh_warp_batch: bad size .*the source must be at least 2x2"):
        ctx.mesh_warp_batch(torch.zeros((2, 1, 8, 3), device="cuda"), eye, (8, 8), np.zeros((2, 2, 2, 2), np.float32))


# ---- 3. a known answer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
def test_integer_offset_shifts_the_frame_the_other_way(pkg, ctx, subpix):
    """The forward mesh warp with c = (5, -3) shows src(x - 5, y + 3) at (x, y) (test_integer_offset_shifts_the_source); its
    inverse shows src(x + 5, y - 3)."""
    import torch

    src = util.synth_frames(1, 40, 64, seed=2)
    off = np.tile(np.float32([5.0, -3.0]), (1, 10, 17, 1))
    got, mask, cnt, unc = ctx.mesh_unwarp_batch(torch.from_numpy(src).cuda(), np.eye(3, dtype=np.float32)[None], (64, 40), off,
                                                border=(0.1, 0.2, 0.3), subpix=subpix, want_mask=True, want_count=True,
                                                want_unconverged=True)
    got, mask = got.cpu().numpy()[0], mask.cpu().numpy()[0]
    assert np.array_equal(got[3:, :59], src[0, :37, 5:]) and not mask[3:, :59].any()
    edge = np.float32([0.1, 0.2, 0.3])
    assert (got[:3] == edge).all() and (got[:, 59:] == edge).all() and (mask[:3] == 1).all() and (mask[:, 59:] == 1).all()
    assert int(cnt[0]) == 64 * 40 - 37 * 59 and int(unc[0]) == 0


# ---- 4. / 5. / 6. end to end ---------------------------------------------------------------------------------------------
def _stabilize(ctx, frames, framing, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, "similarity", *LOCK_ARGS, ctx=ctx, keep_on_device=True,
                                estimator="flow", **kw)


def _apply(ctx, frames, meta, **kw):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    return ap.apply_motion(hm._normalize_video_input(frames), meta, RGB, ctx=ctx, keep_on_device=True, **kw)


@pytest.fixture(scope="module")
def runs(pkg, ctx):
    """One 24-frame 480x270 non-rigid clip, stabilized once per framing with the offsets recorded; shared, never changed."""
    import torch

    frames, _, _ = R.nonrigid_clip(CLIP_FRAMES, 270, 480, torch.device("cuda"), seed=5)
    out = {"frames": frames}
    for framing in ("crop_and_pad", "expand"):
        res = _stabilize(ctx, frames, framing, mesh_warp=True, mesh_motion=True)
        res.meta = json.loads(json.dumps(res.meta))                # what a saved workflow hands on
        out[framing] = res
    return out


def test_mesh_motion_only_adds_the_block(pkg, ctx, runs):
    res = _stabilize(ctx, runs["frames"], "crop_and_pad", mesh_warp=True)
    with_block = runs["crop_and_pad"].meta
    block = with_block["mesh_warp"]["motion"]
    assert block["version"] == 1 and block["domain_size"] == [480, 270] and block["vertices"] == [17, 10]
    assert block["frame_count"] == CLIP_FRAMES and np.asarray(block["offsets"]).shape == (CLIP_FRAMES, 10, 17, 2)
    stripped = json.loads(json.dumps(with_block))
    del stripped["mesh_warp"]["motion"]
    assert json.dumps(stripped, sort_keys=True) == json.dumps(res.meta, sort_keys=True)       # False: today's meta
    assert np.abs(np.asarray(block["offsets"])).max() == with_block["mesh_warp"]["correction_px_max"]


@pytest.mark.parametrize("framing", ["crop_and_pad", "expand"])
def test_forward_replay_reproduces_flow(pkg, ctx, runs, framing):
    """Flow under either framing, replayed from its meta on the source frames: the matrices are replayed as recorded
    (crop_and_pad keeps the recorded canvas, which for an expand run is the expanded one), so the bits are Flow's."""
    import torch

    run = runs[framing]
    got = _apply(ctx, runs["frames"], run.meta, framing_mode="crop_and_pad", mesh=True)
    assert got.meta["motion_apply"]["mesh"] == {"direction": "forward", "unconverged_max": 0}
    assert tuple(got.frames.shape) == tuple(run.frames.shape)
    assert torch.equal(got.frames.view(torch.int32), run.frames.view(torch.int32))
    assert torch.equal(got.masks.view(torch.int32), run.masks.view(torch.int32))
    assert not torch.equal(_apply(ctx, runs["frames"], run.meta, framing_mode="crop_and_pad").frames, run.frames)   # the mesh matters


def test_forward_replay_under_expand_framing(pkg, ctx, runs):
    """Motion Apply's own `expand` framing of a crop_and_pad run: its matrices moved onto the canvas that holds every frame,
    the mesh unchanged (it lies over the source) -- the mesh warp of exactly those matrices."""
    import torch

    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm
    from vstab_amd import mesh_warp as mw

    run = runs["crop_and_pad"]
    got = _apply(ctx, runs["frames"], run.meta, framing_mode="expand", mesh=True)
    mats = [np.asarray(e["matrix"], np.float64) for e in run.meta["motion_meta"]["per_frame"]]
    expanded, size = ap._expand_matrices(mats, (480, 270))
    assert got.meta["motion_apply"]["output_size"] == [size[0], size[1]] and tuple(size) != (480, 270)
    want, want_mask, _ = ctx.mesh_warp_batch(runs["frames"], np.stack(expanded).astype(np.float32), size,
                                             mw.parse_motion_block(run.meta).offsets, border=hm.border_value(RGB), want_mask=True)
    assert torch.equal(got.frames.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.masks[..., 0].view(torch.int32), want_mask.view(torch.int32))


def _interior(masks, radius):
    """Pixels at least `radius` inside mask == 0 (the frame's edge counts as padding): bool [N,H,W] on the device."""
    import torch.nn.functional as F

    k = 2 * radius + 1
    padded = F.pad((masks > 0).float()[:, None], (radius,) * 4, value=1.0)
    return F.max_pool2d(padded, k, stride=1)[:, 0] == 0


def _psnr(out, ideal, sel):
    err = ((out - ideal) ** 2).sum(-1)[sel]
    return 10.0 * math.log10(1.0 / (float(err.mean()) / 3.0))


@pytest.mark.parametrize("framing", ["crop_and_pad", "expand"])
def test_inverse_restores_better_than_the_plain_inverse(pkg, ctx, runs, framing):
    """Measured (480x270, seed 5): see profiles/r12_mesh_round_trip.md."""
    import torch

    run = runs[framing]
    meta = {k: v for k, v in run.meta.items() if k != "motion_meta"}           # what the Inverse node hands on
    mesh = _apply(ctx, run.frames, meta, mesh=True)
    plain = _apply(ctx, run.frames, meta)
    info = mesh.meta["motion_apply"]["mesh"]
    assert info["direction"] == "inverse" and info["unconverged_max"] >= 0
    assert tuple(mesh.frames.shape) == tuple(runs["frames"].shape)
    radius = int(math.ceil(run.meta["mesh_warp"]["max_shift"])) + 2
    sel = _interior(torch.maximum(mesh.masks[..., 0], plain.masks[..., 0]), radius)
    assert float(sel.float().mean()) > 0.5
    p_mesh, p_plain = _psnr(mesh.frames, runs["frames"], sel), _psnr(plain.frames, runs["frames"], sel)
    print(f"\nmesh round trip {framing}: restored with mesh=True {p_mesh:.2f} dB, plain restore {p_plain:.2f} dB "
          f"(unconverged_max {info['unconverged_max']}, interior {float(sel.float().mean()):.2f}, correction_px_max {run.meta['mesh_warp']['correction_px_max']:.2f})")
    assert p_mesh >= p_plain + PSNR_MARGIN_DB, (p_mesh, p_plain)


def test_mesh_false_is_todays_result(pkg, ctx, runs):
    import torch

    run = runs["crop_and_pad"]
    bare = json.loads(json.dumps(run.meta))
    del bare["mesh_warp"]["motion"]
    ctx.set_timing(True)
    try:
        # one launch of each mesh kernel, so that both timing kinds exist
        eye, z = np.eye(3, dtype=np.float32)[None], np.zeros((1, 2, 2, 2), np.float32)
        ctx.mesh_warp_batch(torch.zeros((1, 8, 8, 3), device="cuda"), eye, (8, 8), z)
        ctx.mesh_unwarp_batch(torch.zeros((1, 8, 8, 3), device="cuda"), eye, (8, 8), z)
        assert ctx.kernel_ms_stats("mesh_unwarp")[1] == 1
        ctx.set_timing(True)                                   # clears the totals
        for frames, drop in ((runs["frames"], ()), (run.frames, ("motion_meta",))):
            with_block = {k: v for k, v in run.meta.items() if k not in drop}
            without = {k: v for k, v in bare.items() if k not in drop}
            got = _apply(ctx, frames, with_block, mesh=False)
            default = _apply(ctx, frames, with_block)
            want = _apply(ctx, frames, without)
            for other in (default, want):
                assert torch.equal(got.frames.view(torch.int32), other.frames.view(torch.int32))
                assert torch.equal(got.masks.view(torch.int32), other.masks.view(torch.int32))
            assert "mesh" not in got.meta["motion_apply"] and got.meta["motion_apply"] == want.meta["motion_apply"]
        assert ctx.kernel_ms_stats("mesh_warp")[1] == 0 and ctx.kernel_ms_stats("mesh_unwarp")[1] == 0
        assert ctx.kernel_ms_stats("warp")[1] >= 6
    finally:
        ctx.set_timing(False)


def test_nodes_equal_the_keyword_calls(pkg, ctx, runs):
    from vstab_amd import nodes

    def unpack(out):
        return out.result if hasattr(out, "result") else out.args

    short = runs["frames"][:8].contiguous()
    want = _stabilize(ctx, short, "crop_and_pad", mesh_warp=(6, 4), mesh_max_shift=3.5, mesh_motion=True)
    frames, mask, meta = unpack(nodes.VideoStabilizerFlowMeshMotion.execute(short.cpu(), 16.0, "crop_and_pad", "similarity", True, 1.0, 0.5,
                                                                            0.6, "#7F7F7F", 6, 4, 3.5))
    assert np.array_equal(_bits(frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
    assert json.dumps(meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True) and meta["mesh_warp"]["motion"]["vertices"] == [7, 5]
    back = {k: v for k, v in meta.items() if k != "motion_meta"}
    for clip, m, direction in ((short, meta, "forward"), (frames, back, "inverse")):
        ref = _apply(ctx, clip, m, mesh=True)
        got_frames, got_mask, got_meta = unpack(nodes.VideoStabilizerMotionApplyMesh.execute(clip.cpu(), m, "crop_and_pad", "#7F7F7F"))
        assert got_meta["motion_apply"]["mesh"]["direction"] == direction
        assert np.array_equal(_bits(got_frames.cpu().numpy()), _bits(ref.frames.cpu().numpy()))
        assert np.array_equal(_bits(got_mask.cpu().numpy()), _bits(ref.masks[..., 0].cpu().numpy()))
