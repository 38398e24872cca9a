"""Dynamic zoom on the GPU (include/vstab.h "vstab_cover_extent_batch"; flow_pipeline._stabilize_frames(dynamic_zoom=...)).

  1. the kernel == the restatement (tests/dynamic_zoom_restatement.py) exactly: canvases at the tile's edges, even and odd
     sizes, a canvas wider than one column block from a source of another size; identity, nothing covered, a half-pixel
     shift, rotation + scale, a horizon inside the canvas, NaN, singular; n = 1 and n = 5; both subpix modes; mesh offsets
  2. parity with the warp itself, no restatement involved: e reduced over the mask warp_batch / mesh_warp_batch return
  3. argument errors come before any launch
  4. end to end: None is today's call; with the keyword no frame keeps padding, the mean zoom stays below the static one, the
     frames are the warp of the meta's matrices and Motion Apply replays them; a binding limit, scene cuts, mesh warp
"""

import json

import numpy as np
import pytest

from tests import dynamic_zoom_restatement as R
from tests.util import similarity, test_matrices as util_matrices

pytestmark = pytest.mark.gpu

SENTINEL = R.SENTINEL
# (out_w, out_h), (src_w, src_h): the 64 x 8 tile exactly, one pixel over it on both axes, two and a bit tiles across and a
# short one down, and a canvas wider than one column block (1024 / 16 = 64 columns) from a source of another size
SHAPES = [((64, 8), (64, 8)), ((65, 9), (65, 9)), ((130, 7), (130, 7)), ((200, 37), (96, 54))]
SHAPE_IDS = ["64x8", "65x9", "130x7", "200x37_from_96x54"]


def _cover_all(src, out):
    """The source stretched over the canvas enlarged 1.5 x about its centre: every pixel covered."""
    (sw, sh), (ow, oh) = src, out
    return np.array([[1.5 * ow / sw, 0.0, -0.25 * ow], [0.0, 1.5 * oh / sh, -0.25 * oh], [0.0, 0.0, 1.0]])


def _matrices(src, out):
    (sw, sh), (ow, oh) = src, out
    fit = np.array([[ow / sw, 0.0, 0.0], [0.0, oh / sh, 0.0], [0.0, 0.0, 1.0]])      # source onto canvas, edge to edge
    nan = np.eye(3)
    nan[0, 1] = np.nan
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    horizon = util_matrices(2, ow, oh, "horizon")
    return {
        "identity": np.eye(3),
        "cover_all": _cover_all(src, out),
        "nothing_covered": similarity(3.0 * ow + 1000.0, 0.0, 0.0, 1.0),
        "half_pixel": similarity(0.5, 0.5, 0.0, 1.0) @ fit,
        "minus_half_pixel": similarity(-0.5, -1.5, 0.0, 1.0) @ fit,
        "rotation_scale": similarity(1.7, -0.6, 0.21, 0.83, ow / 2, oh / 2) @ fit,
        "horizon_a": horizon[0] @ fit,
        "horizon_b": horizon[1] @ fit,
        "nan": nan,
        "singular": singular,
        "zeros": np.zeros((3, 3)),
    }


# ---- 1. the kernel equals the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("out,src", SHAPES, ids=SHAPE_IDS)
def test_kernel_equals_restatement(ctx, out, src, subpix):
    cases = _matrices(src, out)
    names = list(cases)
    mats = np.stack([cases[k] for k in names]).astype(np.float32)
    want = R.cover_extent(mats, src, out, subpix=subpix)
    got = ctx.cover_extent_batch(mats, src, out, subpix=subpix)
    assert got.dtype == np.uint32 and got.shape == (len(names),)
    assert got.tolist() == want.tolist(), dict(zip(names, zip(got.tolist(), want.tolist())))
    by = dict(zip(names, got.tolist()))
    assert by["cover_all"] == SENTINEL
    if src == out:
        assert by["identity"] == SENTINEL
    ow, oh = out
    centre = max((ow - 1) % 2 * (oh - 1), (oh - 1) % 2 * (ow - 1))            # 0 for odd x odd
    assert by["nothing_covered"] == centre and by["nan"] == centre
    assert 0 < by["rotation_scale"] < (ow - 1) * (oh - 1)
    # n = 1: every case alone lands in slot 0
    for k, name in enumerate(names):
        assert ctx.cover_extent_batch(mats[k:k + 1], src, out, subpix=subpix).tolist() == [int(want[k])], name


@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("out,src", SHAPES, ids=SHAPE_IDS)
def test_five_frames_each_minimum_in_its_own_slot(ctx, out, src, subpix):
    """n = 5 with a different extent per frame, one fully covered frame between two that are not."""
    (sw, sh), (ow, oh) = src, out
    full = _cover_all(src, out)
    fit = np.array([[ow / sw, 0.0, 0.0], [0.0, oh / sh, 0.0], [0.0, 0.0, 1.0]])      # source onto canvas, edge to edge
    mats = np.stack([similarity(0.07 * ow, 0.0, 0.0, 1.0) @ fit, similarity(0.0, 0.30 * oh, 0.0, 1.0) @ fit, full,
                     similarity(-0.4 * ow, -0.1 * oh, 0.0, 1.0) @ fit, similarity(0.3 * ow, -0.2 * oh, 0.1, 1.0) @ fit]).astype(np.float32)
    want = R.cover_extent(mats, src, out, subpix=subpix)
    got = ctx.cover_extent_batch(mats, src, out, subpix=subpix)
    assert got.tolist() == want.tolist()
    assert got[2] == SENTINEL and got[1] != SENTINEL and got[3] != SENTINEL and len(set(got.tolist())) == 5
    assert ctx.cover_extent_batch(mats[::-1].copy(), src, out, subpix=subpix).tolist() == want[::-1].tolist()


def _smooth_field(n, mw, mh, amp, seed):
    return R.smooth_offsets(n, mw, mh, amp=amp, seed=seed)


@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("out,src", [SHAPES[1], SHAPES[3]], ids=[SHAPE_IDS[1], SHAPE_IDS[3]])
def test_mesh_offsets(ctx, out, src, subpix):
    cases = _matrices(src, out)
    names = ["identity", "cover_all", "half_pixel", "rotation_scale", "horizon_a", "nan", "singular"]
    mats = np.stack([cases[k] for k in names]).astype(np.float32)
    n = len(names)
    plain = ctx.cover_extent_batch(mats, src, out, subpix=subpix)
    # all-zero offsets: the plain entry's result, bit for bit
    for mw, mh in ((2, 2), (17, 10)):
        assert ctx.cover_extent_batch(mats, src, out, np.zeros((n, mh, mw, 2), np.float32), subpix=subpix).tolist() == plain.tolist()
    # a smooth non-zero field on 17 x 10 and on 2 x 2 vertices: the restatement
    for (mw, mh), amp in (((17, 10), 2.5), ((2, 2), 3.0), ((65, 65), 1.0)):
        off = _smooth_field(n, mw, mh, amp, seed=mw)
        want = R.cover_extent(mats, src, out, off, subpix=subpix)
        got = ctx.cover_extent_batch(mats, src, out, off, subpix=subpix)
        assert got.tolist() == want.tolist(), (mw, mh, dict(zip(names, zip(got.tolist(), want.tolist()))))
        assert got.tolist() != plain.tolist()                                  # the field matters


# ---- 2. parity with the warp itself ----------------------------------------------------------------------------------------
def _extent_of_device_masks(ctx, mask, out):
    import torch

    e = torch.from_numpy(R.extent_measure(out)).to(mask.device)                # int64 [h,w]
    big = torch.full_like(e, SENTINEL)
    return torch.where(mask == 1.0, e[None], big[None]).reshape(mask.shape[0], -1).min(dim=1).values.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("out,src", SHAPES, ids=SHAPE_IDS)
def test_parity_with_the_warps_own_mask(ctx, out, src, subpix):
    import torch

    cases = _matrices(src, out)
    mats = np.stack(list(cases.values())).astype(np.float32)
    n = len(mats)
    frames = torch.rand((n, src[1], src[0], 3), device=ctx.device)
    _, mask, _ = ctx.warp_batch(frames, mats, out, subpix=subpix)
    assert ctx.cover_extent_batch(mats, src, out, subpix=subpix).tolist() == _extent_of_device_masks(ctx, mask, out).tolist()
    off = _smooth_field(n, 17, 10, 2.5, seed=4)
    _, mask, _ = ctx.mesh_warp_batch(frames, mats, out, off, subpix=subpix)
    assert ctx.cover_extent_batch(mats, src, out, off, subpix=subpix).tolist() == _extent_of_device_masks(ctx, mask, out).tolist()


# ---- 3. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch(pkg, ctx):
    from vstab_amd import native

    eye = np.eye(3, dtype=np.float32)[None]
    ctx.set_timing(True)
    try:
        assert ctx.cover_extent_batch(eye, (8, 8), (8, 8)).tolist() == [SENTINEL]     # so that the timing kind exists
        ctx.set_timing(True)                                                       # clears the totals
        for out in ((1, 8), (8, 1), (0, 0)):
            with pytest.raises(native.VstabError, match="vstab_cover_extent_batch: a .* canvas has no centred extent"):
                ctx.cover_extent_batch(eye, (8, 8), out)
        with pytest.raises(native.VstabError, match="vstab_cover_extent_batch: .*does not fit the 32-bit extent"):
            ctx.cover_extent_batch(eye, (8, 8), (46342, 46342))
        with pytest.raises(native.VstabError, match="vstab_cover_extent_batch: non-positive size"):
            ctx.cover_extent_batch(eye[:0], (8, 8), (8, 8))
        with pytest.raises(native.VstabError, match="vstab_cover_extent_batch: source larger than 32767"):
            ctx.cover_extent_batch(eye, (40000, 8), (8, 8))
        with pytest.raises(native.VstabError, match="vstab_cover_extent_batch: .*the source must be at least 2x2"):
            ctx.cover_extent_batch(eye, (1, 8), (8, 8), np.zeros((1, 2, 2, 2), np.float32))
        with pytest.raises(ValueError):
            ctx.cover_extent_batch(eye, (8, 8), (8, 8), np.zeros((1, 1, 2, 2), np.float32))      # one row of vertices
        with pytest.raises(ValueError):
            ctx.cover_extent_batch(eye, (8, 8), (8, 8), np.zeros((2, 2, 2, 2), np.float32))      # offsets of two frames
        with pytest.raises(KeyError):
            ctx.cover_extent_batch(eye, (8, 8), (8, 8), subpix="q6")
        assert ctx.kernel_ms_stats("cover_extent")[1] == 0
    finally:
        ctx.set_timing(False)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
W, H, N = R.CLIP_W, R.CLIP_H, R.CLIP_N
RGB = (127, 127, 127)
ARGS = (True, 1.0, 0.5, 0.6, RGB, 16.0)      # camera_lock + strength 1 at 16 fps: dynamic_zoom=0.5 is r = 4 frames


def _stabilize(ctx, frames, framing="crop_and_pad", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, "similarity", *ARGS, ctx=ctx, keep_on_device=True,
                                estimator="flow", **kw)


def _bits_equal(a, b):
    import torch

    return tuple(a.shape) == tuple(b.shape) and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _applied(meta):
    return np.asarray([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)


@pytest.fixture(scope="module")
def clip(ctx):
    """About 24 frames at 160 x 90: a calm move with one burst of strong shake (frames 10..13); shared, never changed."""
    import torch

    import bench

    return bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=R.camera_path())


@pytest.fixture(scope="module")
def zoomed(pkg, ctx, clip):
    return _stabilize(ctx, clip, dynamic_zoom=0.5)


def test_none_is_the_call_without_the_keyword(pkg, ctx, clip):
    ctx.set_timing(True)
    try:
        ctx.cover_extent_batch(np.eye(3, dtype=np.float32)[None], (8, 8), (8, 8))    # so that the timing kind exists
        ctx.set_timing(True)                                                      # clears the totals
        plain = _stabilize(ctx, clip)
        off = _stabilize(ctx, clip, dynamic_zoom=None, zoom_limit=None)
        assert ctx.kernel_ms_stats("cover_extent")[1] == 0                        # nothing new is launched
        on = _stabilize(ctx, clip, dynamic_zoom=0.5)
        assert ctx.kernel_ms_stats("cover_extent")[1] == 1                        # one launch per clip
    finally:
        ctx.set_timing(False)
    assert _bits_equal(off.frames, plain.frames) and _bits_equal(off.masks, plain.masks)
    assert json.dumps(off.meta) == json.dumps(plain.meta) and "dynamic_zoom" not in off.meta
    assert off.device_plan["used"] and not on.device_plan["used"]                 # zoom calls form the plan on the host
    assert plain.meta["padding_fraction_max"] > 0                                 # the clip does leave padding without the zoom


def test_zoom_hides_every_border_and_keeps_field_of_view(pkg, ctx, clip, zoomed):
    meta = zoomed.meta
    block = meta["dynamic_zoom"]
    assert json.loads(json.dumps(block)) == block
    assert list(block) == ["version", "window_s", "radius_frames", "zoom_limit", "margin_px", "zoom_required", "zoom", "zoom_mean",
                           "zoom_max", "static_zoom", "frames_capped", "frames_with_padding"]
    assert (block["version"], block["window_s"], block["radius_frames"], block["zoom_limit"], block["margin_px"]) == (1, 0.5, 4, 2.0, 2)
    z, z_req = np.asarray(block["zoom"]), np.asarray(block["zoom_required"])
    assert z.shape == z_req.shape == (N,)
    print(f"\ndynamic zoom: zoom_mean {block['zoom_mean']:.4f} static_zoom {block['static_zoom']:.4f} zoom_max {block['zoom_max']:.4f} "
          f"padding_fraction_max {meta['padding_fraction_max']} frames_with_padding {block['frames_with_padding']}")
    assert meta["padding_fraction_max"] == 0 and meta["padding_fraction_mean"] == 0
    assert block["frames_with_padding"] == 0 and block["frames_capped"] == 0
    assert float(zoomed.masks.max()) == 0.0
    assert np.all(z >= z_req)
    assert block["zoom_mean"] < block["static_zoom"] == z_req.max()               # the point of the feature
    assert block["zoom_max"] <= block["zoom_limit"] and block["zoom_max"] == z.max() and block["zoom_mean"] == float(z.mean())
    assert block["static_zoom"] > 1.05                                            # the burst asks for a real zoom
    assert meta["framing"]["mode"] == "crop_and_pad" and tuple(zoomed.frames.shape) == (N, H, W, 3)


def test_frames_are_the_warp_of_the_metas_matrices(pkg, ctx, clip, zoomed):
    from vstab_amd import dynamic_zoom as dz
    from vstab_amd import host_math as hm

    plain = _stabilize(ctx, clip)
    applied = _applied(zoomed.meta)
    # the meta's matrices are Z @ (the unzoomed plan's), in float32
    Z = dz.zoom_matrices(zoomed.meta["dynamic_zoom"]["zoom"], (W, H))
    assert np.array_equal(applied.view(np.uint32), np.matmul(Z, _applied(plain.meta)).view(np.uint32))
    # and the zoom is what the kernel's extents of the unzoomed plan ask for
    extent = ctx.cover_extent_batch(_applied(plain.meta), (W, H), (W, H))
    assert extent.tolist() == R.cover_extent(_applied(plain.meta), (W, H), (W, H)).tolist()
    assert zoomed.meta["dynamic_zoom"]["zoom_required"] == dz.required_zoom(extent, (W, H)).tolist()
    dst, mask, _ = ctx.warp_batch(clip, applied, (W, H), interp="bilinear", border=hm.border_value(RGB))
    assert _bits_equal(dst, zoomed.frames) and _bits_equal(mask, zoomed.masks[..., 0])
    assert not _bits_equal(zoomed.frames, plain.frames)


def test_motion_apply_replays_the_zoomed_frames(pkg, ctx, clip, zoomed):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    meta = json.loads(json.dumps(zoomed.meta))                                    # what a saved workflow hands on
    got = ap.apply_motion(hm._normalize_video_input(clip), {"motion_meta": meta["motion_meta"]}, RGB, ctx=ctx, keep_on_device=True)
    assert _bits_equal(got.frames, zoomed.frames)


def test_a_binding_limit_reports_what_is_left(pkg, ctx, clip, zoomed):
    capped = _stabilize(ctx, clip, dynamic_zoom=0.5, zoom_limit=1.02)
    block, free = capped.meta["dynamic_zoom"], zoomed.meta["dynamic_zoom"]
    assert block["zoom_limit"] == 1.02 and block["zoom_required"] == free["zoom_required"] and block["static_zoom"] == free["static_zoom"]
    assert block["frames_capped"] == int(np.count_nonzero(np.asarray(block["zoom_required"]) > 1.02)) > 0
    assert block["zoom_max"] == 1.02 and max(block["zoom"]) == 1.02
    padded = (capped.masks[..., 0] > 0.5).reshape(N, -1).sum(dim=1).cpu().numpy()
    assert block["frames_with_padding"] == int(np.count_nonzero(padded)) > 0
    assert capped.meta["padding_fraction_max"] > 0 and capped.meta["framing"]["padding_detected"]
    # frames whose zoom still reaches what they need keep none
    ok = np.asarray(block["zoom"]) >= np.asarray(block["zoom_required"])
    assert np.all(padded[ok] == 0)
    # the fills see the zoomed result: what the cap leaves is filled
    filled = _stabilize(ctx, clip, dynamic_zoom=0.5, zoom_limit=1.02, spatial_fill=True)
    assert filled.meta["dynamic_zoom"] == block and filled.meta["spatial_fill"]["frames_filled"] == block["frames_with_padding"]


def test_scene_cuts_restart_the_envelope(pkg, ctx):
    """Two shots cut at frame 12.  Framing stays global under scene cuts (one common region for the clip), so shot 1 is a
    wide sweep -- a figure of eight of 10 x 5 px, a few pixels per frame, to both sides of where it starts on both axes --
    that owns every extreme of that region; shot 2 is calm in one run and shakes by 1.5 px right behind the cut in the other:
    shot 1's zoom is the same list of numbers."""
    import torch

    import bench

    dev = torch.device("cuda")
    cut = 12
    shot1 = bench.synth_clip(cut, 0, H, W, dev, mats=R.scene_shot1_path(cut))
    runs = []
    for variant in (0, 1):
        shot2 = bench.synth_clip(N - cut, 0, H, W, dev, seed=99, mats=R.scene_shot2_path(N - cut, variant))
        runs.append(_stabilize(ctx, torch.cat([shot1, shot2]).contiguous(), scene_cuts=[cut], dynamic_zoom=0.5))
    a, b = (r.meta["dynamic_zoom"] for r in runs)
    assert runs[0].meta["scene_cuts"]["cuts"] == [cut]
    print(f"\nscene cuts: center_offset {[r.meta['framing']['center_offset'] for r in runs]}\n  required a {np.round(a['zoom_required'], 4).tolist()}"
          f"\n  required b {np.round(b['zoom_required'], 4).tolist()}")
    assert runs[0].meta["framing"]["center_offset"] == runs[1].meta["framing"]["center_offset"]     # shot 1 owns the common region
    assert a["zoom"][:cut] == b["zoom"][:cut] and a["zoom_required"][:cut] == b["zoom_required"][:cut]
    assert a["zoom"][cut:] != b["zoom"][cut:] and max(b["zoom_required"][cut:cut + 4]) > max(a["zoom_required"][cut:cut + 4])
    # each shot is enveloped as a clip of its own
    from vstab_amd import dynamic_zoom as dz

    for blk in (a, b):
        assert blk["zoom"] == dz.envelope(blk["zoom_required"], 4, 2.0, [(0, cut), (cut, N)]).tolist()
        assert blk["zoom"] != dz.envelope(blk["zoom_required"], 4, 2.0).tolist()
        assert blk["frames_with_padding"] == 0


def test_mesh_warp_composes(pkg, ctx, clip):
    from vstab_amd import host_math as hm

    run = _stabilize(ctx, clip, mesh_warp=True, mesh_motion=True, dynamic_zoom=0.5)
    meta = run.meta
    block = meta["dynamic_zoom"]
    offsets = np.asarray(meta["mesh_warp"]["motion"]["offsets"], np.float32)
    assert offsets.shape == (N, 10, 17, 2)
    applied = _applied(meta)
    dst, mask, counts = ctx.mesh_warp_batch(clip, applied, (W, H), offsets, border=hm.border_value(RGB), want_count=True)
    assert _bits_equal(dst, run.frames) and _bits_equal(mask, run.masks[..., 0])
    # under a mesh the padding that is left is reported, not promised
    assert block["frames_with_padding"] == int(np.count_nonzero(counts.cpu().numpy()))
    assert np.all(np.asarray(block["zoom"]) >= np.asarray(block["zoom_required"])) and block["zoom_mean"] < block["static_zoom"]
    # the extents are those of the mesh warp of the unzoomed plan: the same offsets (the displacement lives in source
    # coordinates), the matrices with the zoom taken off again
    bare = _stabilize(ctx, clip, mesh_warp=True, mesh_motion=True)
    assert np.array_equal(np.asarray(bare.meta["mesh_warp"]["motion"]["offsets"], np.float32), offsets)
    extent = ctx.cover_extent_batch(_applied(bare.meta), (W, H), (W, H), offsets)
    assert extent.tolist() == R.cover_extent(_applied(bare.meta), (W, H), (W, H), offsets).tolist()
    from vstab_amd import dynamic_zoom as dz

    assert block["zoom_required"] == dz.required_zoom(extent, (W, H)).tolist()


@pytest.mark.parametrize("estimator", ["flow_tvl1", "classic", "flow_phase_correlate"])
def test_other_estimators_and_fills_compose(pkg, ctx, clip, estimator):
    """The other three estimators, with a cap that binds so that padding is left for the fills: temporal fill and the
    stability report are fed the ZOOMED plan -- the call with temporal_fill equals the fill run by hand on the outputs of the
    call without it, with the zoomed matrices its meta holds -- and the default window composes as well."""
    from vstab_amd import dynamic_zoom as dz
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm
    from vstab_amd import temporal_fill as tf

    def run(**kw):
        return fp._stabilize_frames(hm._normalize_video_input(clip), "crop_and_pad", "similarity", *ARGS, ctx=ctx, keep_on_device=True,
                                    estimator=estimator, **kw)

    bare = run()
    warped = run(dynamic_zoom=0.5, zoom_limit=1.02)
    filled = run(dynamic_zoom=0.5, zoom_limit=1.02, temporal_fill=2, stability_report=True)
    block = warped.meta["dynamic_zoom"]
    assert filled.meta["dynamic_zoom"] == block and block["frames_capped"] > 0 and block["frames_with_padding"] > 0
    # the applied matrices are the zoomed ones, and the zoom is what the unzoomed plan's extents ask for
    Z = dz.zoom_matrices(block["zoom"], (W, H))
    assert np.array_equal(_applied(filled.meta).view(np.uint32), np.matmul(Z, _applied(bare.meta)).view(np.uint32))
    assert block["zoom_required"] == dz.required_zoom(ctx.cover_extent_batch(_applied(bare.meta), (W, H), (W, H)), (W, H)).tolist()
    # temporal fill by hand on the unfilled outputs, from the meta's (zoomed) matrices
    plan = tf.plan_from_meta(json.loads(json.dumps(warped.meta)))
    dst, mask = warped.frames.clone(), warped.masks[..., 0].clone()
    want = tf.fill_on_device(ctx, clip, dst, mask, plan["final_matrices"], plan["transitions"], plan["confidences"], 2)
    assert filled.meta["temporal_fill"] == want and want["filled_fraction_max"] > 0
    assert _bits_equal(dst, filled.frames) and _bits_equal(mask, filled.masks[..., 0])
    assert not _bits_equal(filled.frames, warped.frames)
    # ... and not the unzoomed ones: the same fill from the plan without the zoom gives other pixels
    unzoomed = tf.plan_from_meta(json.loads(json.dumps(bare.meta)))
    dst2, mask2 = warped.frames.clone(), warped.masks[..., 0].clone()
    tf.fill_on_device(ctx, clip, dst2, mask2, unzoomed["final_matrices"], unzoomed["transitions"], unzoomed["confidences"], 2)
    assert not _bits_equal(dst2, filled.frames)
    assert filled.meta["stability"]["after"]["pairs"] == N - 1
    # the default window: r = 16 frames at 16 fps
    wide = run(dynamic_zoom=True)
    blk = wide.meta["dynamic_zoom"]
    assert blk["window_s"] == 2.0 and blk["radius_frames"] == 16 and blk["zoom_limit"] == 2.0
    assert blk["zoom_required"] == dz.required_zoom(ctx.cover_extent_batch(_applied(bare.meta), (W, H), (W, H)), (W, H)).tolist()
    assert np.all(np.asarray(blk["zoom"]) >= np.minimum(blk["zoom_required"], 2.0))
    uncapped = np.asarray(blk["zoom"]) >= np.asarray(blk["zoom_required"])
    padded = (wide.masks[..., 0] > 0.5).reshape(N, -1).sum(dim=1).cpu().numpy()
    assert np.all(padded[uncapped] == 0) and blk["frames_with_padding"] == int(np.count_nonzero(padded))


def test_refusals_come_before_any_gpu_work(pkg, ctx, clip):
    from vstab_amd import distributed

    eye = np.eye(3, dtype=np.float32)[None]
    ctx.set_timing(True)
    try:
        ctx.cover_extent_batch(eye, (8, 8), (8, 8))                                # so that both timing kinds exist
        ctx.warp_batch(clip[:1], eye, (W, H))
        ctx.set_timing(True)                                                       # clears the totals
        with pytest.raises(ValueError, match="framing_mode 'crop': crop framing already has no padding"):
            _stabilize(ctx, clip, "crop", dynamic_zoom=0.5)
        with pytest.raises(ValueError, match="framing_mode 'expand': an expand canvas has no frame to fill"):
            _stabilize(ctx, clip, "expand", dynamic_zoom=True)
        with pytest.raises(ValueError, match="dynamic_zoom=0"):
            _stabilize(ctx, clip, dynamic_zoom=0)
        with pytest.raises(ValueError, match="zoom_limit=0.5"):
            _stabilize(ctx, clip, dynamic_zoom=True, zoom_limit=0.5)
        with pytest.raises(ValueError, match="dynamic zoom is not sharded"):
            distributed.stabilize_sharded(ctx, clip, N, "crop_and_pad", "similarity", *ARGS, dynamic_zoom=0.5)
        for kind in ("cover_extent", "warp"):
            assert ctx.kernel_ms_stats(kind)[1] == 0
    finally:
        ctx.set_timing(False)


def test_node(pkg, ctx, clip, zoomed):
    from vstab_amd import nodes

    out = nodes.VideoStabilizerFlowZoom.execute(clip.cpu(), 16.0, "similarity", True, 1.0, 0.5, 0.6, "#7F7F7F", 0.5, 2.0)
    frames, mask, meta = out[0], out[1], out[2]
    assert json.dumps(meta["dynamic_zoom"]) == json.dumps(zoomed.meta["dynamic_zoom"])
    assert np.array_equal(np.asarray(frames.cpu()).view(np.uint32), zoomed.frames.cpu().numpy().view(np.uint32))
    assert float(mask.max()) == 0.0
