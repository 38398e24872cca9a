"""Rolling shutter round trip on the GPU (include/vstab.h "vstab_rolling_unwarp_batch"; apply_pipeline.apply_motion(rolling=True)).

  1. vstab_rolling_unwarp_batch against the NumPy restatement (tests/rolling_round_trip_restatement.py): frames, mask, pad
     counts and unsolved counts in bits, at the shapes where the tile can go wrong
  2. zero readout and all-zero velocity == vstab_warp_batch in bits
  3. the unsolved branch: the count is the restatement's, and those pixels hold the plain warp's values
  4. argument checks
  5. end to end on the analytic rolling clip of tests/test_rolling_shutter_gpu.py (12 frames, 480 x 270, readout 0.7, 2.7 px of
     skew at the corners, translation mode): forward replay == Flow in bits under both framings; the restore with rolling=True
     beats the plain restore; rolling=False is the call without the keyword; the node; a readout-0 block; the spatial fill

The restore's figures (PSNR of the restored frames against the source frames, over the pixels both restores show, 4 px
inside) were measured on the GPU (tools/rolling_round_trip_report.py, profiles/r22_rolling_round_trip.md):
  restored with rolling=True 45.26 dB, plain restore 27.48 dB: a gain of 17.78 dB
The test asserts half of the measured gain -- half, as tests/test_rolling_shutter_gpu.py takes half of its measured share: a
quality figure on one synthetic clip.
"""

import json

import numpy as np
import pytest

from tests import rolling_round_trip_restatement as RT
from tests import rolling_shutter_restatement as R
from tests import util

pytestmark = pytest.mark.gpu

LOCK_ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the largest corrections
E2E = dict(n=12, w=480, h=270, rho=0.7, amp=(24.0, 20.0, 0.004, 0.004), omega=0.3, seed=4)      # test_rolling_shutter_gpu.py's clip
RGB = (127, 127, 127)
BORDER = (0.2, 0.4, 0.6)
# measured on the GPU (see above; profiles/r22_rolling_round_trip.md)
MEASURED_PSNR = {"rolling": 45.26, "plain": 27.48}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _same(a, b):
    import torch

    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the kernel == the restatement, in bits ---------------------------------------------------------------------------------
def _unwarp_case(size, out_size, kind, seed):
    """3 frames: matrices that map the source onto the output canvas, the last one pushing part of the canvas outside the
    source; velocities: frame 1 all zero, the others a few px per frame with small rotation / scale terms."""
    w, h = size
    ow, oh = out_size
    n = 3
    rng = np.random.default_rng(seed)
    fit = np.diag([ow / w, oh / h, 1.0])
    mats = np.stack([fit @ m for m in util.test_matrices(n, w, h, kind, seed=seed)])
    mats[n - 1] = fit @ util.similarity(0.4 * w, -0.3 * h, 0.05, 1.0, w / 2, h / 2)
    vel = np.zeros((n, 6))
    for i in (0, 2):
        th, sc = rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
        vel[i] = (sc, -th, rng.uniform(-6, 6) - sc * ow / 2 + th * oh / 2, th, sc, rng.uniform(-4, 4) - th * ow / 2 - sc * oh / 2)
    return mats.astype(np.float32), vel


@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("size,out_size,kind", [((61, 45), (61, 45), "similarity"), ((65, 9), (130, 17), "perspective"),
                                                ((160, 90), (177, 95), "similarity"), ((33, 5), (70, 2), "similarity")])
def test_rolling_unwarp_equals_the_restatement(pkg, ctx, subpix, size, out_size, kind):
    """Partial tiles in x and in y, an output that is not the source's size, and a canvas of 2 rows (hm1 == 1)."""
    import torch

    w, h = size
    frames = util.synth_frames(3, h, w, seed=w)
    dev_frames = torch.from_numpy(frames).cuda()
    mats, vel = _unwarp_case(size, out_size, kind, seed=w)
    plain, plain_mask, plain_cnt = ctx.warp_batch(dev_frames, mats, out_size, interp="bilinear", border=BORDER, subpix=subpix,
                                                  want_mask=True, want_count=True)
    for rho in (0.8, -0.6):
        want, want_mask, want_cnt, want_uns = RT.rolling_unwarp(frames, mats, out_size, vel, rho, BORDER, subpix)
        got, got_mask, got_cnt, got_uns = ctx.rolling_unwarp_batch(dev_frames, mats, out_size, vel, rho, border=BORDER, subpix=subpix,
                                                                   want_mask=True, want_count=True, want_unsolved=True)
        assert got_uns.dtype == torch.int32 and got_uns.cpu().numpy().tolist() == want_uns.tolist() == [0, 0, 0]
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (rho, subpix)
        assert np.array_equal(_bits(got_mask.cpu().numpy()), _bits(want_mask)), (rho, subpix)
        assert got_cnt.cpu().numpy().tolist() == want_cnt.tolist()
        assert 0 < want_cnt[2] < out_size[0] * out_size[1]                     # the last matrix: part of the canvas is outside
        assert _same(got[1], plain[1]) and _same(got_mask[1], plain_mask[1])   # all-zero velocity: the plain warp
        assert not _same(got[0], plain[0]) and not _same(got[2], plain[2])     # the displacement did something
        # without the mask: no mask, no counts, the same frames; the counts are optional one by one
        bare = ctx.rolling_unwarp_batch(dev_frames, mats, out_size, vel, rho, border=BORDER, subpix=subpix, want_mask=False)
        assert bare[1] is None and bare[2] is None and bare[3] is None and _same(bare[0], got)
        only = ctx.rolling_unwarp_batch(dev_frames, mats, out_size, vel, rho, border=BORDER, subpix=subpix, want_mask=False,
                                        want_unsolved=True)
        assert only[3].cpu().numpy().tolist() == [0, 0, 0] and _same(only[0], got)


# ---- 2. the invariant ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
def test_zero_readout_and_zero_velocity_are_the_plain_warp(pkg, ctx, subpix):
    import torch

    for kind, (w, h), out_size in (("similarity", (333, 187), (333, 187)), ("perspective", (160, 90), (177, 95)),
                                   ("horizon", (160, 90), (160, 90)), ("similarity", (61, 45), (333, 11)), ("similarity", (33, 5), (70, 2))):
        n = 3
        frames = torch.from_numpy(util.synth_frames(n, h, w, seed=w + h)).cuda()
        mats = util.test_matrices(n, w, h, kind, seed=5).astype(np.float32)
        want, want_mask, want_cnt = ctx.warp_batch(frames, mats, out_size, interp="bilinear", border=BORDER, subpix=subpix,
                                                   want_mask=True, want_count=True)
        moving = np.tile([0.01, -0.004, 5.0, 0.004, 0.01, -3.0], (n, 1))
        for vel, rho in ((np.zeros((n, 6)), 1.0), (-np.zeros((n, 6)), -0.3), (moving, 0.0), (-moving, -0.0)):
            got, got_mask, got_cnt, unsolved = ctx.rolling_unwarp_batch(frames, mats, out_size, vel, rho, border=BORDER, subpix=subpix,
                                                                        want_mask=True, want_count=True, want_unsolved=True)
            assert _same(got, want) and _same(got_mask, want_mask), (kind, subpix, rho)
            assert torch.equal(got_cnt, want_cnt) and not unsolved.any()


# ---- 3. the unsolved branch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
def test_unsolved_pixels_are_counted_and_warped_plainly(pkg, ctx, subpix):
    import torch

    w, h = 61, 45
    vel, rho, rows = RT.unsolved_case(w, h)
    assert 0 < rows < h
    frames = util.synth_frames(1, h, w, seed=3)
    mats = util.test_matrices(1, w, h, "similarity", seed=2).astype(np.float32)
    want, want_mask, want_cnt, want_uns = RT.rolling_unwarp(frames, mats, (w, h), vel, rho, BORDER, subpix)
    assert want_uns.tolist() == [rows * w]                                     # the lower rows, whole
    dev = torch.from_numpy(frames).cuda()
    got, got_mask, got_cnt, got_uns = ctx.rolling_unwarp_batch(dev, mats, (w, h), vel, rho, border=BORDER, subpix=subpix, want_mask=True,
                                                               want_count=True, want_unsolved=True)
    assert got_uns.cpu().numpy().tolist() == want_uns.tolist() and 0 < int(got_uns[0]) < w * h
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and np.array_equal(_bits(got_mask.cpu().numpy()), _bits(want_mask))
    assert got_cnt.cpu().numpy().tolist() == want_cnt.tolist()
    plain, plain_mask, _ = ctx.warp_batch(dev, mats, (w, h), interp="bilinear", border=BORDER, subpix=subpix, want_mask=True)
    assert _same(got[0, h - rows:], plain[0, h - rows:]) and _same(got_mask[0, h - rows:], plain_mask[0, h - rows:])
    assert not _same(got[0, :h - rows], plain[0, :h - rows])
    # a second call starts from zero: the count is zeroed by the call, not accumulated
    again = ctx.rolling_unwarp_batch(dev, mats, (w, h), vel, rho, border=BORDER, subpix=subpix, want_mask=False, want_unsolved=True)
    assert again[3].cpu().numpy().tolist() == want_uns.tolist()


# ---- 4. argument checks -------------------------------------------------------------------------------------------------------
def test_argument_checks(pkg, ctx):
    import torch

    from vstab_amd import native

    frames = torch.zeros((2, 8, 8, 3), device="cuda")
    eye = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    with pytest.raises(ValueError, match=r"rolling_unwarp_batch: velocity \(1, 6\) is not \[2,6\]"):
        ctx.rolling_unwarp_batch(frames, eye, (8, 8), np.zeros((1, 6)), 0.5)
    for bad in (1.5, float("nan")):
        with pytest.raises(ValueError, match=r"rolling_unwarp_batch: readout=.* outside \[-1, 1\]"):
            ctx.rolling_unwarp_batch(frames, eye, (8, 8), np.zeros((2, 6)), bad)
    with pytest.raises(native.VstabError, match="vstab_rolling_unwarp_batch: NULL pointer argument"):
        ctx.rolling_unwarp_batch(frames, eye, (8, 8), None, 0.5)
    with pytest.raises(native.VstabError, match=r"vstab_rolling_unwarp_batch: bad size .*the output must have at least 2 rows"):
        ctx.rolling_unwarp_batch(frames, eye, (8, 1), np.zeros((2, 6)), 0.5)
    # the library's own readout check, under the Python one
    lib, bad_rc = ctx.lib, []
    out = torch.zeros((2, 8, 8, 3), device="cuda")
    vel, border = np.zeros((2, 6)), np.zeros(3, np.float32)
    for readout in (1.5, float("nan")):
        bad_rc.append(lib.vstab_rolling_unwarp_batch(ctx.handle, frames.data_ptr(), 2, 8, 8, eye.ctypes.data, 8, 8, border.ctypes.data, 0,
                                                     vel.ctypes.data, readout, out.data_ptr(), None, None, None))
    assert all(rc != 0 for rc in bad_rc)
    # a source of one row is fine here: the row times belong to the output
    one_row = ctx.rolling_unwarp_batch(torch.zeros((2, 1, 8, 3), device="cuda"), eye, (8, 8), np.zeros((2, 6)), 0.5)
    assert tuple(one_row[0].shape) == (2, 8, 8, 3)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------
def _stabilize(ctx, frames, framing, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, "translation", *LOCK_ARGS, ctx=ctx, keep_on_device=True,
                                estimator="flow", **kw)


def _apply(ctx, frames, meta, **kw):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    return ap.apply_motion(hm._normalize_video_input(frames), meta, RGB, ctx=ctx, keep_on_device=True, **kw)


def _inverse_meta(meta):
    return {k: v for k, v in meta.items() if k != "motion_meta"}           # what the Inverse node hands on


@pytest.fixture(scope="module")
def runs(pkg, ctx):
    """The analytic rolling clip, stabilized once per framing with readout 0.7; shared, never changed."""
    import torch

    path = R.CameraPath(E2E["w"], E2E["h"], amp=E2E["amp"], omega=E2E["omega"], seed=E2E["seed"])
    assert max(path.corner_skew(i, E2E["rho"]) for i in range(E2E["n"])) >= 2.0
    frames = R.rolling_clip(path, E2E["n"], E2E["rho"], torch.device("cuda"))
    out = {"frames": frames}
    for framing in ("crop_and_pad", "expand"):
        res = _stabilize(ctx, frames, framing, rolling_shutter=E2E["rho"])
        res.meta = json.loads(json.dumps(res.meta))                # what a saved workflow hands on
        out[framing] = res
    return out


@pytest.mark.parametrize("framing", ["crop_and_pad", "expand"])
def test_forward_replay_reproduces_flow(pkg, ctx, runs, framing):
    """Flow under either framing, replayed from its meta on the source frames: the matrices are replayed as recorded
    (crop_and_pad keeps the recorded canvas, which for an expand run is the expanded one), so the bits are Flow's."""
    run = runs[framing]
    got = _apply(ctx, runs["frames"], run.meta, framing_mode="crop_and_pad", rolling=True)
    assert got.meta["motion_apply"]["rolling_shutter"] == {"direction": "forward", "readout": E2E["rho"], "unsolved_max": 0}
    assert tuple(got.frames.shape) == tuple(run.frames.shape)
    assert _same(got.frames, run.frames) and _same(got.masks, run.masks)
    assert not _same(_apply(ctx, runs["frames"], run.meta, framing_mode="crop_and_pad").frames, run.frames)   # the rows matter


def test_forward_replay_under_expand_framing(pkg, ctx, runs):
    """Motion Apply's own `expand` framing of a crop_and_pad run: its matrices moved onto the canvas that holds every frame,
    the velocities unchanged (they belong to the source) -- the rolling warp of exactly those matrices."""
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    run = runs["crop_and_pad"]
    size = (E2E["w"], E2E["h"])
    got = _apply(ctx, runs["frames"], run.meta, framing_mode="expand", rolling=True)
    mats = [np.asarray(e["matrix"], np.float64) for e in run.meta["motion_meta"]["per_frame"]]
    expanded, out_size = ap._expand_matrices(mats, size)
    assert got.meta["motion_apply"]["output_size"] == [out_size[0], out_size[1]] and tuple(out_size) != size
    assert got.meta["motion_apply"]["rolling_shutter"]["direction"] == "forward"
    velocity = np.array(run.meta["rolling_shutter"]["velocity"], np.float64)
    want, want_mask, _ = ctx.rolling_warp_batch(runs["frames"], np.stack(expanded).astype(np.float32), out_size, velocity, E2E["rho"],
                                                border=hm.border_value(RGB), want_mask=True)
    assert _same(got.frames, want) and _same(got.masks[..., 0], want_mask)


def _interior(masks, radius):
    """Pixels at least `radius` inside mask == 0 (the frame's edge counts as padding): bool [N,H,W] on the device."""
    import torch.nn.functional as F

    k = 2 * radius + 1
    padded = F.pad((masks > 0).float()[:, None], (radius,) * 4, value=1.0)
    return F.max_pool2d(padded, k, stride=1)[:, 0] == 0


def _psnr(out, ideal, sel):
    import math

    err = ((out - ideal) ** 2).sum(-1)[sel]
    return 10.0 * math.log10(1.0 / (float(err.mean()) / 3.0))


def test_restore_beats_the_plain_restore(pkg, ctx, runs):
    import torch

    run = runs["crop_and_pad"]
    meta = _inverse_meta(run.meta)
    rolling = _apply(ctx, run.frames, meta, rolling=True)
    plain = _apply(ctx, run.frames, meta, rolling=False)
    info = rolling.meta["motion_apply"]["rolling_shutter"]
    assert info == {"direction": "inverse", "readout": E2E["rho"], "unsolved_max": 0}
    assert tuple(rolling.frames.shape) == tuple(runs["frames"].shape)
    sel = _interior(torch.maximum(rolling.masks[..., 0], plain.masks[..., 0]), 4)
    assert float(sel.float().mean()) > 0.5
    p_rolling, p_plain = _psnr(rolling.frames, runs["frames"], sel), _psnr(plain.frames, runs["frames"], sel)
    print(f"\nrolling round trip: restored with rolling=True {p_rolling:.2f} dB, plain restore {p_plain:.2f} dB "
          f"(interior {float(sel.float().mean()):.2f}, skew_px_max {run.meta['rolling_shutter']['skew_px_max']:.2f})")
    assert p_rolling > p_plain
    assert p_rolling - p_plain >= 0.5 * (MEASURED_PSNR["rolling"] - MEASURED_PSNR["plain"]), (p_rolling, p_plain)
    # under `expand` the restore is refused, before the warp
    with pytest.raises(ValueError, match="restores with framing_mode 'crop_and_pad' only"):
        _apply(ctx, run.frames, meta, framing_mode="expand", rolling=True)
    # an expand run restores too: its stabilized canvas is larger, the output is the source's
    big = runs["expand"]
    back = _apply(ctx, big.frames, _inverse_meta(big.meta), rolling=True)
    assert tuple(back.frames.shape) == tuple(runs["frames"].shape) and back.meta["motion_apply"]["rolling_shutter"]["direction"] == "inverse"


def _prime_timing_kinds(ctx):
    """One launch of each rolling kernel, so that both timing kinds exist; then the totals are cleared."""
    import torch

    eye, z = np.eye(3, dtype=np.float32)[None], np.zeros((1, 6))
    ctx.rolling_warp_batch(torch.zeros((1, 8, 8, 3), device="cuda"), eye, (8, 8), z, 0.5)
    ctx.rolling_unwarp_batch(torch.zeros((1, 8, 8, 3), device="cuda"), eye, (8, 8), z, 0.5)
    assert ctx.kernel_ms_stats("rolling_unwarp")[1] == 1 and ctx.kernel_ms_stats("rolling_warp")[1] == 1
    ctx.set_timing(True)                                   # clears the totals


def test_rolling_false_is_todays_result(pkg, ctx, runs):
    run = runs["crop_and_pad"]
    ctx.set_timing(True)
    try:
        _prime_timing_kinds(ctx)
        for frames, meta in ((runs["frames"], run.meta), (run.frames, _inverse_meta(run.meta))):
            got = _apply(ctx, frames, meta, rolling=False)
            default = _apply(ctx, frames, meta)
            assert _same(got.frames, default.frames) and _same(got.masks, default.masks)
            assert json.dumps(got.meta, sort_keys=True) == json.dumps(default.meta, sort_keys=True)
            assert "rolling_shutter" not in got.meta["motion_apply"]
            assert set(got.meta["motion_apply"]) == {"input_size", "output_size", "framing_mode", "interpolation", "motion_blur",
                                                     "motion_blur_samples", "source"}
        assert ctx.kernel_ms_stats("rolling_warp")[1] == 0 and ctx.kernel_ms_stats("rolling_unwarp")[1] == 0
        assert ctx.kernel_ms_stats("warp")[1] >= 4
    finally:
        ctx.set_timing(False)


def test_the_node_equals_the_keyword_call(pkg, ctx, runs):
    from vstab_amd import nodes

    def unpack(out):
        return out.result if hasattr(out, "result") else out.args

    run = runs["crop_and_pad"]
    for clip, meta, direction in ((runs["frames"], run.meta, "forward"), (run.frames, _inverse_meta(run.meta), "inverse")):
        ref = _apply(ctx, clip, meta, rolling=True)
        got_frames, got_mask, got_meta = unpack(nodes.VideoStabilizerMotionApplyRolling.execute(clip.cpu(), meta, "crop_and_pad", "#7F7F7F"))
        assert got_meta["motion_apply"]["rolling_shutter"]["direction"] == direction
        assert np.array_equal(_bits(got_frames.cpu().numpy()), _bits(ref.frames.cpu().numpy()))
        assert np.array_equal(_bits(got_mask.cpu().numpy()), _bits(ref.masks[..., 0].cpu().numpy()))
        assert json.dumps(got_meta, sort_keys=True) == json.dumps(ref.meta, sort_keys=True)
    ref = _apply(ctx, runs["frames"], run.meta, framing_mode="expand", rolling=True)
    got_frames, _, got_meta = unpack(nodes.VideoStabilizerMotionApplyRolling.execute(runs["frames"].cpu(), run.meta, "expand", "#7F7F7F"))
    assert np.array_equal(_bits(got_frames.cpu().numpy()), _bits(ref.frames.cpu().numpy()))
    assert got_meta["motion_apply"] == ref.meta["motion_apply"]


def test_a_block_with_readout_zero_takes_the_plain_path(pkg, ctx, runs):
    run = runs["crop_and_pad"]
    meta = json.loads(json.dumps(run.meta))
    meta["rolling_shutter"].update(readout=0.0, source="not_observable")
    ctx.set_timing(True)
    try:
        _prime_timing_kinds(ctx)
        for frames, m, direction in ((runs["frames"], meta, "forward"), (run.frames, _inverse_meta(meta), "inverse")):
            got = _apply(ctx, frames, m, rolling=True)
            plain = _apply(ctx, frames, m)
            assert _same(got.frames, plain.frames) and _same(got.masks, plain.masks)
            assert got.meta["motion_apply"]["rolling_shutter"] == {"direction": direction, "readout": 0.0, "unsolved_max": 0}
        assert ctx.kernel_ms_stats("rolling_warp")[1] == 0 and ctx.kernel_ms_stats("rolling_unwarp")[1] == 0
        assert ctx.kernel_ms_stats("warp")[1] >= 4
    finally:
        ctx.set_timing(False)


def test_it_composes_with_the_spatial_fill(pkg, ctx, runs):
    import torch

    run = runs["crop_and_pad"]
    for frames, meta in ((runs["frames"], run.meta), (run.frames, _inverse_meta(run.meta))):
        bare = _apply(ctx, frames, meta, rolling=True)
        filled = _apply(ctx, frames, meta, rolling=True, spatial_fill=True, stability_report=True, mask_grow=2)
        assert "spatial_fill" in filled.meta["motion_apply"] and "stability" in filled.meta["motion_apply"]
        assert "mask_handoff" in filled.meta["motion_apply"]
        assert filled.meta["motion_apply"]["rolling_shutter"] == bare.meta["motion_apply"]["rolling_shutter"]
        hole = bare.masks[..., 0] > 0.5
        assert bool(hole.any())
        assert torch.equal(filled.frames[~hole], bare.frames[~hole])           # valid pixels are untouched
        assert not torch.equal(filled.frames[hole], bare.frames[hole])         # the padding is filled
