"""Horizon level on the GPU (include/vstab.h "vstab_orientation_hist_batch"; flow_pipeline._stabilize_frames(horizon_level=...)).

  1. the kernel == the restatement (tests/horizon_level_restatement.py) exactly, the whole [n][513] array: one pixel, frames
     without an interior pixel, an odd frame size whose frames 1 and 2 start off a 16-byte boundary, the clip's size, widths
     around what one pass of a workgroup's lanes covers (16 rows x 256 pixels); constant, 0 / 255 cells (ties, the largest
     masses: 64-bit partial sums), stripes (the largest |gx|, one bin), exact diagonals, random bytes; three thresholds
  2. a clip tilted by 7 degrees comes out level, within 2 x the single-frame error measured on the CPU
     (R.MEASURED_WORST_DEG; profiles/r30_horizon_level.md); without the keyword it reads about 7 degrees
  3. a clip without structure is reported as not observable and comes out as without the keyword, in bits
  4. None is the call without the keyword and launches nothing
  5. composition: per-shot offsets under scene cuts, dynamic zoom, mesh warp, Motion Apply's replay, a binding limit
"""

import json

import numpy as np
import pytest

from tests import horizon_level_restatement as R

pytestmark = pytest.mark.gpu

BOUND_DEG = 2.0 * R.MEASURED_WORST_DEG
MARGIN = 48          # "interior only": a 7 degree turn of a 480 x 270 frame plus the shake uncovers up to ~35 px at the edges


# ---- 1. the kernel equals the restatement ----------------------------------------------------------------------------------
def _contents(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    return np.stack([
        np.full((h, w), 77),
        255 * (((x >> 1) + (y >> 1)) & 1),          # 2 x 2 cells of 0 / 255: |gx| == |gy| == 2550 everywhere
        255 * ((x >> 1) & 1),                       # stripes: |gx| = 4080, gy = 0
        200 * (((x + y) % 8) < 4),                  # exact diagonals: gx == gy
        200 * (((x - y) % 8) < 4) + 20,             # ... and gx == -gy
        rng.integers(0, 256, (h, w)),
    ]).astype(np.uint8)


# (h, w, n)
SHAPES = [(3, 3, 1), (2, 9, 2), (9, 2, 2), (37, 53, 3), (270, 480, 5), (18, 255, 2), (18, 256, 2), (18, 257, 2), (35, 272, 3)]


@pytest.mark.parametrize("h,w,n", SHAPES, ids=[f"{h}x{w}_n{n}" for h, w, n in SHAPES])
def test_kernel_equals_restatement(ctx, h, w, n):
    import torch

    contents = _contents(h, w, seed=h * 1000 + w)
    for start in range(0, len(contents), n):
        clip = np.take(contents, range(start, start + n), axis=0, mode="wrap")
        dev = torch.from_numpy(clip).to(ctx.device)
        for min_mag2 in (0, 65536, 1 << 27):
            want = R.orientation_hist(clip, min_mag2)
            got = ctx.orientation_hist_batch(dev, min_mag2)
            assert got.dtype == torch.int64 and tuple(got.shape) == (n, R.BINS)
            got = got.cpu().numpy()
            assert np.array_equal(got, want), (start, min_mag2, np.argwhere(got != want)[:8].tolist())
            if min_mag2 == 1 << 27 or h < 3 or w < 3:
                assert not got.any()
    if h >= 3 and w >= 3:
        full = R.orientation_hist(contents, 0)
        assert not full[0].any()                                              # constant: everything skipped
        assert full[1].sum() == full[1][0] + full[1][-1] > 0                  # ties land in bins -K and +K
        assert full[2].sum() == full[2][R.K] > 0                              # gy == 0 lands in bin 0
        if h * w >= 270 * 480:
            assert full[2].sum() > 1 << 32                                    # more than 32 bits of mass in one bin


def test_argument_errors_come_before_any_launch(pkg, ctx):
    import torch

    from vstab_amd import native

    a = torch.zeros((2, 8, 9), dtype=torch.uint8, device=ctx.device)
    ctx.set_timing(True)
    try:
        ctx.orientation_hist_batch(a, 0)                   # so that the timing kind exists
        ctx.set_timing(True)                               # clears the totals
        with pytest.raises(ValueError, match="orientation_hist_batch: gray must be a contiguous uint8"):
            ctx.orientation_hist_batch(a.float(), 0)
        with pytest.raises(ValueError, match="orientation_hist_batch: gray must be a contiguous uint8"):
            ctx.orientation_hist_batch(a.transpose(1, 2), 0)
        with pytest.raises(ValueError, match=r"orientation_hist_batch: gray of shape \(2, 8, 9, 1\) is not \[n,h,w\]"):
            ctx.orientation_hist_batch(a[..., None], 0)
        for bad in (-1, 1 << 32, 1.5, True):
            with pytest.raises(ValueError, match="orientation_hist_batch: min_mag2="):
                ctx.orientation_hist_batch(a, bad)
        with pytest.raises(native.VstabError, match="vstab_orientation_hist_batch: bad shape n=0"):
            ctx.orientation_hist_batch(a[:0], 0)
        with pytest.raises(native.VstabError, match="vstab_orientation_hist_batch: 40000 x 1 pixels, the limit is 32768 per axis"):
            ctx.orientation_hist_batch(torch.zeros((1, 1, 40000), dtype=torch.uint8, device=ctx.device), 0)
        assert ctx.kernel_ms_stats("orientation_hist")[1] == 0
    finally:
        ctx.set_timing(False)


# ---- 2..5: end to end ------------------------------------------------------------------------------------------------------
RGB = (127, 127, 127)
ARGS = (True, 1.0, 0.5, 0.6, RGB, 16.0)      # camera_lock + strength 1 at 16 fps
N = 12


def _stabilize(ctx, frames, transform_mode="similarity", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", transform_mode, *ARGS, ctx=ctx,
                                keep_on_device=True, estimator=kw.pop("estimator", "flow"), **kw)


def _bits_equal(a, b):
    import torch

    return tuple(a.shape) == tuple(b.shape) and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rolls(result):
    """The roll of every returned frame, measured with the restatement on the frames' luma, interior only."""
    from vstab_amd import horizon_level as hl

    luma = R.luma_u8(result.frames.cpu().numpy())[:, MARGIN:-MARGIN, MARGIN:-MARGIN]
    rolls = [hl.frame_roll(h)[0] for h in R.orientation_hist(luma, hl.MIN_MAG2)]
    assert all(r is not None for r in rolls)
    return np.asarray(rolls)


def _device(ctx, gray):
    import torch

    return torch.from_numpy(R.rgb_clip(gray)).to(ctx.device)


@pytest.fixture(scope="module")
def tilted(ctx):
    """The analytic clip at a roll of 7 degrees plus a +-2 degree roll shake and a few pixels of translation; shared."""
    gray, _ = R.tilted_clip(R.Scene(), 7.0, frames=N)
    return _device(ctx, gray)


@pytest.fixture(scope="module")
def levelled(pkg, ctx, tilted):
    return _stabilize(ctx, tilted, horizon_level=True)


@pytest.fixture(scope="module")
def plain(pkg, ctx, tilted):
    return _stabilize(ctx, tilted)


def test_levels_a_tilted_clip(pkg, ctx, tilted, levelled, plain):
    block = levelled.meta["horizon_level"]
    assert json.loads(json.dumps(block)) == block
    assert list(block) == ["version", "window_s", "limit_deg", "min_confidence", "roll_deg", "confidence", "frames_measured",
                           "shots_not_observable", "offset_deg", "correction_deg", "correction_deg_max", "frames_limited"]
    assert (block["version"], block["window_s"], block["limit_deg"], block["min_confidence"]) == (1, None, 20.0, 0.25)
    assert block["frames_measured"] == N and block["shots_not_observable"] == 0 and block["frames_limited"] == 0
    assert set(levelled.meta) - set(plain.meta) == {"horizon_level"} and set(plain.meta) <= set(levelled.meta)
    after, before = _rolls(levelled), _rolls(plain)
    print(f"\nhorizon level: bound {BOUND_DEG:.4f} deg;  levelled rolls {np.round(after, 4).tolist()} (worst {np.abs(after).max():.4f})"
          f"\n  without the keyword {np.round(before, 4).tolist()};  confidence {np.round(block['confidence'], 3).tolist()}"
          f"\n  offset {block['offset_deg'][0]:.4f} correction {np.round(block['correction_deg'], 4).tolist()}")
    assert np.abs(before - 7.0).max() < 0.5          # "about 7": camera_lock pins the clip to frame 0, which stands at 7 exactly
    assert np.abs(after).max() <= BOUND_DEG
    assert len(set(block["offset_deg"])) == 1 and abs(block["offset_deg"][0] - 7.0) <= BOUND_DEG
    assert not levelled.device_plan["used"]          # levelled calls form the plan on the host


def test_not_observable_leaves_the_clip_alone(pkg, ctx):
    gray, _ = R.tilted_clip(R.Scene(sinus=0.03, structure=False, freq=(0.1, 0.6)), 7.0, frames=N)
    clip = _device(ctx, gray)
    base, on = _stabilize(ctx, clip), _stabilize(ctx, clip, horizon_level=True)
    block = on.meta["horizon_level"]
    print(f"\nnot observable: confidence {np.round(block['confidence'], 3).tolist()}")
    assert block["shots_not_observable"] == 1 and block["frames_measured"] == 0 and max(block["confidence"]) <= 0.05
    assert block["offset_deg"] == [None] * N and block["correction_deg"] == [0.0] * N and block["correction_deg_max"] == 0.0
    assert _bits_equal(on.frames, base.frames) and _bits_equal(on.masks, base.masks)


def test_none_is_the_call_without_the_keyword(pkg, ctx, tilted, plain):
    import torch

    ctx.set_timing(True)
    try:
        ctx.orientation_hist_batch(torch.zeros((1, 8, 9), dtype=torch.uint8, device=ctx.device), 0)   # so that the timing kind exists
        ctx.set_timing(True)                                                      # clears the totals
        off = _stabilize(ctx, tilted, horizon_level=None, horizon_limit=None)
        assert ctx.kernel_ms_stats("orientation_hist")[1] == 0                    # nothing new is launched
        _stabilize(ctx, tilted, horizon_level=True)
        assert ctx.kernel_ms_stats("orientation_hist")[1] == 1                    # one launch per clip
    finally:
        ctx.set_timing(False)
    assert _bits_equal(off.frames, plain.frames) and _bits_equal(off.masks, plain.masks)
    assert json.dumps(off.meta) == json.dumps(plain.meta) and "horizon_level" not in off.meta
    assert off.device_plan["used"]


def test_scene_cuts_level_every_shot_by_itself(pkg, ctx):
    import torch

    cut = 6
    a, _ = R.tilted_clip(R.Scene(seed=7), 6.0, frames=cut, seed=3)
    b, _ = R.tilted_clip(R.Scene(seed=11), -4.0, frames=N - cut, seed=5)
    clip = _device(ctx, np.concatenate([a, b]))
    run = _stabilize(ctx, clip, scene_cuts=[cut], horizon_level=True)
    block = run.meta["horizon_level"]
    off = block["offset_deg"]
    print(f"\nscene cuts: offsets {np.round(off, 4).tolist()}")
    assert run.meta["scene_cuts"]["cuts"] == [cut] and block["shots_not_observable"] == 0
    assert len(set(off[:cut])) == 1 and len(set(off[cut:])) == 1
    assert abs(off[0] - 6.0) <= BOUND_DEG and abs(off[cut] + 4.0) <= BOUND_DEG
    assert np.abs(_rolls(run)).max() <= BOUND_DEG


def test_dynamic_zoom_measures_the_levelled_matrices(pkg, ctx, tilted):
    zoomed = _stabilize(ctx, tilted, dynamic_zoom=True)
    both = _stabilize(ctx, tilted, dynamic_zoom=True, horizon_level=True)
    keys = list(both.meta)
    assert keys.index("dynamic_zoom") == keys.index("horizon_level") + 1
    z, zl = zoomed.meta["dynamic_zoom"], both.meta["dynamic_zoom"]
    print(f"\ndynamic zoom: static_zoom {z['static_zoom']:.4f} -> levelled {zl['static_zoom']:.4f}")
    assert zl["frames_with_padding"] == 0 and both.meta["padding_fraction_max"] == 0
    assert zl["static_zoom"] >= z["static_zoom"]


def test_mesh_warp_follows_the_levelled_matrices(pkg, ctx, tilted):
    run = _stabilize(ctx, tilted, mesh_warp=True, horizon_level=True)
    rolls = _rolls(run)
    print(f"\nmesh warp: levelled rolls {np.round(rolls, 4).tolist()}")
    assert "mesh_warp" in run.meta and np.abs(rolls).max() <= BOUND_DEG


EXTRAS = [("temporal_fill", dict(temporal_fill=2)), ("spatial_fill", dict(spatial_fill=True)),
          ("sharpness_transfer", dict(sharpness_transfer=2)), ("deflicker", dict(deflicker=True)),
          ("stability", dict(stability_report=True)), ("mask_handoff", dict(mask_grow=2)),
          ("estimation_mask", "mask"), ("drift_correction", dict(drift_correction=4))]


@pytest.mark.parametrize("key,kw", EXTRAS, ids=[k for k, _ in EXTRAS])
def test_every_pass_behind_the_plan_follows(pkg, ctx, tilted, levelled, key, kw):
    """The passes that read the plan's matrices or run behind the warp take the levelled ones: each runs, adds its block, and
    the frames stay level; those that do not touch the estimation leave the levelling's own block as it is."""
    if kw == "mask":
        mask = np.zeros((270, 480), np.float32)
        mask[100:140, 200:260] = 1.0
        kw = dict(estimation_mask=mask)
    run = _stabilize(ctx, tilted, horizon_level=True, **kw)
    rolls = _rolls(run)
    print(f"\n{key}: levelled rolls {np.round(rolls, 4).tolist()}")
    assert key in run.meta and np.abs(rolls).max() <= BOUND_DEG
    if key not in ("estimation_mask", "drift_correction"):
        assert run.meta["horizon_level"] == levelled.meta["horizon_level"]
        assert run.meta["stabilization_warp"] == levelled.meta["stabilization_warp"]


def test_padding_fractions_describe_the_levelled_warp(pkg, ctx, levelled, plain):
    padded = (levelled.masks[..., 0] > 0.5).float().mean(dim=(1, 2)).cpu().numpy()
    assert abs(levelled.meta["padding_fraction_mean"] - float(padded.mean())) < 1e-6
    assert abs(levelled.meta["padding_fraction_max"] - float(padded.max())) < 1e-6
    assert levelled.meta["padding_fraction_mean"] > plain.meta["padding_fraction_mean"]      # a 7 degree turn uncovers corners


def test_motion_apply_replays_the_levelled_frames(pkg, ctx, tilted, levelled):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    meta = json.loads(json.dumps(levelled.meta))                                  # what a saved workflow hands on
    got = ap.apply_motion(hm._normalize_video_input(tilted), {"motion_meta": meta["motion_meta"]}, RGB, ctx=ctx, keep_on_device=True)
    assert _bits_equal(got.frames, levelled.frames) and _bits_equal(got.masks, levelled.masks)


def test_a_binding_limit_is_counted(pkg, ctx, tilted):
    block = _stabilize(ctx, tilted, horizon_level=True, horizon_limit=3).meta["horizon_level"]
    assert block["limit_deg"] == 3.0 and block["frames_limited"] == N
    assert [abs(c) for c in block["correction_deg"]] == [3.0] * N and block["correction_deg_max"] == 3.0


@pytest.mark.parametrize("estimator,mode", [("flow", "translation"), ("classic", "similarity"), ("flow_tvl1", "similarity"),
                                            ("flow_phase_correlate", "similarity")])
def test_every_camera_estimator_levels(pkg, ctx, estimator, mode):
    """A clip that is tilted but does not roll (translation shake only), so that the estimators without a rotation level it too."""
    gray, _ = R.tilted_clip(R.Scene(), 7.0, frames=N, shake_deg=0.0)
    clip = _device(ctx, gray)
    run = _stabilize(ctx, clip, transform_mode=mode, horizon_level=True, estimator=estimator)
    rolls = _rolls(run)
    print(f"\n{estimator} / {mode}: levelled rolls {np.round(rolls, 4).tolist()}")
    assert run.meta["horizon_level"]["frames_measured"] == N and np.abs(rolls).max() <= BOUND_DEG
