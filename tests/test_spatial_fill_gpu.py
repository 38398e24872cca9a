"""GPU: vstab_spatial_fill_batch (csrc/vstab_fill.hip) and the `spatial_fill` keyword / node.

Every comparison of pixels, masks and counts is bit-exact and over all pixels, against the NumPy restatement of the full
pyramid (tests/spatial_fill_restatement.py, whose properties are checked on the CPU in tests/test_spatial_fill_cpu.py).
"""

import json

import numpy as np
import pytest

from tests import spatial_fill_restatement as R
from tests.util import shake_path, synth_frames

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run_kernel(ctx, frames, mask, chunk_frames=0):
    import torch

    d = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(ctx.device).contiguous()
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(ctx.device).contiguous()
    hc, fc = ctx.spatial_fill_batch(d, m, chunk_frames=chunk_frames)
    return d.cpu().numpy(), m.cpu().numpy(), hc.cpu().numpy().astype(np.int64), fc.cpu().numpy().astype(np.int64)


def _assert_equal_to_restatement(frames, mask, got):
    d, m, hc, fc = got
    rd, rhc, rfc = R.fill_batch(frames, mask)
    assert np.array_equal(_bits(m), _bits(mask)), "the mask was written"
    diff = (_bits(d) != _bits(rd)).any(axis=-1)
    assert not diff.any(), f"dst differs at {int(diff.sum())} pixels, first {np.argwhere(diff)[:4].tolist()}"
    assert np.array_equal(hc, rhc) and np.array_equal(fc, rfc), (hc, rhc, fc, rfc)
    return rd, rhc, rfc


# 65x33: one past the first pass's 64 x 32 tile in both axes (as h x w and as w x h); 135x240 / 270x480: several tiles, a
# pyramid whose upper levels the tail kernel holds and lower levels the push kernels walk
SHAPES = [(1, 1), (1, 7), (3, 5), (17, 9), (65, 33), (33, 65), (64, 32), (32, 64), (135, 240), (270, 480)]


def _patterns(h, w):
    """name -> hole mask [h,w] bool: patterns that send the push up to the top level and clip 2 x 2 blocks."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"none": np.zeros((h, w), bool), "all": np.ones((h, w), bool)}
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, w - 1), "corner_bl": (h - 1, 0), "corner_br": (h - 1, w - 1)}.items():
        m = np.zeros((h, w), bool)
        m[y, x] = True
        out[name] = m
    out["last_column"] = xx == w - 1
    out["last_row"] = yy == h - 1
    b = max(1, min(h, w) // 12)
    ring = np.zeros((h, w), bool)
    ring[:b] = ring[:, :b] = True
    ring[h - (b // 2 + 1):] = True
    out["ring"] = ring
    out["wedge"] = (yy < 2 + 0.05 * xx) | (xx > w - 3 - 0.04 * yy) | (yy > h - 3)
    for name, (y, x) in {"single_valid_br": (h - 1, w - 1), "single_valid_tl": (0, 0), "single_valid_mid": (h // 2, w // 2)}.items():
        m = np.ones((h, w), bool)
        m[y, x] = False
        out[name] = m
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_restatement(ctx, shape):
    """All hole patterns of a shape, three frames with different patterns per call (frame indexing)."""
    h, w = shape
    pats = list(_patterns(h, w).items())
    texture = synth_frames(3, h, w, seed=h * 31 + w)
    filled_somewhere = False
    for i in range(0, len(pats), 3):
        group = (pats + pats[:2])[i:i + 3]
        frames = texture[np.arange(3) % len(texture)].copy()
        mask = np.stack([g[1] for g in group]).astype(np.float32)
        got = _run_kernel(ctx, frames, mask)
        _, _, rfc = _assert_equal_to_restatement(frames, mask, got)
        keep = mask <= 0.5
        assert np.array_equal(_bits(got[0])[keep], _bits(frames)[keep]), [g[0] for g in group]
        filled_somewhere = filled_somewhere or rfc.sum() > 0
    assert filled_somewhere or h * w == 1


def test_hole_rule_nan_and_exactly_half(ctx):
    """!(mask <= 0.5f): NaN, +inf and 0.75 are holes; 0.5 exactly, 0.25, -inf and -1 are not."""
    h, w = 37, 53
    rng = np.random.default_rng(5)
    frames = synth_frames(2, h, w, seed=9)
    values = np.array([np.nan, 0.5, np.inf, 0.75, 0.25, -np.inf, -1.0, np.nextafter(np.float32(0.5), np.float32(1.0)), 1.0, 0.0],
                      np.float32)
    mask = values[rng.integers(0, len(values), (2, h, w))]
    got = _run_kernel(ctx, frames, mask)
    rd, rhc, _ = R.fill_batch(frames, mask)
    assert np.array_equal(_bits(got[1]), _bits(mask))                     # (NaN != NaN: the mask is compared in bits)
    assert np.array_equal(_bits(got[0]), _bits(rd)) and np.array_equal(got[2], rhc) and np.array_equal(got[3], rhc)
    expect = np.isnan(mask) | (mask > 0.5)
    assert rhc.tolist() == expect.sum(axis=(1, 2)).tolist() and 0 < rhc[0] < h * w
    assert np.array_equal(_bits(got[0])[~expect], _bits(frames)[~expect])


def test_property_random_shapes_and_densities(ctx):
    """40 seeded draws: h, w in 1..70, hole density in {0.01, 0.5, 0.99}, 1..3 frames."""
    rng = np.random.default_rng(1996)
    for draw in range(40):
        h, w, n = int(rng.integers(1, 71)), int(rng.integers(1, 71)), int(rng.integers(1, 4))
        density = (0.01, 0.5, 0.99)[draw % 3]
        frames = rng.uniform(0.0, 1.0, (n, h, w, 3)).astype(np.float32)
        mask = (rng.uniform(0.0, 1.0, (n, h, w)) < density).astype(np.float32)
        try:
            _assert_equal_to_restatement(frames, mask, _run_kernel(ctx, frames, mask))
        except AssertionError as exc:
            raise AssertionError(f"draw {draw}: {n} x {h} x {w}, density {density}: {exc}") from None


def _five_frames(h=45, w=83):
    frames = synth_frames(5, h, w, seed=12)
    pats = _patterns(h, w)
    mask = np.stack([pats[k] for k in ("ring", "none", "wedge", "all", "single_valid_mid")]).astype(np.float32)
    return frames, mask


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunking_does_not_change_the_result(ctx, chunk):
    frames, mask = _five_frames()
    whole = _run_kernel(ctx, frames, mask, chunk_frames=0)
    _assert_equal_to_restatement(frames, mask, whole)
    parts = _run_kernel(ctx, frames, mask, chunk_frames=chunk)
    assert np.array_equal(_bits(parts[0]), _bits(whole[0])) and np.array_equal(_bits(parts[1]), _bits(whole[1]))
    assert np.array_equal(parts[2], whole[2]) and np.array_equal(parts[3], whole[3])


def test_running_twice_equals_running_once(ctx):
    import torch

    frames, mask = _five_frames()
    d = torch.from_numpy(frames).to(ctx.device).contiguous()
    m = torch.from_numpy(mask).to(ctx.device).contiguous()
    first = [t.cpu().numpy() for t in ctx.spatial_fill_batch(d, m)]
    once = d.cpu().numpy()
    second = [t.cpu().numpy() for t in ctx.spatial_fill_batch(d, m)]
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(once)) and np.array_equal(_bits(m.cpu().numpy()), _bits(mask))
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    _assert_equal_to_restatement(frames, mask, (once, mask, first[0].astype(np.int64), first[1].astype(np.int64)))


def test_invalid_arguments_are_refused(ctx):
    import torch

    from vstab_amd import native

    d = torch.zeros((2, 8, 9, 3), device=ctx.device)
    with pytest.raises(native.VstabError, match="do not match"):
        ctx.spatial_fill_batch(d, torch.zeros((2, 9, 8), device=ctx.device))
    with pytest.raises(native.VstabError, match="mask must be a contiguous float32"):
        ctx.spatial_fill_batch(d, torch.zeros((2, 8, 9), device=ctx.device, dtype=torch.float64))
    with pytest.raises(native.VstabError, match="dst must be a contiguous float32"):
        ctx.spatial_fill_batch(d.cpu(), torch.zeros((2, 8, 9), device=ctx.device))
    with pytest.raises(native.VstabError, match="chunk_frames=-1"):
        ctx.spatial_fill_batch(d, torch.zeros((2, 8, 9), device=ctx.device), chunk_frames=-1)
    assert ctx.spatial_fill_batch(d, torch.zeros((2, 8, 9), device=ctx.device), want_counts=False) == (None, None)


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H, N = 160, 96, 12
ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the whole shake becomes padding
SHAKE_AMP = 8.0    # tests.util.shake_path scales its steps with the frame: amp 8 at 160 px is up to +-4 px per frame


@pytest.fixture(scope="module")
def clip(ctx):
    import torch

    import bench

    return bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=shake_path(N, W, H, "similarity", seed=3, amp=SHAKE_AMP))


def _stabilize(ctx, frames, framing="crop_and_pad", estimator="flow", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, "similarity", *ARGS, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


def _expected_block(rhc, rfc, h, w):
    fractions = (rfc.astype(np.float32) / np.float32(h * w)).astype(np.float64)
    return {"method": "push_pull", "version": 1, "filled_fraction_mean": float(fractions.mean()),
            "filled_fraction_max": float(fractions.max()), "frames_filled": int((rfc > 0).sum()),
            "frames_without_source": int(((rhc > 0) & (rfc == 0)).sum())}


def _assert_is_fill_of(base, filled, block):
    """`filled` is `base` with the restatement applied to its frames: pixels in bits, the mask untouched, the block from the
    restatement's counts.  At least one frame has padding, so the comparison cannot pass vacuously."""
    d0, m0 = base.frames.cpu().numpy(), base.masks.cpu().numpy()[..., 0]
    rd, rhc, rfc = R.fill_batch(d0, m0)
    assert rfc.max() > 0, "no frame has padding: the test would show nothing"
    assert not np.array_equal(_bits(rd), _bits(d0))
    assert np.array_equal(_bits(filled.frames.cpu().numpy()), _bits(rd))
    assert np.array_equal(_bits(filled.masks.cpu().numpy()), _bits(base.masks.cpu().numpy()))
    assert block == _expected_block(rhc, rfc, d0.shape[1], d0.shape[2])


@pytest.mark.parametrize("framing,estimator", [("crop_and_pad", "flow"), ("expand", "flow"), ("crop_and_pad", "classic")])
def test_end_to_end_keyword(pkg, ctx, clip, framing, estimator):
    ctx.set_timing(True)
    try:
        ctx.spatial_fill_batch(clip[:1].clone(), clip[:1, :, :, 0].contiguous())   # so that the timing kind exists
        ctx.set_timing(True)                                                      # clears the totals
        plain = _stabilize(ctx, clip, framing, estimator)                          # the parent's call
        off = _stabilize(ctx, clip, framing, estimator, spatial_fill=False)
        assert ctx.kernel_ms_stats("sfill")[1] == 0                                # False launches nothing
        on = _stabilize(ctx, clip, framing, estimator, spatial_fill=True)
        assert ctx.kernel_ms_stats("sfill")[1] == 1
    finally:
        ctx.set_timing(False)
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(plain.frames.cpu().numpy()))
    assert np.array_equal(_bits(off.masks.cpu().numpy()), _bits(plain.masks.cpu().numpy()))
    assert json.dumps(off.meta) == json.dumps(plain.meta) and "spatial_fill" not in off.meta
    if framing == "crop_and_pad" and estimator == "flow":
        assert on.device_plan["used"]                                              # the device-plan path
    meta_on = dict(on.meta)
    block = meta_on.pop("spatial_fill")
    assert json.dumps(meta_on) == json.dumps(off.meta)                             # padding_fraction_* keep describing the warp
    _assert_is_fill_of(off, on, block)


@pytest.mark.parametrize("extra", [dict(temporal_fill=2), dict(mesh_warp=(4, 3)), dict(scene_cuts=[6], framing="expand")],
                         ids=["temporal_fill", "mesh_warp", "scene_cuts_expand"])
def test_end_to_end_behind_the_other_passes(pkg, ctx, clip, extra):
    base = _stabilize(ctx, clip, **extra)
    on = _stabilize(ctx, clip, spatial_fill=True, **extra)
    meta_on = dict(on.meta)
    block = meta_on.pop("spatial_fill")
    assert json.dumps(meta_on) == json.dumps(base.meta)
    assert [k for k in extra if k != "framing"][0] in base.meta
    _assert_is_fill_of(base, on, block)


def test_crop_framing_is_a_noop_without_a_block(pkg, ctx, clip):
    a = _stabilize(ctx, clip, "crop")
    b = _stabilize(ctx, clip, "crop", spatial_fill=True)
    assert np.array_equal(_bits(a.frames.cpu().numpy()), _bits(b.frames.cpu().numpy()))
    assert json.dumps(a.meta) == json.dumps(b.meta)


def _apply(ctx, frames, meta, **kw):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    return ap.apply_motion(hm._normalize_video_input(frames), meta, (127, 127, 127), ctx=ctx, keep_on_device=True, **kw)


def test_motion_apply_keyword(pkg, ctx, clip):
    run = _stabilize(ctx, clip, mesh_warp=(4, 3), mesh_motion=True)
    meta = json.loads(json.dumps(run.meta))
    inverse_only = {k: v for k, v in meta.items() if k != "motion_meta"}
    cases = [(clip, meta, dict()), (clip, meta, dict(framing_mode="expand")), (clip, meta, dict(interpolation="bicubic")),
             (clip, meta, dict(mesh=True)), (run.frames, inverse_only, dict(mesh=True)), (run.frames, inverse_only, dict())]
    for frames, m, kw in cases:
        base = _apply(ctx, frames, m, **kw)
        off = _apply(ctx, frames, m, spatial_fill=False, **kw)
        on = _apply(ctx, frames, m, spatial_fill=True, **kw)
        assert json.dumps(off.meta) == json.dumps(base.meta) and "spatial_fill" not in off.meta["motion_apply"]
        assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(base.frames.cpu().numpy()))
        meta_on = json.loads(json.dumps(on.meta))
        block = meta_on["motion_apply"].pop("spatial_fill")
        assert json.dumps(meta_on) == json.dumps(base.meta), kw
        _assert_is_fill_of(base, on, block)
    # crop framing has no padding: no block, same pixels
    a, b = _apply(ctx, clip, meta, framing_mode="crop"), _apply(ctx, clip, meta, framing_mode="crop", spatial_fill=True)
    if a.meta["motion_apply"]["framing_mode"] == "crop":
        assert json.dumps(a.meta) == json.dumps(b.meta)
        assert np.array_equal(_bits(a.frames.cpu().numpy()), _bits(b.frames.cpu().numpy()))


def test_motion_blur_is_refused(pkg, ctx, clip):
    run = _stabilize(ctx, clip)
    with pytest.raises(ValueError, match="spatial_fill=True is not supported with motion_blur=0.4"):
        _apply(ctx, clip, run.meta, motion_blur=0.4, spatial_fill=True)
    _apply(ctx, clip, run.meta, motion_blur=0.4)                                   # without the keyword it still runs


def test_node_equals_the_binding(pkg, ctx, clip):
    from vstab_amd import nodes, spatial_fill

    run = _stabilize(ctx, clip)
    d = run.frames.clone()
    m = run.masks[..., 0].contiguous()
    hc, fc = ctx.spatial_fill_batch(d, m)
    want_block = spatial_fill.fill_meta(hc.cpu().numpy(), fc.cpu().numpy(), (W, H))
    assert want_block["frames_filled"] > 0
    for frames_in, mask_in in ((run.frames.cpu(), run.masks[..., 0].cpu()), (run.frames, run.masks)):
        keep = frames_in.clone()
        out = nodes.VideoStabilizerPaddingFill.execute(frames_in, mask_in)
        node_frames, node_meta = out.result if hasattr(out, "result") else out.args
        assert isinstance(node_meta, str) and json.loads(node_meta) == {"spatial_fill": want_block}
        assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(d.cpu().numpy()))
        assert np.array_equal(_bits(frames_in.cpu().numpy()), _bits(keep.cpu().numpy()))     # the inputs stay as they are
    # one mask for every frame
    one = run.masks[:1, ..., 0].contiguous()
    d1 = run.frames.clone()
    ctx.spatial_fill_batch(d1, one.expand(N, H, W).contiguous())
    out = nodes.VideoStabilizerPaddingFill.execute(run.frames.cpu(), one.cpu())
    node_frames = (out.result if hasattr(out, "result") else out.args)[0]
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(d1.cpu().numpy()))
