"""GPU: vstab_mask_moments_batch (csrc/vstab_subject.hip), the "subject" estimator of the Flow pipeline and its node.

sums and bbox are integers and must equal the NumPy restatement (tests/subject_restatement.py, whose properties are checked
on the CPU in tests/test_subject_lock_cpu.py) exactly: no tolerance anywhere in the kernel tests.  The end-to-end tests are
oracle-independent: a saturated disc is painted at known integer centres, the mask is the disc, and what the pipeline reports
and returns is held against those centres.
"""

import json

import numpy as np
import pytest

from tests import subject_restatement as R
from tests.util import synth_frames

pytestmark = pytest.mark.gpu

# (n, h, w): a single pixel; frame sizes that are no multiple of 4 floats (frame k starts k floats (mod 4) off the 16-byte
# boundary: head and tail); whole float4s, less than a tile of 1024 float4s; 9 x 130 = one tile and a part; 37 x 253 = several
# tiles, a workgroup each; 6 x 13 x 67: every head length; 2100 x 2100 all subject: sum_x = 2100^2 * 1049.5 > 2^32, the only
# shape that fails with a 32-bit accumulator or atomic
SHAPES = [(1, 1, 1), (3, 1, 67), (3, 13, 67), (4, 8, 64), (2, 9, 130), (5, 37, 253), (6, 13, 67), (1, 2100, 2100)]


def _dev(ctx, x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(ctx.device).contiguous()


def _call(ctx, mask):
    sums, bbox = ctx.mask_moments_batch(mask)
    assert str(sums.dtype) == "torch.int64" and str(bbox.dtype) == "torch.int32"
    assert tuple(sums.shape) == (mask.shape[0], 3) and tuple(bbox.shape) == (mask.shape[0], 4)
    return sums.cpu().numpy().tolist(), bbox.cpu().numpy().tolist()


def _want(mask):
    sums, bbox = R.moments(mask)
    return sums.tolist(), bbox.tolist()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_restatement(ctx, shape):
    n, h, w = shape
    rng = np.random.default_rng(n * 10007 + h * 101 + w)
    if shape == (1, 2100, 2100):
        mask = np.ones(shape, np.float32)
    else:
        mask = R.MASK_VALUES[rng.integers(0, len(R.MASK_VALUES), shape)]
    if n > 1:
        mask[-1] = 0.0                                   # a frame without a subject: sums 0, bbox four times -1
    if n > 2:
        mask[-2] = 0.0
        mask[-2, h - 1, w - 1] = 1.0                     # a single subject pixel in the last row and column
    d = _dev(ctx, mask)
    keep = d.clone()
    got, want = _call(ctx, d), _want(mask)
    assert got == want, shape
    if n > 1:
        assert got[0][-1] == [0, 0, 0] and got[1][-1] == [-1, -1, -1, -1]
    if n > 2:
        assert got[0][-2] == [1, w - 1, h - 1] and got[1][-2] == [w - 1, h - 1, w - 1, h - 1]
    if shape == (1, 2100, 2100):
        assert got[0][0][1] == 2100 * 2100 * 2099 // 2 > 2 ** 32 and got[1][0] == [0, 0, 2099, 2099]
    assert np.array_equal(_bits(d), _bits(keep))         # nothing is written to the input
    # one subject pixel per frame, walking through the corners and the last row and column: every frame at its own head length
    edges = np.zeros(shape, np.float32)
    spots = [(h - 1, w - 1), (0, 0), (0, w - 1), (h - 1, 0), (h // 2, w - 1), (h - 1, w // 2)]
    for k in range(n):
        edges[k][spots[k % len(spots)]] = np.inf if k % 2 else 1.0
    assert _call(ctx, _dev(ctx, edges)) == _want(edges)
    assert _want(edges)[1][0] == [w - 1, h - 1, w - 1, h - 1]
    if n > 1:
        # a view that starts one frame into the allocation (its own offset from the 16-byte boundary), and frame-by-frame calls
        assert _call(ctx, d[1:]) == ([want[0][k] for k in range(1, n)], [want[1][k] for k in range(1, n)])
        for k in range(n):
            one = _call(ctx, d[k:k + 1].clone())
            assert (one[0][0], one[1][0]) == (want[0][k], want[1][k]), (shape, k)


def test_more_tiles_than_workgroups(ctx):
    """40 frames of 433 x 1001 pixels: 106 tiles per frame for 103 workgroups, so some workgroups loop over two tiles; the
    frame size is odd, so the frames start at every offset from the 16-byte boundary."""
    n, h, w = 40, 433, 1001
    rng = np.random.default_rng(21)
    mask = (rng.uniform(0.0, 1.0, (n, h, w)) < 0.1).astype(np.float32)
    mask[7] = 0.0
    d = _dev(ctx, mask)
    first, second = _call(ctx, d), _call(ctx, d)
    assert first == second == _want(mask)


def test_argument_errors_come_before_any_launch(ctx):
    import torch

    from vstab_amd import native

    a = torch.zeros((2, 8, 9), device=ctx.device)
    ctx.set_timing(True)
    try:
        ctx.mask_moments_batch(a)                        # so that the timing kind exists
        ctx.set_timing(True)                             # clears the totals
        with pytest.raises(ValueError, match="mask_moments_batch: mask must be a contiguous float32"):
            ctx.mask_moments_batch(a.double())
        with pytest.raises(ValueError, match="mask_moments_batch: mask must be a contiguous float32"):
            ctx.mask_moments_batch(a.transpose(1, 2))                          # not contiguous
        with pytest.raises(ValueError, match="mask_moments_batch: mask must be a contiguous float32"):
            ctx.mask_moments_batch(a.cpu())
        with pytest.raises(ValueError, match=r"mask_moments_batch: mask of shape \(2, 8, 9, 1\) is not \[n,h,w\]"):
            ctx.mask_moments_batch(a[..., None])
        with pytest.raises(native.VstabError, match="vstab_mask_moments_batch: bad shape n=0"):
            ctx.mask_moments_batch(a[:0])
        with pytest.raises(native.VstabError, match="vstab_mask_moments_batch: 40000 x 1 pixels, the limit is 32768 per axis"):
            ctx.mask_moments_batch(torch.zeros((1, 1, 40000), device=ctx.device))
        assert ctx.kernel_ms_stats("mask_moments")[1] == 0
    finally:
        ctx.set_timing(False)


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H, N = 160, 96, 12
ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1
# the disc's integer centres: a fixed zig-zag of up to +-14 px around (80, 48).  Radius <= 12: never within 12 px of a
# border.  The extremes are symmetric on both axes, so crop_and_pad's recentring offset (max + min) / 2 is 0 and every
# frame's total shift is an integer: the bilinear warp then copies pixels.
ZIG_X = [0, 5, -3, 9, -7, 14, -14, 8, -2, 11, -6, 3]
ZIG_Y = [0, -4, 6, -8, 10, -12, 12, -5, 7, -3, 2, -1]
CENTRES = [(80 + dx, 48 + dy) for dx, dy in zip(ZIG_X, ZIG_Y)]


def _subject_clip(radii):
    """12 frames of tests.util.synth_frames at 0.45 of their amplitude (every background sample below 0.5, so that "> 0.5"
    finds the disc alone), a saturated disc (1.0 in all channels) painted at CENTRES; the mask is the disc.
    -> (frames f32 [N,H,W,3], mask f32 [N,H,W]), NumPy."""
    frames = synth_frames(N, H, W, seed=5) * np.float32(0.45)
    assert frames.max() < 0.5
    mask = np.stack([R.disc(H, W, cx, cy, r) for (cx, cy), r in zip(CENTRES, radii)])
    frames[mask > 0.5] = 1.0
    for (cx, cy), r in zip(CENTRES, radii):
        assert min(cx - r, cy - r, W - 1 - cx - r, H - 1 - cy - r) >= 12
    return frames, mask


@pytest.fixture(scope="module")
def disc_clip(ctx):
    frames, mask = _subject_clip([9] * N)
    return _dev(ctx, frames), _dev(ctx, mask), frames, mask


def _stabilize(ctx, frames, transform="translation", framing="crop_and_pad", estimator="subject", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, transform, *ARGS, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


@pytest.fixture(scope="module")
def locked(pkg, ctx, disc_clip):
    return _stabilize(ctx, disc_clip[0], subject_mask=disc_clip[1])


def _transitions(meta):
    return np.array([t["matrix"] for t in meta["estimated_motion"]["per_transition"]], np.float64)


def _disc_centroids(result):
    """Centroid of the pixels whose painted channel is > 0.5 and whose returned mask is 0, per returned frame."""
    frames, pad = result.frames.cpu().numpy(), result.masks.cpu().numpy().reshape(result.frames.shape[:3])
    out = []
    for f, m in zip(frames, pad):
        ys, xs = np.nonzero((f[..., 0] > 0.5) & (m == 0.0))
        assert xs.size > 0
        out.append((xs.mean(), ys.mean()))
    return np.array(out, np.float64)


def test_translation_lock_holds_the_disc_still(pkg, ctx, disc_clip, locked):
    meta = locked.meta
    known = np.diff(np.array(CENTRES, np.float64), axis=0)
    t = _transitions(meta)
    err = np.abs(t[:, :2, 2] - known).max()
    print("largest transition error, px:", err)
    assert err <= 1e-4                                   # float32 rounding of a value below 32 px
    assert np.array_equal(t[:, :2, :2], np.tile(np.eye(2), (N - 1, 1, 1)))
    assert meta["subject_lock"]["centroid"] == [[float(x), float(y)] for x, y in CENTRES]
    assert meta["subject_lock"]["frames_without_subject"] == 0 and meta["subject_lock"]["interpolated"] == []
    assert meta["subject_lock"]["mask_frames"] == N and meta["subject_lock"]["frames_touching_border"] == 0
    assert meta["flow_backend"] == "subject_mask" and meta["flow_fallback_reason"] is None
    assert meta["motion_meta"]["source"] == "estimated_subject"
    assert meta["transform_mode_applied"] == "translation"
    assert [p["confidence"] for p in meta["estimated_motion"]["per_transition"]] == [1.0] * (N - 1)
    assert [p["residual"] for p in meta["estimated_motion"]["per_transition"]] == [0.0] * (N - 1)
    c = _disc_centroids(locked)
    spread = np.abs(c - c[0]).max()
    print("disc centroid in the returned frames:", c[0], "largest deviation, px:", spread)
    assert spread <= 0.05                                # the project's analytic gate (tests/test_analytic_gpu.py)
    assert not locked.device_plan["used"] and json.loads(json.dumps(meta)) == meta
    # a host tensor and a NumPy array are the same request
    for m in (disc_clip[1].cpu(), disc_clip[3]):
        again = _stabilize(ctx, disc_clip[0], subject_mask=m)
        assert np.array_equal(_bits(again.frames), _bits(locked.frames)) and json.dumps(again.meta) == json.dumps(meta)


def test_similarity_follows_the_area(pkg, ctx):
    radii = [9 if k % 2 == 0 else 12 for k in range(N)]
    frames, mask = _subject_clip(radii)
    sums, _ = R.moments(mask)
    want = np.sqrt(sums[1:, 0] / sums[:-1, 0].astype(np.float64))       # of the rasterised discs, not of pi r^2
    run = _stabilize(ctx, _dev(ctx, frames), "similarity", subject_mask=_dev(ctx, mask))
    t = _transitions(run.meta)
    rel = np.abs(t[:, 0, 0] / want - 1.0).max()
    print("largest relative scale error:", rel)
    assert rel <= 0.02 and np.abs(t[:, 1, 1] / want - 1.0).max() <= 0.02
    assert np.abs(t[:, 0, 1]).max() == 0.0 and np.abs(t[:, 1, 0]).max() == 0.0     # no rotation
    assert run.meta["transform_mode_applied"] == "similarity" and run.meta["subject_lock"]["centroid"] == [[float(x), float(y)] for x, y in CENTRES]
    ctx.set_timing(True)
    try:
        ctx.mask_moments_batch(_dev(ctx, mask[:1]))      # so that the timing kind exists
        ctx.set_timing(True)                             # clears the totals
        with pytest.raises(ValueError, match="transform_mode='perspective' is not supported with estimator 'subject'"):
            _stabilize(ctx, _dev(ctx, frames), "perspective", subject_mask=_dev(ctx, mask))
        assert ctx.kernel_ms_stats("mask_moments")[1] == 0                          # before any launch
    finally:
        ctx.set_timing(False)


def test_gaps_are_interpolated_and_reported(pkg, ctx, disc_clip):
    mask = disc_clip[3].copy()
    mask[4:6] = 0.0
    run = _stabilize(ctx, disc_clip[0], subject_mask=_dev(ctx, mask))
    block = run.meta["subject_lock"]
    assert block["frames_without_subject"] == 2 and block["interpolated"] == [4, 5] and block["mask_frames"] == N
    conf = [p["confidence"] for p in run.meta["estimated_motion"]["per_transition"]]
    assert [k for k, v in enumerate(conf) if v == 0.0] == [3, 4, 5] and all(v > 0.0 for k, v in enumerate(conf) if k not in (3, 4, 5))
    assert tuple(run.frames.shape) == (N, H, W, 3) and len(block["centroid"]) == N
    c = np.array(block["centroid"])
    assert np.allclose(c[4], (2 * c[3] + c[6]) / 3, rtol=0, atol=1e-9) and np.allclose(c[5], (c[3] + 2 * c[6]) / 3, rtol=0, atol=1e-9)
    all_empty = np.zeros_like(mask)
    with pytest.raises(ValueError, match="subject_mask holds no subject pixel"):
        _stabilize(ctx, disc_clip[0], subject_mask=_dev(ctx, all_empty))


def test_composition_and_refusals(pkg, ctx, disc_clip, locked):
    frames, mask = disc_clip[0], disc_clip[1]
    for kw, key in ((dict(spatial_fill=True), "spatial_fill"), (dict(stability_report=True), "stability"),
                    (dict(dynamic_zoom=True), "dynamic_zoom"), (dict(scene_cuts=[6]), "scene_cuts")):
        run = _stabilize(ctx, frames, subject_mask=mask, **kw)
        assert key in run.meta and "subject_lock" in run.meta and key not in locked.meta, key
        assert run.meta["subject_lock"] == locked.meta["subject_lock"]
    for kw, text in ((dict(temporal_fill=2), "temporal_fill=2 is not supported with estimator 'subject'"),
                     (dict(scene_cuts="auto"), "scene_cuts='auto' is not supported with estimator 'subject'"),
                     (dict(estimation_mask=mask), "estimation_mask is not supported with estimator 'subject'"),
                     (dict(mesh_warp=True), "mesh_warp is not supported with estimator 'subject'")):
        with pytest.raises(ValueError, match=text):
            _stabilize(ctx, frames, subject_mask=mask, **kw)
    for framing in ("expand", "crop"):
        run = _stabilize(ctx, frames, framing=framing, subject_mask=mask)
        assert run.meta["subject_lock"] == locked.meta["subject_lock"] and run.meta["framing"]["mode"] == framing


def test_value_range_rule_is_honoured_without_a_gray_pass(pkg, ctx, disc_clip, locked):
    """0..255 float input (F0): the frames' maxima come from a pass of their own, the clip is rescaled and the cheap
    estimation repeated.  The result is that of the clip divided by 255 beforehand (IEEE float32 division, NumPy), bit for bit."""
    import torch

    big = disc_clip[2] * np.float32(255.0)
    assert big.reshape(N, -1).max(axis=1).min() > 1.5
    a = _stabilize(ctx, torch.from_numpy(big / np.float32(255.0)).to(ctx.device), subject_mask=disc_clip[1])
    b = _stabilize(ctx, torch.from_numpy(big).to(ctx.device), subject_mask=disc_clip[1])
    assert np.array_equal(_bits(a.frames), _bits(b.frames)) and np.array_equal(_bits(a.masks), _bits(b.masks))
    assert json.dumps(a.meta, sort_keys=True) == json.dumps(b.meta, sort_keys=True)
    assert json.dumps(a.meta["subject_lock"]) == json.dumps(locked.meta["subject_lock"])
    assert float(b.frames.max()) <= 1.0


def test_the_default_path_is_untouched(pkg, ctx, disc_clip):
    ctx.set_timing(True)
    try:
        ctx.mask_moments_batch(disc_clip[1][:1])         # so that the timing kind exists
        ctx.set_timing(True)                             # clears the totals
        plain = _stabilize(ctx, disc_clip[0], "similarity", estimator="flow")
        off = _stabilize(ctx, disc_clip[0], "similarity", estimator="flow", subject_mask=None)
        assert ctx.kernel_ms_stats("mask_moments")[1] == 0                          # nothing new is launched
        _stabilize(ctx, disc_clip[0], subject_mask=disc_clip[1])
        assert ctx.kernel_ms_stats("mask_moments")[1] == 1                          # one launch per clip
    finally:
        ctx.set_timing(False)
    assert np.array_equal(_bits(plain.frames), _bits(off.frames)) and np.array_equal(_bits(plain.masks), _bits(off.masks))
    assert json.dumps(plain.meta) == json.dumps(off.meta) and "subject_lock" not in off.meta
    assert plain.meta["flow_backend"] == "DIS"
    with pytest.raises(ValueError, match="subject_mask needs estimator='subject', got estimator='flow'"):
        _stabilize(ctx, disc_clip[0], estimator="flow", subject_mask=disc_clip[1])
    with pytest.raises(ValueError, match="estimator='subject' needs subject_mask"):
        _stabilize(ctx, disc_clip[0])


def test_motion_apply_replays_the_lock(pkg, ctx, disc_clip, locked):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    meta = json.loads(json.dumps(locked.meta))
    out = ap.apply_motion(hm._normalize_video_input(disc_clip[0]), meta, (127, 127, 127), ctx=ctx, keep_on_device=True)
    assert out.meta["motion_apply"]["source"] == "estimated_subject"
    c = _disc_centroids(out)                             # the recorded lock, applied again: the disc stands still
    assert np.abs(c - c[0]).max() <= 0.05


def test_node(pkg, ctx, disc_clip, locked):
    import asyncio

    from vstab_amd import nodes

    out = nodes.VideoStabilizerFlowSubject.execute(disc_clip[0].cpu(), 16.0, "crop_and_pad", "translation", True, 1.0, 0.5, 0.6,
                                                   "#7F7F7F", disc_clip[1].cpu())
    frames, mask, meta = out[0], out[1], out[2]
    block = json.loads(json.dumps(meta))["subject_lock"]
    assert block == locked.meta["subject_lock"] and block["version"] == 1
    assert tuple(frames.shape) == (N, H, W, 3) and tuple(mask.shape) == (N, H, W)
    assert np.array_equal(np.asarray(frames.cpu()).view(np.uint32), _bits(locked.frames))
    assert len(nodes.NODE_CLASSES) == 6 and nodes.VideoStabilizerFlowSubject not in nodes.NODE_CLASSES
    entry = asyncio.run(pkg.comfy_entrypoint())
    assert type(entry) is nodes.VideoStabilizerAmdMaskedExtension
    assert asyncio.run(entry.get_node_list()) == list(nodes.NODE_CLASSES) + [nodes.VideoStabilizerTemporalFill, nodes.VideoStabilizerFlowMasked]
