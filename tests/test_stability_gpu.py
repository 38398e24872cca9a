"""GPU: vstab_frame_sse_batch (csrc/vstab_stability.hip), the `stability_report` keyword and the report node.

sse and count are integers and must equal the NumPy restatement (tests/stability_restatement.py, whose properties are
checked on the CPU in tests/test_stability_cpu.py) exactly: no tolerance anywhere.  The kernel takes one of two paths per
pair -- float4 loads where a[k] and b[k] sit at the same offset from a 16-byte boundary, one float per lane where they do
not -- so every shape runs in both forms: a and b as tensors of their own (same offset; frames k >= 1 of an odd-sized clip
start off the boundary: a head and a tail) and as the consecutive form of one clip (offsets differ for odd-sized frames).
"""

import json

import numpy as np
import pytest

from tests import stability_restatement as R
from tests.util import shake_path, synth_frames

pytestmark = pytest.mark.gpu

MASK_VALUES = np.array([0.0, 1.0, 0.5, np.nan, np.inf, 0.0, 0.0], np.float32)

# (n, h, w): a single pixel; one row; frame sizes that are no multiple of 16 bytes (3 x 13 x 67 floats: frame k starts k floats
# past the boundary); a frame of whole float4s (8 x 64 pixels, half a tile of 1024); 9 x 130 = one tile and a part; 37 x 253 =
# ten tiles, a workgroup each; 13 x 79 = one tile and three pixels: the second workgroup sums over two lanes of one wave
SHAPES = [(1, 1, 1), (3, 1, 67), (3, 13, 67), (4, 8, 64), (2, 9, 130), (5, 37, 253), (2, 13, 79)]


def _dev(ctx, x):
    import torch

    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(ctx.device).contiguous()


def _call(ctx, a, b, ma=None, mb=None):
    sse, count = ctx.frame_sse_batch(a, b, ma, mb)
    assert str(sse.dtype) == "torch.int64" and str(count.dtype) == "torch.int32"
    return [int(v) for v in sse.cpu().numpy()], [int(v) for v in count.cpu().numpy()]


def _want(a, b, ma=None, mb=None):
    sse, count = R.frame_sse(a, b, ma, mb)
    return [int(v) for v in sse], [int(v) for v in count]


def _masks(rng, n, h, w):
    """Two masks of 0 / 1 / 0.5 / NaN / inf; pair 0 has all pixels valid in mask_a; the last pair has no common valid pixel
    (where there is more than one pair)."""
    ma = MASK_VALUES[rng.integers(0, len(MASK_VALUES), (n, h, w))]
    mb = MASK_VALUES[rng.integers(0, len(MASK_VALUES), (n, h, w))]
    ma[0] = 0.0
    if n > 1:
        ma[-1] = np.where(R.valid_of(mb[-1], (h, w)), np.float32(1.0), np.float32(0.0))
    return ma, mb


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_restatement(ctx, shape):
    n, h, w = shape
    rng = np.random.default_rng(n * 10007 + h * 101 + w)
    a = rng.uniform(0.0, 1.0, (n, h, w, 3)).astype(np.float32)
    b = (rng.integers(0, 256, (n, h, w, 3)).astype(np.float32) / np.float32(255.0)).astype(np.float32)     # k / 255 values
    ma, mb = _masks(rng, n, h, w)
    da, db, dma, dmb = (_dev(ctx, x) for x in (a, b, ma, mb))
    keep = [t.clone() for t in (da, db, dma, dmb)]
    for use_a, use_b in ((False, False), (True, False), (False, True), (True, True)):
        got = _call(ctx, da, db, dma if use_a else None, dmb if use_b else None)
        want = _want(a, b, ma if use_a else None, mb if use_b else None)
        assert got == want, (shape, use_a, use_b)
        if not use_a and not use_b:
            assert got[1] == [h * w] * n
        if use_a and use_b and n > 1:
            assert got[0][-1] == 0 and got[1][-1] == 0                     # no common valid pixel
        if use_a and not use_b:
            assert got[1][0] == h * w                                        # all pixels valid
    for t, k in zip((da, db, dma, dmb), keep):                               # nothing is written to the inputs
        assert np.array_equal(t.cpu().numpy().view(np.uint32), k.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES + [(6, 13, 67)], ids=lambda s: "x".join(map(str, s)))
def test_consecutive_form_equals_restatement_and_separate_calls(ctx, shape):
    """b = a + one frame over a clip of n + 1 frames, masks included; equal to n one-pair calls on copies of the frames.
    6 x 13 x 67: six pairs (seven frames) of an odd-sized clip, every frame at another offset from the 16-byte boundary."""
    n, h, w = shape
    rng = np.random.default_rng(n * 7 + h * 3 + w)
    clip = synth_frames(n + 1, h, w, seed=n + h + w)
    mask = MASK_VALUES[rng.integers(0, len(MASK_VALUES), (n + 1, h, w))]
    d, m = _dev(ctx, clip), _dev(ctx, mask)
    for with_mask in (False, True):
        got = _call(ctx, d[:-1], d[1:], m[:-1] if with_mask else None, m[1:] if with_mask else None)
        want = R.consecutive(clip, mask if with_mask else None)
        assert got == ([int(v) for v in want[0]], [int(v) for v in want[1]]), (shape, with_mask)
        for k in range(n):
            one = _call(ctx, d[k:k + 1].clone(), d[k + 1:k + 2].clone(), m[k:k + 1].clone() if with_mask else None,
                        m[k + 1:k + 2].clone() if with_mask else None)
            assert (one[0][0], one[1][0]) == (got[0][k], got[1][k]), (shape, with_mask, k)


def test_more_tiles_than_workgroups(ctx):
    """2 pairs of 1031 x 2101 pixels: 2116 tiles per pair for 2048 workgroups, so some workgroups loop over two tiles -- as
    two clips (float4 path, pair 1 behind a head) and as the consecutive form (an odd pixel count: the one-float path)."""
    n, h, w = 2, 1031, 2101
    rng = np.random.default_rng(21)
    clip = rng.integers(0, 256, (n + 1, h, w, 3)).astype(np.float32) / np.float32(255.0)
    mask = (rng.uniform(0.0, 1.0, (n + 1, h, w)) < 0.1).astype(np.float32)
    d, m = _dev(ctx, clip), _dev(ctx, mask)
    want = R.consecutive(clip, mask)
    want = ([int(v) for v in want[0]], [int(v) for v in want[1]])
    assert _call(ctx, d[:-1], d[1:], m[:-1], m[1:]) == want
    assert _call(ctx, d[:-1].clone(), d[1:].clone(), m[:-1].clone(), m[1:].clone()) == want


def test_planted_non_finite_values_take_the_cap(ctx):
    n, h, w = 3, 13, 67
    rng = np.random.default_rng(11)
    a = rng.uniform(0.0, 1.0, (n, h, w, 3)).astype(np.float32)
    b = rng.uniform(0.0, 1.0, (n, h, w, 3)).astype(np.float32)
    planted = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    for arr, seed in ((a, 1), (b, 2)):
        r = np.random.default_rng(seed)
        for v in planted:
            for _ in range(6):
                arr[r.integers(n), r.integers(h), r.integers(w), r.integers(3)] = v
    a[0, 0, 0], b[0, 0, 0] = np.inf, np.inf                                  # inf - inf = NaN
    ma, mb = _masks(rng, n, h, w)
    for x, y in ((ma, mb), (None, None)):
        got = _call(ctx, _dev(ctx, a), _dev(ctx, b), _dev(ctx, x), _dev(ctx, y))
        assert got == _want(a, b, x, y)
    assert _want(a, b)[0][0] >= 3 * 2 ** 34


def test_sums_above_32_bits(ctx):
    """64 x 64 pixels with every difference at 2 or more: sse = 3 * 64 * 64 * 2^34, far above 2^32 (64-bit accumulation from
    the thread to the atomic)."""
    rng = np.random.default_rng(3)
    a = rng.uniform(2.0, 5.0, (1, 64, 64, 3)).astype(np.float32)
    b = np.zeros_like(a)
    a[0, ::2] *= -1.0
    got = _call(ctx, _dev(ctx, a), _dev(ctx, b))
    assert got == ([3 * 64 * 64 * 2 ** 34], [64 * 64]) == _want(a, b)


def test_a_against_itself(ctx):
    n, h, w = 3, 13, 67
    a = synth_frames(n, h, w, seed=4)
    ma, _ = _masks(np.random.default_rng(5), n, h, w)
    d, m = _dev(ctx, a), _dev(ctx, ma)
    assert _call(ctx, d, d) == ([0] * n, [h * w] * n)
    assert _call(ctx, d, d, m, m) == ([0] * n, [int(v) for v in R.valid_of(ma, ma.shape).reshape(n, -1).sum(axis=1)])


def test_two_runs_are_identical(ctx):
    n, h, w = 5, 37, 253
    rng = np.random.default_rng(8)
    a, b = synth_frames(n, h, w, seed=1), synth_frames(n, h, w, seed=2)
    ma, mb = _masks(rng, n, h, w)
    args = [_dev(ctx, x) for x in (a, b, ma, mb)]
    first, second = _call(ctx, *args), _call(ctx, *args)
    assert first == second == _want(a, b, ma, mb)


def test_argument_errors_come_before_any_launch(ctx):
    import torch

    from vstab_amd import native

    a = torch.zeros((2, 8, 9, 3), device=ctx.device)
    ctx.set_timing(True)
    try:
        ctx.frame_sse_batch(a, a)                     # so that the timing kind exists
        ctx.set_timing(True)                          # clears the totals
        with pytest.raises(native.VstabError, match="vstab_frame_sse_batch: bad shape n=0"):
            ctx.frame_sse_batch(a[:0], a[:0])
        with pytest.raises(ValueError, match=r"mask_a of shape \(2, 9, 8\) does not match"):
            ctx.frame_sse_batch(a, a, torch.zeros((2, 9, 8), device=ctx.device))
        with pytest.raises(ValueError, match=r"mask_b of shape \(1, 8, 9\) does not match"):
            ctx.frame_sse_batch(a, a, None, torch.zeros((1, 8, 9), device=ctx.device))
        with pytest.raises(ValueError, match=r"b of shape \(1, 8, 9, 3\) does not match"):
            ctx.frame_sse_batch(a, a[:1])
        with pytest.raises(ValueError, match="a must be a contiguous float32"):
            ctx.frame_sse_batch(a.double(), a)
        assert ctx.kernel_ms_stats("stability")[1] == 0
    finally:
        ctx.set_timing(False)


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H, N = 160, 96, 12
ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1
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


def _same_outputs(x, y):
    return (np.array_equal(x.frames.cpu().numpy().view(np.uint32), y.frames.cpu().numpy().view(np.uint32))
            and np.array_equal(x.masks.cpu().numpy().view(np.uint32), y.masks.cpu().numpy().view(np.uint32)))


def _expected(source, result, masked=True, cuts=None):
    before = R.itf_block(source.cpu().numpy(), None, cuts or ())
    after = R.itf_block(result.frames.cpu().numpy(), result.masks.cpu().numpy()[..., 0] if masked else None, cuts or ())
    return R.report(before, after, None if cuts is None else len(cuts))


@pytest.mark.parametrize("framing,estimator,extra", [
    ("crop_and_pad", "flow", {}), ("expand", "flow", {}), ("crop", "flow", {}), ("crop_and_pad", "classic", {}),
    ("crop_and_pad", "flow", dict(temporal_fill=2, spatial_fill=True)), ("crop_and_pad", "flow", dict(mesh_warp=(4, 3)))],
    ids=["flow", "expand", "crop", "classic", "fills", "mesh"])
def test_pipeline_keyword(pkg, ctx, clip, framing, estimator, extra):
    ctx.set_timing(True)
    try:
        ctx.frame_sse_batch(clip[:1], clip[:1])                                    # so that the timing kind exists
        ctx.set_timing(True)                                                       # clears the totals
        plain = _stabilize(ctx, clip, framing, estimator, **extra)                 # the parent's call
        off = _stabilize(ctx, clip, framing, estimator, stability_report=False, **extra)
        assert ctx.kernel_ms_stats("stability")[1] == 0                            # False launches nothing
        on = _stabilize(ctx, clip, framing, estimator, stability_report=True, **extra)
        assert ctx.kernel_ms_stats("stability")[1] == 2                            # one launch per clip
    finally:
        ctx.set_timing(False)
    assert _same_outputs(off, plain) and json.dumps(off.meta) == json.dumps(plain.meta) and "stability" not in off.meta
    assert _same_outputs(on, off)
    meta_on = dict(on.meta)
    block = meta_on.pop("stability")
    assert json.dumps(meta_on) == json.dumps(off.meta)
    want = _expected(clip, on, masked=framing != "crop")
    assert block == want and json.loads(json.dumps(block)) == block
    assert block["before"]["pairs"] == block["after"]["pairs"] == N - 1 and "pairs_across_cuts" not in block
    if framing != "crop":                                                          # the mask matters: without it the figures differ
        assert on.masks.max() > 0.5 and block["after"]["overlap_fraction_mean"] < 1.0
        assert block["after"] != R.itf_block(on.frames.cpu().numpy(), None)
    if framing == "crop_and_pad" and estimator == "flow" and not extra:
        assert on.device_plan["used"]                                              # the device-plan path


def test_pipeline_scene_cuts_leave_the_pair_across_the_cut_out(pkg, ctx, clip):
    import torch

    import bench

    other = bench.synth_clip(N - 6, 0, H, W, torch.device("cuda"), seed=99, mats=shake_path(N - 6, W, H, "similarity", seed=4, amp=SHAKE_AMP))
    two_shots = torch.cat([clip[:6], other]).contiguous()
    off = _stabilize(ctx, two_shots, scene_cuts=[6])
    on = _stabilize(ctx, two_shots, scene_cuts=[6], stability_report=True)
    meta_on = dict(on.meta)
    block = meta_on.pop("stability")
    assert _same_outputs(on, off) and json.dumps(meta_on) == json.dumps(off.meta)
    assert block == _expected(two_shots, on, cuts=[6])
    assert block["pairs_across_cuts"] == 1 and block["before"]["pairs"] == block["after"]["pairs"] == N - 2
    # with the pair across the cut the figures would be other ones
    with_cut_pair = R.itf_block(two_shots.cpu().numpy())
    assert with_cut_pair["pairs"] == N - 1 and with_cut_pair["itf_db"] != block["before"]["itf_db"]


def _apply(ctx, frames, meta, **kw):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    return ap.apply_motion(hm._normalize_video_input(frames), meta, (127, 127, 127), ctx=ctx, keep_on_device=True, **kw)


def test_motion_apply_keyword(pkg, ctx, clip):
    run = _stabilize(ctx, clip)
    meta = json.loads(json.dumps(run.meta))
    for kw in (dict(), dict(framing_mode="expand"), dict(interpolation="bicubic", spatial_fill=True), dict(framing_mode="crop")):
        base = _apply(ctx, clip, meta, **kw)
        off = _apply(ctx, clip, meta, stability_report=False, **kw)
        on = _apply(ctx, clip, meta, stability_report=True, **kw)
        assert _same_outputs(off, base) and json.dumps(off.meta) == json.dumps(base.meta)
        assert "stability" not in off.meta["motion_apply"] and _same_outputs(on, base)
        meta_on = json.loads(json.dumps(on.meta))
        block = meta_on["motion_apply"].pop("stability")
        assert json.dumps(meta_on) == json.dumps(base.meta), kw
        assert block == _expected(clip, on, masked=on.meta["motion_apply"]["framing_mode"] != "crop"), kw
    with pytest.raises(ValueError, match="stability_report=True is not supported with motion_blur=0.4"):
        _apply(ctx, clip, meta, motion_blur=0.4, stability_report=True)


def test_locked_camera_gains(pkg, ctx):
    """Not a tolerance on the code under test, a sanity check of the figure's sign: the analytic translation shake of
    tests/test_analytic_gpu.py, stabilized with camera_lock and strength 1, must come out steadier than it went in.  (The
    restatement alone shows the same sign on a clip of this kind: tests/test_stability_cpu.py.)"""
    import torch

    import bench
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    w, h, n = 960, 540, 12
    frames = bench.synth_clip(n, 0, h, w, torch.device("cuda"), mats=shake_path(n, w, h, "translation", seed=5, amp=1.0))
    res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "translation", True, 1.0, 0.5, 0.6, (127, 127, 127),
                               16.0, ctx=ctx, keep_on_device=True, stability_report=True)
    block = res.meta["stability"]
    print(block)
    assert block["before"]["itf_db"] is not None and block["after"]["itf_db"] is not None
    assert block["gain_db"] > 0 and block["gain_db"] == block["after"]["itf_db"] - block["before"]["itf_db"]


def test_node_on_cpu_tensors(pkg, ctx, clip):
    from vstab_amd import nodes

    run = _stabilize(ctx, clip)
    frames, mask, reference = run.frames.cpu(), run.masks[..., 0].cpu(), clip.cpu()
    keep = frames.clone()

    def call(*args, **kw):
        out = nodes.VideoStabilizerStabilityReport.execute(*args, **kw)
        (text,) = out.result if hasattr(out, "result") else out.args
        assert isinstance(text, str)
        return json.loads(text)

    after = R.itf_block(frames.numpy(), mask.numpy())
    before = R.itf_block(reference.numpy())
    assert call(frames, mask, reference) == {"stability": R.report(before, after)}
    assert call(frames, padding_mask=mask) == {"stability": R.report(None, after)}
    assert call(frames) == {"stability": R.report(None, R.itf_block(frames.numpy()))}
    one = mask[:1]                                                                 # one mask for every frame
    assert call(frames, one) == {"stability": R.report(None, R.itf_block(frames.numpy(), one.expand(N, H, W).numpy()))}
    assert np.array_equal(frames.numpy().view(np.uint32), keep.numpy().view(np.uint32))
