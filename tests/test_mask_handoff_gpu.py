"""GPU: the mask hand-off kernels (csrc/vstab_handoff.hip) against tests/mask_handoff_restatement.py.  There is no tolerance
anywhere: every comparison is `view(np.uint32)` equality.  The shapes are the places where the kernel can break -- one pixel,
one row, a frame smaller than every radius, exactly one 64 x 32 core tile and one more row and column than that, the
+-1 neighbours of tile + halo (80 x 48) and of the widest staged region (96 x 64), widths that are no multiple of 4 -- and
the radii are those around a pass boundary (16 steps), with both footprints."""

import json

import numpy as np
import pytest

from tests import mask_handoff_restatement as R
from tests.util import shake_path

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 1, 67), (2, 5, 3), (2, 31, 63), (2, 32, 64), (2, 33, 65), (1, 47, 79), (1, 48, 80), (1, 49, 81), (1, 63, 95),
          (1, 64, 96), (1, 65, 97), (3, 67, 131), (2, 131, 197)]
SMALL = [(1, 1, 1), (2, 5, 3), (2, 33, 65), (1, 49, 81), (2, 67, 131)]        # where the restatement's feather (O(f^2) array passes) stays quick
GROWS = [0, 1, 2, 5, 15, 16, 17, 32, 33, 64, -1, -5, -17, -64]
FEATHERS = [0, 1, 5, 16, 17, 64]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ctx.device)


def _grow(ctx, m, g, tapered=True, f=0):
    out, count = ctx.mask_grow_batch(_dev(ctx, m), g, tapered=tapered, feather=f, want_count=True)
    return out.cpu().numpy(), count.cpu().numpy().astype(np.uint32)


def _check(ctx, m, g, tapered, f, what=""):
    got, count = _grow(ctx, m, g, tapered, f)
    want, want_count = R.grow_feather(m, g, tapered, f)
    where = f"{what} shape {m.shape} grow {g} tapered {tapered} feather {f}"
    assert got.shape == want.shape, where
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{where}: {len(bad)} pixels differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    assert count.tolist() == want_count.tolist(), where


def _masks(shape, seed):
    yield "table", R.random_mask(shape, seed)
    yield "sparse", R.random_mask(shape, seed + 1, sparse=True)
    yield "corners", R.corner_mask(*shape)


# ---- grow --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tapered", [True, False], ids=["tapered", "square"])
@pytest.mark.parametrize("g", GROWS)
def test_grow_equals_restatement(ctx, g, tapered):
    for k, shape in enumerate(SHAPES):
        for what, m in _masks(shape, 1000 + 37 * k + abs(g)):
            if what == "table" or abs(g) in (1, 16, 17, 64):
                _check(ctx, m, g, tapered, 0, what)


# ---- feather, alone and behind a grow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tapered", [True, False], ids=["tapered", "square"])
@pytest.mark.parametrize("f", FEATHERS)
def test_feather_equals_restatement(ctx, f, tapered):
    for k, shape in enumerate(SHAPES if f <= 17 else SMALL):
        for what, m in _masks(shape, 2000 + 41 * k + f):
            if what != "table" or f <= 5:                 # (dense random values leave a ramp nowhere to go: the sparse ones carry it)
                _check(ctx, m, 0, tapered, f, what)


@pytest.mark.parametrize("tapered", [True, False], ids=["tapered", "square"])
@pytest.mark.parametrize("g,f", [(17, 17), (5, 5), (11, 5), (15, 1), (16, 1), (16, 16), (-5, 16), (-17, 17), (33, 17), (64, 64), (-64, 64), (1, 64)])
def test_grow_then_feather_equals_restatement(ctx, g, f, tapered):
    """(11, 5): both kinds of step inside one pass; (15, 1) / (16, 1): the switch at the pass boundary and one before it."""
    for k, shape in enumerate(SMALL + [(2, 32, 64)]):
        _check(ctx, R.random_mask(shape, 3000 + 43 * k + f, sparse=True), g, tapered, f, "sparse")
    _check(ctx, R.corner_mask(2, 49, 81), g, tapered, f, "corners")
    if f <= 17:
        _check(ctx, R.random_mask((2, 131, 197), 3100 + f, sparse=True), g, tapered, f, "sparse")


def test_nothing_crosses_from_one_frame_into_another(ctx):
    for h, w in ((5, 3), (33, 65), (67, 131)):
        m = np.zeros((3, h, w), np.float32)
        m[1] = 1.0
        for g, f, tapered in ((5, 0, True), (64, 0, False), (0, 64, True), (17, 17, False), (33, 5, True)):
            got, count = _grow(ctx, m, g, tapered, f)
            assert not got[0].any() and not got[2].any() and (got[1] == 1).all(), (h, w, g, f)
            assert count.tolist() == [0, h * w, 0]
        got, count = _grow(ctx, 1 - m, -17, True, 0)                     # and no minimum either
        assert (got[0] == 1).all() and (got[2] == 1).all() and not got[1].any() and count.tolist() == [h * w, 0, h * w]


def test_zero_steps_keep_the_bits_and_the_input_is_never_written(ctx):
    m = R.random_mask((2, 33, 65), 7)
    assert np.isnan(m).any()
    src = _dev(ctx, m)
    for tapered in (True, False):
        out, count = ctx.mask_grow_batch(src, 0, tapered=tapered, feather=0, want_count=True)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(m)) and count.cpu().numpy().tolist() == R.count_above(m).tolist()
    assert isinstance(ctx.mask_grow_batch(src, 3), ctx.torch.Tensor)       # without want_count: the mask alone
    ctx.mask_grow_batch(src, 64, feather=64)
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(m))


def test_invalid_arguments_are_refused(ctx):
    torch = ctx.torch
    m = torch.zeros((2, 8, 12), device=ctx.device)
    with pytest.raises(ValueError, match="out shares memory with mask"):
        ctx.mask_grow_batch(m, 1, out=m)
    big = torch.zeros((3, 8, 12), device=ctx.device)
    with pytest.raises(ValueError, match="out shares memory with mask"):
        ctx.mask_grow_batch(big[:2], 1, out=big[1:])
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
        ctx.mask_grow_batch(m, 1, out=torch.zeros((2, 8, 13), device=ctx.device))
    for bad in (m.cpu(), m.double(), m[:, :, ::2], m[0], None):
        with pytest.raises(ValueError, match="mask_grow_batch: mask"):
            ctx.mask_grow_batch(bad, 1)
        with pytest.raises(ValueError, match="mask_hold_batch: mask"):
            ctx.mask_hold_batch(bad, 1)
    for kw, word in ((dict(grow=65), "grow=65"), (dict(grow=True), "grow=True"), (dict(grow=1.0), "grow=1.0"), (dict(grow=1, feather=65), "feather=65"),
                     (dict(grow=1, feather=-1), "feather=-1"), (dict(grow=1, tapered=1), "tapered=1")):
        with pytest.raises(ValueError, match=word):
            ctx.mask_grow_batch(m, **kw)
    for hold, word in ((17, "hold=17"), (-1, "hold=-1"), (True, "hold=True"), (1.0, "hold=1.0")):
        with pytest.raises(ValueError, match=word):
            ctx.mask_hold_batch(m, hold)
    for shots in ([0], [1, 0], [[0, 1]] * 2):
        with pytest.raises(ValueError, match="shots"):
            ctx.mask_hold_batch(m, 1, shots)


# ---- hold --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 40])
@pytest.mark.parametrize("T", [0, 1, 2, 16])
def test_hold_equals_restatement(ctx, n, T):
    """7 x 9 and 5 x 13: frames that do not start on 16-byte boundaries (one float per lane); 8 x 12 and 33 x 64: the float4 path."""
    cut = np.zeros(n, np.int32)
    cut[n // 2:] = 3                                       # a cut inside every window that reaches across the middle
    cut[n - 1] += 1 if n >= 5 else 0                       # and a shot of one frame at the end
    for k, (h, w) in enumerate(((7, 9), (8, 12), (5, 13), (33, 64), (1, 1))):
        m = R.random_mask((n, h, w), 4000 + 10 * n + T + k)
        m[0, 0, 0] = np.nan
        src = _dev(ctx, m)
        for shot in (None, cut):
            got = ctx.mask_hold_batch(src, T, shot).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(R.hold(m, T, shot))), (n, T, h, w, shot is None)
        assert np.array_equal(_bits(src.cpu().numpy()), _bits(m))
        if h * w > 50:
            assert np.isnan(m).any() and np.isnan(got).any() == (T == 0)   # T = 0 keeps the NaNs, T > 0 reads them as 1.0


def test_hold_on_an_unaligned_view(ctx):
    """A view that starts one float past a 16-byte boundary with h * w a multiple of 4: the scalar path, by the pointers."""
    m = R.random_mask((4, 8, 12), 77)
    flat = ctx.torch.zeros((4 * 8 * 12 + 1,), device=ctx.device)
    flat[1:] = _dev(ctx, m).reshape(-1)
    view = flat[1:].reshape(4, 8, 12)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert np.array_equal(_bits(ctx.mask_hold_batch(view, 2).cpu().numpy()), _bits(R.hold(m, 2)))
    out, count = ctx.mask_grow_batch(view, 3, feather=2, want_count=True)
    want, want_count = R.grow_feather(m, 3, True, 2)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and count.cpu().numpy().tolist() == want_count.tolist()


# ---- end to end --------------------------------------------------------------------------------------------------------------
W, H, N = 160, 96, 12
ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the whole shake becomes padding
SHAKE_AMP = 8.0


@pytest.fixture(scope="module")
def clip(ctx):
    import torch

    import bench

    return bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=shake_path(N, W, H, "similarity", seed=3, amp=SHAKE_AMP))


def _stabilize(ctx, frames, framing="crop_and_pad", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, "similarity", *ARGS, ctx=ctx, keep_on_device=True, **kw)


def _expected_block(request, counts, h, w):
    frac = (counts.astype(np.float32) / np.float32(h * w)).astype(np.float64)
    hold, grow, tapered, feather = request
    return {"version": 1, "hold": hold, "grow": grow, "tapered": tapered, "feather": feather,
            "masked_fraction_mean": float(frac.mean()), "masked_fraction_max": float(frac.max())}


def _assert_is_handoff_of(base, on, block, request, shot=None):
    """`on` is `base` with the restatement applied to its mask: frames untouched, the block from the restatement's counts."""
    hold, grow, tapered, feather = request
    m0 = base.masks.cpu().numpy()[..., 0]
    assert 0 < (m0 > 0.5).sum() < m0.size, "no frame has padding: the test would show nothing"
    want, counts = R.handoff(m0, hold, grow, tapered, feather, shot)
    assert not np.array_equal(_bits(want), _bits(m0))
    assert np.array_equal(_bits(on.masks.cpu().numpy()[..., 0]), _bits(want))
    assert np.array_equal(_bits(on.frames.cpu().numpy()), _bits(base.frames.cpu().numpy()))
    assert block == _expected_block(request, counts, m0.shape[1], m0.shape[2])


@pytest.mark.parametrize("framing", ["crop_and_pad", "expand"])
def test_end_to_end_keyword(pkg, ctx, clip, framing):
    ctx.set_timing(True)
    try:
        ctx.mask_grow_batch(clip[:1, :, :, 0].contiguous(), 1)                 # so that the timing kinds exist
        ctx.mask_hold_batch(clip[:2, :, :, 0].contiguous(), 1)
        ctx.set_timing(True)                                                   # clears the totals
        plain = _stabilize(ctx, clip, framing)                                  # the parent's call
        off = _stabilize(ctx, clip, framing, mask_grow=None, mask_feather=None, mask_hold=None, mask_tapered=None)
        assert ctx.kernel_ms_stats("mask_grow")[1] == 0 and ctx.kernel_ms_stats("mask_hold")[1] == 0     # None launches nothing
        on = _stabilize(ctx, clip, framing, mask_grow=5)
        assert ctx.kernel_ms_stats("mask_grow")[1] == 1 and ctx.kernel_ms_stats("mask_hold")[1] == 0
    finally:
        ctx.set_timing(False)
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(plain.frames.cpu().numpy()))
    assert np.array_equal(_bits(off.masks.cpu().numpy()), _bits(plain.masks.cpu().numpy()))
    assert json.dumps(off.meta) == json.dumps(plain.meta) and "mask_handoff" not in off.meta
    if framing == "crop_and_pad":
        assert on.device_plan["used"]                                           # the device-plan path
    meta_on = dict(on.meta)
    block = meta_on.pop("mask_handoff")
    assert json.dumps(meta_on) == json.dumps(off.meta)                          # padding_fraction_* keep describing the warp
    _assert_is_handoff_of(off, on, block, (0, 5, True, 0))


def test_end_to_end_behind_the_other_passes(pkg, ctx, clip):
    """temporal_fill, spatial_fill and stability_report see the true mask: their blocks and the frames are those of the call
    without the hand-off, and the returned mask is the restatement of THAT call's mask (the temporal fill has cleared part)."""
    extra = dict(temporal_fill=2, spatial_fill=True, stability_report=True)
    base = _stabilize(ctx, clip, **extra)
    on = _stabilize(ctx, clip, mask_grow=3, mask_feather=6, mask_hold=1, mask_tapered=False, **extra)
    meta_on = dict(on.meta)
    block = meta_on.pop("mask_handoff")
    assert json.dumps(meta_on) == json.dumps(base.meta)
    assert all(k in base.meta for k in ("temporal_fill", "spatial_fill", "stability"))
    _assert_is_handoff_of(base, on, block, (1, 3, False, 6))


def test_scene_cuts_keep_the_hold_inside_a_shot(pkg, ctx, clip):
    base = _stabilize(ctx, clip, scene_cuts=[5])
    on = _stabilize(ctx, clip, scene_cuts=[5], mask_hold=2)
    meta_on = dict(on.meta)
    block = meta_on.pop("mask_handoff")
    assert json.dumps(meta_on) == json.dumps(base.meta) and "scene_cuts" in base.meta
    shot = R.shots_from_segments([(0, 5), (5, N)], N)
    _assert_is_handoff_of(base, on, block, (2, 0, True, 0), shot)
    m0 = base.masks.cpu().numpy()[..., 0]
    assert not np.array_equal(_bits(R.hold(m0, 2, shot)), _bits(R.hold(m0, 2)))          # the cut matters on this clip


def test_crop_framing_is_a_noop_without_a_block(pkg, ctx, clip):
    a = _stabilize(ctx, clip, "crop")
    b = _stabilize(ctx, clip, "crop", mask_grow=5, mask_feather=3)
    assert np.array_equal(_bits(a.frames.cpu().numpy()), _bits(b.frames.cpu().numpy()))
    assert np.array_equal(_bits(a.masks.cpu().numpy()), _bits(b.masks.cpu().numpy()))
    assert json.dumps(a.meta) == json.dumps(b.meta)


def _apply(ctx, frames, meta, **kw):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    return ap.apply_motion(hm._normalize_video_input(frames), meta, (127, 127, 127), ctx=ctx, keep_on_device=True, **kw)


def test_motion_apply_inverse_with_motion_blur(pkg, ctx, clip):
    run = _stabilize(ctx, clip)
    inverse_only = {k: v for k, v in json.loads(json.dumps(run.meta)).items() if k != "motion_meta"}
    for kw in (dict(motion_blur=0.5, motion_blur_samples=5), dict()):
        base = _apply(ctx, run.frames, inverse_only, **kw)
        on = _apply(ctx, run.frames, inverse_only, mask_grow=4, mask_feather=4, **kw)
        if kw:
            frac = base.masks.cpu().numpy()
            assert ((frac > 0) & (frac < 1)).any()                                         # the blur's masks are fractions
        meta_on = json.loads(json.dumps(on.meta))
        block = meta_on["motion_apply"].pop("mask_handoff")
        assert json.dumps(meta_on) == json.dumps(base.meta)
        _assert_is_handoff_of(base, on, block, (0, 4, True, 4))
    a, b = _apply(ctx, clip, run.meta, framing_mode="crop"), _apply(ctx, clip, run.meta, framing_mode="crop", mask_grow=5)
    if a.meta["motion_apply"]["framing_mode"] == "crop":                                   # no mask: no block
        assert json.dumps(a.meta) == json.dumps(b.meta)
        assert np.array_equal(_bits(a.masks.cpu().numpy()), _bits(b.masks.cpu().numpy()))


def test_node_on_host_tensors_with_a_feather(pkg, ctx, clip, monkeypatch):
    import torch

    from vstab_amd import nodes

    run = _stabilize(ctx, clip)
    m0 = run.masks.cpu().numpy()[..., 0]
    want, _ = R.handoff(m0, 1, 5, True, 8)
    assert ((want > 0) & (want < 1)).any()                                                 # not a 0 / 1 mask any more
    for coded in ("1", "0"):
        monkeypatch.setenv("VSTAB_XFER_CODED", coded)
        host_in = torch.from_numpy(m0.copy())
        out = nodes.VideoStabilizerMaskGrow.execute(host_in, 5, True, 8, 1)
        (got,) = out.result if hasattr(out, "result") else out.args
        assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == m0.shape
        assert np.array_equal(_bits(got.numpy()), _bits(want))
        assert np.array_equal(_bits(host_in.numpy()), _bits(m0))                            # the input stays as it is
        hard = nodes.VideoStabilizerMaskGrow.execute(host_in, 5, False, 0, 0)               # a 0 / 1 result may cross as bytes
        (got,) = hard.result if hasattr(hard, "result") else hard.args
        assert np.array_equal(_bits(got.numpy()), _bits(R.handoff(m0, 0, 5, False, 0)[0]))
    one = nodes.VideoStabilizerMaskGrow.execute(torch.from_numpy(m0[3].copy()), 2, True, 0, 0)   # [H,W]
    (got,) = one.result if hasattr(one, "result") else one.args
    assert tuple(got.shape) == m0[3].shape and np.array_equal(_bits(got.numpy()), _bits(R.grow(m0[3:4], 2)[0]))
    monkeypatch.setenv("VSTAB_KEEP_ON_DEVICE", "1")
    kept = nodes.VideoStabilizerMaskGrow.execute(run.masks[..., 0], 5, True, 8, 1)
    (got,) = kept.result if hasattr(kept, "result") else kept.args
    assert got.device.type == "cuda" and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
