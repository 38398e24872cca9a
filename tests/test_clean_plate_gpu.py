"""GPU: the clean plate's three entries (csrc/vstab_plate.hip), the `plate_fill` keyword and the node.

  1. vstab_plate_median_batch equals the NumPy restatement (tests/clean_plate_restatement.py) IN BITS, counts included, at the
     sample counts where the kernel changes form (native.PLATE_PATH_STEPS), at shapes around its tiles, with several shots,
     masks and special values; and what it refuses
  2. vstab_plate_fill_batch / vstab_plate_matte_batch equal the restatement in bits on both access forms
  3. the pipeline keyword against the restatement applied on the host to the outputs of the calls without it, and the node
"""

import json

import numpy as np
import pytest

from tests import clean_plate_restatement as R
from tests.drift_util import LOCK_ARGS
from tests.drift_util import stabilize as _stabilize
from tests.test_clean_plate_cpu import drawn

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _dev(ctx, a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _check_median(ctx, frames, mask, table, dev=None):
    table = np.asarray(table, np.int32)
    want, want_count = R.plate_median(frames, mask, table)
    f, m = dev if dev is not None else (_dev(ctx, frames), _dev(ctx, mask))
    plate, count = ctx.plate_median_batch(f, m, table)
    plate, count = plate.cpu().numpy(), count.cpu().numpy()
    assert plate.shape == want.shape and plate.dtype == np.float32 and count.shape == want_count.shape and count.dtype == np.int32
    assert np.array_equal(count, want_count), np.argwhere(count != want_count)[:5].tolist()
    assert np.array_equal(_bits(plate), _bits(want)), np.argwhere(plate.view(np.uint32) != want.view(np.uint32))[:5].tolist()
    return want, want_count


# ---- 1. the median -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_clip(ctx):
    """257 frames of 16 x 9 (432 elements: two workgroups of the register form, seven of the LDS form) with special values, ties
    and a mask of every kind, shared by the sample-count cases, on the host and on the device."""
    frames, mask = drawn(7, 257, 9, 16, special=0.2, masked=0.35)
    return frames, mask, (_dev(ctx, frames), _dev(ctx, mask))


# 1..4 (odd, even, the lower-median choice), every count at which the kernel changes form and the first count of the next form,
# and the most a row can hold; the test holds the list to the constants the module exports
SAMPLE_COUNTS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256]


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_median_at_every_sample_count_where_the_kernel_changes(pkg, ctx, long_clip, S):
    from vstab_amd import native

    steps = list(native.PLATE_PATH_STEPS)
    assert SAMPLE_COUNTS == sorted(set([1, 2, 3, 4] + steps + [s + 1 for s in steps] + [native.PLATE_SAMPLES_MAX]))
    assert native.PLATE_REGISTER_MAX in steps
    frames, mask, dev = long_clip
    # S consecutive frames from frame 1 on (the row starts off frame 0), masked and not
    table = np.arange(1, S + 1, dtype=np.int32)[None]
    _, count = _check_median(ctx, frames, mask, table, dev)
    assert count.min() < count.max() <= S                                            # the counts do vary over the picture
    _check_median(ctx, frames, None, table, (dev[0], None))


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (5, 17), (2, 43), (3, 7), (2, 11), (1, 22)])
def test_median_at_shapes_around_the_tiles(pkg, ctx, h, w):
    """h * w * 3 = 3, 105 (no multiple of 4 or 64), 255 and 258 (the register form's tile of 256 -1 and +2: 257 is no multiple
    of 3), 63 and 66 (the LDS form's tile of 64 -1 and +2), 66 again as one row."""
    frames, mask = drawn(h * 100 + w, 70, h, w)
    for S in (3, 70):                                   # the register form and the LDS form
        _check_median(ctx, frames, mask, np.arange(S)[None])


def test_median_rows_of_unequal_length_and_non_consecutive_frames(pkg, ctx):
    frames, mask = drawn(3, 90, 6, 10)
    two = np.full((2, 80), -1, np.int32)                # the LDS form
    two[0, :80] = np.arange(80)
    two[1, :7] = [1, 2, 9, 17, 30, 48, 89]
    _check_median(ctx, frames, mask, two)
    three = np.full((3, 12), -1, np.int32)              # the widest row decides the form for all: the register one here
    three[0, :12] = np.arange(0, 48, 4)
    three[1, :1] = [49]
    three[2, :5] = [0, 10, 11, 12, 40]
    want, count = _check_median(ctx, frames, mask, three)
    assert np.array_equal(count[1], (mask[49] <= 0.5).astype(np.int32))               # a row of one sample: that frame, where valid
    # nothing crosses from one row to another: each row alone gives its own plate
    for s in range(3):
        alone, _ = R.plate_median(frames, mask, three[s:s + 1])
        assert np.array_equal(_bits(alone[0]), _bits(want[s]))
    # -1 padding wider than the rows need
    wide = np.full((2, 256), -1, np.int32)
    wide[:, :5] = three[2, :5]
    _check_median(ctx, frames, None, wide)


@pytest.mark.parametrize("S", [5, 80])                  # the register form and the LDS form
def test_median_masks_and_values(pkg, ctx, S):
    """Pixels with count 0, 1 and S; all samples equal; -0.0 / +0.0; infinities; denormals; NaNs in fewer and in more than
    half of the samples; NaN, 0.5 and nextafter(0.5) in the mask."""
    h, w = 4, 6
    rng = np.random.default_rng(S)
    frames = rng.uniform(0, 1, (S, h, w, 3)).astype(np.float32)
    mask = np.zeros((S, h, w), np.float32)
    mask[:, 0, 0] = 1.0                                   # count 0
    mask[1:, 0, 1] = np.nan                               # count 1
    mask[:, 0, 2] = 0.5                                   # every sample valid, at the bound
    mask[::2, 0, 3] = np.nextafter(np.float32(0.5), np.float32(1))
    mask[::3, 0, 4] = np.inf
    mask[::3, 0, 5] = -np.inf                             # valid
    frames[:, 1, 0] = 0.375                               # all equal
    frames[::2, 1, 1] = -0.0
    frames[1::2, 1, 1] = 0.0
    frames[::2, 1, 2] = np.inf
    frames[1::2, 1, 2] = -np.inf
    frames[:, 1, 3] = (rng.integers(1, 100, (S, 3)).astype(np.uint32)).view(np.float32) * np.float32(1.0)       # denormals
    frames[:, 1, 4] = -(rng.integers(1, 100, (S, 3)).astype(np.uint32)).view(np.float32)
    frames[:(S - 1) // 2, 2, 0] = np.nan                  # fewer than half
    frames[:S // 2 + 1, 2, 1] = np.nan                    # more than half
    frames[:, 2, 2] = np.nan
    frames[:S // 2 + 1, 2, 3].view(np.uint32)[...] = 0xFFC00001      # negative NaNs with a payload
    want, count = _check_median(ctx, frames, mask, np.arange(S)[None])
    assert count[0, 0, :3].tolist() == [0, 1, S] and not want[0, 0, 0].view(np.uint32).any()
    assert np.isfinite(want[0, 2, 0]).all() and (want[0, 2, 1:4].view(np.uint32) == 0x7FC00000).all()
    assert (want[0, 1, 3] > 0).all() and (want[0, 1, 3] < 1e-40).all()
    assert (want[0, 1, 1].view(np.uint32) == 0x80000000).all()              # rank (S - 1) // 2 lies in the -0.0 half, odd S or even
    assert (want[0, 1, 2] == (np.inf if S % 2 else -np.inf)).all()          # (+inf is the even-numbered samples: one more for odd S)
    _check_median(ctx, frames, None, np.arange(S)[None])


def test_median_refusals(pkg, ctx):
    import torch

    from vstab_amd import native

    frames = torch.zeros((6, 3, 4, 3), device=ctx.device)
    for table, text in (([[0, 2, 1]], "row 0 is not strictly increasing at column 2 (1 after 2)"),
                        ([[0, 1, 1]], "row 0 is not strictly increasing at column 2 (1 after 1)"),
                        ([[0, 1], [4, 6]], "sample_frame[1][1]=6 is not a frame index in 0..5"),
                        ([[0, -2]], "sample_frame[0][1]=-2 is not a frame index in 0..5"),
                        ([[0, -1, 3]], "row 0 holds the index 3 behind its -1 padding"),
                        ([[0, 1], [-1, -1]], "sample_frame row 1 is empty"),
                        ([[-1, 2]], "sample_frame row 0 is empty"),
                        (np.zeros((1, 0), np.int32), "S=0 samples per shot outside 1..256"),
                        (np.arange(257, dtype=np.int32)[None] % 6, "S=257 samples per shot outside 1..256")):
        with pytest.raises(native.VstabError, match=r"vstab_plate_median_batch: .*" + __import__("re").escape(text)):
            ctx.plate_median_batch(frames, None, np.asarray(table, np.int32))
    with pytest.raises(ValueError, match="mask of shape"):
        ctx.plate_median_batch(frames, torch.zeros((6, 4, 3), device=ctx.device), [[0]])
    with pytest.raises(ValueError, match="frames must be a contiguous float32 tensor"):
        ctx.plate_median_batch(frames.cpu(), None, [[0]])


# ---- 2. fill and matte ---------------------------------------------------------------------------------------------------------
def _plate_case(seed, n, h, w, shots=1):
    """Frames and mask with every special value, a plate and counts 0..5 drawn on their own (the entries take any)."""
    rng = np.random.default_rng(seed)
    frames, mask = drawn(seed, n, h, w, special=0.15, masked=0.5)
    plate, _ = drawn(seed + 1, shots, h, w, special=0.15)
    same = rng.uniform(size=(n, h, w)) < 0.4              # frames that equal their plate, or sit exactly at a threshold of 0.25
    shot = np.sort(rng.integers(0, shots, n)).astype(np.int32) if shots > 1 else None
    of = np.zeros(n, np.int64) if shot is None else shot
    frames[same] = plate[of][same]
    at = rng.uniform(size=(n, h, w)) < 0.2
    frames[at] = (plate[of] + np.float32(0.25))[at]
    count = rng.integers(0, 6, (shots, h, w)).astype(np.int32)
    return frames, mask, plate, count, shot


def _check_fill_and_matte(ctx, frames, mask, plate, count, shot, align=0):
    """align: floats by which every device tensor is moved off its allocation's boundary (1: no 16-byte access is possible)."""
    import torch

    def dev(a):
        if a is None:
            return None
        flat = torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device).reshape(-1)
        buf = torch.empty((flat.numel() + align,), dtype=flat.dtype, device=ctx.device)
        buf[align:] = flat
        return buf[align:].view(a.shape)

    n = frames.shape[0]
    d_plate, d_count = dev(plate), dev(count)
    for min_count in (1, 3, 6):                            # 6: above the largest count, nothing may change
        want_f, want_m, want_c = R.plate_fill(frames, mask, plate, count, shot, min_count)
        d_f, d_m = dev(frames), dev(mask)
        filled = ctx.plate_fill_batch(d_f, d_m, d_plate, d_count, shot, min_count).cpu().numpy()
        assert filled.tolist() == want_c.tolist()
        assert np.array_equal(_bits(d_f.cpu().numpy()), _bits(want_f)) and np.array_equal(_bits(d_m.cpu().numpy()), _bits(want_m))
        if min_count == 6:
            assert not filled.any() and np.array_equal(_bits(want_f), _bits(frames)) and np.array_equal(_bits(want_m), _bits(mask))
        else:
            assert filled.sum() > 0 or frames.size < 50
        for threshold in (0.0, 0.25):
            for m in (mask, None):
                want, want_total = R.plate_matte(frames, m, plate, count, shot, threshold, min_count)
                d_src = dev(frames)
                matte, total = ctx.plate_matte_batch(d_src, dev(m), d_plate, d_count, shot, threshold, min_count)
                assert np.array_equal(_bits(matte.cpu().numpy()), _bits(want)) and total.cpu().numpy().tolist() == want_total.tolist()
                assert np.array_equal(_bits(d_src.cpu().numpy()), _bits(frames))          # read only
    assert np.array_equal(_bits(d_plate.cpu().numpy()), _bits(plate)) and np.array_equal(d_count.cpu().numpy(), count)


@pytest.mark.parametrize("n,h,w,shots,align", [(2, 1, 1, 1, 0), (3, 5, 7, 1, 0), (3, 9, 16, 2, 0), (2, 4, 257, 1, 0), (4, 9, 16, 3, 1),
                                               (2, 3, 85, 1, 0), (5, 33, 32, 2, 0)])
def test_fill_and_matte_equal_the_restatement_in_bits(pkg, ctx, n, h, w, shots, align):
    """1 x 1; 35 pixels (one per lane); 144 (four per lane); 1028 = a workgroup's 256 x 4 and one lane more; 144 off a
    16-byte boundary (one per lane again); 255 pixels; 1056 pixels in more than one workgroup per frame."""
    frames, mask, plate, count, shot = _plate_case(n * 1000 + h * w, n, h, w, shots)
    _check_fill_and_matte(ctx, frames, mask, plate, count, shot, align)


def test_fill_and_matte_special_pixels(pkg, ctx):
    """shot = None against an all-zero shot; a NaN mask pixel is filled and is not own; a NaN on either side of the matte's
    difference differs; values exactly at the threshold do not."""
    frames = np.full((2, 1, 8, 3), 0.5, np.float32)
    plate = np.full((1, 1, 8, 3), 0.25, np.float32)
    count = np.full((1, 1, 8), 4, np.int32)
    mask = np.zeros((2, 1, 8), np.float32)
    mask[0, 0, 0] = np.nan
    mask[0, 0, 1] = 1.0
    mask[0, 0, 2] = np.nextafter(np.float32(0.5), np.float32(1))
    mask[0, 0, 3] = 0.5
    frames[1, 0, 0, 1] = np.nan
    plate[0, 0, 1, 2] = np.nan
    frames[1, 0, 2] = plate[0, 0, 2]
    frames[1, 0, 3, 0] = np.nextafter(np.float32(0.5), np.float32(1))
    want_f, want_m, want_c = R.plate_fill(frames, mask, plate, count, None, 1)
    assert want_c.tolist() == [3, 0] and want_m[0, 0, :4].tolist() == [0.0, 0.0, 0.0, 0.5]
    want_matte, want_total = R.plate_matte(frames, mask, plate, count, None, 0.25, 1)
    assert want_matte[0, 0].tolist() == [0.0] * 8                                     # |0.5 - 0.25| is at the threshold; NaN mask: not own
    assert want_matte[1, 0].tolist() == [1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]      # NaN frame, NaN plate, equal, one ulp over
    for shot in (None, np.zeros(2, np.int32)):
        d_f, d_m = _dev(ctx, frames), _dev(ctx, mask)
        filled = ctx.plate_fill_batch(d_f, d_m, _dev(ctx, plate), _dev(ctx, count), shot, 1)
        assert filled.cpu().numpy().tolist() == want_c.tolist()
        assert np.array_equal(_bits(d_f.cpu().numpy()), _bits(want_f)) and np.array_equal(_bits(d_m.cpu().numpy()), _bits(want_m))
        matte, total = ctx.plate_matte_batch(_dev(ctx, frames), _dev(ctx, mask), _dev(ctx, plate), _dev(ctx, count), shot, 0.25, 1)
        assert np.array_equal(_bits(matte.cpu().numpy()), _bits(want_matte)) and total.cpu().numpy().tolist() == want_total.tolist()


def test_fill_and_matte_refusals(pkg, ctx):
    import torch

    from vstab_amd import native

    f = torch.zeros((3, 2, 4, 3), device=ctx.device)
    m = torch.zeros((3, 2, 4), device=ctx.device)
    plate = torch.zeros((2, 2, 4, 3), device=ctx.device)
    count = torch.zeros((2, 2, 4), dtype=torch.int32, device=ctx.device)
    for shot, text in (([0, 1, 0], "non-decreasing"), ([0, 1, 2], "0..1"), ([0, 1], "n=3"), (None, "one shot, but plate holds 2")):
        with pytest.raises(ValueError, match=text):
            ctx.plate_fill_batch(f, m, plate, count, shot, 1)
    for bad in (0, 257, True, 1.0):
        with pytest.raises(ValueError, match="min_count="):
            ctx.plate_matte_batch(f, m, plate, count, [0, 0, 1], 0.1, bad)
    for bad in (-0.1, np.nan, np.inf, "x"):
        with pytest.raises(ValueError, match="threshold="):
            ctx.plate_matte_batch(f, m, plate, count, [0, 0, 1], bad, 1)
    with pytest.raises(ValueError, match="count of shape"):
        ctx.plate_fill_batch(f, m, plate, count[:1], [0, 0, 1], 1)
    # the library's own checks, under its name
    import ctypes as C

    rc = ctx.lib.vstab_plate_fill_batch(ctx.handle, f.data_ptr(), m.data_ptr(), 3, 2, 4, plate.data_ptr(), count.data_ptr(),
                                        np.array([0, 1, 0], np.int32).ctypes.data, 2, 1, None)
    assert rc != 0 and ctx.lib.vstab_last_error().decode() == "vstab_plate_fill_batch: shot is not non-decreasing at frame 2"
    rc = ctx.lib.vstab_plate_matte_batch(ctx.handle, f.data_ptr(), None, 3, 2, 4, plate.data_ptr(), count.data_ptr(), None, 1,
                                         C.c_float(float("nan")), 1, m.data_ptr(), None)
    assert rc != 0 and "threshold=nan is not finite and >= 0" in ctx.lib.vstab_last_error().decode()
    assert isinstance(native.VstabError("x"), RuntimeError)


# ---- 3. the pipeline -----------------------------------------------------------------------------------------------------------
N, H, W = 12, 135, 240
# integer shake, frame 0 at rest, the four diagonal extremes present: every canvas pixel is seen by some frame
SHIFTS = np.array([[0, 0], [4, 3], [-4, -3], [2, -1], [4, -3], [-1, 2], [-4, 3], [3, 1], [-2, -2], [1, 3], [-3, 0], [0, -3]])


def plate_clip():
    """12 frames of 240 x 135 of the kind tests/test_deflicker_gpu.py builds, without the flicker: the bench's texture recipe
    under a known integer shake, and a 24 x 24 subject that crosses the scene 16 px per frame -- no scene point shows it in more
    than two frames.  -> (frames, the static background, the subject's footprints in frame coordinates)."""
    from tests.deflicker_restatement import _texture

    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = np.empty((N, H, W, 3), np.float32)
    footprint = np.zeros((N, H, W), bool)
    for i, (dx, dy) in enumerate(SHIFTS):
        img = 0.1 + 0.8 * _texture(xx - dx, yy - dy, 1234)
        x0, y0 = 10 + 16 * i + dx, 50 + 2 * i + dy
        footprint[i] = (xx >= x0) & (xx < x0 + 24) & (yy >= y0) & (yy < y0 + 24)
        img[footprint[i]] = (0.95, 0.1, 0.1 + 0.05 * (i % 2))
        frames[i] = img.astype(np.float32)
    background = (0.1 + 0.8 * _texture(xx, yy, 1234)).astype(np.float32)
    return frames, background, footprint


def locked_model(frames):
    """What a perfectly locked camera returns for the clip, on the CPU: frame i moved back by its shift (the shake is
    symmetric, so crop_and_pad centres nothing), padding where frame i did not see."""
    out = np.full_like(frames, 127 / 255)
    mask = np.ones(frames.shape[:3], np.float32)
    for i, (dx, dy) in enumerate(SHIFTS):
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
        yd, xd = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
        out[i, ys, xs] = frames[i, yd, xd]
        mask[i, ys, xs] = 0.0
    return out, mask


@pytest.fixture(scope="module")
def clip():
    frames, background, footprint = plate_clip()
    # the condition the clip is built by, on the restatement alone, here on the CPU: the fill does something, and at least
    # one frame ends with no padding at all -- otherwise the pipeline tests could pass with a fill that does nothing
    out, mask = locked_model(frames)
    for segments in (None, [(0, 6), (6, 12)]):
        _, after, block, plate, count = R.pipeline(out, mask, out, mask, segments, 1)
        assert block["filled_fraction_mean"] > 0 and block["frames_with_padding_after"] < N, block
    _, _, block, plate, count = R.pipeline(out, mask, out, mask, None, 1)
    assert block["frames_with_padding_after"] == 0 and block["unseen_fraction"] == [0.0]
    seen3 = count[0] >= 3
    assert np.array_equal(_bits(plate[0][seen3]), _bits(background[seen3]))          # the subject is gone from the model's plate
    return {"frames": frames, "background": background, "footprint": footprint}


def _launches(ctx, kind):
    """Launches of `kind` the context's timing record shows since set_timing(True); a kind it has never seen has no record."""
    from vstab_amd import native

    try:
        return ctx.kernel_ms_stats(kind)[1]
    except native.VstabError:
        return 0


def _run(ctx, frames, **kw):
    return _stabilize(ctx, frames, "translation", LOCK_ARGS, **kw)


def _host(res):
    return res.frames.cpu().numpy(), res.masks.cpu().numpy()[..., 0]


@pytest.fixture(scope="module")
def runs(ctx, clip):
    import torch

    frames = torch.from_numpy(clip["frames"]).to(ctx.device)
    ctx.set_timing(True)
    bare = _run(ctx, frames)
    off = _run(ctx, frames, plate_fill=None)
    kinds = {kind: _launches(ctx, kind) for kind in ("plate_median", "plate_fill", "plate_matte")}
    ctx.set_timing(False)
    return {"frames": frames, "bare": bare, "off": off, "kinds_off": kinds}


def test_off_is_off(pkg, ctx, runs):
    (f0, m0), (f1, m1) = _host(runs["bare"]), _host(runs["off"])
    assert np.array_equal(_bits(f0), _bits(f1)) and np.array_equal(_bits(m0), _bits(m1))
    assert json.dumps(runs["bare"].meta) == json.dumps(runs["off"].meta) and "plate_fill" not in runs["off"].meta
    assert json.dumps(_run(ctx, runs["frames"], plate_fill=False).meta) == json.dumps(runs["bare"].meta)
    # the context's timing record shows none of the three new kinds
    assert runs["kinds_off"] == {"plate_median": 0, "plate_fill": 0, "plate_matte": 0}
    ctx.set_timing(True)                                   # (and the record does show them when the keyword is on)
    _run(ctx, runs["frames"], plate_fill=True)
    on = {kind: _launches(ctx, kind) for kind in runs["kinds_off"]}
    ctx.set_timing(False)
    assert on == {"plate_median": 1, "plate_fill": 1, "plate_matte": 0}
    assert (m0 > 0.5).any(), "the warp left no padding: the tests below would show nothing"


def _assert_is_pipeline_of(unfilled, before_fill, got, segments, min_count, spatial=False):
    """`got` is `before_fill` (the call with the same keywords but plate_fill) with the restatement's plate -- formed from
    `unfilled`, the call without any fill -- filled in on the host; its meta differs by the plate_fill block only."""
    fa, ma = _host(unfilled)
    fb, mb = _host(before_fill)
    want_f, want_m, block, plate, count = R.pipeline(fa, ma, fb, mb, segments, min_count)
    assert block["filled_fraction_mean"] > 0 and block["frames_with_padding_after"] < N, block
    if spatial:
        from tests import spatial_fill_restatement as SF

        want_f = SF.fill_batch(want_f, want_m)[0]
    gf, gm = _host(got)
    assert np.array_equal(_bits(gm), _bits(want_m)), np.argwhere(gm != want_m)[:5].tolist()
    assert np.array_equal(_bits(gf), _bits(want_f)), np.argwhere(gf.view(np.uint32) != want_f.view(np.uint32))[:5].tolist()
    assert got.meta["plate_fill"] == block
    rest = {k: v for k, v in got.meta.items() if k not in ("plate_fill", "spatial_fill")}
    assert rest == {k: v for k, v in before_fill.meta.items() if k != "spatial_fill"}
    return block, plate, count


def test_keyword_equals_the_restatement_on_the_host(pkg, ctx, runs):
    on = _run(ctx, runs["frames"], plate_fill=True)
    block, _, _ = _assert_is_pipeline_of(runs["bare"], runs["bare"], on, None, 1)
    assert list(on.meta) == list(runs["bare"].meta) + ["plate_fill"]
    assert block["shots"] == 1 and block["samples_per_shot"] == [N] and block["min_count"] == 1
    # a min_count that the canvas corners, seen by few of the 12 frames, do not reach fills less and leaves more
    eight = _run(ctx, runs["frames"], plate_fill=8)
    block8, _, _ = _assert_is_pipeline_of(runs["bare"], runs["bare"], eight, None, 8)
    assert block8["filled_fraction_mean"] < block["filled_fraction_mean"] and block8["unseen_fraction"][0] > block["unseen_fraction"][0]
    assert block8["frames_with_padding_after"] > block["frames_with_padding_after"]


def test_plate_before_the_temporal_fill_and_fill_behind_it(pkg, ctx, runs):
    temporal = _run(ctx, runs["frames"], temporal_fill=2)
    both = _run(ctx, runs["frames"], temporal_fill=2, plate_fill=True)
    block, _, _ = _assert_is_pipeline_of(runs["bare"], temporal, both, None, 1)
    keys = list(both.meta)
    assert keys.index("temporal_fill") + 1 == keys.index("plate_fill")
    # the plate was NOT formed from the temporally filled frames: that restatement differs
    ft, mt = _host(temporal)
    wrong = R.pipeline(ft, mt, ft, mt, None, 1)
    assert wrong[2] != block or not np.array_equal(_bits(wrong[0]), _bits(_host(both)[0]))


def test_two_plates_under_scene_cuts(pkg, ctx, runs):
    cut = _run(ctx, runs["frames"], scene_cuts=[6])
    on = _run(ctx, runs["frames"], scene_cuts=[6], plate_fill=True)
    block, plate, _ = _assert_is_pipeline_of(cut, cut, on, [(0, 6), (6, 12)], 1)
    assert block["shots"] == 2 and block["samples_per_shot"] == [6, 6] and plate.shape[0] == 2


def test_spatial_fill_runs_behind_it(pkg, ctx, runs):
    on = _run(ctx, runs["frames"], plate_fill=8, spatial_fill=True)
    block, _, _ = _assert_is_pipeline_of(runs["bare"], runs["bare"], on, None, 8, spatial=True)
    assert block["frames_with_padding_after"] > 0 and on.meta["spatial_fill"]["frames_filled"] == block["frames_with_padding_after"]
    keys = list(on.meta)
    assert keys.index("plate_fill") + 1 == keys.index("spatial_fill")


def test_crop_framing_launches_nothing_and_adds_no_block(pkg, ctx, runs):
    a = _stabilize(ctx, runs["frames"], "translation", LOCK_ARGS, framing="crop")
    ctx.set_timing(True)
    b = _stabilize(ctx, runs["frames"], "translation", LOCK_ARGS, framing="crop", plate_fill=True)
    launches = _launches(ctx, "plate_median") + _launches(ctx, "plate_fill")
    ctx.set_timing(False)
    assert launches == 0
    assert np.array_equal(_bits(a.frames.cpu().numpy()), _bits(b.frames.cpu().numpy())) and json.dumps(a.meta) == json.dumps(b.meta)


def test_the_node_against_the_module_functions(pkg, ctx, runs):
    from vstab_amd import clean_plate, nodes

    base = runs["bare"]
    frames, mask = base.frames, base.masks[..., 0].contiguous()
    before_f, before_m = _host(base)
    plate, count, table = clean_plate.plate_on_device(ctx, frames, mask)
    matte, matte_count = clean_plate.matte_on_device(ctx, frames, mask, plate, count, None, 0.1, 3)
    want_f, want_m = frames.clone(), mask.clone()
    block = clean_plate.fill_and_report(ctx, want_f, want_m, plate, count, table, None, 2)
    out = nodes.VideoStabilizerCleanPlate.execute(frames, mask, True, 2, 0.1, 3)
    n_plate, n_frames, n_mask, n_matte, n_meta = out.result if hasattr(out, "result") else out.args
    assert tuple(n_plate.shape) == (1, H, W, 3) and tuple(n_matte.shape) == (N, H, W)
    assert np.array_equal(_bits(n_plate.cpu().numpy()), _bits(plate.cpu().numpy()))
    assert np.array_equal(_bits(n_frames.cpu().numpy()), _bits(want_f.cpu().numpy()))
    assert np.array_equal(_bits(n_mask.cpu().numpy()), _bits(want_m.cpu().numpy()))
    assert np.array_equal(_bits(n_matte.cpu().numpy()), _bits(matte.cpu().numpy()))
    meta = json.loads(n_meta)["clean_plate"]
    assert meta["plate_fill"] == block and meta["samples"] == N and meta["matte_threshold"] == 0.1 and meta["matte_min_count"] == 3
    share = matte_count.cpu().numpy().astype(np.float32) / np.float32(H * W)
    assert meta["matte_fraction_max"] == float(share.max()) and 0 < meta["matte_fraction_max"] < 0.05
    # the module functions themselves against the restatement, and the inputs are not written to
    rp, rc = R.plate_median(before_f, before_m, R.sample_table(None, N))
    assert np.array_equal(_bits(plate.cpu().numpy()), _bits(rp)) and np.array_equal(count.cpu().numpy(), rc)
    assert np.array_equal(_bits(matte.cpu().numpy()), _bits(R.plate_matte(before_f, before_m, rp, rc, None, 0.1, 3)[0]))
    assert np.array_equal(_bits(base.frames.cpu().numpy()), _bits(before_f))
    # fill off, and no mask at all: frames as given, a zero mask
    out = nodes.VideoStabilizerCleanPlate.execute(frames, None, False)
    _, n_frames, n_mask, _, n_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(n_frames.cpu().numpy()), _bits(before_f)) and not n_mask.cpu().numpy().any()
    assert "plate_fill" not in json.loads(n_meta)["clean_plate"]


# ---- the quality figure ---------------------------------------------------------------------------------------------------------
def true_matrices(jitter_seed=None, jitter_px=0.05):
    """The locked camera's final matrices for the clip's known shake (source -> output: frame i moved back by its shift);
    with a seed, every frame's matrix is shifted by an independent translation of jitter_px in a drawn direction."""
    mats = np.tile(np.eye(3, dtype=np.float64), (N, 1, 1))
    mats[:, 0, 2], mats[:, 1, 2] = -SHIFTS[:, 0], -SHIFTS[:, 1]
    if jitter_seed is not None:
        angle = np.random.default_rng(jitter_seed).uniform(0, 2 * np.pi, N)
        mats[:, 0, 2] += jitter_px * np.cos(angle)
        mats[:, 1, 2] += jitter_px * np.sin(angle)
    return mats.astype(np.float32)


def psnr_db(image, reference, where):
    err = (image.astype(np.float64) - reference.astype(np.float64))[where]
    return float(10.0 * np.log10(1.0 / np.mean(err * err)))


def quality_reference(oracle):
    """-> (the static background through the true matrices with the oracle's warp, reduced to one image; the clip's frames; the
    lowest plate PSNR of the restatement over 8 seeded runs with 0.05 px of error in every frame's matrix, and the 8 figures)."""
    frames, background, _ = plate_clip()
    from tests.deflicker_restatement import _texture

    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    still = np.stack([(0.1 + 0.8 * _texture(xx - dx, yy - dy, 1234)).astype(np.float32) for dx, dy in SHIFTS])    # the clip without its subject
    border = (127 / 255,) * 3
    ref_frames, ref_mask, _ = oracle.warp_clip(still, true_matrices(), (W, H), border=border)
    reference, ref_count = R.plate_median(ref_frames, ref_mask, R.sample_table(None, N))
    figures = []
    for seed in range(8):
        out, mask, _ = oracle.warp_clip(frames, true_matrices(seed), (W, H), border=border)
        plate, count = R.plate_median(out, mask, R.sample_table(None, N))
        figures.append(psnr_db(plate[0], reference[0], (count[0] >= 3) & (ref_count[0] >= 3)))
    return reference[0], ref_count[0], frames, min(figures), figures


def temporal_mean(frames, mask):
    """The plain temporal mean of the valid samples, float64: what the subject stains."""
    valid = (mask <= 0.5)[..., None]
    return (np.where(valid, frames, 0).astype(np.float64).sum(axis=0) / np.maximum(valid.sum(axis=0), 1)).astype(np.float32)


def test_plate_quality_against_the_rendered_background(pkg, ctx, oracle, runs):
    """PSNR of the pipeline's plate (estimated transitions, whose error tests/test_analytic_gpu.py bounds at 0.05 px) against the
    background rendered through the true matrices, over the pixels with count >= 3; it must not fall below the lowest figure
    the CPU restatement gives over 8 seeded runs with 0.05 px of error in every frame's true matrix.  The bound comes from the
    oracle's warp and the restatement on the CPU, never from the code under test."""
    from vstab_amd import clean_plate

    reference, ref_count, _, bound, figures = quality_reference(oracle)
    base = runs["bare"]
    plate, count, _ = clean_plate.plate_on_device(ctx, base.frames, base.masks[..., 0].contiguous())
    plate, count = plate.cpu().numpy()[0], count.cpu().numpy()[0]
    where = (count >= 3) & (ref_count >= 3)
    got = psnr_db(plate, reference, where)
    mean = psnr_db(temporal_mean(*_host(base)), reference, where)
    print(f"plate PSNR {got:.2f} dB, temporal mean {mean:.2f} dB, bound {bound:.2f} dB (8 runs: {[round(f, 2) for f in figures]}), "
          f"pixels {int(where.sum())} of {H * W}")
    assert where.mean() > 0.99 and got > mean
    assert got >= bound, (got, bound)
