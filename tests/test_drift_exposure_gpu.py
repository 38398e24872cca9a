"""GPU: vstab_anchor_sums_ex_batch (csrc/vstab_anchor.hip) and the `drift_exposure` / `drift_mask` keywords of the Flow pipeline.

  1. the kernel equals the NumPy restatement of the second form of the rule (tests/drift_exposure_restatement.py), all 31
     integers, at the shapes where it can go wrong: one pixel, odd sizes, both load paths, the grid's clamp, more than one
     workgroup per frame, an unaligned base, every gain and offset of the range's edges, masks of every kind, the cap's edge
     on the compensated residual; the first entry point still equals its own restatement on the same inputs
  2. end to end on the 64-frame 960x540 similarity clip: an exposure ramp, per-frame flicker, a masked moving subject
  3. composition: off is off, the node
"""

import json

import numpy as np
import pytest

from tests import drift_exposure_restatement as RX
from tests import drift_restatement as R
from tests.drift_util import H, N, W
from tests.drift_util import chain_error as _chain_error
from tests.drift_util import stabilize as _stabilize
from tests.util import shake_path

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
GAINS = (512, 1024, 1331, 2048)
OFFSETS = (-65536, 0, 4097)


def _matrices(h, w):
    """identity, every coordinate a Q5 tie, half out of the frame, a NaN and an inf entry, a similarity, a shift"""
    c, s = 1.003 * np.cos(0.01), 1.003 * np.sin(0.01)
    return np.array([[1, 0, 0, 0, 1, 0], [1, 0, 1 / 64, 0, 1, 1 / 64], [1, 0, w / 2, 0, 1, 0], [1, np.nan, 0, 0, 1, 0],
                     [1, 0, 0, 0, 1, np.inf], [c, -s, 0.37, s, c, -0.81], [1, 0, -0.7, 0, 1, 0.6], [1, 0, 0.4, 0, 1, 2.3]], np.float64)


def _clip(h, w, n, rng):
    """related images at roughly the gains the frames are given, so that pixels fall on both sides of every cap"""
    base = rng.integers(0, 256, (h, w)).astype(np.float64)
    gray = np.empty((n, h, w), np.uint8)
    for i in range(n):
        g = GAINS[i % len(GAINS)] / 1024.0
        gray[i] = np.clip(np.rint(base / 2 * g + OFFSETS[i % len(OFFSETS)] / 1024.0 / 8 + rng.integers(-20, 21, (h, w))), 0, 255)
    gray[0] = (base / 2).astype(np.uint8)
    return gray


@pytest.mark.parametrize("h,w", [(3, 3), (5, 7), (33, 64), (37, 53), (2, 9), (270, 480)])
def test_kernel_equals_the_restatement(pkg, ctx, h, w):
    import torch

    rng = np.random.default_rng(h * 1000 + w)
    mats = _matrices(h, w)
    big = h * w > 10000
    n = 4 if big else 12                                 # 12: every (gain, offset) pair of the two cycles occurs
    gray = _clip(h, w, n, rng)
    anchor = np.zeros(n, np.int64)
    anchor[[1, 2]] = [-1, n - 1]                         # none, and a later frame
    Rm = mats[(np.arange(n) + 5) % len(mats)]
    gain = np.array([GAINS[i % len(GAINS)] for i in range(n)])
    offset = np.array([OFFSETS[i % len(OFFSETS)] for i in range(n)])
    gh, gw = -(-h // 8), -(-w // 8)
    masks = {"none": None, "empty": np.zeros((n, gh, gw), np.uint8), "full": np.full((n, gh, gw), 1, np.uint8),
             "random": (rng.random((n, gh, gw)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (n, gh, gw), dtype=np.uint8)}
    cases = [("none", 32), ("random", 32), ("random", 255)] if big else [(m, cap) for m in masks for cap in (0, 32, 255)]
    dev = torch.from_numpy(gray).cuda()
    buf = torch.empty(n * h * w + 1, dtype=torch.uint8, device="cuda")     # the same bytes one byte into a buffer
    off = buf[1:].view(n, h, w)
    off.copy_(dev)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    for name, cap in cases:
        blocked = masks[name]
        want = RX.anchor_sums_ex_batch(gray, anchor, Rm, cap, gain, offset, blocked, 8)
        dev_blocked = None if blocked is None else torch.from_numpy(blocked).cuda()
        got = ctx.anchor_sums_ex_batch(dev, anchor, Rm, cap, gain, offset, dev_blocked, 8)
        assert got.dtype == np.int64 and got.shape == (n, 31)
        assert np.array_equal(got, want), (name, cap, np.argwhere(got != want)[:5].tolist())
        # w % 16 == 0 with an unaligned base takes the byte loads: the same numbers
        assert np.array_equal(ctx.anchor_sums_ex_batch(off, anchor, Rm, cap, gain, offset, dev_blocked, 8), want), (name, cap)
        if h < 3 or w < 3:
            assert not got.any()
        else:
            assert not got[1].any()                          # anchor -1: zeros
            if name == "full":
                assert not np.delete(got, 2, axis=1).any() and got[0, 2] > 0
            if name == "empty":
                assert np.array_equal(got, RX.anchor_sums_ex_batch(gray, anchor, Rm, cap, gain, offset, None, 8))
    # the defaults are G = 1024, O = 0, and there the 31 numbers hold the 17 of the first entry point, which is unchanged
    for cap in ((32,) if big else (0, 32, 255)):
        plain = ctx.anchor_sums_batch(dev, anchor, Rm, cap)
        assert np.array_equal(plain, R.anchor_sums_batch(gray, anchor, Rm, cap))
        assert np.array_equal(ctx.anchor_sums_ex_batch(dev, anchor, Rm, cap)[:, RX.OLD_SLOTS], plain)
    # a step other than 8 (an odd one, and one larger than the image)
    for step in (3, 1000):
        sh, sw = -(-h // step), -(-w // step)
        blocked = (rng.random((n, sh, sw)) < 0.5).astype(np.uint8)
        want = RX.anchor_sums_ex_batch(gray, anchor, Rm, 32, gain, offset, blocked, step)
        assert np.array_equal(ctx.anchor_sums_ex_batch(dev, anchor, Rm, 32, gain, offset, torch.from_numpy(blocked).cuda(), step), want), step


@pytest.mark.parametrize("cap", [0, 32, 255])
@pytest.mark.parametrize("h,w", [(9, 16), (8, 11)])
def test_the_caps_edge_on_the_compensated_residual(pkg, ctx, h, w, cap):
    """Flat images under the identity: every pixel of frame i has r = 1024 * 150 - 1331 * 100 - O_i = 20500 - O_i.  O puts it
    at +1024 cap (counted), +1024 cap + 1 (capped), -1024 cap (counted) and -1024 cap - 1 (capped): with a gain even cap 255
    caps.  Then the first rule's own edge case through the second entry point: flat images t and t + cap under a shift of
    (1/32, 1/32) with one image pixel one level up -- the four template pixels around it are capped."""
    import torch

    gray = np.stack([np.full((h, w), 100, np.uint8)] + [np.full((h, w), 150, np.uint8)] * 4)
    eye = np.tile([1.0, 0, 0, 0, 1, 0], (5, 1))
    gain = [1024, 1331, 1331, 1331, 1331]
    offset = [0, 20500 - 1024 * cap, 20500 - 1024 * cap - 1, 20500 + 1024 * cap, 20500 + 1024 * cap + 1]
    got = ctx.anchor_sums_ex_batch(torch.from_numpy(gray).cuda(), [-1, 0, 0, 0, 0], eye, cap, gain, offset)
    assert np.array_equal(got, RX.anchor_sums_ex_batch(gray, [-1, 0, 0, 0, 0], eye, cap, gain, offset))
    pixels = (h - 2) * (w - 2)
    assert got[:, :4].tolist() == [[0, 0, 0, 0], [pixels, 0, 0, 1024 * cap * pixels], [0, pixels, 0, 0],
                                   [pixels, 0, 0, 1024 * cap * pixels], [0, pixels, 0, 0]]
    # a flat template has no gradient: of b only the gain's and the offset's entries are set, b4 = T sum r and b5 = sum r
    assert not got[:, 4:8].any() and got[1, 8:10].tolist() == [100 * 1024 * cap * pixels, 1024 * cap * pixels]
    assert got[3, 8:10].tolist() == [-100 * 1024 * cap * pixels, -1024 * cap * pixels]
    t = 0 if cap == 255 else 100
    pair = np.stack([np.full((h, w), t, np.uint8), np.full((h, w), t + cap, np.uint8)])
    pair[1, 3, 3] = t + cap + (-1 if cap == 255 else 1)
    mats = np.array([[1, 0, 0, 0, 1, 0], [1, 0, 1 / 32, 0, 1, 1 / 32]], np.float64)
    got = ctx.anchor_sums_ex_batch(torch.from_numpy(pair).cuda(), [-1, 0], mats, cap)
    assert np.array_equal(got, RX.anchor_sums_ex_batch(pair, [-1, 0], mats, cap))
    assert got[1, :3].tolist() == ([pixels, 0, 0] if cap == 255 else [pixels - 4, 4, 0])


def test_argument_checks(pkg, ctx):
    """Every bad argument is an error of the binding, and past the binding an error code of the library: nothing is launched."""
    import ctypes

    import torch

    from vstab_amd import native

    g = torch.zeros((2, 8, 16), dtype=torch.uint8, device="cuda")
    eye = np.tile([1.0, 0, 0, 0, 1, 0], (2, 1))
    ok_blocked = torch.zeros((2, 1, 2), dtype=torch.uint8, device="cuda")
    for args, kw, match in (((g.float(), [0, 0], eye, 32), {}, "uint8"), ((g, [0], eye, 32), {}, "anchor"), ((g, [0, 2], eye, 32), {}, "outside -1..1"),
                            ((g, [0, 0], eye[:1], 32), {}, "R"), ((g, [0, 0], eye, 256), {}, "cap"), ((g, [0, 0], eye, 32), dict(gain=[1024]), "gain"),
                            ((g, [0, 0], eye, 32), dict(gain=[255, 1024]), "gain outside 256..4096"),
                            ((g, [0, 0], eye, 32), dict(gain=[1024, 4097]), "gain outside 256..4096"),
                            ((g, [0, 0], eye, 32), dict(offset=[0, (1 << 20) + 1]), "offset outside"),
                            ((g, [0, 0], eye, 32), dict(offset=[-(1 << 20) - 1, 0]), "offset outside"),
                            ((g, [0, 0], eye, 32), dict(step=0), "step"), ((g, [0, 0], eye, 32), dict(step=2.5), "step"),
                            ((g, [0, 0], eye, 32), dict(blocked=ok_blocked, step=4), "blocked"),
                            ((g, [0, 0], eye, 32), dict(blocked=ok_blocked.float()), "blocked"),
                            ((torch.zeros((1, 2, 1025), dtype=torch.uint8, device="cuda"), [0], eye[:1], 0), {}, "1024")):
        with pytest.raises(ValueError, match=match):
            ctx.anchor_sums_ex_batch(*args, **kw)
    # the range's ends are accepted
    out = ctx.anchor_sums_ex_batch(g, [-1, 0], eye, 32, gain=[256, 4096], offset=[-(1 << 20), 1 << 20], blocked=ok_blocked)
    assert out.shape == (2, 31) and out[1, 1] == 6 * 14 and not np.delete(out[1], 1).any()       # r = -2^20: all capped
    lib = native.load_library()
    dev_out = torch.zeros((2, 31), dtype=torch.int64, device="cuda")
    a, gain, offset = np.array([0, 0], np.int32), np.array([1024, 1024], np.int32), np.array([0, 0], np.int32)

    def call(anchor=a, gains=gain, offsets=offset, cap=32, blocked=None, step=8, gh=1, gw=2):
        return lib.vstab_anchor_sums_ex_batch(ctx.handle, ctypes.c_void_p(g.data_ptr()), 2, 8, 16, anchor.ctypes.data, eye.ctypes.data,
                                              gains.ctypes.data if gains is not None else None, offsets.ctypes.data, cap,
                                              ctypes.c_void_p(blocked.data_ptr()) if blocked is not None else None, step, gh, gw,
                                              ctypes.c_void_p(dev_out.data_ptr()))

    assert call() == 0
    for kw, words in ((dict(anchor=np.array([0, 5], np.int32)), "anchor[1] = 5 outside"), (dict(gains=np.array([1024, 255], np.int32)), "gain[1] = 255 outside"),
                      (dict(gains=np.array([4097, 1024], np.int32)), "gain[0] = 4097 outside"),
                      (dict(offsets=np.array([0, -(1 << 20) - 1], np.int32)), "offset[1] = -1048577 outside"), (dict(cap=256), "cap 256 outside"),
                      (dict(step=0), "step 0 is not positive"), (dict(blocked=ok_blocked, gh=2), "block grid"),
                      (dict(blocked=ok_blocked, step=4), "block grid"), (dict(gains=None), "NULL pointer")):
        assert call(**kw) != 0 and words in lib.vstab_last_error().decode(), (kw, lib.vstab_last_error().decode())
    assert call(gh=7, gw=9) == 0                                                  # without a grid its size is not read
    torch.cuda.synchronize()


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip(pkg, ctx):
    """The 64-frame 960x540 similarity clip under tests.util.shake_path(seed=3, amp=1.0), as test_drift_correction_gpu.py's."""
    import torch

    import bench

    cam = shake_path(N, W, H, "similarity", seed=3, amp=1.0)
    return cam, bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=cam)


def _report(case, **fields):
    print(json.dumps({"case": case, **fields}))


def test_an_exposure_ramp_no_longer_halves_the_correction(pkg, ctx, clip):
    """frames * linspace(1.0, 0.8): without drift_exposure the keyframe alignment keeps frames by `cost` and the chain's corner
    error is 0.39 px.  With it the chain must meet the project's single-pair bound, 0.05 px at the centre and
    0.075 px at every corner, with no frame kept by `cost`, and be strictly better than without.
    Measured (profiles/r25_drift_exposure.md), centre / corner: 0.126 / 0.393 px without the option (15 frames kept by
    `cost`), 0.0004 / 0.0011 px with it (63 refined, 3 iterations, gains 0.887 .. 1.0)."""
    import torch

    cam, frames = clip
    dim = frames * torch.linspace(1.0, 0.8, N, device=frames.device).view(-1, 1, 1, 1)
    without = _stabilize(ctx, dim, "similarity", drift_correction=True)
    with_it = _stabilize(ctx, dim, "similarity", drift_correction=True, drift_exposure=True)
    c0, k0 = _chain_error(without.meta, cam)
    c1, k1 = _chain_error(with_it.meta, cam)
    b0, b1 = without.meta["drift_correction"], with_it.meta["drift_correction"]
    ex = b1["exposure"]
    _report("ramp", without=[round(c0, 4), round(k0, 4)], with_it=[round(c1, 4), round(k1, 4)], kept_without=b0["frames_kept"],
            kept_with=b1["frames_kept"], iterations=b1["iterations"], gain_min=ex["gain_min"], gain_max=ex["gain_max"],
            residual=[b1["residual_before"], b1["residual_after"]])
    assert "exposure" not in b0 and "gain" not in b0["frames_kept"] and "masked_fraction_mean" not in b1
    assert b1["frames_kept"]["cost"] == 0 and b1["frames_kept"]["gain"] == 0
    assert c1 <= 0.05 and k1 <= 0.075, (c1, k1)
    assert k1 < k0, (c0, k0, c1, k1)
    assert ex["matched"] is True and len(ex["gain"]) == len(ex["offset"]) == N and ex["residual_before_launch"] == 2
    assert ex["gain"][0] == 1.0 and ex["offset"][0] == 0.0 and 0.8 <= ex["gain_min"] < ex["gain_max"] <= 1.0


FLICKER_MEASURED = 0.0051    # the worst |gain[i] - g_i / g_anchor(i)| of the run recorded in profiles/r25_drift_exposure.md
# + one unit of G's quantisation, and one more for the u8 truncation of the gray pass (its mean goes into the offset; what is left
# is noise of 0.29 levels a pixel over half a million pixels)
FLICKER_MARGIN = 2 / 1024


def test_flicker_is_matched_frame_by_frame(pkg, ctx, clip):
    """Per-frame gains in [0.75, 0.95] and offsets in [0, 0.04] (nothing exceeds 1.0, nothing clips).  With drift_exposure
    every anchored frame is refined and its reported gain is the ratio of its gain to its anchor's; without, the block shows
    frames kept by `cost` or `overlap`.  Measured (profiles/r25_drift_exposure.md): worst gain deviation 0.00502, chain 0.0006 /
    0.0016 px with the option; 24 frames kept by `cost` and 0.352 / 0.527 px without."""
    import torch

    cam, frames = clip
    rng = np.random.default_rng(11)
    g, o = rng.uniform(0.75, 0.95, N), rng.uniform(0.0, 0.04, N)
    dev = frames.device
    lit = frames * torch.from_numpy(g).float().to(dev).view(-1, 1, 1, 1) + torch.from_numpy(o).float().to(dev).view(-1, 1, 1, 1)
    assert float(lit.max()) <= 1.0
    without = _stabilize(ctx, lit, "similarity", drift_correction=True).meta["drift_correction"]
    res = _stabilize(ctx, lit, "similarity", drift_correction=True, drift_exposure=True)
    block = res.meta["drift_correction"]
    anchor = [-1] + [32 * ((i - 1) // 32) for i in range(1, N)]               # keyframes 0 and 32; 32's anchor is 0
    want = np.array([1.0] + [g[i] / g[anchor[i]] for i in range(1, N)])
    worst = float(np.max(np.abs(np.array(block["exposure"]["gain"]) - want)))
    c1, k1 = _chain_error(res.meta, cam)
    _report("flicker", worst_gain_deviation=round(worst, 5), chain=[round(c1, 4), round(k1, 4)], kept_with=block["frames_kept"],
            kept_without=without["frames_kept"], refined_without=without["frames_refined"], iterations=block["iterations"])
    assert block["frames_refined"] == N - 1 and block["keyframes"] == [0, 32]
    assert without["frames_kept"]["cost"] + without["frames_kept"]["overlap"] > 0
    assert worst <= FLICKER_MEASURED + FLICKER_MARGIN, worst


def _with_a_subject(frames):
    """A textured rectangle of 0.6 W x 0.5 H (30 % of the frame) that moves 2 px a frame to the right and 1 px down, against a
    camera that only shakes -> (frames with it, its mask [N,H,W])"""
    import torch

    dev = frames.device
    gen = torch.Generator(device="cpu").manual_seed(5)
    rw, rh = int(0.6 * W), int(0.5 * H)
    coarse = torch.rand((1, 3, rh // 6 + 2, rw // 6 + 2), generator=gen)
    texture = torch.nn.functional.interpolate(coarse, scale_factor=6, mode="bilinear", align_corners=False)[0, :, :rh, :rw]
    texture = texture.permute(1, 2, 0).to(dev)
    out = frames.clone()
    mask = torch.zeros((N, H, W), device=dev)
    for i in range(N):
        x0, y0 = 100 + 2 * i, 80 + i
        out[i, y0:y0 + rh, x0:x0 + rw] = texture
        mask[i, y0:y0 + rh, x0:x0 + rw] = 1.0
    return out, mask


def test_a_masked_subject_can_be_anchored(pkg, ctx, clip):
    """drift_correction + estimation_mask raises today's message; with drift_mask=True it runs, reports the masked fraction,
    and the chain's corner error is below that of the same masked call without drift correction.
    Measured (profiles/r25_drift_exposure.md), centre / corner: 0.442 / 0.889 px with estimation_mask alone, 0.0005 / 0.0013 px
    with drift_mask (63 refined, masked_fraction_mean 0.401)."""
    cam, frames = clip
    busy, mask = _with_a_subject(frames)
    with pytest.raises(ValueError) as caught:
        _stabilize(ctx, busy, "similarity", drift_correction=True, estimation_mask=mask)
    assert str(caught.value) == ("drift_correction does not support estimation_mask: the keyframe alignment has no per-pixel exclusion "
                                 "yet (its residual cap is the only guard against moving subjects).")
    plain = _stabilize(ctx, busy, "similarity", estimation_mask=mask)
    res = _stabilize(ctx, busy, "similarity", drift_correction=True, estimation_mask=mask, drift_mask=True)
    c0, k0 = _chain_error(plain.meta, cam)
    c1, k1 = _chain_error(res.meta, cam)
    block = res.meta["drift_correction"]
    _report("mask", without_drift_correction=[round(c0, 4), round(k0, 4)], with_it=[round(c1, 4), round(k1, 4)],
            masked_fraction_mean=block["masked_fraction_mean"], kept=block["frames_kept"], refined=block["frames_refined"],
            capped_fraction_mean=block["capped_fraction_mean"])
    assert 0.0 < block["masked_fraction_mean"] < 1.0 and "exposure" not in block and "estimation_mask" in res.meta
    assert k1 < k0, (k0, k1)
    both = _stabilize(ctx, busy, "similarity", drift_correction=True, estimation_mask=mask, drift_mask=True, drift_exposure=True)
    assert both.meta["drift_correction"]["exposure"]["matched"] and both.meta["drift_correction"]["masked_fraction_mean"] > 0.0


# ---- 3. composition --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short(pkg, ctx):
    import torch

    import bench

    cam = shake_path(14, 480, 270, "similarity", seed=9, amp=1.0)
    return cam, bench.synth_clip(14, 0, 270, 480, torch.device("cuda"), mats=cam)


def test_off_is_off(pkg, ctx, short):
    import torch

    _, frames = short
    ctx.set_timing(True)
    try:
        ctx.anchor_sums_ex_batch(torch.zeros((2, 8, 16), dtype=torch.uint8, device="cuda"), [-1, 0], np.tile([1.0, 0, 0, 0, 1, 0], (2, 1)), 32)
        before = ctx.kernel_ms_stats("anchor_ex")[1]
        for drift in (None, 4):
            want = _stabilize(ctx, frames, "similarity", drift_correction=drift)
            for off in (None, False):
                got = _stabilize(ctx, frames, "similarity", drift_correction=drift, drift_exposure=off, drift_mask=off)
                assert np.array_equal(_bits(got.frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
                assert np.array_equal(_bits(got.masks.cpu().numpy()), _bits(want.masks.cpu().numpy()))
                assert json.dumps(got.meta) == json.dumps(want.meta) and got.device_plan == want.device_plan
        assert ctx.kernel_ms_stats("anchor_ex")[1] == before                   # no launch of the new kernel
        on = _stabilize(ctx, frames, "similarity", drift_correction=4, drift_exposure=True)
        launches = ctx.kernel_ms_stats("anchor_ex")[1] - before
        assert launches == on.meta["drift_correction"]["iterations"] + 1 >= 3
    finally:
        ctx.set_timing(False)
    assert list(on.meta["drift_correction"])[:len(want.meta["drift_correction"])] == list(want.meta["drift_correction"])
    # bypass paths ignore the options as they ignore the keyword
    a = _stabilize(ctx, frames, "similarity", framing="crop", args=(False, 0.7, 0.5, 1.0, (127, 127, 127), 16.0))
    b = _stabilize(ctx, frames, "similarity", framing="crop", args=(False, 0.7, 0.5, 1.0, (127, 127, 127), 16.0), drift_correction=4, drift_exposure=True)
    assert json.dumps(a.meta) == json.dumps(b.meta)


def test_node_equals_the_keyword_call(pkg, ctx, short):
    import torch

    from vstab_amd import nodes

    _, frames = short
    mask = torch.zeros((14, 270, 480))
    mask[:, 60:140, 100:220] = 1.0
    node = nodes.VideoStabilizerFlowAnchoredExposure
    for node_args, kw in (((5, True), dict(drift_exposure=True)), ((5, False), {}),
                          ((5, True, mask, 12), dict(drift_exposure=True, estimation_mask=mask, mask_margin=12, drift_mask=True))):
        want = _stabilize(ctx, frames, "similarity", drift_correction=5, **kw)
        out = node.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F", *node_args)
        node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
        assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
        assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
        assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True)
        assert ("exposure" in node_meta["drift_correction"]) == node_args[1]
