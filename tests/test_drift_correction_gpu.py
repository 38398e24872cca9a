"""GPU: vstab_anchor_sums_batch (csrc/vstab_anchor.hip) and the `drift_correction` keyword of the Flow pipeline.

  1. the kernel equals the NumPy restatement of the rule (tests/drift_restatement.py), all 17 integers, at the shapes where
     it can go wrong: one pixel, odd sizes, both load paths, more than one workgroup per frame, an unaligned base, anchors
     of every kind, matrices that leave the frame or are not finite, the cap's edge
  2. accuracy: the chain of the reported transitions of a 64-frame clip against the analytic camera path, every frame
  3. the lock: a camera-locked similarity clip shows the static texture better with the keyword than without
  4. composition: off is off, scene cuts, temporal fill, stability report, the sharded refusal, the node
"""

import json

import numpy as np
import pytest

from tests import drift_restatement as R
from tests.drift_util import ARGS, LOCK_ARGS, H, N, W
from tests.drift_util import chain_error as _chain_error
from tests.drift_util import stabilize as _stabilize
from tests.util import shake_path

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
def _matrices(h, w):
    """identity, every coordinate a Q5 tie, half out of the frame, far outside, a flip, a NaN and an inf entry, a similarity"""
    c, s = 1.003 * np.cos(0.01), 1.003 * np.sin(0.01)
    return np.array([
        [1, 0, 0, 0, 1, 0],
        [1, 0, 1 / 64, 0, 1, 1 / 64],
        [1, 0, w / 2, 0, 1, 0],
        [1, 0, 10.0 * w, 0, 1, -10.0 * h],
        [-1, 0, w - 1, 0, 1, 0],
        [1, np.nan, 0, 0, 1, 0],
        [1, 0, 0, 0, 1, np.inf],
        [c, -s, 0.37, s, c, -0.81],
        [1, 0, -0.7, 0, 1, 0.6],
    ], np.float64)


def _anchors(n, rng):
    """-1, the frame itself, a later frame and an earlier one all occur"""
    a = rng.integers(-1, n, n)
    a[0] = n - 1            # a later frame
    a[1] = 1                # the frame itself
    if n > 2:
        a[2] = -1
    if n > 3:
        a[3] = 0
    return a


@pytest.mark.parametrize("h,w", [(3, 3), (5, 7), (33, 64), (37, 53), (270, 480), (2, 9)])
def test_kernel_equals_the_restatement(pkg, ctx, h, w):
    import torch

    rng = np.random.default_rng(h * 1000 + w)
    mats = _matrices(h, w)
    for n in range(2, 10):
        gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        if n % 2:                                   # related images, so that b and H are not only noise
            gray[1:] = np.roll(gray[:1], 1, axis=2)
        anchor = _anchors(n, rng)
        Rm = mats[(np.arange(n) + n) % len(mats)]
        for cap in (0, 32, 255):
            want = R.anchor_sums_batch(gray, anchor, Rm, cap)
            got = ctx.anchor_sums_batch(torch.from_numpy(gray).cuda(), anchor, Rm, cap)
            assert got.dtype == np.int64 and got.shape == (n, 17)
            assert np.array_equal(got, want), (n, cap, np.argwhere(got != want)[:5].tolist())
            if h < 3 or w < 3:
                assert not got.any()
    # every matrix at least once on one clip, anchored to frame 0
    n = len(mats)
    gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    anchor = np.zeros(n, np.int64)
    want = R.anchor_sums_batch(gray, anchor, mats, 255)
    dev = torch.from_numpy(gray).cuda()
    assert np.array_equal(ctx.anchor_sums_batch(dev, anchor, mats, 255), want)
    if h >= 3 and w >= 3:
        assert want[0, 0] == (h - 2) * (w - 2) and not want[3].any() and not want[5].any() and not want[6].any()
    # an unaligned base address: the same bytes one byte into a buffer (the 16-byte loads are not taken)
    buf = torch.empty(n * h * w + 1, dtype=torch.uint8, device="cuda")
    off = buf[1:].view(n, h, w)
    off.copy_(dev)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    assert np.array_equal(ctx.anchor_sums_batch(off, anchor, mats, 255), want)


@pytest.mark.parametrize("cap", [0, 32, 255])
@pytest.mark.parametrize("h,w", [(9, 16), (8, 11)])
def test_the_caps_edge(pkg, ctx, h, w, cap):
    """A pixel with |r| == 1024 cap exactly counts, one with 1024 cap + 1 is capped.  Flat images t and t + cap under a shift of
    (1/32, 1/32): every pixel has r = 1024 cap.  One image pixel raised by 1 enters the four template pixels around it with
    the weights 1, 31, 31 and 961: r = 1024 cap + 1, ... -- four capped pixels.  cap 255 caps nothing: there the pixel is
    lowered by 1 instead (255 is the top of the range)."""
    import torch

    t = 0 if cap == 255 else 100
    gray = np.stack([np.full((h, w), t, np.uint8), np.full((h, w), t + cap, np.uint8)])
    gray[1, 3, 3] = t + cap + (-1 if cap == 255 else 1)
    mats = np.array([[1, 0, 0, 0, 1, 0], [1, 0, 1 / 32, 0, 1, 1 / 32]], np.float64)
    got = ctx.anchor_sums_batch(torch.from_numpy(gray).cuda(), [-1, 0], mats, cap)
    assert np.array_equal(got, R.anchor_sums_batch(gray, [-1, 0], mats, cap))
    pixels = (h - 2) * (w - 2)
    if cap == 255:
        assert got[1, :3].tolist() == [pixels, 0, 1024 * cap * pixels - (1 + 31 + 31 + 961)]
    else:
        assert got[1, :3].tolist() == [pixels - 4, 4, 1024 * cap * (pixels - 4)]
    assert not got[0].any() and not got[1, 3:].any()          # a flat template has no gradient


@pytest.mark.parametrize("h,w", [(3, 3), (37, 53), (48, 64)])
def test_equal_images_under_the_identity(pkg, ctx, h, w):
    import torch

    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    got = ctx.anchor_sums_batch(torch.from_numpy(np.stack([img, img, img])).cuda(), [1, 2, 0], np.tile([1.0, 0, 0, 0, 1, 0], (3, 1)), 0)
    assert np.all(got[:, 0] == (h - 2) * (w - 2)) and not got[:, 1:7].any()
    assert np.all(got[:, 7] > 0) or (h, w) == (3, 3)


def test_argument_checks(pkg, ctx):
    import torch

    from vstab_amd import native

    g = torch.zeros((2, 8, 16), dtype=torch.uint8, device="cuda")
    eye = np.tile([1.0, 0, 0, 0, 1, 0], (2, 1))
    for bad, match in (((g.float(), [0, 0], eye, 32), "uint8"), ((g, [0], eye, 32), "anchor"), ((g, [0, 2], eye, 32), "outside -1..1"),
                       ((g, [0, -2], eye, 32), "outside -1..1"), ((g, [0, 0], eye[:1], 32), "R"), ((g, [0, 0], eye, 256), "cap"),
                       ((g, [0, 0], eye, 1.5), "cap"), ((torch.zeros((1, 2, 1025), dtype=torch.uint8, device="cuda"), [0], eye[:1], 0), "1024")):
        with pytest.raises(ValueError, match=match):
            ctx.anchor_sums_batch(*bad)
    # the library's own checks, reached past the binding's
    import ctypes

    lib = native.load_library()
    out = torch.zeros((2, 17), dtype=torch.int64, device="cuda")
    a = np.array([0, 5], np.int32)
    rc = lib.vstab_anchor_sums_batch(ctx.handle, ctypes.c_void_p(g.data_ptr()), 2, 8, 16, a.ctypes.data, eye.ctypes.data, 32,
                                     ctypes.c_void_p(out.data_ptr()))
    assert rc != 0 and "anchor[1] = 5 outside" in lib.vstab_last_error().decode()


# ---- 2. accuracy -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clips(pkg, ctx):
    """The 64-frame 960x540 clips under tests.util.shake_path(seed=3, amp=1.0), made once."""
    import torch

    import bench

    out = {}
    for kind in ("similarity", "translation"):
        cam = shake_path(N, W, H, kind, seed=3, amp=1.0)
        out[kind] = (cam, bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=cam))
    return out


@pytest.fixture(scope="module")
def plain_runs(ctx, clips):
    return {kind: _stabilize(ctx, clips[kind][1], kind) for kind in clips}


@pytest.mark.parametrize("kind,spacing,drifts", [("similarity", True, 0.3), ("similarity", 16, 0.3), ("translation", True, 0.1)])
def test_the_chain_stays_on_the_analytic_path(pkg, ctx, clips, plain_runs, kind, spacing, drifts):
    """Without the keyword the chain of 63 pair estimates drifts (the CPU oracle, which the HIP path equals: 0.759 px at the
    worst corner of the similarity clip, 0.161 px on the translation clip); with it every frame of the chain meets the
    project's single-pair bounds, 0.05 px at the centre and 0.075 px at every corner (a float64 prototype: 0.003 px).
    Measured, centre / corner: similarity 0.275 / 0.759 without, 0.0004 / 0.0012 with a keyframe every 32 frames and 0.0007 /
    0.0015 every 16; translation 0.171 without, 0.0011 with; 2 iterations and 63 frames refined in each
    (profiles/r23_drift_correction.md)."""
    cam, frames = clips[kind]
    centre0, corner0 = _chain_error(plain_runs[kind].meta, cam)
    res = _stabilize(ctx, frames, kind, drift_correction=spacing)
    centre1, corner1 = _chain_error(res.meta, cam)
    block = res.meta["drift_correction"]
    print(json.dumps({"case": f"{kind} spacing {spacing}", "without": [round(centre0, 4), round(corner0, 4)],
                      "with": [round(centre1, 4), round(corner1, 4)], "block": {k: v for k, v in block.items() if k != "keyframes"}}))
    assert "drift_correction" not in plain_runs[kind].meta
    assert corner0 > drifts, (centre0, corner0)                    # the clip drifts
    assert centre1 <= 0.05 and corner1 <= 0.075, (centre1, corner1)
    s = 32 if spacing is True else spacing
    assert block["frames_refined"] == N - 1 and block["frames_kept"] == {"singular": 0, "overlap": 0, "cost": 0, "step": 0, "no_anchor": 1}
    assert block["version"] == 1 and block["spacing"] == s and block["keyframes"] == list(range(0, N, s)) and block["path_model"] == "anchored"
    assert 1 <= block["iterations"] <= 6 and block["residual_cap"] == 32 and block["residual_after"] <= block["residual_before"]
    assert 0.0 < block["correction_px_max"] < 4.0 and 0.0 <= block["capped_fraction_mean"] < 0.5
    assert list(res.meta).index("drift_correction") > list(res.meta).index("motion_meta") and not res.device_plan["used"]
    tr = res.meta["estimated_motion"]["per_transition"]
    plain = plain_runs[kind].meta["estimated_motion"]["per_transition"]
    assert [(t["mode"], t["confidence"], t["residual"]) for t in tr] == [(t["mode"], t["confidence"], t["residual"]) for t in plain]


# ---- 3. the lock -----------------------------------------------------------------------------------------------------------
LOCK_GATE_DB = 61.27    # the measured PSNR with the keyword, 62.27 dB, less 1 dB of headroom (profiles/r23_drift_correction.md)


def test_a_locked_similarity_clip_shows_the_static_texture(pkg, ctx, clips):
    """camera_lock at strength 1 on the SIMILARITY clip (the existing translation-only test reaches 51-55 dB and gates at 48).
    With the keyword the PSNR against the analytically sampled static texture must exceed the run without it.  Measured:
    43.24 dB without (mean |error| 0.0076, worst frame 63: the drift and the additive path), 62.27 dB with (mean |error|
    0.0010, max 0.0049, worst frame 8): above the translation-only clip's 48 dB gate, so no remainder is left to explain."""
    import torch

    import bench

    cam, frames = clips["similarity"]
    dev = torch.device("cuda")
    without = bench.static_texture_error(_stabilize(ctx, frames, "similarity", args=LOCK_ARGS), cam, frames, dev)
    res = _stabilize(ctx, frames, "similarity", args=LOCK_ARGS, drift_correction=True)
    with_it = bench.static_texture_error(res, cam, frames, dev)
    print(json.dumps({"case": "lock", "without": without, "with": with_it}))
    assert np.all(np.array(res.meta["estimated_motion"]["target_path"]) == 0.0)
    assert with_it["safe_fraction"] > 0.8
    assert with_it["psnr_db"] > without["psnr_db"], (with_it, without)
    assert with_it["psnr_db"] >= LOCK_GATE_DB, with_it
    # strength 1 applies C_i^-1: the applied matrix times the pose is the recentring shift alone
    off = res.meta["framing"]["center_offset"]
    applied = np.array([f["applied_matrix"] for f in res.meta["stabilization_warp"]["per_frame"]], np.float64)
    acc = np.eye(3)
    worst = 0.0
    pts = np.array([[0, 0, 1.0], [W - 1, 0, 1.0], [0, H - 1, 1.0], [W - 1, H - 1, 1.0]]).T
    for i, t in enumerate(res.meta["estimated_motion"]["per_transition"]):
        acc = np.asarray(t["matrix"], np.float64) @ acc
        moved = (applied[i + 1] @ acc @ pts)[:2] - pts[:2] - np.array(off)[:, None]
        worst = max(worst, float(np.hypot(*moved).max()))
    assert worst < 2e-3, worst                    # float32 matrices at 960 px


# ---- 4. composition --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short(pkg, ctx):
    import torch

    import bench

    cam = shake_path(14, 480, 270, "similarity", seed=9, amp=1.0)
    return cam, bench.synth_clip(14, 0, 270, 480, torch.device("cuda"), mats=cam)


def test_off_is_off(pkg, ctx, short):
    _, frames = short
    want = _stabilize(ctx, frames, "similarity")
    for off in (None, 0, False):
        got = _stabilize(ctx, frames, "similarity", drift_correction=off)
        assert np.array_equal(_bits(got.frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
        assert np.array_equal(_bits(got.masks.cpu().numpy()), _bits(want.masks.cpu().numpy()))
        assert json.dumps(got.meta) == json.dumps(want.meta) and got.device_plan == want.device_plan
    for bypass_kw in (dict(framing="crop", args=(False, 0.7, 0.5, 1.0, (127, 127, 127), 16.0)),):
        a = _stabilize(ctx, frames, "similarity", **bypass_kw)
        b = _stabilize(ctx, frames, "similarity", drift_correction=4, **bypass_kw)
        assert json.dumps(a.meta) == json.dumps(b.meta) and "drift_correction" not in b.meta
    one = _stabilize(ctx, frames[:1].contiguous(), "similarity", drift_correction=4)
    assert "drift_correction" not in one.meta and one.meta["frames"] == 1


def test_every_shot_equals_the_shot_run_alone(pkg, ctx, short):
    _, frames = short
    res = _stabilize(ctx, frames, "similarity", scene_cuts=[5, 6], drift_correction=3)
    em = res.meta["estimated_motion"]
    block = res.meta["drift_correction"]
    assert block["keyframes"] == [0, 3, 5, 6, 9, 12] and block["frames_kept"]["no_anchor"] == 3
    refined = 0
    for s, e in ((0, 5), (5, 6), (6, 14)):
        alone = _stabilize(ctx, frames[s:e].contiguous(), "similarity", drift_correction=3)
        if e - s < 2:
            assert "drift_correction" not in alone.meta
            continue
        am = alone.meta["estimated_motion"]
        assert em["path"][s:e] == am["path"] and em["target_path"][s:e] == am["target_path"]
        for a, b in zip(em["per_transition"][s:e - 1], am["per_transition"]):
            assert (a["mode"], a["confidence"], a["residual"], a["matrix"]) == (b["mode"], b["confidence"], b["residual"], b["matrix"])
        assert alone.meta["drift_correction"]["keyframes"] == [k - s for k in block["keyframes"] if s <= k < e]
        refined += alone.meta["drift_correction"]["frames_refined"]
    assert block["frames_refined"] == refined == 14 - 3


def test_it_composes_and_the_sharded_path_refuses(pkg, ctx, short):
    from vstab_amd import distributed

    _, frames = short
    res = _stabilize(ctx, frames, "similarity", drift_correction=4, temporal_fill=2, stability_report=True)
    assert "temporal_fill" in res.meta and "stability" in res.meta and res.meta["drift_correction"]["frames_refined"] == 13
    both = list(_stabilize(ctx, frames, "similarity", drift_correction=4, rolling_shutter=0.3).meta)
    assert both.index("drift_correction") == both.index("rolling_shutter") + 1        # behind it in the key order
    for estimator in ("flow_tvl1", "flow_phase_correlate", "classic"):
        mode = "translation" if estimator == "flow_phase_correlate" else "similarity"
        for framing in ("crop", "expand"):
            got = _stabilize(ctx, frames, mode, framing=framing, estimator=estimator, drift_correction=4)
            kept = got.meta["drift_correction"]["frames_kept"]
            assert got.meta["drift_correction"]["frames_refined"] + sum(kept.values()) == 14 and kept["no_anchor"] >= 1
    with pytest.raises(ValueError, match="the keyframe alignment is not sharded"):
        distributed.stabilize_sharded(ctx, frames, len(frames), "crop_and_pad", "similarity", *ARGS, drift_correction=True)


def test_node_equals_the_keyword_call(pkg, ctx, short):
    from vstab_amd import nodes

    _, frames = short
    want = _stabilize(ctx, frames, "similarity", drift_correction=5)
    out = nodes.VideoStabilizerFlowAnchored.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F", 5)
    node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
    assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
    assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True) and node_meta["drift_correction"]["spacing"] == 5
