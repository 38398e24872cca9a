"""Rolling shutter on the GPU (include/vstab.h "rolling shutter"; flow_pipeline._stabilize_frames(rolling_shutter=...)).

  1. vstab_rolling_warp_batch against the NumPy restatement (tests/rolling_shutter_restatement.py): frames, mask and counts in
     bits, at the shapes where the tile can go wrong; all-zero velocity == vstab_warp_batch in bits
  2. vstab_row_residual_batch against the restatement: exact equality
  3. end to end on an analytic rolling clip: (a) the run == the restatement's warp with the run's own matrices and velocities,
     (b) it helps, (c) "auto" finds the readout, (d) off is off

The clip of test 3: the bench's texture seen through a smooth analytic camera (rolling_shutter_restatement.CameraPath) whose
rows are taken at time i + rho * (y/(H-1) - 1/2), rho = 0.7; rho = 0 renders the global-shutter twin.  12 frames, 480 x 270,
camera_lock and strength 1, so the ideal output is the static texture.  The path moves the picture by up to 6.4 x 5.3 px per
frame: enough for 2.7 px of skew at the corners (asserted from the path), and little enough for DIS, which lost half a frame
on several paths that moved this texture by 8 px per frame at this size, the global-shutter twin's included.

The figures behind (b) and (c) were measured on the CPU, through the oracle's estimation chain, the package's host plan and the
restatement's warp (tools/rolling_shutter_report.py --cpu), and are recorded in profiles/r20_rolling_shutter.md:
  similarity   PSNR none 26.81 dB, rolling 30.21 dB, twin 35.91 dB: share 0.374 of the gap; "auto" readout 0.6433 (error 0.0567)
  translation  PSNR none 25.35 dB, rolling 30.61 dB, twin 31.81 dB: share 0.814 of the gap; "auto" readout 0.7146 (error 0.0146)
(b) asserts half of the measured share -- half, because it is a quality figure on one synthetic clip -- and (c) twice the
measured error.  (The similarity share is the smaller one because a similarity fit takes part of the shear for rotation and
scale, into the transitions themselves: the plan then turns the frames by it, which no row correction undoes.  DESIGN 8k.)
"""

import json
import math

import numpy as np
import pytest

from tests import rolling_shutter_restatement as R
from tests import util

pytestmark = pytest.mark.gpu

LOCK_ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the target path is 0
ARGS = (False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
E2E = dict(n=12, w=480, h=270, rho=0.7, amp=(24.0, 20.0, 0.004, 0.004), omega=0.3, seed=4)
SKEW_MIN_PX = 2.0
# measured on the CPU (see above; profiles/r20_rolling_shutter.md)
MEASURED_SHARE = {"similarity": 0.374, "translation": 0.814}
MEASURED_AUTO_ERROR = {"similarity": 0.0567, "translation": 0.0146}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _stabilize(ctx, frames, mode="similarity", estimator="flow", framing="crop_and_pad", args=LOCK_ARGS, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, *args, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


# ---- 1. the warp == the restatement, in bits -------------------------------------------------------------------------------
def _warp_case(n, size, out_size, rho, seed):
    """n frames with one velocity of each kind (cycled) and matrices that map the source onto the output canvas, one of them
    pushing part of the canvas outside the source."""
    w, h = size
    ow, oh = out_size
    rng = np.random.default_rng(seed)
    fit = np.diag([ow / w, oh / h, 1.0])
    mats = np.stack([fit @ m for m in util.test_matrices(n, w, h, "similarity", seed=seed)])
    mats[n - 1] = fit @ util.similarity(0.4 * w, -0.3 * h, 0.05, 1.0, w / 2, h / 2)          # part of the canvas sees no source
    sign = 1.0 if rho >= 0 else -1.0
    kinds = []
    vel = np.zeros((n, 6))
    for i in range(n):
        kind = ("realistic", "zeros", "nan", "clamp", "realistic")[i % 5]
        if kind == "realistic":      # a few px per frame plus small rotation / scale terms
            th, sc = rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
            vel[i] = (sc, -th, rng.uniform(-6, 6) - sc * w / 2 + th * h / 2, th, sc, rng.uniform(-4, 4) - th * w / 2 - sc * h / 2)
        elif kind == "nan":
            vel[i] = (0.0, 0.0, 3.0, np.nan, 0.0, -2.0)
        elif kind == "clamp":        # rho * vy / (H - 1) > 1/2 everywhere: D is clamped to 0.5
            vel[i] = (0.0, 0.0, 2.5, 0.0, 0.0, sign * 4.0 * h / max(abs(rho), 0.25))
            assert rho * vel[i, 5] / (h - 1) > 0.5
        kinds.append(kind)
    return mats.astype(np.float32), vel, kinds


@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("size,out_size", [((61, 45), (61, 45)), ((65, 9), (130, 17)), ((160, 90), (177, 95))])
def test_rolling_warp_equals_the_restatement(pkg, ctx, subpix, size, out_size):
    import torch

    w, h = size
    border = (0.2, 0.4, 0.6)
    seen = set()
    for n in (1, 5):
        frames = util.synth_frames(n, h, w, seed=w + n)
        dev_frames = torch.from_numpy(frames).cuda()
        for rho in (1.0, -1.0, 0.3):
            mats, vel, kinds = _warp_case(n, size, out_size, rho, seed=w + n)
            seen.update(kinds)
            want, want_mask, want_cnt = R.rolling_warp(frames, mats, out_size, vel, rho, border, subpix)
            got, got_mask, got_cnt = ctx.rolling_warp_batch(dev_frames, mats, out_size, vel, rho, border=border, subpix=subpix)
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (n, rho, subpix)
            assert np.array_equal(_bits(got_mask.cpu().numpy()), _bits(want_mask)), (n, rho, subpix)
            assert got_cnt.cpu().numpy().tolist() == want_cnt.tolist()
            assert 0 < want_cnt[n - 1] < out_size[0] * out_size[1]              # the last matrix: part of the canvas is outside
            no_mask = ctx.rolling_warp_batch(dev_frames, mats, out_size, vel, rho, border=border, subpix=subpix, want_mask=False)
            assert no_mask[1] is None and no_mask[2] is None
            assert np.array_equal(_bits(no_mask[0].cpu().numpy()), _bits(want))
            no_count = ctx.rolling_warp_batch(dev_frames, mats, out_size, vel, rho, border=border, subpix=subpix, want_count=False)
            assert no_count[2] is None                                         # the mask without the count reduction
            assert torch.equal(no_count[0].view(torch.int32), got.view(torch.int32))
            assert torch.equal(no_count[1].view(torch.int32), got_mask.view(torch.int32))
            plain, plain_mask, plain_cnt = ctx.warp_batch(dev_frames, mats, out_size, interp="bilinear", border=border, subpix=subpix,
                                                          want_mask=True, want_count=True)
            for i, kind in enumerate(kinds):
                same = torch.equal(got[i].view(torch.int32), plain[i].view(torch.int32))
                if kind == "zeros":      # all-zero velocity: the plain warp, bit for bit
                    assert same and torch.equal(got_mask[i].view(torch.int32), plain_mask[i].view(torch.int32))
                    assert int(got_cnt[i]) == int(plain_cnt[i])
                elif kind in ("realistic", "clamp"):
                    assert not same, (kind, rho)                               # the displacement did something
    assert seen == {"realistic", "zeros", "nan", "clamp"}


@pytest.mark.parametrize("subpix", ["q5", "exact"])
def test_zero_readout_and_zero_velocity_are_the_plain_warp(pkg, ctx, subpix):
    import torch

    for kind, (w, h), out_size in (("similarity", (333, 187), (333, 187)), ("perspective", (160, 90), (177, 95)),
                                   ("horizon", (160, 90), (160, 90)), ("similarity", (61, 45), (333, 11))):
        n = 3
        frames = torch.from_numpy(util.synth_frames(n, h, w, seed=w + h)).cuda()
        mats = util.test_matrices(n, w, h, kind, seed=5).astype(np.float32)
        border = (0.2, 0.4, 0.6)
        want, want_mask, want_cnt = ctx.warp_batch(frames, mats, out_size, interp="bilinear", border=border, subpix=subpix,
                                                   want_mask=True, want_count=True)
        moving = np.tile([0.01, -0.004, 5.0, 0.004, 0.01, -3.0], (n, 1))
        for vel, rho in ((np.zeros((n, 6)), 1.0), (np.zeros((n, 6)), -0.3), (moving, 0.0)):
            got, got_mask, got_cnt = ctx.rolling_warp_batch(frames, mats, out_size, vel, rho, border=border, subpix=subpix)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, subpix, rho)
            assert torch.equal(got_mask.view(torch.int32), want_mask.view(torch.int32))
            assert torch.equal(got_cnt, want_cnt)


@pytest.mark.parametrize("subpix", ["q5", "exact"])
def test_a_row_time_shifts_the_rows_by_a_known_amount(pkg, ctx, subpix):
    """Known answer: a horizontal velocity of 8 px per frame and readout 1 move the top row by -1/2 * 8 = -4 px, the bottom row
    by +4 px and leave the middle row alone (H - 1 = 16 rows apart, so rows 0, 8 and 16 are shifted by whole pixels)."""
    import torch

    h, w = 17, 48
    src = util.synth_frames(1, h, w, seed=4)
    vel = np.array([[0.0, 0.0, 8.0, 0.0, 0.0, 0.0]])
    got, mask, _ = ctx.rolling_warp_batch(torch.from_numpy(src).cuda(), np.eye(3, dtype=np.float32)[None], (w, h), vel, 1.0,
                                          border=(0.1, 0.2, 0.3), subpix=subpix)
    got, mask = got.cpu().numpy()[0], mask.cpu().numpy()[0]
    # s = q + tau * v: the top row (tau = -1/2) samples 4 px to the left, the bottom row (tau = +1/2) 4 px to the right
    assert np.array_equal(got[0, 4:], src[0, 0, :w - 4]) and (mask[0, :4] == 1).all() and not mask[0, 4:].any()
    assert np.array_equal(got[8], src[0, 8]) and not mask[8].any()
    assert np.array_equal(got[16, :w - 4], src[0, 16, 4:]) and (mask[16, w - 4:] == 1).all()


def test_argument_checks(pkg, ctx):
    import torch

    from vstab_amd import native

    frames = torch.zeros((2, 8, 8, 3), device="cuda")
    eye = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    with pytest.raises(ValueError, match=r"velocity \(1, 6\) is not \[2,6\]"):
        ctx.rolling_warp_batch(frames, eye, (8, 8), np.zeros((1, 6)), 0.5)
    for bad in (1.5, float("nan")):
        with pytest.raises(ValueError, match=r"readout=.* outside \[-1, 1\]"):
            ctx.rolling_warp_batch(frames, eye, (8, 8), np.zeros((2, 6)), bad)
    with pytest.raises(native.VstabError, match="the source must have at least 2 rows"):
        ctx.rolling_warp_batch(torch.zeros((2, 1, 8, 3), device="cuda"), eye, (8, 8), np.zeros((2, 6)), 0.5)
    g = torch.zeros((2, 5, 8, 2), device="cuda")
    with pytest.raises(ValueError, match="is not a 64x48 image at step 8"):
        ctx.row_residual_batch(g, 8, (64, 48), eye)
    with pytest.raises(ValueError, match=r"are not \[2,3,3\]"):
        ctx.row_residual_batch(g, 8, (64, 40), eye[:1])
    with pytest.raises(ValueError, match="blocked"):
        ctx.row_residual_batch(g, 8, (64, 40), eye, blocked=torch.zeros((2, 5, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(native.VstabError, match="a row of 4100 grid positions exceeds 4096"):
        ctx.row_residual_batch(torch.zeros((1, 2, 4100, 2), device="cuda"), 8, (32800, 16), eye[:1])


# ---- 2. the row residual == the restatement, exactly ----------------------------------------------------------------------
def _draw_rows(rng, pairs, w, h, step):
    gh, gw = -(-h // step), -(-w // step)
    x = (np.arange(gw) * step).astype(np.float64)[None, :].repeat(gh, 0)
    y = (np.arange(gh) * step).astype(np.float64)[:, None].repeat(gw, 1)
    kinds = ["perspective", "similarity", "translation"]          # pair 0 is projective
    mats = np.stack([util.test_matrices(1, w, h, kinds[i % 3], seed=int(rng.integers(0, 1 << 30)))[0] for i in range(pairs)]).astype(np.float32)
    flow = np.empty((pairs, gh, gw, 2), np.float32)
    for i in range(pairs):
        A = mats[i].astype(np.float64)
        W = A[2, 0] * x + A[2, 1] * y + A[2, 2]
        flow[i, ..., 0] = (A[0, 0] * x + A[0, 1] * y + A[0, 2]) / W - x + rng.normal(0, 0.7, (gh, gw)) + 0.02 * (y - h / 2)
        flow[i, ..., 1] = (A[1, 0] * x + A[1, 1] * y + A[1, 2]) / W - y + rng.normal(0, 0.7, (gh, gw))
    flow[:, : max(1, gh // 2), : max(1, gw // 3)] = np.round(flow[:, : max(1, gh // 2), : max(1, gw // 3)] * 2) / 2      # ties in the rank
    return flow, mats, gh, gw


@pytest.mark.parametrize("pairs", [1, 4])
@pytest.mark.parametrize("w,h", [(61, 45), (64, 64), (960, 16)])
def test_row_residual_equals_the_restatement(pkg, ctx, w, h, pairs):
    import torch

    rng = np.random.default_rng(w * 7 + h + pairs)
    step = 8
    flow, mats, gh, gw = _draw_rows(rng, pairs, w, h, step)
    assert mats[0, 2, 0] != 0.0                                   # a projective transition
    # row 0: every sample admitted (an even count: gw is 8 or 120).  Row 1: one non-finite sample (7 of 8: below the minimum;
    # 119 of 120: an odd count).  The last row: blocked down to 3 samples.
    flow[:, 1, 2, 0] = np.nan
    if gh > 2:
        flow[:, 2, 1, 1] = np.inf
        flow[:, 2, 5, 0] = -np.inf
    blocked = np.zeros((pairs + 1, gh, gw), np.uint8)
    blocked[0, gh - 1, 3:] = 1                                    # in frame 0: blocks pair 0
    blocked[1:, gh - 1, : gw - 3] = 1                             # in the later frames: blocks every pair
    if gw > 8:
        blocked[pairs, 0, 7] = 1                                  # the second frame of the last pair: row 0 has 119 there
    seen = {}
    for blk in (None, blocked):
        want_res, want_cnt = R.row_residual(flow, step, (w, h), mats, blk)
        got_res, got_cnt = ctx.row_residual_batch(torch.from_numpy(flow).cuda(), step, (w, h), mats,
                                                  blocked=None if blk is None else torch.from_numpy(blk).cuda())
        assert got_cnt.dtype == torch.int32 and got_res.dtype == torch.float32
        assert tuple(got_res.shape) == (pairs, gh, 2) and tuple(got_cnt.shape) == (pairs, gh)
        assert np.array_equal(got_cnt.cpu().numpy(), want_cnt)
        assert np.array_equal(_bits(got_res.cpu().numpy()), _bits(want_res))
        assert np.isfinite(want_res).all()
        seen[blk is None] = (want_res, want_cnt)
    res, cnt = seen[True]
    assert (cnt[:, 0] == gw).all() and gw % 2 == 0 and res[:, 0].any()          # an even count: (lo + hi) / 2
    assert (cnt[:, 1] == gw - 1).all()
    if gw == 8:
        assert not res[:, 1].any()                                             # 7 samples: below VSTAB_ROW_MIN_SAMPLES
    else:
        assert res[:, 1].any()                                                 # 119 samples, an odd count: the middle element
    res_b, cnt_b = seen[False]
    assert (cnt_b[:, gh - 1] <= 3).all() and not res_b[:, gh - 1].any()        # starved: (0, 0) and the true count
    if gw > 8:
        assert cnt_b[pairs - 1, 0] == gw - 1 and res_b[pairs - 1, 0].any()


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
def e2e_path():
    return R.CameraPath(E2E["w"], E2E["h"], amp=E2E["amp"], omega=E2E["omega"], seed=E2E["seed"])


def final_matrices(meta):
    return np.array([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)


def interior(masks, radius):
    """Pixels at least `radius` inside mask == 0 (the frame's edge counts as padding): bool [N,H,W]."""
    import torch.nn.functional as F

    k = 2 * radius + 1
    padded = F.pad((masks > 0).float()[:, None], (radius,) * 4, value=1.0)
    return F.max_pool2d(padded, k, stride=1)[:, 0] == 0


def psnr(out, ideal, sel):
    err = ((out - ideal) ** 2).sum(-1)[sel]
    return 10.0 * math.log10(1.0 / (float(err.mean()) / 3.0))


def static_ideal(final0, h, w, device, seed=1234):
    """The locked camera shows frame 0's content -- the texture itself, the path vanishes at t = 0 -- moved by frame 0's
    matrix (the recentring translation)."""
    import torch

    from tests import mesh_restatement as M

    assert np.array_equal(final0[:2, :2], np.eye(2, dtype=np.float32)) and np.array_equal(final0[2], np.float32([0, 0, 1]))
    yy, xx = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32), torch.arange(w, device=device, dtype=torch.float32),
                            indexing="ij")
    return M.texture(xx - float(final0[0, 2]), yy - float(final0[1, 2]), h, w, seed)


def share_of_the_gap(runs, h, w, device):
    """runs = (none, rolling, twin): (frames [N,H,W,3], mask [N,H,W], final matrices) each -> (PSNR of each against the static
    texture over the pixels all three show, 4 px inside; the share of the none-to-twin gap that `rolling` recovers)."""
    import torch

    sel = interior(torch.maximum(torch.maximum(runs[0][1], runs[1][1]), runs[2][1]), 4)
    assert float(sel.float().mean()) > 0.5
    p = [psnr(f, static_ideal(final[0], h, w, device), sel) for f, _, final in runs]
    return p, (p[1] - p[0]) / (p[2] - p[0])


def test_the_clip_is_skewed_by_two_pixels():
    path = e2e_path()
    skew = [path.corner_skew(i, E2E["rho"]) for i in range(E2E["n"])]
    assert max(skew) >= SKEW_MIN_PX, skew


@pytest.mark.parametrize("mode", ["translation", "similarity"])
def test_end_to_end_on_a_rolling_clip(pkg, ctx, mode):
    import torch

    dev = torch.device("cuda")
    n, w, h, rho = E2E["n"], E2E["w"], E2E["h"], E2E["rho"]
    path = e2e_path()
    assert max(path.corner_skew(i, rho) for i in range(n)) >= SKEW_MIN_PX
    frames = R.rolling_clip(path, n, rho, dev)
    twin_frames = R.rolling_clip(path, n, 0.0, dev)
    none = _stabilize(ctx, frames, mode)
    on = _stabilize(ctx, frames, mode, rolling_shutter=rho)
    twin = _stabilize(ctx, twin_frames, mode)
    auto = _stabilize(ctx, frames, mode, rolling_shutter="auto")

    # (a) the run is the restatement's warp of the clip with the run's own matrices and velocities, in bits
    block = on.meta["rolling_shutter"]
    assert block["version"] == 1 and block["readout"] == rho and block["source"] == "given" and block["estimate"] is None
    final = final_matrices(on.meta)
    assert np.array_equal(final, final_matrices(none.meta))                # the global part is the same plan
    velocity = np.array(block["velocity"], np.float64)
    assert velocity.shape == (n, 6) and np.abs(velocity[:, [2, 5]]).max() > 3.0
    want, want_mask, want_cnt = R.rolling_warp(frames.cpu().numpy(), final, (w, h), velocity, rho, np.float32([127, 127, 127]) / np.float32(255.0))
    assert np.array_equal(_bits(on.frames.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(on.masks[..., 0].cpu().numpy()), _bits(want_mask))
    pixels = np.float32(w * h)
    assert on.meta["padding_fraction_max"] == float((want_cnt.astype(np.float32) / pixels).astype(np.float64).max())
    assert set(on.meta) - set(none.meta) == {"rolling_shutter"} and set(none.meta) <= set(on.meta)
    assert block["skew_px_max"] >= SKEW_MIN_PX * 0.8                        # what the estimated velocities amount to

    # (b) it helps: at least half of the share of the gap to the global-shutter twin that was measured on the CPU
    runs = [(r.frames, r.masks[..., 0], final_matrices(r.meta)) for r in (none, on, twin)]
    (p_none, p_on, p_twin), share = share_of_the_gap(runs, h, w, dev)
    print(f"\nrolling_shutter {mode}: PSNR none {p_none:.2f} dB, rolling {p_on:.2f} dB, global-shutter twin {p_twin:.2f} dB; "
          f"share {share:.3f}; meta {json.dumps({k: v for k, v in block.items() if k != 'velocity'})}")
    assert p_on > p_none
    assert share >= 0.5 * MEASURED_SHARE[mode], (p_none, p_on, p_twin)

    # (c) "auto" finds the readout: the sign, and the value within twice the error measured on the CPU
    ab = auto.meta["rolling_shutter"]
    print(f"rolling_shutter {mode} auto: {json.dumps({k: v for k, v in ab.items() if k != 'velocity'})}")
    assert ab["source"] == "estimated" and ab["readout"] > 0.0
    assert abs(ab["readout"] - rho) <= 2.0 * MEASURED_AUTO_ERROR[mode], ab["readout"]
    assert ab["estimate"]["pairs_used"] == n - 3 and ab["estimate"]["signal_rms_px"] >= 0.05
    assert ab["velocity"] == block["velocity"]
    json.loads(json.dumps(auto.meta))


@pytest.mark.parametrize("estimator,framing,mode", [("flow", "crop_and_pad", "similarity"), ("flow", "expand", "translation"),
                                                    ("classic", "crop_and_pad", "similarity")])
def test_off_is_off(pkg, ctx, estimator, framing, mode):
    """(d) None and 0 are the call without the keyword: frames, mask and meta byte for byte, no new kernel launched."""
    import bench
    import torch

    n, w, h = 12, 480, 270
    frames = bench.synth_clip(n, 0, h, w, torch.device("cuda"), mats=util.shake_path(n, w, h, mode, seed=3))
    ctx.set_timing(True)
    try:
        # one launch of each new kernel, so that both timing kinds exist
        ctx.row_residual_batch(torch.zeros((1, 2, 2, 2), device="cuda"), 8, (16, 16), np.eye(3, dtype=np.float32)[None])
        ctx.rolling_warp_batch(torch.zeros((1, 8, 8, 3), device="cuda"), np.eye(3, dtype=np.float32)[None], (8, 8), np.zeros((1, 6)), 0.5)
        ctx.set_timing(True)                                   # clears the totals: 0 launches of either kind from here on
        plain = _stabilize(ctx, frames, mode, estimator, framing, args=ARGS)
        offs = [_stabilize(ctx, frames, mode, estimator, framing, args=ARGS, rolling_shutter=v) for v in (None, 0, 0.0)]
        assert ctx.kernel_ms_stats("row_residual")[1] == 0 and ctx.kernel_ms_stats("rolling_warp")[1] == 0
        given = _stabilize(ctx, frames, mode, estimator, framing, args=ARGS, rolling_shutter=-0.4)
        assert ctx.kernel_ms_stats("row_residual")[1] == 0 and ctx.kernel_ms_stats("rolling_warp")[1] == 1
        assert given.meta["rolling_shutter"]["readout"] == -0.4 and given.meta["rolling_shutter"]["source"] == "given"
        assert tuple(given.frames.shape) == tuple(plain.frames.shape)
        if estimator == "flow":
            _stabilize(ctx, frames, mode, estimator, framing, args=ARGS, rolling_shutter="auto")
            assert ctx.kernel_ms_stats("row_residual")[1] == 1 and ctx.kernel_ms_stats("rolling_warp")[1] == 2
    finally:
        ctx.set_timing(False)
    for off in offs:
        assert np.array_equal(_bits(plain.frames.cpu().numpy()), _bits(off.frames.cpu().numpy()))
        assert np.array_equal(_bits(plain.masks.cpu().numpy()), _bits(off.masks.cpu().numpy()))
        assert json.dumps(plain.meta, sort_keys=True) == json.dumps(off.meta, sort_keys=True) and "rolling_shutter" not in off.meta
        assert plain.device_plan == off.device_plan


def test_it_composes_and_the_refusals_raise(pkg, ctx):
    import torch

    from vstab_amd import distributed

    dev = torch.device("cuda")
    path = e2e_path()
    frames = R.rolling_clip(path, 8, 0.7, dev)
    mask = torch.zeros((E2E["h"], E2E["w"]))
    mask[100:170, 200:300] = 1.0
    res = _stabilize(ctx, frames, estimation_mask=mask, rolling_shutter="auto", framing="expand", scene_cuts=[4], spatial_fill=True,
                     stability_report=True, mask_grow=3)
    block = res.meta["rolling_shutter"]
    assert res.meta["estimation_mask"]["blocked_fraction_max"] > 0.0 and res.meta["scene_cuts"]["cuts"] == [4]
    assert "spatial_fill" in res.meta and "stability" in res.meta and "mask_handoff" in res.meta
    assert block["source"] in ("estimated", "not_observable") and block["estimate"]["pairs_used"] == 2      # pairs 1 and 5
    for estimator in ("flow_tvl1", "classic", "flow_phase_correlate"):
        small = frames[:4, ::2, ::2].contiguous()
        got = _stabilize(ctx, small, "translation", estimator, rolling_shutter=0.5)
        assert got.meta["rolling_shutter"]["readout"] == 0.5 and len(got.meta["rolling_shutter"]["velocity"]) == 4
    for kw, text in ((dict(mode="perspective"), "is not affine"), (dict(framing="crop"), "the crop solver bounds matrices only"),
                     (dict(mesh_warp=True), "the warp takes one displacement"), (dict(temporal_fill=3), "have not been corrected"),
                     (dict(sharpness_transfer=2), "have not been corrected"), (dict(dynamic_zoom=True), "does not know the per-row"),
                     (dict(estimator="classic", rolling_shutter="auto"), "no grid of flow samples")):
        with pytest.raises(ValueError, match=text):
            _stabilize(ctx, frames, **dict(dict(rolling_shutter=0.5), **kw))
    with pytest.raises(ValueError, match="the rolling-shutter correction is not sharded"):
        distributed.stabilize_sharded(ctx, frames, len(frames), "crop_and_pad", "similarity", *ARGS, rolling_shutter=0.5)


def test_node_equals_the_keyword_call(pkg, ctx):
    import torch

    from vstab_amd import nodes

    frames = R.rolling_clip(e2e_path(), 8, 0.7, torch.device("cuda"))
    for readout, kw in ((0.0, dict(rolling_shutter="auto")), (0.7, dict(rolling_shutter=0.7))):
        want = _stabilize(ctx, frames, args=ARGS, **kw)
        out = nodes.VideoStabilizerFlowRolling.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F",
                                                       readout)
        node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
        assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
        assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
        assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True)
        assert node_meta["rolling_shutter"]["source"] == ("given" if readout else "estimated")
