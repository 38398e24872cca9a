"""GPU: the deflicker's three entries (csrc/vstab_deflicker.hip) and the `deflicker` / `deflicker_mode` keywords.

  1. vstab_pair_gain_hist_batch / vstab_pair_gain_sums_batch equal the NumPy restatement (tests/deflicker_restatement.py)
     EXACTLY -- they are integers -- at the shapes where they can go wrong: sizes that are no multiple of the stride, frame
     bytes that are no multiple of 16, two lattice pixels, none, more than one workgroup per pair; transitions with ties,
     outside, W <= 0, a NaN; an inactive pair; levels at both bounds and a float either side; a saturated ratio
  2. vstab_apply_gain_batch equals the restatement in bits: one float32 multiply, untouched values keep theirs
  3. end to end on the synthetic flicker clip, and the node
"""

import json

import numpy as np
import pytest

from tests import deflicker_restatement as R
from tests.drift_util import stabilize as _stabilize

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. the measurement ------------------------------------------------------------------------------------------------------
def _transitions(h, w):
    """identity; a shift of exactly half a pixel (ties to even); a shift that maps every pixel outside; a perspective row with
    W <= 0 over part of the frame; a matrix with a NaN; a small similarity"""
    c, s = 1.01 * np.cos(0.02), 1.01 * np.sin(0.02)
    return np.array([np.eye(3),
                     [[1, 0, 0.5], [0, 1, -0.5], [0, 0, 1]],
                     [[1, 0, 10.0 * w], [0, 1, 0], [0, 0, 1]],
                     [[1, 0, 0], [0, 1, 0], [-2.0 / max(w, 2), 0, 1]],
                     [[1, np.nan, 0], [0, 1, 0], [0, 0, 1]],
                     [[c, -s, 0.4], [s, c, -0.3], [0, 0, 1]]], np.float32)


def _content(n, h, w, rng):
    """Related frames (so that the histograms have a peak), with negative values, values above 1 and NaNs, every level bound
    and one float either side of it on lattice pixels of frames 0 and 1, and lattice pixels whose ratio saturates bin 1023."""
    base = rng.uniform(-0.05, 1.1, (h, w, 3))
    src = np.empty((n, h, w, 3), np.float32)
    for i in range(n):
        src[i] = base * (1.0 + 0.07 * i) + rng.normal(0, 0.01, base.shape)
    src[rng.random(src.shape) < 0.01] = np.nan
    ys, xs = R.lattice(h, w)
    one = np.float32(1)
    edges = [np.float32(v) for v in (2048 / 65536, 63488 / 65536)]
    levels = [f(e) for e in edges for f in (lambda e: e, lambda e: np.nextafter(e, -one), lambda e: np.nextafter(e, one))]
    for j, (y, x) in enumerate(zip(ys, xs)):
        if j < 2 * len(levels):                    # frame 0 at a bound against a mid level, then the other way round
            a, b = (levels[j], np.float32(0.5)) if j < len(levels) else (np.float32(0.5), levels[j - len(levels)])
            src[0, y, x], src[1, y, x] = (a, 0.5, 0.5), (b, 0.5, 0.5)
        elif j < 2 * len(levels) + 3:
            src[0, y, x], src[1, y, x] = (0.04, 0.04, 0.04), (0.9, 0.95, 0.6)      # ratios of 22, 23 and 15: bin 1023
    return src


@pytest.mark.parametrize("n,h,w", [(3, 37, 53), (4, 70, 130), (2, 4, 8), (2, 2, 2), (2, 260, 300)])
def test_hist_and_sums_equal_the_restatement(pkg, ctx, n, h, w):
    import torch

    from vstab_amd import deflicker as D

    rng = np.random.default_rng(n * 100000 + h * 1000 + w)
    src = _content(n, h, w, rng)
    if (h, w) == (37, 53):
        assert (h * w * 12) % 16 != 0                                # frame 1 starts off a 16-byte boundary
    dev = torch.from_numpy(src).to(ctx.device)
    T = _transitions(h, w)
    pairs = n - 1
    rounds = [0] if h * w > 50000 else range(len(T))                 # the large clip: more than one workgroup per pair
    for r in rounds:
        mats = T[(np.arange(pairs) + r) % len(T)]
        for active in ([None] + ([np.arange(pairs) != 1] if pairs > 1 else [np.zeros(1, bool)])):
            want_hist, want_stats = R.pair_gain_hist(src, mats, active)
            hist, stats = ctx.pair_gain_hist_batch(dev, mats, active)
            assert hist.shape == (pairs, 4, 1024) and stats.shape == (pairs, 2)
            hist, stats = hist.cpu().numpy().astype(np.int64), stats.cpu().numpy().astype(np.int64)
            assert np.array_equal(stats, want_stats), (r, stats.tolist(), want_stats.tolist())
            assert np.array_equal(hist, want_hist), (r, np.argwhere(hist != want_hist)[:5].tolist())
            if active is not None:
                off = ~np.asarray(active)
                assert not hist[off].any() and not stats[off].any()
            bands = {"median": D.bands_from_hist(hist)[0], "empty": np.tile(np.array([5, 4], np.int32), (pairs, 4, 1)),
                     "all": np.tile(np.array([0, 1023], np.int32), (pairs, 4, 1)),
                     "mixed": np.tile(np.array([[0, 255], [256, 256], [1023, 1023], [-7, 2000]], np.int32), (pairs, 1, 1))}
            for name, band in bands.items():
                want = R.pair_gain_sums(src, mats, band, active)
                got = ctx.pair_gain_sums_batch(dev, mats, band, active).cpu().numpy()
                assert got.dtype == np.int64 and np.array_equal(got, want), (r, name, np.argwhere(got != want)[:5].tolist())
                if name == "empty":
                    assert not got.any()
                if name == "all":                                    # every well-exposed pixel, in every channel
                    assert np.array_equal(got[:, :, 0], np.repeat(stats[:, 1:2], 4, axis=1))
    if (h, w) == (2, 2):
        assert not want_hist.any() and not want_stats.any()          # no lattice pixel: all outputs are zero
    if (h, w) == (4, 8):
        assert int(R.pair_gain_hist(src, T[:1])[1][0, 0]) == 2       # two lattice pixels, both inside under the identity
    if h * w > 2000:                                                  # the planted content does what it is there for
        hist0, stats0 = R.pair_gain_hist(src, T[:1].repeat(pairs, axis=0))
        assert hist0[0, :, 1023].min() >= 3 and 0 < stats0[0, 1] < stats0[0, 0]


# ---- 2. the correction --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(2, 1, 1), (3, 3, 5), (3, 45, 67), (2, 13, 79)])      # 13 x 79: a tile of 1024 pixels and 3 more
def test_apply_equals_the_restatement_in_bits(pkg, ctx, n, h, w):
    import torch

    rng = np.random.default_rng(h * 1000 + w)
    frames = rng.uniform(-0.2, 1.3, (n, h, w, 3)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.1, 0.9, 1.2, 1.0, 0.0, 0.8], np.float32)
    flat = frames.reshape(-1)
    where = rng.choice(flat.size, size=min(flat.size, max(6, flat.size // 10)), replace=False)
    flat[where] = special[np.arange(len(where)) % len(special)]
    bits = flat.view(np.uint32)
    nan_at = where[np.arange(len(where)) % len(special) == 0]
    bits[nan_at] = 0x7FC00000 | (np.arange(len(nan_at), dtype=np.uint32) * 0x1357 + 1) & 0x3FFFFF        # NaN payloads
    gains = np.tile(np.array([1.25, 1.0, 0.8], np.float32), (n, 1))
    gains[0] = 1.0                                                     # a frame that is not read at all
    if n > 2:
        gains[2] = (1.0, 0.5, 1.0)
    below = np.nextafter(np.float32(1), np.float32(0))
    mask = rng.choice(np.array([0.0, 1.0, below, np.nan, 0.5], np.float32), size=(n, h, w)).astype(np.float32)
    if (h, w) != (1, 1):
        assert (h * w * 12) % 16 != 0                                    # frames start off a 16-byte boundary
    for m in (None, mask):
        want, want_clamped = R.apply_gain(frames, gains, m)
        dev = torch.from_numpy(frames.copy()).to(ctx.device)
        dev_mask = None if m is None else torch.from_numpy(m).to(ctx.device)
        clamped = ctx.apply_gain_batch(dev, gains, dev_mask)
        got = dev.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got.view(np.int32) != want.view(np.int32))[:5].tolist()
        assert np.array_equal(clamped.cpu().numpy().astype(np.int64), want_clamped)
        assert np.array_equal(got[0].view(np.int32), frames[0].view(np.int32))          # gains of exactly 1: the frame's bits
        if m is not None:
            padded = m == np.float32(1.0)
            assert np.array_equal(got[padded].view(np.int32), frames[padded].view(np.int32))
            changed = (got.view(np.int32) != frames.view(np.int32)).any(axis=-1)
            if h * w > 100:
                # only 1.0f itself is padding (a pixel of NaNs, zeros or infinities keeps its bits under any gain)
                assert changed[1][m[1] == below].mean() > 0.9 and changed[1][np.isnan(m[1])].mean() > 0.9
        assert ctx.apply_gain_batch(dev, np.ones((n, 3), np.float32), dev_mask, want_count=False) is None
        assert np.array_equal(dev.cpu().numpy().view(np.int32), want.view(np.int32))
    if h * w > 100:
        assert want_clamped[1] > 0 and want_clamped[0] == 0


def test_apply_single_values(pkg, ctx):
    """0.9 is clamped, 1.2 scaled and not clamped, -0.1 scaled, NaN and inf stay; the count is the clamped values'."""
    import torch

    v = np.array([[[[0.9, 0.9, 0.9]], [[1.2, np.nan, -0.1]], [[np.inf, 1.0, 0.5]]]], np.float32)
    dev = torch.from_numpy(v.copy()).to(ctx.device)
    clamped = ctx.apply_gain_batch(dev, [[1.25, 1.0, 0.8]])
    got = dev.cpu().numpy()
    assert got[0, 0, 0].tolist() == [1.0, np.float32(0.9), np.float32(0.9) * np.float32(0.8)] and clamped.cpu().tolist() == [1]
    assert got[0, 1, 0, 0] == np.float32(1.2) * np.float32(1.25) and np.isnan(got[0, 1, 0, 1])
    assert got[0, 1, 0, 2] == np.float32(-0.1) * np.float32(0.8) and np.isinf(got[0, 2, 0, 0]) and got[0, 2, 0, 1] == 1.0


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
# The restatement's own worst relative error of a pair gain on the clip, with the clip's TRUE transitions, on the CPU
# (tests/test_deflicker_cpu.py asserts them): 0.00171 in mode "exposure", 0.00204 in mode "rgb".  The bound on the GPU run, with
# ESTIMATED transitions, is twice that, for the float32 noise of another seed.  Neither number comes from a GPU run.
BOUND_EXPOSURE = 2 * 0.00171
BOUND_RGB = 2 * 0.00204


@pytest.fixture(scope="module")
def clip():
    frames, gains, shifts, boxes = R.flicker_clip()
    mats = R.true_transitions(shifts)
    pair_gain, measured, inlier = R.measure(frames, mats)
    # the conditions the clip is chosen by, on the restatement alone
    assert measured.all() and inlier.min() >= 0.5
    assert frames[np.isfinite(frames)].max() < 1.5                    # (the value-range rule leaves it alone)
    assert (boxes[:, 2] - boxes[:, 0]).max() * (boxes[:, 3] - boxes[:, 1]).max() <= 0.3 * R.CLIP_W * R.CLIP_H
    return {"frames": frames, "true": gains[1:] / gains[:-1], "mats": mats}


@pytest.fixture(scope="module")
def runs(ctx, clip):
    import torch

    frames = torch.from_numpy(clip["frames"]).to(ctx.device)
    return {"frames": frames, "bare": _stabilize(ctx, frames, "similarity"), "off": _stabilize(ctx, frames, "similarity", deflicker=None),
            "on": _stabilize(ctx, frames, "similarity", deflicker=60)}


def _host(res):
    return res.frames.cpu().numpy(), res.masks.cpu().numpy()


def test_off_is_off(pkg, ctx, runs):
    (f0, m0), (f1, m1) = _host(runs["bare"]), _host(runs["off"])
    assert np.array_equal(_bits(f0), _bits(f1)) and np.array_equal(_bits(m0), _bits(m1))
    assert json.dumps(runs["bare"].meta) == json.dumps(runs["off"].meta) and "deflicker" not in runs["off"].meta
    off2 = _stabilize(ctx, runs["frames"], "similarity", deflicker=False)
    assert json.dumps(off2.meta) == json.dumps(runs["bare"].meta)


def test_pair_gains_are_the_true_ratios_and_beat_the_plain_ratio_of_sums(pkg, ctx, clip, runs):
    from vstab_amd import deflicker as D

    meta = runs["on"].meta
    block = meta["deflicker"]
    assert list(meta) == list(runs["off"].meta) + ["deflicker"]                                  # behind the warp's keys
    assert block["pairs_unmeasured"] == 0 and block["inlier_fraction_min"] >= 0.5 and block["mode"] == "exposure"
    got = np.asarray(block["pair_gain"], np.float64)
    err = np.abs(got / clip["true"] - 1).max(axis=1)
    print("pair_gain relative error per pair:", np.round(err, 5).tolist(), "bound", BOUND_EXPOSURE)
    # the plain ratio of sums (band [0, 1023]) through the same transitions; the subject touches every pair of this clip
    mats = np.array([t["matrix"] for t in meta["estimated_motion"]["per_transition"]], np.float32)
    sums = ctx.pair_gain_sums_batch(runs["frames"], mats, np.tile(np.array([0, 1023], np.int32), (len(mats), 4, 1))).cpu().numpy()
    plain = D.gains_from_sums(sums)[0][:, 3]
    err_plain = np.abs(plain / clip["true"][:, 0] - 1)
    print("plain ratio of sums, relative error per pair:", np.round(err_plain, 5).tolist())
    print("step rms before / after:", block["step_rms_before"], block["step_rms_after"])
    assert (err <= BOUND_EXPOSURE).all(), err.tolist()
    assert (err < err_plain).all(), (err.tolist(), err_plain.tolist())
    assert block["step_rms_after"] < block["step_rms_before"]
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()                     # one gain for the three colours
    corr = np.asarray(block["correction"])
    assert (corr[:, 0] == corr[:, 1]).all() and (corr[:, 0] == corr[:, 2]).all() and block["frames_clamped"] == 0
    # the frames are the warp's, times the corrections, under the mask -- the restatement's apply rule on the run without it
    f_off, m_off = _host(runs["off"])
    f_on, m_on = _host(runs["on"])
    want, clamped = R.apply_gain(f_off, corr.astype(np.float32), m_off[..., 0])
    assert np.array_equal(_bits(f_on), _bits(want)) and np.array_equal(_bits(m_on), _bits(m_off))
    assert block["values_clamped"] == int(clamped.sum())
    assert {k: v for k, v in meta.items() if k != "deflicker"} == runs["off"].meta              # nothing else in the meta moves


def test_the_stability_report_sees_it(pkg, ctx, runs):
    off = _stabilize(ctx, runs["frames"], "similarity", stability_report=True)
    on = _stabilize(ctx, runs["frames"], "similarity", stability_report=True, deflicker=60)
    a, b = off.meta["stability"]["after"]["itf_db"], on.meta["stability"]["after"]["itf_db"]
    print("after.itf_db without / with deflicker:", a, b)
    assert b > a
    assert on.meta["stability"]["before"] == off.meta["stability"]["before"]                     # the source is not touched
    assert list(on.meta).index("deflicker") < list(on.meta).index("stability")


def test_both_plan_paths_give_the_same_bits(pkg, ctx, runs, monkeypatch):
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("VSTAB_DEVICE_PLAN", flag)
        out[flag] = _stabilize(ctx, runs["frames"], "similarity", deflicker=60)
    assert out["1"].device_plan["used"] and not out["0"].device_plan["used"]
    (f0, m0), (f1, m1) = _host(out["0"]), _host(out["1"])
    assert np.array_equal(_bits(f0), _bits(f1)) and np.array_equal(_bits(m0), _bits(m1))
    assert out["0"].meta["deflicker"] == out["1"].meta["deflicker"] == runs["on"].meta["deflicker"]


def test_rgb_mode_recovers_a_white_balance_step(pkg, ctx):
    import torch

    frames, gains, shifts, _ = R.flicker_clip(rgb=True)
    assert frames[np.isfinite(frames)].max() < 1.5
    true = gains[1:] / gains[:-1]
    assert np.abs(true[:, 1] / true[:, 0] - 1).max() > 0.1              # green really differs from red and blue
    dev = torch.from_numpy(frames).to(ctx.device)
    rgb = _stabilize(ctx, dev, "similarity", deflicker=60, deflicker_mode="rgb").meta["deflicker"]
    got = np.asarray(rgb["pair_gain"], np.float64)
    err = np.abs(got / true - 1)
    print("rgb pair_gain relative error:", float(err.max()), "bound", BOUND_RGB)
    assert rgb["mode"] == "rgb" and rgb["pairs_unmeasured"] == 0 and (err <= BOUND_RGB).all(), err.max(axis=1).tolist()
    assert np.abs((got[:, 1] / got[:, 0]) / (true[:, 1] / true[:, 0]) - 1).max() <= 2 * BOUND_RGB
    exp = _stabilize(ctx, dev, "similarity", deflicker=60, deflicker_mode="exposure").meta["deflicker"]
    corr = np.asarray(exp["correction"])
    assert exp["mode"] == "exposure" and (corr[:, 0] == corr[:, 1]).all() and (corr[:, 0] == corr[:, 2]).all()
    assert rgb["step_rms_after"] < rgb["step_rms_before"]


def test_it_composes_with_the_other_passes(pkg, ctx, runs):
    """`crop` framing has no mask; the exposure-matched fill, the spatial fill and scene cuts run behind it."""
    crop = _stabilize(ctx, runs["frames"], "translation", framing="crop", deflicker=60)
    assert crop.meta["deflicker"]["pairs_unmeasured"] == 0 and crop.meta["deflicker"]["step_rms_after"] < 0.01
    res = _stabilize(ctx, runs["frames"], "similarity", deflicker=True, deflicker_mode="rgb", temporal_fill=2, fill_exposure=True,
                     spatial_fill=True, scene_cuts=[6], estimator="classic")
    keys = list(res.meta)
    assert keys.index("deflicker") < keys.index("temporal_fill") < keys.index("spatial_fill")
    assert res.meta["deflicker"]["pair_gain"][5] is None and res.meta["deflicker"]["radius_frames"] == 8


# ---- the node -------------------------------------------------------------------------------------------------------------------
def test_the_node_with_and_without_a_meta(pkg, ctx, clip, runs):
    import torch

    from vstab_amd import deflicker as D
    from vstab_amd import nodes

    off, on = runs["off"], runs["on"]
    meta = json.loads(json.dumps(off.meta))
    before = off.frames.cpu().numpy()
    out = nodes.VideoStabilizerDeflicker.execute(runs["frames"], off.frames, off.masks, meta, 60.0, "exposure")
    node_frames, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(on.frames.cpu().numpy()))
    assert json.loads(node_meta) == {"deflicker": on.meta["deflicker"]}
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(before))                        # the input is not written to

    # without a meta: identity transitions on the frames themselves -- the whole restatement on the CPU
    still = np.minimum(clip["frames"][:1].repeat(6, axis=0) * np.linspace(0.8, 1.2, 6, dtype=np.float32)[:, None, None, None],
                       np.float32(1.45))
    eye = np.tile(np.eye(3, dtype=np.float32), (5, 1, 1))
    gains, finish = D.solve(D.Request(0.25, "rgb"), lambda act: R.pair_gain_hist(still, eye, act),
                            lambda act, band: R.pair_gain_sums(still, eye, band, act), np.ones(5), 6, 16.0)
    want, clamped = R.apply_gain(still, gains)
    dev = torch.from_numpy(still).to(ctx.device)
    out = nodes.VideoStabilizerDeflicker.execute(dev, dev, None, None, 0.25, "rgb")
    node_frames, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want))
    assert json.loads(node_meta) == {"deflicker": finish(int(clamped.sum()))}
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(still))
