"""CPU: the deflicker's restatement against an independent referee, its host arithmetic (deflicker.py) on hand-made cases,
and every refusal of the keyword -- all without a GPU."""

import asyncio
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import deflicker_restatement as R

ROOT = Path(__file__).resolve().parents[1]


class NoClip:                      # never touched: the checks come first (len(None) would be a TypeError)
    frames = None


def _call(**keywords):
    from vstab_amd import flow_pipeline

    framing = keywords.pop("framing_mode", "crop_and_pad")
    return flow_pipeline._stabilize_frames(NoClip(), framing, "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0, **keywords)


# ---- the restatement against a referee of per-pixel Python loops ----------------------------------------------------------
def _q_scalar(v):
    v = np.float32(v)
    if not v > 0:                  # a NaN too
        return 0
    if not v < 1:
        return 65536
    return int(np.float32(v * np.float32(65536.0)))


def _referee(a, b, A, band=None):
    """One 12 x 9 pair, pixel by pixel -> (inside, well, bins per channel as lists, sums [4][3])."""
    h, w = a.shape[:2]
    A = np.asarray(A, np.float32).astype(np.float64).reshape(9)
    inside = well = 0
    bins = [[], [], [], []]
    sums = [[0, 0, 0] for _ in range(4)]
    for y in range(h):
        for x in range(w):
            if x % 4 != 2 or y % 4 != 2:
                continue
            X, Y, W = (A[0] * x + A[1] * y) + A[2], (A[3] * x + A[4] * y) + A[5], (A[6] * x + A[7] * y) + A[8]
            if not (W > 0 and np.isfinite(W)):
                continue
            qx, qy = np.rint(X / W), np.rint(Y / W)
            if not (0 <= qx <= w - 1 and 0 <= qy <= h - 1):
                continue
            inside += 1
            qa = [_q_scalar(a[y, x, c]) for c in range(3)]
            qb = [_q_scalar(b[int(qy), int(qx), c]) for c in range(3)]
            if not all(2048 <= v <= 63488 for v in qa + qb):
                continue
            well += 1
            qa.append(sum(qa))
            qb.append(sum(qb))
            for c in range(4):
                bn = min((qb[c] * 256) // qa[c], 1023)
                bins[c].append(bn)
                if band is not None and band[c][0] <= bn <= band[c][1]:
                    sums[c][0] += 1
                    sums[c][1] += qa[c]
                    sums[c][2] += qb[c]
    return inside, well, bins, sums


@pytest.mark.parametrize("matrix", [np.eye(3), [[1, 0, 0.5], [0, 1, 1.5], [0, 0, 1]], [[1, 0, 2.5], [0, 1, -1], [0, 0, 1]],
                                    [[1, 0.02, 1], [-0.02, 1, 0], [1e-3, 0, 0.995]], [[1, 0, 0], [0, 1, 0], [-0.2, 0, 1]]])
def test_restatement_equals_the_per_pixel_referee(matrix):
    rng = np.random.default_rng(3)
    a = rng.uniform(0.02, 1.02, (9, 12, 3)).astype(np.float32)
    b = (a * np.float32(1.1) + rng.normal(0, 0.02, a.shape)).astype(np.float32)
    a[2, 2] = (np.nan, 0.5, 0.5)
    a[2, 6] = (2048 / 65536, 63488 / 65536, 0.5)                         # exactly at both bounds: well exposed
    b[6, 6] = (-0.5, 0.5, 0.5)
    src, mats = np.stack([a, b]), np.asarray(matrix, np.float32)[None]
    hist, stats = R.pair_gain_hist(src, mats)
    band = [[0, 1023], [250, 300], [5, 4], [281, 281]]
    inside, well, bins, sums = _referee(a, b, matrix, band)
    assert (int(stats[0, 0]), int(stats[0, 1])) == (inside, well)
    for c in range(4):
        assert np.array_equal(hist[0, c], np.bincount(np.asarray(bins[c], np.int64), minlength=1024))
    assert R.pair_gain_sums(src, mats, [band]).tolist() == [sums]
    assert R.pair_gain_sums(src, mats, [band], active=[0]).tolist() == [[[0, 0, 0]] * 4]
    assert not R.pair_gain_hist(src, mats, active=[0])[0].any()
    # the cumulative-count median is numpy's lower median of the per-pixel bins
    _, med = R.bands_from_hist(hist)
    for c in range(4):
        if bins[c]:
            assert med[0, c] == np.sort(bins[c])[(len(bins[c]) - 1) // 2]
            if len(bins[c]) % 2:
                assert med[0, c] == np.median(bins[c])


def test_ties_round_to_even_and_the_lattice_of_small_frames():
    assert [len(R.lattice(h, w)[0]) for h, w in ((2, 2), (4, 8), (3, 3), (37, 53))] == [0, 2, 1, 9 * 13]
    a = np.full((9, 12, 3), 0.25, np.float32)
    b = np.full((9, 12, 3), 0.25, np.float32)
    b[:, 2::4] = 0.5                       # x + 0.5 = 2.5, 6.5, 10.5 -> 2, 6, 10 (ties to even), never 3, 7, 11
    hist, stats = R.pair_gain_hist(np.stack([a, b]), np.array([[[1, 0, 0.5], [0, 1, 0], [0, 0, 1]]], np.float32))
    assert stats.tolist() == [[6, 6]] and hist[0, :, 512].tolist() == [6, 6, 6, 6]


def test_apply_restatement_on_single_values():
    v = np.array([[[[0.9, 0.9, 0.9]], [[1.2, np.nan, -0.1]], [[np.inf, 1.0, 0.5]]]], np.float32)      # [1,3,1,3]
    out, clamped = R.apply_gain(v, [[1.25, 1.0, 0.8]])
    assert out[0, 0, 0].tolist() == [1.0, np.float32(0.9), np.float32(np.float32(0.9) * np.float32(0.8))] and clamped.tolist() == [1]
    assert out[0, 1, 0, 0] == np.float32(1.2) * np.float32(1.25) and np.isnan(out[0, 1, 0, 1])           # scaled, not clamped
    assert out[0, 1, 0, 2] == np.float32(-0.1) * np.float32(0.8)
    assert np.isinf(out[0, 2, 0, 0]) and out[0, 2, 0, 1] == 1.0
    mask = np.array([[[1.0], [np.nan], [np.nextafter(np.float32(1), np.float32(0))]]], np.float32)
    out2, clamped2 = R.apply_gain(v, [[1.25, 1.0, 0.8]], mask)
    assert np.array_equal(out2[0, 0].view(np.int32), v[0, 0].view(np.int32)) and clamped2.tolist() == [0]
    assert np.array_equal(out2[0, 1:].view(np.int32), out[0, 1:].view(np.int32))


# ---- deflicker.py against the restatement and on hand-made cases ----------------------------------------------------------
def test_bands_from_hist(pkg):
    from vstab_amd import deflicker as D

    hist = np.zeros((4, 4, 1024), np.int64)
    hist[0, 0, [10, 20, 30]] = (1, 1, 1)          # median 20
    hist[0, 1, [10, 20]] = (1, 1)                 # two samples: the LOWER one
    hist[0, 2, 1023] = 5
    hist[0, 3, 256] = 7
    hist[1, :, 0] = 3                             # bin 0: the band is [0, 0]
    hist[2, 0, [100, 300]] = (5, 4)
    hist[2, 1, [100, 300]] = (4, 5)
    band, med = D.bands_from_hist(hist)
    assert med[0].tolist() == [20, 10, 1023, 256] and band[0].tolist() == [[18, 23], [9, 12], [896, 1151], [224, 288]]
    assert band[1].tolist() == [[0, 0]] * 4
    assert med[2, :2].tolist() == [100, 300]
    assert med[3].tolist() == [-1] * 4 and band[3].tolist() == [[1, 0]] * 4 and band.dtype == np.int32      # empty: lo > hi
    rng = np.random.default_rng(0)
    many = rng.integers(0, 50, (6, 4, 1024)) * (rng.random((6, 4, 1024)) < 0.1)
    got, want = D.bands_from_hist(many), R.bands_from_hist(many)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="are not"):
        D.bands_from_hist(np.zeros((2, 3, 1024)))


def test_gains_from_sums_and_modes(pkg):
    from vstab_amd import deflicker as D

    sums = np.zeros((3, 4, 3), np.int64)
    sums[0] = [[256, 1000, 1100], [300, 1000, 900], [1000, 4000, 4000], [256, 3000, 3300]]
    sums[1] = [[255, 1000, 2000]] * 3 + [[256, 100, 200]]               # one sample short in r, g, b
    g, ok = D.gains_from_sums(sums)
    assert g[0].tolist() == [1.1, 0.9, 1.0, 1.1] and ok[0].all()
    assert ok[1].tolist() == [False, False, False, True] and g[1].tolist() == [1.0, 1.0, 1.0, 2.0]
    assert not ok[2].any()
    gr, okr = R.gains_from_sums(sums)
    assert np.array_equal(g, gr) and np.array_equal(ok, okr)
    pg, m = D.pair_gains(g, ok, "exposure")
    assert pg.tolist() == [[1.1] * 3, [2.0] * 3, [1.0] * 3] and m.tolist() == [True, True, False]
    pg, m = D.pair_gains(g, ok, "rgb")
    assert pg.tolist() == [[1.1, 0.9, 1.0], [1.0] * 3, [1.0] * 3] and m.tolist() == [True, False, False]


def test_corrections_hand_made(pkg):
    from vstab_amd import deflicker as D

    # a lone flash in a flat chain: L = 0, ln 2, 0 -> mean ln2 / 3
    c, hit, L = D.corrections([[2.0] * 3, [0.5] * 3], [True, True], 3, 1)
    assert np.allclose(L[:, 0], [0, np.log(2), 0]) and not hit.any()
    assert np.allclose(c[:, 0], [np.exp(np.log(2) / 2), np.exp(np.log(2) / 3 - np.log(2)), np.exp(np.log(2) / 2)])
    # a window longer than the clip: every frame is brought to the chain's mean, and the corrected chain is flat
    g = np.array([[1.2] * 3, [0.7] * 3, [1.1] * 3, [0.95] * 3])
    c, hit, L = D.corrections(g, [True] * 4, 5, 1000)
    assert np.allclose(np.log(g[:, 0]) + np.log(c[1:, 0]) - np.log(c[:-1, 0]), 0, atol=1e-15)
    assert D.step_rms(g, [True] * 4, c) < 1e-15 < D.step_rms(g, [True] * 4)
    # a segment split at an unmeasured pair: nothing is carried over it, and a frame alone in its segment gets exactly 1
    c, hit, L = D.corrections([[2.0] * 3, [1.0] * 3, [1.0] * 3, [3.0] * 3], [True, True, False, True], 5, 10)
    assert D.chain_segments(5, [True, True, False, True]) == [(0, 3), (3, 5)]
    assert np.allclose(L[:, 0], [0, np.log(2), np.log(2), 0, np.log(3)])
    assert np.allclose(c[3:, 0], [np.sqrt(3), 1 / np.sqrt(3)])
    c, _, _ = D.corrections([[2.0] * 3, [1.0] * 3, [3.0] * 3], [False, True, False], 4, 2)
    assert c[0].tolist() == [1.0] * 3 and c[3].tolist() == [1.0] * 3 and np.allclose(c[1:3], 1.0)
    # scene cuts split as well
    assert D.chain_segments(6, [True] * 5, [(0, 2), (2, 6)]) == [(0, 2), (2, 6)]
    assert D.chain_segments(6, [True, True, True, False, True], [(0, 2), (2, 6)]) == [(0, 2), (2, 4), (4, 6)]
    # the clamp: one stop at most, and counted
    c, hit, _ = D.corrections([[16.0, 1.0, 1.0]], [True], 2, 5)
    assert c[:, 0].tolist() == [2.0, 0.5] and hit.tolist() == [True, True] and c[:, 1].tolist() == [1.0, 1.0]
    # a constant gain is a ramp: its high-pass is small in the middle of a long clip
    c, _, _ = D.corrections(np.full((20, 3), 1.02), [True] * 20, 21, 2)
    assert np.allclose(c[2:-2], 1.0, atol=1e-12) and c[0, 0] > 1.0 > c[-1, 0]
    # and against the restatement's loops
    rng = np.random.default_rng(5)
    g = np.exp(rng.normal(0, 0.2, (30, 3)))
    linked = rng.random(30) > 0.15
    segs = [(0, 11), (11, 12), (12, 31)]
    for r in (1, 3, 50):
        got = D.corrections(np.where(linked[:, None], g, 1.0), linked, 31, r, segs)
        want = R.corrections(np.where(linked[:, None], g, 1.0), linked, 31, r, segs)
        assert np.allclose(got[0], want[0], rtol=1e-12) and np.array_equal(got[1], want[1])
    assert [D.radius_frames(*a) for a in ((1.0, 16.0), (0.01, 16.0), (60, 16.0), (1.0, 25.0), (0.5, 30.0))] == [8, 1, 480, 13, 8]


def test_active_pairs(pkg):
    from vstab_amd import deflicker as D

    assert D.active_pairs([0.5, 0.0, np.nan, 1.0], 5).tolist() == [True, False, False, True]
    assert D.active_pairs([0.5, 0.5, 0.5, 1.0], 5, [(0, 2), (2, 5)]).tolist() == [True, False, True, True]
    with pytest.raises(ValueError, match="confidences"):
        D.active_pairs([1.0], 5)


def test_solve_on_the_restatement_and_the_meta_block(pkg):
    """The module's arithmetic end to end on the CPU, fed by the restatement's two passes on the synthetic clip with its true
    transitions.  These are the conditions the GPU test's clip is chosen by."""
    from vstab_amd import deflicker as D

    frames, gains, shifts, _ = R.flicker_clip()
    mats = R.true_transitions(shifts)
    conf = np.ones(len(mats))
    request = D.check_request(60, None)
    g32, finish = D.solve(request, lambda act: R.pair_gain_hist(frames, mats, act),
                          lambda act, band: R.pair_gain_sums(frames, mats, band, act), conf, len(frames), 16.0)
    block = finish(7)
    assert json.loads(json.dumps(block)) == block                       # survives JSON as it is
    assert list(block) == ["version", "mode", "window_s", "radius_frames", "stride", "pair_gain", "pairs_unmeasured",
                           "well_exposed_fraction_mean", "inlier_fraction_mean", "inlier_fraction_min", "correction",
                           "correction_min", "correction_max", "frames_clamped", "values_clamped", "step_rms_before",
                           "step_rms_after"]
    assert (block["version"], block["mode"], block["window_s"], block["radius_frames"], block["stride"]) == (1, "exposure", 60.0, 480, 4)
    assert block["pairs_unmeasured"] == 0 and block["inlier_fraction_min"] >= 0.5 and block["values_clamped"] == 7
    assert block["frames_clamped"] == 0 and 0.5 < block["correction_min"] < 1 < block["correction_max"] < 2
    true = gains[1:] / gains[:-1]
    err = np.abs(np.asarray(block["pair_gain"]) / true - 1).max()
    assert err <= 0.0018, err                                           # measured 0.00171: what the GPU test's bound doubles
    want, _, _ = R.measure(frames, mats)
    assert np.array_equal(np.asarray(block["pair_gain"]), want)
    assert block["step_rms_after"] < 1e-6 < 0.1 < block["step_rms_before"]
    assert g32.dtype == np.float32 and np.array_equal(np.asarray(block["correction"], np.float32), g32)
    # a pair without confidence is neither measured nor chained over
    conf[4] = 0.0
    _, finish = D.solve(request, lambda act: R.pair_gain_hist(frames, mats, act),
                        lambda act, band: R.pair_gain_sums(frames, mats, band, act), conf, len(frames), 16.0)
    block = finish(0)
    assert block["pair_gain"][4] is None and block["pairs_unmeasured"] == 0 and json.loads(json.dumps(block)) == block
    # ... and one with too few well-exposed samples counts as unmeasured
    dark = frames.copy()
    dark[7] = 0.01
    _, finish = D.solve(request, lambda act: R.pair_gain_hist(dark, mats, act),
                        lambda act, band: R.pair_gain_sums(dark, mats, band, act), np.ones(len(mats)), len(frames), 16.0)
    block = finish(0)
    assert block["pairs_unmeasured"] == 2 and block["pair_gain"][6] is None and block["pair_gain"][7] is None
    assert block["correction"][7] == [1.0, 1.0, 1.0]                    # alone in its segment


# ---- the keyword: refusals, their order, defaults ---------------------------------------------------------------------------
@pytest.mark.parametrize("keywords, message", [
    (dict(deflicker=0), "deflicker=0: expected None, False, True or a finite window in seconds in (0, 60]"),
    (dict(deflicker=61.0), "deflicker=61.0: expected None, False, True or a finite window in seconds in (0, 60]"),
    (dict(deflicker=float("nan")), "deflicker=nan: expected None, False, True or a finite window in seconds in (0, 60]"),
    (dict(deflicker="on"), "deflicker='on': expected None, False, True or a finite window in seconds in (0, 60]"),
    (dict(deflicker=True, deflicker_mode=True), "deflicker_mode=True: expected None, 'exposure' or 'rgb'"),
    (dict(deflicker=True, deflicker_mode="luma"), "deflicker_mode='luma': expected None, 'exposure' or 'rgb'"),
    (dict(deflicker_mode="rgb"), "deflicker_mode='rgb' needs deflicker: without a deflicker there are no gains to form."),
    (dict(deflicker=False, deflicker_mode="exposure"),
     "deflicker_mode='exposure' needs deflicker: without a deflicker there are no gains to form."),
    (dict(deflicker=True, estimator="subject", subject_mask=np.zeros((2, 4, 4), np.float32)),
     "deflicker is not supported with estimator 'subject': its transitions register the subject, not the scene, so the pixels "
     "the measurement compares would not show the same scene point."),
    (dict(deflicker=2.0, temporal_fill=2),
     "deflicker with temporal_fill needs fill_exposure=True: a hard fill would paste the uncorrected pixels of neighbouring "
     "frames next to corrected content."),
    (dict(deflicker=2.0, temporal_fill=2, fill_feather=8),
     "deflicker with temporal_fill needs fill_exposure=True: a hard fill would paste the uncorrected pixels of neighbouring "
     "frames next to corrected content."),
    (dict(deflicker=True, sharpness_transfer=2),
     "deflicker is not supported with sharpness_transfer: the samples it blends in are the uncorrected pixels of neighbouring "
     "frames."),
])
def test_every_refusal_is_a_value_error_before_any_gpu_work(pkg, monkeypatch, keywords, message):
    monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    with pytest.raises(ValueError) as caught:
        _call(**keywords)
    assert str(caught.value) == message


@pytest.mark.parametrize("keywords, message", [
    (dict(deflicker=99, mask_grow=999), "mask_grow=999 is not None or an integer in -64..64"),
    (dict(deflicker="on", dynamic_zoom=99.0), "dynamic_zoom=99.0: expected None, True or a finite window in seconds in (0, 60]"),
    (dict(deflicker_mode=3, temporal_fill=99), "temporal_fill=99 outside [0, 32]"),
    (dict(deflicker=True, sharpness_transfer=99), "sharpness_transfer=99 is not 0, None, False or an integer in 1..16"),
    (dict(deflicker=-1, rolling_shutter=7.0),
     "rolling_shutter=7.0: expected None, 0, 'auto' or a finite readout in [-1, 1] (a fraction of the frame interval; negative: "
     "bottom to top)"),
    (dict(deflicker=-1, rolling_refit=True), None),
])
def test_a_call_that_is_also_wrong_in_an_older_way_raises_the_older_message(pkg, monkeypatch, keywords, message):
    monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    with pytest.raises(ValueError) as caught:
        _call(**keywords)
    if message is None:
        assert "rolling_refit" in str(caught.value) and "deflicker" not in str(caught.value)
    else:
        assert str(caught.value) == message


def test_accepted_requests_and_defaults(pkg):
    from vstab_amd import deflicker as D
    from vstab_amd import distributed, flow_pipeline, native

    assert D.check_request(None) is None and D.check_request(False) is None
    assert D.check_request(True) == D.Request(1.0, "exposure") and D.check_request(60, "rgb") == D.Request(60.0, "rgb")
    assert D.check_request(np.float32(0.5), "exposure") == D.Request(0.5, "exposure")
    D.check_pipeline("classic", 2, True, None)                       # the blended, exposure-matched fill composes
    params = inspect.signature(flow_pipeline._stabilize_frames).parameters
    assert list(params).index("deflicker_mode") == list(params).index("deflicker") + 1
    assert all(params[k].default is None and params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("deflicker", "deflicker_mode"))
    fields = list(flow_pipeline.FlowRequest.__dataclass_fields__)
    # among the fields with a default, behind the ones that are given positionally (tests of earlier keywords pin the last one)
    assert fields.index("deflicker") > fields.index("drift_mask") and flow_pipeline.FlowRequest.__dataclass_fields__["deflicker"].default is None
    kw = {k: p.default for k, p in params.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    off = flow_pipeline.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw))
    on = flow_pipeline.check_flow_request("crop", "perspective", "classic", dict(kw, deflicker=True, deflicker_mode="rgb"))
    assert off.deflicker is None and on.deflicker == D.Request(1.0, "rgb")
    assert off.needs_host_plan is False and on.needs_host_plan is False          # it runs behind both plan paths
    assert (D.STRIDE, D.LEVEL_LO, D.LEVEL_HI, D.BINS, D.MIN_COUNT, D.CLAMP) == (4, 2048, 63488, 1024, 256, (0.5, 2.0))
    sharded = inspect.signature(distributed.stabilize_sharded).parameters
    assert sharded["deflicker"].default is None and sharded["deflicker_mode"].default is None
    for name, args in (("pair_gain_hist_batch", ["src", "transitions", "active"]),
                       ("pair_gain_sums_batch", ["src", "transitions", "band", "active"]),
                       ("apply_gain_batch", ["frames", "gains", "mask", "want_count"])):
        assert list(inspect.signature(getattr(native.Context, name)).parameters)[1:] == args
        assert "vstab_" + name in native.EXPORTED_SYMBOLS


@pytest.mark.parametrize("keywords, start", [
    (dict(deflicker=True), "stabilize_sharded does not support deflicker=True: the deflicker is not sharded (a pair may straddle"),
    (dict(deflicker=2.5, deflicker_mode="rgb"), "stabilize_sharded does not support deflicker=2.5:"),
    (dict(deflicker_mode="rgb"), "stabilize_sharded does not support deflicker_mode='rgb':"),
    (dict(deflicker=True, scene_cuts="auto"), "stabilize_sharded does not support scene_cuts:"),
])
def test_stabilize_sharded_refuses_the_keyword(pkg, keywords, start):
    from vstab_amd import distributed

    with pytest.raises(ValueError) as caught:
        distributed.stabilize_sharded(None, None, 12, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0,
                                      **keywords)
    assert str(caught.value).startswith(start)


# ---- header, node, documents ------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entries_and_states_both_rules(pkg):
    from vstab_amd import native

    text = (ROOT / "include" / "vstab.h").read_text()
    flat = re.sub(r"\s+", " ", text)
    for proto in ("int vstab_pair_gain_hist_batch(vstab_ctx* ctx, const float* src, int n, int h, int w, const float* transitions, "
                  "const uint8_t* active, uint32_t* hist, uint32_t* stats);",
                  "int vstab_pair_gain_sums_batch(vstab_ctx* ctx, const float* src, int n, int h, int w, const float* transitions, "
                  "const uint8_t* active, const int32_t* band, uint64_t* sums);",
                  "int vstab_apply_gain_batch(vstab_ctx* ctx, float* frames, const float* mask, int n, int h, int w, "
                  "const float* gains, uint32_t* clamped);"):
        assert proto in flat
    for define in ("#define VSTAB_DEFLICKER_STRIDE 4", "#define VSTAB_DEFLICKER_LO 2048", "#define VSTAB_DEFLICKER_HI 63488"):
        assert define in text
    block = flat[flat.index("---- deflicker"):flat.index("int vstab_pair_gain_hist_batch")]
    for phrase in ("x % S == S/2 && y % S == S/2", "vstab_pair_residual_batch's, literally", "ties to even", "WELL EXPOSED",
                   "min((qb_c * 256) / qa_c, 1023)", "choices, not calibrations", "mask[f, y, x] == 1.0f", "out > 1.0f && v <= 1.0f",
                   'timing kinds "gain_hist" and "gain_sums"', 'Timing kind "apply_gain"', "reads nothing and reports zeros"):
        assert phrase in block, phrase
    assert native.load_library().vstab_abi_version() == 1
    assert "vstab_deflicker.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()


def test_node_sockets_equal_its_execute_parameters_and_where_it_is_listed(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerDeflicker
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_deflicker" and schema.display_name == "Video Stabilizer Deflicker"
    ids = [s.id for s in schema.inputs]
    assert ids == ["frames", "frames_stabilized", "padding_mask", "meta", "window", "mode"]
    assert ids == list(inspect.signature(node.execute).parameters)
    optional = [s.id for s in schema.inputs if getattr(s, "optional", False) or getattr(s, "options", {}).get("optional")]
    assert optional == ["padding_mask", "meta"]        # (ComfyUI's socket has the attribute, the stand-in keeps its options)
    assert [s.id for s in schema.outputs] == ["frames", "meta"]
    listed = asyncio.run(nodes.VideoStabilizerAmdDeflickerExtension().get_node_list())
    before = asyncio.run(nodes.VideoStabilizerAmdRollingRefitExtension().get_node_list())
    assert listed == before + [node] and node not in nodes.NODE_CLASSES
    assert issubclass(nodes.VideoStabilizerAmdDeflickerExtension, nodes.VideoStabilizerAmdRollingRefitExtension)
    entry = asyncio.run(vstab_amd.comfy_entrypoint())                   # unchanged: the node is not handed to ComfyUI
    assert type(entry) is nodes.VideoStabilizerAmdMaskedExtension and node not in asyncio.run(entry.get_node_list())
    # the node's own checks come before any GPU work
    clip = np.zeros((3, 8, 8, 3), np.float32)
    with pytest.raises(ValueError, match="deflicker_mode='luma'"):
        node.execute(clip, clip, None, None, 1.0, "luma")
    with pytest.raises(ValueError, match="as many stabilized as original"):
        node.execute(clip, clip[:2], None, None, 1.0, "rgb")
    with pytest.raises(ValueError, match="stabilization_warp"):
        node.execute(clip, clip, None, {"frames": 3}, 1.0, "rgb")


def test_documents_name_the_feature():
    for name, words in (("README.md", ("deflicker=", "deflicker_mode", "Video Stabilizer Deflicker", "profiles/r27_deflicker.md")),
                        ("DESIGN.md", ("six passes", "vstab_deflicker.hip", "high-pass")),
                        ("INTEGRATION.md", ("vstab_pair_gain_hist_batch", "vstab_pair_gain_sums_batch", "vstab_apply_gain_batch",
                                            "VideoStabilizerAmdDeflickerExtension"))):
        text = (ROOT / name).read_text()
        for word in words:
            assert word in text, (name, word)
