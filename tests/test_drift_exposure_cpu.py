"""CPU: the exposure-matched, masked keyframe alignment (`drift_exposure`, `drift_mask`) without a GPU.

  1. the NumPy restatement of the second form of the rule (tests/drift_exposure_restatement.py): at G = 1024, O = 0 and without
     a mask its 31 numbers, mapped onto the 17 of the first form, equal tests/drift_restatement.py exactly; the mask by hand
  2. solve_update_ex on sums of a smooth pair with a known shift, gain and offset
  3. refine_ex driven by the restatement: the bootstrap launch, the integer state, the "gain" reason at the clamps
  4. every new ValueError and its place in the order; the request object with the options off; node, header, documents
"""

import inspect
from pathlib import Path

import numpy as np
import pytest

from tests import drift_exposure_restatement as RX
from tests import drift_restatement as R
from tests.util import shake_path

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def dc(pkg):
    from vstab_amd import drift_correction

    return drift_correction


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
def _mats(h, w):
    c, s = 1.003 * np.cos(0.01), 1.003 * np.sin(0.01)
    return np.array([[1, 0, 0, 0, 1, 0], [1, 0, 1 / 64, 0, 1, 1 / 64], [1, 0, w / 2, 0, 1, 0], [1, np.nan, 0, 0, 1, 0],
                     [c, -s, 0.37, s, c, -0.81], [1, 0, -0.7, 0, 1, 0.6]], np.float64)


@pytest.mark.parametrize("h,w", [(3, 3), (5, 7), (33, 64), (37, 53), (2, 9)])
def test_the_plain_rule_is_the_second_form_at_unit_gain(dc, h, w):
    rng = np.random.default_rng(h * 100 + w)
    mats = _mats(h, w)
    n = len(mats)
    gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    gray[1::2] = np.roll(gray[0], 1, axis=1)
    anchor = np.array([n - 1, 1, -1, 0, 0, 2])
    assert RX.SLOTS == 31 == dc.SLOTS_EX and RX.OLD_SLOTS == dc.PLAIN_SLOTS and len(set(RX.OLD_SLOTS)) == 17
    for cap in (0, 32, 255):
        want = R.anchor_sums_batch(gray, anchor, mats, cap)
        got = RX.anchor_sums_ex_batch(gray, anchor, mats, cap)
        assert got.shape == (n, 31) and np.array_equal(got[:, RX.OLD_SLOTS], want)
        assert not got[:, 2].any()                                             # nothing is masked
        # the two new columns by their meaning: H55 = count, H45 = sum T, H05 / H15 = sum gx / gy
        assert np.array_equal(got[:, RX.H_INDEX[(5, 5)]], got[:, 0])
        empty = np.zeros((n, -(-h // 8), -(-w // 8)), np.uint8)
        assert np.array_equal(RX.anchor_sums_ex_batch(gray, anchor, mats, cap, blocked=empty), got)


def test_the_mask_by_hand():
    """24 x 24 at step 8: a 3 x 3 grid with samples at (0, 0), (8, 0), (16, 0), (0, 8), ...  Blocking sample (1, 1) = pixel
    (8, 8) in the ANCHOR masks the template pixels nearest to it, x in 4..11 and y in 4..11 (64 pixels); blocking it in the
    FRAME under a shift of +3 px in x masks the template pixels whose sample lands there, x in 1..8 (x + 3 in 4..11)."""
    rng = np.random.default_rng(5)
    gray = rng.integers(0, 256, (2, 24, 24), dtype=np.uint8)
    eye = np.array([[1.0, 0, 0, 0, 1, 0]] * 2)
    blocked = np.zeros((2, 3, 3), np.uint8)
    blocked[0, 1, 1] = 1
    got = RX.anchor_sums_ex_batch(gray, [-1, 0], eye, 255, blocked=blocked)
    inside = 22 * 22
    assert got[1, :3].tolist() == [inside - 64, 0, 64] and not got[0].any()
    blocked[:] = 0
    blocked[1, 1, 1] = 9                                                      # any non-zero byte blocks
    shift = np.array([[1.0, 0, 0, 0, 1, 0], [1.0, 0, 3.0, 0, 1, 0]])
    got = RX.anchor_sums_ex_batch(gray, [-1, 0], shift, 255, blocked=blocked)
    inside = 22 * 20                                                          # x + 3 <= 23: x in 1..20
    assert got[1, :3].tolist() == [inside - 8 * 8, 0, 64]
    full = np.ones((2, 3, 3), np.uint8)
    got = RX.anchor_sums_ex_batch(gray, [-1, 0], shift, 32, blocked=full)
    assert got[1, 2] == inside and not np.delete(got[1], 2).any()             # a masked pixel adds to `masked` and nothing else
    # the gh-1 clamp: on 16 rows the grid has two, and rows 12..14 round to a third that does not exist -- they read row 1
    low = np.zeros((2, 2, 3), np.uint8)
    low[0, 1, 1] = 1
    got = RX.anchor_sums_ex_batch(gray[:, :16], [-1, 0], eye, 255, blocked=low)
    assert got[1, :3].tolist() == [14 * 22 - 11 * 8, 0, 11 * 8]               # y in 4..14, x in 4..11
    # the gain and the offset enter r alone: r = v - (G T + O)
    flat = np.stack([np.full((8, 8), 100, np.uint8), np.full((8, 8), 91, np.uint8)])
    got = RX.anchor_sums_ex_batch(flat, [-1, 0], eye, 0, gain=[1024, 870], offset=[0, 6184])
    assert got[1, 0] == 36 and got[1, 3] == 0 and got[1, 1] == 0              # 91 * 1024 == 870 * 100 + 6184 exactly
    got = RX.anchor_sums_ex_batch(flat, [-1, 0], eye, 0, gain=[1024, 870], offset=[0, 6185])
    assert got[1, 0] == 0 and got[1, 1] == 36                                 # one unit off: every pixel is over a cap of 0


# ---- 2. the solve ------------------------------------------------------------------------------------------------------------
def _smooth(h, w, dx=0.0, dy=0.0):
    """a smooth texture, analytic so that it can be sampled at any shift; about 40..215 grey levels"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    return 128 + 45 * np.sin(x / 7.0) * np.cos(y / 9.0) + 40 * np.sin((x + 2 * y) / 11.0 + 1.0)


BILINEAR_LOSS = (1 / 49 + 1 / 81) / 8      # of sin(x / 7) cos(y / 9); the other component, (1 / 121 + 4 / 121) / 8, loses less


@pytest.mark.parametrize("mode", ["similarity", "translation"])
def test_solve_update_recovers_shift_gain_and_offset(dc, mode):
    """I = 0.85 T(p - s) + 6 with s = (0.4, -0.3) px, both images rounded to u8.  Gauss-Newton with solve_update_ex on the
    restatement's sums, the integer state as refine_ex keeps it, from the identity at G = 1024, O = 0, must recover all three.
    Nothing is fitted in the gates: the shift at the project's CPU recovery bound of 0.03 px.  The gain at 2 / 1024 (one unit
    of G's quantisation, one for the u8 rounding of two images of ~170 levels of range) plus what bilinear sampling takes from
    the contrast: between two pixels at fraction f a wave of wavenumber k loses f (1 - f) k^2 / 2 of its amplitude, at most
    (kx^2 + ky^2) / 8 = BILINEAR_LOSS for the texture's sharpest component, and the alignment sees that as gain.  The offset at
    the gain's bound times the template's mean (128: a gain error moves the offset through the mean) plus 0.05 grey level."""
    h, w = 64, 96
    T = np.rint(_smooth(h, w)).astype(np.uint8)
    I = np.rint(0.85 * _smooth(h, w, 0.4, -0.3) + 6.0).astype(np.uint8)
    gray = np.stack([T, I])
    Rm = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    G, O = 1024, 0
    for it in range(5):
        sums = RX.anchor_sums_ex(T, I, Rm.reshape(6), 255 if it == 0 else dc.RESIDUAL_CAP, G, O)
        d, dG, dO = dc.solve_update_ex(sums, mode, G, True)
        G, O = int(np.rint(G + dG)), int(np.rint(O + dO))
        Rm = (dc._affine3(dc.sampled_at(Rm, (w, h))) @ np.linalg.inv(dc.warp_matrix(d, (w, h))))[:2]
    centre = Rm @ np.array([(w - 1) / 2, (h - 1) / 2, 1.0]) - np.array([(w - 1) / 2, (h - 1) / 2])
    corner = dc.corner_distance(Rm, np.array([[1.0, 0, 0.4], [0, 1.0, -0.3]]), (w, h))
    print({"mode": mode, "shift": centre.round(4).tolist(), "corner_error": round(corner, 4), "gain": G / 1024, "offset": O / 1024})
    assert gray.dtype == np.uint8 and corner <= 0.03, corner
    gain_bound = 2 / 1024 + 0.85 * BILINEAR_LOSS
    assert abs(G / 1024 - 0.85) <= gain_bound and abs(O / 1024 - 6.0) <= 128 * gain_bound + 0.05
    # without exposure matching the same call solves today's system from the new slots, bit for bit
    plain = R.anchor_sums(T, I, np.array([1.0, 0, 0, 0, 1, 0]), 32)
    ex = RX.anchor_sums_ex(T, I, np.array([1.0, 0, 0, 0, 1, 0]), 32)
    d_old, (d_new, dG, dO) = dc.solve_update(plain, mode), dc.solve_update_ex(ex, mode, 1024, False)
    assert np.array_equal(d_old, d_new) and dG == 0.0 and dO == 0.0
    # a flat template has no gradient and no contrast: singular in both forms
    flat = RX.anchor_sums_ex(np.full((h, w), 90, np.uint8), I, np.array([1.0, 0, 0, 0, 1, 0]), 255)
    assert dc.solve_update_ex(flat, mode, 1024, True) is None and dc.solve_update_ex(flat, mode, 1024, False) is None


# ---- 3. the refinement -------------------------------------------------------------------------------------------------------
W, H, N = 96, 64, 6
GAINS = np.array([1.0, 0.9, 0.8, 1.1, 0.4, 0.95])        # frame 4 lies outside the [0.5, 2] clamp


@pytest.fixture(scope="module")
def clip():
    """6 frames of 96 x 64: the smooth texture under a small similarity path, frame i at gain GAINS[i] and offset i grey levels"""
    cam = shake_path(N, W, H, "similarity", seed=2, amp=0.3)
    truth = np.stack([cam[i] @ np.linalg.inv(cam[0]) for i in range(N)])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gray = []
    for i in range(N):
        inv = np.linalg.inv(truth[i])                     # frame pixel -> anchor pixel
        ax, ay = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2], inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
        img = 128 + 45 * np.sin(ax / 7.0) * np.cos(ay / 9.0) + 40 * np.sin((ax + 2 * ay) / 11.0 + 1.0)
        gray.append(np.rint(GAINS[i] * img + i).astype(np.uint8))
    return truth, np.stack(gray)


def _sums_ex_fn(gray, blocked=None, calls=None):
    def fn(anchor, mats, gain, offset, cap):
        if calls is not None:
            calls.append((np.array(anchor), np.array(gain), np.array(offset), cap, np.array(mats)))
        return RX.anchor_sums_ex_batch(gray, anchor, mats, cap, gain, offset, blocked, 8)
    return fn


def test_refine_ex_bootstrap_integer_state_and_the_gain_reason(dc, clip):
    truth, gray = clip
    off = np.array([[1.0, 0, 0.4], [0, 1.0, -0.3], [0, 0, 1.0]])
    start = np.stack([truth[0]] + [off @ truth[i] for i in range(1, N)])
    work = np.stack([start[k + 1] @ np.linalg.inv(start[k]) for k in range(N - 1)])
    sched = dc.schedule(N, None, [0.9] * (N - 1), 32)
    calls = []
    got = dc.refine_ex(_sums_ex_fn(gray, calls=calls), work, sched, "similarity", (W, H), True)
    err = [dc.corner_distance(got.R[i], truth[i][:2], (W, H)) for i in range(N)]
    print({"reason": got.reason, "gain": (got.gain / 1024).round(4).tolist(), "offset": (got.offset / 1024).round(3).tolist(),
           "corner_error": np.round(err, 4).tolist(), "launches": got.launches})
    assert got.reason == ["no_anchor", None, None, None, "gain", None]
    # the bootstrap: the first launch is uncapped, at G = 1024 / O = 0, and every anchored frame is still there for the
    # second, which is the launch the cost test starts from; every later launch runs under the cap
    assert [c[3] for c in calls] == [dc.BOOTSTRAP_CAP] + [dc.RESIDUAL_CAP] * (len(calls) - 1) and len(calls) == got.launches >= 3
    assert np.all(calls[0][1] == 1024) and not calls[0][2].any()
    assert calls[0][0].tolist() == [-1, 0, 0, 0, 0, 0] and calls[1][0].tolist() == [-1, 0, 0, 0, -1, 0]
    assert got.before_launch == 2 and calls[-1][0].tolist() == [-1, 0, 0, 0, -1, 0]
    # ... and only its gain and offset are taken: the second launch is at the chained matrices still, the third is not
    assert np.array_equal(calls[1][4], got.R_chained.reshape(N, 6)) and not np.array_equal(calls[2][4], calls[1][4])
    assert not np.array_equal(calls[1][1], calls[0][1])
    # the integer state: what the kernel is given are integers in the kernel's range, and the last launch saw the reported ones
    for _, g, o, _, _ in calls:
        assert g.dtype.kind == "i" and o.dtype.kind == "i" and g.min() >= 256 and g.max() <= 4096
    assert got.gain.dtype == np.int64 and got.offset.dtype == np.int64
    refined = [1, 2, 3, 5]
    assert np.array_equal(calls[-1][1][refined], got.gain[refined]) and np.array_equal(calls[-1][2][refined], got.offset[refined])
    assert got.gain[0] == 1024 and got.gain[4] == 1024 and got.offset[4] == 0 and np.array_equal(got.R[4], got.R_chained[4])
    for i in refined:
        assert abs(got.gain[i] / 1024 - GAINS[i]) <= 2 / 1024 + GAINS[i] * BILINEAR_LOSS, (i, got.gain[i])   # (the solve test's bound)
        assert err[i] <= 0.03, (i, err[i])
    assert got.sums_first.shape == (N, 17) and got.sums_final.shape == (N, 17) and not got.masked_first.any()
    # without exposure matching the same clip is kept by the guards or mis-registered: the cap and the cost test see the step
    plain = dc.refine_ex(_sums_ex_fn(gray), work, sched, "similarity", (W, H), False)
    assert plain.before_launch == 1 and np.all(plain.gain == 1024) and "gain" not in plain.reason


def test_refine_ex_with_the_mask_alone_is_refine_on_an_empty_grid(dc, clip):
    truth, gray = clip
    same = np.stack([gray[0]] + [np.rint((gray[i].astype(np.float64) - i) / GAINS[i]).astype(np.uint8) for i in range(1, N)])
    work = np.stack([truth[k + 1] @ np.linalg.inv(truth[k]) for k in range(N - 1)])
    sched = dc.schedule(N, None, [0.9] * (N - 1), 32)
    want = dc.refine(lambda a, m: R.anchor_sums_batch(same, a, m, dc.RESIDUAL_CAP), work, sched, "similarity", (W, H))
    empty = np.zeros((N, H // 8, W // 8), np.uint8)
    got = dc.refine_ex(_sums_ex_fn(same, empty), work, sched, "similarity", (W, H), False)
    assert got.reason == want.reason and np.array_equal(got.R, want.R) and got.launches == want.launches
    assert np.array_equal(got.sums_first, want.sums_first) and np.array_equal(got.sums_final, want.sums_final)
    # a grid that blocks the left half: those pixels are counted as masked, and meta reports the fraction
    left = empty.copy()
    left[:, :, :4] = 1
    got = dc.refine_ex(_sums_ex_fn(same, left), work, sched, "similarity", (W, H), False)
    block = dc.meta_block_ex(sched, got, False, True)
    assert 0.25 < block["masked_fraction_mean"] < 0.45 and "exposure" not in block
    assert list(block["frames_kept"]) == ["singular", "overlap", "cost", "step", "no_anchor", "gain"]


def test_meta_block_ex(dc, clip):
    truth, gray = clip
    work = np.stack([truth[k + 1] @ np.linalg.inv(truth[k]) for k in range(N - 1)])
    sched = dc.schedule(N, None, [0.9] * (N - 1), 32)
    got = dc.refine_ex(_sums_ex_fn(gray), work, sched, "similarity", (W, H), True)
    block = dc.meta_block_ex(sched, got, True, False)
    ex = block["exposure"]
    assert list(block) == ["frames_kept", "exposure"] and block["frames_kept"]["gain"] == 1
    assert list(ex) == ["matched", "gain", "offset", "gain_min", "gain_max", "residual_before_launch"] and ex["matched"] is True
    assert ex["gain"][0] == 1.0 and ex["gain"][4] == 1.0 and ex["offset"][4] == 0.0 and ex["residual_before_launch"] == 2
    assert ex["gain_min"] == min(ex["gain"]) and ex["gain_max"] == max(ex["gain"]) and len(ex["gain"]) == len(ex["offset"]) == N
    assert dc.KEEP_REASONS == ("singular", "overlap", "cost", "step", "no_anchor")           # today's tuple is today's
    assert (dc.GAIN_MIN, dc.GAIN_MAX, dc.MAX_OFFSET_LEVELS, dc.BOOTSTRAP_CAP) == (512, 2048, 64, 255)


# ---- 4. requests, node, header -----------------------------------------------------------------------------------------------
class NoClip:
    frames = None


ARGS = ("crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0)
M = np.zeros((4, 4), np.float32)
M3 = np.zeros((2, 4, 4), np.float32)
TODAY = ("drift_correction does not support estimation_mask: the keyframe alignment has no per-pixel exclusion yet (its residual "
         "cap is the only guard against moving subjects).")

REFUSALS = [
    ("similarity", dict(drift_correction=8, drift_exposure="yes"), "drift_exposure='yes': expected None / False (off) or True."),
    ("similarity", dict(drift_correction=8, drift_exposure=1), "drift_exposure=1: expected None / False (off) or True."),
    ("similarity", dict(drift_correction=8, estimation_mask=M, drift_mask=1.0), TODAY),     # not True: the mask is still refused
    ("similarity", dict(drift_correction=8, drift_mask=2), "drift_mask=2: expected None / False (off) or True."),
    ("similarity", dict(drift_exposure=True), "drift_exposure=True needs drift_correction: it changes how the keyframe alignment is solved, and without drift_correction there is none."),
    ("similarity", dict(drift_correction=0, drift_mask=True, estimation_mask=M), "drift_mask=True needs drift_correction: it changes how the keyframe alignment is solved, and without drift_correction there is none."),
    ("similarity", dict(drift_correction=8, drift_mask=True), "drift_mask=True needs estimation_mask: the keyframe alignment leaves out the pixels that mask's block grid names, and without estimation_mask there is no grid."),
    # today's refusals stand, the options do not lift them (drift_mask=True lifts the mask's alone)
    ("similarity", dict(drift_correction=8, estimation_mask=M), TODAY),
    ("similarity", dict(drift_correction=8, estimation_mask=M, drift_exposure=True), TODAY),
    ("similarity", dict(drift_correction=8, estimation_mask=M, drift_mask=False), TODAY),
    ("perspective", dict(drift_correction=True, drift_exposure=True), "drift_correction does not support transform_mode='perspective': the keyframe alignment updates a similarity (shift, zoom, rotation); use 'translation' or 'similarity'."),
    ("similarity", dict(drift_correction=8, estimator="subject", subject_mask=M3, drift_exposure=True), "drift_correction does not support estimator='subject': its transitions follow the subject, while the estimation images the keyframe alignment reads show the background."),
    # behind the drift check: a wrong drift_correction, or a pipeline it refuses, wins over a wrong option
    ("similarity", dict(drift_correction=1.5, drift_exposure="yes"), "drift_correction=1.5: expected None / False / 0 (off), True (a keyframe every 32 frames) or an int in 2..4096, the keyframe spacing."),
    ("perspective", dict(drift_correction=True, drift_exposure="yes"), "drift_correction does not support transform_mode='perspective': the keyframe alignment updates a similarity (shift, zoom, rotation); use 'translation' or 'similarity'."),
    # and every older check wins over both
    ("similarity", dict(drift_exposure="yes", rolling_shutter=7.0), None),
    ("similarity", dict(drift_mask=True, mask_tapered=False), None),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_and_its_place(pkg, monkeypatch, case):
    from vstab_amd import flow_pipeline

    monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    mode, keywords, message = REFUSALS[case]
    with pytest.raises(ValueError) as caught:
        flow_pipeline._stabilize_frames(NoClip(), "crop_and_pad", mode, *ARGS[2:], **keywords)
    if message is None:
        assert "drift_" not in str(caught.value), str(caught.value)
    else:
        assert str(caught.value) == message


def test_the_request_with_the_options_off_is_todays(pkg):
    from vstab_amd import flow_pipeline as fp

    params = inspect.signature(fp._stabilize_frames).parameters
    for name in ("drift_exposure", "drift_mask"):
        assert params[name].default is None and params[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(params)[-3:] == ["drift_correction", "drift_exposure", "drift_mask"]
    kw = {name: prm.default for name, prm in params.items() if prm.kind is inspect.Parameter.KEYWORD_ONLY}
    today = {k: v for k, v in kw.items() if k not in ("drift_exposure", "drift_mask")}
    for drift in (None, True, 5):
        want = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(today, drift_correction=drift))
        # the object a call of today's tree builds: the fifteen fields, positionally
        fields = [getattr(want, f) for f in list(fp.FlowRequest.__dataclass_fields__)[:15]]
        assert want == fp.FlowRequest(*fields) and want.drift_exposure is False and want.drift_mask is False
        for off in (None, False):
            got = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, drift_correction=drift, drift_exposure=off, drift_mask=off))
            assert got == want and got.kept_by_products == want.kept_by_products and got.needs_host_plan == want.needs_host_plan
    on = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, drift_correction=4, drift_exposure=True))
    assert (on.drift, on.drift_exposure, on.drift_mask) == (4, True, False) and on.kept_by_products == ("gray_out",)
    both = fp.check_flow_request("crop_and_pad", "translation", "flow", dict(kw, drift_correction=True, drift_exposure=True, drift_mask=True, estimation_mask=M))
    assert (both.drift, both.drift_exposure, both.drift_mask, both.mask_margin) == (32, True, True, 16)


def test_sharded_refusals(pkg):
    from vstab_amd import distributed

    call = (None, None, 12, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
    for name in ("drift_exposure", "drift_mask"):
        with pytest.raises(ValueError) as caught:
            distributed.stabilize_sharded(*call, **{name: True})
        assert str(caught.value) == (f"stabilize_sharded does not support {name}=True: the keyframe alignment it belongs to is not "
                                     "sharded; run the single-GPU pipeline for it")
        with pytest.raises(ValueError, match="does not support drift_correction=16"):       # the older refusal wins
            distributed.stabilize_sharded(*call, drift_correction=16, **{name: True})
        for off in (None, False):
            with pytest.raises(ValueError, match="does not support scene_cuts"):
                distributed.stabilize_sharded(*call, scene_cuts="auto", **{name: off})
        assert inspect.signature(distributed.stabilize_sharded).parameters[name].default is None


def test_node_schema(pkg):
    import asyncio

    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerFlowAnchoredExposure
    s, base = node.define_schema(), nodes.VideoStabilizerFlowAnchored.define_schema()
    assert s.node_id == "video_stabilizer_flow_anchored_exposure"
    assert s.display_name == "Video Stabilizer Flow (Drift-Free, Exposure-Matched)"
    assert [i.id for i in s.inputs] == [i.id for i in base.inputs] + ["match_exposure", "exclude_mask", "mask_margin"]
    assert [o.id for o in s.outputs] == [o.id for o in base.outputs]
    by_id = {i.id: i for i in s.inputs}
    assert by_id["match_exposure"].kind.upper() == "BOOLEAN" and by_id["match_exposure"].options["default"] is True
    assert by_id["exclude_mask"].kind.upper() == "MASK" and by_id["exclude_mask"].options["optional"] is True and "optional" not in by_id["mask_margin"].options
    assert list(inspect.signature(node.execute).parameters)[-4:] == ["keyframe_spacing", "match_exposure", "exclude_mask", "mask_margin"]
    assert node not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    listed = asyncio.run(nodes.VideoStabilizerAmdAnchorExposureExtension().get_node_list())
    before = asyncio.run(nodes.VideoStabilizerAmdAnchorExtension().get_node_list())
    assert listed == before + [node] and node not in before
    assert node not in asyncio.run(asyncio.run(vstab_amd.comfy_entrypoint()).get_node_list())


def test_header_binding_and_documents_agree(pkg):
    from vstab_amd import native

    text = (ROOT / "include" / "vstab.h").read_text()
    assert ("int vstab_anchor_sums_ex_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const int32_t* anchor,\n"
            "                               const double* R, const int32_t* gain, const int32_t* offset, int cap, const uint8_t* blocked,\n"
            "                               int step, int gh, int gw, int64_t* out);") in text
    assert "#define VSTAB_ANCHOR_EX_SLOTS 31" in text and "#define VSTAB_ANCHOR_SLOTS 17" in text
    assert text.count("---- Drift correction") == 1                        # the rule lives in one section
    for words in ("r = v - (G T[y,x] + O)", "mask_margin < step / 2", "does not cover every subject pixel", "J4 = T[y,x]", "J5 = 1",
                  "no sum reaches 2^59", 'timing kind "anchor_ex"'):
        assert words in text, words
    assert "vstab_anchor_sums_ex_batch" in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), "vstab_anchor_sums_ex_batch")
    assert list(inspect.signature(native.Context.anchor_sums_ex_batch).parameters)[1:] == ["gray", "anchor", "R", "cap", "gain", "offset", "blocked", "step"]
    for doc, words in (("INTEGRATION.md", ("vstab_anchor_sums_ex_batch", "VideoStabilizerAmdAnchorExposureExtension")),
                       ("README.md", ("drift_exposure", "drift_mask", "Exposure-Matched")),
                       ("DESIGN.md", ("vstab_anchor_sums_ex_batch", "drift_exposure"))):
        body = (ROOT / doc).read_text()
        for word in words:
            assert word in body, (doc, word)
