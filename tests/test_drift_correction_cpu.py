"""Drift correction without a GPU: the host arithmetic of drift_correction.py driven by the NumPy restatement of the kernel's
rule (tests/drift_restatement.py), the schedule, the path parameters, the keep reasons, the requests and the node.

  1. the restatement itself on cases small enough to do by hand
  2. schedule: spacing larger than the clip, shots of one and two frames, a confidence-0 pair at a keyframe and next to one
  3. path_params: params_to_matrix(-path_params(C)) = C^-1; the written float32 transitions chain back to the poses
  4. recovery: a 0.95 px initial error comes back within 0.03 px of the analytic truth, in both modes
  5. every keep reason, provoked once
  6. requests: every refusal and its message, the new checks lose to every older one, the plan hook, the node, the header
"""

import inspect
from pathlib import Path

import numpy as np
import pytest

from tests import drift_restatement as R
from tests.util import shake_path, similarity

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def dc(pkg):
    from vstab_amd import drift_correction

    return drift_correction


def _gray(frames):
    """float RGB [n,h,w,3] in 0..1 -> u8 [n,h,w] (any fixed luma will do here: both images of a pair go through it)."""
    f = np.asarray(frames, dtype=np.float64)
    return np.floor(255.0 * (0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2])).astype(np.uint8)


def _sums_fn(gray, cap=32, calls=None):
    def fn(anchor, mats):
        if calls is not None:
            calls.append(np.array(anchor))
        return R.anchor_sums_batch(gray, anchor, mats, cap)
    return fn


def _corner_error(got, want, size):
    w, h = size
    c = np.array([[0, 0, 1.0], [w - 1, 0, 1.0], [0, h - 1, 1.0], [w - 1, h - 1, 1.0]]).T
    return float(np.max(np.hypot(*(np.asarray(got)[:2] @ c - np.asarray(want)[:2] @ c))))


# ---- 1. the restatement by hand ----------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 6), dtype=np.uint8)
    eye = [1, 0, 0, 0, 1, 0]
    s = R.anchor_sums(img, img, eye, 255)
    assert s[0] == 3 * 4 and s[1] == 0 and s[2] == 0 and np.all(s[3:7] == 0)
    gx = img[1:4, 2:6].astype(int) - img[1:4, 0:4].astype(int)
    gy = img[2:5, 1:5].astype(int) - img[0:3, 1:5].astype(int)
    assert s[7] == (gx * gx).sum() and s[8] == (gx * gy).sum() and s[11] == (gy * gy).sum()
    # one pixel of a 3x3 image: u = q = 0, so J2 = J3 = 0
    t = np.array([[0, 10, 0], [20, 50, 26], [0, 14, 0]], np.uint8)
    i = t.copy()
    i[1, 1] = 53
    s = R.anchor_sums(t, i, eye, 255)
    assert s.tolist() == [1, 0, 3 * 1024, 6 * 3 * 1024, 4 * 3 * 1024, 0, 0, 36, 24, 0, 0, 16, 0, 0, 0, 0, 0]
    # the cap: |r| == 1024 cap counts, one more does not
    assert R.anchor_sums(t, i, eye, 3)[:3].tolist() == [1, 0, 3072] and R.anchor_sums(t, i, eye, 2)[:3].tolist() == [0, 1, 0]
    # a Q5 tie rounds to even: x + 1/64 -> 32 x + 0.5 -> the even neighbour, so fx alternates between 0 and 1
    s = R.anchor_sums(t, t, [1, 0, 1 / 64, 0, 1, 0], 255)
    assert s[0] == 1 and s[2] == abs(32 * 32 * 50 - 1024 * 50)            # x = 1: rint(32.5) = 32, no shift
    # outside, NaN, inf, too small
    for bad in ([1, 0, 5, 0, 1, 0], [np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0]):
        assert not R.anchor_sums(t, t, bad, 255).any()
    assert not R.anchor_sums(np.zeros((2, 9), np.uint8), np.zeros((2, 9), np.uint8), eye, 255).any()
    batch = R.anchor_sums_batch(np.stack([t, i]), [-1, 0], [eye, eye], 255)
    assert not batch[0].any() and batch[1].tolist() == R.anchor_sums(t, i, eye, 255).tolist()


# ---- 2. schedule ---------------------------------------------------------------------------------------------------------------
def test_schedule(dc):
    s = dc.schedule(5, None, [0.9] * 4, 32)                                # spacing larger than the clip
    assert s.anchor.tolist() == [-1, 0, 0, 0, 0] and s.keyframes == [0] and s.shot_start.tolist() == [True, False, False, False, False]
    s = dc.schedule(9, None, [0.9] * 8, 3)
    assert s.anchor.tolist() == [-1, 0, 0, 0, 3, 3, 3, 6, 6] and s.keyframes == [0, 3, 6]
    # shots of one and two frames
    s = dc.schedule(7, [(0, 1), (1, 3), (3, 7)], [0.0, 0.8, 0.0, 0.8, 0.8, 0.8], 2)
    assert s.anchor.tolist() == [-1, -1, 1, -1, 3, 3, 5] and s.keyframes == [0, 1, 3, 5]
    assert s.shot_start.tolist() == [True, True, False, True, False, False, False]
    # a confidence-0 pair AT a keyframe (pair 3: frames 3 -> 4 with S = 4) and NEXT to one (pair 4)
    s = dc.schedule(10, None, [0.9, 0.9, 0.9, 0.0, 0.9, 0.9, 0.9, 0.9, 0.9], 4)
    assert s.anchor.tolist() == [-1, 0, 0, 0, -1, 4, 4, 4, 4, 8] and s.keyframes == [0, 4, 8]
    s = dc.schedule(10, None, [0.9, 0.9, 0.9, 0.9, 0.0, 0.9, 0.9, 0.9, 0.9], 4)
    assert s.anchor.tolist() == [-1, 0, 0, 0, 0, -1, 5, 5, 5, 5] and s.keyframes == [0, 4, 5, 9]
    assert s.shot_start.tolist() == [True] + [False] * 9                   # a lost pair is not a new shot
    with pytest.raises(ValueError, match="confidences"):
        dc.schedule(4, None, [0.9], 2)


def test_poses_restart_per_shot_and_continue_across_a_lost_pair(dc):
    sched = dc.schedule(6, [(0, 3), (3, 6)], [0.9, 0.9, 0.0, 0.9, 0.0], 2)
    assert sched.anchor.tolist() == [-1, 0, 0, -1, 3, -1]
    mats = np.tile(np.eye(3), (5, 1, 1))
    mats[:, 0, 2] = [1.0, 2.0, 50.0, 4.0, 8.0]
    C = dc.poses(dc.chained(mats, sched), sched)
    assert C[:, 0, 2].tolist() == [0.0, 1.0, 3.0, 0.0, 4.0, 4.0]           # shot 2 starts at 0; frame 5 continues as under I
    A = dc.transitions(C)
    assert np.allclose(A[:, 0, 2], [1.0, 2.0, -3.0, 4.0, 0.0])


# ---- 3. path parameters --------------------------------------------------------------------------------------------------------
def test_path_params_negate_to_the_inverse(dc, pkg):
    from vstab_amd import host_math as hm

    rng = np.random.default_rng(7)
    for _ in range(100):
        C = similarity(rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(-0.5, 0.5), np.exp(rng.uniform(-0.3, 0.3)),
                       rng.uniform(0, 900), rng.uniform(0, 500)).astype(np.float64)
        p = dc.path_params(C[None], "similarity")[0]
        ct, st, s = np.cos(-p[2]), np.sin(-p[2]), np.exp(-p[3])
        inv = np.array([[s * ct, -s * st, -p[0]], [s * st, s * ct, -p[1]], [0, 0, 1.0]])   # _params_to_matrix in float64
        assert np.abs(inv - np.linalg.inv(C)).max() < 1e-9
        assert np.abs(hm._params_to_matrix(-p, "similarity") - np.linalg.inv(C)).max() < 1e-4  # (its own float32 cast)
        T = np.eye(3)
        T[:2, 2] = C[:2, 2]
        assert np.array_equal(dc.path_params(T[None], "translation")[0], C[:2, 2])
    with pytest.raises(ValueError, match="perspective"):
        dc.path_params(np.eye(3)[None], "perspective")


def test_poses_rescale_to_full_resolution_as_the_transitions_do(dc, pkg):
    """1080p is estimated at 960x540: rescale_to_full is host_math.rescale_transforms_to_full without its float32 cast, the
    path parameters of the rescaled pose negate to its inverse, and the path's steps telescope to it."""
    from vstab_amd import host_math as hm

    size, work = (1920, 1080), (960, 540)
    n = 40
    cam = shake_path(n, work[0], work[1], "similarity", seed=5, amp=1.0)
    C = np.stack([cam[i] @ np.linalg.inv(cam[0]) for i in range(n)])
    full = dc.rescale_to_full(C, size, work)
    assert full.dtype == np.float64 and np.array_equal(full.astype(np.float32), hm.rescale_transforms_to_full(C, size, work))
    assert np.allclose(full[:, :2, 2], 2.0 * C[:, :2, 2], rtol=1e-15, atol=0) and np.allclose(full[:, :2, :2], C[:, :2, :2], rtol=1e-15, atol=0)
    assert np.array_equal(dc.rescale_to_full(C, (960, 540), None), C)
    # an anisotropic working size, as 1000x777 -> 960x746 gives
    odd = dc.rescale_to_full(C, (1000, 777), (960, 746))
    assert np.array_equal(odd.astype(np.float32), hm.rescale_transforms_to_full(C, (1000, 777), (960, 746)))
    p = dc.path_params(full, "similarity")
    for i in range(n):
        ct, st, s = np.cos(-p[i, 2]), np.sin(-p[i, 2]), np.exp(-p[i, 3])
        inv = np.array([[s * ct, -s * st, -p[i, 0]], [s * st, s * ct, -p[i, 1]], [0, 0, 1.0]])
        assert np.abs(inv @ full[i] - np.eye(3)).max() < 1e-9
    d = dc.path_deltas(full, "similarity")
    assert d.shape == (n - 1, 4) and np.abs(np.cumsum(d, axis=0) - p[1:]).max() < 1e-9 and not p[0].any()


def test_written_float32_transitions_chain_back_to_the_poses(dc, pkg):
    from vstab_amd import native

    n = 256
    cam = shake_path(n, 960, 540, "similarity", seed=11, amp=1.0)
    C = np.stack([cam[i] @ np.linalg.inv(cam[0]) for i in range(n)])
    sched = dc.schedule(n, None, [0.9] * (n - 1), 32)
    table = np.zeros((n - 1, 3), native.FIT_DTYPE)
    table["matrix"][:] = np.eye(3, dtype=np.float32).reshape(9)
    table["computed"][:, 1] = table["accepted"][:, 1] = 1
    table["confidence"][:, 1] = 0.9
    table["confidence"][7, 1] = 0.0                                       # a lost pair stays untouched
    conf = table["confidence"][:, 1].copy()
    out = dc.write_transitions(table, dc.transitions(C), ["similarity"] * (n - 1), conf, sched)
    assert np.array_equal(out["matrix"][7, 1], np.eye(3, dtype=np.float32).reshape(9))
    assert np.array_equal(out["matrix"][:, 0], table["matrix"][:, 0]) and np.array_equal(out["confidence"], table["confidence"])
    assert np.array_equal(table["matrix"][3, 1], np.eye(3, dtype=np.float32).reshape(9))   # the input table is not written
    out["matrix"][7, 1] = (C[8] @ np.linalg.inv(C[7])).astype(np.float32).reshape(9)
    acc = np.eye(3)
    worst = 0.0
    for k in range(n - 1):
        acc = out["matrix"][k, 1].reshape(3, 3).astype(np.float64) @ acc
        worst = max(worst, _corner_error(acc, C[k + 1], (960, 540)))
    assert worst < 1e-3, worst


# ---- 4. recovery ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_clip():
    import torch

    import bench

    w, h, n = 240, 135, 6
    cams = {mode: shake_path(n, w, h, mode) for mode in ("similarity", "translation")}
    grays = {mode: _gray(bench.synth_clip(n, 0, h, w, torch.device("cpu"), mats=cam).numpy()) for mode, cam in cams.items()}
    return w, h, n, cams, grays


@pytest.mark.parametrize("mode", ["similarity", "translation"])
def test_a_pixel_of_initial_error_is_recovered(dc, small_clip, mode):
    """The true matrix perturbed by (0.7, -0.4) px, 0.001 rad and scale 1.001 about the centre (0.95 px at a corner) comes back
    within 0.03 px of the analytic truth at the worst corner (a float prototype reaches 0.010).  In translation mode the clip
    is a translation and the perturbation is the shift alone."""
    w, h, n, cams, grays = small_clip
    cam, gray = cams[mode], grays[mode]
    truth = np.stack([cam[i] @ np.linalg.inv(cam[0]) for i in range(n)])
    off = similarity(0.7, -0.4, 0.001, 1.001, (w - 1) / 2, (h - 1) / 2) if mode == "similarity" else similarity(0.7, -0.4, 0.0, 1.0)
    start = np.stack([truth[0]] + [off.astype(np.float64) @ truth[i] for i in range(1, n)])
    work = np.stack([start[k + 1] @ np.linalg.inv(start[k]) for k in range(n - 1)])
    sched = dc.schedule(n, None, [0.9] * (n - 1), 32)
    calls = []
    got = dc.refine(_sums_fn(gray, dc.RESIDUAL_CAP, calls), work, sched, mode, (w, h))
    before = max(_corner_error(got.R_chained[i], truth[i], (w, h)) for i in range(1, n))
    after = max(_corner_error(got.R[i], truth[i], (w, h)) for i in range(1, n))
    print(f"{mode}: worst corner {before:.4f} px -> {after:.4f} px in {got.launches} launches")
    assert (0.9 < before < 1.0) if mode == "similarity" else abs(before - np.hypot(0.7, 0.4)) < 1e-6
    assert got.reason == ["no_anchor"] + [None] * (n - 1)
    assert after <= 0.03, after
    assert 2 <= got.launches <= dc.MAX_ITERATIONS + 1 and got.launches == len(calls) == got.iterations + 1
    assert all(c[0] == -1 for c in calls)
    # a converged frame leaves the later launches, and the last launch evaluates every refined frame
    assert calls[-1].tolist() == sched.anchor.tolist()
    assert int(got.sums_final[1:, 2].sum()) * int(got.sums_first[1:, 0].sum()) < int(got.sums_first[1:, 2].sum()) * int(got.sums_final[1:, 0].sum())


def test_a_pure_shift_is_updated_from_its_rounded_form(dc, small_clip, monkeypatch):
    """Under a pure shift every pixel rounds to the same cell of the 1/32 px grid, so the sums are those of the ROUNDED shift
    and the update has to start there (drift_correction.sampled_at).  Applied to the unrounded shift the iterations hop
    between two cells: on this clip they use all MAX_ITERATIONS and end further from the truth.  In similarity mode the
    first update leaves ~1e-6 of rotation in the matrix, which changes nothing about the rounding: the same must hold."""
    w, h, n, cams, grays = small_clip
    cam, gray = cams["translation"], grays["translation"]
    truth = np.stack([cam[i] @ np.linalg.inv(cam[0]) for i in range(n)])
    off = similarity(0.7, -0.4, 0.0, 1.0).astype(np.float64)
    start = np.stack([truth[0]] + [off @ truth[i] for i in range(1, n)])
    work = np.stack([start[k + 1] @ np.linalg.inv(start[k]) for k in range(n - 1)])
    sched = dc.schedule(n, None, [0.9] * (n - 1), 32)
    assert np.allclose(dc.sampled_at(np.array([[1.0, 0, 0.26], [0, 1.0, -1.49]]), (w, h)), [[1.0, 0, 0.25], [0, 1.0, -1.5]], rtol=0, atol=1e-12)
    assert np.allclose(dc.sampled_at(np.array([[1.0, 1e-7, 0.26], [-1e-7, 1.0, -1.49]]), (w, h)), [[1.0, 1e-7, 0.25], [-1e-7, 1.0, -1.5]], rtol=0, atol=1e-4)
    turned = np.array([[np.cos(0.01), -np.sin(0.01), 0.26], [np.sin(0.01), np.cos(0.01), -1.49]])
    assert np.abs(dc.sampled_at(turned, (w, h)) - turned).max() < 2e-3  # a real rotation or zoom: the rounding averages out
    for mode in ("translation", "similarity"):                         # (a pure-shift chain in similarity mode is one too)
        with_it = dc.refine(_sums_fn(gray, dc.RESIDUAL_CAP), work, sched, mode, (w, h))
        monkeypatch.setattr(dc, "sampled_at", lambda R23, size: np.asarray(R23, dtype=np.float64))
        without = dc.refine(_sums_fn(gray, dc.RESIDUAL_CAP), work, sched, mode, (w, h))
        monkeypatch.undo()
        err = [max(_corner_error(r.R[i], truth[i], (w, h)) for i in range(1, n)) for r in (with_it, without)]
        print(f"{mode}: with {with_it.iterations} iterations, {err[0]:.4f} px; without {without.iterations}, {err[1]:.4f} px")
        assert with_it.iterations < dc.MAX_ITERATIONS and without.iterations == dc.MAX_ITERATIONS     # converges / never does
        assert err[0] < err[1] and err[0] <= 0.03


# ---- 5. keep reasons -----------------------------------------------------------------------------------------------------------
def _blob(h, w, cx, cy, sigma=14.0):
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(30 + 200 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma ** 2)), 0, 255).astype(np.uint8)


def _one_pair(dc, template, image, start, mode="similarity"):
    h, w = template.shape
    gray = np.stack([template, image])
    work = np.asarray(start, np.float64).reshape(1, 3, 3)
    sched = dc.schedule(2, None, [0.9], 32)
    return dc.refine(_sums_fn(gray, dc.RESIDUAL_CAP), work, sched, mode, (w, h))


def test_every_keep_reason_once(dc, small_clip):
    w, h, n, cams, grays = small_clip
    gray = grays["similarity"]
    truth = cams["similarity"][1] @ np.linalg.inv(cams["similarity"][0])
    # singular: a flat template has no gradient
    got = _one_pair(dc, np.full((h, w), 90, np.uint8), gray[1], np.eye(3))
    assert got.reason == ["no_anchor", "singular"] and np.array_equal(got.R[1], got.R_chained[1])
    # overlap: the matrix puts more than half of the template outside the frame
    away = truth.copy()
    away[0, 2] += 0.6 * w
    got = _one_pair(dc, gray[0], gray[1], away)
    assert got.reason[1] == "overlap" and np.array_equal(got.R[1], got.R_chained[1])
    assert int(got.sums_final[1, 0]) < 0.5 * (w - 2) * (h - 2)
    # cost: two unrelated images, a texture and noise within the cap of it, from a half-pixel start.  No motion explains the
    # pair; the half-pixel taps average the noise the most, so wherever the template's gradients send the iterations the
    # image gets sharper and the mean |r| rises
    rng = np.random.default_rng(1)
    soft = (128 + (gray[0].astype(np.float64) - 128) * 0.3).astype(np.uint8)
    half = np.eye(3)
    half[0, 2] = half[1, 2] = 0.5
    got = _one_pair(dc, soft, rng.integers(100, 157, (h, w), dtype=np.uint8), half)
    assert got.reason[1] == "cost", got.reason
    assert int(got.sums_final[1, 0]) >= 0.5 * (w - 2) * (h - 2) and np.array_equal(got.R[1], got.R_chained[1])
    assert int(got.sums_final[1, 2]) * int(got.sums_first[1, 0]) > int(got.sums_first[1, 2]) * int(got.sums_final[1, 0])
    # step: a 10 px initial error on a smooth image converges, and that is not drift
    far = np.eye(3)
    far[0, 2] = 10.0
    got = _one_pair(dc, _blob(h, w, 120, 67), _blob(h, w, 120, 67), far)
    assert got.reason[1] == "step", got.reason
    assert np.array_equal(got.R[1], got.R_chained[1])


# ---- 6. requests, plan hook, node, header ----------------------------------------------------------------------------------------
class NoClip:
    frames = None


ARGS = ("crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0)
M = np.zeros((4, 4), np.float32)
M3 = np.zeros((2, 4, 4), np.float32)


def test_check_request(dc):
    assert dc.check_request(None) is None and dc.check_request(0) is None and dc.check_request(False) is None
    assert dc.check_request(True) == 32 == dc.DEFAULT_SPACING and dc.check_request(2) == 2 and dc.check_request(4096) == 4096
    assert dc.check_request(np.int64(16)) == 16
    for bad in (1, -3, 4097, 16.0, 2.5, "auto", (8,), float("nan")):
        with pytest.raises(ValueError) as caught:
            dc.check_request(bad)
        assert repr(bad) in str(caught.value)
    assert (dc.MAX_ITERATIONS, dc.CONVERGED_PX, dc.MIN_OVERLAP, dc.MAX_CORRECTION_PX, dc.RESIDUAL_CAP) == (6, 0.005, 0.5, 4.0, 32)


REFUSALS = [
    ("similarity", dict(drift_correction=1.5), "drift_correction=1.5: expected None / False / 0 (off), True (a keyframe every 32 frames) or an int in 2..4096, the keyframe spacing."),
    ("perspective", dict(drift_correction=True), "drift_correction does not support transform_mode='perspective': the keyframe alignment updates a similarity (shift, zoom, rotation); use 'translation' or 'similarity'."),
    ("similarity", dict(drift_correction=8, estimator="subject", subject_mask=M3), "drift_correction does not support estimator='subject': its transitions follow the subject, while the estimation images the keyframe alignment reads show the background."),
    ("similarity", dict(drift_correction=8, estimation_mask=M), "drift_correction does not support estimation_mask: the keyframe alignment has no per-pixel exclusion yet (its residual cap is the only guard against moving subjects)."),
]

# wrong in two ways: the new check loses to every older one (one call per older check of check_flow_request, in its order)
OLDER_WINS = [
    (dict(mask_tapered=False), "mask_tapered=False needs"),
    (dict(dynamic_zoom=99.0), "dynamic_zoom=99.0"),
    (dict(spatial_fill="yes"), "spatial_fill='yes'"),
    (dict(stability_report=2), "stability_report=2"),
    (dict(scene_cuts="sometimes"), "scene_cuts='sometimes'"),
    (dict(mesh_warp=(1, 1)), "mesh_warp=(1, 1)"),
    (dict(mesh_motion=True), "mesh_motion=True needs mesh_warp"),
    (dict(estimator="nope"), "Unknown estimator 'nope'"),
    (dict(estimator="subject"), "estimator='subject' needs subject_mask"),
    (dict(temporal_fill=99), "temporal_fill=99 outside"),
    (dict(fill_feather=8), "fill_feather=8"),
    (dict(sharpness_transfer=99), "sharpness_transfer=99"),
    (dict(sharpness_transfer=2, mesh_warp=True), "sharpness_transfer is not supported with mesh_warp"),
    (dict(estimation_mask=M, mask_margin=99), "mask_margin=99"),
    (dict(estimator="classic", estimation_mask=M), "estimation_mask is not supported with estimator 'classic'"),
    (dict(mesh_warp=True, temporal_fill=2), "mesh_warp is not supported with temporal_fill=2"),
    (dict(estimator="subject", subject_mask=M3, temporal_fill=2), "temporal_fill=2 is not supported with estimator 'subject'"),
    (dict(rolling_shutter=7.0), "rolling_shutter=7.0"),
    (dict(rolling_shutter=0.5, temporal_fill=2), "rolling_shutter is not supported with temporal_fill=2"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_and_its_message(pkg, monkeypatch, case):
    from vstab_amd import flow_pipeline

    monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    mode, keywords, message = REFUSALS[case]
    with pytest.raises(ValueError) as caught:
        flow_pipeline._stabilize_frames(NoClip(), "crop_and_pad", mode, *ARGS[2:], **keywords)
    assert str(caught.value) == message


@pytest.mark.parametrize("case", range(len(OLDER_WINS)))
def test_the_new_checks_lose_to_every_older_one(pkg, monkeypatch, case):
    from vstab_amd import flow_pipeline

    monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    keywords, start = OLDER_WINS[case]
    with pytest.raises(ValueError) as caught:
        flow_pipeline._stabilize_frames(NoClip(), *ARGS, drift_correction=1.5, **keywords)
    assert str(caught.value).startswith(start), str(caught.value)


def test_sharded_refusal_is_the_last_of_the_table(pkg):
    from vstab_amd import distributed

    call = (None, None, 12, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
    with pytest.raises(ValueError) as caught:
        distributed.stabilize_sharded(*call, drift_correction=16)
    assert str(caught.value) == ("stabilize_sharded does not support drift_correction=16: the keyframe alignment is not sharded "
                                 "(a frame's keyframe may lie on another rank); run the single-GPU pipeline for it")
    with pytest.raises(ValueError, match="sharpness_transfer=2"):
        distributed.stabilize_sharded(*call, drift_correction=True, sharpness_transfer=2)
    for off in (None, 0, False):                                         # off: the next refusal in the table's order wins
        with pytest.raises(ValueError, match="does not support scene_cuts"):
            distributed.stabilize_sharded(*call, drift_correction=off, scene_cuts="auto")
    assert inspect.signature(distributed.stabilize_sharded).parameters["drift_correction"].default is None


def test_request_and_signature(pkg):
    from vstab_amd import flow_pipeline as fp

    p = inspect.signature(fp._stabilize_frames).parameters["drift_correction"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    kw = {name: prm.default for name, prm in inspect.signature(fp._stabilize_frames).parameters.items() if prm.kind is inspect.Parameter.KEYWORD_ONLY}
    off = fp.check_flow_request("crop_and_pad", "similarity", "flow", kw)
    assert off.drift is None and not off.needs_host_plan and off.kept_by_products == ()
    on = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, drift_correction=True))
    assert on.drift == 32 and on.needs_host_plan and on.kept_by_products == ("gray_out",)
    both = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, drift_correction=5, mesh_warp=True, scene_cuts="auto"))
    assert both.drift == 5 and both.kept_by_products == ("gray_out", "grid_out")
    for est in ("classic", "flow_phase_correlate", "flow_tvl1"):
        if est in fp._ESTIMATORS:
            assert fp.check_flow_request("expand", "translation", est, dict(kw, drift_correction=2)).drift == 2
    assert inspect.signature(fp._plan_stabilization).parameters["path_deltas"].default is None


def test_node_schema(pkg):
    from vstab_amd import nodes

    s = nodes.VideoStabilizerFlowAnchored.define_schema()
    base = nodes.VideoStabilizerFlow.define_schema()
    assert s.node_id == "video_stabilizer_flow_anchored" and s.display_name == "Video Stabilizer Flow (Drift-Free)"
    assert [i.id for i in s.inputs] == [i.id for i in base.inputs] + ["keyframe_spacing"]
    assert [o.id for o in s.outputs] == [o.id for o in base.outputs]
    by_id = {i.id: i for i in s.inputs}
    assert by_id["transform_mode"].options["options"] == ["translation", "similarity"]
    k = by_id["keyframe_spacing"]
    assert k.kind.upper() == "INT" and (k.options["default"], k.options["min"], k.options["max"]) == (32, 2, 4096)
    assert nodes.VideoStabilizerFlowAnchored not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    import asyncio

    listed = asyncio.run(nodes.VideoStabilizerAmdAnchorExtension().get_node_list())
    before = asyncio.run(nodes.VideoStabilizerAmdRollingApplyExtension().get_node_list())
    assert listed == before + [nodes.VideoStabilizerFlowAnchored] and nodes.VideoStabilizerFlowAnchored not in before
    assert list(inspect.signature(nodes.VideoStabilizerFlowAnchored.execute).parameters)[-1] == "keyframe_spacing"
    import vstab_amd

    entry = asyncio.run(vstab_amd.comfy_entrypoint())                    # unchanged: the drift-free node is not handed to ComfyUI
    assert nodes.VideoStabilizerFlowAnchored not in asyncio.run(entry.get_node_list())


def test_header_binding_and_documents_agree(pkg):
    from vstab_amd import native

    text = (ROOT / "include" / "vstab.h").read_text()
    assert ("int vstab_anchor_sums_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const int32_t* anchor,\n"
            "                            const double* R, int cap, int64_t* out);") in text
    assert "#define VSTAB_ANCHOR_SLOTS 17" in text and R.SLOTS == 17
    assert text.count("---- Drift correction") == 1
    assert "vstab_anchor_sums_batch" in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), "vstab_anchor_sums_batch")
    assert list(inspect.signature(native.Context.anchor_sums_batch).parameters)[1:] == ["gray", "anchor", "R", "cap"]
    assert "vstab_anchor.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    for doc, words in (("INTEGRATION.md", ("vstab_anchor_sums_batch", "VideoStabilizerAmdAnchorExtension")),
                       ("README.md", ("drift_correction", "Drift-Free")), ("DESIGN.md", ("8m", "vstab_anchor_sums_batch"))):
        body = (ROOT / doc).read_text()
        for word in words:
            assert word in body, (doc, word)
