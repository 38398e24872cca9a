"""Scene cuts, the parts that need no GPU: the NumPy restatement of the residual's rule on hand-made cases, the decision and
segmentation helpers, the public surface (keywords, export, node) and the ValueErrors raised before any GPU work."""

import asyncio
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import scene_cuts_restatement as R

ROOT = Path(__file__).resolve().parents[1]
ARGS = ("crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)


# ---- the restatement itself, on cases small enough to do by hand ---------------------------------------------------------
def test_identity_on_equal_images():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (7, 11), dtype=np.uint8)
    assert R.pair_residual(img, img, np.eye(3)) == (0, 7 * 11)
    other = img.copy()
    other[3, 4] = np.uint8((int(img[3, 4]) + 100) % 256)
    assert R.pair_residual(img, other, np.eye(3)) == (abs(int(img[3, 4]) - int(other[3, 4])), 77)


def test_integer_shift_overlap_and_sum():
    """x_to = x_from + 3, y_to = y_from - 2 on 10x8 (w x h): the pixels with x <= 6 and y >= 2 land inside: 7 * 6 = 42."""
    h, w = 8, 10
    a = np.arange(h * w, dtype=np.uint8).reshape(h, w)           # a[y, x] = 10 y + x
    b = np.full((h, w), 200, np.uint8)
    m = np.array([[1, 0, 3], [0, 1, -2], [0, 0, 1]], np.float32)
    want = sum(abs(int(a[y, x]) - 200) for y in range(2, h) for x in range(0, w - 3))
    assert R.pair_residual(a, b, m) == (want, 42)
    # the TO image is read at q, not at p: a marker at q = (5, 1) is met by p = (2, 3)
    b2 = np.zeros((h, w), np.uint8)
    b2[1, 5] = 255
    z = np.zeros((h, w), np.uint8)
    assert R.pair_residual(z, b2, m) == (255, 42)


def test_half_pixel_shifts_round_to_even():
    """q = x + 0.5: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4: on a 1x4 row x = 3 leaves the frame (4 > 3)."""
    a = np.zeros((1, 4), np.uint8)
    b = np.array([[10, 20, 30, 40]], np.uint8)
    m = np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]], np.float32)
    assert R.pair_residual(a, b, m) == (10 + 30 + 30, 3)


def test_everything_outside_counts_nothing():
    img = np.full((6, 9), 7, np.uint8)
    far = np.array([[1, 0, 100], [0, 1, 0], [0, 0, 1]], np.float32)
    assert R.pair_residual(img, img, far) == (0, 0)
    behind = np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32)      # w < 0 everywhere
    assert R.pair_residual(img, img, behind) == (0, 0)
    zero_w = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32)       # w == 0 everywhere
    assert R.pair_residual(img, img, zero_w) == (0, 0)


def test_non_finite_entries_count_nothing():
    img = np.full((5, 5), 9, np.uint8)
    for k in range(9):
        for bad in (np.nan, np.inf, -np.inf):
            m = np.eye(3, dtype=np.float32).reshape(9)
            m[k] = bad
            # inf * 0 is NaN and inf * x is inf: X, Y or W is non-finite at every pixel
            assert R.pair_residual(img, img, m.reshape(3, 3)) == (0, 0), (k, bad)


def test_batch_is_the_pairs():
    rng = np.random.default_rng(1)
    gray = rng.integers(0, 256, (4, 9, 13), dtype=np.uint8)
    mats = np.stack([np.eye(3), [[1, 0, 2], [0, 1, 1], [0, 0, 1]], [[0.9, 0.1, 0], [-0.1, 0.9, 1], [1e-3, 0, 1]]]).astype(np.float32)
    s, n = R.pair_residual_batch(gray, mats)
    assert s.dtype == np.int64 and n.dtype == np.int64
    for i in range(3):
        assert (int(s[i]), int(n[i])) == R.pair_residual(gray[i], gray[i + 1], mats[i])


# ---- decision and segmentation ------------------------------------------------------------------------------------------
def test_scores_overlap_and_decision(pkg):
    from vstab_amd import scene_cuts as sc

    h, w = 10, 20                                                  # 200 pixels
    sum_abs = np.array([400, 3000, 0, 1234, 50 * 49])
    inside = np.array([200, 100, 0, 50, 49])                       # overlap 1.0, 0.5, 0.0, 0.25 (exactly), 0.245
    scores, overlap = sc.scores_and_overlap(sum_abs, inside, h, w)
    assert scores.dtype == np.float64 and overlap.dtype == np.float64
    assert scores.tolist() == [2.0, 30.0, 255.0, 1234 / 50, 50.0]  # inside == 0: nothing divided, reported as 255
    assert overlap.tolist() == [1.0, 0.5, 0.0, 0.25, 0.245]
    assert sc.is_cut(scores, overlap, 30.0).tolist() == [False, True, True, False, True]     # score == threshold is a cut
    assert sc.is_cut(scores, overlap, 30.000001).tolist() == [False, False, True, False, True]
    assert sc.is_cut(scores, overlap, 25.0).tolist() == [False, True, True, False, True]     # 24.68 at overlap 0.25: not a cut
    assert sc.is_cut(scores, overlap, 24.0).tolist() == [False, True, True, True, True]
    assert sc.OVERLAP_MIN == 0.25


def test_cuts_and_segments(pkg):
    from vstab_amd import scene_cuts as sc

    assert sc.cuts_from_pairs([False, False, True, False]) == [3]
    assert sc.segments_from_cuts([3], 5) == [(0, 3), (3, 5)]
    assert sc.segments_from_cuts([], 5) == [(0, 5)]
    every = sc.cuts_from_pairs([True] * 4)                         # a cut at every pair: five one-frame shots
    assert every == [1, 2, 3, 4]
    assert sc.segments_from_cuts(every, 5) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert sc.segments_from_cuts([1, 4], 5) == [(0, 1), (1, 4), (4, 5)]


def test_scoring_transition_is_the_pairs_own_best_candidate(pkg):
    from vstab_amd import native
    from vstab_amd import scene_cuts as sc

    def cand(v, accepted=True):
        return {"matrix": np.full((3, 3), v, np.float32), "confidence": 0.5, "residual": 0.1, "accepted": accepted}

    table = native.fit_table_from_dicts([
        {"translation": cand(1), "similarity": cand(2), "perspective": cand(3)},
        {"translation": cand(1), "similarity": cand(2), "perspective": cand(3, accepted=False)},
        {"translation": cand(1), "similarity": cand(2, accepted=False), "perspective": cand(3, accepted=False)},
        {},
        {"translation": cand(1), "similarity": cand(2), "perspective": cand(3)},      # no stickiness: back at the top
    ])
    got = sc.scoring_transitions(table, "perspective")
    assert got.dtype == np.float32 and got.shape == (5, 3, 3)
    assert [float(m[0, 1]) for m in got] == [3.0, 2.0, 1.0, 0.0, 3.0]
    assert np.array_equal(got[3], np.eye(3, dtype=np.float32))
    assert [float(m[0, 1]) for m in sc.scoring_transitions(table, "similarity")] == [2.0, 2.0, 1.0, 0.0, 2.0]
    assert [float(m[0, 1]) for m in sc.scoring_transitions(table, "translation")] == [1.0, 1.0, 1.0, 0.0, 1.0]


def test_selection_restarts_in_every_segment(pkg):
    """The sticky walk: a rejected fit in shot A must not downgrade shot B; the pair across the cut is "no candidate"."""
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import native

    def cand(v, accepted=True):
        return {"matrix": np.array([[1, 0, v], [0, 1, 0], [0, 0, 1]], np.float32), "confidence": 0.5, "residual": 0.1, "accepted": accepted}

    good = {"translation": cand(1), "similarity": cand(2)}
    weak = {"translation": cand(1), "similarity": cand(2, accepted=False)}
    table = native.fit_table_from_dicts([good, weak, good, good, good, good])     # 7 frames; the cut is pair 3 (frame 4 starts B)
    _, modes, _, _, active = fp.select_transitions(table, "similarity")
    assert modes == ["similarity"] + ["translation"] * 5 and active == "translation"           # one clip: sticky to the end
    mats, modes, confs, resids, active = fp._select_per_segment(table, "similarity", [(0, 4), (4, 7)])
    assert modes == ["similarity", "translation", "translation", "translation", "similarity", "similarity"]
    assert active == "similarity"
    assert np.array_equal(mats[3], np.eye(3, dtype=np.float32)) and confs[3] == 0.0 and resids[3] == 0.0
    assert confs[0] == 0.5 and float(mats[4][0, 2]) == 2.0
    # one-frame shots have no transition: every pair is a cut
    mats, modes, confs, _, active = fp._select_per_segment(table, "similarity", [(k, k + 1) for k in range(7)])
    assert modes == ["translation"] * 6 and confs == [0.0] * 6 and active == "similarity"
    assert (mats == np.eye(3, dtype=np.float32)).all()


def test_meta_block_shape(pkg):
    from vstab_amd import scene_cuts as sc

    auto = sc.meta_block(sc.check_request("auto", 12.5), [3], np.array([1.0, 2.0, 40.0, 1.5]), np.array([1.0, 0.9, 1.0, 0.95]))
    assert auto == {"mode": "auto", "threshold": 12.5, "cuts": [3], "segments": 2, "scores": [1.0, 2.0, 40.0, 1.5],
                    "overlap": [1.0, 0.9, 1.0, 0.95]}
    given = sc.meta_block(sc.check_request([2, 4]), [2, 4])
    assert given == {"mode": "given", "threshold": None, "cuts": [2, 4], "segments": 3, "scores": None, "overlap": None}
    assert sc.check_request("auto").threshold == sc.DEFAULT_CUT_THRESHOLD
    assert sc.check_request(None) is None and sc.check_request(None, 5.0) is None


# ---- public surface -------------------------------------------------------------------------------------------------------
def test_keywords_and_export(pkg):
    from vstab_amd import distributed, flow_pipeline, native

    sig = inspect.signature(flow_pipeline._stabilize_frames).parameters
    for name in ("scene_cuts", "cut_threshold"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None
    assert inspect.signature(distributed.stabilize_sharded).parameters["scene_cuts"].default is None
    assert "vstab_pair_residual_batch" in native.EXPORTED_SYMBOLS
    assert list(inspect.signature(native.Context.pair_residual_batch).parameters)[1:] == ["gray", "transitions"]
    assert inspect.signature(flow_pipeline._plan_stabilization).parameters["segments"].default is None


def test_header_exports_the_call_and_states_the_rule():
    text = (ROOT / "include" / "vstab.h").read_text()
    flat = re.sub(r"\s+", " ", text)
    assert ("int vstab_pair_residual_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const float* transitions, "
            "uint64_t* sum_abs, uint32_t* inside);") in flat
    block = text[text.index("---- Scene cuts"):text.index("int vstab_pair_residual_batch")]
    for phrase in ("x_{i+1} = A_i x_i", "no matrix is inverted", "(A0*x + A1*y) + A2", "ties to even", "W <= 0", "not finite",
                   "inside_i += 1", "sum_abs_i += |gray_i[p] - gray_{i+1}[q]|", "order of the reduction", 'timing kind "cut"',
                   "overlap < 0.25"):
        assert phrase in block, phrase
    assert text.count("---- Scene cuts") == 1                      # stated once
    makefile = (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert "vstab_cut.hip" in makefile and (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "vstab_cut.hip").exists()


def test_scene_node_schema(pkg):
    from vstab_amd import nodes
    from vstab_amd import scene_cuts as sc

    assert len(nodes.NODE_CLASSES) == 6 and nodes.VideoStabilizerFlowScenes not in nodes.NODE_CLASSES
    listed = asyncio.run(nodes.VideoStabilizerAmdScenesExtension().get_node_list())
    assert len(listed) == 9 and listed[:6] == nodes.NODE_CLASSES and listed[8] is nodes.VideoStabilizerFlowScenes
    assert listed[:8] == asyncio.run(nodes.VideoStabilizerAmdMaskedExtension().get_node_list())
    s = nodes.VideoStabilizerFlowScenes.define_schema()
    flow = nodes.VideoStabilizerFlow.define_schema()
    assert s.node_id == "video_stabilizer_flow_scenes" and s.display_name == "Video Stabilizer Flow (Scene-Aware)"
    assert [i.id for i in s.inputs] == [i.id for i in flow.inputs] + ["cut_threshold"]      # no temporal_fill socket
    assert [o.id for o in s.outputs] == [o.id for o in flow.outputs]
    for a, b in zip(s.inputs, flow.inputs):
        assert a.kind == b.kind and a.options == b.options
    thr = s.inputs[-1]
    assert thr.kind.upper() == "FLOAT" and thr.options["default"] == sc.DEFAULT_CUT_THRESHOLD and thr.options["min"] == 0.0
    assert list(inspect.signature(nodes.VideoStabilizerFlowScenes.execute).parameters) == \
        list(inspect.signature(nodes.VideoStabilizerFlow.execute).parameters) + ["cut_threshold"]


# ---- argument validation, before any GPU work ---------------------------------------------------------------------------
def _context(pkg, n=4, h=24, w=32):
    import torch

    from vstab_amd import host_math as hm

    return hm._normalize_video_input(torch.zeros((n, h, w, 3)))


@pytest.mark.parametrize("value,text", [
    ("yes", r"scene_cuts='yes': expected None, 'auto' or a sequence of frame indices"),
    (7, r"scene_cuts=7: expected None, 'auto' or a sequence of frame indices"),
    ([0], r"scene_cuts entry 0 outside \[1, 3\] for a clip of 4 frames"),
    ([4], r"scene_cuts entry 4 outside \[1, 3\] for a clip of 4 frames"),
    ([-1, 2], r"scene_cuts entry -1 outside \[1, 3\]"),
    ([2, 2], r"scene_cuts entry 2 does not increase \(after 2\)"),
    ([3, 1], r"scene_cuts entry 1 does not increase \(after 3\)"),
    ([1.5], r"scene_cuts entry 1.5 is not an integer frame index"),
    ([True], r"scene_cuts entry True is not an integer frame index"),
])
def test_bad_scene_cuts_name_the_value(pkg, value, text):
    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError, match=text):
        fp._stabilize_frames(_context(pkg), *ARGS, scene_cuts=value)


@pytest.mark.parametrize("value", [0, 0.0, -3.0, float("nan"), float("inf"), "12", True])
def test_bad_cut_threshold_names_the_value(pkg, value):
    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError, match=r"cut_threshold=.*expected a finite number above 0"):
        fp._stabilize_frames(_context(pkg), *ARGS, scene_cuts="auto", cut_threshold=value)


def test_sharded_path_says_scene_cuts_are_not_sharded(pkg):
    from vstab_amd import distributed

    for value in ("auto", [2]):
        with pytest.raises(ValueError, match="scene cuts are not sharded"):
            distributed.stabilize_sharded(None, None, 4, *ARGS, scene_cuts=value)


def test_bypasses_ignore_the_keyword(pkg):
    """0 / 1 frames: returned before any GPU work, with the reference's meta (no scene_cuts key), whatever the edit list says."""
    import dataclasses

    from vstab_amd import flow_pipeline as fp

    for n in (0, 1):
        def make():
            return _context(pkg, n=n) if n else dataclasses.replace(_context(pkg, n=1), frames=[], batch=None)

        without = fp._stabilize_frames(make(), *ARGS)
        for value in ("auto", [1], [5, 9]):
            got = fp._stabilize_frames(make(), *ARGS, scene_cuts=value)
            assert got.meta == without.meta and "scene_cuts" not in got.meta
