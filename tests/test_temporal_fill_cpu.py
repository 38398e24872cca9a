"""CPU: the temporal fill's host side (temporal_fill.fill_candidates, the meta reader, the seventh node's schema) and the
referee of the validity rule the GPU tests rely on (tests/temporal_fill_restatement.py against oracle.warp_frame)."""

import asyncio
import re
from pathlib import Path

import numpy as np
import pytest

from tests import temporal_fill_restatement as R

ROOT = Path(__file__).resolve().parents[1]


def _translation(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float32)


def _integer_clip(n, seed=5):
    """Frame offsets o_i (integers): x_{i+1} = x_i + (o_i - o_{i+1}); final matrices F_i = translation by an integer s_i."""
    rng = np.random.default_rng(seed)
    offs = rng.integers(-20, 21, size=(n, 2))
    shifts = rng.integers(-6, 7, size=(n, 2))
    trans = np.stack([_translation(*(offs[i] - offs[i + 1])) for i in range(n - 1)])
    final = np.stack([_translation(*shifts[i]) for i in range(n)])
    return offs, shifts, trans, final


def test_candidates_integer_translations_are_exact(pkg):
    from vstab_amd import temporal_fill as tf

    n, radius = 9, 3
    offs, shifts, trans, final = _integer_clip(n)
    mats, cand = tf.fill_candidates(final, trans, np.ones(n - 1), radius)
    assert mats.shape == (n, 2 * radius, 3, 3) and mats.dtype == np.float32
    assert cand.shape == (n, 2 * radius) and cand.dtype == np.int32
    for i in range(n):
        for d in range(1, radius + 1):
            for side, j in ((0, i - d), (1, i + d)):
                k = 2 * (d - 1) + side           # order: d = 1 .. R, the earlier frame before the later one
                if not 0 <= j < n:
                    assert cand[i, k] == -1      # clip edge
                    continue
                assert cand[i, k] == j
                # x_i = x_j + (o_j - o_i), canvas = x_i + s_i
                expect = _translation(*(offs[j] - offs[i] + shifts[i]))
                assert np.array_equal(mats[i, k], expect), (i, j, mats[i, k], expect)


def test_candidates_window_matches_whole_clip(pkg):
    from vstab_amd import temporal_fill as tf

    _, _, trans, final = _integer_clip(8)
    mats, cand = tf.fill_candidates(final, trans, np.ones(7), 2)
    m2, c2 = tf.fill_candidates(final, trans, np.ones(7), 2, first=3, count=4)
    assert np.array_equal(m2, mats[3:7]) and np.array_equal(c2, cand[3:7])


def test_candidates_zero_confidence_cuts_chains_across_only(pkg):
    from vstab_amd import temporal_fill as tf

    n, radius, cut = 8, 3, 3                       # transition 3 (frames 3 -> 4) has no estimate
    _, _, trans, final = _integer_clip(n)
    conf = np.ones(n - 1)
    conf[cut] = 0.0
    _, cand = tf.fill_candidates(final, trans, conf, radius)
    _, full = tf.fill_candidates(final, trans, np.ones(n - 1), radius)
    for i in range(n):
        for k in range(2 * radius):
            j = full[i, k]
            if j < 0:
                assert cand[i, k] == -1
                continue
            crosses = min(i, j) <= cut < max(i, j)
            assert cand[i, k] == (-1 if crosses else j), (i, j)
    # a negative confidence and a NaN one cut as well; min_confidence moves the threshold
    conf[cut] = np.nan
    assert np.array_equal(tf.fill_candidates(final, trans, conf, radius)[1], cand)
    assert (tf.fill_candidates(final, trans, np.full(n - 1, 0.3), radius, min_confidence=0.3)[1] == -1).all()


def test_candidates_neighbours_match_float64_recomputation(pkg):
    from vstab_amd import temporal_fill as tf
    from tests.util import similarity

    rng = np.random.default_rng(11)
    n = 6
    trans = np.stack([similarity(rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.03, 0.03), rng.uniform(0.97, 1.03), 64, 36)
                      for _ in range(n - 1)]).astype(np.float32)
    trans[2, 2, :2] = (1e-5, -2e-5)               # one perspective transition
    final = np.stack([similarity(rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(-0.05, 0.05), 1.05, 64, 36)
                      for _ in range(n)]).astype(np.float32)
    mats, cand = tf.fill_candidates(final, trans, np.ones(n - 1), 1)
    for i in range(n):
        F = final[i].astype(np.float64)
        if i > 0:
            assert cand[i, 0] == i - 1
            assert np.array_equal(mats[i, 0], (F @ trans[i - 1].astype(np.float64)).astype(np.float32))
        if i < n - 1:
            assert cand[i, 1] == i + 1
            assert np.array_equal(mats[i, 1], (F @ np.linalg.inv(trans[i].astype(np.float64))).astype(np.float32))


def test_candidates_reject_singular_and_nonfinite(pkg):
    from vstab_amd import temporal_fill as tf

    _, _, trans, final = _integer_clip(5)
    trans = trans.copy()
    trans[1] = 0.0                                  # singular
    trans[3, 0, 2] = np.inf
    _, cand = tf.fill_candidates(final, trans, np.ones(4), 4)
    _, full = tf.fill_candidates(final, _integer_clip(5)[2], np.ones(4), 4)
    for i in range(5):
        for k in range(8):
            j = full[i, k]
            if j >= 0:
                crosses = any(min(i, j) <= c < max(i, j) for c in (1, 3))
                assert cand[i, k] == (-1 if crosses else j)
    with pytest.raises(ValueError):
        tf.fill_candidates(final, trans, np.ones(4), 0)
    with pytest.raises(ValueError):
        tf.fill_candidates(final, trans[:2], np.ones(2), 2)


# ---- referee of the validity rule: where the restatement calls a candidate valid, the border did not contribute -------
def _drawn_matrices(w, h, seed):
    from tests.util import similarity

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(6):
        out.append(similarity(rng.uniform(-0.4 * w, 0.4 * w), rng.uniform(-0.4 * h, 0.4 * h), rng.uniform(-0.3, 0.3),
                              rng.uniform(0.8, 1.25), w / 2, h / 2))
    for _ in range(6):
        m = similarity(rng.uniform(-0.3 * w, 0.3 * w), rng.uniform(-0.3 * h, 0.3 * h), rng.uniform(-0.2, 0.2),
                       rng.uniform(0.9, 1.1), w / 2, h / 2)
        m[2, :2] = rng.uniform(-8e-4, 8e-4, 2)
        out.append(m)
    out.append(_translation(3, -2))
    out.append(_translation(0.5, 0.25))
    return [np.asarray(m, dtype=np.float32) for m in out]


@pytest.mark.parametrize("interp,subpix", [("bilinear", "q5"), ("bilinear", "exact"), ("bicubic", "q5")])
def test_valid_pixels_do_not_see_the_border(oracle, interp, subpix):
    sw, sh, dw, dh = 83, 47, 97, 61                 # output wider than one 64-column block, not a multiple of anything
    rng = np.random.default_rng(3)
    src = rng.uniform(0.0, 1.0, (sh, sw, 3)).astype(np.float32)
    seen_valid = seen_invalid = 0
    for m in _drawn_matrices(sw, sh, seed=17):
        valid = R.valid_map(m, (sw, sh), (dw, dh), interp, subpix)
        a, _ = oracle.warp_frame(src, m, (dw, dh), interp=interp, border=(0.0, 0.0, 0.0), subpix=subpix)
        b, _ = oracle.warp_frame(src, m, (dw, dh), interp=interp, border=(1.0, 1.0, 1.0), subpix=subpix)
        same = (a.view(np.uint32) == b.view(np.uint32)).all(axis=2)
        assert same[valid].all(), f"{int((~same & valid).sum())} valid pixels depend on the border colour"
        seen_valid += int(valid.sum())
        seen_invalid += int((~valid).sum())
    assert seen_valid > 10000 and seen_invalid > 10000


def test_integer_translation_returns_texture_bits_on_interior_rule(oracle):
    """The GPU known-answer test's premise: under an integer translation the warp of a window returns the texture's bits
    at every pixel of the interior rule (weights 1, 0, 0, 0), none excluded."""
    rng = np.random.default_rng(9)
    tex = rng.uniform(0.0, 1.0, (40, 60, 3)).astype(np.float32)
    m = _translation(7, -4)
    out, _ = oracle.warp_frame(tex, m, (60, 40))
    valid = R.valid_map(m, (60, 40), (60, 40))
    ys, xs = np.nonzero(valid)
    assert valid.mean() > 0.7
    assert np.array_equal(out[ys, xs].view(np.uint32), tex[ys + 4, xs - 7].view(np.uint32))


def test_restatement_fill_order_and_untouched(oracle):
    rng = np.random.default_rng(21)
    src = rng.uniform(0, 1, (3, 20, 30, 3)).astype(np.float32)
    dst = rng.uniform(0, 1, (1, 20, 30, 3)).astype(np.float32)
    mask = np.zeros((1, 20, 30), np.float32)
    mask[0, :, :6] = 1.0
    mats = np.stack([_translation(40, 0), _translation(3, 0), _translation(2, 0)])[None]   # k=0 far outside, k=1 covers x >= 3
    d2, m2, ff, fc, pc = R.temporal_fill(src, mats, [[0, 1, 2]], dst, mask)
    assert np.array_equal(d2[0, :, 6:], dst[0, :, 6:]) and (ff[0, :, 6:] == -1).all()
    assert (ff[0, :19, 3:6] == 1).all() and (ff[0, :19, 2] == 2).all() and (ff[0, :, :2] == -1).all()
    assert np.array_equal(d2[0, :19, 3:6], src[1, :19, 0:3])
    assert fc[0] == 19 * 4 and pc[0] == 20 * 6 - 19 * 4 and (m2[0] == 1.0).sum() == pc[0]


# ---- public surface ------------------------------------------------------------------------------------------------------
def test_node_list_and_schema(pkg):
    from vstab_amd import nodes

    assert len(nodes.NODE_CLASSES) == 6 and nodes.VideoStabilizerTemporalFill not in nodes.NODE_CLASSES
    listed = asyncio.run(nodes.VideoStabilizerAmdExtension().get_node_list())
    assert len(listed) == 7 and listed[:6] == nodes.NODE_CLASSES and listed[6] is nodes.VideoStabilizerTemporalFill
    schema = nodes.VideoStabilizerTemporalFill.define_schema()
    assert schema.node_id == "video_stabilizer_temporal_fill"
    assert schema.display_name == "Video Stabilizer Temporal Fill"
    assert [s.id for s in schema.inputs] == ["frames", "frames_stabilized", "padding_mask", "meta", "radius", "interpolation"]
    assert [s.id for s in schema.outputs] == ["frames", "padding_mask", "meta"]
    def opt(sock, key):   # the stand-in sockets keep their options in a dict, ComfyUI's as attributes
        return sock.options[key] if isinstance(getattr(sock, "options", None), dict) else getattr(sock, key)

    radius = schema.inputs[4]
    assert (opt(radius, "default"), opt(radius, "min"), opt(radius, "max")) == (8, 1, 32)
    assert list(opt(schema.inputs[5], "options")) == ["bilinear", "bicubic"]


def test_meta_without_transitions_is_refused(pkg):
    from vstab_amd import temporal_fill as tf

    eye = np.eye(3).tolist()
    warp = {"source_size": [8, 8], "output_size": [8, 8], "per_frame": [{"index": i, "applied_matrix": eye} for i in range(3)]}
    with pytest.raises(ValueError, match="estimated_motion"):
        tf.plan_from_meta({"stabilization_warp": warp})                 # Motion Apply's meta: no transitions
    with pytest.raises(ValueError, match="stabilization_warp"):
        tf.plan_from_meta({"estimated_motion": {"per_transition": []}})
    with pytest.raises(ValueError, match="per_transition"):
        tf.plan_from_meta({"stabilization_warp": warp, "estimated_motion": {"per_transition": []}})   # bypass: none recorded
    per = [{"index": i, "mode": "similarity", "confidence": 0.5, "matrix": eye} for i in range(2)]
    plan = tf.plan_from_meta({"stabilization_warp": warp, "estimated_motion": {"per_transition": per}})
    assert plan["final_matrices"].shape == (3, 3, 3) and plan["transitions"].shape == (2, 3, 3)
    assert plan["source_size"] == (8, 8) and plan["output_size"] == (8, 8)


def test_keyword_and_sharded_rejection(pkg):
    import inspect

    from vstab_amd import distributed, flow_pipeline

    p = inspect.signature(flow_pipeline._stabilize_frames).parameters["temporal_fill"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0
    assert inspect.signature(distributed.stabilize_sharded).parameters["temporal_fill"].default == 0


def test_header_declares_what_native_binds(pkg):
    from vstab_amd import native

    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "vstab.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+vstab_temporal_fill_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/vstab.h does not declare vstab_temporal_fill_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = native._SIGNATURES["vstab_temporal_fill_batch"]
    assert len(params) == len(args) == 19
    import ctypes as C
    for ptxt, a in zip(params, args):
        assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
    assert "vstab_temporal_fill_batch" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load_library(), "vstab_temporal_fill_batch")
    assert hasattr(native.Context, "temporal_fill_batch")
