"""Mesh warp, the parts that need no GPU: the request checks and their ValueErrors, the host plan (vertex paths), the NumPy
restatements of both rules on cases with a known answer -- the warp restatement at zero offsets against the oracle's warp,
bit for bit -- and the public surface (keywords, exports, header, node)."""

import asyncio
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import mesh_restatement as R
from tests import util
from tests.test_distributed_cpu import NumpyTrajectoryCtx

ROOT = Path(__file__).resolve().parents[1]
ARGS = ("crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
TRAJ = NumpyTrajectoryCtx().trajectory


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _context(pkg, n=4, h=24, w=32):
    import torch

    from vstab_amd import host_math as hm

    return hm._normalize_video_input(torch.zeros((n, h, w, 3)))


# ---- request validation ------------------------------------------------------------------------------------------------
def test_request_forms(pkg):
    from vstab_amd import mesh_warp as mw

    assert mw.check_request(None) is None and mw.check_request(None, 3.0) is None
    r = mw.check_request(True)
    assert (r.cols, r.rows, r.vertices, r.max_shift) == (16, 9, (17, 10), None)
    assert r.max_shift_px(1920) == 30.0 and r.max_shift_px(480) == 7.5          # 1/64 of the width
    r = mw.check_request((2, 64), 4)
    assert (r.cols, r.rows, r.vertices) == (2, 64, (3, 65)) and r.max_shift == 4.0 and r.max_shift_px(1920) == 4.0
    assert mw.check_request([8, np.int64(5)]).vertices == (9, 6)


@pytest.mark.parametrize("value,text", [
    (False, r"mesh_warp=False: expected None, True or a \(cols, rows\) pair"),
    ("yes", r"mesh_warp='yes': expected None, True"),
    (16, r"mesh_warp=16: expected None, True"),
    ((16,), r"mesh_warp=\(16,\): expected None, True"),
    ((16, 9, 2), r"mesh_warp=\(16, 9, 2\): expected None, True"),
    ((16.0, 9), r"mesh_warp=\(16.0, 9\): expected None, True"),
    ((True, 9), r"mesh_warp=\(True, 9\): expected None, True"),
    ((1, 9), r"mesh_warp=\(1, 9\): cols and rows must lie in \[2, 64\]"),
    ((16, 65), r"mesh_warp=\(16, 65\): cols and rows must lie in \[2, 64\]"),
    ((0, -3), r"mesh_warp=\(0, -3\): cols and rows must lie in \[2, 64\]"),
])
def test_bad_mesh_warp_names_the_value(pkg, value, text):
    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError, match=text):
        fp._stabilize_frames(_context(pkg), *ARGS, mesh_warp=value)


@pytest.mark.parametrize("value", [0, 0.0, -2.0, float("nan"), float("inf"), "8", True])
def test_bad_max_shift_names_the_value(pkg, value):
    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError, match=r"mesh_max_shift=.*expected a finite number above 0"):
        fp._stabilize_frames(_context(pkg), *ARGS, mesh_warp=True, mesh_max_shift=value)


def test_unsupported_combinations_name_the_reason(pkg):
    from vstab_amd import distributed
    from vstab_amd import flow_pipeline as fp

    rest = ARGS[1:]
    with pytest.raises(ValueError, match=r"estimator 'classic'.*no dense grid"):
        fp._stabilize_frames(_context(pkg), *ARGS, mesh_warp=True, estimator="classic")
    with pytest.raises(ValueError, match=r"estimator 'flow_phase_correlate'.*no dense grid"):
        fp._stabilize_frames(_context(pkg), *ARGS, mesh_warp=True, estimator="flow_phase_correlate")
    with pytest.raises(ValueError, match=r"framing_mode 'crop': the crop solver bounds matrices only"):
        fp._stabilize_frames(_context(pkg), "crop", *rest, mesh_warp=(4, 4))
    with pytest.raises(ValueError, match=r"temporal_fill=2: fill candidates are global matrices"):
        fp._stabilize_frames(_context(pkg), *ARGS, mesh_warp=True, temporal_fill=2)
    with pytest.raises(ValueError, match="the mesh warp is not sharded"):
        distributed.stabilize_sharded(None, None, 4, *ARGS, mesh_warp=True)


def test_bypasses_ignore_the_keyword(pkg):
    """0 / 1 frames: returned before any GPU work, with the reference's meta (no mesh_warp key)."""
    import dataclasses

    from vstab_amd import flow_pipeline as fp

    for n in (0, 1):
        def make():
            return _context(pkg, n=n) if n else dataclasses.replace(_context(pkg, n=1), frames=[], batch=None)

        without = fp._stabilize_frames(make(), *ARGS)
        got = fp._stabilize_frames(make(), *ARGS, mesh_warp=True, mesh_max_shift=3.0)
        assert got.meta == without.meta and "mesh_warp" not in got.meta


# ---- the host plan ---------------------------------------------------------------------------------------------------
def _plan(pkg, residual, conf=None, segments=None, lock=True, scale=(2.0, 2.0), max_shift=1e9, smooth=0.5, strength=1.0):
    from vstab_amd import mesh_warp as mw

    pairs = residual.shape[0]
    conf = np.ones(pairs) if conf is None else conf
    return mw.plan_offsets(TRAJ, residual, conf, segments, smooth, 16.0, strength, lock, scale, max_shift)


def test_zero_residuals_give_zero_offsets(pkg):
    for lock in (True, False):
        off, path = _plan(pkg, np.zeros((7, 4, 5, 2), np.float32), lock=lock)
        assert off.shape == (8, 4, 5, 2) and off.dtype == np.float32 and not off.any() and not path.any()


def test_constant_residual_under_camera_lock_is_minus_the_path(pkg):
    """r_i(v) = d for every pair and vertex: P_i = i * d, the locked target is 0, so c_i = -P_i (times the up-scale)."""
    d = np.array([0.25, -0.5], np.float32)
    res = np.tile(d, (6, 3, 4, 1))
    off, path = _plan(pkg, res, scale=(2.0, 4.0))
    for i in range(7):
        assert np.array_equal(path[i], np.tile(i * d.astype(np.float64), (3, 4, 1)))
        assert np.array_equal(off[i], np.tile(np.float32([-i * 0.25 * 2.0, i * 0.5 * 4.0]), (3, 4, 1)))
    # without the lock a constant-velocity path is its own moving average away from the clip's ends: no correction there
    off, _ = _plan(pkg, np.tile(d, (40, 3, 4, 1)), lock=False)
    assert np.abs(off[12:28]).max() < 1e-6 and np.abs(off[0]).max() > 0.1


def test_paths_restart_at_cuts_and_skip_confidence_zero(pkg):
    d = np.float32([1.0, 2.0])
    res = np.tile(d, (7, 3, 3, 1))
    conf = np.ones(7)
    conf[2] = 0.0                                            # a failed fit: that pair contributes nothing
    _, path = _plan(pkg, res, conf=conf)
    assert [float(path[i, 1, 1, 0]) for i in range(8)] == [0, 1, 2, 2, 3, 4, 5, 6]
    # a cut in front of frame 5: the pair (4, 5) is a confidence-0 record and frame 5 starts a new path
    conf = np.ones(7)
    conf[4] = 0.0
    off, path = _plan(pkg, res, conf=conf, segments=[(0, 5), (5, 8)], scale=(1.0, 1.0))
    assert [float(path[i, 0, 2, 1]) for i in range(8)] == [0, 2, 4, 6, 8, 0, 2, 4]
    assert not off[0].any() and not off[5].any() and off[4].any() and off[6].any()
    # a one-frame shot has no path of its own
    _, path = _plan(pkg, res, conf=conf, segments=[(0, 5), (5, 6), (6, 8)])
    assert not path[5].any() and not path[6].any() and path[7].any()


def test_the_clamp_is_per_axis_in_full_resolution_px(pkg):
    res = np.tile(np.float32([1.0, -0.125]), (9, 2, 2, 1))
    off, _ = _plan(pkg, res, scale=(2.0, 2.0), max_shift=5.0)
    want_x = -np.minimum(np.arange(10) * 2.0, 5.0)
    want_y = np.minimum(np.arange(10) * 0.25, 5.0)
    assert np.array_equal(off[:, 0, 0, 0], want_x.astype(np.float32)) and np.array_equal(off[:, 1, 1, 1], want_y.astype(np.float32))
    assert np.abs(off).max() == 5.0


def test_vertex_median_removes_an_outlier_vertex(pkg):
    from vstab_amd import mesh_warp as mw

    res = np.full((1, 5, 6, 2), 0.5, np.float32)
    res[0, 2, 3] = (40.0, -40.0)
    res[0, 0, 0] = (9.0, 9.0)                                # a corner: it sees itself four times of nine, still a minority
    out = mw.vertex_median3(res)
    assert out.dtype == np.float32 and np.array_equal(out, np.full_like(res, 0.5))


def test_meta_block(pkg):
    from vstab_amd import mesh_warp as mw

    res = np.zeros((2, 2, 2, 2), np.float32); res[0, 0, 0] = (3.0, -4.0)
    off = np.zeros((3, 2, 2, 2), np.float32); off[2, 1, 1] = (-2.0, 1.0)
    cnt = np.full((2, 2, 2), 10); cnt[1, 0, 1] = 3; cnt[0, 1, 1] = 0
    assert mw.meta_block(mw.check_request((4, 3)), 7.5, res, cnt, off, 4) == {
        "cells": [4, 3], "max_shift": 7.5, "residual_px_mean": 7.0 / 16, "residual_px_max": 4.0, "correction_px_mean": 3.0 / 24,
        "correction_px_max": 2.0, "vertices_without_samples": 2}


# ---- the warp restatement is the oracle's warp at zero offsets ------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("kind", ["similarity", "perspective", "far", "horizon", "identity"])
def test_warp_restatement_at_zero_offsets_is_the_oracle_warp(oracle, subpix, kind):
    cases = [((61, 45), (61, 45)), ((61, 45), (75, 52)), ((40, 33), (1100, 20))]      # (w, h) source, output; the last spans
    for k, (src_size, out_size) in enumerate(cases):                                    # two OpenCV column blocks
        sw, sh = src_size
        src = util.synth_frames(1, sh, sw, seed=10 + k)[0]
        m = util.test_matrices(1, sw, sh, kind, seed=20 + k)[0].astype(np.float32)
        border = (0.25, 0.5, 0.75)
        want, cov = oracle.warp_frame(src, m, out_size, interp="bilinear", border=border, subpix=subpix)
        mask = np.float32(1.0) - (cov > 0.5).astype(np.float32)
        for verts in ((2, 2), (17, 10)):
            got, got_mask = R.mesh_warp_frame(src, m, out_size, np.zeros((verts[1], verts[0], 2), np.float32), border, subpix)
            assert np.array_equal(_bits(got), _bits(want)), (kind, subpix, src_size, out_size)
            assert np.array_equal(got_mask, mask)


def test_warp_restatement_known_answer_integer_shift():
    """Identity matrix, the same integer offset at every vertex: content moves by +offset, border colour and mask 1 behind it."""
    src = util.synth_frames(1, 20, 30, seed=3)[0]
    off = np.tile(np.float32([3.0, -2.0]), (4, 5, 1))
    for subpix in ("q5", "exact"):
        got, mask = R.mesh_warp_frame(src, np.eye(3, dtype=np.float32), (30, 20), off, (0.1, 0.2, 0.3), subpix)
        assert np.array_equal(got[:18, 3:], src[2:, :27]) and np.array_equal(mask[:18, 3:], np.zeros((18, 27), np.float32))
        assert np.array_equal(got[18:], np.tile(np.float32([0.1, 0.2, 0.3]), (2, 30, 1))) and (mask[18:] == 1).all()
        assert np.array_equal(got[:, :3], np.tile(np.float32([0.1, 0.2, 0.3]), (20, 3, 1))) and (mask[:, :3] == 1).all()


def test_displacement_interpolates_the_four_vertices_of_the_cell():
    off = np.zeros((3, 3, 2), np.float32)
    off[1, 1] = (4.0, -8.0)                                  # the centre vertex of a 41 x 21 frame sits at (20, 10)
    q = np.array([20.0, 10.0, 30.0, 0.0, -50.0, np.nan, 1e9])
    cx, cy = R.displacement(q, np.full_like(q, 10.0), off, (41, 21))
    assert cx.tolist() == [4.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0] and cy.tolist() == [-8.0, -4.0, -4.0, 0.0, 0.0, 0.0, 0.0]
    cx, _ = R.displacement(np.full(3, 20.0), np.array([5.0, 15.0, 400.0]), off, (41, 21))
    assert cx.tolist() == [2.0, 2.0, 0.0]


# ---- the residual restatement ----------------------------------------------------------------------------------------------
def _quadrant_field(w, h, step, A, d):
    gh, gw = -(-h // step), -(-w // step)
    x = (np.arange(gw) * step).astype(np.float64)[None, :].repeat(gh, 0)
    y = (np.arange(gh) * step).astype(np.float64)[:, None].repeat(gw, 1)
    W = A[2, 0] * x + A[2, 1] * y + A[2, 2]
    ax, ay = (A[0, 0] * x + A[0, 1] * y + A[0, 2]) / W, (A[1, 0] * x + A[1, 1] * y + A[1, 2]) / W
    quad = (x >= w / 2).astype(int) + 2 * (y >= h / 2).astype(int)
    flow = np.stack([ax - x + d[quad, 0], ay - y + d[quad, 1]], axis=-1).astype(np.float32)
    return flow[None], x, y


@pytest.mark.parametrize("kind", ["translation", "similarity", "perspective"])
def test_residual_restatement_returns_the_quadrant_constants(kind):
    """flow = A(x) - x + d with d constant per quadrant: every vertex whose four cells lie inside one quadrant reports d."""
    w, h, step, mw, mh = 320, 176, 8, 9, 7
    d = np.array([[0.5, -0.25], [-1.0, 0.75], [2.0, 1.5], [-0.5, -2.25]])
    A = np.array([[1, 0, 3.0], [0, 1, -2.0], [0, 0, 1.0]]) if kind == "translation" else util.test_matrices(1, w, h, kind, seed=5)[0]
    A32 = A.astype(np.float32)
    flow, _, _ = _quadrant_field(w, h, step, A32.astype(np.float64), d)
    res, cnt = R.mesh_residual(flow, step, (w, h), A32[None], mw, mh)
    cw, ch = (w - 1) / (mw - 1), (h - 1) / (mh - 1)
    checked = 0
    for b in range(mh):
        for a in range(mw):
            vx, vy = a * cw, b * ch
            qx = {int(max(vx - cw, 0) >= w / 2), int(min(vx + cw, w - 1) >= w / 2)}
            qy = {int(max(vy - ch, 0) >= h / 2), int(min(vy + ch, h - 1) >= h / 2)}
            if len(qx) != 1 or len(qy) != 1:
                continue
            want = d[qx.pop() + 2 * qy.pop()]
            assert cnt[0, b, a] >= R.MIN_SAMPLES
            if kind == "translation":      # integer shift + quarter-px constants: every operation of the rule is exact
                assert res[0, b, a].tolist() == want.tolist()
            else:                          # the float32 flow carries half an ulp of |u| < 64: 4e-6
                assert np.abs(res[0, b, a] - want).max() < 1e-4
            checked += 1
    assert checked >= 12


def test_residual_restatement_admission_rules():
    w, h, step, mw, mh = 64, 48, 8, 3, 3
    gh, gw = 6, 8
    flow = np.zeros((1, gh, gw, 2), np.float32)
    flow[0, ..., 0] = 1.0
    eye = np.eye(3, dtype=np.float32)[None]
    res, cnt = R.mesh_residual(flow, step, (w, h), eye, mw, mh)
    # vertex (0, 0): |x| < 31.5 and |y| < 23.5 -> x in {0, 8, 16, 24}, y in {0, 8, 16}: 12 samples; the centre vertex sees
    # |x - 31.5| < 31.5 -> x = 8..56 (7) and |y - 23.5| < 23.5 -> y = 8..40 (5)
    assert cnt[0, 0, 0] == 12 and cnt[0, 1, 1] == 35 and (res[0, ..., 0] == 1.0).all() and not res[0, ..., 1].any()
    # NaN / Inf samples and blocked samples (either frame of the pair) leave; below MIN_SAMPLES the vertex reports 0
    flow[0, 0, 0, 1] = np.nan
    flow[0, 1, 1, 0] = np.inf
    blocked = np.zeros((2, gh, gw), np.uint8)
    blocked[0, 2, 0] = 1
    blocked[1, 2, 1] = 1
    _, cnt2 = R.mesh_residual(flow, step, (w, h), eye, mw, mh, blocked)
    assert cnt2[0, 0, 0] == 8
    blocked[:, :3, :4] = 1
    blocked[0, 0, 1] = blocked[1, 0, 1] = 0
    res3, cnt3 = R.mesh_residual(flow, step, (w, h), eye, mw, mh, blocked)
    assert cnt3[0, 0, 0] == 1 and res3[0, 0, 0].tolist() == [0.0, 0.0]
    # an even count takes the float32 mean of the two middle values
    flow = np.zeros((1, gh, gw, 2), np.float32)
    flow[0, :3, :4, 0] = np.arange(12, dtype=np.float32).reshape(3, 4)
    res4, _ = R.mesh_residual(flow, step, (w, h), eye, mw, mh)
    assert res4[0, 0, 0, 0] == 5.5


# ---- public surface -------------------------------------------------------------------------------------------------------
def test_keywords_and_exports(pkg):
    from vstab_amd import distributed, flow_pipeline, native

    sig = inspect.signature(flow_pipeline._stabilize_frames).parameters
    for name in ("mesh_warp", "mesh_max_shift"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None
    assert inspect.signature(distributed.stabilize_sharded).parameters["mesh_warp"].default is None
    for name in ("vstab_mesh_residual_batch", "vstab_mesh_warp_batch"):
        assert name in native.EXPORTED_SYMBOLS
    assert list(inspect.signature(native.Context.mesh_residual_batch).parameters)[1:] == [
        "grid_flow", "step", "work_size", "transitions", "mw", "mh", "blocked"]
    assert list(inspect.signature(native.Context.mesh_warp_batch).parameters)[1:5] == ["frames", "matrices", "out_size", "offsets"]
    for est in (flow_pipeline.estimate_transitions, flow_pipeline.estimate_transitions_tvl1):
        assert inspect.signature(est).parameters["grid_out"].default is None
    assert native.MESH_MIN_SAMPLES == R.MIN_SAMPLES


def test_header_states_both_rules_once():
    text = (ROOT / "include" / "vstab.h").read_text()
    flat = re.sub(r"\s+", " ", text)
    assert ("int vstab_mesh_residual_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h, "
            "int work_w, const float* transitions, const uint8_t* blocked, int mw, int mh, float* residual, int32_t* count);") in flat
    assert ("int vstab_mesh_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices, "
            "int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw, int mh, float* dst, "
            "float* mask, uint32_t* pad_count);") in flat
    assert text.count("---- mesh warp") == 1 and f"#define VSTAB_MESH_MIN_SAMPLES {R.MIN_SAMPLES}" in text
    block = flat[flat.index("---- mesh warp"):flat.index("int vstab_mesh_warp_batch(")]
    for phrase in ("(A0*x + A1*y) + A2", "numpy.median", "(lo + hi) / 2 in float32", "|x - vx| < cw", "blocked neither in frame i",
                   "s = q - c(q)", "|c| * |grad c|", "bit-identical to vstab_warp_batch", "Xn*Wq - 32.0*cx", 'timing kind "mesh_residual"',
                   'Timing kind "mesh_warp"', "a NaN becomes 0"):
        assert phrase in block, phrase
    makefile = (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert "vstab_mesh.hip" in makefile and (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "vstab_mesh.hip").exists()


def test_mesh_node_schema(pkg):
    from vstab_amd import nodes

    assert len(nodes.NODE_CLASSES) == 6 and nodes.VideoStabilizerFlowMesh not in nodes.NODE_CLASSES
    listed = asyncio.run(nodes.VideoStabilizerAmdMeshExtension().get_node_list())
    assert len(listed) == 10 and listed[9] is nodes.VideoStabilizerFlowMesh
    assert listed[:9] == asyncio.run(nodes.VideoStabilizerAmdScenesExtension().get_node_list())
    assert issubclass(nodes.VideoStabilizerAmdMeshExtension, nodes.VideoStabilizerAmdScenesExtension)
    s = nodes.VideoStabilizerFlowMesh.define_schema()
    flow = nodes.VideoStabilizerFlow.define_schema()
    assert s.node_id == "video_stabilizer_flow_mesh" and s.display_name == "Video Stabilizer Flow (Mesh)"
    assert [i.id for i in s.inputs] == [i.id for i in flow.inputs] + ["mesh_cols", "mesh_rows", "max_shift"]
    assert [o.id for o in s.outputs] == [o.id for o in flow.outputs]
    cols, rows, shift = s.inputs[-3:]
    assert (cols.options["default"], rows.options["default"], shift.options["default"]) == (16, 9, 0.0)
    assert (cols.options["min"], cols.options["max"], rows.options["min"], rows.options["max"]) == (2, 64, 2, 64)
    assert list(inspect.signature(nodes.VideoStabilizerFlowMesh.execute).parameters) == \
        list(inspect.signature(nodes.VideoStabilizerFlow.execute).parameters) + ["mesh_cols", "mesh_rows", "max_shift"]


def test_library_trajectory_takes_the_vertex_columns(pkg):
    """vstab_trajectory on 2 * 17 * 10 columns (host arithmetic, no GPU): every column equals the same call on that column alone."""
    import ctypes as C

    from vstab_amd import native

    lib = native.load_library()
    rng = np.random.default_rng(4)
    n, p = 30, 340
    d = np.ascontiguousarray(rng.normal(0, 1, (n - 1, p)))
    path, target = np.zeros((n, p)), np.zeros((n, p))
    assert lib.vstab_trajectory(None, d.ctypes.data, n, p, C.c_double(0.5), C.c_double(16.0), C.c_double(0.8), 0, path.ctypes.data,
                                target.ctypes.data) == 0
    for c in (0, 7, 8, 339):
        dc = np.ascontiguousarray(d[:, c:c + 1])
        p1, t1 = np.zeros((n, 1)), np.zeros((n, 1))
        assert lib.vstab_trajectory(None, dc.ctypes.data, n, 1, C.c_double(0.5), C.c_double(16.0), C.c_double(0.8), 0, p1.ctypes.data,
                                    t1.ctypes.data) == 0
        assert np.array_equal(p1[:, 0], path[:, c]) and np.array_equal(t1[:, 0], target[:, c])
    want_path, want_target = TRAJ(d, 0.5, 16.0, 0.8, False)
    assert np.allclose(path, want_path, atol=1e-12) and np.allclose(target, want_target, atol=1e-9)
