"""Rolling shutter, the parts that need no GPU: the request checks and their ValueErrors, the per-frame velocities, the readout
estimate on analytic rolling flows, the meta block, the restatement's known answers and the public surface (keywords,
exports, header, documents, node).

The readout cases: analytic rolling flows (tests/rolling_shutter_restatement.rolling_flow_grid: the exact flow a rolling pair
shows, Gaussian noise of 0.05 px on top), least-squares translation / similarity fits, the row medians of the restatement,
rolling_shutter.estimate_readout.  2 fits x 3 readouts x 3 sizes x 3 seeds = 54 cases; the condition is the issue's,
|rho_hat - rho| <= 0.05.  Measured here (tools/rolling_shutter_report.py --cpu, profiles/r20_rolling_shutter.md): worst 0.0230.
The camera of these cases is slow against the frame rate on purpose -- its components have angular frequencies of at most
0.35 rad per frame: the estimator is first order in time, it forms velocities as finite differences of the transitions, which
see a component of angular frequency o reduced by sin(o) / o (1.5 % at 0.3, 4 % at 0.5, 16 % at 1), and reports a readout
too large by that factor.  DESIGN 8k says so; a faster shake is outside what these cases claim.
"""

import asyncio
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import rolling_shutter_restatement as R
from tests import util

ROOT = Path(__file__).resolve().parents[1]
ARGS = ("crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)

FIT_MODES = ("translation", "similarity")
READOUTS = (0.7, -0.4, 1.0)
SIZES = ((960, 540), (540, 960), (200, 120))
SEEDS = (0, 1, 2)
READOUT_TOLERANCE = 0.05
CLIP_FRAMES = 12


def _context(pkg, n=4, h=24, w=32):
    import torch

    from vstab_amd import host_math as hm

    return hm._normalize_video_input(torch.zeros((n, h, w, 3)))


# ---- request validation ------------------------------------------------------------------------------------------------
def test_request_forms(pkg):
    from vstab_amd import rolling_shutter as rs

    for off in (None, 0, 0.0, -0.0, np.float32(0.0), np.int64(0)):
        assert rs.check_request(off) is None
    assert rs.check_request("auto") == "auto"
    for value in (0.7, -1, 1.0, np.float64(-0.25), np.float32(0.5)):
        got = rs.check_request(value)
        assert isinstance(got, float) and got == float(value)


@pytest.mark.parametrize("value", [True, False, "AUTO", "0.7", 1.5, -1.0001, float("nan"), float("inf"), (0.7,), [0.5], 1 + 0j])
def test_bad_request_names_the_value(pkg, value):
    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError, match=re.escape(f"rolling_shutter={value!r}: expected None, 0, 'auto' or a finite readout in [-1, 1]")):
        fp._stabilize_frames(_context(pkg), *ARGS, rolling_shutter=value)


def test_unsupported_combinations_name_the_reason(pkg):
    """Every refusal comes before any GPU work: nothing below reaches for a GPU, so the test passes without one."""
    from vstab_amd import distributed
    from vstab_amd import flow_pipeline as fp

    rest = ARGS[2:]
    cases = [
        (("crop_and_pad", "perspective"), {}, r"transform_mode 'perspective': the image velocity of a perspective transition is not affine"),
        (("crop", "similarity"), {}, r"framing_mode 'crop': the crop solver bounds matrices only"),
        (ARGS[:2], dict(mesh_warp=True), r"mesh_warp: the warp takes one displacement"),
        (ARGS[:2], dict(temporal_fill=2), r"temporal_fill=2: fill candidates are neighbour frames that have not been corrected"),
        (ARGS[:2], dict(sharpness_transfer=3), r"sharpness_transfer: its candidates are neighbour frames that have not been corrected"),
        (ARGS[:2], dict(dynamic_zoom=True), r"dynamic_zoom: its coverage-extent kernel does not know the per-row displacement"),
        (("crop_and_pad", "translation"), dict(estimator="subject", subject_mask=np.zeros((4, 24, 32), np.float32)),
         r"estimator 'subject': its transitions are the subject's, not the camera's"),
    ]
    for value in (0.5, "auto"):
        for head, kw, text in cases:
            with pytest.raises(ValueError, match=text):
                fp._stabilize_frames(_context(pkg), *head, *rest, rolling_shutter=value, **kw)
    for estimator in ("classic", "flow_phase_correlate"):
        with pytest.raises(ValueError, match=rf"rolling_shutter='auto' is not supported with estimator '{estimator}'.*no grid of flow samples"):
            fp._stabilize_frames(_context(pkg), *ARGS, rolling_shutter="auto", estimator=estimator)
    with pytest.raises(ValueError, match="rolling_shutter=0.5: the rolling-shutter correction is not sharded"):
        distributed.stabilize_sharded(None, None, 4, *ARGS, rolling_shutter=0.5)
    with pytest.raises(ValueError, match="rolling_shutter='auto': the rolling-shutter correction is not sharded"):
        distributed.stabilize_sharded(None, None, 4, *ARGS, rolling_shutter="auto")


def test_check_pipeline_alone(pkg):
    from vstab_amd import rolling_shutter as rs

    rs.check_pipeline(0.5, "similarity", "expand", "classic")
    rs.check_pipeline("auto", "translation", "crop_and_pad", "flow_tvl1")
    rs.check_pipeline(0.5, "translation", "crop_and_pad", "flow_phase_correlate")
    with pytest.raises(ValueError, match="not affine"):
        rs.check_pipeline(0.5, "perspective", "expand", "flow")


def test_bypasses_ignore_the_keyword(pkg):
    """0 / 1 frames: returned before any GPU work, with the reference's meta (no rolling_shutter key)."""
    import dataclasses

    from vstab_amd import flow_pipeline as fp

    for n in (0, 1):
        def make():
            return _context(pkg, n=n) if n else dataclasses.replace(_context(pkg, n=1), frames=[], batch=None)

        without = fp._stabilize_frames(make(), *ARGS)
        for value in (0.7, "auto"):
            got = fp._stabilize_frames(make(), *ARGS, rolling_shutter=value)
            assert got.meta == without.meta and "rolling_shutter" not in got.meta


# ---- the public surface --------------------------------------------------------------------------------------------------
def test_keyword_defaults(pkg):
    from vstab_amd import distributed
    from vstab_amd import flow_pipeline as fp

    p = inspect.signature(fp._stabilize_frames).parameters["rolling_shutter"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(distributed.stabilize_sharded).parameters["rolling_shutter"].default is None


def test_symbols_in_header_exports_and_documents(pkg):
    from vstab_amd import native

    header = (ROOT / "include" / "vstab.h").read_text()
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in ("vstab_rolling_warp_batch", "vstab_row_residual_batch"):
        assert name in native.EXPORTED_SYMBOLS
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in integration
    assert re.search(r"^#define VSTAB_ROW_MIN_SAMPLES 8$", header, re.M)
    assert re.search(r"^#define VSTAB_ABI_VERSION 1$", header, re.M)
    assert "vstab_rolling.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert callable(native.Context.rolling_warp_batch) and callable(native.Context.row_residual_batch)
    sig = inspect.signature(native.Context.rolling_warp_batch).parameters
    assert list(sig)[1:6] == ["frames", "matrices", "out_size", "velocity", "readout"]
    assert sig["subpix"].default is None and sig["want_mask"].default is True and sig["want_count"].default is True
    assert list(inspect.signature(native.Context.row_residual_batch).parameters)[1:] == ["grid_flow", "step", "work_size", "transitions", "blocked"]
    for doc, words in (("README.md", ("rolling_shutter", "Cost:", "video_stabilizer_flow_rolling")), ("DESIGN.md", ("8k", "rolling")),
                       ("INTEGRATION.md", ("VideoStabilizerAmdRollingExtension",))):
        text = (ROOT / doc).read_text()
        for word in words:
            assert word in text, (doc, word)


def test_constants_agree(pkg):
    from vstab_amd import rolling_shutter as rs

    assert rs.ROW_MIN_SAMPLES == R.MIN_SAMPLES == 8 and rs.ROW_MIN_RMS_PX == 0.05 and rs.VERSION == 1


def test_node_sockets_and_where_it_is_listed(pkg):
    from vstab_amd import nodes

    schema = nodes.VideoStabilizerFlowRolling.define_schema()
    flow = nodes.VideoStabilizerFlow.define_schema()
    assert schema.node_id == "video_stabilizer_flow_rolling" and schema.display_name == "Video Stabilizer Flow (Rolling Shutter)"
    assert [s.id for s in schema.inputs] == [s.id for s in flow.inputs] + ["readout"]
    assert [s.id for s in schema.outputs] == [s.id for s in flow.outputs]
    by_id = {s.id: s for s in schema.inputs}
    mode = by_id["transform_mode"].options
    assert list(mode["options"]) == ["translation", "similarity"] and mode["default"] == "similarity"
    readout = by_id["readout"]
    assert readout.kind == "Float" and (readout.options["default"], readout.options["min"], readout.options["max"]) == (0.0, -1.0, 1.0)
    for other in flow.inputs:
        if other.id != "transform_mode":
            assert by_id[other.id].kind == other.kind and by_id[other.id].options == other.options
    assert nodes.VideoStabilizerFlowRolling not in nodes.NODE_CLASSES
    listed = asyncio.run(nodes.VideoStabilizerAmdRollingExtension().get_node_list())
    before = asyncio.run(nodes.VideoStabilizerAmdHandoffExtension().get_node_list())
    assert listed == before + [nodes.VideoStabilizerFlowRolling] and nodes.VideoStabilizerFlowRolling not in before
    assert issubclass(nodes.VideoStabilizerAmdRollingExtension, nodes.VideoStabilizerAmdHandoffExtension)
    assert list(inspect.signature(nodes.VideoStabilizerFlowRolling.execute).parameters)[-1] == "readout"


# ---- velocities ------------------------------------------------------------------------------------------------------------
def _transitions(n, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([util.similarity(rng.uniform(-6, 6), rng.uniform(-4, 4), rng.uniform(-0.01, 0.01), rng.uniform(0.99, 1.01), 240, 135)
                     for _ in range(n - 1)])


def _forward(A):
    return (A - np.eye(3))[:2].reshape(6)


def _backward(A):
    return (np.eye(3) - np.linalg.inv(A))[:2].reshape(6)


def test_velocities_at_the_ends_gaps_and_cuts(pkg):
    from vstab_amd import rolling_shutter as rs

    n = 8
    A = _transitions(n)
    conf = np.ones(n - 1)
    V = rs.velocities(A, conf)
    assert V.shape == (n, 6) and V.dtype == np.float64
    assert np.allclose(V[0], _forward(A[0]), rtol=0, atol=1e-15)                       # clip start: the forward difference alone
    assert np.allclose(V[n - 1], _backward(A[n - 2]), rtol=0, atol=1e-15)              # clip end: the backward difference alone
    for i in range(1, n - 1):
        assert np.allclose(V[i], 0.5 * (_forward(A[i]) + _backward(A[i - 1])), rtol=0, atol=1e-15)
    # a pair with confidence 0 is not available: its two frames fall back to their other side
    conf[3] = 0.0
    Vg = rs.velocities(A, conf)
    assert np.allclose(Vg[3], _backward(A[2]), rtol=0, atol=1e-15) and np.allclose(Vg[4], _forward(A[4]), rtol=0, atol=1e-15)
    keep = [i for i in range(n) if i not in (3, 4)]
    assert np.array_equal(Vg[keep], V[keep])
    # a shot boundary in front of frame 5 takes pair 4 out, whatever its confidence says
    Vc = rs.velocities(A, np.ones(n - 1), [(0, 5), (5, n)])
    assert np.allclose(Vc[4], _backward(A[3]), rtol=0, atol=1e-15) and np.allclose(Vc[5], _forward(A[5]), rtol=0, atol=1e-15)
    # neither side available: zeros (a one-frame shot; a frame between two failed pairs)
    Vs = rs.velocities(A, np.ones(n - 1), [(0, 3), (3, 4), (4, n)])
    assert not Vs[3].any() and Vs[2].any() and Vs[4].any()
    conf = np.ones(n - 1)
    conf[[1, 2]] = 0.0
    assert not rs.velocities(A, conf)[2].any()
    # float32 input (what the plan holds), an identity clip, a two-frame clip
    assert np.allclose(rs.velocities(A.astype(np.float32), np.ones(n - 1)), V, rtol=0, atol=1e-5)
    assert not rs.velocities(np.tile(np.eye(3), (n - 1, 1, 1)), np.ones(n - 1)).any()
    assert rs.velocities(A[:1], [1.0]).shape == (2, 6)
    assert rs.velocities(np.zeros((0, 3, 3)), []).shape == (1, 6)


def test_velocity_of_a_pure_translation_is_the_translation(pkg):
    from vstab_amd import rolling_shutter as rs

    A = np.tile(np.eye(3), (3, 1, 1))
    A[:, 0, 2], A[:, 1, 2] = (3.0, 5.0, 7.0), (-1.0, -2.0, 0.5)
    V = rs.velocities(A, np.ones(3))
    assert np.array_equal(V[:, [2, 5]], [[3.0, -1.0], [4.0, -1.5], [6.0, -0.75], [7.0, 0.5]]) and not V[:, [0, 1, 3, 4]].any()


def test_a_projective_transition_raises(pkg):
    from vstab_amd import rolling_shutter as rs

    A = _transitions(4)
    A[1, 2, 0] = 1e-6
    with pytest.raises(ValueError, match=r"transition 1 has the last row .* not \(0, 0, 1\)"):
        rs.velocities(A, np.ones(3))
    with pytest.raises(ValueError, match="2 confidences for 3 transitions"):
        rs.velocities(_transitions(4), np.ones(2))


# ---- the readout estimate --------------------------------------------------------------------------------------------------
def case_path(mode, size, seed):
    """Amplitudes scale with the frame's width: 16 x 9 px at 480; the similarity cases add small rotation and scale terms."""
    w, h = size
    s = w / 480.0
    amp = (16.0 * s, 9.0 * s, 0.0, 0.0) if mode == "translation" else (16.0 * s, 9.0 * s, 0.003, 0.003)
    return R.CameraPath(w, h, amp=amp, omega=0.3, seed=seed)


def estimate_case(rs, mode, rho, size, seed, n=CLIP_FRAMES, noise=0.05):
    path = case_path(mode, size, seed)
    rng = np.random.default_rng(seed)
    flows = np.stack([R.rolling_flow_grid(path, k, rho, 8, noise=noise, rng=rng) for k in range(n - 1)])
    mats = np.stack([R.least_squares_fit(flows[k], 8, mode) for k in range(n - 1)])
    residual, count = R.row_residual(flows, 8, size, mats)
    return rs.estimate_readout(residual, count, mats, [1.0] * (n - 1), [mode] * (n - 1), None, size, 8)


def test_the_case_paths_are_slow_against_the_frame_rate():
    for mode, size, seed in ((m, s, k) for m in FIT_MODES for s in SIZES for k in SEEDS):
        assert case_path(mode, size, seed).omega.max() <= 0.35


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("rho", READOUTS)
@pytest.mark.parametrize("mode", FIT_MODES)
def test_readout_is_recovered_from_analytic_rolling_flows(pkg, mode, rho, size):
    from vstab_amd import rolling_shutter as rs

    for seed in SEEDS:
        est = estimate_case(rs, mode, rho, size, seed)
        print(f"\nreadout {mode} rho {rho} {size[0]}x{size[1]} seed {seed}: {json.dumps(est)}")
        assert est["source"] == "estimated" and est["pairs_used"] == CLIP_FRAMES - 3
        assert est["rows_used"] == est["pairs_used"] * -(-size[1] // 8)
        assert -1.0 <= est["readout"] <= 1.0 and est["readout"] == float(np.clip(est["readout_raw"], -1.0, 1.0))
        assert abs(est["readout"] - rho) <= READOUT_TOLERANCE, est
        assert np.sign(est["readout"]) == np.sign(rho)


def test_a_global_shutter_clip_reads_zero(pkg):
    from vstab_amd import rolling_shutter as rs

    est = estimate_case(rs, "similarity", 0.0, (960, 540), 0)
    assert est["source"] == "estimated" and abs(est["readout"]) <= READOUT_TOLERANCE


def test_constant_velocity_is_not_observable(pkg):
    """A pan at constant velocity shears every frame alike: the fit of each pair takes the shear for motion, no residual is
    left and no change of velocity predicts one.  The readout cannot be seen, and nothing is corrected."""
    from vstab_amd import rolling_shutter as rs

    w, h, n, rho = 480, 270, 10, 0.7
    gh, gw = -(-h // 8), -(-w // 8)
    flows = np.tile(np.float32([6.0, -3.0]), (n - 1, gh, gw, 1))          # the flow of a rolling pan IS the constant flow
    mats = np.stack([R.least_squares_fit(flows[k], 8, "translation") for k in range(n - 1)])
    residual, count = R.row_residual(flows, 8, (w, h), mats)
    est = rs.estimate_readout(residual, count, mats, [1.0] * (n - 1), ["translation"] * (n - 1), None, (w, h), 8)
    assert est["source"] == "not_observable" and est["readout"] == 0.0 and est["readout_raw"] == 0.0
    assert est["signal_rms_px"] < rs.ROW_MIN_RMS_PX and est["pairs_used"] == n - 3
    block = rs.meta_block(est["readout"], est["source"], est, rs.velocities(mats, np.ones(n - 1)), (w, h))
    assert block["source"] == "not_observable" and block["readout"] == 0.0 and block["skew_px_max"] == 0.0
    assert rho != 0.0


def test_usable_pairs_and_rows(pkg):
    from vstab_amd import rolling_shutter as rs

    size, n = (200, 120), 12
    path = case_path("translation", size, 0)
    flows = np.stack([R.rolling_flow_grid(path, k, 0.7, 8) for k in range(n - 1)])
    mats = np.stack([R.least_squares_fit(flows[k], 8, "translation") for k in range(n - 1)])
    residual, count = R.row_residual(flows, 8, size, mats)
    modes = ["translation"] * (n - 1)
    full = rs.estimate_readout(residual, count, mats, np.ones(n - 1), modes, None, size, 8)
    assert full["pairs_used"] == n - 3                                      # the end pairs have a one-sided velocity
    conf = np.ones(n - 1)
    conf[5] = 0.0                                                           # a failed pair takes its two neighbours with it
    assert rs.estimate_readout(residual, count, mats, conf, modes, None, size, 8)["pairs_used"] == n - 3 - 3
    cut = rs.estimate_readout(residual, count, mats, np.ones(n - 1), modes, [(0, 6), (6, n)], size, 8)
    assert cut["pairs_used"] == n - 3 - 3 and abs(cut["readout"] - 0.7) <= READOUT_TOLERANCE
    starved = count.copy()
    starved[:, 4:] = 7                                                      # rows below ROW_MIN_SAMPLES do not count
    assert rs.estimate_readout(residual, starved, mats, np.ones(n - 1), modes, None, size, 8)["rows_used"] == (n - 3) * 4
    none = rs.estimate_readout(residual, np.zeros_like(count), mats, np.ones(n - 1), modes, None, size, 8)
    assert none["source"] == "not_observable" and none["rows_used"] == 0 and none["signal_rms_px"] == 0.0
    with pytest.raises(ValueError, match="do not describe the same pairs"):
        rs.estimate_readout(residual[:-1], count, mats, np.ones(n - 1), modes, None, size, 8)


def test_similarity_absorbs_the_stated_share_of_a_row_linear_field(pkg):
    """The factor f_k of the estimate: a least-squares similarity leaves w^2 / (w^2 + h^2) of a row-linear field at the central
    column (exactly so for the grid's own second moments, which the continuous w^2 and h^2 stand for)."""
    for w, h in SIZES:
        gh, gw = -(-h // 8), -(-w // 8)
        x = (np.arange(gw) * 8.0)[None, :].repeat(gh, 0)
        y = (np.arange(gh) * 8.0)[:, None].repeat(gw, 1)
        flow = np.stack([0.01 * (y - y.mean()), -0.004 * (y - y.mean())], -1)
        A = R.least_squares_fit(flow, 8, "similarity").astype(np.float64)
        left_x = (x + flow[..., 0]) - (A[0, 0] * x + A[0, 1] * y + A[0, 2])
        col = np.argmin(np.abs(x[0] - x.mean()))
        slope = np.polyfit(y[:, col], left_x[:, col], 1)[0]
        sxx, syy = ((x - x.mean()) ** 2).sum(), ((y - y.mean()) ** 2).sum()
        assert abs(slope / 0.01 - sxx / (sxx + syy)) < 1e-5
        assert abs(sxx / (sxx + syy) - w * w / float(w * w + h * h)) < 0.02


# ---- the meta block ------------------------------------------------------------------------------------------------------
def test_meta_block_survives_json(pkg):
    from vstab_amd import rolling_shutter as rs

    size = (480, 270)
    V = rs.velocities(_transitions(6), np.ones(5))
    given = rs.meta_block(0.7, "given", None, V, size)
    assert list(given) == ["version", "readout", "source", "estimate", "skew_px_mean", "skew_px_max", "velocity"]
    assert given["version"] == 1 and given["readout"] == 0.7 and given["source"] == "given" and given["estimate"] is None
    assert np.array_equal(np.array(given["velocity"]), V) and 0.0 < given["skew_px_mean"] <= given["skew_px_max"]
    est = estimate_case(rs, "translation", 0.7, (200, 120), 0)
    block = rs.meta_block(est["readout"], est["source"], est, V, size)
    assert list(block["estimate"]) == ["readout_raw", "pairs_used", "rows_used", "signal_rms_px"] and block["source"] == "estimated"
    for b in (given, block):
        assert json.loads(json.dumps(b)) == b
    # skew: |tau| * |v| at the corners -- a pure translation of (6, -8) px per frame and readout 0.5: 1/4 * 10 at every corner
    flat = np.tile([0.0, 0.0, 6.0, 0.0, 0.0, -8.0], (3, 1))
    corner = rs.corner_skew(flat, 0.5, size)
    D_top, D_bottom = 1.0 - 0.5 * -8.0 / 269.0, 1.0 - 0.5 * -8.0 / 269.0
    assert np.allclose(corner[:, :2], 0.25 * 10.0 / D_top) and np.allclose(corner[:, 2:], 0.25 * 10.0 / D_bottom)
    assert rs.meta_block(0.0, "not_observable", est, flat, size)["skew_px_max"] == 0.0


# ---- the restatements' known answers ---------------------------------------------------------------------------------------
def test_displacement_rule_known_answers():
    h = 101
    qx, qy = np.float64([10.0, 10.0, 10.0, 10.0]), np.float64([0.0, 50.0, 100.0, 250.0])
    cx, cy = R.displacement(qx, qy, [0.0, 0.0, 8.0, 0.0, 0.0, 0.0], 1.0, h)
    assert np.array_equal(cx, [4.0, -0.0, -4.0, -4.0]) and not cy.any()            # the row is clamped to the frame
    # vy = 25, rho = 1: D = 1 - 25/100 = 0.75; tau = (y/100 - 0.5) / 0.75
    cx, cy = R.displacement(qx, qy, [0.0, 0.0, 3.0, 0.0, 0.0, 25.0], 1.0, h)
    assert np.allclose(cy, -np.float64([-0.5, 0.0, 0.5, 0.5]) / 0.75 * 25.0, rtol=1e-15, atol=0)
    # vy = 80: D = 0.2 -> clamped to 0.5
    cx, cy = R.displacement(qx, qy, [0.0, 0.0, 3.0, 0.0, 0.0, 80.0], 1.0, h)
    assert np.array_equal(cy, -np.float64([-0.5, 0.0, 0.5, 0.5]) / 0.5 * 80.0)
    # NaN anywhere: nothing is moved; a NaN row reads as row 0
    assert not np.any(R.displacement(qx, qy, [0.0, np.nan, 3.0, 0.0, 0.0, 2.0], 0.5, h))
    cx, cy = R.displacement(np.float64([10.0]), np.float64([np.nan]), [0.0, 0.0, 3.0, 0.0, 0.0, 0.0], 0.5, h)
    assert not cx.any() and not cy.any()
    for vel, rho in (([0.0] * 6, 1.0), ([0.01, 0.0, 5.0, 0.0, 0.01, -3.0], 0.0)):
        cx, cy = R.displacement(qx, qy, vel, rho, h)
        assert not cx.any() and not cy.any()


def test_the_restatement_at_zero_is_the_oracle_warp(oracle):
    for subpix in ("q5", "exact"):
        for kind, (w, h), out_size in (("similarity", (61, 45), (61, 45)), ("perspective", (65, 9), (130, 17)), ("horizon", (96, 64), (96, 64))):
            src = util.synth_frames(1, h, w, seed=w)[0]
            m = util.test_matrices(1, w, h, kind, seed=7)[0].astype(np.float32)
            want, cov = oracle.warp_frame(src, m, out_size, "bilinear", (0.2, 0.4, 0.6), subpix)
            for vel, rho in (([0.0] * 6, 1.0), ([0.01, 0.0, 5.0, 0.0, 0.01, -3.0], 0.0)):
                got, mask = R.rolling_warp_frame(src, m, out_size, vel, rho, (0.2, 0.4, 0.6), subpix)
                assert np.array_equal(got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (kind, subpix)
                assert np.array_equal(mask > 0.5, np.asarray(cov) < 0.5)


def test_row_median_rule_known_answers():
    step, w, h = 8, 72, 16                          # 9 x 2 grid
    flow = np.zeros((1, 2, 9, 2), np.float32)
    flow[0, 0, :, 0] = [5, 1, 4, 2, 3, 9, 8, 7, 6]
    flow[0, 1, :, 1] = [5, 1, 4, 2, 3, 9, 8, 7, np.nan]
    eye = np.eye(3, dtype=np.float32)[None]
    res, cnt = R.row_residual(flow, step, (w, h), eye)
    assert cnt.tolist() == [[9, 8]] and res[0, 0].tolist() == [5.0, 0.0] and res[0, 1].tolist() == [0.0, 4.5]
    blocked = np.zeros((2, 2, 9), np.uint8)
    blocked[1, 0, :2] = 1
    res, cnt = R.row_residual(flow, step, (w, h), eye, blocked)
    assert cnt.tolist() == [[7, 8]] and res[0, 0].tolist() == [0.0, 0.0]


def test_the_renderer_and_the_analytic_flow_agree():
    """rolling_flow_grid's fixed point: the texture point a rolling frame shows at s is shown at s + flow by the next one."""
    path = case_path("similarity", (200, 120), 1)
    for rho in (0.0, 0.7, -1.0):
        flow = R.rolling_flow_grid(path, 3, rho, 8).astype(np.float64)
        gh, gw, _ = flow.shape
        x = (np.arange(gw) * 8.0)[None, :].repeat(gh, 0)
        y = (np.arange(gh) * 8.0)[:, None].repeat(gw, 1)
        X0, Y0 = path.to_texture(x, y, path.row_time(3, y, rho))
        X1, Y1 = path.to_texture(x + flow[..., 0], y + flow[..., 1], path.row_time(4, y + flow[..., 1], rho))
        assert np.abs(X1 - X0).max() < 1e-4 and np.abs(Y1 - Y0).max() < 1e-4
    x, y = np.float64([[3.0, 150.0]]), np.float64([[7.0, 90.0]])
    u, v = path.to_image(*path.to_texture(x, y, 2.5), 2.5)
    assert np.allclose(u, x) and np.allclose(v, y)
    m = path.matrix(2.5)
    X, Y = path.to_texture(x, y, 2.5)
    assert np.allclose(m[0, 0] * X + m[0, 1] * Y + m[0, 2], x) and np.allclose(m[1, 0] * X + m[1, 1] * Y + m[1, 2], y)
    assert np.array_equal(path.matrix(0.0), np.eye(3))
