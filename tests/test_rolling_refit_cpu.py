"""Rolling-shutter refit, the parts that need no GPU (include/vstab.h "vstab_rectify_samples_batch";
flow_pipeline._stabilize_frames(rolling_refit=True)): what one refit pass buys on analytic rolling flows, the rule's invariants
on the restatement (tests/rolling_refit_restatement.py), the request checks and the public surface.

The analytic cases: the exact flow a rolling pair shows (tests/rolling_shutter_restatement.rolling_flow_grid, no noise) at the
stride-8 grid of the image itself, least-squares similarity fits, the per-frame velocities of rolling_shutter.velocities on the
first pass's transitions, the restatement's rectified pairs, a least-squares similarity fit of those.  The truth of pair k is
path.matrix(k + 1) @ inv(path.matrix(k)); errors are corner errors in px (restatement.corner_errors).  Measured here:
  480 x 270, 12 frames, amp (24, 20, 0.004, 0.004), readout 0.7: pair error mean 0.3063 -> 0.0314 (0.103 x), chain 2.484 -> 0.191
  (0.077 x); 61 x 45, 8 frames, amp (3, 2.5, 0.004, 0.004): chain 0.179 -> 0.028 (0.155 x).
The bounds are 0.25 x, 0.25 x and 0.35 x: the margin covers float32 storage and the difference between a least-squares fit and
the library's RANSAC / least-squares fit.
"""

import asyncio
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import rolling_refit_restatement as RF
from tests import rolling_shutter_restatement as R
from tests.rolling_refit_restatement import BIG, CHAIN_BOUND, PAIR_BOUND, SMALL, STEP, analytic_case

ROOT = Path(__file__).resolve().parents[1]
ARGS = ("crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def one_pass(pkg, case, flows, first, readout):
    """The refit's transitions [P,3,3]: velocities of the first pass -> rectified pairs -> least-squares similarity."""
    from vstab_amd import rolling_shutter as rs

    velocity = rs.velocities(first, np.ones(len(first)), None)
    pairs, counts, unsolved = RF.rectify_samples(flows, STEP, (case["w"], case["h"]), velocity, readout)
    assert (counts == flows.shape[1] * flows.shape[2]).all() and not unsolved.any()
    return np.stack([RF.similarity_from_pairs(pairs[k], counts[k]) for k in range(len(first))])


# ---- what one pass buys ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big", "small"])
def test_one_pass_on_the_analytic_clip(pkg, name):
    case = BIG if name == "big" else SMALL
    size = (case["w"], case["h"])
    flows, truth, first = analytic_case(case)
    refit = one_pass(pkg, case, flows, first, case["rho"])
    pair0, chain0 = RF.corner_errors(first, truth, size)
    pair1, chain1 = RF.corner_errors(refit, truth, size)
    print(f"\nrolling_refit {name}: pair error mean {pair0.mean():.4f} -> {pair1.mean():.4f} ({pair1.mean() / pair0.mean():.3f} x), "
          f"worst {pair0.max():.3f} -> {pair1.max():.3f}, chain {chain0:.3f} -> {chain1:.3f} ({chain1 / chain0:.3f} x)")
    assert chain1 <= CHAIN_BOUND[name] * chain0, (chain0, chain1)
    if name == "big":
        assert pair1.mean() <= PAIR_BOUND * pair0.mean(), (pair0.mean(), pair1.mean())


def test_the_readout_auto_finds_costs_little(pkg):
    """The refit with the readout "auto" reports on this clip (0.643 for 0.7) stays inside the bound too."""
    flows, truth, first = analytic_case(BIG)
    refit = one_pass(pkg, BIG, flows, first, 0.643)
    size = (BIG["w"], BIG["h"])
    pair0, chain0 = RF.corner_errors(first, truth, size)
    pair1, chain1 = RF.corner_errors(refit, truth, size)
    assert chain1 <= CHAIN_BOUND["big"] * chain0 and pair1.mean() <= PAIR_BOUND * pair0.mean()


# ---- the rule's invariants ------------------------------------------------------------------------------------------------------
def _noisy_flow(rng, pairs, w, h):
    gh, gw = -(-h // STEP), -(-w // STEP)
    return (rng.normal(0.0, 3.0, (pairs, gh, gw, 2)) + np.array([4.0, -2.5])).astype(np.float32), gh, gw


def test_readout_zero_and_zero_velocity_are_the_identity_in_bits():
    rng = np.random.default_rng(5)
    w, h, pairs = 61, 45, 3
    flow, gh, gw = _noisy_flow(rng, pairs, w, h)
    flow[1, 2, 3, 0] = np.nan
    flow[2, 0, 1, 1] = np.inf
    moving = np.tile([0.01, -0.004, 5.0, 0.004, 0.01, -3.0], (pairs + 1, 1))
    px = (np.arange(gw) * STEP).astype(np.float32)[None, :].repeat(gh, 0)
    py = (np.arange(gh) * STEP).astype(np.float32)[:, None].repeat(gw, 1)
    want = np.empty((pairs, gh, gw, 4), np.float32)
    want[..., 0], want[..., 1] = px, py
    with np.errstate(all="ignore"):
        want[..., 2], want[..., 3] = px + flow[..., 0], py + flow[..., 1]
    bad = ~(np.isfinite(want[..., 2]) & np.isfinite(want[..., 3]))
    want[bad, 2:] = np.nan
    want = want.reshape(pairs, gh * gw, 4)
    for velocity, rho in ((moving, 0.0), (moving, -0.0), (np.zeros((pairs + 1, 6)), 0.7), (np.zeros((pairs + 1, 6)), -1.0)):
        got, counts, unsolved = RF.rectify_samples(flow, STEP, (w, h), velocity, rho)
        assert np.array_equal(_bits(got), _bits(want)), rho
        assert (counts == gh * gw).all() and not unsolved.any()
    assert int(bad.sum()) == 2


def test_compaction_keeps_the_order_and_the_tail_is_nan():
    rng = np.random.default_rng(6)
    w, h, pairs = 64, 64, 2
    flow, gh, gw = _noisy_flow(rng, pairs, w, h)
    blocked = (rng.random((pairs + 1, gh, gw)) < 0.3).astype(np.uint8)
    blocked[2] = 1                                                   # the last frame: pair 1 admits nothing
    velocity = np.tile([0.0, 0.0, 6.0, 0.0, 0.0, -2.0], (pairs + 1, 1))
    got, counts, unsolved = RF.rectify_samples(flow, STEP, (w, h), velocity, 0.7, blocked)
    full, _, _ = RF.rectify_samples(flow, STEP, (w, h), velocity, 0.7)
    keep = (blocked[0].ravel() == 0) & (blocked[1].ravel() == 0)
    assert counts.tolist() == [int(keep.sum()), 0] and 0 < counts[0] < gh * gw
    assert np.array_equal(_bits(got[0, : counts[0]]), _bits(full[0][keep]))
    assert (_bits(got[0, counts[0]:]) == 0x7FC00000).all() and (_bits(got[1]) == 0x7FC00000).all()
    assert not unsolved.any()


def test_a_folded_row_is_unsolved_and_left_alone():
    """det = (1 + tau V0)(1 + tau V4) - tau^2 V1 V3 falls below 0.25 at the rows where |tau| is large: e = (0, 0), counted."""
    w, h = 64, 64
    gh = gw = 8
    flow = np.zeros((1, gh, gw, 2), np.float32)
    velocity = np.array([[-2.5, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0] * 6])      # the last row: tau = 0.389, a = 0.028
    got, counts, unsolved = RF.rectify_samples(flow, STEP, (w, h), velocity, 1.0)
    rows = got[0].reshape(gh, gw, 4)
    y = np.arange(gh) * STEP
    tau = y / 63.0 - 0.5
    folded = (1.0 + tau * -2.5) < 0.25
    assert folded.any() and not folded.all() and int(unsolved[0]) == int(folded.sum()) * gw
    assert np.array_equal(rows[folded][..., :2], rows[folded][..., 2:])     # prev == p, next == c == p (zero flow, zero V[1])
    assert (rows[~folded][:, 1:, 0] != (np.arange(1, gw) * STEP)).all()


def test_it_inverts_the_forward_rule():
    """A point q that the forward rule shows at s = q - c(q) comes back from s within 1e-9 px, where no clamp binds: D >= 0.5,
    q_y and s_y inside [0, H - 1], det >= 0.25."""
    rng = np.random.default_rng(7)
    w, h = 480, 270
    worst = 0.0
    for rho in (0.7, -1.0, 0.3):
        for _ in range(5):
            th, sc = rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
            V = np.array([sc, -th, rng.uniform(-8, 8) - sc * w / 2 + th * h / 2, th, sc, rng.uniform(-6, 6) - th * w / 2 - sc * h / 2])
            qx, qy = rng.uniform(0, w - 1, 500), rng.uniform(0.05 * h, 0.95 * h, 500)
            cx, cy = R.displacement(qx, qy, V, rho, h)
            sx, sy = qx - cx, qy - cy
            vy = (V[3] * qx + V[4] * qy) + V[5]
            free = (1.0 - rho * vy / (h - 1) >= 0.5) & (sy >= 0.0) & (sy <= h - 1.0)
            assert free.sum() > 400
            ex, ey, solved = RF.inverse_displacement(sx, sy, V, rho, h)
            assert solved[free].all()
            worst = max(worst, float(np.hypot(sx + ex - qx, sy + ey - qy)[free].max()))
    assert worst <= 1e-9, worst


# ---- request checks -------------------------------------------------------------------------------------------------------------
def _context(n=4, h=24, w=32):
    import torch

    from vstab_amd import host_math as hm

    return hm._normalize_video_input(torch.zeros((n, h, w, 3)))


def test_every_refusal_names_its_reason(pkg):
    """All of them come before any GPU work: nothing below reaches for a GPU."""
    from vstab_amd import distributed
    from vstab_amd import flow_pipeline as fp

    for value in (1, 0, "yes", 0.5, (True,)):
        with pytest.raises(ValueError, match=re.escape(f"rolling_refit={value!r}: expected None or a bool")):
            fp._stabilize_frames(_context(), *ARGS, rolling_shutter=0.5, rolling_refit=value)
    for off in (None, 0, 0.0):
        with pytest.raises(ValueError, match="rolling_refit=True needs rolling_shutter"):
            fp._stabilize_frames(_context(), *ARGS, rolling_shutter=off, rolling_refit=True)
    for estimator in ("classic", "flow_phase_correlate"):
        with pytest.raises(ValueError, match=rf"rolling_refit is not supported with estimator '{estimator}'.*no grid of flow samples to rectify"):
            fp._stabilize_frames(_context(), *ARGS, rolling_shutter=0.5, rolling_refit=True, estimator=estimator)
    with pytest.raises(ValueError, match="rolling_refit is not supported with drift_correction: the keyframe alignment registers images"):
        fp._stabilize_frames(_context(), *ARGS, rolling_shutter=0.5, rolling_refit=True, drift_correction=True)
    # what rolling_shutter refuses stays refused, with its own reason
    with pytest.raises(ValueError, match="is not affine"):
        fp._stabilize_frames(_context(), "crop_and_pad", "perspective", *ARGS[2:], rolling_shutter=0.5, rolling_refit=True)
    with pytest.raises(ValueError, match="mesh_warp: the warp takes one displacement"):
        fp._stabilize_frames(_context(), *ARGS, rolling_shutter="auto", rolling_refit=True, mesh_warp=True)
    with pytest.raises(ValueError, match="the rolling-shutter correction is not sharded"):
        distributed.stabilize_sharded(None, None, 4, *ARGS, rolling_shutter=0.5)
    assert "rolling_refit" not in inspect.signature(distributed.stabilize_sharded).parameters     # the sharded path has no refit


def test_the_request_with_the_option_off_is_todays(pkg):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import rolling_shutter as rs

    params = inspect.signature(fp._stabilize_frames).parameters
    p = params["rolling_refit"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(params).index("rolling_refit") == list(params).index("rolling_shutter") + 1
    kw = {name: prm.default for name, prm in params.items() if prm.kind is inspect.Parameter.KEYWORD_ONLY}
    today = {k: v for k, v in kw.items() if k != "rolling_refit"}
    for rolling in (None, 0.5, "auto"):
        want = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(today, rolling_shutter=rolling))
        assert want.refit is False and list(fp.FlowRequest.__dataclass_fields__)[-1] == "refit"
        assert want == fp.FlowRequest(*[getattr(want, f) for f in list(fp.FlowRequest.__dataclass_fields__)[:-1]])
        for off in (None, False):
            got = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, rolling_shutter=rolling, rolling_refit=off))
            assert got == want and got.kept_by_products == want.kept_by_products and got.needs_host_plan == want.needs_host_plan
    given = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, rolling_shutter=0.5))
    assert given.kept_by_products == ()
    on = fp.check_flow_request("crop_and_pad", "similarity", "flow_tvl1", dict(kw, rolling_shutter=0.5, rolling_refit=True))
    assert on.refit is True and on.rolling == 0.5 and on.kept_by_products == ("grid_out",) and on.needs_host_plan
    assert rs.check_refit_request(np.True_, 0.5, "flow") is True and rs.check_refit_request(np.False_, None, "classic") is False


def test_bypasses_ignore_the_keyword(pkg):
    import dataclasses

    from vstab_amd import flow_pipeline as fp

    for n in (0, 1):
        def make():
            return _context(n=n) if n else dataclasses.replace(_context(n=1), frames=[], batch=None)

        without = fp._stabilize_frames(make(), *ARGS)
        got = fp._stabilize_frames(make(), *ARGS, rolling_shutter=0.7, rolling_refit=True)
        assert got.meta == without.meta and "rolling_shutter" not in got.meta


def test_the_meta_block(pkg):
    from vstab_amd import rolling_shutter as rs

    assert rs.refit_block(0) == {"passes": 0, "pairs_refit": 0, "samples_unsolved_max": 0, "transition_change_px_mean": 0.0,
                                 "transition_change_px_max": 0.0}
    eye = np.eye(3)
    moved = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 4.0], [0.0, 0.0, 1.0]])
    turned = np.array([[1.0, -0.01, 0.0], [0.01, 1.0, 0.0], [0.0, 0.0, 1.0]])
    change = rs.transition_change_px([eye, eye, eye], [eye, moved, turned], (101, 51))
    assert change[0] == 0.0 and change[1] == 5.0 and abs(change[2] - 0.01 * np.hypot(100, 50)) < 1e-12
    block = rs.refit_block(1, [eye, eye, eye], [eye, moved, turned], [1.0, 0.0, 0.9], [(0, 4)], np.array([0, 7, 2]), (101, 51))
    assert block["passes"] == 1 and block["pairs_refit"] == 2 and block["samples_unsolved_max"] == 7
    assert block["transition_change_px_max"] == 5.0 and abs(block["transition_change_px_mean"] - change.mean()) < 1e-12
    # the block rides in meta["rolling_shutter"] and the parser of the round trip ignores it
    meta = {"rolling_shutter": dict(rs.meta_block(0.7, "given", None, np.zeros((4, 6)), (101, 51)), refit=block)}
    readout, velocity = rs.parse_block(meta, 4)
    assert readout == 0.7 and velocity.shape == (4, 6) and meta["rolling_shutter"]["version"] == 1


# ---- the public surface ---------------------------------------------------------------------------------------------------------
def test_header_binding_and_documents_agree(pkg):
    from vstab_amd import native

    header = (ROOT / "include" / "vstab.h").read_text()
    assert ("int vstab_rectify_samples_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,\n"
            "                                const double* velocity, double readout, const uint8_t* blocked, float* point_pairs,\n"
            "                                int32_t* counts, uint32_t* unsolved);") in header
    for words in ("yr = (y < 0) ? 0 : y", 'timing kind "rectify"', "fewer\n * than 12 points or fewer than 8 finite ones",
                  "gh*gw <= 16384", "next = (NaN, NaN)"):
        assert words in header, words
    assert re.search(r"^#define VSTAB_ABI_VERSION 1$", header, re.M) and RF.MIN_DET == 0.25
    assert "vstab_rectify_samples_batch" in native.EXPORTED_SYMBOLS
    assert list(inspect.signature(native.Context.rectify_samples_batch).parameters)[1:] == [
        "grid_flow", "step", "work_size", "velocity", "readout", "blocked"]
    assert inspect.signature(native.Context.rectify_samples_batch).parameters["blocked"].default is None
    for doc, words in (("README.md", ("rolling_refit", "video_stabilizer_flow_rolling_refit")), ("DESIGN.md", ("8k", "rolling_refit", "one pass")),
                       ("INTEGRATION.md", ("vstab_rectify_samples_batch", "VideoStabilizerAmdRollingRefitExtension")),
                       ("tools/README.md", ("rolling_refit_report.py",))):
        text = (ROOT / doc).read_text()
        for word in words:
            assert word in text, (doc, word)


def test_node_sockets_and_where_it_is_listed(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerFlowRollingRefit
    schema, base = node.define_schema(), nodes.VideoStabilizerFlowRolling.define_schema()
    assert schema.node_id == "video_stabilizer_flow_rolling_refit"
    assert schema.display_name == "Video Stabilizer Flow (Rolling Shutter, Refit)"
    assert [s.id for s in schema.inputs] == [s.id for s in base.inputs] + ["refit"]
    assert [s.id for s in schema.outputs] == [s.id for s in base.outputs]
    by_id = {s.id: s for s in schema.inputs}
    assert by_id["refit"].kind.upper() == "BOOLEAN" and by_id["refit"].options["default"] is True
    for other in base.inputs:
        assert by_id[other.id].kind == other.kind and by_id[other.id].options == other.options
    assert list(inspect.signature(node.execute).parameters)[-2:] == ["readout", "refit"]
    assert node not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    listed = asyncio.run(nodes.VideoStabilizerAmdRollingRefitExtension().get_node_list())
    before = asyncio.run(nodes.VideoStabilizerAmdAnchorExposureExtension().get_node_list())
    assert listed == before + [node] and node not in before
    assert issubclass(nodes.VideoStabilizerAmdRollingRefitExtension, nodes.VideoStabilizerAmdAnchorExposureExtension)
    entry = asyncio.run(vstab_amd.comfy_entrypoint())
    assert type(entry) is nodes.VideoStabilizerAmdMaskedExtension and node not in asyncio.run(entry.get_node_list())
