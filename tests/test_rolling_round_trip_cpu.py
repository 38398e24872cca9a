"""Rolling shutter round trip, the parts that need no GPU (include/vstab.h "vstab_rolling_unwarp_batch";
rolling_shutter.parse_block; apply_pipeline.apply_motion(rolling=True)).

  1. the algebra: the restatement of the inverse rule, evaluated at s = q + tau v(q), returns q - s
  2. a coordinate image sent through the forward restatement and back through the inverse one comes back as well as the plain
     round trip does (+ 1/32 px); sent back through the plain inverse it is off by at least half the corner skew
  3. zero readout / all-zero velocity restate the plain warp in bits; the unsolved rows of a collapsing velocity
  4. parse_block: every refusal; float64 velocities survive JSON exactly
  5. the refusals of apply_motion(rolling=True), raised before any GPU use
  6. the public surface: header, exports, keyword, node, extension, documents
"""

import asyncio
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import rolling_round_trip_restatement as RT
from tests import rolling_shutter_restatement as R
from tests import util

ROOT = Path(__file__).resolve().parents[1]
W, H = 160, 90
RHO = 0.7
VELOCITY = np.array([0.01, -0.004, 7.0, 0.004, 0.01, -4.0])
ERODE = 2
RGB = (127, 127, 127)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the algebra ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height", [2, 45, 270])
def test_the_inverse_undoes_the_forward_equation(height):
    """Random affine velocities (entries of L in +-0.05, t in +-20 px), rho in +-1, q on a 480-px-wide canvas `height` rows
    high; s = q + tau v(q) with the closed-form tau, formed in extended precision and rounded to float64 once.  Kept are the
    draws inside the pair's region of validity as include/vstab.h states it: the forward D >= 0.5 and the inverse
    det >= 0.25 (at 2 rows, where rho v_y / (H-1) reaches 45, that is about half of the draws).

    Tolerance, from the operation count.  One component of e goes through 26 rounded fp64 operations (tau 3, a..d 6, det 3,
    vx and vy 8, rx and ry 2, the numerator 3, the quotient 1), each off by at most u = 2^-53 of its own result; none of the
    results exceeds X = max(|s|, |q|, |v|, 1), and the only divisor is det >= 1/4, so the computed e is within
    26 * 4 * u * X of the exact e of the rounded s.  The rounding of s itself (u * X per coordinate) reaches q through
    dq = A^-1 (I - (rho / (H-1)) v e_y^T) ds: tau is read off s_y, so a step of s_y moves the whole solve by rho |v| / (H-1) --
    the factor G = 1 + |rho| |v| / (H-1) with |v| <= 2 max(|v_x|, |v_y|), 1.3 at 270 rows and up to 90 at 2 -- and |A^-1| <= 1 / det^(1/2) <= 2 here.  The same G
    bounds how far the 26 roundings can be carried.  Together below 128 * u * G * X = 64 * eps * G * X: a few ulp of the
    coordinates, times the one factor the equation itself has."""
    rng = np.random.default_rng(height)
    eps = np.finfo(np.float64).eps
    ld = np.longdouble
    kept = worst = 0
    for _ in range(200):
        V = np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-20, 20, 1), rng.uniform(-0.05, 0.05, 2), rng.uniform(-20, 20, 1)])
        rho = rng.uniform(-1.0, 1.0)
        qx, qy = rng.uniform(0, 479, 64), rng.uniform(0, height - 1, 64)
        hm1 = ld(height - 1)
        vx = ld(V[0]) * qx + ld(V[1]) * qy + ld(V[2])
        vy = ld(V[3]) * qx + ld(V[4]) * qy + ld(V[5])
        D = 1 - ld(rho) * vy / hm1
        tau = ld(rho) * (qy.astype(ld) / hm1 - ld(0.5)) / D
        sx, sy = (qx + tau * vx).astype(np.float64), (qy + tau * vy).astype(np.float64)
        ex, ey, unsolved = RT.inverse_displacement(sx, sy, V, rho, height)
        det = (1 + tau * ld(V[0])) * (1 + tau * ld(V[4])) - tau * ld(V[1]) * tau * ld(V[3])
        valid = (D >= 0.5) & (det >= 0.3)                          # (0.3: a hair inside 0.25, so that `unsolved` is decided)
        assert not unsolved[valid].any()
        speed = np.maximum(np.abs(vx), np.abs(vy)).astype(np.float64)
        G = 1.0 + abs(rho) * 2.0 * speed / (height - 1)
        X = np.maximum.reduce([np.abs(sx), np.abs(sy), qx, qy, speed, np.ones_like(qx)])
        tol = 64.0 * eps * G * X
        err = np.maximum(np.abs((ex - (qx.astype(ld) - sx)).astype(np.float64)), np.abs((ey - (qy.astype(ld) - sy)).astype(np.float64)))
        assert (err[valid] <= tol[valid]).all(), (height, float((err[valid] / tol[valid]).max()))
        kept += int(valid.sum())
        if valid.any():
            worst = max(worst, float((err[valid] / tol[valid]).max()))
    print(f"\nalgebra H={height}: {kept} of {200 * 64} draws inside the region of validity, worst error {worst:.3f} of the tolerance")
    assert kept >= 2000


def test_zero_readout_gives_a_zero_displacement():
    ys, xs = np.meshgrid(np.arange(7), np.arange(9), indexing="ij")
    for vel, rho in ((np.zeros(6), 1.0), (np.zeros(6), -0.3), (VELOCITY, 0.0), (-VELOCITY, -0.0)):
        ex, ey, unsolved = RT.inverse_displacement(xs, ys, vel, rho, 7)
        assert not ex.any() and not ey.any() and not unsolved.any()          # zeros of either sign compare equal to zero


# ---- 2. the round trip of a coordinate image -------------------------------------------------------------------------------
def _similarity(scale, angle, tx, ty):
    c, s = scale * np.cos(angle), scale * np.sin(angle)
    return np.array([[c, -s, tx], [s, c, ty], [0, 0, 1]], np.float64)


def _erode(valid, r):
    """Pixels whose (2r+1)^2 neighbourhood is valid; the outside of the frame is not."""
    p = np.pad(valid, r, constant_values=False)
    h, w = valid.shape
    rows = np.ones_like(p[:, r:r + w])
    for d in range(2 * r + 1):
        rows &= p[:, d:d + w]
    out = np.ones_like(valid)
    for d in range(2 * r + 1):
        out &= rows[d:d + h]
    return out


def coordinate_round_trip():
    """Coordinate image -> forward (rolling | plain) -> back (rolling inverse | plain inverse), all on the restatements.  The
    third channel carries validity: it is 1 where the stabilized frame saw the source, so a restored pixel whose taps all saw
    it reads 1 -- the mask of the first pass, seen from the second."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    coord = np.stack([xs, ys, np.ones_like(xs)], -1)[None]
    fwd = _similarity(1.03, 0.02, 4.3, -2.7).astype(np.float32)[None]
    inv = np.linalg.inv(fwd[0].astype(np.float64)).astype(np.float32)[None]
    vel, zero = VELOCITY[None], np.zeros((1, 6))
    black = (0.0, 0.0, 0.0)
    out = {"coord": coord[0]}
    for name, v_fwd, v_back in (("rolling", vel, vel), ("plain", zero, zero), ("plain_inverse", vel, zero)):
        stab, stab_mask, _ = R.rolling_warp(coord, fwd, (W, H), v_fwd, RHO, black, "q5")
        stab[..., 2] = 1.0 - stab_mask                             # validity travels with the pixels
        back, back_mask, _, unsolved = RT.rolling_unwarp(stab, inv, (W, H), v_back, RHO, black, "q5")
        valid = (back[0, ..., 2] == 1.0) & (back_mask[0] == 0)
        out[name] = dict(back=back[0], valid=valid, unsolved=int(unsolved.sum()))
    return out


def round_trip_errors(rt):
    """-> (max |restored - original| px of the rolling round trip, the plain round trip and the plain inverse of the rolling
    forward, over the pixels all three show, eroded by ERODE; the share of the frame those are)."""
    sel = _erode(rt["rolling"]["valid"] & rt["plain"]["valid"] & rt["plain_inverse"]["valid"], ERODE)
    err = {name: float(np.abs(rt[name]["back"][..., :2] - rt["coord"][..., :2])[sel].max()) for name in ("rolling", "plain", "plain_inverse")}
    return err, float(sel.mean())


@pytest.fixture(scope="module")
def round_trip():
    return coordinate_round_trip()


def test_round_trip_restores_the_coordinates(pkg, round_trip):
    """Measured (160 x 90, similarity 1.03 / 0.02 rad, readout 0.7, corner skew 3.15 px): the rolling round trip 0.0303 px, the
    plain round trip of the same matrices 0.0303 px, the plain inverse of the rolling forward 2.68 px."""
    from vstab_amd import rolling_shutter as rs

    skew = float(rs.corner_skew(VELOCITY[None], RHO, (W, H)).max())
    assert skew >= 2.0
    rt = round_trip
    err, interior = round_trip_errors(rt)
    assert interior > 0.5
    print(f"\nrolling round trip {W}x{H}: corner skew {skew:.3f} px; rolling {err['rolling']:.4f} px, plain {err['plain']:.4f} px, "
          f"plain inverse of the rolling forward {err['plain_inverse']:.4f} px; interior {interior:.2f}")
    assert rt["rolling"]["unsolved"] == 0
    # one more Q5 rounding of a coordinate: the displacement adds nothing else to a linear image
    assert err["rolling"] <= err["plain"] + 1.0 / 32.0
    assert err["plain_inverse"] >= 0.5 * skew


# ---- 3. the invariant and the unsolved branch --------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("kind,size,out_size", [("similarity", (96, 64), (96, 64)), ("perspective", (96, 64), (120, 70)),
                                                ("similarity", (61, 45), (333, 11)), ("similarity", (33, 5), (70, 2))])
def test_zero_velocity_restates_the_plain_warp(subpix, kind, size, out_size):
    w, h = size
    src = util.synth_frames(2, h, w, seed=w)
    mats = util.test_matrices(2, w, h, kind, seed=5).astype(np.float32)
    zero = np.zeros((2, 6))
    want = R.rolling_warp(src, mats, out_size, zero, 0.0, (0.2, 0.4, 0.6), subpix)
    for vel, rho in ((zero, 1.0), (-zero, -0.4), (np.tile(VELOCITY, (2, 1)), 0.0)):
        got = RT.rolling_unwarp(src, mats, out_size, vel, rho, (0.2, 0.4, 0.6), subpix)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
        assert got[2].tolist() == want[2].tolist() and not got[3].any()


def test_a_collapsing_velocity_leaves_rows_unsolved():
    w, h = 61, 45
    vel, rho, rows = RT.unsolved_case(w, h)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ex, ey, unsolved = RT.inverse_displacement(xs, ys, vel[0], rho, h)
    per_row = unsolved.sum(axis=1)
    assert set(per_row.tolist()) == {0, w} and int((per_row == w).sum()) == rows and 0 < rows < h
    assert (per_row[h - rows:] == w).all()                         # the lower rows
    assert not ex[unsolved].any() and not ey[unsolved].any() and ex[~unsolved].any()
    src = util.synth_frames(1, h, w, seed=3)
    mats = util.test_matrices(1, w, h, "similarity", seed=2).astype(np.float32)
    got = RT.rolling_unwarp(src, mats, (w, h), vel, rho, (0.2, 0.4, 0.6), "q5")
    plain = R.rolling_warp(src, mats, (w, h), np.zeros((1, 6)), 0.0, (0.2, 0.4, 0.6), "q5")
    assert got[3].tolist() == [rows * w]
    assert np.array_equal(_bits(got[0][0][h - rows:]), _bits(plain[0][0][h - rows:]))      # matrix alone
    assert not np.array_equal(got[0][0][:h - rows], plain[0][0][:h - rows])


# ---- 4. parse_block ------------------------------------------------------------------------------------------------------------
def _block(n=3, readout=0.7, seed=0):
    from vstab_amd import rolling_shutter as rs

    vel = np.random.default_rng(seed).uniform(-8, 8, (n, 6))
    vel[0, 0] = 1.0 / 3.0
    vel[1, 2] = 5e-324                                             # the smallest subnormal
    vel[2 % n, 5] = -1.2345678901234567e100                        # 17 significant digits
    return rs.meta_block(readout, "given", None, vel, (W, H)), vel


def test_velocities_survive_json_exactly(pkg):
    from vstab_amd import rolling_shutter as rs

    block, vel = _block()
    meta = json.loads(json.dumps({"rolling_shutter": block}))
    readout, got = rs.parse_block(meta, 3)
    assert readout == 0.7 and got.dtype == np.float64 and got.shape == (3, 6) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got.view(np.uint64), vel.view(np.uint64))
    assert rs.parse_block({"rolling_shutter": rs.meta_block(0.0, "not_observable", None, vel, (W, H))}, 3)[0] == 0.0
    assert rs.parse_block({"rolling_shutter": rs.meta_block(-1.0, "given", None, np.zeros((0, 6)), (W, H))}, 0)[1].shape == (0, 6)


def test_parse_block_refusals(pkg):
    from vstab_amd import rolling_shutter as rs

    good, _ = _block()

    def broken(**kw):
        return {"rolling_shutter": dict(json.loads(json.dumps(good)), **kw)}

    for meta in ({}, {"rolling_shutter": None}, {"rolling_shutter": [1]}, None, "x"):
        with pytest.raises(ValueError, match=r"needs meta\['rolling_shutter'\]"):
            rs.parse_block(meta, 3)
    for version in (2, None, "1", True):
        with pytest.raises(ValueError, match=r"\['version'\] is .*expected 1"):
            rs.parse_block(broken(version=version), 3)
    for readout in (1.5, -1.0001, float("nan"), float("inf"), None, "0.7", True):
        with pytest.raises(ValueError, match=r"\['readout'\] is .*expected a number in \[-1, 1\]"):
            rs.parse_block(broken(readout=readout), 3)
    with pytest.raises(ValueError, match=r"\['velocity'\] is of shape \[3, 6\]; expected \[4\]\[6\]"):
        rs.parse_block(broken(), 4)
    with pytest.raises(ValueError, match=r"\['velocity'\] is of shape \[3, 5\]; expected \[3\]\[6\]"):
        rs.parse_block(broken(velocity=np.zeros((3, 5)).tolist()), 3)
    for bad in (None, "x", [[0.0] * 6, [0.0] * 5, [0.0] * 6], [["a"] * 6] * 3):
        with pytest.raises(ValueError, match=r"\['velocity'\] is .*expected \[3\]\[6\] finite numbers"):
            rs.parse_block(broken(velocity=bad), 3)
    for bad in (float("nan"), float("inf")):
        meta = broken()
        meta["rolling_shutter"]["velocity"][1][2] = bad
        with pytest.raises(ValueError, match=r"\['velocity'\] is .*expected \[3\]\[6\] finite numbers"):
            rs.parse_block(meta, 3)
    del good["velocity"]
    with pytest.raises(ValueError, match=r"\['velocity'\]"):
        rs.parse_block({"rolling_shutter": good}, 3)


# ---- 5. refusals before any GPU use ----------------------------------------------------------------------------------------------
def _flow_like_meta(n, size, out_size, readout=0.7, with_block=True):
    from vstab_amd import host_math as hm
    from vstab_amd import meta_v2
    from vstab_amd import rolling_shutter as rs

    mats = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    mats[:, 0, 2] = np.arange(n, dtype=np.float32)
    meta = {"stabilization_warp": hm._build_stabilization_warp_meta(source_size=size, output_size=out_size, framing_mode="crop_and_pad",
                                                                   applied_matrices=list(mats)),
            "motion_meta": meta_v2.applied_motion_meta_from_arrays(mats, size, out_size, 16.0, "flow")}
    if with_block:
        meta["rolling_shutter"] = rs.meta_block(readout, "given", None, np.tile(VELOCITY, (n, 1)), size)
    return meta


def _no_gpu(monkeypatch):
    from vstab_amd import native

    def boom(*a, **k):
        raise AssertionError("the GPU context was asked for")

    monkeypatch.setattr(native, "default_context", boom)


def test_apply_motion_rolling_refusals(pkg, monkeypatch):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import distributed
    from vstab_amd import host_math as hm

    _no_gpu(monkeypatch)
    n, size = 3, (64, 40)
    context = hm._normalize_video_input(np.zeros((n, size[1], size[0], 3), np.float32))
    meta = _flow_like_meta(n, size, size)
    for bad in (1, 0, None, "yes", 0.7, np.bool_(True)):
        with pytest.raises(ValueError, match=r"rolling=.*expected True or False"):
            ap.apply_motion(context, meta, RGB, rolling=bad)
    with pytest.raises(ValueError, match="rolling=True is not supported with bicubic interpolation"):
        ap.apply_motion(context, meta, RGB, interpolation="bicubic", rolling=True)
    with pytest.raises(ValueError, match="rolling=True is not supported with motion_blur=0.5"):
        ap.apply_motion(context, meta, RGB, motion_blur=0.5, rolling=True)
    with pytest.raises(ValueError, match="rolling=True is not supported with framing_mode 'crop'"):
        ap.apply_motion(context, meta, RGB, framing_mode="crop", rolling=True)
    with pytest.raises(ValueError, match="rolling=True is not supported with mesh=True"):
        ap.apply_motion(context, meta, RGB, mesh=True, rolling=True)
    inverse_only = {k: v for k, v in meta.items() if k != "motion_meta"}
    with pytest.raises(ValueError, match="rolling=True restores with framing_mode 'crop_and_pad' only"):
        ap.apply_motion(context, inverse_only, RGB, framing_mode="expand", rolling=True)
    with pytest.raises(ValueError, match=r"needs meta\['rolling_shutter'\]"):
        ap.apply_motion(context, _flow_like_meta(n, size, size, with_block=False), RGB, rolling=True)
    short = _flow_like_meta(n, size, size)
    short["rolling_shutter"]["velocity"] = short["rolling_shutter"]["velocity"][:2]
    with pytest.raises(ValueError, match=r"\['velocity'\] is of shape \[2, 6\]; expected \[3\]\[6\]"):
        ap.apply_motion(context, short, RGB, rolling=True)
    sharded = dict(framing_mode="crop_and_pad")
    with pytest.raises(ValueError, match="apply_motion_sharded does not support rolling=True"):
        distributed.apply_motion_sharded(None, np.zeros((n, size[1], size[0], 3), np.float32), 0, n, meta, RGB, rolling=True, **sharded)
    with pytest.raises(ValueError, match=r"rolling=1: expected True or False"):
        distributed.apply_motion_sharded(None, np.zeros((n, size[1], size[0], 3), np.float32), 0, n, meta, RGB, rolling=1, **sharded)


def test_the_direction_follows_the_resolved_block(pkg):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    n, size, big = 3, (64, 40), (80, 50)
    context = hm._normalize_video_input(np.zeros((n, size[1], size[0], 3), np.float32))
    # an expand run: its stabilized frames resolve the inverse, whose OUTPUT canvas is the run's source
    meta = _flow_like_meta(n, size, big)
    stabilized = hm._normalize_video_input(np.zeros((n, big[1], big[0], 3), np.float32))
    motion, derived = ap._resolve_motion_and_origin(meta, stabilized)
    replay = ap._rolling_replay(meta, motion, derived, "crop_and_pad")
    assert derived and replay.direction == "inverse" and replay.readout == 0.7 and replay.velocity.shape == (n, 6)
    assert motion.output_size == size
    motion, derived = ap._resolve_motion_and_origin(meta, context)
    for framing in ("crop_and_pad", "expand"):
        replay = ap._rolling_replay(meta, motion, derived, framing)
        assert not derived and replay.direction == "forward" and np.array_equal(replay.velocity, np.tile(VELOCITY, (n, 1)))
    assert isinstance(replay, ap.RollingReplay)


# ---- 6. the public surface ---------------------------------------------------------------------------------------------------------
def test_symbols_in_header_exports_and_documents(pkg):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import distributed
    from vstab_amd import native
    from vstab_amd import rolling_shutter as rs

    header = (ROOT / "include" / "vstab.h").read_text()
    name = "vstab_rolling_unwarp_batch"
    assert name in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), name)
    assert re.search(rf"^int {name}\(", header, re.M) and name in (ROOT / "INTEGRATION.md").read_text()
    assert re.search(r"^#define VSTAB_ROLLING_UNWARP_MIN_DET 0\.25$", header, re.M) and RT.MIN_DET == 0.25
    assert re.search(r"^#define VSTAB_ABI_VERSION 1$", header, re.M)
    sig = inspect.signature(native.Context.rolling_unwarp_batch).parameters
    assert list(sig)[1:6] == ["frames", "matrices", "out_size", "velocity", "readout"]
    assert sig["subpix"].default is None and sig["want_mask"].default is True
    assert sig["want_count"].default is False and sig["want_unsolved"].default is False
    for fn in (ap.apply_motion, distributed.apply_motion_sharded):
        p = inspect.signature(fn).parameters["rolling"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "Motion Apply replay" not in (rs.__doc__ or "") and "Motion Apply replay and the inverse" not in (ROOT / "README.md").read_text()
    for doc, words in (("README.md", ("Rolling shutter round trip", "video_stabilizer_motion_apply_rolling", "rolling=True")),
                       ("DESIGN.md", ("8l", "vstab_rolling_unwarp_batch")),
                       ("INTEGRATION.md", ("VideoStabilizerAmdRollingApplyExtension",))):
        text = (ROOT / doc).read_text()
        for word in words:
            assert word in text, (doc, word)


def test_node_sockets_and_where_it_is_listed(pkg):
    import vstab_amd
    from vstab_amd import nodes

    schema = nodes.VideoStabilizerMotionApplyRolling.define_schema()
    mesh = nodes.VideoStabilizerMotionApplyMesh.define_schema()
    assert schema.node_id == "video_stabilizer_motion_apply_rolling"
    assert schema.display_name == "Video Stabilizer Motion Apply (Rolling Shutter)"
    assert [i.id for i in schema.inputs] == ["frames", "meta", "framing_mode", "padding_color"]
    assert [(i.kind, i.options) for i in schema.inputs] == [(i.kind, i.options) for i in mesh.inputs]
    assert [o.id for o in schema.outputs] == [o.id for o in mesh.outputs]
    options = schema.inputs[2].options
    assert list(options["options"] if isinstance(options, dict) else options) == ["crop_and_pad", "expand"]
    before = asyncio.run(nodes.VideoStabilizerAmdRollingExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdRollingApplyExtension().get_node_list())
    assert listed == before + [nodes.VideoStabilizerMotionApplyRolling] and nodes.VideoStabilizerMotionApplyRolling not in before
    assert issubclass(nodes.VideoStabilizerAmdRollingApplyExtension, nodes.VideoStabilizerAmdRollingExtension)
    assert nodes.VideoStabilizerMotionApplyRolling not in nodes.NODE_CLASSES
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension
