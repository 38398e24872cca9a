"""Mesh warp round trip, the parts that need no GPU (include/vstab.h "vstab_mesh_unwarp_batch"; mesh_warp.motion_block /
parse_motion_block; apply_pipeline.apply_motion(mesh=True); flow_pipeline._stabilize_frames(mesh_motion=True)).

  1. the restatement of the inverse rule at zero offsets == the forward restatement at zero offsets, in bits
  2. a coordinate image sent through the forward restatement and back through the inverse one comes back within 1/16 px;
     sent back through the plain inverse it is off by more than 1 px
  3. the meta block: float32 values survive JSON exactly; every refusal of the validator
  4. the refusals of apply_motion(mesh=True) and of mesh_motion=True without mesh_warp, raised before any GPU use
  5. the extension's node list
"""

import asyncio
import json

import numpy as np
import pytest

from tests import mesh_inverse_restatement as RI
from tests import mesh_restatement as R
from tests import util

W, H, VERTS = 320, 180, (17, 10)
ERODE = 12


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def smooth_field(w, h, mw, mh, amp, phase=0.0):
    """A smooth vertex field of amplitude `amp` px: Lipschitz constant about 2 * pi * amp / w (0.1 at amp = w / 64)."""
    vx = np.arange(mw) * (w - 1) / (mw - 1) / w
    vy = np.arange(mh) * (h - 1) / (mh - 1) / h
    X, Y = np.meshgrid(vx, vy)
    off = np.empty((mh, mw, 2), np.float32)
    off[..., 0] = amp * np.sin(2 * np.pi * (0.75 * X + 0.4 * Y) + 0.3 + phase)
    off[..., 1] = amp * np.cos(2 * np.pi * (0.5 * X - 0.6 * Y) + 1.1 + phase)
    return off


def similarity(scale, angle, tx, ty):
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


@pytest.fixture(scope="module")
def round_trip():
    """Coordinate image -> forward mesh warp -> (mesh inverse, plain inverse), all on the restatements.  The third channel
    carries validity: it is 1 where the stabilized frame saw the source, so a restored pixel whose taps all saw it reads 1."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    coord = np.stack([xs, ys, np.ones_like(xs)], -1)[None]
    M = similarity(1.03, 0.02, 4.3, -2.7)
    fwd = M.astype(np.float32)[None]
    inv = np.linalg.inv(fwd[0].astype(np.float64)).astype(np.float32)[None]
    offsets = smooth_field(W, H, VERTS[0], VERTS[1], W / 64.0)[None]
    stab, stab_mask, _ = R.mesh_warp(coord, fwd, (W, H), offsets, (0.0, 0.0, 0.0), "q5")
    stab[..., 2] = 1.0 - stab_mask                                 # validity travels with the pixels
    back, back_mask, _, unconverged = RI.mesh_unwarp(stab, inv, (W, H), offsets, (0.0, 0.0, 0.0), "q5")
    plain, plain_mask, _ = R.mesh_warp(stab, inv, (W, H), np.zeros_like(offsets), (0.0, 0.0, 0.0), "q5")
    valid = (back[0, ..., 2] == 1.0) & (back_mask[0] == 0) & (plain[0, ..., 2] == 1.0) & (plain_mask[0] == 0)
    return dict(coord=coord[0], back=back[0], plain=plain[0], interior=_erode(valid, ERODE), unconverged=unconverged,
                offsets=offsets)


# ---- 1. zero offsets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", ["q5", "exact"])
@pytest.mark.parametrize("kind,size,out_size", [("similarity", (96, 64), (96, 64)), ("perspective", (96, 64), (120, 70)),
                                                ("similarity", (61, 45), (333, 11)), ("horizon", (80, 60), (80, 60))])
def test_zero_offsets_restate_the_plain_warp(subpix, kind, size, out_size):
    w, h = size
    src = util.synth_frames(2, h, w, seed=w)
    mats = util.test_matrices(2, w, h, kind, seed=5).astype(np.float32)
    zero = np.zeros((2, 4, 5, 2), np.float32)
    want = R.mesh_warp(src, mats, out_size, zero, (0.2, 0.4, 0.6), subpix)
    for z in (zero, -zero):                                        # zeros of either sign
        got = RI.mesh_unwarp(src, mats, out_size, z, (0.2, 0.4, 0.6), subpix)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
        assert got[2].tolist() == want[2].tolist() and not got[3].any()


# ---- 2. the round trip ----------------------------------------------------------------------------------------------------------
def test_round_trip_restores_the_coordinates(round_trip):
    """Bound 1/16 px: two Q5 roundings of at most 1/64 px each (forward and back), the 2^-7 stop (L/(1-L) * 2^-7 < 2^-7 at
    L ~ 0.1), and the kink term -- the forward warp's sampling position is piecewise bilinear, and interpolating the
    coordinate image across a cell edge of the mesh bends by at most (change of slope) * (1/2 px)^2 / 2 per axis, with slopes
    of at most L ~ 0.1: 1/64 + 1/64 + 1/128 + ~1/80 < 1/16.  Measured: 0.033 px (plain inverse: 5.0 px)."""
    rt = round_trip
    sel = rt["interior"]
    assert sel.mean() > 0.5
    err = np.abs(rt["back"][..., :2] - rt["coord"][..., :2])[sel]
    plain = np.abs(rt["plain"][..., :2] - rt["coord"][..., :2])[sel]
    print(f"\nround trip {W}x{H}: mesh inverse max {err.max():.4f} px mean {err.mean():.4f} px; "
          f"plain inverse max {plain.max():.3f} px mean {plain.mean():.3f} px; interior {sel.mean():.2f}")
    assert err.max() <= 1.0 / 16.0
    assert plain.max() > 1.0                                       # the test has teeth: the plain inverse misses by pixels
    assert int(rt["unconverged"].sum()) == 0


def test_smooth_field_converges_fast_and_rough_field_does_not(round_trip):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    _, _, unconverged, steps = RI.inverse_displacement(xs, ys, round_trip["offsets"][0], (W, H))
    # |q_{k+1} - q_k| <= amp * L^k with amp = 5 px and L <= 0.15 for this field: below 2^-7 from k = 4 on, the 5th step
    assert not unconverged.any() and steps.max() <= 5 and steps.min() >= 1
    rough = np.random.default_rng(1).uniform(-W / 64.0, W / 64.0, (65, 65, 2)).astype(np.float32)
    _, _, unconverged, steps = RI.inverse_displacement(xs, ys, rough, (W, H))
    assert unconverged.any() and steps.max() == RI.MAX_STEPS       # why the limit and the count exist


# ---- 3. the meta block ----------------------------------------------------------------------------------------------------------
def _meta(offsets, size=(W, H)):
    from vstab_amd import mesh_warp as mw

    return {"mesh_warp": {"cells": [16, 9], "motion": mw.motion_block(offsets, size)}}


def test_offsets_survive_json_exactly(pkg):
    from vstab_amd import mesh_warp as mw

    rng = np.random.default_rng(3)
    off = rng.uniform(-5, 5, (3, 10, 17, 2)).astype(np.float32)
    off[0, 0, 0] = (np.float32(1e-38), np.float32(-3.4e38))        # a subnormal neighbour and a huge value
    off[1, 2, 3] = (np.float32(0.1), np.float32(-0.0))
    meta = json.loads(json.dumps(_meta(off)))
    block = meta["mesh_warp"]["motion"]
    assert block["version"] == 1 and block["domain_size"] == [W, H] and block["vertices"] == [17, 10] and block["frame_count"] == 3
    parsed = mw.parse_motion_block(meta, 3, (W, H))
    assert parsed.offsets.dtype == np.float32 and np.array_equal(_bits(parsed.offsets), _bits(off))
    assert parsed.domain_size == (W, H) and parsed.vertices == (17, 10)


def test_validator_refusals(pkg):
    from vstab_amd import mesh_warp as mw

    off = np.zeros((2, 3, 4, 2), np.float32)
    good = _meta(off)

    def broken(**kw):
        meta = json.loads(json.dumps(good))
        meta["mesh_warp"]["motion"].update(kw)
        return meta

    for meta in ({}, {"mesh_warp": {"cells": [16, 9]}}, None):
        with pytest.raises(ValueError, match="no mesh_warp.motion block"):
            mw.parse_motion_block(meta)
    with pytest.raises(ValueError, match=r"motion\.version must be 1"):
        mw.parse_motion_block(broken(version=2))
    with pytest.raises(ValueError, match=r"motion\.domain_size must be a pair of integers"):
        mw.parse_motion_block(broken(domain_size=[W]))
    with pytest.raises(ValueError, match=r"motion\.frame_count is 2, the motion describes 3 frame"):
        mw.parse_motion_block(good, 3, (W, H))
    with pytest.raises(ValueError, match=r"motion\.domain_size \[320, 180\] does not match the motion's canvas \[480, 270\]"):
        mw.parse_motion_block(good, 2, (480, 270))
    with pytest.raises(ValueError, match=r"motion\.vertices \[66, 3\] outside 2\.\.65"):
        mw.parse_motion_block(broken(vertices=[66, 3]))
    with pytest.raises(ValueError, match=r"motion\.vertices \[4, 1\] outside 2\.\.65"):
        mw.parse_motion_block(broken(vertices=[4, 1]))
    with pytest.raises(ValueError, match=r"motion\.offsets has shape \[2, 3, 4, 2\], expected \[2, 3, 5, 2\]"):
        mw.parse_motion_block(broken(vertices=[5, 3]))
    with pytest.raises(ValueError, match=r"motion\.offsets has shape"):
        mw.parse_motion_block(broken(frame_count=3))
    for bad in (float("nan"), float("inf"), 1e39):                 # 1e39 is finite as a double, not as a float32
        meta = broken()
        meta["mesh_warp"]["motion"]["offsets"][1][2][3][0] = bad
        with pytest.raises(ValueError, match=r"motion\.offsets must contain finite"):
            mw.parse_motion_block(meta)
    meta = broken()
    meta["mesh_warp"]["motion"]["offsets"][0][0] = "x"
    with pytest.raises(ValueError, match=r"motion\.offsets"):
        mw.parse_motion_block(meta)
    assert mw.parse_motion_block(good, 2, (W, H)).offsets.shape == (2, 3, 4, 2)


# ---- 4. refusals before any GPU use ----------------------------------------------------------------------------------------------
def _flow_like_meta(n, size, out_size, with_motion=True):
    from vstab_amd import host_math as hm
    from vstab_amd import meta_v2
    from vstab_amd import mesh_warp as mw

    mats = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    mats[:, 0, 2] = np.arange(n, dtype=np.float32)
    meta = {"stabilization_warp": hm._build_stabilization_warp_meta(source_size=size, output_size=out_size, framing_mode="crop_and_pad",
                                                                   applied_matrices=list(mats)),
            "motion_meta": meta_v2.applied_motion_meta_from_arrays(mats, size, out_size, 16.0, "flow"),
            "mesh_warp": {"cells": [3, 2]}}
    if with_motion:
        meta["mesh_warp"]["motion"] = mw.motion_block(np.zeros((n, 3, 4, 2), np.float32), size)
    return meta


def _no_gpu(monkeypatch):
    from vstab_amd import native

    def boom(*a, **k):
        raise AssertionError("the GPU context was asked for")

    monkeypatch.setattr(native, "default_context", boom)


def test_apply_motion_mesh_refusals(pkg, monkeypatch):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    _no_gpu(monkeypatch)
    n, size = 3, (64, 40)
    frames = np.zeros((n, size[1], size[0], 3), np.float32)
    context = hm._normalize_video_input(frames)
    meta = _flow_like_meta(n, size, size)
    rgb = (127, 127, 127)
    with pytest.raises(ValueError, match="mesh=True is not supported with bicubic interpolation"):
        ap.apply_motion(context, meta, rgb, interpolation="bicubic", mesh=True)
    with pytest.raises(ValueError, match="mesh=True is not supported with motion_blur=0.5"):
        ap.apply_motion(context, meta, rgb, motion_blur=0.5, mesh=True)
    with pytest.raises(ValueError, match="mesh=True is not supported with framing_mode 'crop'"):
        ap.apply_motion(context, meta, rgb, framing_mode="crop", mesh=True)
    inverse_only = {k: v for k, v in meta.items() if k != "motion_meta"}
    with pytest.raises(ValueError, match="mesh=True restores with framing_mode 'crop_and_pad' only"):
        ap.apply_motion(context, inverse_only, rgb, framing_mode="expand", mesh=True)
    with pytest.raises(ValueError, match="no mesh_warp.motion block"):
        ap.apply_motion(context, _flow_like_meta(n, size, size, with_motion=False), rgb, mesh=True)
    short = _flow_like_meta(n, size, size)
    short["mesh_warp"]["motion"] = _meta(np.zeros((n - 1, 3, 4, 2), np.float32), size)["mesh_warp"]["motion"]
    with pytest.raises(ValueError, match=r"motion\.frame_count is 2, the motion describes 3 frame"):
        ap.apply_motion(context, short, rgb, mesh=True)
    # an expand run: the stabilized canvas differs from the domain; its frames resolve the inverse, whose OUTPUT is the domain
    big = (80, 50)
    expand_meta = _flow_like_meta(n, size, big)
    stabilized = hm._normalize_video_input(np.zeros((n, big[1], big[0], 3), np.float32))
    motion, derived = ap._resolve_motion_and_origin(expand_meta, stabilized)
    assert derived and ap._mesh_replay(expand_meta, motion, derived, "crop_and_pad").direction == "inverse"
    motion, derived = ap._resolve_motion_and_origin(expand_meta, context)
    assert not derived and ap._mesh_replay(expand_meta, motion, derived, "expand").direction == "forward"
    wrong = _flow_like_meta(n, size, big)
    wrong["mesh_warp"]["motion"]["domain_size"] = [big[0], big[1]]
    with pytest.raises(ValueError, match=r"motion\.domain_size \[80, 50\] does not match the motion's canvas \[64, 40\]"):
        ap.apply_motion(context, wrong, rgb, mesh=True)


def test_mesh_motion_needs_mesh_warp(pkg, monkeypatch):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    _no_gpu(monkeypatch)
    context = hm._normalize_video_input(np.zeros((3, 40, 64, 3), np.float32))
    with pytest.raises(ValueError, match="mesh_motion=True needs mesh_warp"):
        fp._stabilize_frames(context, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0, mesh_motion=True)


# ---- 5. the nodes ----------------------------------------------------------------------------------------------------------------
def test_extension_lists_the_two_nodes(pkg):
    import vstab_amd
    from vstab_amd import nodes

    base = asyncio.run(nodes.VideoStabilizerAmdMeshExtension().get_node_list())
    got = asyncio.run(nodes.VideoStabilizerAmdMeshApplyExtension().get_node_list())
    assert got[:len(base)] == base and got[len(base):] == [nodes.VideoStabilizerFlowMeshMotion, nodes.VideoStabilizerMotionApplyMesh]
    assert issubclass(nodes.VideoStabilizerAmdMeshApplyExtension, nodes.VideoStabilizerAmdMeshExtension)
    assert not set(got[len(base):]) & set(nodes.NODE_CLASSES)
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension
    flow = nodes.VideoStabilizerFlowMeshMotion.define_schema()
    assert flow.node_id == "video_stabilizer_flow_mesh_motion"
    assert [i.id for i in flow.inputs] == [i.id for i in nodes.VideoStabilizerFlowMesh.define_schema().inputs]
    apply_schema = nodes.VideoStabilizerMotionApplyMesh.define_schema()
    assert apply_schema.node_id == "video_stabilizer_motion_apply_mesh"
    assert [i.id for i in apply_schema.inputs] == ["frames", "meta", "framing_mode", "padding_color"]
    options = apply_schema.inputs[2].options           # the stand-in for comfy_api keeps a socket's keywords in a dict
    assert list(options["options"] if isinstance(options, dict) else options) == ["crop_and_pad", "expand"]
