"""CPU: the subject lock's rule on its NumPy restatement (tests/subject_restatement.py, which the GPU tests hold the kernel
to exactly), and the host side (subject_lock.py): centroids, the fit table, the meta block, the refusals, node, header."""

import asyncio
import ctypes as C
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import subject_restatement as R
from tests.util import synth_frames

ROOT = Path(__file__).resolve().parents[1]


# ---- the rule, on the restatement -----------------------------------------------------------------------------------------
def test_translating_a_blob_moves_the_centroid_by_exactly_that_vector():
    rng = np.random.default_rng(1)
    blob = (rng.uniform(0, 1, (9, 11)) < 0.6).astype(np.float32)
    blob[4, 5] = 1.0
    base = np.zeros((1, 40, 60), np.float32)
    base[0, 10:19, 20:31] = blob
    s0, b0 = R.moments(base)
    for dx, dy in ((0, 0), (7, -3), (-20, 21), (29, -10)):
        moved = np.zeros_like(base)
        moved[0, 10 + dy:19 + dy, 20 + dx:31 + dx] = blob
        s, b = R.moments(moved)
        assert s[0, 0] == s0[0, 0]
        # sum / count moves by the vector exactly: compared as integers, sum' = sum + count * d
        assert s[0, 1] == s0[0, 1] + s0[0, 0] * dx and s[0, 2] == s0[0, 2] + s0[0, 0] * dy
        assert b[0].tolist() == (b0[0] + np.array([dx, dy, dx, dy])).tolist()


def test_an_empty_frame_gives_four_minus_one():
    s, b = R.moments(np.zeros((2, 5, 7), np.float32))
    assert s.tolist() == [[0, 0, 0]] * 2 and b.tolist() == [[-1, -1, -1, -1]] * 2
    assert s.dtype == np.int64 and b.dtype == np.int32


def test_nan_is_not_subject_and_inf_is():
    m = np.zeros((1, 3, 4), np.float32)
    m[0, 0, 1] = np.nan
    m[0, 1, 2] = np.inf
    m[0, 2, 3] = -np.inf
    m[0, 2, 0] = 0.5                      # the threshold itself is not subject
    s, b = R.moments(m)
    assert s.tolist() == [[1, 2, 1]] and b.tolist() == [[2, 1, 2, 1]]
    m[0, 2, 0] = np.nextafter(np.float32(0.5), np.float32(1.0))
    assert np.float32(0.50000006) == m[0, 2, 0]
    s, b = R.moments(m)
    assert s.tolist() == [[2, 2, 3]] and b.tolist() == [[0, 1, 2, 2]]


def test_a_disc_on_integers_is_centred_exactly():
    s, b = R.moments(R.disc(96, 160, 70, 40, 9)[None])
    assert s[0, 1] == 70 * s[0, 0] and s[0, 2] == 40 * s[0, 0] and b.tolist() == [[61, 31, 79, 49]]


# ---- centroids ---------------------------------------------------------------------------------------------------------
def _moments_of(centres, areas, size=(160, 96)):
    """sums / bbox as the kernel would report a blob of `area` pixels around (x, y); area 0: no subject."""
    sums = np.array([[a, a * x, a * y] for (x, y), a in zip(centres, areas)], np.int64)
    bbox = np.array([[x - 2, y - 2, x + 2, y + 2] if a else [-1] * 4 for (x, y), a in zip(centres, areas)], np.int32)
    return sums, bbox


def test_centroids_interpolate_gaps_and_hold_the_ends(pkg):
    from vstab_amd import subject_lock as sl

    centres = [(0, 0), (10, 20), (0, 0), (0, 0), (40, 50), (43, 47), (0, 0)]
    areas = [0, 100, 0, 0, 800, 400, 0]
    c, area, measured = sl.centroids(*_moments_of(centres, areas), (160, 96))
    assert measured.tolist() == [False, True, False, False, True, True, False]
    assert c.dtype == np.float64 and area.dtype == np.float64
    assert c[0].tolist() == [10.0, 20.0] and c[6].tolist() == [43.0, 47.0]              # held at the ends
    assert area[0] == 100.0 and area[6] == 400.0
    assert np.allclose(c[2], [20.0, 30.0], rtol=0, atol=1e-12) and np.allclose(c[3], [30.0, 40.0], rtol=0, atol=1e-12)
    assert np.allclose(area[2:4], [200.0, 400.0], rtol=1e-12)                           # log(area) is what is interpolated
    assert c[[1, 4, 5]].tolist() == [[10.0, 20.0], [40.0, 50.0], [43.0, 47.0]] and area[[1, 4, 5]].tolist() == [100.0, 800.0, 400.0]


def test_centroids_of_a_clip_without_a_subject_raise(pkg):
    from vstab_amd import subject_lock as sl

    with pytest.raises(ValueError, match=r"subject_mask holds no subject pixel .* in any of its 3 frames"):
        sl.centroids(np.zeros((3, 3), np.int64), np.full((3, 4), -1, np.int32), (160, 96))


# ---- the fit table -----------------------------------------------------------------------------------------------------
def test_table_rows_pass_through_selection_and_the_rescale(pkg):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import native
    from vstab_amd import subject_lock as sl

    size, work = (1920, 1080), (960, 540)
    centres = [(900, 500), (912, 493), (905, 520), (930, 511)]
    areas = [400, 400, 900, 900]
    c, area, measured = sl.centroids(*_moments_of(centres, areas, size), size)
    table = sl.transition_table(c, area, measured, size, work)
    assert table.shape == (3, 3) and table.dtype == native.FIT_DTYPE
    assert table["computed"].tolist() == [[1, 1, 0]] * 3 and table["accepted"][:, :2].tolist() == [[1, 1]] * 3
    assert (table["valid_points"][:, :2] == 1).all() and (table["total_points"][:, :2] == 1).all()
    assert (table["residual"] == 0.0).all()
    d = np.diff(np.array(centres, np.float64), axis=0)
    for mode in ("translation", "similarity"):
        mats, modes, confs, resids, active = fp.select_transitions(table, mode)
        assert modes == [mode] * 3 and active == mode and resids == [0.0] * 3
        assert confs == [1.0, 400 / 900, 1.0]
        full, params = native.transitions_to_params(mats, mode, size, work)
        if mode == "translation":
            assert np.array_equal(mats[:, :2, 2], (d * 0.5).astype(np.float32))          # working = full / 2
            assert np.array_equal(mats[:, :2, :2], np.tile(np.eye(2, dtype=np.float32), (3, 1, 1)))
            assert np.allclose(full[:, :2, 2], d, rtol=0, atol=1e-4) and np.allclose(params, d, rtol=0, atol=1e-4)
        else:
            s = np.array([1.0, 1.5, 1.0])
            assert np.array_equal(mats[:, 0, 0], s.astype(np.float32)) and np.array_equal(mats[:, 1, 1], s.astype(np.float32))
            assert (mats[:, 0, 1] == 0).all() and (mats[:, 1, 0] == 0).all()
            c64 = np.array(centres, np.float64)
            assert np.allclose(full[:, :2, 2], c64[1:] - s[:, None] * c64[:-1], rtol=0, atol=1e-3)
    # estimated at full size (no working resolution): the matrices are the full-resolution ones
    plain = sl.transition_table(c, area, measured, size, None)
    assert np.array_equal(plain["matrix"][:, 0].reshape(3, 3, 3)[:, :2, 2], d.astype(np.float32))


def test_a_disc_scaled_to_four_times_the_area_gives_s_two(pkg):
    from vstab_amd import subject_lock as sl

    sums, bbox = _moments_of([(80, 48), (80, 48)], [317, 4 * 317])
    c, area, measured = sl.centroids(sums, bbox, (160, 96))
    table = sl.transition_table(c, area, measured, (160, 96), None)
    m = table["matrix"][0, 1].reshape(3, 3)
    assert m[0, 0] == 2.0 and m[1, 1] == 2.0 and m[0, 1] == 0.0 and m[1, 0] == 0.0
    assert m[0, 2] == 80 - 2 * 80 and m[1, 2] == 48 - 2 * 48                            # the centroid is the fixed point
    assert table["confidence"][0, 1] == 0.25 and table["confidence"][0, 0] == 0.25


def test_confidence_is_zero_exactly_where_a_pair_touches_an_interpolated_frame(pkg):
    from vstab_amd import subject_lock as sl

    n = 12
    areas = [300] * n
    areas[4] = areas[5] = 0
    centres = [(40 + 3 * k, 30 + k) for k in range(n)]
    sums, bbox = _moments_of(centres, areas)
    c, area, measured = sl.centroids(sums, bbox, (160, 96))
    table = sl.transition_table(c, area, measured, (160, 96), None)
    conf = table["confidence"][:, 0]
    assert [k for k in range(n - 1) if conf[k] == 0.0] == [3, 4, 5] and (np.delete(conf, [3, 4, 5]) == 1.0).all()
    assert np.array_equal(table["confidence"][:, 1], conf)
    # the transition is carried all the same: a straight line through the gap
    assert np.allclose(table["matrix"][:, 0].reshape(-1, 3, 3)[:, :2, 2], [[3.0, 1.0]] * (n - 1), rtol=0, atol=1e-5)
    block = sl.meta_block(sums, bbox, c, measured, (160, 96))
    assert block["version"] == 1 and block["mask_frames"] == n and block["frames_without_subject"] == 2
    assert block["interpolated"] == [4, 5] and block["frames_touching_border"] == 0
    assert block["area_fraction_min"] == block["area_fraction_max"] == 300 / (160 * 96)
    assert np.allclose(block["centroid"], centres, rtol=0, atol=1e-9) and json.loads(json.dumps(block)) == block


def test_meta_block_counts_frames_whose_box_touches_the_border(pkg):
    from vstab_amd import subject_lock as sl

    mask = np.zeros((5, 20, 30), np.float32)
    mask[0, 5:8, 5:8] = 1          # inside
    mask[1, 0, 10] = 1             # row 0
    mask[2, 10, 0] = 1             # column 0
    mask[3, 19, 10] = 1            # last row
    mask[4, 10, 29] = 1            # last column
    sums, bbox = R.moments(mask)
    c, area, measured = sl.centroids(sums, bbox, (30, 20))
    block = sl.meta_block(sums, bbox, c, measured, (30, 20))
    assert block["frames_touching_border"] == 4 and block["frames_without_subject"] == 0 and block["interpolated"] == []
    assert block["area_fraction_min"] == 1 / 600 and block["area_fraction_max"] == 9 / 600
    assert block["centroid"][0] == [6.0, 6.0]


# ---- refusals: every one names its value, before any GPU work ----------------------------------------------------------------
def test_check_request_names_the_offending_value(pkg):
    from vstab_amd import subject_lock as sl

    mask = np.zeros((4, 16, 24), np.float32)
    assert sl.check_request(None, "similarity", "flow") is False
    assert sl.check_request(mask, "translation") is True and sl.check_request(mask, "similarity", "subject", 4, (24, 16)) is True
    with pytest.raises(ValueError, match="subject_mask needs estimator='subject', got estimator='flow'"):
        sl.check_request(mask, "translation", "flow")
    with pytest.raises(ValueError, match="estimator='subject' needs subject_mask"):
        sl.check_request(None, "translation", "subject")
    with pytest.raises(ValueError, match="transform_mode='perspective' is not supported .* determine no homography"):
        sl.check_request(mask, "perspective")
    with pytest.raises(ValueError, match="transform_mode='affine' is not supported"):
        sl.check_request(mask, "affine")
    with pytest.raises(ValueError, match="subject_mask must be a float array or tensor .*got list"):
        sl.check_request([[0.0]], "translation")
    with pytest.raises(ValueError, match="subject_mask must be floating point .* got dtype uint8"):
        sl.check_request(mask.astype(np.uint8), "translation")
    with pytest.raises(ValueError, match=r"subject_mask of shape \(16, 24\) is not \[N,H,W\].*one mask for the whole clip has no motion"):
        sl.check_request(mask[0], "translation")
    with pytest.raises(ValueError, match=r"subject_mask of shape \(1, 16, 24\) holds one mask for a clip of 4 frames: one mask has no motion"):
        sl.check_request(mask[:1], "translation", "subject", 4, (24, 16))
    for bad in (mask[:3], np.zeros((4, 24, 16), np.float32), np.zeros((4, 16, 24, 1), np.float32)):
        with pytest.raises(ValueError, match=r"subject_mask of shape \(.*\) (does not match the clip: expected \[4,16,24\]|is not \[N,H,W\])"):
            sl.check_request(bad, "translation", "subject", 4, (24, 16))


def test_check_pipeline_names_the_offending_value(pkg):
    from vstab_amd import scene_cuts
    from vstab_amd import subject_lock as sl

    sl.check_pipeline(0, None, None)
    sl.check_pipeline(0, [6], None)
    sl.check_pipeline(0, scene_cuts.check_request([6]), None)
    with pytest.raises(ValueError, match="temporal_fill=2 is not supported with estimator 'subject': .*the subject's"):
        sl.check_pipeline(2)
    for auto in ("auto", scene_cuts.check_request("auto")):
        with pytest.raises(ValueError, match="scene_cuts='auto' is not supported with estimator 'subject': the residual score"):
            sl.check_pipeline(0, auto)
    with pytest.raises(ValueError, match="estimation_mask is not supported with estimator 'subject'"):
        sl.check_pipeline(0, None, np.zeros((2, 2), np.float32))


def test_pipeline_refuses_before_any_gpu_work(pkg):
    """No GPU here: every one of these has to raise its ValueError in front of the first device call."""
    from vstab_amd import distributed, flow_pipeline, mesh_warp
    from vstab_amd import host_math as hm

    p = inspect.signature(flow_pipeline._stabilize_frames).parameters["subject_mask"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert flow_pipeline._META_SOURCE["subject"] == "estimated_subject" and "subject" in flow_pipeline._ESTIMATORS
    assert flow_pipeline._backend_fields("subject") == {"flow_backend": "subject_mask", "flow_fallback_reason": None}
    assert "subject" in flow_pipeline._MASK_LIMITS and "subject" in mesh_warp._ESTIMATOR_LIMITS
    assert not flow_pipeline.device_plan_applies("subject", "crop_and_pad", "translation", 12)

    context = hm._normalize_video_input(synth_frames(3, 16, 24, seed=1))
    mask = np.zeros((3, 16, 24), np.float32)
    mask[:, 4:8, 4:8] = 1.0

    def run(transform="translation", estimator="subject", **kw):
        return flow_pipeline._stabilize_frames(context, "crop_and_pad", transform, True, 1.0, 0.5, 0.6, (0, 0, 0), 16.0,
                                               estimator=estimator, **kw)

    with pytest.raises(ValueError, match="estimator='subject' needs subject_mask"):
        run()
    for estimator in ("flow", "classic", "flow_tvl1"):
        with pytest.raises(ValueError, match=f"subject_mask needs estimator='subject', got estimator='{estimator}'"):
            run(estimator=estimator, subject_mask=mask)
    with pytest.raises(ValueError, match="transform_mode='perspective' is not supported with estimator 'subject'"):
        run("perspective", subject_mask=mask)
    with pytest.raises(ValueError, match="temporal_fill=2 is not supported with estimator 'subject'"):
        run(subject_mask=mask, temporal_fill=2)
    with pytest.raises(ValueError, match="scene_cuts='auto' is not supported with estimator 'subject'"):
        run(subject_mask=mask, scene_cuts="auto")
    with pytest.raises(ValueError, match="estimation_mask is not supported with estimator 'subject'"):
        run(subject_mask=mask, estimation_mask=mask)
    with pytest.raises(ValueError, match="mesh_warp is not supported with estimator 'subject'"):
        run(subject_mask=mask, mesh_warp=True)
    with pytest.raises(ValueError, match=r"subject_mask of shape \(1, 16, 24\) holds one mask for a clip of 3 frames"):
        run(subject_mask=mask[:1])
    with pytest.raises(ValueError, match=r"subject_mask of shape \(3, 24, 16\) does not match the clip: expected \[3,16,24\]"):
        run(subject_mask=np.zeros((3, 24, 16), np.float32))
    with pytest.raises(ValueError, match="stabilize_sharded does not support estimator 'subject'"):
        distributed.stabilize_sharded(None, None, 3, "crop_and_pad", "translation", True, 1.0, 0.5, 0.6, (0, 0, 0), 16.0,
                                      estimator="subject")
    # the one-frame bypass ignores the keyword, as it ignores every extra
    one = hm._normalize_video_input(synth_frames(1, 16, 24, seed=1))
    out = flow_pipeline._stabilize_frames(one, "crop_and_pad", "translation", True, 1.0, 0.5, 0.6, (0, 0, 0), 16.0,
                                          estimator="subject", subject_mask=mask)
    assert out.meta["frames"] == 1 and out.meta["flow_backend"] == "subject_mask" and "subject_lock" not in out.meta
    assert out.meta["motion_meta"]["source"] == "estimated_subject"


# ---- node, header -----------------------------------------------------------------------------------------------------------
def test_node_is_listed_by_the_new_extension_only(pkg):
    from vstab_amd import nodes

    node = nodes.VideoStabilizerFlowSubject
    assert len(nodes.NODE_CLASSES) == 6 and node not in nodes.NODE_CLASSES
    assert issubclass(nodes.VideoStabilizerAmdSubjectExtension, nodes.VideoStabilizerAmdZoomExtension)
    before = asyncio.run(nodes.VideoStabilizerAmdZoomExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdSubjectExtension().get_node_list())
    assert node not in before and listed == before + [node]
    entry = asyncio.run(pkg.comfy_entrypoint())
    assert type(entry) is nodes.VideoStabilizerAmdMaskedExtension and node not in asyncio.run(entry.get_node_list())
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_subject" and schema.display_name == "Video Stabilizer Flow (Subject Lock)"
    flow = nodes.VideoStabilizerFlow.define_schema()
    assert [s.id for s in schema.inputs] == [s.id for s in flow.inputs] + ["subject_mask"]
    assert schema.inputs[-1].kind == "Mask"
    mode = next(s for s in schema.inputs if s.id == "transform_mode")
    assert mode.options["options"] == ["translation", "similarity"] and mode.options["default"] in mode.options["options"]
    assert [(s.id, s.kind) for s in schema.outputs] == [(s.id, s.kind) for s in flow.outputs]
    assert list(inspect.signature(node.execute).parameters) == [s.id for s in schema.inputs]


def test_header_declares_what_native_binds_and_the_library_exports(pkg):
    from vstab_amd import native

    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "vstab.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+vstab_mask_moments_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/vstab.h does not declare vstab_mask_moments_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = native._SIGNATURES["vstab_mask_moments_batch"]
    assert res is C.c_int and len(params) == len(args) == 7
    for ptxt, a in zip(params, args):
        assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
    assert "vstab_mask_moments_batch" in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert hasattr(lib, "vstab_mask_moments_batch") and hasattr(native.Context, "mask_moments_batch")
    assert lib.vstab_abi_version() == 1
    assert "vstab_subject.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    # the argument checks come in front of any GPU work, under the function's name
    raw = C.CDLL(str(native.LIB_PATH))
    raw.vstab_last_error.restype = C.c_char_p
    fn = raw.vstab_mask_moments_batch
    fn.argtypes, fn.restype = args, C.c_int
    assert fn(None, None, 1, 1, 1, None, None) != 0
    assert raw.vstab_last_error().decode().startswith("vstab_mask_moments_batch: NULL context")
