"""CPU: the coverage-extent rule on its NumPy restatement (tests/dynamic_zoom_restatement.py, which the GPU tests hold the
kernel to exactly) and the host side of the dynamic zoom: required zoom, envelope, zoom matrices, request checks, the
zero-padding claim on the clips of the GPU pipeline tests, node, header."""

import asyncio
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import dynamic_zoom_restatement as R
from tests.util import similarity

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def dz(pkg):
    from vstab_amd import dynamic_zoom

    return dynamic_zoom


# ---- the rule, on the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size,src_size", [((7, 5), (7, 5)), ((8, 6), (5, 9)), ((2, 2), (3, 3)), ((9, 4), (6, 6))])
def test_restatement_equals_the_brute_force_loop(out_size, src_size):
    w, h = out_size
    mats = [np.eye(3), similarity(1.0, 0.0, 0.0, 1.0), similarity(-2.0, 1.0, 0.0, 1.0), similarity(0.5, -0.5, 0.3, 0.8, w / 2, h / 2),
            similarity(100.0, 0.0, 0.0, 1.0), similarity(0.0, 0.0, 0.0, 0.5, (w - 1) / 2, (h - 1) / 2)]
    for subpix in ("q5", "exact"):
        got = R.cover_extent(np.stack(mats), src_size, out_size, subpix=subpix)
        for m, g in zip(mats, got):
            mask = R.warp_mask(m, src_size, out_size, subpix=subpix)
            assert int(g) == R.extent_brute_force(mask, out_size) == R.extent_of_mask(mask, out_size)


def test_restatement_hand_cases():
    # identity on an equal canvas: everything covered
    assert R.cover_extent(np.eye(3)[None], (7, 5), (7, 5)).tolist() == [R.SENTINEL]
    # nothing covered: the minimum is the centre's e -- 0 on an odd x odd canvas, the smaller of (H-1), (W-1) on even x even
    far = similarity(1000.0, 0.0, 0.0, 1.0)[None]
    assert R.cover_extent(far, (7, 5), (7, 5)).tolist() == [0]
    assert R.cover_extent(far, (8, 6), (8, 6)).tolist() == [max(1 * 5, 1 * 7)]
    assert R.cover_extent(far, (8, 5), (8, 5)).tolist() == [max(1 * 4, 0)]
    # content moved 2 px to the right on 9 x 5: columns 0 and 1 are uncovered, column 1 is |2 - 8| * 4 = 24 from the centre;
    # in the centre row y = 2 that is the whole of e
    assert R.cover_extent(similarity(2.0, 0.0, 0.0, 1.0)[None], (9, 5), (9, 5)).tolist() == [24]
    # the measure itself: corners sit at E = (W-1) * (H-1)
    e = R.extent_measure((9, 5))
    assert e[0, 0] == e[4, 8] == e[0, 8] == 32 and e[2, 4] == 0 and e.dtype == np.int64


def test_restatement_mesh_zero_offsets_are_the_plain_warp():
    m = np.stack([similarity(3.0, -1.0, 0.05, 1.02, 10, 6), similarity(-2.5, 2.0, -0.03, 0.97, 10, 6)])
    plain = R.cover_extent(m, (21, 13), (20, 12))
    assert np.array_equal(plain, R.cover_extent(m, (21, 13), (20, 12), np.zeros((2, 4, 5, 2), np.float32)))
    moved = R.cover_extent(m, (21, 13), (20, 12), np.full((2, 4, 5, 2), 1.5, np.float32))
    assert not np.array_equal(plain, moved)


# ---- required_zoom --------------------------------------------------------------------------------------------------------
def test_required_zoom(dz):
    size = (161, 91)                        # E = 160 * 90 = 14400, m = 2 * 2 * 160 = 640
    assert dz.MARGIN_PX == 2
    ext = np.array([R.SENTINEL, 14400, 640, 100, 0, 641, 7840, 14400 + 640], np.uint32)
    z = dz.required_zoom(ext, size)
    assert z.dtype == np.float64
    assert z[0] == 1.0                                    # the sentinel: nothing uncovered
    assert z[1] == 14400.0 / (14400 - 640)                # uncovered pixels only at the very edge: the margin alone
    assert z[2] == z[3] == z[4] == 14400.0                # extent <= m: the divisor is clamped to 1
    assert z[5] == 14400.0                                # extent - m == 1
    assert z[6] == 2.0                                    # hand-computed: 14400 / (7840 - 640)
    assert z[7] == 1.0                                    # never below 1
    # the margin is two pixels of the LONGER side's unit
    assert dz.required_zoom([1000], (11, 101))[0] == 1000.0 / (1000 - 2 * 2 * 100)
    with pytest.raises(ValueError, match="1x5"):
        dz.required_zoom([3], (1, 5))


# ---- envelope -------------------------------------------------------------------------------------------------------------
def test_envelope_properties_on_random_input(dz):
    rng = np.random.default_rng(5)
    for n, r, limit in [(40, 3, 2.0), (17, 5, 1.4), (9, 12, 3.0), (1, 2, 2.0), (30, 1, 16.0)]:
        z_req = 1.0 + rng.random(n) ** 3 * 1.5
        z = dz.envelope(z_req, r, limit)
        assert z.dtype == np.float64 and z.shape == (n,)
        assert np.all(z >= np.minimum(z_req, limit)) and np.all(z <= limit)
        assert np.all(z <= max(z_req.max(), 1.0))
        # r = 0: the identity up to the cap
        assert np.array_equal(dz.envelope(z_req, 0, limit), np.minimum(z_req, limit))
        # a constant input gives a constant output
        const = dz.envelope(np.full(n, 1.37), r, limit)
        assert np.all(const == const[0]) and const[0] == min(1.37, limit)


def test_envelope_single_spike_is_a_ramp_of_width_4r_plus_1(dz):
    for r in (1, 3, 4):
        n = 8 * r + 9
        z_req = np.ones(n)
        mid = n // 2
        z_req[mid] = 1.8
        z = dz.envelope(z_req, r, 4.0)
        raised = np.nonzero(z > 1.0)[0]
        assert raised.tolist() == list(range(mid - 2 * r, mid + 2 * r + 1))          # width 4r + 1
        assert z.max() <= 1.8 and z[mid] == 1.8
        assert np.all(np.diff(z[mid - 2 * r - 1:mid + 1]) >= 0) and np.all(np.diff(z[mid:mid + 2 * r + 2]) <= 0)
        assert np.all(np.diff(z[mid - 2 * r - 1:mid - r + 1]) > 0)                   # a ramp, not a step
        # capped
        assert dz.envelope(z_req, r, 1.5).max() == 1.5


def test_envelope_segments_do_not_leak(dz):
    rng = np.random.default_rng(8)
    n, cut, r = 24, 12, 4
    a = 1.0 + rng.random(n) * 0.5
    b = a.copy()
    b[cut:] = 1.0 + rng.random(n - cut) * 1.2
    segs = [(0, cut), (cut, n)]
    za, zb = dz.envelope(a, r, 4.0, segs), dz.envelope(b, r, 4.0, segs)
    assert np.array_equal(za[:cut], zb[:cut]) and not np.array_equal(za[cut:], zb[cut:])
    # a shot is enveloped as a clip of its own
    assert np.array_equal(za[:cut], dz.envelope(a[:cut], r, 4.0)) and np.array_equal(zb[cut:], dz.envelope(b[cut:], r, 4.0))
    # without segments the change does reach the first shot
    assert not np.array_equal(dz.envelope(a, r, 4.0)[:cut], dz.envelope(b, r, 4.0)[:cut])
    assert dz.radius_frames(0.5, 16.0) == 4 and dz.radius_frames(2.0, 30.0) == 30 and dz.radius_frames(0.05, 16.0) == 0


# ---- zoom matrices --------------------------------------------------------------------------------------------------------
def test_zoom_matrices(dz):
    size = (160, 90)
    Z = dz.zoom_matrices([1.0, 1.25, 2.0], size)
    assert Z.dtype == np.float32 and Z.shape == (3, 3, 3)
    assert np.array_equal(Z[0].view(np.uint32), np.eye(3, dtype=np.float32).view(np.uint32))     # z = 1: the exact identity, no -0.0
    c = np.array([79.5, 44.5, 1.0])
    for m in Z.astype(np.float64):
        p = m @ c
        assert np.allclose(p / p[2], c, rtol=0, atol=1e-4)          # the centre pixel maps to itself (float32 entries: ~1e-5 px)
        assert m[1, 0] == m[0, 1] == m[2, 0] == m[2, 1] == 0.0 and m[2, 2] == 1.0 and m[0, 0] == m[1, 1]
    assert Z[2, 0, 0] == 2.0 and Z[2, 0, 2] == np.float32(-79.5) and Z[2, 1, 2] == np.float32(-44.5)


# ---- request checks -------------------------------------------------------------------------------------------------------
def test_request_validation(dz):
    assert dz.check_request(None) is None and dz.check_request(None, None) is None
    req = dz.check_request(True)
    assert (req.window_s, req.zoom_limit) == (2.0, 2.0) == (dz.DEFAULT_WINDOW_S, dz.DEFAULT_ZOOM_LIMIT)
    req = dz.check_request(0.5, 1)
    assert (req.window_s, req.zoom_limit) == (0.5, 1.0) and isinstance(req.zoom_limit, float)
    assert dz.check_request(60, 16.0).window_s == 60.0
    for bad in (False, 0, 0.0, -1.0, 60.5, float("nan"), float("inf"), "2", (1, 2), [2.0]):
        with pytest.raises(ValueError, match=re.escape(f"dynamic_zoom={bad!r}")):
            dz.check_request(bad)
    for bad in (0.99, 16.5, float("nan"), float("inf"), True, "2", -2):
        with pytest.raises(ValueError, match=re.escape(f"zoom_limit={bad!r}")):
            dz.check_request(True, bad)
    with pytest.raises(ValueError, match=re.escape("zoom_limit=1.5 needs dynamic_zoom")):
        dz.check_request(None, 1.5)
    dz.check_pipeline("crop_and_pad")
    with pytest.raises(ValueError, match="framing_mode 'crop': crop framing already has no padding"):
        dz.check_pipeline("crop")
    with pytest.raises(ValueError, match="framing_mode 'expand': an expand canvas has no frame to fill"):
        dz.check_pipeline("expand")


def test_pipelines_refuse_before_any_gpu_work(pkg):
    """crop, expand, a bad value and the sharded entry raise from the arguments alone: no GPU, no clip is touched."""
    from vstab_amd import distributed, flow_pipeline

    args = ("similarity", True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)
    for framing, why in (("crop", "already has no padding"), ("expand", "has no frame to fill")):
        with pytest.raises(ValueError, match=why):
            flow_pipeline._stabilize_frames(None, framing, *args, dynamic_zoom=True)
    with pytest.raises(ValueError, match=re.escape("dynamic_zoom=-3")):
        flow_pipeline._stabilize_frames(None, "crop_and_pad", *args, dynamic_zoom=-3)
    with pytest.raises(ValueError, match=re.escape("zoom_limit=1.5 needs dynamic_zoom")):
        flow_pipeline._stabilize_frames(None, "crop_and_pad", *args, zoom_limit=1.5)
    with pytest.raises(ValueError, match="dynamic zoom is not sharded"):
        distributed.stabilize_sharded(None, None, 24, "crop_and_pad", *args, dynamic_zoom=True)
    sig = inspect.signature(flow_pipeline._stabilize_frames).parameters
    for name in ("dynamic_zoom", "zoom_limit"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None
    assert inspect.signature(distributed.stabilize_sharded).parameters["dynamic_zoom"].default is None


def test_plan_zoom_meta_block(dz):
    size = (160, 90)
    ext = np.array([R.SENTINEL] * 5 + [12000, 6000, 12000] + [R.SENTINEL] * 4, np.uint32)
    Z, block = dz.plan_zoom(dz.check_request(0.5, 1.5), ext, size, 16.0)
    assert list(block) == ["version", "window_s", "radius_frames", "zoom_limit", "margin_px", "zoom_required", "zoom", "zoom_mean",
                           "zoom_max", "static_zoom", "frames_capped", "frames_with_padding"]
    z_req = dz.required_zoom(ext, size)
    assert block["version"] == 1 and block["radius_frames"] == 4 and block["margin_px"] == 2 and block["window_s"] == 0.5
    assert block["zoom_required"] == z_req.tolist() and block["static_zoom"] == z_req.max() > 1.5
    assert block["zoom"] == dz.envelope(z_req, 4, 1.5).tolist() and block["zoom_max"] == 1.5 and block["frames_capped"] == 1
    assert block["zoom_mean"] == float(np.mean(block["zoom"])) and block["frames_with_padding"] is None
    assert np.array_equal(Z, dz.zoom_matrices(block["zoom"], size))
    assert dz.finish_meta(block, [0, 3, 0, 9])["frames_with_padding"] == 2


# ---- the zero-padding claim, on the clips and parameters of the GPU pipeline tests ----------------------------------------
def _pipeline_clips():
    """Every camera path the GPU pipeline tests stabilize: the burst clip, and the two-shot clips of the scene-cut test (each
    shot locked onto its own first frame, as the per-shot plan does) with their segments."""
    cut = R.SCENE_CUT
    clips = {"burst": (R.locked_final_matrices(R.camera_path()), None)}
    for variant in (0, 1):
        shots = [R.locked_final_matrices(R.scene_shot1_path(cut)), R.locked_final_matrices(R.scene_shot2_path(R.CLIP_N - cut, variant))]
        clips[f"two_shots_{variant}"] = (np.concatenate(shots), [(0, cut), (cut, R.CLIP_N)])
    return clips


@pytest.mark.parametrize("mesh", [False, True], ids=["matrix", "mesh"])
@pytest.mark.parametrize("window_s,limit", [(0.5, 2.0), (0.05, 2.0), (0.5, 1.05), (0.5, 1.02), (2.0, 2.0)],
                         ids=["window", "r0", "capped", "capped_1.02", "default_window"])
@pytest.mark.parametrize("clip", ["burst", "two_shots_0", "two_shots_1"])
def test_zoomed_warp_leaves_no_padding_on_uncapped_frames(dz, clip, mesh, window_s, limit):
    """Restatement extents -> required_zoom -> envelope -> zoom_matrices -> the warp's own mask with the zoomed matrices: it
    sums to 0 on every frame whose zoom reaches what the frame needs.  Exact: zero, no allowance.
    The clips, windows and limits are those of the GPU pipeline tests; the matrices are a PROXY for theirs: the exact inverse
    of the synthetic camera path (frame i back onto its shot's first frame), not the estimator's fits with the crop_and_pad
    centre shift, which exist only on the GPU.  The claim does not depend on where the matrices come from -- it follows from
    the rule and the margin for any matrix warp -- and the GPU tests assert the same exact zeros on the pipeline's own
    matrices."""
    size = (R.CLIP_W, R.CLIP_H)
    final, segments = _pipeline_clips()[clip]
    offsets = R.smooth_offsets(R.CLIP_N, 17, 10) if mesh else None
    z_req = dz.required_zoom(R.cover_extent(final, size, size, offsets), size)
    z = dz.envelope(z_req, dz.radius_frames(window_s, 16.0), limit, segments)
    zoomed = np.matmul(dz.zoom_matrices(z, size), final)
    assert zoomed.dtype == np.float32
    padded = np.array([R.warp_mask(zoomed[i], size, size, None if offsets is None else offsets[i]).sum() for i in range(R.CLIP_N)])
    uncapped = z >= z_req
    assert z_req.max() > 1.1 and z_req.min() < 1.06                 # strong motion in an otherwise calm move
    assert np.all(padded[uncapped] == 0)
    if limit >= 2.0:
        assert uncapped.all() and z.mean() <= z_req.max()
        if window_s <= 0.5:                                          # (a window as long as the clip is nearly the static zoom)
            assert z.mean() < z_req.max()
    else:
        assert not uncapped.all() and padded[~uncapped].sum() > 0    # the cap binds: what is left shows


# ---- public surface -------------------------------------------------------------------------------------------------------
def test_node_is_listed_by_the_new_extension_only(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerFlowZoom
    assert len(nodes.NODE_CLASSES) == 6 and node not in nodes.NODE_CLASSES
    assert issubclass(nodes.VideoStabilizerAmdZoomExtension, nodes.VideoStabilizerAmdReportExtension)
    before = asyncio.run(nodes.VideoStabilizerAmdReportExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdZoomExtension().get_node_list())
    assert node not in before and listed == before + [node]
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_flow_zoom" and schema.display_name == "Video Stabilizer Flow (Dynamic Zoom)"
    flow = [s.id for s in nodes.VideoStabilizerFlow.define_schema().inputs]
    assert [s.id for s in schema.inputs] == [i for i in flow if i != "framing_mode"] + ["zoom_window", "zoom_limit"]
    by_id = {s.id: s for s in schema.inputs}
    assert by_id["zoom_window"].options["default"] == 2.0 and by_id["zoom_limit"].options["default"] == 2.0
    assert [s.id for s in schema.outputs] == [s.id for s in nodes.VideoStabilizerFlow.define_schema().outputs]
    assert list(inspect.signature(node.execute).parameters) == [s.id for s in schema.inputs]


def test_header_declares_what_native_binds_and_the_library_exports(pkg):
    from vstab_amd import native

    header = (ROOT / "include" / "vstab.h").read_text()
    assert re.search(r"#define\s+VSTAB_ZOOM_MARGIN_PX\s+2\b", header) and "#define VSTAB_ABI_VERSION 1\n" in header
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+vstab_cover_extent_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/vstab.h does not declare vstab_cover_extent_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = native._SIGNATURES["vstab_cover_extent_batch"]
    assert res is C.c_int and len(params) == len(args) == 12
    for ptxt, a in zip(params, args):
        assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
    assert "vstab_cover_extent_batch" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load_library(), "vstab_cover_extent_batch")
    assert list(inspect.signature(native.Context.cover_extent_batch).parameters)[1:] == ["matrices", "src_size", "out_size", "offsets", "subpix"]
    # the size checks come in front of any GPU work, under the function's name (the context is not touched before them)
    raw = C.CDLL(str(native.LIB_PATH))
    raw.vstab_last_error.restype = C.c_char_p
    fn = raw.vstab_cover_extent_batch
    fn.argtypes, fn.restype = args, C.c_int
    assert fn(None, None, 1, 4, 4, 4, 4, 0, None, 0, 0, None) != 0
    assert raw.vstab_last_error().decode().startswith("vstab_cover_extent_batch: ctx is NULL")
    fake_ctx, mats, out = C.create_string_buffer(8192), np.eye(3, dtype=np.float32).reshape(1, 9), np.zeros(1, np.uint32)
    for oh, ow, text in ((4, 1, "a 1x4 canvas has no centred extent"), (1, 4, "a 4x1 canvas has no centred extent"),
                         (46342, 46342, "does not fit the 32-bit extent"), (3, 2 ** 31 - 1, "does not fit the 32-bit extent")):
        assert fn(C.addressof(fake_ctx), mats.ctypes.data, 1, 4, 4, oh, ow, 0, None, 0, 0, out.ctypes.data) == 2
        assert text in raw.vstab_last_error().decode()
