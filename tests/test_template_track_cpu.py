"""CPU: the template track's second header and its binding, the host arithmetic (template_track.py), every refusal, the node,
and the rule itself (tests/track_restatement.py) against a brute-force double loop and against the truth of an analytic clip.
No GPU: the kernel's parity with the restatement is tests/test_template_track_gpu.py.
"""

import asyncio
import ctypes
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import track_restatement as R
from tests.test_abi_cpu import _ctypes_class, _header_class

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "vstab_track.h"
SENT = int(R.SENTINEL)

# The largest error of the tracked centre against the truth on the analytic clip (key 0, R = 24), measured on the restatement:
# 0.1444 px (test_accuracy_on_the_analytic_clip prints it).  The bound is 1.5 times that: the margin is for the parabola's
# known bias at other sub-pixel phases.
CENTRE_MEASURED = 0.1444
CENTRE_BOUND = 1.5 * CENTRE_MEASURED


def track_prototypes():
    """(name, [parameter type strings], return type string) of every prototype of include/vstab_track.h."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"^[ \t]*((?:const\s+)?\w+(?:\s*\*)?)\s*\b(vstab_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S | re.M):
        out.append((m.group(2), [p.strip() for p in m.group(3).replace("\n", " ").split(",")], m.group(1)))
    return out


# ---- the three guards of the header -----------------------------------------------------------------------------------------
def test_signature_table_matches_the_header(pkg):
    from vstab_amd import native

    protos = {name: (params, ret) for name, params, ret in track_prototypes()}
    assert set(protos) == set(native._TRACK_SIGNATURES) == {"vstab_track_template_batch"}
    for name, (restype, argtypes) in native._TRACK_SIGNATURES.items():
        params, ret = protos[name]
        assert [_ctypes_class(a) for a in argtypes] == [_header_class(p) for p in params], name
        assert _ctypes_class(restype) == _header_class(ret) == "int", name
        assert params[0].startswith("vstab_ctx*")
    assert not set(native._TRACK_SIGNATURES) & set(native.EXPORTED_SYMBOLS)          # vstab.h's table is as it was
    assert '#include "vstab.h"' in HEADER.read_text()
    assert hasattr(native.load_library(), "vstab_track_template_batch")
    assert native.load_library().vstab_track_template_batch.argtypes == native._TRACK_SIGNATURES["vstab_track_template_batch"][1]
    assert native.track_work_words(48) == 512 + 2 * (97 * 97 + 2 * 97) and native.TRACK_SENTINEL == SENT
    text = HEADER.read_text()
    for macro, value in (("VSTAB_TRACK_RADIUS_MAX", native.TRACK_RADIUS_MAX), ("VSTAB_TRACK_MIN_BOX", native.TRACK_MIN_BOX),
                         ("VSTAB_TRACK_MAX_SAMPLES", native.TRACK_MAX_SAMPLES)):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    makefile = (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert "vstab_track.hip" in makefile and (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "vstab_track.hip").exists()


def test_null_arguments_are_refused_before_any_gpu_work(pkg):
    """A NULL context, then NULL pointers behind a context that is never dereferenced: a status and a message, no HIP call (this
    machine has no GPU)."""
    from vstab_amd import native

    lib = ctypes.CDLL(str(native.LIB_PATH))
    lib.vstab_last_error.restype = ctypes.c_char_p
    fn = lib.vstab_track_template_batch
    fn.restype, fn.argtypes = native._TRACK_SIGNATURES["vstab_track_template_batch"]
    zeros = [0] * 10
    assert fn(None, None, *zeros, None, None, None, None, None, None) != 0
    assert "NULL context" in lib.vstab_last_error().decode()
    fake = ctypes.create_string_buffer(4096)
    buf = ctypes.create_string_buffer(4096)
    ctx, p = ctypes.addressof(fake), ctypes.addressof(buf)
    good = [2, 16, 16, 2, 2, 8, 8, 1, 2, 0]
    for hole in (0, 1, 2, 3, 4, 6):  # gray, tsums, pos, best, near, work; surface (5) may be NULL
        ptrs = [p] * 7
        ptrs[hole] = None
        rc = fn(ctx, ptrs[0], *good, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6])
        assert rc != 0 and "NULL pointer" in lib.vstab_last_error().decode(), hole
    for bad, text in (([0, 16, 16, 2, 2, 8, 8, 1, 2, 0], "bad shape n=0"), ([2, 16, 16, 2, 2, 8, 8, 1, 2, 2], "key=2 outside"),
                      ([2, 16, 16, 2, 2, 8, 8, 1, 49, 0], "radius=49 outside 1..48"), ([2, 16, 16, 2, 2, 7, 8, 1, 2, 0], "the minimum is 8"),
                      ([2, 16, 16, 9, 2, 8, 8, 1, 2, 0], "leaves the 16 x 16 frame"), ([2, 16, 16, 2, 2, 8, 8, 2, 2, 0], "stride=2, the rule gives")):
        assert fn(ctx, p, *bad, p, p, p, p, None, p) != 0 and text in lib.vstab_last_error().decode(), text


def test_integration_doc_names_the_entry_point():
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name, _, _ in track_prototypes():
        assert name in doc
    assert "vstab_track.h" in doc


# ---- host arithmetic, by hand ----------------------------------------------------------------------------------------------
def test_subpixel_confidence_interpolation_and_meta(pkg):
    from vstab_amd import template_track as tt

    S = SENT
    near = np.array([[S, 40, S, 30, 10, 50, S, 20, S],        # x: (30 - 50) / (2 (30 - 20 + 50)) = -1/6;  y: (40 - 20) / (2 * 40) = 0.25
                     [0, 10, 0, 10, 10, 10, 0, 12, 0],        # x: denominator 0 -> 0;  y: (10 - 12) / (2 * 2) = -0.5
                     [0, S, 0, 1, 0, 100, 0, 5, 0],           # x: (1 - 100) / (2 * 101) clipped to -0.49..;  y: a sentinel neighbour -> 0
                     [0, 0, 0, 0, 9, 0, 0, 0, 0]], np.uint64)  # a maximum: denominators negative -> 0
    got = tt.subpixel(near)
    assert got.tolist() == [[-1.0 / 6.0, 0.25], [0.0, -0.5], [-99.0 / 202.0, 0.0], [0.0, 0.0]]
    near[2, 5] = 1000
    assert tt.subpixel(near)[2, 0] == -999.0 / 2002.0 and tt.subpixel(np.array([[0, 0, 0, 0, 0, 1000, 0, 0, 0]], np.uint64))[0, 0] == -0.5
    # J_T = 4 * 30 - 10 * 10 = 20
    assert tt.template_energy([4, 10, 30]) == 20
    conf = tt.confidence(np.array([0, 5, 20, 45, S], np.uint64), 20)
    assert conf.tolist() == [1.0, 0.5, 0.0, 0.0, 0.0]
    # six frames, key 1, box 10 x 8 at working = full resolution; frame 3 (confidence 0.2) and frame 5 (sentinel) are lost
    tsums = np.array([80, 800, 8020], np.int64)                       # J_T = 80 * 8020 - 640000 = 1600
    pos = np.array([[4, 6], [5, 5], [7, 5], [13, 5], [13, 9], [13, 9]], np.int32)
    best = np.array([400, 0, 100, 1024, 16, S], np.uint64)            # confidence 0.5, 1, 0.75, 0.2, 0.9, 0
    flat = np.array([[S, 0, S, 0, 0, 0, S, 0, S]] * 6, np.uint64)     # no sub-pixel offset anywhere
    size = (64, 48)
    table, block = tt.solve(tsums, pos, best, flat, (5, 5, 10, 8), 1, 6, (5, 5, 10, 8), size, size)
    assert block["confidence"] == [0.5, 1.0, 0.75, 0.19999999999999996, 0.9, 0.0] and block["lost"] == [3, 5]
    assert block["position"] == [[8.5, 9.5], [9.5, 8.5], [11.5, 8.5], [14.5, 10.5], [17.5, 12.5], [17.5, 12.5]]   # 3: midway; 5: held
    assert {k: block[k] for k in ("version", "box", "key", "radius", "stride", "samples")} == {
        "version": 1, "box": [5, 5, 10, 8], "key": 1, "radius": 6, "stride": 1, "samples": 80}
    assert block["frames_at_window_edge"] == 1                        # frame 3 picked dx = 13 - 7 = 6 = R
    assert json.loads(json.dumps(block)) == block and list(block) == ["version", "box", "key", "radius", "stride", "samples", "position",
                                                                       "confidence", "lost", "frames_at_window_edge"]
    assert table.shape == (5, 3) and table["matrix"][:, 0, 2].tolist() == [1.0, 2.0, 3.0, 3.0, 0.0]
    assert table["matrix"][:, 0, 5].tolist() == [-1.0, 0.0, 2.0, 2.0, 0.0]
    assert table["confidence"][:, 0].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0] and (table["accepted"][:, :2] == 1).all()
    # half resolution: the centre is scaled back to full-resolution pixels, the transitions stay in working pixels
    table2, block2 = tt.solve(tsums, pos, best, flat, (10, 10, 20, 16), 1, 6, (5, 5, 10, 8), (128, 96), size)
    assert block2["position"][0] == [17.0, 19.0] and table2["matrix"][0, 0, 2] == 1.0 and block2["box"] == [10, 10, 20, 16]
    with pytest.raises(ValueError, match="the box holds no texture"):
        tt.solve(np.array([80, 800, 8000]), pos, best, flat, (5, 5, 10, 8), 1, 6, (5, 5, 10, 8), size, size)
    assert tt.working_box((100, 50, 301, 33), (1920, 1080), (960, 540)) == (50, 25, 150, 16) and tt.stride_of(150, 16) == 3
    assert tt.stride_of(64, 64) == 1 and tt.stride_of(65, 9) == 2 and tt.stride_of(130, 70) == 3
    assert R.scale_box((100, 50, 301, 33), (1920, 1080), (960, 540)) == (50, 25, 150, 16) and R.stride_of(130, 70) == 3


# ---- refusals ---------------------------------------------------------------------------------------------------------------
class NoClip:
    frames = None


class Clip:
    def __init__(self, n, w, h):
        self.frames, self.width, self.height = [None] * n, w, h


BOX = (10, 10, 40, 40)
M = np.zeros((4, 4), np.float32)
REFUSALS = [
    (dict(), "estimator='track' needs track_box: (x, y, width, height) around the subject in frame track_key, in full-resolution pixels."),
    (dict(track_box=(1, 2, 3)), "track_box=(1, 2, 3) is not (x, y, width, height), four integers in full-resolution pixels"),
    (dict(track_box=(1, 2, 30.0, 30)), "track_box=(1, 2, 30.0, 30) is not (x, y, width, height), four integers in full-resolution pixels"),
    (dict(track_box=(1, True, 30, 30)), "track_box=(1, True, 30, 30) is not (x, y, width, height), four integers in full-resolution pixels"),
    (dict(track_box="1234"), "track_box='1234' is not (x, y, width, height), four integers in full-resolution pixels"),
    (dict(track_box=(-1, 2, 30, 30)), "track_box=(-1, 2, 30, 30): x and y must be >= 0, width and height >= 1"),
    (dict(track_box=(1, 2, 0, 30)), "track_box=(1, 2, 0, 30): x and y must be >= 0, width and height >= 1"),
    (dict(track_box=BOX, track_key=-1), "track_key=-1 is not a frame index (an integer >= 0)"),
    (dict(track_box=BOX, track_key=True), "track_key=True is not a frame index (an integer >= 0)"),
    (dict(track_box=BOX, track_key=1.0), "track_key=1.0 is not a frame index (an integer >= 0)"),
    (dict(track_box=BOX, track_radius=0), "track_radius=0 is not None or an integer in 1..48 (working pixels)"),
    (dict(track_box=BOX, track_radius=49), "track_radius=49 is not None or an integer in 1..48 (working pixels)"),
    (dict(track_box=BOX, track_radius=True), "track_radius=True is not None or an integer in 1..48 (working pixels)"),
    (dict(track_box=BOX, track_radius=8.0), "track_radius=8.0 is not None or an integer in 1..48 (working pixels)"),
    (dict(track_box=BOX, subject_mask=np.zeros((2, 4, 4), np.float32)), "subject_mask needs estimator='subject', got estimator='track'"),
    (dict(track_box=BOX, scene_cuts="auto"), "scene_cuts is not supported with estimator 'track'"),
    (dict(track_box=BOX, scene_cuts=[3]), "scene_cuts is not supported with estimator 'track'"),
    (dict(track_box=BOX, estimation_mask=M), "estimation_mask is not supported with estimator 'track'"),
    (dict(track_box=BOX, mesh_warp=True), "mesh_warp is not supported with estimator 'track'"),
    (dict(track_box=BOX, temporal_fill=2), "temporal_fill is not supported with estimator 'track'"),
    (dict(track_box=BOX, sharpness_transfer=2), "sharpness_transfer is not supported with estimator 'track'"),
    (dict(track_box=BOX, rolling_shutter=0.5), "rolling_shutter is not supported with estimator 'track'"),
    (dict(track_box=BOX, drift_correction=True), "drift_correction is not supported with estimator 'track'"),
    (dict(track_box=BOX, deflicker=True), "deflicker is not supported with estimator 'track'"),
    (dict(track_box=BOX, horizon_level=True), "horizon_level is not supported with estimator 'track'"),
    (dict(track_box=BOX, plate_fill=True), "plate_fill is not supported with estimator 'track'"),
    (dict(track_box=BOX, mesh_warp=(1, 1)), "mesh_warp=(1, 1): cols and rows must lie in [2, 64]"),     # a malformed value keeps its message
]


def _call(clip, mode="translation", estimator="track", **kw):
    from vstab_amd import flow_pipeline as fp

    return fp._stabilize_frames(clip, "crop_and_pad", mode, True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0, estimator=estimator, **kw)


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals(pkg, case):
    keywords, message = REFUSALS[case]
    with pytest.raises(ValueError) as caught:
        _call(NoClip(), **keywords)
    assert str(caught.value).startswith(message), str(caught.value)


def test_refusals_that_read_the_mode_the_estimator_or_the_clip(pkg):
    from vstab_amd import distributed
    from vstab_amd import flow_pipeline as fp

    for mode in ("similarity", "perspective"):
        with pytest.raises(ValueError, match=f"transform_mode='{mode}' is not supported with estimator 'track': the template is searched at one scale"):
            _call(NoClip(), mode=mode, track_box=BOX)
    for kw, text in ((dict(track_box=BOX), r"track_box=\(10, 10, 40, 40\) needs estimator='track', got estimator='flow'"),
                     (dict(track_key=2), "track_key=2 needs estimator='track', got estimator='classic'"),
                     (dict(track_key=False), "track_key=False needs estimator='track'"),
                     (dict(track_radius=24), "track_radius=24 needs estimator='track'")):
        with pytest.raises(ValueError, match=text):
            _call(NoClip(), mode="similarity", estimator="classic" if "classic" in text else "flow", **kw)
    # against the clip, before any context is asked for: the key frame, the box inside the frame, its size in working pixels
    with pytest.raises(ValueError, match="track_key=5 outside a clip of 5 frames"):
        _call(Clip(5, 1920, 1080), track_box=BOX, track_key=5)
    with pytest.raises(ValueError, match=r"track_box=\(1900, 10, 40, 40\) leaves the 1920 x 1080 frame"):
        _call(Clip(5, 1920, 1080), track_box=(1900, 10, 40, 40))
    with pytest.raises(ValueError, match=r"its height of 15 px is 7 working pixels \(estimation images of 960 x 540\), the minimum is 8"):
        _call(Clip(5, 1920, 1080), track_box=(10, 10, 40, 15))
    with pytest.raises(ValueError, match=r"its width of 7 px is 7 working pixels \(estimation images of 240 x 135\)"):
        _call(Clip(5, 240, 135), track_box=(10, 10, 7, 15))
    with pytest.raises(ValueError, match="stabilize_sharded does not support estimator 'track': the template track is not sharded"):
        distributed.stabilize_sharded(None, None, 12, "crop_and_pad", "translation", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0,
                                      estimator="track")
    # the request: the new field sits in front of `refit` (which a test of the refit pins as the last one), with a default
    params = inspect.signature(fp._stabilize_frames).parameters
    for name, default in (("track_box", None), ("track_key", 0), ("track_radius", None)):
        assert params[name].default == default and params[name].kind is inspect.Parameter.KEYWORD_ONLY
    kw = {name: prm.default for name, prm in params.items() if prm.kind is inspect.Parameter.KEYWORD_ONLY}
    assert fp.check_flow_request("crop_and_pad", "similarity", "flow", kw).track is None
    got = fp.check_flow_request("crop_and_pad", "translation", "track", dict(kw, estimator="track", track_box=BOX, track_radius=None))
    assert got.track == (BOX, 0, 24) and got.estimator == "track" and got.needs_host_plan is False and got.kept_by_products == ()
    assert fp._META_SOURCE["track"] == "estimated_subject" and fp._backend_fields("track") == {"flow_backend": "template_track", "flow_fallback_reason": None}
    assert fp._ESTIMATORS["track"] is fp.estimate_transitions_track
    assert not fp.device_plan_applies("track", "crop_and_pad", "translation", 12)


def test_bypasses_ignore_the_keywords(pkg):
    """0 or 1 frame: the clip-dependent checks are not made (a key frame of 7 in a clip of one frame is not looked at)."""
    clip = Clip(0, 64, 48)
    out = _call(clip, track_box=BOX, track_key=7)
    assert out.meta["frames"] == 0 and out.meta["flow_backend"] == "template_track"


# ---- the node ---------------------------------------------------------------------------------------------------------------
def test_node_schema_and_hand_over(pkg, monkeypatch):
    import vstab_amd
    from vstab_amd import nodes, nodes_track

    cls = nodes_track.VideoStabilizerFlowTrack
    s = cls.define_schema()
    assert s.node_id == "video_stabilizer_flow_track" and issubclass(cls, nodes._FlowVariant) and cls.ESTIMATOR == "track"
    assert [i.id for i in s.inputs] == ["frames", "frame_rate", "framing_mode", "camera_lock", "strength", "smooth", "keep_fov",
                                        "padding_color", "box_x", "box_y", "box_width", "box_height", "key_frame", "search_radius"]
    assert [o.id for o in s.outputs] == ["frames_stabilized", "padding_mask", "meta"]
    radius = [i for i in s.inputs if i.id == "search_radius"][0]
    assert (radius.options["default"], radius.options["min"], radius.options["max"]) == (24, 1, 48)
    seen = {}

    def fake(estimator, *nine, **extras):
        seen.update(estimator=estimator, nine=nine, extras=extras)
        return "out"

    monkeypatch.setattr(nodes, "_run_estimator_node", fake)
    assert cls.execute("F", 16.0, "crop_and_pad", True, 1.0, 0.5, 0.6, "#7F7F7F", 3, 4, 50, 60, key_frame=2, search_radius=9) == "out"
    assert seen["estimator"] == "track" and seen["nine"] == ("F", 16.0, "crop_and_pad", "translation", True, 1.0, 0.5, 0.6, "#7F7F7F")
    assert seen["extras"] == dict(track_box=(3, 4, 50, 60), track_key=2, track_radius=9)
    cls.execute("F", 16.0, "crop_and_pad", True, 1.0, 0.5, 0.6, "#7F7F7F", 3, 4, 50, 60)
    assert seen["extras"] == dict(track_box=(3, 4, 50, 60), track_key=0, track_radius=24)
    # registration: an extension of its own behind the chain's last one; nodes.py's namespace, NODE_CLASSES and the entry point as they were
    ext = nodes_track.VideoStabilizerAmdTrackExtension
    last = getattr(nodes, nodes._EXTENSION_CHAIN[-1][0])
    assert issubclass(ext, last) and asyncio.run(ext().get_node_list()) == asyncio.run(last().get_node_list()) + [cls]
    assert not hasattr(nodes, "VideoStabilizerFlowTrack") and cls not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def _brute(gray, box, s, R_, key):
    """The rule as two plain loops over candidates and samples, Python integers."""
    n, h, w = gray.shape
    bx, by, bw, bh = box
    nx, ny = bw // s, bh // s
    T = [[int(gray[key][by + j * s][bx + i * s]) for i in range(nx)] for j in range(ny)]
    pos, best, surf = {key: (bx, by)}, {key: 0}, {}
    for k in list(range(key + 1, n)) + list(range(key - 1, -1, -1)):
        px, py = pos[k - 1] if k > key else pos[k + 1]
        cands = []
        for dy in range(-R_, R_ + 1):
            for dx in range(-R_, R_ + 1):
                qx, qy = px + dx, py + dy
                if qx < 0 or qy < 0 or qx + (nx - 1) * s > w - 1 or qy + (ny - 1) * s > h - 1:
                    J = SENT
                else:
                    d = [int(gray[k][qy + j * s][qx + i * s]) - T[j][i] for j in range(ny) for i in range(nx)]
                    J = nx * ny * sum(v * v for v in d) - sum(d) ** 2
                surf[k, dy, dx] = J
                cands.append((J, dx * dx + dy * dy, dy, dx))
        J, _, dy, dx = min(cands)
        pos[k], best[k] = (px + dx, py + dy), J
    return pos, best, surf


@pytest.mark.parametrize("key", [0, 1, 2])
def test_restatement_equals_the_double_loop(key):
    rng = np.random.default_rng(7 + key)
    base = rng.integers(0, 256, (40, 44))
    gray = np.stack([base[8 + dy:28 + dy, 10 + dx:34 + dx] for dx, dy in ((0, 0), (2, -1), (-1, 3))]).astype(np.uint8)   # [3,20,24]
    gray[1] = np.clip(gray[1].astype(int) + 17, 0, 255).astype(np.uint8)
    for box, R_ in (((6, 5, 9, 8), 4), ((0, 0, 18, 10), 3), ((2, 1, 22, 19), 2)):
        s = R.stride_of(box[2], box[3])
        got = R.track(gray, box, s, R_, key)
        pos, best, surf = _brute(gray, box, s, R_, key)
        assert got["pos"].tolist() == [list(pos[k]) for k in range(3)] and got["best"].tolist() == [best[k] for k in range(3)]
        for k in range(3):
            if k == key:
                assert got["surface"][k, R_, R_] == 0 and (got["surface"][k] == R.SENTINEL).sum() == (2 * R_ + 1) ** 2 - 1
                continue
            want = np.array([[surf[k, dy, dx] for dx in range(-R_, R_ + 1)] for dy in range(-R_, R_ + 1)], np.uint64)
            assert np.array_equal(got["surface"][k], want)
            dx, dy = (int(v) for v in got["pos"][k] - got["pos"][k - 1 if k > key else k + 1])
            assert got["near"][k].tolist() == [surf.get((k, dy + ey, dx + ex), SENT) for ey in (-1, 0, 1) for ex in (-1, 0, 1)]
        T = R.template(gray[key], box, s)
        assert got["tsums"].tolist() == [T.size, int(T.sum()), int((T * T).sum())]


def test_brightness_offset_and_flat_regions():
    """J is unchanged by a brightness offset (as far as nothing clips), and a flat region stays where it was."""
    rng = np.random.default_rng(3)
    gray = rng.integers(40, 200, (2, 20, 24)).astype(np.uint8)
    gray[1] = gray[0]
    a = R.track(gray, (6, 5, 9, 8), 1, 3, 0)
    gray[1] += 31
    b = R.track(gray, (6, 5, 9, 8), 1, 3, 0)
    assert np.array_equal(a["surface"], b["surface"]) and b["best"][1] == 0 and b["pos"][1].tolist() == [6, 5]
    flat = np.full((3, 20, 24), 50, np.uint8)
    flat[0, 5:13, 6:15] = rng.integers(0, 256, (8, 9))
    c = R.track(flat, (6, 5, 9, 8), 1, 4, 0)
    assert c["pos"].tolist() == [[6, 5]] * 3 and len(set(c["surface"][1][c["surface"][1] != R.SENTINEL].tolist())) == 1


def test_accuracy_on_the_analytic_clip(pkg):
    """The largest error of the tracked centre against the truth: 0.1444 px (measured here, on the restatement; key 0, R = 24,
    a 40 x 32 box on a 12-frame 240 x 135 clip whose patch moves by sub-pixel steps of up to 9 px per axis over a background
    that moves differently).  Asserted: 1.5 times that."""
    from vstab_amd import template_track as tt

    gray, corners = R.analytic_clip()
    assert gray.shape == (12, 135, 240) and np.abs(np.diff(corners, axis=0)).max() == 9.0
    size = (R.CLIP_W, R.CLIP_H)
    box = R.analytic_box(0)
    out = R.track(gray, box, R.stride_of(box[2], box[3]), 24, 0)
    table, block = tt.solve(out["tsums"], out["pos"], out["best"], out["near"], box, 0, 24, box, size, size)
    err = np.abs(np.array(block["position"]) - R.analytic_truth(0)).max()
    print("largest error of the tracked centre, px:", err, "smallest confidence:", min(block["confidence"]))
    assert block["lost"] == [] and min(block["confidence"]) > tt.LOST and block["frames_at_window_edge"] == 0
    assert err <= CENTRE_BOUND
    whole = np.abs(np.array(block["position"]) - np.rint(np.array(block["position"]) - 0.5) - 0.5)
    assert (whole > 1e-9).any()                                        # the parabola moved the centres off the pixel grid
    steps = np.diff(R.analytic_truth(0), axis=0)
    assert np.abs(table["matrix"][:, 0, [2, 5]] - steps).max() <= 2 * CENTRE_BOUND
