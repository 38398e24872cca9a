"""Horizon level without a GPU: the restatement of the device rule against brute force, the host side (horizon_level.py), the
checks of a request, the bindings and the node."""

import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import horizon_level_restatement as R

ROOT = Path(__file__).resolve().parents[1]
K = R.K


@pytest.fixture(scope="module")
def hl(pkg):
    from vstab_amd import horizon_level

    return horizon_level


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def _brute(gray, min_mag2):
    """The rule of include/vstab.h word for word, one pixel at a time in Python integers."""
    n, h, w = gray.shape
    hist = [[0] * (2 * K + 1) for _ in range(n)]
    for f in range(n):
        g = [[int(v) for v in row] for row in gray[f]]
        for y in range(1, h - 1):
            for x in range(1, w - 1):
                gx = 3 * (g[y - 1][x + 1] - g[y - 1][x - 1]) + 10 * (g[y][x + 1] - g[y][x - 1]) + 3 * (g[y + 1][x + 1] - g[y + 1][x - 1])
                gy = 3 * (g[y + 1][x - 1] - g[y - 1][x - 1]) + 10 * (g[y + 1][x] - g[y - 1][x]) + 3 * (g[y + 1][x + 1] - g[y - 1][x + 1])
                m2 = gx * gx + gy * gy
                if m2 < min_mag2 or m2 == 0:
                    continue
                a, b = abs(gx), abs(gy)
                j = (2 * K * min(a, b) + max(a, b)) // (2 * max(a, b))
                sign = (gx * gy > 0) - (gx * gy < 0)
                hist[f][sign * (1 if a >= b else -1) * j + K] += m2
    return np.asarray(hist, dtype=np.int64)


def test_restatement_equals_brute_force():
    rng = np.random.default_rng(0)
    for h, w in ((3, 3), (4, 7), (9, 5), (12, 12)):
        gray = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        gray[1] = (gray[1] // 64) * 64          # flat patches: zero gradients among the pixels
        for min_mag2 in (0, 65536, 1 << 27):
            assert np.array_equal(R.orientation_hist(gray, min_mag2), _brute(gray, min_mag2)), (h, w, min_mag2)
    for shape in ((2, 2, 9), (2, 9, 2), (1, 1, 1)):
        assert not R.orientation_hist(np.full(shape, 200, np.uint8), 0).any()
    assert R.orientation_hist(rng.integers(0, 256, (2, 6, 6), dtype=np.uint8), 0).shape == (2, 2 * K + 1)


def test_ties_and_axis_aligned_gradients_land_where_the_rule_says():
    y, x = np.mgrid[0:12, 0:12]
    diag = (200 * (((x + y) % 8) < 4)).astype(np.uint8)            # gx == gy
    anti = (200 * (((x - y) % 8) < 4)).astype(np.uint8)            # gx == -gy
    vert = (200 * (x >= 6)).astype(np.uint8)                       # gy == 0
    horz = (200 * (y >= 6)).astype(np.uint8)                       # gx == 0
    hist = R.orientation_hist(np.stack([diag, anti, vert, horz]), 0)
    assert hist[0].sum() == hist[0][2 * K] > 0                     # a == b, gx * gy > 0: bin +K
    assert hist[1].sum() == hist[1][0] > 0                         # a == b, gx * gy < 0: bin -K
    assert hist[2].sum() == hist[2][K] > 0 and hist[3].sum() == hist[3][K] > 0
    assert hist[2][K] == 2 * 10 * (16 * 200) ** 2                  # two columns of ten interior pixels, |gx| = 16 * 200


# ---- frame_roll ----------------------------------------------------------------------------------------------------------------
def _peak(hl, deg, mass=1000):
    hist = np.zeros(2 * K + 1, np.int64)
    hist[int(np.argmin(np.abs(hl.bin_angles() - deg)))] = mass
    return hist


def test_frame_roll_finds_a_peak_and_is_periodic(hl):
    assert hl.frame_roll(np.zeros(2 * K + 1, np.int64)) == (None, 0.0)
    for deg in (-30.0, -0.1, 0.0, 12.3, 44.0):
        roll, conf = hl.frame_roll(_peak(hl, deg))
        assert abs(roll - deg) < 0.12 and conf == 1.0              # (bins are up to 0.22 degrees apart)
    hi, _ = hl.frame_roll(_peak(hl, 44.9))
    lo, _ = hl.frame_roll(_peak(hl, -44.9))
    assert abs(hi - 44.9) < 0.12 and abs(lo + 44.9) < 0.12
    assert abs(abs(float(hl.wrap90(hi - lo))) - 0.2) < 0.15          # 0.2 degrees apart across the seam, not 89.8
    # mass on both sides of the seam is one peak: bins -K and +K are the same orientation
    both = _peak(hl, 44.9) + _peak(hl, -44.9)
    both[0] += 500
    both[2 * K] += 500
    roll, conf = hl.frame_roll(both)
    assert abs(abs(roll) - 45.0) < 0.1 and conf == 1.0
    # the confidence is the share of the mass within a degree
    roll, conf = hl.frame_roll(_peak(hl, 10.0, 300) + _peak(hl, -20.0, 100))
    assert abs(roll - 10.0) < 0.12 and conf == 0.75
    with pytest.raises(ValueError, match="a histogram of 12 bins"):
        hl.frame_roll(np.zeros(12))


def test_frame_roll_accuracy_on_the_analytic_frames(hl):
    """The worst single-frame error at the 12 known rolls, measured: 0.0965 degrees (confidence 0.75-0.83); asserted: 1.5 x."""
    scene = R.Scene()
    frames = np.stack([scene.render(roll) for roll in R.ACCURACY_ROLLS])
    rolls, conf = hl.frame_rolls(R.orientation_hist(frames, hl.MIN_MAG2))
    err = hl.wrap90(rolls - np.asarray(R.ACCURACY_ROLLS))
    print(f"\nframe_roll: errors {np.round(err, 4).tolist()} worst {np.abs(err).max():.4f}; confidence {np.round(conf, 3).tolist()}")
    assert np.abs(err).max() <= 1.5 * R.MEASURED_WORST_DEG
    assert conf.min() >= 2 * hl.MIN_CONFIDENCE
    # sinusoids alone stay far below the threshold
    noise = R.Scene(sinus=0.03, structure=False, freq=(0.1, 0.6))
    _, conf = hl.frame_rolls(R.orientation_hist(np.stack([noise.render(r) for r in (0.0, 7.0, 31.0)]), hl.MIN_MAG2))
    assert 0.0 < conf.max() <= 0.05


# ---- chain, offsets, matrices ------------------------------------------------------------------------------------------------
def _rot(deg, tx=0.0, ty=0.0, cx=0.0, cy=0.0):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1.0]])


def test_chain_roll(hl):
    steps = [2.0, -3.0, 0.5, 1.0, 4.0]
    T = np.stack([_rot(d, tx=3.0 * i, cx=240, cy=135) for i, d in enumerate(steps)])
    assert np.allclose(hl.chain_roll(T), [0, 2, -1, -0.5, 0.5, 4.5], atol=1e-12)
    assert np.allclose(hl.chain_roll(T, [(0, 3), (3, 6)]), [0, 2, -1, 0, 1, 5], atol=1e-12)          # restarts in every shot
    assert np.allclose(hl.chain_roll(T, None, [1, 0, 1, 1, 0.5]), [0, 2, 2, 2.5, 3.5, 7.5], atol=1e-12)   # confidence 0: identity
    translations = np.tile(np.eye(3), (4, 1, 1))
    translations[:, 0, 2] = 5.0
    assert not hl.chain_roll(translations).any()
    assert hl.chain_roll(np.zeros((0, 3, 3))).tolist() == [0.0]


def test_offsets(hl):
    n = 20
    rng = np.random.default_rng(1)
    r = np.cumsum(rng.uniform(-1, 1, n))
    r -= r[0]
    roll = hl.wrap90(7.0 + r + rng.uniform(-0.05, 0.05, n))
    conf = np.full(n, 0.6)
    conf[[3, 4, 11]] = 0.1                       # unmeasured frames, with a roll that would spoil a mean
    roll[[3, 4, 11]] = -40.0
    roll[5] = np.nan                             # an empty histogram
    one = hl.Request(None, 20.0)
    beta, measured, lost = hl.offsets(roll, conf, r, one, 16.0)
    assert lost == 0 and measured.sum() == n - 4 and not measured[[3, 4, 5, 11]].any()
    assert len(set(beta.tolist())) == 1 and abs(beta[0] - 7.0) < 0.05
    # near the seam: e = +-45 is one value
    seam = hl.wrap90(44.9 + r + rng.uniform(-0.2, 0.2, n))
    beta, _, _ = hl.offsets(seam, np.full(n, 0.6), r, one, 16.0)
    assert abs(float(hl.wrap90(beta[0] - 44.9))) < 0.2
    # two shots, the second one not observable (2 of 8 frames measured: fewer than max(3, 10 %))
    roll2 = np.concatenate([hl.wrap90(6.0 + r[:12]), hl.wrap90(-4.0 + r[12:] - r[12])])
    r2 = np.concatenate([r[:12], r[12:] - r[12]])
    conf2 = np.full(n, 0.6)
    conf2[14:] = 0.0
    beta, measured, lost = hl.offsets(roll2, conf2, r2, one, 16.0, [(0, 12), (12, 20)])
    assert lost == 1 and np.allclose(beta[:12], 6.0, atol=1e-9) and np.isnan(beta[12:]).all() and measured.sum() == 14
    conf2[14:] = 0.6
    beta, _, lost = hl.offsets(roll2, conf2, r2, one, 16.0, [(0, 12), (12, 20)])
    assert lost == 0 and np.allclose(beta[:12], 6.0, atol=1e-9) and np.allclose(beta[12:], -4.0, atol=1e-9)
    # a window: a camera that tips over by 0.5 degrees per frame is followed, a single outlier is not
    tip = 0.5 * np.arange(n)
    roll3 = hl.wrap90(3.0 + tip)
    roll3[10] += 8.0
    conf3 = np.full(n, 0.6)
    conf3[6] = 0.0
    beta, _, _ = hl.offsets(roll3, conf3, np.zeros(n), hl.Request(0.25, 20.0), 16.0)      # radius_frames(0.25, 16) = 2
    # (an outlier moves a median of five by at most one rank, 0.5 degrees here; the clamped ends lag by up to a frame's tip more)
    assert np.abs(beta[2:-2] - (3.0 + tip[2:-2])).max() <= 0.5 and abs(beta[10] - 8.0) <= 0.5
    assert np.all(np.diff(beta) >= 0)
    # too few frames for any shot
    assert hl.offsets(roll[:2], conf[:2], r[:2], one, 16.0)[2] == 1


def test_level_matrices_clamp_and_count(hl):
    size = (480, 270)
    cx, cy = 239.5, 134.5
    r = np.array([0.0, 1.0, -2.0, 0.5])
    F = np.stack([_rot(-d, tx=2.0, cx=cx, cy=cy) for d in r]).astype(np.float32)      # camera lock: the chain undone
    L, a, limited = hl.level_matrices(np.full(4, 7.0), r, F, size, 20.0)
    assert limited == 0 and np.allclose(a, -7.0, atol=1e-5) and L.dtype == np.float32 and L.shape == (4, 3, 3)
    centre = np.array([cx, cy, 1.0])
    assert np.allclose(L.astype(np.float64) @ centre, centre, atol=1e-4)                  # about the canvas centre
    assert np.allclose(np.degrees(np.arctan2(L[:, 1, 0], L[:, 0, 0])), -7.0, atol=1e-4)
    L, a, limited = hl.level_matrices(np.array([7.0, 2.0, -7.0, np.nan]), r, F, size, 3.0)
    assert limited == 2 and np.allclose(a, [-3.0, -2.0, 3.0, 0.0], atol=1e-5)
    assert np.array_equal(L[3], np.eye(3, dtype=np.float32))                             # no offset: no correction
    # modulo 90: an offset of 80 degrees reads as -10
    _, a, _ = hl.level_matrices(np.full(4, 80.0), r, F, size, 20.0)
    assert np.allclose(a, 10.0, atol=1e-5)


def test_plan_level_levels_a_known_camera(hl):
    """Known rolls, exact transitions, a camera-locked plan: L @ F shows every frame upright."""
    n = 12
    rng = np.random.default_rng(4)
    theta = 7.0 + np.concatenate([[0.0], rng.uniform(-2, 2, n - 1)])
    shift = np.concatenate([[[0.0, 0.0]], rng.uniform(-3, 3, (n - 1, 2))])
    cx, cy = 239.5, 134.5
    pose = np.stack([_rot(t, tx=s[0], ty=s[1], cx=cx, cy=cy) for t, s in zip(theta, shift)])       # scene -> frame i
    T = np.stack([pose[i + 1] @ np.linalg.inv(pose[i]) for i in range(n - 1)])                   # frame i -> frame i + 1
    F = np.stack([pose[0] @ np.linalg.inv(pose[i]) for i in range(n)]).astype(np.float32)         # frame i -> frame 0
    hist = np.stack([_peak(hl, t) for t in theta])
    L, block = hl.plan_level(hl.Request(None, 20.0), hist, T, np.ones(n - 1), F, (480, 270), 16.0)
    assert json.loads(json.dumps(block)) == block
    assert list(block) == ["version", "window_s", "limit_deg", "min_confidence", "roll_deg", "confidence", "frames_measured",
                           "shots_not_observable", "offset_deg", "correction_deg", "correction_deg_max", "frames_limited"]
    out = np.matmul(L.astype(np.float64), F.astype(np.float64)) @ pose                           # scene -> output
    assert np.abs(np.degrees(np.arctan2(out[:, 1, 0], out[:, 0, 0]))).max() < 0.12                # (the peaks sit on bin centres)
    assert block["frames_measured"] == n and block["frames_limited"] == 0 and abs(block["offset_deg"][0] - 7.0) < 0.12
    # nothing measurable: no matrices at all, so that the plan stays as it is
    L, block = hl.plan_level(hl.Request(None, 20.0), np.zeros_like(hist), T, np.ones(n - 1), F, (480, 270), 16.0)
    assert L is None and block["shots_not_observable"] == 1 and block["roll_deg"] == [None] * n and block["offset_deg"] == [None] * n
    assert block["correction_deg"] == [0.0] * n and block["correction_deg_max"] == 0.0 and block["frames_measured"] == 0


# ---- the checks of a request -------------------------------------------------------------------------------------------------
def test_check_request(hl):
    assert hl.check_request(None) is None and hl.check_request(None, None) is None
    assert hl.check_request(True) == hl.Request(None, 20.0)
    assert hl.check_request(2.5, 44.5) == hl.Request(2.5, 44.5) and hl.check_request(60, 1) == hl.Request(60.0, 1.0)
    for bad in (False, 0, 0.0, -1.0, 60.5, float("nan"), float("inf"), "auto", (1, 2)):
        with pytest.raises(ValueError, match=re.escape(f"horizon_level={bad!r}: expected None, True or a finite window in seconds in (0, 60]")):
            hl.check_request(bad)
    for bad in (True, False, 0, 45, 45.0, -3.0, 90, float("nan"), float("inf"), "3"):
        with pytest.raises(ValueError, match=re.escape(f"horizon_limit={bad!r}: expected None or a finite number of degrees in (0, 45)")):
            hl.check_request(True, bad)
    with pytest.raises(ValueError, match=re.escape("horizon_limit=3 needs horizon_level: without a levelling there is no correction to limit.")):
        hl.check_request(None, 3)


class NoClip:                      # never touched: the checks come first
    frames = None


def _call(pkg, framing="crop_and_pad", mode="similarity", **kw):
    from vstab_amd import flow_pipeline as fp

    return fp._stabilize_frames(NoClip(), framing, mode, True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0, **kw)


REFUSED = [
    (dict(framing="crop"), "horizon_level is not supported with framing_mode 'crop': the crop solver has already bounded the matrices"),
    (dict(framing="expand"), "horizon_level is not supported with framing_mode 'expand': an expand canvas is fixed by the plan's matrices"),
    (dict(mode="perspective"), "horizon_level is not supported with transform_mode 'perspective': a homography has no single roll."),
    (dict(estimator="subject", subject_mask=np.zeros((2, 4, 4), np.float32)),
     "horizon_level is not supported with estimator 'subject': the subject lock never makes the estimation images"),
    (dict(rolling_shutter=0.5), "horizon_level is not supported with rolling_shutter=0.5: the two have not been tried together."),
    (dict(rolling_shutter="auto"), "horizon_level is not supported with rolling_shutter='auto':"),
]


@pytest.mark.parametrize("keywords,start", REFUSED, ids=[str(sorted(k)) + str(i) for i, (k, _) in enumerate(REFUSED)])
def test_stabilize_frames_refuses_before_any_gpu_work(pkg, keywords, start):
    with pytest.raises(ValueError) as caught:
        _call(pkg, horizon_level=True, **keywords)
    assert str(caught.value).startswith(start), str(caught.value)


def test_malformed_keywords_raise_before_any_gpu_work(pkg):
    for kw, start in ((dict(horizon_level=-2), "horizon_level=-2: expected None, True"),
                      (dict(horizon_level=True, horizon_limit=True), "horizon_limit=True: expected None or a finite number"),
                      (dict(horizon_limit=5.0), "horizon_limit=5.0 needs horizon_level"),
                      # the new checks stand behind the existing ones
                      (dict(horizon_level=-2, dynamic_zoom=99.0), "dynamic_zoom=99.0: expected None, True"),
                      (dict(horizon_level=-2, deflicker="x"), "deflicker='x'")):
        with pytest.raises(ValueError) as caught:
            _call(pkg, **kw)
        assert str(caught.value).startswith(start), str(caught.value)


def test_request_fields_and_by_products(pkg):
    from vstab_amd import flow_pipeline as fp

    sig = inspect.signature(fp._stabilize_frames).parameters
    for name in ("horizon_level", "horizon_limit"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    kw = {k: p.default for k, p in sig.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    off = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw))
    assert off.level is None and not off.needs_host_plan and off.kept_by_products == ()
    on = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, horizon_level=1.5, horizon_limit=10))
    assert (on.level.window_s, on.level.limit_deg) == (1.5, 10.0) and on.needs_host_plan and on.kept_by_products == ("gray_out",)
    both = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, horizon_level=True, mesh_warp=True))
    assert both.kept_by_products == ("gray_out", "grid_out")
    # a dictionary without the new names is a request without the feature
    for name in ("horizon_level", "horizon_limit"):
        kw.pop(name)
    assert fp.check_flow_request("crop_and_pad", "similarity", "flow", kw).level is None


def test_bypasses_ignore_the_keyword(pkg):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    one = np.zeros((1, 8, 8, 3), np.float32)
    a = fp._stabilize_frames(hm._normalize_video_input(one), "crop_and_pad", "similarity", True, 1.0, 0.5, 0.6, (0, 0, 0), 16.0)
    b = fp._stabilize_frames(hm._normalize_video_input(one), "crop_and_pad", "similarity", True, 1.0, 0.5, 0.6, (0, 0, 0), 16.0,
                             horizon_level=True, horizon_limit=5)
    assert json.dumps(a.meta) == json.dumps(b.meta) and "horizon_level" not in b.meta


def test_stabilize_sharded_refuses_the_keywords(pkg):
    from vstab_amd import distributed

    call = (None, None, 12, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
    with pytest.raises(ValueError, match="stabilize_sharded does not support horizon_level=True: the horizon level is not sharded"):
        distributed.stabilize_sharded(*call, horizon_level=True)
    with pytest.raises(ValueError, match="stabilize_sharded does not support horizon_limit=5: the horizon level it belongs to"):
        distributed.stabilize_sharded(*call, horizon_limit=5)
    with pytest.raises(ValueError, match="stabilize_sharded does not support scene_cuts:"):      # behind the existing refusals
        distributed.stabilize_sharded(*call, horizon_level=True, scene_cuts="auto")
    params = inspect.signature(distributed.stabilize_sharded).parameters
    assert params["horizon_level"].default is None and params["horizon_limit"].default is None


# ---- bindings, header, documents, node ---------------------------------------------------------------------------------------
def test_header_bindings_and_documents_agree(pkg):
    import ctypes

    from vstab_amd import native

    text = (ROOT / "include" / "vstab.h").read_text()
    m = re.search(r"\bint\s+vstab_orientation_hist_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/vstab.h does not declare vstab_orientation_hist_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["vstab_ctx* ctx", "const uint8_t* gray", "int n", "int h", "int w", "uint32_t min_mag2", "uint64_t* hist"]
    res, args = native._SIGNATURES["vstab_orientation_hist_batch"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_uint32, ctypes.c_void_p]
    assert "vstab_orientation_hist_batch" in native.EXPORTED_SYMBOLS and hasattr(native.Context, "orientation_hist_batch")
    assert f"#define VSTAB_ORIENTATION_K {native.ORIENTATION_K}" in text and native.ORIENTATION_K == K
    assert "#define VSTAB_ABI_VERSION 1" in text
    lib = native.load_library()
    fn = lib.vstab_orientation_hist_batch
    assert fn(None, None, 0, 0, 0, 0, None) != 0
    lib.vstab_last_error.restype = ctypes.c_char_p
    assert lib.vstab_last_error().decode().startswith("vstab_orientation_hist_batch: NULL context")
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = (ROOT / doc).read_text()
        assert "vstab_orientation_hist_batch" in body and "horizon_level" in body, doc
    from vstab_amd import horizon_level as hl

    assert hl.K == K and hl.MIN_MAG2 == 65536 and hl.MIN_CONFIDENCE == 0.25


def test_level_node(pkg):
    import asyncio

    from vstab_amd import nodes
    import vstab_amd

    s = nodes.VideoStabilizerFlowLevel.define_schema()
    assert s.node_id == "video_stabilizer_flow_level" and s.display_name == "Video Stabilizer Flow (Horizon Level)"
    base = [i.id for i in nodes.VideoStabilizerFlow.define_schema().inputs]
    assert [i.id for i in s.inputs] == [i for i in base if i != "framing_mode"] + ["level_window", "level_limit"]
    by_id = {i.id: i for i in s.inputs}
    assert list(by_id["transform_mode"].options["options"]) == ["translation", "similarity"]
    assert by_id["level_window"].options["default"] == 0.0 and by_id["level_limit"].options["default"] == 20.0
    assert by_id["level_limit"].options["max"] < 45.0
    assert [o.id for o in s.outputs] == [o.id for o in nodes.VideoStabilizerFlow.define_schema().outputs]
    assert nodes.VideoStabilizerFlowLevel not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    listed = asyncio.run(nodes.VideoStabilizerAmdLevelExtension().get_node_list())
    before = asyncio.run(nodes.VideoStabilizerAmdDeflickerExtension().get_node_list())
    assert listed == before + [nodes.VideoStabilizerFlowLevel]
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension      # unchanged
    # what the node hands on: 0 is one offset per shot
    seen = {}

    def fake(estimator, *args, **extras):
        seen.update(extras, estimator=estimator, framing=args[2])
        return "out"

    real = nodes._run_estimator_node
    nodes._run_estimator_node = fake
    try:
        assert nodes.VideoStabilizerFlowLevel.execute(None, 16.0, "similarity", True, 1.0, 0.5, 0.6, "127,127,127", 0.0, 12.0) == "out"
        assert seen == dict(horizon_level=True, horizon_limit=12.0, estimator="flow", framing="crop_and_pad")
        nodes.VideoStabilizerFlowLevel.execute(None, 16.0, "similarity", True, 1.0, 0.5, 0.6, "127,127,127", 2.5, 12.0)
        assert seen["horizon_level"] == 2.5
    finally:
        nodes._run_estimator_node = real
