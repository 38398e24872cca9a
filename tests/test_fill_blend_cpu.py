"""CPU: the blended temporal fill's host side (temporal_fill.gains_from_sums, the keyword checks, the new node's schema) and
the referees of what the GPU tests rely on (tests/fill_blend_restatement.py): the restatement at feather 0 / gains 1 is the
plain fill's, the feather weight under an integer translation is known in closed form, and on a clip whose frames differ by
known gains the blended restatement returns the frame's own exposure."""

import asyncio
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import fill_blend_restatement as B
from tests import temporal_fill_restatement as R

ROOT = Path(__file__).resolve().parents[1]


def _translation(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _small_case(seed=3, n=2, clip=4, sh=31, sw=45, dh=35, dw=50, K=3):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 1, (clip, sh, sw, 3)).astype(np.float32)
    dst = rng.uniform(0, 1, (n, dh, dw, 3)).astype(np.float32)
    mask = np.zeros((n, dh, dw), np.float32)
    mask[:, :7] = 1.0
    mask[:, :, -9:] = 1.0
    mask[:, 20, 20] = 0.5
    mats = np.stack([[_translation(rng.integers(-12, 13), rng.integers(-9, 10)) for _ in range(K)] for _ in range(n)])
    mats[0, 1, 0, 1] = 0.03                                            # one candidate with a shear
    mats[1, 0, 1] = mats[1, 0, 0] * 2                                   # one singular
    cand = rng.integers(0, clip, (n, K)).astype(np.int32)
    cand[0, 2] = -1
    own = np.stack([_translation(3, 2), _translation(-4, 5)])
    return src, dst, mask, mats, cand, own


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_restatement_without_feather_and_gains_is_the_plain_fill(oracle, interp):
    src, dst, mask, mats, cand, own = _small_case()
    want = R.temporal_fill(src, mats, cand, dst, mask, interp, "q5")
    got = B.temporal_fill_blend(src, mats, cand, own, np.ones(cand.shape + (3,), np.float32), 0, dst, mask, interp)
    assert want[3].sum() > 0
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(got[5], want[4])
    assert (got[4] == 0).all()


@pytest.mark.parametrize("interp,inset", [("bilinear", 0), ("bicubic", 1)])
def test_weight_along_a_row_under_an_integer_translation(interp, inset):
    """Own matrix = translation by (tx, ty): output pixel x has source x' = x - tx and X = 32 x'.  On the output row whose
    source row is the frame's middle and for x' <= 30 the left border is the nearest one, so d32 = 32 (x' - inset) and
    w = min(max(32 (x' - inset), 0), Fe) / Fe exactly."""
    sw, sh, tx, ty = 90, 70, 5, -3
    X, Y = B.q5_coordinates(_translation(tx, ty), (sw, sh))
    xs = np.arange(sw)
    assert np.array_equal(X[0], 32 * (xs - tx)) and np.array_equal(Y[:, 0], 32 * (np.arange(sh) - ty))
    d32 = B.feather_distance(X, Y, (sw, sh), interp)
    y = sh // 2 + ty                                                     # source row sh // 2: 34 px or more from top and bottom
    left = xs - tx <= 30
    for feather in (1, 7, 16, 64):
        fe = 32 * feather
        w = B.feather_weight(d32, feather)
        assert w.dtype == np.float32
        want = np.clip(32 * (xs - tx - inset), 0, fe).astype(np.float32) / np.float32(fe)
        assert np.array_equal(w[y][left], want[left]), feather
        assert (w[d32 >= fe] == 1.0).all() and (w[d32 <= 0] == 0.0).all()
        assert feather == 1 or ((w[y] > 0) & (w[y] < 1)).sum() >= min(feather, 30) - 1


def test_quantise_and_lattice():
    v = np.array([np.nan, -1.0, -0.0, 0.0, 1e-9, 0.5, 1.0 - 2.0 ** -24, 1.0, 3.0, np.inf, -np.inf, 0.2], np.float32)
    q = B.quantise(v)
    assert q.tolist() == [0, 0, 0, 0, 0, 32768, 65535, 65536, 65536, 65536, 0, int(np.float32(0.2) * np.float32(65536.0))]
    # a 3 x 3 canvas has no lattice pixel; a 5 x 13 one has two (x = 4, 12; y = 4)
    src = np.full((1, 9, 9, 3), 0.5, np.float32)
    eye = np.eye(3, dtype=np.float32)
    assert not B.gain_sums(src, eye[None, None], [[0]], eye[None], np.zeros((1, 3, 3, 3), np.float32)).any()


def test_gains_from_sums_on_hand_made_sums(pkg):
    from vstab_amd import temporal_fill as tf

    sums = np.zeros((1, 6, 7), np.int64)
    sums[0, 0] = [100, 3000, 4000, 5000, 6000, 4000, 2500]        # ratios 0.5, 1, 2
    sums[0, 1] = [100, 1000, 9000, 7, 4000, 3000, 8]              # clamped at each end: 0.25 -> 0.5, 3 -> 2; 7 / 8
    sums[0, 2] = [31, 3000, 3000, 3000, 1000, 1000, 1000]         # count 31: not enough overlap
    sums[0, 3] = [32, 3000, 3000, 3000, 1000, 0, 1500]            # count 32 counts; a candidate sum of zero gives 1
    sums[0, 4] = [0, 0, 0, 0, 0, 0, 0]
    sums[0, 5] = [1 << 20, 1 << 40, 3 << 39, 1 << 40, 1 << 40, 1 << 40, 3 << 39]
    g = tf.gains_from_sums(sums)
    assert g.dtype == np.float32 and g.shape == (1, 6, 3)
    want = np.array([[0.5, 1.0, 2.0], [0.5, 2.0, 0.875], [1, 1, 1], [2.0, 1.0, 2.0], [1, 1, 1], [1.0, 1.5, 2.0 / 3.0]], np.float64)
    assert np.array_equal(g[0], want.astype(np.float32))
    assert np.array_equal(g, B.gains_from_sums(sums))              # the restatement's own statement agrees
    assert np.array_equal(tf.gains_from_sums(sums.astype(np.uint64)), g)
    with pytest.raises(ValueError, match="gain sums"):
        tf.gains_from_sums(np.zeros((2, 7)))
    assert (tf.GAIN_MIN_COUNT, tf.GAIN_CLAMP, tf.MAX_FEATHER, tf.DEFAULT_FEATHER) == (32, (0.5, 2.0), 64, 16)


def test_keyword_validation(pkg):
    from vstab_amd import flow_pipeline
    from vstab_amd import temporal_fill as tf

    params = inspect.signature(flow_pipeline._stabilize_frames).parameters
    assert params["fill_feather"].kind is inspect.Parameter.KEYWORD_ONLY and params["fill_feather"].default is None
    assert params["fill_exposure"].kind is inspect.Parameter.KEYWORD_ONLY and params["fill_exposure"].default is False

    assert tf.check_blend_request(0) == (None, False) and tf.check_blend_request(4) == (None, False)
    assert tf.check_blend_request(4, True, False, "q5") == (16, False)
    assert tf.check_blend_request(4, 0, False, "q5") == (0, False) and tf.check_blend_request(4, 64, True, "q5") == (64, True)
    assert tf.check_blend_request(4, None, True, "q5") == (None, True)
    assert tf.check_blend_request(4, np.int64(7), np.bool_(True), "q5") == (7, True)
    for bad in (-1, 65, 8.0, "16", (8,)):
        with pytest.raises(ValueError, match=re.escape(f"fill_feather={bad!r}")):
            tf.check_blend_request(4, bad, False, "q5")
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match=re.escape(f"fill_exposure={bad!r}")):
            tf.check_blend_request(4, None, bad, "q5")
    with pytest.raises(ValueError, match="need temporal_fill > 0"):
        tf.check_blend_request(0, 8, False, "q5")
    with pytest.raises(ValueError, match="need temporal_fill > 0"):
        tf.check_blend_request(0, None, True, "q5")
    with pytest.raises(ValueError, match="sub-pixel mode 'exact'"):
        tf.check_blend_request(4, 8, False, "exact")

    # through the keyword, before any GPU work (the clip is never touched: the checks come first)
    class NoClip:
        frames = None

    def call(**kw):
        return flow_pipeline._stabilize_frames(NoClip(), "crop_and_pad", "similarity", False, 0.9, 0.8, 0.6, (127, 127, 127), 16.0, **kw)

    with pytest.raises(ValueError, match="need temporal_fill > 0"):
        call(fill_feather=8)
    with pytest.raises(ValueError, match="need temporal_fill > 0"):
        call(fill_exposure=True)
    with pytest.raises(ValueError, match=re.escape("fill_feather=99")):
        call(temporal_fill=4, fill_feather=99)
    with pytest.raises(ValueError, match=re.escape("fill_exposure='on'")):
        call(temporal_fill=4, fill_exposure="on")


def test_header_declares_what_native_binds(pkg):
    import ctypes as C

    from vstab_amd import native

    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "vstab.h").read_text(), flags=re.S)
    for name, count, method in (("vstab_fill_gain_sums", 17, "fill_gain_sums"),
                                ("vstab_temporal_fill_blend_batch", 23, "temporal_fill_blend_batch")):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, f"include/vstab.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = native._SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == count
        for ptxt, a in zip(params, args):
            assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), name) and hasattr(native.Context, method)
    assert re.search(r"#define\s+VSTAB_FILL_GAIN_STRIDE\s+8\b", text) and re.search(r"#define\s+VSTAB_FILL_FEATHER_MAX\s+64\b", text)
    assert re.search(r"#define\s+VSTAB_ABI_VERSION\s+1\b", text) or native.load_library().vstab_abi_version() == 1


def test_node_list_and_schema(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerTemporalFillBlend
    assert node not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    before = asyncio.run(nodes.VideoStabilizerAmdSubjectExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdFillBlendExtension().get_node_list())
    assert node not in before and listed == before + [node]
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension
    schema, base = node.define_schema(), nodes.VideoStabilizerTemporalFill.define_schema()
    assert schema.node_id == "video_stabilizer_temporal_fill_blend"
    assert schema.display_name == "Video Stabilizer Temporal Fill (Blended)"
    assert [s.id for s in base.inputs] == ["frames", "frames_stabilized", "padding_mask", "meta", "radius", "interpolation"]
    assert [s.id for s in schema.inputs] == [s.id for s in base.inputs] + ["feather", "match_exposure"]
    assert [s.id for s in schema.outputs] == ["frames", "padding_mask", "meta"]

    def opt(sock, key):   # the stand-in sockets keep their options in a dict, ComfyUI's as attributes
        return sock.options[key] if isinstance(getattr(sock, "options", None), dict) else getattr(sock, key)

    feather, exposure = schema.inputs[6], schema.inputs[7]
    assert (opt(feather, "default"), opt(feather, "min"), opt(feather, "max")) == (16, 0, 64)
    assert opt(exposure, "default") is True


def test_referee_flicker_clip(oracle):
    """Frames are 83 x 117 windows of one texture in [0.25, 0.75] at integer offsets within +-12 px; frame j is multiplied by
    a_j alternating 0.8 / 1.25.  With exposure matching, every pixel the blended restatement fills or blends is within 5e-4
    of a_i * texture; the hard fill is off by at least 0.45 * 0.25 on the filled pixels.

    The bound: every summed value is >= 0.2, so truncating it at 2^-16 loses a relative 2^-16 / 0.2 < 7.6e-5 of each sum;
    a gain is a ratio of two such sums: relative error < 1.6e-4; a pixel is at most 1.25 * 0.75 = 0.9375: < 1.5e-4 absolute,
    and float32 rounding of the multiply and the blend adds a few 1e-7.  5e-4 leaves a factor of three."""
    clip = B.flicker_clip()
    frames, truth, final, mats, cand = clip["frames"], clip["truth"], clip["final"], clip["matrices"], clip["cand_frame"]
    n, h, w = frames.shape[:3]
    dst, mask, _ = oracle.warp_clip(frames, final, (w, h), border=(0.5, 0.5, 0.5))
    assert (mask == 1.0).sum() > 2000

    sums = B.gain_sums(frames, mats, cand, final, dst)
    assert (sums[..., 0][cand >= 0] >= B.GAIN_MIN_COUNT).all(), "every pair must have enough overlap to get a gain"
    assert (sums[..., 0][cand < 0] == 0).all()
    gains = B.gains_from_sums(sums)
    a = clip["a"]
    for i in range(n):
        for k in range(2):
            if cand[i, k] >= 0:
                assert np.allclose(gains[i, k], a[i] / a[cand[i, k]], rtol=1.6e-4, atol=0)

    hard = R.temporal_fill(frames, mats, cand, dst, mask)
    worst = {}
    for feather in (0, 16):
        out = B.temporal_fill_blend(frames, mats, cand, final, gains, feather, dst, mask)
        touched = out[2] >= 0
        filled = (mask == 1.0) & touched
        assert np.array_equal(filled, hard[2] >= 0) and filled.sum() > 2000
        if feather:
            assert (touched & ~filled).sum() > 2000
        err = np.abs(out[0].astype(np.float64) - truth.astype(np.float64)).max(axis=-1)
        worst[feather] = float(err[touched].max())
        print(f"flicker clip, feather {feather}: worst error {worst[feather]:.3e} over {int(touched.sum())} pixels, "
              f"least overlap {int(sums[..., 0][cand >= 0].min())} lattice pixels")
        assert worst[feather] <= B.FLICKER_TOL
    off = np.abs(hard[0].astype(np.float64) - truth.astype(np.float64)).min(axis=-1)
    assert off[hard[2] >= 0].min() >= 0.45 * 0.25 - 1e-6
