"""CPU: the mask hand-off's rules as tests/mask_handoff_restatement.py states them -- the grow against ComfyUI GrowMask's own loop
(iterated scipy grey dilation / erosion), the feather against its iterated form and against scipy's chamfer distance
transform, the hold against a plain loop -- and the host side: mask_handoff.check_request, the pipelines' keywords, the meta
block, what the header and the bindings state, the new node's schema."""

import asyncio
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.ndimage

from tests import mask_handoff_restatement as R

ROOT = Path(__file__).resolve().parents[1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def grow_mask_loop(frame, expand, tapered):
    """ComfyUI's GrowMask, nodes_mask.py: abs(expand) iterations of the 3 x 3 grey dilation / erosion."""
    c = 0 if tapered else 1
    kernel = np.array([[c, 1, c], [1, 1, 1], [c, 1, c]])
    out = frame
    for _ in range(abs(expand)):
        out = (scipy.ndimage.grey_erosion if expand < 0 else scipy.ndimage.grey_dilation)(out, footprint=kernel)
    return out


# ---- grow --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tapered", [True, False])
@pytest.mark.parametrize("g", [1, 3, 7, 20, -1, -3, -7, -20])
def test_grow_is_growmask(g, tapered):
    """Float masks with fractions (no NaN, no -0.0: scipy has no rule for either), 23 x 31 and a frame smaller than the radius."""
    rng = np.random.default_rng(abs(g) * 2 + tapered)
    for shape in ((2, 23, 31), (1, 5, 3), (1, 1, 9)):
        m = rng.choice(np.array([0, 0, 0, 1, 0.25, 0.7, 0.5, 2.5, -3.0, np.inf, -np.inf], np.float32), size=shape)
        m = np.where(rng.random(shape) < 0.3, rng.random(shape, dtype=np.float32), m).astype(np.float32)
        want = np.stack([grow_mask_loop(f, g, tapered) for f in m])
        assert _same(R.grow(m, g, tapered), want)
        if abs(g) <= 7:
            assert _same(R.grow_by_offsets(m, g, tapered), want)


def test_grow_edge_rules():
    m = R.random_mask((2, 9, 11), 5)
    assert np.isnan(m).any()
    assert _same(R.grow(m, 0, True), m)                                   # g = 0: the bits, NaNs included
    one = np.where(np.isnan(m), np.float32(1), m)
    for g, tapered in ((2, True), (-2, False)):                          # a NaN reads as 1.0
        assert _same(R.grow(m, g, tapered), R.grow(one, g, tapered)) and not np.isnan(R.grow(m, g, tapered)).any()
    z = np.array([[[0.0, -0.0, -0.0]]], np.float32)                       # -0.0 orders below +0.0
    assert _bits(R.grow(z, 1, True)).tolist() == [[[0, 0, 0x80000000]]]
    assert _bits(R.grow(z, -1, True)).tolist() == [[[0x80000000, 0x80000000, 0x80000000]]]
    k = R.keys(R.VALUES)
    order = np.argsort(k, kind="stable")
    v = np.where(np.isnan(R.VALUES), np.float32(1), R.VALUES)[order]
    assert (np.diff(v) >= 0).all() and _same(R.unkeys(R.keys(v)), v)
    # nothing crosses from one frame into another
    m = np.zeros((3, 7, 9), np.float32)
    m[1] = 1.0
    for tapered in (True, False):
        out, counts = R.grow_feather(m, 3, tapered, 5)
        assert not out[0].any() and not out[2].any() and (out[1] == 1).all() and counts.tolist() == [0, 63, 0]


# ---- feather -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tapered", [True, False])
@pytest.mark.parametrize("f", [1, 16, 64])
def test_feather_forms_agree_and_ramp_is_chamfer_distance(f, tapered):
    rng = np.random.default_rng(f + tapered)
    shape = (2, 29, 37)
    sparse = R.random_mask(shape, 100 + f, sparse=True)
    sparse[0, 3, 4], sparse[0, 20, 30], sparse[1, 28, 0] = np.nan, 2.5, -3.0
    direct = R.feather(sparse, f, tapered)
    assert _same(direct, R.feather_iterated(sparse, f, tapered))
    if f <= 16:
        assert _same(direct, R.feather_by_offsets(sparse, f, tapered))
    assert direct[0, 3, 4] == 1.0 and direct[0, 20, 30] == 1.0            # the NaN reads as 1.0; 2.5 quantises to 65536
    binary = (rng.random(shape) < 0.01).astype(np.float32)
    binary[1] = 0
    binary[1, 0, 0] = 1
    out = R.feather(binary, f, tapered)
    step = 65536 // (f + 1)
    for k in range(shape[0]):
        d = scipy.ndimage.distance_transform_cdt(binary[k] == 0, metric="taxicab" if tapered else "chessboard").astype(np.int64)
        want = np.where(d <= f, 65536 - d * step, 0).astype(np.float32) / np.float32(65536)
        assert _same(out[k], want)
    assert _same(R.feather(sparse, 0, tapered), sparse)                   # f = 0: float for float


def test_q16_is_the_blended_fills_quantiser():
    v = np.array([-1.0, -0.0, 0.0, 1e-9, 0.5, 1.0 - 2.0 ** -24, 1.0, 3.0, np.inf, -np.inf, 0.2], np.float32)
    assert R.q16(v).tolist() == [0, 0, 0, 0, 32768, 65535, 65536, 65536, 65536, 0, int(np.float32(0.2) * np.float32(65536.0))]
    q = np.arange(0, 65537, 7, dtype=np.int32)                            # a level survives the trip through float
    assert np.array_equal(R.q16(q.astype(np.float32) / np.float32(65536)), q)


# ---- hold --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 12])
@pytest.mark.parametrize("T", [0, 1, 2, 16])
def test_hold_is_the_plain_loop(n, T):
    m = R.random_mask((n, 4, 5), 10 * n + T)
    for shot in (None, np.minimum(np.arange(n) // 3, 2)):
        got = R.hold(m, T, shot)
        if T == 0:
            assert _same(got, m)
            continue
        one = np.where(np.isnan(m), np.float32(1), m)
        want = np.empty_like(one)
        for i in range(n):
            for y in range(4):
                for x in range(5):
                    vals = [one[j, y, x] for j in range(n) if abs(j - i) <= T and (shot is None or shot[j] == shot[i])]
                    want[i, y, x] = max(vals)
        assert _same(got, want)
    assert R.shots_from_segments([(0, 2), (2, 3), (3, n + 3)], n + 3).tolist() == [0, 0, 1] + [2] * n


# ---- host side ---------------------------------------------------------------------------------------------------------------
def test_check_request(pkg):
    from vstab_amd import mask_handoff as mh

    assert (mh.HOLD_MAX, mh.GROW_MAX, mh.FEATHER_MAX) == (R.HOLD_MAX, R.GROW_MAX, R.FEATHER_MAX) == (16, 64, 64)
    assert mh.check_request() is None and mh.check_request(None, None, None, None) is None
    assert mh.check_request(5) == (0, 5, True, 0) == mh.Request(hold=0, grow=5, tapered=True, feather=0)
    assert mh.check_request(mask_feather=8) == (0, 0, True, 8) and mh.check_request(mask_hold=2) == (2, 0, True, 0)
    assert mh.check_request(0) == (0, 0, True, 0)                          # given: on, as a copy
    assert mh.check_request(np.int64(-64), np.int32(64), 16, False) == (16, -64, False, 64)
    for bad in (65, -65, 2.0, "5", True, (5,)):
        with pytest.raises(ValueError, match=re.escape(f"mask_grow={bad!r}")):
            mh.check_request(bad)
    for bad in (-1, 65, 1.5, False):
        with pytest.raises(ValueError, match=re.escape(f"mask_feather={bad!r}")):
            mh.check_request(5, bad)
    for bad in (-1, 17, 1.0, True):
        with pytest.raises(ValueError, match=re.escape(f"mask_hold={bad!r}")):
            mh.check_request(5, None, bad)
    for bad in (1, 0, "yes"):
        with pytest.raises(ValueError, match=re.escape(f"mask_tapered={bad!r}")):
            mh.check_request(5, None, None, bad)
    for lone in (True, False):
        with pytest.raises(ValueError, match="needs mask_grow, mask_feather or mask_hold"):
            mh.check_request(mask_tapered=lone)
    assert mh.shots_from_segments(None, 4) is None
    assert mh.shots_from_segments([(0, 3), (3, 4)], 4).tolist() == [0, 0, 0, 1]


def test_keywords_are_checked_before_any_gpu_work(pkg):
    from vstab_amd import apply_pipeline, distributed, flow_pipeline

    for fn in (flow_pipeline._stabilize_frames, apply_pipeline.apply_motion):
        params = inspect.signature(fn).parameters
        for name in ("mask_grow", "mask_feather", "mask_hold", "mask_tapered"):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None
    for fn in (distributed.stabilize_sharded, distributed.apply_motion_sharded):       # out of scope: not taken there
        assert "mask_grow" not in inspect.signature(fn).parameters

    class NoClip:                                                          # never touched: the checks come first
        frames = None

    def flow(**kw):
        return flow_pipeline._stabilize_frames(NoClip(), "crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0, **kw)

    def apply(**kw):
        return apply_pipeline.apply_motion(NoClip(), {"frames": 3}, (127, 127, 127), **kw)

    for call in (flow, apply):
        with pytest.raises(ValueError, match=re.escape("mask_grow=65")):
            call(mask_grow=65)
        with pytest.raises(ValueError, match=re.escape("mask_grow=True")):
            call(mask_grow=True)
        with pytest.raises(ValueError, match=re.escape("mask_grow=2.0")):
            call(mask_grow=2.0)
        with pytest.raises(ValueError, match=re.escape("mask_feather=-1")):
            call(mask_feather=-1)
        with pytest.raises(ValueError, match=re.escape("mask_feather=False")):
            call(mask_grow=1, mask_feather=False)
        with pytest.raises(ValueError, match=re.escape("mask_hold=17")):
            call(mask_hold=17)
        with pytest.raises(ValueError, match=re.escape("mask_hold=True")):
            call(mask_hold=True)
        with pytest.raises(ValueError, match=re.escape("mask_tapered=1")):
            call(mask_grow=5, mask_tapered=1)
        with pytest.raises(ValueError, match="needs mask_grow, mask_feather or mask_hold"):
            call(mask_tapered=False)


def test_meta_block_shape(pkg):
    import json

    from vstab_amd import mask_handoff as mh

    block = mh.meta_block(mh.Request(2, 5, True, 8), np.array([0, 6, 3], np.int32), (3, 4))
    assert list(block) == ["version", "hold", "grow", "tapered", "feather", "masked_fraction_mean", "masked_fraction_max"]
    assert block == {"version": 1, "hold": 2, "grow": 5, "tapered": True, "feather": 8,
                     "masked_fraction_mean": float(np.mean(np.array([0.0, 0.5, 0.25]))), "masked_fraction_max": 0.5}
    assert json.loads(json.dumps(block)) == block


def test_header_states_the_rules_and_native_binds_them(pkg):
    import ctypes as C

    from vstab_amd import native

    raw = (ROOT / "include" / "vstab.h").read_text()
    flat = re.sub(r"\s*\n \*\s*", " ", raw)
    for phrase in ("A NaN reads as 1.0f", "-0.0f below +0.0f", "held_i(p) = max of m_j(p) over |j - i| <= T, 0 <= j < n, and shot[j] == shot[i]",
                   "T = 0 returns the input's bits", "clipped to the frame", "g = 0 is the identity", "mode=\"reflect\"",
                   "Q(p) = max(0, max over q in the clipped ball of radius f of [ q16(G(q)) - dist(p, q) * step ])",
                   "step = 65536 / (f + 1) in integer division", "q16(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0",
                   "out = (float)Q / 65536", "count_out[k] = the number of pixels of out frame k that are > 0.5f",
                   "must not overlap mask", 'Timing kind "mask_hold"', 'timing kind "mask_grow"'):
        assert phrase in flat, phrase
    for define, value in (("VSTAB_GROW_TAPERED", 0), ("VSTAB_GROW_SQUARE", 1), ("VSTAB_MASK_HOLD_MAX", 16), ("VSTAB_MASK_GROW_MAX", 64),
                          ("VSTAB_MASK_FEATHER_MAX", 64)):
        assert re.search(r"#define %s %d\b" % (define, value), raw), define
    assert (native.GROW_TAPERED, native.GROW_SQUARE) == (0, 1)
    assert (native.MASK_HOLD_MAX, native.MASK_GROW_MAX, native.MASK_FEATHER_MAX) == (16, 64, 64)
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    for name, count, method in (("vstab_mask_hold_batch", 8, "mask_hold_batch"), ("vstab_mask_grow_batch", 10, "mask_grow_batch")):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, f"include/vstab.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = native._SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == count
        for ptxt, a in zip(params, args):
            assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), name) and hasattr(native.Context, method)
    assert list(inspect.signature(native.Context.mask_hold_batch).parameters)[1:] == ["mask", "hold", "shots"]
    assert list(inspect.signature(native.Context.mask_grow_batch).parameters)[1:6] == ["mask", "grow", "tapered", "feather", "want_count"]
    makefile = (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert "vstab_handoff.hip" in makefile


def test_entries_refuse_bad_arguments_before_any_gpu_work(pkg):
    """Through the C ABI with a context that is never dereferenced: every check sits in front of the first HIP call."""
    import ctypes as C

    from vstab_amd import native

    lib = native.load_library()
    lib.vstab_last_error.restype = C.c_char_p
    ctx, a, b = 0x1000, 0x10000, 0x80000                                   # never dereferenced: the calls are refused first

    def hold(*args):
        rc = lib.vstab_mask_hold_batch(*args)
        return rc, (lib.vstab_last_error() or b"").decode()

    def grow(*args):
        rc = lib.vstab_mask_grow_batch(*args)
        return rc, (lib.vstab_last_error() or b"").decode()

    for args, word in (((None, a, 1, 4, 4, 1, None, b), "NULL context"), ((ctx, None, 1, 4, 4, 1, None, b), "NULL pointer"),
                       ((ctx, a, 1, 4, 4, 1, None, None), "NULL pointer"), ((ctx, a, 0, 4, 4, 1, None, b), "bad shape"),
                       ((ctx, a, 1, 4, 4, 17, None, b), "hold=17"), ((ctx, a, 1, 4, 4, -1, None, b), "hold=-1"),
                       ((ctx, a + 2, 1, 4, 4, 1, None, b), "not aligned"), ((ctx, a, 2, 4, 4, 1, None, a + 64), "overlaps mask"),
                       ((ctx, a, 1, 65536, 65536, 1, None, b), "2^31")):
        rc, msg = hold(*args)
        assert rc == 2 and word in msg, (args, rc, msg)
    shot = (C.c_int32 * 3)(0, 1, 0)
    rc, msg = hold(ctx, a, 3, 4, 4, 1, C.addressof(shot), b)
    assert rc == 2 and "not non-decreasing" in msg
    for args, word in (((None, a, 1, 4, 4, 1, 0, 0, b, None), "NULL context"), ((ctx, None, 1, 4, 4, 1, 0, 0, b, None), "NULL pointer"),
                       ((ctx, a, 1, 4, 4, 1, 0, 0, None, None), "NULL pointer"), ((ctx, a, 1, 0, 4, 1, 0, 0, b, None), "bad shape"),
                       ((ctx, a, 1, 4, 4, 65, 0, 0, b, None), "grow=65"), ((ctx, a, 1, 4, 4, -65, 0, 0, b, None), "grow=-65"),
                       ((ctx, a, 1, 4, 4, 1, 2, 0, b, None), "footprint 2"), ((ctx, a, 1, 4, 4, 1, 0, 65, b, None), "feather=65"),
                       ((ctx, a, 1, 4, 4, 1, 0, -1, b, None), "feather=-1"), ((ctx, a, 1, 4, 4, 1, 0, 0, b, 0x90002), "not aligned"),
                       ((ctx, a, 1, 4, 4, 1, 0, 0, a, None), "overlaps mask"), ((ctx, a, 2, 4, 4, 1, 0, 0, a + 64, None), "overlaps mask")):
        rc, msg = grow(*args)
        assert rc == 2 and word in msg, (args, rc, msg)


def test_node_list_and_schema(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerMaskGrow
    assert node not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    before = asyncio.run(nodes.VideoStabilizerAmdSharpnessExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdHandoffExtension().get_node_list())
    assert node not in before and listed == before + [node]
    assert issubclass(nodes.VideoStabilizerAmdHandoffExtension, nodes.VideoStabilizerAmdSharpnessExtension)
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_mask_grow" and schema.display_name == "Video Stabilizer Mask Grow"
    ids = [s.id for s in schema.inputs]
    assert ids == ["mask", "expand", "tapered_corners", "feather", "hold"]
    assert ids == list(inspect.signature(node.execute).parameters)         # socket ids are the execute parameters
    assert [s.id for s in schema.outputs] == ["mask"]

    def opt(sock, key):   # the stand-in sockets keep their options in a dict, ComfyUI's as attributes
        return sock.options[key] if isinstance(getattr(sock, "options", None), dict) else getattr(sock, key)

    expand, tapered, feather, hold = schema.inputs[1:]
    assert (opt(expand, "default"), opt(expand, "min"), opt(expand, "max")) == (5, -64, 64)        # GrowMask's default
    assert opt(tapered, "default") is True
    assert (opt(feather, "default"), opt(feather, "min"), opt(feather, "max")) == (0, 0, 64)
    assert (opt(hold, "default"), opt(hold, "min"), opt(hold, "max")) == (0, 0, 16)
    with pytest.raises(ValueError, match=re.escape("mask_grow=99")):        # refused before any GPU work
        node.execute(None, 99, True, 0, 0)
    with pytest.raises(ValueError, match="socket 'mask'"):
        node.execute(None, 5, True, 0, 0)
    with pytest.raises(ValueError, match="floating-point MASK"):
        node.execute(np.zeros((2, 4, 4), np.uint8), 5, True, 0, 0)
    with pytest.raises(ValueError, match=r"not \[N,H,W\] or \[H,W\]"):
        node.execute(np.zeros((2, 4, 4, 1), np.float32), 5, True, 0, 0)


def test_documents_name_the_feature():
    for doc, words in (("README.md", ("mask_grow", "video_stabilizer_mask_grow", "GrowMask")),
                       ("INTEGRATION.md", ("vstab_mask_hold_batch", "vstab_mask_grow_batch", "VideoStabilizerAmdHandoffExtension")),
                       ("DESIGN.md", ("vstab_handoff.hip", "mask_relax_kernel"))):
        text = (ROOT / doc).read_text()
        for word in words:
            assert word in text, (doc, word)
