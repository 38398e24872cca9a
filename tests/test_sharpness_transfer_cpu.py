"""CPU: the sharpness transfer's host side (sharpness_transfer.ratios_from_energy, the keyword checks, the meta block, the new
node's schema), what the header and the bindings state, and the referee of what the GPU tests rely on
(tests/sharpness_restatement.py): on a clip with known motion whose every fourth frame is blurred, the restated rule brings
the blurred frames back towards their sharp render and returns the others bit for bit."""

import asyncio
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sharpness_restatement as S

ROOT = Path(__file__).resolve().parents[1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement's own properties ------------------------------------------------------------------------------------
def test_flat_frame_has_no_energy_and_thin_frames_have_none():
    flat = np.full((2, 9, 13, 3), 0.37, np.float32)
    assert S.frame_sharpness(flat) == [0, 0]
    rng = np.random.default_rng(1)
    assert S.frame_sharpness(rng.uniform(0, 1, (1, 1, 7, 3)).astype(np.float32)) == [0]      # no pixel has both differences
    assert S.frame_sharpness(rng.uniform(0, 1, (1, 7, 1, 3)).astype(np.float32)) == [0]
    assert S.frame_sharpness(rng.uniform(0, 1, (1, 1, 1, 3)).astype(np.float32)) == [0]


def test_quantise_and_nan_counts_as_zero():
    v = np.array([np.nan, -1.0, -0.0, 0.0, 1e-9, 0.5, 1.0 - 2.0 ** -24, 1.0, 3.0, np.inf, -np.inf, 0.2], np.float32)
    assert S.quantise(v).tolist() == [0, 0, 0, 0, 0, 32768, 65535, 65536, 65536, 65536, 0, int(np.float32(0.2) * np.float32(65536.0))]
    a = np.zeros((1, 2, 2, 3), np.float32)
    b = a.copy()
    a[0, 0, 0] = np.nan                                   # a NaN pixel is a black pixel
    assert S.frame_sharpness(a) == S.frame_sharpness(b) == [0]
    a[0, 0, 1] = 1.0                                      # and a white one next to it gives the full step
    b[0, 0, 1] = 1.0
    assert S.frame_sharpness(a) == S.frame_sharpness(b) == [65536 ** 2]


def test_two_by_two_hand_case():
    """Y = [[16384, 49152], [32768, x]]: the one pixel with both differences is (0, 0): gx = 32768, gy = 16384."""
    f = np.zeros((1, 2, 2, 3), np.float32)
    f[0, 0, 0] = 0.25
    f[0, 0, 1] = 0.75
    f[0, 1, 0] = 0.5
    f[0, 1, 1] = (0.1, 0.9, 0.3)                          # takes no part
    assert S.luma(f[0])[:, 0].tolist() == [16384, 32768] and S.luma(f[0])[0, 1] == 49152
    assert S.frame_sharpness(f) == [32768 ** 2 + 16384 ** 2]
    # the channel weights: (q(r) + 2 q(g) + q(b)) >> 2, truncating
    g = np.zeros((1, 1, 1, 3), np.float32)
    g[0, 0, 0] = (1.0, 0.5, 2.0 ** -16)
    assert S.luma(g[0])[0, 0] == (65536 + 2 * 32768 + 1) >> 2
    # the largest step a pixel can contribute: 2 * 65536^2 = 2^33
    h = np.zeros((1, 2, 2, 3), np.float32)
    h[0, 0, 0] = 5.0
    assert S.frame_sharpness(h) == [2 ** 33]


def test_transfer_restatement_by_hand(oracle):
    """Identity matrices on a 4 x 4 clip: the sample is the candidate's pixel (interior: x, y < 3).  One candidate, ratio 2,
    alpha 4, own 0.25 and sample 0.5 in every channel: D = 0.75, w = 2 / (2 + 3) = 0.4, dst = (0.25 + 0.4 * 0.5) / 1.4."""
    src = np.stack([np.full((4, 4, 3), 0.25, np.float32), np.full((4, 4, 3), 0.5, np.float32)])
    eye = np.eye(3, dtype=np.float32)[None, None]
    dst = src[:1].copy()
    out, count = S.sharp_transfer(src, eye, [[1]], [[2.0]], 4.0, dst)
    w = np.float32(2.0) / (np.float32(2.0) + np.float32(4.0) * np.float32(0.75))
    want = (np.float32(0.25) + w * np.float32(0.5)) / (np.float32(1.0) + w)
    assert count.tolist() == [9] and (out[0, :3, :3] == want).all()
    assert np.array_equal(_bits(out[0, 3]), _bits(dst[0, 3])) and np.array_equal(_bits(out[0, :, 3]), _bits(dst[0, :, 3]))
    # ratio 0, a -1 slot and a padded pixel leave every bit; alpha = 0 is the plain mean of own and sample
    assert np.array_equal(_bits(S.sharp_transfer(src, eye, [[1]], [[0.0]], 4.0, dst)[0]), _bits(dst))
    assert np.array_equal(_bits(S.sharp_transfer(src, eye, [[-1]], [[2.0]], 4.0, dst)[0]), _bits(dst))
    mask = np.zeros((1, 4, 4), np.float32)
    mask[0, 1, 1] = 1.0
    mask[0, 2, 2] = 0.999                                 # not exactly 1: own
    out, count = S.sharp_transfer(src, eye, [[1]], [[2.0]], 0.0, dst, mask)
    assert count.tolist() == [8] and out[0, 1, 1, 0] == np.float32(0.25) and (out[0, 2, 2] == np.float32(0.375)).all()
    # a NaN in the own pixel leaves it; a NaN in the sample is skipped -- and the sample of each of the four pixels whose
    # bilinear taps touch (1, 1) is NaN (weight 0 times NaN), so 9 - 4 pixels are transferred ((0, 0) is one of the four)
    dst2 = dst.copy()
    dst2[0, 0, 0, 1] = np.nan
    src2 = src.copy()
    src2[1, 1, 1, 2] = np.nan
    out, count = S.sharp_transfer(src2, eye, [[1]], [[2.0]], 0.0, dst2)
    assert count.tolist() == [5] and np.array_equal(_bits(out[0, 0, 0]), _bits(dst2[0, 0, 0]))
    assert (out[0, 1, 1] == np.float32(0.25)).all() and (out[0, 0, 1] == np.float32(0.25)).all() and (out[0, 2, 2] == np.float32(0.375)).all()


# ---- host side ----------------------------------------------------------------------------------------------------------
def test_ratios_from_energy_edge_cases(pkg):
    from vstab_amd import sharpness_transfer as st

    assert (st.MIN_RATIO, st.DEFAULT_ALPHA, st.MAX_RADIUS, st.MAX_ALPHA) == (1.1, 16.0, 16, 1024.0)
    energy = np.array([10, 11, 0, 100, 1 << 62], np.int64)
    cand = np.array([[1, 2, -1, 3], [0, 3, 2, 1], [0, 1, 3, 4], [0, 1, 2, 4], [3, 3, 3, 3]], np.int32)
    r = st.ratios_from_energy(energy, cand)
    assert r.dtype == np.float32 and r.shape == cand.shape
    want = np.zeros(cand.shape, np.float64)
    want[0, 0] = 11 / 10                                   # the quotient exactly 1.1 is kept (11 / 10 is the float64 1.1)
    want[0, 3] = 10.0
    want[1, 1] = 100 / 11                                  # 10 / 11 and 11 / 11 are below 1.1
    want[3, 3] = float(1 << 62) / 100.0                    # E_i = 0 (row 2) borrows nothing; nothing borrows from -1
    assert np.array_equal(r, want.astype(np.float32)) and 11 / 10 == 1.1
    assert np.array_equal(r, S.ratios_from_energy([int(e) for e in energy], cand))      # the restatement's own statement agrees
    assert np.array_equal(st.ratios_from_energy(energy.astype(np.uint64), cand), r)
    assert np.array_equal(st.ratios_from_energy(energy, cand[2:4], first=2), r[2:4])
    with pytest.raises(ValueError, match="does not fit"):
        st.ratios_from_energy(energy[:3], cand)
    # the sharpness the meta lists: energy / (2^32 (w - 1)(h - 1))
    assert st.sharpness_from_energy([2 ** 33], (2, 2)).tolist() == [2.0] and st.sharpness_from_energy([5], (1, 9)).tolist() == [0.0]


def test_check_request_and_pipeline(pkg):
    from vstab_amd import distributed, flow_pipeline
    from vstab_amd import sharpness_transfer as st

    params = inspect.signature(flow_pipeline._stabilize_frames).parameters
    for name in ("sharpness_transfer", "sharpness_alpha"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None

    for off in (0, None, False, np.int64(0)):
        assert st.check_request(off) is None and st.check_request(off, None, "exact") is None
    assert st.check_request(1, None, "q5") == (1, 16.0) and st.check_request(16, 0, "q5") == (16, 0.0)
    assert st.check_request(np.int32(2), np.float32(4.0), "q5") == (2, 4.0) and st.check_request(2, 1024, "q5") == (2, 1024.0)
    for bad in (-1, 17, 2.0, "2", True, (2,)):
        with pytest.raises(ValueError, match=re.escape(f"sharpness_transfer={bad!r}")):
            st.check_request(bad, None, "q5")
    for bad in (-0.5, 1024.5, float("nan"), float("inf"), "16", True):
        with pytest.raises(ValueError, match=re.escape(f"sharpness_alpha={bad!r}")):
            st.check_request(2, bad, "q5")
    for off in (0, None, False):
        with pytest.raises(ValueError, match="needs sharpness_transfer > 0"):
            st.check_request(off, 8.0, "q5")
    with pytest.raises(ValueError, match="sub-pixel mode 'exact'"):
        st.check_request(2, None, "exact")
    st.check_pipeline("flow"), st.check_pipeline("classic"), st.check_pipeline("flow_tvl1"), st.check_pipeline("flow_phase_correlate")
    with pytest.raises(ValueError, match="mesh_warp: transfer candidates are global matrices"):
        st.check_pipeline("flow", mesh_warp=object())
    with pytest.raises(ValueError, match="estimator 'subject': its transitions are the subject's"):
        st.check_pipeline("subject")

    # through the keywords, before any GPU work (the clip is never touched: the checks come first)
    class NoClip:
        frames = None

    def call(**kw):
        return flow_pipeline._stabilize_frames(NoClip(), "crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0, **kw)

    with pytest.raises(ValueError, match=re.escape("sharpness_transfer=99")):
        call(sharpness_transfer=99)
    with pytest.raises(ValueError, match="needs sharpness_transfer > 0"):
        call(sharpness_alpha=4.0)
    with pytest.raises(ValueError, match="not supported with mesh_warp"):
        call(sharpness_transfer=2, mesh_warp=True)
    with pytest.raises(ValueError, match="not supported with estimator 'subject'"):
        call(sharpness_transfer=2, estimator="subject", subject_mask=np.zeros((3, 4, 4), np.float32))
    with pytest.raises(ValueError, match="does not support sharpness_transfer=2: the sharpness transfer is not sharded"):
        distributed.stabilize_sharded(None, None, 8, "crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0,
                                      sharpness_transfer=2)


def test_meta_block_shape(pkg):
    from vstab_amd import sharpness_transfer as st

    energy = np.array([2 ** 32 * 6, 2 ** 32 * 3, 0], np.int64)
    ratios = np.array([[0, 0], [2.0, 0], [0, 0]], np.float32)
    block = st.meta_block(1, 16.0, energy, (3, 4), ratios, np.array([0, 6, 0], np.int32), (4, 3))
    assert list(block) == ["version", "radius", "alpha", "min_ratio", "sharpness", "frames_sharpened", "ratio_max",
                           "transferred_fraction_mean", "transferred_fraction_max"]
    assert block == {"version": 1, "radius": 1, "alpha": 16.0, "min_ratio": 1.1, "sharpness": [1.0, 0.5, 0.0], "frames_sharpened": 1,
                     "ratio_max": 2.0, "transferred_fraction_mean": float(np.mean(np.array([0.0, 0.5, 0.0]))),
                     "transferred_fraction_max": 0.5}
    import json

    assert json.loads(json.dumps(block)) == block


def test_header_states_both_rules_and_native_binds_them(pkg):
    import ctypes as C

    from vstab_amd import native

    raw = (ROOT / "include" / "vstab.h").read_text()
    flat = re.sub(r"\s*\n \*\s*", " ", raw)
    for phrase in ("q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0", "Y(x, y) = (q(r) + 2 * q(g) + q(b)) >> 2",
                   "gx = Y(x + 1, y) - Y(x, y)", "gy = Y(x, y + 1) - Y(x, y)", "h * w <= 2^30", "w == 1 or h == 1 gives 0",
                   "D = (|s_r - o_r| + |s_g - o_g|) + |s_b - o_b|", "w = ratio / (ratio + alpha * D)", "den = den + w",
                   "dst_c = (o_c + num_c) / (1.0f + den)", "mask == 1.0f (padded): untouched", "The mask is never written".lower(),
                   'Timing kind "sharp_transfer"', 'timing kind "sharpness"'):
        assert phrase in flat or phrase in flat.lower(), phrase
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    for name, count, method in (("vstab_frame_sharpness_batch", 6, "frame_sharpness_batch"),
                                ("vstab_sharp_transfer_batch", 19, "sharp_transfer_batch")):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, f"include/vstab.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = native._SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == count
        for ptxt, a in zip(params, args):
            assert a is (C.c_void_p if "*" in ptxt else C.c_float if ptxt.startswith("float") else C.c_int), ptxt
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), name) and hasattr(native.Context, method)
    assert native.load_library().vstab_abi_version() == 1
    makefile = (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert "vstab_sharp.hip" in makefile


def test_node_list_and_schema(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerSharpnessTransfer
    assert node not in nodes.NODE_CLASSES and len(nodes.NODE_CLASSES) == 6
    before = asyncio.run(nodes.VideoStabilizerAmdFillBlendExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdSharpnessExtension().get_node_list())
    assert node not in before and listed == before + [node]
    assert type(asyncio.run(vstab_amd.comfy_entrypoint())) is nodes.VideoStabilizerAmdMaskedExtension
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_sharpness_transfer" and schema.display_name == "Video Stabilizer Sharpness Transfer"
    assert [s.id for s in schema.inputs] == ["frames", "frames_stabilized", "meta", "radius", "alpha", "padding_mask"]
    assert [s.id for s in schema.outputs] == ["frames", "meta"]

    def opt(sock, key):   # the stand-in sockets keep their options in a dict, ComfyUI's as attributes
        return sock.options[key] if isinstance(getattr(sock, "options", None), dict) else getattr(sock, key)

    radius, alpha, mask = schema.inputs[3], schema.inputs[4], schema.inputs[5]
    assert (opt(radius, "default"), opt(radius, "min"), opt(radius, "max")) == (2, 1, 16)
    assert (opt(alpha, "default"), opt(alpha, "min"), opt(alpha, "max")) == (16.0, 0.0, 1024.0)
    assert opt(mask, "optional") is True
    with pytest.raises(ValueError, match="meta"):             # a meta without matrices is refused before any GPU work
        node.execute(None, None, {"frames": 3}, 2, 16.0)


# ---- the referee ----------------------------------------------------------------------------------------------------------
def test_referee_blurred_frames_gain_and_sharp_frames_keep_their_bits(oracle):
    """9 frames of 160 x 120 of one procedural texture under a known similarity shake, the TRUE matrices, frames 2 and 6
    blurred with a 5 x 5 box, noise of sigma 0.005 on every frame (tests/sharpness_restatement.py: referee_clip, referee).
    With radius 2 and the default alpha of 16 the PSNR of each blurred frame's output against the warp of its sharp,
    noise-free render rises; a frame that is not blurred has no neighbour a tenth sharper than itself and comes back bit
    for bit.  Measured when this test was written (recorded in the profiles/ report of the feature): 25.11 -> 35.99 dB and
    25.14 -> 35.14 dB, a mean gain of 10.45 dB; the energy ratio of a sharp neighbour to a blurred frame is about 7.5."""
    clip = S.referee_clip()
    assert clip["blurred"] == [2, 6] and clip["frames"].shape == (9, 120, 160, 3)
    energy = S.frame_sharpness(clip["frames"])
    r = S.referee()
    ratios = r["ratios"]
    for i in range(9):
        if i in clip["blurred"]:
            assert (ratios[i] > 5.0).all(), ratios[i]                    # every neighbour within 2 frames is far sharper
        else:
            assert (ratios[i] == 0.0).all(), (ratios[i], energy)         # nothing is a tenth sharper than a sharp frame
    for before, after in zip(r["before"], r["after"]):
        print(f"referee, alpha 16: {before:.2f} dB -> {after:.2f} dB")
        assert after > before
    print(f"referee, alpha 16: mean gain {r['gain_mean']:.2f} dB")
    keep = [i for i in range(9) if i not in clip["blurred"]]
    assert np.array_equal(_bits(r["out"][keep]), _bits(r["warped"][keep])) and (r["count"][keep] == 0).all()
    # padded pixels of the blurred frames keep their bits too, and every own pixel some candidate reaches was transferred
    for i in clip["blurred"]:
        padded = r["mask"][i] == 1.0
        assert padded.any() and np.array_equal(_bits(r["out"][i][padded]), _bits(r["warped"][i][padded]))
        assert 0 < r["count"][i] <= int((~padded).sum())
    for alpha in (0.0, 4.0, 64.0):                                         # for orientation: the sweep the report tabulates
        print(f"referee, alpha {alpha:g}: mean gain {S.referee(alpha)['gain_mean']:.2f} dB")
