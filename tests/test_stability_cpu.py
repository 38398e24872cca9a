"""CPU: the stability report's rule on its NumPy restatement (tests/stability_restatement.py, which the GPU tests hold the
kernel to exactly), and the host side: psnr_db, the meta block, keyword checks, node, header."""

import asyncio
import ctypes as C
import inspect
import json
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import stability_restatement as R
from tests.util import synth_frames

ROOT = Path(__file__).resolve().parents[1]
TWO32 = 2 ** 32


def _pixel(r, g, b):
    return np.array([[[[r, g, b]]]], np.float32)    # [1,1,1,3]


# ---- the rule, on the restatement -----------------------------------------------------------------------------------------
def test_one_pixel_one_over_255_is_the_exact_integer():
    """d = float32(1/255) - 0 per channel: q = floor(d^2 * 2^32) worked out in rationals, no floating point involved."""
    d = Fraction(float(np.float32(1.0) / np.float32(255.0)))       # the float32 value, exactly
    expected = 3 * ((d * d * TWO32).numerator // (d * d * TWO32).denominator)
    v = np.float32(1.0) / np.float32(255.0)
    sse, count = R.frame_sse(_pixel(v, v, v), _pixel(0, 0, 0))
    assert int(sse[0]) == expected == 3 * 66051 and count.tolist() == [1]
    # the other order of the subtraction squares to the same value
    assert int(R.frame_sse(_pixel(0, 0, 0), _pixel(v, v, v))[0][0]) == expected


def test_hand_computed_differences():
    a = np.zeros((2, 1, 2, 3), np.float32)
    b = np.zeros((2, 1, 2, 3), np.float32)
    a[0, 0, 0] = (0.5, 0.25, 1.0)          # 0.25 + 0.0625 + 1 = 1.3125
    b[0, 0, 1] = (0.0, 2.0 ** -16, 2.0 ** -17)   # 2^-32 -> 1, 2^-34 -> 0 (truncation)
    a[1, 0, 1] = (1.5, 0.0, 0.0)
    b[1, 0, 1] = (0.5, 0.0, 1.0)           # 1 + 0 + 1
    sse, count = R.frame_sse(a, b)
    assert [int(v) for v in sse] == [int(1.3125 * TWO32) + 1, 2 * TWO32] and count.tolist() == [2, 2]


@pytest.mark.parametrize("d,expected", [(2.0, 4 * TWO32), (3.0, 4 * TWO32), (np.inf, 4 * TWO32), (np.nan, 4 * TWO32),
                                        (-np.inf, 4 * TWO32), (1e30, 4 * TWO32), (1.999, None)])
def test_clamp_at_four(d, expected):
    """d^2 >= 4, inf and NaN all contribute the cap 4 * 2^32 = 2^34 per channel; just below 2 does not."""
    sse, count = R.frame_sse(_pixel(d, 0, 0), _pixel(0, 0, 0))
    if expected is None:
        dd = Fraction(float(np.float32(d)))
        expected = (dd * dd * TWO32).numerator // (dd * dd * TWO32).denominator
        assert expected < 4 * TWO32
    assert int(sse[0]) == expected and count.tolist() == [1]
    # inf - inf is NaN: the cap as well
    if np.isinf(d):
        assert int(R.frame_sse(_pixel(d, 0, 0), _pixel(d, 0, 0))[0][0]) == 4 * TWO32


def test_mask_convention():
    """valid iff mask <= 0.5: 0 and 0.5 are, 0.5000001, 1, NaN and inf are not (-inf is)."""
    values = np.array([0.0, 0.5, 0.5000001, 1.0, np.nan, np.inf, -np.inf], np.float32)
    assert R.valid_of(values, values.shape).tolist() == [True, True, False, False, False, False, True]
    a = np.ones((1, 1, 7, 3), np.float32)
    b = np.zeros((1, 1, 7, 3), np.float32)
    m = values.reshape(1, 1, 7)
    zero = np.zeros((1, 1, 7), np.float32)
    for ma, mb in ((m, None), (None, m), (m, zero), (zero, m), (m, m)):
        sse, count = R.frame_sse(a, b, ma, mb)
        assert count.tolist() == [3] and int(sse[0]) == 3 * 3 * TWO32
    # a pixel counts only if it is valid in BOTH frames
    sse, count = R.frame_sse(a, b, m, m[:, :, ::-1])
    assert count.tolist() == [int((R.valid_of(values, values.shape) & R.valid_of(values[::-1], values.shape)).sum())]
    # no common valid pixel: 0 and 0
    sse, count = R.frame_sse(a, b, np.ones((1, 1, 7), np.float32), None)
    assert count.tolist() == [0] and int(sse[0]) == 0


def test_a_large_frame_of_capped_differences_needs_64_bits():
    a = np.full((1, 64, 64, 3), 3.0, np.float32)
    sse, count = R.frame_sse(a, np.zeros_like(a))
    assert int(sse[0]) == 3 * 64 * 64 * 2 ** 34 > 2 ** 32 and count.tolist() == [64 * 64]


def test_consecutive_form_equals_separate_pairs():
    clip = synth_frames(5, 7, 9, seed=2)
    mask = (np.random.default_rng(0).uniform(0, 1, (5, 7, 9)) < 0.3).astype(np.float32)
    sse, count = R.consecutive(clip, mask)
    for k in range(4):
        s1, c1 = R.frame_sse(clip[k:k + 1], clip[k + 1:k + 2], mask[k:k + 1], mask[k + 1:k + 2])
        assert int(sse[k]) == int(s1[0]) and count[k] == c1[0]


def test_locked_camera_kind_of_clip_gains_on_the_restatement():
    """The sign the GPU sanity test asserts (gain_db > 0 for a camera_lock run on the analytic shake clip), on the restatement
    alone: the shaken clip of tests/test_analytic_gpu.py's kind (translation shake, amp 1) against what a locked camera
    returns -- the static view up to the measured estimation error (a residual walk of <= 0.05 px steps) with the borders
    the shake exposed masked out."""
    import torch

    import bench
    from tests.util import shake_path

    n, w, h = 8, 240, 136
    cam = shake_path(n, w, h, "translation", seed=5, amp=8.0)       # steps scale with the frame: up to +-6 x +-4 px here too
    shaken = bench.synth_clip(n, 0, h, w, torch.device("cpu"), mats=cam).numpy()
    rng = np.random.default_rng(1)
    residual = np.tile(np.eye(3), (n, 1, 1))
    residual[:, 0, 2] = np.cumsum(rng.uniform(-0.05, 0.05, n))
    residual[:, 1, 2] = np.cumsum(rng.uniform(-0.05, 0.05, n))
    locked = bench.synth_clip(n, 0, h, w, torch.device("cpu"), mats=residual).numpy()
    yy, xx = np.mgrid[0:h, 0:w]
    mask = np.stack([((xx - m[0, 2] < 0) | (xx - m[0, 2] > w - 1) | (yy - m[1, 2] < 0) | (yy - m[1, 2] > h - 1)) for m in cam]).astype(np.float32)
    before, after = R.itf_block(shaken), R.itf_block(locked, mask)
    print(before, after)
    assert before["itf_db"] is not None and after["itf_db"] is not None
    assert R.report(before, after)["gain_db"] > 0


# ---- host arithmetic --------------------------------------------------------------------------------------------------------
def test_psnr_db(pkg):
    from vstab_amd import stability

    got = stability.psnr_db([0, 0, 3 * TWO32, 3 * 100 * TWO32 // 4, 7], [5, 0, 1, 100, 0])
    assert got.dtype == np.float64
    assert got[0] == np.inf and np.isnan(got[1]) and got[2] == 0.0 and np.isnan(got[4])
    assert got[3] == 10.0 * np.log10(4.0)                         # mean squared error 1/4
    assert np.array_equal(got, R.psnr_db([0, 0, 3 * TWO32, 3 * 100 * TWO32 // 4, 7], [5, 0, 1, 100, 0]), equal_nan=True)
    # sums above 2^53 go through float64 once
    big = 3 * 2073600 * 2 ** 33
    assert stability.psnr_db([big], [2073600])[0] == 10.0 * np.log10(3.0 * 2073600 * TWO32 / float(big))
    with pytest.raises(ValueError, match="2 sums and 1 counts"):
        stability.psnr_db([1, 2], [1])


def test_summary_and_report_block_layout(pkg):
    from vstab_amd import stability

    sse = [3 * 10 * TWO32 // 100, 0, 5, 3 * 10 * TWO32 // 10000, 3 * 10 * TWO32]
    count = [10, 10, 0, 10, 10]
    block = stability.summary(sse, count, 20)
    psnr = R.psnr_db(sse, count)
    finite = psnr[np.isfinite(psnr)]
    assert list(block) == ["pairs", "itf_db", "psnr_db_min", "pairs_without_overlap", "overlap_fraction_mean"]
    assert block == {"pairs": 5, "itf_db": float(np.mean(finite)), "psnr_db_min": float(np.min(finite)), "pairs_without_overlap": 1,
                     "overlap_fraction_mean": float(np.mean(np.array(count, np.float64) / 20.0))}
    assert finite.size == 3 and block["psnr_db_min"] == 0.0
    skipped = stability.summary(sse, count, 20, skip=[4, 2])
    assert skipped["pairs"] == 3 and skipped["pairs_without_overlap"] == 0 and skipped["psnr_db_min"] > 0.0
    nothing = stability.summary([0, 9], [4, 0], 4)
    assert nothing["itf_db"] is None and nothing["psnr_db_min"] is None and nothing["pairs"] == 2
    empty = stability.summary([], [], 4)
    assert empty == {"pairs": 0, "itf_db": None, "psnr_db_min": None, "pairs_without_overlap": 0, "overlap_fraction_mean": 0.0}

    report = stability.report_block(skipped, block)
    assert list(report) == ["method", "version", "before", "after", "gain_db"]
    assert report["method"] == "itf" and report["version"] == 1 and report["before"] is skipped and report["after"] is block
    assert report["gain_db"] == block["itf_db"] - skipped["itf_db"]
    assert stability.report_block(nothing, block)["gain_db"] is None and stability.report_block(block, nothing)["gain_db"] is None
    assert stability.report_block(None, block)["gain_db"] is None
    cut = stability.report_block(skipped, block, pairs_across_cuts=2)
    assert list(cut) == ["method", "version", "before", "after", "gain_db", "pairs_across_cuts"] and cut["pairs_across_cuts"] == 2
    assert report == R.report(skipped, block) and cut == R.report(skipped, block, 2)
    json.dumps(cut)                                                # plain Python values only


def test_keyword_validation_names_the_value(pkg):
    from vstab_amd import apply_pipeline, flow_pipeline, stability
    from vstab_amd import host_math as hm

    assert stability.check_request(True) is True and stability.check_request(False) is False
    for bad in (1, 0, "yes", None, 2.5, [True], np.bool_(True)):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            stability.check_request(bad)

    p = inspect.signature(flow_pipeline._stabilize_frames).parameters["stability_report"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    p = inspect.signature(apply_pipeline.apply_motion).parameters["stability_report"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False

    context = hm._normalize_video_input(synth_frames(3, 16, 24, seed=1))
    for estimator in ("flow", "classic"):
        with pytest.raises(ValueError, match="stability_report='on'"):      # before any GPU work
            flow_pipeline._stabilize_frames(context, "crop_and_pad", "similarity", False, 0.9, 0.8, 0.6, (0, 0, 0), 16.0,
                                            estimator=estimator, stability_report="on")
    with pytest.raises(ValueError, match="stability_report=1 "):
        apply_pipeline.apply_motion(context, {}, (0, 0, 0), stability_report=1)
    with pytest.raises(ValueError, match="stability_report=True is not supported with motion_blur=0.3"):
        apply_pipeline.apply_motion(context, {}, (0, 0, 0), motion_blur=0.3, stability_report=True)
    from vstab_amd import distributed

    for fn in (distributed.stabilize_sharded, distributed.apply_motion_sharded):     # the sharded paths do not take it
        assert "stability_report" not in inspect.signature(fn).parameters


def test_node_is_listed_by_the_new_extension_only(pkg):
    from vstab_amd import nodes

    node = nodes.VideoStabilizerStabilityReport
    assert len(nodes.NODE_CLASSES) == 6 and node not in nodes.NODE_CLASSES
    assert issubclass(nodes.VideoStabilizerAmdReportExtension, nodes.VideoStabilizerAmdFillExtension)
    before = asyncio.run(nodes.VideoStabilizerAmdFillExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdReportExtension().get_node_list())
    assert node not in before and listed == before + [node]
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_stability_report" and schema.display_name == "Video Stabilizer Stability Report"
    assert [s.id for s in schema.inputs] == ["frames", "padding_mask", "reference_frames"]
    assert [bool(s.options.get("optional")) for s in schema.inputs] == [False, True, True]
    assert [s.id for s in schema.outputs] == ["meta"] and schema.outputs[0].kind == "String"
    params = inspect.signature(node.execute).parameters
    assert params["padding_mask"].default is None and params["reference_frames"].default is None


def test_node_refuses_mismatched_sockets_by_name(pkg):
    """Shape and dtype are checked in front of any GPU work."""
    import torch

    from vstab_amd import nodes

    frames = torch.zeros((3, 8, 10, 3))
    for mask in (torch.zeros((3, 10, 8)), torch.zeros((2, 8, 10)), torch.zeros((8, 10)), torch.zeros((3, 8, 10, 2))):
        with pytest.raises(ValueError, match="'padding_mask' of shape"):
            nodes.VideoStabilizerStabilityReport.execute(frames, mask)
    with pytest.raises(ValueError, match="'padding_mask' must be a floating-point MASK, got torch.uint8"):
        nodes.VideoStabilizerStabilityReport.execute(frames, torch.zeros((3, 8, 10), dtype=torch.uint8))


def test_header_declares_what_native_binds_and_the_library_exports(pkg):
    from vstab_amd import native

    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "vstab.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+vstab_frame_sse_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/vstab.h does not declare vstab_frame_sse_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = native._SIGNATURES["vstab_frame_sse_batch"]
    assert res is C.c_int and len(params) == len(args) == 10
    for ptxt, a in zip(params, args):
        assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
    assert "vstab_frame_sse_batch" in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert hasattr(lib, "vstab_frame_sse_batch") and hasattr(native.Context, "frame_sse_batch")
    assert "vstab_stability.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    # the argument checks come in front of any GPU work, under the function's name
    raw = C.CDLL(str(native.LIB_PATH))
    raw.vstab_last_error.restype = C.c_char_p
    fn = raw.vstab_frame_sse_batch
    fn.argtypes, fn.restype = args, C.c_int
    assert fn(None, None, None, None, None, 1, 1, 1, None, None) != 0
    assert raw.vstab_last_error().decode().startswith("vstab_frame_sse_batch: NULL context")
