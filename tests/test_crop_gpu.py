"""GPU tests for framing_mode="crop": vstab_crop_analysis and vstab_common_coverage vs the oracle and vs the NumPy restatement
of the morphology (bit-exact integers and bytes, at the shapes of tests/crop_cases.py where the kernels of csrc/vstab_crop.hip
change path), and the reference-pinned properties of crop mode (KA8, scripts/check_crop_aspect_ratio.py:82-120,173-233)."""

import numpy as np
import pytest

from tests import crop_cases as K
from tests import crop_restatement as R
from tests.util import test_matrices as make_matrices

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["similarity", "perspective", "translation", "far"])
@pytest.mark.parametrize("size", [(73, 45), (212, 120)])
def test_crop_analysis_matches_oracle(ctx, oracle, kind, size):
    w, h = size
    mats = make_matrices(6 if kind != "far" else 2, w, h, kind).astype(np.float32)
    ref_bbox, ref_common = oracle.crop_analysis(mats, (w, h), (w, h))
    bbox, common = ctx.crop_analysis(mats, (w, h), (w, h))
    assert np.array_equal(bbox, ref_bbox) and np.array_equal(common, ref_common)


def _sizes(case):
    return (case.src[1], case.src[0]), (case.out[1], case.out[0])   # (w, h), as the entry points take them


def _assert_case(ctx, oracle, case):
    """The four comparisons every case makes; returns the GPU's (bbox, common, common_coverage)."""
    ref = K.reference(oracle, case)
    src, out = _sizes(case)
    bbox, common = ctx.crop_analysis(case.mats, src, out)
    covered = ctx.common_coverage(case.mats, src, out)
    assert bbox.dtype == np.int32 and common.dtype == np.uint8 and covered.dtype == bool
    assert np.array_equal(bbox, ref.bbox), (bbox.tolist(), ref.bbox.tolist())
    assert np.array_equal(common, ref.common)
    assert np.array_equal(bbox, ref.restated_bbox) and np.array_equal(common, ref.restated_common)
    assert np.array_equal(covered, R.common_of(ref.cov))
    assert np.array_equal(R.erode3(covered).astype(np.uint8), common)
    return bbox, common, covered


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_crop_kernels_match_oracle_and_restatement(ctx, oracle, case):
    _assert_case(ctx, oracle, case)


def _rect(h, w, x0, y0, x1, y1):
    """uint8 [h,w]: 1 inside the inclusive rectangle."""
    out = np.zeros((h, w), np.uint8)
    out[y0:y1 + 1, x0:x1 + 1] = 1
    return out


@pytest.mark.parametrize("dx,dy", K.EDGE_SHIFTS)
def test_edge_closing_closed_form(ctx, oracle, dx, dy):
    """An integer shift (dx, dy) covers the rectangle [max(dx,0), w-1+min(dx,0)] x [max(dy,0), h-1+min(dy,0)].  Pixels outside
    the image constrain neither dilate nor erode, so the closing fills a gap of exactly 1 px up to the image edge and leaves a
    gap of 2 px as it is; the erosion of `common` moves a side inwards by 1 px only where that side is not the image edge."""
    h, w = K.EDGE
    x0, y0, x1, y1 = max(dx, 0), max(dy, 0), w - 1 + min(dx, 0), h - 1 + min(dy, 0)

    def closed(lo, hi, size):
        return (0 if lo == 1 else lo), (size - 1 if hi == size - 2 else hi)

    def eroded(lo, hi, size):
        return (lo if lo == 0 else lo + 1), (hi if hi == size - 1 else hi - 1)

    (cx0, cx1), (cy0, cy1) = closed(x0, x1, w), closed(y0, y1, h)
    (ex0, ex1), (ey0, ey1) = eroded(x0, x1, w), eroded(y0, y1, h)
    bbox, common, covered = _assert_case(ctx, oracle, K.BY_NAME[f"edge_shift_{dx}_{dy}"])
    assert bbox.tolist() == [[cx0, cy0, cx1, cy1]]
    assert np.array_equal(covered, _rect(h, w, x0, y0, x1, y1).astype(bool))
    assert np.array_equal(common, _rect(h, w, ex0, ey0, ex1, ey1))


def test_edge_closing_batch_closed_form(ctx, oracle):
    """The five 1 px shifts in one call: every frame's closing is the full frame; they share columns 1..w-2 and rows 1..h-2,
    none of whose sides is the image edge."""
    h, w = K.EDGE
    bbox, common, covered = _assert_case(ctx, oracle, K.BY_NAME["edge_shift_batch"])
    assert bbox.tolist() == [[0, 0, w - 1, h - 1]] * 5
    assert np.array_equal(covered, _rect(h, w, 1, 1, w - 2, h - 2).astype(bool))
    assert np.array_equal(common, _rect(h, w, 2, 2, w - 3, h - 3))


def test_empty_and_full_frames(ctx, oracle):
    bbox, common, covered = _assert_case(ctx, oracle, K.BY_NAME["mixed_empty_frames_1_and_3"])
    assert bbox[[1, 3]].tolist() == [[-1] * 4] * 2
    assert (bbox[[0, 2, 4], 2] > bbox[[0, 2, 4], 0]).all() and (bbox[[0, 2, 4]] >= 0).all()
    assert not common.any() and not covered.any()
    case = K.BY_NAME["full_identity_n3"]
    h, w = case.out
    bbox, common, covered = _assert_case(ctx, oracle, case)
    assert bbox.tolist() == [[0, 0, w - 1, h - 1]] * 3 and common.all() and covered.all()


def test_workspace_reuse_matches_fresh_context(pkg, ctx, oracle):
    """d_gray_tmp and h_fit only grow and other stages share them: a large call, then a small one, then the two entry points
    interleaved on one context give the bytes that a fresh context gives for each."""
    from vstab_amd import native

    big, small, mid = K.BY_NAME["stride_pixels_1100x1920"], K.BY_NAME["bw0_single_block_perspective"], K.BY_NAME["distinct_51x80_similarity"]
    used = native.Context()
    try:
        for case, entry in ((big, "crop_analysis"), (small, "crop_analysis"), (mid, "common_coverage"), (mid, "crop_analysis")):
            ref = K.reference(oracle, case)
            src, out = _sizes(case)
            fresh = native.Context()
            try:
                want = getattr(fresh, entry)(case.mats, src, out)
            finally:
                fresh.close()
            got = getattr(used, entry)(case.mats, src, out)
            if entry == "crop_analysis":
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case.name
                assert np.array_equal(got[0], ref.bbox) and np.array_equal(got[1], ref.common), case.name
            else:
                assert np.array_equal(got, want) and np.array_equal(got, R.common_of(ref.cov)), case.name
    finally:
        used.close()


def test_size_guards_refuse_before_any_launch(pkg, ctx, oracle):
    """out_h = out_w = 46341 has 2^31 + 4633 pixels, beyond the int pixel index of the kernels: both entry points refuse it, and
    a source side of 32768 (beyond the short saturation of the coverage rule), with a message.  The refusals are
    VSTAB_REQUIREs (status 2; a failing HIP call gives 1), which both entry points evaluate before their first HIP call: no
    workspace is reserved, no kernel launched and no output byte written.  The context works afterwards."""
    from vstab_amd import native

    lib = native.load_library()
    mats = np.ascontiguousarray(make_matrices(2, 73, 45, "similarity").astype(np.float32))
    side = 46341
    assert side * side > 2**31 - 1 > (side - 1) * (side - 1)
    probes = [0, 1, side * side // 2, side * side - 1]
    for sh, sw, oh, ow, message in ((45, 73, side, side, b"output too large"), (32768, 73, 45, 73, b"source larger than 32767 px"),
                                    (45, 32768, 45, 73, b"source larger than 32767 px")):
        for entry in ("vstab_crop_analysis", "vstab_common_coverage"):
            bbox = np.full((2, 4), 12345, np.int32)
            common = np.zeros(oh * ow, np.uint8)   # untouched zero pages: never resident unless the call writes them
            args = [ctx.handle, mats.ctypes.data, 2, sh, sw, oh, ow] + ([bbox.ctypes.data] if entry == "vstab_crop_analysis" else [])
            rc = getattr(lib, entry)(*args, common.ctypes.data)
            assert rc == 2, (entry, rc)
            assert entry.encode() in lib.vstab_last_error() and message in lib.vstab_last_error()
            assert (bbox == 12345).all() and not common[[p for p in probes if p < common.size]].any()
    for entry in (ctx.crop_analysis, ctx.common_coverage):
        with pytest.raises(native.VstabError, match="output too large"):
            entry(mats, (73, 45), (side, side))
        with pytest.raises(native.VstabError, match="source larger than 32767 px"):
            entry(mats, (73, 32768), (73, 45))
    _assert_case(ctx, oracle, K.BY_NAME["one_frame"])


def test_largest_rectangle_search(pkg):
    from vstab_amd import crop_solver as cs

    mask = np.zeros((45, 73), np.uint8)
    mask[5:40, 6:70] = 1
    x0, y0, cw, ch = cs._largest_aspect_ratio_rectangle(mask, 73, 45)
    assert abs(cw / ch - 73 / 45) < 1e-9 and mask[int(y0):int(y0 + ch), int(x0):int(np.ceil(x0 + cw))].all()
    assert ch == 35.0 or int(np.ceil(73 / 45 * (ch + 1))) > 64  # cannot grow further
    assert cs._largest_aspect_ratio_rectangle(np.zeros((10, 10), np.uint8), 10, 10) is None


@pytest.mark.parametrize("mode", ["translation", "similarity"])
@pytest.mark.parametrize("keep_fov", [0.0, 0.6])
def test_flow_crop_mode_properties(pkg, ctx, mode, keep_fov):
    """KA8: crop mode has a zero padding mask, the crop keeps the frame aspect (1e-6) and a uniform scale."""
    from tests.test_dis_gpu import moving_clip
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    w, h, n = 480, 270, 8
    gray, _ = moving_clip(n, h, w, seed=11)
    frames = np.ascontiguousarray(np.repeat(gray[..., None].astype(np.float32) / 255.0, 3, axis=-1))
    res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop", mode, False, 0.7, 0.5, keep_fov, (127, 127, 127), 16.0)
    assert res.frames.shape == (n, h, w, 3)
    assert float(res.masks.max()) == 0.0 and res.meta["padding_fraction_max"] == 0.0
    fr = res.meta["framing"]
    assert fr["mode"] == "crop" and fr["keep_fov_status"] in ("met", "clamped", "disabled", "failed")
    cw, ch = fr["crop_size"]
    assert abs(cw / ch - w / h) < 1e-6
    assert fr["keep_fov_effective"] == 1.0 and fr["actual_content_ratio"] == 1.0
    if keep_fov > 1e-6:
        assert fr["keep_fov_requested"] == keep_fov and res.meta["keep_fov_applied"] is True
    for entry in res.meta["stabilization_warp"]["per_frame"]:
        m = np.array(entry["applied_matrix"])
        if mode == "translation":
            assert abs(m[0, 0] - m[1, 1]) < 1e-6 and abs(m[0, 1]) < 1e-6 and abs(m[1, 0]) < 1e-6  # uniform scale, no shear
    assert list(res.meta["framing"].keys())[:4] == ["mode", "input_size", "padding_color_rgb", "min_content_ratio"]
    import json

    json.dumps(res.meta)
