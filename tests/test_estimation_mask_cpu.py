"""Estimation mask, the parts that need no GPU: the NumPy restatement of the rule on hand-made cases, the public surface
(keyword, node, exported symbols) and the ValueErrors that are raised before any GPU work."""

import asyncio
import inspect

import numpy as np
import pytest

from tests import estimation_mask_restatement as R


# ---- the restatement itself, on cases small enough to do by hand ---------------------------------------------------------
def test_empty_and_full_masks():
    for work in (None, (8, 6)):
        h, w = (12, 16)
        empty = R.block_grid(np.zeros((h, w), np.float32), 3, work, 4, 2)
        full = R.block_grid(np.ones((1, h, w), np.float32), 3, work, 4, 2)
        gh, gw = (3, 4) if work is None else (2, 2)
        assert empty.shape == full.shape == (3, gh, gw) and empty.dtype == np.uint8
        assert not empty.any() and (full == 1).all()
        assert R.admitted(empty).all() and not R.admitted(full).any()


def test_subject_is_above_half_or_not_finite():
    m = np.array([[0.0, 0.5, 0.5000001, 1.0, -3.0, np.nan, np.inf, -np.inf]], np.float32)
    assert R.subject(m).tolist() == [[False, False, True, True, False, True, True, True]]


@pytest.mark.parametrize("corner", [(0, 0), (0, 15), (11, 0), (11, 15)])
def test_one_subject_pixel_at_each_corner(corner):
    """16x12 -> 8x6 (2x2 footprints), step 4 -> samples at X in {0, 4}, Y in {0, 4}; margin 1 reaches |d| <= 1."""
    m = np.zeros((12, 16), np.float32)
    m[corner] = 1.0
    cov = R.covered(m, (8, 6))
    want = np.zeros((6, 8), bool)
    want[corner[0] // 2, corner[1] // 2] = True
    assert np.array_equal(cov, want)
    got = R.block_grid(m, 1, (8, 6), 4, 1)[0]
    # covered working pixel: (0,0), (0,7), (5,0) or (5,7); samples: (0,0), (0,4), (4,0), (4,4)
    expect = np.zeros((2, 2), np.uint8)
    Y, X = corner[0] // 2, corner[1] // 2
    for gy in range(2):
        for gx in range(2):
            expect[gy, gx] = abs(Y - 4 * gy) <= 1 and abs(X - 4 * gx) <= 1
    assert np.array_equal(got, expect)
    assert got.sum() == (1 if corner[1] == 0 else 0)   # rows 0 and 5 are within 1 of samples 0 and 4; column 7 is 3 from 4


def test_margin_zero_and_margin_larger_than_the_image():
    m = np.zeros((12, 16), np.float32)
    m[4, 9] = 0.75                       # no downscale: covered (4, 9); not a sample (step 4: X in 0,4,8,12)
    assert not R.block_grid(m, 1, None, 4, 0).any()
    m[4, 8] = 0.75                       # sample (gy 1, gx 2) itself
    z = R.block_grid(m, 1, None, 4, 0)[0]
    assert z.sum() == 1 and z[1, 2] == 1
    assert (R.block_grid(m, 2, None, 4, 64) == 1).all()    # the square covers the whole image from every sample
    one = R.block_grid(m, 1, None, 4, 1)[0]                # (4,8) and (4,9): |dX| <= 1 from X = 8 only
    assert one.sum() == 1 and one[1, 2] == 1


def test_non_integer_footprints_overlap():
    """5 -> 3 columns: footprints [0,2), [1,4), [3,5): source column 1 belongs to working columns 0 and 1."""
    m = np.zeros((1, 5), np.float32)
    m[0, 1] = 1
    assert R.covered(m, (3, 1)).tolist() == [[True, True, False]]
    m[:] = 0
    m[0, 3] = 1
    assert R.covered(m, (3, 1)).tolist() == [[False, True, True]]


def test_admission_needs_both_frames_and_poison_writes_nan():
    b = np.zeros((3, 1, 4), np.uint8)
    b[0, 0, 0] = 1
    b[1, 0, 1] = 1
    b[2, 0, 3] = 1
    adm = R.admitted(b)
    assert adm[:, 0].tolist() == [[False, False, True, True], [True, False, True, False]]
    grid = np.ones((2, 1, 4, 2), np.float32)
    p = R.poison(grid, b)
    assert np.isnan(p[~adm]).all() and (p[adm] == 1).all() and (grid == 1).all()


# ---- public surface -------------------------------------------------------------------------------------------------------
def test_keywords_and_exports(pkg):
    from vstab_amd import distributed, flow_pipeline, native

    sig = inspect.signature(flow_pipeline._stabilize_frames).parameters
    assert sig["estimation_mask"].kind is inspect.Parameter.KEYWORD_ONLY and sig["estimation_mask"].default is None
    assert sig["mask_margin"].kind is inspect.Parameter.KEYWORD_ONLY and sig["mask_margin"].default == 16
    assert inspect.signature(distributed.stabilize_sharded).parameters["estimation_mask"].default is None
    for name in ("vstab_mask_block_grid", "vstab_sample_fit_batch_masked", "vstab_sample_fit_batch_begin_masked"):
        assert name in native.EXPORTED_SYMBOLS
    assert inspect.signature(native.Context.sample_fit_batch).parameters["blocked"].default is None
    assert inspect.signature(native.Context.sample_fit_batch_begin).parameters["blocked"].default is None
    assert list(inspect.signature(native.Context.mask_block_grid).parameters)[1:] == ["mask", "n_frames", "working_size", "step", "margin"]


def test_masked_node_schema(pkg):
    from vstab_amd import nodes

    assert len(nodes.NODE_CLASSES) == 6 and nodes.VideoStabilizerFlowMasked not in nodes.NODE_CLASSES
    import vstab_amd

    ext = asyncio.run(vstab_amd.comfy_entrypoint())              # what ComfyUI loads
    assert isinstance(ext, nodes.VideoStabilizerAmdExtension)
    listed = asyncio.run(ext.get_node_list())
    assert len(listed) == 8 and listed[:6] == nodes.NODE_CLASSES and listed[6] is nodes.VideoStabilizerTemporalFill
    assert listed[7] is nodes.VideoStabilizerFlowMasked
    s = nodes.VideoStabilizerFlowMasked.define_schema()
    flow = nodes.VideoStabilizerFlow.define_schema()
    assert s.node_id == "video_stabilizer_flow_masked" and s.display_name == "Video Stabilizer Flow (Masked)"
    assert [i.id for i in s.inputs] == [i.id for i in flow.inputs] + ["exclude_mask", "mask_margin"]
    assert [o.id for o in s.outputs] == [o.id for o in flow.outputs]
    for a, b in zip(s.inputs, flow.inputs):
        assert a.kind == b.kind and a.options == b.options
    mask_in, margin = s.inputs[-2], s.inputs[-1]
    assert mask_in.kind.upper() == "MASK"
    assert margin.kind.upper() == "INT" and margin.options["default"] == 16 and margin.options["min"] == 0 and margin.options["max"] == 64


def _context(pkg, n=4, h=24, w=32):
    import torch

    from vstab_amd import host_math as hm

    return hm._normalize_video_input(torch.zeros((n, h, w, 3)))


ARGS = ("crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)


@pytest.mark.parametrize("margin", [-1, 65, 1000])
def test_margin_out_of_range(pkg, margin):
    import torch

    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError, match=r"mask_margin=.* outside \[0, 64\]"):
        fp._stabilize_frames(_context(pkg), *ARGS, estimation_mask=torch.zeros((24, 32)), mask_margin=margin)


@pytest.mark.parametrize("shape", [(24, 31), (3, 24, 32), (4, 32, 24), (4, 24, 32, 1), (32,)])
def test_shape_mismatch_names_both_shapes(pkg, shape):
    import torch

    from vstab_amd import flow_pipeline as fp

    with pytest.raises(ValueError) as err:
        fp._stabilize_frames(_context(pkg), *ARGS, estimation_mask=torch.zeros(shape))
    assert str(tuple(shape)) in str(err.value) and "[4,24,32]" in str(err.value)


def test_stated_limits(pkg, monkeypatch):
    import torch

    from vstab_amd import distributed
    from vstab_amd import flow_pipeline as fp

    mask = torch.zeros((24, 32))
    with pytest.raises(ValueError, match="masked corner detector"):
        fp._stabilize_frames(_context(pkg), *ARGS, estimator="classic", estimation_mask=mask)
    with pytest.raises(ValueError, match="no samples to drop"):
        fp._stabilize_frames(_context(pkg), *ARGS, estimator="flow_phase_correlate", estimation_mask=mask)
    monkeypatch.setenv("VSTAB_FLOW_BACKEND", "phase_correlate")   # the Flow node on its fallback estimator
    with pytest.raises(ValueError, match="no samples to drop"):
        fp._stabilize_frames(_context(pkg), *ARGS, estimation_mask=mask)
    monkeypatch.delenv("VSTAB_FLOW_BACKEND")
    with pytest.raises(ValueError, match="does not support estimation_mask"):
        distributed.stabilize_sharded(None, None, 4, *ARGS, estimation_mask=mask)


def test_bypasses_ignore_the_mask(pkg):
    """0 / 1 frames: returned before any GPU work, with the reference's meta (no estimation_mask key)."""
    import torch

    from vstab_amd import flow_pipeline as fp

    mask = torch.ones((24, 32))
    for n in (0, 1):
        with_mask = fp._stabilize_frames(_context(pkg, n=n) if n else _EMPTY(pkg), *ARGS, estimation_mask=mask)
        without = fp._stabilize_frames(_context(pkg, n=n) if n else _EMPTY(pkg), *ARGS)
        assert with_mask.meta == without.meta and "estimation_mask" not in with_mask.meta


def _EMPTY(pkg):
    import dataclasses

    return dataclasses.replace(_context(pkg, n=1), frames=[], batch=None)


def test_meta_block_from_fit_counts(pkg):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import native

    table = np.zeros((3, 3), native.FIT_DTYPE)
    table["total_points"][:, :] = np.array([100, 40, 70])[:, None]
    block = fp.estimation_mask_meta(table, 16, 1, 100)
    assert block == {"margin": 16, "mask_frames": 1, "blocked_fraction_mean": pytest.approx((0.0 + 0.6 + 0.3) / 3),
                     "blocked_fraction_max": pytest.approx(0.6), "admitted_points_min": 40}
