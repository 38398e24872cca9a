"""CPU: the properties of the spatial fill's rule on its NumPy restatement (tests/spatial_fill_restatement.py, which the GPU
tests hold the kernels to in bits), its quality condition, and the host side: keyword checks, meta block, node, header."""

import asyncio
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import spatial_fill_restatement as R
from tests.util import synth_frames

ROOT = Path(__file__).resolve().parents[1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ring(h, w):
    """A stabilizer-shaped border: top and left min(h, w) // 12, bottom about half that."""
    b = max(1, min(h, w) // 12)
    hole = np.zeros((h, w), bool)
    hole[:b] = hole[:, :b] = True
    hole[h - (b // 2 + 1):] = True
    return hole


SHAPES = [(1, 1), (1, 7), (3, 5), (17, 9), (65, 33), (37, 53)]


# ---- the rule's guarantees, on the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_frame_without_holes_comes_back_bit_identical(shape):
    h, w = shape
    img = synth_frames(1, h, w, seed=3)[0]
    for mask in (np.zeros((h, w), np.float32), np.full((h, w), 0.5, np.float32), np.full((h, w), -np.inf, np.float32)):
        out, holes, filled = R.fill_frame(img, mask)
        assert np.array_equal(_bits(out), _bits(img)) and holes == 0 and filled == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_valid_pixels_never_change_and_fill_stays_in_range(shape):
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    img = synth_frames(1, h, w, seed=4)[0]
    for density in (0.01, 0.5, 0.99):
        hole = rng.uniform(0, 1, (h, w)) < density
        out, holes, filled = R.fill_frame(img, hole.astype(np.float32))
        assert out.dtype == np.float32 and holes == int(hole.sum())
        assert np.array_equal(_bits(out)[~hole], _bits(img)[~hole])
        if hole.all():
            assert filled == 0 and np.array_equal(_bits(out), _bits(img))
            continue
        assert filled == holes
        lo, hi = img[~hole].min(axis=0), img[~hole].max(axis=0)
        assert (out >= lo - 1e-6).all() and (out <= hi + 1e-6).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_all_hole_frame_is_untouched(shape):
    h, w = shape
    img = synth_frames(1, h, w, seed=6)[0]
    for value in (1.0, np.nan, np.inf, 0.75):
        out, holes, filled = R.fill_frame(img, np.full((h, w), value, np.float32))
        assert np.array_equal(_bits(out), _bits(img)) and holes == h * w and filled == 0


def test_hole_rule_is_not_mask_le_half():
    m = np.array([[np.nan, 0.5, np.inf, 0.75, 0.25, -np.inf, -1.0, np.nextafter(np.float32(0.5), np.float32(1.0)), 1.0, 0.0]], np.float32)
    assert R.holes_of(m).tolist() == [[True, False, True, True, False, False, False, True, True, False]]


def test_constant_frame_with_random_holes_is_filled_with_the_constant():
    c = np.full((37, 53, 3), 0.5, np.float32)
    hole = np.random.default_rng(0).uniform(0, 1, (37, 53)) < 0.6
    out, holes, filled = R.fill_frame(c, hole.astype(np.float32))
    assert holes == filled == int(hole.sum()) > 0
    assert (out == np.float32(0.5)).all()


@pytest.mark.parametrize("corner", [(0, 0), (0, 12), (8, 0), (8, 12)])
def test_single_valid_pixel_at_a_corner_spreads_everywhere(corner):
    """Every level above the pixel holds its value alone (v / 1), and up() of a constant is v * 0.75f + v * 0.25f.  That sum
    is v exactly for values with a short significand (3v is exact, so is the sum), which is what this test uses; for an
    arbitrary float32 it may differ from v in the last place, which the range property above bounds."""
    h, w = 9, 13
    img = synth_frames(1, h, w, seed=8)[0]
    value = np.array([0.25, 0.5, 0.8125], np.float32)
    img[corner] = value
    hole = np.ones((h, w), bool)
    hole[corner] = False
    out, holes, filled = R.fill_frame(img, hole.astype(np.float32))
    assert holes == filled == h * w - 1
    assert (out == value).all()


def test_pull_level_counts_only_valid_taps_and_clips_blocks():
    """3 x 3 -> 2 x 2: the last row and column give clipped blocks; an invalid tap's colour does not enter."""
    c = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    v = np.ones((3, 3), bool)
    v[0, 1] = False
    c2, v2 = R.pull_level(c, v)
    assert v2.all() and c2.shape == (2, 2, 3)
    assert np.array_equal(c2[0, 0], ((c[0, 0] + np.float32(0)) + (c[1, 0] + c[1, 1])) / np.float32(3))
    assert np.array_equal(c2[0, 1], (c[0, 2] + c[1, 2]) / np.float32(2))
    assert np.array_equal(c2[1, 1], c[2, 2])
    c3, v3 = R.pull_level(c, np.zeros((3, 3), bool))
    assert not v3.any() and (_bits(c3) == 0).all()


def test_upsample_indices_and_weights():
    """One row, coarse [a, b]: fine 0 -> a (far index clamped), 1 -> .75a + .25b, 2 -> .75b + .25a, 3 -> b."""
    f = np.zeros((1, 2, 3), np.float32)
    f[0, 0], f[0, 1] = 1.0, 3.0
    up = R.upsample(f, 1, 4)
    assert up[0, :, 0].tolist() == [1.0, 1.5, 2.5, 3.0]
    assert R.upsample(f, 1, 3)[0, :, 0].tolist() == [1.0, 1.5, 2.5]


# ---- quality: a condition, not a tuned number -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(135, 240), (270, 480)])
def test_fill_beats_the_mean_colour_on_the_procedural_texture(shape):
    """The fill's MSE over the holes of a border ring must be below that of the valid pixels' mean colour, the best any
    constant can do.  Observed: 17.5 dB against 15.2 dB at 135 x 240, 16.6 dB against 15.6 dB at 270 x 480 (black: about 5 dB)."""
    h, w = shape
    img = synth_frames(1, h, w, seed=5)[0]
    hole = _ring(h, w)
    out, _, filled = R.fill_frame(img, hole.astype(np.float32))
    assert filled == int(hole.sum()) > 0
    truth = img.astype(np.float64)[hole]
    mse_fill = float(np.mean((out.astype(np.float64)[hole] - truth) ** 2))
    mean_colour = img[~hole].astype(np.float64).mean(axis=0)
    mse_mean = float(np.mean((mean_colour[None] - truth) ** 2))
    mse_black = float(np.mean(truth ** 2))
    print(f"{h}x{w}: fill {-10 * np.log10(mse_fill):.2f} dB, mean colour {-10 * np.log10(mse_mean):.2f} dB, "
          f"black {-10 * np.log10(mse_black):.2f} dB")
    assert mse_fill < mse_mean < mse_black


# ---- host code ------------------------------------------------------------------------------------------------------------
def test_keyword_validation_names_the_value(pkg):
    from vstab_amd import apply_pipeline, flow_pipeline, spatial_fill
    from vstab_amd import host_math as hm

    assert spatial_fill.check_request(True) is True and spatial_fill.check_request(False) is False
    for bad in (1, 0, "yes", None, 2.5, [True], np.bool_(True)):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            spatial_fill.check_request(bad)

    p = inspect.signature(flow_pipeline._stabilize_frames).parameters["spatial_fill"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    p = inspect.signature(apply_pipeline.apply_motion).parameters["spatial_fill"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False

    context = hm._normalize_video_input(synth_frames(3, 16, 24, seed=1))
    for estimator in ("flow", "classic"):
        with pytest.raises(ValueError, match="spatial_fill='on'"):
            flow_pipeline._stabilize_frames(context, "crop_and_pad", "similarity", False, 0.9, 0.8, 0.6, (0, 0, 0), 16.0,
                                            estimator=estimator, spatial_fill="on")
    with pytest.raises(ValueError, match="spatial_fill=1 "):
        apply_pipeline.apply_motion(context, {}, (0, 0, 0), spatial_fill=1)
    with pytest.raises(ValueError, match="motion_blur=0.3"):      # before the meta is looked at, before any GPU work
        apply_pipeline.apply_motion(context, {}, (0, 0, 0), motion_blur=0.3, spatial_fill=True)


def test_meta_block_from_counts(pkg):
    from vstab_amd import spatial_fill

    holes = [0, 120, 96, 0, 48]
    filled = [0, 120, 0, 0, 48]       # frame 2: all hole, nothing written
    block = spatial_fill.fill_meta(holes, filled, (12, 8))
    pixels = np.float32(96)
    fractions = (np.array(filled, np.float32) / pixels).astype(np.float64)
    assert block == {"method": "push_pull", "version": 1, "filled_fraction_mean": float(fractions.mean()),
                     "filled_fraction_max": float(fractions.max()), "frames_filled": 2, "frames_without_source": 1}
    assert list(block) == ["method", "version", "filled_fraction_mean", "filled_fraction_max", "frames_filled",
                           "frames_without_source"]
    assert block["filled_fraction_max"] == 1.25                      # counts are taken as given
    with pytest.raises(ValueError, match="hole counts"):
        spatial_fill.fill_meta([1, 2], [1], (4, 4))


def test_node_is_listed_by_the_new_extension_only(pkg):
    from vstab_amd import nodes

    node = nodes.VideoStabilizerPaddingFill
    assert len(nodes.NODE_CLASSES) == 6 and node not in nodes.NODE_CLASSES
    assert issubclass(nodes.VideoStabilizerAmdFillExtension, nodes.VideoStabilizerAmdMeshApplyExtension)
    before = asyncio.run(nodes.VideoStabilizerAmdMeshApplyExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdFillExtension().get_node_list())
    assert node not in before and listed == before + [node]
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_padding_fill" and schema.display_name == "Video Stabilizer Padding Fill"
    assert [s.id for s in schema.inputs] == ["frames", "padding_mask"]
    assert [s.id for s in schema.outputs] == ["frames", "meta"]


def test_node_refuses_mismatched_sockets_by_name(pkg):
    """Shape and dtype are checked in front of any GPU work."""
    import torch

    from vstab_amd import nodes

    frames = torch.zeros((3, 8, 10, 3))
    for mask in (torch.zeros((3, 10, 8)), torch.zeros((2, 8, 10)), torch.zeros((8, 10)), torch.zeros((3, 8, 10, 2))):
        with pytest.raises(ValueError, match="'padding_mask' of shape"):
            nodes.VideoStabilizerPaddingFill.execute(frames, mask)
    with pytest.raises(ValueError, match="'padding_mask' must be a floating-point MASK, got torch.uint8"):
        nodes.VideoStabilizerPaddingFill.execute(frames, torch.zeros((3, 8, 10), dtype=torch.uint8))
    with pytest.raises(ValueError, match="'padding_mask' must be a floating-point MASK tensor, got list"):
        nodes.VideoStabilizerPaddingFill.execute(frames, [[0.0]])


def test_header_declares_what_native_binds_and_the_library_exports(pkg):
    from vstab_amd import native

    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "vstab.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+vstab_spatial_fill_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "include/vstab.h does not declare vstab_spatial_fill_batch"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = native._SIGNATURES["vstab_spatial_fill_batch"]
    assert res is C.c_int and len(params) == len(args) == 9
    for ptxt, a in zip(params, args):
        assert a is (C.c_void_p if "*" in ptxt else C.c_int), ptxt
    assert "vstab_spatial_fill_batch" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load_library(), "vstab_spatial_fill_batch")
    assert hasattr(native.Context, "spatial_fill_batch")
    assert "vstab_fill.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
