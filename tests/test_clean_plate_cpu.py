"""CPU: the clean plate's rules on their NumPy restatement (tests/clean_plate_restatement.py, which the GPU tests hold the
kernels to in bits), and the host side: sample table, keyword checks and their order, ABI, node, documents."""

import asyncio
import ctypes as C
import inspect
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import clean_plate_restatement as R

ROOT = Path(__file__).resolve().parents[1]
ARGS = ("crop_and_pad", "similarity", True, 1.0, 0.8, 0.6, (127, 127, 127), 16.0)      # a locked shot


class NoClip:                      # never touched: the checks come first
    frames = None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.0, -1.0, 0.5, 3.4e38], np.float32)


def drawn(seed, n, h, w, special=0.3, masked=0.4):
    """Frames with a share of special values and a mask with a share of 1, NaN, 0.5 and nextafter(0.5)."""
    rng = np.random.default_rng(seed)
    frames = rng.uniform(-1, 2, (n, h, w, 3)).astype(np.float32)
    pick = rng.uniform(size=frames.shape) < special
    frames[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
    frames[rng.uniform(size=frames.shape) < 0.2] = np.float32(0.25)      # ties
    mask = np.zeros((n, h, w), np.float32)
    levels = np.array([1.0, np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), 0.75, np.inf, -np.inf], np.float32)
    pick = rng.uniform(size=mask.shape) < masked
    mask[pick] = levels[rng.integers(0, len(levels), int(pick.sum()))]
    return frames, mask


# ---- the rules, on the restatement -----------------------------------------------------------------------------------------
def test_order_key_is_the_total_order_and_round_trips():
    ordered = np.array([-np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 0.5, 1.0, 3.4e38, np.inf, np.nan], np.float32)
    keys = R.order_key(ordered).astype(np.int64)
    assert (np.diff(keys) > 0).all() and keys[-1] == 0xFFFFFFFF
    assert np.array_equal(_bits(R.unkey(R.order_key(ordered[:-1]))), _bits(ordered[:-1]))
    # every NaN pattern, the negative ones included, is the largest key and comes back as the quiet NaN
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert (R.order_key(nans) == 0xFFFFFFFF).all() and (_bits(R.unkey(R.order_key(nans))) == 0x7FC00000).all()


@pytest.mark.parametrize("seed,n,rows", [(0, 1, [[0]]), (1, 2, [[0, 1]]), (2, 5, [[0, 1, 2, 3, 4]]), (3, 6, [[0, 2, 5, -1], [1, 3, 4, 5]]),
                                         (4, 9, [[0, 1, 2, 3, 4, 5, 6, 7, 8], [4, -1, -1, -1, -1, -1, -1, -1, -1]])])
def test_restatement_equals_np_sort_on_the_valid_keys(seed, n, rows):
    frames, mask = drawn(seed, n, 5, 7)
    for m in (mask, None):
        plate, count = R.plate_median(frames, m, np.array(rows))
        for s, row in enumerate(rows):
            want, want_count = R.plate_median_literal(frames, m, row)
            assert np.array_equal(_bits(plate[s]), _bits(want)) and np.array_equal(count[s], want_count)
    assert (R.plate_median(frames, mask, np.array(rows))[1] == 0).any() or n > 4      # (short rows do meet pixels nobody saw)


def test_lower_median_zero_count_and_mask_convention():
    frames = np.arange(4, dtype=np.float32).reshape(4, 1, 1, 1).repeat(3, axis=3) + np.array([0, 10, 20], np.float32)
    plate, count = R.plate_median(frames, None, np.array([[0, 1, 2, 3]]))
    assert plate[0, 0, 0].tolist() == [1.0, 11.0, 21.0] and count[0, 0, 0] == 4              # rank (4 - 1) // 2 = 1: the lower one
    for level, valid in ((0.5, True), (np.nextafter(np.float32(0.5), np.float32(1)), False), (np.nan, False), (-np.inf, True), (1.0, False)):
        mask = np.zeros((4, 1, 1), np.float32)
        mask[0] = level
        plate, count = R.plate_median(frames, mask, np.array([[0, 1, 2, 3]]))
        assert count[0, 0, 0] == (4 if valid else 3) and plate[0, 0, 0, 0] == (1.0 if valid else 2.0)
    plate, count = R.plate_median(frames, np.ones((4, 1, 1), np.float32), np.array([[0, 1, 2, 3]]))
    assert count[0, 0, 0] == 0 and _bits(plate).tolist() == [[[[0, 0, 0]]]]
    # NaN values: fewer than half leave the median finite, more than half make it the quiet NaN
    frames[3] = np.nan
    assert R.plate_median(frames, None, np.array([[0, 1, 2, 3]]))[0][0, 0, 0, 0] == 1.0
    frames[1:] = np.nan
    assert _bits(R.plate_median(frames, None, np.array([[0, 1, 2, 3]]))[0])[0, 0, 0, 0] == 0x7FC00000
    # -0.0 sorts below +0.0 and keeps its bits
    z = np.array([0.0, -0.0, -0.0], np.float32).reshape(3, 1, 1, 1).repeat(3, axis=3)
    assert _bits(R.plate_median(z, None, np.array([[0, 1, 2]]))[0])[0, 0, 0, 0] == 0x80000000


def test_static_background_and_a_disc_moving_by_whole_pixels():
    """No tolerance anywhere: wherever the disc covers fewer than half of the valid samples the plate IS the background, and
    the matte IS the disc's footprint."""
    n, h, w = 9, 24, 40
    yy, xx = np.mgrid[0:h, 0:w]
    background = np.stack([(xx * 3 + yy) % 17, (xx + yy * 5) % 13, (xx * 7 + yy * 2) % 11], axis=-1).astype(np.float32)
    frames = np.repeat(background[None], n, axis=0)
    disc = np.stack([(xx - (6 + 3 * k)) ** 2 + (yy - 12) ** 2 <= 25 for k in range(n)])
    frames[disc] = np.float32(100.0)
    mask = np.zeros((n, h, w), np.float32)
    for k in range(n):
        mask[k, :, :k] = 1.0            # a border that grows: the valid counts differ over the picture
    valid = mask <= 0.5
    plate, count = R.plate_median(frames, mask, R.sample_table(None, n))
    assert np.array_equal(count[0], valid.sum(axis=0))
    clean = (disc & valid).sum(axis=0) * 2 < valid.sum(axis=0)
    assert clean.sum() > 0.9 * h * w and (~clean).sum() > 0          # the disc's path overlaps itself: some pixels see it half the time
    assert np.array_equal(_bits(plate[0])[clean], _bits(background)[clean])
    matte, matte_count = R.plate_matte(frames, mask, plate, count, None, 0.5, 1)
    assert np.array_equal(matte[:, clean], (disc & valid)[:, clean].astype(np.float32))
    assert matte_count.tolist() == matte.sum(axis=(1, 2)).astype(np.uint32).tolist()
    # the fill: padded pixels become the background, their mask 0, everything else keeps its bits
    filled, new_mask, counts = R.plate_fill(frames, mask, plate, count, None, 1)
    padded = ~valid & (count[0] >= 1)[None]
    assert counts.tolist() == padded.sum(axis=(1, 2)).tolist() and (new_mask[padded] == 0).all()
    assert np.array_equal(_bits(filled)[padded & clean[None]], np.broadcast_to(_bits(background), frames.shape)[padded & clean[None]])
    assert np.array_equal(_bits(filled)[~padded], _bits(frames)[~padded]) and np.array_equal(_bits(new_mask)[~padded], _bits(mask)[~padded])
    # min_count above every count: nothing changes
    same, same_mask, zero = R.plate_fill(frames, mask, plate, count, None, 10)
    assert np.array_equal(_bits(same), _bits(frames)) and np.array_equal(_bits(same_mask), _bits(mask)) and not zero.any()


def test_matte_rule_at_the_threshold_and_with_nan():
    plate = np.zeros((1, 1, 6, 3), np.float32)
    count = np.full((1, 1, 6), 3, np.int32)
    count[0, 0, 5] = 2
    frames = np.zeros((1, 1, 6, 3), np.float32)
    frames[0, 0, :, 1] = [0.25, np.nextafter(np.float32(0.25), np.float32(1)), -0.25, np.nan, 0.0, 9.0]
    matte, total = R.plate_matte(frames, None, plate, count, None, 0.25, 3)
    assert matte[0, 0].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0] and total.tolist() == [2]       # at the threshold: not matte
    assert R.plate_matte(frames, None, plate, count, None, 0.0, 3)[0][0, 0].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    plate[0, 0, 4, 2] = np.nan                                                                     # a NaN plate differs too
    assert R.plate_matte(frames, None, plate, count, None, 0.25, 3)[0][0, 0, 4] == 1.0
    mask = np.zeros((1, 1, 6), np.float32)
    mask[0, 0, 1], mask[0, 0, 3] = np.nan, 0.75                                                    # not own: no matte
    assert R.plate_matte(frames, mask, plate, count, None, 0.25, 3)[0][0, 0].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


# ---- host side ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments,total", [(None, 1), (None, 2), (None, 256), (None, 257), (None, 1000), ([(0, 3), (3, 300), (300, 301)], 301),
                                            ([(0, 700), (700, 710)], 710)])
def test_sample_table(pkg, segments, total):
    from vstab_amd import clean_plate

    table = clean_plate.sample_table(segments, total)
    assert table.dtype == np.int32 and np.array_equal(table, R.sample_table(segments, total))
    segs = [(0, total)] if segments is None else segments
    assert table.shape == (len(segs), min(256, max(e - s for s, e in segs)))
    for row, (s, e) in zip(table, segs):
        used = row[row >= 0]
        assert len(used) == min(e - s, 256) and (row[len(used):] == -1).all()
        assert (np.diff(used) > 0).all() and used[0] >= s and used[-1] < e
        if e - s <= 256:
            assert used.tolist() == list(range(s, e))                 # every frame of a short shot
        else:
            # the frame under the centre (k + 1/2) * L / 256 of each of 256 equal strata, in exact rationals
            assert used.tolist() == [s + int(Fraction(2 * k + 1, 2) * Fraction(e - s, 256)) for k in range(256)]


def test_check_request_names_the_value(pkg):
    from vstab_amd import clean_plate

    assert clean_plate.check_request(None) is None and clean_plate.check_request(False) is None
    assert clean_plate.check_request(True) == 1 and clean_plate.check_request(1) == 1 and clean_plate.check_request(256) == 256
    assert clean_plate.check_request(np.int64(7)) == 7
    for bad in (0, 257, -1, 2.0, "yes", [1], np.bool_(True)):
        with pytest.raises(ValueError, match=re.escape(f"plate_fill={bad!r} is not None, False, True or an integer in 1..256")):
            clean_plate.check_request(bad)
    assert (clean_plate.SAMPLES_MAX, clean_plate.DEFAULT_MATTE_THRESHOLD, clean_plate.DEFAULT_MATTE_MIN_COUNT) == (256, 0.1, 3)
    assert "Choices, not calibrations" in inspect.getsource(clean_plate)


def _call(pkg, *args, **keywords):
    from vstab_amd import flow_pipeline

    return flow_pipeline._stabilize_frames(NoClip(), *args, **keywords)


def test_every_refusal_says_why_before_any_gpu_work(pkg):
    """NoClip has no frames: reaching the clip would be a TypeError, so each of these is raised by the checks alone."""
    framing, mode, lock, strength, *rest = ARGS
    with pytest.raises(ValueError, match=r"plate_fill='on' is not None, False, True or an integer in 1\.\.256"):
        _call(pkg, *ARGS, plate_fill="on")
    for lock_, strength_ in ((False, 1.0), (True, 0.9), (False, 0.5), (0, 1.0)):
        with pytest.raises(ValueError, match="plate_fill needs camera_lock=True and strength=1 .* a median over frames that are not registered is a smear"):
            _call(pkg, framing, mode, lock_, strength_, *rest, plate_fill=True)
    with pytest.raises(ValueError, match="plate_fill is not supported with dynamic_zoom: the per-frame zoom unregisters"):
        _call(pkg, *ARGS, plate_fill=True, dynamic_zoom=True)
    with pytest.raises(ValueError, match="plate_fill is not supported with a horizon_level window: the per-frame turn unregisters"):
        _call(pkg, *ARGS, plate_fill=2, horizon_level=1.5)
    with pytest.raises(ValueError, match="plate_fill is not supported with estimator 'subject': .* the plate would be of the subject"):
        _call(pkg, *ARGS, plate_fill=True, estimator="subject", subject_mask=np.zeros((2, 4, 4), np.float32))
    # allowed: one roll offset per shot, and a strength above 1 (the plan clips it to 1); these get as far as the clip
    for keywords in (dict(horizon_level=True), dict(), dict(temporal_fill=2), dict(spatial_fill=True), dict(scene_cuts=[3])):
        with pytest.raises(TypeError):
            _call(pkg, *ARGS, plate_fill=True, **keywords)
    with pytest.raises(TypeError):
        _call(pkg, framing, mode, True, 1.5, *rest, plate_fill=True)
    # off: the request is today's
    from vstab_amd import flow_pipeline as fp

    params = inspect.signature(fp._stabilize_frames).parameters
    assert params["plate_fill"].default is None and params["plate_fill"].kind is inspect.Parameter.KEYWORD_ONLY
    kw = {name: p.default for name, p in params.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    kw.update(camera_lock=False, strength=0.5)
    today = fp.check_flow_request("crop_and_pad", "similarity", "flow", {k: v for k, v in kw.items() if k != "plate_fill"})
    for off in (None, False):
        got = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, plate_fill=off))
        assert got == today and got.plate is None and got.needs_host_plan == today.needs_host_plan
    on = fp.check_flow_request("crop_and_pad", "similarity", "flow", dict(kw, plate_fill=True, camera_lock=True, strength=1.0))
    assert on.plate == 1 and not on.needs_host_plan and on.kept_by_products == ()
    assert "plate_fill" in fp._stabilize_frames.__doc__


# one doubly-wrong call per neighbour feature: the neighbour's message still wins, whatever is wrong with plate_fill
NEIGHBOURS = [
    (dict(mask_grow=999), "mask_grow=999 is not None or an integer in -64..64"),
    (dict(dynamic_zoom=99.0), "dynamic_zoom=99.0: expected None, True or a finite window in seconds in (0, 60]"),
    (dict(spatial_fill="yes"), "spatial_fill='yes' is not a bool (True fills the leftover padding, False leaves it)"),
    (dict(stability_report=2), "stability_report=2 is not a bool (True adds the ITF of the inputs and of the outputs to the meta, False leaves it out)"),
    (dict(scene_cuts="sometimes"), "scene_cuts='sometimes': expected None, 'auto' or a sequence of frame indices"),
    (dict(mesh_warp=(1, 1)), "mesh_warp=(1, 1): cols and rows must lie in [2, 64]"),
    (dict(estimator="nope"), "Unknown estimator 'nope'; expected 'flow' or 'classic'."),
    (dict(estimator="subject"), "estimator='subject' needs subject_mask: a float mask [N,H,W] of the subject, one per frame."),
    (dict(temporal_fill=99), "temporal_fill=99 outside [0, 32]"),
    (dict(fill_feather=8), "fill_feather=8 / fill_exposure=False need temporal_fill > 0: they change how the temporal fill writes its pixels"),
    (dict(sharpness_transfer=99), "sharpness_transfer=99 is not 0, None, False or an integer in 1..16"),
    (dict(estimation_mask=np.zeros((4, 4), np.float32), mask_margin=99), "mask_margin=99 outside [0, 64] (working pixels)"),
    (dict(rolling_shutter=7.0), "rolling_shutter=7.0: expected None, 0, 'auto' or a finite readout in [-1, 1] (a fraction of the frame interval; negative: bottom to top)"),
    (dict(drift_correction=1), None),
    (dict(rolling_refit=True), None),
    (dict(deflicker=99.0), "deflicker=99.0: expected None, False, True or a finite window in seconds in (0, 60]"),
    (dict(horizon_level=99.0), "horizon_level=99.0: expected None, True or a finite window in seconds in (0, 60]"),
]


@pytest.mark.parametrize("case", range(len(NEIGHBOURS)))
@pytest.mark.parametrize("plate_fill", ["on", True])
def test_the_new_checks_come_last(pkg, monkeypatch, case, plate_fill):
    """plate_fill='on' is malformed; plate_fill=True on an unlocked call is refused by check_pipeline.  Either way the
    neighbour's own message is the one raised, and it is the message the call raises without plate_fill."""
    monkeypatch.delenv("VSTAB_FLOW_BACKEND", raising=False)
    keywords, message = NEIGHBOURS[case]
    unlocked = ("crop_and_pad", "similarity", False, 0.5, 0.8, 0.6, (127, 127, 127), 16.0)
    with pytest.raises(ValueError) as without:
        _call(pkg, *unlocked, **keywords)
    with pytest.raises(ValueError) as caught:
        _call(pkg, *unlocked, plate_fill=plate_fill, **keywords)
    assert str(caught.value) == str(without.value) and "plate_fill" not in str(caught.value)
    assert message is None or str(caught.value) == message


def test_sharded_path_refuses_the_keyword(pkg):
    from vstab_amd import distributed

    args = (None, None, 12, "crop_and_pad", "similarity", True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)
    for value in (True, 3):
        with pytest.raises(ValueError, match=re.escape(f"stabilize_sharded does not support plate_fill={value!r}: the clean plate is not sharded "
                                                       "(the median runs over every frame of a shot, and a rank holds a slice of it)")):
            distributed.stabilize_sharded(*args, plate_fill=value)
    with pytest.raises(ValueError, match="does not support horizon_level"):      # behind the existing refusals
        distributed.stabilize_sharded(*args, plate_fill=True, horizon_level=True)


def test_meta_block_layout(pkg):
    from vstab_amd import clean_plate

    table = R.sample_table([(0, 2), (2, 5)], 5)
    mask_after = np.zeros((5, 2, 4), np.float32)
    mask_after[1, 0, :3] = 1.0
    mask_after[4, 1, 0] = np.nan
    count = np.array([[[0, 1, 2, 2], [2, 2, 2, 2]], [[3, 3, 3, 3], [3, 3, 1, 0]]], np.int32)
    filled = [0, 2, 0, 8, 1]
    left = (~R.valid_of(mask_after, mask_after.shape)).sum(axis=(1, 2))
    block = clean_plate.meta_block(2, table, filled, left, (count < 2).sum(axis=(1, 2)), (2, 4))
    assert list(block) == ["version", "min_count", "shots", "samples_per_shot", "filled_fraction_mean", "filled_fraction_max",
                           "padding_fraction_mean_after", "padding_fraction_max_after", "frames_with_padding_after", "unseen_fraction"]
    assert block == R.meta_block(2, table, filled, mask_after, count)
    assert block["samples_per_shot"] == [2, 3] and block["frames_with_padding_after"] == 2 and block["unseen_fraction"] == [0.25, 0.25]
    assert block["filled_fraction_max"] == 1.0 and block["padding_fraction_max_after"] == 0.375


# ---- ABI, node, documents ------------------------------------------------------------------------------------------------------
ENTRIES = {"vstab_plate_median_batch": ("plate_median_batch", 11), "vstab_plate_fill_batch": ("plate_fill_batch", 12),
           "vstab_plate_matte_batch": ("plate_matte_batch", 14)}


def test_header_declares_what_native_binds_and_the_library_exports(pkg):
    from vstab_amd import native

    header = (ROOT / "include" / "vstab.h").read_text()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    raw = C.CDLL(str(native.LIB_PATH))
    raw.vstab_last_error.restype = C.c_char_p
    for name, (method, count) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"include/vstab.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = native._SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == count
        for ptxt, a in zip(params, args):
            assert a is (C.c_void_p if "*" in ptxt else C.c_float if ptxt.startswith("float") else C.c_int), ptxt
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load_library(), name) and hasattr(native.Context, method)
        # the argument checks come in front of any GPU work, under the function's name
        fn = getattr(raw, name)
        fn.argtypes, fn.restype = args, C.c_int
        assert fn(*[None if a is C.c_void_p else 1 for a in args]) != 0
        assert raw.vstab_last_error().decode().startswith(f"{name}: NULL context")
    assert "vstab_plate.hip" in (ROOT / "comfyui-video-stabilizer_amd" / "csrc" / "Makefile").read_text()
    assert f"#define VSTAB_PLATE_SAMPLES_MAX {native.PLATE_SAMPLES_MAX}\n" in header
    assert f"#define VSTAB_PLATE_REGISTER_MAX {native.PLATE_REGISTER_MAX}\n" in header
    assert native.PLATE_REGISTER_MAX in native.PLATE_PATH_STEPS and max(native.PLATE_PATH_STEPS) < native.PLATE_SAMPLES_MAX == 256


def test_node_is_listed_by_the_new_extension_only(pkg):
    import vstab_amd
    from vstab_amd import nodes

    node = nodes.VideoStabilizerCleanPlate
    assert len(nodes.NODE_CLASSES) == 6 and node not in nodes.NODE_CLASSES
    assert issubclass(nodes.VideoStabilizerAmdPlateExtension, nodes.VideoStabilizerAmdLevelExtension)
    before = asyncio.run(nodes.VideoStabilizerAmdLevelExtension().get_node_list())
    listed = asyncio.run(nodes.VideoStabilizerAmdPlateExtension().get_node_list())
    assert node not in before and listed == before + [node]
    entry = asyncio.run(vstab_amd.comfy_entrypoint())
    assert node not in asyncio.run(entry.get_node_list())             # the entry point is unchanged
    schema = node.define_schema()
    assert schema.node_id == "video_stabilizer_clean_plate" and schema.display_name == "Video Stabilizer Clean Plate"
    ids = [s.id for s in schema.inputs]
    assert ids == ["frames", "padding_mask", "fill", "min_count", "matte_threshold", "matte_min_count"]
    assert ids == list(inspect.signature(node.execute).parameters)
    assert [bool(s.options.get("optional")) for s in schema.inputs] == [False, True, False, False, False, False]
    defaults = {s.id: s.options.get("default") for s in schema.inputs[2:]}
    assert defaults == {"fill": True, "min_count": 1, "matte_threshold": 0.1, "matte_min_count": 3}
    params = inspect.signature(node.execute).parameters
    assert {k: params[k].default for k in defaults} == defaults and params["padding_mask"].default is None
    assert [s.id for s in schema.outputs] == ["plate", "frames", "padding_mask", "matte", "meta"]
    assert [s.kind for s in schema.outputs] == ["Image", "Image", "Mask", "Mask", "String"]


def test_node_refuses_bad_sockets_before_any_gpu_work(pkg):
    import torch

    from vstab_amd import nodes

    frames = torch.zeros((3, 8, 10, 3))
    for mask in (torch.zeros((3, 10, 8)), torch.zeros((2, 8, 10)), torch.zeros((8, 10))):
        with pytest.raises(ValueError, match="'padding_mask' of shape"):
            nodes.VideoStabilizerCleanPlate.execute(frames, mask)
    with pytest.raises(ValueError, match="'padding_mask' must be a floating-point MASK, got torch.uint8"):
        nodes.VideoStabilizerCleanPlate.execute(frames, torch.zeros((3, 8, 10), dtype=torch.uint8))
    for keywords, text in ((dict(min_count=0), "min_count=0"), (dict(matte_min_count=257), "matte_min_count=257"),
                           (dict(matte_threshold=-0.1), "matte_threshold=-0.1"), (dict(fill=1), "fill=1")):
        with pytest.raises(ValueError, match=re.escape("clean plate: " + text)):
            nodes.VideoStabilizerCleanPlate.execute(frames, None, **keywords)


def test_documents_name_the_entries_and_the_extension():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        for name in ENTRIES:
            assert name in text, f"{doc} does not mention {name}"
    for doc in ("README.md", "INTEGRATION.md"):
        text = (ROOT / doc).read_text()
        assert "VideoStabilizerAmdPlateExtension" in text and "Video Stabilizer Clean Plate" in text
    assert "plate_fill" in (ROOT / "README.md").read_text()
    assert "clean_plate_report.py" in (ROOT / "tools" / "README.md").read_text()
