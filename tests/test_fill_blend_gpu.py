"""GPU: vstab_fill_gain_sums and vstab_temporal_fill_blend_batch (csrc/vstab_neighbour.hip: fill_gain_sums_kernel,
temporal_fill_blend_kernel) and the `fill_feather` / `fill_exposure` keywords / the blended node.

Every comparison of pixels, masks, indices, counts and sums is exact and over all pixels: against the NumPy restatement
(tests/fill_blend_restatement.py, refereed on the CPU in tests/test_fill_blend_cpu.py), against vstab_temporal_fill_batch
where the two must agree, and, without any restatement, against a texture whose windows at integer offsets, times known
gains, are the frames.
"""

import json

import numpy as np
import pytest

from tests import fill_blend_restatement as B
from tests.test_temporal_fill_gpu import SHAPES, _drawn_case
from tests.util import shake_path, similarity

pytestmark = pytest.mark.gpu

INTERPS = ["bilinear", "bicubic"]
FEATHERS = [1, 7, 64]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _blend_case(shape, seed=None):
    """_drawn_case of tests/test_temporal_fill_gpu.py (soft mask values, -1 slots, singular and far-outside candidates) plus
    one own matrix per frame whose frame border crosses the canvas (a shrinking similarity about the centre; the last frame
    of a three-frame case gets a perspective one, the first a singular one: no feather there) and gains in [0.5, 2]."""
    n, clip, sh, sw, dh, dw, K = shape
    src, dst, mask, mats, cand = _drawn_case(n, clip, sh, sw, dh, dw, K, seed=dh * 7 + K if seed is None else seed)
    rng = np.random.default_rng(1000 + dh + K)
    own = np.zeros((n, 3, 3), np.float32)
    for f in range(n):
        m = similarity((dw - sw) / 2 + rng.uniform(-0.1, 0.1) * dw, (dh - sh) / 2 + rng.uniform(-0.1, 0.1) * dh,
                       rng.uniform(-0.15, 0.15), rng.uniform(0.8, 0.95), sw / 2, sh / 2)
        if n == 3 and f == 2:
            m[2, :2] = rng.uniform(-4e-4, 4e-4, 2)
        if n == 3 and f == 0:
            m[1] = m[0] * 2.0
        own[f] = m
    gains = rng.uniform(0.5, 2.0, (n, K, 3)).astype(np.float32)
    return src, dst, mask, mats, cand, own, gains


def _run_blend(ctx, src, mats, cand, own, gains, feather, dst, mask, interp, first=0, subpix=None):
    import torch

    d = torch.from_numpy(dst).to(ctx.device).contiguous()
    m = torch.from_numpy(mask).to(ctx.device).contiguous()
    ff, fc, pc, bc = ctx.temporal_fill_blend_batch(torch.from_numpy(src).to(ctx.device), mats, cand, own, gains, d, m,
                                                   feather_px=feather, first=first, interp=interp, subpix=subpix,
                                                   want_filled_from=True)
    i64 = lambda t: t.cpu().numpy().astype(np.int64)   # noqa: E731
    return d.cpu().numpy(), m.cpu().numpy(), ff.cpu().numpy(), i64(fc), i64(bc), i64(pc)


def _run_sums(ctx, src, mats, cand, own, dst, interp):
    import torch

    sums = ctx.fill_gain_sums(torch.from_numpy(src).to(ctx.device), mats, cand, own,
                              torch.from_numpy(dst).to(ctx.device).contiguous(), interp=interp)
    return sums.cpu().numpy().astype(np.uint64)


def _assert_same(got, want):
    d, m, ff, fc, bc, pc = got
    rd, rm, rff, rfc, rbc, rpc = want
    assert np.array_equal(ff, rff), f"filled_from differs at {int((ff != rff).sum())} pixels"
    assert np.array_equal(_bits(m), _bits(rm)), f"mask differs at {int((_bits(m) != _bits(rm)).sum())} pixels"
    assert np.array_equal(_bits(d), _bits(rd)), f"dst differs at {int((_bits(d) != _bits(rd)).any(axis=-1).sum())} pixels"
    assert np.array_equal(fc, rfc) and np.array_equal(bc, rbc) and np.array_equal(pc, rpc), (fc, rfc, bc, rbc, pc, rpc)


@pytest.mark.parametrize("feather", FEATHERS)
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_kernel_matches_restatement(ctx, oracle, shape, interp, feather):
    src, dst, mask, mats, cand, own, gains = _blend_case(shape)
    got = _run_blend(ctx, src, mats, cand, own, gains, feather, dst, mask, interp)
    want = B.temporal_fill_blend(src, mats, cand, own, gains, feather, dst, mask, interp)
    _assert_same(got, want)
    # the case shows every kind of pixel: filled, cross-faded (0 < w < 1), fringe (w == 0, replaced), untouched
    n, sh, sw = mask.shape[0], src.shape[1], src.shape[2]
    kinds = np.zeros(4, np.int64)
    for f in range(n):
        if not B.usable_matrix(own[f]):
            continue
        X, Y = B.q5_coordinates(own[f], (mask.shape[2], mask.shape[1]))
        w = B.feather_weight(B.feather_distance(X, Y, (sw, sh), interp), feather)
        own_px, touched = mask[f] != 1.0, want[2][f] >= 0
        kinds += [int((~own_px & touched).sum()), int((own_px & touched & (w > 0) & (w < 1)).sum()),
                  int((own_px & touched & (w == 0)).sum()), int((~touched).sum())]
    assert (kinds > 0).all(), kinds
    # untouched guarantee: a pixel with filled_from == -1 keeps its input bits, and an own pixel always keeps its mask
    keep = got[2] < 0
    assert np.array_equal(_bits(got[0])[keep], _bits(dst)[keep]) and np.array_equal(_bits(got[1])[keep], _bits(mask)[keep])
    assert np.array_equal(_bits(got[1])[mask != 1.0], _bits(mask)[mask != 1.0])


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gain_sums_match_restatement(ctx, oracle, shape, interp):
    src, dst, _, mats, cand, own, _ = _blend_case(shape)
    got = _run_sums(ctx, src, mats, cand, own, dst, interp)
    want = B.gain_sums(src, mats, cand, own, dst, interp)
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=-1))[:5]
    assert (want[..., 0] > 0).any() and (want[..., 0] == 0).any()
    if shape[0] == 3:
        assert not want[0].any()                          # the frame with the singular own matrix counts nothing


def test_gain_sums_without_a_lattice_pixel_are_zero(ctx):
    rng = np.random.default_rng(5)
    src = rng.uniform(0, 1, (2, 3, 3, 3)).astype(np.float32)
    eye = np.eye(3, dtype=np.float32)
    got = _run_sums(ctx, src, np.tile(eye, (2, 2, 1, 1)), np.array([[1, 0], [0, 1]], np.int32), np.tile(eye, (2, 1, 1)),
                    rng.uniform(0, 1, (2, 3, 3, 3)).astype(np.float32), "bilinear")
    assert got.shape == (2, 2, 7) and not got.any()


@pytest.mark.parametrize("interp", INTERPS)
def test_gain_sums_on_nan_inf_and_out_of_range_values(ctx, oracle, interp):
    src, dst, _, mats, cand, own, _ = _blend_case(SHAPES[2])
    rng = np.random.default_rng(77)
    nasty = np.array([np.nan, np.inf, -np.inf, -0.5, 1.5, 3.0, 0.0, -0.0, 1.0], np.float32)
    for a in (src, dst):
        hit = rng.uniform(0, 1, a.shape) < 0.05
        a[hit] = rng.choice(nasty, size=int(hit.sum()))
    for f in range(dst.shape[0]):                          # and on lattice pixels for certain
        dst[f, 4::8, 4::16] = nasty[f % len(nasty)]
    got = _run_sums(ctx, src, mats, cand, own, dst, interp)
    want = B.gain_sums(src, mats, cand, own, dst, interp)
    assert np.array_equal(got, want) and (want[..., 0] > 0).any()


@pytest.mark.parametrize("interp", INTERPS)
def test_no_feather_and_unit_gains_equal_the_plain_fill(ctx, interp):
    import torch

    for shape in SHAPES:
        src, dst, mask, mats, cand, own, _ = _blend_case(shape)
        got = _run_blend(ctx, src, mats, cand, own, np.ones(cand.shape + (3,), np.float32), 0, dst, mask, interp)
        d = torch.from_numpy(dst).to(ctx.device).contiguous()
        m = torch.from_numpy(mask).to(ctx.device).contiguous()
        ff, fc, pc = ctx.temporal_fill_batch(torch.from_numpy(src).to(ctx.device), mats, cand, d, m, interp=interp, subpix="q5",
                                             want_filled_from=True)
        assert np.array_equal(_bits(got[0]), _bits(d.cpu().numpy())) and np.array_equal(_bits(got[1]), _bits(m.cpu().numpy()))
        assert np.array_equal(got[2], ff.cpu().numpy())
        assert np.array_equal(got[3], fc.cpu().numpy()) and np.array_equal(got[5], pc.cpu().numpy()) and (got[4] == 0).all()


def test_all_interior_frame_keeps_every_byte(ctx):
    """The canvas lies 20 source px or more inside the frame, the feather is 16: w == 1 everywhere, nothing is padded."""
    rng = np.random.default_rng(12)
    src = rng.uniform(0, 1, (3, 80, 120, 3)).astype(np.float32)
    dst = rng.uniform(0, 1, (2, 40, 60, 3)).astype(np.float32)
    mask = np.zeros((2, 40, 60), np.float32)
    mask[0, 5, 5] = 0.5
    own = np.stack([similarity(-30.0, -20.0, 0.0, 1.0)] * 2).astype(np.float32)
    mats = np.stack([[similarity(-20.0, -10.0, 0.0, 1.0), similarity(-25.0, -15.0, 0.0, 1.0)]] * 2).astype(np.float32)
    cand = np.array([[1, 2], [0, 2]], np.int32)
    gains = np.full((2, 2, 3), 1.5, np.float32)
    d, m, ff, fc, bc, pc = _run_blend(ctx, src, mats, cand, own, gains, 16, dst, mask, "bilinear")
    assert np.array_equal(_bits(d), _bits(dst)) and np.array_equal(_bits(m), _bits(mask))
    assert (ff == -1).all() and (fc == 0).all() and (bc == 0).all() and (pc == 0).all()


def test_two_windows_equal_one_call(ctx):
    import torch

    n = 5
    src, dst, mask, mats, cand, own, gains = _blend_case((n, n, 50, 90, 50, 90, 4), seed=8)
    whole = _run_blend(ctx, src, mats, cand, own, gains, 7, dst, mask, "bilinear")
    whole_sums = _run_sums(ctx, src, mats, cand, own, dst, "bilinear")
    s = torch.from_numpy(src).to(ctx.device)
    d = torch.from_numpy(dst).to(ctx.device)
    m = torch.from_numpy(mask).to(ctx.device)
    parts, sums = [], []
    for a, b in ((0, 2), (2, n)):
        sums.append(ctx.fill_gain_sums(s, mats[a:b], cand[a:b], own[a:b], d[a:b], first=a))
        parts.append(ctx.temporal_fill_blend_batch(s, mats[a:b], cand[a:b], own[a:b], gains[a:b], d[a:b], m[a:b], feather_px=7,
                                                   first=a, want_filled_from=True))
    assert np.array_equal(torch.cat(sums).cpu().numpy().astype(np.uint64), whole_sums) and whole_sums[..., 0].any()
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(whole[0])) and np.array_equal(_bits(m.cpu().numpy()), _bits(whole[1]))
    for i, idx in ((0, 2), (1, 3), (2, 5), (3, 4)):       # filled_from, fill_count, pad_count, blend_count
        assert np.array_equal(torch.cat([p[i] for p in parts]).cpu().numpy(), whole[idx])


def test_exact_mode_and_bad_arguments_are_refused(ctx):
    import torch

    from vstab_amd import native

    src, dst, mask, mats, cand, own, gains = _blend_case((2, 3, 40, 70, 40, 70, 2), seed=4)
    with pytest.raises(native.VstabError, match="exact"):
        _run_blend(ctx, src, mats, cand, own, gains, 4, dst, mask, "bilinear", subpix="exact")
    with pytest.raises(native.VstabError, match="exact"):
        ctx.fill_gain_sums(torch.from_numpy(src).to(ctx.device), mats, cand, own, torch.from_numpy(dst).to(ctx.device), subpix="exact")
    for feather in (-1, 65):
        with pytest.raises(native.VstabError, match=f"feather_px={feather}"):
            _run_blend(ctx, src, mats, cand, own, gains, feather, dst, mask, "bilinear")
    bad = cand.copy()
    bad[0, 0] = 3                                            # clip has frames 0..2
    with pytest.raises(native.VstabError, match="cand_frame"):
        _run_blend(ctx, src, mats, bad, own, gains, 4, dst, mask, "bilinear")
    with pytest.raises(native.VstabError, match="cand_frame"):
        _run_sums(ctx, src, mats, bad, own, dst, "bilinear")
    with pytest.raises(native.VstabError, match="outside a clip"):
        _run_blend(ctx, src, mats, cand, own, gains, 4, dst, mask, "bilinear", first=2)
    with pytest.raises(native.VstabError, match="own_matrices"):
        _run_blend(ctx, src, mats, cand, own[:1], gains, 4, dst, mask, "bilinear")
    with pytest.raises(native.VstabError, match="gains"):
        _run_blend(ctx, src, mats, cand, own, gains[:, :1], 4, dst, mask, "bilinear")
    big = np.tile(mats, (1, 40, 1, 1))                       # K = 80
    with pytest.raises(native.VstabError, match="K=80"):
        _run_blend(ctx, src, big, np.tile(cand, (1, 40)), own, np.tile(gains, (1, 40, 1)), 4, dst, mask, "bilinear")


def test_known_answer_flicker_clip(ctx, pkg):
    """No restatement: the referee's clip (windows of one texture at integer offsets, frame j times a_j = 0.8 / 1.25) through
    the two GPU entries and gains_from_sums.  Every filled and every blended pixel is within 5e-4 of a_i * texture (the
    bound is derived in tests/test_fill_blend_cpu.py::test_referee_flicker_clip), where the plain fill is off by
    0.45 * 0.25 or more."""
    import torch

    from vstab_amd import temporal_fill as tf

    clip = B.flicker_clip()
    frames, truth, final, mats, cand = clip["frames"], clip["truth"], clip["final"], clip["matrices"], clip["cand_frame"]
    n, h, w = frames.shape[:3]
    src = torch.from_numpy(frames).to(ctx.device)
    dst0, mask0, _ = ctx.warp_batch(src, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True)
    sums = ctx.fill_gain_sums(src, mats, cand, final, dst0).cpu().numpy()
    assert (sums[..., 0][cand >= 0] >= tf.GAIN_MIN_COUNT).all() and (sums[..., 0][cand < 0] == 0).all()
    gains = tf.gains_from_sums(sums)
    before = mask0.cpu().numpy()
    for feather in (0, 16):
        dst, mask = dst0.clone(), mask0.clone()
        ff, fc, pc, bc = ctx.temporal_fill_blend_batch(src, mats, cand, final, gains, dst, mask, feather_px=feather,
                                                       want_filled_from=True)
        touched = ff.cpu().numpy() >= 0
        filled = touched & (before == 1.0)
        assert filled.sum() > 2000 and int(fc.sum()) == int(filled.sum()) and int(bc.sum()) == int((touched & ~filled).sum())
        assert (feather == 0) == (int(bc.sum()) == 0)
        err = np.abs(dst.cpu().numpy().astype(np.float64) - truth.astype(np.float64)).max(axis=-1)
        print(f"flicker clip on the GPU, feather {feather}: worst error {err[touched].max():.3e} over {int(touched.sum())} pixels")
        assert err[touched].max() <= B.FLICKER_TOL
    hard, hmask = dst0.clone(), mask0.clone()
    hf, _, _ = ctx.temporal_fill_batch(src, mats, cand, hard, hmask, want_filled_from=True)
    off = np.abs(hard.cpu().numpy().astype(np.float64) - truth.astype(np.float64)).min(axis=-1)
    assert off[hf.cpu().numpy() >= 0].min() >= 0.45 * 0.25 - 1e-6


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H, N = 160, 96, 12
PLAIN_KEYS = {"radius", "filled_fraction_mean", "filled_fraction_max", "padding_fraction_mean_after", "padding_fraction_max_after"}
BLEND_KEYS = PLAIN_KEYS | {"feather_px", "blended_fraction_mean", "blended_fraction_max", "exposure"}


def _stabilize(ctx, frames, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", False, 0.9, 0.8, 0.6,
                                (127, 127, 127), 16.0, ctx=ctx, keep_on_device=True, estimator="flow", **kw)


def test_end_to_end_keywords_and_node(pkg, ctx, oracle):
    import torch

    import bench
    from vstab_amd import nodes
    from vstab_amd import temporal_fill as tf

    radius, feather = 4, 8
    cam = shake_path(N, W, H, "similarity", seed=3, amp=6.0)   # up to +-3 x +-2 px per frame at this size
    a = torch.tensor([B.FLICKER_GAINS[j % 2] for j in range(N)], device="cuda", dtype=torch.float32)
    frames = (bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=cam) * 0.75 * a[:, None, None, None]).contiguous()
    off = _stabilize(ctx, frames, temporal_fill=0)
    plain = _stabilize(ctx, frames, temporal_fill=radius)
    on = _stabilize(ctx, frames, temporal_fill=radius, fill_feather=feather, fill_exposure=True)

    assert set(plain.meta["temporal_fill"]) == PLAIN_KEYS                  # temporal_fill alone: today's five keys
    meta_on = dict(on.meta)
    block = meta_on.pop("temporal_fill")
    assert json.dumps(meta_on, sort_keys=True) == json.dumps(off.meta, sort_keys=True)
    assert set(block) == BLEND_KEYS and set(block["exposure"]) == {"matched", "gain_min", "gain_max", "candidates_without_overlap"}

    # the restatement applied to the temporal_fill=0 output, from that run's own meta JSON
    meta = json.loads(json.dumps(off.meta))
    final = np.array([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)
    trans = np.array([e["matrix"] for e in meta["estimated_motion"]["per_transition"]], np.float32)
    conf = np.array([e["confidence"] for e in meta["estimated_motion"]["per_transition"]], np.float64)
    mats, cand = tf.fill_candidates(final, trans, conf, radius)
    src = frames.cpu().numpy()
    d0, m0 = off.frames.cpu().numpy(), off.masks.cpu().numpy()[..., 0]
    sums = B.gain_sums(src, mats, cand, final, d0)
    gains = B.gains_from_sums(sums)
    rd, rm, _, rfc, rbc, rpc = B.temporal_fill_blend(src, mats, cand, final, gains, feather, d0, m0)
    assert rfc.sum() > 0 and rbc.sum() > 0, "the clip has no padding that a neighbour covers: the test would show nothing"
    assert np.array_equal(_bits(on.frames.cpu().numpy()), _bits(rd))
    assert np.array_equal(_bits(on.masks.cpu().numpy()[..., 0]), _bits(rm))

    pixels = np.float32(d0.shape[1] * d0.shape[2])
    frac = lambda c: (c.astype(np.float32) / pixels).astype(np.float64)   # noqa: E731
    used = (cand >= 0) & (sums[..., 0] >= B.GAIN_MIN_COUNT)
    assert used.any()
    assert block == {"radius": radius,
                     "filled_fraction_mean": float(np.mean(frac(rfc))), "filled_fraction_max": float(np.max(frac(rfc))),
                     "padding_fraction_mean_after": float(np.mean(frac(rpc))), "padding_fraction_max_after": float(np.max(frac(rpc))),
                     "feather_px": feather,
                     "blended_fraction_mean": float(np.mean(frac(rbc))), "blended_fraction_max": float(np.max(frac(rbc))),
                     "exposure": {"matched": True, "gain_min": float(gains[used].min()), "gain_max": float(gains[used].max()),
                                  "candidates_without_overlap": int(((cand >= 0) & ~used).sum())}}
    assert block["exposure"]["gain_min"] < 0.7 and block["exposure"]["gain_max"] > 1.4    # the flicker was seen

    # the node, from the meta JSON alone, gives the keywords' bits and leaves its inputs alone
    out = nodes.VideoStabilizerTemporalFillBlend.execute(frames, off.frames, off.masks, meta, radius, "bilinear", feather, True)
    node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(rd)) and np.array_equal(_bits(node_mask.cpu().numpy()), _bits(rm))
    assert node_meta["temporal_fill"] == {**block, "interpolation": "bilinear"}
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(d0))

    # each option works without the other
    only_feather = _stabilize(ctx, frames, temporal_fill=radius, fill_feather=feather).meta["temporal_fill"]
    only_exposure = _stabilize(ctx, frames, temporal_fill=radius, fill_exposure=True).meta["temporal_fill"]
    assert only_feather["exposure"] == {"matched": False, "gain_min": 1.0, "gain_max": 1.0, "candidates_without_overlap": 0}
    assert only_feather["feather_px"] == feather and only_feather["blended_fraction_max"] > 0
    assert only_exposure["feather_px"] == 0 and only_exposure["blended_fraction_max"] == 0.0
    assert only_exposure["exposure"] == block["exposure"]
