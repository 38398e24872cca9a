"""GPU: vstab_temporal_fill_batch (csrc/vstab_neighbour.hip: temporal_fill_kernel) and the `temporal_fill` keyword / node.

Every comparison of pixels, masks, indices and counts is bit-exact and over all pixels: against the NumPy restatement
(tests/temporal_fill_restatement.py, whose validity rule is refereed on the CPU in tests/test_temporal_fill_cpu.py),
and, without any restatement, against a texture whose windows at integer offsets are the frames (weights 1, 0, 0, 0).
"""

import json

import numpy as np
import pytest

from tests import temporal_fill_restatement as R
from tests.util import shake_path, similarity

pytestmark = pytest.mark.gpu

MODES = [("bilinear", "q5"), ("bilinear", "exact"), ("bicubic", "q5")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _drawn_case(n, clip, sh, sw, dh, dw, K, seed):
    """Random clip, prefilled dst (NaN-free), a mask of exact ones (border band + boxes), zeros and a few soft values,
    and K candidates per frame drawn from similarity / perspective / far-outside / singular matrices and -1 slots."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.0, 1.0, (clip, sh, sw, 3)).astype(np.float32)
    dst = rng.uniform(0.0, 1.0, (n, dh, dw, 3)).astype(np.float32)
    mask = np.zeros((n, dh, dw), np.float32)
    band = max(2, dh // 6)
    mask[:, :band] = 1.0
    mask[:, :, -max(2, dw // 5):] = 1.0
    for f in range(n):
        y0, x0 = rng.integers(0, dh // 2), rng.integers(0, dw // 2)
        mask[f, y0:y0 + dh // 3, x0:x0 + dw // 4] = 1.0
    soft = rng.uniform(0, 1, mask.shape) < 0.02
    mask[soft] = rng.choice(np.array([0.5, 0.25, 0.999, 0.0], np.float32), size=int(soft.sum()))
    mats = np.zeros((n, K, 3, 3), np.float32)
    cand = np.zeros((n, K), np.int32)
    for f in range(n):
        for k in range(K):
            kind = rng.integers(0, 6)
            m = similarity(rng.uniform(-0.5 * dw, 0.5 * dw), rng.uniform(-0.5 * dh, 0.5 * dh), rng.uniform(-0.3, 0.3),
                           rng.uniform(0.8, 1.3), dw / 2, dh / 2)
            if kind == 1:
                m[2, :2] = rng.uniform(-6e-4, 6e-4, 2)
            elif kind == 2:
                m = similarity(rng.choice([-1, 1]) * 5.0 * dw, 3.0 * dh, 0.0, 1.0)      # far outside
            elif kind == 3:
                m[1] = m[0] * 2.0                                                        # singular
            elif kind == 4:
                m = similarity(float(rng.integers(-dw // 3, dw // 3)), float(rng.integers(-dh // 3, dh // 3)), 0.0, 1.0)
            mats[f, k] = m
            cand[f, k] = -1 if rng.uniform() < 0.15 else rng.integers(0, clip)
    return src, dst, mask, mats, cand


def _run_kernel(ctx, src, mats, cand, dst, mask, interp, subpix, first=0):
    import torch

    d = torch.from_numpy(dst).to(ctx.device).contiguous()
    m = torch.from_numpy(mask).to(ctx.device).contiguous()
    ff, fc, pc = ctx.temporal_fill_batch(torch.from_numpy(src).to(ctx.device), mats, cand, d, m, first=first, interp=interp,
                                         subpix=subpix, want_filled_from=True)
    return d.cpu().numpy(), m.cpu().numpy(), ff.cpu().numpy(), fc.cpu().numpy().astype(np.int64), pc.cpu().numpy().astype(np.int64)


def _assert_equal_to_restatement(got, want):
    d, m, ff, fc, pc = got
    rd, rm, rff, rfc, rpc = want
    assert np.array_equal(ff, rff), f"filled_from differs at {int((ff != rff).sum())} pixels"
    assert np.array_equal(_bits(m), _bits(rm)), f"mask differs at {int((_bits(m) != _bits(rm)).sum())} pixels"
    assert np.array_equal(_bits(d), _bits(rd)), f"dst differs at {int((_bits(d) != _bits(rd)).any(axis=-1).sum())} pixels"
    assert np.array_equal(fc, rfc) and np.array_equal(pc, rpc), (fc, rfc, pc, rpc)


# (n, clip, src h, src w, out h, out w, K): sizes that are no multiples of the 64 x 8 tile; source != canvas in two of them
SHAPES = [(3, 4, 37, 53, 37, 53, 1), (2, 5, 270, 481, 290, 500, 2), (3, 6, 61, 83, 45, 131, 16)]


@pytest.mark.parametrize("interp,subpix", MODES)
@pytest.mark.parametrize("shape", SHAPES + [(2, 3, 9, 65, 9, 65, 1)])      # 9 x 65: the last 64 x 8 tile holds one (padded) pixel
def test_kernel_matches_restatement(ctx, oracle, shape, interp, subpix):
    n, clip, sh, sw, dh, dw, K = shape
    src, dst, mask, mats, cand = _drawn_case(n, clip, sh, sw, dh, dw, K, seed=dh * 7 + K)
    got = _run_kernel(ctx, src, mats, cand, dst, mask, interp, subpix)
    want = R.temporal_fill(src, mats, cand, dst, mask, interp, subpix)
    _assert_equal_to_restatement(got, want)
    if K > 1:
        assert want[3].sum() > 0 and want[4].sum() > 0      # something was filled, something stayed padded
    # untouched guarantee: where the input mask is not exactly 1, pixel and mask keep their input bits
    keep = mask != 1.0
    assert np.array_equal(_bits(got[0])[keep], _bits(dst)[keep]) and np.array_equal(_bits(got[1])[keep], _bits(mask)[keep])
    assert (got[2][keep] == -1).all()


@pytest.mark.parametrize("interp,subpix", [("bilinear", "q5"), ("bicubic", "q5")])
def test_kernel_matches_restatement_1080p(ctx, oracle, interp, subpix):
    src, dst, mask, mats, cand = _drawn_case(1, 3, 1080, 1920, 1080, 1920, 16, seed=1080)
    got = _run_kernel(ctx, src, mats, cand, dst, mask, interp, subpix)
    want = R.temporal_fill(src, mats, cand, dst, mask, interp, subpix)
    _assert_equal_to_restatement(got, want)
    assert want[3].sum() > 0


def test_all_zero_mask_leaves_every_byte(ctx):
    src, dst, mask, mats, cand = _drawn_case(2, 3, 40, 70, 40, 70, 4, seed=2)
    mask[:] = 0.0
    d, m, ff, fc, pc = _run_kernel(ctx, src, mats, cand, dst, mask, "bilinear", "q5")
    assert np.array_equal(_bits(d), _bits(dst)) and np.array_equal(_bits(m), _bits(mask))
    assert (ff == -1).all() and (fc == 0).all() and (pc == 0).all()


def test_invalid_arguments_are_refused(ctx):
    from vstab_amd import native

    src, dst, mask, mats, cand = _drawn_case(2, 3, 40, 70, 40, 70, 2, seed=4)
    bad = cand.copy()
    bad[0, 0] = 3                                            # clip has frames 0..2
    with pytest.raises(native.VstabError, match="cand_frame"):
        _run_kernel(ctx, src, mats, bad, dst, mask, "bilinear", "q5")
    with pytest.raises(native.VstabError, match="outside a clip"):
        _run_kernel(ctx, src, mats, cand, dst, mask, "bilinear", "q5", first=2)
    big = np.tile(mats, (1, 40, 1, 1))                       # K = 80
    with pytest.raises(native.VstabError, match="K=80"):
        _run_kernel(ctx, src, big, np.tile(cand, (1, 40)), dst, mask, "bilinear", "q5")


def test_two_windows_equal_one_call(ctx):
    import torch

    n = 5
    src, dst, mask, mats, cand = _drawn_case(n, n, 50, 90, 50, 90, 4, seed=8)
    whole = _run_kernel(ctx, src, mats, cand, dst, mask, "bilinear", "q5")
    s = torch.from_numpy(src).to(ctx.device)
    d = torch.from_numpy(dst).to(ctx.device)
    m = torch.from_numpy(mask).to(ctx.device)
    parts = []
    for a, b in ((0, 2), (2, n)):
        parts.append(ctx.temporal_fill_batch(s, mats[a:b], cand[a:b], d[a:b], m[a:b], first=a, want_filled_from=True))
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(whole[0])) and np.array_equal(_bits(m.cpu().numpy()), _bits(whole[1]))
    for i, idx in ((0, 2), (1, 3), (2, 4)):
        assert np.array_equal(torch.cat([p[i] for p in parts]).cpu().numpy(), whole[idx])


def test_known_answer_integer_windows(ctx, pkg):
    """Frames are windows of one random texture at integer offsets, matrices the matching integer translations: every
    filled pixel is the texture's value at that position, bit for bit, and every padded pixel that some frame within the
    radius covers by the interior rule is filled, by the first such frame in candidate order.  No restatement involved."""
    import torch

    from vstab_amd import temporal_fill as tf

    n, h, w, pad, radius = 9, 67, 101, 48, 3
    rng = np.random.default_rng(31)
    tex = rng.uniform(0.0, 1.0, (h + 2 * pad, w + 2 * pad, 3)).astype(np.float32)
    offs = rng.integers(-25, 26, size=(n, 2))               # (ox, oy): frame_i(x, y) = tex[y + oy + pad, x + ox + pad]
    frames = np.stack([tex[pad + oy:pad + oy + h, pad + ox:pad + ox + w] for ox, oy in offs])
    final = np.stack([similarity(float(ox - offs[0, 0]), float(oy - offs[0, 1]), 0.0, 1.0) for ox, oy in offs]).astype(np.float32)
    trans = np.stack([similarity(float(offs[i, 0] - offs[i + 1, 0]), float(offs[i, 1] - offs[i + 1, 1]), 0.0, 1.0)
                      for i in range(n - 1)]).astype(np.float32)
    src = torch.from_numpy(frames).to(ctx.device)
    dst, mask, _ = ctx.warp_batch(src, final, (w, h), border=(0.5, 0.5, 0.5), want_mask=True)
    before = mask.cpu().numpy()
    mats, cand = tf.fill_candidates(final, trans, np.ones(n - 1), radius)
    ff, fc, pc = ctx.temporal_fill_batch(src, mats, cand, dst, mask, want_filled_from=True)
    out, after, ff = dst.cpu().numpy(), mask.cpu().numpy(), ff.cpu().numpy()

    want = tex[pad + offs[0, 1]:pad + offs[0, 1] + h, pad + offs[0, 0]:pad + offs[0, 0] + w]   # every canvas shows frame 0's window
    ys, xs = np.mgrid[0:h, 0:w]
    total_filled = 0
    for i in range(n):
        expect_from = np.full((h, w), -1, np.int8)
        for k in range(2 * radius - 1, -1, -1):             # reverse order: the first candidate in order wins
            j = cand[i, k]
            if j < 0:
                continue
            sx, sy = xs + offs[0, 0] - offs[j, 0], ys + offs[0, 1] - offs[j, 1]      # canvas p -> frame j
            inside = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
            expect_from[inside] = k
        expect_from[before[i] != 1.0] = -1
        assert np.array_equal(ff[i], expect_from), f"frame {i}: {int((ff[i] != expect_from).sum())} pixels filled from another frame"
        filled = expect_from >= 0
        assert np.array_equal(_bits(out[i])[filled], _bits(want)[filled])
        assert (after[i][filled] == 0.0).all() and np.array_equal(after[i][~filled], before[i][~filled])
        assert int(fc[i]) == int(filled.sum()) and int(pc[i]) == int((after[i] == 1.0).sum())
        total_filled += int(filled.sum())
    assert total_filled > 2000 and (before == 1.0).sum() > total_filled     # some padding no frame within the radius saw


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H, N = 480, 270, 12


def _clip(mode, seed=3, amp=1.5):
    import torch

    import bench

    cam = shake_path(N, W, H, mode, seed=seed, amp=amp)
    return cam, bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=cam)


def _stabilize(pkg, ctx, frames, framing, mode, estimator, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, False, 0.9, 0.8, 0.6, (127, 127, 127), 16.0,
                                ctx=ctx, keep_on_device=True, estimator=estimator, **kw)


@pytest.mark.parametrize("framing,mode,estimator", [("crop_and_pad", "similarity", "flow"), ("expand", "perspective", "flow"),
                                                    ("crop_and_pad", "similarity", "classic")])
def test_end_to_end_keyword_and_node(pkg, ctx, oracle, framing, mode, estimator):
    from vstab_amd import nodes
    from vstab_amd import temporal_fill as tf

    radius = 4
    _, frames = _clip(mode)
    plain = _stabilize(pkg, ctx, frames, framing, mode, estimator)                      # the parent's call
    off = _stabilize(pkg, ctx, frames, framing, mode, estimator, temporal_fill=0)
    on = _stabilize(pkg, ctx, frames, framing, mode, estimator, temporal_fill=radius)

    # temporal_fill=0 is the call without the keyword: pixels, mask and meta
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(plain.frames.cpu().numpy()))
    assert np.array_equal(_bits(off.masks.cpu().numpy()), _bits(plain.masks.cpu().numpy()))
    assert json.dumps(off.meta, sort_keys=True) == json.dumps(plain.meta, sort_keys=True) and "temporal_fill" not in off.meta
    if framing == "crop_and_pad" and estimator == "flow":
        assert on.device_plan["used"]                                                    # the device-plan path

    # existing keys keep their pre-fill values
    meta_on = dict(on.meta)
    block = meta_on.pop("temporal_fill")
    assert json.dumps(meta_on, sort_keys=True) == json.dumps(off.meta, sort_keys=True)

    # the restatement applied to the temporal_fill=0 output, from that run's own meta JSON
    meta = json.loads(json.dumps(off.meta))
    final = np.array([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)
    trans = np.array([e["matrix"] for e in meta["estimated_motion"]["per_transition"]], np.float32)
    conf = np.array([e["confidence"] for e in meta["estimated_motion"]["per_transition"]], np.float64)
    mats, cand = tf.fill_candidates(final, trans, conf, radius)
    src = frames.cpu().numpy()
    d0, m0 = off.frames.cpu().numpy(), off.masks.cpu().numpy()[..., 0]
    rd, rm, _, rfc, rpc = R.temporal_fill(src, mats, cand, d0, m0, "bilinear", "q5")
    assert rfc.sum() > 0, "the clip has no padding that a neighbour covers: the test would show nothing"
    assert np.array_equal(_bits(on.frames.cpu().numpy()), _bits(rd))
    assert np.array_equal(_bits(on.masks.cpu().numpy()[..., 0]), _bits(rm))
    pixels = np.float32(d0.shape[1] * d0.shape[2])
    assert block == {"radius": radius,
                     "filled_fraction_mean": float(np.mean((rfc.astype(np.float32) / pixels).astype(np.float64))),
                     "filled_fraction_max": float(np.max((rfc.astype(np.float32) / pixels).astype(np.float64))),
                     "padding_fraction_mean_after": float(np.mean((rpc.astype(np.float32) / pixels).astype(np.float64))),
                     "padding_fraction_max_after": float(np.max((rpc.astype(np.float32) / pixels).astype(np.float64)))}

    # the node, from the meta JSON alone, gives the keyword's bits and leaves its inputs alone
    out = nodes.VideoStabilizerTemporalFill.execute(frames, off.frames, off.masks, meta, radius, "bilinear")
    node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(rd)) and np.array_equal(_bits(node_mask.cpu().numpy()), _bits(rm))
    assert node_meta["temporal_fill"] == {**block, "interpolation": "bilinear"}
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(d0))


def test_crop_framing_is_a_noop(pkg, ctx):
    _, frames = _clip("similarity")
    a = _stabilize(pkg, ctx, frames, "crop", "similarity", "flow")
    b = _stabilize(pkg, ctx, frames, "crop", "similarity", "flow", temporal_fill=4)
    assert np.array_equal(_bits(a.frames.cpu().numpy()), _bits(b.frames.cpu().numpy()))
    assert json.dumps(a.meta, sort_keys=True) == json.dumps(b.meta, sort_keys=True)


def test_node_refuses_meta_without_transitions(pkg, ctx):
    import torch

    from vstab_amd import nodes

    z = torch.zeros((2, 8, 8, 3))
    with pytest.raises(ValueError, match="estimated_motion"):
        nodes.VideoStabilizerTemporalFill.execute(z, z, torch.zeros((2, 8, 8)), {"stabilization_warp": {"per_frame": []}}, 8, "bilinear")


QUALITY_MARGIN_DB = 9.0   # measured gap 7.38 dB -> 8 dB, + 1 dB: see test_filled_pixels_are_as_good_as_the_interior


def _psnr(err2):
    return float(10.0 * np.log10(1.0 / max(float(err2), 1e-20)))


def measure_fill_quality(pkg, ctx, radius=4):
    """(filled PSNR, interior PSNR, filled pixels, interior pixels) on the analytic clip: output frame i must show
    T((F_i M_i)^-1 p) (bench.synth_clip samples it without interpolation).  Interior = pixels the warp never padded, two
    pixels in from the padding (a bilinear tap next to the border blends the padding colour in) -- the existing warp's own
    error, the yardstick; filled = pixels the fill wrote."""
    import torch

    import bench

    cam, frames = _clip("similarity")
    off = _stabilize(pkg, ctx, frames, "crop_and_pad", "similarity", "flow", temporal_fill=0)
    on = _stabilize(pkg, ctx, frames, "crop_and_pad", "similarity", "flow", temporal_fill=radius)
    final = np.array([e["applied_matrix"] for e in on.meta["stabilization_warp"]["per_frame"]], np.float64)
    truth = bench.synth_clip(N, 0, H, W, torch.device("cuda"), mats=final @ cam)
    before, after = off.masks[..., 0], on.masks[..., 0]
    filled = (before == 1.0) & (after == 0.0)
    padded = torch.nn.functional.max_pool2d((before != 0.0)[:, None].float(), 5, stride=1, padding=2)[:, 0] > 0
    interior = ~padded
    interior[:, :2] = interior[:, -2:] = False
    interior[:, :, :2] = interior[:, :, -2:] = False
    err2 = ((on.frames - truth) ** 2).mean(dim=-1)
    return (_psnr(err2[filled].mean().item()), _psnr(err2[interior].mean().item()), int(filled.sum().item()),
            int(interior.sum().item()))


def test_filled_pixels_are_as_good_as_the_interior(pkg, ctx):
    """Oracle-independent quality: PSNR of the filled pixels against the analytic truth next to the PSNR of the never-padded
    interior of the same frames (the existing warp's result).  The margin is the gap observed in one measured run rounded
    up to the next whole dB, plus 1 dB of headroom for clip changes (results are deterministic).  Measured (MI355X, this
    clip, radius 4): filled 43.66 dB over 5789 px, interior 51.04 dB over 1513638 px -- gap 7.38 dB, margin 9 dB
    (profiles/r07_temporal_fill.md; radius 2: 44.00 dB, radius 8: 43.66 dB).  The filled pixels lie at the frame's edge,
    where the transition chain's error is largest, and carry it on top of the interpolation error the interior has."""
    filled_db, interior_db, n_filled, n_interior = measure_fill_quality(pkg, ctx)
    print(f"temporal fill quality: filled {filled_db:.2f} dB over {n_filled} px, interior {interior_db:.2f} dB over {n_interior} px")
    assert n_filled > 1000 and n_interior > 100000
    assert filled_db >= interior_db - QUALITY_MARGIN_DB, (filled_db, interior_db)
