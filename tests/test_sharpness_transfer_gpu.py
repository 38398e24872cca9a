"""GPU: vstab_frame_sharpness_batch (csrc/vstab_sharp.hip), vstab_sharp_transfer_batch (csrc/vstab_neighbour.hip:
sharp_transfer_kernel) and the `sharpness_transfer` keyword / the Sharpness Transfer node.

Every comparison of energies, pixels and counts is exact and over all pixels, against the NumPy restatement
(tests/sharpness_restatement.py, refereed on the CPU in tests/test_sharpness_transfer_cpu.py).  End to end, the referee's clip
goes through the estimator: the blurred frames must come closer to the sharp frame 0 they are locked to, by at least half of
what the CPU referee gains with the true matrices.
"""

import json

import numpy as np
import pytest

from tests import sharpness_restatement as S
from tests.util import similarity

pytestmark = pytest.mark.gpu

INTERPS = ["bilinear", "bicubic"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the sharpness kernel -----------------------------------------------------------------------------------------------
def _energy(ctx, frames):
    import torch

    return [int(v) for v in ctx.frame_sharpness_batch(torch.from_numpy(frames).to(ctx.device)).cpu().numpy()]


def _noise(shape, seed):
    """Noise, so every tile seam carries gradient; a twentieth of the values below 0, above 1, NaN, inf or -inf."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    nasty = np.array([np.nan, np.inf, -np.inf, -0.5, 1.5, 3.0, -0.0, 1.0, 2.0 ** -17], np.float32)
    hit = rng.uniform(0, 1, shape) < 0.05
    a[hit] = rng.choice(nasty, size=int(hit.sum()))
    return a


# (n, h, w): thin frames, one pixel, sizes around the 64 x 32 tile in both orders, more than one tile per axis, and a clip
# whose frames of 33 x 7 x 3 floats start off a 16-byte boundary
SHARP_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 2, 2), (1, 65, 9), (1, 9, 65), (1, 63, 17), (1, 17, 63), (2, 130, 35),
                (2, 35, 130), (5, 33, 7), (5, 7, 33)]


@pytest.mark.parametrize("shape", SHARP_SHAPES)
def test_sharpness_matches_restatement(ctx, shape):
    n, h, w = shape
    frames = _noise((n, h, w, 3), seed=h * 131 + w)
    got, want = _energy(ctx, frames), S.frame_sharpness(frames)
    assert got == want
    assert (w == 1 or h == 1) == (max(want) == 0)
    clean = np.random.default_rng(h + w).uniform(0, 1, (n, h, w, 3)).astype(np.float32)
    assert _energy(ctx, clean) == S.frame_sharpness(clean)


def test_sharpness_of_a_view_that_starts_off_16_bytes(ctx):
    """frames[1:] of a 33 x 7 clip starts 33 * 7 * 12 = 2772 bytes in: 4 past a 16-byte boundary."""
    import torch

    frames = _noise((5, 7, 33, 3), seed=9)
    dev = torch.from_numpy(frames).to(ctx.device)
    got = [int(v) for v in ctx.frame_sharpness_batch(dev[1:]).cpu().numpy()]
    assert dev[1:].data_ptr() % 16 != 0 and got == S.frame_sharpness(frames[1:])


def test_sharpness_1080p_and_extremes(ctx):
    frames = _noise((1, 1080, 1920, 3), seed=1080)
    assert _energy(ctx, frames) == S.frame_sharpness(frames)
    # every pixel at the largest step: a checkerboard of 0 and 5.0 contributes 2^33 per pixel
    ys, xs = np.meshgrid(np.arange(70), np.arange(131), indexing="ij")
    board = np.where(((xs + ys) % 2 == 0)[..., None], np.float32(5.0), np.float32(0.0)) * np.ones((1, 1, 1, 3), np.float32)
    assert _energy(ctx, board) == [2 ** 33 * 130 * 69] == S.frame_sharpness(board)
    assert _energy(ctx, np.full((3, 40, 70, 3), 0.25, np.float32)) == [0, 0, 0]


def test_sharpness_refuses_bad_arguments(ctx):
    import torch

    from vstab_amd import native

    a = torch.zeros((2, 8, 9, 3), device=ctx.device)
    with pytest.raises(ValueError, match="frame_sharpness_batch: frames must be a contiguous float32"):
        ctx.frame_sharpness_batch(a.double())
    with pytest.raises(ValueError, match="frame_sharpness_batch: frames must be a contiguous float32"):
        ctx.frame_sharpness_batch(a.transpose(1, 2))
    with pytest.raises(ValueError, match=r"frame_sharpness_batch: frames of shape \(2, 8, 9\) are not \[n,h,w,3\]"):
        ctx.frame_sharpness_batch(a[..., 0].contiguous())
    with pytest.raises(native.VstabError, match="vstab_frame_sharpness_batch: bad shape n=0"):
        ctx.frame_sharpness_batch(a[:0])


# ---- the transfer kernel --------------------------------------------------------------------------------------------------
SW, SH, CLIP = 80, 48, 5


def _transfer_case(dw, dh, K, seed, n=3):
    """A clip of 5 frames of 80 x 48, n output frames on a dw x dh canvas, K candidates per frame: similarities that cover
    the canvas wholly or in part, a perspective one, a singular one, far-outside ones and -1 slots; ratios 0 or in
    [1.1, 12]; dst prefilled with noise."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0.0, 1.0, (CLIP, SH, SW, 3)).astype(np.float32)
    dst = rng.uniform(0.0, 1.0, (n, dh, dw, 3)).astype(np.float32)
    mats = np.zeros((n, K, 3, 3), np.float32)
    cand = np.zeros((n, K), np.int32)
    for f in range(n):
        for k in range(K):
            kind = (f + k) % 6 if K >= 6 else int(rng.integers(0, 3))
            m = similarity((dw - SW) / 2 + rng.uniform(-0.1, 0.1) * dw, (dh - SH) / 2 + rng.uniform(-0.1, 0.1) * dh,
                           rng.uniform(-0.2, 0.2), rng.uniform(0.9, 1.4), SW / 2, SH / 2)
            if kind == 1:                                                    # covers only a part of the canvas (and of a tile)
                m = similarity(rng.uniform(0.3, 0.6) * dw, rng.uniform(-0.4, 0.4) * dh, rng.uniform(-0.3, 0.3), 1.0)
            elif kind == 3:
                m[2, :2] = rng.uniform(-6e-4, 6e-4, 2)
            elif kind == 4:
                m[1] = m[0] * 2.0                                            # singular
            elif kind == 5:
                m = similarity(5.0 * dw, 3.0 * dh, 0.0, 1.0)                 # far outside
            mats[f, k] = m
            cand[f, k] = -1 if rng.uniform() < 0.15 else rng.integers(0, CLIP)
    ratio = np.where(rng.uniform(0, 1, (n, K)) < 0.3, 0.0, rng.uniform(1.1, 12.0, (n, K))).astype(np.float32)
    return src, dst, mats, cand, ratio


def _masks(n, dh, dw):
    """all own (with soft values that are not exactly 1), half padded (the left half, a band, single pixels), None."""
    own = np.zeros((n, dh, dw), np.float32)
    own[:, ::5, ::7] = 0.999
    own[:, 1::5, ::7] = 0.5
    half = own.copy()
    half[:, :, :dw // 2] = 1.0
    half[:, dh // 3, :] = 1.0
    half[:, ::4, dw // 2 + 1::6] = 1.0
    return {"own": own, "half": half, "none": None}


def _run_transfer(ctx, src, mats, cand, ratio, alpha, dst, mask, interp="bilinear", first=0, subpix=None):
    import torch

    d = torch.from_numpy(dst).to(ctx.device).contiguous()
    m = None if mask is None else torch.from_numpy(mask).to(ctx.device).contiguous()
    count = ctx.sharp_transfer_batch(torch.from_numpy(src).to(ctx.device), mats, cand, ratio, alpha, d, m, first=first,
                                     interp=interp, subpix=subpix)
    if m is not None:
        assert np.array_equal(_bits(m.cpu().numpy()), _bits(mask)), "the mask was written"
    return d.cpu().numpy(), count.cpu().numpy().astype(np.int64)


def _assert_same(got, want):
    (d, c), (rd, rc) = got, want
    assert np.array_equal(_bits(d), _bits(rd)), f"dst differs at {int((_bits(d) != _bits(rd)).any(axis=-1).sum())} pixels"
    assert np.array_equal(c, rc), (c, rc)


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("K", [2, 8, 32])
@pytest.mark.parametrize("canvas", [(96, 40), (33, 19)])
def test_transfer_matches_restatement(ctx, oracle, canvas, K, interp):
    dw, dh = canvas
    src, dst, mats, cand, ratio = _transfer_case(dw, dh, K, seed=dw * 3 + K)
    touched = 0
    for kind, mask in _masks(dst.shape[0], dh, dw).items():
        want = S.sharp_transfer(src, mats, cand, ratio, 16.0, dst, mask, interp)
        got = _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, mask, interp)
        _assert_same(got, want)
        changed = (_bits(got[0]) != _bits(dst)).any(axis=-1)
        if mask is not None:
            assert not changed[mask == 1.0].any()                      # padded pixels keep every bit
        assert int(changed.sum()) <= int(want[1].sum())
        touched += int(want[1].sum())
    assert touched > 0, "the case transfers nothing: the test would show nothing"


@pytest.mark.parametrize("interp", INTERPS)
def test_transfer_alpha_zero_and_large(ctx, oracle, interp):
    src, dst, mats, cand, ratio = _transfer_case(96, 40, 8, seed=5)
    mask = _masks(3, 40, 96)["half"]
    for alpha in (0.0, 1024.0):
        want = S.sharp_transfer(src, mats, cand, ratio, alpha, dst, mask, interp)
        _assert_same(_run_transfer(ctx, src, mats, cand, ratio, alpha, dst, mask, interp), want)
        assert want[1].sum() > 0


def test_all_zero_ratios_and_dead_candidates_keep_every_bit(ctx):
    src, dst, mats, cand, ratio = _transfer_case(96, 40, 8, seed=6)
    d, c = _run_transfer(ctx, src, mats, cand, np.zeros_like(ratio), 16.0, dst, None)
    assert np.array_equal(_bits(d), _bits(dst)) and (c == 0).all()
    d, c = _run_transfer(ctx, src, mats, np.full_like(cand, -1), ratio, 16.0, dst, None)
    assert np.array_equal(_bits(d), _bits(dst)) and (c == 0).all()
    everything_padded = np.ones(dst.shape[:3], np.float32)
    d, c = _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, everything_padded)
    assert np.array_equal(_bits(d), _bits(dst)) and (c == 0).all()


def test_mixed_frames_only_the_live_ones_change(ctx, oracle):
    """Frames 0 and 2 have no positive ratio: they keep every bit, frame 1 equals the restatement."""
    src, dst, mats, cand, ratio = _transfer_case(96, 40, 8, seed=7)
    ratio[0] = 0.0
    ratio[2] = 0.0
    ratio[1, :4] = 3.0
    cand[1, :4] = [0, 1, 2, 3]
    want = S.sharp_transfer(src, mats, cand, ratio, 16.0, dst, None)
    got = _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, None)
    _assert_same(got, want)
    assert want[1][1] > 0 and want[1][0] == want[1][2] == 0
    assert np.array_equal(_bits(got[0][[0, 2]]), _bits(dst[[0, 2]]))


@pytest.mark.parametrize("interp", INTERPS)
def test_nan_own_pixels_stay_and_nan_samples_are_skipped(ctx, oracle, interp):
    src, dst, mats, cand, ratio = _transfer_case(96, 40, 8, seed=8)
    rng = np.random.default_rng(80)
    nasty = np.array([np.nan, np.inf, -np.inf], np.float32)
    for a, share in ((src, 0.01), (dst, 0.03)):
        hit = rng.uniform(0, 1, a.shape) < share
        a[hit] = rng.choice(nasty, size=int(hit.sum()))
    want = S.sharp_transfer(src, mats, cand, ratio, 16.0, dst, None, interp)
    got = _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, None, interp)
    _assert_same(got, want)
    bad_own = ~np.isfinite(dst).all(axis=-1)
    assert bad_own.any() and np.array_equal(_bits(got[0][bad_own]), _bits(dst[bad_own]))     # D is never below infinity there
    assert want[1].sum() > 0 and np.isfinite(got[0][~bad_own]).all()                         # and no NaN leaks into a finite pixel


def test_two_windows_equal_one_call_in_place(ctx):
    import torch

    src, dst, mats, cand, ratio = _transfer_case(96, 40, 4, seed=11, n=5)
    mask = _masks(5, 40, 96)["half"]
    whole = _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, mask)
    s = torch.from_numpy(src).to(ctx.device)
    d = torch.from_numpy(dst).to(ctx.device)
    m = torch.from_numpy(mask).to(ctx.device)
    parts = [ctx.sharp_transfer_batch(s, mats[a:b], cand[a:b], ratio[a:b], 16.0, d[a:b], m[a:b], first=a) for a, b in ((0, 2), (2, 5))]
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(whole[0])) and whole[1].sum() > 0
    assert np.array_equal(torch.cat(parts).cpu().numpy(), whole[1])


def test_exact_mode_and_bad_arguments_are_refused(ctx):
    from vstab_amd import native

    src, dst, mats, cand, ratio = _transfer_case(96, 40, 2, seed=4)
    with pytest.raises(native.VstabError, match="exact"):
        _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, None, subpix="exact")
    for alpha in (-1.0, float("nan"), float("inf")):
        with pytest.raises(native.VstabError, match="alpha="):
            _run_transfer(ctx, src, mats, cand, ratio, alpha, dst, None)
    bad = ratio.copy()
    bad[1, 1] = -2.0
    with pytest.raises(native.VstabError, match=r"ratio\[3\]=-2"):
        _run_transfer(ctx, src, mats, cand, bad, 16.0, dst, None)
    bad[1, 1] = np.inf
    with pytest.raises(native.VstabError, match=r"ratio\[3\]=inf"):
        _run_transfer(ctx, src, mats, cand, bad, 16.0, dst, None)
    with pytest.raises(native.VstabError, match="ratio"):
        _run_transfer(ctx, src, mats, cand, ratio[:, :1], 16.0, dst, None)
    far = cand.copy()
    far[0, 0] = CLIP
    with pytest.raises(native.VstabError, match="cand_frame"):
        _run_transfer(ctx, src, mats, far, ratio, 16.0, dst, None)
    with pytest.raises(native.VstabError, match="outside a clip"):
        _run_transfer(ctx, src, mats, cand, ratio, 16.0, dst, None, first=3)
    big = np.tile(mats, (1, 40, 1, 1))                       # K = 80
    with pytest.raises(native.VstabError, match="K=80"):
        _run_transfer(ctx, src, big, np.tile(cand, (1, 40)), np.tile(ratio, (1, 40)), 16.0, dst, None)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _stabilize(ctx, frames, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", True, 0.9, 0.8, 0.6,
                                (127, 127, 127), 16.0, ctx=ctx, keep_on_device=True, estimator="flow", **kw)


def test_end_to_end_keyword_and_node(pkg, ctx, oracle):
    """The referee's clip through the estimator, camera locked, with and without sharpness_transfer=2.  PSNR of a blurred
    frame against output frame 0 (sharp, and what every frame is locked to) over the pixels neither pads.  The mean gain
    must reach half of the CPU referee's with the true matrices (10.45 dB there, so 5.2 dB here): estimated transitions
    carry sub-pixel error, and a blurred frame's own estimate is the weakest."""
    import torch

    from vstab_amd import nodes
    from vstab_amd import temporal_fill as tf

    clip = S.referee_clip()
    frames = torch.from_numpy(clip["frames"]).to(ctx.device)
    off = _stabilize(ctx, frames)
    on = _stabilize(ctx, frames, sharpness_transfer=2)

    meta_on = dict(on.meta)
    block = meta_on.pop("sharpness_transfer")
    assert "sharpness_transfer" not in off.meta
    assert json.dumps(meta_on, sort_keys=True) == json.dumps(off.meta, sort_keys=True)
    assert list(block) == ["version", "radius", "alpha", "min_ratio", "sharpness", "frames_sharpened", "ratio_max",
                           "transferred_fraction_mean", "transferred_fraction_max"]
    assert (block["version"], block["radius"], block["alpha"], block["min_ratio"]) == (1, 2, 16.0, 1.1)
    assert block["frames_sharpened"] == len(clip["blurred"]) == 2 and 5.0 < block["ratio_max"] < 12.0
    assert 0.0 < block["transferred_fraction_mean"] < block["transferred_fraction_max"] <= 1.0
    energy = S.frame_sharpness(clip["frames"])
    assert block["sharpness"] == [e / (2.0 ** 32 * 159 * 119) for e in energy]

    d_off, d_on = off.frames.cpu().numpy(), on.frames.cpu().numpy()
    m_off, m_on = off.masks.cpu().numpy()[..., 0], on.masks.cpu().numpy()[..., 0]
    assert np.array_equal(_bits(m_on), _bits(m_off))
    keep = [i for i in range(len(d_off)) if i not in clip["blurred"]]
    assert np.array_equal(_bits(d_on[keep]), _bits(d_off[keep]))

    gains = []
    for i in clip["blurred"]:
        both = (m_off[i] == 0) & (m_off[0] == 0)
        before, after = S.psnr(d_off[i], d_off[0], both), S.psnr(d_on[i], d_on[0], both)
        print(f"end to end, frame {i}: {before:.2f} dB -> {after:.2f} dB against output frame 0")
        assert after > before
        gains.append(after - before)
    want = S.referee()["gain_mean"]
    print(f"end to end: mean gain {np.mean(gains):.2f} dB; the CPU referee with the true matrices: {want:.2f} dB")
    assert np.mean(gains) >= 0.5 * want

    # the restatement applied to the run without the keyword, from that run's own meta JSON, gives the keyword's bits
    meta = json.loads(json.dumps(off.meta))
    final = np.array([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)
    trans = np.array([e["matrix"] for e in meta["estimated_motion"]["per_transition"]], np.float32)
    conf = np.array([e["confidence"] for e in meta["estimated_motion"]["per_transition"]], np.float64)
    mats, cand = tf.fill_candidates(final, trans, conf, 2)
    ratios = S.ratios_from_energy(energy, cand)
    rd, rc = S.sharp_transfer(clip["frames"], mats, cand, ratios, 16.0, d_off, m_off)
    assert np.array_equal(_bits(d_on), _bits(rd)) and rc[clip["blurred"]].min() > 0
    pixels = np.float32(d_off.shape[1] * d_off.shape[2])
    frac = (rc.astype(np.float32) / pixels).astype(np.float64)
    assert block["transferred_fraction_mean"] == float(np.mean(frac)) and block["transferred_fraction_max"] == float(np.max(frac))
    assert block["ratio_max"] == float(ratios.max())

    # the node, from the meta JSON alone, gives the keyword's bits and leaves its inputs alone; without a mask every pixel is own
    out = nodes.VideoStabilizerSharpnessTransfer.execute(frames, off.frames, meta, 2, 16.0, off.masks)
    node_frames, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(rd)) and json.loads(node_meta) == {"sharpness_transfer": block}
    assert np.array_equal(_bits(off.frames.cpu().numpy()), _bits(d_off))
    out = nodes.VideoStabilizerSharpnessTransfer.execute(frames, off.frames, meta, 2, 16.0)
    bare = (out.result if hasattr(out, "result") else out.args)[0].cpu().numpy()
    assert np.array_equal(_bits(bare), _bits(S.sharp_transfer(clip["frames"], mats, cand, ratios, 16.0, d_off, None)[0]))

    # it runs in front of the fills: with temporal_fill the fill sees the transferred frames, and padding is filled as before
    filled_off = _stabilize(ctx, frames, temporal_fill=2)
    filled_on = _stabilize(ctx, frames, temporal_fill=2, sharpness_transfer=2, sharpness_alpha=16.0)
    assert filled_on.meta["temporal_fill"] == filled_off.meta["temporal_fill"] and filled_on.meta["sharpness_transfer"] == block
    assert np.array_equal(_bits(filled_on.masks.cpu().numpy()), _bits(filled_off.masks.cpu().numpy()))
    own = m_off == 0
    assert np.array_equal(_bits(filled_on.frames.cpu().numpy()[own]), _bits(d_on[own]))


def test_refusals_are_raised_before_any_gpu_work(pkg, ctx, monkeypatch):
    import torch

    from vstab_amd import distributed, native

    frames = torch.from_numpy(S.referee_clip()["frames"]).to(ctx.device)
    with pytest.raises(ValueError, match="not supported with mesh_warp"):
        _stabilize(ctx, frames, sharpness_transfer=2, mesh_warp=True)
    with pytest.raises(ValueError, match="not supported with estimator 'subject'"):
        from vstab_amd import flow_pipeline as fp
        from vstab_amd import host_math as hm
        fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127),
                             16.0, ctx=ctx, estimator="subject", subject_mask=torch.zeros(frames.shape[:3]), sharpness_transfer=2)
    with pytest.raises(ValueError, match="sharpness_alpha=4.0 needs sharpness_transfer > 0"):
        _stabilize(ctx, frames, sharpness_alpha=4.0)
    with pytest.raises(ValueError, match="not sharded"):
        distributed.stabilize_sharded(ctx, frames, 9, "crop_and_pad", "similarity", True, 0.9, 0.8, 0.6, (127, 127, 127), 16.0,
                                      sharpness_transfer=2)
    monkeypatch.setattr(native, "DEFAULT_SUBPIX", "exact")
    with pytest.raises(ValueError, match="sub-pixel mode 'exact'"):
        _stabilize(ctx, frames, sharpness_transfer=2)
