"""Estimation mask on the GPU (include/vstab.h "Estimation mask"; flow_pipeline._stabilize_frames(estimation_mask=...)).

  * vstab_mask_block_grid against the NumPy restatement of the rule (tests/estimation_mask_restatement.py), bit for bit
  * the masked fit against the unmasked fit on the NaN-poisoned grid (bit for bit) and against the CPU oracle on the same
    grid (the tolerances of tests/test_fit_gpu.py, which are those of the unmasked fit against the oracle)
  * no mask and an all-zero mask: the same frames, masks and meta
  * the purpose, oracle-independent: a clip whose larger part is a moving subject (see subject_clip).  Without the mask
    every pair's estimate is off by more than 1 px (it is the subject's motion); with the exact rectangle masks and the
    default margin every pair is within MASKED_BOUNDS of the background's true transition.

MASKED_BOUNDS (px at working resolution, error of the reported displacement at the frame centre, max over ALL pairs) were
set as tests/test_analytic_gpu.py sets its own: measured with tools/estimation_mask_accuracy.py over 47 pairs per case
(profiles/r08_estimation_mask.md), measured maximum plus 30-50 % headroom:

  case (47 pairs, DIS unless stated)   unmasked min..max   masked, margin 16: max   bound    clean-clip bound (test_analytic_gpu.py)
  960x540   translation                2.01 .. 7.87 px      0.0430 px                0.06     0.05
  960x540   similarity                 1.68 .. 9.03 px      0.0517 px                0.07     0.05
  960x540   perspective                2.14 .. 8.85 px      0.0533 px                0.075    0.08
  1920x1080 translation                2.01 .. 7.87 px      0.0418 px                0.06     0.05
  1920x1080 similarity                 1.66 .. 9.03 px      0.0489 px                0.07     0.05
  1920x1080 perspective                2.18 .. 8.85 px      0.0578 px                0.08     0.08
  480x270   similarity, TV-L1          3.71 .. 7.34 px      0.0491 px                0.07     (none of that size)

No masked bound exceeds twice its clean-clip bound.  The fit sees about a third of the samples it has on a clean clip (68 % are
blocked), all of them in a frame around the subject; the margin sweep (0 / 8 / 16 / 32) is in the profile note.
"""

import json

import numpy as np
import pytest

from tests import estimation_mask_restatement as R
from tests.util import shake_path

pytestmark = pytest.mark.gpu

ARGS = (False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
SUBJECT_SPEED = (5.0, -2.5)     # working px per frame, direction reversed every SUBJECT_RUN pairs so that the subject stays in view
SUBJECT_RUN = 8
SUBJECT_AREA = 0.6              # share of the frame the subject's rectangle covers

# (size, mode) -> centre px
MASKED_BOUNDS = {
    ((960, 540), "translation"): 0.06, ((960, 540), "similarity"): 0.07, ((960, 540), "perspective"): 0.075,
    ((1920, 1080), "translation"): 0.06, ((1920, 1080), "similarity"): 0.07, ((1920, 1080), "perspective"): 0.08,
}
TVL1_BOUND = 0.07


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def subject_clip(n, w, h, mode, device, seed=3):
    """Background: bench.synth_clip under tests.util.shake_path(mode, seed, amp 1).  Subject: a second synth_clip layer
    (seed 99) that translates by SUBJECT_SPEED working px per frame, composited inside a rectangle of SUBJECT_AREA of the
    frame that moves with it.  -> (frames [n,h,w,3] on `device`, masks [n,h,w] float32 0/1 on `device`: the exact
    rectangles, camera path [n,3,3] of the background)."""
    import torch

    import bench

    cam = shake_path(n, w, h, mode, seed=seed, amp=1.0)
    k = max(w, h) / 960.0 if max(w, h) > 960 else 1.0      # full-resolution px per working px
    pos = np.zeros((n, 2))
    for i in range(1, n):
        sign = 1.0 if ((i - 1) // SUBJECT_RUN) % 2 == 0 else -1.0
        pos[i] = pos[i - 1] + sign * np.array(SUBJECT_SPEED) * k
    sub = np.tile(np.eye(3), (n, 1, 1))
    sub[:, 0, 2], sub[:, 1, 2] = pos[:, 0], pos[:, 1]
    frames = bench.synth_clip(n, 0, h, w, device, mats=cam)
    layer = bench.synth_clip(n, 0, h, w, device, seed=99, mats=sub)
    side = np.sqrt(SUBJECT_AREA)
    rw, rh = int(round(w * side)), int(round(h * side))
    masks = torch.zeros((n, h, w), dtype=torch.float32, device=device)
    for i in range(n):
        x0 = int(round((w - rw) / 2 + pos[i, 0] - pos[:, 0].mean()))
        y0 = int(round((h - rh) / 2 + pos[i, 1] - pos[:, 1].mean()))
        x0, y0 = max(0, x0), max(0, y0)
        masks[i, y0:min(h, y0 + rh), x0:min(w, x0 + rw)] = 1.0
    frames = torch.where(masks[..., None] > 0.5, layer, frames)
    return frames, masks, cam


def centre_errors(meta, cam, size, work):
    """Per pair: bench.transition_accuracy's centre error (px at working resolution) of that pair alone."""
    import bench

    mats = [t["matrix"] for t in meta["estimated_motion"]["per_transition"]]
    return np.array([bench.transition_accuracy([mats[i]], cam[i:i + 2], size, work)["centre_px"]["max"] for i in range(len(mats))])


def _stabilize(pkg, ctx, frames, mode, estimator="flow", framing="crop_and_pad", **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, *ARGS, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


# ---- block grid, bit for bit --------------------------------------------------------------------------------------------
def _draw_mask(kind, n, h, w, rng):
    m = np.zeros((n, h, w), np.float32)
    if kind == "full":
        m[:] = 1.0
    elif kind == "rect":
        for f in range(n):
            y0, x0 = rng.integers(0, h - 1), rng.integers(0, w - 1)
            m[f, y0:y0 + rng.integers(1, h), x0:x0 + rng.integers(1, w)] = rng.uniform(0.51, 3.0)
    elif kind == "speckle":
        m[:] = rng.uniform(0.0, 0.5, m.shape)                     # below the threshold everywhere ...
        hit = rng.random(m.shape) < 2e-4
        m[hit] = rng.uniform(0.5000001, 1.0, int(hit.sum()))      # ... but for a few pixels
    elif kind == "nan":
        for f in range(n):
            m[f, rng.integers(0, h), rng.integers(0, w)] = np.nan
            m[f, rng.integers(0, h), rng.integers(0, w)] = np.inf
            m[f, rng.integers(0, h), rng.integers(0, w)] = -np.inf
        m[:, 0, 0] = 0.5                                          # exactly the threshold: not subject
    else:
        assert kind == "empty"
    return m


GRID_CASES = [   # (source w, h), working (w, h) or None
    ((1920, 1080), (960, 540)),     # the flagship: 2x2 footprints
    ((640, 360), None),             # no downscale
    ((540, 960), None),             # portrait, no downscale
    ((1080, 1920), (540, 960)),     # portrait, 2x2
    ((1000, 777), (960, 746)),      # non-integer scale
    ((1283, 721), (960, 540)),      # odd sizes (rows not 16-byte aligned), non-integer scale
    ((333, 187), None),             # odd sizes, no downscale
]


@pytest.mark.parametrize("size,work", GRID_CASES)
def test_block_grid_equals_the_restatement(pkg, ctx, size, work):
    import torch

    w, h = size
    rng = np.random.default_rng(w * 7 + h)
    n = 2
    for kind in ("empty", "full", "rect", "speckle", "nan"):
        for n_masks in (1, n):
            mask = _draw_mask(kind, n_masks, h, w, rng)
            cov = [R.covered(f, work) for f in mask]
            for margin in (0, 1, 16, 64):
                got = ctx.mask_block_grid(torch.from_numpy(mask).cuda(), n, work, 8, margin).cpu().numpy()
                per = [R.blocked_from_covered(c, 8, margin) for c in cov]
                want = np.stack(per * n if n_masks == 1 else per)
                assert got.dtype == np.uint8 and got.shape == want.shape
                assert np.array_equal(got, want), (kind, n_masks, margin, int((got != want).sum()))
    # [H,W] is [1,H,W]
    one = _draw_mask("rect", 1, h, w, rng)
    a = ctx.mask_block_grid(torch.from_numpy(one[0]).cuda(), 3, work, 8, 16)
    b = ctx.mask_block_grid(torch.from_numpy(one).cuda(), 3, work, 8, 16)
    assert torch.equal(a, b) and a.shape[0] == 3


# ---- masked fit -----------------------------------------------------------------------------------------------------------
def _draw_blocked(kind, frames, gh, gw, rng):
    b = np.zeros((frames, gh, gw), np.uint8)
    if kind == "rect":
        for f in range(frames):
            y0, x0 = rng.integers(0, gh // 2), rng.integers(0, gw // 2)
            b[f, y0:y0 + gh // 2, x0:x0 + gw // 2 + f] = 1
    elif kind == "speckle":
        b[:] = rng.random(b.shape) < 0.3
    elif kind == "most":                      # a few dozen admitted samples
        b[:] = 1
        b[:, 2:9, 3:12] = 0
        b[1, 4, 5] = 1
    elif kind == "one_frame":                 # only frame 1 is blocked: pairs 0 and 1 both lose those samples
        b[1, : gh // 2] = 1
    else:
        assert kind == "none"
    return b


@pytest.mark.parametrize("flow_kind", ["clean", "outliers", "nonfinite"])
@pytest.mark.parametrize("mode", ["translation", "similarity", "perspective"])
def test_masked_fit_is_the_fit_on_the_poisoned_grid(pkg, ctx, oracle, mode, flow_kind):
    import torch

    from tests.test_fit_gpu import synth_flow
    from vstab_amd import native

    h, w, step, pairs = 270, 480, 8, 4
    flows = np.stack([synth_flow(h, w, flow_kind, seed) for seed in range(pairs)])
    grid = np.ascontiguousarray(flows[:, ::step, ::step, :])
    gh, gw = grid.shape[1:3]
    rng = np.random.default_rng(5)
    plain = ctx.sample_fit_batch(torch.from_numpy(grid).cuda(), step, mode)
    for kind in ("none", "rect", "speckle", "most", "one_frame"):
        blocked = _draw_blocked(kind, pairs + 1, gh, gw, rng)
        adm = R.admitted(blocked)
        got = ctx.sample_fit_batch(torch.from_numpy(grid).cuda(), step, mode, blocked=torch.from_numpy(blocked).cuda())
        begun = ctx.sample_fit_batch_begin(torch.from_numpy(grid).cuda(), step, mode, blocked=torch.from_numpy(blocked).cuda())
        assert got.tobytes() == ctx.sample_fit_batch_end(begun).tobytes()
        if kind == "none":
            assert got.tobytes() == plain.tobytes()
        poisoned = R.poison(grid, blocked)
        ref_gpu = ctx.sample_fit_batch(torch.from_numpy(poisoned).cuda(), step, mode)
        for name in ("matrix", "accepted", "computed", "residual", "valid_points"):
            assert got[name].tobytes() == ref_gpu[name].tobytes(), (kind, name)
        assert np.array_equal(got["confidence"][:, 1:], ref_gpu["confidence"][:, 1:])          # similarity, perspective
        for p in range(pairs):
            admitted_count = int(adm[p].sum())
            assert (got["total_points"][p] == admitted_count).all()
            nv = int(got["valid_points"][p, 0])
            if got["computed"][p, 0]:
                assert got["confidence"][p, 0] == float(nv) / float(admitted_count)                # float64 division
            # the CPU oracle on the poisoned FIELD (every sample position of the full field carries the grid's value)
            field = flows[p].copy()
            field[::step, ::step] = poisoned[p]
            ref, ref_nv, _ = oracle.fit_all_modes(field, step, mode)
            entry = native.fit_table_to_dicts(got[p:p + 1])[0]
            assert set(entry) == set(ref) and nv == ref_nv, (kind, p)
            for mname, r in ref.items():
                g = entry[mname]
                assert g["accepted"] == r["accepted"] and g["valid_points"] == ref_nv
                if mname != "translation":
                    assert g["confidence"] == r["confidence"]
                if r["accepted"]:
                    if mname == "translation":
                        assert np.array_equal(g["matrix"], r["matrix"])
                    elif mname == "similarity":
                        assert np.allclose(g["matrix"], r["matrix"], rtol=0, atol=1e-6)
                    else:
                        assert np.allclose(g["matrix"], r["matrix"], rtol=2e-5, atol=1e-7)
                    assert g["residual"] == pytest.approx(r["residual"], rel=1e-6)


def test_fewer_than_twelve_admitted_samples_give_the_identity_record(pkg, ctx):
    import torch

    from tests.test_fit_gpu import synth_flow

    grid = np.ascontiguousarray(np.stack([synth_flow(270, 480, "clean", s) for s in range(2)])[:, ::8, ::8, :])
    gh, gw = grid.shape[1:3]
    blocked = np.ones((3, gh, gw), np.uint8)
    blocked[:, 0, :11] = 0                                  # 11 admitted samples in both pairs
    blocked[2, 0, 0] = 1                                    # ... and 10 in the second
    got = ctx.sample_fit_batch(torch.from_numpy(grid).cuda(), 8, "perspective", blocked=torch.from_numpy(blocked).cuda())
    few = np.full_like(grid, np.nan)
    few[:, 0, :11] = grid[:, 0, :11]
    few[1, 0, 0] = np.nan
    ref = ctx.sample_fit_batch(torch.from_numpy(few).cuda(), 8, "perspective")
    for name in ("matrix", "confidence", "residual", "accepted", "computed", "valid_points"):
        assert got[name].tobytes() == ref[name].tobytes(), name
    assert (got["computed"] == 0).all() and (got["accepted"] == 0).all()
    assert (got["matrix"] == np.eye(3, dtype=np.float32).reshape(9)).all()
    assert got["valid_points"][:, 0].tolist() == [11, 10] and got["total_points"][:, 0].tolist() == [11, 10]


# ---- the pipeline ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator,framing,mode", [("flow", "crop_and_pad", "similarity"), ("flow", "crop", "similarity"),
                                                    ("flow", "expand", "perspective"), ("flow_tvl1", "crop_and_pad", "translation")])
def test_all_zero_mask_changes_nothing(pkg, ctx, estimator, framing, mode):
    import torch

    import bench

    n, w, h = (6, 480, 270) if estimator == "flow_tvl1" else (10, 1280, 720)
    frames = bench.synth_clip(n, 0, h, w, torch.device("cuda"), mats=shake_path(n, w, h, mode, seed=4))
    plain = _stabilize(pkg, ctx, frames, mode, estimator, framing)
    none = _stabilize(pkg, ctx, frames, mode, estimator, framing, estimation_mask=None)
    zero = _stabilize(pkg, ctx, frames, mode, estimator, framing, estimation_mask=torch.zeros((n, h, w)))
    for other in (none, zero):
        assert np.array_equal(_bits(plain.frames.cpu().numpy()), _bits(other.frames.cpu().numpy()))
        assert np.array_equal(_bits(plain.masks.cpu().numpy()), _bits(other.masks.cpu().numpy()))
    assert json.dumps(plain.meta, sort_keys=True) == json.dumps(none.meta, sort_keys=True) and "estimation_mask" not in none.meta
    meta = dict(zero.meta)
    block = meta.pop("estimation_mask")
    assert json.dumps(meta, sort_keys=True) == json.dumps(plain.meta, sort_keys=True)
    work = (960, 540) if w > 960 else (w, h)
    samples = -(-work[0] // 8) * -(-work[1] // 8)
    assert block == {"margin": 16, "mask_frames": n, "blocked_fraction_mean": 0.0, "blocked_fraction_max": 0.0,
                     "admitted_points_min": samples}
    assert plain.device_plan == zero.device_plan


def test_mask_shapes_agree_and_the_host_plan_path_agrees(pkg, ctx, monkeypatch):
    """[H,W], [1,H,W] and the same mask N times: one result; device-plan and host-plan path: one result; a host tensor and a
    device tensor: one result."""
    import torch

    n, w, h = 8, 1280, 720
    frames, masks, _ = subject_clip(n, w, h, "similarity", torch.device("cuda"))
    still = masks[0].clone()                       # one mask for the whole clip
    runs = [_stabilize(pkg, ctx, frames, "similarity", estimation_mask=m)
            for m in (still, still[None], still[None].expand(n, h, w).contiguous(), still.cpu(), still[None].cpu().numpy())]
    assert runs[0].device_plan["used"]
    monkeypatch.setenv("VSTAB_DEVICE_PLAN", "0")
    runs.append(_stabilize(pkg, ctx, frames, "similarity", estimation_mask=still))
    assert not runs[-1].device_plan["used"]
    for r in runs[1:]:
        assert np.array_equal(_bits(runs[0].frames.cpu().numpy()), _bits(r.frames.cpu().numpy()))
        assert np.array_equal(_bits(runs[0].masks.cpu().numpy()), _bits(r.masks.cpu().numpy()))
        a, b = dict(runs[0].meta), dict(r.meta)
        assert a.pop("estimation_mask")["mask_frames"] == 1 and b.pop("estimation_mask")["mask_frames"] in (1, n)
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    block = runs[0].meta["estimation_mask"]
    blocked = R.block_grid(still.cpu().numpy(), n, (960, 540), 8, 16)
    frac = 1.0 - R.admitted(blocked).reshape(n - 1, -1).mean(axis=1)
    assert block["blocked_fraction_mean"] == pytest.approx(frac.mean()) and block["blocked_fraction_max"] == pytest.approx(frac.max())
    assert block["admitted_points_min"] == int(R.admitted(blocked).reshape(n - 1, -1).sum(axis=1).min())


def test_value_range_repeat_keeps_the_mask(pkg, ctx):
    """0..255 float input: the estimation is repeated on the rescaled clip (F0) -- with the mask, as the first pass.  The
    result is that of the clip divided by 255 beforehand (IEEE float32 division, done with NumPy here), bit for bit."""
    import torch

    n, w, h = 8, 960, 540
    frames, masks, _ = subject_clip(n, w, h, "translation", torch.device("cuda"))
    big = frames.cpu().numpy() * np.float32(255.0)
    assert big.max() > 1.5
    a = _stabilize(pkg, ctx, torch.from_numpy(big / np.float32(255.0)).cuda(), "translation", estimation_mask=masks)
    b = _stabilize(pkg, ctx, torch.from_numpy(big).cuda(), "translation", estimation_mask=masks)
    assert np.array_equal(_bits(a.frames.cpu().numpy()), _bits(b.frames.cpu().numpy()))
    assert json.dumps(a.meta, sort_keys=True) == json.dumps(b.meta, sort_keys=True) and "estimation_mask" in b.meta
    plain = _stabilize(pkg, ctx, torch.from_numpy(big).cuda(), "translation")
    tp = np.array([t["matrix"] for t in plain.meta["estimated_motion"]["per_transition"]])
    tb = np.array([t["matrix"] for t in b.meta["estimated_motion"]["per_transition"]])
    assert np.abs(tp - tb)[:, :2, 2].max() > 1.0      # the repeat did use the mask: without it the subject is the estimate


def test_node_equals_the_keyword_call(pkg, ctx):
    import torch

    from vstab_amd import nodes

    n, w, h = 8, 960, 540
    frames, masks, _ = subject_clip(n, w, h, "similarity", torch.device("cuda"))
    want = _stabilize(pkg, ctx, frames, "similarity", estimation_mask=masks, mask_margin=8)
    out = nodes.VideoStabilizerFlowMasked.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F",
                                                  masks.cpu(), 8)
    node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
    assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
    assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
    assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True) and node_meta["estimation_mask"]["margin"] == 8


# ---- the purpose ----------------------------------------------------------------------------------------------------------
N_FRAMES = 24


@pytest.mark.parametrize("mode", ["translation", "similarity", "perspective"])
@pytest.mark.parametrize("size", [(960, 540), (1920, 1080)])
def test_subject_is_kept_out_of_the_motion_fit(pkg, ctx, size, mode):
    """The clip of subject_clip: 60 % of the frame is a layer with its own motion.  (a) without the mask every pair's estimate
    is off by more than 1 px; (b) with the exact masks and the default margin every pair is within MASKED_BOUNDS."""
    import torch

    from vstab_amd import host_math as hm

    w, h = size
    frames, masks, cam = subject_clip(N_FRAMES, w, h, mode, torch.device("cuda"))
    work = hm._working_estimation_size(w, h)
    plain = centre_errors(_stabilize(pkg, ctx, frames, mode).meta, cam, size, work)
    res = _stabilize(pkg, ctx, frames, mode, estimation_mask=masks)
    masked = centre_errors(res.meta, cam, size, work)
    print(json.dumps({"case": f"{w}x{h} {mode}", "unmasked_min": float(plain.min()), "unmasked_max": float(plain.max()),
                      "masked_max": float(masked.max()), "block": res.meta["estimation_mask"]}))
    assert plain.shape == masked.shape == (N_FRAMES - 1,)
    assert plain.min() > 1.0, plain
    assert masked.max() <= MASKED_BOUNDS[(size, mode)], masked
    assert [t["mode"] for t in res.meta["estimated_motion"]["per_transition"]] == [mode] * (N_FRAMES - 1)
    assert 0.5 < res.meta["estimation_mask"]["blocked_fraction_mean"] < 0.9


def test_subject_is_kept_out_of_the_motion_fit_tvl1(pkg, ctx):
    import torch

    n, w, h = 6, 480, 270
    frames, masks, cam = subject_clip(n, w, h, "similarity", torch.device("cuda"))
    plain = centre_errors(_stabilize(pkg, ctx, frames, "similarity", "flow_tvl1").meta, cam, (w, h), None)
    res = _stabilize(pkg, ctx, frames, "similarity", "flow_tvl1", estimation_mask=masks)
    masked = centre_errors(res.meta, cam, (w, h), None)
    print(json.dumps({"case": "tvl1 480x270 similarity", "unmasked_min": float(plain.min()), "masked_max": float(masked.max())}))
    assert res.meta["flow_backend"] == "TVL1"
    assert plain.min() > 1.0, plain
    assert masked.max() <= TVL1_BOUND, masked
