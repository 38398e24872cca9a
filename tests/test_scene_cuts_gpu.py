"""Scene cuts on the GPU (include/vstab.h "Scene cuts"; flow_pipeline._stabilize_frames(scene_cuts=...)).

  1. vstab_pair_residual_batch against the NumPy restatement of the rule (tests/scene_cuts_restatement.py): integer equality
  2. detection on analytic two- and three-shot clips equals the construction; single shots and the bench's clip: no cut
  3. every shot of a joined clip is stabilized as if it were alone (estimated_motion bit-equal, warps equal up to the one
     global recentring translation)
  4. it matters: camera-locked PSNR next to the cut, scene-aware vs standalone vs scene_cuts=None
  5. an edit list equal to what "auto" found gives the same result     6. None is the call without the keyword
  7. composition with temporal fill, estimation mask; the sharded refusal     8. the node

The shots: bench.synth_clip (procedural texture, another seed per shot) under tests.util.shake_path (another path seed per
shot), SHOT_FRAMES frames each, joined by concatenation -- the family tools/scene_cuts_accuracy.py calibrates the default
threshold on (profiles/r09_scene_cuts.md).

Measured on an MI355X for test 4 (PSNR in dB over the four frames on either side of the cut, camera_lock, strength 1):
see profiles/r09_scene_cuts.md, "It matters".
"""

import json

import numpy as np
import pytest

from tests import scene_cuts_restatement as R
from tests import util
from tests.util import shake_path

pytestmark = pytest.mark.gpu

ARGS = (False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0)
LOCK_ARGS = (True, 1.0, 0.5, 0.6, (127, 127, 127), 16.0)      # camera_lock + strength 1: the target path is 0
TEXTURE_SEEDS = (1234, 99, 7, 4321)
PATH_SEEDS = (3, 13, 23, 33)
SHOT_FRAMES = 12
PSNR_MARGIN_DB = 1.0
LOCK_WINDOW = 4      # frames on either side of the cut: half of the 9-frame smoothing window of smooth 0.5 at 16 fps


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def shot(k, w, h, mode, amp, device, n=SHOT_FRAMES):
    """Shot k of the family -> (frames [n,h,w,3] on `device`, camera path [n,3,3])."""
    import bench

    cam = shake_path(n, w, h, mode, seed=PATH_SEEDS[k], amp=amp)
    return bench.synth_clip(n, 0, h, w, device, seed=TEXTURE_SEEDS[k], mats=cam), cam


def joined(ks, w, h, mode, amp, device, n=SHOT_FRAMES):
    """-> (frames of the shots ks one after the other, [camera paths], first frames of the shots after the first)."""
    import torch

    parts = [shot(k, w, h, mode, amp, device, n) for k in ks]
    return torch.cat([p[0] for p in parts]), [p[1] for p in parts], [n * i for i in range(1, len(ks))]


def _stabilize(ctx, frames, mode, estimator="flow", framing="crop_and_pad", args=ARGS, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, *args, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


# ---- 1. kernel == restatement, exactly ------------------------------------------------------------------------------------
def _draw_matrices(n_pairs, w, h, rng):
    kinds = ["identity", "translation", "similarity", "perspective", "far", "horizon", "partly", "flip", "minify", "nonfinite"]
    out = []
    for i in range(n_pairs):
        kind = kinds[int(rng.integers(0, len(kinds)))] if i >= len(kinds) or n_pairs < len(kinds) else kinds[i]
        if kind == "partly":          # leaves the frame partly: about half of the width, a third of the height
            m = np.array([[1, 0, rng.uniform(0.3, 0.7) * w], [0, 1, -rng.uniform(0.2, 0.5) * h], [0, 0, 1.0]])
        elif kind == "nonfinite":
            m = np.eye(3)
            m.flat[int(rng.integers(0, 9))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
        else:
            m = util.test_matrices(1, w, h, kind, seed=int(rng.integers(0, 1 << 30)))[0]
        out.append(m)
    return np.stack(out).astype(np.float32)


@pytest.mark.parametrize("h,w", [(37, 53), (270, 480), (540, 960), (33, 64), (5, 7)])
def test_kernel_equals_the_restatement(pkg, ctx, h, w):
    import torch

    rng = np.random.default_rng(h * 1000 + w)
    for n in ((2, 3, 9) if h * w > 200000 else (2, 3, 4, 5, 6, 7, 8, 9)):
        gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        mats = _draw_matrices(n - 1, w, h, rng)
        if n == 3:
            mats[0] = np.eye(3, dtype=np.float32)
            mats[1] = np.array([[1, 0, 2.5], [0, 1, -3.5], [0, 0, 1]], np.float32)     # every coordinate a tie
        want_sum, want_in = R.pair_residual_batch(gray, mats)
        got_sum, got_in = ctx.pair_residual_batch(torch.from_numpy(gray).cuda(), mats)
        assert got_sum.dtype == np.int64 and got_in.dtype == np.int64
        assert got_in.tolist() == want_in.tolist(), (n, mats)
        assert got_sum.tolist() == want_sum.tolist(), (n, mats)
        if n == 3:
            assert got_in[0] == h * w
        # a base address that is not 16-byte aligned takes the byte-load form of the kernel: the same numbers
        flat = torch.empty(n * h * w + 1, dtype=torch.uint8, device="cuda")
        off = flat[1:].view(n, h, w)
        off.copy_(torch.from_numpy(gray))
        again_sum, again_in = ctx.pair_residual_batch(off, mats)
        assert again_sum.tolist() == want_sum.tolist() and again_in.tolist() == want_in.tolist()
    # equal images under the identity: sum 0, inside h*w, for every pair
    same = np.repeat(rng.integers(0, 256, (1, h, w), dtype=np.uint8), 4, axis=0)
    s, i = ctx.pair_residual_batch(torch.from_numpy(same).cuda(), np.tile(np.eye(3, dtype=np.float32), (3, 1, 1)))
    assert s.tolist() == [0, 0, 0] and i.tolist() == [h * w] * 3


def test_kernel_argument_checks(pkg, ctx):
    import torch

    g = torch.zeros((3, 8, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="at least two frames"):
        ctx.pair_residual_batch(g[:1], np.zeros((0, 3, 3), np.float32))
    with pytest.raises(ValueError, match=r"are not \[2,3,3\] for 3 frames"):
        ctx.pair_residual_batch(g, np.tile(np.eye(3, dtype=np.float32), (3, 1, 1)))
    with pytest.raises(ValueError, match="uint8"):
        ctx.pair_residual_batch(g.float(), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)))


# ---- 2. detection ----------------------------------------------------------------------------------------------------------
def _check_detection(ctx, w, h, mode, amp, estimator):
    import torch

    from vstab_amd import scene_cuts as sc

    dev = torch.device("cuda")
    rows = []
    for ks in ((0, 1), (0, 2, 3), (0,)):
        frames, _, cuts = joined(ks, w, h, mode, amp, dev)
        block = _stabilize(ctx, frames, mode, estimator, scene_cuts="auto").meta["scene_cuts"]
        scores = np.array(block["scores"])
        at_cut = [scores[c - 1] for c in cuts]
        inside = np.delete(scores, [c - 1 for c in cuts])
        rows.append({"case": f"{w}x{h} {mode} amp {amp} {estimator} shots {ks}", "within_max": round(float(inside.max()), 3),
                     "across_min": round(float(min(at_cut)), 3) if at_cut else None, "overlap_min": round(float(min(block["overlap"])), 3),
                     "cuts": block["cuts"]})
        print(json.dumps(rows[-1]))
        assert block["cuts"] == cuts, rows[-1]
        assert block["mode"] == "auto" and block["threshold"] == sc.DEFAULT_CUT_THRESHOLD and block["segments"] == len(ks)
        assert len(block["scores"]) == len(block["overlap"]) == len(frames) - 1
        del frames


@pytest.mark.parametrize("amp", [1.0, 3.0])
@pytest.mark.parametrize("mode", ["translation", "similarity", "perspective"])
@pytest.mark.parametrize("size", [(480, 270), (960, 540)])
def test_cuts_are_found_where_the_clip_was_joined(pkg, ctx, size, mode, amp):
    _check_detection(ctx, size[0], size[1], mode, amp, "flow")


@pytest.mark.parametrize("estimator", ["flow_tvl1", "classic"])
def test_cuts_are_found_with_the_other_estimators(pkg, ctx, estimator):
    _check_detection(ctx, 480, 270, "similarity", 1.0, estimator)


def test_no_cut_in_the_bench_clip(pkg, ctx):
    import torch

    import bench

    frames = bench.synth_clip(64, 0, 1080, 1920, torch.device("cuda"))
    block = _stabilize(ctx, frames, "similarity", scene_cuts="auto").meta["scene_cuts"]
    print(json.dumps({"case": "C2 64 frames", "within_max": round(max(block["scores"]), 3), "overlap_min": round(min(block["overlap"]), 3)}))
    assert block["cuts"] == [] and block["segments"] == 1


# ---- 3. each shot is stabilized as if alone ----------------------------------------------------------------------------
def _corners(mats, w, h):
    pts = np.array([[0, 0, 1.0], [w - 1, 0, 1.0], [0, h - 1, 1.0], [w - 1, h - 1, 1.0]]).T
    q = np.asarray(mats, np.float64) @ pts
    return q[:, :2] / q[:, 2:3]             # [n, 2, 4]


@pytest.mark.parametrize("mode", ["similarity", "perspective"])
def test_each_shot_is_stabilized_as_if_alone(pkg, ctx, mode):
    import torch

    w, h = 960, 540
    dev = torch.device("cuda")
    frames, _, cuts = joined((0, 1, 2), w, h, mode, 3.0, dev)
    res = _stabilize(ctx, frames, mode, scene_cuts="auto")
    assert res.meta["scene_cuts"]["cuts"] == cuts and not res.device_plan["used"]
    em = res.meta["estimated_motion"]
    per = em["per_transition"]
    final = np.array([e["applied_matrix"] for e in res.meta["stabilization_warp"]["per_frame"]], np.float32)
    edges = [0] + cuts + [len(frames)]
    for c in cuts:          # the pair across a cut: "no candidate"
        assert per[c - 1] == {"index": c - 1, "mode": "translation", "confidence": 0.0, "residual": 0.0, "matrix": per[c - 1]["matrix"]}
        assert np.allclose(np.array(per[c - 1]["matrix"]), np.eye(3), rtol=0, atol=1e-6)
        assert em["path"][c] == [0.0] * len(em["path"][c])              # every shot's path starts at 0
    for s, e in zip(edges[:-1], edges[1:]):
        alone = _stabilize(ctx, frames[s:e].contiguous(), mode)
        am = alone.meta["estimated_motion"]
        assert em["path"][s:e] == am["path"] and em["target_path"][s:e] == am["target_path"]
        for a, b in zip(per[s:e - 1], am["per_transition"]):
            assert a["index"] == b["index"] + s
            assert (a["mode"], a["confidence"], a["residual"], a["matrix"]) == (b["mode"], b["confidence"], b["residual"], b["matrix"])
        # warps: the joined clip's and the standalone run's differ by the recentring translations only
        t = np.array(res.meta["framing"]["center_offset"]) - np.array(alone.meta["framing"]["center_offset"])
        af = np.array([x["applied_matrix"] for x in alone.meta["stabilization_warp"]["per_frame"]], np.float32)
        d = _corners(final[s:e], w, h) - _corners(af, w, h)
        err = np.abs(d - t[None, :, None]).max()
        print(json.dumps({"case": f"{mode} shot [{s},{e})", "recentring": t.tolist(), "corner_err_px": float(err)}))
        assert err <= 1e-3
    assert res.meta["transform_mode_applied"] == alone.meta["transform_mode_applied"]     # the last segment's


# ---- 4. it matters ---------------------------------------------------------------------------------------------------------
def _locked_sq_error(res, first, count, texture_seed, cam0, device):
    """bench.static_texture_error's truth for one shot of a camera-locked run: output frames [first, first + count) should
    show that shot's frame 0 moved by the run's recentring shift.  -> (sum of squared errors, values) over the pixels that
    none of those frames padded, two pixels in from the padding (as bench.static_texture_error)."""
    import torch

    import bench

    n, h, w, _ = res.frames.shape
    off = res.meta["framing"]["center_offset"]
    shift = np.array([[1, 0, off[0]], [0, 1, off[1]], [0, 0, 1.0]])
    want = bench.synth_clip(1, 0, h, w, device, seed=texture_seed, mats=(shift @ cam0)[None])[0]
    got = res.frames[first:first + count]
    safe = (res.masks.reshape(n, h, w)[first:first + count] == 0).all(dim=0)
    unsafe = torch.nn.functional.max_pool2d((~safe)[None, None].float(), 5, stride=1, padding=2)[0, 0] > 0
    unsafe[:2] = unsafe[-2:] = True
    unsafe[:, :2] = unsafe[:, -2:] = True
    safe = ~unsafe
    sq = ((got - want[None]) ** 2)[:, safe]
    return float(sq.sum().item()), int(sq.numel())


def _psnr(parts):
    total, count = sum(p[0] for p in parts), sum(p[1] for p in parts)
    if count == 0:
        return 0.0          # no pixel that all the frames show: nothing was kept in place
    return float(10 * np.log10(1.0 / max(total / count, 1e-20)))


LOCK_CLIPS = [((960, 540), "similarity", 1.0), ((960, 540), "similarity", 3.0), ((960, 540), "perspective", 3.0),
              ((480, 270), "similarity", 3.0)]


def test_frames_next_to_the_cut_stay_where_they_belong(pkg, ctx):
    """Camera lock next to the cut.  Gate: the scene-aware run's PSNR is within PSNR_MARGIN_DB of the standalone runs' over
    the same frames, on every clip; and on at least one clip scene_cuts=None is worse than scene-aware by more than that."""
    import torch

    dev = torch.device("cuda")
    rows = []
    for (w, h), mode, amp in LOCK_CLIPS:
        frames, cams, cuts = joined((0, 1), w, h, mode, amp, dev)
        c = cuts[0]
        sides = [(c - LOCK_WINDOW, LOCK_WINDOW, 0), (c, LOCK_WINDOW, 1)]      # (first frame, count, shot)
        aware = _stabilize(ctx, frames, mode, args=LOCK_ARGS, scene_cuts="auto")
        assert aware.meta["scene_cuts"]["cuts"] == cuts
        plain = _stabilize(ctx, frames, mode, args=LOCK_ARGS, scene_cuts=None)
        alone = [_stabilize(ctx, frames[:c].contiguous(), mode, args=LOCK_ARGS), _stabilize(ctx, frames[c:].contiguous(), mode, args=LOCK_ARGS)]
        p_aware = _psnr([_locked_sq_error(aware, f, n, TEXTURE_SEEDS[k], cams[k][0], dev) for f, n, k in sides])
        p_plain = _psnr([_locked_sq_error(plain, f, n, TEXTURE_SEEDS[k], cams[k][0], dev) for f, n, k in sides])
        p_alone = _psnr([_locked_sq_error(alone[0], c - LOCK_WINDOW, LOCK_WINDOW, TEXTURE_SEEDS[0], cams[0][0], dev),
                         _locked_sq_error(alone[1], 0, LOCK_WINDOW, TEXTURE_SEEDS[1], cams[1][0], dev)])
        cut_t = plain.meta["estimated_motion"]["per_transition"][c - 1]
        rows.append({"clip": f"{w}x{h} {mode} amp {amp}", "psnr_scene_aware": round(p_aware, 2), "psnr_standalone": round(p_alone, 2),
                     "psnr_none": round(p_plain, 2), "none_cut_pair": {"mode": cut_t["mode"], "confidence": round(cut_t["confidence"], 3)},
                     "none_mode_applied": plain.meta["transform_mode_applied"]})
        print(json.dumps(rows[-1]))
        del frames, aware, plain, alone
    for r in rows:
        assert abs(r["psnr_scene_aware"] - r["psnr_standalone"]) <= PSNR_MARGIN_DB, r
    worse = [r["clip"] for r in rows if r["psnr_none"] < r["psnr_scene_aware"] - PSNR_MARGIN_DB]
    print(json.dumps({"none_worse_by_more_than_the_margin_on": worse}))
    assert worse, rows


# ---- 5. given list == auto; 6. off is off ------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", ["crop_and_pad", "expand", "crop"])
def test_given_list_equals_auto(pkg, ctx, framing):
    import torch

    frames, _, cuts = joined((0, 1, 2), 480, 270, "similarity", 3.0, torch.device("cuda"))
    auto = _stabilize(ctx, frames, "similarity", framing=framing, scene_cuts="auto")
    assert auto.meta["scene_cuts"]["cuts"] == cuts
    given = _stabilize(ctx, frames, "similarity", framing=framing, scene_cuts=list(cuts))
    assert np.array_equal(_bits(auto.frames.cpu().numpy()), _bits(given.frames.cpu().numpy()))
    assert np.array_equal(_bits(auto.masks.cpu().numpy()), _bits(given.masks.cpu().numpy()))
    a, b = dict(auto.meta), dict(given.meta)
    sa, sb = a.pop("scene_cuts"), b.pop("scene_cuts")
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
    assert sb == {"mode": "given", "threshold": None, "cuts": cuts, "segments": 3, "scores": None, "overlap": None}
    assert sa["cuts"] == sb["cuts"] and sa["segments"] == sb["segments"]
    # an empty edit list: one shot, the plain result under another meta block
    none = _stabilize(ctx, frames, "similarity", framing=framing)
    empty = _stabilize(ctx, frames, "similarity", framing=framing, scene_cuts=[])
    assert np.array_equal(_bits(none.frames.cpu().numpy()), _bits(empty.frames.cpu().numpy()))
    e = dict(empty.meta)
    assert e.pop("scene_cuts")["segments"] == 1 and json.dumps(e, sort_keys=True) == json.dumps(none.meta, sort_keys=True)


@pytest.mark.parametrize("estimator,framing,mode", [("flow", "crop_and_pad", "similarity"), ("flow", "crop", "similarity"),
                                                    ("flow", "expand", "perspective"), ("classic", "crop_and_pad", "similarity")])
def test_off_is_off(pkg, ctx, estimator, framing, mode):
    import torch

    frames, _, _ = joined((0, 1), 480, 270, mode, 1.0, torch.device("cuda"))
    ctx.set_timing(True)
    try:
        ctx.pair_residual_batch(torch.zeros((2, 8, 16), dtype=torch.uint8, device="cuda"), np.eye(3, dtype=np.float32)[None])
        before = ctx.kernel_ms_stats("cut")[1]
        plain = _stabilize(ctx, frames, mode, estimator, framing)
        none = _stabilize(ctx, frames, mode, estimator, framing, scene_cuts=None, cut_threshold=None)
        assert ctx.kernel_ms_stats("cut")[1] == before                 # no launch of the residual kernel
        auto = _stabilize(ctx, frames, mode, estimator, framing, scene_cuts="auto")
        assert ctx.kernel_ms_stats("cut")[1] == before + 1             # one launch for the whole clip
    finally:
        ctx.set_timing(False)
    assert np.array_equal(_bits(plain.frames.cpu().numpy()), _bits(none.frames.cpu().numpy()))
    assert np.array_equal(_bits(plain.masks.cpu().numpy()), _bits(none.masks.cpu().numpy()))
    assert json.dumps(plain.meta, sort_keys=True) == json.dumps(none.meta, sort_keys=True) and "scene_cuts" not in none.meta
    assert plain.device_plan == none.device_plan
    assert set(auto.meta) - set(plain.meta) == {"scene_cuts"} and set(plain.meta) <= set(auto.meta)   # the schema is unchanged


# ---- 7. composition --------------------------------------------------------------------------------------------------------
def test_temporal_fill_stays_inside_a_shot(pkg, ctx):
    import torch

    from vstab_amd import temporal_fill as tf

    frames, _, cuts = joined((0, 1), 480, 270, "similarity", 3.0, torch.device("cuda"))
    c, n = cuts[0], len(frames)
    shot_of = np.array([0] * c + [1] * (n - c))
    base = _stabilize(ctx, frames, "similarity", scene_cuts="auto")
    filled = _stabilize(ctx, frames, "similarity", scene_cuts="auto", temporal_fill=4)
    assert filled.meta["scene_cuts"] == base.meta["scene_cuts"] and base.meta["scene_cuts"]["cuts"] == cuts
    assert filled.meta["temporal_fill"]["radius"] == 4 and filled.meta["temporal_fill"]["filled_fraction_max"] > 0.0
    plan = tf.plan_from_meta(base.meta)
    mats, cand = tf.fill_candidates(plan["final_matrices"], plan["transitions"], plan["confidences"], 4)
    for f in range(n):
        offered = cand[f][cand[f] >= 0]
        assert (shot_of[offered] == shot_of[f]).all(), (f, cand[f])
    assert (cand[c - 1, 1::2] == -1).all() and (cand[c, 0::2] == -1).all()       # nothing across the cut, from either side
    dst, mask = base.frames.clone(), base.masks[..., 0].contiguous().clone()
    filled_from, fill_count, _ = ctx.temporal_fill_batch(frames, mats, cand, dst, mask, want_filled_from=True)
    ff = filled_from.cpu().numpy()
    assert int(fill_count.sum()) > 0
    for f in range(n):
        used = np.unique(ff[f][ff[f] >= 0])
        assert (shot_of[cand[f][used]] == shot_of[f]).all(), (f, used)
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(filled.frames.cpu().numpy()))     # the pipeline's fill is this fill


def test_estimation_mask_composes_and_sharding_refuses(pkg, ctx):
    import torch

    from vstab_amd import distributed

    frames, _, cuts = joined((0, 1), 480, 270, "similarity", 1.0, torch.device("cuda"))
    res = _stabilize(ctx, frames, "similarity", scene_cuts="auto", estimation_mask=torch.zeros((270, 480)))
    assert res.meta["scene_cuts"]["cuts"] == cuts and res.meta["estimation_mask"]["blocked_fraction_max"] == 0.0
    plain = _stabilize(ctx, frames, "similarity", scene_cuts="auto")
    assert np.array_equal(_bits(plain.frames.cpu().numpy()), _bits(res.frames.cpu().numpy()))
    with pytest.raises(ValueError, match="scene cuts are not sharded"):
        distributed.stabilize_sharded(ctx, frames, len(frames), "crop_and_pad", "similarity", *ARGS, scene_cuts="auto")


# ---- 8. the node -----------------------------------------------------------------------------------------------------------
def test_node_equals_the_keyword_call_and_replays(pkg, ctx):
    import torch

    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm
    from vstab_amd import nodes
    from vstab_amd import scene_cuts as sc

    frames, _, cuts = joined((0, 1), 480, 270, "similarity", 3.0, torch.device("cuda"))
    want = _stabilize(ctx, frames, "similarity", scene_cuts="auto")
    for threshold in (sc.DEFAULT_CUT_THRESHOLD, 0.0):       # 0 = "use the default"
        out = nodes.VideoStabilizerFlowScenes.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F",
                                                      threshold)
        node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
        assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
        assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
        assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True) and node_meta["scene_cuts"]["cuts"] == cuts
    high = nodes.VideoStabilizerFlowScenes.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6, "#7F7F7F", 250.0)
    assert (high.result if hasattr(high, "result") else high.args)[2]["scene_cuts"]["cuts"] == []
    # KA7: Motion Apply on the node's motion_meta gives the node's frames
    replay = ap.apply_motion(hm._normalize_video_input(frames.cpu().numpy()), node_meta, (127, 127, 127), framing_mode="crop_and_pad")
    assert np.array_equal(replay.frames, want.frames.cpu().numpy()) and np.array_equal(replay.masks, want.masks.cpu().numpy())
