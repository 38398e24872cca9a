"""Rolling-shutter refit on the GPU (include/vstab.h "vstab_rectify_samples_batch"; flow_pipeline._stabilize_frames(rolling_refit=True)).

  1. vstab_rectify_samples_batch against the NumPy restatement (tests/rolling_refit_restatement.py): pairs, counts and unsolved in
     bits, at the sizes where the block compaction changes path; readout 0 / zero velocities == p and p + flow in bits
  2. the refit: vstab_points_fit_batch on the kernel's output against the oracle's point fit on the restatement's pairs, compared
     as tests/test_classic_gpu.py compares that entry, and the chain error of the GPU's records against the CPU test's bound
  3. end to end on the analytic rolling clip of tests/test_rolling_shutter_gpu.py (12 frames, 480 x 270, readout 0.7, camera_lock
     and strength 1, so the ideal output is the static texture): (a) the refit helps, (b) the run == the restatement's warp of the
     run's own matrices and velocities, (c) Motion Apply replays it, (d) it composes, (e) "auto" reports the first pass's readout,
     (f) off is off, (g) the node

The figures behind 3 (a) were measured on an MI355X (tools/rolling_refit_report.py, profiles/r26_rolling_refit.md), through the
whole pipeline, over the pixels that all four runs show, 4 px inside:
  similarity   PSNR none 26.81 dB, rolling 30.22 dB, rolling + refit 35.41 dB, twin 35.92 dB: share 0.374 -> 0.945 of the gap
  translation  PSNR none 25.35 dB, rolling 30.61 dB, rolling + refit 31.93 dB, twin 31.81 dB: share 0.814 -> 1.018 (a translation
               cannot hold the path's rotation and scale: its twin is limited by the model, not by the readout)
(a) asserts that the refit is strictly better than the row correction alone and at least half of the measured share -- half,
because it is a quality figure on one synthetic clip, as tests/test_rolling_shutter_gpu.py treats its own.
"""

import json
import math

import numpy as np
import pytest

from tests import rolling_refit_restatement as RF
from tests import rolling_shutter_restatement as R
from tests import util
from tests.rolling_refit_restatement import CHAIN_BOUND, SMALL, analytic_case

pytestmark = pytest.mark.gpu

STEP = 8
RGB = (127, 127, 127)
LOCK_ARGS = (True, 1.0, 0.5, 0.6, RGB, 16.0)        # camera_lock + strength 1: the target path is 0
ARGS = (False, 0.7, 0.5, 0.6, RGB, 16.0)
E2E = dict(n=12, w=480, h=270, rho=0.7, amp=(24.0, 20.0, 0.004, 0.004), omega=0.3, seed=4)
MEASURED_REFIT_SHARE = 0.945                         # similarity mode, measured on an MI355X (see above)
PARENT_SHARE = 0.374                                 # the row correction alone, as recorded before the refit existed


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _stabilize(ctx, frames, mode="similarity", estimator="flow", framing="crop_and_pad", args=LOCK_ARGS, **kw):
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    return fp._stabilize_frames(hm._normalize_video_input(frames), framing, mode, *args, ctx=ctx, keep_on_device=True,
                                estimator=estimator, **kw)


# ---- 1. the kernel == the restatement, in bits ---------------------------------------------------------------------------------
def _kernel_case(w, h, pairs, rho, seed):
    """Noisy flows with a NaN, two infinities and a huge finite value in them; realistic velocities, all-zero ones for frame 0, and for
    one frame a velocity whose det falls below 0.25 on the rows that are read out first; a block grid with every sample of the
    last frame blocked when there are 4 pairs."""
    rng = np.random.default_rng(seed)
    gh, gw = -(-h // STEP), -(-w // STEP)
    flow = (rng.normal(0.0, 3.0, (pairs, gh, gw, 2)) + np.array([4.0, -2.5])).astype(np.float32)
    flow[0, 0, 1, 0] = np.nan
    flow[pairs - 1, gh - 1, gw - 2, 1] = np.inf
    flow[pairs - 1, 0, 3] = (-np.inf, 1.0)
    flow[0, gh - 1, 0, 0] = 3.0e38                            # finite: rectified, and rounds to float32 as it may
    velocity = np.zeros((pairs + 1, 6))
    for i in range(1, pairs + 1):
        th, sc = rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
        velocity[i] = (sc, -th, rng.uniform(-6, 6) - sc * w / 2 + th * h / 2, th, sc, rng.uniform(-4, 4) - th * w / 2 - sc * h / 2)
    folded = 1 if pairs == 1 else 2
    velocity[folded] = (3.0 * np.sign(rho), 0.0, 2.0, 0.0, 0.0, -1.0)      # row 0: tau = -|rho| / 2 * sign, a = 1 - 1.5 |rho| < 0.25
    blocked = (rng.random((pairs + 1, gh, gw)) < 0.3).astype(np.uint8)
    blocked[:, 0, : gw // 2] = 0                                           # some of the folded row stays admitted
    if pairs == 4:
        blocked[pairs] = 1                                                 # the last pair admits nothing
    return flow, velocity, blocked, folded


@pytest.mark.parametrize("pairs", [1, 4])
@pytest.mark.parametrize("w,h", [(61, 45), (64, 64), (960, 16), (1024, 576)])
def test_rectify_equals_the_restatement(pkg, ctx, w, h, pairs):
    import torch

    for rho in (0.7, -1.0):
        flow, velocity, blocked, folded = _kernel_case(w, h, pairs, rho, seed=w + h + pairs)
        cells = flow.shape[1] * flow.shape[2]
        dev_flow = torch.from_numpy(flow).cuda()
        for blk in (None, blocked):
            want, want_cnt, want_uns = RF.rectify_samples(flow, STEP, (w, h), velocity, rho, blk)
            got, got_cnt, got_uns = ctx.rectify_samples_batch(dev_flow, STEP, (w, h), velocity, rho,
                                                              blocked=None if blk is None else torch.from_numpy(blk).cuda())
            assert got.dtype == torch.float32 and tuple(got.shape) == (pairs, cells, 4)
            assert got_cnt.dtype == torch.int32 and tuple(got_cnt.shape) == (pairs,) and tuple(got_uns.shape) == (pairs,)
            assert np.array_equal(got_cnt.cpu().numpy(), want_cnt), (rho, blk is None)
            assert np.array_equal(got_uns.cpu().numpy().view(np.uint32), want_uns), (rho, blk is None)
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (rho, blk is None)
            # the cases are what they claim to be
            touched = [k for k in range(pairs) if k in (folded - 1, folded)]
            for k in range(pairs):
                if blk is not None and pairs == 4 and k == pairs - 1:
                    assert want_cnt[k] == 0 and want_uns[k] == 0 and (_bits(want[k]) == 0x7FC00000).all()
                elif k in touched:
                    assert want_uns[k] > 0, (k, rho)
                else:
                    assert want_uns[k] == 0, (k, rho)
            if blk is None:
                assert (want_cnt == cells).all()
                assert np.isnan(want[0, 1, 2:]).all() and np.isfinite(want[0, 1, :2]).all()        # untracked: prev is written
            else:
                assert 0 < want_cnt[0] < cells


@pytest.mark.parametrize("w,h", [(61, 45), (1024, 576)])
def test_zero_correction_is_the_fits_own_load(pkg, ctx, w, h):
    """Readout 0 or all-zero velocities: prev == p and next == p + flow, in bits."""
    import torch

    pairs = 2
    flow, velocity, _, _ = _kernel_case(w, h, pairs, 0.7, seed=11)
    gh, gw = flow.shape[1:3]
    px = (np.arange(gw) * STEP).astype(np.float32)[None, :].repeat(gh, 0)
    py = (np.arange(gh) * STEP).astype(np.float32)[:, None].repeat(gw, 1)
    want = np.empty((pairs, gh, gw, 4), np.float32)
    want[..., 0], want[..., 1] = px, py
    with np.errstate(all="ignore"):
        want[..., 2], want[..., 3] = px + flow[..., 0], py + flow[..., 1]
    want[~(np.isfinite(want[..., 2]) & np.isfinite(want[..., 3])), 2:] = np.nan
    want = want.reshape(pairs, gh * gw, 4)
    dev_flow = torch.from_numpy(flow).cuda()
    for vel, rho in ((velocity, 0.0), (np.zeros_like(velocity), 0.7), (np.zeros_like(velocity), -1.0)):
        got, cnt, uns = ctx.rectify_samples_batch(dev_flow, STEP, (w, h), vel, rho)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), rho
        assert cnt.cpu().numpy().tolist() == [gh * gw] * pairs and not uns.cpu().numpy().any()


def test_argument_checks(pkg, ctx):
    import torch

    from vstab_amd import native

    g = torch.zeros((2, 5, 8, 2), device="cuda")
    v = np.zeros((3, 6))
    with pytest.raises(ValueError, match="rectify_samples_batch expects a float32"):
        ctx.rectify_samples_batch(g[..., 0], 8, (64, 40), v, 0.5)
    with pytest.raises(ValueError, match="rectify_samples_batch: a grid of 8x5 samples is not a 64x48 image at step 8"):
        ctx.rectify_samples_batch(g, 8, (64, 48), v, 0.5)
    with pytest.raises(ValueError, match=r"rectify_samples_batch: velocity \(2, 6\) is not \[3,6\]"):
        ctx.rectify_samples_batch(g, 8, (64, 40), v[:2], 0.5)
    for bad in (1.5, float("nan")):
        with pytest.raises(ValueError, match=r"rectify_samples_batch: readout=.* outside \[-1, 1\]"):
            ctx.rectify_samples_batch(g, 8, (64, 40), v, bad)
    with pytest.raises(ValueError, match="blocked"):
        ctx.rectify_samples_batch(g, 8, (64, 40), v, 0.5, blocked=torch.zeros((2, 5, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(native.VstabError, match="vstab_rectify_samples_batch: NULL pointer argument"):
        ctx.rectify_samples_batch(g, 8, (64, 40), None, 0.5)
    with pytest.raises(native.VstabError, match="vstab_rectify_samples_batch: .*an image of at least 2 rows"):
        ctx.rectify_samples_batch(torch.zeros((1, 1, 2, 2), device="cuda"), 8, (16, 1), np.zeros((2, 6)), 0.5)
    with pytest.raises(native.VstabError, match="vstab_rectify_samples_batch: 16512 sample points exceed the supported 16384"):
        ctx.rectify_samples_batch(torch.zeros((1, 129, 128, 2), device="cuda"), 8, (1024, 1032), np.zeros((2, 6)), 0.5)
    lib = ctx.lib
    out = torch.zeros((2, 40, 4), device="cuda")
    cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    rc = lib.vstab_rectify_samples_batch(ctx.handle, g.data_ptr(), 2, 5, 8, 8, 40, v.ctypes.data, 1.25, None, out.data_ptr(),
                                         cnt.data_ptr(), cnt.data_ptr())
    assert rc != 0 and b"readout=1.25 outside [-1, 1]" in lib.vstab_last_error()
    rc = lib.vstab_rectify_samples_batch(ctx.handle, g.data_ptr(), 2, 6, 8, 8, 40, v.ctypes.data, 0.5, None, out.data_ptr(),
                                         cnt.data_ptr(), cnt.data_ptr())
    assert rc != 0 and b"6 grid rows are not ceil(40 / 8)" in lib.vstab_last_error()


# ---- 2. the refit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["translation", "similarity"])
def test_refit_matches_the_oracle_and_meets_the_bound(pkg, ctx, oracle, mode):
    import torch

    from vstab_amd import native
    from vstab_amd import rolling_shutter as rs

    size = (SMALL["w"], SMALL["h"])
    flows, truth, _ = analytic_case(SMALL)
    flows[2, 1, 3, 0] = np.nan                                 # one untracked sample
    dev_flow = torch.from_numpy(flows).cuda()
    first = ctx.sample_fit_batch(dev_flow, STEP, mode)
    names = ("translation", "similarity")
    first_mats = first[:, names.index(mode)]["matrix"].reshape(-1, 3, 3).astype(np.float64)
    assert first[:, names.index(mode)]["accepted"].all()
    velocity = rs.velocities(first_mats, np.ones(len(first_mats)), None)
    got_pairs, got_cnt, got_uns = ctx.rectify_samples_batch(dev_flow, STEP, size, velocity, SMALL["rho"])
    want_pairs, want_cnt, want_uns = RF.rectify_samples(flows, STEP, size, velocity, SMALL["rho"])
    assert np.array_equal(_bits(got_pairs.cpu().numpy()), _bits(want_pairs)) and not want_uns.any()
    got = native.fit_table_to_dicts(ctx.points_fit_batch(got_pairs, got_cnt, mode))
    refit = []
    for k in range(len(flows)):
        rows = want_pairs[k, : want_cnt[k]]
        status = np.isfinite(rows[:, 2:]).all(axis=1).astype(np.uint8)
        ref, nv = oracle.fit_all_modes_points(rows[:, :2], np.nan_to_num(rows[:, 2:]), status, mode)
        assert set(got[k]) == set(ref) and mode in ref, (k, set(got[k]), set(ref))
        assert nv == (47 if k == 2 else 48)
        for name, r in ref.items():
            g = got[k][name]
            assert g["valid_points"] == nv and g["total_points"] == 48                 # the admitted count
            assert g["accepted"] == r["accepted"] and g["confidence"] == r["confidence"], (k, name)
            assert r["accepted"]
            if name == "translation":
                assert np.array_equal(g["matrix"], r["matrix"])
            else:
                assert np.allclose(g["matrix"], r["matrix"], rtol=0, atol=2e-6)
        refit.append(got[k][mode]["matrix"].astype(np.float64))
    if mode == "similarity":
        _, chain0 = RF.corner_errors(first_mats, truth, size)
        _, chain1 = RF.corner_errors(refit, truth, size)
        print(f"\nrolling_refit 61 x 45 on the GPU: chain {chain0:.3f} -> {chain1:.3f} px ({chain1 / chain0:.3f} x)")
        assert chain1 <= CHAIN_BOUND["small"] * chain0, (chain0, chain1)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def _final_matrices(meta):
    return np.array([e["applied_matrix"] for e in meta["stabilization_warp"]["per_frame"]], np.float32)


def _interior(masks, radius):
    import torch.nn.functional as F

    k = 2 * radius + 1
    padded = F.pad((masks > 0).float()[:, None], (radius,) * 4, value=1.0)
    return F.max_pool2d(padded, k, stride=1)[:, 0] == 0


def _static_ideal(final0, h, w, device, seed=1234):
    """The locked camera shows frame 0's content -- the texture itself -- moved by frame 0's matrix (the recentring shift)."""
    import torch

    from tests import mesh_restatement as M

    assert np.array_equal(final0[:2, :2], np.eye(2, dtype=np.float32)) and np.array_equal(final0[2], np.float32([0, 0, 1]))
    yy, xx = torch.meshgrid(torch.arange(h, device=device, dtype=torch.float32), torch.arange(w, device=device, dtype=torch.float32),
                            indexing="ij")
    return M.texture(xx - float(final0[0, 2]), yy - float(final0[1, 2]), h, w, seed)


def psnr_of_runs(runs, h, w, device):
    """runs: results of _stabilize -> the PSNR of each against the static texture over the pixels ALL of them show, 4 px inside."""
    import torch

    worst = runs[0].masks[..., 0]
    for r in runs[1:]:
        worst = torch.maximum(worst, r.masks[..., 0])
    sel = _interior(worst, 4)
    assert float(sel.float().mean()) > 0.5
    out = []
    for r in runs:
        err = ((r.frames - _static_ideal(_final_matrices(r.meta)[0], h, w, device)) ** 2).sum(-1)[sel]
        out.append(10.0 * math.log10(1.0 / (float(err.mean()) / 3.0)))
    return out


@pytest.fixture(scope="module")
def clip(pkg, ctx):
    """The analytic rolling clip, its global-shutter twin and the four similarity runs; shared, never changed."""
    import torch

    dev = torch.device("cuda")
    path = R.CameraPath(E2E["w"], E2E["h"], amp=E2E["amp"], omega=E2E["omega"], seed=E2E["seed"])
    assert max(path.corner_skew(i, E2E["rho"]) for i in range(E2E["n"])) >= 2.0
    frames = R.rolling_clip(path, E2E["n"], E2E["rho"], dev)
    twin = R.rolling_clip(path, E2E["n"], 0.0, dev)
    return {"frames": frames, "none": _stabilize(ctx, frames), "rolling": _stabilize(ctx, frames, rolling_shutter=E2E["rho"]),
            "refit": _stabilize(ctx, frames, rolling_shutter=E2E["rho"], rolling_refit=True), "twin": _stabilize(ctx, twin)}


def test_the_refit_helps(pkg, ctx, clip):
    import torch

    n, w, h = E2E["n"], E2E["w"], E2E["h"]
    p_none, p_roll, p_refit, p_twin = psnr_of_runs([clip[k] for k in ("none", "rolling", "refit", "twin")], h, w, torch.device("cuda"))
    share_roll, share_refit = (p_roll - p_none) / (p_twin - p_none), (p_refit - p_none) / (p_twin - p_none)
    block = clip["refit"].meta["rolling_shutter"]
    print(f"\nrolling_refit similarity: PSNR none {p_none:.2f} dB, rolling {p_roll:.2f} dB, rolling + refit {p_refit:.2f} dB, twin "
          f"{p_twin:.2f} dB; share {share_roll:.3f} -> {share_refit:.3f}; refit {json.dumps(block['refit'])}")
    assert p_refit > p_roll > p_none
    assert share_refit >= 0.5 * MEASURED_REFIT_SHARE, (p_none, p_roll, p_refit, p_twin)
    assert share_refit > PARENT_SHARE
    # the meta: the block of the row correction plus "refit"; nothing else is new
    assert set(clip["refit"].meta) == set(clip["rolling"].meta)
    assert set(block) - set(clip["rolling"].meta["rolling_shutter"]) == {"refit"} and block["version"] == 1
    refit = block["refit"]
    assert refit["passes"] == 1 and refit["pairs_refit"] == n - 1 and refit["samples_unsolved_max"] == 0
    assert 0.0 < refit["transition_change_px_mean"] <= refit["transition_change_px_max"] < 4.0
    assert block["readout"] == E2E["rho"] and block["source"] == "given"
    assert not np.array_equal(_final_matrices(clip["refit"].meta), _final_matrices(clip["rolling"].meta))
    assert block["velocity"] != clip["rolling"].meta["rolling_shutter"]["velocity"]
    json.loads(json.dumps(clip["refit"].meta))


def test_the_run_is_the_restatements_warp_of_its_own_plan(pkg, ctx, clip):
    run = clip["refit"]
    w, h = E2E["w"], E2E["h"]
    block = run.meta["rolling_shutter"]
    velocity = np.array(block["velocity"], np.float64)
    want, want_mask, want_cnt = R.rolling_warp(clip["frames"].cpu().numpy(), _final_matrices(run.meta), (w, h), velocity, E2E["rho"],
                                               np.float32(RGB) / np.float32(255.0))
    assert np.array_equal(_bits(run.frames.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(run.masks[..., 0].cpu().numpy()), _bits(want_mask))
    assert run.meta["padding_fraction_max"] == float((want_cnt.astype(np.float32) / np.float32(w * h)).astype(np.float64).max())
    # the velocities are those of the meta's own (second-plan) transitions
    from vstab_amd import rolling_shutter as rs

    em = run.meta["estimated_motion"]["per_transition"]
    again = rs.velocities(np.array([t["matrix"] for t in em], np.float32), [t["confidence"] for t in em], None)
    assert np.array_equal(again, velocity)


def test_motion_apply_replays_the_run(pkg, ctx, clip):
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import host_math as hm

    run = clip["refit"]
    meta = json.loads(json.dumps(run.meta))                    # what a saved workflow hands on
    got = ap.apply_motion(hm._normalize_video_input(clip["frames"]), meta, RGB, ctx=ctx, keep_on_device=True,
                          framing_mode="crop_and_pad", rolling=True)
    assert got.meta["motion_apply"]["rolling_shutter"] == {"direction": "forward", "readout": E2E["rho"], "unsolved_max": 0}
    assert _same(got.frames, run.frames) and _same(got.masks, run.masks)


def test_auto_reports_the_first_pass_readout(pkg, ctx, clip):
    auto = _stabilize(ctx, clip["frames"], rolling_shutter="auto")
    both = _stabilize(ctx, clip["frames"], rolling_shutter="auto", rolling_refit=True)
    a, b = auto.meta["rolling_shutter"], both.meta["rolling_shutter"]
    assert b["source"] == "estimated" and b["readout"] == a["readout"] and b["estimate"] == a["estimate"]
    assert b["refit"]["passes"] == 1 and b["velocity"] != a["velocity"]


def test_it_composes(pkg, ctx, clip):
    import torch

    frames = clip["frames"][:8]
    mask = torch.zeros((E2E["h"], E2E["w"]))
    mask[100:170, 200:300] = 1.0
    res = _stabilize(ctx, frames, estimation_mask=mask, rolling_shutter=0.7, rolling_refit=True, framing="expand", scene_cuts=[4],
                     spatial_fill=True, stability_report=True, mask_grow=3)
    block = res.meta["rolling_shutter"]
    assert res.meta["estimation_mask"]["blocked_fraction_max"] > 0.0 and res.meta["scene_cuts"]["cuts"] == [4]
    assert "spatial_fill" in res.meta and "stability" in res.meta and "mask_handoff" in res.meta
    assert block["refit"]["passes"] == 1 and block["refit"]["pairs_refit"] == 6             # 7 pairs, one across the cut
    cut = res.meta["estimated_motion"]["per_transition"][3]
    assert cut["confidence"] == 0.0 and np.array_equal(np.array(cut["matrix"]), np.eye(3))
    # the table the meta's counts describe is the refit's: admitted samples, as in the masked grid fit
    plain = _stabilize(ctx, frames, estimation_mask=mask, rolling_shutter=0.7, framing="expand", scene_cuts=[4])
    assert res.meta["estimation_mask"] == plain.meta["estimation_mask"]
    tvl1 = _stabilize(ctx, frames[:4, ::2, ::2].contiguous(), "translation", "flow_tvl1", rolling_shutter=0.5, rolling_refit=True)
    assert tvl1.meta["rolling_shutter"]["refit"]["passes"] == 1


@pytest.mark.parametrize("estimator", ["flow", "flow_tvl1"])
def test_off_is_off(pkg, ctx, estimator):
    """None and False are the call that does not know the keyword: frames, mask and meta byte for byte, no rectifier launch."""
    import bench
    import torch

    n, w, h = (12, 480, 270) if estimator == "flow" else (6, 240, 136)
    frames = bench.synth_clip(n, 0, h, w, torch.device("cuda"), mats=util.shake_path(n, w, h, "similarity", seed=3))
    ctx.set_timing(True)
    try:
        ctx.rectify_samples_batch(torch.zeros((1, 2, 2, 2), device="cuda"), 8, (16, 16), np.zeros((2, 6)), 0.5)   # the kind exists
        assert ctx.kernel_ms_stats("rectify")[1] == 1
        ctx.set_timing(True)                                   # clears the totals
        for kw in ({}, dict(rolling_shutter=0.6), dict(rolling_shutter="auto")):
            plain = _stabilize(ctx, frames, "similarity", estimator, args=ARGS, **kw)
            for off in (None, False):
                got = _stabilize(ctx, frames, "similarity", estimator, args=ARGS, rolling_refit=off, **kw)
                assert _same(plain.frames, got.frames) and _same(plain.masks, got.masks)
                assert json.dumps(plain.meta) == json.dumps(got.meta)
                assert plain.device_plan == got.device_plan
                assert "refit" not in got.meta.get("rolling_shutter", {})
        assert ctx.kernel_ms_stats("rectify")[1] == 0
        on = _stabilize(ctx, frames, "similarity", estimator, args=ARGS, rolling_shutter=0.6, rolling_refit=True)
        assert ctx.kernel_ms_stats("rectify")[1] == 1 and on.meta["rolling_shutter"]["refit"]["passes"] == 1
    finally:
        ctx.set_timing(False)


def test_node_equals_the_keyword_call(pkg, ctx, clip):
    from vstab_amd import nodes

    frames = clip["frames"][:8]
    for readout, refit, kw in ((0.7, True, dict(rolling_shutter=0.7, rolling_refit=True)), (0.0, True, dict(rolling_shutter="auto", rolling_refit=True)),
                               (0.7, False, dict(rolling_shutter=0.7))):
        want = _stabilize(ctx, frames, args=ARGS, **kw)
        out = nodes.VideoStabilizerFlowRollingRefit.execute(frames.cpu(), 16.0, "crop_and_pad", "similarity", False, 0.7, 0.5, 0.6,
                                                            "#7F7F7F", readout, refit)
        node_frames, node_mask, node_meta = out.result if hasattr(out, "result") else out.args
        assert np.array_equal(_bits(node_frames.cpu().numpy()), _bits(want.frames.cpu().numpy()))
        assert np.array_equal(_bits(node_mask.cpu().numpy()), _bits(want.masks[..., 0].cpu().numpy()))
        assert json.dumps(node_meta, sort_keys=True) == json.dumps(want.meta, sort_keys=True)
        assert ("refit" in node_meta["rolling_shutter"]) == refit
