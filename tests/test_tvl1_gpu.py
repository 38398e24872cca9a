"""GPU: vstab_tvl1_flow_batch (HIP, csrc/vstab_tvl1.hip) -- the Flow node's Dual TV-L1 estimator
(nodes/video_stabilizer_flow.py:76-107, cv2.optflow.DualTVL1OpticalFlow_create()).

Tolerance: bit-exact against the NumPy restatement tests/tvl1_restatement.py (dense flow and inner-iteration counts),
which is unpinned against a real OpenCV (see its docstring).  Accuracy against known motion is checked independently of
any restatement.

The cases of tests/tvl1_cases.py take the inner kernel through every rows-per-workgroup choice (8, 4, 2, 1), the row tree
and the row-sum tree across a power of two, last workgroups with fewer rows, the largest level the size guard admits,
every parameter off its default and the content that drives the data-dependent branches; tests/test_tvl1_cases_cpu.py
shows on the CPU that they do.  The scheme itself is refereed on the CPU (tests/test_tvl1_referee_cpu.py: the restatement
against a float64 statement of the published iteration, within 5.4e-5 px after 300 iterations, and against the true
motion of a sub-pixel similarity); since the kernels equal the restatement bit for bit, what the referee shows holds for
them."""

import json

import numpy as np
import pytest

from tests import tvl1_cases as C
from tests import tvl1_restatement as R

pytestmark = pytest.mark.gpu


def textured_clip(n, h, w, seed):
    from scipy.ndimage import gaussian_filter, shift

    rng = np.random.default_rng(seed)
    big = gaussian_filter(rng.uniform(0, 255, (h + 24, w + 24)), 1.5)
    big = (big - big.min()) / (big.max() - big.min()) * 255.0
    frames = []
    for i in range(n):
        dy, dx = (rng.uniform(-1.5, 1.5, 2) if i else (0.0, 0.0))
        moved = shift(big, (dy, dx), order=3, mode="nearest")
        frames.append(np.clip(np.rint(moved[12:12 + h, 12:12 + w]), 0, 255).astype(np.uint8))
    return np.stack(frames)


def _run(ctx, gray, params=None, **kw):
    import torch

    flow, grid, iters = ctx.tvl1_flow_batch(torch.from_numpy(np.array(gray)), params=params, want_full=True, want_grid=True,
                                            want_iterations=True, **kw)
    return flow.cpu().numpy(), grid.cpu().numpy(), iters.cpu().numpy()


# (n, h, w): odd and non-multiple-of-8 sizes; 20x27 stops the pyramid after two scales (16x22, then 13 < 16)
@pytest.mark.parametrize("n,h,w", [(4, 37, 53), (4, 20, 27), (3, 61, 83)])
def test_tvl1_matches_restatement(ctx, n, h, w):
    gray = textured_clip(n, h, w, seed=h * 31 + w)
    flow, grid, iters = _run(ctx, gray)
    ref, counts = R.tvl1_clip(gray)
    assert iters.shape == counts.shape == (n - 1, 5, 5)
    assert np.array_equal(iters, counts), (iters, counts)
    assert np.array_equal(flow, ref), f"max abs diff {np.abs(flow - ref).max()}"
    assert np.array_equal(grid, ref[:, ::8, ::8])
    if h == 20:
        assert (counts[:, 2:] == 0).all() and (counts[:, :2] > 0).all()


def test_tvl1_matches_restatement_at_960x540(ctx):
    """One 960x540 pair with reduced iteration caps (every scale, kernel tiling and row-tree width of the C2 size)."""
    prm = dict(warps=1, outer_iterations=2, inner_iterations=5)
    gray = textured_clip(2, 540, 960, seed=9)
    flow, _, iters = _run(ctx, gray, params=prm)
    ref, counts = R.tvl1_clip(gray, R.params(**prm))
    assert np.array_equal(iters, counts)
    assert np.array_equal(flow, ref), f"max abs diff {np.abs(flow - ref).max()}"


@pytest.mark.parametrize("case_id", C.CASE_IDS)
def test_tvl1_case_matches_restatement(ctx, case_id):
    """Every case of tests/tvl1_cases.py: flow, stride-8 grid and iteration counters bit-equal to the restatement.
    largest-1025x2048 pins the launch that asks for 65 536 B of dynamic LDS beside the kernel's 16 B of static LDS."""
    gray = C.clip(case_id)
    ref, counts = C.restated(case_id)
    flow, grid, iters = _run(ctx, gray, params=C.library_params(case_id) or None)
    assert iters.shape == counts.shape
    assert np.array_equal(iters, counts), (iters, counts)
    assert np.array_equal(flow, ref), f"max abs diff {np.abs(flow - ref).max()}"
    assert np.array_equal(grid, ref[:, ::8, ::8])


def test_tvl1_grid_sampling(ctx):
    """sample_step = 1: the grid is the full flow; a step that divides neither side: ceil(h / step) x ceil(w / step)."""
    ref, _ = C.restated("sum-tree-65x47")
    flow, grid, _ = _run(ctx, C.clip("sum-tree-65x47"), sample_step=1)
    assert np.array_equal(flow, ref) and np.array_equal(grid, ref)
    ref, _ = C.wide_restated()
    _, grid, _ = _run(ctx, C.wide_clip(), sample_step=9)
    assert ref.shape[1] % 9 and ref.shape[2] % 9
    assert grid.shape == (3, 3, 156, 2) and np.array_equal(grid, ref[:, ::9, ::9])


def test_tvl1_batch_invariance_on_the_one_row_path(ctx):
    """Three pairs at 24x1400 (R = 1 at the finest level, R = 2 at the second): one call, one pair per chunk and one
    call per pair give the restatement's bits -- the per-pair buffer index and ticket of the one-row workgroups."""
    gray = C.wide_clip()
    ref, counts = C.wide_restated()
    flow, grid, iters = _run(ctx, gray)
    assert np.array_equal(flow, ref) and np.array_equal(iters, counts) and np.array_equal(grid, ref[:, ::8, ::8])
    f2, g2, i2 = _run(ctx, gray, params={"chunk_pairs": 1})
    assert np.array_equal(f2, flow) and np.array_equal(g2, grid) and np.array_equal(i2, iters)
    for p in range(len(gray) - 1):
        f1, g1, i1 = _run(ctx, gray[p:p + 2])
        assert np.array_equal(f1[0], flow[p]) and np.array_equal(g1[0], grid[p]) and np.array_equal(i1[0], iters[p])


def test_tvl1_batch_and_chunk_invariance(ctx):
    """Pairs are independent: one call over the clip, several forced chunks and one call per pair agree bit for bit."""
    gray = textured_clip(7, 45, 61, seed=4)
    flow, grid, iters = _run(ctx, gray)
    for chunk in (1, 2, 4):
        f2, g2, i2 = _run(ctx, gray, params={"chunk_pairs": chunk, "poll_interval": 3})
        assert np.array_equal(f2, flow) and np.array_equal(g2, grid) and np.array_equal(i2, iters)
    for p in range(len(gray) - 1):
        f1, g1, i1 = _run(ctx, gray[p:p + 2])
        assert np.array_equal(f1[0], flow[p]) and np.array_equal(g1[0], grid[p]) and np.array_equal(i1[0], iters[p])
    # the pairs did converge at different iterations somewhere (the early exit is exercised)
    assert len({tuple(x) for x in iters.reshape(len(iters), -1).tolist()}) > 1


def test_tvl1_state_belongs_to_its_context(ctx):
    """The workspace, the progress word and the launch numbering live in the context: a second context on the same device
    gives the first one's bits, and closing it leaves the first one's state as it was."""
    from vstab_amd import native

    prm = dict(nscales=1, warps=1, outer_iterations=1, inner_iterations=5)
    gray = textured_clip(2, 32, 32, seed=11)
    first = _run(ctx, gray, params=prm)
    other = native.Context()
    try:
        second = _run(other, gray, params=prm)
        assert all(np.array_equal(a, b) for a, b in zip(second, first))
    finally:
        other.close()
    again = _run(ctx, gray, params=prm)
    assert all(np.array_equal(a, b) for a, b in zip(again, first))


def test_tvl1_rejects_what_it_does_not_restate(ctx):
    import torch
    from vstab_amd import native

    gray = torch.from_numpy(textured_clip(3, 32, 40, seed=1))
    with pytest.raises(native.VstabError, match="gamma"):
        ctx.tvl1_flow_batch(gray, params={"gamma": 0.1})
    with pytest.raises(native.VstabError, match="initial flow"):
        ctx.tvl1_flow_batch(gray, params={"use_initial_flow": 1})
    with pytest.raises(ValueError, match="two frames"):
        ctx.tvl1_flow_batch(gray[:1])
    with pytest.raises(ValueError, match="uint8"):
        ctx.tvl1_flow_batch(gray.float())
    with pytest.raises(native.VstabError, match="at least 16x16"):
        ctx.tvl1_flow_batch(torch.zeros((3, 15, 40), dtype=torch.uint8))
    with pytest.raises(native.VstabError, match="at least 16x16"):
        ctx.tvl1_flow_batch(torch.zeros((3, 40, 12), dtype=torch.uint8))
    with pytest.raises(ValueError, match="unknown TV-L1 parameter"):
        ctx.tvl1_flow_batch(gray, params={"lambda": 0.1})
    with pytest.raises(native.VstabError, match="2049x16: at most 2048x2048"):
        ctx.tvl1_flow_batch(torch.zeros((2, 16, 2049), dtype=torch.uint8))
    with pytest.raises(native.VstabError, match="16x2049: at most 2048x2048"):
        ctx.tvl1_flow_batch(torch.zeros((2, 2049, 16), dtype=torch.uint8))
    with pytest.raises(native.VstabError, match="medianFiltering must be 1 .off. or 5, got 3"):
        ctx.tvl1_flow_batch(gray, params={"median_filtering": 3})
    with pytest.raises(native.VstabError, match="nscales must be in .1, 10., got 0"):
        ctx.tvl1_flow_batch(gray, params={"nscales": 0})
    with pytest.raises(native.VstabError, match="scaleStep must be in .0, 1., got 1"):
        ctx.tvl1_flow_batch(gray, params={"scale_step": 1.0})


def _similarity(tx, ty, deg, cx, cy):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    t = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1]], np.float64)
    r = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)
    m = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    return m @ t @ r @ np.linalg.inv(t)


def _analytic_frames(h, w, poses):
    """Frame k shows a smooth analytic texture moved by poses[k] (pixel k(x) = T(poses[k]^-1 x)), float RGB 0..1."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for m in poses:
        inv = np.linalg.inv(m)
        u = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
        v = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
        t = (np.sin(u * 0.071 + 0.3) * np.cos(v * 0.053 - 0.7) + 0.6 * np.sin(u * 0.023 + v * 0.037 + 1.1)
             + 0.5 * np.cos(u * 0.13 - v * 0.09) * np.sin(v * 0.011))
        g = np.clip(0.5 + 0.22 * t, 0, 1).astype(np.float32)
        out.append(np.stack([g, 0.8 * g + 0.1, 1.0 - g], axis=-1))
    return np.ascontiguousarray(np.stack(out))


ACCURACY_PX = 0.1   # max displacement error of a transition over the inner grid (measured on MI355X: 0.067 worst; DIS 0.042)


def test_tvl1_pipeline_recovers_known_motion(pkg, ctx):
    """Known sub-pixel translations and small rotations of a 960x540 clip through the Flow pipeline on TV-L1: every
    estimated transition moves the points of the frame (20 px margin) within ACCURACY_PX of the true motion."""
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    h, w = 540, 960
    steps = [(1.3, -0.6, 0.0), (-2.25, 0.8, 0.15), (0.4, 1.7, -0.2), (-0.9, -1.1, 0.1)]
    poses = [np.eye(3)]
    for tx, ty, deg in steps:
        poses.append(_similarity(tx, ty, deg, w / 2, h / 2) @ poses[-1])
    frames = _analytic_frames(h, w, poses)
    res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", False, 1.0, 0.5, 0.6,
                               (127, 127, 127), 16.0, estimator="flow_tvl1")
    trans = res.meta["estimated_motion"]["per_transition"]
    assert len(trans) == len(steps)
    gy, gx = np.mgrid[20:h - 20:40, 20:w - 20:40].astype(np.float64)
    pts = np.stack([gx.ravel(), gy.ravel(), np.ones(gx.size)])
    worst = []
    for k, t in enumerate(trans):
        est = np.asarray(t["matrix"], np.float64).reshape(3, 3)
        true = poses[k + 1] @ np.linalg.inv(poses[k])
        a, b = est @ pts, true @ pts
        worst.append(float(np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2]).max()))
    assert max(worst) <= ACCURACY_PX, worst


def test_tvl1_estimator_meta_replay_and_shards(pkg, ctx, tmp_path):
    """flow_backend / reason / source of the TV-L1 Flow run, a Motion Apply replay of its meta equal to its frames
    (KA7), and the two-rank sharded run equal to the single process (the harness of test_sharded_gpu.py)."""
    from tests.test_sharded_gpu import _clip, _spawn
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    frames = _clip()
    res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", False, 1.0, 0.5, 0.6,
                               (127, 127, 127), 16.0, estimator="flow_tvl1")
    meta = res.meta
    assert meta["flow_backend"] == "TVL1"
    assert meta["flow_fallback_reason"] == "DIS unavailable (disabled by the caller); using TV-L1."
    assert meta["motion_meta"]["source"] == "estimated_flow"
    assert len(meta["estimated_motion"]["per_transition"]) == len(frames) - 1
    replay = ap.apply_motion(hm._normalize_video_input(frames), meta, (127, 127, 127), framing_mode="crop_and_pad")
    assert np.array_equal(replay.frames, res.frames) and np.array_equal(replay.masks, res.masks)

    _spawn(2, tmp_path, "flow_tvl1")
    ref = fp._stabilize_frames(hm._normalize_video_input(frames), "expand", "similarity", False, 0.7, 0.5, 0.6, (127, 127, 127), 16.0,
                               estimator="flow_tvl1")
    dst = np.concatenate([np.load(tmp_path / f"dst_{r}.npy") for r in range(2)])
    mask = np.concatenate([np.load(tmp_path / f"mask_{r}.npy") for r in range(2)])
    assert np.array_equal(dst, ref.frames) and np.array_equal(mask, ref.masks[..., 0])
    want = json.loads(json.dumps(ref.meta))
    assert want["flow_backend"] == "TVL1"
    for r in range(2):
        assert json.loads((tmp_path / f"meta_{r}.json").read_text()) == want
