"""GPU parity: vstab_phase_correlate_batch (HIP) vs oracle/vo_phase.c -- the Flow node's fallback estimator
(nodes/video_stabilizer_flow.py:110-130, cv2.phaseCorrelate).

Tolerance: bit-exact against the oracle (same Stockham butterflies, same twiddle table, FMA contraction off, double
products where OpenCV uses them).  Against a real OpenCV: parity unpinned (see oracle/vo_phase.c); the independent
checks below are circular shifts, whose correlation surface is a single peak whatever the DFT rounding.

Against the float64 numpy.fft reference (tests/phase_reference.py, which shares no code with the kernel or the oracle):
the kernel is compared directly, on the cases of tests/phase_cases.py -- every radix mix and stage count up to the
2048-point LDS maximum, sides of 1, padded sizes, peaks whose 5 x 5 window is clamped, the working size -- wherever the
reference says the answer is well defined ((top1 - top2) / top1 >= 1e-3 on its shifted surface, response >= 0.2; asserted
for every case, never used to skip).  Tolerances are 10 x the worst figure measured between the oracle and the reference
on the CPU (tests/test_phase_referee_cpu.py), the kernel being bit-equal to the oracle:
    shift     measured 1.94e-6 px  -> tolerance 1.94e-5 px
    response  measured 2.11e-7     -> tolerance 2.11e-6
The library returns no surface or peak position; a different peak moves the shift by a pixel or more."""

import numpy as np
import pytest

from tests import phase_cases as pc

pytestmark = pytest.mark.gpu


def textured_clip(n, h, w, seed):
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    big = gaussian_filter(rng.uniform(0, 255, (h + 48, w + 48)), 1.5)
    big = (big - big.min()) / (big.max() - big.min()) * 255.0
    frames, oy, ox = [], 24, 24
    for i in range(n):
        if i:
            oy += int(rng.integers(-6, 7))
            ox += int(rng.integers(-6, 7))
            oy, ox = int(np.clip(oy, 0, 48)), int(np.clip(ox, 0, 48))
        frames.append(big[oy:oy + h, ox:ox + w].astype(np.uint8))
    return np.stack(frames)


@pytest.mark.parametrize("n,h,w", [(4, 135, 240), (3, 64, 96), (3, 45, 73), (2, 100, 161), (3, 540, 960), (5, 31, 17), (2, 1, 9)])
def test_phase_matches_oracle(ctx, oracle, n, h, w):
    import torch

    gray = textured_clip(n, h, w, seed=h * 7 + w)
    ref = oracle.phase_correlate_clip(gray)
    table, shifts = ctx.phase_correlate_batch(torch.from_numpy(gray))
    assert shifts.shape == ref.shape == (n - 1, 3)
    assert np.array_equal(shifts, ref), f"max abs diff {np.abs(shifts - ref).max()}"
    # record layout: only the translation row is usable, matrix = [1 0 tx; 0 1 ty; 0 0 1] in float32
    assert (table["computed"][:, 0] == 1).all() and (table["accepted"][:, 0] == 1).all()
    assert (table["computed"][:, 1:] == 0).all() and (table["accepted"][:, 1:] == 0).all()
    mats = table["matrix"][:, 0].reshape(-1, 3, 3)
    assert np.array_equal(mats[:, 0, 2], ref[:, 0].astype(np.float32)) and np.array_equal(mats[:, 1, 2], ref[:, 1].astype(np.float32))
    assert np.array_equal(mats[:, :2, :2], np.broadcast_to(np.eye(2, dtype=np.float32), (n - 1, 2, 2)))
    assert np.array_equal(table["confidence"][:, 0], ref[:, 2]) and (table["residual"] == 0).all()


def test_phase_multi_pass_clip(ctx, oracle, monkeypatch):
    """Long clips are processed in passes that share one frame; VSTAB_PHASE_CHUNK forces 2-pair passes here."""
    import torch

    monkeypatch.setenv("VSTAB_PHASE_CHUNK", "2")
    gray = textured_clip(8, 54, 96, seed=77)
    ref = oracle.phase_correlate_clip(gray)
    _, shifts = ctx.phase_correlate_batch(torch.from_numpy(gray))
    assert np.array_equal(shifts, ref)


def test_phase_flat_frames_are_finite(ctx, oracle):
    """Constant frames: zero spectrum except DC -> the helper's eps keeps everything finite (no NaN path)."""
    import torch

    gray = np.full((3, 40, 60), 128, np.uint8)
    gray[2] = 0
    ref = oracle.phase_correlate_clip(gray)
    _, shifts = ctx.phase_correlate_batch(torch.from_numpy(gray))
    assert np.array_equal(shifts, ref) and np.isfinite(shifts).all()


def test_phase_recovers_circular_shift(ctx):
    """Independent of the oracle: a circular shift of white noise correlates to a single peak."""
    import torch

    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (135, 240), dtype=np.uint8)   # 135 x 240 are optimal DFT sizes: no padding
    moves = [(3, -2), (-7, 5), (0, 11)]
    frames = [base]
    for dx, dy in moves:
        frames.append(np.roll(frames[-1], (dy, dx), axis=(0, 1)))
    _, shifts = ctx.phase_correlate_batch(torch.from_numpy(np.stack(frames)))
    for (dx, dy), row in zip(moves, shifts):
        # odd height: OpenCV measures from rows/2.0 = 67.5 while the shifted origin sits at row 67 -> +0.5
        assert abs(row[0] - dx) < 1e-3 and abs(row[1] - (dy + 0.5)) < 1e-3, (dx, dy, row)
        assert 0.9 < row[2] <= 1.0 + 1e-4   # all energy in the peak window


def _assert_close_to_reference(row, ref, what):
    pc.assert_well_conditioned(ref, what)
    d_shift = max(abs(row[0] - ref.shift[0]), abs(row[1] - ref.shift[1]))
    d_resp = abs(row[2] - ref.shift[2])
    print(f"{what}: shift {d_shift:.3g} px, response {d_resp:.3g}")
    assert d_shift <= pc.SHIFT_TOL, f"{what}: shift off by {d_shift:.3g} px: {tuple(row)} vs reference {ref.shift}"
    assert d_resp <= pc.RESPONSE_TOL, f"{what}: response off by {d_resp:.3g}: {row[2]} vs reference {ref.shift[2]}"


@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_phase_matches_float64_reference(ctx, case_id):
    """The kernel against numpy.fft in float64, not via the oracle (see the module docstring)."""
    import torch

    _, shifts = ctx.phase_correlate_batch(torch.from_numpy(pc.pair(case_id).copy()))
    assert shifts.shape == (1, 3)
    _assert_close_to_reference(shifts[0], pc.reference(case_id), case_id)


def test_phase_chunk_seams_against_reference(ctx, monkeypatch):
    """One pass, 1-pair passes and 3-pair passes (3 + 3 + 1: a last pass shorter than the chunk, frames shared by two
    passes, results written at pair offset p0): every pair against its own reference, and the three runs bit-equal."""
    import torch

    gray = torch.from_numpy(pc.clip("seam-8x54x96").copy())
    refs = pc.clip_references("seam-8x54x96")
    runs = {}
    for chunk in (None, "1", "3"):
        if chunk is None:
            monkeypatch.delenv("VSTAB_PHASE_CHUNK", raising=False)
        else:
            monkeypatch.setenv("VSTAB_PHASE_CHUNK", chunk)
        _, shifts = ctx.phase_correlate_batch(gray)
        assert shifts.shape == (len(refs), 3)
        for i, ref in enumerate(refs):
            _assert_close_to_reference(shifts[i], ref, f"chunk {chunk} pair {i}")
        runs[chunk] = shifts
    assert np.array_equal(runs[None], runs["1"]) and np.array_equal(runs[None], runs["3"])


@pytest.mark.parametrize("clip_id,origin", [("repeat-4x45x73", (0.5, 0.5)), ("repeat-4x64x96", (0.0, 0.0))])
def test_phase_identical_consecutive_frames(ctx, clip_id, origin):
    """Frames 1 and 2 are the same image: P = |F|^2, the surface is a single peak at the origin and the reported shift
    is (N/2.0 - N//2, M/2.0 - M//2) -- 0.5 on an odd (here: padded 73 -> 75) side."""
    import torch

    from tests.phase_reference import optimal_dft_size

    frames = pc.clip(clip_id)
    assert np.array_equal(frames[pc.REPEATED_PAIR], frames[pc.REPEATED_PAIR + 1])
    M, N = optimal_dft_size(frames.shape[1]), optimal_dft_size(frames.shape[2])
    assert origin == (N / 2.0 - N // 2, M / 2.0 - M // 2)
    _, shifts = ctx.phase_correlate_batch(torch.from_numpy(frames.copy()))
    refs = pc.clip_references(clip_id)
    for i, ref in enumerate(refs):
        _assert_close_to_reference(shifts[i], ref, f"{clip_id} pair {i}")
    row = shifts[pc.REPEATED_PAIR]
    assert abs(row[0] - origin[0]) <= pc.SHIFT_TOL and abs(row[1] - origin[1]) <= pc.SHIFT_TOL, tuple(row)


@pytest.mark.parametrize("h,w", [(40, 60), (45, 73), (1, 9)])
def test_phase_all_zero_frames(ctx, h, w):
    """P = 0 everywhere: the surface is 0, the first maximum is raster position (0, 0) of the shifted plane and the
    centroid is 0 / (0 + DBL_EPSILON) = 0.  Outside the conditioning rule on purpose: asserted against these analytic
    values, not against the reference."""
    import torch

    from tests.phase_reference import optimal_dft_size

    M, N = optimal_dft_size(h), optimal_dft_size(w)
    _, shifts = ctx.phase_correlate_batch(torch.zeros((3, h, w), dtype=torch.uint8))
    assert np.array_equal(shifts, np.broadcast_to(np.array([N / 2.0, M / 2.0, 0.0]), (2, 3))), shifts


def test_phase_size_guard(ctx):
    """A padded side of 2048 (the LDS maximum) is accepted; a side that pads beyond it (2049 -> 2160) is refused by the
    library's own check, which names the padded size."""
    import torch
    from vstab_amd import native

    for h, w in [(16, 2048), (2048, 16)]:
        _, shifts = ctx.phase_correlate_batch(torch.zeros((2, h, w), dtype=torch.uint8))
        assert np.array_equal(shifts, [[w / 2.0, h / 2.0, 0.0]])
    with pytest.raises(native.VstabError, match=r"padded size 2160x16 exceeds 2048"):
        ctx.phase_correlate_batch(torch.zeros((2, 16, 2049), dtype=torch.uint8))
    with pytest.raises(native.VstabError, match=r"padded size 16x2160 exceeds 2048"):
        ctx.phase_correlate_batch(torch.zeros((2, 2049, 16), dtype=torch.uint8))
    # the context is usable afterwards
    _, shifts = ctx.phase_correlate_batch(torch.from_numpy(pc.pair("radix-16x2048").copy()))
    _assert_close_to_reference(shifts[0], pc.reference("radix-16x2048"), "radix-16x2048 after a refusal")


def test_phase_rejects_bad_arguments(ctx):
    import torch

    with pytest.raises(ValueError):
        ctx.phase_correlate_batch(torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ctx.phase_correlate_batch(torch.zeros((2, 8, 8), dtype=torch.float32))


def test_flow_node_on_the_fallback_backend(pkg, ctx, oracle, monkeypatch):
    """VSTAB_FLOW_BACKEND=phase_correlate: the Flow pipeline reports the fallback exactly as flow.py:98-107 / 325-330
    would (backend name, reason, every transition a translation) and its frames equal a Motion Apply replay."""
    import torch
    from vstab_amd import apply_pipeline as ap
    from vstab_amd import flow_pipeline as fp
    from vstab_amd import host_math as hm

    monkeypatch.setenv("VSTAB_FLOW_BACKEND", "phase_correlate")
    n, h, w = 6, 96, 128
    rng = np.random.default_rng(11)
    base = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    frames = [base]
    moves = [(2, 1), (-3, 2), (1, -2), (0, 3), (-2, -1)]
    for dx, dy in moves:
        frames.append(np.roll(frames[-1], (dy, dx), axis=(0, 1)))
    frames = np.ascontiguousarray(np.stack(frames))
    res = fp._stabilize_frames(hm._normalize_video_input(frames), "crop_and_pad", "similarity", False, 1.0, 0.5, 0.6,
                               (127, 127, 127), 16.0)
    meta = res.meta
    assert meta["flow_backend"] == "phase_correlate"
    assert meta["flow_fallback_reason"].startswith("DIS unavailable (") and meta["flow_fallback_reason"].endswith("using phase correlation.")
    assert meta["transform_mode_requested"] == "similarity" and meta["transform_mode_applied"] == "translation"
    assert meta["motion_meta"]["source"] == "estimated_flow"
    trans = meta["estimated_motion"]["per_transition"]
    assert len(trans) == n - 1 and all(t["mode"] == "translation" for t in trans)
    mats = np.asarray([t["matrix"] for t in trans], np.float64).reshape(-1, 3, 3)
    for (dx, dy), t, m in zip(moves, trans, mats):
        assert abs(m[0, 2] - dx) < 1e-2 and abs(m[1, 2] - dy) < 1e-2 and np.array_equal(m[:2, :2], np.eye(2))
        assert t["residual"] == 0.0 and t["confidence"] > 0.5
    # the estimator leg against the oracle on the same gray images (no working-size rescale at this size)
    gray = ctx.gray_downscale(torch.from_numpy(frames).to(ctx.device), None).cpu().numpy()
    ref = oracle.phase_correlate_clip(gray)
    assert np.array_equal(mats[:, :2, 2].astype(np.float32), ref[:, :2].astype(np.float32))
    assert [t["confidence"] for t in trans] == ref[:, 2].tolist()
    # KA7: replay through Motion Apply is bit-identical
    replay = ap.apply_motion(hm._normalize_video_input(frames), meta, (127, 127, 127), framing_mode="crop_and_pad")
    assert np.array_equal(replay.frames, res.frames) and np.array_equal(replay.masks, res.masks)


def test_unknown_backend_request_is_an_error(pkg, monkeypatch):
    from vstab_amd import flow_pipeline as fp

    monkeypatch.setenv("VSTAB_FLOW_BACKEND", "TVL1")
    with pytest.raises(ValueError, match="VSTAB_FLOW_BACKEND"):
        fp.resolve_flow_backend("flow")
    assert fp.resolve_flow_backend("classic") == "classic"
