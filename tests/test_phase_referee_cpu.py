"""Independent referee for the phase-correlation estimator (CPU suite): oracle/vo_phase.c against a float64 numpy.fft
reference of the whole operation (tests/phase_reference.py).

The oracle's DFT is a hand-written mixed-radix Stockham transform and csrc/vstab_phase.hip mirrors it butterfly for
butterfly, so the bit-for-bit GPU test cannot see an error the two share: a wrong index or twiddle at one radix
position, a wrong Hermitian extension, a wrong purely-real-bin rule, a wrong window clamp.  The reference shares nothing
with either.  It is compared on tests/phase_cases.py: every radix mix and stage count up to the 2048-point LDS maximum,
sides of 1, padded sizes, peaks whose 5 x 5 window is clamped at a border, the working size, and the clips of the GPU
tests.  tests/test_phase_gpu.py compares the HIP kernel with the same reference on the same cases; if this file is red
and the GPU-vs-oracle test is green, both sides share the bug.

Conditioning: a case is compared only where the reference says the answer is well defined, (top1 - top2) / top1 >= 1e-3
on the shifted float64 surface and response >= 0.2 (the centroid divides by the window sum, which is ~ 0 where the window
covers most of a tiny plane).  This is asserted for every case, never used to skip.

Tolerances are measured (test_measured_figures prints the figures; run with -s).  Worst over all cases and clips:
    shift     1.94e-6 px   (radix-5x1)                  -> tolerance 1.94e-5 px
    response  2.11e-7      (seam-8x54x96, pair 3)       -> tolerance 2.11e-6
    surface   4.50e-6      (padded-textured-45x73,      -> tolerance 4.50e-5
                            relative to the surface maximum)
Tolerance = 10 x measured; the peak position is compared exactly.  A well-conditioned case that needs more than 1e-4 px
is a finding about the kernel, the oracle or the reference, not a tolerance to widen."""

import functools

import numpy as np
import pytest

from tests import phase_cases as pc
from tests.phase_reference import optimal_dft_size, phase_reference


@functools.lru_cache(maxsize=None)
def _figures(oracle, case_id):
    """(shift error px, response error, relative surface error, oracle's peak) of one case."""
    frames, ref = pc.pair(case_id), pc.reference(case_id)
    shifts, surface = oracle.phase_correlate_clip(frames, want_surface=True)
    assert shifts.shape == (1, 3) and surface.shape == ref.surface.shape
    M, N = surface.shape
    shifted = np.roll(surface, (M // 2, N // 2), axis=(0, 1))
    peak = tuple(int(v) for v in np.unravel_index(np.argmax(shifted), shifted.shape))
    d_shift = float(max(abs(shifts[0, 0] - ref.shift[0]), abs(shifts[0, 1] - ref.shift[1])))
    d_resp = float(abs(shifts[0, 2] - ref.shift[2]))
    d_surf = float(np.abs(surface - ref.surface).max() / np.abs(ref.surface).max())
    return d_shift, d_resp, d_surf, peak


@functools.lru_cache(maxsize=None)
def _clip_figures(oracle, clip_id):
    """[(shift error px, response error)] per pair of one clip."""
    shifts = oracle.phase_correlate_clip(pc.clip(clip_id))
    return tuple((float(max(abs(row[0] - ref.shift[0]), abs(row[1] - ref.shift[1]))), float(abs(row[2] - ref.shift[2])))
                 for row, ref in zip(shifts, pc.clip_references(clip_id)))


def test_optimal_dft_size():
    smooth = sorted(2 ** a * 3 ** b * 5 ** c for a in range(13) for b in range(8) for c in range(6))
    for n in list(range(1, 300)) + [511, 960, 1921, 2000, 2001, 2025, 2026, 2048, 2049, 2160, 2161]:
        assert optimal_dft_size(n) == next(v for v in smooth if v >= n), n


def test_optimal_dft_size_of_the_oracle(oracle):
    for n in list(range(1, 300)) + [511, 960, 1921, 2000, 2001, 2025, 2026, 2048, 2049]:
        assert oracle.optimal_dft_size(n) == optimal_dft_size(n), n


def test_reference_on_a_known_surface():
    """The reference against values worked out by hand.  Frame 2 = frame 1 rolled by (dy, dx) on an unpadded 9 x 15 plane
    (odd x odd: DC is the only purely real bin, where C = 1 / P ~ 0): C = exp(2 pi i (ky dy / M + kx dx / N)) elsewhere,
    so the surface is M N at (-dy, -dx) minus 1 everywhere (up to 1 / P(0,0)), the 25-point window sums to M N - 25 and
    its centroid sits on the peak."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (9, 15)).astype(np.uint8)
    ref = phase_reference(a, np.roll(a, (1, -3), axis=(0, 1)))
    assert ref.peak == (9 // 2 - 1, 15 // 2 + 3)
    expect = np.full((9, 15), -1.0)
    expect[-1, 3] += 9 * 15
    assert np.abs(ref.surface - expect).max() < 1e-4
    assert abs(ref.response - (9 * 15 - 25) / (9 * 15)) < 1e-6
    assert abs(ref.shift[0] - (7.5 - 10)) < 1e-6 and abs(ref.shift[1] - (4.5 - 3)) < 1e-6
    assert ref.margin > 1.0 and ref.well_conditioned


@pytest.mark.parametrize("case_id", pc.CASE_IDS)
def test_oracle_matches_reference(oracle, case_id):
    ref = pc.reference(case_id)
    pc.assert_well_conditioned(ref, case_id)
    d_shift, d_resp, d_surf, peak = _figures(oracle, case_id)
    print(f"{case_id}: shift {d_shift:.3g} px, response {d_resp:.3g}, surface {d_surf:.3g}, peak {peak}")
    assert peak == ref.peak
    assert d_shift <= pc.SHIFT_TOL, f"shift off by {d_shift:.3g} px (reference {ref.shift})"
    assert d_resp <= pc.RESPONSE_TOL, f"response off by {d_resp:.3g} (reference {ref.shift[2]})"
    assert d_surf <= pc.SURFACE_TOL, f"surface off by {d_surf:.3g} of its maximum"


@pytest.mark.parametrize("clip_id", pc.CLIP_IDS)
def test_oracle_matches_reference_on_clips(oracle, clip_id):
    """Every pair of the clips that the GPU tests run in several passes / with repeated frames."""
    refs = pc.clip_references(clip_id)
    for i, (ref, (d_shift, d_resp)) in enumerate(zip(refs, _clip_figures(oracle, clip_id))):
        pc.assert_well_conditioned(ref, f"{clip_id} pair {i}")
        print(f"{clip_id} pair {i}: shift {d_shift:.3g} px, response {d_resp:.3g}")
        assert d_shift <= pc.SHIFT_TOL and d_resp <= pc.RESPONSE_TOL, (i, d_shift, d_resp, ref.shift)


def test_measured_figures(oracle):
    """The figures behind the tolerances: worst over every case and clip, printed, and each tolerance is 10 x the
    recorded figure, the recorded figure covers what is measured here, and no shift needs more than 1e-4 px."""
    figures = [_figures(oracle, c) for c in pc.CASE_IDS]
    clips = [f for c in pc.CLIP_IDS for f in _clip_figures(oracle, c)]
    worst_shift = max([f[0] for f in figures] + [f[0] for f in clips])
    worst_resp = max([f[1] for f in figures] + [f[1] for f in clips])
    worst_surf = max(f[2] for f in figures)
    print(f"measured worst: shift {worst_shift:.3e} px, response {worst_resp:.3e}, surface {worst_surf:.3e}")
    assert (pc.SHIFT_TOL, pc.RESPONSE_TOL, pc.SURFACE_TOL) == (10 * pc.MEASURED_SHIFT, 10 * pc.MEASURED_RESPONSE, 10 * pc.MEASURED_SURFACE)
    assert pc.SHIFT_TOL <= 1e-4
    assert worst_shift <= pc.SHIFT_TOL and worst_resp <= pc.RESPONSE_TOL and worst_surf <= pc.SURFACE_TOL
