"""Referee of the TV-L1 primal-dual scheme (no GPU): the float32 restatement tests/tvl1_restatement.py, which the HIP
kernels of csrc/vstab_tvl1.hip equal bit for bit (tests/test_tvl1_gpu.py), against

(A) tests/tvl1_reference.py, a float64 statement of the published iteration that shares nothing with the restatement, on
    the solve in isolation: both sides get the same float32 warp products (the bicubic warp has its own referee in
    tests/test_tvl1_cpu.py) and epsilon = 0, so both run exactly the same number of iterations;
(B) the true motion of a known sub-pixel similarity, on a whole pair with default parameters.

The bounds are measured, not chosen: 4 x the worst figure observed on the CPU, the factor absorbing thresholding branches
that flip at a float32 rounding (the step is continuous across the thresholds, so a flip moves u by a rounding, not by a
jump) and another libm behind sqrt / hypot."""

import numpy as np
import pytest

from tests import tvl1_cases as C
from tests import tvl1_reference as ref
from tests import tvl1_restatement as R

F32 = np.float32

# Measured max |restatement - reference| over u1 and u2, in px, after 1 / 10 / 300 iterations (300 = 10 outer x 30 inner,
# a 5x5 median before each outer), defaults lambda 0.15, theta 0.3, tau 0.25, one warp from u = 0 at the finest scale:
#                 1          10         300        (max |u| of the reference after 300)
#   textured   1.19e-7    3.19e-7    1.64e-6       1.86
#   saturated  1.72e-7    9.60e-7    5.35e-5       8.02
#   bars       4.4e-16    1.55e-7    1.40e-5       1.63
# i.e. after 300 iterations the restatement is within 7e-6 of the flow's own magnitude of an exact-arithmetic solve.
MEASURED = {1: 1.72e-7, 10: 9.60e-7, 300: 5.35e-5}
MARGIN = 4.0
SCHEDULE = {1: (1, 1), 10: (1, 10), 300: (10, 30)}   # iterations -> (outer, inner) of the restatement
SOLVE = dict(lambda_=0.15, theta=0.3, tau=0.25)


def _warp_products(i0, i1):
    """The restatement's float32 inputs of the first warp at u = 0: I0, I1, I1wx, I1wy, rho_c."""
    I0, I1 = i0.astype(F32), i1.astype(F32)
    h, w = I0.shape
    I1x, I1y = R.centered_gradient(I1)
    mx = np.arange(w, dtype=F32)[None, :].repeat(h, 0)
    my = np.arange(h, dtype=F32)[:, None].repeat(w, 1)
    I1w, I1wx, I1wy = (R.remap_cubic(img, mx, my) for img in (I1, I1x, I1y))
    return I0, I1, I1wx, I1wy, (I1w - I0).astype(F32)


def _pair(name):
    case_id = {"textured": "param-median-off", "saturated": "content-saturated", "bars": "content-bars"}[name]
    gray = C.clip(case_id)
    return gray[0], gray[1]


@pytest.mark.parametrize("name", ["textured", "saturated", "bars"])
def test_solve_matches_the_float64_reference(name):
    """Figures measured on the CPU: the table above (MEASURED holds each column's worst)."""
    I0, I1, I1wx, I1wy, rho_c = _warp_products(*_pair(name))
    want = ref.solve(I1wx, I1wy, rho_c, outer=10, inner=30, snapshots=tuple(SCHEDULE), **SOLVE)
    for iterations, (outer, inner) in SCHEDULE.items():
        prm = R.params(nscales=1, warps=1, epsilon=0.0, outer_iterations=outer, inner_iterations=inner)
        counts = np.zeros(1, np.int32)
        u1, u2 = R._one_scale(I0, I1, np.zeros(I0.shape, F32), np.zeros(I0.shape, F32), prm, counts)
        assert counts[0] == iterations
        r1, r2 = want[iterations]
        diff = max(np.abs(u1 - r1).max(), np.abs(u2 - r2).max())
        print(f"{name}: after {iterations} iterations max |restatement - reference| = {diff:.3e} px, "
              f"max |u| = {max(np.abs(r1).max(), np.abs(r2).max()):.3f}")
        assert diff <= MARGIN * MEASURED[iterations], (name, iterations, diff)
        assert max(np.abs(r1).max(), np.abs(r2).max()) > 1.0    # a flow to speak of, not a solve that stayed at 0


def test_reference_operators_are_adjoint():
    """The reference's own forward difference and divergence: <grad u, p> = -<u, div p> for arbitrary p."""
    rng = np.random.default_rng(11)
    u, p1, p2 = rng.standard_normal((3, 14, 19))
    ux, uy = ref.forward_difference(u)
    assert abs((ux * p1 + uy * p2).sum() + (u * ref.divergence(p1, p2)).sum()) < 1e-11


def test_reference_decreases_the_energy():
    """The reference is a solver of the TV-L1 energy, not only a twin of the restatement: the relaxed energy
    sum |grad u1| + |grad u2| + lambda |rho(u)| after 300 iterations is far below the one at u = 0."""
    _, _, I1wx, I1wy, rho_c = _warp_products(*_pair("textured"))
    u1, u2 = ref.solve(I1wx, I1wy, rho_c, outer=10, inner=30, **SOLVE)

    def energy(a, b):
        ax, ay = ref.forward_difference(a)
        bx, by = ref.forward_difference(b)
        rho = rho_c.astype(np.float64) + I1wx * a + I1wy * b
        return float((np.hypot(ax, ay) + np.hypot(bx, by)).sum() + SOLVE["lambda_"] * np.abs(rho).sum())

    zero = np.zeros_like(u1)
    assert energy(u1, u2) < 0.5 * energy(zero, zero)


# Measured on the CPU: displacement error of the restated flow against the true motion inside a 10 px margin,
# 72 x 96, translation (0.4, -0.65) px and 0.5 degrees about the centre (true |u| 0.26 .. 1.29 px): max 0.118 px, mean 0.031 px.
SIMILARITY_MAX_PX, SIMILARITY_MEAN_PX = 0.118, 0.031


def test_restatement_recovers_a_subpixel_similarity():
    """Whole pair, default parameters: a smooth analytic texture (test_tvl1_gpu._analytic_frames) moved by a known rotation
    plus translation; the restated flow at every pixel inside a 10 px margin against the true displacement M x - x.
    Measured: max 0.118 px, mean 0.031 px; asserted with the margin of 4."""
    from tests.test_tvl1_gpu import _analytic_frames, _similarity

    h, w = 72, 96
    m = _similarity(0.4, -0.65, 0.5, w / 2, h / 2)
    frames = _analytic_frames(h, w, [np.eye(3), m])
    gray = np.clip(np.rint(frames[..., 0] * 255.0), 0, 255).astype(np.uint8)
    flow, counts = R.tvl1_pair(gray[0], gray[1])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    true_u = m[0, 0] * x + m[0, 1] * y + m[0, 2] - x
    true_v = m[1, 0] * x + m[1, 1] * y + m[1, 2] - y
    err = np.hypot(flow[..., 0] - true_u, flow[..., 1] - true_v)[10:-10, 10:-10]
    print(f"similarity: max error {err.max():.4f} px, mean {err.mean():.4f} px")
    assert np.ptp(true_u) > 0.3 and np.ptp(true_v) > 0.3    # the rotation is visible in the field, not a translation
    assert err.max() <= MARGIN * SIMILARITY_MAX_PX
    assert err.mean() <= MARGIN * SIMILARITY_MEAN_PX
    assert (counts > 0).all()
