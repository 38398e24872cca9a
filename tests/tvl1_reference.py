"""Float64 NumPy reference of the Dual TV-L1 solve at one scale and one warp, written from the published equations
(Zach, Pock, Bischof, "A duality based approach for realtime TV-L1 optical flow", 2007; Sanchez, Meinhardt-Llopis,
Facciolo, "TV-L1 optical flow estimation", IPOL 2013, algorithm 1), not from tests/tvl1_restatement.py: no float32
rounding, no mimicry of an operation order, no helper shared with the restatement.

For fixed warp products -- the warped gradient (I1wx, I1wy) and rho_c = I1w - I1wx*u0_1 - I1wy*u0_2 - I0 -- one iteration is
    rho   = rho_c + I1wx*u1 + I1wy*u2
    v     = u + TH(u):   TH = +l*t*grad(I1w)           where rho < -l*t*|grad(I1w)|^2
                              -l*t*grad(I1w)           where rho > +l*t*|grad(I1w)|^2
                              -rho*grad(I1w)/|grad(I1w)|^2   otherwise (0 where the gradient vanishes)
    u     = v + theta * div p
    p     = (p + (tau/theta) * grad u) / (1 + (tau/theta) * |grad u|)
with grad the forward difference (0 across the last column / row) and div its negative adjoint: a backward difference
whose first column / row takes p itself and whose last takes -p of the one before.  Every `inner` iterations (the start
of an outer iteration) u is replaced by its 5x5 median, as OpenCV's medianFiltering = 5 does.
"""

import numpy as np


def forward_difference(u):
    ux = np.zeros_like(u)
    uy = np.zeros_like(u)
    ux[:, :-1] = u[:, 1:] - u[:, :-1]
    uy[:-1] = u[1:] - u[:-1]
    return ux, uy


def divergence(px, py):
    """-grad^T: <grad u, p> = -<u, div p> for every p."""
    d = np.zeros_like(px)
    d[:, 0] += px[:, 0]
    d[:, 1:-1] += px[:, 1:-1] - px[:, :-2]
    d[:, -1] += -px[:, -2]
    d[0] += py[0]
    d[1:-1] += py[1:-1] - py[:-2]
    d[-1] += -py[-2]
    return d


def solve(i1wx, i1wy, rho_c, *, lambda_, theta, tau, outer, inner, median=True, snapshots=()):
    """u = 0, p = 0, then outer x inner iterations.  Returns (u1, u2) in float64; with `snapshots` (iteration numbers,
    1-based) a dict {iteration: (u1, u2)} of the state after those iterations instead."""
    from scipy.ndimage import median_filter

    gx = np.asarray(i1wx, np.float64)
    gy = np.asarray(i1wy, np.float64)
    rho_c = np.asarray(rho_c, np.float64)
    g2 = gx * gx + gy * gy
    has_grad = g2 > 0
    inv_g2 = np.where(has_grad, 1.0 / np.where(has_grad, g2, 1.0), 0.0)
    lt = lambda_ * theta
    taut = tau / theta
    u1 = np.zeros_like(gx)
    u2 = np.zeros_like(gx)
    p1x, p1y, p2x, p2y = (np.zeros_like(gx) for _ in range(4))
    kept = {}
    done = 0
    for _ in range(outer):
        if median:
            u1 = median_filter(u1, size=5, mode="nearest")
            u2 = median_filter(u2, size=5, mode="nearest")
        for _ in range(inner):
            rho = rho_c + gx * u1 + gy * u2
            step = np.where(rho < -lt * g2, lt, np.where(rho > lt * g2, -lt, -rho * inv_g2))
            u1 = u1 + step * gx + theta * divergence(p1x, p1y)
            u2 = u2 + step * gy + theta * divergence(p2x, p2y)
            u1x, u1y = forward_difference(u1)
            u2x, u2y = forward_difference(u2)
            n1 = 1.0 + taut * np.hypot(u1x, u1y)
            n2 = 1.0 + taut * np.hypot(u2x, u2y)
            p1x, p1y = (p1x + taut * u1x) / n1, (p1y + taut * u1y) / n1
            p2x, p2y = (p2x + taut * u2x) / n2, (p2y + taut * u2y) / n2
            done += 1
            if done in snapshots:
                kept[done] = (u1.copy(), u2.copy())
    return kept if snapshots else (u1, u2)
