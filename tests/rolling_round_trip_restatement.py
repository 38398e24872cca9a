"""NumPy restatement of vstab_rolling_unwarp_batch's rule (include/vstab.h): the plain warp whose output pixel is moved by the
closed-form inverse of the rolling-shutter displacement in front of the frame's matrix.  The forward rule, the analytic camera
and the clip are tests/rolling_shutter_restatement.py's; the way e enters the matrix is tests/mesh_inverse_restatement.py's
(warp_pixel's OUTPUT kind), restated here with the solve in place of the fixed point.  Nothing here imports the package.
"""

from __future__ import annotations

import numpy as np

from tests import mesh_restatement as M
from tests import rolling_shutter_restatement as R

MIN_DET = 0.25           # VSTAB_ROLLING_UNWARP_MIN_DET

displacement = R.displacement                # the forward rule, as it is
rolling_warp = R.rolling_warp
rolling_warp_frame = R.rolling_warp_frame


def inverse_displacement(xs, ys, velocity, readout, out_h):
    """e = q - s of the rule at the output pixels (xs, ys) (arrays of integers, or of float64 positions for the algebra test)
    of a canvas out_h rows high: velocity fp64 [6] -> (ex, ey fp64, unsolved bool); every operation rounded on its own."""
    V = [np.float64(v) for v in np.asarray(velocity, dtype=np.float64).reshape(6)]
    rho, hm1 = np.float64(readout), np.float64(out_h - 1)
    x, y = np.asarray(xs).astype(np.float64), np.asarray(ys).astype(np.float64)
    with np.errstate(all="ignore"):
        tau = rho * (y / hm1 - np.float64(0.5))
        a = np.float64(1.0) + tau * V[0]
        b = tau * V[1]
        c = tau * V[3]
        d = np.float64(1.0) + tau * V[4]
        det = a * d - b * c
        vx = (V[0] * x + V[1] * y) + V[2]
        vy = (V[3] * x + V[4] * y) + V[5]
        rx, ry = tau * vx, tau * vy
        ex = -((d * rx - b * ry) / det)
        ey = -((a * ry - c * rx) / det)
        unsolved = ~(det >= MIN_DET) | ~(np.isfinite(ex) & np.isfinite(ey))
    return np.where(unsolved, 0.0, ex), np.where(unsolved, 0.0, ey), unsolved


def unsolved_case(w, h):
    """A velocity that collapses the lower rows: v0 = v4 = -1.5 and rho = 1 give det = (1 - 1.5 tau)^2, below 0.25 where
    tau > 1/3, the rows with y / (h-1) > 5/6 -> (velocity [1,6], readout, the number of those rows)."""
    vel = np.array([[-1.5, 0.0, 0.75 * (w - 1), 0.0, -1.5, 0.75 * (h - 1)]])       # (the velocity vanishes at the centre)
    rows = int((np.arange(h) / (h - 1.0) > 5.0 / 6.0).sum())
    return vel, 1.0, rows


def rolling_unwarp_frame(src, matrix, out_size, velocity, readout, border=(0.0, 0.0, 0.0), subpix="q5"):
    """One frame of vstab_rolling_unwarp_batch: src f32 [H,W,3], forward f32 matrix, velocity f64 [6] ->
    (dst f32 [h,w,3], mask f32 [h,w], unsolved int)."""
    src = np.asarray(src, dtype=np.float32)
    sh, sw, _ = src.shape
    dw, dh = int(out_size[0]), int(out_size[1])
    border = np.asarray(border, dtype=np.float32).reshape(3)
    m = M._invert3x3(matrix)
    ys, xs = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    ex, ey, unsolved = inverse_displacement(xs, ys, velocity, readout, dh)
    with np.errstate(all="ignore"):
        moved = ~((ex == 0.0) & (ey == 0.0))
        dX, dY, dW = m[0] * ex + m[1] * ey, m[3] * ex + m[4] * ey, m[6] * ex + m[7] * ey
        bh0 = min(16, dh)
        bw0 = min(1024 // bh0, dw)
        xb = np.zeros_like(xs) if bw0 >= dw else (xs // bw0) * bw0
        dxb, dy, dx1 = xb.astype(np.float64), ys.astype(np.float64), (xs - xb).astype(np.float64)
        X0 = m[0] * dxb + m[1] * dy + m[2]
        Y0 = m[3] * dxb + m[4] * dy + m[5]
        W0 = m[6] * dxb + m[7] * dy + m[8]
        Xn, Yn = X0 + m[0] * dx1, Y0 + m[3] * dx1
        Xd, Yd = np.where(moved, Xn + dX, Xn), np.where(moved, Yn + dY, Yn)
        if m[6] == 0.0 and m[7] == 0.0:
            Wq = (np.float64(32.0) / m[8]) if m[8] != 0.0 else np.float64(0.0)
            Wn = (np.float64(1.0) / m[8]) if m[8] != 0.0 else np.float64(0.0)
        else:
            W = W0 + m[6] * dx1
            W = np.where(moved, W + dW, W)
            Wn = np.where(W != 0.0, np.float64(1.0) / np.where(W != 0.0, W, 1.0), 0.0)
            Wq = np.float64(32.0) * Wn
        if subpix == "exact":
            mf = m.astype(np.float32)
            xf, yf = xs.astype(np.float32), ys.astype(np.float32)
            w = xf * mf[6] + yf * mf[7] + mf[8]
            numx = xf * mf[0] + yf * mf[1] + mf[2]
            numy = xf * mf[3] + yf * mf[4] + mf[5]
            w = np.where(moved, w + dW.astype(np.float32), w)
            numx = np.where(moved, numx + dX.astype(np.float32), numx)
            numy = np.where(moved, numy + dY.astype(np.float32), numy)
            fsx, fsy = numx / w, numy / w
            assert fsx.dtype == np.float32
            dst = M._sample_exact(src, fsx, fsy, border)
        else:
            dst = M._sample_q5(src, M._cv_round_clamped(Xd * Wq), M._cv_round_clamped(Yd * Wq), border)
        nx = np.clip(M._cv_round_clamped(Xd * Wn), -32768, 32767)
        ny = np.clip(M._cv_round_clamped(Yd * Wn), -32768, 32767)
    cov = ((nx >= 0) & (nx < sw) & (ny >= 0) & (ny < sh)).astype(np.float32)
    mask = np.float32(1.0) - cov
    mask = np.where(mask < np.float32(1e-3), np.float32(0.0), mask)
    return dst.astype(np.float32), mask.astype(np.float32), int(unsolved.sum())


def rolling_unwarp(src, matrices, out_size, velocity, readout, border=(0.0, 0.0, 0.0), subpix="q5"):
    """-> (dst [N,h,w,3], mask [N,h,w], pad_count int64 [N], unsolved int64 [N])."""
    outs = [rolling_unwarp_frame(src[i], matrices[i], out_size, velocity[i], readout, border, subpix) for i in range(len(src))]
    dst, mask = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return (dst, mask, (mask > 0.5).reshape(len(src), -1).sum(axis=1).astype(np.int64),
            np.array([o[2] for o in outs], np.int64))
