"""NumPy restatement of vstab_mesh_unwarp_batch's rule (include/vstab.h): the plain warp whose output pixel is moved by the
inverse of the mesh displacement, found by a bounded fixed-point iteration, in front of the frame's matrix.  The mesh lookup
and the samplers are tests/mesh_restatement.py's; nothing here imports the package.
"""

from __future__ import annotations

import numpy as np

from tests import mesh_restatement as rs

TOL = 2.0 ** -7          # VSTAB_MESH_UNWARP_TOL
MAX_STEPS = 8            # VSTAB_MESH_UNWARP_MAX_STEPS


def inverse_displacement(xs, ys, offsets, domain_size):
    """The fixed point of the rule at the output pixels (xs, ys) (integer arrays) of a domain_size = (w, h) canvas ->
    (ex, ey fp64: c of the last step taken, unconverged bool, steps int: steps taken per pixel)."""
    px, py = xs.astype(np.float64), ys.astype(np.float64)
    qx, qy = px.copy(), py.copy()
    ex, ey = np.zeros_like(px), np.zeros_like(py)
    done = np.zeros(px.shape, bool)
    steps = np.zeros(px.shape, np.int64)
    with np.errstate(all="ignore"):
        for _ in range(MAX_STEPS):
            live = ~done
            if not live.any():
                break
            cx, cy = rs.displacement(qx, qy, offsets, domain_size)
            nx, ny = px + cx, py + cy
            met = (np.abs(nx - qx) <= TOL) & (np.abs(ny - qy) <= TOL)
            ex, ey = np.where(live, cx, ex), np.where(live, cy, ey)
            qx, qy = np.where(live, nx, qx), np.where(live, ny, qy)
            steps += live
            done |= live & met
    return ex, ey, ~done, steps


def mesh_unwarp_frame(src, matrix, out_size, offsets, border=(0.0, 0.0, 0.0), subpix="q5"):
    """One frame of vstab_mesh_unwarp_batch: src f32 [H,W,3], forward f32 matrix, offsets f32 [mh,mw,2] over the OUTPUT
    canvas -> (dst f32 [h,w,3], mask f32 [h,w], unconverged int)."""
    src = np.asarray(src, dtype=np.float32)
    sh, sw, _ = src.shape
    dw, dh = int(out_size[0]), int(out_size[1])
    border = np.asarray(border, dtype=np.float32).reshape(3)
    m = rs._invert3x3(matrix)
    ys, xs = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    ex, ey, unconverged, _ = inverse_displacement(xs, ys, offsets, (dw, dh))
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
            dst = rs._sample_exact(src, fsx, fsy, border)
        else:
            dst = rs._sample_q5(src, rs._cv_round_clamped(Xd * Wq), rs._cv_round_clamped(Yd * Wq), border)
        nx = np.clip(rs._cv_round_clamped(Xd * Wn), -32768, 32767)
        ny = np.clip(rs._cv_round_clamped(Yd * Wn), -32768, 32767)
    cov = ((nx >= 0) & (nx < sw) & (ny >= 0) & (ny < sh)).astype(np.float32)
    mask = np.float32(1.0) - cov
    mask = np.where(mask < np.float32(1e-3), np.float32(0.0), mask)
    return dst.astype(np.float32), mask.astype(np.float32), int(unconverged.sum())


def mesh_unwarp(src, matrices, out_size, offsets, border=(0.0, 0.0, 0.0), subpix="q5"):
    """-> (dst [N,h,w,3], mask [N,h,w], pad_count int64 [N], unconverged int64 [N])."""
    outs = [mesh_unwarp_frame(src[i], matrices[i], out_size, offsets[i], border, subpix) for i in range(len(src))]
    dst, mask = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return (dst, mask, (mask > 0.5).reshape(len(src), -1).sum(axis=1).astype(np.int64),
            np.array([o[2] for o in outs], np.int64))
