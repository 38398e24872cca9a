"""NumPy restatement of the scene-cut residual's rule (include/vstab.h, "Scene cuts"), written from the rule's text and from
nothing in csrc/: the GPU tests compare `vstab_pair_residual_batch` with it exactly (both accumulators are integers), the
CPU suite checks it on cases small enough to do by hand.

Every product and sum below is one IEEE fp64 operation on arrays (NumPy fuses nothing), in the rule's association:
X = (A0*x + A1*y) + A2, likewise Y and W; q = rint(X / W), rint(Y / W) (ties to even)."""

import numpy as np


def pair_residual(gray_from, gray_to, matrix):
    """One pair: gray_from, gray_to u8 [h,w]; matrix f32 [3,3] (x_to = A x_from) -> (sum_abs, inside) as Python ints."""
    a = np.asarray(gray_from)
    b = np.asarray(gray_to)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 2
    h, w = a.shape
    A = np.asarray(matrix, dtype=np.float32).reshape(9).astype(np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(all="ignore"):
        X = (A[0] * x + A[1] * y) + A[2]
        Y = (A[3] * x + A[4] * y) + A[5]
        W = (A[6] * x + A[7] * y) + A[8]
        ok = (W > 0.0) & np.isfinite(W)                   # False for NaN
        qx = np.rint(X / W)
        qy = np.rint(Y / W)
        ok &= np.isfinite(qx) & np.isfinite(qy)
        ok &= (qx >= 0.0) & (qx <= w - 1) & (qy >= 0.0) & (qy <= h - 1)
    ix = np.where(ok, qx, 0.0).astype(np.int64)
    iy = np.where(ok, qy, 0.0).astype(np.int64)
    diff = np.abs(a.astype(np.int64) - b[iy, ix].astype(np.int64))
    return int(diff[ok].sum()), int(ok.sum())


def pair_residual_batch(gray, transitions):
    """gray u8 [n,h,w], transitions f32 [n-1,3,3] -> (sum_abs int64 [n-1], inside int64 [n-1])."""
    gray = np.asarray(gray)
    mats = np.asarray(transitions, dtype=np.float32).reshape(-1, 3, 3)
    assert mats.shape[0] == gray.shape[0] - 1
    out = [pair_residual(gray[i], gray[i + 1], mats[i]) for i in range(mats.shape[0])]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64)
