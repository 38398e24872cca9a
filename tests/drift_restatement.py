"""NumPy restatement of the drift correction's rule (include/vstab.h, "Drift correction"), written from the rule's text and
from nothing in csrc/: the GPU tests compare `vstab_anchor_sums_batch` with it exactly (all 17 numbers are integers), and the
CPU suite drives drift_correction.py with it in place of the kernel.

Every product and sum of step 1 is one IEEE fp64 operation on arrays (NumPy fuses nothing), in the rule's association:
X = (R0*x + R1*y) + R2, likewise Y; ix = rint(32 X) (ties to even).  Everything behind that is int64."""

import numpy as np

SLOTS = 17


def anchor_sums(template, image, R, cap):
    """One frame: template, image u8 [h,w]; R f64 [6] (anchor pixel -> frame pixel); cap 0..255 -> int64 [17]."""
    T = np.asarray(template)
    I = np.asarray(image)
    assert T.dtype == np.uint8 and I.dtype == np.uint8 and T.shape == I.shape and T.ndim == 2
    assert int(cap) == cap and 0 <= cap <= 255
    h, w = T.shape
    out = np.zeros(SLOTS, np.int64)
    if h < 3 or w < 3:
        return out
    assert max(h, w) <= 1024
    R = np.asarray(R, dtype=np.float64).reshape(6)
    yi, xi = np.mgrid[1:h - 1, 1:w - 1]
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    with np.errstate(all="ignore"):
        X = (R[0] * x + R[1] * y) + R[2]
        Y = (R[3] * x + R[4] * y) + R[5]
        fix = np.rint(32.0 * X)
        fiy = np.rint(32.0 * Y)
        ok = (fix >= 0.0) & (fix <= 32.0 * (w - 1)) & (fiy >= 0.0) & (fiy <= 32.0 * (h - 1))   # False for NaN / inf
    ix = np.where(ok, fix, 0.0).astype(np.int64)
    iy = np.where(ok, fiy, 0.0).astype(np.int64)
    x0, fx = ix >> 5, ix & 31
    y0, fy = iy >> 5, iy & 31
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    Il = I.astype(np.int64)
    v = (32 - fx) * (32 - fy) * Il[y0, x0] + fx * (32 - fy) * Il[y0, x1] + (32 - fx) * fy * Il[y1, x0] + fx * fy * Il[y1, x1]
    Tl = T.astype(np.int64)
    r = v - 1024 * Tl[1:h - 1, 1:w - 1]
    capped = ok & (np.abs(r) > 1024 * int(cap))
    use = ok & ~capped
    gx = Tl[1:h - 1, 2:w] - Tl[1:h - 1, 0:w - 2]
    gy = Tl[2:h, 1:w - 1] - Tl[0:h - 2, 1:w - 1]
    u = 2 * xi.astype(np.int64) - (w - 1)
    q = 2 * yi.astype(np.int64) - (h - 1)
    J = [gx, gy, gx * u + gy * q, gy * u - gx * q]
    out[0] = use.sum()
    out[1] = capped.sum()
    out[2] = np.abs(r)[use].sum()
    for k in range(4):
        out[3 + k] = (J[k] * r)[use].sum()
    slot = 7
    for j in range(4):
        for k in range(j, 4):
            out[slot] = (J[j] * J[k])[use].sum()
            slot += 1
    return out


def anchor_sums_batch(gray, anchor, R, cap):
    """gray u8 [n,h,w], anchor int [n] (-1: none), R f64 [n,6] -> int64 [n,17]."""
    gray = np.asarray(gray)
    anchor = np.asarray(anchor, dtype=np.int64).reshape(-1)
    R = np.asarray(R, dtype=np.float64).reshape(-1, 6)
    assert anchor.shape[0] == gray.shape[0] == R.shape[0]
    out = np.zeros((gray.shape[0], SLOTS), np.int64)
    for i, a in enumerate(anchor.tolist()):
        if a >= 0:
            out[i] = anchor_sums(gray[a], gray[i], R[i], cap)
    return out
