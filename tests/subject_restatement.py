"""NumPy restatement of the subject lock's rule (include/vstab.h, vstab_mask_moments_batch), for the tests.

A pixel is subject iff mask > float32(0.5): a NaN is not (the comparison is false), +inf is.  Per frame: count, the sum of
the subject pixels' x and of their y (int64), and their inclusive bounding box (int32; four -1 without a subject pixel).
Integers, so the kernel must give exactly these.
"""

import numpy as np

# what the GPU tests draw mask values from: both sides of the threshold (0.5 itself is not subject, the next float32 above
# it is), the non-finite values, and mostly background
MASK_VALUES = np.array([0.0, 1.0, 0.5, 0.50000006, np.nan, np.inf, -np.inf, 0.0, 0.0], np.float32)


def subject_of(mask) -> np.ndarray:
    mask = np.asarray(mask, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return mask > np.float32(0.5)


def moments(mask):
    """mask f32 [n,h,w] -> (sums int64 [n,3] = count, sum_x, sum_y;  bbox int32 [n,4] = x0, y0, x1, y1)."""
    mask = np.asarray(mask, dtype=np.float32)
    assert mask.ndim == 3
    n, h, w = mask.shape
    s = subject_of(mask)
    sums = np.zeros((n, 3), np.int64)
    bbox = np.full((n, 4), -1, np.int32)
    cols = s.sum(axis=1, dtype=np.int64)         # [n,w] subject pixels per column
    rows = s.sum(axis=2, dtype=np.int64)         # [n,h] per row
    sums[:, 0] = cols.sum(axis=1)
    sums[:, 1] = (cols * np.arange(w, dtype=np.int64)).sum(axis=1)
    sums[:, 2] = (rows * np.arange(h, dtype=np.int64)).sum(axis=1)
    for k in range(n):
        if sums[k, 0]:
            xs, ys = np.nonzero(cols[k])[0], np.nonzero(rows[k])[0]
            bbox[k] = (xs[0], ys[0], xs[-1], ys[-1])
    return sums, bbox


def disc(h, w, cx, cy, r) -> np.ndarray:
    """A rasterised disc: float32 [h,w], 1 where (x - cx)^2 + (y - cy)^2 <= r^2 (integer centre and radius: symmetric about
    the centre, so its centroid is the centre exactly)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).astype(np.float32)
