"""NumPy restatement of the spatial fill (include/vstab.h: vstab_spatial_fill_batch), for the tests.

The full pyramid, level by level, in float32 with the operations and the association the header states; no level is
skipped and nothing here imports the package.  NumPy's float32 add / multiply / divide are single IEEE operations, so
the library (built without contraction, with correctly rounded division) has to give the same bits.
"""

from __future__ import annotations

import numpy as np

F32 = np.float32


def holes_of(mask) -> np.ndarray:
    """A pixel is a hole iff !(mask <= 0.5f): above 0.5, or not finite (NaN compares false)."""
    m = np.asarray(mask, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return ~(m <= F32(0.5))


def pull_level(c: np.ndarray, v: np.ndarray):
    """(C_l [h,w,3] f32, V_l [h,w] bool) -> (C_{l+1}, V_{l+1}): taps outside the level or invalid enter as +0.0f."""
    h, w = v.shape
    h2, w2 = (h + 1) >> 1, (w + 1) >> 1
    cp = np.zeros((2 * h2, 2 * w2, 3), dtype=np.float32)
    vp = np.zeros((2 * h2, 2 * w2), dtype=bool)
    cp[:h, :w] = np.where(v[..., None], c, F32(0.0))
    vp[:h, :w] = v
    t00, t01, t10, t11 = cp[0::2, 0::2], cp[0::2, 1::2], cp[1::2, 0::2], cp[1::2, 1::2]
    n = (vp[0::2, 0::2].astype(np.int32) + vp[0::2, 1::2].astype(np.int32) + vp[1::2, 0::2].astype(np.int32)
         + vp[1::2, 1::2].astype(np.int32))
    s = (t00 + t01) + (t10 + t11)
    valid = n > 0
    with np.errstate(all="ignore"):
        q = s / np.maximum(n, 1).astype(np.float32)[..., None]
    return np.where(valid[..., None], q, F32(0.0)).astype(np.float32), valid


def upsample(f: np.ndarray, h: int, w: int) -> np.ndarray:
    """Centre-aligned x2 bilinear upsample of F_{l+1} [hc,wc,3] onto an h x w level: horizontally first, then vertically."""
    hc, wc = f.shape[:2]
    y, x = np.arange(h), np.arange(w)
    yn, xn = y >> 1, x >> 1
    yf = np.clip(np.where(y & 1, yn + 1, yn - 1), 0, hc - 1)
    xf = np.clip(np.where(x & 1, xn + 1, xn - 1), 0, wc - 1)

    def row(r):
        return f[r][:, xn] * F32(0.75) + f[r][:, xf] * F32(0.25)

    return (row(yn) * F32(0.75) + row(yf) * F32(0.25)).astype(np.float32)


def fill_frame(frame, mask):
    """One frame [h,w,3] f32 and its mask [h,w] -> (filled frame, hole_count, fill_count)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    hole = holes_of(mask)
    assert frame.shape[:2] == hole.shape and frame.shape[2] == 3
    hole_count = int(hole.sum())
    cs = [np.where(hole[..., None], F32(0.0), frame).astype(np.float32)]
    vs = [~hole]
    while vs[-1].shape != (1, 1):
        c, v = pull_level(cs[-1], vs[-1])
        cs.append(c)
        vs.append(v)
    if not vs[-1][0, 0]:            # the whole frame is hole: untouched
        return frame.copy(), hole_count, 0
    f = cs[-1]
    for l in range(len(cs) - 2, -1, -1):
        h, w = vs[l].shape
        f = np.where(vs[l][..., None], cs[l], upsample(f, h, w)).astype(np.float32)
    out = frame.copy()
    out[hole] = f[hole]
    return out, hole_count, hole_count


def fill_batch(frames, masks):
    """[n,h,w,3] / [n,h,w] -> (filled [n,h,w,3] f32, hole_count [n] int64, fill_count [n] int64)."""
    frames = np.asarray(frames, dtype=np.float32)
    masks = np.asarray(masks, dtype=np.float32)
    out = np.empty_like(frames)
    holes = np.zeros(len(frames), dtype=np.int64)
    filled = np.zeros(len(frames), dtype=np.int64)
    for i in range(len(frames)):
        out[i], holes[i], filled[i] = fill_frame(frames[i], masks[i])
    return out, holes, filled
