"""NumPy restatement of the estimation mask's rule (include/vstab.h, "Estimation mask"), written from the rule's text and
from nothing in csrc/: the GPU tests compare `vstab_mask_block_grid` with it bit for bit, the CPU suite checks it on
hand-made cases.  Deliberately the literal form: one loop (or one index expression) per rule.

  subject   a full-resolution pixel whose value is > 0.5 or is not finite
  covered   a working pixel (X, Y) with a subject pixel in x in [floor(X*src_w/work_w), ceil((X+1)*src_w/work_w)),
            y likewise (exact integer arithmetic)
  blocked   a grid sample (gx*step, gy*step) with a covered working pixel in |dX| <= margin, |dY| <= margin, clipped
  admitted  a sample of pair (i, i+1) blocked neither in frame i nor in frame i+1
"""

import numpy as np


def subject(mask):
    m = np.asarray(mask, np.float32)
    with np.errstate(invalid="ignore"):
        return (m > np.float32(0.5)) | ~np.isfinite(m)


def covered(mask2d, work_size):
    """mask2d [H,W] -> bool [work_h, work_w]; work_size = (w, h) or None (no downscale)."""
    sub = subject(mask2d)
    sh, sw = sub.shape
    ww, wh = (sw, sh) if work_size is None else (int(work_size[0]), int(work_size[1]))
    X = np.arange(ww, dtype=np.int64)
    x0, x1 = (X * sw) // ww, -((-(X + 1) * sw) // ww)
    out = np.zeros((wh, ww), bool)
    for Y in range(wh):
        y0, y1 = (Y * sh) // wh, -((-(Y + 1) * sh) // wh)
        count = np.concatenate([[0], np.cumsum(sub[y0:y1].any(axis=0))])     # subject columns of the footprint's rows left of x
        out[Y] = count[x1] > count[x0]
    return out


def blocked_from_covered(cov, step, margin):
    wh, ww = cov.shape
    gh, gw = -(-wh // step), -(-ww // step)
    out = np.zeros((gh, gw), np.uint8)
    for gy in range(gh):
        for gx in range(gw):
            Y, X = gy * step, gx * step
            out[gy, gx] = cov[max(0, Y - margin):min(wh, Y + margin + 1), max(0, X - margin):min(ww, X + margin + 1)].any()
    return out


def block_grid(mask, n_frames, work_size, step, margin):
    """mask [N,H,W], [1,H,W] or [H,W] -> uint8 [n_frames, gh, gw]."""
    m = np.asarray(mask, np.float32)
    if m.ndim == 2:
        m = m[None]
    assert m.shape[0] in (1, n_frames)
    per = [blocked_from_covered(covered(f, work_size), step, margin) for f in m]
    return np.stack(per * n_frames if len(per) == 1 else per)


def admitted(blocked):
    """uint8 [N,gh,gw] -> bool [N-1,gh,gw]."""
    b = np.asarray(blocked) != 0
    return ~(b[:-1] | b[1:])


def poison(grid_flow, blocked):
    """The grid [P,gh,gw,2] with NaN written into the samples that are not admitted (a copy)."""
    out = np.array(grid_flow, np.float32, copy=True)
    out[~admitted(blocked)] = np.nan
    return out
