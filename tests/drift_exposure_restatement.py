"""NumPy restatement of the exposure-matched, masked drift-correction rule (include/vstab.h, "Drift correction", the second
form), written from the rule's text and from nothing in csrc/: the GPU tests compare `vstab_anchor_sums_ex_batch` with it
exactly (all 31 numbers are integers), and the CPU suite drives drift_correction.py with it in place of the kernel.

Step 1 is IEEE fp64 on arrays in the rule's association (NumPy fuses nothing); everything behind the rounding is int64."""

import numpy as np

SLOTS = 31
# where the 17 numbers of the plain rule sit among the 31: count, capped, sum|r|, b0..b3, and H's 4x4 corner
H_INDEX = {}
_slot = 10
for _j in range(6):
    for _k in range(_j, 6):
        H_INDEX[(_j, _k)] = _slot
        _slot += 1
OLD_SLOTS = [0, 1, 3, 4, 5, 6, 7] + [H_INDEX[(j, k)] for j in range(4) for k in range(j, 4)]


def anchor_sums_ex(template, image, R, cap, gain=1024, offset=0, blocked_t=None, blocked_i=None, step=8):
    """One frame: template, image u8 [h,w]; R f64 [6]; cap 0..255; gain, offset ints in 1/1024; blocked_t / blocked_i the u8
    [gh,gw] block grids of the anchor and of the frame (both or neither) -> int64 [31]."""
    T = np.asarray(template)
    I = np.asarray(image)
    assert T.dtype == np.uint8 and I.dtype == np.uint8 and T.shape == I.shape and T.ndim == 2
    assert int(cap) == cap and 0 <= cap <= 255
    gain, offset, step = int(gain), int(offset), int(step)
    assert 256 <= gain <= 4096 and abs(offset) <= 1 << 20 and step >= 1
    assert (blocked_t is None) == (blocked_i is None)
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
    t = Tl[1:h - 1, 1:w - 1]
    masked = np.zeros_like(ok)
    if blocked_t is not None:
        Bt, Bi = np.asarray(blocked_t), np.asarray(blocked_i)
        gh, gw = -(-h // step), -(-w // step)
        assert Bt.shape == (gh, gw) and Bi.shape == (gh, gw)
        xs, ys = xi.astype(np.int64), yi.astype(np.int64)
        in_t = Bt[np.minimum((ys + step // 2) // step, gh - 1), np.minimum((xs + step // 2) // step, gw - 1)] != 0
        xn, yn = np.minimum((ix + 16) >> 5, w - 1), np.minimum((iy + 16) >> 5, h - 1)
        in_i = Bi[np.minimum((yn + step // 2) // step, gh - 1), np.minimum((xn + step // 2) // step, gw - 1)] != 0
        masked = ok & (in_t | in_i)
    r = v - (gain * t + offset)
    capped = ok & ~masked & (np.abs(r) > 1024 * int(cap))
    use = ok & ~masked & ~capped
    gx = Tl[1:h - 1, 2:w] - Tl[1:h - 1, 0:w - 2]
    gy = Tl[2:h, 1:w - 1] - Tl[0:h - 2, 1:w - 1]
    u = 2 * xi.astype(np.int64) - (w - 1)
    q = 2 * yi.astype(np.int64) - (h - 1)
    J = [gx, gy, gx * u + gy * q, gy * u - gx * q, t, np.ones_like(t)]
    out[0] = use.sum()
    out[1] = capped.sum()
    out[2] = masked.sum()
    out[3] = np.abs(r)[use].sum()
    for k in range(6):
        out[4 + k] = (J[k] * r)[use].sum()
    for (j, k), slot in H_INDEX.items():
        out[slot] = (J[j] * J[k])[use].sum()
    return out


def anchor_sums_ex_batch(gray, anchor, R, cap, gain=None, offset=None, blocked=None, step=8):
    """gray u8 [n,h,w], anchor int [n] (-1: none), R f64 [n,6], gain / offset int [n] or None, blocked u8 [n,gh,gw] or None
    -> int64 [n,31]."""
    gray = np.asarray(gray)
    anchor = np.asarray(anchor, dtype=np.int64).reshape(-1)
    R = np.asarray(R, dtype=np.float64).reshape(-1, 6)
    n = gray.shape[0]
    assert anchor.shape[0] == n == R.shape[0]
    gain = np.full(n, 1024, np.int64) if gain is None else np.asarray(gain, dtype=np.int64).reshape(-1)
    offset = np.zeros(n, np.int64) if offset is None else np.asarray(offset, dtype=np.int64).reshape(-1)
    out = np.zeros((n, SLOTS), np.int64)
    for i, a in enumerate(anchor.tolist()):
        if a >= 0:
            bt, bi = (None, None) if blocked is None else (blocked[a], blocked[i])
            out[i] = anchor_sums_ex(gray[a], gray[i], R[i], cap, gain[i], offset[i], bt, bi, step)
    return out
