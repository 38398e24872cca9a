"""NumPy restatement of the temporal fill (include/vstab.h: vstab_temporal_fill_batch), for the tests.

Validity of a candidate at a pixel comes from this file's OWN statement of the plain warp's coordinate arithmetic
(float32 forward matrix -> float64 closed-form inverse -> float64 coordinate terms per OpenCV column block -> 1/32-px
rounding, or the float32 `exact` chain); pixel values come from `oracle.warp_frame`.  Nothing here imports the package.
"""

from __future__ import annotations

import numpy as np

from oracle import oracle

INT_MAX, INT_MIN = 2147483647.0, -2147483648.0


def invert3x3(m32):
    """cv::invert of the float32 matrix converted to float64 (closed form, fixed operation order); None if det == 0."""
    S = [float(v) for v in np.asarray(m32, dtype=np.float32).reshape(9)]
    with np.errstate(all="ignore"):
        S = [np.float64(v) for v in S]
        d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
        if d == 0.0:
            return None
        d = np.float64(1.0) / d
        t = [
            (S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
            (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
            (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d,
        ]
    return np.array(t, dtype=np.float64)


def usable_matrix(m32) -> bool:
    """The library skips a candidate whose matrix is not finite or has no finite float64 inverse."""
    m32 = np.asarray(m32, dtype=np.float32)
    if not np.isfinite(m32).all():
        return False
    inv = invert3x3(m32)
    return inv is not None and bool(np.isfinite(inv).all())


def _cv_round_clamped(v):
    """cvRound(max(INT_MIN, min(INT_MAX, v))) as the C expressions order their comparisons (NaN -> INT_MAX)."""
    m = np.where(v < INT_MAX, v, INT_MAX)
    r = np.where(INT_MIN < m, m, INT_MIN)
    return np.rint(r).astype(np.int64)


def source_positions(m32, out_size, subpix="q5"):
    """Integer source position (sx, sy) of every output pixel and whether it is representable, as the plain warp forms it.
    q5: sx = saturate_short(X >> 5) of the 1/32-px coordinate; exact: floor of the float32 coordinate (ok = finite)."""
    dw, dh = int(out_size[0]), int(out_size[1])
    m = invert3x3(m32)
    assert m is not None
    ys, xs = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    with np.errstate(all="ignore"):
        if subpix == "exact":
            mf = m.astype(np.float32)
            xf, yf = xs.astype(np.float32), ys.astype(np.float32)
            w = xf * mf[6] + yf * mf[7] + mf[8]
            fsx = (xf * mf[0] + yf * mf[1] + mf[2]) / w
            fsy = (xf * mf[3] + yf * mf[4] + mf[5]) / w
            assert fsx.dtype == np.float32
            flx, fly = np.floor(fsx), np.floor(fsy)
            ok = np.isfinite(flx) & np.isfinite(fly) & (np.abs(flx) < 2.0e9) & (np.abs(fly) < 2.0e9)
            sx = np.where(ok, flx, -1).astype(np.int64)
            sy = np.where(ok, fly, -1).astype(np.int64)
            return sx, sy, ok
        # OpenCV's WarpPerspectiveInvoker: blocks of bw0 columns, row-start terms per block, m * (x - xb) per pixel
        bh0 = min(16, dh)
        bw0 = min(1024 // bh0, dw)
        xb = np.zeros_like(xs) if bw0 >= dw else (xs // bw0) * bw0
        dxb, dy, dx1 = xb.astype(np.float64), ys.astype(np.float64), (xs - xb).astype(np.float64)
        X0 = m[0] * dxb + m[1] * dy + m[2]
        Y0 = m[3] * dxb + m[4] * dy + m[5]
        W0 = m[6] * dxb + m[7] * dy + m[8]
        Xn, Yn = X0 + m[0] * dx1, Y0 + m[3] * dx1
        if m[6] == 0.0 and m[7] == 0.0:
            Wq = (np.float64(32.0) / m[8]) if m[8] != 0.0 else np.float64(0.0)
        else:
            W = W0 + m[6] * dx1
            Wq = np.float64(32.0) * np.where(W != 0.0, np.float64(1.0) / np.where(W != 0.0, W, 1.0), 0.0)
        X, Y = _cv_round_clamped(Xn * Wq), _cv_round_clamped(Yn * Wq)
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    return sx, sy, np.ones_like(sx, dtype=bool)


def valid_map(m32, src_size, out_size, interp="bilinear", subpix="q5"):
    """Where every interpolation tap of the candidate lies inside the source frame (the rule of include/vstab.h)."""
    sw, sh = int(src_size[0]), int(src_size[1])
    sx, sy, ok = source_positions(m32, out_size, subpix)
    if interp == "bicubic":
        return ok & (sx >= 1) & (sx < sw - 2) & (sy >= 1) & (sy < sh - 2)
    return ok & (sx >= 0) & (sx < sw - 1) & (sy >= 0) & (sy < sh - 1)


def temporal_fill(src, matrices, cand_frame, dst, mask, interp="bilinear", subpix="q5"):
    """src [N,H,W,3], matrices [n,K,3,3] f32, cand_frame [n,K], dst [n,h,w,3], mask [n,h,w] ->
    (dst, mask, filled_from int8 [n,h,w], fill_count [n], pad_count [n]); the inputs are not modified."""
    src = np.asarray(src, dtype=np.float32)
    dst = np.array(dst, dtype=np.float32, copy=True)
    mask = np.array(mask, dtype=np.float32, copy=True)
    n, dh, dw = mask.shape
    sh, sw = src.shape[1:3]
    matrices = np.asarray(matrices, dtype=np.float32).reshape(n, -1, 3, 3)
    cand_frame = np.asarray(cand_frame, dtype=np.int32).reshape(n, -1)
    filled_from = np.full((n, dh, dw), -1, dtype=np.int8)
    fill_count = np.zeros(n, dtype=np.int64)
    for f in range(n):
        need = mask[f] == np.float32(1.0)
        for k in range(cand_frame.shape[1]):
            j = int(cand_frame[f, k])
            if not need.any():
                break
            if j < 0 or not usable_matrix(matrices[f, k]):
                continue
            take = need & valid_map(matrices[f, k], (sw, sh), (dw, dh), interp, subpix)
            if not take.any():
                continue
            warped, _ = oracle.warp_frame(src[j], matrices[f, k], (dw, dh), interp=interp, border=(0.0, 0.0, 0.0), subpix=subpix,
                                          want_coverage=False)
            dst[f][take] = warped[take]
            mask[f][take] = 0.0
            filled_from[f][take] = k
            fill_count[f] += int(take.sum())
            need &= ~take
    pad_count = (mask == np.float32(1.0)).reshape(n, -1).sum(axis=1).astype(np.int64)
    return dst, mask, filled_from, fill_count, pad_count
