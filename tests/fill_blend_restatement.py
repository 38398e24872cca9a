"""NumPy restatement of the blended temporal fill (include/vstab.h: vstab_fill_gain_sums, vstab_temporal_fill_blend_batch),
for the tests.

This file makes its OWN statement of the Q5 coordinate X, Y of an output pixel under a float32 forward matrix, of the
interior rule on it, of the feather distance d32 and weight w, of the gain lattice and of q; pixel values come from
`oracle.warp_frame`, as in tests/temporal_fill_restatement.py, from which only the matrix inverse, the usability test and
the clamped rounding are taken.  Nothing here imports the package.
"""

from __future__ import annotations

import numpy as np

from oracle import oracle
from tests.temporal_fill_restatement import _cv_round_clamped, invert3x3, usable_matrix

GAIN_STRIDE = 8          # lattice: x % 8 == 4 and y % 8 == 4
GAIN_MIN_COUNT = 32
GAIN_CLAMP = (0.5, 2.0)


def q5_coordinates(m32, out_size):
    """X, Y (int64 [dh, dw]): the 1/32-px source coordinate the plain warp forms for every output pixel (float32 forward
    matrix -> float64 closed-form inverse -> float64 terms per OpenCV column block -> one clamped rounding)."""
    dw, dh = int(out_size[0]), int(out_size[1])
    m = invert3x3(m32)
    assert m is not None
    ys, xs = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    with np.errstate(all="ignore"):
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
        return _cv_round_clamped(Xn * Wq), _cv_round_clamped(Yn * Wq)


def inside(X, Y, src_size, interp="bilinear"):
    """Every interpolation tap of the Q5 coordinate inside the sw x sh frame (integer parts saturated to short first)."""
    sw, sh = int(src_size[0]), int(src_size[1])
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    if interp == "bicubic":
        return (sx >= 1) & (sx < sw - 2) & (sy >= 1) & (sy < sh - 2)
    return (sx >= 0) & (sx < sw - 1) & (sy >= 0) & (sy < sh - 1)


def feather_distance(X, Y, src_size, interp="bilinear"):
    """d32 (int64): distance of (X, Y) to the tap-interior border in 1/32 px; negative outside."""
    sw, sh = int(src_size[0]), int(src_size[1])
    if interp == "bicubic":
        return np.minimum(np.minimum(X - 32, Y - 32), np.minimum(32 * (sw - 2) - X, 32 * (sh - 2) - Y))
    return np.minimum(np.minimum(X, Y), np.minimum(32 * (sw - 1) - X, 32 * (sh - 1) - Y))


def feather_weight(d32, feather_px):
    """w float32 = (float)min(max(d32, 0), Fe) / (float)Fe, Fe = 32 * feather_px > 0."""
    fe = 32 * int(feather_px)
    return np.clip(d32, 0, fe).astype(np.float32) / np.float32(fe)


def quantise(v):
    """q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0, NaN -> 0; v float32."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        scaled = (v * np.float32(65536.0)).astype(np.float32)
        low = np.where((v > 0) & (v < 1), scaled, np.float32(0.0)).astype(np.int64)     # truncation of a value in [0, 65536)
    return np.where(v > 0, np.where(v < 1, low, 65536), 0).astype(np.uint64)


def _sample(src_frame, m32, out_size, interp):
    out, _ = oracle.warp_frame(src_frame, m32, out_size, interp=interp, border=(0.0, 0.0, 0.0), subpix="q5", want_coverage=False)
    return out


def gain_sums(src, matrices, cand_frame, own_matrices, dst, interp="bilinear"):
    """-> uint64 [n, K, 7]: count, own r g b, candidate r g b over the lattice pixels both the frame and the candidate see."""
    src = np.asarray(src, dtype=np.float32)
    dst = np.asarray(dst, dtype=np.float32)
    n, dh, dw = dst.shape[:3]
    sh, sw = src.shape[1:3]
    matrices = np.asarray(matrices, dtype=np.float32).reshape(n, -1, 3, 3)
    cand_frame = np.asarray(cand_frame, dtype=np.int32).reshape(n, -1)
    own_matrices = np.asarray(own_matrices, dtype=np.float32).reshape(n, 3, 3)
    K = cand_frame.shape[1]
    sums = np.zeros((n, K, 7), np.uint64)
    ys, xs = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    lattice = (xs % GAIN_STRIDE == GAIN_STRIDE // 2) & (ys % GAIN_STRIDE == GAIN_STRIDE // 2)
    for f in range(n):
        if not usable_matrix(own_matrices[f]):
            continue
        own_in = lattice & inside(*q5_coordinates(own_matrices[f], (dw, dh)), (sw, sh), interp)
        for k in range(K):
            j = int(cand_frame[f, k])
            if j < 0 or not usable_matrix(matrices[f, k]):
                continue
            both = own_in & inside(*q5_coordinates(matrices[f, k], (dw, dh)), (sw, sh), interp)
            if not both.any():
                continue
            warped = _sample(src[j], matrices[f, k], (dw, dh), interp)
            sums[f, k, 0] = int(both.sum())
            sums[f, k, 1:4] = quantise(dst[f][both]).sum(axis=0, dtype=np.uint64)
            sums[f, k, 4:7] = quantise(warped[both]).sum(axis=0, dtype=np.uint64)
    return sums


def gains_from_sums(sums):
    """float32 [n, K, 3], in float64: own_c / cand_c clamped to [0.5, 2] where count >= 32 and cand_c >= 1, else 1."""
    sums = np.asarray(sums)
    out = np.ones(sums.shape[:2] + (3,), np.float64)
    for f in range(sums.shape[0]):
        for k in range(sums.shape[1]):
            if int(sums[f, k, 0]) < GAIN_MIN_COUNT:
                continue
            for c in range(3):
                own, cand = int(sums[f, k, 1 + c]), int(sums[f, k, 4 + c])
                if cand >= 1:
                    out[f, k, c] = min(max(own / cand, GAIN_CLAMP[0]), GAIN_CLAMP[1])
    return out.astype(np.float32)


def temporal_fill_blend(src, matrices, cand_frame, own_matrices, gains, feather_px, dst, mask, interp="bilinear"):
    """-> (dst, mask, filled_from int8, fill_count, blend_count, pad_count); the inputs are not modified.  The rule of
    vstab_temporal_fill_blend_batch: padded pixels take gain * sample of the first valid candidate; own pixels with w < 1
    are cross-faded into it (w == 0: replaced by it)."""
    src = np.asarray(src, dtype=np.float32)
    dst = np.array(dst, dtype=np.float32, copy=True)
    mask = np.array(mask, dtype=np.float32, copy=True)
    n, dh, dw = mask.shape
    sh, sw = src.shape[1:3]
    matrices = np.asarray(matrices, dtype=np.float32).reshape(n, -1, 3, 3)
    cand_frame = np.asarray(cand_frame, dtype=np.int32).reshape(n, -1)
    own_matrices = np.asarray(own_matrices, dtype=np.float32).reshape(n, 3, 3)
    gains = np.asarray(gains, dtype=np.float32).reshape(n, -1, 3)
    filled_from = np.full((n, dh, dw), -1, dtype=np.int8)
    fill_count = np.zeros(n, dtype=np.int64)
    blend_count = np.zeros(n, dtype=np.int64)
    one = np.float32(1.0)
    for f in range(n):
        padded = mask[f] == one
        w = np.ones((dh, dw), np.float32)
        if feather_px > 0 and usable_matrix(own_matrices[f]):
            X, Y = q5_coordinates(own_matrices[f], (dw, dh))
            w = np.where(padded, one, feather_weight(feather_distance(X, Y, (sw, sh), interp), feather_px)).astype(np.float32)
        need = padded | (w < one)
        for k in range(cand_frame.shape[1]):
            j = int(cand_frame[f, k])
            if not need.any():
                break
            if j < 0 or not usable_matrix(matrices[f, k]):
                continue
            take = need & inside(*q5_coordinates(matrices[f, k], (dw, dh)), (sw, sh), interp)
            if not take.any():
                continue
            with np.errstate(all="ignore"):
                c = (gains[f, k][None, None, :] * _sample(src[j], matrices[f, k], (dw, dh), interp)).astype(np.float32)
                wk = w[..., None]
                mixed = ((dst[f] * wk).astype(np.float32) + (c * (one - wk)).astype(np.float32)).astype(np.float32)
            fill = take & padded
            blend = take & ~padded
            value = np.where((wk == 0) | padded[..., None], c, mixed)
            dst[f][take] = value[take]
            mask[f][fill] = 0.0
            filled_from[f][take] = k
            fill_count[f] += int(fill.sum())
            blend_count[f] += int(blend.sum())
            need &= ~take
    pad_count = (mask == one).reshape(n, -1).sum(axis=1).astype(np.int64)
    return dst, mask, filled_from, fill_count, blend_count, pad_count


# ---- the flicker clip: the referee's and the GPU known-answer test's setup -------------------------------------------------
FLICKER_GAINS = (0.8, 1.25)
FLICKER_TOL = 5e-4       # derived in tests/test_fill_blend_cpu.py::test_referee_flicker_clip


def flicker_clip(n=8, h=83, w=117, pad=16, max_offset=12, seed=41):
    """Frames are h x w windows of one texture with values in [0.25, 0.75] at integer offsets within +-max_offset px, frame j
    multiplied by a_j = 0.8 (even j) or 1.25 (odd j), so nothing reaches 1.  Every canvas shows frame 0's window: the final
    matrix of frame i is the integer translation by o_i - o_0, and so is the forward matrix of candidate j = i -+ 1 (radius
    1: both neighbours carry the other gain).
    -> dict(frames, truth [n,h,w,3] = a_i * texture on the canvas, final [n,3,3], matrices [n,2,3,3], cand_frame [n,2], a)."""
    rng = np.random.default_rng(seed)
    tex = rng.uniform(0.25, 0.75, (h + 2 * pad, w + 2 * pad, 3)).astype(np.float32)
    offs = rng.integers(-max_offset, max_offset + 1, size=(n, 2))          # (ox, oy): frame_i(x, y) = tex[y + oy + pad, x + ox + pad]
    a = np.array([FLICKER_GAINS[j % 2] for j in range(n)], np.float32)
    frames = np.stack([a[j] * tex[pad + oy:pad + oy + h, pad + ox:pad + ox + w] for j, (ox, oy) in enumerate(offs)]).astype(np.float32)

    def shift(j):
        return np.array([[1, 0, offs[j, 0] - offs[0, 0]], [0, 1, offs[j, 1] - offs[0, 1]], [0, 0, 1]], np.float32)

    final = np.stack([shift(j) for j in range(n)])
    matrices = np.tile(np.eye(3, dtype=np.float32), (n, 2, 1, 1))
    cand = np.full((n, 2), -1, np.int32)
    for i in range(n):
        for k, j in enumerate((i - 1, i + 1)):
            if 0 <= j < n:
                matrices[i, k], cand[i, k] = shift(j), j
    window = tex[pad + offs[0, 1]:pad + offs[0, 1] + h, pad + offs[0, 0]:pad + offs[0, 0] + w]
    truth = (a[:, None, None, None] * window[None]).astype(np.float32)
    return {"frames": frames, "truth": truth, "final": final, "matrices": matrices, "cand_frame": cand, "a": a}
