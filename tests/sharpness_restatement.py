"""NumPy restatement of the sharpness transfer (include/vstab.h: vstab_frame_sharpness_batch, vstab_sharp_transfer_batch),
for the tests.

This file makes its OWN statement of q, of the luma Y, of the gradient energy, and of the transfer's walk, weights and
divisions in float32.  Pixel values of a candidate come from `oracle.warp_frame`; the Q5 coordinate and the interior rule are
taken as tests/fill_blend_restatement.py states them (`q5_coordinates`, `inside`), the usability test of a matrix from
tests/temporal_fill_restatement.py.  Nothing here imports the package.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import oracle
from tests.fill_blend_restatement import inside, q5_coordinates
from tests.temporal_fill_restatement import usable_matrix

MIN_RATIO = 1.1


# ---- the sharpness measure ----------------------------------------------------------------------------------------------
def quantise(v):
    """q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0, NaN -> 0; v float32 -> int64."""
    v = np.asarray(v, dtype=np.float32)
    out = np.zeros(v.shape, np.int64)
    with np.errstate(all="ignore"):
        mid = (v > 0) & (v < 1)
        out[mid] = np.trunc((v[mid] * np.float32(65536.0)).astype(np.float32)).astype(np.int64)
        out[v >= 1] = 65536                      # false for a NaN, like v > 0
    return out


def luma(frame):
    """Y = (q(r) + 2 q(g) + q(b)) >> 2, int64 [h, w] in 0..65536."""
    q = quantise(frame)
    return (q[..., 0] + 2 * q[..., 1] + q[..., 2]) >> 2


def frame_sharpness(frames):
    """-> energy, a list of Python ints (exact, no wrap): sum over x < w - 1, y < h - 1 of gx^2 + gy^2."""
    out = []
    for frame in np.asarray(frames, dtype=np.float32):
        Y = luma(frame)
        c = Y[:-1, :-1]
        gx, gy = Y[:-1, 1:] - c, Y[1:, :-1] - c
        out.append(int((gx * gx + gy * gy).sum(dtype=np.int64)))     # h w <= 2^30 pixels of at most 2^33: below 2^63
    return out


def ratios_from_energy(energy, cand_frame, first=0):
    """float32 [n, K]: E_j / E_i in float64; 0 where cand_frame < 0, E_i == 0 or the quotient is below 1.1."""
    cand_frame = np.asarray(cand_frame)
    out = np.zeros(cand_frame.shape, np.float64)
    for f in range(cand_frame.shape[0]):
        own = int(energy[first + f])
        for k in range(cand_frame.shape[1]):
            j = int(cand_frame[f, k])
            if j >= 0 and own > 0 and float(int(energy[j])) / float(own) >= MIN_RATIO:
                out[f, k] = float(int(energy[j])) / float(own)
    return out.astype(np.float32)


# ---- the transfer -------------------------------------------------------------------------------------------------------
def _sample(src_frame, m32, out_size, interp):
    out, _ = oracle.warp_frame(src_frame, m32, out_size, interp=interp, border=(0.0, 0.0, 0.0), subpix="q5", want_coverage=False)
    return out


def sharp_transfer(src, matrices, cand_frame, ratio, alpha, dst, mask=None, interp="bilinear"):
    """-> (dst, transfer_count int64 [n]); the inputs are not modified.  The rule of vstab_sharp_transfer_batch."""
    src = np.asarray(src, dtype=np.float32)
    dst = np.array(dst, dtype=np.float32, copy=True)
    n, dh, dw = dst.shape[:3]
    sh, sw = src.shape[1:3]
    matrices = np.asarray(matrices, dtype=np.float32).reshape(n, -1, 3, 3)
    cand_frame = np.asarray(cand_frame, dtype=np.int32).reshape(n, -1)
    ratio = np.asarray(ratio, dtype=np.float32).reshape(n, -1)
    alpha = np.float32(alpha)
    one = np.float32(1.0)
    count = np.zeros(n, np.int64)
    for f in range(n):
        own = np.ones((dh, dw), bool) if mask is None else ~(np.asarray(mask[f], dtype=np.float32) == one)
        o = dst[f].copy()
        num = np.zeros((dh, dw, 3), np.float32)
        den = np.zeros((dh, dw), np.float32)
        for k in range(cand_frame.shape[1]):
            j, r = int(cand_frame[f, k]), ratio[f, k]
            if not (r > 0) or j < 0 or not usable_matrix(matrices[f, k]):
                continue
            valid = own & inside(*q5_coordinates(matrices[f, k], (dw, dh)), (sw, sh), interp)
            if not valid.any():
                continue
            s = _sample(src[j], matrices[f, k], (dw, dh), interp)
            with np.errstate(all="ignore"):
                a = np.abs(s - o)
                D = ((a[..., 0] + a[..., 1]) + a[..., 2]).astype(np.float32)
                take = valid & (D < np.float32(np.inf))                       # false for a NaN in s or o
                w = (r / (r + (alpha * D).astype(np.float32)).astype(np.float32)).astype(np.float32)
                new_num = (num + (w[..., None] * s).astype(np.float32)).astype(np.float32)
                new_den = (den + w).astype(np.float32)
            num[take] = new_num[take]
            den[take] = new_den[take]
        with np.errstate(all="ignore"):
            store = own & (den > 0)
            value = ((o + num).astype(np.float32) / (one + den)[..., None].astype(np.float32)).astype(np.float32)
        dst[f][store] = value[store]
        count[f] = int(store.sum())
    return dst, count


# ---- the referee's clip -------------------------------------------------------------------------------------------------
def _value_noise(u, v, lattice):
    """Smoothstep-interpolated random lattice (wraps), evaluated at real coordinates."""
    size = lattice.shape[0]
    iu, iv = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = u - iu, v - iv
    fu, fv = fu * fu * (3 - 2 * fu), fv * fv * (3 - 2 * fv)
    a, b = lattice[iv % size, iu % size], lattice[iv % size, (iu + 1) % size]
    c, d = lattice[(iv + 1) % size, iu % size], lattice[(iv + 1) % size, (iu + 1) % size]
    fu, fv = fu[..., None], fv[..., None]
    return (a * (1 - fu) + b * fu) * (1 - fv) + (c * (1 - fu) + d * fu) * fv


def texture(u, v, seed=7):
    """A procedural texture in [0.1, 0.9], three channels, defined at every real (u, v): value noise at cell sizes 24, 12,
    6, 3 and 1.5 px, so that there is coarse structure for an estimator and fine detail for a blur to destroy."""
    rng = np.random.default_rng(seed)
    total, weight = 0.0, 0.0
    for cell, amp in ((24.0, 1.0), (12.0, 0.8), (6.0, 0.7), (3.0, 0.7), (1.5, 0.6)):
        lattice = rng.uniform(-1.0, 1.0, (97, 97, 3))
        total = total + amp * _value_noise(u / cell + 11.3, v / cell + 5.7, lattice)
        weight += amp
    return 0.5 + 0.4 * np.clip(total / (0.45 * weight), -1.0, 1.0)


def _similarity(tx, ty, angle, scale, cx, cy):
    c, s = scale * np.cos(angle), scale * np.sin(angle)
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1]], np.float64)


def _box5(frame):
    """5 x 5 box blur, the border replicated."""
    h, w = frame.shape[:2]
    p = np.pad(frame.astype(np.float64), ((2, 2), (2, 2), (0, 0)), mode="edge")
    out = np.zeros((h, w, 3), np.float64)
    for dy in range(5):
        for dx in range(5):
            out += p[dy:dy + h, dx:dx + w]
    return out / 25.0


@functools.lru_cache(maxsize=None)
def referee_clip(n=9, w=160, h=120, seed=23, sigma=0.005):
    """9 frames of 160 x 120 of one texture under a known similarity shake (camera C_i: frame 0's coordinates -> frame i's,
    C_0 = I; within +-3 px, +-0.012 rad, +-1 %), frames i % 4 == 2 blurred with a 5 x 5 box, Gaussian noise of sigma 0.005 on
    every frame.  -> dict(frames, sharp [n,h,w,3]: the frames without blur and noise, blurred: the indices, final [n,3,3] =
    C_i^-1 in float32 (camera lock on frame 0), transitions [n-1,3,3] = C_{i+1} C_i^-1, matrices [n,4,3,3] / cand_frame [n,4]:
    the true candidates of radius 2 in the fill's order, H_{i,j} = final_j).  Cached: treat the arrays as read only."""
    rng = np.random.default_rng(seed)
    cams = [np.eye(3)]
    for _ in range(1, n):
        cams.append(_similarity(rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.012, 0.012), rng.uniform(0.99, 1.01), w / 2, h / 2))
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sharp, frames, blurred = [], [], []
    for i, cam in enumerate(cams):
        inv = np.linalg.inv(cam)
        u = inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]
        v = inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]
        frame = texture(u, v)
        sharp.append(frame.astype(np.float32))
        if i % 4 == 2:
            frame = _box5(frame)
            blurred.append(i)
        frames.append((frame + rng.normal(0.0, sigma, frame.shape)).astype(np.float32))
    final = np.stack([np.linalg.inv(c) for c in cams]).astype(np.float32)
    transitions = np.stack([cams[i + 1] @ np.linalg.inv(cams[i]) for i in range(n - 1)]).astype(np.float32)
    matrices = np.tile(np.eye(3, dtype=np.float32), (n, 4, 1, 1))
    cand = np.full((n, 4), -1, np.int32)
    for i in range(n):
        for k, j in enumerate((i - 1, i + 1, i - 2, i + 2)):
            if 0 <= j < n:
                matrices[i, k], cand[i, k] = final[j], j
    return {"frames": np.stack(frames), "sharp": np.stack(sharp), "blurred": blurred, "final": final, "transitions": transitions,
            "matrices": matrices, "cand_frame": cand}


def psnr(a, b, where):
    """10 log10(1 / mean squared error) over the pixels of `where` [h, w], in float64."""
    d = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))[where]
    return float(10.0 * np.log10(1.0 / np.mean(d * d)))


@functools.lru_cache(maxsize=None)
def referee(alpha=16.0):
    """The referee clip through the restatement with the TRUE matrices: every frame is warped onto frame 0's canvas (padding
    0.5), the transfer runs with radius 2, and each blurred frame's output is compared with the warp of its sharp,
    noise-free render over the frame's own pixels.  -> dict(before, after: PSNR in dB per blurred frame, gain_mean,
    ratios, out, warped, mask, count)."""
    clip = referee_clip()
    frames, size = clip["frames"], (clip["frames"].shape[2], clip["frames"].shape[1])
    warped, mask, _ = oracle.warp_clip(frames, clip["final"], size, border=(0.5, 0.5, 0.5))
    truth, _, _ = oracle.warp_clip(clip["sharp"], clip["final"], size, border=(0.5, 0.5, 0.5))
    ratios = ratios_from_energy(frame_sharpness(frames), clip["cand_frame"])
    out, count = sharp_transfer(frames, clip["matrices"], clip["cand_frame"], ratios, alpha, warped, mask)
    before = [psnr(warped[i], truth[i], mask[i] == 0) for i in clip["blurred"]]
    after = [psnr(out[i], truth[i], mask[i] == 0) for i in clip["blurred"]]
    return {"before": before, "after": after, "gain_mean": float(np.mean(np.subtract(after, before))), "ratios": ratios,
            "out": out, "warped": warped, "mask": mask, "count": count}
