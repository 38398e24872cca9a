"""NumPy restatement of the deflicker's two rules (include/vstab.h: vstab_pair_gain_hist_batch, vstab_pair_gain_sums_batch,
vstab_apply_gain_batch) and of its host arithmetic (deflicker.py), written from the header's text and the issue, not from
the kernels or the module.  Everything the measurement sums is an integer, so the GPU has to equal it exactly; the apply
rule is one float32 multiply.  Also the synthetic flicker clip the tests and tools/deflicker_report.py share."""

import numpy as np

STRIDE = 4
LO, HI = 2048, 63488
BINS = 1024
MIN_COUNT = 256


def quantise(v):
    """q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0, NaN -> 0; v float32 -> int64."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        mid = (v > 0) & (v < 1)
        scaled = (np.where(mid, v, np.float32(0)) * np.float32(65536.0)).astype(np.float32)
        out = np.where(mid, np.trunc(scaled).astype(np.int64), 0)
        out = np.where(v >= 1, 65536, out)             # false for a NaN, like v > 0
    return out.astype(np.int64)


def lattice(h, w):
    """The lattice pixels of an h x w frame -> (y int64 [K], x int64 [K])."""
    ys, xs = np.arange(STRIDE // 2, h, STRIDE), np.arange(STRIDE // 2, w, STRIDE)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return yy.reshape(-1).astype(np.int64), xx.reshape(-1).astype(np.int64)


def pair_samples(frame_a, frame_b, matrix):
    """One pair: frames f32 [h,w,3], matrix f32 [3,3] (x_b = A x_a) -> (inside count, qa int64 [K,4], qb int64 [K,4], bins
    int64 [K,4]) over the K well-exposed lattice pixels."""
    a, b = np.asarray(frame_a, np.float32), np.asarray(frame_b, np.float32)
    h, w = a.shape[:2]
    A = np.asarray(matrix, dtype=np.float32).reshape(9).astype(np.float64)
    yi, xi = lattice(h, w)
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    with np.errstate(all="ignore"):
        X = (A[0] * x + A[1] * y) + A[2]
        Y = (A[3] * x + A[4] * y) + A[5]
        W = (A[6] * x + A[7] * y) + A[8]
        ok = (W > 0.0) & np.isfinite(W)
        qx, qy = np.rint(X / W), np.rint(Y / W)
        ok &= np.isfinite(qx) & np.isfinite(qy)
        ok &= (qx >= 0.0) & (qx <= w - 1) & (qy >= 0.0) & (qy <= h - 1)
    ix, iy = qx[ok].astype(np.int64), qy[ok].astype(np.int64)
    qa3, qb3 = quantise(a[yi[ok], xi[ok]]), quantise(b[iy, ix])
    well = ((qa3 >= LO) & (qa3 <= HI) & (qb3 >= LO) & (qb3 <= HI)).all(axis=1)
    qa = np.concatenate([qa3[well], qa3[well].sum(axis=1, keepdims=True)], axis=1)
    qb = np.concatenate([qb3[well], qb3[well].sum(axis=1, keepdims=True)], axis=1)
    bins = np.minimum((qb * 256) // np.maximum(qa, 1), BINS - 1)
    return int(ok.sum()), qa, qb, bins


def _pairs(src, transitions, active):
    src = np.asarray(src, np.float32)
    mats = np.asarray(transitions, dtype=np.float32).reshape(-1, 3, 3)
    assert src.ndim == 4 and src.shape[3] == 3 and mats.shape[0] == src.shape[0] - 1
    act = np.ones(len(mats), bool) if active is None else np.asarray(active) != 0
    return src, mats, act


def pair_gain_hist(src, transitions, active=None):
    """src f32 [n,h,w,3], transitions f32 [n-1,3,3], active [n-1] | None -> (hist int64 [n-1,4,1024], stats int64 [n-1,2])."""
    src, mats, act = _pairs(src, transitions, active)
    hist = np.zeros((len(mats), 4, BINS), np.int64)
    stats = np.zeros((len(mats), 2), np.int64)
    for k in np.nonzero(act)[0]:
        inside, qa, _, bins = pair_samples(src[k], src[k + 1], mats[k])
        stats[k] = (inside, len(qa))
        for c in range(4):
            hist[k, c] = np.bincount(bins[:, c], minlength=BINS)
    return hist, stats


def pair_gain_sums(src, transitions, band, active=None):
    """... band int [n-1,4,2] inclusive -> sums int64 [n-1,4,3] = count, sum qa, sum qb."""
    src, mats, act = _pairs(src, transitions, active)
    band = np.asarray(band, np.int64).reshape(len(mats), 4, 2)
    sums = np.zeros((len(mats), 4, 3), np.int64)
    for k in np.nonzero(act)[0]:
        _, qa, qb, bins = pair_samples(src[k], src[k + 1], mats[k])
        for c in range(4):
            sel = (bins[:, c] >= band[k, c, 0]) & (bins[:, c] <= band[k, c, 1])
            sums[k, c] = (int(sel.sum()), int(qa[sel, c].sum()), int(qb[sel, c].sum()))
    return sums


def apply_gain(frames, gains, mask=None):
    """frames f32 [n,h,w,3], gains f32 [n,3], mask f32 [n,h,w] | None -> (out f32, clamped int64 [n]).  Untouched values keep
    their bits."""
    v = np.asarray(frames, np.float32)
    g = np.broadcast_to(np.asarray(gains, np.float32).reshape(-1, 1, 1, 3), v.shape)
    own = np.ones(v.shape[:3], bool) if mask is None else ~(np.asarray(mask, np.float32) == np.float32(1.0))
    with np.errstate(all="ignore"):
        touch = own[..., None] & (g != np.float32(1.0)) & ~np.isnan(v)
        scaled = (v * g).astype(np.float32)
        clamp = touch & (scaled > np.float32(1.0)) & (v <= np.float32(1.0))
    out = v.copy()
    out[touch] = scaled[touch]
    out[clamp] = np.float32(1.0)
    return out, clamp.reshape(len(v), -1).sum(axis=1).astype(np.int64)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------
def bands_from_hist(hist):
    """Plain loops: the lower median bin m and the band [m - (m >> 3), m + ((m + 7) >> 3)]; empty -> m = -1, band [1, 0]."""
    hist = np.asarray(hist, np.int64)
    band = np.zeros(hist.shape[:2] + (2,), np.int64)
    med = np.zeros(hist.shape[:2], np.int64)
    for k in range(hist.shape[0]):
        for c in range(4):
            total = int(hist[k, c].sum())
            if total == 0:
                med[k, c], band[k, c] = -1, (1, 0)
                continue
            need, run = (total + 1) // 2, 0
            for m in range(BINS):
                run += int(hist[k, c, m])
                if run >= need:
                    break
            med[k, c], band[k, c] = m, (m - (m >> 3), m + ((m + 7) >> 3))
    return band, med


def gains_from_sums(sums):
    sums = np.asarray(sums, np.int64)
    g = np.ones(sums.shape[:2])
    ok = np.zeros(sums.shape[:2], bool)
    for k in range(sums.shape[0]):
        for c in range(4):
            if sums[k, c, 0] >= MIN_COUNT:
                g[k, c], ok[k, c] = float(sums[k, c, 2]) / float(sums[k, c, 1]), True
    return g, ok


def corrections(pair_gain, linked, n, radius, segments=None, clamp=(0.5, 2.0)):
    """Plain loops -> (c float64 [n,3], clamped bool [n])."""
    g = np.asarray(pair_gain, np.float64).reshape(n - 1, 3)
    shot = np.zeros(n, np.int64)                  # chain segment of every frame
    starts = {s for s, _ in (segments or [(0, n)])}
    for i in range(1, n):
        shot[i] = shot[i - 1] + (1 if (i in starts or not linked[i - 1]) else 0)
    L = np.zeros((n, 3))
    for i in range(1, n):
        if shot[i] == shot[i - 1]:
            L[i] = L[i - 1] + np.log(g[i - 1])
    c = np.ones((n, 3))
    for i in range(n):
        win = [j for j in range(max(0, i - radius), min(n, i + radius + 1)) if shot[j] == shot[i]]
        c[i] = np.exp(np.mean(L[win], axis=0) - L[i])
    hit = ((c < clamp[0]) | (c > clamp[1])).any(axis=1)
    return np.clip(c, *clamp), hit


def measure(src, transitions, mode="exposure", active=None, band_override=None):
    """Both passes and the pair gains on the CPU -> (pair_gain float64 [P,3], measured bool [P], inlier float64 [P])."""
    hist, stats = pair_gain_hist(src, transitions, active)
    band, _ = bands_from_hist(hist)
    if band_override is not None:
        band = np.broadcast_to(np.asarray(band_override, np.int64), band.shape)
    sums = pair_gain_sums(src, transitions, band, active)
    g, ok = gains_from_sums(sums)
    if mode == "rgb":
        pair_gain, measured = g[:, :3].copy(), ok[:, :3].all(axis=1)
        count = sums[:, :3, 0].min(axis=1)
    else:
        pair_gain, measured = np.repeat(g[:, 3:4], 3, axis=1), ok[:, 3].copy()
        count = sums[:, 3, 0]
    return pair_gain, measured, count / np.maximum(stats[:, 1], 1)


# ---- the synthetic flicker clip -----------------------------------------------------------------------------------------
CLIP_N, CLIP_H, CLIP_W = 12, 135, 240


def _texture(X, Y, seed, scale=1.0):
    """The bench's band-limited procedural texture recipe (sums of sines through a tanh) in NumPy float64 -> [..., 3] in
    0.05..0.95."""
    rng = np.random.default_rng(seed)
    k = 20
    fx = rng.uniform(-0.11, 0.11, k) * (1920.0 / CLIP_W) * scale * 0.25
    fy = rng.uniform(-0.11, 0.11, k) * (1080.0 / CLIP_H) * scale * 0.25
    ph = rng.uniform(0, 6.28, (3, k))
    amp = rng.uniform(0.3, 1.0, k)
    arg = X[..., None] * fx + Y[..., None] * fy
    out = np.empty(X.shape + (3,))
    for c in range(3):
        out[..., c] = 0.5 + 0.45 * np.tanh(2.5 * (np.sin(arg + ph[c]) * amp).sum(-1) / amp.sum())
    return out


def flicker_clip(seed=11, sigma=0.12, rgb=False):
    """12 frames of 240 x 135: the texture under an integer random-walk shift of up to 2 px per frame and axis, a subject on
    a 120 x 80 rectangle (at most 30 % of the frame) that moves 3 px per frame against the scene and shows other content in
    every frame, brighter in the odd ones (no gain explains it, and a plain ratio of sums is pulled by it), a clipped patch, and a per-frame gain (log-normal, sigma 12 %; rgb=True: green gets a gain of its own).
    -> (frames f32 [n,h,w,3], gains float64 [n,3], shifts int [n,2] (x, y), subject boxes [n,4] = x0, y0, x1, y1)."""
    rng = np.random.default_rng(seed)
    n, h, w = CLIP_N, CLIP_H, CLIP_W
    steps = rng.integers(-2, 3, (n, 2))
    steps[0] = 0
    shifts = np.cumsum(steps, axis=0)
    gains = np.exp(rng.normal(0.0, sigma, (n, 1))) * np.ones((1, 3))
    if rgb:
        gains[:, 1] *= np.exp(rng.normal(0.0, sigma, n))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.empty((n, h, w, 3), np.float32)
    boxes = np.empty((n, 4), np.int64)
    for i in range(n):
        dx, dy = int(shifts[i, 0]), int(shifts[i, 1])
        # frame_i(p) = T(p - shift_i): scene point s shows at s + shift_i.  Moderate levels, so that a gain of e^(3 sigma)
        # clips nothing but the patch
        img = 0.2 + 0.45 * _texture(xx - dx, yy - dy, 1234)
        patch = ((xx - dx - 40) ** 2 + (yy - dy - 100) ** 2) < 15 ** 2
        img[patch] = 1.2                                           # a light source: clipped in every frame (and below 1.5 times
                                                                   # any gain: the pipeline's value-range rule leaves it alone)
        x0, y0 = 60 + 3 * i + dx, 20 + dy
        boxes[i] = (x0, y0, x0 + 120, y0 + 80)
        sub = (xx >= x0) & (xx < x0 + 120) & (yy >= y0) & (yy < y0 + 80)
        other = (0.1 + 0.5 * _texture(xx - x0, yy - y0, 99 + i, scale=4.0)) * (1.25 if i % 2 else 0.8)     # new content in every frame
        img[sub] = other[sub]
        frames[i] = (img * gains[i]).astype(np.float32)
    return frames, gains, shifts, boxes


def true_transitions(shifts):
    """x_{k+1} = A_k x_k for the clip's integer shifts -> f32 [n-1,3,3]."""
    mats = np.tile(np.eye(3, dtype=np.float32), (len(shifts) - 1, 1, 1))
    mats[:, 0, 2] = shifts[1:, 0] - shifts[:-1, 0]
    mats[:, 1, 2] = shifts[1:, 1] - shifts[:-1, 1]
    return mats
