"""NumPy restatement of the horizon level's device rule (include/vstab.h, vstab_orientation_hist_batch) and the analytic
clip its tests are run on.  Not a test module."""

import numpy as np

K = 256
BINS = 2 * K + 1

# The worst single-frame error of frame_roll(orientation_hist(.)) on the analytic frames at the 12 known rolls of
# ACCURACY_ROLLS, measured on the CPU (profiles/r30_horizon_level.md).  The CPU test asserts 1.5 x this figure (the margin
# absorbs the content seed), the GPU test 2 x (estimated transitions and the warp's interpolation come on top).
MEASURED_WORST_DEG = 0.0965
ACCURACY_ROLLS = (-44.0, -36.0, -28.0, -20.0, -12.0, -4.0, 4.0, 12.0, 20.0, 28.0, 36.0, 44.0)


def gradients(gray):
    """gray u8 [..., h, w] -> (gx, gy, m2) int64 [..., h-2, w-2]: the integer Scharr gradients of the pixels with all eight
    neighbours."""
    g = np.asarray(gray).astype(np.int64)
    tl, tc, tr = g[..., :-2, :-2], g[..., :-2, 1:-1], g[..., :-2, 2:]
    ml, mr = g[..., 1:-1, :-2], g[..., 1:-1, 2:]
    bl, bc, br = g[..., 2:, :-2], g[..., 2:, 1:-1], g[..., 2:, 2:]
    gx = 3 * (tr - tl) + 10 * (mr - ml) + 3 * (br - bl)
    gy = 3 * (bl - tl) + 10 * (bc - tc) + 3 * (br - tr)
    return gx, gy, gx * gx + gy * gy


def orientation_hist(gray, min_mag2):
    """gray u8 [n, h, w] -> hist int64 [n, 2K+1], the rule of vstab_orientation_hist_batch."""
    gray = np.asarray(gray)
    n, h, w = gray.shape
    hist = np.zeros((n, BINS), np.int64)
    if h < 3 or w < 3:
        return hist
    for f in range(n):
        gx, gy, m2 = gradients(gray[f])
        keep = (m2 >= int(min_mag2)) & (m2 > 0)
        gx, gy, m2 = gx[keep], gy[keep], m2[keep]
        a, b = np.abs(gx), np.abs(gy)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        j = (2 * K * lo + hi) // (2 * hi)
        k = np.sign(gx * gy) * np.where(a >= b, 1, -1) * j
        np.add.at(hist[f], k + K, m2)
    return hist


# ---- the analytic clip: a grey value for every scene point, rendered through a known similarity per frame ----
class Scene:
    """About 40 axis-aligned rectangles of random size with tanh edges 1.2 px wide and a contrast of 25-120 grey levels, one
    long horizontal step (the horizon) and a sum of 12 random sinusoids of amplitude `sinus` (of full scale) each.
    structure=False leaves the sinusoids alone; freq is the range of their angular frequencies per axis, radians per pixel."""

    def __init__(self, seed=7, size=(480, 270), sinus=0.004, structure=True, rectangles=40, freq=(0.01, 0.08)):
        rng = np.random.default_rng(seed)
        self.size = size
        w, h = size
        span = 1.6 * max(w, h)            # the scene is larger than the frame: any roll and shake stays inside it
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        n = rectangles if structure else 0
        self.x0 = cx + rng.uniform(-span / 2, span / 2, n)
        self.y0 = cy + rng.uniform(-span / 2, span / 2, n)
        self.x1 = self.x0 + rng.uniform(20, 140, n)
        self.y1 = self.y0 + rng.uniform(20, 140, n)
        self.contrast = rng.uniform(25, 120, n) * rng.choice([-1.0, 1.0], n)
        self.horizon = (cy + 11.3, 40.0) if structure else None
        self.freq = rng.uniform(freq[0], freq[1], (12, 2)) * rng.choice([-1.0, 1.0], (12, 2))
        self.phase = rng.uniform(0, 2 * np.pi, 12)
        self.sinus = float(sinus)
        self.edge = 1.2

    def value(self, u, v):
        out = np.full(u.shape, 118.0)
        e = self.edge
        for x0, y0, x1, y1, c in zip(self.x0, self.y0, self.x1, self.y1, self.contrast):
            sx = 0.5 * (np.tanh((u - x0) / e) - np.tanh((u - x1) / e))
            sy = 0.5 * (np.tanh((v - y0) / e) - np.tanh((v - y1) / e))
            out += c * sx * sy
        if self.horizon is not None:
            out += self.horizon[1] * 0.5 * np.tanh((v - self.horizon[0]) / e)
        for (fu, fv), ph in zip(self.freq, self.phase):
            out += 255.0 * self.sinus * np.sin(u * fu + v * fv + ph)
        return out

    def render(self, roll_deg, shift=(0.0, 0.0), scale=1.0):
        """One frame u8 [h, w]: the scene turned by roll_deg (the point matrix [[c, -s], [s, c]], x right, y down) and scaled
        about the frame centre, then shifted: frame point p = centre + scale * R (q - centre) + shift shows scene point q."""
        w, h = self.size
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        px, py = (x - cx - shift[0]) / scale, (y - cy - shift[1]) / scale
        c, s = np.cos(np.radians(roll_deg)), np.sin(np.radians(roll_deg))
        u, v = cx + c * px + s * py, cy - s * px + c * py          # q = centre + R^T (p - centre - shift) / scale
        return np.clip(np.rint(self.value(u, v)), 0, 255).astype(np.uint8)


def tilted_clip(scene, base_roll, frames=12, shake_deg=2.0, shake_px=3.0, seed=3):
    """-> (gray u8 [frames, h, w], rolls [frames]): the scene at base_roll plus a roll shake of +-shake_deg and a few pixels of
    translation; frame 0 stands at base_roll exactly."""
    rng = np.random.default_rng(seed)
    rolls = base_roll + shake_deg * np.concatenate([[0.0], rng.uniform(-1.0, 1.0, frames - 1)])
    shifts = shake_px * np.concatenate([[[0.0, 0.0]], rng.uniform(-1.0, 1.0, (frames - 1, 2))])
    return np.stack([scene.render(r, tuple(t)) for r, t in zip(rolls, shifts)]), rolls


def rgb_clip(gray):
    """u8 [n, h, w] -> float32 [n, h, w, 3] in 0..1, the three channels alike."""
    return np.repeat((gray.astype(np.float32) / np.float32(255.0))[..., None], 3, axis=-1)


def luma_u8(frames):
    """float [n, h, w, 3] in 0..1 -> u8 [n, h, w]: the channel mean, rounded."""
    return np.clip(np.rint(np.asarray(frames, dtype=np.float64).mean(axis=-1) * 255.0), 0, 255).astype(np.uint8)
