"""NumPy restatement of the template track's rule (include/vstab_track.h, vstab_track_template_batch), for the tests.

Integers throughout, so the kernel must give exactly these.  `track` is the rule; `analytic_clip` is the clip the accuracy
tests run on: a textured patch that moves by known sub-pixel offsets over a background that moves differently, both textures
evaluated analytically at every pixel (no interpolation in the generator).
"""

import numpy as np

SENTINEL = np.uint64(2 ** 64 - 1)


def scale_box(box, size, working_size):
    """Full-resolution (x, y, width, height) -> working (bx, by, bw, bh): floor(v * working / full) per value, bw, bh >= 1."""
    x, y, bw, bh = (int(v) for v in box)
    (W, H), (w, h) = size, working_size
    return x * w // W, y * h // H, max(bw * w // W, 1), max(bh * h // H, 1)


def stride_of(bw, bh):
    return -(-max(int(bw), int(bh)) // 64)


def template(key_frame, box, s):
    """-> T int64 [ny,nx]"""
    bx, by, bw, bh = box
    nx, ny = bw // s, bh // s
    return np.asarray(key_frame)[by:by + ny * s:s, bx:bx + nx * s:s].astype(np.int64)


def template_sums(T):
    return np.array([T.size, T.sum(), (T * T).sum()], np.int64)


def cost_surface(frame, T, start, s, R):
    """Every cost of one frame -> uint64 [2R+1, 2R+1], indexed [dy+R][dx+R]."""
    frame = np.asarray(frame).astype(np.int64)
    h, w = frame.shape
    ny, nx = T.shape
    n = np.int64(T.size)
    D = 2 * R + 1
    out = np.full((D, D), SENTINEL, np.uint64)
    qx = start[0] + np.arange(-R, R + 1)
    ok_x = (qx >= 0) & (qx + (nx - 1) * s <= w - 1)
    xs = np.clip(qx[:, None] + np.arange(nx)[None, :] * s, 0, w - 1)          # [D,nx]
    for r, dy in enumerate(range(-R, R + 1)):
        qy = start[1] + dy
        if qy < 0 or qy + (ny - 1) * s > h - 1:
            continue
        rows = frame[qy:qy + ny * s:s]                                        # [ny,w]
        d = rows[:, xs].transpose(1, 0, 2) - T[None]                          # [D,ny,nx]: C - T of every dx of this row
        sd = d.sum(axis=(1, 2))
        sd2 = (d * d).sum(axis=(1, 2))
        J = (n * sd2 - sd * sd).astype(np.uint64)
        out[r] = np.where(ok_x, J, SENTINEL)
    return out


def pick(surface, R):
    """The minimum of (J, dx^2 + dy^2, dy, dx), lexicographic -> (dx, dy, J)."""
    D = 2 * R + 1
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    order = np.lexsort((dx.ravel(), dy.ravel(), (dx * dx + dy * dy).ravel(), surface.ravel()))
    i = int(order[0])
    return int(dx.ravel()[i]), int(dy.ravel()[i]), surface.ravel()[i]


def near_of(surface, R, dx, dy):
    out = np.full(9, SENTINEL, np.uint64)
    for k in range(9):
        cx, cy = dx + k % 3 - 1, dy + k // 3 - 1
        if -R <= cx <= R and -R <= cy <= R:
            out[k] = surface[cy + R, cx + R]
    return out


def track(gray, box, s, R, key):
    """gray u8 [n,h,w]; box = (bx, by, bw, bh) in its pixels -> dict(tsums int64 [3], pos int32 [n,2], best uint64 [n],
    near uint64 [n,9], surface uint64 [n,D,D])."""
    gray = np.asarray(gray)
    n = gray.shape[0]
    D = 2 * R + 1
    T = template(gray[key], box, s)
    pos = np.zeros((n, 2), np.int32)
    best = np.zeros(n, np.uint64)
    near = np.full((n, 9), SENTINEL, np.uint64)
    surface = np.full((n, D, D), SENTINEL, np.uint64)
    pos[key] = box[:2]
    near[key, 4] = 0
    surface[key, R, R] = 0
    for k in list(range(key + 1, n)) + list(range(key - 1, -1, -1)):
        start = pos[k - 1] if k > key else pos[k + 1]
        surface[k] = cost_surface(gray[k], T, (int(start[0]), int(start[1])), s, R)
        dx, dy, J = pick(surface[k], R)
        pos[k] = (start[0] + dx, start[1] + dy)
        best[k] = J
        near[k] = near_of(surface[k], R, dx, dy)
    return {"tsums": template_sums(T), "pos": pos, "best": best, "near": near, "surface": surface}


# ---- the analytic clip ---------------------------------------------------------------------------------------------------
CLIP_N, CLIP_H, CLIP_W = 12, 135, 240
PATCH_W, PATCH_H = 48, 40
# per-frame steps of the patch's corner, px: sub-pixel, up to 9 px per axis
PATCH_STEPS = [(8.3, -3.4), (-4.6, 5.2), (9.0, 2.75), (6.25, -6.1), (-8.7, 4.4), (3.5, 8.8), (-9.0, -7.3), (5.6, -2.2), (7.45, 6.9),
               (-6.8, -8.5), (2.15, 3.3)]
PATCH_START = (90.0, 45.0)


def _background(X, Y):
    return 128.0 + 40.0 * np.sin(0.21 * X + 0.13 * Y) + 30.0 * np.sin(0.085 * X - 0.17 * Y + 1.0) + 25.0 * np.sin(0.33 * Y + 0.05 * X + 2.0)


def _patch(U, V):
    return 128.0 + 45.0 * np.sin(0.5 * U + 0.2 * V) + 35.0 * np.sin(0.27 * V - 0.31 * U + 0.7) + 30.0 * np.sin(0.11 * U + 0.43 * V + 2.1)


def patch_corners():
    """The patch's top-left corner in every frame, float64 [CLIP_N,2]."""
    return np.array(PATCH_START) + np.concatenate([[(0.0, 0.0)], np.cumsum(np.array(PATCH_STEPS), axis=0)])


def analytic_clip():
    """-> (gray u8 [12,135,240], corners float64 [12,2]).  The background slides by (5 sin 1.3k, 4 cos 0.9k)."""
    corners = patch_corners()
    yy, xx = np.mgrid[0:CLIP_H, 0:CLIP_W].astype(np.float64)
    out = np.empty((CLIP_N, CLIP_H, CLIP_W), np.uint8)
    for k in range(CLIP_N):
        img = _background(xx - 5.0 * np.sin(1.3 * k), yy - 4.0 * np.cos(0.9 * k))
        u, v = xx - corners[k, 0], yy - corners[k, 1]
        inside = (u >= 0) & (u < PATCH_W) & (v >= 0) & (v < PATCH_H)
        img = np.where(inside, _patch(u, v), img)
        out[k] = np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8)
    return out, corners


def analytic_box(key):
    """A 40 x 32 box inside the patch of frame `key`, 3..4 px from its edges: (x, y, width, height), ints."""
    cx, cy = patch_corners()[key]
    return int(np.ceil(cx)) + 3, int(np.ceil(cy)) + 3, 40, 32


def analytic_truth(key):
    """Where the centre of analytic_box(key)'s content is in every frame, float64 [CLIP_N,2] (pixel coordinates)."""
    x, y, bw, bh = analytic_box(key)
    corners = patch_corners()
    return np.array([x + (bw - 1) / 2.0, y + (bh - 1) / 2.0]) + (corners - corners[key])
