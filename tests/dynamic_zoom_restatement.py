"""NumPy restatement of the coverage-extent rule of include/vstab.h (vstab_cover_extent_batch) and the clips of the dynamic
zoom tests.  Nothing here imports the package: the coverage bit is the mask of tests/mesh_restatement.mesh_warp_frame (the
warp's own mask rule, all-zero offsets for the plain warp), reduced with the rule's integer measure.
"""

from __future__ import annotations

import numpy as np

from tests.mesh_restatement import mesh_warp_frame

SENTINEL = 0xFFFFFFFF


def extent_measure(out_size):
    """e(x, y) = max(|2x - (W-1)| * (H-1), |2y - (H-1)| * (W-1)) -> int64 [H,W]."""
    w, h = int(out_size[0]), int(out_size[1])
    ys, xs = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    return np.maximum(np.abs(2 * xs - (w - 1)) * (h - 1), np.abs(2 * ys - (h - 1)) * (w - 1))


def warp_mask(matrix, src_size, out_size, offsets=None, subpix="q5"):
    """The mask vstab_warp_batch (offsets None) / vstab_mesh_warp_batch writes for one frame -> f32 [h,w]."""
    sw, sh = int(src_size[0]), int(src_size[1])
    off = np.zeros((2, 2, 2), np.float32) if offsets is None else np.asarray(offsets, dtype=np.float32)
    return mesh_warp_frame(np.zeros((sh, sw, 3), np.float32), np.asarray(matrix, dtype=np.float32), out_size, off, subpix=subpix)[1]


def extent_of_mask(mask, out_size) -> int:
    """The minimum of e over the pixels with mask == 1.0f, the sentinel if there is none."""
    e = extent_measure(out_size)
    uncovered = np.asarray(mask, dtype=np.float32) == np.float32(1.0)
    return int(e[uncovered].min()) if uncovered.any() else SENTINEL


def cover_extent(matrices, src_size, out_size, offsets=None, subpix="q5") -> np.ndarray:
    """vstab_cover_extent_batch: matrices f32 [n,3,3], sizes (w, h), offsets f32 [n,mh,mw,2] | None -> uint32 [n]."""
    mats = np.asarray(matrices, dtype=np.float32).reshape(-1, 3, 3)
    out = np.empty(len(mats), np.uint32)
    for f, m in enumerate(mats):
        out[f] = extent_of_mask(warp_mask(m, src_size, out_size, None if offsets is None else offsets[f], subpix), out_size)
    return out


def extent_brute_force(mask, out_size) -> int:
    """The same by a loop over the pixels in Python integers (tiny canvases only)."""
    w, h = int(out_size[0]), int(out_size[1])
    best = SENTINEL
    for y in range(h):
        for x in range(w):
            if float(mask[y, x]) == 1.0:
                best = min(best, max(abs(2 * x - (w - 1)) * (h - 1), abs(2 * y - (h - 1)) * (w - 1)))
    return best


# ---- the clips of the pipeline tests ----------------------------------------------------------------------------------
CLIP_W, CLIP_H, CLIP_N = 160, 90, 24
BURST = {10: (6.0, -4.0, 0.012), 11: (-5.0, 5.0, -0.015), 12: (6.0, 3.0, 0.01), 13: (-4.0, -5.0, -0.012)}   # frame: (dx, dy, rad)


def camera_path(n=CLIP_N, w=CLIP_W, h=CLIP_H, burst=None, seed=11, calm=0.25, sweep=(0.0, 0.0)):
    """Camera matrices f64 [n,3,3] for bench.synth_clip(mats=...): a calm move (a slow drift plus a random walk of up to
    `calm` px per frame), the frames of `burst` thrown off it by (dx, dy, rotation), and on top one figure of eight of
    half-axes `sweep` px over the clip, which starts on the path and leaves it to both sides on both axes."""
    burst = BURST if burst is None else burst
    rng = np.random.default_rng(seed)
    out = np.empty((n, 3, 3))
    tx = ty = 0.0
    pre = np.array([[1, 0, -w / 2], [0, 1, -h / 2], [0, 0, 1.0]])
    for i in range(n):
        if i:
            tx += 0.15 + rng.uniform(-calm, calm)
            ty += rng.uniform(-calm, calm)
        dx, dy, th = burst.get(i, (0.0, 0.0, 0.0))
        turn = 2.0 * np.pi * i / max(n - 1, 1)
        dx, dy = dx + sweep[0] * np.sin(turn), dy + sweep[1] * np.sin(2.0 * turn)
        c, s = np.cos(th), np.sin(th)
        post = np.array([[1, 0, w / 2 + tx + dx], [0, 1, h / 2 + ty + dy], [0, 0, 1.0]])
        out[i] = post @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ pre
    return out


SCENE_CUT = 12
SCENE_SHAKE = {1: (1.5, -1.5, 0.0), 2: (-1.5, 1.5, 0.0), 3: (1.5, 1.5, 0.0)}


def scene_shot1_path(n=SCENE_CUT):
    """Shot 1 of the scene-cut test: a wide sweep, a few pixels per frame, that owns every extreme of the common framing."""
    return camera_path(n, burst={}, seed=11, sweep=(10.0, 5.0))


def scene_shot2_path(n=CLIP_N - SCENE_CUT, variant=0):
    """Shot 2: calm (variant 0), or shaking by 1.5 px right behind the cut (variant 1)."""
    return camera_path(n, burst=SCENE_SHAKE if variant else {}, seed=12, calm=0.1)


def locked_final_matrices(path) -> np.ndarray:
    """What a locked camera at full strength applies to the clip of `path`: frame i goes back onto frame 0 -> f32 [n,3,3]."""
    path = np.asarray(path, dtype=np.float64)
    return np.stack([path[0] @ np.linalg.inv(m) for m in path]).astype(np.float32)


def smooth_offsets(n, mw, mh, amp=1.5, seed=2) -> np.ndarray:
    """A smooth per-vertex field that drifts over the clip, up to `amp` px -> f32 [n,mh,mw,2]."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 1.0, mw)[None, :]
    b = np.linspace(0.0, 1.0, mh)[:, None]
    ph = rng.uniform(0, 6.28, 4)
    out = np.empty((n, mh, mw, 2), np.float32)
    for i in range(n):
        t = i / max(n - 1, 1)
        out[i, ..., 0] = amp * np.sin(2.2 * a + 1.3 * b + ph[0] + 2.0 * t) * np.cos(0.9 * b + ph[1])
        out[i, ..., 1] = amp * np.cos(1.7 * a - 1.1 * b + ph[2] - 1.5 * t) * np.sin(1.2 * a + ph[3])
    return out
