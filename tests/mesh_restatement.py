"""NumPy restatements of the two mesh-warp rules of include/vstab.h (vstab_mesh_residual_batch, vstab_mesh_warp_batch) and
the non-rigid clip generator of the tests.  Nothing here imports the package; the warp restatement states the plain warp's
coordinate arithmetic AND its bilinear samplers itself (the displaced coordinate differs per pixel, so no whole-frame oracle
call can stand in) -- tests/test_mesh_warp_cpu.py pins it to the oracle's warp, bit for bit, at zero offsets.
"""

from __future__ import annotations

import numpy as np

MIN_SAMPLES = 4          # VSTAB_MESH_MIN_SAMPLES
INT_MAX, INT_MIN = 2147483647.0, -2147483648.0


# ---- rule 1: the per-vertex residual --------------------------------------------------------------------------------------
def mesh_residual(grid_flow, step, work_size, transitions, mw, mh, blocked=None):
    """grid_flow f32 [P,gh,gw,2], work_size (w, h), transitions f32 [P,3,3], blocked u8 [P+1,gh,gw] | None ->
    (residual f32 [P,mh,mw,2], count i32 [P,mh,mw])."""
    grid = np.asarray(grid_flow, dtype=np.float32)
    pairs, gh, gw, _ = grid.shape
    w, h = int(work_size[0]), int(work_size[1])
    mats = np.asarray(transitions, dtype=np.float32).reshape(pairs, 9).astype(np.float64)
    cw, ch = np.float64(w - 1) / np.float64(mw - 1), np.float64(h - 1) / np.float64(mh - 1)
    x = (np.arange(gw) * int(step)).astype(np.float64)[None, :].repeat(gh, 0)
    y = (np.arange(gh) * int(step)).astype(np.float64)[:, None].repeat(gw, 1)
    residual = np.zeros((pairs, mh, mw, 2), np.float32)
    count = np.zeros((pairs, mh, mw), np.int32)
    for i in range(pairs):
        A = mats[i]
        u, v = grid[i, ..., 0], grid[i, ..., 1]
        with np.errstate(all="ignore"):
            X = (A[0] * x + A[1] * y) + A[2]
            Y = (A[3] * x + A[4] * y) + A[5]
            W = (A[6] * x + A[7] * y) + A[8]
            rx = ((x + u.astype(np.float64)) - X / W).astype(np.float32)
            ry = ((y + v.astype(np.float64)) - Y / W).astype(np.float32)
        ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(rx) & np.isfinite(ry)
        if blocked is not None:
            ok &= (np.asarray(blocked[i]) == 0) & (np.asarray(blocked[i + 1]) == 0)
        for b in range(mh):
            vy = np.float64(b) * np.float64(h - 1) / np.float64(mh - 1)
            for a in range(mw):
                vx = np.float64(a) * np.float64(w - 1) / np.float64(mw - 1)
                take = ok & (np.abs(x - vx) < cw) & (np.abs(y - vy) < ch)
                n = int(take.sum())
                count[i, b, a] = n
                if n >= MIN_SAMPLES:
                    residual[i, b, a, 0] = np.median(rx[take])
                    residual[i, b, a, 1] = np.median(ry[take])
    return residual, count


# ---- rule 2: the warp --------------------------------------------------------------------------------------------------
def _invert3x3(m32):
    S = [np.float64(v) for v in np.asarray(m32, dtype=np.float32).reshape(9)]
    with np.errstate(all="ignore"):
        d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
        if d == 0.0:
            return np.zeros(9, np.float64)
        d = np.float64(1.0) / d
        return np.array([
            (S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
            (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
            (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d], np.float64)


def _cv_round_clamped(v):
    """cvRound(max(INT_MIN, min(INT_MAX, v))) as the C expressions order their comparisons (NaN -> INT_MAX)."""
    m = np.where(v < INT_MAX, v, INT_MAX)
    r = np.where(INT_MIN < m, m, INT_MIN)
    return np.rint(r).astype(np.int64)


def _cell(q, size, verts):
    t = np.where(q > 0.0, q, 0.0)
    top = np.float64(size - 1)
    t = np.where(t < top, t, top)
    g = t * np.float64(verts - 1) / top
    i = np.minimum(g.astype(np.int64), verts - 2)
    return i, g - i.astype(np.float64)


def displacement(qx, qy, offsets, src_size):
    """c(q) of the rule: offsets f32 [mh,mw,2], q fp64 arrays -> (cx, cy) fp64."""
    off = np.asarray(offsets, dtype=np.float32).astype(np.float64)
    mh, mw, _ = off.shape
    ia, fa = _cell(qx, int(src_size[0]), mw)
    ib, fb = _cell(qy, int(src_size[1]), mh)
    ga, gb = 1.0 - fa, 1.0 - fb
    out = []
    for k in range(2):
        c00, c10, c01, c11 = off[ib, ia, k], off[ib, ia + 1, k], off[ib + 1, ia, k], off[ib + 1, ia + 1, k]
        out.append((c00 * ga + c10 * fa) * gb + (c01 * ga + c11 * fa) * fb)
    return out[0], out[1]


def _taps(src, sx, sy, border):
    """The four bilinear taps at integer positions (sx, sy) .. (sx+1, sy+1), the border colour outside the source."""
    sh, sw, _ = src.shape
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = sx + dx, sy + dy
            inside = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
            val = src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)]
            out.append(np.where(inside[..., None], val, border[None, None, :]))
    return out


def _sample_q5(src, X, Y, border):
    sh, sw, _ = src.shape
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = (X & 31).astype(np.float32), (Y & 31).astype(np.float32)
    wx1 = fx * np.float32(1.0 / 32); wx0 = np.float32(1.0) - wx1
    wy1 = fy * np.float32(1.0 / 32); wy0 = np.float32(1.0) - wy1
    w0, w1, w2, w3 = (wy0 * wx0)[..., None], (wy0 * wx1)[..., None], (wy1 * wx0)[..., None], (wy1 * wx1)[..., None]
    v0, v1, v2, v3 = _taps(src, sx, sy, border)
    out = v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3
    assert out.dtype == np.float32
    none = (sx >= sw) | (sx + 1 < 0) | (sy >= sh) | (sy + 1 < 0)
    return np.where(none[..., None], border[None, None, :], out)


def _sample_exact(src, fsx, fsy, border):
    sh, sw, _ = src.shape
    with np.errstate(all="ignore"):
        flx, fly = np.floor(fsx), np.floor(fsy)
        bad = np.isnan(fsx) | np.isnan(fsy) | (flx >= 2.0e9) | (flx <= -2.0e9) | (fly >= 2.0e9) | (fly <= -2.0e9)
        ix = np.where(bad, 0, flx).astype(np.int64)
        iy = np.where(bad, 0, fly).astype(np.int64)
        ax = (fsx - ix.astype(np.float32))[..., None]
        ay = (fsy - iy.astype(np.float32))[..., None]
        p00, p01, p10, p11 = _taps(src, ix, iy, border)
        v0 = p00 + ax * (p01 - p00)
        v1 = p10 + ax * (p11 - p10)
        out = v0 + ay * (v1 - v0)
    assert out.dtype == np.float32
    none = bad | (ix >= sw) | (ix + 1 < 0) | (iy >= sh) | (iy + 1 < 0)
    return np.where(none[..., None], border[None, None, :], out)


def mesh_warp_frame(src, matrix, out_size, offsets, border=(0.0, 0.0, 0.0), subpix="q5"):
    """One frame of vstab_mesh_warp_batch: src f32 [H,W,3], forward f32 matrix, offsets f32 [mh,mw,2] ->
    (dst f32 [h,w,3], mask f32 [h,w])."""
    src = np.asarray(src, dtype=np.float32)
    sh, sw, _ = src.shape
    dw, dh = int(out_size[0]), int(out_size[1])
    border = np.asarray(border, dtype=np.float32).reshape(3)
    m = _invert3x3(matrix)
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
            Wn = (np.float64(1.0) / m[8]) if m[8] != 0.0 else np.float64(0.0)
        else:
            W = W0 + m[6] * dx1
            Wn = np.where(W != 0.0, np.float64(1.0) / np.where(W != 0.0, W, 1.0), 0.0)
            Wq = np.float64(32.0) * Wn
        qx, qy = Xn * Wn, Yn * Wn
        cx, cy = displacement(qx, qy, offsets, (sw, sh))
        if subpix == "exact":
            mf = m.astype(np.float32)
            xf, yf = xs.astype(np.float32), ys.astype(np.float32)
            w = xf * mf[6] + yf * mf[7] + mf[8]
            fsx = (xf * mf[0] + yf * mf[1] + mf[2]) / w
            fsy = (xf * mf[3] + yf * mf[4] + mf[5]) / w
            assert fsx.dtype == np.float32
            dst = _sample_exact(src, (fsx.astype(np.float64) - cx).astype(np.float32), (fsy.astype(np.float64) - cy).astype(np.float32), border)
        else:
            dst = _sample_q5(src, _cv_round_clamped(Xn * Wq - np.float64(32.0) * cx), _cv_round_clamped(Yn * Wq - np.float64(32.0) * cy), border)
        nx = np.clip(_cv_round_clamped(qx - cx), -32768, 32767)
        ny = np.clip(_cv_round_clamped(qy - cy), -32768, 32767)
    cov = ((nx >= 0) & (nx < sw) & (ny >= 0) & (ny < sh)).astype(np.float32)
    mask = np.float32(1.0) - cov
    mask = np.where(mask < np.float32(1e-3), np.float32(0.0), mask)
    return dst.astype(np.float32), mask.astype(np.float32)


def mesh_warp(src, matrices, out_size, offsets, border=(0.0, 0.0, 0.0), subpix="q5"):
    """-> (dst [N,h,w,3], mask [N,h,w], pad_count int64 [N])."""
    outs = [mesh_warp_frame(src[i], matrices[i], out_size, offsets[i], border, subpix) for i in range(len(src))]
    dst, mask = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return dst, mask, (mask > 0.5).reshape(len(src), -1).sum(axis=1).astype(np.int64)


# ---- the non-rigid clips of "it helps" --------------------------------------------------------------------------------
def texture(X, Y, height, width, seed=1234):
    """The bench's band-limited procedural texture (bench.synth_clip's recipe for that seed and size) at positions X, Y
    (torch float32 tensors of one shape) -> [..., 3] float32."""
    import torch

    rng = np.random.default_rng(seed)
    k = 20
    dev = X.device
    fx = torch.tensor(rng.uniform(-0.11, 0.11, k) * (1920.0 / width), device=dev, dtype=torch.float32)
    fy = torch.tensor(rng.uniform(-0.11, 0.11, k) * (1080.0 / height), device=dev, dtype=torch.float32)
    ph = torch.tensor(rng.uniform(0, 6.28, (3, k)), device=dev, dtype=torch.float32)
    amp = torch.tensor(rng.uniform(0.3, 1.0, k), device=dev, dtype=torch.float32)
    norm = float(amp.sum())
    arg = X[..., None] * fx + Y[..., None] * fy
    out = torch.empty(tuple(X.shape) + (3,), device=dev, dtype=torch.float32)
    for c in range(3):
        v = (torch.sin(arg + ph[c]) * amp).sum(-1) / norm
        out[..., c] = 0.5 + 0.45 * torch.tanh(2.5 * v)
    return out


def ramp(x, width):
    """a(p): a smooth ramp from 0 at the left edge to 1 at the right edge (smoothstep of x / (width - 1))."""
    t = x / float(width - 1)
    return t * t * (3.0 - 2.0 * t)


def nonrigid_walks(n, width, seed):
    """g_i (global) and e_i (differential) random walks [n,2] in px, g_0 = e_0 = 0; steps scaled to the frame width
    (at 480 px: global up to +-1.5 x +-1 px per frame, differential up to +-0.9 x +-0.6 px per frame -- a few px over 24 frames)."""
    rng = np.random.default_rng(seed)
    s = width / 480.0
    g = np.zeros((n, 2)); e = np.zeros((n, 2))
    for i in range(1, n):
        g[i] = g[i - 1] + rng.uniform(-1.0, 1.0, 2) * (1.5 * s, 1.0 * s)
        e[i] = e[i - 1] + rng.uniform(-1.0, 1.0, 2) * (0.9 * s, 0.6 * s)
    return g, e


def nonrigid_clip(n, height, width, device, seed=5, texture_seed=1234):
    """frame_i(p) = T(p - D_i(p)), D_i(p) = g_i + a(p) * e_i, sampled analytically -> (frames [n,H,W,3] on `device`, g, e)."""
    import torch

    g, e = nonrigid_walks(n, width, seed)
    yy, xx = torch.meshgrid(torch.arange(height, device=device, dtype=torch.float32),
                            torch.arange(width, device=device, dtype=torch.float32), indexing="ij")
    a = ramp(xx, width)
    frames = torch.empty((n, height, width, 3), device=device, dtype=torch.float32)
    for i in range(n):
        frames[i] = texture(xx - (float(g[i, 0]) + a * float(e[i, 0])), yy - (float(g[i, 1]) + a * float(e[i, 1])), height, width,
                            texture_seed)
    return frames, g, e
