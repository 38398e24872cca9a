"""NumPy restatements of the two rolling-shutter rules of include/vstab.h (vstab_row_residual_batch,
vstab_rolling_warp_batch), an analytic rolling-shutter renderer and the analytic flow grids of the readout tests.  Nothing here
imports the package.  The warp is the mesh restatement's machinery (tests/mesh_restatement.py: coordinate terms, roundings,
samplers -- pinned to the oracle's warp by tests/test_mesh_warp_cpu.py) with the row displacement in place of the vertex lookup.
"""

from __future__ import annotations

import numpy as np

from tests import mesh_restatement as M

MIN_SAMPLES = 8          # VSTAB_ROW_MIN_SAMPLES


# ---- rule 1: the per-row median of the global fit's residual ------------------------------------------------------------
def row_residual(grid_flow, step, work_size, transitions, blocked=None):
    """grid_flow f32 [P,gh,gw,2], work_size (w, h), transitions f32 [P,3,3], blocked u8 [P+1,gh,gw] | None ->
    (residual f32 [P,gh,2], count i32 [P,gh])."""
    grid = np.asarray(grid_flow, dtype=np.float32)
    pairs, gh, gw, _ = grid.shape
    mats = np.asarray(transitions, dtype=np.float32).reshape(pairs, 9).astype(np.float64)
    x = (np.arange(gw) * int(step)).astype(np.float64)[None, :].repeat(gh, 0)
    y = (np.arange(gh) * int(step)).astype(np.float64)[:, None].repeat(gw, 1)
    residual = np.zeros((pairs, gh, 2), np.float32)
    count = np.zeros((pairs, gh), np.int32)
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
        for b in range(gh):
            n = int(ok[b].sum())
            count[i, b] = n
            if n >= MIN_SAMPLES:
                residual[i, b, 0] = np.median(rx[b][ok[b]])
                residual[i, b, 1] = np.median(ry[b][ok[b]])
    return residual, count


# ---- rule 2: the displacement and the warp ------------------------------------------------------------------------------
def displacement(qx, qy, velocity, readout, src_h):
    """c(q) of the rule: velocity fp64 [6], readout, q fp64 arrays -> (cx, cy) fp64; every operation rounded on its own."""
    V = [np.float64(v) for v in np.asarray(velocity, dtype=np.float64).reshape(6)]
    rho, hm1 = np.float64(readout), np.float64(src_h - 1)
    with np.errstate(all="ignore"):
        yc = np.where(qy > 0.0, qy, 0.0)
        yc = np.where(yc < hm1, yc, hm1)
        vx = (V[0] * qx + V[1] * qy) + V[2]
        vy = (V[3] * qx + V[4] * qy) + V[5]
        D = np.float64(1.0) - rho * vy / hm1
        D = np.where(D >= 0.5, D, 0.5)
        tau = rho * (yc / hm1 - np.float64(0.5)) / D
        cx, cy = -(tau * vx), -(tau * vy)
        bad = ~(np.isfinite(cx) & np.isfinite(cy))
    return np.where(bad, 0.0, cx), np.where(bad, 0.0, cy)


def rolling_warp_frame(src, matrix, out_size, velocity, readout, border=(0.0, 0.0, 0.0), subpix="q5"):
    """One frame of vstab_rolling_warp_batch: src f32 [H,W,3], forward f32 matrix, velocity f64 [6] ->
    (dst f32 [h,w,3], mask f32 [h,w])."""
    src = np.asarray(src, dtype=np.float32)
    sh, sw, _ = src.shape
    dw, dh = int(out_size[0]), int(out_size[1])
    border = np.asarray(border, dtype=np.float32).reshape(3)
    m = M._invert3x3(matrix)
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
        cx, cy = displacement(qx, qy, velocity, readout, sh)
        if subpix == "exact":
            mf = m.astype(np.float32)
            xf, yf = xs.astype(np.float32), ys.astype(np.float32)
            w = xf * mf[6] + yf * mf[7] + mf[8]
            fsx = (xf * mf[0] + yf * mf[1] + mf[2]) / w
            fsy = (xf * mf[3] + yf * mf[4] + mf[5]) / w
            assert fsx.dtype == np.float32
            dst = M._sample_exact(src, (fsx.astype(np.float64) - cx).astype(np.float32), (fsy.astype(np.float64) - cy).astype(np.float32), border)
        else:
            dst = M._sample_q5(src, M._cv_round_clamped(Xn * Wq - np.float64(32.0) * cx), M._cv_round_clamped(Yn * Wq - np.float64(32.0) * cy), border)
        nx = np.clip(M._cv_round_clamped(qx - cx), -32768, 32767)
        ny = np.clip(M._cv_round_clamped(qy - cy), -32768, 32767)
    cov = ((nx >= 0) & (nx < sw) & (ny >= 0) & (ny < sh)).astype(np.float32)
    mask = np.float32(1.0) - cov
    mask = np.where(mask < np.float32(1e-3), np.float32(0.0), mask)
    return dst.astype(np.float32), mask.astype(np.float32)


def rolling_warp(src, matrices, out_size, velocity, readout, border=(0.0, 0.0, 0.0), subpix="q5"):
    """-> (dst [N,h,w,3], mask [N,h,w], pad_count int64 [N])."""
    outs = [rolling_warp_frame(src[i], matrices[i], out_size, velocity[i], readout, border, subpix) for i in range(len(src))]
    dst, mask = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return dst, mask, (mask > 0.5).reshape(len(src), -1).sum(axis=1).astype(np.int64)


# ---- the analytic camera and its rolling-shutter frames -----------------------------------------------------------------
class CameraPath:
    """A smooth analytic camera: at time t (frame intervals) the texture point X is seen at image position
    p = c + s(t) R(theta(t)) (X - c) + d(t), c the frame centre; d, theta and log s are sums of two sinusoids that vanish at
    t = 0, so frame 0 of a global shutter shows the texture as it is.  amp = (px, px, rad, log scale) peak amplitudes; omega
    (rad per frame interval) is the faster component's angular frequency, the other runs at 0.55 of it.  Velocities formed
    from frame-to-frame transitions are finite differences: they see a component of angular frequency o reduced by
    sin(o) / o, 1.5 % at the default 0.3."""

    def __init__(self, width, height, amp=(16.0, 9.0, 0.0, 0.0), omega=0.3, seed=0):
        rng = np.random.default_rng(seed)
        self.width, self.height = int(width), int(height)
        self.cx, self.cy = (width - 1) / 2.0, (height - 1) / 2.0
        self.amp = np.asarray(amp, dtype=np.float64)
        self.omega = omega * rng.uniform(0.85, 1.15, (4, 2)) * np.array([1.0, 0.55])
        self.phase = rng.uniform(0.0, 2.0 * np.pi, (4, 2))
        self.weight = np.array([0.75, 0.25])

    def params(self, t):
        """-> (dx, dy, theta, log s) at times t (any shape)."""
        t = np.asarray(t, dtype=np.float64)[..., None, None]
        wave = np.sin(self.omega * t + self.phase) - np.sin(self.phase)
        return tuple(np.moveaxis((wave * self.weight).sum(-1) * self.amp, -1, 0))

    def to_image(self, X, Y, t):
        dx, dy, th, ls = self.params(t)
        c, s = np.cos(th) * np.exp(ls), np.sin(th) * np.exp(ls)
        return (self.cx + c * (X - self.cx) - s * (Y - self.cy) + dx, self.cy + s * (X - self.cx) + c * (Y - self.cy) + dy)

    def to_texture(self, x, y, t):
        dx, dy, th, ls = self.params(t)
        c, s = np.cos(th) * np.exp(-ls), np.sin(th) * np.exp(-ls)
        u, v = x - self.cx - dx, y - self.cy - dy
        return self.cx + c * u + s * v, self.cy - s * u + c * v

    def matrix(self, t):
        """The global-shutter camera at time t as a 3x3 matrix (texture -> image)."""
        dx, dy, th, ls = (float(v) for v in self.params(t))
        c, s = np.cos(th) * np.exp(ls), np.sin(th) * np.exp(ls)
        return np.array([[c, -s, self.cx - c * self.cx + s * self.cy + dx], [s, c, self.cy - s * self.cx - c * self.cy + dy], [0.0, 0.0, 1.0]])

    def row_time(self, frame, y, readout):
        return frame + readout * (np.asarray(y, dtype=np.float64) / (self.height - 1) - 0.5)

    def velocity(self, x, y, t, eps=1e-4):
        """Image velocity (px per frame interval) of the texture point seen at (x, y) at time t."""
        X, Y = self.to_texture(x, y, t)
        x1, y1 = self.to_image(X, Y, t + eps)
        x0, y0 = self.to_image(X, Y, t - eps)
        return (x1 - x0) / (2 * eps), (y1 - y0) / (2 * eps)

    def corner_skew(self, frame, readout):
        """|tau| * |v| at the four corners of frame `frame` -> the largest, px."""
        best = 0.0
        for x, y in ((0.0, 0.0), (self.width - 1.0, 0.0), (0.0, self.height - 1.0), (self.width - 1.0, self.height - 1.0)):
            tau = readout * (y / (self.height - 1) - 0.5)
            vx, vy = self.velocity(x, y, float(frame))
            best = max(best, abs(tau) * float(np.hypot(vx, vy)))
        return best


def rolling_clip(path, n, readout, device, texture_seed=1234):
    """Pixel (x, y) of frame i is the texture seen through `path` at time i + readout * (y/(H-1) - 1/2); readout 0 is the
    global-shutter twin -> frames [n,H,W,3] float32 on `device`."""
    import torch

    h, w = path.height, path.width
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    frames = torch.empty((n, h, w, 3), device=device, dtype=torch.float32)
    for i in range(n):
        X, Y = path.to_texture(xs, ys, path.row_time(i, ys, readout))
        frames[i] = M.texture(torch.from_numpy(X.astype(np.float32)).to(device), torch.from_numpy(Y.astype(np.float32)).to(device), h, w, texture_seed)
    return frames


def rolling_flow_grid(path, pair, readout, step, noise=0.0, rng=None):
    """The analytic flow a rolling-shutter pair (pair, pair + 1) shows at the stride-`step` grid of its first frame:
    position s of frame `pair` shows the texture point X = to_texture(s, t(s_y)); in frame pair + 1 it is seen at the s' with
    s' = to_image(X, t'(s'_y)), a fixed point.  -> f32 [gh,gw,2]."""
    h, w = path.height, path.width
    gh, gw = -(-h // step), -(-w // step)
    x = (np.arange(gw) * step).astype(np.float64)[None, :].repeat(gh, 0)
    y = (np.arange(gh) * step).astype(np.float64)[:, None].repeat(gw, 1)
    X, Y = path.to_texture(x, y, path.row_time(pair, y, readout))
    nx, ny = x.copy(), y.copy()
    for _ in range(30):
        nx, ny = path.to_image(X, Y, path.row_time(pair + 1, ny, readout))
    flow = np.stack([nx - x, ny - y], -1)
    if noise:
        flow = flow + rng.normal(0.0, noise, flow.shape)
    return flow.astype(np.float32)


def least_squares_fit(flow, step, mode):
    """The least-squares translation or similarity x' = A x of a flow grid -> f32 [3,3]."""
    flow = np.asarray(flow, dtype=np.float64)
    gh, gw, _ = flow.shape
    x = (np.arange(gw) * step).astype(np.float64)[None, :].repeat(gh, 0).ravel()
    y = (np.arange(gh) * step).astype(np.float64)[:, None].repeat(gw, 1).ravel()
    u, v = flow[..., 0].ravel(), flow[..., 1].ravel()
    if mode == "translation":
        return np.array([[1.0, 0.0, u.mean()], [0.0, 1.0, v.mean()], [0.0, 0.0, 1.0]], np.float32)
    # x' = a x - b y + tx, y' = b x + a y + ty
    rows = np.concatenate([np.stack([x, -y, np.ones_like(x), np.zeros_like(x)], 1), np.stack([y, x, np.zeros_like(x), np.ones_like(x)], 1)])
    a, b, tx, ty = np.linalg.lstsq(rows, np.concatenate([x + u, y + v]), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty], [0.0, 0.0, 1.0]], np.float32)
