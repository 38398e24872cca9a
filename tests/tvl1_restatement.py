"""NumPy float32 restatement of OpenCV's Dual TV-L1 optical flow (cv::optflow::DualTVL1OpticalFlow::calc(I0, I1, flow)
with no initial flow), the third motion estimator of the reference's Flow node (nodes/video_stabilizer_flow.py:76-107).

Restated from OpenCV 4.x contrib, modules/optflow/src/tvl1flow.cpp (the 4.5-4.10 form of the file: calc, procOneScale,
centeredGradient, estimateGradRho, estimateV, divergence, estimateU, forwardGradient, estimateDualVariables) and the
imgproc primitives it calls (resize INTER_LINEAR, remap INTER_CUBIC with float maps, medianBlur 5x5).  UNPINNED against
OpenCV: no cv2 with the optflow module was at hand when this was written; every semantic below is read from the
published source and needs checking against it.  Known places where a real OpenCV can differ in the last bit:
  - resize / remap may run IPP or SIMD paths (v_muladd may fuse), this file never fuses;
  - hypot: restated as sqrt of the double sum of the squared floats, rounded to float;
  - the error sum of estimateU (see row_tree_error): OpenCV sums in its own parallel order.

Every association is written out once here and the HIP kernel (csrc/vstab_tvl1.hip) follows it:
  - all arithmetic is IEEE float32, no fused multiply-add;
  - v:       rho = rho_c + (I1wx*u1 + I1wy*u2); v = u + d (d per the three branches of estimateV)
  - div p:   interior (p1[x] - p1[x-1]) + (p2[y] - p2[y-1]); row 0 (p1[x] - p1[x-1]) + p2; column 0 (p1 + p2) - p2[y-1];
             corner p1 + p2
  - u:       u = v + theta*div;  term = du1*du1 + du2*du2 (float)
  - error:   the terms of a row, zero-padded to a power of two, summed in double by a pairwise tree; the row sums,
             zero-padded to a power of two, by a second tree; rounded to float.  A deliberate, stated deviation: the
             one place where OpenCV's (thread-count dependent) order cannot be reproduced in parallel.
  - p:       g = float(sqrt(double(ux)^2 + double(uy)^2)); ng = 1 + taut*g; p = (p + taut*u_x) / ng
  - rho_c:   ((I1w - I1wx*u1) - I1wy*u2) - I0;  grad = I1wx*I1wx + I1wy*I1wy
"""

from __future__ import annotations

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_EPSILON = np.finfo(np.float32).eps

DEFAULTS = dict(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, inner_iterations=30,
                outer_iterations=10, scale_step=0.8, gamma=0.0, median_filtering=5)


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


# ---------------------------------------------------------------------------------------------- resize INTER_LINEAR

def _round_half_even(v: float) -> int:
    return int(np.rint(v))


def _taps(dn: int, scale: float):
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    return s, f


def resize_linear(src, dw: int, dh: int, scale_x: float, scale_y: float):
    """cv::resize(INTER_LINEAR) of a float32 image, generic path: horizontal pass into float rows, then vertical.
    scale_x / scale_y: source pixels per destination pixel, in double, as resize computes them (1 / inv_scale)."""
    src = np.asarray(src, F32)
    sh, sw = src.shape
    sx, fx = _taps(dw, scale_x)
    neg = sx < 0
    fx[neg] = 0
    sx[neg] = 0
    tail = sx + 1 >= sw   # dx >= xmax: D = S[sx] with sx clamped to sw-1
    sx[tail] = sw - 1
    fx[tail] = 0
    a0 = (F32(1) - fx).astype(F32)
    a1 = fx
    sx1 = np.minimum(sx + 1, sw - 1)
    hor = (src[:, sx] * a0 + src[:, sx1] * a1).astype(F32)
    hor[:, tail] = src[:, sx[tail]]
    sy, fy = _taps(dh, scale_y)
    b0 = (F32(1) - fy).astype(F32)
    b1 = fy
    r0 = np.clip(sy, 0, sh - 1)
    r1 = np.clip(sy + 1, 0, sh - 1)
    return (hor[r0] * b0[:, None] + hor[r1] * b1[:, None]).astype(F32)


def resize_scale(src, step: float):
    """resize(src, Size(), step, step, INTER_LINEAR): destination size rounds w*step, the scale is 1/step."""
    sh, sw = src.shape
    return resize_linear(src, _round_half_even(sw * step), _round_half_even(sh * step), 1.0 / step, 1.0 / step)


def resize_to(src, dw: int, dh: int):
    """resize(src, dst, Size(dw, dh)) (INTER_LINEAR): scale = 1 / (d / s) in double."""
    sh, sw = src.shape
    return resize_linear(src, dw, dh, 1.0 / (dw / sw), 1.0 / (dh / sh))


def pyramid_sizes(h: int, w: int, nscales: int, scale_step: float):
    """The (h, w) of every level calc() keeps: a level narrower or shorter than 16 ends the pyramid before it."""
    sizes = [(h, w)]
    for _ in range(1, nscales):
        ph, pw = sizes[-1]
        nh, nw = _round_half_even(ph * scale_step), _round_half_even(pw * scale_step)
        if nw < 16 or nh < 16:
            break
        sizes.append((nh, nw))
    return sizes


# ---------------------------------------------------------------------------------------------- remap INTER_CUBIC

def cubic_table():
    """initInterTab1D(INTER_CUBIC): interpolateCubic(i/32) in float, A = -0.75."""
    A = F32(-0.75)
    out = np.zeros((32, 4), F32)
    for i in range(32):
        x = F32(i) * F32(1.0 / 32)
        x1 = F32(x + F32(1))
        c0 = F32(F32(F32(F32(F32(A * x1) - F32(5) * A) * x1) + F32(8) * A) * x1) - F32(4) * A
        c1 = F32(F32(F32(F32(F32(A + F32(2)) * x) - F32(A + F32(3))) * x) * x) + F32(1)
        omx = F32(F32(1) - x)
        c2 = F32(F32(F32(F32(F32(A + F32(2)) * omx) - F32(A + F32(3))) * omx) * omx) + F32(1)
        c3 = F32(F32(F32(F32(1) - F32(c0)) - F32(c1)) - F32(c2))
        out[i] = (c0, c1, c2, c3)
    return out


_CUB = cubic_table()


def remap_cubic(src, map_x, map_y):
    """cv::remap(src, dst, map_x, map_y, INTER_CUBIC, BORDER_CONSTANT, 0) with float32 maps: the maps are rounded to
    1/32 px (cvRound(m*32), half to even), the taps use the float 2-D weight table cy[i]*cx[j]."""
    src = np.asarray(src, F32)
    sh, sw = src.shape
    X = np.rint(np.asarray(map_x, F32) * F32(32)).astype(np.int64)
    Y = np.rint(np.asarray(map_y, F32) * F32(32)).astype(np.int64)
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    cx = _CUB[X & 31]
    cy = _CUB[Y & 31]
    x0, y0 = sx - 1, sy - 1
    interior = (x0 >= 0) & (x0 < sw - 3) & (y0 >= 0) & (y0 < sh - 3)
    # interior: per row ((t0 + t1) + t2) + t3 of the four products, rows summed in order
    acc = None
    brd = np.zeros(X.shape, F32)
    for i in range(4):
        yy = y0 + i
        yok = (yy >= 0) & (yy < sh)
        yc = np.clip(yy, 0, sh - 1)
        row = None
        for j in range(4):
            xx = x0 + j
            xok = (xx >= 0) & (xx < sw)
            xc = np.clip(xx, 0, sw - 1)
            wgt = (cy[..., i] * cx[..., j]).astype(F32)
            prod = (src[yc, xc] * wgt).astype(F32)
            row = prod if row is None else (row + prod).astype(F32)
            brd = (brd + np.where(yok & xok, prod, F32(0))).astype(F32)
        acc = row if acc is None else (acc + row).astype(F32)
    return np.where(interior, acc, brd).astype(F32)


# ---------------------------------------------------------------------------------------------- field operators

def centered_gradient(img):
    xp = np.concatenate([img[:, 1:], img[:, -1:]], axis=1)
    xm = np.concatenate([img[:, :1], img[:, :-1]], axis=1)
    yp = np.concatenate([img[1:], img[-1:]], axis=0)
    ym = np.concatenate([img[:1], img[:-1]], axis=0)
    return (F32(0.5) * (xp - xm)).astype(F32), (F32(0.5) * (yp - ym)).astype(F32)


def forward_gradient(u):
    dx = np.zeros_like(u)
    dy = np.zeros_like(u)
    dx[:, :-1] = u[:, 1:] - u[:, :-1]
    dy[:-1, :] = u[1:, :] - u[:-1, :]
    return dx, dy


def divergence(v1, v2):
    div = np.empty_like(v1)
    div[1:, 1:] = (v1[1:, 1:] - v1[1:, :-1]) + (v2[1:, 1:] - v2[:-1, 1:])
    div[0, 1:] = (v1[0, 1:] - v1[0, :-1]) + v2[0, 1:]
    div[1:, 0] = (v1[1:, 0] + v2[1:, 0]) - v2[:-1, 0]
    div[0, 0] = v1[0, 0] + v2[0, 0]
    return div


def median5(u):
    """medianBlur(u, 5) on float32, replicated border: the 13th smallest of the 25 values."""
    h, w = u.shape
    pad = np.pad(u, 2, mode="edge")
    stack = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)])
    return np.partition(stack, 12, axis=0)[12].astype(F32)


def _pairwise(x, axis=-1):
    n = x.shape[axis]
    size = 1
    while size < n:
        size *= 2
    if size != n:
        pad = [(0, 0)] * x.ndim
        pad[axis] = (0, size - n)
        x = np.pad(x, pad)
    x = np.moveaxis(x, axis, -1)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def row_tree_error(term):
    """The stated error-sum order: float terms -> double; each row zero-padded to a power of two and summed by a
    pairwise tree; the row sums the same way; rounded to float."""
    rows = _pairwise(term.astype(np.float64), axis=1)
    return F32(_pairwise(rows, axis=0))


# ---------------------------------------------------------------------------------------------- the algorithm

def _one_scale(I0, I1, u1, u2, p, counts_s):
    h, w = I0.shape
    eps = F32(p["epsilon"] * p["epsilon"] * (h * w))
    l_t = F32(p["lambda_"] * p["theta"])
    taut = F32(p["tau"] / p["theta"])
    theta = F32(p["theta"])
    I1x, I1y = centered_gradient(I1)
    p11 = np.zeros((h, w), F32)
    p12 = np.zeros((h, w), F32)
    p21 = np.zeros((h, w), F32)
    p22 = np.zeros((h, w), F32)
    xs = np.arange(w, dtype=F32)[None, :]
    ys = np.arange(h, dtype=F32)[:, None]
    for wi in range(p["warps"]):
        mx = (xs + u1).astype(F32)
        my = (ys + u2).astype(F32)
        I1w = remap_cubic(I1, mx, my)
        I1wx = remap_cubic(I1x, mx, my)
        I1wy = remap_cubic(I1y, mx, my)
        grad = (I1wx * I1wx + I1wy * I1wy).astype(F32)
        rho_c = (((I1w - I1wx * u1) - I1wy * u2) - I0).astype(F32)
        lt_grad = (l_t * grad).astype(F32)
        d1_lo, d2_lo = (l_t * I1wx).astype(F32), (l_t * I1wy).astype(F32)
        d1_hi, d2_hi = (-l_t * I1wx).astype(F32), (-l_t * I1wy).astype(F32)
        small = ~(grad > F32(FLT_EPSILON))
        safe_grad = np.where(small, F32(1), grad)
        error = F32(FLT_MAX)
        n_outer = 0
        while error > eps and n_outer < p["outer_iterations"]:
            if p["median_filtering"] > 1:
                u1 = median5(u1)
                u2 = median5(u2)
            n_inner = 0
            while error > eps and n_inner < p["inner_iterations"]:
                rho = (rho_c + (I1wx * u1 + I1wy * u2)).astype(F32)
                fi = (-rho / safe_grad).astype(F32)
                d1 = np.where(rho < -lt_grad, d1_lo, np.where(rho > lt_grad, d1_hi, np.where(small, F32(0), fi * I1wx)))
                d2 = np.where(rho < -lt_grad, d2_lo, np.where(rho > lt_grad, d2_hi, np.where(small, F32(0), fi * I1wy)))
                v1 = (u1 + d1).astype(F32)
                v2 = (u2 + d2).astype(F32)
                div1 = divergence(p11, p12)
                div2 = divergence(p21, p22)
                n1 = (v1 + theta * div1).astype(F32)
                n2 = (v2 + theta * div2).astype(F32)
                e1 = (n1 - u1).astype(F32)
                e2 = (n2 - u2).astype(F32)
                error = row_tree_error((e1 * e1 + e2 * e2).astype(F32))
                u1, u2 = n1, n2
                u1x, u1y = forward_gradient(u1)
                u2x, u2y = forward_gradient(u2)
                g1 = np.sqrt(u1x.astype(np.float64) ** 2 + u1y.astype(np.float64) ** 2).astype(F32)
                g2 = np.sqrt(u2x.astype(np.float64) ** 2 + u2y.astype(np.float64) ** 2).astype(F32)
                ng1 = (F32(1) + taut * g1).astype(F32)
                ng2 = (F32(1) + taut * g2).astype(F32)
                p11 = ((p11 + taut * u1x) / ng1).astype(F32)
                p12 = ((p12 + taut * u1y) / ng1).astype(F32)
                p21 = ((p21 + taut * u2x) / ng2).astype(F32)
                p22 = ((p22 + taut * u2y) / ng2).astype(F32)
                n_inner += 1
                counts_s[wi] += 1
            n_outer += 1
    return u1, u2


def tvl1_pair(i0, i1, prm=None):
    """One pair of u8 [h,w] images -> (flow float32 [h,w,2], inner iterations int32 [nscales, warps])."""
    p = params(**(prm or {}))
    if p["gamma"] != 0:
        raise ValueError("gamma != 0 is not restated")
    I0 = [np.asarray(i0, np.uint8).astype(F32)]
    I1 = [np.asarray(i1, np.uint8).astype(F32)]
    h, w = I0[0].shape
    sizes = pyramid_sizes(h, w, p["nscales"], p["scale_step"])
    for s in range(1, len(sizes)):
        I0.append(resize_scale(I0[-1], p["scale_step"]))
        I1.append(resize_scale(I1[-1], p["scale_step"]))
        assert I0[-1].shape == sizes[s]
    counts = np.zeros((p["nscales"], p["warps"]), np.int32)
    ns = len(sizes)
    u1 = np.zeros(sizes[-1], F32)
    u2 = np.zeros(sizes[-1], F32)
    mul = F32(1.0 / p["scale_step"])
    for s in range(ns - 1, -1, -1):
        u1, u2 = _one_scale(I0[s], I1[s], u1, u2, p, counts[s])
        if s == 0:
            break
        fh, fw = sizes[s - 1]
        u1 = (resize_to(u1, fw, fh) * mul).astype(F32)
        u2 = (resize_to(u2, fw, fh) * mul).astype(F32)
    return np.stack([u1, u2], axis=-1), counts


def tvl1_clip(gray, prm=None):
    """Every consecutive pair of a u8 [n,h,w] clip -> (flow [n-1,h,w,2], counts [n-1,nscales,warps])."""
    flows, counts = [], []
    for i in range(len(gray) - 1):
        f, c = tvl1_pair(gray[i], gray[i + 1], prm)
        flows.append(f)
        counts.append(c)
    return np.stack(flows), np.stack(counts)
