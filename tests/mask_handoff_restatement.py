"""NumPy restatement of the mask hand-off rules of include/vstab.h (vstab_mask_hold_batch, vstab_mask_grow_batch): hold, grow,
feather, count.  No product code is involved.  Everything is a maximum over integers -- the order keys of the floats, then
16-bit levels -- so the device's result must equal these functions in bits.

The ball of radius r around a pixel is walked row by row: for |dy| <= r the columns |dx| <= r - |dy| (tapered, the L1 ball) or
|dx| <= r (square, the L-infinity ball); a pixel outside the frame contributes the identity (the ball is clipped).  The
feather is stated through rings: max over q of [v(q) - dist * step] = max over d of [ballmax_d(v) - d * step], because a
pixel at distance dist lies in every ball of radius d >= dist and pays least at d = dist.  `grow_by_offsets` and
`feather_by_offsets` walk every offset of the ball one by one, `feather_iterated` relaxes one pixel at a time: the CPU tests
hold all forms against each other and against scipy."""

import numpy as np

HOLD_MAX, GROW_MAX, FEATHER_MAX = 16, 64, 64
FLAT_IDENT = np.int32(-2 ** 31)
CONE_IDENT = np.int32(-2 ** 30)
ONE_BITS = np.float32(1.0).view(np.int32)


def keys(m, nan_as_one=True):
    """float32 -> int32 order keys: a NaN reads as 1.0f, then v >= +0 keeps its bits and v <= -0 has its low 31 bits inverted,
    so that integer order is the floats' order with -0.0 below +0.0."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    b = m.view(np.int32).copy()
    if nan_as_one:
        b[np.isnan(m)] = ONE_BITS
    return b ^ ((b >> 31) & np.int32(0x7FFFFFFF))


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.int32)
    return (k ^ ((k >> 31) & np.int32(0x7FFFFFFF))).view(np.float32)


def q16(v):
    """The blended fill's quantiser on float32 (a NaN has been read as 1.0f before): v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) :
    65536) : 0."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = (np.where((v > 0) & (v < 1), v, np.float32(0)) * np.float32(65536.0)).astype(np.int32)   # truncating
    return np.where(v > 0, np.where(v < 1, scaled, 65536), 0).astype(np.int32)


def _shifted(a, dy, dx, ident):
    """out[..., y, x] = a[..., y + dy, x + dx] inside the frame, `ident` outside."""
    h, w = a.shape[-2:]
    out = np.full_like(a, ident)
    if abs(dy) >= h or abs(dx) >= w:
        return out
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def ball_max(k, r, tapered, ident):
    """The maximum of the integer array k [..., h, w] over the clipped ball of radius r, per frame."""
    if r == 0:
        return k.copy()
    rows = [k]                                             # rows[c] = max over |dx| <= c of k shifted by dx
    for c in range(1, r + 1):
        rows.append(np.maximum(rows[-1], np.maximum(_shifted(k, 0, c, ident), _shifted(k, 0, -c, ident))))
    out = np.full_like(k, ident)
    for dy in range(-r, r + 1):
        out = np.maximum(out, _shifted(rows[r - abs(dy)] if tapered else rows[r], dy, 0, ident))
    return out


def hold(m, T, shot=None):
    m = np.ascontiguousarray(m, dtype=np.float32)
    n = m.shape[0]
    assert 0 <= T <= HOLD_MAX
    if T == 0:
        return m.copy()
    shot = np.zeros(n, np.int64) if shot is None else np.asarray(shot, dtype=np.int64)
    assert shot.shape == (n,) and (np.diff(shot) >= 0).all()
    k = keys(m)
    out = np.empty_like(k)
    for i in range(n):
        js = [j for j in range(max(0, i - T), min(n, i + T + 1)) if shot[j] == shot[i]]
        out[i] = k[js].max(axis=0)
    return unkeys(out)


def grow(m, g, tapered=True):
    m = np.ascontiguousarray(m, dtype=np.float32)
    assert -GROW_MAX <= g <= GROW_MAX
    if g == 0:
        return m.copy()
    k = keys(m)
    if g < 0:
        return unkeys(~ball_max(~k, -g, tapered, FLAT_IDENT))   # ~ reverses the order: a minimum, identity +"infinity"
    return unkeys(ball_max(k, g, tapered, FLAT_IDENT))


def feather_step(f):
    return 65536 // (f + 1)


def feather(G, f, tapered=True):
    G = np.ascontiguousarray(G, dtype=np.float32)
    assert 0 <= f <= FEATHER_MAX
    if f == 0:
        return G.copy()
    q = q16(unkeys(keys(G)))                               # (a NaN reads as 1.0f)
    step = feather_step(f)
    best = np.zeros_like(q)
    for d in range(f + 1):
        best = np.maximum(best, ball_max(q, d, tapered, CONE_IDENT) - np.int32(d * step))
    return best.astype(np.float32) / np.float32(65536.0)


def count_above(out):
    out = np.asarray(out, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (out > np.float32(0.5)).reshape(out.shape[0], -1).sum(axis=1).astype(np.uint32)


def grow_feather(m, g, tapered=True, f=0):
    out = feather(grow(m, g, tapered), f, tapered)
    return out, count_above(out)


def handoff(m, T=0, g=0, tapered=True, f=0, shot=None):
    """hold, then grow, then feather -> (mask, counts)."""
    return grow_feather(hold(m, T, shot), g, tapered, f)


def shots_from_segments(segments, n):
    shot = np.zeros(n, np.int32)
    if segments is not None:
        for idx, (s, e) in enumerate(segments):
            shot[s:e] = idx
    return shot


# ---- the other forms, for the CPU tests ------------------------------------------------------------------------------------
def _offsets(r, tapered):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (abs(dx) + abs(dy) <= r if tapered else True)]


def grow_by_offsets(m, g, tapered=True):
    m = np.ascontiguousarray(m, dtype=np.float32)
    if g == 0:
        return m.copy()
    k = keys(m) if g > 0 else ~keys(m)
    out = np.full_like(k, FLAT_IDENT)
    for dy, dx in _offsets(abs(g), tapered):
        out = np.maximum(out, _shifted(k, dy, dx, FLAT_IDENT))
    return unkeys(out if g > 0 else ~out)


def feather_by_offsets(G, f, tapered=True):
    if f == 0:
        return np.ascontiguousarray(G, dtype=np.float32).copy()
    q = q16(unkeys(keys(G)))
    step = feather_step(f)
    best = np.zeros_like(q)
    for dy, dx in _offsets(f, tapered):
        dist = abs(dx) + abs(dy) if tapered else max(abs(dx), abs(dy))
        best = np.maximum(best, _shifted(q, dy, dx, CONE_IDENT) - np.int32(dist * step))
    return best.astype(np.float32) / np.float32(65536.0)


def feather_iterated(G, f, tapered=True):
    """f one-pixel relaxations: v <- max(v, max over the 4 or 8 in-frame neighbours of v - step), then max(0, .)."""
    if f == 0:
        return np.ascontiguousarray(G, dtype=np.float32).copy()
    q = q16(unkeys(keys(G)))
    step = np.int32(feather_step(f))
    near = [(dy, dx) for dy, dx in _offsets(1, tapered) if (dy, dx) != (0, 0)]
    for _ in range(f):
        nxt = q
        for dy, dx in near:
            nxt = np.maximum(nxt, _shifted(q, dy, dx, CONE_IDENT) - step)
        q = nxt
    return np.maximum(q, 0).astype(np.float32) / np.float32(65536.0)


# ---- the value table and the masks the tests draw ----------------------------------------------------------------------------
VALUES = np.array([0.0, 1.0, 0.25, 0.7, 1.0 / 3.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0)),
                   np.nextafter(np.float32(0.5), np.float32(1)), np.nan, np.inf, -np.inf, 2.5, -3.0, 2.0 ** -17, 1.0 - 2.0 ** -24],
                  np.float32)


def random_mask(shape, seed, sparse=False):
    """Draws from VALUES; sparse: mostly zeros, so that a radius has something to carry."""
    rng = np.random.default_rng(seed)
    m = VALUES[rng.integers(0, len(VALUES), size=shape)]
    if sparse:
        m = np.where(rng.random(shape) < 0.04, m, np.float32(0)).astype(np.float32)
    return np.ascontiguousarray(m, dtype=np.float32)


def corner_mask(n, h, w):
    m = np.zeros((n, h, w), np.float32)
    m[:, 0, 0] = m[:, 0, w - 1] = m[:, h - 1, 0] = m[:, h - 1, w - 1] = 1.0
    return m
