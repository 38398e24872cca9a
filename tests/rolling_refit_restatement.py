"""NumPy restatement of vstab_rectify_samples_batch's rule (include/vstab.h): the flow grid's samples as point pairs whose two
ends are corrected for the readout -- fp64, every operation rounded on its own, the ordered compaction of the admitted samples
and the NaN tail included -- and the helpers the refit tests share: a least-squares similarity fit of point pairs and the corner
errors of a chain of transitions, the analytic cases.  Nothing here imports the package.
"""

from __future__ import annotations

import numpy as np

from tests import rolling_shutter_restatement as R

MIN_DET = 0.25           # VSTAB_ROLLING_UNWARP_MIN_DET

# The analytic cases of the refit tests and their bounds (tests/test_rolling_refit_cpu.py says where the bounds come from).
STEP = 8
BIG = dict(n=12, w=480, h=270, rho=0.7, amp=(24.0, 20.0, 0.004, 0.004), omega=0.3, seed=4)
SMALL = dict(n=8, w=61, h=45, rho=0.7, amp=(3.0, 2.5, 0.004, 0.004), omega=0.3, seed=4)
CHAIN_BOUND = {"big": 0.25, "small": 0.35}     # chain error after one pass / chain error of the first pass
PAIR_BOUND = 0.25                              # the same for the mean pair error of the big case


def analytic_case(case):
    """-> (flows f32 [P,gh,gw,2]: the exact flow of every rolling pair at the stride-8 grid of the image itself, truth [P,3,3]:
    path.matrix(k + 1) @ inv(path.matrix(k)), the first pass: least-squares similarity transitions f32 [P,3,3])."""
    path = R.CameraPath(case["w"], case["h"], amp=case["amp"], omega=case["omega"], seed=case["seed"])
    pairs = case["n"] - 1
    flows = np.stack([R.rolling_flow_grid(path, k, case["rho"], STEP) for k in range(pairs)])
    truth = np.stack([path.matrix(k + 1) @ np.linalg.inv(path.matrix(k)) for k in range(pairs)])
    first = np.stack([R.least_squares_fit(flows[k], STEP, "similarity") for k in range(pairs)])
    return flows, truth, first


def inverse_displacement(x, y, velocity, readout, work_h):
    """e of the rule at the observed points (x, y) (fp64 arrays) of a frame with velocity fp64 [6] -> (ex, ey, solved):
    vstab_rolling_unwarp_batch's e, with the row that enters tau clamped to [0, work_h - 1] (a NaN stays a NaN)."""
    V = [np.float64(v) for v in np.asarray(velocity, dtype=np.float64).reshape(6)]
    rho, hm1 = np.float64(readout), np.float64(work_h - 1)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        yr = np.where(y < 0.0, 0.0, y)
        yr = np.where(yr > hm1, hm1, yr)
        tau = rho * (yr / hm1 - np.float64(0.5))
        a, b, c, d = np.float64(1.0) + tau * V[0], tau * V[1], tau * V[3], np.float64(1.0) + tau * V[4]
        det = a * d - b * c
        vx = (V[0] * x + V[1] * y) + V[2]
        vy = (V[3] * x + V[4] * y) + V[5]
        rx, ry = tau * vx, tau * vy
        ex = -((d * rx - b * ry) / det)
        ey = -((a * ry - c * rx) / det)
        solved = (det >= MIN_DET) & np.isfinite(ex) & np.isfinite(ey)
    return np.where(solved, ex, 0.0), np.where(solved, ey, 0.0), solved


def rectify_samples(grid_flow, step, work_size, velocity, readout, blocked=None):
    """grid_flow f32 [P,gh,gw,2], work_size (w, h), velocity f64 [P+1,6] in working px per frame, blocked u8 [P+1,gh,gw] | None
    -> (point_pairs f32 [P,gh*gw,4], counts i32 [P], unsolved u32 [P])."""
    grid = np.asarray(grid_flow, dtype=np.float32)
    pairs, gh, gw, _ = grid.shape
    V = np.asarray(velocity, dtype=np.float64).reshape(pairs + 1, 6)
    work_h = int(work_size[1])
    assert (gh, gw) == (-(-work_h // step), -(-int(work_size[0]) // step))
    px = (np.arange(gw) * int(step)).astype(np.float32)[None, :].repeat(gh, 0).ravel()
    py = (np.arange(gh) * int(step)).astype(np.float32)[:, None].repeat(gw, 1).ravel()
    out = np.full((pairs, gh * gw, 4), np.nan, np.float32)
    counts = np.zeros(pairs, np.int32)
    unsolved = np.zeros(pairs, np.uint32)
    for k in range(pairs):
        flow = grid[k].reshape(-1, 2)
        with np.errstate(all="ignore"):
            cx, cy = px + flow[:, 0], py + flow[:, 1]          # float32, the fit's own load
            assert cx.dtype == np.float32
        admitted = np.ones(gh * gw, bool)
        if blocked is not None:
            admitted = (np.asarray(blocked[k]).ravel() == 0) & (np.asarray(blocked[k + 1]).ravel() == 0)
        tracked = np.isfinite(cx) & np.isfinite(cy)
        ex, ey, ok_prev = inverse_displacement(px, py, V[k], readout, work_h)
        fx, fy, ok_next = inverse_displacement(cx, cy, V[k + 1], readout, work_h)
        with np.errstate(all="ignore"):
            rows = np.stack([(px.astype(np.float64) + ex).astype(np.float32), (py.astype(np.float64) + ey).astype(np.float32),
                             np.where(tracked, (cx.astype(np.float64) + fx).astype(np.float32), np.float32(np.nan)),
                             np.where(tracked, (cy.astype(np.float64) + fy).astype(np.float32), np.float32(np.nan))], axis=1)
        n = int(admitted.sum())
        out[k, :n] = rows[admitted]
        counts[k] = n
        unsolved[k] = int((~ok_prev & admitted).sum()) + int((~ok_next & tracked & admitted).sum())
    return out, counts, unsolved


def similarity_from_pairs(point_pairs, count):
    """The least-squares similarity next = A prev of the first `count` rows of one pair's table, NaN rows left out -> f64 [3,3]."""
    rows = np.asarray(point_pairs, dtype=np.float64)[: int(count)]
    rows = rows[np.isfinite(rows).all(axis=1)]
    x, y, X, Y = rows.T
    one, zero = np.ones_like(x), np.zeros_like(x)
    lhs = np.concatenate([np.stack([x, -y, one, zero], 1), np.stack([y, x, zero, one], 1)])
    a, b, tx, ty = np.linalg.lstsq(lhs, np.concatenate([X, Y]), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty], [0.0, 0.0, 1.0]])


def translation_from_pairs(point_pairs, count):
    rows = np.asarray(point_pairs, dtype=np.float64)[: int(count)]
    rows = rows[np.isfinite(rows).all(axis=1)]
    return np.array([[1.0, 0.0, (rows[:, 2] - rows[:, 0]).mean()], [0.0, 1.0, (rows[:, 3] - rows[:, 1]).mean()], [0.0, 0.0, 1.0]])


def corner_errors(transitions, truth, size):
    """transitions, truth [P,3,3] (frame k -> k+1), size (w, h) -> (per-pair error [P]: the largest corner displacement between
    a transition and its truth; chain error: the largest corner displacement between the two chains' products, over all
    frames).  px."""
    w, h = size
    corners = np.array([[0.0, 0.0, 1.0], [w - 1.0, 0.0, 1.0], [0.0, h - 1.0, 1.0], [w - 1.0, h - 1.0, 1.0]]).T

    def gap(A, B):
        d = (A @ corners - B @ corners)[:2]
        return float(np.sqrt((d * d).sum(axis=0)).max())

    pair = np.array([gap(np.asarray(a, np.float64), np.asarray(b, np.float64)) for a, b in zip(transitions, truth)])
    ca = cb = np.eye(3)
    chain = 0.0
    for a, b in zip(transitions, truth):
        ca, cb = np.asarray(a, np.float64) @ ca, np.asarray(b, np.float64) @ cb
        chain = max(chain, gap(ca, cb))
    return pair, chain
