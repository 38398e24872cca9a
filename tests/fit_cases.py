"""Model-fit cases shared by tests/test_fit_cases_cpu.py (the cases are what they claim, on the CPU oracle alone) and
tests/test_fit_paths_gpu.py (csrc/vstab_fit.hip and csrc/vstab_homography.hip against the oracle on every one of them), and
the oracle's records of each, computed once per session.

A grid case is (name, step, build, expect): build() -> (grid f32 [pairs,gh,gw,2], blocked u8 [pairs+1,gh,gw] or None).  The
oracle takes a dense field and samples it at stride `step`; field_of() embeds a grid in a field whose other positions are
NaN.  A masked case reaches the oracle as the grid with the samples blocked in either frame of a pair set to NaN.

What the cases are placed at (FIT_THREADS = 512 lanes compact `scan` = gh*gw samples in ranges of per = ceil(scan / 512); the
median is a 4 x 8-bit radix select over at most MAX_SORT = 16384 keys in LDS; nothing is computed below 12 valid samples;
similarity is accepted from confidence 0.1, perspective from 0.15; homography_kernel is a 256-lane block):

  counts      2x6 (12, the smallest that computes), 1x12 (12, collinear), 1x11 (nothing), 7x73 = 511, 16x32 = 512,
              3x171 = 513 (per becomes 2: lanes 257.. idle, lane 256 owns one sample), 15x17 = 255, 16x16 = 256,
              68x120 = 8160 (the 960x540 working size, per = 16), 128x128 = 16384 (MAX_SORT)
  sparse      34x60 (per = 4), all NaN but: 11 / 12 / 13 scattered valid samples; 12 within the ranges of the first four lanes
              (g < 16) and of the last four (g >= 2024); a mix of one-component NaN and +-inf around 40 valid samples;
              68x120 (per = 16): 12 within lane 0's range alone and within the last active lane's (509) alone
  median      hand-placed shifts, translation mode, compared with numpy: see _MEDIAN
  exact       zero flow, the integer translation (3, -2), two valid rows of constant 0.5
  collinear   one valid row, one valid column, gh == 1 -- as NaN and as a block grid: getSubset fails 10 000 times
  cut short   a full row and one sample off it: getSubset succeeds once, then fails -- the loop ends after iteration 0
  sweep       34x60, inlier shares 0.5 .. 0.05 around both acceptance thresholds, outliers uniform in +-40 px, two seeds
  large       flows of 1e4 px
  mixed       six pairs of different kinds in one batch, and the same six reversed
and point-pair tables for vstab_points_fit_batch (rows beyond counts[p] hold finite decoys that fit another model).
"""

import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name step build expect")

FIT_THREADS = 512
MAX_SORT = 16384
MODES = ("translation", "similarity", "perspective")


def camera_flow(gh, gw, step, seed, noise=0.15):
    """Smooth camera motion (similarity with a slight perspective) plus Gaussian noise, at the grid's sample positions."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:gh, 0:gw].astype(np.float64) * step
    th, s = rng.uniform(-0.01, 0.01), rng.uniform(0.99, 1.01)
    tx, ty = rng.uniform(-6, 6), rng.uniform(-4, 4)
    c, sn = s * np.cos(th), s * np.sin(th)
    g0, g1 = rng.uniform(-2e-5, 2e-5, 2)
    den = g0 * xx + g1 * yy + 1.0
    flow = np.stack([(c * xx - sn * yy + tx) / den - xx, (sn * xx + c * yy + ty) / den - yy], -1)
    return (flow + rng.normal(0, noise, flow.shape)).astype(np.float32)


def garbage_flow(gh, gw, seed):
    return np.random.default_rng(seed).uniform(-40, 40, (gh, gw, 2)).astype(np.float32)


def keep_only(flow, flat_indices):
    """`flow` with every sample but the listed ones (row-major g = gy * gw + gx) set to NaN."""
    out = np.full_like(flow, np.nan)
    idx = np.asarray(flat_indices, np.int64)
    out.reshape(-1, 2)[idx] = flow.reshape(-1, 2)[idx]
    return out


def field_of(grid, step):
    """One pair's grid [gh,gw,2] as the dense field the oracle samples at stride `step`: NaN off the sample positions."""
    gh, gw, _ = grid.shape
    if step == 1:
        return np.ascontiguousarray(grid, np.float32)
    field = np.full(((gh - 1) * step + 1, (gw - 1) * step + 1, 2), np.nan, np.float32)
    field[::step, ::step] = grid
    return field


def admitted(blocked):
    """[pairs,gh,gw] bool: the samples blocked in neither frame of a pair."""
    return (blocked[:-1] | blocked[1:]) == 0


def poisoned(grid, blocked):
    out = grid.copy()
    out[~admitted(blocked)] = np.nan
    return out


def shifts_of(grid, step):
    """The float32 shifts the translation fit takes its medians of: curr - prev = (prev + flow) - prev (flow.py:147,192),
    per valid sample -> [nv,2]."""
    gh, gw, _ = grid.shape
    ys, xs = np.mgrid[0:gh, 0:gw]
    prev = (np.stack([xs, ys], -1) * step).astype(np.float32)
    curr = prev + grid
    ok = np.isfinite(curr).all(-1)
    return (curr - prev)[ok]


# ---- counts -----------------------------------------------------------------------------------------------------------------
# (gh, gw, step): steps 1, 3, 8 and 16 across the table
COUNT_GRIDS = [(2, 6, 16), (1, 12, 1), (1, 11, 3), (7, 73, 8), (16, 32, 3), (3, 171, 8), (15, 17, 16), (16, 16, 1), (68, 120, 8),
           (128, 128, 3)]


def _count_case(gh, gw, step):
    return camera_flow(gh, gw, step, 1000 * gh + gw)[None], None


# ---- sparse -----------------------------------------------------------------------------------------------------------------
SPARSE_SHAPE = (34, 60)     # 2040 samples: per = 4, lanes 0..509 own [4t, 4t+4)
PROD_SHAPE = (68, 120)      # 8160 samples: per = 16, lanes 0..509 own [16t, 16t+16)


def _scattered(n, seed):
    gh, gw = SPARSE_SHAPE
    idx = np.random.default_rng(seed).choice(gh * gw, n, replace=False)
    return keep_only(camera_flow(gh, gw, 8, 77), idx)[None], None


def _ranged(shape, lo, hi, seed):
    """12 valid samples, all with lo <= g < hi."""
    gh, gw = shape
    idx = lo + np.random.default_rng(seed).choice(hi - lo, 12, replace=False)
    return keep_only(camera_flow(gh, gw, 8, 78), idx)[None], None


def _nonfinite_mix():
    gh, gw = SPARSE_SHAPE
    rng = np.random.default_rng(79)
    flow = camera_flow(gh, gw, 8, 79)
    kind = rng.integers(0, 6, (gh, gw))      # 0: NaN in x only, 1: NaN in y only, 2: +inf, 3: -inf, 4: NaN in both, 5: -inf in y
    valid = rng.choice(gh * gw, 40, replace=False)
    out = flow.copy()
    out[kind == 0, 0] = np.nan
    out[kind == 1, 1] = np.nan
    out[kind == 2, 0] = np.inf
    out[kind == 3, 0] = -np.inf
    out[kind == 4] = np.nan
    out[kind == 5, 1] = -np.inf
    out.reshape(-1, 2)[valid] = flow.reshape(-1, 2)[valid]
    return out[None], None


_SPARSE = [
    ("sparse-11", 8, functools.partial(_scattered, 11, 1), {"nv": [11]}),
    ("sparse-12", 8, functools.partial(_scattered, 12, 2), {"nv": [12]}),
    ("sparse-13", 8, functools.partial(_scattered, 13, 3), {"nv": [13]}),
    ("sparse-first-lanes", 8, functools.partial(_ranged, SPARSE_SHAPE, 0, 16, 4), {"nv": [12], "collinear": [0]}),
    ("sparse-last-lanes", 8, functools.partial(_ranged, SPARSE_SHAPE, 2024, 2040, 5), {"nv": [12], "collinear": [0]}),
    ("sparse-lane-0", 8, functools.partial(_ranged, PROD_SHAPE, 0, 16, 6), {"nv": [12], "collinear": [0]}),
    ("sparse-lane-509", 8, functools.partial(_ranged, PROD_SHAPE, 8144, 8160, 7), {"nv": [12], "collinear": [0]}),
    ("sparse-nonfinite-mix", 8, _nonfinite_mix, {"nv": [40]}),
]

# ---- median -----------------------------------------------------------------------------------------------------------------
# x shifts in ascending order; they are placed on a gh x 1 grid (prev.x = 0: the shift is the flow value itself) in a drawn
# order, the y shifts are the same values in another order.  All are multiples of 2^-4 but for the nextafter pair, which only
# the x axis carries (y is 0 there).
_NEXT = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
_MEDIAN = [
    ("median-all-equal", [1.25] * 16),
    ("median-middle-inside-a-run", [-3.0] * 5 + [2.0] * 8 + [5.0] * 3),            # both middles 2.0; 5 keys below, mid = 8
    ("median-middle-straddles-two-runs", [1.0] * 8 + [3.0] * 8),                   # exactly mid keys below, all tied
    ("median-middle-across-zero", [-9.0, -7.5, -4.0, -4.0, -2.0, -1.0, -0.5, -0.25, 0.25, 0.5, 1.0, 1.0, 3.0, 6.0, 6.5, 8.0]),
    ("median-middle-one-ulp-apart", [0.5] * 7 + [1.0, _NEXT] + [1.5] * 7),         # same top three key bytes
    ("median-odd-count", [-2.0] * 4 + [0.75] * 5 + [1.0] * 6),                     # 15 samples, rank 7 is 0.75
    ("median-signed-zeros", [-0.0] * 8 + [0.0] * 8),
]


def _median_case(values):
    v = np.asarray(values, np.float32)
    rng = np.random.default_rng(len(values) * 31 + int(abs(float(v.sum())) * 16))
    grid = np.zeros((1, len(v), 1, 2), np.float32)
    grid[0, :, 0, 0] = v[rng.permutation(len(v))]
    if not np.any(v == np.float32(_NEXT)):
        grid[0, :, 0, 1] = v[rng.permutation(len(v))]
    return grid, None


def _median_quantised(odd):
    gh, gw = SPARSE_SHAPE
    rng = np.random.default_rng(90)
    grid = (rng.integers(-6, 7, (1, gh, gw, 2)) * 0.5).astype(np.float32)
    if odd:
        grid[0, 17, 31] = np.nan
    return grid, None


# ---- exact data, collinear ----------------------------------------------------------------------------------------------------
def _exact():
    gh, gw = SPARSE_SHAPE
    grid = np.zeros((3, gh, gw, 2), np.float32)
    grid[1] = (3.0, -2.0)
    grid[2] = np.nan
    grid[2, 9] = 0.5
    grid[2, 20] = 0.5
    return grid, None


COLLINEAR_ROW, COLLINEAR_COLUMN = 5, 7


def _collinear(masked):
    gh, gw = SPARSE_SHAPE
    grid = np.stack([camera_flow(gh, gw, 8, 60), camera_flow(gh, gw, 8, 61)])
    row = np.zeros((gh, gw), bool)
    row[COLLINEAR_ROW] = True
    col = np.zeros((gh, gw), bool)
    col[:, COLLINEAR_COLUMN] = True
    if not masked:
        grid[0, ~row] = np.nan
        grid[1, ~col] = np.nan
        return grid, None
    blocked = np.zeros((3, gh, gw), np.uint8)
    blocked[0, ~row] = 1
    blocked[1, 20:25, 30:40] = 1            # off the row and off the column: blocks nothing that the others admit
    blocked[2, ~col] = 1
    return grid, blocked


def _single_row(masked):
    grid = camera_flow(1, 40, 3, 62)[None]
    if not masked:
        return grid, None
    blocked = np.zeros((2, 1, 40), np.uint8)
    blocked[0, 0, ::3] = 1
    blocked[1, 0, 5:9] = 1
    return grid, blocked


def _line_and_one_sample():
    """A 2 x 3000 grid at step 1.  Row 0 is complete: a quarter of it follows the camera motion, the rest is uniform in +-40 px.
    Row 1 has ONE valid sample.  A 4-point subset passes checkSubset only with that sample drawn last (1 attempt in ~3000, less
    the orientation test): with OpenCV's RNG stream getSubset succeeds once -- a degenerate sample whose model has 6 inliers here --
    and then fails all 10 000 attempts of iteration 1, which ends the loop (`break`; seen with a print in a scratch build of
    oracle/vo_fit.c).  Perspective is computed from those few and refused: a confidence above 0 says that the failure did not come
    at iteration 0.  A loop that went on drawing instead would find the camera model later (597 inliers of 3001, accepted: the same
    scratch build with `continue` in place of `break`)."""
    gw = 3000
    rng = np.random.default_rng(2000)
    line = camera_flow(1, gw, 1, 2001)[0]
    bad = rng.random(gw) >= 0.25
    line[bad] = rng.uniform(-40, 40, (int(bad.sum()), 2))
    grid = np.full((1, 2, gw, 2), np.nan, np.float32)
    grid[0, 0] = line
    grid[0, 1, 17] = line[np.flatnonzero(~bad)[0]]
    return grid, None


# ---- threshold sweep ------------------------------------------------------------------------------------------------------------
SWEEP_SHARES = (0.5, 0.17, 0.14, 0.12, 0.09, 0.05)
# at a share of 0.14 the 2000 4-point draws hold an all-inlier sample about one time in two: with these seeds they do at 0.14
# (perspective finds the camera model and is refused at 0.14 < 0.15) and do not at 0.12 (the loop ends at its cap without it)
SWEEP_SEEDS = (2, 8)


def _sweep(seed):
    """Per pair: round(share * 2040) drawn samples follow the camera motion (noise 0.15 px), every other sample is uniform in
    +-40 px on both axes."""
    gh, gw = SPARSE_SHAPE
    rng = np.random.default_rng(500 + seed)
    pairs = []
    for i, share in enumerate(SWEEP_SHARES):
        flow = camera_flow(gh, gw, 8, 510 + 10 * seed + i)
        out = rng.uniform(-40, 40, flow.shape).astype(np.float32)
        inl = rng.choice(gh * gw, int(round(share * gh * gw)), replace=False)
        out.reshape(-1, 2)[inl] = flow.reshape(-1, 2)[inl]
        pairs.append(out)
    return np.stack(pairs), None


def _large():
    gh, gw = SPARSE_SHAPE
    grid = np.stack([camera_flow(gh, gw, 8, 70), camera_flow(gh, gw, 8, 71)])
    grid[0] += np.float32(1e4)
    grid[1] -= np.array([1e4, 0.5e4], np.float32)
    return grid, None


# ---- heterogeneous batch ----------------------------------------------------------------------------------------------------
MIXED_KINDS = ("nothing", "clean", "collinear", "twelve", "garbage", "static")


def _mixed(reverse):
    gh, gw = SPARSE_SHAPE
    base = camera_flow(gh, gw, 8, 80)
    rng = np.random.default_rng(81)
    row = np.full_like(base, np.nan)
    row[COLLINEAR_ROW] = base[COLLINEAR_ROW]
    pairs = [
        keep_only(base, rng.choice(gh * gw, 11, replace=False)),
        camera_flow(gh, gw, 8, 82),
        row,
        keep_only(base, rng.choice(gh * gw, 12, replace=False)),
        garbage_flow(gh, gw, 83),
        np.zeros_like(base),
    ]
    if reverse:
        pairs = pairs[::-1]
    return np.stack(pairs), None


_MIXED_NV = [11, 2040, 60, 12, 2040, 2040]


def _build_cases():
    cases = {}

    def add(name, step, build, expect):
        cases[name] = Case(name, step, build, expect)

    for gh, gw, step in COUNT_GRIDS:
        add(f"count-{gh}x{gw}", step, functools.partial(_count_case, gh, gw, step),
            {"nv": [gh * gw], "collinear": [0] if gh == 1 and gw >= 12 else []})
    for name, step, build, expect in _SPARSE:
        add(name, step, build, expect)
    for name, values in _MEDIAN:
        add(name, 8, functools.partial(_median_case, values), {"nv": [len(values)], "median": True})
    add("median-quantised-even", 16, functools.partial(_median_quantised, False), {"nv": [2040], "median": True})
    add("median-quantised-odd", 16, functools.partial(_median_quantised, True), {"nv": [2039], "median": True})
    add("exact", 16, _exact, {"nv": [2040, 2040, 120], "exact": [(0.0, 0.0), (3.0, -2.0), (0.5, 0.5)], "both_forms": True})
    add("collinear-nan", 8, functools.partial(_collinear, False), {"nv": [60, 34], "collinear": [0, 1], "both_forms": True})
    add("collinear-masked", 8, functools.partial(_collinear, True), {"nv": [60, 34], "collinear": [0, 1], "both_forms": True})
    add("single-row", 3, functools.partial(_single_row, False), {"nv": [40], "collinear": [0], "both_forms": True})
    add("single-row-masked", 3, functools.partial(_single_row, True), {"nv": [23], "collinear": [0], "both_forms": True})
    add("line-and-one-sample", 1, _line_and_one_sample, {"nv": [3001], "cut_short": [0]})
    for seed in SWEEP_SEEDS:
        add(f"sweep-{seed}", 8, functools.partial(_sweep, seed), {"nv": [2040] * len(SWEEP_SHARES), "sweep": True})
    add("large-flows", 8, _large, {"nv": [2040, 2040]})
    add("mixed", 8, functools.partial(_mixed, False), {"nv": _MIXED_NV, "collinear": [2], "both_forms": True})
    add("mixed-reversed", 8, functools.partial(_mixed, True), {"nv": _MIXED_NV[::-1], "collinear": [3], "both_forms": True})
    return cases


CASES = _build_cases()
CASE_IDS = tuple(CASES)
MEDIAN_IDS = tuple(c for c in CASE_IDS if CASES[c].expect.get("median"))
SWEEP_IDS = tuple(c for c in CASE_IDS if CASES[c].expect.get("sweep"))
BOTH_FORMS_IDS = tuple(c for c in CASE_IDS if CASES[c].expect.get("both_forms"))
# 2040-sample grids take the oracle a few ms per mode; the median cases are about the translation record alone
CASE_MODES = {c: (("translation",) if CASES[c].expect.get("median") else MODES) for c in CASE_IDS}


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(grid f32 [pairs,gh,gw,2], blocked u8 [pairs+1,gh,gw] or None), read-only."""
    grid, blocked = CASES[case_id].build()
    grid = np.ascontiguousarray(grid, np.float32)
    grid.setflags(write=False)
    if blocked is not None:
        blocked = np.ascontiguousarray(blocked, np.uint8)
        assert blocked.shape == (grid.shape[0] + 1,) + grid.shape[1:3]
        blocked.setflags(write=False)
    return grid, blocked


@functools.lru_cache(maxsize=None)
def effective_grid(case_id):
    """The grid the fit sees: the case's grid, with the samples its block grid takes out set to NaN."""
    grid, blocked = inputs(case_id)
    if blocked is None:
        return grid
    out = poisoned(grid, blocked)
    out.setflags(write=False)
    return out


def admitted_counts(case_id):
    grid, blocked = inputs(case_id)
    if blocked is None:
        return [grid.shape[1] * grid.shape[2]] * grid.shape[0]
    return [int(a.sum()) for a in admitted(blocked)]


@functools.lru_cache(maxsize=None)
def oracle_records(case_id, mode):
    """Per pair (records {mode name: dict}, valid points, total points) of oracle.fit_all_modes on the effective grid.  The
    oracle knows no block grid: its total is gh*gw, and so is the denominator of its translation confidence."""
    from oracle import oracle as O

    O.build()
    step = CASES[case_id].step
    return tuple(O.fit_all_modes(field_of(g, step), step, mode) for g in effective_grid(case_id))


def ransac_iterations(confidence, model_points, cap=2000):
    """RANSACUpdateNumIters (calib3d/src/ptsetreg.cpp) at p = 0.992 for a best model with this inlier share: the iteration
    count the loop is left with; `cap` = it runs to its limit."""
    if confidence <= 0.0:
        return cap
    denom = 1.0 - confidence ** model_points
    if denom <= 0.0:
        return 0
    need = np.log(1.0 - 0.992) / np.log(denom)
    return cap if need >= cap else int(np.rint(need))


# ---- point-pair tables ----------------------------------------------------------------------------------------------------------
POINT_CAPS = (64, 400)
POINT_KINDS = ("count-0", "count-11", "count-12", "twelve-7-tracked", "twelve-8-tracked", "duplicate-prev", "prev-on-a-line", "full")


def similar_tracks(rng, prev, noise=0.2):
    th, s = rng.uniform(-0.02, 0.02), rng.uniform(0.98, 1.02)
    A = np.array([[s * np.cos(th), -s * np.sin(th)], [s * np.sin(th), s * np.cos(th)]])
    return prev @ A.T + rng.uniform(-5, 5, 2) + rng.normal(0, noise, prev.shape)


@functools.lru_cache(maxsize=None)
def point_table(cap):
    """-> (table f32 [P,cap,4], counts i32 [P], per pair (prev [k,2], next [k,2], status u8 [k])), read-only.  Row layout:
    prev.x, prev.y, next.x, next.y; a lost track has NaN in next.  Rows beyond counts[p] are DECOYS: finite point pairs under
    one tight model of their own (a shift by (+31, -17)), enough of them to win every RANSAC and move every median if read."""
    rng = np.random.default_rng(1100 + cap)
    pairs = []
    for kind in POINT_KINDS:
        count = {"count-0": 0, "count-11": 11, "count-12": 12, "twelve-7-tracked": 12, "twelve-8-tracked": 12,
                 "duplicate-prev": 30, "prev-on-a-line": 30, "full": cap}[kind]
        prev = rng.uniform(0, 1, (count, 2)) * [854, 480]
        if kind == "duplicate-prev":
            prev[10:20] = prev[0:10]                      # ten points detected twice: a 2-point sample of one is degenerate
        if kind == "prev-on-a-line":                      # exactly: multiples of 4 in x, y = x / 4 + 40 is exact in float32
            prev[:, 0] = 4.0 * rng.choice(200, count, replace=False)
            prev[:, 1] = 0.25 * prev[:, 0] + 40.0
        nxt = similar_tracks(rng, prev) if count else prev.copy()
        status = np.ones(count, np.uint8)
        if kind == "twelve-7-tracked":
            status[[1, 4, 6, 9, 11]] = 0
        elif kind == "twelve-8-tracked":
            status[[1, 4, 6, 9]] = 0
        elif kind == "full":
            status = (rng.random(count) >= 0.1).astype(np.uint8)
            bad = rng.random(count) < 0.25
            nxt[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
        pairs.append((prev.astype(np.float32), nxt.astype(np.float32), status))
    table = np.zeros((len(pairs), cap, 4), np.float32)
    decoy_prev = rng.uniform(0, 1, (len(pairs), cap, 2)) * [854, 480]
    table[..., :2] = decoy_prev
    table[..., 2:] = decoy_prev + [31.0, -17.0]
    counts = np.zeros(len(pairs), np.int32)
    for i, (prev, nxt, status) in enumerate(pairs):
        k = len(prev)
        counts[i] = k
        table[i, :k, :2] = prev
        table[i, :k, 2:] = np.where(status[:, None] == 1, nxt, np.nan)
    assert np.isfinite(table[np.arange(cap)[None, :] >= counts[:, None]]).all()
    table.setflags(write=False)
    counts.setflags(write=False)
    return table, counts, tuple(pairs)


@functools.lru_cache(maxsize=None)
def oracle_point_records(cap, mode):
    from oracle import oracle as O

    O.build()
    _, _, pairs = point_table(cap)
    return tuple(O.fit_all_modes_points(prev, nxt, status, mode) for prev, nxt, status in pairs)


# ---- known models, for the oracle-independent recovery test ---------------------------------------------------------------------
KNOWN_GRIDS = ((3, 171, 8), (68, 120, 8))


def known_model_grid(gh, gw, step, perspective, seed):
    """Noise-free correspondences of a known model under 30 % gross outliers (5 .. 40 px off on both axes: none within the
    RANSAC thresholds) -> (grid f32 [1,gh,gw,2], model 3x3 float64).  The flow is rounded to float32, the input format."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:gh, 0:gw].astype(np.float64) * step
    cx, cy = (gw - 1) * step / 2.0, (gh - 1) * step / 2.0
    th, s = (0.004, 1.003) if not perspective else (-0.003, 0.998)
    c, sn = s * np.cos(th), s * np.sin(th)
    tx, ty = (3.2, -1.7) if not perspective else (2.1, 1.3)
    model = np.array([[c, -sn, cx - c * cx + sn * cy + tx], [sn, c, cy - sn * cx - c * cy + ty], [0.0, 0.0, 1.0]])
    if perspective:
        model[2, 0], model[2, 1] = 3e-6, -2e-6
    den = model[2, 0] * xx + model[2, 1] * yy + 1.0
    qx = (model[0, 0] * xx + model[0, 1] * yy + model[0, 2]) / den
    qy = (model[1, 0] * xx + model[1, 1] * yy + model[1, 2]) / den
    flow = np.stack([qx - xx, qy - yy], -1)
    bad = rng.random((gh, gw)) < 0.3
    flow[bad] += rng.uniform(5, 40, (int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
    return flow.astype(np.float32)[None], model


def oracle_records_of(grid, step, mode):
    from oracle import oracle as O

    O.build()
    return O.fit_all_modes(field_of(grid, step), step, mode)


# the bounds of tests/test_referee_cpu.py for float32 inputs: similarity (linear part, translation), perspective (transfer, px)
KNOWN_BOUNDS = {False: (2e-7, 1e-4), True: (2e-4,)}


def known_model_errors(matrix, model, gh, gw, step, perspective):
    """Similarity: (max error of the linear part, max error of the translation).  Perspective: (max point-transfer error, px,
    at the grid's four corners and its centre)."""
    m = np.asarray(matrix, np.float64)
    if not perspective:
        return float(np.abs(m[:2, :2] - model[:2, :2]).max()), float(np.abs(m[:2, 2] - model[:2, 2]).max())
    w, h = (gw - 1) * step, (gh - 1) * step
    pts = np.array([[0, 0], [w, 0], [0, h], [w, h], [w / 2.0, h / 2.0]], np.float64)

    def project(H):
        z = pts @ H[2, :2] + H[2, 2]
        return (pts @ H[:2, :2].T + H[:2, 2]) / z[:, None]

    return (float(np.abs(project(m) - project(model)).max()),)
