"""The cases of tests/fit_cases.py are what they claim, shown on the CPU oracle alone (no GPU): the valid counts they state, the
branch of the compaction their samples fall in, the collinear ones refused by getSubset, the sweep on both sides of both
acceptance thresholds, the tie patterns equal to numpy's float32 median, the exact data fitted exactly.  These are conditions
on the cases, not measurements: a case that fails one is replaced, not loosened."""

import numpy as np
import pytest

from tests import fit_cases as C


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case_id", C.CASE_IDS)
def test_case_has_its_stated_counts(oracle, case_id):
    case = C.CASES[case_id]
    grid, blocked = C.inputs(case_id)
    assert grid.ndim == 4 and grid.shape[3] == 2 and grid.shape[1] * grid.shape[2] <= C.MAX_SORT
    assert len(case.expect["nv"]) == grid.shape[0]
    for mode in C.CASE_MODES[case_id]:
        for p, (ref, nv, nt) in enumerate(C.oracle_records(case_id, mode)):
            assert nv == case.expect["nv"][p], (case_id, p, nv)
            assert nt == grid.shape[1] * grid.shape[2]
            assert nv == len(C.shifts_of(C.effective_grid(case_id)[p], case.step))
            wanted = set(C.MODES[:C.MODES.index(mode) + 1]) if nv >= 12 else set()
            assert set(ref) == wanted, (case_id, mode, p, set(ref))
    if blocked is not None:
        for p, count in enumerate(C.admitted_counts(case_id)):
            assert case.expect["nv"][p] <= count < grid.shape[1] * grid.shape[2]


def test_count_cases_sit_at_the_compaction_thresholds():
    per = lambda scan: -(-scan // C.FIT_THREADS)
    scans = {gh * gw for gh, gw, _ in C.COUNT_GRIDS}
    assert {11, 12, 255, 256, C.FIT_THREADS - 1, C.FIT_THREADS, C.FIT_THREADS + 1, 8160, C.MAX_SORT} <= scans
    assert per(511) == per(512) == 1 and per(513) == 2 and per(8160) == 16 and per(C.MAX_SORT) == 32
    assert -(-513 // per(513)) == 257 and 513 - 256 * per(513) == 1     # 257 active lanes, the last one owns one sample
    assert {step for _, step, *_ in C.CASES.values()} >= {1, 3, 8, 16}


def test_sparse_cases_lie_in_the_stated_lane_ranges():
    def lanes(case_id):
        grid = C.inputs(case_id)[0][0]
        scan = grid.shape[0] * grid.shape[1]
        g = np.flatnonzero(np.isfinite(grid).all(-1).ravel())
        return set((g // -(-scan // C.FIT_THREADS)).tolist())

    assert lanes("sparse-first-lanes") <= {0, 1, 2, 3} and len(lanes("sparse-first-lanes")) > 1
    assert lanes("sparse-last-lanes") <= {506, 507, 508, 509} and len(lanes("sparse-last-lanes")) > 1
    assert lanes("sparse-lane-0") == {0}
    assert lanes("sparse-lane-509") == {509}            # the last lane with samples: 510 * 16 = 8160
    assert len(lanes("sparse-12")) >= 10                # scattered: (almost) one lane each
    mix = C.inputs("sparse-nonfinite-mix")[0][0]
    one = np.isnan(mix[..., 0]) ^ np.isnan(mix[..., 1])
    assert one.sum() > 100 and np.isposinf(mix).any() and np.isneginf(mix).any()
    assert (np.isfinite(mix[..., 0]) & ~np.isfinite(mix[..., 1])).any() and (~np.isfinite(mix[..., 0]) & np.isfinite(mix[..., 1])).any()


@pytest.mark.parametrize("case_id", [c for c in C.CASE_IDS if C.CASES[c].expect.get("collinear")])
def test_collinear_pairs_compute_a_refused_perspective(oracle, case_id):
    """Every valid sample of the pair lies on one line: getSubset fails at the first iteration, findHomography returns nothing
    -- the record is computed, not accepted, confidence 0 -- while similarity is accepted."""
    recs = C.oracle_records(case_id, "perspective")
    for p in C.CASES[case_id].expect["collinear"]:
        ref, nv, _ = recs[p]
        grid = C.effective_grid(case_id)[p]
        ys, xs = np.nonzero(np.isfinite(grid).all(-1))
        assert len(set(ys.tolist())) == 1 or len(set(xs.tolist())) == 1
        assert ref["perspective"]["accepted"] is False and ref["perspective"]["confidence"] == 0.0
        assert ref["similarity"]["accepted"] is True and ref["translation"]["accepted"] is True


def test_loop_cut_short_by_getsubset_leaves_a_refused_perspective(oracle):
    """fit_cases._line_and_one_sample: every valid sample but one on a line, a quarter of them under one camera model.  The
    similarity fit finds that model; the homography loop, ended by getSubset's failure after its first iteration, is left with
    the few inliers of a degenerate sample."""
    (ref, nv, _), = C.oracle_records("line-and-one-sample", "perspective")
    grid = C.inputs("line-and-one-sample")[0][0]
    valid = np.isfinite(grid).all(-1)
    assert valid[0].all() and valid[1].sum() == 1 and nv == valid.sum()
    # 6 of 3001 with glibc's hypot; the count of a degenerate sample's model hangs on the last bit (tests/test_fit_paths_gpu.py)
    assert ref["perspective"]["accepted"] is False and ref["perspective"]["confidence"] <= 0.05
    assert ref["similarity"]["accepted"] is True and ref["similarity"]["confidence"] > 0.15


def test_sweep_lies_on_both_sides_of_both_thresholds(oracle):
    sim, per, between, capped = [], [], [], []
    for case_id in C.SWEEP_IDS:
        for p, (ref, nv, _) in enumerate(C.oracle_records(case_id, "perspective")):
            s, h = ref["similarity"], ref["perspective"]
            assert s["accepted"] == (s["confidence"] >= 0.1) and h["accepted"] == (h["confidence"] >= 0.15)
            sim.append(s["confidence"])
            per.append(h["confidence"])
            if s["accepted"] and not h["accepted"]:
                between.append((case_id, p))
            # the loop's iteration count follows from the best model's inlier share: 4-point RANSAC below a share of 0.22
            # never gets under its 2000-iteration cap, 2-point RANSAC does from 0.05
            if s["accepted"] and C.ransac_iterations(h["confidence"], 4) == 2000 and C.ransac_iterations(s["confidence"], 2) < 2000:
                capped.append((case_id, p))
    assert min(sim) < 0.1 <= max(sim) and min(sim) > 0.0
    assert min(per) < 0.15 <= max(per)
    assert any(0.1 <= s < 0.15 for s in sim)
    assert any(0.1 <= h < 0.15 for h in per), per       # found the model, refused: a threshold of 0.1 would accept it
    assert between and capped, (sim, per)
    # a homography RANSAC that ran to its cap WITHOUT finding the camera model: far fewer inliers than similarity found
    assert any(s >= 0.1 and h < 0.75 * s for s, h in zip(sim, per)), (sim, per)


@pytest.mark.parametrize("case_id", C.MEDIAN_IDS)
def test_tie_cases_equal_numpy_median_bit_for_bit(oracle, case_id):
    grid = C.inputs(case_id)[0]
    (ref, nv, nt), = C.oracle_records(case_id, "translation")
    s = C.shifts_of(grid[0], C.CASES[case_id].step)
    assert s.dtype == np.float32 and len(s) == nv
    # the shifts are exactly the hand-placed flow values
    assert np.array_equal(s, grid[0][np.isfinite(grid[0]).all(-1)])
    want = np.array([np.float32(np.median(s[:, 0])), np.float32(np.median(s[:, 1]))], np.float32)
    m = ref["translation"]["matrix"]
    assert np.array_equal(_bits(m[:2, 2]), _bits(want)), (m[:2, 2], want)
    assert np.array_equal(m[:2, :2], np.eye(2, dtype=np.float32))


def test_tie_cases_hold_the_stated_patterns():
    def middles(case_id, axis=0):
        v = np.sort(C.shifts_of(C.inputs(case_id)[0][0], C.CASES[case_id].step)[:, axis])
        return v, v[len(v) // 2 - 1], v[len(v) // 2]

    v, lo, hi = middles("median-all-equal")
    assert lo == hi == v[0] == v[-1]
    v, lo, hi = middles("median-middle-inside-a-run")
    assert lo == hi and 0 < (v < hi).sum() < len(v) // 2            # fewer than mid keys below: the lower middle duplicates hi
    v, lo, hi = middles("median-middle-straddles-two-runs")
    assert lo < hi and (v < hi).sum() == len(v) // 2 and (v == lo).sum() > 1 and (v == hi).sum() > 1
    v, lo, hi = middles("median-middle-across-zero")
    assert (lo, hi) == (-0.25, 0.25)
    v, lo, hi = middles("median-middle-one-ulp-apart")
    assert lo == 1.0 and hi == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert (_bits([lo])[0] >> 8) == (_bits([hi])[0] >> 8)           # the last radix pass decides
    v, lo, hi = middles("median-odd-count")
    assert len(v) % 2 == 1 and (v == v[len(v) // 2]).sum() > 1
    raw = C.inputs("median-signed-zeros")[0][0, :, 0, 0]
    assert np.signbit(raw).sum() == 8 and not raw.any()
    for case_id, odd in (("median-quantised-even", 0), ("median-quantised-odd", 1)):
        for axis in (0, 1):
            v, lo, hi = middles(case_id, axis)
            assert len(v) % 2 == odd and len(np.unique(v)) == 13 and np.array_equal(v * 2, np.rint(v * 2))


def test_exact_data_is_fitted_exactly(oracle):
    recs = C.oracle_records("exact", "perspective")
    for (ref, nv, _), (tx, ty) in zip(recs, C.CASES["exact"].expect["exact"]):
        want = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
        for name in C.MODES:
            assert ref[name]["accepted"] and ref[name]["residual"] < 1e-9, (name, ref[name])
            assert np.abs(ref[name]["matrix"].astype(np.float64) - want).max() < 1e-9, (name, ref[name]["matrix"])
        assert ref["similarity"]["confidence"] == 1.0 and ref["perspective"]["confidence"] == 1.0


def test_mixed_batches_hold_the_stated_kinds(oracle):
    fwd = C.oracle_records("mixed", "perspective")
    rev = C.oracle_records("mixed-reversed", "perspective")
    assert np.array_equal(C.inputs("mixed")[0][::-1], C.inputs("mixed-reversed")[0], equal_nan=True)
    for (ref, nv, _), (ref_r, nv_r, _) in zip(fwd, rev[::-1]):
        assert nv == nv_r and set(ref) == set(ref_r)
    by_kind = dict(zip(C.MIXED_KINDS, fwd))
    assert by_kind["nothing"][0] == {} and by_kind["nothing"][1] == 11
    assert all(by_kind["clean"][0][m]["accepted"] for m in C.MODES)
    assert by_kind["twelve"][1] == 12 and set(by_kind["twelve"][0]) == set(C.MODES)
    assert not by_kind["garbage"][0]["similarity"]["accepted"] and not by_kind["garbage"][0]["perspective"]["accepted"]
    assert np.abs(by_kind["static"][0]["perspective"]["matrix"].astype(np.float64) - np.eye(3)).max() < 1e-9


def test_large_flows_stay_finite_in_float32():
    grid = C.inputs("large-flows")[0]
    assert np.abs(grid).max() > 9e3 and np.isfinite(np.square(grid, dtype=np.float32) * np.float32(4)).all()


@pytest.mark.parametrize("cap", C.POINT_CAPS)
def test_point_tables_hold_the_stated_pairs(oracle, cap):
    table, counts, pairs = C.point_table(cap)
    assert counts.tolist() == [0, 11, 12, 12, 12, 30, 30, cap]
    recs = dict(zip(C.POINT_KINDS, C.oracle_point_records(cap, "perspective")))
    assert [recs[k][1] for k in C.POINT_KINDS[:5]] == [0, 11, 12, 7, 8]
    for kind in ("count-0", "count-11", "twelve-7-tracked"):
        assert recs[kind][0] == {}
    for kind in ("count-12", "twelve-8-tracked", "duplicate-prev", "full"):
        assert set(recs[kind][0]) == set(C.MODES) and all(recs[kind][0][m]["accepted"] for m in C.MODES), kind
    line = recs["prev-on-a-line"][0]
    assert line["perspective"]["accepted"] is False and line["perspective"]["confidence"] == 0.0 and line["similarity"]["accepted"]
    prev = pairs[C.POINT_KINDS.index("duplicate-prev")][0]
    assert np.array_equal(prev[10:20], prev[0:10])
    # the decoys beyond counts[p] would change every fit if they were read: with them the oracle answers otherwise
    from oracle import oracle as O

    for i, kind in enumerate(C.POINT_KINDS):
        if counts[i] == cap:
            continue
        status = np.isfinite(table[i, :, 2:]).all(-1).astype(np.uint8)
        with_decoys, nv = O.fit_all_modes_points(table[i, :, :2], np.nan_to_num(table[i, :, 2:]), status, "perspective")
        assert nv > recs[kind][1] and set(with_decoys) == set(C.MODES)
        for m in C.MODES:
            honest = recs[kind][0].get(m)
            assert honest is None or not np.array_equal(honest["matrix"], with_decoys[m]["matrix"]), (kind, m)


def test_known_models_are_recovered_by_the_oracle(oracle):
    """The recovery bounds of tests/test_referee_cpu.py hold for the oracle on the grids the GPU test uses."""
    for gh, gw, step in C.KNOWN_GRIDS:
        for perspective in (False, True):
            grid, model = C.known_model_grid(gh, gw, step, perspective, seed=gh)
            mode = "perspective" if perspective else "similarity"
            ref, nv, _ = C.oracle_records_of(grid[0], step, mode)
            err = C.known_model_errors(ref[mode]["matrix"], model, gh, gw, step, perspective)
            assert ref[mode]["accepted"] and 0.6 < ref[mode]["confidence"] < 0.8
            assert all(e <= b for e, b in zip(err, C.KNOWN_BOUNDS[perspective])), (gh, gw, mode, err)
