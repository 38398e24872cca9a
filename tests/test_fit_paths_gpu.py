"""GPU parity of fit_kernel (csrc/vstab_fit.hip) and homography_kernel (csrc/vstab_homography.hip) on the cases of
tests/fit_cases.py: the sample counts and contents at which they change path (tests/test_fit_cases_cpu.py shows on the oracle
alone that every case is on the path it names).

Compared as tests/test_fit_gpu.py compares: the set of computed modes, valid and total points, acceptance and confidence equal;
translation bit-equal (and equal to numpy's float32 median where the shifts are hand-placed); similarity 1e-6 absolute;
homography 2e-5 relative + 1e-7 absolute on the entries; residual 1e-6 relative, for all three modes.  A record that is not
accepted carries the identity matrix and residual 0.

EXACT DATA (zero flow, an integer translation, constant rows): the oracle's own residual there is the rounding residue of
float64 sums of products of magnitude 1e3 (measured: oracle 0 .. 8e-13, GPU 4e-14 .. 7e-14), of which a relative bound says
nothing.  Where the oracle's residual is under 1e-9 -- the bound tests/test_fit_cases_cpu.py sets the oracle on those cases --
the GPU's must be too; everywhere else the relative bound applies unchanged.

DEGENERATE MINIMAL SAMPLE (line-and-one-sample): the only model its cut-short loop has comes from three collinear points and
one off their line.  The DLT matrix of such a sample has a TWO-dimensional null space; which vector of it the Jacobi solve
returns hangs on the last bit of its rotations, and the float32 inlier test of the wild matrix that results counts 6 inliers of
3001 in the oracle (glibc's hypot), 7 with OpenCV's own hypot formula in its place (a scratch build), 4 on the MI355X (the device
library's hypot).  Equality of that count is not a property of either side.  What the case is there for is the loop's END:
a loop that went on after getSubset's failure finds the camera model a quarter of the row follows and reports 597 of 3001 (0.2,
accepted).  So on this one pair the perspective confidence is held under 0.05 on both sides -- chance level is
3001 * pi * 2.5^2 / 80^2 = 9 samples, 0.003 -- and everything else is compared as everywhere.

ILL-CONDITIONED HOMOGRAPHIES: no case needed another comparison than the entry tolerance.  Measured on the MI355X, the largest
entry difference over all cases, the 12-sample ones (2x6, sparse-12, sparse-13, count-12 point pairs) included, is 0.004 of the
tolerance (|g - r| / (1e-7 + 2e-5 |r|), printed per case as "entry-diff/tolerance").
"""

import numpy as np
import pytest

from tests import fit_cases as C

pytestmark = pytest.mark.gpu

RESIDUAL_FLOOR = 1e-9
CUT_SHORT_BOUND = 0.05

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()      # a copy: the cases are read-only arrays


def _pair_points(grid, step):
    """(prev [nv,2], curr [nv,2]) float32 of one pair's valid samples, in the kernels' order."""
    gh, gw, _ = grid.shape
    ys, xs = np.mgrid[0:gh, 0:gw]
    prev = (np.stack([xs, ys], -1) * step).astype(np.float32)
    curr = prev + grid
    ok = np.isfinite(curr).all(-1)
    return prev[ok], curr[ok]


def _entry_excess(g, r):
    """Largest homography entry difference in units of the tolerance rtol 2e-5 + atol 1e-7 (<= 1 passes)."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    return float((np.abs(g - r) / (1e-7 + 2e-5 * np.abs(r))).max())


def check_pair(got, ref, nv, total, label, conf_total=None, cut_short=False):
    """One pair's GPU records {mode: dict} against the oracle's.  total: the GPU's total_points (admitted samples under a block
    grid); conf_total: the denominator of the translation confidence where it differs from the oracle's.  Every figure is
    printed, every deviation collected; one assertion at the end."""
    assert set(got) == set(ref), (label, set(got), set(ref))
    wrong = []

    def expect(ok, *what):
        if not ok:
            wrong.append((label,) + what)

    for name, r in ref.items():
        g = got[name]
        expect(g["valid_points"] == nv and g["total_points"] == total, name, "points", g["valid_points"], g["total_points"])
        expect(g["accepted"] == r["accepted"], name, "accepted", g["confidence"], r["confidence"])
        if name == "translation" and conf_total is not None:
            expect(g["confidence"] == float(nv) / float(conf_total), name, "confidence", g["confidence"])
        elif name == "perspective" and cut_short:
            print(f"FIT {label} perspective cut short: inliers gpu {g['confidence'] * nv:.0f} oracle {r['confidence'] * nv:.0f}")
            expect(g["confidence"] <= CUT_SHORT_BOUND and r["confidence"] <= CUT_SHORT_BOUND, name, "confidence", g["confidence"])
        else:
            expect(g["confidence"] == r["confidence"], name, "confidence", g["confidence"], r["confidence"])
        if not r["accepted"]:
            expect(np.array_equal(g["matrix"], np.eye(3, dtype=np.float32)) and g["residual"] == 0.0, name, "refused record", g)
            continue
        if name == "translation":
            expect(np.array_equal(g["matrix"], r["matrix"]), name, "matrix", g["matrix"][:2, 2].tolist(), r["matrix"][:2, 2].tolist())
        elif name == "similarity":
            diff = float(np.abs(g["matrix"].astype(np.float64) - r["matrix"].astype(np.float64)).max())
            print(f"FIT {label} similarity max-entry-diff {diff:.3e}")
            expect(np.allclose(g["matrix"], r["matrix"], rtol=0, atol=1e-6), name, "matrix", diff)
        else:
            excess = _entry_excess(g["matrix"], r["matrix"])
            print(f"FIT {label} perspective entry-diff/tolerance {excess:.3f}")
            expect(np.allclose(g["matrix"], r["matrix"], rtol=2e-5, atol=1e-7), name, "matrix", excess)
        print(f"FIT {label} {name} residual gpu {g['residual']:.12e} oracle {r['residual']:.12e}")
        if r["residual"] < RESIDUAL_FLOOR:
            expect(0.0 <= g["residual"] < RESIDUAL_FLOOR, name, "residual", g["residual"], r["residual"])
        else:
            expect(g["residual"] == pytest.approx(r["residual"], rel=1e-6), name, "residual", g["residual"], r["residual"])
    assert not wrong, wrong


def _same_table(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)


def _run_case(ctx, case_id, mode, form="blocking"):
    grid, blocked = C.inputs(case_id)
    g = _cuda(grid)
    b = None if blocked is None else _cuda(blocked)
    step = C.CASES[case_id].step
    if form == "blocking":
        return ctx.sample_fit_batch(g, step, mode, blocked=b)
    return ctx.sample_fit_batch_end(ctx.sample_fit_batch_begin(g, step, mode, blocked=b))


@pytest.mark.parametrize("case_id", C.CASE_IDS)
def test_fit_paths_match_oracle(ctx, oracle, case_id):
    from vstab_amd import native

    grid, blocked = C.inputs(case_id)
    step = C.CASES[case_id].step
    totals = C.admitted_counts(case_id)
    for mode in C.CASE_MODES[case_id]:
        table = _run_case(ctx, case_id, mode)
        got = native.fit_table_to_dicts(table)
        refs = C.oracle_records(case_id, mode)
        assert len(got) == len(refs) == grid.shape[0]
        for p, (ref, nv, _) in enumerate(refs):
            assert int(table["valid_points"][p, 0]) == nv and int(table["total_points"][p, 0]) == totals[p], (case_id, mode, p)
            check_pair(got[p], ref, nv, totals[p], (case_id, p), conf_total=totals[p] if blocked is not None else None,
                       cut_short=p in C.CASES[case_id].expect.get("cut_short", ()))
        if case_id in C.BOTH_FORMS_IDS:
            assert _same_table(table, _run_case(ctx, case_id, mode, "begin_end")), (case_id, mode)
        if blocked is not None:      # the masked fit is the plain fit on the grid without the blocked samples
            plain = ctx.sample_fit_batch(_cuda(C.effective_grid(case_id)), step, mode)
            for f in ("matrix", "accepted", "computed", "residual", "valid_points"):
                assert table[f].tobytes() == plain[f].tobytes(), (case_id, mode, f)


@pytest.mark.parametrize("case_id", C.MEDIAN_IDS)
def test_medians_of_placed_shifts_equal_numpy(ctx, case_id):
    """The translation record against numpy directly: np.median of the float32 shifts per axis, rounded to float32 as
    flow.py:191-208 does; residual = mean |(prev + t) - curr| with float32 terms summed in float64."""
    table = _run_case(ctx, case_id, "translation")
    grid = C.inputs(case_id)[0][0]
    step = C.CASES[case_id].step
    s = C.shifts_of(grid, step)
    want = np.array([np.float32(np.median(s[:, 0])), np.float32(np.median(s[:, 1]))], np.float32)
    rec = table[0, 0]
    assert rec["computed"] == 1 and rec["accepted"] == 1 and rec["valid_points"] == len(s)
    got = rec["matrix"].reshape(3, 3)
    assert np.array_equal(_bits(got[:2, 2]), _bits(want)), (case_id, got[:2, 2], want)
    assert np.array_equal(_bits(got[:2, :2]), _bits(np.eye(2))) and np.array_equal(_bits(got[2]), _bits([0, 0, 1]))
    prev, curr = _pair_points(grid, step)
    res = np.abs((prev + want) - curr).astype(np.float64).sum() / (2.0 * len(s))
    assert rec["residual"] == pytest.approx(res, rel=1e-12, abs=0.0) and rec["confidence"] == len(s) / float(grid.shape[0] * grid.shape[1])
    assert (table["computed"][0, 1:] == 0).all()


def test_small_call_after_a_large_one_reports_unrequested_modes_as_not_computed(ctx, oracle):
    """The record buffer is reused between calls: six production-size pairs in perspective mode, then one 2 x 6 pair in
    translation mode on the same context."""
    import torch

    from vstab_amd import native

    gh, gw = C.PROD_SHAPE
    six = np.stack([C.inputs("count-68x120")[0][0]] + [C.camera_flow(gh, gw, 8, 900 + i) for i in range(5)])
    first = ctx.sample_fit_batch(_cuda(six), 8, "perspective")
    assert (first["computed"] == 1).all()
    for p, entry in enumerate(native.fit_table_to_dicts(first)):
        ref, nv, nt = oracle.fit_all_modes(C.field_of(six[p], 8), 8, "perspective")
        check_pair(entry, ref, nv, nt, ("six-production-pairs", p))
    small = _run_case(ctx, "count-2x6", "translation")
    assert small["computed"][0].tolist() == [1, 0, 0] and small["accepted"][0].tolist() == [1, 0, 0]
    for mi in (1, 2):
        assert np.array_equal(_bits(small["matrix"][0, mi]), _bits(np.eye(3).reshape(9)))
        assert small["confidence"][0, mi] == 0.0 and small["residual"][0, mi] == 0.0
        assert small["valid_points"][0, mi] == 12 and small["total_points"][0, mi] == 12
    (ref, nv, nt), = C.oracle_records("count-2x6", "translation")
    check_pair(native.fit_table_to_dicts(small)[0], ref, nv, nt, ("count-2x6-after-large", 0))


def test_sample_limit_is_computed_at_and_refused_above(ctx, oracle):
    """gh*gw == 16384 fills the median's LDS array and is computed (test_fit_paths_match_oracle[count-128x128] compares it);
    one more sample is refused with an error that names the limit, and the context goes on working."""
    import torch

    from vstab_amd import native

    assert C.inputs("count-128x128")[0].shape[1:3] == (128, 128) and 128 * 128 == C.MAX_SORT
    over = torch.zeros((1, 5, 3277, 2), dtype=torch.float32, device="cuda")
    blocked = torch.zeros((2, 5, 3277), dtype=torch.uint8, device="cuda")
    for kw in ({}, {"blocked": blocked}):
        with pytest.raises(native.VstabError, match=str(C.MAX_SORT)):
            ctx.sample_fit_batch(over, 8, "similarity", **kw)
        with pytest.raises(native.VstabError, match=str(C.MAX_SORT)):
            ctx.sample_fit_batch_begin(over, 8, "similarity", **kw)
        after = native.fit_table_to_dicts(_run_case(ctx, "count-16x16", "perspective"))[0]
        (ref, nv, nt), = C.oracle_records("count-16x16", "perspective")
        check_pair(after, ref, nv, nt, ("count-16x16-after-refusal", 0))


def test_point_limit_is_computed_at_and_refused_above(ctx, oracle):
    import torch

    from vstab_amd import native

    rng = np.random.default_rng(1200)
    cap = C.MAX_SORT
    prev = (rng.uniform(0, 1, (cap, 2)) * [854, 480]).astype(np.float32)
    nxt = C.similar_tracks(rng, prev.astype(np.float64)).astype(np.float32)
    bad = rng.random(cap) < 0.2
    nxt[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2)).astype(np.float32)
    status = (rng.random(cap) >= 0.05).astype(np.uint8)
    table = np.concatenate([prev, np.where(status[:, None] == 1, nxt, np.float32(np.nan))], 1)[None].astype(np.float32)
    counts = torch.tensor([cap], dtype=torch.int32, device="cuda")
    got = native.fit_table_to_dicts(ctx.points_fit_batch(_cuda(table), counts, "perspective"))[0]
    ref, nv = oracle.fit_all_modes_points(prev, nxt, status, "perspective")
    check_pair(got, ref, nv, cap, ("points-16384", 0))
    over = torch.zeros((1, cap + 1, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(native.VstabError, match=str(C.MAX_SORT)):
        ctx.points_fit_batch(over, torch.tensor([12], dtype=torch.int32, device="cuda"), "perspective")
    small, small_counts, _ = C.point_table(64)
    again = ctx.points_fit_batch(_cuda(small), _cuda(small_counts), "similarity")
    assert again["computed"][:, 0].tolist() == [int(bool(r)) for r, _ in C.oracle_point_records(64, "similarity")]


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("cap", C.POINT_CAPS)
def test_point_tables_match_oracle(ctx, oracle, cap, mode):
    """vstab_points_fit_batch on tables whose rows beyond counts[p] hold finite decoys (tests/test_fit_cases_cpu.py: the oracle
    answers otherwise when it is given them)."""
    import torch

    from vstab_amd import native

    table, counts, pairs = C.point_table(cap)
    raw = ctx.points_fit_batch(_cuda(table), _cuda(counts), mode)
    got = native.fit_table_to_dicts(raw)
    for i, (ref, nv) in enumerate(C.oracle_point_records(cap, mode)):
        prev, nxt, status = pairs[i]
        assert raw["valid_points"][i].tolist() == [nv] * 3 and raw["total_points"][i].tolist() == [len(prev)] * 3
        check_pair(got[i], ref, nv, len(prev), (f"points-{cap}-{C.POINT_KINDS[i]}", i))


@pytest.mark.parametrize("gh,gw,step", C.KNOWN_GRIDS)
@pytest.mark.parametrize("perspective", [False, True])
def test_known_model_is_recovered(ctx, gh, gw, step, perspective):
    """Independent of the oracle: noise-free correspondences of a known similarity / homography under 30 % gross outliers.
    The bounds are those tests/test_referee_cpu.py holds the oracle to for float32 inputs."""
    import torch

    from vstab_amd import native

    grid, model = C.known_model_grid(gh, gw, step, perspective, seed=gh)
    mode = "perspective" if perspective else "similarity"
    got = native.fit_table_to_dicts(ctx.sample_fit_batch(_cuda(grid), step, mode))[0][mode]
    assert got["accepted"] and 0.6 < got["confidence"] < 0.8
    err = C.known_model_errors(got["matrix"], model, gh, gw, step, perspective)
    print(f"FIT known-model {gh}x{gw} {mode} errors {err} bounds {C.KNOWN_BOUNDS[perspective]}")
    assert all(e <= b for e, b in zip(err, C.KNOWN_BOUNDS[perspective])), (gh, gw, mode, err)
