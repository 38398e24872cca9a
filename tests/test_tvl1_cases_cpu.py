"""The cases of tests/tvl1_cases.py are what they claim, shown on the restatement alone (no GPU): which rows per workgroup
and tree widths the inner kernel's launch rule gives every level, and which data-dependent paths the content and parameter
cases take.  These are conditions on the cases, not measurements: a case that fails one is replaced, not loosened."""

import numpy as np
import pytest

from tests import tvl1_cases as C
from tests import tvl1_restatement as R


def test_levels_restate_the_pyramid_rule():
    for h, w, ns, step in [(540, 960, 5, 0.8), (30, 40, 5, 0.8), (16, 100, 5, 0.8), (37, 53, 5, 0.5), (1025, 2048, 1, 0.8),
                           (65, 47, 10, 0.8), (24, 1400, 5, 0.8)]:
        assert C.levels(h, w, ns, step) == R.pyramid_sizes(h, w, ns, step)


def test_launch_rule_at_its_thresholds():
    """Rows per workgroup by hand: 8*(R*L + HL) + 8*(R+1)*w against 65 536."""
    assert C.lds_bytes(4, 540, 960) == 8 * (4 * 1024 + 1024) + 8 * 5 * 960 == 79360
    assert C.lds_bytes(2, 540, 960) == 8 * (2 * 1024 + 1024) + 8 * 3 * 960 == 47616
    assert C.rows_per_workgroup(540, 960) == (2, 1024, 1024)
    assert C.rows_per_workgroup(1025, 2048) == (1, 2048, 2048) and C.lds_bytes(1, 1025, 2048) == C.LDS_LIMIT
    assert C.rows_per_workgroup(1024, 2048) == (1, 2048, 1024) and C.lds_bytes(1, 1024, 2048) < C.LDS_LIMIT
    assert C.rows_per_workgroup(20, 451)[0] == 8 and C.rows_per_workgroup(20, 452)[0] == 4
    assert C.rows_per_workgroup(20, 812)[0] == 4 and C.rows_per_workgroup(20, 813)[0] == 2


@pytest.mark.parametrize("case_id", C.SHAPE_IDS)
def test_shape_case_reaches_its_stated_levels(case_id):
    reach = [C.rows_per_workgroup(h, w) for h, w in C.case_levels(case_id)]
    assert reach == C.CASES[case_id].expect["reach"], (case_id, C.case_levels(case_id), reach)
    # the restatement ran exactly these levels
    _, counts = C.restated(case_id)
    assert (counts[:, :len(reach)] > 0).all() and (counts[:, len(reach):] == 0).all()


def test_shape_cases_cover_the_launch_rule():
    seen, partial, tall = set(), [], []
    for case_id in C.SHAPE_IDS:
        for h, w in C.case_levels(case_id):
            rows, row_tree, sum_tree = C.rows_per_workgroup(h, w)
            seen.add(rows)
            if h % rows:
                partial.append((case_id, h, w, rows))
            if sum_tree >= 64 * row_tree:
                tall.append((case_id, (h + rows - 1) // rows))
    assert seen == {1, 2, 4, 8}
    assert {rows for *_, rows in partial} >= {2, 4, 8}, partial      # a last workgroup with fewer rows, per R > 1
    assert any(groups >= 175 for _, groups in tall), tall            # HL far above L, many workgroups per pair
    for a, b, which in C.PAIRED:
        (ha, wa), (hb, wb) = C.case_levels(a)[0], C.case_levels(b)[0]
        _, la, hla = C.rows_per_workgroup(ha, wa)
        _, lb, hlb = C.rows_per_workgroup(hb, wb)
        if which == "L":
            assert wa == la and lb == 2 * la and hla == hlb, (a, b)     # at the power of two, then just past it
        else:
            assert ha == hla and hlb == 2 * hla and la == lb, (a, b)
    assert C.lds_bytes(1, 1025, 2048) == 65536    # the most the guard admits: largest-1025x2048


@pytest.mark.parametrize("case_id", C.CASE_IDS)
def test_case_meets_its_stated_condition(case_id):
    flow, counts = C.restated(case_id)
    case = C.CASES[case_id]
    prm = C.restatement_params(case_id)
    n, h, w = C.clip(case_id).shape
    assert flow.shape == (n - 1, h, w, 2) and counts.shape == (n - 1, prm["nscales"], prm["warps"])
    assert np.isfinite(flow).all()
    ns = len(C.case_levels(case_id))
    assert (counts[:, ns:] == 0).all()
    what = case.expect.get("is")
    if what == "zero_one_iteration":
        assert not flow.any()
        assert (counts[:, :ns] == 1).all(), counts
    elif what == "all_caps":
        assert (counts[:, :ns] == prm["outer_iterations"] * prm["inner_iterations"]).all(), counts
    else:
        assert (counts[:, :ns] >= 1).all()


def test_parameter_cases_change_the_result():
    """Every parameter case that names a parameter of the scheme computes something else than the defaults do (a parameter
    the call dropped would go unnoticed otherwise); the polling interval changes nothing."""
    base_flow, base_counts = C.restated("param-poll-never")
    for case_id in C.CASE_IDS:
        if not case_id.startswith("param-") or case_id.startswith("param-poll"):
            continue
        flow, _ = C.restated(case_id)
        assert not np.array_equal(flow, base_flow), case_id
    flow, counts = C.restated("param-poll-every-launch")
    assert np.array_equal(flow, base_flow) and np.array_equal(counts, base_counts)


def test_early_exit_differs_between_the_pairs_of_a_default_case():
    differing = []
    for case_id in C.CASE_IDS:
        case = C.CASES[case_id]
        if set(case.params or {}) - {"poll_interval"}:
            continue
        _, counts = C.restated(case_id)
        cap = 10 * 30
        if len(counts) > 1 and not np.array_equal(counts[0], counts[1]) and (counts[counts > 0] < cap).any():
            differing.append(case_id)
    assert "param-poll-every-launch" in differing and "content-saturated" in differing, differing
    _, counts = C.wide_restated()
    assert len({tuple(c.ravel().tolist()) for c in counts}) == len(counts)


def test_jump_samples_fully_outside_the_frame(monkeypatch):
    """During the restated run of the `jump` clip some finest-level sample lies so far outside the frame that none of its
    4 x 4 taps is inside (remap's all-outside path), others have some taps inside (the partial-border path)."""
    gray = C.clip("content-jump")
    _, h, w = gray.shape
    seen = {"outside": 0, "partial": 0, "beyond": 0.0}
    remap = R.remap_cubic

    def watching(src, map_x, map_y):
        if src.shape == (h, w):
            sx = np.rint(np.asarray(map_x, np.float32) * np.float32(32)).astype(np.int64) >> 5
            sy = np.rint(np.asarray(map_y, np.float32) * np.float32(32)).astype(np.int64) >> 5
            x0, y0 = sx - 1, sy - 1
            outside = (x0 >= w) | (x0 + 4 <= 0) | (y0 >= h) | (y0 + 4 <= 0)
            interior = (x0 >= 0) & (x0 < w - 3) & (y0 >= 0) & (y0 < h - 3)
            seen["outside"] += int(outside.sum())
            seen["partial"] += int((~outside & ~interior).sum())
            beyond = np.maximum.reduce([-np.asarray(map_x), np.asarray(map_x) - (w - 1), -np.asarray(map_y), np.asarray(map_y) - (h - 1)])
            seen["beyond"] = max(seen["beyond"], float(beyond.max()))
        return remap(src, map_x, map_y)

    monkeypatch.setattr(R, "remap_cubic", watching)
    flow, _ = R.tvl1_clip(gray)
    monkeypatch.undo()
    assert np.array_equal(flow, C.restated("content-jump")[0])
    assert seen["outside"] > 0 and seen["partial"] > 0, seen
    assert seen["beyond"] > 4.0, seen
    assert np.abs(flow).max() > 10.0    # u grows to tens of pixels
