"""CPU: the NumPy restatement of the crop coverage analysis (tests/crop_restatement.py) proves itself before it judges a kernel.

1. On every case that tests/test_crop_gpu.py runs (tests/crop_cases.py), the restatement applied to the oracle's coverage
   planes equals oracle.crop_analysis exactly.
2. The cases can tell the rule from its near misses: for each mutation below at least one case gives another answer.  The
   mutants live here only.
"""

import numpy as np
import pytest

from tests import crop_cases as K
from tests import crop_restatement as R


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_restatement_equals_oracle(oracle, case):
    ref = K.reference(oracle, case)
    n, (oh, ow) = case.mats.shape[0], case.out
    assert ref.cov.shape == (n, oh, ow) and ref.cov.dtype == bool
    assert ref.restated_bbox.shape == (n, 4) and ref.restated_bbox.dtype == np.int32
    assert np.array_equal(ref.restated_bbox, ref.bbox)
    assert ref.restated_common.dtype == np.uint8 and np.array_equal(ref.restated_common, ref.common)


def test_coverage_planes_are_the_nearest_rule_on_integer_shifts(oracle):
    """The wrapper that hands out the oracle's coverage hands out the right plane: for an integer shift it is the shifted
    rectangle."""
    h, w = K.EDGE
    yy, xx = np.mgrid[0:h, 0:w]
    for dx, dy in K.EDGE_SHIFTS:
        cov = K.reference(oracle, K.BY_NAME[f"edge_shift_{dx}_{dy}"]).cov
        assert np.array_equal(cov[0], (xx - dx >= 0) & (xx - dx < w) & (yy - dy >= 0) & (yy - dy < h))


def test_grid_stride_cases_reach_the_second_round(oracle):
    """What makes the two grid-stride cases tests of the stride: the items behind the first 2,097,152 are not all zero."""
    frames, pixels = K.BY_NAME["stride_frames_40x270x200"], K.BY_NAME["stride_pixels_1100x1920"]
    ref = K.reference(oracle, frames)
    assert ref.cov.reshape(-1)[K.GRID_CAP_ITEMS:].any() and (ref.bbox[-1] >= 0).all()
    ref = K.reference(oracle, pixels)
    assert R.common_of(ref.cov).reshape(-1)[K.GRID_CAP_ITEMS:].any() and ref.common.reshape(-1)[K.GRID_CAP_ITEMS:].any()
    assert ref.cov[0].reshape(-1)[K.GRID_CAP_ITEMS:].any() and not ref.cov[0].reshape(-1)[K.GRID_CAP_ITEMS:].all()


# ---- the mutants ------------------------------------------------------------------------------------------------------------
def _morph(plane, dilate, outside):
    out = np.zeros(plane.shape, bool) if dilate else np.ones(plane.shape, bool)
    for nb in R._neighbours(plane, outside):
        out = (out | nb) if dilate else (out & nb)
    return out


def _analysis(cov, erode_outside=True, dilate_outside=False, bbox_before_closing=False, and_after_closing=False):
    """R.crop_analysis with one rule bent; with the defaults it is R.crop_analysis."""
    def erode(p):
        return _morph(p, False, erode_outside)

    closed = [erode(_morph(p, True, dilate_outside)) for p in cov]
    bbox = np.array([R.bbox_of(p if bbox_before_closing else c) for p, c in zip(cov, closed)], np.int32).reshape(-1, 4)
    return bbox, erode(R.common_of(closed if and_after_closing else cov)).astype(np.uint8)


MUTATIONS = {
    "outside_counts_as_zero_in_erode": dict(erode_outside=False),
    "outside_counts_as_one_in_dilate": dict(dilate_outside=True),
    "bbox_taken_before_the_closing": dict(bbox_before_closing=True),
    "and_taken_after_the_per_frame_closing": dict(and_after_closing=True),
}


def test_unbent_mutant_is_the_restatement(oracle):
    for case in K.CASES:
        ref = K.reference(oracle, case)
        bbox, common = _analysis(ref.cov)
        assert np.array_equal(bbox, ref.restated_bbox) and np.array_equal(common, ref.restated_common)


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_cases_distinguish_mutation(oracle, mutation):
    caught = []
    for case in K.CASES:
        ref = K.reference(oracle, case)
        bbox, common = _analysis(ref.cov, **MUTATIONS[mutation])
        if not (np.array_equal(bbox, ref.restated_bbox) and np.array_equal(common, ref.restated_common)):
            caught.append(case.name)
    print(mutation, "caught by", len(caught), "of", len(K.CASES), "cases:", caught)
    assert caught, f"no case tells {mutation} from the rule"


def test_each_named_edge_shift_decides_the_edge_rule(oracle):
    """The cases meant to pin the edge rule do so one by one, not only as a set: a 1 px gap closes (so a bbox taken before the
    closing differs), a 2 px gap does not (so a dilate that reads the outside as one differs), and both bend the erode's."""
    for dx, dy in K.EDGE_SHIFTS:
        ref = K.reference(oracle, K.BY_NAME[f"edge_shift_{dx}_{dy}"])
        one_px = max(abs(dx), abs(dy)) == 1
        mutation = "bbox_taken_before_the_closing" if one_px else "outside_counts_as_one_in_dilate"
        assert not np.array_equal(_analysis(ref.cov, **MUTATIONS[mutation])[0], ref.restated_bbox), (dx, dy, mutation)
        assert not np.array_equal(_analysis(ref.cov, erode_outside=False)[1], ref.restated_common), (dx, dy)
