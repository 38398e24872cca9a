"""The crop coverage cases that tests/test_crop_restatement_cpu.py (restatement against oracle, no GPU) and
tests/test_crop_gpu.py (kernels against both) share, and one cached reference per case.

A case is (source h x w -> output h x w, float32 matrices [n,3,3]).  Each is the smallest shape that reaches one path of
csrc/vstab_crop.hip; the path is named beside it.  BAND = 8 rows and 256 threads per workgroup in the band kernels, 64-lane
wavefronts, bw0 = vstab_warp_block_width, grid cap = 8192 workgroups x 256 threads = 2,097,152 items.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import crop_restatement as R
from tests.util import similarity
from tests.util import test_matrices as make_matrices

Case = namedtuple("Case", "name src out mats")      # src, out: (h, w)
Reference = namedtuple("Reference", "cov bbox common restated_bbox restated_common")

GRID_CAP_ITEMS = 8192 * 256


def block_width(oh, ow):
    """vstab_warp_block_width (csrc/vstab_internal.h), to state beside a case which bw0 it has."""
    return min(32 * 32 // min(16, oh), ow)


def _fit(src, out):
    """The resize that maps the source rectangle onto the output rectangle (source -> output, like every matrix here)."""
    (sh, sw), (oh, ow) = src, out
    return np.diag([ow / sw, oh / sh, 1.0])


def _kind(n, src, out, kind, fitted=False, seed=1):
    """tests.util.test_matrices for the source frame; fitted: for the output frame, behind the resize source -> output, so that
    the coverage's boundary runs through the whole output and not only its top-left source-sized corner."""
    if fitted:
        return make_matrices(n, out[1], out[0], kind, seed) @ _fit(src, out)
    return make_matrices(n, src[1], src[0], kind, seed)


def _gentle(n, src, seed=5):
    """Hand-made for frames of a few pixels, which the +-9 px of the named kinds leave empty: +-1.5 px, +-0.05 rad, 0.9..1.1x
    about the centre."""
    h, w = src
    rng = np.random.default_rng(seed)
    return np.stack([similarity(rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-0.05, 0.05), rng.uniform(0.9, 1.1),
                                w / 2, h / 2) for _ in range(n)])


def shift(dx, dy):
    """Pure translation: output pixel (x, y) shows source pixel (x - dx, y - dy)."""
    return similarity(float(dx), float(dy), 0.0, 1.0)


def _island(out, src, scale, theta, cx, cy):
    """The source magnified `scale` times and turned by theta, its centre placed at output (cx, cy)."""
    sh, sw = src
    return similarity(cx - sw / 2, cy - sh / 2, theta, scale, sw / 2, sh / 2)


EDGE_SHIFTS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (2, 0), (-2, 0), (0, 2), (0, -2), (2, 2), (-1, -2)]
EDGE = (24, 32)


def _build():
    c = []

    def add(name, src, out, mats):
        mats = np.ascontiguousarray(np.asarray(mats, np.float64).reshape(-1, 3, 3).astype(np.float32))
        mats.setflags(write=False)
        c.append(Case(name, tuple(src), tuple(out), mats))

    # -- column-block origin: bw0 = 1024 / min(16, out_h) capped at out_w; coverage = block-origin term + in-block term
    for kind in ("perspective", "horizon"):
        add(f"bw0_102_two_blocks_{kind}", (45, 73), (10, 150), _kind(3, (45, 73), (10, 150), kind, fitted=True))
        add(f"bw0_85_three_blocks_{kind}", (45, 73), (12, 200), _kind(3, (45, 73), (12, 200), kind, fitted=True))
        add(f"bw0_single_block_{kind}", (24, 32), (9, 40), _kind(2, (24, 32), (9, 40), kind, fitted=True))
        add(f"bw0_64_three_blocks_{kind}", (45, 73), (51, 130), _kind(3, (45, 73), (51, 130), kind, fitted=True))
    # -- source and output sizes distinct (sh / sw bound the coverage test, dh / dw everything else)
    add("distinct_51x80_similarity", (45, 73), (51, 80), _kind(3, (45, 73), (51, 80), "similarity"))
    add("distinct_51x80_perspective_fitted", (45, 73), (51, 80), _kind(3, (45, 73), (51, 80), "perspective", fitted=True))
    add("distinct_64x96_perspective", (120, 212), (64, 96), _kind(2, (120, 212), (64, 96), "perspective"))
    add("distinct_64x96_flip_fitted", (120, 212), (64, 96), _kind(2, (120, 212), (64, 96), "flip", fitted=True))
    add("distinct_1x9_to_3x11", (1, 9), (3, 11), [shift(1, 1), shift(0.6, 0.4) @ np.diag([1.1, 1.0, 1.0])])
    add("distinct_7x1_to_9x5", (7, 1), (9, 5), [shift(2, 1), _kind(1, (7, 1), (9, 5), "quarter_turn")[0]])
    # -- bands: out_h < 8, == 8, % 8 == 1; 8 * dw < 256 (idle wavefronts before the shuffle reduction); dw % 32 != 0
    #    (a one-pixel-wide frame is empty after half a pixel across it: the hand-made motions run along the line)
    add("band_1x37", (1, 37), (1, 37), [shift(1, 0), shift(-2, 0), shift(0.4, 0.3) @ np.diag([0.9, 1.0, 1.0])])
    add("band_37x1", (37, 1), (37, 1), [shift(0, 1), shift(0, -2), shift(0.2, 3.0) @ np.diag([1.0, 0.9, 1.0])])
    add("band_1x1", (1, 1), (1, 1), [np.eye(3), shift(0.6, 0.0)])
    add("band_5x3", (5, 3), (5, 3), _gentle(3, (5, 3)))
    add("band_8x31", (8, 31), (8, 31), _gentle(3, (8, 31)))
    add("band_9x33_minify", (9, 33), (9, 33), _kind(3, (9, 33), (9, 33), "minify"))
    add("band_9x33", (9, 33), (9, 33), _gentle(3, (9, 33)))
    add("band_17x257_flip", (17, 257), (17, 257), _kind(3, (17, 257), (17, 257), "flip"))
    add("band_17x257_translation", (17, 257), (17, 257), _kind(3, (17, 257), (17, 257), "translation"))
    add("band_45x33_quarter_turn", (45, 33), (45, 33), _kind(2, (45, 33), (45, 33), "quarter_turn"))
    add("band_45x3_magnify", (45, 3), (45, 3), _kind(2, (45, 3), (45, 3), "magnify"))
    # -- morphology at the image edge: integer shifts, coverage known in closed form (tests/test_crop_gpu.py states it)
    for dx, dy in EDGE_SHIFTS:
        add(f"edge_shift_{dx}_{dy}", EDGE, EDGE, [shift(dx, dy)])
    add("edge_shift_batch", EDGE, EDGE, [shift(dx, dy) for dx, dy in EDGE_SHIFTS[:5]])
    # -- empty and full frames in one batch (per-frame atomics, the host's per-frame `empty` rewrite)
    sim5 = _kind(5, (45, 73), (45, 73), "similarity")
    far = _kind(1, (45, 73), (45, 73), "far")[0]
    add("mixed_empty_frames_1_and_3", (45, 73), (45, 73), [sim5[0], far, sim5[2], far, sim5[4]])
    add("full_identity_n3", (45, 73), (45, 73), _kind(3, (45, 73), (45, 73), "identity"))
    # -- frame count: blockIdx.y above 64, a long frame loop in common_kernel
    add("one_frame", (45, 73), (45, 73), _kind(1, (45, 73), (45, 73), "similarity"))
    add("frames_70", (24, 32), (24, 32), _kind(70, (24, 32), (24, 32), "similarity"))
    # -- grid stride: above 2,097,152 items a thread takes a second item.  n * npx above the cap: coverage_kernel (frames 38
    #    and 39 are written in the second round); npx above the cap: common_kernel, erode3_kernel, common_coverage_kernel
    #    (rows 1092.. are written in the second round, so the islands reach down to the last row)
    add("stride_frames_40x270x200", (135, 240), (270, 200), _kind(40, (135, 240), (270, 200), "perspective", fitted=True))
    add("stride_pixels_1100x1920", (24, 32), (1100, 1920),
        [_island((1100, 1920), (24, 32), 30.0, 0.1, 960.0, 900.0), _island((1100, 1920), (24, 32), 41.0, -0.07, 1000.0, 860.0)])
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert CASES[-2].mats.shape[0] * 270 * 200 > GRID_CAP_ITEMS and 1100 * 1920 > GRID_CAP_ITEMS

_references = {}


def reference(oracle, case):
    """The oracle's coverage planes and crop analysis of a case and the restatement of the latter, computed once per session
    and read-only."""
    ref = _references.get(case.name)
    if ref is None:
        size_src, size_out = (case.src[1], case.src[0]), (case.out[1], case.out[0])
        cov = oracle.coverage_planes(case.mats, size_src, size_out)
        bbox, common = oracle.crop_analysis(case.mats, size_src, size_out)
        rb, rc = R.crop_analysis(cov)
        for a in (cov, bbox, common, rb, rc):
            a.setflags(write=False)
        ref = _references[case.name] = Reference(cov, bbox, common, rb, rc)
    return ref
