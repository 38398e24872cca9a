"""TV-L1 cases shared by tests/test_tvl1_cases_cpu.py (the cases are what they claim, on the restatement alone) and
tests/test_tvl1_gpu.py (csrc/vstab_tvl1.hip equals the restatement bit for bit on every one of them), and the restated
flow of each, computed once per session.

A case is (name, gray u8 [n,h,w], params dict or None, expectations).  Every clip is deterministic from a seed and comes
from the generators the suite already has: textured_clip of tests/test_tvl1_gpu.py, _content_clips of tests/test_dis_gpu.py.

(a) shapes: the inner kernel takes R rows per workgroup, R in {8, 4, 2, 1} per pyramid level, the most whose dynamic LDS
    8*(R*L + HL) + 8*(R+1)*w stays within 64 KB, with L = pow2_at_least(w) the width of the row tree and
    HL = pow2_at_least(h) the width of the row-sum tree (rows_per_workgroup below restates the rule; it is used to SHOW
    which R, L, HL a case reaches, never to compute a flow).
      24x1400    finest level R = 1 (L = 2048), second level 19x1120 R = 2, then the pyramid stops (15 rows)
      1400x24    HL = 2048 against L = 32, 175 workgroups per pair (1400 = 175 * 8: the last one is full)
      1401x24    the same with a 176th workgroup that owns one row and has no halo row below it
      20x512 / 20x513   L 512 -> 1024 (R = 4 at the finest level of both: 8 rows of L = 512 already pass 64 KB at
                 w = 512; the second level, 16x410, has R = 8)
      30x810     every level R = 4.  Found from the rule: with HL = 32, R = 4 holds for exactly 452 <= w <= 812 (8 rows
                 pass 64 KB once 72 w > 32512 under L = 512 and always under L = 1024; 4 rows fit while 40 w <= 32512),
                 so 810 -> 648 -> 518 stays inside, and h = 30 -> 24 -> 19 ends the pyramid before the 414-wide level.
                 30 and 19 are no multiples of 4 (last workgroups of 2 and 3 rows).
      64x47 / 65x47     HL 64 -> 128; 65 rows leave a ninth workgroup of one row
      1025x2048  the widest level with HL = 2048: R = 1 and exactly 65 536 B of dynamic LDS, the most the size guard
                 admits; the iteration caps are cut to 1 warp x 1 outer x 2 inner (one scale)
(b) parameters, all on the 3x37x53 textured clip: every parameter other than the iteration caps off its default, and the
    host's polling interval at 1 and beyond inner x outer (the host then never polls inside a warp).
(c) content, all at 3x45x61, the clips of test_dis_gpu._content_clips: the data-dependent branches.
"""

import functools
from collections import namedtuple

import numpy as np

from tests import tvl1_restatement as R

Case = namedtuple("Case", "name build params expect")

LDS_LIMIT = 64 * 1024


def pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


def lds_bytes(rows, h, w):
    """Dynamic LDS of one inner workgroup of `rows` rows: the row-tree terms [rows][L] and the row sums [HL] in double,
    the new u1 and u2 of rows + 1 rows in float."""
    return 8 * (rows * pow2_at_least(w) + pow2_at_least(h)) + 8 * (rows + 1) * w


def rows_per_workgroup(h, w):
    """(R, L, HL) of an h x w level: R = the largest of 8, 4, 2, 1 whose dynamic LDS is within 64 KB."""
    rows = 8
    while rows > 1 and lds_bytes(rows, h, w) > LDS_LIMIT:
        rows //= 2
    return rows, pow2_at_least(w), pow2_at_least(h)


def levels(h, w, nscales, scale_step):
    """The (h, w) of every pyramid level: each side times scale_step, rounded half to even; a level with a side under 16
    ends the pyramid before it."""
    out = [(h, w)]
    while len(out) < nscales:
        nh, nw = round(out[-1][0] * scale_step), round(out[-1][1] * scale_step)
        if nh < 16 or nw < 16:
            break
        out.append((nh, nw))
    return out


def _textured(n, h, w, seed):
    from tests.test_tvl1_gpu import textured_clip

    return textured_clip(n, h, w, seed)


def _content(name):
    from tests.test_dis_gpu import _content_clips

    return _content_clips(*CONTENT_SIZE)[name]


CONTENT_SIZE = (45, 61)
PARAM_CLIP = (3, 37, 53)
BIG_PARAMS = dict(nscales=1, warps=1, outer_iterations=1, inner_iterations=2)

# (name, (n, h, w), params, what every level must reach: a list of (R, L, HL), finest first)
_SHAPES = [
    ("wide-24x1400", (2, 24, 1400), None, [(1, 2048, 32), (2, 2048, 32)]),
    ("tall-1400x24", (2, 1400, 24), None, [(8, 32, 2048), (8, 32, 2048)]),
    ("tall-1401x24", (2, 1401, 24), None, [(8, 32, 2048), (8, 32, 2048)]),
    ("row-tree-20x512", (2, 20, 512), None, [(4, 512, 32), (8, 512, 16)]),
    ("row-tree-20x513", (2, 20, 513), None, [(4, 1024, 32), (8, 512, 16)]),
    ("all-R4-30x810", (2, 30, 810), None, [(4, 1024, 32), (4, 1024, 32), (4, 1024, 32)]),
    ("sum-tree-64x47", (2, 64, 47), None, [(8, 64, 64), (8, 64, 64), (8, 32, 64), (8, 32, 64), (8, 32, 32)]),
    ("sum-tree-65x47", (2, 65, 47), None, [(8, 64, 128), (8, 64, 64), (8, 32, 64), (8, 32, 64), (8, 32, 32)]),
    ("largest-1025x2048", (2, 1025, 2048), BIG_PARAMS, [(1, 2048, 2048)]),
]
# pairs of shape cases between which a tree width crosses a power of two at the finest level: (a, b, "L" or "HL")
PAIRED = [("row-tree-20x512", "row-tree-20x513", "L"), ("sum-tree-64x47", "sum-tree-65x47", "HL")]

_PARAMS = [
    ("median-off", dict(median_filtering=1), None),
    ("scale-step-0.5", dict(scale_step=0.5), None),
    ("one-scale-two-warps", dict(nscales=1, warps=2), None),
    ("lambda-0", dict(lambda_=0.0, outer_iterations=2), "zero_one_iteration"),
    ("epsilon-0", dict(epsilon=0.0, warps=1, outer_iterations=2, inner_iterations=7), "all_caps"),
    ("theta-tau-lambda", dict(theta=0.5, tau=0.1, lambda_=0.3), None),
    ("poll-every-launch", dict(poll_interval=1), None),
    ("poll-never", dict(poll_interval=10 * 30 + 1), None),   # beyond outer_iterations x inner_iterations
]

_CONTENT = [("flat", "zero_one_iteration"), ("still", "zero_one_iteration"), ("noise", None), ("bars", "all_caps"),
            ("jump", "leaves_frame"), ("saturated", None), ("half_noise", None)]


def _build_cases():
    cases = {}
    for name, (n, h, w), prm, reach in _SHAPES:
        cases[name] = Case(name, functools.partial(_textured, n, h, w, 31 * h + w), prm, {"reach": reach})
    n, h, w = PARAM_CLIP
    for name, prm, expect in _PARAMS:
        cases["param-" + name] = Case("param-" + name, functools.partial(_textured, n, h, w, 31 * h + w), prm, {"is": expect})
    for name, expect in _CONTENT:
        cases["content-" + name] = Case("content-" + name, functools.partial(_content, name), None, {"is": expect})
    return cases


CASES = _build_cases()
CASE_IDS = tuple(CASES)
SHAPE_IDS = tuple(name for name, *_ in _SHAPES)
# the grid-sampling and batch-invariance clip of the GPU tests: three pairs on the R = 1 / R = 2 path
WIDE_CLIP = (4, 24, 1400)


def library_params(case_id):
    """The case's parameters as the library takes them (poll_interval is the host loop's, the restatement has none)."""
    return dict(CASES[case_id].params or {})


def restatement_params(case_id):
    prm = dict(CASES[case_id].params or {})
    prm.pop("poll_interval", None)
    return R.params(**prm)


@functools.lru_cache(maxsize=None)
def clip(case_id):
    """u8 [n, h, w], read-only."""
    frames = np.ascontiguousarray(CASES[case_id].build(), dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def restated(case_id):
    """(flow f32 [n-1,h,w,2], counts i32 [n-1,nscales,warps]) of the restatement, read-only."""
    flow, counts = R.tvl1_clip(clip(case_id), restatement_params(case_id))
    flow.setflags(write=False)
    counts.setflags(write=False)
    return flow, counts


@functools.lru_cache(maxsize=None)
def wide_clip():
    frames = np.ascontiguousarray(_textured(*WIDE_CLIP, seed=2414), dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def wide_restated():
    flow, counts = R.tvl1_clip(wide_clip())
    flow.setflags(write=False)
    counts.setflags(write=False)
    return flow, counts


def case_levels(case_id):
    prm = restatement_params(case_id)
    _, h, w = clip(case_id).shape
    return levels(h, w, prm["nscales"], prm["scale_step"])
