"""Referees for the primitives of the TV-L1 restatement (tests/tvl1_restatement.py), which the HIP kernels of
csrc/vstab_tvl1.hip follow bit for bit: each primitive against an independent implementation, and the whole
restatement against a known sub-pixel translation.  No GPU."""

import numpy as np
import pytest

from tests import tvl1_restatement as R


def _field(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-40, 300, (h, w)).astype(np.float32)


@pytest.mark.parametrize("h,w", [(540, 960), (37, 53), (16, 17), (432, 768)])
def test_linear_resize_matches_torch_interpolate_inside(h, w):
    """resize(Size(), 0.8, 0.8, INTER_LINEAR) = bilinear with align_corners=False at scale 1.25 away from the borders."""
    import torch

    src = _field(h, w, h * 3 + w)
    got = R.resize_scale(src, 0.8)
    dh, dw = int(np.rint(h * 0.8)), int(np.rint(w * 0.8))
    assert got.shape == (dh, dw)
    # recompute_scale_factor=False: source coordinate (d + 0.5) / 0.8 - 0.5 as resize's 1/inv_scale; torch floors the
    # output size where resize rounds it, so compare the rows and columns both have
    ref = torch.nn.functional.interpolate(torch.from_numpy(src)[None, None].double(), scale_factor=0.8,
                                          recompute_scale_factor=False, mode="bilinear", align_corners=False)[0, 0].numpy()
    ch, cw = min(dh, ref.shape[0]), min(dw, ref.shape[1])
    inner = (slice(2, ch - 2), slice(2, cw - 2))
    # float32 weights and products against a double evaluation: a few ulps of values up to ~300
    assert np.abs(got[inner] - ref[inner]).max() < 1e-3


def test_linear_resize_matches_the_oracle_bilinear(oracle):
    """The upsampling between scales (dsize given) against the oracle's cv::resize INTER_LINEAR f32 restatement."""
    for (h, w, dh, dw) in [(432, 768, 540, 960), (22, 29, 28, 36), (16, 16, 20, 20)]:
        src = _field(h, w, h + w)
        got = R.resize_to(src, dw, dh)
        ref = oracle.resize_linear_f32(src, (dw, dh))[..., 0]
        assert got.shape == ref.shape
        inner = (slice(2, dh - 2), slice(2, dw - 2))
        assert np.abs(got[inner] - ref[inner]).max() <= 1e-3


@pytest.mark.parametrize("h,w", [(20, 31), (5, 5), (64, 48)])
def test_median5_matches_scipy(h, w):
    from scipy.ndimage import median_filter

    rng = np.random.default_rng(h * w)
    u = rng.standard_normal((h, w)).astype(np.float32)
    u[rng.uniform(size=(h, w)) < 0.3] = 0.25   # ties
    assert np.array_equal(R.median5(u), median_filter(u, size=5, mode="nearest"))


def test_cubic_table_matches_the_oracle(oracle):
    _, cub = oracle.interp_tables()
    assert np.array_equal(R.cubic_table(), cub)


@pytest.mark.parametrize("k", [0, 1, 5, 16, 31])
def test_cubic_remap_matches_the_oracle_warp(oracle, k):
    """remap(INTER_CUBIC, BORDER_CONSTANT 0) at x + k/32, y + (31-k)/32 (and a few pixels further, so that the border
    taps are exercised) equals the oracle's bicubic warp by the inverse translation, bit for bit."""
    h, w = 29, 41
    src = _field(h, w, 7 + k)
    for ox, oy in [(k / 32.0, (31 - k) / 32.0), (3 + k / 32.0, -2 - k / 32.0)]:
        mx = (np.arange(w, dtype=np.float32)[None, :] + np.float32(ox)).repeat(h, 0).astype(np.float32)
        my = (np.arange(h, dtype=np.float32)[:, None] + np.float32(oy)).repeat(w, 1).astype(np.float32)
        got = R.remap_cubic(src, mx, my)
        # warpPerspective maps dst -> src through the inverse of M: M = translation by (-ox, -oy)
        m = np.array([[1, 0, -ox], [0, 1, -oy], [0, 0, 1]], np.float32)
        ref, _ = oracle.warp_frame(np.repeat(src[..., None], 3, axis=2), m, (w, h), interp="bicubic", want_coverage=False)
        assert np.array_equal(got, ref[..., 0]), np.abs(got - ref[..., 0]).max()


def test_gradients_and_divergence_are_adjoint():
    """forward_gradient and divergence are the discrete -adjoint pair of the primal-dual scheme: <grad u, p> = -<u, div p>
    for p with p1 = 0 on the last column and p2 = 0 on the last row (what the dual update keeps)."""
    rng = np.random.default_rng(3)
    u = rng.standard_normal((13, 17)).astype(np.float64)
    p1 = rng.standard_normal((13, 17))
    p2 = rng.standard_normal((13, 17))
    p1[:, -1] = 0
    p2[-1, :] = 0
    ux, uy = R.forward_gradient(u)
    lhs = (ux * p1 + uy * p2).sum()
    rhs = -(u * R.divergence(p1, p2)).sum()
    assert abs(lhs - rhs) < 1e-9


def test_error_sum_is_the_stated_tree():
    t = np.arange(1, 8 * 5 + 1, dtype=np.float32).reshape(5, 8) / 7
    d = t.astype(np.float64)
    row = ((d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3])) + ((d[:, 4] + d[:, 5]) + (d[:, 6] + d[:, 7]))
    total = (((row[0] + row[1]) + (row[2] + row[3])) + ((row[4] + 0.0) + (0.0 + 0.0)))
    assert R.row_tree_error(t) == np.float32(total)


def test_pyramid_stops_before_a_level_under_16():
    assert R.pyramid_sizes(540, 960, 5, 0.8) == [(540, 960), (432, 768), (346, 614), (277, 491), (222, 393)]
    assert R.pyramid_sizes(30, 40, 5, 0.8) == [(30, 40), (24, 32), (19, 26)]
    assert R.pyramid_sizes(16, 100, 5, 0.8) == [(16, 100)]


def _texture(h, w, dx, dy):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x = x - dx
    y = y - dy
    v = (np.sin(x * 0.31 + 0.4) * np.cos(y * 0.23 - 0.2) + 0.6 * np.sin(x * 0.11 + y * 0.17 + 1.0)
         + 0.4 * np.cos(x * 0.05 - y * 0.07))
    return np.clip(np.rint(128 + 55 * v), 0, 255).astype(np.uint8)


def test_restatement_recovers_a_subpixel_translation():
    """I1(x) = I0(x - d): the flow of I0 -> I1 is d everywhere; inside a 10 px margin the mean flow is within 0.05 px."""
    h, w, d = 72, 96, (0.4, -0.65)
    i0 = _texture(h, w, 0.0, 0.0)
    i1 = _texture(h, w, d[0], d[1])
    flow, counts = R.tvl1_pair(i0, i1)
    inner = flow[10:-10, 10:-10]
    assert abs(float(inner[..., 0].mean()) - d[0]) <= 0.05
    assert abs(float(inner[..., 1].mean()) - d[1]) <= 0.05
    assert counts.shape == (5, 5) and (counts[:4] > 0).all()
