"""GPU parity of the range sniff's wave-level tail: every wavefront of the gray pass (and of the stand-alone range pass)
leaves its own partial maximum -- a DPP maximum and a ballot of the NaN flag, no LDS and no barrier -- and one kernel
reduces a frame's partials.  The reference is numpy's max on the host, compared exactly (NaN as numpy propagates it,
+0 == -0 as numpy compares), at the smallest shapes where the tail can go wrong: wavefronts without a pixel, ragged loop
trips, every fused box size, the two-pass path, a single output row, and a second workgroup size."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.util import synth_frames

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

SHAPES = [
    # (n, h, w, work (w, h) or None)
    (2, 5, 64, None),            # K = 1: one wavefront has pixels, the other three have none
    (2, 7, 73, None),            # K = 1: odd width, scalar gray tail, the range pass takes its 4-byte loads
    (3, 14, 192, (96, 7)),       # K = 2: the last wavefront of the workgroup has no pixel
    (2, 20, 384, (96, 5)),       # K = 4: six wavefronts, all with pixels
    (1, 67, 121, (60, 33)),      # two passes: the range comes from the K = 1 launch over the 67 source rows
    (1, 6, 1920, (960, 3)),      # K = 2, 640 threads: two loop trips, the second one ragged
    (1, 8, 1000, (500, 4)),      # K = 2, 512 threads: the second half of the one trip is ragged
    (1, 2, 128, (64, 1)),        # K = 2: a single output row
    (1, 1, 64, None),            # K = 1: a single row, a single wavefront with pixels
]


def launch_threads(cols):
    """The gray launch's workgroup size for a row of `cols` source columns (csrc/vstab_gray.hip, threads_for): the
    multiple of 64 that covers the row in whole passes with the fewest idle lanes, ties to the size nearest 640."""
    best, best_cost = 256, None
    for t in range(256, 1025, 64):
        cost = -(-cols // t) * t
        if best_cost is None or cost < best_cost or (cost == best_cost and abs(t - 640) < abs(best - 640)):
            best, best_cost = t, cost
    return best


def last_wave_column(w, threads=None):
    """A source column that only the highest-numbered wavefront with any pixel reads (lane 63 of it where the row is long
    enough): for the rows of 384, 1000 and 1920 columns that is the last wavefront of the workgroup."""
    t = threads or launch_threads(w)
    wave = (min(t, w) - 1) >> 6
    return min(wave * 64 + 63, w - 1)


NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]


def special_inputs(n, h, w):
    """(name, frames) pairs; every one is unambiguous for numpy (checked by `expected` below)."""
    base = synth_frames(n, h, w, seed=h * 3 + w)
    col = last_wave_column(w)
    out = []

    def variant(name, frames=None):
        f = base.copy() if frames is None else frames
        out.append((name, f))
        return f

    variant("nan in the first sample")[0, 0, 0, 0] = np.nan
    variant("nan in the last sample of the last row")[-1, h - 1, w - 1, 2] = np.nan
    variant("nan in a column of the last wavefront")[0, 0, col, 1] = np.nan
    variant("nan in the second row of a box")[0, min(1, h - 1), w // 2, 0] = np.nan
    variant("nan with the sign bit set")[n - 1, h // 2, w // 3, 2] = NEG_NAN
    three = np.concatenate([base[:1] * 0.5, base[:1], base[:1] * 0.75])
    three[1, h - 1, col, 0] = np.nan
    variant("nan in frame 1 of 3 only", three)
    variant("all negative", -(base + np.float32(0.125)))
    variant("all -inf", np.full_like(base, -np.inf))
    variant("+inf and -inf in one pixel")[0, h // 2, w // 2] = (np.inf, -np.inf, 0.25)
    zeros = variant("-0 with one +0", np.full_like(base, -0.0))
    zeros[0, h - 1, w - 1, 0] = 0.0
    variant("maximum in a lane of the last wavefront only")[0, h - 1, col, 1] = 7.5
    return out


def expected(name, frames):
    """numpy's per-frame max, and a check that the input says what its name says."""
    n = frames.shape[0]
    want = frames.reshape(n, -1).max(axis=1)
    assert want.dtype == np.float32
    if name.startswith("nan"):
        assert np.isnan(want).sum() == 1, name
        if "frame 1 of 3" in name:
            assert n == 3 and np.isnan(want[1]) and np.isfinite(want[0]) and np.isfinite(want[2]) and want[0] != want[2]
    elif name == "all negative":
        assert np.all(want < 0) and np.all(want == -np.abs(frames).reshape(n, -1).min(axis=1))
    elif name == "all -inf":
        assert np.all(np.isneginf(want))
    elif name.startswith("+inf"):
        assert np.isposinf(want[0]) and np.all(np.isfinite(want[1:]))
    elif name.startswith("-0"):
        assert np.all(want == 0.0)
    else:
        assert want[0] == np.float32(7.5) and np.all(want[1:] <= 1.0)
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_partials_of_every_wavefront_reach_the_frame_maximum(ctx, shape):
    n, h, w, work = shape
    for name, frames in special_inputs(n, h, w):
        want = expected(name, frames)
        gray, peaks = ctx.gray_downscale(frames, work, want_range=True)
        got = peaks.cpu().numpy()
        alone = ctx.frame_range(frames).cpu().numpy()
        plain = ctx.gray_downscale(frames, work).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), (name, got, want)
        assert alone.dtype == np.float32 and np.array_equal(alone, want, equal_nan=True), (name, alone, want)
        assert np.array_equal(gray.cpu().numpy(), plain), name


CHILD = """
import os, sys
sys.path.insert(0, {root!r})
import numpy as np
import __graft_entry__ as graft
graft.load_package()
from vstab_amd import native
ctx = native.default_context()
data = np.load({inputs!r})
out = {{}}
for key, threads, work in (("a", "256", (96, 7)), ("a", "128", (96, 7)), ("b", "256", (960, 3))):
    os.environ["VSTAB_GRAY_THREADS"] = threads       # read by every call
    gray, peaks = ctx.gray_downscale(data[key], work, want_range=True)
    out[key + threads + "_gray"] = gray.cpu().numpy()
    out[key + threads + "_peaks"] = peaks.cpu().numpy()
np.savez({outputs!r}, **out)
"""


def test_another_workgroup_size_gives_the_same_maxima(ctx, tmp_path):
    """VSTAB_GRAY_THREADS (the A/B switch of the gray launch) changes the number of partials per row: the K = 2 case at
    256 threads (its own choice) and at 128 (two wavefronts, the second half of the trip ragged), and the 1920-column
    row at 256 instead of 640 (four wavefronts, four trips, the last one ragged).  A child process: the variable is the
    launch's, the context is the process's."""
    a = synth_frames(3, 14, 192, seed=5)
    a[0, 13, 191, 2] = 3.25                      # highest wavefront with pixels, last row
    a[1, 6, 130, 1] = np.nan
    a[2] = -(a[2] + np.float32(0.125))
    b = synth_frames(1, 6, 1920, seed=6)
    b[0, 5, last_wave_column(1920, 256) + 1536, 0] = 2.5   # last wavefront, last trip
    np.savez(tmp_path / "in.npz", a=a, b=b)
    code = CHILD.format(root=str(ROOT), inputs=str(tmp_path / "in.npz"), outputs=str(tmp_path / "out.npz"))
    env = {k: v for k, v in os.environ.items() if k != "VSTAB_GRAY_THREADS"}
    proc = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert proc.returncode == 0, proc.stdout[-2000:] + "\n" + proc.stderr[-4000:]
    got = np.load(tmp_path / "out.npz")
    for key, frames, work, sizes in (("a", a, (96, 7), ("256", "128")), ("b", b, (960, 3), ("256",))):
        want = frames.reshape(frames.shape[0], -1).max(axis=1)
        plain = ctx.gray_downscale(frames, work).cpu().numpy()
        for threads in sizes:
            peaks = got[key + threads + "_peaks"]
            assert peaks.dtype == np.float32 and np.array_equal(peaks, want, equal_nan=True), (key, threads, peaks, want)
            assert np.array_equal(got[key + threads + "_gray"], plain), (key, threads)
    want = a.reshape(3, -1).max(axis=1)
    assert want[0] == np.float32(3.25) and np.isnan(want[1]) and want[2] < 0
    assert b.max() == np.float32(2.5)
