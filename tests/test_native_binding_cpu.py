"""CPU tests of the ctypes binding layer (native.Context) against a stub library: which exception and text every refusal
raises, and which entry point every public method calls with which arguments, in which order, with the stream set or not.

Context's checks need only `self.torch` and `self.device`, so a context made with object.__new__ and a recording `lib`
runs every method on the CPU.  The refusals' texts are literals; the call records are tests/golden/native_calls.json,
written once by `python tests/test_native_binding_cpu.py` (record() below) and replayed here."""

import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "native_calls.json"

N, H, W = 3, 8, 10          # frames of 8 x 10, n = 3
STEP, GH, GW = 4, 2, 3      # the sample grid of an 8 x 10 image at step 4
P = N - 1


# ---------------------------------------------------------------- the stub
class RaisingLib:
    """Every attribute raises: a refusal that passes with this lib came before any library call.  `allow`: entry points a
    method is known to call ahead of its checks (they return 0)."""

    def __init__(self, allow=()):
        self._allow = tuple(allow)

    def __getattr__(self, name):
        if name in self._allow:
            return lambda *args: 0
        raise AssertionError(f"the library was reached ({name}) before the refusal")


def _plain(v):
    """One argument as the record keeps it: None, "ptr" for an address (any int at or above 2^32: sizes here are far below
    that, addresses on this platform above), the value of any other int or float."""
    if v is None:
        return None
    if isinstance(v, bytes):
        return v.decode()
    if isinstance(v, (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int)):
        return _plain(v.value)
    if type(v).__name__ == "CArgObject":        # ctypes.byref(...)
        return "ref"
    if isinstance(v, (bool, np.bool_)):
        return int(v)
    if isinstance(v, (int, np.integer)):
        return "ptr" if int(v) >= 1 << 32 else int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    raise AssertionError(f"the library was handed a {type(v).__name__}: {v!r}")


class RecordingLib:
    """Every attribute is an entry point that returns 0 and records its call."""

    def __init__(self, events):
        self._events = events

    def __getattr__(self, name):
        if not name.startswith("vstab_"):
            raise AttributeError(name)

        def entry(*args):
            stream = bool(self._events) and self._events[-1] == "stream"
            self._events.append([name, stream, [_plain(a) for a in args]])
            return 0

        return entry


def make_context(native, lib, events=None):
    import torch

    ctx = object.__new__(native.Context)
    ctx.torch = torch
    ctx.device = torch.device("cpu")
    ctx.device_index = 0
    ctx.lib = lib
    ctx.handle = 7
    ctx.last_upload_coded = (0, 0)
    ctx.last_download_coded = False
    ctx.use_torch_stream = (lambda: events.append("stream")) if events is not None else (lambda: None)
    ctx.close = lambda: None        # (no vstab_destroy of the made-up handle when the object goes away)
    return ctx


# ---------------------------------------------------------------- small valid arguments
def _t():
    import torch

    return torch


def frames(n=N, ch=3, h=H, w=W):
    return _t().zeros((n, h, w, ch), dtype=_t().float32)


def gray(n=N, h=H, w=W):
    return _t().zeros((n, h, w), dtype=_t().uint8)


def mask(n=N, h=H, w=W):
    return _t().zeros((n, h, w), dtype=_t().float32)


def eye(n=N, dtype=np.float32):
    return np.tile(np.eye(3, dtype=dtype), (n, 1, 1))


def grid_flow(pairs=P):
    return _t().zeros((pairs, GH, GW, 2), dtype=_t().float32)


def blocked(n=N):
    return _t().zeros((n, GH, GW), dtype=_t().uint8)


def i32(*shape):
    return _t().zeros(shape, dtype=_t().int32)


def offsets(n=N, mh=2, mw=3):
    return np.zeros((n, mh, mw, 2), np.float32)


def strided():
    """A float32 tensor that is not contiguous."""
    return _t().zeros((N, H, W, 6), dtype=_t().float32)[..., ::2]


K = 2                                                   # candidates per frame of the neighbour passes
SIZE = (W, H)


def cand(n=N):
    return np.zeros((n, K), np.int32)


def nmats(n=N):
    return np.zeros((n, K, 3, 3), np.float32)


def plate(shots=1):
    return _t().zeros((shots, H, W, 3), dtype=_t().float32)


def pcount(shots=1):
    return i32(shots, H, W)


# ---------------------------------------------------------------- refusals
V, E = "VstabError", "ValueError"
DEV = "cpu"
TENSOR = "must be a contiguous float32 tensor on cpu"


def _three_channel_rows():
    f4 = lambda: frames(ch=4)   # noqa: E731
    rows = [
        ("warp_batch", lambda c: c.warp_batch(f4(), eye(), SIZE)),
        ("warp_blur_batch", lambda c: c.warp_blur_batch(f4(), eye(dtype=np.float64), SIZE, 0.5, 3)),
        ("gray_downscale", lambda c: c.gray_downscale(f4(), None)),
        ("warp_batch_planned", lambda c: c.warp_batch_planned(f4(), 0, SIZE)),
        ("mesh_warp_batch", lambda c: c.mesh_warp_batch(f4(), eye(), SIZE, offsets())),
        ("mesh_unwarp_batch", lambda c: c.mesh_unwarp_batch(f4(), eye(), SIZE, offsets())),
        ("rolling_warp_batch", lambda c: c.rolling_warp_batch(f4(), eye(), SIZE, np.zeros((N, 6)), 0.5)),
        ("rolling_unwarp_batch", lambda c: c.rolling_unwarp_batch(f4(), eye(), SIZE, np.zeros((N, 6)), 0.5)),
        ("temporal_fill_batch", lambda c: c.temporal_fill_batch(f4(), nmats(), cand(), frames(), mask())),
        ("fill_gain_sums", lambda c: c.fill_gain_sums(f4(), nmats(), cand(), eye(), frames())),
        ("temporal_fill_blend_batch",
         lambda c: c.temporal_fill_blend_batch(f4(), nmats(), cand(), eye(), np.ones((N, K, 3)), frames(), mask())),
        ("sharp_transfer_batch", lambda c: c.sharp_transfer_batch(f4(), nmats(), cand(), np.ones((N, K)), 0.5, frames())),
    ]
    return [(f"{who}-channels", call, V, f"{who} expects 3-channel frames, got 4") for who, call in rows]


def _neighbour_rows():
    """The checks of _neighbour_io through each of its four entries."""
    def entry(who, **over):
        a = dict(clip=frames(), m=nmats(), cf=cand(), own=eye(), dst=frames(), mask=mask(), subpix=None)
        a.update(over)
        if who == "temporal_fill_batch":
            return lambda c: c.temporal_fill_batch(a["clip"], a["m"], a["cf"], a["dst"], a["mask"], subpix=a["subpix"])
        if who == "fill_gain_sums":
            return lambda c: c.fill_gain_sums(a["clip"], a["m"], a["cf"], a["own"], a["dst"], subpix=a["subpix"])
        if who == "temporal_fill_blend_batch":
            return lambda c: c.temporal_fill_blend_batch(a["clip"], a["m"], a["cf"], a["own"], np.ones((N, K, 3)), a["dst"], a["mask"],
                                                         subpix=a["subpix"])
        return lambda c: c.sharp_transfer_batch(a["clip"], a["m"], a["cf"], np.ones((N, K)), 0.5, a["dst"], a["mask"], subpix=a["subpix"])

    rows = []
    for who in ("temporal_fill_batch", "fill_gain_sums", "temporal_fill_blend_batch", "sharp_transfer_batch"):
        if who != "temporal_fill_batch":
            rows.append((f"{who}-subpix", entry(who, subpix="exact"), V,
                         f"{who}: sub-pixel mode 'exact' is not supported; the entry is 'q5' only"))
        rows.append((f"{who}-dst-tensor", entry(who, dst=strided()), V, f"{who}: dst {TENSOR}"))
        rows.append((f"{who}-dst-shape", entry(who, dst=frames(ch=4)), V,
                     f"{who}: dst (3, 8, 10, 4) / mask {None if who == 'fill_gain_sums' else (3, 8, 10)} do not match"))
        if who != "fill_gain_sums":
            rows.append((f"{who}-mask-tensor", entry(who, mask=mask().double()), V, f"{who}: mask {TENSOR}"))
            rows.append((f"{who}-mask-shape", entry(who, mask=mask(n=2)), V, f"{who}: dst (3, 8, 10, 3) / mask (2, 8, 10) do not match"))
        rows.append((f"{who}-cand", entry(who, cf=cand(n=2)), V, f"{who}: cand_frame (2, 2) is not [n=3, K]"))
        rows.append((f"{who}-matrices", entry(who, m=nmats(n=2)), V, f"{who}: matrices (2, 2, 3, 3) are not [n=3, K=2, 3, 3]"))
        if who in ("fill_gain_sums", "temporal_fill_blend_batch"):
            rows.append((f"{who}-own", entry(who, own=eye(2)), V, f"{who}: own_matrices (2, 3, 3) are not [n=3, 3, 3]"))
    return rows


def _anchor_rows():
    rows = []
    for who in ("anchor_sums_batch", "anchor_sums_ex_batch"):
        def call(g=None, a=None, r=None, cap=32, _who=who, **kw):
            g = gray() if g is None else g
            n = g.shape[0]
            a = np.full(n, -1) if a is None else a
            r = np.zeros((n, 6)) if r is None else r
            return lambda c: getattr(c, _who)(g, a, r, cap, **kw)

        rows += [
            (f"{who}-dtype", call(g=mask()), E, f"{who} expects a uint8 [N,h,w] tensor"),
            (f"{who}-empty", call(g=gray(n=0)), E, f"{who} needs at least one frame"),
            (f"{who}-sizes", call(a=np.full(2, -1)), E, f"{who}: anchor (2,) / R (3, 6) are not [3] / [3,6] for 3 frames"),
            (f"{who}-anchor", call(a=np.array([0, 3, -1])), E, f"{who}: an anchor outside -1..2"),
            (f"{who}-large", call(g=gray(n=1, h=1, w=1025)), E, f"{who}: 1025x1 image larger than 1024 on a side"),
            (f"{who}-cap", call(cap=256), E, f"{who}: cap 256 is not an integer in 0..255"),
            (f"{who}-cap-fraction", call(cap=1.5), E, f"{who}: cap 1.5 is not an integer in 0..255"),
        ]
    who = "anchor_sums_ex_batch"
    rows += [
        (f"{who}-gain-size", call(gain=np.full(2, 1024)), E, f"{who}: gain (2,) / offset (3,) are not [3] for 3 frames"),
        (f"{who}-gain", call(gain=np.full(N, 255)), E, f"{who}: a gain outside 256..4096"),
        (f"{who}-offset", call(offset=np.full(N, (1 << 20) + 1)), E, f"{who}: an offset outside -2^20..2^20"),
        (f"{who}-step", call(step=0), E, f"{who}: step 0 is not a positive integer"),
        (f"{who}-step-fraction", call(step=2.5), E, f"{who}: step 2.5 is not a positive integer"),
        (f"{who}-blocked", call(blocked=blocked(n=2), step=STEP), E, f"{who}: blocked (2, 2, 3) torch.uint8 is not uint8 [3,2,3]"),
    ]
    return rows


def _residual_rows():
    rows = []
    fit_blocked = ("sample_fit_batch: blocked (2, 2, 3) torch.uint8 is not uint8 [3,2,3] (one row per frame of the 2 pairs)")
    calls = {
        "mesh_residual_batch": lambda gf=None, step=STEP, size=SIZE, tr=None, bl=None: (
            lambda c: c.mesh_residual_batch(grid_flow() if gf is None else gf, step, size, eye(P) if tr is None else tr, 3, 2, bl)),
        "row_residual_batch": lambda gf=None, step=STEP, size=SIZE, tr=None, bl=None: (
            lambda c: c.row_residual_batch(grid_flow() if gf is None else gf, step, size, eye(P) if tr is None else tr, bl)),
        "rectify_samples_batch": lambda gf=None, step=STEP, size=SIZE, tr=None, bl=None: (
            lambda c: c.rectify_samples_batch(grid_flow() if gf is None else gf, step, size, np.zeros((N, 6)), 0.5, bl)),
    }
    for who, call in calls.items():
        rows += [
            (f"{who}-grid-dtype", call(gf=grid_flow().double()), E, f"{who} expects a float32 [P,gh,gw,2] tensor"),
            (f"{who}-grid-last", call(gf=_t().zeros((P, GH, GW, 3))), E, f"{who} expects a float32 [P,gh,gw,2] tensor"),
            (f"{who}-blocked", call(bl=blocked(n=2)), E, fit_blocked),
            (f"{who}-grid-size", call(size=(W + 4, H)), E, f"{who}: a grid of 3x2 samples is not a 14x8 image at step 4"),
            (f"{who}-grid-step", call(step=0), E, f"{who}: a grid of 3x2 samples is not a 10x8 image at step 0"),
        ]
        if who != "rectify_samples_batch":
            rows.append((f"{who}-transitions", call(tr=eye(N)), E, f"{who}: transitions (3, 3, 3) are not [2,3,3]"))
    rows += [
        ("sample_fit_batch-blocked", lambda c: c.sample_fit_batch(grid_flow(), STEP, "similarity", blocked(n=2)), E, fit_blocked),
        ("sample_fit_batch_begin-blocked", lambda c: c.sample_fit_batch_begin(grid_flow(), STEP, "similarity", blocked(n=2)), E, fit_blocked),
        ("mesh_residual_batch-vertices", lambda c: c.mesh_residual_batch(grid_flow(), STEP, SIZE, eye(P), 1, 2), E,
         "mesh_residual_batch: 1x2 vertices outside 2..65 per axis"),
        ("mesh_residual_batch-vertices-many", lambda c: c.mesh_residual_batch(grid_flow(), STEP, SIZE, eye(P), 3, 66), E,
         "mesh_residual_batch: 3x66 vertices outside 2..65 per axis"),
    ]
    return rows


def _displaced_rows():
    rows = []
    mesh = {
        "mesh_warp_batch": lambda off: (lambda c: c.mesh_warp_batch(frames(), eye(), SIZE, off)),
        "mesh_unwarp_batch": lambda off: (lambda c: c.mesh_unwarp_batch(frames(), eye(), SIZE, off)),
        "cover_extent_batch": lambda off: (lambda c: c.cover_extent_batch(eye(), SIZE, SIZE, off)),
    }
    for who, call in mesh.items():
        rows += [
            (f"{who}-offsets-n", call(offsets(n=2)), E, f"{who}: offsets (2, 2, 3, 2) torch.float32 are not float32 [3,mh,mw,2]"),
            (f"{who}-offsets-dtype", call(_t().zeros((N, 2, 3, 2), dtype=_t().float64)), E,
             f"{who}: offsets (3, 2, 3, 2) torch.float64 are not float32 [3,mh,mw,2]"),
            (f"{who}-vertices", call(offsets(mh=2, mw=1)), E, f"{who}: 1x2 vertices outside 2..65 per axis"),
        ]
    rolling = {
        "rolling_warp_batch": lambda v, r: (lambda c: c.rolling_warp_batch(frames(), eye(), SIZE, v, r)),
        "rolling_unwarp_batch": lambda v, r: (lambda c: c.rolling_unwarp_batch(frames(), eye(), SIZE, v, r)),
        "rectify_samples_batch": lambda v, r: (lambda c: c.rectify_samples_batch(grid_flow(), STEP, SIZE, v, r)),
    }
    for who, call in rolling.items():
        rows += [
            (f"{who}-velocity", call(np.zeros((2, 6)), 0.5), E, f"{who}: velocity (2, 6) is not [3,6]"),
            (f"{who}-readout", call(np.zeros((N, 6)), 1.5), E, f"{who}: readout=1.5 outside [-1, 1]"),
            (f"{who}-readout-nan", call(np.zeros((N, 6)), float("nan")), E, f"{who}: readout=nan outside [-1, 1]"),
        ]
    return rows


def _plate_rows():
    rows = []
    calls = {
        "plate_median_batch": lambda f=None, m=None, **kw: (
            lambda c: c.plate_median_batch(frames() if f is None else f, m, kw.get("tab", np.zeros((1, 3), np.int32)))),
        "plate_fill_batch": lambda f=None, m=None, **kw: (
            lambda c: c.plate_fill_batch(frames() if f is None else f, mask() if m is None else m, kw.get("plate", plate()),
                                         kw.get("count", pcount()), kw.get("shot"), kw.get("min_count", 2))),
        "plate_matte_batch": lambda f=None, m=None, **kw: (
            lambda c: c.plate_matte_batch(frames() if f is None else f, m, kw.get("plate", plate()), kw.get("count", pcount()),
                                          kw.get("shot"), kw.get("threshold", 0.1), kw.get("min_count", 2))),
    }
    for who, call in calls.items():
        name = "dst" if who == "plate_fill_batch" else "frames"
        rows += [
            (f"{who}-frames-tensor", call(f=strided()), E, f"{who}: {name} {TENSOR}"),
            (f"{who}-frames-shape", call(f=frames(ch=4)), E, f"{who}: {name} of shape (3, 8, 10, 4) are not [n,h,w,3] with n, h, w >= 1"),
            (f"{who}-frames-empty", call(f=frames(n=0)), E, f"{who}: {name} of shape (0, 8, 10, 3) are not [n,h,w,3] with n, h, w >= 1"),
            (f"{who}-mask-tensor", call(m=mask().double()), E, f"{who}: mask {TENSOR}"),
            (f"{who}-mask-shape", call(m=mask(n=2)), E, f"{who}: mask of shape (2, 8, 10) is not (3, 8, 10)"),
        ]
        if who == "plate_median_batch":
            continue
        rows += [
            (f"{who}-plate-tensor", call(plate=plate().double()), E, f"{who}: plate {TENSOR}"),
            (f"{who}-plate-shape", call(plate=_t().zeros((1, H, W + 1, 3))), E, f"{who}: plate of shape (1, 8, 11, 3) is not [shots,8,10,3]"),
            (f"{who}-count-tensor", call(count=pcount().long()), E, f"{who}: count must be a contiguous int32 tensor on cpu"),
            (f"{who}-count-shape", call(count=i32(2, H, W)), E, f"{who}: count of shape (2, 8, 10) is not (1, 8, 10)"),
            (f"{who}-min-count", call(min_count=0), E, f"{who}: min_count=0 is not an integer in 1..256"),
            (f"{who}-min-count-bool", call(min_count=True), E, f"{who}: min_count=True is not an integer in 1..256"),
            (f"{who}-min-count-float", call(min_count=2.0), E, f"{who}: min_count=2.0 is not an integer in 1..256"),
            (f"{who}-shot-order", call(shot=[0, 1, 0], plate=plate(2), count=pcount(2)), E,
             f"{who}: shot of shape (3,) is not a non-decreasing sequence of n=3 shot numbers in 0..1"),
            (f"{who}-shot-range", call(shot=[0, 0, 1]), E,
             f"{who}: shot of shape (3,) is not a non-decreasing sequence of n=3 shot numbers in 0..0"),
            (f"{who}-shot-length", call(shot=[0, 0]), E,
             f"{who}: shot of shape (2,) is not a non-decreasing sequence of n=3 shot numbers in 0..0"),
            (f"{who}-shot-none", call(plate=plate(2), count=pcount(2)), E, f"{who}: shot=None means one shot, but plate holds 2"),
        ]
    rows += [
        ("plate_fill_batch-mask-none", lambda c: c.plate_fill_batch(frames(), None, plate(), pcount(), None, 2), E,
         f"plate_fill_batch: mask {TENSOR}"),
        ("plate_median_batch-table", calls["plate_median_batch"](tab=np.zeros(3, np.int32)), E,
         "plate_median_batch: sample_frame of shape (3,) is not [shots,S]"),
        ("plate_median_batch-table-empty", calls["plate_median_batch"](tab=np.zeros((0, 3), np.int32)), E,
         "plate_median_batch: sample_frame of shape (0, 3) is not [shots,S]"),
        ("plate_matte_batch-threshold", calls["plate_matte_batch"](threshold=-1.0), E,
         "plate_matte_batch: threshold=-1.0 is not a finite number >= 0"),
        ("plate_matte_batch-threshold-nan", calls["plate_matte_batch"](threshold=float("nan")), E,
         "plate_matte_batch: threshold=nan is not a finite number >= 0"),
        ("plate_matte_batch-threshold-bool", calls["plate_matte_batch"](threshold=True), E,
         "plate_matte_batch: threshold=True is not a finite number >= 0"),
        ("plate_matte_batch-threshold-text", calls["plate_matte_batch"](threshold="0.1"), E,
         "plate_matte_batch: threshold='0.1' is not a finite number >= 0"),
    ]
    return rows


def _other_rows():
    who = "frame_sse_batch"
    sse = lambda a=None, b=None, ma=None, mb=None: (   # noqa: E731
        lambda c: c.frame_sse_batch(frames() if a is None else a, frames() if b is None else b, ma, mb))
    rows = [
        ("upload_u8_as_f32-dtype", lambda c: c.upload_u8_as_f32(mask()), V, "upload_u8_as_f32: a uint8 CPU tensor is required"),
        ("warp_blur_batch-clip", lambda c: c.warp_blur_batch(frames(), eye(dtype=np.float64), SIZE, 0.5, 3, clip_first=1), V,
         "warp_blur_batch: frames [1, 4) outside a clip of 3 matrices"),
        ("warp_blur_batch-clip-negative", lambda c: c.warp_blur_batch(frames(), eye(dtype=np.float64), SIZE, 0.5, 3, clip_first=-1), V,
         "warp_blur_batch: frames [-1, 2) outside a clip of 3 matrices"),
        ("dis_flow_batch-pairs", lambda c: c.dis_flow_batch(gray(n=1)), V, "dis_flow_batch needs at least two frames"),
        ("tvl1_flow_batch-dtype", lambda c: c.tvl1_flow_batch(mask()), E, "tvl1_flow_batch expects a uint8 [N,h,w] tensor"),
        ("tvl1_flow_batch-dim", lambda c: c.tvl1_flow_batch(gray()[0]), E, "tvl1_flow_batch expects a uint8 [N,h,w] tensor"),
        ("tvl1_flow_batch-pairs", lambda c: c.tvl1_flow_batch(gray(n=1)), E, "tvl1_flow_batch needs at least two frames"),
        ("tvl1_flow_batch-parameter", lambda c: c.tvl1_flow_batch(gray(), {"bogus": 1}), E, "unknown TV-L1 parameter 'bogus'"),
        ("mask_block_grid-shape", lambda c: c.mask_block_grid(mask(n=2), N, None, STEP, 0), E,
         "mask_block_grid: mask (2, 8, 10) is not [3,H,W], [1,H,W] or [H,W]"),
        ("mask_block_grid-dim", lambda c: c.mask_block_grid(frames(), N, None, STEP, 0), E,
         "mask_block_grid: mask (3, 8, 10, 3) is not [3,H,W], [1,H,W] or [H,W]"),
        ("mask_block_grid-margin", lambda c: c.mask_block_grid(mask(), N, None, STEP, 65), E, "mask_block_grid: margin 65 outside [0, 64]"),
        ("pair_residual_batch-dtype", lambda c: c.pair_residual_batch(mask(), eye(P)), E, "pair_residual_batch expects a uint8 [N,h,w] tensor"),
        ("pair_residual_batch-pairs", lambda c: c.pair_residual_batch(gray(n=1), eye(0)), E, "pair_residual_batch needs at least two frames"),
        ("pair_residual_batch-transitions", lambda c: c.pair_residual_batch(gray(), eye(N)), E,
         "pair_residual_batch: transitions (3, 3, 3) are not [2,3,3] for 3 frames"),
        ("fit_records_device-none", lambda c: c.fit_records_device(), V, "fit_records_device: no fit is pending"),
        ("flow_plan_device-framing", lambda c: c.flow_plan_device(1 << 40, P, "similarity", SIZE, None, 1.0, 30.0, 1.0, False, framing="crop"),
         V, "flow_plan_device: framing 'crop' is not formed on the device"),
        ("temporal_fill_batch-mask-none", lambda c: c.temporal_fill_batch(frames(), nmats(), cand(), frames(), None), V,
         f"temporal_fill_batch: mask {TENSOR}"),
        ("temporal_fill_blend_batch-mask-none",
         lambda c: c.temporal_fill_blend_batch(frames(), nmats(), cand(), eye(), np.ones((N, K, 3)), frames(), None), V,
         "temporal_fill_blend_batch: mask must be a contiguous float32 tensor"),
        ("temporal_fill_blend_batch-gains",
         lambda c: c.temporal_fill_blend_batch(frames(), nmats(), cand(), eye(), np.ones((N, K)), frames(), mask()), V,
         "temporal_fill_blend_batch: gains (3, 2) are not [n=3, K=2, 3]"),
        ("sharp_transfer_batch-ratio", lambda c: c.sharp_transfer_batch(frames(), nmats(), cand(), np.ones((N, 3)), 0.5, frames()), V,
         "sharp_transfer_batch: ratio (3, 3) is not [n=3, K=2]"),
        ("spatial_fill_batch-dst", lambda c: c.spatial_fill_batch(strided(), mask()), V, f"spatial_fill_batch: dst {TENSOR}"),
        ("spatial_fill_batch-dst-host", lambda c: c.spatial_fill_batch(frames().numpy(), mask()), V, f"spatial_fill_batch: dst {TENSOR}"),
        ("spatial_fill_batch-mask", lambda c: c.spatial_fill_batch(frames(), None), V, f"spatial_fill_batch: mask {TENSOR}"),
        ("spatial_fill_batch-shapes", lambda c: c.spatial_fill_batch(frames(), mask(n=2)), V,
         "spatial_fill_batch: dst (3, 8, 10, 3) / mask (2, 8, 10) do not match"),
        ("spatial_fill_batch-shapes-transposed", lambda c: c.spatial_fill_batch(frames(), mask(h=W, w=H)), V,
         "spatial_fill_batch: dst (3, 8, 10, 3) / mask (3, 10, 8) do not match"),
        ("spatial_fill_batch-chunk", lambda c: c.spatial_fill_batch(frames(), mask(), chunk_frames=-1), V,
         "spatial_fill_batch: chunk_frames=-1 is negative"),
        (f"{who}-a", sse(a=strided()), E, f"{who}: a {TENSOR}"),
        (f"{who}-b", sse(b=frames().double()), E, f"{who}: b {TENSOR}"),
        (f"{who}-mask-a", sse(ma=mask().double()), E, f"{who}: mask_a {TENSOR}"),
        (f"{who}-mask-b", sse(mb=mask().numpy()), E, f"{who}: mask_b {TENSOR}"),
        (f"{who}-a-shape", sse(a=frames(ch=4), b=frames(ch=4)), E, f"{who}: a of shape (3, 8, 10, 4) is not [n,h,w,3]"),
        (f"{who}-b-shape", sse(b=frames(n=2)), E, f"{who}: b of shape (2, 8, 10, 3) does not match a (3, 8, 10, 3)"),
        (f"{who}-mask-a-shape", sse(ma=mask(n=2)), E, f"{who}: mask_a of shape (2, 8, 10) does not match the frames: expected (3, 8, 10)"),
        (f"{who}-mask-b-shape", sse(mb=mask(n=2)), E, f"{who}: mask_b of shape (2, 8, 10) does not match the frames: expected (3, 8, 10)"),
        ("apply_gain_batch-frames", lambda c: c.apply_gain_batch(strided(), np.ones((N, 3))), E, f"apply_gain_batch: frames {TENSOR}"),
        ("apply_gain_batch-mask", lambda c: c.apply_gain_batch(frames(), np.ones((N, 3)), mask().double()), E, f"apply_gain_batch: mask {TENSOR}"),
        ("apply_gain_batch-shape", lambda c: c.apply_gain_batch(frames(ch=4), np.ones((N, 3))), E,
         "apply_gain_batch: frames of shape (3, 8, 10, 4) are not [n,h,w,3]"),
        ("apply_gain_batch-mask-shape", lambda c: c.apply_gain_batch(frames(), np.ones((N, 3)), mask(n=2)), E,
         "apply_gain_batch: mask of shape (2, 8, 10) does not match the frames: expected (3, 8, 10)"),
        ("apply_gain_batch-gains", lambda c: c.apply_gain_batch(frames(), np.ones((N, 4))), E, "apply_gain_batch: gains of shape (3, 4) are not [3,3]"),
        ("mask_moments_batch-tensor", lambda c: c.mask_moments_batch(mask().double()), E, f"mask_moments_batch: mask {TENSOR}"),
        ("mask_moments_batch-shape", lambda c: c.mask_moments_batch(frames()), E, "mask_moments_batch: mask of shape (3, 8, 10, 3) is not [n,h,w]"),
        ("orientation_hist_batch-tensor", lambda c: c.orientation_hist_batch(mask(), 0), E,
         "orientation_hist_batch: gray must be a contiguous uint8 tensor on cpu"),
        ("orientation_hist_batch-shape", lambda c: c.orientation_hist_batch(gray()[0], 0), E, "orientation_hist_batch: gray of shape (8, 10) is not [n,h,w]"),
        ("orientation_hist_batch-min", lambda c: c.orientation_hist_batch(gray(), -1), E,
         "orientation_hist_batch: min_mag2=-1 is not an integer in [0, 2^32 - 1]"),
        ("orientation_hist_batch-min-large", lambda c: c.orientation_hist_batch(gray(), 1 << 32), E,
         "orientation_hist_batch: min_mag2=4294967296 is not an integer in [0, 2^32 - 1]"),
        ("orientation_hist_batch-min-bool", lambda c: c.orientation_hist_batch(gray(), True), E,
         "orientation_hist_batch: min_mag2=True is not an integer in [0, 2^32 - 1]"),
        ("orientation_hist_batch-min-float", lambda c: c.orientation_hist_batch(gray(), 4.0), E,
         "orientation_hist_batch: min_mag2=4.0 is not an integer in [0, 2^32 - 1]"),
        ("frame_sharpness_batch-tensor", lambda c: c.frame_sharpness_batch(strided()), E, f"frame_sharpness_batch: frames {TENSOR}"),
        ("frame_sharpness_batch-shape", lambda c: c.frame_sharpness_batch(mask()), E,
         "frame_sharpness_batch: frames of shape (3, 8, 10) are not [n,h,w,3]"),
        ("lk_track_batch-pairs", lambda c: c.lk_track_batch(gray(n=1), _t().zeros((1, 4, 2)), i32(1)), V, "lk_track_batch needs at least two frames"),
        ("phase_correlate_batch-dtype", lambda c: c.phase_correlate_batch(mask()), E, "phase_correlate_batch expects a uint8 [N,h,w] tensor"),
        ("phase_correlate_batch-pairs", lambda c: c.phase_correlate_batch(gray(n=1)), E, "phase_correlate_batch needs at least two frames"),
    ]
    for who in ("pair_gain_hist_batch", "pair_gain_sums_batch"):
        def call(src=None, tr=None, active=None, band=None, _who=who):
            src = frames() if src is None else src
            tr = eye(P) if tr is None else tr
            if _who == "pair_gain_hist_batch":
                return lambda c: c.pair_gain_hist_batch(src, tr, active)
            return lambda c: c.pair_gain_sums_batch(src, tr, np.zeros((P, 4, 2), np.int32) if band is None else band, active)

        rows += [
            (f"{who}-src", call(src=strided()), E, f"{who}: src {TENSOR}"),
            (f"{who}-src-shape", call(src=frames(ch=4)), E, f"{who}: src of shape (3, 8, 10, 4) is not [n,h,w,3] with n >= 2"),
            (f"{who}-src-one", call(src=frames(n=1), tr=eye(0)), E, f"{who}: src of shape (1, 8, 10, 3) is not [n,h,w,3] with n >= 2"),
            (f"{who}-transitions", call(tr=eye(N)), E, f"{who}: transitions (3, 3, 3) are not [2,3,3] for 3 frames"),
            (f"{who}-active", call(active=[1, 1, 1]), E, f"{who}: active of shape (3,) is not [2]"),
        ]
    rows.append(("pair_gain_sums_batch-band", call(band=np.zeros((P, 4), np.int32)), E, "pair_gain_sums_batch: band of shape (2, 4) is not [2,4,2]"))
    for who in ("mask_hold_batch", "mask_grow_batch"):
        call = (lambda m, _who=who: (lambda c: getattr(c, _who)(m, 1)))
        rows += [
            (f"{who}-tensor", call(mask().double()), E, f"{who}: mask {TENSOR}"),
            (f"{who}-shape", call(frames()), E, f"{who}: mask of shape (3, 8, 10, 3) is not [n,h,w] with n, h, w >= 1"),
            (f"{who}-empty", call(mask(n=0)), E, f"{who}: mask of shape (0, 8, 10) is not [n,h,w] with n, h, w >= 1"),
        ]
    shared = mask()
    rows += [
        ("mask_hold_batch-hold", lambda c: c.mask_hold_batch(mask(), 17), E, "mask_hold_batch: hold=17 is not an integer in 0..16"),
        ("mask_hold_batch-hold-bool", lambda c: c.mask_hold_batch(mask(), True), E, "mask_hold_batch: hold=True is not an integer in 0..16"),
        ("mask_hold_batch-hold-float", lambda c: c.mask_hold_batch(mask(), 1.0), E, "mask_hold_batch: hold=1.0 is not an integer in 0..16"),
        ("mask_hold_batch-shots-length", lambda c: c.mask_hold_batch(mask(), 1, [0, 0]), E,
         "mask_hold_batch: shots of shape (2,) is not a non-decreasing sequence of n=3 integers"),
        ("mask_hold_batch-shots-order", lambda c: c.mask_hold_batch(mask(), 1, [0, 1, 0]), E,
         "mask_hold_batch: shots of shape (3,) is not a non-decreasing sequence of n=3 integers"),
        ("mask_grow_batch-grow", lambda c: c.mask_grow_batch(mask(), -65), E, "mask_grow_batch: grow=-65 is not an integer in -64..64"),
        ("mask_grow_batch-grow-bool", lambda c: c.mask_grow_batch(mask(), False), E, "mask_grow_batch: grow=False is not an integer in -64..64"),
        ("mask_grow_batch-feather", lambda c: c.mask_grow_batch(mask(), 1, feather=65), E, "mask_grow_batch: feather=65 is not an integer in 0..64"),
        ("mask_grow_batch-feather-float", lambda c: c.mask_grow_batch(mask(), 1, feather=1.0), E,
         "mask_grow_batch: feather=1.0 is not an integer in 0..64"),
        ("mask_grow_batch-tapered", lambda c: c.mask_grow_batch(mask(), 1, tapered=1), E, "mask_grow_batch: tapered=1 is not a bool"),
        ("mask_grow_batch-out", lambda c: c.mask_grow_batch(mask(), 1, out=mask(n=2)), E,
         "mask_grow_batch: out must be a contiguous float32 tensor of shape (3, 8, 10) on cpu"),
        ("mask_grow_batch-out-dtype", lambda c: c.mask_grow_batch(mask(), 1, out=mask().double()), E,
         "mask_grow_batch: out must be a contiguous float32 tensor of shape (3, 8, 10) on cpu"),
        ("mask_grow_batch-out-shared", lambda c: c.mask_grow_batch(shared, 1, out=shared), E,
         "mask_grow_batch: out shares memory with mask: a tile's halo would read pixels already written"),
    ]
    return rows


# refusals that come behind a library call the method makes ahead of its checks today
CALLS_AHEAD = {
    "dis_flow_batch-pairs": ("vstab_dis_set_clip_start",),        # the clip-start flag is set before gray is looked at
    "fit_records_device-none": ("vstab_fit_records_device",),     # the refusal IS the library's answer (a NULL address)
}

REFUSALS = (_three_channel_rows() + _neighbour_rows() + _anchor_rows() + _residual_rows() + _displaced_rows() + _plate_rows()
            + _other_rows())


def test_refusal_ids_are_unique():
    ids = [r[0] for r in REFUSALS]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_class_and_text(pkg, case):
    """Every refusal of a public Context method: its class, its exact text, and that it comes before any library call."""
    from vstab_amd import native

    case_id, call, exc, text = case
    ctx = make_context(native, RaisingLib(CALLS_AHEAD.get(case_id, ())))
    with pytest.raises((native.VstabError, ValueError)) as info:
        call(ctx)
    assert type(info.value) is {V: native.VstabError, E: ValueError}[exc]
    assert str(info.value) == text


# ---------------------------------------------------------------- call records
def _flags(**names):
    """Every combination of the named flags: [{name: value, ...}, ...]."""
    import itertools

    keys = list(names)
    return [dict(zip(keys, combo)) for combo in itertools.product(*(names[k] for k in keys))]


def _tag(kw):
    return ",".join(f"{k}={'given' if callable(v) else v}" for k, v in kw.items()) or "plain"


TF = (True, False)


def call_cases():
    """(id, call(ctx)) of every public method that reaches the library, once per combination that changes the argument list."""
    torch = _t()
    cases = []

    def add(name, call, label=None, **kw):
        cases.append((f"{name}[{label or _tag(kw)}]", lambda c, call=call, kw=kw: call(c, **kw)))

    def opt(make):
        """An optional tensor or array: once given, once None."""
        return (make, None)

    def given(v):
        return v() if callable(v) else v

    add("synchronize", lambda c: c.synchronize())
    for kw in ({"enabled": False}, {"enabled": True}, {"enabled": True, "detail": True}, {"enabled": True, "warp_only": True}):
        add("set_timing", lambda c, **kw: c.set_timing(**kw), **kw)
    add("dis_stage_ms", lambda c: c.dis_stage_ms())
    add("last_kernel_ms", lambda c: c.last_kernel_ms("warp"))
    add("kernel_ms_stats", lambda c: c.kernel_ms_stats("warp"))
    add("upload", lambda c: c.upload(frames()), "float32")
    add("upload", lambda c: c.upload(i32(N, 4)), "int32")
    add("upload_u8_as_f32", lambda c: c.upload_u8_as_f32(gray()))
    add("download", lambda c: c.download(mask()))
    add("download", lambda c: c.download(mask(), mask=True, levels=5), "mask")
    add("download", lambda c: c.download(gray(), mask=True), "mask,uint8")
    for kw in _flags(want_mask=TF, want_count=TF, out=opt(frames), out_mask=opt(mask)):
        add("warp_batch", lambda c, out, out_mask, **kw: c.warp_batch(frames(), eye(), SIZE, out=given(out), out_mask=given(out_mask), **kw), **kw)
    add("warp_batch", lambda c: c.warp_batch(frames().numpy(), eye(), (W + 2, H + 2), interp="bicubic", subpix="exact", border=(0.1, 0.2, 0.3)),
        "host,bicubic,exact")
    for kw in _flags(want_mask=TF, out=opt(frames), out_mask=opt(mask)):
        add("warp_blur_batch", lambda c, out, out_mask, **kw: c.warp_blur_batch(
            frames(), eye(dtype=np.float64), SIZE, 0.5, 5, out=given(out), out_mask=given(out_mask), **kw), **kw)
    add("warp_blur_batch", lambda c: c.warp_blur_batch(frames(n=2), eye(5, np.float64), SIZE, 0.5, 5, clip_first=2), "clip_first=2")
    for kw in _flags(want_range=TF, work_size=((5, 4), None)):
        add("gray_downscale", lambda c, work_size, **kw: c.gray_downscale(frames(), work_size, **kw), **kw)
    add("last_pad_counts", lambda c: c.last_pad_counts(N))
    add("last_frame_peaks", lambda c: c.last_frame_peaks(N))
    add("frame_range", lambda c: c.frame_range(frames()))
    add("apply_value_range", lambda c: c.apply_value_range(frames(), torch.zeros(N)))
    for kw in _flags(want_full=TF, want_grid=TF, clip_start=TF):
        add("dis_flow_batch", lambda c, **kw: c.dis_flow_batch(gray(), sample_step=STEP, **kw), **kw)
    for kw in _flags(want_full=TF, want_grid=TF, want_iterations=TF):
        add("tvl1_flow_batch", lambda c, **kw: c.tvl1_flow_batch(gray(), sample_step=STEP, **kw), **kw)
    add("tvl1_flow_batch", lambda c: c.tvl1_flow_batch(gray(), {"warps": 2, "nscales": 3}, want_iterations=True), "params=dict")
    add("mask_block_grid", lambda c: c.mask_block_grid(mask(), N, None, STEP, 2), "working_size=None")
    add("mask_block_grid", lambda c: c.mask_block_grid(np.zeros((H, W)), N, (5, 4), 2, 0), "host,working_size")
    add("pair_residual_batch", lambda c: c.pair_residual_batch(gray(), eye(P)))
    add("anchor_sums_batch", lambda c: c.anchor_sums_batch(gray(), np.full(N, -1), np.zeros((N, 6)), 32))
    for kw in _flags(gain=opt(lambda: np.full(N, 1024)), offset=opt(lambda: np.zeros(N, np.int64)), blocked=opt(blocked)):
        add("anchor_sums_ex_batch", lambda c, gain, offset, blocked: c.anchor_sums_ex_batch(
            gray(), np.array([-1, 0, 0]), np.zeros((N, 2, 3)), 32.0, given(gain), given(offset), given(blocked), step=STEP), **kw)
    for kw in _flags(blocked=opt(blocked)):
        add("mesh_residual_batch", lambda c, blocked: c.mesh_residual_batch(grid_flow(), STEP, SIZE, eye(P), 3, 2, given(blocked)), **kw)
        add("row_residual_batch", lambda c, blocked: c.row_residual_batch(grid_flow(), STEP, SIZE, eye(P), given(blocked)), **kw)
        add("sample_fit_batch", lambda c, blocked: c.sample_fit_batch(grid_flow(), STEP, "similarity", given(blocked)), **kw)
        add("sample_fit_batch_begin", lambda c, blocked: c.sample_fit_batch_begin(grid_flow(), STEP, "perspective", given(blocked)), **kw)
    for kw in _flags(blocked=opt(blocked), velocity=opt(lambda: np.zeros((N, 6)))):
        add("rectify_samples_batch", lambda c, blocked, velocity: c.rectify_samples_batch(
            grid_flow(), STEP, SIZE, given(velocity), -0.25, given(blocked)), **kw)
    for kw in _flags(want_mask=TF, want_count=TF):
        add("mesh_warp_batch", lambda c, **kw: c.mesh_warp_batch(frames(), eye(), SIZE, offsets(), **kw), **kw)
        add("rolling_warp_batch", lambda c, **kw: c.rolling_warp_batch(frames(), eye(), SIZE, np.zeros((N, 6)), 0.5, **kw), **kw)
        add("warp_batch_planned", lambda c, **kw: c.warp_batch_planned(frames(), 1, SIZE, **kw), **kw)
    for kw in _flags(want_mask=TF, want_count=TF, want_unconverged=TF):
        add("mesh_unwarp_batch", lambda c, **kw: c.mesh_unwarp_batch(frames(), eye(), SIZE, torch.zeros((N, 2, 3, 2)), **kw), **kw)
    for kw in _flags(want_mask=TF, want_count=TF, want_unsolved=TF, velocity=opt(lambda: np.zeros((N, 6)))):
        add("rolling_unwarp_batch", lambda c, velocity, **kw: c.rolling_unwarp_batch(frames(), eye(), SIZE, given(velocity), 0.5, **kw), **kw)
    for kw in _flags(offsets=opt(offsets)):
        add("cover_extent_batch", lambda c, offsets: c.cover_extent_batch(eye(), SIZE, (W + 2, H + 2), given(offsets)), **kw)
    add("fit_records_device", lambda c: pytest.raises(Exception, c.fit_records_device))     # the stub's 0 is "no fit is pending"
    add("sample_fit_batch_end", lambda c: c.sample_fit_batch_end(P))
    add("fit_records_copy", lambda c: c.fit_records_copy(torch.zeros(P * 3 * 72, dtype=torch.uint8), P))
    for kw in _flags(working_size=((5, 4), None), seg_pairs=opt(lambda: [2, 1]), warp_frames=(0, N), framing=("crop_and_pad", "expand")):
        add("flow_plan_device", lambda c, working_size, seg_pairs, warp_frames, framing: c.flow_plan_device(
            1 << 40, P, "similarity", SIZE, working_size, 1.5, 30.0, 0.75, True, given(seg_pairs), 2, warp_frames, framing), **kw)

    def planned_then_warp(c, want_mask, want_count):
        c.flow_plan_device(1 << 40, P, "similarity", SIZE, None, 1.5, 30.0, 0.75, False, warp_frames=N)
        return c.warp_batch_planned(frames(), 0, SIZE, want_mask=want_mask, want_count=want_count)

    for kw in _flags(want_mask=TF, want_count=TF):
        add("flow_plan_device+warp_batch_planned", planned_then_warp, **kw)
    add("flow_plan_result", lambda c: c.flow_plan_result(N, 4))
    for kw in _flags(want_filled_from=TF, want_counts=TF):
        add("temporal_fill_batch", lambda c, **kw: c.temporal_fill_batch(frames(5), nmats(), cand(), frames(), mask(), first=1, **kw), **kw)
        add("temporal_fill_blend_batch", lambda c, **kw: c.temporal_fill_blend_batch(
            frames(5), nmats(), cand(), eye(), np.ones((N, K, 3)), frames(), mask(), feather_px=3, first=1, **kw), **kw)
    add("temporal_fill_batch", lambda c: c.temporal_fill_batch(frames(), nmats(), cand(), frames(), mask(), interp="bicubic", subpix="exact"),
        "bicubic,exact")
    add("fill_gain_sums", lambda c: c.fill_gain_sums(frames(5), nmats(), cand(), eye(), frames(), first=1))
    for kw in _flags(want_counts=TF):
        add("spatial_fill_batch", lambda c, **kw: c.spatial_fill_batch(frames(), mask(), chunk_frames=2, **kw), **kw)
    add("spatial_fill_batch", lambda c: c.spatial_fill_batch(frames(n=0), mask(n=0)), "empty")
    for kw in _flags(mask_a=opt(mask), mask_b=opt(mask)):
        add("frame_sse_batch", lambda c, mask_a, mask_b: c.frame_sse_batch(frames(), frames(), given(mask_a), given(mask_b)), **kw)
    for kw in _flags(active=opt(lambda: [1, 0])):
        add("pair_gain_hist_batch", lambda c, active: c.pair_gain_hist_batch(frames(), eye(P), given(active)), **kw)
        add("pair_gain_sums_batch", lambda c, active: c.pair_gain_sums_batch(frames(), eye(P), np.zeros((P, 4, 2)), given(active)), **kw)
    for kw in _flags(mask=opt(mask), want_count=TF):
        add("apply_gain_batch", lambda c, mask, want_count: c.apply_gain_batch(frames(), np.ones((N, 3)), given(mask), want_count), **kw)
    add("mask_moments_batch", lambda c: c.mask_moments_batch(mask()))
    add("orientation_hist_batch", lambda c: c.orientation_hist_batch(gray(), 0xFFFFFFFF))
    for kw in _flags(mask=opt(mask)):
        add("plate_median_batch", lambda c, mask: c.plate_median_batch(frames(), given(mask), [[0, 1, 2, -1], [2, -1, -1, -1]]), **kw)
    for kw in _flags(shot=opt(lambda: [0, 0, 1])):
        shots = 2 if kw["shot"] is not None else 1
        add("plate_fill_batch", lambda c, shot, shots=shots: c.plate_fill_batch(frames(), mask(), plate(shots), pcount(shots), given(shot), 2), **kw)
    for kw in _flags(mask=opt(mask), shot=opt(lambda: [0, 0, 1])):
        shots = 2 if kw["shot"] is not None else 1
        add("plate_matte_batch", lambda c, mask, shot, shots=shots: c.plate_matte_batch(
            frames(), given(mask), plate(shots), pcount(shots), given(shot), 0.1, 3), **kw)
    add("frame_sharpness_batch", lambda c: c.frame_sharpness_batch(frames()))
    for kw in _flags(mask=opt(mask), want_counts=TF):
        add("sharp_transfer_batch", lambda c, mask, want_counts: c.sharp_transfer_batch(
            frames(5), nmats(), cand(), np.ones((N, K)), 0.5, frames(), given(mask), first=1, want_counts=want_counts), **kw)
    for kw in _flags(shots=opt(lambda: [0, 0, 1])):
        add("mask_hold_batch", lambda c, shots: c.mask_hold_batch(mask(), 2, given(shots)), **kw)
    for kw in _flags(tapered=TF, want_count=TF, out=opt(mask)):
        add("mask_grow_batch", lambda c, out, **kw: c.mask_grow_batch(mask(), -3, feather=5, out=given(out), **kw), **kw)
    add("gftt_batch", lambda c: c.gftt_batch(gray(), max_corners=6))
    for kw in _flags(want_raw=TF):
        add("lk_track_batch", lambda c, **kw: c.lk_track_batch(gray(), torch.zeros((N, 6, 2)), i32(N), **kw), **kw)
    add("points_fit_batch", lambda c: c.points_fit_batch(torch.zeros((P, 6, 4)), i32(N), "translation"))
    add("phase_correlate_batch", lambda c: c.phase_correlate_batch(gray()))
    add("crop_analysis", lambda c: c.crop_analysis(eye(), SIZE, (W + 2, H + 2)))
    add("common_coverage", lambda c: c.common_coverage(eye(), SIZE, (W + 2, H + 2)))
    add("trajectory", lambda c: c.trajectory(np.zeros((P, 4)), 1.5, 30.0, 0.75, True))
    return cases


def run_cases(native):
    """{case id: [[entry point, stream set directly before, [arguments]], ...]}"""
    out = {}
    for case_id, call in call_cases():
        events = []
        call(make_context(native, RecordingLib(events), events))
        assert case_id not in out, case_id
        out[case_id] = [e for e in events if e != "stream"]
    return out


def record():
    """Writes the golden records from the code as it stands (run once, at the commit the refactor started from)."""
    import os

    os.environ.pop("VSTAB_XFER_CODED", None)
    os.environ.pop("VSTAB_SUBPIX", None)
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as graft

    graft.load_package()
    from vstab_amd import native

    GOLDEN.write_text(json.dumps(run_cases(native), indent=0, separators=(",", ":")) + "\n")
    print(f"{GOLDEN}: {len(json.loads(GOLDEN.read_text()))} cases")


# Entry points that take a context and are reached by no public Context method.
CONTEXT_ITSELF = {     # they manage the context itself: Context.__init__ / close / use_torch_stream, which the stub replaces
    "vstab_create", "vstab_destroy", "vstab_set_stream",
}
UNBOUND = {            # declared, exported and listed in _SIGNATURES, but no Context method calls them (tests reach them through
    "vstab_download_mask_coded",   # ctx.lib): download() takes vstab_download_mask_levels, of which this is levels = 1,
    "vstab_warp_blur_batch",       # warp_blur_batch() takes vstab_warp_blur_clip_batch, of which this is first = 0, total = n
}


def context_entry_points():
    from tests.test_abi_cpu import header_prototypes

    return {name for name, params, _ in header_prototypes(any_return=True) if params and params[0].startswith("vstab_ctx*")}


def test_call_records_match_the_golden_file(pkg, monkeypatch):
    from vstab_amd import native

    monkeypatch.delenv("VSTAB_XFER_CODED", raising=False)
    monkeypatch.setattr(native, "DEFAULT_SUBPIX", "q5")
    golden = json.loads(GOLDEN.read_text())
    got = json.loads(json.dumps(run_cases(native)))
    assert set(got) == set(golden)
    for case_id in golden:
        assert got[case_id] == golden[case_id], case_id


def test_call_records_cover_every_context_entry_point(pkg):
    """Every entry point of _SIGNATURES whose first parameter is a vstab_ctx* is in the records, but for the three that manage
    the context itself -- and the two that native.py binds nowhere, which is asserted here so that a binding added for one of
    them has to be recorded."""
    from vstab_amd import native

    golden = json.loads(GOLDEN.read_text())
    recorded = {entry[0] for calls in golden.values() for entry in calls}
    with_context = context_entry_points()
    assert with_context <= set(native._SIGNATURES)
    assert CONTEXT_ITSELF | UNBOUND <= with_context
    assert recorded == with_context - CONTEXT_ITSELF - UNBOUND
    source = (Path(native.__file__)).read_text()
    body = source[source.index("EXPORTED_SYMBOLS = "):]
    for name in UNBOUND:
        short = name[len("vstab_"):]
        assert f"{name}(" not in body and f'_call("{short}"' not in body, f"{name} is bound now: record its call and drop it from UNBOUND"


if __name__ == "__main__":
    record()
