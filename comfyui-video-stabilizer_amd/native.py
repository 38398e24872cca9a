"""ctypes binding of libvstab.so (include/vstab.h) -- the only compute path of this package.

There is no CPU fallback: if the HIP library is missing or no MI355X is visible every
entry point raises.  torch tensors are used as the device-memory container only.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np

_PKG_DIR = Path(__file__).resolve().parent
# VSTAB_LIB: another build of the library (A/B measurements of kernel variants inside one GPU session, tools/*.py)
LIB_PATH = Path(os.environ["VSTAB_LIB"]).resolve() if os.environ.get("VSTAB_LIB") else _PKG_DIR / "lib" / "libvstab.so"

INTERP = {"bilinear": 0, "bicubic": 1}
SUBPIX = {"q5": 0, "exact": 1}
MODES = {"translation": 0, "similarity": 1, "perspective": 2}
GROW_TAPERED, GROW_SQUARE = 0, 1                               # VSTAB_GROW_* of include/vstab.h
MASK_HOLD_MAX, MASK_GROW_MAX, MASK_FEATHER_MAX = 16, 64, 64    # VSTAB_MASK_*_MAX
MODE_NAMES = ("translation", "similarity", "perspective")
MESH_MAX_VERTS = 65      # vertices per axis of a mesh warp (64 cells; include/vstab.h)
MESH_MIN_SAMPLES = 4     # VSTAB_MESH_MIN_SAMPLES
ORIENTATION_K = 256      # VSTAB_ORIENTATION_K
PLATE_SAMPLES_MAX = 256  # VSTAB_PLATE_SAMPLES_MAX
PLATE_REGISTER_MAX = 64  # VSTAB_PLATE_REGISTER_MAX: the widest row the register form of the median kernel takes
# the sample counts at which vstab_plate_median_batch changes kernel: 4 / 8 / 16 / 32 / 64 key registers, then 128 / 256 LDS rows
PLATE_PATH_STEPS = (4, 8, 16, 32, PLATE_REGISTER_MAX, 128)

# Sub-pixel model used by the node path; see include/vstab.h (vstab_subpix) and DESIGN.md.
DEFAULT_SUBPIX = os.environ.get("VSTAB_SUBPIX", "q5")


class VstabError(RuntimeError):
    pass


class FitRecord(C.Structure):
    _fields_ = [
        ("matrix", C.c_float * 9),
        ("confidence", C.c_double),
        ("residual", C.c_double),
        ("accepted", C.c_int32),
        ("computed", C.c_int32),
        ("valid_points", C.c_int32),
        ("total_points", C.c_int32),
    ]


class Tvl1Params(C.Structure):
    """vstab_tvl1_params (include/vstab.h): cv2.optflow.DualTVL1OpticalFlow's parameters."""
    _fields_ = [
        ("tau", C.c_double), ("lambda_", C.c_double), ("theta", C.c_double), ("epsilon", C.c_double),
        ("scale_step", C.c_double), ("gamma", C.c_double),
        ("nscales", C.c_int), ("warps", C.c_int), ("inner_iterations", C.c_int), ("outer_iterations", C.c_int),
        ("median_filtering", C.c_int), ("use_initial_flow", C.c_int), ("chunk_pairs", C.c_int), ("poll_interval", C.c_int),
    ]


def tvl1_params(**overrides) -> Tvl1Params:
    """The library's defaults (OpenCV's DualTVL1OpticalFlow_create()) with `overrides` applied; `lambda_` is lambda."""
    prm = Tvl1Params()
    load_library().vstab_tvl1_default_params(C.byref(prm))
    for key, value in overrides.items():
        if key not in dict(Tvl1Params._fields_):
            raise ValueError(f"unknown TV-L1 parameter {key!r}")
        setattr(prm, key, value)
    return prm


# numpy view of vstab_fit_record (include/vstab.h): same layout as the ctypes structure above
FIT_DTYPE = np.dtype({
    "names": ["matrix", "confidence", "residual", "accepted", "computed", "valid_points", "total_points"],
    "formats": [(np.float32, (9,)), np.float64, np.float64, np.int32, np.int32, np.int32, np.int32],
    "offsets": [0, 40, 48, 56, 60, 64, 68],
    "itemsize": 72,
})
assert C.sizeof(FitRecord) == FIT_DTYPE.itemsize


def fit_table_from_dicts(records) -> np.ndarray:
    """List of {mode_name: candidate dict} (the oracle-side shape used in tests) -> structured [P,3] table."""
    table = np.zeros((len(records), 3), FIT_DTYPE)
    table["matrix"][:] = np.eye(3, dtype=np.float32).reshape(9)
    for p, entry in enumerate(records):
        for mi, name in enumerate(MODE_NAMES):
            cand = entry.get(name)
            if cand is None:
                continue
            row = table[p, mi]
            row["matrix"] = np.asarray(cand["matrix"], np.float32).reshape(9)
            row["confidence"] = cand["confidence"]
            row["residual"] = cand["residual"]
            row["accepted"] = 1 if cand["accepted"] else 0
            row["computed"] = 1
            row["valid_points"] = cand.get("valid_points", 0)
            row["total_points"] = cand.get("total_points", 0)
    return table


def fit_table_to_dicts(table: np.ndarray):
    out = []
    for p in range(table.shape[0]):
        entry = {}
        for mi, name in enumerate(MODE_NAMES):
            r = table[p, mi]
            if not r["computed"]:
                continue
            entry[name] = {
                "matrix": np.array(r["matrix"], dtype=np.float32).reshape(3, 3),
                "confidence": float(r["confidence"]),
                "residual": float(r["residual"]),
                "accepted": bool(r["accepted"]),
                "valid_points": int(r["valid_points"]),
                "total_points": int(r["total_points"]),
            }
        out.append(entry)
    return out


_SIGNATURES = {
    "vstab_abi_version": (C.c_int, []),
    "vstab_last_pad_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_flow_plan_zero_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "vstab_last_frame_peaks": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_test_hooks": (C.c_int, []),
    "vstab_last_error": (C.c_char_p, []),
    "vstab_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "vstab_destroy": (C.c_int, [C.c_void_p]),
    "vstab_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vstab_synchronize": (C.c_int, [C.c_void_p]),
    "vstab_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "vstab_last_kernel_ms": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_float)]),
    "vstab_kernel_ms_stats": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "vstab_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "vstab_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "vstab_upload_f32_coded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "vstab_upload_u8_as_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "vstab_download_mask_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int)]),
    "vstab_download_mask_coded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "vstab_warp_batch": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "vstab_warp_blur_batch": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
         C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    ),
    "vstab_warp_blur_clip_batch": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
         C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    ),
    "vstab_blur_sample_matrices": (
        C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_common_coverage": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_gray_downscale": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_gray_downscale_range": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_frame_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_apply_value_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_dis_flow_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "vstab_dis_set_clip_start": (C.c_int, [C.c_void_p, C.c_int]),
    "vstab_sample_fit_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_sample_fit_batch_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "vstab_mask_block_grid": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_sample_fit_batch_masked": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_sample_fit_batch_begin_masked": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_pair_residual_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_anchor_sums_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_anchor_sums_ex_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_mesh_residual_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                  C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_mesh_warp_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_mesh_unwarp_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_rolling_warp_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_rolling_unwarp_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_row_residual_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p]),
    "vstab_rectify_samples_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_cover_extent_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                  C.c_void_p]),
    "vstab_fit_records_device": (C.c_void_p, [C.c_void_p]),
    "vstab_sample_fit_batch_end": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_flow_plan_device": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int,
                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "vstab_fit_records_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "vstab_flow_plan_result": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_warp_batch_planned": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_temporal_fill_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_fill_gain_sums": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_temporal_fill_blend_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p]),
    "vstab_spatial_fill_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_frame_sse_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_mask_moments_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_frame_sharpness_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_sharp_transfer_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_mask_hold_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_mask_grow_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_pair_gain_hist_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_pair_gain_sums_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_apply_gain_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_orientation_hist_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]),
    "vstab_plate_median_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_plate_fill_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                  C.c_void_p]),
    "vstab_plate_matte_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                  C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_gftt_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p,
                  C.c_void_p]),
    "vstab_lk_levels": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "vstab_lk_track_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                  C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_points_fit_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vstab_phase_correlate_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_tvl1_default_params": (None, [C.c_void_p]),
    "vstab_tvl1_flow_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_host_math": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vstab_transitions_to_params": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vstab_params_to_matrices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vstab_bounding_boxes": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "vstab_crop_analysis": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vstab_trajectory": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p,
         C.c_void_p],
    ),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# include/vstab_track.h, the second public header of the same library: a table of its own, applied by load_library() beside
# the one above and not part of EXPORTED_SYMBOLS (which is what include/vstab.h declares)
_TRACK_SIGNATURES = {
    "vstab_track_template_batch": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
TRACK_SENTINEL = (1 << 64) - 1     # VSTAB_TRACK_SENTINEL
TRACK_RADIUS_MAX = 48              # VSTAB_TRACK_RADIUS_MAX
TRACK_MIN_BOX = 8                  # VSTAB_TRACK_MIN_BOX
TRACK_MAX_SAMPLES = 4096           # VSTAB_TRACK_MAX_SAMPLES


def track_work_words(radius: int) -> int:
    """VSTAB_TRACK_WORK_WORDS(radius): the 64-bit words of scratch vstab_track_template_batch needs."""
    d = 2 * int(radius) + 1
    return TRACK_MAX_SAMPLES // 8 + 2 * (d * d + 2 * d)

_lib = None


def load_library():
    """Load libvstab.so; raises VstabError if it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise VstabError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). This package has no CPU fallback."
            )
        # torch first: its wheel bundles its own libamdhip64.so.7 (+ libhsa-runtime64), and libvstab.so needs the same
        # SONAME.  Loaded after torch, libvstab binds to torch's copy: one HIP runtime in the process, torch's streams
        # and allocations are ours.  Loaded BEFORE torch it would pull in /opt/rocm's copy, torch would then find the
        # SONAME taken and run on a runtime that does not match its other bundled libraries ("no ROCm-capable device").
        import torch  # noqa: F401

        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in {**_SIGNATURES, **_TRACK_SIGNATURES}.items():
            fn = getattr(lib, name)  # AttributeError here means the ABI and the header diverged
            fn.restype = res
            fn.argtypes = args
        if lib.vstab_abi_version() != 1:
            raise VstabError(f"libvstab ABI version {lib.vstab_abi_version()} != 1")
        _lib = lib
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().vstab_last_error()
        raise VstabError(f"{what} failed ({rc}): {msg.decode('utf-8', 'replace') if msg else 'unknown error'}")


def _host_arg(full, v):
    """One argument of vstab_<...> as ctypes takes it: an array as its host address, None, ctypes objects and Python scalars
    as they are.  The caller hands over the array itself, so it is referenced for the whole call."""
    if isinstance(v, np.ndarray):
        if not v.flags.c_contiguous:
            raise VstabError(f"{full}: an array argument of shape {v.shape} is not contiguous")
        return v.ctypes.data
    return v


def _host_call(name, *args):
    """vstab_<name>(*args) for the entry points that take no context: Context._call without handle and stream."""
    full = "vstab_" + name
    _check(getattr(load_library(), full)(*[_host_arg(full, v) for v in args]), full)


def _int_in(who, name, v, lo, hi, span=None):
    """v as an int if it is an integer (a bool is not one) in lo..hi, else a ValueError; span: the range as the text spells it."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {name}={v!r} is not an integer in {span or f'{lo}..{hi}'}")
    return int(v)


def _shot_sequence(seq, n, refusal, shots=None):
    """seq -> contiguous i32 [n] if it is a non-decreasing sequence of n integers (in 0..shots-1 where `shots` is given),
    else ValueError(refusal)."""
    s = np.ascontiguousarray(seq, dtype=np.int32).reshape(-1)
    if s.shape[0] != n or (np.diff(s.astype(np.int64)) < 0).any() or (shots is not None and (s.min() < 0 or s.max() >= shots)):
        raise ValueError(refusal)
    return s


HOST_OPS = {"sqrt": 0, "atan2": 1, "log": 2, "exp": 3, "cos": 4, "sin": 5}


def host_math(op: str, a, b=None) -> np.ndarray:
    """Element-wise libm call over fp64 arrays (vstab_host_math): the functions Python's math module binds."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bb = np.ascontiguousarray(b, dtype=np.float64) if b is not None else None
    _host_call("host_math", HOST_OPS[op], a, bb, a.size, out)
    return out


PARAM_COUNT = {"translation": 2, "similarity": 4, "perspective": 8}


def transitions_to_params(work_mats, base_mode: str, source_size=None, working_size=None):
    """flow.py:340-346 for a clip (vstab_transitions_to_params): f32 [P,3,3] at working resolution ->
    (f32 [P,3,3] at full resolution, f64 [P,K] parameter deltas).  working_size None: estimated at full size."""
    m = np.ascontiguousarray(work_mats, dtype=np.float32).reshape(-1, 9)
    count = m.shape[0]
    full = np.empty((count, 9), np.float32)
    params = np.empty((count, PARAM_COUNT[base_mode]), np.float64)
    up = down = None
    if working_size is not None:
        sx = working_size[0] / float(source_size[0])
        sy = working_size[1] / float(source_size[1])
        up = np.array([1.0 / sx, 1.0 / sy, 1.0], np.float64)
        down = np.array([sx, sy, 1.0], np.float64)
    _host_call("transitions_to_params", m, count, MODES[base_mode], up, down, full, params)
    return full.reshape(count, 3, 3), params


def params_to_matrices(params, base_mode: str) -> np.ndarray:
    """_params_to_matrix for a clip (vstab_params_to_matrices): f64 [N,K] -> f32 [N,3,3]."""
    p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, PARAM_COUNT[base_mode])
    out = np.empty((p.shape[0], 3, 3), np.float32)
    _host_call("params_to_matrices", p, p.shape[0], MODES[base_mode], out)
    return out


def bounding_boxes(matrices, width: int, height: int):
    """_compute_bounding_boxes for a stacked f32 [N,3,3] array (vstab_bounding_boxes) -> (mins [N,2], maxs [N,2]) f64."""
    m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 9)
    mins = np.empty((m.shape[0], 2), np.float64)
    maxs = np.empty((m.shape[0], 2), np.float64)
    _host_call("bounding_boxes", m, m.shape[0], float(width), float(height), mins, maxs)
    return mins, maxs


def blur_sample_matrices(matrices64, first: int, count: int, blur: float, samples: int) -> np.ndarray:
    """The float32 shutter-sample matrices the blur warp uses for frames [first, first+count) of a clip
    (vstab_blur_sample_matrices; motion_apply.py:125-134 + the cast of :172) -> [count, S', 3, 3] float32."""
    m = np.ascontiguousarray(matrices64, dtype=np.float64).reshape(-1, 9)
    ts = np.ascontiguousarray(np.linspace(0.0, float(blur), int(samples), dtype=np.float64))
    per_frame = 1 if m.shape[0] <= 1 else int(samples)
    out = np.zeros((int(count), per_frame, 3, 3), np.float32)
    _host_call("blur_sample_matrices", m, m.shape[0], int(first), int(count), ts, int(samples), out)
    return out


def _coded_transfers():
    return os.environ.get("VSTAB_XFER_CODED", "1") not in ("0", "false", "False")


class Context:
    """One libvstab context bound to one GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device: Optional[int] = None):
        import torch

        if not torch.cuda.is_available():
            raise VstabError("no MI355X / HIP device visible: the stabilizer hot path has no CPU fallback")
        self.torch = torch
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.lib = load_library()
        handle = C.c_void_p()
        _check(self.lib.vstab_create(C.byref(handle), self.device_index), "vstab_create")
        self.handle = handle
        # what the most recent node-boundary transfers did (upload / download below): chunks that crossed PCIe as bytes of
        # all chunks; whether the mask came back as bytes
        self.last_upload_coded = (0, 0)
        self.last_download_coded = False
        self.use_torch_stream()

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.vstab_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def side_stream(self):
        """A second torch stream of this context's device (created once): for a pass that may run beside the main work."""
        s = getattr(self, "_side_stream", None)
        if s is None:
            s = self._side_stream = self.torch.cuda.Stream(device=self.device)
        return s

    def _call(self, name, *args, stream=True, check=True):
        """The one path into the library: vstab_<name>(handle, *args), after use_torch_stream() unless stream=False (an entry
        point that launches nothing, or whose caller has just set the stream), the status handed to _check (check=False: the
        value is returned as it is, for the entry point that returns an address and the query that may fail).  A tensor goes
        as its device address and an array as its host address: callers pass the object, not its address, so every buffer
        is referenced for the whole call.  None, ctypes objects and Python scalars go as they are.  A tensor or array that is
        not contiguous, or a tensor on another device, is refused here whatever the method checked before."""
        full = "vstab_" + name
        fn = getattr(self.lib, full)
        if stream:
            self.use_torch_stream()
        tensor = self.torch.Tensor
        converted = [self.handle]
        for v in args:
            if v is None or type(v) is int or type(v) is float:     # (most arguments: sizes and flags)
                converted.append(v)
            elif isinstance(v, tensor):
                if v.device != self.device or not v.is_contiguous():
                    raise VstabError(f"{full}: a tensor argument of shape {tuple(v.shape)} on {v.device} is not contiguous on {self.device}")
                converted.append(v.data_ptr())
            else:
                converted.append(_host_arg(full, v))
        rc = fn(*converted)
        if check:
            _check(rc, full)
        return rc

    def use_torch_stream(self) -> None:
        stream = self.torch.cuda.current_stream(self.device)
        self._call("set_stream", C.c_void_p(stream.cuda_stream), stream=False)

    def synchronize(self) -> None:
        self._call("synchronize", stream=False)

    def set_timing(self, enabled: bool, detail: bool = False, warp_only: bool = False) -> None:
        """detail: also bracket the stages inside a DIS call (a measurement pass of its own: see vstab.h).
        warp_only: events around the warp launches only (what a timed loop keeps: an event pair costs the stream ~10 us)."""
        level = 0 if not enabled else (3 if warp_only else (2 if detail else 1))
        self._call("set_timing", level, stream=False)

    def dis_stage_ms(self) -> Dict[str, Any]:
        """Milliseconds of the stages of the last DIS call under set_timing(True, detail=True):
        {"prep": pyramid + coarsest level's preparation, "pis4": {"L5": .., ..}, "level": {..}, "final": ..} -- levels by
        pyramid index (2 = the finest of the default configuration)."""
        def ms(kind):
            out = C.c_float()
            return float(out.value) if self._call("last_kernel_ms", kind.encode(), C.byref(out), stream=False, check=False) == 0 else None

        res: Dict[str, Any] = {"prep": ms("dis_prep"), "pis4": {}, "level": {}, "final": ms("dis_final")}
        for lvl in range(16):
            for stage in ("pis4", "level"):
                v = ms(f"dis_{stage}_L{lvl}")
                if v is not None:
                    res[stage][f"L{lvl}"] = round(v, 4)
        for k in ("prep", "final"):
            res[k] = round(res[k], 4) if res[k] is not None else None
        res["pis4_total"] = round(sum(res["pis4"].values()), 4)
        res["level_total"] = round(sum(res["level"].values()), 4)
        return res

    def last_kernel_ms(self, kind: str) -> float:
        out = C.c_float()
        self._call("last_kernel_ms", kind.encode(), C.byref(out), stream=False)
        return float(out.value)

    def kernel_ms_stats(self, kind: str):
        """(total ms, launches) of all calls of `kind` since set_timing(True)."""
        total, launches = C.c_double(), C.c_int()
        self._call("kernel_ms_stats", kind.encode(), C.byref(total), C.byref(launches), stream=False)
        return float(total.value), int(launches.value)

    # ------------------------------------------------------------------ helpers
    def _as_device_frames(self, frames):
        torch = self.torch
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32))
        if frames.dtype != torch.float32:
            frames = frames.to(torch.float32)
        if frames.device != self.device:
            frames = frames.to(self.device, non_blocking=True)
        return frames.contiguous()

    def _frames3(self, who, frames):
        """The frame intake of the passes that move or convert their input: frames [N,H,W,3] (device or host, any float
        type) -> (contiguous f32 device tensor, n, h, w); anything but three channels is refused."""
        src = self._as_device_frames(frames)
        n, h, w, ch = src.shape
        if ch != 3:
            raise VstabError(f"{who} expects 3-channel frames, got {ch}")
        return src, n, h, w

    def _tensor(self, who, name, t, dtype, *, shape=None, optional=False, exc=ValueError, text=None):
        """The strict check of the passes that refuse what they are not handed ready: `t` is a contiguous `dtype` tensor on
        this device (and of `shape`, where given), or None where optional.  exc: the class this caller raises; text: the
        caller's own refusal where it is not the common one."""
        if t is None and optional:
            return
        torch = self.torch
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device and t.is_contiguous()):
            raise exc(text or f"{who}: {name} must be a contiguous {str(dtype).replace('torch.', '')} tensor on {self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise exc(text or f"{who}: {name} of shape {tuple(t.shape)} is not {tuple(shape)}")

    def _new(self, shape, dtype, want=True):
        """A fresh device tensor for the library to write, or None (a NULL pointer: the output is not wanted)."""
        return self.torch.empty(tuple(shape), dtype=dtype, device=self.device) if want else None

    # ------------------------------------------------------------------ node-boundary transfers
    def upload(self, host_tensor):
        """CPU tensor (pageable) -> new device tensor through the library's pinned ring.  float32 tensors take
        vstab_upload_f32_coded: chunks that hold nothing but float32(k) / 255 -- a ComfyUI IMAGE decoded from 8-bit video --
        cross PCIe as bytes and are expanded on the device to the same bits (VSTAB_XFER_CODED=0: always as float32).
        `last_upload_coded` = (chunks that crossed as bytes, chunks) of the most recent call."""
        torch = self.torch
        src = host_tensor.contiguous()
        dst = self._new(src.shape, src.dtype)
        host = C.c_void_p(src.data_ptr())   # (a torch tensor in host memory: `src` holds it for the call)
        if src.dtype == torch.float32 and _coded_transfers():
            coded = C.c_size_t(0)
            self._call("upload_f32_coded", host, dst, src.numel(), C.byref(coded))
            self.last_upload_coded = (int(coded.value), -(-src.numel() // (32 << 20)))
        else:
            self._call("upload", host, dst, src.numel() * src.element_size())
            self.last_upload_coded = (0, -(-src.numel() // (32 << 20)))
        return dst

    def upload_u8_as_f32(self, host_tensor):
        """uint8 CPU tensor -> new float32 device tensor holding float32(k) / 255 (stabilizer_utils.py:122-126): the bytes cross
        PCIe, the division runs on the device (vstab_upload_u8_as_f32)."""
        torch = self.torch
        src = host_tensor.contiguous()
        if src.dtype != torch.uint8 or src.device.type != "cpu":
            raise VstabError("upload_u8_as_f32: a uint8 CPU tensor is required")
        dst = self._new(src.shape, torch.float32)
        self._call("upload_u8_as_f32", C.c_void_p(src.data_ptr()), dst, src.numel())
        return dst

    def download(self, device_tensor, mask=False, levels=1):
        """Device tensor -> new CPU tensor (pageable, as the reference returns) through the pinned ring (vstab_download).
        mask=True (a float32 padding mask): vstab_download_mask_levels -- a mask of zeros and ones (levels = 1), or the motion-blur
        warp's 1 - c / S (levels = S samples), crosses as bytes and is expanded by the host threads; a mask with any other value
        takes the plain path.  `last_download_coded` tells which."""
        torch = self.torch
        src = device_tensor.contiguous()
        dst = torch.empty(src.shape, dtype=src.dtype)
        host = C.c_void_p(dst.data_ptr())   # (a torch tensor in host memory: `dst` holds it for the call)
        if mask and src.dtype == torch.float32 and _coded_transfers():
            coded = C.c_int(0)
            self._call("download_mask_levels", src, host, src.numel(), max(1, min(255, int(levels))), C.byref(coded))
            self.last_download_coded = bool(coded.value)
        else:
            self._call("download", src, host, src.numel() * src.element_size())
            self.last_download_coded = False
        return dst

    # ------------------------------------------------------------------ warp
    def _warp_out(self, n, out_size, border, want_mask, out=None, out_mask=None):
        """The output side every warp prepares alike: the sizes, the border colour and the dst / mask tensors (`out` /
        `out_mask` are taken instead of fresh ones where given).  -> ((out_h, out_w), border f32 [3], dst, mask | None)"""
        f32 = self.torch.float32
        out_w, out_h = int(out_size[0]), int(out_size[1])
        b = np.ascontiguousarray(border, dtype=np.float32).reshape(3)
        dst = out if out is not None else self._new((n, out_h, out_w, 3), f32)
        mask = out_mask if want_mask and out_mask is not None else self._new((n, out_h, out_w), f32, want_mask)
        return (out_h, out_w), b, dst, mask

    def _warp_io(self, who, frames, out_size, border, want_mask, want_count, out=None, out_mask=None, counts=None):
        """What warp_batch, warp_batch_planned and mesh_warp_batch prepare alike: the source on the device, the sizes, the border colour and the
        dst / mask / counts tensors (`out` / `out_mask` / `counts` are taken instead of fresh ones where given and fitting).
        -> (src, (n, sh, sw), (out_h, out_w), border f32 [3], dst, mask | None, counts | None)"""
        src, n, sh, sw = self._frames3(who, frames)
        out_hw, b, dst, mask = self._warp_out(n, out_size, border, want_mask, out, out_mask)
        if not (want_count and want_mask):
            counts = None
        elif counts is None or counts.shape[0] != n:
            counts = self._new((n,), self.torch.int32)
        return src, (n, sh, sw), out_hw, b, dst, mask, counts

    def warp_batch(self, frames, matrices, out_size, interp="bilinear", border=(0.0, 0.0, 0.0),
                   subpix=None, want_mask=True, want_count=False, out=None, out_mask=None):
        """frames [N,H,W,3] f32 (device or host) -> (dst [N,h,w,3], mask [N,h,w] | None, counts [N] | None)."""
        src, (n, sh, sw), (out_h, out_w), b, dst, mask, counts = self._warp_io(
            "warp_batch", frames, out_size, border, want_mask, want_count, out, out_mask)
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(n, 9)
        self._call("warp_batch", src, n, sh, sw, m, out_h, out_w, INTERP[interp], b, SUBPIX[subpix or DEFAULT_SUBPIX], dst, mask, counts)
        if counts is not None and out is None:
            counts._vstab_fetch = lambda n=n: self.last_pad_counts(n)   # valid until the next warp with counts of this context
        return dst, mask, counts

    def warp_blur_batch(self, frames, matrices64, out_size, blur, samples, interp="bilinear",
                        border=(0.0, 0.0, 0.0), subpix=None, want_mask=True, out=None, out_mask=None, clip_first=0):
        """frames = frames [clip_first, clip_first + n) of the clip whose motion matrices are `matrices64` [total,3,3]
        (total == n and clip_first == 0 for a whole clip; a shard passes the replicated table of the whole clip)."""
        src, n, sh, sw = self._frames3("warp_blur_batch", frames)
        m = np.ascontiguousarray(matrices64, dtype=np.float64).reshape(-1, 9)
        total = m.shape[0]
        if clip_first < 0 or clip_first + n > total:
            raise VstabError(f"warp_blur_batch: frames [{clip_first}, {clip_first + n}) outside a clip of {total} matrices")
        ts = np.ascontiguousarray(np.linspace(0.0, float(blur), int(samples), dtype=np.float64))
        (out_h, out_w), b, dst, mask = self._warp_out(n, out_size, border, want_mask, out, out_mask)
        self._call("warp_blur_clip_batch", src, n, sh, sw, m, total, int(clip_first), ts, int(samples), out_h, out_w, INTERP[interp], b,
                   SUBPIX[subpix or DEFAULT_SUBPIX], dst, mask)
        return dst, mask

    # ------------------------------------------------------------------ estimation
    def gray_downscale(self, frames, work_size, want_range=False):
        """frames [N,H,W,3] f32 -> gray u8 [N,work_h,work_w] (work_size=(w,h) or None for full size).
        want_range: also the per-frame maximum sample (device f32 [N], NaN-propagating) from the same pass."""
        torch = self.torch
        src, n, sh, sw = self._frames3("gray_downscale", frames)
        ww, wh = (sw, sh) if work_size is None else (int(work_size[0]), int(work_size[1]))
        gray = self._new((n, wh, ww), torch.uint8)
        if want_range:
            peaks = self._new((n,), torch.float32)
            self._call("gray_downscale_range", src, n, sh, sw, wh, ww, gray, peaks)
            # the host's copy needs no transfer: the kernel mirrors the maxima into coherent host memory and this fetch waits
            # for that kernel alone (host_math.apply_value_range uses it; valid until the next range pass of this context)
            peaks._vstab_fetch = lambda n=n: self.last_frame_peaks(n)
            return gray, peaks
        self._call("gray_downscale", src, n, sh, sw, wh, ww, gray)
        return gray

    def last_pad_counts(self, n: int) -> np.ndarray:
        """Host copy of the padded-pixel counts of the latest warp_batch / warp_batch_planned(want_count=True) over n frames."""
        out = np.empty((int(n),), np.uint32)
        self._call("last_pad_counts", int(n), out, stream=False)
        return out.astype(np.int64)

    def last_frame_peaks(self, n: int) -> np.ndarray:
        """Host copy of the per-frame maxima of the latest gray_downscale(..., want_range=True) over n frames."""
        out = np.empty((int(n),), np.float32)
        self._call("last_frame_peaks", int(n), out, stream=False)
        return out

    def frame_range(self, frames):
        """Per-frame maximum sample of frames [N,H,W,3] f32 on the device (NaN-propagating) -> device f32 [N]."""
        src = self._as_device_frames(frames)
        n, sh, sw, ch = src.shape
        peaks = self._new((n,), self.torch.float32)
        self._call("frame_range", src, n, sh, sw * ch // 3, peaks)
        return peaks

    def apply_value_range(self, frames, peaks):
        """stabilizer_utils.py:127-131 on a device clip: a NEW tensor with the frames whose maximum (peaks, device f32 [N])
        exceeds 1.5 divided by 255 in IEEE float32, the others copied."""
        torch = self.torch
        src = self._as_device_frames(frames)
        n, sh, sw, ch = src.shape
        out = torch.empty_like(src)
        peaks = peaks.to(device=self.device, dtype=torch.float32).contiguous()
        self._call("apply_value_range", src, n, sh, sw * ch // 3, peaks, out)
        return out

    def _flow_outputs(self, pairs, h, w, sample_step, want_full, want_grid):
        """-> (flow [pairs,h,w,2] | None, grid_flow [pairs,gh,gw,2] | None) for the two dense estimators to write."""
        gh, gw = (h + sample_step - 1) // sample_step, (w + sample_step - 1) // sample_step
        f32 = self.torch.float32
        return self._new((pairs, h, w, 2), f32, want_full), self._new((pairs, gh, gw, 2), f32, want_grid)

    def dis_flow_batch(self, gray, sample_step=8, want_full=False, want_grid=True, clip_start=True):
        """gray u8 [N,h,w] (device) -> (flow [N-1,h,w,2] | None, grid_flow [N-1,gh,gw,2] | None).
        clip_start=False: these frames are a later shard of a clip (see vstab_dis_set_clip_start)."""
        self._call("dis_set_clip_start", 1 if clip_start else 0, stream=False)
        if gray.device != self.device:
            gray = gray.to(self.device)
        gray = gray.contiguous()
        n, h, w = gray.shape
        pairs = n - 1
        if pairs < 1:
            raise VstabError("dis_flow_batch needs at least two frames")
        flow, grid = self._flow_outputs(pairs, h, w, sample_step, want_full, want_grid)
        self._call("dis_flow_batch", gray, n, h, w, flow, grid, int(sample_step))
        return flow, grid

    def tvl1_flow_batch(self, gray, params=None, sample_step=8, want_full=False, want_grid=True, want_iterations=False):
        """Dual TV-L1 flow of every consecutive pair: gray u8 [N,h,w] (device) -> (flow [N-1,h,w,2] | None,
        grid_flow [N-1,gh,gw,2] | None, iterations int32 [N-1,nscales,warps] | None).  params: a Tvl1Params, a dict of
        overrides of the defaults, or None (OpenCV's defaults)."""
        torch = self.torch
        if gray.device != self.device:
            gray = gray.to(self.device)
        gray = gray.contiguous()
        if gray.dtype != torch.uint8 or gray.dim() != 3:
            raise ValueError("tvl1_flow_batch expects a uint8 [N,h,w] tensor")
        n, h, w = gray.shape
        if n < 2:
            raise ValueError("tvl1_flow_batch needs at least two frames")
        if params is None:
            prm = tvl1_params()
        elif isinstance(params, Tvl1Params):
            prm = params
        else:
            prm = tvl1_params(**params)
        pairs = n - 1
        flow, grid = self._flow_outputs(pairs, h, w, sample_step, want_full, want_grid)
        iters = self._new((pairs, max(prm.nscales, 1), max(prm.warps, 1)), torch.int32, want_iterations)
        self._call("tvl1_flow_batch", gray, n, h, w, C.byref(prm), flow, grid, int(sample_step), iters)
        return flow, grid, iters

    def mask_block_grid(self, mask, n_frames, working_size, step, margin):
        """Estimation mask -> the grid samples the fit must not use (vstab_mask_block_grid; the rule is in include/vstab.h).
        mask [n_frames,H,W], [1,H,W] or [H,W] float (device or host; > 0.5 or not finite = subject), working_size = (w, h) or
        None for no downscale, margin in working pixels (0..64) -> blocked u8 [n_frames,gh,gw] on the device."""
        torch = self.torch
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32))
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if mask.dim() != 3 or mask.shape[0] not in (1, int(n_frames)):
            raise ValueError(f"mask_block_grid: mask {tuple(mask.shape)} is not [{int(n_frames)},H,W], [1,H,W] or [H,W]")
        if not 0 <= int(margin) <= 64:
            raise ValueError(f"mask_block_grid: margin {margin} outside [0, 64]")
        mask = mask.to(device=self.device, dtype=torch.float32).contiguous()
        n_masks, sh, sw = (int(v) for v in mask.shape)
        ww, wh = (sw, sh) if working_size is None else (int(working_size[0]), int(working_size[1]))
        gh, gw = (wh + step - 1) // step, (ww + step - 1) // step
        blocked = self._new((int(n_frames), gh, gw), torch.uint8)
        self._call("mask_block_grid", mask, n_masks, int(n_frames), sh, sw, wh, ww, int(step), int(margin), blocked)
        return blocked

    def pair_residual_batch(self, gray, transitions):
        """Scene cuts: the motion-compensated residual of every consecutive pair (vstab_pair_residual_batch; the rule is in
        include/vstab.h).  gray u8 [N,h,w] (device), transitions f32 [N-1,3,3] at working resolution (x_{i+1} = A_i x_i) ->
        (sum_abs int64 [N-1], inside int64 [N-1]) on the host: integers, equal to the NumPy restatement exactly."""
        torch = self.torch
        if gray.dtype != torch.uint8 or gray.dim() != 3:
            raise ValueError("pair_residual_batch expects a uint8 [N,h,w] tensor")
        gray = gray.to(self.device).contiguous()
        n, h, w = (int(v) for v in gray.shape)
        if n < 2:
            raise ValueError("pair_residual_batch needs at least two frames")
        m = np.ascontiguousarray(transitions, dtype=np.float32)
        if m.size != (n - 1) * 9:
            raise ValueError(f"pair_residual_batch: transitions {m.shape} are not [{n - 1},3,3] for {n} frames")
        sums = self._new((n - 1,), torch.int64)      # the library's u64 / u32, in torch's containers
        inside = self._new((n - 1,), torch.int32)
        self._call("pair_residual_batch", gray, n, h, w, m, sums, inside)
        return sums.cpu().numpy(), inside.cpu().numpy().astype(np.int64)

    def anchor_sums_batch(self, gray, anchor, R, cap):
        """Drift correction: the normal equations of aligning every frame to its anchor (vstab_anchor_sums_batch; the rule is
        in include/vstab.h).  gray u8 [N,h,w] (device), anchor int [N] (-1: no anchor), R f64 [N,6] or [N,2,3] (anchor pixel ->
        frame pixel, working resolution), cap 0..255 -> int64 [N,17] on the host: integers, equal to the NumPy restatement
        exactly."""
        return self._anchor_sums(False, gray, anchor, R, cap)

    def anchor_sums_ex_batch(self, gray, anchor, R, cap, gain=None, offset=None, blocked=None, step=8):
        """Drift correction, exposure-matched and masked (vstab_anchor_sums_ex_batch; the rule is in include/vstab.h).  gray,
        anchor, R, cap as anchor_sums_batch; gain, offset int [N] in units of 1/1024 (None: 1024 / 0 for every frame), blocked
        u8 [N,gh,gw] on the device (mask_block_grid at `step`) or None -> int64 [N,31] on the host: integers, equal to the
        NumPy restatement exactly."""
        return self._anchor_sums(True, gray, anchor, R, cap, gain, offset, blocked, step)

    def _anchor_sums(self, ex, gray, anchor, R, cap, gain=None, offset=None, blocked=None, step=8):
        """Both forms of the rule: the checks they share, then the second form's own (ex), then the call."""
        torch = self.torch
        who = "anchor_sums_ex_batch" if ex else "anchor_sums_batch"
        if gray.dtype != torch.uint8 or gray.dim() != 3:
            raise ValueError(f"{who} expects a uint8 [N,h,w] tensor")
        if gray.device != self.device or not gray.is_contiguous():   # (a contiguous view keeps its own, possibly unaligned, base)
            gray = gray.to(self.device).contiguous()
        n, h, w = (int(v) for v in gray.shape)
        if n < 1:
            raise ValueError(f"{who} needs at least one frame")
        a = np.ascontiguousarray(anchor, dtype=np.int32).reshape(-1)
        m = np.ascontiguousarray(R, dtype=np.float64)
        if a.size != n or m.size != n * 6:
            raise ValueError(f"{who}: anchor {a.shape} / R {m.shape} are not [{n}] / [{n},6] for {n} frames")
        if a.size and (a.min() < -1 or a.max() >= n):
            raise ValueError(f"{who}: an anchor outside -1..{n - 1}")
        if max(h, w) > 1024:
            raise ValueError(f"{who}: {w}x{h} image larger than 1024 on a side")
        if int(cap) != cap or not 0 <= int(cap) <= 255:      # (an integral float passes: not _int_in's set)
            raise ValueError(f"{who}: cap {cap!r} is not an integer in 0..255")
        args = (int(cap),)
        if ex:
            g = np.full(n, 1024, np.int32) if gain is None else np.ascontiguousarray(gain, dtype=np.int64).reshape(-1)
            o = np.zeros(n, np.int32) if offset is None else np.ascontiguousarray(offset, dtype=np.int64).reshape(-1)
            if g.size != n or o.size != n:
                raise ValueError(f"{who}: gain {g.shape} / offset {o.shape} are not [{n}] for {n} frames")
            if g.min() < 256 or g.max() > 4096:
                raise ValueError(f"{who}: a gain outside 256..4096")
            if np.abs(o).max() > 1 << 20:
                raise ValueError(f"{who}: an offset outside -2^20..2^20")
            g, o = g.astype(np.int32), o.astype(np.int32)
            if int(step) != step or int(step) < 1:           # (as cap)
                raise ValueError(f"{who}: step {step!r} is not a positive integer")
            step = int(step)
            gh, gw = (h + step - 1) // step, (w + step - 1) // step
            if blocked is not None:
                if blocked.dtype != torch.uint8 or tuple(blocked.shape) != (n, gh, gw):
                    raise ValueError(f"{who}: blocked {tuple(blocked.shape)} {blocked.dtype} is not uint8 [{n},{gh},{gw}]")
                blocked = blocked.to(self.device).contiguous()
            args = (g, o, int(cap), blocked, step, gh, gw)
        out = self._new((n, 31 if ex else 17), torch.int64)
        self._call(who, gray, n, h, w, a, m, *args, out)
        return out.cpu().numpy()

    # ------------------------------------------------------------------ mesh warp
    @staticmethod
    def _check_mesh(who, mw, mh):
        if not (2 <= int(mw) <= MESH_MAX_VERTS and 2 <= int(mh) <= MESH_MAX_VERTS):
            raise ValueError(f"{who}: {mw}x{mh} vertices outside 2..{MESH_MAX_VERTS} per axis")
        return int(mw), int(mh)

    def mesh_residual_batch(self, grid_flow, step, work_size, transitions, mw, mh, blocked=None):
        """Per-vertex residual of the global fit (vstab_mesh_residual_batch; the rule is in include/vstab.h).
        grid_flow f32 [P,gh,gw,2] (device), work_size = (w, h) of the estimation images, transitions f32 [P,3,3] at working
        resolution, mw x mh vertices, blocked u8 [P+1,gh,gw] or None -> (residual f32 [P,mh,mw,2], count i32 [P,mh,mw]),
        device tensors."""
        torch = self.torch
        mw, mh = self._check_mesh("mesh_residual_batch", mw, mh)
        grid_flow, blocked, pairs, gh, gw, step, wh, ww, m = self._residual_inputs(
            "mesh_residual_batch", grid_flow, step, work_size, transitions, blocked)
        residual = self._new((pairs, mh, mw, 2), torch.float32)
        count = self._new((pairs, mh, mw), torch.int32)
        self._call("mesh_residual_batch", grid_flow, pairs, gh, gw, step, wh, ww, m, blocked, mw, mh, residual, count)
        return residual, count

    def _grid_inputs(self, who, grid_flow, step, work_size, blocked):
        """What the passes over a flow grid check alike: the grid flow, `blocked`, the grid against the working size at `step`.
        -> (grid_flow, blocked, pairs, gh, gw, step, work_h, work_w)"""
        if grid_flow.dtype != self.torch.float32 or grid_flow.dim() != 4 or grid_flow.shape[3] != 2:
            raise ValueError(f"{who} expects a float32 [P,gh,gw,2] tensor")
        grid_flow, blocked, pairs, gh, gw = self._fit_inputs(grid_flow, blocked)
        ww, wh, step = int(work_size[0]), int(work_size[1]), int(step)
        if step < 1 or (gh, gw) != ((wh + step - 1) // step, (ww + step - 1) // step):
            raise ValueError(f"{who}: a grid of {gw}x{gh} samples is not a {ww}x{wh} image at step {step}")
        return grid_flow, blocked, pairs, gh, gw, step, wh, ww

    def _residual_inputs(self, who, grid_flow, step, work_size, transitions, blocked):
        """What mesh_residual_batch and row_residual_batch check alike: the grid flow, its grid against the working size at
        `step`, the transitions.  -> (grid_flow, blocked, pairs, gh, gw, step, work_h, work_w, transitions f32)"""
        grid_flow, blocked, pairs, gh, gw, step, wh, ww = self._grid_inputs(who, grid_flow, step, work_size, blocked)
        m = np.ascontiguousarray(transitions, dtype=np.float32)
        if m.size != pairs * 9:
            raise ValueError(f"{who}: transitions {m.shape} are not [{pairs},3,3]")
        return grid_flow, blocked, pairs, gh, gw, step, wh, ww, m

    def _mesh_offsets(self, who, offsets, n):
        """offsets f32 [n,mh,mw,2] (host or device) -> (contiguous device tensor, mw, mh)."""
        torch = self.torch
        if not isinstance(offsets, torch.Tensor):
            offsets = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.float32))
        if offsets.dim() != 4 or offsets.shape[0] != n or offsets.shape[3] != 2 or offsets.dtype != torch.float32:
            raise ValueError(f"{who}: offsets {tuple(offsets.shape)} {offsets.dtype} are not float32 [{n},mh,mw,2]")
        mw, mh = self._check_mesh(who, offsets.shape[2], offsets.shape[1])
        return offsets.to(self.device).contiguous(), mw, mh

    def mesh_warp_batch(self, frames, matrices, out_size, offsets, border=(0.0, 0.0, 0.0), subpix=None, want_mask=True,
                        want_count=False):
        """warp_batch (bilinear) with a per-vertex displacement of the source frame (vstab_mesh_warp_batch; the rule is in
        include/vstab.h).  offsets f32 [N,mh,mw,2] in full-resolution px (host or device) ->
        (dst [N,h,w,3], mask [N,h,w] | None, counts [N] | None).  All-zero offsets give warp_batch's bits."""
        return self._displaced_warp("mesh_warp_batch", frames, matrices, out_size, border, subpix, want_mask, want_count,
                                    lambda n: self._mesh_offsets("mesh_warp_batch", offsets, n))

    def _displaced_warp(self, name, frames, matrices, out_size, border, subpix, want_mask, want_count, own, want_second=()):
        """The wrapper of the displaced warps (vstab_<name>: the mesh and rolling-shutter forms and their inverses).  own(n) ->
        the entry point's own arguments, between subpix and dst (a tensor goes as its device pointer, an array as its host
        pointer); want_second: () for a forward form, (flag,) for an inverse, whose second counter i32 [N] | None is appended
        to (dst, mask, counts)."""
        src, (n, sh, sw), (out_h, out_w), b, dst, mask, counts = self._warp_io(name, frames, out_size, border, want_mask, want_count)
        own = own(n)
        second = tuple(self._new((n,), self.torch.int32, want) for want in want_second)
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(n, 9)
        self._call(name, src, n, sh, sw, m, out_h, out_w, b, SUBPIX[subpix or DEFAULT_SUBPIX], *own, dst, mask, counts, *second)
        return (dst, mask, counts) + second

    def mesh_unwarp_batch(self, frames, matrices, out_size, offsets, border=(0.0, 0.0, 0.0), subpix=None, want_mask=True,
                          want_count=False, want_unconverged=False):
        """The inverse of mesh_warp_batch's displacement (vstab_mesh_unwarp_batch; the rule is in include/vstab.h): warp_batch
        (bilinear) whose output pixel is moved by the inverse of the mesh displacement in front of the matrix.  offsets f32
        [N,mh,mw,2] in px of the OUTPUT canvas (host or device) -> (dst [N,h,w,3], mask [N,h,w] | None, counts [N] | None,
        unconverged [N] i32 | None: pixels per frame whose fixed point hit the step limit).  All-zero offsets give
        warp_batch's bits."""
        return self._displaced_warp("mesh_unwarp_batch", frames, matrices, out_size, border, subpix, want_mask, want_count,
                                    lambda n: self._mesh_offsets("mesh_unwarp_batch", offsets, n), (want_unconverged,))

    # ------------------------------------------------------------------ rolling shutter
    def rolling_warp_batch(self, frames, matrices, out_size, velocity, readout, border=(0.0, 0.0, 0.0), subpix=None,
                           want_mask=True, want_count=True):
        """warp_batch (bilinear) that samples every source row where a sensor read out over `readout` of the frame interval
        showed it (vstab_rolling_warp_batch; the rule is in include/vstab.h).  velocity f64 [N,6] (host), full-resolution px per
        frame interval; readout in [-1, 1] -> (dst [N,h,w,3], mask [N,h,w] | None, counts [N] | None).  All-zero velocity or
        readout == 0 give warp_batch's bits."""
        return self._displaced_warp("rolling_warp_batch", frames, matrices, out_size, border, subpix, want_mask, want_count,
                                    lambda n: self._rolling_inputs("rolling_warp_batch", velocity, readout, n))

    @staticmethod
    def _rolling_inputs(who, velocity, readout, n, null_ok=False):
        """velocity -> contiguous f64 of n * 6 values (None with null_ok: None, a NULL pointer for the library to refuse),
        readout -> float in [-1, 1]."""
        v = None if (velocity is None and null_ok) else np.ascontiguousarray(velocity, dtype=np.float64)
        if v is not None and v.size != n * 6:
            raise ValueError(f"{who}: velocity {v.shape} is not [{n},6]")
        readout = float(readout)
        if not -1.0 <= readout <= 1.0:       # (a NaN fails it too)
            raise ValueError(f"{who}: readout={readout!r} outside [-1, 1]")
        return v, readout

    def rolling_unwarp_batch(self, frames, matrices, out_size, velocity, readout, border=(0.0, 0.0, 0.0), subpix=None,
                             want_mask=True, want_count=False, want_unsolved=False):
        """The inverse of rolling_warp_batch's displacement (vstab_rolling_unwarp_batch; the rule is in include/vstab.h):
        warp_batch (bilinear) whose output pixel is moved by the closed-form inverse of the row displacement in front of the
        matrix.  velocity f64 [N,6] (host) and readout as rolling_warp_batch's; the row lever is the OUTPUT canvas's height ->
        (dst [N,h,w,3], mask [N,h,w] | None, counts [N] | None, unsolved [N] i32 | None: pixels per frame whose solve was
        refused and that were warped by the matrix alone).  All-zero velocity or readout == 0 give warp_batch's bits."""
        return self._displaced_warp(
            "rolling_unwarp_batch", frames, matrices, out_size, border, subpix, want_mask, want_count,
            lambda n: self._rolling_inputs("rolling_unwarp_batch", velocity, readout, n, null_ok=True), (want_unsolved,))

    def row_residual_batch(self, grid_flow, step, work_size, transitions, blocked=None):
        """Per-row median of the global fit's residual (vstab_row_residual_batch; the rule is in include/vstab.h).
        grid_flow f32 [P,gh,gw,2] (device), work_size = (w, h) of the estimation images, transitions f32 [P,3,3] at working
        resolution, blocked u8 [P+1,gh,gw] or None -> (residual f32 [P,gh,2], count i32 [P,gh]), device tensors."""
        torch = self.torch
        grid_flow, blocked, pairs, gh, gw, step, wh, ww, m = self._residual_inputs(
            "row_residual_batch", grid_flow, step, work_size, transitions, blocked)
        residual = self._new((pairs, gh, 2), torch.float32)
        count = self._new((pairs, gh), torch.int32)
        self._call("row_residual_batch", grid_flow, pairs, gh, gw, step, wh, ww, m, blocked, residual, count)
        return residual, count

    def rectify_samples_batch(self, grid_flow, step, work_size, velocity, readout, blocked=None):
        """The flow grid's samples as point pairs corrected for the readout (vstab_rectify_samples_batch; the rule is in
        include/vstab.h).  grid_flow f32 [P,gh,gw,2] (device), work_size = (w, h) of the estimation images, velocity f64 [P+1,6]
        (host) in working px per frame interval, readout in [-1, 1], blocked u8 [P+1,gh,gw] or None ->
        (point_pairs f32 [P,gh*gw,4]: the admitted samples in grid order, NaN rows behind them; counts i32 [P]; unsolved i32 [P]),
        device tensors: what points_fit_batch takes."""
        torch = self.torch
        who = "rectify_samples_batch"
        grid_flow, blocked, pairs, gh, gw, step, wh, ww = self._grid_inputs(who, grid_flow, step, work_size, blocked)
        v, readout = self._rolling_inputs(who, velocity, readout, pairs + 1, null_ok=True)
        point_pairs = self._new((pairs, gh * gw, 4), torch.float32)
        counts = self._new((pairs,), torch.int32)
        unsolved = self._new((pairs,), torch.int32)
        self._call(who, grid_flow, pairs, gh, gw, step, wh, v, readout, blocked, point_pairs, counts, unsolved)
        return point_pairs, counts, unsolved

    def cover_extent_batch(self, matrices, src_size, out_size, offsets=None, subpix=None):
        """How far the warp's own coverage reaches around the canvas centre (vstab_cover_extent_batch; the rule is in
        include/vstab.h): matrices f32 [N,3,3] forward, src_size / out_size (w, h), offsets f32 [N,mh,mw,2] (host or device) for
        the mesh warp's coverage or None for the plain warp's -> uint32 [N] on the host: per frame the minimum of
        e = max(|2x-(w-1)|*(h-1), |2y-(h-1)|*(w-1)) over the pixels the warp would leave uncovered, 0xFFFFFFFF if there is none."""
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 9)
        n = m.shape[0]
        sw, sh = int(src_size[0]), int(src_size[1])
        ow, oh = int(out_size[0]), int(out_size[1])
        mw = mh = 0
        if offsets is not None:
            offsets, mw, mh = self._mesh_offsets("cover_extent_batch", offsets, n)
        extent = self._new((max(n, 1),), self.torch.int32)
        self._call("cover_extent_batch", m, n, sh, sw, oh, ow, SUBPIX[subpix or DEFAULT_SUBPIX], offsets, mw, mh, extent)
        return extent[:n].cpu().numpy().view(np.uint32)

    def _fit_inputs(self, grid_flow, blocked):
        if grid_flow.device != self.device:
            grid_flow = grid_flow.to(self.device)
        grid_flow = grid_flow.contiguous()
        pairs, gh, gw, _ = grid_flow.shape
        if blocked is not None:
            if blocked.dtype != self.torch.uint8 or tuple(blocked.shape) != (pairs + 1, gh, gw):
                raise ValueError(f"sample_fit_batch: blocked {tuple(blocked.shape)} {blocked.dtype} is not uint8 "
                                 f"[{pairs + 1},{gh},{gw}] (one row per frame of the {pairs} pairs)")
            blocked = blocked.to(self.device).contiguous()
        return grid_flow, blocked, pairs, gh, gw

    def sample_fit_batch(self, grid_flow, step, requested_mode, blocked=None):
        """grid_flow [P,gh,gw,2] (device) -> structured table [P,3] (FIT_DTYPE), one row per pair and mode.
        blocked (u8 [P+1,gh,gw], mask_block_grid): the fit uses the samples blocked in neither frame of a pair."""
        grid_flow, blocked, pairs, gh, gw = self._fit_inputs(grid_flow, blocked)
        table = np.zeros((pairs, 3), FIT_DTYPE)
        masked = () if blocked is None else (blocked,)      # the masked entry point takes it in front of the table
        self._call("sample_fit_batch_masked" if masked else "sample_fit_batch", grid_flow, pairs, gh, gw, int(step),
                   MODES[requested_mode], *masked, table)
        return table

    def sample_fit_batch_begin(self, grid_flow, step, requested_mode, blocked=None):
        """Launch the fits of sample_fit_batch without waiting: the records stay on the device (fit_records_device) and
        their download is queued; sample_fit_batch_end(pairs) collects the host table.  Work queued in between (the
        device plan, the warp) does not delay that download."""
        grid_flow, blocked, pairs, gh, gw = self._fit_inputs(grid_flow, blocked)
        masked = () if blocked is None else (blocked,)
        self._call("sample_fit_batch_begin_masked" if masked else "sample_fit_batch_begin", grid_flow, pairs, gh, gw, int(step),
                   MODES[requested_mode], *masked)
        self._fit_grid = (grid_flow, blocked)   # keep the inputs alive until the kernels have run
        return pairs

    def fit_records_device(self) -> int:
        """Device address of the records of the last sample_fit_batch_begin ([pairs*3] vstab_fit_record)."""
        ptr = self._call("fit_records_device", stream=False, check=False)
        if not ptr:
            raise VstabError("fit_records_device: no fit is pending")
        return int(ptr)

    def sample_fit_batch_end(self, pairs):
        table = np.zeros((pairs, 3), FIT_DTYPE)
        self._call("sample_fit_batch_end", int(pairs), table, stream=False)
        self._fit_grid = None
        return table

    # ------------------------------------------------------------------ speculative device plan (F6-F12, crop_and_pad)
    def fit_records_copy(self, dst, pairs):
        """The pending fit's device records into `dst` (device uint8 tensor of >= pairs * 3 records), stream-ordered."""
        self._call("fit_records_copy", dst, int(pairs))

    def flow_plan_device(self, records_ptr, pairs, requested_mode, source_size, working_size, smooth, fps, strength, camera_lock,
                         seg_pairs=None, seg_rows=0, warp_frames=0, framing="crop_and_pad"):
        """Queue plan_kernel behind the fits: records (device address) -> the warp's transform table, on the device.
        seg_pairs / seg_rows: the records are an all-gather's receive buffer (seg_rows pairs per rank, seg_pairs[r] valid).
        warp_frames: frames the following warp_batch_planned(want_count=True) will warp -- its count array is allocated here
        and zeroed by the plan kernel, so that no fill launch sits between plan and warp.
        framing: "crop_and_pad" (matrices recentred on the frames' common region) or "expand" (shifted so that the frames'
        union starts at the origin; the canvas size comes from flow_plan_result's region: expand_canvas())."""
        if framing not in ("crop_and_pad", "expand"):
            raise VstabError(f"flow_plan_device: framing {framing!r} is not formed on the device")
        self._planned_counts = None
        up = down = None
        if working_size is not None:
            sx, sy = working_size[0] / float(source_size[0]), working_size[1] / float(source_size[1])
            up = np.array([1.0 / sx, 1.0 / sy, 1.0], np.float64)
            down = np.array([sx, sy, 1.0], np.float64)
        seg = np.ascontiguousarray(seg_pairs, np.int32) if seg_pairs is not None else None
        if warp_frames:
            # registered right in front of the plan call, with every argument already built: the library hands the pointer to
            # THAT call's kernel only (and drops it if the call is refused), so no stale registration can outlive the tensor
            counts = self._new((int(warp_frames),), self.torch.int32)
            self._call("flow_plan_zero_counts", counts, int(warp_frames))
            self._planned_counts = counts
        self._call("flow_plan_device", C.c_void_p(int(records_ptr)), int(pairs), MODES[requested_mode], up, down,
                   float(smooth), float(fps), float(strength), 1 if camera_lock else 0, int(source_size[0]), int(source_size[1]),
                   0 if seg is None else len(seg), seg, int(seg_rows), 1 if framing == "expand" else 0,
                   stream=not warp_frames)      # (the registration has just set the stream)

    @staticmethod
    def expand_canvas(region):
        """(width, height) of the expand canvas from the device plan's region x_min, y_min, x_max, y_max -- the arithmetic of
        _prepare_expand_transform (stabilizer_utils.py:386-406); None if the region is not finite."""
        import math

        x0, y0, x1, y1 = (float(v) for v in region)
        if not all(math.isfinite(v) for v in (x0, y0, x1, y1)):
            return None
        return max(int(math.ceil(x1 - x0)), 1), max(int(math.ceil(y1 - y0)), 1)

    def flow_plan_result(self, frames, params):
        """(final float32 matrices [frames,3,3], path, target [frames,params], region [4]) of the pending device plan."""
        final = np.zeros((frames, 3, 3), np.float32)
        path = np.zeros((frames, params), np.float64)
        target = np.zeros((frames, params), np.float64)
        region = np.zeros(4, np.float64)
        self._call("flow_plan_result", int(frames), final, path, target, region, stream=False)
        return final, path, target, region

    def warp_batch_planned(self, frames, first, out_size, border=(0.0, 0.0, 0.0), subpix=None, want_mask=True, want_count=False):
        """warp_batch (bilinear) for frames [first, first + n) of the clip whose plan is pending on the device."""
        handed = None
        if want_count and want_mask:
            handed = getattr(self, "_planned_counts", None)      # zeroed by the plan kernel, if the plan call was told of this warp
            self._planned_counts = None
        src, (n, sh, sw), (out_h, out_w), b, dst, mask, counts = self._warp_io(
            "warp_batch_planned", frames, out_size, border, want_mask, want_count, counts=handed)
        self._call("warp_batch_planned", src, int(first), n, sh, sw, out_h, out_w, INTERP["bilinear"], b,
                   SUBPIX[subpix or DEFAULT_SUBPIX], dst, mask, counts)
        if counts is not None:
            counts._vstab_fetch = lambda n=n: self.last_pad_counts(n)   # valid until the next warp with counts of this context
        return dst, mask, counts

    # ------------------------------------------------------------------ temporal fill
    def temporal_fill_batch(self, clip_frames, matrices, cand_frame, dst, mask, first=0, interp="bilinear", subpix=None,
                            want_filled_from=False, want_counts=True):
        """Fills the padded pixels (mask == 1) of output frames [first, first + n) from neighbouring source frames, in place.
        clip_frames [N,H,W,3] f32 device (the whole clip), matrices [n,K,3,3] f32 forward (candidate source -> output canvas),
        cand_frame [n,K] i32 (-1: none), dst [n,h,w,3] / mask [n,h,w] f32 device and contiguous (see include/vstab.h for the
        rule).  -> (filled_from i8 [n,h,w] | None, fill_count i32 [n] | None, pad_count i32 [n] | None), device tensors."""
        torch = self.torch
        if mask is None:
            raise VstabError(f"temporal_fill_batch: mask must be a contiguous float32 tensor on {self.device}")
        src, (total, sh, sw), (n, out_h, out_w, k), m, cf, _ = self._neighbour_io(
            "temporal_fill_batch", clip_frames, matrices, cand_frame, None, dst, mask, subpix, accepts_exact=True)
        filled_from = self._new((n, out_h, out_w), torch.int8, want_filled_from)
        fill_count = self._new((n,), torch.int32, want_counts)
        pad_count = self._new((n,), torch.int32, want_counts)
        self._call("temporal_fill_batch", src, total, sh, sw, int(first), n, m, cf, k, out_h, out_w, INTERP[interp],
                   SUBPIX[subpix or DEFAULT_SUBPIX], dst, mask, filled_from, fill_count, pad_count)
        return filled_from, fill_count, pad_count

    def _neighbour_io(self, who, clip_frames, matrices, cand_frame, own_matrices, dst, mask, subpix, accepts_exact=False):
        """The arguments the temporal fill, the two blended-fill entries and the sharpness transfer share (csrc/vstab_neighbour.hip),
        checked in one place.  own_matrices None: the entry takes none; mask None: the entry's own affair; accepts_exact: the
        entry (the plain fill) has the 'exact' sub-pixel mode besides 'q5'."""
        torch = self.torch
        src, total, sh, sw = self._frames3(who, clip_frames)
        if not accepts_exact and (subpix or DEFAULT_SUBPIX) != "q5":
            raise VstabError(f"{who}: sub-pixel mode {(subpix or DEFAULT_SUBPIX)!r} is not supported; the entry is 'q5' only")
        self._tensor(who, "dst", dst, torch.float32, exc=VstabError)
        self._tensor(who, "mask", mask, torch.float32, optional=True, exc=VstabError)
        if dst.dim() != 4 or dst.shape[3] != 3 or (mask is not None and mask.numel() * 3 != dst.numel()):
            raise VstabError(f"{who}: dst {tuple(dst.shape)} / mask {tuple(mask.shape) if mask is not None else None} do not match")
        n, out_h, out_w = int(dst.shape[0]), int(dst.shape[1]), int(dst.shape[2])
        cf = np.ascontiguousarray(cand_frame, dtype=np.int32)
        if cf.ndim != 2 or cf.shape[0] != n:
            raise VstabError(f"{who}: cand_frame {cf.shape} is not [n={n}, K]")
        k = int(cf.shape[1])
        m = np.ascontiguousarray(matrices, dtype=np.float32)
        if m.size != n * k * 9:
            raise VstabError(f"{who}: matrices {m.shape} are not [n={n}, K={k}, 3, 3]")
        own = None
        if own_matrices is not None:
            own = np.ascontiguousarray(own_matrices, dtype=np.float32)
            if own.size != n * 9:
                raise VstabError(f"{who}: own_matrices {own.shape} are not [n={n}, 3, 3]")
        return src, (total, sh, sw), (n, out_h, out_w, k), m, cf, own

    def fill_gain_sums(self, clip_frames, matrices, cand_frame, own_matrices, dst, first=0, interp="bilinear", subpix=None):
        """The integer sums behind the blended fill's exposure gains (include/vstab.h: vstab_fill_gain_sums), for output frames
        [first, first + n): clip_frames / matrices / cand_frame as temporal_fill_batch takes them, own_matrices [n,3,3] f32 (the
        frames' own forward matrices), dst [n,h,w,3] f32 device as the warp left it (read only).
        -> sums i64 [n,K,7] device tensor: count, own r g b, candidate r g b (see temporal_fill.gains_from_sums)."""
        src, (total, sh, sw), (n, out_h, out_w, k), m, cf, own = self._neighbour_io(
            "fill_gain_sums", clip_frames, matrices, cand_frame, own_matrices, dst, None, subpix)
        sums = self._new((n, k, 7), self.torch.int64)
        self._call("fill_gain_sums", src, total, sh, sw, int(first), n, m, cf, k, own, out_h, out_w, INTERP[interp], SUBPIX["q5"],
                   dst, sums)
        return sums

    def temporal_fill_blend_batch(self, clip_frames, matrices, cand_frame, own_matrices, gains, dst, mask, feather_px=0, first=0,
                                  interp="bilinear", subpix=None, want_filled_from=False, want_counts=True):
        """temporal_fill_batch with a gain per (frame, candidate, channel) on what a candidate supplies and a feather of
        feather_px (0..64) source pixels in which the frame's own border pixels fade into the first valid candidate, in
        place (include/vstab.h: vstab_temporal_fill_blend_batch).  own_matrices [n,3,3] f32, gains [n,K,3] f32; the rest as
        temporal_fill_batch.  'q5' only.
        -> (filled_from i8 [n,h,w] | None, fill_count, pad_count, blend_count i32 [n] | None), device tensors."""
        torch = self.torch
        src, (total, sh, sw), (n, out_h, out_w, k), m, cf, own = self._neighbour_io(
            "temporal_fill_blend_batch", clip_frames, matrices, cand_frame, own_matrices, dst, mask, subpix)
        if mask is None:     # (a text of its own, without the device: not _tensor's)
            raise VstabError("temporal_fill_blend_batch: mask must be a contiguous float32 tensor")
        g = np.ascontiguousarray(gains, dtype=np.float32)
        if g.size != n * k * 3:
            raise VstabError(f"temporal_fill_blend_batch: gains {g.shape} are not [n={n}, K={k}, 3]")
        feather_px = int(feather_px)
        filled_from = self._new((n, out_h, out_w), torch.int8, want_filled_from)
        counts = [self._new((n,), torch.int32, want_counts) for _ in range(3)]
        self._call("temporal_fill_blend_batch", src, total, sh, sw, int(first), n, m, cf, k, own, g, feather_px, out_h, out_w,
                   INTERP[interp], SUBPIX["q5"], dst, mask, filled_from, *counts)
        return filled_from, counts[0], counts[1], counts[2]

    # ------------------------------------------------------------------ spatial fill
    def spatial_fill_batch(self, dst, mask, chunk_frames=0, want_counts=True):
        """Fills the hole pixels (!(mask <= 0.5)) of dst [n,h,w,3] from the frame's own valid pixels by pyramid push-pull, in
        place; mask [n,h,w] (or [n,h,w,1]) is read only.  Both f32, device, contiguous (see include/vstab.h for the rule).
        chunk_frames: frames per pass over the workspace, 0 = automatic; the result does not depend on it.
        -> (hole_count i32 [n] | None, fill_count i32 [n] | None), device tensors."""
        torch = self.torch
        self._tensor("spatial_fill_batch", "dst", dst, torch.float32, exc=VstabError)
        self._tensor("spatial_fill_batch", "mask", mask, torch.float32, exc=VstabError)
        if dst.dim() != 4 or dst.shape[3] != 3 or mask.dim() not in (3, 4) or mask.numel() * 3 != dst.numel() \
                or tuple(mask.shape[:3]) != tuple(dst.shape[:3]):
            raise VstabError(f"spatial_fill_batch: dst {tuple(dst.shape)} / mask {tuple(mask.shape)} do not match")
        chunk_frames = int(chunk_frames)
        if chunk_frames < 0:
            raise VstabError(f"spatial_fill_batch: chunk_frames={chunk_frames} is negative")
        n, h, w = int(dst.shape[0]), int(dst.shape[1]), int(dst.shape[2])
        hole_count = self._new((n,), torch.int32, want_counts)
        fill_count = self._new((n,), torch.int32, want_counts)
        if n == 0 or h == 0 or w == 0:
            return hole_count, fill_count
        self._call("spatial_fill_batch", dst, mask, n, h, w, chunk_frames, hole_count, fill_count)
        return hole_count, fill_count

    # ------------------------------------------------------------------ stability report
    def frame_sse_batch(self, a, b, mask_a=None, mask_b=None):
        """Masked squared error of frame a[k] against frame b[k] as exact integers (include/vstab.h states the rule): a, b
        [n,h,w,3], mask_a / mask_b [n,h,w] or None (every pixel valid), all f32, device, contiguous.  a and b may be views of
        one tensor (b = clip[1:], a = clip[:-1] is the consecutive-frame form); nothing is written to them.
        -> (sse i64 [n], count i32 [n]), device tensors."""
        torch = self.torch
        for name, t in (("a", a), ("b", b), ("mask_a", mask_a), ("mask_b", mask_b)):
            self._tensor("frame_sse_batch", name, t, torch.float32, optional=name.startswith("mask"))
        if a.dim() != 4 or a.shape[3] != 3:
            raise ValueError(f"frame_sse_batch: a of shape {tuple(a.shape)} is not [n,h,w,3]")
        if tuple(b.shape) != tuple(a.shape):
            raise ValueError(f"frame_sse_batch: b of shape {tuple(b.shape)} does not match a {tuple(a.shape)}")
        for name, t in (("mask_a", mask_a), ("mask_b", mask_b)):
            if t is not None and tuple(t.shape) != tuple(a.shape[:3]):
                raise ValueError(f"frame_sse_batch: {name} of shape {tuple(t.shape)} does not match the frames: expected "
                                 f"{tuple(a.shape[:3])}")
        n, h, w = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
        sse = self._new((n,), torch.int64)
        count = self._new((n,), torch.int32)
        self._call("frame_sse_batch", a, mask_a, b, mask_b, n, h, w, sse, count)
        return sse, count

    # ------------------------------------------------------------------ deflicker
    def _pair_gain_args(self, who, src, transitions, active):
        """The arguments the two measuring entries share, checked -> (n, h, w, transitions f32 [n-1,9], active u8 [n-1] | None)."""
        self._tensor(who, "src", src, self.torch.float32)
        if src.dim() != 4 or src.shape[3] != 3 or src.shape[0] < 2:
            raise ValueError(f"{who}: src of shape {tuple(src.shape)} is not [n,h,w,3] with n >= 2")
        n, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
        m = np.ascontiguousarray(transitions, dtype=np.float32)
        if m.size != (n - 1) * 9:
            raise ValueError(f"{who}: transitions {m.shape} are not [{n - 1},3,3] for {n} frames")
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active) != 0, dtype=np.uint8)
            if act.shape != (n - 1,):
                raise ValueError(f"{who}: active of shape {act.shape} is not [{n - 1}]")
        return n, h, w, m, act

    def pair_gain_hist_batch(self, src, transitions, active=None):
        """Deflicker, first pass (vstab_pair_gain_hist_batch; include/vstab.h states the rule): the histograms of the registered
        level ratios of every consecutive pair.  src f32 [n,h,w,3] (device, contiguous, read only), transitions f32 [n-1,3,3] at
        full resolution (x_{k+1} = A_k x_k), active [n-1] or None (a pair with 0 reads nothing and reports zeros)
        -> (hist i32 [n-1,4,1024], stats i32 [n-1,2] = inside, well_exposed), device tensors."""
        n, h, w, m, act = self._pair_gain_args("pair_gain_hist_batch", src, transitions, active)
        hist = self._new((n - 1, 4, 1024), self.torch.int32)      # the library's u32, in torch's container
        stats = self._new((n - 1, 2), self.torch.int32)
        self._call("pair_gain_hist_batch", src, n, h, w, m, act, hist, stats)
        return hist, stats

    def pair_gain_sums_batch(self, src, transitions, band, active=None):
        """Deflicker, second pass (vstab_pair_gain_sums_batch): count and level sums of the well-exposed lattice pixels whose
        ratio bin lies in the pair's band.  src, transitions, active as above; band int [n-1,4,2], inclusive bins (lo > hi counts
        nothing) -> sums i64 [n-1,4,3] = count, sum qa, sum qb, device tensor."""
        n, h, w, m, act = self._pair_gain_args("pair_gain_sums_batch", src, transitions, active)
        b = np.ascontiguousarray(band, dtype=np.int32)
        if b.shape != (n - 1, 4, 2):
            raise ValueError(f"pair_gain_sums_batch: band of shape {b.shape} is not [{n - 1},4,2]")
        sums = self._new((n - 1, 4, 3), self.torch.int64)
        self._call("pair_gain_sums_batch", src, n, h, w, m, act, b, sums)
        return sums

    def apply_gain_batch(self, frames, gains, mask=None, want_count=True):
        """Deflicker, the correction (vstab_apply_gain_batch; include/vstab.h states the rule): frames f32 [n,h,w,3] (device,
        contiguous) are scaled IN PLACE by gains f32 [n,3], one float32 multiply per value; pixels with mask == 1.0f (mask f32
        [n,h,w] or None: every pixel is own), channels with a gain of exactly 1 and NaNs are untouched; a value that the gain
        would push above 1 is set to 1 and counted.  -> clamped i32 [n] (device) or None."""
        torch = self.torch
        self._tensor("apply_gain_batch", "frames", frames, torch.float32)
        self._tensor("apply_gain_batch", "mask", mask, torch.float32, optional=True)
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"apply_gain_batch: frames of shape {tuple(frames.shape)} are not [n,h,w,3]")
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if mask is not None and tuple(mask.shape) != (n, h, w):
            raise ValueError(f"apply_gain_batch: mask of shape {tuple(mask.shape)} does not match the frames: expected {(n, h, w)}")
        g = np.ascontiguousarray(gains, dtype=np.float32)
        if g.shape != (n, 3):
            raise ValueError(f"apply_gain_batch: gains of shape {g.shape} are not [{n},3]")
        clamped = self._new((n,), torch.int32, want_count)
        self._call("apply_gain_batch", frames, mask, n, h, w, g, clamped)
        return clamped

    # ------------------------------------------------------------------ subject lock
    def mask_moments_batch(self, mask):
        """Count, coordinate sums and bounding box of the subject pixels (mask > 0.5; a NaN is not subject, +inf is) of every
        frame of mask [n,h,w], f32, device, contiguous, as exact integers (include/vstab.h states the rule); nothing is
        written to it.  -> (sums i64 [n,3] = count, sum_x, sum_y;  bbox i32 [n,4] = x0, y0, x1, y1 inclusive, four -1 for a
        frame without a subject pixel), device tensors."""
        torch = self.torch
        self._tensor("mask_moments_batch", "mask", mask, torch.float32)
        if mask.dim() != 3:
            raise ValueError(f"mask_moments_batch: mask of shape {tuple(mask.shape)} is not [n,h,w]")
        n, h, w = int(mask.shape[0]), int(mask.shape[1]), int(mask.shape[2])
        sums = self._new((n, 3), torch.int64)
        bbox = self._new((n, 4), torch.int32)
        self._call("mask_moments_batch", mask, n, h, w, sums, bbox)
        return sums, bbox

    # ------------------------------------------------------------------ template track
    def track_template_batch(self, gray, box, stride, radius, key, want_surface=False):
        """One box followed through a clip by a fixed-template search (include/vstab_track.h states the rule): gray [n,h,w], u8,
        device, contiguous; box = (bx, by, bw, bh) inside frame `key`, in pixels of gray; stride = ceil(max(bw, bh) / 64);
        radius in 1..48.  Nothing is written to gray.  -> (tsums i64 [3] = samples, sum T, sum T^2;  pos i32 [n,2] = (x, y) of
        the box;  best u64 [n];  near u64 [n,9], the 3 x 3 costs around the pick;  surface u64 [n,2R+1,2R+1] | None), device
        tensors; the 64-bit costs as torch.int64 bit patterns (the sentinel 2^64 - 1 reads -1; `.cpu().numpy().view(np.uint64)`)."""
        torch = self.torch
        who = "track_template_batch"
        self._tensor(who, "gray", gray, torch.uint8)
        if gray.dim() != 3:
            raise ValueError(f"{who}: gray of shape {tuple(gray.shape)} is not [n,h,w]")
        n, h, w = int(gray.shape[0]), int(gray.shape[1]), int(gray.shape[2])
        if len(box) != 4:
            raise ValueError(f"{who}: box={box!r} is not (bx, by, bw, bh)")
        bx, by, bw, bh = (_int_in(who, name, v, 0, 1 << 30) for name, v in zip(("bx", "by", "bw", "bh"), box))
        stride = _int_in(who, "stride", stride, 1, 1 << 30)
        radius = _int_in(who, "radius", radius, 1, TRACK_RADIUS_MAX)
        key = _int_in(who, "key", key, 0, max(n - 1, 0))
        d = 2 * radius + 1
        tsums = self._new((3,), torch.int64)
        pos = self._new((n, 2), torch.int32)
        best = self._new((n,), torch.int64)
        near = self._new((n, 9), torch.int64)
        surface = self._new((n, d, d), torch.int64, bool(want_surface))
        work = self._new((track_work_words(radius),), torch.int64)
        self._call("track_template_batch", gray, n, h, w, bx, by, bw, bh, stride, radius, key, tsums, pos, best, near, surface, work)
        return tsums, pos, best, near, surface

    # ------------------------------------------------------------------ horizon level
    def orientation_hist_batch(self, gray, min_mag2: int):
        """The histogram of gradient orientations, folded modulo 90 degrees and weighted by the squared Scharr gradient, of every
        frame of gray [n,h,w], u8, device, contiguous, as exact integers (include/vstab.h states the rule); pixels with a
        squared gradient below min_mag2 (0 .. 2^32 - 1) are left out; nothing is written to the images.
        -> hist i64 [n, 2 * ORIENTATION_K + 1], device tensor; bin k + ORIENTATION_K stands for atan(k / ORIENTATION_K)."""
        torch = self.torch
        self._tensor("orientation_hist_batch", "gray", gray, torch.uint8)
        if gray.dim() != 3:
            raise ValueError(f"orientation_hist_batch: gray of shape {tuple(gray.shape)} is not [n,h,w]")
        min_mag2 = _int_in("orientation_hist_batch", "min_mag2", min_mag2, 0, 0xFFFFFFFF, span="[0, 2^32 - 1]")
        n, h, w = int(gray.shape[0]), int(gray.shape[1]), int(gray.shape[2])
        hist = self._new((n, 2 * ORIENTATION_K + 1), torch.int64)
        self._call("orientation_hist_batch", gray, n, h, w, min_mag2, hist)
        return hist

    # ------------------------------------------------------------------ clean plate
    def _plate_frames(self, who, name, frames, mask, mask_optional=True):
        """frames [n,h,w,3] and mask [n,h,w] | None, both f32, device, contiguous -> (n, h, w)."""
        self._tensor(who, name, frames, self.torch.float32)
        if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) < 1:
            raise ValueError(f"{who}: {name} of shape {tuple(frames.shape)} are not [n,h,w,3] with n, h, w >= 1")
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        self._tensor(who, "mask", mask, self.torch.float32, shape=(n, h, w), optional=mask_optional)
        return n, h, w

    def _plate_inputs(self, who, plate, count, h, w, shot, n, min_count):
        """plate [shots,h,w,3] f32 and count [shots,h,w] i32 (device), shot [n] | None, min_count -> (shots, shot i32 | None)."""
        self._tensor(who, "plate", plate, self.torch.float32)
        if plate.dim() != 4 or tuple(plate.shape[1:]) != (h, w, 3) or plate.shape[0] < 1:
            raise ValueError(f"{who}: plate of shape {tuple(plate.shape)} is not [shots,{h},{w},3]")
        shots = int(plate.shape[0])
        self._tensor(who, "count", count, self.torch.int32, shape=(shots, h, w))
        _int_in(who, "min_count", min_count, 1, PLATE_SAMPLES_MAX)
        sh = None
        if shot is not None:
            sh = _shot_sequence(shot, n, f"{who}: shot of shape {np.shape(shot)} is not a non-decreasing sequence of n={n} shot "
                                         f"numbers in 0..{shots - 1}", shots)
        elif shots != 1:
            raise ValueError(f"{who}: shot=None means one shot, but plate holds {shots}")
        return shots, sh

    def plate_median_batch(self, frames, mask, sample_frame):
        """Clean plate (vstab_plate_median_batch; include/vstab.h states the rule): the per-pixel, per-channel lower median over
        the sampled frames of every shot, among the samples whose mask is <= 0.5.  frames f32 [n,h,w,3] and mask f32 [n,h,w] or
        None (device, contiguous, read only), sample_frame int [shots,S], S in 1..256: strictly increasing frame indices per row,
        then -1 padding (the library refuses anything else by name).  -> (plate f32 [shots,h,w,3], count i32 [shots,h,w])."""
        who = "plate_median_batch"
        n, h, w = self._plate_frames(who, "frames", frames, mask)
        tab = np.ascontiguousarray(sample_frame, dtype=np.int32)
        if tab.ndim != 2 or tab.shape[0] < 1:
            raise ValueError(f"{who}: sample_frame of shape {tab.shape} is not [shots,S]")
        shots, S = int(tab.shape[0]), int(tab.shape[1])
        plate = self._new((shots, h, w, 3), self.torch.float32)
        count = self._new((shots, h, w), self.torch.int32)
        self._call(who, frames, mask, n, h, w, tab, shots, S, plate, count)
        return plate, count

    def plate_fill_batch(self, dst, mask, plate, count, shot, min_count):
        """Fills what is still padding from the plate IN PLACE (vstab_plate_fill_batch): a pixel of frame i with
        !(mask <= 0.5) and count[shot[i]] >= min_count takes the plate's colour and mask 0; every other pixel keeps its bits.
        dst f32 [n,h,w,3], mask f32 [n,h,w], plate / count as plate_median_batch returns them, shot int [n] non-decreasing or None
        (one shot), min_count an int in 1..256.  -> filled_count i32 [n], device tensor."""
        who = "plate_fill_batch"
        n, h, w = self._plate_frames(who, "dst", dst, mask, mask_optional=False)
        shots, sh = self._plate_inputs(who, plate, count, h, w, shot, n, min_count)
        filled = self._new((n,), self.torch.int32)
        self._call(who, dst, mask, n, h, w, plate, count, sh, shots, int(min_count), filled)
        return filled

    def plate_matte_batch(self, frames, mask, plate, count, shot, threshold, min_count):
        """The difference matte against the plate (vstab_plate_matte_batch): 1.0 where the pixel is own (mask <= 0.5, or mask
        None), count[shot[i]] >= min_count and some channel has !(|frame - plate| <= threshold), else 0.0.  Arguments as
        plate_fill_batch; threshold a finite float >= 0; nothing is written to the inputs.
        -> (matte f32 [n,h,w], matte_count i32 [n]), device tensors."""
        who = "plate_matte_batch"
        n, h, w = self._plate_frames(who, "frames", frames, mask)
        shots, sh = self._plate_inputs(who, plate, count, h, w, shot, n, min_count)
        if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
                or not (np.isfinite(threshold) and threshold >= 0):
            raise ValueError(f"{who}: threshold={threshold!r} is not a finite number >= 0")
        matte = self._new((n, h, w), self.torch.float32)
        marked = self._new((n,), self.torch.int32)
        self._call(who, frames, mask, n, h, w, plate, count, sh, shots, float(np.float32(threshold)), int(min_count), matte, marked)
        return matte, marked

    # ------------------------------------------------------------------ sharpness transfer
    def frame_sharpness_batch(self, frames):
        """The gradient energy of every frame of frames [n,h,w,3], f32, device, contiguous, as one exact integer per frame
        (include/vstab.h states the rule: 16-bit fixed-point luma, forward differences, sum of squares); nothing is written
        to the frames.  -> energy i64 [n], device tensor."""
        self._tensor("frame_sharpness_batch", "frames", frames, self.torch.float32)
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"frame_sharpness_batch: frames of shape {tuple(frames.shape)} are not [n,h,w,3]")
        n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        energy = self._new((n,), self.torch.int64)
        self._call("frame_sharpness_batch", frames, n, h, w, energy)
        return energy

    def sharp_transfer_batch(self, clip_frames, matrices, cand_frame, ratio, alpha, dst, mask=None, first=0, interp="bilinear",
                             subpix=None, want_counts=True):
        """Pulls the own pixels (mask != 1; every pixel where mask is None) of output frames [first, first + n) towards what the
        candidates with a positive ratio show there, in place (include/vstab.h: vstab_sharp_transfer_batch).  clip_frames /
        matrices / cand_frame as temporal_fill_batch takes them, ratio [n,K] f32 (finite, >= 0), alpha a finite float >= 0,
        dst [n,h,w,3] f32 device and contiguous, mask [n,h,w] f32 device (read only) or None.  'q5' only.
        -> transfer_count i32 [n] device tensor | None."""
        src, (total, sh, sw), (n, out_h, out_w, k), m, cf, _ = self._neighbour_io(
            "sharp_transfer_batch", clip_frames, matrices, cand_frame, None, dst, mask, subpix)
        r = np.ascontiguousarray(ratio, dtype=np.float32)
        if r.shape != (n, k):
            raise VstabError(f"sharp_transfer_batch: ratio {r.shape} is not [n={n}, K={k}]")
        counts = self._new((n,), self.torch.int32, want_counts)
        self._call("sharp_transfer_batch", src, total, sh, sw, int(first), n, m, cf, k, r, float(alpha), out_h, out_w,
                   INTERP[interp], SUBPIX["q5"], dst, mask, counts)
        return counts

    # ------------------------------------------------------------------ mask hand-off
    def _handoff_mask(self, who, mask):
        self._tensor(who, "mask", mask, self.torch.float32)
        if mask.dim() != 3 or min(mask.shape) < 1:
            raise ValueError(f"{who}: mask of shape {tuple(mask.shape)} is not [n,h,w] with n, h, w >= 1")
        return int(mask.shape[0]), int(mask.shape[1]), int(mask.shape[2])

    def mask_hold_batch(self, mask, hold, shots=None):
        """The maximum of every pixel of mask [n,h,w] (f32, device, contiguous) over the frames within `hold` (an int in 0..16)
        of its own that belong to the same shot (include/vstab.h states the rule; a NaN reads as 1.0, hold = 0 returns the
        input's bits).  shots: None (one shot) or a non-decreasing integer sequence [n].  -> a new device tensor [n,h,w]."""
        n, h, w = self._handoff_mask("mask_hold_batch", mask)
        hold = _int_in("mask_hold_batch", "hold", hold, 0, MASK_HOLD_MAX)
        shot = None
        if shots is not None:
            shot = _shot_sequence(shots, n, f"mask_hold_batch: shots of shape {np.shape(shots)} is not a non-decreasing sequence of "
                                            f"n={n} integers")
        out = self.torch.empty_like(mask)
        self._call("mask_hold_batch", mask, n, h, w, hold, shot, out)
        return out

    def mask_grow_batch(self, mask, grow, tapered=True, feather=0, want_count=False, out=None):
        """ComfyUI's GrowMask on mask [n,h,w] (f32, device, contiguous) and an outward feather behind it (include/vstab.h states
        both rules): grow an int in -64..64 (negative erodes), tapered True = the L1 ball (GrowMask's tapered_corners), False
        = the square one, feather an int in 0..64.  `out`: a tensor like mask to write into (it must not share memory with
        mask), None for a new one.  -> out, or (out, count i32 [n] of pixels > 0.5, a device tensor) with want_count."""
        n, h, w = self._handoff_mask("mask_grow_batch", mask)
        grow = _int_in("mask_grow_batch", "grow", grow, -MASK_GROW_MAX, MASK_GROW_MAX)
        feather = _int_in("mask_grow_batch", "feather", feather, 0, MASK_FEATHER_MAX)
        if not isinstance(tapered, (bool, np.bool_)):
            raise ValueError(f"mask_grow_batch: tapered={tapered!r} is not a bool")
        torch = self.torch
        if out is None:
            out = torch.empty_like(mask)
        else:
            self._tensor("mask_grow_batch", "out", out, torch.float32, shape=mask.shape, text="mask_grow_batch: out must be a "
                         f"contiguous float32 tensor of shape {tuple(mask.shape)} on {self.device}")
            if out.data_ptr() < mask.data_ptr() + mask.numel() * 4 and mask.data_ptr() < out.data_ptr() + out.numel() * 4:
                raise ValueError("mask_grow_batch: out shares memory with mask: a tile's halo would read pixels already written")
        count = self._new((n,), torch.int32, want_count)
        self._call("mask_grow_batch", mask, n, h, w, grow, GROW_TAPERED if tapered else GROW_SQUARE, feather, out, count)
        return (out, count) if want_count else out

    # ------------------------------------------------------------------ Classic estimator (sparse features + LK)
    def gftt_batch(self, gray, max_corners=400, quality=0.01, min_distance=7.0, block_size=21):
        """gray u8 [N,h,w] (device) -> (corners [N,max_corners,2] f32, counts [N] i32), both on the device."""
        torch = self.torch
        if gray.device != self.device:
            gray = gray.to(self.device)
        gray = gray.contiguous()
        n, h, w = gray.shape
        corners = torch.zeros((n, int(max_corners), 2), dtype=torch.float32, device=self.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=self.device)
        self._call("gftt_batch", gray, n, h, w, int(max_corners), float(quality), float(min_distance), int(block_size), corners, counts)
        return corners, counts

    def lk_track_batch(self, gray, points, counts, win=31, max_level=3, max_count=50, epsilon=0.01, want_raw=False):
        """Track points[i] (features of frame i) from frame i to frame i+1 for the N-1 pairs of gray [N,h,w].
        Returns point_pairs [N-1,max,4] (next = NaN where untracked) and, with want_raw, (next [N-1,max,2], status)."""
        torch = self.torch
        gray = gray.contiguous()
        n, h, w = gray.shape
        pairs = n - 1
        if pairs < 1:
            raise VstabError("lk_track_batch needs at least two frames")
        points = points[:pairs].contiguous()
        counts = counts[:pairs].contiguous()
        max_pts = int(points.shape[1])
        out = self._new((pairs, max_pts, 4), torch.float32)
        nxt = torch.zeros((pairs, max_pts, 2), dtype=torch.float32, device=self.device) if want_raw else None
        status = torch.zeros((pairs, max_pts), dtype=torch.uint8, device=self.device) if want_raw else None
        self._call("lk_track_batch", gray, n, h, w, points, counts, max_pts, int(win), int(max_level), int(max_count), float(epsilon),
                   out, nxt, status)
        return (out, nxt, status) if want_raw else out

    def points_fit_batch(self, point_pairs, counts, requested_mode):
        """point_pairs [P,max,4] + counts [P] (device) -> structured table [P,3] (FIT_DTYPE)."""
        point_pairs = point_pairs.contiguous()
        counts = counts[: point_pairs.shape[0]].contiguous()
        pairs, max_pts, _ = point_pairs.shape
        table = np.zeros((pairs, 3), FIT_DTYPE)
        self._call("points_fit_batch", point_pairs, counts, pairs, max_pts, MODES[requested_mode], table)
        return table

    # ------------------------------------------------------------------ fallback estimator (phase correlation)
    def phase_correlate_batch(self, gray):
        """gray u8 [N,h,w] (device) -> (structured table [N-1,3] (FIT_DTYPE, translation row only),
        shifts f64 [N-1,3] = (tx, ty, response) of cv2.phaseCorrelate for every consecutive pair)."""
        if gray.device != self.device:
            gray = gray.to(self.device)
        gray = gray.contiguous()
        if gray.dtype != self.torch.uint8 or gray.dim() != 3:
            raise ValueError("phase_correlate_batch expects a uint8 [N,h,w] tensor")
        n, h, w = gray.shape
        if n < 2:
            raise ValueError("phase_correlate_batch needs at least two frames")
        table = np.zeros((n - 1, 3), FIT_DTYPE)
        shifts = np.zeros((n - 1, 3), np.float64)
        self._call("phase_correlate_batch", gray, n, h, w, table, shifts)
        return table, shifts

    def crop_analysis(self, matrices, src_size, out_size):
        """Nearest coverage of every frame -> (bbox [n,4] of the 3x3-closed coverage or -1, AND of all frames eroded 3x3)."""
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 9)
        n = m.shape[0]
        sw, sh = int(src_size[0]), int(src_size[1])
        ow, oh = int(out_size[0]), int(out_size[1])
        bbox = np.zeros((n, 4), np.int32)
        common = np.zeros((oh, ow), np.uint8)
        self._call("crop_analysis", m, n, sh, sw, oh, ow, bbox, common)
        return bbox, common

    def common_coverage(self, matrices, src_size, out_size):
        """AND over frames of the nearest coverage (motion_apply.py:205-227) -> bool [out_h,out_w] on the host."""
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 9)
        sw, sh = int(src_size[0]), int(src_size[1])
        ow, oh = int(out_size[0]), int(out_size[1])
        common = np.zeros((oh, ow), np.uint8)
        self._call("common_coverage", m, m.shape[0], sh, sw, oh, ow, common)
        return common.astype(bool)

    def trajectory(self, deltas, smooth, fps, strength, camera_lock):
        d = np.ascontiguousarray(deltas, dtype=np.float64)
        n = d.shape[0] + 1
        p = d.shape[1]
        path = np.zeros((n, p), np.float64)
        target = np.zeros((n, p), np.float64)
        self._call("trajectory", d, n, p, float(smooth), float(fps), float(strength), 1 if camera_lock else 0, path, target, stream=False)
        return path, target


_default_ctx: dict = {}


def default_context() -> Context:
    """Per-process context on the current torch device."""
    import torch

    if not torch.cuda.is_available():
        raise VstabError("no MI355X / HIP device visible: the stabilizer hot path has no CPU fallback")
    idx = torch.cuda.current_device()
    ctx = _default_ctx.get(idx)
    if ctx is None:
        ctx = Context(idx)
        _default_ctx[idx] = ctx
    return ctx
