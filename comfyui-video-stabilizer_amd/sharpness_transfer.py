"""Sharpness transfer: repair shake-blurred frames from sharper neighbours (not a feature of the reference).

A camera jolt blurs the frames it hits.  While the picture shakes nobody sees that; once it stands still, those frames read
as a sharpness pulse.  Matsushita et al. ("Full-frame video stabilization with motion inpainting", PAMI 2006) treat this as
the second half of full-frame stabilization (section 5): pixels are transferred from sharper neighbouring frames, registered
by the transitions the stabilizer already has.  Their first half, motion inpainting, is this package's temporal fill, and
the candidates are the fill's: `temporal_fill.fill_candidates` forms H_{i,j} = F_i (chain i -> j)^-1 for the up to 2R
neighbours of every frame.

Two device passes (include/vstab.h states both rules):
  * `native.Context.frame_sharpness_batch` (csrc/vstab_sharp.hip) gives every SOURCE frame's gradient energy E as one exact
    integer; `ratios_from_energy` turns it into the relative sharpness E_j / E_i of candidate j against frame i, 0 where the
    neighbour is not clearly sharper;
  * `native.Context.sharp_transfer_batch` (csrc/vstab_neighbour.hip: sharp_transfer_kernel) pulls every own pixel of frame i's
    OUTPUT towards the candidates' samples, each weighted by ratio / (ratio + alpha * D) with D the L1 colour distance to
    the pixel, the pixel itself with weight 1.  Padded pixels are left to the fills, which run afterwards.

Off by default.  The per-frame sharpness list in the meta is also the companion of the stability report's ITF, which
rewards blur (README "Stability report").
"""

from __future__ import annotations

import math
from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import temporal_fill

MAX_RADIUS = 16           # K = 2 * radius <= 32 candidates per frame, every one of them sampled
MAX_ALPHA = 1024.0
# Choices, not calibrations.  MIN_RATIO: a neighbour must carry a tenth more gradient energy than the frame before the frame
# borrows from it -- it exists so that noise does not make every frame borrow from every other.  DEFAULT_ALPHA: how fast a
# sample that disagrees with the pixel loses its say (at alpha = 16 and ratio = 1 a sample 1/16 away in L1 has weight 1/2);
# tried on synthetic material only.
MIN_RATIO = 1.1
DEFAULT_ALPHA = 16.0


def check_request(sharpness_transfer=None, sharpness_alpha=None, subpix=None) -> Optional[Tuple[int, float]]:
    """-> (radius, alpha) of a `sharpness_transfer` / `sharpness_alpha` request, None = off.  sharpness_transfer: 0, None or
    False is off, otherwise an int in 1..MAX_RADIUS; sharpness_alpha: None is DEFAULT_ALPHA, else a finite number in
    [0, MAX_ALPHA].  Everything is checked here, before any GPU work, the 'q5' sub-pixel mode included."""
    off = sharpness_transfer is None or sharpness_transfer is False or \
        (isinstance(sharpness_transfer, (int, np.integer)) and not isinstance(sharpness_transfer, (bool, np.bool_)) and int(sharpness_transfer) == 0)
    if not off:
        if isinstance(sharpness_transfer, (bool, np.bool_)) or not isinstance(sharpness_transfer, (int, np.integer)) \
                or not 1 <= int(sharpness_transfer) <= MAX_RADIUS:
            raise ValueError(f"sharpness_transfer={sharpness_transfer!r} is not 0, None, False or an integer in 1..{MAX_RADIUS}")
    alpha = DEFAULT_ALPHA
    if sharpness_alpha is not None:
        if isinstance(sharpness_alpha, (bool, np.bool_)) or not isinstance(sharpness_alpha, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(sharpness_alpha)) or not 0.0 <= float(sharpness_alpha) <= MAX_ALPHA:
            raise ValueError(f"sharpness_alpha={sharpness_alpha!r} is not None or a finite number in [0, {MAX_ALPHA:g}]")
        if off:
            raise ValueError(f"sharpness_alpha={sharpness_alpha!r} needs sharpness_transfer > 0: it weights the transferred samples")
        alpha = float(sharpness_alpha)
    if off:
        return None
    if subpix is None:
        from . import native
        subpix = native.DEFAULT_SUBPIX
    if subpix != "q5":
        raise ValueError(f"sharpness_transfer is not supported in sub-pixel mode {subpix!r}: the transfer samples on the 1/32-px "
                         "coordinates of 'q5'")
    return int(sharpness_transfer), alpha


def check_pipeline(estimator: str, mesh_warp=None) -> None:
    """What the transfer cannot be combined with, each with its reason (checked before any GPU work)."""
    if mesh_warp is not None:
        raise ValueError("sharpness_transfer is not supported with mesh_warp: transfer candidates are global matrices, and a "
                         "mesh-warped frame is not the image of its neighbours under one matrix")
    if estimator == "subject":
        raise ValueError("sharpness_transfer is not supported with estimator 'subject': its transitions are the subject's, not the "
                         "camera's, so they do not register a neighbour's background")


def ratios_from_energy(energy, cand_frame, first: int = 0) -> np.ndarray:
    """energy [N] (vstab_frame_sharpness_batch, the whole clip), cand_frame [n, K] of output frames [first, first + n)
    -> ratio float32 [n, K]: E_j / E_i formed in float64 and cast to float32; 0 where cand_frame < 0, where E_i == 0 (a flat
    frame has nothing to compare against) or where the quotient is below MIN_RATIO."""
    e = np.asarray(energy).astype(np.float64).reshape(-1)
    cand = np.asarray(cand_frame, dtype=np.int64)
    if cand.ndim != 2 or first < 0 or first + cand.shape[0] > e.shape[0] or (cand >= e.shape[0]).any():
        raise ValueError(f"sharpness transfer: cand_frame {cand.shape} from frame {first} does not fit {e.shape[0]} energies")
    own = e[first:first + cand.shape[0], None]
    ok = (cand >= 0) & (own > 0.0)
    quotient = np.where(ok, e[np.where(cand >= 0, cand, 0)], 0.0) / np.where(ok, own, 1.0)
    return np.where(ok & (quotient >= MIN_RATIO), quotient, 0.0).astype(np.float32)


def sharpness_from_energy(energy, source_size) -> np.ndarray:
    """energy / (2^32 (w - 1)(h - 1)): the mean squared luma difference per pixel, luma in 0..1; 0 for a one-pixel-wide frame."""
    w, h = int(source_size[0]), int(source_size[1])
    pairs = (w - 1) * (h - 1)
    e = np.asarray(energy).astype(np.float64).reshape(-1)
    return e / (4294967296.0 * pairs) if pairs > 0 else np.zeros_like(e)


def meta_block(radius: int, alpha: float, energy, source_size, ratios, transfer_counts, output_size) -> Dict[str, Any]:
    """meta["sharpness_transfer"].  frames_sharpened counts the frames with at least one transferred pixel; the fractions
    are formed like `padding_fraction_*` (float32 count / float32 pixels)."""
    pixels = np.float32(int(output_size[0]) * int(output_size[1]))
    counts = np.asarray(transfer_counts, dtype=np.int64).reshape(-1)
    frac = (counts.astype(np.float32) / pixels).astype(np.float64)
    r = np.asarray(ratios, dtype=np.float32)
    return {"version": 1, "radius": int(radius), "alpha": float(alpha), "min_ratio": MIN_RATIO,
            "sharpness": [float(v) for v in sharpness_from_energy(energy, source_size)],
            "frames_sharpened": int((counts > 0).sum()),
            "ratio_max": float(r.max()) if r.size else 0.0,
            "transferred_fraction_mean": float(np.mean(frac)) if frac.size else 0.0,
            "transferred_fraction_max": float(np.max(frac)) if frac.size else 0.0}


def transfer_on_device(ctx, device_frames, dst, mask, final_matrices, transitions, confidences, radius: int, alpha: float,
                       interp: str = "bilinear", subpix=None, energy=None) -> Dict[str, Any]:
    """Runs the transfer over a whole clip in place (dst [N,h,w,3] device; mask [N,h,w] device, read only, or None: every pixel
    is own) and returns the meta block.  energy: the source clip's `frame_sharpness_batch` result where the caller queued
    it earlier, else it is launched here.  One small download (the energies) sits between the two launches."""
    if energy is None:
        energy = ctx.frame_sharpness_batch(device_frames)
    mats, cand = temporal_fill.fill_candidates(final_matrices, transitions, confidences, radius)
    energy = energy.cpu().numpy()
    ratios = ratios_from_energy(energy, cand)
    counts = ctx.sharp_transfer_batch(device_frames, mats, cand, ratios, alpha, dst, mask, first=0, interp=interp, subpix=subpix)
    return meta_block(radius, alpha, energy, (device_frames.shape[2], device_frames.shape[1]), ratios, counts.cpu().numpy(),
                      (dst.shape[2], dst.shape[1]))
