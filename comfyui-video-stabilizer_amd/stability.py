"""Stability report: how steady a clip is, as the inter-frame transformation fidelity (ITF) of the stabilization literature.

ITF is the mean PSNR between consecutive frames, here over the pixels both frames really show (`mask <= 0.5` in both).  The
sums come from `native.Context.frame_sse_batch` (csrc/vstab_stability.hip) as exact integers -- see include/vstab.h for the
rule -- and everything in this module is host arithmetic on those integers, in float64.  The peak value is 1.0: frames are
the ComfyUI IMAGE range.  Off by default everywhere; a report reads its frames and writes nothing to them.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import numpy as np

METHOD = "itf"
VERSION = 1
SSE_SCALE = 4294967296.0   # the kernel's fixed point: 2^32 per unit of squared difference


def check_request(stability_report) -> bool:
    """The keyword of the pipelines: a bool, anything else is a ValueError naming the value."""
    if not isinstance(stability_report, bool):
        raise ValueError(f"stability_report={stability_report!r} is not a bool (True adds the ITF of the inputs and of the "
                         "outputs to the meta, False leaves it out)")
    return stability_report


def psnr_db(sse, count) -> np.ndarray:
    """Per-pair PSNR in dB from the kernel's integers: 10 * log10(3 * count * 2^32 / sse), float64.  sse == 0 (identical
    where both are valid) gives inf, count == 0 (no common valid pixel) gives nan."""
    sse = np.asarray(sse, dtype=np.float64).reshape(-1)
    count = np.asarray(count, dtype=np.float64).reshape(-1)
    if sse.shape != count.shape:
        raise ValueError(f"stability: {sse.shape[0]} sums and {count.shape[0]} counts")
    out = np.full(sse.shape, np.nan, np.float64)
    some = count > 0
    out[some & (sse == 0)] = np.inf
    finite = some & (sse > 0)
    out[finite] = 10.0 * np.log10(3.0 * count[finite] * SSE_SCALE / sse[finite])
    return out


def summary(sse, count, pixels: int, skip: Sequence[int] = ()) -> Dict[str, Any]:
    """The ITF block of one clip from its per-pair integers.  skip: indices of pairs left out of every figure (the pairs
    across scene cuts).  Mean and minimum are over the pairs with a finite PSNR; None if there is none."""
    sse = np.asarray(sse, dtype=np.int64).reshape(-1)
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    keep = np.ones(sse.shape, bool)
    keep[[int(k) for k in skip]] = False
    sse, count = sse[keep], count[keep]
    psnr = psnr_db(sse, count)
    finite = psnr[np.isfinite(psnr)]
    return {"pairs": int(sse.shape[0]),
            "itf_db": float(np.mean(finite)) if finite.size else None,
            "psnr_db_min": float(np.min(finite)) if finite.size else None,
            "pairs_without_overlap": int(np.count_nonzero(count == 0)),
            "overlap_fraction_mean": float(np.mean(count.astype(np.float64) / float(pixels))) if count.size else 0.0}


def _frames_mask(ctx, frames, mask):
    torch = ctx.torch
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"stability: frames of shape {tuple(frames.shape)} are not [N,H,W,3]")
    if mask is not None:
        if mask.dim() == 4 and mask.shape[3] == 1:
            mask = mask.reshape(mask.shape[:3])
        if tuple(mask.shape) != tuple(frames.shape[:3]):
            raise ValueError(f"stability: mask of shape {tuple(mask.shape)} does not match frames {tuple(frames.shape)}")
        mask = mask.to(dtype=torch.float32).contiguous()
    return frames.contiguous(), mask


def itf(frames, mask=None, *, ctx=None, cuts: Sequence[int] = ()) -> Dict[str, Any]:
    """The consecutive-frame form on a device clip: frames [N,H,W,3] f32, mask [N,H,W] (or [N,H,W,1]) or None.  Every frame
    is compared with the next one in ONE call (b = a + one frame).  cuts: first frames of shots; the pair that ends at such
    a frame is left out.  -> {pairs, itf_db, psnr_db_min, pairs_without_overlap, overlap_fraction_mean}."""
    from . import native

    ctx = ctx or native.default_context()
    frames, mask = _frames_mask(ctx, frames, mask)
    n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    if n < 2:
        return summary([], [], max(1, h * w))
    sse, count = ctx.frame_sse_batch(frames[:-1], frames[1:], None if mask is None else mask[:-1], None if mask is None else mask[1:])
    sse, count = sse.cpu().numpy(), count.cpu().numpy()
    return summary(sse, count, h * w, skip=[int(c) - 1 for c in cuts])


def compare(a, b, mask_a=None, mask_b=None, *, ctx=None) -> np.ndarray:
    """The frame-against-frame form: PSNR in dB of a[k] against b[k] over the pixels valid in both, float64 [n] (inf for
    identical frames, nan without a common valid pixel)."""
    from . import native

    ctx = ctx or native.default_context()
    a, mask_a = _frames_mask(ctx, a, mask_a)
    b, mask_b = _frames_mask(ctx, b, mask_b)
    if int(a.shape[0]) == 0:
        return np.zeros((0,), np.float64)
    sse, count = ctx.frame_sse_batch(a, b, mask_a, mask_b)
    return psnr_db(sse.cpu().numpy(), count.cpu().numpy())


def report_block(before: Optional[Dict[str, Any]], after: Dict[str, Any], pairs_across_cuts: Optional[int] = None) -> Dict[str, Any]:
    """The meta block.  gain_db = after.itf_db - before.itf_db, None where either is missing.  pairs_across_cuts: only for a
    scene-aware run, whose pairs across a cut are in neither mean."""
    gain = None
    if before is not None and before.get("itf_db") is not None and after.get("itf_db") is not None:
        gain = float(after["itf_db"] - before["itf_db"])
    block = {"method": METHOD, "version": VERSION, "before": before, "after": after, "gain_db": gain}
    if pairs_across_cuts is not None:
        block["pairs_across_cuts"] = int(pairs_across_cuts)
    return block


def report_on_device(ctx, source, frames, mask, cuts: Optional[Sequence[int]] = None) -> Dict[str, Any]:
    """The pipelines' block: the ITF of the source frames without a mask, and of the returned frames under the returned
    padding mask (None: `crop` framing has none)."""
    cut_list = [] if cuts is None else [int(c) for c in cuts]
    before = itf(source, None, ctx=ctx, cuts=cut_list)
    after = itf(frames, mask, ctx=ctx, cuts=cut_list)
    return report_block(before, after, None if cuts is None else len(cut_list))
