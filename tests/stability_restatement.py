"""NumPy restatement of the stability report's rule (include/vstab.h, vstab_frame_sse_batch), for the tests.

Per pair: a pixel is valid in a frame iff mask <= 0.5 (a NaN is not); it counts iff valid in both frames.  Per counting
pixel and channel: d = a - b in float32, e = d * d in float64 (exact), capped at 4 (a NaN takes the cap), q = floor(e * 2^32)
as an integer.  sse is the integer sum of q, count the number of counting pixels.  Integer sums have no order: the kernel
must equal this exactly.  The summary below restates stability.summary / report_block from the formulas of the issue.
"""

import numpy as np

TWO32 = 4294967296.0


def valid_of(mask, shape):
    """mask [..] float or None -> bool of `shape`: mask <= 0.5, NaN (and inf, and anything above 0.5) not valid."""
    if mask is None:
        return np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32) <= np.float32(0.5)


def terms(a, b):
    """a, b [...] float32 -> uint64 [...]: q of every element."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (a - b).astype(np.float32)                   # one float32 subtraction
        e = d.astype(np.float64) * d.astype(np.float64)  # exact: 24-bit significands
        e = np.where(e < 4.0, e, 4.0)                    # NaN and inf take the cap
    return np.floor(e * TWO32).astype(np.uint64)         # e * 2^32 <= 2^34 is exact; floor of a non-negative = truncation


def frame_sse(a, b, mask_a=None, mask_b=None):
    """a, b [n,h,w,3]; masks [n,h,w] or None -> (sse [n] Python-int object array, count [n] int64)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    n = a.shape[0]
    counting = valid_of(mask_a, a.shape[:3]) & valid_of(mask_b, a.shape[:3])
    q = terms(a, b)
    q[~counting] = 0
    sse = np.array([int(q[k].sum(dtype=np.uint64)) for k in range(n)], dtype=object)   # < 2^59 per frame: no wrap
    count = counting.reshape(n, -1).sum(axis=1).astype(np.int64)
    return sse, count


def consecutive(frames, mask=None):
    frames = np.asarray(frames, np.float32)
    if mask is not None:
        mask = np.asarray(mask, np.float32).reshape(frames.shape[:3])
    return frame_sse(frames[:-1], frames[1:], None if mask is None else mask[:-1], None if mask is None else mask[1:])


def psnr_db(sse, count):
    """10 * log10(3 * count * 2^32 / sse) in float64; inf where sse == 0, nan where count == 0."""
    s = np.array([float(int(v)) for v in sse], np.float64)
    c = np.array([float(int(v)) for v in count], np.float64)
    out = np.where(c == 0, np.nan, np.inf)
    some = (c > 0) & (s > 0)
    out[some] = 10.0 * np.log10(3.0 * c[some] * TWO32 / s[some])
    return out


def itf_block(frames, mask=None, cuts=()):
    """{pairs, itf_db, psnr_db_min, pairs_without_overlap, overlap_fraction_mean} of a clip, the pairs ending at a frame of
    `cuts` left out."""
    frames = np.asarray(frames, np.float32)
    pixels = frames.shape[1] * frames.shape[2]
    if frames.shape[0] < 2:
        return {"pairs": 0, "itf_db": None, "psnr_db_min": None, "pairs_without_overlap": 0, "overlap_fraction_mean": 0.0}
    sse, count = consecutive(frames, mask)
    keep = [k for k in range(len(sse)) if (k + 1) not in set(int(c) for c in cuts)]
    sse, count = sse[keep], count[keep]
    psnr = psnr_db(sse, count)
    finite = psnr[np.isfinite(psnr)]
    return {"pairs": len(keep),
            "itf_db": float(np.mean(finite)) if finite.size else None,
            "psnr_db_min": float(np.min(finite)) if finite.size else None,
            "pairs_without_overlap": int((count == 0).sum()),
            "overlap_fraction_mean": float(np.mean(count.astype(np.float64) / float(pixels))) if len(keep) else 0.0}


def report(before, after, pairs_across_cuts=None):
    gain = None
    if before is not None and before["itf_db"] is not None and after["itf_db"] is not None:
        gain = float(after["itf_db"] - before["itf_db"])
    block = {"method": "itf", "version": 1, "before": before, "after": after, "gain_db": gain}
    if pairs_across_cuts is not None:
        block["pairs_across_cuts"] = int(pairs_across_cuts)
    return block
