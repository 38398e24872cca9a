"""NumPy restatement of the clean plate's three rules (include/vstab.h: vstab_plate_median_batch, vstab_plate_fill_batch,
vstab_plate_matte_batch) and of clean_plate.py's host side.  The GPU tests hold the kernels to it in bits; nothing here is
imported from the package."""

import numpy as np

SAMPLES_MAX = 256
TOP = np.uint32(0xFFFFFFFF)
QNAN = np.uint32(0x7FC00000)


def order_key(values):
    """float32 -> uint32 order key: the total order of the sign-magnitude bits, -0.0 below +0.0; every NaN the largest key."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    b = v.view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), TOP, key).astype(np.uint32)


def unkey(keys):
    """The sample's own bits back; the NaN key gives 0x7FC00000."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == TOP, QNAN, b).astype(np.uint32).view(np.float32)


def valid_of(mask, shape):
    """mask <= 0.5, a NaN is not; None: every pixel."""
    if mask is None:
        return np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, dtype=np.float32) <= np.float32(0.5)


def plate_median(frames, mask, sample_frame):
    """frames [n,h,w,3], mask [n,h,w] | None, sample_frame int [shots,S] (-1 padded) -> (plate f32 [shots,h,w,3], count i32
    [shots,h,w]).  Samples that are not valid sort as the largest key, where rank (count - 1) // 2 < count never reaches them."""
    frames = np.asarray(frames, dtype=np.float32)
    n, h, w, _ = frames.shape
    table = np.asarray(sample_frame, dtype=np.int64)
    plate = np.zeros((table.shape[0], h, w, 3), np.float32)
    count = np.zeros((table.shape[0], h, w), np.int32)
    for s, row in enumerate(table):
        idx = row[row >= 0]
        valid = valid_of(None if mask is None else np.asarray(mask)[idx], (len(idx), h, w))
        keys = np.where(valid[..., None], order_key(frames[idx]), TOP)
        keys = np.sort(keys, axis=0)
        cnt = valid.sum(axis=0).astype(np.int32)
        rank = np.maximum(cnt - 1, 0) // 2
        picked = np.take_along_axis(keys, np.broadcast_to(rank[None, ..., None], (1, h, w, 3)), axis=0)[0]
        plate[s] = np.where((cnt > 0)[..., None], unkey(picked), np.float32(0.0))
        count[s] = cnt
    return plate, count


def plate_median_literal(frames, mask, row):
    """One shot, pixel by pixel, channel by channel: np.sort on the keys of the valid samples only (the slow form the fast
    one above is checked against)."""
    frames = np.asarray(frames, dtype=np.float32)
    n, h, w, _ = frames.shape
    idx = [int(f) for f in row if f >= 0]
    plate = np.zeros((h, w, 3), np.float32)
    count = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            ok = [f for f in idx if mask is None or bool(np.float32(mask[f, y, x]) <= np.float32(0.5))]
            count[y, x] = len(ok)
            if not ok:
                continue
            for c in range(3):
                keys = np.sort(order_key(np.array([frames[f, y, x, c] for f in ok], np.float32)))
                plate[y, x, c] = unkey(keys[(len(ok) - 1) // 2:(len(ok) - 1) // 2 + 1])[0]
    return plate, count


def _shots(shot, n):
    return np.zeros((n,), np.int64) if shot is None else np.asarray(shot, dtype=np.int64)


def plate_fill(dst, mask, plate, count, shot, min_count):
    """-> (dst', mask', filled_count u32 [n]); the inputs are left as they are."""
    dst, mask = np.array(dst, dtype=np.float32), np.array(mask, dtype=np.float32)
    sh = _shots(shot, dst.shape[0])
    filled = np.zeros((dst.shape[0],), np.uint32)
    for i in range(dst.shape[0]):
        fill = ~valid_of(mask[i], mask[i].shape) & (np.asarray(count)[sh[i]] >= int(min_count))
        dst[i].view(np.uint32)[fill] = np.asarray(plate, dtype=np.float32)[sh[i]].view(np.uint32)[fill]
        mask[i][fill] = np.float32(0.0)
        filled[i] = fill.sum()
    return dst, mask, filled


def plate_matte(frames, mask, plate, count, shot, threshold, min_count):
    """-> (matte f32 [n,h,w], matte_count u32 [n])."""
    frames = np.asarray(frames, dtype=np.float32)
    n, h, w, _ = frames.shape
    sh = _shots(shot, n)
    thr = np.float32(threshold)
    matte = np.zeros((n, h, w), np.float32)
    for i in range(n):
        own = valid_of(None if mask is None else np.asarray(mask)[i], (h, w))
        with np.errstate(invalid="ignore", over="ignore"):
            same = (np.abs(frames[i] - np.asarray(plate, dtype=np.float32)[sh[i]]) <= thr).all(axis=-1)     # float32 throughout
        matte[i] = (own & (np.asarray(count)[sh[i]] >= int(min_count)) & ~same).astype(np.float32)
    return matte, matte.sum(axis=(1, 2)).astype(np.uint32)


def sample_table(segments, total_frames):
    """Per shot [s, e) of length L: min(L, 256) samples at s + ((2k + 1) * L) // (2 * S), rows padded with -1."""
    segs = [(0, total_frames)] if segments is None else list(segments)
    rows = []
    for s, e in segs:
        length = e - s
        size = min(length, SAMPLES_MAX)
        rows.append([s + ((2 * k + 1) * length) // (2 * size) for k in range(size)])
    width = max(len(r) for r in rows)
    return np.array([r + [-1] * (width - len(r)) for r in rows], np.int32)


def shots_of(segments, total_frames):
    if segments is None:
        return None
    shot = np.zeros((total_frames,), np.int32)
    for k, (s, e) in enumerate(segments):
        shot[s:e] = k
    return shot


def meta_block(min_count, table, filled, mask_after, count):
    """meta["plate_fill"] from the fill's counts, the mask behind the fill and the plate's counts."""
    n, h, w = mask_after.shape
    pixels = np.float32(h * w)

    def fraction(c):
        return (np.asarray(c, dtype=np.int64).astype(np.float32) / pixels).astype(np.float64)

    left = (~valid_of(mask_after, mask_after.shape)).sum(axis=(1, 2))
    unseen = (np.asarray(count) < int(min_count)).sum(axis=(1, 2))
    return {"version": 1, "min_count": int(min_count), "shots": int(table.shape[0]),
            "samples_per_shot": [int(v) for v in (np.asarray(table) >= 0).sum(axis=1)],
            "filled_fraction_mean": float(np.mean(fraction(filled))), "filled_fraction_max": float(np.max(fraction(filled))),
            "padding_fraction_mean_after": float(np.mean(fraction(left))), "padding_fraction_max_after": float(np.max(fraction(left))),
            "frames_with_padding_after": int((left > 0).sum()), "unseen_fraction": [float(v) for v in fraction(unseen)]}


def pipeline(warped, warped_mask, before_fill, before_fill_mask, segments, min_count):
    """The order the pipeline keeps: the plate from the frames under the warp's true mask (warped, warped_mask: the outputs of
    a call without any fill), the fill on what the temporal fill left (before_fill, before_fill_mask: the outputs of the call
    with the temporal fill only; the same arrays where there is none).  -> (frames, mask, meta block, plate, count)."""
    n = warped.shape[0]
    table = sample_table(segments, n)
    plate, count = plate_median(warped, warped_mask, table)
    frames, mask, filled = plate_fill(before_fill, before_fill_mask, plate, count, shots_of(segments, n), min_count)
    return frames, mask, meta_block(min_count, table, filled, mask, count), plate, count
