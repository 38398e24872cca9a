"""NumPy restatement of the crop coverage analysis behind framing_mode="crop" (include/vstab.h: vstab_crop_analysis), for the
tests.

It starts from per-frame boolean coverage planes and restates only what happens to them afterwards: the 3x3 morphology with
the border ignored (cv2.dilate / cv2.erode with their default border: a pixel outside the image never wins the max nor the
min), the bounding box of the closing, the AND over frames and its erosion.  Where the planes come from (the nearest-neighbour
coordinate rule) is not restated here: the oracle's vo_warp_frame supplies them (oracle.coverage_planes).  Nothing here imports
the package.
"""

from __future__ import annotations

import numpy as np


def _neighbours(plane, outside):
    """The nine 3x3 neighbours of every pixel of a bool plane [h,w], as a list of nine [h,w] planes; a neighbour that lies
    outside the image reads `outside`."""
    p = np.asarray(plane, dtype=bool)
    h, w = p.shape
    padded = np.full((h + 2, w + 2), bool(outside))
    padded[1:h + 1, 1:w + 1] = p
    return [padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def dilate3(plane):
    """3x3 dilate: OR over the neighbours inside the image (an outside neighbour reads 0, which an OR ignores)."""
    out = np.zeros(np.asarray(plane).shape, bool)
    for nb in _neighbours(plane, False):
        out |= nb
    return out


def erode3(plane):
    """3x3 erode: AND over the neighbours inside the image (an outside neighbour reads 1, which an AND ignores)."""
    out = np.ones(np.asarray(plane).shape, bool)
    for nb in _neighbours(plane, True):
        out &= nb
    return out


def closing3(plane):
    return erode3(dilate3(plane))


def bbox_of(plane):
    """(x_min, y_min, x_max, y_max) of the set pixels, inclusive; (-1, -1, -1, -1) if none is set."""
    ys, xs = np.nonzero(np.asarray(plane, dtype=bool))
    if ys.size == 0:
        return (-1, -1, -1, -1)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def common_of(cov):
    """AND over the frames of the coverage planes [n,h,w] -> bool [h,w]."""
    cov = np.asarray(cov, dtype=bool)
    out = np.ones(cov.shape[1:], bool)
    for plane in cov:
        out &= plane
    return out


def crop_analysis(cov):
    """Coverage planes bool [n,h,w] -> (bbox int32 [n,4] of each frame's closing, uint8 [h,w] eroded AND of the planes): the
    two results of vstab_crop_analysis."""
    cov = np.asarray(cov, dtype=bool)
    bbox = np.array([bbox_of(closing3(plane)) for plane in cov], np.int32).reshape(-1, 4)
    return bbox, erode3(common_of(cov)).astype(np.uint8)
