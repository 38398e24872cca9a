"""Float64 reference of the phase-correlation estimator (cv2.phaseCorrelate without a window) for the referee tests.

Plain NumPy: numpy.fft for both transforms, no butterflies, no twiddle table, nothing restated from oracle/vo_phase.c
or csrc/vstab_phase.hip.  The operation is the one documented in the header of vstab_phase.hip:

  zero-pad both images to (M, N) = optimal DFT sizes;  P = F1 conj(F2);  C = P |P| / (|P|^2 + FLT_EPSILON), except at
  the purely real bins kx in {0, N/2 if N even} x ky in {0, M/2 if M even}, where C = Re(P) / (Re(P)^2 + FLT_EPSILON);
  unscaled inverse transform, real part;  circular shift by (M/2, N/2);  first maximum in raster order;  5 x 5 window
  clamped to the plane;  sum, cx, cy in double with cx, cy divided by sum + DBL_EPSILON;  response = sum / (M N);
  shift = (N/2.0 - cx, M/2.0 - cy).

Besides the result it reports how well defined that result is (`margin`, `response`): the centroid divides by the window
sum, so where the clamped window covers most of a tiny plane (sum ~ 0) or two maxima tie, the shift means nothing and no
implementation can be held to it."""

from typing import NamedTuple, Tuple

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)

# a case is compared only where the reference itself says the answer is well defined
MIN_MARGIN = 1e-3     # (top1 - top2) / top1 on the shifted float64 surface
MIN_RESPONSE = 0.2


def optimal_dft_size(n):
    """Smallest 2^a 3^b 5^c >= n."""
    v = int(n)
    while True:
        t = v
        for r in (2, 3, 5):
            while t % r == 0:
                t //= r
        if t == 1:
            return v
        v += 1


class PhaseReference(NamedTuple):
    shift: Tuple[float, float, float]   # (tx, ty, response) as cv2.phaseCorrelate returns them
    surface: np.ndarray                 # f64 [M, N], unshifted, scaled like an unscaled inverse transform
    peak: Tuple[int, int]               # (row, column) of the first maximum in the shifted plane
    margin: float                       # (top1 - top2) / top1 of the shifted surface
    response: float

    @property
    def well_conditioned(self):
        return self.margin >= MIN_MARGIN and self.response >= MIN_RESPONSE


def phase_reference(a, b, optimal_dft_size=optimal_dft_size):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.ndim == 2 and a.shape == b.shape
    h, w = a.shape
    M, N = optimal_dft_size(h), optimal_dft_size(w)
    P = np.fft.fft2(a, s=(M, N)) * np.conj(np.fft.fft2(b, s=(M, N)))   # s= pads with zeros at the bottom / right
    mag = np.abs(P)
    C = P * mag / (mag * mag + FLT_EPSILON)
    for ky in {0, M // 2} if M % 2 == 0 else {0}:
        for kx in {0, N // 2} if N % 2 == 0 else {0}:
            pr = P[ky, kx].real
            C[ky, kx] = pr / (pr * pr + FLT_EPSILON)
    surface = np.fft.ifft2(C).real * (M * N)
    shifted = np.roll(surface, (M // 2, N // 2), axis=(0, 1))
    py, px = (int(v) for v in np.unravel_index(np.argmax(shifted), shifted.shape))   # argmax: first maximum, C order
    r0, r1 = max(py - 2, 0), min(py + 2, M - 1)
    c0, c1 = max(px - 2, 0), min(px + 2, N - 1)
    win = shifted[r0:r1 + 1, c0:c1 + 1]
    total = float(win.sum())
    cx = float((win * np.arange(c0, c1 + 1)[None, :]).sum()) / (total + DBL_EPSILON)
    cy = float((win * np.arange(r0, r1 + 1)[:, None]).sum()) / (total + DBL_EPSILON)
    response = total / (M * N)
    if shifted.size > 1:
        top2, top1 = np.partition(shifted.ravel(), shifted.size - 2)[-2:]
        margin = float((top1 - top2) / top1) if top1 > 0 else 0.0
    else:
        margin = 1.0
    return PhaseReference((N / 2.0 - cx, M / 2.0 - cy, response), surface, (py, px), margin, response)
