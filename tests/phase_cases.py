"""Frame pairs shared by tests/test_phase_referee_cpu.py (oracle vs float64 reference) and tests/test_phase_gpu.py (HIP
kernel vs the same reference), their references (computed once per session) and the tolerances measured on the CPU side.

(a) radix / stage coverage: every length is an optimal DFT size, so a circular roll of white noise is circular in the
    transform's domain.  The lengths cover each radix alone (8..2048, 9..729, 5..625), each radix as first, middle and
    last stage, butterflies per stage below and above the 256 threads of a workgroup, the LDS maximum (2048), odd and even
    lengths (1, 2 or 4 purely real bins) and a side of 1.
(b) sizes that are padded (rows, columns or both), as crops of a larger image: the shift is not circular there.
(c) rolls that put the peak on row / column 0, 1 or last of the shifted plane: the 5 x 5 window is clamped.
(d) one pair at the working size."""

import functools

import numpy as np

from tests.phase_reference import phase_reference

# Worst figures of the oracle against the reference over every case and clip below (measured, not chosen:
# tests/test_phase_referee_cpu.py::test_measured_figures prints them), and the tolerances = 10 x measured: the HIP kernel
# equals the oracle bit for bit, the factor absorbs another libm behind the twiddle table.
#   shift 1.94e-6 px (radix-5x1), response 2.11e-7 (seam-8x54x96 pair 3), surface 4.50e-6 (padded-textured-45x73)
MEASURED_SHIFT, MEASURED_RESPONSE, MEASURED_SURFACE = 1.94e-6, 2.11e-7, 4.50e-6
SHIFT_TOL = 10 * MEASURED_SHIFT          # px, |tx - tx_ref| and |ty - ty_ref|
RESPONSE_TOL = 10 * MEASURED_RESPONSE    # |response - response_ref|
SURFACE_TOL = 10 * MEASURED_SURFACE      # max |surface - surface_ref| / max |surface_ref|

RADIX_LENGTHS = (5, 8, 9, 15, 16, 18, 25, 27, 30, 32, 45, 75, 81, 125, 243, 250, 256, 512, 625, 729, 768, 1024, 1280, 1875,
                 1944, 2000, 2025, 2048)
PADDED_SIZES = ((31, 17), (45, 73), (100, 161), (257, 511), (33, 2000), (2048, 17))
CLAMP_SIZES = ((135, 240), (64, 96), (45, 75), (1, 16), (16, 1))
WORKING_SIZE = (540, 960)


def crop_clip(n, h, w, seed, textured, max_shift=6):
    """n crops of one larger image whose origin walks by a drawn (dy, dx), |d| <= max_shift, per frame: Gaussian-smoothed
    texture (as the clips of tests/test_phase_gpu.py) or white noise."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    big = rng.uniform(0, 255, (h + 48, w + 48))
    if textured:
        big = gaussian_filter(big, 1.5)
        big = (big - big.min()) / (big.max() - big.min()) * 255.0
    frames, oy, ox = [], 24, 24
    for i in range(n):
        if i:
            dy, dx = (int(v) for v in rng.integers(-max_shift, max_shift + 1, 2))
            oy, ox = int(np.clip(oy + dy, 0, 48)), int(np.clip(ox + dx, 0, 48))
        frames.append(big[oy:oy + h, ox:ox + w].astype(np.uint8))
    return np.stack(frames)


def crop_pair(h, w, seed, textured):
    return crop_clip(2, h, w, seed, textured)


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _radix_pair(h, w, length):
    rng = np.random.default_rng(100003 * h + w)
    bound = min(7, length // 2 - 1)
    # a component is never drawn as 0 on a side > 1: on the 5-, 8- and 9-point planes a window around an unmoved peak
    # covers the whole plane and its sum is ~ 0
    dy, dx = (int(rng.integers(1, bound + 1)) * int(rng.choice((-1, 1))) if side > 1 else 0 for side in (h, w))
    base = _noise(h, w, rng)
    return np.stack([base, np.roll(base, (dy, dx), axis=(0, 1))])


def _clamp_rolls(h, w):
    rolls = [(0, w // 2), (h // 2, 0), (h // 2, w // 2), (-(h // 2) + 1, -(w // 2) + 1), ((h - 1) // 2, (w - 1) // 2)]
    return [(dy if h > 1 else 0, dx if w > 1 else 0) for dy, dx in rolls]


def _clamp_pair(h, w, dy, dx):
    base = _noise(h, w, 7919 * h + w)
    return np.stack([base, np.roll(base, (dy, dx), axis=(0, 1))])


def _build_cases():
    cases = {}
    for length in RADIX_LENGTHS:
        shapes = [(16, length), (length, 16)] if length >= 15 else [(length, length), (1, length), (length, 1)]
        for h, w in shapes:
            cases[f"radix-{h}x{w}"] = functools.partial(_radix_pair, h, w, length)
    for h, w in PADDED_SIZES:
        cases[f"padded-textured-{h}x{w}"] = functools.partial(crop_pair, h, w, 31 * h + w, True)
        cases[f"padded-noise-{h}x{w}"] = functools.partial(crop_pair, h, w, 37 * h + w, False)
    for h, w in CLAMP_SIZES:
        for i, (dy, dx) in enumerate(_clamp_rolls(h, w)):
            cases[f"clamp-{h}x{w}-roll{i}({dy},{dx})"] = functools.partial(_clamp_pair, h, w, dy, dx)
    h, w = WORKING_SIZE
    cases[f"working-{h}x{w}"] = functools.partial(crop_pair, h, w, 540960, True)
    return cases


_CASES = _build_cases()
CASE_IDS = tuple(_CASES)


@functools.lru_cache(maxsize=None)
def pair(case_id):
    """u8 [2, h, w], read-only."""
    frames = np.ascontiguousarray(_CASES[case_id](), dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def reference(case_id):
    frames = pair(case_id)
    return phase_reference(frames[0], frames[1])


def _repeat_clip(h, w):
    a, b, c = crop_clip(3, h, w, 53 * h + w, True)
    return np.stack([a, b, b, c])


# clips of the GPU tests (chunk seams, identical consecutive frames); the CPU referee runs them too, so the measured
# figures above cover every comparison that uses the tolerances
_CLIPS = {
    "seam-8x54x96": functools.partial(crop_clip, 8, 54, 96, 77, True),
    "repeat-4x45x73": functools.partial(_repeat_clip, 45, 73),     # padded to 45 x 75: origin at (0.5, 0.5)
    "repeat-4x64x96": functools.partial(_repeat_clip, 64, 96),     # origin at (0, 0)
}
CLIP_IDS = tuple(_CLIPS)
REPEATED_PAIR = 1   # frames 1 and 2 of a repeat clip are identical


@functools.lru_cache(maxsize=None)
def clip(clip_id):
    """u8 [n, h, w], read-only."""
    frames = np.ascontiguousarray(_CLIPS[clip_id](), dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def clip_references(clip_id):
    frames = clip(clip_id)
    return tuple(phase_reference(frames[i], frames[i + 1]) for i in range(len(frames) - 1))


def assert_well_conditioned(ref, what):
    """The conditioning rule is a condition on the INPUT, asserted and never used to skip: a listed case that fails it
    needs another input."""
    assert ref.well_conditioned, f"{what}: ill-conditioned input (margin {ref.margin:.3g}, response {ref.response:.3g})"
