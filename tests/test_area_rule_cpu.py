"""csrc/vstab_area.h on the CPU: the one statement of cv2.resize(..., INTER_AREA) on 8-bit gray that the gray pass's resize
kernels and the DIS pyramid call.  The header includes nothing from HIP, so tests/area_check.cpp (a program of its own)
resizes with it on the host, built with the library's host flags plus AddressSanitizer and UBSan and run as a child
process; every image must equal oracle/vo_gray.c's vo_resize_area_u8 byte for byte."""
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "comfyui-video-stabilizer_amd" / "csrc"
HOST_FLAGS = ["-std=c++17", "-O3", "-fPIC", "-fno-fast-math", "-Wall"]   # csrc/Makefile, as vstab_codec.cpp is built

CLIPPED = (14, 77, 14, 35)   # 77 -> 35: see test_the_clipped_case_is_one

# name -> (sh, sw, dh, dw, constant or None)
CASES = {
    "one_to_one": (30, 40, 30, 40, None),
    "box_2x2": (48, 64, 24, 32, None),
    "box_3x2": (60, 90, 30, 30, None),
    "box_4x4": (32, 64, 8, 16, None),
    "ratio_1_333": (72, 128, 54, 96, None),
    "halving_135_33": (33, 135, 16, 67, None),
    "halving_33_135": (135, 33, 67, 16, None),
    "ratio_4_03": (67, 121, 16, 30, None),
    "above_eight_taps": (70, 130, 11, 20, None),      # 6.5 x 6.36
    "ratio_25_6": (256, 256, 10, 10, None),
    "clipped_last_cell": CLIPPED + (None,),
    "constant_255": (67, 121, 16, 30, 255),
    "constant_1": (72, 128, 54, 96, 1),
    "constant_77_above_eight_taps": (70, 130, 11, 20, 77),
}


@pytest.fixture(scope="module")
def resized(tmp_path_factory, oracle):
    tmp = tmp_path_factory.mktemp("area")
    exe = tmp / "area_check"
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", *HOST_FLAGS, "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
           str(ROOT / "tests" / "area_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    rng = np.random.default_rng(37)
    images = {}
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for name, (sh, sw, dh, dw, const) in CASES.items():
            img = rng.integers(0, 256, (sh, sw), dtype=np.uint8) if const is None else np.full((sh, sw), const, np.uint8)
            images[name] = img
            f.write(struct.pack("<4i", sh, sw, dh, dw))
            f.write(img.tobytes())
    ran = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-4000:]   # a sanitizer report goes to stderr
    tables = [int(line.split()[3]) for line in ran.stdout.splitlines()]
    assert len(tables) == len(CASES)
    raw = np.fromfile(tmp / "out.bin", dtype=np.uint8)
    out, at = {}, 0
    for (name, (sh, sw, dh, dw, _)), same in zip(CASES.items(), tables):
        got = raw[at:at + dh * dw].reshape(dh, dw)
        at += dh * dw
        out[name] = (got, oracle.resize_area_u8(images[name], (dw, dh)), same)
    assert at == raw.size
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_header_rule_matches_oracle(resized, name):
    got, ref, _ = resized[name]
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("name", list(CASES))
def test_eight_weight_tables_give_the_run_form(resized, name):
    """Below the eight-weight limit the AreaTaps records (the LDS kernels' form) give the bytes of the run form; at or
    above it the program does not form them, as the library does not."""
    sh, sw, dh, dw, _ = CASES[name]
    same = resized[name][2]
    assert same == (1 if max(sh / dh, sw / dw) < 6.0 else -1)


def test_constant_images_stay_constant(resized):
    for name, (_, _, _, _, const) in CASES.items():
        if const is not None:
            assert np.all(resized[name][0] == const), name


def test_the_clipped_case_is_one():
    """computeResizeAreaTab's cellWidth is min(scale, ssize - fsx1): in fp64 the last cell of 77 -> 35 starts past
    ssize - scale, so its width is the clipped one."""
    ssize, dsize = CLIPPED[1], CLIPPED[3]
    scale = 1.0 / (dsize / ssize)
    assert ssize - (dsize - 1) * scale < scale
