"""csrc/vstab_wait.h on the CPU: the bounded spin that vstab_last_pad_counts, vstab_last_frame_peaks and the TV-L1 poll
share, and the wrap-safe sequence comparison.  The header includes nothing from HIP, so tests/wait_check.cpp (a program of
its own, a second thread in the GPU's place) is built from it alone with the library's host flags plus AddressSanitizer
and UBSan, and run as a child process.  No thread sanitizer: the helper reads a plain volatile word because its real
peer is a GPU."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "comfyui-video-stabilizer_amd" / "csrc"
HOST_FLAGS = ["-std=c++17", "-O3", "-fPIC", "-fno-fast-math", "-Wall"]   # csrc/Makefile, as vstab_codec.cpp is built


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wait") / "wait_check"
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", *HOST_FLAGS, "-Werror", "-pthread",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
           str(ROOT / "tests" / "wait_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-4000:]   # a sanitizer report goes to stderr
    return {k: float(v) for k, v in (line.split() for line in ran.stdout.splitlines())}


def test_word_already_at_its_target_returns_at_once(facts):
    # the limit is 60 s: under 1 s means it did not wait for it
    assert facts["ready_ok"] == 1 and facts["ready_ms"] < 1000.0, facts


def test_word_set_by_a_second_thread_is_seen(facts):
    # set after ~20 ms, limit 60 s; what the writer stored before the word is visible behind the helper's fence
    assert facts["late_ok"] == 1 and facts["late_payload"] == 1234, facts
    assert 20.0 <= facts["late_ms"] < 5000.0, facts


def test_word_never_set_gives_up_behind_the_limit(facts):
    # no sooner than the 50 ms limit; the 5 s cap only keeps a broken clock check from passing, it is no timing claim
    assert facts["never_ok"] == 0 and 50.0 <= facts["never_ms"] < 5000.0, facts


def test_sequence_comparison_across_wrap_around(facts):
    assert facts["seq_before_wrap"] == 0   # have 0xFFFFFFFF, want 2: not reached
    assert facts["seq_after_wrap"] == 1    # have 2, want 0xFFFFFFFE: reached
    assert facts["seq_equal"] == 1
