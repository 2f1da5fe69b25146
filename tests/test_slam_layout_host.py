"""CPU: the one buffer layout of the vo_slam_* entry points (visual_odometry_amd/csrc/slam_layout.h: SlamDims, slam_layout,
slam_seq) under AddressSanitizer + UBSan.  The header is pointer arithmetic and calls nothing of the HIP runtime, so
tests/native/slam_layout_driver.cpp places it at a made-up base for every row of SlamDims' table — restart, statistics and
snapshot on and off, one sequence and three of unequal length, a stream's total_pairs on both sides of max_cameras + 1 — and
checks every sub-buffer and every sequence's descriptor against the formulas, restated there.  Nothing is preloaded: the
driver is a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual_odometry_amd", "csrc")


def test_slam_layout_is_sound_under_asan_ubsan():
    if not shutil.which("hipcc") or not shutil.which("make"):
        pytest.skip("no compiler for the project's headers")
    subprocess.check_call(["make", "-s", "-C", CSRC, "slam_layout_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "slam_layout_asan")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
