"""CPU: what the host prepares for vo_pose_graph_batch (visual_odometry_amd/csrc/pgo_layout.h: validation, the elimination order,
the CSR lists, the scratch layout) under AddressSanitizer + UBSan.  The header calls nothing of the HIP runtime, so
tests/native/pgo_layout_driver.cpp runs it on the small graphs of tests/test_gpu_pose_graph.py, alone and as one batch with an
over-capacity and an invalid graph between them, and checks: the order is a permutation of the free vertices, every free vertex
lies in exactly one run or is a separator, the CSR lists are complete and in input order, every buffer lies inside the allocation.
Nothing is preloaded: the driver is a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual_odometry_amd", "csrc")


def test_pgo_layout_is_sound_under_asan_ubsan():
    if not shutil.which("hipcc") or not shutil.which("make"):
        pytest.skip("no compiler for the project's headers")
    subprocess.check_call(["make", "-s", "-C", CSRC, "pgo_layout_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "pgo_layout_asan")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failures" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
