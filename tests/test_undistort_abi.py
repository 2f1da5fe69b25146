"""No GPU: vo_undistort_points and vo_frames_undistort as include/vo_hip.h declares them are what visual_odometry_amd/_lib.py binds —
argument for argument, by count and by kind (a pointer or array, or an int passed by value) — and the Python entries carry cv2's
argument names."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "vo_hip.h")).read()


def _declared(name):
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/vo_hip.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        pointer = "*" in a or "[" in a
        out.append((re.sub(r"\[.*", "", a.split()[-1].lstrip("*")), "pointer" if pointer else a.rsplit(" ", 1)[0]))
    return out


def _check(name, names, kinds):
    from visual_odometry_amd import _lib
    declared = _declared(name)
    restype, argtypes = _lib._SIGS[name]
    assert restype is C.c_int and len(argtypes) == len(declared) == len(names)
    assert [n for n, _ in declared] == names
    assert [k for _, k in declared] == kinds
    for (arg, kind), t in zip(declared, argtypes):
        assert t is (C.c_void_p if kind == "pointer" else C.c_int), (arg, kind, t)
    assert name in _lib.exported_symbols()


def test_the_prototypes_match_the_bindings():
    _check("vo_undistort_points", ["ctx", "points", "N", "point_type", "K", "dist", "ndist", "R", "P", "out"],
           ["pointer", "pointer", "int", "int", "pointer", "pointer", "int", "pointer", "pointer", "pointer"])
    _check("vo_frames_undistort", ["ctx", "first_slot", "F", "K", "dist", "ndist"], ["pointer", "int", "int", "pointer", "pointer", "int"])


def test_the_stage_count_and_the_header_block():
    from visual_odometry_amd import _lib
    h = _header()
    assert int(re.search(r"#define\s+VO_STAGE_COUNT\s+(\d+)", h).group(1)) == _lib.VO_STAGE_COUNT == 30
    block = h[h.index("cv2.undistortPoints"):h.index("int vo_frames_undistort")]
    for phrase in ("src/image_and_keypoints.py:21-25", "five fixed-point iterations", "thin-prism", "tilt", "unpinned", "after any resize",
                   "dimensionless"):
        assert phrase in block, phrase
    lib = _lib.load()
    assert lib.vo_stage_name(29) == b"undistort_points" and lib.vo_stage_name(28) == b"slam_map_statistics" and lib.vo_stage_name(30) == b"?"


def test_the_python_entries_take_cv2s_arguments():
    from visual_odometry_amd import cv2_surface, geometry
    from visual_odometry_amd.frontend import FrontEnd
    assert list(inspect.signature(geometry.undistortPoints).parameters) == ["src", "cameraMatrix", "distCoeffs", "R", "P", "ctx"]
    assert list(inspect.signature(cv2_surface.undistortPoints).parameters) == ["src", "cameraMatrix", "distCoeffs", "R", "P"]
    assert "undistortPoints" in cv2_surface.ARITHMETIC and hasattr(cv2_surface.HipBackend, "undistortPoints")
    assert list(inspect.signature(FrontEnd.undistort).parameters) == ["self", "first_slot", "count", "K", "dist"]
    assert "BEFORE" in FrontEnd.undistort.__doc__
