"""No GPU: vo_map_align_guided as include/vo_hip.h declares it is what the built library exports and what visual_odometry_amd/_lib.py
binds; vo_guided_opts and vo_align_opts are what they were; the refusals that return before the device is touched; the header states
the contract; the Python entries exist with defaults that leave today's calls what they are."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_ERR_INVALID = -1

NAMES = ["ctx", "rows", "points", "off", "Q", "prior", "g", "opts", "sim", "n_match", "n_inl", "status", "n_seen"]


def _header():
    return open(os.path.join(ROOT, "include", "vo_hip.h")).read()


def test_the_symbol_is_declared_exported_and_bound():
    from visual_odometry_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+vo_map_align_guided\s*\(([^;]*)\)\s*;", header)
    assert m, "vo_map_align_guided is not declared in include/vo_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == NAMES
    restype, argtypes = _lib._SIGS["vo_map_align_guided"]
    assert restype is C.c_int and len(argtypes) == len(args)
    for a, t in zip(args, argtypes):
        assert (t is C.c_int) == (a == "int Q") and (t is C.c_void_p) == (a != "int Q"), a
    assert "vo_map_align_guided" in _lib.exported_symbols() and hasattr(lib, "vo_map_align_guided")
    assert lib.vo_version() >= 128
    # the option structs are reused as they stand
    s = re.search(r"typedef struct \{([^}]*)\} vo_guided_opts;", header)
    assert s and re.findall(r"(\w+)\s+(\w+)\s*;", s.group(1)) == [("double", "radius"), ("double", "ratio")]
    assert _lib.GuidedOpts._fields_ == [("radius", C.c_double), ("ratio", C.c_double)] and C.sizeof(_lib.GuidedOpts) == 16
    assert len(re.findall(r"\}\s*vo_guided_opts\s*;", header)) == 1
    assert [n for n, _ in _lib.AlignOpts._fields_] == ["max_distance", "max_error", "iterations", "confidence", "seed", "min_inliers"]
    # the declaration stands behind both structs and behind vo_map_align
    assert header.index("} vo_guided_opts;") < header.index("} vo_align_opts;") < header.index("vo_map_align_matches(") < m.start()


def test_refusals_before_the_device_is_touched():
    from visual_odometry_amd import _lib
    lib = _lib.load()
    rows = (C.c_uint8 * 32)(); pts = (C.c_double * 3)(); off = (C.c_int32 * 2)(0, 1)
    prior = (C.c_double * 13)(*[1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    g = _lib.GuidedOpts(0.5, 0.0); o = _lib.AlignOpts(0.0, 0.05, 1000, 0.99, 0xFFFFFFFFFFFFFFFF, 0)
    sim = (C.c_double * 13)(*[7.0] * 13); i32 = [(C.c_int32 * 1)(7) for _ in range(4)]

    def call(h):
        return lib.vo_map_align_guided(h, rows, pts, off, 1, prior, C.addressof(g), C.addressof(o), sim, *i32)
    assert call(None) == VO_ERR_INVALID
    h = C.c_void_p()
    if lib.vo_create(0, C.byref(h)) != 0:                                  # no device at all: the NULL check above is what can be seen
        return
    try:
        assert call(h) == VO_ERR_INVALID                                   # no staged map
        assert list(sim) == [7.0] * 13 and all(v[0] == 7 for v in i32)
    finally:
        lib.vo_destroy(h)


def test_the_header_states_the_contract():
    h = _header()
    sec = h[h.index("guided map alignment: two maps' points matched in space"):h.index("int vo_map_align_guided(")]
    for phrase in ("y_k = s * ((R[k][0] bx + R[k][1] by) + R[k][2] bz) + t_k", "all three y_k are", "(dx dx + dy dy) + dz dz <= r2", "r2 = radius radius",
                   "STAGED map's units", "never a candidate", "smallest (d, j)", "second-smallest d", "FLT_MAX", "n_seen",
                   "(double)fd < max_distance", "(double)fd < ratio * (double)fd2", "smallest (d, i)", "The filters come first",
                   "ascending query-row order", "the untransformed", "k_sim3_ransac unchanged", "vo_set_map_match is not read",
                   "rows == points == off == prior == NULL", "copied aside", "keeps that status", "serve the most recent", "whatever `ratio` was",
                   "nothing written", "Q <= 64", "65536", "match_nn", "match_select", "merge_maps", "Out of scope"):
        assert phrase in sec, phrase
    out = " ".join(sec[sec.rindex("Out of scope"):].replace("*", " ").split())
    for still_out in ("fusing on the device", "inside the walks", "redirecting a stream's observations", "beyond 65536 points", "averaging the positions",
                      "scale-aware or covariance-aware radius", "grid cached across calls"):
        assert still_out in out, still_out


def test_the_python_entries():
    from visual_odometry_amd import _lib, frontend
    FE = frontend.FrontEnd
    p = inspect.signature(FE.align_maps).parameters
    assert p["refine_radius"].default is None and list(p)[-1] == "refine_radius"
    assert list(p)[1:4] == ["rows", "points", "max_error"] and p["match"].default == "cross"
    p = inspect.signature(FE.align_maps_guided).parameters
    assert list(p)[1:6] == ["rows", "points", "prior", "radius", "max_error"] and p["max_error"].default is inspect.Parameter.empty
    assert p["offsets"].default is None and p["ratio"].default == 0.0 and p["max_distance"].default == 0.0
    a = inspect.signature(FE.align_maps).parameters
    assert all(p[k].default == a[k].default for k in ("iterations", "confidence", "seed", "min_inliers"))
    p = inspect.signature(frontend.merge_maps).parameters
    assert list(p) == ["rows_a", "points_a", "rows_b", "points_b", "scale", "R", "t", "a_idx", "b_idx", "mask"]
    p = inspect.signature(FE.fuse_map).parameters
    assert list(p)[1:5] == ["rows", "points", "max_error", "radius"]
    assert callable(_lib.Context.map_align_guided)
    src = open(os.path.join(ROOT, "examples", "fuse_maps.py")).read()
    assert "align_maps_guided" in src or "refine_radius" in src
    assert "fuse_map" in src or "merge_maps" in src
