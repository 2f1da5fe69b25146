"""No GPU: vo_map_localize_guided and vo_guided_opts as include/vo_hip.h declares them are what the built library exports and what
visual_odometry_amd/_lib.py binds; the refusals that return before the device is touched; the header states the contract; the Python
entries exist with defaults that leave today's calls what they are."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_ERR_INVALID, VO_ERR_NOT_CONFIGURED = -1, -5

NAMES = ["ctx", "slots", "Q", "K[9]", "prior", "g", "opts", "poses", "n_match", "n_inl", "status", "n_seen"]


def _header():
    return open(os.path.join(ROOT, "include", "vo_hip.h")).read()


def test_the_symbol_and_the_struct_are_declared_exported_and_bound():
    from visual_odometry_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+vo_map_localize_guided\s*\(([^;]*)\)\s*;", header)
    assert m, "vo_map_localize_guided is not declared in include/vo_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == NAMES
    restype, argtypes = _lib._SIGS["vo_map_localize_guided"]
    assert restype is C.c_int and len(argtypes) == len(args)
    for a, t in zip(args, argtypes):
        assert (t is C.c_int) == (a == "int Q") and (t is C.c_void_p) == (a != "int Q"), a
    assert "vo_map_localize_guided" in _lib.exported_symbols() and hasattr(lib, "vo_map_localize_guided")
    assert lib.vo_version() >= 127
    s = re.search(r"typedef struct \{([^}]*)\} vo_guided_opts;", header)
    assert s and re.findall(r"(\w+)\s+(\w+)\s*;", s.group(1)) == [("double", "radius"), ("double", "ratio")]
    assert _lib.GuidedOpts._fields_ == [("radius", C.c_double), ("ratio", C.c_double)] and C.sizeof(_lib.GuidedOpts) == 16
    assert (_lib.GuidedOpts.radius.offset, _lib.GuidedOpts.ratio.offset) == (0, 8)
    # the option struct of the pose part is what it was
    assert [n for n, _ in _lib.RelocOpts._fields_] == ["max_distance", "pnp_iterations", "reproj_err", "confidence", "seed", "min_inliers"]


def test_refusals_before_the_device_is_touched():
    from visual_odometry_amd import _lib
    lib = _lib.load()
    sl = (C.c_int32 * 1)(0); K = (C.c_double * 9)(*[1, 0, 0, 0, 1, 0, 0, 0, 1]); P = (C.c_double * 12)(*[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    g = _lib.GuidedOpts(5.0, 0.0); o = _lib.RelocOpts(0.0, 100, 8.0, 0.99, 0xFFFFFFFFFFFFFFFF, 0)
    poses = (C.c_double * 12)(*[7.0] * 12); i32 = [(C.c_int32 * 1)(7) for _ in range(4)]

    def call(h):
        return lib.vo_map_localize_guided(h, sl, 1, K, P, C.addressof(g), C.addressof(o), poses, *i32)
    assert call(None) == VO_ERR_INVALID
    h = C.c_void_p()
    if lib.vo_create(0, C.byref(h)) != 0:                                  # no device at all: the NULL check above is what can be seen
        return
    try:
        assert call(h) == VO_ERR_NOT_CONFIGURED                            # before any batch configuration, hence before any staged map
        assert list(poses) == [7.0] * 12 and all(v[0] == 7 for v in i32)
    finally:
        lib.vo_destroy(h)


def test_the_header_states_the_contract():
    h = _header()
    sec = h[h.index("guided relocalisation: map points matched by projection"):h.index("} vo_guided_opts;")]
    for phrase in ("c_2 > 0", "dx dx + dy dy <= r2", "r2 = radius radius", "K's third row", "no image-bounds test", "smallest (d, i)",
                   "second-smallest d", "FLT_MAX", "n_seen", "(double)fd < max_distance", "(double)fd < ratio * (double)fd2", "smallest (d, j)",
                   "The filters come first", "ascending keypoint order", "k_pnp_ransac unchanged", "vo_set_map_match is not read",
                   "prior == NULL", "copied aside", "keeps that status", "vo_map_matches serves the most recent", "whatever `ratio` was",
                   "nothing written", "match_nn", "match_select", "Out of scope"):
        assert phrase in sec, phrase
    out = " ".join(sec[sec.rindex("Out of scope"):].replace("*", " ").split())
    for still_out in ("inside the walks", "octave and scale prediction", "viewing-angle tests", "more than one point per keypoint"):
        assert still_out in out, still_out
    reloc = h[h.index("relocalisation: a resident frame placed in a map"):h.index("} vo_reloc_opts;")]
    assert "automatic use inside the walks" in reloc[reloc.rindex("Out of scope"):]
    assert "guided relocalisation, below" in reloc


def test_the_python_entries():
    from visual_odometry_amd import _lib, frontend, geometry
    FE = frontend.FrontEnd
    p = inspect.signature(FE.relocalize).parameters
    assert p["refine_radius"].default is None and list(p)[-1] == "refine_radius"
    p = inspect.signature(FE.relocalize_guided).parameters
    assert list(p)[1:5] == ["slots", "K", "prior", "radius"] and p["ratio"].default == 0.0 and p["max_distance"].default == 0.0
    assert (p["iterations"].default, p["reproj_err"].default, p["confidence"].default, p["min_inliers"].default) == (100, 8.0, 0.99, 0)
    assert p["seed"].default == inspect.signature(FE.relocalize).parameters["seed"].default
    p = inspect.signature(geometry.relocalize_guided).parameters
    assert list(p)[:7] == ["map_points", "map_descriptors", "keypoints_xy", "descriptors", "K", "prior", "radius"]
    assert callable(_lib.Context.map_localize_guided)
    src = open(os.path.join(ROOT, "examples", "loop_flight.py")).read()
    assert '"--guided"' in src and "refine_radius" in src or "relocalize_guided" in src
