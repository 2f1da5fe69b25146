"""No GPU: vo_set_map_match and vo_map_match_seconds as include/vo_hip.h declares them are what the built library exports and what
visual_odometry_amd/_lib.py binds; the setting's argument checks (they touch no device); the header states the rule and no longer lists
ratio matching against the map as out of scope; the Python entries take match / ratio with defaults that are today's calls."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_ERR_INVALID = -1

ENTRIES = {
    "vo_set_map_match": (["ctx", "mode", "ratio"], [C.c_void_p, C.c_int, C.c_double]),
    "vo_map_match_seconds": (["ctx", "which", "q", "dist2", "cap", "n_out"], [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
}


def _header():
    return open(os.path.join(ROOT, "include", "vo_hip.h")).read()


def test_both_symbols_are_declared_exported_and_bound():
    from visual_odometry_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, (names, types) in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/vo_hip.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names, name
        restype, argtypes = _lib._SIGS[name]
        assert restype is C.c_int and list(argtypes) == types, name
        for a, t in zip(args, types):
            assert ("*" in a) == (t is C.c_void_p) and ("double" in a and "*" not in a) == (t is C.c_double), (name, a)
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.vo_version() >= 125


def test_the_setting_checks_its_arguments():
    """vo_create and the setting touch no device buffer: this runs without a GPU as tests/test_abi_and_host.py's context checks do."""
    from visual_odometry_amd import _lib
    lib = _lib.load()
    assert lib.vo_set_map_match(None, 0, 0.75) == VO_ERR_INVALID
    h = C.c_void_p()
    if lib.vo_create(0, C.byref(h)) != 0:                                  # no device at all: the NULL check above is what can be seen
        return
    try:
        nan, inf = float("nan"), float("inf")
        for mode in (1, 2):
            assert lib.vo_set_map_match(h, mode, 0.75) == 0 and lib.vo_set_map_match(h, mode, 1.5) == 0
            for ratio in (0.0, -0.5, nan, inf, -inf):
                assert lib.vo_set_map_match(h, mode, ratio) == VO_ERR_INVALID, (mode, ratio)
        for mode in (3, -1, 17):
            assert lib.vo_set_map_match(h, mode, 0.75) == VO_ERR_INVALID, mode
        for ratio in (0.75, 0.0, -1.0, nan, inf):                          # mode 0 does not read it
            assert lib.vo_set_map_match(h, 0, ratio) == 0, ratio
        n = C.c_int32(0)
        assert lib.vo_map_match_seconds(h, 0, 0, None, 0, C.addressof(n)) == VO_ERR_INVALID      # nothing staged, nothing run
        assert lib.vo_map_match_seconds(h, 2, 0, None, 0, C.addressof(n)) == VO_ERR_INVALID
    finally:
        lib.vo_destroy(h)


def test_the_header_states_the_rule():
    h = _header()
    assert not re.search(r"ratio\s+matching\s*(\*\s*)?(against\s+the\s+map)?\s*\.?\s*(\*/|\()", h)
    reloc = h[h.index("relocalisation: a resident frame placed in a map"):h.index("} vo_reloc_opts;")]
    align = h[h.index("map alignment: the similarity that joins two maps"):h.index("} vo_align_opts;")]
    for block in (reloc, align):
        out = block[block.rindex("Out of scope"):]
        assert "ratio matching" not in " ".join(out.replace("*", " ").split())
    for phrase in ("vo_set_map_match", "knnMatch(k=2)", "(double)fd < ratio * (double)fd2", "at least 2 rows", "lowest index among the nearest rows",
                   "a tie with m counting as a second neighbour", "mode 2", "vo_map_match_seconds", "FLT_MAX", "VO_ERR_TOO_FEW", "Several query rows may keep one map point"):
        assert phrase in reloc, phrase
    assert "vo_set_map_match" in align and "vo_map_match_seconds(which = 1)" in align
    # the option structs are what they were
    assert re.search(r"typedef struct \{\s*double\s+max_distance;[^}]*int32_t\s+min_inliers;[^}]*\} vo_reloc_opts;", h)
    from visual_odometry_amd import _lib
    assert [n for n, _ in _lib.RelocOpts._fields_] == ["max_distance", "pnp_iterations", "reproj_err", "confidence", "seed", "min_inliers"]
    assert [n for n, _ in _lib.AlignOpts._fields_] == ["max_distance", "max_error", "iterations", "confidence", "seed", "min_inliers"]


def test_the_python_entries_default_to_the_cross_check():
    from visual_odometry_amd import _lib, frontend, geometry
    FE = frontend.FrontEnd
    for f in (FE.relocalize, FE.align_maps, geometry.relocalize):
        p = inspect.signature(f).parameters
        assert p["match"].default == "cross" and p["ratio"].default == 0.75, f
    assert _lib.MAP_MATCH_MODES == {"cross": 0, "ratio": 1, "cross+ratio": 2}
    assert callable(FE.map_match_seconds) and callable(FE.map_align_match_seconds) and callable(_lib.Context.set_map_match)
    src = open(os.path.join(ROOT, "examples", "loop_flight.py")).read()
    assert '"--ratio"' in src and 'match="ratio"' in src
