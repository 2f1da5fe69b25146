"""No GPU: the entries of a stream's descriptor store (vo_set_stream_rows, vo_stream_rows_info, vo_map_from_stream) as
include/vo_hip.h declares them are what the built library exports and what visual_odometry_amd/_lib.py binds — argument for
argument, by count and by kind (a pointer, an int or an int64_t passed by value); the header says what the tests hold the device
to and what remains out of scope; the kernels are built from a file of their own; the Python entries exist with their defaults."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "vo_set_stream_rows": (["ctx", "capacity_rows"], ["pointer", "int64_t"]),
    "vo_stream_rows_info": (["ctx", "capacity", "stored", "dropped"], ["pointer", "pointer", "pointer", "pointer"]),
    "vo_map_from_stream": (["ctx", "frame_first", "frame_end", "n_staged", "n_without_row"], ["pointer", "int", "int", "pointer", "pointer"]),
}
CTYPE = {"pointer": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64}


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


def test_the_prototypes_match_the_bindings_and_the_library():
    from visual_odometry_amd import _lib
    lib = _lib.load()
    for name, (names, kinds) in ENTRIES.items():
        declared = _declared(name)
        restype, argtypes = _lib._SIGS[name]
        assert restype is C.c_int and len(argtypes) == len(declared) == len(names), name
        assert [n for n, _ in declared] == names, name
        assert [k for _, k in declared] == kinds, name
        for (arg, kind), t in zip(declared, argtypes):
            assert t is CTYPE[kind], (name, arg, kind, t)
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name), f"{name} is not exported by libvo_hip.so"
    assert lib.vo_version() >= 124
    # the counts come back as int64_t, the staged sizes as int32_t
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"vo_stream_rows_info\s*\(\s*vo_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*capacity\s*,\s*int64_t\s*\*\s*stored\s*,\s*int64_t\s*\*\s*dropped\s*\)", header)
    assert re.search(r"int32_t\s*\*\s*n_staged\s*,\s*int32_t\s*\*\s*n_without_row\s*\)", header)


def test_the_header_states_the_rules_and_what_remains_out():
    h = _header()
    block = h[h.index("vo_set_stream_rows / vo_stream_rows_info / vo_map_from_stream"):h.index("} vo_reloc_opts;")]
    for phrase in ("capacity_rows D + 4 (total_pairs + 1) kp_cap", "IN MAP ORDER", "a hole", "dropped", "for good", "vo_set_slam_stats' rule",
                   "[frame_first, frame_end)", "frame_end < 0", "n_without_row", "An empty selection", "65536", "VO_ERR_UNSUPPORTED", "VO_ERR_INVALID",
                   "A failed call leaves no staged map", "resume = 1", "vo_slam_stream_restart", "vo_slam_streams", "Out of scope",
                   "archive of earlier segments", "automatic use inside the walks", "window of more than 65536 points"):
        assert phrase in block, phrase
    assert "a stream keeps no descriptor store of its own" not in h and "a stream's own descriptor store, " not in h
    assert h.count("restart streams and multi-streams") == 2             # the relocaliser's and the aligner's "Out of scope"


def test_the_kernels_are_a_file_of_their_own_and_the_walk_is_untouched():
    csrc = os.path.join(ROOT, "visual_odometry_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "stream_rows_kernels.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    src = open(os.path.join(csrc, "stream_rows_kernels.hip")).read()
    assert src.count("__global__") == 2 and "k_stream_rows_append(" in src and "k_stream_rows_select(" in src
    assert "atomic" not in src.lower()                                    # positions come from counting, in map order: no atomics, no inter-workgroup word
    for name in ("slam_kernels.hip", "slam_layout.h"):
        assert "row_of" not in open(os.path.join(csrc, name)).read(), name   # the walk does not know the store exists


def test_the_python_entries():
    from visual_odometry_amd import frontend
    FE = frontend.FrontEnd
    assert list(inspect.signature(FE.stream_rows).parameters) == ["self", "capacity"]
    assert inspect.signature(FE.stream_rows).parameters["capacity"].default == -1
    assert list(inspect.signature(FE.stream_rows_info).parameters) == ["self"]
    p = inspect.signature(FE.map_from_stream).parameters
    assert list(p) == ["self", "first", "end"] and (p["first"].default, p["end"].default) == (0, None)
    assert list(inspect.signature(FE.map_from_slam).parameters) == ["self", "which", "seq"]
    assert "map_from_stream" in FE.map_from_slam.__doc__
