"""No GPU: the entries of a stream's archive of evicted points (vo_set_stream_archive, vo_stream_archive_info,
vo_stream_archive_read, vo_map_from_stream_archive) as include/vo_hip.h declares them are what the built library exports and what
visual_odometry_amd/_lib.py binds — argument for argument, by count and by kind; the header states the rules; the kernels are where
the kernel page says they are, and the walk's other kernels carry none of it; the Python entries exist with their defaults."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "vo_set_stream_archive": (["ctx", "capacity_points"], ["pointer", "int64_t"]),
    "vo_stream_archive_info": (["ctx", "capacity", "stored", "dropped"], ["pointer", "pointer", "pointer", "pointer"]),
    "vo_stream_archive_read": (["ctx", "first", "n", "feature", "xyz", "evicted_at", "has_row", "rows"],
                               ["pointer", "int64_t", "int64_t", "pointer", "pointer", "pointer", "pointer", "pointer"]),
    "vo_map_from_stream_archive": (["ctx", "frame_first", "frame_end", "with_live", "n_staged", "n_archived", "n_without_row"],
                                   ["pointer", "int", "int", "int", "pointer", "pointer", "pointer"]),
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
    assert lib.vo_version() >= 126
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int32_t\s*\*\s*n_staged\s*,\s*int32_t\s*\*\s*n_archived\s*,\s*int32_t\s*\*\s*n_without_row\s*\)", header)
    # vo_map_from_stream itself is as it was
    assert re.search(r"int vo_map_from_stream\(vo_ctx\* ctx, int frame_first, int frame_end, int32_t\* n_staged, int32_t\* n_without_row\);", header)


def test_the_header_states_the_rules():
    h = _header()
    block = h[h.index("vo_set_stream_archive / vo_stream_archive_info"):h.index(" * vo_map_rows:")]
    assert h.index("relocalisation: a resident frame placed in a map") < h.index("vo_set_stream_archive / vo_stream_archive_info") < h.index("} vo_reloc_opts;")
    for phrase in ("capacity_points (D + 40) bytes", "0 = no archive", "-1 = (total_pairs + 1) kp_cap", "< -1: VO_ERR_INVALID", "resume = 0",
                   "An archive needs the store", "starts nothing", "vo_slam_stream_restart, vo_slam_streams and the chains ignore it",
                   "a point left with exactly one goes, a point with none stays", "in map order", "pair order", "evicted_at", "has_row = 0",
                   "The archive\n *     owns its rows", "for good", "No deduplication", "the bytes they are with it off", "any pointer may be NULL",
                   "with_live = 1", "with_live = 0", "lowest-index tie", "65536", "VO_ERR_UNSUPPORTED", "A failed call leaves no staged map",
                   "vo_map_from_stream itself is unchanged"):
        assert phrase in block, phrase


def test_where_the_kernels_are_and_that_the_other_kernels_carry_none_of_it():
    csrc = os.path.join(ROOT, "visual_odometry_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "stream_archive_kernels.o" in re.search(r"^OBJS\s*=(.*)$", mk, flags=re.M).group(1).split()
    src = open(os.path.join(csrc, "stream_archive_kernels.hip")).read()
    assert src.count("__global__") == 2 and "k_stream_archive_count(" in src and "k_stream_archive_emit(" in src
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower()                                   # positions come from counting, in archive order
    slam = open(os.path.join(csrc, "slam_kernels.hip")).read()
    # one instantiation of the limit appends; SlamBuf and the other instantiations' calls are as they were
    assert len(re.findall(r"slam_limit_wg<true, false, true>", slam)) == 1 and "k_slam_limit_stream_archive(" in slam
    assert slam.count("if constexpr (AR)") == 3 and "SlamArchive" not in open(os.path.join(csrc, "slam_layout.h")).read()
    assert re.search(r"#define SA_TILE (\d+)", open(os.path.join(csrc, "vo_internal.h")).read()).group(1) in ("64", "128", "256")
    reloc = open(os.path.join(csrc, "reloc_kernels.hip")).read()
    assert "k_map_gather_from(" in reloc and reloc.count("void k_map_gather(") == 1
    assert os.path.exists(os.path.join(ROOT, "docs", "kernels", "k_stream_archive.md"))


def test_the_python_entries():
    from visual_odometry_amd import frontend
    FE = frontend.FrontEnd
    assert list(inspect.signature(FE.stream_archive).parameters) == ["self", "capacity"]
    assert inspect.signature(FE.stream_archive).parameters["capacity"].default == -1
    assert list(inspect.signature(FE.stream_archive_info).parameters) == ["self"]
    p = inspect.signature(FE.stream_archive_points).parameters
    assert list(p) == ["self", "first", "n"] and (p["first"].default, p["n"].default) == (0, None)
    p = inspect.signature(FE.map_from_stream_archive).parameters
    assert list(p) == ["self", "first", "end", "live"] and (p["first"].default, p["end"].default, p["live"].default) == (0, None, True)
    # today's call is today's call
    p = inspect.signature(FE.map_from_stream).parameters
    assert list(p) == ["self", "first", "end"] and (p["first"].default, p["end"].default) == (0, None)
