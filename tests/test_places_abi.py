"""No GPU: the place-recognition entries (vo_vocab_*, vo_places_*) as include/vo_hip.h declares them are what the built library
exports and what visual_odometry_amd/_lib.py binds — argument for argument, by count and by kind (a pointer or array, or an int
passed by value); vo_places_opts is PlacesOpts field for field; the stage count stays 30 (the assignment is bracketed under match_nn,
the rest under misc); the header's section says what the tests hold the device to; the Python entries exist with their defaults."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "vo_vocab_train": (["ctx", "slots", "F", "K", "iterations", "iterations_run"], ["pointer", "pointer", "int", "int", "int", "pointer"]),
    "vo_vocab_set": (["ctx", "words", "K"], ["pointer", "pointer", "int"]),
    "vo_vocab_get": (["ctx", "words", "cap", "K"], ["pointer", "pointer", "int", "pointer"]),
    "vo_vocab_words": (["ctx", "slot", "word", "cap", "n"], ["pointer", "int", "pointer", "int", "pointer"]),
    "vo_places_open": (["ctx", "capacity"], ["pointer", "int"]),
    "vo_places_add": (["ctx", "slots", "F", "ids", "first_entry"], ["pointer", "pointer", "int", "pointer", "pointer"]),
    "vo_places_add_hist": (["ctx", "hist", "ids", "n", "first_entry"], ["pointer", "pointer", "pointer", "int", "pointer"]),
    "vo_places_entries": (["ctx", "first", "n", "hist", "sum", "ids"], ["pointer", "int", "int", "pointer", "pointer", "pointer"]),
    "vo_places_size": (["ctx", "n", "K"], ["pointer", "pointer", "pointer"]),
    "vo_places_query": (["ctx", "entries", "Q", "opts", "out_entry", "out_shared"], ["pointer", "pointer", "int", "pointer", "pointer", "pointer"]),
}


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
            assert t is (C.c_void_p if kind == "pointer" else C.c_int), (name, arg, kind, t)
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name), f"{name} is not exported by libvo_hip.so"
    assert lib.vo_version() >= 123


def test_the_options_and_the_stage_count():
    from visual_odometry_amd import _lib
    h = _header()
    m = re.search(r"typedef struct \{([^}]*)\} vo_places_opts;", h)
    fields = [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", m.group(1)).split(";") if f.strip()]
    assert fields == ["int32_t top_k", "int32_t min_gap", "int32_t min_shared"]
    assert [(n, t) for n, t in _lib.PlacesOpts._fields_] == [("top_k", C.c_int32), ("min_gap", C.c_int32), ("min_shared", C.c_int32)]
    assert C.sizeof(_lib.PlacesOpts) == 12 and _lib.PlacesOpts.min_shared.offset == 8
    assert int(re.search(r"#define\s+VO_STAGE_COUNT\s+(\d+)", h).group(1)) == _lib.VO_STAGE_COUNT == 30
    block = h[h.index("place recognition: device vocabulary"):h.index("} vo_places_opts;")]
    for phrase in ("floor(w n / K)", "2 ones_b > c", "(2 sum_j + c) / (2 c)", "keeps its row", "min(255,", "compared in 64-bit", "never meets itself",
                   "lower entry index first", "VO_ERR_TOO_FEW", "VO_ERR_UNSUPPORTED", "VO_ERR_NOT_CONFIGURED", "closes the index", "match_nn", "the same bytes",
                   "Out of scope", "tf-idf"):
        assert phrase in block, phrase


def test_the_limits_are_the_same_everywhere():
    src = open(os.path.join(ROOT, "visual_odometry_amd", "csrc", "places_api.hip")).read()
    lim = {k: re.search(r"#define\s+%s\s+(\S+)" % k, src).group(1) for k in ("VO_VOCAB_MIN_K", "VO_VOCAB_MAX_K", "VO_PLACES_MAX_ENTRIES", "VO_PLACES_MAX_TOP_K")}
    assert lim == {"VO_VOCAB_MIN_K": "256", "VO_VOCAB_MAX_K": "4096", "VO_PLACES_MAX_ENTRIES": "65536", "VO_PLACES_MAX_TOP_K": "16"}
    kern = open(os.path.join(ROOT, "visual_odometry_amd", "csrc", "reloc_kernels.hip")).read()
    assert re.search(r"#define\s+PL_MAX_K\s+4096", kern)
    # the quantiser calls the bodies the relocaliser has; they are stated once
    assert kern.count("void nn_map_l2_body(") == 1 and kern.count("void nn_map_hamming_body(") == 1
    assert kern.count("nn_map_l2_body(s_b") >= 5 and kern.count("nn_map_hamming_body(s_b") >= 5


def test_the_python_entries():
    from visual_odometry_amd import frontend
    FE = frontend.FrontEnd
    assert list(inspect.signature(FE.train_vocabulary).parameters) == ["self", "slots", "K", "iterations"]
    assert inspect.signature(FE.train_vocabulary).parameters["K"].default == 1024
    assert inspect.signature(FE.train_vocabulary).parameters["iterations"].default == 8
    assert list(inspect.signature(FE.places_query).parameters) == ["self", "entries", "top_k", "min_gap", "min_shared"]
    q = inspect.signature(FE.places_query).parameters
    assert (q["entries"].default, q["top_k"].default, q["min_gap"].default, q["min_shared"].default) == (None, 3, 0, 0)
    for name in ("set_vocabulary", "vocabulary", "words", "places_open", "places_add", "places_add_histograms", "places_entries"):
        assert callable(getattr(FE, name)), name
    res = dict(entry=[[1, -1], [0, 2], [1, -1]], id=[[11, 0], [10, 12], [11, 0]], shared=[[7, 0], [7, 5], [5, 0]])
    assert frontend.loop_candidates(res, [10, 11, 12]) == [(10, 11, 7), (11, 12, 5)]
