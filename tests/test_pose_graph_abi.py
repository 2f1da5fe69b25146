"""No GPU: vo_pose_graph_batch and vo_pose_graph as include/vo_hip.h declares them are what visual_odometry_amd/_lib.py binds —
argument for argument, by count and by kind (a pointer or array, or an int passed by value); vo_pgo_opts is PgoOpts field for field;
the stage count stays 30 (the kernel is bracketed under misc); the g2o surface got no Sim(3) names."""
import ctypes as C
import inspect
import os
import re

import pytest

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
    _check("vo_pose_graph_batch", ["ctx", "B", "vert_off", "edge_off", "sims", "fixed", "edges", "meas", "info", "opts", "chi2", "iterations_run",
                                   "trials_run", "status"], ["pointer", "int"] + ["pointer"] * 12)
    _check("vo_pose_graph", ["ctx", "sims", "fixed", "nv", "edges", "meas", "info", "ne", "opts", "chi2", "iterations_run", "trials_run"],
           ["pointer", "pointer", "pointer", "int", "pointer", "pointer", "pointer", "int", "pointer", "pointer", "pointer", "pointer"])


def test_the_options_the_limits_and_the_stage_count():
    from visual_odometry_amd import _lib
    h = _header()
    m = re.search(r"typedef struct \{([^}]*)\} vo_pgo_opts;", h)
    fields = [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", m.group(1)).split(";") if f.strip()]
    assert fields == ["int32_t iterations", "double huber_delta"]
    assert [(n, t) for n, t in _lib.PgoOpts._fields_] == [("iterations", C.c_int32), ("huber_delta", C.c_double)]
    assert C.sizeof(_lib.PgoOpts) == 16 and _lib.PgoOpts.huber_delta.offset == 8
    assert int(re.search(r"#define\s+VO_PGO_MAX_VERTICES\s+(\d+)", h).group(1)) == _lib.VO_PGO_MAX_VERTICES == 8192
    assert int(re.search(r"#define\s+VO_PGO_MAX_LOOPS\s+(\d+)", h).group(1)) == _lib.VO_PGO_MAX_LOOPS == 32
    assert int(re.search(r"#define\s+VO_STAGE_COUNT\s+(\d+)", h).group(1)) == _lib.VO_STAGE_COUNT == 30
    block = h[h.index("pose graph: Sim(3)"):h.index("int vo_pose_graph_batch")]
    for phrase in ("rotation, translation, log-scale", "th >= 1e-2", "|sigma| <  1e-2", "n = 1e-8", "Ad(S)", "without g2o's + 1e-3", "at most 10 trials",
                   "VO_ERR_UNSUPPORTED", "not connected to a fixed vertex", "the same bytes", "Out of scope"):
        assert phrase in block, phrase
    align = h[h.index("map alignment: the similarity"):h.index("} vo_align_opts;")]
    assert "pose-graph or bundle refinement" not in align and "vo_pose_graph" in align


def test_the_thresholds_are_the_same_everywhere():
    import pose_graph_reference as P
    from visual_odometry_amd import frontend
    src = open(os.path.join(ROOT, "visual_odometry_amd", "csrc", "pgo_kernels.hip")).read()
    dev = {k: float(re.search(r"#define\s+%s\s+(\S+)" % k, src).group(1)) for k in ("PGO_TH_W", "PGO_TH_S", "PGO_TH_LOG")}
    assert (dev["PGO_TH_W"], dev["PGO_TH_S"], dev["PGO_TH_LOG"]) == (P.TH_W, P.TH_S, P.TH_LOG) == (1e-2, 1e-2, 1e-8)
    assert (frontend.SIM3_TH_W, frontend.SIM3_TH_S, frontend.SIM3_TH_LOG) == (P.TH_W, P.TH_S, P.TH_LOG)
    assert (P.MAX_VERTICES, P.MAX_LOOPS) == (8192, 32)


def test_the_python_entries():
    from visual_odometry_amd import frontend, g2o_surface, map_filters
    assert list(inspect.signature(map_filters.optimize_pose_graph).parameters) == ["sims", "fixed", "edges", "meas", "info", "iterations", "huber_delta", "ctx"]
    assert list(inspect.signature(map_filters.optimize_pose_graph_batch).parameters) == ["problems", "iterations", "huber_delta", "ctx"]
    assert inspect.signature(map_filters.optimize_pose_graph).parameters["iterations"].default == 10
    for name in ("sim3_exp", "sim3_log", "sim3_inverse", "sim3_compose", "track_vertices", "odometry_edges", "loop_edge", "vertices_to_poses", "correct_points"):
        assert callable(getattr(frontend, name)), name
    with pytest.raises(Exception):
        g2o_surface.VertexSim3Expmap
