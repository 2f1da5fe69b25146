"""No GPU: vo_slam_streams as include/vo_hip.h declares it is what visual_odometry_amd/_lib.py binds — argument for argument, by
count and by kind (a pointer, or an int passed by value) — and FrontEnd.slam_streams takes slam_stream_restart's options."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared in include/vo_hip.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append((a.split()[-1].lstrip("*"), "pointer" if "*" in a else a.rsplit(" ", 1)[0]))
    return out


def test_the_prototype_matches_the_binding():
    from visual_odometry_amd import _lib
    declared = _declared("vo_slam_streams")
    restype, argtypes = _lib._SIGS["vo_slam_streams"]
    assert restype is C.c_int and len(argtypes) == len(declared) == 26
    for (name, kind), t in zip(declared, argtypes):
        assert kind in ("pointer", "int"), (name, kind)
        assert t is (C.c_void_p if kind == "pointer" else C.c_int), (name, kind, t)
    names = [n for n, _ in declared]
    assert names[:8] == ["ctx", "resume", "S", "total_pairs", "seq_off", "K", "opts", "snapshot_seq"]
    assert [k for _, k in declared[:8]] == ["pointer", "int", "int", "pointer", "pointer", "pointer", "pointer", "int"]
    # then vo_slam_chains_restart's outputs in its order, then vo_slam_stream_restart's carried rows
    chains = [n for n, _ in _declared("vo_slam_chains_restart")]
    assert names[8:23] == chains[6:] and names[19:23] == ["segment", "cause", "seg_poses_pnp", "seg_poses"]
    assert names[23:] == [n for n, _ in _declared("vo_slam_stream_restart")][17:20] == ["n_carried", "carried_frame", "carried_poses"]


def test_the_method_takes_the_streams_options():
    from visual_odometry_amd import frontend
    from visual_odometry_amd.frontend import FrontEnd
    multi = list(inspect.signature(FrontEnd.slam_streams).parameters)
    single = list(inspect.signature(FrontEnd.slam_stream_restart).parameters)
    assert multi[1] == "seq_lengths" and multi[2:] == single[2:]
    assert callable(frontend.stream_slice) and callable(frontend.join_streams)
