"""No GPU: vo_slam_streams_open and vo_slam_streams_replace as include/vo_hip.h declares them are what visual_odometry_amd/_lib.py
binds — argument for argument, by count and by kind (a pointer, or an int passed by value) — vo_slam_streams is the entry it was,
and the FrontEnd methods take slam_streams' options."""
import ctypes as C
import inspect
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_slam_streams_abi import _declared  # noqa: E402


def _matches(name, names, kinds):
    from visual_odometry_amd import _lib
    declared = _declared(name)
    restype, argtypes = _lib._SIGS[name]
    assert restype is C.c_int and len(argtypes) == len(declared) == len(names)
    for (arg, kind), t in zip(declared, argtypes):
        assert kind in ("pointer", "int"), (arg, kind)
        assert t is (C.c_void_p if kind == "pointer" else C.c_int), (arg, kind, t)
    assert [n for n, _ in declared] == names and [k for _, k in declared] == kinds


def test_the_prototypes_match_the_bindings():
    _matches("vo_slam_streams_open", ["ctx", "S", "total_pairs", "K", "opts"], ["pointer", "int", "pointer", "pointer", "pointer"])
    _matches("vo_slam_streams_replace", ["ctx", "seq", "total_pairs"], ["pointer", "int", "int"])


def test_vo_slam_streams_is_the_entry_it_was():
    from visual_odometry_amd import _lib
    declared = _declared("vo_slam_streams")
    assert len(declared) == len(_lib._SIGS["vo_slam_streams"][1]) == 26
    assert [n for n, _ in declared][:8] == ["ctx", "resume", "S", "total_pairs", "seq_off", "K", "opts", "snapshot_seq"]
    assert [n for n, _ in declared][23:] == ["n_carried", "carried_frame", "carried_poses"]


def test_the_library_exports_the_entries():
    from visual_odometry_amd import _lib
    assert {"vo_slam_streams_open", "vo_slam_streams_replace"} <= set(_lib.exported_symbols())
    lib = _lib.load()                                                           # (loading the library needs no GPU)
    assert lib.vo_slam_streams_replace(None, 0, 1) == _lib.VO_ERR_INVALID       # no context: refused before anything is touched


def test_the_methods_take_the_streams_options():
    from visual_odometry_amd import flight_pool, frontend
    from visual_odometry_amd.frontend import FrontEnd
    opened = list(inspect.signature(FrontEnd.slam_streams_open).parameters)
    multi = list(inspect.signature(FrontEnd.slam_streams).parameters)
    assert opened[:4] == ["self", "n_seats", "total_pairs", "K"]
    assert opened[4:] == [p for p in multi[3:] if p not in ("resume", "total_pairs")]
    assert list(inspect.signature(FrontEnd.slam_streams_replace).parameters) == ["self", "seq", "total_pairs"]
    assert list(inspect.signature(frontend.split_flights).parameters) == ["outs", "took_seat"]
    assert list(inspect.signature(flight_pool.plan_calls).parameters) == ["lengths", "n_seats", "chunk", "n_slots"]
    assert list(inspect.signature(flight_pool.FlightPool.__init__).parameters) == ["self", "fe", "K", "n_seats", "chunk", "capacity", "options"]
