"""GPU: a stream's descriptor store (FrontEnd.stream_rows / map_from_stream; vo_set_stream_rows, vo_stream_rows_info,
vo_map_from_stream; k_stream_rows_append and k_stream_rows_select) against the rules of tests/stream_rows_reference.py and against
the parent's code path: slam_chain on the whole flight with every frame resident, then map_from_slam + map_rows.  Every comparison
is exact — rows are copied, never computed.

Sequence A of tests/test_gpu_slam_stream.py: synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4, 6 pairs,
evictions at pairs 3, 4 and 5; the stream runs on a FrontEnd with 4 slots (one more than a chunk's pairs where that is more), so
slots are reused and a frame's descriptors are gone from the slots when a later call's map is staged.  Each frame's descriptor rows
are recorded on the host when it is detected; the maps the reference's Store is fed are the device's own slam_map() lists.
tests/test_stream_rows_reference.py pins on the CPU that on every split a point that already has a row is moved by a later
eviction, and that the overflow capacity drops points that survive."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import stream_rows_reference as SR  # noqa: E402
import track_cases as TC  # noqa: E402
import relocalize_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
PER_PAIR = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
OUT_KEYS = PER_PAIR + ("poses_pnp", "poses", "carried_frame", "carried_poses")
DEAD_ROOT_NORM = 8.0


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _copy(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def _stage(fe, first=0, end=None):
    res = fe.map_from_stream(first, end)
    rows, pts = fe.map_rows()
    return dict(n=res["n"], without_row=res["without_row"], rows=rows, points=pts)


class Flight:
    """A flight of n frames given as put(fe, slot, frame) and the descriptor rows a frame has once it is in a slot."""

    def __init__(self, n, K, make_fe, put, chain_opts):
        self.n, self.K, self.make_fe, self.put, self.chain_opts = n, K, make_fe, put, chain_opts
        self.fes, self.whole_cache, self.desc = {}, {}, {}

    def fe(self, slots):
        if slots not in self.fes:
            self.fes[slots] = self.make_fe(slots)
        return self.fes[slots]

    def load(self, fe, slot, frame):
        self.put(fe, slot, frame)
        d = fe.features(slot)["desc"].astype(np.uint8)
        if frame in self.desc:
            assert np.array_equal(self.desc[frame], d), frame              # a frame's rows do not depend on its slot
        self.desc[frame] = d

    def picked(self, pt_feature):
        D = next(iter(self.desc.values())).shape[1]
        return np.stack([self.desc[int(f)][int(k)] for f, k in pt_feature]) if len(pt_feature) else np.zeros((0, D), np.uint8)

    def whole(self, **opts):
        """slam_chain on all pairs with every frame resident, then map_from_slam + map_rows: the parent's code path"""
        o = dict(self.chain_opts); o.update(opts)
        key = tuple(sorted(o.items()))
        if key not in self.whole_cache:
            fe = self.fe(self.n)
            for f in range(self.n):
                self.load(fe, f, f)
            fe.run_pairs([[k, k + 1] for k in range(self.n - 1)], self.K, want_points=True)
            out = fe.slam_chain(self.n - 1, self.K, **o)
            m = fe.slam_map(0)
            fe.map_from_slam(0)
            rows, pts = fe.map_rows()
            reloc = fe.relocalize([self.n - 1], self.K)
            self.whole_cache[key] = dict(out=_copy(out), map=m, rows=rows, points=pts, reloc=_copy(reloc), matches=fe.map_matches(0))
        return self.whole_cache[key]

    def stream(self, split, capacity=-1, stage=True, after_call=None, **opts):
        """slam_stream over the chunks of `split` with slot reuse; capacity None: the store off.  stage: map_from_stream() +
        map_rows() after every call.  after_call(fe, call index, call dict): what a test does between two calls.
        -> [dict(out, map, frame0, slots, info, staged)] per call"""
        o = dict(self.chain_opts); o.update(opts)
        n_slots = max(4, max(split) + 1)
        fe = self.fe(n_slots)
        fe.stream_rows(0 if capacity is None else capacity)
        free, slot_of, calls, at = list(range(n_slots)), {}, [], 0
        try:
            for c, n in enumerate(split):
                for f in range(at + (c > 0), at + n + 1):                 # the anchor stays where it is
                    slot_of[f] = free.pop(0)
                    self.load(fe, slot_of[f], f)
                fe.run_pairs([[slot_of[at + j], slot_of[at + j + 1]] for j in range(n)], self.K, want_points=True)
                out = fe.slam_stream(n, self.K, resume=c > 0, total_pairs=sum(split), **o)
                call = dict(out=_copy(out), map=fe.slam_map(0), frame0=at, slots=[slot_of[at + j] for j in range(n + 1)], info=None, staged=None)
                if capacity is not None:
                    call["info"] = fe.stream_rows_info()
                    if stage:
                        call["staged"] = _stage(fe)
                if after_call is not None:
                    after_call(fe, c, call)
                calls.append(call)
                for f in range(at, at + n):
                    free.append(slot_of.pop(f))
                free.sort()
                at += n
        finally:
            fe.stream_rows(0)
        return calls


def _orb_flight():
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")

    def put(fe, slot, frame):
        fe.upload(seq["frames"][frame][None], first_slot=slot); fe.detect(slot, 1)

    fl = Flight(N, seq["K"], lambda slots: FrontEnd(H, W, max_frames=slots, max_pairs=N - 1, nfeatures=NFEAT), put, dict(max_cameras=MAX_CAMERAS))
    fl.frames = seq["frames"]
    return fl


@pytest.fixture(scope="module")
def run():
    fl = _orb_flight()
    yield fl
    for fe in fl.fes.values():
        fe.ctx.close()


def _check_calls(fl, calls, capacity, kp_cap):
    """items 1 and 7: after every call the staged map is the reference's subset of the live map, with the recorded rows"""
    store = SR.Store(capacity, sum(len(c["out"]["status"]) for c in calls), kp_cap)
    for i, c in enumerate(calls):
        m, st = c["map"], c["staged"]
        store.append(m["pt_feature"], c["frame0"])
        assert c["info"] == store.info(), (i, c["info"], store.info())
        keep, rows, without = store.stage(m["pt_feature"])
        print("call", i, "map points", len(m["points"]), "staged", st["n"], "without a row", st["without_row"], c["info"])
        assert st["n"] == len(keep) == len(st["points"]) and st["without_row"] == without, i
        assert st["points"].tobytes() == np.ascontiguousarray(m["points"][keep]).tobytes(), i
        assert st["rows"].tobytes() == fl.picked(m["pt_feature"][keep]).tobytes(), i
    return store


# ------------------------------------------------------------------ 1, 2: every call, and the end against the chain
@pytest.mark.parametrize("split", SR.SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_the_live_map_is_staged_after_every_call_and_ends_as_the_chains(run, split):
    whole = run.whole()
    calls = run.stream(split)
    kp_cap = run.fe(max(4, max(split) + 1)).kp_cap
    store = _check_calls(run, calls, -1, kp_cap)
    for c in calls:
        assert c["staged"]["without_row"] == 0 and c["staged"]["n"] == len(c["map"]["points"]) > 0
        assert c["staged"]["points"].tobytes() == c["map"]["points"].tobytes()
        assert c["info"]["capacity"] == N * kp_cap and c["info"]["dropped"] == 0
    last = calls[-1]
    assert store.stored > len(last["map"]["points"])                      # the store has holes: rows of points that are gone
    _same(whole["map"], last["map"], S.MAP_KEYS, "final map")
    assert last["staged"]["rows"].tobytes() == whole["rows"].tobytes() and last["staged"]["points"].tobytes() == whole["points"].tobytes()
    used = [s for c in calls for s in c["slots"][1:]] + calls[0]["slots"][:1]
    assert len(used) == N and len(set(used)) < N                          # some slot held two frames of the flight


# ------------------------------------------------------------------ 3: the store changes nothing the stream returns
@pytest.mark.parametrize("split", SR.SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_store_on_is_store_off_byte_for_byte(run, split):
    off = run.stream(split, capacity=None)
    on = run.stream(split, stage=False)
    staged = run.stream(split)                                            # ... with a map_from_stream between every two calls
    windowed = run.stream(split, stage=False, after_call=lambda fe, c, call: fe.map_from_stream(1, 3))
    for a, b, s, w in zip(off, on, staged, windowed):
        assert a["info"] is None and b["info"] is not None
        for other in (b, s, w):
            _same(a["out"], other["out"], OUT_KEYS)
            _same(a["map"], other["map"], S.MAP_KEYS)
        assert b["info"] == s["info"] == w["info"]


# ------------------------------------------------------------------ 4: windows
def test_windows_are_the_host_filter_by_owning_frame(run):
    seen = {}

    def windows(fe, c, call):
        whole = _stage(fe)
        frame = call["map"]["pt_feature"][:, 0]
        assert whole["n"] == len(frame)
        for first, end in ((0, 2), (2, 5), (5, -1), (5, None), (3, 3), (0, 0), (7, 9), (0, 7)):
            got = _stage(fe, first, end)
            keep = (frame >= first) & ((frame < end) if end is not None and end >= 0 else True)
            assert got["n"] == int(keep.sum()) and got["without_row"] == 0, (c, first, end)
            assert got["rows"].tobytes() == whole["rows"][keep].tobytes() and got["points"].tobytes() == whole["points"][keep].tobytes(), (c, first, end)
            seen[(c, first, end)] = got["n"]
        assert _stage(fe)["rows"].tobytes() == whole["rows"].tobytes()    # an empty window, then the whole map again

    run.stream((2, 2, 2), stage=False, after_call=windows)
    print(seen)
    assert seen[(2, 0, 2)] > 0 and seen[(2, 2, 5)] > 0 and seen[(2, 5, -1)] > 0 and seen[(2, 3, 3)] == 0 and seen[(2, 7, 9)] == 0
    assert seen[(2, 0, 2)] + seen[(2, 2, 5)] + seen[(2, 5, -1)] == seen[(2, 0, 7)]
    assert seen[(0, 5, -1)] == 0 and seen[(0, 0, 2)] > 0                  # after the first call no frame past 2 owns a point


# ------------------------------------------------------------------ 5: the slots no longer matter
def test_staging_after_every_slot_but_the_anchors_was_overwritten(run):
    calls = run.stream((3, 3))
    fe = run.fe(4)
    fe.stream_rows(-1)                                                    # (a live stream keeps the setting it started with: this is not read)
    before = _stage(fe)
    assert before["rows"].tobytes() == calls[-1]["staged"]["rows"].tobytes()
    anchor = calls[-1]["slots"][-1]
    blank = np.full_like(run.frames[0], 127)
    for s in range(4):
        if s != anchor:
            old = fe.features(s)["desc"]
            fe.upload(run.frames[0][None], first_slot=s); fe.detect(s, 1)       # another frame's descriptors in the slot ...
            new = fe.features(s)["desc"]
            assert new.shape != old.shape or not np.array_equal(new, old)
            fe.upload(blank[None], first_slot=s); fe.detect(s, 1)                # ... then a blank frame
    after = _stage(fe)
    assert after["n"] == before["n"] and after["rows"].tobytes() == before["rows"].tobytes() and after["points"].tobytes() == before["points"].tobytes()
    assert fe.stream_rows_info() == calls[-1]["info"]
    fe.stream_rows(0)


# ------------------------------------------------------------------ 6: points whose key is none keep their rows
def test_a_dead_root_and_keyless_points_keep_their_rows(run):
    opts = dict(max_point_norm=DEAD_ROOT_NORM)
    whole = run.whole(**opts)
    assert whole["out"]["status"].tolist() == [0] * 6
    assert not np.array_equal(whole["out"]["n_pts"], run.whole()["out"]["n_pts"])   # the bound does skip something
    calls = run.stream((3, 3), **opts)
    _check_calls(run, calls, -1, run.fe(4).kp_cap)
    last = calls[-1]
    _same(whole["map"], last["map"], S.MAP_KEYS, "final map")
    # points of the first call that are neither in the anchor frame nor reached through it lose their key at the carry; frames 0 .. 2
    # left their slots before the second call
    old = int((last["map"]["pt_feature"][:, 0] < 3).sum())
    print("points of the last map owned by frames 0 .. 2:", old)
    assert old >= 1 and last["staged"]["without_row"] == 0
    assert last["staged"]["rows"].tobytes() == whole["rows"].tobytes() and last["staged"]["points"].tobytes() == whole["points"].tobytes()


# ------------------------------------------------------------------ 7: overflow
def test_a_full_store_drops_in_map_order_and_changes_nothing_else(run):
    split, cap = SR.OVERFLOW_SPLIT, SR.OVERFLOW_CAPACITY
    a = run.stream(split, capacity=cap)
    b = run.stream(split, capacity=cap)
    off = run.stream(split, capacity=None)
    store = _check_calls(run, a, cap, run.fe(4).kp_cap)
    assert a[0]["info"]["dropped"] == 0 and a[1]["info"]["stored"] == cap and a[1]["info"]["dropped"] >= 1      # it fills inside the second call
    assert a[2]["info"]["dropped"] > a[1]["info"]["dropped"] and a[2]["info"]["capacity"] == cap
    last = a[-1]
    assert last["staged"]["without_row"] >= 1 and last["staged"]["n"] >= 1                                       # a dropped point survives to the end
    assert last["staged"]["n"] + last["staged"]["without_row"] == len(last["map"]["points"])
    full = SR.Store(-1, N - 1, run.fe(4).kp_cap)
    for c in a:
        full.append(c["map"]["pt_feature"], c["frame0"])
    assert store.rows == full.rows[:cap]                                  # the first rows in map order
    for x, y, z in zip(a, b, off):
        _same(x["out"], z["out"], OUT_KEYS); _same(x["map"], z["map"], S.MAP_KEYS)
        assert x["info"] == y["info"] and x["staged"]["n"] == y["staged"]["n"] and x["staged"]["without_row"] == y["staged"]["without_row"]
        assert x["staged"]["rows"].tobytes() == y["staged"]["rows"].tobytes() and x["staged"]["points"].tobytes() == y["staged"]["points"].tobytes()


# ------------------------------------------------------------------ 8: the relocaliser on the stream-staged map
def test_relocalize_against_the_streams_map_is_relocalize_against_the_chains(run):
    whole = run.whole()
    got = {}

    def reloc(fe, c, call):
        if c == 1:
            fe.map_from_stream()
            got["out"] = _copy(fe.relocalize([call["slots"][-1]], run.K)); got["matches"] = fe.map_matches(0)

    run.stream((3, 3), stage=False, after_call=reloc)
    _same(whole["reloc"], got["out"], ("poses", "n_match", "n_inl", "status"))
    assert whole["reloc"]["status"][0] == 0 and whole["reloc"]["n_match"][0] > 0 and len(whole["matches"][0]) == whole["reloc"]["n_match"][0]
    for x, y in zip(whole["matches"], got["matches"]):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ------------------------------------------------------------------ 9: 128-byte rows
def test_sift_rows_split_3_3(oracle):
    """tests/test_gpu_relocalize.py's SIFT-like tracks on the seven frames of tracks_births (30 points throughout, 10 born in frame 2,
    8 in frame 4): one distinct 128-byte row per scene point, staged per slot through vo_stage_sift_rows."""
    from visual_odometry_amd.frontend import FrontEnd
    c = TC.cases()["tracks_births"]
    fr = TC.frames(oracle, c)
    table = RR.rand_rows(np.random.default_rng(31), len(c.X), "sift")
    assert c.n == 7 and len(np.unique(table, axis=0)) == len(table) and all((f["ids"] >= 0).all() for f in fr)

    def make(slots):
        fe = FrontEnd(32, 32, max_frames=slots, max_pairs=6, detector="sift", kp_cap=256)
        fe.ctx.set_poly_solver("opencv300")
        return fe

    fl = Flight(7, TC.K, make, lambda fe, slot, f: fe.set_sift_rows(slot, table[fr[f]["ids"]], fr[f]["xy"]), dict(ba_iterations=0, filter_threshold=1.0, max_cameras=4))
    try:
        whole = fl.whole()
        assert whole["out"]["status"].tolist() == [0] * 6 and whole["rows"].shape[1] == 128
        calls = fl.stream((3, 3))
        store = _check_calls(fl, calls, -1, fl.fe(4).kp_cap)
        assert all(np.array_equal(fl.desc[f], table[fr[f]["ids"]]) for f in range(7))
        last = calls[-1]
        _same(whole["map"], last["map"], S.MAP_KEYS, "final map")
        assert last["staged"]["without_row"] == 0 and last["staged"]["n"] == len(last["map"]["points"]) > 0
        assert last["staged"]["rows"].tobytes() == whole["rows"].tobytes() and last["staged"]["points"].tobytes() == whole["points"].tobytes()
        assert 0 < calls[0]["info"]["stored"] < store.stored and calls[1]["info"]["capacity"] == 7 * fl.fe(4).kp_cap   # frame 4's births come in the second call
    finally:
        for fe in fl.fes.values():
            fe.ctx.close()


# ------------------------------------------------------------------ 10: refusals and lifetimes
def test_refusals_and_lifetimes():
    import ctypes as C
    from visual_odometry_amd import _lib, synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(4, 640, 480, cache_dir="/tmp")
    K, frames = seq["K"], seq["frames"]
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500)
    lib, h = fe.ctx.lib, fe.ctx.handle
    try:
        fe.upload(frames); fe.detect(0, 4)

        def invalid(fn, *a):
            with pytest.raises(_lib.VoError) as e:
                fn(*a)
            assert e.value.code == _lib.VO_ERR_INVALID, e.value

        def start(n=2, total=3, entry=fe.slam_stream):
            fe.run_pairs([[k, k + 1] for k in range(n)], K, want_points=True)
            return entry(n, K, total_pairs=total)

        invalid(fe.stream_rows_info); invalid(fe.map_from_stream)        # no stream at all
        assert lib.vo_set_stream_rows(h, -2) == _lib.VO_ERR_INVALID and lib.vo_set_stream_rows(h, 0) == 0
        # the store off: today's refusal
        start()
        with pytest.raises(NotImplementedError):
            fe.map_from_slam(0)
        invalid(fe.stream_rows_info); invalid(fe.map_from_stream)
        # a setting changed mid-stream does not reach the live stream, in either direction
        fe.stream_rows(-1)
        invalid(fe.map_from_stream)
        fe.run_pairs([[2, 3]], K, want_points=True)
        assert fe.slam_stream(1, K, resume=True)["status"].tolist() == [0]
        invalid(fe.stream_rows_info)
        with pytest.raises(NotImplementedError):
            fe.map_from_slam(0)
        out = start()                                                     # ... a stream that starts now has one
        assert out["status"].tolist() == [0, 0]
        fe.stream_rows(0)
        info, first_map = fe.stream_rows_info(), fe.slam_map(0)
        assert info["capacity"] == 4 * fe.kp_cap and info["stored"] == len(fe.slam_map(0)["points"]) > 0 and info["dropped"] == 0
        a = _stage(fe)
        fe.map_from_slam(0)                                               # map_from_slam(0) is map_from_stream(0, -1)
        rows, pts = fe.map_rows()
        assert a["rows"].tobytes() == rows.tobytes() and a["points"].tobytes() == pts.tobytes() and a["n"] == info["stored"]
        with pytest.raises(NotImplementedError):
            fe.map_from_slam(1)                                           # the snapshot stays refused
        # bad windows are refused, and a refused call leaves no staged map
        n, w = C.c_int32(7), C.c_int32(7)
        for first, end in ((-1, 2), (2, 1), (3, 0), (-5, -1)):
            fe.map_from_stream()
            assert lib.vo_map_from_stream(h, first, end, C.addressof(n), C.addressof(w)) == _lib.VO_ERR_INVALID, (first, end)
            invalid(fe.map_rows)
        assert lib.vo_map_from_stream(h, 0, -1, None, C.addressof(w)) == _lib.VO_ERR_INVALID
        assert fe.map_from_stream(2, 2) == dict(n=0, without_row=0) and len(fe.map_rows()[0]) == 0     # an empty window stages an empty map
        fe.run_pairs([[2, 3]], K, want_points=True)
        assert fe.slam_stream(1, K, resume=True)["status"].tolist() == [0]                            # the stream goes on, the store with it
        ref = SR.Store(-1, 3, fe.kp_cap)
        ref.append(first_map["pt_feature"], 0); ref.append(fe.slam_map(0)["pt_feature"], 2)
        assert fe.stream_rows_info() == ref.info()
        assert _stage(fe)["points"].tobytes() == fe.slam_map(0)["points"].tobytes()
        # slam_chain releases the stream and its store
        fe.run_pairs([[0, 1]], K, want_points=True)
        assert fe.slam_chain(1, K)["status"].tolist() == [0]
        invalid(fe.stream_rows_info); invalid(fe.map_from_stream)
        fe.map_from_slam(0)                                               # (the chain's own map is staged as ever)
        # the restart stream and the multi-stream ignore the setting: no store, their maps stay refused
        fe.stream_rows(-1)
        start(entry=fe.slam_stream_restart)
        invalid(fe.stream_rows_info); invalid(fe.map_from_stream)
        with pytest.raises(NotImplementedError):
            fe.map_from_slam(0)
        fe.run_pairs([[0, 1], [2, 3]], K, want_points=True)
        fe.slam_streams([1, 1], K)
        invalid(fe.stream_rows_info); invalid(fe.map_from_stream)
        with pytest.raises(NotImplementedError):
            fe.map_from_slam(0)
        # a capacity the stream cannot index
        assert lib.vo_set_stream_rows(h, 2 ** 31) == 0
        fe.run_pairs([[0, 1]], K, want_points=True)
        invalid(fe.slam_stream, 1, K)
        fe.stream_rows(0)
    finally:
        fe.ctx.close()
