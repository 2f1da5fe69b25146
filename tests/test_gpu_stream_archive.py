"""GPU: a stream's archive of evicted points (FrontEnd.stream_archive / stream_archive_points / map_from_stream_archive;
vo_set_stream_archive, vo_stream_archive_info, vo_stream_archive_read, vo_map_from_stream_archive; k_slam_limit_stream_archive,
k_stream_archive_count / _emit, k_map_gather_from) against the rules of tests/stream_archive_reference.py.  Every comparison is
exact: coordinates and rows are copied, never computed.

The yardstick is the parent's code path, never the archive itself: slam_chain on all seven frames resident with snapshot=(p, 3)
for p = 3, 4, 5 gives the map as it stands before each evicting limit; the removal rule is applied to those lists on the host.
The store the reference needs is fed the maps of a stream that runs WITHOUT an archive.  Rows are the descriptors recorded on the
host when a frame is detected.

Sequence A of tests/test_gpu_slam_stream.py: synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4, 6 pairs,
evictions at pairs 3, 4 and 5 of about 200 points each out of about 1040 (tests/test_stream_archive_reference.py pins the CPU walk's
201 + 224 + 224 = 649 and that each crosses a 256-point round of the limit's scan); the 649 entries span three tiles of the
selection and three of its workgroups.  The stream runs on a FrontEnd with 4 slots where a chunk allows (slots are reused)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import stream_rows_reference as SR  # noqa: E402
import stream_archive_reference as AR  # noqa: E402
import track_cases as TC  # noqa: E402
import relocalize_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
PER_PAIR = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
OUT_KEYS = PER_PAIR + ("poses_pnp", "poses", "carried_frame", "carried_poses")
ARC_KEYS = ("feature", "xyz", "evicted_at", "has_row", "rows")
WINDOWS = ((0, 1), (1, 2), (0, 3), (1, 3), (3, 3), (0, None))


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def _copy(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


class Flight:
    """A flight of n frames given as put(fe, slot, frame) and the descriptor rows a frame has once it is in a slot (the pattern of
    tests/test_gpu_stream_rows.py, restated)."""

    def __init__(self, n, K, make_fe, put, chain_opts, evicting):
        self.n, self.K, self.make_fe, self.put, self.chain_opts, self.evicting = n, K, make_fe, put, chain_opts, evicting
        self.fes, self.desc, self.stage3_cache, self.cache = {}, {}, None, {}

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

    def picked(self, feature):
        D = next(iter(self.desc.values())).shape[1]
        return np.stack([self.desc[int(f)][int(k)] for f, k in feature]) if len(feature) else np.zeros((0, D), np.uint8)

    def stage3(self):
        """{p: the map before pair p's limit} for the evicting pairs, from slam_chain with every frame resident: the parent's path"""
        if self.stage3_cache is None:
            fe = self.fe(self.n)
            for f in range(self.n):
                self.load(fe, f, f)
            fe.run_pairs([[k, k + 1] for k in range(self.n - 1)], self.K, want_points=True)
            maps = {}
            for p in self.evicting:
                out = fe.slam_chain(self.n - 1, self.K, snapshot=(p, 3), **self.chain_opts)
                assert out["status"].tolist() == [0] * (self.n - 1)
                maps[p] = fe.slam_map(1)
                assert len(maps[p]["cam_frame"]) > self.chain_opts["max_cameras"], p          # the limit of pair p does evict
            ncam = out["n_cam"].tolist()                                  # ... and no other pair's does
            assert [p for p in range(self.n - 1) if (2 if p == 0 else ncam[p - 1] + 1) > self.chain_opts["max_cameras"]] == list(self.evicting)
            self.stage3_cache = maps
        return self.stage3_cache

    def stream(self, split, archive=-1, capacity=-1, after_call=None, n_slots=None):
        """slam_stream over the chunks of `split`; archive None: off.  after_call(fe, call index, call dict).
        -> [dict(out, map, frame0, slots, info, ainfo)] per call"""
        n_slots = n_slots or max(4, max(split) + 1)
        fe = self.fe(n_slots)
        fe.stream_rows(capacity); fe.stream_archive(0 if archive is None else archive)
        free, slot_of, calls, at = list(range(n_slots)), {}, [], 0
        try:
            for c, n in enumerate(split):
                for f in range(at + (c > 0), at + n + 1):                 # the anchor stays where it is
                    slot_of[f] = free.pop(0)
                    self.load(fe, slot_of[f], f)
                fe.run_pairs([[slot_of[at + j], slot_of[at + j + 1]] for j in range(n)], self.K, want_points=True)
                out = fe.slam_stream(n, self.K, resume=c > 0, total_pairs=sum(split), **self.chain_opts)
                call = dict(out=_copy(out), map=fe.slam_map(0), frame0=at, slots=[slot_of[at + j] for j in range(n + 1)],
                            info=fe.stream_rows_info(), ainfo=None if archive is None else fe.stream_archive_info())
                if after_call is not None:
                    after_call(fe, c, call)
                calls.append(call)
                for f in range(at, at + n):
                    free.append(slot_of.pop(f))
                free.sort()
                at += n
        finally:
            fe.stream_rows(0); fe.stream_archive(0)
        return calls

    def off(self, split, capacity=-1):
        """the stream without an archive (cached): the parent's path, and what the reference's Store is fed"""
        key = ("off", split, capacity)
        if key not in self.cache:
            got = {}

            def stage(fe, c, call):
                fe.map_from_stream()
                got[c] = fe.map_rows()

            calls = self.stream(split, archive=None, capacity=capacity, after_call=stage)
            for c, call in enumerate(calls):
                call["staged"] = got[c]
            self.cache[key] = calls
        return self.cache[key]

    def reference(self, split, archive=-1, capacity=-1):
        """-> (Store, Archive, [archive info per call]) by the rules, from the parent's maps"""
        off = self.off(split, capacity)
        kp_cap = self.fe(max(4, max(split) + 1)).kp_cap
        end_maps = [dict(frame0=c["frame0"], pt_feature=c["map"]["pt_feature"]) for c in off]
        return AR.run_split(split, self.stage3(), end_maps, archive, sum(split), kp_cap, store_capacity=capacity)


def _orb_flight():
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")

    def put(fe, slot, frame):
        fe.upload(seq["frames"][frame][None], first_slot=slot); fe.detect(slot, 1)

    fl = Flight(N, seq["K"], lambda slots: FrontEnd(H, W, max_frames=slots, max_pairs=N - 1, nfeatures=NFEAT), put, dict(max_cameras=MAX_CAMERAS), (3, 4, 5))
    fl.frames = seq["frames"]
    return fl


@pytest.fixture(scope="module")
def run():
    fl = _orb_flight()
    yield fl
    for fe in fl.fes.values():
        fe.ctx.close()


def _check_entries(fl, got, ref, what=""):
    """the device's entries against the reference Archive: everything but the rows by value, the rows as recorded at detection"""
    a = ref.arrays()
    assert got["feature"].tobytes() == a["feature"].tobytes() and got["xyz"].tobytes() == a["xyz"].tobytes(), what
    assert got["evicted_at"].tobytes() == a["evicted_at"].tobytes() and np.array_equal(got["has_row"], a["has_row"]), what
    want = fl.picked(a["feature"])
    want[~a["has_row"]] = 0
    assert got["rows"].tobytes() == want.tobytes(), what


# ------------------------------------------------------------------ 1: the entries, for every split
@pytest.mark.parametrize("split", AR.SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_the_entries_are_the_points_the_limit_removed_whatever_the_split(run, split):
    store, ref, infos = run.reference(split)
    got = {}

    def read(fe, c, call):
        got[c] = fe.stream_archive_points()

    calls = run.stream(split, after_call=read)
    for c, (call, info) in enumerate(zip(calls, infos)):
        print("split", split, "call", c, call["ainfo"])
        assert call["ainfo"] == info, (c, call["ainfo"], info)
        assert len(got[c]["feature"]) == info["stored"]
        _same({k: v[:len(got[c][k])] for k, v in got[len(calls) - 1].items()}, got[c], ARC_KEYS, "an entry never changes")
    last = got[len(calls) - 1]
    _check_entries(run, last, ref, split)
    assert ref.stored == sum(len(AR.removed_points(m["obs_cam"], m["obs_pt"], len(m["points"]))) for m in run.stage3().values()) > 3 * 256 // 2
    assert last["has_row"].all() and ref.dropped == 0                    # every entry has its row, whatever the chunking
    assert sorted(set(last["evicted_at"].tolist())) == [3, 4, 5] and (np.diff(last["evicted_at"]) >= 0).all()
    first = run.cache.setdefault("entries", last)                         # the bytes are the same for every split
    _same(first, last, ARC_KEYS, "split")
    # part reads
    fe = run.fe(max(4, max(split) + 1))
    part = fe.stream_archive_points(250, 20)
    _same({k: v[250:270] for k, v in last.items()}, part, ARC_KEYS, "part")
    assert len(fe.stream_archive_points(ref.stored)["feature"]) == 0


# ------------------------------------------------------------------ 2: the archive changes nothing the stream returns or keeps
@pytest.mark.parametrize("split", AR.SPLITS, ids=lambda s: "+".join(map(str, s)))
def test_archive_on_is_archive_off_byte_for_byte(run, split):
    off = run.off(split)
    got = {}

    def stage(fe, c, call):
        fe.map_from_stream()
        got[c] = fe.map_rows()

    def stage_archive_first(fe, c, call):
        fe.map_from_stream_archive(0, 2, live=True); fe.map_from_stream_archive(1, None, live=False)
        stage(fe, c, call)

    for after in (stage, stage_archive_first, None):
        got.clear()
        on = run.stream(split, after_call=after)
        for c, (a, b) in enumerate(zip(off, on)):
            _same(a["out"], b["out"], OUT_KEYS, c); _same(a["map"], b["map"], S.MAP_KEYS, c)
            assert a["info"] == b["info"] and a["ainfo"] is None and b["ainfo"] is not None
            if after is not None:                                         # the store's staged bytes
                assert a["staged"][0].tobytes() == got[c][0].tobytes() and a["staged"][1].tobytes() == got[c][1].tobytes(), c


# ------------------------------------------------------------------ 3: staging
def _staged(fe, first, end, live):
    res = fe.map_from_stream_archive(first, end, live=live)
    rows, pts = fe.map_rows()
    return res, rows, pts


def _reloc(fe, slot, K):
    out = _copy(fe.relocalize([slot], K))
    return out, fe.map_matches(0)


@pytest.mark.parametrize("split", [(2, 2, 2), (5, 1)], ids=lambda s: "+".join(map(str, s)))
def test_windows_alone_and_behind_the_live_points(run, split):
    store, ref, _ = run.reference(split)
    seen = {}

    def windows(fe, c, call):
        if c != len(split) - 1:
            return
        m, anchor = call["map"], call["slots"][-1]
        for first, end in WINDOWS:
            for live in (True, False):
                want = AR.stage(store, ref, m["pt_feature"], m["points"], first, end, live=live)
                res, rows, pts = _staged(fe, first, end, live)
                assert res == dict(n=want["n"], n_archived=want["n_archived"], without_row=want["without_row"]), (first, end, live, res)
                assert rows.tobytes() == run.picked(want["feature"]).tobytes() and pts.tobytes() == want["points"].tobytes(), (first, end, live)
                seen[(first, end, live)] = (res["n"], res["n_archived"])
                if live:                                                  # the live part is map_from_stream's, byte for byte
                    n_live = fe.map_from_stream(first, end)["n"]
                    lrows, lpts = fe.map_rows()
                    assert n_live == res["n"] - res["n_archived"] and rows[:n_live].tobytes() == lrows.tobytes() and pts[:n_live].tobytes() == lpts.tobytes()
                    fe.map_from_stream_archive(first, end, live=True)
                # the relocaliser and its match list on it are what they are on the same arrays staged from the host
                a = _reloc(fe, anchor, run.K)
                fe.stage_map(rows, pts)
                b = _reloc(fe, anchor, run.K)
                _same(a[0], b[0], ("poses", "n_match", "n_inl", "status"), (first, end, live))
                for x, y in zip(a[1], b[1]):
                    assert x.dtype == y.dtype and np.array_equal(x, y), (first, end, live)
        # staging again after every slot but the anchor's was overwritten gives the same bytes
        before = _staged(fe, 0, None, True)
        blank = np.full_like(run.frames[0], 127)
        for s in range(fe.max_frames):
            if s != anchor:
                fe.upload(blank[None], first_slot=s); fe.detect(s, 1)
        after = _staged(fe, 0, None, True)
        assert before[0] == after[0] and before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
        assert fe.stream_archive_info() == call["ainfo"]

    run.stream(split, after_call=windows)
    print(seen)
    total = ref.stored
    assert seen[(0, None, False)] == (total, total) and seen[(0, 3, False)] == (total, total)      # the archived points are owned by frames 0 .. 2
    assert seen[(0, 1, False)][0] + seen[(1, 3, False)][0] == total and seen[(1, 2, False)][0] > 0 and seen[(3, 3, True)] == (0, 0)
    assert seen[(0, None, True)][0] > total and seen[(0, None, True)][1] == total


# ------------------------------------------------------------------ 4: a full archive
def test_a_full_archive_keeps_the_first_entries_and_counts_the_rest(run):
    split = (2, 2, 2)
    n = {p: len(AR.removed_points(m["obs_cam"], m["obs_pt"], len(m["points"]))) for p, m in run.stage3().items()}
    cap = n[3] + n[4] // 2 - 1                                            # smaller than the first eviction plus half the second
    store, ref, infos = run.reference(split, archive=cap)
    full = run.reference(split)[1]
    got = []
    for _ in range(2):
        pts = {}
        calls = run.stream(split, archive=cap, after_call=lambda fe, c, call: pts.update({c: (fe.stream_archive_points(), fe.map_from_stream_archive(0, None, live=False))}))
        assert [c["ainfo"] for c in calls] == infos
        got.append(pts[2])
    last, res = got[0]
    print("capacity", cap, "evictions", n, calls[-1]["ainfo"])
    assert calls[-1]["ainfo"] == dict(capacity=cap, stored=cap, dropped=sum(n.values()) - cap)
    assert calls[0]["ainfo"]["stored"] == 0 and calls[1]["ainfo"] == dict(capacity=cap, stored=n[3], dropped=0)   # it fills inside pair 4's eviction
    _check_entries(run, last, ref)
    fa = full.arrays()
    assert last["feature"].tobytes() == fa["feature"][:cap].tobytes() and last["xyz"].tobytes() == fa["xyz"][:cap].tobytes()
    assert res == dict(n=cap, n_archived=cap, without_row=0)
    _same(got[0][0], got[1][0], ARC_KEYS, "two runs")
    off = run.off(split)
    for a, b in zip(off, calls):
        _same(a["out"], b["out"], OUT_KEYS); _same(a["map"], b["map"], S.MAP_KEYS)


# ------------------------------------------------------------------ 5: a store that overflowed
@pytest.mark.parametrize("store_capacity", sorted(AR.STORE_OVERFLOW_WITHOUT_ROW))
def test_entries_the_store_dropped_have_no_row(run, store_capacity):
    split = SR.OVERFLOW_SPLIT
    store, ref, infos = run.reference(split, capacity=store_capacity)
    got = {}

    def read(fe, c, call):
        if c == len(split) - 1:
            got["points"] = fe.stream_archive_points()
            got["alone"] = _staged(fe, 0, None, False)
            got["live"] = _staged(fe, 0, None, True)
            got["map"] = call["map"]

    calls = run.stream(split, capacity=store_capacity, after_call=read)
    assert [c["ainfo"] for c in calls] == infos and calls[-1]["info"] == store.info() and store.dropped > 0
    _check_entries(run, got["points"], ref)
    without = int((~got["points"]["has_row"]).sum())
    print("store", store.info(), "entries without a row", without, "of", ref.stored)
    assert without == AR.STORE_OVERFLOW_WITHOUT_ROW[store_capacity]      # the CPU walk's count (the entries themselves: the reference on the device's own maps)
    for live in (False, True):
        want = AR.stage(store, ref, got["map"]["pt_feature"], got["map"]["points"], 0, None, live=live)
        res, rows, pts = got["live" if live else "alone"]
        assert res == dict(n=want["n"], n_archived=want["n_archived"], without_row=want["without_row"]), (live, res)
        assert rows.tobytes() == run.picked(want["feature"]).tobytes() and pts.tobytes() == want["points"].tobytes()
    assert got["alone"][0]["without_row"] == without and got["alone"][0]["n"] == ref.stored - without


# ------------------------------------------------------------------ 6: 128-byte rows
def test_sift_rows_split_2_4(oracle):
    """tests/track_cases.py's `eviction` scene (7 frames, max_cameras = 3, no bundle adjustment: the limits of pairs 2 and 5 remove 8
    points each, owned by frame 0 and by frame 3) with one distinct 128-byte row per scene point, staged per slot through
    vo_stage_sift_rows.  Split (2, 4): the entries of pair 2 take their rows from the store (frame 0 left with the first call), those
    of pair 5 from the slots."""
    from visual_odometry_amd.frontend import FrontEnd
    c = TC.cases()["eviction"]
    fr = TC.frames(oracle, c)
    table = RR.rand_rows(np.random.default_rng(37), len(c.X), "sift")
    assert c.n == 7 and len(np.unique(table, axis=0)) == len(table) and all((f["ids"] >= 0).all() for f in fr)

    def make(slots):
        fe = FrontEnd(32, 32, max_frames=slots, max_pairs=6, detector="sift", kp_cap=256)
        fe.ctx.set_poly_solver("opencv300")
        return fe

    fl = Flight(7, TC.K, make, lambda fe, slot, f: fe.set_sift_rows(slot, table[fr[f]["ids"]], fr[f]["xy"]), dict(c.opts), (2, 3, 4, 5))
    try:
        split = (2, 4)
        store, ref, infos = fl.reference(split)
        got = {}

        def read(fe, k, call):
            if k == 1:
                got["points"] = fe.stream_archive_points()
                got["map"] = call["map"]
                for live in (True, False):
                    res = fe.map_from_stream_archive(0, None, live=live)
                    got[live] = (res,) + fe.map_rows()
                    a = _reloc(fe, call["slots"][-1], TC.K)
                    fe.stage_map(got[live][1], got[live][2])
                    b = _reloc(fe, call["slots"][-1], TC.K)
                    _same(a[0], b[0], ("poses", "n_match", "n_inl", "status"), live)
                    for x, y in zip(a[1], b[1]):
                        assert x.dtype == y.dtype and np.array_equal(x, y), live

        calls = fl.stream(split, after_call=read, n_slots=5)
        assert [k["ainfo"] for k in calls] == infos
        print("entries", ref.stored, ref.arrays()["feature"].tolist(), ref.evicted_at)
        assert got["points"]["rows"].shape[1] == 128 and ref.stored == 16 and all(ref.has_row)
        assert ref.arrays()["feature"][:, 0].tolist() == [0] * 8 + [3] * 8 and ref.evicted_at == [2] * 8 + [5] * 8
        _check_entries(fl, got["points"], ref)
        for live in (True, False):
            want = AR.stage(store, ref, got["map"]["pt_feature"], got["map"]["points"], 0, None, live=live)
            res, rows, pts = got[live]
            assert res == dict(n=want["n"], n_archived=16, without_row=0)
            assert rows.tobytes() == fl.picked(want["feature"]).tobytes() and pts.tobytes() == want["points"].tobytes()
        off = fl.off(split)
        for a, b in zip(off, calls):
            _same(a["out"], b["out"], OUT_KEYS); _same(a["map"], b["map"], S.MAP_KEYS)
    finally:
        for fe in fl.fes.values():
            fe.ctx.close()


# ------------------------------------------------------------------ 7: refusals and lifetimes
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

        def invalid(fn, *a, **k):
            with pytest.raises(_lib.VoError) as e:
                fn(*a, **k)
            assert e.value.code == _lib.VO_ERR_INVALID, e.value

        def start(n=2, total=3, entry=fe.slam_stream, **o):
            fe.run_pairs([[k, k + 1] for k in range(n)], K, want_points=True)
            return entry(n, K, total_pairs=total, **o)

        def no_archive():
            invalid(fe.stream_archive_info); invalid(fe.stream_archive_points, 0, 0); invalid(fe.map_from_stream_archive)
            invalid(fe.map_from_stream_archive, 0, None, live=False)

        no_archive()                                                      # no stream at all
        assert lib.vo_set_stream_archive(h, -2) == _lib.VO_ERR_INVALID and lib.vo_set_stream_archive(h, 0) == 0
        # an archive without the store: refused, and nothing is started
        fe.stream_archive(-1)
        fe.run_pairs([[0, 1], [1, 2]], K, want_points=True)
        invalid(fe.slam_stream, 2, K, total_pairs=3)
        invalid(fe.slam_map, 0); no_archive()
        invalid(fe.slam_stream, 1, K, resume=True)                        # there is no stream to continue
        # a stream with a store and no archive: archived staging is refused, the store's works
        fe.stream_archive(0); fe.stream_rows(-1)
        start()
        no_archive()
        assert fe.map_from_stream()["n"] > 0
        # a setting changed mid-stream has no effect, in either direction
        fe.stream_archive(-1)
        fe.run_pairs([[2, 3]], K, want_points=True)
        assert fe.slam_stream(1, K, resume=True)["status"].tolist() == [0]
        no_archive()
        out = start(max_cameras=2)                                        # a stream that starts now has one; pair 1 evicts
        assert out["status"].tolist() == [0, 0] and out["n_cam"].tolist() == [2, 2]
        fe.stream_archive(0)
        info = fe.stream_archive_info()
        assert info["capacity"] == 4 * fe.kp_cap and info["stored"] > 0 and info["dropped"] == 0
        pts = fe.stream_archive_points()
        assert len(pts["feature"]) == info["stored"] and pts["has_row"].all() and set(pts["evicted_at"].tolist()) == {1}
        fe.run_pairs([[2, 3]], K, want_points=True)
        assert fe.slam_stream(1, K, resume=True, max_cameras=2)["status"].tolist() == [0]           # the stream goes on, the archive with it
        more = fe.stream_archive_info()
        assert more["stored"] > info["stored"]
        _same({k: v[:info["stored"]] for k, v in fe.stream_archive_points().items()}, pts, ARC_KEYS)
        # reads past the stored entries and bad windows are refused; a refused staging leaves no staged map; NULL outputs are refused
        invalid(fe.stream_archive_points, more["stored"], 1); invalid(fe.stream_archive_points, 1, more["stored"])
        for first, cnt in ((-1, 1), (0, -1)):
            with pytest.raises(ValueError):
                fe.stream_archive_points(first, cnt)
            assert lib.vo_stream_archive_read(h, first, cnt, None, None, None, None, None) == _lib.VO_ERR_INVALID
        assert lib.vo_stream_archive_read(h, 0, more["stored"], None, None, None, None, None) == 0      # any pointer may be NULL
        n, a, w = C.c_int32(7), C.c_int32(7), C.c_int32(7)
        for first, end in ((-1, 2), (2, 1), (3, 0), (-5, -1)):
            fe.map_from_stream_archive()
            assert lib.vo_map_from_stream_archive(h, first, end, 1, C.addressof(n), C.addressof(a), C.addressof(w)) == _lib.VO_ERR_INVALID, (first, end)
            invalid(fe.map_rows)
        assert lib.vo_map_from_stream_archive(h, 0, -1, 1, C.addressof(n), None, C.addressof(w)) == _lib.VO_ERR_INVALID
        assert fe.map_from_stream_archive(3, 3) == dict(n=0, n_archived=0, without_row=0) and len(fe.map_rows()[0]) == 0
        # a new resume = 0 frees the archive (the setting is off now) ...
        start()
        no_archive()
        assert fe.stream_rows_info()["stored"] > 0
        # ... slam_chain releases the stream with its store and archive ...
        fe.stream_archive(-1)
        start(max_cameras=2)
        assert fe.stream_archive_info()["stored"] > 0
        fe.run_pairs([[0, 1]], K, want_points=True)
        assert fe.slam_chain(1, K)["status"].tolist() == [0]
        no_archive()
        # ... and the restart stream and the multi-stream ignore the setting
        start(entry=fe.slam_stream_restart, max_cameras=2)
        no_archive()
        fe.run_pairs([[0, 1], [2, 3]], K, want_points=True)
        fe.slam_streams([1, 1], K)
        no_archive()
        # with the store off they ignore it as well: no refusal
        fe.stream_rows(0)
        start(entry=fe.slam_stream_restart)
        # a capacity the stream cannot index
        fe.stream_rows(-1)
        assert lib.vo_set_stream_archive(h, 2 ** 31) == 0
        fe.run_pairs([[0, 1]], K, want_points=True)
        invalid(fe.slam_stream, 1, K)
        fe.stream_rows(0); fe.stream_archive(0)
    finally:
        fe.ctx.close()
