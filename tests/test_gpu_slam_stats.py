"""GPU: the map statistics of the resident map (FrontEnd.map_stats / slam_stats, vo_set_slam_stats / vo_slam_stats) in every
vo_slam_* entry, against tests/map_stats_reference.py on the device's own snapshots.  Every comparison is exact: byte equality
on the doubles, array_equal on the integers.

The sequences of the existing slam tests: synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4 (flight A, six
pairs, pairs 3-5 evict a camera) and flight L of the restart tests — frames 0 1 2 3 blank 2 3 4 5 6: pairs 0-2 segment 0, pairs
3 and 4 fail, pairs 5-8 segment 1.

Row p describes the map that n_pts[p], n_obs[p], n_cam[p] describe: the snapshot of (p, 4).  While flight L is lost (pairs 3, 4)
that map is segment 0's, untouched (n_cam stays 4: tests/test_gpu_slam_stream_restart.py), so those rows repeat row 2; a row
is all zeros where the three counts are zero (a first pair that fails)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_stats_reference as R  # noqa: E402
import slam_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
STATS_KEYS = ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix", "cam_frame")
FLIGHTS = dict(L=[0, 1, 2, 3, None, 2, 3, 4, 5, 6], A=[0, 1, 2, 3, 4, 5, 6])          # None: a blank frame (127)


def _same_rows(a, b, what=""):
    for k in STATS_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _row_is(stats, p, m, K, what=""):
    """row p of a slam_stats dict == the checker on map m"""
    want = R.stats(m, K)
    got = {k: stats[k][p] for k in STATS_KEYS}
    n = len(m["cam_frame"])
    C = stats["cam_frame"].shape[1]
    assert C == MAX_CAMERAS and stats["obs_matrix"].shape[1:] == (C, C)
    R.same(got, want, ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist"), (what, p))
    assert np.array_equal(got["obs_matrix"][:n, :n], want["obs_matrix"]) and got["obs_matrix"].sum() == want["obs_matrix"].sum(), (what, p)
    assert got["cam_frame"][:n].tolist() == m["cam_frame"].tolist() and (got["cam_frame"][n:] == -1).all(), (what, p)


def _zero_row(stats, p):
    return not any(np.asarray(stats[k][p]).any() for k in STATS_KEYS if k != "cam_frame") and (stats["cam_frame"][p] == -1).all()


class Run:
    """One FrontEnd with both flights resident (L in slots 0-9, A in slots 10-16) and the runs on them, cached."""

    def __init__(self):
        from visual_odometry_amd import synth
        from visual_odometry_amd.frontend import FrontEnd
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K, frames = seq["K"], seq["frames"]
        blank = np.full_like(frames[0], 127)
        self.slot0 = dict(L=0, A=10)
        self.fe = FrontEnd(H, W, max_frames=17, max_pairs=15, nfeatures=NFEAT)
        self.fe.upload(np.stack([blank if k is None else frames[k] for k in FLIGHTS["L"] + FLIGHTS["A"]])); self.fe.detect(0, 17)
        self.cache, self.resident = {}, None

    def pairs(self, flight, first=0, count=None):
        n = len(FLIGHTS[flight]) - 1 if count is None else count
        a = self.slot0[flight] + first
        return [[a + j, a + j + 1] for j in range(n)]

    def run_pairs(self, pairs):
        if self.resident != pairs:
            self.fe.run_pairs(pairs, self.K, want_points=True)
            self.resident = [list(p) for p in pairs]

    def chain(self, flight, stats=True, snapshot=None, **opts):
        """slam_chain on the whole flight -> dict(out, map, snap, stats)"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (flight, stats, snapshot, tuple(sorted(opts.items())))
        if key not in self.cache:
            fe = self.fe
            self.run_pairs(self.pairs(flight))
            fe.map_stats(stats)
            out = fe.slam_chain(len(FLIGHTS[flight]) - 1, self.K, snapshot=snapshot, **opts)
            self.cache[key] = dict(out=out, map=fe.slam_map(0), snap=fe.slam_map(1) if snapshot is not None else None,
                                   stats=fe.slam_stats() if stats else None)
            fe.map_stats(False)
        return self.cache[key]


@pytest.fixture(scope="module")
def run():
    return Run()


def test_statistics_change_nothing_and_are_off_by_default(run):
    from visual_odometry_amd import _lib
    off, on = run.chain("A", stats=False), run.chain("A")
    assert set(off["out"]) == set(on["out"])
    for k in off["out"]:
        assert off["out"][k].dtype == on["out"][k].dtype and off["out"][k].tobytes() == on["out"][k].tobytes(), k
    for k in S.MAP_KEYS:
        assert off["map"][k].tobytes() == on["map"][k].tobytes(), k
    assert on["out"]["status"].tolist() == [0] * 6 and on["out"]["n_cam"].tolist() == [2, 3, 4, 4, 4, 4]
    # with statistics off there are no rows to report, whatever an earlier call left
    run.run_pairs(run.pairs("A"))
    run.fe.slam_chain(6, run.K, max_cameras=MAX_CAMERAS)
    with pytest.raises(_lib.VoError) as e:
        run.fe.slam_stats()
    assert e.value.code == _lib.VO_ERR_INVALID


def test_every_row_is_the_checker_on_that_pairs_snapshot(run):
    whole = run.chain("A")
    st, out = whole["stats"], whole["out"]
    assert set(st) == set(STATS_KEYS) and st["total_sqerr"].shape == (6,) and st["obs_hist"].shape == (6, 64)
    for p in range(6):                                                  # no pair is left out
        r = run.chain("A", snapshot=(p, 4))
        _same_rows(r["stats"], st, ("a snapshot changes no row", p))
        m = r["snap"]
        assert (len(m["cam_frame"]), len(m["points"]), len(m["obs_cam"])) == (out["n_cam"][p], out["n_pts"][p], out["n_obs"][p])
        _row_is(st, p, m, run.K, "snapshot")
        assert st["obs_hist"][p].sum() == out["n_pts"][p] and st["total_sqerr"][p] > 0 and st["mean_sqerr"][p] == st["total_sqerr"][p] / out["n_obs"][p]
    _row_is(st, 5, whole["map"], run.K, "final map")
    assert st["obs_hist"][5][0] > 0                                     # an eviction leaves points without observations (bin 0, the addition)
    assert st["obs_matrix"][5][0, 1] > 0 and not np.tril(st["obs_matrix"][5]).any()


@pytest.mark.parametrize("pair", [1, 3])
def test_other_options(run, pair):
    """free_cameras = 3 and no filter: observations above the threshold of 10 stay in the map, n_high can be non-zero"""
    opts = dict(free_cameras=3, filter_threshold=0.0)
    r = run.chain("A", snapshot=(pair, 4), **opts)
    _row_is(r["stats"], pair, r["snap"], run.K, "no filter")
    _row_is(r["stats"], 5, r["map"], run.K, "no filter, final")
    assert not np.array_equal(r["stats"]["total_sqerr"], run.chain("A")["stats"]["total_sqerr"])


@pytest.mark.parametrize("order", ["LA", "AL"])
def test_slam_chains_rows_are_each_chains_own(run, order):
    """two sequences in two listing orders (restart=True, so that flight L runs through): per-sequence rows = the single chain's"""
    fe = run.fe
    want = dict(L=run.chain("L", restart=True), A=run.chain("A", restart=True))
    _same_rows(want["A"]["stats"], run.chain("A")["stats"], "restart=True changes nothing on a flight that never fails")
    pairs = [p for f in order for p in run.pairs(f)]
    run.run_pairs(pairs)
    fe.map_stats(True)
    outs = fe.slam_chains([len(FLIGHTS[f]) - 1 for f in order], run.K, max_cameras=MAX_CAMERAS, restart=True)
    got = [fe.slam_stats(s) for s in range(2)]
    fe.map_stats(False)
    for s, f in enumerate(order):
        assert np.array_equal(outs[s]["n_obs"], want[f]["out"]["n_obs"]), f
        _same_rows(got[s], want[f]["stats"], f)


def test_restart_rows_follow_the_counts(run):
    """flight L with restart=True: every segment's rows are the checker on that segment's snapshots; the rows of the lost pairs
    describe what n_pts / n_obs / n_cam describe there — segment 0's map, untouched"""
    whole = run.chain("L", restart=True)
    st, out = whole["stats"], whole["out"]
    assert out["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1] and out["n_cam"].tolist() == [2, 3, 4, 4, 4, 2, 3, 4, 4]
    for p in (2, 3, 5, 8):                                              # the end of segment 0, a lost pair, the restart, the eviction
        r = run.chain("L", restart=True, snapshot=(p, 4))
        m = r["snap"]
        assert (len(m["cam_frame"]), len(m["points"]), len(m["obs_cam"])) == (out["n_cam"][p], out["n_pts"][p], out["n_obs"][p])
        _row_is(st, p, m, run.K, "L")
    _row_is(st, 8, whole["map"], run.K, "L, final")
    for p in (3, 4):                                                    # lost: the map is not touched
        assert (out["n_cam"][p], out["n_pts"][p], out["n_obs"][p]) == (out["n_cam"][2], out["n_pts"][2], out["n_obs"][2])
        for k in STATS_KEYS:
            assert np.asarray(st[k][p]).tobytes() == np.asarray(st[k][2]).tobytes(), (p, k)
    assert st["cam_frame"][5].tolist() == [5, 6, -1, -1] and st["cam_frame"][8].tolist() == [6, 7, 8, 9]


def test_a_row_is_zero_where_the_counts_are(run):
    """a chain whose first pair fails (blank, frame 2 of flight L's second half) has no map: n_* = 0 and all-zero rows"""
    fe = run.fe
    pairs = run.pairs("L", first=4, count=3)                            # (blank, 2), (2, 3), (3, 4) without restart: dead from pair 0
    run.run_pairs(pairs)
    fe.map_stats(True)
    out = fe.slam_chain(3, run.K, max_cameras=MAX_CAMERAS)
    st = fe.slam_stats()
    fe.map_stats(False)
    assert out["status"][0] != 0 and not out["n_cam"].any() and not out["n_pts"].any() and not out["n_obs"].any()
    assert all(_zero_row(st, p) for p in range(3))


def _stream(run, flight, split, restart):
    """the flight in chunks through slam_stream / slam_stream_restart with statistics on -> the calls' slam_stats dicts"""
    fe, at, got = run.fe, 0, []
    fe.map_stats(True)
    call = fe.slam_stream_restart if restart else fe.slam_stream
    for c, n in enumerate(split):
        run.run_pairs(run.pairs(flight, first=at, count=n))
        out = call(n, run.K, resume=c > 0, total_pairs=sum(split), max_cameras=MAX_CAMERAS)
        st = fe.slam_stats()
        assert st["total_sqerr"].shape == (n,) and len(out["status"]) == n
        got.append(st)
        at += n
    fe.map_stats(False)
    return got


@pytest.mark.parametrize("split", [(3, 3), (2, 2, 2)], ids=["3+3", "2+2+2"])
def test_a_stream_joins_to_the_one_call_rows(run, split):
    from visual_odometry_amd.frontend import join_stats
    joined = join_stats(_stream(run, "A", split, restart=False))
    _same_rows(joined, run.chain("A")["stats"], split)
    assert joined["cam_frame"][-1].tolist() == [3, 4, 5, 6]             # stream indices


def test_a_restart_stream_joins_to_the_one_call_rows(run):
    from visual_odometry_amd.frontend import join_stats
    joined = join_stats(_stream(run, "L", (4, 5), restart=True))
    _same_rows(joined, run.chain("L", restart=True)["stats"], "4+5")


def test_a_stream_keeps_the_setting_it_started_with(run):
    from visual_odometry_amd import _lib
    fe = run.fe
    run.run_pairs(run.pairs("A", first=0, count=3))
    fe.map_stats(True)
    fe.slam_stream(3, run.K, total_pairs=6, max_cameras=MAX_CAMERAS)
    fe.map_stats(False)
    run.run_pairs(run.pairs("A", first=3, count=3))
    with pytest.raises(_lib.VoError) as e:
        fe.slam_stream(3, run.K, resume=True, total_pairs=6, max_cameras=MAX_CAMERAS)
    assert e.value.code == _lib.VO_ERR_INVALID
    fe.map_stats(True)                                                  # the stream is unharmed
    fe.slam_stream(3, run.K, resume=True, total_pairs=6, max_cameras=MAX_CAMERAS)
    st = fe.slam_stats()
    fe.map_stats(False)
    for k in STATS_KEYS:
        assert st[k].tobytes() == run.chain("A")["stats"][k][3:].tobytes(), k


def test_slam_streams_rows_are_each_streams_own(run):
    """(L, A) in calls of (3, 2) pairs with each sequence idle once: every sequence's joined rows are its own flight's"""
    from visual_odometry_amd.frontend import join_stats
    fe = run.fe
    calls = [(3, 2), (3, 0), (3, 2), (0, 2)]
    at, got = dict(L=0, A=0), dict(L=[], A=[])
    fe.map_stats(True)
    for c, (nl, na) in enumerate(calls):
        run.run_pairs(run.pairs("L", at["L"], nl) + run.pairs("A", at["A"], na))
        out = fe.slam_streams([nl, na], run.K, resume=c > 0, total_pairs=[9, 6], max_cameras=MAX_CAMERAS)
        assert out["seq_off"].tolist() == [0, nl, nl + na]
        for s, (f, n) in enumerate((("L", nl), ("A", na))):
            st = fe.slam_stats(s)
            assert st["total_sqerr"].shape == (n,) and st["obs_matrix"].shape == (n, MAX_CAMERAS, MAX_CAMERAS)
            got[f].append(st)
        at["L"] += nl; at["A"] += na
    fe.map_stats(False)
    _same_rows(join_stats(got["L"]), run.chain("L", restart=True)["stats"], "L")
    _same_rows(join_stats(got["A"]), run.chain("A")["stats"], "A")
