"""GPU: vo_slam_chains_restart (FrontEnd.slam_chains / slam_chain with restart=True) — a sequence that loses tracking starts a
new map from the next usable pair, on the device — against vo_slam_chain on every segment's pairs alone.  The premise is the one
of tests/test_gpu_slam_chains.py, asserted first in every test: a pair's vo_pairs_run result does not depend on the other pairs
of the run.  After it all comparisons are exact: a tolerance would hide the one thing these tests exist to find, anything of the
old segment leaking into the new one.

Twenty resident slots cut from synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4:
  L  frames 0, 1, 2, 3, blank (127), 2, 3, 4, 5, 6   slots 0..9     9 pairs: 0-2 segment 0, 3 and 4 fail in vo_pairs_run, 5-8 segment 1
  A  frames 0..6                                     slots 10..16   6 pairs, never fails (also the source of every "alone" chain)
  C  frames 0, 1, 2                                  slots 17..19   2 pairs, never fails
L's segment 1 is frames 2..6 — sequence B of tests/test_gpu_slam_chains.py, which evicts a camera at its pair 3.

Rule 2 (solvePnPRansac fails on a pair that is itself fine) is reached through options; what the CPU run of the free-running
checker showed on sequence A (tests/test_slam_restart_reference.py pins it):
  reproj_err = 1e-9                        no correspondence reprojects that closely: VO_ERR_NO_MODEL at every pair >= 1, with 203,
                                           202, 181, 213, 246 correspondences in a default run — six segments of one pair each
  max_point_norm = 1e-6, max_cameras = 3   add_information_to_map skips every match (:177), so every point keeps its two first
                                           observations and the eviction at pair 2 removes them all: 0 correspondences at pair 3,
                                           VO_ERR_TOO_FEW — segments 0-2 and 3-5, and pair 5 empties the map again
Both are structural, not a matter of the sampler's draws."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
PAIR_KEYS = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
OUT_KEYS = ("poses_pnp", "poses") + PAIR_KEYS
FRAMES = dict(L=[0, 1, 2, 3, None, 2, 3, 4, 5, 6], A=[0, 1, 2, 3, 4, 5, 6], C=[0, 1, 2])          # None: a blank frame (127)
FIRST_SLOT = dict(L=0, A=10, C=17)
BLANK_SLOT = 4
A0 = FIRST_SLOT["A"]


def _slots(name):
    return list(range(FIRST_SLOT[name], FIRST_SLOT[name] + len(FRAMES[name])))


def a_slots(first_frame, last_frame):
    """the slots of A that hold these frames: the chain a segment is compared with, alone"""
    return list(range(A0 + first_frame, A0 + last_frame + 1))


def _pairs(slots):
    return [[a, b] for a, b in zip(slots[:-1], slots[1:])]


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _shifted(m, first):
    """a map with cam_frame and pt_feature[:, 0] counted from the segment's first chain index"""
    m = {k: np.array(v) for k, v in m.items()}
    m["cam_frame"] = m["cam_frame"] - first
    m["pt_feature"][:, 0] -= first
    return m


class Run:
    """The resident slots; run_pairs of any list of chains (slot lists), remembered; slam_chain on one chain alone and
    slam_chains(restart=True) on several, cached by slots and options."""

    def __init__(self):
        from visual_odometry_amd import synth
        from visual_odometry_amd.frontend import FrontEnd
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K = seq["K"]
        blank = np.full_like(seq["frames"][0], 127)
        slots = [None] * 20
        for name, frames in FRAMES.items():
            for k, f in enumerate(frames):
                slots[FIRST_SLOT[name] + k] = blank if f is None else seq["frames"][f]
        self.fe = FrontEnd(H, W, max_frames=20, max_pairs=17, nfeatures=NFEAT)
        self.fe.upload(np.stack(slots)); self.fe.detect(0, 20)
        self.resident, self.pairs, self.cache = None, None, {}

    def run_pairs(self, chains):
        """run_pairs of the chains' pairs, in this order -> what the map step reads of every pair, copied"""
        key = tuple(tuple(c) for c in chains)
        if self.resident != key:
            pairs = [p for c in chains for p in _pairs(c)]
            res, X = self.fe.run_pairs(pairs, self.K, want_points=True)
            got = []
            for p in range(len(pairs)):
                qi, ti, d, mask = self.fe.pair_matches(p)
                n_inl = int((mask > 0).sum())
                got.append(dict(res=res[p].copy(), q=qi, t=ti, d=d, mask=mask, X=X[p][:, :n_inl].copy() if res[p]["status"] == 0 else None))
            self.resident, self.pairs = key, got
        return self.pairs

    def alone(self, slots, snapshot=None, **opts):
        """vo_slam_chain on this chain alone -> dict(out, map, snap, pairs)"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = ("alone", tuple(slots), snapshot, tuple(sorted(opts.items())))
        if key not in self.cache:
            pairs = self.run_pairs([slots])
            out = self.fe.slam_chain(len(slots) - 1, self.K, snapshot=snapshot, **opts)
            self.cache[key] = dict(out=out, map=self.fe.slam_map(0), snap=self.fe.slam_map(1) if snapshot is not None else None, pairs=pairs)
        return self.cache[key]

    def chains(self, chains, snapshot=None, restart=True, **opts):
        """slam_chains on these chains in one call -> dict(outs, maps, snap, pairs)"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = ("chains", tuple(tuple(c) for c in chains), snapshot, restart, tuple(sorted(opts.items())))
        if key not in self.cache:
            pairs = self.run_pairs(chains)
            outs = self.fe.slam_chains([len(c) - 1 for c in chains], self.K, snapshot=snapshot, restart=restart, **opts)
            self.cache[key] = dict(outs=outs, maps=[self.fe.slam_map(0, seq=i) for i in range(len(chains))],
                                   snap=self.fe.slam_map(1, seq=snapshot[0]) if snapshot is not None else None, pairs=pairs)
        return self.cache[key]


@pytest.fixture(scope="module")
def run():
    return Run()


def _premise(run, got, want):
    """two runs' results of what must be the same pairs (same frames, in other slots or beside other pairs) are the same"""
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["res"]["status"] == w["res"]["status"], p
        for k in ("q", "t", "d", "mask"):
            assert np.array_equal(g[k], w[k]), (p, k)
        if w["res"]["status"] == 0:
            for k in w["res"].dtype.names:
                if k != "reserved":
                    assert np.asarray(g["res"][k]).tobytes() == np.asarray(w["res"][k]).tobytes(), (p, k)
            assert g["X"].tobytes() == w["X"].tobytes(), p


def _segment_is_alone(out, k, alone, what=""):
    """segment k of a restart run equals vo_slam_chain on its pairs alone: every per-pair output and the pose rows"""
    sg = out["segments"][k]
    a, n = sg["first_pair"], sg["n_pairs"]
    want = alone["out"]
    assert n == len(want["status"]), (what, k)
    assert out["segment"][a:a + n].tolist() == [k] * n and out["cause"][a + 1:a + n].tolist() == [0] * (n - 1), (what, k)
    for key in PAIR_KEYS:
        assert out[key][a:a + n].dtype == want[key].dtype and np.array_equal(out[key][a:a + n], want[key]), (what, k, key)
    for key in ("poses_pnp", "poses"):
        assert sg[key].shape == want[key].shape and np.array_equal(sg[key], want[key]), (what, k, key)
        assert np.array_equal(out[key][a + 1:a + n + 1], want[key][1:]), (what, k, key)
    return a, n


def test_a_lost_stretch(run):
    """rules 1, 3, 5, 6"""
    from visual_odometry_amd import _lib
    L = _slots("L")
    r = run.chains([L])
    seg0, seg1 = run.alone(a_slots(0, 3)), run.alone(a_slots(2, 6))
    _premise(run, r["pairs"][0:3], seg0["pairs"]); _premise(run, r["pairs"][5:9], seg1["pairs"])
    out, m = r["outs"][0], r["maps"][0]
    failed = [int(r["pairs"][p]["res"]["status"]) for p in (3, 4)]
    assert failed[0] != 0 and failed[1] != 0
    assert out["status"].tolist() == [0, 0, 0, failed[0], failed[1], 0, 0, 0, 0]
    assert out["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1]
    assert out["cause"].tolist() == [0, 0, 0, 0, 0, failed[0], 0, 0, 0]
    assert _lib.VO_ERR_NOT_CONFIGURED not in out["status"].tolist()
    assert [(s["first_pair"], s["n_pairs"]) for s in out["segments"]] == [(0, 3), (5, 4)]
    _segment_is_alone(out, 0, seg0); _segment_is_alone(out, 1, seg1)
    assert np.array_equal(out["segments"][1]["poses"][0], seg1["out"]["poses"][0])
    assert np.array_equal(out["poses"][0], seg0["out"]["poses"][0]) and np.array_equal(out["poses_pnp"][0], seg0["out"]["poses_pnp"][0])
    assert not out["poses"][4:6].any() and not out["poses_pnp"][4:6].any()        # the second frames of the failed pairs; row 5 is not the new segment's
    # the final map is segment 1's, in indices along the whole chain (rule 5); the camera limit worked inside the restarted segment
    assert seg1["out"]["n_cam"].tolist() == [2, 3, 4, 4] and m["cam_frame"].tolist() == [6, 7, 8, 9]
    _same(_shifted(m, 5), seg1["map"], S.MAP_KEYS, "final map")
    assert m["pt_feature"][:, 0].min() >= 5
    # snapshots count along the sequence: pair 6 is pair 1 of segment 1
    for stage in (1, 2, 3, 4):
        snap = run.chains([L], snapshot=(0, 6, stage))
        _same(_shifted(snap["snap"], 5), run.alone(a_slots(2, 6), snapshot=(1, stage))["snap"], S.MAP_KEYS, ("snapshot", stage))
        _same(snap["outs"][0], out, OUT_KEYS + ("segment", "cause"), ("snapshot", stage))
    # while the sequence is lost the map stays as segment 0 left it (rule 1)
    lost = run.chains([L], snapshot=(0, 4, 4))
    _same(lost["snap"], seg0["map"], S.MAP_KEYS, "the map while lost")


RULE2 = {
    "no_model": (dict(reproj_err=1e-9), "VO_ERR_NO_MODEL", [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5)]),
    "too_few": (dict(max_point_norm=1e-6, max_cameras=3), "VO_ERR_TOO_FEW", [(0, 2), (3, 5)]),
}


@pytest.mark.parametrize("case", sorted(RULE2))
def test_reinitialisation_in_the_same_step(run, case):
    """rule 2: the pair is fine, its solvePnPRansac is not"""
    from visual_odometry_amd import _lib
    opts, code, segments = RULE2[case]
    code = getattr(_lib, code)
    A = _slots("A")
    r = run.chains([A], **opts)
    out, m = r["outs"][0], r["maps"][0]
    assert out["status"].tolist() == [0] * 6
    assert out["segment"].tolist() == [k for k, (a, b) in enumerate(segments) for _ in range(a, b + 1)]
    assert out["cause"].tolist() == [code if p > 0 and any(p == a for a, _ in segments) else 0 for p in range(6)]
    off = run.chains([A], restart=False, **opts)["outs"][0]                     # today: the chain ends there
    assert off["status"].tolist() == [0] * segments[1][0] + [code] + [_lib.VO_ERR_NOT_CONFIGURED] * (5 - segments[1][0])
    for k, (a, b) in enumerate(segments):
        alone = run.alone(a_slots(a, b + 1), **opts)
        _premise(run, r["pairs"][a:b + 1], alone["pairs"])
        assert _segment_is_alone(out, k, alone, case) == (a, b - a + 1)
        assert np.array_equal(out["n_corr"][a:a + 1], [0]) and np.array_equal(out["n_inl"][a:a + 1], [0])       # as pair 0 reports them
    a, b = segments[-1]
    _same(_shifted(m, a), run.alone(a_slots(a, b + 1), **opts)["map"], S.MAP_KEYS, "final map")
    # a segment in the middle, through the snapshot of its last pair
    a, b = segments[1]
    snap = run.chains([A], snapshot=(0, b, 4), **opts)
    _same(_shifted(snap["snap"], a), run.alone(a_slots(a, b + 1), **opts)["map"], S.MAP_KEYS, "snapshot")


def test_the_first_pair_is_lost_and_a_chain_that_ends_lost(run):
    head = [BLANK_SLOT] + a_slots(0, 2)
    r = run.chains([head])
    alone = run.alone(a_slots(0, 2))
    _premise(run, r["pairs"][1:], alone["pairs"])
    out = r["outs"][0]
    failed = int(r["pairs"][0]["res"]["status"])
    assert failed != 0 and out["status"].tolist() == [failed, 0, 0]
    assert out["segment"].tolist() == [-1, 0, 0] and out["cause"].tolist() == [0, failed, 0]
    assert [(s["first_pair"], s["n_pairs"]) for s in out["segments"]] == [(1, 2)]
    _segment_is_alone(out, 0, alone, "lost head")
    assert not out["poses"][:2].any() and not out["poses_pnp"][:2].any()          # no camera for the blank frame; row 1 is not the segment's
    _same(_shifted(r["maps"][0], 1), alone["map"], S.MAP_KEYS, "lost head")
    tail = a_slots(0, 3) + [BLANK_SLOT]
    r = run.chains([tail])
    alone = run.alone(a_slots(0, 3))
    _premise(run, r["pairs"][:3], alone["pairs"])
    out = r["outs"][0]
    failed = int(r["pairs"][3]["res"]["status"])
    assert failed != 0 and out["status"].tolist() == [0, 0, 0, failed]
    assert out["segment"].tolist() == [0, 0, 0, -1] and out["cause"].tolist() == [0, 0, 0, 0]
    _segment_is_alone(out, 0, alone, "lost tail")
    _same(r["maps"][0], alone["map"], S.MAP_KEYS, "the map of a chain that ends lost")   # rule 6
    assert not out["poses"][4].any()


@pytest.mark.parametrize("order", ["CLA", "ALC"])
def test_several_sequences(run, order):
    chains = [_slots(name) for name in order]
    r = run.chains(chains)
    off = run.chains(chains, restart=False)
    at = 0
    for i, name in enumerate(order):
        own = run.chains([_slots(name)])
        n = len(own["pairs"])
        _premise(run, r["pairs"][at:at + n], own["pairs"])
        at += n
        _same(own["outs"][0], r["outs"][i], OUT_KEYS + ("segment", "cause"), name)
        _same(own["maps"][0], r["maps"][i], S.MAP_KEYS, name)
        assert len(own["outs"][0]["segments"]) == len(r["outs"][i]["segments"])
        for a, b in zip(own["outs"][0]["segments"], r["outs"][i]["segments"]):
            assert (a["first_pair"], a["n_pairs"]) == (b["first_pair"], b["n_pairs"])
            _same(a, b, ("poses_pnp", "poses"), name)
        if name != "L":                                                         # never fails: restart changes no byte
            _same(off["outs"][i], r["outs"][i], OUT_KEYS, name)
            _same(off["maps"][i], r["maps"][i], S.MAP_KEYS, name)
            assert r["outs"][i]["status"].tolist() == [0] * n
            assert r["outs"][i]["segment"].tolist() == [0] * n and r["outs"][i]["cause"].tolist() == [0] * n
            assert set(r["outs"][i]) == set(off["outs"][i]) | {"segment", "cause", "segments"}
    assert r["outs"][order.index("L")]["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1]


def test_off_is_off_and_call_is_call(run):
    from visual_odometry_amd import _lib
    L = _slots("L")
    pairs = run.run_pairs([L])
    failed = int(pairs[3]["res"]["status"])
    off = run.fe.slam_chains([9], run.K, max_cameras=MAX_CAMERAS)[0]
    assert off["status"].tolist() == [0, 0, 0, failed] + [_lib.VO_ERR_NOT_CONFIGURED] * 5
    assert "segment" not in off and "segments" not in off
    one = run.fe.slam_chain(9, run.K, max_cameras=MAX_CAMERAS)
    _same(off, one, OUT_KEYS)
    # slam_chain(restart=True) is the chains entry with one sequence; two calls return the same bytes
    a = run.fe.slam_chain(9, run.K, max_cameras=MAX_CAMERAS, restart=True); ma = run.fe.slam_map(0)
    b = run.fe.slam_chains([9], run.K, max_cameras=MAX_CAMERAS, restart=True)[0]; mb = run.fe.slam_map(0, seq=0)
    _same(a, b, OUT_KEYS + ("segment", "cause")); _same(ma, mb, S.MAP_KEYS)
    _same(a, run.chains([L])["outs"][0], OUT_KEYS + ("segment", "cause")); _same(ma, run.chains([L])["maps"][0], S.MAP_KEYS)
    for x, y in zip(a["segments"], b["segments"]):
        _same(x, y, ("poses_pnp", "poses"))
    # no bundle adjustment, no filter, no eviction: every segment is vo_tracks_pnp_batch on its pairs
    plain = run.fe.slam_chains([9], run.K, ba_iterations=0, filter_threshold=0.0, max_cameras=N, restart=True)[0]
    assert plain["segment"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, 1]
    for k, (f0, f1) in enumerate(((0, 3), (2, 6))):
        _premise(run, pairs[(0, 5)[k]:(3, 9)[k]], run.run_pairs([a_slots(f0, f1)]))
        lc = run.fe.localize_chain(f1 - f0, run.K)
        sg = plain["segments"][k]
        a0, n = sg["first_pair"], sg["n_pairs"]
        assert np.array_equal(sg["poses_pnp"], lc["poses"]) and np.array_equal(sg["poses"], lc["poses"]), k
        for key in ("n_corr", "n_inl", "status"):
            assert np.array_equal(plain[key][a0:a0 + n], lc[key]), (k, key)
        assert np.array_equal(plain["n_pts"][a0:a0 + n], lc["n_map"]) and not plain["chi2"].any(), k
        assert plain["n_cam"][a0:a0 + n].tolist() == list(range(2, n + 2)), k


def test_rejections():
    from visual_odometry_amd import _lib, synth
    from visual_odometry_amd.frontend import FrontEnd, MATCH_RATIO
    seq = synth.sequence(4, 640, 480, cache_dir="/tmp")
    K = seq["K"]
    c = _lib.Context(0)
    fe = FrontEnd(480, 640, max_frames=4, max_pairs=3, nfeatures=500, ctx=c)
    fe.upload(seq["frames"]); fe.detect(0, 4)
    chain = [[0, 1], [1, 2], [2, 3]]

    def no_map_left():
        for kw in (dict(), dict(seq=1)):
            with pytest.raises(_lib.VoError):
                fe.slam_map(0, **kw)

    def refused(code, lengths, before=None, **kw):
        if before is not None:                                             # a map to lose
            fe.slam_chains(before, K, restart=True); fe.slam_map(0)
        with pytest.raises(_lib.VoError) as e:
            fe.slam_chains(lengths, K, restart=True, **kw)
        assert e.value.code == code, (e.value.code, code, lengths, kw)
        no_map_left()

    def raw(seq_off, n_seq, null=None):
        """vo_slam_chains_restart itself, past the Python helper; null: the index of a new output passed as a null pointer"""
        off = np.asarray(seq_off, np.int32)
        B = 8
        opts = _lib.SlamOpts(100, 8.0, 0.99, 0, 50.0, 40, 1.0, 2, 1.0, 18, -1, 0)
        Kc = np.ascontiguousarray(K, np.float64)
        bufs = [np.zeros((B + 4, 12)), np.zeros((B + 4, 12))] + [np.zeros(B, np.int32) for _ in range(6)] + [np.zeros((B, 2)), np.zeros(B, np.int32), np.zeros(B, np.int32)]
        new = [np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 12)), np.zeros((B, 12))]
        ptrs = [b.ctypes.data for b in bufs] + [None if i == null else b.ctypes.data for i, b in enumerate(new)]
        return c.lib.vo_slam_chains_restart(c.handle, n_seq, off.ctypes.data, Kc.ctypes.data, C.addressof(opts), 0, *ptrs)

    fe.run_pairs(chain, K, opts=fe.make_opts(match_mode=MATCH_RATIO, want_points=True))
    refused(_lib.VO_ERR_UNSUPPORTED, [3])                                  # ratio matches stay refused
    fe.run_pairs(chain, K, want_points=True)
    for null in range(4):                                                  # segment, cause, seg_poses_pnp, seg_poses
        fe.slam_chains([3], K, restart=True); fe.slam_map(0)
        assert raw([0, 3], 1, null=null) == _lib.VO_ERR_INVALID; no_map_left()
    assert raw([0, 3], 1) == _lib.VO_OK and len(fe.slam_map(0)["cam_frame"]) == 4
    refused(_lib.VO_ERR_INVALID, [2, 1], before=[3])                       # frame slot 2 would belong to both sequences
    for lengths in ([2], [2, 2], [3, 0], []):                              # not the run's pairs / an empty sequence / none
        fe.slam_chains([3], K, restart=True)
        with pytest.raises(ValueError):
            fe.slam_chains(lengths, K, restart=True)
    fe.slam_chains([3], K, restart=True); fe.slam_map(0)
    assert raw([0, 2], 1) == _lib.VO_ERR_INVALID; no_map_left()
    assert raw([0, 0, 3], 2) == _lib.VO_ERR_INVALID and raw([0, 3], 0) == _lib.VO_ERR_INVALID and raw([1, 3], 1) == _lib.VO_ERR_INVALID
    refused(_lib.VO_ERR_UNSUPPORTED, [3], before=[3], max_cameras=_lib.VO_BA_MAX_CAMERAS)
    refused(_lib.VO_ERR_INVALID, [3], before=[3], snapshot=(9, 0, 1))      # no sequence 9
    refused(_lib.VO_ERR_INVALID, [3], before=[3], snapshot=(0, 3, 1))      # no pair 3 in it
    refused(_lib.VO_ERR_INVALID, [3], before=[3], free_cameras=0)
    fe.run_pairs([[0, 1], [2, 3]], K, want_points=True)
    refused(_lib.VO_ERR_INVALID, [2], before=[1, 1])                       # one sequence of these two pairs is not a chain
    # afterwards both forms work on a plain chain and agree
    fe.run_pairs(chain, K, want_points=True)
    no_map_left()
    on = fe.slam_chain(3, K, restart=True)
    out = fe.slam_chain(3, K)
    assert out["status"].tolist() == [0, 0, 0] and on["segment"].tolist() == [0, 0, 0] and on["cause"].tolist() == [0, 0, 0]
    _same(out, on, OUT_KEYS)
    c.close()
