"""GPU: vo_slam_chains (FrontEnd.slam_chains) — the resident map step for S independent sequences in one call, one workgroup per
sequence and kernel — against vo_slam_chain on every sequence alone.  All comparisons are exact: the same kernels' code runs on
the same lists in the same order, and a tolerance would hide the one thing these tests exist to find, leakage between sequences.

Four sequences cut from synth.sequence(7, 640, 480, step=4.0) / 1000 features / max_cameras = 4, each on slots of its own (so the
same frames are uploaded more than once):
  A  frames 0..6            slots 0..6    6 pairs  evicts a camera at pairs 3, 4, 5
  B  frames 2..6            slots 7..11   4 pairs  starts elsewhere, evicts at its pair 3
  C  frames 0, 1, 2         slots 12..14  2 pairs  the shortest: idles while the others run
  D  frames 0, 1, blank, 3  slots 15..18  3 pairs  its pair 1 fails in vo_pairs_run: the sequence stops, the others must not
tests/test_slam_chains_reference.py pins on the CPU that A, B and C localise every pair and evict where this table says."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, W, H, NFEAT, MAX_CAMERAS = 7, 640, 480, 1000, 4
OUT_KEYS = ("poses_pnp", "poses", "chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")
FRAMES = dict(A=[0, 1, 2, 3, 4, 5, 6], B=[2, 3, 4, 5, 6], C=[0, 1, 2], D=[0, 1, None, 3])       # None: a blank frame (127)
FIRST_SLOT = dict(A=0, B=7, C=12, D=15)
BLANK_PAIR = 1                                                                                    # D's pair (1, blank)


def _pairs(name):
    a = FIRST_SLOT[name]
    return [[a + k, a + k + 1] for k in range(len(FRAMES[name]) - 1)]


def _same(a, b, keys, what=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


class Run:
    """The 19 resident slots; every sequence's run on its own (run_pairs of its pairs -> slam_chain); slam_chains on runs of all
    15 pairs, cached by order and options."""

    def __init__(self):
        from visual_odometry_amd import synth
        from visual_odometry_amd.frontend import FrontEnd
        seq = synth.sequence(N, W, H, step=4.0, cache_dir="/tmp")
        self.K = seq["K"]
        blank = np.full_like(seq["frames"][0], 127)
        slots = [None] * 19
        for name, frames in FRAMES.items():
            for k, f in enumerate(frames):
                slots[FIRST_SLOT[name] + k] = blank if f is None else seq["frames"][f]
        self.fe = FrontEnd(H, W, max_frames=19, max_pairs=15, nfeatures=NFEAT)
        self.fe.upload(np.stack(slots)); self.fe.detect(0, 19)
        self.alone, self.alone_cache, self.cache, self.resident = {}, {}, {}, None
        for name in FRAMES:
            n = len(FRAMES[name]) - 1
            pair_results = self._run_pairs([name])
            out = self.fe.slam_chain(n, self.K, max_cameras=MAX_CAMERAS)
            self.alone[name] = dict(pairs=pair_results, out=out, map=self.fe.slam_map(0))

    def _run_pairs(self, order):
        """run_pairs of the sequences' pairs in this order; what the chain reads of every pair, copied."""
        pairs = [p for name in order for p in _pairs(name)]
        res, X = self.fe.run_pairs(pairs, self.K, want_points=True)
        self.resident = tuple(order)
        got = []
        for p in range(len(pairs)):
            qi, ti, d, mask = self.fe.pair_matches(p)
            n_inl = int((mask > 0).sum())
            got.append(dict(res=res[p].copy(), q=qi, t=ti, d=d, mask=mask, X=X[p][:, :n_inl].copy() if res[p]["status"] == 0 else None))
        return got

    def alone_chain(self, name, snapshot=None, **opts):
        """slam_chain on the sequence alone -> (outputs, final map, snapshot map or None)"""
        key = (name, snapshot, tuple(sorted(opts.items())))
        if key not in self.alone_cache:
            if self.resident != (name,):
                self._run_pairs([name])
            out = self.fe.slam_chain(len(FRAMES[name]) - 1, self.K, snapshot=snapshot, **opts)
            self.alone_cache[key] = (out, self.fe.slam_map(0), self.fe.slam_map(1) if snapshot is not None else None)
        return self.alone_cache[key]

    def together(self, order, snapshot=None, **opts):
        """slam_chains on one run of all the sequences' pairs, in this order -> its list of outputs"""
        self.joint_pairs(order)
        lengths = [len(FRAMES[name]) - 1 for name in order]
        return self.fe.slam_chains(lengths, self.K, snapshot=snapshot, **opts)

    def joint_pairs(self, order):
        if self.resident != tuple(order):
            self.pairs_together = self._run_pairs(order)
        return self.pairs_together

    def chains(self, order, **opts):
        """-> dict(name -> (outputs, final map)), cached"""
        opts.setdefault("max_cameras", MAX_CAMERAS)
        key = (tuple(order), tuple(sorted(opts.items())))
        if key not in self.cache:
            outs = self.together(order, **opts)
            self.cache[key] = {name: (outs[i], self.fe.slam_map(0, seq=i)) for i, name in enumerate(order)}
        return self.cache[key]


@pytest.fixture(scope="module")
def run():
    return Run()


def test_one_sequence_is_todays_call(run):
    fe, K = run.fe, run.K
    run._run_pairs(["A"])
    a = fe.slam_chain(6, K, max_cameras=MAX_CAMERAS, snapshot=(4, 2)); ma, sa = fe.slam_map(0), fe.slam_map(1)
    outs = fe.slam_chains([6], K, max_cameras=MAX_CAMERAS, snapshot=(0, 4, 2))
    assert len(outs) == 1
    _same(a, outs[0], OUT_KEYS)
    assert set(outs[0]) == set(a)
    _same(ma, fe.slam_map(0), S.MAP_KEYS, "final map"); _same(sa, fe.slam_map(1), S.MAP_KEYS, "snapshot")
    _same(ma, fe.slam_map(0, seq=0), S.MAP_KEYS); _same(sa, fe.slam_map(1, seq=0), S.MAP_KEYS)
    assert a["status"].tolist() == [0] * 6 and a["n_cam"].tolist() == [2, 3, 4, 4, 4, 4]
    assert len(sa["cam_frame"]) == 5 and len(ma["cam_frame"]) == 4         # the snapshot is of pair 4 before its eviction
    from visual_odometry_amd import _lib
    with pytest.raises(_lib.VoError):
        fe.slam_map(0, seq=1)                                              # there is no second sequence


def _premise(run, order):
    """A pair's vo_pairs_run result does not depend on which other pairs are in the run (test_a_shorter_chain_is_a_prefix relies
    on the same): the pair results of the joint run, sequence by sequence, are those of the sequence's own run."""
    at, joint = 0, run.joint_pairs(order)
    for name in order:
        for p, want in enumerate(run.alone[name]["pairs"]):
            got = joint[at + p]
            assert got["res"]["status"] == want["res"]["status"], (name, p)
            for k in ("q", "t", "d", "mask"):
                assert np.array_equal(got[k], want[k]), (name, p, k)
            if want["res"]["status"] == 0:
                for k in want["res"].dtype.names:
                    if k != "reserved":
                        assert np.asarray(got["res"][k]).tobytes() == np.asarray(want["res"][k]).tobytes(), (name, p, k)
                assert got["X"].tobytes() == want["X"].tobytes(), (name, p)
        at += len(run.alone[name]["pairs"])


@pytest.mark.parametrize("order", ["DCAB", "ABCD"])
def test_a_sequence_does_not_depend_on_its_neighbours(run, order):
    from visual_odometry_amd import _lib
    _premise(run, order)
    got = run.chains(order)
    for name in order:
        out, m = got[name]
        _same(run.alone[name]["out"], out, OUT_KEYS, name)
        _same(run.alone[name]["map"], m, S.MAP_KEYS, name)
    a, b, c, d = (got[name][0] for name in "ABCD")
    assert a["status"].tolist() == [0] * 6 and a["n_cam"].tolist() == [2, 3, 4, 4, 4, 4] and got["A"][1]["cam_frame"].tolist() == [3, 4, 5, 6]
    assert b["status"].tolist() == [0] * 4 and b["n_cam"].tolist() == [2, 3, 4, 4] and got["B"][1]["cam_frame"].tolist() == [1, 2, 3, 4]
    assert (a["chi2"][:, 1] < a["chi2"][:, 0]).all() and (b["chi2"][:, 1] < b["chi2"][:, 0]).all()
    assert c["status"].tolist() == [0, 0] and c["n_cam"].tolist() == [2, 3] and got["C"][1]["cam_frame"].tolist() == [0, 1, 2]
    failed = int(run.alone["D"]["pairs"][BLANK_PAIR]["res"]["status"])
    assert failed != 0 and d["status"].tolist() == [0, failed, _lib.VO_ERR_NOT_CONFIGURED]
    assert np.all(d["poses"][2:] == 0) and np.all(d["poses_pnp"][2:] == 0) and np.abs(d["poses"][:2]).max() > 0
    assert d["n_cam"].tolist() == [2, 2, 2] and got["D"][1]["cam_frame"].tolist() == [0, 1]
    # C is the shortest: its map after its last pair is its map at the end of the call, four steps of the others later
    i = order.index("C")
    outs = run.together(order, snapshot=(i, 1, 4), max_cameras=MAX_CAMERAS)
    _same(run.fe.slam_map(1, seq=i), run.fe.slam_map(0, seq=i), S.MAP_KEYS, "C after its end")
    _same(run.fe.slam_map(0, seq=i), got["C"][1], S.MAP_KEYS)
    _same(outs[i], c, OUT_KEYS)


def test_snapshot_of_a_middle_sequence(run):
    order = "DCAB"
    i = order.index("A")
    from visual_odometry_amd import _lib
    wants = {stage: run.alone_chain("A", snapshot=(3, stage), max_cameras=MAX_CAMERAS)[2] for stage in (1, 2, 3, 4)}
    plain = run.chains(order)
    for stage, want in wants.items():
        outs = run.together(order, snapshot=(i, 3, stage), max_cameras=MAX_CAMERAS)
        _same(want, run.fe.slam_map(1, seq=i), S.MAP_KEYS, stage)
        for other in range(4):
            if other != i:
                with pytest.raises(_lib.VoError):
                    run.fe.slam_map(1, seq=other)
        for k, name in enumerate(order):                                   # the snapshot does not alter any output
            _same(plain[name][0], outs[k], OUT_KEYS, (stage, name))
            _same(plain[name][1], run.fe.slam_map(0, seq=k), S.MAP_KEYS, (stage, name))
    s2, s4 = wants[2], wants[4]
    assert len(s2["cam_frame"]) == 5 and len(s4["cam_frame"]) == 4        # the stages differ: pair 3 evicts


def test_determinism_and_switches(run):
    order = "DCAB"
    a = run.together(order, max_cameras=MAX_CAMERAS); ma = [run.fe.slam_map(0, seq=i) for i in range(4)]
    b = run.together(order, max_cameras=MAX_CAMERAS); mb = [run.fe.slam_map(0, seq=i) for i in range(4)]
    for i in range(4):
        _same(a[i], b[i], OUT_KEYS, i); _same(ma[i], mb[i], S.MAP_KEYS, i)
    # no bundle adjustment, no filter, no eviction: vo_tracks_pnp_batch on every sequence alone
    off = run.together(order, ba_iterations=0, filter_threshold=0.0, max_cameras=N)
    for i, name in enumerate(order):
        n = len(FRAMES[name]) - 1
        run._run_pairs([name])
        lc = run.fe.localize_chain(n, run.K)
        assert np.array_equal(off[i]["poses_pnp"], lc["poses"]) and np.array_equal(off[i]["poses"], lc["poses"]), name
        for k in ("n_corr", "n_inl", "status"):
            assert np.array_equal(off[i][k], lc[k]), (name, k)
        assert np.array_equal(off[i]["n_pts"], lc["n_map"]) and not off[i]["chi2"].any() and not off[i]["ba_iterations"].any(), name
        if name != "D":
            assert off[i]["n_cam"].tolist() == list(range(2, n + 2)), name


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
            fe.slam_chains(before, K); fe.slam_map(0)
        with pytest.raises(_lib.VoError) as e:
            fe.slam_chains(lengths, K, **kw)
        assert e.value.code == code, (e.value.code, code, lengths, kw)
        no_map_left()

    def raw(seq_off, n_seq):
        """vo_slam_chains itself, past the Python helper"""
        off = np.asarray(seq_off, np.int32)
        B = 8
        opts = _lib.SlamOpts(100, 8.0, 0.99, 0, 50.0, 40, 1.0, 2, 1.0, 18, -1, 0)
        Kc = np.ascontiguousarray(K, np.float64)
        bufs = [np.zeros((B + 4, 12)), np.zeros((B + 4, 12))] + [np.zeros(B, np.int32) for _ in range(6)] + [np.zeros((B, 2)), np.zeros(B, np.int32), np.zeros(B, np.int32)]
        return c.lib.vo_slam_chains(c.handle, n_seq, off.ctypes.data, Kc.ctypes.data, C.addressof(opts), 0, *[b.ctypes.data for b in bufs])

    fe.run_pairs(chain, K, opts=fe.make_opts(match_mode=MATCH_RATIO, want_points=True))
    refused(_lib.VO_ERR_UNSUPPORTED, [3])                                  # ratio matches are not one-to-one
    fe.run_pairs(chain, K, want_points=True)
    refused(_lib.VO_ERR_INVALID, [2, 1], before=[3])                       # frame slot 2 would belong to both sequences
    for lengths in ([2], [2, 2], [3, 0], []):                              # not the run's pairs / an empty sequence / none
        fe.slam_chains([3], K)
        with pytest.raises(ValueError):
            fe.slam_chains(lengths, K)
    fe.slam_chains([3], K); fe.slam_map(0)
    assert raw([0, 2], 1) == _lib.VO_ERR_INVALID; no_map_left()            # ... and the library's own answer to them
    fe.slam_chains([3], K)
    assert raw([0, 0, 3], 2) == _lib.VO_ERR_INVALID; no_map_left()
    assert raw([0, 3], 0) == _lib.VO_ERR_INVALID and raw([1, 3], 1) == _lib.VO_ERR_INVALID and raw([0, 4], 1) == _lib.VO_ERR_INVALID
    refused(_lib.VO_ERR_UNSUPPORTED, [3], before=[3], max_cameras=_lib.VO_BA_MAX_CAMERAS)
    refused(_lib.VO_ERR_INVALID, [3], before=[3], snapshot=(9, 0, 1))      # no sequence 9
    refused(_lib.VO_ERR_INVALID, [3], before=[3], snapshot=(0, 3, 1))      # no pair 3 in it
    refused(_lib.VO_ERR_INVALID, [3], before=[3], free_cameras=0)
    fe.run_pairs([[0, 1], [2, 3]], K, want_points=True)
    refused(_lib.VO_ERR_INVALID, [2], before=[1, 1])                       # one sequence of these two pairs is not a chain
    refused(_lib.VO_ERR_INVALID, [1, 1], before=[1, 1], snapshot=(1, 1, 1))  # sequence 1 has one pair: no pair 1
    two = fe.slam_chains([1, 1], K, snapshot=(1, 0, 4))                    # two sequences of one pair each are fine
    assert [o["status"].tolist() for o in two] == [[0], [0]] and fe.slam_map(1, seq=1)["cam_frame"].tolist() == [0, 1]
    with pytest.raises(_lib.VoError):
        fe.slam_map(1)                                                     # the old accessor: sequence 0, which has no snapshot
    # afterwards slam_chain on a plain chain still works, and forgets the sequences' maps
    fe.run_pairs(chain, K, want_points=True)
    no_map_left()
    many = fe.slam_chains([3], K)
    out = fe.slam_chain(3, K)
    assert out["status"].tolist() == [0, 0, 0] and out["n_cam"].tolist() == [2, 3, 4] and len(fe.slam_map(0)["cam_frame"]) == 4
    _same(out, many[0], OUT_KEYS)
    with pytest.raises(_lib.VoError):
        fe.slam_map(0, seq=1)
    c.close()
