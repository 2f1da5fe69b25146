"""GPU: the profiling brackets of every vo_slam_* entry point (slam_api.hip, slam_walk).  One walk issues the steps of all six; what
it must bracket does not depend on the entry point, only on the steps n of the call (B of a single form, the longest sequence's
pairs otherwise), on whether the call is resumed, and on the options:

  misc                  n, plus 1 on a resumed call (the carry)
  slam_ba_prepare       n with BA on, else 0
  slam_bundle_adjust    n with BA on, else 0
  slam_filter           n with BA on; with BA off and a filter threshold n - 1 on a first call, n on a resumed one; else 0
  slam_camera_limit     n
  slam_map_statistics   n with statistics on, else 0

Four 320x240 synthetic frames, 300 features, 3 pairs a run.  The counters are reset after run_pairs, so what profile_read reports is
the SLAM call's alone.  Whether a pair is localised does not matter to the host loop (the restart forms go on after a lost one)."""
import pytest

pytestmark = pytest.mark.gpu

H, W, NFEAT = 240, 320, 300
STAGES = ("misc", "slam_ba_prepare", "slam_bundle_adjust", "slam_filter", "slam_camera_limit", "slam_map_statistics")
CASES = {
    "ba_filter": dict(ba_iterations=3, filter_threshold=1.0, stats=False),
    "filter_only_stats": dict(ba_iterations=0, filter_threshold=1.0, stats=True),
    "ba_only_stats": dict(ba_iterations=3, filter_threshold=0.0, stats=True),
    "neither": dict(ba_iterations=0, filter_threshold=0.0, stats=False),
}


def expected(n, resumed, ba_iterations, filter_threshold, stats):
    ba, filt = ba_iterations > 0, filter_threshold > 0
    return dict(misc=n + (1 if resumed else 0), slam_ba_prepare=n if ba else 0, slam_bundle_adjust=n if ba else 0,
                slam_filter=n if ba else ((n if resumed else n - 1) if filt else 0), slam_camera_limit=n, slam_map_statistics=n if stats else 0)


@pytest.fixture(scope="module")
def rig():
    from visual_odometry_amd import synth
    from visual_odometry_amd.frontend import FrontEnd
    seq = synth.sequence(4, W, H, step=4.0, cache_dir="/tmp")
    fe = FrontEnd(H, W, max_frames=6, max_pairs=3, nfeatures=NFEAT)
    yield dict(fe=fe, K=seq["K"], frames=seq["frames"])
    fe.profile(False)
    fe.map_stats(False)


def put(rig, frame, slot):
    rig["fe"].upload(rig["frames"][frame][None], first_slot=slot)
    rig["fe"].detect(slot, 1)


def brackets(rig, pairs, call):
    """run_pairs, reset the counters, the SLAM call -> brackets per stage"""
    fe = rig["fe"]
    fe.run_pairs(pairs, rig["K"], want_points=True)
    fe.profile(True)
    call()
    got = fe.profile_read()
    fe.profile(False)
    return {s: got.get(s, (0.0, 0))[1] for s in STAGES}


@pytest.mark.parametrize("case", sorted(CASES))
def test_brackets_of_every_entry_point(rig, case):
    c = CASES[case]
    fe, K = rig["fe"], rig["K"]
    opts = dict(ba_iterations=c["ba_iterations"], filter_threshold=c["filter_threshold"], max_cameras=3, free_cameras=2)
    want = lambda n, resumed: expected(n, resumed, **c)
    fe.map_stats(c["stats"])
    seen = {}
    # slots 0 .. 3: the four frames, a chain of 3 pairs; slots 4, 5: frames 2, 3 again, a second sequence
    for k in range(4):
        put(rig, k, k)
    put(rig, 2, 4); put(rig, 3, 5)
    chain = [[0, 1], [1, 2], [2, 3]]
    two = [[0, 1], [1, 2], [4, 5]]                                   # sequences of 2 and 1 pairs
    seen["chain"] = (brackets(rig, chain, lambda: fe.slam_chain(3, K, **opts)), want(3, False))
    seen["chains"] = (brackets(rig, two, lambda: fe.slam_chains([2, 1], K, **opts)), want(2, False))
    seen["chains_restart"] = (brackets(rig, two, lambda: fe.slam_chains([2, 1], K, restart=True, **opts)), want(2, False))
    for name, stream in (("stream", fe.slam_stream), ("stream_restart", fe.slam_stream_restart)):
        first = {}
        seen[name] = (brackets(rig, chain[:2], lambda: first.update(stream(2, K, total_pairs=3, **opts))), want(2, False))
        if name == "stream":
            assert (first["status"] == 0).all(), "vo_slam_stream cannot be resumed after a pair that was not localised: choose other frames"
        seen[name + "_resumed"] = (brackets(rig, chain[2:], lambda: stream(1, K, resume=True, **opts)), want(1, True))
    seen["streams"] = (brackets(rig, two, lambda: fe.slam_streams([2, 1], K, total_pairs=[4, 1], **opts)), want(2, False))
    # sequence 0 goes on from slot 2 to frame 3 in slot 3 while sequence 1 is idle; then seat 1 is vacated, and sequence 0 goes on
    # to frame 0 in slot 0: the carry of that call is the seats form
    seen["streams_resumed"] = (brackets(rig, [[2, 3]], lambda: fe.slam_streams([1, 0], K, resume=True, **opts)), want(1, True))
    fe.slam_streams_replace(1, 1)
    put(rig, 0, 0)
    seen["streams_vacant_seat"] = (brackets(rig, [[3, 0]], lambda: fe.slam_streams([1, 0], K, resume=True, **opts)), want(1, True))
    for name, (got, exp) in seen.items():
        print(case, name, got)
    for name, (got, exp) in seen.items():
        assert got == exp, (case, name, got, exp)
