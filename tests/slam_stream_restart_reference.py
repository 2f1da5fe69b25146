"""The checker of vo_slam_stream_restart: the rules of tests/slam_restart_reference.py's run() walked chunk by chunk, with
tests/slam_stream_reference.py's carry() between two chunks (both imported, neither edited).  The frames of every chunk get new
ids, as in run_chunked there, so nothing can lean on an id saying where in the stream its frame lies; what outlives a chunk is what
the device keeps between two calls: the state (renamed by carry), whether the stream is alive, the number of segments started and
the status that ended tracking and has not been reported yet.

After a chunk that ends lost the anchor frame — the second frame of a pair that failed on its own — has no entry in the mapper:
carry() finds no anchor link to restate, every point loses its key, and the state is only kept to be reported (rule 6) until a
usable pair starts from an empty state.  run_chunked says so per carry (`carries`) and refuses a lost carry that did find a link."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
import slam_restart_reference as RR  # noqa: E402
import slam_stream_reference as SR  # noqa: E402


def run_chunked(O, pair_inputs, K, split, opts=None):
    """pair_inputs: slam_restart_reference's (frame1 = k, frame2 = k + 1, or dict(status=code)).  split: pairs per chunk.
    Returns (one dict per pair as slam_restart_reference.run returns them, final state with cam_frame and pt_feature as stream
    indices, carries = one dict(chunk, lost, anchor_links, cameras) per carry)."""
    assert sum(split) == len(pair_inputs)
    feat_of, stream_of, ids = {}, {}, {}
    s, res, alive, nseg, pending, at, carries = S.empty_state(), [], False, 0, 0, 0, []
    for c, n in enumerate(split):
        if c > 0:
            anchor = ids[at]
            links = sum(1 for fid in s["mapper"] if fid[0] == anchor)
            in_map = anchor in s["cam_frame"]
            assert in_map == alive                                        # the anchor is a camera of the map exactly when the stream is alive
            if not alive:
                assert links == 0, "a chunk that ended lost left feature tracks at its last frame"
            carries.append(dict(chunk=c, lost=not alive, anchor_links=links, cameras=[stream_of[f] for f in s["cam_frame"]]))
            s = SR.carry(s, anchor, SR.GHOST0 + c, feat_of, stream_of)
        for j in range(n + 1):
            if at + j not in ids:                                         # (the anchor keeps its id)
                ids[at + j] = SR.frame_id(c, j); stream_of[ids[at + j]] = at + j
        for j in range(n):
            pr = pair_inputs[at + j]
            if pr.get("status", 0) != 0:                                  # rule 1
                pending = pending or pr["status"]
                alive = False
                res.append(dict(status=pr["status"], state=s, segment=-1, cause=0, n_corr=0, n_inl=0))
                continue
            pr = dict(pr); pr["frame1"] = ids[at + j]; pr["frame2"] = ids[at + j + 1]
            r, cause = None, 0
            if alive:
                r = S.step(O, s, pr, K, opts)
                if r["status"] != 0:                                      # rule 2
                    pending, r = r["status"], None
            if r is None:                                                 # rules 2, 3: initialize_map on a clean map
                r = S.step(O, S.empty_state(), pr, K, opts)
                assert r["status"] == 0
                cause, pending, nseg = pending, 0, nseg + 1
            r["segment"], r["cause"] = nseg - 1, cause
            res.append(r)
            s, alive = r["state"], True
        at += n
    out = S.to_lists(s)
    out["cam_frame"] = [stream_of[f] for f in out["cam_frame"]]
    out["pt_feature"] = [feat_of[fid] if fid in feat_of else (stream_of[fid[0]], fid[1]) for fid in out["pt_feature"]]
    return res, out, carries


def same_table(res_a, res_b):
    """Two walks report the same statuses, segments, causes and correspondence counts."""
    key = lambda r: (r["status"], r["segment"], r["cause"], r["n_corr"], r["n_inl"])   # noqa: E731
    return len(res_a) == len(res_b) and all(key(a) == key(b) for a, b in zip(res_a, res_b))
