"""The checker of vo_slam_chains_restart: tests/slam_reference.py's free-running chain with the recovery the reference names
but never wires up — initialize_map begins with self.map.clean() (src/visual_slam.py:43-45) — by the rules of include/vo_hip.h:
  1 a pair that failed on its own keeps its status, leaves the map as it stands and the sequence lost;
  2 a pair that is fine but whose solvePnPRansac fails starts a new segment in the same step: step() again, from an empty state;
  3 a lost sequence that meets a fine pair starts a new segment from it, the same way;
  4 the empty state has no map, no mappointdict and no feature_mapper: nothing of the old segment can be reached.
Frames stay numbered along the whole chain (rule 5); the state a run leaves is the last segment's (rule 6).

A pair's input is slam_reference's dict, here with R, t_rel and X for EVERY pair (any pair can start a segment), or
dict(status=code) for a pair that failed on its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402
from test_gpu_chain import _KP, _inv_pose  # noqa: E402

FAILED = -1000                                                            # a pair the oracle's front end could not make (no status of the library's)


def pair_inputs_from_oracle(O, feats, K, min_matches=8):
    """slam_reference.pair_inputs_from_oracle for the chain feats[0], feats[1], ... with recoverPose and the triangulated points on
    every pair; a pair with fewer than min_matches matches or no essential matrix becomes dict(status=FAILED)."""
    out = []
    for k in range(len(feats) - 1):
        a, b = feats[k], feats[k + 1]
        if len(a["desc"]) == 0 or len(b["desc"]) == 0:
            out.append(dict(status=FAILED)); continue
        qi, ti, _ = O.match_hamming(a["desc"], b["desc"], 2)
        if len(qi) < min_matches:
            out.append(dict(status=FAILED)); continue
        p1 = a["xy"][qi].astype(np.float64); p2 = b["xy"][ti].astype(np.float64)
        rc, E, mask, _ = O.find_essential_ransac(p1, p2, K)
        if rc != 0:
            out.append(dict(status=FAILED)); continue
        inl = mask > 0
        _, R, t, _ = O.recover_pose(E[0], p1[inl], p2[inl], K)
        X = O.triangulate(_KP(K, _inv_pose(R, t)), _KP(K, np.eye(3, 4)), p1[inl].T, p2[inl].T)
        out.append(dict(frame1=k, frame2=k + 1, q=qi[inl], t=ti[inl], p1=p1[inl], p2=p2[inl], R=R, t_rel=t, X=X / X[3]))
    return out


def run(O, pair_inputs, K, opts=None):
    """The free-running chain with restarts.  Returns a list, one dict per pair: slam_reference.step's result (status 0 at a pair
    that starts a segment) or dict(status=code, state=the map as it stands), each with `segment` (-1: in none) and `cause`."""
    s, res, alive, nseg, pending = S.empty_state(), [], False, 0, 0
    for pr in pair_inputs:
        if pr.get("status", 0) != 0:                                      # rule 1
            pending = pending or pr["status"]
            alive = False
            res.append(dict(status=pr["status"], state=s, segment=-1, cause=0, n_corr=0, n_inl=0))
            continue
        r, cause = None, 0
        if alive:
            r = S.step(O, s, pr, K, opts)
            if r["status"] != 0:                                          # rule 2
                pending, r = r["status"], None
        if r is None:                                                     # rules 2, 3: initialize_map on a clean map
            r = S.step(O, S.empty_state(), pr, K, opts)
            assert r["status"] == 0
            cause, pending, nseg = pending, 0, nseg + 1
        r["segment"], r["cause"] = nseg - 1, cause
        res.append(r)
        s, alive = r["state"], True
    return res
