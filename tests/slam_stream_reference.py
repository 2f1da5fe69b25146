"""The checker of vo_slam_stream: the carry between two calls as a RENAMING of the free-running checker's state
(tests/slam_reference.py, imported, not edited).  A chunked walk gives every frame of a new chunk a new id (a slot has no meaning
on the CPU; what matters is that an id says nothing about the frame's place in the stream), and between two chunks carry()
rewrites `mapper` and the points' feature ids by the rules of k_slam_carry (docs/kernels/k_slam.md):

  * an anchor keypoint (anchor = the stream's last frame) whose track root lies in an older frame is linked to (ghost, k), and the
    point the root owns is re-keyed there — also when the root owns NO point (the dead root): the link is made all the same;
  * every other mapper entry goes (the frames behind the anchor can never be named again);
  * a point keyed neither in the anchor frame nor in the new ghost frame gets a key no track can produce (NONE, n).

Every id that leaves the slot space keeps its (stream frame, keypoint) in `feat_of`, which is how the final lists are compared
with the free-running walk's.  dead_root_links=False is the variant that leaves a dead-rooted anchor keypoint as its own root;
tests/test_slam_stream_reference.py pins that it does NOT reproduce the free-running walk."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_reference as S  # noqa: E402

NONE = -1                                   # frame id of a key that no track reaches
GHOST0 = 10 ** 6                            # ghost frame ids: GHOST0 + number of the carry


def frame_id(chunk, local):
    """An id that is not the stream index: frame `local` of chunk `chunk` (the anchor keeps the id its own chunk gave it)."""
    return 1000 * (chunk + 1) + 7 * local + 3


def carry(state, anchor, ghost, feat_of, stream_of, dead_root_links=True):
    """The state the next chunk starts from (a new dict; `state` is not modified).  feat_of: {(id, k): (stream frame, k)} for keys
    outside the frames' ids, extended here; stream_of: {frame id: stream index}."""
    s = S.to_lists(state)
    owner = {fid: i for i, fid in enumerate(s["pt_feature"])}

    def feature(fid):
        return feat_of[fid] if fid in feat_of else (stream_of[fid[0]], fid[1])

    mapper = {}
    for (f, k) in sorted(fid for fid in state["mapper"] if fid[0] == anchor):
        root = S.track_feature_back_in_time(state, (f, k))
        if root not in owner and not dead_root_links:
            continue                                                      # the variant: (anchor, k) becomes its own root
        mapper[(anchor, k)] = (ghost, k)
        feat_of[(ghost, k)] = feature(root)
        if root in owner:
            s["pt_feature"][owner[root]] = (ghost, k)
    for i, fid in enumerate(s["pt_feature"]):
        if fid[0] not in (anchor, ghost):
            key = (NONE, len(feat_of))
            feat_of[key] = feature(fid)
            s["pt_feature"][i] = key
    s["mapper"] = mapper
    return s


def run_chunked(O, pair_inputs, K, split, opts=None, dead_root_links=True):
    """pair_inputs: the free-running walk's (frame1 = k, frame2 = k + 1).  split: pairs per chunk.  Returns (list of step results,
    final state with cam_frame and pt_feature as stream indices)."""
    assert sum(split) == len(pair_inputs)
    feat_of, stream_of, ids = {}, {}, {}
    s, res, at = S.empty_state(), [], 0
    for c, n in enumerate(split):
        if c > 0:
            s = carry(s, ids[at], GHOST0 + c, feat_of, stream_of, dead_root_links)
        for j in range(n + 1):
            if at + j not in ids:                                         # (the anchor keeps its id)
                ids[at + j] = frame_id(c, j); stream_of[ids[at + j]] = at + j
        for j in range(n):
            pr = dict(pair_inputs[at + j]); pr["frame1"] = ids[at + j]; pr["frame2"] = ids[at + j + 1]
            r = S.step(O, s, pr, K, opts)
            res.append(r)
            if r["status"] != 0:
                return res, None
            s = r["state"]
        at += n
    out = S.to_lists(s)
    out["cam_frame"] = [stream_of[f] for f in out["cam_frame"]]
    out["pt_feature"] = [feat_of[fid] if fid in feat_of else (stream_of[fid[0]], fid[1]) for fid in out["pt_feature"]]
    return res, out


def same_walk(res_a, res_b):
    """Two lists of step results report the same statuses, counts and cameras, exactly."""
    if len(res_a) != len(res_b):
        return False
    for a, b in zip(res_a, res_b):
        if (a["status"], a["n_corr"], a["n_inl"]) != (b["status"], b["n_corr"], b["n_inl"]):
            return False
        if (a["pose_pnp"] is None) != (b["pose_pnp"] is None) or (a["pose_pnp"] is not None and not np.array_equal(a["pose_pnp"], b["pose_pnp"])):
            return False
    return True


def same_lists(state_a, state_b):
    a, b = S.to_arrays(state_a), S.to_arrays(state_b)
    return all(a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in S.MAP_KEYS)


def dead_root_counts(snapshots, matches, carry_pair):
    """What test 4 of tests/test_gpu_slam_stream.py needs of a whole run: snapshots[p] = the map after pair p's stage 1
    (add_information_to_map; p = 0 .. B - 1, slam_map layout with pt_feature as (chain frame, keypoint)), matches[p] = (q, t) of
    pair p's E inliers.  Returns (anchor keypoints whose track root owns no map point at the carry after pair carry_pair,
    points added after the carry under such a track).  The owners at the carry are taken from stage 1 of pair carry_pair, a
    superset if that pair's camera limit removes points: both counts are lower bounds that need no other stage."""
    mapper = {}
    for p in range(carry_pair + 1):
        q, t = matches[p]
        for a, b in zip(q, t):
            mapper[(p + 1, int(b))] = (p, int(a))
    anchor = carry_pair + 1

    def root(fid):
        while fid in mapper:
            fid = mapper[fid]
        return fid

    owned = {(int(a), int(b)) for a, b in snapshots[carry_pair]["pt_feature"]}    # superset of the owners at the carry: pair carry_pair's limit may remove some
    dead = {k for (f, k) in mapper if f == anchor and root((f, k)) not in owned}
    added = 0
    for p in range(carry_pair + 1, len(matches)):
        q, t = matches[p]
        for a, b in zip(q, t):
            mapper[(p + 1, int(b))] = (p, int(a))
        for (f, k) in {(int(a), int(b)) for a, b in snapshots[p]["pt_feature"] if a == p}:   # pair p's new points: keyed by featureid1 = (frame p, q)
            r = (f, k)
            while r in mapper and r[0] > anchor:
                r = mapper[r]
            if r[0] == anchor and r[1] in dead:
                added += 1
    return len(dead), added
