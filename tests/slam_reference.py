"""The checker of vo_slam_chain: the reference's list and dict walks of one frame, re-typed — VisualSlam.initialize_map
(src/visual_slam.py:43-92), add_information_to_map with its Observations (:101-180), freeze_nonlast_cameras (:270-275), the
threshold filter (src/map.py:46-70), remove_camera_from_map / limit_number_of_camera_in_map (map.py:188-232, 299-318) —
composed around oracle.solve_pnp_ransac / rodrigues / triangulate / reprojection_sqerr and tests/ba_reference.lm, the way
reference_chain in tests/test_gpu_chain.py composes its three oracles (its helpers are imported, not copied).

A state is a dict: the map's three lists in the layout FrontEnd.slam_map returns (cam_frame, cam_pose [n, 3, 4], cam_fixed,
pt_feature [n, 2] = (frame, keypoint), points [n, 3], obs_cam, obs_pt, obs_xy) plus `mapper`, VisualSlam.feature_mapper as a
dict {(frame, keypoint): (frame, keypoint)}.  A pair's input is dict(frame1, frame2, q, t, p1, p2[, R, t_rel, X]): the E inliers
in match order (keypoint indices and pixel coordinates) and, for pair 0, recoverPose's result and the triangulated points.

Deviations kept from vo_tracks_pnp_batch (include/vo_hip.h): the initial cameras are stored consistently with the initial
points (camera 2 = identity), and a pair whose localisation fails does nothing further and ends the chain."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_reference as BA  # noqa: E402
from test_gpu_chain import _KP, _inv_pose  # noqa: E402

DEFAULTS = dict(iterations=100, reproj_err=8.0, confidence=0.99, seed=0xFFFFFFFFFFFFFFFF,
                max_point_norm=50.0, ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18)
MAP_KEYS = ("cam_frame", "cam_pose", "cam_fixed", "pt_feature", "points", "obs_cam", "obs_pt", "obs_xy")


def empty_state():
    return dict(cam_frame=[], cam_pose=[], cam_fixed=[], pt_feature=[], points=[], obs_cam=[], obs_pt=[], obs_xy=[], mapper={})


def to_lists(m, mapper=None):
    """A state with python lists (the walks append) from a slam_map dict or another state."""
    s = dict(cam_frame=[int(v) for v in m["cam_frame"]], cam_pose=[np.array(T, np.float64).reshape(3, 4) for T in m["cam_pose"]],
             cam_fixed=[bool(v) for v in m["cam_fixed"]], pt_feature=[(int(a), int(b)) for a, b in m["pt_feature"]],
             points=[np.array(X, np.float64) for X in m["points"]], obs_cam=[int(v) for v in m["obs_cam"]],
             obs_pt=[int(v) for v in m["obs_pt"]], obs_xy=[np.array(v, np.float64) for v in m["obs_xy"]])
    s["mapper"] = dict(m.get("mapper", {}) if mapper is None else mapper)
    return s


def to_arrays(s):
    """The layout FrontEnd.slam_map returns."""
    return dict(cam_frame=np.array(s["cam_frame"], np.int32), cam_pose=np.array(s["cam_pose"], np.float64).reshape(-1, 3, 4),
                cam_fixed=np.array(s["cam_fixed"], bool), pt_feature=np.array(s["pt_feature"], np.int32).reshape(-1, 2),
                points=np.array(s["points"], np.float64).reshape(-1, 3), obs_cam=np.array(s["obs_cam"], np.int32),
                obs_pt=np.array(s["obs_pt"], np.int32), obs_xy=np.array(s["obs_xy"], np.float64).reshape(-1, 2))


def update_feature_mapper(s, pr):
    for q, t in zip(pr["q"], pr["t"]):                                   # :183-188 / :49-53
        s["mapper"][(pr["frame2"], int(t))] = (pr["frame1"], int(q))


def track_feature_back_in_time(s, fid):
    while fid in s["mapper"]:                                            # :94-99
        fid = s["mapper"][fid]
    return fid


def _observe(s, pt, cam, xy):
    s["obs_cam"].append(cam); s["obs_pt"].append(pt); s["obs_xy"].append(np.array(xy, np.float64))


def initialize_map(s, pr):
    """:43-92 up to optimize_map; camera 1 = [R^T | -R^T t] fixed, camera 2 = identity free (the documented deviation)."""
    update_feature_mapper(s, pr)
    s["cam_frame"] += [pr["frame1"], pr["frame2"]]
    s["cam_pose"] += [_inv_pose(pr["R"], pr["t_rel"]), np.eye(3, 4)]
    s["cam_fixed"] += [True, False]
    for i, q in enumerate(pr["q"]):
        s["pt_feature"].append((pr["frame1"], int(q))); s["points"].append(np.array(pr["X"][:3, i], np.float64))
        pt = len(s["points"]) - 1
        _observe(s, pt, 0, pr["p1"][i]); _observe(s, pt, 1, pr["p2"][i])


def add_information_to_map(s, pr, X, max_norm):
    """:152-179 after the camera of frame 2 was added (:250); X = the pair's inliers triangulated, [3, n]."""
    mappointdict = {fid: i for i, fid in enumerate(s["pt_feature"])}     # the snapshot of :154-156
    cam = {f: i for i, f in enumerate(s["cam_frame"])}
    c1, c2 = cam[pr["frame1"]], cam[pr["frame2"]]
    for i, (q, t) in enumerate(zip(pr["q"], pr["t"])):
        if not np.linalg.norm(X[:3, i]) <= max_norm:                      # :177 (NaN: kept out)
            continue
        fid = track_feature_back_in_time(s, (pr["frame2"], int(t)))
        if fid in mappointdict:                                           # add_new_observation_of_existing_point (:121-129)
            _observe(s, mappointdict[fid], c2, pr["p2"][i])
        else:                                                             # add_new_match_to_map (:101-119)
            s["pt_feature"].append((pr["frame1"], int(q))); s["points"].append(np.array(X[:3, i], np.float64))
            pt = len(s["points"]) - 1
            _observe(s, pt, c1, pr["p1"][i]); _observe(s, pt, c2, pr["p2"][i])


def freeze_nonlast_cameras(s, free_cameras=2):
    n = len(s["cam_fixed"])                                               # :270-275 (free_cameras = 2), unfreeze_cameras (:281-286)
    s["cam_fixed"] = [i < n - free_cameras for i in range(n)]


def optimize_map(s, K, iterations=40, delta=1.0, order=None):
    """map.py:104-186 through the numpy LM; writes poses and points back, returns lm's dict."""
    a = to_arrays(s)
    r = BA.lm(a["cam_pose"], a["cam_fixed"], a["points"], a["obs_cam"], a["obs_pt"], a["obs_xy"], K[0, 0], K[0, 2], K[1, 2],
              iterations=iterations, delta=delta, order=order)
    s["cam_pose"] = [T.copy() for T in r["poses"]]; s["points"] = [X.copy() for X in r["points"]]
    return r


def reprojection_keep(O, s, K, threshold):
    a = to_arrays(s)
    if len(a["obs_cam"]) == 0:
        return np.zeros(0, bool)
    T = np.zeros((len(a["cam_pose"]), 4, 4)); T[:, :3] = a["cam_pose"]; T[:, 3, 3] = 1
    return O.reprojection_sqerr(T, a["points"], a["obs_cam"], a["obs_pt"], a["obs_xy"], K, threshold)[1]


def remove_observations_above_threshold(O, s, K, threshold):
    keep = reprojection_keep(O, s, K, threshold)                          # map.py:46-70: sqerror < threshold stays
    for k in ("obs_cam", "obs_pt", "obs_xy"):
        s[k] = [v for v, f in zip(s[k], keep) if f]
    return keep


def remove_camera_from_map(s, c):
    """map.py:188-232.  Returns what it did: dict(points_removed, zero_observation_points_kept)."""
    keep_obs = [oc != c for oc in s["obs_cam"]]                           # :199-205
    count = {}                                                            # the defaultdict of :208-210: only points that still have one
    for oc, op, f in zip(s["obs_cam"], s["obs_pt"], keep_obs):
        if f:
            count[op] = count.get(op, 0) + 1
    gone = {pt for pt, n in count.items() if n < 2}                       # :213-216
    new_pt, k = {}, 0
    for pt in range(len(s["points"])):
        if pt not in gone:
            new_pt[pt] = k; k += 1
    obs = [(oc - (oc > c), new_pt[op], xy) for oc, op, xy, f in zip(s["obs_cam"], s["obs_pt"], s["obs_xy"], keep_obs) if f and op not in gone]
    s["obs_cam"], s["obs_pt"], s["obs_xy"] = [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs]
    n_pts = len(s["points"])
    s["pt_feature"] = [v for pt, v in enumerate(s["pt_feature"]) if pt not in gone]
    s["points"] = [v for pt, v in enumerate(s["points"]) if pt not in gone]
    for k in ("cam_frame", "cam_pose", "cam_fixed"):
        s[k] = [v for i, v in enumerate(s[k]) if i != c]
    return dict(points_removed=len(gone), zero_observation_points_kept=n_pts - len(count))


def limit_number_of_camera_in_map(s, max_cameras):
    if len(s["cam_frame"]) > max_cameras:                                 # map.py:299-318
        return remove_camera_from_map(s, 0)
    return None


def chi2_of(s, K, delta=1.0):
    a = to_arrays(s)
    e, _ = BA.residuals(a["cam_pose"], a["points"], a["obs_cam"].astype(np.int64), a["obs_pt"].astype(np.int64), a["obs_xy"], K[0, 0], K[0, 2], K[1, 2])
    return BA.seq_sum(BA.robust(e, delta)[0])


def step(O, state, pr, K, opts=None, follow=None, stages=False):
    """One frame of the reference from `state` (not modified).  Returns dict(state, status, n_corr, n_inl, pose_pnp, X, ba,
    evicted[, stage = {1..4: arrays}]).  follow: continue from this camera instead of the computed solvePnPRansac result
    (the device's, so that the comparison is on identical inputs)."""
    o = dict(DEFAULTS); o.update(opts or {})
    s = to_lists(state)
    out = dict(status=0, n_corr=0, n_inl=0, pose_pnp=None, X=None, ba=None, evicted=None, stage={})
    first = len(s["cam_frame"]) == 0
    update_feature_mapper(s, pr)
    if first:
        initialize_map(s, pr)
    else:
        mappointdict = {fid: i for i, fid in enumerate(s["pt_feature"])}
        obj, img = [], []                                                 # :201-227
        for t, kp2 in zip(pr["t"], pr["p2"]):
            fid = track_feature_back_in_time(s, (pr["frame2"], int(t)))
            if fid in mappointdict:
                obj.append(s["points"][mappointdict[fid]]); img.append(kp2)
        out["n_corr"] = len(obj)
        obj, img = np.array(obj).reshape(-1, 3), np.array(img).reshape(-1, 2)
        rc, rvec, tvec, _, ninl = O.solve_pnp_ransac(obj, img, K, o["iterations"], o["reproj_err"], o["confidence"], o["seed"]) if len(obj) >= 4 else (-3, None, None, None, 0)
        out["n_inl"] = int(ninl)
        if rc != 0:
            out["status"] = rc; out["state"] = s
            return out
        T2 = np.hstack([O.rodrigues(rvec), tvec.reshape(3, 1)])           # :243-249
        out["pose_pnp"] = T2
        if follow is not None:
            T2 = np.array(follow, np.float64).reshape(3, 4)
        T1 = s["cam_pose"][s["cam_frame"].index(pr["frame1"])]
        s["cam_frame"].append(pr["frame2"]); s["cam_pose"].append(T2); s["cam_fixed"].append(False)
        X = O.triangulate(_KP(K, T1), _KP(K, T2), np.array(pr["p1"]).reshape(-1, 2).T, np.array(pr["p2"]).reshape(-1, 2).T)   # :164-172
        X = X / X[3]
        out["X"] = X
        add_information_to_map(s, pr, X, o["max_point_norm"])
        freeze_nonlast_cameras(s, o["free_cameras"])
    if stages: out["stage"][1] = to_arrays(s)
    if o["ba_iterations"] > 0:
        out["ba"] = optimize_map(s, K, o["ba_iterations"], o["huber_delta"])
    if stages: out["stage"][2] = to_arrays(s)
    if not first and o["filter_threshold"] > 0:
        remove_observations_above_threshold(O, s, K, o["filter_threshold"])
    if stages: out["stage"][3] = to_arrays(s)
    out["evicted"] = limit_number_of_camera_in_map(s, o["max_cameras"])
    if stages: out["stage"][4] = to_arrays(s)
    out["state"] = s
    return out


def pair_inputs_from_oracle(O, feats, pairs, K):
    """Every pair's input from the oracle's front end, as reference_chain builds it."""
    out = []
    for k, (a, b) in enumerate(pairs):
        qi, ti, _ = O.match_hamming(feats[a]["desc"], feats[b]["desc"], 2)
        p1 = feats[a]["xy"][qi].astype(np.float64); p2 = feats[b]["xy"][ti].astype(np.float64)
        rc, E, mask, _ = O.find_essential_ransac(p1, p2, K)
        assert rc == 0
        inl = mask > 0
        pr = dict(frame1=k, frame2=k + 1, q=qi[inl], t=ti[inl], p1=p1[inl], p2=p2[inl])
        if k == 0:
            _, R, t, _ = O.recover_pose(E[0], p1[inl], p2[inl], K)
            X = O.triangulate(_KP(K, _inv_pose(R, t)), _KP(K, np.eye(3, 4)), p1[inl].T, p2[inl].T)
            pr.update(R=R, t_rel=t, X=X / X[3])
        out.append(pr)
    return out


def run(O, pair_inputs, K, opts=None):
    """The free-running chain.  Returns a list of step() results (the chain stops at the first failed pair)."""
    s, res = empty_state(), []
    for pr in pair_inputs:
        r = step(O, s, pr, K, opts)
        res.append(r)
        if r["status"] != 0:
            break
        s = r["state"]
    return res
