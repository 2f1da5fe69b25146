"""Map methods on the GPU.  Reprojection-error filter over all map observations (reference: src/map.py:46-94).

Also the map's bundle adjustment (reference: src/map.py:104-186, g2o) as one device call: bundle_adjust / optimize_map.

The reference walks Python lists of Observation / TrackedCamera / TrackedPoint objects and multiplies 4x4
matrices per observation; here the same quantities go to the GPU as arrays (one lane per observation).  The
object-level helpers accept the reference's record types unchanged (duck typed: .camera_id/.pose(),
.point_id/.point, .camera_id/.point_id/.image_coordinates)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


def reprojection_sqerr(poses, points, obs_cam, obs_pt, obs_xy, camera_matrix, threshold=100.0, ctx=None):
    """Arrays in, (sqerr [N] float64, keep [N] bool) out. obs_cam / obs_pt index rows of poses / points."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32)
    xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(camera_matrix, np.float64).reshape(3, 3)
    n = len(oc)
    if not (len(op) == n == len(xy)):
        raise ValueError("observation arrays differ in length")
    err = np.zeros(n); keep = np.zeros(n, np.uint8)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_reprojection_filter(ctx.handle, poses.ctypes.data, len(poses), points.ctypes.data, len(points),
                                             oc.ctypes.data, op.ctypes.data, xy.ctypes.data, n, K.ctypes.data,
                                             float(threshold), err.ctypes.data, keep.ctypes.data))
    return err, keep.astype(bool)


def _index_arrays(cameras, points, observations):
    cam_row = {c.camera_id: i for i, c in enumerate(cameras)}
    pt_row = {p.point_id: i for i, p in enumerate(points)}
    pts = np.array([p.point for p in points], dtype=np.float64).reshape(-1, 3)
    oc = np.array([cam_row[o.camera_id] for o in observations], np.int32)
    op = np.array([pt_row[o.point_id] for o in observations], np.int32)
    xy = np.array([o.image_coordinates for o in observations], dtype=np.float64).reshape(-1, 2)
    return pts, oc, op, xy


def _arrays(cameras, points, observations):
    poses = np.stack([c.pose() for c in cameras]) if cameras else np.zeros((0, 4, 4))
    return (poses,) + _index_arrays(cameras, points, observations)


def remove_observations_with_reprojection_errors_above_threshold(cameras, points, observations, camera_matrix,
                                                                 threshold=100, ctx=None):
    """map.py:46-68 — returns the observations whose squared reprojection error is below the threshold."""
    if not observations:
        return []
    _, keep = reprojection_sqerr(*_arrays(cameras, points, observations), camera_matrix, threshold, ctx)
    return [o for o, k in zip(observations, keep) if k]


def calculate_reprojection_error(cameras, points, observations, camera_matrix, ctx=None):
    """map.py:70-94 — total squared reprojection error, summed in observation order."""
    if not observations:
        return 0.0
    err, _ = reprojection_sqerr(*_arrays(cameras, points, observations), camera_matrix, np.inf, ctx)
    total = 0.0
    for e in err.tolist():
        total += e
    return total


def map_statistics(poses, points, obs_cam, obs_pt, obs_xy, camera_matrix, high_threshold=10.0, ctx=None):
    """map.py:234-297 — Map.show_map_statistics as numbers, in one device call (vo_map_statistics); nothing is printed.  Arrays as
    reprojection_sqerr takes them (poses [ncam, 4, 4]).  Returns dict(n_cam, n_pts, n_obs (the three list lengths), total_sqerr
    (calculate_reprojection_error: the sum in observation order), mean_sqerr (total / n_obs, 0.0 without observations), max_sqerr,
    n_high (observations with sqerr > high_threshold), obs_hist [64] (points by number of observations; bin 63 = 63 or more, bin 0 =
    none), obs_matrix [ncam, ncam] (points two cameras see together, upper triangle, by position in the camera list)).
    More than 64 cameras raise NotImplementedError, an observation of a missing camera or point VoError."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    oc = np.ascontiguousarray(obs_cam, np.int32).ravel(); op = np.ascontiguousarray(obs_pt, np.int32).ravel()
    xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(camera_matrix, np.float64).reshape(3, 3)
    n = len(oc)
    if not (len(op) == n == len(xy)):
        raise ValueError("observation arrays differ in length")
    total, mx, nh = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int32(0)
    hist = np.zeros(_lib.VO_STATS_HIST, np.int32); mat = np.zeros((len(poses), len(poses)), np.int32)
    ctx = ctx or _lib.default_context()
    rc = ctx.lib.vo_map_statistics(ctx.handle, _lib.ptr(poses), len(poses), _lib.ptr(points), len(points), _lib.ptr(oc), _lib.ptr(op), _lib.ptr(xy), n,
                                   K.ctypes.data, float(high_threshold), ctypes.addressof(total), ctypes.addressof(mx), ctypes.addressof(nh),
                                   hist.ctypes.data, _lib.ptr(mat))
    if rc == _lib.VO_ERR_UNSUPPORTED:
        raise NotImplementedError(ctx.last_error())
    ctx.check(rc)
    return dict(n_cam=len(poses), n_pts=len(points), n_obs=n, total_sqerr=total.value, mean_sqerr=total.value / n if n > 0 else 0.0,
                max_sqerr=mx.value, n_high=nh.value, obs_hist=hist, obs_matrix=mat)


def show_map_statistics(cameras, points, observations, camera_matrix, ctx=None):
    """map.py:234-297 on the reference's record types (duck typed, as the functions above): the dict map_statistics returns."""
    return map_statistics(*_arrays(cameras, points, observations), camera_matrix, 10.0, ctx)


def feature_tracks(n_frames, cap, pair_frames, matches, ctx=None):
    """update_feature_mapper + track_feature_back_in_time (visual_slam.py:183-188, :94-99) for every feature at once.

    pair_frames: [P, 2] frame ids (f1, f2); matches: list of P (q_idx, t_idx) int arrays — the matches with 3-D
    information of each pair, in the order the reference would process the pairs.  Returns (root_frame, root_idx,
    hops), each [n_frames, cap]: feature (f, i) traces back to (root_frame[f, i], root_idx[f, i])."""
    pf = np.ascontiguousarray(pair_frames, np.int32).reshape(-1, 2)
    P = len(pf)
    off = np.zeros(P + 1, np.int32)
    for p, (q, t) in enumerate(matches):
        if len(q) != len(t):
            raise ValueError("q and t differ in length")
        off[p + 1] = off[p] + len(q)
    mq = np.ascontiguousarray(np.concatenate([np.asarray(q, np.int32) for q, _ in matches]) if P else np.zeros(0, np.int32))
    mt = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32) for _, t in matches]) if P else np.zeros(0, np.int32))
    rf = np.zeros((n_frames, cap), np.int32); ri = np.zeros((n_frames, cap), np.int32); hops = np.zeros((n_frames, cap), np.int32)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_feature_tracks(ctx.handle, int(n_frames), int(cap), pf.ctypes.data, off.ctypes.data, mq.ctypes.data,
                                        mt.ctypes.data, P, rf.ctypes.data, ri.ctypes.data, hops.ctypes.data))
    return rf, ri, hops


def _ba_problem(poses, fixed, points, obs_cam, obs_pt, obs_xy):
    poses = np.array(poses, np.float64).reshape(-1, 12)
    fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8)).ravel()
    points = np.array(points, np.float64).reshape(-1, 3)
    oc = np.ascontiguousarray(obs_cam, np.int32).ravel(); op = np.ascontiguousarray(obs_pt, np.int32).ravel()
    xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    if len(fixed) != len(poses):
        raise ValueError("one fixed flag per camera")
    if not (len(op) == len(oc) == len(xy)):
        raise ValueError("observation arrays differ in length")
    return poses, fixed, points, oc, op, xy


def bundle_adjust_batch(problems, focal, cx, cy, iterations=40, huber_delta=1.0, ctx=None):
    """Map.optimize_map (map.py:104-186) for B independent maps in one launch, one workgroup each.  problems: a list of
    (poses [ncam, 3, 4] world -> camera [R | t], fixed [ncam], points [npt, 3], obs_cam, obs_pt, obs_xy [nobs, 2]) with
    obs_cam / obs_pt indexing that problem's rows.  Returns one dict per problem: poses, points (new arrays), chi2_before,
    chi2_after (g2o's activeRobustChi2), iterations, trials, status (VO_OK; VO_ERR_UNSUPPORTED beyond 64 cameras / 16 free
    cameras, VO_ERR_INVALID for an observation of a missing camera or point: such a problem comes back unchanged)."""
    probs = [_ba_problem(*p) for p in problems]
    B = len(probs)
    off = np.zeros((3, B + 1), np.int32)
    for b, p in enumerate(probs):
        off[:, b + 1] = off[:, b] + (len(p[0]), len(p[2]), len(p[3]))
    cat = lambda k, shape, dt: np.ascontiguousarray(np.concatenate([p[k] for p in probs]) if B else np.zeros(shape, dt))  # noqa: E731
    poses, fixed, points = cat(0, (0, 12), np.float64), cat(1, 0, np.uint8), cat(2, (0, 3), np.float64)
    oc, op, xy = cat(3, 0, np.int32), cat(4, 0, np.int32), cat(5, (0, 2), np.float64)
    chi2 = np.zeros((B, 2)); it = np.zeros(B, np.int32); tr = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
    opts = _lib.BaOpts(int(iterations), 0, float(huber_delta))
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_bundle_adjust_batch(ctx.handle, B, off[0].ctypes.data, off[1].ctypes.data, off[2].ctypes.data, poses.ctypes.data,
                                             fixed.ctypes.data, points.ctypes.data, oc.ctypes.data, op.ctypes.data, xy.ctypes.data,
                                             float(focal), float(cx), float(cy), ctypes.addressof(opts), chi2.ctypes.data,
                                             it.ctypes.data, tr.ctypes.data, st.ctypes.data))
    return [dict(poses=poses[off[0, b]:off[0, b + 1]].reshape(-1, 3, 4).copy(), points=points[off[1, b]:off[1, b + 1]].copy(),
                 chi2_before=float(chi2[b, 0]), chi2_after=float(chi2[b, 1]), iterations=int(it[b]), trials=int(tr[b]),
                 status=int(st[b])) for b in range(B)]


def bundle_adjust(poses, fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, iterations=40, huber_delta=1.0, ctx=None):
    """One map (vo_bundle_adjust): dict(poses, points, chi2_before, chi2_after, iterations, trials, status).  A map the
    kernel cannot hold or an observation of a missing camera / point raises VoError; the inputs are not modified."""
    poses, fixed, points, oc, op, xy = _ba_problem(poses, fixed, points, obs_cam, obs_pt, obs_xy)
    chi2 = np.zeros(2); it = np.zeros(1, np.int32); tr = np.zeros(1, np.int32)
    opts = _lib.BaOpts(int(iterations), 0, float(huber_delta))
    ctx = ctx or _lib.default_context()
    rc = ctx.check(ctx.lib.vo_bundle_adjust(ctx.handle, poses.ctypes.data, fixed.ctypes.data, len(poses), points.ctypes.data, len(points),
                                            oc.ctypes.data, op.ctypes.data, xy.ctypes.data, len(oc), float(focal), float(cx), float(cy),
                                            ctypes.addressof(opts), chi2.ctypes.data, it.ctypes.data, tr.ctypes.data))
    return dict(poses=poses.reshape(-1, 3, 4), points=points, chi2_before=float(chi2[0]), chi2_after=float(chi2[1]),
                iterations=int(it[0]), trials=int(tr[0]), status=int(rc))


def optimize_map(cameras, points, observations, camera_matrix, iterations=40, ctx=None):
    """map.py:104-186 — Map.optimize_map: cameras need .camera_id, .R, .t, .fixed; points .point_id, .point; observations
    .camera_id, .point_id, .image_coordinates.  One focal length, camera_matrix[0, 0], as the reference passes it (:113).
    Writes camera.t (a 3-vector), camera.R and point.point (a fresh array) back as :175-186 do; returns (chi2 before, after)."""
    K = np.asarray(camera_matrix, np.float64).reshape(3, 3)
    pts, oc, op, xy = _index_arrays(cameras, points, observations)
    poses = np.zeros((len(cameras), 3, 4))
    for i, c in enumerate(cameras):
        poses[i, :, :3] = np.asarray(c.R, np.float64).reshape(3, 3); poses[i, :, 3] = np.asarray(c.t, np.float64).ravel()
    r = bundle_adjust(poses, [bool(c.fixed) for c in cameras], pts, oc, op, xy, K[0, 0], K[0, 2], K[1, 2], iterations, 1.0, ctx)
    for i, c in enumerate(cameras):
        c.t = r["poses"][i, :, 3].copy()
        c.R = r["poses"][i, :, :3].copy()
    for i, p in enumerate(points):
        p.point = np.copy(r["points"][i])
    return r["chi2_before"], r["chi2_after"]


def bundle_adjust_large(poses, fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, iterations=40, huber_delta=1.0, ctx=None):
    """One map of hundreds of cameras (vo_bundle_adjust_large): bundle_adjust's arguments, rules and dict, with the reduced
    camera system factored in device memory by a blocked Cholesky over the whole GPU.  At most _lib.VO_BA_LARGE_MAX_FREE free
    cameras, any number of fixed ones.  A map beyond that or an observation of a missing camera / point raises VoError; the
    inputs are not modified."""
    poses, fixed, points, oc, op, xy = _ba_problem(poses, fixed, points, obs_cam, obs_pt, obs_xy)
    chi2 = np.zeros(2); it = np.zeros(1, np.int32); tr = np.zeros(1, np.int32)
    opts = _lib.BaOpts(int(iterations), 0, float(huber_delta))
    ctx = ctx or _lib.default_context()
    rc = ctx.check(ctx.lib.vo_bundle_adjust_large(ctx.handle, poses.ctypes.data, fixed.ctypes.data, len(poses), points.ctypes.data, len(points),
                                                  oc.ctypes.data, op.ctypes.data, xy.ctypes.data, len(oc), float(focal), float(cx), float(cy),
                                                  ctypes.addressof(opts), chi2.ctypes.data, it.ctypes.data, tr.ctypes.data))
    return dict(poses=poses.reshape(-1, 3, 4), points=points, chi2_before=float(chi2[0]), chi2_after=float(chi2[1]),
                iterations=int(it[0]), trials=int(tr[0]), status=int(rc))


def ba_large_solve(A, b, want_factor=False, ctx=None):
    """A x = b by bundle_adjust_large's blocked Cholesky (vo_ba_large_solve): A symmetric positive definite, n x n with n = 6 F,
    1 <= F <= _lib.VO_BA_LARGE_MAX_FREE, of which the lower triangle is used.  dict(x, y, pivot_failed) and, with want_factor,
    L (upper triangle zero); after a failed pivot x, y and L are None."""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64).ravel()
    n = len(b)
    if A.shape != (n, n):
        raise ValueError(f"A must be {n} x {n}, got {A.shape}")
    x = np.zeros(n); y = np.zeros(n); L = np.zeros((n, n)) if want_factor else None
    failed = np.zeros(1, np.int32)
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_ba_large_solve(ctx.handle, A.ctypes.data, b.ctypes.data, n, x.ctypes.data, L.ctypes.data if want_factor else None,
                                        y.ctypes.data, failed.ctypes.data))
    out = dict(x=None, y=None, pivot_failed=bool(failed[0])) if failed[0] else dict(x=x, y=y, pivot_failed=False)
    if want_factor:
        out["L"] = None if failed[0] else L
    return out


def optimize_map_large(cameras, points, observations, camera_matrix, iterations=40, ctx=None):
    """optimize_map for a map beyond vo_bundle_adjust's capacity: the same duck typing and write-back, through bundle_adjust_large."""
    K = np.asarray(camera_matrix, np.float64).reshape(3, 3)
    pts, oc, op, xy = _index_arrays(cameras, points, observations)
    poses = np.zeros((len(cameras), 3, 4))
    for i, c in enumerate(cameras):
        poses[i, :, :3] = np.asarray(c.R, np.float64).reshape(3, 3); poses[i, :, 3] = np.asarray(c.t, np.float64).ravel()
    r = bundle_adjust_large(poses, [bool(c.fixed) for c in cameras], pts, oc, op, xy, K[0, 0], K[0, 2], K[1, 2], iterations, 1.0, ctx)
    for i, c in enumerate(cameras):
        c.t = r["poses"][i, :, 3].copy()
        c.R = r["poses"][i, :, :3].copy()
    for i, p in enumerate(points):
        p.point = np.copy(r["points"][i])
    return r["chi2_before"], r["chi2_after"]


def _pgo_problem(sims, fixed, edges, meas, info=None):
    sims = np.array(sims, np.float64).reshape(-1, 13)
    fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8)).ravel()
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 13)
    info = np.ones((len(edges), 7)) if info is None else np.ascontiguousarray(info, np.float64).reshape(-1, 7)
    if len(fixed) != len(sims):
        raise ValueError("one fixed flag per vertex")
    if not (len(edges) == len(meas) == len(info)):
        raise ValueError("edge arrays differ in length")
    return sims, fixed, edges, meas, info


def optimize_pose_graph_batch(problems, iterations=10, huber_delta=0.0, ctx=None):
    """Sim(3) pose-graph optimisation (include/vo_hip.h, "pose graph") of B independent graphs in one launch, one workgroup each.
    problems: a list of (sims [nv, 13] = s, R row-major, t of world -> camera, fixed [nv], edges [ne, 2] indexing that graph's rows,
    meas [ne, 13], info [ne, 7] or None = all weights 1).  Returns one dict per problem: sims (a new array), chi2_initial, chi2_final,
    iterations, trials, status (VO_OK; VO_ERR_UNSUPPORTED beyond 8192 vertices / 32 loop edges; VO_ERR_INVALID for a bad index, an
    edge from a vertex to itself, a weight that is not positive, a vertex that reaches no fixed vertex: such a graph comes back unchanged).
    iterations outside 1 .. 1000 raise VoError for the call."""
    probs = [_pgo_problem(*p) for p in problems]
    B = len(probs)
    off = np.zeros((2, B + 1), np.int32)
    for b, p in enumerate(probs):
        off[:, b + 1] = off[:, b] + (len(p[0]), len(p[2]))
    cat = lambda k, shape, dt: np.ascontiguousarray(np.concatenate([p[k] for p in probs]) if B else np.zeros(shape, dt))  # noqa: E731
    sims, fixed, edges, meas, info = cat(0, (0, 13), np.float64), cat(1, 0, np.uint8), cat(2, (0, 2), np.int32), cat(3, (0, 13), np.float64), cat(4, (0, 7), np.float64)
    chi2 = np.zeros((B, 2)); it = np.zeros(B, np.int32); tr = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
    opts = _lib.PgoOpts(int(iterations), float(huber_delta))
    ctx = ctx or _lib.default_context()
    ctx.check(ctx.lib.vo_pose_graph_batch(ctx.handle, B, off[0].ctypes.data, off[1].ctypes.data, sims.ctypes.data, fixed.ctypes.data,
                                          edges.ctypes.data, meas.ctypes.data, info.ctypes.data, ctypes.addressof(opts), chi2.ctypes.data,
                                          it.ctypes.data, tr.ctypes.data, st.ctypes.data))
    return [dict(sims=sims[off[0, b]:off[0, b + 1]].copy(), chi2_initial=float(chi2[b, 0]), chi2_final=float(chi2[b, 1]),
                 iterations=int(it[b]), trials=int(tr[b]), status=int(st[b])) for b in range(B)]


def optimize_pose_graph(sims, fixed, edges, meas, info=None, iterations=10, huber_delta=0.0, ctx=None):
    """One graph (vo_pose_graph): dict(sims, chi2_initial, chi2_final, iterations, trials, status).  A graph over capacity raises
    NotImplementedError, an invalid one VoError, as do iterations outside 1 .. 1000; the inputs are not modified.  frontend.track_vertices, odometry_edges and loop_edge
    build the arguments, frontend.vertices_to_poses and correct_points take the result back."""
    sims, fixed, edges, meas, info = _pgo_problem(sims, fixed, edges, meas, info)
    chi2 = np.zeros(2); it = np.zeros(1, np.int32); tr = np.zeros(1, np.int32)
    opts = _lib.PgoOpts(int(iterations), float(huber_delta))
    ctx = ctx or _lib.default_context()
    rc = ctx.lib.vo_pose_graph(ctx.handle, sims.ctypes.data, fixed.ctypes.data, len(sims), edges.ctypes.data, meas.ctypes.data,
                               info.ctypes.data, len(edges), ctypes.addressof(opts), chi2.ctypes.data, it.ctypes.data, tr.ctypes.data)
    if rc == _lib.VO_ERR_UNSUPPORTED:
        raise NotImplementedError(ctx.last_error())
    ctx.check(rc)
    return dict(sims=sims, chi2_initial=float(chi2[0]), chi2_final=float(chi2[1]), iterations=int(it[0]), trials=int(tr[0]), status=int(rc))
