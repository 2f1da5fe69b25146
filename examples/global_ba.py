#!/usr/bin/env python3
"""The whole loop-closing back end on one synthetic flight, no images: pose graph, map correction, then a bundle adjustment of the
whole corrected map on the device (map_filters.bundle_adjust_large).

    python examples/global_ba.py [--frames 100] [--landmarks 3000] [--drift 0.01] [--seed 0]

The course is examples/close_loop.py's circle, flown once, the cameras looking outwards at a ring of landmarks.  The track is dead
reckoning with noise and `--drift` scale drift per step.  Every landmark was triangulated in the gauge of the first camera that saw
it, so the map drifts with the track.
  1. One loop constraint between the first and the last frame (the truth's relative pose, as align_maps would measure it) and
     map_filters.optimize_pose_graph.
  2. frontend.vertices_to_poses for the cameras and frontend.correct_points for every landmark, with its first camera's vertex.
  3. map_filters.bundle_adjust_large over all cameras, points and observations, the first two cameras fixed.
Printed after each stage: the robust chi2 of all observations (Huber, delta = 1 px) and the mean distance between camera centres
and ground truth."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_odometry_amd import frontend as F, map_filters  # noqa: E402

FOCAL, CX, CY = 802.832, 565.427, 240.124


def course(n, radius=10.0):
    """world -> camera similarities (s = 1) on a circle, looking outwards"""
    out = np.empty((n, 13))
    for i in range(n):
        a = 2 * np.pi * i / n
        R = np.array([[-np.sin(a), 0, np.cos(a)], [np.cos(a), 0, np.sin(a)], [0, 1.0, 0]]).T
        c = np.array([radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(3 * a)])
        out[i] = np.r_[1.0, R.ravel(), -R @ c]
    return out


def apply(S, X):
    return S[0] * (X @ S[1:10].reshape(3, 3).T) + S[10:13]


def centres(poses):
    return -np.einsum("nji,nj->ni", poses[:, :, :3], poses[:, :, 3])


def aligned_error(c, truth):
    """mean distance after the least-squares similarity (Umeyama) that takes the centres c onto the truth: the error of the map's
    shape, whatever gauge and scale the two fixed cameras gave it"""
    mc, mt = c.mean(0), truth.mean(0)
    U, d, Vt = np.linalg.svd((truth - mt).T @ (c - mc) / len(c))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = (d * np.diag(D)).sum() / ((c - mc) ** 2).sum(1).mean()
    return float(np.linalg.norm(s * (c - mc) @ R.T + mt - truth, axis=1).mean())


def robust_chi2(poses, points, oc, op, xy, delta=1.0):
    q = np.einsum("nij,nj->ni", poses[oc, :, :3], points[op]) + poses[oc, :, 3]
    e = xy - np.c_[FOCAL * q[:, 0] / q[:, 2] + CX, FOCAL * q[:, 1] / q[:, 2] + CY]
    e2 = (e * e).sum(1); s = np.sqrt(e2)
    return float(np.where(s > delta, 2 * delta * s - delta * delta, e2).sum())


def flight(frames, landmarks, drift, seed):
    """truth and drifted track (vertices), observations of the truth, and the map as the drifted track triangulated it"""
    rng = np.random.default_rng(seed)
    truth = course(frames)
    track = truth.copy()
    for i in range(1, frames):
        step = F.sim3_compose(truth[i], F.sim3_inverse(truth[i - 1]))
        err = F.sim3_exp(np.r_[rng.normal(0, 0.002, 3), rng.normal(0, 0.01, 3), drift])
        track[i] = F.sim3_compose(F.sim3_compose(err, step), track[i - 1])
    ang, rad = rng.uniform(0, 2 * np.pi, landmarks), rng.uniform(15, 22, landmarks)
    world = np.c_[rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-2.5, 2.5, landmarks)]
    oc, op, xy = [], [], []
    for i in range(frames):
        q = apply(truth[i], world)
        u, v = FOCAL * q[:, 0] / q[:, 2] + CX, FOCAL * q[:, 1] / q[:, 2] + CY
        seen = np.flatnonzero((q[:, 2] > 3) & (q[:, 2] < 14) & (u > 0) & (u < 2 * CX) & (v > 0) & (v < 2 * CY))
        oc.append(np.full(len(seen), i)); op.append(seen); xy.append(np.c_[u[seen], v[seen]] + rng.normal(0, 0.5, (len(seen), 2)))
    oc, op, xy = np.concatenate(oc), np.concatenate(op), np.concatenate(xy)
    views = np.bincount(op, minlength=landmarks)
    keep = np.flatnonzero(views >= 3)                                   # the map holds what three cameras saw
    renum = -np.ones(landmarks, np.int64); renum[keep] = np.arange(len(keep))
    sel = renum[op] >= 0
    oc, op, xy = oc[sel].astype(np.int32), renum[op[sel]].astype(np.int32), xy[sel]
    first = np.full(len(keep), frames, np.int64)
    np.minimum.at(first, op, oc)                                        # the camera that triangulated the point
    points = np.empty((len(keep), 3))
    for a in np.unique(first):
        m = first == a
        points[m] = apply(F.sim3_inverse(track[a]), apply(truth[a], world[keep][m])) + rng.normal(0, 0.01, (int(m.sum()), 3))
    return dict(truth=truth, track=track, oc=oc, op=op, xy=xy, points=points, first=first)


def run(frames=100, landmarks=3000, drift=0.01, seed=0, iterations=10, out=print):
    fl = flight(frames, landmarks, drift, seed)
    truth, track, oc, op, xy = fl["truth"], fl["track"], fl["oc"], fl["op"], fl["xy"]
    true_centres = centres(F.vertices_to_poses(truth))
    stages = []

    def report(name, poses, points):
        st = dict(name=name, chi2=robust_chi2(poses, points, oc, op, xy), centre_error=float(np.linalg.norm(centres(poses) - true_centres, axis=1).mean()),
                  aligned_error=aligned_error(centres(poses), true_centres))
        stages.append(st)
        out(f"{name:<22} chi2 {st['chi2']:.6g}   mean camera-centre error {st['centre_error']:.4f}   after a similarity fit {st['aligned_error']:.4f}")

    out(f"{frames} cameras, {len(fl['points'])} points, {len(oc)} observations")
    report("dead reckoning", F.vertices_to_poses(track), fl["points"])
    # 1. the loop: the last frame as seen from the first
    edges, meas = F.odometry_edges(track)
    observed = F.sim3_compose(F.sim3_compose(truth[frames - 1], F.sim3_inverse(truth[0])), track[0])
    edges = np.vstack([edges, [[0, frames - 1]]]).astype(np.int32)
    meas = np.vstack([meas, F.loop_edge(track[0], observed)[None]])
    fixed = np.zeros(frames, np.uint8); fixed[0] = 1
    pg = map_filters.optimize_pose_graph(track, fixed, edges, meas, iterations=10)
    # 2. cameras and map into the corrected gauge
    poses = F.vertices_to_poses(pg["sims"])
    points = fl["points"].copy()
    for a in np.unique(fl["first"]):
        m = fl["first"] == a
        points[m] = F.correct_points(points[m], track[a], pg["sims"][a])
    report("pose graph + map", poses, points)
    # 3. bundle adjustment of the whole map
    ba_fixed = np.zeros(frames, bool); ba_fixed[:2] = True
    ba = map_filters.bundle_adjust_large(poses, ba_fixed, points, oc, op, xy, FOCAL, CX, CY, iterations=iterations)
    report("bundle adjustment", ba["poses"], ba["points"])
    out(f"bundle adjustment: {int((~ba_fixed).sum())} free cameras, chi2 {ba['chi2_before']:.6g} -> {ba['chi2_after']:.6g} in {ba['iterations']} iterations, {ba['trials']} trials")
    return stages, ba


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--landmarks", type=int, default=3000)
    ap.add_argument("--drift", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=10)
    a = ap.parse_args()
    run(a.frames, a.landmarks, a.drift, a.seed, a.iterations)


if __name__ == "__main__":
    main()
