#!/usr/bin/env python3
"""A loop closure used: a drifted monocular track on a closed course, corrected by the device pose-graph optimisation.

    python examples/close_loop.py [--frames 80] [--drift 0.01] [--loops 3] [--seed 0]

The course is a circle flown once, so its last frames see the ground of its first.  The track is dead reckoning from odometry with
noise and `--drift` scale drift per step: what the restart walks and join_segments hand over, every frame in the gauge of the first.
Where the course overlaps, the map around an early frame i and the map around a late frame j hold the same landmarks, each in the
gauge its own stretch of the track gave it.  The similarity between the two is what FrontEnd.align_maps measures from the maps'
descriptor rows; here the correspondences are given, so its RANSAC alone runs (geometry.estimate_similarity, the same kernel).  That
similarity says where frame j lies as seen from frame i's stretch (loop_edge), the odometry gives the chain edges (odometry_edges), and
map_filters.optimize_pose_graph distributes the contradiction over all frames.  Printed: the mean distance between camera centres and
ground truth before and after."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_odometry_amd import frontend as F, geometry, map_filters  # noqa: E402


def course(n, radius=10.0):
    """world -> camera similarities (s = 1) on a circle, looking along the tangent"""
    out = np.empty((n, 13))
    for i in range(n):
        a = 2 * np.pi * i / n
        R = np.array([[-np.sin(a), 0, np.cos(a)], [np.cos(a), 0, np.sin(a)], [0, 1.0, 0]]).T
        c = np.array([radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(3 * a)])
        out[i] = np.r_[1.0, R.ravel(), -R @ c]
    return out


def apply(S, X):
    return S[0] * (X @ S[1:10].reshape(3, 3).T) + S[10:13]


def centres(V):
    P = F.vertices_to_poses(V)
    return -np.einsum("nji,nj->ni", P[:, :, :3], P[:, :, 3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--drift", type=float, default=0.01)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    n = a.frames
    truth = course(n)
    track = truth.copy()                                  # dead reckoning: every step carries noise and scale drift
    for i in range(1, n):
        step = F.sim3_compose(truth[i], F.sim3_inverse(truth[i - 1]))
        err = F.sim3_exp(np.r_[rng.normal(0, 0.002, 3), rng.normal(0, 0.01, 3), a.drift])
        track[i] = F.sim3_compose(F.sim3_compose(err, step), track[i - 1])
    edges, meas = F.odometry_edges(track)

    landmarks = np.c_[rng.uniform(-14, 14, 4000), rng.uniform(-14, 14, 4000), rng.uniform(-2, 2, 4000)]
    for k in range(a.loops):                              # frame i of the first stretch and frame j of the last see the same ground
        i, j = 2 * k, n - 1 - 2 * k
        seen = np.flatnonzero((np.linalg.norm(landmarks - centres(truth[i:i + 1]), axis=1) < 6) & (np.linalg.norm(landmarks - centres(truth[j:j + 1]), axis=1) < 6))
        map_i = apply(F.sim3_inverse(track[i]), apply(truth[i], landmarks[seen])) + rng.normal(0, 0.005, (len(seen), 3))
        map_j = apply(F.sim3_inverse(track[j]), apply(truth[j], landmarks[seen])) + rng.normal(0, 0.005, (len(seen), 3))
        sim = geometry.estimate_similarity(map_j, map_i, max_error=0.05)          # X_i = s R X_j + t, as align_maps returns it
        if sim["status"] != 0:
            print(f"loop {i} - {j}: no similarity from {len(seen)} landmarks")
            continue
        A = np.r_[sim["scale"], sim["R"].ravel(), sim["t"]]
        observed = F.sim3_compose(track[j], F.sim3_inverse(A))                     # frame j in the gauge of frame i's stretch
        edges = np.vstack([edges, [[i, j]]]).astype(np.int32)
        meas = np.vstack([meas, F.loop_edge(track[i], observed)[None]])
        print(f"loop {i} - {j}: {len(seen)} landmarks, {sim['n_inl']} inliers, scale {sim['scale']:.4f}")

    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    r = map_filters.optimize_pose_graph(track, fixed, edges, meas, iterations=10)
    before = np.linalg.norm(centres(track) - centres(truth), axis=1).mean()
    after = np.linalg.norm(centres(r["sims"]) - centres(truth), axis=1).mean()
    print(f"pose graph: {n} vertices, {len(edges)} edges, chi2 {r['chi2_initial']:.4g} -> {r['chi2_final']:.4g} in {r['iterations']} iterations, {r['trials']} trials")
    print(f"mean distance between camera centres and ground truth: {before:.4f} before, {after:.4f} after")


if __name__ == "__main__":
    main()
