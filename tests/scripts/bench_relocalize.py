#!/usr/bin/env python3
"""vo_map_localize against the only way to do the same work without it (docs/kernels/k_nn_map.md, Measured):
    python tests/scripts/bench_relocalize.py [--reps 7] [--inner 25] [--maps 4096,32768]
Q = 64 SIFT slots of 3500 staged rows (kp_cap 3584) against staged maps of 4096 and 32768 points.  Every frame sees 3500 of the
map's points from a pose of its own: their rows with a few elements nudged, float32 projections, 10 % of them at a wrong pixel.
  resident   one FrontEnd.relocalize call for the 64 slots: wall time around the synchronous call, and the split match_nn
             (k_nn_map) / match_select (k_map_select) / misc (k_pnp_ransac + poses) from the stage brackets, in a run of its own;
  host path  what a caller could do before: download every slot's features, vo_match_l2(crossCheck) per frame against the map's
             rows, gather the correspondences with numpy, one vo_solve_pnp_ransac_batch for the 64 frames.
Both paths are warmed up on the shape they are timed on and must agree (matches equal, poses byte for byte) before a time is
printed.  Times are the median and the range over --reps repetitions — of the mean of --inner back-to-back calls for the resident
path, whose single call is too short a window — and rates are frames per second of wall time."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import relocalize_reference as R  # noqa: E402
from visual_odometry_amd import geometry  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402
from visual_odometry_amd.matcher import L2Matcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=25, help="resident calls per timed window (a single call is a few ms: too short a window)")
ap.add_argument("--maps", default="4096,32768")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--rows", type=int, default=3500)
args = ap.parse_args()
Q, N = args.frames, args.rows
fe = FrontEnd(32, 32, max_frames=Q, max_pairs=Q, detector="sift", kp_cap=N)
print(f"{Q} SIFT slots x {N} rows (kp_cap {fe.kp_cap})")


def scene(npt, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (npt, 3))
    rows = R.rand_rows(rng, npt, "sift")
    frames = []
    for q in range(Q):
        Rm = R.rotation(rng.normal(size=3), rng.uniform(0.05, 0.4)); t = np.array([0.3, -0.2, 6.0]) + rng.normal(0, 0.3, 3)
        ids = rng.choice(npt, min(N, npt), replace=False)
        Xc = X[ids] @ Rm.T + t
        uv = ((Xc / Xc[:, 2:]) @ R.K.T)[:, :2]
        wrong = rng.random(len(ids)) < 0.1
        uv[wrong] += rng.uniform(40, 120, (int(wrong.sum()), 2))
        f = rows[ids].copy()
        f[:, :4] += rng.integers(0, 2, (len(ids), 4), dtype=np.uint8)        # a few elements off by one: near, not equal
        frames.append((f, uv.astype(np.float32), Rm, t))
    return X, rows, frames


def spread(ts):
    ts = sorted(ts)
    return f"{1e3 * ts[len(ts) // 2]:.2f} ms (range {1e3 * ts[0]:.2f} .. {1e3 * ts[-1]:.2f}, {len(ts)} reps)"


def host_path(map_rows_f32, X):
    """download -> vo_match_l2 per frame -> numpy gather -> one vo_solve_pnp_ransac_batch"""
    matcher = L2Matcher(crossCheck=True, ctx=fe.ctx)
    objs, imgs, off, ms = [], [], [0], []
    for q in range(Q):
        ft = fe.features(q)
        qi, ti, d = matcher.match_arrays(ft["desc"], map_rows_f32)
        objs.append(X[ti]); imgs.append(ft["xy"][qi].astype(np.float64)); off.append(off[-1] + len(qi)); ms.append((qi, ti, d))
    st, rvec, tvec, mask, ninl = geometry.solve_pnp_ransac_batch(np.concatenate(objs), np.concatenate(imgs), np.array(off, np.int32), R.K, ctx=fe.ctx)
    poses = np.zeros((Q, 3, 4))
    for q in range(Q):
        if st[q] == 0:
            poses[q] = np.hstack([geometry.Rodrigues(rvec[q], ctx=fe.ctx)[0], tvec[q].reshape(3, 1)])
    return poses, st, ms


for npt in [int(v) for v in args.maps.split(",")]:
    X, rows, frames = scene(npt, 1000 + npt)
    for q, (f, xy, _, _) in enumerate(frames):
        fe.set_sift_rows(q, f, xy)
    t0 = time.perf_counter(); fe.stage_map(rows, X); t_stage = time.perf_counter() - t0
    slots = np.arange(Q, dtype=np.int32)
    out = fe.relocalize(slots, R.K)                                           # warm-up, and the result both paths must give
    rows_f32 = rows.astype(np.float32)
    poses, st, ms = host_path(rows_f32, X)                                    # warm-up of the host path
    assert np.array_equal(st, out["status"]) and poses.tobytes() == out["poses"].tobytes(), "the two paths disagree"
    for q in (0, Q - 1):
        pi, ki, d, _ = fe.map_matches(q)
        assert np.array_equal(ki, ms[q][0]) and np.array_equal(pi, ms[q][1]) and np.array_equal(d, ms[q][2])
    err = max(np.abs(out["poses"][q][:, :3] - frames[q][2]).max() for q in range(Q))
    print(f"map {npt}: status ok {int((out['status'] == 0).sum())}/{Q}, matches {int(out['n_match'].mean())} per frame, inliers {int(out['n_inl'].mean())}, "
          f"max |dR| against the generating poses {err:.1e}; stage_map {1e3 * t_stage:.2f} ms (first call: with its allocation)")
    ta, tb = [], []
    for _ in range(args.reps):                                                # the two versions alternate
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fe.relocalize(slots, R.K)
        ta.append((time.perf_counter() - t0) / args.inner)
        t0 = time.perf_counter(); host_path(rows_f32, X); tb.append(time.perf_counter() - t0)
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    print(f"  resident  {spread(ta)}: {Q / ma:.0f} frames/s")
    print(f"  host path {spread(tb)}: {Q / mb:.0f} frames/s   ({mb / ma:.1f}x the resident call's time)")
    fe.profile(True)
    for _ in range(args.reps):
        fe.relocalize(slots, R.K)
    prof = fe.profile_read()
    fe.profile(False)
    print("  split per call (stage brackets, a run of its own): " +
          ", ".join(f"{k} {prof[k][0] / args.reps:.3f} ms" for k in ("match_nn", "match_select", "misc") if k in prof))
    ops = 2.0 * 2 * Q * N * npt * 128                                        # int8 multiply-adds of both directions, as operations
    if "match_nn" in prof:
        print(f"  k_nn_map: {ops / 1e12:.2f} T int8 operations per call -> {ops / (prof['match_nn'][0] / args.reps * 1e-3) / 1e12:.0f} TOP/s achieved")
