#!/usr/bin/env python3
"""vo_map_align against the only way to do the same work without it (docs/kernels/k_sim3_ransac.md, Measured):
    python tests/scripts/bench_map_align.py [--reps 7] [--inner 10] [--maps 4096,32768]
Q = 8 SIFT query maps of 4096 rows against staged maps of 4096 and 32768 points.  Every query map holds 4096 of the staged map's
points in a gauge of its own (a similarity of its own, inverted exactly): their rows with a few elements nudged, 10 % of the points
somewhere else.
  resident   one FrontEnd.align_maps call for the 8 maps: wall time around the synchronous call (upload of the query maps included),
             and the split match_nn (k_align_gather + k_nn_align) / match_select (k_align_select) / misc (k_sim3_ransac) from the
             stage brackets, in a run of its own;
  host path  what a caller could do before: vo_match_l2(crossCheck) per query map against the staged rows, gather the
             correspondences with numpy, one vo_sim3_ransac_batch for the 8 maps.
Both paths are warmed up on the shape they are timed on and must agree (matches equal, similarities byte for byte) before a time is
printed.  Times are the median and the range over --reps repetitions — of the mean of --inner back-to-back calls for the resident
path — and no threshold is set on them."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import map_align_reference as A  # noqa: E402
import relocalize_reference as R  # noqa: E402
from visual_odometry_amd import geometry  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402
from visual_odometry_amd.matcher import L2Matcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=10, help="resident calls per timed window")
ap.add_argument("--maps", default="4096,32768")
ap.add_argument("--queries", type=int, default=8)
ap.add_argument("--rows", type=int, default=4096)
args = ap.parse_args()
Q, N, MAX_ERROR = args.queries, args.rows, 0.05
fe = FrontEnd(32, 32, max_frames=1, max_pairs=1, detector="sift", kp_cap=64)
print(f"{Q} SIFT query maps x {N} rows")


def scene(npt, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (npt, 3)) + [0, 0, 6]
    rows = R.rand_rows(rng, npt, "sift")
    maps = []
    for q in range(Q):
        s = float(rng.uniform(0.3, 3)); Rm = R.rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)); t = rng.uniform(-4, 4, 3)
        ids = rng.choice(npt, min(N, npt), replace=False)
        pts = (X[ids] - t) @ Rm / s
        wrong = rng.random(len(ids)) < 0.1
        pts[wrong] += rng.uniform(1, 3, (int(wrong.sum()), 3))
        f = rows[ids].copy()
        f[:, :4] += rng.integers(0, 2, (len(ids), 4), dtype=np.uint8)        # a few elements off by one: near, not equal
        maps.append((f, pts, (s, Rm, t)))
    return X, rows, maps


def spread(ts):
    ts = sorted(ts)
    return f"{1e3 * ts[len(ts) // 2]:.2f} ms (range {1e3 * ts[0]:.2f} .. {1e3 * ts[-1]:.2f}, {len(ts)} reps)"


def host_path(maps, map_rows_f32, X):
    """vo_match_l2 per query map -> numpy gather -> one vo_sim3_ransac_batch"""
    matcher = L2Matcher(crossCheck=True, ctx=fe.ctx)
    src, dst, off, ms = [], [], [0], []
    for f32, pts in maps:
        bi, ai, d = matcher.match_arrays(f32, map_rows_f32)
        src.append(pts[bi]); dst.append(X[ai]); off.append(off[-1] + len(bi)); ms.append((bi, ai, d))
    out = geometry.estimate_similarity_batch(np.concatenate(src), np.concatenate(dst), np.array(off, np.int32), MAX_ERROR, ctx=fe.ctx)
    return out, ms


for npt in [int(v) for v in args.maps.split(",")]:
    X, rows, maps = scene(npt, 2000 + npt)
    q_rows = np.concatenate([m[0] for m in maps]); q_pts = np.concatenate([m[1] for m in maps])
    off = np.arange(Q + 1, dtype=np.int32) * len(maps[0][0])
    t0 = time.perf_counter(); fe.stage_map(rows, X); t_stage = time.perf_counter() - t0
    out = fe.align_maps(q_rows, q_pts, MAX_ERROR, offsets=off)                # warm-up, and the result both paths must give
    rows_f32 = rows.astype(np.float32)
    host_maps = [(m[0].astype(np.float32), m[1]) for m in maps]
    ref, ms = host_path(host_maps, rows_f32, X)                               # warm-up of the host path
    assert all(out[k].tobytes() == ref[k].tobytes() for k in ("status", "scale", "R", "t", "n_inl")), "the two paths disagree"
    for q in (0, Q - 1):
        ai, bi, d, _ = fe.map_align_matches(q)
        assert np.array_equal(bi, ms[q][0]) and np.array_equal(ai, ms[q][1]) and np.array_equal(d, ms[q][2])
    err = np.max([A.model_error((out["scale"][q], out["R"][q], out["t"][q]), maps[q][2]) for q in range(Q)], axis=0)
    print(f"map {npt}: status ok {int((out['status'] == 0).sum())}/{Q}, matches {int(out['n_match'].mean())} per map, inliers {int(out['n_inl'].mean())}, "
          f"error against the generating similarities s {err[0]:.1e} R {err[1]:.1e} t {err[2]:.1e}; stage_map {1e3 * t_stage:.2f} ms (first call: with its allocation)")
    ta, tb = [], []
    for _ in range(args.reps):                                                # the two versions alternate
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fe.align_maps(q_rows, q_pts, MAX_ERROR, offsets=off)
        ta.append((time.perf_counter() - t0) / args.inner)
        t0 = time.perf_counter(); host_path(host_maps, rows_f32, X); tb.append(time.perf_counter() - t0)
    ma, mb = sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]
    print(f"  resident  {spread(ta)}: {Q / ma:.0f} maps/s")
    print(f"  host path {spread(tb)}: {Q / mb:.0f} maps/s   ({mb / ma:.1f}x the resident call's time)")
    fe.profile(True)
    for _ in range(args.reps):
        fe.align_maps(q_rows, q_pts, MAX_ERROR, offsets=off)
    prof = fe.profile_read()
    fe.profile(False)
    print("  split per call (stage brackets, a run of its own): " +
          ", ".join(f"{k} {prof[k][0] / args.reps:.3f} ms" for k in ("match_nn", "match_select", "misc") if k in prof))
