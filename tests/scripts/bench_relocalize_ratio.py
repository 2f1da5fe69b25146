#!/usr/bin/env python3
"""vo_map_localize by the ratio rule (vo_set_map_match mode 1) against the cross-check (mode 0) (docs/kernels/k_nn_map.md, Measured):
    python tests/scripts/bench_relocalize_ratio.py [--reps 7] [--inner 25] [--maps 4096,32768]
bench_relocalize.py's shapes and method: Q = 64 SIFT slots of 3500 staged rows (kp_cap 3584) against staged maps of 4096 and 32768
points, every frame seeing 3500 of the map's points from a pose of its own (rows with a few elements nudged, 10 % wrong pixels).
Modes 0 and 1 alternate in one process; a time is the mean of --inner back-to-back FrontEnd.relocalize calls, reported as the median
and the range over --reps repetitions; the match_nn stage bracket (k_nn_map) is read in a run of its own per mode.  The two modes'
list sizes are printed first.

Mode 1 skips the reverse direction, so the expectation to confirm or refute is "about half of match_nn, plus the med3".

No time is printed unless mode 0 returns what the library returned before it had a mode: tests/golden/relocalize_ratio_parent.json
holds, per map size, the SHA-256 of that library's relocalize outputs and match lists on this script's input.  It was written by
    python tests/scripts/bench_relocalize_ratio.py --dump tests/golden/relocalize_ratio_parent.json --package-root <checkout of the parent commit, built>
which calls nothing the parent does not have."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "relocalize_ratio_parent.json")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=25, help="calls per timed window (a single call is a few ms: too short a window)")
ap.add_argument("--maps", default="4096,32768")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--rows", type=int, default=3500)
ap.add_argument("--ratio", type=float, default=0.75)
ap.add_argument("--dump", default=None, help="write mode 0's digests to this file and stop (run against the parent commit's build)")
ap.add_argument("--package-root", default=ROOT, help="the tree whose visual_odometry_amd is loaded")
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.package_root), os.path.join(ROOT, "tests"), ROOT]
import relocalize_reference as R  # noqa: E402
from visual_odometry_amd.frontend import FrontEnd  # noqa: E402

Q, N = args.frames, args.rows
fe = FrontEnd(32, 32, max_frames=Q, max_pairs=Q, detector="sift", kp_cap=N)
print(f"{Q} SIFT slots x {N} rows (kp_cap {fe.kp_cap}); library version {fe.ctx.lib.vo_version()}")


def scene(npt, seed):
    """bench_relocalize.py's scene, draw for draw."""
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
        f[:, :4] += rng.integers(0, 2, (len(ids), 4), dtype=np.uint8)
        frames.append((f, uv.astype(np.float32), Rm, t))
    return X, rows, frames


def digest(out):
    """SHA-256 over relocalize's four arrays and every query's match list (map point, keypoint, distance, inlier mask)."""
    h = hashlib.sha256()
    for k in ("poses", "n_match", "n_inl", "status"):
        h.update(np.ascontiguousarray(out[k]).tobytes())
    for q in range(Q):
        for a in fe.map_matches(q):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def spread(ts):
    ts = sorted(ts)
    return f"{1e3 * ts[len(ts) // 2]:.2f} ms (range {1e3 * ts[0]:.2f} .. {1e3 * ts[-1]:.2f}, {len(ts)} reps)"


maps = [int(v) for v in args.maps.split(",")]
slots = np.arange(Q, dtype=np.int32)
if args.dump:
    got = {}
    for npt in maps:
        X, rows, frames = scene(npt, 1000 + npt)
        for q, (f, xy, _, _) in enumerate(frames):
            fe.set_sift_rows(q, f, xy)
        fe.stage_map(rows, X)
        got[str(npt)] = digest(fe.relocalize(slots, R.K))
        print(f"map {npt}: {got[str(npt)]}")
    with open(args.dump, "w") as fh:
        json.dump(dict(what="SHA-256 of FrontEnd.relocalize(range(64), K) and its 64 match lists on bench_relocalize_ratio.py's input, per map size, "
                            "from the library before vo_set_map_match", frames=Q, rows=N, library_version=int(fe.ctx.lib.vo_version()), sha256=got), fh, indent=1)
        fh.write("\n")
    sys.exit(0)

golden = json.load(open(GOLDEN))
assert (golden["frames"], golden["rows"]) == (Q, N), "the golden digests were made for another shape"
call = {0: lambda: fe.relocalize(slots, R.K), 1: lambda: fe.relocalize(slots, R.K, match="ratio", ratio=args.ratio)}
for npt in maps:
    X, rows, frames = scene(npt, 1000 + npt)
    for q, (f, xy, _, _) in enumerate(frames):
        fe.set_sift_rows(q, f, xy)
    fe.stage_map(rows, X)
    out = {m: call[m]() for m in (0, 1)}                                     # warm-up of both modes on the shape
    print(f"map {npt}: list sizes per frame: mode 0 (cross-check) {out[0]['n_match'].mean():.1f}, mode 1 (ratio {args.ratio}) {out[1]['n_match'].mean():.1f}; "
          f"solved {int((out[0]['status'] == 0).sum())}/{Q} and {int((out[1]['status'] == 0).sum())}/{Q}; inliers {out[0]['n_inl'].mean():.0f} and {out[1]['n_inl'].mean():.0f}")
    want = golden["sha256"].get(str(npt))
    got = digest(call[0]())
    if got != want:
        raise SystemExit(f"map {npt}: mode 0 does not return what the parent commit returned on this input ({got} against {want}): no time is printed")
    print("  mode 0 returns the parent commit's bytes")
    t = {0: [], 1: []}
    for _ in range(args.reps):                                                # the two modes alternate
        for m in (0, 1):
            t0 = time.perf_counter()
            for _ in range(args.inner):
                call[m]()
            t[m].append((time.perf_counter() - t0) / args.inner)
    med = {m: sorted(t[m])[len(t[m]) // 2] for m in (0, 1)}
    for m in (0, 1):
        print(f"  mode {m} whole call  {spread(t[m])}: {Q / med[m]:.0f} frames/s")
    print(f"  whole call, mode 1 / mode 0: {med[1] / med[0]:.3f}")
    nn = {}
    for m in (0, 1):
        fe.profile(True)
        for _ in range(args.reps):
            call[m]()
        prof = fe.profile_read()
        fe.profile(False)
        nn[m] = prof["match_nn"][0] / args.reps if "match_nn" in prof else float("nan")
        print(f"  mode {m} split per call (stage brackets, a run of its own): " +
              ", ".join(f"{k} {prof[k][0] / args.reps:.3f} ms" for k in ("match_nn", "match_select", "misc") if k in prof))
    print(f"  match_nn, mode 1 / mode 0: {nn[1] / nn[0]:.3f}")
