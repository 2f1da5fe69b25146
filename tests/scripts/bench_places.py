#!/usr/bin/env python3
"""Place recognition against the only way to ask "which frames see the same ground" without it (docs/kernels/k_places.md, Measured):
    python tests/scripts/bench_places.py [--detector orb|sift] [--reps 5] [--sizes 1024,4541]
64 slots of 2000 chosen rows (kp_cap 2048).  Frames q and q + 32 see the same 2000 landmarks — their rows with a few bits flipped (ORB)
or a few elements nudged (SIFT) — and no other two frames share a landmark.
  places       train_vocabulary on the 64 slots at K = 1024, places_add of the 64 slots, places_query all against all: wall time around
               each synchronous call, and the split match_nn (the assignment) / misc (everything else) of a training run from the
               stage brackets, in a run of its own;
  brute force  what a caller could do before: one run_pairs over all 2016 pairs (i, j) of the 64 resident frames, reading n_match
               (cross-check matches; its E-RANSAC cut to one iteration, which this question does not need), the partner of a frame
               being the frame it has the most matches with.
Both paths run once on the shape before they are timed and must agree — every frame's best candidate is its partner in both — before
a time is printed.  The all-against-all query is then timed on indexes of --sizes entries (the 64 histograms repeated, ids 0 .. n - 1;
a sample of queries is held to numpy first); the brute-force time for those sizes is the 64-frame time SCALED by the number of pairs
and labelled so: nobody can keep 4541 frames' rows resident.  Times are the median and the range over --reps repetitions."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from visual_odometry_amd.frontend import FrontEnd, MATCH_CROSSCHECK  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--detector", default="orb", choices=("orb", "sift"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="1024,4541")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--words", type=int, default=1024)
args = ap.parse_args()
F, N, K, det = args.frames, args.rows, args.words, args.detector
pairs = np.array([[i, j] for i in range(F) for j in range(i + 1, F)], np.int32)
if det == "sift":
    fe = FrontEnd(32, 32, max_frames=F, max_pairs=len(pairs), detector="sift", kp_cap=N)
else:
    fe = FrontEnd(64, 64, max_frames=F, max_pairs=len(pairs), nfeatures=N, nlevels=1)
assert fe.kp_cap >= N
print(f"{F} {det.upper()} slots x {N} rows (kp_cap {fe.kp_cap}), K = {K}, {len(pairs)} pairs")

rng = np.random.default_rng(7)
half = F // 2
for q in range(half):
    if det == "sift":
        base = rng.integers(0, 91, (N, 128), dtype=np.uint8)
        seen = [base.copy(), base.copy()]
        seen[1][:, :4] += rng.integers(0, 2, (N, 4), dtype=np.uint8)
    else:
        base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        seen = [base ^ np.packbits(rng.random((N, 256)) < 0.02, axis=1) for _ in range(2)]
    xy = rng.uniform(0, 60, (N, 2)).astype(np.float32)
    for k in range(2):
        (fe.set_sift_rows if det == "sift" else fe.set_orb_rows)(q + k * half, seen[k], xy)
slots = np.arange(F, dtype=np.int32)
partner = (slots + half) % F
Kmat = np.array([[700.0, 0, 32], [0, 700.0, 32], [0, 0, 1]])
opts = fe.make_opts(match_mode=MATCH_CROSSCHECK, max_iters=1)


def spread(ts):
    ts = sorted(ts)
    return f"{1e3 * ts[len(ts) // 2]:.2f} ms (range {1e3 * ts[0]:.2f} .. {1e3 * ts[-1]:.2f}, {len(ts)} reps)"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def brute_force():
    res, _ = fe.run_pairs(pairs, Kmat, opts)
    m = np.zeros((F, F), np.int64)
    m[pairs[:, 0], pairs[:, 1]] = res["n_match"]
    m = m + m.T
    return m.argmax(axis=1)


def places():
    run = fe.train_vocabulary(slots, K=K)
    fe.places_open(F)
    fe.places_add(slots, slots)
    return run, fe.places_query(top_k=1)


# once on the shape, and the agreement
run, out = places()
best = brute_force()
assert np.array_equal(best, partner), "brute force does not find the partners"
assert np.array_equal(out["entry"][:, 0], partner), "places_query does not find the partners"
e = fe.places_entries()
print(f"vocabulary after {run} updates; both paths name every frame's partner; sum of a histogram {int(e['sum'].min())} .. {int(e['sum'].max())}, "
      f"shared with the partner {int(out['shared'].min())} .. {int(out['shared'].max())}")

t_train, t_add, t_query, t_brute = [], [], [], []
for _ in range(args.reps):                                                     # the two versions alternate
    t0 = time.perf_counter(); fe.train_vocabulary(slots, K=K); t_train.append(time.perf_counter() - t0)
    fe.places_open(F)
    t0 = time.perf_counter(); fe.places_add(slots, slots); t_add.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); fe.places_query(top_k=1); t_query.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); brute_force(); t_brute.append(time.perf_counter() - t0)
print(f"  train_vocabulary ({F * N} rows, {run} updates)  {spread(t_train)}")
print(f"  places_add ({F} slots)                       {spread(t_add)}")
print(f"  places_query ({F} x {F})                       {spread(t_query)}")
print(f"  brute force: run_pairs over {len(pairs)} pairs        {spread(t_brute)}   "
      f"({median(t_brute) / (median(t_add) + median(t_query)):.0f}x add + query; {median(t_brute) / (median(t_train) + median(t_add) + median(t_query)):.1f}x with the training)")
fe.profile(True)
fe.train_vocabulary(slots, K=K)
prof = fe.profile_read()
fe.profile(False)
print("  training split (stage brackets, a run of its own): " + ", ".join(f"{k} {prof[k][0]:.3f} ms in {prof[k][1]} brackets" for k in ("match_nn", "misc") if k in prof))

# the all-against-all query on larger indexes
hist = e["hist"]
for n in [int(v) for v in args.sizes.split(",")]:
    big = hist[np.arange(n) % F]
    ids = np.arange(n, dtype=np.int32)
    fe.places_open(n)
    fe.places_add_histograms(big, ids)
    got = fe.places_query(top_k=3, min_gap=1)                                  # once on the shape
    wide = big.astype(np.int64)
    for q in rng.choice(n, 8, replace=False):
        s = np.minimum(wide, wide[q]).sum(axis=1)
        s[q] = -1
        order = np.lexsort((np.arange(n), -s))[:3]
        assert np.array_equal(got["entry"][q], order) and np.array_equal(got["shared"][q], s[order]), "the query disagrees with numpy"
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); fe.places_query(top_k=3, min_gap=1); ts.append(time.perf_counter() - t0)
    npairs = n * (n - 1) // 2
    scaled = median(t_brute) * npairs / len(pairs)
    print(f"  places_query ({n} x {n}, top_k 3)  {spread(ts)}: {n * n / median(ts) / 1e6:.1f} M scores/s, {n * n * K / median(ts) / 1e9:.0f} G byte differences/s;  "
          f"brute force SCALED from {len(pairs)} to {npairs} pairs: {scaled:.1f} s ({scaled / median(ts):.0f}x)")
