"""Two maps of one ground patch, aligned by descriptors, refined by matching their points in space, and merged into one.

No images: two synthetic maps, half overlapping, in different gauges.  Map A holds n points of a thin slab; map B sees half of them
again — with noise, from a gauge of its own — and as many new ones beside them.  A share of B's rows have a look-alike in A: a point
somewhere else that carries exactly their row, which the descriptor-only match prefers.

    python examples/fuse_maps.py [--n 2000] [--alike 0.25] [--noise 0.004] [--radius 0.15] [--detector orb|sift]

Prints matches and inliers for the descriptor-only alignment (FrontEnd.align_maps) and for the guided refinement on top of it
(align_maps(refine_radius=)), the error of each similarity against the generating one, the merged size and n_fused
(FrontEnd.fuse_map), and how many true duplicates were fused and how many false ones."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def rand_rows(rng, n, sift):
    return rng.integers(0, 91, (n, 128), dtype=np.uint8) if sift else rng.integers(0, 256, (n, 32), dtype=np.uint8)


def nudged(rng, rows, sift):
    """copies a few steps away in descriptor space: 1 .. 6 elements moved by one (SIFT) / bits flipped (ORB)"""
    out = rows.copy()
    for r in out:
        for e in rng.choice(len(r) * (1 if sift else 8), int(rng.integers(1, 7)), replace=False):
            if sift:
                r[e] += 1
            else:
                r[e // 8] ^= np.uint8(1 << (e % 8))
    return out


def two_maps(n, alike, noise, sift, seed=0):
    rng = np.random.default_rng(seed)
    side = np.sqrt(n / 8.0)                                                # about 8 points per unit of ground
    a = np.column_stack([rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(-0.25, 0.25, n)])
    rows_a = rand_rows(rng, n, sift)
    half = n // 2
    seen_again = np.argsort(a[:, 0])[half:]                                # the half of A with the larger x
    y = np.column_stack([rng.uniform(side, 1.5 * side, n), rng.uniform(0, side, n), rng.uniform(-0.25, 0.25, n)])
    rows_b = rand_rows(rng, n, sift)
    y[:half] = a[seen_again] + rng.normal(0, noise, (half, 3))
    rows_b[:half] = nudged(rng, rows_a[seen_again], sift)
    n_alike = int(alike * half)
    others = np.argsort(a[:, 0])[:half]
    rows_a[others[:n_alike]] = rows_b[:n_alike]                            # look-alikes in the part of A that B does not see
    s, R, t = 2.5, rotation([0.2, -0.4, 0.9], 0.8), np.array([3.0, -1.0, 0.5])
    b = (y - t) @ R / s                                                    # X_b = R^T (X_a - t) / s
    order = rng.permutation(n)                                             # B's own row order
    truth_a = np.full(n, -1); truth_a[:half] = seen_again
    return dict(rows_a=rows_a, pts_a=a, rows_b=rows_b[order], pts_b=b[order], truth_a=truth_a[order], model=(s, R, t))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--alike", type=float, default=0.25)
    ap.add_argument("--noise", type=float, default=0.004)
    ap.add_argument("--radius", type=float, default=0.15)
    ap.add_argument("--max-error", type=float, default=0.05)
    ap.add_argument("--detector", choices=("orb", "sift"), default="orb")
    args = ap.parse_args()
    from visual_odometry_amd.frontend import FrontEnd
    sift = args.detector == "sift"
    m = two_maps(args.n, args.alike, args.noise, sift)
    fe = FrontEnd(32, 32, max_frames=1, max_pairs=1, detector="sift", kp_cap=64) if sift else FrontEnd(64, 64, max_frames=1, max_pairs=1, nfeatures=64, nlevels=1)
    s, R, t = m["model"]

    def err(o):
        return abs(o["scale"][0] - s), float(np.abs(o["R"][0] - R).max()), float(np.abs(o["t"][0] - t).max())

    fe.stage_map(m["rows_a"], m["pts_a"])
    first = fe.align_maps(m["rows_b"], m["pts_b"], args.max_error)
    print("descriptor-only: status %d  matches %d  inliers %d   error  s %.2e  R %.2e  t %.2e" % ((first["status"][0], first["n_match"][0], first["n_inl"][0]) + err(first)))
    both = fe.align_maps(m["rows_b"], m["pts_b"], args.max_error, refine_radius=args.radius)
    print("guided on top:   status %d  matches %d  inliers %d   error  s %.2e  R %.2e  t %.2e   (points with a neighbour: %d)"
          % ((both["status"][0], both["n_match"][0], both["n_inl"][0]) + err(both) + (both["n_seen"][0],)))
    fused = fe.fuse_map(m["rows_b"], m["pts_b"], args.max_error, args.radius)
    if fused["rows"] is None:
        print("the alignment failed: nothing merged")
        return 1
    ib, na = fused["index_b"], fused["n_a"]
    into_a = ib < na
    true_dup = m["truth_a"] >= 0
    right = int((into_a & true_dup & (ib == m["truth_a"])).sum())
    print("merged: %d + %d points -> %d, n_fused %d   true duplicates fused %d of %d, false fusions %d"
          % (na, len(ib), len(fused["rows"]), fused["n_fused"], right, int(true_dup.sum()), int(into_a.sum()) - right))
    rows_now, _ = fe.map_rows()
    print("staged now: %d points" % len(rows_now))
    fe.ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
