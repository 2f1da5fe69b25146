"""Chosen correspondences for the batched geometry tail (k_match_select's gather -> k_ransac -> k_pose_prepare / k_pose /
k_pose_finish -> k_triangulate_pairs), built with numpy and the CPU oracle alone (not a test module).

A case is a list of correspondences p1[i] <-> p2[i] (float32 pixels, because kp_xy is float32) under one camera matrix.
`slots` turns it into what the parity seams take (FrontEnd.set_orb_rows / set_sift_rows): slot A holds M pairwise distinct
random descriptor rows with xy = p1, slot B the same rows in a seeded non-identity permutation with xy = p2 permuted
alike, so that the strict cross-check gives qi = 0..M-1, ti = the inverse permutation, every distance 0 — asserted here
with the oracle's matcher — and a gather by anything but the train index pairs the wrong points.  `expected` composes the
oracle's stages as twoview.oracle_pair_stages does and adds what decides recoverPose (the four candidates' counts).

What each case is FOR is in `want`; tests/test_two_view_cases_reference.py asserts it on the CPU for every case, so a case
that drifts off its path fails there instead of passing for nothing on the device.

Structured five-point samples (small integers and binary fractions in normalised coordinates, SPECIAL_SAMPLES of
tests/test_gpu_ransac_quad.py) are mapped to pixels with a power-of-two focal length: u = f x + 32 is exact in float32
and u * (1 / f) - 32 / f gives x back exactly."""
import numpy as np

import hamming_reference as HR
import l2i8_reference as LR
from test_gpu_chain import _KP, _inv_pose
from test_gpu_ransac_quad import SPECIAL_SAMPLES, oracle_iterations
from twoview import rot, scene

VO_OK, VO_ERR_TOO_FEW, VO_ERR_NO_MODEL, VO_ERR_AMBIGUOUS = 0, -3, -4, -6      # include/vo_hip.h

K8 = np.array([[8.0, 0, 32], [0, 8.0, 32], [0, 0, 1]])
K64 = np.array([[64.0, 0, 32], [0, 64.0, 32], [0, 0, 1]])
K60 = np.array([[60.0, 0, 32], [0, 60.0, 32], [0, 0, 1]])
K_NONSQUARE = np.array([[60.0, 0, 32], [0, 60.0 * 1.07, 32], [0, 0, 1]])
K_SCENE = scene(0, 1)[0]                                                      # twoview.scene's: 800 / 320 / 240
DIST_THRESHOLDS = (50.0, 9.0, 8.0, 7.0, 1.0)


class Case:
    def __init__(self, name, group, K, p1, p2, want, max_iters=1000):
        self.name, self.group, self.K, self.want, self.max_iters = name, group, K, want, max_iters
        self.p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        self.p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(self.p1) == len(self.p2)
        self.M = len(self.p1)
        self._slots, self._expected = {}, {}

    def __repr__(self):
        return f"Case({self.name})"

    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) % 100003


# ------------------------------------------------------------------ descriptors and the intended match list
def slots(O, case, detector="orb"):
    """(rows1, xy1, rows2, xy2, qi, ti): what the two slots of the case hold and the match list that must come out."""
    if detector in case._slots:
        return case._slots[detector]
    rng = np.random.default_rng(7000 + case.seed())
    M = case.M
    rows1 = HR.rand_rows(rng, M) if detector == "orb" else LR.sift_like(rng, M)
    perm = rng.permutation(M)
    while M >= 2 and np.array_equal(perm, np.arange(M)):
        perm = rng.permutation(M)
    rows2, xy2 = rows1[perm], case.p2[perm]                                   # slot B row j is slot A row perm[j]
    ti = np.empty(M, np.int32); ti[perm] = np.arange(M, dtype=np.int32)       # the inverse permutation
    qi = np.arange(M, dtype=np.int32)
    assert M < 2 or not np.array_equal(ti, qi)
    if detector == "orb":
        q, t, d = O.match_hamming(rows1, rows2, 2)
    else:
        assert (rows1.astype(np.int64) ** 2).sum(1).max(initial=0) <= LR.NORM_BOUND
        q, t, d = O.match_l2(rows1.astype(np.float32), rows2.astype(np.float32), 2)
    assert np.array_equal(q, qi) and np.array_equal(t, ti) and not d.any(), case.name     # distinct rows: one mutual match each
    assert np.array_equal(xy2[ti], case.p2)
    case._slots[detector] = (rows1, case.p1, rows2, xy2, qi, ti)
    return case._slots[detector]


# ------------------------------------------------------------------ the oracle's answer
def expected(O, case, dist_thresh=50.0, max_iters=None):
    """The pair's record as the oracle's stages give it, in whichever root-finder mode the oracle is in now:
    status (the device's code), n_match, n_inl, n_good, ransac_iters, mask, models (all stacked ones of M == 5), and for a
    VO_OK pair E, R, t, counts[4], best, pose_mask, X (4 x n_inl, w = 1), q1 / q2 (the inliers, in order).  max_iters: the
    launch's RANSAC budget where it is not the case's own."""
    max_iters = case.max_iters if max_iters is None else max_iters
    key = (float(dist_thresh), O.get_dk_early_exit(), max_iters)
    if key in case._expected:
        return case._expected[key]
    p1, p2, K, M = case.p1.astype(np.float64), case.p2.astype(np.float64), case.K, case.M
    rc, E, mask, ninl = O.find_essential_ransac(p1, p2, K, prob=0.99, thresh=1.0, max_iters=max_iters)
    assert rc in (0, VO_ERR_TOO_FEW, VO_ERR_NO_MODEL)
    e = dict(n_match=M, n_inl=ninl, n_good=0, mask=mask, models=E, ransac_iters=0)
    if M > 5:
        e["ransac_iters"] = oracle_iterations(O, p1, p2, K, 0.99, 1.0, max_iters)
    if rc != 0:
        e["status"] = rc
    elif len(E) != 1:
        e["status"] = VO_ERR_AMBIGUOUS                                        # decomposeEssentialMat needs one 3 x 3 matrix
    else:
        inl = mask > 0
        good, best, R, t, pm = O.recover_pose_counts(E[0], p1[inl], p2[inl], K, dist_thresh)
        X = O.triangulate(_KP(K, _inv_pose(R, t)), _KP(K, np.eye(3, 4)), p1[inl].T, p2[inl].T)
        with np.errstate(all="ignore"):
            X = X / X[3]
        e.update(status=VO_OK, E=E[0], R=R, t=t, counts=good, best=best, n_good=int(good[best]), pose_mask=pm, X=X,
                 q1=p1[inl], q2=p2[inl])
    case._expected[key] = e
    return e


# ------------------------------------------------------------------ builders
def _project(K, X):
    x = X / X[:, 2:]
    return np.stack([K[0, 0] * x[:, 0] + K[0, 2], K[1, 1] * x[:, 1] + K[1, 2]], axis=1).astype(np.float32)


def posed(seed, n_front, n_behind, K, spread=2.0, shuffle=True):
    """A noise-free two-view scene without outliers: R = rot(., 0.02 .. 0.15), unit t, points uniform(-spread, spread)^3 +
    (0, 0, 8); the last n_behind of them mirrored through the origin, which puts them behind both cameras and leaves them on
    the same epipolar geometry (they are the points of the motion (R, -t)).  Rounded to float32 pixels."""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(0.02, 0.15))
    t = rng.normal(size=3); t /= np.linalg.norm(t)
    n = n_front + n_behind
    X = rng.uniform(-spread, spread, (n, 3)) + np.array([0, 0, 8.0])
    X[n_front:] *= -1.0
    if shuffle:
        X = X[rng.permutation(n)]
    return _project(K, X), _project(K, X @ R.T + t)


def _structured(name, K, twice=False):
    a, b = SPECIAL_SAMPLES[name][:2]
    a, b = np.array(a, np.float64), np.array(b, np.float64)
    if twice:
        a, b = np.vstack([a, a]), np.vstack([b, b])
    f, c = K[0, 0], K[0, 2]
    p1, p2 = (f * a + c).astype(np.float32), (f * b + c).astype(np.float32)
    assert np.array_equal(p1.astype(np.float64) * (1 / f) - c * (1 / f), a)   # the device's normalisation gives the sample back
    assert np.array_equal(p2.astype(np.float64) * (1 / f) - c * (1 / f), b)
    return p1, p2


# ------------------------------------------------------------------ the cases
# Every seed below was picked on the CPU with the oracle (scanned below 40); what a case reaches is its `want`: status;
# models (stacked solutions of M == 5); counts / best (the four candidates of recoverPose at dist_thresh 50); n_inl; n_good
# (per dist_thresh where it is a dict); iters (RANSAC iterations).  tests/test_two_view_cases_reference.py asserts all of it.
N_WIN = 40
WINNERS = {      # name: (seed, in front, behind) -> the candidate that takes all 40 points
    "winner0_front": (5, N_WIN, 0, 0), "winner1_front": (0, N_WIN, 0, 1), "winner2_front": (2, N_WIN, 0, 2), "winner3_front": (3, N_WIN, 0, 3),
    "winner0_behind": (1, 0, N_WIN, 0), "winner1_behind": (3, 0, N_WIN, 1), "winner2_behind": (7, 0, N_WIN, 2), "winner3_behind": (5, 0, N_WIN, 3),
}
TIES = {         # name: (seed, in front, behind, counts, best)
    "tie_20_20_first_pair": (2, 20, 20, [20, 0, 20, 0], 0), "tie_20_20_second_pair": (0, 20, 20, [0, 20, 0, 20], 1),
    "split_21_19_first_pair": (2, 21, 19, [19, 0, 21, 0], 2), "split_19_21_first_pair": (2, 19, 21, [21, 0, 19, 0], 0),
    "split_21_19_second_pair": (0, 21, 19, [0, 19, 0, 21], 3), "split_19_21_second_pair": (0, 19, 21, [0, 21, 0, 19], 1),
}
THRESHOLD_N_GOOD = {50.0: 60, 9.0: 34, 8.0: 23, 7.0: 12, 1.0: 0}              # one scene of 60 points in front, spread 3
BLOCK_EDGES = {  # M: (seed, best); kp_cap 768
    255: (1, 2), 256: (1, 0), 257: (1, 1), 511: (0, 0), 512: (0, 1), 513: (1, 0), 768: (1, 0),
}
BLOCK_KP_CAP = 768
WAVE_EDGES = {   # M: (n_inl, counts, best, iterations) of twoview.scene(101, M, outliers=0.3) rounded to float32
    63: (43, [0, 42, 0, 1], 1, 29), 64: (43, [42, 0, 1, 0], 0, 32), 65: (42, [41, 0, 1, 0], 0, 56),
}


def _cases():
    out = []

    def add(name, group, K, pts, want, **k):
        out.append(Case(name, group, K, pts[0], pts[1], want, **k))

    some = posed(11, 4, 0, K60)
    for m in range(5):
        add(f"few_{m}", "few", K60, (some[0][:m], some[1][:m]), dict(status=VO_ERR_TOO_FEW, n_inl=0))
    for K, tag in ((K8, ""), (K64, "_k64")):
        for name in ("rank_deficient_null_space", "zero_pivot", "zero_pivot_all_zero"):
            add(f"five_{name}{tag}", "five_no_model", K, _structured(name, K), dict(status=VO_ERR_NO_MODEL, models=0, n_inl=0))
        for name in ("degree_9_and_skipped_root", "degree_8", "ten_nan_models"):
            add(f"five_{name}{tag}", "five_stacked", K, _structured(name, K),
                dict(status=VO_ERR_AMBIGUOUS, models=SPECIAL_SAMPLES[name][2], n_inl=5))
        add(f"five_degree_9_one_real_root{tag}", "five_one_model", K, _structured("degree_9_one_real_root", K),
            dict(status=VO_OK, models=1, n_inl=5, counts=[3, 2, 0, 0], best=0, n_good=3))
        add(f"ten_equal_points{tag}", "many_no_model", K, _structured("zero_pivot_all_zero", K, twice=True),
            dict(status=VO_ERR_NO_MODEL, n_inl=0, iters=100), max_iters=100)
    for name, (seed, nf, nb, best) in WINNERS.items():
        counts = [0, 0, 0, 0]; counts[best] = N_WIN
        add(name, "winner", K60, posed(seed, nf, nb, K60), dict(status=VO_OK, n_inl=N_WIN, counts=counts, best=best, n_good=N_WIN, iters=1))
    for name, (seed, nf, nb, counts, best) in TIES.items():
        add(name, "tie", K60, posed(seed, nf, nb, K60), dict(status=VO_OK, n_inl=nf + nb, counts=counts, best=best, n_good=counts[best], iters=1))
    add("threshold", "threshold", K60, posed(3, 60, 0, K60, spread=3.0),
        dict(status=VO_OK, n_inl=60, counts=[0, 0, 60, 0], best=2, n_good=dict(THRESHOLD_N_GOOD), iters=1))
    for M, (seed, best) in BLOCK_EDGES.items():
        counts = [0, 0, 0, 0]; counts[best] = M
        add(f"block_{M}", "block", K60, posed(seed, M, 0, K60), dict(status=VO_OK, n_inl=M, counts=counts, best=best, n_good=M, iters=1))
    # in front first, behind after: the candidates' counts come from different blocks of k_pose
    add("block_256_256", "block", K60, posed(0, 256, 256, K60, shuffle=False), dict(status=VO_OK, n_inl=512, counts=[256, 0, 256, 0], best=0, n_good=256, iters=1))
    add("block_257_256", "block", K60, posed(0, 257, 256, K60, shuffle=False), dict(status=VO_OK, n_inl=513, counts=[256, 0, 257, 0], best=2, n_good=257, iters=1))
    for M, (n_inl, counts, best, iters) in WAVE_EDGES.items():
        _, _, _, p1, p2 = scene(101, M, outliers=0.3)
        add(f"wave_{M}", "wave", K_SCENE, (p1, p2), dict(status=VO_OK, n_inl=n_inl, counts=counts, best=best, n_good=counts[best], iters=iters))
    add("non_square", "non_square", K_NONSQUARE, posed(0, 50, 0, K_NONSQUARE), dict(status=VO_OK, n_inl=50, counts=[49, 0, 1, 0], best=0, n_good=49, iters=1))
    # the same constructions under the power-of-two camera of the mixed and the SIFT launch
    add("k8_winner2", "winner", K8, posed(0, N_WIN, 0, K8), dict(status=VO_OK, n_inl=N_WIN, counts=[0, 0, N_WIN, 0], best=2, n_good=N_WIN, iters=1))
    add("k8_winner3", "winner", K8, posed(1, N_WIN, 0, K8), dict(status=VO_OK, n_inl=N_WIN, counts=[0, 0, 0, N_WIN], best=3, n_good=N_WIN, iters=1))
    add("k64_winner3", "winner", K64, posed(1, N_WIN, 0, K64), dict(status=VO_OK, n_inl=N_WIN, counts=[0, 0, 0, N_WIN], best=3, n_good=N_WIN, iters=1))
    add("k64_tie_second_pair", "tie", K64, posed(0, 20, 20, K64), dict(status=VO_OK, n_inl=40, counts=[0, 20, 0, 20], best=1, n_good=20, iters=1))
    assert len({c.name for c in out}) == len(out)
    return out


_ALL = None


def cases():
    """name -> Case, built once."""
    global _ALL
    if _ALL is None:
        _ALL = {c.name: c for c in _cases()}
    return _ALL


def group(*names):
    return [c for c in cases().values() if c.group in names]
