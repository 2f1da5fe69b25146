"""The checker of the device bundle adjustment: a numpy restatement of what the reference's Map.optimize_map asks g2o
for (src/map.py:104-186) — VertexSE3Expmap / VertexPointXYZ / EdgeProjectXYZ2UV, Huber kernel, Levenberg over a Schur
complement — from g2o's 2020 sources as recalled (g2o is not installed anywhere this project runs; parity with a g2o
build is unpinned).  Written differently from the kernel on purpose: dense per-observation Jacobians, every sum taken
sequentially in observation order (np.add.at is unbuffered: it adds one item after the other), numpy.linalg for the 3x3
inverses, the Cholesky factor and the triangular solves.  Also the seeded map generator the tests and bench_ba.py share.
A plain helper module (like tests/twoview.py), no test in it."""
import numpy as np

F0, CX, CY = 802.832, 565.427, 240.124            # the reference's camera (test.g2o:1)
DBL_MAX = np.finfo(np.float64).max


# ---------------------------------------------------------------- SE3Quat
def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def quat_from_rot(m):
    """Eigen's Quaternion(Matrix3) + SE3Quat::normalizeRotation; q = (x, y, z, w), w >= 0, unit norm"""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t; t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def rot_from_quat(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def quat_mul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def se3_exp(d):
    """SE3Quat::exp: rotation part first; below 1e-5 rad g2o takes R = I + W + W^2 / 2 and V = R"""
    w, u = np.asarray(d[:3], float), np.asarray(d[3:], float)
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = hat(w); W2 = W @ W
    if th < 1e-5:
        R = np.eye(3) + W + 0.5 * W2
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * W2
        V = np.eye(3) + (1 - np.cos(th)) / (th * th) * W + (th - np.sin(th)) / (th * th * th) * W2
    return R, V @ u


def pose_update(d, q, T):
    """T <- exp(d) T on (unit quaternion, [R | t]); returns the new pair"""
    dR, dt = se3_exp(d)
    qn = quat_mul(quat_from_rot(dR), q)
    if qn[3] < 0:
        qn = -qn
    qn = qn / np.sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3])
    Tn = np.empty((3, 4))
    Tn[:, :3] = rot_from_quat(qn)
    Tn[:, 3] = dR @ T[:, 3] + dt
    return qn, Tn


# ---------------------------------------------------------------- the edge
def project(T, X, f=F0, cx=CX, cy=CY):
    q = T[:, :3] @ X + T[:, 3]
    return np.array([f * q[0] / q[2] + cx, f * q[1] / q[2] + cy])


def residuals(poses, X, oc, op, xy, f, cx, cy):
    q = np.einsum("nij,nj->ni", poses[oc, :, :3], X[op]) + poses[oc, :, 3]
    return xy - np.c_[f * q[:, 0] / q[:, 2] + cx, f * q[:, 1] / q[:, 2] + cy], q


def jacobians(poses, q, oc, f):
    """d e / d pose [n, 2, 6] (columns omega, upsilon) and d e / d X [n, 2, 3] of EdgeProjectXYZ2UV"""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    o = 0 * z
    Jp = np.empty((len(z), 2, 6)); A = np.empty((len(z), 2, 3))
    Jp[:, 0] = np.c_[x * y / z ** 2 * f, -(1 + x * x / z ** 2) * f, y / z * f, -1 / z * f, o, x / z ** 2 * f]
    Jp[:, 1] = np.c_[(1 + y * y / z ** 2) * f, -x * y / z ** 2 * f, -x / z * f, o, -1 / z * f, y / z ** 2 * f]
    A[:, 0] = np.c_[f / z, o, -f * x / z ** 2]
    A[:, 1] = np.c_[o, f / z, -f * y / z ** 2]
    return Jp, -np.einsum("nij,njk->nik", A, poses[oc, :, :3])


def robust(e, delta):
    """RobustKernelHuber on the edge's 2-vector: rho and the weight rho' (g2o uses no second-order term)"""
    e2 = (e * e).sum(1)
    s = np.sqrt(e2)
    if delta <= 0:
        return e2, np.ones(len(e2))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = s > delta
        return np.where(out, 2 * delta * s - delta * delta, e2), np.where(out, delta / s, 1.0)


def seq_sum(v):
    t = 0.0
    for x in v.tolist():
        t += x
    return t


# ---------------------------------------------------------------- Levenberg-Marquardt as g2o runs it
def lm(poses, fixed, points, oc, op, xy, f=F0, cx=CX, cy=CY, iterations=40, delta=1.0, order=None, lam_trace=None):
    """Returns dict(poses, points, chi2_before, chi2_after, iterations, trials, accepts).  order: a permutation of the
    observations (every sum then runs in that order).  lam_trace: a list that receives lambda before every trial."""
    T = np.array(poses, np.float64).reshape(-1, 3, 4).copy()
    X = np.array(points, np.float64).reshape(-1, 3).copy()
    fixed = np.asarray(fixed).astype(bool)
    oc = np.asarray(oc, np.int64); op = np.asarray(op, np.int64); xy = np.asarray(xy, np.float64).reshape(-1, 2)
    if order is not None:
        oc, op, xy = oc[order], op[order], xy[order]
    free = np.flatnonzero(~fixed)
    col = -np.ones(len(T), np.int64); col[free] = np.arange(len(free))
    F, n, npt = len(free), 6 * len(free), len(X)
    quat = {}
    for k in free:                                   # g2o keeps the rotation as a unit quaternion
        quat[k] = quat_from_rot(T[k, :, :3]); T[k, :, :3] = rot_from_quat(quat[k])
    seen = np.bincount(op, minlength=npt) > 0
    oc_col = col[oc]
    fo = np.flatnonzero(oc_col >= 0)                 # observations by free cameras, and the pairs of them that share a point
    j1s, j2s = [], []
    by_pt = {}
    for j in fo.tolist():
        by_pt.setdefault(int(op[j]), []).append(j)
    for lst in by_pt.values():
        for a in lst:
            for b in lst:
                j1s.append(a); j2s.append(b)
    j1s = np.array(j1s, np.int64); j2s = np.array(j2s, np.int64)

    e, q = residuals(T, X, oc, op, xy, f, cx, cy)
    rho_e, w = robust(e, delta)
    cur = seq_sum(rho_e)
    out = dict(chi2_before=cur, accepts=[])
    lam, ni, n_it, trials = None, 2.0, 0, 0
    for _ in range(int(iterations)):
        n_it += 1
        Jp, Jx = jacobians(T, q, oc, f)
        Hpp = np.zeros((npt, 3, 3)); bp = np.zeros((npt, 3)); Hcc = np.zeros((F, 6, 6)); bc = np.zeros((F, 6))
        np.add.at(Hpp, op, w[:, None, None] * np.einsum("nki,nkj->nij", Jx, Jx))
        np.add.at(bp, op, -w[:, None] * np.einsum("nki,nk->ni", Jx, e))
        np.add.at(Hcc, oc_col[fo], w[fo, None, None] * np.einsum("nki,nkj->nij", Jp[fo], Jp[fo]))
        np.add.at(bc, oc_col[fo], -w[fo, None] * np.einsum("nki,nk->ni", Jp[fo], e[fo]))
        Wb = np.zeros((len(oc), 6, 3))
        Wb[fo] = w[fo, None, None] * np.einsum("nki,nkj->nij", Jp[fo], Jx[fo])
        if lam is None:                              # computeLambdaInit: tau * the largest diagonal entry of H
            md = 0.0
            for h in list(Hcc) + list(Hpp):
                md = max(md, float(np.diag(h).max()))
            lam = 1e-5 * md
        rho, q_max = 0.0, 0
        while True:
            if lam_trace is not None:
                lam_trace.append(lam)
            trials += 1
            ok = True
            Hl = Hpp + lam * np.eye(3)
            with np.errstate(all="ignore"):
                det = np.linalg.det(Hl) if npt else np.zeros(0)
            if npt and (np.any(det == 0) or not np.all(np.isfinite(det))):
                ok = False
            dc = np.zeros(n); dp = np.zeros((npt, 3))
            if ok:
                Hpi = np.linalg.inv(Hl) if npt else np.zeros((0, 3, 3))
                S = np.zeros((F, F, 6, 6)); g = bc.copy()
                for c in range(F):
                    S[c, c] = Hcc[c] + lam * np.eye(6)
                Y = np.einsum("nij,njk->nik", Wb, Hpi[op]) if len(oc) else np.zeros((0, 6, 3))
                np.add.at(g, oc_col[fo], -np.einsum("nij,nj->ni", Y[fo], bp[op[fo]]))
                if len(j1s):
                    np.add.at(S, (oc_col[j1s], oc_col[j2s]), -np.einsum("nij,nkj->nik", Y[j1s], Wb[j2s]))
                S = S.transpose(0, 2, 1, 3).reshape(n, n)
                if n:
                    try:
                        with np.errstate(all="ignore"):
                            L = np.linalg.cholesky(S)
                            dc = np.linalg.solve(L.T, np.linalg.solve(L, g.reshape(-1)))
                    except np.linalg.LinAlgError:
                        ok = False
                    if not np.all(np.isfinite(dc)):
                        ok = False
            tmp, scale = DBL_MAX, 0.0
            if ok:
                rhs = bp.copy()
                np.add.at(rhs, op[fo], -np.einsum("nij,ni->nj", Wb[fo], dc.reshape(-1, 6)[oc_col[fo]]))
                dp = np.einsum("pij,pj->pi", Hpi, rhs)
                dp[~seen] = 0.0
                T2 = T.copy(); quat2 = dict(quat)
                for c, k in enumerate(free):
                    quat2[k], T2[k] = pose_update(dc[6 * c:6 * c + 6], quat[k], T[k])
                X2 = X + dp
                with np.errstate(all="ignore"):
                    e2, q2 = residuals(T2, X2, oc, op, xy, f, cx, cy)
                    rho2, w2 = robust(e2, delta)
                    tmp = seq_sum(rho2)
                    scale = seq_sum(dc * (lam * dc + bc.reshape(-1))) + seq_sum((dp * (lam * dp + bp)).reshape(-1))
                if not np.isfinite(tmp):
                    tmp = DBL_MAX
            else:
                dc = np.zeros(n)
            with np.errstate(all="ignore"):
                rho = (cur - tmp) / (scale + 1e-3)
            if rho > 0 and tmp < DBL_MAX:
                t3 = 2 * rho - 1
                alpha = min(1.0 - t3 * t3 * t3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0
                cur, w, e, q, T, X, quat = tmp, w2, e2, q2, T2, X2, quat2
                out["accepts"].append(1)
            else:
                out["accepts"].append(0)
                with np.errstate(all="ignore"):
                    lam *= ni; ni *= 2
                if not np.isfinite(lam):
                    break
            q_max += 1
            if not (rho < 0 and q_max < 10):
                break
        if q_max == 10 or rho == 0 or not np.isfinite(lam):
            break
    out.update(poses=T, points=X, chi2_after=cur, iterations=n_it, trials=trials)
    return out


# ---------------------------------------------------------------- seeded maps
def make_map(seed, ncam=6, npt=300, nfixed=2, vis=0.8, noise=0.5, outliers=0.05, pert_t=0.05, pert_r=0.01, pert_x=0.05,
             min_views=3):
    """Cameras along a baseline, points 6-12 units deep, `noise` px Gaussian noise, start perturbed by pert_*.  The first
    nfixed cameras are fixed AT THEIR TRUE POSES (the reference froze them after earlier optimisation).  With min_views
    = 3 every point is seen by >= 3 cameras and a gross outlier (20 px) only hits a point seen by >= 4 (at most one per
    point): with nfixed >= 2 that fixes the gauge and keeps the minimum well conditioned.  min_views = 2, nfixed = 1 is the
    reference's initialize_map shape: scale stays free."""
    rng = np.random.default_rng(seed)
    Xt = np.c_[rng.uniform(-4, 4, npt), rng.uniform(-2, 2, npt), rng.uniform(6, 12, npt)]
    Tt = np.zeros((ncam, 3, 4))
    for c in range(ncam):
        Tt[c, :, :3], _ = se3_exp(np.r_[rng.normal(0, 0.03, 3), 0, 0, 0])
        Tt[c, :, 3] = [-0.4 * c, 0.05 * rng.normal(), 0.05 * rng.normal()]
    oc, op, xy = [], [], []
    for p in range(npt):
        cams = [c for c in range(ncam) if rng.random() < vis]
        for c in range(ncam):
            if len(cams) >= min(min_views, ncam):
                break
            if c not in cams:
                cams.append(c)
        for c in sorted(cams):
            oc.append(c); op.append(p); xy.append(project(Tt[c], Xt[p]) + rng.normal(0, noise, 2))
    oc, op, xy = np.array(oc, np.int32), np.array(op, np.int32), np.array(xy)
    cnt = np.bincount(op, minlength=npt)
    hit = np.zeros(npt, bool)
    for i in range(len(oc)):
        if cnt[op[i]] >= 4 and not hit[op[i]] and rng.random() < outliers:
            xy[i] += rng.normal(0, 20, 2); hit[op[i]] = True
    T0 = Tt.copy()
    for c in range(nfixed, ncam):
        dR, dt = se3_exp(np.r_[rng.normal(0, pert_r, 3), rng.normal(0, pert_t, 3)])
        T0[c, :, :3] = dR @ Tt[c, :, :3]; T0[c, :, 3] = dR @ Tt[c, :, 3] + dt
    X0 = Xt + rng.normal(0, pert_x, Xt.shape)
    fixed = np.zeros(ncam, bool); fixed[:nfixed] = True
    return dict(poses=T0, fixed=fixed, points=X0, oc=oc, op=op, xy=xy, poses_true=Tt, points_true=Xt)


def args(m):
    return m["poses"], m["fixed"], m["points"], m["oc"], m["op"], m["xy"]


BANDED_FIXED, BANDED_VIEWS = 2, 8


def banded_map(free, seed=0, per_camera=300):
    """A flight's shape for hundreds of cameras (bench_ba_large.py and the parity cases past 128 free cameras): free + 2 cameras
    0.4 apart along x looking down z, the first two fixed at their true poses, points 6-12 deep; a point is seen by 8 consecutive
    cameras, about per_camera points per camera.  Returns lm's arguments: poses, fixed, points, obs_cam, obs_pt, obs_xy."""
    rng = np.random.default_rng(seed)
    ncam = free + BANDED_FIXED
    npt = ncam * per_camera // BANDED_VIEWS
    Tt = np.zeros((ncam, 3, 4))
    for c in range(ncam):
        Tt[c, :, :3], _ = se3_exp(np.r_[rng.normal(0, 0.02, 3), 0, 0, 0])
        Tt[c, :, 3] = [-0.4 * c, 0.05 * rng.normal(), 0.05 * rng.normal()]
    start = rng.integers(0, ncam - BANDED_VIEWS + 1, npt)
    mid = 0.4 * (start + 0.5 * (BANDED_VIEWS - 1))
    Xt = np.c_[mid + rng.uniform(-1.5, 1.5, npt), rng.uniform(-2, 2, npt), rng.uniform(6, 12, npt)]
    oc = (start[:, None] + np.arange(BANDED_VIEWS)[None]).ravel().astype(np.int32)
    op = np.repeat(np.arange(npt), BANDED_VIEWS).astype(np.int32)
    xy = np.array([project(Tt[c], Xt[p]) for c, p in zip(oc, op)]) + rng.normal(0, 0.5, (len(oc), 2))
    T0 = Tt.copy()
    for c in range(BANDED_FIXED, ncam):
        dR, dt = se3_exp(np.r_[rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)])
        T0[c, :, :3] = dR @ Tt[c, :, :3]; T0[c, :, 3] = dR @ Tt[c, :, 3] + dt
    fixed = np.zeros(ncam, bool); fixed[:BANDED_FIXED] = True
    return T0, fixed, Xt + rng.normal(0, 0.05, Xt.shape), oc, op, xy


# ---------------------------------------------------------------- parity cases and the tolerance rule
# (seed, cameras, fixed, points, visibility, iterations).  Gauge fixed (>= 2 fixed cameras at their true poses), every point
# seen by >= 3 cameras: 3-18 cameras; 1, 2, 12 and 16 free; 50-3000 points.  40 iterations as the reference runs wherever the
# run is still descending at iteration 40.  A run that reaches the rounding floor earlier goes on deciding accept / reject by
# the last bit of chi2, differently in ANY two summation orders (two CPU orders disagreed at 40 iterations on seeds 14, 17, 21
# and on 6 of 6 seeds of the 3-camera shape, which has no point seen by 4 cameras, hence no gross outlier, and converges
# quadratically in about 10 iterations).  By the rule below that is no parity case; instead of replacing those seeds the
# same maps are compared after 14 (3 cameras: 8) iterations, before the floor.  No seed was replaced.
PARITY_CASES = [
    (11, 3, 2, 50, 1.0, 8), (12, 3, 2, 400, 1.0, 8), (13, 4, 2, 120, 0.9, 40), (14, 6, 4, 300, 0.8, 14), (15, 6, 5, 300, 0.8, 40),
    (16, 8, 6, 500, 0.6, 40), (17, 18, 16, 600, 0.4, 14), (18, 18, 16, 3000, 0.3, 40), (19, 18, 17, 600, 0.4, 40), (20, 14, 2, 300, 0.5, 40),
    (21, 18, 6, 400, 0.4, 14), (22, 18, 2, 600, 0.4, 40), (23, 18, 2, 1200, 0.3, 40), (24, 18, 6, 500, 0.4, 40), (25, 18, 16, 800, 0.4, 40),
]
# The reference's initialize_map shape (camera 1 fixed, camera 2 free) and the next frame's (1 fixed, 2 free): the cost is flat
# along global scale, so only chi2, the counts, R and t / X divided by |t| of the last camera are compared; 8 iterations for
# the reason above (no outliers on points seen by 2 or 3 cameras).
GAUGE_FREE_CASES = [(51, 2, 1, 200, 1.0, 8), (52, 2, 1, 500, 1.0, 8), (53, 3, 1, 200, 1.0, 8), (54, 3, 1, 500, 1.0, 8)]


def case_map(case):
    seed, ncam, nfixed, npt, vis, _ = case
    return make_map(seed, ncam=ncam, npt=npt, nfixed=nfixed, vis=vis, min_views=3 if nfixed >= 2 else 2)


def quantities(poses, points, chi2, normalise=False):
    """The compared quantities; normalise: t and X divided by |t| of the last camera (gauge-free maps)"""
    s = np.linalg.norm(poses[-1, :, 3]) if normalise else 1.0
    return dict(R=poses[:, :, :3], t=poses[:, :, 3] / s, X=points / s, chi2=np.float64(chi2))


def order_floor_of(problem, iterations, seed, normalise=False, delta=1.0):
    """The same numpy LM in two summation orders: observations as given and in a seeded permutation.  Returns the first
    run, the largest difference per quantity and whether both took the same accept / reject decisions."""
    a = lm(*problem, iterations=iterations, delta=delta)
    b = lm(*problem, iterations=iterations, delta=delta, order=np.random.default_rng(1000 + seed).permutation(len(problem[3])))
    qa, qb = quantities(a["poses"], a["points"], a["chi2_after"], normalise), quantities(b["poses"], b["points"], b["chi2_after"], normalise)
    return a, {k: float(np.abs(qa[k] - qb[k]).max()) for k in qa}, a["accepts"] == b["accepts"]


def order_floor(case, normalise=False):
    return order_floor_of(args(case_map(case)), case[5], case[0], normalise)


def tolerances(ref, floor, normalise=False):
    """The rule: per quantity 100 x the order floor, floored at 1e-12 relative to the quantity's largest magnitude.  The
    kernel's reduction tree is a third summation order; two decimal digits over the spread two orders already show,
    because LM amplifies a last-bit difference over its accept / reject decisions."""
    q = quantities(ref["poses"], ref["points"], ref["chi2_after"], normalise)
    return {k: max(100 * floor[k], 1e-12 * float(np.abs(q[k]).max())) for k in floor}
