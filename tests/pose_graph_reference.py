"""The checker of the device pose-graph optimisation: include/vo_hip.h, section "pose graph", in numpy.  The rules are the
library's own (the reference has no counterpart, g2o is not installed anywhere this project runs).  Written differently from the
kernel on purpose: one dense Hessian over all free vertices, np.linalg.cholesky and triangular solves, every sum taken edge after edge
in input order.  `perm_seed` permutes the unknowns before the factorisation: a second solve order, whose distance from the first is
the order floor the GPU tests hold the kernel to (100 x, floored at 1e-12 relative).  Also the seeded graph generators the tests,
the layout driver's cases and tests/scripts/bench_pose_graph.py share.  A plain helper module, no test in it."""
import math

import numpy as np
from scipy.linalg import solve_triangular

VO_OK, VO_ERR_INVALID, VO_ERR_UNSUPPORTED = 0, -1, -7
MAX_VERTICES, MAX_LOOPS = 8192, 32
TH_W, TH_S, TH_LOG = 1e-2, 1e-2, 1e-8        # the header's switch-over thresholds
DBL_MAX = np.finfo(np.float64).max


# ---------------------------------------------------------------- Sim(3): 13 doubles s, R row-major, t
def hat3(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def pack(s, R, t):
    return np.r_[float(s), np.asarray(R, float).reshape(9), np.asarray(t, float).reshape(3)]


def unpack(S):
    S = np.asarray(S, float)
    return S[0], S[1:10].reshape(3, 3), S[10:13]


def identity():
    return pack(1.0, np.eye(3), np.zeros(3))


def moments(sigma):
    """m_k = integral over [0, 1] of tau^k e^(tau sigma), k = 0 .. 6: the series below TH_S, the recurrence from expm1 above"""
    m = np.empty(7)
    if abs(sigma) < TH_S:
        for k in range(7):
            acc, p = 0.0, 1.0
            for n in range(8):
                acc += p / (math.factorial(n) * (n + k + 1)); p *= sigma
            m[k] = acc
    else:
        es = math.exp(sigma)
        m[0] = math.expm1(sigma) / sigma
        for k in range(1, 7):
            m[k] = (es - k * m[k - 1]) / sigma
    return m


def rot_coef(th):
    """sin th / th and (1 - cos th) / th^2"""
    if th < TH_W:
        t2 = th * th
        return 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42)), 0.5 - t2 / 24 * (1 - t2 / 30 * (1 - t2 / 56))
    h = math.sin(0.5 * th)
    return math.sin(th) / th, 2 * h * h / (th * th)


def v_coef(th, sigma):
    """V = C I + A [w]x + B [w]x^2"""
    if th < TH_W:
        m = moments(sigma)
        t2 = th * th
        return m[1] - t2 * m[3] / 6 + t2 * t2 * m[5] / 120, m[2] / 2 - t2 * m[4] / 24 + t2 * t2 * m[6] / 720, m[0]
    C = moments(sigma)[0]
    em = math.expm1(sigma)
    h = math.sin(0.5 * th)
    a = (em + 1) * math.sin(th)                    # e^sigma sin th
    omb = 2 * h * h - em * math.cos(th)            # 1 - e^sigma cos th
    c = th * th + sigma * sigma
    return (a * sigma + omb * th) / (th * c), (C - (a * th - omb * sigma) / c) / (th * th), C


def sim3_exp(d):
    d = np.asarray(d, float)
    w, u, sigma = d[:3], d[3:6], d[6]
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = hat3(w); W2 = W @ W
    sa, ca = rot_coef(th)
    A, B, C = v_coef(th, sigma)
    return pack(math.exp(sigma), np.eye(3) + sa * W + ca * W2, (C * np.eye(3) + A * W + B * W2) @ u)


def quat_from_rot(m):
    """Eigen's Quaternion(Matrix3), w >= 0, unit norm; q = (x, y, z, w)"""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t; t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    if q[3] < 0:
        q = -q
    return q / math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def sim3_log(S):
    s, R, t = unpack(S)
    q = quat_from_rot(R)
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    if n < TH_LOG:
        x = n / q[3]
        k = 2 / q[3] * (1 - x * x / 3)
    else:
        k = 2 * math.atan2(n, q[3]) / n
    w = k * q[:3]
    sigma = math.log(s)
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = hat3(w)
    A, B, C = v_coef(th, sigma)
    return np.r_[w, np.linalg.solve(C * np.eye(3) + A * W + B * (W @ W), t), sigma]


def sim3_inverse(S):
    s, R, t = unpack(S)
    return pack(1 / s, R.T, -(R.T @ t) / s)


def sim3_compose(A, B):
    sa, Ra, ta = unpack(A); sb, Rb, tb = unpack(B)
    return pack(sa * sb, Ra @ Rb, sa * (Ra @ tb) + ta)


def sim3_matrix(S):
    s, R, t = unpack(S)
    M = np.eye(4); M[:3, :3] = s * R; M[:3, 3] = t
    return M


def hat7(d):
    M = np.zeros((4, 4)); M[:3, :3] = hat3(d[:3]) + d[6] * np.eye(3); M[:3, 3] = d[3:6]
    return M


def vee7(M):
    sigma = (M[0, 0] + M[1, 1] + M[2, 2]) / 3
    return np.array([M[2, 1], M[0, 2], M[1, 0], M[0, 3], M[1, 3], M[2, 3], sigma])


def adjoint(S):
    s, R, t = unpack(S)
    Ad = np.zeros((7, 7))
    Ad[:3, :3] = R
    Ad[3:6, :3] = hat3(t) @ R; Ad[3:6, 3:6] = s * R; Ad[3:6, 6] = -t
    Ad[6, 6] = 1
    return Ad


# ---------------------------------------------------------------- the edge
def edge_error(C, Si, Sj):
    E = sim3_compose(sim3_compose(C, Si), sim3_inverse(Sj))
    return sim3_log(E), E


def robust(e, w, delta):
    """chi2_k = sum w e^2, Huber as k_bundle_adjust: returns rho and the weight rho'"""
    e2 = 0.0
    for k in range(7):
        e2 += w[k] * (e[k] * e[k])
    s = math.sqrt(e2)
    if delta > 0 and s > delta:
        return 2 * delta * s - delta * delta, delta / s
    return e2, 1.0


# ---------------------------------------------------------------- validity and capacity
def verdict(nv, fixed, edges, info):
    """VO_OK, VO_ERR_INVALID or VO_ERR_UNSUPPORTED for one graph: indices, i != j and weights first; then capacity; then whether
    every vertex reaches a fixed one (union-find)"""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    info = np.asarray(info, np.float64).reshape(-1, 7)
    for (i, j), w in zip(edges.tolist(), info):
        if i < 0 or i >= nv or j < 0 or j >= nv or i == j:
            return VO_ERR_INVALID
        if not (np.all(np.isfinite(w)) and np.all(w > 0)):
            return VO_ERR_INVALID
    if nv > MAX_VERTICES or sum(1 for i, j in edges.tolist() if abs(i - j) != 1) > MAX_LOOPS:
        return VO_ERR_UNSUPPORTED
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        return a
    for i, j in edges.tolist():
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    anchored = {find(v) for v in range(nv) if fixed[v]}
    return VO_OK if all(find(v) in anchored for v in range(nv)) else VO_ERR_INVALID


# ---------------------------------------------------------------- Levenberg-Marquardt
def optimize(sims, fixed, edges, meas, info=None, iterations=10, huber_delta=0.0, perm_seed=None, chi2_trace=None, general_solves=False):
    """Returns dict(sims, chi2_initial, chi2_final, iterations, trials, accepts, status).  perm_seed: the unknowns are permuted
    (seeded) before the Cholesky factorisation.  chi2_trace: a list that receives chi2 after every accepted step."""
    S = np.array(sims, np.float64).reshape(-1, 13).copy()
    nv = len(S)
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    meas = np.asarray(meas, np.float64).reshape(-1, 13)
    info = np.ones((len(edges), 7)) if info is None else np.asarray(info, np.float64).reshape(-1, 7)
    st = verdict(nv, fixed, edges, info)
    out = dict(sims=S, chi2_initial=0.0, chi2_final=0.0, iterations=0, trials=0, accepts=[], status=st)
    if st != VO_OK:
        return out
    free = np.flatnonzero(~fixed)
    col = -np.ones(nv, np.int64); col[free] = np.arange(len(free))
    n = 7 * len(free)
    perm = np.arange(n) if perm_seed is None else np.random.default_rng(perm_seed).permutation(n)
    Ji = [adjoint(c) for c in meas]

    def evaluate(Sx):
        es, Es, rhos, ws = [], [], [], []
        tot = 0.0
        for k, (i, j) in enumerate(edges.tolist()):
            e, E = edge_error(meas[k], Sx[i], Sx[j])
            rho, w = robust(e, info[k], huber_delta)
            es.append(e); Es.append(E); ws.append(w)
            tot += rho
        return tot, es, Es, ws

    with np.errstate(all="ignore"):
        cur, es, Es, ws = evaluate(S)
    out["chi2_initial"] = cur
    lam, ni, n_it, trials = None, 2.0, 0, 0
    for _ in range(int(iterations)):
        n_it += 1
        H = np.zeros((n, n)); b = np.zeros(n)
        for k, (i, j) in enumerate(edges.tolist()):
            W = ws[k] * info[k]
            J = {i: Ji[k], j: -adjoint(Es[k])}
            for a in (i, j):
                if col[a] < 0:
                    continue
                ra = slice(7 * col[a], 7 * col[a] + 7)
                b[ra] -= J[a].T @ (W * es[k])
                for c in (i, j):
                    if col[c] >= 0:
                        H[ra, 7 * col[c]:7 * col[c] + 7] += J[a].T @ (W[:, None] * J[c])
        if lam is None:
            lam = 1e-5 * (float(np.diag(H).max()) if n else 0.0)
        rho, q_max = 0.0, 0
        while True:
            trials += 1
            ok = True
            d = np.zeros(n)
            if n:
                Hl = (H + lam * np.eye(n))[np.ix_(perm, perm)]
                try:
                    with np.errstate(all="ignore"):
                        L = np.linalg.cholesky(Hl)
                        if general_solves:       # a third order: LAPACK's general solver (LU with pivoting) on the two triangles
                            d[perm] = np.linalg.solve(L.T, np.linalg.solve(L, b[perm]))
                        else:
                            d[perm] = solve_triangular(L, solve_triangular(L, b[perm], lower=True), lower=True, trans=1)
                except np.linalg.LinAlgError:
                    ok = False
                if not np.all(np.isfinite(d)):
                    ok = False
            tmp, scale = DBL_MAX, 0.0
            if ok:
                S2 = S.copy()
                with np.errstate(all="ignore"):
                    for c, v in enumerate(free):
                        S2[v] = sim3_compose(sim3_exp(d[7 * c:7 * c + 7]), S[v])
                    tmp, es2, Es2, ws2 = evaluate(S2)
                    for x in (d * (lam * d + b)).tolist():
                        scale += x
            if ok and np.isfinite(tmp) and np.isfinite(scale) and scale > 0:
                rho = (cur - tmp) / scale
            else:
                rho = -1.0                            # a rejected trial
            if rho > 0:
                t3 = 2 * rho - 1
                alpha = min(1.0 - t3 * t3 * t3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0
                cur, es, Es, ws, S = tmp, es2, Es2, ws2, S2
                out["accepts"].append(1)
                if chi2_trace is not None:
                    chi2_trace.append(cur)
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
    out.update(sims=S, chi2_final=cur, iterations=n_it, trials=trials)
    return out


# ---------------------------------------------------------------- seeded graphs
def course(n, radius=10.0, wobble=0.0, seed=0):
    """n world -> camera similarities (s = 1) on a closed circular course, looking along the tangent"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 13))
    for i in range(n):
        a = 2 * math.pi * i / n
        Rwc = np.array([[-math.sin(a), 0, math.cos(a)], [math.cos(a), 0, math.sin(a)], [0, 1.0, 0]]).T   # camera axes in the world, rows
        Rwc = unpack(sim3_exp(np.r_[rng.normal(0, wobble, 3), 0, 0, 0, 0]))[1] @ Rwc if wobble else Rwc
        c = np.array([radius * math.cos(a), radius * math.sin(a), 0.3 * math.sin(3 * a)])
        out[i] = pack(1.0, Rwc, -Rwc @ c)
    return out


def relative(Si, Sj):
    """C with C S_i S_j^-1 = I"""
    return sim3_compose(Sj, sim3_inverse(Si))


def drifted(truth, seed, scale_drift=0.01, rot=0.002, trans=0.01):
    """Dead reckoning from vertex 0 with a per-step error: the start a monocular track gives"""
    rng = np.random.default_rng(seed)
    out = truth.copy()
    for i in range(1, len(truth)):
        step = relative(truth[i - 1], truth[i])
        err = sim3_exp(np.r_[rng.normal(0, rot, 3), rng.normal(0, trans, 3), scale_drift])
        out[i] = sim3_compose(sim3_compose(err, step), out[i - 1])
    return out


def make_graph(n, loops, seed=0, noise=0.0, fixed=(0,), extra_edges=(), info=None, scale_drift=0.01, start_seed=None):
    """A closed course of n vertices, chain edges (i, i + 1), the given loop edges, exact measurements plus `noise` (tangent sigma)"""
    rng = np.random.default_rng(1000 + seed)
    truth = course(n, wobble=0.02, seed=seed)
    edges = [(i, i + 1) for i in range(n - 1)] + list(loops) + list(extra_edges)
    meas = np.empty((len(edges), 13))
    for k, (i, j) in enumerate(edges):
        C = relative(truth[i], truth[j])
        meas[k] = sim3_compose(sim3_exp(rng.normal(0, noise, 7)), C) if noise else C
    fx = np.zeros(n, np.uint8); fx[list(fixed)] = 1
    start = drifted(truth, seed if start_seed is None else start_seed, scale_drift=scale_drift)
    for v in fixed:
        start[v] = truth[v]
    w = np.ones((len(edges), 7)) if info is None else np.asarray(info, float)
    return dict(sims=start, fixed=fx, edges=np.array(edges, np.int32).reshape(-1, 2), meas=meas, info=w, truth=truth)


def args(g):
    return g["sims"], g["fixed"], g["edges"], g["meas"], g["info"]


def centre_error(sims, truth):
    """mean distance between camera centres -R^T t / s"""
    d = 0.0
    for a, b in zip(sims, truth):
        sa, Ra, ta = unpack(a); sb, Rb, tb = unpack(b)
        d += np.linalg.norm(-(Ra.T @ ta) / sa + (Rb.T @ tb) / sb)
    return d / len(sims)


# ---------------------------------------------------------------- the small graphs of the GPU tests and of the layout driver
def _complete6():
    g = make_graph(6, [(i, j) for i in range(6) for j in range(i + 2, 6)], seed=26, noise=1e-3)
    return g


def _wrong_loop():
    g = make_graph(20, [(0, 19), (3, 15)], seed=29, noise=1e-3)
    g["meas"][-1] = sim3_compose(sim3_exp(np.r_[0.3, -0.2, 0.1, 1.0, -2.0, 0.5, 0.2]), g["meas"][-1])
    return g


def _capacity():
    loops = [(k, 69 - k) for k in range(32)]
    return make_graph(70, loops, seed=31, noise=1e-3)


def _weights():
    g = make_graph(12, [(1, 10)], seed=28, noise=1e-3)
    g["info"] = np.random.default_rng(28).uniform(0.5, 200.0, g["info"].shape)
    return g


# name -> (builder, huber_delta, iterations).  tests/test_gpu_bundle_adjust.py's rule for the compared count would be: 10 iterations
# where the checker's two solve orders take the same accept / reject decisions, else the largest count where they do, never below 3.
# It proved unsound on these graphs.  They converge in a few steps, after which a run accepts or rejects by the last bit of chi2,
# and two orders may still agree there by chance (adjacent_separators: the two orders agree at 10 with 10 trials, yet a third order,
# optimize(general_solves=True), decides otherwise from its eighth iteration on and ends 1e-10 away, as the kernel does with its 18
# trials: tests/test_pose_graph_reference.py::test_a_third_order_diverges_where_two_agree), or because the permutation changes
# no bit (pair: one free vertex, H all but diagonal, floor 0).  So every case is compared at decisive_iterations(): the leading
# iterations that decide by more than the last bits, where the two orders agree as well (the same test file keeps this column equal
# to the function for every case but n300, which takes too long there).  By the two-orders rule the counts would be: pair 10,
# chain5 10, loop_to_fixed 7, adjacent_separators 10, fixed_in_the_middle 8, complete6 6, duplicated_chain_edge 7, weights 8,
# huber_wrong_loop 10, n300 10, capacity 10.
SMALL_CASES = {
    "pair": (lambda: make_graph(2, [], seed=21, noise=1e-3), 0.0, 3),
    "chain5": (lambda: make_graph(5, [], seed=22, noise=1e-3), 0.0, 8),
    "loop_to_fixed": (lambda: make_graph(12, [(0, 11)], seed=23, noise=1e-3), 0.0, 4),
    "adjacent_separators": (lambda: make_graph(12, [(2, 9), (3, 9)], seed=24, noise=1e-3), 0.0, 7),
    "fixed_in_the_middle": (lambda: make_graph(9, [(0, 8)], seed=25, noise=1e-3, fixed=(4,)), 0.0, 5),
    "complete6": (_complete6, 0.0, 3),
    "duplicated_chain_edge": (lambda: make_graph(8, [(0, 7)], seed=27, noise=1e-3, extra_edges=[(3, 4), (5, 4)]), 0.0, 4),
    "weights": (_weights, 0.0, 6),
    "huber_wrong_loop": (_wrong_loop, 0.05, 6),
    "n300": (lambda: make_graph(300, [(0, 299), (40, 280)], seed=30, noise=1e-3, scale_drift=0.002), 0.0, 10),
    "capacity": (_capacity, 0.0, 9),
}


def over_capacity():
    return make_graph(70, [(k, 69 - k) for k in range(32)] + [(0, 40)], seed=32, noise=1e-3)


def invalid_graph():
    g = make_graph(6, [], seed=33, noise=1e-3)
    g["edges"] = g["edges"][[0, 1, 3, 4]]; g["meas"] = g["meas"][[0, 1, 3, 4]]; g["info"] = g["info"][[0, 1, 3, 4]]   # 3 .. 5 reach no fixed vertex
    return g


def quantities(sims, chi2):
    sims = np.asarray(sims).reshape(-1, 13)
    return dict(s=sims[:, 0], R=sims[:, 1:10], t=sims[:, 10:13], chi2=np.float64(chi2))


def order_floor(problem, iterations=10, huber_delta=0.0, seed=0):
    """The checker in its two solve orders.  Returns the first run, the largest difference per quantity, and whether both took
    the same accept / reject decisions."""
    a = optimize(*problem, iterations=iterations, huber_delta=huber_delta)
    b = optimize(*problem, iterations=iterations, huber_delta=huber_delta, perm_seed=2000 + seed)
    qa, qb = quantities(a["sims"], a["chi2_final"]), quantities(b["sims"], b["chi2_final"])
    return a, {k: float(np.abs(qa[k] - qb[k]).max()) for k in qa}, a["accepts"] == b["accepts"], b


def chi2_rounding(sims, info, chi2):
    """What no summation order can know chi2 better than.  A residual component is a difference of numbers as large as the
    graph's largest |t|, so it carries eps = 8 ulp (2^-50) of that; chi2 = sum w e^2 then moves by at most
    2 sqrt(chi2 sum w) eps + sum w eps^2 (Cauchy-Schwarz).  It matters where chi2 is a cancellation residue: a graph without loops
    fits its measurements exactly, its final chi2 is 1e-28 where the terms it began with were 1e-3."""
    eps = 2.0 ** -50 * max(1.0, float(np.abs(np.asarray(sims).reshape(-1, 13)[:, 10:13]).max()))
    sw = float(np.asarray(info).sum())
    return 2 * math.sqrt(max(float(chi2), 0.0) * sw) * eps + sw * eps * eps


CHI2_RESIDUE = 1e-24         # a final chi2 below this is a cancellation residue (its terms began at 1e-3 and more)


def tolerances(ref, floor, edges=None, info=None):
    """Per quantity 100 x the order floor, floored at 1e-12 relative to the quantity's largest magnitude.  Only where the final
    chi2 is a cancellation residue — the graph has no loop edge, so it fits its measurements exactly, or chi2_final < CHI2_RESIDUE —
    chi2's bound is also never below chi2_rounding (pass edges and info); every other case keeps the rule as it stands."""
    q = quantities(ref["sims"], ref["chi2_final"])
    tol = {k: max(100 * floor[k], 1e-12 * float(np.abs(q[k]).max())) for k in floor}
    if edges is not None:
        e = np.asarray(edges).reshape(-1, 2)
        if not np.any(np.abs(e[:, 0] - e[:, 1]) != 1) or ref["chi2_final"] < CHI2_RESIDUE:
            tol["chi2"] = max(tol["chi2"], chi2_rounding(ref["sims"], info, ref["chi2_final"]))
    return tol


def decisive_iterations(problem, huber_delta=0.0, most=10):
    """How many leading iterations of the checker decide by more than the last bits: the iteration takes one trial, accepts it,
    chi2 falls by more than 1e-6 relative and starts above 1e-26 (the rounding residue of an exact fit).  From there on a run sits
    at its rounding floor and accepts or rejects by the last bit of chi2, differently in any two summation orders.  Never below 3."""
    trace = []
    r = optimize(*problem, iterations=most, huber_delta=huber_delta, chi2_trace=trace)
    prev, k = r["chi2_initial"], 0
    while k < min(most, len(trace)) and r["accepts"][k] == 1 and prev > 1e-26 and trace[k] < prev * (1 - 1e-6):
        prev = trace[k]; k += 1
    return max(3, k)
