"""The control flow of solvePnPRansac's RANSAC loop (oracle/voo_pnp.c, k_pnp_ransac) restated in Python integers and numpy:
the random stream, the five-index draw, the adaptive iteration bound, and what follows from them about a run of the oracle
seen only through its results.  No GPU and no oracle code: tests/test_pnp_control_reference.py holds this restatement
against the oracle, tests/test_gpu_pnp_control.py holds the kernel against the oracle on the cases frozen there.

Terms: sample s (1-based) is the s-th five-subset drawn; a round is 64 consecutive samples (round 1 = samples 1..64), a group
four consecutive samples inside a round; the stream position of a sample is the index (0-based) of the first random number
its draw consumes."""
import math

import numpy as np

DEFAULT_SEED = 0xFFFFFFFFFFFFFFFF
ROUND, GROUP = 64, 4            # hypotheses per round of k_pnp_ransac / scored together
WINDOW, TABLE = 448, 8192       # PNP_STREAM numbers staged per round, RNG_TAB_N numbers tabulated per seed
WINDOW_E = 512                  # RS_STREAM: what k_ransac, the essential-matrix twin with the same sampler, stages per round
NO_STOP = 1.0 - 1e-12           # a confidence under which the adaptive bound never falls below a budget <= 4000 in these cases


def rng_stream(seed, count):
    """cv::RNG (multiply-with-carry): the first `count` 32-bit outputs for `seed`, as a list of Python integers."""
    state = (seed & 0xFFFFFFFFFFFFFFFF) or 0xFFFFFFFF
    out = []
    for _ in range(count):
        state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
        out.append(state & 0xFFFFFFFF)
    return out


def subsets(seed, n, k, m=5):
    """[(indices, start)] for the first k samples of m distinct indices below n: each index is stream % n, a value already in
    the subset is drawn again; start = stream position of the sample's first draw.  One more entry than samples would need is
    never read: the list of length k + 1 ends with ((), position after the k-th sample)."""
    assert n >= m
    state = (seed & 0xFFFFFFFFFFFFFFFF) or 0xFFFFFFFF
    pos, out = 0, []
    for _ in range(k):
        idx, start = [], pos
        while len(idx) < m:
            state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
            pos += 1
            v = (state & 0xFFFFFFFF) % n
            if v not in idx:
                idx.append(v)
        out.append((tuple(idx), start))
    out.append(((), pos))
    return out


def round_of(sample):
    """1-based round of a 1-based sample."""
    return (sample - 1) // ROUND + 1


def round_span(subs, rnd):
    """(first position, numbers consumed) of round `rnd` when all of its 64 samples are drawn; subs = subsets(seed, n, k)
    with k >= 64 * rnd."""
    a, b = subs[ROUND * (rnd - 1)][1], subs[ROUND * rnd][1]
    return a, b - a


def update_num_iters(confidence, ep, max_iters):
    """RANSACUpdateNumIters (ptsetreg.cpp) for 5 model points."""
    tiny = float(np.finfo(np.float64).tiny)
    p = min(max(confidence, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, tiny)
    denom = 1.0 - (1.0 - ep) ** 5
    if denom < tiny:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def first_accept(oracle, X, uv, K, budget, **opts):
    """The smallest iteration budget <= `budget` for which the oracle returns a model (rc == 0), by bisection: the sample
    sequence does not depend on the budget, and with a model once accepted the verdict stays.  None: no model within budget."""
    if oracle.solve_pnp_ransac(X, uv, K, iterations=budget, **opts)[0] != 0:
        return None
    lo, hi = 1, budget
    while lo < hi:
        mid = (lo + hi) // 2
        if oracle.solve_pnp_ransac(X, uv, K, iterations=mid, **opts)[0] == 0:
            hi = mid
        else:
            lo = mid + 1
    return lo


def history(oracle, X, uv, K, upto, **opts):
    """The improvement sequence [(sample number, n_inl)] of the first `upto` samples: every budget b <= upto at which the
    oracle's (mask, n_inl) changes, with a confidence under which nothing stops early.  An improvement raises n_inl
    strictly, so the budgets at which it changes are found by bisection on n_inl between two budgets that differ."""
    opts = dict(opts); opts["confidence"] = NO_STOP
    cache = {}

    def at(b):
        if b not in cache:
            rc, _, _, mask, ninl = oracle.solve_pnp_ransac(X, uv, K, iterations=b, **opts)
            cache[b] = (ninl if rc == 0 else 0, mask.tobytes())
        return cache[b]

    out = []

    def walk(lo, hi):                       # changes in (lo, hi], given the states at both ends
        if at(lo) == at(hi):
            return                          # n_inl never decreases: equal ends, no change between
        if hi == lo + 1:
            out.append((hi, at(hi)[0]))
            return
        mid = (lo + hi) // 2
        walk(lo, mid); walk(mid, hi)

    cache[0] = (0, bytes(len(X)))
    walk(0, upto)
    return out


def stop_of(hist, n, confidence, budget):
    """The serial loop replayed along an improvement sequence: `iter < niters` with niters = update_num_iters after every
    improvement.  Returns (stop, used): stop = samples the loop runs, used = the improvements among them."""
    niters = max(budget, 1)
    used = []
    for s, good in hist:
        if s > niters:
            break
        used.append((s, good))
        niters = update_num_iters(confidence, (n - good) / n, niters)
    return niters if not used else max(niters, used[-1][0]), used
