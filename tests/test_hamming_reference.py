"""CPU: the numpy statement of the Hamming matchers (tests/hamming_reference.py) against the oracle's C (oracle/voo_match.c) on every
case tests/test_gpu_match_orb_rows.py runs, and every case held to what it is named for — two independently written references
agree before a device is involved, and a case that has drifted off its path fails here instead of passing quietly on the GPU."""
import numpy as np
import pytest

import hamming_reference as R

ORACLE_MODE = {"nearest": 0, "legacy": 1, "mutual": 2}


def _agree(oracle, ref, ratios):
    q, t = ref.q, ref.t
    for mode, om in ORACLE_MODE.items():
        oq, ot, od = oracle.match_hamming(q, t, om)
        gq, gt, gd = ref.select(mode)
        assert np.array_equal(gq, oq) and np.array_equal(gt, ot), mode
        assert gd.dtype == np.float32 and np.array_equal(gd, od), mode
    idx, d = oracle.knn2_hamming(q, t)
    gi, gd = ref.knn2()
    k = gi.shape[1]
    assert np.array_equal(gi, idx[:, :k]) and np.array_equal(gd, d[:, :k])
    for ratio in ratios:
        oq, ot, od = oracle.knn2_ratio_hamming(q, t, ratio)
        gq, gt, gd = ref.select("ratio", ratio)
        assert np.array_equal(gq, oq) and np.array_equal(gt, ot) and np.array_equal(gd, od), ratio


@pytest.mark.parametrize("name", R.GROUPS)
def test_numpy_statement_equals_the_oracle(oracle, name):
    g = R.group(name)
    for a, b in g.pairs:
        _agree(oracle, g.ref(a, b), g.ratios)


SMALL = ("ties", "shrink")


@pytest.mark.parametrize("name", SMALL)
def test_chunked_two_nearest_is_the_stable_argsort_of_the_xor_popcount(name):
    g = R.group(name)
    for a, b in g.pairs:
        q, t = g.sets[a], g.sets[b]
        if len(q) * len(t) > 400 * 400:
            q, t = q[:400], t[-400:]
        D = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2).astype(np.int32)       # the definition
        assert np.array_equal(R.hamming_matrix(q, t), D)
        if D.size == 0:
            continue
        order = np.argsort(D, axis=1, kind="stable")[:, :2]
        idx, d = R.two_nearest_rows(q, t)
        assert np.array_equal(idx, order) and np.array_equal(d, np.take_along_axis(D, order, 1))


def test_chunks_join_without_a_seam():
    g = R.group("remainders")
    q, t = g.sets[2256], g.sets[1537]                     # three chunks of query rows
    idx, d = R.two_nearest_rows(q, t)
    i2, d2 = R.two_nearest(R.hamming_matrix(q, t))
    assert np.array_equal(idx, i2) and np.array_equal(d, d2)


# ------------------------------------------------------------------ every case is what it is named for
def test_capacities_and_kernel_rule():
    for name in R.GROUPS:
        g = R.group(name)
        for k, rows in g.sets.items():
            assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.shape[1] == 32 and len(rows) <= g.kp_cap, (name, k)
    assert R.group("remainders").kp_cap == R.group("ties").kp_cap == R.group("shrink").kp_cap == 2256
    assert R.group("edge4096").kp_cap == 4096 and R.group("edge4104").kp_cap == 4104
    for cap, (nf, kernel) in R.INDEX_LIMITS.items():
        g = R.group(f"limit{cap}")
        assert g.kp_cap == cap == R.kp_cap_for(nf) and R.kernel_for("mfma_fp4", cap) == kernel == g.kernel
        assert len(g.sets["bigA"]) == len(g.sets["bigB"]) == cap and len(g.sets["small"]) == 600
    # the last capacity of each kernel and the first of its fallback
    assert [R.kernel_for("mfma_fp4", c) for c in (8184, 8192, 16128, 16136)] == ["mfma_fp4", "mfma", "mfma", "popcount"]
    assert R.kernel_for("mfma", 16128) == "mfma" and R.kernel_for("mfma", 16136) == "popcount" and R.kernel_for("popcount", 8) == "popcount"


def test_remainder_pairs_cover_the_issue():
    g = R.group("remainders")
    assert set(g.sets) == set(R.REMAINDER_COUNTS) and all(len(g.sets[n]) == n for n in g.sets)
    assert list(g.sets)[-1] == 2256 == g.kp_cap                                         # n == kp_cap, in the last slot
    fwd = g.launches[:len(g.launches) // 2]
    assert g.launches[len(fwd):] == [l[::-1] for l in fwd]                              # every launch once more, reversed
    assert sorted(len(l) for l in fwd) == [7, 7, 8, 8]
    gx = (g.kp_cap + 511) // 512
    assert gx == 5 and {gx * len(l) % 8 for l in fwd} == {0, 3}                         # 40 workgroups on, 35 off a multiple of the 8 XCDs
    pairs = [p for l in fwd for p in l]
    assert {n for p in pairs for n in p} == set(R.REMAINDER_COUNTS)
    assert sum(a == b for a, b in pairs) >= 2 and (2255, 2255) in pairs                 # a slot with itself
    assert any(a == 0 and b > 0 for a, b in pairs) and any(b == 0 and a > 0 for a, b in pairs)      # empty on either side
    q, t = {a for a, b in pairs}, {b for a, b in pairs}
    assert len(q & t) >= 20                                                             # query in one pair, train in another
    assert any(a <= 2 and b >= 1025 for a, b in pairs) and any(b <= 2 and a >= 1025 for a, b in pairs)   # small and large meet both ways
    r = g.ref(1537, 2256)                                 # perturbed copies of one pool: the nearest neighbours mean something
    assert (r.fd[:, 0] < 30).all() and (r.fd[:, 1] > 80).mean() > 0.99
    assert len(np.unique(r.fidx[:, 0] // 512)) == 5       # winners in all five blocks


def test_tie_cases_hold_their_ties():
    g = R.group("ties")
    for a, b in (("q300", "t280"), ("q17", "t900")):
        r = g.ref(a, b)
        for q, (i, j) in R.TIE_COLUMNS.items():           # query q is base row q: first and second neighbour tied at the chosen columns
            if j >= r.nt:
                assert (a, b) == ("q300", "t280") and q == 5
                continue
            assert list(r.fidx[q]) == [i, j] and r.fd[q, 0] == r.fd[q, 1] == 0
            assert list(np.nonzero(r.D[q, :j + 1] == 0)[0]) == [i, j]
        assert r.nt == 900 or r.nt == 280
    (i, j) = R.TIE_COLUMNS[0]; assert i // 16 == j // 16
    (i, j) = R.TIE_COLUMNS[1]; assert j == i + 16 and (i // 16) % 2 == 0 and i // 128 == j // 128       # groups g, g + 1 of one FP4 step
    (i, j) = R.TIE_COLUMNS[2]; assert i // 128 != j // 128
    (i, j) = R.TIE_COLUMNS[3]; assert i // 64 != j // 64 and i // 128 == j // 128
    (i, j) = R.TIE_COLUMNS[4]; assert i // 256 != j // 256
    (i, j) = R.TIE_COLUMNS[5]; assert i // 512 != j // 512
    r = g.ref("q300", "t280")
    tied01 = r.fd[:, 0] == r.fd[:, 1]
    assert tied01.mean() > 0.9 and ((r.fd[:, 0] > 0) & tied01).sum() > 20               # ties at a distance > 0 too
    assert np.array_equal(r.select("ratio", 1.0)[0], np.nonzero(r.fd[:, 0] < r.fd[:, 1])[0])
    # a ratio above 1 keeps the tied ones: the index shown is the first of the equals
    kept = r.select("ratio", 1.5)[0]
    tied = kept[r.fd[kept, 0] == r.fd[kept, 1]]
    assert len(tied) > 20 and (r.fd[tied, 0] > 0).all()
    for q in tied:
        assert r.fidx[q, 0] == np.nonzero(r.D[q] == r.fd[q, 0])[0][0] < r.fidx[q, 1]


def test_query_duplicates_tie_in_the_reverse_direction():
    g = R.group("ties")
    qd, td = g.sets["qd1100"], g.sets["td300"]
    r = g.ref("qd1100", "td300")
    (i, j) = R.TIE_QUERY_ROWS[0]; assert i // 4 == j // 4                               # one lane's row quad
    (i, j) = R.TIE_QUERY_ROWS[1]; assert i // 16 != j // 16 and i // 64 == j // 64      # two 16-row blocks of one wave
    (i, j) = R.TIE_QUERY_ROWS[2]; assert i // 64 != j // 64 and i // 512 == j // 512    # two waves
    (i, j) = R.TIE_QUERY_ROWS[3]; assert i // 512 != j // 512                           # two 512-row blocks
    for c, (i, j) in zip(R.TIE_QUERY_TRAIN, R.TIE_QUERY_ROWS):
        assert np.array_equal(qd[i], qd[j]) and np.array_equal(td[c], qd[i])
        assert list(np.nonzero(r.D[:, c] == 0)[0]) == [i, j]                           # the two equal candidates ...
        assert list(r.ridx[c]) == [i, j] and r.rd[c, 0] == r.rd[c, 1] == 0             # ... and the lower one is chosen
        mq, mt, _ = r.select("mutual")
        assert i in mq and j not in mq and mt[list(mq).index(i)] == c
        lq, lt, _ = r.select("legacy")
        assert i in lq and j not in lq
        nq_, nt_, _ = r.select("nearest")
        assert nt_[i] == c and nt_[j] == c


def test_zero_one_sets_tie_everywhere():
    g = R.group("ties")
    r = g.ref("zeros40", "ones50")
    assert (r.D == 256).all() and (r.fidx[:, 0] == 0).all() and (r.fidx[:, 1] == 1).all() and (r.ridx[:, 0] == 0).all()
    assert list(r.select("mutual")[0]) == [0] and list(r.select("mutual")[1]) == [0] and r.select("mutual")[2][0] == 256.0
    for a, b in (("mix600", "mix530"), ("mix530", "mix600"), ("mix600", "mix600")):
        r = g.ref(a, b)
        assert set(np.unique(r.D)) == {0, 256} and (r.fd == 0).all()
        first = {0: int(np.nonzero(g.sets[b][:, 0] == 0)[0][0]), 255: int(np.nonzero(g.sets[b][:, 0] == 255)[0][0])}
        assert all(r.fidx[q, 0] == first[int(g.sets[a][q, 0])] for q in range(r.nq))     # the lowest index wins everywhere
        assert len(r.select("mutual")[0]) == 2
    assert len(g.sets["mix600"]) > 512


def test_ratio_boundaries_sit_on_the_boundary():
    g = R.group("ties")
    r = g.ref("rq", "rt")
    assert [tuple(x) for x in r.fd] == list(R.RATIO_EDGE_DISTANCES)
    assert g.ratios == R.TIE_RATIOS and {0.5, 0.75, 1.0, 1.5} == set(g.ratios)
    assert 0.5 * np.float32(80) == np.float32(40) and 0.75 * np.float32(4) == np.float32(3)     # exactly equal: the strict < drops them
    assert list(r.select("ratio", 0.5)[0]) == [1, 2]
    assert list(r.select("ratio", 0.75)[0]) == [0, 1, 2, 4, 5]
    assert list(r.select("ratio", 1.0)[0]) == [0, 1, 2, 3, 4, 5]


def test_stale_rows_would_change_the_answer():
    g = R.group("shrink")
    o, s, s17 = g.sets["o2200"], g.sets["s2256"], g.sets["s17"]
    assert len(s) == 2256 == g.kp_cap and len(s17) == 17 and len(g.sets["s0"]) == 0 and np.array_equal(s17, s[:17])
    assert np.array_equal(s[17:2217], o) and all(((np.arange(17, 2256) // 512) == b).any() for b in range(5))
    assert g.launches == [[(k, "o2200"), ("o2200", k)] for k in ("s2256", "s17", "s0")]        # the same pair indices, step after step
    full_q, full_t, cut_q, cut_t = g.ref("s2256", "o2200"), g.ref("o2200", "s2256"), g.ref("s17", "o2200"), g.ref("o2200", "s17")
    # every row past the count is an exact copy of a row of the other set, in every 512-row block; none of the 17 that stay is
    assert (full_q.fd[17:, 0] == 0).all() and (cut_q.fd[:, 0] > 0).all() and (cut_t.fd[:, 0] > 0).all()
    stale = full_t.fidx[:, 0]                                                            # where a read past the count would land
    assert (full_t.fd[:, 0] == 0).all() and (stale >= 17).all() and set(np.unique(stale // 512)) == {0, 1, 2, 3, 4}
    # as query (the FP4 single pass's column partials of row blocks 1-4): the reverse neighbours of the train rows move
    assert (full_q.ridx[:, 0] >= 17).all() and set(np.unique(full_q.ridx[:, 0] // 512)) == {0, 1, 2, 3, 4} and (cut_q.ridx[:, 0] < 17).all()
    for mode in R.MODES:
        for full, cut in ((full_q, cut_q), (full_t, cut_t)):
            fq, ft, _ = full.select(mode); cq, ct, _ = cut.select(mode)
            if full is full_q and mode in ("legacy", "mutual"):      # the same 17 queries: the stale reverse neighbours take their matches
                m = fq < 17
                assert len(cq) > 0 and not (np.array_equal(fq[m], cq) and np.array_equal(ft[m], ct)), mode
            else:
                assert not (np.array_equal(fq, cq) and np.array_equal(ft, ct)), mode
    for k in (("s0", "o2200"), ("o2200", "s0")):
        for mode in R.MODES:
            assert len(g.ref(*k).select(mode)[0]) == 0


@pytest.mark.parametrize("name, na, nb", [("edge4096", 4095, 4096), ("edge4104", 4097, 4104)])
def test_single_pass_edge_sits_on_the_edge(name, na, nb):
    g = R.group(name)
    a, b = f"a{na}", f"b{nb}"
    assert g.pairs == [(a, b), (b, a)] and len(g.sets[a]) == na and len(g.sets[b]) == nb == g.kp_cap
    assert g.kernels == ("mfma_fp4",) and set(g.modes) == {"nearest", "mutual"}
    assert (g.kp_cap <= 4096) == (name == "edge4096")                                   # NN_COLS_MAX: single pass / two sweeps
    r = g.ref(a, b)
    last_group, last_block = (nb - 1) // 16 * 16, (na - 1) // 512 * 512
    assert r.fidx[5, 0] == nb - 1 >= last_group                                          # a winner in the last column (group)
    assert r.fidx[na - 1, 0] == 3 and na - 1 >= last_block                               # the last row, in the last row block
    assert r.fidx[na - 2, 0] == nb - 2 >= last_group and r.ridx[nb - 2, 0] == na - 2     # last block and last group at once, mutual
    mq = r.select("mutual")[0]
    assert na - 2 in mq and 5 in mq and len(mq) > 0.9 * na
    r = g.ref(b, a)                                                                      # the other way round
    assert r.fidx[nb - 2, 0] == na - 2 and nb - 2 >= (nb - 1) // 512 * 512              # a query of the last row block
    assert r.fidx[3, 0] == na - 1 >= (na - 1) // 16 * 16 and r.ridx[na - 1, 0] == 3     # a winner in the last column


@pytest.mark.parametrize("cap", list(R.INDEX_LIMITS))
def test_index_limit_cases_reach_the_last_index(cap):
    g = R.group(f"limit{cap}")
    want = [("small", "bigA"), ("bigA", "small"), ("small", "bigB"), ("bigB", "small")] + ([("bigB", "bigB")] if cap == 8184 else [])
    assert sorted(g.pairs) == sorted(want)                                               # both ways round
    assert g.kernels == ("mfma_fp4",) and ("legacy" in g.modes) == (cap == 16128) and {"nearest", "mutual", "ratio"} <= set(g.modes)
    A, B = g.sets["bigA"], g.sets["bigB"]
    assert np.array_equal(B[cap - 1], B[0]) and np.array_equal(A[:cap - 1], B[:cap - 1]) and not np.array_equal(A[cap - 1], A[0])
    r = g.ref("small", "bigA")
    assert (r.fidx[R.LIMIT_LAST, 0] == cap - 1).all() and (r.fd[R.LIMIT_LAST, 0] < 0.5 * r.fd[R.LIMIT_LAST, 1]).all()     # the true neighbour is the last row
    assert r.ridx[cap - 1, 0] in range(0, 10)
    assert (r.fidx[R.LIMIT_FIRST, 0] == 0).all()
    r = g.ref("small", "bigB")
    assert (r.fidx[R.LIMIT_FIRST] == [0, cap - 1]).all() and (r.fd[R.LIMIT_FIRST, 0] == r.fd[R.LIMIT_FIRST, 1]).all()     # row 0, its duplicate last
    assert (r.fidx[R.LIMIT_LAST, 0] != cap - 1).all()
    assert len(r.select("ratio")[0]) < 600 - 10 and len(r.select("ratio")[0]) > 500      # the tied ten are dropped by the ratio
    r = g.ref("bigB", "small")                                                           # the last row as a query, row index cap - 1
    assert r.fidx[cap - 1, 0] == r.fidx[0, 0] in range(10, 20) and r.ridx[r.fidx[0, 0], 0] == 0
    r = g.ref("bigA", "small")
    assert r.fidx[cap - 1, 0] in range(0, 10) and cap - 1 in r.select("mutual")[0]
    if cap == 8184:
        r = g.ref("bigB", "bigB")
        assert (r.fidx[:cap - 1, 0] == np.arange(cap - 1)).all() and list(r.fidx[cap - 1]) == [0, cap - 1] and list(r.fidx[0]) == [0, cap - 1]
        mq = r.select("mutual")[0]
        assert len(mq) == cap - 1 and cap - 1 not in mq
