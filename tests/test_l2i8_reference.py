"""CPU: the numpy statement of the SIFT matcher (tests/l2i8_reference.py) against the oracle's C (oracle/voo_match.c) on every case
tests/test_gpu_match_l2i8.py runs, and every case held to what it is named for — two independently written references agree
before a device is involved, and a case that has drifted fails here instead of passing quietly on the GPU."""
import numpy as np
import pytest

import l2i8_reference as R

ORACLE_MODE = {"nearest": 0, "legacy": 1, "mutual": 2}


def _script_ratio(idx, d, nt, ratio):
    """`for m, n in knnMatch(q, t, k=2): if m.distance < ratio * n.distance` (the reference's ratio test), on knn2_l2's arrays."""
    if nt < 2:
        return [], [], []
    qi, ti, dd = [], [], []
    for i in range(len(idx)):
        if float(d[i, 0]) < ratio * float(d[i, 1]):
            qi.append(i); ti.append(int(idx[i, 0])); dd.append(d[i, 0])
    return qi, ti, dd


def _agree(oracle, ref, q, t, ratio):
    qf, tf = q.astype(np.float32), t.astype(np.float32)
    for mode, om in ORACLE_MODE.items():
        oq, ot, od = oracle.match_l2(qf, tf, om)
        gq, gt, gd = ref.select(mode)
        assert np.array_equal(gq, oq) and np.array_equal(gt, ot), mode
        assert gd.dtype == np.float32 and np.array_equal(gd, od), mode
    idx, d = oracle.knn2_l2(qf, tf)
    gi, gd = ref.knn2()
    k = gi.shape[1]
    assert np.array_equal(gi, idx[:, :k]) and np.array_equal(gd, d[:, :k])
    gq, gt, gd = ref.select("ratio", ratio)
    sq, st, sd = _script_ratio(idx, d, len(t), ratio)
    assert list(gq) == sq and list(gt) == st and np.array_equal(gd, np.array(sd, np.float32))


@pytest.mark.parametrize("name", R.GROUPS)
def test_numpy_statement_equals_the_oracle(oracle, name):
    g = R.group(name)
    for a, b in g.pairs:
        _agree(oracle, g.ref(a, b), g.sets[a], g.sets[b], g.ratio)


def test_stale_flag_and_empty_cases_equal_the_oracle(oracle):
    s = R.stale_case()
    for t in (s["t300"], s["t17"], s["t17"][:0]):
        _agree(oracle, R.Pair(s["q"], t), s["q"], t, R.RATIO)
    _agree(oracle, R.Pair(s["q"][:0], s["t17"]), s["q"][:0], s["t17"], R.RATIO)


@pytest.mark.parametrize("name", [n for n in R.GROUPS if n != "edge4096"])
def test_two_nearest_is_the_stable_argsort(name):
    g = R.group(name)
    for a, b in g.pairs:
        D2 = R.d2_matrix(g.sets[a], g.sets[b])
        order = np.argsort(D2, axis=1, kind="stable")[:, :2]
        idx, d2 = R.two_nearest(D2)
        assert np.array_equal(idx, order) and np.array_equal(d2, np.take_along_axis(D2, order, 1))


def test_d2_matrix_is_exact():
    # against int64 arithmetic, on the rows with the largest products
    b = R.bound_rows().astype(np.int64)
    want = ((b[:, None, :] - b[None, :, :]) ** 2).sum(2)
    assert np.array_equal(R.d2_matrix(b, b), want.astype(np.float64))


# ------------------------------------------------------------------ every case is what it is named for
def _all_sets():
    for name in R.GROUPS:
        for k, rows in R.group(name).sets.items():
            yield f"{name}/{k}", rows
    for k, rows in R.stale_case().items():
        yield f"stale/{k}", rows


def test_rows_respect_the_norm_bound_and_the_range_argument():
    for name, rows in _all_sets():
        assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.shape[1] == 128, name
        assert (rows.astype(np.int64) ** 2).sum(1).max(initial=0) <= R.NORM_BOUND, name        # no unflagged case breaks the bound
    for name in R.GROUPS:
        g = R.group(name)
        for a, b in g.pairs:
            assert g.ref(a, b).D2.max() < 1 << 22, (name, a, b)
    f = R.flagged_row().astype(np.int64)
    assert (f * f).sum() == R.NORM_BOUND + 1


def test_sift_like_rows_look_like_sift():
    g = R.group("remainders")
    n2 = (g.sets[1025].astype(np.int64) ** 2).sum(1)
    assert abs(np.sqrt(n2) - 512).max() < 8                        # norm 512 up to rounding: |row|^2 ~ 2^18
    ref = g.ref(1025, 1025)
    assert (ref.fidx[:, 0] == np.arange(1025)).all() and (ref.fd2[:, 0] == 0).all()
    r = g.ref(513, 1025)                                          # perturbed copies of one pool: the nearest neighbours mean something
    assert (r.fd2[:, 0] < 0.5 * r.fd2[:, 1]).mean() > 0.9


def test_remainder_pairs_cover_the_issue():
    g = R.group("remainders")
    assert set(g.sets) == set(R.REMAINDER_COUNTS) and all(len(g.sets[n]) == n for n in g.sets)
    assert len(g.pairs) >= 20 and any(a == b for a, b in g.pairs)
    assert sum((b, a) in g.pairs for a, b in g.pairs if a != b) >= 6                   # both orders of several
    assert {n for p in g.pairs for n in p} == set(R.REMAINDER_COUNTS)
    assert g.kp_cap == 1280 and (g.kp_cap + 511) // 512 * len(g.pairs) > 8            # gx = 3; more workgroups than XCDs


def test_edge_cases_sit_on_the_edge():
    g = R.group("edge4096")
    assert [(len(g.sets[a]), len(g.sets[b])) for a, b in g.pairs] == [(64, 4095), (64, 4096), (64, 4097), (4096, 4096), (4097, 4100)]
    a, b = g.sets["a64"], g.sets["b4096"]
    r = g.ref("a64", "b4096")
    # one row at columns 5 and 4090: tied at distance 0, the lower index is the answer
    assert np.array_equal(b[5], a[7]) and np.array_equal(b[4090], a[7]) and r.D2[7, 5] == 0 and r.D2[7, 4090] == 0 and r.fidx[7, 0] == 5
    assert list(np.nonzero(r.D2[7] == 0)[0]) == [5, 4090]
    # the same in one lane (column % 16), groups 1 and 255: what `255 - group` in the packed key decides
    assert list(np.nonzero(r.D2[11] == 0)[0]) == [21, 4085] and 21 % 16 == 4085 % 16 and r.fidx[11, 0] == 21
    # the "last group" case: a winner at an index >= 4080 of 4096, in every train set of 4095 .. 4097 rows
    for t in ("b4095", "b4096", "b4097"):
        assert g.ref("a64", t).fidx[3, 0] == 4087
    assert g.ref("a64", "b4097").fidx[9, 0] == 4096 and g.ref("a64", "b4096").fidx[9, 0] < 4096      # group 256 exists above 4096 rows only
    r = g.ref("c4096", "b4096")
    assert r.fidx[4095, 0] == 4094 and r.ridx[4094, 0] == 4095
    r = g.ref("b4097", "d4100")
    assert r.fidx[4096, 0] == 4099 and r.ridx[4099, 0] == 4096


def test_tie_cases_hold_their_ties():
    g = R.group("ties")
    assert g.ratio == 1.0
    assert [(len(g.sets[a]), len(g.sets[b])) for a, b in g.pairs[:2]] == [(300, 280), (17, 900)]
    for a, b in g.pairs[:2]:
        r = g.ref(a, b)
        for q, (i, j) in R.TIE_COLUMNS.items():              # query q is base row q: first and second neighbour tied at the chosen columns
            assert list(r.fidx[q]) == [i, j] and r.fd2[q, 0] == r.fd2[q, 1] == 0
            assert list(np.nonzero(r.D2[q, :j + 1] == 0)[0]) == [i, j]
        (i, j) = R.TIE_COLUMNS[0]; assert i // 16 == j // 16 and i % 16 != j % 16                       # one 16-group, different lanes
        (i, j) = R.TIE_COLUMNS[1]; assert i // 16 != j // 16 and i // 128 == j // 128 and i % 16 != j % 16   # two groups of one stage
        (i, j) = R.TIE_COLUMNS[2]; assert i // 128 != j // 128                                           # two stages
        (i, j) = R.TIE_COLUMNS[3]; assert i // 16 != j // 16 and i % 16 == j % 16                       # one lane, two groups
        tied01 = r.fd2[:, 0] == r.fd2[:, 1]
        assert tied01.mean() > 0.9                            # first and second neighbour tie for nearly every query ...
        first_tied = (r.D2 == r.fd2[:, :1]).sum(1) > 1
        assert first_tied.mean() > 0.9                        # ... and so does the first with some other column
    r = g.ref("q300", "t280")
    assert ((r.fd2[:, 0] > 0) & (r.fd2[:, 0] == r.fd2[:, 1])).sum() > 20       # ties at a distance > 0 too
    assert len(r.select("ratio", 1.0)[0]) < len(r.select("nearest")[0])         # ratio 1.0 drops exactly the tied ones
    assert np.array_equal(r.select("ratio", 1.0)[0], np.nonzero(r.fd2[:, 0] < r.fd2[:, 1])[0])


def test_ties_above_ratio_one_show_the_first_of_equals(oracle):
    g = R.group("ties")
    r = g.ref("q300", "t280")
    _agree(oracle, r, g.sets["q300"], g.sets["t280"], R.TIE_RATIO_ABOVE_ONE)
    kept = r.select("ratio", R.TIE_RATIO_ABOVE_ONE)[0]
    tied = kept[r.fd2[kept, 0] == r.fd2[kept, 1]]
    assert len(tied) > 20 and (r.fd2[tied, 0] > 0).all()
    # ... and for most of them a LATER equal column sits in the winner's own lane (column % 16): what a `>=` in the per-lane
    # update of the unpacked form would pick instead
    lane = np.arange(r.nt) % 16
    later = [q for q in tied if ((r.D2[q] == r.fd2[q, 0]) & (lane == r.fidx[q, 0] % 16)).sum() > 1]
    assert len(later) > 20


def test_bound_cases_reach_the_bound():
    g = R.group("bound")
    b = g.sets["bound"].astype(np.int64)
    n2 = (b * b).sum(1)
    assert (n2 == 1 << 20).sum() >= 6 and n2[0] == 0 and (n2 == 16 * 255 * 255).sum() >= 4 and (n2 == 255 * 255).sum() >= 4
    r = g.ref("bound", "bound")
    assert r.D2.max() == 1 << 21                              # two 2^20 rows on disjoint supports: the largest d^2 met
    assert r.D2[0, 0] == 0 and r.fidx[0, 0] == 0 and r.fd2[0, 1] == 0     # the zero row against itself; the second zero row ties
    assert max(g.ref(a, c).D2.max() for a, c in g.pairs) == 1 << 21
    # |v - 128|^2 of the zero row is the largest norm the operand image can hold
    assert ((b - 128) ** 2).sum(1).max() == ((b[0] - 128) ** 2).sum() == 1 << 21


def test_stale_rows_would_change_the_answer():
    s = R.stale_case()
    q, t300, t17 = s["q"], s["t300"], s["t17"]
    assert len(t300) == 300 and len(t17) == 17 and np.array_equal(t17, t300[:17]) and np.array_equal(t300[17:32], q[:15])
    D = R.d2_matrix(q, t300)
    # every one of the rows 17..31 a frame of 17 rows leaves behind in its last 16-group would win, at distance 0, if it were read
    assert (D[np.arange(15), 17 + np.arange(15)] == 0).all() and (D[:15, :17].min(1) > 0).all()
    a, b = R.Pair(q, t17), R.Pair(q, t300[:32])
    for mode in R.MODES:
        assert not np.array_equal(a.select(mode)[1], b.select(mode)[1]) or len(a.select(mode)[0]) != len(b.select(mode)[0]), mode


def test_one_train_row_and_fuzz_shapes():
    g = R.group("one_train")
    r = g.ref("q40", "t1")
    assert (r.select("nearest")[1] == 0).all() and len(r.select("nearest")[0]) == 40 and len(r.select("ratio")[0]) == 0
    assert list(r.select("mutual")[0]) == [13] and list(r.select("legacy")[0]) == [13]
    for s in R.FUZZ_SEEDS:
        g = R.group(f"fuzz{s}")
        for k, rows in g.sets.items():
            assert 1 <= len(rows) <= 700
            if len(rows) >= 40:
                assert len(np.unique(rows, axis=0)) < len(rows)          # duplicated rows
