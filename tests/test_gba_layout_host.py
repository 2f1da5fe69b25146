"""CPU: what the host prepares for vo_bundle_adjust_large (visual_odometry_amd/csrc/gba_layout.h: validation, the observations
sorted by point, the CSR lists by point and by free camera, the list of S's non-empty blocks with their observation pairs, the
scratch layout) under AddressSanitizer + UBSan.  The header calls nothing of the HIP runtime, so tests/native/gba_layout_driver.cpp
(a program of its own; nothing is preloaded) runs it on the maps of tests/test_gpu_bundle_adjust_large.py and on edge shapes and
prints every list; this file holds them equal to a numpy restatement written from the rule, not from the header:
  observations sorted by point, stable in input order; a free camera's observations ascending in that order;
  blocks (c1 <= c2) by (c1, c2): every diagonal block, an off-diagonal one only if it has a pair;
  a block's pairs (one observation of c1, one of c2, on a shared point) by point, then by first and by second observation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual_odometry_amd", "csrc")
MAX_FREE, NB = 512, 48


@pytest.fixture(scope="module")
def driver():
    if not shutil.which("hipcc") or not shutil.which("make"):
        pytest.skip("no compiler for the project's headers")
    subprocess.check_call(["make", "-s", "-C", CSRC, "gba_layout_asan"])
    return os.path.join(CSRC, "gba_layout_asan")


def _run(driver, tmp_path, fixed, npt, oc, op):
    path = os.path.join(str(tmp_path), "map.txt")
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (len(fixed), npt, len(oc)))
        for v in (np.asarray(fixed).astype(int), oc, op):
            f.write(" ".join(str(int(x)) for x in v) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver, path], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = {}
    regions = []
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "region":
            regions.append((w[1], int(w[2]), int(w[3])))
        elif w[0] not in ("gba_layout_driver:", "FAIL"):
            out[w[0]] = np.array([int(x) for x in w[1:]], np.int64)
    out["regions"] = regions
    out["stdout"] = r.stdout
    return out


def _restate(fixed, npt, oc, op):
    fixed = np.asarray(fixed).astype(bool); oc = np.asarray(oc, np.int64); op = np.asarray(op, np.int64)
    free = np.flatnonzero(~fixed)
    col = -np.ones(len(fixed), np.int64); col[free] = np.arange(len(free))
    order = np.argsort(op, kind="stable")
    s_cam, s_pt = oc[order], op[order]
    pt_first = np.concatenate([[0], np.cumsum(np.bincount(op, minlength=npt))]) if npt or len(op) else np.zeros(1, np.int64)
    scol = col[s_cam] if len(s_cam) else np.zeros(0, np.int64)
    lists = [np.flatnonzero(scol == c) for c in range(len(free))]
    cam_first = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    cam_list = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    blocks = {(c, c): [] for c in range(len(free))}
    for p in range(npt):
        js = [j for j in range(pt_first[p], pt_first[p + 1]) if scol[j] >= 0]
        for j1 in js:
            for j2 in js:
                if scol[j1] <= scol[j2]:
                    blocks.setdefault((int(scol[j1]), int(scol[j2])), []).append((j1, j2))
    keys = sorted(blocks)
    blk_first = np.concatenate([[0], np.cumsum([len(blocks[k]) for k in keys])]).astype(np.int64)
    pairs = np.array([x for k in keys for x in blocks[k]], np.int64).reshape(-1)
    return dict(col=col, free_cam=free, pt_first=pt_first, s_cam=s_cam, s_pt=s_pt, s_src=order, cam_first=cam_first, cam_list=cam_list,
                blocks=np.array(keys, np.int64).reshape(-1), blk_first=blk_first, pairs=pairs)


def _check(driver, tmp_path, fixed, npt, oc, op):
    got = _run(driver, tmp_path, fixed, npt, oc, op)
    assert got["status"][0] == 0 and " 0 failures" in got["stdout"], got["stdout"][-2000:]
    ref = _restate(fixed, npt, oc, op)
    for k, v in ref.items():
        assert np.array_equal(got[k], v), (k, got[k][:20], v[:20])
    F = len(ref["free_cam"])
    ncam, npt_, nobs, nfree, n, ld, npw = got["dims"]
    assert (ncam, npt_, nobs, nfree, n) == (len(fixed), npt, len(oc), F, 6 * F) and ld >= n + 1 and ld % 8 == 0 and npw == (npt + 255) // 256
    # the layout: every region inside the allocation, on a 256-byte boundary, disjoint; S and Ld as large as the kernels index them
    total = int(got["layout_bytes"][0])
    spans = sorted((off, off + size, name) for name, off, size in got["regions"] if size)
    for off, end, name in spans:
        assert off % 256 == 0 and 0 <= off and end <= total, name
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], (a, b)
    size = {name: sz for name, _, sz in got["regions"]}
    assert size["S"] == 8 * (n + 1) * ld and size["Ld"] == 8 * NB * NB * ((n + NB - 1) // NB) and size["rec"] == 64
    assert size["pairs"] == 4 * len(ref["pairs"]) and size["W"] == 144 * nobs
    return got


LARGE_CASES = [(101, 19, 2, 300, 0.4), (105, 66, 60, 300, 0.1), (103, 40, 4, 500, 0.2), (102, 65, 2, 400, 0.1), (104, 130, 2, 600, 0.06)]


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: "seed%d_%dcam" % c[:2])
def test_lists_of_the_parity_maps(driver, tmp_path, case):
    seed, ncam, nfixed, npt, vis = case
    m = R.make_map(seed, ncam=ncam, npt=npt, nfixed=nfixed, vis=vis)
    _check(driver, tmp_path, m["fixed"], npt, m["oc"], m["op"])


def test_edge_shapes(driver, tmp_path):
    m = R.make_map(71, ncam=4, npt=40, nfixed=2)
    _check(driver, tmp_path, m["fixed"], 40, m["oc"][:0], m["op"][:0])                        # no observations: the diagonal blocks alone
    _check(driver, tmp_path, np.ones(3, bool), 40, m["oc"] % 3, m["op"])                      # no free camera: no block, S is g's empty row
    _check(driver, tmp_path, np.zeros(0, bool), 0, np.zeros(0, int), np.zeros(0, int))        # nothing at all
    keep = m["oc"] != 3
    g = _check(driver, tmp_path, m["fixed"], 42, m["oc"][keep], m["op"][keep])                # a free camera and two points without observations
    assert g["cam_first"][-1] == g["cam_first"][-2] and g["blocks"].tolist() == [0, 0, 1, 1]
    rng = np.random.default_rng(5)                                                            # unsorted input, a camera that sees a point twice
    oc = rng.integers(0, 7, 200); op = rng.integers(0, 30, 200)
    _check(driver, tmp_path, np.array([0, 1, 0, 0, 1, 0, 0], bool), 30, oc, op)


def test_refusals(driver, tmp_path):
    n = MAX_FREE + 3                                                                          # 513 free cameras, one point each
    fixed = np.zeros(n, bool); fixed[:2] = True
    got = _run(driver, tmp_path, fixed, n, np.arange(n), np.arange(n))
    assert got["status"][0] == -7 and "dims" not in got
    fixed[2] = True                                                                           # 512: the capacity itself
    got = _check(driver, tmp_path, fixed, n, np.arange(n), np.arange(n))
    assert got["dims"][3] == MAX_FREE and len(got["blocks"]) == 2 * MAX_FREE
    m = R.make_map(71, ncam=4, npt=40, nfixed=2)
    for bad_c, bad_p in ((4, 0), (-1, 0), (0, 40), (0, -1)):
        oc, op = m["oc"].copy(), m["op"].copy()
        oc[7], op[7] = bad_c, bad_p
        assert _run(driver, tmp_path, m["fixed"], 40, oc, op)["status"][0] == -1
