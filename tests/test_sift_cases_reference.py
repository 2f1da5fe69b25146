"""CPU: every case of tests/sift_cases.py reaches the branch it is named for, from the oracle alone — by the path census
(oracle.sift_census: counters inside the functions sift_detect_and_compute runs, voo_sift_census_t in oracle/voo.h).
tests/test_gpu_sift_chosen.py runs the same cases through the per-image call and the batched path on the device; a case that
drifts off its path fails here instead of passing for nothing there."""
import numpy as np
import pytest

import sift_cases as S

NAMES = [c.name for c in S.CASES]
# what a group must state, so that no scene is checked for less than it is there for: census keys of `least`, or of `exact`
# with these values at least
REQUIRED = {
    "layers": {}, "widest_filter": {"taps[3]": 63}, "too_wide": {"taps[3]": 69},
    "two_chunks": {"desc_r64": 1, "desc_side_gt128": 1, "ori_side_gt64": 1, "desc_clipped": 1},
    "two_chunks_small": {"desc_r64": 1, "desc_clipped": 1},
    "clipped_default": {"desc_clipped_small": 1},
    "wide": {"sort_x_clamped": 2, "sort_x_clamped_cols": 2},
    "peaks": {"ori_peaks[2]": 1, "ori_peaks[3]": 1, "ori_peaks[4]": 1, "ori_bin_neg": 1},
    "border": {k: 1 for k in [f"ori_cut_side[{i}]" for i in range(4)] + [f"desc_cut_side[{i}]" for i in range(4)] +
               ["cand_row_first[0]", "cand_row_last[0]", "cand_col_last[0]"]},
    "seams": {"cand_strip_first[1]": 1, "cand_strip_last[1]": 1, "cand_seg_first[1]": 1, "cand_seg_last[1]": 1},
    "refine": {"ref_kept_steps[0]": 1, "ref_kept_steps[1]": 1, "ref_kept_steps[2]": 1, "ref_drop_layer": 1, "ref_drop_border": 1,
               "ref_drop_contrast": 1, "ref_drop_det": 1, "ref_drop_edge": 1},
}


def _stated(case, key):
    """What the case's `want` promises for a census key: the exact value, or the minimum, or nothing."""
    if case.exact:
        return S.census_get({**{k: 0 for k in ("desc_r64", "desc_side_gt128", "ori_side_gt64", "desc_clipped", "desc_clipped_small",
                                               "sort_x_clamped", "sort_x_clamped_cols")}, **case.exact}, key)
    return case.least.get(key)


def test_every_group_of_the_issue_is_there():
    assert {c.group for c in S.CASES} == set(S.GROUPS) == set(REQUIRED) and len(set(NAMES)) == len(NAMES)
    by_layers = {c.params["nOctaveLayers"]: c for c in S.CASES if c.group == "layers"}
    assert sorted(by_layers) == [1, 6, 7, 8]                                  # k_sb_extrema<3>, <8>, <9>, <10>
    assert by_layers[1].exact["taps"] == [3, 15, 29, 57]
    assert all(min(by_layers[L].exact["kp_layer"][1:L + 1]) >= 1 for L in (6, 8))     # a keypoint in every layer
    for c in S.CASES:
        assert c.img.dtype == np.uint8 and c.img.ndim == 2
        assert c.img.shape[0] <= 160 and (c.img.shape[1] <= 200 or c.group == "wide"), c.name
        assert bool(c.exact) != bool(c.least) or c.unsupported, c.name
    for g, need in REQUIRED.items():
        for key, least in need.items():                                        # some case of the group states every requirement
            assert any((_stated(c, key) or 0) >= least for c in S.CASES if c.group == g), (g, key)
    assert [c.name for c in S.CASES if c.unsupported] == ["too_wide"]
    # the batches of the device test: every supported case in exactly one, same size and parameters within a batch
    assert sorted(n for b in S.BATCHES for n in b) == sorted(c.name for c in S.CASES if not c.unsupported)
    assert all(len({S.BY_NAME[n].batch_key for n in b}) == 1 for b in S.BATCHES) and set(S.PAIRED) <= set(S.BATCHES)
    assert {"two_chunks", "wide", "layers_8"} <= {n for b in S.PAIRED for n in b}


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_is_named_for(oracle, name):
    c = S.BY_NAME[name]
    cen = S.census(oracle, c)
    print(name, {k: v for k, v in cen.items() if v != 0 and not (isinstance(v, list) and not any(v))})     # the census table: pytest -s
    if c.exact:
        for key, v in cen.items():
            assert v == c.exact.get(key, [0] * len(v) if isinstance(v, list) else 0), (name, key)
    for key, least in c.least.items():
        assert S.census_get(cen, key) >= least, (name, key)
    # the census is the detector's own run: same keypoint count, and every candidate ends in exactly one exit of the refinement
    want = S.expected(oracle, c)
    assert cen["n_keypoints"] == want["n_found"] == len(want["xy"])
    exits = sum(cen["ref_kept_steps"]) + sum(cen[k] for k in ("ref_drop_layer", "ref_drop_border", "ref_drop_steps", "ref_drop_huge",
                                                             "ref_drop_contrast", "ref_drop_det", "ref_drop_edge"))
    assert exits == cen["cand"][0] and sum(cen["ori_peaks"]) == sum(cen["ref_kept_steps"])
    records = sum(n * k for n, k in enumerate(cen["ori_peaks"])) - cen["sort_dups"]      # (the last class is "4 or more")
    assert sum(cen["kp_layer"]) == cen["n_keypoints"] >= records and (cen["n_keypoints"] == records or cen["ori_peaks"][4] > 0)
    assert cen["n_octaves"] == oracle.lib().voo_sift_octaves(*c.img.shape) and len(cen["taps"]) == c.params["nOctaveLayers"] + 3
    if c.unsupported:
        assert max(cen["taps"]) > 63                                           # what the device refuses; the oracle has no limit
    else:
        assert max(cen["taps"]) <= 63 and want["n_found"] >= 1


def test_census_leaves_the_detector_alone(oracle):
    """The counters sit behind a pointer that is NULL outside sift_census: the same bytes before and after a census."""
    c = S.BY_NAME["border"]
    a = oracle.sift_detect_and_compute(c.img)
    S.census(oracle, c)
    b = oracle.sift_detect_and_compute(c.img)
    for k in ("xy", "size", "angle", "response", "octave", "desc"):
        assert np.array_equal(a[k], b[k]), k
