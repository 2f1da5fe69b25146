"""Chosen scenes for the SIFT kernels of sift_batch.hip (not a test module): name -> (image builder, parameters, want).

The whole-detector tests compare the device with the oracle on images that reach whatever they happen to reach.  Here every
case is NAMED for the branch it is for, and `want` states, in the counters of the oracle's path census (oracle.sift_census,
voo_sift_census_t in oracle/voo.h), what the scene must reach.  tests/test_sift_cases_reference.py asserts it on the CPU from
the oracle alone, so a scene that drifts off its path fails there and does not pass for nothing on the device;
tests/test_gpu_sift_chosen.py sends every case through the per-image call and through the batched path and compares
keypoints and descriptors with the oracle byte for byte.

Images are built in numpy from fixed seeds; nothing is stored.  `want` has two parts: `exact` — the census numbers the CPU
oracle gave when the table was written (the scenes whose numbers the table's specification quotes) — and `least`, minima.
A key is a census field, or field[i] for one element of a list."""
import re

import numpy as np

DEFAULTS = dict(nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10.0, sigma=1.6)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def oracle_kw(p):
    """The oracle's names for SiftDetector's / FrontEnd's parameters."""
    return dict(n_layers=p["nOctaveLayers"], contrast_threshold=p["contrastThreshold"], edge_threshold=p["edgeThreshold"], sigma=p["sigma"])


def census_get(census, key):
    m = re.fullmatch(r"(\w+)\[(\d+)\]", key)
    return census[m.group(1)][int(m.group(2))] if m else census[key]


class Case:
    def __init__(self, name, group, build, prm, exact=None, least=None, unsupported=False):
        self.name, self.group, self._build, self.params = name, group, build, prm
        self.exact, self.least, self.unsupported = exact or {}, least or {}, unsupported
        self._img = None

    def __repr__(self):
        return f"Case({self.name})"

    @property
    def img(self):
        if self._img is None:
            self._img = self._build()
            self._img.setflags(write=False)
        return self._img

    @property
    def batch_key(self):
        """Cases with equal keys can share one FrontEnd(detector="sift") batch."""
        return (self.img.shape, tuple(sorted(self.params.items())))


# ------------------------------------------------------------------ builders
def _ground(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return yy, xx, 40.0 + 0.4 * xx * 200 / w + 0.2 * yy * 200 / h


def _u8(img):
    return np.clip(img, 0, 255).astype(np.uint8)


def blobs(h, w, n, smin, smax, seed):
    """n Gaussian blobs (centre anywhere in the image, sigma smin..smax, amplitude -90..90) on a gradient: kind 1 of
    test_sift_differential_fuzz with the gradient scaled to the image size."""
    rng = np.random.default_rng(seed)
    yy, xx, img = _ground(h, w)
    for _ in range(n):
        cy, cx, sg = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(smin, smax)
        img = img + rng.uniform(-90, 90) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    return _u8(img)


def placed(h, w, spots, ground=None, base=None):
    """Gaussian blobs at stated places on the gradient (or on a constant `ground`, or on the image `base`): a spot is
    (cy, cx, sigma, amplitude) or (cy, cx, sigma along, sigma across, angle of the long axis in degrees, amplitude)."""
    yy, xx, img = _ground(h, w)
    if ground is not None:
        img = np.full((h, w), float(ground))
    if base is not None:
        img = base.astype(np.float64)
    for s in spots:
        cy, cx, sa, sb, ang, a = s if len(s) == 6 else (s[0], s[1], s[2], s[2], 0.0, s[3])
        t = np.deg2rad(ang)
        u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
        v = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        img = img + a * np.exp(-(u * u / (2 * sa * sa) + v * v / (2 * sb * sb)))
    return _u8(img)


def wide_right():
    """`wide` with six more blobs right of input column 2047.5: several records in k_sb_bucket's clamped last bucket."""
    extra = [(8, 2052.5, 1.6, 80), (30, 2058.0, 2.0, -80), (14, 2066.5, 1.6, 80), (26, 2074.0, 2.4, 80), (10, 2081.5, 1.6, -80), (30, 2088.0, 2.0, 80)]
    return placed(40, 2100, extra, base=blobs(40, 2100, 120, 1.5, 6, 2))


def peaks():
    """Step edges in an L and in a cross, and two groups of three blobs side by side: orientation histograms with several
    peaks above 0.8 of the largest."""
    h, w = 96, 128
    img = np.full((h, w), 60.0)
    img[20:50, 14:20] += 100; img[44:50, 14:44] += 100
    img[60:66, 70:110] += 100; img[45:81, 87:93] += 100
    return placed(h, w, [(18, 66, 3, 80), (18, 76, 3, 80), (26, 71, 3, 80), (75, 20, 3, 80), (75, 28, 3, 80), (83, 24, 3, 80)], base=img)


def border():
    """Twenty blobs centred within 6 pixels of the four image edges, five per edge."""
    h, w = 96, 128
    rng = np.random.default_rng(0)
    spots = []
    for _ in range(5):
        spots += [(rng.uniform(0, 6), rng.uniform(10, w - 10), rng.uniform(1.5, 5), rng.choice([-80, 80])),
                  (h - 1 - rng.uniform(0, 6), rng.uniform(10, w - 10), rng.uniform(1.5, 5), rng.choice([-80, 80])),
                  (rng.uniform(10, h - 10), rng.uniform(0, 6), rng.uniform(1.5, 5), rng.choice([-80, 80])),
                  (rng.uniform(10, h - 10), w - 1 - rng.uniform(0, 6), rng.uniform(1.5, 5), rng.choice([-80, 80]))]
    return placed(h, w, spots)


def seams():
    """150 rows: octave 0 (300 rows) has a second 256-row segment.  Pixel d of the doubled image is input position d / 2 - 1 / 4:
    blobs of sigma 1.6 centred on doubled columns 67 = 5 + 62 (first lane of strip 1) and 66 (last lane of strip 0), and on
    doubled rows 261 = 5 + 256 (first row of segment 1) and 260 (last row of segment 0)."""
    sg = 1.6
    return placed(150, 130, [(30, 33.25, sg, 80), (60, 32.75, sg, -80), (130.25, 70, sg, 80), (129.75, 100, sg, -80),
                             (90, 95.25, sg, 70), (100, 94.75, sg, -70)])


def refine():
    """On a constant ground (with seven layers and contrastThreshold 0.03 the extrema threshold is floor(0.5 * 0.03 / 7 * 255)
    = 0, so the flat parts are candidates that meet d == 0): top left a ridge with a shallow saddle centred on a pixel of the
    doubled image, its axis at atan(1 / 2) to the rows — a 3 x 3 x 3 extremum whose Hessian has det <= 0; elsewhere forty
    blobs, some elongated, at any angle."""
    h, w = 120, 150
    rng = np.random.default_rng(0)
    ang, sa, sb = 26.57, 9.0, 3.0
    t = np.deg2rad(ang); d = 2.3 * sa / 2; cy, cx = 32.25, 40.25
    spots = [(cy - d * np.sin(t), cx - d * np.cos(t), sa, sb, ang, 90), (cy + d * np.sin(t), cx + d * np.cos(t), sa, sb, ang, 90)]
    while len(spots) < 42:
        y, x = rng.uniform(0, h), rng.uniform(0, w)
        if y < 72 and x < 88:
            continue
        s2 = rng.uniform(1.2, 4)
        spots.append((y, x, s2 * rng.choice([1, 1, 1.3, 3]), s2, rng.uniform(0, 180), rng.uniform(-90, 90)))
    return placed(h, w, spots, ground=100.0)


# ------------------------------------------------------------------ the table
# exact: every census field that is not zero, as the CPU oracle gave it when the table was written (fields not named are 0)
_SCENE_A = lambda: blobs(120, 150, 40, 1.5, 9, 1)
_TAPS_DEFAULT = [11, 11, 13, 17, 21, 27]

CASES = [
    # ---- layers: k_sb_extrema<NP> for NP = 3, 8, 9, 10; L = 1, sigma = 1.0: the 3-tap base filter and a 57-tap sweep
    Case("layers_1", "layers", _SCENE_A, params(nOctaveLayers=1, sigma=1.0), exact={
        'n_keypoints': 23, 'n_octaves': 7, 'n_taps': 4, 'taps': [3, 15, 29, 57], 'cand': [24, 0], 'cand_strip_last': [1, 0], 'cand_col_first': [1, 0],
        'ref_kept_steps': [16, 1, 0, 0, 0], 'ref_drop_steps': 2, 'ref_drop_contrast': 5, 'ori_peaks': [0, 11, 6, 0, 0], 'ori_cut': 5,
        'ori_cut_side': [2, 2, 1, 1], 'ori_max_side': 25, 'ori_sample_wrap': 113, 'kp_layer': [0, 23, 0, 0, 0, 0, 0, 0, 0], 'desc_max_radius': 27,
        'desc_max_side': 55, 'desc_cut': 13, 'desc_cut_side': [3, 6, 4, 5], 'desc_max_samples': 1493}),
    Case("layers_6", "layers", _SCENE_A, params(nOctaveLayers=6), exact={
        'n_keypoints': 23, 'n_octaves': 7, 'n_taps': 9, 'taps': [11, 9, 9, 9, 11, 11, 13, 15, 17], 'cand': [58, 18], 'cand_strip_last': [1, 0],
        'cand_col_first': [1, 0], 'cand_col_last': [1, 0], 'cand_row_last': [1, 0], 'ref_kept_steps': [13, 4, 1, 0, 0], 'ref_drop_layer': 5,
        'ref_drop_steps': 5, 'ref_drop_contrast': 30, 'ori_peaks': [0, 14, 3, 1, 0], 'ori_cut': 8, 'ori_cut_side': [3, 3, 1, 3], 'ori_max_side': 31,
        'ori_sample_wrap': 206, 'kp_layer': [0, 1, 3, 2, 9, 3, 5, 0, 0], 'desc_max_radius': 35, 'desc_max_side': 71, 'desc_cut': 18,
        'desc_cut_side': [9, 9, 5, 9], 'desc_max_samples': 2509}),
    Case("layers_7", "layers", _SCENE_A, params(nOctaveLayers=7), exact={
        'n_keypoints': 22, 'n_octaves': 7, 'n_taps': 10, 'taps': [11, 7, 9, 9, 9, 11, 11, 13, 13, 15], 'cand': [66, 23], 'cand_strip_last': [1, 0],
        'cand_col_first': [1, 0], 'cand_col_last': [1, 0], 'cand_row_last': [2, 0], 'ref_kept_steps': [14, 2, 1, 2, 0], 'ref_drop_layer': 7,
        'ref_drop_border': 2, 'ref_drop_steps': 6, 'ref_drop_contrast': 32, 'ori_peaks': [0, 16, 2, 1, 0], 'ori_cut': 10, 'ori_cut_side': [3, 5, 1, 3],
        'ori_max_side': 31, 'ori_sample_wrap': 223, 'sort_dups': 1, 'kp_layer': [0, 0, 1, 3, 6, 6, 3, 3, 0], 'desc_max_radius': 35, 'desc_max_side': 71,
        'desc_cut': 18, 'desc_cut_side': [9, 10, 5, 8], 'desc_max_samples': 1876}),
    Case("layers_8", "layers", _SCENE_A, params(nOctaveLayers=8), exact={
        'n_keypoints': 24, 'n_octaves': 7, 'n_taps': 11, 'taps': [11, 7, 7, 9, 9, 9, 11, 11, 11, 13, 13], 'cand': [75, 32], 'cand_strip_last': [1, 0],
        'cand_col_first': [1, 0], 'cand_col_last': [1, 0], 'cand_row_last': [2, 0], 'ref_kept_steps': [17, 1, 1, 0, 0], 'ref_drop_layer': 8,
        'ref_drop_border': 2, 'ref_drop_steps': 12, 'ref_drop_contrast': 34, 'ori_peaks': [0, 15, 3, 1, 0], 'ori_cut': 9, 'ori_cut_side': [4, 3, 1, 4],
        'ori_max_side': 31, 'ori_sample_wrap': 208, 'kp_layer': [0, 3, 1, 3, 1, 5, 6, 2, 3], 'desc_max_radius': 35, 'desc_max_side': 71, 'desc_cut': 20,
        'desc_cut_side': [11, 9, 5, 11], 'desc_max_samples': 1898}),
    # ---- widest_filter: k_sb_sweep<0, .> with 5 taps (base) and at its limit of 63
    Case("widest_filter", "widest_filter", _SCENE_A, params(nOctaveLayers=1, sigma=1.1), exact={
        'n_keypoints': 24, 'n_octaves': 7, 'n_taps': 4, 'taps': [5, 17, 31, 63], 'cand': [23, 0], 'cand_col_first': [1, 0],
        'ref_kept_steps': [16, 1, 0, 0, 0], 'ref_drop_steps': 3, 'ref_drop_contrast': 3, 'ori_peaks': [0, 11, 5, 1, 0], 'ori_cut': 4,
        'ori_cut_side': [1, 2, 1, 1], 'ori_max_side': 25, 'ori_sample_wrap': 134, 'kp_layer': [0, 24, 0, 0, 0, 0, 0, 0, 0], 'desc_max_radius': 27,
        'desc_max_side': 55, 'desc_cut': 13, 'desc_cut_side': [3, 7, 4, 5], 'desc_max_samples': 1513}),
    # ---- too_wide: one step above the limit; the device refuses (VO_ERR_UNSUPPORTED), the oracle has no limit
    Case("too_wide", "too_wide", _SCENE_A, params(nOctaveLayers=1, sigma=1.2), unsupported=True, least={'taps[3]': 69}),    # [7, 19, 35, 69]
    # ---- two_chunks: k_sb_descriptor's second chunk of window rows (side > 128), k_sb_orient's step_i == 0 (side > 64)
    Case("two_chunks", "two_chunks", lambda: blobs(160, 200, 40, 2, 12, 3), params(sigma=3.5), exact={
        'n_keypoints': 21, 'n_octaves': 7, 'n_taps': 6, 'taps': [29, 23, 29, 35, 45, 55], 'cand': [38, 8], 'ref_kept_steps': [12, 2, 1, 0, 0],
        'ref_drop_layer': 5, 'ref_drop_steps': 3, 'ref_drop_contrast': 15, 'ori_peaks': [0, 10, 3, 1, 1], 'ori_cut': 10, 'ori_cut_side': [5, 4, 1, 2],
        'ori_side_gt64': 5, 'ori_max_side': 69, 'ori_sample_wrap': 1127, 'sort_dups': 2, 'kp_layer': [0, 3, 6, 12, 0, 0, 0, 0, 0], 'desc_r64': 13,
        'desc_max_radius': 80, 'desc_clipped': 1, 'desc_side_gt128': 13, 'desc_max_side': 161, 'desc_cut': 19, 'desc_cut_side': [11, 7, 7, 5],
        'desc_max_samples': 11285}),
    # ---- two_chunks_small: two radii >= 64 (the larger 71) clipped to the diagonal 62 of octave 1 (40 x 48): one chunk of 125 rows
    Case("two_chunks_small", "two_chunks_small", lambda: blobs(40, 48, 6, 3, 8, 4), params(sigma=3.5), exact={
        'n_keypoints': 2, 'n_octaves': 5, 'n_taps': 6, 'taps': [29, 23, 29, 35, 45, 55], 'cand': [2, 1], 'ref_kept_steps': [0, 1, 0, 0, 0],
        'ref_drop_contrast': 1, 'ori_peaks': [0, 0, 1, 0, 0], 'ori_cut': 1, 'ori_cut_side': [1, 1, 1, 1], 'ori_max_side': 61, 'ori_sample_wrap': 89,
        'kp_layer': [0, 0, 0, 2, 0, 0, 0, 0, 0], 'desc_r64': 2, 'desc_max_radius': 71, 'desc_clipped': 2, 'desc_max_side': 125, 'desc_cut': 2,
        'desc_cut_side': [2, 2, 2, 2], 'desc_max_samples': 1748}),
    # ---- clipped_default: a radius below 64 clipped to the diagonal, cv2's default parameters
    Case("clipped_default", "clipped_default", lambda: blobs(30, 34, 6, 2, 6, 5), params(), exact={
        'n_keypoints': 1, 'n_octaves': 5, 'n_taps': 6, 'taps': _TAPS_DEFAULT, 'cand': [2, 0], 'cand_col_last': [1, 0], 'cand_row_last': [1, 0],
        'ref_kept_steps': [1, 0, 0, 0, 0], 'ref_drop_steps': 1, 'ori_peaks': [0, 1, 0, 0, 0], 'ori_cut': 1, 'ori_cut_side': [1, 1, 1, 1],
        'ori_max_side': 27, 'ori_sample_wrap': 10, 'kp_layer': [0, 0, 1, 0, 0, 0, 0, 0, 0], 'desc_max_radius': 30, 'desc_clipped': 1,
        'desc_clipped_small': 1, 'desc_max_side': 45, 'desc_cut': 1, 'desc_cut_side': [1, 1, 1, 1], 'desc_max_samples': 195}),
    # ---- wide: k_sb_bucket / k_sb_rank's clamped last bucket (x >= 4095 in doubled coordinates).  The scene as specified puts ONE
    #      record there (largest x 2093.3); wide_right adds blobs at the right end: 23 records in 7 integer columns share the bucket
    Case("wide", "wide", lambda: blobs(40, 2100, 120, 1.5, 6, 2), params(), exact={
        'n_keypoints': 97, 'n_octaves': 5, 'n_taps': 6, 'taps': _TAPS_DEFAULT, 'cand': [151, 28], 'cand_strip_first': [2, 0], 'cand_strip_last': [2, 0],
        'cand_row_first': [7, 1], 'cand_row_last': [2, 0], 'ref_kept_steps': [54, 1, 0, 0, 0], 'ref_drop_layer': 19, 'ref_drop_border': 3,
        'ref_drop_steps': 15, 'ref_drop_contrast': 59, 'ori_peaks': [0, 27, 17, 8, 3], 'ori_cut': 35, 'ori_cut_side': [21, 18, 0, 1], 'ori_max_side': 33,
        'ori_sample_wrap': 350, 'ori_bin_neg': 2, 'sort_x_clamped': 1, 'sort_x_clamped_cols': 1, 'kp_layer': [0, 25, 29, 43, 0, 0, 0, 0, 0],
        'desc_max_radius': 38, 'desc_max_side': 77, 'desc_cut': 90, 'desc_cut_side': [67, 71, 0, 1], 'desc_max_samples': 2817}),
    Case("wide_right", "wide", wide_right, params(), least={'sort_x_clamped': 2, 'sort_x_clamped_cols': 2, 'n_keypoints': 100}),
    # ---- peaks: 2, 3 and >= 4 orientations of one extremum; a peak whose interpolated bin is negative
    Case("peaks", "peaks", peaks, params(), least={'ori_peaks[2]': 1, 'ori_peaks[3]': 1, 'ori_peaks[4]': 1, 'ori_bin_neg': 1}),
    # ---- border: windows cut at the top, bottom, left and right; candidates on the outermost rows and the last column searched
    Case("border", "border", border, params(), least={
        'ori_cut_side[0]': 1, 'ori_cut_side[1]': 1, 'ori_cut_side[2]': 1, 'ori_cut_side[3]': 1, 'desc_cut_side[0]': 1, 'desc_cut_side[1]': 1,
        'desc_cut_side[2]': 1, 'desc_cut_side[3]': 1, 'cand_row_first[0]': 1, 'cand_row_last[0]': 1, 'cand_col_last[0]': 1}),
    # ---- seams: candidates of octave 0 on both sides of a strip seam and of a segment seam of k_sb_extrema
    Case("seams", "seams", seams, params(), least={'cand_strip_first[1]': 1, 'cand_strip_last[1]': 1, 'cand_seg_first[1]': 1, 'cand_seg_last[1]': 1}),
    # ---- refine: every way out of adjustLocalExtrema but the INT_MAX / 3 one
    Case("refine", "refine", refine, params(nOctaveLayers=7, contrastThreshold=0.03, edgeThreshold=8.0), least={
        'ref_kept_steps[0]': 1, 'ref_kept_steps[1]': 1, 'ref_kept_steps[2]': 1, 'ref_drop_layer': 1, 'ref_drop_border': 1, 'ref_drop_contrast': 1,
        'ref_drop_det': 1, 'ref_drop_edge': 1}),
]
# counters a scene may or may not reach; recorded by test_sift_cases_reference.py's census table, required of no case
OPTIONAL = ("ref_drop_steps", "ref_drop_huge", "ref_singular", "ori_snapped")
GROUPS = ("layers", "widest_filter", "too_wide", "two_chunks", "two_chunks_small", "clipped_default", "wide", "peaks", "border", "seams", "refine")
BY_NAME = {c.name: c for c in CASES}
# the batched path's list capacities follow kp_cap; refine's flat ground makes 52594 candidates (vo_batch_configure_sift keeps
# max(8 kp_cap, 65536) of them per frame)
KP_CAP = {"refine": 16384}


def census(O, case):
    if getattr(case, "_census", None) is None:
        case._census = O.sift_census(case.img, **oracle_kw(case.params))
    return case._census


def expected(O, case):
    """oracle.sift_detect_and_compute of the case, computed once."""
    if getattr(case, "_expected", None) is None:
        case._expected = O.sift_detect_and_compute(case.img, **oracle_kw(case.params))
    return case._expected


# Cases that go into one FrontEnd(detector="sift") batch together (same size, same parameters); every case the device
# supports is in exactly one.  tests/test_gpu_sift_chosen.py adds random_image frames until a batch has three different ones.
BATCHES = (("layers_1",), ("layers_6",), ("layers_7",), ("layers_8",), ("widest_filter",), ("two_chunks",), ("two_chunks_small",),
           ("clipped_default",), ("wide", "wide_right"), ("peaks", "border"), ("seams",), ("refine",))
# batches of which one pair also goes through the matcher (operand image and norms of the rows are read)
PAIRED = (("two_chunks",), ("wide", "wide_right"), ("layers_8",))
