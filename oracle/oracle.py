"""ctypes wrapper over oracle/libvoo.so — the CPU ORACLE (test infrastructure only).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module;
nothing under visual_odometry_amd/ does.  PARITY UNPINNED (see oracle/voo.h).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("edge_threshold", C.c_int32), ("first_level", C.c_int32), ("wta_k", C.c_int32),
                ("score_type", C.c_int32), ("patch_size", C.c_int32), ("fast_threshold", C.c_int32)]


class PairResult(C.Structure):
    _fields_ = [("n_kp1", C.c_int32), ("n_kp2", C.c_int32), ("n_match", C.c_int32),
                ("n_inl_E", C.c_int32), ("n_good_pose", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("E", C.c_double * 9)]


def orb_params(nfeatures=500, scale_factor=1.2, nlevels=8, edge_threshold=31, first_level=0,
               wta_k=2, score_type=0, patch_size=31, fast_threshold=20):
    return OrbParams(nfeatures, scale_factor, nlevels, edge_threshold, first_level, wta_k,
                     score_type, patch_size, fast_threshold)


def build(force=False):
    so = os.path.join(_HERE, "libvoo.so")
    srcs = [os.path.join(_HERE, f) for f in os.listdir(_HERE) if f.endswith((".c", ".cpp", ".h", ".inc"))]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", _HERE, "libvoo.so"], stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def level_geometry(h, w, params):
    L = params.nlevels
    lw = np.zeros(L, np.int32); lh = np.zeros(L, np.int32); q = np.zeros(L, np.int32)
    ls = np.zeros(L, np.float32)
    rc = lib().voo_level_geometry(h, w, C.byref(params), _p(lw, C.c_int32), _p(lh, C.c_int32),
                                  _p(ls, C.c_float), _p(q, C.c_int32))
    assert rc == 0
    return lw, lh, ls, q


def gray(img):
    img = _u8(img)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    out = np.empty((h, w), np.uint8)
    rc = lib().voo_gray(_p(img, C.c_uint8), h, w, ch, img.strides[0], _p(out, C.c_uint8))
    assert rc == 0
    return out


def resize_linear_exact(src, dw, dh):
    src = _u8(src)
    sh, sw = src.shape
    dst = np.empty((dh, dw), np.uint8)
    rc = lib().voo_resize_linear_exact(_p(src, C.c_uint8), sw, sh, sw, _p(dst, C.c_uint8), dw, dh, dw)
    assert rc == 0
    return dst


def pyramid(gray_img, params):
    g = _u8(gray_img)
    h, w = g.shape
    lw, lh, _, _ = level_geometry(h, w, params)
    total = int((lw.astype(np.int64) * lh).sum())
    out = np.empty(total, np.uint8)
    rc = lib().voo_pyramid(_p(g, C.c_uint8), h, w, C.byref(params), _p(out, C.c_uint8))
    assert rc == 0
    levels, off = [], 0
    for l in range(params.nlevels):
        n = int(lw[l]) * int(lh[l])
        levels.append(out[off:off + n].reshape(int(lh[l]), int(lw[l])))
        off += n
    return levels


def fast_score_nms(img, threshold=20):
    img = _u8(img)
    h, w = img.shape
    out = np.empty((h, w), np.uint8)
    rc = lib().voo_fast_score_nms(_p(img, C.c_uint8), w, h, w, threshold, _p(out, C.c_uint8))
    assert rc == 0
    return out


def gaussian_blur7(img):
    img = _u8(img)
    h, w = img.shape
    out = np.empty((h, w), np.uint8)
    rc = lib().voo_gaussian_blur7(_p(img, C.c_uint8), w, h, w, _p(out, C.c_uint8), w)
    assert rc == 0
    return out


def orb_detect_and_compute(img, params, cap=None):
    img = _u8(img)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    cap = cap or (params.nfeatures * 2 + 4096)
    xy = np.zeros((cap, 2), np.float32); size = np.zeros(cap, np.float32)
    ang = np.zeros(cap, np.float32); resp = np.zeros(cap, np.float32)
    octv = np.zeros(cap, np.int32); desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int32(0)
    rc = lib().voo_orb_detect_and_compute(_p(img, C.c_uint8), h, w, ch, img.strides[0], C.byref(params),
                                          _p(xy, C.c_float), _p(size, C.c_float), _p(ang, C.c_float),
                                          _p(resp, C.c_float), _p(octv, C.c_int32), _p(desc, C.c_uint8),
                                          cap, C.byref(n))
    if rc < 0:
        raise RuntimeError(f"voo_orb_detect_and_compute failed: {rc}")
    n = n.value
    return dict(xy=xy[:n].copy(), size=size[:n].copy(), angle=ang[:n].copy(), response=resp[:n].copy(),
                octave=octv[:n].copy(), desc=desc[:n].copy(), overflow=(rc == 1))


def set_keypoint_order(order):
    """'cv2' (default): KeyPointsFilter::retainBest's libstdc++ order, the list cv2.ORB returns; 'canonical': (octave, y, x) order."""
    lib().voo_set_keypoint_order({"canonical": 0, "cv2": 1}[order])


def retain_best_cv2(response, n_points):
    """cv::KeyPointsFilter::retainBest on a response list: the kept original indices in cv2's order."""
    r = np.ascontiguousarray(response, np.float32)
    out = np.zeros(max(len(r), 1), np.int32)
    m = lib().voo_retain_best_cv2(_p(r, C.c_float), len(r), int(n_points), _p(out, C.c_int32))
    return out[:m].copy()


def match_hamming(q, t, cross_check=2):
    q = _u8(q).reshape(-1, 32); t = _u8(t).reshape(-1, 32)
    nq, nt = len(q), len(t)
    qi = np.zeros(max(nq, 1), np.int32); ti = np.zeros(max(nq, 1), np.int32); d = np.zeros(max(nq, 1), np.float32)
    n = C.c_int32(0)
    rc = lib().voo_match_hamming(_p(q, C.c_uint8), nq, _p(t, C.c_uint8), nt, int(cross_check),
                                 _p(qi, C.c_int32), _p(ti, C.c_int32), _p(d, C.c_float), C.byref(n))
    assert rc == 0
    return qi[:n.value].copy(), ti[:n.value].copy(), d[:n.value].copy()


def match_l2(q, t, cross_check=2):
    """cv2.BFMatcher(cv2.NORM_L2, crossCheck).match on float32 descriptors."""
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    nq, nt = len(q), len(t)
    dim = q.shape[1] if nq else (t.shape[1] if nt else 1)
    qi = np.zeros(max(nq, 1), np.int32); ti = np.zeros(max(nq, 1), np.int32); d = np.zeros(max(nq, 1), np.float32)
    n = C.c_int32(0)
    rc = lib().voo_match_l2(_p(q, C.c_float), nq, _p(t, C.c_float), nt, int(dim), int(cross_check),
                            _p(qi, C.c_int32), _p(ti, C.c_int32), _p(d, C.c_float), C.byref(n))
    assert rc == 0
    return qi[:n.value].copy(), ti[:n.value].copy(), d[:n.value].copy()


def knn2_ratio_hamming(q, t, ratio):
    q = _u8(q).reshape(-1, 32); t = _u8(t).reshape(-1, 32)
    nq, nt = len(q), len(t)
    qi = np.zeros(max(nq, 1), np.int32); ti = np.zeros(max(nq, 1), np.int32); d = np.zeros(max(nq, 1), np.float32)
    n = C.c_int32(0)
    lib().voo_knn2_ratio_hamming.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = lib().voo_knn2_ratio_hamming(q.ctypes.data, nq, t.ctypes.data, nt, float(ratio),
                                      qi.ctypes.data, ti.ctypes.data, d.ctypes.data, C.addressof(n))
    assert rc == 0
    return qi[:n.value].copy(), ti[:n.value].copy(), d[:n.value].copy()


def knn2_hamming(q, t):
    """matcher.knnMatch(q, t, k=2) for NORM_HAMMING: (idx [nq, 2], dist [nq, 2]); missing neighbours -1 / FLT_MAX."""
    q = _u8(q).reshape(-1, 32); t = _u8(t).reshape(-1, 32)
    idx = np.zeros((max(len(q), 1), 2), np.int32); d = np.zeros((max(len(q), 1), 2), np.float32)
    f = lib().voo_knn2_hamming
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert f(q.ctypes.data, len(q), t.ctypes.data, len(t), idx.ctypes.data, d.ctypes.data) == 0
    return idx[:len(q)], d[:len(q)]


def knn2_l2(q, t):
    """matcher.knnMatch(q, t, k=2) for NORM_L2 on float32 rows."""
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    dim = q.shape[1] if len(q) else (t.shape[1] if len(t) else 1)
    idx = np.zeros((max(len(q), 1), 2), np.int32); d = np.zeros((max(len(q), 1), 2), np.float32)
    f = lib().voo_knn2_l2
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert f(q.ctypes.data, len(q), t.ctypes.data, len(t), int(dim), idx.ctypes.data, d.ctypes.data) == 0
    return idx[:len(q)], d[:len(q)]


def set_dk_early_exit(on):
    """False (default): cv::solvePoly's fixed 300 sweeps; True: the noise-floor exit of the kernel's throughput mode."""
    lib().voo_set_dk_early_exit(int(bool(on)))


def get_dk_early_exit():
    return bool(lib().voo_get_dk_early_exit())


def five_point(x1, x2):
    x1 = np.ascontiguousarray(x1, np.float64).reshape(5, 2); x2 = np.ascontiguousarray(x2, np.float64).reshape(5, 2)
    E = np.zeros((10, 9), np.float64); n = C.c_int32(0)
    rc = lib().voo_five_point(_p(x1, C.c_double), _p(x2, C.c_double), _p(E, C.c_double), C.byref(n))
    assert rc == 0
    return E[:n.value].reshape(-1, 3, 3).copy()


def find_essential_ransac(p1, p2, K, prob=0.99, thresh=1.0, max_iters=1000, seed=0xFFFFFFFFFFFFFFFF):
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2); p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64)
    M = len(p1)
    E = np.zeros((10, 9), np.float64); mask = np.zeros(max(M, 1), np.uint8)
    ninl = C.c_int32(0); nmod = C.c_int32(0)
    f = lib().voo_find_essential_ransac
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_uint64,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(p1.ctypes.data, p2.ctypes.data, M, K.ctypes.data, prob, thresh, max_iters, seed,
           E.ctypes.data, mask.ctypes.data, C.addressof(ninl), C.addressof(nmod))
    return rc, E[:max(nmod.value, 0)].reshape(-1, 3, 3).copy(), mask[:M].copy(), ninl.value


def recover_pose(E, p1, p2, K, dist_thresh=50.0):
    E = np.ascontiguousarray(E, np.float64).reshape(3, 3)
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2); p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64)
    M = len(p1)
    R = np.zeros((3, 3)); t = np.zeros((3, 1)); mask = np.zeros(max(M, 1), np.uint8); ng = C.c_int32(0)
    f = lib().voo_recover_pose
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p]
    rc = f(E.ctypes.data, p1.ctypes.data, p2.ctypes.data, M, K.ctypes.data, dist_thresh, R.ctypes.data,
           t.ctypes.data, mask.ctypes.data, C.addressof(ng))
    assert rc == 0
    return ng.value, R, t, mask[:M].copy()


def recover_pose_counts(E, p1, p2, K, dist_thresh=50.0):
    """recover_pose with what decides it: (good[4] of the candidates (R1,t) (R2,t) (R1,-t) (R2,-t), best, R, t, mask)."""
    E = np.ascontiguousarray(E, np.float64).reshape(3, 3)
    p1 = np.ascontiguousarray(p1, np.float64).reshape(-1, 2); p2 = np.ascontiguousarray(p2, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64)
    M = len(p1)
    R = np.zeros((3, 3)); t = np.zeros((3, 1)); mask = np.zeros(max(M, 1), np.uint8)
    good = np.zeros(4, np.int32); best = C.c_int32(0)
    f = lib().voo_recover_pose_counts
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(E.ctypes.data, p1.ctypes.data, p2.ctypes.data, M, K.ctypes.data, dist_thresh, R.ctypes.data,
           t.ctypes.data, mask.ctypes.data, good.ctypes.data, C.addressof(best))
    assert rc == 0
    return good, best.value, R, t, mask[:M].copy()


def triangulate(P1, P2, x1, x2):
    P1 = np.ascontiguousarray(P1, np.float64).reshape(3, 4); P2 = np.ascontiguousarray(P2, np.float64).reshape(3, 4)
    x1 = np.ascontiguousarray(x1, np.float64).reshape(2, -1); x2 = np.ascontiguousarray(x2, np.float64).reshape(2, -1)
    M = x1.shape[1]
    X = np.zeros((4, M), np.float64)
    rc = lib().voo_triangulate(_p(P1, C.c_double), _p(P2, C.c_double), _p(x1, C.c_double), _p(x2, C.c_double),
                               M, _p(X, C.c_double))
    assert rc == 0
    return X


def pair(img1, img2, params, K, match_mode=0, ratio=0.75, want_points=True):
    img1 = _u8(img1); img2 = _u8(img2)
    h, w = img1.shape
    K = np.ascontiguousarray(K, np.float64)
    res = PairResult()
    cap = params.nfeatures * 2 + 4096
    X = np.zeros((4, cap), np.float64)
    f = lib().voo_pair
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                  C.c_void_p, C.c_void_p, C.c_int32]
    rc = f(img1.ctypes.data, img2.ctypes.data, h, w, C.addressof(params), K.ctypes.data, match_mode, ratio,
           C.addressof(res), X.ctypes.data if want_points else None, cap)
    out = dict(rc=rc, n_kp1=res.n_kp1, n_kp2=res.n_kp2, n_match=res.n_match, n_inl=res.n_inl_E,
               n_good=res.n_good_pose, R=np.array(res.R).reshape(3, 3), t=np.array(res.t).reshape(3, 1),
               E=np.array(res.E).reshape(3, 3))
    if want_points:
        out["X"] = X[:, :res.n_inl_E].copy()
    return out


def reprojection_sqerr(poses, points, obs_cam, obs_pt, obs_xy, K, threshold=100.0):
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16); points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    oc = np.ascontiguousarray(obs_cam, np.int32); op = np.ascontiguousarray(obs_pt, np.int32)
    xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2); K = np.ascontiguousarray(K, np.float64)
    n = len(oc)
    err = np.zeros(n); keep = np.zeros(n, np.uint8)
    f = lib().voo_reprojection_sqerr
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_double, C.c_void_p, C.c_void_p]
    rc = f(poses.ctypes.data, len(poses), points.ctypes.data, len(points), oc.ctypes.data, op.ctypes.data,
           xy.ctypes.data, n, K.ctypes.data, float(threshold), err.ctypes.data, keep.ctypes.data)
    if rc:
        raise IndexError("observation refers to a missing camera or point")
    return err, keep.astype(bool)


def resize_linear(src, dw, dh):
    """cv2.resize(src, (dw, dh)) with INTER_LINEAR, 8-bit, 1 / 3 / 4 channels (voo_ingest.c)."""
    src = _u8(src)
    sh, sw = src.shape[:2]
    cn = 1 if src.ndim == 2 else src.shape[2]
    dst = np.empty((dh, dw) if src.ndim == 2 else (dh, dw, cn), np.uint8)
    f = lib().voo_resize_linear
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    rc = f(src.ctypes.data, sw, sh, cn, src.strides[0], dst.ctypes.data, dw, dh, dst.strides[0])
    assert rc == 0
    return dst


def resize_area(src, dw, dh):
    """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) for a shrinking 8-bit image (voo_ingest.c)."""
    src = _u8(src)
    sh, sw = src.shape[:2]
    cn = 1 if src.ndim == 2 else src.shape[2]
    dst = np.empty((dh, dw) if src.ndim == 2 else (dh, dw, cn), np.uint8)
    f = lib().voo_resize_area
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    rc = f(src.ctypes.data, sw, sh, cn, src.strides[0], dst.ctypes.data, dw, dh, dst.strides[0])
    if rc == -2:
        raise NotImplementedError("INTER_AREA enlargement is not restated")
    assert rc == 0
    return dst


def sift_pyramid_image(gray, which, octave, layer, n_layers=3, sigma=1.6):
    """Image `layer` of octave `octave` of SIFT's Gaussian (which=0) or DoG (which=1) pyramid (voo_sift.c)."""
    g = _u8(gray)
    h, w = g.shape
    ow = C.c_int32(0); oh = C.c_int32(0)
    f = lib().voo_sift_pyramid_image
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    out = np.empty((2 * h, 2 * w), np.float32)
    rc = f(g.ctypes.data, h, w, n_layers, sigma, which, octave, layer, out.ctypes.data, C.addressof(ow), C.addressof(oh))
    assert rc == 0
    return out.ravel()[:ow.value * oh.value].reshape(oh.value, ow.value).copy()


def sift_detect_and_compute(img, n_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, cap=None, nfeatures=0):
    """cv2.SIFT_create().detectAndCompute(img, None) -> dict(xy, size, angle, response, octave, desc [N, 128] float32)."""
    a = _u8(img)
    h, w = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    f = lib().voo_sift_detect_and_compute
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    n = C.c_int32(0)
    if cap is None:
        rc = f(a.ctypes.data, h, w, cn, a.strides[0], nfeatures, n_layers, contrast_threshold, edge_threshold, sigma, None, None, None, None, None, None, 0, C.addressof(n))
        assert rc == 0
        cap = n.value
    xy = np.zeros((cap, 2), np.float32); size = np.zeros(cap, np.float32); ang = np.zeros(cap, np.float32); resp = np.zeros(cap, np.float32)
    octv = np.zeros(cap, np.int32); desc = np.zeros((cap, 128), np.float32)
    rc = f(a.ctypes.data, h, w, cn, a.strides[0], nfeatures, n_layers, contrast_threshold, edge_threshold, sigma, xy.ctypes.data, size.ctypes.data,
           ang.ctypes.data, resp.ctypes.data, octv.ctypes.data, desc.ctypes.data, cap, C.addressof(n))
    assert rc == 0
    k = min(n.value, cap)
    return dict(xy=xy[:k], size=size[:k], angle=ang[:k], response=resp[:k], octave=octv[:k], desc=desc[:k], n_found=n.value)


# voo_sift_census_t (voo.h), field for field: (name, length); every element is an int32
_SIFT_CENSUS_FIELDS = (("n_keypoints", 1), ("n_octaves", 1), ("n_taps", 1), ("taps", 12),
                       ("cand", 2), ("cand_strip_first", 2), ("cand_strip_last", 2), ("cand_col_first", 2), ("cand_col_last", 2),
                       ("cand_seg_first", 2), ("cand_seg_last", 2), ("cand_row_first", 2), ("cand_row_last", 2),
                       ("ref_kept_steps", 5), ("ref_drop_layer", 1), ("ref_drop_border", 1), ("ref_drop_steps", 1), ("ref_drop_huge", 1),
                       ("ref_drop_contrast", 1), ("ref_drop_det", 1), ("ref_drop_edge", 1), ("ref_singular", 1),
                       ("ori_peaks", 5), ("ori_cut", 1), ("ori_cut_side", 4), ("ori_side_gt64", 1), ("ori_max_side", 1), ("ori_sample_wrap", 1),
                       ("ori_bin_neg", 1), ("ori_bin_ge_n", 1), ("ori_snapped", 1),
                       ("sort_dups", 1), ("sort_x_clamped", 1), ("sort_x_clamped_cols", 1),
                       ("kp_layer", 9), ("desc_r64", 1), ("desc_max_radius", 1), ("desc_clipped", 1), ("desc_clipped_small", 1),
                       ("desc_side_gt128", 1), ("desc_max_side", 1),                        ("desc_cut", 1), ("desc_cut_side", 4), ("desc_max_samples", 1))


def sift_census(img, n_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, nfeatures=0):
    """Which branches of sift_detect_and_compute(img, same parameters) the image takes (voo_sift_census): a dict of ints and
    lists of ints, named as voo_sift_census_t's fields; `taps` holds the n_taps Gaussian tap counts.  Pairs [a, b] of the
    extrema counters are [all octaves, octave 0 alone]."""
    a = _u8(img)
    h, w = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    f = lib().voo_sift_census
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    raw = np.zeros(sum(n for _, n in _SIFT_CENSUS_FIELDS) + 16, np.int32)
    assert lib().voo_sift_census_size() == 4 * (len(raw) - 16)
    raw[-16:] = -12345                                                    # (a struct that outgrew this table would write here)
    rc = f(a.ctypes.data, h, w, cn, a.strides[0], nfeatures, n_layers, contrast_threshold, edge_threshold, sigma, raw.ctypes.data)
    assert rc == 0 and (raw[-16:] == -12345).all()
    out, at = {}, 0
    for name, n in _SIFT_CENSUS_FIELDS:
        out[name] = int(raw[at]) if n == 1 else raw[at:at + n].tolist()
        at += n
    out["taps"] = out["taps"][:out["n_taps"]]
    return out


JPEG_ERRORS = {-1: "corrupt", -2: "unsupported", -3: "output too small"}


def jpeg_info(buf):
    """(h, w, components, sampling of component 0 as h << 4 | v, EXIF orientation or 0) of a JPEG in memory (voo_jpeg.c)."""
    b = np.frombuffer(bytes(buf), np.uint8)
    v = [C.c_int32(0) for _ in range(5)]
    f = lib().voo_jpeg_info
    f.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
    rc = f(b.ctypes.data, len(b), *[C.addressof(x) for x in v])
    if rc == -1:
        raise ValueError("corrupt JPEG header")
    return tuple(x.value for x in v) + (rc == 0,)


def jpeg_decode(buf):
    """cv2.imdecode(buf, cv2.IMREAD_COLOR) / cv2.imread(file) for a baseline JPEG -> [h, w, 3] uint8, B G R (voo_jpeg.c)."""
    b = np.frombuffer(bytes(buf), np.uint8)
    h, w = jpeg_info(buf)[:2]
    out = np.empty((h, w, 3), np.uint8)
    f = lib().voo_jpeg_decode
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]
    rc = f(b.ctypes.data, len(b), out.ctypes.data, out.strides[0], h, w)
    if rc == -2:
        raise NotImplementedError("JPEG layout outside the restated subset")
    if rc != 0:
        raise ValueError("JPEG decode failed: " + JPEG_ERRORS.get(rc, str(rc)))
    return out


def solve_pnp_ransac(obj, img, K, iterations=100, reproj_err=8.0, confidence=0.99, seed=0xFFFFFFFFFFFFFFFF):
    """cv2.solvePnPRansac(obj, img, K, zeros(4)) -> (rc, rvec [3], tvec [3], inlier mask, n_inliers)  (voo_pnp.c)."""
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3); img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64)
    n = len(obj)
    rvec = np.zeros(3); tvec = np.zeros(3); mask = np.zeros(max(n, 1), np.uint8); ninl = C.c_int32(0)
    f = lib().voo_solve_pnp_ransac
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_uint64,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(obj.ctypes.data, img.ctypes.data, n, K.ctypes.data, iterations, reproj_err, confidence, seed,
           rvec.ctypes.data, tvec.ctypes.data, mask.ctypes.data, C.addressof(ninl))
    return rc, rvec, tvec, mask[:n].copy(), ninl.value


def set_pnp_refine(mode):
    """"cv2" (default): solvePnPRansac's final pose as cv2 computes it (DLT / homography start, CvLevMarq);
    "fast": the product's fast mode (the same cost minimised from the best RANSAC model)."""
    f = lib().voo_set_pnp_refine
    f.argtypes = [C.c_int]; f.restype = None
    f({"cv2": 1, "fast": 0}[mode])


def rodrigues(x):
    """cv2.Rodrigues: 3-vector -> 3x3 matrix, 3x3 matrix -> 3-vector."""
    x = np.ascontiguousarray(x, np.float64)
    f = lib().voo_rodrigues
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    if x.size == 9:
        out = np.zeros(3); f(x.ctypes.data, 1, out.ctypes.data); return out
    out = np.zeros((3, 3)); f(x.reshape(3).ctypes.data, 0, out.ctypes.data); return out
