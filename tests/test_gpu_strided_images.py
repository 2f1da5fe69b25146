"""GPU: every image entry point of the C ABI on padded rows, sub-image views and unaligned bases — the layout contract at the top
of include/vo_hip.h.  The Python wrappers compact their inputs, so nothing else in the suite passes a row_stride other than
w * channels, a frame_stride other than h * row_stride, a dst_stride other than dw * channels or a base that is not the start of
an allocation; a kernel that used `w` where it should use `row_stride` would pass all of it.

The calls go through ctx.lib / ctx.handle with the address and the byte strides of numpy views.  The reference is always the CPU
oracle on the compact copy of the view, and the library's own dense call on that copy must give the same bytes; everything is
np.array_equal, no tolerance anywhere.  Every padding byte of a source parent is random, so padding that reaches a result shows;
every destination parent is filled with 0xA5 and every byte outside the destination rows must still be 0xA5 afterwards (a ROI
always has spare parent rows below it, so a library that wrote beyond the rows would fail the assertion, not the process).

Layouts (bytes): dense (control); odd (row_stride = w * cn + 1: every row on another alignment); roi (parent rows of w * cn + 37,
view at row 3, byte 5, two spare rows below); interlaced (every other parent row of w * cn + 8); tail (the last row of the view ends
on the parent's last byte — the contract's edge, run last in each test).  Frame stacks: frame_stride = h * row_stride, a gap of 3
rows + 11 bytes, the contract's minimum (h - 1) * row_stride + w * cn, and 0 for the gray upload.

What this file cannot see is an over-READ: bytes fetched past the last row's last pixel change no result.  That half of the contract
is held by reading: every host-to-device image copy in vo_api.hip takes its length from the one helper image_span(), and the gray
uploads are 2-D copies of the true width.

The whole file (36 cases) takes 1.05 s on an MI355X (measured), the slowest case 0.06 s."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_image

pytestmark = pytest.mark.gpu

LAYOUTS = ("dense", "odd", "roi", "interlaced", "tail")
ORB_KEYS = ("xy", "octave", "response", "angle", "size", "desc")
SENTINEL = 0xA5


# ------------------------------------------------------------------ layouts
def _strided(data, row_stride, frame_stride=None, lead=0, spare=0, seed=0, buf=None):
    """data [F, h, rb] uint8 -> (view, parent): a view of these byte strides onto a 1-D parent of random bytes which begins `lead`
    bytes before the view and ends `spare` bytes after the contract's span (F - 1) * frame_stride + (h - 1) * row_stride + rb."""
    F, h, rb = data.shape
    fs = h * row_stride if frame_stride is None else frame_stride
    assert row_stride >= rb and fs >= (h - 1) * row_stride + rb
    n = lead + (F - 1) * fs + (h - 1) * row_stride + rb + spare
    parent = np.empty(n, np.uint8) if buf is None else buf[:n]
    parent[:] = np.random.default_rng(7000 + seed).integers(0, 256, n, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(parent[lead:], shape=(F, h, rb), strides=(fs, row_stride, 1))
    view[...] = data
    return view, parent


def _layout(name, data, frame_gap=0, seed=0, buf=None):
    """One of LAYOUTS for data [F, h, rb]; frame_gap: extra bytes between the frames."""
    F, h, rb = data.shape
    rs, lead, spare = {"dense": (rb, 0, 0), "odd": (rb + 1, 0, 1), "roi": (rb + 37, 3 * (rb + 37) + 5, 32 + 2 * (rb + 37)),
                       "interlaced": (2 * (rb + 8), 0, rb + 16), "tail": (rb + 13, 2 * (rb + 13) + 13, 0)}[name]
    return _strided(data, rs, h * rs + frame_gap, lead, spare, seed, buf)


def _bytes(img):
    """[h, w(, cn)] or [F, h, w(, cn)] -> [F, h, w * cn]"""
    a = np.ascontiguousarray(img)
    if a.ndim == 2 or (a.ndim == 3 and a.shape[-1] in (3, 4) and a.shape[1] > 4):
        a = a[None]
    return a.reshape(a.shape[0], a.shape[1], -1)


def _compact(view, cn):
    """the compact copy of a [F, h, rb] view, as [F, h, w] or [F, h, w, cn]"""
    a = np.ascontiguousarray(view)
    return a if cn == 1 else a.reshape(a.shape[0], a.shape[1], a.shape[2] // cn, cn)


def _image(seed, h, w, cn):
    """gray random_image, B G R of rolled copies of it, or B G R A with a random alpha plane"""
    g = random_image(seed, h, w)
    if cn == 1:
        return g
    planes = [g, np.roll(g, 3, 0), np.roll(g, 5, 1)]
    if cn == 4:
        planes.append(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8))
    return np.ascontiguousarray(np.stack(planes, -1))


def _gap(row_stride):
    return 3 * row_stride + 11


# ------------------------------------------------------------------ calls
@pytest.fixture(scope="module")
def own_ctx():
    """A context of this file's own for the batched calls (they switch the detector and the batch geometry)."""
    from visual_odometry_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _orb_params(nfeatures=200, nlevels=3):
    from visual_odometry_amd.detector import make_params
    return make_params(nfeatures=nfeatures, nlevels=nlevels)


def _orb_cap(n):
    return n + max(n // 8, 256) + 8


def _orb_single(ctx, v, w, cn, params):
    """vo_orb_detect_and_compute on the [h, rb] view v"""
    from visual_odometry_amd import _lib
    kp = _lib.KeypointBuffers(_orb_cap(params.nfeatures), 32)
    rc = ctx.lib.vo_orb_detect_and_compute(ctx.handle, v.ctypes.data, v.shape[0], w, cn, v.strides[0], C.addressof(params), *kp.args())
    assert rc == 0, (rc, ctx.last_error())
    return kp.result(rc)


def _sift_single(ctx, v, w, cn):
    from visual_odometry_amd import _lib
    kp = _lib.KeypointBuffers(1 << 14, 128, np.float32)
    rc = ctx.lib.vo_sift_detect_and_compute(ctx.handle, v.ctypes.data, v.shape[0], w, cn, v.strides[0], None, *kp.args())
    assert rc == 0, (rc, ctx.last_error())
    return kp.result(rc)


def _slot_features(fe, slot):
    f = fe.features(slot)
    assert not f["truncated"]
    return f


def _same_orb(got, want, what):
    assert len(want["xy"]) > 0, what
    for k in ORB_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def _same_sift(got, want, what):
    assert want["n_found"] > 0 and len(got["xy"]) == want["n_found"], what
    for k in ("xy", "size", "angle", "response", "octave"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["desc"].dtype == np.float32 and np.array_equal(got["desc"], want["desc"]), what


def _front_end(ctx, h, w, frames, detector="orb"):
    from visual_odometry_amd.frontend import FrontEnd
    if detector == "sift":
        return FrontEnd(h, w, max_frames=frames, max_pairs=1, detector="sift", ctx=ctx, kp_cap=4096)
    return FrontEnd(h, w, max_frames=frames, max_pairs=1, nfeatures=200, nlevels=3, ctx=ctx, keypoint_order="cv2")


def _clear_slots(fe, n):
    """zeros into the slots through the dense upload, so that a strided upload that wrote nothing cannot pass on stale data"""
    fe.upload(np.zeros((n, fe.h, fe.w), np.uint8))


# ------------------------------------------------------------------ vo_stage_pyramid: k_gray and the upload paths
@pytest.mark.parametrize("h,w", [(70, 100), (64, 128)])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_stage_pyramid_strided(ctx, oracle, h, w, cn):
    p, po = _orb_params(), oracle.orb_params(nfeatures=200, nlevels=3)
    img = _image(11 + cn, h, w, cn)
    nbytes = int(ctx.lib.vo_packed_pyramid_bytes(h, w, C.addressof(p)))
    gray = img if cn == 1 else oracle.gray(img)
    want = np.concatenate([lv.ravel() for lv in oracle.pyramid(gray, po)])
    assert nbytes == len(want)
    for k, name in enumerate(LAYOUTS):
        v, parent = _layout(name, _bytes(img), seed=k)
        assert np.array_equal(_compact(v, cn)[0], img)
        out = np.zeros(nbytes, np.uint8)
        rc = ctx.lib.vo_stage_pyramid(ctx.handle, v.ctypes.data, h, w, cn, v.strides[1], C.addressof(p), out.ctypes.data)
        assert rc == 0, (name, ctx.last_error())
        assert np.array_equal(out[:h * w].reshape(h, w), gray), name                 # level 0 = oracle.gray(compact)
        assert np.array_equal(out, want), name


# ------------------------------------------------------------------ vo_orb_detect_and_compute
@pytest.mark.parametrize("h,w", [(96, 128), (100, 140)])    # level 0 unpadded (dense gray path) / padded (staging path)
@pytest.mark.parametrize("cn", [1, 3])
def test_orb_detect_strided(ctx, oracle, h, w, cn):
    ctx.set_keypoint_order("cv2")
    p, po = _orb_params(), oracle.orb_params(nfeatures=200, nlevels=3)
    img = _image(21, h, w, cn)
    want = oracle.orb_detect_and_compute(img, po)
    assert len(want["xy"]) >= 100                              # an empty comparison cannot pass
    dense = _orb_single(ctx, _bytes(img)[0], w, cn, p)
    _same_orb(dense, want, "dense")
    for k, name in enumerate(("odd", "roi", "tail")):
        v, parent = _layout(name, _bytes(img), seed=k)
        _same_orb(_orb_single(ctx, v[0], w, cn, p), want, name)


# ------------------------------------------------------------------ vo_sift_detect_and_compute: the unaligned dword loader of the first sweep
@pytest.mark.parametrize("h,w", [(64, 80), (97, 131)])
@pytest.mark.parametrize("cn", [1, 3])
def test_sift_detect_strided(ctx, oracle, h, w, cn):
    img = _image(31, h, w, cn)
    want = oracle.sift_detect_and_compute(img)
    assert want["n_found"] >= 100
    _same_sift(_sift_single(ctx, _bytes(img)[0], w, cn), want, "dense")
    for k, name in enumerate(("odd", "roi", "tail")):
        v, parent = _layout(name, _bytes(img), seed=k)
        _same_sift(_sift_single(ctx, v[0], w, cn), want, name)


# ------------------------------------------------------------------ vo_frames_upload, vo_frames_upload_async
@pytest.mark.parametrize("h,w", [(96, 128), (100, 140)])    # copy path 1 (one strided copy) / path 2 (staging + k_gray) for dense rows
def test_frames_upload_strided(own_ctx, oracle, h, w):
    from visual_odometry_amd import _lib
    c = own_ctx
    fe = _front_end(c, h, w, 3)
    po = oracle.orb_params(nfeatures=200, nlevels=3)
    frames = np.stack([random_image(40 + k, h, w) for k in range(3)])
    want = [oracle.orb_detect_and_compute(f, po) for f in frames]
    assert min(len(x["xy"]) for x in want) >= 100

    def check(what, order=(0, 1, 2)):
        c.check(c.lib.vo_frames_detect(c.handle, 0, 3))
        for s in range(3):
            _same_orb(_slot_features(fe, s), want[order[s]], (what, s))

    fe.upload(frames); check("compact")
    # dense rows with a gap between the frames (paths 1 / 2), padded rows (path 3) with and without a gap, the contract's edge last
    cases = [("dense", _gap(w)), ("odd", 0), ("roi", _gap(w + 37)), ("interlaced", 0), ("tail", _gap(w + 13))]
    for k, (name, gap) in enumerate(cases):
        v, parent = _layout(name, frames, frame_gap=gap, seed=k)
        _clear_slots(fe, 3)
        assert c.lib.vo_frames_upload(c.handle, v.ctypes.data, 3, v.strides[1], v.strides[0], 0) == 0, (name, c.last_error())
        check(name)
    # frame_stride = 0: the three slots all receive frame 0 (dense rows and padded rows)
    for k, name in enumerate(("dense", "roi")):
        v, parent = _layout(name, frames[1:2], seed=10 + k)
        _clear_slots(fe, 3)
        assert c.lib.vo_frames_upload(c.handle, v.ctypes.data, 3, v.strides[1], 0, 0) == 0, (name, c.last_error())
        check("frame_stride 0 " + name, (1, 1, 1))
    # the enqueue-only form from page-locked memory, padded rows and a frame gap; valid after vo_sync
    pinned = _lib.PinnedArray((4 * (h + 8) * (w + 64),), np.uint8)
    v, parent = _layout("roi", frames[::-1], frame_gap=_gap(w + 37), seed=20, buf=pinned.array)
    _clear_slots(fe, 3)
    assert c.lib.vo_frames_upload_async(c.handle, v.ctypes.data, 3, v.strides[1], v.strides[0], 0) == 0, c.last_error()
    assert c.lib.vo_sync(c.handle) == 0
    check("async pinned roi", (2, 1, 0))
    v = parent = None


# ------------------------------------------------------------------ vo_frames_upload_color (k_gray, k_gray_plain) and the SIFT slots' gray upload
def _stack_cases(h, rb):
    """(name, layout, frame gap): ROI views back to back, with a gap, and at the contract's minimum frame_stride (negative gap)"""
    rs = rb + 37
    return [("roi", "roi", 0), ("roi + gap", "roi", _gap(rs)), ("dense + gap", "dense", _gap(rb)), ("roi, minimum frame_stride", "roi", rb - rs)]


@pytest.mark.parametrize("cn", [3, 4])
def test_frames_upload_color_strided_orb(own_ctx, oracle, cn):
    c = own_ctx
    h, w = 100, 140
    fe = _front_end(c, h, w, 2)
    po = oracle.orb_params(nfeatures=200, nlevels=3)
    frames = np.stack([_image(50 + k, h, w, cn) for k in range(2)])
    want = [oracle.orb_detect_and_compute(f, po) for f in frames]
    assert min(len(x["xy"]) for x in want) >= 100
    fe.upload(frames); fe.detect(0, 2)
    for s in range(2):
        _same_orb(_slot_features(fe, s), want[s], ("compact", s))
    for k, (what, name, gap) in enumerate(_stack_cases(h, w * cn)):
        v, parent = _layout(name, _bytes(frames), frame_gap=gap, seed=k)
        assert np.array_equal(_compact(v, cn), frames)
        _clear_slots(fe, 2)
        assert c.lib.vo_frames_upload_color(c.handle, v.ctypes.data, 2, cn, v.strides[1], v.strides[0], 0) == 0, (what, c.last_error())
        fe.detect(0, 2)
        for s in range(2):
            _same_orb(_slot_features(fe, s), want[s], (what, s))


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_frames_upload_strided_sift(own_ctx, oracle, cn):
    """The SIFT front end at 64x80: k_gray_plain from strided B G R (A) frames; for gray frames both branches of
    sift_frames_upload_enqueue (dense rows with a frame gap: one strided copy; padded rows: a 2-D copy per frame)."""
    c = own_ctx
    h, w = 64, 80
    fe = _front_end(c, h, w, 2, detector="sift")
    frames = np.stack([_image(60 + k, h, w, cn) for k in range(2)])
    want = [oracle.sift_detect_and_compute(f) for f in frames]
    assert min(x["n_found"] for x in want) >= 100
    fe.upload(frames); fe.detect(0, 2)
    for s in range(2):
        _same_sift(_slot_features(fe, s), want[s], ("compact", s))
    cases = _stack_cases(h, w * cn) if cn > 1 else [("dense + gap", "dense", _gap(w)), ("roi + gap", "roi", _gap(w + 37)), ("odd", "odd", 0), ("tail", "tail", 0)]
    for k, (what, name, gap) in enumerate(cases):
        v, parent = _layout(name, _bytes(frames), frame_gap=gap, seed=k)
        _clear_slots(fe, 2)
        if cn == 1:
            rc = c.lib.vo_frames_upload(c.handle, v.ctypes.data, 2, v.strides[1], v.strides[0], 0)
        else:
            rc = c.lib.vo_frames_upload_color(c.handle, v.ctypes.data, 2, cn, v.strides[1], v.strides[0], 0)
        assert rc == 0, (what, c.last_error())
        fe.detect(0, 2)
        for s in range(2):
            _same_sift(_slot_features(fe, s), want[s], (what, s))


# ------------------------------------------------------------------ vo_resize_linear, vo_resize_area
def _destinations(dh, rb):
    """(name, parent [rows, width] full of 0xA5, row0, col0): dense; a ROI with dst_stride = rb + 7 (the rows' alignment changes from
    row to row); a ROI with dst_stride a multiple of 4 whose base is 1 byte off a dword.  Every ROI has two spare parent rows below."""
    out = [("dense", np.full((dh, rb), SENTINEL, np.uint8), 0, 0)]
    out.append(("stride + 7", np.full((dh + 4, rb + 7), SENTINEL, np.uint8), 2, 3))
    width = (rb + 8 + 3) // 4 * 4
    par = np.full((dh + 4, width), SENTINEL, np.uint8)
    col = (1 - (par.ctypes.data + 2 * width)) % 4
    col += 4 if col == 0 else 0
    assert (par.ctypes.data + 2 * width + col) % 4 == 1 and col + rb <= width and width % 4 == 0
    out.append(("dword + 1", par, 2, col))
    return out


def _resize_strided(ctx, fn_name, oracle_fn, shape, dw, dh, seed):
    h, w = shape[:2]
    cn = 1 if len(shape) == 2 else shape[2]
    img = _image(seed, h, w, cn)
    want = oracle_fn(img, dw, dh).reshape(dh, dw * cn)
    fn = getattr(ctx.lib, fn_name)
    for k, name in enumerate(LAYOUTS):
        v, sparent = _layout(name, _bytes(img), seed=k)
        for dname, par, r0, c0 in _destinations(dh, dw * cn):
            roi = par[r0:r0 + dh, c0:c0 + dw * cn]
            rc = fn(ctx.handle, v.ctypes.data, h, w, cn, v.strides[1], roi.ctypes.data, dh, dw, roi.strides[0])
            assert rc == 0, (name, dname, ctx.last_error())
            assert np.array_equal(roi, want), (name, dname)
            rest = par.copy()
            rest[r0:r0 + dh, c0:c0 + dw * cn] = SENTINEL
            assert (rest == SENTINEL).all(), (name, dname, "bytes outside the destination rows were written")


@pytest.mark.parametrize("shape,dw,dh", [((97, 131), 64, 48),          # one channel, fractional
                                         ((60, 80, 3), 40, 30),        # the exact 2:1 branch
                                         ((50, 70, 3), 33, 21),        # k_resize_linear_bgr4, a last group of fewer than 4 pixels
                                         ((50, 70, 4), 140, 100)])     # enlarging
def test_resize_linear_strided(ctx, oracle, shape, dw, dh):
    _resize_strided(ctx, "vo_resize_linear", oracle.resize_linear, shape, dw, dh, 70)


@pytest.mark.parametrize("shape,dw,dh", [((216, 384, 3), 128, 72),     # 3 x 3 blocks
                                         ((60, 80, 3), 40, 30),        # 2 x 2
                                         ((97, 131), 64, 48),          # fractional
                                         ((60, 80, 4), 79, 59)])       # fractional
def test_resize_area_strided(ctx, oracle, shape, dw, dh):
    _resize_strided(ctx, "vo_resize_area", oracle.resize_area, shape, dw, dh, 80)


# ------------------------------------------------------------------ vo_frames_ingest
@pytest.mark.parametrize("sh,sw,cn,name,resized", [(160, 200, 3, "roi", True),      # the 2:1 branch
                                                   (123, 187, 3, "odd", True),      # generic (k_resize_linear_bgr4)
                                                   (123, 187, 1, "roi", True),      # generic, gray
                                                   (123, 187, 1, "tail", False),    # gray straight into the slots
                                                   (80, 100, 3, "roi", False),      # gray conversion straight from the strided source
                                                   (80, 100, 3, "roi", True)])      # the identity resize returns the source pixels
def test_frames_ingest_strided(own_ctx, oracle, sh, sw, cn, name, resized):
    c = own_ctx
    h, w = 80, 100
    fe = _front_end(c, h, w, 2)
    po = oracle.orb_params(nfeatures=200, nlevels=3)
    frames = np.stack([_image(90 + k, sh, sw, cn) for k in range(2)])
    small = [oracle.resize_linear(f, w, h) for f in frames]
    if (sh, sw) == (h, w):
        assert np.array_equal(small[0], frames[0])
    want = [oracle.orb_detect_and_compute(f, po) for f in small]
    assert min(len(x["xy"]) for x in want) >= 30
    ref_out = fe.ingest(frames, want_resized=True)                      # the library's dense call
    assert all(np.array_equal(ref_out[s], small[s]) for s in range(2))
    rs = {"roi": sw * cn + 37, "odd": sw * cn + 1, "tail": sw * cn + 13}[name]
    v, parent = _layout(name, _bytes(frames), frame_gap=_gap(rs), seed=sh)
    _clear_slots(fe, 2)
    out = np.full((2, h, w * cn), SENTINEL, np.uint8) if resized else None
    rc = c.lib.vo_frames_ingest(c.handle, v.ctypes.data, 2, sh, sw, cn, v.strides[1], v.strides[0], 0, None if out is None else out.ctypes.data)
    assert rc == 0, c.last_error()
    if resized:
        for s in range(2):
            assert np.array_equal(out[s], small[s].reshape(h, w * cn)), s
    fe.detect(0, 2)
    for s in range(2):
        _same_orb(_slot_features(fe, s), want[s], s)


# ------------------------------------------------------------------ rejections
def test_strides_below_the_minimum_are_refused(own_ctx, oracle):
    from visual_odometry_amd import _lib
    c = own_ctx
    lib, hnd, INV = c.lib, c.handle, _lib.VO_ERR_INVALID
    h, w = 64, 80
    p = _orb_params()
    n = C.c_int32(0)
    out = np.zeros(4 * h * w * 4, np.uint8)
    for cn in (1, 3, 4):
        img = np.zeros((2, h + 1, w * cn), np.uint8)               # a spare row and frame: even an accepted call stays inside
        bad = w * cn - 1
        kp = _lib.KeypointBuffers(600, 32)
        assert lib.vo_orb_detect_and_compute(hnd, img.ctypes.data, h, w, cn, bad, C.addressof(p), *kp.args()) == INV
        for fn in (lib.vo_stage_pyramid, lib.vo_stage_fast_scores, lib.vo_stage_blur):
            assert fn(hnd, img.ctypes.data, h, w, cn, bad, C.addressof(p), out.ctypes.data) == INV
        ks = _lib.KeypointBuffers(16, 128, np.float32)
        assert lib.vo_sift_detect_and_compute(hnd, img.ctypes.data, h, w, cn, bad, None, *ks.args()) == INV
        for fn in (lib.vo_resize_linear, lib.vo_resize_area):
            assert fn(hnd, img.ctypes.data, h, w, cn, bad, out.ctypes.data, h // 2, w // 2, w // 2 * cn) == INV
            assert fn(hnd, img.ctypes.data, h, w, cn, w * cn, out.ctypes.data, h // 2, w // 2, w // 2 * cn - 1) == INV
            assert fn(hnd, img.ctypes.data, h, w, cn, w * cn, out.ctypes.data, h // 2, w // 2, w // 2 * cn) == 0
    for detector in ("orb", "sift"):
        fe = _front_end(c, h, w, 2, detector=detector)
        for cn in (1, 3, 4):
            rb = w * cn
            rs = rb + 5
            lo = (h - 1) * rs + rb                                  # the minimum frame_stride of the contract
            img = np.zeros((2 * h + 2) * rs, np.uint8)
            if cn == 1:
                assert lib.vo_frames_upload(hnd, img.ctypes.data, 2, rb - 1, h * rb, 0) == INV
                assert lib.vo_frames_upload_async(hnd, img.ctypes.data, 2, rb - 1, h * rb, 0) == INV
            else:
                assert lib.vo_frames_upload_color(hnd, img.ctypes.data, 2, cn, rb - 1, h * rb, 0) == INV
                assert lib.vo_frames_upload_color(hnd, img.ctypes.data, 2, cn, rs, lo - 1, 0) == INV
                assert lib.vo_frames_upload_color(hnd, img.ctypes.data, 2, cn, rs, lo, 0) == 0, c.last_error()
            assert lib.vo_frames_ingest(hnd, img.ctypes.data, 2, h, w, cn, rb - 1, h * rb, 0, None) == INV
            assert lib.vo_frames_ingest(hnd, img.ctypes.data, 2, h, w, cn, rs, lo - 1, 0, None) == INV
            assert lib.vo_frames_ingest(hnd, img.ctypes.data, 2, h, w, cn, rs, lo, 0, None) == 0, c.last_error()
