"""Batched, device-resident front end: frames live in HBM, detection + matching + E-RANSAC + pose (+ DLT) run
batch-major through the C ABI with no host round trip between stages.  This is the throughput path
bench.py measures; the per-pair order is that of src/visual_slam.py:294-298.  detector="orb" is the north-star
instantiation (ORB + Hamming, src/image_and_keypoints.py:8-9); detector="sift" is the configuration the reference runs
live (cv2.SIFT_create() + BFMatcher(NORM_L2, crossCheck=True), src/visual_slam.py:17,19)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .detector import make_params
from .geometry import OPENCV_RNG_SEED

MATCH_CROSSCHECK, MATCH_RATIO, MATCH_CROSSCHECK_LEGACY, MATCH_NEAREST = 0, 1, 2, 3


class FrontEnd:
    def __init__(self, height, width, max_frames, max_pairs, nfeatures=500, nlevels=8, device=0, ctx=None,
                 keypoint_order="cv2", detector="orb", kp_cap=0, **det_kw):
        self.ctx = ctx or _lib.Context(device)
        self.h, self.w = int(height), int(width)
        self.max_frames, self.max_pairs = int(max_frames), int(max_pairs)
        self.detector = detector
        c = self.ctx
        if detector == "sift":
            # cv2.SIFT_create(nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6); kp_cap: keypoints
            # kept per frame (0 = a default from the frame size; more are truncated and flagged)
            self.params = _lib.SiftParams(0, int(det_kw.pop("nOctaveLayers", 3)), float(det_kw.pop("contrastThreshold", 0.04)),
                                          float(det_kw.pop("edgeThreshold", 10.0)), float(det_kw.pop("sigma", 1.6)))
            if det_kw:
                raise TypeError(f"unknown SIFT arguments {sorted(det_kw)}")
            rc = c.lib.vo_batch_configure_sift(c.handle, self.h, self.w, C.addressof(self.params), self.max_frames, self.max_pairs, int(kp_cap))
            if rc == _lib.VO_ERR_UNSUPPORTED:
                raise NotImplementedError(c.last_error())
            c.check(rc)
        elif detector == "orb":
            self.ctx.set_keypoint_order(keypoint_order)       # 'cv2': keypoint / match indices as cv2.ORB + BFMatcher number them
            self.params = make_params(nfeatures=nfeatures, nlevels=nlevels, **det_kw)
            c.check(c.lib.vo_batch_configure(c.handle, self.h, self.w, C.addressof(self.params), self.max_frames,
                                             self.max_pairs))
        else:
            raise ValueError("detector must be 'orb' or 'sift'")
        self.kp_cap = int(c.lib.vo_batch_kp_capacity(c.handle))
        self._res = _lib.PinnedArray((self.max_pairs,), _lib.PAIR_RESULT_DTYPE)      # page-locked result buffers,
        self._X = None                                                                # reused by every run_pairs call

    def pinned_frames(self, count):
        """Page-locked [count, H, W] uint8 staging array for upload(..., wait=False) (kept alive by the caller)."""
        return _lib.PinnedArray((int(count), self.h, self.w), np.uint8)

    def upload(self, frames, first_slot=0, wait=True):
        """frames: [F, H, W] gray or [F, H, W, 3|4] BGR(A) uint8 (BGR is converted on the device, as ORB does).
        wait=False (gray only): enqueue the copy; `frames` should come from pinned_frames() and must not change
        before the next wait()."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim == 2 or (f.ndim == 3 and f.shape[-1] in (3, 4) and f.shape[:2] == (self.h, self.w)):
            f = f[None]
        if f.ndim not in (3, 4) or f.shape[1:3] != (self.h, self.w):
            raise ValueError(f"frames must be [F, {self.h}, {self.w}] or [F, {self.h}, {self.w}, 3|4] uint8")
        c = self.ctx
        if f.ndim == 3 and not wait:
            self._keep_frames = f
            c.check(c.lib.vo_frames_upload_async(c.handle, f.ctypes.data, f.shape[0], f.strides[1], f.strides[0], int(first_slot)))
        elif f.ndim == 3:
            c.check(c.lib.vo_frames_upload(c.handle, f.ctypes.data, f.shape[0], f.strides[1], f.strides[0], int(first_slot)))
        else:
            c.check(c.lib.vo_frames_upload_color(c.handle, f.ctypes.data, f.shape[0], f.shape[3], f.strides[1], f.strides[0],
                                                 int(first_slot)))

    def ingest(self, frames, first_slot=0, want_resized=False):
        """Full-resolution frames [F, H0, W0] or [F, H0, W0, 3|4] uint8 (as cv2.imread returns them): resized on the
        device to this front end's (w, h) with cv2.resize's default INTER_LINEAR (visual_slam.py:346-352), converted
        to gray as ORB does, stored as level 0 of the slots.  Returns the resized frames if want_resized."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim == 2 or (f.ndim == 3 and f.shape[-1] in (3, 4) and f.shape[1] > 4):
            f = f[None]
        if f.ndim not in (3, 4):
            raise ValueError("frames must be [F, H, W] or [F, H, W, 3|4] uint8")
        cn = 1 if f.ndim == 3 else f.shape[3]
        out = None
        if want_resized:
            out = np.empty((f.shape[0], self.h, self.w) if f.ndim == 3 else (f.shape[0], self.h, self.w, cn), np.uint8)
        c = self.ctx
        c.check(c.lib.vo_frames_ingest(c.handle, f.ctypes.data, f.shape[0], f.shape[1], f.shape[2], cn, f.strides[1],
                                       f.strides[0], int(first_slot), _lib.ptr(out)))
        return out

    def ingest_jpeg(self, buffers, first_slot=0, want_resized=False):
        """buffers: a sequence of bytes-like objects or an ingest.PackedFiles (files packed in page-locked memory).
        The reference's whole ingest (visual_slam.py:346-352) for JPEG files of one size: cv2.imread -> cv2.resize to this
        front end's (w, h) -> gray into level 0 of the slots, all on the device (only the compressed bytes cross PCIe).
        Returns the resized B G R frames if want_resized (the reference keeps them as Frame.image)."""
        from .ingest import _packed
        blob, offs, _keep = _packed(buffers)                 # a PackedFiles (page-locked) goes over PCIe by DMA as it is
        n = len(offs) - 1
        out = np.empty((n, self.h, self.w, 3), np.uint8) if want_resized else None
        c = self.ctx
        rc = c.lib.vo_frames_ingest_jpeg(c.handle, blob.ctypes.data, offs.ctypes.data, n, int(first_slot), _lib.ptr(out))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return out

    def detect(self, first_slot, count, wait=True, after=None):
        """ORB detect + describe of `count` resident slots. wait=False only enqueues the work on the ctx stream;
        the next run_pairs (same stream) is ordered after it.  after=<another FrontEnd on this GPU>: start only when
        that one's latest asynchronous detection has finished (keeps two alternating contexts out of phase)."""
        c = self.ctx
        if after is not None and after is not self:
            c.check(c.lib.vo_detect_after(c.handle, after.ctx.handle))
        fn = c.lib.vo_frames_detect if wait else c.lib.vo_frames_detect_async
        self._warn_capacity(c.check(fn(c.handle, int(first_slot), int(count))))

    def undistort(self, first_slot, count, K, dist):
        """A camera with a real lens (vo_frames_undistort): rewrites the keypoint positions of `count` detected slots in place with
        cv2.undistortPoints(xy, K, dist, None, K) — five iterations, float64 arithmetic, one rounding back to float32 — on the
        device, ordered behind detect(wait=False) and before the next run_pairs.  Everything downstream (run_pairs, localize_chain,
        the slam_* calls) reads positions from there only and so runs on ideal pixels; features(slot)["xy"] returns them too.
        The detected positions are not kept: a caller who wants them reads features(slot)["xy"] BEFORE this call.
        K: the camera matrix of the frames as they sit in the slots (after ingest's resize); dist: 4, 5 or 8 coefficients
        (k1 k2 p1 p2 [k3 [k4 k5 k6]]), which a resize leaves unchanged.  A slot can be undistorted once per detection: a second
        call on it raises VoError (VO_ERR_INVALID) until the slot is uploaded to, detected or staged again."""
        from .geometry import dist_coeffs
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        d = dist_coeffs(dist)
        c = self.ctx
        rc = c.lib.vo_frames_undistort(c.handle, int(first_slot), int(count), K.ctypes.data, d.ctypes.data, len(d))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)

    def features(self, slot):
        """Keypoints and descriptors of a detected slot.  ORB: desc [n, 32] uint8; SIFT: desc [n, 128] float32 (the integer bin
        values 0..255 cv2 returns as floats).  After undistort() on the slot, xy holds the ideal (undistorted) pixels."""
        sift = self.detector == "sift"
        kp = _lib.KeypointBuffers(self.kp_cap, 128 if sift else 32)
        c = self.ctx
        fn = c.lib.vo_frame_features_sift if sift else c.lib.vo_frame_features
        rc = c.check(fn(c.handle, int(slot), *kp.args()))
        return kp.result(rc, np.float32 if sift else None)

    def set_sift_rows(self, slot, rows, xy=None):
        """SIFT mode's parity seam (vo_stage_sift_rows): rows [n, 128] uint8 become the slot's descriptors as if they had been
        detected (desc, the matcher's operand image and norms, count, flags); xy [n, 2] float32 pixel positions, zeros when None.
        Operand rows past n keep what the slot held before."""
        if self.detector != "sift":
            raise ValueError("set_sift_rows needs detector='sift'")
        r = np.asarray(rows)
        if r.dtype != np.uint8 or r.ndim != 2 or r.shape[1] != 128:
            raise ValueError("rows must be [n, 128] uint8")
        r = np.ascontiguousarray(r)
        p = None
        if xy is not None:
            p = np.ascontiguousarray(xy, dtype=np.float32)
            if p.shape != (len(r), 2):
                raise ValueError("xy must be [n, 2]")
        c = self.ctx
        c.check(c.lib.vo_stage_sift_rows(c.handle, int(slot), r.ctypes.data, len(r), _lib.ptr(p)))

    def set_orb_rows(self, slot, rows, xy=None):
        """ORB mode's parity seam (vo_stage_orb_rows): rows [n, 32] uint8 become the slot's descriptors as a detection of that slot
        would leave them (desc, count, flags, the operand image of the matcher kernel selected now); xy [n, 2] float32 pixel
        positions, zeros when None.  Descriptor rows past n keep what the slot held before."""
        if self.detector != "orb":
            raise ValueError("set_orb_rows needs detector='orb'")
        r = np.asarray(rows)
        if r.dtype != np.uint8 or r.ndim != 2 or r.shape[1] != 32:
            raise ValueError("rows must be [n, 32] uint8")
        r = np.ascontiguousarray(r)
        p = None
        if xy is not None:
            p = np.ascontiguousarray(xy, dtype=np.float32)
            if p.shape != (len(r), 2):
                raise ValueError("xy must be [n, 2]")
        c = self.ctx
        c.check(c.lib.vo_stage_orb_rows(c.handle, int(slot), r.ctypes.data, len(r), _lib.ptr(p)))

    def make_opts(self, match_mode=MATCH_CROSSCHECK, ratio=0.75, prob=0.99, thresh=1.0, max_iters=1000,
                  seed=OPENCV_RNG_SEED, dist_thresh=50.0, want_points=False):
        return _lib.PairOpts(int(match_mode), float(ratio), float(prob), float(thresh), int(max_iters), int(seed),
                             float(dist_thresh), int(bool(want_points)))

    def run_pairs(self, pair_slots, K, opts=None, want_points=False, wait=True):
        """pair_slots: [B, 2] int32 of detected slots. Returns (results structured array [B], X or None) — views of
        reused page-locked buffers (copy them if they must outlive the next call).  wait=False only enqueues the
        work; the returned views are valid after self.wait()."""
        ps = np.ascontiguousarray(pair_slots, dtype=np.int32).reshape(-1, 2)
        B = len(ps)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        opts = opts or self.make_opts(want_points=want_points)
        if B > self.max_pairs:
            raise ValueError(f"{B} pairs > max_pairs={self.max_pairs}")
        res = self._res.array[:B]
        X = None
        if opts.want_points:
            if self._X is None:
                self._X = _lib.PinnedArray((self.max_pairs, 4, self.kp_cap), np.float64)
            X = self._X.array[:B]
        c = self.ctx
        fn = c.lib.vo_pairs_run if wait else c.lib.vo_pairs_run_async
        self._keep = (ps, K, opts)                  # keep the argument buffers alive until the work has been consumed
        self._warn_capacity(c.check(fn(c.handle, ps.ctypes.data, B, K.ctypes.data, C.addressof(opts), res.ctypes.data, _lib.ptr(X), self.kp_cap)))
        self._last_pairs = B
        return res, X

    def _warn_capacity(self, rc):
        if rc == _lib.VO_WARN_CAPACITY:
            import warnings
            warnings.warn("a frame's keypoint list hit its capacity and was cut (SIFT: in x order, the right edge of the image first): "
                          "raise kp_cap; features(slot)['truncated'] names the slots", RuntimeWarning, stacklevel=3)

    def wait(self):
        c = self.ctx
        c.check(c.lib.vo_sync(c.handle))

    def localize_chain(self, n_pairs, K, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED, max_point_norm=50.0):
        """The step after the pair path on resident data (vo_tracks_pnp_batch; src/visual_slam.py:183-266 without the bundle
        adjustment): the `n_pairs` pairs of the latest run_pairs(..., want_points=True) — a chain (f0, f1), (f1, f2), ... — are
        walked in order: feature tracks -> map / image coordinates -> solvePnPRansac -> camera -> new map points.
        Returns dict(poses [n_pairs + 1, 3, 4] world -> camera, n_corr, n_inl, status, n_map, each [n_pairs])."""
        B = int(n_pairs)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        poses = np.zeros((B + 1, 12)); nc = np.zeros(B, np.int32); ni = np.zeros(B, np.int32); st = np.zeros(B, np.int32); nm = np.zeros(B, np.int32)
        c = self.ctx
        c.check(c.lib.vo_tracks_pnp_batch(c.handle, B, K.ctypes.data, int(iterations), float(reproj_err), float(confidence), int(seed),
                                          float(max_point_norm), poses.ctypes.data, nc.ctypes.data, ni.ctypes.data, st.ctypes.data, nm.ctypes.data))
        return dict(poses=poses.reshape(B + 1, 3, 4), n_corr=nc, n_inl=ni, status=st, n_map=nm)

    def slam_chain(self, n_pairs, K, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED, max_point_norm=50.0,
                   ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18, snapshot=None, restart=False):
        """The reference's complete per-frame map step on resident data (vo_slam_chain; src/visual_slam.py:190-266 and :311):
        localize_chain's walk with the Observation list, freeze_nonlast_cameras, Map.optimize_map, the reprojection filter and
        limit_number_of_camera_in_map after every pair, on a map that stays on the device.  snapshot=(pair, stage): keep a copy
        of the map as it was at that pair after stage 1 add_information_to_map, 2 bundle adjustment, 3 filter, 4 camera limit
        (slam_map(1)).  Returns dict(poses_pnp, poses [n_pairs + 1, 3, 4], n_corr, n_inl, status, n_pts, n_obs, n_cam,
        ba_iterations, ba_trials [n_pairs], chi2 [n_pairs, 2]).  restart=True: slam_chains(restart=True) on this one chain."""
        B = int(n_pairs)
        if restart:
            return self.slam_chains([B], K, iterations, reproj_err, confidence, seed, max_point_norm, ba_iterations, huber_delta, free_cameras,
                                    filter_threshold, max_cameras, None if snapshot is None else (0, snapshot[0], snapshot[1]), restart=True)[0]
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        sp, ss = (-1, 0) if snapshot is None else (int(snapshot[0]), int(snapshot[1]))
        opts = _lib.SlamOpts(int(iterations), float(reproj_err), float(confidence), int(seed), float(max_point_norm), int(ba_iterations),
                             float(huber_delta), int(free_cameras), float(filter_threshold), int(max_cameras), sp, ss)
        pp = np.zeros((B + 1, 12)); pl = np.zeros((B + 1, 12)); chi2 = np.zeros((B, 2))
        i32 = {k: np.zeros(B, np.int32) for k in ("n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")}
        c = self.ctx
        c.check(c.lib.vo_slam_chain(c.handle, B, K.ctypes.data, C.addressof(opts), pp.ctypes.data, pl.ctypes.data, i32["n_corr"].ctypes.data,
                                    i32["n_inl"].ctypes.data, i32["status"].ctypes.data, i32["n_pts"].ctypes.data, i32["n_obs"].ctypes.data,
                                    i32["n_cam"].ctypes.data, chi2.ctypes.data, i32["ba_iterations"].ctypes.data, i32["ba_trials"].ctypes.data))
        return dict(poses_pnp=pp.reshape(B + 1, 3, 4), poses=pl.reshape(B + 1, 3, 4), chi2=chi2, **i32)

    def slam_stream(self, n_pairs, K, resume=False, total_pairs=None, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED,
                    max_point_norm=50.0, ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18, snapshot=None):
        """slam_chain on a map that outlives the call (vo_slam_stream): resume=False starts a stream with the `n_pairs` pairs of the
        latest run_pairs(..., want_points=True) and computes what slam_chain computes; total_pairs (default n_pairs) is how many
        pairs the whole stream may reach.  Then, as often as needed: upload and detect the next frames into any slots but the one
        of the stream's last frame, run_pairs on a chain that starts at that slot, slam_stream(..., resume=True) with the same K and
        options.  The calls together compute what one slam_chain on the whole flight computes, byte for byte.
        Returns slam_chain's dict (in a resumed call poses_pnp / poses row 0 is the stream's last frame of the call before, and
        snapshot=(pair, stage) counts along the call) plus carried_frame [n] and carried_poses [n, 3, 4]: the cameras the map held
        at the start of a resumed call beside that frame, by their index along the whole stream, as the map last held them
        during this call.  slam_map()'s cam_frame and pt_feature[:, 0] count along the whole stream.  A pair that cannot be localised
        ends the stream; slam_stream_restart is the stream that starts a new map instead."""
        return self._slam_stream(False, n_pairs, K, resume, total_pairs, iterations, reproj_err, confidence, seed, max_point_norm, ba_iterations,
                                 huber_delta, free_cameras, filter_threshold, max_cameras, snapshot)

    def slam_stream_restart(self, n_pairs, K, resume=False, total_pairs=None, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED,
                            max_point_norm=50.0, ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18, snapshot=None):
        """slam_stream on a stream that survives a lost frame (vo_slam_stream_restart): slam_chain(restart=True)'s rules on a map
        that outlives the call.  A pair that failed in run_pairs keeps its status and leaves the stream lost; a lost stream, or one
        whose solvePnPRansac finds no camera, starts a new map from the next usable pair — in this call or a later one.  Restart is
        a property of the stream: one begun here is continued here (resume=True), one begun by slam_stream there.  The calls
        together compute what slam_chain(restart=True) computes on the whole flight, byte for byte (join_stream).
        Returns slam_stream's dict plus segment, cause [n_pairs] (segments count along the whole stream; cause may name a pair of an
        earlier call) and seg_poses_pnp, seg_poses [n_pairs, 3, 4]: at a pair of this call that starts a segment, its first camera
        as it entered the map and as the map last held it during this call.  After a call that ended lost the stream's last frame
        is not in the map and carried_frame names all of the map's cameras."""
        return self._slam_stream(True, n_pairs, K, resume, total_pairs, iterations, reproj_err, confidence, seed, max_point_norm, ba_iterations,
                                 huber_delta, free_cameras, filter_threshold, max_cameras, snapshot)

    def _slam_stream(self, restart, n_pairs, K, resume, total_pairs, iterations, reproj_err, confidence, seed, max_point_norm, ba_iterations,
                     huber_delta, free_cameras, filter_threshold, max_cameras, snapshot):
        B = int(n_pairs)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        sp, ss = (-1, 0) if snapshot is None else (int(snapshot[0]), int(snapshot[1]))
        opts = _lib.SlamOpts(int(iterations), float(reproj_err), float(confidence), int(seed), float(max_point_norm), int(ba_iterations),
                             float(huber_delta), int(free_cameras), float(filter_threshold), int(max_cameras), sp, ss)
        pp = np.zeros((B + 1, 12)); pl = np.zeros((B + 1, 12)); chi2 = np.zeros((B, 2))
        i32 = {k: np.zeros(B, np.int32) for k in ("n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")}
        rows = max(int(max_cameras), 1)
        nc = C.c_int32(0); cf = np.zeros(rows, np.int32); cp = np.zeros((rows, 12))
        c = self.ctx
        args = [c.handle, int(bool(resume)), B if total_pairs is None else int(total_pairs), B, K.ctypes.data, C.addressof(opts),
                pp.ctypes.data, pl.ctypes.data, i32["n_corr"].ctypes.data, i32["n_inl"].ctypes.data, i32["status"].ctypes.data,
                i32["n_pts"].ctypes.data, i32["n_obs"].ctypes.data, i32["n_cam"].ctypes.data, chi2.ctypes.data,
                i32["ba_iterations"].ctypes.data, i32["ba_trials"].ctypes.data, C.addressof(nc), cf.ctypes.data, cp.ctypes.data]
        seg = {}
        if restart:
            seg = dict(segment=np.zeros(B, np.int32), cause=np.zeros(B, np.int32), seg_poses_pnp=np.zeros((B, 12)), seg_poses=np.zeros((B, 12)))
            c.check(c.lib.vo_slam_stream_restart(*args, *[seg[k].ctypes.data for k in ("segment", "cause", "seg_poses_pnp", "seg_poses")]))
            seg["seg_poses_pnp"] = seg["seg_poses_pnp"].reshape(B, 3, 4); seg["seg_poses"] = seg["seg_poses"].reshape(B, 3, 4)
        else:
            c.check(c.lib.vo_slam_stream(*args))
        n = nc.value
        return dict(poses_pnp=pp.reshape(B + 1, 3, 4), poses=pl.reshape(B + 1, 3, 4), chi2=chi2, carried_frame=cf[:n].copy(),
                    carried_poses=cp[:n].reshape(n, 3, 4).copy(), **i32, **seg)

    def slam_chains(self, seq_lengths, K, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED, max_point_norm=50.0,
                    ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18, snapshot=None, restart=False):
        """slam_chain for several independent sequences in one call (vo_slam_chains), one workgroup per sequence and kernel: the
        pairs of the latest run_pairs(..., want_points=True) are sequence 0's seq_lengths[0] pairs, then sequence 1's, ...; every
        sequence is a chain of its own and no frame slot belongs to two of them (a frame two sequences share is uploaded into
        two slots).  snapshot=(seq, pair, stage), the pair counted along that sequence (slam_map(1, seq=seq)).  Returns a list of
        len(seq_lengths) dicts, each what slam_chain returns for that sequence alone: a pair that cannot be localised ends its
        own sequence only.
        restart=True (vo_slam_chains_restart): a sequence that loses tracking — a pair that failed in run_pairs, or a solvePnPRansac
        that finds no camera — starts a new map from the next usable pair and goes on, on the device (initialize_map's
        self.map.clean(), src/visual_slam.py:43-45).  A failed pair keeps its own status and none gets VO_ERR_NOT_CONFIGURED.  Every
        dict then also has segment [n_pairs] (index of the pair's segment, -1: in none), cause [n_pairs] (at a pair that starts a
        segment after a loss: the status that ended tracking) and segments, a list of dict(first_pair, n_pairs, poses_pnp, poses
        [n + 1, 3, 4]): each segment's trajectory in its own gauge (split_segments).  Segments are not joined, and the map a
        sequence leaves is its last segment's; cam_frame and pt_feature[:, 0] still count along the whole sequence."""
        off = sequence_offsets(seq_lengths, len(self._keep[0]) if getattr(self, "_keep", None) else 0)
        S, B = len(off) - 1, int(off[-1])
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        sq, sp, ss = (0, -1, 0) if snapshot is None else (int(snapshot[0]), int(snapshot[1]), int(snapshot[2]))
        opts = _lib.SlamOpts(int(iterations), float(reproj_err), float(confidence), int(seed), float(max_point_norm), int(ba_iterations),
                             float(huber_delta), int(free_cameras), float(filter_threshold), int(max_cameras), sp, ss)
        flat = dict(poses_pnp=np.zeros((B + S, 12)), poses=np.zeros((B + S, 12)), chi2=np.zeros((B, 2)))
        flat.update({k: np.zeros(B, np.int32) for k in ("n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")})
        c = self.ctx
        keys = ("poses_pnp", "poses", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "chi2", "ba_iterations", "ba_trials")
        if not restart:
            c.check(c.lib.vo_slam_chains(c.handle, S, off.ctypes.data, K.ctypes.data, C.addressof(opts), sq, *[flat[k].ctypes.data for k in keys]))
            return split_sequences(flat, off)
        seg = dict(segment=np.zeros(B, np.int32), cause=np.zeros(B, np.int32), seg_poses_pnp=np.zeros((B, 12)), seg_poses=np.zeros((B, 12)))
        c.check(c.lib.vo_slam_chains_restart(c.handle, S, off.ctypes.data, K.ctypes.data, C.addressof(opts), sq, *[flat[k].ctypes.data for k in keys],
                                             *[seg[k].ctypes.data for k in ("segment", "cause", "seg_poses_pnp", "seg_poses")]))
        out = split_sequences(flat, off)
        for s, d in enumerate(out):
            a, b = int(off[s]), int(off[s + 1])
            d["segment"] = seg["segment"][a:b].copy(); d["cause"] = seg["cause"][a:b].copy()
            d["segments"] = split_segments(d["segment"], d["poses_pnp"], d["poses"], seg["seg_poses_pnp"][a:b], seg["seg_poses"][a:b])
        return out

    def slam_streams(self, seq_lengths, K, resume=False, total_pairs=None, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED,
                     max_point_norm=50.0, ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18, snapshot=None):
        """slam_stream_restart for several sequences at once (vo_slam_streams), one workgroup per sequence and kernel: the pairs of
        the latest run_pairs(..., want_points=True) are sequence 0's seq_lengths[0] pairs, then sequence 1's, ...  resume=False
        starts the stream: every sequence has at least one pair, no frame slot belongs to two sequences, total_pairs is a list of
        len(seq_lengths) — how many pairs each sequence may reach (default: its pairs of this call).  resume=True continues it
        with the same number of sequences, K and options: a sequence that advances starts at the slot of its last frame, and a
        sequence may be idle (length 0) as long as one advances — it keeps its last frame's slot, its map and its state, and goes
        on in a later call as if the idle calls had not happened.  Every slot but the sequences' last frames' is free between calls.
        For every sequence the calls together compute what slam_stream_restart computes for that flight alone, byte for byte.
        snapshot=(seq, pair, stage), the pair counted along that sequence's pairs of this call (slam_map(1, seq=seq)).
        Returns one dict for the call, laid out as vo_slam_chains_restart lays its outputs out: seq_off [S + 1]; poses_pnp, poses
        [B + S, 3, 4] (sequence s owns rows seq_off[s] + s .. seq_off[s + 1] + s; an idle one its last frame's row); n_corr, n_inl,
        status, n_pts, n_obs, n_cam, ba_iterations, ba_trials, segment, cause [B]; chi2 [B, 2]; seg_poses_pnp, seg_poses [B, 3, 4];
        n_carried [S]; carried_frame, carried_poses: lists of S arrays [n_s] / [n_s, 3, 4], frames counted along the sequence's own
        stream.  stream_slice(out, s) is sequence s's part as slam_stream_restart returns it, join_streams(outs) the whole flights.
        slam_map(which, seq) reports every sequence after every call, an idle one too."""
        lengths = [int(v) for v in seq_lengths]
        if not lengths or min(lengths) < 0:
            raise ValueError(f"slam_streams takes at least one sequence and no negative length, got {lengths}")
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        S, B = len(lengths), int(off[-1])
        total = np.ascontiguousarray(lengths if total_pairs is None else [int(v) for v in total_pairs], dtype=np.int32)
        if len(total) != S:
            raise ValueError(f"total_pairs names {len(total)} sequences, seq_lengths {S}")
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        sq, sp, ss = (0, -1, 0) if snapshot is None else (int(snapshot[0]), int(snapshot[1]), int(snapshot[2]))
        opts = _lib.SlamOpts(int(iterations), float(reproj_err), float(confidence), int(seed), float(max_point_norm), int(ba_iterations),
                             float(huber_delta), int(free_cameras), float(filter_threshold), int(max_cameras), sp, ss)
        flat = dict(poses_pnp=np.zeros((B + S, 12)), poses=np.zeros((B + S, 12)), chi2=np.zeros((B, 2)))
        flat.update({k: np.zeros(B, np.int32) for k in ("n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials", "segment", "cause")})
        flat.update(seg_poses_pnp=np.zeros((B, 12)), seg_poses=np.zeros((B, 12)))
        rows = max(int(max_cameras), 1)
        nc = np.zeros(S, np.int32); cf = np.zeros((S, rows), np.int32); cp = np.zeros((S, rows, 12))
        keys = ("poses_pnp", "poses", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "chi2", "ba_iterations", "ba_trials",
                "segment", "cause", "seg_poses_pnp", "seg_poses")
        c = self.ctx
        c.check(c.lib.vo_slam_streams(c.handle, int(bool(resume)), S, total.ctypes.data, off.ctypes.data, K.ctypes.data, C.addressof(opts), sq,
                                      *[_lib.ptr(flat[k]) for k in keys], nc.ctypes.data, cf.ctypes.data, cp.ctypes.data))
        for k in ("poses_pnp", "poses", "seg_poses_pnp", "seg_poses"):
            flat[k] = flat[k].reshape(-1, 3, 4)
        return dict(seq_off=off, n_carried=nc, carried_frame=[cf[s, :nc[s]].copy() for s in range(S)],
                    carried_poses=[cp[s, :nc[s]].reshape(-1, 3, 4).copy() for s in range(S)], **flat)

    def slam_streams_open(self, n_seats, total_pairs, K, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED,
                          max_point_norm=50.0, ba_iterations=40, huber_delta=1.0, free_cameras=2, filter_threshold=1.0, max_cameras=18, snapshot=None):
        """A slam_streams stream of n_seats vacant seats (vo_slam_streams_open): nothing is walked and no run_pairs is needed.
        total_pairs (a list of n_seats, or one number for all) is every seat's capacity — the longest flight it may hold.  Every
        later call is slam_streams(..., resume=True) with this K and these options: a vacant seat may stay idle or take a flight,
        whose pair 0 starts at any slot no other sequence holds and for which everything counts from zero (slam_streams_replace).
        snapshot is accepted for symmetry with slam_streams and ignored: there is no pair to take one of."""
        S = int(n_seats)
        total = np.ascontiguousarray(np.broadcast_to(np.asarray(total_pairs, dtype=np.int32), (max(S, 0),)), dtype=np.int32)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        opts = _lib.SlamOpts(int(iterations), float(reproj_err), float(confidence), int(seed), float(max_point_norm), int(ba_iterations),
                             float(huber_delta), int(free_cameras), float(filter_threshold), int(max_cameras), -1, 0)
        c = self.ctx
        c.check(c.lib.vo_slam_streams_open(c.handle, S, total.ctypes.data, K.ctypes.data, C.addressof(opts)))

    def slam_streams_replace(self, seq, total_pairs):
        """Between two calls of a live slam_streams stream: the flight of seat `seq` is over (vo_slam_streams_replace).  The seat is
        vacant, its last frame's slot is free at once, and the next flight that takes it — in any later call, from any slot no
        other sequence holds — starts from zero and may reach total_pairs pairs (at most the seat's capacity: what the stream's
        first call or slam_streams_open was given for it).  That flight's calls together compute what slam_stream_restart computes
        for it alone, byte for byte (split_flights).  Host only; replacing a vacant seat only sets the bound."""
        c = self.ctx
        c.check(c.lib.vo_slam_streams_replace(c.handle, int(seq), int(total_pairs)))

    def slam_map(self, which=0, seq=0):
        """The map of the latest slam_chain, or of sequence `seq` of the latest slam_chains or slam_streams call: which=0 at the end of the
        chain, 1 the snapshot.  dict(cam_frame [ncam] index of the camera's frame in the chain, cam_pose [ncam, 3, 4], cam_fixed [ncam] bool,
        pt_feature [npt, 2] (chain frame, keypoint), points [npt, 3], obs_cam, obs_pt [nobs], obs_xy [nobs, 2])."""
        if seq:
            return self._slam_chains_map(int(seq), int(which))
        c = self.ctx
        n = [C.c_int32(0) for _ in range(3)]
        c.check(c.lib.vo_slam_map_size(c.handle, int(which), *[C.addressof(v) for v in n]))
        nc, npt, no = (v.value for v in n)
        m = dict(cam_frame=np.zeros(nc, np.int32), cam_pose=np.zeros((nc, 3, 4)), cam_fixed=np.zeros(nc, np.uint8),
                 pt_feature=np.zeros((npt, 2), np.int32), points=np.zeros((npt, 3)), obs_cam=np.zeros(no, np.int32),
                 obs_pt=np.zeros(no, np.int32), obs_xy=np.zeros((no, 2)))
        c.check(c.lib.vo_slam_map(c.handle, int(which), *[_lib.ptr(m[k]) for k in ("cam_frame", "cam_pose", "cam_fixed", "pt_feature", "points",
                                                                                  "obs_cam", "obs_pt", "obs_xy")]))
        m["cam_fixed"] = m["cam_fixed"].astype(bool)
        return m

    def _slam_chains_map(self, seq, which):
        c = self.ctx
        n = [C.c_int32(0) for _ in range(3)]
        c.check(c.lib.vo_slam_chains_map_size(c.handle, seq, which, *[C.addressof(v) for v in n]))
        nc, npt, no = (v.value for v in n)
        m = dict(cam_frame=np.zeros(nc, np.int32), cam_pose=np.zeros((nc, 3, 4)), cam_fixed=np.zeros(nc, np.uint8),
                 pt_feature=np.zeros((npt, 2), np.int32), points=np.zeros((npt, 3)), obs_cam=np.zeros(no, np.int32),
                 obs_pt=np.zeros(no, np.int32), obs_xy=np.zeros((no, 2)))
        c.check(c.lib.vo_slam_chains_map(c.handle, seq, which, *[_lib.ptr(m[k]) for k in ("cam_frame", "cam_pose", "cam_fixed", "pt_feature", "points",
                                                                                          "obs_cam", "obs_pt", "obs_xy")]))
        m["cam_fixed"] = m["cam_fixed"].astype(bool)
        return m

    def map_stats(self, on=True):
        """Switch Map.show_map_statistics (src/map.py:234-297) for the resident map on or off (vo_set_slam_stats; off by default).
        While on, every slam_chain / slam_chains / slam_stream / slam_stream_restart / slam_streams call runs one more kernel per
        step and slam_stats() reports its rows; the calls' own results do not change.  A stream keeps the setting it started with."""
        c = self.ctx
        c.check(c.lib.vo_set_slam_stats(c.handle, int(bool(on))))

    def slam_stats(self, seq=0):
        """The statistics of sequence `seq` of the latest slam_* call, one row per pair of that sequence in the call, each for the
        map as n_pts / n_obs / n_cam of that pair describe it: dict(total_sqerr [B] (calculate_reprojection_error: the sum in
        observation order), mean_sqerr [B] (total / n_obs, 0 without observations), max_sqerr [B], n_high [B] (sqerr > 10),
        obs_hist [B, 64] (points by number of observations, bin 63 = 63 or more, bin 0 = none), obs_matrix [B, C, C] (points two
        cameras see together, upper triangle, by position in the camera list; C = max_cameras), cam_frame [B, C] (the camera
        list, -1 past its end, counted as slam_map counts it)).  Raises VoError if the call ran with map_stats off."""
        c = self.ctx
        nb, nc = C.c_int32(0), C.c_int32(0)
        c.check(c.lib.vo_slam_stats_size(c.handle, int(seq), C.addressof(nb), C.addressof(nc)))
        B, cm = nb.value, nc.value
        d = dict(total_sqerr=np.zeros(B), max_sqerr=np.zeros(B), n_high=np.zeros(B, np.int32), obs_hist=np.zeros((B, _lib.VO_STATS_HIST), np.int32),
                 obs_matrix=np.zeros((B, cm, cm), np.int32), cam_frame=np.zeros((B, cm), np.int32))
        c.check(c.lib.vo_slam_stats(c.handle, int(seq), B, cm, *[d[k].ctypes.data for k in ("total_sqerr", "max_sqerr", "n_high", "obs_hist",
                                                                                            "obs_matrix", "cam_frame")]))
        n = [np.zeros(B, np.int32) for _ in range(3)]
        c.check(c.lib.vo_slam_stats_counts(c.handle, int(seq), B, *[v.ctypes.data for v in n]))
        d["mean_sqerr"] = mean_sqerr(d["total_sqerr"], n[2])
        return d

    def gather_records(self, B, world=1, wait=True):
        """All-gather the [R|t] + counts records (16 float64 per pair) of the first B pairs of the latest run_pairs
        over the context's RCCL communicator (ctx.comm_init; without one: the local records).  Returns a
        [world, B, 16] view of a reused page-locked buffer, valid at once (wait) or after self.wait()."""
        if getattr(self, "_gath", None) is None or self._gath.array.shape[0] < world * self.max_pairs:
            self._gath = _lib.PinnedArray((world * self.max_pairs, _lib.VO_RECORD_DOUBLES), np.float64)
        out = self._gath.array[:world * B]
        c = self.ctx
        c.check(c.lib.vo_pairs_gather(c.handle, int(B), out.ctypes.data, int(bool(wait))))
        return out.reshape(world, B, _lib.VO_RECORD_DOUBLES)

    def epipolar_stats(self, K, want_dist=False, n_pairs=None):
        """The symmetric epipolar distances of src/feature_detection.py:127-140 for every pair of the latest run_pairs, computed
        on what it left on the device (vo_pairs_epipolar): per E inlier k in match order d_k = |l1 . (x2, 1)| + |l2 . (x1, 1)|
        with the epilines of the PIXEL fundamental matrix K^-T E K^-1 [deviation: the script passes E with pixel points].
        Returns dict(n [B] int32, mean, std, max [B] float64: sequential sums in match order, so np.mean / np.std of the same
        distances can differ in the last bits; dist: with want_dist a list of B arrays [n[p]], else None).  A failed pair gives
        n = 0 and zeros.  n_pairs defaults to the latest run's pair count; any other value is refused by the library."""
        B = int(getattr(self, "_last_pairs", 0) if n_pairs is None else n_pairs)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        n = np.zeros(max(B, 1), np.int32); mean = np.zeros(max(B, 1)); sd = np.zeros(max(B, 1)); mx = np.zeros(max(B, 1))
        dist = np.zeros((max(B, 1), self.kp_cap)) if want_dist else None
        c = self.ctx
        rc = c.lib.vo_pairs_epipolar(c.handle, B, K.ctypes.data, n.ctypes.data, mean.ctypes.data, sd.ctypes.data, mx.ctypes.data, _lib.ptr(dist))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return dict(n=n[:B], mean=mean[:B], std=sd[:B], max=mx[:B],
                    dist=[dist[p, :n[p]].copy() for p in range(B)] if want_dist else None)

    def pair_matches(self, pair):
        cap = self.kp_cap
        qi = np.empty(cap, np.int32); ti = np.empty(cap, np.int32); d = np.empty(cap, np.float32)
        m = np.empty(cap, np.uint8); n = C.c_int32(0)
        c = self.ctx
        c.check(c.lib.vo_pair_matches(c.handle, int(pair), qi.ctypes.data, ti.ctypes.data, d.ctypes.data,
                                      m.ctypes.data, cap, C.addressof(n)))
        k = n.value
        return qi[:k].copy(), ti[:k].copy(), d[:k].copy(), m[:k].copy()

    # ---- relocalisation: a resident frame placed in a map by its descriptors (vo_map_*) -------
    def _map_row_width(self):
        return 128 if self.detector == "sift" else 32

    def _map_rows_u8(self, rows):
        """a map's descriptor rows as the library takes them: [npt, D] uint8, contiguous"""
        D = self._map_row_width()
        r = np.asarray(rows)
        if r.ndim != 2 or r.shape[1] != D:
            raise ValueError(f"rows must be [npt, {D}]")
        if r.dtype != np.uint8:
            u = r.astype(np.uint8)
            if not np.array_equal(u.astype(r.dtype), r):
                raise ValueError("descriptor rows must hold integer values 0..255")
            r = u
        return np.ascontiguousarray(r)

    def stage_map(self, rows, points):
        """Stage a map the caller holds (vo_map_stage): rows [npt, 32] uint8 under ORB, [npt, 128] under SIFT (uint8, or the
        integer-valued float32 rows features() hands out); points [npt, 3] float64 in the map's own gauge.  Replaces the map
        staged before; up to 65536 points (NotImplementedError beyond)."""
        r = self._map_rows_u8(rows)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        if len(p) != len(r):
            raise ValueError("points must be [npt, 3]")
        c = self.ctx
        rc = c.lib.vo_map_stage(c.handle, r.ctypes.data, p.ctypes.data, len(r))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)

    def map_from_slam(self, which=0, seq=0):
        """Stage the map of the latest slam_chain (seq=0) or of sequence `seq` of the latest slam_chains (vo_map_from_slam; which
        as in slam_map), on the device: the map's coordinates, and per point the descriptor row of its owning feature
        (TrackedPoint.descriptor = match.descriptor1) gathered from the slot it was detected in.  Call it right after the chain,
        while the slots still hold its frames.  A stream's map: NotImplementedError (its older frames have left their slots) —
        unless it is a slam_stream started with stream_rows() on: then which=0 is map_from_stream(), at any time."""
        c = self.ctx
        rc = c.lib.vo_map_from_slam(c.handle, int(seq), int(which))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)

    def stream_rows(self, capacity=-1):
        """Give the next slam_stream a descriptor store (vo_set_stream_rows; off by default): the stream then keeps the descriptor row
        of every map point on the device from the call the point is born in, and map_from_stream() stages its live map at any later
        time.  capacity: rows the store holds — -1 one per feature the stream can hold, (total_pairs + 1) * kp_cap, which never
        drops a point; 0 switches the store off.  Memory: capacity * D + 4 * (total_pairs + 1) * kp_cap bytes (D = 32 ORB, 128 SIFT).
        Takes effect at the next slam_stream(resume=False); a live stream keeps the setting it started with.  slam_stream_restart,
        slam_streams and the chains ignore it.  The stream's own outputs do not change."""
        c = self.ctx
        c.check(c.lib.vo_set_stream_rows(c.handle, int(capacity)))

    def stream_rows_info(self):
        """The live slam_stream's descriptor store (vo_stream_rows_info): dict(capacity, stored — rows handed out so far, holes
        included —, dropped — points that found the store full and stay without a row).  VoError without such a stream."""
        c = self.ctx
        v = [C.c_int64(0) for _ in range(3)]
        c.check(c.lib.vo_stream_rows_info(c.handle, *[C.addressof(x) for x in v]))
        return dict(capacity=v[0].value, stored=v[1].value, dropped=v[2].value)

    def map_from_stream(self, first=0, end=None):
        """Stage the live slam_stream's map from its descriptor store (vo_map_from_stream), restricted to the points whose owning
        frame — pt_feature[:, 0], counted along the stream — lies in [first, end); end=None: no upper bound.  Works at any time
        while the stream lives: after its frames have lost their slots, between two calls, after a call that ended lost.  Points and
        rows come in map order (map_rows() returns them); points without a row (dropped at capacity) are left out.  Returns
        dict(n=points staged, without_row=points of the window left out).  More than 65536 points: NotImplementedError — stage a
        window.  The stream is left as it was."""
        c = self.ctx
        n, w = C.c_int32(0), C.c_int32(0)
        rc = c.lib.vo_map_from_stream(c.handle, int(first), -1 if end is None else int(end), C.addressof(n), C.addressof(w))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return dict(n=n.value, without_row=w.value)

    def stream_archive(self, capacity=-1):
        """Give the next slam_stream an archive of evicted points (vo_set_stream_archive; off by default): every point the camera
        limit removes is then kept on the device in removal order — its coordinates as the map held them, its owning feature, a
        copy of its descriptor row and the pair at which it went — and map_from_stream_archive() stages those points long after
        max_cameras has taken their cameras.  capacity: entries — -1 one per feature the stream can hold, which never drops a
        point; 0 switches the archive off.  Memory: capacity * (D + 40) bytes (D = 32 ORB, 128 SIFT) plus 8 bytes per 256 entries.
        Needs stream_rows() on as well (the rows of earlier calls' points come from the store): slam_stream(resume=False) raises
        VoError otherwise.  Takes effect at the next slam_stream(resume=False); a live stream keeps the setting it started with.
        slam_stream_restart, slam_streams and the chains ignore it.  The stream's own outputs, its map and its store do not change."""
        c = self.ctx
        c.check(c.lib.vo_set_stream_archive(c.handle, int(capacity)))

    def stream_archive_info(self):
        """The live slam_stream's archive (vo_stream_archive_info): dict(capacity, stored — entries so far —, dropped — removed
        points that found the archive full, for good).  VoError without such a stream."""
        c = self.ctx
        v = [C.c_int64(0) for _ in range(3)]
        c.check(c.lib.vo_stream_archive_info(c.handle, *[C.addressof(x) for x in v]))
        return dict(capacity=v[0].value, stored=v[1].value, dropped=v[2].value)

    def stream_archive_points(self, first=0, n=None):
        """Entries first .. first + n - 1 of the live slam_stream's archive, in removal order (vo_stream_archive_read; n=None: all
        from `first`): dict(feature [n, 2] int32 — frame along the stream, keypoint —, xyz [n, 3] float64, evicted_at [n] int32,
        has_row [n] bool, rows [n, D] uint8 — zeros where has_row is False).  What to save, and what stage_map takes later."""
        first = int(first)
        if n is None:
            n = max(self.stream_archive_info()["stored"] - first, 0)
        n = int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        out = dict(feature=np.zeros((n, 2), np.int32), xyz=np.zeros((n, 3)), evicted_at=np.zeros(n, np.int32), has_row=np.zeros(n, np.int32),
                   rows=np.zeros((n, self._map_row_width()), np.uint8))
        c = self.ctx
        c.check(c.lib.vo_stream_archive_read(c.handle, first, n, *[out[k].ctypes.data for k in ("feature", "xyz", "evicted_at", "has_row", "rows")]))
        out["has_row"] = out["has_row"] != 0
        return out

    def map_from_stream_archive(self, first=0, end=None, live=True):
        """map_from_stream() with the archived points (vo_map_from_stream_archive): the points the camera limit has removed whose
        owning frame lies in [first, end), in removal order, behind the live points of the window (live=True: exactly what
        map_from_stream(first, end) stages, first, so that a live point wins the cross-check's lowest-index tie on a duplicated row)
        or alone (live=False).  Entries without a row are left out.  Returns dict(n=points staged, n_archived=archived ones among
        them, without_row=points of the window left out).  More than 65536 points: NotImplementedError — stage a window.  The
        stream and its archive are left as they were.  VoError on a stream started without stream_archive()."""
        c = self.ctx
        n, a, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rc = c.lib.vo_map_from_stream_archive(c.handle, int(first), -1 if end is None else int(end), 1 if live else 0, C.addressof(n), C.addressof(a),
                                              C.addressof(w))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return dict(n=n.value, n_archived=a.value, without_row=w.value)

    def map_rows(self):
        """The staged map back (vo_map_rows): (rows [npt, D] uint8, points [npt, 3] float64) — what to save before a segment's
        frames leave their slots, and what stage_map takes later."""
        c = self.ctx
        n = C.c_int32(0)
        c.check(c.lib.vo_map_rows(c.handle, None, None, 0, C.addressof(n)))
        rows = np.zeros((n.value, self._map_row_width()), np.uint8); pts = np.zeros((n.value, 3))
        c.check(c.lib.vo_map_rows(c.handle, rows.ctypes.data, pts.ctypes.data, n.value, C.addressof(n)))
        return rows, pts

    def relocalize(self, slots, K, max_distance=0.0, iterations=100, reproj_err=8.0, confidence=0.99, seed=OPENCV_RNG_SEED, min_inliers=0,
                   match="cross", ratio=0.75, refine_radius=None):
        """Place detected slots in the staged map by their descriptors (vo_map_localize), all in one call on the device:
        bf.match(frame, map) with crossCheck=True -> `distance < max_distance` (0: no filter) -> cv2.solvePnPRansac on the 3D-2D
        matches.  match='ratio': knnMatch(frame, map, k=2) and `m.distance < ratio * n.distance` (src/feature_detection.py:20-26) in
        the place of the cross-check — no reverse direction is computed, several keypoints may keep one map point;
        match='cross+ratio': both.  The call sets the context's vo_set_map_match to what it is given.  Returns dict(poses [Q, 3, 4] world -> camera in the map's gauge, zeros where status != 0; n_match, n_inl,
        status [Q]: 0, VO_ERR_TOO_FEW (fewer than 4 matches) or VO_ERR_NO_MODEL (no model, or fewer than min_inliers inliers)).
        refine_radius=R (pixels): the refinement pass on top — relocalize_guided(prior=None, radius=R) with the same options and no
        ratio rule, started from these poses on the device; the result is that call's (n_seen included), with this pass's counts
        as first_n_match and first_n_inl.  None (default): no such pass."""
        sl = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        Q = len(sl)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        opts = _lib.RelocOpts(float(max_distance), int(iterations), float(reproj_err), float(confidence), int(seed), int(min_inliers))
        poses = np.zeros((Q, 12)); nm = np.zeros(Q, np.int32); ni = np.zeros(Q, np.int32); st = np.zeros(Q, np.int32)
        c = self.ctx
        c.set_map_match(match, ratio)
        c.check(c.lib.vo_map_localize(c.handle, sl.ctypes.data, Q, K.ctypes.data, C.addressof(opts), poses.ctypes.data, nm.ctypes.data,
                                      ni.ctypes.data, st.ctypes.data))
        if refine_radius is None:
            return dict(poses=poses.reshape(Q, 3, 4), n_match=nm, n_inl=ni, status=st)
        out = self.relocalize_guided(sl, K, None, refine_radius, 0.0, max_distance, iterations, reproj_err, confidence, seed, min_inliers)
        out.update(first_n_match=nm, first_n_inl=ni)
        return out

    def relocalize_guided(self, slots, K, prior, radius, ratio=0.0, max_distance=0.0, iterations=100, reproj_err=8.0, confidence=0.99,
                          seed=OPENCV_RNG_SEED, min_inliers=0):
        """Place detected slots in the staged map by projection under a prior pose (vo_map_localize_guided; ORB-SLAM's
        SearchByProjection), all in one call on the device: every map point in front of the camera prior[q] ([Q, 3, 4] world ->
        camera in the map's gauge) is projected with K, takes the keypoint with the nearest descriptor among those within `radius`
        pixels of its projection (ratio > 0: only if it has one candidate or `distance < ratio * second distance`; max_distance > 0:
        only if `distance < max_distance`), a keypoint keeps the nearest point that took it, and cv2.solvePnPRansac runs on those
        3D-2D matches as in relocalize().  prior=None: the refinement pass — the priors are the poses the relocalize() just before
        this call left on the device (same slots, same staged map; VoError otherwise), and a query that failed there keeps its
        status with zero counts.  Returns relocalize()'s dict plus n_seen [Q]: the points with at least one keypoint in their
        window.  map_matches(q) and map_match_seconds(q) serve this call afterwards."""
        opts = _lib.RelocOpts(float(max_distance), int(iterations), float(reproj_err), float(confidence), int(seed), int(min_inliers))
        poses, nm, ni, st, ns = self.ctx.map_localize_guided(slots, K, prior, radius, ratio, opts)
        return dict(poses=poses, n_match=nm, n_inl=ni, status=st, n_seen=ns)

    def map_matches(self, q):
        """Query q's matches of the latest relocalize(): (map point [n], keypoint [n], distance [n] float32 as cv2 reports it —
        the value of the reference's `distance = 0  # TODO` — and solvePnPRansac's inlier mask [n] uint8), in keypoint order."""
        cap = self.kp_cap
        pi = np.empty(cap, np.int32); ki = np.empty(cap, np.int32); d = np.empty(cap, np.float32)
        m = np.empty(cap, np.uint8); n = C.c_int32(0)
        c = self.ctx
        c.check(c.lib.vo_map_matches(c.handle, int(q), pi.ctypes.data, ki.ctypes.data, d.ctypes.data, m.ctypes.data, cap, C.addressof(n)))
        k = n.value
        return pi[:k].copy(), ki[:k].copy(), d[:k].copy(), m[:k].copy()

    def _match_seconds(self, which, q, cap):
        d2 = np.empty(max(int(cap), 1), np.float32); n = C.c_int32(0)
        c = self.ctx
        c.check(c.lib.vo_map_match_seconds(c.handle, which, int(q), d2.ctypes.data, len(d2), C.addressof(n)))
        return d2[:n.value].copy()

    def map_match_seconds(self, q):
        """n.distance of knnMatch(k=2) for every entry of map_matches(q), float32, in list order (vo_map_match_seconds) — what the
        ratio rule compared, and what re-thresholding on the host needs.  VoError after a relocalize(match='cross')."""
        return self._match_seconds(0, q, self.kp_cap)

    def map_align_match_seconds(self, q):
        """The same for map_align_matches(q) of the latest align_maps(match='ratio' | 'cross+ratio')."""
        rows = getattr(self, "_align_rows", ())
        return self._match_seconds(1, q, rows[int(q)] if 0 <= int(q) < len(rows) else 1)

    # ---- map alignment: the similarity that joins two maps, by their descriptors (vo_map_align) ------
    def align_maps(self, rows, points, max_error, offsets=None, max_distance=0.0, iterations=1000, confidence=0.99, seed=OPENCV_RNG_SEED,
                   min_inliers=0, match="cross", ratio=0.75, refine_radius=None):
        """Align Q query maps to the staged map by their descriptors (vo_map_align), all in one call on the device: the cross-check
        match of every query map's rows against the staged rows -> `distance < max_distance` (0: no filter) -> RANSAC over the
        3D-3D matches for X_staged = scale R X_query + t.  rows [total, D] and points [total, 3] hold the query maps one after
        the other, map q being rows offsets[q]:offsets[q + 1] (offsets None: one map); what map_rows() returned for them.
        max_error is the inlier bound in the STAGED map's units and has no default.  match / ratio: as in relocalize(), with a
        query map's rows in the place of a frame's (map_align_match_seconds(q) returns the second distances).  Returns dict(scale [Q], R [Q, 3, 3], t [Q, 3]
        (zeros where status != 0), n_match, n_inl, status [Q]: 0, VO_ERR_TOO_FEW (fewer than 3 matches) or VO_ERR_NO_MODEL).
        Up to 64 maps and 65536 rows in one call (NotImplementedError beyond).
        refine_radius=R (a length in the staged map's units): the refinement pass on top — align_maps_guided(None, ..., radius=R)
        with the same options and no ratio rule, started from these similarities on the device; the result is that call's (n_seen
        included), with this pass's counts as first_n_match and first_n_inl.  None (default): no such pass."""
        r = self._map_rows_u8(rows)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        if len(p) != len(r):
            raise ValueError("points must be [total, 3]")
        off = np.ascontiguousarray([0, len(r)] if offsets is None else offsets, dtype=np.int32).ravel()
        Q = len(off) - 1
        if Q < 0 or int(off[-1]) != len(r):
            raise ValueError("offsets must be [Q + 1] and end at the number of rows")
        opts = _lib.AlignOpts(float(max_distance), float(max_error), int(iterations), float(confidence), int(seed), int(min_inliers))
        sim = np.zeros((Q, 13)); nm = np.zeros(Q, np.int32); ni = np.zeros(Q, np.int32); st = np.zeros(Q, np.int32)
        c = self.ctx
        c.set_map_match(match, ratio)
        rc = c.lib.vo_map_align(c.handle, r.ctypes.data, p.ctypes.data, off.ctypes.data, Q, C.addressof(opts), sim.ctypes.data, nm.ctypes.data,
                                ni.ctypes.data, st.ctypes.data)
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        self._align_rows = np.diff(off)
        if refine_radius is None:
            return dict(scale=sim[:, 0].copy(), R=sim[:, 1:10].reshape(Q, 3, 3).copy(), t=sim[:, 10:].copy(), n_match=nm, n_inl=ni, status=st)
        out = self.align_maps_guided(None, None, None, refine_radius, max_error, max_distance=max_distance, iterations=iterations,
                                     confidence=confidence, seed=seed, min_inliers=min_inliers)
        out.update(first_n_match=nm, first_n_inl=ni)
        return out

    def align_maps_guided(self, rows, points, prior, radius, max_error, offsets=None, ratio=0.0, max_distance=0.0, iterations=1000,
                          confidence=0.99, seed=OPENCV_RNG_SEED, min_inliers=0):
        """Align Q query maps to the staged map by matching their points in space under a prior similarity (vo_map_align_guided; the
        3D-3D half of ORB-SLAM's SearchAndFuse), all in one call on the device: every query point is moved into the staged map's
        gauge by prior[q] = (scale, R, t) — a tuple of arrays [Q], [Q, 3, 3], [Q, 3] as align_maps returns them, or [Q, 13] —,
        takes the staged point with the nearest descriptor among those within `radius` (staged units) of it (ratio > 0: only if it
        has one candidate or `distance < ratio * second distance`; max_distance > 0: only if `distance < max_distance`), a staged
        point keeps the nearest query point that took it, and the similarity is refitted by align_maps' RANSAC on those matches.
        rows=None (points and prior None too): the refinement pass — the query maps and the priors are the ones the align_maps()
        just before this call left on the device (same staged map; VoError otherwise), and a query that failed there keeps its
        status with zero counts.  Returns align_maps' dict plus n_seen [Q]: the query points with at least one staged point in
        their sphere.  map_align_matches(q) and map_align_match_seconds(q) serve this call afterwards."""
        c = self.ctx
        opts = _lib.AlignOpts(float(max_distance), float(max_error), int(iterations), float(confidence), int(seed), int(min_inliers))
        if rows is None:
            if points is not None or prior is not None or offsets is not None:
                raise ValueError("the refinement pass takes no rows, points, prior or offsets")
            rc, sim, nm, ni, st, ns = c.map_align_guided(None, None, len(getattr(self, "_align_rows", ())), None, radius, ratio, opts)
        else:
            r = self._map_rows_u8(rows)
            p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
            if len(p) != len(r):
                raise ValueError("points must be [total, 3]")
            off = np.ascontiguousarray([0, len(r)] if offsets is None else offsets, dtype=np.int32).ravel()
            Q = len(off) - 1
            if Q < 0 or int(off[-1]) != len(r):
                raise ValueError("offsets must be [Q + 1] and end at the number of rows")
            if isinstance(prior, (tuple, list)) and len(prior) == 3 and np.ndim(prior[1]) >= 2:
                s, R, t = prior
                prior = np.concatenate([np.reshape(np.asarray(s, np.float64), (-1, 1)), np.reshape(np.asarray(R, np.float64), (-1, 9)),
                                        np.reshape(np.asarray(t, np.float64), (-1, 3))], axis=1)
            rc, sim, nm, ni, st, ns = c.map_align_guided(r, p, off, prior, radius, ratio, opts)
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        if rows is not None:
            self._align_rows = np.diff(off)
        Q = len(sim)
        return dict(scale=sim[:, 0].copy(), R=sim[:, 1:10].reshape(Q, 3, 3).copy(), t=sim[:, 10:].copy(), n_match=nm, n_inl=ni, status=st, n_seen=ns)

    def fuse_map(self, rows, points, max_error, radius, max_distance=0.0, iterations=1000, confidence=0.99, seed=OPENCV_RNG_SEED, min_inliers=0,
                 match="cross", ratio=0.75):
        """Fuse map B (rows [nb, D], points [nb, 3]) into the staged map A: map_rows() for A, align_maps(B) by descriptors, the
        refinement pass within `radius` (A's units), map_align_matches, merge_maps on the host, and stage_map of the result — one
        map, each ground point once.  Returns dict(rows, points — the merged map, now staged —, index_b [nb] (where each point
        of B went), n_fused, n_a, the refined align result as `align` and its map_align_matches(0) as `matches`).  When the alignment
        fails (status != 0) nothing is merged
        or staged: rows and points are None, index_b None, n_fused 0.  A merged map of more than 65536 points: NotImplementedError,
        as stage_map raises it, with A still staged."""
        rows_a, pts_a = self.map_rows()
        r = self._map_rows_u8(rows)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        al = self.align_maps(r, p, max_error, max_distance=max_distance, iterations=iterations, confidence=confidence, seed=seed,
                             min_inliers=min_inliers, match=match, ratio=ratio, refine_radius=radius)
        out = dict(rows=None, points=None, index_b=None, n_fused=0, n_a=len(rows_a), align=al)
        if al["status"][0] != 0:
            return out
        out["matches"] = ai, bi, _, mask = self.map_align_matches(0)      # (staging the merged map forgets them on the device)
        m = merge_maps(rows_a, pts_a, r, p, al["scale"][0], al["R"][0], al["t"][0], ai, bi, mask)
        if len(m["rows"]) > 65536:
            raise NotImplementedError("a staged map holds at most 65536 points, the merged map has %d" % len(m["rows"]))
        self.stage_map(m["rows"], m["points"])
        out.update(m)
        return out

    def map_align_matches(self, q):
        """Query map q's matches of the latest align_maps(): (staged row [n], query row [n], distance [n] float32 as cv2 reports
        it, the RANSAC inlier mask [n] uint8), in query-row order."""
        c = self.ctx
        n = C.c_int32(0)
        rows = getattr(self, "_align_rows", ())
        cap = max(int(rows[int(q)]), 1) if 0 <= int(q) < len(rows) else 1
        ai = np.empty(cap, np.int32); bi = np.empty(cap, np.int32); d = np.empty(cap, np.float32); m = np.empty(cap, np.uint8)
        c.check(c.lib.vo_map_align_matches(c.handle, int(q), ai.ctypes.data, bi.ctypes.data, d.ctypes.data, m.ctypes.data, cap, C.addressof(n)))
        k = n.value
        return ai[:k].copy(), bi[:k].copy(), d[:k].copy(), m[:k].copy()

    # ---- place recognition: device vocabulary, keyframe index, loop query (vo_vocab_*, vo_places_*) ------
    def _slot_list(self, slots):
        return np.ascontiguousarray(slots, dtype=np.int32).ravel()

    def train_vocabulary(self, slots, K=1024, iterations=8):
        """Train a vocabulary of K words (a multiple of 256, 256 .. 4096) on the descriptor rows of the detected `slots`, on the
        device (vo_vocab_train): word w starts as training row floor(w n / K); a round assigns every row to its nearest word (lowest
        index on a tie) and replaces every word by its rows' bitwise majority (ORB) or rounded mean (SIFT); at most `iterations`
        rounds, fewer when an assignment moves no row.  Returns the number of updates done.  Closes an open index."""
        sl = self._slot_list(slots)
        c = self.ctx
        run = C.c_int32(0)
        rc = c.lib.vo_vocab_train(c.handle, sl.ctypes.data, len(sl), int(K), int(iterations), C.addressof(run))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return run.value

    def set_vocabulary(self, words):
        """Take a vocabulary from the host (vo_vocab_set): words [K, 32] uint8 under ORB, [K, 128] integer values 0..255 under SIFT —
        what vocabulary() returned.  Closes an open index."""
        w = self._map_rows_u8(words)
        c = self.ctx
        c.check(c.lib.vo_vocab_set(c.handle, w.ctypes.data, len(w)))

    def vocabulary(self):
        """The vocabulary's words [K, D] uint8 (vo_vocab_get)."""
        c = self.ctx
        k = C.c_int32(0)
        c.check(c.lib.vo_vocab_get(c.handle, None, 0, C.addressof(k)))
        w = np.zeros((k.value, self._map_row_width()), np.uint8)
        c.check(c.lib.vo_vocab_get(c.handle, w.ctypes.data, k.value, C.addressof(k)))
        return w

    def words(self, slot):
        """The word index of every descriptor row of a detected slot, [n] int32 (vo_vocab_words)."""
        c = self.ctx
        out = np.zeros(self.kp_cap, np.int32); n = C.c_int32(0)
        c.check(c.lib.vo_vocab_words(c.handle, int(slot), out.ctypes.data, self.kp_cap, C.addressof(n)))
        return out[:n.value].copy()

    def places_open(self, capacity):
        """Open an empty keyframe index of up to `capacity` entries (1 .. 65536) over the current vocabulary (vo_places_open)."""
        c = self.ctx
        c.check(c.lib.vo_places_open(c.handle, int(capacity)))

    def places_add(self, slots, ids):
        """Quantise the detected `slots` and append one entry each to the index, `ids` being the caller's frame numbers
        (vo_places_add).  Returns the index of the first new entry.  NotImplementedError when the index is full (nothing is added)."""
        sl = self._slot_list(slots)
        fid = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if len(fid) != len(sl):
            raise ValueError("one id per slot")
        c = self.ctx
        first = C.c_int32(0)
        rc = c.lib.vo_places_add(c.handle, sl.ctypes.data, len(sl), fid.ctypes.data, C.addressof(first))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return first.value

    def places_add_histograms(self, hist, ids):
        """Append given histograms [n, K] uint8 with their ids (vo_places_add_hist): how a saved index comes back.  Returns the index
        of the first new entry."""
        _, K = self._places_size()
        h = np.asarray(hist)
        if h.dtype != np.uint8 or h.ndim != 2 or h.shape[1] != K:
            raise ValueError(f"hist must be [n, {K}] uint8")
        h = np.ascontiguousarray(h)
        fid = np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if len(fid) != len(h):
            raise ValueError("one id per histogram")
        c = self.ctx
        first = C.c_int32(0)
        rc = c.lib.vo_places_add_hist(c.handle, h.ctypes.data, fid.ctypes.data, len(h), C.addressof(first))
        if rc == _lib.VO_ERR_UNSUPPORTED:
            raise NotImplementedError(c.last_error())
        c.check(rc)
        return first.value

    def _places_size(self):
        c = self.ctx
        n, K = C.c_int32(0), C.c_int32(0)
        c.check(c.lib.vo_places_size(c.handle, C.addressof(n), C.addressof(K)))
        return n.value, K.value

    def places_entries(self):
        """The index back (vo_places_entries): dict(hist [n, K] uint8, sum [n] int32 — the sum of the saturated counts —, id [n]
        int32): what to save, and what places_add_histograms takes later."""
        n, K = self._places_size()
        hist = np.zeros((n, K), np.uint8); s = np.zeros(n, np.int32); fid = np.zeros(n, np.int32)
        c = self.ctx
        c.check(c.lib.vo_places_entries(c.handle, 0, n, hist.ctypes.data, s.ctypes.data, fid.ctypes.data))
        return dict(hist=hist, sum=s, id=fid)

    def places_query(self, entries=None, top_k=3, min_gap=0, min_shared=0):
        """For every query entry (entries=None: every entry of the index) the top_k other entries that share the most words with it
        (vo_places_query): shared = sum over words of min(hist_q, hist_d); entries with |id_q - id_d| < min_gap or shared <
        min_shared are left out; equal scores in ascending entry order.  Returns dict(entry [Q, top_k] int32, -1 in unused places;
        id [Q, top_k] the found entries' ids (0 in unused places); shared [Q, top_k] int32)."""
        n, _ = self._places_size()
        q = np.arange(n, dtype=np.int32) if entries is None else np.ascontiguousarray(entries, dtype=np.int32).ravel()
        Q = len(q)
        opts = _lib.PlacesOpts(int(top_k), int(min_gap), int(min_shared))
        ent = np.full((Q, max(int(top_k), 0)), -1, np.int32); sh = np.zeros(ent.shape, np.int32)
        c = self.ctx
        c.check(c.lib.vo_places_query(c.handle, q.ctypes.data, Q, C.addressof(opts), ent.ctypes.data, sh.ctypes.data))
        ids = np.zeros(n, np.int32)
        if n:
            c.check(c.lib.vo_places_entries(c.handle, 0, n, None, None, ids.ctypes.data))
        found = np.where(ent >= 0, ids[np.maximum(ent, 0)], 0).astype(np.int32) if n else np.zeros(ent.shape, np.int32)
        return dict(entry=ent, id=found, shared=sh)

    # ---- measurement ------------------------------------------------------------------------
    def profile(self, on=True):
        c = self.ctx
        c.check(c.lib.vo_profile_enable(c.handle, int(on)))
        c.check(c.lib.vo_profile_reset(c.handle))

    def profile_read(self):
        ms = np.zeros(_lib.VO_STAGE_COUNT, np.float32); n = np.zeros(_lib.VO_STAGE_COUNT, np.int32)
        c = self.ctx
        c.check(c.lib.vo_profile_read(c.handle, ms.ctypes.data, n.ctypes.data))
        names = [c.lib.vo_stage_name(i).decode() for i in range(_lib.VO_STAGE_COUNT)]
        return {names[i]: (float(ms[i]), int(n[i])) for i in range(_lib.VO_STAGE_COUNT) if n[i] > 0}

    def stage_bytes(self, stage_name, frames):
        c = self.ctx
        for i in range(_lib.VO_STAGE_COUNT):
            if c.lib.vo_stage_name(i).decode() == stage_name:
                return float(c.lib.vo_stage_bytes(c.handle, i, int(frames)))
        raise KeyError(stage_name)


def loop_candidates(result, ids):
    """The loop candidates of a places_query() result as a list of (id_query, id_found, shared), each unordered pair of frames once
    (shared is symmetric, so a pair found from both ends carries one number), in the order the queries report them.  ids [Q]: the
    frame numbers of the query entries, row for row of `result`."""
    ids = np.asarray(ids).ravel()
    ent, found, shared = (np.asarray(result[k]) for k in ("entry", "id", "shared"))
    if len(ids) != len(ent):
        raise ValueError("one id per query row")
    seen, out = set(), []
    for q in range(len(ent)):
        for k in range(ent.shape[1]):
            if ent[q, k] < 0:
                continue
            a, b = int(ids[q]), int(found[q, k])
            key = (min(a, b), max(a, b))
            if key not in seen:
                seen.add(key)
                out.append((a, b, int(shared[q, k])))
    return out


def sequence_offsets(seq_lengths, n_pairs):
    """slam_chains' seq_off: [0, l0, l0 + l1, ...] as int32 for the pair counts `seq_lengths` of the sequences that make up a
    run of `n_pairs` pairs.  ValueError on an empty list, a length < 1 or a sum different from n_pairs."""
    lengths = [int(v) for v in seq_lengths]
    if not lengths:
        raise ValueError("seq_lengths is empty: slam_chains takes at least one sequence")
    if min(lengths) < 1:
        raise ValueError(f"every sequence has at least one pair, got {lengths}")
    if sum(lengths) != int(n_pairs):
        raise ValueError(f"the sequences' {sum(lengths)} pairs are not the {int(n_pairs)} pairs of the latest run_pairs")
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def split_sequences(flat, seq_off):
    """vo_slam_chains' flat outputs -> one slam_chain dict per sequence (copies): per-pair arrays are rows seq_off[s] ..
    seq_off[s + 1] - 1, the pose arrays rows seq_off[s] + s .. seq_off[s + 1] + s (a sequence of B_s pairs has B_s + 1 cameras)."""
    out = []
    for s in range(len(seq_off) - 1):
        a, b = int(seq_off[s]), int(seq_off[s + 1])
        d = {k: (v[a + s:b + s + 1].reshape(-1, 3, 4) if k in ("poses_pnp", "poses") else v[a:b]).copy() for k, v in flat.items()}
        out.append(d)
    return out


def split_segments(segment, poses_pnp, poses, seg_poses_pnp, seg_poses):
    """One sequence's outputs of vo_slam_chains_restart -> its segments, in order of start: a list of dict(first_pair, n_pairs,
    poses_pnp, poses [n_pairs + 1, 3, 4]) (copies).  segment [P]: the pairs' segment indices (-1: in none; a segment's pairs are
    consecutive); poses_pnp / poses [P + 1, ...]: row p + 1 = the second frame of pair p; seg_poses_pnp / seg_poses [P, ...]: at the
    pair that starts a segment, the segment's first camera.  That row goes in front of the rows of the segment's pairs, so every
    segment is a trajectory in one gauge: camera k of the segment is row k, the frame first_pair + k of the sequence."""
    segment = np.asarray(segment).ravel()
    pp, pl = np.asarray(poses_pnp, np.float64).reshape(-1, 3, 4), np.asarray(poses, np.float64).reshape(-1, 3, 4)
    sp, sl = np.asarray(seg_poses_pnp, np.float64).reshape(-1, 3, 4), np.asarray(seg_poses, np.float64).reshape(-1, 3, 4)
    P = len(segment)
    if len(pp) != P + 1 or len(pl) != P + 1 or len(sp) != P or len(sl) != P:
        raise ValueError(f"{P} pairs take {P + 1} pose rows and {P} first-camera rows, got {len(pp)}, {len(pl)}, {len(sp)}, {len(sl)}")
    out, p = [], 0
    while p < P:
        k = int(segment[p])
        if k < 0:
            p += 1
            continue
        if k != len(out):
            raise ValueError(f"pair {p} is in segment {k}, expected segment {len(out)}: segments are numbered in order of start")
        n = 1
        while p + n < P and segment[p + n] == k:
            n += 1
        out.append(dict(first_pair=p, n_pairs=n, poses_pnp=np.concatenate([sp[p:p + 1], pp[p + 1:p + n + 1]]),
                        poses=np.concatenate([sl[p:p + 1], pl[p + 1:p + n + 1]])))
        p += n
    return out


def apply_similarity(poses, scale, R, t):
    """World -> camera poses [..., 3, 4] of gauge B in gauge A, for the similarity X_a = scale R X_b + t (align_maps,
    geometry.estimate_similarity): [R_c | t_c] -> [R_c R^T | scale t_c - R_c R^T t].  The rotation stays a proper rotation; the
    camera frame's units become A's, so a point scale R X + t of gauge A has the camera coordinates scale (R_c X + t_c).  Pure."""
    T = np.asarray(poses, np.float64)
    if T.shape[-2:] != (3, 4):
        raise ValueError("poses must be [..., 3, 4]")
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    Rc = T[..., :3] @ R.T
    return np.concatenate([Rc, (float(scale) * T[..., 3] - Rc @ t)[..., None]], axis=-1)


def merge_maps(rows_a, points_a, rows_b, points_b, scale, R, t, a_idx, b_idx, mask):
    """One map from two aligned ones: B's points go into A's gauge by X_a = scale R X_b + t (componentwise, in the operation order of
    vo_map_align_guided's transform); every match (a_idx[k], b_idx[k]) with mask[k] == 1 is a duplicate, and A's row and point are
    kept for it; the merged map is all of A, then B's non-duplicates in B's order.  The lists are what map_align_matches returns:
    a row of either map appears in at most one match.  Returns dict(rows [n, D], points [n, 3], index_b [nb] int32 — the merged row
    of every point of B: a row of A for a fused point, n_a + its rank among the others otherwise —, n_fused).  A's points keep
    their rows, so its own table is the identity.  Pure numpy; positions of fused points are not averaged."""
    ra = np.asarray(rows_a); rb = np.asarray(rows_b)
    pa = np.asarray(points_a, np.float64).reshape(-1, 3); pb = np.asarray(points_b, np.float64).reshape(-1, 3)
    if len(pa) != len(ra) or len(pb) != len(rb) or (len(ra) and len(rb) and ra.shape[1:] != rb.shape[1:]):
        raise ValueError("rows and points of both maps must agree in length and width")
    ai = np.asarray(a_idx, np.int64).ravel(); bi = np.asarray(b_idx, np.int64).ravel(); keep = np.asarray(mask).ravel() != 0
    if not (len(ai) == len(bi) == len(keep)):
        raise ValueError("a_idx, b_idx and mask must have one entry per match")
    ai, bi = ai[keep], bi[keep]
    if len(ai) and (ai.min() < 0 or ai.max() >= len(ra) or bi.min() < 0 or bi.max() >= len(rb)):
        raise ValueError("a match names a row outside its map")
    if len(np.unique(ai)) != len(ai) or len(np.unique(bi)) != len(bi):
        raise ValueError("a row appears in more than one inlier match")
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3); s = float(scale)
    moved = np.stack([s * ((R[k, 0] * pb[:, 0] + R[k, 1] * pb[:, 1]) + R[k, 2] * pb[:, 2]) + t[k] for k in range(3)], axis=1).reshape(-1, 3)
    fused = np.zeros(len(rb), bool); fused[bi] = True
    index_b = np.empty(len(rb), np.int32)
    index_b[bi] = ai
    index_b[~fused] = len(ra) + np.arange(int((~fused).sum()))
    rows = np.concatenate([ra, rb[~fused]]) if len(rb) else ra.copy()
    return dict(rows=rows, points=np.concatenate([pa, moved[~fused]]), index_b=index_b, n_fused=int(fused.sum()))


def compose_similarity(outer, inner):
    """(scale, R, t) of X -> outer(inner(X)) for two similarities given as (scale, R, t)."""
    s1, R1, t1 = float(outer[0]), np.asarray(outer[1], np.float64).reshape(3, 3), np.asarray(outer[2], np.float64).reshape(3)
    s2, R2, t2 = float(inner[0]), np.asarray(inner[1], np.float64).reshape(3, 3), np.asarray(inner[2], np.float64).reshape(3)
    return s1 * s2, R1 @ R2, s1 * (R1 @ t2) + t1


# ---- Sim(3) vertices of the pose graph (include/vo_hip.h, "pose graph"; map_filters.optimize_pose_graph).  A similarity is 13 doubles
# s, R row-major, t and acts as x -> s R x + t; a tangent is (w, u, sigma): rotation, translation, log-scale.  Pure numpy.
SIM3_TH_W, SIM3_TH_S, SIM3_TH_LOG = 1e-2, 1e-2, 1e-8


def _sim3(S):
    S = np.asarray(S, np.float64).reshape(13)
    return float(S[0]), S[1:10].reshape(3, 3), S[10:13]


def _sim3_pack(s, R, t):
    return np.concatenate([[float(s)], np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def _hat3(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _sim3_v(w, sigma):
    """V = C I + A [w]x + B [w]x^2, the header's closed forms and series"""
    th = float(np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
    m = np.empty(7)
    if abs(sigma) < SIM3_TH_S:
        fact = [1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0]
        for k in range(7):
            m[k] = sum(sigma ** n / (fact[n] * (n + k + 1)) for n in range(8))
    else:
        m[0] = np.expm1(sigma) / sigma
        for k in range(1, 7):
            m[k] = (np.exp(sigma) - k * m[k - 1]) / sigma
    if th < SIM3_TH_W:
        t2 = th * th
        A = m[1] - t2 * m[3] / 6 + t2 * t2 * m[5] / 120
        B = m[2] / 2 - t2 * m[4] / 24 + t2 * t2 * m[6] / 720
    else:
        em, h = np.expm1(sigma), np.sin(0.5 * th)
        a, omb, c = (em + 1) * np.sin(th), 2 * h * h - em * np.cos(th), th * th + sigma * sigma
        A = (a * sigma + omb * th) / (th * c)
        B = (m[0] - (a * th - omb * sigma) / c) / (th * th)
    W = _hat3(w)
    return m[0] * np.eye(3) + A * W + B * (W @ W)


def sim3_exp(d):
    """The similarity exp(hat(d)) of a tangent d = (w, u, sigma)."""
    d = np.asarray(d, np.float64).reshape(7)
    w, sigma = d[:3], float(d[6])
    th = float(np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
    if th < SIM3_TH_W:
        t2 = th * th
        sa = 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42)); ca = 0.5 - t2 / 24 * (1 - t2 / 30 * (1 - t2 / 56))
    else:
        sa = np.sin(th) / th; ca = 2 * np.sin(0.5 * th) ** 2 / (th * th)
    W = _hat3(w)
    return _sim3_pack(np.exp(sigma), np.eye(3) + sa * W + ca * (W @ W), _sim3_v(w, sigma) @ d[3:6])


def sim3_log(S):
    """The tangent of a similarity, rotation angle in [0, pi): the inverse of sim3_exp."""
    s, R, t = _sim3(S)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.empty(4)                                   # (x, y, z, w), Eigen's conversion
    if tr > 0:
        r = np.sqrt(tr + 1.0); q[3] = 0.5 * r; r = 0.5 / r
        q[:3] = [(R[2, 1] - R[1, 2]) * r, (R[0, 2] - R[2, 0]) * r, (R[1, 0] - R[0, 1]) * r]
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        r = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0); q[i] = 0.5 * r; r = 0.5 / r
        q[3] = (R[k, j] - R[j, k]) * r; q[j] = (R[j, i] + R[i, j]) * r; q[k] = (R[k, i] + R[i, k]) * r
    if q[3] < 0:
        q = -q
    q = q / np.sqrt(q @ q)
    n = float(np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]))
    f = 2 / q[3] * (1 - (n / q[3]) ** 2 / 3) if n < SIM3_TH_LOG else 2 * np.arctan2(n, q[3]) / n
    w, sigma = f * q[:3], float(np.log(s))
    return np.concatenate([w, np.linalg.solve(_sim3_v(w, sigma), t), [sigma]])


def sim3_inverse(S):
    s, R, t = _sim3(S)
    return _sim3_pack(1.0 / s, R.T, -(R.T @ t) / s)


def sim3_compose(outer, inner):
    """x -> outer(inner(x))"""
    s1, R1, t1 = _sim3(outer); s2, R2, t2 = _sim3(inner)
    return _sim3_pack(s1 * s2, R1 @ R2, s1 * (R1 @ t2) + t1)


def track_vertices(poses, sim=None):
    """Pose-graph vertices [N, 13] of world -> camera poses [N, 3, 4].  sim = (s, R, t) of align_maps, X_a = s R X_b + t, takes a
    track of gauge B into gauge A: S_i = (1 / s, R_i R^T, t_i - R_i R^T t / s), so the camera frame keeps its own units."""
    T = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    s, R, t = (1.0, np.eye(3), np.zeros(3)) if sim is None else (float(sim[0]), np.asarray(sim[1], np.float64).reshape(3, 3), np.asarray(sim[2], np.float64).reshape(3))
    out = np.empty((len(T), 13))
    for i, P in enumerate(T):
        Rc = P[:, :3] @ R.T
        out[i] = _sim3_pack(1.0 / s, Rc, P[:, 3] - Rc @ t / s)
    return out


def odometry_edges(vertices):
    """The chain edges (i, i + 1) of a track: (edges [N - 1, 2] int32, meas [N - 1, 13]) with C = S_(i+1) S_i^-1."""
    V = np.asarray(vertices, np.float64).reshape(-1, 13)
    n = max(len(V) - 1, 0)
    edges = np.stack([np.arange(n), np.arange(n) + 1], axis=1).astype(np.int32)
    return edges, np.array([sim3_compose(V[i + 1], sim3_inverse(V[i])) for i in range(n)]).reshape(n, 13)


def loop_edge(S_i, S_j_observed):
    """The measurement C = S_j_observed S_i^-1 of an edge (i, j): where vertex j was observed to lie, as seen from vertex i."""
    return sim3_compose(S_j_observed, sim3_inverse(S_i))


def vertices_to_poses(vertices):
    """[N, 3, 4] world -> camera poses [R | t / s] of pose-graph vertices: the same camera centres, unit scale."""
    V = np.asarray(vertices, np.float64).reshape(-1, 13)
    return np.concatenate([V[:, 1:10].reshape(-1, 3, 3), (V[:, 10:13] / V[:, :1])[..., None]], axis=-1)


def correct_points(points, S_before, S_after):
    """Map points [n, 3] seen from a vertex that moved: X' = S_after^-1 S_before X."""
    s, R, t = _sim3(sim3_compose(sim3_inverse(S_after), S_before))
    return s * (np.asarray(points, np.float64).reshape(-1, 3) @ R.T) + t


def join_segments(segments, sims):
    """split_segments' list in ONE gauge, segment 0's.  sims[k - 1], for every later segment k, is the similarity that takes
    segment k's gauge to segment k - 1's — (scale, R, t) or a dict with those keys, as align_maps / estimate_similarity return for
    segment k's map against segment k - 1's — or None where the two maps could not be aligned.  Returns (joined, unconnected):
    joined = the segments connected to segment 0 through an unbroken run of similarities, as copies with poses_pnp and poses taken
    through the composed similarity (apply_similarity) and two more keys, `index` (its place in `segments`) and `sim` (the composed
    (scale, R, t) into segment 0's gauge); unconnected = the indices of the others, which stay in gauges of their own.  Pure."""
    segments = list(segments); sims = list(sims)
    if len(sims) != max(len(segments) - 1, 0):
        raise ValueError(f"{len(segments)} segments take {max(len(segments) - 1, 0)} similarities, got {len(sims)}")
    joined, unconnected = [], []
    total = (1.0, np.eye(3), np.zeros(3))
    for k, seg in enumerate(segments):
        if k > 0 and total is not None:
            s = sims[k - 1]
            if isinstance(s, dict):
                s = (s["scale"], s["R"], s["t"])
            total = None if s is None else compose_similarity(total, s)
        if total is None:
            unconnected.append(k)
            continue
        d = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in seg.items()}
        for key in ("poses_pnp", "poses"):
            if key in d:
                d[key] = apply_similarity(d[key], *total)
        d["index"] = k; d["sim"] = total
        joined.append(d)
    return joined, unconnected


STREAM_PAIR_KEYS = ("chi2", "n_corr", "n_inl", "status", "n_pts", "n_obs", "n_cam", "ba_iterations", "ba_trials")


def join_stream(outs):
    """The dicts the calls of one stream returned, in order (slam_stream, or slam_stream_restart) -> the whole flight's dict: what
    slam_chain, or slam_chain(restart=True) without `segments`, returns for all the pairs at once.  Pure: no GPU, no library.
    Per-pair arrays are concatenated; poses_pnp joins on the anchor rows (row 0 of a resumed call is the last row of the call
    before).  poses, and seg_poses of a restart stream, take the LATEST report of every frame: a call's own rows, then its seg_poses
    rows, then its carried rows — a carried frame that is the first camera of a segment (the frame of the pair that started it)
    reports to seg_poses, and to poses as well if it is frame 0; any other to poses.  With the restart keys the result has segment,
    cause, seg_poses_pnp, seg_poses and split_segments works on it unchanged.
    ValueError on what the library cannot produce: an anchor row of poses_pnp that differs between two calls, segment numbers that
    go backwards, a carried frame that is not earlier than its call's first frame."""
    outs = list(outs)
    if not outs:
        raise ValueError("join_stream takes at least one call")
    restart = "segment" in outs[0]
    if any(("segment" in o) != restart for o in outs):
        raise ValueError("the calls of one stream all have the restart keys or none has")
    out = {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in STREAM_PAIR_KEYS if k in outs[0]}
    pnp = [np.asarray(o["poses_pnp"], np.float64).reshape(-1, 3, 4) for o in outs]
    for c in range(1, len(outs)):
        if not np.array_equal(pnp[c][0], pnp[c - 1][-1]):
            raise ValueError(f"poses_pnp row 0 of call {c} is not the last row of call {c - 1}: these are not consecutive calls of one stream")
    out["poses_pnp"] = np.concatenate([pnp[0]] + [a[1:] for a in pnp[1:]])
    P = len(out["poses_pnp"]) - 1
    starts = np.zeros(P, bool)
    if restart:
        seg = np.concatenate([np.asarray(o["segment"]).ravel() for o in outs])
        last = -1
        for p, k in enumerate(seg):
            if k < 0:
                continue
            if k < last or k > last + 1:
                raise ValueError(f"pair {p} is in segment {int(k)} after segment {last}: segments are numbered in order of start along the stream")
            starts[p] = k != last
            last = int(k)
        out["segment"] = seg
        out["cause"] = np.concatenate([np.asarray(o["cause"]).ravel() for o in outs])
        out["seg_poses_pnp"] = np.concatenate([np.asarray(o["seg_poses_pnp"], np.float64).reshape(-1, 3, 4) for o in outs])
        seg_poses = np.concatenate([np.asarray(o["seg_poses"], np.float64).reshape(-1, 3, 4) for o in outs])
    poses = np.zeros((P + 1, 3, 4))
    at = 0
    for c, o in enumerate(outs):
        own = np.asarray(o["poses"], np.float64).reshape(-1, 3, 4)
        poses[at:at + len(own)] = own
        for f, T in zip(np.asarray(o["carried_frame"]).ravel(), np.asarray(o["carried_poses"], np.float64).reshape(-1, 3, 4)):
            f = int(f)
            if f < 0 or f >= at:
                raise ValueError(f"call {c} carries frame {f}, which is not earlier than its first frame {at}")
            if restart and starts[f]:
                seg_poses[f] = T
            if not (restart and starts[f]) or f == 0:
                poses[f] = T
        at += len(own) - 1
    out["poses"] = poses
    if restart:
        out["seg_poses"] = seg_poses
    return out


STATS_KEYS = ("total_sqerr", "mean_sqerr", "max_sqerr", "n_high", "obs_hist", "obs_matrix", "cam_frame")


def mean_sqerr(total_sqerr, n_obs):
    """show_map_statistics' mean (src/map.py:240-241): total / n_obs where there are observations, 0.0 elsewhere."""
    total, n = np.asarray(total_sqerr, np.float64), np.asarray(n_obs)
    return np.divide(total, n, out=np.zeros(total.shape), where=n > 0)


def join_stats(stats):
    """The slam_stats() dicts of the calls of one stream, in order -> the whole flight's rows: every key concatenated along the pair
    axis (a row is complete in itself; cam_frame already counts along the stream).  Calls in which the sequence was idle have no
    rows and add nothing.  For slam_streams: join_stats([fe.slam_stats(s) after each call]) per sequence s.  Pure: no GPU, no library."""
    stats = list(stats)
    if not stats:
        raise ValueError("join_stats takes at least one call")
    widths = {np.asarray(d["cam_frame"]).shape[1] for d in stats}
    if len(widths) != 1:
        raise ValueError(f"the calls of one stream all have the same max_cameras, got row widths {sorted(widths)}")
    return {k: np.concatenate([np.asarray(d[k]) for d in stats]) for k in STATS_KEYS}


def stream_slice(out, s):
    """Sequence s's part of the dict one slam_streams call returned, in the shape slam_stream_restart returns (copies): the
    per-pair arrays' rows seq_off[s] .. seq_off[s + 1] - 1, the pose rows seq_off[s] + s .. seq_off[s + 1] + s, its carried rows.
    A sequence that was idle in the call has no pairs and one pose row, its last frame's."""
    off = np.asarray(out["seq_off"]).ravel()
    s = int(s)
    if s < 0 or s >= len(off) - 1:
        raise ValueError(f"no sequence {s} in a call of {len(off) - 1}")
    a, b = int(off[s]), int(off[s + 1])
    d = {k: np.array(np.asarray(out[k])[a:b], copy=True) for k in STREAM_PAIR_KEYS + ("segment", "cause", "seg_poses_pnp", "seg_poses")}
    for k in ("poses_pnp", "poses"):
        d[k] = np.array(np.asarray(out[k])[a + s:b + s + 1], copy=True)
    d["carried_frame"] = np.array(out["carried_frame"][s], np.int32, copy=True)
    d["carried_poses"] = np.array(out["carried_poses"][s], np.float64, copy=True).reshape(-1, 3, 4)
    return d


def join_streams(outs):
    """The dicts the calls of one slam_streams stream returned, in order -> one whole-flight dict per sequence: join_stream over
    that sequence's slices of the calls in which it advanced (an idle call adds nothing to a flight).  Pure: no GPU, no library."""
    outs = list(outs)
    if not outs:
        raise ValueError("join_streams takes at least one call")
    S = len(np.asarray(outs[0]["seq_off"]).ravel()) - 1
    if any(len(np.asarray(o["seq_off"]).ravel()) - 1 != S for o in outs):
        raise ValueError("the calls of one stream all have the same number of sequences")
    joined = []
    for s in range(S):
        own = [stream_slice(o, s) for o in outs]
        joined.append(join_stream([d for d in own if len(d["status"]) > 0]))
    return joined


def split_flights(outs, took_seat):
    """The dicts the calls of one slam_streams stream with seats returned, in order, and per seat s the call indices took_seat[s]
    (increasing) at which a new flight took it -> per seat a list of flights, each the list of that flight's per-call
    stream_slice dicts, ready for join_stream.  A flight owns the calls from the one in which it took the seat up to the next
    flight's; calls in which the seat was idle — between two flights too — add nothing.  Pure: no GPU, no library."""
    outs = list(outs)
    if not outs:
        raise ValueError("split_flights takes at least one call")
    S = len(np.asarray(outs[0]["seq_off"]).ravel()) - 1
    if any(len(np.asarray(o["seq_off"]).ravel()) - 1 != S for o in outs):
        raise ValueError("the calls of one stream all have the same number of sequences")
    if len(took_seat) != S:
        raise ValueError(f"took_seat names {len(took_seat)} seats, the calls {S}")
    flights = []
    for s in range(S):
        starts = [int(c) for c in took_seat[s]]
        if any(b <= a for a, b in zip(starts, starts[1:])) or any(c < 0 or c >= len(outs) for c in starts):
            raise ValueError(f"seat {s}: the calls at which flights took it must be increasing call indices, got {starts}")
        own = [stream_slice(o, s) for o in outs]
        if any(len(own[c]["status"]) == 0 for c in starts):
            raise ValueError(f"seat {s}: a flight takes a seat in a call in which it advances, got {starts}")
        if any(len(d["status"]) > 0 for d in own[:starts[0] if starts else len(outs)]):
            raise ValueError(f"seat {s} advances before its first flight took it")
        flights.append([[d for d in own[a:b] if len(d["status"]) > 0] for a, b in zip(starts, starts[1:] + [len(outs)])])
    return flights


def chain_poses(R, t):
    """Compose relative poses x_{k+1} ~ R_k x_k + t_k into camera-to-world 4x4 matrices (unit-norm t: the
    scale of every step is unobservable, as in the reference's monocular front end)."""
    T = np.eye(4)
    out = [T.copy()]
    for Rk, tk in zip(R, t):
        step = np.eye(4)
        step[:3, :3] = Rk
        step[:3, 3] = np.asarray(tk).ravel()
        T = T @ np.linalg.inv(step)
        out.append(T.copy())
    return np.stack(out)
