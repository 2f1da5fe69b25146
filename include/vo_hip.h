/* vo_hip.h — C ABI of libvo_hip.so: the MI355X (gfx950) per-frame-pair visual-odometry front end.
 *
 * Drop-in boundary.  The reference (Samirez/Visual_odometry) is pure Python and reaches its
 * arithmetic through five cv2 calls; this library replaces exactly those calls with
 * hand-written HIP kernels.  Each entry point cites the reference call it stands in for
 * (paths relative to the reference repository root).  Host code binds it with ctypes
 * (visual_odometry_amd/_lib.py); no torch types, plain pointers and sizes only.
 *
 * Conventions: every function returns 0 on success, > 0 for a completed call with a warning
 * (VO_WARN_*), < 0 on error (VO_ERR_*); vo_last_error(ctx) gives the message.  All pointer
 * arguments are HOST memory owned by the caller unless a name ends in _dev.  One vo_ctx per
 * (thread, device); a ctx owns its device buffers and one HIP stream; calls are synchronous.
 */
#ifndef VO_HIP_H
#define VO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VO_MAX_LEVELS 16

#define VO_OK                 0
#define VO_WARN_CAPACITY      1   /* a candidate / keypoint list hit its capacity and was truncated */
#define VO_ERR_INVALID       -1
#define VO_ERR_HIP           -2
#define VO_ERR_TOO_FEW       -3   /* fewer than 5 correspondences (cv2.findEssentialMat returns None) */
#define VO_ERR_NO_MODEL      -4   /* RANSAC found no model with > 4 inliers */
#define VO_ERR_NOT_CONFIGURED -5
#define VO_ERR_UNSUPPORTED    -7   /* a branch of the cv2 call that is not built (INTER_AREA enlargement) */
#define VO_ERR_AMBIGUOUS      -6   /* exactly 5 correspondences: findEssentialMat stacks up to 10 solutions, which
                                     cv2.recoverPose (and the reference) cannot consume */

typedef struct vo_ctx vo_ctx;

/* cv2.ORB_create(...) parameters — src/image_and_keypoints.py:8 (all defaults), overridden by
 * BASELINE configs (nfeatures 500/2000/4000, nlevels 8/4). */
typedef struct {
    int32_t nfeatures;       /* 500  */
    float   scale_factor;    /* 1.2f */
    int32_t nlevels;         /* 8    */
    int32_t edge_threshold;  /* 31   */
    int32_t first_level;     /* 0  (only 0 supported) */
    int32_t wta_k;           /* 2  (only 2 supported) */
    int32_t score_type;      /* 0 = HARRIS_SCORE, 1 = FAST_SCORE */
    int32_t patch_size;      /* 31 (only 31 supported) */
    int32_t fast_threshold;  /* 20 */
} vo_orb_params;

/* ------------------------------------------------------------------ lifetime */
int         vo_create(int device_id, vo_ctx** out);
void        vo_destroy(vo_ctx* ctx);
const char* vo_last_error(const vo_ctx* ctx);
int         vo_version(void);

/* ------------------------------------------------------------------ single-call operators */

/* IMAGE LAYOUT CONTRACT — holds for every entry point that takes row_stride, frame_stride or dst_stride (all in bytes):
 * vo_orb_detect_and_compute, vo_stage_pyramid / _fast_scores / _blur, vo_frames_upload[_async], vo_frames_upload_color,
 * vo_frames_ingest, vo_sift_detect_and_compute, vo_resize_linear, vo_resize_area.  A cv::Mat ROI (data, step) or a decoder's
 * padded frame is passed as it is.
 *   Source image: h rows of w * channels bytes, row y at img + y * row_stride.  The library reads only inside
 *     [img, img + (h - 1) * row_stride + w * channels): nothing after the last row's last pixel, nothing before img.
 *   Source frame stack: frame f at frames + f * frame_stride; for F frames the span is
 *     (F - 1) * frame_stride + (h - 1) * row_stride + w * channels bytes.  The bytes between rows and between frames may be read
 *     (a padded stack crosses the bus in one copy) but never influence a result.
 *   Destination (vo_resize_*): dh rows at dst_stride; the library writes only the dw * channels bytes of each row — never the
 *     bytes between the rows, never anything after the last row's last pixel.
 *   Alignment: none is required of img, dst or any stride; rows may start on any byte.
 *   row_stride < w * channels and dst_stride < dw * channels are refused (VO_ERR_INVALID).
 *   frame_stride: vo_frames_upload[_async] take any value, 0 included (every slot then receives frame 0; the single-image calls
 *     pass 0 themselves); vo_frames_upload_color (channels 3, 4) and vo_frames_ingest require
 *     frame_stride >= (h - 1) * row_stride + w * channels — a frame may begin where the previous one's last row ends, which a
 *     stack of ROI views needs — and refuse less (VO_ERR_INVALID).
 * Tight strides (row_stride == w * channels, frame_stride == h * row_stride, dst_stride == dw * channels) are the fast path: one
 * linear copy each way. */

/* detector.detectAndCompute(image, None) — src/frame_generator.py:25-26, src/image_and_keypoints.py:46.
 * img: h x w x channels u8 (1 = gray, 3 = BGR, 4 = BGRA), laid out as the contract above says.  Outputs hold up to cap keypoints in
 * canonical order (octave, y, x); desc is cap x 32 bytes. */
int vo_orb_detect_and_compute(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                              const vo_orb_params* params,
                              float* kp_xy, float* kp_size, float* kp_angle, float* kp_response,
                              int32_t* kp_octave, uint8_t* desc, int cap, int32_t* n_out);

/* Which kernel computes the Hamming nearest neighbours (same results, bit for bit): 2 = block-scaled FP4 MFMA over
 * e2m1 +1/-1 descriptors (default; sets of 8192 rows or more fall back to 0), 0 = int8 MFMA over +127/-127 bytes
 * (16129 rows or more fall back to 1), 1 = XOR + popcount on the packed descriptors (the formulation BASELINE.json's
 * north_star names).  The detector writes the operand image of the matrix-core kernel selected at that time and the
 * matcher reads that image in its own format, so a change between 0 and 2 takes effect with the next detection. */
int vo_set_matcher_kernel(vo_ctx* ctx, int kind);

/* Order of the keypoint list (and therefore of every keypoint / match index): 0 (default) = canonical (octave, y, x);
 * 1 = cv2's — the permutation cv::KeyPointsFilter::retainBest's std::nth_element + std::partition leave behind, which
 * is what makes `Feature.feature_id = (frame.id, idx)` (src/frame_generator.py:34-36) and DMatch.queryIdx / trainIdx
 * (src/image_pair.py:243-252) the same numbers cv2 produces.  Same keypoint set, responses and descriptors either way;
 * mode 1 costs an extra pass over every FAST corner of the frame.  Takes effect at the next detection. */
int vo_set_keypoint_order(vo_ctx* ctx, int kind);

/* How the five-point solver inside findEssentialMat finds the roots of its degree-10 polynomial (cv::solvePoly,
 * Durand-Kerner): 1 = OpenCV's fixed 300 sweeps, operation for operation; 0 (default) = the same sweeps, stopped per
 * sample once every correction is rounding noise (~20 sweeps; identical inlier masks, [R|t] equal to ~1e-12 on the
 * test sets, 10x less RANSAC time).  Applies to vo_find_essential_ransac, vo_stage_five_point and vo_pairs_run. */
int vo_set_poly_solver(vo_ctx* ctx, int kind);

/* How vo_solve_pnp_ransac(_batch) computes the final pose from the consensus set (cv2.solvePnPRansac ends with
 * solvePnP(inliers, SOLVEPNP_ITERATIVE, useExtrinsicGuess = false) — src/visual_slam.py:231-235): 1 (default) = as
 * OpenCV 4.7 does: DLT start (homography start for a planar structure; the RANSAC model itself when only 5 non-planar
 * inliers exist), then CvLevMarq on (rvec, tvec) for at most 20 iterations with the FLT_EPSILON step rule;
 * 0 = fast mode: the same reprojection cost minimised from the best RANSAC model to tight convergence (agrees with
 * mode 1 to ~1e-7 wherever both converge to the same minimum, ~25 % less kernel time). */
int vo_set_pnp_refine(vo_ctx* ctx, int kind);

/* self.matcher.match(d1, d2) for cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=...) —
 * src/image_pair.py:234-236, matcher built at src/visual_slam.py:18 / src/image_and_keypoints.py:9.
 * cross_check: 0 = nearest neighbour (crossCheck=False); 2 = crossCheck=True as OpenCV 4.x computes it: strict
 * mutual nearest neighbours, lowest index winning ties in both directions (core/batch_distance.cpp keeps train i
 * for its nearest query idx only if `sidx[idx] == i`); 1 = the older rule without that forward test (every train
 * row votes for its nearest query, a query keeps its closest voter) — [unverified] which releases used it.
 * Outputs (capacity nq) are ordered by ascending queryIdx. */
int vo_match_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int cross_check,
                     int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out);

/* self.matcher.match(d1, d2) for cv2.BFMatcher(cv2.NORM_L2, crossCheck=...) on float32 descriptors (nq x dim, nt x dim) —
 * the reference's live matcher (src/visual_slam.py:19, SIFT rows: dim 128; also src/feature_detection.py:37-39).
 * cross_check and the outputs as vo_match_hamming; distance = sqrt(sum of squared differences), float32, summed in
 * cv::hal::normL2Sqr_'s order. */
int vo_match_l2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int cross_check,
                int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out);

/* matcher.knnMatch(d1, d2, k=2) + `m.distance < ratio * n.distance` — src/feature_detection.py:20-26. */
int vo_knn2_ratio_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio,
                          int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out);
/* matcher.knnMatch(d1, d2, k=2) itself — src/feature_detection.py:21 (and :90): BOTH neighbours of every query row, as
 * batchDistance's K = 2 insertion leaves them (ascending scan of the train rows, strict `<`: equal distances keep their
 * train order).  idx / dist: nq x 2; a neighbour that does not exist (fewer than two train rows) is -1 / FLT_MAX — cv2
 * leaves it out of the row's list.  vo_knn2_l2: the same for cv2.BFMatcher(cv2.NORM_L2) on float rows (the script runs its
 * ratio rule on SIFT descriptors, :7-8); vo_knn2_ratio_l2: knnMatch + the rule of :24-26 in one call. */
int vo_knn2_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, float* dist);
int vo_knn2_l2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int32_t* idx, float* dist);
int vo_knn2_ratio_l2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, double ratio,
                     int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out);

/* cv2.findEssentialMat(p1, p2, K, cv2.FM_RANSAC, prob, thresh) — src/image_pair.py:280-286.
 * p1, p2: M x 2 float64 pixel coordinates; K: 3x3 row-major; seed: OpenCV's RNG seed 2^64-1.
 * E: 9 doubles (M == 5: up to 10 stacked models, n_models tells how many); mask: M bytes (0/1). */
int vo_find_essential_ransac(vo_ctx* ctx, const double* p1, const double* p2, int M, const double* K,
                             double prob, double thresh_px, int max_iters, uint64_t seed,
                             double* E, uint8_t* mask, int32_t* n_inl, int32_t* n_models);

/* cv2.recoverPose(E, p1, p2, K) — src/image_pair.py:304-308 (distanceThresh 50).
 * R: 9, t: 3 (unit norm), mask: M bytes (0/255, may be NULL). */
int vo_recover_pose(vo_ctx* ctx, const double* E, const double* p1, const double* p2, int M, const double* K,
                    double dist_thresh, double* R, double* t, uint8_t* mask, int32_t* n_good);

/* cv2.triangulatePoints(P1, P2, x1, x2) — src/image_pair.py:332-336. x1, x2: 2 x M; X: 4 x M
 * (NOT normalised by w; the caller divides, as src/image_pair.py:339 does). */
int vo_triangulate(vo_ctx* ctx, const double* P1, const double* P2, const double* x1, const double* x2,
                   int M, double* X);

/* cv2.computeCorrespondEpilines(points, whichImage, F) — src/feature_detection.py:118-125.  OpenCV 4.7's behaviour, restated
 * from its source as remembered; parity with a cv2 build is unpinned, like the rest of this library.
 * points: N x 2 of point_type 0 (f64), 1 (f32) or 2 (i32); F: 9 doubles, used as given for which_image 1 and transposed for 2.
 * Per point, in f64, left to right, one rounding per operation: a = f0 x + f1 y + f2, b = f3 x + f4 y + f5,
 * c = f6 x + f7 y + f8; nu = a a + b b; nu = nu ? 1 / sqrt(nu) : 1; line = (a nu, b nu, c nu).
 * lines: N x 3 of depth max(input depth, f32): f64 for f64 points, f32 (each value cast once at the end) for f32 and i32
 * points.  N = 0 is legal.  Three-column (homogeneous) points are not built. */
int vo_correspond_epilines(vo_ctx* ctx, const void* points, int N, int point_type, int which_image, const double* F, void* lines);

/* The symmetric epipolar distances of src/feature_detection.py:127-140 and their statistics for the B pairs the most recent
 * vo_pairs_run left on the device (res[p].E and the pixel inliers), one workgroup per pair, no host round trip.
 *   F = K^-T E K^-1, with K^-1 as the pair path normalises pixels: ifx = 1 / K[0], ify = 1 / K[4], bx = -K[2] ifx,
 *   by = -K[5] ify; G = E K^-1 (G[r][2] = E[r][0] bx + E[r][1] by + E[r][2]); F = K^-T G (F[2][c] = bx G[0][c] + by G[1][c]
 *   + G[2][c]).  K must be [fx 0 cx; 0 fy cy; 0 0 1] with finite entries and fx, fy != 0: skew, another last row or a zero
 *   focal length is VO_ERR_UNSUPPORTED (the pair path reads only those four entries).
 *   [deviation] The reference script passes its ESSENTIAL matrix together with PIXEL points to computeCorrespondEpilines,
 *   which measures nothing; here the lines are those of the pixel fundamental matrix, so the distances are in pixels.
 *   Per E inlier k, in match order: d_k = |l1_k . (x2_k, 1)| + |l2_k . (x1_k, 1)|, l1 = epiline of x1 in image 2
 *   (which_image 1), l2 = epiline of x2 in image 1 (which_image 2), normalised as vo_correspond_epilines does, each dot
 *   product as l0 x + l1 y + l2.
 *   mean[p], std[p] (population, two passes, as np.std) and max[p] are SEQUENTIAL sums over k in match order starting from
 *   0.0 (the rule of vo_slam_stats' total_sqerr), so the bytes are defined by the data; numpy's pairwise np.mean / np.std
 *   can differ from them in the last bits.
 * n[p]: the pair's inliers; a pair whose status is not VO_OK or that has no inliers gives n = 0 and zeros; one inlier
 * gives std = 0.  dist: NULL, or B x kp_cap doubles (vo_batch_kp_capacity): row p holds d_0 .. d_{n[p]-1}, then zeros.
 * Refused as vo_tracks_pnp_batch refuses: VO_ERR_NOT_CONFIGURED before vo_batch_configure, VO_ERR_INVALID when B is not
 * the most recent run's pair count (a configure call in between clears it).  The run need not have triangulated. */
int vo_pairs_epipolar(vo_ctx* ctx, int B, const double* K, int32_t* n, double* mean, double* std_dev, double* max_dist, double* dist);

/* cv2.undistortPoints(src, K, dist, R, P) with its default termination — the lens model the reference names and never wires
 * up: src/image_and_keypoints.py:21-25 stores the drone camera's five coefficients (k1, k2, p1, p2, k3) in self.distCoeffs and
 * nothing reads them.  OpenCV 4.7's undistort.dispatch.cpp, restated from its source as remembered.
 * [deviations] five fixed-point iterations, always (cv2's default criteria; no epsilon-terminated form); no thin-prism and no
 *   tilt terms (ndist 12 and 14: VO_ERR_UNSUPPORTED); parity with a cv2 build is unpinned, like the rest of this library — the
 *   checker is the numpy restatement tests/undistort_reference.py, and the contract is byte equality with it.
 * dist: ndist doubles in cv2's order k1 k2 p1 p2 [k3 [k4 k5 k6]]; ndist 4, 5 or 8 (absent coefficients are zero and go through
 * the same expressions); any other count, 0 included, and dist == NULL: VO_ERR_INVALID (no distortion = four zeros).  K: 3x3 row-major, read as fx = K[0], cx = K[2],
 * fy = K[4], cy = K[5]; fx == 0 or fy == 0: VO_ERR_INVALID.  R, P: 9 doubles each (3x3 row-major; of a 3x4 P its left 3x3)
 * or NULL = identity.  RR = P R is formed on the host, RR[i][j] = P[i][0] R[0][j] + P[i][1] R[1][j] + P[i][2] R[2][j].
 * Per point (u, v), in f64, left to right, one rounding per operation:
 *   ifx = 1 / fx, ify = 1 / fy;  x = (u - cx) ifx, y = (v - cy) ify;  x0 = x, y0 = y
 *   five times:  r2 = x x + y y
 *                icdist = (1 + ((k6 r2 + k5) r2 + k4) r2) / (1 + ((k3 r2 + k2) r2 + k1) r2)
 *                if (icdist < 0) { x = x0, y = y0; stop }            (cv2's fallback outside the model's valid range)
 *                dx = ((2 p1) x) y + p2 (r2 + (2 x) x),  dy = p1 (r2 + (2 y) y) + ((2 p2) x) y
 *                x = (x0 - dx) icdist,  y = (y0 - dy) icdist
 *   xx = RR0 x + RR1 y + RR2, yy = RR3 x + RR4 y + RR5, ww = 1 / (RR6 x + RR7 y + RR8);  out = (xx ww, yy ww)
 * All-zero coefficients give the bytes of plain normalisation; NaN / Inf input propagates through its own row only.
 * points: N x 2 of point_type 0 (f64) or 1 (f32), as vo_correspond_epilines names them; out: N x 2 of the same type, an f32 value
 * being the f64 result rounded once.  N = 0 returns VO_OK and touches nothing. */
int vo_undistort_points(vo_ctx* ctx, const void* points, int N, int point_type, const double K[9], const double* dist, int ndist,
                        const double* R /*9 or NULL*/, const double* P /*9 or NULL*/, void* out);
/* The resident form: the same arithmetic with R = I and P = K on the keypoint positions of slots [first_slot, first_slot + F) of the
 * live batch configuration (ORB or SIFT), in place: kp_xy = float32(undistort(double(kp_xy))), for the slot's kp_count keypoints
 * as the device holds the count — no host round trip.  Every kernel after detection takes pixel positions from that array only, so
 * the pair path, the chain and the map step then run on ideal pixels, unchanged.
 * K is the camera matrix of the frames AS THEY SIT IN THE SLOTS, i.e. after any resize (vo_frames_ingest[_jpeg] scale fx, fy, cx,
 * cy with the image); the coefficients are dimensionless — they act on normalised coordinates — and survive a resize unchanged.
 * Enqueued on the context's stream: behind vo_frames_detect_async, before the next vo_pairs_run; returns after the stream's work,
 * as vo_frames_detect does.  Only kp_xy of those slots changes: descriptors, angles, sizes, responses, octaves, counts and flags
 * keep their bytes, as does everything of every other slot.  The detected positions are not kept: read them before the call.
 * The context marks an undistorted slot (host side): a call whose range holds a marked slot is refused (VO_ERR_INVALID, nothing
 * changed) — also for the anchor slot of a live vo_slam_stream*, undistorted when it was a new frame.  Whatever gives a slot new
 * keypoints clears its mark: vo_frames_detect[_async], vo_frames_upload*, vo_frames_ingest[_jpeg], vo_stage_orb_rows,
 * vo_stage_sift_rows; a configure call clears all.  VO_ERR_NOT_CONFIGURED before a batch configuration; VO_ERR_INVALID for a
 * slot range out of bounds; ndist, K as vo_undistort_points.  Profiling stage "undistort_points". */
int vo_frames_undistort(vo_ctx* ctx, int first_slot, int F, const double K[9], const double* dist, int ndist);

/* ------------------------------------------------------------------ stage outputs (parity tests) */
/* size in bytes of the packed outputs below (sum over levels of w_l * h_l); < 0 for invalid parameters */
int64_t vo_packed_pyramid_bytes(int h, int w, const vo_orb_params* params);
/* gray + INTER_LINEAR_EXACT pyramid, levels packed tightly one after the other (img: see IMAGE LAYOUT CONTRACT; out_packed is dense) */
int vo_stage_pyramid(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                     const vo_orb_params* params, uint8_t* out_packed);
/* per level: FAST-9/16 score after 3x3 NMS (dense, packed like the pyramid) and the 7x7 blur */
int vo_stage_fast_scores(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                         const vo_orb_params* params, uint8_t* out_packed);
int vo_stage_blur(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                  const vo_orb_params* params, uint8_t* out_packed);
/* cv::KeyPointsFilter::retainBest(keypoints, n_points) on a list of n responses: order (capacity n) receives the kept
 * ORIGINAL indices in the order cv2 leaves them in */
int vo_stage_retain_best(vo_ctx* ctx, const float* response, int n, int n_points, int32_t* order, int32_t* n_out);
/* EMEstimatorCallback::runKernel on one 5-point sample of normalised coordinates */
int vo_stage_five_point(vo_ctx* ctx, const double* x1, const double* x2, double* E /*10x9*/, int32_t* n_models);

/* ------------------------------------------------------------------ batched, device-resident path
 * The throughput path: frames live in HBM, every stage runs batch-major on the ctx stream,
 * nothing returns to the host between stages.  Mirrors the per-pair order of
 * src/visual_slam.py:294-298 (match_features -> determine_essential_matrix ->
 * estimate_camera_movement -> reconstruct_3d_points). */
typedef struct {
    int32_t match_mode;     /* 0 = BFMatcher(crossCheck=True).match (strict mutual NN), 1 = knnMatch(k=2) + ratio,
                               2 = the legacy cross-check rule (vo_match_hamming cross_check = 1),
                               3 = BFMatcher(crossCheck=False).match: every query's nearest train row, not one-to-one */
    double  ratio;          /* ratio for match_mode 1 */
    double  ransac_prob;    /* 0.99  src/image_pair.py:278 */
    double  ransac_thresh;  /* 1.0   src/image_pair.py:279 */
    int32_t ransac_max_iters; /* 1000 (cv2 default) */
    uint64_t ransac_seed;   /* 0xFFFFFFFFFFFFFFFF */
    double  pose_dist_thresh; /* 50 */
    int32_t want_points;    /* also triangulate (reconstruct_3d_points) */
} vo_pair_opts;

typedef struct {
    int32_t n_kp1, n_kp2, n_match, n_inl, n_good, status, ransac_iters, reserved;
    double  R[9], t[3], E[9];
} vo_pair_result;

/* (re)allocate device buffers for frames of h x w, up to max_frames resident frames and
 * max_pairs pairs per vo_pair_batch call */
int vo_batch_configure(vo_ctx* ctx, int h, int w, const vo_orb_params* params, int max_frames, int max_pairs);
/* copy F gray frames (u8, row_stride / frame_stride in bytes: IMAGE LAYOUT CONTRACT, any frame_stride) into slots [first_slot, first_slot+F) */
int vo_frames_upload(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot);
/* Same, enqueue only: `frames` should be page-locked (vo_host_alloc) and must stay unchanged until vo_sync(ctx).
 * Streaming drivers alternate two contexts: one's upload (DMA) runs beside the other's kernels. */
int vo_frames_upload_async(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot);
/* same for BGR (channels 3) / BGRA (4) frames: converted to gray on the device (cv2's BGR2GRAY, as ORB does); strides per the
 * IMAGE LAYOUT CONTRACT, frame_stride >= (h - 1) * row_stride + w * channels */
int vo_frames_upload_color(vo_ctx* ctx, const uint8_t* frames, int F, int channels, int row_stride,
                           int64_t frame_stride, int first_slot);
/* detect + describe slots [first_slot, first_slot+F); results stay on the device */
int vo_frames_detect(vo_ctx* ctx, int first_slot, int F);
/* same, but only enqueued on the ctx stream (the next synchronous call, e.g. vo_pairs_run, waits for it) */
int vo_frames_detect_async(vo_ctx* ctx, int first_slot, int F);
/* keypoint / match capacity per frame of the current configuration (row length of X in vo_pairs_run) */
int vo_batch_kp_capacity(vo_ctx* ctx);
/* page-locked host memory for result buffers (full-rate D2H copies); plain malloc'ed memory also works */
int  vo_host_alloc(size_t bytes, void** out);
void vo_host_free(void* p);
/* download one slot's keypoints / descriptors (capacity cap) */
int vo_frame_features(vo_ctx* ctx, int slot, float* kp_xy, float* kp_size, float* kp_angle, float* kp_response,
                      int32_t* kp_octave, uint8_t* desc, int cap, int32_t* n_out);
/* run match + E-RANSAC + pose (+ triangulation) for B pairs of already detected slots.
 * pair_slots: B x 2 int32.  results: B entries.  X (optional, may be NULL): B x 4 x x_cap
 * doubles, w normalised to 1; X is valid only for VO_OK pairs, in their first n_inl columns (the inliers in match order).
 * A pair's record is zeroed before the run; n_kp1, n_kp2 and n_match are always written.  What else a pair holds, by status
 * (tests/test_gpu_pairs_chosen.py asserts it field for field):
 *   VO_OK             every field; a pair of exactly 5 matches whose five-point solve has ONE solution is such a pair
 *                     (n_inl = 5, ransac_iters = 0, recoverPose and X on the five points)
 *   VO_ERR_TOO_FEW    n_match < 5: nothing else; n_inl, n_good, ransac_iters, E, R, t stay 0
 *   VO_ERR_NO_MODEL   ransac_iters (the whole budget max(ransac_max_iters, 1) when n_match > 5; 0 for n_match == 5); the rest stays 0
 *   VO_ERR_AMBIGUOUS  n_match == 5 with several stacked solutions: n_inl = 5, E = the first of them, n_good = 0, R and t stay 0
 * vo_pair_matches' inlier mask has no byte set for TOO_FEW and NO_MODEL pairs and all five set for an AMBIGUOUS one. */
int vo_pairs_run(vo_ctx* ctx, const int32_t* pair_slots, int B, const double* K, const vo_pair_opts* opts,
                 vo_pair_result* results, double* X, int32_t x_cap);
/* enqueue-only form: results / X must be page-locked (vo_host_alloc), X needs x_cap == vo_batch_kp_capacity();
 * they are valid after vo_sync(ctx).  Two contexts on one GPU can overlap one's detection with the other's
 * latency-bound RANSAC / pose kernels. */
int vo_pairs_run_async(vo_ctx* ctx, const int32_t* pair_slots, int B, const double* K, const vo_pair_opts* opts,
                       vo_pair_result* results, double* X, int32_t x_cap);
/* The synchronous forms (vo_frames_detect, vo_pairs_run) return VO_WARN_CAPACITY (> 0, results valid) when a keypoint list of an
 * involved slot hit its capacity: the batched SIFT path cuts such a frame at kp_cap in cv2's list order — x ascending, i.e. the
 * right edge of the image goes first — so E-RANSAC would run on a one-sided set; raise kp_cap.  The asynchronous forms cannot
 * know: vo_frame_features[_sift] reports the flag per slot.
 * SIFT: vo_pairs_run returns VO_ERR_INVALID when a slot of the pair list holds a descriptor row with |row|^2 > 2^20 (the bound
 * under which the integer matcher's order is cv2's; SIFT's normalisation gives ~2^18).  Like the capacity warning the error is
 * reported AFTER the run — the results of the other pairs are in `results`, those of a pair with such a slot are not to be
 * used — and the asynchronous form cannot know: vo_frame_features_sift reports the slot. */
int vo_sync(vo_ctx* ctx);
/* Orders ctx's next enqueued work after `other`'s most recent vo_frames_detect_async (same device).  Chaining the
 * detections of two contexts keeps them out of phase: one's RANSAC / pose always runs beside the other's ORB. */
int vo_detect_after(vo_ctx* ctx, vo_ctx* other);
/* per-pair match list of the last vo_pairs_run (capacity cap each).  A configure call (vo_batch_configure[_sift]) forgets
 * that run: every pair index is then refused (VO_ERR_INVALID), as on a fresh context. */
int vo_pair_matches(vo_ctx* ctx, int pair, int32_t* qidx, int32_t* tidx, float* dist, uint8_t* inlier_mask,
                    int cap, int32_t* n_out);

/* ------------------------------------------------------------------ multi-GPU: the trajectory gather
 * One process per GPU, every rank runs its own block of independent pairs (visual_odometry_amd/sharding.py); the only
 * exchange is ONE all-gather of the per-pair records at the end of a batch: VO_RECORD_DOUBLES float64 per pair =
 * R (9, row-major), t (3), n_kp1, n_match, n_inl (or the negative status of a failed pair), n_good.  RCCL is bound at
 * run time.  vo_comm_unique_id on rank 0, hand the 128 bytes to every rank by any host channel, vo_comm_init on all. */
#define VO_COMM_ID_BYTES 128
#define VO_RECORD_DOUBLES 16
int vo_comm_unique_id(uint8_t id[VO_COMM_ID_BYTES]);
int vo_comm_init(vo_ctx* ctx, const uint8_t id[VO_COMM_ID_BYTES], int rank, int world);
int vo_comm_destroy(vo_ctx* ctx);
/* One communicator per PROCESS: further contexts of the same GPU (the chunk pipeline alternates over several) join the
 * one `owner` created instead of creating their own.  A collective runs on the calling context's stream, after an event wait
 * for the collective submitted before it (by whichever context): the process's collectives execute one at a time in host
 * submit order (the same order on every rank).  vo_comm_destroy drops a context's reference; the last one destroys
 * the communicator.  vo_comm_info: ncclCommCount and this process's rank (1 and 0 without a communicator). */
int vo_comm_share(vo_ctx* ctx, vo_ctx* owner);
int vo_comm_info(vo_ctx* ctx, int32_t* n_ranks, int32_t* rank);
/* Packs the records of the first B pairs of the most recent vo_pairs_run[_async] on the device and all-gathers them
 * over RCCL, ordered after the ctx stream's work (every rank must pass the same B; pad short blocks).  gathered (host, page-locked for
 * the asynchronous form, world * B * VO_RECORD_DOUBLES doubles, rank-major) is valid after the call (wait != 0) or
 * after the next vo_sync(ctx).  Without vo_comm_init (single process) it degenerates to the local records. */
int vo_pairs_gather(vo_ctx* ctx, int B, double* gathered, int wait);
/* Rows at and beyond the pair count of that run (a short or empty last block, or every row after a configure call, which
 * forgets the run) arrive as zeros with VO_ERR_NOT_CONFIGURED in the n_inl column.  vo_comm_allgather_f64: synchronous all-gather of n <= 4096 host doubles per rank over the same communicator
 * (recv: world * n, rank-major) — a launcher's barrier and timing reduction without another communication library; without
 * a communicator it copies send to recv. */
int vo_comm_allgather_f64(vo_ctx* ctx, const double* send, int n, double* recv);

/* ------------------------------------------------------------------ "next" row
 * Map.remove_observations_with_reprojection_errors_above_threshold / calculate_reprojection_error —
 * src/map.py:46-94.  poses: ncam x 16 (row-major 4x4, TrackedCamera.pose()), points: npt x 3, observation i =
 * (obs_cam[i], obs_pt[i], obs_xy[2i..]) as INDICES into those arrays.  sqerr[i] = squared pixel error,
 * keep[i] = sqerr < threshold (the reference's default threshold is 100). */
int vo_reprojection_filter(vo_ctx* ctx, const double* poses, int ncam, const double* points, int npt,
                           const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs,
                           const double* K, double threshold, double* sqerr, uint8_t* keep);

/* cv2.solvePnPRansac(objectPoints, imagePoints, K, zeros(4)) with its default arguments (iterationsCount 100,
 * reprojectionError 8.0, confidence 0.99, SOLVEPNP_ITERATIVE) — src/visual_slam.py:231-235.
 * obj n x 3, img n x 2 (float64, row-major); rvec / tvec as cv2 returns them; mask[n] = 1 for inliers (cv2 returns
 * their indices).  n == 4 takes cv2's P3P branch (all four points inliers).  VO_ERR_TOO_FEW: n < 4 (cv2 asserts);
 * VO_ERR_NO_MODEL = retval False.  The final pose restates cv2's solvePnP(SOLVEPNP_ITERATIVE) (CvLevMarq) and is tested
 * against oracle/voo_pnp.c only: cv2 takes its SVDs from LAPACK and its sums in build-dependent order, so agreement with a cv2
 * wheel is to tolerance (tests/test_cv2_crosscheck.py states it where cv2 exists), never claimed bit for bit. */
int vo_solve_pnp_ransac(vo_ctx* ctx, const double* obj, const double* img, int n, const double K[9], int iterations,
                        double reproj_err, double confidence, uint64_t seed, double rvec[3], double tvec[3],
                        uint8_t* mask, int32_t* n_inl);
/* B independent problems in one launch (one workgroup each): problem b owns points offsets[b] .. offsets[b+1];
 * rvec / tvec are B x 3, mask has offsets[B] bytes, n_inl and status B ints (status[b] as the single call returns). */
int vo_solve_pnp_ransac_batch(vo_ctx* ctx, const double* obj, const double* img, const int32_t* offsets, int B,
                              const double K[9], int iterations, double reproj_err, double confidence, uint64_t seed,
                              double* rvec, double* tvec, uint8_t* mask, int32_t* n_inl, int32_t* status);
/* cv2.Rodrigues (src/visual_slam.py:243): in_is_matrix = 0: 3-vector -> 3x3 (row-major); 1: 3x3 -> 3-vector. */
int vo_rodrigues(vo_ctx* ctx, const double* in, int in_is_matrix, double* out);

/* cv2.resize(img, dim) with the default INTER_LINEAR, 8-bit, 1 / 3 / 4 channels — src/visual_slam.py:346-352
 * (cv2.imread's JPEG decode stays on the host).  Host image in, host image out; src and dst may be strided
 * views (IMAGE LAYOUT CONTRACT): the padding of dst is never written. */
int vo_resize_linear(vo_ctx* ctx, const uint8_t* src, int sh, int sw, int channels, int row_stride,
                     uint8_t* dst, int dh, int dw, int dst_stride);
/* cv2.resize(img, dim, interpolation=cv2.INTER_AREA) for an image that shrinks on both axes —
 * src/image_and_keypoints.py:42 (ImageAndKeypoints.set_image).  VO_ERR_UNSUPPORTED: enlargement.  Layout as vo_resize_linear. */
int vo_resize_area(vo_ctx* ctx, const uint8_t* src, int sh, int sw, int channels, int row_stride,
                   uint8_t* dst, int dh, int dw, int dst_stride);
/* cv2.SIFT_create(...).detectAndCompute(img, None) — the reference's LIVE detector, /root/reference/src/visual_slam.py:17
 * (FrameGenerator.make_frame, src/frame_generator.py:25-26); its descriptors go to vo_match_l2 (visual_slam.py:19).
 * OpenCV 4.7's sift.dispatch.cpp / sift.simd.hpp stage for stage: doubled base image, Gaussian and DoG pyramids, scale-space
 * extrema with sub-pixel refinement, contrast and edge tests, orientation histograms, 4 x 4 x 8 descriptors (float, values
 * 0..255), keypoints in removeDuplicatedSorted's order, octave packed as cv2 packs it.  nfeatures > 0 applies
 * KeyPointsFilter::retainBest (libstdc++'s nth_element + partition, ties kept) as cv2 does.  VO_WARN_CAPACITY: more than `cap` keypoints (n_out = the number found).
 * Keypoints and descriptors are bit-identical to the ORACLE (oracle/voo_sift.c: the scalar code paths of sift.simd.hpp, one rounding
 * per operation); a cv2 wheel accumulates the descriptor norm in SIMD lanes, so its uint8 bins can differ by +-1 where value * scale
 * lands near .5 — parity with cv2 itself is unpinned (tests/test_cv2_crosscheck.py carries the tolerance for machines that have cv2).
 * img / row_stride: IMAGE LAYOUT CONTRACT (above vo_orb_detect_and_compute). */
typedef struct {
    int32_t nfeatures;            /* 0 = keep every keypoint */
    int32_t n_octave_layers;      /* 3 */
    double  contrast_threshold;   /* 0.04 */
    double  edge_threshold;       /* 10 */
    double  sigma;                /* 1.6 */
} vo_sift_params;
int vo_sift_detect_and_compute(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride, const vo_sift_params* params,
                               float* kp_xy /*cap x 2*/, float* kp_size, float* kp_angle, float* kp_response, int32_t* kp_octave,
                               float* desc /*cap x 128*/, int cap, int32_t* n_out);

/* The same detector as the detector of the batched, HBM-resident path — the configuration the reference runs live:
 * cv2.SIFT_create() (src/visual_slam.py:17, injected at :21) + cv2.BFMatcher(cv2.NORM_L2, crossCheck=True) (:19), per pair
 * in the order of src/visual_slam.py:294-298.  After vo_batch_configure_sift the calls vo_frames_upload[_async],
 * vo_frames_detect[_async], vo_pairs_run[_async], vo_pair_matches, vo_pairs_gather and vo_sync act on the SIFT state
 * (vo_batch_configure switches back to ORB).  Frames are detected in sub-batches whose float scale space (5 Gaussian + 5 DoG
 * planes per octave of the 2x up-sampled image) is scratch; keypoints, the 128-byte descriptors (integer bin values 0..255),
 * and the int8 operand image of the matrix-core L2 matcher stay resident per slot.  nfeatures must be 0 (cv2's default: keep
 * every keypoint); kp_cap = keypoints kept per frame (0: a default from the frame size, rounded up to 256); a frame with more
 * is truncated in cv2's list order and flagged (VO_WARN_CAPACITY from vo_frame_features_sift). */
int vo_batch_configure_sift(vo_ctx* ctx, int h, int w, const vo_sift_params* params, int max_frames, int max_pairs, int kp_cap);
/* like vo_frame_features; desc: cap x 128 bytes = the descriptor values cv2 hands out as float32 */
int vo_frame_features_sift(vo_ctx* ctx, int slot, float* kp_xy, float* kp_size, float* kp_angle, float* kp_response,
                           int32_t* kp_octave, uint8_t* desc /*cap x 128*/, int cap, int32_t* n_out);

/* Parity seam of the SIFT matcher: rows[n][128] (values 0..255; 0 <= n <= vo_batch_kp_capacity) become slot `slot` as if they
 * had been detected: descriptors, the matcher's int8 operand image and norms, the keypoint count, the flags (the norm-bound bit
 * by the descriptor kernel's rule, the capacity bit clear), kp_xy = xy[n][2] (zeros when NULL), size / angle / response / octave
 * zero.  Operand rows past n keep what an earlier frame left in the slot.  Needs vo_batch_configure_sift; synchronous. */
int vo_stage_sift_rows(vo_ctx* ctx, int slot, const uint8_t* rows /*[n][128]*/, int n, const float* xy /*[n][2] or NULL*/);

/* Parity seam of the Hamming matchers — a TEST seam, the ORB counterpart of vo_stage_sift_rows: rows[n][32] (0 <= n <=
 * vo_batch_kp_capacity) become slot `slot` exactly as a detection of that one slot would leave them: the descriptors, the keypoint
 * count, the flags clear, kp_xy = xy[n][2] (zeros when NULL), size / angle / response / octave zero, and the matrix-core matcher's
 * operand image of the slot in the format the kernel chosen by vo_set_matcher_kernel reads (when that differs from the image the
 * other slots hold, they are expanded again, as after a detection).  Descriptor rows past n keep what an earlier frame left in
 * the slot.  vo_frame_features returns what was put in.  Needs vo_batch_configure (VO_ERR_NOT_CONFIGURED without, or in SIFT
 * mode); VO_ERR_INVALID for a bad slot, n < 0, n > capacity, or rows == NULL with n > 0; synchronous. */
int vo_stage_orb_rows(vo_ctx* ctx, int slot, const uint8_t* rows /*[n][32]*/, int n, const float* xy /*[n][2] or NULL*/);

/* cv2.imread(filename) for a .jpg — /root/reference/src/visual_slam.py:346 (also triangulate_points_from_images.py:14-15,
 * feature_detection.py:5,10).  What cv2 does with such a file is libjpeg-turbo's default decompression: baseline Huffman
 * decoding, the 13-bit integer IDCT (JDCT_ISLOW), triangle-filter ("fancy") chroma upsampling, fixed-point YCbCr -> RGB,
 * channels delivered as B, G, R; a grey-scale file comes back with three equal channels (IMREAD_COLOR).  All of it runs
 * on the device, Huffman decoding included (parallel inside one scan by self-synchronisation).
 * Supported: SOF0 / SOF1 8-bit, grey or three components in one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0, restart
 * intervals.  VO_ERR_UNSUPPORTED: progressive, lossless, arithmetic, 12-bit, CMYK, other sampling ratios, multi-scan
 * files.  VO_ERR_INVALID: not a JPEG / broken marker structure.  EXIF orientation is reported by vo_jpeg_info and NOT
 * applied (cv2.imread applies it; the Python wrapper does the flip / transpose).
 * vo_jpeg_info: header only, no context, no GPU.  sampling = (h << 4) | v of the first component. */
int vo_jpeg_info(const uint8_t* data, size_t nbytes, int32_t* h, int32_t* w, int32_t* ncomp, int32_t* sampling, int32_t* orientation);
/* cv2.imdecode(buf, cv2.IMREAD_COLOR): bgr_out = [h][w][3] dense, needs cap_h x cap_w >= h x w (sizes from vo_jpeg_info) */
int vo_jpeg_decode(vo_ctx* ctx, const uint8_t* data, size_t nbytes, uint8_t* bgr_out, int cap_h, int cap_w, int32_t* h, int32_t* w);
/* F files of identical size h x w, file f = blob[offsets[f] .. offsets[f + 1]); bgr_out = [F][h][w][3] dense */
int vo_jpeg_decode_batch(vo_ctx* ctx, const uint8_t* blob, const int64_t* offsets, int F, uint8_t* bgr_out, int h, int w);
/* The reference's whole ingest (visual_slam.py:346-352) for F files of identical size: imread -> cv2.resize(img, (w, h) of
 * the batch configuration) -> gray into level 0 of slots first_slot ..; nothing but the compressed bytes crosses PCIe.
 * resized_out (optional, host, [F][h][w][3]) receives the resized B G R frames (Frame.image). */
int vo_frames_ingest_jpeg(vo_ctx* ctx, const uint8_t* blob, const int64_t* offsets, int F, int first_slot, uint8_t* resized_out);

/* The batched form of the same step: F full-resolution host frames are resized on the device to the configured
 * (w, h), converted to gray as ORB does, and become level 0 of slots first_slot..; resized_out (optional, host,
 * [F][h][w][channels] dense) receives the resized frames (the reference keeps them as Frame.image).  Source strides per the
 * IMAGE LAYOUT CONTRACT, frame_stride >= (sh - 1) * row_stride + sw * channels. */
int vo_frames_ingest(vo_ctx* ctx, const uint8_t* frames, int F, int sh, int sw, int channels, int row_stride,
                     int64_t frame_stride, int first_slot, uint8_t* resized_out);

/* VisualSlam.update_feature_mapper + track_feature_back_in_time — src/visual_slam.py:183-188, :94-99, for ALL
 * features at once.  A feature id is (frame, index) with frame < F, index < cap.  Pair p maps
 * every matched feature (pair_frames[2p+1], mt[k]) to (pair_frames[2p], mq[k]), k in [match_off[p], match_off[p+1]);
 * pairs are applied in order (a later pair overwrites an earlier entry, as the dict does).  Outputs are F x cap:
 * the first feature of every feature's chain and the number of links followed. */
int vo_feature_tracks(vo_ctx* ctx, int F, int cap, const int32_t* pair_frames, const int32_t* match_off,
                      const int32_t* mq, const int32_t* mt, int P, int32_t* root_frame, int32_t* root_idx, int32_t* hops);

/* The step after the pair path ON RESIDENT DATA — VisualSlam.update_feature_mapper / estimate_current_camera_position /
 * add_information_to_map, src/visual_slam.py:183-266 and :153-180, without the bundle adjustment (src/map.py:104-186).
 * Consumes what the most recent vo_pairs_run (want_points = 1) left in HBM — the pairs' inlier lists, inlier pixel
 * coordinates and triangulated points (a configure call in between forgets them: VO_ERR_INVALID) — for ALL its B pairs, which must form a chain of distinct frames (a0, b0), (b0, b1), ...
 * (the order the reference walks a sequence in), and runs on the context's stream without a host round trip:
 *   pair 0: initialize_map (:43-92) — the two cameras and one map point per E inlier, keyed by featureid1.  [deviation] the
 *     reference stores camera 1 = (I, 0), camera 2 = (R, t) but the points in camera-2 coordinates and leaves the
 *     reconciliation to g2o; here camera 2 = (I, 0), camera 1 = (R^T, -R^T t): consistent with the points.
 *   pair p >= 1: feature_mapper links of every inlier (:183-188); for every inlier in match order the track is traced back
 *     (:94-99) and, if its root owns a map point, (map point, keypoint2) joins the correspondences (:201-227);
 *     cv2.solvePnPRansac(map, image, K, zeros(4)) with `iterations`, `reproj_err`, `confidence` (cv2's defaults 100, 8.0,
 *     0.99; :231-235); the camera (Rodrigues(rvec), tvec) (:243-251); reconstruct_3d_points with K pose(frame2), K pose(frame1)
 *     (:164-172); points within max_point_norm (50, :177) whose root is not in the map become map points under featureid1.
 * poses: (B + 1) x 12 — world -> camera [R | t] of pair 0's first frame, then of every pair's second frame (zeros from a
 * pair that could not be localised on).  status[p]: VO_OK; VO_ERR_TOO_FEW (fewer than 4 correspondences: cv2 raises) or
 * VO_ERR_NO_MODEL (retval False) at the pair where the reference stops adding cameras; VO_ERR_NOT_CONFIGURED for the pairs
 * after it; a pair's own failure status if vo_pairs_run could not solve it.  n_corr / n_inl: correspondences and PnP
 * inliers of the pair; n_map: map points after it. */
int vo_tracks_pnp_batch(vo_ctx* ctx, int B, const double* K, int iterations, double reproj_err, double confidence, uint64_t seed,
                        double max_point_norm, double* poses, int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_map);

/* ------------------------------------------------------------------ bundle adjustment
 * Map.optimize_map — src/map.py:104-186, called at the end of every frame (src/visual_slam.py:90, :265, :367): g2o's
 * Levenberg-Marquardt over VertexSE3Expmap cameras (fixed where cam_fixed is set), marginalised VertexPointXYZ points and
 * one EdgeProjectXYZ2UV per observation with information I, RobustKernelHuber(huber_delta) and
 * CameraParameters(focal, (cx, cy), 0) — ONE focal length, as the reference passes camera_matrix[0, 0] only (map.py:113).
 * OptimizationAlgorithmLevenberg over BlockSolverSE3: tau 1e-5, lambda from the first linearisation, at most 10 trials per
 * iteration, Schur complement on the points, exactly `iterations` iterations unless 10 trials fail, rho == 0 or lambda
 * overflows (there is no convergence test).  g2o is not vendored: this restates its 2020 sources (g2o-python 0.0.11) from
 * memory; parity with a g2o build is unpinned, the checker is the numpy restatement tests/ba_reference.py.
 * B independent problems, one workgroup each: problem b owns cameras cam_off[b] .. cam_off[b+1], points pt_off[b] ..,
 * observations obs_off[b] ..; obs_cam / obs_pt are indices LOCAL to the problem.  poses: [camera][12] world -> camera
 * [R | t] (3 x 4 row-major), in / out; points: [point][3], in / out (map.py:175-186 writes both back).  A fixed camera
 * and a point without observations keep their input bytes; a free camera's R comes back from the unit quaternion g2o
 * keeps.  chi2: [B][2] = activeRobustChi2 before and after; iterations_run / trials_run: LM iterations started and linear
 * solves attempted.  Two calls on the same input return the same bytes (every sum has a fixed order).
 * status[b]: VO_OK; VO_ERR_UNSUPPORTED for a problem with more than VO_BA_MAX_CAMERAS cameras or VO_BA_MAX_FREE free ones
 * (a map that large goes to vo_bundle_adjust_large, below); VO_ERR_INVALID for an observation that names a missing camera or
 * point.  Such a problem's data come back unchanged and the rest of the batch is solved.
 * vo_bundle_adjust: one problem; a negative status is the return value. */
#define VO_BA_MAX_CAMERAS 64
#define VO_BA_MAX_FREE    16
typedef struct {
    int32_t iterations;     /* 40 (map.py:171), at most 1000 */
    int32_t reserved;
    double  huber_delta;    /* 1.0 (g2o's RobustKernelHuber default); <= 0: no robust kernel */
} vo_ba_opts;
int vo_bundle_adjust_batch(vo_ctx* ctx, int B, const int32_t* cam_off, const int32_t* pt_off, const int32_t* obs_off,
                           double* poses, const uint8_t* cam_fixed, double* points, const int32_t* obs_cam,
                           const int32_t* obs_pt, const double* obs_xy, double focal, double cx, double cy,
                           const vo_ba_opts* opts, double* chi2, int32_t* iterations_run, int32_t* trials_run,
                           int32_t* status);
int vo_bundle_adjust(vo_ctx* ctx, double* poses, const uint8_t* cam_fixed, int ncam, double* points, int npt,
                     const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs,
                     double focal, double cx, double cy, const vo_ba_opts* opts, double* chi2 /* [2] */,
                     int32_t* iterations_run, int32_t* trials_run);

/* ------------------------------------------------------------------ bundle adjustment, large maps
 * vo_bundle_adjust for ONE map of hundreds of cameras (the joined flight after vo_pose_graph and correct_points, two maps joined
 * by vo_map_align): the same Levenberg-Marquardt, rule for rule (tau 1e-5, lambda from the first linearisation, nu = 2, rho with
 * g2o's + 1e-3, at most 10 trials per iteration, the Huber weight rho' only, unit-quaternion cameras, no convergence test), on
 * other linear algebra.  The reduced camera system S (6 F x 6 F, g carried as its last row) lies in device memory and is factored
 * exactly by a blocked dense Cholesky whose panels and trailing updates span the whole GPU; the host drives the LM loop and reads
 * a 64-byte decision record once per trial.  Workgroups synchronise at kernel boundaries only; no floating-point atomics: every
 * sum has one fixed order, so two calls on the same input return the same bytes (docs/kernels/k_bundle_adjust_large.md).
 * Arguments, in / out conventions and vo_ba_opts as vo_bundle_adjust; obs_cam / obs_pt index this map's rows.
 * Capacity: at most VO_BA_LARGE_MAX_FREE free cameras (S: 3073 x 3080 doubles = 75.7 MB), any number of fixed ones; points,
 * observations and listed pairs (one observation each of free cameras c1 <= c2 on a shared point) are bounded by int32 and by
 * the call's scratch.  With C cameras, F free, N points, O observations, B listed blocks, Q listed pairs, n = 6 F,
 * ld = (n + 8) & ~7 and G = ceil(N / 256) the scratch is, each term rounded up to 256 bytes,
 *   4 (C + F + N + 1 + 2 O + F + 1 + Of + B + 1) + 8 B + 8 Q + 16 O                      the lists (Of: observations by free cameras)
 *   + 2 * 8 (12 C + 4 F + 3 N) + 8 (18 O + 15 N + 48 F)                                  estimates, W, H_pp, b_p, H_pp^-1, H_cc, b_c, delta_c
 *   + 8 (n + 1) ld + 8 * 48 * 48 ceil(n / 48) + 3 * 8 max(G, 1) + 64                     S, the factored diagonal blocks, the reductions' partials, the record.
 * Beyond the capacity: VO_ERR_UNSUPPORTED; an observation of a missing camera or point, a NULL argument or iterations > 1000:
 * VO_ERR_INVALID; the data stay unchanged either way.  A fixed camera and a point without observations keep their input bytes, a
 * free camera without observations takes delta = 0, F = 0 is structure only, a map without observations runs ten failed
 * factorisations and moves nothing: as vo_bundle_adjust and tests/ba_reference.py.
 * Out of scope: the band structure of a flight's S, batches of large maps, an iterative solver. */
#define VO_BA_LARGE_MAX_FREE 512
int vo_bundle_adjust_large(vo_ctx* ctx, double* poses, const uint8_t* cam_fixed, int ncam, double* points, int npt,
                           const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs,
                           double focal, double cx, double cy, const vo_ba_opts* opts, double* chi2 /* [2] */,
                           int32_t* iterations_run, int32_t* trials_run);
/* vo_ba_large_solve: the factorisation and solve of one trial of vo_bundle_adjust_large on a system of the caller's, A x = b with
 * A symmetric positive definite, n = 6 F, 1 <= F <= VO_BA_LARGE_MAX_FREE: for callers that build their own normal equations, and
 * for the tests, which hand the blocked Cholesky matrices no map produces (tests/test_gpu_ba_large_solve.py).  The same kernels
 * in the same order as a trial runs them, nothing of the LM loop.  A: [n][n] row-major, of a row only the part up to its diagonal
 * is used; b: [n].  x: [n]; L: [n][n], the Cholesky factor's lower triangle written, the rest left as it came, or NULL; y: [n],
 * the forward-substituted b (L y = b, L^T x = y), or NULL.  *pivot_failed = 1 for a pivot that is not positive and finite: x, L
 * and y are then left as they came and the return value is VO_OK; otherwise 0.  n that is no multiple of 6 or < 6, a NULL A, b, x
 * or pivot_failed: VO_ERR_INVALID; n > 6 VO_BA_LARGE_MAX_FREE: VO_ERR_UNSUPPORTED; nothing is written then.  Scratch, each term
 * rounded up to 256 bytes, ld = (n + 8) & ~7: 8 (n + 1) ld + 8 * 48 * 48 ceil(n / 48) + 8 n + 64. */
int vo_ba_large_solve(vo_ctx* ctx, const double* A, const double* b, int n, double* x, double* L, double* y,
                      int32_t* pivot_failed);

/* ------------------------------------------------------------------ the complete per-frame map step on resident data
 * vo_tracks_pnp_batch's walk joined to what ends every frame of VisualSlam.estimate_current_camera_position
 * (src/visual_slam.py:190-266) and of its caller (:306-311), on a map that stays on the device: points, cameras and the
 * Observation list (src/map.py).  Same input as vo_tracks_pnp_batch (all B pairs of the most recent vo_pairs_run with
 * want_points, a chain of distinct frames), same stop rule and statuses; additionally the run's match_mode must be
 * one-to-one (0 or 2): with ratio matches two inliers can share a track root and the reference's insert order is not
 * defined by the data (VO_ERR_UNSUPPORTED).
 *   pair 0: initialize_map (:43-92) — cameras as vo_tracks_pnp_batch stores them (first fixed, second free), one point
 *     per E inlier under featureid1, per inlier in match order the observations (point, camera 1, keypoint1), (point,
 *     camera 2, keypoint2) (:79-87); optimize_map (:90).  No filter, no PnP (len(list_of_frames) < 3, :198).
 *   pair p >= 1: correspondences -> solvePnPRansac -> camera -> triangulation as vo_tracks_pnp_batch, reading the map
 *     points and the camera of frame 1 as bundle adjustment and filter left them; add_information_to_map (:152-179):
 *     every inlier within max_point_norm, in match order, decided against the map as it was before the loop (:154-156) —
 *     root in the map: one observation (that point, camera 2, keypoint2) (:121-129); otherwise a new point under featureid1
 *     with observations on camera 1, then camera 2 (:101-119); freeze_nonlast_cameras (:270-275): all cameras fixed but
 *     the last free_cameras (1 .. VO_BA_MAX_FREE covers unfreeze_cameras, :281-286); optimize_map (:265, src/map.py:104-186:
 *     vo_bundle_adjust's kernel on the resident lists, poses and points written back); the filter (:266, map.py:46-70):
 *     an observation stays when its squared reprojection error < filter_threshold, points are not removed;
 *     limit_number_of_camera_in_map(max_cameras) (:311, map.py:299-318): beyond that, remove_camera_from_map(cameras[0])
 *     (map.py:188-232) — its observations go, then every point that is left with exactly ONE observation and that
 *     observation (a point with none is not counted by the defaultdict and stays); a removed point's feature id can
 *     receive a new point later.
 * A pair whose localisation fails does none of this and ends the chain [deviation, as vo_tracks_pnp_batch; vo_slam_chains_restart
 * starts a new map instead].
 * ba_iterations = 0, filter_threshold <= 0 and max_cameras >= B + 1 give vo_tracks_pnp_batch's poses and counts, byte for
 * byte.  max_cameras + 1 must not exceed VO_BA_MAX_CAMERAS (VO_ERR_UNSUPPORTED); max_cameras >= 2.
 * poses_pnp: every camera as it entered the map (rows 0, 1: the initial pair; then solvePnPRansac's result); poses: every
 * camera as the map last held it (at the end of the chain, or when it was evicted); zeros for a pair not localised.
 * n_pts / n_obs / n_cam: the map's sizes after every pair; chi2 [B][2], ba_iterations_run, ba_trials_run: as
 * vo_bundle_adjust reports them, per pair.
 * vo_slam_map_size / vo_slam_map: which = 0 the map at the end of the chain, 1 the snapshot — a device-to-device copy
 * taken during the run at pair snapshot_pair after stage 1 add_information_to_map (before bundle adjustment), 2 bundle
 * adjustment, 3 the filter, 4 the camera limit (the seam the tests use, as vo_stage_* is for the detector).  cam_frame:
 * index of the camera's frame in the chain; pt_feature: [npt][2] = (index of the frame in the chain, keypoint) of the
 * owning feature id.  A configure call or a vo_pairs_run forgets both maps (VO_ERR_INVALID). */
typedef struct {
    int32_t pnp_iterations; double reproj_err, confidence; uint64_t seed;   /* cv2's 100, 8.0, 0.99 (:231-235) */
    double  max_point_norm;          /* 50 (:177) */
    int32_t ba_iterations;           /* 40 (map.py:172); 0: no bundle adjustment */
    double  huber_delta;             /* 1.0 (map.py:161) */
    int32_t free_cameras;            /* 2 (:270-275) */
    double  filter_threshold;        /* 1.0 (:266); <= 0: no filter */
    int32_t max_cameras;             /* 18 (:311) */
    int32_t snapshot_pair, snapshot_stage;   /* -1, 0: none */
} vo_slam_opts;
int vo_slam_chain(vo_ctx* ctx, int B, const double* K, const vo_slam_opts* opts, double* poses_pnp /*(B+1)x12*/, double* poses /*(B+1)x12*/,
                  int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                  double* chi2 /*[B][2]*/, int32_t* ba_iterations_run, int32_t* ba_trials_run);
int vo_slam_map_size(vo_ctx* ctx, int which, int32_t* ncam, int32_t* npt, int32_t* nobs);
int vo_slam_map(vo_ctx* ctx, int which, int32_t* cam_frame, double* cam_pose /*[ncam][12]*/, uint8_t* cam_fixed, int32_t* pt_feature /*[npt][2]*/,
                double* points /*[npt][3]*/, int32_t* obs_cam, int32_t* obs_pt, double* obs_xy /*[nobs][2]*/);

/* ------------------------------------------------------------------ the map step as a stream: one map, one call after another
 * vo_slam_chain walks one vo_pairs_run and its map ends with the call; a flight longer than one batch configuration needs the
 * reference's loop (src/visual_slam.py:333-374): one frame after another into one Map.  vo_slam_stream keeps the map, the
 * feature tracks and every table of the walk on the device when it returns, in an allocation of their own, and a later call
 * continues them.  The contract: the calls of a stream together compute the bytes one vo_slam_chain on the whole flight computes.
 *   resume = 0 starts a stream: vo_slam_chain's checks, options, statuses and bytes (outputs and vo_slam_map) for the B pairs of
 *     the most recent vo_pairs_run; n_carried = 0.  total_pairs >= B is the number of pairs the whole stream may reach; it sizes
 *     the lists once — points (total_pairs + 1) kp_cap; observations 2 kp_cap min(max_cameras + 1, total_pairs) (a camera is
 *     observed at most kp_cap times as a pair's second frame and kp_cap times as the next pair's first) and the bundle
 *     adjustment's pair list from those — and nothing grows afterwards.  A call that would pass it: VO_ERR_INVALID.
 *   Between calls the caller uploads and detects the next frames into any slot EXCEPT THE ANCHOR SLOT, the slot of the stream's
 *     last frame, and runs vo_pairs_run (want_points) on a chain that starts there.  vo_pairs_run forgets vo_slam_map's host
 *     copies as always but leaves the stream alone.  An upload, ingest, detection or vo_stage_sift_rows that covers the anchor
 *     slot ends the stream's use: a later resume = 1 is refused.
 *   resume = 1 continues it.  VO_ERR_INVALID, with the stream left as it is: no live stream; its last call ended lost; pair 0
 *     does not start at the anchor slot; the run is not a chain of distinct frames (so no later pair can use the anchor slot);
 *     K or an option other than snapshot_pair / snapshot_stage differs from the stream's; total_pairs would be passed.  Ratio
 *     matches: VO_ERR_UNSUPPORTED.  total_pairs is ignored.  Every pair is a p >= 1 step of vo_slam_chain; there is no
 *     initial step.  Per-pair outputs [B] as vo_slam_chain reports them for these pairs; snapshot_pair counts along the call.
 *     poses_pnp row 0: the anchor camera as it entered the map (the previous call's last row), rows 1 .. B the new cameras; poses:
 *     the same cameras as the map last held them, in this call or when evicted.  The cameras the map held at the start of the
 *     call beside the anchor have no row: carried_frame [n_carried] names them by their index along the whole stream, in map
 *     order, and carried_poses [n_carried][12] is each one as the map last held it during this call (with free_cameras >= 3
 *     one of them is still free in the first steps and changes).  Both arrays take max_cameras rows.
 *   vo_slam_map after either: cam_frame and pt_feature[:, 0] count along the whole stream.
 * The stream ends — its memory is released — with vo_destroy, vo_batch_configure[_sift], a new resume = 0 or any vo_slam_chain*
 * call.  A call that ends lost (vo_slam_chain's stop rule and statuses) leaves the map for vo_slam_map; it cannot be continued
 * (vo_slam_stream_restart, below, is the stream that can).
 * How a call continues a map whose frames have lost their slots (k_slam_carry): the slot-keyed tables get two ghost rows behind
 * the max_frames slots (max_frames + 2 < 2^20).  Every keypoint of the anchor frame whose track root lies in an older frame is
 * linked to an entry of a ghost row that takes over the root's map point — also a root that owns no point, which must stay
 * one: the reference finds nothing under it at every later frame and adds a new point each time (:139-146).  A point no track
 * can reach any more keeps its place in the lists and in the bundle adjustment, as in the reference, but has no key.
 * [deviation] none in the results; the per-call cost is one k_slam_carry launch and the download of the map for vo_slam_map.
 * Several sequences per stream call: vo_slam_streams, below.  Out of scope: pruning points that have lost every
 * observation (the reference keeps them: the lists and k_bundle_adjust's cost grow with the flight), relocalisation inside the
 * walk (vo_map_localize, below, is the operator; nothing here calls it), and any change to the entries above. */
int vo_slam_stream(vo_ctx* ctx, int resume, int total_pairs, int B, const double* K, const vo_slam_opts* opts,
                   double* poses_pnp /*(B+1)x12*/, double* poses /*(B+1)x12*/,
                   int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                   double* chi2 /*[B][2]*/, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                   int32_t* n_carried, int32_t* carried_frame /*[max_cameras]*/, double* carried_poses /*[max_cameras][12]*/);

/* ------------------------------------------------------------------ the same map step for S independent sequences in one call
 * vo_slam_chain is sequential by nature — frame k + 1 is localised against the map frame k left — and runs as one workgroup
 * per kernel; several sequences (several flights, or one flight cut into shards) are what runs in parallel.  vo_slam_chains
 * walks S of them at once, one workgroup per sequence and kernel: the launches per call stay those of the longest sequence.
 *   B = seq_off[S] is all the pairs of the most recent vo_pairs_run (want_points); sequence s is its pairs seq_off[s] ..
 *   seq_off[s + 1] - 1 (seq_off[0] = 0, strictly increasing, S >= 1) and must by itself be a chain of distinct frames, as
 *   vo_slam_chain asks of its one chain.  NO FRAME SLOT MAY BELONG TO TWO SEQUENCES (VO_ERR_INVALID): the slot-keyed
 *   tables are shared between the sequences exactly because their slots are disjoint.  A frame two shards share (a halo
 *   frame) is uploaded into two slots; sequences that share a slot are out of scope.
 * Every option, check and code of vo_slam_chain applies (ratio matches: VO_ERR_UNSUPPORTED).  opts->snapshot_pair counts
 * along sequence snapshot_seq (0 .. S - 1, and snapshot_pair < its pair count); snapshot_seq is ignored when snapshot_pair < 0.
 * Per-pair outputs are indexed by the pair's position in the run; sequence s owns the pose rows seq_off[s] + s ..
 * seq_off[s + 1] + s (its B_s + 1 cameras).  Every sequence computes exactly what vo_slam_chain computes for it alone: the
 * sequences are independent, a pair that cannot be localised ends ITS sequence (the failing status at that pair,
 * VO_ERR_NOT_CONFIGURED after it) and the others run to their end.
 * vo_slam_chains_map_size / vo_slam_chains_map: the map of sequence seq, which = 0 at its end, 1 the snapshot (valid only
 * for seq == snapshot_seq); cam_frame and pt_feature[:, 0] are indices along the sequence's own chain.  After a
 * vo_slam_chains call vo_slam_map_size / vo_slam_map report sequence 0 (and the snapshot only if snapshot_seq == 0).  A
 * configure call, a vo_pairs_run, a vo_slam_chain or a later vo_slam_chains forgets these maps; a refused call leaves none. */
int vo_slam_chains(vo_ctx* ctx, int S, const int32_t* seq_off /*[S+1]*/, const double* K, const vo_slam_opts* opts, int snapshot_seq,
                   double* poses_pnp /*(B+S)x12*/, double* poses /*(B+S)x12*/,
                   int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam /*[B] each*/,
                   double* chi2 /*[B][2]*/, int32_t* ba_iterations_run, int32_t* ba_trials_run /*[B] each*/);
int vo_slam_chains_map_size(vo_ctx* ctx, int seq, int which, int32_t* ncam, int32_t* npt, int32_t* nobs);
int vo_slam_chains_map(vo_ctx* ctx, int seq, int which, int32_t* cam_frame, double* cam_pose /*[ncam][12]*/, uint8_t* cam_fixed,
                       int32_t* pt_feature /*[npt][2]*/, double* points /*[npt][3]*/, int32_t* obs_cam, int32_t* obs_pt, double* obs_xy /*[nobs][2]*/);

/* ------------------------------------------------------------------ ... that starts a new map after a lost frame and goes on
 * vo_slam_chains ends a sequence at its first lost frame [deviation]; the reference prints "Failed to estimate the camera
 * position" (src/visual_slam.py:254), adds no camera, and dies at the next frame on camera_dict[ip.frame1.id] (:167, inside the
 * try of :258).  The recovery it names but never wires up: initialize_map begins with self.map.clean() (:43-45) and can be
 * called again.  vo_slam_chains_restart is vo_slam_chains — same arguments, checks, options and outputs — with that
 * recovery, decided and done on the device, per sequence, inside the step loop:
 *   1 A pair that failed in vo_pairs_run (its own status != VO_OK) gets that status; the map is left as it stands and the
 *     sequence is LOST until rule 3 applies.  No pair ever gets VO_ERR_NOT_CONFIGURED.
 *   2 A pair whose own result is VO_OK but whose solvePnPRansac fails (VO_ERR_TOO_FEW, VO_ERR_NO_MODEL) starts a new
 *     SEGMENT in the same step: the map is cleaned and initialize_map (:43-92) runs on this pair exactly as on pair 0 —
 *     second camera = identity, first = (R^T, -R^T t), first fixed, second free; one point per E inlier under featureid1
 *     with its two observations, in match order (:56-87); optimize_map (:90); no filter; the camera limit (:311).  Nothing
 *     of the failed localisation reaches the new map.
 *   3 A lost sequence that meets a pair whose own result is VO_OK starts a new segment from it, as in rule 2.
 *   4 A new segment forgets the old one: the map's lists restart at length 0, no feature id of the old map stays in
 *     mappointdict (:154-156), and every feature track (feature_mapper, :183-188; track_feature_back_in_time, :94-99) is cut
 *     at the segment's first frame.
 *   5 cam_frame and pt_feature[:, 0] stay indices along the sequence's whole chain; they do not restart with the segment.
 *   6 The map a call leaves (vo_slam_chains_map, vo_slam_map) is the last segment's; if the sequence ends lost, the one it
 *     had when it was lost.  snapshot_pair still counts along the sequence.
 * A pair that starts a segment reports status, n_corr, n_inl, n_pts, n_obs, n_cam, chi2 and the bundle adjustment's counts
 * as pair 0 of a chain does.  segment [B]: index of the pair's segment within its sequence, 0, 1, ... in order of start;
 * -1 for a pair in no segment (rule 1).  cause [B]: 0 for a pair that continues its segment, or starts segment 0 at the
 * sequence's first pair; otherwise, at a pair that starts a segment, the status that ended tracking before it — the
 * solvePnPRansac status of rule 2, or the status of the FIRST failed pair of the lost stretch (rule 3).  seg_poses_pnp,
 * seg_poses [B][12]: at a pair p that starts a segment, the segment's first camera (frame 1 of the pair) as it entered
 * the map and as the map last held it; zeros elsewhere.  Row p + 1 of poses_pnp / poses holds the pair's second frame as
 * always; row p belongs to the previous segment's gauge (or is zero) — except row 0 of a sequence whose first pair starts
 * segment 0, which holds that first camera as it does in vo_slam_chains.  A sequence that never loses a frame gets
 * vo_slam_chains' bytes in every output and map, segment = 0, cause = 0.
 * Out of scope: joining segments into one gauge inside the walk (vo_map_align, below, joins two saved maps afterwards), using vo_map_localize
 * (below) against the old map from inside the walk, a restart form of vo_tracks_pnp_batch, ratio matches (VO_ERR_UNSUPPORTED as before). */
int vo_slam_chains_restart(vo_ctx* ctx, int S, const int32_t* seq_off /*[S+1]*/, const double* K, const vo_slam_opts* opts, int snapshot_seq,
                           double* poses_pnp /*(B+S)x12*/, double* poses /*(B+S)x12*/,
                           int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam /*[B] each*/,
                           double* chi2 /*[B][2]*/, int32_t* ba_iterations_run, int32_t* ba_trials_run /*[B] each*/,
                           int32_t* segment /*[B]*/, int32_t* cause /*[B]*/, double* seg_poses_pnp /*[B][12]*/, double* seg_poses /*[B][12]*/);

/* ------------------------------------------------------------------ the stream that starts a new map after a lost frame
 * vo_slam_stream ends at its first lost frame and vo_slam_chains_restart needs the whole flight resident in one vo_pairs_run; a
 * long flight needs both.  vo_slam_stream_restart is vo_slam_stream — same arguments, sizing, slot rules and carry — with
 * vo_slam_chains_restart's recovery and its four outputs.  The contract: the calls of a restart stream together compute the
 * bytes one vo_slam_chains_restart call with S = 1 computes on the whole flight.
 *   Mode: restart is a property of the stream.  A stream begun by one of the two entry points is continued only by the same
 *     one; the other returns VO_ERR_INVALID and leaves the stream as it was, still continuable by the right entry point.
 *     vo_slam_stream itself is unchanged and still refuses to continue after a call that ended lost.
 *   resume = 0: vo_slam_chains_restart's checks, rules 1-6 and bytes with S = 1 for the B pairs of the most recent
 *     vo_pairs_run; n_carried = 0.  The lists are sized from total_pairs as for vo_slam_stream; a restart sets their lengths
 *     back to 0, so nothing can outgrow them.
 *   resume = 1: vo_slam_stream's refusals — no live stream, the anchor slot was written, pair 0 does not start at the anchor,
 *     not a chain of distinct frames, K or an option differs, total_pairs would be passed (VO_ERR_INVALID), ratio matches
 *     (VO_ERR_UNSUPPORTED) — except the one for a lost stream: a call that ended lost IS continued.  The first usable pair then
 *     starts a new segment by rule 3.  A call whose every pair fails leaves the stream lost, still continuable, and still holding
 *     the map it had when tracking was lost (rule 6).
 *   Carried between the calls, on the device: whether the stream is alive, the number of segments started and the status that
 *     ended tracking and has not been reported yet.  So segment counts along the whole stream, and cause, at a pair that starts
 *     a segment, is the status of the FIRST failed pair of the lost stretch even when that pair was in an earlier call.
 *   Pose rows: row 0 of poses_pnp / poses is the previous call's last row — zeros if that frame was never localised — and is
 *     never the first camera of a segment.  seg_poses_pnp / seg_poses [B][12] are written at a pair of THIS call that starts a
 *     segment, pair 0 included (its first frame is the anchor).  carried_frame / carried_poses name every camera the map held
 *     at the start of the call other than the anchor; after a call that ended lost the anchor is not in the map, so they name
 *     ALL its cameras (n_carried <= max_cameras as before).  A segment's first camera that was started in an earlier call is
 *     reported through the carried rows like any other carried camera.  A whole-flight row is therefore always the latest
 *     report of a frame across the calls' own rows, seg_poses rows and carried rows; a carried frame f reports to seg_poses
 *     row f if pair f started a segment (and to poses row 0 as well for f = 0), to poses row f otherwise.
 *   vo_slam_map after a call: cam_frame and pt_feature[:, 0] are stream indices; the map is the last segment's, or the one
 *     held when tracking was lost.
 *   A flight that never fails gets vo_slam_stream's bytes in every shared output and in the map, segment = 0, cause = 0.
 * How: k_slam_restart_stream between k_chain_pose and k_chain_triangulate of every step; the step kernels that name a pose row
 * and k_slam_carry have a restart form (slam_kernels.hip).  A point whose key the carry marked none has nothing to clear at a
 * restart; a key in a ghost row is cleared like any other.  The ghost rows keep alternating across segments.
 * [deviation] none in the results; the cost is one more launch per step, and four small downloads and the alive word per call.
 * Several sequences per stream call: vo_slam_streams, below.  Out of scope: joining segments into one gauge inside the walk (vo_map_align), relocalisation
 * against an old map from inside the walk (vo_map_localize is the operator), pruning points without observations, ratio matches, a restart form of vo_tracks_pnp_batch, any change
 * to the entries above. */
int vo_slam_stream_restart(vo_ctx* ctx, int resume, int total_pairs, int B, const double* K, const vo_slam_opts* opts,
                           double* poses_pnp /*(B+1)x12*/, double* poses /*(B+1)x12*/,
                           int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                           double* chi2 /*[B][2]*/, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                           int32_t* n_carried, int32_t* carried_frame /*[max_cameras]*/, double* carried_poses /*[max_cameras][12]*/,
                           int32_t* segment /*[B]*/, int32_t* cause /*[B]*/, double* seg_poses_pnp /*[B][12]*/, double* seg_poses /*[B][12]*/);

/* ------------------------------------------------------------------ S restart streams at once, carried from call to call
 * One stream is one workgroup per kernel; several long flights (several cameras, or one flight cut into shards) are what runs in
 * parallel, and vo_slam_chains needs every frame of every flight resident in one vo_pairs_run.  vo_slam_streams is
 * vo_slam_stream_restart for S sequences in one call, laid out as vo_slam_chains_restart lays them out.  The contract is one
 * equality: for every sequence s the calls together compute the bytes a vo_slam_stream_restart stream computes for that flight
 * alone with the same chunking (so, by that entry's contract, the bytes of vo_slam_chains_restart with S = 1 on the whole
 * flight) — whatever the other sequences do, in whatever order they are listed, whichever slots they use.
 *   B = seq_off[S] is all the pairs of the most recent vo_pairs_run (want_points); sequence s is its pairs seq_off[s] ..
 *     seq_off[s + 1] - 1, B_s of them.  Per-pair outputs [B] are indexed by the pair's position in the run, sequence s owns the
 *     pose rows seq_off[s] + s .. seq_off[s + 1] + s, and segment, cause, seg_poses_pnp, seg_poses are vo_slam_chains_restart's
 *     with vo_slam_stream_restart's meaning in a resumed call.  n_carried [S], carried_frame [S][max_cameras] and carried_poses
 *     [S][max_cameras][12] are vo_slam_stream_restart's per sequence; carried_frame counts along the sequence's own stream.
 *     opts->snapshot_pair counts along the call's pairs of sequence snapshot_seq.
 *   resume = 0 starts the stream and drops the one it replaces: every B_s >= 1; vo_slam_chains_restart's checks (NO FRAME SLOT
 *     MAY BELONG TO TWO SEQUENCES, every sequence a chain of distinct frames, ratio matches VO_ERR_UNSUPPORTED);
 *     total_pairs[s] >= B_s sizes sequence s's lists once by vo_slam_stream's formulas.  The slot-keyed tables get two ghost rows
 *     per sequence behind the max_frames slots, rows max_frames + 2 s and + 2 s + 1 (max_frames + 2 S < 2^20).
 *   resume = 1 continues it: the same S, K and options (the snapshot's excepted); total_pairs is ignored.  Pair 0 of every
 *     sequence that advances starts at that sequence's anchor slot, the slot of its last frame.  B_s = 0 IS ALLOWED — seq_off is
 *     then only non-decreasing — as long as one sequence advances: an idle sequence keeps its anchor, its map and its restart
 *     state, owns one pose row (its anchor's, unchanged), reports n_carried[s] = 0, and continues in a later call as if the
 *     idle calls had not happened.
 *   The slot rule: after any call every slot except the S anchor slots is free for any sequence; an idle sequence holds only
 *     its anchor.  (Every sequence is carried at the start of every resumed call, advancing or not, and a carry clears the rows
 *     of the slots its own sequence's frames had and no others.)
 *   Refusals (VO_ERR_INVALID; the whole stream stays as it was and continuable): no live multi-stream; another S; an
 *     advancing sequence whose anchor slot was uploaded to or detected again; any anchor slot, an idle sequence's included, among
 *     another sequence's pairs; a pair 0 that does not start at its anchor; total_pairs[s] would be passed; K or an option
 *     changed; every sequence idle.  Ratio matches: VO_ERR_UNSUPPORTED.
 *   Stream kinds: vo_slam_stream and vo_slam_stream_restart refuse to continue a stream begun here and vo_slam_streams refuses
 *     to continue one of theirs (VO_ERR_INVALID, the stream unharmed); a resume = 0 call of any of the three drops whatever
 *     stream there is, as a configure call or a vo_slam_chain* call does.
 *   Maps: vo_slam_chains_map_size / vo_slam_chains_map report sequence seq after every call (which = 1: the snapshot, for seq ==
 *     snapshot_seq), cam_frame and pt_feature[:, 0] counted along that sequence's own stream; vo_slam_map reports sequence 0.
 * How: vo_slam_chains_restart's host loop — every kernel once per step j = 0 .. max B_s - 1 with the sequence on a grid axis —
 * on the stream / restart kernel bodies (k_slam_*_stream_restart_seqs), with one k_slam_carry_restart_seqs launch in front.
 * [deviation] none in the results.
 * Out of scope: a multi-stream without restart, changing S of a live stream (a flight that ends hands its seat to the next:
 * vo_slam_streams_replace, below), sequences that share a slot, joining segments or shards into one gauge, relocalisation from inside the walk,
 * pruning, ratio matches. */
int vo_slam_streams(vo_ctx* ctx, int resume, int S, const int32_t* total_pairs /*[S]*/, const int32_t* seq_off /*[S+1]*/,
                    const double* K, const vo_slam_opts* opts, int snapshot_seq,
                    double* poses_pnp /*(B+S)x12*/, double* poses /*(B+S)x12*/,
                    int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam /*[B] each*/,
                    double* chi2 /*[B][2]*/, int32_t* ba_iterations_run, int32_t* ba_trials_run /*[B] each*/,
                    int32_t* segment /*[B]*/, int32_t* cause /*[B]*/, double* seg_poses_pnp /*[B][12]*/, double* seg_poses /*[B][12]*/,
                    int32_t* n_carried /*[S]*/, int32_t* carried_frame /*[S][max_cameras]*/, double* carried_poses /*[S][max_cameras][12]*/);

/* ------------------------------------------------------------------ seats: a sequence takes a new flight when its own has ended
 * With flights of unequal length a fixed set of S sequences leaves seats idle: a step costs nearly the same whether 1 or S
 * sequences work in it.  A sequence index of a multi-stream is a SEAT; a seat is either held by a flight or VACANT.
 * The contract is the family's one equality: for every flight, the calls from the one in which it took its seat to its last
 * together compute the bytes a vo_slam_stream_restart stream computes for that flight alone with the same chunking — every
 * output, vo_slam_chains_map after every call, vo_slam_stats — whichever seat it takes, whatever flight sat there before (longer,
 * shorter, ended lost, carried many times), whatever the other seats do, whichever slots are used, and whether the stream began
 * with vo_slam_streams(resume = 0) or vo_slam_streams_open.  A seat nobody replaces keeps the bytes it had without these entries.
 *   vo_slam_streams_open: a multi-stream of S vacant seats.  What vo_slam_streams(resume = 0) does before its walk — drops the
 *     stream there is, checks S, K and the options, allocates and clears — and no walk: it needs a batch configuration and no
 *     vo_pairs_run.  total_pairs[s] >= 1 is the seat's CAPACITY: it sizes the seat's lists as resume = 0 sizes them.  The stream
 *     keeps the statistics setting (vo_set_slam_stats) the context has at this call.  Every later call is vo_slam_streams(resume = 1).
 *   vo_slam_streams_replace, between two calls of a live multi-stream: the flight of seat seq is over, the seat is vacant and its
 *     anchor slot is free at once.  Host only, nothing is launched.  total_pairs is the bound of the next flight that takes the
 *     seat, 1 .. the seat's capacity (what resume = 0 or open was given for it).  Replacing a vacant seat only sets the bound.
 *     Refusals (VO_ERR_INVALID, the stream untouched and continuable): no live multi-stream; a stream of the single kinds; seq
 *     out of range; total_pairs out of range.
 *   A vacant seat in vo_slam_streams(resume = 1): it may be idle (B_s = 0) — it owns no anchor, so nothing of it appears in the
 *     slot checks; it owns one pose row, all zero; n_carried[s] = 0 — or advance (B_s >= 1): a new flight takes the seat.  Its pair
 *     0 may start at any slot no other sequence holds, and for it everything counts from zero: frame0, the pairs done, n_carried
 *     = 0; segments are numbered from 0 with cause = 0 at its first pair; pose row 0 is the first camera, as at a stream's pair 0;
 *     cam_frame and pt_feature[:, 0] of vo_slam_chains_map and vo_slam_stats count along the new flight.  After the first call
 *     following a replace in which the seat stays vacant its map reports as empty.  "Every sequence idle" stays refused.
 * How: the seat is reset on the device by the carry launch of the next resumed call, before k_chain_link — other sequences may
 * already have frames in the slots it gave up.  A call of a stream with no vacant seat launches the kernels it launched before; a
 * call with one launches k_slam_carry_restart_seats instead of k_slam_carry_restart_seqs: a seat whose flight goes on runs the
 * same carry, a replaced one the reset (slam_kernels.hip), a vacant one that was reset already returns at once.
 * [deviation] none in the results.
 * Out of scope: changing S of a live stream, a flight with another K or other options than the stream's, a bound above the
 * seat's capacity, seats for vo_slam_stream / vo_slam_stream_restart, sequences that share a slot, joining flights or segments
 * into one gauge. */
int vo_slam_streams_open(vo_ctx* ctx, int S, const int32_t* total_pairs /*[S]*/, const double* K, const vo_slam_opts* opts);
int vo_slam_streams_replace(vo_ctx* ctx, int seq, int total_pairs);

/* ------------------------------------------------------------------ Map.show_map_statistics (src/map.py:234-297) on the device
 * The second thing VisualSlam.run() does per frame (src/visual_slam.py:354), as numbers (nothing is printed).  For a map given as
 * its three dense lists in the reference's append order:
 *   total_sqerr  calculate_reprojection_error() (:72-97): the observations' squared reprojection errors — the value
 *                vo_reprojection_filter reports for each — ADDED IN OBSERVATION ORDER STARTING FROM 0.0, one after the other, as
 *                the reference's loop does: the bytes are those of that sequential sum.  (The mean of :240-241 is total / nobs.)
 *   max_sqerr    the largest of them: m = 0.0; if (e > m) m = e — a NaN never becomes the maximum.
 *   n_high       how many have sqerr > high_threshold (the "high reprojection error" lines of :92; the reference's threshold is 10).
 *   obs_hist     [VO_STATS_HIST]: bin k = points of the list with exactly k observations, the last bin = points with
 *                VO_STATS_HIST - 1 or more (:245-254).  Bin 0, points that have no observation, is an addition: the reference's
 *                defaultdict does not see them.
 *   obs_matrix   [ncam][ncam], indices = positions in the camera list (:267-297): for every point, every pair of its observations
 *                whose cameras differ adds 1 at [min(c1, c2)][max(c1, c2)].  Two observations of one point in one camera pair with
 *                nothing between themselves and each with every observation in other cameras.  Diagonal and lower triangle: 0.
 * vo_map_statistics: one map from host arrays, arguments as vo_reprojection_filter (poses ncam x 16).  More than VO_BA_MAX_CAMERAS
 * cameras: VO_ERR_UNSUPPORTED; an observation of a missing camera or point: VO_ERR_INVALID.  An empty map is legal: all zeros.
 *
 * vo_set_slam_stats(ctx, on): a switch of the context, off by default.  While it is off no vo_slam_* entry launches or allocates
 * anything for statistics.  While it is on, every vo_slam_chain / vo_slam_chains[_restart] / vo_slam_stream[_restart] /
 * vo_slam_streams call runs one more kernel per step, after the camera limit (after snapshot stage 4), with high_threshold = 10:
 * row p describes the map state that n_pts[p], n_obs[p], n_cam[p] describe (zeros wherever those are zero; a pair that was not
 * localised reports the map it left untouched).  A stream keeps the setting it was started with: a resume = 1 call under the
 * other setting is refused (VO_ERR_INVALID, the stream unharmed).
 * vo_slam_stats: the rows of sequence seq (0 for the single-sequence entries) of the most recent vo_slam_* call.  B = that
 * sequence's pairs in the call, C >= the call's max_cameras.  cam_frame [B][C]: the map's camera list at that pair, -1 past
 * n_cam[p], counted as vo_slam_map counts it (along the stream in the stream forms).  VO_ERR_INVALID when the call ran with
 * statistics off, when the sizes do not fit, or after anything that forgets the maps.  vo_slam_stats_size reports B and
 * max_cameras of such a sequence, vo_slam_stats_counts the three list lengths the rows were computed on (show_map_statistics'
 * first three lines; n_obs is the divisor of the mean). */
#define VO_STATS_HIST 64
int vo_map_statistics(vo_ctx* ctx, const double* poses /*[ncam][16]*/, int ncam, const double* points, int npt,
                      const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs, const double* K, double high_threshold,
                      double* total_sqerr, double* max_sqerr, int32_t* n_high, int32_t* obs_hist /*[VO_STATS_HIST]*/,
                      int32_t* obs_matrix /*[ncam][ncam]*/);
int vo_set_slam_stats(vo_ctx* ctx, int on);
int vo_slam_stats_size(vo_ctx* ctx, int seq, int32_t* B, int32_t* max_cameras);
int vo_slam_stats_counts(vo_ctx* ctx, int seq, int B, int32_t* n_cam /*[B]*/, int32_t* n_pts /*[B]*/, int32_t* n_obs /*[B]*/);
int vo_slam_stats(vo_ctx* ctx, int seq, int B, int C, double* total_sqerr /*[B]*/, double* max_sqerr /*[B]*/, int32_t* n_high /*[B]*/,
                  int32_t* obs_hist /*[B][VO_STATS_HIST]*/, int32_t* obs_matrix /*[B][C][C]*/, int32_t* cam_frame /*[B][C]*/);

/* ------------------------------------------------------------------ relocalisation: a resident frame placed in a map by its descriptors
 * What the reference carries and never uses: TrackedPoint keeps match.descriptor1 for every map point (src/visual_slam.py:72-76,
 * :102-106) and MatchWithMap has descriptor1 (image), descriptor2 (map) and a distance that is always `0  # TODO: Set to the proper
 * feature distance` (:211-217).  Localisation there, and in vo_tracks_pnp_batch / vo_slam_*, goes through feature tracks from the
 * previous frame only; a frame without a track into the map — after a loss, a loop frame, another camera's frame — cannot be placed.
 * These entries place it: for a staged map of npt points (xyz float64, one descriptor row each) and Q detected slots,
 *   1 matches = bf.match(frame descriptors, map descriptors) of cv2.BFMatcher(NORM_L2 for SIFT rows / NORM_HAMMING for ORB rows,
 *     crossCheck=True): query = frame, train = map (MatchWithMap's orientation); strict mutual nearest neighbours, the lowest index
 *     winning ties in both directions (vo_pair_opts.match_mode 0); ascending keypoint order; distance as cv2 reports it, float32:
 *     sqrtf((float)d^2) for SIFT rows, the integer as float for ORB rows — the value the reference's TODO asks for.  Then
 *     `m.distance < max_distance`, strict, the float32 value against the double (visual_odometry_template_02/visual_slam.py:205-208);
 *     max_distance <= 0: no filter.  That is map-match mode 0, the default; vo_set_map_match (below) selects Lowe's ratio rule on
 *     knnMatch(k=2) in its place (mode 1) or on top of it (mode 2).
 *   2 correspondences in match order: obj[k] = the map point of trainIdx, img[k] = float64(kp_xy[queryIdx]).
 *   3 cv2.solvePnPRansac(obj, img, K, zeros(4)) with pnp_iterations, reproj_err, confidence, seed (cv2: 100, 8.0, 0.99, 2^64 - 1) and
 *     the context's vo_set_pnp_refine mode: exactly vo_solve_pnp_ransac_batch on those arrays (k_pnp_ransac, unchanged).
 *     poses[q] = [Rodrigues(rvec) | tvec], world -> camera IN THE MAP'S OWN GAUGE.  status[q]: VO_OK; VO_ERR_TOO_FEW (fewer than 4
 *     correspondences: cv2 raises) or VO_ERR_NO_MODEL (retval False), pose zeros; a model with fewer than min_inliers inliers becomes
 *     VO_ERR_NO_MODEL, pose zeros, its n_inl still reported.  A failed query does not touch the others.
 * Nothing returns to the host between the three steps.  Two calls on the same input return the same bytes.
 *
 * vo_map_stage: the map from host arrays — rows [npt][D], D = 32 under an ORB batch configuration and 128 (values 0..255) under a
 *   SIFT one; points [npt][3].  The parity seam, and how a caller brings back a map saved earlier (vo_map_rows).  npt 0 .. 65536;
 *   more: VO_ERR_UNSUPPORTED.  VO_ERR_NOT_CONFIGURED before a batch configuration.  VO_ERR_INVALID for a SIFT row with |row|^2 > 2^20,
 *   the bound the integer matcher's order rests on (vo_stage_sift_rows' rule); no map is staged then.
 * vo_map_from_slam: the map of the latest vo_slam_chain (seq = 0) or of sequence seq of the latest vo_slam_chains[_restart]; which as
 *   in vo_slam_map.  Copied ON THE DEVICE, no host round trip: the coordinates as the map's list holds them, and per point the
 *   descriptor row of its owning feature, gathered from the slot it was detected in (pt_feature -> chain frame -> slot of the latest
 *   vo_pairs_run, keypoint): TrackedPoint.descriptor = match.descriptor1.  The slots must still hold those frames.  VO_ERR_INVALID
 *   where vo_slam_map / vo_slam_chains_map would refuse, and when another call has laid out the context's scratch buffer since the
 *   chain ran (the single-call operators, vo_tracks_pnp_batch, another chain): call it right after the chain.  VO_ERR_UNSUPPORTED for
 *   a stream's map (vo_slam_stream*, vo_slam_streams): its older frames have left their slots and their descriptor rows are gone —
 *   unless the stream is a vo_slam_stream that keeps a descriptor store (vo_set_stream_rows, below): then (0, 0) is
 *   vo_map_from_stream(0, -1), and which = 1, the snapshot, stays VO_ERR_UNSUPPORTED.
 * vo_set_stream_rows / vo_stream_rows_info / vo_map_from_stream: a stream's own descriptor store.  With it a vo_slam_stream keeps the
 *   descriptor row of every map point on the device from the call the point is born in, in an allocation of the stream's lifetime
 *   beside the walk's (capacity_rows D + 4 (total_pairs + 1) kp_cap bytes, D = 32 / 128), and its live map can be staged at any
 *   later time — after the frames have lost their slots, between two calls, after a call that ended lost.
 *   vo_set_stream_rows: capacity_rows 0 = no store (the default: every call then returns the bytes and the refusals it returns
 *     without this section), -1 = (total_pairs + 1) kp_cap rows, which can never drop a point, > 0 = that many rows (at most
 *     2^31 - 1: VO_ERR_INVALID at the call that starts the stream), < -1: VO_ERR_INVALID.  It takes effect at the next
 *     vo_slam_stream(resume = 0); a live stream keeps the setting it started with (vo_set_slam_stats' rule).  vo_slam_stream_restart,
 *     vo_slam_streams and the chains ignore it.
 *   Append, at the end of every vo_slam_stream call (resume 0 or 1, also one that ends lost), one launch behind the walk while the
 *     call's frames are in their slots: every point of the end map whose owning frame is one of this call's and whose feature has no
 *     row takes the next free row IN MAP ORDER, and the row of its owning feature (the one vo_map_from_slam gathers) is copied there.
 *     A point that finds the store full is counted as dropped and stays without a row for good; which points those are is a
 *     function of the inputs alone.  A point born and removed inside one call never gets a row; a row whose point is removed later
 *     stays as a hole (the store is not compacted; the store serves the LIVE map: a point the camera limit has removed is gone from
 *     it, whatever its row).  The walk's kernels are untouched: with the store on, every output of the
 *     stream is the bytes it is with the store off.
 *   vo_stream_rows_info: the live stream's store: rows it holds, rows handed out, points dropped.  VO_ERR_INVALID without a live
 *     vo_slam_stream that has a store.
 *   vo_map_from_stream: stages the live stream's end map restricted to the points whose owning frame (pt_feature's frame, along the
 *     stream) lies in [frame_first, frame_end); frame_end < 0: no upper bound.  Points and rows in map order, as vo_map_from_slam
 *     stages a chain's map; points without a row are left out and counted in n_without_row.  An empty selection stages an empty
 *     map.  VO_ERR_INVALID: no live vo_slam_stream with a store, frame_first < 0, 0 <= frame_end < frame_first.  VO_ERR_UNSUPPORTED:
 *     more than 65536 points selected.  A failed call leaves no staged map.  The stream, the pair results and vo_slam_map's copies
 *     are left alone: a later resume = 1 returns what it would have returned without the call.
 * vo_set_stream_archive / vo_stream_archive_info / vo_stream_archive_read / vo_map_from_stream_archive: a stream's archive of the
 *   points the camera limit has removed.  The store serves the live map; with max_cameras = 18 a long flight that returns to its
 *   start has nothing of its start left to match against.  With the archive every point k_slam_limit removes is kept on the device,
 *   in removal order, in one more allocation of the stream's lifetime: capacity_points (D + 40) bytes, plus 8 bytes per 256 entries
 *   for the selection's tile counts and the 1.75 MiB of selection buffers.
 *   vo_set_stream_archive: capacity_points 0 = no archive (the default: every call then returns the bytes and the refusals it
 *     returns without this paragraph), -1 = (total_pairs + 1) kp_cap entries, which can never drop a point, > 0 = that many entries
 *     (at most 2^31 - 1: VO_ERR_INVALID at the call that starts the stream), < -1: VO_ERR_INVALID.  Read by the next
 *     vo_slam_stream(resume = 0); a live stream keeps the setting it started with.  An archive needs the store: the frames of
 *     earlier calls have no slot, so their points' rows can only come from it — resume = 0 with the archive on and
 *     vo_set_stream_rows off is VO_ERR_INVALID and starts nothing.  vo_slam_stream_restart, vo_slam_streams and the chains ignore it.
 *   What is archived: at every step whose camera limit evicts a camera, exactly the points that step removes, by the limit's own
 *     rule (observations counted among cameras other than the first; a point left with exactly one goes, a point with none stays),
 *     in map order; evictions follow one another in pair order.  An entry holds feature = pt_feature (frame along the stream,
 *     keypoint), xyz = the three doubles the limit read, evicted_at = the pair along the stream, and a COPY of the descriptor row:
 *     from the slots by the point's key when the point was born in this call (feature frame >= the call's first frame), otherwise
 *     from the store, otherwise none (has_row = 0, the row reads zeros: the store dropped the point at capacity).  The archive
 *     owns its rows, so an entry is complete however the flight was chunked into calls.  A full archive counts the remaining
 *     points as dropped, for good: the entries kept are the first in that order, so which are dropped follows from the inputs
 *     alone.  No deduplication: a removed point's feature may later own a new point, and both are legitimate — the same feature can
 *     occur in several entries, or in an entry and in the live map.  With the archive on, every output of the stream, its map
 *     after every call and the store are the bytes they are with it off.
 *   vo_stream_archive_info: entries it holds, entries stored, points dropped.  VO_ERR_INVALID without a live vo_slam_stream that
 *     has an archive.
 *   vo_stream_archive_read: entries first .. first + n - 1 back on the host, for tests and for saving; any pointer may be NULL.
 *     VO_ERR_INVALID without such a stream, or when the range is not among the stored entries.
 *   vo_map_from_stream_archive: vo_map_from_stream's window rule over the archive.  with_live = 1 stages the live points of the
 *     window first, exactly as vo_map_from_stream stages them, then the archived entries of the window that have a row, in archive
 *     order (on a duplicated row the live point wins the cross-check's lowest-index tie); with_live = 0 the archived entries only.
 *     n_staged = points staged, n_archived = the archived ones among them, n_without_row = points of the window left out (live
 *     and archived).  The staged map is the bytes vo_map_stage produces from the same rows and points (SIFT: the int8 operand
 *     image, the norms and the norm flag included: the one row store).  VO_ERR_UNSUPPORTED: more than 65536 points selected;
 *     VO_ERR_INVALID: no live vo_slam_stream with an archive, or no window.  A failed call leaves no staged map.  The stream is
 *     left as it was.  vo_map_from_stream itself is unchanged.
 * vo_map_rows: the staged map back (up to cap points; *npt = its size): what a caller saves before the frames leave their slots.
 * vo_map_localize: Q <= max_pairs detected slots against the staged map in one call.  No staged map: VO_ERR_INVALID.  A slot flagged
 *   for its descriptor norm (SIFT): VO_ERR_INVALID AFTER the run, as vo_pairs_run reports it.  Profiling stages: match_nn (k_nn_map),
 *   match_select (k_map_select), misc (k_pnp_ransac and the poses).
 * vo_map_matches: query q's match list of the latest vo_map_localize — map point, keypoint, distance — and solvePnPRansac's inlier
 *   mask (0 / 1) over it.
 * vo_set_map_match: the rule by which vo_map_localize AND vo_map_align match rows against the staged map; a context setting like
 *   vo_set_pnp_refine: read by the next of those calls, kept across staging and configure calls.
 *     mode 0 (default): the cross-check of step 1; `ratio` is not read.  Every byte those calls return is what it is without this entry.
 *     mode 1: the ratio rule of src/feature_detection.py:20-26 against the map.  For query row i (a keypoint / a query map's row:
 *       cv2's query) and the staged map as train, m, n = knnMatch(k=2): batchDistance's K = 2 insertion — ascending scan, strict `<`,
 *       equal distances keep train order — so m.trainIdx is the lowest index among the nearest rows and n.distance the second-smallest
 *       distance, a tie with m counting as a second neighbour.  Row i is kept iff the staged map has at least 2 rows and
 *       (double)fd < ratio * (double)fd2, fd and fd2 the float32 distances cv2 reports (sqrtf((float)d^2) for SIFT rows, the integer as
 *       float for ORB rows): vo_pair_opts.match_mode 1's expression.  A map of 0 or 1 rows gives no match.  No reverse direction is
 *       computed.  Several query rows may keep one map point; all of them stay in the list.
 *     mode 2: the cross-check AND the ratio rule: mode 0's list filtered by mode 1's rule on the forward neighbours.  This library's own
 *       combination (cv2 refuses knnMatch(k=2) on a crossCheck matcher).
 *     In every mode `m.distance < max_distance` applies as in step 1, strictly and conjunctively, and the list is in ascending query
 *     order.  Statuses are unchanged: fewer than 4 (vo_map_localize) or 3 (vo_map_align) correspondences is VO_ERR_TOO_FEW.
 *     VO_ERR_INVALID: a mode other than 0, 1, 2; in modes 1 and 2 a ratio that is not finite or not > 0.
 * vo_map_match_seconds: n.distance (float32) for every entry of query q's match list, in list order; which = 0 the latest
 *   vo_map_localize, 1 the latest vo_map_align.  FLT_MAX where there is no second neighbour.  The parity seam of the top-2 selection,
 *   and what a caller needs to re-threshold on the host without another run.  VO_ERR_INVALID when that call ran in mode 0, and where
 *   vo_map_matches / vo_map_align_matches would refuse q.
 * Lifetime: the staged map and vo_map_localize's work buffers are an allocation of their own, released by vo_destroy and by a
 *   configure call.  vo_pairs_run, the vo_slam_* calls and detections leave it alone; vo_map_localize leaves the pair results, the
 *   chain's maps and a live stream alone.  A new vo_map_stage / vo_map_from_slam replaces the map (also when it fails).
 * Out of scope: automatic use inside the walks, a descriptor store for restart streams and multi-streams (vo_slam_stream_restart,
 * vo_slam_streams) and the archive of earlier segments they would need, staging a window of more than 65536 points, knnMatch with
 * k > 2 against the map.  (The similarity that joins two segments' gauges: map alignment, below.  Matching by projection under a
 * prior pose: guided relocalisation, below; vo_map_matches and vo_map_match_seconds(0, ...) serve the latest call of either kind.) */
typedef struct {
    double   max_distance;      /* 0: no filter */
    int32_t  pnp_iterations;    /* 100 */
    double   reproj_err;        /* 8.0 */
    double   confidence;        /* 0.99 */
    uint64_t seed;              /* 0xFFFFFFFFFFFFFFFF */
    int32_t  min_inliers;       /* 0 */
} vo_reloc_opts;
int vo_map_stage(vo_ctx* ctx, const uint8_t* rows /*[npt][D]*/, const double* points /*[npt][3]*/, int npt);
int vo_map_from_slam(vo_ctx* ctx, int seq, int which);
int vo_set_stream_rows(vo_ctx* ctx, int64_t capacity_rows);
int vo_stream_rows_info(vo_ctx* ctx, int64_t* capacity, int64_t* stored, int64_t* dropped);
int vo_map_from_stream(vo_ctx* ctx, int frame_first, int frame_end, int32_t* n_staged, int32_t* n_without_row);
int vo_set_stream_archive(vo_ctx* ctx, int64_t capacity_points);
int vo_stream_archive_info(vo_ctx* ctx, int64_t* capacity, int64_t* stored, int64_t* dropped);
int vo_stream_archive_read(vo_ctx* ctx, int64_t first, int64_t n, int32_t* feature /*[n][2]*/, double* xyz /*[n][3]*/, int32_t* evicted_at /*[n]*/,
                           int32_t* has_row /*[n]*/, uint8_t* rows /*[n][D]*/);
int vo_map_from_stream_archive(vo_ctx* ctx, int frame_first, int frame_end, int with_live, int32_t* n_staged, int32_t* n_archived,
                               int32_t* n_without_row);
int vo_map_rows(vo_ctx* ctx, uint8_t* rows /*[cap][D]*/, double* points /*[cap][3]*/, int cap, int32_t* npt);
int vo_map_localize(vo_ctx* ctx, const int32_t* slots, int Q, const double K[9], const vo_reloc_opts* opts,
                    double* poses /*[Q][12]*/, int32_t* n_match, int32_t* n_inl, int32_t* status);
int vo_map_matches(vo_ctx* ctx, int q, int32_t* pt_idx, int32_t* kp_idx, float* dist, uint8_t* inlier_mask, int cap, int32_t* n_out);
int vo_set_map_match(vo_ctx* ctx, int mode /*0 cross-check, 1 ratio, 2 both*/, double ratio);
int vo_map_match_seconds(vo_ctx* ctx, int which /*0 localize, 1 align*/, int q, float* dist2, int cap, int32_t* n_out);

/* ------------------------------------------------------------------ guided relocalisation: map points matched by projection
 * vo_map_localize compares every keypoint with every staged point: right when nothing is known about the frame's pose.  A caller
 * that holds a prior — a stream's drifted pose, the pose of a frame just relocalised from a few dozen inliers, the pose of the frame
 * before — projects the map with it and looks only at the keypoints in a window around each projection (ORB-SLAM's
 * SearchByProjection): look-alike descriptors elsewhere in the image cannot win, and the work per query drops from
 * npt x n_keypoints distances to a handful per point.  The reference has no counterpart; the rules are this library's own.
 * The frame is slot slots[q]: nq = min(kp_count, kp_cap) keypoints, keypoint i at (x_i, y_i) in float32 with one descriptor row;
 * the staged map has npt points X_j = (X, Y, Z) in float64 with one row each; P = prior[q], row-major 3 x 4.  Every operation below
 * is one float64 rounding, in the order written (the library is built with -ffp-contract=off).
 *   1 projection.  c_k = ((P[k][0] X + P[k][1] Y) + P[k][2] Z) + P[k][3], k = 0, 1, 2.  Point j takes part iff c_2 > 0 (strict; a
 *     NaN fails it).  xn = c_0 / c_2, yn = c_1 / c_2; u = (K[0] xn + K[1] yn) + K[2], v = (K[3] xn + K[4] yn) + K[5]: K's third row
 *     is not read.  There is no image-bounds test (vo_frames_undistort moves keypoints outside the image, and a batch configured
 *     for 32 x 32 may carry keypoints from anywhere).
 *   2 window.  Keypoint i is a candidate of point j iff dx dx + dy dy <= r2, dx = (double)x_i - u, dy = (double)y_i - v,
 *     r2 = radius radius computed once.  A u or v that is infinite or NaN has no candidate under this rule.
 *   3 distance.  d(i, j), the exact integer: Hamming for ORB rows, sum (a - b)^2 over the 128 uint8 values for SIFT rows (the rows as
 *     vo_stage_sift_rows / the detector store them, and as vo_map_rows returns the map's).  Reported as cv2 reports it, float32:
 *     fd = (float)d for ORB rows, sqrtf((float)d) for SIFT rows.
 *   4 per point.  best(j) = the candidate with the smallest (d, i), lexicographically: the lowest keypoint wins a tie.  d2(j) = the
 *     second-smallest d among the candidates as a multiset (a tie with the best counts as a second); fewer than two candidates:
 *     fd2 = FLT_MAX.  n_seen[q] = the points with at least one candidate.
 *   5 filters, per point, conjunctive.  opts->max_distance > 0: (double)fd < max_distance, strictly.  g->ratio > 0: the point is
 *     kept iff it has fewer than two candidates or (double)fd < ratio * (double)fd2 (vo_set_map_match mode 1's expression).
 *   6 one point per keypoint.  Among the points that pass step 5 and whose best is keypoint i, the one with the smallest (d, j)
 *     keeps it.  The filters come first: a point that fails them blocks nobody.
 *   7 the match list, in ascending keypoint order: (keypoint i, point j, fd, fd2), obj = X_j, img = (double)(x_i, y_i); at most nq
 *     entries.
 *   8 the pose: from here on exactly vo_map_localize's step 3 on those arrays — k_pnp_ransac unchanged, the same seed,
 *     pnp_iterations, reproj_err, confidence, min_inliers and vo_set_pnp_refine mode, the same statuses and zeroed poses.
 * vo_set_map_match is not read: the window rule has its own two options.  The result does not depend on scheduling: two calls on
 * the same input return the same bytes.
 * prior == NULL, the refinement pass: the priors are the poses of the most recent vo_map_localize on this staged map, taken from
 *   the device buffer (nothing returns to the host between the descriptor-only pose and the guided one) and copied aside before
 *   any work buffer is overwritten.  That call must have succeeded with the same Q and the same slots, and no vo_map_localize_guided
 *   may have run since (it overwrites those poses): otherwise VO_ERR_INVALID.  A query whose status there was not VO_OK is not
 *   matched: it keeps that status, with n_match = n_inl = n_seen = 0 and a zero pose.
 * After the call vo_map_matches serves the most recent of vo_map_localize and vo_map_localize_guided, and
 *   vo_map_match_seconds(0, q, ...) is valid after a guided call whatever `ratio` was.  A later vo_map_localize returns the bytes it
 *   returns without this section.  The staged map, the pair results, the chains' maps and a live stream are left alone.
 * VO_ERR_INVALID, the whole call failing and nothing written: what vo_map_localize refuses; g == NULL; a radius that is negative or
 *   not finite; a ratio that is negative or not finite; a non-finite entry in a given prior; the prior == NULL conditions above.
 *   A slot flagged for its descriptor norm (SIFT): VO_ERR_INVALID AFTER the run, as vo_map_localize reports it.
 * Profiling stages: match_nn (k_guided_grid, k_guided_match), match_select (k_guided_select), misc (k_pnp_ransac and the poses).
 * Out of scope: use inside the walks, octave and scale prediction, viewing-angle tests, more than one point per keypoint. */
typedef struct {
    double radius;              /* pixels, finite, >= 0 */
    double ratio;               /* 0: no ratio rule; else finite and > 0 */
} vo_guided_opts;
int vo_map_localize_guided(vo_ctx* ctx, const int32_t* slots, int Q, const double K[9],
                           const double* prior /*[Q][12] world -> camera in the map's gauge, or NULL*/,
                           const vo_guided_opts* g, const vo_reloc_opts* opts,
                           double* poses /*[Q][12]*/, int32_t* n_match, int32_t* n_inl, int32_t* status,
                           int32_t* n_seen /*[Q], may be NULL*/);

/* ------------------------------------------------------------------ map alignment: the similarity that joins two maps, by descriptors
 * After a lost frame the restart walks start a new map, and every segment is a trajectory in a gauge of its own: its origin is its
 * first camera, its unit its first pair's baseline.  A frame's pose in the other map (vo_map_localize) fixes rotation and translation
 * and says nothing about the ratio of the units; two MAPS that see the same ground fix all seven degrees of freedom.  The reference
 * has no counterpart (it re-initialises with self.map.clean() and forgets the old map), so the rules are this library's own, in the
 * spirit of cv::RANSACPointSetRegistrator as k_ransac and k_pnp_ransac follow it.  For one problem of n correspondences (b_i, a_i),
 * X_a = s R X_b + t, float64 throughout:
 *   Fit of m >= 3 points (Umeyama / Horn): centroids ac, bc; var_b = sum |b_i - bc|^2 / m; H = sum (a_i - ac)(b_i - bc)^T / m;
 *     H = U D V^T by the one-sided Jacobi SVD (rotations and threshold of the library's jacobi_svd, sigma descending);
 *     S = diag(1, 1, sign(det U det V)); R = U S V^T; s = tr(D S) / var_b; t = ac - s R bc.  The third column of U is taken as
 *     u1 x u2, so det U = +1, sign(det V) decides S and tr(D S) = sigma_1 + sigma_2 + sign(det V) u3 . (H v3): what any orthonormal
 *     completion gives, and well defined for the rank-2 H of a three-point sample, where the S branch is taken on about half of all
 *     samples.  No model when var_b == 0, when s, R or t is not finite, or when s <= 0.
 *   Subset check: a sample is rejected when, on either side (a or b), the difference vectors d1, d2 from its point 0 have
 *     |d1 . d2| > 0.996 sqrt(|d1|^2 |d2|^2), or one of them is zero — exactly that comparison, no division.  0.996 is this library's
 *     constant.  A rejected sample is an iteration that produced no model: it has consumed its random numbers and counts towards niters.
 *   Sampling: OpenCV's MWC stream from `seed` (the context's table, as k_pnp_ransac reads it); three indices next() % n, a repeat is
 *     redrawn immediately.
 *   Scoring: e_i = |s R b_i + t - a_i|^2 in float64, cast to float32; point i is an inlier iff e_i <= (float)(max_error^2).  max_error
 *     is in the units of map A.
 *   Update and stop: hypotheses are consumed in order; update iff good > max(best, 2), strictly; then niters =
 *     RANSACUpdateNumIters(confidence, (n - good) / n, 3, niters).  iterations < 1 counts as 1.
 *   n < 3: VO_ERR_TOO_FEW.  n == 3: one fit (the subset check applies), every point an inlier; rejected or no model: VO_ERR_NO_MODEL.
 *   Result: mask = the best RANSAC model's inlier mask, n_inl its count; the reported (s, R, t) is the same fit over the inliers (the
 *     arrangement of solvePnPRansac).  Fewer than min_inliers inliers, or a refit without a model: VO_ERR_NO_MODEL, the model zeroed,
 *     n_inl and the mask still reported.  A failed problem does not touch the others.  Two calls on the same input return the same bytes.
 *
 * vo_sim3_ransac_batch: the parity seam — B problems of given correspondences, problem b = rows offsets[b] .. offsets[b + 1] - 1 of
 *   src (b) and dst (a), [n][3] each; sim [B][13] = s, R row-major, t; mask over all rows.  max_distance is not read.  VO_ERR_INVALID:
 *   max_error <= 0, confidence outside (0, 1), decreasing offsets, missing arrays.
 * vo_map_align: Q query maps (rows [off[Q]][D] as vo_map_stage takes them, points [off[Q]][3], off [Q + 1] with off[0] == 0) against the
 *   staged map, in one call on the device: every query map is stored the way the staged one is (the same row store, the same norm
 *   bound: a flagged SIFT row is VO_ERR_INVALID for the call); matches = the cross-check match of query rows (cv2's query) against the
 *   staged rows (train) under vo_map_localize's rules — strict mutual nearest neighbours, lowest index winning ties in both
 *   directions, float32 `distance < max_distance` (<= 0: no filter), ascending query-row order; b = the query's point, a = the staged
 *   point (vo_set_map_match modes 1 and 2: the ratio rule stated there, with the query map's rows as cv2's query, in the place of or on
 *   top of the cross-check; vo_map_match_seconds(which = 1) returns the second distances); then exactly vo_sim3_ransac_batch on those lists.  sim[q] takes query map q's gauge to the staged map's.  An empty query map
 *   is VO_ERR_TOO_FEW for that query alone.  VO_ERR_UNSUPPORTED: Q > 64, off[Q] > 65536.  VO_ERR_INVALID: no staged map, max_error <= 0,
 *   confidence outside (0, 1), off[0] != 0 or decreasing offsets.  Profiling stages: match_nn, match_select, misc.
 * vo_map_align_matches: query q's match list of the latest vo_map_align — staged row, query row, distance — and the inlier mask.
 * Lifetime: the query maps and work buffers are an allocation of their own, made by the first vo_map_align and ended with the staged
 *   map's; a newly staged map forgets the queries.  The pair results, the chains' maps, a live stream and vo_map_localize's results
 *   are left alone.
 * Out of scope: a descriptor store for restart streams and multi-streams and an archive of their earlier segments (a vo_slam_stream
 * has one: vo_set_stream_rows), automatic joining inside the walks, staging a window of more than 65536 points, bundle refinement after
 * the join (the pose-graph refinement is vo_pose_graph, below). */
typedef struct {
    double   max_distance;      /* descriptor filter as in vo_reloc_opts; 0: none */
    double   max_error;         /* inlier bound in map A's units; > 0 */
    int32_t  iterations;        /* 1000 */
    double   confidence;        /* 0.99 */
    uint64_t seed;              /* 0xFFFFFFFFFFFFFFFF */
    int32_t  min_inliers;       /* 0 */
} vo_align_opts;
int vo_sim3_ransac_batch(vo_ctx* ctx, const double* src /*b*/, const double* dst /*a*/, const int32_t* offsets /*[B + 1]*/, int B,
                         const vo_align_opts* opts, double* sim /*[B][13]*/, uint8_t* mask, int32_t* n_inl, int32_t* status);
int vo_map_align(vo_ctx* ctx, const uint8_t* rows, const double* points, const int32_t* off /*[Q + 1]*/, int Q, const vo_align_opts* opts,
                 double* sim /*[Q][13]*/, int32_t* n_match, int32_t* n_inl, int32_t* status);
int vo_map_align_matches(vo_ctx* ctx, int q, int32_t* a_idx, int32_t* b_idx, float* dist, uint8_t* inlier_mask, int cap, int32_t* n_out);

/* ------------------------------------------------------------------ guided map alignment: two maps' points matched in space
 * vo_map_align matches query rows against staged rows by descriptor alone: look-alike rows anywhere in the other map win or block a
 * match, the weakness vo_map_localize_guided removed for frames.  Once a similarity is known — from the descriptor-only call, from a
 * loop edge, from join_segments — the question is spatial: for each query point moved into the staged map's gauge, which staged point
 * lies within a radius of it and has the nearest descriptor?  (The 3D-3D half of ORB-SLAM's SearchAndFuse.)  On that result the
 * similarity is refitted from many more inliers.  The reference has no counterpart; the rules are this library's own.
 * Query map q holds points b_i and rows off[q] .. off[q + 1] - 1 of the caller's arrays; the staged map holds points a_j with one row
 * each; S = prior[q] = s, R row-major, t, taking the query map's gauge to the staged map's.  Every operation below is one float64
 * rounding, in the order written (the library is built with -ffp-contract=off).
 *   1 transform.  y_k = s * ((R[k][0] bx + R[k][1] by) + R[k][2] bz) + t_k, k = 0, 1, 2.  Point i takes part iff all three y_k are
 *     finite.
 *   2 window.  Staged point j is a candidate of i iff (dx dx + dy dy) + dz dz <= r2, d = a_j - y componentwise, r2 = radius radius
 *     computed once.  g->radius is a length in the STAGED map's units here (in vo_map_localize_guided it is pixels).  A staged point
 *     with a coordinate that is not finite is never a candidate under this rule.
 *   3 distance.  d(i, j), the exact integer: Hamming for ORB rows, sum (a - b)^2 over the 128 raw uint8 values for SIFT rows (the rows
 *     as vo_map_stage and vo_map_align take them).  Reported as cv2 reports it, float32: fd = (float)d for ORB rows,
 *     sqrtf((float)d) for SIFT rows.
 *   4 per query point.  best(i) = the candidate with the smallest (d, j), lexicographically: the lowest staged point wins a tie.
 *     d2(i) = the second-smallest d among the candidates as a multiset (a tie with the best counts as a second); fewer than two
 *     candidates: fd2 = FLT_MAX.  n_seen[q] = the query points with at least one candidate.
 *   5 filters, per query point, conjunctive.  opts->max_distance > 0: (double)fd < max_distance, strictly.  g->ratio > 0: the point
 *     is kept iff it has fewer than two candidates or (double)fd < ratio * (double)fd2.
 *   6 one query point per staged point.  Among the points that pass step 5 and whose best is j, the one with the smallest (d, i)
 *     keeps j.  The filters come first: a point that fails them blocks nobody.
 *   7 the match list of query q, in ascending query-row order: (query row i, staged row j, fd, fd2), src = b_i (the untransformed
 *     point), dst = a_j; fd2 is there for every entry.
 *   8 the similarity: from here on exactly vo_map_align's tail — k_sim3_ransac unchanged on those lists, the same max_error,
 *     iterations, confidence, seed and min_inliers, the same statuses, failed models zeroed the same way.
 * vo_set_map_match is not read.  The result does not depend on scheduling: two calls on the same input return the same bytes.
 * rows == points == off == prior == NULL, the refinement pass: the query maps are the ones the most recent vo_map_align on this staged
 *   map left on the device and the priors are the sims it left there; nothing is uploaded and nothing returns to the host in between,
 *   and the sims are copied aside before any work buffer is overwritten.  Q must equal that call's Q, no map may have been staged
 *   since and no vo_map_align_guided may have run since (it overwrites those sims): otherwise VO_ERR_INVALID.  A query whose status
 *   there was not VO_OK is not matched: it keeps that status, with n_match = n_inl = n_seen = 0 and a zero sim.  A second pass takes
 *   its priors explicitly.
 * After the call vo_map_align_matches and vo_map_match_seconds(1, q, ...) serve the most recent of vo_map_align and
 *   vo_map_align_guided, and vo_map_match_seconds(1, q, ...) is valid after a guided call whatever `ratio` was.  A later vo_map_align
 *   returns the bytes it returns without this section.  Limits are vo_map_align's: Q <= 64, off[Q] <= 65536 (VO_ERR_UNSUPPORTED).
 * VO_ERR_INVALID, the whole call failing and nothing written: what vo_map_align refuses; g == NULL; a radius that is negative or not
 *   finite; a ratio that is negative or not finite; a non-finite entry in a given prior; some but not all of rows, points, off and
 *   prior NULL; the refinement conditions above.  A flagged SIFT row of a query map: VO_ERR_INVALID AFTER the run, as vo_map_align
 *   reports it.
 * Profiling stages: match_nn (k_fuse_grid, k_fuse_match), match_select (k_fuse_select), misc (k_sim3_ransac).
 * Merging the two maps afterwards — one list, each ground point once, and the table that says where every old point went — is host
 * work on these match lists: frontend.merge_maps, FrontEnd.fuse_map.
 * Out of scope: fusing on the device and inside the walks, redirecting a stream's observations, merged maps beyond 65536 points,
 * averaging the positions of fused points, a scale-aware or covariance-aware radius, a grid cached across calls on one staged map. */
int vo_map_align_guided(vo_ctx* ctx, const uint8_t* rows, const double* points, const int32_t* off /*[Q + 1]*/, int Q,
                        const double* prior /*[Q][13] s, R row-major, t: query gauge -> staged gauge*/,
                        const vo_guided_opts* g, const vo_align_opts* opts,
                        double* sim /*[Q][13]*/, int32_t* n_match, int32_t* n_inl, int32_t* status,
                        int32_t* n_seen /*[Q], may be NULL*/);

/* ------------------------------------------------------------------ pose graph: Sim(3) pose-graph optimisation on the device
 * The restart walks cut a flight into segments, vo_map_localize places a frame in an older map, vo_map_align measures the similarity
 * between two maps: a loop closure arrives as seven numbers.  This section uses it: loop and join constraints are distributed over
 * all poses of a flight, as ORB-SLAM's essential graph and g2o's types_sim3 do.  The reference has no counterpart and g2o is not
 * installed anywhere this project runs, so the rules are this library's own; the checker is tests/pose_graph_reference.py.
 *   Elements: S = (s, R, t) acts as x -> s R x + t; 13 doubles s, R row-major, t (vo_sim3_ransac_batch's `sim`).
 *   Tangent: d = (w, u, sigma) in R^7: rotation, translation, log-scale.  hat(d) = [[ [w]x + sigma I, u ], [0, 0]] (4x4);
 *     exp(d) = its matrix exponential: R = exp([w]x), s = e^sigma, t = V u, V = integral over [0, 1] of e^(tau sigma) exp(tau [w]x)
 *     = C I + A [w]x + B [w]x^2.  With th = |w| and the moments m_k(sigma) = integral of tau^k e^(tau sigma):
 *       th >= 1e-2: R from sin th / th and 2 sin^2(th / 2) / th^2; a = e^sigma sin th, 1 - b = 2 sin^2(th / 2) - expm1(sigma) cos th,
 *         c = th^2 + sigma^2, C = m_0, A = (a sigma + (1 - b) th) / (th c), B = (C - (a th - (1 - b) sigma) / c) / th^2;
 *       th <  1e-2: series to th^6 for R; A = m_1 - th^2 m_3 / 6 + th^4 m_5 / 120, B = m_2 / 2 - th^2 m_4 / 24 + th^4 m_6 / 720, C = m_0;
 *       |sigma| >= 1e-2: m_0 = expm1(sigma) / sigma, m_k = (e^sigma - k m_(k-1)) / sigma;
 *       |sigma| <  1e-2: m_k = sum over n = 0 .. 7 of sigma^n / (n! (n + k + 1)).
 *     log is the inverse, the rotation angle in [0, pi): the unit quaternion of R (Eigen's conversion, w >= 0), n = |(x, y, z)|,
 *     w = (2 atan2(n, q_w) / n) (x, y, z), below n = 1e-8 the factor is (2 / q_w)(1 - (n / q_w)^2 / 3); sigma = ln s; u = V^-1 t.
 *   Adjoint: Ad(S) = [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]] (blocks 3, 3, 1): S exp(d) S^-1 = exp(Ad(S) d).
 *   Vertices: vertex i is S_i, world -> camera i (a pose [R | t] of this library has s = 1).  Update S_i <- exp(d_i) S_i, stored as
 *     the product of the 13 numbers (no re-orthogonalisation).  A fixed vertex keeps its input bytes.
 *   Edges: edge k = (i, j, C_k, w_k[7]), w_k > 0: E_k = C_k S_i S_j^-1, e_k = log(E_k), chi2_k = sum w_k e_k^2.  Huber as in the bundle
 *     adjustment (rho = 2 delta sqrt(chi2_k) - delta^2 beyond delta, the weight is rho' only); huber_delta <= 0 turns it off.
 *     Jacobians, first order (exact at E_k = I): d e_k / d d_i = Ad(C_k), d e_k / d d_j = -Ad(E_k).
 *   Levenberg-Marquardt: exactly the bundle adjustment's rules (tau = 1e-5, lambda from the first linearisation, its nu and lambda
 *     updates, at most 10 trials per iteration, a non-positive Cholesky pivot is a failed trial, no convergence test, `iterations`
 *     fixed by the caller) with one change: rho = (chi2 - chi2_trial) / (d^T (lambda d + b)), without g2o's + 1e-3 (residuals here
 *     are radians and map units; chi2 itself is of the order 1e-3: docs/kernels/k_pose_graph.md).  A trial is rejected if that
 *     denominator is <= 0 or not finite, or if the trial chi2 is not finite.
 *   Capacity: an edge with |i - j| == 1 is a chain edge, every other a loop edge.  Per graph at most VO_PGO_MAX_VERTICES vertices and
 *     VO_PGO_MAX_LOOPS loop edges, any number of chain edges, duplicates included.  Beyond: VO_ERR_UNSUPPORTED in that graph's status,
 *     its data unchanged, the rest of the batch runs.
 *   Validity, each VO_ERR_INVALID for that graph alone, checked before capacity except the last: an index out of range, i == j, a
 *     weight <= 0 or not finite; a vertex that is not connected to a fixed vertex.  The call itself returns VO_ERR_INVALID for
 *     decreasing offsets, missing arrays or iterations outside 1 .. 1000.
 *   Determinism: two calls on the same input return the same bytes; a graph alone returns the same bytes as anywhere in a batch.
 * vo_pose_graph_batch: graph b = vertices vert_off[b] .. vert_off[b + 1] - 1 and edges edge_off[b] .. edge_off[b + 1] - 1; edge indices
 *   are local to the graph.  chi2[b] = robust chi2 before and after; iterations_run, trials_run as vo_bundle_adjust_batch reports them.
 *   Profiling stage: misc (k_pose_graph).  vo_pose_graph: one graph; a status other than VO_OK is its return value.
 * Out of scope: automatic loop detection inside the streams, more than 32 loop edges or a multi-workgroup solver for one graph, full
 * 7x7 information matrices, exact Jacobians (the left-Jacobian inverse of Sim(3)), bundle adjustment of the corrected map. */
#define VO_PGO_MAX_VERTICES 8192
#define VO_PGO_MAX_LOOPS    32
typedef struct {
    int32_t iterations;         /* 10 */
    double  huber_delta;        /* 0: off */
} vo_pgo_opts;
int vo_pose_graph_batch(vo_ctx* ctx, int B, const int32_t* vert_off /*[B + 1]*/, const int32_t* edge_off /*[B + 1]*/,
                        double* sims /*[V][13], in and out*/, const uint8_t* fixed /*[V]*/, const int32_t* edges /*[E][2], local indices*/,
                        const double* meas /*[E][13]*/, const double* info /*[E][7]*/, const vo_pgo_opts* opts,
                        double* chi2 /*[B][2]: initial, final*/, int32_t* iterations_run, int32_t* trials_run, int32_t* status);
int vo_pose_graph(vo_ctx* ctx, double* sims /*[nv][13]*/, const uint8_t* fixed, int nv, const int32_t* edges /*[ne][2]*/, const double* meas,
                  const double* info, int ne, const vo_pgo_opts* opts, double* chi2 /*[2]*/, int32_t* iterations_run, int32_t* trials_run);

/* ------------------------------------------------------------------ place recognition: device vocabulary, keyframe index, loop query
 * vo_map_localize, vo_map_align and vo_pose_graph are all told which two frames see the same ground.  This section finds them: a bag
 * of visual words, as DBoW2 and ORB-SLAM's loop detector use one.  Descriptor rows are quantised against a small vocabulary, one
 * short histogram is kept per keyframe — it outlives the frame's slot — and histograms are compared instead of descriptors.  The
 * reference has no counterpart, so the rules are this library's own; all of them are integers and no floating point is used, so a
 * checker (tests/places_reference.py) is held to equality.  Rows are the configured detector's: D = 32 bytes compared by Hamming
 * distance under an ORB batch configuration, D = 128 values 0..255 compared by the integer squared L2 distance under a SIFT one
 * (|row|^2 <= 2^20 as in vo_map_stage).  Every entry that reads slots returns VO_ERR_NOT_CONFIGURED before a batch configuration.
 *   Vocabulary: K words, each a row in the descriptor's own format; K a multiple of 256, 256 <= K <= 4096.
 *   Quantiser: a row's word is its nearest word, the lowest word index winning a tie (the selection of vo_pair_opts.match_mode 3; the
 *     device bodies are k_nn_map's and k_nn_map_orb's).
 *   Training (vo_vocab_train): the training set is the descriptor rows of the F detected slots in slot-list order, then keypoint order,
 *     n rows.  Start: word w = training row floor(w n / K), in 64-bit integers.  A round is an assignment of every row to its word
 *     followed by an update: for a word with c > 0 rows, ORB bit b (bit b % 8 of byte b / 8) is 1 iff 2 ones_b > c — a strict
 *     majority, a tie gives 0 — and SIFT component j is (2 sum_j + c) / (2 c) in integer division, the mean rounded half up; a word
 *     with c = 0 keeps its row.  The sums are int32 (atomics; their order cannot matter).  At most `iterations` rounds (below 1 counts
 *     as 1); from the second round on, a round whose assignment moved no row ends the training before its update.  *iterations_run =
 *     updates done; the vocabulary is what the last update wrote.  Every word is written through the row store of the staged map, so
 *     the matcher's operand image and norms exist for it.  Two runs on the same input give the same bytes.
 *   Entry of the index: hist[w] = min(255, rows of the frame whose word is w), uint8 [K]; sum = the sum of those saturated bytes; id =
 *     the caller's frame number, any int32.
 *   Score: shared(q, d) = sum over w of min(hist_q[w], hist_d[w]) = (sum_q + sum_d - L1(hist_q, hist_d)) / 2, an int32 (L1 on
 *     v_sad_u8, four bytes an instruction).
 *   Query: for a query entry q, every other entry d is a candidate (an entry never meets itself, whatever min_gap is) unless
 *     |id_q - id_d| < min_gap (compared in 64-bit) or shared(q, d) < min_shared.  Reported: the top_k candidates of largest shared, the
 *     lower entry index first among equals, in descending order; unused places hold entry -1, shared 0.
 * vo_vocab_train: VO_ERR_INVALID for K outside the rule, F < 1 or F > max_frames, a slot out of range, a slot flagged for its descriptor
 *   norm (SIFT), a trained word over the norm bound; VO_ERR_TOO_FEW for n < K; VO_ERR_UNSUPPORTED for n > 2^22 rows.  After an error
 *   past the argument checks there is no vocabulary.
 * vo_vocab_set: the vocabulary from the host, words [K][D]: the parity seam, and how a saved vocabulary comes back.  VO_ERR_INVALID for
 *   K outside the rule and for a SIFT word with |row|^2 > 2^20; nothing is set then, an earlier vocabulary and its index stay.
 * vo_vocab_get: up to cap words back; *K = the vocabulary's size.  vo_vocab_words: the word index of every row of a detected slot (up to
 *   cap; *n = the slot's rows): the parity seam of the quantiser.  VO_ERR_INVALID without a vocabulary.
 * A new vocabulary, trained or set, closes the index: its histograms count another vocabulary's words.
 * vo_places_open: an empty index of `capacity` entries, 1 <= capacity <= 65536 (hist [capacity][K] uint8, sum and id [capacity] int32);
 *   it replaces an open one.  VO_ERR_INVALID without a vocabulary or for a capacity outside the range.
 * vo_places_add: quantises F <= max_frames detected slots and appends their entries in order; *first_entry = the index of the first.
 *   A slot without rows gives an all-zero entry.  VO_ERR_UNSUPPORTED when the capacity would be exceeded, nothing is added then;
 *   VO_ERR_INVALID without an open index, for a slot out of range or flagged for its descriptor norm (SIFT).
 * vo_places_add_hist: appends n given histograms [n][K] with their ids; it restores a saved index and is the parity seam of the scorer.
 *   VO_ERR_UNSUPPORTED / VO_ERR_INVALID as vo_places_add.
 * vo_places_entries: entries first .. first + n - 1 back (any of the three arrays may be NULL); VO_ERR_INVALID outside the index.
 * vo_places_size: *n = entries held, *K = words of a histogram; VO_ERR_INVALID without an open index.
 * vo_places_query: Q <= 65536 query entries, each an entry of the index (a live frame is added first and then asked about: one path,
 *   no second quantiser); Q may be the whole index — the flight's all-against-all pass.  VO_ERR_INVALID without an open index, for
 *   top_k outside 1 .. 16, for a query entry outside the index.
 * Profiling stages: match_nn (the assignment: k_vocab_assign), misc (everything else).
 * Lifetime: the vocabulary and the index are allocations of their own, released by vo_destroy and by a configure call.  Detections,
 *   vo_pairs_run, the vo_slam_* calls, a live stream, the staged map and vo_map_align's buffers are left alone, and they leave these
 *   alone: the index is meant to be fed chunk after chunk while a stream walks a flight.
 * Out of scope: tf-idf weights, a vocabulary tree, inverted files, K above 4096, geometric verification inside the call (the candidates
 * go to vo_map_localize / vo_map_align), automatic use inside the restart walks. */
typedef struct {
    int32_t top_k;              /* 3; 1 .. 16 */
    int32_t min_gap;            /* 0: candidates at any distance in id */
    int32_t min_shared;         /* 0 */
} vo_places_opts;
int vo_vocab_train(vo_ctx* ctx, const int32_t* slots, int F, int K, int iterations, int32_t* iterations_run);
int vo_vocab_set(vo_ctx* ctx, const uint8_t* words /*[K][D]*/, int K);
int vo_vocab_get(vo_ctx* ctx, uint8_t* words /*[cap][D]*/, int cap, int32_t* K);
int vo_vocab_words(vo_ctx* ctx, int slot, int32_t* word /*[cap]*/, int cap, int32_t* n);
int vo_places_open(vo_ctx* ctx, int capacity);
int vo_places_add(vo_ctx* ctx, const int32_t* slots, int F, const int32_t* ids, int32_t* first_entry);
int vo_places_add_hist(vo_ctx* ctx, const uint8_t* hist /*[n][K]*/, const int32_t* ids, int n, int32_t* first_entry);
int vo_places_entries(vo_ctx* ctx, int first, int n, uint8_t* hist /*[n][K]*/, int32_t* sum, int32_t* ids);
int vo_places_size(vo_ctx* ctx, int32_t* n, int32_t* K);
int vo_places_query(vo_ctx* ctx, const int32_t* entries /*[Q]*/, int Q, const vo_places_opts* opts,
                    int32_t* out_entry /*[Q][top_k]*/, int32_t* out_shared /*[Q][top_k]*/);

/* ------------------------------------------------------------------ measurement
 * With profiling on, every kernel family of the batched path is bracketed by hipEvents on the
 * ctx stream; vo_profile_read returns accumulated milliseconds and launch counts per stage since
 * the last vo_profile_reset. */
#define VO_STAGE_COUNT 30
int vo_profile_enable(vo_ctx* ctx, int on);
int vo_profile_reset(vo_ctx* ctx);
int vo_profile_read(vo_ctx* ctx, float* ms /*VO_STAGE_COUNT*/, int32_t* launches /*VO_STAGE_COUNT*/);
const char* vo_stage_name(int stage);
/* algorithmic HBM bytes one launch of `stage` moves for F frames of the configured geometry */
double vo_stage_bytes(vo_ctx* ctx, int stage, int F);

#ifdef __cplusplus
}
#endif
#endif
