// vo_internal.h — shared declarations of libvo_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vo_hip.h"

// ---- stage ids for vo_profile_* (index into ctx->prof) -------------------------------------
enum {
    ST_GRAY = 0, ST_RESIZE, ST_FAST, ST_SELECT_FAST, ST_HARRIS, ST_SELECT_HARRIS, ST_ANGLE,
    ST_BLUR, ST_BRIEF, ST_MATCH_NN, ST_MATCH_SELECT, ST_RANSAC, ST_POSE, ST_TRIANGULATE,
    ST_MISC, ST_RESERVED, ST_SIFT_SCALE, ST_SIFT_EXTREMA, ST_SIFT_ORIENT, ST_SIFT_SORT, ST_SIFT_DESC, ST_CV2_ORDER, ST_GATHER, ST_RESERVED2,
    ST_SLAM_PREPARE, ST_SLAM_BA, ST_SLAM_FILTER, ST_SLAM_LIMIT, ST_SLAM_STATS, ST_UNDISTORT
};

// ---- pyramid / work geometry, passed to kernels by value ------------------------------------
struct LevelGeom {
    int w, h, stride, off;       // level image; off = byte offset inside one frame's pyramid
    int quota;                   // ORB per-level feature budget
    float scale;                 // layerScale[l]
    int ftile_base, ftiles_x;    // FAST tiles of the pipeline (prefix over levels): they cover only what can hold a keypoint — the
    int fox, foy;                //   level minus its edgeThreshold border — and start at (fox, foy)
    int dtile_base, dtiles_x;    // FAST tiles of the dense score map (stage API): the whole level from (0, 0)
    int btile_base, btiles_x;    // blur tiles
    int cand_off, cand_cap;      // candidate slots of this level inside a frame's candidate arrays
    int sel_chunk_base;          // first selection chunk (= row of FAST tiles) of this level
};

struct PyrGeom {
    int nlevels, frame_bytes;    // frame_bytes: pyramid bytes per frame
    int edge, fast_thr, score_type, nfeatures;
    int ftiles_total, btiles_total, dtiles_total;
    int cand_total, kp_cap;
    int sel_chunks_total;
    LevelGeom lv[VO_MAX_LEVELS];
};

// the direct pyramid kernel: a wavefront = RS2_WW x RS2_WH destination pixels (lane = 4 columns, swept down the rows), a
// workgroup = four of them stacked
#define RS2_WW 256
#define RS2_WH 16
#ifndef RS2_WAVES
#define RS2_WAVES 4
#endif
#define RS2_THREADS (64 * RS2_WAVES)
#define RS2_TH (RS2_WAVES * RS2_WH)

struct ResizeTab {               // INTER_LINEAR_EXACT tables for one level (device pointers)
    const int* xofs; const uint16_t* xc1;
    const int* yofs; const uint16_t* yc1;
    int min_x, max_x, min_y, max_y;
    int direct;                  // 1: the geometry fits k_resize_direct (scale factor <= 1.27: ORB's 1.2); 0: the generic k_resize
};

#ifndef FAST_TW
#define FAST_TW 112
#endif
#ifndef FAST_TH
#define FAST_TH 20               // (24 until the tiles were restricted to the kept region in round 4: 0.634 -> 0.606 ms per 257 frames; 16: 0.644, 28: 0.724)
#endif
#define BLUR_TW 128
#ifndef BLUR_TH
#define BLUR_TH 48
#endif
#define FAST_LISTCAP ((FAST_TW / 2) * (FAST_TH / 2))

// per-frame feature arrays (device), F = number of slots
struct FrameFeat {
    uint32_t* cand_pos;   // [F][cand_total]  (y << 16 | x), level coordinates
    float*    cand_resp;  // [F][cand_total]
    int*      cand_count; // [F][VO_MAX_LEVELS]
    uint32_t* kp_pos;     // [F][kp_cap]
    int*      kp_level;   // [F][kp_cap]
    float*    kp_resp;    // [F][kp_cap]
    float*    kp_angle;   // [F][kp_cap]
    float*    kp_xy;      // [F][kp_cap][2]   level-0 coordinates (pt * layerScale)
    float*    kp_size;    // [F][kp_cap]
    uint8_t*  desc;       // [F][kp_cap][32]
    int*      kp_count;   // [F]
    int*      flags;      // [F]  bit0: capacity overflow
    uint32_t* hist;       // [F][VO_MAX_LEVELS][256] FAST score histogram
    uint32_t* tile_list;  // [F][ftiles_total][FAST_LISTCAP] NMS winners inside the border, per FAST tile
    int*      tile_count; // [F][ftiles_total]
};

// cv2 keypoint order (vo_set_keypoint_order(ctx, 1)): per frame and level the raster-ordered list of ALL NMS winners
// inside the border (cv2 runs retainBest on that list) and the work arrays of the re-enacted std::nth_element /
// std::partition (cv2order_kernels.hip)
struct Cv2Buf {
    uint32_t* all_pos;    // [F][all_total]  (y << 16 | x)
    float*    all_resp;   // [F][all_total]  FAST score
    uint32_t* all_cand;   // [F][all_total]  kept winners only: index into the level's candidate list; the rest is never written
    int*      all_count;  // [F][VO_MAX_LEVELS]
    int*      chunk_count;// [F][sel_chunks_total + 1] listed winners per row of FAST tiles
    uint2*    work;       // [F][all_total]  (response bits, index into the all-list)
    uint32_t* lpos;       // [F][all_total]  positions where the left / right cursor of a partition pass stops
    uint32_t* rpos;
    int all_off[VO_MAX_LEVELS], all_cap[VO_MAX_LEVELS], all_total;
};

// recoverPose between its launches: k_pose_prepare writes it, k_pose adds the candidates' counts, k_pose_finish reads it
struct PoseState {
    int active;           // 0: the pair failed or is ambiguous (k_pose_prepare has written its result)
    int ninl;
    int good[4];          // points in front of both cameras: (R1, t), (R2, t), (R1, -t), (R2, -t)
    double R1[9], R2[9], t[3];
};

// per-pair arrays (device), P = number of pairs
struct PairBuf {
    int*      slots;      // [P][2]
    int*      nn_idx;     // [P][2 dirs][kp_cap]      dir 0: frame1->frame2, dir 1: frame2->frame1
    int*      nn_dist;    // [P][2][kp_cap]
    int*      nn_idx2;    // [P][kp_cap] second neighbour (knn2)
    int*      nn_dist2;   // [P][kp_cap]
    int*      nn_colkey;  // [P][row blocks][kp_cap] reverse-direction keys of the single-pass FP4 matcher (nullptr: kp_cap too large)
    int*      m_q;        // [P][kp_cap]
    int*      m_t;        // [P][kp_cap]
    float*    m_d;        // [P][kp_cap]
    int*      m_count;    // [P]
    double*   px1;        // [P][kp_cap][2] pixel coords of matches (float64)
    double*   px2;
    double*   xn1;        // [P][kp_cap][2] normalised coords
    double*   xn2;
    uint8_t*  mask;       // [P][kp_cap] E-RANSAC inlier mask
    double*   models;     // [P][64][90] workspace: five-point models of one RANSAC round
    PoseState* pose_state; // [P]
    double*   in1;        // [P][kp_cap][2] normalised inliers
    double*   in2;
    double*   ipx1;       // [P][kp_cap][2] pixel inliers
    double*   ipx2;
    vo_pair_result* res;  // [P]
    double*   X;          // [P][4][kp_cap]
    uint8_t*  pose_mask;  // [P][kp_cap] recoverPose mask (0/255); only allocated for the single-call path
};

struct RansacParams {
    double prob, thresh_px;
    int max_iters;
    uint64_t seed;
    double K[9];
    double dist_thresh;
    int dk_early;                // five-point root finder: 1 = stop at the noise floor, 0 = OpenCV's fixed 300 sweeps
};

// ---- trajectory gather over RCCL (gather_rccl.hip); the const char* results are error texts, nullptr = success
const char* rccl_load(void);
const char* rccl_unique_id(uint8_t* id128);
const char* rccl_comm_init(void** comm, const uint8_t* id128, int rank, int world);
void rccl_comm_destroy(void* comm);
const char* rccl_comm_count(void* comm, int* n);
const char* rccl_all_gather_f64(void* comm, const double* send, double* recv, size_t count, hipStream_t s);
void launch_pack_records(hipStream_t s, const vo_pair_result* res, int B, int valid, double* rec);

// ---- launchers (defined in the .hip files) --------------------------------------------------
void launch_gray(hipStream_t s, const uint8_t* src, int channels, int row_stride, int64_t frame_stride,
                 uint8_t* pyr, const PyrGeom& g, int F);
void launch_gray_plain(hipStream_t s, const uint8_t* src, int channels, int row_stride, int64_t frame_stride,
                       uint8_t* dst, int w, int h, int dstride, int64_t dframe, int F);
void launch_resize(hipStream_t s, uint8_t* pyr, const PyrGeom& g, int level, const ResizeTab& tab, int F);
void launch_fast(hipStream_t s, const uint8_t* pyr, uint8_t* score, uint32_t* hist, const PyrGeom& g, int F,
                 uint32_t* tile_list, int* tile_count);      // tile_list == nullptr: dense score map instead of winner lists
// cb != nullptr (cv2 keypoint order): the same two launches also write the raster-ordered list of every NMS winner inside the
// border (the list cv2's first retainBest sees) into cb->all_*
void launch_select_fast(hipStream_t s, const PyrGeom& g, FrameFeat ff, int F, int* thr, int* chunk_count,
                        const uint32_t* tile_list, const int* tile_count, const Cv2Buf* cb);
void launch_harris(hipStream_t s, const uint8_t* pyr, const PyrGeom& g, FrameFeat ff, int F);
void launch_cv2_order(hipStream_t s, const PyrGeom& g, FrameFeat ff, Cv2Buf cb, int F, const int* kept);
void launch_retain_raw(hipStream_t s, const float* resp, int n, int n_points, uint2* a, uint32_t* lpos, uint32_t* rpos,
                       int* order, int* n_out);
void launch_select_harris(hipStream_t s, const PyrGeom& g, FrameFeat ff, int F, float* thr, int* kept);
void launch_resize_linear(hipStream_t st, const uint8_t* src, int sw, int sh, int cn, int sstride, int64_t sframe,
                          uint8_t* dst, int dw, int dh, int dstride, int64_t dframe,
                          const int* xofs, const void* xa, const int* yofs, const void* yb, int area2, int F);
void launch_resize_area(hipStream_t st, const uint8_t* src, int cn, int sstride, uint8_t* dst, int dw, int dh, int dstride,
                        int isx, int isy, const int* xsi, const float* xal, const int* xst, const int* ysi, const float* yal, const int* yst);
// ---- SIFT (sift_batch.hip): the reference's live detector, cv2.SIFT_create(), frame-batched
#define SIFT_IMG_BORDER 5
#define SIFT_MAX_INTERP_STEPS 5
#define SIFT_MAX_OCT 16
#define SIFT_MAX_TAPS 64
// One frame's Gaussian pyramid (floats): octave o holds its nLayers + 3 Gaussian planes of w[o] x h[o] with a row pitch of
// stride[o] floats (a multiple of 16: every row starts on a 64-byte boundary).  The DoG planes are not stored: a DoG sample is
// one subtraction of two stored Gaussian samples, made by the kernels that read it (k_sb_extrema, k_sb_refine).
struct SiftGeom {
    int nOct, nLayers;
    int w[SIFT_MAX_OCT], h[SIFT_MAX_OCT], stride[SIFT_MAX_OCT];
    size_t plane[SIFT_MAX_OCT];                         // stride * h
    size_t goff[SIFT_MAX_OCT];                          // float offset of the octave's first plane inside a frame's block
    size_t gframe;                                      // floats per frame
};
struct SiftCand { int o, layer, r, c; };
struct SiftKp { float x, y, size, angle, response; int octave; };
struct SiftSurv { SiftKp kp; int o, layer, r, c; };      // a refined extremum awaiting its orientation(s)
struct SiftExpTab { float tab[64]; };                   // 2^(i/64), the table of cv::hal::exp32f
// per-frame counters of a sub-batch: counts[f][4] = {extrema candidates, refined extrema, oriented keypoints, final keypoints}
int launch_sb_sweep_base(hipStream_t s, const uint8_t* img, int channels, int row_stride, int64_t frame_stride, int sw, int sh,
                         float* dstG, size_t g_fs, int stride, int F, const float* taps, int ntaps);
int launch_sb_sweep(hipStream_t s, const float* src, size_t src_fs, float* dstG, size_t g_fs, int w, int h, int stride, int F,
                    const float* taps, int ntaps, float* dstH = nullptr, size_t h_fs = 0, int hstride = 0, int hw = 0, int hh = 0);
void launch_sb_extrema(hipStream_t s, const SiftGeom& P, const float* gauss, int o, float threshold, SiftCand* cand, int* counts, int cap, int F);
void launch_sb_refine_orient(hipStream_t s, const SiftGeom& P, const float* gauss, const SiftCand* cand, int cand_cap, float contrastThr,
                             float edgeThr, float sigma, const SiftExpTab& E, SiftSurv* surv, int surv_cap, SiftKp* kps, int kp_cap, int* counts, int F, int waves);
void launch_sb_sort_emit(hipStream_t s, const SiftKp* kps, int kp_cap, int* counts, int* rank /*[F][4097]*/, void* rank_tmp /*[F][kp_cap] records*/, SiftKp* sorted,
                         SiftKp* out, int out_cap, int* out_count, int* out_flags, int cand_cap, int surv_cap, int F);
void launch_sb_descriptor(hipStream_t s, const SiftGeom& P, const float* gauss, const SiftKp* kps, int kp_cap, const int* counts, const SiftExpTab& E,
                          uint8_t* desc, uint8_t* desc_x, int cap_x, int* norms, int* flags, int first_slot, int F, int waves);
// n chosen descriptor rows (device, [n][128] values 0..255) into a slot exactly as launch_sb_descriptor leaves detected ones
void launch_sb_pack_rows(hipStream_t s, const uint8_t* rows, int n, int slot, int kp_cap, uint8_t* desc, uint8_t* desc_x, int cap_x, int* norms, int* flags);
void launch_sb_unpack(hipStream_t s, const SiftKp* kps, int kp_cap, const int* counts, int first_slot, float* kp_xy, float* kp_size, float* kp_angle,
                      float* kp_resp, int* kp_oct, int* kp_count, const int* fin_count, const int* fin_flags, int* flags, int F);
// L2 nearest neighbours of integer-valued (0..255) 128-element descriptors on the matrix cores (match_kernels.hip)
void launch_match_nn_l2i8(hipStream_t s, const uint8_t* desc_x, const int* norms, const int* kp_count, int kp_cap, int cap_x, PairBuf pb, int P,
                          int dirs_mask, int knn2);

// ---- JPEG decode (jpeg_kernels.hip, jpeg_host.cpp): cv2.imread in front of the path
#include "jpeg_host.h"
void launch_jpeg_decode(hipStream_t s, const uint8_t* blob, JpegImage* imgs, const JpegTables* tabs, int F, uint8_t* clean, uint32_t* rst,
                        int16_t* coef, uint8_t* planes, uint8_t* out, int max_blocks, int max_w, int max_h, bool gray = false,
                        bool packed_tables = false /* no file of the batch names more than four Huffman tables */,
                        hipEvent_t coef_cleared = nullptr /* the coefficient buffer is cleared on another stream: k_jpeg_huffman waits for this */);

// problem b is rows offsets[b * off_stride] .. offsets[b * off_stride + 1] - 1: off_stride 1 = problems packed back to back,
// 2 = a {first, end} pair per problem (vo_slam_chains: every sequence's rows sit in its own range)
void launch_pnp_ransac(hipStream_t s, const double* obj, const double* img, const int* offsets, int B, const double* Kd,
                       int iterations, double reproj_err, double confidence, uint64_t seed, const uint32_t* rng_tab, int rng_n,
                       int refine_cv2, double* rvec, double* tvec, uint8_t* mask, int* ninl, int* status, int off_stride = 1);
void launch_rodrigues(hipStream_t s, const double* in, int in_is_matrix, double* out);
void launch_blur(hipStream_t s, const uint8_t* pyr, uint8_t* blur, const PyrGeom& g, int F);
// orientation (kp_angle) and descriptor of every keypoint: reads the raw pyramid and its blurred copy
void launch_brief(hipStream_t s, const uint8_t* pyr, const uint8_t* blur, const PyrGeom& g, FrameFeat ff, int F, uint8_t* desc_x, int cap_x, int fp4);

// Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8, each with its own L2).  Neighbouring
// work items share data (image tiles: halo rows and 128-byte lines; the row blocks of a pair: the other frame's
// descriptors), so indices are remapped to give every XCD one
// contiguous run of tiles (bijective for any n; placement is a speed matter only, never correctness).
__device__ __forceinline__ int xcd_tile(int b, int n)
{
    const int q = n >> 3, r = n & 7, x = b & 7, k = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

// expanded descriptors: [frame][cap_x / 16][16 chunks][16 rows][16 B] of +1 / -1 bytes, cap_x = desc_x_rows(kp_cap)
static inline int desc_x_rows(int kp_cap) { return (kp_cap + 255) & ~255; }
void launch_desc_expand(hipStream_t s, const uint8_t* desc, const int* kp_count, int kp_cap, int cap_x, uint8_t* desc_x, int F, int fp4);
// returns 1 when the reverse direction was left as per-row-block column keys in pb.nn_colkey (launch_match_select's col_parts)
int launch_match_nn(hipStream_t s, const uint8_t* desc_x, const int* kp_count, int kp_cap, int cap_x, PairBuf pb, int P,
                    int dirs_mask, int knn2, int fp4);
size_t nn_colkey_ints(int P, int kp_cap);   // size of PairBuf::nn_colkey; 0 above the single pass's LDS capacity
void launch_match_nn_popcount(hipStream_t s, const uint8_t* desc, const int* kp_count, int kp_cap, PairBuf pb, int P,
                              int dirs_mask, int knn2);
void launch_match_select(hipStream_t s, const float* kp_xy, const int* kp_count, int kp_cap, PairBuf pb, int P,
                         int mode, double ratio, const double* K, int l2 = 0,   // l2: nn_dist holds squared L2 distances, reported as sqrtf
                         int col_parts = 0);                                     // col_parts: reverse direction from pb.nn_colkey

size_t nn_l2_knn2_keys(int na, int nb);
void launch_nn_l2_knn2(hipStream_t s, const float* A, int na, const float* B, int nb, int dim, int* idx, float* dist, unsigned long long* part);
void launch_nn_l2(hipStream_t s, const float* A, int na, const float* B, int nb, int dim, int* idx, float* dist, unsigned long long* key);

void launch_ransac(hipStream_t s, PairBuf pb, int kp_cap, int P, RansacParams rp, const uint32_t* rng_tab, int rng_n);
void launch_pose(hipStream_t s, PairBuf pb, int kp_cap, int P, RansacParams rp);
void launch_triangulate_pairs(hipStream_t s, PairBuf pb, int kp_cap, int P, RansacParams rp);
void launch_triangulate_raw(hipStream_t s, const double* P1, const double* P2, const double* x1, const double* x2,
                            int M, double* X);
void launch_five_point_raw(hipStream_t s, const double* x1, const double* x2, double* E, int* nm, int dk_early);
// cv2.computeCorrespondEpilines: F is already transposed for whichImage 2; point_type 0 f64 (f64 lines), 1 f32, 2 i32 (f32 lines)
void launch_epilines(hipStream_t s, const void* pts, int point_type, int N, const double* F, void* lines);
// cv2.undistortPoints (undistort_kernels.hip): the camera, the eight rational-model coefficients (absent ones zero) and RR = P R,
// passed to the kernels by value
struct UndistortParams {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
    double RR[9];
};
// point_type 0: f64 points in and out, 1: f32 in and out (the f64 result rounded once)
void launch_undistort_points(hipStream_t s, const void* pts, int point_type, int N, UndistortParams up, void* out);
// the keypoints of F slots in place: kp_xy [F][kp_cap][2], kp_count [F] (both already offset to the first slot)
void launch_undistort_frames(hipStream_t s, float* kp_xy, const int* kp_count, int kp_cap, int F, UndistortParams up);
// per resident pair: dist [P][kp_cap] (zeros past the pair's inliers), n / mean / sd / mx [P]
void launch_pairs_epipolar(hipStream_t s, PairBuf pb, int kp_cap, int P, const double* Kd, double* dist, int* n, double* mean, double* sd, double* mx);
void launch_reprojection(hipStream_t s, const double* poses, int ncam, const double* points, int npt, const int* obs_cam,
                         const int* obs_pt, const double* obs_xy, int nobs, const double* Kd, double threshold,
                         double* sqerr, uint8_t* keep, int* bad);
// ---- the localisation chain on resident pair results (geom_kernels.hip / pnp_kernels.hip): src/visual_slam.py:183-266
// vo_slam_chains_restart, vo_slam_stream_restart: what a sequence needs to start a new map after a lost frame (initialize_map's
// self.map.clean(), src/visual_slam.py:43-45).  st == nullptr everywhere else: the chain stops at the first lost frame.
enum { SEG_INIT = 0,    // 1: this step is an initial step of the sequence — its pair starts a segment as pair 0 starts a chain
       SEG_FIRST = 1,   // the pair that started the current segment (vo_slam_stream_restart: of this call; -1 if an earlier call's)
       SEG_COUNT = 2,    // segments started so far
       SEG_CAUSE = 3 }; // the status that ended tracking and has not been reported yet (0: none)
struct RestartBuf {
    int*    st;                   // [4] the SEG_* words
    int*    segment; int* cause;  // [P] per-pair outputs
    double* seg_poses;            // [P][12] at a pair that starts a segment: its first camera as it entered the map
    double* seg_poses_last;       // [P][12] ... as the map last held it
};
struct ChainBuf {
    unsigned long long* parent;   // [F][cap] packed feature_mapper entry (k_track_link's format), 0 = no entry
    uint8_t* in_map;              // [F][cap] 1: a map point is keyed by this feature id (mappointdict)
    double*  map_pt;              // [F][cap][3] world coordinates
    double*  cam;                 // [F][12] world -> camera [R | t] of a slot's camera (TrackedCamera.pose()[0:3])
    int*     cam_ok;              // [F]
    double*  obj;                 // [cap][3] the current problem's map coordinates
    double*  img;                 // [cap][2] ... image coordinates
    int*     off;                 // [2] {obj0, obj0 + n}: the offsets k_pnp_ransac reads
    int      obj0;                // first row of this chain's problem in the arrays k_pnp_ransac is handed (0 unless several chains share them)
    double*  rvec; double* tvec;  // [3] each: solvePnPRansac's result for the current pair
    uint8_t* pmask;               // [cap]
    int*     pninl; int* pstatus; // [1] each
    double*  P1; double* P2;      // [12] each: K pose(frame1)[0:3], K pose(frame2)[0:3] of the current pair
    double*  Xw;                  // [cap][4] the current pair's inliers triangulated in world coordinates
    int*     alive;               // [1] 1 while every pair so far was localised
    int*     n_corr; int* n_inl; int* status; int* n_map;   // [P] per-pair outputs
    double*  poses;               // [P + 1][12]: camera of pair 0's first frame, then of every pair's second frame
    int*     map_count;           // [1]
    RestartBuf rs;                // set with SlamDims::restart (slam_layout.h), all nullptr without it
};
void launch_chain_link(hipStream_t s, PairBuf pb, int kp_cap, int P, ChainBuf cb);
void launch_chain_init(hipStream_t s, PairBuf pb, int kp_cap, ChainBuf cb);
void launch_chain_gather(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, ChainBuf cb);
void launch_chain_pose(hipStream_t s, PairBuf pb, int p, const double* Kd, ChainBuf cb);
void launch_chain_triangulate(hipStream_t s, PairBuf pb, int kp_cap, int p, ChainBuf cb);
void launch_chain_insert(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, ChainBuf cb, uint8_t* dec);   // dec: [cap] scratch
// ---- bundle adjustment (ba_kernels.hip): Map.optimize_map, src/map.py:104-186.  One workgroup per problem.
struct BaProblem {
    int cam0, pt0, obs0, pair0, blk0;   // where the problem's cameras / points / observations / pair list / block offsets start
    int ncam, npt, nobs, nfree;
    int skip;                           // 1: rejected on the host (status says why), its data stay as they are
};
struct BaBuf {
    const BaProblem* prob;              // [B]
    double*       poses;                // [cameras][12] world -> camera [R | t], in / out
    const int*    cam_col;              // [cameras] column block of a free camera in S, -1 for a fixed one
    double*       X; double* X2;        // [points][3]: in / out, and the trial estimate
    const int*    pt_first;             // per problem npt + 1: first observation of a point (observations sorted by point)
    const int*    obs_cam; const int* obs_pt; const double* obs_xy;   // sorted observations, indices local to the problem
    double*       W;                    // [observations][18]: w Jp^T Jx of a free camera's observation
    double*       Hpp; double* bp; double* Hpi;   // [points][6], [3], [6]: H_pp, b_p, (H_pp + lambda I)^-1 (symmetric: 00 01 02 11 12 22)
    const int2*   pairs;                // per block (c1 <= c2) of free cameras: the (observation of c1, observation of c2) that share a point
    const int*    blk_first;            // per problem nfree (nfree + 1) / 2 + 1 offsets into its pairs
    double*       chi2;                 // [B][2] robust chi2 before, after
    int*          iterations_run; int* trials_run;   // [B]
};
struct BaParams { double focal, cx, cy, delta; int iterations; };
void launch_bundle_adjust(hipStream_t s, const BaBuf& D, const BaParams& P, int B, int max_free);
// ---- the resident map of vo_slam_chain (slam_kernels.hip): src/map.py's three lists, dense, in the reference's append order
struct SlamMap {
    int*     cnt;                       // [4] cameras, points, observations, unused
    int*     cam_frame;                 // [cameras] index of the camera's frame in the chain (0 = pair 0's first frame, p + 1 = pair p's second)
    double*  cam_pose;                  // [cameras][12] world -> camera [R | t]
    uint8_t* cam_fixed;                 // [cameras]
    int*     pt_key;                    // [points] owning feature id: slot * kp_cap + keypoint (TrackedPoint.feature_id)
    double*  pt_xyz;                    // [points][3]
    int*     obs_cam; int* obs_pt;      // [observations] indices into the two lists above
    double*  obs_xy;                    // [observations][2]
    int*     pt_feat;                   // set with SlamDims::stream (nullptr without it): [points][2] the owning feature id as (frame along the stream, keypoint)
};
// A stream (SlamDims::stream): what a call that continues a map needs beside the lists.  All zero / nullptr without the switch.
struct StreamBuf {
    int      frame0;                    // index along the stream of the call's first frame (0: the call that starts the stream)
    int      n_carried;                 // cameras the map held at the carry beside the anchor: they have no slot in this call
    int*     carried_frame;             // [n_carried] their frames along the stream, in map order at the carry
    double*  carried_poses;             // [n_carried][12] ... as the map last held them
};
struct SlamBuf {
    SlamMap  m;
    int      cam_cap, pt_cap, obs_cap, pair_cap;   // entries the map's three lists and `pairs` can hold
    int*     pt_of;                     // [F][cap] 1 + index of the map point keyed by this feature id, 0 = none (mappointdict)
    int*     dec;                       // [cap] add_information_to_map's decision per match, taken against the pre-loop snapshot
    int*     tmp;                       // [points] per-point counts / cursors / new indices
    int*     idx;                       // [observations] input index of every observation sorted by point
    int*     n_pts; int* n_obs; int* n_cam;   // [P] the map's sizes after every pair
    double*  poses_last;                // [P + 1][12] every camera as the map last held it
    // what k_slam_ba_prepare hands k_bundle_adjust (BaBuf's const members)
    BaProblem* prob; int* cam_col; int* pt_first; int* s_cam; int* s_pt; double* s_xy; int2* pairs; int* blk_first;
    BaProblem base;                     // where this map's lists start in the arrays BaBuf names: cam0 .. blk0 (all 0 for a single chain)
    StreamBuf st;                       // set with SlamDims::stream
};
void launch_slam_add(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras, ChainBuf cb, SlamBuf sb);
void launch_slam_ba_prepare(hipStream_t s, ChainBuf cb, SlamBuf sb);
void launch_slam_filter(hipStream_t s, PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb);
void launch_slam_limit(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb);
// ---- the same step on a map carried from an earlier call (vo_slam_stream): the kernels whose code differs, and the carry.
// The slot-keyed tables have max_frames + 2 rows there: rows F and F + 1 are the ghost rows (slam_kernels.hip, k_slam_carry).
void launch_slam_add_stream(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras, ChainBuf cb, SlamBuf sb);
void launch_slam_filter_stream(hipStream_t s, PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb);
void launch_slam_limit_stream(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb);
struct SlamCarry {
    int kp_cap, F;                      // rows 0 .. F - 1 are frame slots
    int anchor;                         // slot of the stream's last frame: pair 0 of the new call starts there
    int ghost_new, ghost_old;           // F and F + 1, alternating between carries
    const double* keep;                 // [2][12] the anchor camera as it entered the map / as the map last held it (the previous call's last rows)
};
void launch_slam_carry(hipStream_t s, SlamCarry c, ChainBuf cb, SlamBuf sb);
// ---- a stream's descriptor store (stream_rows_kernels.hip; vo_set_stream_rows, vo_map_from_stream): an allocation beside the
// walk's layout, which no kernel of the walk reads or writes.
struct StreamRows {
    int      D;                         // bytes of a descriptor row: 32 (ORB) or 128 (SIFT)
    int      capacity;                  // rows the store holds
    int      kp_cap, frames;            // row_of is [frames][kp_cap]: frames = total_pairs + 1
    uint8_t* rows;                      // [capacity][D] raw rows as the slots' descriptor array holds them; a row whose point is gone stays (a hole)
    int*     row_of;                    // [frames][kp_cap] the store row of feature (frame along the stream, keypoint), -1: none
    int*     counters;                  // [2] rows stored, points dropped because the store was full
    int      sel_cap;                   // entries sel_key / sel_xyz hold: the bound of a staged map, or the list's capacity if that is less
    int*     sel_key;                   // [sel_cap] k_stream_rows_select: the store rows of the selected points, in map order
    double*  sel_xyz;                   // [sel_cap][3] ... and their coordinates
    int*     sel_cnt;                   // [2] points selected (may pass sel_cap: nothing is written past it), points of the window without a row
};
// pt_bound: points the map's list can hold (the grid is sized from it; the kernels read the count from m.cnt)
void launch_stream_rows_append(hipStream_t s, SlamMap m, StreamRows st, size_t pt_bound, const uint8_t* desc, int n_keys, int frame0, int stored0,
                               int dropped0);
void launch_stream_rows_select(hipStream_t s, SlamMap m, StreamRows st, size_t pt_bound, int first, int end);
// ---- a stream's archive of evicted points (vo_set_stream_archive, vo_map_from_stream_archive; docs/kernels/k_stream_archive.md):
// one more allocation beside the store's.  Every point the camera limit removes is appended by k_slam_limit_stream_archive
// (slam_kernels.hip), in removal order, with a copy of its descriptor row; stream_archive_kernels.hip selects over the entries.
#define SA_TILE 256                     // entries of a tile of the selection's count and emit passes
struct StreamArchive {
    int      D;                         // bytes of a descriptor row: 32 (ORB) or 128 (SIFT)
    int      capacity;                  // entries the archive holds
    int*     feature;                   // [capacity][2] the owning feature (frame along the stream, keypoint): pt_feat
    double*  xyz;                       // [capacity][3] the coordinates the limit read
    int*     evicted_at;                // [capacity] the pair along the stream whose limit removed the point
    int*     has_row;                   // [capacity] 1: rows holds the entry's descriptor row; 0: there was none to copy
    uint8_t* rows;                      // [capacity][D] the archive's own copies: an entry is complete however the flight was chunked
    int*     counters;                  // [2] entries stored, points dropped because the archive was full
    int*     tile_cnt;                  // [ceil(capacity / SA_TILE)][2] the count pass: per tile, entries selected with a row / without
    int      sel_cap;                   // entries sel_key / sel_xyz hold: the bound of a staged map
    int*     sel_key;                   // [sel_cap] indexed by staged position: the archive entry of an archived point
    double*  sel_xyz;                   // [sel_cap][3] ... and its coordinates
    int*     sel_cnt;                   // [2] entries selected with a row (may pass what fits: nothing is written past sel_cap), without
};
// What the limit of a stream with an archive needs beside its own arguments: where the rows come from.  An argument of its own;
// SlamBuf is as it was.
struct SlamArchive {
    StreamArchive a;
    const uint8_t* desc; int n_keys;    // the slots' descriptor rows [n_keys][D]: the row of a point born in this call, by pt_key
    const uint8_t* store_rows; int store_cap;   // the descriptor store's rows [store_cap][D] ...
    const int* feat_row;                // ... and its table [frames][kp_cap] of the store row of a feature, -1: none
    int      kp_cap, frames;
};
void launch_slam_limit_stream_archive(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb, SlamArchive ar);
// the entries [0, stored) owned by frames [first, end): counts per tile, then the entries that have a row to a.sel_key / a.sel_xyz in
// archive order, the first at staged position *live (device; nullptr: 0); a.sel_cnt <- {with a row, without}
void launch_stream_archive_select(hipStream_t s, StreamArchive a, int stored, int first, int end, const int* live);
// ---- ... on a stream that starts a new map after a lost frame (vo_slam_stream_restart): cb.rs is set, its state words and the
// alive flag outlive the call.  k_slam_restart_stream goes between k_chain_pose and k_chain_triangulate of every step.
void launch_slam_restart_stream(hipStream_t s, PairBuf pb, int kp_cap, int p, ChainBuf cb, SlamBuf sb);
void launch_slam_add_stream_restart(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras, ChainBuf cb, SlamBuf sb);
void launch_slam_filter_stream_restart(hipStream_t s, PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb);
void launch_slam_limit_stream_restart(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb);
void launch_slam_carry_restart(hipStream_t s, SlamCarry c, ChainBuf cb, SlamBuf sb);
// ---- the same step for S independent sequences at once (vo_slam_chains): one workgroup per sequence and kernel, the sequence on a
// grid axis.  A workgroup reads its sequence's descriptor from a device array — its pairs inside the run, and a ChainBuf / SlamBuf
// whose slot-keyed tables (parent, in_map, map_pt, cam, cam_ok, pt_of) are the shared ones (the sequences' slots are disjoint) and
// whose other members are the sequence's own — and does step j of its chain on pair first + j; with j >= count it returns at once.
struct SlamSeq { int first, count; ChainBuf cb; SlamBuf sb; };
void launch_chain_init_seqs(hipStream_t s, PairBuf pb, int kp_cap, const SlamSeq* seqs, int S);
void launch_chain_gather_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, int F, const SlamSeq* seqs, int S);
void launch_chain_pose_seqs(hipStream_t s, PairBuf pb, int j, const double* Kd, const SlamSeq* seqs, int S);
void launch_chain_triangulate_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const SlamSeq* seqs, int S);
void launch_slam_add_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, int F, double max_norm, int free_cameras, const SlamSeq* seqs, int S);
void launch_slam_ba_prepare_seqs(hipStream_t s, int j, const SlamSeq* seqs, int S);
void launch_slam_filter_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const double* Kd, double threshold, const SlamSeq* seqs, int S);
void launch_slam_limit_seqs(hipStream_t s, int j, int max_cameras, const SlamSeq* seqs, int S);
void launch_slam_restart_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const SlamSeq* seqs, int S);
// ---- ... on S maps carried from call to call (vo_slam_streams): the stream / restart kernels with the sequence on the grid axis.
// The slot-keyed tables have max_frames + 2 S rows: sequence s owns the ghost rows F + 2 s and F + 2 s + 1.  A descriptor's sb.st is
// the sequence's own (frame0 counts along its stream); a sequence that is idle in a call has count = 0.
struct SlamSeqCarry {
    SlamCarry c;                        // the sequence's anchor slot, its ghost rows, its anchor camera; c.F = max_frames
    int hops;                           // rows of the slot-keyed tables (F + 2 S): the bound of a track walk
    const int* rows; int n_rows;        // the rows only this sequence holds and does not keep: the slots of its last call's frames, its old ghost row
};
void launch_slam_carry_restart_seqs(hipStream_t s, const SlamSeq* seqs, const SlamSeqCarry* car, int S);
// ... with seats (vo_slam_streams_replace / vo_slam_streams_open): what the carry launch does for a sequence, in an array of its own
// beside SlamSeqCarry.  A seat that is reset gives up car.rows (the slots of its last call's frames) and rows[] here.
enum { SEAT_CARRY = 0,      // its flight goes on: the carry
       SEAT_RESET = 1,      // replaced since the last call: cleared to what a stream's first call starts from
       SEAT_VACANT = 2 };   // vacant and already reset: nothing
struct SlamSeat {
    int mode;
    int n_rows; int rows[3];            // SEAT_RESET: the old anchor row (if it had one) and both ghost rows
    double* keep;                       // [24] the seat's kept anchor camera
};
void launch_slam_carry_restart_seats(hipStream_t s, const SlamSeq* seqs, const SlamSeqCarry* car, const SlamSeat* seats, int S);
void launch_slam_restart_stream_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const SlamSeq* seqs, int S);
void launch_slam_add_stream_restart_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, int F, double max_norm, int free_cameras, const SlamSeq* seqs, int S);
void launch_slam_filter_stream_restart_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const double* Kd, double threshold, const SlamSeq* seqs, int S);
void launch_slam_limit_stream_restart_seqs(hipStream_t s, int j, int max_cameras, const SlamSeq* seqs, int S);
// ---- show_map_statistics (src/map.py:234-297) of a resident map (slam_kernels.hip, k_slam_stats): one row of statistics per pair.
// Passed to the two statistics kernels only; no other kernel sees it, and SlamBuf / SlamMap / ChainBuf / SlamSeq are as they were.
struct StatsBuf {
    double*  total_sqerr; double* max_sqerr;   // [rows] calculate_reprojection_error's sum in observation order; the largest term
    int*     n_high;                    // [rows] observations with sqerr > high
    int*     counts;                    // [rows][3] the three list lengths: cameras, points, observations
    int*     obs_hist;                  // [rows][VO_STATS_HIST] points by number of observations, the last bin open-ended
    int*     obs_matrix;                // [rows][C][C] points a pair of cameras sees together, upper triangle
    int*     cam_frame;                 // [rows][C] the map's camera list, -1 past its end (nullptr: not wanted)
    int      C;                         // cameras a row has room for (<= VO_BA_MAX_CAMERAS)
    int*     pt_cur;                    // the kernel's own scratch: per point a count, then a cursor, then the end of its slots; a map
    int*     slot;                      //   uses the range that starts at its pt0 / obs0.  slot: per observation, grouped by point, its camera
    int*     bad;                       // [1] set when an observation names a missing camera or point (it is skipped)
    const double* Kd;
    double   high;                      // show_map_statistics' threshold of a "high reprojection error" (src/map.py:72: 10)
};
void launch_slam_stats(hipStream_t s, int p, SlamBuf sb, StatsBuf out);
void launch_slam_stats_seqs(hipStream_t s, int j, const SlamSeq* seqs, int S, StatsBuf out);
// ---- relocalisation of resident frames against a staged map by descriptors (reloc_kernels.hip): vo_map_stage / _from_slam / _localize
struct MapBuf {
    int      D;                         // bytes of a descriptor row: 32 under an ORB configuration, 128 under a SIFT one
    int      cap_rows;                  // rows the arrays have room for (a multiple of 256); rows past npt keep what a larger map left
    int      npt;
    uint8_t* rows;                      // [cap_rows][D] the rows as staged: what vo_map_rows returns, and the operand of the popcount kernel
    uint8_t* img;                       // SIFT: the int8 operand image k_nn_l2i8 reads, one "slot" of cap_rows rows (sift_rows.h)
    int*     norms;                     // SIFT: [cap_rows] |v - 128|^2
    double*  xyz;                       // [cap_rows][3]
    int*     flag;                      // [1] bit 1: a SIFT row broke the norm bound
};
struct RelocBuf {
    int*     slots;                     // [Q] the queries' frame slots
    int*     nn_idx; int* nn_dist;      // [Q][kp_cap] nearest map row of every keypoint and its distance (SIFT: integer d^2; ORB: Hamming)
    int*     nn_dist2;                  // [Q][kp_cap] the second-smallest distance (knnMatch(k=2)'s n.distance): written in map-match modes 1, 2
    int*     rn_idx;                    // [Q][cap_rows] nearest keypoint of query q for every map row (not written in mode 1)
    float*   m_d2;                      // [Q][kp_cap] n.distance of every entry of the match list, in list order (modes 1, 2)
    int*     m_q; int* m_t; float* m_d; // [Q][kp_cap] the match list: keypoint, map point, cv2's float32 distance
    int*     m_count;                   // [Q]
    double*  obj; double* img;          // [Q][kp_cap][3], [Q][kp_cap][2]: query q's problem starts at row q kp_cap
    int*     off;                       // [Q][2] {first, end}: k_pnp_ransac's offsets with off_stride 2
    double*  rvec; double* tvec;        // [Q][3]
    uint8_t* mask;                      // [Q][kp_cap]
    int*     ninl; int* status;         // [Q]
    double*  poses;                     // [Q][12]
};
// rows of a map from the slots' descriptors (src [slot][kp_cap][D], key = slot kp_cap + keypoint, n_keys = rows src holds) or, with
// key == nullptr, from src [npt][D] as it stands: both through the one store
void launch_map_gather(hipStream_t s, MapBuf m, const uint8_t* src, const int* key, int n_keys, const double* xyz);
// ... rows id0 .. m.npt - 1 of the map only, key and xyz indexed by the map row (a part staged behind another: vo_map_from_stream_archive)
void launch_map_gather_from(hipStream_t s, MapBuf m, int id0, const uint8_t* src, const int* key, int n_keys, const double* xyz);
void launch_nn_map(hipStream_t s, MapBuf m, RelocBuf r, int Q, const uint8_t* desc, const uint8_t* desc_x, const int* norms, const int* kp_count,
                   int kp_cap, int cap_x, int mode);
// mode, ratio: vo_set_map_match (0 cross-check, 1 ratio, 2 both)
void launch_map_select(hipStream_t s, MapBuf m, RelocBuf r, int Q, const float* kp_xy, const int* kp_count, int kp_cap, double max_distance,
                       int mode, double ratio);
// [Rodrigues(rvec) | tvec] of B solved problems, zeros for the others; a model with fewer than min_inliers inliers becomes VO_ERR_NO_MODEL
void launch_pnp_poses(hipStream_t s, const double* rvec, const double* tvec, const int* ninl, int* status, int B, int min_inliers, double* poses);
// ---- guided relocalisation: the staged map's points matched by projection under a prior pose (guided_kernels.hip): vo_map_localize_guided
#define GUIDED_G 64                     // the keypoint grid is GUIDED_G x GUIDED_G square cells over the keypoints' own box
#define GUIDED_CELLS (GUIDED_G * GUIDED_G)
#define GUIDED_TILE 256                 // points per workgroup of k_guided_match, one lane each
struct GuidedBuf {
    int*     cell_off;                  // [Q][GUIDED_CELLS + 1] where a cell's keypoints start in cell_kp (row-major cells: cy GUIDED_G + cx)
    int*     cell_kp;                   // [Q][kp_cap] the query's keypoints in cell order
    double*  box;                       // [Q][4] x0, y0, 1 / cell edge, cell edge
    unsigned long long* claim;          // [Q][kp_cap] (d << 32) | point of the point that keeps the keypoint; all ones: nobody
    int*     pt_d2;                     // [Q][cap_rows] a claiming point's second distance (INT_MAX: fewer than two candidates)
    double*  prior;                     // [Q][12]
    int*     skip;                      // [Q] not VO_OK: the query is not matched and keeps this status (the refinement pass)
    int*     n_seen;                    // [Q]
};
// k_guided_grid + k_guided_match, then k_guided_select: RelocBuf's match list, correspondences and offsets as launch_map_select leaves them
void launch_guided_match(hipStream_t s, MapBuf m, RelocBuf r, GuidedBuf g, int Q, const uint8_t* desc, const float* kp_xy, const int* kp_count,
                         int kp_cap, const double* Kd, double radius, double max_distance, double ratio);
void launch_guided_select(hipStream_t s, MapBuf m, RelocBuf r, GuidedBuf g, int Q, const float* kp_xy, const int* kp_count, int kp_cap);
// after launch_pnp_poses: a skipped query takes its earlier status back, with no inliers and a zero pose
void launch_guided_keep(hipStream_t s, RelocBuf r, GuidedBuf g, int Q);
// ---- map alignment: Q query maps against the staged one (reloc_kernels.hip): vo_map_align, vo_sim3_ransac_batch
struct AlignBuf {
    int      Q, D, total;               // query maps, bytes of a row, rows of all of them
    int*     off;                       // [Q + 1] query q's rows and points in the caller's arrays: off[q] .. off[q + 1] - 1
    int*     pad;                       // [Q + 1] where its operand starts in the padded arrays: every map on a multiple of 256 rows
    uint8_t* rows;                      // [pad[Q]][D] the rows as MapBuf::rows holds a map's
    uint8_t* img; int* norms;           // SIFT: the int8 operand image and |v - 128|^2, a "slot" per query map
    double*  xyz;                       // [total][3] the queries' points as uploaded
    int*     flag;                      // [1] bit 1: a SIFT row broke the norm bound
    int*     nn_idx; int* nn_dist;      // [pad[Q]] nearest staged row of every query row and its distance
    int*     nn_dist2;                  // [pad[Q]] the second-smallest distance (map-match modes 1, 2)
    int*     rn_idx;                    // [Q][cap_rows of the staged map] nearest row of query q for every staged row (not written in mode 1)
    float*   m_d2;                      // [total] n.distance of every entry of the match lists, in list order (modes 1, 2)
    int*     m_b; int* m_a; float* m_d; // [total] the match lists, query q's at off[q]: query row, staged row, cv2's float32 distance
    int*     m_count;                   // [Q]
    double*  src; double* dst;          // [total][3] the correspondences: b = the query's point, a = the staged map's
    int*     poff;                      // [Q][2] {first, end}: k_sim3_ransac's offsets with off_stride 2
    double*  sim;                       // [Q][13] s, R row-major, t
    uint8_t* mask;                      // [total]
    int*     ninl; int* status;         // [Q]
};
// the queries' rows (device, [total][D]) into their operands, then both directions' nearest neighbours; max_rows = the largest query map
void launch_map_align_match(hipStream_t s, MapBuf m, AlignBuf a, const uint8_t* src_rows, int max_rows, int mode);
void launch_map_align_select(hipStream_t s, MapBuf m, AlignBuf a, double max_distance, int mode, double ratio);
// B problems src -> dst ([n][3] each); problem b is rows offsets[b off_stride] .. offsets[b off_stride + 1] - 1; sim [B][13]
void launch_sim3_ransac(hipStream_t s, const double* src, const double* dst, const int* offsets, int off_stride, int B, int iterations, double max_error,
                        double confidence, uint64_t seed, const uint32_t* rng_tab, int rng_n, int min_inliers, double* sim, uint8_t* mask, int* ninl,
                        int* status);
// the gather of launch_map_align_match alone: the queries' rows (device, [total][D]) into their operands
void launch_map_align_gather(hipStream_t s, AlignBuf a, const uint8_t* src_rows);
// ---- guided map alignment: the query maps' points matched in space under a prior similarity (map_fuse_kernels.hip): vo_map_align_guided
#define FUSE_G 16                       // the grid over the staged map is FUSE_G^3 cells over its points' own box, an edge per axis
#define FUSE_CELLS (FUSE_G * FUSE_G * FUSE_G)
#define FUSE_TILE 256                   // query points per workgroup of k_fuse_match, one lane each
struct FuseBuf {
    int*     cell_off;                  // [FUSE_CELLS + 1] where a cell's points start in cell_pt (cells (cz FUSE_G + cy) FUSE_G + cx)
    int*     cell_pt;                   // [cap_rows of the staged map] the staged points in cell order
    double*  box;                       // [3][2] per axis: lowest finite coordinate, 1 / cell edge (0: the axis is one cell)
    unsigned long long* claim;          // [Q][cap_rows] (d << 32) | query row of the row that keeps the staged point; all ones: nobody
    unsigned long long* pt_best;        // [total] (d << 32) | staged point of a query row that passed the filters; all ones: none
    int*     pt_d2;                     // [total] ... its second distance (INT_MAX: fewer than two candidates)
    double*  prior;                     // [Q][13]
    int*     skip;                      // [Q] not VO_OK: the query is not matched and keeps this status (the refinement pass)
    int*     n_seen;                    // [Q]
};
// k_fuse_grid + k_fuse_match, then k_fuse_select: AlignBuf's match lists, correspondences and offsets as launch_map_align_select leaves
// them (m_d2 always written); max_rows = the largest query map
void launch_fuse_match(hipStream_t s, MapBuf m, AlignBuf a, FuseBuf f, int max_rows, double radius, double max_distance, double ratio);
void launch_fuse_select(hipStream_t s, MapBuf m, AlignBuf a, FuseBuf f);
// after launch_sim3_ransac: a skipped query takes its earlier status back, with no inliers and a zero similarity
void launch_fuse_keep(hipStream_t s, AlignBuf a, FuseBuf f);

// ---- place recognition (reloc_kernels.hip): vo_vocab_*, vo_places_*
// The vocabulary is a map of K rows without points (v.xyz == nullptr, v.npt == v.cap_rows == K): the matcher's operand image and
// norms exist for it because every word goes through map_store_row_sift / _orb.
struct VocabBuf {
    MapBuf   v;
    uint8_t* tmp;                       // [K][D] the new words on their way into the store
    int*     acc;                       // [K][256] ones per bit (ORB) / [K][128] sums per component (SIFT)
    int*     cnt;                       // [K] rows assigned
    int*     slots;                     // [F] the frame slots of a call
    int*     word;                      // [F][kp_cap] the word of every row of slot slots[q]
    int*     prev;                      // [F][kp_cap] ... in the assignment before
    int*     changed;                   // [1] rows whose word differs from prev
    int*     key;                       // [K] the start words: slot * kp_cap + keypoint
    int*     ids;                       // [F] the caller's frame numbers on their way into the index
};
// rows of the vocabulary: row key[w] of src ([..][D]), or row w with key == nullptr
void launch_vocab_store(hipStream_t s, VocabBuf vb, const uint8_t* src, const int* key);
// the nearest word of every row of F slots (lowest index on a tie) -> vb.word
void launch_vocab_assign(hipStream_t s, VocabBuf vb, int F, const uint8_t* desc, const uint8_t* desc_x, const int* norms, const int* kp_count,
                         int kp_cap, int cap_x);
// vb.acc / vb.cnt / vb.changed (cleared by the caller) from vb.word; vb.prev <- vb.word
void launch_vocab_accumulate(hipStream_t s, VocabBuf vb, int F, const uint8_t* desc, const int* kp_count, int kp_cap);
void launch_vocab_update(hipStream_t s, VocabBuf vb);
// entries first .. first + F - 1 of the index from vb.word and vb.ids
void launch_places_hist(hipStream_t s, VocabBuf vb, int F, const int* kp_count, int kp_cap, uint8_t* hist, int* sum, int* id);
void launch_places_sums(hipStream_t s, const uint8_t* hist, int K, int n, int* sum);
#define VO_PLACES_MAX_SPLITS 64
struct PlacesQuery {
    const uint8_t* hist; const int* sum; const int* id;   // the index: [n][K], [n], [n]
    int      n, K;
    const int* qent; int Q;             // the query entries
    int      top_k, min_gap, min_shared;
    int      splits, per_split;         // the entries are dealt over `splits` workgroups per query block, per_split (a multiple of 64) each
    unsigned long long* part;           // [Q][splits][16] the best keys of every split, descending, 0 = none
    int*     out_entry; int* out_shared;   // [Q][top_k]
};
void launch_places_query(hipStream_t s, PlacesQuery p);

void launch_tracks(hipStream_t s, const int* pair_frames, const int* match_off, const int* mq, const int* mt, int P, int max_m,
                   int F, int cap, unsigned long long* parent, int* root_frame, int* root_idx, int* hops, int* bad);
