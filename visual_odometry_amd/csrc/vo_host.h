// vo_host.h — the context of libvo_hip.so and the host-side helpers its API files share (vo_api.hip, slam_api.hip).
#pragma once
#include "vo_internal.h"
#include "slam_layout.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <type_traits>
#include <algorithm>

#define MAX_EVENTS 384                        // a vo_slam_* call brackets six kernel groups per step (vo_set_slam_stats on), and the carry of a resumed one

// The device (and pinned host) allocations of one lifetime: each one its own hipMalloc, all freed together by release() or
// the destructor.  n == 0 allocates one element.
struct DevList {
    struct Entry { void* p; bool pinned; };
    std::vector<Entry> ptrs;
    DevList() = default;
    DevList(const DevList&) = delete;
    DevList& operator=(DevList&& o) noexcept { if (this != &o) { release(); ptrs.swap(o.ptrs); } return *this; }
    ~DevList() { release(); }
    template <typename T> hipError_t alloc(T** p, size_t n) { return keep(hipMalloc((void**)p, (n ? n : 1) * sizeof(T)), (void**)p, false); }
    template <typename T> hipError_t alloc_pinned(T** p, size_t n)
    {
        return keep(hipHostMalloc((void**)p, (n ? n : 1) * sizeof(T), hipHostMallocDefault), (void**)p, true);
    }
    void release()
    {
        for (const Entry& e : ptrs) (void)(e.pinned ? hipHostFree(e.p) : hipFree(e.p));
        ptrs.clear();
    }
private:
    hipError_t keep(hipError_t e, void** p, bool pinned) { if (e == hipSuccess) ptrs.push_back({*p, pinned}); return e; }
};

// A device scratch buffer that only grows (capacity in elements): grow() is defined below vo_ctx
template <typename T> struct Growable {
    T* p = nullptr;
    size_t cap = 0;
    Growable() = default;
    Growable(const Growable&) = delete;
    ~Growable() { if (p) (void)hipFree(p); }
    int grow(struct vo_ctx* ctx, size_t need, size_t n);
    int grow(struct vo_ctx* ctx, size_t need) { return grow(ctx, need, need); }
};

// One SIFT configuration: per-slot results for max_frames slots + the scale-space scratch of one sub-batch of fb frames
struct SiftState {
    DevList mem;
    bool configured = false, with_operands = false;
    vo_sift_params prm{};
    int h = 0, w = 0, fstride = 0, max_frames = 0, kp_cap = 0, cap_x = 0, raw_cap = 0, cand_cap = 0, surv_cap = 0, fb = 0;
    SiftGeom P{};
    float taps[16][SIFT_MAX_TAPS]; int ntaps[16];
    SiftExpTab E{};
    uint8_t* frames = nullptr;                                    // [slot][h][fstride] gray
    float *kp_xy = nullptr, *kp_size = nullptr, *kp_angle = nullptr, *kp_resp = nullptr; int *kp_oct = nullptr, *kp_count = nullptr, *flags = nullptr;
    uint8_t *desc = nullptr, *desc_x = nullptr; int* norms = nullptr;   // [slot][kp_cap][128] u8; int8 operand image + |v - 128|^2 for the matrix-core matcher
    float *G = nullptr, *up = nullptr;                            // sub-batch scratch: the Gaussian pyramids (the DoG planes are never stored)
    SiftCand* cand = nullptr; SiftSurv* surv = nullptr; SiftKp *kraw = nullptr, *ksorted = nullptr, *kfin = nullptr;
    int *rank = nullptr, *counts = nullptr, *fin_count = nullptr, *fin_flags = nullptr;
};

// The process's ONE RCCL communicator.  Every context of the GPU holds a reference and issues its collectives on its own
// stream, but each collective first waits (event) for the one submitted before it, whichever context that was: collectives
// run one after the other in the order the host submitted them (the same on every rank), never two at once.
// (A dedicated communicator stream was tried first: with 3 context streams it shares a hardware queue with one of them and
//  cost 9 % of the single-GPU rate — 76.4 k vs 83.7 k pairs/s — through false serialisation.)
struct CommShared {
    void* comm = nullptr;
    int rank = 0, world = 1, refs = 0;
    hipEvent_t last = nullptr;            // end of the most recently submitted collective
    bool last_set = false;
};

// What the most recent vo_pairs_run[_async] left in the pair buffers: cleared whenever those buffers may have changed
struct LastRun {
    int pairs = 0;
    std::vector<int32_t> slots;           // its pair slots (host copy)
    int points = 0;                       // ... and whether it triangulated (want_points)
    int match_mode = 0;                   // ... and its vo_pair_opts.match_mode (vo_slam_chain needs one-to-one matches)
    // host copies of the maps of the most recent vo_slam_chain: [0] at the end of the chain, [1] the snapshot
    struct Map {
        bool valid = false;
        std::vector<int32_t> cam_frame, pt_feature, obs_cam, obs_pt;
        std::vector<uint8_t> cam_fixed;
        std::vector<double> cam_pose, points, obs_xy;
    } map[2];
    // ... of the most recent vo_slam_chains: every sequence's map at its end, and the snapshot of sequence snap_seq (-1: none)
    std::vector<Map> seq_map;
    Map snap_map;
    int snap_seq = -1;
    // ... and, if it ran with vo_set_slam_stats on, its statistics rows: sequence s owns rows seq_off[s] .. seq_off[s + 1] - 1
    struct Stats {
        bool valid = false;
        int C = 0;                        // cameras a row holds: the call's max_cameras + 1
        std::vector<int32_t> seq_off, n_high, counts, obs_hist, obs_matrix, cam_frame;
        std::vector<double> total_sqerr, max_sqerr;
    } stats;
    // ... and where those maps still lie on the device, for vo_map_from_slam: the lists of a chain call live in the scratch buffer,
    // which belongs to the next call that lays it out (scratch_epoch then moves on); a stream's map has lost its older frames' rows
    struct DevMaps {
        struct Lists { const int* pt_key = nullptr; const double* pt_xyz = nullptr; };
        std::vector<Lists> seq;           // per sequence: the map at its end
        Lists snap;                       // the snapshot's lists (of sequence snap_seq, or of the one chain)
        bool stream = false;              // the call was a stream's: keys name ghost rows and frames that have left their slots
        int n_keys = 0;                   // rows the slots' descriptor array holds: max_frames * kp_cap
        uint64_t epoch = 0;               // scratch_epoch when the call laid the buffer out
    } dev;
};

// The staged map of the relocaliser (vo_map_stage / vo_map_from_slam) and the work buffers of vo_map_localize: an allocation of its
// own lifetime, released by vo_destroy and by a configure call; vo_pairs_run, the vo_slam_* calls and detections leave it alone.
// It is sized when a map is staged — for that map's rows rounded up to 256 and the configuration's max_pairs x kp_cap — and kept
// while the next map fits: rows past npt then hold what the larger map left, and k_nn_map has to bound its reads by npt alone.
struct MapState {
    DevList mem;
    bool staged = false;
    MapBuf m{};
    RelocBuf r{};
    double* dK = nullptr;
    int Q_cap = 0, kp_cap = 0;            // what the work buffers were sized for
    int last_Q = 0;                       // queries of the most recent vo_map_localize (vo_map_matches); 0: none since the map was staged
    int last_mode = 0;                    // ... and the vo_set_map_match mode it ran in (vo_map_match_seconds)
    GuidedBuf g{};                        // vo_map_localize_guided's work buffers, allocated with the others
    bool loc_ok = false;                  // r.poses / r.status hold a vo_map_localize of this map over loc_slots (the priors of a refinement pass)
    std::vector<int32_t> loc_slots;
    // vo_map_align's query maps and work buffers: a second allocation, made by the first call that needs it and kept while the next
    // one fits; it ends with the staged map (drop_map), and a newly staged map forgets its queries
    struct Align {
        DevList mem;
        AlignBuf a{};
        int Q_cap = 0, pad_cap = 0, total_cap = 0, map_rows = 0;   // what it was sized for
        int last_Q = 0;                   // queries of the most recent vo_map_align (vo_map_align_matches)
        int last_mode = 0;                // ... and the vo_set_map_match mode it ran in (1 after a vo_map_align_guided: its lists carry seconds)
        std::vector<int32_t> off, pad;    // host copies of that call's offsets
        FuseBuf f{};                      // vo_map_align_guided's work buffers, allocated with the others
        bool guided = false;              // the most recent of the two align calls was the guided one: a.sim / a.status are no priors
    } al;
};

// Place recognition (places_api.hip): the vocabulary with its training buffers, and the keyframe index.  Two allocations of their own
// lifetime, released by vo_destroy and by a configure call; nothing else touches them, and they touch nothing else.  A new
// vocabulary closes the index (its histograms count another vocabulary's words).
struct VocabState {
    DevList mem;
    bool valid = false;                   // a vocabulary has been trained or set
    VocabBuf b{};
    int K = 0, F_cap = 0, kp_cap = 0;     // what the buffers were sized for
};
struct PlacesState {
    DevList mem;
    bool open = false;
    int capacity = 0, n = 0, K = 0;
    uint8_t* hist = nullptr;              // [capacity][K]
    int *sum = nullptr, *id = nullptr;    // [capacity]
};

// vo_slam_stream: the map one call leaves on the device for the next, with every table and work buffer of the walk — one
// allocation that lives from the call that starts the stream (resume = 0) until the stream is dropped.
struct SlamStream {
    DevList mem;
    bool live = false;                    // a resume = 0 call has run and nothing has dropped the stream since
    bool lost = false;                    // its last call ended with a pair that was not localised
    bool restart = false;                 // begun by vo_slam_stream_restart: a lost stream is continued and starts a new map
    bool touched = false;                 // the anchor slot was uploaded to or detected again: the stream's last frame is gone
    int anchor = -1;                      // slot of the stream's last frame
    int done = 0, total = 0;              // pairs so far, pairs the stream may reach (what the lists were sized for)
    int carries = 0, last_ncam = 0;       // resumed calls so far; cameras the map held at the end of the last call
    int F = 0, cap = 0, max_pairs = 0;    // the configuration it was sized for
    vo_slam_opts opts{};
    double K[9] = {0};
    uint8_t* base = nullptr;              // the allocation: b.bytes long; a resumed call clears [b.call0, b.bytes), the per-pair outputs
    SlamDims dims;                        // what it was sized for (dims.stats: started with vo_set_slam_stats on, the rows and the kernel's scratch are part of it)
    SlamBufs b;                           // the whole arrays, of which a sequence's descriptor owns its ranges (slam_seq)
    // vo_slam_streams: S sequences in the one allocation.  The scalars above that describe the one sequence of vo_slam_stream*
    // (anchor, done, total, last_ncam, lost, touched) are per sequence here; `carries` counts the resumed calls — every sequence is
    // carried in each.
    struct Seq {
        int anchor = -1, done = 0, total = 0, last_ncam = 0;
        bool lost = false, touched = false;
        int n_rows = 0;                   // slots its last call's frames had, the anchor excepted: rows[s * (max_pairs + 1) ..]
        // seats (vo_slam_streams_replace / vo_slam_streams_open): a vacant seat has no flight and no anchor (anchor = -1, done = 0,
        // total = the bound of the flight that takes it); until the carry launch of the next call has reset it (clean), old_anchor
        // names the row its last flight's anchor had
        int capacity = 0;                 // total_pairs of the call that sized its lists: the most a flight in this seat may reach
        bool vacant = false, clean = false;
        int old_anchor = -1;
    };
    bool multi = false;                   // begun by vo_slam_streams
    int S = 0;
    std::vector<Seq> seq;
    std::vector<int32_t> rows;
    // vo_slam_stream with vo_set_stream_rows on when the stream began: the descriptor store, one more allocation of the stream's
    // lifetime (StreamRows, stream_rows_kernels.hip).  counters: the device's two words as the last call left them, read back with
    // the call's results — the next append starts from them.
    struct Store {
        DevList mem;
        bool on = false;
        StreamRows d{};
        int32_t counters[2] = {0, 0};     // rows stored, points dropped
    } store;
    // ... and with vo_set_stream_archive on as well: the archive of the points the camera limit removes, a third allocation of the
    // stream's lifetime (StreamArchive; k_slam_limit_stream_archive appends, stream_archive_kernels.hip selects).  counters as above.
    struct Archive {
        DevList mem;
        bool on = false;
        StreamArchive d{};
        int32_t counters[2] = {0, 0};     // entries stored, points dropped
    } archive;
};

struct vo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;         // non-blocking: no implicit ordering with the NULL stream (PyTorch / RCCL use it)
    hipStream_t stream_jpg = nullptr;     // the JPEG decoder's coefficient buffer is cleared here, beside the upload of the files and k_jpeg_unstuff
    hipEvent_t ev_jpg[2] = {nullptr, nullptr};
    char err[512] = {0};
    DevList mem;                          // context lifetime: dK, rng_tab, rng_host

    bool configured = false;
    DevList orb_mem;                      // the ORB configuration: tables, pyramid, blur, scores, ff.*, desc_x, selection state, cv2.*
    int h = 0, w = 0, max_frames = 0, max_pairs = 0;
    vo_orb_params params{};
    PyrGeom g{};
    ResizeTab tabs[VO_MAX_LEVELS]{};
    uint8_t *pyr = nullptr, *blur = nullptr, *score = nullptr;
    uint8_t* desc_x = nullptr;            // descriptors expanded to +1 / -1 bytes for the MFMA matcher
    Growable<uint8_t> staging;                                       // host frames on their way into the slots
    Growable<uint8_t> ingest_out;                                    // resized frames (frame ingest)
    SiftState sift, sift1;                                           // SIFT: the batched detector's state; the single-image call's
    Growable<uint8_t> sift_img;                                      // the single-image call's input on the device
    int detector = 0;                                                // detector of the batched path: 0 = ORB (vo_batch_configure), 1 = SIFT (vo_batch_configure_sift)
    int sift_pairs = 0;
    // JPEG decode: the batch's files, clean streams, restart lists, coefficients, component planes, B G R output, descriptors
    Growable<uint8_t> jpg_blob, jpg_clean, jpg_rst, jpg_coef, jpg_planes, jpg_out, jpg_img, jpg_tab;
    Growable<int> ingest_tab;                                        // resize tables
    int *sel_thr = nullptr, *sel_chunk_count = nullptr, *har_kept = nullptr;
    float* har_thr = nullptr;
    FrameFeat ff{};
    DevList pb_mem;                       // the pair buffers, shared by ORB and SIFT
    PairBuf pb{};
    int pb_pairs = 0, pb_cap = 0;
    double* dK = nullptr;
    LastRun last;
    SlamStream stream_map;                // vo_slam_stream's resident map (its own lifetime: see drop_slam_stream)
    MapState map;                         // the relocaliser's staged map (its own lifetime: see drop_map)
    VocabState vocab;                     // place recognition: the vocabulary and the keyframe index (their own lifetimes: see drop_places)
    PlacesState places;
    Growable<uint8_t> places_work;        // vo_places_query's query list, partial lists and results on the device
    uint64_t scratch_epoch = 0;           // counts the layouts placed in `scratch`: what an earlier call left there is gone when it has moved

    // scratch for the single-call operators
    DevList raw_mem;                      // the single-call matcher: raw_desc, raw_desc_x, raw_xy, raw_count, raw_pb.*
    int raw_cap = 0;
    uint8_t* raw_desc = nullptr; float* raw_xy = nullptr; int* raw_count = nullptr; uint8_t* raw_desc_x = nullptr;
    PairBuf raw_pb{};
    Growable<uint8_t> scratch;                       // one call's device memory, laid out by ScratchLayout
    uint32_t* rng_tab = nullptr; uint32_t* rng_host = nullptr; uint64_t rng_seed = 0; bool rng_valid = false;   // OpenCV RNG stream for the RANSAC seed

    bool prof = false;
    float prof_ms[VO_STAGE_COUNT] = {0};
    int prof_n[VO_STAGE_COUNT] = {0};
    hipEvent_t ev[MAX_EVENTS][2];
    int ev_stage[MAX_EVENTS];
    int n_ev = 0;
    bool ev_ready = false;
    hipEvent_t ev_det = nullptr;          // end of the most recent vo_frames_detect_async (vo_detect_after waits on it)
    bool ev_det_set = false;
    int descx_fp4 = -1;                   // operand image EVERY resident slot's desc_x holds: 1 FP4, 0 int8, -1 none written yet (descx_begin_write)
    int matcher_kernel = 2;               // 2: block-scaled FP4 MFMA (default), 0: int8 MFMA on +127/-127 bytes, 1: XOR + popcount
    CommShared* cs = nullptr;             // RCCL communicator of the trajectory gather: ONE per process, shared by its contexts (vo_comm_share)
    Growable<double> rec_send, rec_recv;  // the gather's packed records: this rank's and every rank's
    int kp_order = 1;                     // 1 (default): cv2's retainBest order — keypoint / match indices as cv2 numbers them; 0: canonical (octave, y, x)
    Cv2Buf cv2{};
    bool cv2_ready = false;
    int map_match = 0; double map_ratio = 0.75;   // vo_set_map_match: 0 cross-check (default), 1 ratio, 2 both; read by vo_map_localize / vo_map_align
    int pnp_refine = 1;                   // solvePnPRansac's final pose: 1 = cv2's solvePnP(ITERATIVE) (default), 0 = fast minimiser
    int dk_early = 1;                     // five-point polynomial roots: 1 = noise-floor exit (default), 0 = fixed 300 sweeps
    int slam_stats = 0;                   // 1: every vo_slam_* call also runs k_slam_stats once per step (vo_set_slam_stats); 0 (default): nothing of it
    int64_t stream_archive = 0;           // vo_set_stream_archive: entries of the archive of evicted points the next vo_slam_stream(resume = 0) starts with; 0 (default): none, -1: one per feature
    int64_t stream_rows = 0;              // vo_set_stream_rows: rows of the descriptor store the next vo_slam_stream(resume = 0) starts with; 0 (default): none, -1: one per feature
    std::vector<uint8_t> undistorted;     // per slot: vo_frames_undistort has rewritten its kp_xy (empty: no slot); cleared by whatever gives the slot new keypoints
};

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            snprintf(ctx->err, sizeof(ctx->err), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,    \
                     hipGetErrorString(e_));                                                      \
            return VO_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

#define FAIL(code, ...)                                                                           \
    do { snprintf(ctx->err, sizeof(ctx->err), __VA_ARGS__); return (code); } while (0)

// Room for `need` elements.  Without it: wait for the context's stream (queued work may still use the buffer), free, and
// allocate n >= need elements.
template <typename T> int Growable<T>::grow(vo_ctx* ctx, size_t need, size_t n)
{
    if (need <= cap) return VO_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    HIPCHK(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)));
    cap = n;
    return VO_OK;
}

inline int ScratchLayout::place(vo_ctx* ctx)
{
    int rc = ctx->scratch.grow(ctx, bytes, bytes + bytes / 4 + 64); if (rc) return rc;
    ctx->scratch_epoch++;
    place_at(ctx->scratch.p);
    return VO_OK;
}

// The end of a stream: vo_destroy (the context's destructor), a configure call, a vo_slam_stream[_restart] or vo_slam_streams that
// starts a new one and every vo_slam_chain* call come here.  (Every call that uses the allocation has waited for the context's stream before it returned.)
static inline void drop_slam_stream(vo_ctx* ctx) { ctx->stream_map = SlamStream(); }

// The end of the staged map: vo_destroy (the context's destructor) and the configure calls.  (vo_map_localize waits for the stream.)
static inline void drop_map(vo_ctx* ctx) { ctx->map = MapState(); }

// The end of the vocabulary and of the keyframe index: vo_destroy (the context's destructor) and the configure calls.  (Every
// vo_vocab_* / vo_places_* call waits for the stream before it returns.)
static inline void drop_places(vo_ctx* ctx) { ctx->places = PlacesState(); ctx->vocab = VocabState(); }

static inline void forget_slam_maps(vo_ctx* ctx)
{
    ctx->last.dev = LastRun::DevMaps();
    ctx->last.map[0] = LastRun::Map(); ctx->last.map[1] = LastRun::Map();
    ctx->last.seq_map.clear(); ctx->last.snap_map = LastRun::Map(); ctx->last.snap_seq = -1;
    ctx->last.stats = LastRun::Stats();
}

// ------------------------------------------------------------------ profiling brackets
struct StageTimer {
    vo_ctx* c; int idx;
    StageTimer(vo_ctx* ctx, int stage) : c(ctx), idx(-1)
    {
        if (c->prof && c->n_ev < MAX_EVENTS) {
            idx = c->n_ev++;
            c->ev_stage[idx] = stage;
            (void)hipEventRecord(c->ev[idx][0], c->stream);
        }
    }
    ~StageTimer() { if (idx >= 0) (void)hipEventRecord(c->ev[idx][1], c->stream); }
};

void prof_collect(vo_ctx* c);

// ---- the batched path, whichever detector is configured: ORB (vo_batch_configure) or SIFT (vo_batch_configure_sift)
struct Batch {
    bool sift, ready;
    int w, h, max_frames, max_pairs, kp_cap;
    // the slots' resident results, as the pair stage reads them
    const uint8_t *desc, *desc_x; const float* kp_xy; const int *kp_count, *flags, *norms;
    int fp4;                              // operand image in desc_x (ORB: the one written at detection; SIFT: int8 rows + L2 norms)
    // slot k's gray image at gray + k * gray_frame, rows of gray_stride bytes: level 0 of the ORB pyramid, or the SIFT slots' frames
    uint8_t* gray; int gray_stride; size_t gray_frame;
    uint8_t* gray_slot(int k) const { return gray + (size_t)k * gray_frame; }
};

Batch batch(const vo_ctx* ctx);

// cv::RNG (multiply-with-carry, core/operations.hpp RNG::next) output stream for `seed`; it depends on
// nothing but the seed, so it is tabulated once and shared by every pair of every batch.
#define RNG_TAB_N 8192
int ensure_rng(vo_ctx* ctx, uint64_t seed);

// What vo_tracks_pnp_batch and vo_slam_chain ask of the most recent vo_pairs_run: all its B pairs, triangulated, every slot
// inside the configuration, the pairs a chain of distinct frames (a0, b0), (b0, b1), ...: the order the reference walks a sequence in
int chain_check(vo_ctx* ctx, int B, const char* who, int* F_out, int* cap_out);

#define VO_MAP_MAX_POINTS 65536               // points a staged map holds (vo_map_stage, vo_map_from_slam, vo_map_from_stream)

// The one way a map is staged (reloc_api.hip): npt rows through k_map_gather — row i of `src` (device, [npt][D]) with key ==
// nullptr, else row key[i] of the slots' descriptors — and its coordinates xyz (device, [npt][3]).  vo_map_stage uploads and
// comes here; vo_map_from_slam (slam_api.hip) comes here with the map's own lists, vo_map_from_stream with the
// stream's descriptor store as src and the key list k_stream_rows_select wrote.  Synchronous.
int map_stage_device(vo_ctx* ctx, const uint8_t* src, const int* key, int n_keys, const double* xyz, int npt, const char* who);
// ... with a second part behind the first: rows n0 .. npt - 1 of the map through k_map_gather_from, src2's row key2[i] and xyz2[i]
// for map row i (vo_map_from_stream_archive: the archived points behind the live ones).  n0 == npt or src2 == nullptr: no second part.
struct MapPart2 { const uint8_t* src; const int* key; int n_keys; const double* xyz; };
int map_stage_device2(vo_ctx* ctx, const uint8_t* src, const int* key, int n_keys, const double* xyz, int n0, const MapPart2& p2, int npt, const char* who);
