// vo_api.hip — context, device buffers and the C ABI of libvo_hip.so (see include/vo_hip.h).
// Host-side plumbing only: every arithmetic stage is a HIP kernel in orb_/match_/geom_kernels.hip.
#include "vo_internal.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <type_traits>
#include <algorithm>

#define MAX_EVENTS 384                        // vo_slam_chain brackets five kernel groups per pair, six with vo_set_slam_stats on

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
    uint8_t* base = nullptr; size_t bytes = 0;
    uint8_t* call_mem = nullptr; size_t call_bytes = 0;     // the per-pair outputs: cleared at the start of every call
    ChainBuf cb{}; SlamBuf sb{}; BaBuf D{}; SlamMap snap{};
    double *dK = nullptr, *dchi2 = nullptr, *keep = nullptr; int *dit = nullptr, *dtr = nullptr;
    uint8_t *map_mem = nullptr, *snap_mem = nullptr; size_t map_bytes = 0;
    // vo_slam_streams: S sequences in the one allocation.  The scalars above that describe the one sequence of vo_slam_stream*
    // (anchor, done, total, last_ncam, lost, touched) are per sequence here; `carries` counts the resumed calls — every sequence is
    // carried in each — and cb / sb / D / snap name the whole arrays, of which a sequence's descriptor owns its ranges.
    struct Seq {
        int anchor = -1, done = 0, total = 0, last_ncam = 0;
        bool lost = false, touched = false;
        int n_rows = 0;                   // slots its last call's frames had, the anchor excepted: rows[s * (max_pairs + 1) ..]
        SlamSeq at{};                     // its descriptor before a call's offsets: the ranges of the lists that are its own
        size_t np = 0, no = 0;            // points and observations its lists hold
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
    SlamSeq* dseq = nullptr; SlamSeqCarry* dcar = nullptr; int* drows = nullptr;
    SlamSeat* dseat = nullptr;            // what the carry launch does for every seat, when one of them is vacant
    size_t snap_np = 0, snap_no = 0;
    bool stats = false;                   // started with vo_set_slam_stats on: the rows and the kernel's scratch are part of the allocation
    StatsBuf sbuf{};
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
    int pnp_refine = 1;                   // solvePnPRansac's final pose: 1 = cv2's solvePnP(ITERATIVE) (default), 0 = fast minimiser
    int dk_early = 1;                     // five-point polynomial roots: 1 = noise-floor exit (default), 0 = fixed 300 sweeps
    int slam_stats = 0;                   // 1: every vo_slam_* call also runs k_slam_stats once per step (vo_set_slam_stats); 0 (default): nothing of it
};

static const char* k_stage_names[VO_STAGE_COUNT] = {
    "gray", "pyramid_resize", "fast_score_nms", "select_fast", "harris", "select_harris", "ic_angle",
    "gaussian_blur", "rbrief", "match_nn", "match_select", "essential_ransac", "recover_pose",
    "triangulate", "misc", "reserved", "sift_scale_space", "sift_extrema", "sift_refine_orient", "sift_sort_unique",
    "sift_descriptor", "cv2_keypoint_order", "trajectory_gather", "reserved2", "slam_ba_prepare", "slam_bundle_adjust", "slam_filter",
    "slam_camera_limit", "slam_map_statistics"};

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

static void clear_last_run(vo_ctx* ctx) { ctx->last = LastRun(); }

// The end of a stream: vo_destroy (the context's destructor), a configure call, a vo_slam_stream[_restart] or vo_slam_streams that
// starts a new one and every vo_slam_chain* call come here.  (Every call that uses the allocation has waited for the context's stream before it returned.)
static void drop_slam_stream(vo_ctx* ctx) { ctx->stream_map = SlamStream(); }

// An upload, ingest or detection into slots first .. first + n - 1: if the stream's last frame is among them, no call can continue it
// (vo_slam_streams: the sequence whose last frame it is cannot advance any more; the others can).
static void slam_stream_slots_written(vo_ctx* ctx, int first, int n)
{
    SlamStream& st = ctx->stream_map;
    if (st.live && st.anchor >= first && st.anchor < first + n) st.touched = true;
    for (SlamStream::Seq& q : st.seq)
        if (st.live && q.anchor >= first && q.anchor < first + n) q.touched = true;
}

// The device memory of one call: typed sub-buffers of ctx->scratch, each on a 256-byte boundary.  take() names a pointer
// and its element count; place() grows the buffer to what was taken and sets the pointers, so size and offsets agree.
struct ScratchLayout {
    size_t bytes = 0;                     // all sub-buffers: they start at ctx->scratch.p
    template <typename T> void take(T** p, size_t n)
    {
        slots.push_back({p, bytes, [](void* dst, uint8_t* at) { *static_cast<T**>(dst) = reinterpret_cast<T*>(at); }});
        bytes += (n * sizeof(T) + 255) & ~(size_t)255;
    }
    void place_at(uint8_t* base) { for (const Slot& s : slots) s.set(s.dst, base + s.off); }   // (an allocation of the caller's, `bytes` long)
    int place(vo_ctx* ctx)
    {
        int rc = ctx->scratch.grow(ctx, bytes, bytes + bytes / 4 + 64); if (rc) return rc;
        for (const Slot& s : slots) s.set(s.dst, ctx->scratch.p + s.off);
        return VO_OK;
    }
    struct Slot { void* dst; size_t off; void (*set)(void*, uint8_t*); };
    std::vector<Slot> slots;
};

// vo_set_slam_stats: the statistics rows of P pairs with room for cm cameras, and k_slam_stats' scratch for np points and no
// observations, as sub-buffers of a call's layout.  Off: nothing is taken, the layout is byte for byte what it was.
static void slam_stats_take_scratch(ScratchLayout& sc, StatsBuf& d, bool on, size_t np, size_t no)
{
    if (!on) return;
    sc.take(&d.pt_cur, np); sc.take(&d.slot, no); sc.take(&d.bad, 1);
}

static void slam_stats_take_rows(ScratchLayout& sc, StatsBuf& d, bool on, size_t P, size_t cm)
{
    if (!on) return;
    sc.take(&d.total_sqerr, P); sc.take(&d.max_sqerr, P); sc.take(&d.n_high, P); sc.take(&d.counts, P * 3); sc.take(&d.obs_hist, P * VO_STATS_HIST);
    sc.take(&d.obs_matrix, P * cm * cm); sc.take(&d.cam_frame, P * cm);
    d.C = (int)cm; d.high = 10.0;
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

static void prof_collect(vo_ctx* c)
{
    for (int i = 0; i < c->n_ev; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[i][0], c->ev[i][1]) == hipSuccess) {
            c->prof_ms[c->ev_stage[i]] += ms;
            c->prof_n[c->ev_stage[i]] += 1;
        }
    }
    c->n_ev = 0;
}

// ------------------------------------------------------------------ geometry (host)
static inline int cv_round_f(float v) { return (int)lrintf(v); }
static inline int cv_floor_d(double v) { int i = (int)v; return i - (i > v); }
static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

static int check_params(vo_ctx* ctx, const vo_orb_params* p)
{
    if (!p) FAIL(VO_ERR_INVALID, "params is NULL");
    if (p->first_level != 0 || p->wta_k != 2 || p->patch_size != 31)
        FAIL(VO_ERR_INVALID, "only firstLevel=0, WTA_K=2, patchSize=31 are supported");
    if (p->nlevels < 1 || p->nlevels > VO_MAX_LEVELS) FAIL(VO_ERR_INVALID, "nlevels out of range");
    if (p->edge_threshold < 19 || p->edge_threshold > 255) FAIL(VO_ERR_INVALID, "edgeThreshold must be in [19, 255]");
    if (p->fast_threshold < 1 || p->fast_threshold > 254) FAIL(VO_ERR_INVALID, "fastThreshold must be in [1, 254]");
    if (p->score_type != 0 && p->score_type != 1) FAIL(VO_ERR_INVALID, "scoreType must be 0 (HARRIS) or 1 (FAST)");
    if (p->nfeatures < 0 || p->nfeatures > 50000) FAIL(VO_ERR_INVALID, "nfeatures out of range (0..50000)");
    if (!(p->scale_factor > 1.0f)) FAIL(VO_ERR_INVALID, "scaleFactor must be > 1");
    return VO_OK;
}

// orb.cpp: layerScale, level sizes and per-level quotas
static int make_geometry(vo_ctx* ctx, int h, int w, const vo_orb_params* p, PyrGeom* g)
{
    memset(g, 0, sizeof(*g));
    const int L = p->nlevels;
    g->nlevels = L; g->edge = p->edge_threshold; g->fast_thr = p->fast_threshold;
    g->score_type = p->score_type; g->nfeatures = p->nfeatures;
    const double sf = (double)p->scale_factor;
    const float factor = (float)(1.0 / sf);
    float nd = p->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0, off = 0, ft = 0, bt = 0, co = 0, sc = 0, dt = 0;
    for (int l = 0; l < L; l++) {
        LevelGeom& lv = g->lv[l];
        lv.scale = (float)pow(sf, (double)l);
        lv.w = cv_round_f((float)w / lv.scale);
        lv.h = cv_round_f((float)h / lv.scale);
        if (lv.w < 1 || lv.h < 1) FAIL(VO_ERR_INVALID, "pyramid level %d is empty (%dx%d input)", l, w, h);
        if (lv.w > 65535 || lv.h > 65535) FAIL(VO_ERR_INVALID, "image too large");
        lv.stride = align_up(lv.w, 64);
        lv.off = off;
        off += lv.stride * lv.h;
        if (l < L - 1) { lv.quota = cv_round_f(nd); sum += lv.quota; nd *= factor; }
        else lv.quota = p->nfeatures - sum > 0 ? p->nfeatures - sum : 0;
        // FAST in the pipeline only matters where a keypoint can lie: runByImageBorder drops everything within edgeThreshold of the
        // level's edge, and a pixel there takes part in the 3 x 3 suppression of a kept one only if it is the border's innermost
        // ring.  The tiles therefore cover columns edge .. w - edge - 1 and rows edge .. h - edge - 1 (their one-pixel ring supplies
        // the neighbours): 13 % fewer tiles at 1280 x 720 / 8 levels, and no candidates from the border band in the tiles that remain.
        // (fox is a multiple of 16: the staging loads stay 16-byte aligned — with fox = 28 the tiles were 18 % fewer and k_fast slower,
        // 0.73 ms against 0.64: profiles/r04_k_fast_border_restriction.txt.)
        lv.fox = (p->edge_threshold - 1) & ~15; lv.foy = p->edge_threshold;
        const int iw = lv.w - p->edge_threshold - lv.fox, ih = lv.h - p->edge_threshold - lv.foy;
        const int trows = iw > 0 && ih > 0 ? (ih + FAST_TH - 1) / FAST_TH : 0;
        lv.ftile_base = ft; lv.ftiles_x = trows > 0 ? (iw + FAST_TW - 1) / FAST_TW : 0;
        ft += lv.ftiles_x * trows;
        lv.dtile_base = dt; lv.dtiles_x = (lv.w + FAST_TW - 1) / FAST_TW;
        dt += lv.dtiles_x * ((lv.h + FAST_TH - 1) / FAST_TH);
        lv.btile_base = bt; lv.btiles_x = (lv.w + BLUR_TW - 1) / BLUR_TW;
        bt += lv.btiles_x * ((lv.h + BLUR_TH - 1) / BLUR_TH);
        const int want = p->score_type == 0 ? 2 * lv.quota : lv.quota;
        lv.sel_chunk_base = sc;
        sc += trows;
        lv.cand_off = co;
        lv.cand_cap = align_up(want + (want > 1024 ? want : 1024), 8);
        co += lv.cand_cap;
    }
    g->frame_bytes = align_up(off, 256);
    g->ftiles_total = ft; g->btiles_total = bt; g->dtiles_total = dt;
    g->cand_total = co;
    g->sel_chunks_total = sc;
    g->kp_cap = align_up(p->nfeatures + (p->nfeatures / 8 > 256 ? p->nfeatures / 8 : 256), 8);
    return VO_OK;
}

// resize.cpp interpolationLinear<ufixedpoint16>::getCoeffs
static void build_lin_tab(int ssize, int dsize, int* ofs, uint16_t* c1, int* pmin, int* pmax)
{
    const double inv_scale = (double)dsize / (double)ssize;
    const double scale = 1.0 / inv_scale;
    int minofst = 0, maxofst = dsize;
    for (int val = 0; val < dsize; val++) {
        volatile double fval = scale * ((double)val + 0.5);
        fval = fval - 0.5;
        const double fv = fval;
        const int ival = cv_floor_d(fv);
        ofs[val] = 0; c1[val] = 0;
        if (ival >= 0 && ssize > 1) {
            if (ival < ssize - 1) {
                ofs[val] = ival;
                volatile double fr = fv - (double)ival;
                fr = fr * 256.0;
                c1[val] = (uint16_t)lrint((double)fr);
            } else {
                ofs[val] = ssize - 1;
                if (val < maxofst) maxofst = val;
            }
        } else if (val + 1 > minofst) minofst = val + 1;
    }
    *pmin = minofst; *pmax = maxofst;
}

// ------------------------------------------------------------------ buffers
static hipError_t alloc_pairbuf(DevList& mem, PairBuf& pb, int P, int cap, bool with_pose_mask)
{
    hipError_t e;
    const size_t pc = (size_t)P * cap;
    pb = PairBuf{};
#define A_(field, n) if ((e = mem.alloc(&pb.field, (n))) != hipSuccess) return e
    A_(slots, (size_t)P * 2); A_(nn_idx, pc * 2); A_(nn_dist, pc * 2); A_(nn_idx2, pc); A_(nn_dist2, pc);
    A_(m_q, pc); A_(m_t, pc); A_(m_d, pc); A_(m_count, (size_t)P);
    A_(px1, pc * 2); A_(px2, pc * 2); A_(xn1, pc * 2); A_(xn2, pc * 2);
    A_(mask, pc); A_(models, (size_t)P * 64 * 90); A_(pose_state, (size_t)P);
    A_(in1, pc * 2); A_(in2, pc * 2); A_(ipx1, pc * 2); A_(ipx2, pc * 2);
    A_(res, (size_t)P); A_(X, pc * 4);
    if (with_pose_mask) { A_(pose_mask, pc); }
    if (const size_t n = nn_colkey_ints(P, cap)) { A_(nn_colkey, n); }
#undef A_
    return hipSuccess;
}

// all-winner lists + work arrays of the cv2 order mode for the current configuration.  Capacity per level: an eighth
// of its pixels (natural images leave 1 - 4 % of the pixels as FAST corners; 3x3 NMS allows at most a quarter).
static int alloc_cv2(vo_ctx* ctx)
{
    if (ctx->cv2_ready) return VO_OK;
    const PyrGeom& g = ctx->g;
    Cv2Buf& cb = ctx->cv2;
    int off = 0;
    for (int l = 0; l < g.nlevels; l++) {
        const int px8 = g.lv[l].w * g.lv[l].h / 8 + 1024;
        cb.all_off[l] = off;
        cb.all_cap[l] = align_up(px8 > g.lv[l].cand_cap ? px8 : g.lv[l].cand_cap, 8);
        off += cb.all_cap[l];
    }
    cb.all_total = off;
    const size_t F = (size_t)ctx->max_frames, n = F * off;
    DevList& m = ctx->orb_mem;
    HIPCHK(m.alloc(&cb.all_pos, n)); HIPCHK(m.alloc(&cb.all_resp, n)); HIPCHK(m.alloc(&cb.work, n));
    HIPCHK(m.alloc(&cb.all_cand, n)); HIPCHK(m.alloc(&cb.lpos, n)); HIPCHK(m.alloc(&cb.rpos, n));
    HIPCHK(m.alloc(&cb.all_count, F * VO_MAX_LEVELS));
    HIPCHK(m.alloc(&cb.chunk_count, F * (size_t)(g.sel_chunks_total + 1)));
    HIPCHK(hipMemset(cb.all_count, 0, F * VO_MAX_LEVELS * sizeof(int)));
    HIPCHK(hipDeviceSynchronize());
    ctx->cv2_ready = true;
    return VO_OK;
}

// the ORB configuration and the pair buffers, with the last run that described them
static void free_config(vo_ctx* c)
{
    c->configured = c->cv2_ready = false;
    c->descx_fp4 = -1;
    c->orb_mem.release();
    c->pb_mem.release();
    c->pb_pairs = c->pb_cap = 0;
    clear_last_run(c);
    drop_slam_stream(c);
}

static void comm_release(vo_ctx* ctx);
static int sift_frames_upload_enqueue(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot);
static int sift_frames_detect_enqueue(vo_ctx* ctx, int first_slot, int F);

extern "C" int vo_version(void) { return 120; }

extern "C" int vo_create(int device_id, vo_ctx** out)
{
    if (!out) return VO_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return VO_ERR_HIP;
    vo_ctx* ctx = new vo_ctx();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        ctx->mem.alloc(&ctx->dK, 16) != hipSuccess) {
        delete ctx;
        return VO_ERR_HIP;
    }
    for (int i = 0; i < MAX_EVENTS; i++) { (void)hipEventCreate(&ctx->ev[i][0]); (void)hipEventCreate(&ctx->ev[i][1]); }
    ctx->ev_ready = true;
    (void)hipEventCreateWithFlags(&ctx->ev_det, hipEventDisableTiming);
    *out = ctx;
    return VO_OK;
}

extern "C" void vo_destroy(vo_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream_jpg) { (void)hipStreamSynchronize(ctx->stream_jpg); (void)hipStreamDestroy(ctx->stream_jpg); }
    for (int i = 0; i < 2; i++) if (ctx->ev_jpg[i]) (void)hipEventDestroy(ctx->ev_jpg[i]);
    if (ctx->ev_ready) for (int i = 0; i < MAX_EVENTS; i++) { (void)hipEventDestroy(ctx->ev[i][0]); (void)hipEventDestroy(ctx->ev[i][1]); }
    if (ctx->ev_det) (void)hipEventDestroy(ctx->ev_det);
    comm_release(ctx);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;                           // the buffers go with their owners
}

// The Hamming nearest-neighbour kernel for sets of `cap` rows and, on the matrix cores, the image of the descriptors (desc_x)
// it reads: detection writes that image, the single-call matcher expands it.  The matrix-core kernels carry the column index
// inside their accumulator: fewer than 127^2 = 16129 rows per set.
enum { NN_POPCOUNT, NN_INT8, NN_FP4 };
static int nn_kernel(const vo_ctx* ctx, int cap)
{
    if (ctx->matcher_kernel == 1 || cap >= 16129) return NN_POPCOUNT;          // XOR + popcount on the packed descriptors
    return ctx->matcher_kernel == 2 && cap < 8192 ? NN_FP4 : NN_INT8;          // block-scaled FP4 MFMA: fewer than 8192 rows
}

// The Hamming nearest neighbours of P pairs into pb (dirs_mask, knn2 as launch_match_nn takes them) on nn_kernel's kernel.  The
// matrix cores read desc_x as image `fp4`: the one that was written, whatever the setter says now.  Returns col_parts.
static int launch_hamming_nn(const vo_ctx* ctx, const PairBuf& pb, const uint8_t* desc, const uint8_t* desc_x, int fp4,
                             const int* kp_count, int cap, int P, int dirs, int knn2)
{
    if (nn_kernel(ctx, cap) == NN_POPCOUNT) { launch_match_nn_popcount(ctx->stream, desc, kp_count, cap, pb, P, dirs, knn2); return 0; }
    return launch_match_nn(ctx->stream, desc_x, kp_count, cap, desc_x_rows(cap), pb, P, dirs, knn2, fp4);
}

// Slots first .. first + n - 1 of the ORB configuration are about to get the operand image nn_kernel selects now; returns it (1:
// FP4).  ONE flag names the image of every resident slot, so when a writer of some slots changes it — the setter was called
// between two detections — the slots outside its range are expanded again from ff.desc in the new format (a slot never written
// has count 0: no rows).  A run whose format does not change, and the first writer after a configure, launch nothing.
static int descx_begin_write(vo_ctx* ctx, int first, int n)
{
    const PyrGeom& g = ctx->g;
    const int fp4 = nn_kernel(ctx, g.kp_cap) == NN_FP4, cx = desc_x_rows(g.kp_cap), F = ctx->max_frames;
    if (ctx->descx_fp4 >= 0 && ctx->descx_fp4 != fp4) {
        const FrameFeat& ff = ctx->ff;
        launch_desc_expand(ctx->stream, ff.desc, ff.kp_count, g.kp_cap, cx, ctx->desc_x, first, fp4);
        const int a = first + n;
        launch_desc_expand(ctx->stream, ff.desc + (size_t)a * g.kp_cap * 32, ff.kp_count + a, g.kp_cap, cx, ctx->desc_x + (size_t)a * cx * 256, F - a, fp4);
    }
    ctx->descx_fp4 = fp4;
    return fp4;
}

extern "C" int vo_set_matcher_kernel(vo_ctx* ctx, int kind)
{
    if (!ctx) return VO_ERR_INVALID;
    if (kind < 0 || kind > 2) FAIL(VO_ERR_INVALID, "matcher kernel must be 0 (int8 MFMA), 1 (XOR + popcount) or 2 (block-scaled FP4 MFMA)");
    ctx->matcher_kernel = kind;
    return VO_OK;
}

extern "C" int vo_set_keypoint_order(vo_ctx* ctx, int kind)
{
    if (!ctx) return VO_ERR_INVALID;
    if (kind != 0 && kind != 1) FAIL(VO_ERR_INVALID, "keypoint order must be 0 (canonical) or 1 (cv2)");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->kp_order = kind;
    if (kind == 1 && ctx->configured && !ctx->cv2_ready) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return alloc_cv2(ctx);
    }
    return VO_OK;
}

extern "C" int vo_set_poly_solver(vo_ctx* ctx, int kind)
{
    if (!ctx) return VO_ERR_INVALID;
    if (kind != 0 && kind != 1) FAIL(VO_ERR_INVALID, "poly solver must be 0 (noise-floor exit) or 1 (OpenCV's fixed 300 sweeps)");
    ctx->dk_early = kind == 0;
    return VO_OK;
}

extern "C" int vo_set_pnp_refine(vo_ctx* ctx, int kind)
{
    if (!ctx) return VO_ERR_INVALID;
    if (kind != 0 && kind != 1) FAIL(VO_ERR_INVALID, "pnp refine must be 1 (cv2's solvePnP(ITERATIVE) on the inliers) or 0 (fast minimiser from the RANSAC model)");
    ctx->pnp_refine = kind;
    return VO_OK;
}

extern "C" int vo_set_slam_stats(vo_ctx* ctx, int on)
{
    if (!ctx) return VO_ERR_INVALID;
    if (on != 0 && on != 1) FAIL(VO_ERR_INVALID, "slam stats must be 0 (off) or 1 (one k_slam_stats launch per step of every vo_slam_* call)");
    ctx->slam_stats = on;
    return VO_OK;
}

extern "C" const char* vo_last_error(const vo_ctx* ctx) { return ctx ? ctx->err : "ctx is NULL"; }

// ------------------------------------------------------------------ configuration
extern "C" int vo_batch_configure(vo_ctx* ctx, int h, int w, const vo_orb_params* params, int max_frames, int max_pairs)
{
    if (!ctx) return VO_ERR_INVALID;
    int rc = check_params(ctx, params);
    if (rc) return rc;
    if (h < 1 || w < 1 || max_frames < 1 || max_pairs < 1) FAIL(VO_ERR_INVALID, "bad sizes");
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->configured && ctx->h == h && ctx->w == w && memcmp(&ctx->params, params, sizeof(*params)) == 0 &&
        ctx->max_frames >= max_frames && ctx->max_pairs >= max_pairs && ctx->pb_cap == ctx->g.kp_cap) {
        ctx->detector = 0;
        clear_last_run(ctx);
        drop_slam_stream(ctx);
        return VO_OK;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    free_config(ctx);
    PyrGeom g;
    rc = make_geometry(ctx, h, w, params, &g);
    if (rc) return rc;
    ctx->g = g; ctx->h = h; ctx->w = w; ctx->params = *params;
    ctx->max_frames = max_frames; ctx->max_pairs = max_pairs;

    // resize tables
    size_t tab_ints = 0, tab_u16 = 0;
    for (int l = 1; l < g.nlevels; l++) { tab_ints += g.lv[l].w + g.lv[l].h; tab_u16 += g.lv[l].w + g.lv[l].h; }
    std::vector<int> hofs(tab_ints + 1);
    std::vector<uint16_t> hc(tab_u16 + 1);
    const size_t int_bytes = (tab_ints + 1) * sizeof(int);
    DevList& m = ctx->orb_mem;
    uint8_t* tab_mem = nullptr;
    HIPCHK(m.alloc(&tab_mem, int_bytes + (tab_u16 + 1) * sizeof(uint16_t) + 64));
    int* d_ofs = (int*)tab_mem;
    uint16_t* d_c = (uint16_t*)(tab_mem + int_bytes);
    size_t oi = 0;
    for (int l = 1; l < g.nlevels; l++) {
        ResizeTab& t = ctx->tabs[l];
        const LevelGeom &s = g.lv[l - 1], &d = g.lv[l];
        build_lin_tab(s.w, d.w, &hofs[oi], &hc[oi], &t.min_x, &t.max_x);
        t.xofs = d_ofs + oi; t.xc1 = d_c + oi; oi += d.w;
        build_lin_tab(s.h, d.h, &hofs[oi], &hc[oi], &t.min_y, &t.max_y);
        t.yofs = d_ofs + oi; t.yc1 = d_c + oi; oi += d.h;
        // k_resize_direct's assumptions (they hold for scale factors <= 1.27, ORB's 1.2 included): 4 destination pixels read
        // within an 8-byte source window starting at the first one's tap; every source row is the lower row of at most one
        // destination row; the 16 destination rows of a wavefront span at most 23 source rows.  Otherwise: the generic k_resize.
        {
            const int* xo = &hofs[oi - d.h - d.w]; const int* yo = &hofs[oi - d.h];
            bool ok = true;
            for (int x = 0; x + 3 < d.w && ok; x++) ok = xo[x + 3] - xo[x] <= 4;
            for (int y = 0; y + 1 < d.h && ok; y++) ok = yo[y + 1] > yo[y];
            for (int y0 = 0; y0 < d.h && ok; y0 += RS2_WH) { const int yl = (y0 + RS2_WH < d.h ? y0 + RS2_WH : d.h) - 1; ok = yo[yl] + 2 - yo[y0] <= (RS2_WH * 127 + 99) / 100 + 3; }
            t.direct = ok ? 1 : 0;
        }
    }
    HIPCHK(hipMemcpy(d_ofs, hofs.data(), int_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_c, hc.data(), (tab_u16 + 1) * sizeof(uint16_t), hipMemcpyHostToDevice));

    const size_t F = (size_t)max_frames, fb = (size_t)g.frame_bytes;
    HIPCHK(m.alloc(&ctx->pyr, F * fb + 256));                  // + slack: k_resize_direct reads whole dwords around its last taps
    HIPCHK(m.alloc(&ctx->blur, F * fb));
    HIPCHK(m.alloc(&ctx->score, F * fb));
    HIPCHK(hipMemset(ctx->pyr, 0, F * fb));
    FrameFeat& ff = ctx->ff;
    HIPCHK(m.alloc(&ff.cand_pos, F * g.cand_total)); HIPCHK(m.alloc(&ff.cand_resp, F * g.cand_total));
    HIPCHK(m.alloc(&ff.cand_count, F * VO_MAX_LEVELS));
    HIPCHK(m.alloc(&ff.kp_pos, F * g.kp_cap)); HIPCHK(m.alloc(&ff.kp_level, F * g.kp_cap));
    HIPCHK(m.alloc(&ff.kp_resp, F * g.kp_cap)); HIPCHK(m.alloc(&ff.kp_angle, F * g.kp_cap));
    HIPCHK(m.alloc(&ff.kp_xy, F * g.kp_cap * 2)); HIPCHK(m.alloc(&ff.kp_size, F * g.kp_cap));
    HIPCHK(m.alloc(&ff.desc, F * g.kp_cap * 32));
    HIPCHK(m.alloc(&ctx->desc_x, F * (size_t)desc_x_rows(g.kp_cap) * 256));
    // k_brief writes only the rows below kp_count; k_nn_mfma still multiplies the rest of the last 16-row group and
    // relies on |dot| <= 16384, which holds for +1 / -1 bytes but not for whatever a recycled allocation held
    HIPCHK(hipMemset(ctx->desc_x, 0xFF, F * (size_t)desc_x_rows(g.kp_cap) * 256));
    HIPCHK(m.alloc(&ff.kp_count, F)); HIPCHK(m.alloc(&ff.flags, F));
    HIPCHK(m.alloc(&ff.hist, F * VO_MAX_LEVELS * 256));
    HIPCHK(m.alloc(&ff.tile_list, F * (size_t)g.ftiles_total * FAST_LISTCAP));
    HIPCHK(m.alloc(&ff.tile_count, F * (size_t)g.ftiles_total));
    HIPCHK(m.alloc(&ctx->sel_thr, F * VO_MAX_LEVELS));
    HIPCHK(m.alloc(&ctx->har_kept, F * VO_MAX_LEVELS));
    HIPCHK(m.alloc(&ctx->har_thr, F * VO_MAX_LEVELS));
    HIPCHK(m.alloc(&ctx->sel_chunk_count, F * (size_t)(g.sel_chunks_total + 1)));
    HIPCHK(hipMemset(ff.kp_count, 0, F * sizeof(int)));
    HIPCHK(hipMemset(ff.flags, 0, F * sizeof(int)));
    HIPCHK(alloc_pairbuf(ctx->pb_mem, ctx->pb, max_pairs, g.kp_cap, false));
    ctx->pb_pairs = max_pairs; ctx->pb_cap = g.kp_cap;
    HIPCHK(hipDeviceSynchronize());                         // the initialising memsets ran on the NULL stream
    ctx->configured = true;
    ctx->detector = 0;
    if (ctx->kp_order == 1) { rc = alloc_cv2(ctx); if (rc) return rc; }
    return VO_OK;
}

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

static Batch batch(const vo_ctx* ctx)
{
    if (ctx->detector == 1) {
        const SiftState& S = ctx->sift;
        return {true, S.configured, S.w, S.h, S.max_frames, ctx->sift_pairs, S.kp_cap, S.desc, S.desc_x, S.kp_xy, S.kp_count, S.flags, S.norms, 0,
                S.frames, S.fstride, (size_t)S.fstride * S.h};
    }
    const PyrGeom& g = ctx->g;
    return {false, ctx->configured, ctx->w, ctx->h, ctx->max_frames, ctx->max_pairs, g.kp_cap, ctx->ff.desc, ctx->desc_x, ctx->ff.kp_xy,
            ctx->ff.kp_count, ctx->ff.flags, nullptr, ctx->descx_fp4 > 0, ctx->pyr + g.lv[0].off, g.lv[0].stride, (size_t)g.frame_bytes};
}

// Bytes from the first byte of a host image (stack) to the last byte of its last row: n frames at frame_stride, h rows of row_bytes
// at row_stride.  The layout contract of include/vo_hip.h: no host-to-device image copy reads beyond it.  Tight strides
// (row_stride == row_bytes, frame_stride == h * row_stride) give n * h * row_bytes.
static inline size_t image_span(int n, int64_t frame_stride, int h, int row_stride, int row_bytes)
{
    return (size_t)(n - 1) * (size_t)frame_stride + (size_t)(h - 1) * (size_t)row_stride + (size_t)row_bytes;
}

// cvtColor(BGR2GRAY) (or a copy of gray input) of n device frames into slots first_slot..
static void gray_into_slots(vo_ctx* ctx, hipStream_t s, const uint8_t* src, int channels, int row_stride, int64_t frame_stride, int first_slot, int n)
{
    const Batch b = batch(ctx);
    if (b.sift) launch_gray_plain(s, src, channels, row_stride, frame_stride, b.gray_slot(first_slot), b.w, b.h, b.gray_stride, (int64_t)b.gray_frame, n);
    else launch_gray(s, src, channels, row_stride, frame_stride, ctx->pyr + (size_t)first_slot * ctx->g.frame_bytes, ctx->g, n);
}

static int frames_upload_enqueue(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot)
{
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (!frames || F < 0 || first_slot < 0 || first_slot + F > b.max_frames) FAIL(VO_ERR_INVALID, "slot range out of bounds");
    slam_stream_slots_written(ctx, first_slot, F);
    if (row_stride < b.w) FAIL(VO_ERR_INVALID, "row_stride < width");
    if (F == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    if (b.sift) return sift_frames_upload_enqueue(ctx, frames, F, row_stride, frame_stride, first_slot);
    const LevelGeom& lv = ctx->g.lv[0];
    uint8_t* dst0 = ctx->pyr + (size_t)first_slot * ctx->g.frame_bytes + lv.off;
    if (row_stride == ctx->w && lv.stride == ctx->w && frame_stride >= (int64_t)ctx->w * ctx->h) {
        // dense frames and an unpadded level 0: the whole batch is ONE strided copy (a "row" = a frame)
        HIPCHK(hipMemcpy2DAsync(dst0, ctx->g.frame_bytes, frames, (size_t)frame_stride, (size_t)ctx->w * ctx->h, F,
                                hipMemcpyHostToDevice, ctx->stream));
        return VO_OK;
    }
    if (row_stride == ctx->w && frame_stride >= (int64_t)ctx->w * ctx->h) {
        // dense frames, padded level-0 rows (width not a multiple of 64, e.g. KITTI's 1241): ONE transfer of the dense bytes into
        // a staging buffer, then a kernel lays the rows out (a 2-D copy per frame runs at a fraction of the PCIe rate)
        const size_t per = (size_t)ctx->w * ctx->h;
        int rc = ctx->staging.grow(ctx, per * F); if (rc) return rc;
        HIPCHK(hipMemcpy2DAsync(ctx->staging.p, per, frames, (size_t)frame_stride, per, F, hipMemcpyHostToDevice, ctx->stream));
        launch_gray(ctx->stream, ctx->staging.p, 1, ctx->w, (int64_t)per, ctx->pyr + (size_t)first_slot * ctx->g.frame_bytes, ctx->g, F);
        HIPCHK(hipGetLastError());
        return VO_OK;
    }
    for (int f = 0; f < F; f++)
        HIPCHK(hipMemcpy2DAsync(dst0 + (size_t)f * ctx->g.frame_bytes, lv.stride, frames + (size_t)f * frame_stride, row_stride,
                                ctx->w, ctx->h, hipMemcpyHostToDevice, ctx->stream));
    return VO_OK;
}

extern "C" int vo_frames_upload(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot)
{
    if (!ctx) return VO_ERR_INVALID;
    int rc = frames_upload_enqueue(ctx, frames, F, row_stride, frame_stride, first_slot);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

// Enqueue only (gray frames).  With page-locked source memory (vo_host_alloc) the copy runs on the DMA engines
// behind the work already queued on this ctx and beside the other ctx's kernels; the source must stay untouched
// until the next vo_sync(ctx).
extern "C" int vo_frames_upload_async(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot)
{
    if (!ctx) return VO_ERR_INVALID;
    return frames_upload_enqueue(ctx, frames, F, row_stride, frame_stride, first_slot);
}

extern "C" int vo_frames_upload_color(vo_ctx* ctx, const uint8_t* frames, int F, int channels, int row_stride,
                                      int64_t frame_stride, int first_slot)
{
    if (!ctx) return VO_ERR_INVALID;
    if (channels == 1) return vo_frames_upload(ctx, frames, F, row_stride, frame_stride, first_slot);
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (channels != 3 && channels != 4) FAIL(VO_ERR_INVALID, "channels must be 1, 3 or 4");
    if (!frames || F < 0 || first_slot < 0 || first_slot + F > b.max_frames) FAIL(VO_ERR_INVALID, "slot range out of bounds");
    slam_stream_slots_written(ctx, first_slot, F);
    if (row_stride < b.w * channels || frame_stride < (int64_t)image_span(1, 0, b.h, row_stride, b.w * channels)) FAIL(VO_ERR_INVALID, "strides too small");
    if (F == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t per = (size_t)frame_stride;
    // B G R (A) frames pass through a staging buffer (at most 64 frames of it, grown once: the first call of a size pays for it);
    // the chunks follow one another in stream order — the next chunk's copy waits for the previous chunk's conversion by
    // itself — and the call returns when the last conversion has finished
    const int chunk = F < 64 ? F : 64;
    int rc = ctx->staging.grow(ctx, per * chunk); if (rc) return rc;
    for (int f0 = 0; f0 < F; f0 += chunk) {
        const int n = F - f0 < chunk ? F - f0 : chunk;
        HIPCHK(hipMemcpyAsync(ctx->staging.p, frames + (size_t)f0 * per, image_span(n, frame_stride, b.h, row_stride, b.w * channels),
                              hipMemcpyHostToDevice, ctx->stream));
        StageTimer t(ctx, ST_GRAY);
        gray_into_slots(ctx, ctx->stream, ctx->staging.p, channels, row_stride, frame_stride, first_slot + f0, n);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// stages up to `upto` (0 = pyramid only, 1 = + FAST score map, 2 = everything)
static int run_detect(vo_ctx* ctx, int first_slot, int F, int upto)
{
    const PyrGeom& g = ctx->g;
    hipStream_t s = ctx->stream;
    uint8_t* pyr = ctx->pyr + (size_t)first_slot * g.frame_bytes;
    uint8_t* blur = ctx->blur + (size_t)first_slot * g.frame_bytes;
    uint8_t* score = ctx->score + (size_t)first_slot * g.frame_bytes;
    FrameFeat ff = ctx->ff;
    ff.cand_pos += (size_t)first_slot * g.cand_total; ff.cand_resp += (size_t)first_slot * g.cand_total;
    ff.cand_count += (size_t)first_slot * VO_MAX_LEVELS;
    ff.kp_pos += (size_t)first_slot * g.kp_cap; ff.kp_level += (size_t)first_slot * g.kp_cap;
    ff.kp_resp += (size_t)first_slot * g.kp_cap; ff.kp_angle += (size_t)first_slot * g.kp_cap;
    ff.kp_xy += (size_t)first_slot * g.kp_cap * 2; ff.kp_size += (size_t)first_slot * g.kp_cap;
    ff.desc += (size_t)first_slot * g.kp_cap * 32;
    ff.kp_count += first_slot; ff.flags += first_slot;
    ff.hist += (size_t)first_slot * VO_MAX_LEVELS * 256;
    ff.tile_list += (size_t)first_slot * g.ftiles_total * FAST_LISTCAP; ff.tile_count += (size_t)first_slot * g.ftiles_total;
    {
        StageTimer t(ctx, ST_RESIZE);
        for (int l = 1; l < g.nlevels; l++) launch_resize(s, pyr, g, l, ctx->tabs[l], F);
    }
    if (upto < 1) return VO_OK;
    const bool cv2 = ctx->kp_order == 1 && ctx->cv2_ready;
    Cv2Buf cb = ctx->cv2;
    if (cv2) {
        const size_t fo = (size_t)first_slot;
        cb.all_pos += fo * cb.all_total; cb.all_resp += fo * cb.all_total; cb.work += fo * cb.all_total;
        cb.all_cand += fo * cb.all_total; cb.lpos += fo * cb.all_total; cb.rpos += fo * cb.all_total;
        cb.all_count += fo * VO_MAX_LEVELS; cb.chunk_count += fo * g.sel_chunks_total;
    }
    {
        StageTimer t(ctx, ST_MISC);
        HIPCHK(hipMemsetAsync(ff.hist, 0, (size_t)F * VO_MAX_LEVELS * 256 * sizeof(uint32_t), s));
        // the selection clears the flags and writes every level's counts itself (launch_select_fast); a run that stops at the
        // score map leaves them cleared as before
        if (upto < 2) {
            HIPCHK(hipMemsetAsync(ff.flags, 0, (size_t)F * sizeof(int), s));
            HIPCHK(hipMemsetAsync(ff.cand_count, 0, (size_t)F * VO_MAX_LEVELS * sizeof(int), s));
            if (cv2) HIPCHK(hipMemsetAsync(cb.all_count, 0, (size_t)F * VO_MAX_LEVELS * sizeof(int), s));
        }
    }
    { StageTimer t(ctx, ST_FAST); launch_fast(s, pyr, score, ff.hist, g, F, upto < 2 ? nullptr : ff.tile_list, ff.tile_count); }
    if (upto < 2) return VO_OK;
    { StageTimer t(ctx, ST_SELECT_FAST); launch_select_fast(s, g, ff, F, ctx->sel_thr + (size_t)first_slot * VO_MAX_LEVELS, ctx->sel_chunk_count + (size_t)first_slot * g.sel_chunks_total, ff.tile_list, ff.tile_count, cv2 ? &cb : nullptr); }
    if (g.score_type == 0) { StageTimer t(ctx, ST_HARRIS); launch_harris(s, pyr, g, ff, F); }
    { StageTimer t(ctx, ST_SELECT_HARRIS); launch_select_harris(s, g, ff, F, ctx->har_thr + (size_t)first_slot * VO_MAX_LEVELS, ctx->har_kept + (size_t)first_slot * VO_MAX_LEVELS); }
    if (cv2) {
        // cv2's list order: permute every level's keypoints the way retainBest's nth_element / partition leave them
        StageTimer t(ctx, ST_CV2_ORDER);
        launch_cv2_order(s, g, ff, cb, F, ctx->har_kept + (size_t)first_slot * VO_MAX_LEVELS);
    }
    { StageTimer t(ctx, ST_ANGLE); launch_angle(s, pyr, g, ff, F); }
    { StageTimer t(ctx, ST_BLUR); launch_blur(s, pyr, blur, g, F); }
    {
        StageTimer t(ctx, ST_BRIEF);
        const int cx = desc_x_rows(g.kp_cap);
        const int fp4 = descx_begin_write(ctx, first_slot, F);
        launch_brief(s, blur, g, ff, F, ctx->desc_x + (size_t)first_slot * cx * 256, cx, fp4);
    }
    return VO_OK;
}

extern "C" int vo_batch_kp_capacity(vo_ctx* ctx)
{
    if (!ctx) return 0;
    const Batch b = batch(ctx);
    return b.ready ? b.kp_cap : 0;
}

extern "C" int vo_host_alloc(size_t bytes, void** out)
{
    if (!out) return VO_ERR_INVALID;
    *out = nullptr;
    return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? VO_OK : VO_ERR_HIP;
}

extern "C" void vo_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

// the detection of slots first_slot .. first_slot + F - 1 with the configured detector, enqueued on the context's stream
static int detect_enqueue(vo_ctx* ctx, int first_slot, int F)
{
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (F < 0 || first_slot < 0 || first_slot + F > b.max_frames) FAIL(VO_ERR_INVALID, "slot range out of bounds");
    slam_stream_slots_written(ctx, first_slot, F);
    HIPCHK(hipSetDevice(ctx->device));
    if (F == 0) return VO_OK;
    if (b.sift) return sift_frames_detect_enqueue(ctx, first_slot, F);
    int rc = run_detect(ctx, first_slot, F, 2);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return VO_OK;
}

extern "C" int vo_frames_detect_async(vo_ctx* ctx, int first_slot, int F)
{
    if (!ctx) return VO_ERR_INVALID;
    int rc = detect_enqueue(ctx, first_slot, F);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->ev_det, ctx->stream));
    ctx->ev_det_set = true;
    return VO_OK;
}

// Software pipelining over two contexts of one GPU: ctx's next work starts only after `other`'s most recent
// vo_frames_detect_async has finished.  Chaining the detections (A.detect -> B.detect -> A.detect ...) keeps the
// two contexts out of phase, so each one's latency-bound RANSAC / pose kernels always run beside the other's
// issue-bound ORB kernels instead of beside its RANSAC.
extern "C" int vo_detect_after(vo_ctx* ctx, vo_ctx* other)
{
    if (!ctx || !other) return VO_ERR_INVALID;
    if (ctx->device != other->device) FAIL(VO_ERR_INVALID, "the two contexts are on different devices");
    if (ctx == other || !other->ev_det_set) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamWaitEvent(ctx->stream, other->ev_det, 0));
    return VO_OK;
}

#define SIFT_NORM_BOUND_MSG "a SIFT descriptor row broke the norm bound of the integer matcher (slot %d)"
// VO_ERR_INVALID if a slot of the pair list `slots` holds a flagged SIFT row (flags bit 1), else
// VO_WARN_CAPACITY if a keypoint / candidate list of one of the given slots overflowed (flags bit 0) — after a stream sync.
// SIFT cuts an over-full frame at kp_cap in cv2's list order (x ascending after removeDuplicatedSorted): the keypoints at the
// right edge of the image are the ones lost, so a caller should know before it trusts the pose of such a pair.
static int capacity_warning(vo_ctx* ctx, const int32_t* slots, int n, int first_slot, int F)
{
    const Batch b = batch(ctx);
    if (!b.ready || b.max_frames <= 0) return VO_OK;
    std::vector<int> fl((size_t)b.max_frames);
    HIPCHK(hipMemcpy(fl.data(), b.flags, (size_t)b.max_frames * sizeof(int), hipMemcpyDeviceToHost));
    // (SIFT, flags bit 1: a descriptor row of a pair's slot broke the norm bound under which k_nn_l2i8's integer order is cv2's
    // float order — the matches of that pair cannot be trusted, which is an error and not a warning)
    if (b.sift)
        for (int i = 0; i < n; i++)
            if (fl[(size_t)slots[i]] & 2) FAIL(VO_ERR_INVALID, SIFT_NORM_BOUND_MSG, (int)slots[i]);
    for (int i = 0; i < F; i++) if (fl[(size_t)first_slot + i] & 1) return VO_WARN_CAPACITY;
    for (int i = 0; i < n; i++) if (fl[(size_t)slots[i]] & 1) return VO_WARN_CAPACITY;
    return VO_OK;
}

extern "C" int vo_frames_detect(vo_ctx* ctx, int first_slot, int F)
{
    if (!ctx) return VO_ERR_INVALID;
    int rc = detect_enqueue(ctx, first_slot, F);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    return capacity_warning(ctx, nullptr, 0, first_slot, F);
}

// The device arrays of a detector's keypoints: [slot][kp_cap] each, xy two floats and desc desc_bytes per keypoint
struct KpArrays { const float *xy, *size, *angle, *resp; const int* octave; const uint8_t* desc; int desc_bytes; };

// n keypoints from row `first` of the arrays into the caller's (a NULL output is skipped)
static int download_keypoints(vo_ctx* ctx, const KpArrays& d, size_t first, int n, float* kp_xy, float* kp_size, float* kp_angle,
                              float* kp_response, int32_t* kp_octave, uint8_t* desc)
{
    if (n <= 0) return VO_OK;
    if (kp_xy) HIPCHK(hipMemcpy(kp_xy, d.xy + first * 2, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (kp_size) HIPCHK(hipMemcpy(kp_size, d.size + first, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (kp_angle) HIPCHK(hipMemcpy(kp_angle, d.angle + first, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (kp_response) HIPCHK(hipMemcpy(kp_response, d.resp + first, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (kp_octave) HIPCHK(hipMemcpy(kp_octave, d.octave + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (desc) HIPCHK(hipMemcpy(desc, d.desc + first * d.desc_bytes, (size_t)n * d.desc_bytes, hipMemcpyDeviceToHost));
    return VO_OK;
}

extern "C" int vo_frame_features(vo_ctx* ctx, int slot, float* kp_xy, float* kp_size, float* kp_angle, float* kp_response,
                                 int32_t* kp_octave, uint8_t* desc, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!ctx->configured) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (slot < 0 || slot >= ctx->max_frames || !n_out) FAIL(VO_ERR_INVALID, "bad slot");
    HIPCHK(hipSetDevice(ctx->device));
    const FrameFeat& ff = ctx->ff;
    int n = 0, flags = 0;
    HIPCHK(hipStreamSynchronize(ctx->stream));              // an asynchronous detection may still be running
    HIPCHK(hipMemcpy(&n, ff.kp_count + slot, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&flags, ff.flags + slot, sizeof(int), hipMemcpyDeviceToHost));
    int warn = (flags & 1) ? VO_WARN_CAPACITY : VO_OK;
    if (n > cap) { n = cap; warn = VO_WARN_CAPACITY; }
    *n_out = n;
    const int rc = download_keypoints(ctx, {ff.kp_xy, ff.kp_size, ff.kp_angle, ff.kp_resp, ff.kp_level, ff.desc, 32}, (size_t)slot * ctx->g.kp_cap, n,
                                      kp_xy, kp_size, kp_angle, kp_response, kp_octave, desc);
    return rc ? rc : warn;
}

// Parity seam of the Hamming matchers (a test seam, not a production entry): n descriptor rows the caller chose become slot `slot`
// exactly as a detection of that one slot would leave them — ff.desc rows 0 .. n - 1, kp_count = n, kp_xy = xy (zeros without),
// size / angle / response / octave / level zero for those rows, the flags clear, and the matcher's operand image of the slot
// written by k_desc_expand in the format nn_kernel selects now.  ff.desc rows past n keep what an earlier, fuller frame left
// there: k_nn_pairs has to bound its reads by the count alone.
extern "C" int vo_stage_orb_rows(vo_ctx* ctx, int slot, const uint8_t* rows, int n, const float* xy)
{
    if (!ctx) return VO_ERR_INVALID;
    if (ctx->detector != 0 || !ctx->configured) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    const PyrGeom& g = ctx->g;
    if (slot < 0 || slot >= ctx->max_frames) FAIL(VO_ERR_INVALID, "bad slot");
    if (n < 0 || n > g.kp_cap || (n > 0 && !rows)) FAIL(VO_ERR_INVALID, "0 <= n <= kp_cap rows are needed");
    slam_stream_slots_written(ctx, slot, 1);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIPCHK(hipStreamSynchronize(s));                        // an asynchronous detection may still be writing the slot
    const FrameFeat& ff = ctx->ff;
    const size_t o = (size_t)slot * g.kp_cap;
    HIPCHK(hipMemsetAsync(ff.flags + slot, 0, sizeof(int), s));
    HIPCHK(hipMemcpyAsync(ff.kp_count + slot, &n, sizeof(int), hipMemcpyHostToDevice, s));
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(ff.desc + o * 32, rows, (size_t)n * 32, hipMemcpyHostToDevice, s));
        if (xy) HIPCHK(hipMemcpyAsync(ff.kp_xy + o * 2, xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(ff.kp_xy + o * 2, 0, (size_t)n * 2 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(ff.kp_size + o, 0, (size_t)n * sizeof(float), s)); HIPCHK(hipMemsetAsync(ff.kp_angle + o, 0, (size_t)n * sizeof(float), s));
        HIPCHK(hipMemsetAsync(ff.kp_resp + o, 0, (size_t)n * sizeof(float), s)); HIPCHK(hipMemsetAsync(ff.kp_level + o, 0, (size_t)n * sizeof(int), s));
    }
    const int cx = desc_x_rows(g.kp_cap), fp4 = descx_begin_write(ctx, slot, 1);
    launch_desc_expand(s, ff.desc + o * 32, ff.kp_count + slot, g.kp_cap, cx, ctx->desc_x + (size_t)slot * cx * 256, 1, fp4);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));                        // (the caller's rows, xy and n have been read)
    return VO_OK;
}

// upload one host image (any channel count) into slot 0 and build its gray level 0
static int load_single(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride, const vo_orb_params* params)
{
    if (!img || h < 1 || w < 1) FAIL(VO_ERR_INVALID, "bad image");
    if (channels != 1 && channels != 3 && channels != 4) FAIL(VO_ERR_INVALID, "channels must be 1, 3 or 4");
    if (row_stride < w * channels) FAIL(VO_ERR_INVALID, "row_stride too small");
    int mf = ctx->configured ? ctx->max_frames : 1, mp = ctx->configured ? ctx->max_pairs : 1;
    int rc = vo_batch_configure(ctx, h, w, params, mf, mp);
    if (rc) return rc;
    if (channels == 1) return vo_frames_upload(ctx, img, 1, row_stride, 0, 0);
    const size_t bytes = image_span(1, 0, h, row_stride, w * channels);
    rc = ctx->staging.grow(ctx, bytes); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->staging.p, img, bytes, hipMemcpyHostToDevice, ctx->stream));
    { StageTimer t(ctx, ST_GRAY); launch_gray(ctx->stream, ctx->staging.p, channels, row_stride, 0, ctx->pyr, ctx->g, 1); }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return VO_OK;
}

extern "C" int vo_orb_detect_and_compute(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                                         const vo_orb_params* params, float* kp_xy, float* kp_size, float* kp_angle,
                                         float* kp_response, int32_t* kp_octave, uint8_t* desc, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!n_out || cap < 0) FAIL(VO_ERR_INVALID, "bad output arguments");
    int rc = check_params(ctx, params);
    if (rc) return rc;
    rc = load_single(ctx, img, h, w, channels, row_stride, params);
    if (rc) return rc;
    rc = vo_frames_detect(ctx, 0, 1);
    if (rc) return rc;
    return vo_frame_features(ctx, 0, kp_xy, kp_size, kp_angle, kp_response, kp_octave, desc, cap, n_out);
}

// download a padded per-level buffer of slot 0 into tight packing
static int download_packed(vo_ctx* ctx, const uint8_t* dev_base, uint8_t* out)
{
    const PyrGeom& g = ctx->g;
    std::vector<uint8_t> tmp((size_t)g.frame_bytes);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(tmp.data(), dev_base, (size_t)g.frame_bytes, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (int l = 0; l < g.nlevels; l++) {
        const LevelGeom& lv = g.lv[l];
        for (int y = 0; y < lv.h; y++) { memcpy(out + o, tmp.data() + lv.off + (size_t)y * lv.stride, (size_t)lv.w); o += lv.w; }
    }
    return VO_OK;
}

static int stage_common(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                        const vo_orb_params* params, int upto)
{
    if (!ctx) return VO_ERR_INVALID;
    int rc = check_params(ctx, params);
    if (rc) return rc;
    rc = load_single(ctx, img, h, w, channels, row_stride, params);
    if (rc) return rc;
    rc = run_detect(ctx, 0, 1, upto);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// bytes vo_stage_pyramid / vo_stage_fast_scores / vo_stage_blur write (levels packed tightly): sum of w_l * h_l
extern "C" int64_t vo_packed_pyramid_bytes(int h, int w, const vo_orb_params* params)
{
    if (!params || h < 1 || w < 1 || params->nlevels < 1 || params->nlevels > VO_MAX_LEVELS || !(params->scale_factor > 1.0f)) return VO_ERR_INVALID;
    int64_t total = 0;
    for (int l = 0; l < params->nlevels; l++) {
        const float scale = (float)pow((double)params->scale_factor, (double)l);
        const int lw = cv_round_f((float)w / scale), lh = cv_round_f((float)h / scale);
        if (lw < 1 || lh < 1) return VO_ERR_INVALID;
        total += (int64_t)lw * lh;
    }
    return total;
}

extern "C" int vo_stage_pyramid(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                                const vo_orb_params* params, uint8_t* out_packed)
{
    int rc = stage_common(ctx, img, h, w, channels, row_stride, params, 0);
    return rc ? rc : download_packed(ctx, ctx->pyr, out_packed);
}

extern "C" int vo_stage_fast_scores(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                                    const vo_orb_params* params, uint8_t* out_packed)
{
    int rc = stage_common(ctx, img, h, w, channels, row_stride, params, 1);
    return rc ? rc : download_packed(ctx, ctx->score, out_packed);
}

extern "C" int vo_stage_blur(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride,
                             const vo_orb_params* params, uint8_t* out_packed)
{
    int rc = stage_common(ctx, img, h, w, channels, row_stride, params, 2);
    return rc ? rc : download_packed(ctx, ctx->blur, out_packed);
}

// ------------------------------------------------------------------ pairs
// cv::RNG (multiply-with-carry, core/operations.hpp RNG::next) output stream for `seed`; it depends on
// nothing but the seed, so it is tabulated once and shared by every pair of every batch.
#define RNG_TAB_N 8192
static int ensure_rng(vo_ctx* ctx, uint64_t seed)
{
    if (ctx->rng_valid && ctx->rng_seed == seed) return VO_OK;
    if (!ctx->rng_tab) HIPCHK(ctx->mem.alloc(&ctx->rng_tab, RNG_TAB_N));
    if (!ctx->rng_host) HIPCHK(ctx->mem.alloc_pinned(&ctx->rng_host, RNG_TAB_N));
    // an earlier asynchronous batch may still be reading the table (and the host buffer may still be feeding the
    // previous copy): the rewrite is ordered on the ctx stream, behind both
    HIPCHK(hipStreamSynchronize(ctx->stream));
    uint32_t* tab = ctx->rng_host;
    uint64_t st = seed ? seed : 0xffffffffULL;
    for (int i = 0; i < RNG_TAB_N; i++) {
        st = (uint64_t)(uint32_t)st * 4164903690ULL + (uint32_t)(st >> 32);
        tab[i] = (uint32_t)st;
    }
    HIPCHK(hipMemcpyAsync(ctx->rng_tab, tab, RNG_TAB_N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    ctx->rng_seed = seed; ctx->rng_valid = true;
    return VO_OK;
}

// vo_pair_opts.match_mode -> k_match_select mode.  BFMatcher(crossCheck=True) of OpenCV 4.x is the strict mutual
// nearest neighbour (batchDistance compares the forward result too: `d < d0 && sidx[idx] == i`); the older
// reverse-NN-only update rule stays selectable as match_mode 2; 3 is BFMatcher(crossCheck=False).match, every query's nearest.
static int map_select_mode(int match_mode) { return match_mode == 0 ? 2 : match_mode == 2 ? 1 : match_mode == 3 ? 0 : 3; }

static int run_pairs(vo_ctx* ctx, PairBuf pb, const uint8_t* desc, const uint8_t* desc_x, const float* kp_xy, const int* kp_count, int cap,
                     int P, int select_mode, double ratio, const RansacParams& rp, bool do_geometry, bool want_points, int descx_fp4,
                     const int* l2_norms = nullptr)
{
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemsetAsync(pb.res, 0, (size_t)P * sizeof(vo_pair_result), s));
    const int knn2 = select_mode == 3, dirs = select_mode == 1 ? 2 : select_mode == 2 ? 3 : 1;
    int col_parts = 0;                                           // the FP4 single pass left the reverse direction as column keys
    {
        StageTimer t(ctx, ST_MATCH_NN);
        if (l2_norms) launch_match_nn_l2i8(s, desc_x, l2_norms, kp_count, cap, desc_x_rows(cap), pb, P, dirs, knn2);   // SIFT rows: squared L2 distances
        else col_parts = launch_hamming_nn(ctx, pb, desc, desc_x, descx_fp4, kp_count, cap, P, dirs, knn2);
    }
    { StageTimer t(ctx, ST_MATCH_SELECT); launch_match_select(s, kp_xy, kp_count, cap, pb, P, select_mode, ratio, ctx->dK, l2_norms ? 1 : 0, col_parts); }
    if (!do_geometry) return VO_OK;
    { int rc = ensure_rng(ctx, rp.seed); if (rc) return rc; }
    { StageTimer t(ctx, ST_RANSAC); launch_ransac(s, pb, cap, P, rp, ctx->rng_tab, RNG_TAB_N); }
    { StageTimer t(ctx, ST_POSE); launch_pose(s, pb, cap, P, rp); }
    if (want_points) { StageTimer t(ctx, ST_TRIANGULATE); launch_triangulate_pairs(s, pb, cap, P, rp); }
    return VO_OK;
}

static int pairs_enqueue(vo_ctx* ctx, const int32_t* pair_slots, int B, const double* K, const vo_pair_opts* opts,
                         vo_pair_result* results, double* X, int32_t x_cap, bool* whole_x_out)
{
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (!pair_slots || !K || !opts || !results || B < 0 || B > b.max_pairs) FAIL(VO_ERR_INVALID, "bad pair batch arguments");
    if (opts->match_mode < 0 || opts->match_mode > 3) FAIL(VO_ERR_INVALID, "match_mode must be 0, 1, 2 or 3");
    if (!(opts->ransac_prob > 0 && opts->ransac_prob < 1)) FAIL(VO_ERR_INVALID, "ransac_prob must be in (0, 1)");
    for (int i = 0; i < 2 * B; i++)
        if (pair_slots[i] < 0 || pair_slots[i] >= b.max_frames) FAIL(VO_ERR_INVALID, "pair slot %d out of range", pair_slots[i]);
    *whole_x_out = false;
    clear_last_run(ctx);                                    // the pair buffers are about to be overwritten
    const bool wp = opts->want_points != 0;
    auto done = [&]() {
        ctx->last.pairs = B;
        ctx->last.slots.assign(pair_slots, pair_slots + 2 * (size_t)B);
        ctx->last.points = wp;
        ctx->last.match_mode = opts->match_mode;
        return VO_OK;
    };
    if (B == 0) return done();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int cap = b.kp_cap;
    HIPCHK(hipMemcpyAsync(ctx->pb.slots, pair_slots, (size_t)B * 2 * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->dK, K, 9 * sizeof(double), hipMemcpyHostToDevice, s));
    RansacParams rp{};
    rp.prob = opts->ransac_prob; rp.thresh_px = opts->ransac_thresh; rp.max_iters = opts->ransac_max_iters;
    rp.seed = opts->ransac_seed; rp.dist_thresh = opts->pose_dist_thresh; rp.dk_early = ctx->dk_early;
    memcpy(rp.K, K, sizeof(rp.K));
    int rc = run_pairs(ctx, ctx->pb, b.desc, b.desc_x, b.kp_xy, b.kp_count, cap, B, map_select_mode(opts->match_mode), opts->ratio, rp, true, wp,
                       b.fp4, b.norms);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(results, ctx->pb.res, (size_t)B * sizeof(vo_pair_result), hipMemcpyDeviceToHost, s));
    const bool whole_x = X && wp && x_cap == cap;       // caller's layout equals the device layout: one copy
    if (X && wp && x_cap < 1) FAIL(VO_ERR_INVALID, "x_cap must be positive");
    if (whole_x) HIPCHK(hipMemcpyAsync(X, ctx->pb.X, (size_t)B * 4 * cap * sizeof(double), hipMemcpyDeviceToHost, s));
    *whole_x_out = whole_x;
    return done();
}

extern "C" int vo_pairs_run(vo_ctx* ctx, const int32_t* pair_slots, int B, const double* K, const vo_pair_opts* opts,
                            vo_pair_result* results, double* X, int32_t x_cap)
{
    if (!ctx) return VO_ERR_INVALID;
    bool whole_x = false;
    int rc = pairs_enqueue(ctx, pair_slots, B, K, opts, results, X, x_cap, &whole_x);
    if (rc || B == 0) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    const int cap = batch(ctx).kp_cap;
    if (X && opts->want_points && !whole_x) {
        for (int p = 0; p < B; p++) {
            const int n = results[p].status == VO_OK ? (results[p].n_inl < x_cap ? results[p].n_inl : x_cap) : 0;
            if (n <= 0) continue;
            HIPCHK(hipMemcpy2D(X + (size_t)p * 4 * x_cap, (size_t)x_cap * sizeof(double),
                               ctx->pb.X + (size_t)p * 4 * cap, (size_t)cap * sizeof(double),
                               (size_t)n * sizeof(double), 4, hipMemcpyDeviceToHost));
        }
    }
    return capacity_warning(ctx, pair_slots, 2 * B, 0, 0);
}

// Enqueue only: results (and X, which must use x_cap == vo_batch_kp_capacity) have to be page-locked
// (vo_host_alloc) and are valid after the next vo_sync(ctx).  Lets a second ctx's detection overlap this
// ctx's latency-bound RANSAC / pose kernels on the same GPU.
extern "C" int vo_pairs_run_async(vo_ctx* ctx, const int32_t* pair_slots, int B, const double* K, const vo_pair_opts* opts,
                                  vo_pair_result* results, double* X, int32_t x_cap)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (X && opts && opts->want_points && b.ready && x_cap != b.kp_cap)
        FAIL(VO_ERR_INVALID, "vo_pairs_run_async needs x_cap == vo_batch_kp_capacity()");
    bool whole_x = false;
    return pairs_enqueue(ctx, pair_slots, B, K, opts, results, X, x_cap, &whole_x);
}

extern "C" int vo_sync(vo_ctx* ctx)
{
    if (!ctx) return VO_ERR_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_pair_matches(vo_ctx* ctx, int pair, int32_t* qidx, int32_t* tidx, float* dist, uint8_t* inlier_mask,
                               int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (pair < 0 || pair >= ctx->last.pairs || !n_out) FAIL(VO_ERR_INVALID, "bad pair index");
    HIPCHK(hipSetDevice(ctx->device));
    int n = 0;
    HIPCHK(hipStreamSynchronize(ctx->stream));              // an asynchronous batch may still be running
    HIPCHK(hipMemcpy(&n, ctx->pb.m_count + pair, sizeof(int), hipMemcpyDeviceToHost));
    if (n > cap) n = cap;
    *n_out = n;
    const size_t o = (size_t)pair * b.kp_cap;
    if (n > 0) {
        if (qidx) HIPCHK(hipMemcpy(qidx, ctx->pb.m_q + o, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (tidx) HIPCHK(hipMemcpy(tidx, ctx->pb.m_t + o, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (dist) HIPCHK(hipMemcpy(dist, ctx->pb.m_d + o, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        if (inlier_mask) HIPCHK(hipMemcpy(inlier_mask, ctx->pb.mask + o, (size_t)n, hipMemcpyDeviceToHost));
    }
    return VO_OK;
}

// ------------------------------------------------------------------ multi-GPU: trajectory gather over RCCL
extern "C" int vo_comm_unique_id(uint8_t* id)
{
    if (!id) return VO_ERR_INVALID;
    return rccl_unique_id(id) ? VO_ERR_HIP : VO_OK;
}

static void comm_release(vo_ctx* ctx)
{
    CommShared* cs = ctx->cs;
    ctx->cs = nullptr;
    if (!cs || --cs->refs > 0) return;
    if (cs->last) { if (cs->last_set) (void)hipEventSynchronize(cs->last); (void)hipEventDestroy(cs->last); }
    if (cs->comm) rccl_comm_destroy(cs->comm);
    delete cs;
}

extern "C" int vo_comm_init(vo_ctx* ctx, const uint8_t* id, int rank, int world)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!id || world < 1 || rank < 0 || rank >= world) FAIL(VO_ERR_INVALID, "bad communicator arguments");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    comm_release(ctx);
    CommShared* cs = new CommShared();
    if (hipEventCreateWithFlags(&cs->last, hipEventDisableTiming) != hipSuccess) { delete cs; FAIL(VO_ERR_HIP, "no event for the communicator"); }
    const char* e = rccl_comm_init(&cs->comm, id, rank, world);
    if (e) { (void)hipEventDestroy(cs->last); delete cs; FAIL(VO_ERR_HIP, "ncclCommInitRank(rank %d of %d) failed: %s", rank, world, e); }
    cs->rank = rank; cs->world = world; cs->refs = 1;
    ctx->cs = cs;
    return VO_OK;
}

// ctx joins the communicator `owner` created (same process, same device): one communicator per process however many
// contexts alternate over the chunks.
extern "C" int vo_comm_share(vo_ctx* ctx, vo_ctx* owner)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!owner || !owner->cs) FAIL(VO_ERR_INVALID, "the other context has no communicator (vo_comm_init)");
    if (owner->device != ctx->device) FAIL(VO_ERR_INVALID, "contexts of different devices cannot share a communicator");
    if (ctx->cs == owner->cs) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    comm_release(ctx);
    ctx->cs = owner->cs;
    ctx->cs->refs++;
    return VO_OK;
}

extern "C" int vo_comm_destroy(vo_ctx* ctx)
{
    if (!ctx) return VO_ERR_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    comm_release(ctx);
    return VO_OK;
}

// ranks the communicator really holds (ncclCommCount) and this process's rank in it; 1 / 0 without a communicator
extern "C" int vo_comm_info(vo_ctx* ctx, int32_t* n_ranks, int32_t* rank)
{
    if (!ctx) return VO_ERR_INVALID;
    int n = 1, r = 0;
    if (ctx->cs) {
        const char* e = rccl_comm_count(ctx->cs->comm, &n);
        if (e) FAIL(VO_ERR_HIP, "ncclCommCount failed: %s", e);
        r = ctx->cs->rank;
    }
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    return VO_OK;
}

// A collective of this context, on its own stream: it starts after the collective submitted before it (by any context of the
// process) has finished, and leaves its own end behind for the next one.
static int comm_bracket_begin(vo_ctx* ctx)
{
    if (ctx->cs->last_set) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->cs->last, 0));
    return VO_OK;
}

static int comm_bracket_end(vo_ctx* ctx)
{
    HIPCHK(hipEventRecord(ctx->cs->last, ctx->stream));
    ctx->cs->last_set = true;
    return VO_OK;
}

extern "C" int vo_pairs_gather(vo_ctx* ctx, int B, double* gathered, int wait)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (B < 0 || B > b.max_pairs || !gathered) FAIL(VO_ERR_INVALID, "bad gather arguments");
    if (B == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const int world = ctx->cs ? ctx->cs->world : 1;
    const size_t n = (size_t)B * VO_RECORD_DOUBLES, mp = (size_t)b.max_pairs * VO_RECORD_DOUBLES;
    int rc = ctx->rec_send.grow(ctx, n, mp); if (rc) return rc;
    rc = ctx->rec_recv.grow(ctx, n * world, mp * world); if (rc) return rc;
    hipStream_t s = ctx->stream;
    StageTimer t(ctx, ST_GATHER);
    launch_pack_records(s, ctx->pb.res, B, ctx->last.pairs, ctx->rec_send.p);      // pairs past the last run: VO_ERR_NOT_CONFIGURED
    HIPCHK(hipGetLastError());
    const double* src = ctx->rec_send.p;
    if (ctx->cs) {
        rc = comm_bracket_begin(ctx); if (rc) return rc;
        const char* e = rccl_all_gather_f64(ctx->cs->comm, ctx->rec_send.p, ctx->rec_recv.p, n, s);
        if (e) FAIL(VO_ERR_HIP, "ncclAllGather failed: %s", e);
        rc = comm_bracket_end(ctx); if (rc) return rc;
        src = ctx->rec_recv.p;
    }
    HIPCHK(hipMemcpyAsync(gathered, src, n * world * sizeof(double), hipMemcpyDeviceToHost, s));
    if (wait) HIPCHK(hipStreamSynchronize(s));
    return VO_OK;
}

// A small all-gather of host doubles over the context's communicator, synchronous: what a launcher needs for its
// barrier (n = 1) and for the max-over-ranks of a timing, without any other communication library.
extern "C" int vo_comm_allgather_f64(vo_ctx* ctx, const double* send, int n, double* recv)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!send || !recv || n < 1 || n > 4096) FAIL(VO_ERR_INVALID, "bad all-gather arguments");
    HIPCHK(hipSetDevice(ctx->device));
    const int world = ctx->cs ? ctx->cs->world : 1;
    if (!ctx->cs) { memcpy(recv, send, (size_t)n * sizeof(double)); return VO_OK; }
    double *dsend, *drecv;
    ScratchLayout sc;
    sc.take(&dsend, n); sc.take(&drecv, (size_t)n * world);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dsend, send, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    rc = comm_bracket_begin(ctx); if (rc) return rc;
    const char* e = rccl_all_gather_f64(ctx->cs->comm, dsend, drecv, (size_t)n, s);
    if (e) FAIL(VO_ERR_HIP, "ncclAllGather failed: %s", e);
    rc = comm_bracket_end(ctx); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(recv, drecv, (size_t)n * world * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VO_OK;
}

// ------------------------------------------------------------------ single-call matcher / geometry
static int ensure_raw(vo_ctx* ctx, int cap)
{
    if (cap <= ctx->raw_cap) return VO_OK;
    cap = align_up(cap + cap / 4 + 64, 64);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    DevList& m = ctx->raw_mem;
    m.release();
    ctx->raw_cap = 0;
    HIPCHK(m.alloc(&ctx->raw_desc, (size_t)2 * cap * 32));
    HIPCHK(m.alloc(&ctx->raw_desc_x, (size_t)2 * desc_x_rows(cap) * 256));
    HIPCHK(m.alloc(&ctx->raw_xy, (size_t)2 * cap * 2));
    HIPCHK(m.alloc(&ctx->raw_count, 2));
    HIPCHK(hipMemsetAsync(ctx->raw_xy, 0, (size_t)2 * cap * 2 * sizeof(float), ctx->stream));
    HIPCHK(alloc_pairbuf(m, ctx->raw_pb, 1, cap, true));
    ctx->raw_cap = cap;
    return VO_OK;
}

// Query and train descriptors into sets 0 and 1 of the single-call matcher, with their counts {nq, nt} (host memory that
// outlives the upload) and the pair's slots.  Only the matrix cores get the operand image; *fp4 names it.
static int upload_raw_pair(vo_ctx* ctx, const uint8_t* q, const uint8_t* t, const int* counts, int* fp4)
{
    static const int slots[2] = {0, 1};
    int rc = ensure_raw(ctx, counts[0] > counts[1] ? counts[0] : counts[1]); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const int cap = ctx->raw_cap, kernel = nn_kernel(ctx, cap);
    HIPCHK(hipMemcpyAsync(ctx->raw_desc, q, (size_t)counts[0] * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->raw_desc + (size_t)cap * 32, t, (size_t)counts[1] * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->raw_count, counts, 2 * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->raw_pb.slots, slots, sizeof(slots), hipMemcpyHostToDevice, s));
    *fp4 = kernel == NN_FP4;
    if (kernel != NN_POPCOUNT) { StageTimer tm(ctx, ST_BRIEF); launch_desc_expand(s, ctx->raw_desc, ctx->raw_count, cap, desc_x_rows(cap), ctx->raw_desc_x, 2, *fp4); }
    return VO_OK;
}

static int match_raw(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int select_mode, double ratio,
                     int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!n_out || nq < 0 || nt < 0 || (nq > 0 && !q) || (nt > 0 && !t)) FAIL(VO_ERR_INVALID, "bad matcher arguments");
    *n_out = 0;
    if (nq == 0 || nt == 0) return VO_OK;
    if (nq > 65535 || nt > 65535) FAIL(VO_ERR_INVALID, "at most 65535 descriptors per set");
    // the legacy cross-check rule keeps an 8-byte (distance, train) slot per query in LDS: 160 KB per workgroup
    if (select_mode == 1 && (size_t)align_up((nq > nt ? nq : nt) + (nq > nt ? nq : nt) / 4 + 64, 64) * 8 > 160 * 1024)
        FAIL(VO_ERR_INVALID, "cross_check = 1 (legacy rule) supports at most 16000 descriptors per set (LDS), got %d / %d", nq, nt);
    HIPCHK(hipSetDevice(ctx->device));
    const int counts[2] = {nq, nt};
    int fp4 = 0;
    int rc = upload_raw_pair(ctx, q, t, counts, &fp4); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const double Kid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    HIPCHK(hipMemcpyAsync(ctx->dK, Kid, sizeof(Kid), hipMemcpyHostToDevice, s));
    RansacParams rp{};
    rc = run_pairs(ctx, ctx->raw_pb, ctx->raw_desc, ctx->raw_desc_x, ctx->raw_xy, ctx->raw_count, ctx->raw_cap, 1, select_mode, ratio, rp, false, false, fp4);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, ctx->raw_pb.m_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    *n_out = n;
    if (n > 0) {
        HIPCHK(hipMemcpy(qidx, ctx->raw_pb.m_q, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(tidx, ctx->raw_pb.m_t, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist, ctx->raw_pb.m_d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return VO_OK;
}

extern "C" int vo_match_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int cross_check,
                                int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (cross_check < 0 || cross_check > 2) FAIL(VO_ERR_INVALID, "cross_check must be 0, 1 or 2");
    return match_raw(ctx, q, nq, t, nt, cross_check, 0.0, qidx, tidx, dist, n_out);
}

// cv2.BFMatcher(cv2.NORM_L2, crossCheck).match on float rows: the two nearest-neighbour passes run on the device, the
// cross-check rule (a scan over nq + nt integers) and the ordered output on the host
extern "C" int vo_match_l2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int cross_check,
                           int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!n_out || nq < 0 || nt < 0 || dim < 1 || dim > 1024 || (nq > 0 && !q) || (nt > 0 && !t)) FAIL(VO_ERR_INVALID, "bad matcher arguments");
    if (cross_check < 0 || cross_check > 2) FAIL(VO_ERR_INVALID, "cross_check must be 0, 1 or 2");
    *n_out = 0;
    if (nq == 0 || nt == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    float *dq, *dt, *fd, *rd; int *fi, *ri; unsigned long long *fkey, *rkey;
    ScratchLayout sc;
    sc.take(&dq, (size_t)nq * dim); sc.take(&dt, (size_t)nt * dim);
    sc.take(&fi, nq); sc.take(&ri, nt); sc.take(&fd, nq); sc.take(&rd, nt); sc.take(&fkey, nq); sc.take(&rkey, nt);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dq, q, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dt, t, (size_t)nt * dim * sizeof(float), hipMemcpyHostToDevice, s));
    {
        StageTimer tm(ctx, ST_MATCH_NN);
        if (cross_check != 1) launch_nn_l2(s, dq, nq, dt, nt, dim, fi, fd, fkey);
        if (cross_check != 0) launch_nn_l2(s, dt, nt, dq, nq, dim, ri, rd, rkey);
    }
    HIPCHK(hipGetLastError());
    std::vector<int> hfi(nq, -1), hri(nt, -1);
    std::vector<float> hfd(nq, FLT_MAX), hrd(nt, FLT_MAX);
    if (cross_check != 1) {
        HIPCHK(hipMemcpyAsync(hfi.data(), fi, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hfd.data(), fd, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if (cross_check != 0) {
        HIPCHK(hipMemcpyAsync(hri.data(), ri, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hrd.data(), rd, (size_t)nt * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    if (cross_check == 1) {                               // legacy rule: every train row votes for its nearest query
        for (int i = 0; i < nt; i++) { const int k = hri[i]; if (k >= 0 && hrd[i] < hfd[k]) { hfd[k] = hrd[i]; hfi[k] = i; } }
    } else if (cross_check == 2) {                        // OpenCV 4.x: mutual nearest neighbours
        for (int i = 0; i < nq; i++) if (hfi[i] >= 0 && hri[hfi[i]] != i) hfi[i] = -1;
    }
    int n = 0;
    for (int i = 0; i < nq; i++) if (hfi[i] >= 0) { qidx[n] = i; tidx[n] = hfi[i]; dist[n] = hfd[i]; n++; }
    *n_out = n;
    return VO_OK;
}

extern "C" int vo_knn2_ratio_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, double ratio,
                                     int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out)
{
    return match_raw(ctx, q, nq, t, nt, 3, ratio, qidx, tidx, dist, n_out);
}

// matcher.knnMatch(d1, d2, k=2) itself: both neighbours of every query row (src/feature_detection.py:21,90)
extern "C" int vo_knn2_hamming(vo_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx, float* dist)
{
    if (!ctx) return VO_ERR_INVALID;
    if (nq < 0 || nt < 0 || (nq > 0 && (!q || !idx || !dist)) || (nt > 0 && !t)) FAIL(VO_ERR_INVALID, "bad matcher arguments");
    if (nq == 0) return VO_OK;
    if (nt == 0) { for (int i = 0; i < 2 * nq; i++) { idx[i] = -1; dist[i] = FLT_MAX; } return VO_OK; }
    if (nq > 65535 || nt > 65535) FAIL(VO_ERR_INVALID, "at most 65535 descriptors per set");
    HIPCHK(hipSetDevice(ctx->device));
    const int counts[2] = {nq, nt};
    int fp4 = 0;
    int rc = upload_raw_pair(ctx, q, t, counts, &fp4); if (rc) return rc;
    hipStream_t s = ctx->stream;
    { StageTimer tm(ctx, ST_MATCH_NN); launch_hamming_nn(ctx, ctx->raw_pb, ctx->raw_desc, ctx->raw_desc_x, fp4, ctx->raw_count, ctx->raw_cap, 1, 1, 1); }
    HIPCHK(hipGetLastError());
    std::vector<int> i0(nq), d0(nq), i1(nq), d1(nq);
    HIPCHK(hipMemcpyAsync(i0.data(), ctx->raw_pb.nn_idx, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(d0.data(), ctx->raw_pb.nn_dist, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(i1.data(), ctx->raw_pb.nn_idx2, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(d1.data(), ctx->raw_pb.nn_dist2, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    for (int i = 0; i < nq; i++) {
        idx[2 * i] = i0[i]; dist[2 * i] = i0[i] >= 0 ? (float)d0[i] : FLT_MAX;
        const bool two = nt >= 2 && i1[i] >= 0;
        idx[2 * i + 1] = two ? i1[i] : -1; dist[2 * i + 1] = two ? (float)d1[i] : FLT_MAX;
    }
    return VO_OK;
}

// ... on float rows (cv2.BFMatcher(cv2.NORM_L2).knnMatch(q, t, k=2): the script applies its ratio rule to SIFT descriptors)
extern "C" int vo_knn2_l2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int32_t* idx, float* dist)
{
    if (!ctx) return VO_ERR_INVALID;
    if (nq < 0 || nt < 0 || dim < 1 || dim > 1024 || (nq > 0 && (!q || !idx || !dist)) || (nt > 0 && !t)) FAIL(VO_ERR_INVALID, "bad matcher arguments");
    if (nq == 0) return VO_OK;
    if (nt == 0) { for (int i = 0; i < 2 * nq; i++) { idx[i] = -1; dist[i] = FLT_MAX; } return VO_OK; }
    HIPCHK(hipSetDevice(ctx->device));
    float *dq, *dt, *dd; int* di; unsigned long long* part;
    ScratchLayout sc;
    sc.take(&dq, (size_t)nq * dim); sc.take(&dt, (size_t)nt * dim); sc.take(&di, (size_t)2 * nq); sc.take(&dd, (size_t)2 * nq);
    sc.take(&part, nn_l2_knn2_keys(nq, nt));
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dq, q, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dt, t, (size_t)nt * dim * sizeof(float), hipMemcpyHostToDevice, s));
    { StageTimer tm(ctx, ST_MATCH_NN); launch_nn_l2_knn2(s, dq, nq, dt, nt, dim, di, dd, part); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx, di, (size_t)2 * nq * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(dist, dd, (size_t)2 * nq * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// knnMatch(k=2) + `m.distance < ratio * n.distance` on float rows (src/feature_detection.py:20-26 as the script runs it: on SIFT)
extern "C" int vo_knn2_ratio_l2(vo_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, double ratio,
                                int32_t* qidx, int32_t* tidx, float* dist, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!n_out || nq < 0 || (nq > 0 && (!qidx || !tidx || !dist))) FAIL(VO_ERR_INVALID, "bad matcher arguments");
    *n_out = 0;
    if (nq == 0 || nt < 2) return nt < 0 ? VO_ERR_INVALID : VO_OK;      // fewer than two neighbours: the script's `for m, n in` has nothing to unpack
    std::vector<int32_t> i2((size_t)2 * nq); std::vector<float> d2((size_t)2 * nq);
    const int rc = vo_knn2_l2(ctx, q, nq, t, nt, dim, i2.data(), d2.data());
    if (rc) return rc;
    int n = 0;
    for (int i = 0; i < nq; i++)
        if (i2[2 * i] >= 0 && i2[2 * i + 1] >= 0 && (double)d2[2 * i] < ratio * (double)d2[2 * i + 1]) { qidx[n] = i; tidx[n] = i2[2 * i]; dist[n] = d2[2 * i]; n++; }
    *n_out = n;
    return VO_OK;
}

__global__ void k_prepare_points(PairBuf pb, int M, const double* Kd, int fill_mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) pb.m_count[0] = M;
    if (i >= M) return;
    const double ifx = 1. / Kd[0], ify = 1. / Kd[4];
    const double bx = -Kd[2] * ifx, by = -Kd[5] * ify;
    pb.xn1[2 * i] = pb.px1[2 * i] * ifx + bx; pb.xn1[2 * i + 1] = pb.px1[2 * i + 1] * ify + by;
    pb.xn2[2 * i] = pb.px2[2 * i] * ifx + bx; pb.xn2[2 * i + 1] = pb.px2[2 * i + 1] * ify + by;
    if (fill_mask) pb.mask[i] = 1;
}

static int upload_points(vo_ctx* ctx, const double* p1, const double* p2, int M, const double* K, int fill_mask)
{
    int rc = ensure_raw(ctx, M > 8 ? M : 8);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemsetAsync(ctx->raw_pb.res, 0, sizeof(vo_pair_result), s));
    if (M > 0) {
        HIPCHK(hipMemcpyAsync(ctx->raw_pb.px1, p1, (size_t)M * 2 * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->raw_pb.px2, p2, (size_t)M * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(ctx->dK, K, 9 * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_prepare_points, dim3((M + 255) / 256 + 1), dim3(256), 0, s, ctx->raw_pb, M, ctx->dK, fill_mask);
    return VO_OK;
}

extern "C" int vo_find_essential_ransac(vo_ctx* ctx, const double* p1, const double* p2, int M, const double* K,
                                        double prob, double thresh_px, int max_iters, uint64_t seed,
                                        double* E, uint8_t* mask, int32_t* n_inl, int32_t* n_models)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!p1 || !p2 || !K || !E || !mask || !n_inl || !n_models || M < 0) FAIL(VO_ERR_INVALID, "bad arguments");
    *n_inl = 0; *n_models = 0;
    if (M < 5) FAIL(VO_ERR_TOO_FEW, "findEssentialMat needs at least 5 correspondences, got %d", M);
    if (!(prob > 0 && prob < 1)) FAIL(VO_ERR_INVALID, "prob must be in (0, 1)");
    HIPCHK(hipSetDevice(ctx->device));
    int rc = upload_points(ctx, p1, p2, M, K, 0);
    if (rc) return rc;
    RansacParams rp{};
    rp.prob = prob; rp.thresh_px = thresh_px; rp.max_iters = max_iters; rp.seed = seed; rp.dist_thresh = 50; rp.dk_early = ctx->dk_early;
    memcpy(rp.K, K, sizeof(rp.K));
    rc = ensure_rng(ctx, rp.seed);
    if (rc) return rc;
    { StageTimer t(ctx, ST_RANSAC); launch_ransac(ctx->stream, ctx->raw_pb, ctx->raw_cap, 1, rp, ctx->rng_tab, RNG_TAB_N); }
    HIPCHK(hipGetLastError());
    vo_pair_result res;
    HIPCHK(hipMemcpyAsync(&res, ctx->raw_pb.res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(mask, ctx->raw_pb.mask, (size_t)M, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    if (res.status != VO_OK) FAIL(res.status, "essential-matrix RANSAC found no model");
    *n_inl = res.n_inl;
    if (M == 5) {
        const int nm = res.reserved;
        *n_models = nm;
        HIPCHK(hipMemcpy(E, ctx->raw_pb.models, (size_t)nm * 9 * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        *n_models = 1;
        memcpy(E, res.E, sizeof(res.E));
    }
    return VO_OK;
}

extern "C" int vo_recover_pose(vo_ctx* ctx, const double* E, const double* p1, const double* p2, int M, const double* K,
                               double dist_thresh, double* R, double* t, uint8_t* mask, int32_t* n_good)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!E || !K || !R || !t || !n_good || M < 0 || (M > 0 && (!p1 || !p2))) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    int rc = upload_points(ctx, p1, p2, M, K, 1);
    if (rc) return rc;
    vo_pair_result res{};
    memcpy(res.E, E, sizeof(res.E));
    res.status = VO_OK; res.n_match = M; res.reserved = 1;
    HIPCHK(hipMemcpyAsync(ctx->raw_pb.res, &res, sizeof(res), hipMemcpyHostToDevice, ctx->stream));
    RansacParams rp{};
    rp.dist_thresh = dist_thresh; rp.prob = 0.99; rp.thresh_px = 1; rp.max_iters = 1;
    memcpy(rp.K, K, sizeof(rp.K));
    { StageTimer tm(ctx, ST_POSE); launch_pose(ctx->stream, ctx->raw_pb, ctx->raw_cap, 1, rp); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&res, ctx->raw_pb.res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    if (mask && M > 0) HIPCHK(hipMemcpyAsync(mask, ctx->raw_pb.pose_mask, (size_t)M, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    memcpy(R, res.R, sizeof(res.R)); memcpy(t, res.t, sizeof(res.t));
    *n_good = res.n_good;
    return VO_OK;
}

extern "C" int vo_triangulate(vo_ctx* ctx, const double* P1, const double* P2, const double* x1, const double* x2,
                              int M, double* X)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!P1 || !P2 || M < 0 || (M > 0 && (!x1 || !x2 || !X))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (M == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    double *dP1, *dP2, *dx1, *dx2, *dX;
    ScratchLayout sc;
    sc.take(&dP1, 12); sc.take(&dP2, 12); sc.take(&dx1, (size_t)2 * M); sc.take(&dx2, (size_t)2 * M); sc.take(&dX, (size_t)4 * M);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dP1, P1, 12 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dP2, P2, 12 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dx1, x1, (size_t)2 * M * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dx2, x2, (size_t)2 * M * sizeof(double), hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_TRIANGULATE); launch_triangulate_raw(s, dP1, dP2, dx1, dx2, M, dX); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(X, dX, (size_t)4 * M * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_stage_five_point(vo_ctx* ctx, const double* x1, const double* x2, double* E, int32_t* n_models)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!x1 || !x2 || !E || !n_models) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    double *dx1, *dx2, *dE; int* dnm;
    ScratchLayout sc;
    sc.take(&dx1, 10); sc.take(&dx2, 10); sc.take(&dE, 10 * 9); sc.take(&dnm, 1);   // at most 10 models
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dx1, x1, 10 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dx2, x2, 10 * sizeof(double), hipMemcpyHostToDevice, s));
    launch_five_point_raw(s, dx1, dx2, dE, dnm, ctx->dk_early);
    HIPCHK(hipGetLastError());
    int nm = 0;
    HIPCHK(hipMemcpyAsync(&nm, dnm, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_models = nm;
    if (nm > 0) HIPCHK(hipMemcpy(E, dE, (size_t)nm * 9 * sizeof(double), hipMemcpyDeviceToHost));
    return VO_OK;
}

// KeyPointsFilter::retainBest on one response list (the stage the cv2 order mode is built from): order receives the
// kept original indices in cv2's order
extern "C" int vo_stage_retain_best(vo_ctx* ctx, const float* response, int n, int n_points, int32_t* order, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (n < 0 || !n_out || (n > 0 && (!response || !order))) FAIL(VO_ERR_INVALID, "bad arguments");
    *n_out = 0;
    if (n == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    uint2* work; float* dresp; uint32_t *lpos, *rpos; int *dorder, *dn;
    ScratchLayout sc;
    sc.take(&work, n); sc.take(&dresp, n); sc.take(&lpos, n); sc.take(&rpos, n); sc.take(&dorder, n); sc.take(&dn, 1);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dresp, response, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    launch_retain_raw(s, dresp, n, n_points, work, lpos, rpos, dorder, dn);
    HIPCHK(hipGetLastError());
    int m = 0;
    HIPCHK(hipMemcpyAsync(&m, dn, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_out = m;
    if (m > 0) HIPCHK(hipMemcpy(order, dorder, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    return VO_OK;
}

// ------------------------------------------------------------------ "next" row: reprojection-error filter
extern "C" int vo_reprojection_filter(vo_ctx* ctx, const double* poses, int ncam, const double* points, int npt,
                                      const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs,
                                      const double* K, double threshold, double* sqerr, uint8_t* keep)
{
    if (!ctx) return VO_ERR_INVALID;
    if (ncam < 0 || npt < 0 || nobs < 0 || !K || (nobs > 0 && (!poses || !points || !obs_cam || !obs_pt || !obs_xy || !sqerr || !keep)))
        FAIL(VO_ERR_INVALID, "bad arguments");
    if (nobs == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    double *dposes, *dpoints, *dxy, *dK, *derr; int *dcam, *dpt, *dbad; uint8_t* dkeep;
    ScratchLayout sc;
    sc.take(&dposes, (size_t)16 * ncam); sc.take(&dpoints, (size_t)3 * npt); sc.take(&dxy, (size_t)2 * nobs); sc.take(&dK, 9);
    sc.take(&derr, nobs); sc.take(&dcam, nobs); sc.take(&dpt, nobs); sc.take(&dbad, 1); sc.take(&dkeep, nobs);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dposes, poses, (size_t)16 * ncam * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dpoints, points, (size_t)3 * npt * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dxy, obs_xy, (size_t)2 * nobs * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dK, K, 9 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcam, obs_cam, (size_t)nobs * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dpt, obs_pt, (size_t)nobs * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dbad, 0, sizeof(int), s));
    { StageTimer t(ctx, ST_MISC); launch_reprojection(s, dposes, ncam, dpoints, npt, dcam, dpt, dxy, nobs, dK, threshold, derr, dkeep, dbad); }
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(sqerr, derr, (size_t)nobs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(keep, dkeep, (size_t)nobs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    if (bad) FAIL(VO_ERR_INVALID, "an observation refers to a missing camera or point");
    return VO_OK;
}

// ------------------------------------------------------------------ Map.show_map_statistics, src/map.py:234-297
// The host arrays as a SlamMap (counts, [R | t] rows at stride 12) and one launch of the resident maps' k_slam_stats on it.
extern "C" int vo_map_statistics(vo_ctx* ctx, const double* poses, int ncam, const double* points, int npt,
                                 const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs, const double* K, double high_threshold,
                                 double* total_sqerr, double* max_sqerr, int32_t* n_high, int32_t* obs_hist, int32_t* obs_matrix)
{
    if (!ctx) return VO_ERR_INVALID;
    if (ncam < 0 || npt < 0 || nobs < 0 || !K || !total_sqerr || !max_sqerr || !n_high || !obs_hist || (ncam > 0 && (!poses || !obs_matrix)) || (npt > 0 && !points) ||
        (nobs > 0 && (!obs_cam || !obs_pt || !obs_xy))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (ncam > VO_BA_MAX_CAMERAS) FAIL(VO_ERR_UNSUPPORTED, "the observation matrix holds at most %d cameras, got %d", VO_BA_MAX_CAMERAS, ncam);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> rt((size_t)12 * ncam);
    for (int c = 0; c < ncam; c++) memcpy(rt.data() + (size_t)12 * c, poses + (size_t)16 * c, 96);
    const int cnt[4] = {ncam, npt, nobs, 0};
    SlamBuf sb{}; StatsBuf d{}; double* dK;
    ScratchLayout sc;
    sc.take(&sb.m.cnt, 4); sc.take(&sb.m.cam_pose, (size_t)12 * ncam); sc.take(&sb.m.pt_xyz, (size_t)3 * npt);
    sc.take(&sb.m.obs_cam, nobs); sc.take(&sb.m.obs_pt, nobs); sc.take(&sb.m.obs_xy, (size_t)2 * nobs); sc.take(&dK, 9);
    slam_stats_take_scratch(sc, d, true, npt, nobs); slam_stats_take_rows(sc, d, true, 1, ncam);
    int rc = sc.place(ctx); if (rc) return rc;
    d.Kd = dK; d.high = high_threshold; d.cam_frame = nullptr;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(sb.m.cnt, cnt, sizeof(cnt), hipMemcpyHostToDevice, s));
    if (ncam) HIPCHK(hipMemcpyAsync(sb.m.cam_pose, rt.data(), (size_t)96 * ncam, hipMemcpyHostToDevice, s));
    if (npt) HIPCHK(hipMemcpyAsync(sb.m.pt_xyz, points, (size_t)24 * npt, hipMemcpyHostToDevice, s));
    if (nobs) {
        HIPCHK(hipMemcpyAsync(sb.m.obs_cam, obs_cam, (size_t)4 * nobs, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sb.m.obs_pt, obs_pt, (size_t)4 * nobs, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sb.m.obs_xy, obs_xy, (size_t)16 * nobs, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(dK, K, 72, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d.bad, 0, sizeof(int), s));
    { StageTimer t(ctx, ST_SLAM_STATS); launch_slam_stats(s, 0, sb, d); }
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(total_sqerr, d.total_sqerr, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(max_sqerr, d.max_sqerr, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_high, d.n_high, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(obs_hist, d.obs_hist, VO_STATS_HIST * 4, hipMemcpyDeviceToHost, s));
    if (ncam) HIPCHK(hipMemcpyAsync(obs_matrix, d.obs_matrix, (size_t)4 * ncam * ncam, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, d.bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    if (bad) FAIL(VO_ERR_INVALID, "an observation refers to a missing camera or point");
    return VO_OK;
}

// ------------------------------------------------------------------ bundle adjustment: Map.optimize_map, src/map.py:104-186
// The host's part is the bookkeeping g2o's graph does: reject what the kernel cannot hold, sort each problem's observations
// by point (counting sort, stable in input order: a lane owns a point) and list, per block (c1 <= c2) of free cameras, the
// observation pairs that share a point (a wave owns a block of the Schur complement).
extern "C" int vo_bundle_adjust_batch(vo_ctx* ctx, int B, const int32_t* cam_off, const int32_t* pt_off, const int32_t* obs_off,
                                      double* poses, const uint8_t* cam_fixed, double* points, const int32_t* obs_cam,
                                      const int32_t* obs_pt, const double* obs_xy, double focal, double cx, double cy,
                                      const vo_ba_opts* opts, double* chi2, int32_t* iterations_run, int32_t* trials_run,
                                      int32_t* status)
{
    if (!ctx) return VO_ERR_INVALID;
    if (B < 0 || !opts || (B > 0 && (!cam_off || !pt_off || !obs_off || !chi2 || !iterations_run || !trials_run || !status)))
        FAIL(VO_ERR_INVALID, "bad arguments");
    if (opts->iterations < 0 || opts->iterations > 1000) FAIL(VO_ERR_INVALID, "iterations must be 0 .. 1000, got %d", opts->iterations);
    if (!(focal == focal) || !(cx == cx) || !(cy == cy) || !(opts->huber_delta == opts->huber_delta)) FAIL(VO_ERR_INVALID, "camera parameters must be numbers");
    if (B == 0) return VO_OK;
    if (cam_off[0] < 0 || pt_off[0] < 0 || obs_off[0] < 0) FAIL(VO_ERR_INVALID, "offsets must not be negative");
    for (int b = 0; b < B; b++)
        if (cam_off[b + 1] < cam_off[b] || pt_off[b + 1] < pt_off[b] || obs_off[b + 1] < obs_off[b]) FAIL(VO_ERR_INVALID, "offsets must not decrease");
    const int c0 = cam_off[0], p0 = pt_off[0], o0 = obs_off[0];
    const int ncam = cam_off[B] - c0, npt = pt_off[B] - p0, nobs = obs_off[B] - o0;
    if ((ncam > 0 && (!poses || !cam_fixed)) || (npt > 0 && !points) || (nobs > 0 && (!obs_cam || !obs_pt || !obs_xy))) FAIL(VO_ERR_INVALID, "bad arguments");

    std::vector<BaProblem> prob(B);
    std::vector<int> col(ncam, -1), pt_first((size_t)npt + B, 0), s_cam(nobs), s_pt(nobs), blk_first, fill;
    std::vector<double> s_xy((size_t)2 * nobs);
    std::vector<int2> pairs;
    int max_free = 0;
    for (int b = 0; b < B; b++) {
        BaProblem& q = prob[b];
        q.cam0 = cam_off[b] - c0; q.pt0 = pt_off[b] - p0; q.obs0 = obs_off[b] - o0;
        q.ncam = cam_off[b + 1] - cam_off[b]; q.npt = pt_off[b + 1] - pt_off[b]; q.nobs = obs_off[b + 1] - obs_off[b];
        q.pair0 = (int)pairs.size(); q.blk0 = (int)blk_first.size(); q.nfree = 0; q.skip = 0;
        status[b] = VO_OK; chi2[2 * b] = chi2[2 * b + 1] = 0; iterations_run[b] = trials_run[b] = 0;
        const uint8_t* fx = cam_fixed + cam_off[b];
        for (int i = 0; i < q.ncam; i++) if (!fx[i]) q.nfree++;
        const int32_t* oc = obs_cam + obs_off[b]; const int32_t* op = obs_pt + obs_off[b];
        if (q.ncam > VO_BA_MAX_CAMERAS || q.nfree > VO_BA_MAX_FREE) status[b] = VO_ERR_UNSUPPORTED;
        else for (int i = 0; i < q.nobs; i++) if (oc[i] < 0 || oc[i] >= q.ncam || op[i] < 0 || op[i] >= q.npt) { status[b] = VO_ERR_INVALID; break; }
        if (status[b] != VO_OK) { q.skip = 1; q.nfree = 0; continue; }
        int* cl = col.data() + q.cam0;
        for (int i = 0, f = 0; i < q.ncam; i++) if (!fx[i]) cl[i] = f++;
        max_free = std::max(max_free, q.nfree);
        // counting sort by point
        int* first = pt_first.data() + q.pt0 + b;
        for (int i = 0; i < q.nobs; i++) first[op[i] + 1]++;
        for (int p = 0; p < q.npt; p++) first[p + 1] += first[p];
        fill.assign(first, first + q.npt);
        for (int i = 0; i < q.nobs; i++) {
            const int j = q.obs0 + fill[op[i]]++;
            s_cam[j] = oc[i]; s_pt[j] = op[i];
            s_xy[2 * (size_t)j] = obs_xy[2 * ((size_t)obs_off[b] + i)]; s_xy[2 * (size_t)j + 1] = obs_xy[2 * ((size_t)obs_off[b] + i) + 1];
        }
        // pair lists per block, blocks in the order (0,0) (0,1) .. (0,F-1) (1,1) ..; within a block by point, then input order
        const int F = q.nfree, nblk = F * (F + 1) / 2;
        auto blk = [F](int a, int c) { return a * F - a * (a - 1) / 2 + (c - a); };
        std::vector<size_t> cnt((size_t)nblk + 1, 0);
        const int* sc = s_cam.data() + q.obs0;
        for (int pass = 0; pass < 2; pass++) {
            for (int p = 0; p < q.npt; p++)
                for (int j1 = first[p]; j1 < first[p + 1]; j1++) {
                    const int a = cl[sc[j1]]; if (a < 0) continue;
                    for (int j2 = first[p]; j2 < first[p + 1]; j2++) {
                        const int c = cl[sc[j2]]; if (c < a) continue;
                        if (pass == 0) cnt[blk(a, c) + 1]++;
                        else pairs[(size_t)q.pair0 + cnt[blk(a, c)]++] = make_int2(j1, j2);
                    }
                }
            if (pass == 0) {
                for (int k = 0; k < nblk; k++) cnt[k + 1] += cnt[k];
                if ((size_t)q.pair0 + cnt[nblk] > (size_t)INT32_MAX) FAIL(VO_ERR_INVALID, "problem %d: too many observation pairs", b);
                for (int k = 0; k <= nblk; k++) blk_first.push_back((int)cnt[k]);
                pairs.resize((size_t)q.pair0 + cnt[nblk]);
            }
        }
    }

    HIPCHK(hipSetDevice(ctx->device));
    BaBuf D{};
    BaProblem* dprob; int *dcol, *dptf, *dcam, *dpt, *dblk; double* dxy; int2* dpairs;
    ScratchLayout sc;
    sc.take(&dprob, B); sc.take(&D.poses, (size_t)12 * ncam); sc.take(&dcol, ncam); sc.take(&D.X, (size_t)3 * npt); sc.take(&D.X2, (size_t)3 * npt);
    sc.take(&dptf, pt_first.size()); sc.take(&dcam, nobs); sc.take(&dpt, nobs); sc.take(&dxy, (size_t)2 * nobs); sc.take(&D.W, (size_t)18 * nobs);
    sc.take(&D.Hpp, (size_t)6 * npt); sc.take(&D.bp, (size_t)3 * npt); sc.take(&D.Hpi, (size_t)6 * npt); sc.take(&dpairs, pairs.size());
    sc.take(&dblk, blk_first.size()); sc.take(&D.chi2, (size_t)2 * B); sc.take(&D.iterations_run, B); sc.take(&D.trials_run, B);
    int rc = sc.place(ctx); if (rc) return rc;
    D.prob = dprob; D.cam_col = dcol; D.pt_first = dptf; D.obs_cam = dcam; D.obs_pt = dpt; D.obs_xy = dxy; D.pairs = dpairs; D.blk_first = dblk;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dprob, prob.data(), (size_t)B * sizeof(BaProblem), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dptf, pt_first.data(), pt_first.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (ncam > 0) {
        HIPCHK(hipMemcpyAsync(D.poses, poses + (size_t)12 * c0, (size_t)12 * ncam * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dcol, col.data(), (size_t)ncam * sizeof(int), hipMemcpyHostToDevice, s));
    }
    if (npt > 0) HIPCHK(hipMemcpyAsync(D.X, points + (size_t)3 * p0, (size_t)3 * npt * sizeof(double), hipMemcpyHostToDevice, s));
    if (nobs > 0) {
        HIPCHK(hipMemcpyAsync(dcam, s_cam.data(), (size_t)nobs * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dpt, s_pt.data(), (size_t)nobs * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dxy, s_xy.data(), (size_t)2 * nobs * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (!pairs.empty()) HIPCHK(hipMemcpyAsync(dpairs, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    if (!blk_first.empty()) HIPCHK(hipMemcpyAsync(dblk, blk_first.data(), blk_first.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(D.chi2, 0, (size_t)2 * B * sizeof(double), s));
    HIPCHK(hipMemsetAsync(D.iterations_run, 0, (size_t)B * sizeof(int), s));
    HIPCHK(hipMemsetAsync(D.trials_run, 0, (size_t)B * sizeof(int), s));
    HIPCHK(hipStreamSynchronize(s));                                 // the staging vectors live on this stack
    const BaParams prm{focal, cx, cy, opts->huber_delta, opts->iterations};
    { StageTimer t(ctx, ST_MISC); launch_bundle_adjust(s, D, prm, B, max_free); }
    HIPCHK(hipGetLastError());
    if (ncam > 0) HIPCHK(hipMemcpyAsync(poses + (size_t)12 * c0, D.poses, (size_t)12 * ncam * sizeof(double), hipMemcpyDeviceToHost, s));
    if (npt > 0) HIPCHK(hipMemcpyAsync(points + (size_t)3 * p0, D.X, (size_t)3 * npt * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(chi2, D.chi2, (size_t)2 * B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(iterations_run, D.iterations_run, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(trials_run, D.trials_run, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_bundle_adjust(vo_ctx* ctx, double* poses, const uint8_t* cam_fixed, int ncam, double* points, int npt,
                                const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs,
                                double focal, double cx, double cy, const vo_ba_opts* opts, double* chi2,
                                int32_t* iterations_run, int32_t* trials_run)
{
    if (!ctx) return VO_ERR_INVALID;
    if (ncam < 0 || npt < 0 || nobs < 0 || !chi2 || !iterations_run || !trials_run) FAIL(VO_ERR_INVALID, "bad arguments");
    const int32_t co[2] = {0, ncam}, po[2] = {0, npt}, oo[2] = {0, nobs};
    int32_t status = 0;
    int rc = vo_bundle_adjust_batch(ctx, 1, co, po, oo, poses, cam_fixed, points, obs_cam, obs_pt, obs_xy, focal, cx, cy, opts,
                                    chi2, iterations_run, trials_run, &status);
    if (rc) return rc;
    if (status == VO_ERR_UNSUPPORTED)
        FAIL(VO_ERR_UNSUPPORTED, "bundle adjustment holds at most %d cameras, %d of them free, per problem", VO_BA_MAX_CAMERAS, VO_BA_MAX_FREE);
    if (status == VO_ERR_INVALID) FAIL(VO_ERR_INVALID, "an observation refers to a missing camera or point");
    return VO_OK;
}

// ------------------------------------------------------------------ "next" row: PnP-RANSAC localisation
extern "C" int vo_solve_pnp_ransac_batch(vo_ctx* ctx, const double* obj, const double* img, const int32_t* offsets, int B,
                                         const double* K, int iterations, double reproj_err, double confidence, uint64_t seed,
                                         double* rvec, double* tvec, uint8_t* mask, int32_t* n_inl, int32_t* status)
{
    if (!ctx) return VO_ERR_INVALID;
    if (B < 0 || !offsets || !K || (B > 0 && (!rvec || !tvec || !n_inl || !status))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (B == 0) return VO_OK;
    for (int b = 0; b < B; b++) if (offsets[b + 1] < offsets[b]) FAIL(VO_ERR_INVALID, "offsets must not decrease");
    const int total = offsets[B] - offsets[0];
    if (total > 0 && (!obj || !img || !mask)) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    int rc = ensure_rng(ctx, seed); if (rc) return rc;
    double *dobj, *dimg, *dK, *drv, *dtv; int *doff, *dninl, *dst; uint8_t* dmask;
    ScratchLayout sc;
    sc.take(&dobj, (size_t)3 * total); sc.take(&dimg, (size_t)2 * total); sc.take(&dK, 9); sc.take(&drv, (size_t)3 * B); sc.take(&dtv, (size_t)3 * B);
    sc.take(&doff, (size_t)B + 1); sc.take(&dninl, B); sc.take(&dst, B); sc.take(&dmask, total);
    rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    std::vector<int> off(B + 1);
    for (int b = 0; b <= B; b++) off[b] = offsets[b] - offsets[0];
    if (total > 0) {
        HIPCHK(hipMemcpyAsync(dobj, obj + (size_t)3 * offsets[0], (size_t)3 * total * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dimg, img + (size_t)2 * offsets[0], (size_t)2 * total * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(dK, K, 9 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(doff, off.data(), (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                                 // `off` is a stack vector
    { StageTimer t(ctx, ST_MISC); launch_pnp_ransac(s, dobj, dimg, doff, B, dK, iterations, reproj_err, confidence, seed, ctx->rng_tab, RNG_TAB_N,
                                                   ctx->pnp_refine, drv, dtv, dmask, dninl, dst); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rvec, drv, (size_t)3 * B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(tvec, dtv, (size_t)3 * B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, dninl, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, dst, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (total > 0) HIPCHK(hipMemcpyAsync(mask + offsets[0], dmask, (size_t)total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_solve_pnp_ransac(vo_ctx* ctx, const double* obj, const double* img, int n, const double* K, int iterations,
                                   double reproj_err, double confidence, uint64_t seed, double* rvec, double* tvec,
                                   uint8_t* mask, int32_t* n_inl)
{
    if (!ctx) return VO_ERR_INVALID;
    if (n < 0 || !rvec || !tvec || !n_inl || (n > 0 && (!obj || !img || !mask))) FAIL(VO_ERR_INVALID, "bad arguments");
    const int32_t offsets[2] = {0, n};
    int32_t status = 0;
    uint8_t dummy = 0;
    *n_inl = 0;
    int rc = vo_solve_pnp_ransac_batch(ctx, obj, img, offsets, 1, K, iterations, reproj_err, confidence, seed, rvec, tvec,
                                       n > 0 ? mask : &dummy, n_inl, &status);
    if (rc) return rc;
    if (status == VO_ERR_TOO_FEW) FAIL(VO_ERR_TOO_FEW, "solvePnPRansac needs at least 4 correspondences, got %d", n);
    if (status == VO_ERR_NO_MODEL) FAIL(VO_ERR_NO_MODEL, "no pose with more than 4 inliers");
    if (status < 0) FAIL(status, "solvePnPRansac failed");
    return VO_OK;
}

extern "C" int vo_rodrigues(vo_ctx* ctx, const double* in, int in_is_matrix, double* out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!in || !out) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    double *din, *dout;
    ScratchLayout sc;
    sc.take(&din, 9); sc.take(&dout, 9);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(din, in, (in_is_matrix ? 9 : 3) * sizeof(double), hipMemcpyHostToDevice, s));
    launch_rodrigues(s, din, in_is_matrix, dout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, (in_is_matrix ? 3 : 9) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VO_OK;
}

// ------------------------------------------------------------------ "next" row: frame ingest (cv2.resize INTER_LINEAR)
// resize.cpp resize(): fx = (float)((dx + 0.5) * scale_x - 0.5), scale_x = 1. / ((double)dw / sw); columns force
// (offset, weight) at the borders, rows keep the weight and clamp the row index; coefficients are
// saturate_cast<short>(cvRound(w * 2048)).
static void linear_tab(int ssize, int dsize, bool clamp_weight, int* ofs, short* c /*pairs*/)
{
    const double scale = 1. / ((double)dsize / ssize);
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= s;
        if (clamp_weight) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        }
        ofs[d] = s;
        const long r0 = lrintf((1.f - f) * 2048.f), r1 = lrintf(f * 2048.f);
        c[2 * d] = (short)(r0 > 32767 ? 32767 : r0); c[2 * d + 1] = (short)(r1 > 32767 ? 32767 : r1);
    }
}

// device tables for (sw, sh) -> (dw, dh): [xofs dw][xa dw pairs][yofs dh][yb dh pairs] as ints
static int ingest_tables(vo_ctx* ctx, int sw, int sh, int dw, int dh, const int** xofs, const void** xa, const int** yofs, const void** yb)
{
    const size_t n = (size_t)2 * (dw + dh);
    int rc = ctx->ingest_tab.grow(ctx, n); if (rc) return rc;
    int* d = ctx->ingest_tab.p;
    std::vector<int> host(n);
    linear_tab(sw, dw, true, host.data(), (short*)(host.data() + dw));
    linear_tab(sh, dh, false, host.data() + 2 * dw, (short*)(host.data() + 2 * dw + dh));
    HIPCHK(hipMemcpyAsync(d, host.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                       // `host` is a stack vector
    *xofs = d; *xa = d + dw; *yofs = d + 2 * dw; *yb = d + 2 * dw + dh;
    return VO_OK;
}

// The resized image (ctx->ingest_out, rows at dst_stride) back to the caller's dst, enqueued: a dense destination is one linear copy;
// otherwise a 2-D copy of the rows' row_bytes, so that the bytes between the caller's rows and after its last row are never written.
static int resized_to_host(vo_ctx* ctx, uint8_t* dst, int dh, int row_bytes, int dst_stride)
{
    if (dst_stride == row_bytes) HIPCHK(hipMemcpyAsync(dst, ctx->ingest_out.p, (size_t)dst_stride * dh, hipMemcpyDeviceToHost, ctx->stream));
    else HIPCHK(hipMemcpy2DAsync(dst, (size_t)dst_stride, ctx->ingest_out.p, (size_t)dst_stride, (size_t)row_bytes, (size_t)dh, hipMemcpyDeviceToHost, ctx->stream));
    return VO_OK;
}

extern "C" int vo_resize_linear(vo_ctx* ctx, const uint8_t* src, int sh, int sw, int channels, int row_stride,
                                uint8_t* dst, int dh, int dw, int dst_stride)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!src || !dst || sh < 1 || sw < 1 || dh < 1 || dw < 1 || (channels != 1 && channels != 3 && channels != 4) ||
        row_stride < sw * channels || dst_stride < dw * channels) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t sbytes = image_span(1, 0, sh, row_stride, sw * channels), dbytes = (size_t)dst_stride * dh;
    int rc = ctx->staging.grow(ctx, sbytes); if (rc) return rc;
    rc = ctx->ingest_out.grow(ctx, dbytes); if (rc) return rc;
    const int* xofs; const void* xa; const int* yofs; const void* yb;
    rc = ingest_tables(ctx, sw, sh, dw, dh, &xofs, &xa, &yofs, &yb); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->staging.p, src, sbytes, hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MISC); launch_resize_linear(s, ctx->staging.p, sw, sh, channels, row_stride, 0, ctx->ingest_out.p, dw, dh, dst_stride, 0,
                                                       xofs, xa, yofs, yb, sw == 2 * dw && sh == 2 * dh, 1); }
    HIPCHK(hipGetLastError());
    rc = resized_to_host(ctx, dst, dh, dw * channels, dst_stride); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// resize.cpp computeResizeAreaTab: for every destination index the source cells it covers and their weights
static int area_tab(int ssize, int dsize, double scale, std::vector<int>& si, std::vector<float>& al, std::vector<int>& start)
{
    si.clear(); al.clear(); start.assign((size_t)dsize + 1, 0);
    for (int dx = 0; dx < dsize; dx++) {
        start[dx] = (int)si.size();
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = scale < ssize - fsx1 ? scale : ssize - fsx1;
        int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
        sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
        sx1 = sx1 < sx2 ? sx1 : sx2;
        if (sx1 - fsx1 > 1e-3) { si.push_back(sx1 - 1); al.push_back((float)((sx1 - fsx1) / cell)); }
        for (int sx = sx1; sx < sx2; sx++) { si.push_back(sx); al.push_back((float)(1.0 / cell)); }
        if (fsx2 - sx2 > 1e-3) {
            double a = fsx2 - sx2; a = a < 1. ? a : 1.; a = a < cell ? a : cell;
            si.push_back(sx2); al.push_back((float)(a / cell));
        }
    }
    start[dsize] = (int)si.size();
    return (int)si.size();
}

extern "C" int vo_resize_area(vo_ctx* ctx, const uint8_t* src, int sh, int sw, int channels, int row_stride,
                              uint8_t* dst, int dh, int dw, int dst_stride)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!src || !dst || sh < 1 || sw < 1 || dh < 1 || dw < 1 || (channels != 1 && channels != 3 && channels != 4) ||
        row_stride < sw * channels || dst_stride < dw * channels) FAIL(VO_ERR_INVALID, "bad arguments");
    if (dw > sw || dh > sh) FAIL(VO_ERR_UNSUPPORTED, "INTER_AREA enlargement (a bilinear variant in OpenCV) is not built");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t sbytes = image_span(1, 0, sh, row_stride, sw * channels), dbytes = (size_t)dst_stride * dh;
    int rc = ctx->staging.grow(ctx, sbytes); if (rc) return rc;
    rc = ctx->ingest_out.grow(ctx, dbytes); if (rc) return rc;
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);     // as resize() forms them
    const int isx = (int)lrint(scale_x), isy = (int)lrint(scale_y);
    const bool fast = fabs(scale_x - isx) < DBL_EPSILON && fabs(scale_y - isy) < DBL_EPSILON;
    hipStream_t s = ctx->stream;
    const int *xsi = nullptr, *xst = nullptr, *ysi = nullptr, *yst = nullptr; const float *xal = nullptr, *yal = nullptr;
    std::vector<int> hxs, hys, hxst, hyst; std::vector<float> hxa, hya;
    if (!fast) {
        const int nx = area_tab(sw, dw, scale_x, hxs, hxa, hxst), ny = area_tab(sh, dh, scale_y, hys, hya, hyst);
        int *dxs, *dxst, *dys, *dyst; float *dxa, *dya;
        ScratchLayout sc;
        sc.take(&dxs, nx); sc.take(&dxa, nx); sc.take(&dxst, (size_t)dw + 1); sc.take(&dys, ny); sc.take(&dya, ny); sc.take(&dyst, (size_t)dh + 1);
        rc = sc.place(ctx); if (rc) return rc;
        HIPCHK(hipMemcpyAsync(dxs, hxs.data(), (size_t)nx * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dxa, hxa.data(), (size_t)nx * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dxst, hxst.data(), (size_t)(dw + 1) * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dys, hys.data(), (size_t)ny * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dya, hya.data(), (size_t)ny * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dyst, hyst.data(), (size_t)(dh + 1) * 4, hipMemcpyHostToDevice, s));
        xsi = dxs; xal = dxa; xst = dxst; ysi = dys; yal = dya; yst = dyst;
    }
    HIPCHK(hipMemcpyAsync(ctx->staging.p, src, sbytes, hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MISC); launch_resize_area(s, ctx->staging.p, channels, row_stride, ctx->ingest_out.p, dw, dh, dst_stride,
                                                     fast ? isx : 0, fast ? isy : 0, xsi, xal, xst, ysi, yal, yst); }
    HIPCHK(hipGetLastError());
    rc = resized_to_host(ctx, dst, dh, dw * channels, dst_stride); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));                                 // also keeps the host tables alive until copied
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// n full-resolution frames already on the device -> cv2.resize to the configured (w, h) -> gray -> level 0 of the slots
static int ingest_from_device(vo_ctx* ctx, const uint8_t* src, int n, int sh, int sw, int channels, int row_stride, int64_t frame_stride,
                              int first_slot, uint8_t* resized_out)
{
    const Batch b = batch(ctx);
    const int dw = b.w, dh = b.h;
    const size_t dper = (size_t)dw * dh * channels;
    hipStream_t s = ctx->stream;
    if (sw == dw && sh == dh && (!resized_out || (row_stride == dw * channels && frame_stride == (int64_t)dper))) {
        // cv::resize to the source's own size is a copy: gray straight from the source frames
        { StageTimer t(ctx, ST_GRAY); gray_into_slots(ctx, s, src, channels, row_stride, frame_stride, first_slot, n); }
        if (resized_out) HIPCHK(hipMemcpyAsync(resized_out, src, dper * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
        return VO_OK;
    }
    int rc = ctx->ingest_out.grow(ctx, dper * n); if (rc) return rc;
    const int* xofs; const void* xa; const int* yofs; const void* yb;
    rc = ingest_tables(ctx, sw, sh, dw, dh, &xofs, &xa, &yofs, &yb); if (rc) return rc;
    {
        StageTimer t(ctx, ST_MISC);
        if (channels == 1 && !resized_out)                   // gray input: straight into the slots' gray frames
            launch_resize_linear(s, src, sw, sh, 1, row_stride, frame_stride, b.gray_slot(first_slot), dw, dh, b.gray_stride, (int64_t)b.gray_frame,
                                 xofs, xa, yofs, yb, sw == 2 * dw && sh == 2 * dh, n);
        else
            launch_resize_linear(s, src, sw, sh, channels, row_stride, frame_stride, ctx->ingest_out.p, dw, dh, dw * channels,
                                 (int64_t)dper, xofs, xa, yofs, yb, sw == 2 * dw && sh == 2 * dh, n);
    }
    if (!(channels == 1 && !resized_out)) {
        StageTimer t(ctx, ST_GRAY);
        gray_into_slots(ctx, s, ctx->ingest_out.p, channels, dw * channels, (int64_t)dper, first_slot, n);
        if (resized_out) HIPCHK(hipMemcpyAsync(resized_out, ctx->ingest_out.p, dper * n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return VO_OK;
}

// Full-resolution frames (host) -> resized to the configured (w, h) on the device -> gray -> level 0 of the slots.
// `resized_out` (optional, host, [F][h][w][channels] dense) receives the resized frames, which the reference
// keeps as Frame.image.
extern "C" int vo_frames_ingest(vo_ctx* ctx, const uint8_t* frames, int F, int sh, int sw, int channels, int row_stride,
                                int64_t frame_stride, int first_slot, uint8_t* resized_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (!frames || F < 0 || first_slot < 0 || first_slot + F > b.max_frames) FAIL(VO_ERR_INVALID, "slot range out of bounds");
    slam_stream_slots_written(ctx, first_slot, F);
    if (sh < 1 || sw < 1 || (channels != 1 && channels != 3 && channels != 4) || row_stride < sw * channels ||
        frame_stride < (int64_t)image_span(1, 0, sh, row_stride, sw * channels)) FAIL(VO_ERR_INVALID, "bad source geometry");
    if (F == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t per = (size_t)frame_stride, dper = (size_t)b.w * b.h * channels;
    size_t chunk = (size_t)512 * 1024 * 1024 / per; if (chunk < 1) chunk = 1; if (chunk > (size_t)F) chunk = F;
    int rc = ctx->staging.grow(ctx, per * chunk); if (rc) return rc;
    hipStream_t s = ctx->stream;
    for (int f0 = 0; f0 < F; f0 += (int)chunk) {
        const int n = F - f0 < (int)chunk ? F - f0 : (int)chunk;
        HIPCHK(hipMemcpyAsync(ctx->staging.p, frames + (size_t)f0 * per, image_span(n, frame_stride, sh, row_stride, sw * channels), hipMemcpyHostToDevice, s));
        rc = ingest_from_device(ctx, ctx->staging.p, n, sh, sw, channels, row_stride, (int64_t)per, first_slot + f0,
                                resized_out ? resized_out + (size_t)f0 * dper : nullptr);
        if (rc) return rc;
    }
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}


// ------------------------------------------------------------------ SIFT, the reference's live detector (visual_slam.py:17), frame-batched
// getGaussianKernel(n, sigma, CV_32F) with n = cvRound(sigma * 8 + 1) | 1
static int sift_gauss_taps(double sigma, float* k)
{
    const int n = (int)lrint(sigma * 4 * 2 + 1) | 1;
    if (n > SIFT_MAX_TAPS) return -1;
    double t[SIFT_MAX_TAPS], sum = 0;
    const double s2 = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; t[i] = exp(s2 * x * x); sum += t[i]; }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) k[i] = (float)(t[i] * sum);
    return n;
}

// Buffers of one SIFT configuration: the per-slot results (keypoints, descriptors, matcher operands) for max_frames slots and
// the scale-space scratch of one sub-batch of `fb` frames.
static int sift_setup(vo_ctx* ctx, SiftState& S, int h, int w, const vo_sift_params* p, int max_frames, int kp_cap, int raw_cap, int cand_cap,
                      int surv_cap, int fb, bool with_operands)
{
    if (p->n_octave_layers < 1 || p->n_octave_layers > 8 || !(p->sigma > 0.5) || p->nfeatures < 0)
        FAIL(VO_ERR_UNSUPPORTED, "SIFT: nOctaveLayers 1..8, sigma > 0.5 and nfeatures >= 0 are built");
    if (S.configured && S.h == h && S.w == w && memcmp(&S.prm, p, sizeof(*p)) == 0 && S.max_frames >= max_frames && S.kp_cap == kp_cap &&
        S.raw_cap == raw_cap && S.cand_cap == cand_cap && S.surv_cap == surv_cap && S.fb >= fb && S.with_operands == with_operands)
        return VO_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    S = SiftState();                                           // frees the previous configuration's buffers
    S.h = h; S.w = w; S.prm = *p; S.max_frames = max_frames; S.kp_cap = kp_cap; S.raw_cap = raw_cap; S.cand_cap = cand_cap; S.surv_cap = surv_cap;
    S.fb = fb; S.with_operands = with_operands; S.cap_x = desc_x_rows(kp_cap);
    S.fstride = w;                                             // dense rows: a batch of frames is one transfer (the first sweep's loader reads bytes)
    const int L = p->n_octave_layers;
    SiftGeom& P = S.P; memset(&P, 0, sizeof(P));
    P.nLayers = L;
    int nOct = (int)lrint(log((double)(2 * (w < h ? w : h))) / log(2.) - 2) + 1;
    if (nOct < 1) nOct = 1;
    if (nOct > SIFT_MAX_OCT) nOct = SIFT_MAX_OCT;
    size_t gtot = 0;
    for (int o = 0; o < nOct; o++) {
        P.w[o] = o ? P.w[o - 1] / 2 : 2 * w; P.h[o] = o ? P.h[o - 1] / 2 : 2 * h;
        if (P.w[o] < 1 || P.h[o] < 1) { nOct = o; break; }
        P.stride[o] = align_up(P.w[o], 16);
        P.plane[o] = (size_t)P.stride[o] * P.h[o];
        P.goff[o] = gtot;
        gtot += (size_t)(L + 3) * P.plane[o];
    }
    P.nOct = nOct; P.gframe = gtot;
    // Gaussian taps of the base image (createInitialImage) and of the incremental blurs (buildGaussianPyramid)
    {
        const double k = pow(2., 1. / L);
        const float sd = sqrtf(fmaxf((float)(p->sigma * p->sigma - 0.5 * 0.5 * 4), 0.01f));
        S.ntaps[0] = sift_gauss_taps((double)sd, S.taps[0]);
        for (int i = 1; i < L + 3; i++) {
            const double sp = pow(k, (double)(i - 1)) * p->sigma, st = sp * k;
            S.ntaps[i] = sift_gauss_taps(sqrt(st * st - sp * sp), S.taps[i]);
        }
        for (int i = 0; i < L + 3; i++) if (S.ntaps[i] < 0 || S.ntaps[i] > 63) FAIL(VO_ERR_UNSUPPORTED, "SIFT: blur kernel wider than 63 taps");
    }
    for (int i = 0; i < 64; i++) S.E.tab[i] = (float)pow(2.0, i / 64.0);
    const size_t F = (size_t)max_frames, B = (size_t)fb;
    DevList& m = S.mem;
    HIPCHK(m.alloc(&S.frames, F * S.fstride * h + 64));
    HIPCHK(m.alloc(&S.kp_xy, F * kp_cap * 2)); HIPCHK(m.alloc(&S.kp_size, F * kp_cap)); HIPCHK(m.alloc(&S.kp_angle, F * kp_cap));
    HIPCHK(m.alloc(&S.kp_resp, F * kp_cap)); HIPCHK(m.alloc(&S.kp_oct, F * kp_cap));
    HIPCHK(m.alloc(&S.kp_count, F)); HIPCHK(m.alloc(&S.flags, F));
    HIPCHK(hipMemset(S.kp_count, 0, F * sizeof(int))); HIPCHK(hipMemset(S.flags, 0, F * sizeof(int)));
    HIPCHK(m.alloc(&S.desc, F * kp_cap * 128));
    if (with_operands) {
        HIPCHK(m.alloc(&S.desc_x, F * (size_t)S.cap_x * 128)); HIPCHK(m.alloc(&S.norms, F * (size_t)S.cap_x));
        HIPCHK(hipMemset(S.desc_x, 0, F * (size_t)S.cap_x * 128)); HIPCHK(hipMemset(S.norms, 0, F * (size_t)S.cap_x * sizeof(int)));
    }
    HIPCHK(m.alloc(&S.G, B * gtot));                                       // (the up-sampled base image is never stored: S.up stays null)
    HIPCHK(m.alloc(&S.cand, B * cand_cap)); HIPCHK(m.alloc(&S.surv, B * surv_cap));
    HIPCHK(m.alloc(&S.kraw, B * raw_cap)); HIPCHK(m.alloc(&S.ksorted, B * raw_cap)); HIPCHK(m.alloc(&S.kfin, B * kp_cap));
    HIPCHK(m.alloc(&S.rank, B * 4097)); HIPCHK(m.alloc(&S.counts, B * 4)); HIPCHK(m.alloc(&S.fin_count, B)); HIPCHK(m.alloc(&S.fin_flags, B));
    HIPCHK(hipDeviceSynchronize());
    S.configured = true;
    return VO_OK;
}

// Scale space, extrema, refinement, orientation, sort + duplicate removal of the frames src[0..F) (F <= S.fb): everything up to the
// final keypoint list S.kfin / S.counts[.][3], enqueued on the context's stream, no host round trip.
static int sift_detect_enqueue(vo_ctx* ctx, SiftState& S, const uint8_t* src, int channels, int row_stride, int64_t frame_stride, int F)
{
    hipStream_t s = ctx->stream;
    const SiftGeom& P = S.P;
    const int L = P.nLayers;
    HIPCHK(hipMemsetAsync(S.counts, 0, (size_t)F * 4 * sizeof(int), s));
    {
        StageTimer t(ctx, ST_SIFT_SCALE);
        // G[0] of octave 0 = blur(2 x up-sampled input): the up-sampling happens in the sweep's loader
        if (launch_sb_sweep_base(s, src, channels, row_stride, frame_stride, S.w, S.h, S.G + P.goff[0], P.gframe, P.stride[0], F, S.taps[0], S.ntaps[0]))
            FAIL(VO_ERR_UNSUPPORTED, "SIFT: unsupported blur size");
    }
    const float threshold = (float)(int)floor(0.5 * S.prm.contrast_threshold / L * 255);
    for (int o = 0; o < P.nOct; o++) {
        {
            StageTimer t(ctx, ST_SIFT_SCALE);
            float* g0 = S.G + P.goff[o];
            for (int i = 1; i < L + 3; i++) {
                // G[i] = blur(G[i-1]); the sweep that makes layer L also writes it at half size: the first image of the next
                // octave (cv::resize INTER_NEAREST)
                const bool seed = i == L && o + 1 < P.nOct;
                launch_sb_sweep(s, g0 + (size_t)(i - 1) * P.plane[o], P.gframe, g0 + (size_t)i * P.plane[o], P.gframe,
                                P.w[o], P.h[o], P.stride[o], F, S.taps[i], S.ntaps[i],
                                seed ? S.G + P.goff[o + 1] : nullptr, P.gframe, seed ? P.stride[o + 1] : 0, seed ? P.w[o + 1] : 0, seed ? P.h[o + 1] : 0);
            }
        }
        { StageTimer t(ctx, ST_SIFT_EXTREMA); launch_sb_extrema(s, P, S.G, o, threshold, S.cand, S.counts, S.cand_cap, F); }
    }
    const int waves = 2048 / (F < 8 ? F : 8) > 64 ? 2048 / (F < 8 ? F : 8) : 64;        // persistent wavefronts per frame for the wave-per-item kernels
    {
        StageTimer t(ctx, ST_SIFT_ORIENT);
        launch_sb_refine_orient(s, P, S.G, S.cand, S.cand_cap, (float)S.prm.contrast_threshold, (float)S.prm.edge_threshold, (float)S.prm.sigma, S.E,
                                S.surv, S.surv_cap, S.kraw, S.raw_cap, S.counts, F, waves);
    }
    {
        StageTimer t(ctx, ST_SIFT_SORT);
        // (the survivor list is dead once the orientations are assigned: its memory holds the bucket-ordered copy of the records)
        launch_sb_sort_emit(s, S.kraw, S.raw_cap, S.counts, S.rank, S.surv, S.ksorted, S.kfin, S.kp_cap, S.fin_count, S.fin_flags, S.cand_cap, S.surv_cap, F);
    }
    HIPCHK(hipGetLastError());
    return VO_OK;
}

// descriptors of the final keypoints of the sub-batch into slots first_slot.. + the SoA arrays the pair stage reads
static int sift_describe_enqueue(vo_ctx* ctx, SiftState& S, int first_slot, int F)
{
    hipStream_t s = ctx->stream;
    const int waves = 2048 / (F < 8 ? F : 8) > 64 ? 2048 / (F < 8 ? F : 8) : 64;
    {
        StageTimer t(ctx, ST_SIFT_SORT);
        launch_sb_unpack(s, S.kfin, S.kp_cap, S.counts, first_slot, S.kp_xy, S.kp_size, S.kp_angle, S.kp_resp, S.kp_oct, S.kp_count, S.fin_count, S.fin_flags, S.flags, F);
    }
    { StageTimer t(ctx, ST_SIFT_DESC); launch_sb_descriptor(s, S.P, S.G, S.kfin, S.kp_cap, S.counts, S.E, S.desc, S.desc_x, S.cap_x, S.norms, S.flags, first_slot, F, waves); }
    HIPCHK(hipGetLastError());
    return VO_OK;
}

extern "C" int vo_sift_detect_and_compute(vo_ctx* ctx, const uint8_t* img, int h, int w, int channels, int row_stride, const vo_sift_params* p,
                                          float* kp_xy, float* kp_size, float* kp_angle, float* kp_response, int32_t* kp_octave, float* desc,
                                          int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    vo_sift_params def = {0, 3, 0.04, 10.0, 1.6};
    if (!p) p = &def;
    if (!img || !n_out || h < 2 || w < 2 || (channels != 1 && channels != 3 && channels != 4) || row_stride < w * channels || cap < 0)
        FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    // the single-image call = the batched pipeline with one frame; capacities as generous as the per-image lists of cv2 need
    SiftState& S = ctx->sift1;
    // the candidate list can hold EVERY sample of every DoG layer that is searched: with a contrast threshold that rounds to 0
    // (floor(0.5 * contrastThreshold / nOctaveLayers * 255) — e.g. 0.015 with five layers) every sample of a flat region is a
    // scale-space "extremum" (cv2 compares with >=) and only the refinement throws them out again; cv2's lists are unbounded
    long long cand_all = (long long)(2 * w) * (2 * h) * 4 / 3 * (p->n_octave_layers > 0 ? p->n_octave_layers : 1) + 4096;
    if (cand_all < (1 << 20)) cand_all = 1 << 20;
    if (cand_all > (1 << 27)) cand_all = 1 << 27;
    int rc = sift_setup(ctx, S, h, w, p, 1, 1 << 18, 1 << 18, (int)cand_all, 1 << 18, 1, false);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const size_t img_bytes = image_span(1, 0, h, row_stride, w * channels);
    rc = ctx->sift_img.grow(ctx, img_bytes); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->sift_img.p, img, img_bytes, hipMemcpyHostToDevice, s));
    rc = sift_detect_enqueue(ctx, S, ctx->sift_img.p, channels, row_stride, 0, 1); if (rc) return rc;
    int counts[4] = {0, 0, 0, 0}, fin = 0, fl = 0;
    HIPCHK(hipMemcpyAsync(counts, S.counts, sizeof(counts), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&fin, S.fin_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&fl, S.fin_flags, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int warn = fl ? VO_WARN_CAPACITY : VO_OK;
    int m = counts[3];
    std::vector<SiftKp> kps;
    if (p->nfeatures > 0 && m > p->nfeatures) {
        // KeyPointsFilter::retainBest(keypoints, nfeatures): literally what cv2 runs — libstdc++'s nth_element on the response,
        // then every tie with the n-th response kept by partition; the list stays in that permutation
        kps.resize((size_t)m);
        HIPCHK(hipMemcpy(kps.data(), S.kfin, (size_t)m * sizeof(SiftKp), hipMemcpyDeviceToHost));
        auto greater = [](const SiftKp& a, const SiftKp& b) { return a.response > b.response; };
        std::nth_element(kps.begin(), kps.begin() + p->nfeatures - 1, kps.begin() + m, greater);
        const float amb = kps[(size_t)p->nfeatures - 1].response;
        auto new_end = std::partition(kps.begin() + p->nfeatures, kps.begin() + m, [amb](const SiftKp& k) { return k.response >= amb; });
        m = (int)(new_end - kps.begin());
        HIPCHK(hipMemcpyAsync(S.kfin, kps.data(), (size_t)m * sizeof(SiftKp), hipMemcpyHostToDevice, s));
        counts[3] = m;
        HIPCHK(hipMemcpyAsync(S.counts + 3, &counts[3], sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(S.fin_count, &counts[3], sizeof(int), hipMemcpyHostToDevice, s));
    }
    *n_out = m;
    const int nw = m < cap ? m : cap;
    if (nw > 0) {
        rc = sift_describe_enqueue(ctx, S, 0, 1); if (rc) return rc;
        HIPCHK(hipStreamSynchronize(s));
        std::vector<uint8_t> d8(desc ? (size_t)nw * 128 : 0);
        rc = download_keypoints(ctx, {S.kp_xy, S.kp_size, S.kp_angle, S.kp_resp, S.kp_oct, S.desc, 128}, 0, nw,
                                kp_xy, kp_size, kp_angle, kp_response, kp_octave, desc ? d8.data() : nullptr);
        if (rc) return rc;
        for (size_t i = 0; i < d8.size(); i++) desc[i] = (float)d8[i];         // cv2 hands the integer bin values out as float32
    }
    if (ctx->prof) prof_collect(ctx);
    if (m > cap) warn = VO_WARN_CAPACITY;
    return warn;
}

// ---- SIFT as the detector of the batched, HBM-resident path (vo_frames_upload / _detect / vo_pairs_run dispatch on it)
extern "C" int vo_batch_configure_sift(vo_ctx* ctx, int h, int w, const vo_sift_params* params, int max_frames, int max_pairs, int kp_cap)
{
    if (!ctx) return VO_ERR_INVALID;
    vo_sift_params def = {0, 3, 0.04, 10.0, 1.6};
    if (!params) params = &def;
    if (h < 2 || w < 2 || max_frames < 1 || max_pairs < 1 || kp_cap < 0) FAIL(VO_ERR_INVALID, "bad sizes");
    if (params->nfeatures != 0) FAIL(VO_ERR_UNSUPPORTED, "the batched SIFT path keeps every keypoint (nfeatures = 0, cv2.SIFT_create()'s default, as the reference runs it)");
    if (kp_cap == 0) {                                          // default: ~2.5x what a textured frame of this size yields, at least 1024
        const long long px = (long long)h * w;
        kp_cap = (int)(px / 100 < 1024 ? 1024 : px / 100);
    }
    kp_cap = align_up(kp_cap, 256);
    if (kp_cap > 65536) FAIL(VO_ERR_INVALID, "kp_cap > 65536");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    clear_last_run(ctx);                                        // the pair buffers may be replaced below
    drop_slam_stream(ctx);
    // frames per launch chain: the small octaves' launches are latency-bound (a dependent chain of ~50 launches per sub-batch)
    // and the wave-per-keypoint kernels like long grids, so the more frames share a chain the better (1280 x 720, pairs/s with
    // 64 / 96 / 128 / 192 / 256 frames: 4.59 / 4.68 / 4.79 / 4.94 / 4.94 k): up to 192 frames, within 48 GB of scale-space scratch
    // (211 MB per 1280 x 720 frame: the card has 288 GB)
    const char* ev = getenv("VO_SIFT_SUBBATCH");
    int fb = ev ? atoi(ev) : 0;
    if (fb < 1) {
        size_t px = 0;                                         // floats of one plane per octave (the geometry of sift_setup)
        for (int ww = 2 * w, hh = 2 * h; ww >= 1 && hh >= 1; ww /= 2, hh /= 2) px += (size_t)align_up(ww, 16) * hh;
        const size_t per_frame = px * (size_t)(params->n_octave_layers + 3) * sizeof(float);
        const size_t fit = ((size_t)48 << 30) / (per_frame ? per_frame : 1);
        fb = (int)(fit < 192 ? fit : 192);
        if (fb < 1) fb = 1;
    }
    if (fb > max_frames) fb = max_frames;
    // the intermediate lists (sub-batch scratch) are generous whatever kp_cap is: only the final list is cut at kp_cap, in cv2's
    // list order, as long as they do not overflow themselves (flagged)
    const int raw_cap = 2 * kp_cap > 16384 ? 2 * kp_cap : 16384, cand_cap = 8 * kp_cap > 65536 ? 8 * kp_cap : 65536;
    int rc = sift_setup(ctx, ctx->sift, h, w, params, max_frames, kp_cap, raw_cap, cand_cap, raw_cap, fb, true);
    if (rc) return rc;
    if (ctx->pb_pairs < max_pairs || ctx->pb_cap != kp_cap) {
        ctx->pb_mem.release();
        ctx->pb_pairs = ctx->pb_cap = 0;
        HIPCHK(alloc_pairbuf(ctx->pb_mem, ctx->pb, max_pairs, kp_cap, false));
        ctx->pb_pairs = max_pairs; ctx->pb_cap = kp_cap;
    }
    ctx->sift_pairs = max_pairs;
    ctx->detector = 1;
    return VO_OK;
}

extern "C" int vo_frame_features_sift(vo_ctx* ctx, int slot, float* kp_xy, float* kp_size, float* kp_angle, float* kp_response,
                                      int32_t* kp_octave, uint8_t* desc, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    SiftState& S = ctx->sift;
    if (ctx->detector != 1 || !S.configured) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure_sift has not been called");
    if (slot < 0 || slot >= S.max_frames || !n_out) FAIL(VO_ERR_INVALID, "bad slot");
    HIPCHK(hipSetDevice(ctx->device));
    int n = 0, flags = 0;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(&n, S.kp_count + slot, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&flags, S.flags + slot, sizeof(int), hipMemcpyDeviceToHost));
    int warn = (flags & 1) ? VO_WARN_CAPACITY : VO_OK;
    if (n > S.kp_cap) n = S.kp_cap;
    if (n > cap) { n = cap; warn = VO_WARN_CAPACITY; }
    *n_out = n;
    const int rc = download_keypoints(ctx, {S.kp_xy, S.kp_size, S.kp_angle, S.kp_resp, S.kp_oct, S.desc, 128}, (size_t)slot * S.kp_cap, n,
                                      kp_xy, kp_size, kp_angle, kp_response, kp_octave, desc);
    if (rc) return rc;
    if (flags & 2) FAIL(VO_ERR_INVALID, SIFT_NORM_BOUND_MSG, slot);
    return warn;
}

// Parity seam of the SIFT matcher: n descriptor rows the caller chose become slot `slot`, written as if they had been detected —
// desc, the int8 operand image and the norms through the function k_sb_descriptor ends in, kp_count = n, flags recomputed (bit 1
// by the descriptor's rule, bit 0 clear), kp_xy = xy (zeros without), the other keypoint arrays zero for n rows.  The operand
// image and the norms past row n keep whatever an earlier, fuller frame left there: k_nn_l2i8 has to mask them.
extern "C" int vo_stage_sift_rows(vo_ctx* ctx, int slot, const uint8_t* rows, int n, const float* xy)
{
    if (!ctx) return VO_ERR_INVALID;
    SiftState& S = ctx->sift;
    if (ctx->detector != 1 || !S.configured || !S.with_operands) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure_sift has not been called");
    if (slot < 0 || slot >= S.max_frames) FAIL(VO_ERR_INVALID, "bad slot");
    if (n < 0 || n > S.kp_cap || (n > 0 && !rows)) FAIL(VO_ERR_INVALID, "0 <= n <= kp_cap rows are needed");
    slam_stream_slots_written(ctx, slot, 1);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIPCHK(hipStreamSynchronize(s));                        // an asynchronous detection may still be writing the slot; the staging buffer may be in use
    if (n > 0) { int rc = ctx->staging.grow(ctx, (size_t)n * 128); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(S.flags + slot, 0, sizeof(int), s));
    HIPCHK(hipMemcpyAsync(S.kp_count + slot, &n, sizeof(int), hipMemcpyHostToDevice, s));
    if (n > 0) {
        const size_t o = (size_t)slot * S.kp_cap;
        HIPCHK(hipMemcpyAsync(ctx->staging.p, rows, (size_t)n * 128, hipMemcpyHostToDevice, s));
        if (xy) HIPCHK(hipMemcpyAsync(S.kp_xy + o * 2, xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(S.kp_xy + o * 2, 0, (size_t)n * 2 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(S.kp_size + o, 0, (size_t)n * sizeof(float), s)); HIPCHK(hipMemsetAsync(S.kp_angle + o, 0, (size_t)n * sizeof(float), s));
        HIPCHK(hipMemsetAsync(S.kp_resp + o, 0, (size_t)n * sizeof(float), s)); HIPCHK(hipMemsetAsync(S.kp_oct + o, 0, (size_t)n * sizeof(int), s));
        launch_sb_pack_rows(s, ctx->staging.p, n, slot, S.kp_cap, S.desc, S.desc_x, S.cap_x, S.norms, S.flags);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));                        // (the caller's rows, xy and n have been read)
    return VO_OK;
}

// (frames_upload_enqueue has checked the arguments)
static int sift_frames_upload_enqueue(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot)
{
    SiftState& S = ctx->sift;
    const size_t fbytes = (size_t)S.fstride * S.h;
    uint8_t* dst0 = S.frames + (size_t)first_slot * fbytes;
    if (row_stride == S.w && S.fstride == S.w && frame_stride >= (int64_t)S.w * S.h) {
        HIPCHK(hipMemcpy2DAsync(dst0, fbytes, frames, (size_t)frame_stride, fbytes, F, hipMemcpyHostToDevice, ctx->stream));
        return VO_OK;
    }
    for (int f = 0; f < F; f++)
        HIPCHK(hipMemcpy2DAsync(dst0 + (size_t)f * fbytes, S.fstride, frames + (size_t)f * frame_stride, row_stride, S.w, S.h, hipMemcpyHostToDevice, ctx->stream));
    return VO_OK;
}

// (detect_enqueue has checked the arguments)
static int sift_frames_detect_enqueue(vo_ctx* ctx, int first_slot, int F)
{
    SiftState& S = ctx->sift;
    const size_t fbytes = (size_t)S.fstride * S.h;
    for (int f0 = 0; f0 < F; f0 += S.fb) {
        const int n = F - f0 < S.fb ? F - f0 : S.fb;
        int rc = sift_detect_enqueue(ctx, S, S.frames + (size_t)(first_slot + f0) * fbytes, 1, S.fstride, (int64_t)fbytes, n);
        if (rc) return rc;
        rc = sift_describe_enqueue(ctx, S, first_slot + f0, n);
        if (rc) return rc;
    }
    return VO_OK;
}

// ------------------------------------------------------------------ "next" row: JPEG decode (cv2.imread, visual_slam.py:346)
extern "C" int vo_jpeg_info(const uint8_t* data, size_t nbytes, int32_t* h, int32_t* w, int32_t* ncomp, int32_t* sampling, int32_t* orientation)
{
    int hh = 0, ww = 0, nc = 0, sa = 0, orr = 0;
    const int rc = jpeg_info(data, nbytes, &hh, &ww, &nc, &sa, &orr);
    if (rc == VO_ERR_INVALID) return rc;
    if (h) *h = hh; if (w) *w = ww; if (ncomp) *ncomp = nc; if (sampling) *sampling = sa; if (orientation) *orientation = orr;
    return rc;
}

// Decodes files [f0, f0 + n) of the blob into ctx->jpg_out.p (device, B G R, image k at k * out_frame bytes, rows of
// out_w * 3 bytes).  Every file must be exactly out_h x out_w.  Leaves the work queued on the context's stream.
// With `gray` (device; image k's plane at gray + k * gray_frame, rows of gray_stride >= align_up(out_w, 4) bytes) the colour
// conversion writes cvtColor(BGR2GRAY) of the decoded pixels there instead and ctx->jpg_out.p is not touched.
static int jpeg_decode_device(vo_ctx* ctx, const uint8_t* blob, const int64_t* offsets, int f0, int n, int out_h, int out_w,
                              uint8_t* gray = nullptr, size_t gray_frame = 0, int gray_stride = 0)
{
    std::vector<JpegImage> imgs((size_t)n);
    std::vector<JpegTables> tabs;                          // one per DISTINCT header (the frames of one camera share theirs)
    tabs.reserve(4);
    JpegTables scratch;
    const size_t base = (size_t)offsets[f0], bytes = (size_t)(offsets[f0 + n] - offsets[f0]);
    size_t clean = 0, rst = 0, blocks = 0, planes = 0;
    int max_blocks = 0;
    static const bool full_tables = getenv("VO_JPEG_FULL_TABLES") != nullptr;    // (test hook: the eight-slot kernel for every batch)
    bool packed_tables = !full_tables;
    for (int k = 0; k < n; k++) {
        const char* why = "";
        const size_t o = (size_t)offsets[f0 + k], len = (size_t)(offsets[f0 + k + 1] - offsets[f0 + k]);
        bool same = false;
        const int rc = k == 0 ? jpeg_parse(blob + o, len, &imgs[k], &scratch, &why)
                              : jpeg_parse(blob + o, len, &imgs[k], &scratch, &why, blob + (size_t)offsets[f0 + k - 1], imgs[k - 1].hdr_len,
                                           &imgs[k - 1], nullptr, &same);
        if (rc) FAIL(rc, "JPEG %d: %s", f0 + k, why);
        JpegImage& im = imgs[k];
        if (!same) tabs.push_back(scratch);
        im.tab_idx = (uint32_t)tabs.size() - 1;
        if (im.H != out_h || im.W != out_w) FAIL(VO_ERR_INVALID, "JPEG %d is %d x %d, the batch expects %d x %d", f0 + k, im.W, im.H, out_w, out_h);
        im.raw_off = (uint32_t)(o - base + im.hdr_len);
        im.clean_off = (uint32_t)clean; clean += ((size_t)im.raw_len + JPG_PAD + 15) & ~(size_t)15;
        im.rst_off = (uint32_t)rst; im.rst_cap = im.ri ? (uint32_t)((im.mx * im.my + im.ri - 1) / im.ri + 2) : 0; rst += im.rst_cap;
        im.coef_blk = (uint32_t)blocks; blocks += (size_t)im.total_blocks;
        for (int c = 0; c < im.nc; c++) { im.plane_off[c] = planes; planes += ((size_t)im.bw[c] * 8 * im.bh[c] * 8 + 255) & ~(size_t)255; }
        if (gray) { im.out_off = (uint64_t)k * gray_frame; im.out_stride = (uint32_t)gray_stride; }
        else { im.out_off = (uint64_t)k * out_h * out_w * 3; im.out_stride = (uint32_t)out_w * 3; }
        if (im.total_blocks > max_blocks) max_blocks = im.total_blocks;
        {
            unsigned named = 0;                            // Huffman tables the scan names (bits 0-3: DC, 4-7: AC)
            for (int c = 0; c < im.nc && c < 3; c++) named |= (1u << (im.td[c] & 3)) | (16u << (im.ta[c] & 3));
            if (__builtin_popcount(named) > 4) packed_tables = false;
        }
        if (clean > 0xf0000000ull || blocks > 0xf0000000ull) FAIL(VO_ERR_UNSUPPORTED, "JPEG batch too large for one launch");
    }
    if (bytes > 0xf0000000ull) FAIL(VO_ERR_UNSUPPORTED, "JPEG batch too large for one launch");
    int rc;
    if ((rc = ctx->jpg_blob.grow(ctx, bytes + 16))) return rc;
    if ((rc = ctx->jpg_clean.grow(ctx, clean + 16))) return rc;
    if ((rc = ctx->jpg_rst.grow(ctx, (rst + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = ctx->jpg_coef.grow(ctx, blocks * 128 + 16))) return rc;
    if ((rc = ctx->jpg_planes.grow(ctx, planes + 256))) return rc;
    if (!gray && (rc = ctx->jpg_out.grow(ctx, (size_t)n * out_h * out_w * 3 + 16))) return rc;
    if ((rc = ctx->jpg_img.grow(ctx, (size_t)n * sizeof(JpegImage)))) return rc;
    if ((rc = ctx->jpg_tab.grow(ctx, tabs.size() * sizeof(JpegTables)))) return rc;
    hipStream_t s = ctx->stream;
    // The coefficient blocks start out cleared (the entropy decoder stores only the coefficients the stream names): 2.8 MB per
    // 1280 x 720 file.  The fill runs on a stream of its own — ordered behind everything queued so far (the previous batch's
    // IDCT still reads the buffer), in front of k_jpeg_huffman — so that it shares the time of the files' upload and of
    // k_jpeg_unstuff instead of standing in the decoder's way (in front of the kernels: 0.15 ms per 257 files; inside
    // k_jpeg_huffman: 0.14 ms, the first wait for a load also waits for the stores issued before it).
    if (!ctx->stream_jpg && hipStreamCreateWithFlags(&ctx->stream_jpg, hipStreamNonBlocking) == hipSuccess) {
        if (hipEventCreateWithFlags(&ctx->ev_jpg[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_jpg[1], hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(ctx->stream_jpg); ctx->stream_jpg = nullptr;
        }
    }
    hipEvent_t cleared = nullptr;
    if (ctx->stream_jpg) {
        HIPCHK(hipEventRecord(ctx->ev_jpg[0], s));
        HIPCHK(hipStreamWaitEvent(ctx->stream_jpg, ctx->ev_jpg[0], 0));
        HIPCHK(hipMemsetAsync(ctx->jpg_coef.p, 0, blocks * 128, ctx->stream_jpg));
        HIPCHK(hipEventRecord(ctx->ev_jpg[1], ctx->stream_jpg));
        cleared = ctx->ev_jpg[1];
    } else HIPCHK(hipMemsetAsync(ctx->jpg_coef.p, 0, blocks * 128, s));
    HIPCHK(hipMemcpyAsync(ctx->jpg_blob.p, blob + base, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->jpg_img.p, imgs.data(), (size_t)n * sizeof(JpegImage), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->jpg_tab.p, tabs.data(), tabs.size() * sizeof(JpegTables), hipMemcpyHostToDevice, s));
    {
        StageTimer t(ctx, ST_MISC);
        launch_jpeg_decode(s, ctx->jpg_blob.p, (JpegImage*)ctx->jpg_img.p, (const JpegTables*)ctx->jpg_tab.p, n, ctx->jpg_clean.p, (uint32_t*)ctx->jpg_rst.p,
                           (int16_t*)ctx->jpg_coef.p, ctx->jpg_planes.p, gray ? gray : ctx->jpg_out.p, max_blocks, out_w, out_h, gray != nullptr, packed_tables, cleared);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));                  // the host vectors must outlive their copies
    if (getenv("VO_DEBUG")) {
        HIPCHK(hipMemcpy(imgs.data(), ctx->jpg_img.p, (size_t)n * sizeof(JpegImage), hipMemcpyDeviceToHost));
        uint32_t mx = 0; double sum = 0;
        for (int k = 0; k < n; k++) { mx = imgs[k].sync_rounds > mx ? imgs[k].sync_rounds : mx; sum += imgs[k].sync_rounds; }
        fprintf(stderr, "jpeg: %d files, synchronisation rounds mean %.2f max %u (clean bytes of file 0: %u)\n", n, sum / n, mx, imgs[0].clean_len);
    }
    return VO_OK;
}

// how many files of a batch go through the device at once (coefficients: 2 bytes per sample and component)
static int jpeg_chunk(int h, int w, int F)
{
    // one workgroup decodes one file's entropy stream, so a launch wants at least as many files as the GPU has CUs (256):
    // 24 GB of work buffers per launch = 360 files of 3840 x 2160 (the card has 288 GB)
    const size_t per = (size_t)h * w * 8 + (1 << 20);
    size_t c = ((size_t)24 << 30) / per;
    if (c < 1) c = 1;
    return c > (size_t)F ? F : (int)c;
}

extern "C" int vo_jpeg_decode_batch(vo_ctx* ctx, const uint8_t* blob, const int64_t* offsets, int F, uint8_t* bgr_out, int h, int w)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!blob || !offsets || !bgr_out || F < 0 || h < 1 || w < 1) FAIL(VO_ERR_INVALID, "bad arguments");
    for (int f = 0; f < F; f++) if (offsets[f + 1] < offsets[f] + 4) FAIL(VO_ERR_INVALID, "file %d is empty", f);
    if (F == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const int chunk = jpeg_chunk(h, w, F);
    const size_t per = (size_t)h * w * 3;
    for (int f0 = 0; f0 < F; f0 += chunk) {
        const int n = F - f0 < chunk ? F - f0 : chunk;
        const int rc = jpeg_decode_device(ctx, blob, offsets, f0, n, h, w);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(bgr_out + (size_t)f0 * per, ctx->jpg_out.p, per * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_jpeg_decode(vo_ctx* ctx, const uint8_t* data, size_t nbytes, uint8_t* bgr_out, int cap_h, int cap_w, int32_t* h, int32_t* w)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!data || !bgr_out) FAIL(VO_ERR_INVALID, "bad arguments");
    int hh = 0, ww = 0, nc = 0, sa = 0, orr = 0;
    const int irc = jpeg_info(data, nbytes, &hh, &ww, &nc, &sa, &orr);
    if (irc == VO_ERR_INVALID) FAIL(VO_ERR_INVALID, "not a JPEG file");
    if (h) *h = hh; if (w) *w = ww;
    if (irc) FAIL(irc, "JPEG frame type outside the baseline decoder (progressive, lossless, arithmetic or 12-bit)");
    if (hh > cap_h || ww > cap_w) FAIL(VO_ERR_INVALID, "output buffer %d x %d too small for a %d x %d image", cap_w, cap_h, ww, hh);
    const int64_t offs[2] = {0, (int64_t)nbytes};
    return vo_jpeg_decode_batch(ctx, data, offs, 1, bgr_out, hh, ww);
}

extern "C" int vo_frames_ingest_jpeg(vo_ctx* ctx, const uint8_t* blob, const int64_t* offsets, int F, int first_slot, uint8_t* resized_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (!blob || !offsets || F < 0 || first_slot < 0 || first_slot + F > b.max_frames) FAIL(VO_ERR_INVALID, "slot range out of bounds");
    slam_stream_slots_written(ctx, first_slot, F);
    for (int f = 0; f < F; f++) if (offsets[f + 1] < offsets[f] + 4) FAIL(VO_ERR_INVALID, "file %d is empty", f);
    if (F == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    int sh = 0, sw = 0, nc = 0, sa = 0, orr = 0;
    const int irc = jpeg_info(blob + offsets[0], (size_t)(offsets[1] - offsets[0]), &sh, &sw, &nc, &sa, &orr);
    if (irc) FAIL(irc, "file 0 is not a baseline JPEG");
    const int chunk = jpeg_chunk(sh, sw, F);
    const int dw = b.w, dh = b.h;
    const size_t dper = (size_t)dw * dh * 3;
    for (int f0 = 0; f0 < F; f0 += chunk) {
        const int n = F - f0 < chunk ? F - f0 : chunk;
        if (sw == dw && sh == dh && !resized_out && b.gray_stride >= align_up(dw, 4)) {
            // files of the configured size and nobody wants the colour frames: cv::resize is a copy, so the decoder's colour
            // conversion writes the gray frames of the slots itself (no B G R frames in memory, no k_gray pass)
            const int rc = jpeg_decode_device(ctx, blob, offsets, f0, n, sh, sw, b.gray_slot(first_slot + f0), b.gray_frame, b.gray_stride);
            if (rc) return rc;
            continue;
        }
        int rc = jpeg_decode_device(ctx, blob, offsets, f0, n, sh, sw);
        if (rc) return rc;
        rc = ingest_from_device(ctx, ctx->jpg_out.p, n, sh, sw, 3, sw * 3, (int64_t)sh * sw * 3, first_slot + f0,
                                resized_out ? resized_out + (size_t)f0 * dper : nullptr);
        if (rc) return rc;
    }
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// ------------------------------------------------------------------ "next" row: feature-track bookkeeping
extern "C" int vo_feature_tracks(vo_ctx* ctx, int F, int cap, const int32_t* pair_frames, const int32_t* match_off,
                                 const int32_t* mq, const int32_t* mt, int P, int32_t* root_frame, int32_t* root_idx, int32_t* hops)
{
    if (!ctx) return VO_ERR_INVALID;
    if (F < 1 || cap < 1 || P < 0 || F >= (1 << 20) || cap >= (1 << 20) || !root_frame || !root_idx || !hops ||
        (P > 0 && (!pair_frames || !match_off || !mq || !mt))) FAIL(VO_ERR_INVALID, "bad arguments");
    int total = 0, max_m = 0;
    for (int p = 0; p < P; p++) {
        const int n = match_off[p + 1] - match_off[p];
        if (n < 0 || pair_frames[2 * p] < 0 || pair_frames[2 * p] >= F || pair_frames[2 * p + 1] < 0 || pair_frames[2 * p + 1] >= F)
            FAIL(VO_ERR_INVALID, "pair %d refers to a missing frame", p);
        if (n > max_m) max_m = n;
    }
    if (P > 0) total = match_off[P] - match_off[0];
    for (int i = 0; i < total; i++)
        if (mq[match_off[0] + i] < 0 || mq[match_off[0] + i] >= cap || mt[match_off[0] + i] < 0 || mt[match_off[0] + i] >= cap)
            FAIL(VO_ERR_INVALID, "match %d refers to a missing feature", i);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t fc = (size_t)F * cap;
    unsigned long long* dparent; int *dpf, *doff, *dq, *dt, *drf, *dri, *dh, *dbad;
    ScratchLayout sc;
    sc.take(&dparent, fc); sc.take(&dpf, (size_t)2 * P); sc.take(&doff, (size_t)P + 1); sc.take(&dq, total); sc.take(&dt, total);
    sc.take(&drf, fc); sc.take(&dri, fc); sc.take(&dh, fc); sc.take(&dbad, 1);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemsetAsync(dparent, 0, fc * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(dbad, 0, sizeof(int), s));
    if (P > 0) {
        std::vector<int> off(P + 1);
        for (int p = 0; p <= P; p++) off[p] = match_off[p] - match_off[0];
        HIPCHK(hipMemcpyAsync(dpf, pair_frames, (size_t)2 * P * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(doff, off.data(), (size_t)(P + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (total > 0) {
            HIPCHK(hipMemcpyAsync(dq, mq + match_off[0], (size_t)total * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(dt, mt + match_off[0], (size_t)total * sizeof(int), hipMemcpyHostToDevice, s));
        }
        HIPCHK(hipStreamSynchronize(s));                              // `off` is a stack vector
    }
    { StageTimer t(ctx, ST_MISC); launch_tracks(s, dpf, doff, dq, dt, P, max_m, F, cap, dparent, drf, dri, dh, dbad); }
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(root_frame, drf, fc * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(root_idx, dri, fc * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hops, dh, fc * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    if (bad) FAIL(VO_ERR_INVALID, "the feature map contains a cycle");
    return VO_OK;
}

// What vo_tracks_pnp_batch and vo_slam_chain ask of the most recent vo_pairs_run: all its B pairs, triangulated, every slot
// inside the configuration, the pairs a chain of distinct frames (a0, b0), (b0, b1), ...: the order the reference walks a sequence in
static int chain_check(vo_ctx* ctx, int B, const char* who, int* F_out, int* cap_out)
{
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (B < 1 || B != ctx->last.pairs) FAIL(VO_ERR_INVALID, "%s takes all %d pairs of the most recent vo_pairs_run", who, ctx->last.pairs);
    if (!ctx->last.points) FAIL(VO_ERR_INVALID, "the most recent vo_pairs_run did not triangulate (want_points)");
    const int F = b.max_frames, cap = b.kp_cap;
    const int32_t* sl = ctx->last.slots.data();
    for (int i = 0; i < 2 * B; i++)
        if (sl[i] < 0 || sl[i] >= F) FAIL(VO_ERR_INVALID, "pair slot %d of the most recent vo_pairs_run is out of range", sl[i]);
    std::vector<char> seen((size_t)F, 0);
    seen[(size_t)sl[0]] = 1;
    for (int p = 0; p < B; p++) {
        if ((p > 0 && sl[2 * p] != sl[2 * p - 1]) || seen[(size_t)sl[2 * p + 1]])
            FAIL(VO_ERR_INVALID, "pair %d (%d, %d) does not continue a chain of distinct frames", p, sl[2 * p], sl[2 * p + 1]);
        seen[(size_t)sl[2 * p + 1]] = 1;
    }
    if (F >= (1 << 20) || cap >= (1 << 20)) FAIL(VO_ERR_INVALID, "too many frames or keypoints for the packed track table");
    *F_out = F; *cap_out = cap;
    return VO_OK;
}

// ------------------------------------------------------------------ measurement
// ------------------------------------------------------------------ the step after the pair path, on resident data
// VisualSlam.estimate_current_camera_position + add_information_to_map (src/visual_slam.py:183-266, 153-180) for the pairs the
// most recent vo_pairs_run (want_points) left in HBM: feature tracks -> (map, image) coordinates -> solvePnPRansac -> camera ->
// new map points, pair after pair on the context's stream with no host round trip (the kernels: geom_kernels.hip k_chain_*,
// pnp_kernels.hip k_pnp_ransac / k_chain_pose).
extern "C" int vo_tracks_pnp_batch(vo_ctx* ctx, int B, const double* K, int iterations, double reproj_err, double confidence, uint64_t seed,
                                   double max_point_norm, double* poses, int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_map)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!K || !poses || !n_corr || !n_inl || !status || !n_map) FAIL(VO_ERR_INVALID, "bad arguments");
    int F, cap;
    int rc = chain_check(ctx, B, "vo_tracks_pnp_batch", &F, &cap); if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const size_t fc = (size_t)F * cap;
    ChainBuf cb{}; double* dK; uint8_t* dec;
    ScratchLayout sc;
    sc.take(&cb.parent, fc); sc.take(&cb.map_pt, fc * 3); sc.take(&cb.cam, (size_t)F * 12); sc.take(&cb.obj, (size_t)cap * 3); sc.take(&cb.img, (size_t)cap * 2);
    sc.take(&cb.rvec, 3); sc.take(&cb.tvec, 3); sc.take(&cb.P1, 12); sc.take(&cb.P2, 12); sc.take(&cb.Xw, (size_t)cap * 4); sc.take(&cb.poses, (size_t)(B + 1) * 12);
    sc.take(&dK, 9); sc.take(&cb.in_map, fc); sc.take(&dec, cap); sc.take(&cb.cam_ok, F); sc.take(&cb.off, 2); sc.take(&cb.pmask, cap); sc.take(&cb.pninl, 1); sc.take(&cb.pstatus, 1);
    sc.take(&cb.alive, 1); sc.take(&cb.n_corr, B); sc.take(&cb.n_inl, B); sc.take(&cb.status, B); sc.take(&cb.n_map, B); sc.take(&cb.map_count, 1);
    rc = sc.place(ctx); if (rc) return rc;
    HIPCHK(hipMemsetAsync(ctx->scratch.p, 0, sc.bytes, s));          // empty feature_mapper, empty map, no cameras
    HIPCHK(hipMemcpyAsync(dK, K, 72, hipMemcpyHostToDevice, s));
    {
        StageTimer t(ctx, ST_MISC);
        launch_chain_link(s, ctx->pb, cap, B, cb);
        launch_chain_init(s, ctx->pb, cap, cb);
        for (int p = 1; p < B; p++) {
            launch_chain_gather(s, ctx->pb, cap, p, F, cb);
            launch_pnp_ransac(s, cb.obj, cb.img, cb.off, 1, dK, iterations, reproj_err, confidence, seed, ctx->rng_tab, RNG_TAB_N, ctx->pnp_refine,
                              cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus);
            launch_chain_pose(s, ctx->pb, p, dK, cb);
            launch_chain_triangulate(s, ctx->pb, cap, p, cb);
            launch_chain_insert(s, ctx->pb, cap, p, F, max_point_norm, cb, dec);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(poses, cb.poses, (size_t)(B + 1) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_corr, cb.n_corr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, cb.n_inl, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, cb.status, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_map, cb.n_map, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// ------------------------------------------------------------------ the reference's complete per-frame map step, on resident data
// vo_tracks_pnp_batch's walk with what ends every frame of VisualSlam.estimate_current_camera_position (src/visual_slam.py:190-266)
// joined to it: the Observations of add_information_to_map, freeze_nonlast_cameras, Map.optimize_map, the threshold filter and
// limit_number_of_camera_in_map — on a map that stays in HBM (slam_kernels.hip), pair after pair with no host round trip.
// The map's three lists, carved from one block so that a snapshot is one device-to-device copy; base == nullptr: the size only
static size_t slam_map_carve(uint8_t* base, size_t ncam, size_t npt, size_t nobs, SlamMap* m)
{
    size_t o = 0;
    auto put = [&](auto** p, size_t n) {
        using T = typename std::remove_pointer<typename std::remove_pointer<decltype(p)>::type>::type;
        if (base) *p = reinterpret_cast<T*>(base + o);
        o += (n * sizeof(T) + 255) & ~(size_t)255;
    };
    put(&m->cnt, 4); put(&m->cam_frame, ncam); put(&m->cam_pose, ncam * 12); put(&m->cam_fixed, ncam); put(&m->pt_key, npt); put(&m->pt_xyz, npt * 3);
    put(&m->obs_cam, nobs); put(&m->obs_pt, nobs); put(&m->obs_xy, nobs * 2);
    return o;
}

// first, count: the pairs of the run that are the map's chain (pt_feature names a frame by its index along that chain)
static int slam_map_download(vo_ctx* ctx, const SlamMap& m, int cap, LastRun::Map* out, int first = 0, int count = -1)
{
    int cnt[4];
    HIPCHK(hipMemcpy(cnt, m.cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    const size_t nc = cnt[0], np = cnt[1], no = cnt[2];
    std::vector<int32_t> key(np);
    out->cam_frame.resize(nc); out->cam_pose.resize(nc * 12); out->cam_fixed.resize(nc); out->points.resize(np * 3);
    out->obs_cam.resize(no); out->obs_pt.resize(no); out->obs_xy.resize(no * 2); out->pt_feature.resize(np * 2);
    if (nc) {
        HIPCHK(hipMemcpy(out->cam_frame.data(), m.cam_frame, nc * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->cam_pose.data(), m.cam_pose, nc * 96, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->cam_fixed.data(), m.cam_fixed, nc, hipMemcpyDeviceToHost));
    }
    if (np) {
        HIPCHK(hipMemcpy(key.data(), m.pt_key, np * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->points.data(), m.pt_xyz, np * 24, hipMemcpyDeviceToHost));
    }
    if (no) {
        HIPCHK(hipMemcpy(out->obs_cam.data(), m.obs_cam, no * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->obs_pt.data(), m.obs_pt, no * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out->obs_xy.data(), m.obs_xy, no * 16, hipMemcpyDeviceToHost));
    }
    if (m.pt_feat) {                                                  // vo_slam_stream keeps the feature ids as (frame, keypoint) on the device
        if (np) HIPCHK(hipMemcpy(out->pt_feature.data(), m.pt_feat, np * 8, hipMemcpyDeviceToHost));
        out->valid = true;
        return VO_OK;
    }
    // feature id (slot, keypoint) -> (index of the frame in the chain, keypoint)
    const int32_t* sl = ctx->last.slots.data() + 2 * (size_t)first;
    const size_t npairs = count < 0 ? ctx->last.slots.size() / 2 : (size_t)count;
    for (size_t i = 0; i < np; i++) {
        const int slot = key[i] / cap;
        int frame = sl[0] == slot ? 0 : -1;
        for (size_t p = 0; frame < 0 && p < npairs; p++) if (sl[2 * p + 1] == slot) frame = (int)p + 1;
        out->pt_feature[2 * i] = frame; out->pt_feature[2 * i + 1] = key[i] % cap;
    }
    out->valid = true;
    return VO_OK;
}

static void forget_slam_maps(vo_ctx* ctx)
{
    ctx->last.map[0] = LastRun::Map(); ctx->last.map[1] = LastRun::Map();
    ctx->last.seq_map.clear(); ctx->last.snap_map = LastRun::Map(); ctx->last.snap_seq = -1;
    ctx->last.stats = LastRun::Stats();
}

// the rows of a call that has come through (its stream has been waited for) -> the context's host copy
static int slam_stats_download(vo_ctx* ctx, const StatsBuf& d, std::vector<int32_t> seq_off)
{
    LastRun::Stats& h = ctx->last.stats;
    const size_t P = (size_t)seq_off.back(), C = (size_t)d.C;
    h = LastRun::Stats();
    h.total_sqerr.resize(P); h.max_sqerr.resize(P); h.n_high.resize(P); h.counts.resize(P * 3); h.obs_hist.resize(P * VO_STATS_HIST); h.obs_matrix.resize(P * C * C); h.cam_frame.resize(P * C);
    HIPCHK(hipMemcpy(h.total_sqerr.data(), d.total_sqerr, P * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.max_sqerr.data(), d.max_sqerr, P * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.n_high.data(), d.n_high, P * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.counts.data(), d.counts, P * 12, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.obs_hist.data(), d.obs_hist, P * VO_STATS_HIST * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.obs_matrix.data(), d.obs_matrix, P * C * C * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.cam_frame.data(), d.cam_frame, P * C * 4, hipMemcpyDeviceToHost));
    h.C = d.C; h.seq_off = std::move(seq_off); h.valid = true;
    return VO_OK;
}

// the option checks that ask nothing of a vo_pairs_run (vo_slam_streams_open has none)
static int slam_opts_check_values(vo_ctx* ctx, const vo_slam_opts* o, const double* K)
{
    if (o->ba_iterations < 0 || o->ba_iterations > 1000) FAIL(VO_ERR_INVALID, "ba_iterations must be 0 .. 1000, got %d", o->ba_iterations);
    if (o->free_cameras < 1) FAIL(VO_ERR_INVALID, "free_cameras must be at least 1, got %d", o->free_cameras);
    if (o->free_cameras > VO_BA_MAX_FREE) FAIL(VO_ERR_UNSUPPORTED, "bundle adjustment frees at most %d cameras, got %d", VO_BA_MAX_FREE, o->free_cameras);
    if (o->max_cameras < 2) FAIL(VO_ERR_INVALID, "max_cameras must be at least 2, got %d", o->max_cameras);
    if ((int64_t)o->max_cameras + 1 > VO_BA_MAX_CAMERAS)
        FAIL(VO_ERR_UNSUPPORTED, "the map holds max_cameras + 1 cameras before the limit is applied, bundle adjustment at most %d", VO_BA_MAX_CAMERAS);
    if (!(o->huber_delta == o->huber_delta) || !(o->filter_threshold == o->filter_threshold) || !(K[0] == K[0]) || !(K[2] == K[2]) || !(K[5] == K[5]))
        FAIL(VO_ERR_INVALID, "camera parameters and thresholds must be numbers");
    return VO_OK;
}

// the option checks of vo_slam_chain and vo_slam_chains; B_snap: pairs of the chain snapshot_pair counts along
static int slam_opts_check(vo_ctx* ctx, const vo_slam_opts* o, const double* K, int B_snap, const char* who)
{
    if (ctx->last.match_mode == 1 || ctx->last.match_mode == 3)
        FAIL(VO_ERR_UNSUPPORTED, "%s needs one-to-one matches (cross-check): with ratio or nearest-neighbour matches two inliers can share a track root", who);
    const int rc = slam_opts_check_values(ctx, o, K); if (rc) return rc;
    if ((o->snapshot_pair >= 0) != (o->snapshot_stage >= 1) || o->snapshot_pair >= B_snap || o->snapshot_stage > 4)
        FAIL(VO_ERR_INVALID, "snapshot_pair must be -1 or a pair of the chain, snapshot_stage 1 .. 4 with it");
    return VO_OK;
}

extern "C" int vo_slam_chain(vo_ctx* ctx, int B, const double* K, const vo_slam_opts* o, double* poses_pnp, double* poses,
                             int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                             double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!K || !o || !poses_pnp || !poses || !n_corr || !n_inl || !status || !n_pts || !n_obs || !n_cam || !chi2 || !ba_iterations_run || !ba_trials_run)
        FAIL(VO_ERR_INVALID, "bad arguments");
    int F, cap;
    drop_slam_stream(ctx);
    int rc = chain_check(ctx, B, "vo_slam_chain", &F, &cap); if (rc) return rc;
    forget_slam_maps(ctx);
    rc = slam_opts_check(ctx, o, K, B, "vo_slam_chain"); if (rc) return rc;
    const size_t fc = (size_t)F * cap;
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    // capacities from the configuration: a pair adds at most one point and two observations per match
    const size_t cm = (size_t)o->max_cameras + 1, np = fc, no = (size_t)2 * B * cap, npair = no * (o->free_cameras + 1) / 2;
    const int nblk = o->free_cameras * (o->free_cameras + 1) / 2;
    if (np >= ((size_t)1 << 31) || npair >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the map's lists would not fit 32-bit indices");
    ChainBuf cb{}; SlamBuf sb{}; BaBuf D{}; double* dK; uint8_t *map_mem, *snap_mem;
    const size_t map_bytes = slam_map_carve(nullptr, cm, np, no, &sb.m);
    ScratchLayout sc;
    sc.take(&cb.parent, fc); sc.take(&cb.map_pt, fc * 3); sc.take(&cb.cam, (size_t)F * 12); sc.take(&cb.obj, (size_t)cap * 3); sc.take(&cb.img, (size_t)cap * 2);
    sc.take(&cb.rvec, 3); sc.take(&cb.tvec, 3); sc.take(&cb.P1, 12); sc.take(&cb.P2, 12); sc.take(&cb.Xw, (size_t)cap * 4); sc.take(&cb.poses, (size_t)(B + 1) * 12);
    sc.take(&dK, 9); sc.take(&cb.in_map, fc); sc.take(&cb.cam_ok, F); sc.take(&cb.off, 2); sc.take(&cb.pmask, cap); sc.take(&cb.pninl, 1); sc.take(&cb.pstatus, 1);
    sc.take(&cb.alive, 1); sc.take(&cb.n_corr, B); sc.take(&cb.n_inl, B); sc.take(&cb.status, B); sc.take(&cb.n_map, B); sc.take(&cb.map_count, 1);
    sc.take(&map_mem, map_bytes); sc.take(&snap_mem, map_bytes);
    sc.take(&sb.pt_of, fc); sc.take(&sb.dec, cap); sc.take(&sb.tmp, np); sc.take(&sb.idx, no); sc.take(&sb.n_pts, B); sc.take(&sb.n_obs, B); sc.take(&sb.n_cam, B);
    sc.take(&sb.poses_last, (size_t)(B + 1) * 12);
    sc.take(&sb.prob, 1); sc.take(&sb.cam_col, cm); sc.take(&sb.pt_first, np + 1); sc.take(&sb.s_cam, no); sc.take(&sb.s_pt, no); sc.take(&sb.s_xy, no * 2);
    sc.take(&sb.pairs, npair); sc.take(&sb.blk_first, (size_t)nblk + 1);
    sc.take(&D.X2, np * 3); sc.take(&D.W, no * 18); sc.take(&D.Hpp, np * 6); sc.take(&D.bp, np * 3); sc.take(&D.Hpi, np * 6);
    double* dchi2; int *dit, *dtr;
    sc.take(&dchi2, (size_t)2 * B); sc.take(&dit, B); sc.take(&dtr, B);
    const bool stats_on = ctx->slam_stats != 0;
    StatsBuf stats{};
    slam_stats_take_scratch(sc, stats, stats_on, np, no); slam_stats_take_rows(sc, stats, stats_on, B, cm);
    rc = sc.place(ctx); if (rc) return rc;
    stats.Kd = dK;
    SlamMap snap{};
    slam_map_carve(map_mem, cm, np, no, &sb.m); slam_map_carve(snap_mem, cm, np, no, &snap);
    sb.cam_cap = (int)cm; sb.pt_cap = (int)np; sb.obs_cap = (int)no; sb.pair_cap = (int)npair;
    D.prob = sb.prob; D.poses = sb.m.cam_pose; D.cam_col = sb.cam_col; D.X = sb.m.pt_xyz; D.pt_first = sb.pt_first;
    D.obs_cam = sb.s_cam; D.obs_pt = sb.s_pt; D.obs_xy = sb.s_xy; D.pairs = sb.pairs; D.blk_first = sb.blk_first;
    HIPCHK(hipMemsetAsync(ctx->scratch.p, 0, sc.bytes, s));          // empty feature_mapper, empty map, no cameras, zero results
    HIPCHK(hipMemcpyAsync(dK, K, 72, hipMemcpyHostToDevice, s));
    const BaParams prm{K[0], K[2], K[5], o->huber_delta, o->ba_iterations};
    const bool ba = o->ba_iterations > 0, filt = o->filter_threshold > 0;
    auto snapshot = [&](int p, int stage) {
        if (p == o->snapshot_pair && stage == o->snapshot_stage) (void)hipMemcpyAsync(snap_mem, map_mem, map_bytes, hipMemcpyDeviceToDevice, s);
    };
    launch_chain_link(s, ctx->pb, cap, B, cb);
    for (int p = 0; p < B; p++) {
        {
            StageTimer t(ctx, ST_MISC);
            if (p == 0) launch_chain_init(s, ctx->pb, cap, cb);
            else {
                launch_chain_gather(s, ctx->pb, cap, p, F, cb);
                launch_pnp_ransac(s, cb.obj, cb.img, cb.off, 1, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                                  ctx->pnp_refine, cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus);
                launch_chain_pose(s, ctx->pb, p, dK, cb);
                launch_chain_triangulate(s, ctx->pb, cap, p, cb);
            }
            launch_slam_add(s, ctx->pb, cap, p, F, o->max_point_norm, o->free_cameras, cb, sb);
        }
        snapshot(p, 1);
        if (ba) {
            { StageTimer t(ctx, ST_SLAM_PREPARE); launch_slam_ba_prepare(s, cb, sb); }
            BaBuf Dp = D;
            Dp.chi2 = dchi2 + 2 * p; Dp.iterations_run = dit + p; Dp.trials_run = dtr + p;
            { StageTimer t(ctx, ST_SLAM_BA); launch_bundle_adjust(s, Dp, prm, 1, o->free_cameras); }
        }
        snapshot(p, 2);
        // pair 0 ends with optimize_map (:90); what it wrote back still has to reach the tables the next pair reads
        if (ba || (filt && p > 0)) { StageTimer t(ctx, ST_SLAM_FILTER); launch_slam_filter(s, ctx->pb, dK, p > 0 ? o->filter_threshold : 0.0, cb, sb); }
        snapshot(p, 3);
        { StageTimer t(ctx, ST_SLAM_LIMIT); launch_slam_limit(s, p, o->max_cameras, cb, sb); }
        snapshot(p, 4);
        if (stats_on) { StageTimer t(ctx, ST_SLAM_STATS); launch_slam_stats(s, p, sb, stats); }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(poses_pnp, cb.poses, (size_t)(B + 1) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(poses, sb.poses_last, (size_t)(B + 1) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_corr, cb.n_corr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, cb.n_inl, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, cb.status, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_pts, sb.n_pts, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_obs, sb.n_obs, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_cam, sb.n_cam, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(chi2, dchi2, (size_t)B * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ba_iterations_run, dit, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ba_trials_run, dtr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    // the scratch buffer belongs to the next call: the two maps are kept as host copies
    rc = slam_map_download(ctx, sb.m, cap, &ctx->last.map[0]); if (rc) return rc;
    if (o->snapshot_pair >= 0) { rc = slam_map_download(ctx, snap, cap, &ctx->last.map[1]); if (rc) return rc; }
    if (stats_on) { rc = slam_stats_download(ctx, stats, {0, B}); if (rc) return rc; }
    return VO_OK;
}

static int slam_map_copy_out(vo_ctx* ctx, const LastRun::Map* m, int32_t* cam_frame, double* cam_pose, uint8_t* cam_fixed, int32_t* pt_feature, double* points,
                             int32_t* obs_cam, int32_t* obs_pt, double* obs_xy)
{
    if ((!m->cam_frame.empty() && (!cam_frame || !cam_pose || !cam_fixed)) || (!m->points.empty() && (!pt_feature || !points)) ||
        (!m->obs_cam.empty() && (!obs_cam || !obs_pt || !obs_xy))) FAIL(VO_ERR_INVALID, "bad arguments");
    auto copy = [](auto* dst, const auto& v) { if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    copy(cam_frame, m->cam_frame); copy(cam_pose, m->cam_pose); copy(cam_fixed, m->cam_fixed); copy(pt_feature, m->pt_feature); copy(points, m->points);
    copy(obs_cam, m->obs_cam); copy(obs_pt, m->obs_pt); copy(obs_xy, m->obs_xy);
    return VO_OK;
}

static const LastRun::Map* slam_map_of(vo_ctx* ctx, int which)
{
    if (which < 0 || which > 1 || !ctx->last.map[which].valid) {
        snprintf(ctx->err, sizeof(ctx->err), which < 0 || which > 1 ? "which must be 0 (the map at the end of the chain) or 1 (the snapshot)"
                                                                   : "no such map: vo_slam_chain has not run (or not with a snapshot) since the last configure / vo_pairs_run");
        return nullptr;
    }
    return &ctx->last.map[which];
}

extern "C" int vo_slam_map_size(vo_ctx* ctx, int which, int32_t* ncam, int32_t* npt, int32_t* nobs)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!ncam || !npt || !nobs) FAIL(VO_ERR_INVALID, "bad arguments");
    const LastRun::Map* m = slam_map_of(ctx, which);
    if (!m) return VO_ERR_INVALID;
    *ncam = (int32_t)m->cam_frame.size(); *npt = (int32_t)(m->points.size() / 3); *nobs = (int32_t)m->obs_cam.size();
    return VO_OK;
}

extern "C" int vo_slam_map(vo_ctx* ctx, int which, int32_t* cam_frame, double* cam_pose, uint8_t* cam_fixed, int32_t* pt_feature, double* points,
                           int32_t* obs_cam, int32_t* obs_pt, double* obs_xy)
{
    if (!ctx) return VO_ERR_INVALID;
    const LastRun::Map* m = slam_map_of(ctx, which);
    if (!m) return VO_ERR_INVALID;
    return slam_map_copy_out(ctx, m, cam_frame, cam_pose, cam_fixed, pt_feature, points, obs_cam, obs_pt, obs_xy);
}

// ------------------------------------------------------------------ the map step, one call after another on one resident map
// vo_slam_chain's walk on buffers of their own lifetime (SlamStream): the first call of a stream clears them as vo_slam_chain
// clears the scratch buffer and runs vo_slam_chain's steps; a call that continues it clears the per-pair outputs only, lets
// k_slam_carry restate the keys (slam_kernels.hip) and runs a p >= 1 step for every pair.  The work buffers keep what the last
// step left in them, as they do between two steps of one call.
static int slam_stream_allocate(vo_ctx* ctx, SlamStream& st, bool restart, int F, int cap, int max_pairs, int total, const vo_slam_opts* o, const double* K)
{
    // the slot-keyed tables have two ghost rows behind the F slots.  Lists: a pair adds at most one point per match; a camera takes
    // at most kp_cap observations as a pair's second frame and kp_cap as the next pair's first (one-to-one matches), and the map
    // holds at most max_cameras + 1 cameras — or every pair's two observations per match, if the stream is shorter than that.
    const size_t fc = (size_t)(F + 2) * cap, cm = (size_t)o->max_cameras + 1, np = ((size_t)total + 1) * cap;
    const size_t no = (size_t)2 * cap * std::min(cm, (size_t)total), npair = no * (o->free_cameras + 1) / 2;
    const int nblk = o->free_cameras * (o->free_cameras + 1) / 2;
    const size_t P = (size_t)max_pairs;
    if (F + 2 >= (1 << 20)) FAIL(VO_ERR_INVALID, "too many frames for the packed track table");
    if (np >= ((size_t)1 << 31) || npair >= ((size_t)1 << 31) || fc >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the map's lists would not fit 32-bit indices");
    ChainBuf& cb = st.cb; SlamBuf& sb = st.sb; BaBuf& D = st.D;
    size_t o_feat = 0;
    st.map_bytes = slam_map_carve(nullptr, cm, np, no, &sb.m);
    o_feat = st.map_bytes; st.map_bytes += (np * 2 * sizeof(int) + 255) & ~(size_t)255;       // pt_feat rides behind the lists: a snapshot takes it along
    ScratchLayout sc;
    sc.take(&cb.parent, fc); sc.take(&cb.map_pt, fc * 3); sc.take(&cb.cam, (size_t)F * 12); sc.take(&cb.obj, (size_t)cap * 3); sc.take(&cb.img, (size_t)cap * 2);
    sc.take(&cb.rvec, 3); sc.take(&cb.tvec, 3); sc.take(&cb.P1, 12); sc.take(&cb.P2, 12); sc.take(&cb.Xw, (size_t)cap * 4);
    sc.take(&st.dK, 9); sc.take(&cb.in_map, fc); sc.take(&cb.cam_ok, F); sc.take(&cb.off, 2); sc.take(&cb.pmask, cap); sc.take(&cb.pninl, 1); sc.take(&cb.pstatus, 1);
    sc.take(&cb.alive, 1); sc.take(&cb.map_count, 1); sc.take(&st.keep, 24);
    sc.take(&cb.rs.st, restart ? 4 : 0);                              // (the segment state outlives the call, as the alive flag does)
    sc.take(&st.map_mem, st.map_bytes); sc.take(&st.snap_mem, st.map_bytes);
    sc.take(&sb.pt_of, fc); sc.take(&sb.dec, cap); sc.take(&sb.tmp, np); sc.take(&sb.idx, no);
    sc.take(&sb.prob, 1); sc.take(&sb.cam_col, cm); sc.take(&sb.pt_first, np + 1); sc.take(&sb.s_cam, no); sc.take(&sb.s_pt, no); sc.take(&sb.s_xy, no * 2);
    sc.take(&sb.pairs, npair); sc.take(&sb.blk_first, (size_t)nblk + 1);
    sc.take(&D.X2, np * 3); sc.take(&D.W, no * 18); sc.take(&D.Hpp, np * 6); sc.take(&D.bp, np * 3); sc.take(&D.Hpi, np * 6);
    st.stats = ctx->slam_stats != 0;
    slam_stats_take_scratch(sc, st.sbuf, st.stats, np, no);
    const size_t call0 = sc.bytes;                                    // from here on: what a call reports, sized for max_pairs pairs
    slam_stats_take_rows(sc, st.sbuf, st.stats, P, cm);
    sc.take(&cb.poses, (P + 1) * 12); sc.take(&cb.n_corr, P); sc.take(&cb.n_inl, P); sc.take(&cb.status, P); sc.take(&cb.n_map, P);
    sc.take(&sb.n_pts, P); sc.take(&sb.n_obs, P); sc.take(&sb.n_cam, P); sc.take(&sb.poses_last, (P + 1) * 12);
    sc.take(&st.dchi2, 2 * P); sc.take(&st.dit, P); sc.take(&st.dtr, P);
    sc.take(&sb.st.carried_frame, cm); sc.take(&sb.st.carried_poses, cm * 12);
    sc.take(&cb.rs.segment, restart ? P : 0); sc.take(&cb.rs.cause, restart ? P : 0);
    sc.take(&cb.rs.seg_poses, restart ? P * 12 : 0); sc.take(&cb.rs.seg_poses_last, restart ? P * 12 : 0);
    HIPCHK(st.mem.alloc(&st.base, sc.bytes));
    sc.place_at(st.base);
    st.sbuf.Kd = st.dK;
    if (!restart) cb.rs = RestartBuf{};
    st.restart = restart;
    st.bytes = sc.bytes; st.call_mem = st.base + call0; st.call_bytes = sc.bytes - call0;
    slam_map_carve(st.map_mem, cm, np, no, &sb.m); slam_map_carve(st.snap_mem, cm, np, no, &st.snap);
    sb.m.pt_feat = reinterpret_cast<int*>(st.map_mem + o_feat); st.snap.pt_feat = reinterpret_cast<int*>(st.snap_mem + o_feat);
    sb.cam_cap = (int)cm; sb.pt_cap = (int)np; sb.obs_cap = (int)no; sb.pair_cap = (int)npair;
    D.prob = sb.prob; D.poses = sb.m.cam_pose; D.cam_col = sb.cam_col; D.X = sb.m.pt_xyz; D.pt_first = sb.pt_first;
    D.obs_cam = sb.s_cam; D.obs_pt = sb.s_pt; D.obs_xy = sb.s_xy; D.pairs = sb.pairs; D.blk_first = sb.blk_first;
    st.F = F; st.cap = cap; st.max_pairs = max_pairs; st.total = total; st.opts = *o; memcpy(st.K, K, sizeof(st.K));
    return VO_OK;
}

// K and every option but the snapshot's are those the stream was started with
static bool slam_stream_same_setup(const SlamStream& st, const double* K, const vo_slam_opts* o)
{
    const vo_slam_opts& a = st.opts;
    return memcmp(K, st.K, sizeof(st.K)) == 0 && o->pnp_iterations == a.pnp_iterations && o->reproj_err == a.reproj_err && o->confidence == a.confidence &&
           o->seed == a.seed && o->max_point_norm == a.max_point_norm && o->ba_iterations == a.ba_iterations && o->huber_delta == a.huber_delta &&
           o->free_cameras == a.free_cameras && o->filter_threshold == a.filter_threshold && o->max_cameras == a.max_cameras;
}

// The walk of vo_slam_stream and vo_slam_stream_restart.  restart: vo_slam_chains_restart's step for the one chain of the stream —
// k_chain_gather / k_chain_pose decide (cb.rs is set), k_slam_restart_stream joins every step, step 0 of the stream is an initial
// step like any other — and the alive flag and the segment state words stay on the device between the calls.  Without it the
// stream carries vo_slam_stream's launches and nothing else.
static int slam_stream_run(vo_ctx* ctx, bool restart, int resume, int total_pairs, int B, const double* K, const vo_slam_opts* o, double* poses_pnp, double* poses,
                           int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                           double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                           int32_t* n_carried, int32_t* carried_frame, double* carried_poses,
                           int32_t* segment, int32_t* cause, double* seg_poses_pnp, double* seg_poses)
{
    if (!ctx) return VO_ERR_INVALID;
    const char* who = restart ? "vo_slam_stream_restart" : "vo_slam_stream";
    if (!resume) drop_slam_stream(ctx);
    forget_slam_maps(ctx);
    if (!K || !o || !poses_pnp || !poses || !n_corr || !n_inl || !status || !n_pts || !n_obs || !n_cam || !chi2 || !ba_iterations_run || !ba_trials_run ||
        !n_carried || !carried_frame || !carried_poses) FAIL(VO_ERR_INVALID, "bad arguments");
    if (restart && (!segment || !cause || !seg_poses_pnp || !seg_poses)) FAIL(VO_ERR_INVALID, "bad arguments");
    SlamStream& st = ctx->stream_map;
    if (resume) {
        if (!st.live) FAIL(VO_ERR_INVALID, "%s: there is no stream to continue (none was started, or a configure or vo_slam_chain* call dropped it)", who);
        if (st.multi) FAIL(VO_ERR_INVALID, "%s: the stream was started by vo_slam_streams and is continued only by it", who);
        if (st.restart != restart)
            FAIL(VO_ERR_INVALID, "%s: the stream was started by %s and is continued only by it", who, st.restart ? "vo_slam_stream_restart" : "vo_slam_stream");
        if (st.lost && !restart) FAIL(VO_ERR_INVALID, "vo_slam_stream: the stream's last call ended with a pair that was not localised; it cannot be continued");
        if (st.touched) FAIL(VO_ERR_INVALID, "%s: slot %d, the stream's last frame, was uploaded to or detected again", who, st.anchor);
        if (st.stats != (ctx->slam_stats != 0)) FAIL(VO_ERR_INVALID, "%s: the stream was started with statistics %s (vo_set_slam_stats) and is continued only so", who, st.stats ? "on" : "off");
    }
    int F, cap;
    int rc = chain_check(ctx, B, who, &F, &cap); if (rc) return rc;
    rc = slam_opts_check(ctx, o, K, B, who); if (rc) return rc;
    const int32_t* sl = ctx->last.slots.data();
    if (resume) {
        if (sl[0] != st.anchor) FAIL(VO_ERR_INVALID, "%s: pair 0 starts at slot %d, the stream's last frame is in slot %d", who, sl[0], st.anchor);
        if (!slam_stream_same_setup(st, K, o)) FAIL(VO_ERR_INVALID, "%s: K and every option but the snapshot's must be those the stream was started with", who);
        if ((int64_t)st.done + B > st.total) FAIL(VO_ERR_INVALID, "%s: %d + %d pairs pass the stream's total_pairs = %d", who, st.done, B, st.total);
    } else if (total_pairs < B) FAIL(VO_ERR_INVALID, "%s: total_pairs = %d is less than the call's %d pairs", who, total_pairs, B);
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (!resume) {
        rc = slam_stream_allocate(ctx, st, restart, F, cap, batch(ctx).max_pairs, total_pairs, o, K);
        if (rc) { drop_slam_stream(ctx); return rc; }
        HIPCHK(hipMemsetAsync(st.base, 0, st.bytes, s));              // empty feature_mapper, empty map, no cameras, zero results
        HIPCHK(hipMemcpyAsync(st.dK, K, 72, hipMemcpyHostToDevice, s));
    } else HIPCHK(hipMemsetAsync(st.call_mem, 0, st.call_bytes, s));
    ChainBuf cb = st.cb; SlamBuf sb = st.sb;
    sb.st.frame0 = resume ? st.done : 0;
    // (after a call that ended lost the anchor frame is not in the map: every camera of the map is a carried one)
    sb.st.n_carried = !resume ? 0 : restart && st.lost ? st.last_ncam : st.last_ncam - 1;
    double* dK = st.dK;
    const BaParams prm{K[0], K[2], K[5], o->huber_delta, o->ba_iterations};
    const bool ba = o->ba_iterations > 0, filt = o->filter_threshold > 0;
    auto snapshot = [&](int p, int stage) {
        if (p == o->snapshot_pair && stage == o->snapshot_stage) (void)hipMemcpyAsync(st.snap_mem, st.map_mem, st.map_bytes, hipMemcpyDeviceToDevice, s);
    };
    st.live = false;                                                  // (until the call has come through)
    if (resume) {
        StageTimer t(ctx, ST_MISC);
        const int gn = F + (st.carries & 1);
        const SlamCarry carry{cap, F, st.anchor, gn, 2 * F + 1 - gn, st.keep};
        if (restart) launch_slam_carry_restart(s, carry, cb, sb);
        else launch_slam_carry(s, carry, cb, sb);
    }
    launch_chain_link(s, ctx->pb, cap, B, cb);
    for (int p = 0; p < B; p++) {
        {
            StageTimer t(ctx, ST_MISC);
            if (restart) {
                launch_chain_gather(s, ctx->pb, cap, p, F + 2, cb);
                if (p > 0 || resume) {
                    launch_pnp_ransac(s, cb.obj, cb.img, cb.off, 1, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                                      ctx->pnp_refine, cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus);
                    launch_chain_pose(s, ctx->pb, p, dK, cb);
                }
                launch_slam_restart_stream(s, ctx->pb, cap, p, cb, sb);
                if (p > 0 || resume) launch_chain_triangulate(s, ctx->pb, cap, p, cb);
            }
            else if (p == 0 && !resume) launch_chain_init(s, ctx->pb, cap, cb);
            else {
                launch_chain_gather(s, ctx->pb, cap, p, F + 2, cb);   // (a track may end in a ghost row: two more hops at most)
                launch_pnp_ransac(s, cb.obj, cb.img, cb.off, 1, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                                  ctx->pnp_refine, cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus);
                launch_chain_pose(s, ctx->pb, p, dK, cb);
                launch_chain_triangulate(s, ctx->pb, cap, p, cb);
            }
            if (restart) launch_slam_add_stream_restart(s, ctx->pb, cap, p, F + 2, o->max_point_norm, o->free_cameras, cb, sb);
            else launch_slam_add_stream(s, ctx->pb, cap, p, F + 2, o->max_point_norm, o->free_cameras, cb, sb);
        }
        snapshot(p, 1);
        if (ba) {
            { StageTimer t(ctx, ST_SLAM_PREPARE); launch_slam_ba_prepare(s, cb, sb); }
            BaBuf Dp = st.D;
            Dp.chi2 = st.dchi2 + 2 * p; Dp.iterations_run = st.dit + p; Dp.trials_run = st.dtr + p;
            { StageTimer t(ctx, ST_SLAM_BA); launch_bundle_adjust(s, Dp, prm, 1, o->free_cameras); }
        }
        snapshot(p, 2);
        const bool step0 = p == 0 && !resume;
        if (ba || (filt && !step0)) {
            StageTimer t(ctx, ST_SLAM_FILTER);
            if (restart) launch_slam_filter_stream_restart(s, ctx->pb, dK, step0 ? 0.0 : o->filter_threshold, cb, sb);
            else launch_slam_filter_stream(s, ctx->pb, dK, step0 ? 0.0 : o->filter_threshold, cb, sb);
        }
        snapshot(p, 3);
        {
            StageTimer t(ctx, ST_SLAM_LIMIT);
            if (restart) launch_slam_limit_stream_restart(s, p, o->max_cameras, cb, sb);
            else launch_slam_limit_stream(s, p, o->max_cameras, cb, sb);
        }
        snapshot(p, 4);
        if (st.stats) { StageTimer t(ctx, ST_SLAM_STATS); launch_slam_stats(s, p, sb, st.sbuf); }
    }
    HIPCHK(hipGetLastError());
    // the anchor camera of the next call: this call's last rows
    HIPCHK(hipMemcpyAsync(st.keep, cb.poses + (size_t)B * 12, 96, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(st.keep + 12, sb.poses_last + (size_t)B * 12, 96, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(poses_pnp, cb.poses, (size_t)(B + 1) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(poses, sb.poses_last, (size_t)(B + 1) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_corr, cb.n_corr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, cb.n_inl, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, cb.status, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_pts, sb.n_pts, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_obs, sb.n_obs, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_cam, sb.n_cam, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(chi2, st.dchi2, (size_t)B * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ba_iterations_run, st.dit, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ba_trials_run, st.dtr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    *n_carried = sb.st.n_carried;
    if (sb.st.n_carried > 0) {
        HIPCHK(hipMemcpyAsync(carried_frame, sb.st.carried_frame, (size_t)sb.st.n_carried * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(carried_poses, sb.st.carried_poses, (size_t)sb.st.n_carried * 96, hipMemcpyDeviceToHost, s));
    }
    int alive = 1;
    if (restart) {
        HIPCHK(hipMemcpyAsync(segment, cb.rs.segment, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cause, cb.rs.cause, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(seg_poses_pnp, cb.rs.seg_poses, (size_t)B * 96, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(seg_poses, cb.rs.seg_poses_last, (size_t)B * 96, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&alive, cb.alive, 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    rc = slam_map_download(ctx, sb.m, cap, &ctx->last.map[0]); if (rc) return rc;
    if (o->snapshot_pair >= 0) { rc = slam_map_download(ctx, st.snap, cap, &ctx->last.map[1]); if (rc) return rc; }
    if (st.stats) { rc = slam_stats_download(ctx, st.sbuf, {0, B}); if (rc) return rc; }
    // (a restart stream is lost when the device says so: a pair that fails and a pair that restarts can share a call)
    st.lost = restart && !alive;
    for (int p = 0; p < B && !restart; p++) if (status[p] != VO_OK) st.lost = true;
    st.anchor = sl[2 * B - 1]; st.done = (resume ? st.done : 0) + B; st.carries = resume ? st.carries + 1 : 0;
    st.last_ncam = n_cam[B - 1]; st.touched = false; st.live = true;
    return VO_OK;
}

extern "C" int vo_slam_stream(vo_ctx* ctx, int resume, int total_pairs, int B, const double* K, const vo_slam_opts* o, double* poses_pnp, double* poses,
                              int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                              double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                              int32_t* n_carried, int32_t* carried_frame, double* carried_poses)
{
    return slam_stream_run(ctx, false, resume, total_pairs, B, K, o, poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2, ba_iterations_run,
                           ba_trials_run, n_carried, carried_frame, carried_poses, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int vo_slam_stream_restart(vo_ctx* ctx, int resume, int total_pairs, int B, const double* K, const vo_slam_opts* o, double* poses_pnp, double* poses,
                                      int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs, int32_t* n_cam,
                                      double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                                      int32_t* n_carried, int32_t* carried_frame, double* carried_poses,
                                      int32_t* segment, int32_t* cause, double* seg_poses_pnp, double* seg_poses)
{
    return slam_stream_run(ctx, true, resume, total_pairs, B, K, o, poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2, ba_iterations_run,
                           ba_trials_run, n_carried, carried_frame, carried_poses, segment, cause, seg_poses_pnp, seg_poses);
}

// ------------------------------------------------------------------ the map step for S independent sequences in one call
// vo_slam_chain's walk, every kernel of a step launched once with the sequence on a grid axis (k_*_seqs): the host loop runs over
// the step j = 0 .. max B_s - 1, a workgroup does step j of its own sequence on pair seq_off[s] + j.  The slot-keyed tables are
// shared (the sequences' slots are disjoint: checked here); every list is carved once for all sequences and a sequence owns the
// range its capacities give it — cameras max_cameras + 1, points (B_s + 1) kp_cap, observations 2 B_s kp_cap — so k_bundle_adjust
// runs the S problems through BaProblem's offsets unchanged and the scratch grows with B, not with S * B.
static int chains_check(vo_ctx* ctx, int S, const int32_t* seq_off, int* F_out, int* cap_out)
{
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (S < 1) FAIL(VO_ERR_INVALID, "vo_slam_chains takes at least one sequence, got %d", S);
    if (seq_off[0] != 0) FAIL(VO_ERR_INVALID, "seq_off[0] must be 0, got %d", seq_off[0]);
    for (int s = 0; s < S; s++)
        if (seq_off[s + 1] <= seq_off[s]) FAIL(VO_ERR_INVALID, "seq_off must be strictly increasing: sequence %d has %d pairs", s, seq_off[s + 1] - seq_off[s]);
    if (ctx->last.pairs < 1 || seq_off[S] != ctx->last.pairs)
        FAIL(VO_ERR_INVALID, "vo_slam_chains takes all %d pairs of the most recent vo_pairs_run, seq_off ends at %d", ctx->last.pairs, seq_off[S]);
    if (!ctx->last.points) FAIL(VO_ERR_INVALID, "the most recent vo_pairs_run did not triangulate (want_points)");
    const int F = b.max_frames, cap = b.kp_cap, B = seq_off[S];
    const int32_t* sl = ctx->last.slots.data();
    for (int i = 0; i < 2 * B; i++)
        if (sl[i] < 0 || sl[i] >= F) FAIL(VO_ERR_INVALID, "pair slot %d of the most recent vo_pairs_run is out of range", sl[i]);
    std::vector<int> owner((size_t)F, -1);                  // the sequence a slot's frame belongs to
    for (int s = 0; s < S; s++)
        for (int p = seq_off[s]; p < seq_off[s + 1]; p++) {
            const bool head = p == seq_off[s];
            const int a = sl[2 * p], c = sl[2 * p + 1];
            const int other = head && owner[(size_t)a] >= 0 ? owner[(size_t)a] : owner[(size_t)c];
            if (other >= 0 && other != s)
                FAIL(VO_ERR_INVALID, "sequences %d and %d share a frame slot (pair %d (%d, %d)): a frame two sequences share is uploaded into two slots", other, s, p, a, c);
            if ((!head && a != sl[2 * p - 1]) || (head && a == c) || owner[(size_t)c] == s)
                FAIL(VO_ERR_INVALID, "pair %d (%d, %d) does not continue sequence %d as a chain of distinct frames", p, a, c, s);
            owner[(size_t)a] = s; owner[(size_t)c] = s;
        }
    if (F >= (1 << 20) || cap >= (1 << 20)) FAIL(VO_ERR_INVALID, "too many frames or keypoints for the packed track table");
    *F_out = F; *cap_out = cap;
    return VO_OK;
}

// The walk of vo_slam_chains and vo_slam_chains_restart.  restart: a sequence that loses tracking starts a new map from the next
// usable pair, decided on the device (k_chain_gather, k_chain_pose) and done by k_slam_restart_seqs, which joins every step;
// step 0 is then an initial step like any other (k_chain_gather meets a sequence that has no map yet).  Without it the stream
// carries vo_slam_chains' launches and nothing else.
static int slam_chains_run(vo_ctx* ctx, bool restart, int S, const int32_t* seq_off, const double* K, const vo_slam_opts* o, int snapshot_seq,
                           double* poses_pnp, double* poses, int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs,
                           int32_t* n_cam, double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                           int32_t* segment, int32_t* cause, double* seg_poses_pnp, double* seg_poses)
{
    if (!ctx) return VO_ERR_INVALID;
    drop_slam_stream(ctx);
    forget_slam_maps(ctx);
    if (!seq_off || !K || !o || !poses_pnp || !poses || !n_corr || !n_inl || !status || !n_pts || !n_obs || !n_cam || !chi2 || !ba_iterations_run || !ba_trials_run)
        FAIL(VO_ERR_INVALID, "bad arguments");
    if (restart && (!segment || !cause || !seg_poses_pnp || !seg_poses)) FAIL(VO_ERR_INVALID, "bad arguments");
    int F, cap;
    int rc = chains_check(ctx, S, seq_off, &F, &cap); if (rc) return rc;
    const bool snap_on = o->snapshot_pair >= 0;        // (snapshot_seq is ignored otherwise)
    if (snap_on && (snapshot_seq < 0 || snapshot_seq >= S)) FAIL(VO_ERR_INVALID, "snapshot_seq must be a sequence of the call (0 .. %d), got %d", S - 1, snapshot_seq);
    const int ss = snap_on ? snapshot_seq : 0;
    const int B = seq_off[S], Bss = seq_off[ss + 1] - seq_off[ss];
    rc = slam_opts_check(ctx, o, K, Bss, "vo_slam_chains"); if (rc) return rc;
    int maxB = 0;
    for (int q = 0; q < S; q++) maxB = std::max(maxB, seq_off[q + 1] - seq_off[q]);
    const size_t fc = (size_t)F * cap;
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    // capacities from the configuration: a pair adds at most one point and two observations per match
    const size_t cm = (size_t)o->max_cameras + 1, NC = cm * S, NP = (size_t)(B + S) * cap, NO = (size_t)2 * B * cap;
    const int nblk = o->free_cameras * (o->free_cameras + 1) / 2;
    std::vector<size_t> pair0((size_t)S + 1, 0);
    for (int q = 0; q < S; q++) pair0[q + 1] = pair0[q] + (size_t)2 * (seq_off[q + 1] - seq_off[q]) * cap * (o->free_cameras + 1) / 2;
    const size_t NPAIR = pair0[S];
    if (NP >= ((size_t)1 << 31) || NPAIR >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the maps' lists would not fit 32-bit indices");
    ChainBuf cb{}; SlamBuf sb{}; BaBuf D{}; SlamMap snap{}; double* dK; uint8_t* snap_mem; SlamSeq* dseq;
    const size_t snap_np = (size_t)(Bss + 1) * cap, snap_no = (size_t)2 * Bss * cap;
    ScratchLayout sc;
    // shared, keyed by slot
    sc.take(&cb.parent, fc); sc.take(&cb.map_pt, fc * 3); sc.take(&cb.cam, (size_t)F * 12); sc.take(&cb.in_map, fc); sc.take(&cb.cam_ok, F); sc.take(&sb.pt_of, fc);
    sc.take(&dK, 9);
    // per sequence: the current problem and the step's state
    sc.take(&cb.obj, (size_t)S * cap * 3); sc.take(&cb.img, (size_t)S * cap * 2); sc.take(&cb.Xw, (size_t)S * cap * 4); sc.take(&cb.pmask, (size_t)S * cap);
    sc.take(&sb.dec, (size_t)S * cap); sc.take(&cb.off, (size_t)2 * S); sc.take(&cb.rvec, (size_t)3 * S); sc.take(&cb.tvec, (size_t)3 * S);
    sc.take(&cb.pninl, S); sc.take(&cb.pstatus, S); sc.take(&cb.P1, (size_t)12 * S); sc.take(&cb.P2, (size_t)12 * S); sc.take(&cb.alive, S); sc.take(&cb.map_count, S);
    // per pair, in the run's order; sequence s owns the pose rows seq_off[s] + s .. seq_off[s + 1] + s
    sc.take(&cb.poses, (size_t)(B + S) * 12); sc.take(&sb.poses_last, (size_t)(B + S) * 12);
    sc.take(&cb.n_corr, B); sc.take(&cb.n_inl, B); sc.take(&cb.status, B); sc.take(&cb.n_map, B); sc.take(&sb.n_pts, B); sc.take(&sb.n_obs, B); sc.take(&sb.n_cam, B);
    // the maps' lists and the bundle adjustment's, each carved once: a sequence's range starts at its BaProblem offsets
    sc.take(&sb.m.cnt, (size_t)4 * S); sc.take(&sb.m.cam_frame, NC); sc.take(&sb.m.cam_pose, NC * 12); sc.take(&sb.m.cam_fixed, NC);
    sc.take(&sb.m.pt_key, NP); sc.take(&sb.m.pt_xyz, NP * 3); sc.take(&sb.m.obs_cam, NO); sc.take(&sb.m.obs_pt, NO); sc.take(&sb.m.obs_xy, NO * 2);
    sc.take(&sb.tmp, NP); sc.take(&sb.idx, NO); sc.take(&sb.prob, S); sc.take(&sb.cam_col, NC); sc.take(&sb.pt_first, NP + S);
    sc.take(&sb.s_cam, NO); sc.take(&sb.s_pt, NO); sc.take(&sb.s_xy, NO * 2); sc.take(&sb.pairs, NPAIR); sc.take(&sb.blk_first, (size_t)S * (nblk + 1));
    sc.take(&D.X2, NP * 3); sc.take(&D.W, NO * 18); sc.take(&D.Hpp, NP * 6); sc.take(&D.bp, NP * 3); sc.take(&D.Hpi, NP * 6);
    // k_bundle_adjust writes problem s of step j at [j][s]
    double* dchi2; int *dit, *dtr;
    sc.take(&dchi2, (size_t)2 * maxB * S); sc.take(&dit, (size_t)maxB * S); sc.take(&dtr, (size_t)maxB * S);
    sc.take(&snap_mem, snap_on ? slam_map_carve(nullptr, cm, snap_np, snap_no, &snap) : 0);
    sc.take(&dseq, S);
    sc.take(&cb.rs.st, restart ? (size_t)4 * S : 0); sc.take(&cb.rs.segment, restart ? B : 0); sc.take(&cb.rs.cause, restart ? B : 0);
    sc.take(&cb.rs.seg_poses, restart ? (size_t)B * 12 : 0); sc.take(&cb.rs.seg_poses_last, restart ? (size_t)B * 12 : 0);
    const bool stats_on = ctx->slam_stats != 0;
    StatsBuf stats{};
    slam_stats_take_scratch(sc, stats, stats_on, NP, NO); slam_stats_take_rows(sc, stats, stats_on, B, cm);
    rc = sc.place(ctx); if (rc) return rc;
    stats.Kd = dK;
    if (!restart) cb.rs = RestartBuf{};
    if (snap_on) slam_map_carve(snap_mem, cm, snap_np, snap_no, &snap);
    D.prob = sb.prob; D.poses = sb.m.cam_pose; D.cam_col = sb.cam_col; D.X = sb.m.pt_xyz; D.pt_first = sb.pt_first;
    D.obs_cam = sb.s_cam; D.obs_pt = sb.s_pt; D.obs_xy = sb.s_xy; D.pairs = sb.pairs; D.blk_first = sb.blk_first;
    std::vector<SlamSeq> seq((size_t)S);
    for (int q = 0; q < S; q++) {
        const int first = seq_off[q], Bq = seq_off[q + 1] - first;
        SlamSeq& e = seq[(size_t)q];
        e.first = first; e.count = Bq;
        BaProblem at{};
        at.cam0 = (int)(cm * q); at.pt0 = (int)((size_t)(first + q) * cap); at.obs0 = (int)((size_t)2 * first * cap); at.pair0 = (int)pair0[q]; at.blk0 = q * (nblk + 1);
        ChainBuf& c = e.cb; c = cb;
        c.obj0 = q * cap;                                    // k_pnp_ransac indexes the whole arrays by the sequence's {first, end}
        c.off += 2 * q; c.rvec += 3 * q; c.tvec += 3 * q; c.pmask += (size_t)q * cap; c.pninl += q; c.pstatus += q; c.P1 += 12 * q; c.P2 += 12 * q;
        c.obj += (size_t)q * cap * 3; c.img += (size_t)q * cap * 2; c.Xw += (size_t)q * cap * 4; c.alive += q; c.map_count += q;
        c.n_corr += first; c.n_inl += first; c.status += first; c.n_map += first; c.poses += (size_t)(first + q) * 12;
        if (restart) { c.rs.st += 4 * q; c.rs.segment += first; c.rs.cause += first; c.rs.seg_poses += (size_t)first * 12; c.rs.seg_poses_last += (size_t)first * 12; }
        SlamBuf& m = e.sb; m = sb;
        m.base = at;
        m.cam_cap = (int)cm; m.pt_cap = (Bq + 1) * cap; m.obs_cap = 2 * Bq * cap; m.pair_cap = (int)(pair0[q + 1] - pair0[q]);
        m.m.cnt += 4 * q; m.m.cam_frame += at.cam0; m.m.cam_pose += (size_t)at.cam0 * 12; m.m.cam_fixed += at.cam0;
        m.m.pt_key += at.pt0; m.m.pt_xyz += (size_t)at.pt0 * 3; m.m.obs_cam += at.obs0; m.m.obs_pt += at.obs0; m.m.obs_xy += (size_t)at.obs0 * 2;
        m.dec += (size_t)q * cap; m.tmp += at.pt0; m.idx += at.obs0; m.n_pts += first; m.n_obs += first; m.n_cam += first; m.poses_last += (size_t)(first + q) * 12;
        m.prob += q; m.cam_col += at.cam0; m.pt_first += at.pt0 + q; m.s_cam += at.obs0; m.s_pt += at.obs0; m.s_xy += (size_t)at.obs0 * 2;
        m.pairs += at.pair0; m.blk_first += at.blk0;
    }
    HIPCHK(hipMemsetAsync(ctx->scratch.p, 0, sc.bytes, s));          // empty feature_mapper, empty maps, no cameras, zero results
    HIPCHK(hipMemcpyAsync(dK, K, 72, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dseq, seq.data(), (size_t)S * sizeof(SlamSeq), hipMemcpyHostToDevice, s));
    const BaParams prm{K[0], K[2], K[5], o->huber_delta, o->ba_iterations};
    const bool ba = o->ba_iterations > 0, filt = o->filter_threshold > 0;
    const SlamMap live = seq[(size_t)ss].sb.m;
    auto snapshot = [&](int j, int stage) {                          // the sequence's ranges of the lists: a few device-to-device copies
        if (!snap_on || j != o->snapshot_pair || stage != o->snapshot_stage) return;
        auto cp = [&](auto* dst, const auto* src, size_t n) { (void)hipMemcpyAsync(dst, src, n * sizeof(*src), hipMemcpyDeviceToDevice, s); };
        cp(snap.cnt, live.cnt, 4); cp(snap.cam_frame, live.cam_frame, cm); cp(snap.cam_pose, live.cam_pose, cm * 12); cp(snap.cam_fixed, live.cam_fixed, cm);
        cp(snap.pt_key, live.pt_key, snap_np); cp(snap.pt_xyz, live.pt_xyz, snap_np * 3);
        cp(snap.obs_cam, live.obs_cam, snap_no); cp(snap.obs_pt, live.obs_pt, snap_no); cp(snap.obs_xy, live.obs_xy, snap_no * 2);
    };
    launch_chain_link(s, ctx->pb, cap, B, cb);
    for (int j = 0; j < maxB; j++) {
        {
            StageTimer t(ctx, ST_MISC);
            if (restart) {
                launch_chain_gather_seqs(s, ctx->pb, cap, j, F, dseq, S);
                if (j > 0) {
                    launch_pnp_ransac(s, cb.obj, cb.img, cb.off, S, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                                      ctx->pnp_refine, cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus, 2);
                    launch_chain_pose_seqs(s, ctx->pb, j, dK, dseq, S);
                }
                launch_slam_restart_seqs(s, ctx->pb, cap, j, dseq, S);
                if (j > 0) launch_chain_triangulate_seqs(s, ctx->pb, cap, j, dseq, S);
            }
            else if (j == 0) launch_chain_init_seqs(s, ctx->pb, cap, dseq, S);
            else {
                launch_chain_gather_seqs(s, ctx->pb, cap, j, F, dseq, S);
                launch_pnp_ransac(s, cb.obj, cb.img, cb.off, S, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                                  ctx->pnp_refine, cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus, 2);
                launch_chain_pose_seqs(s, ctx->pb, j, dK, dseq, S);
                launch_chain_triangulate_seqs(s, ctx->pb, cap, j, dseq, S);
            }
            launch_slam_add_seqs(s, ctx->pb, cap, j, F, o->max_point_norm, o->free_cameras, dseq, S);
        }
        snapshot(j, 1);
        if (ba) {
            { StageTimer t(ctx, ST_SLAM_PREPARE); launch_slam_ba_prepare_seqs(s, j, dseq, S); }
            BaBuf Dj = D;
            Dj.chi2 = dchi2 + (size_t)2 * j * S; Dj.iterations_run = dit + (size_t)j * S; Dj.trials_run = dtr + (size_t)j * S;
            { StageTimer t(ctx, ST_SLAM_BA); launch_bundle_adjust(s, Dj, prm, S, o->free_cameras); }
        }
        snapshot(j, 2);
        // step 0 ends with optimize_map (:90); what it wrote back still has to reach the tables the next pair reads
        if (ba || (filt && j > 0)) { StageTimer t(ctx, ST_SLAM_FILTER); launch_slam_filter_seqs(s, ctx->pb, cap, j, dK, j > 0 ? o->filter_threshold : 0.0, dseq, S); }
        snapshot(j, 3);
        { StageTimer t(ctx, ST_SLAM_LIMIT); launch_slam_limit_seqs(s, j, o->max_cameras, dseq, S); }
        snapshot(j, 4);
        if (stats_on) { StageTimer t(ctx, ST_SLAM_STATS); launch_slam_stats_seqs(s, j, dseq, S, stats); }
    }
    HIPCHK(hipGetLastError());
    std::vector<double> hchi((size_t)2 * maxB * S); std::vector<int32_t> hit((size_t)maxB * S), htr((size_t)maxB * S);
    HIPCHK(hipMemcpyAsync(poses_pnp, cb.poses, (size_t)(B + S) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(poses, sb.poses_last, (size_t)(B + S) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_corr, cb.n_corr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, cb.n_inl, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, cb.status, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_pts, sb.n_pts, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_obs, sb.n_obs, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_cam, sb.n_cam, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hchi.data(), dchi2, hchi.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hit.data(), dit, hit.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(htr.data(), dtr, htr.size() * 4, hipMemcpyDeviceToHost, s));
    if (restart) {
        HIPCHK(hipMemcpyAsync(segment, cb.rs.segment, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cause, cb.rs.cause, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(seg_poses_pnp, cb.rs.seg_poses, (size_t)B * 96, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(seg_poses, cb.rs.seg_poses_last, (size_t)B * 96, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    for (int q = 0; q < S; q++)                                       // [step][sequence] -> the pair's position in the run
        for (int j = 0; j < seq_off[q + 1] - seq_off[q]; j++) {
            const size_t at = (size_t)j * S + q, p = (size_t)seq_off[q] + j;
            chi2[2 * p] = hchi[2 * at]; chi2[2 * p + 1] = hchi[2 * at + 1]; ba_iterations_run[p] = hit[at]; ba_trials_run[p] = htr[at];
        }
    // the scratch buffer belongs to the next call: the maps are kept as host copies
    std::vector<LastRun::Map> maps((size_t)S);
    for (int q = 0; q < S; q++) { rc = slam_map_download(ctx, seq[(size_t)q].sb.m, cap, &maps[(size_t)q], seq_off[q], seq_off[q + 1] - seq_off[q]); if (rc) return rc; }
    LastRun::Map smap;
    if (snap_on) { rc = slam_map_download(ctx, snap, cap, &smap, seq_off[ss], Bss); if (rc) return rc; }
    ctx->last.map[0] = maps[0];                                       // what vo_slam_map reports: sequence 0, and its snapshot if it has one
    if (snap_on && ss == 0) ctx->last.map[1] = smap;
    ctx->last.seq_map = std::move(maps);
    if (snap_on) { ctx->last.snap_map = std::move(smap); ctx->last.snap_seq = ss; }
    if (stats_on) { rc = slam_stats_download(ctx, stats, std::vector<int32_t>(seq_off, seq_off + S + 1)); if (rc) return rc; }
    return VO_OK;
}

extern "C" int vo_slam_chains(vo_ctx* ctx, int S, const int32_t* seq_off, const double* K, const vo_slam_opts* o, int snapshot_seq,
                              double* poses_pnp, double* poses, int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs,
                              int32_t* n_cam, double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run)
{
    return slam_chains_run(ctx, false, S, seq_off, K, o, snapshot_seq, poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2,
                           ba_iterations_run, ba_trials_run, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int vo_slam_chains_restart(vo_ctx* ctx, int S, const int32_t* seq_off, const double* K, const vo_slam_opts* o, int snapshot_seq,
                                      double* poses_pnp, double* poses, int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts, int32_t* n_obs,
                                      int32_t* n_cam, double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                                      int32_t* segment, int32_t* cause, double* seg_poses_pnp, double* seg_poses)
{
    return slam_chains_run(ctx, true, S, seq_off, K, o, snapshot_seq, poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2,
                           ba_iterations_run, ba_trials_run, segment, cause, seg_poses_pnp, seg_poses);
}

// ------------------------------------------------------------------ S restart streams in one call, carried from call to call
// vo_slam_stream_restart's walk with vo_slam_chains_restart's layout: the slot-keyed tables are shared (disjoint slots, and two ghost
// rows per sequence behind them), every list is carved once for all sequences — a sequence owns the range total_pairs[s] gives it —
// and the per-pair outputs are laid out per call by seq_off.  One allocation with the stream's lifetime (SlamStream).
static int slam_streams_allocate(vo_ctx* ctx, SlamStream& st, int S, int F, int cap, int max_pairs, const int32_t* total, const vo_slam_opts* o, const double* K)
{
    const size_t R = (size_t)F + 2 * (size_t)S, fc = R * cap, cm = (size_t)o->max_cameras + 1, NC = cm * S, P = (size_t)max_pairs;
    const int nblk = o->free_cameras * (o->free_cameras + 1) / 2;
    if (R >= ((size_t)1 << 20)) FAIL(VO_ERR_INVALID, "vo_slam_streams: max_frames + 2 S = %zu rows are too many for the packed track table", R);
    std::vector<size_t> pt0((size_t)S + 1, 0), ob0((size_t)S + 1, 0), pr0((size_t)S + 1, 0);
    st.seq.assign((size_t)S, SlamStream::Seq());
    st.rows.assign((size_t)S * (P + 1), 0);
    st.snap_np = 0; st.snap_no = 0;
    for (int q = 0; q < S; q++) {
        SlamStream::Seq& e = st.seq[(size_t)q];
        e.total = total[q]; e.capacity = total[q];
        e.np = ((size_t)total[q] + 1) * cap; e.no = (size_t)2 * cap * std::min(cm, (size_t)total[q]);
        pt0[q + 1] = pt0[q] + e.np; ob0[q + 1] = ob0[q] + e.no; pr0[q + 1] = pr0[q] + e.no * (o->free_cameras + 1) / 2;
        st.snap_np = std::max(st.snap_np, e.np); st.snap_no = std::max(st.snap_no, e.no);
    }
    const size_t NP = pt0[S], NO = ob0[S], NPAIR = pr0[S];
    if (NP >= ((size_t)1 << 31) || NPAIR >= ((size_t)1 << 31) || fc >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the maps' lists would not fit 32-bit indices");
    ChainBuf& cb = st.cb; SlamBuf& sb = st.sb; BaBuf& D = st.D; SlamMap& snap = st.snap;
    ScratchLayout sc;
    // shared, keyed by slot (and ghost row)
    sc.take(&cb.parent, fc); sc.take(&cb.map_pt, fc * 3); sc.take(&cb.cam, (size_t)F * 12); sc.take(&cb.in_map, fc); sc.take(&cb.cam_ok, F); sc.take(&sb.pt_of, fc);
    sc.take(&st.dK, 9);
    // per sequence: the current problem, the step's state, and what outlives a call — alive, the segment state words, the anchor camera
    sc.take(&cb.obj, (size_t)S * cap * 3); sc.take(&cb.img, (size_t)S * cap * 2); sc.take(&cb.Xw, (size_t)S * cap * 4); sc.take(&cb.pmask, (size_t)S * cap);
    sc.take(&sb.dec, (size_t)S * cap); sc.take(&cb.off, (size_t)2 * S); sc.take(&cb.rvec, (size_t)3 * S); sc.take(&cb.tvec, (size_t)3 * S);
    sc.take(&cb.pninl, S); sc.take(&cb.pstatus, S); sc.take(&cb.P1, (size_t)12 * S); sc.take(&cb.P2, (size_t)12 * S); sc.take(&cb.alive, S); sc.take(&cb.map_count, S);
    sc.take(&cb.rs.st, (size_t)4 * S); sc.take(&st.keep, (size_t)24 * S);
    // the maps' lists and the bundle adjustment's, each carved once: a sequence's range starts at its BaProblem offsets
    sc.take(&sb.m.cnt, (size_t)4 * S); sc.take(&sb.m.cam_frame, NC); sc.take(&sb.m.cam_pose, NC * 12); sc.take(&sb.m.cam_fixed, NC);
    sc.take(&sb.m.pt_key, NP); sc.take(&sb.m.pt_xyz, NP * 3); sc.take(&sb.m.pt_feat, NP * 2);
    sc.take(&sb.m.obs_cam, NO); sc.take(&sb.m.obs_pt, NO); sc.take(&sb.m.obs_xy, NO * 2);
    sc.take(&sb.tmp, NP); sc.take(&sb.idx, NO); sc.take(&sb.prob, S); sc.take(&sb.cam_col, NC); sc.take(&sb.pt_first, NP + S);
    sc.take(&sb.s_cam, NO); sc.take(&sb.s_pt, NO); sc.take(&sb.s_xy, NO * 2); sc.take(&sb.pairs, NPAIR); sc.take(&sb.blk_first, (size_t)S * (nblk + 1));
    sc.take(&D.X2, NP * 3); sc.take(&D.W, NO * 18); sc.take(&D.Hpp, NP * 6); sc.take(&D.bp, NP * 3); sc.take(&D.Hpi, NP * 6);
    // the snapshot: room for the largest sequence
    sc.take(&snap.cnt, 4); sc.take(&snap.cam_frame, cm); sc.take(&snap.cam_pose, cm * 12); sc.take(&snap.cam_fixed, cm);
    sc.take(&snap.pt_key, st.snap_np); sc.take(&snap.pt_xyz, st.snap_np * 3); sc.take(&snap.pt_feat, st.snap_np * 2);
    sc.take(&snap.obs_cam, st.snap_no); sc.take(&snap.obs_pt, st.snap_no); sc.take(&snap.obs_xy, st.snap_no * 2);
    sc.take(&st.dseq, S); sc.take(&st.dcar, S); sc.take(&st.drows, (size_t)S * (P + 1)); sc.take(&st.dseat, S);
    st.stats = ctx->slam_stats != 0;
    slam_stats_take_scratch(sc, st.sbuf, st.stats, NP, NO);
    const size_t call0 = sc.bytes;                                    // from here on: what a call reports, sized for max_pairs pairs
    slam_stats_take_rows(sc, st.sbuf, st.stats, P, cm);
    sc.take(&cb.poses, (P + S) * 12); sc.take(&sb.poses_last, (P + S) * 12);
    sc.take(&cb.n_corr, P); sc.take(&cb.n_inl, P); sc.take(&cb.status, P); sc.take(&cb.n_map, P); sc.take(&sb.n_pts, P); sc.take(&sb.n_obs, P); sc.take(&sb.n_cam, P);
    sc.take(&st.dchi2, 2 * P * S); sc.take(&st.dit, P * S); sc.take(&st.dtr, P * S);       // k_bundle_adjust writes problem s of step j at [j][s]
    sc.take(&sb.st.carried_frame, NC); sc.take(&sb.st.carried_poses, NC * 12);
    sc.take(&cb.rs.segment, P); sc.take(&cb.rs.cause, P); sc.take(&cb.rs.seg_poses, P * 12); sc.take(&cb.rs.seg_poses_last, P * 12);
    HIPCHK(st.mem.alloc(&st.base, sc.bytes));
    sc.place_at(st.base);
    st.sbuf.Kd = st.dK;
    st.bytes = sc.bytes; st.call_mem = st.base + call0; st.call_bytes = sc.bytes - call0;
    D.prob = sb.prob; D.poses = sb.m.cam_pose; D.cam_col = sb.cam_col; D.X = sb.m.pt_xyz; D.pt_first = sb.pt_first;
    D.obs_cam = sb.s_cam; D.obs_pt = sb.s_pt; D.obs_xy = sb.s_xy; D.pairs = sb.pairs; D.blk_first = sb.blk_first;
    for (int q = 0; q < S; q++) {
        SlamStream::Seq& e = st.seq[(size_t)q];
        BaProblem at{};
        at.cam0 = (int)(cm * q); at.pt0 = (int)pt0[q]; at.obs0 = (int)ob0[q]; at.pair0 = (int)pr0[q]; at.blk0 = q * (nblk + 1);
        ChainBuf& c = e.at.cb; c = cb;
        c.obj0 = q * cap;                                    // k_pnp_ransac indexes the whole arrays by the sequence's {first, end}
        c.off += 2 * q; c.rvec += 3 * q; c.tvec += 3 * q; c.pmask += (size_t)q * cap; c.pninl += q; c.pstatus += q; c.P1 += 12 * q; c.P2 += 12 * q;
        c.obj += (size_t)q * cap * 3; c.img += (size_t)q * cap * 2; c.Xw += (size_t)q * cap * 4; c.alive += q; c.map_count += q; c.rs.st += 4 * q;
        SlamBuf& m = e.at.sb; m = sb;
        m.base = at;
        m.cam_cap = (int)cm; m.pt_cap = (int)e.np; m.obs_cap = (int)e.no; m.pair_cap = (int)(pr0[q + 1] - pr0[q]);
        m.m.cnt += 4 * q; m.m.cam_frame += at.cam0; m.m.cam_pose += (size_t)at.cam0 * 12; m.m.cam_fixed += at.cam0;
        m.m.pt_key += at.pt0; m.m.pt_xyz += (size_t)at.pt0 * 3; m.m.pt_feat += (size_t)at.pt0 * 2;
        m.m.obs_cam += at.obs0; m.m.obs_pt += at.obs0; m.m.obs_xy += (size_t)at.obs0 * 2;
        m.dec += (size_t)q * cap; m.tmp += at.pt0; m.idx += at.obs0;
        m.prob += q; m.cam_col += at.cam0; m.pt_first += at.pt0 + q; m.s_cam += at.obs0; m.s_pt += at.obs0; m.s_xy += (size_t)at.obs0 * 2;
        m.pairs += at.pair0; m.blk_first += at.blk0;
        m.st.carried_frame += at.cam0; m.st.carried_poses += (size_t)at.cam0 * 12;
    }
    st.restart = true; st.multi = true; st.S = S;
    st.F = F; st.cap = cap; st.max_pairs = max_pairs; st.opts = *o; memcpy(st.K, K, sizeof(st.K));
    return VO_OK;
}

// What vo_slam_streams asks of the most recent vo_pairs_run: vo_slam_chains' checks, and in a resumed call the stream's — a
// sequence may be idle, one that advances starts at its anchor slot, and no anchor slot is among another sequence's pairs.
static int streams_check(vo_ctx* ctx, int resume, int S, const int32_t* seq_off, int* F_out, int* cap_out)
{
    const SlamStream& st = ctx->stream_map;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (S < 1) FAIL(VO_ERR_INVALID, "vo_slam_streams takes at least one sequence, got %d", S);
    if (seq_off[0] != 0) FAIL(VO_ERR_INVALID, "seq_off[0] must be 0, got %d", seq_off[0]);
    for (int s = 0; s < S; s++) {
        const int n = seq_off[s + 1] - seq_off[s];
        if (n < 0 || (n == 0 && !resume))
            FAIL(VO_ERR_INVALID, "vo_slam_streams: sequence %d has %d pairs (a sequence may be idle, with none, only in a resumed call)", s, n);
    }
    if (seq_off[S] < 1) FAIL(VO_ERR_INVALID, "vo_slam_streams: every sequence is idle; at least one must advance");
    if (seq_off[S] != ctx->last.pairs)
        FAIL(VO_ERR_INVALID, "vo_slam_streams takes all %d pairs of the most recent vo_pairs_run, seq_off ends at %d", ctx->last.pairs, seq_off[S]);
    if (!ctx->last.points) FAIL(VO_ERR_INVALID, "the most recent vo_pairs_run did not triangulate (want_points)");
    const int F = b.max_frames, cap = b.kp_cap, B = seq_off[S];
    const int32_t* sl = ctx->last.slots.data();
    for (int i = 0; i < 2 * B; i++)
        if (sl[i] < 0 || sl[i] >= F) FAIL(VO_ERR_INVALID, "pair slot %d of the most recent vo_pairs_run is out of range", sl[i]);
    std::vector<int> owner((size_t)F, -1);                  // the sequence a slot's frame belongs to: first of all the anchors
    if (resume) for (int s = 0; s < S; s++) if (!st.seq[(size_t)s].vacant) owner[(size_t)st.seq[(size_t)s].anchor] = s;   // (a vacant seat has none)
    for (int s = 0; s < S; s++)
        for (int p = seq_off[s]; p < seq_off[s + 1]; p++) {
            const bool head = p == seq_off[s];
            const int a = sl[2 * p], c = sl[2 * p + 1];
            if (head && resume && !st.seq[(size_t)s].vacant) {
                const SlamStream::Seq& e = st.seq[(size_t)s];
                if (a != e.anchor) FAIL(VO_ERR_INVALID, "vo_slam_streams: pair 0 of sequence %d starts at slot %d, the sequence's last frame is in slot %d", s, a, e.anchor);
                if (e.touched) FAIL(VO_ERR_INVALID, "vo_slam_streams: slot %d, the last frame of sequence %d, was uploaded to or detected again", e.anchor, s);
            } else if (head) {                                  // a stream's pair 0, or a new flight's in a vacant seat: any slot nobody holds
                if (owner[(size_t)a] >= 0)
                    FAIL(VO_ERR_INVALID, "sequences %d and %d share a frame slot (pair %d (%d, %d)): a frame two sequences share is uploaded into two slots", owner[(size_t)a], s, p, a, c);
                owner[(size_t)a] = s;
            }
            if ((!head && a != sl[2 * p - 1]) || owner[(size_t)c] == s)
                FAIL(VO_ERR_INVALID, "pair %d (%d, %d) does not continue sequence %d as a chain of distinct frames", p, a, c, s);
            if (owner[(size_t)c] >= 0)
                FAIL(VO_ERR_INVALID, "sequences %d and %d share a frame slot (pair %d (%d, %d)): a frame two sequences share is uploaded into two slots", owner[(size_t)c], s, p, a, c);
            owner[(size_t)c] = s;
        }
    if (cap >= (1 << 20)) FAIL(VO_ERR_INVALID, "too many keypoints for the packed track table");
    *F_out = F; *cap_out = cap;
    return VO_OK;
}

extern "C" int vo_slam_streams(vo_ctx* ctx, int resume, int S, const int32_t* total_pairs, const int32_t* seq_off, const double* K, const vo_slam_opts* o,
                               int snapshot_seq, double* poses_pnp, double* poses, int32_t* n_corr, int32_t* n_inl, int32_t* status, int32_t* n_pts,
                               int32_t* n_obs, int32_t* n_cam, double* chi2, int32_t* ba_iterations_run, int32_t* ba_trials_run,
                               int32_t* segment, int32_t* cause, double* seg_poses_pnp, double* seg_poses,
                               int32_t* n_carried, int32_t* carried_frame, double* carried_poses)
{
    if (!ctx) return VO_ERR_INVALID;
    const char* who = "vo_slam_streams";
    if (!resume) drop_slam_stream(ctx);
    forget_slam_maps(ctx);
    if (!seq_off || !K || !o || !poses_pnp || !poses || !n_corr || !n_inl || !status || !n_pts || !n_obs || !n_cam || !chi2 || !ba_iterations_run || !ba_trials_run ||
        !segment || !cause || !seg_poses_pnp || !seg_poses || !n_carried || !carried_frame || !carried_poses || (!resume && !total_pairs))
        FAIL(VO_ERR_INVALID, "bad arguments");
    SlamStream& st = ctx->stream_map;
    if (resume) {
        if (!st.live) FAIL(VO_ERR_INVALID, "%s: there is no stream to continue (none was started, or a configure or vo_slam_chain* call dropped it)", who);
        if (!st.multi) FAIL(VO_ERR_INVALID, "%s: the stream was started by %s and is continued only by it", who, st.restart ? "vo_slam_stream_restart" : "vo_slam_stream");
        if (S != st.S) FAIL(VO_ERR_INVALID, "%s: the stream has %d sequences, the call names %d", who, st.S, S);
        if (st.stats != (ctx->slam_stats != 0)) FAIL(VO_ERR_INVALID, "%s: the stream was started with statistics %s (vo_set_slam_stats) and is continued only so", who, st.stats ? "on" : "off");
    }
    int F, cap;
    int rc = streams_check(ctx, resume, S, seq_off, &F, &cap); if (rc) return rc;
    const bool snap_on = o->snapshot_pair >= 0;        // (snapshot_seq is ignored otherwise)
    if (snap_on && (snapshot_seq < 0 || snapshot_seq >= S)) FAIL(VO_ERR_INVALID, "snapshot_seq must be a sequence of the call (0 .. %d), got %d", S - 1, snapshot_seq);
    const int ss = snap_on ? snapshot_seq : 0;
    const int B = seq_off[S];
    rc = slam_opts_check(ctx, o, K, snap_on ? seq_off[ss + 1] - seq_off[ss] : 1, who); if (rc) return rc;
    int maxB = 0;
    for (int q = 0; q < S; q++) {
        const int Bq = seq_off[q + 1] - seq_off[q];
        maxB = std::max(maxB, Bq);
        if (resume) {
            const SlamStream::Seq& e = st.seq[(size_t)q];
            if ((int64_t)e.done + Bq > e.total) FAIL(VO_ERR_INVALID, "%s: sequence %d: %d + %d pairs pass its total_pairs = %d", who, q, e.done, Bq, e.total);
        } else if (total_pairs[q] < Bq) FAIL(VO_ERR_INVALID, "%s: total_pairs[%d] = %d is less than the sequence's %d pairs in this call", who, q, total_pairs[q], Bq);
    }
    if (resume && !slam_stream_same_setup(st, K, o))
        FAIL(VO_ERR_INVALID, "%s: K and every option but the snapshot's must be those the stream was started with", who);
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const int max_pairs = batch(ctx).max_pairs;
    if (!resume) {
        rc = slam_streams_allocate(ctx, st, S, F, cap, max_pairs, total_pairs, o, K);
        if (rc) { drop_slam_stream(ctx); return rc; }
        HIPCHK(hipMemsetAsync(st.base, 0, st.bytes, s));              // empty feature_mapper, empty maps, no cameras, zero results
        HIPCHK(hipMemcpyAsync(st.dK, K, 72, hipMemcpyHostToDevice, s));
    } else HIPCHK(hipMemsetAsync(st.call_mem, 0, st.call_bytes, s));
    const ChainBuf& cb = st.cb; const SlamBuf& sb = st.sb;
    const size_t cm = (size_t)o->max_cameras + 1, row_cap = (size_t)max_pairs + 1;
    const int R = F + 2 * S, gpar = st.carries & 1;
    // the descriptors of this call: a sequence's ranges of the lists, and its rows of the call's outputs
    std::vector<SlamSeq> seq((size_t)S); std::vector<SlamSeqCarry> car((size_t)S); std::vector<int32_t> hrows(st.rows);
    std::vector<SlamSeat> seat((size_t)S);
    bool seats = false;                                               // some seat is vacant: the carry launch is the seats form
    for (int q = 0; q < S; q++) {
        const SlamStream::Seq& h = st.seq[(size_t)q];
        const int first = seq_off[q];
        SlamSeq& e = seq[(size_t)q]; e = h.at;
        e.first = first; e.count = seq_off[q + 1] - first;
        ChainBuf& c = e.cb;
        c.n_corr += first; c.n_inl += first; c.status += first; c.n_map += first; c.poses += (size_t)(first + q) * 12;
        c.rs.segment += first; c.rs.cause += first; c.rs.seg_poses += (size_t)first * 12; c.rs.seg_poses_last += (size_t)first * 12;
        SlamBuf& m = e.sb;
        m.n_pts += first; m.n_obs += first; m.n_cam += first; m.poses_last += (size_t)(first + q) * 12;
        m.st.frame0 = resume ? h.done : 0;
        // (after a call that ended lost the anchor frame is not in the map: every camera of the map is a carried one)
        m.st.n_carried = !resume ? 0 : h.lost ? h.last_ncam : h.last_ncam - 1;
        SlamSeqCarry& k = car[(size_t)q];
        const int gn = F + 2 * q + gpar, go = F + 2 * q + 1 - gpar;
        k.c = SlamCarry{cap, F, h.anchor, gn, go, st.keep + (size_t)24 * q};
        k.hops = R; k.rows = st.drows + (size_t)q * row_cap;
        hrows[(size_t)q * row_cap + h.n_rows] = go; k.n_rows = h.n_rows + 1;
        // seats: a vacant seat is not carried.  One replaced since the last call is reset — it gives up the slots of its last call's
        // frames (k.rows without the ghost row above), its old anchor row and both ghost rows; one already reset is left alone.
        SlamSeat& t = seat[(size_t)q];
        t = SlamSeat{SEAT_CARRY, 0, {0, 0, 0}, st.keep + (size_t)24 * q};
        if (resume && h.vacant) {
            seats = true;
            t.mode = h.clean ? SEAT_VACANT : SEAT_RESET;
            k.n_rows = h.n_rows;
            if (h.old_anchor >= 0) t.rows[t.n_rows++] = h.old_anchor;
            t.rows[t.n_rows++] = gn; t.rows[t.n_rows++] = go;
        }
    }
    HIPCHK(hipMemcpyAsync(st.dseq, seq.data(), (size_t)S * sizeof(SlamSeq), hipMemcpyHostToDevice, s));
    const BaParams prm{K[0], K[2], K[5], o->huber_delta, o->ba_iterations};
    const bool ba = o->ba_iterations > 0, filt = o->filter_threshold > 0;
    const SlamMap live = seq[(size_t)ss].sb.m, snap = st.snap;
    const size_t snap_np = st.seq[(size_t)ss].np, snap_no = st.seq[(size_t)ss].no;
    auto snapshot = [&](int j, int stage) {                          // the sequence's ranges of the lists: a few device-to-device copies
        if (!snap_on || j != o->snapshot_pair || stage != o->snapshot_stage) return;
        auto cp = [&](auto* dst, const auto* src, size_t n) { (void)hipMemcpyAsync(dst, src, n * sizeof(*src), hipMemcpyDeviceToDevice, s); };
        cp(snap.cnt, live.cnt, 4); cp(snap.cam_frame, live.cam_frame, cm); cp(snap.cam_pose, live.cam_pose, cm * 12); cp(snap.cam_fixed, live.cam_fixed, cm);
        cp(snap.pt_key, live.pt_key, snap_np); cp(snap.pt_xyz, live.pt_xyz, snap_np * 3); cp(snap.pt_feat, live.pt_feat, snap_np * 2);
        cp(snap.obs_cam, live.obs_cam, snap_no); cp(snap.obs_pt, live.obs_pt, snap_no); cp(snap.obs_xy, live.obs_xy, snap_no * 2);
    };
    st.live = false;                                                  // (until the call has come through)
    SlamSeq* dseq = st.dseq; double* dK = st.dK;
    if (resume) {
        HIPCHK(hipMemcpyAsync(st.dcar, car.data(), (size_t)S * sizeof(SlamSeqCarry), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(st.drows, hrows.data(), hrows.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (seats) HIPCHK(hipMemcpyAsync(st.dseat, seat.data(), (size_t)S * sizeof(SlamSeat), hipMemcpyHostToDevice, s));
        StageTimer t(ctx, ST_MISC);
        if (seats) launch_slam_carry_restart_seats(s, dseq, st.dcar, st.dseat, S);
        else launch_slam_carry_restart_seqs(s, dseq, st.dcar, S);
    }
    launch_chain_link(s, ctx->pb, cap, B, cb);
    for (int j = 0; j < maxB; j++) {
        const bool step0 = j == 0 && !resume;
        {
            StageTimer t(ctx, ST_MISC);
            launch_chain_gather_seqs(s, ctx->pb, cap, j, R, dseq, S);  // (a track may end in a ghost row)
            if (!step0) {
                launch_pnp_ransac(s, cb.obj, cb.img, cb.off, S, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                                  ctx->pnp_refine, cb.rvec, cb.tvec, cb.pmask, cb.pninl, cb.pstatus, 2);
                launch_chain_pose_seqs(s, ctx->pb, j, dK, dseq, S);
            }
            launch_slam_restart_stream_seqs(s, ctx->pb, cap, j, dseq, S);
            if (!step0) launch_chain_triangulate_seqs(s, ctx->pb, cap, j, dseq, S);
            launch_slam_add_stream_restart_seqs(s, ctx->pb, cap, j, R, o->max_point_norm, o->free_cameras, dseq, S);
        }
        snapshot(j, 1);
        if (ba) {
            { StageTimer t(ctx, ST_SLAM_PREPARE); launch_slam_ba_prepare_seqs(s, j, dseq, S); }
            BaBuf Dj = st.D;
            Dj.chi2 = st.dchi2 + (size_t)2 * j * S; Dj.iterations_run = st.dit + (size_t)j * S; Dj.trials_run = st.dtr + (size_t)j * S;
            { StageTimer t(ctx, ST_SLAM_BA); launch_bundle_adjust(s, Dj, prm, S, o->free_cameras); }
        }
        snapshot(j, 2);
        if (ba || (filt && !step0)) {
            StageTimer t(ctx, ST_SLAM_FILTER);
            launch_slam_filter_stream_restart_seqs(s, ctx->pb, cap, j, dK, step0 ? 0.0 : o->filter_threshold, dseq, S);
        }
        snapshot(j, 3);
        { StageTimer t(ctx, ST_SLAM_LIMIT); launch_slam_limit_stream_restart_seqs(s, j, o->max_cameras, dseq, S); }
        snapshot(j, 4);
        if (st.stats) { StageTimer t(ctx, ST_SLAM_STATS); launch_slam_stats_seqs(s, j, dseq, S, st.sbuf); }
    }
    HIPCHK(hipGetLastError());
    // the anchor camera of a sequence's next call: its last rows of this call (an idle sequence keeps the one it has)
    for (int q = 0; q < S; q++) {
        const int Bq = seq[(size_t)q].count;
        if (Bq == 0) continue;
        HIPCHK(hipMemcpyAsync(st.keep + (size_t)24 * q, seq[(size_t)q].cb.poses + (size_t)Bq * 12, 96, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(st.keep + (size_t)24 * q + 12, seq[(size_t)q].sb.poses_last + (size_t)Bq * 12, 96, hipMemcpyDeviceToDevice, s));
    }
    std::vector<double> hchi((size_t)2 * maxB * S); std::vector<int32_t> hit((size_t)maxB * S), htr((size_t)maxB * S), alive((size_t)S, 1);
    HIPCHK(hipMemcpyAsync(poses_pnp, cb.poses, (size_t)(B + S) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(poses, sb.poses_last, (size_t)(B + S) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_corr, cb.n_corr, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, cb.n_inl, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, cb.status, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_pts, sb.n_pts, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_obs, sb.n_obs, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_cam, sb.n_cam, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hchi.data(), st.dchi2, hchi.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hit.data(), st.dit, hit.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(htr.data(), st.dtr, htr.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(segment, cb.rs.segment, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cause, cb.rs.cause, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(seg_poses_pnp, cb.rs.seg_poses, (size_t)B * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(seg_poses, cb.rs.seg_poses_last, (size_t)B * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(alive.data(), cb.alive, (size_t)S * 4, hipMemcpyDeviceToHost, s));
    for (int q = 0; q < S; q++) {
        const int n = seq[(size_t)q].count > 0 ? seq[(size_t)q].sb.st.n_carried : 0;
        n_carried[q] = n;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(carried_frame + (size_t)q * o->max_cameras, seq[(size_t)q].sb.st.carried_frame, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(carried_poses + (size_t)q * o->max_cameras * 12, seq[(size_t)q].sb.st.carried_poses, (size_t)n * 96, hipMemcpyDeviceToHost, s));
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    for (int q = 0; q < S; q++)                                       // [step][sequence] -> the pair's position in the run
        for (int j = 0; j < seq[(size_t)q].count; j++) {
            const size_t at = (size_t)j * S + q, p = (size_t)seq_off[q] + j;
            chi2[2 * p] = hchi[2 * at]; chi2[2 * p + 1] = hchi[2 * at + 1]; ba_iterations_run[p] = hit[at]; ba_trials_run[p] = htr[at];
        }
    // host copies of every sequence's map, an idle one's too: vo_pairs_run forgot the ones of the call before
    std::vector<LastRun::Map> maps((size_t)S);
    for (int q = 0; q < S; q++) { rc = slam_map_download(ctx, seq[(size_t)q].sb.m, cap, &maps[(size_t)q]); if (rc) return rc; }
    LastRun::Map smap;
    if (snap_on) { rc = slam_map_download(ctx, snap, cap, &smap); if (rc) return rc; }
    ctx->last.map[0] = maps[0];                                       // what vo_slam_map reports: sequence 0, and its snapshot if it has one
    if (snap_on && ss == 0) ctx->last.map[1] = smap;
    ctx->last.seq_map = std::move(maps);
    if (snap_on) { ctx->last.snap_map = std::move(smap); ctx->last.snap_seq = ss; }
    if (st.stats) { rc = slam_stats_download(ctx, st.sbuf, std::vector<int32_t>(seq_off, seq_off + S + 1)); if (rc) return rc; }
    // the stream's state for the next call.  A sequence that advanced gives back every slot but its new anchor's; an idle one has
    // given back all it had at this call's carry.
    const int32_t* sl = ctx->last.slots.data();
    for (int q = 0; q < S; q++) {
        SlamStream::Seq& h = st.seq[(size_t)q];
        const int first = seq_off[q], Bq = seq[(size_t)q].count;
        h.n_rows = 0;
        if (resume && h.vacant) { h.clean = true; h.old_anchor = -1; }    // (reset at this call's carry, if it had not been)
        if (Bq == 0) continue;
        h.vacant = false;                                             // a flight has taken the seat
        int32_t* rows = st.rows.data() + (size_t)q * row_cap;
        rows[h.n_rows++] = sl[2 * first];
        for (int j = 0; j + 1 < Bq; j++) rows[h.n_rows++] = sl[2 * (first + j) + 1];
        h.anchor = sl[2 * (first + Bq) - 1]; h.done = (resume ? h.done : 0) + Bq; h.last_ncam = n_cam[first + Bq - 1];
        h.lost = !alive[(size_t)q]; h.touched = false;
    }
    st.carries = resume ? st.carries + 1 : 0;
    st.live = true;
    return VO_OK;
}

// A multi-stream of S vacant seats: what vo_slam_streams(resume = 0) does before its walk, and no walk.  Every seat is as the memset
// leaves it — the state a stream's first call starts from — so no seat needs a reset; the flights arrive in resumed calls.
extern "C" int vo_slam_streams_open(vo_ctx* ctx, int S, const int32_t* total_pairs, const double* K, const vo_slam_opts* o)
{
    if (!ctx) return VO_ERR_INVALID;
    const char* who = "vo_slam_streams_open";
    drop_slam_stream(ctx);
    forget_slam_maps(ctx);
    if (!total_pairs || !K || !o) FAIL(VO_ERR_INVALID, "bad arguments");
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (S < 1) FAIL(VO_ERR_INVALID, "%s takes at least one seat, got %d", who, S);
    for (int q = 0; q < S; q++)
        if (total_pairs[q] < 1) FAIL(VO_ERR_INVALID, "%s: total_pairs[%d] = %d: a seat holds flights of at least one pair", who, q, total_pairs[q]);
    if (b.kp_cap >= (1 << 20)) FAIL(VO_ERR_INVALID, "too many keypoints for the packed track table");
    int rc = slam_opts_check_values(ctx, o, K); if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SlamStream& st = ctx->stream_map;
    rc = slam_streams_allocate(ctx, st, S, b.max_frames, b.kp_cap, b.max_pairs, total_pairs, o, K);
    if (rc) { drop_slam_stream(ctx); return rc; }
    rc = [&]() -> int {
        HIPCHK(hipMemsetAsync(st.base, 0, st.bytes, s));
        HIPCHK(hipMemcpyAsync(st.dK, K, 72, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return VO_OK;
    }();
    if (rc) { drop_slam_stream(ctx); return rc; }
    for (SlamStream::Seq& h : st.seq) { h.vacant = true; h.clean = true; h.lost = true; }
    st.carries = 0;
    st.live = true;
    return VO_OK;
}

// The flight of seat `seq` is over.  Host only: the seat gives its anchor slot back at once and is reset on the device by the carry
// launch of the next call (k_slam_carry_restart_seats), whether a new flight takes it in that call or later.
extern "C" int vo_slam_streams_replace(vo_ctx* ctx, int seq, int total_pairs)
{
    if (!ctx) return VO_ERR_INVALID;
    const char* who = "vo_slam_streams_replace";
    SlamStream& st = ctx->stream_map;
    if (!st.live) FAIL(VO_ERR_INVALID, "%s: there is no stream (none was started, or a configure or vo_slam_chain* call dropped it)", who);
    if (!st.multi) FAIL(VO_ERR_INVALID, "%s: the stream was started by %s, which has no seats", who, st.restart ? "vo_slam_stream_restart" : "vo_slam_stream");
    if (seq < 0 || seq >= st.S) FAIL(VO_ERR_INVALID, "%s: the stream has seats 0 .. %d, got %d", who, st.S - 1, seq);
    SlamStream::Seq& h = st.seq[(size_t)seq];
    if (total_pairs < 1 || total_pairs > h.capacity)
        FAIL(VO_ERR_INVALID, "%s: seat %d holds flights of 1 .. %d pairs (what its lists were sized for), got %d", who, seq, h.capacity, total_pairs);
    h.total = total_pairs;
    if (h.vacant) return VO_OK;                                       // (only the bound of the flight to come)
    h.vacant = true; h.clean = false;
    h.old_anchor = h.anchor; h.anchor = -1;
    h.done = 0; h.last_ncam = 0; h.lost = true; h.touched = false;
    return VO_OK;
}

static const LastRun::Map* slam_chains_map_of(vo_ctx* ctx, int seq, int which)
{
    const LastRun& l = ctx->last;
    const char* why = nullptr;
    if (which < 0 || which > 1) why = "which must be 0 (the map at the end of the sequence) or 1 (the snapshot)";
    else if (l.seq_map.empty()) why = "no such map: vo_slam_chains has not run since the last configure / vo_pairs_run / chain call";
    else if (seq < 0 || seq >= (int)l.seq_map.size()) why = "no such sequence in the most recent vo_slam_chains";
    else if (which == 1 && seq != l.snap_seq) why = "no such map: the most recent vo_slam_chains took no snapshot of this sequence";
    if (why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); return nullptr; }
    return which == 1 ? &l.snap_map : &l.seq_map[(size_t)seq];
}

extern "C" int vo_slam_chains_map_size(vo_ctx* ctx, int seq, int which, int32_t* ncam, int32_t* npt, int32_t* nobs)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!ncam || !npt || !nobs) FAIL(VO_ERR_INVALID, "bad arguments");
    const LastRun::Map* m = slam_chains_map_of(ctx, seq, which);
    if (!m) return VO_ERR_INVALID;
    *ncam = (int32_t)m->cam_frame.size(); *npt = (int32_t)(m->points.size() / 3); *nobs = (int32_t)m->obs_cam.size();
    return VO_OK;
}

extern "C" int vo_slam_chains_map(vo_ctx* ctx, int seq, int which, int32_t* cam_frame, double* cam_pose, uint8_t* cam_fixed, int32_t* pt_feature,
                                  double* points, int32_t* obs_cam, int32_t* obs_pt, double* obs_xy)
{
    if (!ctx) return VO_ERR_INVALID;
    const LastRun::Map* m = slam_chains_map_of(ctx, seq, which);
    if (!m) return VO_ERR_INVALID;
    return slam_map_copy_out(ctx, m, cam_frame, cam_pose, cam_fixed, pt_feature, points, obs_cam, obs_pt, obs_xy);
}

// the statistics rows of sequence seq of the most recent vo_slam_* call, nullptr (and the reason in ctx->err) if there are none
static const LastRun::Stats* slam_stats_of(vo_ctx* ctx, int seq)
{
    const LastRun::Stats& h = ctx->last.stats;
    const char* why = nullptr;
    if (!h.valid) why = "no statistics: no vo_slam_* call has run with vo_set_slam_stats on since the last configure / vo_pairs_run / chain call";
    else if (seq < 0 || seq + 1 >= (int)h.seq_off.size()) why = "no such sequence in the most recent vo_slam_* call";
    if (why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); return nullptr; }
    return &h;
}

extern "C" int vo_slam_stats_size(vo_ctx* ctx, int seq, int32_t* B, int32_t* max_cameras)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!B || !max_cameras) FAIL(VO_ERR_INVALID, "bad arguments");
    const LastRun::Stats* h = slam_stats_of(ctx, seq);
    if (!h) return VO_ERR_INVALID;
    *B = h->seq_off[(size_t)seq + 1] - h->seq_off[(size_t)seq]; *max_cameras = h->C - 1;
    return VO_OK;
}

extern "C" int vo_slam_stats_counts(vo_ctx* ctx, int seq, int B, int32_t* n_cam, int32_t* n_pts, int32_t* n_obs)
{
    if (!ctx) return VO_ERR_INVALID;
    const LastRun::Stats* h = slam_stats_of(ctx, seq);
    if (!h) return VO_ERR_INVALID;
    const int first = h->seq_off[(size_t)seq], n = h->seq_off[(size_t)seq + 1] - first;
    if (B != n) FAIL(VO_ERR_INVALID, "sequence %d had %d pairs in the call, B = %d", seq, n, B);
    if (B > 0 && (!n_cam || !n_pts || !n_obs)) FAIL(VO_ERR_INVALID, "bad arguments");
    for (int p = 0; p < B; p++) {
        const int32_t* c = h->counts.data() + 3 * ((size_t)first + p);
        n_cam[p] = c[0]; n_pts[p] = c[1]; n_obs[p] = c[2];
    }
    return VO_OK;
}

extern "C" int vo_slam_stats(vo_ctx* ctx, int seq, int B, int C, double* total_sqerr, double* max_sqerr, int32_t* n_high, int32_t* obs_hist,
                             int32_t* obs_matrix, int32_t* cam_frame)
{
    if (!ctx) return VO_ERR_INVALID;
    const LastRun::Stats* h = slam_stats_of(ctx, seq);
    if (!h) return VO_ERR_INVALID;
    const int first = h->seq_off[(size_t)seq], n = h->seq_off[(size_t)seq + 1] - first, hc = h->C;
    if (B != n) FAIL(VO_ERR_INVALID, "sequence %d had %d pairs in the call, B = %d", seq, n, B);
    if (C < hc - 1) FAIL(VO_ERR_INVALID, "C = %d is less than the call's max_cameras = %d", C, hc - 1);
    if (B > 0 && (!total_sqerr || !max_sqerr || !n_high || !obs_hist || !obs_matrix || !cam_frame)) FAIL(VO_ERR_INVALID, "bad arguments");
    // (a row holds max_cameras + 1 cameras, the map after the limit at most max_cameras: the last row and column are empty)
    const int k = std::min(C, hc);
    for (int p = 0; p < B; p++) {
        const size_t r = (size_t)first + p;
        total_sqerr[p] = h->total_sqerr[r]; max_sqerr[p] = h->max_sqerr[r]; n_high[p] = h->n_high[r];
        memcpy(obs_hist + (size_t)p * VO_STATS_HIST, h->obs_hist.data() + r * VO_STATS_HIST, VO_STATS_HIST * sizeof(int32_t));
        for (int a = 0; a < C; a++) {
            cam_frame[(size_t)p * C + a] = a < k ? h->cam_frame[r * hc + a] : -1;
            for (int b = 0; b < C; b++) obs_matrix[((size_t)p * C + a) * C + b] = a < k && b < k ? h->obs_matrix[(r * hc + a) * hc + b] : 0;
        }
    }
    return VO_OK;
}

extern "C" int vo_profile_enable(vo_ctx* ctx, int on)
{
    if (!ctx) return VO_ERR_INVALID;
    ctx->prof = on != 0;
    ctx->n_ev = 0;
    return VO_OK;
}

extern "C" int vo_profile_reset(vo_ctx* ctx)
{
    if (!ctx) return VO_ERR_INVALID;
    memset(ctx->prof_ms, 0, sizeof(ctx->prof_ms));
    memset(ctx->prof_n, 0, sizeof(ctx->prof_n));
    ctx->n_ev = 0;
    return VO_OK;
}

extern "C" int vo_profile_read(vo_ctx* ctx, float* ms, int32_t* launches)
{
    if (!ctx || !ms || !launches) return VO_ERR_INVALID;
    memcpy(ms, ctx->prof_ms, sizeof(ctx->prof_ms));
    memcpy(launches, ctx->prof_n, sizeof(ctx->prof_n));
    return VO_OK;
}

extern "C" const char* vo_stage_name(int stage)
{
    return stage >= 0 && stage < VO_STAGE_COUNT ? k_stage_names[stage] : "?";
}

// Algorithmic HBM bytes per launch (SURVEY.md 8(d) accounting: u8 pixels = 1 B; each streaming stage reads its
// input once and writes its output once; padding columns are not counted).
extern "C" double vo_stage_bytes(vo_ctx* ctx, int stage, int F)
{
    const Batch bt = ctx ? batch(ctx) : Batch{};
    if (bt.sift && bt.ready) {
        // SIFT: float planes.  One layer sweep reads its source plane and writes a Gaussian plane; per octave nLayers + 2
        // sweeps; the base image: u8 in, float out, one blur; next-octave seeds.  The extrema search reads the octave's nLayers + 3
        // Gaussian planes (the DoG planes are differences made in registers, never stored).
        const SiftState& S = ctx->sift;
        const int L = S.P.nLayers;
        double px = 0;
        for (int o = 0; o < S.P.nOct; o++) px += (double)S.P.w[o] * S.P.h[o];
        const double p0 = (double)S.P.w[0] * S.P.h[0];
        double b = 0;
        if (stage == ST_SIFT_SCALE) b = (double)S.w * S.h + 4.0 * p0 * 3 + 4.0 * px * ((L + 2) + (L + 2)) + 4.0 * (px - p0) * 1.25;
        else if (stage == ST_SIFT_EXTREMA) b = 4.0 * px * (L + 3);
        else if (stage == ST_MATCH_NN) b = 2.0 * S.kp_cap * 128;
        return b * F;
    }
    if (!ctx || !ctx->configured) return 0.0;
    const PyrGeom& g = ctx->g;
    double px[VO_MAX_LEVELS], total = 0;
    for (int l = 0; l < g.nlevels; l++) { px[l] = (double)g.lv[l].w * g.lv[l].h; total += px[l]; }
    const double N = g.nfeatures;
    double b = 0;
    switch (stage) {
    case ST_RESIZE: b = (total - px[g.nlevels - 1]) + (total - px[0]); break;   // reads levels 0..L-2, writes 1..L-1
    case ST_FAST: b = total; break;                                               // FAST reads P (winner lists are a few KB)
    case ST_SELECT_FAST: b = 2 * 2 * N * 12; break;                               // ~2N kept winners: list entry read twice, 8 B written
    case ST_HARRIS: b = 2 * N * 81 + 2 * N * 4; break;
    case ST_ANGLE: b = N * 749; break;
    case ST_BLUR: b = total + total; break;
    case ST_BRIEF: b = N * 512 + N * 32 + N * 28; break;
    case ST_MATCH_NN: b = 2 * N * 32; break;                                       // per pair ~ per frame: both descriptor sets
    case ST_MATCH_SELECT: b = 16 * N; break;
    case ST_RANSAC: b = 33 * N; break;                                             // SURVEY 8(d) geometry 65 N: 4 f64 coords + mask per match ...
    case ST_POSE: b = 32 * N; break;                                               // ... + the inliers' coordinates again
    default: b = 0;
    }
    return b * F;
}
