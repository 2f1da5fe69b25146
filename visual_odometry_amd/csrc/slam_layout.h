// slam_layout.h — the shape of one vo_slam_* call and where its device buffers lie (slam_api.hip).
// Pointer arithmetic over ScratchLayout only: nothing in this header calls the HIP runtime, so tests/native/slam_layout_driver.cpp
// places the layout at a made-up base on a machine without a GPU.
#pragma once
#include "vo_internal.h"
#include <vector>

struct vo_ctx;

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
    int place(vo_ctx* ctx);               // (vo_host.h)
    struct Slot { void* dst; size_t off; void (*set)(void*, uint8_t*); };
    std::vector<Slot> slots;
};

// The shape of a call.  Every entry point fills it by its own formulas (the kernels receive these values as capacities):
//   entry                      S   rows     np of a sequence     no of a sequence            P
//   vo_slam_chain              1   F        F cap                2 B cap                     B
//   vo_slam_chains[_restart]   S   F        (B_q + 1) cap        2 B_q cap                   B
//   vo_slam_stream[_restart]   1   F + 2    (total + 1) cap      2 cap min(cm, total)        max_pairs
//   vo_slam_streams / _open    S   F + 2 S  (total_q + 1) cap    2 cap min(cm, total_q)      max_pairs
struct SlamDims {
    int S = 1;                            // sequences
    int F = 0;                            // frame slots: rows of cam / cam_ok
    size_t rows = 0;                      // rows of the other slot-keyed tables (parent, in_map, map_pt, pt_of): the slots, then the ghost rows
    size_t cap = 0, cm = 0;               // keypoints a frame holds; cameras a map holds before the limit: max_cameras + 1
    int free_cameras = 1;
    std::vector<size_t> np, no;           // [S] points and observations a sequence's lists hold
    size_t P = 0;                         // rows of the per-pair outputs
    size_t steps = 0;                     // steps dchi2 / dit / dtr hold, [step][S] each
    size_t snap_np = 0, snap_no = 0;      // points and observations the snapshot holds (with `snapshot`)
    bool stream = false;                  // carried from call to call: pt_feat, keep, the carried rows, dcar / drows / dseat; the per-call part is cleared alone
    bool restart = false;                 // RestartBuf: the segment state words and the per-pair segment rows
    bool stats = false;                   // StatsBuf: k_slam_stats' scratch and its rows
    bool snapshot = false;                // a second map's lists, for one sequence
    size_t npair(int q) const { return no[(size_t)q] * (free_cameras + 1) / 2; }   // the pair list of a sequence
    int nblk() const { return free_cameras * (free_cameras + 1) / 2; }             // its block offsets: nblk + 1
    size_t fc() const { return rows * cap; }
    size_t NP() const { size_t n = 0; for (size_t v : np) n += v; return n; }
    size_t NO() const { size_t n = 0; for (size_t v : no) n += v; return n; }
    size_t NPAIR() const { size_t n = 0; for (int q = 0; q < S; q++) n += npair(q); return n; }
};

// What the layout names: the whole arrays (a sequence's descriptor owns its ranges of them: slam_seq) and the few loose buffers
struct SlamBufs {
    ChainBuf cb{}; SlamBuf sb{}; BaBuf D{}; StatsBuf stats{}; SlamMap snap{};
    double *dK = nullptr, *dchi2 = nullptr, *keep = nullptr; int *dit = nullptr, *dtr = nullptr;   // dchi2 / dit / dtr: k_bundle_adjust writes problem s of step j at [j][s]
    SlamSeq* dseq = nullptr; SlamSeqCarry* dcar = nullptr; int* drows = nullptr;
    SlamSeat* dseat = nullptr;            // what the carry launch does for every seat, when one of them is vacant
    size_t bytes = 0, call0 = 0;          // [call0, bytes): what a call reports — the part a resumed call of a stream clears
};

// The statistics rows of P pairs with room for cm cameras, and k_slam_stats' scratch for np points and no observations, as
// sub-buffers of a call's layout (vo_set_slam_stats, vo_map_statistics).
static inline void slam_stats_take_scratch(ScratchLayout& sc, StatsBuf& d, size_t np, size_t no)
{
    sc.take(&d.pt_cur, np); sc.take(&d.slot, no); sc.take(&d.bad, 1);
}

static inline void slam_stats_take_rows(ScratchLayout& sc, StatsBuf& d, size_t P, size_t cm)
{
    sc.take(&d.total_sqerr, P); sc.take(&d.max_sqerr, P); sc.take(&d.n_high, P); sc.take(&d.counts, P * 3); sc.take(&d.obs_hist, P * VO_STATS_HIST);
    sc.take(&d.obs_matrix, P * cm * cm); sc.take(&d.cam_frame, P * cm);
    d.C = (int)cm; d.high = 10.0;
}

static inline void slam_map_take(ScratchLayout& sc, SlamMap& m, size_t maps, size_t ncam, size_t npt, size_t nobs, bool feat)
{
    sc.take(&m.cnt, 4 * maps); sc.take(&m.cam_frame, ncam); sc.take(&m.cam_pose, ncam * 12); sc.take(&m.cam_fixed, ncam);
    sc.take(&m.pt_key, npt); sc.take(&m.pt_xyz, npt * 3);
    if (feat) sc.take(&m.pt_feat, npt * 2);
    sc.take(&m.obs_cam, nobs); sc.take(&m.obs_pt, nobs); sc.take(&m.obs_xy, nobs * 2);
}

// The one layout of every vo_slam_* call: returns its bytes, and with a base sets every pointer of b.  What outlives a call comes
// first and the per-call outputs last, so a stream clears [call0, bytes) with one memset and a scratch call everything with one.
// Every list is carved once for all sequences.  A switch that is off takes nothing and leaves its pointers nullptr.
static inline size_t slam_layout(const SlamDims& d, uint8_t* base, SlamBufs& b)
{
    const size_t S = (size_t)d.S, fc = d.fc(), F = (size_t)d.F, cap = d.cap, NC = d.cm * S, NP = d.NP(), NO = d.NO(), P = d.P;
    b = SlamBufs();
    ChainBuf& cb = b.cb; SlamBuf& sb = b.sb; BaBuf& D = b.D; StatsBuf& st = b.stats;
    ScratchLayout sc;
    // shared, keyed by slot (and ghost row)
    sc.take(&cb.parent, fc); sc.take(&cb.map_pt, fc * 3); sc.take(&cb.cam, F * 12); sc.take(&cb.in_map, fc); sc.take(&cb.cam_ok, F); sc.take(&sb.pt_of, fc);
    sc.take(&b.dK, 9);
    // per sequence: the current problem, the step's state, and what outlives a call — alive, the segment state words, the anchor camera
    sc.take(&cb.obj, S * cap * 3); sc.take(&cb.img, S * cap * 2); sc.take(&cb.Xw, S * cap * 4); sc.take(&cb.pmask, S * cap);
    sc.take(&sb.dec, S * cap); sc.take(&cb.off, 2 * S); sc.take(&cb.rvec, 3 * S); sc.take(&cb.tvec, 3 * S);
    sc.take(&cb.pninl, S); sc.take(&cb.pstatus, S); sc.take(&cb.P1, 12 * S); sc.take(&cb.P2, 12 * S); sc.take(&cb.alive, S); sc.take(&cb.map_count, S);
    if (d.restart) sc.take(&cb.rs.st, 4 * S);
    if (d.stream) sc.take(&b.keep, 24 * S);
    // the maps' lists and the bundle adjustment's: a sequence's range starts at its BaProblem offsets
    slam_map_take(sc, sb.m, S, NC, NP, NO, d.stream);
    sc.take(&sb.tmp, NP); sc.take(&sb.idx, NO); sc.take(&sb.prob, S); sc.take(&sb.cam_col, NC); sc.take(&sb.pt_first, NP + S);
    sc.take(&sb.s_cam, NO); sc.take(&sb.s_pt, NO); sc.take(&sb.s_xy, NO * 2); sc.take(&sb.pairs, d.NPAIR()); sc.take(&sb.blk_first, S * ((size_t)d.nblk() + 1));
    sc.take(&D.X2, NP * 3); sc.take(&D.W, NO * 18); sc.take(&D.Hpp, NP * 6); sc.take(&D.bp, NP * 3); sc.take(&D.Hpi, NP * 6);
    if (d.snapshot) slam_map_take(sc, b.snap, 1, d.cm, d.snap_np, d.snap_no, d.stream);
    sc.take(&b.dseq, S);
    if (d.stream) { sc.take(&b.dcar, S); sc.take(&b.drows, S * (P + 1)); sc.take(&b.dseat, S); }
    if (d.stats) slam_stats_take_scratch(sc, st, NP, NO);
    b.call0 = sc.bytes;
    // per pair, in the run's order; sequence s owns the pose rows seq_off[s] + s .. seq_off[s + 1] + s
    if (d.stats) slam_stats_take_rows(sc, st, P, d.cm);
    sc.take(&cb.poses, (P + S) * 12); sc.take(&sb.poses_last, (P + S) * 12);
    sc.take(&cb.n_corr, P); sc.take(&cb.n_inl, P); sc.take(&cb.status, P); sc.take(&cb.n_map, P); sc.take(&sb.n_pts, P); sc.take(&sb.n_obs, P); sc.take(&sb.n_cam, P);
    sc.take(&b.dchi2, 2 * d.steps * S); sc.take(&b.dit, d.steps * S); sc.take(&b.dtr, d.steps * S);
    if (d.stream) { sc.take(&sb.st.carried_frame, NC); sc.take(&sb.st.carried_poses, NC * 12); }
    if (d.restart) { sc.take(&cb.rs.segment, P); sc.take(&cb.rs.cause, P); sc.take(&cb.rs.seg_poses, P * 12); sc.take(&cb.rs.seg_poses_last, P * 12); }
    b.bytes = sc.bytes;
    if (!base) return sc.bytes;
    sc.place_at(base);
    if (d.stats) st.Kd = b.dK;
    D.prob = sb.prob; D.poses = sb.m.cam_pose; D.cam_col = sb.cam_col; D.X = sb.m.pt_xyz; D.pt_first = sb.pt_first;
    D.obs_cam = sb.s_cam; D.obs_pt = sb.s_pt; D.obs_xy = sb.s_xy; D.pairs = sb.pairs; D.blk_first = sb.blk_first;
    return sc.bytes;
}

// Sequence q's descriptor: its ranges of the whole arrays, its capacities, and its rows of this call's outputs — pairs
// first .. first + count - 1 of the run, the pose rows from first + q.  frame0 and n_carried are a stream's (StreamBuf).
// With S = 1 and first = 0 every base is 0 and cb / sb name the whole arrays: what the single forms hand their kernels.
static inline SlamSeq slam_seq(const SlamDims& d, const SlamBufs& b, int q, int first, int count, int frame0 = 0, int n_carried = 0)
{
    const size_t cap = d.cap;
    SlamSeq e{};
    e.first = first; e.count = count;
    BaProblem at{};
    size_t pt0 = 0, ob0 = 0, pr0 = 0;
    for (int i = 0; i < q; i++) { pt0 += d.np[(size_t)i]; ob0 += d.no[(size_t)i]; pr0 += d.npair(i); }
    at.cam0 = (int)(d.cm * q); at.pt0 = (int)pt0; at.obs0 = (int)ob0; at.pair0 = (int)pr0; at.blk0 = q * (d.nblk() + 1);
    ChainBuf& c = e.cb; c = b.cb;
    c.obj0 = q * (int)cap;                                   // k_pnp_ransac indexes the whole arrays by the sequence's {first, end}
    c.off += 2 * q; c.rvec += 3 * q; c.tvec += 3 * q; c.pmask += (size_t)q * cap; c.pninl += q; c.pstatus += q; c.P1 += 12 * q; c.P2 += 12 * q;
    c.obj += (size_t)q * cap * 3; c.img += (size_t)q * cap * 2; c.Xw += (size_t)q * cap * 4; c.alive += q; c.map_count += q;
    c.n_corr += first; c.n_inl += first; c.status += first; c.n_map += first; c.poses += (size_t)(first + q) * 12;
    if (d.restart) { c.rs.st += 4 * q; c.rs.segment += first; c.rs.cause += first; c.rs.seg_poses += (size_t)first * 12; c.rs.seg_poses_last += (size_t)first * 12; }
    SlamBuf& m = e.sb; m = b.sb;
    m.base = at;
    m.cam_cap = (int)d.cm; m.pt_cap = (int)d.np[(size_t)q]; m.obs_cap = (int)d.no[(size_t)q]; m.pair_cap = (int)d.npair(q);
    m.m.cnt += 4 * q; m.m.cam_frame += at.cam0; m.m.cam_pose += (size_t)at.cam0 * 12; m.m.cam_fixed += at.cam0;
    m.m.pt_key += at.pt0; m.m.pt_xyz += (size_t)at.pt0 * 3; m.m.obs_cam += at.obs0; m.m.obs_pt += at.obs0; m.m.obs_xy += (size_t)at.obs0 * 2;
    m.dec += (size_t)q * cap; m.tmp += at.pt0; m.idx += at.obs0; m.n_pts += first; m.n_obs += first; m.n_cam += first; m.poses_last += (size_t)(first + q) * 12;
    m.prob += q; m.cam_col += at.cam0; m.pt_first += at.pt0 + q; m.s_cam += at.obs0; m.s_pt += at.obs0; m.s_xy += (size_t)at.obs0 * 2;
    m.pairs += at.pair0; m.blk_first += at.blk0;
    if (d.stream) {
        m.m.pt_feat += (size_t)at.pt0 * 2; m.st.carried_frame += at.cam0; m.st.carried_poses += (size_t)at.cam0 * 12;
        m.st.frame0 = frame0; m.st.n_carried = n_carried;
    }
    return e;
}
