// slam_api.hip — the vo_slam_* entry points of libvo_hip.so: the reference's complete per-frame map step, on resident data.
// vo_tracks_pnp_batch's walk (vo_api.hip) with what ends every frame of VisualSlam.estimate_current_camera_position
// (src/visual_slam.py:190-266) joined to it: the Observations of add_information_to_map, freeze_nonlast_cameras, Map.optimize_map,
// the threshold filter and limit_number_of_camera_in_map — on a map that stays in HBM (slam_kernels.hip), pair after pair with no
// host round trip.  Host code only, and one of each: every entry point describes its call as a SlamDims, slam_layout
// (slam_layout.h) places the buffers, slam_seq names a sequence's ranges of them, slam_walk issues the steps and slam_download
// brings the results back.  An entry point keeps its own checks, its own formulas for the dims and its own end-of-call state.
#include "vo_host.h"

// A snapshot: the lists of one map copied beside it, pt_feat with them where the map has it (a stream's).  dst has room for
// cm cameras, np points, no observations.
static void slam_map_copy(hipStream_t s, const SlamMap& dst, const SlamMap& src, size_t cm, size_t np, size_t no)
{
    auto cp = [&](auto* d, const auto* from, size_t n) { (void)hipMemcpyAsync(d, from, n * sizeof(*from), hipMemcpyDeviceToDevice, s); };
    cp(dst.cnt, src.cnt, 4); cp(dst.cam_frame, src.cam_frame, cm); cp(dst.cam_pose, src.cam_pose, cm * 12); cp(dst.cam_fixed, src.cam_fixed, cm);
    cp(dst.pt_key, src.pt_key, np); cp(dst.pt_xyz, src.pt_xyz, np * 3);
    if (src.pt_feat) cp(dst.pt_feat, src.pt_feat, np * 2);
    cp(dst.obs_cam, src.obs_cam, no); cp(dst.obs_pt, src.obs_pt, no); cp(dst.obs_xy, src.obs_xy, no * 2);
}

// first, count: the pairs of the run that are the map's chain (pt_feature names a frame by its index along that chain)
static int slam_map_download(vo_ctx* ctx, const SlamMap& m, int cap, LastRun::Map* out, int first, int count)
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
    if (m.pt_feat) {                                                  // a stream keeps the feature ids as (frame, keypoint) on the device
        if (np) HIPCHK(hipMemcpy(out->pt_feature.data(), m.pt_feat, np * 8, hipMemcpyDeviceToHost));
        out->valid = true;
        return VO_OK;
    }
    // feature id (slot, keypoint) -> (index of the frame in the chain, keypoint)
    const int32_t* sl = ctx->last.slots.data() + 2 * (size_t)first;
    for (size_t i = 0; i < np; i++) {
        const int slot = key[i] / cap;
        int frame = sl[0] == slot ? 0 : -1;
        for (int p = 0; frame < 0 && p < count; p++) if (sl[2 * p + 1] == slot) frame = p + 1;
        out->pt_feature[2 * i] = frame; out->pt_feature[2 * i + 1] = key[i] % cap;
    }
    out->valid = true;
    return VO_OK;
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

// the dims every entry point fills the same way; np, no, P, steps and the stream / restart / snapshot switches are its own
static SlamDims slam_dims(const vo_ctx* ctx, int S, int F, size_t rows, int cap, const vo_slam_opts* o)
{
    SlamDims d;
    d.S = S; d.F = F; d.rows = rows; d.cap = (size_t)cap; d.cm = (size_t)o->max_cameras + 1; d.free_cameras = o->free_cameras;
    d.stats = ctx->slam_stats != 0;
    return d;
}

// a call that lives in the scratch buffer: the buffer belongs to the next call, whatever is kept is kept as host copies
static int slam_place_scratch(vo_ctx* ctx, const SlamDims& d, SlamBufs& b)
{
    const size_t bytes = slam_layout(d, nullptr, b);
    int rc = ctx->scratch.grow(ctx, bytes, bytes + bytes / 4 + 64); if (rc) return rc;
    ctx->scratch_epoch++;
    slam_layout(d, ctx->scratch.p, b);
    return VO_OK;
}

// a stream's allocation: it lives from the call that starts the stream until the stream is dropped
static int slam_place_stream(vo_ctx* ctx, SlamStream& st, const SlamDims& d)
{
    st.dims = d;
    const size_t bytes = slam_layout(d, nullptr, st.b);
    HIPCHK(st.mem.alloc(&st.base, bytes));
    slam_layout(d, st.base, st.b);
    return VO_OK;
}

// ------------------------------------------------------------------ the walk
// One call's launches, for every entry point.  A step j works on pair j of a single form, on pair first + j of every sequence
// that has one otherwise (the sequence is on a grid axis, the host loop runs to the longest sequence's pairs).  step 0: j = 0 of
// a call that is not resumed.  What a family launches, phase by phase (every launcher in slam_walk's lambdas, nowhere else):
//
//   family             carry, resumed call           localise, step 0          localise, later steps                    add / filter / limit
//   chain              -                             init                      gather pnp pose triangulate              k_slam_add, _filter, _limit
//   stream             k_slam_carry                  init                      gather pnp pose triangulate              the _stream forms
//   stream-restart     k_slam_carry_restart          gather restart            gather pnp pose restart triangulate      the _stream_restart forms
//   sequences          -                             init                      gather pnp pose triangulate              the _seqs forms
//   sequences-restart  -                             gather restart            gather pnp pose restart triangulate      the _seqs forms
//   streams            k_slam_carry_restart_seqs,    gather restart            gather pnp pose restart triangulate      the _stream_restart_seqs forms
//                      _seats with a vacant seat
//
// From sequences on, every launcher is the _seqs form and k_pnp_ransac takes the S problems with a {first, end} pair each.
// k_chain_link runs once before the loop, outside any bracket.  Brackets per step: misc (localise and add), slam_ba_prepare and
// slam_bundle_adjust with BA on, slam_filter with BA on or with a threshold past step 0, slam_camera_limit, slam_map_statistics
// with statistics on; and misc once for the carry.  The snapshot follows add (1), BA (2), filter (3) or limit (4).
enum SlamFamily { FAM_CHAIN, FAM_STREAM, FAM_STREAM_RESTART, FAM_SEQS, FAM_SEQS_RESTART, FAM_STREAMS };

struct SlamWalk {
    SlamFamily fam;
    bool resume;                          // the maps are carried from an earlier call: the carry launch first, and no step 0
    int rows;                             // rows of the slot-keyed tables: the bound of a track walk
    int steps;                            // B of a single form, the longest sequence's pairs otherwise
    int snap_seq;                         // the sequence whose map the snapshot copies, -1: none
    SlamCarry carry;                      // stream, stream-restart: the carry of a resumed call
    bool seats;                           // streams: some seat is vacant
    const SlamArchive* archive = nullptr; // stream with an archive (vo_set_stream_archive): the limit that also appends what it removes
};

static int slam_walk(vo_ctx* ctx, const SlamWalk& w, const SlamDims& d, const SlamBufs& b, const std::vector<SlamSeq>& seq, const double* K, const vo_slam_opts* o)
{
    hipStream_t s = ctx->stream;
    const PairBuf& pb = ctx->pb;
    const SlamFamily fam = w.fam;
    const bool multi = fam >= FAM_SEQS, with_restart = fam == FAM_STREAM_RESTART || fam == FAM_SEQS_RESTART || fam == FAM_STREAMS;
    const int S = d.S, cap = (int)d.cap, R = w.rows;
    const ChainBuf& cb = seq[0].cb; const SlamBuf& sb = seq[0].sb;   // a single form's: the whole arrays
    const SlamSeq* dseq = b.dseq; const double* dK = b.dK;
    int B = 0;
    for (const SlamSeq& e : seq) B += e.count;
    auto carry = [&]() {
        if (fam == FAM_STREAM) launch_slam_carry(s, w.carry, cb, sb);
        else if (fam == FAM_STREAM_RESTART) launch_slam_carry_restart(s, w.carry, cb, sb);
        else if (w.seats) launch_slam_carry_restart_seats(s, dseq, b.dcar, b.dseat, S);
        else launch_slam_carry_restart_seqs(s, dseq, b.dcar, S);
    };
    auto init = [&]() { if (multi) launch_chain_init_seqs(s, pb, cap, dseq, S); else launch_chain_init(s, pb, cap, cb); };
    auto gather = [&](int j) { if (multi) launch_chain_gather_seqs(s, pb, cap, j, R, dseq, S); else launch_chain_gather(s, pb, cap, j, R, cb); };
    auto pnp_pose = [&](int j) {
        launch_pnp_ransac(s, b.cb.obj, b.cb.img, b.cb.off, S, dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                          ctx->pnp_refine, b.cb.rvec, b.cb.tvec, b.cb.pmask, b.cb.pninl, b.cb.pstatus, multi ? 2 : 1);
        if (multi) launch_chain_pose_seqs(s, pb, j, dK, dseq, S); else launch_chain_pose(s, pb, j, dK, cb);
    };
    auto restart = [&](int j) {
        if (fam == FAM_STREAM_RESTART) launch_slam_restart_stream(s, pb, cap, j, cb, sb);
        else if (fam == FAM_SEQS_RESTART) launch_slam_restart_seqs(s, pb, cap, j, dseq, S);
        else launch_slam_restart_stream_seqs(s, pb, cap, j, dseq, S);
    };
    auto triangulate = [&](int j) { if (multi) launch_chain_triangulate_seqs(s, pb, cap, j, dseq, S); else launch_chain_triangulate(s, pb, cap, j, cb); };
    auto add = [&](int j) {
        switch (fam) {
        case FAM_CHAIN: launch_slam_add(s, pb, cap, j, R, o->max_point_norm, o->free_cameras, cb, sb); break;
        case FAM_STREAM: launch_slam_add_stream(s, pb, cap, j, R, o->max_point_norm, o->free_cameras, cb, sb); break;
        case FAM_STREAM_RESTART: launch_slam_add_stream_restart(s, pb, cap, j, R, o->max_point_norm, o->free_cameras, cb, sb); break;
        case FAM_SEQS: case FAM_SEQS_RESTART: launch_slam_add_seqs(s, pb, cap, j, R, o->max_point_norm, o->free_cameras, dseq, S); break;
        case FAM_STREAMS: launch_slam_add_stream_restart_seqs(s, pb, cap, j, R, o->max_point_norm, o->free_cameras, dseq, S); break;
        }
    };
    auto prepare = [&](int j) { if (multi) launch_slam_ba_prepare_seqs(s, j, dseq, S); else launch_slam_ba_prepare(s, cb, sb); };
    auto filter = [&](int j, double threshold) {
        switch (fam) {
        case FAM_CHAIN: launch_slam_filter(s, pb, dK, threshold, cb, sb); break;
        case FAM_STREAM: launch_slam_filter_stream(s, pb, dK, threshold, cb, sb); break;
        case FAM_STREAM_RESTART: launch_slam_filter_stream_restart(s, pb, dK, threshold, cb, sb); break;
        case FAM_SEQS: case FAM_SEQS_RESTART: launch_slam_filter_seqs(s, pb, cap, j, dK, threshold, dseq, S); break;
        case FAM_STREAMS: launch_slam_filter_stream_restart_seqs(s, pb, cap, j, dK, threshold, dseq, S); break;
        }
    };
    auto limit = [&](int j) {
        switch (fam) {
        case FAM_CHAIN: launch_slam_limit(s, j, o->max_cameras, cb, sb); break;
        case FAM_STREAM:
            if (w.archive) launch_slam_limit_stream_archive(s, j, o->max_cameras, cb, sb, *w.archive);
            else launch_slam_limit_stream(s, j, o->max_cameras, cb, sb);
            break;
        case FAM_STREAM_RESTART: launch_slam_limit_stream_restart(s, j, o->max_cameras, cb, sb); break;
        case FAM_SEQS: case FAM_SEQS_RESTART: launch_slam_limit_seqs(s, j, o->max_cameras, dseq, S); break;
        case FAM_STREAMS: launch_slam_limit_stream_restart_seqs(s, j, o->max_cameras, dseq, S); break;
        }
    };
    auto stats = [&](int j) { if (multi) launch_slam_stats_seqs(s, j, dseq, S, b.stats); else launch_slam_stats(s, j, sb, b.stats); };
    auto snapshot = [&](int j, int stage) {
        if (w.snap_seq < 0 || j != o->snapshot_pair || stage != o->snapshot_stage) return;
        slam_map_copy(s, b.snap, seq[(size_t)w.snap_seq].sb.m, d.cm, d.np[(size_t)w.snap_seq], d.no[(size_t)w.snap_seq]);
    };

    const BaParams prm{K[0], K[2], K[5], o->huber_delta, o->ba_iterations};
    const bool ba = o->ba_iterations > 0, filt = o->filter_threshold > 0;
    if (w.resume) { StageTimer t(ctx, ST_MISC); carry(); }
    launch_chain_link(s, pb, cap, B, b.cb);
    for (int j = 0; j < w.steps; j++) {
        const bool step0 = j == 0 && !w.resume;
        {
            StageTimer t(ctx, ST_MISC);
            if (with_restart) {                                       // (step 0 is an initial step like any other: k_chain_gather meets a map that is empty)
                gather(j);
                if (!step0) pnp_pose(j);
                restart(j);
                if (!step0) triangulate(j);
            }
            else if (step0) init();
            else { gather(j); pnp_pose(j); triangulate(j); }         // (a stream's track may end in a ghost row: two more hops at most)
            add(j);
        }
        snapshot(j, 1);
        if (ba) {
            { StageTimer t(ctx, ST_SLAM_PREPARE); prepare(j); }
            BaBuf Dj = b.D;
            Dj.chi2 = b.dchi2 + (size_t)2 * j * S; Dj.iterations_run = b.dit + (size_t)j * S; Dj.trials_run = b.dtr + (size_t)j * S;
            { StageTimer t(ctx, ST_SLAM_BA); launch_bundle_adjust(s, Dj, prm, S, o->free_cameras); }
        }
        snapshot(j, 2);
        // step 0 ends with optimize_map (:90); what it wrote back still has to reach the tables the next pair reads
        if (ba || (filt && !step0)) { StageTimer t(ctx, ST_SLAM_FILTER); filter(j, step0 ? 0.0 : o->filter_threshold); }
        snapshot(j, 3);
        { StageTimer t(ctx, ST_SLAM_LIMIT); limit(j); }
        snapshot(j, 4);
        if (d.stats) { StageTimer t(ctx, ST_SLAM_STATS); stats(j); }
    }
    HIPCHK(hipGetLastError());
    return VO_OK;
}

// ------------------------------------------------------------------ the download
// Where a call's results go.  The restart rows are wanted with dims.restart, the carried rows with dims.stream; alive ([S], host)
// where the entry point reads the device's word on whether a sequence is lost.
struct SlamOut {
    double *poses_pnp, *poses; int32_t *n_corr, *n_inl, *status, *n_pts, *n_obs, *n_cam;
    double* chi2; int32_t *ba_iterations_run, *ba_trials_run;
    int32_t *segment, *cause; double *seg_poses_pnp, *seg_poses;
    int32_t *n_carried, *carried_frame; double* carried_poses;
    int32_t* alive;
};

// What follows the loop: the rows to the caller (chi2, ba_iterations_run and ba_trials_run from [step][sequence] to the pair's
// position in the run), a stream's anchor cameras kept for its next call, the wait, the brackets, then host copies of the maps
// and the statistics rows.  multi: the call has sequences (vo_slam_chains_map reports them); snap_seq as in SlamWalk.
static int slam_download(vo_ctx* ctx, bool multi, int steps, int snap_seq, const SlamDims& d, const SlamBufs& b, const std::vector<SlamSeq>& seq, const SlamOut& out)
{
    hipStream_t s = ctx->stream;
    const ChainBuf& cb = b.cb; const SlamBuf& sb = b.sb;
    const size_t S = (size_t)d.S, max_cameras = d.cm - 1;
    std::vector<int32_t> seq_off(S + 1, 0);
    for (size_t q = 0; q < S; q++) seq_off[q + 1] = seq[q].first + seq[q].count;
    const size_t B = (size_t)seq_off[S];
    std::vector<double> hchi(2 * steps * S); std::vector<int32_t> hit(steps * S), htr(steps * S);
    HIPCHK(hipMemcpyAsync(out.poses_pnp, cb.poses, (B + S) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.poses, sb.poses_last, (B + S) * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.n_corr, cb.n_corr, B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.n_inl, cb.n_inl, B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.status, cb.status, B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.n_pts, sb.n_pts, B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.n_obs, sb.n_obs, B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out.n_cam, sb.n_cam, B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hchi.data(), b.dchi2, hchi.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hit.data(), b.dit, hit.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(htr.data(), b.dtr, htr.size() * 4, hipMemcpyDeviceToHost, s));
    if (d.restart) {
        HIPCHK(hipMemcpyAsync(out.segment, cb.rs.segment, B * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out.cause, cb.rs.cause, B * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out.seg_poses_pnp, cb.rs.seg_poses, B * 96, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out.seg_poses, cb.rs.seg_poses_last, B * 96, hipMemcpyDeviceToHost, s));
    }
    if (out.alive) HIPCHK(hipMemcpyAsync(out.alive, cb.alive, S * 4, hipMemcpyDeviceToHost, s));
    for (size_t q = 0; q < S && d.stream; q++) {
        const SlamSeq& e = seq[q];
        const int n = e.count > 0 ? e.sb.st.n_carried : 0;           // (an idle sequence reports none)
        out.n_carried[q] = n;
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(out.carried_frame + q * max_cameras, e.sb.st.carried_frame, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out.carried_poses + q * max_cameras * 12, e.sb.st.carried_poses, (size_t)n * 96, hipMemcpyDeviceToHost, s));
        }
        if (e.count == 0) continue;
        // the anchor camera of the sequence's next call: its last rows of this call (an idle sequence keeps the one it has)
        HIPCHK(hipMemcpyAsync(b.keep + 24 * q, e.cb.poses + (size_t)e.count * 12, 96, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(b.keep + 24 * q + 12, e.sb.poses_last + (size_t)e.count * 12, 96, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    for (size_t q = 0; q < S; q++)                                    // [step][sequence] -> the pair's position in the run
        for (int j = 0; j < seq[q].count; j++) {
            const size_t at = (size_t)j * S + q, p = (size_t)seq_off[q] + j;
            out.chi2[2 * p] = hchi[2 * at]; out.chi2[2 * p + 1] = hchi[2 * at + 1]; out.ba_iterations_run[p] = hit[at]; out.ba_trials_run[p] = htr[at];
        }
    // host copies of every sequence's map, an idle one's too: vo_pairs_run forgot the ones of the call before
    const int cap = (int)d.cap;
    std::vector<LastRun::Map> maps(S);
    for (size_t q = 0; q < S; q++) { int rc = slam_map_download(ctx, seq[q].sb.m, cap, &maps[q], seq[q].first, seq[q].count); if (rc) return rc; }
    LastRun::Map smap;
    if (snap_seq >= 0) { int rc = slam_map_download(ctx, b.snap, cap, &smap, seq[(size_t)snap_seq].first, seq[(size_t)snap_seq].count); if (rc) return rc; }
    ctx->last.map[0] = maps[0];                                       // what vo_slam_map reports: sequence 0, and its snapshot if it has one
    if (snap_seq == 0) ctx->last.map[1] = smap;
    if (multi) {
        ctx->last.seq_map = std::move(maps);
        if (snap_seq >= 0) { ctx->last.snap_map = std::move(smap); ctx->last.snap_seq = snap_seq; }
    }
    // ... and where the lists themselves still lie, for vo_map_from_slam
    LastRun::DevMaps& dv = ctx->last.dev;
    dv = LastRun::DevMaps();
    for (size_t q = 0; q < S; q++) dv.seq.push_back({seq[q].sb.m.pt_key, seq[q].sb.m.pt_xyz});
    if (snap_seq >= 0) dv.snap = {b.snap.pt_key, b.snap.pt_xyz};
    dv.stream = d.stream; dv.n_keys = (int)((size_t)d.F * d.cap); dv.epoch = ctx->scratch_epoch;
    if (d.stats) { int rc = slam_stats_download(ctx, b.stats, std::move(seq_off)); if (rc) return rc; }
    return VO_OK;
}

// ------------------------------------------------------------------ one chain, in the scratch buffer
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
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    // capacities from the configuration: a pair adds at most one point and two observations per match
    SlamDims d = slam_dims(ctx, 1, F, (size_t)F, cap, o);
    d.np = {(size_t)F * cap}; d.no = {(size_t)2 * B * cap}; d.P = (size_t)B; d.steps = (size_t)B;
    d.snapshot = o->snapshot_pair >= 0; d.snap_np = d.np[0]; d.snap_no = d.no[0];
    if (d.np[0] >= ((size_t)1 << 31) || d.npair(0) >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the map's lists would not fit 32-bit indices");
    SlamBufs b;
    rc = slam_place_scratch(ctx, d, b); if (rc) return rc;
    HIPCHK(hipMemsetAsync(ctx->scratch.p, 0, b.bytes, s));           // empty feature_mapper, empty map, no cameras, zero results
    HIPCHK(hipMemcpyAsync(b.dK, K, 72, hipMemcpyHostToDevice, s));
    const std::vector<SlamSeq> seq{slam_seq(d, b, 0, 0, B)};
    const int snap_seq = d.snapshot ? 0 : -1;
    rc = slam_walk(ctx, SlamWalk{FAM_CHAIN, false, F, B, snap_seq, SlamCarry{}, false}, d, b, seq, K, o); if (rc) return rc;
    const SlamOut out{poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2, ba_iterations_run, ba_trials_run,
                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return slam_download(ctx, false, B, snap_seq, d, b, seq, out);
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
// k_slam_carry restate the keys (slam_kernels.hip) and runs a later step for every pair.  The work buffers keep what the last
// step left in them, as they do between two steps of one call.
static int slam_stream_allocate(vo_ctx* ctx, SlamStream& st, bool restart, int F, int cap, int max_pairs, int total, const vo_slam_opts* o, const double* K)
{
    // the slot-keyed tables have two ghost rows behind the F slots.  Lists: a pair adds at most one point per match; a camera takes
    // at most kp_cap observations as a pair's second frame and kp_cap as the next pair's first (one-to-one matches), and the map
    // holds at most max_cameras + 1 cameras — or every pair's two observations per match, if the stream is shorter than that.
    SlamDims d = slam_dims(ctx, 1, F, (size_t)F + 2, cap, o);
    d.np = {((size_t)total + 1) * cap}; d.no = {(size_t)2 * cap * std::min(d.cm, (size_t)total)}; d.P = (size_t)max_pairs; d.steps = d.P;
    d.stream = true; d.restart = restart; d.snapshot = true; d.snap_np = d.np[0]; d.snap_no = d.no[0];
    if (F + 2 >= (1 << 20)) FAIL(VO_ERR_INVALID, "too many frames for the packed track table");
    if (d.np[0] >= ((size_t)1 << 31) || d.npair(0) >= ((size_t)1 << 31) || d.fc() >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the map's lists would not fit 32-bit indices");
    const int rc = slam_place_stream(ctx, st, d); if (rc) return rc;
    st.restart = restart;
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

// the buffers as a stream's call finds them: a first call clears everything, as vo_slam_chain clears the scratch buffer; a resumed
// one the per-pair outputs only
static int slam_stream_clear(vo_ctx* ctx, const SlamStream& st, int resume, const double* K)
{
    hipStream_t s = ctx->stream;
    if (!resume) {
        HIPCHK(hipMemsetAsync(st.base, 0, st.b.bytes, s));            // empty feature_mapper, empty maps, no cameras, zero results
        HIPCHK(hipMemcpyAsync(st.b.dK, K, 72, hipMemcpyHostToDevice, s));
    } else HIPCHK(hipMemsetAsync(st.base + st.b.call0, 0, st.b.bytes - st.b.call0, s));
    return VO_OK;
}

// ------------------------------------------------------------------ a stream's descriptor store (vo_set_stream_rows)
// One more allocation of the stream's lifetime, beside slam_layout's and not inside it: the walk's kernels never see it.  It is made
// by the call that starts a vo_slam_stream while the setting is on; vo_slam_stream_restart and vo_slam_streams have none.
extern "C" int vo_set_stream_rows(vo_ctx* ctx, int64_t capacity_rows)
{
    if (!ctx) return VO_ERR_INVALID;
    if (capacity_rows < -1) FAIL(VO_ERR_INVALID, "stream rows must be 0 (no store), -1 (a row for every feature the stream can hold) or a number of rows, got %lld", (long long)capacity_rows);
    ctx->stream_rows = capacity_rows;
    return VO_OK;
}

static int stream_rows_allocate(vo_ctx* ctx, SlamStream& st, int64_t setting, bool sift)
{
    SlamStream::Store& so = st.store;
    StreamRows& d = so.d;
    const size_t feats = st.dims.np[0];                               // (total_pairs + 1) kp_cap: below 2^31 (slam_stream_allocate)
    const int64_t capacity = setting < 0 ? (int64_t)feats : setting;
    if (capacity > INT32_MAX) FAIL(VO_ERR_INVALID, "vo_slam_stream: a descriptor store holds at most 2^31 - 1 rows (vo_set_stream_rows), got %lld", (long long)capacity);
    d.D = sift ? 128 : 32; d.capacity = (int)capacity; d.kp_cap = st.cap; d.frames = st.total + 1;
    d.sel_cap = (int)std::min(feats, (size_t)VO_MAP_MAX_POINTS);
    ScratchLayout sc;
    sc.take(&d.rows, (size_t)capacity * d.D); sc.take(&d.row_of, feats); sc.take(&d.counters, 2);
    sc.take(&d.sel_key, (size_t)d.sel_cap); sc.take(&d.sel_xyz, (size_t)d.sel_cap * 3); sc.take(&d.sel_cnt, 2);
    uint8_t* base = nullptr;
    HIPCHK(so.mem.alloc(&base, sc.bytes));
    sc.place_at(base);
    HIPCHK(hipMemsetAsync(d.row_of, 0xFF, feats * sizeof(int), ctx->stream));     // -1: no feature has a row
    HIPCHK(hipMemsetAsync(d.counters, 0, 2 * sizeof(int), ctx->stream));
    so.counters[0] = so.counters[1] = 0;
    so.on = true;
    return VO_OK;
}

// The end of a vo_slam_stream call with a store: the rows of the points born in it, while their frames are in their slots.  On the
// call's stream behind the walk; the counters come back with the call's results (slam_download waits).
static int stream_rows_append(vo_ctx* ctx, SlamStream& st, const SlamMap& m, int frame0)
{
    SlamStream::Store& so = st.store;
    const Batch b = batch(ctx);
    {
        StageTimer t(ctx, ST_MISC);
        launch_stream_rows_append(ctx->stream, m, so.d, st.dims.np[0], b.desc, st.F * st.cap, frame0, so.counters[0], so.counters[1]);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(so.counters, so.d.counters, sizeof(so.counters), hipMemcpyDeviceToHost, ctx->stream));
    return VO_OK;
}

// ------------------------------------------------------------------ a stream's archive of evicted points (vo_set_stream_archive)
// A third allocation of the stream's lifetime, made with the store's by the call that starts a vo_slam_stream while both settings are
// on.  The one kernel of the walk that knows it is k_slam_limit_stream_archive, launched in k_slam_limit_stream's place.
extern "C" int vo_set_stream_archive(vo_ctx* ctx, int64_t capacity_points)
{
    if (!ctx) return VO_ERR_INVALID;
    if (capacity_points < -1) FAIL(VO_ERR_INVALID, "a stream archive must be 0 (none), -1 (an entry for every feature the stream can hold) or a number of entries, got %lld", (long long)capacity_points);
    ctx->stream_archive = capacity_points;
    return VO_OK;
}

static int stream_archive_allocate(vo_ctx* ctx, SlamStream& st, int64_t setting)
{
    SlamStream::Archive& ar = st.archive;
    StreamArchive& d = ar.d;
    const size_t feats = st.dims.np[0];                               // (total_pairs + 1) kp_cap: below 2^31 (slam_stream_allocate)
    const int64_t capacity = setting < 0 ? (int64_t)feats : setting;
    if (capacity > INT32_MAX) FAIL(VO_ERR_INVALID, "vo_slam_stream: an archive holds at most 2^31 - 1 entries (vo_set_stream_archive), got %lld", (long long)capacity);
    d.D = st.store.d.D; d.capacity = (int)capacity; d.sel_cap = VO_MAP_MAX_POINTS;
    const size_t tiles = ((size_t)capacity + SA_TILE - 1) / SA_TILE;
    ScratchLayout sc;
    sc.take(&d.rows, (size_t)capacity * d.D); sc.take(&d.xyz, (size_t)capacity * 3); sc.take(&d.feature, (size_t)capacity * 2);
    sc.take(&d.evicted_at, (size_t)capacity); sc.take(&d.has_row, (size_t)capacity); sc.take(&d.counters, 2); sc.take(&d.tile_cnt, tiles * 2);
    sc.take(&d.sel_key, (size_t)d.sel_cap); sc.take(&d.sel_xyz, (size_t)d.sel_cap * 3); sc.take(&d.sel_cnt, 2);
    uint8_t* base = nullptr;
    HIPCHK(ar.mem.alloc(&base, sc.bytes));
    sc.place_at(base);
    HIPCHK(hipMemsetAsync(base, 0, sc.bytes, ctx->stream));           // no entries; an entry without a row reads zeros
    ar.counters[0] = ar.counters[1] = 0;
    ar.on = true;
    return VO_OK;
}

// the live vo_slam_stream with an archive, nullptr (and the reason in ctx->err) if there is none
static SlamStream* stream_with_archive(vo_ctx* ctx, const char* who)
{
    SlamStream& st = ctx->stream_map;
    const char* why = nullptr;
    if (!st.live) why = "there is no live stream (none was started, or a configure or vo_slam_chain* call dropped it)";
    else if (st.multi || st.restart) why = "the live stream was started by vo_slam_stream_restart or vo_slam_streams, which keep no archive";
    else if (!st.archive.on) why = "the live stream was started without an archive (vo_set_stream_archive before vo_slam_stream(resume = 0))";
    if (why) { snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, why); return nullptr; }
    return &st;
}

extern "C" int vo_stream_archive_info(vo_ctx* ctx, int64_t* capacity, int64_t* stored, int64_t* dropped)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!capacity || !stored || !dropped) FAIL(VO_ERR_INVALID, "bad arguments");
    const SlamStream* st = stream_with_archive(ctx, "vo_stream_archive_info");
    if (!st) return VO_ERR_INVALID;
    *capacity = st->archive.d.capacity; *stored = st->archive.counters[0]; *dropped = st->archive.counters[1];
    return VO_OK;
}

extern "C" int vo_stream_archive_read(vo_ctx* ctx, int64_t first, int64_t n, int32_t* feature, double* xyz, int32_t* evicted_at, int32_t* has_row, uint8_t* rows)
{
    if (!ctx) return VO_ERR_INVALID;
    const SlamStream* st = stream_with_archive(ctx, "vo_stream_archive_read");
    if (!st) return VO_ERR_INVALID;
    const StreamArchive& d = st->archive.d;
    if (first < 0 || n < 0 || first + n > st->archive.counters[0])
        FAIL(VO_ERR_INVALID, "vo_stream_archive_read: entries [%lld, %lld + %lld) are not among the %d the archive holds", (long long)first, (long long)first, (long long)n, st->archive.counters[0]);
    if (n == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t f = (size_t)first, c = (size_t)n;
    if (feature) HIPCHK(hipMemcpyAsync(feature, d.feature + 2 * f, c * 8, hipMemcpyDeviceToHost, s));
    if (xyz) HIPCHK(hipMemcpyAsync(xyz, d.xyz + 3 * f, c * 24, hipMemcpyDeviceToHost, s));
    if (evicted_at) HIPCHK(hipMemcpyAsync(evicted_at, d.evicted_at + f, c * 4, hipMemcpyDeviceToHost, s));
    if (has_row) HIPCHK(hipMemcpyAsync(has_row, d.has_row + f, c * 4, hipMemcpyDeviceToHost, s));
    if (rows) HIPCHK(hipMemcpyAsync(rows, d.rows + f * d.D, c * d.D, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VO_OK;
}

// the live vo_slam_stream with a store, nullptr (and the reason in ctx->err) if there is none
static SlamStream* stream_with_rows(vo_ctx* ctx, const char* who)
{
    SlamStream& st = ctx->stream_map;
    const char* why = nullptr;
    if (!st.live) why = "there is no live stream (none was started, or a configure or vo_slam_chain* call dropped it)";
    else if (st.multi || st.restart) why = "the live stream was started by vo_slam_stream_restart or vo_slam_streams, which keep no descriptor store";
    else if (!st.store.on) why = "the live stream was started without a descriptor store (vo_set_stream_rows before vo_slam_stream(resume = 0))";
    if (why) { snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, why); return nullptr; }
    return &st;
}

extern "C" int vo_stream_rows_info(vo_ctx* ctx, int64_t* capacity, int64_t* stored, int64_t* dropped)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!capacity || !stored || !dropped) FAIL(VO_ERR_INVALID, "bad arguments");
    const SlamStream* st = stream_with_rows(ctx, "vo_stream_rows_info");
    if (!st) return VO_ERR_INVALID;
    *capacity = st->store.d.capacity; *stored = st->store.counters[0]; *dropped = st->store.counters[1];
    return VO_OK;
}

// The relocaliser's map from the live stream's end map, at any time while the stream lives: k_stream_rows_select writes the store
// rows of the window's points as a key list and their coordinates as a dense list, then the one staging path runs with the store as
// the source of the rows.  Reads the stream's lists and writes the store's own selection buffers: the stream is left as it was.
extern "C" int vo_map_from_stream(vo_ctx* ctx, int frame_first, int frame_end, int32_t* n_staged, int32_t* n_without_row)
{
    if (!ctx) return VO_ERR_INVALID;
    ctx->map.staged = false; ctx->map.last_Q = 0; ctx->map.al.last_Q = 0;          // a failed call leaves no staged map
    if (!n_staged || !n_without_row) FAIL(VO_ERR_INVALID, "bad arguments");
    *n_staged = 0; *n_without_row = 0;
    SlamStream* st = stream_with_rows(ctx, "vo_map_from_stream");
    if (!st) return VO_ERR_INVALID;
    if (frame_first < 0 || (frame_end >= 0 && frame_end < frame_first))
        FAIL(VO_ERR_INVALID, "vo_map_from_stream: the window [%d, %d) is not one (frame_first >= 0; frame_end >= frame_first, or negative for no upper bound)", frame_first, frame_end);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const StreamRows& d = st->store.d;
    const SlamMap& m = st->b.sb.m;                                    // (one sequence: the whole arrays)
    launch_stream_rows_select(s, m, d, st->dims.np[0], frame_first, frame_end);
    HIPCHK(hipGetLastError());
    int32_t cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, d.sel_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_without_row = cnt[1];
    if (cnt[0] > VO_MAP_MAX_POINTS)
        FAIL(VO_ERR_UNSUPPORTED, "vo_map_from_stream: a staged map holds at most %d points, the window [%d, %d) selects %d", VO_MAP_MAX_POINTS, frame_first, frame_end, cnt[0]);
    const int rc = map_stage_device(ctx, d.rows, d.sel_key, d.capacity, d.sel_xyz, cnt[0], "vo_map_from_stream"); if (rc) return rc;
    *n_staged = cnt[0];
    return VO_OK;
}

// vo_map_from_stream with the archived points of the window behind the live ones (with_live) or alone.  The live part is
// k_stream_rows_select's, unchanged; its count stays on the device, where the archive's emit pass starts from it; then one wait for
// the four counts, and the two parts go through the one staging path.
extern "C" int vo_map_from_stream_archive(vo_ctx* ctx, int frame_first, int frame_end, int with_live, int32_t* n_staged, int32_t* n_archived, int32_t* n_without_row)
{
    if (!ctx) return VO_ERR_INVALID;
    ctx->map.staged = false; ctx->map.last_Q = 0; ctx->map.al.last_Q = 0;          // a failed call leaves no staged map
    if (!n_staged || !n_archived || !n_without_row) FAIL(VO_ERR_INVALID, "bad arguments");
    *n_staged = 0; *n_archived = 0; *n_without_row = 0;
    SlamStream* st = stream_with_archive(ctx, "vo_map_from_stream_archive");
    if (!st) return VO_ERR_INVALID;
    if (frame_first < 0 || (frame_end >= 0 && frame_end < frame_first))
        FAIL(VO_ERR_INVALID, "vo_map_from_stream_archive: the window [%d, %d) is not one (frame_first >= 0; frame_end >= frame_first, or negative for no upper bound)", frame_first, frame_end);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const StreamRows& d = st->store.d;
    const StreamArchive& a = st->archive.d;
    const SlamMap& m = st->b.sb.m;
    if (with_live) launch_stream_rows_select(s, m, d, st->dims.np[0], frame_first, frame_end);
    launch_stream_archive_select(s, a, st->archive.counters[0], frame_first, frame_end, with_live ? d.sel_cnt : nullptr);
    HIPCHK(hipGetLastError());
    int32_t live[2] = {0, 0}, arc[2] = {0, 0};
    if (with_live) HIPCHK(hipMemcpyAsync(live, d.sel_cnt, sizeof(live), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(arc, a.sel_cnt, sizeof(arc), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_without_row = live[1] + arc[1];
    const int64_t total = (int64_t)live[0] + arc[0];
    if (total > VO_MAP_MAX_POINTS)
        FAIL(VO_ERR_UNSUPPORTED, "vo_map_from_stream_archive: a staged map holds at most %d points, the window [%d, %d) selects %d live and %d archived", VO_MAP_MAX_POINTS,
             frame_first, frame_end, live[0], arc[0]);
    const int rc = map_stage_device2(ctx, d.rows, d.sel_key, d.capacity, d.sel_xyz, live[0], MapPart2{a.rows, a.sel_key, a.capacity, a.sel_xyz}, (int)total,
                                     "vo_map_from_stream_archive");
    if (rc) return rc;
    *n_staged = (int32_t)total; *n_archived = arc[0];
    return VO_OK;
}

// vo_slam_stream and vo_slam_stream_restart.  restart: vo_slam_chains_restart's step for the one chain of the stream, and the alive
// flag and the segment state words stay on the device between the calls.
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
        if (st.dims.stats != (ctx->slam_stats != 0)) FAIL(VO_ERR_INVALID, "%s: the stream was started with statistics %s (vo_set_slam_stats) and is continued only so", who, st.dims.stats ? "on" : "off");
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
    if (!resume && !restart && ctx->stream_archive != 0 && ctx->stream_rows == 0)
        FAIL(VO_ERR_INVALID, "vo_slam_stream: an archive (vo_set_stream_archive) needs the descriptor store (vo_set_stream_rows): the rows of earlier calls' points come from it");
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    if (!resume) {
        rc = slam_stream_allocate(ctx, st, restart, F, cap, batch(ctx).max_pairs, total_pairs, o, K);
        if (!rc && !restart && ctx->stream_rows != 0) rc = stream_rows_allocate(ctx, st, ctx->stream_rows, batch(ctx).sift);
        if (!rc && !restart && ctx->stream_archive != 0) rc = stream_archive_allocate(ctx, st, ctx->stream_archive);
        if (rc) { drop_slam_stream(ctx); return rc; }
    }
    rc = slam_stream_clear(ctx, st, resume, K); if (rc) return rc;
    // (after a call that ended lost the anchor frame is not in the map: every camera of the map is a carried one)
    const int carried = !resume ? 0 : restart && st.lost ? st.last_ncam : st.last_ncam - 1;
    const std::vector<SlamSeq> seq{slam_seq(st.dims, st.b, 0, 0, B, resume ? st.done : 0, carried)};
    const int snap_seq = o->snapshot_pair >= 0 ? 0 : -1;
    st.live = false;                                                  // (until the call has come through)
    const int gn = F + (st.carries & 1);
    SlamArchive sa{};
    if (st.archive.on) {
        const StreamRows& sr = st.store.d;
        sa = SlamArchive{st.archive.d, batch(ctx).desc, st.F * st.cap, sr.rows, sr.capacity, sr.row_of, sr.kp_cap, sr.frames};
    }
    const SlamWalk w{restart ? FAM_STREAM_RESTART : FAM_STREAM, resume != 0, F + 2, B, snap_seq, SlamCarry{cap, F, st.anchor, gn, 2 * F + 1 - gn, st.b.keep}, false,
                     st.archive.on ? &sa : nullptr};
    rc = slam_walk(ctx, w, st.dims, st.b, seq, K, o); if (rc) return rc;
    if (st.archive.on) HIPCHK(hipMemcpyAsync(st.archive.counters, st.archive.d.counters, sizeof(st.archive.counters), hipMemcpyDeviceToHost, ctx->stream));
    if (st.store.on) { rc = stream_rows_append(ctx, st, seq[0].sb.m, resume ? st.done : 0); if (rc) return rc; }
    int32_t alive = 1;
    const SlamOut out{poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2, ba_iterations_run, ba_trials_run,
                      segment, cause, seg_poses_pnp, seg_poses, n_carried, carried_frame, carried_poses, restart ? &alive : nullptr};
    rc = slam_download(ctx, false, B, snap_seq, st.dims, st.b, seq, out); if (rc) return rc;
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

// vo_slam_chains and vo_slam_chains_restart.  restart: a sequence that loses tracking starts a new map from the next usable pair,
// decided on the device (k_chain_gather, k_chain_pose) and done by k_slam_restart_seqs, which joins every step.
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
    const int B = seq_off[S];
    rc = slam_opts_check(ctx, o, K, seq_off[ss + 1] - seq_off[ss], "vo_slam_chains"); if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    // capacities from the configuration: a pair adds at most one point and two observations per match
    SlamDims d = slam_dims(ctx, S, F, (size_t)F, cap, o);
    int maxB = 0;
    for (int q = 0; q < S; q++) {
        const int Bq = seq_off[q + 1] - seq_off[q];
        maxB = std::max(maxB, Bq);
        d.np.push_back((size_t)(Bq + 1) * cap); d.no.push_back((size_t)2 * Bq * cap);
    }
    d.P = (size_t)B; d.steps = (size_t)maxB; d.restart = restart;
    d.snapshot = snap_on; d.snap_np = d.np[(size_t)ss]; d.snap_no = d.no[(size_t)ss];
    if (d.NP() >= ((size_t)1 << 31) || d.NPAIR() >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the maps' lists would not fit 32-bit indices");
    SlamBufs b;
    rc = slam_place_scratch(ctx, d, b); if (rc) return rc;
    std::vector<SlamSeq> seq;
    for (int q = 0; q < S; q++) seq.push_back(slam_seq(d, b, q, seq_off[q], seq_off[q + 1] - seq_off[q]));
    HIPCHK(hipMemsetAsync(ctx->scratch.p, 0, b.bytes, s));           // empty feature_mapper, empty maps, no cameras, zero results
    HIPCHK(hipMemcpyAsync(b.dK, K, 72, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.dseq, seq.data(), (size_t)S * sizeof(SlamSeq), hipMemcpyHostToDevice, s));
    const int snap_seq = snap_on ? ss : -1;
    rc = slam_walk(ctx, SlamWalk{restart ? FAM_SEQS_RESTART : FAM_SEQS, false, F, maxB, snap_seq, SlamCarry{}, false}, d, b, seq, K, o); if (rc) return rc;
    const SlamOut out{poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2, ba_iterations_run, ba_trials_run,
                      segment, cause, seg_poses_pnp, seg_poses, nullptr, nullptr, nullptr, nullptr};
    return slam_download(ctx, true, maxB, snap_seq, d, b, seq, out);
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
    const size_t R = (size_t)F + 2 * (size_t)S;
    if (R >= ((size_t)1 << 20)) FAIL(VO_ERR_INVALID, "vo_slam_streams: max_frames + 2 S = %zu rows are too many for the packed track table", R);
    SlamDims d = slam_dims(ctx, S, F, R, cap, o);
    st.seq.assign((size_t)S, SlamStream::Seq());
    st.rows.assign((size_t)S * ((size_t)max_pairs + 1), 0);
    d.P = (size_t)max_pairs; d.steps = d.P; d.stream = true; d.restart = true; d.snapshot = true;   // (the snapshot: room for the largest sequence)
    for (int q = 0; q < S; q++) {
        st.seq[(size_t)q].total = total[q]; st.seq[(size_t)q].capacity = total[q];
        d.np.push_back(((size_t)total[q] + 1) * cap); d.no.push_back((size_t)2 * cap * std::min(d.cm, (size_t)total[q]));
        d.snap_np = std::max(d.snap_np, d.np.back()); d.snap_no = std::max(d.snap_no, d.no.back());
    }
    if (d.NP() >= ((size_t)1 << 31) || d.NPAIR() >= ((size_t)1 << 31) || d.fc() >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "the maps' lists would not fit 32-bit indices");
    const int rc = slam_place_stream(ctx, st, d); if (rc) return rc;
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
        if (st.dims.stats != (ctx->slam_stats != 0)) FAIL(VO_ERR_INVALID, "%s: the stream was started with statistics %s (vo_set_slam_stats) and is continued only so", who, st.dims.stats ? "on" : "off");
    }
    int F, cap;
    int rc = streams_check(ctx, resume, S, seq_off, &F, &cap); if (rc) return rc;
    const bool snap_on = o->snapshot_pair >= 0;        // (snapshot_seq is ignored otherwise)
    if (snap_on && (snapshot_seq < 0 || snapshot_seq >= S)) FAIL(VO_ERR_INVALID, "snapshot_seq must be a sequence of the call (0 .. %d), got %d", S - 1, snapshot_seq);
    const int ss = snap_on ? snapshot_seq : 0;
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
    }
    rc = slam_stream_clear(ctx, st, resume, K); if (rc) return rc;
    const SlamBufs& b = st.b;
    const size_t row_cap = (size_t)max_pairs + 1;
    const int R = F + 2 * S, gpar = st.carries & 1;
    // the descriptors of this call: a sequence's ranges of the lists, and its rows of the call's outputs
    std::vector<SlamSeq> seq; std::vector<SlamSeqCarry> car((size_t)S); std::vector<int32_t> hrows(st.rows);
    std::vector<SlamSeat> seat((size_t)S);
    bool seats = false;                                               // some seat is vacant: the carry launch is the seats form
    for (int q = 0; q < S; q++) {
        const SlamStream::Seq& h = st.seq[(size_t)q];
        // (after a call that ended lost the anchor frame is not in the map: every camera of the map is a carried one)
        seq.push_back(slam_seq(st.dims, b, q, seq_off[q], seq_off[q + 1] - seq_off[q], resume ? h.done : 0, !resume ? 0 : h.lost ? h.last_ncam : h.last_ncam - 1));
        SlamSeqCarry& k = car[(size_t)q];
        const int gn = F + 2 * q + gpar, go = F + 2 * q + 1 - gpar;
        k.c = SlamCarry{cap, F, h.anchor, gn, go, b.keep + (size_t)24 * q};
        k.hops = R; k.rows = b.drows + (size_t)q * row_cap;
        hrows[(size_t)q * row_cap + h.n_rows] = go; k.n_rows = h.n_rows + 1;
        // seats: a vacant seat is not carried.  One replaced since the last call is reset — it gives up the slots of its last call's
        // frames (k.rows without the ghost row above), its old anchor row and both ghost rows; one already reset is left alone.
        SlamSeat& t = seat[(size_t)q];
        t = SlamSeat{SEAT_CARRY, 0, {0, 0, 0}, b.keep + (size_t)24 * q};
        if (resume && h.vacant) {
            seats = true;
            t.mode = h.clean ? SEAT_VACANT : SEAT_RESET;
            k.n_rows = h.n_rows;
            if (h.old_anchor >= 0) t.rows[t.n_rows++] = h.old_anchor;
            t.rows[t.n_rows++] = gn; t.rows[t.n_rows++] = go;
        }
    }
    HIPCHK(hipMemcpyAsync(b.dseq, seq.data(), (size_t)S * sizeof(SlamSeq), hipMemcpyHostToDevice, s));
    st.live = false;                                                  // (until the call has come through)
    if (resume) {
        HIPCHK(hipMemcpyAsync(b.dcar, car.data(), (size_t)S * sizeof(SlamSeqCarry), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(b.drows, hrows.data(), hrows.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (seats) HIPCHK(hipMemcpyAsync(b.dseat, seat.data(), (size_t)S * sizeof(SlamSeat), hipMemcpyHostToDevice, s));
    }
    const int snap_seq = snap_on ? ss : -1;
    rc = slam_walk(ctx, SlamWalk{FAM_STREAMS, resume != 0, R, maxB, snap_seq, SlamCarry{}, seats}, st.dims, b, seq, K, o); if (rc) return rc;
    std::vector<int32_t> alive((size_t)S, 1);
    const SlamOut out{poses_pnp, poses, n_corr, n_inl, status, n_pts, n_obs, n_cam, chi2, ba_iterations_run, ba_trials_run,
                      segment, cause, seg_poses_pnp, seg_poses, n_carried, carried_frame, carried_poses, alive.data()};
    rc = slam_download(ctx, true, maxB, snap_seq, st.dims, b, seq, out); if (rc) return rc;
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
    SlamStream& st = ctx->stream_map;
    rc = slam_streams_allocate(ctx, st, S, b.max_frames, b.kp_cap, b.max_pairs, total_pairs, o, K);
    if (rc) { drop_slam_stream(ctx); return rc; }
    rc = [&]() -> int {
        const int rc_clear = slam_stream_clear(ctx, st, 0, K); if (rc_clear) return rc_clear;
        HIPCHK(hipStreamSynchronize(ctx->stream));
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

// The relocaliser's map from a chain that has just run: the coordinates as the map's list holds them and, per point, the
// descriptor row of its owning feature (TrackedPoint.descriptor = match.descriptor1, src/visual_slam.py:72-76) gathered from the
// slots by k_map_gather — pt_key is slot * kp_cap + keypoint already, the device form of pt_feature -> chain frame -> slot.  Device
// to device: the host contributes the point count it already holds.
extern "C" int vo_map_from_slam(vo_ctx* ctx, int seq, int which)
{
    if (!ctx) return VO_ERR_INVALID;
    const LastRun& l = ctx->last;
    const SlamStream& st = ctx->stream_map;
    if (st.live && !st.multi && st.store.on && seq == 0 && (which == 0 || which == 1)) {   // a vo_slam_stream with a descriptor store: the latest vo_slam_* call is its
        if (which == 1) FAIL(VO_ERR_UNSUPPORTED, "vo_map_from_slam: a stream's snapshot is not staged: the store serves the map at the end of the call");
        int32_t n = 0, without = 0;
        return vo_map_from_stream(ctx, 0, -1, &n, &without);
    }
    const bool multi = !l.seq_map.empty();
    if (!multi && seq != 0) FAIL(VO_ERR_INVALID, "the most recent vo_slam_* call had one sequence: seq must be 0, got %d", seq);
    const LastRun::Map* m = multi ? slam_chains_map_of(ctx, seq, which) : slam_map_of(ctx, which);
    if (!m) return VO_ERR_INVALID;
    const LastRun::DevMaps& dv = l.dev;
    if (dv.stream)
        FAIL(VO_ERR_UNSUPPORTED, "vo_map_from_slam: a stream's map names frames that have left their slots, and their descriptor rows with them "
                                 "(vo_slam_stream keeps them with vo_set_stream_rows: vo_map_from_stream)");
    if (dv.epoch != ctx->scratch_epoch || (size_t)seq >= dv.seq.size())
        FAIL(VO_ERR_INVALID, "vo_map_from_slam: another call has used the scratch buffer the chain's map lay in; call it right after the chain");
    const LastRun::DevMaps::Lists& L = which == 1 ? dv.snap : dv.seq[(size_t)seq];
    const Batch b = batch(ctx);
    return map_stage_device(ctx, b.desc, L.pt_key, dv.n_keys, L.pt_xyz, (int)(m->points.size() / 3), "vo_map_from_slam");
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
