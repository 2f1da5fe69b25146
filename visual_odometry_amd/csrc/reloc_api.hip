// reloc_api.hip — the vo_map_* entry points of libvo_hip.so: a frame placed in a map by its descriptors (include/vo_hip.h,
// "relocalisation", "guided relocalisation").  Host code only; the kernels are reloc_kernels.hip, guided_kernels.hip and, unchanged,
// k_pnp_ransac (pnp_kernels.hip).
// vo_map_from_slam is in slam_api.hip, beside the maps it reads; it stages through map_stage_device like vo_map_stage.
#include "vo_host.h"

// Room for npt rows and for the work of max_pairs queries of kp_cap keypoints.  The allocation is kept while it fits (rows past npt
// then keep what a larger map left); otherwise it is released as a whole and made again.
static int map_reserve(vo_ctx* ctx, const Batch& b, int npt)
{
    MapState& M = ctx->map;
    const int D = b.sift ? 128 : 32, rows = std::max(256, (npt + 255) & ~255);
    if (M.m.rows && M.m.D == D && M.m.cap_rows >= rows && M.Q_cap >= b.max_pairs && M.kp_cap == b.kp_cap) return VO_OK;
    if ((size_t)b.max_pairs * b.kp_cap >= ((size_t)1 << 31) || (size_t)b.max_pairs * rows >= ((size_t)1 << 31))
        FAIL(VO_ERR_INVALID, "max_pairs x kp_cap and max_pairs x map rows must fit 32-bit indices");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    drop_map(ctx);
    const size_t R = (size_t)rows, Q = (size_t)b.max_pairs, C = (size_t)b.kp_cap;
    DevList& mem = M.mem; MapBuf& m = M.m; RelocBuf& r = M.r;
    HIPCHK(mem.alloc(&m.rows, R * D)); HIPCHK(mem.alloc(&m.xyz, R * 3)); HIPCHK(mem.alloc(&m.flag, 1));
    if (b.sift) {
        HIPCHK(mem.alloc(&m.img, R * 128)); HIPCHK(mem.alloc(&m.norms, R));
        HIPCHK(hipMemsetAsync(m.img, 0, R * 128, ctx->stream)); HIPCHK(hipMemsetAsync(m.norms, 0, R * sizeof(int), ctx->stream));
    }
    HIPCHK(hipMemsetAsync(m.rows, 0, R * D, ctx->stream));
    HIPCHK(mem.alloc(&r.slots, Q)); HIPCHK(mem.alloc(&r.nn_idx, Q * C)); HIPCHK(mem.alloc(&r.nn_dist, Q * C)); HIPCHK(mem.alloc(&r.rn_idx, Q * R));
    HIPCHK(mem.alloc(&r.nn_dist2, Q * C)); HIPCHK(mem.alloc(&r.m_d2, Q * C));
    HIPCHK(mem.alloc(&r.m_q, Q * C)); HIPCHK(mem.alloc(&r.m_t, Q * C)); HIPCHK(mem.alloc(&r.m_d, Q * C)); HIPCHK(mem.alloc(&r.m_count, Q));
    HIPCHK(mem.alloc(&r.obj, Q * C * 3)); HIPCHK(mem.alloc(&r.img, Q * C * 2)); HIPCHK(mem.alloc(&r.off, 2 * Q));
    HIPCHK(mem.alloc(&r.rvec, 3 * Q)); HIPCHK(mem.alloc(&r.tvec, 3 * Q)); HIPCHK(mem.alloc(&r.mask, Q * C));
    HIPCHK(mem.alloc(&r.ninl, Q)); HIPCHK(mem.alloc(&r.status, Q)); HIPCHK(mem.alloc(&r.poses, 12 * Q)); HIPCHK(mem.alloc(&M.dK, 9));
    GuidedBuf& g = M.g;                                     // vo_map_localize_guided's: the keypoint grid, the claim table, the priors
    HIPCHK(mem.alloc(&g.cell_off, Q * (GUIDED_CELLS + 1))); HIPCHK(mem.alloc(&g.cell_kp, Q * C)); HIPCHK(mem.alloc(&g.box, 4 * Q));
    HIPCHK(mem.alloc(&g.claim, Q * C)); HIPCHK(mem.alloc(&g.pt_d2, Q * R)); HIPCHK(mem.alloc(&g.prior, 12 * Q));
    HIPCHK(mem.alloc(&g.skip, Q)); HIPCHK(mem.alloc(&g.n_seen, Q));
    m.D = D; m.cap_rows = rows; m.npt = 0;
    M.Q_cap = b.max_pairs; M.kp_cap = b.kp_cap;
    return VO_OK;
}

int map_stage_device(vo_ctx* ctx, const uint8_t* src, const int* key, int n_keys, const double* xyz, int npt, const char* who)
{
    return map_stage_device2(ctx, src, key, n_keys, xyz, npt, MapPart2{nullptr, nullptr, 0, nullptr}, npt, who);
}

int map_stage_device2(vo_ctx* ctx, const uint8_t* src, const int* key, int n_keys, const double* xyz, int n0, const MapPart2& p2, int npt, const char* who)
{
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "%s: vo_batch_configure[_sift] has not been called", who);
    if (npt < 0 || n0 < 0 || n0 > npt) FAIL(VO_ERR_INVALID, "%s: npt must not be negative", who);
    if (npt > VO_MAP_MAX_POINTS) FAIL(VO_ERR_UNSUPPORTED, "%s: a staged map holds at most %d points, got %d", who, VO_MAP_MAX_POINTS, npt);
    HIPCHK(hipSetDevice(ctx->device));
    int rc = map_reserve(ctx, b, npt); if (rc) return rc;
    MapState& M = ctx->map;
    hipStream_t s = ctx->stream;
    M.staged = false; M.last_Q = 0; M.al.last_Q = 0; M.loc_ok = false;
    M.m.npt = npt;
    HIPCHK(hipMemsetAsync(M.m.flag, 0, sizeof(int), s));
    MapBuf head = M.m; head.npt = n0;                       // (the whole map without a second part: the launch it always was)
    launch_map_gather(s, head, src, key, n_keys, xyz);
    if (p2.src && n0 < npt) launch_map_gather_from(s, M.m, n0, p2.src, p2.key, p2.n_keys, p2.xyz);
    HIPCHK(hipGetLastError());
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, M.m.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flag & 2) FAIL(VO_ERR_INVALID, "%s: a SIFT descriptor row of the map broke the norm bound of the integer matcher (|row|^2 > 2^20)", who);
    M.staged = true;
    return VO_OK;
}

extern "C" int vo_map_stage(vo_ctx* ctx, const uint8_t* rows, const double* points, int npt)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_map_stage: vo_batch_configure[_sift] has not been called");
    if (npt < 0 || (npt > 0 && (!rows || !points))) FAIL(VO_ERR_INVALID, "vo_map_stage: npt >= 0 rows and points are needed");
    if (npt > VO_MAP_MAX_POINTS) FAIL(VO_ERR_UNSUPPORTED, "vo_map_stage: a staged map holds at most %d points, got %d", VO_MAP_MAX_POINTS, npt);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIPCHK(hipStreamSynchronize(s));                        // the staging buffer may be in use
    const size_t D = b.sift ? 128 : 32, row_bytes = ((size_t)npt * D + 255) & ~(size_t)255, need = row_bytes + (size_t)npt * 24;
    uint8_t* drows = nullptr; double* dxyz = nullptr;
    if (npt > 0) {
        int rc = ctx->staging.grow(ctx, need); if (rc) return rc;
        drows = ctx->staging.p; dxyz = (double*)(ctx->staging.p + row_bytes);
        HIPCHK(hipMemcpyAsync(drows, rows, (size_t)npt * D, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dxyz, points, (size_t)npt * 24, hipMemcpyHostToDevice, s));
    }
    return map_stage_device(ctx, drows, nullptr, 0, dxyz, npt, "vo_map_stage");
}

extern "C" int vo_map_rows(vo_ctx* ctx, uint8_t* rows, double* points, int cap, int32_t* npt)
{
    if (!ctx) return VO_ERR_INVALID;
    const MapState& M = ctx->map;
    if (!M.staged) FAIL(VO_ERR_INVALID, "vo_map_rows: no map is staged");
    if (!npt || cap < 0) FAIL(VO_ERR_INVALID, "bad arguments");
    *npt = M.m.npt;
    const size_t n = (size_t)std::min(cap, M.m.npt);
    if (n == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (rows) HIPCHK(hipMemcpy(rows, M.m.rows, n * M.m.D, hipMemcpyDeviceToHost));
    if (points) HIPCHK(hipMemcpy(points, M.m.xyz, n * 24, hipMemcpyDeviceToHost));
    return VO_OK;
}

extern "C" int vo_map_localize(vo_ctx* ctx, const int32_t* slots, int Q, const double K[9], const vo_reloc_opts* o, double* poses,
                               int32_t* n_match, int32_t* n_inl, int32_t* status)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_map_localize: vo_batch_configure[_sift] has not been called");
    MapState& M = ctx->map;
    if (!M.staged) FAIL(VO_ERR_INVALID, "vo_map_localize: no map is staged (vo_map_stage, vo_map_from_slam)");
    if (Q < 0 || Q > b.max_pairs || Q > M.Q_cap) FAIL(VO_ERR_INVALID, "vo_map_localize: 0 <= Q <= max_pairs queries, got %d", Q);
    if (!K || !o || (Q > 0 && (!slots || !poses || !n_match || !n_inl || !status))) FAIL(VO_ERR_INVALID, "bad arguments");
    for (int q = 0; q < Q; q++) if (slots[q] < 0 || slots[q] >= b.max_frames) FAIL(VO_ERR_INVALID, "vo_map_localize: slot %d out of range", slots[q]);
    M.last_Q = 0; M.loc_ok = false;
    if (Q == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    int rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const RelocBuf& r = M.r;
    const int cap = b.kp_cap, mode = ctx->map_match;
    const double ratio = ctx->map_ratio;
    HIPCHK(hipMemcpyAsync(r.slots, slots, (size_t)Q * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(M.dK, K, 72, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(r.rvec, 0, (size_t)Q * 24, s)); HIPCHK(hipMemsetAsync(r.tvec, 0, (size_t)Q * 24, s));
    { StageTimer t(ctx, ST_MATCH_NN); launch_nn_map(s, M.m, r, Q, b.desc, b.desc_x, b.norms, b.kp_count, cap, desc_x_rows(cap), mode); }
    { StageTimer t(ctx, ST_MATCH_SELECT); launch_map_select(s, M.m, r, Q, b.kp_xy, b.kp_count, cap, o->max_distance, mode, ratio); }
    {
        StageTimer t(ctx, ST_MISC);
        launch_pnp_ransac(s, r.obj, r.img, r.off, Q, M.dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                          ctx->pnp_refine, r.rvec, r.tvec, r.mask, r.ninl, r.status, 2);
        launch_pnp_poses(s, r.rvec, r.tvec, r.ninl, r.status, Q, o->min_inliers, r.poses);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(poses, r.poses, (size_t)Q * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_match, r.m_count, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, r.ninl, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, r.status, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    M.last_Q = Q; M.last_mode = mode;
    if (b.sift) {                                           // a flagged slot, reported after the run as vo_pairs_run reports it
        std::vector<int> fl((size_t)b.max_frames);
        HIPCHK(hipMemcpy(fl.data(), b.flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int q = 0; q < Q; q++)
            if (fl[(size_t)slots[q]] & 2) FAIL(VO_ERR_INVALID, "a SIFT descriptor row broke the norm bound of the integer matcher (slot %d)", (int)slots[q]);
    }
    M.loc_slots.assign(slots, slots + Q); M.loc_ok = true;  // what a refinement pass (vo_map_localize_guided, prior == NULL) starts from
    return VO_OK;
}

// Matching by projection under a prior pose (include/vo_hip.h, "guided relocalisation"): k_guided_grid, k_guided_match and
// k_guided_select (guided_kernels.hip) in the place of k_nn_map and k_map_select; from the match list on it is vo_map_localize.
extern "C" int vo_map_localize_guided(vo_ctx* ctx, const int32_t* slots, int Q, const double K[9], const double* prior, const vo_guided_opts* gopt,
                                      const vo_reloc_opts* o, double* poses, int32_t* n_match, int32_t* n_inl, int32_t* status, int32_t* n_seen)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_map_localize_guided: vo_batch_configure[_sift] has not been called");
    MapState& M = ctx->map;
    if (!M.staged) FAIL(VO_ERR_INVALID, "vo_map_localize_guided: no map is staged (vo_map_stage, vo_map_from_slam)");
    if (Q < 0 || Q > b.max_pairs || Q > M.Q_cap) FAIL(VO_ERR_INVALID, "vo_map_localize_guided: 0 <= Q <= max_pairs queries, got %d", Q);
    if (!K || !o || !gopt || (Q > 0 && (!slots || !poses || !n_match || !n_inl || !status))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (!std::isfinite(gopt->radius) || gopt->radius < 0) FAIL(VO_ERR_INVALID, "vo_map_localize_guided: the radius must be finite and >= 0");
    if (!std::isfinite(gopt->ratio) || gopt->ratio < 0) FAIL(VO_ERR_INVALID, "vo_map_localize_guided: the ratio must be 0 (no rule) or finite and > 0");
    for (int q = 0; q < Q; q++) if (slots[q] < 0 || slots[q] >= b.max_frames) FAIL(VO_ERR_INVALID, "vo_map_localize_guided: slot %d out of range", slots[q]);
    if (prior) {
        for (size_t k = 0; k < (size_t)Q * 12; k++)
            if (!std::isfinite(prior[k])) FAIL(VO_ERR_INVALID, "vo_map_localize_guided: prior %d has an entry that is not finite", (int)(k / 12));
    } else if (!M.loc_ok || (int)M.loc_slots.size() != Q || !std::equal(M.loc_slots.begin(), M.loc_slots.end(), slots))
        FAIL(VO_ERR_INVALID, "vo_map_localize_guided: prior == NULL needs the most recent call on this staged map to be a vo_map_localize of the same slots");
    if (Q == 0) { M.last_Q = 0; M.loc_ok = false; return VO_OK; }
    HIPCHK(hipSetDevice(ctx->device));
    int rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const RelocBuf& r = M.r;
    const GuidedBuf& g = M.g;
    const int cap = b.kp_cap;
    M.last_Q = 0; M.loc_ok = false;
    // the priors first: a refinement pass takes them from the buffers this call goes on to overwrite
    if (prior) {
        HIPCHK(hipMemcpyAsync(g.prior, prior, (size_t)Q * 96, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(g.skip, 0, (size_t)Q * sizeof(int), s));
    } else {
        HIPCHK(hipMemcpyAsync(g.prior, r.poses, (size_t)Q * 96, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(g.skip, r.status, (size_t)Q * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(r.slots, slots, (size_t)Q * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(M.dK, K, 72, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(r.rvec, 0, (size_t)Q * 24, s)); HIPCHK(hipMemsetAsync(r.tvec, 0, (size_t)Q * 24, s));
    HIPCHK(hipMemsetAsync(g.claim, 0xff, (size_t)Q * cap * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(g.n_seen, 0, (size_t)Q * sizeof(int), s));
    {
        StageTimer t(ctx, ST_MATCH_NN);
        launch_guided_match(s, M.m, r, g, Q, b.desc, b.kp_xy, b.kp_count, cap, M.dK, gopt->radius, o->max_distance, gopt->ratio);
    }
    { StageTimer t(ctx, ST_MATCH_SELECT); launch_guided_select(s, M.m, r, g, Q, b.kp_xy, b.kp_count, cap); }
    {
        StageTimer t(ctx, ST_MISC);
        launch_pnp_ransac(s, r.obj, r.img, r.off, Q, M.dK, o->pnp_iterations, o->reproj_err, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N,
                          ctx->pnp_refine, r.rvec, r.tvec, r.mask, r.ninl, r.status, 2);
        launch_pnp_poses(s, r.rvec, r.tvec, r.ninl, r.status, Q, o->min_inliers, r.poses);
        launch_guided_keep(s, r, g, Q);
    }
    HIPCHK(hipGetLastError());
    std::vector<int32_t> seen((size_t)Q);                   // (the caller's n_seen may be NULL)
    HIPCHK(hipMemcpyAsync(poses, r.poses, (size_t)Q * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_match, r.m_count, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, r.ninl, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, r.status, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(seen.data(), g.n_seen, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_seen) std::copy(seen.begin(), seen.end(), n_seen);
    if (ctx->prof) prof_collect(ctx);
    M.last_Q = Q; M.last_mode = 1;                          // every guided list carries its second distances (vo_map_match_seconds)
    if (b.sift) {
        std::vector<int> fl((size_t)b.max_frames);
        HIPCHK(hipMemcpy(fl.data(), b.flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int q = 0; q < Q; q++)
            if (fl[(size_t)slots[q]] & 2) FAIL(VO_ERR_INVALID, "a SIFT descriptor row broke the norm bound of the integer matcher (slot %d)", (int)slots[q]);
    }
    return VO_OK;
}

extern "C" int vo_map_matches(vo_ctx* ctx, int q, int32_t* pt_idx, int32_t* kp_idx, float* dist, uint8_t* inlier_mask, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const MapState& M = ctx->map;
    if (!M.staged || q < 0 || q >= M.last_Q || !n_out || cap < 0) FAIL(VO_ERR_INVALID, "vo_map_matches: no such query in the most recent vo_map_localize");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int n = 0;
    HIPCHK(hipMemcpy(&n, M.r.m_count + q, sizeof(int), hipMemcpyDeviceToHost));
    if (n > cap) n = cap;
    *n_out = n;
    const size_t o = (size_t)q * M.kp_cap;
    if (n > 0) {
        if (pt_idx) HIPCHK(hipMemcpy(pt_idx, M.r.m_t + o, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (kp_idx) HIPCHK(hipMemcpy(kp_idx, M.r.m_q + o, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (dist) HIPCHK(hipMemcpy(dist, M.r.m_d + o, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        if (inlier_mask) HIPCHK(hipMemcpy(inlier_mask, M.r.mask + o, (size_t)n, hipMemcpyDeviceToHost));
    }
    return VO_OK;
}

// n.distance of knnMatch(k=2) for every entry of a match list: which = 0 the latest vo_map_localize, 1 the latest vo_map_align
extern "C" int vo_map_match_seconds(vo_ctx* ctx, int which, int q, float* dist2, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const MapState& M = ctx->map;
    const MapState::Align& A = M.al;
    if (which != 0 && which != 1) FAIL(VO_ERR_INVALID, "vo_map_match_seconds: which is 0 (vo_map_localize) or 1 (vo_map_align)");
    const int last_Q = which ? A.last_Q : M.last_Q, mode = which ? A.last_mode : M.last_mode;
    if (!M.staged || q < 0 || q >= last_Q || !n_out || cap < 0)
        FAIL(VO_ERR_INVALID, "vo_map_match_seconds: no such query in the most recent %s", which ? "vo_map_align" : "vo_map_localize");
    if (mode == 0) FAIL(VO_ERR_INVALID, "vo_map_match_seconds: that call ran in map-match mode 0, which finds no second neighbour (vo_set_map_match)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int n = 0;
    HIPCHK(hipMemcpy(&n, (which ? A.a.m_count : M.r.m_count) + q, sizeof(int), hipMemcpyDeviceToHost));
    if (n > cap) n = cap;
    *n_out = n;
    const float* src = which ? A.a.m_d2 + (size_t)A.off[(size_t)q] : M.r.m_d2 + (size_t)q * M.kp_cap;
    if (n > 0 && dist2) HIPCHK(hipMemcpy(dist2, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return VO_OK;
}
