// align_api.hip — vo_sim3_ransac_batch, vo_map_align, vo_map_align_guided and vo_map_align_matches of libvo_hip.so: the similarity
// that takes one map's gauge to another's, from the descriptor rows both carry (include/vo_hip.h, "map alignment", "guided map
// alignment").  Host code only; the kernels are in reloc_kernels.hip and map_fuse_kernels.hip.  The staged map is reloc_api.hip's; this file adds the query maps and their work buffers (MapState::Align).
#include "vo_host.h"

#define VO_ALIGN_MAX_QUERIES 64
#define VO_ALIGN_MAX_ROWS 65536

static int align_opts_check(vo_ctx* ctx, const vo_align_opts* o, const char* who)
{
    if (!o) FAIL(VO_ERR_INVALID, "%s: options are needed", who);
    if (!(o->max_error > 0)) FAIL(VO_ERR_INVALID, "%s: max_error must be positive (it is in the units of map A; there is no default)", who);
    if (!(o->confidence > 0 && o->confidence < 1)) FAIL(VO_ERR_INVALID, "%s: confidence must lie in (0, 1)", who);
    return VO_OK;
}

extern "C" int vo_sim3_ransac_batch(vo_ctx* ctx, const double* src, const double* dst, const int32_t* offsets, int B, const vo_align_opts* o,
                                    double* sim, uint8_t* mask, int32_t* n_inl, int32_t* status)
{
    if (!ctx) return VO_ERR_INVALID;
    int rc = align_opts_check(ctx, o, "vo_sim3_ransac_batch"); if (rc) return rc;
    if (B < 0 || !offsets || (B > 0 && (!sim || !n_inl || !status))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (B == 0) return VO_OK;
    for (int b = 0; b < B; b++) if (offsets[b + 1] < offsets[b]) FAIL(VO_ERR_INVALID, "offsets must not decrease");
    const int total = offsets[B] - offsets[0];
    if (total > 0 && (!src || !dst || !mask)) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    double *dsrc, *ddst, *dsim; int *doff, *dninl, *dst_; uint8_t* dmask;
    ScratchLayout sc;
    sc.take(&dsrc, (size_t)3 * total); sc.take(&ddst, (size_t)3 * total); sc.take(&dsim, (size_t)13 * B);
    sc.take(&doff, (size_t)B + 1); sc.take(&dninl, B); sc.take(&dst_, B); sc.take(&dmask, total);
    rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    std::vector<int> off(B + 1);
    for (int b = 0; b <= B; b++) off[b] = offsets[b] - offsets[0];
    if (total > 0) {
        HIPCHK(hipMemcpyAsync(dsrc, src + (size_t)3 * offsets[0], (size_t)3 * total * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ddst, dst + (size_t)3 * offsets[0], (size_t)3 * total * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(doff, off.data(), (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                                 // `off` is a stack vector
    {
        StageTimer t(ctx, ST_MISC);
        launch_sim3_ransac(s, dsrc, ddst, doff, 1, B, o->iterations, o->max_error, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N, o->min_inliers,
                           dsim, dmask, dninl, dst_);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sim, dsim, (size_t)13 * B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, dninl, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, dst_, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (total > 0) HIPCHK(hipMemcpyAsync(mask + offsets[0], dmask, (size_t)total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// Room for Q query maps of `total` rows, pad_total rows once every map starts on a multiple of 256, against the staged map as it is
// allocated now.  Kept while the next call fits; otherwise released as a whole and made again.
static int align_reserve(vo_ctx* ctx, int Q, int total, int pad_total)
{
    MapState& M = ctx->map;
    MapState::Align& A = M.al;
    if (A.a.rows && Q <= A.Q_cap && pad_total <= A.pad_cap && total <= A.total_cap && A.map_rows == M.m.cap_rows && A.a.D == M.m.D) return VO_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    A.mem.release();
    A.a = AlignBuf{}; A.f = FuseBuf{};
    A.Q_cap = A.pad_cap = A.total_cap = A.map_rows = 0;
    const size_t q = (size_t)Q, P = (size_t)std::max(pad_total, 256), T = (size_t)std::max(total, 1), D = (size_t)M.m.D;
    DevList& mem = A.mem; AlignBuf& a = A.a;
    HIPCHK(mem.alloc(&a.off, q + 1)); HIPCHK(mem.alloc(&a.pad, q + 1)); HIPCHK(mem.alloc(&a.rows, P * D)); HIPCHK(mem.alloc(&a.xyz, T * 3));
    HIPCHK(mem.alloc(&a.flag, 1));
    if (D == 128) { HIPCHK(mem.alloc(&a.img, P * 128)); HIPCHK(mem.alloc(&a.norms, P)); }
    HIPCHK(mem.alloc(&a.nn_idx, P)); HIPCHK(mem.alloc(&a.nn_dist, P)); HIPCHK(mem.alloc(&a.rn_idx, q * (size_t)M.m.cap_rows));
    HIPCHK(mem.alloc(&a.nn_dist2, P)); HIPCHK(mem.alloc(&a.m_d2, T));
    HIPCHK(mem.alloc(&a.m_b, T)); HIPCHK(mem.alloc(&a.m_a, T)); HIPCHK(mem.alloc(&a.m_d, T)); HIPCHK(mem.alloc(&a.m_count, q));
    HIPCHK(mem.alloc(&a.src, T * 3)); HIPCHK(mem.alloc(&a.dst, T * 3)); HIPCHK(mem.alloc(&a.poff, 2 * q));
    HIPCHK(mem.alloc(&a.sim, 13 * q)); HIPCHK(mem.alloc(&a.mask, T)); HIPCHK(mem.alloc(&a.ninl, q)); HIPCHK(mem.alloc(&a.status, q));
    FuseBuf& f = A.f;                                       // vo_map_align_guided's: the grid over the staged map, the claims, the priors
    HIPCHK(mem.alloc(&f.cell_off, FUSE_CELLS + 1)); HIPCHK(mem.alloc(&f.cell_pt, (size_t)M.m.cap_rows)); HIPCHK(mem.alloc(&f.box, 6));
    HIPCHK(mem.alloc(&f.claim, q * (size_t)M.m.cap_rows)); HIPCHK(mem.alloc(&f.pt_best, T)); HIPCHK(mem.alloc(&f.pt_d2, T));
    HIPCHK(mem.alloc(&f.prior, 13 * q)); HIPCHK(mem.alloc(&f.skip, q)); HIPCHK(mem.alloc(&f.n_seen, q));
    a.D = (int)D;
    A.Q_cap = Q; A.pad_cap = (int)P; A.total_cap = (int)T; A.map_rows = M.m.cap_rows;
    return VO_OK;
}

extern "C" int vo_map_align(vo_ctx* ctx, const uint8_t* rows, const double* points, const int32_t* off, int Q, const vo_align_opts* o,
                            double* sim, int32_t* n_match, int32_t* n_inl, int32_t* status)
{
    if (!ctx) return VO_ERR_INVALID;
    MapState& M = ctx->map;
    MapState::Align& A = M.al;
    A.last_Q = 0;
    if (!M.staged) FAIL(VO_ERR_INVALID, "vo_map_align: no map is staged (vo_map_stage, vo_map_from_slam)");
    int rc = align_opts_check(ctx, o, "vo_map_align"); if (rc) return rc;
    if (Q < 0 || !off || (Q > 0 && (!sim || !n_match || !n_inl || !status))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (Q > VO_ALIGN_MAX_QUERIES) FAIL(VO_ERR_UNSUPPORTED, "vo_map_align: at most %d query maps in one call, got %d", VO_ALIGN_MAX_QUERIES, Q);
    if (off[0] != 0) FAIL(VO_ERR_INVALID, "vo_map_align: off[0] must be 0");
    for (int q = 0; q < Q; q++) if (off[q + 1] < off[q]) FAIL(VO_ERR_INVALID, "vo_map_align: offsets must not decrease");
    const int total = off[Q];
    if (total > VO_ALIGN_MAX_ROWS) FAIL(VO_ERR_UNSUPPORTED, "vo_map_align: at most %d query rows in one call, got %d", VO_ALIGN_MAX_ROWS, total);
    if (total > 0 && (!rows || !points)) FAIL(VO_ERR_INVALID, "bad arguments");
    if (Q == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int32_t> pad((size_t)Q + 1, 0);
    int max_rows = 0;
    for (int q = 0; q < Q; q++) { const int n = off[q + 1] - off[q]; pad[q + 1] = pad[q] + ((n + 255) & ~255); max_rows = std::max(max_rows, n); }
    rc = align_reserve(ctx, Q, total, pad[Q]); if (rc) return rc;
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipStreamSynchronize(s));                        // the staging buffer and the host copies of the offsets may be in use
    A.off.assign(off, off + Q + 1); A.pad = pad;
    const size_t D = (size_t)M.m.D;
    if (total > 0) { rc = ctx->staging.grow(ctx, (size_t)total * D); if (rc) return rc; }
    AlignBuf a = A.a;
    a.Q = Q; a.total = total;
    const int mode = ctx->map_match;
    if (total > 0) {
        HIPCHK(hipMemcpyAsync(ctx->staging.p, rows, (size_t)total * D, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(a.xyz, points, (size_t)total * 24, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(a.off, A.off.data(), ((size_t)Q + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(a.pad, A.pad.data(), ((size_t)Q + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(a.flag, 0, sizeof(int), s));
    { StageTimer t(ctx, ST_MATCH_NN); launch_map_align_match(s, M.m, a, ctx->staging.p, max_rows, mode); }
    { StageTimer t(ctx, ST_MATCH_SELECT); launch_map_align_select(s, M.m, a, o->max_distance, mode, ctx->map_ratio); }
    {
        StageTimer t(ctx, ST_MISC);
        launch_sim3_ransac(s, a.src, a.dst, a.poff, 2, Q, o->iterations, o->max_error, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N, o->min_inliers,
                           a.sim, a.mask, a.ninl, a.status);
    }
    HIPCHK(hipGetLastError());
    int flag = 0;
    HIPCHK(hipMemcpyAsync(sim, a.sim, (size_t)Q * 13 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_match, a.m_count, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, a.ninl, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, a.status, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    if (flag & 2) FAIL(VO_ERR_INVALID, "vo_map_align: a SIFT descriptor row of a query map broke the norm bound of the integer matcher (|row|^2 > 2^20)");
    A.a.Q = Q; A.a.total = total;
    A.last_Q = Q; A.last_mode = mode; A.guided = false;     // what a refinement pass (vo_map_align_guided without arrays) starts from
    return VO_OK;
}

// Matching in space under a prior similarity (include/vo_hip.h, "guided map alignment"): k_fuse_grid, k_fuse_match and k_fuse_select
// (map_fuse_kernels.hip) in the place of k_nn_align and k_align_select; from the match lists on it is vo_map_align.
extern "C" int vo_map_align_guided(vo_ctx* ctx, const uint8_t* rows, const double* points, const int32_t* off, int Q, const double* prior,
                                   const vo_guided_opts* gopt, const vo_align_opts* o, double* sim, int32_t* n_match, int32_t* n_inl, int32_t* status,
                                   int32_t* n_seen)
{
    if (!ctx) return VO_ERR_INVALID;
    MapState& M = ctx->map;
    MapState::Align& A = M.al;
    if (!M.staged) FAIL(VO_ERR_INVALID, "vo_map_align_guided: no map is staged (vo_map_stage, vo_map_from_slam)");
    int rc = align_opts_check(ctx, o, "vo_map_align_guided"); if (rc) return rc;
    if (!gopt) FAIL(VO_ERR_INVALID, "vo_map_align_guided: the guided options are needed");
    if (!std::isfinite(gopt->radius) || gopt->radius < 0) FAIL(VO_ERR_INVALID, "vo_map_align_guided: the radius must be finite and >= 0");
    if (!std::isfinite(gopt->ratio) || gopt->ratio < 0) FAIL(VO_ERR_INVALID, "vo_map_align_guided: the ratio must be 0 (no rule) or finite and > 0");
    if (Q < 0 || (Q > 0 && (!sim || !n_match || !n_inl || !status))) FAIL(VO_ERR_INVALID, "bad arguments");
    const bool refine = !rows && !points && !off && !prior;
    int total = 0, max_rows = 0;
    std::vector<int32_t> pad;
    if (refine) {
        if (A.last_Q <= 0 || A.guided || Q != A.last_Q)
            FAIL(VO_ERR_INVALID, "vo_map_align_guided: without arrays the most recent align call on this staged map must be a vo_map_align of the same Q");
        total = A.a.total;
        for (int q = 0; q < Q; q++) max_rows = std::max(max_rows, A.off[(size_t)q + 1] - A.off[(size_t)q]);
    } else {
        if (!rows || !points || !off || !prior)
            FAIL(VO_ERR_INVALID, "vo_map_align_guided: rows, points, off and prior are given together or all left NULL");
        if (Q > VO_ALIGN_MAX_QUERIES) FAIL(VO_ERR_UNSUPPORTED, "vo_map_align_guided: at most %d query maps in one call, got %d", VO_ALIGN_MAX_QUERIES, Q);
        if (off[0] != 0) FAIL(VO_ERR_INVALID, "vo_map_align_guided: off[0] must be 0");
        for (int q = 0; q < Q; q++) if (off[q + 1] < off[q]) FAIL(VO_ERR_INVALID, "vo_map_align_guided: offsets must not decrease");
        total = off[Q];
        if (total > VO_ALIGN_MAX_ROWS) FAIL(VO_ERR_UNSUPPORTED, "vo_map_align_guided: at most %d query rows in one call, got %d", VO_ALIGN_MAX_ROWS, total);
        for (size_t k = 0; k < (size_t)Q * 13; k++)
            if (!std::isfinite(prior[k])) FAIL(VO_ERR_INVALID, "vo_map_align_guided: prior %d has an entry that is not finite", (int)(k / 13));
        pad.assign((size_t)Q + 1, 0);
        for (int q = 0; q < Q; q++) { const int n = off[q + 1] - off[q]; pad[q + 1] = pad[q] + ((n + 255) & ~255); max_rows = std::max(max_rows, n); }
    }
    A.last_Q = 0;
    if (Q == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    if (!refine) { rc = align_reserve(ctx, Q, total, pad[Q]); if (rc) return rc; }
    rc = ensure_rng(ctx, o->seed); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const size_t D = (size_t)M.m.D;
    AlignBuf a = A.a;
    const FuseBuf f = A.f;
    a.Q = Q; a.total = total;
    if (refine) {
        // the priors first: they lie in buffers this call goes on to overwrite
        HIPCHK(hipMemcpyAsync(f.prior, a.sim, (size_t)Q * 13 * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(f.skip, a.status, (size_t)Q * sizeof(int), hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(hipStreamSynchronize(s));                    // the staging buffer and the host copies of the offsets may be in use
        A.off.assign(off, off + Q + 1); A.pad = pad;
        if (total > 0) {
            rc = ctx->staging.grow(ctx, (size_t)total * D); if (rc) return rc;
            HIPCHK(hipMemcpyAsync(ctx->staging.p, rows, (size_t)total * D, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(a.xyz, points, (size_t)total * 24, hipMemcpyHostToDevice, s));
        }
        HIPCHK(hipMemcpyAsync(a.off, A.off.data(), ((size_t)Q + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(a.pad, A.pad.data(), ((size_t)Q + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(f.prior, prior, (size_t)Q * 13 * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(f.skip, 0, (size_t)Q * sizeof(int), s));
        HIPCHK(hipMemsetAsync(a.flag, 0, sizeof(int), s));
    }
    {
        StageTimer t(ctx, ST_MATCH_NN);
        if (!refine) launch_map_align_gather(s, a, ctx->staging.p);
        HIPCHK(hipMemsetAsync(f.claim, 0xff, (size_t)Q * M.m.cap_rows * sizeof(unsigned long long), s));
        HIPCHK(hipMemsetAsync(f.n_seen, 0, (size_t)Q * sizeof(int), s));
        launch_fuse_match(s, M.m, a, f, max_rows, gopt->radius, o->max_distance, gopt->ratio);
    }
    { StageTimer t(ctx, ST_MATCH_SELECT); launch_fuse_select(s, M.m, a, f); }
    {
        StageTimer t(ctx, ST_MISC);
        launch_sim3_ransac(s, a.src, a.dst, a.poff, 2, Q, o->iterations, o->max_error, o->confidence, o->seed, ctx->rng_tab, RNG_TAB_N, o->min_inliers,
                           a.sim, a.mask, a.ninl, a.status);
        launch_fuse_keep(s, a, f);
    }
    HIPCHK(hipGetLastError());
    int flag = 0;
    std::vector<int32_t> seen((size_t)Q);                   // (the caller's n_seen may be NULL)
    HIPCHK(hipMemcpyAsync(sim, a.sim, (size_t)Q * 13 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_match, a.m_count, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_inl, a.ninl, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, a.status, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(seen.data(), f.n_seen, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_seen) std::copy(seen.begin(), seen.end(), n_seen);
    if (ctx->prof) prof_collect(ctx);
    if (flag & 2) FAIL(VO_ERR_INVALID, "vo_map_align_guided: a SIFT descriptor row of a query map broke the norm bound of the integer matcher (|row|^2 > 2^20)");
    A.a.Q = Q; A.a.total = total;
    A.last_Q = Q; A.last_mode = 1; A.guided = true;         // every guided list carries its second distances (vo_map_match_seconds)
    return VO_OK;
}

extern "C" int vo_map_align_matches(vo_ctx* ctx, int q, int32_t* a_idx, int32_t* b_idx, float* dist, uint8_t* inlier_mask, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const MapState& M = ctx->map;
    const MapState::Align& A = M.al;
    if (!M.staged || q < 0 || q >= A.last_Q || !n_out || cap < 0) FAIL(VO_ERR_INVALID, "vo_map_align_matches: no such query in the most recent vo_map_align");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int n = 0;
    HIPCHK(hipMemcpy(&n, A.a.m_count + q, sizeof(int), hipMemcpyDeviceToHost));
    if (n > cap) n = cap;
    *n_out = n;
    const size_t o = (size_t)A.off[(size_t)q];
    if (n > 0) {
        if (a_idx) HIPCHK(hipMemcpy(a_idx, A.a.m_a + o, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (b_idx) HIPCHK(hipMemcpy(b_idx, A.a.m_b + o, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        if (dist) HIPCHK(hipMemcpy(dist, A.a.m_d + o, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        if (inlier_mask) HIPCHK(hipMemcpy(inlier_mask, A.a.mask + o, (size_t)n, hipMemcpyDeviceToHost));
    }
    return VO_OK;
}
