// vo_api.hip — context, device buffers and the C ABI of libvo_hip.so (see include/vo_hip.h).
// Host-side plumbing only: every arithmetic stage is a HIP kernel in orb_/match_/geom_kernels.hip.
// The vo_slam_* entry points are slam_api.hip; vo_host.h has the context and the helpers the two files share.
#include "vo_host.h"

static const char* k_stage_names[VO_STAGE_COUNT] = {
    "gray", "pyramid_resize", "fast_score_nms", "select_fast", "harris", "select_harris", "ic_angle",
    "gaussian_blur", "rbrief", "match_nn", "match_select", "essential_ransac", "recover_pose",
    "triangulate", "misc", "reserved", "sift_scale_space", "sift_extrema", "sift_refine_orient", "sift_sort_unique",
    "sift_descriptor", "cv2_keypoint_order", "trajectory_gather", "reserved2", "slam_ba_prepare", "slam_bundle_adjust", "slam_filter",
    "slam_camera_limit", "slam_map_statistics", "undistort_points"};

static void clear_last_run(vo_ctx* ctx) { ctx->last = LastRun(); }

// An upload, ingest or detection into slots first .. first + n - 1: if the stream's last frame is among them, no call can continue it
// (vo_slam_streams: the sequence whose last frame it is cannot advance any more; the others can).
// ... and the slots' keypoints are no longer the ones vo_frames_undistort rewrote: their marks go.
static void slam_stream_slots_written(vo_ctx* ctx, int first, int n)
{
    for (int k = first < 0 ? 0 : first; k < first + n && k < (int)ctx->undistorted.size(); k++) ctx->undistorted[(size_t)k] = 0;
    SlamStream& st = ctx->stream_map;
    if (st.live && st.anchor >= first && st.anchor < first + n) st.touched = true;
    for (SlamStream::Seq& q : st.seq)
        if (st.live && q.anchor >= first && q.anchor < first + n) q.touched = true;
}

void prof_collect(vo_ctx* c)
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
    drop_map(c);
    drop_places(c);
    c->undistorted.clear();
}

static void comm_release(vo_ctx* ctx);
static int sift_frames_upload_enqueue(vo_ctx* ctx, const uint8_t* frames, int F, int row_stride, int64_t frame_stride, int first_slot);
static int sift_frames_detect_enqueue(vo_ctx* ctx, int first_slot, int F);

extern "C" int vo_version(void) { return 128; }

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

extern "C" int vo_set_map_match(vo_ctx* ctx, int mode, double ratio)
{
    if (!ctx) return VO_ERR_INVALID;
    if (mode < 0 || mode > 2) FAIL(VO_ERR_INVALID, "map match mode must be 0 (cross-check), 1 (ratio) or 2 (cross-check and ratio)");
    if (mode != 0) {
        if (!(ratio > 0 && ratio <= DBL_MAX)) FAIL(VO_ERR_INVALID, "map match ratio must be finite and positive");
        ctx->map_ratio = ratio;
    }
    ctx->map_match = mode;
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
        drop_map(ctx);
    drop_places(ctx);
        ctx->undistorted.clear();
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

Batch batch(const vo_ctx* ctx)
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
    { StageTimer t(ctx, ST_BLUR); launch_blur(s, pyr, blur, g, F); }
    {
        StageTimer t(ctx, ST_BRIEF);                            // orientation and descriptor: one kernel (ST_ANGLE has no launches)
        const int cx = desc_x_rows(g.kp_cap);
        const int fp4 = descx_begin_write(ctx, first_slot, F);
        launch_brief(s, pyr, blur, g, ff, F, ctx->desc_x + (size_t)first_slot * cx * 256, cx, fp4);
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
int ensure_rng(vo_ctx* ctx, uint64_t seed)
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

extern "C" int vo_correspond_epilines(vo_ctx* ctx, const void* points, int N, int point_type, int which_image, const double* F, void* lines)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!F || N < 0 || (N > 0 && (!points || !lines))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (point_type < 0 || point_type > 2) FAIL(VO_ERR_INVALID, "point_type must be 0 (f64), 1 (f32) or 2 (i32)");
    if (which_image != 1 && which_image != 2) FAIL(VO_ERR_INVALID, "whichImage must be 1 or 2");
    if (N == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t in_b = (size_t)2 * N * (point_type == 0 ? 8 : 4), out_b = (size_t)3 * N * (point_type == 0 ? 8 : 4);
    double Fh[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Fh[3 * r + c] = which_image == 1 ? F[3 * r + c] : F[3 * c + r];
    double *dF, *dpts, *dlines;                                   // doubles: both arrays start 8-byte aligned whatever the type
    ScratchLayout sc;
    sc.take(&dF, 9); sc.take(&dpts, (in_b + 7) / 8); sc.take(&dlines, (out_b + 7) / 8);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dF, Fh, sizeof(Fh), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dpts, points, in_b, hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MISC); launch_epilines(s, dpts, point_type, N, dF, dlines); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(lines, dlines, out_b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                               // Fh is a stack array: the call ends synchronised
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// cv2.undistortPoints' arguments as the kernels take them: the camera, the coefficients by name (absent ones zero), RR = P R
static int undistort_params(vo_ctx* ctx, const double* K, const double* dist, int ndist, const double* R, const double* P, UndistortParams* up)
{
    if (!K) FAIL(VO_ERR_INVALID, "K is NULL");
    if (ndist == 12 || ndist == 14) FAIL(VO_ERR_UNSUPPORTED, "thin-prism and tilt coefficients (%d distortion coefficients) are not built", ndist);
    if (ndist != 4 && ndist != 5 && ndist != 8) FAIL(VO_ERR_INVALID, "4, 5 or 8 distortion coefficients are needed, not %d", ndist);
    if (!dist) FAIL(VO_ERR_INVALID, "dist is NULL");
    if (K[0] == 0 || K[4] == 0) FAIL(VO_ERR_INVALID, "fx and fy must not be 0");
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; i++) k[i] = dist[i];
    up->fx = K[0]; up->fy = K[4]; up->cx = K[2]; up->cy = K[5];
    up->k1 = k[0]; up->k2 = k[1]; up->p1 = k[2]; up->p2 = k[3]; up->k3 = k[4]; up->k4 = k[5]; up->k5 = k[6]; up->k6 = k[7];
    static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* Rm = R ? R : I3;
    const double* Pm = P ? P : I3;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) up->RR[3 * i + j] = Pm[3 * i] * Rm[j] + Pm[3 * i + 1] * Rm[3 + j] + Pm[3 * i + 2] * Rm[6 + j];
    return VO_OK;
}

extern "C" int vo_undistort_points(vo_ctx* ctx, const void* points, int N, int point_type, const double K[9], const double* dist, int ndist,
                                   const double* R, const double* P, void* out)
{
    if (!ctx) return VO_ERR_INVALID;
    if (N < 0 || (N > 0 && (!points || !out))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (point_type != 0 && point_type != 1) FAIL(VO_ERR_INVALID, "point_type must be 0 (f64) or 1 (f32)");
    UndistortParams up;
    int rc = undistort_params(ctx, K, dist, ndist, R, P, &up); if (rc) return rc;
    if (N == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)2 * N * (point_type == 0 ? 8 : 4);
    double *dpts, *dout;                                          // doubles: both arrays start 8-byte aligned whatever the type
    ScratchLayout sc;
    sc.take(&dpts, (bytes + 7) / 8); sc.take(&dout, (bytes + 7) / 8);
    rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dpts, points, bytes, hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_UNDISTORT); launch_undistort_points(s, dpts, point_type, N, up, dout); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_frames_undistort(vo_ctx* ctx, int first_slot, int F, const double K[9], const double* dist, int ndist)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (F < 0 || first_slot < 0 || first_slot + F > b.max_frames) FAIL(VO_ERR_INVALID, "slot range out of bounds");
    UndistortParams up;
    int rc = undistort_params(ctx, K, dist, ndist, nullptr, K, &up); if (rc) return rc;
    for (int k = first_slot; k < first_slot + F && k < (int)ctx->undistorted.size(); k++)
        if (ctx->undistorted[(size_t)k]) FAIL(VO_ERR_INVALID, "slot %d has been undistorted already", k);
    if (F == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    {
        StageTimer t(ctx, ST_UNDISTORT);
        launch_undistort_frames(ctx->stream, const_cast<float*>(b.kp_xy) + (size_t)first_slot * b.kp_cap * 2, b.kp_count + first_slot, b.kp_cap, F, up);
    }
    HIPCHK(hipGetLastError());
    if (ctx->undistorted.size() < (size_t)b.max_frames) ctx->undistorted.resize((size_t)b.max_frames, 0);
    for (int k = first_slot; k < first_slot + F; k++) ctx->undistorted[(size_t)k] = 1;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_pairs_epipolar(vo_ctx* ctx, int B, const double* K, int32_t* n, double* mean, double* std_dev, double* max_dist, double* dist)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!K || !n || !mean || !std_dev || !max_dist) FAIL(VO_ERR_INVALID, "bad arguments");
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_batch_configure has not been called");
    if (B < 1 || B != ctx->last.pairs) FAIL(VO_ERR_INVALID, "vo_pairs_epipolar takes all %d pairs of the most recent vo_pairs_run", ctx->last.pairs);
    // K^-1 is restated as the pair path normalises pixels: it reads fx, fy, cx, cy only.  Any other shape would be read differently
    // there and here, so it is refused: skew, a last row that is not (0, 0, 1), a zero or non-finite focal length
    if (K[1] != 0 || K[3] != 0 || K[6] != 0 || K[7] != 0 || K[8] != 1 || !(K[0] != 0) || !(K[4] != 0) || !std::isfinite(K[0]) || !std::isfinite(K[4]) ||
        !std::isfinite(K[2]) || !std::isfinite(K[5]))
        FAIL(VO_ERR_UNSUPPORTED, "vo_pairs_epipolar takes K = [fx 0 cx; 0 fy cy; 0 0 1] with finite entries and fx, fy != 0");
    HIPCHK(hipSetDevice(ctx->device));
    const int cap = b.kp_cap;
    double *dK, *dmean, *dsd, *dmx, *ddist; int* dn;
    ScratchLayout sc;
    sc.take(&dK, 9); sc.take(&dmean, B); sc.take(&dsd, B); sc.take(&dmx, B); sc.take(&ddist, (size_t)B * cap); sc.take(&dn, B);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(dK, K, 72, hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MISC); launch_pairs_epipolar(s, ctx->pb, cap, B, dK, ddist, dn, dmean, dsd, dmx); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n, dn, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(mean, dmean, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(std_dev, dsd, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(max_dist, dmx, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    if (dist) HIPCHK(hipMemcpyAsync(dist, ddist, (size_t)B * cap * 8, hipMemcpyDeviceToHost, s));
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
    slam_stats_take_scratch(sc, d, npt, nobs); slam_stats_take_rows(sc, d, 1, ncam);
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
    drop_map(ctx);
    drop_places(ctx);
    ctx->undistorted.clear();
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
int chain_check(vo_ctx* ctx, int B, const char* who, int* F_out, int* cap_out)
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
        else if (stage == ST_UNDISTORT) b = 16.0 * S.kp_cap;                       // a full slot: 8 B read and 8 B written per keypoint
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
    case ST_BLUR: b = total + total; break;
    case ST_BRIEF: b = N * 749 + N * 512 + N * 32 + N * 28; break;                 // the raw patch of the orientation + gathers, descriptor, record
    case ST_MATCH_NN: b = 2 * N * 32; break;                                       // per pair ~ per frame: both descriptor sets
    case ST_MATCH_SELECT: b = 16 * N; break;
    case ST_RANSAC: b = 33 * N; break;                                             // SURVEY 8(d) geometry 65 N: 4 f64 coords + mask per match ...
    case ST_POSE: b = 32 * N; break;                                               // ... + the inliers' coordinates again
    case ST_UNDISTORT: b = 16 * N; break;                                          // kp_xy: 8 B read and 8 B written per keypoint
    default: b = 0;
    }
    return b * F;
}
