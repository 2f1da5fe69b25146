// ba_large_api.hip — vo_bundle_adjust_large of libvo_hip.so: bundle adjustment of one map of hundreds of cameras
// (include/vo_hip.h, "bundle adjustment, large maps").  Host code only: gba_layout.h prepares the lists and names the buffers,
// the kernels are in ba_large_kernels.hip.  The LM loop runs here: per iteration one linearisation, per trial one chain of
// kernels that ends in k_gba_decide and one read of the 64-byte record it wrote.
#include "vo_host.h"
#include "gba_layout.h"

static_assert(sizeof(GbaRec) == 64, "the decision record is what the host reads once per trial");

extern "C" int vo_bundle_adjust_large(vo_ctx* ctx, double* poses, const uint8_t* cam_fixed, int ncam, double* points, int npt,
                                      const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, int nobs,
                                      double focal, double cx, double cy, const vo_ba_opts* opts, double* chi2,
                                      int32_t* iterations_run, int32_t* trials_run)
{
    if (!ctx) return VO_ERR_INVALID;
    if (ncam < 0 || npt < 0 || nobs < 0 || !opts || !chi2 || !iterations_run || !trials_run) FAIL(VO_ERR_INVALID, "vo_bundle_adjust_large: bad arguments");
    if ((ncam > 0 && (!poses || !cam_fixed)) || (npt > 0 && !points) || (nobs > 0 && (!obs_cam || !obs_pt || !obs_xy))) FAIL(VO_ERR_INVALID, "vo_bundle_adjust_large: bad arguments");
    if (opts->iterations < 0 || opts->iterations > 1000) FAIL(VO_ERR_INVALID, "vo_bundle_adjust_large: iterations must be 0 .. 1000, got %d", opts->iterations);
    if (!(focal == focal) || !(cx == cx) || !(cy == cy) || !(opts->huber_delta == opts->huber_delta)) FAIL(VO_ERR_INVALID, "vo_bundle_adjust_large: camera parameters must be numbers");
    chi2[0] = chi2[1] = 0; *iterations_run = *trials_run = 0;

    GbaPlan plan;
    const int st = gba_prepare(ncam, cam_fixed, npt, nobs, obs_cam, obs_pt, obs_xy, plan);
    if (st == VO_ERR_UNSUPPORTED) FAIL(VO_ERR_UNSUPPORTED, "vo_bundle_adjust_large holds at most %d free cameras and 2^31 - 1 observation pairs", VO_BA_LARGE_MAX_FREE);
    if (st != VO_OK) FAIL(VO_ERR_INVALID, "vo_bundle_adjust_large: an observation refers to a missing camera or point");

    HIPCHK(hipSetDevice(ctx->device));
    GbaBuf D{};
    ScratchLayout sc;
    gba_take(sc, plan, D);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    auto up = [&](const void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(up(D.col, plan.col.data(), plan.col.size() * sizeof(int)));
    HIPCHK(up(D.free_cam, plan.free_cam.data(), plan.free_cam.size() * sizeof(int)));
    HIPCHK(up(D.pt_first, plan.pt_first.data(), plan.pt_first.size() * sizeof(int)));
    HIPCHK(up(D.obs_cam, plan.s_cam.data(), plan.s_cam.size() * sizeof(int)));
    HIPCHK(up(D.obs_pt, plan.s_pt.data(), plan.s_pt.size() * sizeof(int)));
    HIPCHK(up(D.obs_xy, plan.s_xy.data(), plan.s_xy.size() * sizeof(double)));
    HIPCHK(up(D.cam_first, plan.cam_first.data(), plan.cam_first.size() * sizeof(int)));
    HIPCHK(up(D.cam_list, plan.cam_list.data(), plan.cam_list.size() * sizeof(int)));
    HIPCHK(up(D.blocks, plan.blocks.data(), plan.blocks.size() * sizeof(GbaBlock)));
    HIPCHK(up(D.blk_first, plan.blk_first.data(), plan.blk_first.size() * sizeof(int)));
    HIPCHK(up(D.pairs, plan.pairs.data(), plan.pairs.size() * sizeof(int2)));
    HIPCHK(up(D.cam[0], poses, (size_t)12 * ncam * sizeof(double)));
    HIPCHK(up(D.X[0], points, (size_t)3 * npt * sizeof(double)));
    HIPCHK(hipStreamSynchronize(s));                                 // the plan's vectors live on this stack

    const BaParams prm{focal, cx, cy, opts->huber_delta, opts->iterations};
    GbaRec rec{};
    int cur = 0, it_run = 0, trials = 0;
    {
        StageTimer t(ctx, ST_MISC);
        launch_gba_init(s, D, prm);
        HIPCHK(hipMemcpyAsync(&rec, D.rec, sizeof(GbaRec), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        chi2[0] = rec.chi;
        bool stop = false;
        for (int it = 0; it < opts->iterations && !stop; it++) {
            it_run++;
            launch_gba_linearise(s, D, prm, cur, it == 0);
            for (int q = 0; q < 10; q++) {                           // k_gba_decide ends the loop; 10 is g2o's bound on it
                launch_gba_trial(s, D, prm, cur, q == 0);
                trials++;
                HIPCHK(hipMemcpyAsync(&rec, D.rec, sizeof(GbaRec), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (rec.accepted) cur ^= 1;
                if (!rec.go_on) break;
            }
            stop = rec.stop != 0;
        }
    }
    HIPCHK(hipGetLastError());
    // every camera and point of the current estimate: a fixed camera and a point without observations hold their input bytes
    if (ncam > 0) HIPCHK(hipMemcpyAsync(poses, D.cam[cur], (size_t)12 * ncam * sizeof(double), hipMemcpyDeviceToHost, s));
    if (npt > 0) HIPCHK(hipMemcpyAsync(points, D.X[cur], (size_t)3 * npt * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    chi2[1] = rec.chi; *iterations_run = it_run; *trials_run = trials;
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

// The factorisation and solve of a trial on a system of the caller's (include/vo_hip.h): launch_gba_factor_solve between an upload
// and a download, nothing of the LM loop.
extern "C" int vo_ba_large_solve(vo_ctx* ctx, const double* A, const double* b, int n, double* x, double* L, double* y,
                                 int32_t* pivot_failed)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!A || !b || !x || !pivot_failed) FAIL(VO_ERR_INVALID, "vo_ba_large_solve: bad arguments");
    if (n < 6 || n % 6 != 0) FAIL(VO_ERR_INVALID, "vo_ba_large_solve: n must be 6 F with F >= 1, got %d", n);
    if (n / 6 > VO_BA_LARGE_MAX_FREE) FAIL(VO_ERR_UNSUPPORTED, "vo_ba_large_solve holds at most n = 6 * %d", VO_BA_LARGE_MAX_FREE);

    HIPCHK(hipSetDevice(ctx->device));
    GbaBuf D{};
    ScratchLayout sc;
    gba_take_solve(sc, n, D);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    const size_t N = (size_t)n, ld = (size_t)D.ld, row = N * sizeof(double);
    HIPCHK(hipMemsetAsync(D.rec, 0, sizeof(GbaRec), s));
    // rows 0 .. n - 1 whole (the kernels read a row up to its diagonal only), b as row n
    HIPCHK(hipMemcpy2DAsync(D.S, ld * sizeof(double), A, row, row, N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D.S + N * ld, b, row, hipMemcpyHostToDevice, s));
    launch_gba_factor_solve(s, D);
    GbaRec rec{};
    HIPCHK(hipMemcpyAsync(&rec, D.rec, sizeof(GbaRec), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (rec.fail) {
        HIPCHK(hipMemsetAsync(D.rec, 0, sizeof(GbaRec), s));          // the next call starts clean
        HIPCHK(hipStreamSynchronize(s));
        *pivot_failed = 1;
        return VO_OK;
    }
    HIPCHK(hipMemcpyAsync(x, D.dc, row, hipMemcpyDeviceToHost, s));
    if (y) HIPCHK(hipMemcpyAsync(y, D.S + N * ld, row, hipMemcpyDeviceToHost, s));
    if (L) {
        // the factor lies in two places: a row's columns left of its panel in S, those inside the diagonal block in Ld
        const size_t panels = (N + GBA_NB - 1) / GBA_NB;
        std::vector<double> hs(N * ld), hd(panels * GBA_NB * GBA_NB);
        HIPCHK(hipMemcpyAsync(hs.data(), D.S, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hd.data(), D.Ld, hd.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t i = 0; i < N; i++) {
            const size_t k = i / GBA_NB, c0 = k * GBA_NB;
            for (size_t j = 0; j < c0; j++) L[i * N + j] = hs[i * ld + j];
            for (size_t j = c0; j <= i; j++) L[i * N + j] = hd[k * GBA_NB * GBA_NB + (i - c0) * GBA_NB + (j - c0)];
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    *pivot_failed = 0;
    return VO_OK;
}
