// pgo_api.hip — vo_pose_graph_batch and vo_pose_graph of libvo_hip.so: Sim(3) pose-graph optimisation (include/vo_hip.h, "pose
// graph").  Host code only: pgo_layout.h prepares the lists and names the buffers, the kernel is in pgo_kernels.hip.
#include "vo_host.h"
#include "pgo_layout.h"

extern "C" int vo_pose_graph_batch(vo_ctx* ctx, int B, const int32_t* vert_off, const int32_t* edge_off, double* sims, const uint8_t* fixed,
                                   const int32_t* edges, const double* meas, const double* info, const vo_pgo_opts* opts, double* chi2,
                                   int32_t* iterations_run, int32_t* trials_run, int32_t* status)
{
    if (!ctx) return VO_ERR_INVALID;
    if (B < 0 || !opts || (B > 0 && (!vert_off || !edge_off || !chi2 || !iterations_run || !trials_run || !status))) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: bad arguments");
    if (opts->iterations < 1 || opts->iterations > 1000) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: iterations must be 1 .. 1000, got %d", opts->iterations);
    if (!(opts->huber_delta == opts->huber_delta)) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: huber_delta must be a number");
    if (B == 0) return VO_OK;
    if (vert_off[0] < 0 || edge_off[0] < 0) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: offsets must not be negative");
    for (int b = 0; b < B; b++)
        if (vert_off[b + 1] < vert_off[b] || edge_off[b + 1] < edge_off[b]) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: offsets must not decrease");
    const int v0 = vert_off[0], e0 = edge_off[0], nv = vert_off[B] - v0, ne = edge_off[B] - e0;
    if ((nv > 0 && (!sims || !fixed)) || (ne > 0 && (!edges || !meas || !info))) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: bad arguments");

    PgoPlan plan;
    if (!pgo_prepare(B, vert_off, edge_off, fixed, edges, info, status, plan)) FAIL(VO_ERR_INVALID, "vo_pose_graph_batch: bad offsets");
    for (int b = 0; b < B; b++) { chi2[2 * b] = chi2[2 * b + 1] = 0; iterations_run[b] = trials_run[b] = 0; }

    HIPCHK(hipSetDevice(ctx->device));
    PgoBuf D{};
    ScratchLayout sc;
    pgo_take(sc, plan, D);
    int rc = sc.place(ctx); if (rc) return rc;
    hipStream_t s = ctx->stream;
    auto up = [&](const void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(up(D.graph, plan.graphs.data(), (size_t)B * sizeof(PgoGraph)));
    HIPCHK(up(D.run, plan.runs.data(), plan.runs.size() * sizeof(PgoRun)));
    HIPCHK(up(D.kind, plan.kind.data(), (size_t)nv * sizeof(int)));
    HIPCHK(up(D.first, plan.first.data(), plan.first.size() * sizeof(int)));
    HIPCHK(up(D.list, plan.list.data(), plan.list.size() * sizeof(int)));
    HIPCHK(up(D.edges, ne ? edges + 2 * (size_t)e0 : nullptr, (size_t)2 * ne * sizeof(int)));
    HIPCHK(up(D.meas, ne ? meas + 13 * (size_t)e0 : nullptr, (size_t)13 * ne * sizeof(double)));
    HIPCHK(up(D.info, ne ? info + 7 * (size_t)e0 : nullptr, (size_t)7 * ne * sizeof(double)));
    HIPCHK(up(D.sims, nv ? sims + 13 * (size_t)v0 : nullptr, (size_t)13 * nv * sizeof(double)));
    HIPCHK(hipMemsetAsync(D.chi2, 0, (size_t)2 * B * sizeof(double), s));
    HIPCHK(hipMemsetAsync(D.iterations_run, 0, (size_t)B * sizeof(int), s));
    HIPCHK(hipMemsetAsync(D.trials_run, 0, (size_t)B * sizeof(int), s));
    HIPCHK(hipStreamSynchronize(s));                                 // the plan's vectors live on this stack
    const PgoParams prm{opts->huber_delta, opts->iterations};
    { StageTimer t(ctx, ST_MISC); launch_pose_graph(s, D, prm, B, plan.lds_bytes); }
    HIPCHK(hipGetLastError());
    // a graph that did not run keeps its bytes: only the rows of the others come back
    for (int b = 0; b < B; b++) {
        const PgoGraph& g = plan.graphs[b];
        if (g.skip || g.nv == 0) continue;
        HIPCHK(hipMemcpyAsync(sims + 13 * (size_t)(v0 + g.v0), D.sims + 13 * (size_t)g.v0, (size_t)13 * g.nv * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(chi2, D.chi2, (size_t)2 * B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(iterations_run, D.iterations_run, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(trials_run, D.trials_run, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}

extern "C" int vo_pose_graph(vo_ctx* ctx, double* sims, const uint8_t* fixed, int nv, const int32_t* edges, const double* meas, const double* info,
                             int ne, const vo_pgo_opts* opts, double* chi2, int32_t* iterations_run, int32_t* trials_run)
{
    if (!ctx) return VO_ERR_INVALID;
    if (nv < 0 || ne < 0 || !chi2 || !iterations_run || !trials_run) FAIL(VO_ERR_INVALID, "vo_pose_graph: bad arguments");
    const int32_t vo[2] = {0, nv}, eo[2] = {0, ne};
    int32_t status = 0;
    int rc = vo_pose_graph_batch(ctx, 1, vo, eo, sims, fixed, edges, meas, info, opts, chi2, iterations_run, trials_run, &status);
    if (rc) return rc;
    if (status == VO_ERR_UNSUPPORTED)
        FAIL(VO_ERR_UNSUPPORTED, "a pose graph holds at most %d vertices and %d loop edges", VO_PGO_MAX_VERTICES, VO_PGO_MAX_LOOPS);
    if (status == VO_ERR_INVALID)
        FAIL(VO_ERR_INVALID, "pose graph: an edge names a missing vertex or joins a vertex to itself, a weight is not positive, or a vertex reaches no fixed vertex");
    return VO_OK;
}
