// pgo_layout.h — what the host prepares for one vo_pose_graph_batch call (pgo_api.hip) and where its device buffers lie:
// validation, the elimination order (runs of consecutive free vertices, then the separators), every vertex's edges in input
// order (a CSR list) and the scratch layout.  Index arithmetic over std::vector and ScratchLayout only: nothing in this header
// calls the HIP runtime, so tests/native/pgo_layout_driver.cpp runs it on a machine without a GPU.
#pragma once
#include "slam_layout.h"
#include <cmath>
#include <vector>

#define PGO_MAX_SEPARATORS (2 * VO_PGO_MAX_LOOPS)
#define PGO_LDS_DENSE_BYTES 65536          // a separator system of at most this many bytes is factored in LDS, a larger one in the call's scratch

// One graph of the batch.  Vertex and edge indices are local to the graph; v0 / e0 are its rows in the call's arrays.
struct PgoGraph {
    int v0, e0, nv, ne;
    int first0;                            // its nv + 1 CSR offsets start here; they index list[] from 2 * e0
    int run0, nrun;                        // its runs
    int nsep;                              // separators: free vertices touched by a loop edge, numbered in vertex order
    int skip;                              // status != VO_OK: the kernel leaves it alone
    int dense_lds;                         // the separator system fits PGO_LDS_DENSE_BYTES
    unsigned long long dense0;             // doubles into dense[]: Hss, then (unless dense_lds) the trial's copy
};

// A maximal run a .. b of consecutive free vertices that are no separators.  Its Hessian is block tridiagonal; it couples to the
// rest only through the chain edges to a - 1 and b + 1, when those are separators (a fixed neighbour contributes nothing).
struct PgoRun { int a, b, lsep, rsep; };   // lsep / rsep: separator number of a - 1 / b + 1, or -1

struct PgoPlan {
    std::vector<PgoGraph> graphs;
    std::vector<PgoRun> runs;
    std::vector<int> kind;                 // [V] -2 fixed, -1 in a run, >= 0 separator number
    std::vector<int> first, list;          // CSR: per graph nv + 1 offsets; [2 E] edge numbers (local), per vertex in input order
    std::vector<int> order;                // [V] per graph: the free vertices, runs first, then separators; the rest -1
    size_t dense = 0;                      // doubles of all separator systems
    size_t lds_bytes = 0;                  // dynamic LDS of the launch
    int nv = 0, ne = 0;
};

static inline size_t pgo_dense_doubles(int nsep) { const size_t n = 7 * (size_t)nsep; return (n + 1) * (n | 1); }

// status[b] per graph (VO_OK, VO_ERR_INVALID, VO_ERR_UNSUPPORTED): indices, i != j and weights first, then capacity, then whether
// every vertex reaches a fixed one.  Returns false when the offsets themselves are unusable.
static inline bool pgo_prepare(int B, const int32_t* vert_off, const int32_t* edge_off, const uint8_t* fixed, const int32_t* edges,
                               const double* info, int32_t* status, PgoPlan& P)
{
    if (B < 0 || !vert_off || !edge_off || vert_off[0] < 0 || edge_off[0] < 0) return false;
    for (int b = 0; b < B; b++) if (vert_off[b + 1] < vert_off[b] || edge_off[b + 1] < edge_off[b]) return false;
    const int V0 = vert_off[0], E0 = edge_off[0];
    P = PgoPlan();
    P.nv = vert_off[B] - V0; P.ne = edge_off[B] - E0;
    P.graphs.resize(B);
    P.kind.assign(P.nv, -2); P.order.assign(P.nv, -1);
    P.first.assign((size_t)P.nv + B, 0); P.list.assign((size_t)2 * P.ne, 0);
    std::vector<int> parent, fill;
    for (int b = 0; b < B; b++) {
        PgoGraph& g = P.graphs[b];
        g.v0 = vert_off[b] - V0; g.e0 = edge_off[b] - E0; g.nv = vert_off[b + 1] - vert_off[b]; g.ne = edge_off[b + 1] - edge_off[b];
        g.first0 = g.v0 + b; g.run0 = (int)P.runs.size(); g.nrun = 0; g.nsep = 0; g.skip = 0; g.dense_lds = 0; g.dense0 = P.dense;
        const uint8_t* fx = g.nv ? fixed + vert_off[b] : nullptr;          // a call without vertices or edges may pass no arrays
        const int32_t* ed = g.ne ? edges + 2 * (size_t)edge_off[b] : nullptr;
        const double* wi = g.ne ? info + 7 * (size_t)edge_off[b] : nullptr;
        int st = VO_OK, loops = 0;
        for (int k = 0; k < g.ne && st == VO_OK; k++) {
            const int i = ed[2 * k], j = ed[2 * k + 1];
            if (i < 0 || i >= g.nv || j < 0 || j >= g.nv || i == j) { st = VO_ERR_INVALID; break; }
            for (int c = 0; c < 7; c++) if (!(wi[7 * (size_t)k + c] > 0) || !std::isfinite(wi[7 * (size_t)k + c])) st = VO_ERR_INVALID;
            if (i - j != 1 && j - i != 1) loops++;
        }
        if (st == VO_OK && (g.nv > VO_PGO_MAX_VERTICES || loops > VO_PGO_MAX_LOOPS)) st = VO_ERR_UNSUPPORTED;
        if (st == VO_OK) {                  // union-find: every component must hold a fixed vertex
            parent.resize(g.nv);
            for (int v = 0; v < g.nv; v++) parent[v] = v;
            auto find = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
            for (int k = 0; k < g.ne; k++) {
                const int a = find(ed[2 * k]), c = find(ed[2 * k + 1]);
                if (a != c) parent[a > c ? a : c] = a > c ? c : a;
            }
            std::vector<uint8_t> anchored(g.nv, 0);
            for (int v = 0; v < g.nv; v++) if (fx[v]) anchored[find(v)] = 1;
            for (int v = 0; v < g.nv; v++) if (!anchored[find(v)]) { st = VO_ERR_INVALID; break; }
        }
        status[b] = st;
        if (st != VO_OK) { g.skip = 1; continue; }
        int* kind = P.kind.data() + g.v0;
        for (int v = 0; v < g.nv; v++) kind[v] = fx[v] ? -2 : -1;
        for (int k = 0; k < g.ne; k++) {
            const int i = ed[2 * k], j = ed[2 * k + 1];
            if (i - j == 1 || j - i == 1) continue;
            if (!fx[i]) kind[i] = 0;
            if (!fx[j]) kind[j] = 0;
        }
        for (int v = 0; v < g.nv; v++) if (kind[v] >= 0) kind[v] = g.nsep++;
        // the order: runs, then separators
        int* order = P.order.data() + g.v0;
        int at = 0;
        for (int v = 0; v < g.nv; v++) {
            if (kind[v] != -1) continue;
            PgoRun r{v, v, v > 0 && kind[v - 1] >= 0 ? kind[v - 1] : -1, -1};
            while (r.b + 1 < g.nv && kind[r.b + 1] == -1) r.b++;
            if (r.b + 1 < g.nv && kind[r.b + 1] >= 0) r.rsep = kind[r.b + 1];
            for (int u = r.a; u <= r.b; u++) order[at++] = u;
            P.runs.push_back(r); g.nrun++;
            v = r.b;
        }
        for (int v = 0; v < g.nv; v++) if (kind[v] >= 0) order[at++] = v;
        // every vertex's edges, in input order
        int* first = P.first.data() + g.first0;
        int* list = P.list.data() + 2 * (size_t)g.e0;
        for (int k = 0; k < g.ne; k++) { first[ed[2 * k] + 1]++; first[ed[2 * k + 1] + 1]++; }
        for (int v = 0; v < g.nv; v++) first[v + 1] += first[v];
        fill.assign(first, first + g.nv);
        for (int k = 0; k < g.ne; k++) { list[fill[ed[2 * k]]++] = k; list[fill[ed[2 * k + 1]]++] = k; }
        const size_t dd = pgo_dense_doubles(g.nsep);
        g.dense_lds = dd * sizeof(double) <= PGO_LDS_DENSE_BYTES;
        if (g.dense_lds && dd * sizeof(double) > P.lds_bytes) P.lds_bytes = dd * sizeof(double);
        P.dense += g.dense_lds ? dd : 2 * dd;
    }
    return true;
}

// The device side of a call: what k_pose_graph reads and writes.  Per-vertex and per-edge arrays hold every graph of the call.
struct PgoBuf {
    const PgoGraph* graph; const PgoRun* run;
    const int *kind, *first, *list, *edges;        // edges [E][2]
    const double *meas, *info;                     // [E][13], [E][7]
    double *sims, *trial;                          // [V][13]: in / out, and the trial estimate
    double *J;                                     // [E][2][49]: d e / d S_i = Ad(C), d e / d S_j = -Ad(E)
    double *err, *wgt;                             // [E][7]: e, and rho' w
    double *Hd, *bv, *U;                           // [V][49] diagonal block, [V][7] b, [V][49] H(v, v + 1)
    double *X;                                     // [V][15][7]: a run's solves: b, then the 7 + 7 coupling columns
    double *Lf, *Wf;                               // [V][28] Cholesky factor of a run's pivot block, [V][49] L^-1 H(v, v + 1)
    double *dense;                                 // the separator systems (PgoGraph::dense0)
    double *chi2; int *iterations_run, *trials_run;   // [B][2], [B], [B]
};

static inline void pgo_take(ScratchLayout& sc, const PgoPlan& P, PgoBuf& D)
{
    const size_t V = (size_t)P.nv, E = (size_t)P.ne, B = P.graphs.size();
    sc.take(const_cast<PgoGraph**>(&D.graph), B); sc.take(const_cast<PgoRun**>(&D.run), P.runs.size());
    sc.take(const_cast<int**>(&D.kind), V); sc.take(const_cast<int**>(&D.first), P.first.size()); sc.take(const_cast<int**>(&D.list), 2 * E);
    sc.take(const_cast<int**>(&D.edges), 2 * E); sc.take(const_cast<double**>(&D.meas), 13 * E); sc.take(const_cast<double**>(&D.info), 7 * E);
    sc.take(&D.sims, 13 * V); sc.take(&D.trial, 13 * V); sc.take(&D.J, 98 * E); sc.take(&D.err, 7 * E); sc.take(&D.wgt, 7 * E);
    sc.take(&D.Hd, 49 * V); sc.take(&D.bv, 7 * V); sc.take(&D.U, 49 * V); sc.take(&D.X, 105 * V);
    sc.take(&D.Lf, 28 * V); sc.take(&D.Wf, 49 * V); sc.take(&D.dense, P.dense);
    sc.take(&D.chi2, 2 * B); sc.take(&D.iterations_run, B); sc.take(&D.trials_run, B);
}

struct PgoParams { double delta; int iterations; };
void launch_pose_graph(hipStream_t s, const PgoBuf& D, const PgoParams& P, int B, size_t lds_bytes);
