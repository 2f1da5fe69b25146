// Driver of the sanitizer build of visual_odometry_amd/csrc/pgo_layout.h (CPU only, no HIP call): prepares the small graphs of
// tests/test_gpu_pose_graph.py — alone and as one batch with an over-capacity and an invalid graph between them — and checks what
// k_pose_graph relies on: the order is a permutation of the free vertices, every free vertex lies in exactly one run or is a
// separator, the runs are maximal and name their neighbours, the CSR lists hold every edge once per endpoint in input order, and
// the layout places every buffer inside the allocation without overlap.
#include "pgo_layout.h"
#include <stdio.h>
#include <algorithm>
#include <string>
#include <utility>

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL [%s] ", g_case.c_str()); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Graph { std::string name; int nv; std::vector<int> fixed; std::vector<std::pair<int, int>> edges; double weight; int expect; };

static Graph chain(const char* name, int nv, std::vector<std::pair<int, int>> more, std::vector<int> fixed = {0})
{
    Graph g{name, nv, fixed, {}, 1.0, VO_OK};
    for (int i = 0; i + 1 < nv; i++) g.edges.push_back({i, i + 1});
    for (auto e : more) g.edges.push_back(e);
    return g;
}

static std::vector<Graph> graphs()
{
    std::vector<Graph> out;
    out.push_back(chain("pair", 2, {}));
    out.push_back(chain("chain5", 5, {}));
    out.push_back(chain("loop_to_fixed", 12, {{0, 11}}));
    out.push_back(chain("adjacent_separators", 12, {{2, 9}, {3, 9}}));
    out.push_back(chain("fixed_in_the_middle", 9, {{0, 8}}, {4}));
    { std::vector<std::pair<int, int>> all; for (int i = 0; i < 6; i++) for (int j = i + 2; j < 6; j++) all.push_back({i, j}); out.push_back(chain("complete6", 6, all)); }
    out.push_back(chain("duplicated_chain_edge", 8, {{0, 7}, {3, 4}, {5, 4}}));
    out.push_back(chain("n300", 300, {{0, 299}, {40, 280}}));
    { std::vector<std::pair<int, int>> l; for (int k = 0; k < 32; k++) l.push_back({k, 69 - k}); out.push_back(chain("capacity", 70, l)); }
    { std::vector<std::pair<int, int>> l; for (int k = 0; k < 32; k++) l.push_back({k, 69 - k}); l.push_back({0, 40}); Graph g = chain("over_capacity", 70, l); g.expect = VO_ERR_UNSUPPORTED; out.push_back(g); }
    { Graph g = chain("unanchored", 6, {}); g.edges.erase(g.edges.begin() + 2); g.expect = VO_ERR_INVALID; out.push_back(g); }
    { Graph g = chain("index_out_of_range", 4, {{1, 4}}); g.expect = VO_ERR_INVALID; out.push_back(g); }
    { Graph g = chain("self_edge", 4, {{2, 2}}); g.expect = VO_ERR_INVALID; out.push_back(g); }
    { Graph g = chain("zero_weight", 4, {}); g.weight = 0.0; g.expect = VO_ERR_INVALID; out.push_back(g); }
    { Graph g = chain("too_many_vertices", VO_PGO_MAX_VERTICES + 1, {}); g.expect = VO_ERR_UNSUPPORTED; out.push_back(g); }
    out.push_back(chain("most_vertices", VO_PGO_MAX_VERTICES, {{0, VO_PGO_MAX_VERTICES - 1}}));
    out.push_back(chain("all_fixed", 3, {}, {0, 1, 2}));
    out.push_back(Graph{"empty", 0, {}, {}, 1.0, VO_OK});
    return out;
}

static void check_batch(const std::vector<Graph>& gs)
{
    const int B = (int)gs.size();
    std::vector<int32_t> voff(B + 1, 3), eoff(B + 1, 2);            // the call's rows need not start at 0
    for (int b = 0; b < B; b++) { voff[b + 1] = voff[b] + gs[b].nv; eoff[b + 1] = eoff[b] + (int)gs[b].edges.size(); }
    std::vector<uint8_t> fixed(voff[B], 0);
    std::vector<int32_t> edges(2 * (size_t)eoff[B], 0), status(B, 99);
    std::vector<double> info(7 * (size_t)eoff[B], 1.0);
    for (int b = 0; b < B; b++) {
        for (int v : gs[b].fixed) fixed[voff[b] + v] = 1;
        for (size_t k = 0; k < gs[b].edges.size(); k++) {
            edges[2 * (eoff[b] + k)] = gs[b].edges[k].first; edges[2 * (eoff[b] + k) + 1] = gs[b].edges[k].second;
            for (int c = 0; c < 7; c++) info[7 * (eoff[b] + k) + c] = gs[b].weight;
        }
    }
    PgoPlan P;
    CHECK(pgo_prepare(B, voff.data(), eoff.data(), fixed.data(), edges.data(), info.data(), status.data(), P), "pgo_prepare refused the offsets");
    CHECK(P.nv == voff[B] - voff[0] && P.ne == eoff[B] - eoff[0], "totals");
    size_t dense = 0, lds = 0;
    for (int b = 0; b < B; b++) {
        const Graph& g = gs[b];
        const PgoGraph& q = P.graphs[b];
        g_case = g.name + (B > 1 ? " (batch)" : "");
        CHECK(status[b] == g.expect, "status %d, expected %d", status[b], g.expect);
        CHECK(q.skip == (g.expect != VO_OK), "skip");
        CHECK(q.v0 == voff[b] - voff[0] && q.e0 == eoff[b] - eoff[0] && q.nv == g.nv && q.ne == (int)g.edges.size(), "rows");
        if (q.skip) { for (int v = 0; v < g.nv; v++) CHECK(P.order[q.v0 + v] == -1 && P.kind[q.v0 + v] == -2, "a skipped graph has no order"); continue; }
        const int* kind = P.kind.data() + q.v0;
        const int* order = P.order.data() + q.v0;
        std::vector<int> is_fixed(g.nv, 0), touched(g.nv, 0), seen(g.nv, 0), in_run(g.nv, 0);
        for (int v : g.fixed) is_fixed[v] = 1;
        for (auto e : g.edges) if (e.first - e.second != 1 && e.second - e.first != 1) { touched[e.first] = 1; touched[e.second] = 1; }
        int nfree = 0, nsep = 0;
        for (int v = 0; v < g.nv; v++) {
            nfree += !is_fixed[v];
            if (is_fixed[v]) CHECK(kind[v] == -2, "vertex %d is fixed", v);
            else if (touched[v]) { CHECK(kind[v] == nsep, "vertex %d is separator %d, got %d", v, nsep, kind[v]); nsep++; }
            else CHECK(kind[v] == -1, "vertex %d belongs to a run", v);
        }
        CHECK(q.nsep == nsep && nsep <= PGO_MAX_SEPARATORS, "separators %d, expected %d", q.nsep, nsep);
        // the order: a permutation of the free vertices, runs first
        for (int k = 0; k < g.nv; k++) {
            if (k < nfree) { CHECK(order[k] >= 0 && order[k] < g.nv && !is_fixed[order[k]] && !seen[order[k]], "order[%d] = %d", k, order[k]); if (order[k] >= 0 && order[k] < g.nv) seen[order[k]] = 1; }
            else CHECK(order[k] == -1, "order[%d] past the free vertices", k);
        }
        for (int k = 0; k + 1 < nfree; k++) CHECK(!(kind[order[k]] >= 0 && kind[order[k + 1]] == -1), "a separator before a run vertex in the order");
        // the runs: maximal, disjoint, ascending, and they name their neighbours
        int at = 0, prev_b = -1;
        for (int r = 0; r < q.nrun; r++) {
            const PgoRun& rn = P.runs[q.run0 + r];
            CHECK(rn.a > prev_b && rn.a <= rn.b && rn.b < g.nv, "run %d = %d .. %d", r, rn.a, rn.b);
            if (!(rn.a > prev_b && rn.a <= rn.b && rn.b < g.nv)) break;
            for (int v = rn.a; v <= rn.b; v++) { CHECK(kind[v] == -1 && !in_run[v], "run %d holds vertex %d", r, v); in_run[v]++; CHECK(order[at] == v, "order[%d] is not run %d's vertex %d", at, r, v); at++; }
            CHECK(rn.a == 0 || kind[rn.a - 1] != -1, "run %d is not maximal on the left", r);
            CHECK(rn.b == g.nv - 1 || kind[rn.b + 1] != -1, "run %d is not maximal on the right", r);
            CHECK(rn.lsep == (rn.a > 0 && kind[rn.a - 1] >= 0 ? kind[rn.a - 1] : -1), "run %d lsep %d", r, rn.lsep);
            CHECK(rn.rsep == (rn.b + 1 < g.nv && kind[rn.b + 1] >= 0 ? kind[rn.b + 1] : -1), "run %d rsep %d", r, rn.rsep);
            prev_b = rn.b;
        }
        for (int v = 0; v < g.nv; v++) CHECK((kind[v] == -1) == (in_run[v] == 1), "vertex %d lies in %d runs", v, in_run[v]);
        // the CSR lists: every edge once per endpoint, in input order
        const int* first = P.first.data() + q.first0;
        const int* list = P.list.data() + 2 * (size_t)q.e0;
        CHECK(first[0] == 0 && first[g.nv] == 2 * q.ne, "CSR ends at %d, expected %d", g.nv ? first[g.nv] : 0, 2 * q.ne);
        std::vector<int> count(2 * (size_t)q.ne + 1, 0);
        for (int v = 0; v < g.nv; v++) {
            CHECK(first[v] <= first[v + 1], "CSR offsets decrease at %d", v);
            for (int l = first[v]; l < first[v + 1]; l++) {
                const int k = list[l];
                CHECK(k >= 0 && k < q.ne && (g.edges[k].first == v || g.edges[k].second == v), "vertex %d lists edge %d", v, k);
                CHECK(l == first[v] || list[l - 1] < k, "vertex %d's list is not in input order", v);
                if (k >= 0 && k < q.ne) count[k]++;
            }
        }
        for (int k = 0; k < q.ne; k++) CHECK(count[k] == 2, "edge %d is listed %d times", k, count[k]);
        // the dense systems
        const size_t dd = pgo_dense_doubles(nsep);
        CHECK(q.dense0 == dense, "dense0");
        CHECK(q.dense_lds == (dd * 8 <= PGO_LDS_DENSE_BYTES), "dense_lds");
        dense += q.dense_lds ? dd : 2 * dd;
        if (q.dense_lds) lds = std::max(lds, dd * 8);
    }
    g_case = "layout";
    CHECK(P.dense == dense && P.lds_bytes == lds && lds <= PGO_LDS_DENSE_BYTES, "dense %zu / %zu, lds %zu / %zu", P.dense, dense, P.lds_bytes, lds);
    PgoBuf D{};
    ScratchLayout sc;
    pgo_take(sc, P, D);
    std::vector<uint8_t> mem(sc.bytes + 256);
    uint8_t* base = mem.data() + (256 - ((uintptr_t)mem.data() & 255)) % 256;
    sc.place_at(base);
    struct Region { const char* name; const uint8_t* p; size_t bytes; };
    const size_t V = (size_t)P.nv, E = (size_t)P.ne;
    std::vector<Region> rs = {
        {"graph", (const uint8_t*)D.graph, (size_t)B * sizeof(PgoGraph)}, {"run", (const uint8_t*)D.run, P.runs.size() * sizeof(PgoRun)}, {"kind", (const uint8_t*)D.kind, V * 4},
        {"first", (const uint8_t*)D.first, P.first.size() * 4}, {"list", (const uint8_t*)D.list, 2 * E * 4}, {"edges", (const uint8_t*)D.edges, 2 * E * 4},
        {"meas", (const uint8_t*)D.meas, 13 * E * 8}, {"info", (const uint8_t*)D.info, 7 * E * 8}, {"sims", (const uint8_t*)D.sims, 13 * V * 8}, {"trial", (const uint8_t*)D.trial, 13 * V * 8},
        {"J", (const uint8_t*)D.J, 98 * E * 8}, {"err", (const uint8_t*)D.err, 7 * E * 8}, {"wgt", (const uint8_t*)D.wgt, 7 * E * 8}, {"Hd", (const uint8_t*)D.Hd, 49 * V * 8},
        {"bv", (const uint8_t*)D.bv, 7 * V * 8}, {"U", (const uint8_t*)D.U, 49 * V * 8}, {"X", (const uint8_t*)D.X, 105 * V * 8},
        {"Lf", (const uint8_t*)D.Lf, 28 * V * 8}, {"Wf", (const uint8_t*)D.Wf, 49 * V * 8}, {"dense", (const uint8_t*)D.dense, P.dense * 8}, {"chi2", (const uint8_t*)D.chi2, (size_t)2 * B * 8},
        {"iterations_run", (const uint8_t*)D.iterations_run, (size_t)B * 4}, {"trials_run", (const uint8_t*)D.trials_run, (size_t)B * 4}};
    for (size_t i = 0; i < rs.size(); i++) {
        CHECK(rs[i].p >= base && rs[i].p + rs[i].bytes <= base + sc.bytes && ((uintptr_t)rs[i].p & 255) == 0, "%s lies outside the allocation or off a 256-byte boundary", rs[i].name);
        for (size_t j = 0; j < i; j++) CHECK(rs[i].p + rs[i].bytes <= rs[j].p || rs[j].p + rs[j].bytes <= rs[i].p || !rs[i].bytes || !rs[j].bytes, "%s overlaps %s", rs[i].name, rs[j].name);
    }
}

int main()
{
    const std::vector<Graph> gs = graphs();
    for (const Graph& g : gs) check_batch({g});
    check_batch(gs);
    {   // offsets that cannot be used
        g_case = "offsets";
        PgoPlan P; int32_t st[2]; const int32_t down[3] = {0, 4, 2}, ok[3] = {0, 2, 4}; const uint8_t fx[4] = {1, 0, 1, 0}; const int32_t ed[4] = {0, 1, 0, 1}; double w[14];
        for (double& x : w) x = 1.0;
        CHECK(!pgo_prepare(2, down, ok, fx, ed, w, st, P), "decreasing vertex offsets were accepted");
        CHECK(!pgo_prepare(2, ok, down, fx, ed, w, st, P), "decreasing edge offsets were accepted");
    }
    {   // a call without vertices and edges passes no arrays at all
        g_case = "null arrays";
        PgoPlan P; int32_t st[2] = {99, 99}; const int32_t zero[3] = {0, 0, 0};
        CHECK(pgo_prepare(2, zero, zero, nullptr, nullptr, nullptr, st, P), "two empty graphs without arrays were refused");
        CHECK(st[0] == VO_OK && st[1] == VO_OK && P.nv == 0 && P.ne == 0 && P.runs.empty() && !P.graphs[0].skip, "two empty graphs without arrays");
        PgoBuf D{}; ScratchLayout sc; pgo_take(sc, P, D);
        CHECK(sc.bytes > 0, "the layout of an empty call still holds the graph records");
    }
    printf("pgo_layout_driver: %zu graphs, %d failures\n", gs.size(), g_fail);
    return g_fail ? 1 : 0;
}
