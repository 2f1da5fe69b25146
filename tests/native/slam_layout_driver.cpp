// Driver of the sanitizer build of visual_odometry_amd/csrc/slam_layout.h (CPU only, no HIP call): places the one layout of the
// vo_slam_* entry points at a made-up base for every row of SlamDims' table and checks it against the formulas restated here —
// every sub-buffer inside the allocation on a 256-byte boundary, none overlapping, the per-call part one tail, every sequence's
// descriptor inside the whole arrays and apart from the others', and statistics that cost nothing when they are off.
#include "slam_layout.h"
#include <stdio.h>
#include <algorithm>
#include <string>

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL [%s] ", g_case.c_str()); printf(__VA_ARGS__); printf("\n"); } } while (0)

static size_t up(size_t n) { return (n + 255) & ~(size_t)255; }

// the shapes of the issue: cap = 8, F = 5, max_cameras = 3, free_cameras = 2
static const size_t CAP = 8, F = 5, MAXCAM = 3, CM = MAXCAM + 1, FREE = 2, NBLK = FREE * (FREE + 1) / 2, MAX_PAIRS = 6;
enum Form { CHAIN, CHAINS, STREAM, STREAMS };

struct Shape {
    Form form; size_t S; std::vector<size_t> len, total;      // pairs of a sequence in the call; total_pairs of a stream
    bool restart, stats, snapshot; size_t ss;
    size_t B() const { size_t n = 0; for (size_t v : len) n += v; return n; }
    size_t maxB() const { return *std::max_element(len.begin(), len.end()); }
    bool stream() const { return form == STREAM || form == STREAMS; }
    // the table of the layout, restated
    size_t rows() const { return form == CHAIN || form == CHAINS ? F : form == STREAM ? F + 2 : F + 2 * S; }
    size_t np(size_t q) const { return form == CHAIN ? F * CAP : form == CHAINS ? (len[q] + 1) * CAP : (total[q] + 1) * CAP; }
    size_t no(size_t q) const { return stream() ? 2 * CAP * std::min(CM, total[q]) : 2 * len[q] * CAP; }
    size_t npair(size_t q) const { return no(q) * (FREE + 1) / 2; }
    size_t P() const { return stream() ? MAX_PAIRS : B(); }
    size_t steps() const { return stream() ? MAX_PAIRS : maxB(); }
    size_t snap_np() const { size_t m = 0; for (size_t q = 0; q < S; q++) m = std::max(m, np(q)); return stream() ? m : np(ss); }
    size_t snap_no() const { size_t m = 0; for (size_t q = 0; q < S; q++) m = std::max(m, no(q)); return stream() ? m : no(ss); }
    size_t sum(size_t (Shape::*f)(size_t) const, size_t upto) const { size_t n = 0; for (size_t q = 0; q < upto; q++) n += (this->*f)(q); return n; }
};

static SlamDims dims_of(const Shape& h)
{
    SlamDims d;
    d.S = (int)h.S; d.F = (int)F; d.rows = h.rows(); d.cap = CAP; d.cm = CM; d.free_cameras = (int)FREE;
    for (size_t q = 0; q < h.S; q++) { d.np.push_back(h.np(q)); d.no.push_back(h.no(q)); }
    d.P = h.P(); d.steps = h.steps(); d.stream = h.stream(); d.restart = h.restart; d.stats = h.stats; d.snapshot = h.snapshot;
    d.snap_np = h.snap_np(); d.snap_no = h.snap_no();
    return d;
}

struct Region { const char* name; const uint8_t* p; size_t bytes; bool call, stats; };

// every sub-buffer the layout should have placed, with the bytes the formulas give it
static std::vector<Region> regions_of(const Shape& h, const SlamBufs& b)
{
    std::vector<Region> r;
    const size_t S = h.S, fc = h.rows() * CAP, NC = CM * S, NP = h.sum(&Shape::np, S), NO = h.sum(&Shape::no, S), NPAIR = h.sum(&Shape::npair, S), P = h.P();
    bool call = false, stats = false;
    auto put = [&](const char* name, auto* p, size_t n) { r.push_back({name, (const uint8_t*)p, n * sizeof(*p), call, stats}); };
    auto map = [&](const SlamMap& m, size_t maps, size_t nc, size_t np, size_t no) {
        put("cnt", m.cnt, 4 * maps); put("cam_frame", m.cam_frame, nc); put("cam_pose", m.cam_pose, nc * 12); put("cam_fixed", m.cam_fixed, nc);
        put("pt_key", m.pt_key, np); put("pt_xyz", m.pt_xyz, np * 3); put("obs_cam", m.obs_cam, no); put("obs_pt", m.obs_pt, no); put("obs_xy", m.obs_xy, no * 2);
        if (h.stream()) put("pt_feat", m.pt_feat, np * 2);
        else CHECK(m.pt_feat == nullptr, "pt_feat is set outside a stream");
    };
    const ChainBuf& c = b.cb; const SlamBuf& m = b.sb; const BaBuf& D = b.D; const StatsBuf& t = b.stats;
    put("parent", c.parent, fc); put("map_pt", c.map_pt, fc * 3); put("cam", c.cam, F * 12); put("in_map", c.in_map, fc); put("cam_ok", c.cam_ok, F); put("pt_of", m.pt_of, fc);
    put("dK", b.dK, 9);
    put("obj", c.obj, S * CAP * 3); put("img", c.img, S * CAP * 2); put("Xw", c.Xw, S * CAP * 4); put("pmask", c.pmask, S * CAP); put("dec", m.dec, S * CAP);
    put("off", c.off, 2 * S); put("rvec", c.rvec, 3 * S); put("tvec", c.tvec, 3 * S); put("pninl", c.pninl, S); put("pstatus", c.pstatus, S);
    put("P1", c.P1, 12 * S); put("P2", c.P2, 12 * S); put("alive", c.alive, S); put("map_count", c.map_count, S);
    map(m.m, S, NC, NP, NO);
    put("tmp", m.tmp, NP); put("idx", m.idx, NO); put("prob", m.prob, S); put("cam_col", m.cam_col, NC); put("pt_first", m.pt_first, NP + S);
    put("s_cam", m.s_cam, NO); put("s_pt", m.s_pt, NO); put("s_xy", m.s_xy, NO * 2); put("pairs", m.pairs, NPAIR); put("blk_first", m.blk_first, S * (NBLK + 1));
    put("X2", D.X2, NP * 3); put("W", D.W, NO * 18); put("Hpp", D.Hpp, NP * 6); put("bp", D.bp, NP * 3); put("Hpi", D.Hpi, NP * 6);
    put("dseq", b.dseq, S);
    if (h.snapshot) map(b.snap, 1, CM, h.snap_np(), h.snap_no());
    else CHECK(b.snap.cnt == nullptr && b.snap.pt_key == nullptr, "a snapshot is placed though the switch is off");
    if (h.stream()) { put("keep", b.keep, 24 * S); put("dcar", b.dcar, S); put("drows", b.drows, S * (P + 1)); put("dseat", b.dseat, S); }
    else CHECK(!b.keep && !b.dcar && !b.drows && !b.dseat && !m.st.carried_frame && !m.st.carried_poses, "a stream's buffer is placed outside a stream");
    if (h.restart) put("rs.st", c.rs.st, 4 * S);
    else CHECK(!c.rs.st && !c.rs.segment && !c.rs.cause && !c.rs.seg_poses && !c.rs.seg_poses_last, "a restart buffer is placed though the switch is off");
    stats = true;
    if (h.stats) { put("pt_cur", t.pt_cur, NP); put("slot", t.slot, NO); put("bad", t.bad, 1); }
    else CHECK(!t.pt_cur && !t.slot && !t.bad && !t.total_sqerr && !t.obs_matrix && !t.cam_frame, "a statistics buffer is placed though the switch is off");
    call = true;
    if (h.stats) {
        put("total_sqerr", t.total_sqerr, P); put("max_sqerr", t.max_sqerr, P); put("n_high", t.n_high, P); put("counts", t.counts, P * 3);
        put("obs_hist", t.obs_hist, P * VO_STATS_HIST); put("obs_matrix", t.obs_matrix, P * CM * CM); put("stats.cam_frame", t.cam_frame, P * CM);
    }
    stats = false;
    put("poses", c.poses, (P + S) * 12); put("poses_last", m.poses_last, (P + S) * 12);
    put("n_corr", c.n_corr, P); put("n_inl", c.n_inl, P); put("status", c.status, P); put("n_map", c.n_map, P);
    put("n_pts", m.n_pts, P); put("n_obs", m.n_obs, P); put("n_cam", m.n_cam, P);
    put("dchi2", b.dchi2, 2 * h.steps() * S); put("dit", b.dit, h.steps() * S); put("dtr", b.dtr, h.steps() * S);
    if (h.stream()) { put("carried_frame", m.st.carried_frame, NC); put("carried_poses", m.st.carried_poses, NC * 12); }
    if (h.restart) { put("segment", c.rs.segment, P); put("cause", c.rs.cause, P); put("seg_poses", c.rs.seg_poses, P * 12); put("seg_poses_last", c.rs.seg_poses_last, P * 12); }
    return r;
}

// one member of a sequence's descriptor: its range, and the whole array it must lie in
struct Member { const char* name; const uint8_t *whole, *p; size_t whole_bytes, off, bytes; };

static std::vector<Member> members_of(const Shape& h, const SlamBufs& b, const SlamSeq& e, size_t q, size_t first)
{
    std::vector<Member> v;
    const size_t S = h.S, NC = CM * S, NP = h.sum(&Shape::np, S), NO = h.sum(&Shape::no, S), NPAIR = h.sum(&Shape::npair, S), P = h.P(), n = h.len[q];
    const size_t pt0 = h.sum(&Shape::np, q), ob0 = h.sum(&Shape::no, q), pr0 = h.sum(&Shape::npair, q), np = h.np(q), no = h.no(q);
    auto put = [&](const char* name, auto* whole, size_t total, auto* p, size_t off, size_t len) {
        v.push_back({name, (const uint8_t*)whole, (const uint8_t*)p, total * sizeof(*whole), off * sizeof(*whole), len * sizeof(*whole)});
    };
    const ChainBuf &C = b.cb, &c = e.cb; const SlamBuf &M = b.sb, &m = e.sb;
    put("off", C.off, 2 * S, c.off, 2 * q, 2); put("rvec", C.rvec, 3 * S, c.rvec, 3 * q, 3); put("tvec", C.tvec, 3 * S, c.tvec, 3 * q, 3);
    put("pmask", C.pmask, S * CAP, c.pmask, q * CAP, CAP); put("pninl", C.pninl, S, c.pninl, q, 1); put("pstatus", C.pstatus, S, c.pstatus, q, 1);
    put("P1", C.P1, 12 * S, c.P1, 12 * q, 12); put("P2", C.P2, 12 * S, c.P2, 12 * q, 12);
    put("obj", C.obj, S * CAP * 3, c.obj, q * CAP * 3, CAP * 3); put("img", C.img, S * CAP * 2, c.img, q * CAP * 2, CAP * 2); put("Xw", C.Xw, S * CAP * 4, c.Xw, q * CAP * 4, CAP * 4);
    put("alive", C.alive, S, c.alive, q, 1); put("map_count", C.map_count, S, c.map_count, q, 1); put("dec", M.dec, S * CAP, m.dec, q * CAP, CAP);
    put("n_corr", C.n_corr, P, c.n_corr, first, n); put("n_inl", C.n_inl, P, c.n_inl, first, n); put("status", C.status, P, c.status, first, n); put("n_map", C.n_map, P, c.n_map, first, n);
    put("poses", C.poses, (P + S) * 12, c.poses, (first + q) * 12, (n + 1) * 12); put("poses_last", M.poses_last, (P + S) * 12, m.poses_last, (first + q) * 12, (n + 1) * 12);
    put("n_pts", M.n_pts, P, m.n_pts, first, n); put("n_obs", M.n_obs, P, m.n_obs, first, n); put("n_cam", M.n_cam, P, m.n_cam, first, n);
    if (h.restart) {
        put("rs.st", C.rs.st, 4 * S, c.rs.st, 4 * q, 4); put("segment", C.rs.segment, P, c.rs.segment, first, n); put("cause", C.rs.cause, P, c.rs.cause, first, n);
        put("seg_poses", C.rs.seg_poses, P * 12, c.rs.seg_poses, first * 12, n * 12); put("seg_poses_last", C.rs.seg_poses_last, P * 12, c.rs.seg_poses_last, first * 12, n * 12);
    }
    put("cnt", M.m.cnt, 4 * S, m.m.cnt, 4 * q, 4); put("cam_frame", M.m.cam_frame, NC, m.m.cam_frame, CM * q, CM); put("cam_pose", M.m.cam_pose, NC * 12, m.m.cam_pose, CM * q * 12, CM * 12);
    put("cam_fixed", M.m.cam_fixed, NC, m.m.cam_fixed, CM * q, CM); put("pt_key", M.m.pt_key, NP, m.m.pt_key, pt0, np); put("pt_xyz", M.m.pt_xyz, NP * 3, m.m.pt_xyz, pt0 * 3, np * 3);
    put("obs_cam", M.m.obs_cam, NO, m.m.obs_cam, ob0, no); put("obs_pt", M.m.obs_pt, NO, m.m.obs_pt, ob0, no); put("obs_xy", M.m.obs_xy, NO * 2, m.m.obs_xy, ob0 * 2, no * 2);
    put("tmp", M.tmp, NP, m.tmp, pt0, np); put("idx", M.idx, NO, m.idx, ob0, no); put("prob", M.prob, S, m.prob, q, 1); put("cam_col", M.cam_col, NC, m.cam_col, CM * q, CM);
    put("pt_first", M.pt_first, NP + S, m.pt_first, pt0 + q, np + 1); put("s_cam", M.s_cam, NO, m.s_cam, ob0, no); put("s_pt", M.s_pt, NO, m.s_pt, ob0, no);
    put("s_xy", M.s_xy, NO * 2, m.s_xy, ob0 * 2, no * 2); put("pairs", M.pairs, NPAIR, m.pairs, pr0, h.npair(q)); put("blk_first", M.blk_first, S * (NBLK + 1), m.blk_first, q * (NBLK + 1), NBLK + 1);
    if (h.stream()) {
        put("pt_feat", M.m.pt_feat, NP * 2, m.m.pt_feat, pt0 * 2, np * 2);
        put("carried_frame", M.st.carried_frame, NC, m.st.carried_frame, CM * q, CM); put("carried_poses", M.st.carried_poses, NC * 12, m.st.carried_poses, CM * q * 12, CM * 12);
    }
    // the slot-keyed tables are the shared ones
    CHECK(c.parent == C.parent && c.in_map == C.in_map && c.map_pt == C.map_pt && c.cam == C.cam && c.cam_ok == C.cam_ok && m.pt_of == M.pt_of, "sequence %zu: a slot-keyed table is not the shared one", q);
    CHECK(m.cam_cap == (int)CM && m.pt_cap == (int)np && m.obs_cap == (int)no && m.pair_cap == (int)h.npair(q), "sequence %zu: capacities %d %d %d %d", q, m.cam_cap, m.pt_cap, m.obs_cap, m.pair_cap);
    CHECK(m.base.cam0 == (int)(CM * q) && m.base.pt0 == (int)pt0 && m.base.obs0 == (int)ob0 && m.base.pair0 == (int)pr0 && m.base.blk0 == (int)(q * (NBLK + 1)) && c.obj0 == (int)(q * CAP),
          "sequence %zu: bases %d %d %d %d %d, obj0 %d", q, m.base.cam0, m.base.pt0, m.base.obs0, m.base.pair0, m.base.blk0, c.obj0);
    CHECK(e.first == (int)first && e.count == (int)n, "sequence %zu: rows %d + %d", q, e.first, e.count);
    return v;
}

static void check(const Shape& h)
{
    char name[160];
    snprintf(name, sizeof name, "form %d S %zu total0 %zu restart %d stats %d snapshot %d", (int)h.form, h.S, h.total.empty() ? 0 : h.total[0], h.restart, h.stats, h.snapshot);
    g_case = name;
    const SlamDims d = dims_of(h);
    uint8_t* const base = reinterpret_cast<uint8_t*>((uintptr_t)0x7f0000000000ull);   // never read or written
    SlamBufs b;
    const size_t bytes = slam_layout(d, nullptr, b);
    CHECK(slam_layout(d, base, b) == bytes && b.bytes == bytes, "the size changes with the base");
    // 1, 2: every sub-buffer in [0, bytes) on a 256-byte boundary; together they tile it; the per-call ones are its tail from call0
    std::vector<Region> r = regions_of(h, b);
    std::sort(r.begin(), r.end(), [](const Region& x, const Region& y) { return x.p < y.p || (x.p == y.p && x.bytes < y.bytes); });
    size_t at = 0, stats_bytes = 0; bool tail = false;
    for (const Region& g : r) {
        const size_t off = (size_t)(g.p - base);
        CHECK(g.p >= base && off % 256 == 0 && off + g.bytes <= bytes, "%s: offset %zu, %zu bytes of %zu", g.name, off, g.bytes, bytes);
        CHECK(off == at, "%s: offset %zu, the buffers before it end at %zu", g.name, off, at);
        if (g.call && !tail) { tail = true; CHECK(off == b.call0, "%s: the per-call part starts at %zu, call0 = %zu", g.name, off, b.call0); }
        CHECK(g.call == tail, "%s: %s", g.name, g.call ? "a per-call buffer before call0" : "a buffer that outlives the call inside the per-call tail");
        at = off + up(g.bytes);
        if (g.stats) stats_bytes += up(g.bytes);
    }
    CHECK(at == bytes && tail && b.call0 < bytes, "the buffers end at %zu of %zu bytes", at, bytes);
    // the bundle adjustment's const members and the statistics' K are the step's own buffers
    CHECK(b.D.prob == b.sb.prob && b.D.poses == b.sb.m.cam_pose && b.D.cam_col == b.sb.cam_col && b.D.X == b.sb.m.pt_xyz && b.D.pt_first == b.sb.pt_first && b.D.obs_cam == b.sb.s_cam &&
          b.D.obs_pt == b.sb.s_pt && b.D.obs_xy == b.sb.s_xy && b.D.pairs == b.sb.pairs && b.D.blk_first == b.sb.blk_first, "BaBuf's const members");
    if (h.stats) CHECK(b.stats.Kd == b.dK && b.stats.C == (int)CM, "StatsBuf's K and C");
    // 3: the descriptors
    std::vector<std::vector<Member>> ms;
    size_t first = 0;
    for (size_t q = 0; q < h.S; q++) {
        const SlamSeq e = slam_seq(d, b, (int)q, (int)first, (int)h.len[q], 7, 2);
        ms.push_back(members_of(h, b, e, q, first));
        CHECK(e.sb.st.frame0 == (h.stream() ? 7 : 0) && e.sb.st.n_carried == (h.stream() ? 2 : 0), "sequence %zu: frame0 %d n_carried %d", q, e.sb.st.frame0, e.sb.st.n_carried);
        first += h.len[q];
    }
    for (size_t q = 0; q < h.S; q++)
        for (size_t i = 0; i < ms[q].size(); i++) {
            const Member& m = ms[q][i];
            CHECK(m.p == m.whole + m.off, "sequence %zu %s: at %td, the formulas say %zu", q, m.name, m.p - m.whole, m.off);
            CHECK(m.off + m.bytes <= m.whole_bytes, "sequence %zu %s: %zu + %zu bytes pass the array's %zu", q, m.name, m.off, m.bytes, m.whole_bytes);
            if (h.S == 1) CHECK(m.p == m.whole, "S = 1, %s: base %td", m.name, m.p - m.whole);
            for (size_t k = 0; k < q; k++) {
                const Member& o = ms[k][i];
                CHECK(o.p + o.bytes <= m.p || m.p + m.bytes <= o.p, "%s: sequences %zu and %zu overlap", m.name, k, q);
            }
        }
    // 4: statistics off cost nothing
    if (h.stats) {
        Shape off = h; off.stats = false;
        SlamBufs bo;
        CHECK(slam_layout(dims_of(off), nullptr, bo) == bytes - stats_bytes, "statistics off: %zu bytes, on %zu less the members' %zu", bo.bytes, bytes, stats_bytes);
    }
}

int main()
{
    int cases = 0;
    const std::vector<size_t> len3{2, 1, 3};
    for (int restart = 0; restart < 2; restart++)
        for (int stats = 0; stats < 2; stats++)
            for (int snapshot = 0; snapshot < 2; snapshot++) {
                const bool r = restart, t = stats, n = snapshot;
                std::vector<Shape> hs;
                if (!r) hs.push_back({CHAIN, 1, {2}, {}, false, t, n, 0});
                for (size_t ss = 0; ss < 3; ss++) hs.push_back({CHAINS, 3, len3, {}, r, t, n, ss});
                hs.push_back({CHAINS, 1, {2}, {}, r, t, n, 0});
                for (size_t total : {3, 4, 6}) hs.push_back({STREAM, 1, {2}, {total}, r, t, n, 0});           // total on both sides of cm = 4
                if (r) {                                              // (vo_slam_streams is a restart form)
                    hs.push_back({STREAMS, 3, len3, {2, 4, 7}, r, t, n, 1});
                    for (size_t total : {3, 6}) hs.push_back({STREAMS, 1, {2}, {total}, r, t, n, 0});
                }
                for (const Shape& h : hs) { check(h); cases++; }
            }
    printf("slam layout: %d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
