// Driver of the sanitizer build of visual_odometry_amd/csrc/gba_layout.h (CPU only, no HIP call): reads one map's index arrays
// from the file named on the command line (ncam npt nobs, then the fixed flags, obs_cam, obs_pt), runs gba_prepare and gba_take
// on it and prints every list they made, one per line, for tests/test_gba_layout_host.py to hold against its numpy restatement.
// Observation i gets the coordinates (i, i + 0.5), so the sorted coordinates name the input observation they came from.  The
// layout is placed at a made-up base; the driver checks that every buffer lies inside it on a 256-byte boundary and overlaps none.
#include "gba_layout.h"
#include <stdio.h>

template <typename T> static void line(const char* name, const std::vector<T>& v)
{
    printf("%s", name);
    for (const T& x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: gba_layout_asan MAP_FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int ncam = 0, npt = 0, nobs = 0;
    if (fscanf(f, "%d %d %d", &ncam, &npt, &nobs) != 3 || ncam < 0 || npt < 0 || nobs < 0) { fclose(f); return 2; }
    std::vector<uint8_t> fixed(ncam);
    std::vector<int32_t> oc(nobs), op(nobs);
    std::vector<double> xy(2 * (size_t)nobs);
    bool ok = true;
    for (int i = 0; i < ncam; i++) { int v; ok = ok && fscanf(f, "%d", &v) == 1; fixed[i] = (uint8_t)v; }
    for (int i = 0; i < nobs; i++) ok = ok && fscanf(f, "%d", &oc[i]) == 1;
    for (int i = 0; i < nobs; i++) ok = ok && fscanf(f, "%d", &op[i]) == 1;
    fclose(f);
    if (!ok) { fprintf(stderr, "short file\n"); return 2; }
    for (int i = 0; i < nobs; i++) { xy[2 * (size_t)i] = i; xy[2 * (size_t)i + 1] = i + 0.5; }

    GbaPlan P;
    const int st = gba_prepare(ncam, fixed.data(), npt, nobs, oc.data(), op.data(), xy.data(), P);
    printf("status %d\n", st);
    if (st != VO_OK) return 0;
    printf("dims %d %d %d %d %d %d %d\n", P.ncam, P.npt, P.nobs, P.nfree, P.n, P.ld, P.npw);
    line("col", P.col); line("free_cam", P.free_cam); line("pt_first", P.pt_first); line("s_cam", P.s_cam); line("s_pt", P.s_pt);
    std::vector<int> src(nobs);
    int bad_xy = 0;
    for (int j = 0; j < nobs; j++) { src[j] = (int)P.s_xy[2 * (size_t)j]; if (P.s_xy[2 * (size_t)j + 1] != src[j] + 0.5) bad_xy++; }
    line("s_src", src);
    line("cam_first", P.cam_first); line("cam_list", P.cam_list); line("blk_first", P.blk_first);
    printf("blocks"); for (const GbaBlock& b : P.blocks) printf(" %d %d", b.c1, b.c2); printf("\n");
    printf("pairs"); for (const int2& p : P.pairs) printf(" %d %d", p.x, p.y); printf("\n");

    GbaBuf D{};
    ScratchLayout sc;
    gba_take(sc, P, D);
    std::vector<uint8_t> mem(sc.bytes + 256);
    uint8_t* base = mem.data() + (256 - ((uintptr_t)mem.data() & 255)) % 256;
    sc.place_at(base);
    struct Region { const char* name; const void* p; size_t bytes; };
    const size_t C = (size_t)ncam, N = (size_t)npt, O = (size_t)nobs, F = (size_t)P.nfree, W = (size_t)(P.npw ? P.npw : 1);
    const size_t panels = ((size_t)P.n + GBA_NB - 1) / GBA_NB;
    const std::vector<Region> rs = {
        {"col", D.col, 4 * C}, {"free_cam", D.free_cam, 4 * F}, {"pt_first", D.pt_first, 4 * (N + 1)}, {"obs_cam", D.obs_cam, 4 * O}, {"obs_pt", D.obs_pt, 4 * O},
        {"obs_xy", D.obs_xy, 16 * O}, {"cam_first", D.cam_first, 4 * (F + 1)}, {"cam_list", D.cam_list, 4 * P.cam_list.size()},
        {"blocks", D.blocks, 8 * P.blocks.size()}, {"blk_first", D.blk_first, 4 * P.blk_first.size()}, {"pairs", D.pairs, 8 * P.pairs.size()},
        {"cam0", D.cam[0], 96 * C}, {"cam1", D.cam[1], 96 * C}, {"quat0", D.quat[0], 32 * F}, {"quat1", D.quat[1], 32 * F}, {"X0", D.X[0], 24 * N}, {"X1", D.X[1], 24 * N},
        {"W", D.W, 144 * O}, {"Hpp", D.Hpp, 48 * N}, {"bp", D.bp, 24 * N}, {"Hpi", D.Hpi, 48 * N}, {"Hcc", D.Hcc, 288 * F}, {"bc", D.bc, 48 * F}, {"dc", D.dc, 48 * F},
        {"S", D.S, 8 * (size_t)(P.n + 1) * (size_t)P.ld}, {"Ld", D.Ld, 8 * (size_t)GBA_NB * GBA_NB * panels},
        {"part_chi", D.part_chi, 8 * W}, {"part_scale", D.part_scale, 8 * W}, {"part_max", D.part_max, 8 * W}, {"rec", D.rec, sizeof(GbaRec)}};
    int failures = bad_xy;
    printf("layout_bytes %zu\n", sc.bytes);
    for (size_t i = 0; i < rs.size(); i++) {
        const uint8_t* p = (const uint8_t*)rs[i].p;
        printf("region %s %zu %zu\n", rs[i].name, (size_t)(p - base), rs[i].bytes);
        if (!(p >= base && p + rs[i].bytes <= base + sc.bytes && ((uintptr_t)p & 255) == 0)) { failures++; printf("FAIL %s lies outside the allocation or off a 256-byte boundary\n", rs[i].name); }
        for (size_t j = 0; j < i; j++) {
            const uint8_t* q = (const uint8_t*)rs[j].p;
            if (rs[i].bytes && rs[j].bytes && !(p + rs[i].bytes <= q || q + rs[j].bytes <= p)) { failures++; printf("FAIL %s overlaps %s\n", rs[i].name, rs[j].name); }
        }
    }
    // the kernels' own bounds: S rows hold g's column of the diagonal, the last panel fits its Ld slot
    if (P.ld < P.n + 1 || (P.ld & 7)) { failures++; printf("FAIL ld %d for n %d\n", P.ld, P.n); }
    printf("gba_layout_driver: %d failures\n", failures);
    return failures ? 1 : 0;
}
