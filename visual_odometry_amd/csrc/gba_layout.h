// gba_layout.h — what the host prepares for one vo_bundle_adjust_large call (ba_large_api.hip) and where its device buffers lie:
// validation, the observations sorted by point (stable) with a CSR list per point, a CSR list per free camera, the list of the
// non-empty blocks (c1 <= c2) of the reduced camera system S with each block's observation pairs, and the scratch layout.
// Index arithmetic over std::vector and ScratchLayout only: nothing in this header calls the HIP runtime, so
// tests/native/gba_layout_driver.cpp runs it on a machine without a GPU.
#pragma once
#include "slam_layout.h"
#include <vector>

#define GBA_PANEL_CAMS 8                       // P: free cameras per panel of the blocked Cholesky
#define GBA_NB (6 * GBA_PANEL_CAMS)            // columns of a panel
#define GBA_TILE 48                            // T: rows and columns of a tile of the trailing update
#define GBA_THREADS 256                        // lanes of a workgroup of the per-point, per-block and tile kernels
#define GBA_PANEL_ROWS 64                      // rows of S below a panel's diagonal block that one workgroup solves

struct GbaBlock { int c1, c2; };               // a listed block of S: free cameras c1 <= c2

// The LM state on the device: k_gba_decide writes it, the host reads it once per trial (64 bytes).
struct GbaRec {
    double lam, nu, chi, rho;                  // lambda, nu, the current robust chi2, the last trial's gain ratio
    int fail;                                  // the trial's solver failed: every later kernel of the trial returns at once
    int accepted, go_on, stop;                 // the last trial's verdict: take the trial state; try again; end the LM loop
    int qmax;                                  // trials of this iteration that count towards g2o's limit of 10
    int pad[3];
};

struct GbaPlan {
    int ncam = 0, npt = 0, nobs = 0, nfree = 0;
    int n = 0, ld = 0;                         // S: 6 nfree columns, n + 1 rows (row n = g) of ld doubles
    int npw = 0;                               // workgroups of the per-point kernels = partials of the wide reductions
    std::vector<int> col, free_cam;            // [ncam] column block of a free camera or -1; [nfree] its camera
    std::vector<int> pt_first;                 // [npt + 1] CSR by point over the sorted observations
    std::vector<int> s_cam, s_pt;              // [nobs] the sorted observations
    std::vector<double> s_xy;                  // [nobs][2]
    std::vector<int> cam_first, cam_list;      // [nfree + 1] CSR by free camera; sorted-observation numbers, ascending
    std::vector<GbaBlock> blocks;              // every diagonal block, and the off-diagonal ones with a pair; by (c1, c2)
    std::vector<int> blk_first;                // [blocks + 1] offsets into pairs
    std::vector<int2> pairs;                   // (observation of c1, observation of c2) on a shared point: by point, then input order
    size_t s_doubles() const { return (size_t)(n + 1) * (size_t)ld; }
};

static inline int gba_ld(int n) { return (n + 1 + 7) & ~7; }    // row pitch of S in doubles: n columns and one more, a multiple of 8

// VO_OK, VO_ERR_UNSUPPORTED (more than VO_BA_LARGE_MAX_FREE free cameras, or more pairs than an int32 counts) or
// VO_ERR_INVALID (an observation of a missing camera or point).  Capacity is checked first, as vo_bundle_adjust does.
static inline int gba_prepare(int ncam, const uint8_t* cam_fixed, int npt, int nobs, const int32_t* obs_cam, const int32_t* obs_pt,
                              const double* obs_xy, GbaPlan& P)
{
    P = GbaPlan();
    if (ncam < 0 || npt < 0 || nobs < 0) return VO_ERR_INVALID;
    P.ncam = ncam; P.npt = npt; P.nobs = nobs;
    for (int i = 0; i < ncam; i++) if (!cam_fixed[i]) P.nfree++;
    if (P.nfree > VO_BA_LARGE_MAX_FREE) return VO_ERR_UNSUPPORTED;
    for (int i = 0; i < nobs; i++)
        if (obs_cam[i] < 0 || obs_cam[i] >= ncam || obs_pt[i] < 0 || obs_pt[i] >= npt) return VO_ERR_INVALID;
    const int F = P.nfree;
    P.n = 6 * F; P.ld = gba_ld(P.n);
    P.npw = (npt + GBA_THREADS - 1) / GBA_THREADS;
    P.col.assign(ncam, -1); P.free_cam.resize(F);
    for (int i = 0, f = 0; i < ncam; i++) if (!cam_fixed[i]) { P.col[i] = f; P.free_cam[f++] = i; }
    // counting sort by point, stable in input order
    P.pt_first.assign((size_t)npt + 1, 0);
    P.s_cam.resize(nobs); P.s_pt.resize(nobs); P.s_xy.resize((size_t)2 * nobs);
    for (int i = 0; i < nobs; i++) P.pt_first[obs_pt[i] + 1]++;
    for (int p = 0; p < npt; p++) P.pt_first[p + 1] += P.pt_first[p];
    std::vector<int> fill(P.pt_first.begin(), P.pt_first.end() - 1);
    for (int i = 0; i < nobs; i++) {
        const int j = fill[obs_pt[i]]++;
        P.s_cam[j] = obs_cam[i]; P.s_pt[j] = obs_pt[i];
        P.s_xy[2 * (size_t)j] = obs_xy[2 * (size_t)i]; P.s_xy[2 * (size_t)j + 1] = obs_xy[2 * (size_t)i + 1];
    }
    // every free camera's observations, ascending in the sorted order
    P.cam_first.assign((size_t)F + 1, 0);
    for (int j = 0; j < nobs; j++) { const int c = P.col[P.s_cam[j]]; if (c >= 0) P.cam_first[c + 1]++; }
    for (int c = 0; c < F; c++) P.cam_first[c + 1] += P.cam_first[c];
    P.cam_list.resize(F ? P.cam_first[F] : 0);
    fill.assign(P.cam_first.begin(), P.cam_first.end() - 1);
    for (int j = 0; j < nobs; j++) { const int c = P.col[P.s_cam[j]]; if (c >= 0) P.cam_list[fill[c]++] = j; }
    // the blocks that exist and their pairs: count, list the blocks by (c1, c2), then fill in point order
    std::vector<size_t> cnt((size_t)F * F, 0);
    for (int pass = 0; pass < 2; pass++) {
        for (int p = 0; p < npt; p++)
            for (int j1 = P.pt_first[p]; j1 < P.pt_first[p + 1]; j1++) {
                const int a = P.col[P.s_cam[j1]]; if (a < 0) continue;
                for (int j2 = P.pt_first[p]; j2 < P.pt_first[p + 1]; j2++) {
                    const int c = P.col[P.s_cam[j2]]; if (c < a) continue;
                    if (pass == 0) cnt[(size_t)a * F + c]++;
                    else P.pairs[cnt[(size_t)a * F + c]++] = make_int2(j1, j2);
                }
            }
        if (pass == 0) {
            size_t total = 0;
            for (int a = 0; a < F; a++)
                for (int c = a; c < F; c++) {
                    const size_t k = (size_t)a * F + c;
                    if (cnt[k] == 0 && a != c) continue;
                    P.blocks.push_back(GbaBlock{a, c});
                    P.blk_first.push_back((int)total);
                    const size_t here = cnt[k];
                    cnt[k] = total;                                  // from now on: where the block's next pair goes
                    total += here;
                    if (total > (size_t)INT32_MAX) { P = GbaPlan(); return VO_ERR_UNSUPPORTED; }
                }
            P.blk_first.push_back((int)total);
            P.pairs.resize(total);
        }
    }
    return VO_OK;
}

// The device side of a call.  cam / quat / X hold the current and the trial estimate; which is which flips at every accepted trial.
struct GbaBuf {
    const int *col, *free_cam, *pt_first, *obs_cam, *obs_pt, *cam_first, *cam_list, *blk_first;
    const GbaBlock* blocks; const int2* pairs; const double* obs_xy;
    double *cam[2], *quat[2], *X[2];               // [ncam][12] world -> camera [R | t]; [F][4] unit quaternions; [npt][3]
    double *W;                                     // [nobs][18]: w Jp^T Jx of a free camera's observation
    double *Hpp, *bp, *Hpi;                        // [npt][6], [3], [6] (symmetric: 00 01 02 11 12 22)
    double *Hcc, *bc, *dc;                         // [F][36], [F][6], [F][6]
    double *S;                                     // [(n + 1)][ld]: lower triangle of the reduced camera system, row n = g
    double *Ld;                                    // [panels][GBA_NB][GBA_NB]: the factored diagonal blocks (S keeps the unfactored ones)
    double *part_chi, *part_scale, *part_max;      // [npw] per-workgroup partials of the wide reductions, combined in index order
    GbaRec* rec;
    int ncam, npt, nobs, F, n, ld, nblk, npw;
};

// Scratch bytes of a call, each term rounded up to 256: the sum of what is taken here (stated in include/vo_hip.h).
static inline void gba_take(ScratchLayout& sc, const GbaPlan& P, GbaBuf& D)
{
    const size_t C = (size_t)P.ncam, N = (size_t)P.npt, O = (size_t)P.nobs, F = (size_t)P.nfree, W = (size_t)(P.npw ? P.npw : 1);
    sc.take(const_cast<int**>(&D.col), C); sc.take(const_cast<int**>(&D.free_cam), F); sc.take(const_cast<int**>(&D.pt_first), N + 1);
    sc.take(const_cast<int**>(&D.obs_cam), O); sc.take(const_cast<int**>(&D.obs_pt), O); sc.take(const_cast<double**>(&D.obs_xy), 2 * O);
    sc.take(const_cast<int**>(&D.cam_first), F + 1); sc.take(const_cast<int**>(&D.cam_list), P.cam_list.size());
    sc.take(const_cast<GbaBlock**>(&D.blocks), P.blocks.size()); sc.take(const_cast<int**>(&D.blk_first), P.blk_first.size());
    sc.take(const_cast<int2**>(&D.pairs), P.pairs.size());
    for (int k = 0; k < 2; k++) { sc.take(&D.cam[k], 12 * C); sc.take(&D.quat[k], 4 * F); sc.take(&D.X[k], 3 * N); }
    sc.take(&D.W, 18 * O); sc.take(&D.Hpp, 6 * N); sc.take(&D.bp, 3 * N); sc.take(&D.Hpi, 6 * N);
    sc.take(&D.Hcc, 36 * F); sc.take(&D.bc, 6 * F); sc.take(&D.dc, 6 * F); sc.take(&D.S, P.s_doubles());
    sc.take(&D.Ld, (size_t)GBA_NB * GBA_NB * (size_t)((P.n + GBA_NB - 1) / GBA_NB));
    sc.take(&D.part_chi, W); sc.take(&D.part_scale, W); sc.take(&D.part_max, W); sc.take(&D.rec, 1);
    D.ncam = P.ncam; D.npt = P.npt; D.nobs = P.nobs; D.F = P.nfree; D.n = P.n; D.ld = P.ld; D.nblk = (int)P.blocks.size(); D.npw = P.npw;
}

// vo_ba_large_solve's part of the layout: S, Ld, delta_c and the record of a system of n = 6 F unknowns, nothing else named.
static inline void gba_take_solve(ScratchLayout& sc, int n, GbaBuf& D)
{
    D.F = n / 6; D.n = n; D.ld = gba_ld(n);
    sc.take(&D.S, (size_t)(n + 1) * (size_t)D.ld);
    sc.take(&D.Ld, (size_t)GBA_NB * GBA_NB * (size_t)((n + GBA_NB - 1) / GBA_NB));
    sc.take(&D.dc, (size_t)n); sc.take(&D.rec, 1);
}

void launch_gba_init(hipStream_t s, const GbaBuf& D, const BaParams& P);
void launch_gba_linearise(hipStream_t s, const GbaBuf& D, const BaParams& P, int cur, bool first);
void launch_gba_trial(hipStream_t s, const GbaBuf& D, const BaParams& P, int cur, bool first_trial);
void launch_gba_factor_solve(hipStream_t s, const GbaBuf& D);
