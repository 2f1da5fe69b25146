// geom_kernels.hip — two-view geometry on gfx950, float64, no MFMA (no dense contraction here).
//
// Replaces (reference call sites, paths relative to the reference repo):
//   cv2.findEssentialMat(p1, p2, K, cv2.FM_RANSAC, 0.99, 1)   src/image_pair.py:280-286
//   cv2.recoverPose(E, p1, p2, K)                              src/image_pair.py:304-308
//   cv2.triangulatePoints(P, P0, p1.T, p2.T) and `/= w`        src/image_pair.py:332-339
//
// Mapping: one workgroup (4 wavefronts) per frame pair.  A RANSAC round solves 16 five-point samples per
// solver wave, one per quad of lanes (Nister's solver: Householder null space, 10x20 elimination, degree-10
// root finding by Durand-Kerner); the models are then scored strictly in OpenCV's sequential order, each model
// by the 64 lanes of a wave over the correspondences with a wavefront ballot + popcount, so the adaptive
// iteration count (RANSACUpdateNumIters) and the strict `>` best-model rule are emulated exactly.
// Compiled with -ffp-contract=off: every operation rounds on its own.
#include "vo_internal.h"
#include "chain_common.h"
#include <float.h>

#define WAVE 64
// throughput mode gives up on a sample after this many sweeps (oracle/voo_geom.c VOO_DK_FAST_CAP: 0.07 % of the samples
// never settle, and one such lane would hold its wavefront for all 300 sweeps)
#ifndef VO_DK_FAST_CAP
#define VO_DK_FAST_CAP 64
#endif
#ifndef VO_DK_ITERS
#define VO_DK_ITERS 300
#endif

// hypot from IEEE operations only (same expression as the CPU oracle, so the rotations agree bit for bit)
__device__ __forceinline__ double vo_hypot(double a, double b)
{
    a = fabs(a); b = fabs(b);
    if (a < b) { double t = a; a = b; b = t; }
    if (a == 0) return 0;
    double r = b / a;
    return a * sqrt(1 + r * r);
}

// ------------------------------------------------------------------ one-sided Jacobi SVD
// At: N rows of length M (row i = column i of the M x N matrix). Returns At rows = sigma_i u_i,
// W descending, Vt rows = right singular vectors (Hestenes rotations, as OpenCV's JacobiSVDImpl_).
template <int M, int N>
__device__ __forceinline__ void jacobi_svd(double* At, double* W, double* Vt)
{
    const double eps = DBL_EPSILON * 10;
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += At[i * M + k] * At[i * M + k];
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < N; k++) Vt[i * N + k] = (k == i) ? 1.0 : 0.0;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < N - 1; i++) {
#pragma unroll
            for (int j = i + 1; j < N; j++) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < M; k++) p += At[i * M + k] * At[j * M + k];
                if (fabs(p) > eps * sqrt(a * b)) {
                    p *= 2;
                    double beta = a - b, gamma = vo_hypot(p, beta), c, s;
                    if (beta < 0) {
                        double delta = (gamma - beta) * 0.5;
                        s = sqrt(delta / gamma);
                        c = p / (gamma * s * 2);
                    } else {
                        c = sqrt((gamma + beta) / (gamma * 2));
                        s = p / (gamma * c * 2);
                    }
                    a = 0; b = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        double t0 = c * At[i * M + k] + s * At[j * M + k];
                        double t1 = -s * At[i * M + k] + c * At[j * M + k];
                        At[i * M + k] = t0; At[j * M + k] = t1;
                        a += t0 * t0; b += t1 * t1;
                    }
                    W[i] = a; W[j] = b;
                    changed = true;
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        double t0 = c * Vt[i * N + k] + s * Vt[j * N + k];
                        double t1 = -s * Vt[i * N + k] + c * Vt[j * N + k];
                        Vt[i * N + k] = t0; Vt[j * N + k] = t1;
                    }
                }
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += At[i * M + k] * At[i * M + k];
        W[i] = sqrt(sd);
    }
    // selection sort, descending (static indices only: compare-and-swap network of the same order)
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        // find j = argmax W[i..N) with the first maximum winning, as `if (W[j] < W[k]) j = k`
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) if (wj < W[k]) { j = k; wj = W[k]; }
#pragma unroll
        for (int k2 = i + 1; k2 < N; k2++) {
            if (j == k2) {
                double t = W[i]; W[i] = W[k2]; W[k2] = t;
#pragma unroll
                for (int k = 0; k < M; k++) { t = At[i * M + k]; At[i * M + k] = At[k2 * M + k]; At[k2 * M + k] = t; }
#pragma unroll
                for (int k = 0; k < N; k++) { t = Vt[i * N + k]; Vt[i * N + k] = Vt[k2 * N + k]; Vt[k2 * N + k] = t; }
            }
        }
    }
}

template <int N>
__device__ __forceinline__ void solve_z(const double* A, double* x)   // A row-major N x N
{
    double At[N * N], W[N], Vt[N * N];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int k = 0; k < N; k++) At[i * N + k] = A[k * N + i];
    jacobi_svd<N, N>(At, W, Vt);
#pragma unroll
    for (int k = 0; k < N; k++) x[k] = Vt[(N - 1) * N + k];
}

// ------------------------------------------------------------------ polynomial index tables
struct PolyTab { int t11[4][4]; int t21[10][4]; };

constexpr int k_e1[4][3] = {{1,0,0},{0,1,0},{0,0,1},{0,0,0}};
constexpr int k_e2[10][3] = {{2,0,0},{1,1,0},{1,0,1},{1,0,0},{0,2,0},{0,1,1},{0,1,0},{0,0,2},{0,0,1},{0,0,0}};
// Nister's elimination order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
constexpr int k_e3[20][3] = {
    {3,0,0},{0,3,0},{2,1,0},{1,2,0},{2,0,1},{2,0,0},{0,2,1},{0,2,0},{1,1,1},{1,1,0},
    {1,0,2},{1,0,1},{1,0,0},{0,1,2},{0,1,1},{0,1,0},{0,0,3},{0,0,2},{0,0,1},{0,0,0}};

constexpr PolyTab make_poly_tab()
{
    PolyTab t{};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            int a = k_e1[i][0] + k_e1[j][0], b = k_e1[i][1] + k_e1[j][1], c = k_e1[i][2] + k_e1[j][2];
            int idx = -1;
            for (int m = 0; m < 10; m++) if (k_e2[m][0] == a && k_e2[m][1] == b && k_e2[m][2] == c) idx = m;
            t.t11[i][j] = idx;
        }
    for (int i = 0; i < 10; i++)
        for (int j = 0; j < 4; j++) {
            int a = k_e2[i][0] + k_e1[j][0], b = k_e2[i][1] + k_e1[j][1], c = k_e2[i][2] + k_e1[j][2];
            int idx = -1;
            for (int m = 0; m < 20; m++) if (k_e3[m][0] == a && k_e3[m][1] == b && k_e3[m][2] == c) idx = m;
            t.t21[i][j] = idx;
        }
    return t;
}

__device__ __forceinline__ void mul11_acc(const double* p, const double* q, double s, double* r)
{
    constexpr PolyTab T = make_poly_tab();
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) r[T.t11[i][j]] += s * p[i] * q[j];
}

__device__ __forceinline__ void mul21_acc(const double* p, const double* q, double s, double* r)
{
    constexpr PolyTab T = make_poly_tab();
#pragma unroll
    for (int i = 0; i < 10; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) r[T.t21[i][j]] += s * p[i] * q[j];
}

struct cplx { double re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx cdiv(cplx a, cplx b)
{
    double t = 1. / (b.re * b.re + b.im * b.im);
    return {(a.re * b.re + a.im * b.im) * t, (-a.re * b.im + a.im * b.re) * t};
}

template <int NA, int NB>
__device__ __forceinline__ void conv(const double* a, const double* b, double* r)   // degrees NA, NB
{
#pragma unroll
    for (int i = 0; i <= NA + NB; i++) r[i] = 0;
#pragma unroll
    for (int i = 0; i <= NA; i++)
#pragma unroll
        for (int j = 0; j <= NB; j++) r[i + j] += a[i] * b[j];
}

// ------------------------------------------------------------------ quad exchange
// A five-point sample is solved by four adjacent lanes (a quad).  Values travel inside the quad with DPP quad_perm
// moves, a double as its two 32-bit halves; every lane of the quad must be active at such a move.
template <int O>
__device__ __forceinline__ int quad_bcast(int v) { return __builtin_amdgcn_mov_dpp(v, O * 0x55, 0xf, 0xf, true); }
template <int O>
__device__ __forceinline__ double quad_bcast(double v)
{
    const int lo = quad_bcast<O>(__double2loint(v)), hi = quad_bcast<O>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_bcast_from(int o, double v)      // o: a constant once the caller's loop is unrolled
{
    switch (o) {
    case 0: return quad_bcast<0>(v);
    case 1: return quad_bcast<1>(v);
    case 2: return quad_bcast<2>(v);
    default: return quad_bcast<3>(v);
    }
}
__device__ __forceinline__ double sel4(int q, double a, double b, double c, double d) { return q == 0 ? a : q == 1 ? b : q == 2 ? c : d; }

// cv::solvePoly's Durand-Kerner sweeps (Gauss-Seidel updates from the starting points (1+i)^k).  OpenCV always runs its
// 300 sweeps (its exit test is maxDiff <= 0); early == false does the same (vo_set_poly_solver(ctx, 1)).  With early ==
// true a sample stops as soon as further sweeps can only move rounding noise: every correction below 4 ulp of its root,
// or the largest correction has been small and has stopped shrinking for two sweeps (the noise floor of an
// ill-conditioned / multiple root).  The roots agree with the full iteration to that noise floor; the exit is per
// sample, so a sample's result does not depend on its wave mates.
//
// dk_exit: the exit rule after a sweep, shared by the two forms below.  max_diff is the largest SQUARED correction.
__device__ __forceinline__ bool dk_exit(double max_diff, double max_mag, bool conv_all, bool early, double& prev, int& stall)
{
    if (max_diff <= 0 || (early && conv_all)) return true;
    const double small = 1e-7 * (1.0 + max_mag);
    if (early && max_diff < small * small) {
        if (max_diff > 0.25 * prev) { if (++stall >= 2) return true; }
        else stall = 0;
    }
    prev = max_diff;
    return false;
}

// Degree 10, the normal case: the work of a sweep is dealt over the quad, the root state (rr, ri) is replicated in its
// four lanes.  Lane q owns the roots q, q + 4, q + 8 (slots 0..2; slot 2 is idle in lanes 2 and 3).
//  - The polynomial value at root i depends only on last sweep's root i: each lane runs the Horner recurrences of its
//    three roots, interleaved, each in the operation order of the sequential form.
//  - The denominator of root k is c10 * prod_{j != k} (p_k - r_j) taken in ascending j, with this sweep's new r_j for
//    j < k.  Each lane keeps the running products of its roots; as soon as root i is new, every lane multiplies the factor
//    j = i into the products of the roots k > i it owns, so a product receives its factors in ascending j.  At step i the
//    owner of root i appends the old-root factors j > i, divides, and hands the correction to the quad.
//  - Every lane applies the correction to its copy of root i and runs the exit tests itself: all four lanes hold the same
//    values, so the exit is uniform over the quad.
__device__ __forceinline__ void dk_iterate_quad(const double* c, double* rr, double* ri, bool early, int q)
{
    double prev = 1e300;
    int stall = 0;
    const int sweeps = early ? VO_DK_FAST_CAP : VO_DK_ITERS;
#pragma unroll 1
    for (int iter = 0; iter < sweeps; iter++) {
        bool conv_all = true;
        double max_diff = 0, max_mag = 0;
        double pr[3], pi[3], nr[3], ni[3], dr[3], di[3];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            pr[t] = sel4(q, rr[4 * t], rr[4 * t + 1], rr[4 * t + 2], rr[4 * t + 3]);
            pi[t] = sel4(q, ri[4 * t], ri[4 * t + 1], ri[4 * t + 2], ri[4 * t + 3]);
        }
        pr[2] = (q & 1) ? rr[9] : rr[8]; pi[2] = (q & 1) ? ri[9] : ri[8];
#pragma unroll
        for (int t = 0; t < 3; t++) { nr[t] = c[10]; ni[t] = 0; dr[t] = c[10]; di[t] = 0; }
#pragma unroll
        for (int j = 0; j < 10; j++)
#pragma unroll
            for (int t = 0; t < 3; t++) {
                const cplx np = cmul({nr[t], ni[t]}, {pr[t], pi[t]});
                nr[t] = np.re + c[9 - j]; ni[t] = np.im;
            }
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const int t = i >> 2, o = i & 3;
            // owner: the old-root factors j > i (lanes that do not own root i compute on, their result is not used)
            cplx denom = {dr[t], di[t]};
#pragma unroll
            for (int j = i + 1; j < 10; j++) denom = cmul(denom, {pr[t] - rr[j], pi[t] - ri[j]});
            // Two estimates exactly equal: OpenCV skips that factor.  A factor (0, 0) leaves both parts of every later
            // product at zero or NaN, so only such a product is formed again with the exact test; one that merely
            // underflowed has no factor to skip and comes out the same.
            const bool coincident = q == o && !(fabs(denom.re) > 0) && !(fabs(denom.im) > 0);
            if (__any(coincident)) {                     // wave-uniform branch; never taken from the distinct starting points (1+i)^k in practice
                if (coincident) {
                    denom = {c[10], 0};
#pragma unroll
                    for (int j = 0; j < 10; j++)
                        if (j != i) {
                            const cplx d = {rr[i] - rr[j], ri[i] - ri[j]};
                            if (d.re != 0 || d.im != 0) denom = cmul(denom, d);
                        }
                }
            }
            cplx num = cdiv({nr[t], ni[t]}, denom);
            num.re = quad_bcast_from(o, num.re); num.im = quad_bcast_from(o, num.im);
            rr[i] = rr[i] - num.re; ri[i] = ri[i] - num.im;
            // squared magnitudes: the exit tests compare squares (no square root per root)
            const double ab2 = num.re * num.re + num.im * num.im;
            max_diff = fmax(max_diff, ab2);
            const double mag = fabs(rr[i]) + fabs(ri[i]);
            max_mag = fmax(max_mag, mag);
            const double lim = 4 * DBL_EPSILON * mag;
            conv_all &= ab2 <= lim * lim;
            // the new root i is the factor j = i of every root k > i
#pragma unroll
            for (int t2 = t; t2 < 3; t2++) {
                if (t2 == t && o == 3) continue;
                const cplx m = cmul({dr[t2], di[t2]}, {pr[t2] - rr[i], pi[t2] - ri[i]});
                const bool mine = t2 > t || q > o;
                dr[t2] = mine ? m.re : dr[t2]; di[t2] = mine ? m.im : di[t2];
            }
        }
        if (dk_exit(max_diff, max_mag, conv_all, early, prev, stall)) break;
    }
}

// Degree below 10 (a vanishing leading coefficient, rare): the sequential form, run by every lane of the quad on its copy.
__device__ __forceinline__ void dk_iterate_low(const double* c, int n, double* rr, double* ri, bool early)
{
    // s[k] = c[k - (10 - n)]: the coefficients moved up so that the leading one sits at s[10] and coefficient n - 1 - j at
    // s[9 - j], by 10 - n one-place moves under a select (c[n - 1 - j] itself would be a dynamic index, i.e. scratch)
    double s[11];
#pragma unroll
    for (int k = 0; k <= 10; k++) s[k] = c[k];
#pragma unroll
    for (int step = 0; step < 9; step++) {
        const bool move = step < 10 - n;
#pragma unroll
        for (int k = 10; k >= 1; k--) s[k] = move ? s[k - 1] : s[k];
        s[0] = move ? 0.0 : s[0];
    }
    double prev = 1e300;
    int stall = 0;
    const int sweeps = early ? VO_DK_FAST_CAP : VO_DK_ITERS;
#pragma unroll 1
    for (int iter = 0; iter < sweeps; iter++) {
        bool conv_all = true;
        double max_diff = 0, max_mag = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            if (i < n) {
                cplx p = {rr[i], ri[i]};
                const double lead = s[10];
                cplx num = {lead, 0}, denom = {lead, 0};
#pragma unroll
                for (int j = 0; j < 10; j++) {
                    if (j < n) {
                        const double cj = s[9 - j];
                        cplx np = cmul(num, p);
                        num.re = np.re + cj; num.im = np.im;
                        if (j != i) {
                            cplx d = {p.re - rr[j], p.im - ri[j]};
                            if (d.re != 0 || d.im != 0) denom = cmul(denom, d);
                        }
                    }
                }
                num = cdiv(num, denom);
                rr[i] = p.re - num.re; ri[i] = p.im - num.im;
                const double ab2 = num.re * num.re + num.im * num.im;
                max_diff = fmax(max_diff, ab2);
                const double mag = fabs(rr[i]) + fabs(ri[i]);
                max_mag = fmax(max_mag, mag);
                const double lim = 4 * DBL_EPSILON * mag;
                conv_all &= ab2 <= lim * lim;
            }
        }
        if (dk_exit(max_diff, max_mag, conv_all, early, prev, stall)) break;
    }
}

// One column of the Gauss-Jordan elimination with partial pivoting, on the quad's 10 x 20 matrix held in registers: lane q
// has the columns 5q .. 5q+4 in cmr.  COL is a template argument so that every register index is a constant (a loop
// over the columns is only unrolled in part, which sends the matrix to scratch).  The owner of column COL hands it to
// the quad; the pivot search runs in all four lanes on the same values, so the pivot row and the singular exit (false)
// are uniform over the quad.  The pivot row is read and written through selects.
template <int COL>
__device__ __forceinline__ bool elim_step(double (&cmr)[10][5])
{
    double colv[10];
#pragma unroll
    for (int r = 0; r < 10; r++) colv[r] = quad_bcast<COL / 5>(cmr[r][COL % 5]);
    int piv = COL;
    double best = fabs(colv[COL]), pv = colv[COL];
#pragma unroll
    for (int r = COL + 1; r < 10; r++) { const double v = fabs(colv[r]); if (v > best) { best = v; piv = r; pv = colv[r]; } }
    if (best < 1e-300) return false;
    double prow[5];
    const double inv = 1.0 / pv;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const double b = cmr[COL][j];
        double a = b;
#pragma unroll
        for (int r = COL + 1; r < 10; r++) a = piv == r ? cmr[r][j] : a;
        prow[j] = a * inv;
#pragma unroll
        for (int r = COL + 1; r < 10; r++) cmr[r][j] = piv == r ? b : cmr[r][j];      // row swap (no-op when piv == COL)
        cmr[COL][j] = prow[j];
    }
#pragma unroll
    for (int r = 0; r < 10; r++) {
        if (r == COL) continue;
        const double f = (r > COL && piv == r) ? colv[COL] : colv[r];       // column COL after the swap
        const bool skip = f == 0;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const double v = cmr[r][j] - f * prow[j];
            cmr[r][j] = skip ? cmr[r][j] : v;
        }
    }
    return true;
}

// ------------------------------------------------------------------ five-point solver, one sample per quad
// x1, x2: 5 normalised correspondences (interleaved x,y). Writes up to 10 row-major 3x3 models
// (x2^T E x1 = 0, unit Frobenius norm) to Eout and returns their number.  Called by the four lanes of a quad with the
// same arguments (q = lane & 3); the return value and every early return are uniform over the quad.
//   null space, constraints, polynomial: every lane computes them (the same values in the four lanes)
//   10x20 elimination: lane q owns the columns 5q .. 5q+4 and keeps them in registers; the pivot column travels by
//   quad broadcast, the row swap is a select chain over the rows (no LDS, no dynamic register index)
//   Durand-Kerner: see dk_iterate_quad
//   models: the real roots are dealt over the lanes in ascending index, four per pass
// park: the wave's block of LDS, FP_PARK doubles per sample.  What is cold while the roots are found (the null-space
// basis and B(z), 150 registers) waits there, so that the sweep loop runs in about 120 registers and the kernel fits
// two waves per SIMD.  Value i of the quad's sample sits at park[i * FP_QUADS + lane / 4]; the four lanes hold the
// same values, each writes all of them and reads back what it wrote (no exchange, so no barrier).
#define FP_QUADS 16          // samples a wave solves at once
#define FP_PARK 75           // 36 basis + 12 Bx + 12 By + 15 Bc
typedef __attribute__((address_space(3))) double lds_double;
#define PARK(i) park[(i) * FP_QUADS + (lane >> 2)]

__device__ __forceinline__ int five_point_solve_quad(const double* x1, const double* x2, double* Eout, lds_double* park, bool dk_early)
{
    const int lane = threadIdx.x & 63, q = lane & 3;
    double cmr[10][5];       // element (r, 5q + j) of the 10 x 20 constraint matrix
    double basis[36];
    {
        // Householder QR of Q^T (9 x 5); null space = last 4 columns of the orthogonal factor
        double A[9][5], V[5][9];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            double u1 = x1[2 * i], v1 = x1[2 * i + 1], u2 = x2[2 * i], v2 = x2[2 * i + 1];
            A[0][i] = u2 * u1; A[1][i] = u2 * v1; A[2][i] = u2;
            A[3][i] = v2 * u1; A[4][i] = v2 * v1; A[5][i] = v2;
            A[6][i] = u1; A[7][i] = v1; A[8][i] = 1.0;
        }
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            double nrm = 0;
#pragma unroll
            for (int r = k; r < 9; r++) nrm += A[r][k] * A[r][k];
            nrm = sqrt(nrm);
            bad |= nrm < 1e-300;
            double alpha = A[k][k] > 0 ? -nrm : nrm;
#pragma unroll
            for (int r = 0; r < 9; r++) V[k][r] = r < k ? 0.0 : A[r][k];
            V[k][k] -= alpha;
            double vn = 0;
#pragma unroll
            for (int r = k; r < 9; r++) vn += V[k][r] * V[k][r];
            vn = sqrt(vn);
            bad |= vn < 1e-300;
#pragma unroll
            for (int r = k; r < 9; r++) V[k][r] /= vn;
#pragma unroll
            for (int c = k; c < 5; c++) {
                double d = 0;
#pragma unroll
                for (int r = k; r < 9; r++) d += V[k][r] * A[r][c];
#pragma unroll
                for (int r = k; r < 9; r++) A[r][c] -= 2 * d * V[k][r];
            }
        }
        if (bad) return 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double e[9];
#pragma unroll
            for (int r = 0; r < 9; r++) e[r] = (r == 5 + j) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 4; k >= 0; k--) {
                double d = 0;
#pragma unroll
                for (int r = k; r < 9; r++) d += V[k][r] * e[r];
#pragma unroll
                for (int r = k; r < 9; r++) e[r] -= 2 * d * V[k][r];
            }
#pragma unroll
            for (int r = 0; r < 9; r++) basis[j * 9 + r] = e[r];
        }
    }

    // 10 cubic constraints in (x, y, z): det(E) = 0 and (E E^T - 0.5 tr(E E^T) I) E = 0; each lane stores its columns
    {
        double E[3][3][4];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int k = 0; k < 4; k++) E[r][c][k] = basis[k * 9 + r * 3 + c];
        {
            double row[20];
#pragma unroll
            for (int i = 0; i < 20; i++) row[i] = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                double m[10];
#pragma unroll
                for (int i = 0; i < 10; i++) m[i] = 0;
                mul11_acc(E[1][c1], E[2][c2], 1.0, m);
                mul11_acc(E[1][c2], E[2][c1], -1.0, m);
                mul21_acc(m, E[0][c], 1.0, row);
            }
#pragma unroll
            for (int j = 0; j < 5; j++) cmr[0][j] = sel4(q, row[j], row[5 + j], row[10 + j], row[15 + j]);
        }
        // E E^T - 0.5 tr(E E^T) I: the diagonal first (the trace needs all of it), then one row of off-diagonal entries
        // at a time, so that three of the nine products are alive at once
        double D[3][10], tr[10];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int i = 0; i < 10; i++) D[r][i] = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) mul11_acc(E[r][k], E[r][k], 1.0, D[r]);
        }
#pragma unroll
        for (int i = 0; i < 10; i++) tr[i] = D[0][i] + D[1][i] + D[2][i];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 10; i++) D[r][i] -= 0.5 * tr[i];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double L[3][10];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (c == r) {
#pragma unroll
                    for (int i = 0; i < 10; i++) L[c][i] = D[r][i];
                } else {
#pragma unroll
                    for (int i = 0; i < 10; i++) L[c][i] = 0;
#pragma unroll
                    for (int k = 0; k < 3; k++) mul11_acc(E[r][k], E[c][k], 1.0, L[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                double row[20];
#pragma unroll
                for (int i = 0; i < 20; i++) row[i] = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) mul21_acc(L[k], E[k][c], 1.0, row);
#pragma unroll
                for (int j = 0; j < 5; j++) cmr[1 + r * 3 + c][j] = sel4(q, row[j], row[5 + j], row[10 + j], row[15 + j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 36; i++) PARK(i) = basis[i];

    // Gauss-Jordan with partial pivoting on the left 10 columns, one instance of the step per column
    if (!elim_step<0>(cmr) || !elim_step<1>(cmr) || !elim_step<2>(cmr) || !elim_step<3>(cmr) || !elim_step<4>(cmr) ||
        !elim_step<5>(cmr) || !elim_step<6>(cmr) || !elim_step<7>(cmr) || !elim_step<8>(cmr) || !elim_step<9>(cmr)) return 0;

    // B(z) [x y 1]^T = 0, from the rows 4..9 of the right half (the columns of lanes 2 and 3)
    double Bx[3][4], By[3][4], Bc[3][5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double r1[10], r2[10];
#pragma unroll
        for (int k = 0; k < 10; k++) {
            r1[k] = quad_bcast_from(2 + k / 5, cmr[2 * i + 4][k % 5]);
            r2[k] = quad_bcast_from(2 + k / 5, cmr[2 * i + 5][k % 5]);
        }
        Bx[i][3] = -r2[0]; Bx[i][2] = r1[0] - r2[1]; Bx[i][1] = r1[1] - r2[2]; Bx[i][0] = r1[2];
        By[i][3] = -r2[3]; By[i][2] = r1[3] - r2[4]; By[i][1] = r1[4] - r2[5]; By[i][0] = r1[5];
        Bc[i][4] = -r2[6]; Bc[i][3] = r1[6] - r2[7]; Bc[i][2] = r1[7] - r2[8]; Bc[i][1] = r1[8] - r2[9]; Bc[i][0] = r1[9];
    }
    double c[11];
    {
        double t1[8], t2[8], t3[11];
#pragma unroll
        for (int i = 0; i < 11; i++) c[i] = 0;
        conv<3, 4>(By[1], Bc[2], t1); conv<3, 4>(By[2], Bc[1], t2);
#pragma unroll
        for (int i = 0; i < 8; i++) t1[i] -= t2[i];
        conv<3, 7>(Bx[0], t1, t3);
#pragma unroll
        for (int i = 0; i < 11; i++) c[i] += t3[i];
        conv<3, 4>(Bx[1], Bc[2], t1); conv<3, 4>(Bx[2], Bc[1], t2);
#pragma unroll
        for (int i = 0; i < 8; i++) t1[i] -= t2[i];
        conv<3, 7>(By[0], t1, t3);
#pragma unroll
        for (int i = 0; i < 11; i++) c[i] -= t3[i];
        conv<3, 3>(Bx[1], By[2], t1); conv<3, 3>(Bx[2], By[1], t2);
#pragma unroll
        for (int i = 0; i < 7; i++) t1[i] -= t2[i];
        conv<4, 6>(Bc[0], t1, t3);
#pragma unroll
        for (int i = 0; i < 11; i++) c[i] += t3[i];
    }

    // B(z) waits in LDS for the model stage; the compiler barrier keeps it from carrying the values over in registers
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 4; k++) { PARK(36 + i * 4 + k) = Bx[i][k]; PARK(48 + i * 4 + k) = By[i][k]; }
#pragma unroll
        for (int k = 0; k < 5; k++) PARK(60 + i * 5 + k) = Bc[i][k];
    }
    __asm__ volatile("" ::: "memory");

    // cv::solvePoly: Durand-Kerner from the starting points (1+i)^k, Gauss-Seidel updates
    int n = 10;
#pragma unroll
    for (int k = 10; k > 1; k--) if (n == k && !(fabs(c[k]) > DBL_EPSILON)) n = k - 1;      // a select chain, not c[n]
    double rr[10], ri[10];
    {
        cplx p = {1, 0}, r = {1, 1};
#pragma unroll
        for (int i = 0; i < 10; i++) { rr[i] = p.re; ri[i] = p.im; p = cmul(p, r); }
    }
    if (n == 10) dk_iterate_quad(c, rr, ri, dk_early, q);
    else dk_iterate_low(c, n, rr, ri, dk_early);

    // real roots, in ascending index (OpenCV's order): root number 4 * pass + q of the sample goes to lane q, so a
    // sample needs at most three passes.  The models a pass keeps are stored in root order by the whole quad.
    uint32_t real_mask = 0;
#pragma unroll
    for (int k = 0; k < 10; k++) {
        double zi = ri[k];
        if (fabs(zi) < 1e-100) zi = 0;
        if (k < n && !(fabs(zi) > 1e-10)) real_mask |= 1u << k;
    }
    const int nreal = __popc(real_mask);
    int count = 0;
#pragma unroll 1
    for (int m0 = 0; m0 < nreal; m0 += 4) {
        const int m = m0 + q;
        double zr = 0;
        {
            int ord = 0;
#pragma unroll
            for (int k = 0; k < 10; k++) {
                const bool set = (real_mask >> k) & 1;
                if (set && ord == m) zr = rr[k];
                ord += set;
            }
        }
        double en[9];
#pragma unroll
        for (int k = 0; k < 9; k++) en[k] = 0;
        int keep = 0;
        if (m < nreal) {
            double z1 = zr, z2 = z1 * z1, z3 = z2 * z1, z4 = z3 * z1;
            double bz[9], xy1[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int bx = 36 + j * 4, by = 48 + j * 4, bc = 60 + j * 5;      // B(z) and the basis come back from LDS
                bz[j * 3 + 0] = PARK(bx + 3) * z3 + PARK(bx + 2) * z2 + PARK(bx + 1) * z1 + PARK(bx);
                bz[j * 3 + 1] = PARK(by + 3) * z3 + PARK(by + 2) * z2 + PARK(by + 1) * z1 + PARK(by);
                bz[j * 3 + 2] = PARK(bc + 4) * z4 + PARK(bc + 3) * z3 + PARK(bc + 2) * z2 + PARK(bc + 1) * z1 + PARK(bc);
            }
            solve_z<3>(bz, xy1);
            if (!(fabs(xy1[2]) < 1e-10)) {
                double x = xy1[0] / xy1[2], y = xy1[1] / xy1[2], nrm = 0, e[9];
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    e[k] = PARK(k) * x + PARK(9 + k) * y + PARK(18 + k) * z1 + PARK(27 + k);
                    nrm += e[k] * e[k];
                }
                nrm = sqrt(nrm);
#pragma unroll
                for (int k = 0; k < 9; k++) en[k] = e[k] / nrm;
                keep = 1;
            }
        }
        // the quad stores lane o's model: every branch below is uniform over the quad
#define FP_STORE_MODEL(o)                                                                             \
        if (quad_bcast<o>(keep)) {                                                                    \
            double w[9];                                                                              \
            _Pragma("unroll") for (int k = 0; k < 9; k++) w[k] = quad_bcast<o>(en[k]);                \
            double* dst = Eout + count * 9;                                                           \
            dst[q] = sel4(q, w[0], w[1], w[2], w[3]);                                                 \
            dst[4 + q] = sel4(q, w[4], w[5], w[6], w[7]);                                             \
            dst[8] = w[8];                                                                            \
            count++;                                                                                  \
        }
        FP_STORE_MODEL(0) FP_STORE_MODEL(1) FP_STORE_MODEL(2) FP_STORE_MODEL(3)
#undef FP_STORE_MODEL
    }
    return count;
}

// ------------------------------------------------------------------ RANSAC helpers
__device__ __forceinline__ uint32_t rng_next(uint64_t& state)
{
    state = (uint64_t)(uint32_t)state * 4164903690ULL + (uint32_t)(state >> 32);
    return (uint32_t)state;
}

__device__ int ransac_update_num_iters(double p, double ep, int model_points, int max_iters)
{
    p = fmax(p, 0.); p = fmin(p, 1.);
    ep = fmax(ep, 0.); ep = fmin(ep, 1.);
    double num = fmax(1. - p, DBL_MIN);
    double denom = 1. - pow(1. - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : __double2int_rn(num / denom);
}

// Sampson error as EMEstimatorCallback::computeError stores it (float32)
__device__ __forceinline__ float sampson_err(const double* E, double u1, double v1, double u2, double v2)
{
    double Ex0 = E[0] * u1 + E[1] * v1 + E[2], Ex1 = E[3] * u1 + E[4] * v1 + E[5], Ex2 = E[6] * u1 + E[7] * v1 + E[8];
    double Et0 = E[0] * u2 + E[3] * v2 + E[6], Et1 = E[1] * u2 + E[4] * v2 + E[7];
    double d = u2 * Ex0 + v2 * Ex1 + Ex2;
    return (float)(d * d / (Ex0 * Ex0 + Ex1 * Ex1 + Et0 * Et0 + Et1 * Et1));
}

// inliers of one model counted by one wavefront (ballot + popcount); optionally writes the mask
__device__ __forceinline__ int count_inliers(const double* E, const double* x1, const double* x2, int M, float t,
                                             int lane, int stride, int first, uint8_t* mask_out)
{
    int good = 0;
    for (int base = first; base < M; base += stride) {
        const int i = base + lane;
        bool f = false;
        if (i < M) {
            f = sampson_err(E, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]) <= t;
            if (mask_out) mask_out[i] = f ? 1 : 0;
        }
        good += __popcll(__ballot(f));
    }
    return good;
}

// ------------------------------------------------------------------ RANSACPointSetRegistrator::run, one workgroup (4 waves) per pair
// Round = RS_ROUND minimal samples, 16 per solver wave (one per quad) — the adaptive count ends at 9..30 on textured
// pairs (one round), 50..1000 on wide-baseline or low-inlier pairs; the solver parks 9.6 KB per solver wave in LDS, the
// elimination runs in registers and the models live in global memory (L2).  The kernel is held to RS_OCC waves per SIMD
// (256 registers) and 43 KB of LDS, so two workgroups, or another context's kernels, fit on a CU beside it.  E, mask and inlier count do not depend on the
// round size; the reported iteration count can, where a sample without models sits at the end of a round.
// (1) sample indices: the RNG stream (OpenCV's MWC, data independent) is read
// from a table, `% M` is taken by all threads in parallel, thread 0 only applies the repeat rejection;
// (2) the first RS_SOLVERS waves solve the samples, one per quad, elimination matrices in registers; (3) the models
// are scored four at a time (one per wave, ballot + popcount over the correspondences) and consumed strictly
// in OpenCV's order, so the adaptive iteration count and the strict `>` rule behave as in the serial loop.
#define RS_STREAM 512                     // RNG numbers staged per round (up to 64 subsets x 5 + rejections)
#define RS_SCORE_G 4                       // models a wave scores at once
#ifndef RS_WAVES
#define RS_WAVES 4                         // wavefronts of the workgroup: the first RS_SOLVERS solve, all of them score
#endif
#ifndef RS_SOLVERS
#define RS_SOLVERS 4                       // solver waves: 1, 2 or 4 -> 16, 32 or 64 samples and 10, 19 or 38 KB of LDS per round
#endif                                     // (measured: 2 and 4 tie while one round serves every pair, 4 wins beyond; docs/experiments.md)
#ifndef RS_OCC
#define RS_OCC 2                           // waves per SIMD the register allocation is held to: 2 -> at most 256 registers
#endif
#define RS_ROUND (FP_QUADS * RS_SOLVERS)
#define RS_THREADS (64 * RS_WAVES)
static_assert(RS_SOLVERS >= 1 && RS_SOLVERS <= RS_WAVES && RS_ROUND <= 64, "the sampler and the model list hold at most 64 samples per round");

struct RansacShared {
    double park[FP_PARK * RS_ROUND];
    uint32_t stream[RS_STREAM];
    int sub[64][5];
    int nm[64];
    int off[65];
    uint8_t eh[640];
    int cnt[RS_WAVES * RS_SCORE_G];
    int used;
};

__global__ __launch_bounds__(RS_THREADS) __attribute__((amdgpu_waves_per_eu(RS_OCC, RS_OCC))) void k_ransac(PairBuf pb, int kp_cap, RansacParams rp, const uint32_t* rng_tab, int rng_n)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    RansacShared& sh = *(RansacShared*)s_dyn;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = pb.m_count[p];
    const double* x1 = pb.xn1 + (size_t)p * kp_cap * 2;
    const double* x2 = pb.xn2 + (size_t)p * kp_cap * 2;
    uint8_t* mask = pb.mask + (size_t)p * kp_cap;
    vo_pair_result* res = pb.res + p;

    if (M < 5) {
        if (tid == 0) { res->status = VO_ERR_TOO_FEW; res->n_inl = 0; res->ransac_iters = 0; }
        for (int i = tid; i < M; i += RS_THREADS) mask[i] = 0;
        return;
    }
    const double threshold = rp.thresh_px / ((rp.K[0] + rp.K[4]) / 2);
    const float t = (float)(threshold * threshold);

    if (M == 5) {       // ptsetreg.cpp: count == modelPoints -> all solutions, every point an inlier
        if (tid < 4) {                   // one quad
            double* models = pb.models + (size_t)p * 64 * 90;
            const int nm = five_point_solve_quad(x1, x2, models, (lds_double*)sh.park, rp.dk_early != 0);
            __threadfence_block();       // lane 0 reads what the quad stored
            if (tid == 0) {
                for (int k = 0; k < 9; k++) res->E[k] = nm > 0 ? models[k] : 0.0;
                res->status = nm > 0 ? VO_OK : VO_ERR_NO_MODEL;
                res->n_inl = nm > 0 ? 5 : 0;
                res->reserved = nm;      // number of stacked models left in pb.models
                res->ransac_iters = 0;
                for (int k = 0; k < 5; k++) mask[k] = nm > 0 ? 1 : 0;      // no model: no inlier, as for M > 5
            }
        }
        return;
    }

    // every thread carries the same copy of the sequential state
    int niters = rp.max_iters > 1 ? rp.max_iters : 1;
    int max_good = 0, iters_done = 0, pos = 0;
    double bestE[9];
#pragma unroll
    for (int k = 0; k < 9; k++) bestE[k] = 0;

#ifdef VO_EXP_TIMING
    long long tA = clock64(), tB = 0, tC = 0, tD = 0, tE = 0;
#endif
    double* gmodels = pb.models + (size_t)p * 64 * 90;
    for (int r0 = 0; r0 < niters; r0 += RS_ROUND) {
        const int nh = min(RS_ROUND, niters - r0);
        // (1) sample indices.  Subset h starts where subset h - 1 stopped in the RNG stream, and a subset that draws an
        //     index twice uses extra numbers; that happens in well under 1 % of the subsets, so the lanes of wave 0 draw
        //     their subsets in parallel from assumed start positions (5 numbers per earlier subset), a prefix sum of the
        //     numbers actually used gives the true starts, and the lanes repeat until the starts stop moving (one or two
        //     passes; each pass fixes at least the first lane that was wrong, so it ends).
        for (int i = tid; i < RS_STREAM; i += RS_THREADS) sh.stream[i] = pos + i < rng_n ? rng_tab[pos + i] % (uint32_t)M : 0u;
        __syncthreads();
        if (wave == 0) {
            int start = 5 * lane, used = 5;
            for (;;) {
                int idx[5];
                used = 0;
                if (lane < nh) {
#pragma unroll
                    for (int i = 0; i < 5; i++) {
                        int v; bool dup;
                        do {
                            const int at = start + used;
                            if (at < RS_STREAM && pos + at < rng_n) v = (int)sh.stream[at];
                            else {                          // beyond the staged window / table: recompute directly
                                uint64_t st = rp.seed ? rp.seed : 0xffffffffULL;
                                uint32_t x = 0;
                                if (pos + at < rng_n) x = rng_tab[pos + at];
                                else { for (int q = 0; q <= pos + at; q++) x = rng_next(st); }
                                v = (int)(x % (uint32_t)M);
                            }
                            used++;
                            dup = false;
#pragma unroll
                            for (int k = 0; k < 5; k++) dup |= k < i && idx[k] == v;
                        } while (dup);
                        idx[i] = v;
                    }
#pragma unroll
                    for (int i = 0; i < 5; i++) sh.sub[lane][i] = idx[i];
                }
                int inc = used;                              // inclusive prefix of the numbers used
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
                const int true_start = inc - used;
                const bool moved = lane < nh && true_start != start;
                start = true_start;
                if (lane == 63) sh.used = inc;
                if (!__any(moved)) break;
            }
        }
        __syncthreads();
        pos += sh.used;
#ifdef VO_EXP_TIMING
        if (r0 == 0) tB = clock64();
#endif
        // (2) solve: sample h = 16 * wave + lane / 4, by the four lanes of its quad
        if (wave < RS_SOLVERS) {
            const int h = wave * FP_QUADS + (lane >> 2);
            if (h < nh) {
                double s1[10], s2[10];
#pragma unroll
                for (int i = 0; i < 5; i++) {
                    const int v = sh.sub[h][i];
                    s1[2 * i] = x1[2 * v]; s1[2 * i + 1] = x1[2 * v + 1];
                    s2[2 * i] = x2[2 * v]; s2[2 * i + 1] = x2[2 * v + 1];
                }
                const int nm = five_point_solve_quad(s1, s2, gmodels + h * 90, (lds_double*)sh.park + wave * (FP_PARK * FP_QUADS), rp.dk_early != 0);
                if ((lane & 3) == 0) sh.nm[h] = nm;
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int nm = lane < nh ? sh.nm[lane] : 0;
            // exclusive prefix of the model counts + flattened (sample, model) list
            int inc = nm;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { int v = __shfl_up(inc, d, 64); if (lane >= d) inc += v; }
            sh.off[lane] = inc - nm;
            if (lane == 63) sh.off[64] = inc;
            for (int m = 0; m < nm; m++) sh.eh[inc - nm + m] = (uint8_t)lane;
        }
        __syncthreads();
#ifdef VO_EXP_TIMING
        if (r0 == 0) tC = clock64();
#endif
        // (3) score sixteen models per step — four per wave, interleaved in one pass over the correspondences (one load
        //     of a point serves four models, and four independent error chains keep the wave's f64 pipe busy) — then
        //     consume the sixteen counts strictly in OpenCV's order
        const int T = sh.off[64];
        bool done = false;
        int last_h = -1;
        for (int b0 = 0; b0 < T && !done; b0 += RS_WAVES * RS_SCORE_G) {
            {
                double E[RS_SCORE_G][9];
                int ne = 0;
#pragma unroll
                for (int gq = 0; gq < RS_SCORE_G; gq++) {
                    const int e = b0 + gq * RS_WAVES + wave;
                    const int ee = e < T ? e : (b0 + wave < T ? b0 + wave : 0);      // a dummy model keeps the lanes uniform
                    const int h = sh.eh[ee], m = ee - sh.off[h];
#pragma unroll
                    for (int k = 0; k < 9; k++) E[gq][k] = gmodels[h * 90 + m * 9 + k];
                    ne += e < T;
                }
                if (ne > 0) {
                    int good[RS_SCORE_G];
#pragma unroll
                    for (int gq = 0; gq < RS_SCORE_G; gq++) good[gq] = 0;
                    for (int base = 0; base < M; base += 64) {
                        const int i = base + lane;
                        const bool in = i < M;
                        const double u1 = in ? x1[2 * i] : 0.0, v1 = in ? x1[2 * i + 1] : 0.0, u2 = in ? x2[2 * i] : 0.0, v2 = in ? x2[2 * i + 1] : 0.0;
#pragma unroll
                        for (int gq = 0; gq < RS_SCORE_G; gq++)
                            good[gq] += (int)__popcll(__ballot(in && sampson_err(E[gq], u1, v1, u2, v2) <= t));
                    }
                    if (lane == 0) {
#pragma unroll
                        for (int gq = 0; gq < RS_SCORE_G; gq++) sh.cnt[gq * RS_WAVES + wave] = good[gq];
                    }
                }
            }
            __syncthreads();
            for (int q = 0; q < RS_WAVES * RS_SCORE_G; q++) {
                const int e2 = b0 + q;
                if (e2 >= T) break;
                const int h = sh.eh[e2];
                if (h != last_h) {               // `iter < niters` is tested once per sample; all models of a sample
                    if (r0 + h >= niters) { done = true; break; }   // that has started are scored (ptsetreg.cpp)
                    last_h = h;
                    iters_done = r0 + h + 1;
                }
                const int good = sh.cnt[q];
                if (good > max(max_good, 4)) {
                    const int m = e2 - sh.off[h];
#pragma unroll
                    for (int k = 0; k < 9; k++) bestE[k] = gmodels[h * 90 + m * 9 + k];
                    max_good = good;
                    niters = ransac_update_num_iters(rp.prob, (double)(M - good) / M, 5, niters);
                }
            }
            __syncthreads();
        }
        if (!done) iters_done = min(r0 + nh, niters);
        __syncthreads();
#ifdef VO_EXP_TIMING
        if (r0 == 0) tD = clock64();
#endif
    }

    if (max_good > 0) {
        count_inliers(bestE, x1, x2, M, t, tid, RS_THREADS, 0, mask);
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) res->E[k] = bestE[k];
            res->n_inl = max_good; res->status = VO_OK; res->ransac_iters = iters_done; res->reserved = 1;
#ifdef VO_EXP_TIMING
            tE = clock64();
            res->n_kp1 = (int)(tB - tA); res->n_kp2 = (int)(tC - tB); res->n_match = (int)(tD - tC); res->n_good = (int)(tE - tD); res->reserved = iters_done;
#endif
        }
    } else {
        for (int i = tid; i < M; i += RS_THREADS) mask[i] = 0;
        if (tid == 0) { res->n_inl = 0; res->status = VO_ERR_NO_MODEL; res->ransac_iters = iters_done; res->reserved = 0; }
    }
}

void launch_ransac(hipStream_t s, PairBuf pb, int kp_cap, int P, RansacParams rp, const uint32_t* rng_tab, int rng_n)
{
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_ransac, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(RansacShared)); attr = true; }
    hipLaunchKernelGGL(k_ransac, dim3(P), dim3(RS_THREADS), sizeof(RansacShared), s, pb, kp_cap, rp, rng_tab, rng_n);
}

// ------------------------------------------------------------------ triangulation (DLT, 4x4 SVD per point)
__device__ __forceinline__ void triangulate_one(const double* P1, const double* P2, double x1, double y1,
                                                double x2, double y2, double* X)
{
    double A[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        A[0 * 4 + k] = x1 * P1[8 + k] - P1[k];
        A[1 * 4 + k] = y1 * P1[8 + k] - P1[4 + k];
        A[2 * 4 + k] = x2 * P2[8 + k] - P2[k];
        A[3 * 4 + k] = y2 * P2[8 + k] - P2[4 + k];
    }
    solve_z<4>(A, X);
}

__global__ void k_triangulate_raw(const double* P1g, const double* P2g, const double* x1, const double* x2,
                                  int M, double* X)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double P1[12], P2[12], q[4];
#pragma unroll
    for (int k = 0; k < 12; k++) { P1[k] = P1g[k]; P2[k] = P2g[k]; }
    triangulate_one(P1, P2, x1[i], x1[M + i], x2[i], x2[M + i], q);
#pragma unroll
    for (int k = 0; k < 4; k++) X[(size_t)k * M + i] = q[k];
}

void launch_triangulate_raw(hipStream_t s, const double* P1, const double* P2, const double* x1, const double* x2,
                            int M, double* X)
{
    if (M <= 0) return;
    hipLaunchKernelGGL(k_triangulate_raw, dim3((M + 63) / 64), dim3(64), 0, s, P1, P2, x1, x2, M, X);
}

// image_pair.py:316-339: P = K [R^T | -R^T t] with frame-1 points, P0 = K [I | 0] with frame-2 points, X /= w
__global__ void k_triangulate_pairs(PairBuf pb, int kp_cap, RansacParams rp)
{
    const int p = blockIdx.y;
    const vo_pair_result* res = pb.res + p;
    if (res->status != VO_OK) return;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= res->n_inl) return;
    const double* R = res->R; const double* t = res->t; const double* K = rp.K;
    double T[12], P[12], P0[12];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T[r * 4 + c] = R[c * 3 + r];
        T[r * 4 + 3] = -(R[0 * 3 + r] * t[0] + R[1 * 3 + r] * t[1] + R[2 * 3 + r] * t[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            P[r * 4 + c] = K[r * 3] * T[c] + K[r * 3 + 1] * T[4 + c] + K[r * 3 + 2] * T[8 + c];
            P0[r * 4 + c] = c < 3 ? K[r * 3 + c] : 0.0;
        }
    const double* a = pb.ipx1 + ((size_t)p * kp_cap + i) * 2;
    const double* b = pb.ipx2 + ((size_t)p * kp_cap + i) * 2;
    double q[4];
    triangulate_one(P, P0, a[0], a[1], b[0], b[1], q);
    double* X = pb.X + (size_t)p * 4 * kp_cap;
    double w = q[3];
#pragma unroll
    for (int k = 0; k < 4; k++) X[(size_t)k * kp_cap + i] = q[k] / w;
}

void launch_triangulate_pairs(hipStream_t s, PairBuf pb, int kp_cap, int P, RansacParams rp)
{
    hipLaunchKernelGGL(k_triangulate_pairs, dim3((kp_cap + 63) / 64, P), dim3(64), 0, s, pb, kp_cap, rp);
}

// ------------------------------------------------------------------ decomposeEssentialMat + recoverPose, one wave per pair
__device__ __forceinline__ double det3(const double* m)
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

__device__ __forceinline__ void mat3mul(const double* a, const double* b, double* r)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += a[i * 3 + k] * b[k * 3 + j];
            r[i * 3 + j] = s;
        }
}

__device__ void decompose_essential(const double* E, double* R1, double* R2, double* t)
{
    double At[9], W[3], Vt[9], U[9], u[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) At[i * 3 + k] = E[k * 3 + i];
    jacobi_svd<3, 3>(At, W, Vt);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        double s = W[i] > DBL_MIN ? 1. / W[i] : 0.;
#pragma unroll
        for (int k = 0; k < 3; k++) u[i][k] = At[i * 3 + k] * s;
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) U[k * 3 + i] = u[i][k];
    if (det3(U) < 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) U[k] = -U[k];
    }
    if (det3(Vt) < 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) Vt[k] = -Vt[k];
    }
    const double Wm[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    double T[9];
    mat3mul(U, Wm, T); mat3mul(T, Vt, R1);
    mat3mul(U, Wt, T); mat3mul(T, Vt, R2);
    t[0] = U[2]; t[1] = U[5]; t[2] = U[8];
}

// The E-RANSAC inliers are compacted in order (determine_essential_matrix returns them as a list,
// image_pair.py:288-290), then the four (R, t) candidates are cheirality-tested on them: one workgroup per
// pair, every thread triangulates its share of the points (4x4 Jacobi SVD per point and candidate), the
// per-candidate counts are wavefront ballots + popcounts summed through LDS.
// recoverPose's test of one point for the candidates (R, t) [pos] and (R, -t) [neg] from ONE triangulation.  With P0 = [I | 0]
// the DLT matrix of (R, -t) is the matrix of (R, t) with its fourth column negated; the one-sided Jacobi SVD (jacobi_svd above)
// is sign-symmetric — a negated column only negates dot products, rotation sines / cosines and rows, never a magnitude — so
// its null vector for (R, -t) is +-(Q0, Q1, Q2, -Q3) with the same bits, and so are the quotients and the depth sum below
// (z' = -z exactly: every term changes sign).  An overall sign of Q cancels in every test.
__device__ __forceinline__ void cheirality2(const double* P0, const double* P, const double* a, const double* b, double dist, bool& pos, bool& neg)
{
    double Q[4];
    triangulate_one(P0, P, a[0], a[1], b[0], b[1], Q);
    const double w = Q[2] * Q[3];
    const double q0 = Q[0] / Q[3], q1 = Q[1] / Q[3], q2 = Q[2] / Q[3], q3 = Q[3] / Q[3];
    const double z = P[8] * q0 + P[9] * q1 + P[10] * q2 + P[11] * q3;
    pos = w > 0 && q2 < dist && z > 0 && z < dist;
    neg = w < 0 && -q2 < dist && -z > 0 && -z < dist;
}

// recoverPose in three launches, none with a workgroup over 256 threads (a 1024-thread workgroup at 128 registers is the
// register file of a whole CU and waits for an empty one):
//  k_pose_prepare  one workgroup per pair: the in-order inlier compaction and decomposeEssentialMat (one wavefront) -> pb.pose_state
//  k_pose          (pair, block of 256 inliers, rotation): one triangulation per thread serves both signs of t; wavefront
//                  ballots, one integer atomicAdd per wave and candidate into the pair's four counts (bound by the
//                  dependent-issue latency of the f64 Jacobi sweeps, so it wants many independent waves, not large groups)
//  k_pose_finish   the best of the four counts in recoverPose's tie order -> R, t, n_good, n_inl (+ the single-call mask)
__global__ __launch_bounds__(256) void k_pose_prepare(PairBuf pb, int kp_cap)
{
    __shared__ int s_w[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    vo_pair_result* res = pb.res + p;
    PoseState* ps = pb.pose_state + p;
    if (res->status != VO_OK) {
        if (tid == 0) { res->n_good = 0; ps->active = 0; }
        return;
    }
    if (res->reserved != 1) {           // M == 5: stacked solutions; decomposeEssentialMat needs a single 3x3 matrix
        __syncthreads();                // every thread has read the status before it changes
        if (tid == 0) { res->status = VO_ERR_AMBIGUOUS; res->n_good = 0; ps->active = 0; }
        return;
    }
    const int M = pb.m_count[p];
    const size_t base2 = (size_t)p * kp_cap * 2;
    const uint8_t* mask = pb.mask + (size_t)p * kp_cap;
    double* in1 = pb.in1 + base2; double* in2 = pb.in2 + base2;
    double* ip1 = pb.ipx1 + base2; double* ip2 = pb.ipx2 + base2;
    int ninl = 0;
    for (int b = 0; b < M; b += 256) {
        const int i = b + tid;
        const bool f = i < M && mask[i] != 0;
        const unsigned long long bal = __ballot(f);
        __syncthreads();
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { const int c = s_w[w]; if (w < wave) off += c; tot += c; }
        if (f) {
            const int pos = ninl + off + __popcll(bal & ((1ULL << lane) - 1));
            in1[2 * pos] = pb.xn1[base2 + 2 * i]; in1[2 * pos + 1] = pb.xn1[base2 + 2 * i + 1];
            in2[2 * pos] = pb.xn2[base2 + 2 * i]; in2[2 * pos + 1] = pb.xn2[base2 + 2 * i + 1];
            ip1[2 * pos] = pb.px1[base2 + 2 * i]; ip1[2 * pos + 1] = pb.px1[base2 + 2 * i + 1];
            ip2[2 * pos] = pb.px2[base2 + 2 * i]; ip2[2 * pos + 1] = pb.px2[base2 + 2 * i + 1];
        }
        ninl += tot;
    }
    if (tid < 64) {                     // decomposeEssentialMat once, by the first wavefront
        double E[9], R1[9], R2[9], tt[3];
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = res->E[k];
        decompose_essential(E, R1, R2, tt);
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) { ps->R1[k] = R1[k]; ps->R2[k] = R2[k]; }
#pragma unroll
            for (int k = 0; k < 3; k++) ps->t[k] = tt[k];
#pragma unroll
            for (int k = 0; k < 4; k++) ps->good[k] = 0;
            ps->ninl = ninl; ps->active = 1;
        }
    }
}

// P = [R | t] of candidate rotation c (R1 / R2) from the pair's record
__device__ __forceinline__ void pose_candidate(const PoseState* ps, int c, double* P)
{
    const double* Rc = c ? ps->R2 : ps->R1;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) P[r * 4 + k] = Rc[r * 3 + k];
        P[r * 4 + 3] = ps->t[r];
    }
}

__global__ __launch_bounds__(256) void k_pose(PairBuf pb, int kp_cap, RansacParams rp)
{
    const int p = blockIdx.x, blk = blockIdx.y, c = blockIdx.z, lane = threadIdx.x & 63;      // candidates c (R, t) and c + 2 (R, -t), R = R1 / R2
    PoseState* ps = pb.pose_state + p;
    if (!ps->active) return;
    const int ninl = ps->ninl, i = blk * 256 + threadIdx.x;
    if (blk * 256 >= ninl) return;
    const size_t base2 = (size_t)p * kp_cap * 2;
    const double* in1 = pb.in1 + base2; const double* in2 = pb.in2 + base2;
    const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double P[12];
    pose_candidate(ps, c, P);
    bool mp = false, mn = false;
    if (i < ninl) cheirality2(P0, P, in1 + 2 * i, in2 + 2 * i, rp.dist_thresh, mp, mn);
    const int gp = __popcll(__ballot(mp)), gn = __popcll(__ballot(mn));
    if (lane == 0 && gp) atomicAdd(&ps->good[c], gp);
    if (lane == 0 && gn) atomicAdd(&ps->good[c + 2], gn);
}

// 64 threads per pair; 256 where the single-call mask is wanted (the winning candidate's test again)
__global__ __launch_bounds__(256) void k_pose_finish(PairBuf pb, int kp_cap, RansacParams rp)
{
    const int p = blockIdx.x;
    const PoseState* ps = pb.pose_state + p;
    if (!ps->active) return;
    vo_pair_result* res = pb.res + p;
    const int ninl = ps->ninl;
    const int g0 = ps->good[0], g1 = ps->good[1], g2 = ps->good[2], g3 = ps->good[3];
    int best;
    if (g0 >= g1 && g0 >= g2 && g0 >= g3) best = 0;
    else if (g1 >= g0 && g1 >= g2 && g1 >= g3) best = 1;
    else if (g2 >= g0 && g2 >= g1 && g2 >= g3) best = 2;
    else best = 3;
    if (pb.pose_mask) {      // single-call cv2.recoverPose mask
        const size_t base2 = (size_t)p * kp_cap * 2;
        const double* in1 = pb.in1 + base2; const double* in2 = pb.in2 + base2;
        const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        double P[12];
        pose_candidate(ps, best & 1, P);
        uint8_t* pm = pb.pose_mask + (size_t)p * kp_cap;
        for (int i = threadIdx.x; i < ninl; i += blockDim.x) {
            bool mp, mn;
            cheirality2(P0, P, in1 + 2 * i, in2 + 2 * i, rp.dist_thresh, mp, mn);
            pm[i] = (best >= 2 ? mn : mp) ? 255 : 0;
        }
    }
    if (threadIdx.x == 0) {
        const double* Rb = (best & 1) ? ps->R2 : ps->R1;
#pragma unroll
        for (int k = 0; k < 9; k++) res->R[k] = Rb[k];
#pragma unroll
        for (int k = 0; k < 3; k++) res->t[k] = best >= 2 ? -ps->t[k] : ps->t[k];
        res->n_good = best == 0 ? g0 : best == 1 ? g1 : best == 2 ? g2 : g3;
        res->n_inl = ninl;
    }
}

void launch_pose(hipStream_t s, PairBuf pb, int kp_cap, int P, RansacParams rp)
{
    hipLaunchKernelGGL(k_pose_prepare, dim3(P), dim3(256), 0, s, pb, kp_cap);
    hipLaunchKernelGGL(k_pose, dim3(P, (kp_cap + 255) / 256, 2), dim3(256), 0, s, pb, kp_cap, rp);
    hipLaunchKernelGGL(k_pose_finish, dim3(P), dim3(pb.pose_mask ? 256 : 64), 0, s, pb, kp_cap, rp);
}

// ------------------------------------------------------------------ single five-point sample (stage test)
__global__ __launch_bounds__(64) void k_five_point_raw(const double* x1, const double* x2, double* E, int* nm, int dk_early)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    if (threadIdx.x < 4 && blockIdx.x == 0) {       // one quad
        const int n = five_point_solve_quad(x1, x2, E, (lds_double*)s_dyn, dk_early != 0);
        if (threadIdx.x == 0) *nm = n;
    }
}

void launch_five_point_raw(hipStream_t s, const double* x1, const double* x2, double* E, int* nm, int dk_early)
{
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_five_point_raw, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FP_PARK * FP_QUADS * sizeof(double))); attr = true; }
    hipLaunchKernelGGL(k_five_point_raw, dim3(1), dim3(64), FP_PARK * FP_QUADS * sizeof(double), s, x1, x2, E, nm, dk_early);
}

// ------------------------------------------------------------------ reprojection-error filter
// src/map.py:46-94: project every observation's map point with its camera pose and K, squared pixel error,
// keep iff below the threshold.  One lane per observation; poses / points are gathered through L2.
__global__ void k_reprojection(const double* poses, int ncam, const double* points, int npt, const int* obs_cam,
                               const int* obs_pt, const double* obs_xy, int nobs, const double* Kd, double threshold,
                               double* sqerr, uint8_t* keep, int* bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nobs) return;
    const int ci = obs_cam[i], pi = obs_pt[i];
    if (ci < 0 || ci >= ncam || pi < 0 || pi >= npt) { atomicOr(bad, 1); sqerr[i] = 0; keep[i] = 0; return; }
    const double e = reprojection_sqerr_one(poses + 16 * (size_t)ci, points + 3 * (size_t)pi, Kd, obs_xy[2 * i], obs_xy[2 * i + 1]);
    sqerr[i] = e;
    keep[i] = e < threshold ? 1 : 0;
}

void launch_reprojection(hipStream_t s, const double* poses, int ncam, const double* points, int npt, const int* obs_cam,
                         const int* obs_pt, const double* obs_xy, int nobs, const double* Kd, double threshold,
                         double* sqerr, uint8_t* keep, int* bad)
{
    if (nobs <= 0) return;
    hipLaunchKernelGGL(k_reprojection, dim3((nobs + 255) / 256), dim3(256), 0, s, poses, ncam, points, npt, obs_cam, obs_pt,
                       obs_xy, nobs, Kd, threshold, sqerr, keep, bad);
}

// ------------------------------------------------------------------ feature-track bookkeeping
// src/visual_slam.py:183-188 (update_feature_mapper: feature_mapper[featureid2] = featureid1 for every match of the
// current pair, later pairs overwrite earlier ones) and :94-99 (track_feature_back_in_time: follow the chain to its
// first feature).  Feature ids are (frame, index); the dict becomes a [F][cap] table of packed parents.
__global__ void k_track_link(const int* pair_frames, const int* match_off, const int* mq, const int* mt, int P, int cap,
                             unsigned long long* parent)
{
    const int p = blockIdx.y;
    const int n = match_off[p + 1] - match_off[p];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f1 = pair_frames[2 * p], f2 = pair_frames[2 * p + 1];
    const int q = mq[match_off[p] + i], t = mt[match_off[p] + i];
    // key (pair + 1) in the high bits: an atomic max keeps the LAST pair's entry, as the dict assignment order does
    const unsigned long long v = ((unsigned long long)(p + 1) << 40) | ((unsigned long long)(unsigned)f1 << 20) | (unsigned)q;
    atomicMax(&parent[(size_t)f2 * cap + t], v);
}

__global__ void k_track_roots(const unsigned long long* parent, int F, int cap, int* root_frame, int* root_idx, int* hops, int* bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= cap) return;
    int cf = f, ci = i, n = 0;
    for (;;) {
        const unsigned long long v = parent[(size_t)cf * cap + ci];
        if (v == 0) break;
        cf = (int)((v >> 20) & 0xfffffu); ci = (int)(v & 0xfffffu);
        if (++n > F) { atomicOr(bad, 1); break; }       // a cycle: the reference's while-loop would never end
    }
    root_frame[(size_t)f * cap + i] = cf; root_idx[(size_t)f * cap + i] = ci; hops[(size_t)f * cap + i] = n;
}

void launch_tracks(hipStream_t s, const int* pair_frames, const int* match_off, const int* mq, const int* mt, int P, int max_m,
                   int F, int cap, unsigned long long* parent, int* root_frame, int* root_idx, int* hops, int* bad)
{
    if (P > 0 && max_m > 0)
        hipLaunchKernelGGL(k_track_link, dim3((max_m + 255) / 256, P), dim3(256), 0, s, pair_frames, match_off, mq, mt, P, cap, parent);
    hipLaunchKernelGGL(k_track_roots, dim3((cap + 255) / 256, F), dim3(256), 0, s, parent, F, cap, root_frame, root_idx, hops, bad);
}


// ------------------------------------------------------------------ the localisation chain on resident pair results
// VisualSlam's steady state (src/visual_slam.py:183-266, 153-180) for the pairs vo_pairs_run left in HBM, in their order,
// without a host round trip and without the bundle adjustment (src/map.py:104-186; vo_slam_chain runs it after every pair, slam_kernels.hip):
//   update_feature_mapper (:183-188)            -> k_chain_link, all pairs at once (a feature id is a key of one pair only)
//   initialize_map (:43-92)                     -> k_chain_init: cameras of pair 0, one map point per inlier keyed by featureid1
//   estimate_current_camera_position (:190-235) -> k_chain_gather: matches whose track root is in the map -> (map, image) coordinates
//                                                  k_pnp_ransac on them (pnp_kernels.hip), k_chain_pose: Rodrigues, the camera
//   add_information_to_map (:153-180)           -> k_chain_triangulate with K pose(frame2), K pose(frame1); k_chain_insert:
//                                                  points beyond 50 units dropped, a point whose root is unmapped is added under
//                                                  featureid1 (as add_new_match_to_map does)
__global__ void k_chain_link(PairBuf pb, int kp_cap, ChainBuf cb)
{
    const int p = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (pb.res[p].status != VO_OK || i >= pb.m_count[p] || !pb.mask[(size_t)p * kp_cap + i]) return;
    const int f1 = pb.slots[2 * p], f2 = pb.slots[2 * p + 1];
    const int q = pb.m_q[(size_t)p * kp_cap + i], t = pb.m_t[(size_t)p * kp_cap + i];
    const unsigned long long v = ((unsigned long long)(p + 1) << 40) | ((unsigned long long)(unsigned)f1 << 20) | (unsigned)q;
    atomicMax(&cb.parent[chain_key(f2, t, kp_cap)], v);
}

void launch_chain_link(hipStream_t s, PairBuf pb, int kp_cap, int P, ChainBuf cb)
{
    hipLaunchKernelGGL(k_chain_link, dim3((kp_cap + 255) / 256, P), dim3(256), 0, s, pb, kp_cap, cb);
}

// (chain_init_wg: chain_common.h — k_slam_restart_seqs starts a new map with it)
__global__ __launch_bounds__(256) void k_chain_init(PairBuf pb, int kp_cap, ChainBuf cb) { chain_init_wg(pb, kp_cap, cb); }

// vo_slam_chains: workgroup = sequence (blockIdx.x); the sequence's pair 0 is pair `first` of the run
__global__ __launch_bounds__(256) void k_chain_init_seqs(PairBuf pb, int kp_cap, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    chain_init_wg(chain_pairs_from(pb, q.first, kp_cap), kp_cap, q.cb);
}

void launch_chain_init_seqs(hipStream_t s, PairBuf pb, int kp_cap, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_chain_init_seqs, dim3(S), dim3(256), 0, s, pb, kp_cap, seqs);
}

void launch_chain_init(hipStream_t s, PairBuf pb, int kp_cap, ChainBuf cb)
{
    hipLaunchKernelGGL(k_chain_init, dim3(1), dim3(256), 0, s, pb, kp_cap, cb);
}

// matches_with_map (:201-218): for every match with 3-D information of the current pair, in order — trace featureid2 back, keep
// the match if the root feature owns a map point: (imagecoord = keypoint2, mapcoord = the point)
__device__ __forceinline__ void chain_gather_wg(PairBuf pb, int kp_cap, int p, int F, ChainBuf cb)
{
    __shared__ int s_w[4];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const vo_pair_result& r = pb.res[p];
    const int f1 = pb.slots[2 * p], f2 = pb.slots[2 * p + 1];
    if (cb.rs.st) {
        // vo_slam_chains_restart: a failed pair keeps its status and leaves the sequence lost (the first such status is the cause
        // the next segment reports); a lost sequence that meets a good pair starts a new map from it — no PnP, an initial step
        const bool lost = !cb.alive[0];
        if (r.status != VO_OK || lost) {
            if (tid == 0) {
                cb.off[0] = cb.obj0; cb.off[1] = cb.obj0; cb.n_corr[p] = 0;
                if (r.status != VO_OK) {
                    cb.status[p] = r.status; cb.alive[0] = 0; cb.rs.st[SEG_INIT] = 0;
                    if (cb.rs.st[SEG_CAUSE] == 0) cb.rs.st[SEG_CAUSE] = r.status;
                } else cb.rs.st[SEG_INIT] = 1;
            }
            return;
        }
        if (tid == 0) cb.rs.st[SEG_INIT] = 0;
    }
    const bool ok = cb.alive[0] && r.status == VO_OK && cb.cam_ok[f1];
    if (!ok) {
        if (tid == 0) {
            cb.off[0] = cb.obj0; cb.off[1] = cb.obj0; cb.n_corr[p] = 0;
            cb.status[p] = !cb.alive[0] ? VO_ERR_NOT_CONFIGURED : r.status != VO_OK ? r.status : VO_ERR_INVALID;   // the chain broke earlier / this pair failed / no camera for frame 1
            cb.alive[0] = 0;
            if (cb.rs.st && cb.rs.st[SEG_CAUSE] == 0) cb.rs.st[SEG_CAUSE] = cb.status[p];
        }
        return;
    }
    if (tid == 0) s_base = 0;
    const int M = pb.m_count[p];
    const uint8_t* mask = pb.mask + (size_t)p * kp_cap;
    const double* px2 = pb.px2 + (size_t)p * kp_cap * 2;
    for (int b = 0; b < M; b += 256) {
        const int i = b + tid;
        bool take = false; size_t key = 0;
        if (i < M && mask[i]) {
            int rf = f2, ri = pb.m_t[(size_t)p * kp_cap + i];
            chain_root(cb.parent, kp_cap, F, rf, ri);
            key = chain_key(rf, ri, kp_cap);
            take = cb.in_map[key] != 0;
        }
        const unsigned long long bal = __ballot(take);
        __syncthreads();
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < 4; w++) { const int c = s_w[w]; if (w < wave) off += c; tot += c; }
        if (take) {
            const int pos = s_base + off + (int)__popcll(bal & ((1ULL << lane) - 1));
            for (int d = 0; d < 3; d++) cb.obj[3 * pos + d] = cb.map_pt[3 * key + d];
            cb.img[2 * pos] = px2[2 * i]; cb.img[2 * pos + 1] = px2[2 * i + 1];
        }
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    if (tid == 0) { cb.off[0] = cb.obj0; cb.off[1] = cb.obj0 + s_base; cb.n_corr[p] = s_base; }
}

__global__ __launch_bounds__(256) void k_chain_gather(PairBuf pb, int kp_cap, int p, int F, ChainBuf cb) { chain_gather_wg(pb, kp_cap, p, F, cb); }

// vo_slam_chains, step j: workgroup = sequence (blockIdx.x).  A sequence that has ended hands k_pnp_ransac an empty problem.
__global__ __launch_bounds__(256) void k_chain_gather_seqs(PairBuf pb, int kp_cap, int j, int F, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) {
        if (threadIdx.x == 0) { q.cb.off[0] = q.cb.obj0; q.cb.off[1] = q.cb.obj0; }
        return;
    }
    chain_gather_wg(chain_pairs_from(pb, q.first, kp_cap), kp_cap, j, F, q.cb);
}

void launch_chain_gather_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, int F, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_chain_gather_seqs, dim3(S), dim3(256), 0, s, pb, kp_cap, j, F, seqs);
}

void launch_chain_gather(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, ChainBuf cb)
{
    hipLaunchKernelGGL(k_chain_gather, dim3(1), dim3(256), 0, s, pb, kp_cap, p, F, cb);
}

// add_information_to_map's reconstruct_3d_points(essential_matches, pose(frame2)[0:3], pose(frame1)[0:3]) (:164-172):
// cv2.triangulatePoints(K pose(frame1), K pose(frame2), pts1, pts2), X /= w, for every E inlier of the pair
__device__ __forceinline__ void chain_triangulate_one(PairBuf pb, int kp_cap, int p, ChainBuf cb)
{
    if (!cb.alive[0] || (cb.rs.st && cb.rs.st[SEG_INIT])) return;   // (an initial step takes pair 0's points, not these)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;    // keypoint tiles on x, in both kernels
    if (i >= pb.res[p].n_inl) return;
    double P1[12], P2[12], q[4];
    for (int k = 0; k < 12; k++) { P1[k] = cb.P1[k]; P2[k] = cb.P2[k]; }
    const double* a = pb.ipx1 + ((size_t)p * kp_cap + i) * 2;
    const double* b = pb.ipx2 + ((size_t)p * kp_cap + i) * 2;
    triangulate_one(P1, P2, a[0], a[1], b[0], b[1], q);
    const double w = q[3];
    for (int k = 0; k < 4; k++) cb.Xw[4 * (size_t)i + k] = q[k] / w;
}

__global__ void k_chain_triangulate(PairBuf pb, int kp_cap, int p, ChainBuf cb) { chain_triangulate_one(pb, kp_cap, p, cb); }

// vo_slam_chains, step j: the keypoint tiles stay on x, the sequence is blockIdx.y
__global__ void k_chain_triangulate_seqs(PairBuf pb, int kp_cap, int j, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.y];
    if (j >= q.count) return;
    chain_triangulate_one(chain_pairs_from(pb, q.first, kp_cap), kp_cap, j, q.cb);
}

void launch_chain_triangulate_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_chain_triangulate_seqs, dim3((kp_cap + 63) / 64, S), dim3(64), 0, s, pb, kp_cap, j, seqs);
}

void launch_chain_triangulate(hipStream_t s, PairBuf pb, int kp_cap, int p, ChainBuf cb)
{
    hipLaunchKernelGGL(k_chain_triangulate, dim3((kp_cap + 63) / 64), dim3(64), 0, s, pb, kp_cap, p, cb);
}

// the loop of :174-178 with add_point_observation_to_map (:138-151): skip points farther than max_norm; a match whose track root
// already owns a map point only adds an observation (nothing to store without BA); otherwise a new point under featureid1.
// Pass 1 takes every decision against the map as it was before the loop (self.mappointdict is built at :154-156, before it) and
// stores it in dec[match index]; pass 2 writes, after a barrier — as slam_add_wg does.  With nearest or ratio matches two queries
// q < q' may share a train row whose track root is the unmapped (f1, q'): both get a point, whichever wave runs first.
__global__ __launch_bounds__(256) void k_chain_insert(PairBuf pb, int kp_cap, int p, int F, double max_norm, ChainBuf cb, uint8_t* dec)
{
    __shared__ int s_w[4];
    __shared__ int s_added;
    if (!cb.alive[0]) { if (threadIdx.x == 0) cb.n_map[p] = cb.map_count[0]; return; }
    const int f1 = pb.slots[2 * p], f2 = pb.slots[2 * p + 1];
    if (threadIdx.x == 0) s_added = 0;
    chain_for_each_inlier(pb, kp_cap, p, s_w, [&](bool f, int i, int pos) {
        if (!f) return;
        const double x = cb.Xw[4 * (size_t)pos], y = cb.Xw[4 * (size_t)pos + 1], z = cb.Xw[4 * (size_t)pos + 2];
        bool add = sqrt(x * x + y * y + z * z) <= max_norm;                      // np.linalg.norm(match.point) > 50: continue (NaN: kept out)
        if (add) {
            int rf = f2, ri = pb.m_t[(size_t)p * kp_cap + i];
            chain_root(cb.parent, kp_cap, F, rf, ri);
            add = !cb.in_map[chain_key(rf, ri, kp_cap)];                         // mapped: add_new_observation_of_existing_point
        }
        dec[i] = add;
    });
    __syncthreads();
    int added = 0;
    chain_for_each_inlier(pb, kp_cap, p, s_w, [&](bool f, int i, int pos) {
        if (!f || !dec[i]) return;
        const size_t k = chain_key(f1, pb.m_q[(size_t)p * kp_cap + i], kp_cap);  // add_new_match_to_map: keyed by featureid1
        cb.in_map[k] = 1;
        for (int d = 0; d < 3; d++) cb.map_pt[3 * k + d] = cb.Xw[4 * (size_t)pos + d];
        added++;
    });
    __syncthreads();
    atomicAdd(&s_added, added);
    __syncthreads();
    if (threadIdx.x == 0) { cb.map_count[0] += s_added; cb.n_map[p] = cb.map_count[0]; }
}

void launch_chain_insert(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, ChainBuf cb, uint8_t* dec)
{
    hipLaunchKernelGGL(k_chain_insert, dim3(1), dim3(256), 0, s, pb, kp_cap, p, F, max_norm, cb, dec);
}

// ------------------------------------------------------------------ computeCorrespondEpilines and the epipolar distances
// cv2.computeCorrespondEpilines(points, whichImage, F) (src/feature_detection.py:118-125), restated from OpenCV 4.7's
// fundam.cpp; parity with a cv2 build is unpinned, like the rest of the project.  f[] is F for whichImage 1 and F^T for 2 (the
// caller transposes).  All arithmetic is f64, left to right, one rounding per operation (-ffp-contract=off):
//   a = f0 x + f1 y + f2, b = f3 x + f4 y + f5, c = f6 x + f7 y + f8;  nu = a a + b b;  nu = nu ? 1 / sqrt(nu) : 1;  (a, b, c) *= nu
__device__ __forceinline__ void epiline_one(const double* f, double x, double y, double* l)
{
    const double a = f[0] * x + f[1] * y + f[2];
    const double b = f[3] * x + f[4] * y + f[5];
    const double c = f[6] * x + f[7] * y + f[8];
    double nu = a * a + b * b;
    nu = nu != 0.0 ? 1.0 / sqrt(nu) : 1.0;
    l[0] = a * nu; l[1] = b * nu; l[2] = c * nu;
}

// One lane per point.  point_type 0: f64 points, f64 lines; 1: f32 points, 2: i32 points, both f32 lines (cv2's output depth is
// max(input depth, f32)), every value cast once at the end.
__global__ void k_epilines(const void* pts, int point_type, int N, const double* Fg, void* lines)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double f[9], l[3], x, y;
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = Fg[k];
    if (point_type == 0)      { x = ((const double*)pts)[2 * (size_t)i]; y = ((const double*)pts)[2 * (size_t)i + 1]; }
    else if (point_type == 1) { x = (double)((const float*)pts)[2 * (size_t)i]; y = (double)((const float*)pts)[2 * (size_t)i + 1]; }
    else                      { x = (double)((const int32_t*)pts)[2 * (size_t)i]; y = (double)((const int32_t*)pts)[2 * (size_t)i + 1]; }
    epiline_one(f, x, y, l);
    if (point_type == 0) {
        double* o = (double*)lines + 3 * (size_t)i;
        o[0] = l[0]; o[1] = l[1]; o[2] = l[2];
    } else {
        float* o = (float*)lines + 3 * (size_t)i;
        o[0] = (float)l[0]; o[1] = (float)l[1]; o[2] = (float)l[2];
    }
}

void launch_epilines(hipStream_t s, const void* pts, int point_type, int N, const double* F, void* lines)
{
    if (N <= 0) return;
    hipLaunchKernelGGL(k_epilines, dim3((N + 63) / 64), dim3(64), 0, s, pts, point_type, N, F, lines);
}

// The symmetric epipolar distance of every E inlier of a resident pair and its statistics (src/feature_detection.py:127-140), one
// workgroup per pair.  F = K^-T E K^-1 with K^-1 as the pair path normalises pixels (k_match_select, k_prepare_points):
//   ifx = 1 / K[0], ify = 1 / K[4], bx = -K[2] ifx, by = -K[5] ify,  K^-1 = [ifx 0 bx; 0 ify by; 0 0 1]
//   G = E K^-1:  G[r][0] = E[r][0] ifx, G[r][1] = E[r][1] ify, G[r][2] = E[r][0] bx + E[r][1] by + E[r][2]
//   F = K^-T G:  F[0][c] = ifx G[0][c], F[1][c] = ify G[1][c], F[2][c] = bx G[0][c] + by G[1][c] + G[2][c]
// d_k = |l1 . (x2, 1)| + |l2 . (x1, 1)|, l1 = epiline of x1 under F, l2 = epiline of x2 under F^T, each dot as l0 x + l1 y + l2.
// mean, the population standard deviation (two passes, as np.std) and the maximum are SEQUENTIAL sums in match order from 0.0
// (k_slam_stats' rule for total_sqerr), made by one lane: the bytes are defined by the data, not by a reduction tree.
__device__ __forceinline__ void pixel_fundamental(const double* E, const double* K, double* F)
{
    const double ifx = 1. / K[0], ify = 1. / K[4];
    const double bx = -K[2] * ifx, by = -K[5] * ify;
    double G[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        G[3 * r] = E[3 * r] * ifx; G[3 * r + 1] = E[3 * r + 1] * ify;
        G[3 * r + 2] = E[3 * r] * bx + E[3 * r + 1] * by + E[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        F[c] = ifx * G[c]; F[3 + c] = ify * G[3 + c];
        F[6 + c] = bx * G[c] + by * G[3 + c] + G[6 + c];
    }
}

__global__ __launch_bounds__(256) void k_pairs_epipolar(PairBuf pb, int kp_cap, const double* Kd, double* dist, int* n_out, double* mean_out,
                                                        double* std_out, double* max_out)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    const vo_pair_result* res = pb.res + p;
    int n = res->status == VO_OK ? res->n_inl : 0;
    n = n < 0 ? 0 : (n > kp_cap ? kp_cap : n);
    double* d = dist + (size_t)p * kp_cap;
    if (n > 0) {
        double K[9], E[9], F[9], Ft[9];
#pragma unroll
        for (int k = 0; k < 9; k++) { K[k] = Kd[k]; E[k] = res->E[k]; }
        pixel_fundamental(E, K, F);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) Ft[3 * r + c] = F[3 * c + r];
        const double* a = pb.ipx1 + (size_t)p * kp_cap * 2;
        const double* b = pb.ipx2 + (size_t)p * kp_cap * 2;
        for (int k = tid; k < n; k += 256) {
            const double x1 = a[2 * k], y1 = a[2 * k + 1], x2 = b[2 * k], y2 = b[2 * k + 1];
            double l1[3], l2[3];
            epiline_one(F, x1, y1, l1);
            epiline_one(Ft, x2, y2, l2);
            d[k] = fabs(l1[0] * x2 + l1[1] * y2 + l1[2]) + fabs(l2[0] * x1 + l2[1] * y1 + l2[2]);
        }
    }
    for (int k = n + tid; k < kp_cap; k += 256) d[k] = 0.0;
    __syncthreads();                    // the workgroup's own global writes, read back by its lane 0
    if (tid != 0) return;
    double mean = 0.0, sd = 0.0, mx = 0.0;
    if (n > 0) {
        double sum = 0.0;
        for (int k = 0; k < n; k++) { const double v = d[k]; sum += v; mx = v > mx ? v : mx; }
        mean = sum / (double)n;
        double sq = 0.0;
        for (int k = 0; k < n; k++) { const double e = d[k] - mean; sq += e * e; }
        sd = sqrt(sq / (double)n);
    }
    n_out[p] = n; mean_out[p] = mean; std_out[p] = sd; max_out[p] = mx;
}

void launch_pairs_epipolar(hipStream_t s, PairBuf pb, int kp_cap, int P, const double* Kd, double* dist, int* n, double* mean, double* sd, double* mx)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(k_pairs_epipolar, dim3(P), dim3(256), 0, s, pb, kp_cap, Kd, dist, n, mean, sd, mx);
}
