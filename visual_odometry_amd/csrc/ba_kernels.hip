// ba_kernels.hip — Map.optimize_map (src/map.py:104-186): the g2o bundle adjustment the reference runs after every frame,
// restated for maps of its size.  g2o itself is not vendored; what follows restates, from its 2020 sources as recalled,
// what the reference configures: VertexSE3Expmap / VertexPointXYZ / EdgeProjectXYZ2UV with one focal length, information I,
// RobustKernelHuber, OptimizationAlgorithmLevenberg over BlockSolverSE3 (Schur complement on the points).  Parity with a g2o
// build is unpinned; the checker is tests/ba_reference.py.
//
// One workgroup of 256 lanes per map, the whole Levenberg-Marquardt loop inside the kernel; only __syncthreads().
//   per point  (a lane owns a point, observations sorted by point on the host): H_pp, b_p, the 6x3 blocks W of its
//               free-camera observations, (H_pp + lambda I)^-1, the point's step, its new residuals;
//   per camera / per pair of free cameras (a wave owns a block, the host lists the observation pairs of every block):
//               H_cc, b_c and the Schur complement S = H_cc + lambda I - sum W (H_pp + lambda I)^-1 W^T, g = b_c - sum W H_pp^-1 b_p;
//   Cholesky of S (<= 96 x 96, LDS) with g carried as an extra row, back-substitution, SE3 exponential update.
// Every sum has a fixed order: a lane adds its items in list order, 64 lane partials are combined by an xor butterfly
// (32, 16, ..., 1), wave partials are added in wave order.  No floating-point atomics: a call's bytes depend on its input only.
// Compiled with -ffp-contract=off.
#include "vo_internal.h"
#include <float.h>

#define BA_THREADS 256
#define BA_WAVES (BA_THREADS / 64)

__device__ __forceinline__ double ba_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of one value per lane over the workgroup, the same bits in every lane; red: BA_WAVES doubles of LDS
__device__ __forceinline__ double ba_block_sum(double v, double* red)
{
    v = ba_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < BA_WAVES; w++) s += red[w];
    return s;
}

__device__ __forceinline__ double ba_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < BA_WAVES; w++) s = fmax(s, red[w]);
    return s;
}

// EdgeProjectXYZ2UV::computeError + RobustKernelHuber: camera coordinates q, error e = obs - projection, rho and weight
struct BaEdge { double x, y, z, ex, ey, rho, w; };

__device__ __forceinline__ BaEdge ba_edge(const double* T, const double* X, double u, double v, const BaParams& P)
{
    BaEdge E;
    E.x = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3];
    E.y = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7];
    E.z = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    E.ex = u - (P.focal * E.x / E.z + P.cx);
    E.ey = v - (P.focal * E.y / E.z + P.cy);
    const double e2 = E.ex * E.ex + E.ey * E.ey;
    const double s = sqrt(e2);
    if (P.delta > 0 && s > P.delta) { E.rho = 2 * P.delta * s - P.delta * P.delta; E.w = P.delta / s; }
    else { E.rho = e2; E.w = 1.0; }
    return E;
}

// EdgeProjectXYZ2UV::linearizeOplus: d e / d pose (columns omega, upsilon) and d e / d X = -(1/z) [[f 0 -fx/z] [0 f -fy/z]] R
__device__ __forceinline__ void ba_jac_pose(const BaEdge& E, double f, double Jp[2][6])
{
    const double iz = 1.0 / E.z, iz2 = 1.0 / (E.z * E.z);
    Jp[0][0] = E.x * E.y * iz2 * f;          Jp[0][1] = -(1 + E.x * E.x * iz2) * f;  Jp[0][2] = E.y * iz * f;
    Jp[0][3] = -iz * f;                      Jp[0][4] = 0;                           Jp[0][5] = E.x * iz2 * f;
    Jp[1][0] = (1 + E.y * E.y * iz2) * f;    Jp[1][1] = -E.x * E.y * iz2 * f;        Jp[1][2] = -E.x * iz * f;
    Jp[1][3] = 0;                            Jp[1][4] = -iz * f;                     Jp[1][5] = E.y * iz2 * f;
}

__device__ __forceinline__ void ba_jac_point(const BaEdge& E, const double* T, double f, double Jx[2][3])
{
    const double a = f / E.z, bx = -f * E.x / (E.z * E.z), by = -f * E.y / (E.z * E.z);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        Jx[0][k] = -(a * T[k] + bx * T[8 + k]);
        Jx[1][k] = -(a * T[4 + k] + by * T[8 + k]);
    }
}

// Eigen's Quaternion(Matrix3) followed by SE3Quat::normalizeRotation (w >= 0, unit norm); q = (x, y, z, w), R row-major 3x3 with stride ld
__device__ void ba_quat_from_rot(const double* R, int ld, double q[4])
{
    double m[3][3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) m[r][c] = R[ld * r + c];
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t;
    }
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// Eigen's Quaternion::toRotationMatrix into the rotation part of a 3x4 [R | t]
__device__ void ba_rot_from_quat(const double q[4], double* T)
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    T[0] = 1 - (tyy + tzz); T[1] = txy - twz;       T[2] = txz + twy;
    T[4] = txy + twz;       T[5] = 1 - (txx + tzz); T[6] = tyz - twx;
    T[8] = txz - twy;       T[9] = tyz + twx;       T[10] = 1 - (txx + tyy);
}

// SE3Quat::exp (rotation first; below 1e-5 rad g2o takes R = I + W + W^2/2 and V = R) and T <- exp(d) T
__device__ void ba_pose_update(const double* d, const double* q_old, const double* T_old, double* q_new, double* T_new)
{
    const double w0 = d[0], w1 = d[1], w2 = d[2];
    const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double W[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double W2[9], R[9], V[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) W2[3 * r + c] = W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c] + W[3 * r + 2] * W[6 + c];
    if (th < 1e-5) {
        for (int i = 0; i < 9; i++) { R[i] = (i % 4 == 0 ? 1.0 : 0.0) + W[i] + 0.5 * W2[i]; V[i] = R[i]; }
    } else {
        const double a = sin(th) / th, b = (1 - cos(th)) / (th * th), c = (th - sin(th)) / (th * th * th);
        for (int i = 0; i < 9; i++) {
            R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * W[i] + b * W2[i];
            V[i] = (i % 4 == 0 ? 1.0 : 0.0) + b * W[i] + c * W2[i];
        }
    }
    double dq[4];
    ba_quat_from_rot(R, 3, dq);
    // Quaternion product dq * q_old, then normalizeRotation
    const double ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = q_old[0], by = q_old[1], bz = q_old[2], bw = q_old[3];
    double q[4];
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by + ay * bw + az * bx - ax * bz;
    q[2] = aw * bz + az * bw + ax * by - ay * bx;
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q_new[i] = q[i] / n;
    ba_rot_from_quat(q_new, T_new);
    for (int r = 0; r < 3; r++) {
        const double rt = R[3 * r] * T_old[3] + R[3 * r + 1] * T_old[7] + R[3 * r + 2] * T_old[11];
        const double vt = V[3 * r] * d[3] + V[3 * r + 1] * d[4] + V[3 * r + 2] * d[5];
        T_new[4 * r + 3] = rt + vt;
    }
}

__device__ __forceinline__ int ba_block_index(int c1, int c2, int F) { return c1 * F - c1 * (c1 - 1) / 2 + (c2 - c1); }

__global__ __launch_bounds__(BA_THREADS) void k_bundle_adjust(BaBuf D, BaParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    double* S = (double*)s_dyn;                              // [(n + 1)][ld]: lower triangle of the Schur complement, row n = g
    __shared__ double s_cam[2][VO_BA_MAX_CAMERAS * 12];      // [R | t] of every camera: current and trial
    __shared__ double s_q[2][VO_BA_MAX_FREE * 4];            // unit quaternions of the free cameras: current and trial
    __shared__ double s_Hcc[VO_BA_MAX_FREE * 36], s_bc[VO_BA_MAX_FREE * 6], s_dc[VO_BA_MAX_FREE * 6];
    __shared__ double s_red[BA_WAVES], s_lm[4];              // lambda, nu, chi2, rho
    __shared__ int s_col[VO_BA_MAX_CAMERAS], s_free[VO_BA_MAX_FREE], s_blk[VO_BA_MAX_FREE * (VO_BA_MAX_FREE + 1) / 2];
    __shared__ int s_fail, s_ctl[2];                         // solver failure of the trial; {accepted, go on with another trial}

    const BaProblem pb = D.prob[blockIdx.x];
    if (pb.skip) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ncam = pb.ncam, npt = pb.npt, F = pb.nfree, n = 6 * F, ld = n | 1, nblk = F * (F + 1) / 2;
    double* poses = D.poses + (size_t)12 * pb.cam0;
    const int* col_g = D.cam_col + pb.cam0;
    double* Xbuf[2] = {D.X + (size_t)3 * pb.pt0, D.X2 + (size_t)3 * pb.pt0};
    const int* ptf = D.pt_first + pb.pt0 + blockIdx.x;       // npt + 1 entries per problem
    const int* ocam = D.obs_cam + pb.obs0;
    const int* opt = D.obs_pt + pb.obs0;
    const double* oxy = D.obs_xy + (size_t)2 * pb.obs0;
    double* Wg = D.W + (size_t)18 * pb.obs0;
    double* Hpp = D.Hpp + (size_t)6 * pb.pt0;
    double* bp = D.bp + (size_t)3 * pb.pt0;
    double* Hpi = D.Hpi + (size_t)6 * pb.pt0;
    const int2* pairs = D.pairs + pb.pair0;
    const int* blk_first = D.blk_first + pb.blk0;            // nblk + 1 entries per problem

    for (int i = tid; i < ncam * 12; i += BA_THREADS) { s_cam[0][i] = poses[i]; s_cam[1][i] = poses[i]; }
    for (int i = tid; i < ncam; i += BA_THREADS) { const int c = col_g[i]; s_col[i] = c; if (c >= 0) s_free[c] = i; }
    for (int c1 = tid; c1 < F; c1 += BA_THREADS)
        for (int c2 = c1; c2 < F; c2++) s_blk[ba_block_index(c1, c2, F)] = c1 | (c2 << 8);
    __syncthreads();
    if (tid < F) {                                           // g2o keeps a free camera's rotation as a unit quaternion
        double q[4];
        double* T = s_cam[0] + 12 * s_free[tid];
        ba_quat_from_rot(T, 4, q);
        for (int i = 0; i < 4; i++) s_q[0][4 * tid + i] = q[i];
        ba_rot_from_quat(q, T);
    }
    __syncthreads();

    int cur = 0;                                             // which of Xbuf / s_cam / s_q holds the current estimate
    {
        double part = 0;
        for (int p = tid; p < npt; p += BA_THREADS) {
            const double* X = Xbuf[0] + 3 * p;
            for (int j = ptf[p]; j < ptf[p + 1]; j++) part += ba_edge(s_cam[0] + 12 * ocam[j], X, oxy[2 * j], oxy[2 * j + 1], P).rho;
        }
        const double chi = ba_block_sum(part, s_red);
        if (tid == 0) { s_lm[0] = -1.0; s_lm[1] = 2.0; s_lm[2] = chi; s_lm[3] = 0; D.chi2[2 * blockIdx.x] = chi; }
    }
    __syncthreads();

    int it_run = 0, trials = 0;
    for (int it = 0; it < P.iterations; it++) {
        it_run++;
        const double* C = s_cam[cur];
        const double* Xc = Xbuf[cur];
        double* Xn = Xbuf[cur ^ 1];
        // ---- linearise: per point H_pp, b_p and the W blocks
        double dmax = 0;
        for (int p = tid; p < npt; p += BA_THREADS) {
            double h[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
            const double* X = Xc + 3 * p;
            for (int j = ptf[p]; j < ptf[p + 1]; j++) {
                const int ci = ocam[j];
                const double* T = C + 12 * ci;
                const BaEdge E = ba_edge(T, X, oxy[2 * j], oxy[2 * j + 1], P);
                double Jx[2][3];
                ba_jac_point(E, T, P.focal, Jx);
                h[0] += E.w * (Jx[0][0] * Jx[0][0] + Jx[1][0] * Jx[1][0]);
                h[1] += E.w * (Jx[0][0] * Jx[0][1] + Jx[1][0] * Jx[1][1]);
                h[2] += E.w * (Jx[0][0] * Jx[0][2] + Jx[1][0] * Jx[1][2]);
                h[3] += E.w * (Jx[0][1] * Jx[0][1] + Jx[1][1] * Jx[1][1]);
                h[4] += E.w * (Jx[0][1] * Jx[0][2] + Jx[1][1] * Jx[1][2]);
                h[5] += E.w * (Jx[0][2] * Jx[0][2] + Jx[1][2] * Jx[1][2]);
#pragma unroll
                for (int k = 0; k < 3; k++) b[k] -= E.w * (Jx[0][k] * E.ex + Jx[1][k] * E.ey);
                if (s_col[ci] >= 0) {
                    double Jp[2][6];
                    ba_jac_pose(E, P.focal, Jp);
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int k = 0; k < 3; k++) Wg[18 * (size_t)j + 3 * a + k] = E.w * (Jp[0][a] * Jx[0][k] + Jp[1][a] * Jx[1][k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 6; k++) Hpp[6 * (size_t)p + k] = h[k];
#pragma unroll
            for (int k = 0; k < 3; k++) bp[3 * (size_t)p + k] = b[k];
            dmax = fmax(dmax, fmax(h[0], fmax(h[3], h[5])));
        }
        // ---- linearise: per free camera H_cc, b_c (a wave per camera, over the diagonal block's observation list)
        for (int c = wave; c < F; c += BA_WAVES) {
            const int blk = ba_block_index(c, c, F);
            const double* T = C + 12 * s_free[c];
            double h[21], b[6];
#pragma unroll
            for (int k = 0; k < 21; k++) h[k] = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) b[k] = 0;
            for (int e = blk_first[blk] + lane; e < blk_first[blk + 1]; e += 64) {
                const int2 pr = pairs[e];
                if (pr.x != pr.y) continue;                  // a camera that observes a point twice: cross terms belong to S only
                const int j = pr.x;
                const BaEdge E = ba_edge(T, Xc + 3 * opt[j], oxy[2 * j], oxy[2 * j + 1], P);
                double Jp[2][6];
                ba_jac_pose(E, P.focal, Jp);
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int bb = a; bb < 6; bb++) h[k++] += E.w * (Jp[0][a] * Jp[0][bb] + Jp[1][a] * Jp[1][bb]);
                    b[a] -= E.w * (Jp[0][a] * E.ex + Jp[1][a] * E.ey);
                }
            }
#pragma unroll
            for (int k = 0; k < 21; k++) h[k] = ba_wave_sum(h[k]);
#pragma unroll
            for (int k = 0; k < 6; k++) b[k] = ba_wave_sum(b[k]);
            if (lane == 0) {
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int bb = a; bb < 6; bb++) { s_Hcc[36 * c + 6 * a + bb] = h[k]; s_Hcc[36 * c + 6 * bb + a] = h[k]; k++; }
                    s_bc[6 * c + a] = b[a];
                }
            }
        }
        __syncthreads();
        if (s_lm[0] < 0) {                                   // computeLambdaInit: tau * max diag(H), first iteration only (uniform branch)
            for (int i = tid; i < n; i += BA_THREADS) dmax = fmax(dmax, s_Hcc[36 * (i / 6) + 7 * (i % 6)]);
            const double m = ba_block_max(dmax, s_red);
            __syncthreads();
            if (tid == 0) s_lm[0] = 1e-5 * m;
            __syncthreads();
        }

        int qmax = 0, go_on = 1, accepted = 0;
        while (go_on) {                                      // at most 10 trials
            const double lam = s_lm[0];
            if (tid == 0) s_fail = 0;
            __syncthreads();
            // ---- (H_pp + lambda I)^-1 per point
            for (int p = tid; p < npt; p += BA_THREADS) {
                const double a = Hpp[6 * (size_t)p] + lam, b = Hpp[6 * (size_t)p + 1], c = Hpp[6 * (size_t)p + 2];
                const double d = Hpp[6 * (size_t)p + 3] + lam, e = Hpp[6 * (size_t)p + 4], f = Hpp[6 * (size_t)p + 5] + lam;
                const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
                const double det = a * c00 + b * c01 + c * c02;
                if (!(fabs(det) > 0) || !(fabs(det) <= DBL_MAX)) { atomicOr(&s_fail, 1); continue; }
                const double id = 1.0 / det;
                double* o = Hpi + 6 * (size_t)p;
                o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
                o[3] = (a * f - c * c) * id; o[4] = (b * c - a * e) * id; o[5] = (a * d - b * b) * id;
            }
            __syncthreads();
            const int failed_pts = s_fail;
            // ---- Schur complement: a wave per block (c1 <= c2) of free cameras
            if (!failed_pts) for (int blk = wave; blk < nblk; blk += BA_WAVES) {
                const int c1 = s_blk[blk] & 255, c2 = s_blk[blk] >> 8;
                double acc[6][6], ga[6];
#pragma unroll
                for (int a = 0; a < 6; a++) { ga[a] = 0;
#pragma unroll
                    for (int b = 0; b < 6; b++) acc[a][b] = 0; }
                for (int e = blk_first[blk] + lane; e < blk_first[blk + 1]; e += 64) {
                    const int2 pr = pairs[e];
                    const int p = opt[pr.x];
                    const double* W1 = Wg + 18 * (size_t)pr.x;
                    const double* W2 = Wg + 18 * (size_t)pr.y;
                    const double* hi = Hpi + 6 * (size_t)p;
                    const double i0 = hi[0], i1 = hi[1], i2 = hi[2], i3 = hi[3], i4 = hi[4], i5 = hi[5];
                    double w2[18];
#pragma unroll
                    for (int k = 0; k < 18; k++) w2[k] = W2[k];
                    const bool diag = c1 == c2 && pr.x == pr.y;
                    const double b0 = bp[3 * (size_t)p], b1 = bp[3 * (size_t)p + 1], b2 = bp[3 * (size_t)p + 2];
#pragma unroll
                    for (int a = 0; a < 6; a++) {
                        const double wa0 = W1[3 * a], wa1 = W1[3 * a + 1], wa2 = W1[3 * a + 2];
                        const double y0 = wa0 * i0 + wa1 * i1 + wa2 * i2, y1 = wa0 * i1 + wa1 * i3 + wa2 * i4, y2 = wa0 * i2 + wa1 * i4 + wa2 * i5;
#pragma unroll
                        for (int b = 0; b < 6; b++) acc[a][b] += y0 * w2[3 * b] + y1 * w2[3 * b + 1] + y2 * w2[3 * b + 2];
                        if (diag) ga[a] += y0 * b0 + y1 * b1 + y2 * b2;
                    }
                }
#pragma unroll
                for (int a = 0; a < 6; a++) {
#pragma unroll
                    for (int b = 0; b < 6; b++) acc[a][b] = ba_wave_sum(acc[a][b]);
                    if (c1 == c2) ga[a] = ba_wave_sum(ga[a]);
                }
                if (lane == 0) {
                    if (c1 == c2) {
#pragma unroll
                        for (int a = 0; a < 6; a++) {
#pragma unroll
                            for (int b = 0; b <= a; b++)
                                S[(6 * c1 + a) * ld + 6 * c1 + b] = (s_Hcc[36 * c1 + 6 * a + b] + (a == b ? lam : 0.0)) - acc[a][b];
                            S[n * ld + 6 * c1 + a] = s_bc[6 * c1 + a] - ga[a];
                        }
                    } else {
#pragma unroll
                        for (int a = 0; a < 6; a++)
#pragma unroll
                            for (int b = 0; b < 6; b++) S[(6 * c2 + b) * ld + 6 * c1 + a] = -acc[a][b];
                    }
                }
            }
            __syncthreads();
            // ---- Cholesky of S with g as row n (forward substitution for free), column by column; a non-positive pivot is
            //      g2o's "solver failed".  Every lane computes the pivot, so the verdict is uniform.
            int failed = failed_pts;
            for (int j = 0; j < n && !failed; j++) {
                const int i = j + 1 + tid;                   // the rows below the pivot
                double sjj = S[j * ld + j], sij = i <= n ? S[i * ld + j] : 0.0;
                for (int k = 0; k < j; k++) {
                    const double ljk = S[j * ld + k];
                    sjj -= ljk * ljk;
                    if (i <= n) sij -= S[i * ld + k] * ljk;
                }
                if (!(sjj > 0) || !(sjj <= DBL_MAX)) { failed = 1; break; }
                const double piv = sqrt(sjj);
                __syncthreads();                             // every lane has read row j's old diagonal
                if (tid == 0) S[j * ld + j] = piv;
                if (i <= n) S[i * ld + j] = sij / piv;
                __syncthreads();
            }
            // ---- back substitution L^T x = y (y = row n)
            if (!failed) {
                for (int j = n - 1; j >= 0; j--) {
                    const double xj = S[n * ld + j] / S[j * ld + j];
                    __syncthreads();
                    if (tid == 0) { S[n * ld + j] = xj; s_dc[j] = xj; }
                    if (tid < j) S[n * ld + tid] -= S[j * ld + tid] * xj;
                    __syncthreads();
                }
            }
            __syncthreads();
            // ---- trial state: poses, then per point the step, the new point and its new residuals
            if (!failed && tid < F)
                ba_pose_update(s_dc + 6 * tid, s_q[cur] + 4 * tid, s_cam[cur] + 12 * s_free[tid], s_q[cur ^ 1] + 4 * tid, s_cam[cur ^ 1] + 12 * s_free[tid]);
            __syncthreads();
            double part_chi = 0, part_scale = 0;
            if (!failed) {
                const double* Cn = s_cam[cur ^ 1];
                for (int p = tid; p < npt; p += BA_THREADS) {
                    const int j0 = ptf[p], j1 = ptf[p + 1];
                    const double* X = Xc + 3 * p;
                    if (j0 == j1) { Xn[3 * p] = X[0]; Xn[3 * p + 1] = X[1]; Xn[3 * p + 2] = X[2]; continue; }
                    double r[3] = {bp[3 * (size_t)p], bp[3 * (size_t)p + 1], bp[3 * (size_t)p + 2]};
                    const double b0 = r[0], b1 = r[1], b2 = r[2];
                    for (int j = j0; j < j1; j++) {
                        const int c = s_col[ocam[j]];
                        if (c < 0) continue;
                        const double* W = Wg + 18 * (size_t)j;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            const double da = s_dc[6 * c + a];
                            r[0] -= W[3 * a] * da; r[1] -= W[3 * a + 1] * da; r[2] -= W[3 * a + 2] * da;
                        }
                    }
                    const double* hi = Hpi + 6 * (size_t)p;
                    const double d0 = hi[0] * r[0] + hi[1] * r[1] + hi[2] * r[2];
                    const double d1 = hi[1] * r[0] + hi[3] * r[1] + hi[4] * r[2];
                    const double d2 = hi[2] * r[0] + hi[4] * r[1] + hi[5] * r[2];
                    const double Xp[3] = {X[0] + d0, X[1] + d1, X[2] + d2};
                    Xn[3 * p] = Xp[0]; Xn[3 * p + 1] = Xp[1]; Xn[3 * p + 2] = Xp[2];
                    part_scale += d0 * (lam * d0 + b0) + d1 * (lam * d1 + b1) + d2 * (lam * d2 + b2);
                    for (int j = j0; j < j1; j++) part_chi += ba_edge(Cn + 12 * ocam[j], Xp, oxy[2 * j], oxy[2 * j + 1], P).rho;
                }
            }
            const double chi_new = ba_block_sum(part_chi, s_red);
            const double scale_p = ba_block_sum(part_scale, s_red);
            trials++;
            if (tid == 0) {                                  // OptimizationAlgorithmLevenberg::solve's accept / reject rule
                double tmp = chi_new, scale = 0;
                int bad = failed;
                for (int i = 0; i < n && !bad; i++) if (!(fabs(s_dc[i]) <= DBL_MAX)) bad = 1;   // a solve that did not produce numbers failed too
                if (!bad) {
                    for (int i = 0; i < n; i++) scale += s_dc[i] * (lam * s_dc[i] + s_bc[i]);
                    scale += scale_p;
                }
                if (bad || !(fabs(tmp) <= DBL_MAX)) tmp = DBL_MAX;
                scale += 1e-3;
                const double rho = (s_lm[2] - tmp) / scale;
                int acc = 0, more = 1;
                if (rho > 0 && tmp < DBL_MAX) {
                    const double t = 2 * rho - 1;
                    double alpha = 1.0 - t * t * t;
                    alpha = fmin(alpha, 2.0 / 3.0);
                    s_lm[0] = lam * fmax(1.0 / 3.0, alpha);
                    s_lm[1] = 2.0; s_lm[2] = tmp; acc = 1;
                } else {
                    s_lm[0] = lam * s_lm[1];
                    s_lm[1] *= 2;
                    if (!(fabs(s_lm[0]) <= DBL_MAX)) more = 0;
                }
                s_lm[3] = rho;
                s_ctl[0] = acc;
                s_ctl[1] = more;
            }
            __syncthreads();
            accepted = s_ctl[0];
            const int more = s_ctl[1];
            const double rho = s_lm[3];
            if (more) qmax++;
            go_on = more && rho < 0 && qmax < 10;
            __syncthreads();
            if (accepted) break;                             // rho > 0: the trial loop ends here anyway
        }
        if (accepted) cur ^= 1;
        {
            const double rho = s_lm[3], lam = s_lm[0];
            if (qmax == 10 || rho == 0 || !(fabs(lam) <= DBL_MAX)) break;
        }
    }

    // ---- results: free cameras, observed points (everything else keeps its input bytes)
    __syncthreads();
    if (tid < F) {
        const int ci = s_free[tid];
        for (int i = 0; i < 12; i++) poses[12 * ci + i] = s_cam[cur][12 * ci + i];
    }
    if (cur == 1)
        for (int p = tid; p < npt; p += BA_THREADS)
            if (ptf[p] != ptf[p + 1]) { Xbuf[0][3 * p] = Xbuf[1][3 * p]; Xbuf[0][3 * p + 1] = Xbuf[1][3 * p + 1]; Xbuf[0][3 * p + 2] = Xbuf[1][3 * p + 2]; }
    if (tid == 0) {
        D.chi2[2 * blockIdx.x + 1] = s_lm[2];
        D.iterations_run[blockIdx.x] = it_run;
        D.trials_run[blockIdx.x] = trials;
    }
}

size_t ba_dynamic_lds(int max_free) { const int n = 6 * max_free; return (size_t)(n + 1) * (n | 1) * sizeof(double); }

void launch_bundle_adjust(hipStream_t s, const BaBuf& D, const BaParams& P, int B, int max_free)
{
    if (B <= 0) return;
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_bundle_adjust, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ba_dynamic_lds(VO_BA_MAX_FREE)); attr = true; }
    hipLaunchKernelGGL(k_bundle_adjust, dim3(B), dim3(BA_THREADS), ba_dynamic_lds(max_free), s, D, P);
}
