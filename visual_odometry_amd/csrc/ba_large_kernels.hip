// ba_large_kernels.hip — vo_bundle_adjust_large: k_bundle_adjust's Levenberg-Marquardt (ba_kernels.hip) for one map of up to
// VO_BA_LARGE_MAX_FREE free cameras, as a sequence of kernels over the whole GPU.  The host drives the LM loop
// (ba_large_api.hip); workgroups synchronise at the kernel boundary only.
//   linearise   k_gba_lin_points: a lane owns a point (H_pp, b_p, W per free observation); k_gba_lin_cams: a wave owns a free
//               camera (H_cc, b_c); k_gba_lambda0 once: tau * the largest diagonal entry.
//   trial       k_gba_hpi: (H_pp + lambda I)^-1 by cofactors; k_gba_build: a wave owns a listed block of S; per panel of
//               GBA_NB columns k_gba_panel (the diagonal block factored in LDS by every workgroup alike, the rows below it
//               solved GBA_PANEL_ROWS per workgroup) and k_gba_update (the trailing update, one GBA_TILE x GBA_TILE tile
//               per workgroup); k_gba_backsub (one workgroup: L^T x = y); k_gba_step_cams (exp(delta) T); k_gba_step_points: a lane
//               owns a point (delta_p, the trial point, its robust residuals, its share of the gain denominator);
//               k_gba_decide: accept / reject, lambda, nu and the stop conditions into the device record.
// Every element of S sees its products subtracted one by one in ascending column order, each rounded (-ffp-contract=off), so
// the factor has the bits of the unblocked column Cholesky of k_bundle_adjust (tests/test_gpu_ba_large_solve.py compares them
// through vo_ba_large_solve).  Every sum has a fixed order: a lane adds its
// items in list order, 64 lane partials are combined by an xor butterfly, wave partials in wave order, workgroup partials
// in workgroup order.  No floating-point atomics.  A non-positive or non-finite pivot, or a singular H_pp + lambda I,
// sets GbaRec::fail; every later kernel of the trial reads it and returns; k_gba_decide then takes chi2 = DBL_MAX.
// The edge, Jacobian and SE3 routines restate ba_kernels.hip's (device code is not linked across translation units).
#include "gba_layout.h"
#include <float.h>

#define GBA_WAVES (GBA_THREADS / 64)
#define GBA_LDP (GBA_NB + 1)                   // row pitch of a panel tile in LDS, in doubles: odd, no bank conflicts
#define GBA_BACK_THREADS 512

__device__ __forceinline__ double gba_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of one value per lane over a workgroup of GBA_THREADS, the same bits in every lane; red: GBA_WAVES doubles of LDS
__device__ __forceinline__ double gba_block_sum(double v, double* red)
{
    v = gba_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < GBA_WAVES; w++) s += red[w];
    return s;
}

__device__ __forceinline__ double gba_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < GBA_WAVES; w++) s = fmax(s, red[w]);
    return s;
}

// second stage of a wide reduction: m per-workgroup partials, a lane adds every GBA_THREADS-th in index order
__device__ __forceinline__ double gba_sum_parts(const double* part, int m, double* red)
{
    double s = 0;
    for (int i = threadIdx.x; i < m; i += GBA_THREADS) s += part[i];
    return gba_block_sum(s, red);
}

// EdgeProjectXYZ2UV::computeError + RobustKernelHuber: camera coordinates, error = obs - projection, rho and weight
struct GbaEdge { double x, y, z, ex, ey, rho, w; };

__device__ __forceinline__ GbaEdge gba_edge(const double* T, const double* X, double u, double v, const BaParams& P)
{
    GbaEdge E;
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

__device__ __forceinline__ void gba_jac_pose(const GbaEdge& E, double f, double Jp[2][6])
{
    const double iz = 1.0 / E.z, iz2 = 1.0 / (E.z * E.z);
    Jp[0][0] = E.x * E.y * iz2 * f;          Jp[0][1] = -(1 + E.x * E.x * iz2) * f;  Jp[0][2] = E.y * iz * f;
    Jp[0][3] = -iz * f;                      Jp[0][4] = 0;                           Jp[0][5] = E.x * iz2 * f;
    Jp[1][0] = (1 + E.y * E.y * iz2) * f;    Jp[1][1] = -E.x * E.y * iz2 * f;        Jp[1][2] = -E.x * iz * f;
    Jp[1][3] = 0;                            Jp[1][4] = -iz * f;                     Jp[1][5] = E.y * iz2 * f;
}

__device__ __forceinline__ void gba_jac_point(const GbaEdge& E, const double* T, double f, double Jx[2][3])
{
    const double a = f / E.z, bx = -f * E.x / (E.z * E.z), by = -f * E.y / (E.z * E.z);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        Jx[0][k] = -(a * T[k] + bx * T[8 + k]);
        Jx[1][k] = -(a * T[4 + k] + by * T[8 + k]);
    }
}

// Eigen's Quaternion(Matrix3) followed by SE3Quat::normalizeRotation (w >= 0, unit norm); q = (x, y, z, w), R row-major with stride ld
__device__ void gba_quat_from_rot(const double* R, int ld, double q[4])
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
__device__ void gba_rot_from_quat(const double q[4], double* T)
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
__device__ void gba_pose_update(const double* d, const double* q_old, const double* T_old, double* q_new, double* T_new)
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
    gba_quat_from_rot(R, 3, dq);
    const double ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = q_old[0], by = q_old[1], bz = q_old[2], bw = q_old[3];
    double q[4];
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by + ay * bw + az * bx - ax * bz;
    q[2] = aw * bz + az * bw + ax * by - ay * bx;
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q_new[i] = q[i] / n;
    gba_rot_from_quat(q_new, T_new);
    for (int r = 0; r < 3; r++) {
        const double rt = R[3 * r] * T_old[3] + R[3 * r + 1] * T_old[7] + R[3 * r + 2] * T_old[11];
        const double vt = V[3 * r] * d[3] + V[3 * r + 1] * d[4] + V[3 * r + 2] * d[5];
        T_new[4 * r + 3] = rt + vt;
    }
}

// ------------------------------------------------------------------ start of a call
// cam[0] holds the input poses.  A free camera's rotation goes through the unit quaternion g2o keeps; cam[1] becomes a copy.
__global__ __launch_bounds__(GBA_THREADS) void k_gba_init_cams(GbaBuf D)
{
    const int i = blockIdx.x * GBA_THREADS + threadIdx.x;
    if (i >= D.ncam) return;
    double* T = D.cam[0] + 12 * (size_t)i;
    const int c = D.col[i];
    if (c >= 0) {
        double q[4];
        gba_quat_from_rot(T, 4, q);
        for (int k = 0; k < 4; k++) { D.quat[0][4 * (size_t)c + k] = q[k]; D.quat[1][4 * (size_t)c + k] = q[k]; }
        gba_rot_from_quat(q, T);
    }
    for (int k = 0; k < 12; k++) D.cam[1][12 * (size_t)i + k] = T[k];
}

// robust chi2 of the input: per-workgroup partials
__global__ __launch_bounds__(GBA_THREADS) void k_gba_chi2(GbaBuf D, BaParams P)
{
    __shared__ double s_red[GBA_WAVES];
    const int p = blockIdx.x * GBA_THREADS + threadIdx.x;
    double part = 0;
    if (p < D.npt) {
        const double* X = D.X[0] + 3 * (size_t)p;
        for (int j = D.pt_first[p]; j < D.pt_first[p + 1]; j++)
            part += gba_edge(D.cam[0] + 12 * (size_t)D.obs_cam[j], X, D.obs_xy[2 * (size_t)j], D.obs_xy[2 * (size_t)j + 1], P).rho;
    }
    const double s = gba_block_sum(part, s_red);
    if (threadIdx.x == 0) D.part_chi[blockIdx.x] = s;
}

__global__ __launch_bounds__(GBA_THREADS) void k_gba_rec_init(GbaBuf D)
{
    __shared__ double s_red[GBA_WAVES];
    const double chi = gba_sum_parts(D.part_chi, D.npw, s_red);
    if (threadIdx.x == 0) {
        GbaRec r;
        r.lam = -1.0; r.nu = 2.0; r.chi = chi; r.rho = 0;
        r.fail = 0; r.accepted = 0; r.go_on = 0; r.stop = 0; r.qmax = 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
        *D.rec = r;
    }
}

// ------------------------------------------------------------------ linearise
__global__ __launch_bounds__(GBA_THREADS) void k_gba_lin_points(GbaBuf D, BaParams P, int cur)
{
    __shared__ double s_red[GBA_WAVES];
    const int p = blockIdx.x * GBA_THREADS + threadIdx.x;
    const double* C = D.cam[cur];
    double dmax = 0;
    if (p < D.npt) {
        double h[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
        const double* X = D.X[cur] + 3 * (size_t)p;
        for (int j = D.pt_first[p]; j < D.pt_first[p + 1]; j++) {
            const int ci = D.obs_cam[j];
            const double* T = C + 12 * (size_t)ci;
            const GbaEdge E = gba_edge(T, X, D.obs_xy[2 * (size_t)j], D.obs_xy[2 * (size_t)j + 1], P);
            double Jx[2][3];
            gba_jac_point(E, T, P.focal, Jx);
            h[0] += E.w * (Jx[0][0] * Jx[0][0] + Jx[1][0] * Jx[1][0]);
            h[1] += E.w * (Jx[0][0] * Jx[0][1] + Jx[1][0] * Jx[1][1]);
            h[2] += E.w * (Jx[0][0] * Jx[0][2] + Jx[1][0] * Jx[1][2]);
            h[3] += E.w * (Jx[0][1] * Jx[0][1] + Jx[1][1] * Jx[1][1]);
            h[4] += E.w * (Jx[0][1] * Jx[0][2] + Jx[1][1] * Jx[1][2]);
            h[5] += E.w * (Jx[0][2] * Jx[0][2] + Jx[1][2] * Jx[1][2]);
#pragma unroll
            for (int k = 0; k < 3; k++) b[k] -= E.w * (Jx[0][k] * E.ex + Jx[1][k] * E.ey);
            if (D.col[ci] >= 0) {
                double Jp[2][6];
                gba_jac_pose(E, P.focal, Jp);
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int k = 0; k < 3; k++) D.W[18 * (size_t)j + 3 * a + k] = E.w * (Jp[0][a] * Jx[0][k] + Jp[1][a] * Jx[1][k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 6; k++) D.Hpp[6 * (size_t)p + k] = h[k];
#pragma unroll
        for (int k = 0; k < 3; k++) D.bp[3 * (size_t)p + k] = b[k];
        dmax = fmax(h[0], fmax(h[3], h[5]));
    }
    const double m = gba_block_max(dmax, s_red);
    if (threadIdx.x == 0) D.part_max[blockIdx.x] = m;
}

// a wave per free camera, over the camera's observations in sorted order
__global__ __launch_bounds__(GBA_THREADS) void k_gba_lin_cams(GbaBuf D, BaParams P, int cur)
{
    const int lane = threadIdx.x & 63, c = blockIdx.x * GBA_WAVES + (threadIdx.x >> 6);
    if (c >= D.F) return;
    const double* T = D.cam[cur] + 12 * (size_t)D.free_cam[c];
    const double* Xc = D.X[cur];
    double h[21], b[6];
#pragma unroll
    for (int k = 0; k < 21; k++) h[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) b[k] = 0;
    for (int e = D.cam_first[c] + lane; e < D.cam_first[c + 1]; e += 64) {
        const int j = D.cam_list[e];
        const GbaEdge E = gba_edge(T, Xc + 3 * (size_t)D.obs_pt[j], D.obs_xy[2 * (size_t)j], D.obs_xy[2 * (size_t)j + 1], P);
        double Jp[2][6];
        gba_jac_pose(E, P.focal, Jp);
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int bb = a; bb < 6; bb++) h[k++] += E.w * (Jp[0][a] * Jp[0][bb] + Jp[1][a] * Jp[1][bb]);
            b[a] -= E.w * (Jp[0][a] * E.ex + Jp[1][a] * E.ey);
        }
    }
#pragma unroll
    for (int k = 0; k < 21; k++) h[k] = gba_wave_sum(h[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) b[k] = gba_wave_sum(b[k]);
    if (lane == 0) {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int bb = a; bb < 6; bb++) { D.Hcc[36 * (size_t)c + 6 * a + bb] = h[k]; D.Hcc[36 * (size_t)c + 6 * bb + a] = h[k]; k++; }
            D.bc[6 * (size_t)c + a] = b[a];
        }
    }
}

// computeLambdaInit: tau * the largest diagonal entry of H (a maximum has no order)
__global__ __launch_bounds__(GBA_THREADS) void k_gba_lambda0(GbaBuf D)
{
    __shared__ double s_red[GBA_WAVES];
    double m = 0;
    for (int i = threadIdx.x; i < D.npw; i += GBA_THREADS) m = fmax(m, D.part_max[i]);
    for (int i = threadIdx.x; i < D.n; i += GBA_THREADS) m = fmax(m, D.Hcc[36 * (size_t)(i / 6) + 7 * (i % 6)]);
    m = gba_block_max(m, s_red);
    if (threadIdx.x == 0) D.rec->lam = 1e-5 * m;
}

// ------------------------------------------------------------------ a trial
__global__ __launch_bounds__(GBA_THREADS) void k_gba_hpi(GbaBuf D)
{
    const int p = blockIdx.x * GBA_THREADS + threadIdx.x;
    if (p >= D.npt) return;
    const double lam = D.rec->lam;
    const double a = D.Hpp[6 * (size_t)p] + lam, b = D.Hpp[6 * (size_t)p + 1], c = D.Hpp[6 * (size_t)p + 2];
    const double d = D.Hpp[6 * (size_t)p + 3] + lam, e = D.Hpp[6 * (size_t)p + 4], f = D.Hpp[6 * (size_t)p + 5] + lam;
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = a * c00 + b * c01 + c * c02;
    if (!(fabs(det) > 0) || !(fabs(det) <= DBL_MAX)) { atomicOr(&D.rec->fail, 1); return; }
    const double id = 1.0 / det;
    double* o = D.Hpi + 6 * (size_t)p;
    o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
    o[3] = (a * f - c * c) * id; o[4] = (b * c - a * e) * id; o[5] = (a * d - b * b) * id;
}

// S = H_cc + lambda I - sum W (H_pp + lambda I)^-1 W^T, g = b_c - sum W H_pp^-1 b_p: a wave per listed block.  The blocks that
// are not listed were cleared before the launch.
__global__ __launch_bounds__(GBA_THREADS) void k_gba_build(GbaBuf D)
{
    if (D.rec->fail) return;
    const int lane = threadIdx.x & 63, blk = blockIdx.x * GBA_WAVES + (threadIdx.x >> 6);
    if (blk >= D.nblk) return;
    const double lam = D.rec->lam;
    const int c1 = D.blocks[blk].c1, c2 = D.blocks[blk].c2, n = D.n;
    const size_t ld = (size_t)D.ld;
    double acc[6][6], ga[6];
#pragma unroll
    for (int a = 0; a < 6; a++) { ga[a] = 0;
#pragma unroll
        for (int b = 0; b < 6; b++) acc[a][b] = 0; }
    for (int e = D.blk_first[blk] + lane; e < D.blk_first[blk + 1]; e += 64) {
        const int2 pr = D.pairs[e];
        const int p = D.obs_pt[pr.x];
        const double* W1 = D.W + 18 * (size_t)pr.x;
        const double* W2 = D.W + 18 * (size_t)pr.y;
        const double* hi = D.Hpi + 6 * (size_t)p;
        const double i0 = hi[0], i1 = hi[1], i2 = hi[2], i3 = hi[3], i4 = hi[4], i5 = hi[5];
        double w2[18];
#pragma unroll
        for (int k = 0; k < 18; k++) w2[k] = W2[k];
        const bool diag = c1 == c2 && pr.x == pr.y;
        const double b0 = D.bp[3 * (size_t)p], b1 = D.bp[3 * (size_t)p + 1], b2 = D.bp[3 * (size_t)p + 2];
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
        for (int b = 0; b < 6; b++) acc[a][b] = gba_wave_sum(acc[a][b]);
        if (c1 == c2) ga[a] = gba_wave_sum(ga[a]);
    }
    if (lane != 0) return;
    if (c1 == c2) {
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = 0; b <= a; b++)
                D.S[(size_t)(6 * c1 + a) * ld + 6 * c1 + b] = (D.Hcc[36 * (size_t)c1 + 6 * a + b] + (a == b ? lam : 0.0)) - acc[a][b];
            D.S[(size_t)n * ld + 6 * c1 + a] = D.bc[6 * (size_t)c1 + a] - ga[a];
        }
    } else {
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) D.S[(size_t)(6 * c2 + b) * ld + 6 * c1 + a] = -acc[a][b];
    }
}

// Panel c0 .. c0 + nb: every workgroup factors the diagonal block in its LDS, column by column as k_bundle_adjust does, so every
// lane of the grid sees the same pivots and the same verdict; workgroup 0 writes the factor to Ld.  Then workgroup w solves the
// rows c0 + nb + GBA_PANEL_ROWS w .. below the block (row n = g among them): a lane owns a row.
__global__ __launch_bounds__(GBA_THREADS) void k_gba_panel(GbaBuf D, int c0, int nb)
{
    __shared__ double s_L[GBA_NB * GBA_LDP];
    __shared__ double s_A[GBA_PANEL_ROWS * GBA_LDP];
    if (D.rec->fail) return;
    const int tid = threadIdx.x, col = tid & 63, wave = tid >> 6, n = D.n;     // loads and stores: a wave moves a row, lane = column
    const size_t ld = (size_t)D.ld;
    const int row0 = c0 + nb + blockIdx.x * GBA_PANEL_ROWS;
    const int rows = min(GBA_PANEL_ROWS, n + 1 - row0);                        // >= 1 by the grid
    if (col < nb) {
#pragma unroll 4
        for (int r = wave; r < nb; r += GBA_WAVES) s_L[r * GBA_LDP + col] = D.S[(size_t)(c0 + r) * ld + c0 + col];
#pragma unroll 4
        for (int r = wave; r < rows; r += GBA_WAVES) s_A[r * GBA_LDP + col] = D.S[(size_t)(row0 + r) * ld + c0 + col];
    }
    __syncthreads();
    int failed = 0;
    for (int j = 0; j < nb; j++) {
        const int i = j + 1 + tid;                           // the rows below the pivot, inside the block
        double sjj = s_L[j * GBA_LDP + j], sij = i < nb ? s_L[i * GBA_LDP + j] : 0.0;
        for (int k = 0; k < j; k++) {
            const double ljk = s_L[j * GBA_LDP + k];
            sjj -= ljk * ljk;
            if (i < nb) sij -= s_L[i * GBA_LDP + k] * ljk;
        }
        if (!(sjj > 0) || !(sjj <= DBL_MAX)) { failed = 1; break; }   // uniform: every lane computed the same pivot
        const double piv = sqrt(sjj);
        __syncthreads();
        if (tid == 0) s_L[j * GBA_LDP + j] = piv;
        if (i < nb) s_L[i * GBA_LDP + j] = sij / piv;
        __syncthreads();
    }
    if (failed) {
        if (blockIdx.x == 0 && tid == 0) D.rec->fail = 1;
        return;
    }
    if (blockIdx.x == 0 && col < nb) {                       // (not into S: the other workgroups may still be reading the block)
        double* out = D.Ld + (size_t)(c0 / GBA_NB) * GBA_NB * GBA_NB;
        for (int r = wave; r < nb; r += GBA_WAVES) if (col <= r) out[r * GBA_NB + col] = s_L[r * GBA_LDP + col];
    }
    if (tid < rows) {
        double* a = s_A + tid * GBA_LDP;
        for (int j = 0; j < nb; j++) {
            double s = a[j];
            for (int k = 0; k < j; k++) s -= a[k] * s_L[j * GBA_LDP + k];
            a[j] = s / s_L[j * GBA_LDP + j];
        }
    }
    __syncthreads();
    if (col < nb) {
#pragma unroll 4
        for (int r = wave; r < rows; r += GBA_WAVES) D.S[(size_t)(row0 + r) * ld + c0 + col] = s_A[r * GBA_LDP + col];
    }
}

// Trailing update after panel c0 .. c0 + nb: S[i][j] -= sum_k S[i][k] S[j][k] over the panel's columns, k ascending, one rounded
// product at a time, for r0 = c0 + nb <= j <= i <= n (j < n: row n is g and has no diagonal).  Workgroup (tj, ti), tj <= ti, owns
// the GBA_TILE x GBA_TILE tile at (r0 + GBA_TILE ti, r0 + GBA_TILE tj); a lane owns 3 x 3 of it.
__global__ __launch_bounds__(GBA_THREADS) void k_gba_update(GbaBuf D, int c0, int nb)
{
    __shared__ double s_I[GBA_TILE * GBA_LDP], s_J[GBA_TILE * GBA_LDP];
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (tj > ti) return;
    if (D.rec->fail) return;
    const int tid = threadIdx.x, n = D.n, r0 = c0 + nb;
    const size_t ld = (size_t)D.ld;
    const int rowI = r0 + GBA_TILE * ti, rowJ = r0 + GBA_TILE * tj;
    for (int idx = tid; idx < GBA_TILE * nb; idx += GBA_THREADS) {
        const int r = idx / nb, c = idx - r * nb;
        s_I[r * GBA_LDP + c] = rowI + r <= n ? D.S[(size_t)(rowI + r) * ld + c0 + c] : 0.0;
        s_J[r * GBA_LDP + c] = rowJ + r <= n ? D.S[(size_t)(rowJ + r) * ld + c0 + c] : 0.0;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    double acc[3][3];
    bool live[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int gr = rowI + 3 * ty + i, gc = rowJ + 3 * tx + j;
            live[i][j] = gr <= n && gc <= gr && gc < n;
            acc[i][j] = live[i][j] ? D.S[(size_t)gr * ld + gc] : 0.0;
        }
    for (int k = 0; k < nb; k++) {
        double a[3], b[3];
#pragma unroll
        for (int i = 0; i < 3; i++) { a[i] = s_I[(3 * ty + i) * GBA_LDP + k]; b[i] = s_J[(3 * tx + i) * GBA_LDP + k]; }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) acc[i][j] -= a[i] * b[j];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (live[i][j]) D.S[(size_t)(rowI + 3 * ty + i) * ld + rowJ + 3 * tx + j] = acc[i][j];
}

// L^T x = y (y = row n, already forward-substituted), panels from the last to the first, x_j subtracted from the rows above in
// descending j as k_bundle_adjust does; x is delta_c.  One workgroup; y lies in LDS.
__global__ __launch_bounds__(GBA_BACK_THREADS) void k_gba_backsub(GbaBuf D)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    double* y = (double*)s_dyn;                              // [n]
    __shared__ double s_L[GBA_NB * GBA_LDP];
    if (D.rec->fail) return;
    const int tid = threadIdx.x, n = D.n;
    const size_t ld = (size_t)D.ld;
    for (int i = tid; i < n; i += GBA_BACK_THREADS) y[i] = D.S[(size_t)n * ld + i];
    __syncthreads();
    for (int c0 = ((n - 1) / GBA_NB) * GBA_NB; c0 >= 0; c0 -= GBA_NB) {
        const int nb = min(GBA_NB, n - c0);
        for (int idx = tid; idx < nb * nb; idx += GBA_BACK_THREADS) {
            const int r = idx / nb, c = idx - r * nb;
            if (c <= r) s_L[r * GBA_LDP + c] = D.Ld[(size_t)(c0 / GBA_NB) * GBA_NB * GBA_NB + r * GBA_NB + c];
        }
        __syncthreads();
        for (int j = nb - 1; j >= 0; j--) {
            const double xj = y[c0 + j] / s_L[j * GBA_LDP + j];
            __syncthreads();
            if (tid == 0) y[c0 + j] = xj;
            if (tid < j) y[c0 + tid] -= s_L[j * GBA_LDP + tid] * xj;
            __syncthreads();
        }
        for (int c = tid; c < c0; c += GBA_BACK_THREADS) {
            double acc = y[c];
#pragma unroll 8
            for (int j = nb - 1; j >= 0; j--) acc -= D.S[(size_t)(c0 + j) * ld + c] * y[c0 + j];
            y[c] = acc;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += GBA_BACK_THREADS) D.dc[i] = y[i];
}

// the trial cameras exp(delta_c) T: a lane owns a free camera
__global__ __launch_bounds__(GBA_THREADS) void k_gba_step_cams(GbaBuf D, int cur)
{
    if (D.rec->fail) return;
    const int c = blockIdx.x * GBA_THREADS + threadIdx.x;
    if (c >= D.F) return;
    const size_t ci = (size_t)D.free_cam[c];
    gba_pose_update(D.dc + 6 * (size_t)c, D.quat[cur] + 4 * (size_t)c, D.cam[cur] + 12 * ci, D.quat[cur ^ 1] + 4 * (size_t)c, D.cam[cur ^ 1] + 12 * ci);
}

// per point: the step, the trial point, its robust residuals and its share of sum delta (lambda delta + b)
__global__ __launch_bounds__(GBA_THREADS) void k_gba_step_points(GbaBuf D, BaParams P, int cur)
{
    __shared__ double s_red[GBA_WAVES];
    if (D.rec->fail) return;
    const double lam = D.rec->lam;
    const int p = blockIdx.x * GBA_THREADS + threadIdx.x;
    const double* Cn = D.cam[cur ^ 1];
    double part_chi = 0, part_scale = 0;
    if (p < D.npt) {
        const int j0 = D.pt_first[p], j1 = D.pt_first[p + 1];
        const double* X = D.X[cur] + 3 * (size_t)p;
        double* Xn = D.X[cur ^ 1] + 3 * (size_t)p;
        if (j0 == j1) { Xn[0] = X[0]; Xn[1] = X[1]; Xn[2] = X[2]; }
        else {
            double r[3] = {D.bp[3 * (size_t)p], D.bp[3 * (size_t)p + 1], D.bp[3 * (size_t)p + 2]};
            const double b0 = r[0], b1 = r[1], b2 = r[2];
            for (int j = j0; j < j1; j++) {
                const int c = D.col[D.obs_cam[j]];
                if (c < 0) continue;
                const double* W = D.W + 18 * (size_t)j;
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    const double da = D.dc[6 * (size_t)c + a];
                    r[0] -= W[3 * a] * da; r[1] -= W[3 * a + 1] * da; r[2] -= W[3 * a + 2] * da;
                }
            }
            const double* hi = D.Hpi + 6 * (size_t)p;
            const double d0 = hi[0] * r[0] + hi[1] * r[1] + hi[2] * r[2];
            const double d1 = hi[1] * r[0] + hi[3] * r[1] + hi[4] * r[2];
            const double d2 = hi[2] * r[0] + hi[4] * r[1] + hi[5] * r[2];
            const double Xp[3] = {X[0] + d0, X[1] + d1, X[2] + d2};
            Xn[0] = Xp[0]; Xn[1] = Xp[1]; Xn[2] = Xp[2];
            part_scale = d0 * (lam * d0 + b0) + d1 * (lam * d1 + b1) + d2 * (lam * d2 + b2);
            for (int j = j0; j < j1; j++)
                part_chi += gba_edge(Cn + 12 * (size_t)D.obs_cam[j], Xp, D.obs_xy[2 * (size_t)j], D.obs_xy[2 * (size_t)j + 1], P).rho;
        }
    }
    const double chi = gba_block_sum(part_chi, s_red);
    const double scale = gba_block_sum(part_scale, s_red);
    if (threadIdx.x == 0) { D.part_chi[blockIdx.x] = chi; D.part_scale[blockIdx.x] = scale; }
}

// OptimizationAlgorithmLevenberg::solve's accept / reject rule, as k_bundle_adjust's lane 0 applies it.  One workgroup adds the
// partials in index order; lane 0 decides and clears the failure flag for the next trial.
__global__ __launch_bounds__(GBA_THREADS) void k_gba_decide(GbaBuf D, int first_trial)
{
    __shared__ double s_red[GBA_WAVES];
    __shared__ int s_bad;
    GbaRec r = *D.rec;
    const double lam = r.lam;
    if (threadIdx.x == 0) s_bad = r.fail;
    __syncthreads();
    double chi_new = 0, scale_p = 0, scale_c = 0;
    if (!r.fail) {                                           // uniform
        chi_new = gba_sum_parts(D.part_chi, D.npw, s_red);
        scale_p = gba_sum_parts(D.part_scale, D.npw, s_red);
        double part = 0;
        int bad = 0;
        for (int i = threadIdx.x; i < D.n; i += GBA_THREADS) {
            const double d = D.dc[i];
            if (!(fabs(d) <= DBL_MAX)) bad = 1;              // a solve that did not produce numbers failed too
            part += d * (lam * d + D.bc[i]);
        }
        if (bad) atomicOr(&s_bad, 1);
        scale_c = gba_block_sum(part, s_red);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int bad = s_bad;
    double tmp = chi_new, scale = 0;
    if (!bad) scale = scale_c + scale_p;
    if (bad || !(fabs(tmp) <= DBL_MAX)) tmp = DBL_MAX;
    scale += 1e-3;
    const double rho = (r.chi - tmp) / scale;
    int acc = 0, more = 1;
    if (rho > 0 && tmp < DBL_MAX) {
        const double t = 2 * rho - 1;
        double alpha = 1.0 - t * t * t;
        alpha = fmin(alpha, 2.0 / 3.0);
        r.lam = lam * fmax(1.0 / 3.0, alpha);
        r.nu = 2.0; r.chi = tmp; acc = 1;
    } else {
        r.lam = lam * r.nu;
        r.nu *= 2;
        if (!(fabs(r.lam) <= DBL_MAX)) more = 0;
    }
    if (first_trial) r.qmax = 0;
    if (more) r.qmax++;
    r.rho = rho;
    r.accepted = acc;
    r.go_on = more && rho < 0 && r.qmax < 10;
    r.stop = !r.go_on && (r.qmax == 10 || rho == 0 || !(fabs(r.lam) <= DBL_MAX));
    r.fail = 0;
    *D.rec = r;
}

// ------------------------------------------------------------------ launches
static inline int gba_groups(int items, int per) { return (items + per - 1) / per; }

void launch_gba_init(hipStream_t s, const GbaBuf& D, const BaParams& P)
{
    if (D.ncam > 0) hipLaunchKernelGGL(k_gba_init_cams, dim3(gba_groups(D.ncam, GBA_THREADS)), dim3(GBA_THREADS), 0, s, D);
    if (D.npw > 0) hipLaunchKernelGGL(k_gba_chi2, dim3(D.npw), dim3(GBA_THREADS), 0, s, D, P);
    hipLaunchKernelGGL(k_gba_rec_init, dim3(1), dim3(GBA_THREADS), 0, s, D);
}

void launch_gba_linearise(hipStream_t s, const GbaBuf& D, const BaParams& P, int cur, bool first)
{
    if (D.npw > 0) hipLaunchKernelGGL(k_gba_lin_points, dim3(D.npw), dim3(GBA_THREADS), 0, s, D, P, cur);
    if (D.F > 0) hipLaunchKernelGGL(k_gba_lin_cams, dim3(gba_groups(D.F, GBA_WAVES)), dim3(GBA_THREADS), 0, s, D, P, cur);
    if (first) hipLaunchKernelGGL(k_gba_lambda0, dim3(1), dim3(GBA_THREADS), 0, s, D);
}

// S x = g on the device, n = 6 F > 0: the lower triangle of S and g as row n go in; the factor comes out in Ld (diagonal blocks)
// and S (below them), the forward-substituted g in row n, x in dc; a pivot that is not positive and finite sets rec->fail and
// leaves dc as it was.  2 ceil(n / GBA_NB) kernels: the last panel has no trailing update (below it lies g's row alone).
// Reads of D: S, Ld, dc, rec, n, ld.  A trial's solve (launch_gba_trial) and vo_ba_large_solve.
void launch_gba_factor_solve(hipStream_t s, const GbaBuf& D)
{
    for (int c0 = 0; c0 < D.n; c0 += GBA_NB) {
        const int nb = D.n - c0 < GBA_NB ? D.n - c0 : GBA_NB;
        const int below = D.n + 1 - (c0 + nb);                       // >= 1: g's row
        hipLaunchKernelGGL(k_gba_panel, dim3(gba_groups(below, GBA_PANEL_ROWS)), dim3(GBA_THREADS), 0, s, D, c0, nb);
        if (below > 1) {                                             // with g's row alone there is nothing left to update
            const int nt = gba_groups(below, GBA_TILE);
            hipLaunchKernelGGL(k_gba_update, dim3(nt, nt), dim3(GBA_THREADS), 0, s, D, c0, nb);
        }
    }
    hipLaunchKernelGGL(k_gba_backsub, dim3(1), dim3(GBA_BACK_THREADS), (size_t)D.n * sizeof(double), s, D);
}

// One trial: 2 ceil(n / GBA_NB) + 5 kernels and one clear of S for F > 0, 3 kernels for F = 0.
void launch_gba_trial(hipStream_t s, const GbaBuf& D, const BaParams& P, int cur, bool first_trial)
{
    if (D.npw > 0) hipLaunchKernelGGL(k_gba_hpi, dim3(D.npw), dim3(GBA_THREADS), 0, s, D);
    if (D.F > 0) {
        (void)hipMemsetAsync(D.S, 0, (size_t)(D.n + 1) * (size_t)D.ld * sizeof(double), s);
        hipLaunchKernelGGL(k_gba_build, dim3(gba_groups(D.nblk, GBA_WAVES)), dim3(GBA_THREADS), 0, s, D);
        launch_gba_factor_solve(s, D);
        hipLaunchKernelGGL(k_gba_step_cams, dim3(gba_groups(D.F, GBA_THREADS)), dim3(GBA_THREADS), 0, s, D, cur);
    }
    if (D.npw > 0) hipLaunchKernelGGL(k_gba_step_points, dim3(D.npw), dim3(GBA_THREADS), 0, s, D, P, cur);
    hipLaunchKernelGGL(k_gba_decide, dim3(1), dim3(GBA_THREADS), 0, s, D, first_trial ? 1 : 0);
}
