// pgo_kernels.hip — k_pose_graph: Sim(3) pose-graph optimisation (include/vo_hip.h, "pose graph"; the checker is
// tests/pose_graph_reference.py).  One workgroup of 256 lanes per graph, the whole Levenberg-Marquardt loop inside the kernel; only
// __syncthreads().
//   per edge    (a lane owns an edge): E = C S_i S_j^-1, e = log E, Huber, d e / d S_j = -Ad(E); d e / d S_i = Ad(C) once;
//   per (free vertex, row) (a lane owns one row of the vertex's 7x7 blocks): H(v, v), b(v), H(v, v + 1) gathered over the vertex's
//               edge list in input order; a separator also adds its blocks against lower-numbered separators into the dense Hss;
//   per run     (a wave owns a run of consecutive free vertices, lanes 0 .. 14 own the right-hand sides b and the 7 + 7 coupling
//               columns of its two ends): block-tridiagonal Cholesky, forward and backward substitution, vertex after vertex;
//   separators: S = Hss + lambda I - the runs' Schur complements (dense, g carried as the last row), k_bundle_adjust's column
//               Cholesky and back-substitution; in LDS when it fits PGO_LDS_DENSE_BYTES, in the call's scratch otherwise;
//   then the runs' steps from their solves and the separators' steps, the trial vertices exp(d) S and the trial chi2.
// Every sum has a fixed order: a lane adds its items in list order, 64 lane partials are combined by an xor butterfly, wave
// partials are added in wave order.  No floating-point atomics: a graph's bytes depend on its input only.  Compiled with
// -ffp-contract=off.
#include "pgo_layout.h"
#include <float.h>

#define PGO_THREADS 256
#define PGO_WAVES (PGO_THREADS / 64)
#define PGO_TH_W 1e-2                     // the header's switch-over thresholds
#define PGO_TH_S 1e-2
#define PGO_TH_LOG 1e-8

__device__ __forceinline__ double pgo_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double pgo_block_sum(double v, double* red)
{
    v = pgo_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < PGO_WAVES; w++) s += red[w];
    return s;
}

__device__ __forceinline__ double pgo_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < PGO_WAVES; w++) s = fmax(s, red[w]);
    return s;
}

// ---------------------------------------------------------------- Sim(3)
struct PgoSim { double s, R[9], t[3]; };

__device__ __forceinline__ PgoSim pgo_load(const double* p)
{
    PgoSim S; S.s = p[0];
#pragma unroll
    for (int i = 0; i < 9; i++) S.R[i] = p[1 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) S.t[i] = p[10 + i];
    return S;
}

__device__ __forceinline__ void pgo_store(double* p, const PgoSim& S)
{
    p[0] = S.s;
#pragma unroll
    for (int i = 0; i < 9; i++) p[1 + i] = S.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) p[10 + i] = S.t[i];
}

__device__ __forceinline__ PgoSim pgo_compose(const PgoSim& A, const PgoSim& B)          // x -> A (B x)
{
    PgoSim C; C.s = A.s * B.s;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) C.R[3 * r + c] = A.R[3 * r] * B.R[c] + A.R[3 * r + 1] * B.R[3 + c] + A.R[3 * r + 2] * B.R[6 + c];
        C.t[r] = A.s * (A.R[3 * r] * B.t[0] + A.R[3 * r + 1] * B.t[1] + A.R[3 * r + 2] * B.t[2]) + A.t[r];
    }
    return C;
}

__device__ __forceinline__ PgoSim pgo_inverse(const PgoSim& A)
{
    PgoSim C; C.s = 1.0 / A.s;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) C.R[3 * r + c] = A.R[3 * c + r];
        C.t[r] = -(A.R[r] * A.t[0] + A.R[3 + r] * A.t[1] + A.R[6 + r] * A.t[2]) / A.s;
    }
    return C;
}

// m_k = integral over [0, 1] of tau^k e^(tau sigma), k = 0 .. 6
__device__ void pgo_moments(double sigma, double m[7])
{
    if (fabs(sigma) < PGO_TH_S) {
        const double fact[8] = {1, 1, 2, 6, 24, 120, 720, 5040};
#pragma unroll
        for (int k = 0; k < 7; k++) {
            double acc = 0, p = 1;
#pragma unroll
            for (int n = 0; n < 8; n++) { acc += p / (fact[n] * (n + k + 1)); p *= sigma; }
            m[k] = acc;
        }
    } else {
        const double es = exp(sigma);
        m[0] = expm1(sigma) / sigma;
#pragma unroll
        for (int k = 1; k < 7; k++) m[k] = (es - k * m[k - 1]) / sigma;
    }
}

// V = C I + A [w]x + B [w]x^2
__device__ void pgo_v_coef(double th, double sigma, double& A, double& B, double& C)
{
    if (th < PGO_TH_W) {
        double m[7];
        pgo_moments(sigma, m);
        const double t2 = th * th;
        A = m[1] - t2 * m[3] / 6 + t2 * t2 * m[5] / 120;
        B = m[2] / 2 - t2 * m[4] / 24 + t2 * t2 * m[6] / 720;
        C = m[0];
        return;
    }
    double c0 = 0;
    if (fabs(sigma) < PGO_TH_S) {
        const double fact[8] = {1, 1, 2, 6, 24, 120, 720, 5040};
        double p = 1;
#pragma unroll
        for (int n = 0; n < 8; n++) { c0 += p / (fact[n] * (n + 1)); p *= sigma; }
    } else c0 = expm1(sigma) / sigma;
    const double em = expm1(sigma), h = sin(0.5 * th);
    const double a = (em + 1) * sin(th);
    const double omb = 2 * h * h - em * cos(th);
    const double c = th * th + sigma * sigma;
    A = (a * sigma + omb * th) / (th * c);
    B = (c0 - (a * th - omb * sigma) / c) / (th * th);
    C = c0;
}

__device__ __forceinline__ void pgo_hat_sq(const double* w, double W[9], double W2[9])
{
    W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) W2[3 * r + c] = W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c] + W[3 * r + 2] * W[6 + c];
}

__device__ PgoSim pgo_exp(const double* d)
{
    const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), sigma = d[6];
    double W[9], W2[9], sa, ca, A, B, C;
    pgo_hat_sq(d, W, W2);
    if (th < PGO_TH_W) {
        const double t2 = th * th;
        sa = 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42));
        ca = 0.5 - t2 / 24 * (1 - t2 / 30 * (1 - t2 / 56));
    } else {
        const double h = sin(0.5 * th);
        sa = sin(th) / th; ca = 2 * h * h / (th * th);
    }
    pgo_v_coef(th, sigma, A, B, C);
    PgoSim S; S.s = exp(sigma);
#pragma unroll
    for (int i = 0; i < 9; i++) S.R[i] = (i % 4 == 0 ? 1.0 : 0.0) + sa * W[i] + ca * W2[i];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double v = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) v += ((r == c ? C : 0.0) + A * W[3 * r + c] + B * W2[3 * r + c]) * d[3 + c];
        S.t[r] = v;
    }
    return S;
}

// Eigen's Quaternion(Matrix3), w >= 0, unit norm; q = (x, y, z, w)
__device__ void pgo_quat_from_rot(const double* R, double q[4])
{
    const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7], m22 = R[8];
    double t = m00 + m11 + m22;
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m21 - m12) * t; q[1] = (m02 - m20) * t; q[2] = (m10 - m01) * t;
    } else {                                                 // the largest diagonal entry, the first of equals (no indexed registers)
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > (i ? m11 : m00)) i = 2;
        if (i == 0) {
            t = sqrt(m00 - m11 - m22 + 1.0);
            q[0] = 0.5 * t; t = 0.5 / t;
            q[3] = (m21 - m12) * t; q[1] = (m10 + m01) * t; q[2] = (m20 + m02) * t;
        } else if (i == 1) {
            t = sqrt(m11 - m22 - m00 + 1.0);
            q[1] = 0.5 * t; t = 0.5 / t;
            q[3] = (m02 - m20) * t; q[2] = (m21 + m12) * t; q[0] = (m01 + m10) * t;
        } else {
            t = sqrt(m22 - m00 - m11 + 1.0);
            q[2] = 0.5 * t; t = 0.5 / t;
            q[3] = (m10 - m01) * t; q[0] = (m02 + m20) * t; q[1] = (m12 + m21) * t;
        }
    }
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

__device__ void pgo_log(const PgoSim& S, double* e)
{
    double q[4];
    pgo_quat_from_rot(S.R, q);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    double k;
    if (n < PGO_TH_LOG) { const double x = n / q[3]; k = 2 / q[3] * (1 - x * x / 3); }
    else k = 2 * atan2(n, q[3]) / n;
    const double w[3] = {k * q[0], k * q[1], k * q[2]};
    const double sigma = log(S.s);
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double W[9], W2[9], A, B, C, V[9];
    pgo_hat_sq(w, W, W2);
    pgo_v_coef(th, sigma, A, B, C);
#pragma unroll
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0 ? C : 0.0) + A * W[i] + B * W2[i];
    // u = V^-1 t by the adjugate
    const double c00 = V[4] * V[8] - V[5] * V[7], c01 = V[5] * V[6] - V[3] * V[8], c02 = V[3] * V[7] - V[4] * V[6];
    const double det = V[0] * c00 + V[1] * c01 + V[2] * c02;
    const double i00 = c00, i01 = V[2] * V[7] - V[1] * V[8], i02 = V[1] * V[5] - V[2] * V[4];
    const double i10 = c01, i11 = V[0] * V[8] - V[2] * V[6], i12 = V[2] * V[3] - V[0] * V[5];
    const double i20 = c02, i21 = V[1] * V[6] - V[0] * V[7], i22 = V[0] * V[4] - V[1] * V[3];
    e[0] = w[0]; e[1] = w[1]; e[2] = w[2];
    e[3] = (i00 * S.t[0] + i01 * S.t[1] + i02 * S.t[2]) / det;
    e[4] = (i10 * S.t[0] + i11 * S.t[1] + i12 * S.t[2]) / det;
    e[5] = (i20 * S.t[0] + i21 * S.t[1] + i22 * S.t[2]) / det;
    e[6] = sigma;
}

// sign * Ad(S) = sign * [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]], row-major 7x7
__device__ void pgo_adjoint(const PgoSim& S, double sign, double* out)
{
    for (int i = 0; i < 49; i++) out[i] = 0;
    const double T[9] = {0, -S.t[2], S.t[1], S.t[2], 0, -S.t[0], -S.t[1], S.t[0], 0};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            out[7 * r + c] = sign * S.R[3 * r + c];
            out[7 * (3 + r) + c] = sign * (T[3 * r] * S.R[c] + T[3 * r + 1] * S.R[3 + c] + T[3 * r + 2] * S.R[6 + c]);
            out[7 * (3 + r) + 3 + c] = sign * (S.s * S.R[3 * r + c]);
        }
        out[7 * (3 + r) + 6] = sign * -S.t[r];
    }
    out[48] = sign;
}

// chi2_k = sum w e^2 and Huber as k_bundle_adjust has it: rho, and the weight rho'
__device__ __forceinline__ double pgo_robust(const double* e, const double* w, double delta, double& weight)
{
    double e2 = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) e2 += w[k] * (e[k] * e[k]);
    const double s = sqrt(e2);
    if (delta > 0 && s > delta) { weight = delta / s; return 2 * delta * s - delta * delta; }
    weight = 1.0;
    return e2;
}

__device__ __forceinline__ int pgo_tri(int r, int c) { return r * (r + 1) / 2 + c; }   // c <= r

__global__ __launch_bounds__(PGO_THREADS) void k_pose_graph(PgoBuf D, PgoParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    __shared__ double s_ds[7 * PGO_MAX_SEPARATORS];          // the separators' step
    __shared__ double s_red[PGO_WAVES], s_lm[4];             // lambda, nu, chi2, rho
    __shared__ int s_fail, s_ctl[2];

    const PgoGraph G = D.graph[blockIdx.x];
    if (G.skip) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = G.nv, ne = G.ne, nrun = G.nrun, nsep = G.nsep, n = 7 * nsep, ld = n | 1;
    const PgoRun* runs = D.run + G.run0;
    const int* kind = D.kind + G.v0;
    const int* first = D.first + G.first0;
    const int* list = D.list + 2 * (size_t)G.e0;
    const int* edges = D.edges + 2 * (size_t)G.e0;
    const double* meas = D.meas + 13 * (size_t)G.e0;
    const double* info = D.info + 7 * (size_t)G.e0;
    double* simbuf[2] = {D.sims + 13 * (size_t)G.v0, D.trial + 13 * (size_t)G.v0};
    double* J = D.J + 98 * (size_t)G.e0;
    double* err = D.err + 7 * (size_t)G.e0;
    double* wgt = D.wgt + 7 * (size_t)G.e0;
    double* Hd = D.Hd + 49 * (size_t)G.v0;
    double* bv = D.bv + 7 * (size_t)G.v0;
    double* U = D.U + 49 * (size_t)G.v0;
    double* X = D.X + 105 * (size_t)G.v0;
    double* Lf = D.Lf + 28 * (size_t)G.v0;
    double* Wf = D.Wf + 49 * (size_t)G.v0;
    const size_t dd = (size_t)(n + 1) * ld;
    double* Hss = D.dense + G.dense0;                        // [(n + 1)][ld]: lower triangle, row n = g
    double* S = G.dense_lds ? (double*)s_dyn : Hss + dd;     // the trial's copy, factored in place

    // ---- the start: trial = current, d e / d S_i = Ad(C) of every edge, chi2 of the input
    for (int i = tid; i < 13 * nv; i += PGO_THREADS) simbuf[1][i] = simbuf[0][i];
    {
        double part = 0;
        for (int k = tid; k < ne; k += PGO_THREADS) {
            const PgoSim C = pgo_load(meas + 13 * (size_t)k);
            pgo_adjoint(C, 1.0, J + 98 * (size_t)k);
            const PgoSim E = pgo_compose(pgo_compose(C, pgo_load(simbuf[0] + 13 * edges[2 * k])), pgo_inverse(pgo_load(simbuf[0] + 13 * edges[2 * k + 1])));
            double e[7], w;
            pgo_log(E, e);
            part += pgo_robust(e, info + 7 * (size_t)k, P.delta, w);
        }
        const double chi = pgo_block_sum(part, s_red);
        if (tid == 0) { s_lm[0] = -1.0; s_lm[1] = 2.0; s_lm[2] = chi; s_lm[3] = 0; D.chi2[2 * blockIdx.x] = chi; }
    }
    __syncthreads();

    int cur = 0, it_run = 0, trials = 0;
    for (int it = 0; it < P.iterations; it++) {
        it_run++;
        const double* Sc = simbuf[cur];
        double* Sn = simbuf[cur ^ 1];
        // ---- linearise: per edge e, the weights and -Ad(E); Hss cleared
        for (int k = tid; k < ne; k += PGO_THREADS) {
            const PgoSim E = pgo_compose(pgo_compose(pgo_load(meas + 13 * (size_t)k), pgo_load(Sc + 13 * edges[2 * k])), pgo_inverse(pgo_load(Sc + 13 * edges[2 * k + 1])));
            double e[7], w;
            pgo_log(E, e);
            (void)pgo_robust(e, info + 7 * (size_t)k, P.delta, w);
#pragma unroll
            for (int c = 0; c < 7; c++) { err[7 * (size_t)k + c] = e[c]; wgt[7 * (size_t)k + c] = w * info[7 * (size_t)k + c]; }
            pgo_adjoint(E, -1.0, J + 98 * (size_t)k + 49);
        }
        for (size_t i = tid; i < dd; i += PGO_THREADS) Hss[i] = 0;
        __syncthreads();
        // ---- linearise: per (free vertex, row) the diagonal block, b, the block to v + 1, and a separator's dense rows
        double dmax = 0;
        for (int item = tid; item < 7 * nv; item += PGO_THREADS) {
            const int v = item / 7, r = item - 7 * v, kv = kind[v];
            if (kv == -2) continue;
            const bool next_free = v + 1 < nv && kind[v + 1] != -2;
            double hd[7], hu[7], b = 0;
#pragma unroll
            for (int c = 0; c < 7; c++) { hd[c] = 0; hu[c] = 0; }
            for (int l = first[v]; l < first[v + 1]; l++) {
                const int k = list[l];
                const int side = edges[2 * k] == v ? 0 : 1, o = edges[2 * k + 1 - side];
                const double* Mv = J + 98 * (size_t)k + 49 * side;
                const double* Mo = J + 98 * (size_t)k + 49 * (1 - side);
                const int ko = kind[o];
                const bool up = next_free && o == v + 1, dense = kv >= 0 && ko >= 0 && ko < kv;
                double hs[7];
#pragma unroll
                for (int c = 0; c < 7; c++) hs[c] = 0;
#pragma unroll
                for (int q = 0; q < 7; q++) {
                    const double t = Mv[7 * q + r] * wgt[7 * (size_t)k + q];
                    b -= t * err[7 * (size_t)k + q];
#pragma unroll
                    for (int c = 0; c < 7; c++) hd[c] += t * Mv[7 * q + c];
                    if (up || dense) {
#pragma unroll
                        for (int c = 0; c < 7; c++) hs[c] += t * Mo[7 * q + c];
                    }
                }
                if (up) {
#pragma unroll
                    for (int c = 0; c < 7; c++) hu[c] += hs[c];
                }
                if (dense) {
                    double* row = Hss + (size_t)(7 * kv + r) * ld + 7 * ko;
#pragma unroll
                    for (int c = 0; c < 7; c++) row[c] += hs[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 7; c++) { Hd[49 * (size_t)v + 7 * r + c] = hd[c]; U[49 * (size_t)v + 7 * r + c] = hu[c]; }
            bv[7 * (size_t)v + r] = b;
            if (kv >= 0) {
                double* row = Hss + (size_t)(7 * kv + r) * ld + 7 * kv;
#pragma unroll
                for (int c = 0; c < 7; c++) if (c <= r) row[c] = hd[c];
                Hss[(size_t)n * ld + 7 * kv + r] = b;
            }
#pragma unroll
            for (int c = 0; c < 7; c++) if (c == r) dmax = fmax(dmax, hd[c]);
        }
        __syncthreads();
        if (s_lm[0] < 0) {                                   // lambda from the first linearisation: tau * max diag(H) (uniform branch)
            const double m = pgo_block_max(dmax, s_red);
            __syncthreads();
            if (tid == 0) s_lm[0] = 1e-5 * m;
            __syncthreads();
        }

        int qmax = 0, go_on = 1, accepted = 0;
        while (go_on) {                                      // at most 10 trials
            const double lam = s_lm[0];
            if (tid == 0) s_fail = 0;
            __syncthreads();
            // ---- runs: factor the block-tridiagonal matrix and substitute forward, 15 right-hand sides on 15 lanes
            for (int ri = wave; ri < nrun; ri += PGO_WAVES) {
                const PgoRun rn = runs[ri];
                const int c = lane < 15 ? lane : 0, cc = lane % 7;
                double W[49], y[7];
#pragma unroll
                for (int i = 0; i < 49; i++) W[i] = 0;
#pragma unroll
                for (int i = 0; i < 7; i++) y[i] = 0;
                int bad = 0;
                for (int v = rn.a; v <= rn.b && !bad; v++) {
                    double L[28];
#pragma unroll
                    for (int r = 0; r < 7; r++)
#pragma unroll
                        for (int q = 0; q <= r; q++) {
                            double s = 0;
#pragma unroll
                            for (int k = 0; k < 7; k++) s += W[7 * k + r] * W[7 * k + q];   // zero at the run's first vertex
                            L[pgo_tri(r, q)] = (Hd[49 * (size_t)v + 7 * r + q] + (r == q ? lam : 0.0)) - s;
                        }
#pragma unroll
                    for (int j = 0; j < 7; j++) {
                        double d = L[pgo_tri(j, j)];
#pragma unroll
                        for (int k = 0; k < j; k++) d -= L[pgo_tri(j, k)] * L[pgo_tri(j, k)];
                        if (!(d > 0) || !(d <= DBL_MAX)) bad = 1;
                        const double piv = sqrt(d);
                        L[pgo_tri(j, j)] = piv;
#pragma unroll
                        for (int i = j + 1; i < 7; i++) {
                            double s = L[pgo_tri(i, j)];
#pragma unroll
                            for (int k = 0; k < j; k++) s -= L[pgo_tri(i, k)] * L[pgo_tri(j, k)];
                            L[pgo_tri(i, j)] = s / piv;
                        }
                    }
                    if (bad) break;                          // the same in every lane: they all factor the same block
                    double rv[7];
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        double x = 0;
                        if (c == 0) x = bv[7 * (size_t)v + k];
                        else if (c <= 7) { if (v == rn.a && rn.lsep >= 0) x = U[49 * (size_t)(v - 1) + 7 * (c - 1) + k]; }
                        else if (v == rn.b && rn.rsep >= 0) x = U[49 * (size_t)v + 7 * k + (c - 8)];
                        rv[k] = x;
                    }
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        double s = 0;
#pragma unroll
                        for (int m = 0; m < 7; m++) s += W[7 * m + k] * y[m];
                        rv[k] -= s;
                    }
#pragma unroll
                    for (int i = 0; i < 7; i++) {
                        double s = rv[i];
#pragma unroll
                        for (int k = 0; k < i; k++) s -= L[pgo_tri(i, k)] * y[k];
                        y[i] = s / L[pgo_tri(i, i)];
                    }
                    if (lane < 15) {
#pragma unroll
                        for (int k = 0; k < 7; k++) X[105 * (size_t)v + 7 * c + k] = y[k];
                    }
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < 28; i++) Lf[28 * (size_t)v + i] = L[i];
                    }
                    if (v < rn.b) {                          // W = L^-1 H(v, v + 1): lane cc solves column cc, then all lanes take all columns
                        double wc[7];
#pragma unroll
                        for (int i = 0; i < 7; i++) {
                            double s = U[49 * (size_t)v + 7 * i + cc];
#pragma unroll
                            for (int k = 0; k < i; k++) s -= L[pgo_tri(i, k)] * wc[k];
                            wc[i] = s / L[pgo_tri(i, i)];
                        }
                        if (lane < 7) {
#pragma unroll
                            for (int k = 0; k < 7; k++) Wf[49 * (size_t)v + 7 * k + cc] = wc[k];
                        }
#pragma unroll
                        for (int k = 0; k < 7; k++)
#pragma unroll
                            for (int q = 0; q < 7; q++) W[7 * k + q] = __shfl(wc[k], q);
                    }
                }
                if (bad && lane == 0) atomicOr(&s_fail, 1);
            }
            __syncthreads();
            int failed = s_fail;
            // ---- runs: substitute backward
            if (!failed) for (int ri = wave; ri < nrun; ri += PGO_WAVES) {
                const PgoRun rn = runs[ri];
                if (lane >= 15) continue;
                double x[7];
#pragma unroll
                for (int i = 0; i < 7; i++) x[i] = 0;
                for (int v = rn.b; v >= rn.a; v--) {
                    double y[7];
#pragma unroll
                    for (int k = 0; k < 7; k++) y[k] = X[105 * (size_t)v + 7 * lane + k];
                    if (v < rn.b) {
#pragma unroll
                        for (int k = 0; k < 7; k++) {
                            double s = 0;
#pragma unroll
                            for (int m = 0; m < 7; m++) s += Wf[49 * (size_t)v + 7 * k + m] * x[m];
                            y[k] -= s;
                        }
                    }
                    const double* L = Lf + 28 * (size_t)v;
#pragma unroll
                    for (int i = 6; i >= 0; i--) {
                        double s = y[i];
#pragma unroll
                        for (int k = i + 1; k < 7; k++) s -= L[pgo_tri(k, i)] * x[k];
                        x[i] = s / L[pgo_tri(i, i)];
                    }
#pragma unroll
                    for (int k = 0; k < 7; k++) X[105 * (size_t)v + 7 * lane + k] = x[k];
                }
            }
            // ---- the separator system: S = Hss + lambda I, minus what the runs contribute through their ends
            if (!failed) {
                for (size_t i = tid; i < dd; i += PGO_THREADS) {
                    const int r = (int)(i / ld), c = (int)(i - (size_t)r * ld);
                    S[i] = Hss[i] + (r == c && r < n ? lam : 0.0);
                }
            }
            __syncthreads();
            if (!failed) for (int item = tid; item < 105 * nrun; item += PGO_THREADS) {   // a run's left end, and the block between its two ends
                const int ri = item / 105, e = item - 105 * ri;
                const PgoRun rn = runs[ri];
                if (rn.lsep < 0) continue;
                const double* Ul = U + 49 * (size_t)(rn.a - 1);              // H(a - 1, a)
                if (e < 49) {
                    const int i = e / 7, j = e - 7 * i;
                    if (j > i) continue;
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) s += Ul[7 * i + k] * X[105 * (size_t)rn.a + 7 * (1 + j) + k];
                    S[(size_t)(7 * rn.lsep + i) * ld + 7 * rn.lsep + j] -= s;
                } else if (e < 56) {
                    const int i = e - 49;
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) s += Ul[7 * i + k] * X[105 * (size_t)rn.a + k];
                    S[(size_t)n * ld + 7 * rn.lsep + i] -= s;
                } else if (rn.rsep >= 0) {
                    const int i = (e - 56) / 7, j = (e - 56) - 7 * i;
                    const double* Ur = U + 49 * (size_t)rn.b;                // H(b, b + 1)
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) s += Ur[7 * k + i] * X[105 * (size_t)rn.b + 7 * (1 + j) + k];
                    S[(size_t)(7 * rn.rsep + i) * ld + 7 * rn.lsep + j] -= s;
                }
            }
            __syncthreads();
            if (!failed) for (int item = tid; item < 56 * nrun; item += PGO_THREADS) {    // a run's right end
                const int ri = item / 56, e = item - 56 * ri;
                const PgoRun rn = runs[ri];
                if (rn.rsep < 0) continue;
                const double* Ur = U + 49 * (size_t)rn.b;
                if (e < 49) {
                    const int i = e / 7, j = e - 7 * i;
                    if (j > i) continue;
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) s += Ur[7 * k + i] * X[105 * (size_t)rn.b + 7 * (8 + j) + k];
                    S[(size_t)(7 * rn.rsep + i) * ld + 7 * rn.rsep + j] -= s;
                } else {
                    const int i = e - 49;
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 7; k++) s += Ur[7 * k + i] * X[105 * (size_t)rn.b + k];
                    S[(size_t)n * ld + 7 * rn.rsep + i] -= s;
                }
            }
            __syncthreads();
            // ---- Cholesky of S with g as row n, column by column; a non-positive pivot is a failed trial.  Every lane computes
            //      the pivot, so the verdict is uniform.  A lane owns the rows j + 1 + tid and j + 1 + tid + 256 (n + 1 <= 449).
            for (int j = 0; j < n && !failed; j++) {
                const int i0 = j + 1 + tid, i1 = i0 + PGO_THREADS;
                double sjj = S[(size_t)j * ld + j], s0 = i0 <= n ? S[(size_t)i0 * ld + j] : 0.0, s1 = i1 <= n ? S[(size_t)i1 * ld + j] : 0.0;
                for (int k = 0; k < j; k++) {
                    const double ljk = S[(size_t)j * ld + k];
                    sjj -= ljk * ljk;
                    if (i0 <= n) s0 -= S[(size_t)i0 * ld + k] * ljk;
                    if (i1 <= n) s1 -= S[(size_t)i1 * ld + k] * ljk;
                }
                if (!(sjj > 0) || !(sjj <= DBL_MAX)) { failed = 1; break; }
                const double piv = sqrt(sjj);
                __syncthreads();
                if (tid == 0) S[(size_t)j * ld + j] = piv;
                if (i0 <= n) S[(size_t)i0 * ld + j] = s0 / piv;
                if (i1 <= n) S[(size_t)i1 * ld + j] = s1 / piv;
                __syncthreads();
            }
            if (!failed) {
                for (int j = n - 1; j >= 0; j--) {
                    const double xj = S[(size_t)n * ld + j] / S[(size_t)j * ld + j];
                    __syncthreads();
                    if (tid == 0) { S[(size_t)n * ld + j] = xj; s_ds[j] = xj; }
                    for (int k = tid; k < j; k += PGO_THREADS) S[(size_t)n * ld + k] -= S[(size_t)j * ld + k] * xj;
                    __syncthreads();
                }
            }
            __syncthreads();
            // ---- every free vertex's step, the trial vertex, and d . (lambda d + b)
            double part_scale = 0;
            int nan_step = 0;
            if (!failed) for (int v = tid; v < nv; v += PGO_THREADS) {
                const int kv = kind[v];
                if (kv == -2) continue;
                double d[7];
                if (kv >= 0) {
#pragma unroll
                    for (int k = 0; k < 7; k++) d[k] = s_ds[7 * kv + k];
                } else {
                    int lo = 0, hi = nrun - 1;               // the run that holds v
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (runs[mid].b < v) lo = mid + 1; else hi = mid; }
                    const PgoRun rn = runs[lo];
                    const double* xv = X + 105 * (size_t)v;
#pragma unroll
                    for (int k = 0; k < 7; k++) {
                        double s = xv[k];
                        if (rn.lsep >= 0) {
#pragma unroll
                            for (int j = 0; j < 7; j++) s -= xv[7 * (1 + j) + k] * s_ds[7 * rn.lsep + j];
                        }
                        if (rn.rsep >= 0) {
#pragma unroll
                            for (int j = 0; j < 7; j++) s -= xv[7 * (8 + j) + k] * s_ds[7 * rn.rsep + j];
                        }
                        d[k] = s;
                    }
                }
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    if (!(fabs(d[k]) <= DBL_MAX)) nan_step = 1;
                    part_scale += d[k] * (lam * d[k] + bv[7 * (size_t)v + k]);
                }
                pgo_store(Sn + 13 * (size_t)v, pgo_compose(pgo_exp(d), pgo_load(Sc + 13 * (size_t)v)));
            }
            if (nan_step) atomicOr(&s_fail, 2);
            __syncthreads();
            if (s_fail) failed = 1;
            double part_chi = 0;
            if (!failed) for (int k = tid; k < ne; k += PGO_THREADS) {
                const PgoSim E = pgo_compose(pgo_compose(pgo_load(meas + 13 * (size_t)k), pgo_load(Sn + 13 * edges[2 * k])), pgo_inverse(pgo_load(Sn + 13 * edges[2 * k + 1])));
                double e[7], w;
                pgo_log(E, e);
                part_chi += pgo_robust(e, info + 7 * (size_t)k, P.delta, w);
            }
            const double chi_new = pgo_block_sum(part_chi, s_red);
            const double scale = pgo_block_sum(part_scale, s_red);
            trials++;
            if (tid == 0) {                                  // the accept / reject rule: k_bundle_adjust's, without g2o's + 1e-3
                double rho = -1.0;                           // a rejected trial
                if (!failed && fabs(chi_new) <= DBL_MAX && fabs(scale) <= DBL_MAX && scale > 0) rho = (s_lm[2] - chi_new) / scale;
                int acc = 0, more = 1;
                if (rho > 0) {
                    const double t = 2 * rho - 1;
                    double alpha = 1.0 - t * t * t;
                    alpha = fmin(alpha, 2.0 / 3.0);
                    s_lm[0] = lam * fmax(1.0 / 3.0, alpha);
                    s_lm[1] = 2.0; s_lm[2] = chi_new; acc = 1;
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
            if (accepted) break;
        }
        if (accepted) cur ^= 1;                              // (both buffers hold the fixed vertices since the start)
        {
            const double rho = s_lm[3], lam = s_lm[0];
            if (qmax == 10 || rho == 0 || !(fabs(lam) <= DBL_MAX)) break;
        }
    }

    // ---- results: free vertices (a fixed vertex keeps its input bytes)
    __syncthreads();
    if (cur == 1)
        for (int v = tid; v < nv; v += PGO_THREADS)
            if (kind[v] != -2) for (int i = 0; i < 13; i++) simbuf[0][13 * (size_t)v + i] = simbuf[1][13 * (size_t)v + i];
    if (tid == 0) {
        D.chi2[2 * blockIdx.x + 1] = s_lm[2];
        D.iterations_run[blockIdx.x] = it_run;
        D.trials_run[blockIdx.x] = trials;
    }
}

void launch_pose_graph(hipStream_t s, const PgoBuf& D, const PgoParams& P, int B, size_t lds_bytes)
{
    if (B <= 0) return;
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_pose_graph, hipFuncAttributeMaxDynamicSharedMemorySize, PGO_LDS_DENSE_BYTES); attr = true; }
    hipLaunchKernelGGL(k_pose_graph, dim3(B), dim3(PGO_THREADS), lds_bytes, s, D, P);
}
