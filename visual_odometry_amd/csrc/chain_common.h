// chain_common.h — device helpers shared by the chain kernels (geom_kernels.hip) and the map kernels (slam_kernels.hip).
#pragma once
#include "vo_internal.h"

// squared reprojection error of one observation (src/map.py:56-66): T = the camera's [R | t] rows (row r at T[4r .. 4r+3]), X the point,
// (u, v) the keypoint.  One expression for k_reprojection and k_slam_filter, so the two keep the same bits.
__device__ __forceinline__ double reprojection_sqerr_one(const double* T, const double* X, const double* Kd, double u, double v)
{
    double c[3], t[3];
#pragma unroll
    for (int r = 0; r < 3; r++) c[r] = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2] + T[4 * r + 3] * 1.0;
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = Kd[3 * r] * c[0] + Kd[3 * r + 1] * c[1] + Kd[3 * r + 2] * c[2];
    const double dx = t[0] / t[2] - u, dy = t[1] / t[2] - v;
    return dx * dx + dy * dy;
}

__device__ __forceinline__ size_t chain_key(int f, int i, int cap) { return (size_t)f * cap + i; }

__device__ __forceinline__ void chain_root(const unsigned long long* parent, int cap, int F, int& f, int& i)
{
    for (int n = 0; n <= F; n++) {                      // track_feature_back_in_time (:94-99)
        const unsigned long long v = parent[chain_key(f, i, cap)];
        if (v == 0) return;
        f = (int)((v >> 20) & 0xfffffu); i = (int)(v & 0xfffffu);
    }
}

// The pair buffers as one sequence of a run sees them: its pair 0 is pair `first` of the run.  Only the members the chain and map
// kernels read are moved (slots, res, m_count, m_q, m_t, mask, px1, px2, ipx1, ipx2, X).
__device__ __forceinline__ PairBuf chain_pairs_from(PairBuf pb, int first, int kp_cap)
{
    const size_t c = (size_t)first * kp_cap;
    pb.slots += 2 * (size_t)first; pb.res += first; pb.m_count += first;
    pb.m_q += c; pb.m_t += c; pb.mask += c;
    pb.px1 += 2 * c; pb.px2 += 2 * c; pb.ipx1 += 2 * c; pb.ipx2 += 2 * c;
    pb.X += 4 * c;
    return pb;
}

// the j-th inlier's match index: inliers are numbered in match order, as k_pose_prepare compacts them (and as X's columns run)
template <typename F>
__device__ __forceinline__ void chain_for_each_inlier(const PairBuf& pb, int kp_cap, int p, int* s_w, F&& body)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = pb.m_count[p];
    const uint8_t* mask = pb.mask + (size_t)p * kp_cap;
    int base = 0;
    for (int b = 0; b < M; b += 256) {
        const int i = b + tid;
        const bool f = i < M && mask[i] != 0;
        const unsigned long long bal = __ballot(f);
        __syncthreads();
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < 4; w++) { const int c = s_w[w]; if (w < wave) off += c; tot += c; }
        body(f, i, base + off + (int)__popcll(bal & ((1ULL << lane) - 1)));
        base += tot;
    }
}
