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

// [deviation, documented in DESIGN.md] the reference stores camera 1 = (I, 0) and camera 2 = (R, t) but its first points in
// camera-2 coordinates (reconstruct_3d_points' default matrices) and lets the bundle adjustment reconcile them; without BA the
// cameras are stored consistently with the points: camera 2 = (I, 0), camera 1 = (R^T, -R^T t).
// initialize_map (:43-92) on pair p of the chain: p = 0 for k_chain_init, the pair that starts a new segment for
// k_slam_restart_seqs — there the first camera goes to seg_poses[p], since pose row p belongs to the segment before (p > 0).
// row0 = false (k_slam_restart_stream in a resumed call): pose row 0 is the anchor's row of the call before, also for p = 0.
__device__ __forceinline__ void chain_init_wg(PairBuf pb, int kp_cap, ChainBuf cb, int p = 0, bool row0 = true)
{
    __shared__ int s_w[4];
    const int tid = threadIdx.x;
    const vo_pair_result& r = pb.res[p];
    const int f1 = pb.slots[2 * p], f2 = pb.slots[2 * p + 1];
    if (r.status != VO_OK) {
        if (tid == 0) { cb.alive[0] = 0; cb.status[p] = r.status; cb.n_corr[p] = 0; cb.n_inl[p] = 0; cb.n_map[p] = 0; }
        return;
    }
    if (tid < 12) {
        const int rr = tid / 4, c = tid % 4;
        const double a = c < 3 ? r.R[c * 3 + rr] : -(r.R[0 * 3 + rr] * r.t[0] + r.R[1 * 3 + rr] * r.t[1] + r.R[2 * 3 + rr] * r.t[2]);
        const double b = c < 3 ? (rr == c ? 1.0 : 0.0) : 0.0;
        cb.cam[(size_t)f1 * 12 + tid] = a; cb.cam[(size_t)f2 * 12 + tid] = b;
        if (p == 0 && row0) cb.poses[tid] = a;
        if (cb.rs.st) cb.rs.seg_poses[(size_t)p * 12 + tid] = a;
        cb.poses[(size_t)(p + 1) * 12 + tid] = b;
    }
    if (tid == 0) { cb.cam_ok[f1] = 1; cb.cam_ok[f2] = 1; cb.alive[0] = 1; cb.status[p] = VO_OK; cb.n_corr[p] = 0; cb.n_inl[p] = 0; }
    const double* X = pb.X + (size_t)4 * p * kp_cap;         // the pair's [4][kp_cap], w = 1
    __shared__ int s_added;
    if (tid == 0) s_added = 0;
    int added = 0;
    chain_for_each_inlier(pb, kp_cap, p, s_w, [&](bool f, int i, int pos) {
        if (!f) return;
        const size_t k = chain_key(f1, pb.m_q[(size_t)p * kp_cap + i], kp_cap);   // TrackedPoint(match.point, ..., match.featureid1)  (:70-75)
        cb.in_map[k] = 1;
        for (int d = 0; d < 3; d++) cb.map_pt[3 * k + d] = X[(size_t)d * kp_cap + pos];
        added++;
    });
    __syncthreads();
    atomicAdd(&s_added, added);
    __syncthreads();
    if (tid == 0) { cb.map_count[0] = s_added; cb.n_map[p] = s_added; }
}
