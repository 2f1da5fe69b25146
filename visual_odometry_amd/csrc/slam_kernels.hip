// slam_kernels.hip — the map step that ends every frame of the reference's loop, on a map that stays in HBM (vo_slam_chain):
//   add_information_to_map with its Observations (src/visual_slam.py:101-180) -> k_slam_add
//   freeze_nonlast_cameras (:270-275)                                         -> k_slam_add (the flags are part of the camera list)
//   Map.optimize_map's graph bookkeeping (src/map.py:121-164)                 -> k_slam_ba_prepare, then k_bundle_adjust (ba_kernels.hip)
//   remove_observations_with_reprojection_errors_above_threshold (:46-70)     -> k_slam_filter
//   limit_number_of_camera_in_map / remove_camera_from_map (:188-232, 299-318)-> k_slam_limit
//   initialize_map's self.map.clean() (src/visual_slam.py:43-45), called again  -> k_slam_restart_seqs (vo_slam_chains_restart only)
//   Map.show_map_statistics (src/map.py:234-297; src/visual_slam.py:354)       -> k_slam_stats (vo_set_slam_stats on, and vo_map_statistics)
// One workgroup of 256 lanes per map and kernel: the walk is sequential by nature and the maps are the reference's size.
// Every step is written once, as a workgroup-wide device function, and has two kernels: k_slam_* for the one chain of vo_slam_chain
// (its buffers by value) and k_slam_*_seqs for the S independent sequences of vo_slam_chains — workgroup = sequence (blockIdx.x),
// which reads its SlamSeq descriptor and does step j of its own chain, or returns at once when its chain has fewer steps.
// vo_slam_stream continues a map an earlier call left: k_slam_carry restates its keys at the start of such a call, and the three
// steps that name a frame or a key have a third kernel, k_slam_*_stream — the same device function compiled with ST = true; the
// other kernels are compiled with ST = false and carry none of it.  vo_slam_stream_restart is the stream whose map restarts after
// a lost frame: k_slam_restart_stream, and k_slam_*_stream_restart / k_slam_carry_restart — the stream kernels compiled with RS = true.
// vo_slam_streams carries S such maps at once: k_slam_*_stream_restart_seqs, the same bodies with the sequence on the grid axis, and
// k_slam_carry_restart_seqs, whose workgroups clear the rows their own sequence held and no others (SQ = true).
// A seat of vo_slam_streams whose flight has ended takes another: k_slam_carry_restart_seats, the carry launch that also resets such a seat.
// Every list order is fixed by the input: positions come from ordered prefix sums (ballots / wave scans combined in wave
// order), integer atomics only count or hand out slots that are ordered afterwards, and there are no floating-point sums — but one:
// k_slam_stats' total reprojection error, which one lane adds in observation order because that order is its contract.  That kernel
// only reads the map and writes a statistics row of its own (StatsBuf); it is launched behind a switch that is off by default.
#include "chain_common.h"

#define SLAM_THREADS 256
#define SLAM_WAVES (SLAM_THREADS / 64)

// Ordered exclusive prefix sum over get(0) .. get(n - 1), 256 items per round: put(i, sum of the items before i, get(i)).
// n is uniform.  Within a round every get() runs before every put() (barriers), and a round's put() never writes where a
// later round's get() reads as long as put(i, pos, ..) writes at or below position i: a list can be compacted in place.
template <typename G, typename W>
__device__ __forceinline__ int slam_scan(int n, int* s_w, G&& get, W&& put)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int b = 0; b < n; b += SLAM_THREADS) {
        const int i = b + tid;
        const int v = i < n ? get(i) : 0;
        int x = v;
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
        __syncthreads();
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < SLAM_WAVES; w++) { const int c = s_w[w]; if (w < wave) off += c; tot += c; }
        if (i < n) put(i, base + off + x - v, v);
        base += tot;
    }
    return base;
}

// initialize_map (:56-87) for pair 0, add_information_to_map's loop (:152-179) for pair p >= 1: the camera of frame 2 joins the
// camera list, and every E inlier in match order appends what the reference appends — a new point under featureid1 with its
// observations on camera 1 and camera 2, or one observation of the point its track root owns.  Pass 1 takes every decision
// against the map as it was before the loop (the snapshot of :154-156) and stores it; pass 2 writes, after a barrier.
// RS (vo_slam_stream_restart): pose row 0 of a resumed call is the anchor's row of the call before, so a segment that starts at
// the call's pair 0 takes its first camera from seg_poses[0] like any other.
template <bool ST, bool RS = false>
__device__ __forceinline__ void slam_add_wg(PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras,
                                            ChainBuf cb, SlamBuf sb)
{
    __shared__ int s_w[SLAM_WAVES], s_cnt[3][SLAM_WAVES];
    if (!cb.alive[0]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f1 = pb.slots[2 * p], f2 = pb.slots[2 * p + 1];
    const int ncam0 = sb.m.cnt[0], npt0 = sb.m.cnt[1], nobs0 = sb.m.cnt[2];
    const int frame0 = ST ? sb.st.frame0 : 0;                  // vo_slam_stream: the call's pair 0 is pair frame0 of the stream
    const bool first = (p == 0 && frame0 == 0) || (cb.rs.st && cb.rs.st[SEG_INIT]);   // pair 0, or the pair that starts a new segment on a cleaned map
    const int newn = ncam0 + (first ? 2 : 1);
    if (newn > sb.cam_cap || (!first && ncam0 < 1)) return;   // cannot happen: the host sizes the list from max_cameras
    const int c1 = newn - 2, c2 = newn - 1;
    if (first) {
        if (tid < 12) sb.m.cam_pose[tid] = !RS && p == 0 ? cb.poses[tid] : cb.rs.seg_poses[(size_t)p * 12 + tid];
        else if (tid < 24) sb.m.cam_pose[tid] = cb.poses[(size_t)p * 12 + tid];
        if (tid < 2) sb.m.cam_frame[tid] = frame0 + p + tid;
    } else {
        if (tid < 12) sb.m.cam_pose[(size_t)c2 * 12 + tid] = cb.cam[(size_t)f2 * 12 + tid];
        if (tid == 0) sb.m.cam_frame[c2] = frame0 + p + 1;
    }
    // initialize_map: first camera fixed, second free; afterwards freeze_nonlast_cameras: all fixed but the last free_cameras
    for (int c = tid; c < newn; c += SLAM_THREADS) sb.m.cam_fixed[c] = first ? (c == 0) : (c < newn - free_cameras);

    chain_for_each_inlier(pb, kp_cap, p, s_w, [&](bool f, int i, int pos) {
        if (!f) return;
        int d = -1;                                            // -1: new point, -2: skipped, >= 0: observation of that point
        if (!first) {
            const double x = cb.Xw[4 * (size_t)pos], y = cb.Xw[4 * (size_t)pos + 1], z = cb.Xw[4 * (size_t)pos + 2];
            if (!(sqrt(x * x + y * y + z * z) <= max_norm)) d = -2;   // np.linalg.norm(match.point) > 50: continue (NaN: kept out)
            else {
                int rf = f2, ri = pb.m_t[(size_t)p * kp_cap + i];
                chain_root(cb.parent, kp_cap, F, rf, ri);
                d = sb.pt_of[chain_key(rf, ri, kp_cap)] - 1;
            }
        }
        sb.dec[i] = d;
    });
    __syncthreads();

    const int M = pb.m_count[p];
    const uint8_t* mask = pb.mask + (size_t)p * kp_cap;
    const double* px1 = pb.px1 + (size_t)p * kp_cap * 2;
    const double* px2 = pb.px2 + (size_t)p * kp_cap * 2;
    int ibase = 0, pbase = 0, obase = 0;
    for (int b = 0; b < M; b += SLAM_THREADS) {
        const int i = b + tid;
        const bool inl = i < M && mask[i] != 0;
        const int d = inl ? sb.dec[i] : -2;
        const bool is_new = d == -1, is_old = d >= 0;
        const unsigned long long bal_i = __ballot(inl), bal_n = __ballot(is_new), bal_o = __ballot(is_old);
        __syncthreads();
        if (lane == 0) { s_cnt[0][wave] = __popcll(bal_i); s_cnt[1][wave] = __popcll(bal_n); s_cnt[2][wave] = __popcll(bal_o); }
        __syncthreads();
        int off[3] = {0, 0, 0}, tot[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++)
            for (int w = 0; w < SLAM_WAVES; w++) { const int c = s_cnt[k][w]; if (w < wave) off[k] += c; tot[k] += c; }
        const unsigned long long lower = (1ULL << lane) - 1;
        const int ipos = ibase + off[0] + (int)__popcll(bal_i & lower);
        const int nb = off[1] + (int)__popcll(bal_n & lower), ob = off[2] + (int)__popcll(bal_o & lower);
        const int pi = npt0 + pbase + nb, oi = nobs0 + obase + 2 * nb + ob;
        if (is_new && pi < sb.pt_cap && oi + 2 <= sb.obs_cap) {     // add_new_match_to_map / initialize_map's loop
            const size_t k = chain_key(f1, pb.m_q[(size_t)p * kp_cap + i], kp_cap);
            double X[3];
            for (int a = 0; a < 3; a++) X[a] = first ? cb.map_pt[3 * k + a] : cb.Xw[4 * (size_t)ipos + a];
            if (!first) { cb.in_map[k] = 1; for (int a = 0; a < 3; a++) cb.map_pt[3 * k + a] = X[a]; }
            sb.pt_of[k] = pi + 1;
            sb.m.pt_key[pi] = (int)k;
            if (ST) { sb.m.pt_feat[2 * (size_t)pi] = frame0 + p; sb.m.pt_feat[2 * (size_t)pi + 1] = pb.m_q[(size_t)p * kp_cap + i]; }
            for (int a = 0; a < 3; a++) sb.m.pt_xyz[3 * (size_t)pi + a] = X[a];
            sb.m.obs_cam[oi] = c1; sb.m.obs_pt[oi] = pi;
            sb.m.obs_xy[2 * (size_t)oi] = px1[2 * i]; sb.m.obs_xy[2 * (size_t)oi + 1] = px1[2 * i + 1];
            sb.m.obs_cam[oi + 1] = c2; sb.m.obs_pt[oi + 1] = pi;
            sb.m.obs_xy[2 * (size_t)oi + 2] = px2[2 * i]; sb.m.obs_xy[2 * (size_t)oi + 3] = px2[2 * i + 1];
        }
        if (is_old && oi < sb.obs_cap) {                            // add_new_observation_of_existing_point
            sb.m.obs_cam[oi] = c2; sb.m.obs_pt[oi] = d;
            sb.m.obs_xy[2 * (size_t)oi] = px2[2 * i]; sb.m.obs_xy[2 * (size_t)oi + 1] = px2[2 * i + 1];
        }
        ibase += tot[0]; pbase += tot[1]; obase += 2 * tot[1] + tot[2];
    }
    __syncthreads();
    if (tid == 0) { sb.m.cnt[0] = newn; sb.m.cnt[1] = min(npt0 + pbase, sb.pt_cap); sb.m.cnt[2] = min(nobs0 + obase, sb.obs_cap); }
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_add(PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras,
                                                           ChainBuf cb, SlamBuf sb)
{
    slam_add_wg<false>(pb, kp_cap, p, F, max_norm, free_cameras, cb, sb);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_add_stream(PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras,
                                                                  ChainBuf cb, SlamBuf sb)
{
    slam_add_wg<true>(pb, kp_cap, p, F, max_norm, free_cameras, cb, sb);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_add_stream_restart(PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras,
                                                                          ChainBuf cb, SlamBuf sb)
{
    slam_add_wg<true, true>(pb, kp_cap, p, F, max_norm, free_cameras, cb, sb);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_add_seqs(PairBuf pb, int kp_cap, int j, int F, double max_norm, int free_cameras,
                                                                const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_add_wg<false>(chain_pairs_from(pb, q.first, kp_cap), kp_cap, j, F, max_norm, free_cameras, q.cb, q.sb);
}

void launch_slam_add_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, int F, double max_norm, int free_cameras, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_add_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, pb, kp_cap, j, F, max_norm, free_cameras, seqs);
}

// vo_slam_streams, step j: workgroup = sequence; one that is idle in this call (count = 0) or has ended returns at once
__global__ __launch_bounds__(SLAM_THREADS) void k_slam_add_stream_restart_seqs(PairBuf pb, int kp_cap, int j, int F, double max_norm, int free_cameras,
                                                                               const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_add_wg<true, true>(chain_pairs_from(pb, q.first, kp_cap), kp_cap, j, F, max_norm, free_cameras, q.cb, q.sb);
}

void launch_slam_add_stream_restart_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, int F, double max_norm, int free_cameras, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_add_stream_restart_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, pb, kp_cap, j, F, max_norm, free_cameras, seqs);
}

void launch_slam_add(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_add, dim3(1), dim3(SLAM_THREADS), 0, s, pb, kp_cap, p, F, max_norm, free_cameras, cb, sb);
}

void launch_slam_add_stream(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_add_stream, dim3(1), dim3(SLAM_THREADS), 0, s, pb, kp_cap, p, F, max_norm, free_cameras, cb, sb);
}

void launch_slam_add_stream_restart(hipStream_t s, PairBuf pb, int kp_cap, int p, int F, double max_norm, int free_cameras, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_add_stream_restart, dim3(1), dim3(SLAM_THREADS), 0, s, pb, kp_cap, p, F, max_norm, free_cameras, cb, sb);
}

// the problem k_bundle_adjust is handed: the map's place in the lists (all 0 for a single chain), its sizes, skip or not
__device__ __forceinline__ BaProblem slam_problem(const BaProblem& at, int ncam, int npt, int nobs, int nfree, int skip)
{
    return BaProblem{at.cam0, at.pt0, at.obs0, at.pair0, at.blk0, ncam, npt, nobs, nfree, skip};
}

// g2o's graph bookkeeping for the resident map — the lists the host loop of vo_bundle_adjust_batch builds, entry for entry:
// camera -> column of S, the observations sorted by point (stable in input order) with pt_first, and per block (c1 <= c2) of
// free cameras the (observation of c1, observation of c2) that share a point: blocks (0,0) (0,1) .. (F-1,F-1), within a block
// by point, then input order.
__device__ __forceinline__ void slam_ba_prepare_wg(ChainBuf cb, SlamBuf sb)
{
    __shared__ int s_w[SLAM_WAVES], s_col[VO_BA_MAX_CAMERAS], s_nfree, s_over;
    const int tid = threadIdx.x;
    const int ncam = sb.m.cnt[0], npt = sb.m.cnt[1], nobs = sb.m.cnt[2];
    if (!cb.alive[0] || ncam > VO_BA_MAX_CAMERAS) {
        if (tid == 0) sb.prob[0] = slam_problem(sb.base, 0, 0, 0, 0, 1);
        return;
    }
    if (tid == 0) {
        int f = 0;
        for (int i = 0; i < ncam; i++) { const int c = sb.m.cam_fixed[i] ? -1 : f++; s_col[i] = c; sb.cam_col[i] = c; }
        s_nfree = f; s_over = 0;
    }
    for (int q = tid; q < npt; q += SLAM_THREADS) sb.tmp[q] = 0;
    __syncthreads();
    const int nfree = s_nfree;
    for (int i = tid; i < nobs; i += SLAM_THREADS) atomicAdd(&sb.tmp[sb.m.obs_pt[i]], 1);
    __syncthreads();
    // pt_first; tmp becomes the points' fill cursors
    slam_scan(npt, s_w, [&](int q) { return sb.tmp[q]; }, [&](int q, int at, int) { sb.pt_first[q] = at; sb.tmp[q] = at; });
    if (tid == 0) sb.pt_first[npt] = nobs;
    __syncthreads();
    // every observation takes a slot of its point; the lane that owns the point then puts its slots in input order
    for (int i = tid; i < nobs; i += SLAM_THREADS) sb.idx[atomicAdd(&sb.tmp[sb.m.obs_pt[i]], 1)] = i;
    __syncthreads();
    for (int q = tid; q < npt; q += SLAM_THREADS) {
        const int j0 = sb.pt_first[q], j1 = sb.pt_first[q + 1];
        for (int a = j0 + 1; a < j1; a++) {
            const int v = sb.idx[a];
            int b = a - 1;
            while (b >= j0 && sb.idx[b] > v) { sb.idx[b + 1] = sb.idx[b]; b--; }
            sb.idx[b + 1] = v;
        }
    }
    __syncthreads();
    for (int j = tid; j < nobs; j += SLAM_THREADS) {
        const int i = sb.idx[j];
        sb.s_cam[j] = sb.m.obs_cam[i]; sb.s_pt[j] = sb.m.obs_pt[i];
        sb.s_xy[2 * (size_t)j] = sb.m.obs_xy[2 * (size_t)i]; sb.s_xy[2 * (size_t)j + 1] = sb.m.obs_xy[2 * (size_t)i + 1];
    }
    __syncthreads();
    // pair lists, block after block: a lane owns a point, the points' offsets inside a block are an ordered scan of their counts
    int base = 0, blk = 0;
    if (tid == 0) sb.blk_first[0] = 0;
    for (int a = 0; a < nfree; a++)
        for (int c = a; c < nfree; c++, blk++) {
            const int total = slam_scan(npt, s_w,
                [&](int q) {
                    int na = 0, nc = 0;
                    for (int j = sb.pt_first[q]; j < sb.pt_first[q + 1]; j++) { const int k = s_col[sb.s_cam[j]]; na += k == a; nc += k == c; }
                    return na * nc;
                },
                [&](int q, int at, int n) {
                    if (n == 0) return;
                    if (base + at + n > sb.pair_cap) { s_over = 1; return; }
                    int o = base + at;
                    for (int j1 = sb.pt_first[q]; j1 < sb.pt_first[q + 1]; j1++) {
                        if (s_col[sb.s_cam[j1]] != a) continue;
                        for (int j2 = sb.pt_first[q]; j2 < sb.pt_first[q + 1]; j2++)
                            if (s_col[sb.s_cam[j2]] == c) sb.pairs[o++] = make_int2(j1, j2);
                    }
                });
            base = min(base + total, sb.pair_cap);
            if (tid == 0) sb.blk_first[blk + 1] = base;
        }
    __syncthreads();
    if (tid == 0) {
        // (skipped: a pair list beyond its capacity — a point seen twice by one camera, which one-to-one matches exclude)
        sb.prob[0] = slam_problem(sb.base, ncam, npt, nobs, nfree, s_over || nfree > VO_BA_MAX_FREE);
    }
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_ba_prepare(ChainBuf cb, SlamBuf sb) { slam_ba_prepare_wg(cb, sb); }

// a sequence that has ended marks its problem skipped: k_bundle_adjust is launched for all S and must leave its map as it is
__global__ __launch_bounds__(SLAM_THREADS) void k_slam_ba_prepare_seqs(int j, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) {
        if (threadIdx.x == 0) q.sb.prob[0] = slam_problem(q.sb.base, 0, 0, 0, 0, 1);
        return;
    }
    slam_ba_prepare_wg(q.cb, q.sb);
}

void launch_slam_ba_prepare_seqs(hipStream_t s, int j, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_ba_prepare_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, j, seqs);
}

void launch_slam_ba_prepare(hipStream_t s, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_ba_prepare, dim3(1), dim3(SLAM_THREADS), 0, s, cb, sb);
}

__device__ __forceinline__ int slam_slot_of(const PairBuf& pb, int chain_frame)
{
    return chain_frame == 0 ? pb.slots[0] : pb.slots[2 * (chain_frame - 1) + 1];
}

// What optimize_map wrote back (map.py:175-186) reaches the tables the next pair's k_chain_gather / k_chain_pose read; then
// remove_observations_with_reprojection_errors_above_threshold (map.py:46-70) with k_reprojection's arithmetic, the list
// compacted in place and in order.  Points are not removed here: one that loses every observation stays usable for PnP.
// vo_slam_stream: a camera of an earlier call has no slot any more (its frame lies before frame0), and a point whose key was
// marked none by k_slam_carry has no row in the slot-keyed tables: neither is written back.
template <bool ST>
__device__ __forceinline__ void slam_filter_wg(PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    __shared__ int s_w[SLAM_WAVES];
    if (!cb.alive[0]) return;
    const int tid = threadIdx.x;
    const int ncam = sb.m.cnt[0], npt = sb.m.cnt[1], nobs = sb.m.cnt[2];
    for (int k = tid; k < ncam * 12; k += SLAM_THREADS) {
        const int fr = sb.m.cam_frame[k / 12] - (ST ? sb.st.frame0 : 0);
        if (ST && fr < 0) continue;
        cb.cam[(size_t)slam_slot_of(pb, fr) * 12 + k % 12] = sb.m.cam_pose[k];
    }
    for (int q = tid; q < npt; q += SLAM_THREADS) {
        const int key = sb.m.pt_key[q];
        if (ST && key < 0) continue;
        for (int a = 0; a < 3; a++) cb.map_pt[3 * (size_t)key + a] = sb.m.pt_xyz[3 * (size_t)q + a];
    }
    if (!(threshold > 0)) return;
    int ci = 0, pi = 0; double u = 0, v = 0;
    const int kept = slam_scan(nobs, s_w,
        [&](int i) {
            ci = sb.m.obs_cam[i]; pi = sb.m.obs_pt[i]; u = sb.m.obs_xy[2 * (size_t)i]; v = sb.m.obs_xy[2 * (size_t)i + 1];
            return reprojection_sqerr_one(sb.m.cam_pose + 12 * (size_t)ci, sb.m.pt_xyz + 3 * (size_t)pi, Kd, u, v) < threshold ? 1 : 0;
        },
        [&](int, int at, int keep) {
            if (!keep) return;
            sb.m.obs_cam[at] = ci; sb.m.obs_pt[at] = pi; sb.m.obs_xy[2 * (size_t)at] = u; sb.m.obs_xy[2 * (size_t)at + 1] = v;
        });
    __syncthreads();
    if (tid == 0) sb.m.cnt[2] = kept;
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_filter(PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    slam_filter_wg<false>(pb, Kd, threshold, cb, sb);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_filter_stream(PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    slam_filter_wg<true>(pb, Kd, threshold, cb, sb);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_filter_stream_restart(PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    if (cb.rs.st[SEG_INIT]) threshold = 0.0;                       // (a pair that starts a new segment is step 0 of it)
    slam_filter_wg<true>(pb, Kd, threshold, cb, sb);
}

// (threshold is the step's: 0 at step 0, where initialize_map's optimize_map is only written back)
__global__ __launch_bounds__(SLAM_THREADS) void k_slam_filter_seqs(PairBuf pb, int kp_cap, int j, const double* Kd, double threshold,
                                                                   const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    if (q.cb.rs.st && q.cb.rs.st[SEG_INIT]) threshold = 0.0;       // (a pair that starts a new segment is step 0 of it)
    slam_filter_wg<false>(chain_pairs_from(pb, q.first, kp_cap), Kd, threshold, q.cb, q.sb);
}

void launch_slam_filter_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const double* Kd, double threshold, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_filter_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, pb, kp_cap, j, Kd, threshold, seqs);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_filter_stream_restart_seqs(PairBuf pb, int kp_cap, int j, const double* Kd, double threshold,
                                                                                  const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    if (q.cb.rs.st[SEG_INIT]) threshold = 0.0;                     // (a pair that starts a new segment is step 0 of it)
    slam_filter_wg<true>(chain_pairs_from(pb, q.first, kp_cap), Kd, threshold, q.cb, q.sb);
}

void launch_slam_filter_stream_restart_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const double* Kd, double threshold, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_filter_stream_restart_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, pb, kp_cap, j, Kd, threshold, seqs);
}

void launch_slam_filter(hipStream_t s, PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_filter, dim3(1), dim3(SLAM_THREADS), 0, s, pb, Kd, threshold, cb, sb);
}

void launch_slam_filter_stream(hipStream_t s, PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_filter_stream, dim3(1), dim3(SLAM_THREADS), 0, s, pb, Kd, threshold, cb, sb);
}

void launch_slam_filter_stream_restart(hipStream_t s, PairBuf pb, const double* Kd, double threshold, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_filter_stream_restart, dim3(1), dim3(SLAM_THREADS), 0, s, pb, Kd, threshold, cb, sb);
}

// The archive's part of k_slam_limit_stream_archive (docs/kernels/k_stream_archive.md).  slam_archive_entry: entry e of the archive
// from what the limit's scan holds for a removed point.  has_row takes the source of the row until slam_archive_rows has copied it:
// 1 + key — row `key` of the slots' descriptors (the point was born in this call, its frame is in its slot); -1 - r — row r of the
// descriptor store (a point of an earlier call); 0 — none (the store dropped the point at capacity).
__device__ __forceinline__ void slam_archive_entry(const SlamArchive& ar, int e, int key, int ff, int fk, const double* X, int frame0, int p)
{
    if (e < 0 || e >= ar.a.capacity) return;                   // a full archive: the point is dropped, for good
    int src = 0;
    if (ff >= frame0 && key >= 0 && key < ar.n_keys) src = 1 + key;
    else if (ff >= 0 && ff < ar.frames && fk >= 0 && fk < ar.kp_cap) {
        const int r = ar.feat_row[(size_t)ff * ar.kp_cap + fk];
        if (r >= 0 && r < ar.store_cap) src = -1 - r;
    }
    ar.a.feature[2 * (size_t)e] = ff; ar.a.feature[2 * (size_t)e + 1] = fk;
    for (int a = 0; a < 3; a++) ar.a.xyz[3 * (size_t)e + a] = X[a];
    ar.a.evicted_at[e] = frame0 + p;
    ar.a.has_row[e] = src;
}

// ... then, behind a barrier: the rows of the nrem points this limit removed, entries cnt0 .. of the archive as far as it has room,
// 16 bytes per lane (2 lanes move an ORB row, 8 a SIFT row: k_stream_rows_append's copy); has_row becomes 0 / 1; lane 0 advances
// the two counters.  Plain vector loads and stores; the one workgroup of the limit, so no other reads or writes the archive.
__device__ __forceinline__ void slam_archive_rows(const SlamArchive& ar, int cnt0, int nrem)
{
    __shared__ int s_src[SLAM_THREADS];
    const int tid = threadIdx.x, D = ar.a.D, lsh = D == 128 ? 3 : 1;
    const int n = min(nrem, max(ar.a.capacity - cnt0, 0));
    for (int e0 = 0; e0 < n; e0 += SLAM_THREADS) {
        const int e = e0 + tid;
        int src = 0;
        if (e < n) { src = ar.a.has_row[cnt0 + e]; ar.a.has_row[cnt0 + e] = src != 0 ? 1 : 0; }
        s_src[tid] = src;
        __syncthreads();
        for (int k = tid; k < (SLAM_THREADS << lsh); k += SLAM_THREADS) {
            const int i = k >> lsh, part = k & ((1 << lsh) - 1), sr = s_src[i];
            if (sr == 0) continue;                             // (past n, or no row: the archive's row stays zero)
            const uint8_t* from = sr > 0 ? ar.desc + (size_t)(sr - 1) * D : ar.store_rows + (size_t)(-1 - sr) * D;
            *(uint4*)(ar.a.rows + (size_t)(cnt0 + e0 + i) * D + 16 * part) = *(const uint4*)(from + 16 * part);
        }
        __syncthreads();
    }
    if (tid == 0) { ar.a.counters[0] = cnt0 + n; ar.a.counters[1] += nrem - n; }
}

// limit_number_of_camera_in_map (map.py:299-318): with more than max_cameras cameras, remove_camera_from_map(cameras[0])
// (:188-232) with the quirk it has — observations are counted per point AMONG POINTS THAT STILL HAVE ONE (a defaultdict), so a
// point left with one observation goes and a point with none stays.  A removed point leaves mappointdict: its feature id can
// receive a new point later.  Camera and point indices in the observations are renumbered.  Also the end of a pair: every
// camera's pose as the map holds it goes to poses_last (an evicted camera keeps its last row), the map's sizes to n_*.
// vo_slam_stream: poses_last has the call's rows only; a camera of an earlier call reports to its carried row instead.  A point
// whose key is none (k_slam_carry) has no entry in pt_of / in_map; pt_feat moves with pt_key.
// RS (vo_slam_stream_restart): row 0 of a resumed call is the anchor's, never the first camera of a segment that starts at its pair 0;
// SEG_FIRST names a pair of this call or none (k_slam_carry_restart), so a segment's first camera of an earlier call is a carried one.
// AR (vo_set_stream_archive; k_slam_limit_stream_archive alone): every point removed here is appended to the stream's archive, in
// map order — its feature, the coordinates read here and the pair, then a copy of its descriptor row (slam_archive_rows).  A removed
// point's rank among the removed is q - at; its entry is count-before + rank, and an entry at or past the capacity is dropped.
template <bool ST, bool RS = false, bool AR = false>
__device__ __forceinline__ void slam_limit_wg(int p, int max_cameras, ChainBuf cb, SlamBuf sb, const SlamArchive* ar = nullptr)
{
    __shared__ int s_w[SLAM_WAVES];
    const int tid = threadIdx.x;
    int ncam = sb.m.cnt[0], npt = sb.m.cnt[1], nobs = sb.m.cnt[2];
    if (cb.alive[0]) {
        // (vo_slam_chains_restart: pose row `first pair of the segment` belongs to the segment before; the first camera has its own)
        const int seg0 = cb.rs.st ? cb.rs.st[SEG_FIRST] : -1;
        for (int k = tid; k < ncam * 12; k += SLAM_THREADS) {
            int fr = sb.m.cam_frame[k / 12];
            if (ST) {
                fr -= sb.st.frame0;
                if (fr < 0) {
                    for (int j = 0; j < sb.st.n_carried; j++)
                        if (sb.st.carried_frame[j] == fr + sb.st.frame0) sb.st.carried_poses[(size_t)j * 12 + k % 12] = sb.m.cam_pose[k];
                    continue;
                }
            }
            if (fr == seg0) cb.rs.seg_poses_last[(size_t)fr * 12 + k % 12] = sb.m.cam_pose[k];
            if (fr != seg0 || (fr == 0 && (!RS || sb.st.frame0 == 0))) sb.poses_last[(size_t)fr * 12 + k % 12] = sb.m.cam_pose[k];
        }
        if (ncam > max_cameras) {
            for (int q = tid; q < npt; q += SLAM_THREADS) sb.tmp[q] = 0;
            __syncthreads();
            for (int i = tid; i < nobs; i += SLAM_THREADS) if (sb.m.obs_cam[i] != 0) atomicAdd(&sb.tmp[sb.m.obs_pt[i]], 1);
            __syncthreads();
            // the points, in order; tmp becomes old index -> new index (-1: removed)
            int key = 0, ff = 0, fk = 0; double X[3] = {0, 0, 0};
            int acnt0 = 0;
            if constexpr (AR) acnt0 = ar->a.counters[0];
            const int npt2 = slam_scan(npt, s_w,
                [&](int q) {
                    key = sb.m.pt_key[q]; for (int a = 0; a < 3; a++) X[a] = sb.m.pt_xyz[3 * (size_t)q + a];
                    if (ST) { ff = sb.m.pt_feat[2 * (size_t)q]; fk = sb.m.pt_feat[2 * (size_t)q + 1]; }
                    return sb.tmp[q] != 1 ? 1 : 0;
                },
                [&](int q, int at, int keep) {
                    const bool keyed = !ST || key >= 0;
                    if constexpr (AR) if (!keep) slam_archive_entry(*ar, acnt0 + (q - at), key, ff, fk, X, sb.st.frame0, p);
                    if (!keep) { sb.tmp[q] = -1; if (keyed) { sb.pt_of[key] = 0; cb.in_map[key] = 0; } return; }
                    sb.tmp[q] = at; if (keyed) sb.pt_of[key] = at + 1; sb.m.pt_key[at] = key;
                    if (ST) { sb.m.pt_feat[2 * (size_t)at] = ff; sb.m.pt_feat[2 * (size_t)at + 1] = fk; }
                    for (int a = 0; a < 3; a++) sb.m.pt_xyz[3 * (size_t)at + a] = X[a];
                });
            __syncthreads();
            if constexpr (AR) slam_archive_rows(*ar, acnt0, npt - npt2);
            int ci = 0, pi = 0; double u = 0, v = 0;
            const int nobs2 = slam_scan(nobs, s_w,
                [&](int i) {
                    ci = sb.m.obs_cam[i]; pi = sb.tmp[sb.m.obs_pt[i]]; u = sb.m.obs_xy[2 * (size_t)i]; v = sb.m.obs_xy[2 * (size_t)i + 1];
                    return ci != 0 && pi >= 0 ? 1 : 0;
                },
                [&](int, int at, int keep) {
                    if (!keep) return;
                    sb.m.obs_cam[at] = ci - 1; sb.m.obs_pt[at] = pi; sb.m.obs_xy[2 * (size_t)at] = u; sb.m.obs_xy[2 * (size_t)at + 1] = v;
                });
            // the camera list moves up by one
            double T[12]; int fr = 0; uint8_t fx = 0;
            const bool mv = tid + 1 < ncam;
            if (mv) { for (int k = 0; k < 12; k++) T[k] = sb.m.cam_pose[(size_t)(tid + 1) * 12 + k]; fr = sb.m.cam_frame[tid + 1]; fx = sb.m.cam_fixed[tid + 1]; }
            __syncthreads();
            if (mv) { for (int k = 0; k < 12; k++) sb.m.cam_pose[(size_t)tid * 12 + k] = T[k]; sb.m.cam_frame[tid] = fr; sb.m.cam_fixed[tid] = fx; }
            ncam--; npt = npt2; nobs = nobs2;
            __syncthreads();
            if (tid == 0) { sb.m.cnt[0] = ncam; sb.m.cnt[1] = npt; sb.m.cnt[2] = nobs; }
        }
    }
    if (tid == 0) { sb.n_cam[p] = ncam; sb.n_pts[p] = npt; sb.n_obs[p] = nobs; }
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_limit(int p, int max_cameras, ChainBuf cb, SlamBuf sb) { slam_limit_wg<false>(p, max_cameras, cb, sb); }

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_limit_stream(int p, int max_cameras, ChainBuf cb, SlamBuf sb) { slam_limit_wg<true>(p, max_cameras, cb, sb); }

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_limit_stream_restart(int p, int max_cameras, ChainBuf cb, SlamBuf sb) { slam_limit_wg<true, true>(p, max_cameras, cb, sb); }

// vo_slam_stream with an archive: k_slam_limit_stream that also appends what it removes
__global__ __launch_bounds__(SLAM_THREADS) void k_slam_limit_stream_archive(int p, int max_cameras, ChainBuf cb, SlamBuf sb, SlamArchive ar)
{
    slam_limit_wg<true, false, true>(p, max_cameras, cb, sb, &ar);
}

void launch_slam_limit_stream_archive(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb, SlamArchive ar)
{
    hipLaunchKernelGGL(k_slam_limit_stream_archive, dim3(1), dim3(SLAM_THREADS), 0, s, p, max_cameras, cb, sb, ar);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_limit_seqs(int j, int max_cameras, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_limit_wg<false>(j, max_cameras, q.cb, q.sb);
}

void launch_slam_limit_seqs(hipStream_t s, int j, int max_cameras, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_limit_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, j, max_cameras, seqs);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_limit_stream_restart_seqs(int j, int max_cameras, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_limit_wg<true, true>(j, max_cameras, q.cb, q.sb);
}

void launch_slam_limit_stream_restart_seqs(hipStream_t s, int j, int max_cameras, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_limit_stream_restart_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, j, max_cameras, seqs);
}

void launch_slam_limit(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_limit, dim3(1), dim3(SLAM_THREADS), 0, s, p, max_cameras, cb, sb);
}

void launch_slam_limit_stream(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_limit_stream, dim3(1), dim3(SLAM_THREADS), 0, s, p, max_cameras, cb, sb);
}

void launch_slam_limit_stream_restart(hipStream_t s, int p, int max_cameras, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_limit_stream_restart, dim3(1), dim3(SLAM_THREADS), 0, s, p, max_cameras, cb, sb);
}

// vo_slam_chains_restart, between k_chain_pose and k_chain_triangulate of every step: the end of the step's decision.  On an
// initial step (SEG_INIT: k_chain_gather met a good pair while the sequence was lost, or k_chain_pose a failed solvePnPRansac)
// the pair starts a new segment — initialize_map's self.map.clean() (src/visual_slam.py:43-45): the lists restart at length 0
// and every point's feature id leaves mappointdict (pt_of, in_map); the first frame's feature_mapper row is cleared, so no
// track reaches behind the segment; then initialize_map on this pair (chain_init_wg).  Every pair gets its segment here.
// ST (vo_slam_stream_restart): a point whose key k_slam_carry marked none (-1) has no entry to clear and is skipped; a key in a
// ghost row is cleared like any other (pt_of and in_map have the ghost rows).  The state words come from the call before, so the
// segments count along the stream; in a resumed call pose row 0 stays the anchor's (chain_init_wg, row0).
template <bool ST>
__device__ __forceinline__ void slam_restart_wg(PairBuf pb, int kp_cap, int p, ChainBuf cb, SlamBuf sb)
{
    const int tid = threadIdx.x;
    const int init = cb.rs.st[SEG_INIT], nseg = cb.rs.st[SEG_COUNT], cause = cb.rs.st[SEG_CAUSE], npt = sb.m.cnt[1];
    if (!init) {
        if (tid == 0) cb.rs.segment[p] = cb.alive[0] ? nseg - 1 : -1;
        return;
    }
    for (int q = tid; q < npt; q += SLAM_THREADS) {
        const int key = sb.m.pt_key[q];
        if (ST && key < 0) continue;
        sb.pt_of[key] = 0; cb.in_map[key] = 0;
    }
    unsigned long long* row = cb.parent + chain_key(pb.slots[2 * p], 0, kp_cap);
    for (int i = tid; i < kp_cap; i += SLAM_THREADS) row[i] = 0;
    __syncthreads();                                           // every lane has read the state words and the old point count
    if (tid == 0) {
        sb.m.cnt[0] = 0; sb.m.cnt[1] = 0; sb.m.cnt[2] = 0;
        cb.rs.st[SEG_FIRST] = p; cb.rs.st[SEG_COUNT] = nseg + 1; cb.rs.st[SEG_CAUSE] = 0;
        cb.rs.segment[p] = nseg; cb.rs.cause[p] = cause;
    }
    chain_init_wg(pb, kp_cap, cb, p, !ST || sb.st.frame0 == 0);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_restart_seqs(PairBuf pb, int kp_cap, int j, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_restart_wg<false>(chain_pairs_from(pb, q.first, kp_cap), kp_cap, j, q.cb, q.sb);
}

void launch_slam_restart_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_restart_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, pb, kp_cap, j, seqs);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_restart_stream(PairBuf pb, int kp_cap, int p, ChainBuf cb, SlamBuf sb)
{
    slam_restart_wg<true>(pb, kp_cap, p, cb, sb);
}

void launch_slam_restart_stream(hipStream_t s, PairBuf pb, int kp_cap, int p, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_restart_stream, dim3(1), dim3(SLAM_THREADS), 0, s, pb, kp_cap, p, cb, sb);
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_restart_stream_seqs(PairBuf pb, int kp_cap, int j, const SlamSeq* __restrict__ seqs)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_restart_wg<true>(chain_pairs_from(pb, q.first, kp_cap), kp_cap, j, q.cb, q.sb);
}

void launch_slam_restart_stream_seqs(hipStream_t s, PairBuf pb, int kp_cap, int j, const SlamSeq* seqs, int S)
{
    hipLaunchKernelGGL(k_slam_restart_stream_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, pb, kp_cap, j, seqs);
}

// vo_slam_stream, at the start of a call that continues the map of the call before (before k_chain_link): the frames of that call
// lose their slots, so every key that still matters is restated in rows that stay.  Integers and copies only; one workgroup, its
// phases separated by barriers; the result is a function of the tables alone (a lane owns a keypoint, a point or a table entry).
//   A  every keypoint k of the anchor row — the stream's last frame, the only one a later track can pass through — walks to its
//      track root on the old table.  A root other than (anchor, k) itself moves to entry k of the new ghost row: parent[(anchor, k)]
//      names it, it takes the root's pt_of / in_map / map_pt, and the point the root owns is re-keyed.  A root that owns no point
//      moves as well: left as its own root, the anchor keypoint would own the first point a later pair keys there and later
//      pairs would find it, where the one-call walk finds the old, empty root every time and adds a new point (:139-146).
//      The old ghost row is read here (a root of the call before last), the new one written: two rows, alternating.
//   B  a point keyed neither in the anchor row nor in the new ghost row can never be reached again: its key becomes none (-1).
//      (Its feature id for vo_slam_map was stored in pt_feat when it was added.)  The cameras beside the anchor go to the carried rows.
//   C  every row but the anchor's and the new ghost's is cleared in parent, in_map, map_pt, pt_of, cam and cam_ok: a reused slot
//      starts empty, as every slot does in a single call.
// RS (vo_slam_stream_restart): after a call that ended lost the anchor frame is not in the map — every camera is a carried one, no
// track starts in the anchor row (its pair failed) and every point loses its key, which is all the map needs to be kept for
// vo_slam_map until a usable pair restarts it.  SEG_FIRST is an index into the pairs of the call before: it becomes none (-1).
// SQ (vo_slam_streams): the tables are shared with other sequences, whose workgroups carry their own maps in the same launch.  This
// sequence's tracks and keys live in its anchor row, its two ghost rows and the rows of the slots its last call's frames had; step C
// clears exactly those of them that are not kept — rows[0 .. n_rows - 1] — and a walk is bounded by all the rows of the table (hops).
template <bool RS, bool SQ = false>
__device__ __forceinline__ void slam_carry_wg(SlamCarry c, ChainBuf cb, SlamBuf sb, int hops = 0, const int* rows = nullptr, int n_rows = 0)
{
    const int tid = threadIdx.x, cap = c.kp_cap;
    const int ncam = sb.m.cnt[0], npt = sb.m.cnt[1];
    const int ncar = RS && !cb.alive[0] ? ncam : ncam - 1;
    for (int k = tid; k < cap; k += SLAM_THREADS) {
        int rf = c.anchor, ri = k;
        chain_root(cb.parent, cap, SQ ? hops : c.F + 2, rf, ri);
        const size_t g = chain_key(c.ghost_new, k, cap);
        int own = 0; uint8_t in = 0; double X[3] = {0, 0, 0};
        if (rf != c.anchor) {                                   // (a root in the anchor row is the keypoint itself: tracks are one-to-one)
            const size_t r = chain_key(rf, ri, cap);
            own = sb.pt_of[r]; in = cb.in_map[r];
            for (int a = 0; a < 3; a++) X[a] = cb.map_pt[3 * r + a];
            if (own) sb.m.pt_key[own - 1] = (int)g;
            cb.parent[chain_key(c.anchor, k, cap)] = (1ULL << 40) | ((unsigned long long)(unsigned)c.ghost_new << 20) | (unsigned)k;
        }
        sb.pt_of[g] = own; cb.in_map[g] = in; cb.parent[g] = 0;
        for (int a = 0; a < 3; a++) cb.map_pt[3 * g + a] = X[a];
    }
    if (tid < 12) cb.poses[tid] = c.keep[tid];
    else if (tid < 24) sb.poses_last[tid - 12] = c.keep[tid];
    for (int k = tid; k < ncar * 12; k += SLAM_THREADS) sb.st.carried_poses[k] = sb.m.cam_pose[k];
    for (int i = tid; i < ncar; i += SLAM_THREADS) sb.st.carried_frame[i] = sb.m.cam_frame[i];
    if (RS && tid == 0) cb.rs.st[SEG_FIRST] = -1;
    __syncthreads();
    for (int q = tid; q < npt; q += SLAM_THREADS) {
        const int key = sb.m.pt_key[q];
        if (key < 0) continue;
        const int row = key / cap;
        if (row != c.anchor && row != c.ghost_new) sb.m.pt_key[q] = -1;
    }
    if (SQ) {
        for (int n = 0; n < n_rows; n++) {
            const int r = rows[n];
            const size_t at = chain_key(r, 0, cap);
            for (int k = tid; k < cap; k += SLAM_THREADS) { cb.parent[at + k] = 0; cb.in_map[at + k] = 0; sb.pt_of[at + k] = 0; }
            for (int k = tid; k < 3 * cap; k += SLAM_THREADS) cb.map_pt[3 * at + k] = 0.0;
            if (r < c.F) {                                          // a frame slot: its camera goes too; a ghost row has none
                if (tid < 12) cb.cam[(size_t)r * 12 + tid] = 0.0;
                if (tid == 0) cb.cam_ok[r] = 0;
            }
        }
        return;
    }
    for (int r = 0; r < c.F + 2; r++) {
        if (r == c.anchor || r == c.ghost_new) continue;
        const size_t at = chain_key(r, 0, cap);
        for (int k = tid; k < cap; k += SLAM_THREADS) { cb.parent[at + k] = 0; cb.in_map[at + k] = 0; sb.pt_of[at + k] = 0; }
        for (int k = tid; k < 3 * cap; k += SLAM_THREADS) cb.map_pt[3 * at + k] = 0.0;
    }
    for (int k = tid; k < c.F * 12; k += SLAM_THREADS) if (k / 12 != c.anchor) cb.cam[k] = 0.0;
    for (int r = tid; r < c.F; r += SLAM_THREADS) if (r != c.anchor) cb.cam_ok[r] = 0;
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_carry(SlamCarry c, ChainBuf cb, SlamBuf sb) { slam_carry_wg<false>(c, cb, sb); }

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_carry_restart(SlamCarry c, ChainBuf cb, SlamBuf sb) { slam_carry_wg<true>(c, cb, sb); }

void launch_slam_carry(hipStream_t s, SlamCarry c, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_carry, dim3(1), dim3(SLAM_THREADS), 0, s, c, cb, sb);
}

void launch_slam_carry_restart(hipStream_t s, SlamCarry c, ChainBuf cb, SlamBuf sb)
{
    hipLaunchKernelGGL(k_slam_carry_restart, dim3(1), dim3(SLAM_THREADS), 0, s, c, cb, sb);
}

// vo_slam_streams: every sequence of the stream is carried at the start of every resumed call, also one that is idle in it (a
// carry of a carried map moves the ghost entries to the other ghost row and changes nothing else), so after the launch a
// sequence holds its anchor row and one ghost row and every other slot is free for any sequence.
__global__ __launch_bounds__(SLAM_THREADS) void k_slam_carry_restart_seqs(const SlamSeq* __restrict__ seqs, const SlamSeqCarry* __restrict__ car)
{
    const SlamSeq& q = seqs[blockIdx.x];
    const SlamSeqCarry& c = car[blockIdx.x];
    slam_carry_wg<true, true>(c.c, q.cb, q.sb, c.hops, c.rows, c.n_rows);
}

void launch_slam_carry_restart_seqs(hipStream_t s, const SlamSeq* seqs, const SlamSeqCarry* car, int S)
{
    hipLaunchKernelGGL(k_slam_carry_restart_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, seqs, car);
}

// vo_slam_streams with seats (vo_slam_streams_replace, vo_slam_streams_open): the carry launch of a call in which some seat is
// vacant.  A seat whose flight goes on is carried by the body above.  A seat that was replaced since the last call is reset here,
// before k_chain_link: other sequences may already have frames in the slots it gives up, and the flight that takes the seat — in
// this call or a later one — must find what a stream's first call finds after its memset.  Integers and zeros only:
//   the rows only this seat held — the slots of its last call's frames (car.rows), its old anchor row and BOTH its ghost rows
//   (seat.rows) — are cleared in parent, in_map, pt_of, map_pt, and a frame slot's camera with them, as step C clears a row;
//   the three list lengths, alive, map_count, the four segment state words and the seat's kept anchor camera become 0: the
//   sequence is lost with nothing to report, so the next usable pair is an initial step that numbers its segment 0, cause 0.
// The lists' tails, pt_feat, tmp and the bundle adjustment's buffers keep their old bytes: every kernel writes an entry of them
// before it reads it (k_slam_restart_stream starts maps on such lists in every stream that loses a frame).
// A seat that is vacant and was reset in an earlier call (or has been vacant since vo_slam_streams_open) returns at once.
__device__ __forceinline__ void slam_seat_clear_row(int r, int F, int cap, ChainBuf cb, SlamBuf sb)
{
    const int tid = threadIdx.x;
    const size_t at = chain_key(r, 0, cap);
    for (int k = tid; k < cap; k += SLAM_THREADS) { cb.parent[at + k] = 0; cb.in_map[at + k] = 0; sb.pt_of[at + k] = 0; }
    for (int k = tid; k < 3 * cap; k += SLAM_THREADS) cb.map_pt[3 * at + k] = 0.0;
    if (r < F) {
        if (tid < 12) cb.cam[(size_t)r * 12 + tid] = 0.0;
        if (tid == 0) cb.cam_ok[r] = 0;
    }
}

__device__ __forceinline__ void slam_seat_reset_wg(const SlamSeqCarry& c, const SlamSeat& t, ChainBuf cb, SlamBuf sb)
{
    const int tid = threadIdx.x, cap = c.c.kp_cap, F = c.c.F;
    for (int n = 0; n < c.n_rows; n++) slam_seat_clear_row(c.rows[n], F, cap, cb, sb);
    for (int n = 0; n < t.n_rows; n++) slam_seat_clear_row(t.rows[n], F, cap, cb, sb);
    if (tid < 4) { sb.m.cnt[tid] = 0; cb.rs.st[tid] = 0; }
    if (tid < 24) t.keep[tid] = 0.0;
    if (tid == 0) { cb.alive[0] = 0; cb.map_count[0] = 0; }
}

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_carry_restart_seats(const SlamSeq* __restrict__ seqs, const SlamSeqCarry* __restrict__ car,
                                                                           const SlamSeat* __restrict__ seats)
{
    const SlamSeq& q = seqs[blockIdx.x];
    const SlamSeqCarry& c = car[blockIdx.x];
    const SlamSeat& t = seats[blockIdx.x];
    if (t.mode == SEAT_VACANT) return;
    if (t.mode == SEAT_RESET) { slam_seat_reset_wg(c, t, q.cb, q.sb); return; }
    slam_carry_wg<true, true>(c.c, q.cb, q.sb, c.hops, c.rows, c.n_rows);
}

void launch_slam_carry_restart_seats(hipStream_t s, const SlamSeq* seqs, const SlamSeqCarry* car, const SlamSeat* seats, int S)
{
    hipLaunchKernelGGL(k_slam_carry_restart_seats, dim3(S), dim3(SLAM_THREADS), 0, s, seqs, car, seats);
}

// show_map_statistics (src/map.py:234-297) of the map as it stands: calculate_reprojection_error's total (:72-97), the largest term
// and the number of "high" ones (:92), the points by number of observations (:245-254, with bin 0 for the points the reference's
// defaultdict never sees) and show_observation_matrix (:267-297).  The map is only read; one row of out is written.
// The total is the one floating-point sum of this file and its order is the contract: the terms are added one after the other in
// observation order, from 0.0, by lane 0 — all lanes put a round's 256 terms (reprojection_sqerr_one, the expression k_slam_filter
// uses) into one of two LDS buffers, and after the barrier lane 0 adds that round while every lane fills the other buffer with the
// next one.  Everything else is free of order: the maximum (a NaN never wins: e > m) and the count per lane, then per wave
// (shuffles), then over the waves in wave order; the grouping by point as k_slam_ba_prepare does it — integer atomics count,
// an ordered scan turns the counts into cursors, an atomic cursor hands out slots — but unsorted and in scratch of the kernel's
// own: what a slot holds is its observation's camera, and the histogram and the matrix do not depend on the order of a point's slots.
// The lane that owns a point adds it to its bin (LDS atomic); every pair of its slots with two different cameras adds 1 to the matrix.
// An observation that names no camera or point of the lists is not dereferenced: it is skipped and flagged (vo_map_statistics
// reports it; a resident map has none).  pt0, obs0: where the map's ranges of the scratch start.
__device__ __forceinline__ void slam_stats_wg(SlamMap m, int pt0, int obs0, int row, StatsBuf out)
{
    __shared__ int s_mat[VO_BA_MAX_CAMERAS * VO_BA_MAX_CAMERAS], s_hist[VO_STATS_HIST], s_w[SLAM_WAVES], s_nh[SLAM_WAVES];
    __shared__ double s_err[2][SLAM_THREADS], s_mx[SLAM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ncam = m.cnt[0], npt = m.cnt[1], nobs = m.cnt[2], C = out.C;
    if (ncam > C || C > VO_BA_MAX_CAMERAS) {                    // cannot happen: the host sizes the rows from max_cameras
        if (tid == 0) out.bad[0] = 1;
        return;
    }
    int* cur = out.pt_cur + pt0;
    int* slot = out.slot + obs0;
    for (int k = tid; k < VO_BA_MAX_CAMERAS * VO_BA_MAX_CAMERAS; k += SLAM_THREADS) s_mat[k] = 0;
    if (tid < VO_STATS_HIST) s_hist[tid] = 0;
    for (int q = tid; q < npt; q += SLAM_THREADS) cur[q] = 0;
    __syncthreads();

    double total = 0.0, mx = 0.0;                               // (total: lane 0's)
    int nh = 0;
    const int rounds = (nobs + SLAM_THREADS - 1) / SLAM_THREADS;
    for (int b = 0; b <= rounds; b++) {
        if (b < rounds) {
            const int i = b * SLAM_THREADS + tid;
            double e = 0.0;
            if (i < nobs) {
                const int ci = m.obs_cam[i], pi = m.obs_pt[i];
                if ((unsigned)ci < (unsigned)ncam && (unsigned)pi < (unsigned)npt) {
                    e = reprojection_sqerr_one(m.cam_pose + 12 * (size_t)ci, m.pt_xyz + 3 * (size_t)pi, out.Kd, m.obs_xy[2 * (size_t)i], m.obs_xy[2 * (size_t)i + 1]);
                    if (e > mx) mx = e;
                    nh += e > out.high ? 1 : 0;
                    atomicAdd(&cur[pi], 1);
                } else out.bad[0] = 1;
            }
            s_err[b & 1][tid] = e;
        }
        if (tid == 0 && b > 0) {
            const double* v = s_err[(b - 1) & 1];
            const int n = min(SLAM_THREADS, nobs - (b - 1) * SLAM_THREADS);
            // 16 terms at a time: their LDS reads are issued together, so that the add chain waits for one read latency per 16
            // terms and not per term; the adds stay one after the other, in index order
            int k = 0;
            for (; k + 16 <= n; k += 16) {
                double r[16];
#pragma unroll
                for (int j = 0; j < 16; j++) r[j] = v[k + j];
#pragma unroll
                for (int j = 0; j < 16; j++) total += r[j];
            }
            for (; k < n; k++) total += v[k];
        }
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) {
        nh += __shfl_down(nh, d);
        const double o = __shfl_down(mx, d);
        if (o > mx) mx = o;
    }
    if (lane == 0) { s_nh[wave] = nh; s_mx[wave] = mx; }

    // counts -> cursors; after the slots are handed out a point's cursor is the end of its slots, the point before it gives the start
    slam_scan(npt, s_w, [&](int q) { return cur[q]; }, [&](int q, int at, int) { cur[q] = at; });
    __syncthreads();
    for (int i = tid; i < nobs; i += SLAM_THREADS) {
        const int ci = m.obs_cam[i], pi = m.obs_pt[i];
        if ((unsigned)ci < (unsigned)ncam && (unsigned)pi < (unsigned)npt) slot[atomicAdd(&cur[pi], 1)] = ci;
    }
    __syncthreads();
    // A lane owns a point and reads its slots once, into a mask of the cameras that see it.  A point no camera sees twice adds 1 at
    // every pair of its cameras: such a cell is counted over the wave's 64 points at once (a ballot per cell, one LDS add by lane
    // 0).  A point some camera sees twice (the dead-rooted track) walks the pairs of its slots on its own and leaves the ballots.
    for (int b = 0; b < npt; b += SLAM_THREADS) {               // (uniform trip count: there are ballots inside)
        const int q = b + tid;
        unsigned long long seen = 0;
        bool twice = false;
        int j0 = 0, j1 = 0;
        if (q < npt) {
            j0 = q > 0 ? cur[q - 1] : 0; j1 = cur[q];
            for (int a = j0; a < j1; a++) { const unsigned long long bit = 1ULL << slot[a]; twice |= (seen & bit) != 0; seen |= bit; }
            atomicAdd(&s_hist[min(j1 - j0, VO_STATS_HIST - 1)], 1);
        }
        if (twice) {
            for (int a = j0; a < j1; a++) {
                const int c1 = slot[a];
                for (int k = a + 1; k < j1; k++) {
                    const int c2 = slot[k];
                    if (c1 != c2) atomicAdd(&s_mat[min(c1, c2) * VO_BA_MAX_CAMERAS + max(c1, c2)], 1);
                }
            }
            seen = 0;
        }
        for (int c1 = 0; c1 + 1 < ncam; c1++) {
            if (__ballot((int)((seen >> c1) & 1)) == 0) continue;  // (wave-uniform)
            for (int c2 = c1 + 1; c2 < ncam; c2++) {
                const unsigned long long w = __ballot((int)((seen >> c1) & (seen >> c2) & 1));
                if (w != 0 && lane == 0) atomicAdd(&s_mat[c1 * VO_BA_MAX_CAMERAS + c2], (int)__popcll(w));
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SLAM_WAVES; w++) { nh += s_nh[w]; if (s_mx[w] > mx) mx = s_mx[w]; }
        out.total_sqerr[row] = total; out.max_sqerr[row] = mx; out.n_high[row] = nh;
        out.counts[3 * (size_t)row] = ncam; out.counts[3 * (size_t)row + 1] = npt; out.counts[3 * (size_t)row + 2] = nobs;
    }
    if (tid < VO_STATS_HIST) out.obs_hist[(size_t)row * VO_STATS_HIST + tid] = s_hist[tid];
    for (int k = tid; k < C * C; k += SLAM_THREADS) out.obs_matrix[(size_t)row * C * C + k] = s_mat[(k / C) * VO_BA_MAX_CAMERAS + k % C];
    if (out.cam_frame && tid < C) out.cam_frame[(size_t)row * C + tid] = tid < ncam ? m.cam_frame[tid] : -1;
}

// (sb.base: where this map's ranges start — all 0 for a single chain, as for k_bundle_adjust)
__global__ __launch_bounds__(SLAM_THREADS) void k_slam_stats(int p, SlamBuf sb, StatsBuf out) { slam_stats_wg(sb.m, sb.base.pt0, sb.base.obs0, p, out); }

__global__ __launch_bounds__(SLAM_THREADS) void k_slam_stats_seqs(int j, const SlamSeq* __restrict__ seqs, StatsBuf out)
{
    const SlamSeq& q = seqs[blockIdx.x];
    if (j >= q.count) return;
    slam_stats_wg(q.sb.m, q.sb.base.pt0, q.sb.base.obs0, q.first + j, out);
}

void launch_slam_stats(hipStream_t s, int p, SlamBuf sb, StatsBuf out)
{
    hipLaunchKernelGGL(k_slam_stats, dim3(1), dim3(SLAM_THREADS), 0, s, p, sb, out);
}

void launch_slam_stats_seqs(hipStream_t s, int j, const SlamSeq* seqs, int S, StatsBuf out)
{
    hipLaunchKernelGGL(k_slam_stats_seqs, dim3(S), dim3(SLAM_THREADS), 0, s, j, seqs, out);
}
