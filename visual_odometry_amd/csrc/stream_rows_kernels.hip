// stream_rows_kernels.hip — the descriptor store of vo_slam_stream (vo_set_stream_rows, vo_map_from_stream): the descriptor row of
// every map point, kept in the stream's own memory from the call the point is born in, so that the stream's map can be staged for
// the relocaliser after its frames have left their slots.  docs/kernels/k_stream_rows.md.
//
//   k_stream_rows_append   end of every vo_slam_stream call: every point of the end map born in this call takes the next free store
//                          row, in map order, and the row of its owning feature is copied there from the slots' descriptors
//   k_stream_rows_select   vo_map_from_stream: the live map's points owned by a window of frames -> store rows as a key list and the
//                          coordinates as a dense list, in map order (k_map_gather, reloc_kernels.hip, stages from them unchanged)
//
// Both hand out positions in map order over a full grid without a word passing between workgroups: every workgroup counts the
// whole list in tiles of SR_THREADS points — the flags are a few bytes per point and stay in L2 — and writes the tiles
// t = blockIdx.x, blockIdx.x + gridDim.x, ...  The position of a point is the count before its tile plus its rank in the tile, so
// what is stored, and what is dropped when the store is full, depends on the lists alone: not on the grid, not on dispatch order.
// The walk's kernels (slam_kernels.hip) do not know the store exists.
#include "vo_internal.h"
#include <limits.h>

#define SR_THREADS 256
#define SR_WAVES (SR_THREADS / 64)

// f of every lane of the workgroup -> this lane's rank among the set ones, and their number.  s_w: [SR_WAVES] of a buffer the
// caller alternates between two consecutive calls (the second call's writes then cannot pass a slow wave's reads of the first).
__device__ __forceinline__ int sr_rank(bool f, int* s_w, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < SR_WAVES; w++) { const int c = s_w[w]; if (w < wave) off += c; tot += c; }
    total = tot;
    return off + (int)__popcll(bal & ((1ULL << lane) - 1));
}

// The entry of row_of a point's owning feature has, -1 if pt_feat names none (cannot happen: the walk writes frames of the stream)
__device__ __forceinline__ int sr_feature(const StreamRows& st, const int* pt_feat, int q)
{
    const int fr = pt_feat[2 * (size_t)q], kp = pt_feat[2 * (size_t)q + 1];
    return fr >= 0 && fr < st.frames && kp >= 0 && kp < st.kp_cap ? fr * st.kp_cap + kp : -1;
}

// A point is new when its owning frame is one of this call's (pt_feat.frame >= frame0) and its feature has no row yet.  "No row yet"
// is read as: row_of < 0, or row_of >= stored0 — a row this very launch has handed out (another workgroup's store that this one's
// count may or may not see; either value says the entry was -1 when the launch began).  stored0 / dropped0: the counters as the
// call before left them (the host keeps them), so no workgroup reads a counter another one writes.
// desc: the slots' descriptor rows [n_keys][D]; pt_key of a point born in this call is slot * kp_cap + keypoint, its row there.
__global__ __launch_bounds__(SR_THREADS) void k_stream_rows_append(SlamMap m, StreamRows st, const uint8_t* __restrict__ desc, int n_keys,
                                                                   int frame0, int stored0, int dropped0)
{
    __shared__ int s_w[2][SR_WAVES], s_row[SR_THREADS], s_key[SR_THREADS];
    const int tid = threadIdx.x, npt = m.cnt[1];
    const int room = st.capacity - stored0;                  // rows still free: >= 0
    const int lsh = st.D == 128 ? 3 : 1;                     // 16 bytes per lane: 8 lanes move a SIFT row, 2 an ORB row
    int before = 0;                                          // new points in the tiles before this one
    for (int t = 0, q0 = 0; q0 < npt; t++, q0 += SR_THREADS) {
        const int q = q0 + tid;
        int at = -1;
        if (q < npt && m.pt_feat[2 * (size_t)q] >= frame0) {
            at = sr_feature(st, m.pt_feat, q);
            if (at >= 0) { const int r = st.row_of[at]; if (r >= 0 && r < stored0) at = -1; }
        }
        int total;
        const int pos = before + sr_rank(at >= 0, s_w[t & 1], total);
        before += total;
        if (t % (int)gridDim.x != (int)blockIdx.x) continue;   // (the same for every lane of the workgroup)
        const bool ok = at >= 0 && pos < room;               // a point that finds the store full stays without a row
        if (ok) st.row_of[at] = stored0 + pos;
        s_row[tid] = ok ? stored0 + pos : -1;
        s_key[tid] = q < npt ? m.pt_key[q] : -1;
        __syncthreads();
        for (int e = tid; e < (SR_THREADS << lsh); e += SR_THREADS) {
            const int i = e >> lsh, part = e & ((1 << lsh) - 1), row = s_row[i], key = s_key[i];
            if (row < 0) continue;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);            // (a key outside the slots names no row: zeros, as k_map_gather stores them)
            if (key >= 0 && key < n_keys) v = *(const uint4*)(desc + (size_t)key * st.D + 16 * part);
            *(uint4*)(st.rows + (size_t)row * st.D + 16 * part) = v;
        }
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        st.counters[0] = stored0 + min(before, room);
        st.counters[1] = dropped0 + max(before - room, 0);
    }
}

// The points with first <= pt_feat.frame < end, in map order: those with a row go to sel_key / sel_xyz (the first sel_cap of them:
// the host refuses a larger selection by the count), the others are counted.  sel_cnt: [2] selected, without a row.
__global__ __launch_bounds__(SR_THREADS) void k_stream_rows_select(SlamMap m, StreamRows st, int first, int end)
{
    __shared__ int s_w[2][SR_WAVES], s_n[2][SR_WAVES];
    const int tid = threadIdx.x, npt = m.cnt[1];
    int before = 0, without = 0;
    for (int t = 0, q0 = 0; q0 < npt; t++, q0 += SR_THREADS) {
        const int q = q0 + tid;
        int row = -1; bool in = false;
        if (q < npt) {
            const int fr = m.pt_feat[2 * (size_t)q];
            in = fr >= first && fr < end;
            if (in) { const int at = sr_feature(st, m.pt_feat, q); if (at >= 0) row = st.row_of[at]; }
        }
        int total, total_in;
        (void)sr_rank(in, s_n[t & 1], total_in);
        const int pos = before + sr_rank(row >= 0, s_w[t & 1], total);
        before += total; without += total_in - total;
        if (t % (int)gridDim.x != (int)blockIdx.x || row < 0 || pos >= st.sel_cap) continue;
        st.sel_key[pos] = row;
        for (int a = 0; a < 3; a++) st.sel_xyz[3 * (size_t)pos + a] = m.pt_xyz[3 * (size_t)q + a];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) { st.sel_cnt[0] = before; st.sel_cnt[1] = without; }
}

// bound: points the list can hold — the grid is sized from it, one workgroup per tile up to one per CU (every workgroup reads the
// whole list, so more of them than tiles, or than CUs, only adds reads)
static int sr_grid(size_t bound)
{
    const size_t tiles = (bound + SR_THREADS - 1) / SR_THREADS;
    return (int)(tiles < 1 ? 1 : tiles > 256 ? 256 : tiles);
}

void launch_stream_rows_append(hipStream_t s, SlamMap m, StreamRows st, size_t pt_bound, const uint8_t* desc, int n_keys, int frame0, int stored0,
                               int dropped0)
{
    hipLaunchKernelGGL(k_stream_rows_append, dim3(sr_grid(pt_bound)), dim3(SR_THREADS), 0, s, m, st, desc, n_keys, frame0, stored0, dropped0);
}

void launch_stream_rows_select(hipStream_t s, SlamMap m, StreamRows st, size_t pt_bound, int first, int end)
{
    hipLaunchKernelGGL(k_stream_rows_select, dim3(sr_grid(pt_bound)), dim3(SR_THREADS), 0, s, m, st, first, end < 0 ? INT_MAX : end);
}
