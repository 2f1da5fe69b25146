// stream_archive_kernels.hip — selecting over a stream's archive of evicted points (vo_set_stream_archive,
// vo_map_from_stream_archive): docs/kernels/k_stream_archive.md.  The archive is filled by the camera limit itself
// (k_slam_limit_stream_archive, slam_kernels.hip); here its entries owned by a window of frames become a key list and a dense
// coordinate list in archive order, from which k_map_gather_from (reloc_kernels.hip) stages.
//
//   k_stream_archive_count   per tile of SA_TILE entries: how many the window selects with a row, and without
//   k_stream_archive_emit    the selected entries that have a row -> sel_key / sel_xyz, densely, in archive order
//
// The archive grows with the flight, not with the live map, so the store's scheme — every workgroup counts the whole list — would
// re-read it once per workgroup.  Here every entry is read twice: the count pass leaves two ints per tile, and a workgroup of the
// emit pass, which owns a contiguous range of tiles, adds up the counts of the tiles before its range (a few thousand ints, read
// redundantly) and then ranks inside its own tiles.  A position is the sum of the counts before the tile plus the rank in the tile:
// integer sums of values that depend on the entries alone, so the result depends neither on the grid nor on dispatch order.  No
// atomics, no word one workgroup writes and another reads inside a launch.
#include "vo_internal.h"
#include <limits.h>

#define SA_WAVES (SA_TILE / 64)

// f of every lane of the workgroup -> this lane's rank among the set ones, and their number.  s_w: [SA_WAVES] of a buffer the
// caller alternates between two consecutive calls.
__device__ __forceinline__ int sa_rank(bool f, int* s_w, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < SA_WAVES; w++) { const int c = s_w[w]; if (w < wave) off += c; tot += c; }
    total = tot;
    return off + (int)__popcll(bal & ((1ULL << lane) - 1));
}

// the sum of v over the workgroup, in every lane.  s_w: [SA_WAVES], free again after the call's second barrier
__device__ __forceinline__ long long sa_sum(long long v, long long* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    long long tot = 0;
    for (int w = 0; w < SA_WAVES; w++) tot += s_w[w];
    __syncthreads();
    return tot;
}

// the tiles this workgroup owns: a contiguous range, the same in both passes
__device__ __forceinline__ void sa_range(int tiles, int& t0, int& t1)
{
    const int per = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const long long b = (long long)blockIdx.x * per;
    t0 = (int)(b < tiles ? b : tiles);
    t1 = t0 + per < tiles ? t0 + per : tiles;
}

// entry e: in the window?  with a row?
__device__ __forceinline__ void sa_flags(const StreamArchive& a, int stored, int first, int end, long long e, bool& in, bool& row)
{
    in = false; row = false;
    if (e >= stored) return;
    const int fr = a.feature[2 * (size_t)e];
    in = fr >= first && fr < end;
    row = in && a.has_row[e] != 0;
}

__global__ __launch_bounds__(SA_TILE) void k_stream_archive_count(StreamArchive a, int stored, int first, int end)
{
    __shared__ int s_w[2][SA_WAVES], s_n[2][SA_WAVES];
    const int tid = threadIdx.x, tiles = (int)(((long long)stored + SA_TILE - 1) / SA_TILE);
    int t0, t1;
    sa_range(tiles, t0, t1);
    for (int t = t0; t < t1; t++) {
        bool in, row;
        sa_flags(a, stored, first, end, (long long)t * SA_TILE + tid, in, row);
        int n_in, n_row;
        (void)sa_rank(in, s_n[t & 1], n_in);
        (void)sa_rank(row, s_w[t & 1], n_row);
        if (tid == 0) { a.tile_cnt[2 * (size_t)t] = n_row; a.tile_cnt[2 * (size_t)t + 1] = n_in - n_row; }
    }
}

// live: the number of points staged before the archived ones (k_stream_rows_select's count, still on the device), nullptr: none
__global__ __launch_bounds__(SA_TILE) void k_stream_archive_emit(StreamArchive a, int stored, int first, int end, const int* __restrict__ live)
{
    __shared__ int s_w[2][SA_WAVES];
    __shared__ long long s_sum[SA_WAVES];
    const int tid = threadIdx.x, tiles = (int)(((long long)stored + SA_TILE - 1) / SA_TILE);
    int t0, t1;
    sa_range(tiles, t0, t1);
    long long part = 0;
    for (int t = tid; t < t0; t += SA_TILE) part += a.tile_cnt[2 * (size_t)t];
    long long before = sa_sum(part, s_sum) + (live ? live[0] : 0);
    for (int t = t0; t < t1; t++) {
        const long long e = (long long)t * SA_TILE + tid;
        bool in, row;
        sa_flags(a, stored, first, end, e, in, row);
        int total;
        const long long pos = before + sa_rank(row, s_w[t & 1], total);
        before += total;
        if (!row || pos >= a.sel_cap) continue;                // (nothing is written past the selection buffers: the host refuses by the count)
        a.sel_key[pos] = (int)e;
        for (int k = 0; k < 3; k++) a.sel_xyz[3 * (size_t)pos + k] = a.xyz[3 * (size_t)e + k];
    }
    if (blockIdx.x != 0) return;
    long long with = 0, without = 0;
    for (int t = tid; t < tiles; t += SA_TILE) { with += a.tile_cnt[2 * (size_t)t]; without += a.tile_cnt[2 * (size_t)t + 1]; }
    with = sa_sum(with, s_sum); without = sa_sum(without, s_sum);
    if (tid == 0) { a.sel_cnt[0] = (int)with; a.sel_cnt[1] = (int)without; }
}

void launch_stream_archive_select(hipStream_t s, StreamArchive a, int stored, int first, int end, const int* live)
{
    const long long tiles = ((long long)stored + SA_TILE - 1) / SA_TILE;
    const int grid = (int)(tiles < 1 ? 1 : tiles > 256 ? 256 : tiles);   // one workgroup per tile up to one per CU
    if (end < 0) end = INT_MAX;
    hipLaunchKernelGGL(k_stream_archive_count, dim3(grid), dim3(SA_TILE), 0, s, a, stored, first, end);
    hipLaunchKernelGGL(k_stream_archive_emit, dim3(grid), dim3(SA_TILE), 0, s, a, stored, first, end, live);
}
