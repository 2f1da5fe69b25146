// map_fuse_kernels.hip — matching the points of Q query maps to the staged map's points in space under a prior similarity
// (vo_map_align_guided; the contract is in include/vo_hip.h, "guided map alignment"; docs/kernels/k_map_fuse.md).
//
//   k_fuse_grid     one workgroup: the staged map's points bucketed into FUSE_G^3 cells over their own box, an edge per axis; built
//                   once per call and read by all Q queries
//   k_fuse_match    one lane per query point: transform, walk the cells its window touches, test the sphere in float64, keep the best
//                   (d, staged point) and the second distance, apply the filters, claim the staged point with one 64-bit atomicMin
//   k_fuse_select   one workgroup per query: the query rows in order, a row being an entry iff the claim of its best names it ->
//                   AlignBuf's match lists and correspondences
//   k_fuse_keep     a query the refinement pass skipped takes its earlier status back
// Every decision is taken on a (distance, index) key, so neither the order of a cell's points nor the order in which rows claim
// changes a byte of the result.
#include "vo_internal.h"
#include <limits.h>
#include <float.h>

// ------------------------------------------------------------------ the grid
// The argument of k_guided_grid (guided_kernels.hip), with a third axis and an edge per axis.  Coordinates are clamped to
// [-FUSE_BOUND, FUSE_BOUND] before anything else is done with them, so the box is finite whatever the points hold, and a cell index
// is computed from a finite double inside [0, FUSE_G - 1] — never from an unclamped, infinite or NaN value.  fuse_cell is monotone
// (non-decreasing) in x: clamp, subtract, multiply by a non-negative number, floor and clamp all are.  The same function places a
// point and bounds a window, so a point with lo <= x <= hi lies in a cell of [fuse_cell(lo), fuse_cell(hi)], wherever lo, x and hi
// fall relative to the box, and a range is never inverted.  An axis whose extent is below FUSE_G FUSE_MIN_EDGE — zero extent
// included — has inv = 0: every value lands in cell 0, the axis is one cell, and nothing is divided by a small number.
#define FUSE_BOUND 1099511627776.0      // 2^40 map units
#define FUSE_MIN_EDGE 0x1p-20           // map units: (2 FUSE_BOUND) / FUSE_MIN_EDGE = 2^61 is a finite double
#define FUSE_GRID_T 1024

__device__ __forceinline__ double fuse_clamp(double x)  // NaN -> -FUSE_BOUND (fmax returns the other operand)
{
    return fmin(fmax(x, -FUSE_BOUND), FUSE_BOUND);
}

__device__ __forceinline__ int fuse_cell(double x, double x0, double inv)
{
    const double f = floor((fuse_clamp(x) - x0) * inv);
    return (int)fmin(fmax(f, 0.0), (double)(FUSE_G - 1));
}

// min over the workgroup of FUSE_GRID_T, every thread gets it; s_r: FUSE_GRID_T / 64 doubles
__device__ __forceinline__ double fuse_block_min(double v, double* s_r)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s_r[0];
#pragma unroll
    for (int w = 1; w < FUSE_GRID_T / 64; w++) r = fmin(r, s_r[w]);
    return r;
}

__global__ __launch_bounds__(FUSE_GRID_T) void k_fuse_grid(MapBuf m, FuseBuf f)
{
    __shared__ int s_cnt[FUSE_CELLS];
    __shared__ int s_w[FUSE_GRID_T / 64];
    __shared__ double s_r[FUSE_GRID_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, n = m.npt;

    // the box of the finite (clamped) coordinates, axis by axis
    double lo[3] = {FUSE_BOUND, FUSE_BOUND, FUSE_BOUND}, hi[3] = {-FUSE_BOUND, -FUSE_BOUND, -FUSE_BOUND};
    for (int i = tid; i < n; i += FUSE_GRID_T) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double x = m.xyz[(size_t)i * 3 + k];
            if (isfinite(x)) { const double c = fuse_clamp(x); lo[k] = fmin(lo[k], c); hi[k] = fmax(hi[k], c); }
        }
    }
    double x0[3], inv[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double l = fuse_block_min(lo[k], s_r), h = -fuse_block_min(-hi[k], s_r);
        if (!(l <= h)) l = h = 0;                           // no finite coordinate on this axis
        const double edge = (h - l) / FUSE_G;               // <= 2^37
        x0[k] = l; inv[k] = edge >= FUSE_MIN_EDGE ? 1.0 / edge : 0.0;
        if (tid == 0) { f.box[2 * k] = l; f.box[2 * k + 1] = inv[k]; }
    }

    // count, scan, fill
    for (int c = tid; c < FUSE_CELLS; c += FUSE_GRID_T) s_cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += FUSE_GRID_T) {
        const double* p = m.xyz + (size_t)i * 3;
        const int c = (fuse_cell(p[2], x0[2], inv[2]) * FUSE_G + fuse_cell(p[1], x0[1], inv[1])) * FUSE_G + fuse_cell(p[0], x0[0], inv[0]);
        atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    constexpr int PER = FUSE_CELLS / FUSE_GRID_T;           // consecutive cells per thread
    int sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) sum += s_cnt[tid * PER + k];
    int inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    int base = inc - sum;
    for (int w = 0; w < wid; w++) base += s_w[w];
#pragma unroll
    for (int k = 0; k < PER; k++) {                          // the count becomes the cell's start, then its fill cursor
        const int c = tid * PER + k, cn = s_cnt[c];
        f.cell_off[c] = base; s_cnt[c] = base;
        base += cn;
    }
    if (tid == FUSE_GRID_T - 1) f.cell_off[FUSE_CELLS] = base;   // = npt
    __syncthreads();
    for (int i = tid; i < n; i += FUSE_GRID_T) {
        const double* p = m.xyz + (size_t)i * 3;
        const int c = (fuse_cell(p[2], x0[2], inv[2]) * FUSE_G + fuse_cell(p[1], x0[1], inv[1])) * FUSE_G + fuse_cell(p[0], x0[0], inv[0]);
        f.cell_pt[atomicAdd(&s_cnt[c], 1)] = i;              // a position in [cell_off[c], cell_off[c + 1]) < npt <= cap_rows
    }
}

// ------------------------------------------------------------------ the match
// The exact integer distance between a query row held in registers and staged row `b`: k_guided_match's (guided_kernels.hip).
template <bool SIFT> struct FuseRow;
template <> struct FuseRow<false> {
    uint4 a0, a1;
    __device__ __forceinline__ void load(const uint8_t* p) { a0 = *(const uint4*)p; a1 = *(const uint4*)(p + 16); }
    __device__ __forceinline__ int dist(const uint8_t* b) const
    {
        const uint4 b0 = *(const uint4*)b, b1 = *(const uint4*)(b + 16);
        return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
               __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
    }
};
// sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a b over uint8 values: three exact integer sums below 2^24 (v_dot4_u32_u8)
__device__ __forceinline__ unsigned fuse_dot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }
template <> struct FuseRow<true> {
    uint4 a[8];
    unsigned aa;
    __device__ __forceinline__ void load(const uint8_t* p)
    {
        aa = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            a[k] = *(const uint4*)(p + 16 * k);
            aa = fuse_dot4(a[k].x, a[k].x, aa); aa = fuse_dot4(a[k].y, a[k].y, aa);
            aa = fuse_dot4(a[k].z, a[k].z, aa); aa = fuse_dot4(a[k].w, a[k].w, aa);
        }
    }
    __device__ __forceinline__ int dist(const uint8_t* b) const
    {
        unsigned bb = 0, ab = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint4 v = *(const uint4*)(b + 16 * k);
            bb = fuse_dot4(v.x, v.x, bb); bb = fuse_dot4(v.y, v.y, bb); bb = fuse_dot4(v.z, v.z, bb); bb = fuse_dot4(v.w, v.w, bb);
            ab = fuse_dot4(a[k].x, v.x, ab); ab = fuse_dot4(a[k].y, v.y, ab); ab = fuse_dot4(a[k].z, v.z, ab); ab = fuse_dot4(a[k].w, v.w, ab);
        }
        return (int)(aa + bb - 2u * ab);
    }
};

// Grid (row tiles of the largest query map, Q), FUSE_TILE lanes: lane t of tile b owns row b FUSE_TILE + t of query map q.  The
// staged positions and rows are read through L2 (the lanes of a wavefront walk different cells: there is no common tile to stage).
// Reads are bounded by the counts alone: query rows by off[q + 1] - off[q], staged points by the cell lists, which hold 0 .. npt - 1.
template <bool SIFT>
__global__ __launch_bounds__(FUSE_TILE) void k_fuse_match(MapBuf m, AlignBuf a, FuseBuf f, double radius, double r2, double max_distance, double ratio)
{
    constexpr int D = SIFT ? 128 : 32;
    const int q = blockIdx.y, i = blockIdx.x * FUSE_TILE + threadIdx.x;
    if (f.skip[q] != VO_OK) return;                         // (uniform)
    const int o = a.off[q], nq = a.off[q + 1] - o;
    if (blockIdx.x * FUSE_TILE >= nq) return;               // (uniform) a tile past this query map's end
    const double* S = f.prior + 13 * (size_t)q;

    bool seen = false;
    if (i < nq) {
        unsigned long long mine = ~0ull;
        int mine_d2 = INT_MAX;
        const double bx = a.xyz[(size_t)(o + i) * 3], by = a.xyz[(size_t)(o + i) * 3 + 1], bz = a.xyz[(size_t)(o + i) * 3 + 2];
        const double s = S[0];
        const double y0 = s * ((S[1] * bx + S[2] * by) + S[3] * bz) + S[10];
        const double y1 = s * ((S[4] * bx + S[5] * by) + S[6] * bz) + S[11];
        const double y2 = s * ((S[7] * bx + S[8] * by) + S[9] * bz) + S[12];
        if (isfinite(y0) && isfinite(y1) && isfinite(y2)) {
            // The window's cell range.  A candidate has |a_k - y_k| <= radius up to a few roundings; the bounds are widened by far
            // more than that (2^-40 of radius + |y_k|, against roundings of 2^-52 of either), then clamped as floating-point values
            // inside fuse_cell before any conversion.  fuse_cell being monotone, lo <= hi gives c0 <= c1 on every axis.
            const double w0 = radius + (radius + fabs(y0)) * 0x1p-40, w1 = radius + (radius + fabs(y1)) * 0x1p-40,
                         w2 = radius + (radius + fabs(y2)) * 0x1p-40;
            const int cx0 = fuse_cell(y0 - w0, f.box[0], f.box[1]), cx1 = fuse_cell(y0 + w0, f.box[0], f.box[1]);
            const int cy0 = fuse_cell(y1 - w1, f.box[2], f.box[3]), cy1 = fuse_cell(y1 + w1, f.box[2], f.box[3]);
            const int cz0 = fuse_cell(y2 - w2, f.box[4], f.box[5]), cz1 = fuse_cell(y2 + w2, f.box[4], f.box[5]);
            FuseRow<SIFT> row;
            row.load(a.rows + ((size_t)a.pad[q] + i) * D);
            // best = (d << 32) | staged point, the smallest; d2 = the second-smallest distance of the multiset
            unsigned long long best = ~0ull;
            int d2 = INT_MAX, cnt = 0;
            for (int cz = cz0; cz <= cz1; cz++)
                for (int cy = cy0; cy <= cy1; cy++) {
                    // the cells cx0 .. cx1 of a row are consecutive in cell order: one run of cell_pt
                    const int c = (cz * FUSE_G + cy) * FUSE_G;
                    const int k1 = f.cell_off[c + cx1 + 1];
                    for (int k = f.cell_off[c + cx0]; k < k1; k++) {
                        const int j = f.cell_pt[k];
                        const double* p = m.xyz + (size_t)j * 3;
                        const double dx = p[0] - y0, dy = p[1] - y1, dz = p[2] - y2;
                        if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
                        const int d = row.dist(m.rows + (size_t)j * D);
                        const unsigned long long key = ((unsigned long long)(unsigned)d << 32) | (unsigned)j;
                        if (key < best) { if (cnt) d2 = (int)(best >> 32); best = key; }
                        else d2 = min(d2, d);
                        cnt++;
                    }
                }
            if (cnt > 0) {
                seen = true;
                const int d = (int)(best >> 32), j = (int)(best & 0xffffffffu);
                const float fd = SIFT ? sqrtf((float)d) : (float)d;
                const float fd2 = cnt < 2 ? FLT_MAX : SIFT ? sqrtf((float)d2) : (float)d2;
                bool keep = true;
                if (max_distance > 0 && !((double)fd < max_distance)) keep = false;
                if (ratio > 0 && cnt >= 2 && !((double)fd < ratio * (double)fd2)) keep = false;
                if (keep) {
                    mine = best; mine_d2 = cnt < 2 ? INT_MAX : d2;
                    atomicMin(f.claim + (size_t)q * m.cap_rows + j, ((unsigned long long)(unsigned)d << 32) | (unsigned)i);
                }
            }
        }
        f.pt_best[o + i] = mine; f.pt_d2[o + i] = mine_d2;
    }
    const unsigned long long any = __ballot(seen);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(f.n_seen + q, __popcll(any));
}

void launch_fuse_match(hipStream_t s, MapBuf m, AlignBuf a, FuseBuf f, int max_rows, double radius, double max_distance, double ratio)
{
    if (a.Q <= 0) return;
    hipLaunchKernelGGL(k_fuse_grid, dim3(1), dim3(FUSE_GRID_T), 0, s, m, f);
    if (max_rows <= 0) return;
    const dim3 grid((max_rows + FUSE_TILE - 1) / FUSE_TILE, a.Q);
    const double r2 = radius * radius;
    if (m.D == 128) hipLaunchKernelGGL(k_fuse_match<true>, grid, dim3(FUSE_TILE), 0, s, m, a, f, radius, r2, max_distance, ratio);
    else hipLaunchKernelGGL(k_fuse_match<false>, grid, dim3(FUSE_TILE), 0, s, m, a, f, radius, r2, max_distance, ratio);
}

// ------------------------------------------------------------------ the match lists, one workgroup per query (k_align_select's scan)
__global__ __launch_bounds__(256) void k_fuse_select(MapBuf m, AlignBuf a, FuseBuf f)
{
    __shared__ int s_w[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int o = a.off[q], nq = f.skip[q] != VO_OK ? 0 : a.off[q + 1] - o;
    const unsigned long long* claim = f.claim + (size_t)q * m.cap_rows;
    const bool l2 = m.D == 128;
    int out_base = 0;
    for (int base = 0; base < nq; base += 256) {
        const int i = base + tid;
        const unsigned long long b = i < nq ? f.pt_best[o + i] : ~0ull;
        const int j = (int)(b & 0xffffffffu);                // (< npt whenever b is a key: it came out of the cell lists)
        const bool has = b != ~0ull && claim[j] == ((b & 0xffffffff00000000ull) | (unsigned)i);
        int inc = has ? 1 : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
        __syncthreads();
        if (lane == 63) s_w[wid] = inc;
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { const int x = s_w[w]; if (w < wid) off += x; tot += x; }
        if (has) {
            const size_t pos = (size_t)o + out_base + off + inc - 1;
            const int d = (int)(b >> 32), d2 = f.pt_d2[o + i];
            a.m_b[pos] = i; a.m_a[pos] = j;
            a.m_d[pos] = l2 ? sqrtf((float)d) : (float)d;
            a.m_d2[pos] = d2 == INT_MAX ? FLT_MAX : l2 ? sqrtf((float)d2) : (float)d2;
            for (int k = 0; k < 3; k++) { a.src[pos * 3 + k] = a.xyz[(size_t)(o + i) * 3 + k]; a.dst[pos * 3 + k] = m.xyz[(size_t)j * 3 + k]; }
        }
        out_base += tot;
    }
    if (tid == 0) { a.m_count[q] = out_base; a.poff[2 * q] = o; a.poff[2 * q + 1] = o + out_base; }
}

void launch_fuse_select(hipStream_t s, MapBuf m, AlignBuf a, FuseBuf f)
{
    if (a.Q <= 0) return;
    hipLaunchKernelGGL(k_fuse_select, dim3(a.Q), dim3(256), 0, s, m, a, f);
}

__global__ void k_fuse_keep(AlignBuf a, FuseBuf f)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.Q || f.skip[q] == VO_OK) return;
    a.status[q] = f.skip[q]; a.ninl[q] = 0;
    for (int k = 0; k < 13; k++) a.sim[13 * (size_t)q + k] = 0;
}

void launch_fuse_keep(hipStream_t s, AlignBuf a, FuseBuf f)
{
    if (a.Q <= 0) return;
    hipLaunchKernelGGL(k_fuse_keep, dim3((a.Q + 63) / 64), dim3(64), 0, s, a, f);
}
