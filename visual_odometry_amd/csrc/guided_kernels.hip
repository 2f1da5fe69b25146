// guided_kernels.hip — matching the staged map's points to a frame's keypoints by projection under a prior pose
// (vo_map_localize_guided; the contract is in include/vo_hip.h, "guided relocalisation"; docs/kernels/k_map_guided.md).
//
//   k_guided_grid    one workgroup per query: the frame's keypoints bucketed into GUIDED_G x GUIDED_G square cells over their own box
//   k_guided_match   one lane per map point: project, walk the cells its window touches, test the circle in float64, keep the best
//                    (d, keypoint) and the second distance, apply the filters, claim the keypoint with one 64-bit atomicMin
//   k_guided_select  one workgroup per query: the claim table in keypoint order -> RelocBuf's match list and correspondences
//   k_guided_keep    a query the refinement pass skipped takes its earlier status back
// Every decision is taken on a (distance, index) key, so neither the order of a cell's keypoints nor the order in which points
// claim changes a byte of the result.
#include "vo_internal.h"
#include <limits.h>
#include <float.h>

// ------------------------------------------------------------------ the grid
// Coordinates are clamped to [-GUIDED_BOUND, GUIDED_BOUND] before anything else is done with them, so the box is finite whatever
// the keypoints hold, and a cell index is computed from a finite double inside [0, GUIDED_G - 1] — never from an unclamped,
// infinite or NaN value.  guided_cell is monotone (non-decreasing) in x: clamp, subtract, multiply by a positive number, floor
// and clamp all are.  The same function places a keypoint and bounds a window, so a keypoint with lo <= x <= hi lies in a cell
// of [guided_cell(lo), guided_cell(hi)], wherever lo, x and hi fall relative to the box.
#define GUIDED_BOUND 1048576.0          // 2^20 px
#define GUIDED_MIN_EDGE 1.0             // px: a box narrower than GUIDED_G px keeps cells of one pixel

__device__ __forceinline__ double guided_clamp(double x)  // NaN -> -GUIDED_BOUND (fmax returns the other operand)
{
    return fmin(fmax(x, -GUIDED_BOUND), GUIDED_BOUND);
}

__device__ __forceinline__ int guided_cell(double x, double x0, double inv)
{
    const double f = floor((guided_clamp(x) - x0) * inv);
    return (int)fmin(fmax(f, 0.0), (double)(GUIDED_G - 1));
}

// min over the workgroup of 256, every thread gets it; s_r: 4 doubles
__device__ __forceinline__ double guided_block_min(double v, double* s_r)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_r[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(s_r[0], s_r[1]), fmin(s_r[2], s_r[3]));
}

__global__ __launch_bounds__(256) void k_guided_grid(RelocBuf r, GuidedBuf g, const float* kp_xy, const int* kp_count, int kp_cap)
{
    __shared__ int s_cnt[GUIDED_CELLS];
    __shared__ int s_w[4];
    __shared__ double s_r[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (g.skip[q] != VO_OK) return;                         // (uniform) not matched: nothing reads its grid
    const int slot = r.slots[q], nq = min(kp_count[slot], kp_cap);
    const float* xy = kp_xy + (size_t)slot * kp_cap * 2;
    int* cell_off = g.cell_off + (size_t)q * (GUIDED_CELLS + 1);
    int* cell_kp = g.cell_kp + (size_t)q * kp_cap;

    // the box of the (clamped) keypoints
    double lx = GUIDED_BOUND, ly = GUIDED_BOUND, hx = -GUIDED_BOUND, hy = -GUIDED_BOUND;
    for (int i = tid; i < nq; i += 256) {
        const double x = guided_clamp((double)xy[2 * i]), y = guided_clamp((double)xy[2 * i + 1]);
        lx = fmin(lx, x); hx = fmax(hx, x); ly = fmin(ly, y); hy = fmax(hy, y);
    }
    lx = guided_block_min(lx, s_r); ly = guided_block_min(ly, s_r);
    hx = -guided_block_min(-hx, s_r); hy = -guided_block_min(-hy, s_r);
    if (nq == 0) { lx = ly = hx = hy = 0; }
    const double edge = fmax(fmax(hx - lx, hy - ly) / GUIDED_G, GUIDED_MIN_EDGE), inv = 1.0 / edge;
    if (tid == 0) { double* bx = g.box + 4 * (size_t)q; bx[0] = lx; bx[1] = ly; bx[2] = inv; bx[3] = edge; }

    // count, scan, fill
    for (int c = tid; c < GUIDED_CELLS; c += 256) s_cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < nq; i += 256) {
        const int c = guided_cell((double)xy[2 * i + 1], ly, inv) * GUIDED_G + guided_cell((double)xy[2 * i], lx, inv);
        atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    constexpr int PER = GUIDED_CELLS / 256;                 // consecutive cells per thread
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
        const int c = tid * PER + k, n = s_cnt[c];
        cell_off[c] = base; s_cnt[c] = base;
        base += n;
    }
    if (tid == 255) cell_off[GUIDED_CELLS] = base;           // = nq
    __syncthreads();
    for (int i = tid; i < nq; i += 256) {
        const int c = guided_cell((double)xy[2 * i + 1], ly, inv) * GUIDED_G + guided_cell((double)xy[2 * i], lx, inv);
        cell_kp[atomicAdd(&s_cnt[c], 1)] = i;                // a position in [cell_off[c], cell_off[c + 1]) < nq <= kp_cap
    }
}

// ------------------------------------------------------------------ the match
// The exact integer distance between a map row held in registers and keypoint row `b`.
template <bool SIFT> struct GuidedRow;
template <> struct GuidedRow<false> {
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
__device__ __forceinline__ unsigned guided_dot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }
template <> struct GuidedRow<true> {
    uint4 a[8];
    unsigned aa;
    __device__ __forceinline__ void load(const uint8_t* p)
    {
        aa = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            a[k] = *(const uint4*)(p + 16 * k);
            aa = guided_dot4(a[k].x, a[k].x, aa); aa = guided_dot4(a[k].y, a[k].y, aa);
            aa = guided_dot4(a[k].z, a[k].z, aa); aa = guided_dot4(a[k].w, a[k].w, aa);
        }
    }
    __device__ __forceinline__ int dist(const uint8_t* b) const
    {
        unsigned bb = 0, ab = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint4 v = *(const uint4*)(b + 16 * k);
            bb = guided_dot4(v.x, v.x, bb); bb = guided_dot4(v.y, v.y, bb); bb = guided_dot4(v.z, v.z, bb); bb = guided_dot4(v.w, v.w, bb);
            ab = guided_dot4(a[k].x, v.x, ab); ab = guided_dot4(a[k].y, v.y, ab); ab = guided_dot4(a[k].z, v.z, ab); ab = guided_dot4(a[k].w, v.w, ab);
        }
        return (int)(aa + bb - 2u * ab);
    }
};

// Grid (point tiles, Q), GUIDED_TILE lanes: lane t of tile b owns point b GUIDED_TILE + t.  The frame's positions and rows are
// read through L2 (the lanes of a wavefront walk different cells: there is no common tile of the frame to stage).
template <bool SIFT>
__global__ __launch_bounds__(GUIDED_TILE) void k_guided_match(MapBuf m, RelocBuf r, GuidedBuf g, const uint8_t* desc, const float* kp_xy, int kp_cap,
                                                              const double* Kd, double radius, double r2, double max_distance, double ratio)
{
    constexpr int D = SIFT ? 128 : 32;
    const int q = blockIdx.y, j = blockIdx.x * GUIDED_TILE + threadIdx.x;
    if (g.skip[q] != VO_OK) return;                         // (uniform)
    const int slot = r.slots[q];
    const float* xy = kp_xy + (size_t)slot * kp_cap * 2;
    const uint8_t* rows = desc + (size_t)slot * kp_cap * D;
    const int* cell_off = g.cell_off + (size_t)q * (GUIDED_CELLS + 1);
    const int* cell_kp = g.cell_kp + (size_t)q * kp_cap;
    const double* P = g.prior + 12 * (size_t)q;
    const double* bx = g.box + 4 * (size_t)q;

    bool seen = false;
    if (j < m.npt) {
        const double X = m.xyz[(size_t)j * 3], Y = m.xyz[(size_t)j * 3 + 1], Z = m.xyz[(size_t)j * 3 + 2];
        const double c0 = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
        const double c1 = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
        const double c2 = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
        const double xn = c0 / c2, yn = c1 / c2;
        const double u = (Kd[0] * xn + Kd[1] * yn) + Kd[2], v = (Kd[3] * xn + Kd[4] * yn) + Kd[5];
        // a point behind the camera takes no part; an infinite or NaN u or v has no candidate (dx dx + dy dy <= r2 is false for
        // every float32 keypoint), so such a point never reaches the cell arithmetic
        if (c2 > 0 && isfinite(u) && isfinite(v)) {
            // The window's cell range.  A candidate has |x_i - u| <= radius up to a few roundings; the bounds are widened by far
            // more than that (2^-40 of radius + |u|, against roundings of 2^-52 of either), then clamped as floating-point
            // values inside guided_cell before any conversion.  guided_cell being monotone, lo <= hi gives cx0 <= cx1.
            const double wx = radius + (radius + fabs(u)) * 0x1p-40, wy = radius + (radius + fabs(v)) * 0x1p-40;
            const double x0 = bx[0], y0 = bx[1], inv = bx[2];
            const int cx0 = guided_cell(u - wx, x0, inv), cx1 = guided_cell(u + wx, x0, inv);
            const int cy0 = guided_cell(v - wy, y0, inv), cy1 = guided_cell(v + wy, y0, inv);
            GuidedRow<SIFT> row;
            row.load(m.rows + (size_t)j * D);
            // best = (d << 32) | keypoint, the smallest; d2 = the second-smallest distance of the multiset
            unsigned long long best = ~0ull;
            int d2 = INT_MAX, cnt = 0;
            for (int cy = cy0; cy <= cy1; cy++) {
                // the cells cx0 .. cx1 of a row are consecutive in cell order: one run of cell_kp
                const int k1 = cell_off[cy * GUIDED_G + cx1 + 1];
                for (int k = cell_off[cy * GUIDED_G + cx0]; k < k1; k++) {
                    const int i = cell_kp[k];
                    const float2 p = *(const float2*)(xy + 2 * (size_t)i);
                    const double dx = (double)p.x - u, dy = (double)p.y - v;
                    if (!(dx * dx + dy * dy <= r2)) continue;
                    const int d = row.dist(rows + (size_t)i * D);
                    const unsigned long long key = ((unsigned long long)(unsigned)d << 32) | (unsigned)i;
                    if (key < best) { if (cnt) d2 = (int)(best >> 32); best = key; }
                    else d2 = min(d2, d);
                    cnt++;
                }
            }
            if (cnt > 0) {
                seen = true;
                const int d = (int)(best >> 32), i = (int)(best & 0xffffffffu);
                const float fd = SIFT ? sqrtf((float)d) : (float)d;
                const float fd2 = cnt < 2 ? FLT_MAX : SIFT ? sqrtf((float)d2) : (float)d2;
                bool keep = true;
                if (max_distance > 0 && !((double)fd < max_distance)) keep = false;
                if (ratio > 0 && cnt >= 2 && !((double)fd < ratio * (double)fd2)) keep = false;
                if (keep) {
                    g.pt_d2[(size_t)q * m.cap_rows + j] = cnt < 2 ? INT_MAX : d2;
                    atomicMin(g.claim + (size_t)q * kp_cap + i, ((unsigned long long)(unsigned)d << 32) | (unsigned)j);
                }
            }
        }
    }
    const unsigned long long any = __ballot(seen);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(g.n_seen + q, __popcll(any));
}

void launch_guided_match(hipStream_t s, MapBuf m, RelocBuf r, GuidedBuf g, int Q, const uint8_t* desc, const float* kp_xy, const int* kp_count,
                         int kp_cap, const double* Kd, double radius, double max_distance, double ratio)
{
    if (Q <= 0) return;
    hipLaunchKernelGGL(k_guided_grid, dim3(Q), dim3(256), 0, s, r, g, kp_xy, kp_count, kp_cap);
    if (m.npt <= 0) return;
    const dim3 grid((m.npt + GUIDED_TILE - 1) / GUIDED_TILE, Q);
    const double r2 = radius * radius;
    if (m.D == 128) hipLaunchKernelGGL(k_guided_match<true>, grid, dim3(GUIDED_TILE), 0, s, m, r, g, desc, kp_xy, kp_cap, Kd, radius, r2, max_distance, ratio);
    else hipLaunchKernelGGL(k_guided_match<false>, grid, dim3(GUIDED_TILE), 0, s, m, r, g, desc, kp_xy, kp_cap, Kd, radius, r2, max_distance, ratio);
}

// ------------------------------------------------------------------ the match list, one workgroup per query (k_map_select's scan)
__global__ __launch_bounds__(256) void k_guided_select(MapBuf m, RelocBuf r, GuidedBuf g, const float* kp_xy, const int* kp_count, int kp_cap)
{
    __shared__ int s_w[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int slot = r.slots[q], nq = g.skip[q] != VO_OK ? 0 : min(kp_count[slot], kp_cap);
    const size_t o = (size_t)q * kp_cap;
    const float* xy = kp_xy + (size_t)slot * kp_cap * 2;
    const bool l2 = m.D == 128;
    int out_base = 0;
    for (int base = 0; base < nq; base += 256) {
        const int i = base + tid;
        const unsigned long long c = i < nq ? g.claim[o + i] : ~0ull;
        const bool has = c != ~0ull;
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
            const size_t pos = o + out_base + off + inc - 1;
            const int d = (int)(c >> 32), t = (int)(c & 0xffffffffu), d2 = g.pt_d2[(size_t)q * m.cap_rows + t];
            r.m_q[pos] = i; r.m_t[pos] = t;
            r.m_d[pos] = l2 ? sqrtf((float)d) : (float)d;
            r.m_d2[pos] = d2 == INT_MAX ? FLT_MAX : l2 ? sqrtf((float)d2) : (float)d2;
            for (int k = 0; k < 3; k++) r.obj[pos * 3 + k] = m.xyz[(size_t)t * 3 + k];
            r.img[pos * 2] = (double)xy[2 * i]; r.img[pos * 2 + 1] = (double)xy[2 * i + 1];
        }
        out_base += tot;
    }
    if (tid == 0) { r.m_count[q] = out_base; r.off[2 * q] = (int)o; r.off[2 * q + 1] = (int)o + out_base; }
}

void launch_guided_select(hipStream_t s, MapBuf m, RelocBuf r, GuidedBuf g, int Q, const float* kp_xy, const int* kp_count, int kp_cap)
{
    if (Q <= 0) return;
    hipLaunchKernelGGL(k_guided_select, dim3(Q), dim3(256), 0, s, m, r, g, kp_xy, kp_count, kp_cap);
}

__global__ void k_guided_keep(RelocBuf r, GuidedBuf g, int Q)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q || g.skip[q] == VO_OK) return;
    r.status[q] = g.skip[q]; r.ninl[q] = 0;
    for (int k = 0; k < 12; k++) r.poses[12 * (size_t)q + k] = 0;
}

void launch_guided_keep(hipStream_t s, RelocBuf r, GuidedBuf g, int Q)
{
    if (Q <= 0) return;
    hipLaunchKernelGGL(k_guided_keep, dim3((Q + 63) / 64), dim3(64), 0, s, r, g, Q);
}
