// reloc_kernels.hip — relocalisation of resident frames against a map by its descriptors (vo_map_stage, vo_map_from_slam,
// vo_map_localize): what the reference carries and never uses — TrackedPoint.descriptor = match.descriptor1
// (src/visual_slam.py:72-76, :102-106) and MatchWithMap.distance, "TODO: Set to the proper feature distance" (:211-217).
//
//   k_map_gather   a map's rows, from the slots' descriptors by the owning feature id or from rows a caller staged, into the
//                  matcher's operand — both through map_store_rows
//   k_nn_map       nearest neighbours in both directions between Q frames and the one map (SIFT: integer d^2 on the matrix cores;
//   k_nn_map_orb   ORB: XOR + popcount)
//   k_map_select   bf.match(frame, map) with crossCheck=True, the distance filter, and the 3D-2D correspondences in the layout
//                  k_pnp_ransac takes (pnp_kernels.hip, launched unchanged)
// Semantics follow OpenCV's batchDistance: ascending scan, strict `<`, so the lowest index wins ties, in both directions.
#include "vo_internal.h"
#include "sift_rows.h"
#include <limits.h>

// ------------------------------------------------------------------ the map store
// Row `id` of the map from `src_row` (D bytes).  SIFT (D = 128): called by a whole wavefront, lane l moves bytes 2 l, 2 l + 1 —
// the raw row, the int8 operand image, the norm and the norm-bound flag are sb_store_row's, the map being slot 0 of an image of
// cap_rows rows.  ORB (D = 32): called by 8 consecutive lanes (part = 0..7), lane `part` moves bytes 4 part .. 4 part + 3.
// k_map_gather is the only caller; the rows of vo_map_stage and of vo_map_from_slam differ only in where src_row points.
__device__ __forceinline__ void map_store_row_sift(const MapBuf& m, int id, const uint8_t* src_row, int lane)
{
    const unsigned v = src_row ? *(const uint16_t*)(src_row + 2 * lane) : 0u;
    sb_store_row((int)(v & 255u), (int)(v >> 8), lane, 0, id, 0, m.rows, m.img, m.cap_rows, m.norms, m.flag);
}

__device__ __forceinline__ void map_store_row_orb(const MapBuf& m, int id, const uint8_t* src_row, int part)
{
    *(uint32_t*)(m.rows + (size_t)id * 32 + 4 * part) = src_row ? *(const uint32_t*)(src_row + 4 * part) : 0u;
}

// key == nullptr: row i of src.  Otherwise row key[i] of src (slot * kp_cap + keypoint: SlamMap::pt_key); a key outside
// [0, n_keys) names no row and stores zeros (the map kernels never write one).
__global__ __launch_bounds__(256) void k_map_gather(MapBuf m, const uint8_t* src, const int* key, int n_keys, const double* xyz)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (m.D == 128) {
        for (int id = blockIdx.x * 4 + (tid >> 6); id < m.npt; id += gridDim.x * 4) {
            const int k = key ? key[id] : id;
            map_store_row_sift(m, id, key && (k < 0 || k >= n_keys) ? nullptr : src + (size_t)k * 128, lane);
            if (lane < 3) m.xyz[(size_t)id * 3 + lane] = xyz[(size_t)id * 3 + lane];
        }
    } else {
        for (int id = blockIdx.x * 32 + (tid >> 3); id < m.npt; id += gridDim.x * 32) {
            const int k = key ? key[id] : id, part = tid & 7;
            map_store_row_orb(m, id, key && (k < 0 || k >= n_keys) ? nullptr : src + (size_t)k * 32, part);
            if (part < 3) m.xyz[(size_t)id * 3 + part] = xyz[(size_t)id * 3 + part];
        }
    }
}

void launch_map_gather(hipStream_t s, MapBuf m, const uint8_t* src, const int* key, int n_keys, const double* xyz)
{
    if (m.npt <= 0) return;
    const int per = m.D == 128 ? 4 : 32, g = (m.npt + per - 1) / per;
    hipLaunchKernelGGL(k_map_gather, dim3(g < 4096 ? g : 4096), dim3(256), 0, s, m, src, key, n_keys, xyz);
}

// ------------------------------------------------------------------ k_nn_map: SIFT rows, integer d^2 on the matrix cores
// The identity and the selection argument are k_nn_l2i8's (docs/kernels/k_nn_l2i8.md): d^2 = |a|^2 + |b|^2 - 2 a.b on
// v_mfma_i32_16x16x64_i8 over rows shifted to int8, ordered by the integer (sqrtf is strictly increasing below 2^22; rows that
// would allow more are flagged at the store).  That kernel's body is tied to a PairBuf and to two slots of one image, so its
// unpacked (value, group) form is restated here over two operand images given by pointer: A, whose rows get a neighbour each, and
// B, which is streamed through LDS in CHUNKS of NM_STAGE_ROWS rows, double buffered.  B may be the map (up to 65536 rows: the
// group index stays a plain int, there is no bound from a packed key) or a frame.  Within a chunk and across chunks a later
// column replaces the best only when strictly nearer, and the 16 lanes of a row fold with the lower column winning: the lowest
// B index wins a tie wherever the tied rows lie — in one lane, in two lanes, in two chunks.
typedef int v4i __attribute__((ext_vector_type(4)));
#define NM_WAVES 8
#define NM_THREADS (NM_WAVES * 64)
#define NM_RB 4                           // 16-row blocks of A per wave, held in registers as MFMA fragments
#define NM_WAVE_ROWS (NM_RB * 16)
#define NM_BLOCK_ROWS (NM_WAVES * NM_WAVE_ROWS)
#define NM_STAGE_ROWS 128                 // rows of B per chunk (8 groups of 16, 16 KB)
#define NM_LD (NM_STAGE_ROWS * 128 / 16 / NM_THREADS)   // 16-byte staging loads per thread and chunk

// out_dist may be nullptr (the reverse direction: the mutual test needs the index only)
__device__ __forceinline__ void nn_map_l2_body(uint8_t (*s_b)[NM_STAGE_ROWS * 128], const uint8_t* A, const int* nA, int na, const uint8_t* B, const int* nB,
                                               int nb, int row0, int* out_idx, int* out_dist)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int wrow0 = row0 + wave * NM_WAVE_ROWS;
    const bool active = wrow0 < na;

    v4i a[NM_RB][2];
#pragma unroll
    for (int rb = 0; rb < NM_RB; rb++)
#pragma unroll
        for (int s = 0; s < 2; s++)
            a[rb][s] = active ? *(const v4i*)(A + ((size_t)((wrow0 >> 4) + rb) * 8 + 4 * s + lg) * 256 + li * 16) : (v4i){0, 0, 0, 0};
    v4i bv[NM_RB], bg[NM_RB];
#pragma unroll
    for (int rb = 0; rb < NM_RB; rb++) { bv[rb] = (v4i){INT_MIN, INT_MIN, INT_MIN, INT_MIN}; bg[rb] = (v4i){-1, -1, -1, -1}; }

    const int nstages = (nb + NM_STAGE_ROWS - 1) / NM_STAGE_ROWS;
#define NM_GLDS(stage, buf)                                                                                        \
    _Pragma("unroll") for (int q = 0; q < NM_LD; q++)                                                              \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(B + (size_t)(stage) * (NM_STAGE_ROWS * 128) + (size_t)(q * NM_THREADS + tid) * 16), \
                                         (__attribute__((address_space(3))) void*)(s_b[buf] + (q * NM_THREADS + wave * 64) * 16), 16, 0, 0)
    // |b - 128|^2 of the chunk's rows, loaded a chunk ahead like the rows themselves
    constexpr int NGS = NM_STAGE_ROWS / 16;
    int nbn[NGS], nbs[NGS];
#define NM_NORMS(stage)                                                                                            \
    _Pragma("unroll") for (int g = 0; g < NGS; g++) {                                                              \
        const int jn = ((stage) * NGS + g) * 16 + li;                                                              \
        nbn[g] = jn < nb ? nB[jn] : 0x3fffffff;          /* columns past the end can never win */                  \
    }
    if (nstages > 0) { NM_NORMS(0); NM_GLDS(0, 0); }
    for (int sg = 0; sg < nstages; sg++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int g = 0; g < NGS; g++) nbs[g] = nbn[g];
        if (sg + 1 < nstages) { NM_NORMS(sg + 1); NM_GLDS(sg + 1, (sg + 1) & 1); }
        const uint8_t* sb = s_b[sg & 1];
        const int ng = active ? min(NGS, (nb - sg * NM_STAGE_ROWS + 15) >> 4) : 0;
#pragma unroll
        for (int g = 0; g < NGS; g++) {
            if (g >= ng) break;
            const int gi = sg * NGS + g;
            const int nbj = nbs[g];
            v4i b[2], acc[NM_RB];
#pragma unroll
            for (int s = 0; s < 2; s++) b[s] = *(const v4i*)(sb + g * 2048 + (4 * s + lg) * 256 + li * 16);
            const v4i zero = {0, 0, 0, 0};
#pragma unroll
            for (int rb = 0; rb < NM_RB; rb++) acc[rb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[rb][0], b[0], zero, 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NM_RB; rb++) acc[rb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[rb][1], b[1], acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NM_RB; rb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int val = 2 * acc[rb][r] - nbj;             // larger = nearer
                    const bool gt = val > bv[rb][r];                  // strict: the earlier group of this lane's column stays
                    bv[rb][r] = gt ? val : bv[rb][r];
                    bg[rb][r] = gt ? gi : bg[rb][r];
                }
        }
    }
#undef NM_GLDS
#undef NM_NORMS
    // fold the 16 lanes (columns li of every group) of a row: 64-bit keys (value + 2^31) << 32 | ~column — larger value first,
    // then the lower column
#pragma unroll
    for (int rb = 0; rb < NM_RB; rb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int g = bg[rb][r];
            unsigned long long k0 = g < 0 ? 0ull : ((unsigned long long)((unsigned)bv[rb][r] ^ 0x80000000u) << 32) | (unsigned)(0x7fffffff - (g * 16 + li));
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { const unsigned long long u0 = __shfl_xor(k0, d, 64); k0 = k0 > u0 ? k0 : u0; }
            const int row = wrow0 + rb * 16 + lg * 4 + r;
            if (li == 0 && row < na) {
                const int v0 = (int)((unsigned)(k0 >> 32) ^ 0x80000000u), j0 = 0x7fffffff - (int)(k0 & 0xffffffffu);
                out_idx[row] = k0 ? j0 : -1;
                if (out_dist) out_dist[row] = k0 ? nA[row] - v0 : INT_MAX;
            }
        }
}

// Workgroup b of query q = b / (fwd_blocks + rev_blocks): the first fwd_blocks take NM_BLOCK_ROWS keypoints of the frame each and
// walk the map; the others take NM_BLOCK_ROWS map rows each and walk the frame.
__global__ __launch_bounds__(NM_THREADS) void k_nn_map(MapBuf m, RelocBuf r, const uint8_t* desc_x, const int* norms, const int* kp_count, int kp_cap,
                                                       int cap_x, int fwd_blocks, int rev_blocks)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_b[2][NM_STAGE_ROWS * 128];
    const int q = blockIdx.x / (fwd_blocks + rev_blocks), blk = blockIdx.x % (fwd_blocks + rev_blocks);
    const int slot = r.slots[q], nq = min(kp_count[slot], kp_cap);
    const uint8_t* F = desc_x + (size_t)slot * cap_x * 128;
    const int* nF = norms + (size_t)slot * cap_x;
    if (blk < fwd_blocks) {
        const int row0 = blk * NM_BLOCK_ROWS;
        if (row0 >= nq) return;
        nn_map_l2_body(s_b, F, nF, nq, m.img, m.norms, m.npt, row0, r.nn_idx + (size_t)q * kp_cap, r.nn_dist + (size_t)q * kp_cap);
    } else {
        const int row0 = (blk - fwd_blocks) * NM_BLOCK_ROWS;
        if (row0 >= m.npt) return;
        nn_map_l2_body(s_b, m.img, m.norms, m.npt, F, nF, nq, row0, r.rn_idx + (size_t)q * m.cap_rows, nullptr);
    }
}

// ------------------------------------------------------------------ k_nn_map_orb: ORB rows, XOR + popcount
// k_nn_pairs' formulation (match_kernels.hip) restated over two row arrays given by pointer: a lane holds NO_Q rows of A in
// registers, B is streamed through LDS in chunks of NO_TILE rows and read as wave-wide broadcasts; best = one key
// (distance << 16 | B row), an unsigned min is the ascending scan with strict `<`.  B rows < 65536: vo_map_stage's bound on npt
// and the keypoint capacity.  The matrix-core Hamming kernels carry the column inside their accumulator (< 16129, < 8192 rows) and
// would need a key per chunk; this pull request does not build that form.
#define NO_TILE 256
#define NO_Q 2
#define NO_BLOCK_ROWS (256 * NO_Q)

__device__ __forceinline__ void nn_map_hamming_body(uint4* s_b, const uint8_t* A, int na, const uint8_t* B, int nb, int row0, int* out_idx, int* out_dist)
{
    const int tid = threadIdx.x;
    uint4 ma[NO_Q], mb[NO_Q];
    int row[NO_Q];
    uint32_t k0[NO_Q];
#pragma unroll
    for (int q = 0; q < NO_Q; q++) {
        row[q] = row0 + q * 256 + tid;
        ma[q] = make_uint4(0, 0, 0, 0); mb[q] = ma[q];
        if (row[q] < na) { ma[q] = *(const uint4*)(A + (size_t)row[q] * 32); mb[q] = *(const uint4*)(A + (size_t)row[q] * 32 + 16); }
        k0[q] = 0xffffffffu;
    }
    for (int base = 0; base < nb; base += NO_TILE) {
        const int j = base + tid;
        __syncthreads();
        if (j < nb) { s_b[2 * tid] = *(const uint4*)(B + (size_t)j * 32); s_b[2 * tid + 1] = *(const uint4*)(B + (size_t)j * 32 + 16); }
        __syncthreads();
        const int lim = min(NO_TILE, nb - base);
#pragma unroll 4
        for (int k = 0; k < lim; k++) {
            const uint4 ba = s_b[2 * k], bb = s_b[2 * k + 1];
#pragma unroll
            for (int q = 0; q < NO_Q; q++) {
                const int h = __popc(ma[q].x ^ ba.x) + __popc(ma[q].y ^ ba.y) + __popc(ma[q].z ^ ba.z) + __popc(ma[q].w ^ ba.w) +
                              __popc(mb[q].x ^ bb.x) + __popc(mb[q].y ^ bb.y) + __popc(mb[q].z ^ bb.z) + __popc(mb[q].w ^ bb.w);
                k0[q] = min(k0[q], ((uint32_t)h << 16) | (uint32_t)(base + k));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NO_Q; q++)
        if (row[q] < na) {
            const bool has = k0[q] != 0xffffffffu;
            out_idx[row[q]] = has ? (int)(k0[q] & 0xffffu) : -1;
            if (out_dist) out_dist[row[q]] = has ? (int)(k0[q] >> 16) : INT_MAX;
        }
}

__global__ __launch_bounds__(256) void k_nn_map_orb(MapBuf m, RelocBuf r, const uint8_t* desc, const int* kp_count, int kp_cap, int fwd_blocks, int rev_blocks)
{
    __shared__ uint4 s_b[NO_TILE * 2];
    const int q = blockIdx.x / (fwd_blocks + rev_blocks), blk = blockIdx.x % (fwd_blocks + rev_blocks);
    const int slot = r.slots[q], nq = min(kp_count[slot], kp_cap);
    const uint8_t* F = desc + (size_t)slot * kp_cap * 32;
    if (blk < fwd_blocks) {
        const int row0 = blk * NO_BLOCK_ROWS;
        if (row0 >= nq) return;
        nn_map_hamming_body(s_b, F, nq, m.rows, m.npt, row0, r.nn_idx + (size_t)q * kp_cap, r.nn_dist + (size_t)q * kp_cap);
    } else {
        const int row0 = (blk - fwd_blocks) * NO_BLOCK_ROWS;
        if (row0 >= m.npt) return;
        nn_map_hamming_body(s_b, m.rows, m.npt, F, nq, row0, r.rn_idx + (size_t)q * m.cap_rows, nullptr);
    }
}

void launch_nn_map(hipStream_t s, MapBuf m, RelocBuf r, int Q, const uint8_t* desc, const uint8_t* desc_x, const int* norms, const int* kp_count,
                   int kp_cap, int cap_x)
{
    if (Q <= 0) return;
    static_assert(NM_BLOCK_ROWS == NO_BLOCK_ROWS, "one grid formula for both kernels");
    const int fwd = (kp_cap + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS, rev = (m.npt + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS;
    if (m.D == 128) hipLaunchKernelGGL(k_nn_map, dim3((unsigned)Q * (fwd + rev)), dim3(NM_THREADS), 0, s, m, r, desc_x, norms, kp_count, kp_cap, cap_x, fwd, rev);
    else hipLaunchKernelGGL(k_nn_map_orb, dim3((unsigned)Q * (fwd + rev)), dim3(256), 0, s, m, r, desc, kp_count, kp_cap, fwd, rev);
}

// ------------------------------------------------------------------ k_map_select: the match list and the correspondences, one workgroup per query
// bf.match(frame, map) with crossCheck=True — keypoint i and its nearest map row t are a match when t's nearest keypoint is i —
// then `m.distance < max_distance` on cv2's float32 distance (sqrtf((float)d^2) for SIFT rows, the integer as float for ORB rows;
// max_distance <= 0: no filter), compacted in ascending keypoint order; obj[k] = the map point of trainIdx, img[k] =
// float64(kp_xy[queryIdx]): MatchWithMap's orientation (src/visual_slam.py:211-217).
__device__ __forceinline__ int ms_excl_scan_256(int v, int* s_w, int* total)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { int t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    __syncthreads();
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { int x = s_w[w]; if (w < wid) off += x; tot += x; }
    *total = tot;
    return off + inc - v;
}

__global__ __launch_bounds__(256) void k_map_select(MapBuf m, RelocBuf r, const float* kp_xy, const int* kp_count, int kp_cap, double max_distance)
{
    __shared__ int s_w[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int slot = r.slots[q], nq = min(kp_count[slot], kp_cap);
    const size_t o = (size_t)q * kp_cap;
    const int* fidx = r.nn_idx + o; const int* fdist = r.nn_dist + o;
    const int* ridx = r.rn_idx + (size_t)q * m.cap_rows;
    const float* xy = kp_xy + (size_t)slot * kp_cap * 2;
    const bool l2 = m.D == 128;
    int out_base = 0;
    for (int base = 0; base < nq; base += 256) {
        const int i = base + tid;
        int t = -1; float fd = 0.f;
        if (i < nq && m.npt > 0) {
            t = fidx[i];
            if (t >= 0 && ridx[t] != i) t = -1;
            if (t >= 0) {
                const int d = fdist[i];
                fd = l2 ? sqrtf((float)d) : (float)d;
                if (max_distance > 0 && !((double)fd < max_distance)) t = -1;
            }
        }
        int tot;
        const int pos = out_base + ms_excl_scan_256(t >= 0 ? 1 : 0, s_w, &tot);
        if (t >= 0) {
            r.m_q[o + pos] = i; r.m_t[o + pos] = t; r.m_d[o + pos] = fd;
            for (int k = 0; k < 3; k++) r.obj[(o + pos) * 3 + k] = m.xyz[(size_t)t * 3 + k];
            r.img[(o + pos) * 2] = (double)xy[2 * i]; r.img[(o + pos) * 2 + 1] = (double)xy[2 * i + 1];
        }
        out_base += tot;
    }
    if (tid == 0) { r.m_count[q] = out_base; r.off[2 * q] = (int)o; r.off[2 * q + 1] = (int)o + out_base; }
}

void launch_map_select(hipStream_t s, MapBuf m, RelocBuf r, int Q, const float* kp_xy, const int* kp_count, int kp_cap, double max_distance)
{
    if (Q <= 0) return;
    hipLaunchKernelGGL(k_map_select, dim3(Q), dim3(256), 0, s, m, r, kp_xy, kp_count, kp_cap, max_distance);
}
