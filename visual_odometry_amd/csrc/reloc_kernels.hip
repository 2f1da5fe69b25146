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
// vo_set_map_match modes 1 and 2: Lowe's ratio rule on knnMatch(k=2) against the map (src/feature_detection.py:20-26) — the K2 instantiations
// of the two bodies keep the second distance, k_map_select / k_align_select apply the rule; mode 1 launches no reverse blocks.
// Further down: map alignment (vo_map_align, vo_sim3_ransac_batch) — k_align_gather, k_nn_align[_orb], k_align_select over the same stores
// and bodies, and k_sim3_ransac.
#include "vo_internal.h"
#include "sift_rows.h"
#include <limits.h>
#include <float.h>
#include <type_traits>

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

// k_map_gather for the rows id0 .. m.npt - 1 of the map: the part vo_map_from_stream_archive stages behind the live points.  key
// and xyz are indexed by the map row, as k_map_gather's are; a kernel of its own, so that k_map_gather's code is what it was.
__global__ __launch_bounds__(256) void k_map_gather_from(MapBuf m, int id0, const uint8_t* src, const int* key, int n_keys, const double* xyz)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (m.D == 128) {
        for (int id = id0 + blockIdx.x * 4 + (tid >> 6); id < m.npt; id += gridDim.x * 4) {
            const int k = key[id];
            map_store_row_sift(m, id, k < 0 || k >= n_keys ? nullptr : src + (size_t)k * 128, lane);
            if (lane < 3) m.xyz[(size_t)id * 3 + lane] = xyz[(size_t)id * 3 + lane];
        }
    } else {
        for (int id = id0 + blockIdx.x * 32 + (tid >> 3); id < m.npt; id += gridDim.x * 32) {
            const int k = key[id], part = tid & 7;
            map_store_row_orb(m, id, k < 0 || k >= n_keys ? nullptr : src + (size_t)k * 32, part);
            if (part < 3) m.xyz[(size_t)id * 3 + part] = xyz[(size_t)id * 3 + part];
        }
    }
}

void launch_map_gather_from(hipStream_t s, MapBuf m, int id0, const uint8_t* src, const int* key, int n_keys, const double* xyz)
{
    if (id0 < 0 || m.npt <= id0) return;
    const int per = m.D == 128 ? 4 : 32, g = (m.npt - id0 + per - 1) / per;
    hipLaunchKernelGGL(k_map_gather_from, dim3(g < 4096 ? g : 4096), dim3(256), 0, s, m, id0, src, key, n_keys, xyz);
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

// out_dist may be nullptr (the reverse direction: the mutual test needs the index only).
// K2 (knnMatch(k=2): the ratio rule of k_map_select) keeps the second-largest value per element as well: bs <= bv always, so the
// value that is second after `val` has been seen is the median of the three — one v_med3_i32 before the update of the best.  A
// value equal to the best counts as a second neighbour.  out_dist2[row] = the second-smallest d^2 (INT_MAX when B has one row).
// K2 is deduced from the last argument; a call without it is the code it was before there was a K2.
template <bool K2 = false>
__device__ __forceinline__ void nn_map_l2_body(uint8_t (*s_b)[NM_STAGE_ROWS * 128], const uint8_t* A, const int* nA, int na, const uint8_t* B, const int* nB,
                                               int nb, int row0, int* out_idx, int* out_dist, int* out_dist2 = nullptr, std::bool_constant<K2> = {})
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
    v4i bs[K2 ? NM_RB : 1];
    if constexpr (K2) {
#pragma unroll
        for (int rb = 0; rb < NM_RB; rb++) bs[rb] = (v4i){INT_MIN, INT_MIN, INT_MIN, INT_MIN};
    }

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
                    if constexpr (K2) bs[rb][r] = max(min(val, bv[rb][r]), min(max(val, bv[rb][r]), bs[rb][r]));   // v_med3_i32
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
            const unsigned long long mine = k0;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { const unsigned long long u0 = __shfl_xor(k0, d, 64); k0 = k0 > u0 ? k0 : u0; }
            // the row's second value: the winning lane's own second, every other lane's best (a tie with the winner included)
            int v1 = INT_MIN;
            if constexpr (K2) {
                v1 = mine == k0 ? bs[rb][r] : bv[rb][r];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) v1 = max(v1, __shfl_xor(v1, d, 64));
            }
            const int row = wrow0 + rb * 16 + lg * 4 + r;
            if (li == 0 && row < na) {
                const int v0 = (int)((unsigned)(k0 >> 32) ^ 0x80000000u), j0 = 0x7fffffff - (int)(k0 & 0xffffffffu);
                out_idx[row] = k0 ? j0 : -1;
                if (out_dist) out_dist[row] = k0 ? nA[row] - v0 : INT_MAX;
                if constexpr (K2) out_dist2[row] = nb >= 2 ? nA[row] - v1 : INT_MAX;
            }
        }
}

// Workgroup b of query q = b / (fwd_blocks + rev_blocks): the first fwd_blocks take NM_BLOCK_ROWS keypoints of the frame each and
// walk the map; the others take NM_BLOCK_ROWS map rows each and walk the frame.
// K2: the forward blocks keep the second distance too (nn_dist2).  The ratio rule alone (vo_set_map_match mode 1) needs no reverse
// direction: it is launched with rev_blocks = 0.
template <bool K2>
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
        nn_map_l2_body(s_b, F, nF, nq, m.img, m.norms, m.npt, row0, r.nn_idx + (size_t)q * kp_cap, r.nn_dist + (size_t)q * kp_cap,
                       r.nn_dist2 + (size_t)q * kp_cap, std::bool_constant<K2>{});
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

// K2: two keys, k1 = the second smallest (keys are distinct: a tied distance at a higher row is the second neighbour).
template <bool K2 = false>
__device__ __forceinline__ void nn_map_hamming_body(uint4* s_b, const uint8_t* A, int na, const uint8_t* B, int nb, int row0, int* out_idx, int* out_dist,
                                                    int* out_dist2 = nullptr, std::bool_constant<K2> = {})
{
    const int tid = threadIdx.x;
    uint4 ma[NO_Q], mb[NO_Q];
    int row[NO_Q];
    uint32_t k0[NO_Q], k1[NO_Q];
#pragma unroll
    for (int q = 0; q < NO_Q; q++) {
        k1[q] = 0xffffffffu;
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
                const uint32_t key = ((uint32_t)h << 16) | (uint32_t)(base + k);
                if constexpr (K2) k1[q] = min(k1[q], max(k0[q], key));
                k0[q] = min(k0[q], key);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NO_Q; q++)
        if (row[q] < na) {
            const bool has = k0[q] != 0xffffffffu;
            out_idx[row[q]] = has ? (int)(k0[q] & 0xffffu) : -1;
            if (out_dist) out_dist[row[q]] = has ? (int)(k0[q] >> 16) : INT_MAX;
            if constexpr (K2) out_dist2[row[q]] = k1[q] != 0xffffffffu ? (int)(k1[q] >> 16) : INT_MAX;
        }
}

template <bool K2>
__global__ __launch_bounds__(256) void k_nn_map_orb(MapBuf m, RelocBuf r, const uint8_t* desc, const int* kp_count, int kp_cap, int fwd_blocks, int rev_blocks)
{
    __shared__ uint4 s_b[NO_TILE * 2];
    const int q = blockIdx.x / (fwd_blocks + rev_blocks), blk = blockIdx.x % (fwd_blocks + rev_blocks);
    const int slot = r.slots[q], nq = min(kp_count[slot], kp_cap);
    const uint8_t* F = desc + (size_t)slot * kp_cap * 32;
    if (blk < fwd_blocks) {
        const int row0 = blk * NO_BLOCK_ROWS;
        if (row0 >= nq) return;
        nn_map_hamming_body(s_b, F, nq, m.rows, m.npt, row0, r.nn_idx + (size_t)q * kp_cap, r.nn_dist + (size_t)q * kp_cap,
                            r.nn_dist2 + (size_t)q * kp_cap, std::bool_constant<K2>{});
    } else {
        const int row0 = (blk - fwd_blocks) * NO_BLOCK_ROWS;
        if (row0 >= m.npt) return;
        nn_map_hamming_body(s_b, m.rows, m.npt, F, nq, row0, r.rn_idx + (size_t)q * m.cap_rows, nullptr);
    }
}

void launch_nn_map(hipStream_t s, MapBuf m, RelocBuf r, int Q, const uint8_t* desc, const uint8_t* desc_x, const int* norms, const int* kp_count,
                   int kp_cap, int cap_x, int mode)
{
    if (Q <= 0) return;
    static_assert(NM_BLOCK_ROWS == NO_BLOCK_ROWS, "one grid formula for both kernels");
    const int fwd = (kp_cap + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS, rev = mode == 1 ? 0 : (m.npt + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS;
    const dim3 grid((unsigned)Q * (fwd + rev));
    if (m.D == 128) {
        if (mode == 0) hipLaunchKernelGGL(k_nn_map<false>, grid, dim3(NM_THREADS), 0, s, m, r, desc_x, norms, kp_count, kp_cap, cap_x, fwd, rev);
        else hipLaunchKernelGGL(k_nn_map<true>, grid, dim3(NM_THREADS), 0, s, m, r, desc_x, norms, kp_count, kp_cap, cap_x, fwd, rev);
    } else {
        if (mode == 0) hipLaunchKernelGGL(k_nn_map_orb<false>, grid, dim3(256), 0, s, m, r, desc, kp_count, kp_cap, fwd, rev);
        else hipLaunchKernelGGL(k_nn_map_orb<true>, grid, dim3(256), 0, s, m, r, desc, kp_count, kp_cap, fwd, rev);
    }
}

// ------------------------------------------------------------------ k_map_select: the match list and the correspondences, one workgroup per query
// bf.match(frame, map) with crossCheck=True — keypoint i and its nearest map row t are a match when t's nearest keypoint is i —
// then `m.distance < max_distance` on cv2's float32 distance (sqrtf((float)d^2) for SIFT rows, the integer as float for ORB rows;
// max_distance <= 0: no filter), compacted in ascending keypoint order; obj[k] = the map point of trainIdx, img[k] =
// float64(kp_xy[queryIdx]): MatchWithMap's orientation (src/visual_slam.py:211-217).
// mode (vo_set_map_match) 0: that; 1: knnMatch(k=2) and `m.distance < ratio * n.distance` in the place of the mutual test (rn_idx
// is not read: k_nn_map wrote none); 2: the mutual test and the ratio rule.  The rule is k_match_select's: no match when the map has
// fewer than two rows, else (double)fd < ratio * (double)fd2 on cv2's float32 distances; fd2 goes to m_d2 in list order.
__device__ __forceinline__ bool map_ratio_keeps(int mode, double ratio, bool l2, int npt, float fd, const int* fdist2, int i, float* fd2)
{
    if (mode == 0) return true;
    if (npt < 2) return false;
    const int d2 = fdist2[i];
    *fd2 = d2 == INT_MAX ? FLT_MAX : l2 ? sqrtf((float)d2) : (float)d2;
    return (double)fd < ratio * (double)*fd2;
}

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

__global__ __launch_bounds__(256) void k_map_select(MapBuf m, RelocBuf r, const float* kp_xy, const int* kp_count, int kp_cap, double max_distance,
                                                    int mode, double ratio)
{
    __shared__ int s_w[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int slot = r.slots[q], nq = min(kp_count[slot], kp_cap);
    const size_t o = (size_t)q * kp_cap;
    const int* fidx = r.nn_idx + o; const int* fdist = r.nn_dist + o; const int* fdist2 = r.nn_dist2 + o;
    const int* ridx = r.rn_idx + (size_t)q * m.cap_rows;
    const float* xy = kp_xy + (size_t)slot * kp_cap * 2;
    const bool l2 = m.D == 128;
    int out_base = 0;
    for (int base = 0; base < nq; base += 256) {
        const int i = base + tid;
        int t = -1; float fd = 0.f, fd2 = FLT_MAX;
        if (i < nq && m.npt > 0) {
            t = fidx[i];
            if (mode != 1 && t >= 0 && ridx[t] != i) t = -1;
            if (t >= 0) {
                const int d = fdist[i];
                fd = l2 ? sqrtf((float)d) : (float)d;
                if (max_distance > 0 && !((double)fd < max_distance)) t = -1;
                if (t >= 0 && !map_ratio_keeps(mode, ratio, l2, m.npt, fd, fdist2, i, &fd2)) t = -1;
            }
        }
        int tot;
        const int pos = out_base + ms_excl_scan_256(t >= 0 ? 1 : 0, s_w, &tot);
        if (t >= 0) {
            r.m_q[o + pos] = i; r.m_t[o + pos] = t; r.m_d[o + pos] = fd;
            if (mode != 0) r.m_d2[o + pos] = fd2;
            for (int k = 0; k < 3; k++) r.obj[(o + pos) * 3 + k] = m.xyz[(size_t)t * 3 + k];
            r.img[(o + pos) * 2] = (double)xy[2 * i]; r.img[(o + pos) * 2 + 1] = (double)xy[2 * i + 1];
        }
        out_base += tot;
    }
    if (tid == 0) { r.m_count[q] = out_base; r.off[2 * q] = (int)o; r.off[2 * q + 1] = (int)o + out_base; }
}

void launch_map_select(hipStream_t s, MapBuf m, RelocBuf r, int Q, const float* kp_xy, const int* kp_count, int kp_cap, double max_distance,
                       int mode, double ratio)
{
    if (Q <= 0) return;
    hipLaunchKernelGGL(k_map_select, dim3(Q), dim3(256), 0, s, m, r, kp_xy, kp_count, kp_cap, max_distance, mode, ratio);
}

// ================================================================== map-to-map alignment (vo_map_align, vo_sim3_ransac_batch)
//   k_align_gather     Q query maps' rows into operands of their own, through the map's stores (map_store_row_sift / _orb)
//   k_nn_align[_orb]   nearest neighbours in both directions between every query map and the staged one: the bodies above, both
//                      operands given by pointer
//   k_align_select     the cross-check match, the distance filter, and the 3D-3D lists (b = query point, a = staged point)
//   k_sim3_ransac      X_a = s R X_b + t by RANSAC over Umeyama's closed form (include/vo_hip.h, "map alignment")

// Query q's operand as a map of its own: its rows start at row pad[q] (a multiple of 256) of the padded arrays, so that the 64-row
// fragments and the 128-row chunks of nn_map_l2_body stay inside what belongs to it.
__device__ __forceinline__ MapBuf align_query_map(const AlignBuf& a, int q)
{
    const int p0 = a.pad[q];
    MapBuf m;
    m.D = a.D; m.cap_rows = a.pad[q + 1] - p0; m.npt = a.off[q + 1] - a.off[q];
    m.rows = a.rows + (size_t)p0 * a.D; m.img = a.img ? a.img + (size_t)p0 * 128 : nullptr; m.norms = a.norms ? a.norms + p0 : nullptr;
    m.xyz = a.xyz + (size_t)a.off[q] * 3; m.flag = a.flag;
    return m;
}

// row g of the caller's concatenated rows -> row g - off[q] of query map q
__global__ __launch_bounds__(256) void k_align_gather(AlignBuf a, const uint8_t* src)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int per = a.D == 128 ? 4 : 32, sub = a.D == 128 ? tid >> 6 : tid >> 3;
    for (int g = blockIdx.x * per + sub; g < a.total; g += gridDim.x * per) {
        int q = 0;
        while (q + 1 < a.Q && a.off[q + 1] <= g) q++;
        const MapBuf m = align_query_map(a, q);
        if (a.D == 128) map_store_row_sift(m, g - a.off[q], src + (size_t)g * 128, lane);
        else map_store_row_orb(m, g - a.off[q], src + (size_t)g * 32, tid & 7);
    }
}

template <bool K2>
__global__ __launch_bounds__(NM_THREADS) void k_nn_align(MapBuf m, AlignBuf a, int fwd_blocks, int rev_blocks)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_b[2][NM_STAGE_ROWS * 128];
    const int q = blockIdx.x / (fwd_blocks + rev_blocks), blk = blockIdx.x % (fwd_blocks + rev_blocks);
    const MapBuf f = align_query_map(a, q);
    if (blk < fwd_blocks) {
        const int row0 = blk * NM_BLOCK_ROWS;
        if (row0 >= f.npt) return;
        nn_map_l2_body(s_b, f.img, f.norms, f.npt, m.img, m.norms, m.npt, row0, a.nn_idx + a.pad[q], a.nn_dist + a.pad[q], a.nn_dist2 + a.pad[q],
                       std::bool_constant<K2>{});
    } else {
        const int row0 = (blk - fwd_blocks) * NM_BLOCK_ROWS;
        if (row0 >= m.npt) return;
        nn_map_l2_body(s_b, m.img, m.norms, m.npt, f.img, f.norms, f.npt, row0, a.rn_idx + (size_t)q * m.cap_rows, nullptr);
    }
}

template <bool K2>
__global__ __launch_bounds__(256) void k_nn_align_orb(MapBuf m, AlignBuf a, int fwd_blocks, int rev_blocks)
{
    __shared__ uint4 s_b[NO_TILE * 2];
    const int q = blockIdx.x / (fwd_blocks + rev_blocks), blk = blockIdx.x % (fwd_blocks + rev_blocks);
    const MapBuf f = align_query_map(a, q);
    if (blk < fwd_blocks) {
        const int row0 = blk * NO_BLOCK_ROWS;
        if (row0 >= f.npt) return;
        nn_map_hamming_body(s_b, f.rows, f.npt, m.rows, m.npt, row0, a.nn_idx + a.pad[q], a.nn_dist + a.pad[q], a.nn_dist2 + a.pad[q],
                            std::bool_constant<K2>{});
    } else {
        const int row0 = (blk - fwd_blocks) * NO_BLOCK_ROWS;
        if (row0 >= m.npt) return;
        nn_map_hamming_body(s_b, m.rows, m.npt, f.rows, f.npt, row0, a.rn_idx + (size_t)q * m.cap_rows, nullptr);
    }
}

// k_map_select's rules with a map's rows in the place of a frame's; the lists of query q start at off[q]: b_idx (query row),
// a_idx (staged row), cv2's float32 distance, src[k] = the query's point, dst[k] = the staged map's point.
__global__ __launch_bounds__(256) void k_align_select(MapBuf m, AlignBuf a, double max_distance, int mode, double ratio)
{
    __shared__ int s_w[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int o = a.off[q], nq = a.off[q + 1] - o;
    const int* fidx = a.nn_idx + a.pad[q]; const int* fdist = a.nn_dist + a.pad[q]; const int* fdist2 = a.nn_dist2 + a.pad[q];
    const int* ridx = a.rn_idx + (size_t)q * m.cap_rows;
    const bool l2 = m.D == 128;
    int out_base = 0;
    for (int base = 0; base < nq; base += 256) {
        const int i = base + tid;
        int t = -1; float fd = 0.f, fd2 = FLT_MAX;
        if (i < nq && m.npt > 0) {
            t = fidx[i];
            if (mode != 1 && t >= 0 && ridx[t] != i) t = -1;
            if (t >= 0) {
                const int d = fdist[i];
                fd = l2 ? sqrtf((float)d) : (float)d;
                if (max_distance > 0 && !((double)fd < max_distance)) t = -1;
                if (t >= 0 && !map_ratio_keeps(mode, ratio, l2, m.npt, fd, fdist2, i, &fd2)) t = -1;
            }
        }
        int tot;
        const int pos = o + out_base + ms_excl_scan_256(t >= 0 ? 1 : 0, s_w, &tot);
        if (t >= 0) {
            a.m_b[pos] = i; a.m_a[pos] = t; a.m_d[pos] = fd;
            if (mode != 0) a.m_d2[pos] = fd2;
            for (int k = 0; k < 3; k++) { a.src[(size_t)pos * 3 + k] = a.xyz[(size_t)(o + i) * 3 + k]; a.dst[(size_t)pos * 3 + k] = m.xyz[(size_t)t * 3 + k]; }
        }
        out_base += tot;
    }
    if (tid == 0) { a.m_count[q] = out_base; a.poff[2 * q] = o; a.poff[2 * q + 1] = o + out_base; }
}

void launch_map_align_gather(hipStream_t s, AlignBuf a, const uint8_t* src_rows)
{
    if (a.Q <= 0 || a.total <= 0) return;
    const int per = a.D == 128 ? 4 : 32, g = (a.total + per - 1) / per;
    hipLaunchKernelGGL(k_align_gather, dim3(g < 4096 ? g : 4096), dim3(256), 0, s, a, src_rows);
}

void launch_map_align_match(hipStream_t s, MapBuf m, AlignBuf a, const uint8_t* src_rows, int max_rows, int mode)
{
    if (a.Q <= 0) return;
    launch_map_align_gather(s, a, src_rows);
    const int fwd = (max_rows + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS, rev = mode == 1 ? 0 : (m.npt + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS;
    if (fwd + rev > 0) {
        const dim3 grid((unsigned)a.Q * (fwd + rev));
        if (m.D == 128) {
            if (mode == 0) hipLaunchKernelGGL(k_nn_align<false>, grid, dim3(NM_THREADS), 0, s, m, a, fwd, rev);
            else hipLaunchKernelGGL(k_nn_align<true>, grid, dim3(NM_THREADS), 0, s, m, a, fwd, rev);
        } else {
            if (mode == 0) hipLaunchKernelGGL(k_nn_align_orb<false>, grid, dim3(256), 0, s, m, a, fwd, rev);
            else hipLaunchKernelGGL(k_nn_align_orb<true>, grid, dim3(256), 0, s, m, a, fwd, rev);
        }
    }
}

void launch_map_align_select(hipStream_t s, MapBuf m, AlignBuf a, double max_distance, int mode, double ratio)
{
    if (a.Q <= 0) return;
    hipLaunchKernelGGL(k_align_select, dim3(a.Q), dim3(256), 0, s, m, a, max_distance, mode, ratio);
}

// ------------------------------------------------------------------ k_sim3_ransac: X_a = s R X_b + t from 3D-3D correspondences
// The operator is stated in include/vo_hip.h ("map alignment"); the skeleton is k_pnp_ransac's (pnp_kernels.hip): one workgroup per
// problem, rounds of 64 hypotheses — wave 0 draws the 64 subsets from the tabulated MWC stream and fits one model per lane, the four
// waves score four hypotheses at a time, and every lane carries the same copy of niters / best, so hypotheses are consumed in order
// and the stop rule is the sequential one.  A fit is closed form: the moments of the sample, a 3 x 3 one-sided Jacobi SVD held in
// registers (dp_jacobi_svd's rotations and threshold, unrolled over constant indices: no scratch), and U completed by u3 = u1 x u2.
// A three-point H has rank 2, so sigma_3 u_3 is rounding noise; with u3 = u1 x u2, det U = +1 and S = diag(1, 1, sign(det V)),
// tr(D S) = sigma_1 + sigma_2 + sign(det V) u3 . (H v3): the same R and s as any orthonormal completion gives, and continuous in H.
// The correspondences of a problem of up to SIM3_LDS_PTS points are staged in LDS, one array per coordinate (consecutive lanes,
// consecutive banks); a larger problem reads global memory.
#define SIM3_LDS_PTS 3072                  // 6 doubles each: 144 KB of the 160 KB a workgroup can have
#define SIM3_STREAM 448
#define SIM3_COS 0.996                     // the subset check's cosine (include/vo_hip.h)
struct Sim3Shared {
    double   pts[6][SIM3_LDS_PTS];          // b.x b.y b.z a.x a.y a.z
    double   model[64][13];                 // s, R row-major, t
    double   red[4][10];
    uint32_t stream[SIM3_STREAM];
    int      sub[64][3];
    int      ok[64];
    int      cnt[2][4];
    int      used;
};

// cv::RNG::next and cv::RANSACUpdateNumIters as pnp_kernels.hip states them (static there)
__device__ static inline uint32_t sim3_rng_next(uint64_t* state)
{
    *state = (uint64_t)(uint32_t)*state * 4164903690U + (uint32_t)(*state >> 32);
    return (uint32_t)*state;
}

__device__ static int sim3_update_num_iters(double p, double ep, int model_points, int max_iters)
{
    p = p < 0 ? 0 : p; p = p > 1 ? 1 : p;
    ep = ep < 0 ? 0 : ep; ep = ep > 1 ? 1 : ep;
    double num = 1. - p > DBL_MIN ? 1. - p : DBL_MIN;
    double denom = 1. - pow(1. - ep, model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)lrint(num / denom);
}

template <bool ST>
__device__ __forceinline__ void sim3_point(const Sim3Shared& sh, const double* src, const double* dst, int i, double* b, double* a)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        b[k] = ST ? sh.pts[k][i] : src[(size_t)i * 3 + k];
        a[k] = ST ? sh.pts[3 + k][i] : dst[(size_t)i * 3 + k];
    }
}

__device__ __forceinline__ double sim3_dot(const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// one side of the subset check: the two difference vectors from point 0 are neither zero nor nearly collinear
__device__ __forceinline__ bool sim3_side_ok(const double* p0, const double* p1, const double* p2)
{
    const double d1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, d2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double n1 = sim3_dot(d1, d1), n2 = sim3_dot(d2, d2), dt = sim3_dot(d1, d2);
    return n1 != 0 && n2 != 0 && !(fabs(dt) > SIM3_COS * sqrt(n1 * n2));
}

// The model M = {s, R row-major, t} from the centroids ac, bc, var_b = sum |b - bc|^2 / m and H = sum (a - ac)(b - bc)^T / m
// (row-major).  false: no model (M is then not to be used).
__device__ __forceinline__ bool sim3_from_moments(const double* ac, const double* bc, double var_b, const double* H, double* M)
{
    const double eps = DBL_EPSILON * 10;
    double c[3][3], v[3][3], w[3];          // c[i] = column i of H, then sigma_i u_i; v[i] = right singular vector i
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 3; k++) { c[i][k] = H[3 * k + i]; v[i][k] = i == k ? 1. : 0.; }
        w[i] = sim3_dot(c[i], c[i]);
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = i + 1; j < 3; j++) {
                double a = w[i], p = sim3_dot(c[i], c[j]), b = w[j];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b;
                double gamma, cs, sn;
                {
                    double x = fabs(p), y = fabs(beta);
                    if (x < y) { const double t = x; x = y; y = t; }
                    const double r = y / x;          // x > 0: |p| > 0 here
                    gamma = x * sqrt(1 + r * r);
                }
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    sn = sqrt(delta / gamma);
                    cs = p / (gamma * sn * 2);
                } else {
                    cs = sqrt((gamma + beta) / (gamma * 2));
                    sn = p / (gamma * cs * 2);
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double t0 = cs * c[i][k] + sn * c[j][k], t1 = -sn * c[i][k] + cs * c[j][k];
                    c[i][k] = t0; c[j][k] = t1;
                    a += t0 * t0; b += t1 * t1;
                    const double s0 = cs * v[i][k] + sn * v[j][k], s1 = -sn * v[i][k] + cs * v[j][k];
                    v[i][k] = s0; v[j][k] = s1;
                }
                w[i] = a; w[j] = b;
                changed = true;
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = sqrt(sim3_dot(c[i], c[i]));
    // descending sigma: a three-element network of compare-and-swaps, constant indices
#define SIM3_CSWAP(i, j)                                                                                           \
    {                                                                                                              \
        const bool sw = w[i] < w[j];                                                                               \
        const double tw = w[i]; w[i] = sw ? w[j] : w[i]; w[j] = sw ? tw : w[j];                                    \
        _Pragma("unroll") for (int k = 0; k < 3; k++) {                                                            \
            const double tc = c[i][k], tv = v[i][k];                                                               \
            c[i][k] = sw ? c[j][k] : tc; c[j][k] = sw ? tc : c[j][k];                                              \
            v[i][k] = sw ? v[j][k] : tv; v[j][k] = sw ? tv : v[j][k];                                              \
        }                                                                                                          \
    }
    SIM3_CSWAP(0, 1) SIM3_CSWAP(0, 2) SIM3_CSWAP(1, 2)
#undef SIM3_CSWAP
    double u1[3], u2[3], u3[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { u1[k] = c[0][k] / w[0]; u2[k] = c[1][k] / w[1]; }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double detv = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                        v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    const double sg = detv < 0 ? -1. : 1.;
    const double s = (w[0] + w[1] + sg * sim3_dot(u3, c[2])) / var_b;
    M[0] = s;
    bool fin = isfinite(s);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) { M[1 + 3 * r + k] = u1[r] * v[0][k] + u2[r] * v[1][k] + sg * u3[r] * v[2][k]; fin = fin && isfinite(M[1 + 3 * r + k]); }
#pragma unroll
    for (int r = 0; r < 3; r++) { M[10 + r] = ac[r] - s * sim3_dot(M + 1 + 3 * r, bc); fin = fin && isfinite(M[10 + r]); }
    return var_b > 0 && fin && s > 0;
}

// the subset check and the fit of three correspondences
__device__ __forceinline__ bool sim3_minimal(const double (*b)[3], const double (*a)[3], double* M)
{
    if (!sim3_side_ok(a[0], a[1], a[2]) || !sim3_side_ok(b[0], b[1], b[2])) return false;
    double ac[3], bc[3], H[9], var_b = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) { ac[k] = (a[0][k] + a[1][k] + a[2][k]) / 3; bc[k] = (b[0][k] + b[1][k] + b[2][k]) / 3; }
#pragma unroll
    for (int k = 0; k < 9; k++) H[k] = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double da[3] = {a[i][0] - ac[0], a[i][1] - ac[1], a[i][2] - ac[2]}, db[3] = {b[i][0] - bc[0], b[i][1] - bc[1], b[i][2] - bc[2]};
        var_b += sim3_dot(db, db);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) H[3 * r + k] += da[r] * db[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) H[k] /= 3;
    return sim3_from_moments(ac, bc, var_b / 3, H, M);
}

// e_i = |s R b_i + t - a_i|^2 in float64, compared as float32
template <bool ST>
__device__ __forceinline__ bool sim3_inlier(const Sim3Shared& sh, const double* src, const double* dst, int i, const double* M, float thr)
{
    double b[3], a[3], e = 0;
    sim3_point<ST>(sh, src, dst, i, b, a);
#pragma unroll
    for (int r = 0; r < 3; r++) { const double d = M[0] * sim3_dot(M + 1 + 3 * r, b) + M[10 + r] - a[r]; e += d * d; }
    return (float)e <= thr;
}

// K sums over the workgroup in a fixed order: the butterfly of a wavefront, then the four wavefronts in turn; every thread gets them
template <int K>
__device__ __forceinline__ void sim3_reduce(Sim3Shared& sh, double* acc)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d, 64);
    __syncthreads();                                        // the previous sums have been read
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; k++) sh.red[wave][k] = acc[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = ((sh.red[0][k] + sh.red[1][k]) + sh.red[2][k]) + sh.red[3][k];
}

template <bool ST>
__device__ __forceinline__ void sim3_problem(Sim3Shared& sh, const double* src, const double* dst, int n, int iterations, float thr, double confidence,
                                             uint64_t seed, const uint32_t* rng_tab, int rng_n, int min_inliers, double* sim, uint8_t* mask,
                                             int* ninl, int* status)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (ST) {
        for (int i = tid; i < n; i += 256)
#pragma unroll
            for (int k = 0; k < 3; k++) { sh.pts[k][i] = src[(size_t)i * 3 + k]; sh.pts[3 + k][i] = dst[(size_t)i * 3 + k]; }
        __syncthreads();
    }
    auto fail = [&](int good) {                             // no model: zeros, the count of the mask as it stands
        if (tid == 0) {
            for (int k = 0; k < 13; k++) sim[k] = 0;
            *status = VO_ERR_NO_MODEL; *ninl = good;
        }
    };
    // every thread carries the same copy of the sequential state
    int niters = iterations > 1 ? iterations : 1, max_good = 0, pos = 0;
    double best[13];
#pragma unroll
    for (int k = 0; k < 13; k++) best[k] = 0;
    if (n == 3) {                                           // model_points == npoints: one fit, every point an inlier
        double b[3][3], a[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) sim3_point<ST>(sh, src, dst, i, b[i], a[i]);
        if (sim3_minimal(b, a, best)) max_good = 3;
        if (tid < 3) mask[tid] = max_good > 0 ? 1 : 0;
    } else {
        for (int r0 = 0; r0 < niters; r0 += 64) {
            const int nh = min(64, niters - r0);
            for (int i = tid; i < SIM3_STREAM; i += 256) sh.stream[i] = pos + i < rng_n ? rng_tab[pos + i] % (uint32_t)n : 0u;
            __syncthreads();
            // subset h starts where subset h - 1 stopped in the RNG stream; a repeated index costs extra numbers, so the 64 lanes of
            // wave 0 draw in parallel from assumed starts (3 numbers per earlier subset), a prefix sum of the numbers actually used
            // gives the true starts, and the lanes repeat until the starts stop moving
            if (wave == 0) {
                int start = 3 * lane, used = 3;
                for (;;) {
                    int idx[3];
                    used = 0;
                    if (lane < nh) {
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            int v; bool dup;
                            do {
                                const int at = start + used;
                                if (at < SIM3_STREAM && pos + at < rng_n) v = (int)sh.stream[at];
                                else {                      // beyond the staged window / table: recompute directly
                                    uint64_t st = seed ? seed : 0xffffffffULL;
                                    uint32_t x = 0;
                                    if (pos + at < rng_n) x = rng_tab[pos + at];
                                    else { for (int q = 0; q <= pos + at; q++) x = sim3_rng_next(&st); }
                                    v = (int)(x % (uint32_t)n);
                                }
                                used++;
                                dup = false;
#pragma unroll
                                for (int k = 0; k < 3; k++) dup |= k < i && idx[k] == v;
                            } while (dup);
                            idx[i] = v;
                        }
#pragma unroll
                        for (int i = 0; i < 3; i++) sh.sub[lane][i] = idx[i];
                    }
                    int inc = used;                          // inclusive prefix of the numbers used
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
                    const int true_start = inc - used;
                    const bool moved = lane < nh && true_start != start;
                    start = true_start;
                    if (lane == 63) sh.used = inc;
                    if (!__any(moved)) break;
                }
            }
            __syncthreads();
            pos += sh.used;
            if (wave == 0 && lane < nh) {                   // one closed-form fit per lane
                double b[3][3], a[3][3], M[13];
#pragma unroll
                for (int i = 0; i < 3; i++) sim3_point<ST>(sh, src, dst, sh.sub[lane][i], b[i], a[i]);
                const bool ok = sim3_minimal(b, a, M);
#pragma unroll
                for (int k = 0; k < 13; k++) sh.model[lane][k] = M[k];
                sh.ok[lane] = ok ? 1 : 0;
            }
            __syncthreads();
            bool done = false;
            for (int bt = 0; bt * 4 < nh && !done; bt++) {  // four hypotheses at a time, consumed in order
                const int h = bt * 4 + wave;
                if (h < nh) {
                    int good = 0;
                    if (sh.ok[h]) {                         // a rejected sample is an iteration without a model
                        double M[13];
#pragma unroll
                        for (int k = 0; k < 13; k++) M[k] = sh.model[h][k];
                        for (int base = 0; base < n; base += 64) {
                            const int i = base + lane;
                            const bool in = i < n && sim3_inlier<ST>(sh, src, dst, i, M, thr);
                            good += __popcll(__ballot(in));
                        }
                    }
                    if (lane == 0) sh.cnt[bt & 1][wave] = good;
                }
                __syncthreads();
                for (int w = 0; w < 4; w++) {
                    const int h2 = bt * 4 + w;
                    if (h2 >= nh) break;
                    if (r0 + h2 >= niters) { done = true; break; }
                    const int good = sh.cnt[bt & 1][w];
                    if (good > max(max_good, 2)) {
#pragma unroll
                        for (int k = 0; k < 13; k++) best[k] = sh.model[h2][k];
                        max_good = good;
                        niters = sim3_update_num_iters(confidence, (double)(n - good) / n, 3, niters);
                    }
                }
            }
            __syncthreads();
        }
        // the mask of the best RANSAC model; thread t writes, and later reads, points t, t + 256, ...
        for (int i = tid; i < n; i += 256) mask[i] = max_good > 0 && sim3_inlier<ST>(sh, src, dst, i, best, thr) ? 1 : 0;
    }
    if (max_good <= 0 || max_good < min_inliers) { fail(max_good); return; }
    // the same fit over the inliers: centroids first, then the centred moments
    const double m = (double)max_good;
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = 0;
    for (int i = tid; i < n; i += 256)
        if (mask[i]) {
            double b[3], a[3];
            sim3_point<ST>(sh, src, dst, i, b, a);
#pragma unroll
            for (int k = 0; k < 3; k++) { acc[k] += a[k]; acc[3 + k] += b[k]; }
        }
    sim3_reduce<6>(sh, acc);
    const double ac[3] = {acc[0] / m, acc[1] / m, acc[2] / m}, bc[3] = {acc[3] / m, acc[4] / m, acc[5] / m};
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = 0;
    for (int i = tid; i < n; i += 256)
        if (mask[i]) {
            double b[3], a[3];
            sim3_point<ST>(sh, src, dst, i, b, a);
            const double da[3] = {a[0] - ac[0], a[1] - ac[1], a[2] - ac[2]}, db[3] = {b[0] - bc[0], b[1] - bc[1], b[2] - bc[2]};
            acc[9] += sim3_dot(db, db);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) acc[3 * r + k] += da[r] * db[k];
        }
    sim3_reduce<10>(sh, acc);
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] /= m;
    double M[13];
    const bool ok = sim3_from_moments(ac, bc, acc[9], acc, M);
    if (!ok) { fail(max_good); return; }
    if (tid == 0) {
        for (int k = 0; k < 13; k++) sim[k] = M[k];
        *status = VO_OK; *ninl = max_good;
    }
}

__global__ __launch_bounds__(256) void k_sim3_ransac(const double* src_all, const double* dst_all, const int* offsets, int off_stride, int iterations,
                                                     double max_error, double confidence, uint64_t seed, const uint32_t* rng_tab, int rng_n,
                                                     int min_inliers, double* sim_out, uint8_t* mask_all, int* ninl_out, int* status_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn_sim3[];   // more than the static limit
    Sim3Shared& sh = *(Sim3Shared*)s_dyn_sim3;
    const int pb = blockIdx.x, tid = threadIdx.x;
    const int o0 = offsets[pb * off_stride], n = offsets[pb * off_stride + 1] - o0;
    const double* src = src_all + (size_t)o0 * 3; const double* dst = dst_all + (size_t)o0 * 3;
    uint8_t* mask = mask_all + o0;
    double* sim = sim_out + (size_t)pb * 13;
    if (n < 3) {
        if (tid == 0) {
            for (int k = 0; k < 13; k++) sim[k] = 0;
            status_out[pb] = VO_ERR_TOO_FEW; ninl_out[pb] = 0;
        }
        for (int i = tid; i < n; i += 256) mask[i] = 0;
        return;
    }
    const float thr = (float)(max_error * max_error);
    if (n <= SIM3_LDS_PTS)
        sim3_problem<true>(sh, src, dst, n, iterations, thr, confidence, seed, rng_tab, rng_n, min_inliers, sim, mask, ninl_out + pb, status_out + pb);
    else
        sim3_problem<false>(sh, src, dst, n, iterations, thr, confidence, seed, rng_tab, rng_n, min_inliers, sim, mask, ninl_out + pb, status_out + pb);
}

void launch_sim3_ransac(hipStream_t s, const double* src, const double* dst, const int* offsets, int off_stride, int B, int iterations, double max_error,
                        double confidence, uint64_t seed, const uint32_t* rng_tab, int rng_n, int min_inliers, double* sim, uint8_t* mask, int* ninl,
                        int* status)
{
    if (B <= 0) return;
    static_assert(sizeof(Sim3Shared) <= 160 * 1024, "one workgroup's LDS");
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_sim3_ransac, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Sim3Shared)); attr = true; }
    hipLaunchKernelGGL(k_sim3_ransac, dim3(B), dim3(256), sizeof(Sim3Shared), s, src, dst, offsets, off_stride, iterations, max_error, confidence, seed,
                       rng_tab, rng_n, min_inliers, sim, mask, ninl, status);
}

// ================================================================== place recognition (vo_vocab_*, vo_places_*; include/vo_hip.h)
//   k_vocab_store        K rows into the vocabulary, through the map's stores (map_store_row_sift / _orb)
//   k_vocab_assign[_orb] the nearest word of every row of F slots: the bodies above, A = a slot's rows, B = the vocabulary
//   k_vocab_accumulate   per word the rows assigned and their bit counts / component sums (int32 atomics: the order cannot matter),
//                        and the number of rows that changed their word
//   k_vocab_update       the majority word / the rounded mean, stored as k_vocab_store stores
//   k_places_hist        a frame's saturated word counts, their sum and the caller's id: one entry of the index
//   k_places_score       shared(q, d) of a block of queries against a range of entries on v_sad_u8, the best top_k per query
//   k_places_merge       the ranges' lists into the answer
// No floating point in any of them.
__global__ __launch_bounds__(256) void k_vocab_store(MapBuf v, const uint8_t* src, const int* key)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (v.D == 128) {
        for (int w = blockIdx.x * 4 + (tid >> 6); w < v.npt; w += gridDim.x * 4)
            map_store_row_sift(v, w, src + (size_t)(key ? key[w] : w) * 128, lane);
    } else {
        for (int w = blockIdx.x * 32 + (tid >> 3); w < v.npt; w += gridDim.x * 32)
            map_store_row_orb(v, w, src + (size_t)(key ? key[w] : w) * 32, tid & 7);
    }
}

void launch_vocab_store(hipStream_t s, VocabBuf vb, const uint8_t* src, const int* key)
{
    const int per = vb.v.D == 128 ? 4 : 32;
    hipLaunchKernelGGL(k_vocab_store, dim3((vb.v.npt + per - 1) / per), dim3(256), 0, s, vb.v, src, key);
}

// workgroup b: rows blk NM_BLOCK_ROWS .. of query q = b / blocks
__global__ __launch_bounds__(NM_THREADS) void k_vocab_assign(VocabBuf vb, const uint8_t* desc_x, const int* norms, const int* kp_count, int kp_cap, int cap_x,
                                                             int blocks)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_b[2][NM_STAGE_ROWS * 128];
    const int q = blockIdx.x / blocks, row0 = (blockIdx.x % blocks) * NM_BLOCK_ROWS;
    const int slot = vb.slots[q], nq = min(kp_count[slot], kp_cap);
    if (row0 >= nq) return;
    nn_map_l2_body(s_b, desc_x + (size_t)slot * cap_x * 128, norms + (size_t)slot * cap_x, nq, vb.v.img, vb.v.norms, vb.v.npt, row0,
                   vb.word + (size_t)q * kp_cap, nullptr);
}

__global__ __launch_bounds__(256) void k_vocab_assign_orb(VocabBuf vb, const uint8_t* desc, const int* kp_count, int kp_cap, int blocks)
{
    __shared__ uint4 s_b[NO_TILE * 2];
    const int q = blockIdx.x / blocks, row0 = (blockIdx.x % blocks) * NO_BLOCK_ROWS;
    const int slot = vb.slots[q], nq = min(kp_count[slot], kp_cap);
    if (row0 >= nq) return;
    nn_map_hamming_body(s_b, desc + (size_t)slot * kp_cap * 32, nq, vb.v.rows, vb.v.npt, row0, vb.word + (size_t)q * kp_cap, nullptr);
}

void launch_vocab_assign(hipStream_t s, VocabBuf vb, int F, const uint8_t* desc, const uint8_t* desc_x, const int* norms, const int* kp_count,
                         int kp_cap, int cap_x)
{
    if (F <= 0) return;
    const int blocks = (kp_cap + NM_BLOCK_ROWS - 1) / NM_BLOCK_ROWS;
    if (vb.v.D == 128) hipLaunchKernelGGL(k_vocab_assign, dim3((unsigned)F * blocks), dim3(NM_THREADS), 0, s, vb, desc_x, norms, kp_count, kp_cap, cap_x, blocks);
    else hipLaunchKernelGGL(k_vocab_assign_orb, dim3((unsigned)F * blocks), dim3(256), 0, s, vb, desc, kp_count, kp_cap, blocks);
}

// Row g = q kp_cap + i of the call's slots, a wavefront (SIFT: lane l adds components 2 l, 2 l + 1) or eight lanes (ORB: lane `part`
// adds the set bits of bytes 4 part .. 4 part + 3; bit b of the row is bit b % 8 of byte b / 8) per row.
__global__ __launch_bounds__(256) void k_vocab_accumulate(VocabBuf vb, int F, const uint8_t* desc, const int* kp_count, int kp_cap)
{
    const int tid = threadIdx.x;
    const bool l2 = vb.v.D == 128;
    const int per = l2 ? 4 : 32, sub = l2 ? tid >> 6 : tid >> 3, part = l2 ? tid & 63 : tid & 7;
    const long long total = (long long)F * kp_cap;
    for (long long g = (long long)blockIdx.x * per + sub; g < total; g += (long long)gridDim.x * per) {
        const int q = (int)(g / kp_cap), i = (int)(g % kp_cap), slot = vb.slots[q];
        if (i >= min(kp_count[slot], kp_cap)) continue;
        const int w = vb.word[g];
        if (part == 0) {
            if (vb.prev[g] != w) atomicAdd(vb.changed, 1);
            vb.prev[g] = w;
            atomicAdd(vb.cnt + w, 1);
        }
        if (l2) {
            const unsigned v = *(const uint16_t*)(desc + ((size_t)slot * kp_cap + i) * 128 + 2 * part);
            if (v & 255u) atomicAdd(vb.acc + (size_t)w * 128 + 2 * part, (int)(v & 255u));
            if (v >> 8) atomicAdd(vb.acc + (size_t)w * 128 + 2 * part + 1, (int)(v >> 8));
        } else {
            uint32_t bits = *(const uint32_t*)(desc + ((size_t)slot * kp_cap + i) * 32 + 4 * part);
            int* a = vb.acc + (size_t)w * 256 + 32 * part;
            while (bits) { const int b = __ffs(bits) - 1; bits &= bits - 1; atomicAdd(a + b, 1); }
        }
    }
}

void launch_vocab_accumulate(hipStream_t s, VocabBuf vb, int F, const uint8_t* desc, const int* kp_count, int kp_cap)
{
    if (F <= 0) return;
    const int per = vb.v.D == 128 ? 4 : 32;
    const long long g = ((long long)F * kp_cap + per - 1) / per;
    hipLaunchKernelGGL(k_vocab_accumulate, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(256), 0, s, vb, F, desc, kp_count, kp_cap);
}

// Word w with c = cnt[w] > 0 rows: ORB bit b = 1 iff 2 ones_b > c (a tie gives 0); SIFT component j = (2 sum_j + c) / (2 c).  The new
// row goes to vb.tmp and from there through the map's store, by the lanes that wrote it; a word without rows keeps its row.
__global__ __launch_bounds__(256) void k_vocab_update(VocabBuf vb)
{
    const int tid = threadIdx.x;
    if (vb.v.D == 128) {
        const int lane = tid & 63;
        for (int w = blockIdx.x * 4 + (tid >> 6); w < vb.v.npt; w += gridDim.x * 4) {
            const int c = vb.cnt[w];
            if (c <= 0) continue;
            const int u0 = (2 * vb.acc[(size_t)w * 128 + 2 * lane] + c) / (2 * c), u1 = (2 * vb.acc[(size_t)w * 128 + 2 * lane + 1] + c) / (2 * c);
            uint8_t* row = vb.tmp + (size_t)w * 128;
            *(uint16_t*)(row + 2 * lane) = (uint16_t)(u0 | (u1 << 8));
            map_store_row_sift(vb.v, w, row, lane);
        }
    } else {
        const int part = tid & 7;
        for (int w = blockIdx.x * 32 + (tid >> 3); w < vb.v.npt; w += gridDim.x * 32) {
            const int c = vb.cnt[w];
            if (c <= 0) continue;
            const int* a = vb.acc + (size_t)w * 256 + 32 * part;
            uint32_t bits = 0;
#pragma unroll 8
            for (int b = 0; b < 32; b++) bits |= (2 * a[b] > c ? 1u : 0u) << b;
            uint8_t* row = vb.tmp + (size_t)w * 32;
            *(uint32_t*)(row + 4 * part) = bits;
            map_store_row_orb(vb.v, w, row, part);
        }
    }
}

void launch_vocab_update(hipStream_t s, VocabBuf vb)
{
    const int per = vb.v.D == 128 ? 4 : 32;
    hipLaunchKernelGGL(k_vocab_update, dim3((vb.v.npt + per - 1) / per), dim3(256), 0, s, vb);
}

// ------------------------------------------------------------------ the keyframe index
#define PL_MAX_K 4096
// entry q of the call: hist[w] = min(255, rows of slot slots[q] whose word is w), sum = the sum of those bytes, id = ids[q]
__global__ __launch_bounds__(256) void k_places_hist(VocabBuf vb, const int* kp_count, int kp_cap, uint8_t* hist, int* sum, int* id)
{
    __shared__ int s_h[PL_MAX_K];
    __shared__ int s_w[4];
    const int q = blockIdx.x, tid = threadIdx.x, K = vb.v.npt;
    const int nq = min(kp_count[vb.slots[q]], kp_cap);
    for (int w = tid; w < K; w += 256) s_h[w] = 0;
    __syncthreads();
    for (int i = tid; i < nq; i += 256) atomicAdd(&s_h[vb.word[(size_t)q * kp_cap + i]], 1);
    __syncthreads();
    int s = 0;
    for (int w4 = tid; w4 < K / 4; w4 += 256) {
        uint32_t pk = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const int c = min(255, s_h[4 * w4 + k]); s += c; pk |= (uint32_t)c << (8 * k); }
        *(uint32_t*)(hist + (size_t)q * K + 4 * w4) = pk;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) { sum[q] = s_w[0] + s_w[1] + s_w[2] + s_w[3]; id[q] = vb.ids[q]; }
}

void launch_places_hist(hipStream_t s, VocabBuf vb, int F, const int* kp_count, int kp_cap, uint8_t* hist, int* sum, int* id)
{
    if (F <= 0) return;
    hipLaunchKernelGGL(k_places_hist, dim3(F), dim3(256), 0, s, vb, kp_count, kp_cap, hist, sum, id);
}

// sum[e] of n given histograms, a wavefront each
__global__ __launch_bounds__(256) void k_places_sums(const uint8_t* hist, int K, int n, int* sum)
{
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= n) return;
    unsigned s = 0;
    for (int w4 = lane; w4 < K / 4; w4 += 64) s = __builtin_amdgcn_sad_u8(*(const uint32_t*)(hist + (size_t)e * K + 4 * w4), 0u, s);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) sum[e] = (int)s;
}

void launch_places_sums(hipStream_t s, const uint8_t* hist, int K, int n, int* sum)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_places_sums, dim3((n + 3) / 4), dim3(256), 0, s, hist, K, n, sum);
}

// ------------------------------------------------------------------ k_places_score: shared(q, d) = (sum_q + sum_d - L1(q, d)) / 2
// A workgroup takes PQ_T query entries and the entries [sp per_split, (sp + 1) per_split) of the index, PQ_T at a time.  For a tile
// of PQ_T x PQ_T pairs the histograms pass through LDS PQ_KC bytes of every row at a time (row pitch PQ_LD: the 16 rows a quarter
// wavefront reads with one ds_read_b128 lie in 16 different bank groups); thread (ty, tx) holds the L1 sums of queries i 16 + ty and
// entries j 16 + tx, i, j < 4, four bytes per v_sad_u8.  The tile's sums then go to LDS and lane q of wave 0 takes query q's 64
// candidates in ascending entry order into its list of the best top_k keys (shared << 32 | ~entry: larger shared first, then the
// lower entry), kept descending in LDS.  An entry never meets itself; |id_q - id_d| < min_gap (64-bit) and shared < min_shared drop
// a candidate.  Key 0 is no candidate: ~entry is never 0.
#define PQ_T 64
#define PQ_KC 256
#define PQ_LD (PQ_KC + 16)
__global__ __launch_bounds__(256) void k_places_score(PlacesQuery p)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_q[PQ_T * PQ_LD];
    __shared__ __attribute__((aligned(16))) uint8_t s_e[PQ_T * PQ_LD];
    __shared__ int s_l1[PQ_T][PQ_T + 1];
    __shared__ unsigned long long s_top[16][PQ_T];
    __shared__ int s_qe[PQ_T], s_qs[PQ_T], s_qid[PQ_T], s_es[PQ_T], s_eid[PQ_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int q0 = (blockIdx.x / p.splits) * PQ_T, sp = blockIdx.x % p.splits;
    const int e_begin = sp * p.per_split, e_end = min(p.n, e_begin + p.per_split);
    if (tid < PQ_T) {
        const int e = q0 + tid < p.Q ? p.qent[q0 + tid] : -1;
        s_qe[tid] = e; s_qs[tid] = e >= 0 ? p.sum[e] : 0; s_qid[tid] = e >= 0 ? p.id[e] : 0;
    }
    for (int i = tid; i < 16 * PQ_T; i += 256) (&s_top[0][0])[i] = 0ull;
    __syncthreads();
    for (int e0 = e_begin; e0 < e_end; e0 += PQ_T) {
        if (tid < PQ_T) {                                   // wave 0, after its selection of the tile before
            const int d = e0 + tid;
            s_es[tid] = d < e_end ? p.sum[d] : 0; s_eid[tid] = d < e_end ? p.id[d] : 0;
        }
        unsigned acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = 0u;
        for (int k0 = 0; k0 < p.K; k0 += PQ_KC) {
            __syncthreads();                                // the stage before has been read (and wave 0 has left its selection)
#pragma unroll
            for (int t = tid; t < 2 * PQ_T * (PQ_KC / 16); t += 256) {
                const int r = (t >> 4) & (PQ_T - 1), c = t & 15;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (t < PQ_T * (PQ_KC / 16)) {
                    const int e = s_qe[r];
                    if (e >= 0) v = *(const uint4*)(p.hist + (size_t)e * p.K + k0 + c * 16);
                    *(uint4*)(s_q + r * PQ_LD + c * 16) = v;
                } else {
                    const int e = e0 + r;
                    if (e < e_end) v = *(const uint4*)(p.hist + (size_t)e * p.K + k0 + c * 16);
                    *(uint4*)(s_e + r * PQ_LD + c * 16) = v;
                }
            }
            __syncthreads();
#pragma unroll 2
            for (int c = 0; c < PQ_KC / 16; c++) {
                uint4 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; i++) { a[i] = *(const uint4*)(s_q + (i * 16 + ty) * PQ_LD + c * 16); b[i] = *(const uint4*)(s_e + (i * 16 + tx) * PQ_LD + c * 16); }
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        unsigned s = acc[i][j];
                        s = __builtin_amdgcn_sad_u8(a[i].x, b[j].x, s); s = __builtin_amdgcn_sad_u8(a[i].y, b[j].y, s);
                        s = __builtin_amdgcn_sad_u8(a[i].z, b[j].z, s); s = __builtin_amdgcn_sad_u8(a[i].w, b[j].w, s);
                        acc[i][j] = s;
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) s_l1[i * 16 + ty][j * 16 + tx] = (int)acc[i][j];
        __syncthreads();
        if (tid < PQ_T && s_qe[tid] >= 0) {
            const int qe = s_qe[tid], qs = s_qs[tid], lim = min(PQ_T, e_end - e0);
            const long long qid = s_qid[tid];
            unsigned long long worst = s_top[p.top_k - 1][tid];
            for (int e = 0; e < lim; e++) {
                const int d = e0 + e;
                if (d == qe) continue;
                long long gap = qid - (long long)s_eid[e];
                gap = gap < 0 ? -gap : gap;
                if (gap < (long long)p.min_gap) continue;
                const int sh = (qs + s_es[e] - s_l1[tid][e]) >> 1;
                if (sh < p.min_shared) continue;
                const unsigned long long key = ((unsigned long long)(unsigned)sh << 32) | (unsigned)~(unsigned)d;
                if (key <= worst) continue;
                int pos = p.top_k - 1;
                while (pos > 0 && s_top[pos - 1][tid] < key) { s_top[pos][tid] = s_top[pos - 1][tid]; pos--; }
                s_top[pos][tid] = key;
                worst = s_top[p.top_k - 1][tid];
            }
        }
    }
    __syncthreads();
    if (tid < PQ_T && q0 + tid < p.Q)
        for (int k = 0; k < 16; k++) p.part[((size_t)(q0 + tid) * p.splits + sp) * 16 + k] = k < p.top_k ? s_top[k][tid] : 0ull;
}

// query q's lists of all splits (their entries are disjoint, so no key repeats) -> its top_k, a wavefront per query
__global__ __launch_bounds__(256) void k_places_merge(PlacesQuery p)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= p.Q) return;
    const unsigned long long* src = p.part + (size_t)q * p.splits * 16;
    const int n = p.splits * 16;
    unsigned long long k[VO_PLACES_MAX_SPLITS * 16 / 64];
#pragma unroll
    for (int t = 0; t < VO_PLACES_MAX_SPLITS * 16 / 64; t++) k[t] = t * 64 + lane < n ? src[t * 64 + lane] : 0ull;
    for (int r = 0; r < p.top_k; r++) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int t = 0; t < VO_PLACES_MAX_SPLITS * 16 / 64; t++) m = k[t] > m ? k[t] : m;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        if (lane == 0) {
            p.out_entry[(size_t)q * p.top_k + r] = m ? (int)~(unsigned)(m & 0xffffffffull) : -1;
            p.out_shared[(size_t)q * p.top_k + r] = (int)(m >> 32);
        }
#pragma unroll
        for (int t = 0; t < VO_PLACES_MAX_SPLITS * 16 / 64; t++) k[t] = k[t] == m ? 0ull : k[t];
    }
}

void launch_places_query(hipStream_t s, PlacesQuery p)
{
    if (p.Q <= 0) return;
    const int qblocks = (p.Q + PQ_T - 1) / PQ_T;
    hipLaunchKernelGGL(k_places_score, dim3((unsigned)qblocks * p.splits), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_places_merge, dim3((p.Q + 3) / 4), dim3(256), 0, s, p);
}
