// sift_rows.h — the one statement of how a SIFT descriptor row lies on the device: shared by the detector (sift_batch.hip:
// k_sb_descriptor, k_sb_pack_rows) and the map store of the relocaliser (reloc_kernels.hip: k_map_gather).
#pragma once
#include "vo_internal.h"

// One finished descriptor row (integer bin values 0..255) -> everything the host and the pair stage read of it: the 128 bytes of
// `desc`, the matrix-core operand image and |v - 128|^2 for k_nn_l2i8, and the norm-bound flag.  Called by a whole wavefront; lane
// l owns elements 2 l (u0) and 2 l + 1 (u1).  The layout and the bound are stated here only: k_sb_descriptor (detected rows),
// k_sb_pack_rows (rows a caller chose) and k_map_gather (a map's rows: slot 0 of an image of its own) all end in this function.
__device__ __forceinline__ void sb_store_row(int u0, int u1, int lane, size_t slot, int id, int kp_cap, uint8_t* desc, uint8_t* desc_x, int cap_x,
                                             int* norms, int* flags)
{
    if (desc) *(uint16_t*)(desc + (slot * kp_cap + id) * 128 + 2 * lane) = (uint16_t)(u0 | (u1 << 8));
    // |v - 128|^2 summed over the row (exact integer), and the matrix-core operand image: bytes v - 128 as int8,
    // [slot][group = row / 16][chunk 0..7 = 16 elements][row % 16][16 B]
    int sq = (u0 - 128) * (u0 - 128) + (u1 - 128) * (u1 - 128), raw = u0 * u0 + u1 * u1;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) { sq += __shfl_xor(sq, dd, 64); raw += __shfl_xor(raw, dd, 64); }
    // the matrix-core matcher orders candidates by the exact integer d^2 instead of sqrtf(d^2): the same order as long as
    // d^2 < 2^22 (sqrtf is strictly increasing on those integers), which |row|^2 <= 2^20 guarantees; SIFT's normalisation
    // gives |row|^2 ~ 2^18.  A row that breaks the bound is flagged (bit 1) instead of silently matched.
    if (lane == 0 && raw > (1 << 20) && flags) atomicOr(flags + slot, 2);
    if (desc_x) {
        *(uint16_t*)(desc_x + slot * (size_t)cap_x * 128 + ((size_t)((id >> 4) * 8 + (lane >> 3)) * 16 + (id & 15)) * 16 + 2 * (lane & 7)) =
            (uint16_t)(((u0 - 128) & 255) | (((u1 - 128) & 255) << 8));
        if (lane == 0) norms[slot * cap_x + id] = sq;
    }
}
