// The split-plane pair walk of the feature-space operators, shared by propagate.hip (propagate_scores_kernel), knn.hip
// (knn_scores_kernel), kmeans.hip (kmeans_assign_kernel) and ncut.hip (ncut_graph_kernel), and the small pieces of the unit-row planes
// they all read: ONE copy of the staging, the slice order and the fragment reads, so all of them form <x_q, x_k> by the same arithmetic
// bit for bit.  What propagate.hip and knn.hip do with the scores -- the top-k selection -- is select_common.h, on top of this header.
//
// The family's geometry: one workgroup of 4 waves owns 64 query rows and walks key rows in blocks of 64.  Rows are unit rows scaled
// by 2^10 and split into fp16 hi + lo planes (split_unit); a plane's row is D halves, D a multiple of 64.  Per block and 64-wide
// slice of D the query tile and the key block, hi and lo, sit in four LDS panes of 64 rows x 128 bytes under the library's swizzle
// (tile_off_bytes): thread t stages 16 bytes (chunk t & 7) of rows t >> 3 and (t >> 3) + 32 of each pane.  The next slice's eight
// global loads are issued right after the second barrier and stay in flight under the current slice's MFMAs.  Wave (qh, kh) = (wave
// >> 1, wave & 1) reads the fragments of query rows 32 qh .. and key rows 32 kh ..: row lr = lane & 31 of its half, chunk 2 s + lh
// (lh = lane >> 5) of the 128-byte row, s = 0 .. 3, and hands them to the kernel's slice body, which issues its own three
// v_mfma_f32_32x32x16_f16 (lo.hi, hi.lo, hi.hi) in its own operand order.  Blocks and slices are walked in ascending order.
#pragma once
#include "common.h"

namespace dseg {

constexpr int PAIR_TILE = 64;                   // query rows of a workgroup, key rows of a block, halves of a slice
constexpr int PAIR_STAGE = 32768;               // the four panes: 64 rows x 128 B each
constexpr int PAIR_QHI = 0, PAIR_QLO = 8192, PAIR_KHI = 16384, PAIR_KLO = 24576;
constexpr float PAIR_UNSCALE = 0x1p-20f;        // planes carry 2^10 x: products are 2^20 <x_q, x_k>

// the widths the walk takes: whole slices of 64 halves, a row offset inside int
inline int pair_width_check(const char* who, int D) {
    if (D < 64 || D % 64 != 0 || D > 8192) {
        dinoseg_set_error("%s: width D = %d (a multiple of 64 up to 8192)", who, D);
        return -1;
    }
    return 0;
}

// the total order of the selections: score descending, index ascending
__device__ __forceinline__ bool better(float s, int i, float s2, int i2) { return s > s2 || (s == s2 && i < i2); }

// v = hi + lo in fp16 (v: a unit row's component scaled by 2^10, so that lo stays clear of the fp16 subnormals)
struct UnitSplit {
    uint16_t hi, lo;
};
__device__ __forceinline__ UnitSplit split_unit(double v) {
    const _Float16 h = (_Float16)(float)v;
    const _Float16 l = (_Float16)(float)(v - (double)(float)h);
    return {__builtin_bit_cast(uint16_t, h), __builtin_bit_cast(uint16_t, l)};
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);             // (xor tree: every lane holds the same bits)
    return v;
}

// the row that this thread stages into half h of a pane (a query row of the tile, a key row of the block)
__device__ __forceinline__ int pair_stage_row(int h) { return ((int)threadIdx.x >> 3) + 32 * h; }

// The walk over nkb key blocks x ndc slices.  lds: PAIR_STAGE bytes, 16-byte aligned.  q / k: the hi planes, their lo planes q_lo /
// k_lo elements further on.  qrow[h]: the element offset of query row pair_stage_row(h)'s start (clamped by the kernel: a row past
// the end re-reads a real one); key_row(kb * 64 + pair_stage_row(h)): the same for a key row.  Per block, in this order:
//   block_sync(kb)                  after the first barrier of the block's first slice, before the stores into the panes: everything
//                                   the workgroup wrote to LDS during the previous block is visible, and nobody reads the panes
//   block_begin()                   after the second barrier of the first slice: zero the accumulators
//   slice(qhi, qlo, khi, klo)       four times per slice of D
//   block_end(kb)                   after the last slice
// Every callable is inlined.  No barrier follows the last block_end.
template <class KeyRow, class Sync, class Begin, class Slice, class End>
__device__ __forceinline__ void pair_walk(char* lds, const uint16_t* q, size_t q_lo, const size_t (&qrow)[2], const uint16_t* k,
                                          size_t k_lo, int nkb, int ndc, KeyRow key_row, Sync block_sync, Begin block_begin, Slice slice,
                                          End block_end) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int qh = wave >> 1, kh = wave & 1, total = nkb * ndc;
    const int schunk = tid & 7;
    const int soff[2] = {tile_off_bytes(pair_stage_row(0), schunk), tile_off_bytes(pair_stage_row(1), schunk)};
    const size_t qat[2] = {qrow[0] + schunk * 8, qrow[1] + schunk * 8};
    uint4 g_qh0, g_qh1, g_ql0, g_ql1, g_kh0, g_kh1, g_kl0, g_kl1;         // the slice in flight (named: an array would live in scratch)
    auto ld16 = [](const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); };
    auto fetch = [&](int it) {
        const int kb = it / ndc;
        const size_t dofs = (size_t)(it - kb * ndc) * 64;               // (wave-uniform; the thread's chunk is in qat and added to the key row)
        const size_t q0 = qat[0] + dofs, q1 = qat[1] + dofs;
        const size_t k0 = key_row(kb * 64 + pair_stage_row(0)) + schunk * 8 + dofs;
        const size_t k1 = key_row(kb * 64 + pair_stage_row(1)) + schunk * 8 + dofs;
        g_qh0 = ld16(q + q0);
        g_qh1 = ld16(q + q1);
        g_ql0 = ld16(q + q_lo + q0);
        g_ql1 = ld16(q + q_lo + q1);
        g_kh0 = ld16(k + k0);
        g_kh1 = ld16(k + k1);
        g_kl0 = ld16(k + k_lo + k0);
        g_kl1 = ld16(k + k_lo + k1);
    };

    // fragment addresses: row lr of the wave's half, chunk 2 s + lh of the 128-byte row
    int fq[4], fk[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        fq[s] = PAIR_QHI + tile_off_bytes(qh * 32 + lr, s * 2 + lh);
        fk[s] = PAIR_KHI + tile_off_bytes(kh * 32 + lr, s * 2 + lh);
    }

    fetch(0);
    for (int it = 0; it < total; ++it) {
        const int kb = it / ndc, dc = it - kb * ndc;
        __syncthreads();                                                // everyone is done reading the previous slice
        if (dc == 0) block_sync(kb);
        *reinterpret_cast<uint4*>(lds + PAIR_QHI + soff[0]) = g_qh0;
        *reinterpret_cast<uint4*>(lds + PAIR_QHI + soff[1]) = g_qh1;
        *reinterpret_cast<uint4*>(lds + PAIR_QLO + soff[0]) = g_ql0;
        *reinterpret_cast<uint4*>(lds + PAIR_QLO + soff[1]) = g_ql1;
        *reinterpret_cast<uint4*>(lds + PAIR_KHI + soff[0]) = g_kh0;
        *reinterpret_cast<uint4*>(lds + PAIR_KHI + soff[1]) = g_kh1;
        *reinterpret_cast<uint4*>(lds + PAIR_KLO + soff[0]) = g_kl0;
        *reinterpret_cast<uint4*>(lds + PAIR_KLO + soff[1]) = g_kl1;
        __syncthreads();
        if (it + 1 < total) fetch(it + 1);
        if (dc == 0) block_begin();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bf16x8 qhi = lds_frag(lds + fq[s]), qlo = lds_frag(lds + (PAIR_QLO - PAIR_QHI) + fq[s]);
            const bf16x8 khi = lds_frag(lds + fk[s]), klo = lds_frag(lds + (PAIR_KLO - PAIR_KHI) + fk[s]);
            slice(qhi, qlo, khi, klo);
        }
        if (dc == ndc - 1) block_end(kb);
    }
}

}  // namespace dseg
