// The top-k selection of propagate.hip (video label propagation) and knn.hip (k-NN retrieval from a memory bank): ONE copy of all that
// turns the pair walk's scores (pair_common.h) into a selection, its weights and its debug outputs, so both operators select, order and
// weigh by the same arithmetic bit for bit.  The operators keep what differs: which rows a workgroup walks, which keys a query may take,
// how a key becomes its index g, and where the labels of g are.
//   scores kernel   one workgroup owns 64 queries and one of G groups of keys (a context frame, a bank range).  A lane owns one query
//                   and 16 keys of a block; a key the operator admits goes into the lane's own sorted list of k (score, g) in LDS behind
//                   the walk's panes ([slot][thread]: conflict-free), gated by the list's last entry in registers (sel_insert).  At the
//                   end thread q < 64 merges the four lists of query q under the total order into the scratch (sel_merge4): [G][N][k]
//                   fp32 scores, then [G][N][k] int32 indices, -1 marking an empty slot.
//   merge kernel    one wave per query: the G k <= 256 candidates sit 4 to a lane as 64-bit keys (order-preserving score bits, then
//                   ~g), k rounds of a wave maximum select rank 0 .. K'-1 (sel_wave_select); the weights exp2((s - s_0) a), a = log2(e)
//                   / tau, their sum W and 1 / W are wave-uniform.  The operator gathers its labels; sel_write_topk writes the rest.
#pragma once
#include "pair_common.h"

#include <climits>
#include <cmath>

namespace dseg {

constexpr int SEL_EMPTY = INT_MAX;              // g of an empty list slot (score -inf): after every candidate in the total order
constexpr int SEL_MAX_K = 16;                   // k of either operator; G k <= 256 = 4 keys for each lane of the merge's wave

// (score, g) as one unsigned key whose order is the total order: larger = earlier.  0 = no candidate.
__device__ __forceinline__ unsigned long long prp_key(float s, int g) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)g);
}
__device__ __forceinline__ float prp_key_score(unsigned long long key) {
    const uint32_t o = (uint32_t)(key >> 32);
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// ---- the scores kernel ----------------------------------------------------------------------------------------------------------
// the walk's block_begin and slice body: lo.hi + hi.lo + hi.hi into one accumulator, keys as the MFMA's rows
__device__ __forceinline__ void sel_zero(f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}
__device__ __forceinline__ void sel_slice(f32x16& acc, bf16x8 qhi, bf16x8 qlo, bf16x8 khi, bf16x8 klo) {
    acc = mfma32f<FMT_FP16>(klo, qhi, acc);
    acc = mfma32f<FMT_FP16>(khi, qlo, acc);
    acc = mfma32f<FMT_FP16>(khi, qhi, acc);
}

// an accumulator register as a score (+ 0: a negative zero becomes the positive one)
__device__ __forceinline__ float sel_score(float acc) { return acc * PAIR_UNSCALE + 0.f; }

struct SelLists {
    float* ls;                                  // [k][256] scores of the lanes' lists, best first
    int* lg;                                    // [k][256] their indices g
    float* my_ls;                               // the lane's own list: slot s at [s * 256]
    int* my_lg;
    float thr_s;                                // the list's last entry: what a candidate must beat
    int thr_g;
    int k;
};

// the workgroup's lists behind the walk's panes (lds: sel_lds_bytes(k)), every one empty
__device__ __forceinline__ SelLists sel_lists(char* lds, int k) {
    const int tid = threadIdx.x;
    SelLists L;
    L.ls = reinterpret_cast<float*>(lds + PAIR_STAGE);
    L.lg = reinterpret_cast<int*>(lds + PAIR_STAGE + k * 1024);
    for (int s = 0; s < k; ++s) {
        L.ls[s * 256 + tid] = -INFINITY;
        L.lg[s * 256 + tid] = SEL_EMPTY;
    }
    L.my_ls = L.ls + tid;
    L.my_lg = L.lg + tid;
    L.thr_s = -INFINITY;
    L.thr_g = SEL_EMPTY;
    L.k = k;
    return L;
}

// candidate (s, g) of the lane's query: into the lane's list if it beats the last entry
__device__ __forceinline__ void sel_insert(SelLists& L, float s, int g) {
    if (!better(s, g, L.thr_s, L.thr_g)) return;
    int pos = L.k - 1;                                                  // the last entry leaves
    while (pos > 0) {
        const float ps = L.my_ls[(pos - 1) * 256];
        const int pg = L.my_lg[(pos - 1) * 256];
        if (!better(s, g, ps, pg)) break;
        L.my_ls[pos * 256] = ps;
        L.my_lg[pos * 256] = pg;
        --pos;
    }
    L.my_ls[pos * 256] = s;
    L.my_lg[pos * 256] = g;
    L.thr_s = L.my_ls[(L.k - 1) * 256];
    L.thr_g = L.my_lg[(L.k - 1) * 256];
}

// thread q < 64, after a barrier behind the walk: the lists of the tile's query q -- waves (qh, 0) and (qh, 1), both lane halves -- 4-way
// under the total order into the query's k slots of the scratch
__device__ __forceinline__ void sel_merge4(const SelLists& L, int q, float* __restrict__ out_s, int* __restrict__ out_g) {
    const float* ls = L.ls;
    const int* lg = L.lg;
    const int t0 = ((q >> 5) * 2) * 64 + (q & 31), t1 = t0 + 32, t2 = t0 + 64, t3 = t0 + 96;
    int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    for (int i = 0; i < L.k; ++i) {
        // (a list's head index reaches k only after k picks from it: the loop has ended by then)
        float bs = ls[p0 * 256 + t0];
        int bg = lg[p0 * 256 + t0], which = 0;
        const float s1 = ls[p1 * 256 + t1], s2 = ls[p2 * 256 + t2], s3 = ls[p3 * 256 + t3];
        const int g1 = lg[p1 * 256 + t1], g2 = lg[p2 * 256 + t2], g3 = lg[p3 * 256 + t3];
        if (better(s1, g1, bs, bg)) { bs = s1; bg = g1; which = 1; }
        if (better(s2, g2, bs, bg)) { bs = s2; bg = g2; which = 2; }
        if (better(s3, g3, bs, bg)) { bs = s3; bg = g3; which = 3; }
        p0 += which == 0;
        p1 += which == 1;
        p2 += which == 2;
        p3 += which == 3;
        out_s[i] = bs;
        out_g[i] = bg == SEL_EMPTY ? -1 : bg;
    }
}

// ---- the merge kernel -----------------------------------------------------------------------------------------------------------
// the selections of a workgroup's four waves, in rank order: written by lane 0, read by the wave after a barrier
struct alignas(16) SelPicks {
    float w[4][SEL_MAX_K];                      // exp2((s - s_0) a), not yet divided by W
    int g[4][SEL_MAX_K];
};
struct SelSum { int kept; float W; };           // K' <= k selected, the sum of their weights in rank order

// One wave selects for query q from the [G][N][k] scratch; a wave with q >= N selects nothing.  picked(i, g), on lane 0 alone: rank i
// went to g.  A barrier makes the picks readable.
template <class Picked>
__device__ __forceinline__ SelSum sel_wave_select(const float* __restrict__ cand_s, const int* __restrict__ cand_g, int G, int N, int q,
                                                  int k, float a, SelPicks& picks, Picked picked) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    SelSum sum = {0, 0.f};
    if (q >= N) return sum;
    unsigned long long key[4];
    const int ncand = G * k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        key[j] = 0;
        if (e < ncand) {
            const int gi = e / k, i = e - gi * k;
            const size_t at = ((size_t)gi * N + q) * k + i;
            const int g = cand_g[at];
            if (g >= 0) key[j] = prp_key(cand_s[at], g);
        }
    }
    float s0 = 0.f;
    for (int i = 0; i < k; ++i) {
        unsigned long long m = key[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) m = key[j] > m ? key[j] : m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o);
            m = other > m ? other : m;
        }
        if (m == 0) break;                                              // K' = i candidates in all (wave-uniform)
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = key[j] == m ? 0 : key[j];   // (g is unique: exactly one slot of one lane)
        const float s = prp_key_score(m);
        if (i == 0) s0 = s;
        const float w = __builtin_amdgcn_exp2f((s - s0) * a);
        sum.W += w;
        if (lane == 0) {
            const int g = (int)(0xFFFFFFFFu - (uint32_t)m);
            picks.w[wave][i] = w;
            picks.g[wave][i] = g;
            picked(i, g);
        }
        sum.kept = i + 1;
    }
    return sum;
}

// the factor of every output: 1 / W correctly rounded
__device__ __forceinline__ float sel_inv(float W) { return __fdiv_rn(1.f, W); }

// the debug outputs of query q (each nullable): the selected indices and their normalized weights in rank order, -1 / 0 beyond K'
__device__ __forceinline__ void sel_write_topk(const SelPicks& picks, int kept, float inv, int q, int k, int32_t* __restrict__ topk_idx,
                                               float* __restrict__ topk_w) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < k) {
        if (topk_idx) topk_idx[(size_t)q * k + lane] = lane < kept ? picks.g[wave][lane] : -1;
        if (topk_w) topk_w[(size_t)q * k + lane] = lane < kept ? picks.w[wave][lane] * inv : 0.f;
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
inline size_t sel_lds_bytes(int k) { return PAIR_STAGE + (size_t)k * 2048; }
inline long long sel_scratch_bytes(long long G, long long N, int k) { return G * N * k * 8; }

struct SelScratch { float* cand_s; int* cand_g; };   // [G][N][k] fp32 scores, then [G][N][k] int32 indices
inline SelScratch sel_scratch(void* scratch, long long G, long long N, int k) {
    float* cand_s = reinterpret_cast<float*>(scratch);
    return {cand_s, reinterpret_cast<int*>(cand_s + (size_t)G * N * k)};
}

// the width, the class count and k, refused in this order
inline int sel_shape_check(const char* who, int D, int C, int k, int max_k) {
    if (pair_width_check(who, D)) return -1;
    if (C < 1 || C > 256) {
        dinoseg_set_error("%s: C = %d classes (1 <= C <= 256)", who, C);
        return -1;
    }
    if (k < 1 || k > max_k) {
        dinoseg_set_error("%s: k = %d (1 <= k <= %d)", who, k, max_k);
        return -1;
    }
    return 0;
}

// the temperature as the merge kernel's a = log2(e) / tau
inline int sel_temperature(const char* who, double tau, float* a) {
    if (!(std::isfinite(tau) && tau > 0.0)) {
        dinoseg_set_error("%s: temperature %g (finite and positive)", who, tau);
        return -1;
    }
    *a = (float)(1.4426950408889634074 / tau);
    if (!std::isfinite(*a)) {
        dinoseg_set_error("%s: temperature %g is too small (log2(e) / tau exceeds fp32)", who, tau);
        return -1;
    }
    return 0;
}

}  // namespace dseg
