// Few-shot segmentation: k-NN label retrieval from a flat memory bank of labelled patch features, without the [N, M] score matrix.
// The rule is stated in full in include/dinoseg.h (dinoseg_op_knn_labels); in short, every query cell takes the k best-scoring live
// rows of the bank -- score and order are dinoseg_op_propagate's, without a neighbourhood test -- and averages their labels with
// weights exp((s - s_0) / tau).
//
//   knn_scores_kernel   one workgroup (4 waves) per (64 consecutive queries, one of S contiguous bank ranges).  A range is whole key
//                       blocks of 64 rows (knn_range), the last one clipped at M, walked by the family's pair walk (pair_common.h)
//                       with the slice body and the per-lane list of k (score, g) of propagate_scores_kernel: [slot][thread] in LDS,
//                       gated by the list's last entry in registers.  A query is row i / n, cell i % n of the [B][2][n][D] planes, so
//                       a tile may span frames; the bank is one "frame" of bank_rows rows.  At the end 64 threads merge the 4 lists
//                       of their query (4-way, the total order) into the scratch: [S][N][k] scores, then [S][N][k] indices.
//                       LDS: 32 KiB + 2 KiB k <= 64 KiB; no atomics; every loop bound is a function of the shapes.
//   knn_merge_kernel    one wave per query: the S k <= 256 candidates sit 4 to a lane as 64-bit keys (prp_key), k rounds of a wave
//                       maximum select rank 0 .. K'-1; weights, W, 1 / W are wave-uniform; lanes stride the C classes with k gathers
//                       and fmaf each (soft rows), or k compares against the selected rows' labels (hard labels, read once per query).
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "pair_common.h"

#include <climits>
#include <cmath>

namespace dseg {

namespace {

constexpr int KNN_EMPTY = INT_MAX;              // g of an empty list slot (score -inf): after every candidate in the total order
constexpr int KNN_MAX_SPLITS = 16;
constexpr long long KNN_MAX_ROWS = 1ll << 24;   // bank rows: g and 64 key blocks stay far inside int
constexpr long long KNN_MAX_QUERIES = (1ll << 31) - 256;

// the key blocks of split s of S over nblk blocks of 64 rows: [s nblk / S, (s + 1) nblk / S), never empty for S <= nblk
__device__ __forceinline__ int knn_range(int nblk, int S, int s) { return (int)(((long long)s * nblk) / S); }

int knn_split_cap(long long M, int k) {
    const long long nblk = (M + 63) / 64;
    long long cap = KNN_MAX_SPLITS;
    if (256 / k < cap) cap = 256 / k;
    if (nblk < cap) cap = nblk;
    return (int)cap;
}

__global__ __launch_bounds__(256) void knn_scores_kernel(const uint16_t* __restrict__ qp, int N, int n, const uint16_t* __restrict__ bank,
                                                         int M, size_t bank_lo, int D, int k, float* __restrict__ cand_s,
                                                         int* __restrict__ cand_g) {
    extern __shared__ __attribute__((aligned(16))) char knn_lds[];
    float* ls = reinterpret_cast<float*>(knn_lds + PAIR_STAGE);          // [k][256] scores of the lanes' lists, best first
    int* lg = reinterpret_cast<int*>(knn_lds + PAIR_STAGE + k * 1024);   // [k][256] their bank rows
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int qh = wave >> 1, kh = wave & 1;
    const int i0 = (int)blockIdx.x * PAIR_TILE;                         // (N <= 2^31 - 256: i0 + 63 fits)
    const int nblk = (M + 63) >> 6, S = (int)gridDim.y, si = (int)blockIdx.y;
    const int b0 = knn_range(nblk, S, si), b1 = knn_range(nblk, S, si + 1);
    const int row0 = b0 * 64, row1 = min(b1 * 64, M);                   // the range's rows: row0 .. row1 - 1, at least one

    for (int s = 0; s < k; ++s) {
        ls[s * 256 + tid] = -INFINITY;
        lg[s * 256 + tid] = KNN_EMPTY;
    }
    float* my_ls = ls + tid;                                            // the lane's own list: slot s at [s * 256]
    int* my_lg = lg + tid;
    float thr_s = -INFINITY;                                            // the list's last entry: what a candidate must beat
    int thr_g = KNN_EMPTY;

    // the lane's query in the selection
    const bool qvalid = i0 + qh * 32 + lr < N;

    // the tile's query rows as the walk stages them (pair_common.h)
    size_t qrow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = min(i0 + pair_stage_row(h), N - 1);               // (a row past the last query re-reads a real one)
        const int b = i / n, c = i - b * n;
        qrow[h] = ((size_t)b * 2 * n + c) * D;
    }
    // (a row past the range re-reads the range's first one; never selected)
    auto key_row = [&](int w) { return (size_t)(row0 + w < row1 ? row0 + w : row0) * D; };

    f32x16 acc;
    auto zero = [&]() {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    };
    auto slice = [&](bf16x8 qhi, bf16x8 qlo, bf16x8 khi, bf16x8 klo) {
        acc = mfma32f<FMT_FP16>(klo, qhi, acc);
        acc = mfma32f<FMT_FP16>(khi, qlo, acc);
        acc = mfma32f<FMT_FP16>(khi, qhi, acc);
    };
    // the block's scores: register r of this lane is key acc_row(r, lh) of the wave's half, query lr
    auto select = [&](int kb) {
        if (!qvalid) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int g = row0 + kb * 64 + kh * 32 + acc_row(r, lh);
            if (g >= row1) continue;
            const float s = acc[r] * PAIR_UNSCALE + 0.f;                // (+ 0: a negative zero becomes the positive one)
            if (!better(s, g, thr_s, thr_g)) continue;
            int pos = k - 1;                                            // the last entry leaves
            while (pos > 0) {
                const float ps = my_ls[(pos - 1) * 256];
                const int pg = my_lg[(pos - 1) * 256];
                if (!better(s, g, ps, pg)) break;
                my_ls[pos * 256] = ps;
                my_lg[pos * 256] = pg;
                --pos;
            }
            my_ls[pos * 256] = s;
            my_lg[pos * 256] = g;
            thr_s = my_ls[(k - 1) * 256];
            thr_g = my_lg[(k - 1) * 256];
        }
    };
    pair_walk(knn_lds, qp, (size_t)n * D, qrow, bank, bank_lo, (row1 - row0 + 63) >> 6, D >> 6, key_row, [](int) {}, zero, slice, select);
    __syncthreads();
    // 4-way merge of the query's lists (waves (qh, 0) and (qh, 1), both lane halves) under the total order
    if (tid < 64 && i0 + tid < N) {
        const int q = tid;
        const int t0 = ((q >> 5) * 2) * 64 + (q & 31), t1 = t0 + 32, t2 = t0 + 64, t3 = t0 + 96;
        int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
        const size_t out = ((size_t)si * N + (size_t)(i0 + q)) * k;
        for (int i = 0; i < k; ++i) {
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
            cand_s[out + i] = bs;
            cand_g[out + i] = bg == KNN_EMPTY ? -1 : bg;
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_g,
                                                        const void* __restrict__ bank_labels, int N, int S, int k, int C, float a,
                                                        float* __restrict__ seg_out, int32_t* __restrict__ topk_idx,
                                                        float* __restrict__ topk_w) {
    __shared__ float sel_w[4][DINOSEG_KNN_MAX_K];
    __shared__ int sel_g[4][DINOSEG_KNN_MAX_K];
    __shared__ int sel_l[4][DINOSEG_KNN_MAX_K];                         // (hard labels) the selected rows' labels
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    const bool valid = q < N;
    int kept = 0;
    float W = 0.f;
    if (valid) {
        unsigned long long key[4];
        const int ncand = S * k;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            key[j] = 0;
            if (e < ncand) {
                const int si = e / k, i = e - si * k;
                const size_t at = ((size_t)si * N + q) * k + i;
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
            if (m == 0) break;                                          // K' = i candidates in all (wave-uniform)
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = key[j] == m ? 0 : key[j];   // (g is unique: exactly one slot of one lane)
            const float s = prp_key_score(m);
            if (i == 0) s0 = s;
            const float w = __builtin_amdgcn_exp2f((s - s0) * a);
            W += w;
            if (lane == 0) {
                const int g = (int)(0xFFFFFFFFu - (uint32_t)m);
                sel_w[wave][i] = w;
                sel_g[wave][i] = g;
                if (KIND == 1) sel_l[wave][i] = (int)reinterpret_cast<const uint8_t*>(bank_labels)[g];
            }
            kept = i + 1;
        }
    }
    __syncthreads();
    if (!valid) return;
    const float inv = __fdiv_rn(1.f, W);
    for (int c = lane; c < C; c += 64) {
        float v = 0.f;
        for (int i = 0; i < kept; ++i) {
            if (KIND == 0)
                v = __builtin_fmaf(sel_w[wave][i], reinterpret_cast<const float*>(bank_labels)[(size_t)sel_g[wave][i] * C + c], v);
            else
                v += sel_l[wave][i] == c ? sel_w[wave][i] : 0.f;        // (a void label, >= C, meets no class)
        }
        seg_out[(size_t)q * C + c] = v * inv;
    }
    if (lane < k) {
        if (topk_idx) topk_idx[(size_t)q * k + lane] = lane < kept ? sel_g[wave][lane] : -1;
        if (topk_w) topk_w[(size_t)q * k + lane] = lane < kept ? sel_w[wave][lane] * inv : 0.f;
    }
}

bool knn_sizes_ok(long long N, long long M, int k) {
    return N >= 1 && N <= KNN_MAX_QUERIES && M >= 1 && M <= KNN_MAX_ROWS && k >= 1 && k <= DINOSEG_KNN_MAX_K;
}

}  // namespace

int knn_splits(int N, int M, int k) {
    if (!knn_sizes_ok(N, M, k)) return -1;
    // two workgroups per compute unit (256 of them) when the query tiles alone do not give that many, a range of at least 4 key blocks
    const long long tiles = ((long long)N + 63) / 64, nblk = ((long long)M + 63) / 64;
    long long S = (512 + tiles - 1) / tiles;
    if (nblk / 4 < S) S = nblk / 4;
    if (S < 1) S = 1;
    const int cap = knn_split_cap(M, k);
    return S > cap ? cap : (int)S;
}

long long knn_scratch_bytes(int N, int M, int k, int splits) {
    if (!knn_sizes_ok(N, M, k) || splits < 0 || splits > knn_split_cap(M, k)) return -1;
    const int S = splits ? splits : knn_splits(N, M, k);
    return (long long)S * N * k * 8;                                    // fp32 scores, then int32 indices, [S][N][k] each
}

int launch_knn_labels(const void* query_planes, int B, int n, const void* bank_planes, long long M, long long bank_rows,
                      const void* bank_labels, int label_kind, int D, int C, int k, double tau, int splits, float* seg_out,
                      int32_t* topk_idx, float* topk_w, void* scratch, hipStream_t s) {
    const char* who = "dinoseg_op_knn_labels";
    if (!query_planes || !bank_planes || !bank_labels || !seg_out || !scratch) {
        dinoseg_set_error("%s: null pointer (query planes, bank planes, bank labels, seg_out and scratch are required)", who);
        return -1;
    }
    if (B < 1 || n < 1 || n > (1 << 24)) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive, n <= 2^24)", who, B, n);
        return -1;
    }
    const long long N = (long long)B * n;
    if (N > KNN_MAX_QUERIES) {
        dinoseg_set_error("%s: B n = %lld queries exceed the launch range", who, N);
        return -1;
    }
    if (M < 1 || M > bank_rows || bank_rows > KNN_MAX_ROWS) {
        dinoseg_set_error("%s: M = %lld live rows of bank_rows = %lld (1 <= M <= bank_rows <= 2^24)", who, M, bank_rows);
        return -1;
    }
    if (label_kind != 0 && label_kind != 1) {
        dinoseg_set_error("%s: label kind %d (0 = soft fp32 [bank_rows, C], 1 = hard uint8 [bank_rows])", who, label_kind);
        return -1;
    }
    if (D < 64 || D % 64 != 0 || D > 8192) {
        dinoseg_set_error("%s: width D = %d (a multiple of 64 up to 8192)", who, D);
        return -1;
    }
    if (C < 1 || C > 256) {
        dinoseg_set_error("%s: C = %d classes (1 <= C <= 256)", who, C);
        return -1;
    }
    if (k < 1 || k > DINOSEG_KNN_MAX_K) {
        dinoseg_set_error("%s: k = %d (1 <= k <= %d)", who, k, DINOSEG_KNN_MAX_K);
        return -1;
    }
    const int cap = knn_split_cap(M, k);
    if (splits < 0 || splits > cap) {
        dinoseg_set_error("%s: splits = %d (0 = the library's choice, or 1 .. min(16, 256 / k, ceil(M / 64)) = %d)", who, splits, cap);
        return -1;
    }
    if (!(std::isfinite(tau) && tau > 0.0)) {
        dinoseg_set_error("%s: temperature %g (finite and positive)", who, tau);
        return -1;
    }
    const float a = (float)(1.4426950408889634074 / tau);
    if (!std::isfinite(a)) {
        dinoseg_set_error("%s: temperature %g is too small (log2(e) / tau exceeds fp32)", who, tau);
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(query_planes) & 15) != 0 || (reinterpret_cast<uintptr_t>(bank_planes) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(scratch) & 3) != 0 || (label_kind == 0 && (reinterpret_cast<uintptr_t>(bank_labels) & 3) != 0)) {
        dinoseg_set_error("%s: query and bank planes must be 16-byte aligned, scratch and soft labels 4-byte aligned", who);
        return -1;
    }
    const int S = splits ? splits : knn_splits((int)N, (int)M, k);
    float* cand_s = reinterpret_cast<float*>(scratch);
    int* cand_g = reinterpret_cast<int*>(cand_s + (size_t)S * N * k);
    const size_t lds = PAIR_STAGE + (size_t)k * 2048;
    hipLaunchKernelGGL(knn_scores_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)S), dim3(256), lds, s,
                       reinterpret_cast<const uint16_t*>(query_planes), (int)N, n, reinterpret_cast<const uint16_t*>(bank_planes), (int)M,
                       (size_t)bank_rows * D, D, k, cand_s, cand_g);
    DSEG_CHECK_HIP(hipGetLastError());
    if (label_kind == 0)
        hipLaunchKernelGGL(knn_merge_kernel<0>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, cand_s, cand_g, bank_labels, (int)N, S, k, C,
                           a, seg_out, topk_idx, topk_w);
    else
        hipLaunchKernelGGL(knn_merge_kernel<1>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, cand_s, cand_g, bank_labels, (int)N, S, k, C,
                           a, seg_out, topk_idx, topk_w);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
