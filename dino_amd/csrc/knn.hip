// Few-shot segmentation: k-NN label retrieval from a flat memory bank of labelled patch features, without the [N, M] score matrix.
// The rule is stated in full in include/dinoseg.h (dinoseg_op_knn_labels); in short, every query cell takes the k best-scoring live
// rows of the bank -- score and order are dinoseg_op_propagate's, without a neighbourhood test -- and averages their labels with
// weights exp((s - s_0) / tau).
//
//   knn_scores_kernel   one workgroup (4 waves) per (64 consecutive queries, one of S contiguous bank ranges).  A range is whole key
//                       blocks of 64 rows (knn_range), the last one clipped at M, walked by the family's pair walk (pair_common.h);
//                       every live row of the block is a candidate for the selection of select_common.h (the slice body, the
//                       per-lane lists of k (score, g) in LDS, the 4-way merge into the scratch: [S][N][k] scores, then indices).
//                       A query is row i / n, cell i % n of the [B][2][n][D] planes, so a tile may span frames; the bank is one
//                       "frame" of bank_rows rows.  LDS: 32 KiB + 2 KiB k <= 64 KiB; no atomics; every loop bound is a function
//                       of the shapes.
//   knn_merge_kernel    one wave per query: the wave select of select_common.h over the S k <= 256 candidates; lanes stride the C
//                       classes with k gathers and fmaf each (soft rows), or k compares against the selected rows' labels (hard
//                       labels, read once per query by lane 0).
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "select_common.h"

namespace dseg {

namespace {

constexpr int KNN_MAX_SPLITS = 16;
constexpr long long KNN_MAX_ROWS = 1ll << 24;   // bank rows: g and 64 key blocks stay far inside int
constexpr long long KNN_MAX_QUERIES = (1ll << 31) - 256;
static_assert(DINOSEG_KNN_MAX_K <= SEL_MAX_K, "the selection's k");

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
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int qh = wave >> 1, kh = wave & 1;
    const int i0 = (int)blockIdx.x * PAIR_TILE;                         // (N <= 2^31 - 256: i0 + 63 fits)
    const int nblk = (M + 63) >> 6, S = (int)gridDim.y, si = (int)blockIdx.y;
    const int b0 = knn_range(nblk, S, si), b1 = knn_range(nblk, S, si + 1);
    const int row0 = b0 * 64, row1 = min(b1 * 64, M);                   // the range's rows: row0 .. row1 - 1, at least one

    SelLists lists = sel_lists(knn_lds, k);

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
    auto zero = [&]() { sel_zero(acc); };
    auto slice = [&](bf16x8 qhi, bf16x8 qlo, bf16x8 khi, bf16x8 klo) { sel_slice(acc, qhi, qlo, khi, klo); };
    // the block's scores: register r of this lane is key acc_row(r, lh) of the wave's half, query lr
    auto select = [&](int kb) {
        if (!qvalid) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int g = row0 + kb * 64 + kh * 32 + acc_row(r, lh);
            if (g >= row1) continue;
            sel_insert(lists, sel_score(acc[r]), g);
        }
    };
    pair_walk(knn_lds, qp, (size_t)n * D, qrow, bank, bank_lo, (row1 - row0 + 63) >> 6, D >> 6, key_row, [](int) {}, zero, slice, select);
    __syncthreads();
    // thread q merges the lists of the tile's query q into the range's slots of the scratch
    if (tid < 64 && i0 + tid < N) {
        const size_t out = ((size_t)si * N + (size_t)(i0 + tid)) * k;
        sel_merge4(lists, tid, cand_s + out, cand_g + out);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_g,
                                                        const void* __restrict__ bank_labels, int N, int S, int k, int C, float a,
                                                        float* __restrict__ seg_out, int32_t* __restrict__ topk_idx,
                                                        float* __restrict__ topk_w) {
    __shared__ SelPicks picks;
    __shared__ int sel_l[4][DINOSEG_KNN_MAX_K];                         // (hard labels) the selected rows' labels
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    const SelSum sum = sel_wave_select(cand_s, cand_g, S, N, q, k, a, picks, [&](int i, int g) {
        if (KIND == 1) sel_l[wave][i] = (int)reinterpret_cast<const uint8_t*>(bank_labels)[g];
    });
    __syncthreads();
    if (q >= N) return;
    const float inv = sel_inv(sum.W);
    for (int c = lane; c < C; c += 64) {
        float v = 0.f;
        for (int i = 0; i < sum.kept; ++i) {
            if (KIND == 0)
                v = __builtin_fmaf(picks.w[wave][i], reinterpret_cast<const float*>(bank_labels)[(size_t)picks.g[wave][i] * C + c], v);
            else
                v += sel_l[wave][i] == c ? picks.w[wave][i] : 0.f;        // (a void label, >= C, meets no class)
        }
        seg_out[(size_t)q * C + c] = v * inv;
    }
    sel_write_topk(picks, sum.kept, inv, q, k, topk_idx, topk_w);
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
    return sel_scratch_bytes(S, N, k);
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
    if (sel_shape_check(who, D, C, k, DINOSEG_KNN_MAX_K)) return -1;
    const int cap = knn_split_cap(M, k);
    if (splits < 0 || splits > cap) {
        dinoseg_set_error("%s: splits = %d (0 = the library's choice, or 1 .. min(16, 256 / k, ceil(M / 64)) = %d)", who, splits, cap);
        return -1;
    }
    float a;
    if (sel_temperature(who, tau, &a)) return -1;
    if ((reinterpret_cast<uintptr_t>(query_planes) & 15) != 0 || (reinterpret_cast<uintptr_t>(bank_planes) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(scratch) & 3) != 0 || (label_kind == 0 && (reinterpret_cast<uintptr_t>(bank_labels) & 3) != 0)) {
        dinoseg_set_error("%s: query and bank planes must be 16-byte aligned, scratch and soft labels 4-byte aligned", who);
        return -1;
    }
    const int S = splits ? splits : knn_splits((int)N, (int)M, k);
    const SelScratch c = sel_scratch(scratch, S, N, k);
    hipLaunchKernelGGL(knn_scores_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)S), dim3(256), sel_lds_bytes(k), s,
                       reinterpret_cast<const uint16_t*>(query_planes), (int)N, n, reinterpret_cast<const uint16_t*>(bank_planes), (int)M,
                       (size_t)bank_rows * D, D, k, c.cand_s, c.cand_g);
    DSEG_CHECK_HIP(hipGetLastError());
    if (label_kind == 0)
        hipLaunchKernelGGL(knn_merge_kernel<0>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, c.cand_s, c.cand_g, bank_labels, (int)N, S, k, C,
                           a, seg_out, topk_idx, topk_w);
    else
        hipLaunchKernelGGL(knn_merge_kernel<1>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, c.cand_s, c.cand_g, bank_labels, (int)N, S, k, C,
                           a, seg_out, topk_idx, topk_w);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
