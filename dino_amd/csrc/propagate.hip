// Video label propagation from patch features (the semi-supervised video segmentation protocol of the DINO paper) without the
// [n_ctx, n, n] affinity.  The rule is stated in full in include/dinoseg.h (dinoseg_op_propagate); in short, every cell of the target
// frame takes the k best-scoring cells within R cells of itself over all context frames -- score = the inner product of the unit
// feature rows, order = (score descending, global index ascending) -- and averages their label rows with weights exp((s - s_0) / tau).
//
//   normalize_tokens_kernel   one wave per patch token: ||f||^2 and the quotient in fp64, the row scaled by 2^10 and split into fp16
//                             hi + lo planes [2][n][D] (a unit row's components are about D^-1/2: unscaled, the lo plane would sit in
//                             fp16 subnormals; scaled, hi + lo carries 22 significand bits down to |f^| = 2^-13).  The CLS row is skipped.
//   label_cells_kernel        one wave per cell: lane l counts classes l, l + 64, ... over the cell's pixels (every lane reads the same
//                             pixel: a broadcast), integer counts, no atomics; seg_0 = count / pixels of the cell.
//   propagate_scores_kernel   one workgroup (4 waves) per (8 x 8 query tile, context frame).  The tile's key window is the tile widened
//                             by R cells and clipped to the grid (32 x 32 keys at R = 12), walked in blocks of 64 keys by the family's
//                             pair walk (pair_common.h); wave (qh, kh) multiplies keys 32 kh .. by queries 32 qh .. .  Every (key,
//                             query) element of an MFMA goes through the same arithmetic, so a score depends on the two rows alone.
//                             A lane owns one query and 16 keys of the block: the neighbourhood test in integers, then the key is a
//                             candidate for the selection of select_common.h (the slice body, the per-lane lists of k (score, g) in
//                             LDS, the 4-way merge into the scratch: [n_ctx][n][k] scores, then indices).  LDS: 32 KiB + 2 KiB k <=
//                             64 KiB; no atomics; every loop bound is a function of the shapes.
//   propagate_merge_kernel    one wave per query: the wave select of select_common.h over the n_ctx k <= 256 candidates; lanes
//                             stride the C classes with k gathers and fmaf each.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "select_common.h"

namespace dseg {

namespace {

constexpr int PRP_TILE = 8;                     // query tile side, 64 queries
constexpr int PRP_MAX_SIDE = 4096;              // grid side: n <= 2^24, 16 n < 2^31
static_assert(DINOSEG_PROPAGATE_MAX_K <= SEL_MAX_K, "the selection's k");

__global__ __launch_bounds__(256) void normalize_tokens_kernel(const float* __restrict__ tokens, long long rows, int n, int D,
                                                               uint16_t* __restrict__ planes) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                            // (a whole wave: no barrier follows)
    const long long b = row / n, j = row - b * n;
    const float* src = tokens + ((size_t)b * (n + 1) + 1 + j) * D;
    double ss = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)src[d];
        ss = fma(v, v, ss);
    }
    ss = wave_sum_f64(ss);
    const double inv = 1024.0 / fmax(sqrt(ss), 1e-12);
    uint16_t* hi = planes + ((size_t)b * 2 * n + j) * D;
    uint16_t* lo = hi + (size_t)n * D;
    for (int d = lane; d < D; d += 64) {
        const UnitSplit v = split_unit((double)src[d] * inv);
        hi[d] = v.hi;
        lo[d] = v.lo;
    }
}

__global__ __launch_bounds__(256) void label_cells_kernel(const void* __restrict__ labels, int mask_kind, int OH, int OW, int hp, int wp,
                                                          int C, float* __restrict__ seg) {
    const int lane = threadIdx.x & 63;
    const int cell = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= hp * wp) return;                                        // (a whole wave: no barrier follows)
    const int r = cell / wp, c = cell - r * wp;
    // the pixels y with (y hp) / OH == r: ceil(r OH / hp) .. ceil((r + 1) OH / hp) - 1 (never empty: OH >= hp)
    const int y0 = (int)(((long long)r * OH + hp - 1) / hp), y1 = (int)(((long long)(r + 1) * OH + hp - 1) / hp);
    const int x0 = (int)(((long long)c * OW + wp - 1) / wp), x1 = (int)(((long long)(c + 1) * OW + wp - 1) / wp);
    int cnt[4] = {0, 0, 0, 0};                                          // classes lane, lane + 64, lane + 128, lane + 192
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const size_t at = (size_t)y * OW + x;
            const long long v = mask_kind == 0 ? (long long)reinterpret_cast<const uint8_t*>(labels)[at]
                                               : reinterpret_cast<const int64_t*>(labels)[at];
#pragma unroll
            for (int i = 0; i < 4; ++i) cnt[i] += v == (long long)(lane + 64 * i) ? 1 : 0;
        }
    const float npix = (float)((long long)(y1 - y0) * (x1 - x0));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cls = lane + 64 * i;
        if (cls < C) seg[(size_t)cell * C + cls] = __fdiv_rn((float)cnt[i], npix);
    }
}

struct PrpCtx {
    const uint16_t* planes[DINOSEG_PROPAGATE_MAX_CONTEXT];
    const float* segs[DINOSEG_PROPAGATE_MAX_CONTEXT];
};

__global__ __launch_bounds__(256) void propagate_scores_kernel(const uint16_t* __restrict__ tq, PrpCtx ctx, int hp, int wp, int D, int R,
                                                               int k, int tiles_x, float* __restrict__ cand_s, int* __restrict__ cand_g) {
    extern __shared__ __attribute__((aligned(16))) char prp_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int qh = wave >> 1, kh = wave & 1;
    const int n = hp * wp, ci = blockIdx.y;
    const int r0 = ((int)blockIdx.x / tiles_x) * PRP_TILE, c0 = ((int)blockIdx.x % tiles_x) * PRP_TILE;
    // the key window: the tile widened by R, clipped to the grid
    const int wr0 = max(r0 - R, 0), wr1 = min(min(r0 + PRP_TILE - 1, hp - 1) + R, hp - 1);
    const int wc0 = max(c0 - R, 0), wc1 = min(min(c0 + PRP_TILE - 1, wp - 1) + R, wp - 1);
    const int ww = wc1 - wc0 + 1, nkeys = ww * (wr1 - wr0 + 1);
    const int nkb = (nkeys + 63) >> 6;
    const uint16_t* kp = ctx.planes[ci];

    SelLists lists = sel_lists(prp_lds, k);

    // the lane's query in the selection
    const int qi = qh * 32 + lr, qr = r0 + (qi >> 3), qc = c0 + (qi & 7);
    const bool qvalid = qr < hp && qc < wp;

    // the tile's query rows as the walk stages them (pair_common.h)
    size_t qrow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = pair_stage_row(h);
        const int r = min(r0 + (row >> 3), hp - 1), c = min(c0 + (row & 7), wp - 1);   // (a row past the grid re-reads a real one)
        qrow[h] = (size_t)(r * wp + c) * D;
    }
    auto key_row = [&](int w) {
        if (w >= nkeys) w = 0;                                          // (a key past the window re-reads a real one; never selected)
        const int wr = w / ww;
        return (size_t)((wr0 + wr) * wp + wc0 + (w - wr * ww)) * D;
    };

    f32x16 acc;
    auto zero = [&]() { sel_zero(acc); };
    auto slice = [&](bf16x8 qhi, bf16x8 qlo, bf16x8 khi, bf16x8 klo) { sel_slice(acc, qhi, qlo, khi, klo); };
    // the block's scores: register r of this lane is key acc_row(r, lh) of the wave's half, query lr
    auto select = [&](int kb) {
        if (!qvalid) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int w = kb * 64 + kh * 32 + acc_row(r, lh);
            if (w >= nkeys) continue;
            const int wr = w / ww, kr = wr0 + wr, kc = wc0 + (w - wr * ww);
            if (abs(kr - qr) > R || abs(kc - qc) > R) continue;
            sel_insert(lists, sel_score(acc[r]), ci * n + kr * wp + kc);
        }
    };
    pair_walk(prp_lds, tq, (size_t)n * D, qrow, kp, (size_t)n * D, nkb, D >> 6, key_row, [](int) {}, zero, slice, select);
    __syncthreads();
    // thread q merges the lists of the tile's query q into the frame's slots of the scratch
    if (tid < 64) {
        const int r = r0 + (tid >> 3), c = c0 + (tid & 7);
        if (r < hp && c < wp) {
            const size_t out = ((size_t)ci * n + (size_t)r * wp + c) * k;
            sel_merge4(lists, tid, cand_s + out, cand_g + out);
        }
    }
}

__global__ __launch_bounds__(256) void propagate_merge_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_g, PrpCtx ctx,
                                                              int n, int n_ctx, int k, int C, float a, float* __restrict__ seg_out,
                                                              int32_t* __restrict__ topk_idx, float* __restrict__ topk_w) {
    __shared__ SelPicks picks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    const SelSum sum = sel_wave_select(cand_s, cand_g, n_ctx, n, q, k, a, picks, [](int, int) {});
    __syncthreads();
    if (q >= n) return;
    const float inv = sel_inv(sum.W);
    for (int c = lane; c < C; c += 64) {
        float v = 0.f;
        for (int i = 0; i < sum.kept; ++i) {
            const int g = picks.g[wave][i], ci = g / n, j = g - ci * n;
            v = __builtin_fmaf(picks.w[wave][i], ctx.segs[ci][(size_t)j * C + c], v);
        }
        seg_out[(size_t)q * C + c] = v * inv;
    }
    sel_write_topk(picks, sum.kept, inv, q, k, topk_idx, topk_w);
}

int prp_grid_check(const char* who, int hp, int wp) {
    if (hp < 1 || wp < 1 || hp > PRP_MAX_SIDE || wp > PRP_MAX_SIDE) {
        dinoseg_set_error("%s: patch grid %d x %d (each side 1 .. %d)", who, hp, wp, PRP_MAX_SIDE);
        return -1;
    }
    return 0;
}

}  // namespace

int launch_normalize_tokens(const float* tokens, int B, int n, int D, void* planes, hipStream_t s) {
    const char* who = "dinoseg_op_normalize_tokens";
    if (!tokens || !planes) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (B < 1 || n < 1 || n > PRP_MAX_SIDE * PRP_MAX_SIDE || D < 64 || D % 64 != 0 || D > 8192) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells, width D = %d (positive; D a multiple of 64 up to 8192)", who, B, n, D);
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(planes) & 15) != 0) {
        dinoseg_set_error("%s: planes must be 16-byte aligned", who);
        return -1;
    }
    const long long rows = (long long)B * n;
    if (rows > (1ll << 31) - 4) {
        dinoseg_set_error("%s: B n = %lld rows exceed the launch range", who, rows);
        return -1;
    }
    hipLaunchKernelGGL(normalize_tokens_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, tokens, rows, n, D,
                       reinterpret_cast<uint16_t*>(planes));
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_label_cells(const void* labels, int mask_kind, int OH, int OW, int hp, int wp, int C, float* seg, hipStream_t s) {
    const char* who = "dinoseg_op_label_cells";
    if (!labels || !seg) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (mask_kind != 0 && mask_kind != 1) {
        dinoseg_set_error("%s: mask kind %d (0 = uint8, 1 = int64)", who, mask_kind);
        return -1;
    }
    if (C < 1 || C > 256) {
        dinoseg_set_error("%s: C = %d classes (1 <= C <= 256)", who, C);
        return -1;
    }
    if (prp_grid_check(who, hp, wp)) return -1;
    if (OH < hp || OW < wp || OH > (1 << 20) || OW > (1 << 20)) {
        dinoseg_set_error("%s: labels of %d x %d for a grid of %d x %d (OH >= hp, OW >= wp, each side <= 2^20)", who, OH, OW, hp, wp);
        return -1;
    }
    hipLaunchKernelGGL(label_cells_kernel, dim3((unsigned)((hp * wp + 3) / 4)), dim3(256), 0, s, labels, mask_kind, OH, OW, hp, wp, C, seg);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

long long propagate_scratch_bytes(int hp, int wp, int n_ctx, int k) {
    if (hp < 1 || wp < 1 || hp > PRP_MAX_SIDE || wp > PRP_MAX_SIDE || n_ctx < 1 || n_ctx > DINOSEG_PROPAGATE_MAX_CONTEXT || k < 1 ||
        k > DINOSEG_PROPAGATE_MAX_K)
        return -1;
    return sel_scratch_bytes(n_ctx, (long long)hp * wp, k);
}

int launch_propagate(const void* target_planes, const void* const* ctx_planes, const float* const* ctx_segs, int n_ctx, int hp, int wp,
                     int D, int C, int radius, int k, double tau, float* seg_out, int32_t* topk_idx, float* topk_w, void* scratch,
                     hipStream_t s) {
    const char* who = "dinoseg_op_propagate";
    if (n_ctx < 1 || n_ctx > DINOSEG_PROPAGATE_MAX_CONTEXT) {
        dinoseg_set_error("%s: %d context frames (1 <= n_ctx <= %d)", who, n_ctx, DINOSEG_PROPAGATE_MAX_CONTEXT);
        return -1;
    }
    if (!target_planes || !ctx_planes || !ctx_segs || !seg_out || !scratch) {
        dinoseg_set_error("%s: null pointer (target planes, the two context tables, seg_out and scratch are required)", who);
        return -1;
    }
    PrpCtx ctx = {};
    for (int i = 0; i < n_ctx; ++i) {
        if (!ctx_planes[i] || !ctx_segs[i]) {
            dinoseg_set_error("%s: null planes or seg of context frame %d", who, i);
            return -1;
        }
        if ((reinterpret_cast<uintptr_t>(ctx_planes[i]) & 15) != 0) {
            dinoseg_set_error("%s: the planes of context frame %d are not 16-byte aligned", who, i);
            return -1;
        }
        ctx.planes[i] = reinterpret_cast<const uint16_t*>(ctx_planes[i]);
        ctx.segs[i] = ctx_segs[i];
    }
    if ((reinterpret_cast<uintptr_t>(target_planes) & 15) != 0 || (reinterpret_cast<uintptr_t>(scratch) & 3) != 0) {
        dinoseg_set_error("%s: target planes must be 16-byte aligned, scratch 4-byte aligned", who);
        return -1;
    }
    if (prp_grid_check(who, hp, wp)) return -1;
    if (sel_shape_check(who, D, C, k, DINOSEG_PROPAGATE_MAX_K)) return -1;
    if (radius < 0) {
        dinoseg_set_error("%s: radius %d (>= 0)", who, radius);
        return -1;
    }
    float a;
    if (sel_temperature(who, tau, &a)) return -1;
    const int n = hp * wp;
    const int R = radius > PRP_MAX_SIDE ? PRP_MAX_SIDE : radius;         // (beyond the grid's side the window is the whole grid)
    const int tiles_x = (wp + PRP_TILE - 1) / PRP_TILE, tiles_y = (hp + PRP_TILE - 1) / PRP_TILE;
    const SelScratch c = sel_scratch(scratch, n_ctx, n, k);
    hipLaunchKernelGGL(propagate_scores_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_ctx), dim3(256), sel_lds_bytes(k), s,
                       reinterpret_cast<const uint16_t*>(target_planes), ctx, hp, wp, D, R, k, tiles_x, c.cand_s, c.cand_g);
    DSEG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(propagate_merge_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, c.cand_s, c.cand_g, ctx, n, n_ctx, k, C, a,
                       seg_out, topk_idx, topk_w);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
