// Wide classifier tail: the last Linear of the segmentation head (K -> C, 33 <= C <= 256), log_softmax(dim=1) and the first-max
// argmax in one launch (pl_torch_modules.py:108-138 with n_classes up to 256: ADE20K 150, COCO-Stuff 171 / 182).
//
// head_final_kernel (elementwise.hip) keeps a row's logits in a float z[32] array and stages the fp32 classifier in LDS: it stops at
// 32 classes.  Here the classifier is a pair of hi+lo planes packed at weight refresh, [Cpad][ld] with Cpad = round_up(C, 32) and
// zeros beyond K and C, and the product runs on MFMAs like gemm.hip: v_mfma_f32_32x32x16_{bf16,f16}, hi*hi + hi*lo + lo*hi with fp32
// accumulation.
//
// Layout: a 256-thread workgroup owns 128 rows across ALL Cpad columns; wave w owns rows 32w .. 32w+31 and holds NT = Cpad / 32
// accumulators (128 fp32 per lane at Cpad = 256).  Because a wave owns whole rows, the row reductions never leave the wave: the
// classes of a row are spread over the 32 lanes of one half-wave (acc_row: lane half h holds rows (r&3) + 8(r>>2) + 4h), so max,
// argmax and the sum of exponentials are a local pass over the NT tiles and five xor-shuffles.  Pad columns get a -inf bias.
// The classifier streams through LDS in 32-column k-slabs ([Cpad][32] bf16 per plane, 64-byte rows, the gemm_ln swizzle aln::off64),
// prefetched into registers while the previous slab is multiplied; each wave reads its A fragments straight from the row-major
// activation planes.  logp rows are written as 128-byte segments (32 lanes, 32 consecutive classes), argmax by one lane per row.
//
// Work at ViT-S/8 @480, batch 32, C = 150 (Cpad 160), MLP head (K = 100 in 128 columns): 115200 rows x 160 x 128 x 2 x 3 products
// = 14 GFLOP of MFMA issue, 59 MB of activations read, 69 MB of logp written -- HBM-bound at ~20 us; the classifier planes (82 KB) are
// re-read from L2 once per 128-row block.
#include "common.h"
#include "gemm_ln_common.h"
#include "kernels.h"

namespace dseg {

namespace hw {
constexpr int BM = 128;          // rows per workgroup (4 waves x 32)
constexpr int BK = 32;           // classifier k-slab
}  // namespace hw

template <int FMT, int NT>
__global__ __launch_bounds__(256) void head_wide_kernel(const bf16_t* __restrict__ in, long in_plane, int ld, int M, int K,
                                                        const bf16_t* __restrict__ Wp, long w_plane, const float* __restrict__ bias,
                                                        int C, float* __restrict__ logp, int32_t* __restrict__ amax) {
    constexpr int CP = NT * 32;                          // padded classes
    constexpr int SLAB = CP * 64;                        // bytes of one plane's [CP][32] slab
    constexpr int PER_T = CP * 4 * 2 / 256;              // 16-byte chunks per thread and slab (both planes) = NT
    __shared__ __attribute__((aligned(16))) char ws[2 * SLAB];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const long m0 = (long)blockIdx.x * hw::BM;
    const int nk = (K + hw::BK - 1) / hw::BK;

    // this lane's A row (clamped: rows >= M compute garbage that is never stored)
    long arow = m0 + wave * 32 + lr;
    arow = arow < M ? arow : M - 1;
    const bf16_t* ah = in + arow * ld + lh * 8;
    const bf16_t* al = ah + in_plane;

    uint4 wreg[PER_T];
    auto fetch_w = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER_T; ++u) {
            const int i = tid + 256 * u;
            const int pl = i / (CP * 4), rem = i - pl * (CP * 4);
            const int n = rem >> 2, q = rem & 3;
            wreg[u] = *reinterpret_cast<const uint4*>(Wp + pl * w_plane + (long)n * ld + kt * hw::BK + q * 8);
        }
    };
    auto store_w = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER_T; ++u) {
            const int i = tid + 256 * u;
            const int pl = i / (CP * 4), rem = i - pl * (CP * 4);
            const int n = rem >> 2, q = rem & 3;
            *reinterpret_cast<uint4*>(ws + pl * SLAB + aln::off64(n, q)) = wreg[u];
        }
    };
    uint4 areg[2][2];                                    // [kk][plane]
    auto fetch_a = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            areg[kk][0] = *reinterpret_cast<const uint4*>(ah + kt * hw::BK + kk * 16);
            areg[kk][1] = *reinterpret_cast<const uint4*>(al + kt * hw::BK + kk * 16);
        }
    };

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    fetch_w(0);
    fetch_a(0);
    store_w();
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        bf16x8 a[2][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            a[kk][0] = __builtin_bit_cast(bf16x8, areg[kk][0]);
            a[kk][1] = __builtin_bit_cast(bf16x8, areg[kk][1]);
        }
        if (kt + 1 < nk) {                               // next slab in flight while this one is multiplied
            fetch_w(kt + 1);
            fetch_a(kt + 1);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = j * 32 + lr;
                const bf16x8 bh = lds_frag(ws + aln::off64(n, kk * 2 + lh));
                const bf16x8 bl = lds_frag(ws + SLAB + aln::off64(n, kk * 2 + lh));
                acc[j] = mfma32f<FMT>(a[kk][1], bh, acc[j]);
                acc[j] = mfma32f<FMT>(a[kk][0], bl, acc[j]);
                acc[j] = mfma32f<FMT>(a[kk][0], bh, acc[j]);
            }
        if (kt + 1 < nk) {
            __syncthreads();                             // every wave is done reading slab kt
            store_w();
            __syncthreads();
        }
    }

    // ---- epilogue: bias (-inf on pad columns), row max / first argmax / log-sum-exp over the 32 lanes of the half-wave
    float bj[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = j * 32 + lr;
        bj[j] = c < C ? bias[c] : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long m = m0 + wave * 32 + acc_row(r, lh);
        float z[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) z[j] = acc[j][r] + bj[j];
        float mx = z[0];
        int am = lr;
#pragma unroll
        for (int j = 1; j < NT; ++j)
            if (z[j] > mx) {
                mx = z[j];
                am = j * 32 + lr;
            }
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const float om = __shfl_xor(mx, o);
            const int oa = __shfl_xor(am, o);
            if (om > mx || (om == mx && oa < am)) {
                mx = om;
                am = oa;
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) sum += expf(z[j] - mx);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) sum += __shfl_xor(sum, o);
        const float lse = logf(sum);
        if (m < M) {
            float* row = logp + m * C;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int c = j * 32 + lr;
                if (c < C) row[c] = (z[j] - mx) - lse;
            }
            if (amax && lr == 0) amax[m] = am;
        }
    }
}

template <int FMT>
static int launch_wide_fmt(const bf16_t* in, long in_plane, int ld, int M, int K, const bf16_t* Wp, long w_plane, const float* b, int C,
                           float* logp, int32_t* argmax, hipStream_t s) {
    const dim3 grid((unsigned)((M + hw::BM - 1) / hw::BM));
    switch ((C + 31) / 32) {
#define DSEG_WIDE_CASE(nt) \
    case nt: hipLaunchKernelGGL((head_wide_kernel<FMT, nt>), grid, dim3(256), 0, s, in, in_plane, ld, M, K, Wp, w_plane, b, C, logp, argmax); break;
        DSEG_WIDE_CASE(1) DSEG_WIDE_CASE(2) DSEG_WIDE_CASE(3) DSEG_WIDE_CASE(4)
        DSEG_WIDE_CASE(5) DSEG_WIDE_CASE(6) DSEG_WIDE_CASE(7) DSEG_WIDE_CASE(8)
#undef DSEG_WIDE_CASE
    }
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_head_wide(const bf16_t* in, long in_plane, int ld, int M, int K, const bf16_t* Wp, long w_plane, const float* b, int C,
                     float* logp, int32_t* argmax, hipStream_t s, int fmt) {
    if (M <= 0) return 0;
    if (C < 1 || C > HEAD_WIDE_MAX_C || K < 1 || K > ld || ld % hw::BK != 0 || !Wp || w_plane < (long)((C + 31) / 32 * 32) * ld || !b ||
        !logp) {
        dinoseg_set_error("head_wide: need 1 <= C <= %d, K <= ld, ld %% 32 == 0 and packed [round_up(C, 32)][ld] classifier planes "
                          "(C=%d K=%d ld=%d)", HEAD_WIDE_MAX_C, C, K, ld);
        return -1;
    }
    if (fmt == FMT_FP16) return launch_wide_fmt<FMT_FP16>(in, in_plane, ld, M, K, Wp, w_plane, b, C, logp, argmax, s);
    return launch_wide_fmt<FMT_BF16>(in, in_plane, ld, M, K, Wp, w_plane, b, C, logp, argmax, s);
}

}  // namespace dseg
