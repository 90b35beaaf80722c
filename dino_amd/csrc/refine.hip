// Image-guided iterative label refinement at pixel resolution: PAMR (pixel-adaptive mask refinement, Araslanov & Roth, CVPR 2020).
// A per-pixel state P [B, C, OH, OW] is averaged `iters` times over 8 M dilated taps with weights that fall off with the guide's
// colour difference measured in local standard deviations, so that mass stops at the image's edges.  The rule is stated in full in
// include/dinoseg.h (dinoseg_op_refine_iterate); nothing here is atomic and no workgroup waits for another.
//
//   refine_seed_labels_kernel   a lane per pixel: the one-hot planes of an int32 label map (a label outside [0, C): all zero).
//   refine_seed_scores_kernel   the bilinear family's geometry and strip walk (upsample_common.h: the values are upsample_argmax's
//                               dense values bit for bit), then softmax_k(gain v_k) per pixel in three walks over the lane's own
//                               stores: gain v and its maximum, up_exp and the sum in class order, times the one reciprocal.
//   refine_pass_kernel<M>       one workgroup per 64 x 32 output tile, wave w rows 8w .. 8w+7, lane l column l.  The guide of the tile
//                               plus a halo of the largest dilation, clamped to the frame, is staged in LDS as packed RGB words, the
//                               state CC class planes at a time beside it (plane-major: the lanes of a wave read consecutive words).
//                               A lane takes its 8 pixels one at a time: the 8 M weights and LDS offsets of the pixel are formed in
//                               registers (M is a template parameter: the arrays unroll), then the staged classes are walked with one
//                               LDS read and one fmaf per tap and class.  With C > CC the weights are formed again per class pass.
//                               The last pass keeps the running first maximum of the 8 pixels in registers and writes the labels.
//   refine_label_kernel         iters = 0: the labels (and the copy) of the seed.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

#include <cmath>
#include <type_traits>

namespace dseg {

namespace {

constexpr int RF_CLASSES = 3;               // classes a lane accumulates side by side (independent fmaf chains, each in tap order)

struct RefineDil {
    int d[REFINE_MAX_DIL];
};

__global__ __launch_bounds__(256) void refine_seed_labels_kernel(const int32_t* __restrict__ labels, int C, size_t plane, size_t npix,
                                                                 float* __restrict__ state) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const size_t b = i / plane, p = i - b * plane;
    const int l = labels[i];
    float* dst = state + b * (size_t)C * plane + p;
    for (int k = 0; k < C; ++k) dst[(size_t)k * plane] = l == k ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void refine_seed_scores_kernel(const float* __restrict__ logp, int hp, int wp, int C, int OH, int OW,
                                                                 int tiles_x, int tiles_y, int CC, int stride, int kw_log2, float gain,
                                                                 float* state) {
    extern __shared__ float rfs_lds[];
    const UpTile T = up_tile(tiles_x, tiles_y, OH, OW);
    const int b = T.b, y0 = T.y0;
    const UpStrip S = up_strip(T, hp, wp, OH, OW, stride);
    float mx[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) mx[j] = -INFINITY;
    const size_t plane = T.plane;
    float* base = state + (size_t)b * C * plane + T.pix0;

    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cn = C - c0 < CC ? C - c0 : CC;
        if (c0) __syncthreads();
        up_stage(rfs_lds, logp, b, hp, wp, C, S.fr0, S.fc0, S.ncols, S.ncells, c0, cn, stride, kw_log2);
        __syncthreads();
        if (!T.active) continue;
        for (int k = 0; k < cn; ++k) {
            const float* p = rfs_lds + k;
            UpWalk w(p, S.ro0[0], S.ro1[0], S.off0, S.off1, S.lx);
#pragma unroll
            for (int j = 0; j < UP_ROWS; ++j) {
                const float v = w.at(p, j > 0 && S.ro0[j] != S.ro0[j - 1], S.ro1[j], S.off0, S.off1, S.lx, S.ly[j]);
                const float g = gain * v;
                mx[j] = __builtin_fmaxf(mx[j], g);
                if (T.x_ok && y0 + j < OH) base[(size_t)(c0 + k) * plane + (size_t)j * OW] = g;
            }
        }
    }
    if (!T.active || !T.x_ok) return;
    // the lane's own stores, read back in class order
    for (int j = 0; j < UP_ROWS; ++j) {
        if (y0 + j >= OH) break;
        float* q = base + (size_t)j * OW;
        float sum = 0.f;
        for (int k = 0; k < C; ++k) {
            const float e = up_exp(q[(size_t)k * plane] - mx[j]);
            q[(size_t)k * plane] = e;
            sum += e;
        }
        const float inv = __fdiv_rn(1.0f, sum);
        for (int k = 0; k < C; ++k) q[(size_t)k * plane] *= inv;
    }
}

__global__ __launch_bounds__(256) void refine_label_kernel(const float* __restrict__ state, int C, size_t plane, size_t npix,
                                                           int32_t* __restrict__ labels, float* __restrict__ dense) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const size_t b = i / plane, p = i - b * plane;
    const float* src = state + b * (size_t)C * plane + p;
    float best = -INFINITY;
    int idx = 0;
    for (int k = 0; k < C; ++k) {
        const float v = src[(size_t)k * plane];
        if (dense) dense[b * (size_t)C * plane + (size_t)k * plane + p] = v;
        up_first_max(best, idx, v, k);
    }
    if (labels) labels[i] = best > 0.f ? idx : -1;
}

// the staged span of one axis under output pixels first .. last: widened by the halo, clamped to the frame
__host__ __device__ inline void rf_span(int first, int last, int o, int halo, int* f0, int* count) {
    const int a = first - halo < 0 ? 0 : first - halo, b = last + halo > o - 1 ? o - 1 : last + halo;
    *f0 = a;
    *count = b - a + 1;
}

template <int M>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void refine_pass_kernel(
    const uint8_t* __restrict__ guide, const float* __restrict__ src, float* __restrict__ dst, int C, int OH, int OW, int tiles_x,
    int tiles_y, int CC, int plane_words, RefineDil dil, float kconst, int32_t* __restrict__ labels) {
#pragma clang fp contract(off)      // (every fused multiply-add below is written out)
    constexpr int T = 8 * M, S = 9 * M;
    extern __shared__ float rf_lds[];
    uint32_t* colours = reinterpret_cast<uint32_t*>(rf_lds);                    // [nrows][ncols] packed R | G << 8 | B << 16
    float* vals = rf_lds + plane_words;                                         // [CC][nrows][ncols] the pass's state planes
    const UpTile Tl = up_tile(tiles_x, tiles_y, OH, OW);
    const int b = Tl.b, y0 = Tl.y0, halo = dil.d[M - 1];
    int fc0, fr0, ncols, nrows;
    rf_span(Tl.x_first, Tl.x_last, OW, halo, &fc0, &ncols);
    rf_span(Tl.y_first, Tl.y_last, OH, halo, &fr0, &nrows);
    const int ncells = ncols * nrows;                                           // <= plane_words (the host's bound)
    for (int cell = Tl.tid; cell < ncells; cell += 256) {
        const int r = cell / ncols, col = cell - r * ncols;
        const uint8_t* gp = guide + (((size_t)b * OH + fr0 + r) * OW + fc0 + col) * 3;
        colours[cell] = (uint32_t)gp[0] | ((uint32_t)gp[1] << 8) | ((uint32_t)gp[2] << 16);
    }

    // the lane's clamped tap columns as footprint offsets: per dilation x - d, x, x + d
    const int xo = Tl.xc - fc0;
    int cof[M][3];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int d = dil.d[m];
        cof[m][0] = (Tl.xc - d < 0 ? 0 : Tl.xc - d) - fc0;
        cof[m][1] = xo;
        cof[m][2] = (Tl.xc + d > OW - 1 ? OW - 1 : Tl.xc + d) - fc0;
    }
    float best[UP_ROWS];
    int idx[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        best[j] = -INFINITY;
        idx[j] = 0;
    }
    const size_t plane = Tl.plane, pix0 = Tl.pix0;

    for (int k0 = 0; k0 < C; k0 += CC) {
        const int cn = C - k0 < CC ? C - k0 : CC;
        __syncthreads();                                                        // (the colours, or the last pass's readers)
        for (int k = 0; k < cn; ++k) {
            const float* sp = src + ((size_t)b * C + k0 + k) * plane;
            float* vp = vals + (size_t)k * plane_words;
            for (int cell = Tl.tid; cell < ncells; cell += 256) {
                const int r = cell / ncols, col = cell - r * ncols;
                vp[cell] = sp[(size_t)(fr0 + r) * OW + fc0 + col];
            }
        }
        __syncthreads();
        if (!Tl.active) continue;
#pragma unroll 1
        for (int j = 0; j < UP_ROWS; ++j) {
            const int y = y0 + j < OH ? y0 + j : OH - 1;                        // (the same for the whole wave)
            float w[T];
            int off[T];
            float inv;
            {
                const uint32_t q0 = colours[(y - fr0) * ncols + xo];
                const int g0 = (int)(q0 & 255u), g1 = (int)((q0 >> 8) & 255u), g2 = (int)(q0 >> 16);
                // the centre counts once per dilation
                int s10 = M * g0, s11 = M * g1, s12 = M * g2, s20 = M * g0 * g0, s21 = M * g1 * g1, s22 = M * g2 * g2;
                uint32_t a[T];                                                  // |differences| packed like the colours
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const int d = dil.d[m];
                    const int ro[3] = {((y - d < 0 ? 0 : y - d) - fr0) * ncols, (y - fr0) * ncols,
                                       ((y + d > OH - 1 ? OH - 1 : y + d) - fr0) * ncols};
                    int t = 8 * m;
#pragma unroll
                    for (int iy = 0; iy < 3; ++iy)
#pragma unroll
                        for (int ix = 0; ix < 3; ++ix) {
                            if (iy == 1 && ix == 1) continue;
                            const int cell = ro[iy] + cof[m][ix];
                            const uint32_t q = colours[cell];
                            const int c0 = (int)(q & 255u), c1 = (int)((q >> 8) & 255u), c2 = (int)(q >> 16);
                            s10 += c0;
                            s11 += c1;
                            s12 += c2;
                            s20 += c0 * c0;
                            s21 += c1 * c1;
                            s22 += c2 * c2;
                            const int e0 = g0 - c0, e1 = g1 - c1, e2 = g2 - c2;
                            a[t] = (uint32_t)(e0 < 0 ? -e0 : e0) | ((uint32_t)(e1 < 0 ? -e1 : e1) << 8) | ((uint32_t)(e2 < 0 ? -e2 : e2) << 16);
                            off[t] = cell;
                            ++t;
                        }
                }
                const int n0 = S * s20 - s10 * s10, n1 = S * s21 - s11 * s11, n2 = S * s22 - s12 * s12;
                const float r0 = n0 == 0 ? 0.f : __fdiv_rn(kconst, __fsqrt_rn((float)n0));
                const float r1 = n1 == 0 ? 0.f : __fdiv_rn(kconst, __fsqrt_rn((float)n1));
                const float r2 = n2 == 0 ? 0.f : __fdiv_rn(kconst, __fsqrt_rn((float)n2));
                float emax = -INFINITY;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    float e = (float)(a[t] & 255u) * r0;
                    e = __builtin_fmaf((float)((a[t] >> 8) & 255u), r1, e);
                    e = __builtin_fmaf((float)(a[t] >> 16), r2, e);
                    w[t] = -e;
                    emax = __builtin_fmaxf(emax, w[t]);
                }
                float W = 0.f;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    w[t] = __builtin_amdgcn_exp2f(w[t] - emax);
                    W += w[t];
                }
                inv = __fdiv_rn(1.0f, W);
            }
            float bv = -INFINITY;
            int bi = 0;
#pragma unroll
            for (int jj = 0; jj < UP_ROWS; ++jj)
                if (jj == j) {
                    bv = best[jj];
                    bi = idx[jj];
                }
            const bool store = dst != nullptr && Tl.x_ok && y0 + j < OH;
            float* dp = dst ? dst + ((size_t)b * C + k0) * plane + pix0 + (size_t)j * OW : nullptr;
            auto classes = [&](int k, auto n_) {
                constexpr int N = decltype(n_)::value;
                float acc[N];
#pragma unroll
                for (int n = 0; n < N; ++n) acc[n] = 0.f;
                const float* vk = vals + (size_t)k * plane_words;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float* q = vk + off[t];
                    float v[N];
#pragma unroll
                    for (int n = 0; n < N; ++n) v[n] = q[(size_t)n * plane_words];
#pragma unroll
                    for (int n = 0; n < N; ++n) acc[n] = __builtin_fmaf(w[t], v[n], acc[n]);
                }
#pragma unroll
                for (int n = 0; n < N; ++n) {
                    const float v = acc[n] * inv;
                    if (store) *dp = v;
                    if (dst) dp += plane;                                       // (walks the classes of the pass in order)
                    up_first_max(bv, bi, v, k0 + k + n);
                }
            };
            int k = 0;
            for (; k + RF_CLASSES <= cn; k += RF_CLASSES) classes(k, std::integral_constant<int, RF_CLASSES>());
            for (; k < cn; ++k) classes(k, std::integral_constant<int, 1>());
#pragma unroll
            for (int jj = 0; jj < UP_ROWS; ++jj)
                if (jj == j) {
                    best[jj] = bv;
                    idx[jj] = bi;
                }
        }
    }
    if (labels && Tl.active && Tl.x_ok) {
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j)
            if (y0 + j < OH) labels[(size_t)b * plane + pix0 + (size_t)j * OW] = best[j] > 0.f ? idx[j] : -1;
    }
}

template <int M>
const void* rf_fn() {
    return reinterpret_cast<const void*>(&refine_pass_kernel<M>);
}

int rf_allow_large_lds() {
    static PerDeviceOnce once;
    if (!once.first()) return 0;
    const void* fn[REFINE_MAX_DIL] = {rf_fn<1>(), rf_fn<2>(), rf_fn<3>(), rf_fn<4>(), rf_fn<5>(), rf_fn<6>()};
    for (int i = 0; i < REFINE_MAX_DIL; ++i) {
        const hipError_t e = hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, UP_LDS_LARGE_WORDS * (int)sizeof(float));
        if (e != hipSuccess) {
            dinoseg_set_error("hipFuncSetAttribute(refine_pass_kernel<%d>, MaxDynamicSharedMemorySize) failed: %s", i + 1, hipGetErrorString(e));
            return -2;
        }
    }
    once.mark();
    return 0;
}

template <int M>
void rf_launch(unsigned grid, hipStream_t s, const uint8_t* guide, const float* src, float* dst, int C, int OH, int OW, const RefinePlan& pl,
               const RefineDil& dil, int32_t* labels) {
    hipLaunchKernelGGL((refine_pass_kernel<M>), dim3(grid), dim3(256), pl.lds_bytes, s, guide, src, dst, C, OH, OW, pl.tiles_x, pl.tiles_y,
                       pl.CC, pl.plane_words, dil, pl.k, labels);
}

int rf_check_frame(const char* who, int B, int C, int OH, int OW) {
    if (B < 1 || C < 1 || C > REFINE_MAX_C || OH < 1 || OW < 1 || OH > REFINE_MAX_SIDE || OW > REFINE_MAX_SIDE) {
        dinoseg_set_error("%s: bad argument (B=%d C=%d OH=%d OW=%d; B >= 1, 1 <= C <= %d, 1 <= OH, OW <= %d)", who, B, C, OH, OW, REFINE_MAX_C,
                          REFINE_MAX_SIDE);
        return -1;
    }
    const long long tiles = (long long)((OW + UP_TW - 1) / UP_TW) * ((OH + UP_TH - 1) / UP_TH);
    if (tiles * B > 0x7fffffffll || ((long long)B * OH * OW + 255) / 256 > 0x7fffffffll) {
        dinoseg_set_error("%s: %d frames of %dx%d are too many for one launch", who, B, OH, OW);
        return -1;
    }
    return 0;
}

}  // namespace

long long refine_scratch_bytes(int B, int C, int OH, int OW) {
    if (rf_check_frame("dinoseg_refine_scratch_bytes", B, C, OH, OW)) return -1;
    return 2ll * B * C * OH * OW * (long long)sizeof(float);
}

int refine_seed_check(const char* who, int kind, int B, int C, int OH, int OW, int hp, int wp, double gain) {
    if (kind != REFINE_SEED_LABELS && kind != REFINE_SEED_SCORES) {
        dinoseg_set_error("%s: kind=%d must be 0 (labels) or 1 (scores)", who, kind);
        return -1;
    }
    if (rf_check_frame(who, B, C, OH, OW)) return -1;
    if (kind == REFINE_SEED_SCORES) {
        if (!(std::isfinite(gain) && gain > 0.0 && std::isfinite((float)gain) && (float)gain > 0.f)) {
            dinoseg_set_error("%s: gain=%g must be positive and finite", who, gain);
            return -1;
        }
        if (upsample_check_shape(who, B, hp, wp, C, OH, OW)) return -1;
    }
    return 0;
}

int launch_refine_seed(const char* who, const void* seed, int kind, int B, int C, int OH, int OW, int hp, int wp, double gain, void* scratch,
                       hipStream_t s) {
    if (!seed || !scratch) {
        dinoseg_set_error("%s: null pointer (seed and scratch are required)", who);
        return -1;
    }
    if (refine_seed_check(who, kind, B, C, OH, OW, hp, wp, gain)) return -1;
    float* state = static_cast<float*>(scratch);
    const size_t plane = (size_t)OH * OW, npix = plane * B;
    if (kind == REFINE_SEED_LABELS) {
        hipLaunchKernelGGL(refine_seed_labels_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, static_cast<const int32_t*>(seed), C,
                           plane, npix, state);
    } else {
        UpTilePlan pl;
        if (upsample_tile_plan(who, hp, wp, C, OH, OW, &pl)) return -1;
        const unsigned grid = (unsigned)((long long)pl.tiles_x * pl.tiles_y * B);
        hipLaunchKernelGGL(refine_seed_scores_kernel, dim3(grid), dim3(256), pl.lds_bytes, s, static_cast<const float*>(seed), hp, wp, C, OH, OW,
                           pl.tiles_x, pl.tiles_y, pl.CC, pl.stride, pl.kw_log2, (float)gain, state);
    }
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int refine_iterate_check(const char* who, int B, int C, int OH, int OW, const int32_t* dilations, int n_dil, double sigma, int iters,
                         RefinePlan* plan) {
    if (rf_check_frame(who, B, C, OH, OW)) return -1;
    if (!dilations) {
        dinoseg_set_error("%s: null pointer (dilations is a host array of n_dil entries)", who);
        return -1;
    }
    if (n_dil < 1 || n_dil > REFINE_MAX_DIL) {
        dinoseg_set_error("%s: n_dil=%d must be in 1..%d", who, n_dil, REFINE_MAX_DIL);
        return -1;
    }
    for (int m = 0; m < n_dil; ++m) {
        if (dilations[m] < 1 || dilations[m] > REFINE_MAX_DILATION) {
            dinoseg_set_error("%s: dilation %d (entry %d) must be in 1..%d", who, dilations[m], m, REFINE_MAX_DILATION);
            return -1;
        }
        if (m && dilations[m] <= dilations[m - 1]) {
            dinoseg_set_error("%s: dilations must ascend strictly (entry %d = %d after %d)", who, m, dilations[m], dilations[m - 1]);
            return -1;
        }
    }
    if (!(std::isfinite(sigma) && sigma >= 1e-3 && sigma <= 1e3)) {
        dinoseg_set_error("%s: sigma=%g must be in [1e-3, 1e3]", who, sigma);
        return -1;
    }
    if (iters < 0 || iters > REFINE_MAX_ITERS) {
        dinoseg_set_error("%s: iters=%d must be in 0..%d", who, iters, REFINE_MAX_ITERS);
        return -1;
    }
    const int halo = dilations[n_dil - 1];
    const long long cols = OW < UP_TW + 2 * halo ? OW : UP_TW + 2 * halo, rows = OH < UP_TH + 2 * halo ? OH : UP_TH + 2 * halo;
    const long long words = cols * rows;                                        // <= 112 * 80
    long long CC = UP_LDS_LARGE_WORDS / words - 1;                              // one plane of colours beside CC planes of state
    if (CC < 1) {
        dinoseg_set_error("%s: a tile's footprint of %lld pixels (halo %d) exceeds the LDS budget", who, words, halo);
        return -1;
    }
    if (CC > C) CC = C;
    if (plan) {
        const double S = 9.0 * n_dil, l2e = 1.44269504088896340736;
        *plan = {(OW + UP_TW - 1) / UP_TW, (OH + UP_TH - 1) / UP_TH, (int)CC, (int)words, (size_t)(words * (CC + 1)) * sizeof(float),
                 (float)(l2e * std::sqrt(S * (S - 1.0)) / (3.0 * sigma))};
    }
    return 0;
}

int launch_refine_iterate(const char* who, const uint8_t* guide, void* scratch, int B, int C, int OH, int OW, const int32_t* dilations,
                          int n_dil, double sigma, int iters, int32_t* labels, float* dense, hipStream_t s) {
    if (!guide || !scratch || (!labels && !dense)) {
        dinoseg_set_error("%s: null pointer (guide, scratch, and at least one of labels_out / dense_out, are required)", who);
        return -1;
    }
    RefinePlan pl;
    if (refine_iterate_check(who, B, C, OH, OW, dilations, n_dil, sigma, iters, &pl)) return -1;
    float* half[2] = {static_cast<float*>(scratch), static_cast<float*>(scratch) + (size_t)B * C * OH * OW};
    if (iters == 0) {
        const size_t plane = (size_t)OH * OW, npix = plane * B;
        hipLaunchKernelGGL(refine_label_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, half[0], C, plane, npix, labels, dense);
        DSEG_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (pl.lds_bytes > (size_t)UP_LDS_WORDS * sizeof(float)) {
        const int rc = rf_allow_large_lds();
        if (rc) return rc;
    }
    RefineDil dil = {};
    for (int m = 0; m < n_dil; ++m) dil.d[m] = dilations[m];
    const unsigned grid = (unsigned)((long long)pl.tiles_x * pl.tiles_y * B);
    for (int it = 0; it < iters; ++it) {
        const bool last = it == iters - 1;
        const float* src = half[it & 1];
        float* dst = last ? dense : half[(it + 1) & 1];
        int32_t* lab = last ? labels : nullptr;
        switch (n_dil) {
            case 1: rf_launch<1>(grid, s, guide, src, dst, C, OH, OW, pl, dil, lab); break;
            case 2: rf_launch<2>(grid, s, guide, src, dst, C, OH, OW, pl, dil, lab); break;
            case 3: rf_launch<3>(grid, s, guide, src, dst, C, OH, OW, pl, dil, lab); break;
            case 4: rf_launch<4>(grid, s, guide, src, dst, C, OH, OW, pl, dil, lab); break;
            case 5: rf_launch<5>(grid, s, guide, src, dst, C, OH, OW, pl, dil, lab); break;
            default: rf_launch<6>(grid, s, guide, src, dst, C, OH, OW, pl, dil, lab); break;
        }
        DSEG_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace dseg
