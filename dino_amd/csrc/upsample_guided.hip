// Image-guided pixel-resolution output: joint bilateral upsampling (Kopf et al. 2007) of the head's log-probabilities, guided by the
// full-resolution uint8 frame, fused with the argmax over classes.  The rule is stated in full in include/dinoseg.h
// (dinoseg_op_upsample_guided); in short, per output pixel the values of the (2R+1)^2 cells around its own cell are averaged with
// weights exp2(-(spatial distance^2) a_s - (colour distance^2 - the smallest one) a_r), the colour of a cell being the rounded mean
// of the guide over the cell's pixels.
//
//   guide_cells_kernel       one wave per cell: the lanes stride over the cell's pixels (the nearest rule: pixel (y, x) belongs to
//                            cell ((y hp) / OH, (x wp) / OW)), integer sums per channel, the xor tree of the wave (integer sums do not
//                            depend on their order), m = (2 sum + n) / (2 n), one packed uint32 per cell.  No atomics.
//   upsample_guided_kernel   the family's geometry (upsample_common.h): one workgroup per 64 x 32 output tile, wave w rows 8w .. 8w+7,
//                            lane l column l.  The tile's cells under the nearest rule plus an R-cell halo clamped to the grid are
//                            staged in LDS: the packed colours once, the log-probs CC classes at a time, cell-major with the odd
//                            stride.  A lane takes its 8 pixels one at a time: the (2R+1)^2 weights and LDS offsets of the pixel are
//                            formed in registers (R is a template parameter: the arrays unroll), then the staged classes are walked
//                            with one LDS read and one fmaf per tap and class.  Lanes inside one cell read one address (a broadcast),
//                            lanes in different cells different banks by the odd stride.  A tap outside the grid reads a clamped cell
//                            with weight 0 (fmaf(0, finite, acc) == acc: the same bits as skipping it).  The running first maximum of
//                            the 8 pixels stays in registers across class passes; with C > CC the weights are formed again per pass.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

#include <cmath>
#include <type_traits>

namespace dseg {

namespace {

constexpr int UPG_MAX_R = 3;
// classes a lane accumulates side by side (independent chains, all their LDS reads in flight before the first use): as many as the
// registers hold beside the (2R+1)^2 weights and offsets
constexpr int upg_classes(int R) { return R >= 3 ? 2 : 4; }
constexpr int UPG_OUTSIDE = 1 << 30;        // above every squared colour distance (<= 195 075)
constexpr int UPG_MAX_SIDE = 1 << 20;       // keeps float(my) exact: |my| <= (2R + 2) OH < 2^24

__global__ __launch_bounds__(256) void guide_cells_kernel(const uint8_t* __restrict__ guide, int OH, int OW, int hp, int wp, long long ncell,
                                                          uint32_t* __restrict__ cells) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= ncell) return;                                          // (a whole wave: no barrier follows)
    const int c = (int)(cell % wp);
    const long long t = cell / wp;
    const int r = (int)(t % hp);
    const long long b = t / hp;
    // the pixels y with (y hp) / OH == r: ceil(r OH / hp) .. ceil((r + 1) OH / hp) - 1 (never empty: OH >= hp)
    const int y0 = (int)(((long long)r * OH + hp - 1) / hp), y1 = (int)(((long long)(r + 1) * OH + hp - 1) / hp);
    const int x0 = (int)(((long long)c * OW + wp - 1) / wp), x1 = (int)(((long long)(c + 1) * OW + wp - 1) / wp);
    const int cw = x1 - x0;
    const long long n = (long long)(y1 - y0) * cw;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    for (long long i = lane; i < n; i += 64) {
        const int yy = (int)(i / cw), xx = (int)(i - (long long)yy * cw);
        const uint8_t* p = guide + ((size_t)(b * OH + y0 + yy) * OW + x0 + xx) * 3;
        s0 += p[0];
        s1 += p[1];
        s2 += p[2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        const unsigned long long d = 2ull * (unsigned long long)n;
        const uint32_t m0 = (uint32_t)((2 * s0 + n) / d), m1 = (uint32_t)((2 * s1 + n) / d), m2 = (uint32_t)((2 * s2 + n) / d);
        cells[cell] = m0 | (m1 << 8) | (m2 << 16);
    }
}

// the cells of an axis under output pixels first .. last by the nearest rule, widened by the halo and clamped to the grid
__host__ __device__ inline void upg_span(int first, int last, int i, int o, int R, int* f0, int* count) {
    int a = (int)(((unsigned)first * (unsigned)i) / (unsigned)o) - R, b = (int)(((unsigned)last * (unsigned)i) / (unsigned)o) + R;
    if (a < 0) a = 0;
    if (b > i - 1) b = i - 1;
    *f0 = a;
    *count = b - a + 1;
}

template <int R, bool DENSE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void upsample_guided_kernel(const float* __restrict__ logp, const uint8_t* __restrict__ guide,
                                                              const uint32_t* __restrict__ cells, int hp, int wp, int C, int OH, int OW,
                                                              int tiles_x, int tiles_y, int CC, int stride, int kw_log2, int col_words,
                                                              float a_s, float a_r, int32_t* __restrict__ labels,
                                                              float* __restrict__ dense) {
#pragma clang fp contract(off)      // (every fused multiply-add below is written out: both instantiations round alike)
    constexpr int S = 2 * R + 1, T = S * S;
    extern __shared__ float upg_lds[];
    const uint32_t* colours = reinterpret_cast<const uint32_t*>(upg_lds);       // [ncells] packed cell colours
    float* vals = upg_lds + col_words;                                          // [ncells][stride] the pass's log-probs
    const UpTile Tl = up_tile(tiles_x, tiles_y, OH, OW);
    const int b = Tl.b, y0 = Tl.y0;
    int fc0, fr0, ncols, nrows;
    upg_span(Tl.x_first, Tl.x_last, wp, OW, R, &fc0, &ncols);
    upg_span(Tl.y_first, Tl.y_last, hp, OH, R, &fr0, &nrows);
    const int ncells = ncols * nrows;
    for (int cell = Tl.tid; cell < ncells; cell += 256) {
        const int r = cell / ncols, col = cell - r * ncols;
        reinterpret_cast<uint32_t*>(upg_lds)[cell] = cells[((size_t)b * hp + fr0 + r) * wp + fc0 + col];
    }

    // the lane's column: its cell, the clamped tap columns as footprint offsets and their squared distances.  A column outside the grid
    // carries an infinite distance (its weight is exp2(-inf) = 0) and a bit above every D (it never sets Dmin); rows likewise below.
    const int c0 = (int)(((unsigned)Tl.xc * (unsigned)wp) / (unsigned)OW);
    int coff[S], cbad[S];
    float dx2[S];
    {
        const int mx0 = 2 * c0 * OW - ((2 * Tl.xc + 1) * wp - OW);
        const float den = (float)(2 * OW);
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const int c = c0 + i - R;
            const bool cok = c >= 0 && c < wp;
            cbad[i] = cok ? 0 : UPG_OUTSIDE;
            coff[i] = (c < 0 ? 0 : c > wp - 1 ? wp - 1 : c) - fc0;
            const float dx = __fdiv_rn((float)(mx0 + 2 * (i - R) * OW), den);
            dx2[i] = cok ? dx * dx : INFINITY;
        }
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
        if (k0) __syncthreads();
        up_stage(vals, logp, b, hp, wp, C, fr0, fc0, ncols, ncells, k0, cn, stride, kw_log2);
        __syncthreads();
        if (!Tl.active) continue;
#pragma unroll 1
        for (int j = 0; j < UP_ROWS; ++j) {
            const int y = y0 + j < OH ? y0 + j : OH - 1;
            const int r0 = (int)(((unsigned)y * (unsigned)hp) / (unsigned)OH);  // (the same for the whole wave)
            float w[T];
            int off[T];
            float inv = 1.0f;
            if constexpr (R == 0) {
                w[0] = 1.0f;                                                    // one tap: the quotient is its value, bit for bit
                off[0] = ((r0 - fr0) * ncols + coff[0]) * stride;
            } else {
                const uint8_t* gp = guide + (((size_t)b * OH + y) * OW + Tl.xc) * 3;
                const int g0 = gp[0], g1 = gp[1], g2 = gp[2];
                const int my0 = 2 * r0 * OH - ((2 * y + 1) * hp - OH);
                const float den = (float)(2 * OH);
                int D[T];
                int Dmin = 0x7fffffff;
#pragma unroll
                for (int a = 0; a < S; ++a) {
                    const int r = r0 + a - R;
                    const int rbad = r >= 0 && r < hp ? 0 : UPG_OUTSIDE;
                    const int roff = ((r < 0 ? 0 : r > hp - 1 ? hp - 1 : r) - fr0) * ncols;
#pragma unroll
                    for (int i = 0; i < S; ++i) {
                        const int t = a * S + i, cell = roff + coff[i];
                        const uint32_t q = colours[cell];
                        const int e0 = g0 - (int)(q & 255u), e1 = g1 - (int)((q >> 8) & 255u), e2 = g2 - (int)(q >> 16);
                        D[t] = e0 * e0 + e1 * e1 + e2 * e2;
                        off[t] = cell * stride;
                        const int dm = D[t] | rbad | cbad[i];
                        if (dm < Dmin) Dmin = dm;
                    }
                }
                float W = 0.f;
#pragma unroll
                for (int a = 0; a < S; ++a) {
                    const float dy = __fdiv_rn((float)(my0 + 2 * (a - R) * OH), den);
                    const int r = r0 + a - R;
                    const float dy2 = r >= 0 && r < hp ? dy * dy : INFINITY;
#pragma unroll
                    for (int i = 0; i < S; ++i) {
                        const int t = a * S + i;
                        const float s = dy2 + dx2[i];
                        const float e = -(s * a_s) - (float)(D[t] - Dmin) * a_r;
                        w[t] = __builtin_amdgcn_exp2f(e);
                        W += w[t];
                    }
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
            const bool store = DENSE && Tl.x_ok && y0 + j < OH;
            float* dp = DENSE ? dense + ((size_t)b * C + k0) * plane + pix0 + (size_t)j * OW : nullptr;
            // N classes at a time: per tap one address and N reads at constant offsets, N independent fmaf chains (each in tap order)
            auto classes = [&](int k, auto n_) {
                constexpr int N = decltype(n_)::value;
                float acc[N];
#pragma unroll
                for (int n = 0; n < N; ++n) acc[n] = 0.f;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float* q = vals + off[t] + k;
                    float v[N];
#pragma unroll
                    for (int n = 0; n < N; ++n) v[n] = q[n];
#pragma unroll
                    for (int n = 0; n < N; ++n) acc[n] = __builtin_fmaf(w[t], v[n], acc[n]);
                }
#pragma unroll
                for (int n = 0; n < N; ++n) {
                    const float v = acc[n] * inv;
                    if (DENSE) {
                        if (store) *dp = v;
                        dp += plane;                                            // (walks the classes of the pass in order)
                    }
                    up_first_max(bv, bi, v, k0 + k + n);
                }
            };
            int k = 0;
            for (; k + upg_classes(R) <= cn; k += upg_classes(R)) classes(k, std::integral_constant<int, upg_classes(R)>());
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
            if (y0 + j < OH) labels[(size_t)b * plane + pix0 + (size_t)j * OW] = idx[j];
    }
}

// the widest run of cells, along one axis, under any tile of `step` output pixels: the kernel's own span rule
int upg_max_span(int i, int o, int step, int R) {
    int widest = 1;
    for (int first = 0; first < o; first += step) {
        const int last = (first + step < o ? first + step : o) - 1;
        int f0, n;
        upg_span(first, last, i, o, R, &f0, &n);
        if (n > widest) widest = n;
    }
    return widest;
}

template <int R>
const void* upg_fn(bool dense) {
    return dense ? reinterpret_cast<const void*>(&upsample_guided_kernel<R, true>) : reinterpret_cast<const void*>(&upsample_guided_kernel<R, false>);
}

int upg_allow_large_lds() {
    static PerDeviceOnce once;
    if (!once.first()) return 0;
    const void* fn[8] = {upg_fn<0>(true), upg_fn<0>(false), upg_fn<1>(true), upg_fn<1>(false),
                         upg_fn<2>(true), upg_fn<2>(false), upg_fn<3>(true), upg_fn<3>(false)};
    for (int i = 0; i < 8; ++i) {
        const hipError_t e = hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, UP_LDS_LARGE_WORDS * (int)sizeof(float));
        if (e != hipSuccess) {
            dinoseg_set_error("hipFuncSetAttribute(upsample_guided_kernel<%d, %s>, MaxDynamicSharedMemorySize) failed: %s", i / 2,
                              i % 2 ? "false" : "true", hipGetErrorString(e));
            return -2;
        }
    }
    once.mark();
    return 0;
}

template <int R>
void upg_launch(bool want_dense, unsigned grid, size_t lds, hipStream_t s, const float* logp, const uint8_t* guide, const uint32_t* cells, int hp,
                int wp, int C, int OH, int OW, const UpGuidedPlan& pl, int32_t* labels, float* dense) {
    if (want_dense)
        hipLaunchKernelGGL((upsample_guided_kernel<R, true>), dim3(grid), dim3(256), lds, s, logp, guide, cells, hp, wp, C, OH, OW, pl.tiles_x,
                           pl.tiles_y, pl.CC, pl.stride, pl.kw_log2, pl.col_words, pl.a_s, pl.a_r, labels, dense);
    else
        hipLaunchKernelGGL((upsample_guided_kernel<R, false>), dim3(grid), dim3(256), lds, s, logp, guide, cells, hp, wp, C, OH, OW, pl.tiles_x,
                           pl.tiles_y, pl.CC, pl.stride, pl.kw_log2, pl.col_words, pl.a_s, pl.a_r, labels, dense);
}

}  // namespace

int guide_cells_check(const char* who, int B, int hp, int wp, int OH, int OW) {
    if (B < 1 || hp < 1 || wp < 1 || OH < 1 || OW < 1) {
        dinoseg_set_error("%s: bad argument (B=%d hp=%d wp=%d OH=%d OW=%d; sizes must be positive)", who, B, hp, wp, OH, OW);
        return -1;
    }
    if (OH < hp || OW < wp) {
        dinoseg_set_error("%s: guide %dx%d is smaller than the cell grid %dx%d (every cell needs a pixel)", who, OH, OW, hp, wp);
        return -1;
    }
    if (OH > UPG_MAX_SIDE || OW > UPG_MAX_SIDE || ((long long)B * hp * wp + 3) / 4 > 0x7fffffffll) {
        dinoseg_set_error("%s: guide %dx%d (B=%d, grid %dx%d) is too large (sides up to %d)", who, OH, OW, B, hp, wp, UPG_MAX_SIDE);
        return -1;
    }
    return 0;
}

int launch_guide_cells(const char* who, const uint8_t* guide, int B, int OH, int OW, int hp, int wp, uint32_t* cells, hipStream_t s) {
    if (!guide || !cells) {
        dinoseg_set_error("%s: null pointer (guide and cells are required)", who);
        return -1;
    }
    if (guide_cells_check(who, B, hp, wp, OH, OW)) return -1;
    const long long ncell = (long long)B * hp * wp;
    hipLaunchKernelGGL(guide_cells_kernel, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, s, guide, OH, OW, hp, wp, ncell, cells);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int upsample_guided_check(const char* who, int B, int hp, int wp, int C, int OH, int OW, int radius, double sigma_spatial, double sigma_range,
                          UpGuidedPlan* plan) {
    if (radius < 0 || radius > UPG_MAX_R) {
        dinoseg_set_error("%s: radius=%d must be in 0..%d", who, radius, UPG_MAX_R);
        return -1;
    }
    if (!(std::isfinite(sigma_spatial) && sigma_spatial >= 0.5 && sigma_spatial <= 16.0)) {
        dinoseg_set_error("%s: sigma_spatial=%g must be in [0.5, 16] (cells)", who, sigma_spatial);
        return -1;
    }
    if (!(std::isfinite(sigma_range) && sigma_range >= 1e-3 && sigma_range <= 1e3)) {
        dinoseg_set_error("%s: sigma_range=%g must be in [1e-3, 1e3] (of the 0..255 range)", who, sigma_range);
        return -1;
    }
    if (upsample_check_shape(who, B, hp, wp, C, OH, OW)) return -1;
    if (OH > UPG_MAX_SIDE || OW > UPG_MAX_SIDE) {
        dinoseg_set_error("%s: output %dx%d is too large (sides up to %d)", who, OH, OW, UPG_MAX_SIDE);
        return -1;
    }
    const long long cells = (long long)upg_max_span(wp, OW, UP_TW, radius) * upg_max_span(hp, OH, UP_TH, radius);     // <= 70 * 38
    long long budget = 0;
    const UpPass ps = up_pass_two_budgets(cells, cells, C, &budget);
    if (ps.CC < 1) {
        dinoseg_set_error("%s: a tile's footprint of %lld cells (radius %d) exceeds the LDS budget", who, cells, radius);
        return -1;
    }
    if (plan) {
        const double l2e = 1.44269504088896340736, sr = 255.0 * sigma_range;
        *plan = {(OW + UP_TW - 1) / UP_TW, (OH + UP_TH - 1) / UP_TH, ps.CC, ps.stride, ps.kw_log2, (int)cells,
                 (size_t)(cells + cells * ps.stride) * sizeof(float), (float)(l2e / (2.0 * sigma_spatial * sigma_spatial)),
                 (float)(l2e / (2.0 * sr * sr))};
    }
    return 0;
}

int launch_upsample_guided(const char* who, const float* logp, const uint8_t* guide, const uint32_t* cells, int B, int hp, int wp, int C, int OH, int OW,
                           int radius, double sigma_spatial, double sigma_range, int32_t* labels, float* dense, hipStream_t s) {
    if (!logp || !guide || !cells || (!labels && !dense)) {
        dinoseg_set_error("%s: null pointer (logp, guide, cells, and at least one of labels / dense, are required)", who);
        return -1;
    }
    UpGuidedPlan pl;
    if (upsample_guided_check(who, B, hp, wp, C, OH, OW, radius, sigma_spatial, sigma_range, &pl)) return -1;
    if (pl.lds_bytes > (size_t)UP_LDS_WORDS * sizeof(float)) {
        const int rc = upg_allow_large_lds();
        if (rc) return rc;
    }
    const unsigned grid = (unsigned)((long long)pl.tiles_x * pl.tiles_y * B);
    switch (radius) {
        case 0: upg_launch<0>(dense != nullptr, grid, pl.lds_bytes, s, logp, guide, cells, hp, wp, C, OH, OW, pl, labels, dense); break;
        case 1: upg_launch<1>(dense != nullptr, grid, pl.lds_bytes, s, logp, guide, cells, hp, wp, C, OH, OW, pl, labels, dense); break;
        case 2: upg_launch<2>(dense != nullptr, grid, pl.lds_bytes, s, logp, guide, cells, hp, wp, C, OH, OW, pl, labels, dense); break;
        default: upg_launch<3>(dense != nullptr, grid, pl.lds_bytes, s, logp, guide, cells, hp, wp, C, OH, OW, pl, labels, dense); break;
    }
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
