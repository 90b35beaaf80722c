// Pixel-resolution output: bilinear upsample of the head's log-probabilities fused with the argmax over classes.
//
// What a ViT segmenter does after the head -- F.interpolate(logp [B, C, hp, wp], size=(OH, OW), mode="bilinear",
// align_corners=False).argmax(1) -- without the [B, C, OH, OW] fp32 transient: the low-res log-probs are read once, the running
// maximum of every pixel stays in registers, 4 bytes per pixel are written (and, on request, the dense values in torch's layout).
//
// Coordinates are exact.  Per axis, input size i, output size o, output index d:
//     num = max((2d + 1) i - o, 0),  den = 2 o                    (integers)
//     i0 = min(num / den, i - 1),  i1 = min(i0 + 1, i - 1)
//     lambda = float(num % den) / float(den),  0 when num / den >= i - 1
// and the value is a + (b - a) lambda (one fused multiply-add), along x and then along y, in fp32.  The label is the FIRST
// maximum over classes (head_final's tie rule).  An fp32 source coordinate would carry ulp(80) ~ 5e-6 into lambda.
//
// One workgroup = one 64 x 32 output tile of one frame, its source footprint staged in LDS CC classes at a time and walked strip
// by strip (upsample_common.h: the tile, the staging and the walk of the whole family).  What is this kernel's own: a lane keeps
// the running first maximum of its 8 pixels in registers, and stores each value as it is formed when the dense values are asked for.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

template <bool DENSE>
__global__ __launch_bounds__(256) void upsample_argmax_kernel(const float* __restrict__ logp, int hp, int wp, int C, int OH, int OW,
                                                              int tiles_x, int tiles_y, int CC, int stride, int kw_log2,
                                                              int32_t* __restrict__ labels, float* __restrict__ dense) {
    extern __shared__ float up_lds[];
    const UpTile T = up_tile(tiles_x, tiles_y, OH, OW);
    const int b = T.b, y0 = T.y0;
    const UpStrip S = up_strip(T, hp, wp, OH, OW, stride);
    float best[UP_ROWS];
    int idx[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        best[j] = -INFINITY;
        idx[j] = 0;
    }
    const size_t plane = T.plane, pix0 = T.pix0;

    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cn = C - c0 < CC ? C - c0 : CC;
        if (c0) __syncthreads();
        up_stage(up_lds, logp, b, hp, wp, C, S.fr0, S.fc0, S.ncols, S.ncells, c0, cn, stride, kw_log2);
        __syncthreads();
        if (!T.active) continue;
        for (int k = 0; k < cn; ++k) {
            const float* p = up_lds + k;
            UpWalk w(p, S.ro0[0], S.ro1[0], S.off0, S.off1, S.lx);
            const int c = c0 + k;
#pragma unroll
            for (int j = 0; j < UP_ROWS; ++j) {
                const float v = w.at(p, j > 0 && S.ro0[j] != S.ro0[j - 1], S.ro1[j], S.off0, S.off1, S.lx, S.ly[j]);
                if (DENSE) {
                    if (T.x_ok && y0 + j < OH) dense[((size_t)b * C + c) * plane + pix0 + (size_t)j * OW] = v;
                }
                up_first_max(best[j], idx[j], v, c);
            }
        }
    }
    if (labels && T.active && T.x_ok) {
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j)
            if (y0 + j < OH) labels[(size_t)b * plane + pix0 + (size_t)j * OW] = idx[j];
    }
}

// the one shape check of the upsample, for the operator and for dinoseg_forward_dense_hw (which asks before its forward enqueues anything)
int upsample_check_shape(const char* who, int B, int hp, int wp, int C, int OH, int OW) {
    if (B < 1 || hp < 1 || wp < 1 || OH < 1 || OW < 1 || C < 1 || C > HEAD_WIDE_MAX_C) {
        dinoseg_set_error("%s: bad argument (B=%d hp=%d wp=%d C=%d OH=%d OW=%d; sizes must be positive, 1 <= C <= %d)", who, B, hp, wp, C, OH,
                          OW, HEAD_WIDE_MAX_C);
        return -1;
    }
    if (OH < hp || OW < wp) {
        dinoseg_set_error("%s: output %dx%d is smaller than the input grid %dx%d (upsampling and identity only)", who, OH, OW, hp, wp);
        return -1;
    }
    const long long tiles = (long long)((OW + UP_TW - 1) / UP_TW) * ((OH + UP_TH - 1) / UP_TH);
    if (OH > (1 << 22) || OW > (1 << 22) || (2ll * OH + 1) * hp > 0x7fffffffll || (2ll * OW + 1) * wp > 0x7fffffffll ||
        tiles * B > 0x7fffffffll) {
        dinoseg_set_error("%s: output %dx%d (B=%d) is too large", who, OH, OW, B);
        return -1;
    }
    return 0;
}

// ---- the family's host pieces (upsample_common.h)
int up_max_footprint(int i, int o, int step) {
    int widest = 1;
    for (int first = 0; first < o; first += step) {
        const int last = (first + step < o ? first + step : o) - 1;
        int a0, a1, b0, b1;
        unsigned rem;
        up_index(first, i, o, &a0, &a1, &rem);
        up_index(last, i, o, &b0, &b1, &rem);
        if (b1 - a0 + 1 > widest) widest = b1 - a0 + 1;
    }
    return widest;
}

UpPass up_pass_two_budgets(long long tables, long long cells, int C, long long* budget) {
    UpPass ps = up_pass_of(0);
    for (int pass = 0; pass < 2; ++pass) {
        *budget = (pass ? UP_LDS_LARGE_WORDS : UP_LDS_WORDS) - tables;
        ps = cells <= *budget ? up_pass((int)*budget, (int)cells, C) : up_pass_of(0);
        if (ps.CC >= (C < 8 ? C : 8)) break;
    }
    return ps;
}

int up_allow_large_lds(PerDeviceOnce& once, const char* kernel, const void* with_output, const void* without) {
    if (!once.first()) return 0;
    for (int i = 0; i < 2; ++i) {
        const hipError_t e = hipFuncSetAttribute(i ? without : with_output, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 UP_LDS_LARGE_WORDS * (int)sizeof(float));
        if (e != hipSuccess) {
            dinoseg_set_error("hipFuncSetAttribute(%s<%s>, MaxDynamicSharedMemorySize) failed: %s", kernel, i ? "false" : "true",
                              hipGetErrorString(e));
            return -2;
        }
    }
    once.mark();
    return 0;
}

// the tile grid and the LDS staging of a tile's source footprint (upsample_common.h); the shape has passed upsample_check_shape
int upsample_tile_plan(const char* who, int hp, int wp, int C, int OH, int OW, UpTilePlan* plan) {
    const int cells = up_max_footprint(wp, OW, UP_TW) * up_max_footprint(hp, OH, UP_TH);      // <= 65 * 33
    const UpPass ps = up_pass(UP_LDS_WORDS, cells, C);
    if (ps.CC < 1) {
        dinoseg_set_error("upsample_argmax: a tile's footprint of %d cells exceeds the LDS budget", cells);
        return -1;
    }
    *plan = {(OW + UP_TW - 1) / UP_TW, (OH + UP_TH - 1) / UP_TH, ps.CC, ps.stride, ps.kw_log2, (size_t)cells * ps.stride * sizeof(float)};
    return 0;
}

int launch_upsample_argmax(const float* logp, int B, int hp, int wp, int C, int OH, int OW, int32_t* labels, float* dense,
                           hipStream_t s) {
    if (!logp || (!labels && !dense)) {
        dinoseg_set_error("upsample_argmax: null pointer (logp, and at least one of labels / dense, are required)");
        return -1;
    }
    if (upsample_check_shape("upsample_argmax", B, hp, wp, C, OH, OW)) return -1;
    UpTilePlan pl;
    if (upsample_tile_plan("upsample_argmax", hp, wp, C, OH, OW, &pl)) return -1;
    const int tiles_x = pl.tiles_x, tiles_y = pl.tiles_y, CC = pl.CC, stride = pl.stride, kw_log2 = pl.kw_log2;
    const size_t lds = pl.lds_bytes;
    const unsigned grid = (unsigned)((long long)tiles_x * tiles_y * B);
    if (dense)
        hipLaunchKernelGGL(upsample_argmax_kernel<true>, dim3(grid), dim3(256), lds, s, logp, hp, wp, C, OH, OW, tiles_x, tiles_y, CC, stride,
                           kw_log2, labels, dense);
    else
        hipLaunchKernelGGL(upsample_argmax_kernel<false>, dim3(grid), dim3(256), lds, s, logp, hp, wp, C, OH, OW, tiles_x, tiles_y, CC, stride,
                           kw_log2, labels, dense);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
