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
// One workgroup = one 64 x 32 output tile of one frame; its source footprint (every cell a pixel of the tile reads, CC classes
// at a time) is staged in LDS cell-major with an ODD row stride, so lanes at different x -- different source columns of one
// class -- fall on different banks for any class count.  Wave w owns the tile's rows 8w .. 8w+7, lane l column l: per class a
// lane forms the two horizontally interpolated values of its source row pair once and walks down its 8 pixels with one
// multiply-add each; when the walk enters the next source row (the same row for the whole wave: a scalar branch) the lower
// value moves up and one new one is formed -- 6 LDS reads per class for 8 pixels at an 8x ratio instead of 32.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

template <bool DENSE>
__global__ __launch_bounds__(256) void upsample_argmax_kernel(const float* __restrict__ logp, int hp, int wp, int C, int OH, int OW,
                                                              int tiles_x, int tiles_y, int CC, int stride, int kw_log2,
                                                              int32_t* __restrict__ labels, float* __restrict__ dense) {
    extern __shared__ float up_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int x_first = tx * UP_TW, y_first = ty * UP_TH;
    const int x_last = (x_first + UP_TW < OW ? x_first + UP_TW : OW) - 1, y_last = (y_first + UP_TH < OH ? y_first + UP_TH : OH) - 1;
    // the tile's source footprint: i0 and i1 are monotonic in the output index
    const int fc0 = up_coord(x_first, wp, OW).i0, fr0 = up_coord(y_first, hp, OH).i0;
    const int ncols = up_coord(x_last, wp, OW).i1 - fc0 + 1, nrows = up_coord(y_last, hp, OH).i1 - fr0 + 1;
    const int ncells = ncols * nrows;

    // this lane's column (lanes beyond the frame compute its last column and store nothing)
    const int x = x_first + lane, xc = x < OW ? x : OW - 1;
    const UpCoord cx = up_coord(xc, wp, OW);
    const int off0 = (cx.i0 - fc0) * stride, off1 = (cx.i1 - fc0) * stride;
    const float lx = cx.lam;
    // this wave's rows: the same for every lane, so the table lives in scalar registers
    const int y0 = y_first + wave * UP_ROWS;
    const bool active = y0 < OH;
    int ro0[UP_ROWS], ro1[UP_ROWS];
    float ly[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        const int y = y0 + j < OH ? y0 + j : OH - 1;
        const UpCoord cy = up_coord(y, hp, OH);
        ro0[j] = (cy.i0 - fr0) * ncols * stride;
        ro1[j] = (cy.i1 - fr0) * ncols * stride;
        ly[j] = cy.lam;
    }
    float best[UP_ROWS];
    int idx[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        best[j] = -INFINITY;
        idx[j] = 0;
    }
    const size_t plane = (size_t)OH * OW;
    const size_t pix0 = (size_t)y0 * OW + x;        // first pixel of the lane's strip inside one [OH, OW] plane
    const bool x_ok = x < OW;

    const int kw = 1 << kw_log2;
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cn = C - c0 < CC ? C - c0 : CC;
        if (c0) __syncthreads();
        // stage classes c0 .. c0+cn of the footprint: kw lanes walk the classes of one cell (contiguous in memory)
        for (int cell = tid >> kw_log2; cell < ncells; cell += 256 >> kw_log2) {
            const int r = cell / ncols, col = cell - r * ncols;
            const float* g = logp + (((size_t)b * hp + fr0 + r) * wp + fc0 + col) * C + c0;
            float* d = up_lds + cell * stride;
            for (int k = tid & (kw - 1); k < cn; k += kw) d[k] = g[k];
        }
        __syncthreads();
        if (!active) continue;
        for (int k = 0; k < cn; ++k) {
            const float* p = up_lds + k;
            float a = p[ro0[0] + off0], bb = p[ro0[0] + off1];
            float h0 = __builtin_fmaf(bb - a, lx, a);
            a = p[ro1[0] + off0];
            bb = p[ro1[0] + off1];
            float h1 = __builtin_fmaf(bb - a, lx, a);
            float dh = h1 - h0;
            const int c = c0 + k;
#pragma unroll
            for (int j = 0; j < UP_ROWS; ++j) {
                if (j > 0 && ro0[j] != ro0[j - 1]) {        // the next source row: i0 grows by exactly one when OH >= hp
                    h0 = h1;
                    a = p[ro1[j] + off0];
                    bb = p[ro1[j] + off1];
                    h1 = __builtin_fmaf(bb - a, lx, a);
                    dh = h1 - h0;
                }
                const float v = __builtin_fmaf(dh, ly[j], h0);
                if (DENSE) {
                    if (x_ok && y0 + j < OH) dense[((size_t)b * C + c) * plane + pix0 + (size_t)j * OW] = v;
                }
                if (v > best[j]) {
                    best[j] = v;
                    idx[j] = c;
                }
            }
        }
    }
    if (labels && active && x_ok) {
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

// the tile grid and the LDS staging of a tile's source footprint (upsample_common.h); the shape has passed upsample_check_shape
int upsample_tile_plan(const char* who, int hp, int wp, int C, int OH, int OW, UpTilePlan* plan) {
    const int tiles_x = (OW + UP_TW - 1) / UP_TW, tiles_y = (OH + UP_TH - 1) / UP_TH;
    // the largest source footprint of a tile, with the kernel's own index rule
    int max_cols = 1, max_rows = 1;
    for (int axis = 0; axis < 2; ++axis) {
        const int o = axis ? OH : OW, i = axis ? hp : wp, step = axis ? UP_TH : UP_TW;
        int& widest = axis ? max_rows : max_cols;
        for (int first = 0; first < o; first += step) {
            const int last = (first + step < o ? first + step : o) - 1;
            int a0, a1, b0, b1;
            unsigned rem;
            up_index(first, i, o, &a0, &a1, &rem);
            up_index(last, i, o, &b0, &b1, &rem);
            if (b1 - a0 + 1 > widest) widest = b1 - a0 + 1;
        }
    }
    const int cells = max_cols * max_rows;      // <= 65 * 33
    int CC = UP_LDS_WORDS / cells;
    if (CC > C) CC = C;
    if ((CC | 1) * cells > UP_LDS_WORDS) --CC;  // the stride is odd: an even CC takes one more word per cell
    if (CC < 1) {
        dinoseg_set_error("upsample_argmax: a tile's footprint of %d cells exceeds the LDS budget", cells);
        return -1;
    }
    const int stride = CC | 1;
    int kw_log2 = 0;
    while (kw_log2 < 6 && (1 << kw_log2) < CC) ++kw_log2;
    *plan = {tiles_x, tiles_y, CC, stride, kw_log2, (size_t)cells * stride * sizeof(float)};
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
