// The bilinear upsample's coordinate rule, tile decode, footprint staging, strip walk and pass plan, shared by upsample.hip (argmax /
// dense values), upsample_loss.hip (cross-entropy and its gradient), upsample_ensemble.hip (multi-scale + flip ensemble) and
// windows.hip (sliding-window merge): ONE copy of the integer arithmetic and of the lerp order, so all of them interpolate the same
// values bit for bit.
//
// The family's geometry: one workgroup = one 64 x 32 output tile of one frame, wave w owns the tile's rows 8w .. 8w+7, lane l column
// l.  A tile's source footprint (every cell a pixel of the tile reads, CC classes at a time) is staged in LDS cell-major with an ODD
// stride, so lanes at different x -- different source columns of one class -- fall on different banks for any class count.  Per
// class a lane forms the two horizontally interpolated values of its source row pair once and walks down its 8 pixels with one
// multiply-add each; when the walk enters the next source row (the same row for the whole wave: a scalar branch) the lower value
// moves up and one new one is formed -- 6 LDS reads per class for 8 pixels at an 8x ratio instead of 32.
#pragma once
#include "common.h"

namespace dseg {

constexpr int UP_TW = 64, UP_ROWS = 8, UP_WAVES = 4, UP_TH = UP_ROWS * UP_WAVES;
constexpr int UP_LDS_WORDS = 16384;         // 64 KiB: the footprint of a 64 x 32 tile at an 8x ratio holds 256 classes in one pass
constexpr int UP_LDS_LARGE_WORDS = 40960;   // the CU's whole 160 KiB, for the kernels that stage several footprints side by side

struct UpCoord {
    int i0, i1;
    float lam;
};
// (the host guarantees (2 o + 1) i < 2^31 and o <= 2^22: every integer below is exact in its type)
__host__ __device__ inline void up_index(int d, int i, int o, int* i0, int* i1, unsigned* rem) {
    int num = (2 * d + 1) * i - o;
    if (num < 0) num = 0;
    const unsigned den = 2u * (unsigned)o;
    unsigned q = (unsigned)num / den;
    *rem = (unsigned)num - q * den;
    if ((int)q >= i - 1) {
        q = (unsigned)(i - 1);
        *rem = 0;
    }
    *i0 = (int)q;
    *i1 = (int)q + 1 < i ? (int)q + 1 : i - 1;
}
__device__ inline UpCoord up_coord(int d, int i, int o) {
    UpCoord c;
    unsigned rem;
    up_index(d, i, o, &c.i0, &c.i1, &rem);
    c.lam = __fdiv_rn((float)rem, (float)(2u * (unsigned)o));
    return c;
}

// Classes per staging pass from a word budget: as many as fit (at most C), the odd stride (an even CC takes one more word per
// cell), and kw = 2^kw_log2 lanes per cell.  CC < 1: the cells do not fit.
struct UpPass {
    int CC, stride, kw_log2;
};
__host__ __device__ inline UpPass up_pass_of(int CC) {
    int kw_log2 = 0;
    while (kw_log2 < 6 && (1 << kw_log2) < CC) ++kw_log2;
    return {CC, CC | 1, kw_log2};
}
__host__ __device__ inline UpPass up_pass(int words, int cells, int C) {
    int CC = words / cells;
    if (CC > C) CC = C;
    if ((CC | 1) * cells > words) --CC;
    return up_pass_of(CC);
}

// blockIdx.x -> frame b, the tile's first / last pixel per axis, this lane's column x (xc: clamped to the frame; lanes beyond it
// compute its last column and store nothing), this wave's first row y0, and the first pixel of the lane's strip inside one
// [OH, OW] plane.  wave is the same for every lane, so whatever is indexed by it (the row tables) lives in scalar registers.
struct UpTile {
    int tid, lane, wave, b, x_first, y_first, x_last, y_last, x, xc, y0;
    int active, x_ok;           // 0 / 1 (as int: bool members cost upsample_ensemble_kernel a register)
    size_t plane, pix0;
};
__device__ __forceinline__ UpTile up_tile(int tiles_x, int tiles_y, int OH, int OW) {
    UpTile T;
    T.tid = threadIdx.x;
    T.lane = T.tid & 63;
    T.wave = __builtin_amdgcn_readfirstlane(T.tid >> 6);
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    T.b = t / tiles_y;
    T.x_first = tx * UP_TW;
    T.y_first = ty * UP_TH;
    T.x_last = (T.x_first + UP_TW < OW ? T.x_first + UP_TW : OW) - 1;
    T.y_last = (T.y_first + UP_TH < OH ? T.y_first + UP_TH : OH) - 1;
    T.x = T.x_first + T.lane;
    T.xc = T.x < OW ? T.x : OW - 1;
    T.y0 = T.y_first + T.wave * UP_ROWS;
    T.active = T.y0 < OH;
    T.x_ok = T.x < OW;
    T.plane = (size_t)OH * OW;
    T.pix0 = (size_t)T.y0 * OW + T.x;
    return T;
}

// One grid's footprint under the tile (i0 and i1 are monotonic in the output index) and the lane's strip inside it, as offsets into
// the staged footprint: the lane's two columns and lambda, and per pixel of the strip the two source rows and lambda.  The rows are
// the same for every lane of the wave, so that table lives in scalar registers.
struct UpStrip {
    int fc0, fr0, ncols, ncells, off0, off1;
    float lx;
    int ro0[UP_ROWS], ro1[UP_ROWS];
    float ly[UP_ROWS];
};
__device__ __forceinline__ UpStrip up_strip(const UpTile& T, int hp, int wp, int OH, int OW, int stride) {
    UpStrip S;
    S.fc0 = up_coord(T.x_first, wp, OW).i0;
    S.fr0 = up_coord(T.y_first, hp, OH).i0;
    S.ncols = up_coord(T.x_last, wp, OW).i1 - S.fc0 + 1;
    const int nrows = up_coord(T.y_last, hp, OH).i1 - S.fr0 + 1;
    S.ncells = S.ncols * nrows;
    const UpCoord cx = up_coord(T.xc, wp, OW);
    S.off0 = (cx.i0 - S.fc0) * stride;
    S.off1 = (cx.i1 - S.fc0) * stride;
    S.lx = cx.lam;
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        const int y = T.y0 + j < OH ? T.y0 + j : OH - 1;
        const UpCoord cy = up_coord(y, hp, OH);
        S.ro0[j] = (cy.i0 - S.fr0) * S.ncols * stride;
        S.ro1[j] = (cy.i1 - S.fr0) * S.ncols * stride;
        S.ly[j] = cy.lam;
    }
    return S;
}

// Stage classes c0 .. c0+cn of the ncells = nrows x ncols footprint whose first cell is (fr0, fc0) of frame b's [hp, wp, C] grid:
// kw lanes walk the classes of one cell (contiguous in memory).
__device__ __forceinline__ void up_stage(float* lds, const float* __restrict__ logp, int b, int hp, int wp, int C, int fr0, int fc0,
                                         int ncols, int ncells, int c0, int cn, int stride, int kw_log2) {
    const int tid = threadIdx.x, kw = 1 << kw_log2;
    for (int cell = tid >> kw_log2; cell < ncells; cell += 256 >> kw_log2) {
        const int r = cell / ncols, col = cell - r * ncols;
        const float* g = logp + (((size_t)b * hp + fr0 + r) * wp + fc0 + col) * C + c0;
        float* d = lds + cell * stride;
        for (int k = tid & (kw - 1); k < cn; k += kw) d[k] = g[k];
    }
}

// one source row of one class, interpolated along x at the lane's column
__device__ __forceinline__ float up_hlerp(const float* p, int ro, int off0, int off1, float lx) {
    const float a = p[ro + off0], bb = p[ro + off1];
    return __builtin_fmaf(bb - a, lx, a);
}
// The strip walk of one class (p = the staged footprint + the class): the constructor forms the row pair of the strip's first
// pixel, at() returns the value of the next pixel down.  `enters`: this pixel's upper source row is not the one of the pixel above
// (i0 grows by exactly one when the output is no smaller than the grid: the lower value moves up and row ro1 is formed).  The
// loop over the 8 pixels and what is done with each value stay in the kernel.
struct UpWalk {
    float h0, h1, dh;
    __device__ __forceinline__ UpWalk(const float* p, int ro0, int ro1, int off0, int off1, float lx) {
        h0 = up_hlerp(p, ro0, off0, off1, lx);
        h1 = up_hlerp(p, ro1, off0, off1, lx);
        dh = h1 - h0;
    }
    __device__ __forceinline__ float at(const float* p, bool enters, int ro1, int off0, int off1, float lx, float ly) {
        if (enters) {
            h0 = h1;
            h1 = up_hlerp(p, ro1, off0, off1, lx);
            dh = h1 - h0;
        }
        return __builtin_fmaf(dh, ly, h0);
    }
};

// exp of an argument <= 0 (up to rounding): v_exp_f32 of x log2(e).  The product's rounding moves the result by at most
// |x| e^x 2^-24 <= 2.2e-8 ABSOLUTE (|x| e^x <= 1 / e), the instruction by one ulp of a value <= 1: far inside what the sums carry.
__device__ __forceinline__ float up_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
constexpr float UP_LSE_MX0 = -3.0e38f;      // a running maximum's start (with sum = 0)
// running max-subtracted sum: one exp per class, whichever of (v, max) is the larger
__device__ __forceinline__ void up_lse_update(float& mx, float& sum, float v) {
    const float d = v - mx;
    const float e = up_exp(-__builtin_fabsf(d));
    sum = d > 0.f ? __builtin_fmaf(sum, e, 1.f) : sum + e;
    mx = __builtin_fmaxf(mx, v);
}
// the FIRST maximum over classes visited in ascending order (head_final's tie rule); start from (-INFINITY, 0)
__device__ __forceinline__ void up_first_max(float& best, int& idx, float v, int c) {
    if (v > best) {
        best = v;
        idx = c;
    }
}

// ---- host side (upsample.hip)
// the widest source footprint, along one axis (input i, output o), of any tile of `step` output pixels: the kernels' own index rule
int up_max_footprint(int i, int o, int step);
// Classes per pass for `cells` cells beside `tables` words of tables: inside the default 64 KiB when that leaves at least 8
// classes per pass (or all C), else inside the CU's 160 KiB.  *budget: the data words of the choice made.  CC < 1: they do not fit.
UpPass up_pass_two_budgets(long long tables, long long cells, int C, long long* budget);
// lets both instantiations of a kernel (its <true> and <false>) take the large budget as dynamic LDS, once per device; 0, or -2 and
// a message that names the kernel
int up_allow_large_lds(PerDeviceOnce& once, const char* kernel, const void* with_output, const void* without);

// How a 64 x 32 output tile's source footprint is staged in LDS (upsample.hip): CC classes per pass, cell-major with the odd
// stride, kw = 2^kw_log2 lanes per cell.  -1 (and a message starting with `who`) when a footprint does not fit.
struct UpTilePlan {
    int tiles_x, tiles_y, CC, stride, kw_log2;
    size_t lds_bytes;
};
int upsample_tile_plan(const char* who, int hp, int wp, int C, int OH, int OW, UpTilePlan* plan);

}  // namespace dseg
