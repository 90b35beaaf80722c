// The bilinear upsample's coordinate rule and tile plan, shared by upsample.hip (argmax / dense values), upsample_loss.hip
// (cross-entropy and its gradient) and upsample_ensemble.hip (multi-scale + flip ensemble): ONE copy of the integer arithmetic, so
// all of them interpolate the same values bit for bit.
#pragma once
#include "common.h"

namespace dseg {

constexpr int UP_TW = 64, UP_ROWS = 8, UP_WAVES = 4, UP_TH = UP_ROWS * UP_WAVES;
constexpr int UP_LDS_WORDS = 16384;         // 64 KiB: the footprint of a 64 x 32 tile at an 8x ratio holds 256 classes in one pass

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

// How a 64 x 32 output tile's source footprint is staged in LDS (upsample.hip): CC classes per pass, cell-major with the odd
// stride, kw = 2^kw_log2 lanes per cell.  -1 (and a message starting with `who`) when a footprint does not fit.
struct UpTilePlan {
    int tiles_x, tiles_y, CC, stride, kw_log2;
    size_t lds_bytes;
};
int upsample_tile_plan(const char* who, int hp, int wp, int C, int OH, int OW, UpTilePlan* plan);

}  // namespace dseg
