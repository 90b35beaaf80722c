// Augmentation of fine-tuning frames and label masks (the reference's get_augmented_transforms(), pl_torch_modules.py:44-57) as a pure
// function of a per-frame parameter table (dinoseg_augment_frame, include/dinoseg.h, where the rule is stated in full): no device
// random numbers, integer coordinates, no atomics -- bit-identical from run to run.
//
// augment_warp_kernel, per output pixel (ox, oy) of frame b:
//     Ux = a0 ox + a1 oy + a2, Uy = a3 ox + a4 oy + a5 in int64 (Q16, edge convention);  V = U - 32768, i0 = V >> 16,
//     l = (V & 0xFFFF) / 65536;  four taps folded by the border rule (reflect-101, or fill[c] per tap), lerp x then y with
//     fmaf(b - a, l, a);  colour: fmaf(gain, v, bias), gray, fmaf(sat, v - gray, gray), clamp to [0, 255];
//     label = mask at (Uy >> 16, Ux >> 16) folded, or void_label;  patch label = the pixel label at (p i, p j).
// With max_radius == 0 it writes the final image; otherwise the fp32 planar scratch [B, 3, OH, OW] (0..255 scale).
//
// augment_blur_kernel: one workgroup = one 64 x 32 output tile of one frame, wave w rows 8w .. 8w+7, lane l column l.  The frame's
// radius r is workgroup-uniform (one table read) and picks one of five fully unrolled bodies, RB = 4, 8, 12, 16, 20 >= r, whose taps
// beyond r carry the weight 0: fmaf(0, v, acc) is acc exactly for finite v, so the sum is the stated one, d = -r .. r in order, while
// the loops have no branches, the weights sit in scalar registers and every LDS offset is an immediate.  Per channel the tile with
// its RB-wide halo -- (32 + 2 RB) x (64 + 2 RB) values, coordinates folded by reflect-101 at the frame's edge while staging -- goes
// to LDS, the horizontal pass writes (32 + 2 RB) x 64 values to a second LDS array, and the vertical pass reads each of its wave's
// 8 + 2 RB rows of those ONCE into eight running sums: no HBM between the passes.  At RB = 20: 72 x 104 + 72 x 64 words =
// 47.25 KiB, three workgroups per CU.  Every LDS access of a wave is one row at 64 consecutive words (ds_read_b32 / ds_write_b32
// are served in 32-lane halves over 32 banks): conflict-free at ANY row stride, so the strides are the plain 64 + 2 RB and 64.  A
// frame with radius 0 is converted straight through from the scratch.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"

namespace dseg {

namespace {

constexpr int AUG_TW = 64, AUG_TH = 32, AUG_ROWS = 8;                  // tile of one workgroup; rows of one wave
constexpr int AUG_MAX_R = 20;                                          // kernel size 41
constexpr int AUG_MAX_SIDE = 16384;
constexpr int AUG_STAGE = (AUG_TH + 2 * AUG_MAX_R) * (AUG_TW + 2 * AUG_MAX_R);   // words of the staged tile + halo
constexpr int AUG_HRES = (AUG_TH + 2 * AUG_MAX_R) * AUG_TW;                      // words of the horizontal pass's result
enum { AUG_OUT_U8 = 0, AUG_OUT_F32 = 1, AUG_OUT_SCRATCH = 2 };

// reflect-101 of any integer onto [0, n): period 2 (n - 1); a side of 1 folds to 0
__device__ __forceinline__ int fold101(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int P = 2 * (n - 1);
    int m = i % P;
    if (m < 0) m += P;
    return m < n ? m : P - m;
}

__device__ __forceinline__ float aug_norm(float v, int c) {
    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
    return __fdiv_rn(__fdiv_rn(v, 255.f) - mean, sd);
}
__device__ __forceinline__ uint8_t aug_u8(float v) { return (uint8_t)rintf(__builtin_amdgcn_fmed3f(v, 0.f, 255.f)); }

// one pixel's three final values to the image in either kind, or raw to the planar scratch
__device__ __forceinline__ void aug_store(int mode, void* out, size_t b, int oy, int ox, int OH, int OW, const float v[3]) {
    const size_t plane = (size_t)OH * OW, pix = (size_t)oy * OW + ox;
    if (mode == AUG_OUT_U8) {
        uint8_t* o = reinterpret_cast<uint8_t*>(out) + (b * plane + pix) * 3;
        o[0] = aug_u8(v[0]);
        o[1] = aug_u8(v[1]);
        o[2] = aug_u8(v[2]);
    } else {
        float* o = reinterpret_cast<float*>(out) + b * 3 * plane + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = mode == AUG_OUT_F32 ? aug_norm(v[c], c) : v[c];
    }
}

// One tile of one frame through both passes at halo RB >= r, three channels into res[c][row of the wave].
template <int RB>
__device__ __forceinline__ void blur_tile(const float* __restrict__ src, size_t plane, const dinoseg_augment_frame& f, int r, int OH, int OW,
                                          int x_first, int y_first, int wave, int lane, float* stage, float* hres,
                                          float (&res)[3][AUG_ROWS]) {
    constexpr int SW = AUG_TW + 2 * RB, SH = AUG_TH + 2 * RB;
    float w[RB + 1];                                                    // workgroup-uniform: scalar registers; 0 beyond r
#pragma unroll
    for (int k = 0; k <= RB; ++k) w[k] = k <= r ? f.w[k] : 0.f;
    for (int c = 0; c < 3; ++c) {
        if (c) __syncthreads();
        // one wave stages one row at a time: consecutive lanes, consecutive columns
        for (int ry = wave; ry < SH; ry += 4) {
            const float* row = src + c * plane + (size_t)fold101(y_first - RB + ry, OH) * OW;
            for (int rx = lane; rx < SW; rx += 64) stage[ry * SW + rx] = row[fold101(x_first - RB + rx, OW)];
        }
        __syncthreads();
        for (int ry = wave; ry < SH; ry += 4) {
            const float* s = stage + ry * SW + lane + RB;
            float acc = 0.f;
#pragma unroll
            for (int d = -RB; d <= RB; ++d) acc = __builtin_fmaf(w[d < 0 ? -d : d], s[d], acc);
            hres[ry * AUG_TW + lane] = acc;
        }
        __syncthreads();
        // output row j of the wave takes the rows i = j .. j + 2 RB of its strip, d = i - j - RB ascending with i
        float acc[AUG_ROWS];
#pragma unroll
        for (int j = 0; j < AUG_ROWS; ++j) acc[j] = 0.f;
        const float* s = hres + wave * AUG_ROWS * AUG_TW + lane;
#pragma unroll
        for (int i = 0; i < AUG_ROWS + 2 * RB; ++i) {
            const float h = s[i * AUG_TW];
#pragma unroll
            for (int j = 0; j < AUG_ROWS; ++j) {
                const int d = i - j - RB;
                if (d >= -RB && d <= RB) acc[j] = __builtin_fmaf(w[d < 0 ? -d : d], h, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < AUG_ROWS; ++j) res[c][j] = acc[j];
    }
}

// block = 64 x 4 output pixels of one frame (blockIdx.x walks tiles_x * tiles_y * B)
__global__ __launch_bounds__(256) void augment_warp_kernel(const uint8_t* __restrict__ frames, const void* __restrict__ masks, int mask_kind,
                                                           int H, int W, const dinoseg_augment_frame* __restrict__ table, int OH, int OW,
                                                           int tiles_x, int tiles_y, int mode, void* __restrict__ out,
                                                           int64_t* __restrict__ pixel_labels, int64_t* __restrict__ patch_labels,
                                                           int patch) {
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int ox = tx * AUG_TW + (threadIdx.x & 63), oy = ty * 4 + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    const dinoseg_augment_frame& f = table[b];
    const bool constant = f.border & 1;
    const long long Ux = (long long)f.a[0] * ox + (long long)f.a[1] * oy + f.a[2];
    const long long Uy = (long long)f.a[3] * ox + (long long)f.a[4] * oy + f.a[5];

    if (masks) {
        const int sx = (int)(Ux >> 16), sy = (int)(Uy >> 16);
        long long label;
        if (constant && ((unsigned)sx >= (unsigned)W || (unsigned)sy >= (unsigned)H)) {
            label = f.void_label;
        } else {
            const size_t at = ((size_t)b * H + fold101(sy, H)) * W + fold101(sx, W);
            label = mask_kind == 0 ? (long long)reinterpret_cast<const uint8_t*>(masks)[at] : reinterpret_cast<const int64_t*>(masks)[at];
        }
        if (pixel_labels) pixel_labels[((size_t)b * OH + oy) * OW + ox] = label;
        if (patch_labels && oy % patch == 0 && ox % patch == 0)
            patch_labels[(size_t)b * (OH / patch) * (OW / patch) + (size_t)(oy / patch) * (OW / patch) + ox / patch] = label;
    }

    const long long Vx = Ux - 32768, Vy = Uy - 32768;
    const int x0 = (int)(Vx >> 16), y0 = (int)(Vy >> 16);
    const float lx = (float)(int)(Vx & 0xFFFF) * (1.f / 65536.f), ly = (float)(int)(Vy & 0xFFFF) * (1.f / 65536.f);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const bool xin0 = (unsigned)x0 < (unsigned)W, xin1 = (unsigned)x1 < (unsigned)W;
    const bool yin0 = (unsigned)y0 < (unsigned)H, yin1 = (unsigned)y1 < (unsigned)H;
    const int fx0 = fold101(x0, W), fx1 = fold101(x1, W), fy0 = fold101(y0, H), fy1 = fold101(y1, H);
    const uint8_t* fr = frames + (size_t)b * H * W * 3;
    const uint8_t* p00 = fr + ((size_t)fy0 * W + fx0) * 3;
    const uint8_t* p01 = fr + ((size_t)fy0 * W + fx1) * 3;
    const uint8_t* p10 = fr + ((size_t)fy1 * W + fx0) * 3;
    const uint8_t* p11 = fr + ((size_t)fy1 * W + fx1) * 3;
    const bool in00 = !constant || (yin0 && xin0), in01 = !constant || (yin0 && xin1);
    const bool in10 = !constant || (yin1 && xin0), in11 = !constant || (yin1 && xin1);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float fill = f.fill[c];
        const float v00 = in00 ? (float)p00[c] : fill, v01 = in01 ? (float)p01[c] : fill;
        const float v10 = in10 ? (float)p10[c] : fill, v11 = in11 ? (float)p11[c] : fill;
        const float top = __builtin_fmaf(v01 - v00, lx, v00), bot = __builtin_fmaf(v11 - v10, lx, v10);
        v[c] = __builtin_fmaf(f.gain, __builtin_fmaf(bot - top, ly, top), f.bias);
    }
    const float gray = __builtin_fmaf(0.114f, v[2], __builtin_fmaf(0.587f, v[1], 0.299f * v[0]));
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __builtin_amdgcn_fmed3f(__builtin_fmaf(f.sat, v[c] - gray, gray), 0.f, 255.f);
    aug_store(mode, out, (size_t)b, oy, ox, OH, OW, v);
}

__global__ __launch_bounds__(256) void augment_blur_kernel(const float* __restrict__ scratch, const dinoseg_augment_frame* __restrict__ table,
                                                           int max_radius, int OH, int OW, int tiles_x, int tiles_y, int mode,
                                                           void* __restrict__ out) {
    __shared__ float lds[AUG_STAGE + AUG_HRES];
    float* stage = lds;
    float* hres = lds + AUG_STAGE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const dinoseg_augment_frame& f = table[b];
    int r = f.radius;
    r = r < 0 ? 0 : r > max_radius ? max_radius : r;
    r = __builtin_amdgcn_readfirstlane(r);
    const int x_first = tx * AUG_TW, y_first = ty * AUG_TH;
    const int x = x_first + lane, y0 = y_first + wave * AUG_ROWS;
    const size_t plane = (size_t)OH * OW;
    const float* src = scratch + (size_t)b * 3 * plane;
    float res[3][AUG_ROWS];

    if (r == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < AUG_ROWS; ++j) res[c][j] = (x < OW && y0 + j < OH) ? src[c * plane + (size_t)(y0 + j) * OW + x] : 0.f;
    } else {
        if (r <= 4) blur_tile<4>(src, plane, f, r, OH, OW, x_first, y_first, wave, lane, stage, hres, res);
        else if (r <= 8) blur_tile<8>(src, plane, f, r, OH, OW, x_first, y_first, wave, lane, stage, hres, res);
        else if (r <= 12) blur_tile<12>(src, plane, f, r, OH, OW, x_first, y_first, wave, lane, stage, hres, res);
        else if (r <= 16) blur_tile<16>(src, plane, f, r, OH, OW, x_first, y_first, wave, lane, stage, hres, res);
        else blur_tile<20>(src, plane, f, r, OH, OW, x_first, y_first, wave, lane, stage, hres, res);
    }
    if (x >= OW) return;
#pragma unroll
    for (int j = 0; j < AUG_ROWS; ++j) {
        if (y0 + j >= OH) break;
        const float v[3] = {res[0][j], res[1][j], res[2][j]};
        aug_store(mode, out, (size_t)b, y0 + j, x, OH, OW, v);
    }
}

}  // namespace

int launch_augment(const uint8_t* frames, const void* masks, int mask_kind, int B, int H, int W, const dinoseg_augment_frame* table,
                   int max_radius, int OH, int OW, int out_kind, void* out, int64_t* pixel_labels, int64_t* patch_labels, int patch,
                   float* scratch, hipStream_t s) {
    const char* who = "augment";
    if (!frames || !table || !out) {
        dinoseg_set_error("%s: null pointer (%s)", who, !frames ? "frames" : !table ? "table" : "out");
        return -1;
    }
    if (mask_kind != 0 && mask_kind != 1) {
        dinoseg_set_error("%s: mask kind %d (0 = uint8, 1 = int64)", who, mask_kind);
        return -1;
    }
    if (out_kind != DINOSEG_INPUT_U8_HWC && out_kind != DINOSEG_INPUT_F32_CHW) {
        dinoseg_set_error("%s: output kind %d (0 = uint8 [B,OH,OW,3], 1 = fp32 [B,3,OH,OW])", who, out_kind);
        return -1;
    }
    if (B < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) {
        dinoseg_set_error("%s: bad argument (B=%d, source %d x %d, output %d x %d; sizes must be positive)", who, B, H, W, OH, OW);
        return -1;
    }
    if (H > AUG_MAX_SIDE || W > AUG_MAX_SIDE || OH > AUG_MAX_SIDE || OW > AUG_MAX_SIDE) {
        dinoseg_set_error("%s: source %d x %d, output %d x %d: a side is above %d", who, H, W, OH, OW, AUG_MAX_SIDE);
        return -1;
    }
    if (max_radius < 0 || max_radius > AUG_MAX_R) {
        dinoseg_set_error("%s: max_radius %d (0 <= max_radius <= %d)", who, max_radius, AUG_MAX_R);
        return -1;
    }
    if (OH <= max_radius || OW <= max_radius) {
        dinoseg_set_error("%s: output %d x %d does not exceed max_radius %d (the blur folds its halo once)", who, OH, OW, max_radius);
        return -1;
    }
    if (!masks && (pixel_labels || patch_labels)) {
        dinoseg_set_error("%s: a label output without masks", who);
        return -1;
    }
    if (patch_labels && ((patch != 8 && patch != 16) || OH % patch != 0 || OW % patch != 0)) {
        if (patch != 8 && patch != 16) dinoseg_set_error("%s: patch %d (8 or 16)", who, patch);
        else dinoseg_set_error("%s: output %d x %d is not a multiple of the patch (%d)", who, OH, OW, patch);
        return -1;
    }
    if (max_radius > 0 && !scratch) {
        dinoseg_set_error("%s: null pointer (scratch is required when max_radius > 0)", who);
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0) {
        dinoseg_set_error("%s: the destination is not 16-byte aligned", who);
        return -1;
    }
    const int tiles_x = (OW + AUG_TW - 1) / AUG_TW;
    const long long warp_blocks = (long long)B * tiles_x * ((OH + 3) / 4);
    if (warp_blocks > 0x7fffffffll) {
        dinoseg_set_error("%s: %d frames of %d x %d are too many", who, B, OH, OW);
        return -1;
    }
    const int mode = out_kind == DINOSEG_INPUT_U8_HWC ? AUG_OUT_U8 : AUG_OUT_F32;
    hipLaunchKernelGGL(augment_warp_kernel, dim3((unsigned)warp_blocks), dim3(256), 0, s, frames, masks, mask_kind, H, W, table, OH, OW,
                       tiles_x, (OH + 3) / 4, max_radius > 0 ? (int)AUG_OUT_SCRATCH : mode, max_radius > 0 ? (void*)scratch : out,
                       pixel_labels, patch_labels, patch);
    DSEG_CHECK_HIP(hipGetLastError());
    if (max_radius > 0) {
        const int tiles_y = (OH + AUG_TH - 1) / AUG_TH;
        hipLaunchKernelGGL(augment_blur_kernel, dim3((unsigned)((long long)B * tiles_x * tiles_y)), dim3(256), 0, s, scratch, table,
                           max_radius, OH, OW, tiles_x, tiles_y, mode, out);
        DSEG_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace dseg
