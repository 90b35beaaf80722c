// Pixel-resolution training loss: cross-entropy of the bilinearly upsampled log-probs against pixel labels, and its gradient with
// respect to the LOW-RES log-probs, without any [B, C, OH, OW] tensor.
//
//     U[b,c,y,x] = bilinear upsample of L[b, hp*wp, C] to OH x OW (upsample_common.h: the coordinates and the lerp order of upsample.hip)
//     lse[b,y,x] = log sum_c exp(U)                       (a convex combination of log-probs is not normalised)
//     loss       = (1/n) sum over valid pixels of lse - U[b,t,y,x]                      n = number of valid pixels of the batch
//     dL[b,p,c]  = (1/n) sum over valid pixels of w(p; y,x) (exp(U[b,c,y,x] - lse) - [c == t])       (transpose of the bilinear map)
// A pixel is valid when 0 <= t < C; ignore_index and -100 are skipped silently, any other label is skipped and latches flags[0].
//
// Two passes, both stream-ordered:
//   upnll_lse_kernel   one workgroup per 64 x 32 output tile, the footprint staged exactly as upsample_argmax_kernel stages it; every
//                      lane carries a running (max, sum) pair per pixel over the classes, writes lse (4 bytes per pixel, the only
//                      per-pixel storage) and the tile's loss sum and valid count go to two accumulators -- fp32 atomics, or under
//                      option deterministic one partial pair per tile added in tile order by launch_det_finalize.
//   upnll_grad_kernel  a GATHER: one workgroup per low-res cell.  The pixels that read cell (r, c) have i0 in {r-1, r} x {c-1, c}:
//                      four rectangles, inside each of which the four corner cells of every pixel are the same, so a thread (class k,
//                      pixel slot) holds its class's 3 x 3 cells in registers, recomputes U_k with the forward's own multiply-adds
//                      from the staged lambda / label / lse tables, and adds w (p - onehot) in a fixed pixel order.  The pixel slots of a class
//                      are then added in slot order.  No floating-point atomic anywhere: dL is bit-identical run to run.  Every exp
//                      is computed about four times (once per corner cell).  1/n is read from the device accumulator.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

namespace {

constexpr int UPNLL_IGNORE = -100;          // F.cross_entropy's default ignore_index: always skipped, beside the caller's own
constexpr int UPNLL_ACC_BYTES = 256;        // scratch: [0, 256) the accumulators {loss sum, valid pixels}, then lse, then the tile partials
constexpr int GQ = 32;                      // the gather stages a quadrant in chunks of at most GQ x GQ pixels

__device__ __forceinline__ void upnll_finish(const float* acc, float* loss, float* n_valid) {
    const float n = acc[1];
    *loss = n > 0.f ? acc[0] / n : __builtin_nanf("");      // torch: the mean over zero pixels is nan
    if (n_valid) *n_valid = n;
}

__global__ __launch_bounds__(256) void upnll_lse_kernel(const float* __restrict__ logp, int hp, int wp, int C, int OH, int OW, int tiles_x,
                                                        int tiles_y, int CC, int stride, int kw_log2, const int64_t* __restrict__ labels,
                                                        int ignore_index, float* __restrict__ lse_out, float* __restrict__ acc,
                                                        int* __restrict__ flags, float* __restrict__ det) {
    extern __shared__ float up_lds[];
    const UpTile T = up_tile(tiles_x, tiles_y, OH, OW);
    const int tid = T.tid, lane = T.lane, wave = T.wave, b = T.b, y0 = T.y0;
    const bool active = T.active, x_ok = T.x_ok;
    const UpStrip S = up_strip(T, hp, wp, OH, OW, stride);
    const size_t pix0 = (size_t)b * T.plane + T.pix0;
    // this lane's labels: -1 = not a valid pixel (outside the frame, ignored, or out of range)
    int tl[UP_ROWS];
    float mx[UP_ROWS], sum[UP_ROWS], ut[UP_ROWS];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        tl[j] = -1;
        mx[j] = UP_LSE_MX0;
        sum[j] = 0.f;
        ut[j] = 0.f;
        if (active && x_ok && y0 + j < OH) {
            const long long yy = labels[pix0 + (size_t)j * OW];
            if (yy >= 0 && yy < C)
                tl[j] = (int)yy;
            else if (yy != ignore_index && yy != UPNLL_IGNORE)
                bad = true;
        }
    }
    if (bad && flags) atomicOr(flags, 1);

    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cn = C - c0 < CC ? C - c0 : CC;
        if (c0) __syncthreads();
        up_stage(up_lds, logp, b, hp, wp, C, S.fr0, S.fc0, S.ncols, S.ncells, c0, cn, stride, kw_log2);
        __syncthreads();
        if (!active) continue;
        for (int k = 0; k < cn; ++k) {
            const float* p = up_lds + k;
            UpWalk w(p, S.ro0[0], S.ro1[0], S.off0, S.off1, S.lx);
            const int c = c0 + k;
#pragma unroll
            for (int j = 0; j < UP_ROWS; ++j) {
                const float v = w.at(p, j > 0 && S.ro0[j] != S.ro0[j - 1], S.ro1[j], S.off0, S.off1, S.lx, S.ly[j]);
                up_lse_update(mx[j], sum[j], v);
                if (c == tl[j]) ut[j] = v;
            }
        }
    }
    float l = 0.f, n = 0.f;
    if (active && x_ok) {
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j) {
            if (y0 + j < OH) {
                const float lse = mx[j] + logf(sum[j]);
                lse_out[pix0 + (size_t)j * OW] = lse;
                if (tl[j] >= 0) {
                    l += lse - ut[j];
                    n += 1.f;
                }
            }
        }
    }
    l = wave_sum(l);
    n = wave_sum(n);
    if (det) {          // deterministic mode: the tile's four wave sums in wave order, one partial pair per tile
        __syncthreads();        // (every wave has left the staged footprint: its first words now hold the wave sums)
        if (lane == 0) {
            up_lds[wave] = l;
            up_lds[4 + wave] = n;
        }
        __syncthreads();
        if (tid < 2) det[(size_t)blockIdx.x * 2 + tid] = ((up_lds[4 * tid] + up_lds[4 * tid + 1]) + up_lds[4 * tid + 2]) + up_lds[4 * tid + 3];
        return;
    }
    if (lane == 0 && n != 0.f) {
        atomicAdd(acc, l);
        atomicAdd(acc + 1, n);
    }
}

__global__ void upnll_finish_kernel(const float* __restrict__ acc, float* __restrict__ loss, float* __restrict__ n_valid) {
    upnll_finish(acc, loss, n_valid);
}

// the first output index whose i0 is at least `cell` (i0 is monotonic and, with o >= i, takes every value 0 .. i-1); o for cell >= i.
// The closed form is only a starting point: up_index itself decides.
__device__ inline int upnll_first(int cell, int i, int o) {
    if (cell <= 0) return 0;
    if (cell >= i) return o;
    int g = (int)(((2u * (unsigned)cell + 1u) * (unsigned)o + (unsigned)i - 1u) / (2u * (unsigned)i));     // (< (2 o + 1) i < 2^31)
    g = g < 0 ? 0 : g > o ? o : g;
    int i0, i1;
    unsigned rem;
    while (g > 0) {
        up_index(g - 1, i, o, &i0, &i1, &rem);
        if (i0 < cell) break;
        --g;
    }
    while (g < o) {
        up_index(g, i, o, &i0, &i1, &rem);
        if (i0 >= cell) break;
        ++g;
    }
    return g;
}

// One workgroup per (frame, low-res cell) and per KL = 2^kl_log2 <= 64 classes (blockIdx.y).  Thread = (class lane kl of KL, pixel
// slot ps of 256 / KL).
__global__ __launch_bounds__(256) void upnll_grad_kernel(const float* __restrict__ logp, int hp, int wp, int C, int OH, int OW, int kl_log2,
                                                         const int64_t* __restrict__ labels, const float* __restrict__ lse,
                                                         const float* __restrict__ acc, float* __restrict__ dlogp,
                                                         float* __restrict__ loss, float* __restrict__ n_valid) {
    __shared__ float q_lse[GQ * GQ];
    __shared__ int q_t[GQ * GQ];
    __shared__ float q_lx[GQ], q_ly[GQ];
    __shared__ float red[256];
    __shared__ int q_bnd[6];
    const int tid = threadIdx.x;
    const int KL = 1 << kl_log2, NPS = 256 >> kl_log2;
    const int kl = tid & (KL - 1), ps = tid >> kl_log2;
    int cell = blockIdx.x;
    const int b = cell / (hp * wp);
    cell -= b * hp * wp;
    const int r = cell / wp, c = cell - r * wp;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0 && loss) upnll_finish(acc, loss, n_valid);
    const float nv = acc[1];
    const float inv_n = nv > 0.f ? 1.0f / nv : 0.f;

    // rows / columns whose i0 is r-1 (this cell is their i1: weight lambda) and whose i0 is r (weight 1 - lambda): six bounds, one
    // thread each
    if (tid < 6) {
        const int ax = tid / 3, d = tid - 3 * ax - 1;
        q_bnd[tid] = ax ? upnll_first(c + d, wp, OW) : upnll_first(r + d, hp, OH);
    }
    const size_t plane = (size_t)OH * OW;
    const float* Lb = logp + (size_t)b * hp * wp * C;
    const int k = blockIdx.y * KL + kl;
    const int kk = k < C ? k : C - 1;       // (lanes beyond C compute the last class and store nothing)
    // this class's 3 x 3 neighbourhood of the cell (clamped as the forward clamps i1; a clamped row or column only ever meets lambda = 0)
    float nb[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int rr = r + dy - 1 < 0 ? 0 : r + dy - 1 > hp - 1 ? hp - 1 : r + dy - 1;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int cc = c + dx - 1 < 0 ? 0 : c + dx - 1 > wp - 1 ? wp - 1 : c + dx - 1;
            nb[dy][dx] = Lb[((size_t)rr * wp + cc) * C + kk];
        }
    }
    __syncthreads();
    const int ys[3] = {q_bnd[0], q_bnd[1], q_bnd[2]}, xs[3] = {q_bnd[3], q_bnd[4], q_bnd[5]};
    float sacc = 0.f;

    // the cell's whole support, staged in chunks of at most GQ x GQ pixels; inside a chunk the four rectangles one after another
    for (int yc = ys[0]; yc < ys[2]; yc += GQ) {
        const int ch = ys[2] - yc < GQ ? ys[2] - yc : GQ;
        for (int xc = xs[0]; xc < xs[2]; xc += GQ) {
            const int cw = xs[2] - xc < GQ ? xs[2] - xc : GQ;
            const int npix = ch * cw;
            __syncthreads();
            if (tid < cw) q_lx[tid] = up_coord(xc + tid, wp, OW).lam;
            if (tid >= 64 && tid < 64 + ch) q_ly[tid - 64] = up_coord(yc + tid - 64, hp, OH).lam;
            for (int i = tid; i < npix; i += 256) {
                const int yy = i / cw, xx = i - yy * cw;
                const size_t pix = (size_t)b * plane + (size_t)(yc + yy) * OW + xc + xx;
                const long long lab = labels[pix];
                const bool ok = lab >= 0 && lab < C;
                q_t[i] = ok ? (int)lab : -1;
                q_lse[i] = ok ? lse[pix] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int qy = 0; qy < 2; ++qy) {
                const int ya = (ys[qy] > yc ? ys[qy] : yc) - yc, yb = (ys[qy + 1] < yc + ch ? ys[qy + 1] : yc + ch) - yc;
#pragma unroll
                for (int qx = 0; qx < 2; ++qx) {
                    const int xa = (xs[qx] > xc ? xs[qx] : xc) - xc, xb = (xs[qx + 1] < xc + cw ? xs[qx + 1] : xc + cw) - xc;
                    if (ya >= yb || xa >= xb) continue;
                    const int qw = xb - xa, qn = (yb - ya) * qw;
                    const float a = nb[qy][qx], a2 = nb[qy + 1][qx];
                    const float d0 = nb[qy][qx + 1] - a, d1 = nb[qy + 1][qx + 1] - a2;
                    const int step_y = NPS / qw, step_x = NPS - step_y * qw;
                    int yy = ps / qw, xx = ps - yy * qw;
                    for (int i = ps; i < qn; i += NPS) {
                        const int ti = (ya + yy) * cw + xa + xx;
                        const int tt = q_t[ti];
                        if (tt >= 0) {
                            const float lx = q_lx[xa + xx], ly = q_ly[ya + yy];
                            const float h0 = __builtin_fmaf(d0, lx, a), h1 = __builtin_fmaf(d1, lx, a2);
                            const float v = __builtin_fmaf(h1 - h0, ly, h0);
                            const float g = up_exp(v - q_lse[ti]) - (tt == k ? 1.f : 0.f);
                            const float w = (qx ? 1.f - lx : lx) * (qy ? 1.f - ly : ly);
                            sacc = __builtin_fmaf(w, g, sacc);
                        }
                        xx += step_x;
                        yy += step_y;
                        if (xx >= qw) {
                            xx -= qw;
                            ++yy;
                        }
                    }
                }
            }
        }
    }
    // the pixel slots of a class, added in slot order
    red[tid] = sacc;
    __syncthreads();
    if (ps == 0 && k < C) {
        float s = red[kl];
        for (int j = 1; j < NPS; ++j) s += red[(j << kl_log2) + kl];
        dlogp[((size_t)b * hp * wp + cell) * C + k] = s * inv_n;
    }
}

}  // namespace

// scratch: the accumulators, one fp32 lse per pixel, one partial pair per tile (option deterministic); <= 8 bytes per pixel + 64 KiB
// (a tile has at least one pixel; only B > 8000 frames of a single pixel would pass that)
static void upnll_layout(int B, int OH, int OW, size_t* lse_off, size_t* det_off, size_t* total) {
    const size_t pix = (size_t)B * OH * OW, tiles = (size_t)B * ((OW + UP_TW - 1) / UP_TW) * ((OH + UP_TH - 1) / UP_TH);
    *lse_off = UPNLL_ACC_BYTES;
    *det_off = *lse_off + (pix * 4 + 255) / 256 * 256;
    *total = *det_off + (tiles * 8 + 255) / 256 * 256;
}

long long upsample_nll_scratch_bytes(int B, int hp, int wp, int C, int OH, int OW) {
    if (upsample_check_shape("upsample_nll_scratch_bytes", B, hp, wp, C, OH, OW)) return -1;
    size_t lse_off, det_off, total;
    upnll_layout(B, OH, OW, &lse_off, &det_off, &total);
    return (long long)total;
}

int upsample_nll_check(const char* who, int B, int hp, int wp, int C, int OH, int OW, int ignore_index) {
    if (upsample_check_shape(who, B, hp, wp, C, OH, OW)) return -1;
    if (ignore_index >= 0 && ignore_index < C) {
        dinoseg_set_error("%s: ignore_index %d is a class (0 <= ignore_index < C = %d); use a value outside the classes, e.g. 255 or -100", who,
                          ignore_index, C);
        return -1;
    }
    if ((long long)B * hp * wp > 0x7fffffffll) {
        dinoseg_set_error("%s: input grid %dx%d (B=%d) is too large", who, hp, wp, B);
        return -1;
    }
    return 0;
}

int launch_upsample_nll(const float* logp, int B, int hp, int wp, int C, int OH, int OW, const int64_t* labels, int ignore_index,
                        float* loss, float* dlogp, float* n_valid, int* flags, void* scratch, hipStream_t s) {
    if (!logp || !labels || !loss || !scratch) {
        dinoseg_set_error("upsample_nll: null pointer (logp, labels, loss_out and scratch are required)");
        return -1;
    }
    if (upsample_nll_check("upsample_nll", B, hp, wp, C, OH, OW, ignore_index)) return -1;
    UpTilePlan pl;
    if (upsample_tile_plan("upsample_nll", hp, wp, C, OH, OW, &pl)) return -1;
    size_t lse_off, det_off, total;
    upnll_layout(B, OH, OW, &lse_off, &det_off, &total);
    char* base = static_cast<char*>(scratch);
    float* acc = reinterpret_cast<float*>(base);
    float* lse = reinterpret_cast<float*>(base + lse_off);
    float* det = options().deterministic ? reinterpret_cast<float*>(base + det_off) : nullptr;
    const unsigned tiles = (unsigned)((long long)pl.tiles_x * pl.tiles_y * B);
    DSEG_CHECK_HIP(hipMemsetAsync(acc, 0, 2 * sizeof(float), s));
    const size_t lds = pl.lds_bytes < 32 ? 32 : pl.lds_bytes;       // (the tile's wave sums reuse the first 8 words)
    hipLaunchKernelGGL(upnll_lse_kernel, dim3(tiles), dim3(256), lds, s, logp, hp, wp, C, OH, OW, pl.tiles_x, pl.tiles_y, pl.CC,
                       pl.stride, pl.kw_log2, labels, ignore_index, lse, acc, flags, det);
    DSEG_CHECK_HIP(hipGetLastError());
    if (det) {
        const int rc = launch_det_finalize(det, (int)tiles, 2, 2, acc, s);
        if (rc) return rc;
    }
    if (!dlogp) {
        hipLaunchKernelGGL(upnll_finish_kernel, dim3(1), dim3(1), 0, s, acc, loss, n_valid);
        DSEG_CHECK_HIP(hipGetLastError());
        return 0;
    }
    int kl_log2 = 0;
    while (kl_log2 < 6 && (1 << kl_log2) < C) ++kl_log2;
    hipLaunchKernelGGL(upnll_grad_kernel, dim3((unsigned)(B * hp * wp), (unsigned)((C + (1 << kl_log2) - 1) >> kl_log2)), dim3(256), 0, s, logp, hp, wp, C, OH, OW, kl_log2, labels, lse, acc,
                       dlogp, loss, n_valid);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
