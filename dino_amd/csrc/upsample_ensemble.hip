// Multi-scale + flip ensemble at pixel resolution: K low-res log-prob grids (one per view of the frame: several scales, each
// optionally mirrored) -> per pixel the mean over views of the softmax of each view's bilinearly upsampled scores, its first-maximum
// label and its confidence, in ONE launch and without any [B, C, OH, OW] transient (unless the probabilities themselves are asked for).
//
//     v_k[c]   = bilinear value of view k at the pixel: up_coord and the two chained fmaf lerps of upsample.hip, x first, then y.
//                flip_k == 1 mirrors the view's grid horizontally first: the taps are columns wp_k-1-i0 and wp_k-1-i1, in that
//                order, with the same lambda ("flip the low-res grid back, then upsample").
//     lse_k    = m_k + logf(sum_c exp(v_k[c] - m_k)),  m_k = max_c v_k[c]       (a running maximum: one exp per class)
//     p_k[c]   = exp(v_k[c] - lse_k)                    (the softmax of the interpolated scores: mmseg's protocol; exp = up_exp)
//     s[c]     = p_0[c] + p_1[c] + ... in view order, fp32;   probs[c] = s[c] / K
//     label    = the FIRST maximum of s over classes;   conf = max_c s[c] / K
// No atomics: bit-identical from run to run.
//
// One workgroup = one 64 x 32 output tile of one frame: the tile, the staging and the strip walk of upsample_common.h.  Two phases
// inside the launch:
//   A  per view: the view's footprint is staged in LDS (as many classes per pass as fit), every lane carries a running (max, sum)
//      per pixel and leaves the 8 log-sum-exps of its strip in the caller's scratch ([K, B, OH, OW] fp32; each lane reads back
//      only what it wrote itself).
//   B  per class chunk: the footprints of ALL views are staged side by side; four classes at a time a lane walks the views (view
//      parameters and the 8 LSEs are fetched once per four classes), adds exp(v - lse) into s[4][8], and keeps the running first
//      maximum.  4 (+4, +4 C) bytes per pixel are written.
// The per-view coordinates (footprint origin, the lane's two columns and lambda, the rows' two source rows and lambda, whether a row
// enters a new source row) are worked out once per workgroup into LDS tables: 392 words per view.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

namespace {

constexpr int UPE_VT = 8, UPE_XT = 4 * UP_TW, UPE_RT = 4 * UP_TH;     // table words per view: footprint, columns, rows
constexpr int UPE_TABLE_WORDS = UPE_VT + UPE_XT + UPE_RT;
constexpr int UPE_CR = 4;                                              // classes per walk over the views in phase B

struct UpEnsPlan {
    int tiles_x, tiles_y, CCB, data_words;
    size_t lds_bytes;
};

template <bool PROBS>
__global__ __launch_bounds__(256) void upsample_ensemble_kernel(UpEnsViews views, int K, int B, int C, int OH, int OW, int tiles_x,
                                                                int tiles_y, int CCB, int data_words, int32_t* __restrict__ labels,
                                                                float* __restrict__ conf, float* __restrict__ probs, float* lse_buf) {
    extern __shared__ float upe_lds[];
    int* vt = reinterpret_cast<int*>(upe_lds);      // [K][8]: fc0, fr0, ncols, ncells, first cell of the view in phase B
    int* xt = vt + K * UPE_VT;                      // [K][64][4]: the lane's two footprint columns, lambda
    int* rt = xt + K * UPE_XT;                      // [K][32][4]: the row's two footprint rows (in cells), lambda, enters-a-new-row
    float* data = reinterpret_cast<float*>(rt + K * UPE_RT);
    const UpTile T = up_tile(tiles_x, tiles_y, OH, OW);
    const int tid = T.tid, lane = T.lane, wave = T.wave, b = T.b, y0 = T.y0;
    const int x_first = T.x_first, y_first = T.y_first, x_last = T.x_last, y_last = T.y_last, xc = T.xc;
    const bool active = T.active, x_ok = T.x_ok;
    const size_t plane = T.plane, pix0 = T.pix0;

    // the coordinate tables: wave w fills views w, w+4, ...
    for (int k = wave; k < K; k += UP_WAVES) {
        const int hp = views.v[k].hp, wp = views.v[k].wp, flip = views.v[k].flip;
        const UpCoord xf = up_coord(x_first, wp, OW), xl = up_coord(x_last, wp, OW);
        const int fc0 = flip ? wp - 1 - xl.i1 : xf.i0, ncols = xl.i1 - xf.i0 + 1;
        const int fr0 = up_coord(y_first, hp, OH).i0, nrows = up_coord(y_last, hp, OH).i1 - fr0 + 1;
        if (lane == 0) {
            vt[k * UPE_VT + 0] = fc0;
            vt[k * UPE_VT + 1] = fr0;
            vt[k * UPE_VT + 2] = ncols;
            vt[k * UPE_VT + 3] = ncols * nrows;
        }
        const UpCoord cx = up_coord(xc, wp, OW);
        int* xe = xt + (k * UP_TW + lane) * 4;
        xe[0] = (flip ? wp - 1 - cx.i0 : cx.i0) - fc0;
        xe[1] = (flip ? wp - 1 - cx.i1 : cx.i1) - fc0;
        xe[2] = __float_as_int(cx.lam);
        xe[3] = 0;
        if (lane < UP_TH) {
            const int y = y_first + lane < OH ? y_first + lane : OH - 1;
            const UpCoord cy = up_coord(y, hp, OH);
            int adv = 0;
            if (lane & (UP_ROWS - 1)) {
                const int yp = y_first + lane - 1 < OH ? y_first + lane - 1 : OH - 1;
                adv = up_coord(yp, hp, OH).i0 != cy.i0;
            }
            int* re = rt + (k * UP_TH + lane) * 4;
            re[0] = (cy.i0 - fr0) * ncols;
            re[1] = (cy.i1 - fr0) * ncols;
            re[2] = __float_as_int(cy.lam);
            re[3] = adv;
        }
    }
    __syncthreads();
    if (tid == 0) {                                 // (read in phase B, many barriers from here)
        int base = 0;
        for (int k = 0; k < K; ++k) {
            vt[k * UPE_VT + 4] = base;
            base += vt[k * UPE_VT + 3];
        }
    }

    // ---- phase A: the log-sum-exp of every view at every pixel of the tile
    for (int k = 0; k < K; ++k) {
        const float* __restrict__ logp = views.v[k].logp;
        const int hp = views.v[k].hp, wp = views.v[k].wp;
        const int fc0 = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 0]), fr0 = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 1]);
        const int ncols = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 2]), ncells = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 3]);
        const UpPass ps = up_pass(data_words, ncells, C);
        const int CC = ps.CC, stride = ps.stride;

        const int* xe = xt + (k * UP_TW + lane) * 4;
        const int off0 = xe[0] * stride, off1 = xe[1] * stride;
        const float lx = __int_as_float(xe[2]);
        int ro0[UP_ROWS], ro1[UP_ROWS], adv[UP_ROWS];
        float ly[UP_ROWS], mx[UP_ROWS], sum[UP_ROWS];
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j) {
            const int* re = rt + (k * UP_TH + wave * UP_ROWS + j) * 4;
            ro0[j] = __builtin_amdgcn_readfirstlane(re[0]) * stride;
            ro1[j] = __builtin_amdgcn_readfirstlane(re[1]) * stride;
            ly[j] = __int_as_float(__builtin_amdgcn_readfirstlane(re[2]));
            adv[j] = __builtin_amdgcn_readfirstlane(re[3]);
            mx[j] = UP_LSE_MX0;
            sum[j] = 0.f;
        }
        for (int c0 = 0; c0 < C; c0 += CC) {
            const int cn = C - c0 < CC ? C - c0 : CC;
            __syncthreads();
            up_stage(data, logp, b, hp, wp, C, fr0, fc0, ncols, ncells, c0, cn, stride, ps.kw_log2);
            __syncthreads();
            if (!active) continue;
            for (int q = 0; q < cn; ++q) {
                const float* p = data + q;
                UpWalk w(p, ro0[0], ro1[0], off0, off1, lx);
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) up_lse_update(mx[j], sum[j], w.at(p, adv[j], ro1[j], off0, off1, lx, ly[j]));
            }
        }
        if (active && x_ok) {
            float* out = lse_buf + ((size_t)k * B + b) * plane + pix0;
#pragma unroll
            for (int j = 0; j < UP_ROWS; ++j)
                if (y0 + j < OH) out[(size_t)j * OW] = mx[j] + logf(sum[j]);
        }
    }

    // ---- phase B: the sum over views of exp(v - lse), class by class, and its first maximum
    float best[UP_ROWS];
    int idx[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        best[j] = -INFINITY;
        idx[j] = 0;
    }
    const float Kf = (float)K;
    const int stride = up_pass_of(CCB).stride, kw_log2 = up_pass_of(CCB).kw_log2;
    for (int c0 = 0; c0 < C; c0 += CCB) {
        const int cn = C - c0 < CCB ? C - c0 : CCB;
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const float* __restrict__ logp = views.v[k].logp;
            const int hp = views.v[k].hp, wp = views.v[k].wp;
            const int fc0 = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 0]), fr0 = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 1]);
            const int ncols = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 2]), ncells = __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 3]);
            float* vd = data + __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 4]) * stride;
            up_stage(vd, logp, b, hp, wp, C, fr0, fc0, ncols, ncells, c0, cn, stride, kw_log2);
        }
        __syncthreads();
        if (!active) continue;
        for (int q0 = 0; q0 < cn; q0 += UPE_CR) {
            const int qn = cn - q0 < UPE_CR ? cn - q0 : UPE_CR;
            float s[UPE_CR][UP_ROWS];
#pragma unroll
            for (int q = 0; q < UPE_CR; ++q)
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) s[q][j] = 0.f;
            for (int k = 0; k < K; ++k) {
                const float* vd = data + __builtin_amdgcn_readfirstlane(vt[k * UPE_VT + 4]) * stride + q0;
                const int* xe = xt + (k * UP_TW + lane) * 4;
                const int off0 = xe[0] * stride, off1 = xe[1] * stride;
                const float lx = __int_as_float(xe[2]);
                const float* lse_in = lse_buf + ((size_t)k * B + b) * plane + pix0;
                int ro0, ro1[UP_ROWS], adv[UP_ROWS];
                float ly[UP_ROWS], lse[UP_ROWS];
                ro0 = __builtin_amdgcn_readfirstlane(rt[(k * UP_TH + wave * UP_ROWS) * 4]) * stride;
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) {
                    const int* re = rt + (k * UP_TH + wave * UP_ROWS + j) * 4;
                    ro1[j] = __builtin_amdgcn_readfirstlane(re[1]) * stride;
                    ly[j] = __int_as_float(__builtin_amdgcn_readfirstlane(re[2]));
                    adv[j] = __builtin_amdgcn_readfirstlane(re[3]);
                    lse[j] = x_ok && y0 + j < OH ? lse_in[(size_t)j * OW] : 0.f;     // what this lane wrote in phase A
                }
#pragma unroll
                for (int q = 0; q < UPE_CR; ++q) {
                    if (q >= qn) break;
                    const float* p = vd + q;
                    // UpWalk's steps written out: inside this four-class, all-views loop the struct compiles to a stream that
                    // measures 0.6-0.8 % slower at 150 classes (profiles/upsample_family_ab.md)
                    float h0 = up_hlerp(p, ro0, off0, off1, lx), h1 = up_hlerp(p, ro1[0], off0, off1, lx), dh = h1 - h0;
#pragma unroll
                    for (int j = 0; j < UP_ROWS; ++j) {
                        if (adv[j]) {
                            h0 = h1;
                            h1 = up_hlerp(p, ro1[j], off0, off1, lx);
                            dh = h1 - h0;
                        }
                        s[q][j] += up_exp(__builtin_fmaf(dh, ly[j], h0) - lse[j]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < UPE_CR; ++q) {
                if (q >= qn) break;
                const int c = c0 + q0 + q;
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) {
                    if (PROBS) {
                        if (x_ok && y0 + j < OH) probs[((size_t)b * C + c) * plane + pix0 + (size_t)j * OW] = s[q][j] / Kf;
                    }
                    up_first_max(best[j], idx[j], s[q][j], c);
                }
            }
        }
    }
    if (active && x_ok) {
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j) {
            if (y0 + j >= OH) continue;
            const size_t o = (size_t)b * plane + pix0 + (size_t)j * OW;
            if (labels) labels[o] = idx[j];
            if (conf) conf[o] = best[j] / Kf;
        }
    }
}

// The tile grid and the LDS budget: the tables, then the summed footprints of all views at CCB classes per pass (phase B), which is
// also room for phase A's one view at a time.  64 KiB when that leaves at least 8 classes per pass, else up to the CU's 160 KiB.
int upsample_ensemble_plan(const char* who, const UpEnsViews& views, int K, int C, int OH, int OW, UpEnsPlan* plan) {
    long long cells = 0, widest = 0;
    for (int k = 0; k < K; ++k) {
        const long long view = (long long)up_max_footprint(views.v[k].wp, OW, UP_TW) * up_max_footprint(views.v[k].hp, OH, UP_TH);
        cells += view;                                  // <= 65 * 33 per view
        if (view > widest) widest = view;
    }
    const int tables = K * UPE_TABLE_WORDS;
    long long budget;
    const UpPass ps = up_pass_two_budgets(tables, cells, C, &budget);
    const int CC = ps.CC;
    if (CC < 1) {
        dinoseg_set_error("%s: the %d views' footprints of one tile add up to %lld cells, more than the LDS holds (%d words)", who, K, cells,
                          (int)budget);
        return -1;
    }
    // phase A stages one view: let it take all its classes in one pass where the default 64 KiB allows
    long long data_words = cells * ps.stride;
    long long want = widest * up_pass_of(C).stride;
    if (want > UP_LDS_WORDS - tables) want = UP_LDS_WORDS - tables;
    if (want > data_words) data_words = want;
    *plan = {(OW + UP_TW - 1) / UP_TW, (OH + UP_TH - 1) / UP_TH, CC, (int)data_words, (size_t)(tables + data_words) * sizeof(float)};
    return 0;
}

}  // namespace

long long upsample_ensemble_scratch_bytes(int K, int B, int OH, int OW) {
    if (K < 1 || K > UPE_MAX_VIEWS || B < 1 || OH < 1 || OW < 1) return -1;
    return 4ll * K * B * OH * OW;
}

// every host-side refusal of the ensemble, before anything is enqueued
int upsample_ensemble_check(const char* who, const UpEnsViews& views, int K, int B, int C, int OH, int OW) {
    if (K < 1 || K > UPE_MAX_VIEWS) {
        dinoseg_set_error("%s: %d views (1 <= K <= %d)", who, K, UPE_MAX_VIEWS);
        return -1;
    }
    for (int k = 0; k < K; ++k) {
        if (!views.v[k].logp) {
            dinoseg_set_error("%s: view %d: null pointer", who, k);
            return -1;
        }
        if (views.v[k].flip != 0 && views.v[k].flip != 1) {
            dinoseg_set_error("%s: view %d: flip is %d (0 or 1)", who, k, views.v[k].flip);
            return -1;
        }
        char name[96];
        snprintf(name, sizeof(name), "%s: view %d", who, k);
        if (upsample_check_shape(name, B, views.v[k].hp, views.v[k].wp, C, OH, OW)) return -1;
    }
    UpEnsPlan pl;
    return upsample_ensemble_plan(who, views, K, C, OH, OW, &pl);
}

int launch_upsample_ensemble(const UpEnsViews& views, int K, int B, int C, int OH, int OW, int32_t* labels, float* conf, float* probs,
                             void* scratch, hipStream_t s) {
    if (upsample_ensemble_check("upsample_ensemble", views, K, B, C, OH, OW)) return -1;
    if (!labels && !conf && !probs) {
        dinoseg_set_error("upsample_ensemble: null pointer (at least one of labels / conf / probs is required)");
        return -1;
    }
    if (!scratch) {
        dinoseg_set_error("upsample_ensemble: null scratch (dinoseg_op_upsample_ensemble_scratch_bytes of device memory)");
        return -1;
    }
    UpEnsPlan pl;
    if (upsample_ensemble_plan("upsample_ensemble", views, K, C, OH, OW, &pl)) return -1;
    static PerDeviceOnce once;
    const int rc = up_allow_large_lds(once, "upsample_ensemble_kernel", reinterpret_cast<const void*>(&upsample_ensemble_kernel<true>),
                                      reinterpret_cast<const void*>(&upsample_ensemble_kernel<false>));
    if (rc) return rc;
    const unsigned grid = (unsigned)((long long)pl.tiles_x * pl.tiles_y * B);
    float* lse = reinterpret_cast<float*>(scratch);
    if (probs)
        hipLaunchKernelGGL(upsample_ensemble_kernel<true>, dim3(grid), dim3(256), pl.lds_bytes, s, views, K, B, C, OH, OW, pl.tiles_x,
                           pl.tiles_y, pl.CCB, pl.data_words, labels, conf, probs, lse);
    else
        hipLaunchKernelGGL(upsample_ensemble_kernel<false>, dim3(grid), dim3(256), pl.lds_bytes, s, views, K, B, C, OH, OW, pl.tiles_x,
                           pl.tiles_y, pl.CCB, pl.data_words, labels, conf, probs, lse);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
