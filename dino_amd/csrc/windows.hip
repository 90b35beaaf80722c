// Sliding-window inference at pixel resolution: the frame is cut into overlapping windows of the training size, the model runs on
// every window, and ONE launch brings all windows' log-probs to pixel resolution, averages them where windows overlap and takes
// the argmax -- without a [B, C, H, W] accumulator, a count plane, or one interpolate per window.
//
// The window rule, per axis (frame side L, window w <= L, stride s >= 1):
//     g    = max(L - w + s - 1, 0) / s + 1
//     o[i] = max(min(i s + w, L) - w, 0),  i = 0 .. g-1              (the last window is shifted back to end at L)
// Windows of a frame are row-major over (gy, gx), windows of a batch frame-major: index (b gh + gy) gw + gx.
//
// crop_windows_kernel gathers a run of that list into one contiguous batch for the forward (one launch per chunk).
//
// window_merge_kernel, per pixel (y, x) and class c:
//     u_w[c] = bilinear value of window w's grid at the window's local pixel (y - oy, x - ox), upsampled from (wh/patch, ww/patch)
//              to (wh, ww): up_coord and the two chained fmaf lerps of upsample.hip, x first, then y
//     m[c]   = (u_w0[c] + u_w1[c] + ...) / (float)n     over the n windows that contain the pixel, in window order, fp32 adds,
//              IEEE division
//     dense = m,  label = the FIRST maximum of m.   No atomics, no scratch: bit-identical from run to run.
// One workgroup = one 64 x 32 output tile of one frame, wave w rows 8w .. 8w+7, lane l column l.  The windows that intersect a tile
// are a contiguous range of window rows times a contiguous range of window columns (tile-uniform), and the footprint of window
// (gy, gx) under the tile is rows(gy) x cols(gx): all footprints together are ONE staged grid of (sum of rows) x (sum of columns)
// cells, cell-major with an odd stride, CC classes per pass.  Four classes at a time a lane walks the windows (scalar loops), adds
// the window's value where its column (per-lane predicate) and the row (per-row, wave-uniform) are inside, and keeps the running
// first maximum of the quotient.  The coordinates of every window row / column of the tile live in LDS tables built once.
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

namespace {

constexpr int WM_CR = 4;                                               // classes per walk over the windows
constexpr int WM_MAX_COVERAGE = 4;                                     // windows over one pixel row / column

// one axis of the window rule; s is clamped to max(L - w, 1) on the host (the same origins), so i s + w stays far inside int32
struct WinAxis {
    int L, w, s, g, gp;                                                // frame side, window, stride, windows, window grid side (w / patch)
};

__host__ __device__ inline int win_origin(const WinAxis& a, int i) {
    int e = i * a.s + a.w;
    if (e > a.L) e = a.L;
    return e - a.w;                                                    // >= 0: w <= L
}
// the windows [lo, hi] that intersect the pixels first .. last (0 <= first <= last < L): origins are non-decreasing, every window
// but the last starts at i s, and the last ends at L
__host__ __device__ inline void win_range(const WinAxis& a, int first, int last, int* lo, int* hi) {
    int l = first >= a.w ? (first - a.w) / a.s + 1 : 0;
    if (l > a.g - 1) l = a.g - 1;
    int h = last / a.s;
    if (h > a.g - 1) h = a.g - 1;
    if (h < a.g - 1 && win_origin(a, a.g - 1) <= last) h = a.g - 1;
    *lo = l;
    *hi = h;
}
// the footprint of window i under those pixels: first grid index and extent
__host__ __device__ inline void win_footprint(const WinAxis& a, int i, int first, int last, int* f0, int* ext) {
    const int o = win_origin(a, i);
    const int pa = (first > o ? first : o) - o, pb = (last < o + a.w - 1 ? last : o + a.w - 1) - o;
    int a0, a1, b0, b1;
    unsigned rem;
    up_index(pa, a.gp, a.w, &a0, &a1, &rem);
    up_index(pb, a.gp, a.w, &b0, &b1, &rem);
    *f0 = a0;
    *ext = b1 - a0 + 1;
}

struct WinPlan {
    int tiles_x, tiles_y, CC, nwy, nwx, totr, totc;
    size_t lds_bytes;
};

__host__ __device__ inline int wm_table_words(int nwy, int nwx, int totr, int totc) {
    return 4 * nwy + 4 * nwx + 2 * UP_TH * nwy + 2 * UP_TW * nwx + totr + totc + UP_TH + 4;
}

template <bool DENSE>
__global__ __launch_bounds__(256) void window_merge_kernel(const float* __restrict__ logp, WinAxis ay, WinAxis ax, int C, int tiles_x,
                                                           int tiles_y, int CC, int nwy_cap, int nwx_cap, int totr_cap, int totc_cap,
                                                           int32_t* __restrict__ labels, float* __restrict__ dense) {
    extern __shared__ float wm_lds[];
    int* yv = reinterpret_cast<int*>(wm_lds);       // [nwy][4]: origin, first footprint row, rows, first row in the staged grid
    int* xv = yv + 4 * nwy_cap;                     // [nwx][4]: the same for columns
    int* yt = xv + 4 * nwx_cap;                     // [nwy][32][2]: staged row | second row is the next << 16 | mode << 17, lambda
    int* xt = yt + 2 * UP_TH * nwy_cap;             // [nwx][64][2]: staged column | second is the next << 16 | inside << 17, lambda
    int* rowpart = xt + 2 * UP_TW * nwx_cap;        // [totr]: source cell of the staged row's first column of window column 0
    int* colpart = rowpart + totr_cap;              // [totc]: what the staged column adds to it
    int* ycnt = colpart + totc_cap;                 // [32]: windows over each row of the tile
    int* tot = ycnt + UP_TH;                        // staged rows, staged columns
    float* data = reinterpret_cast<float*>(tot + 4);
    const int H = ay.L, W = ax.L;
    const UpTile T = up_tile(tiles_x, tiles_y, H, W);
    const int tid = T.tid, lane = T.lane, wave = T.wave, b = T.b, y0 = T.y0;
    const int x_first = T.x_first, y_first = T.y_first, x_last = T.x_last, y_last = T.y_last, xc = T.xc;
    const bool active = T.active, x_ok = T.x_ok;
    const size_t plane = T.plane, pix0 = T.pix0;
    const int ncell_win = ay.gp * ax.gp;                        // cells of one window's grid

    int gy_lo, gy_hi, gx_lo, gx_hi;
    win_range(ay, y_first, y_last, &gy_lo, &gy_hi);
    win_range(ax, x_first, x_last, &gx_lo, &gx_hi);
    const int nwy = gy_hi - gy_lo + 1, nwx = gx_hi - gx_lo + 1;

    // the windows' footprints under the tile, then where each starts in the staged grid
    for (int k = tid; k < nwy + nwx; k += 256) {
        const bool isy = k < nwy;
        const int kk = isy ? k : k - nwy;
        int f0, ext;
        if (isy) win_footprint(ay, gy_lo + kk, y_first, y_last, &f0, &ext);
        else win_footprint(ax, gx_lo + kk, x_first, x_last, &f0, &ext);
        int* v = (isy ? yv : xv) + 4 * kk;
        v[0] = isy ? win_origin(ay, gy_lo + kk) : win_origin(ax, gx_lo + kk);
        v[1] = f0;
        v[2] = ext;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
        int* v = tid ? xv : yv;
        const int n = tid ? nwx : nwy;
        int base = 0;
        for (int k = 0; k < n; ++k) {
            v[4 * k + 3] = base;
            base += v[4 * k + 2];
        }
        tot[tid ? 1 : 0] = base;
    }
    __syncthreads();
    const int totr = __builtin_amdgcn_readfirstlane(tot[0]), totc = __builtin_amdgcn_readfirstlane(tot[1]);

    // the coordinate tables: wave w fills window columns / rows w, w+4, ...
    int cnt_x = 0;
    for (int k = wave; k < nwx; k += UP_WAVES) {
        const int ox = xv[4 * k], fc0 = xv[4 * k + 1], ncols = xv[4 * k + 2], base = xv[4 * k + 3];
        const bool in = xc >= ox && xc < ox + ax.w;
        int e = base;
        float lam = 0.f;
        if (in) {
            const UpCoord cx = up_coord(xc - ox, ax.gp, ax.w);
            e = (base + cx.i0 - fc0) | ((cx.i1 - cx.i0) << 16) | (1 << 17);
            lam = cx.lam;
        }
        xt[(k * UP_TW + lane) * 2] = e;
        xt[(k * UP_TW + lane) * 2 + 1] = __float_as_int(lam);
        for (int c = lane; c < ncols; c += 64) colpart[base + c] = (gx_lo + k) * ncell_win + fc0 + c;
    }
    for (int k = wave; k < nwy; k += UP_WAVES) {
        const int oy = yv[4 * k], fr0 = yv[4 * k + 1], nrows = yv[4 * k + 2], base = yv[4 * k + 3];
        if (lane < UP_TH) {
            const int y = y_first + lane < H ? y_first + lane : H - 1;
            const bool in = y >= oy && y < oy + ay.w;
            int e = base;
            float lam = 0.f;
            if (in) {
                const UpCoord cy = up_coord(y - oy, ay.gp, ay.w);
                // 3: the first row of the wave's strip inside this window (both source rows are read), 2: the walk enters the next
                // source row (i0 grows by exactly one: the window is no smaller than its grid), 1: the same pair as the row above
                int mode = 3;
                const int yp = y_first + lane - 1 < H ? y_first + lane - 1 : H - 1;
                if ((lane & (UP_ROWS - 1)) && yp >= oy && yp < oy + ay.w) mode = up_coord(yp - oy, ay.gp, ay.w).i0 != cy.i0 ? 2 : 1;
                e = (base + cy.i0 - fr0) | ((cy.i1 - cy.i0) << 16) | (mode << 17);
                lam = cy.lam;
            }
            yt[(k * UP_TH + lane) * 2] = e;
            yt[(k * UP_TH + lane) * 2 + 1] = __float_as_int(lam);
        }
        for (int r = lane; r < nrows; r += 64) rowpart[base + r] = ((b * ay.g + gy_lo + k) * ax.g) * ncell_win + (fr0 + r) * ax.gp;
    }
    if (tid < UP_TH) {
        const int y = y_first + tid < H ? y_first + tid : H - 1;
        int n = 0;
        for (int k = 0; k < nwy; ++k) n += y >= yv[4 * k] && y < yv[4 * k] + ay.w;
        ycnt[tid] = n;
    }
    for (int k = 0; k < nwx; ++k) cnt_x += xc >= xv[4 * k] && xc < xv[4 * k] + ax.w;
    __syncthreads();

    float nf[UP_ROWS], best[UP_ROWS];
    int idx[UP_ROWS];
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        nf[j] = (float)(cnt_x * ycnt[wave * UP_ROWS + j]);      // >= 1: every pixel of the frame lies in a window
        best[j] = -INFINITY;
        idx[j] = 0;
    }
    const int stride = up_pass_of(CC).stride;
    const int rstride = totc * stride;
    const int ncells = totr * totc;
    const int kw_log2 = up_pass_of(CC).kw_log2, kw = 1 << kw_log2;    // (after rstride and ncells: kw_log2 first costs one s_waitcnt)

    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cn = C - c0 < CC ? C - c0 : CC;
        if (c0) __syncthreads();
        // stage classes c0 .. c0+cn of every window's footprint: up_stage's loop, the source cell from the two tables
        for (int cell = tid >> kw_log2; cell < ncells; cell += 256 >> kw_log2) {
            const int r = cell / totc, col = cell - r * totc;
            const float* g = logp + (size_t)(rowpart[r] + colpart[col]) * C + c0;
            float* d = data + cell * stride;
            for (int q = tid & (kw - 1); q < cn; q += kw) d[q] = g[q];
        }
        __syncthreads();
        if (!active) continue;
        for (int q0 = 0; q0 < cn; q0 += WM_CR) {
            const int qn = cn - q0 < WM_CR ? cn - q0 : WM_CR;
            float s[WM_CR][UP_ROWS];
#pragma unroll
            for (int q = 0; q < WM_CR; ++q)
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) s[q][j] = 0.f;
            for (int ky = 0; ky < nwy; ++ky) {
                int mode[UP_ROWS], ro0[UP_ROWS], ro1[UP_ROWS], any = 0;
                float ly[UP_ROWS];
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) {
                    const int* re = yt + (ky * UP_TH + wave * UP_ROWS + j) * 2;
                    const int e = __builtin_amdgcn_readfirstlane(re[0]);
                    ly[j] = __int_as_float(__builtin_amdgcn_readfirstlane(re[1]));
                    mode[j] = e >> 17;
                    any |= mode[j];
                    ro0[j] = (e & 0xffff) * rstride;
                    ro1[j] = ro0[j] + ((e >> 16) & 1) * rstride;
                }
                if (!any) continue;                 // none of this wave's rows lies in this window row
                for (int kx = 0; kx < nwx; ++kx) {
                    const int xe = xt[(kx * UP_TW + lane) * 2];
                    const float lx = __int_as_float(xt[(kx * UP_TW + lane) * 2 + 1]);
                    const bool in = (xe >> 17) & 1;
                    const int off0 = (xe & 0xffff) * stride, off1 = off0 + ((xe >> 16) & 1) * stride;
#pragma unroll
                    for (int q = 0; q < WM_CR; ++q) {
                        if (q >= qn) break;
                        const float* p = data + q0 + q;
                        float h0 = 0.f, h1 = 0.f, dh = 0.f;
#pragma unroll
                        for (int j = 0; j < UP_ROWS; ++j) {
                            if (mode[j] == 0) continue;
                            if (mode[j] == 3) h0 = up_hlerp(p, ro0[j], off0, off1, lx);
                            else if (mode[j] == 2) h0 = h1;
                            if (mode[j] >= 2) {
                                h1 = up_hlerp(p, ro1[j], off0, off1, lx);
                                dh = h1 - h0;
                            }
                            const float v = __builtin_fmaf(dh, ly[j], h0);
                            s[q][j] = in ? s[q][j] + v : s[q][j];
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < WM_CR; ++q) {
                if (q >= qn) break;
                const int c = c0 + q0 + q;
#pragma unroll
                for (int j = 0; j < UP_ROWS; ++j) {
                    const float m = __fdiv_rn(s[q][j], nf[j]);
                    if (DENSE) {
                        if (x_ok && y0 + j < H) dense[((size_t)b * C + c) * plane + pix0 + (size_t)j * W] = m;
                    }
                    up_first_max(best[j], idx[j], m, c);
                }
            }
        }
    }
    if (labels && active && x_ok) {
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j)
            if (y0 + j < H) labels[(size_t)b * plane + pix0 + (size_t)j * W] = idx[j];
    }
}

// One thread = 8 bytes (uint8 HWC: a row of a window is ww * 3 contiguous bytes on both sides) or 4 floats (fp32 CHW) of the
// destination: element-wise loads (a window starts at any pixel), one vector store (ww % 8 == 0, the destination 16-byte aligned).
template <int KIND>
__global__ __launch_bounds__(256) void crop_windows_kernel(const void* __restrict__ xin, WinAxis ay, WinAxis ax, int first,
                                                           long long units, void* __restrict__ out) {
    const int H = ay.L, W = ax.L, G = ay.g * ax.g;
    const int row_units = KIND == 0 ? ax.w * 3 / 8 : ax.w / 4;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
        const int ru = (int)(u % row_units);
        long long tt = u / row_units;
        const int r = (int)(tt % ay.w);
        tt /= ay.w;
        int ch = 0;
        if (KIND == 1) {
            ch = (int)(tt % 3);
            tt /= 3;
        }
        const int wi = first + (int)tt;
        const int b = wi / G, rem = wi - b * G;
        const int gy = rem / ax.g, gx = rem - gy * ax.g;
        const int oy = win_origin(ay, gy), ox = win_origin(ax, gx);
        if (KIND == 0) {
            const uint8_t* src = reinterpret_cast<const uint8_t*>(xin) + (((size_t)b * H + oy + r) * W + ox) * 3 + (size_t)ru * 8;
            uint2 v;
            v.x = src[0] | (src[1] << 8) | (src[2] << 16) | ((unsigned)src[3] << 24);
            v.y = src[4] | (src[5] << 8) | (src[6] << 16) | ((unsigned)src[7] << 24);
            reinterpret_cast<uint2*>(out)[u] = v;
        } else {
            const float* src = reinterpret_cast<const float*>(xin) + (((size_t)b * 3 + ch) * H + oy + r) * W + ox + (size_t)ru * 4;
            reinterpret_cast<float4*>(out)[u] = make_float4(src[0], src[1], src[2], src[3]);
        }
    }
}

// one axis of the rule on the host: -1 (and a message) for a bad window / stride; the stride clamped to max(L - w, 1)
int win_axis(const char* who, const char* name, int L, int w, int s, int patch, WinAxis* a) {
    if (L < 1 || w < 1) {
        dinoseg_set_error("%s: bad argument (%s: frame %d, window %d; sizes must be positive)", who, name, L, w);
        return -1;
    }
    if (s < 1) {
        dinoseg_set_error("%s: %s stride %d (strides must be positive)", who, name, s);
        return -1;
    }
    if (w % patch != 0) {
        dinoseg_set_error("%s: %s window %d is not a multiple of %d", who, name, w, patch);
        return -1;
    }
    if (w > L) {
        dinoseg_set_error("%s: %s window %d is larger than the frame (%d)", who, name, w, L);
        return -1;
    }
    if (L > (1 << 22)) {
        dinoseg_set_error("%s: %s frame side %d is too large", who, name, L);
        return -1;
    }
    const int cap = L - w > 1 ? L - w : 1;
    if (s > cap) s = cap;
    *a = {L, w, s, (L - w + s - 1) / s + 1, w / patch};
    return 0;
}

// the most windows over one pixel of the axis: attained at a window's first pixel, and the earliest window that still reaches it
// only moves forward with j
int win_axis_coverage(const WinAxis& a) {
    int most = 1;
    for (int j = 1, i = 0; j < a.g; ++j) {
        const int oj = win_origin(a, j);
        while (win_origin(a, i) + a.w <= oj) ++i;
        if (j - i + 1 > most) most = j - i + 1;
    }
    return most;
}

// the tile grid and the LDS budget: the tables, then the staged grid of the worst tile at CC classes per pass.  64 KiB when that
// leaves at least 8 classes per pass, else up to the CU's 160 KiB.
int window_merge_plan(const char* who, const WinAxis& ay, const WinAxis& ax, int C, WinPlan* plan) {
    int most_win[2] = {1, 1}, most_ext[2] = {1, 1};
    for (int axis = 0; axis < 2; ++axis) {
        const WinAxis& a = axis ? ax : ay;
        const int step = axis ? UP_TW : UP_TH;
        for (int first = 0; first < a.L; first += step) {
            const int last = (first + step < a.L ? first + step : a.L) - 1;
            int lo, hi, sum = 0;
            win_range(a, first, last, &lo, &hi);
            for (int i = lo; i <= hi; ++i) {
                int f0, ext;
                win_footprint(a, i, first, last, &f0, &ext);
                sum += ext;
            }
            if (hi - lo + 1 > most_win[axis]) most_win[axis] = hi - lo + 1;
            if (sum > most_ext[axis]) most_ext[axis] = sum;
        }
    }
    const long long cells = (long long)most_ext[0] * most_ext[1];
    const long long tables = wm_table_words(most_win[0], most_win[1], most_ext[0], most_ext[1]);
    long long budget;
    const UpPass ps = up_pass_two_budgets(tables, cells, C, &budget);
    if (ps.CC < 1) {
        dinoseg_set_error("%s: the windows' footprints under one tile add up to %lld cells, more than the LDS holds (%lld words)", who,
                          cells, budget);
        return -1;
    }
    *plan = {(ax.L + UP_TW - 1) / UP_TW, (ay.L + UP_TH - 1) / UP_TH, ps.CC, most_win[0], most_win[1], most_ext[0], most_ext[1],
             (size_t)(tables + cells * ps.stride) * sizeof(float)};
    return 0;
}

}  // namespace

int window_origins(int L, int win, int stride, int32_t* out, int cap) {
    if (L < 1 || win < 1 || win > L || stride < 1) {
        dinoseg_set_error("dinoseg_window_origins: bad argument (L=%d window=%d stride=%d; 1 <= window <= L, stride >= 1)", L, win, stride);
        return -1;
    }
    const long long g = ((long long)L - win + stride - 1) / stride + 1;
    if (!out && cap == 0) return g > 0x7fffffffll ? -1 : (int)g;
    if (!out || cap < g) {
        dinoseg_set_error("dinoseg_window_origins: room for %d origins, %lld needed", out ? cap : 0, g);
        return -1;
    }
    for (long long i = 0; i < g; ++i) {
        long long e = i * stride + win;
        if (e > L) e = L;
        out[i] = (int32_t)(e - win > 0 ? e - win : 0);
    }
    return (int)g;
}

int window_merge_check(const char* who, int B, int H, int W, int patch, int win_h, int win_w, int stride_h, int stride_w, int C) {
    if (C < 1 || C > HEAD_WIDE_MAX_C) {
        dinoseg_set_error("%s: %d classes (1 <= C <= %d)", who, C, HEAD_WIDE_MAX_C);
        return -1;
    }
    if (patch != 8 && patch != 16) {
        dinoseg_set_error("%s: patch %d (8 or 16)", who, patch);
        return -1;
    }
    if (B < 1) {
        dinoseg_set_error("%s: bad argument (B=%d; sizes must be positive)", who, B);
        return -1;
    }
    WinAxis ay, ax;
    if (win_axis(who, "vertical", H, win_h, stride_h, patch, &ay) || win_axis(who, "horizontal", W, win_w, stride_w, patch, &ax)) return -1;
    if (upsample_check_shape(who, B, ay.gp, ax.gp, C, H, W)) return -1;
    for (int axis = 0; axis < 2; ++axis) {
        const int cov = win_axis_coverage(axis ? ax : ay);
        if (cov > WM_MAX_COVERAGE) {
            dinoseg_set_error("%s: %s coverage %d: window %d at stride %d puts %d windows over one pixel %s (at most %d per axis)", who,
                              axis ? "horizontal" : "vertical", cov, axis ? win_w : win_h, axis ? stride_w : stride_h, cov,
                              axis ? "column" : "row", WM_MAX_COVERAGE);
            return -1;
        }
    }
    if ((long long)B * ay.g * ax.g * ay.gp * ax.gp > 0x7fffffffll) {
        dinoseg_set_error("%s: %d x %d x %d windows of %d x %d cells are too many", who, B, ay.g, ax.g, ay.gp, ax.gp);
        return -1;
    }
    WinPlan pl;
    return window_merge_plan(who, ay, ax, C, &pl);
}

int launch_window_merge(const float* logp, int B, int H, int W, int patch, int win_h, int win_w, int stride_h, int stride_w, int C,
                        int32_t* labels, float* dense, hipStream_t s) {
    const char* who = "window_merge";
    if (window_merge_check(who, B, H, W, patch, win_h, win_w, stride_h, stride_w, C)) return -1;
    if (!logp) {
        dinoseg_set_error("%s: null pointer (logp)", who);
        return -1;
    }
    if (!labels && !dense) {
        dinoseg_set_error("%s: null pointer (at least one of labels / dense is required)", who);
        return -1;
    }
    WinAxis ay, ax;
    WinPlan pl;
    if (win_axis(who, "vertical", H, win_h, stride_h, patch, &ay) || win_axis(who, "horizontal", W, win_w, stride_w, patch, &ax) ||
        window_merge_plan(who, ay, ax, C, &pl))
        return -1;
    static PerDeviceOnce once;
    const int rc = up_allow_large_lds(once, "window_merge_kernel", reinterpret_cast<const void*>(&window_merge_kernel<true>),
                                      reinterpret_cast<const void*>(&window_merge_kernel<false>));
    if (rc) return rc;
    const unsigned grid = (unsigned)((long long)pl.tiles_x * pl.tiles_y * B);
    if (dense)
        hipLaunchKernelGGL(window_merge_kernel<true>, dim3(grid), dim3(256), pl.lds_bytes, s, logp, ay, ax, C, pl.tiles_x, pl.tiles_y,
                           pl.CC, pl.nwy, pl.nwx, pl.totr, pl.totc, labels, dense);
    else
        hipLaunchKernelGGL(window_merge_kernel<false>, dim3(grid), dim3(256), pl.lds_bytes, s, logp, ay, ax, C, pl.tiles_x, pl.tiles_y,
                           pl.CC, pl.nwy, pl.nwx, pl.totr, pl.totc, labels, dense);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_crop_windows(const void* x, int kind, int B, int H, int W, int win_h, int win_w, int stride_h, int stride_w, int first,
                        int count, void* out, hipStream_t s) {
    const char* who = "crop_windows";
    if (!x || !out) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (kind != 0 && kind != 1) {
        dinoseg_set_error("%s: input kind %d (0 = uint8 [B,H,W,3], 1 = fp32 [B,3,H,W])", who, kind);
        return -1;
    }
    if (B < 1) {
        dinoseg_set_error("%s: bad argument (B=%d; sizes must be positive)", who, B);
        return -1;
    }
    WinAxis ay, ax;
    if (win_axis(who, "vertical", H, win_h, stride_h, 1, &ay) || win_axis(who, "horizontal", W, win_w, stride_w, 8, &ax)) return -1;
    const long long total = (long long)B * ay.g * ax.g;
    if (total > 0x7fffffffll) {
        dinoseg_set_error("%s: %d x %d x %d windows are too many", who, B, ay.g, ax.g);
        return -1;
    }
    if (first < 0 || count < 1 || (long long)first + count > total) {
        dinoseg_set_error("%s: windows %d .. %lld are outside the list of %lld", who, first, (long long)first + count - 1, total);
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0) {
        dinoseg_set_error("%s: the destination is not 16-byte aligned", who);
        return -1;
    }
    if ((long long)count * win_h > (1ll << 40) / (3ll * win_w)) {
        dinoseg_set_error("%s: %d windows of %d x %d are too large", who, count, win_h, win_w);
        return -1;
    }
    const long long units = (long long)count * win_h * (kind == 0 ? win_w * 3 / 8 : 3 * (win_w / 4));
    const long long blocks = (units + 255) / 256;
    const unsigned grid = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
    if (kind == 0)
        hipLaunchKernelGGL(crop_windows_kernel<0>, dim3(grid), dim3(256), 0, s, x, ay, ax, first, units, out);
    else
        hipLaunchKernelGGL(crop_windows_kernel<1>, dim3(grid), dim3(256), 0, s, x, ay, ax, first, units, out);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
