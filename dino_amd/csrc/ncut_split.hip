// The normalized cut's passes (ncut.hip; the rule: include/dinoseg.h, dinoseg_op_ncut_graph and its addendum) with a frame's rows
// dealt to many workgroups.  The rule fixes every order of summation as a function of n alone, so these launches give the same bits as
// ncut_iterate_kernel; what differs is who computes a row.  The only ordering between workgroups is the stream order of consecutive
// launches: no grid barrier, no flag, no atomic.
//
//   ncs_weights_kernel    one workgroup per frame: r and u (step 4) into the scratch.
//   ncs_pass_kernel       one launch per pass, B x (ceil(n / R) + [not the first pass]) workgroups of 1024 threads.  A row workgroup
//                         prepares the pass's input redundantly -- p = (z + y) / 2 from the old halves of the scratch, DN, DN (first
//                         pass: DN(z_in)), xv = z r, S; thread t owns cells t, t + 1024, ..., the sums are block sums in the rule's
//                         order, so every workgroup holds the same bits -- IN PLACE in the one LDS vector, which ends up as xv; a
//                         cell's thread writes z_i into the new half where the row is the workgroup's own.  Then the inner loop of
//                         ncut_iterate_kernel over its own R rows (scalar words as the lane mask of one select, two row streams per
//                         wave, an xor tree) and y_i into the new half.  The extra workgroup of a frame forms the previous pass's rho
//                         from the old halves: wave w chains rows w, w + 16, .. by fp64 fma, the waves are added in wave order.
//   ncs_result_kernel     one workgroup per frame: the last p, DN, the last rho, step 7.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace dseg {

namespace {

constexpr int NCS_THREADS = 1024, NCS_WAVES = NCS_THREADS / 64;
constexpr int NCS_LDS_BYTES = 160 * 1024;       // the CU's whole LDS
constexpr int NCS_FIXED_BYTES = 1024;           // the reduction slots: 2 x 16 fp64, 16 fp32 + 16 int32
constexpr int NCS_PAD_BYTES = 256;              // the last word's pad lanes read up to 63 floats past xv: they stay inside
constexpr int NCS_MAX_CELLS = (NCS_LDS_BYTES - NCS_FIXED_BYTES - NCS_PAD_BYTES) / 4;        // 40 640
constexpr int NCS_DEFAULT_LDS_BYTES = 64 * 1024;
constexpr int NCS_MAX_ITERS = 4096;
constexpr int NCS_TILE = 64;                    // query cells of a graph workgroup (ncut.hip)
constexpr int NCS_VECTORS = 6;                  // the scratch: z and y twice, r, u
constexpr int NCS_CUS = 256;
constexpr int NCS_MAX_CHOSEN_ROWS = 256;         // rows_per_group = 0 never chooses more
constexpr long long NCS_MAX_GRID = 0x7fffffffll;

static_assert(NCS_MAX_CELLS >= 14400, "960 x 960 at patch 8 must fit");

// x where the lane's bit of the wave-uniform word is set, else 0 (ncut.hip: nc_pick)
__device__ __forceinline__ float ncs_pick(unsigned long long word, float x) {
    float r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(word));
    return r;
}

__device__ __forceinline__ double ncs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the global sum of one value per thread: an xor tree per wave, the waves in wave order; the barrier also publishes LDS writes
struct NcsBlockSum {
    double* slots;
    int flip, lane, wave;
    __device__ __forceinline__ double operator()(double v) {
        double* s = slots + 16 * flip;
        flip ^= 1;
        v = ncs_wave_sum(v);
        if (lane == 0) s[wave] = v;
        __syncthreads();
        double t = s[0];
#pragma unroll
        for (int w = 1; w < NCS_WAVES; ++w) t += s[w];
        return t;
    }
};

// z <- (z - <u, z> u) / || . || on the LDS vector; every element is its thread's own
__device__ __forceinline__ void ncs_deflate_normalise(float* z, const float* __restrict__ u, int n, int tid, NcsBlockSum& block_sum) {
    double c = 0.0;
    for (int i = tid; i < n; i += NCS_THREADS) c = fma((double)u[i], (double)z[i], c);
    c = block_sum(c);
    double ss = 0.0;
    for (int i = tid; i < n; i += NCS_THREADS) {
        const float q = (float)((double)z[i] - c * (double)u[i]);
        z[i] = q;
        ss = fma((double)q, (double)q, ss);
    }
    ss = block_sum(ss);
    const double nrm = sqrt(ss);
    for (int i = tid; i < n; i += NCS_THREADS) z[i] = nrm > 0.0 ? (float)((double)z[i] / nrm) : 0.f;
}

// rho of the pass whose z and y these are: wave w chains rows w, w + 16, .. in order, the waves are added in wave order.  The chain is
// serial by the rule; the loads are not: a wave fetches 64 of its rows at a time, one per lane, and reads them back lane by lane.
__device__ __forceinline__ void ncs_rho(const float* __restrict__ z, const float* __restrict__ y, int n, int lane, int wave, double* s,
                                        float* __restrict__ out) {
    const int rows = wave < n ? (n - wave + NCS_WAVES - 1) / NCS_WAVES : 0;
    double rp = 0.0;
    for (int k0 = 0; k0 < rows; k0 += 64) {
        const int k = k0 + lane;
        const float zv = k < rows ? z[wave + NCS_WAVES * k] : 0.f;
        const float yv = k < rows ? y[wave + NCS_WAVES * k] : 0.f;
        auto step = [&](int l) {
            const float zl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(zv), l));
            const float yl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yv), l));
            rp = fma((double)zl, (double)yl, rp);
        };
        if (rows - k0 >= 64) {                                          // (constant lanes: with a lane index in a register the chain took 1.2x a batch-1 pass)
#pragma unroll
            for (int l = 0; l < 64; ++l) step(l);
        } else {
            for (int l = 0; l < rows - k0; ++l) step(l);
        }
    }
    if (lane == 0) s[wave] = rp;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s[0];
#pragma unroll
        for (int w = 1; w < NCS_WAVES; ++w) r += s[w];
        *out = (float)r;
    }
}

__global__ __launch_bounds__(NCS_THREADS) void ncs_weights_kernel(const int32_t* __restrict__ degree, int n, double eps,
                                                                  float* __restrict__ rr, float* __restrict__ u) {
    __shared__ double slots[2 * NCS_WAVES];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * n;
    NcsBlockSum block_sum{slots, 0, tid & 63, __builtin_amdgcn_readfirstlane(tid >> 6)};
    double part = 0.0;
    for (int i = tid; i < n; i += NCS_THREADS) {
        const int c = degree[base + i];
        const float d = (float)(eps * (double)(n - c) + (double)c);
        rr[base + i] = d > 0.f ? (float)(1.0 / sqrt((double)d)) : 0.f;
        u[base + i] = d;                                                // (its own thread reads it back below)
        part += (double)d;
    }
    const double dsum = block_sum(part);
    const double dnorm = sqrt(dsum);
    for (int i = tid; i < n; i += NCS_THREADS) u[base + i] = dnorm > 0.0 ? (float)(sqrt((double)u[base + i]) / dnorm) : 0.f;
}

// z_src / y_src: the old halves (first pass: the caller's z_in and no y); z_dst / y_dst: the new halves.  per = the workgroups of a frame.
__global__ __launch_bounds__(NCS_THREADS) void ncs_pass_kernel(const unsigned long long* __restrict__ graph, int n, double eps, int first,
                                                               const float* __restrict__ z_src, const float* __restrict__ y_src,
                                                               const float* __restrict__ rr_all, const float* __restrict__ u_all,
                                                               float* __restrict__ z_dst, float* __restrict__ y_dst, int R, int groups,
                                                               int per, float* __restrict__ rho_prev, int rho_stride) {
    extern __shared__ __attribute__((aligned(16))) char ncs_lds[];
    double* slots = reinterpret_cast<double*>(ncs_lds);                // [2][16]
    float* v = reinterpret_cast<float*>(ncs_lds + NCS_FIXED_BYTES);    // [n] p, then z, then xv (a word's pad lanes read past it, inside the allocation; never selected)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)blockIdx.x / per, g = (int)blockIdx.x - b * per, W = (n + 63) >> 6;
    const size_t base = (size_t)b * n;
    z_src += base;
    if (g == groups) {                                                  // the frame's record workgroup (never on the first pass)
        ncs_rho(z_src, y_src + base, n, lane, wave, slots, rho_prev + (size_t)b * rho_stride);
        return;
    }
    const float* rr = rr_all + base;
    const float* u = u_all + base;
    NcsBlockSum block_sum{slots, 0, lane, wave};
    const int row0 = g * R, row_end = min(n, row0 + R);

    if (first) {
        for (int i = tid; i < n; i += NCS_THREADS) v[i] = z_src[i];
    } else {
        for (int i = tid; i < n; i += NCS_THREADS) v[i] = 0.5f * (z_src[i] + y_src[base + i]);
        ncs_deflate_normalise(v, u, n, tid, block_sum);
    }
    ncs_deflate_normalise(v, u, n, tid, block_sum);

    double S = 0.0;
    for (int i = tid; i < n; i += NCS_THREADS) {
        const float zi = v[i];
        const float x = zi * rr[i];
        v[i] = x;
        S += (double)x;
        if (i >= row0 && i < row_end) z_dst[base + i] = zi;
    }
    S = block_sum(S);
    const double epsS = eps * S, om = 1.0 - eps;
    auto finish = [&](int i, float ti) {                                // (ti: the xor tree left the same bits in every lane)
        const float y = (float)((double)rr[i] * (epsS + om * (double)ti));
        if (lane == 0) y_dst[base + i] = y;
    };
    // two rows of the wave at a time, i and i + 16: one read of xv serves both, and two streams of words are in flight
    for (int i = row0 + wave; i < row_end; i += 2 * NCS_WAVES) {
        const bool two = i + NCS_WAVES < row_end;
        const unsigned long long* row_a = graph + (base + i) * W;
        const unsigned long long* row_b = two ? row_a + (size_t)NCS_WAVES * W : row_a;   // (no second row: the first again, unused)
        float acc_a = 0.f, acc_b = 0.f;
        int w = 0;
        if (W >= 8) {                                                   // eight words at a time, the next eight in flight
            unsigned long long cur_a[8], cur_b[8], nxt_a[8], nxt_b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                cur_a[k] = row_a[k];
                cur_b[k] = row_b[k];
            }
            for (; w + 8 <= W; w += 8) {
                const int ahead = w + 16 <= W ? w + 8 : 0;              // (past the last group: re-read the first)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    nxt_a[k] = row_a[ahead + k];
                    nxt_b[k] = row_b[ahead + k];
                }
                float x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = v[(w + k) * 64 + lane];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    acc_a += ncs_pick(cur_a[k], x[k]);
                    acc_b += ncs_pick(cur_b[k], x[k]);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    cur_a[k] = nxt_a[k];
                    cur_b[k] = nxt_b[k];
                }
            }
        }
        for (; w < W; ++w) {
            const float x = v[w * 64 + lane];
            acc_a += ncs_pick(row_a[w], x);
            acc_b += ncs_pick(row_b[w], x);
        }
        finish(i, wave_sum(acc_a));
        if (two) finish(i + NCS_WAVES, wave_sum(acc_b));
    }
}

// z_src may be z_out (iters = 0: both the caller's): element i of both belongs to thread i % 1024, which reads first and writes after
__global__ __launch_bounds__(NCS_THREADS) void ncs_result_kernel(int n, int first, const float* z_src, const float* __restrict__ y_src,
                                                                 const float* __restrict__ rr_all, const float* __restrict__ u_all,
                                                                 float* z_out, float* __restrict__ rho_last, int rho_stride,
                                                                 uint8_t* __restrict__ fg, float* __restrict__ eigvec,
                                                                 float* __restrict__ margin, int32_t* __restrict__ seed_cell) {
    extern __shared__ __attribute__((aligned(16))) char ncs_lds[];
    double* slots = reinterpret_cast<double*>(ncs_lds);                // [2][16]: the waves' sums, two uses alternating
    double* rslots = reinterpret_cast<double*>(ncs_lds + 512);         // [16] the waves' shares of rho
    float* amax = reinterpret_cast<float*>(ncs_lds + 256);             // [16] the waves' largest |v|
    int* aidx = reinterpret_cast<int*>(ncs_lds + 320);                 // [16] ... and its cell
    float* v = reinterpret_cast<float*>(ncs_lds + NCS_FIXED_BYTES);    // [n] p, then z, then v = z r
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const size_t base = (size_t)b * n;
    const float* rr = rr_all + base;
    const float* u = u_all + base;
    NcsBlockSum block_sum{slots, 0, lane, wave};

    if (first) {
        for (int i = tid; i < n; i += NCS_THREADS) v[i] = z_src[base + i];
    } else {
        ncs_rho(z_src + base, y_src + base, n, lane, wave, rslots, rho_last + (size_t)b * rho_stride);
        for (int i = tid; i < n; i += NCS_THREADS) v[i] = 0.5f * (z_src[base + i] + y_src[base + i]);
    }
    ncs_deflate_normalise(v, u, n, tid, block_sum);

    // the result: v = z r, its mean, the seed, the sign, the partition
    double vs = 0.0;
    float ba = -1.f;
    int bi = INT_MAX;
    for (int i = tid; i < n; i += NCS_THREADS) {
        const float zi = v[i];
        const float x = zi * rr[i];
        z_out[base + i] = zi;
        v[i] = x;
        vs += (double)x;
        const float a = fabsf(x);
        if (a > ba) {                                                   // (strict: the lower cell keeps an exact tie)
            ba = a;
            bi = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a2 = __shfl_xor(ba, o);
        const int i2 = __shfl_xor(bi, o);
        if (a2 > ba || (a2 == ba && i2 < bi)) {
            ba = a2;
            bi = i2;
        }
    }
    if (lane == 0) {
        amax[wave] = ba;
        aidx[wave] = bi;
    }
    const double avg = block_sum(vs) / (double)n;                       // (its barrier publishes v, amax and aidx)
    ba = amax[0];
    bi = aidx[0];
#pragma unroll
    for (int w = 1; w < NCS_WAVES; ++w) {
        const float a2 = amax[w];
        const int i2 = aidx[w];
        if (a2 > ba || (a2 == ba && i2 < bi)) {
            ba = a2;
            bi = i2;
        }
    }
    if (bi == INT_MAX) bi = 0;                                          // (no |v| compared greater than -1: not a finite input)
    const float sigma = (double)v[bi] > avg ? 1.f : -1.f;
    if (tid == 0) seed_cell[b] = bi;
    for (int i = tid; i < n; i += NCS_THREADS) {
        const float x = v[i];
        const float m = (float)((double)sigma * ((double)x - avg));
        eigvec[base + i] = sigma * x;
        fg[base + i] = m > 0.f ? 1 : 0;
        if (margin) margin[base + i] = m;
    }
}

bool ncs_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

bool ncs_shape_ok(int B, int n) {
    return B >= 1 && n >= 1 && n <= NCS_MAX_CELLS && (long long)B * ((n + NCS_TILE - 1) / NCS_TILE) <= NCS_MAX_GRID;
}

// The library's choice (measured: tools/ncut_split_cost.py --rows): the smallest multiple of 32 (every wave walks whole pairs of rows)
// at which a pass's B ceil(n / R) row workgroups are at most one per compute unit -- all of them run at once and the redundant
// preparation is paid once per pass -- but never more than 256 rows: at batch 32 groups of 256 rows, two rounds of workgroups,
// measured 1.2x faster than one round of 480 or 608 rows.
int ncs_choose_rows(int B, int n) {
    int R = 32;
    while (R < n && R < NCS_MAX_CHOSEN_ROWS && (long long)B * ((n + R - 1) / R) > NCS_CUS) R += 32;
    return R;
}

}  // namespace

int ncut_split_max_cells() { return NCS_MAX_CELLS; }

long long ncut_split_graph_bytes(int B, int n) { return ncs_shape_ok(B, n) ? 8ll * B * n * ((n + 63) / 64) : -1; }

long long ncut_split_scratch_bytes(int B, int n) { return ncs_shape_ok(B, n) ? 4ll * NCS_VECTORS * B * n : -1; }

int launch_ncut_iterate_split(const void* graph, const int32_t* degree, int B, int n, double eps, const float* z_in, int iters,
                              int rows_per_group, float* z_out, float* rho, uint8_t* fg, float* eigvec, float* margin, int32_t* seed_cell,
                              void* scratch, hipStream_t s) {
    const char* who = "dinoseg_op_ncut_iterate_split";
    if (!graph || !degree || !z_in || !z_out || !fg || !eigvec || !seed_cell || !scratch) {
        dinoseg_set_error("%s: null pointer (only margin, and rho with iters = 0, are optional)", who);
        return -1;
    }
    if (B < 1 || n < 1) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive)", who, B, n);
        return -1;
    }
    if (n > NCS_MAX_CELLS) {
        dinoseg_set_error("%s: n = %d cells exceed the %d whose vector fits the LDS of a row workgroup", who, n, NCS_MAX_CELLS);
        return -1;
    }
    if (rows_per_group < 0) {
        dinoseg_set_error("%s: rows_per_group = %d (0 for the library's choice, or at least 1)", who, rows_per_group);
        return -1;
    }
    const int R = rows_per_group == 0 ? ncs_choose_rows(B, n) : std::min(rows_per_group, n);
    const int groups = (n + R - 1) / R;
    if (!ncs_shape_ok(B, n) || (long long)B * (groups + 1) > NCS_MAX_GRID) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells in groups of %d rows exceed the launch range", who, B, n, R);
        return -1;
    }
    if (iters < 0 || iters > NCS_MAX_ITERS) {
        dinoseg_set_error("%s: iters = %d (0 .. %d)", who, iters, NCS_MAX_ITERS);
        return -1;
    }
    if (iters > 0 && !rho) {
        dinoseg_set_error("%s: null pointer (rho is required with iters > 0)", who);
        return -1;
    }
    if (!(eps >= 0.0 && eps < 1.0)) {
        dinoseg_set_error("%s: eps = %g (inside [0, 1))", who, eps);
        return -1;
    }
    if (ncs_misaligned(graph, 7) || ncs_misaligned(degree, 3) || ncs_misaligned(z_in, 3) || ncs_misaligned(z_out, 3) || ncs_misaligned(rho, 3) ||
        ncs_misaligned(eigvec, 3) || ncs_misaligned(margin, 3) || ncs_misaligned(seed_cell, 3) || ncs_misaligned(scratch, 15)) {
        dinoseg_set_error("%s: the graph must be 8-byte aligned, a 32-bit array 4-byte aligned, the scratch 16-byte aligned", who);
        return -1;
    }
    const size_t lds = (size_t)NCS_FIXED_BYTES + NCS_PAD_BYTES + (size_t)n * 4;
    if (lds > NCS_DEFAULT_LDS_BYTES) {
        static PerDeviceOnce once;
        if (once.first()) {
            DSEG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ncs_pass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               NCS_LDS_BYTES));
            DSEG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ncs_result_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               NCS_LDS_BYTES));
            once.mark();
        }
    }
    // the scratch: z[2], y[2], r, u, each [B][n] fp32.  Pass t reads half (t - 1) & 1 and writes half t & 1.
    const size_t vec = (size_t)B * n;
    float* sc = reinterpret_cast<float*>(scratch);
    float* zh[2] = {sc, sc + vec};
    float* yh[2] = {sc + 2 * vec, sc + 3 * vec};
    float* rr = sc + 4 * vec;
    float* u = sc + 5 * vec;
    const unsigned long long* g64 = reinterpret_cast<const unsigned long long*>(graph);
    hipLaunchKernelGGL(ncs_weights_kernel, dim3((unsigned)B), dim3(NCS_THREADS), 0, s, degree, n, eps, rr, u);
    DSEG_CHECK_HIP(hipGetLastError());
    for (int t = 0; t < iters; ++t) {
        const int first = t == 0, per = groups + (first ? 0 : 1), o = (t + 1) & 1, h = t & 1;
        hipLaunchKernelGGL(ncs_pass_kernel, dim3((unsigned)((long long)B * per)), dim3(NCS_THREADS), lds, s, g64, n, eps, first,
                           first ? z_in : zh[o], first ? nullptr : yh[o], rr, u, zh[h], yh[h], R, groups, per,
                           first ? nullptr : rho + (t - 1), iters);
        DSEG_CHECK_HIP(hipGetLastError());
    }
    const int first = iters == 0, o = (iters + 1) & 1;
    hipLaunchKernelGGL(ncs_result_kernel, dim3((unsigned)B), dim3(NCS_THREADS), lds, s, n, first, first ? z_in : zh[o],
                       first ? nullptr : yh[o], rr, u, z_out, first ? nullptr : rho + (iters - 1), iters, fg, eigvec, margin, seed_cell);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
