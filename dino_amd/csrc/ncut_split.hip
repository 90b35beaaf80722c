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
//                         cell's thread writes z_i into the new half where the row is the workgroup's own.  Then the row sums of its
//                         own R rows and y_i into the new half.  The extra workgroup of a frame forms the previous pass's rho from
//                         the old halves: wave w chains rows w, w + 16, .. by fp64 fma, the waves are added in wave order.
//   ncs_result_kernel     one workgroup per frame: the last p, DN, the last rho, step 7.
// The weights, the deflation (DN), the row sums, the block sums and step 7 are the pieces of ncut_common.h, the same code that
// ncut_iterate_kernel runs; this file owns who computes a row, the scratch and ncs_rho.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "ncut_common.h"

#include <algorithm>
#include <cmath>

namespace dseg {

namespace {

constexpr int NCS_MAX_CELLS = nc_cell_limit(1); // 40 640: the one LDS vector of a row workgroup
constexpr int NCS_VECTORS = 6;                  // the scratch: z and y twice, r, u
constexpr int NCS_CUS = 256;
constexpr int NCS_MAX_CHOSEN_ROWS = 256;         // rows_per_group = 0 never chooses more

static_assert(NCS_MAX_CELLS == 40640, "the split entries publish this limit");
static_assert(NCS_MAX_CELLS >= 14400, "960 x 960 at patch 8 must fit");

// rho of the pass whose z and y these are: wave w chains rows w, w + 16, .. in order, the waves are added in wave order.  The chain is
// serial by the rule; the loads are not: a wave fetches 64 of its rows at a time, one per lane, and reads them back lane by lane.
__device__ __forceinline__ void ncs_rho(const float* __restrict__ z, const float* __restrict__ y, int n, int lane, int wave, double* s,
                                        float* __restrict__ out) {
    const int rows = wave < n ? (n - wave + NC_WAVES - 1) / NC_WAVES : 0;
    double rp = 0.0;
    for (int k0 = 0; k0 < rows; k0 += 64) {
        const int k = k0 + lane;
        const float zv = k < rows ? z[wave + NC_WAVES * k] : 0.f;
        const float yv = k < rows ? y[wave + NC_WAVES * k] : 0.f;
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
        for (int w = 1; w < NC_WAVES; ++w) r += s[w];
        *out = (float)r;
    }
}

__global__ __launch_bounds__(NC_THREADS) void ncs_weights_kernel(const int32_t* __restrict__ degree, int n, double eps,
                                                                  float* __restrict__ rr, float* __restrict__ u) {
    __shared__ double slots[2 * NC_WAVES];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * n;
    NcBlockSum block_sum{slots, 0, tid & 63, __builtin_amdgcn_readfirstlane(tid >> 6)};
    nc_weights(degree + base, n, eps, rr + base, u + base, tid, block_sum);
}

// z_src / y_src: the old halves (first pass: the caller's z_in and no y); z_dst / y_dst: the new halves.  per = the workgroups of a frame.
__global__ __launch_bounds__(NC_THREADS) void ncs_pass_kernel(const unsigned long long* __restrict__ graph, int n, double eps, int first,
                                                               const float* __restrict__ z_src, const float* __restrict__ y_src,
                                                               const float* __restrict__ rr_all, const float* __restrict__ u_all,
                                                               float* __restrict__ z_dst, float* __restrict__ y_dst, int R, int groups,
                                                               int per, float* __restrict__ rho_prev, int rho_stride) {
    extern __shared__ __attribute__((aligned(16))) char ncs_lds[];
    double* slots = reinterpret_cast<double*>(ncs_lds);                // [2][16]
    float* v = reinterpret_cast<float*>(ncs_lds + NC_FIXED_BYTES);    // [n] p, then z, then xv (a word's pad lanes read past it, inside the allocation; never selected)
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
    NcBlockSum block_sum{slots, 0, lane, wave};
    const int row0 = g * R, row_end = min(n, row0 + R);

    if (first) {
        for (int i = tid; i < n; i += NC_THREADS) v[i] = z_src[i];
    } else {
        for (int i = tid; i < n; i += NC_THREADS) v[i] = 0.5f * (z_src[i] + y_src[base + i]);
        nc_deflate_normalise(v, u, n, tid, block_sum);
    }
    nc_deflate_normalise(v, u, n, tid, block_sum);

    double S = 0.0;
    for (int i = tid; i < n; i += NC_THREADS) {
        const float zi = v[i];
        const float x = zi * rr[i];
        v[i] = x;
        S += (double)x;
        if (i >= row0 && i < row_end) z_dst[base + i] = zi;
    }
    S = block_sum(S);
    const double epsS = eps * S, om = 1.0 - eps;
    nc_row_walk(graph + base * W, W, row0, row_end, v, lane, wave, [&](int i, float ti) {
        const float y = (float)((double)rr[i] * (epsS + om * (double)ti));
        if (lane == 0) y_dst[base + i] = y;
    });
}

// z_src may be z_out (iters = 0: both the caller's): element i of both belongs to thread i % 1024, which reads first and writes after
__global__ __launch_bounds__(NC_THREADS) void ncs_result_kernel(int n, int first, const float* z_src, const float* __restrict__ y_src,
                                                                 const float* __restrict__ rr_all, const float* __restrict__ u_all,
                                                                 float* z_out, float* __restrict__ rho_last, int rho_stride,
                                                                 uint8_t* __restrict__ fg, float* __restrict__ eigvec,
                                                                 float* __restrict__ margin, int32_t* __restrict__ seed_cell) {
    extern __shared__ __attribute__((aligned(16))) char ncs_lds[];
    double* slots = reinterpret_cast<double*>(ncs_lds);                // [2][16]: the waves' sums, two uses alternating
    double* rslots = reinterpret_cast<double*>(ncs_lds + NC_SLOT_RHO); // [16] the waves' shares of rho
    float* v = reinterpret_cast<float*>(ncs_lds + NC_FIXED_BYTES);    // [n] p, then z, then v = z r
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const size_t base = (size_t)b * n;
    const float* rr = rr_all + base;
    const float* u = u_all + base;
    NcBlockSum block_sum{slots, 0, lane, wave};

    if (first) {
        for (int i = tid; i < n; i += NC_THREADS) v[i] = z_src[base + i];
    } else {
        ncs_rho(z_src + base, y_src + base, n, lane, wave, rslots, rho_last + (size_t)b * rho_stride);
        for (int i = tid; i < n; i += NC_THREADS) v[i] = 0.5f * (z_src[base + i] + y_src[base + i]);
    }
    nc_deflate_normalise(v, u, n, tid, block_sum);
    nc_result(ncs_lds, v, rr, n, tid, block_sum, z_out + base, eigvec + base, fg + base, margin ? margin + base : nullptr, seed_cell + b);
}

bool ncs_shape_ok(int B, int n) {
    return B >= 1 && n >= 1 && n <= NCS_MAX_CELLS && (long long)B * ((n + NC_TILE - 1) / NC_TILE) <= NC_MAX_GRID;
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
    const NcIterateArgs args{graph, degree, B, n, eps, z_in, iters, z_out, rho, fg, eigvec, margin, seed_cell};
    int R = 0, groups = 0;
    auto route_checks = [&]() {
        if (rows_per_group < 0) {
            dinoseg_set_error("%s: rows_per_group = %d (0 for the library's choice, or at least 1)", who, rows_per_group);
            return -1;
        }
        R = rows_per_group == 0 ? ncs_choose_rows(B, n) : std::min(rows_per_group, n);
        groups = (n + R - 1) / R;
        if (!ncs_shape_ok(B, n) || (long long)B * (groups + 1) > NC_MAX_GRID) {
            dinoseg_set_error("%s: B = %d frames of n = %d cells in groups of %d rows exceed the launch range", who, B, n, R);
            return -1;
        }
        return 0;
    };
    if (nc_iterate_check(who, args, true, scratch, NCS_MAX_CELLS, "vector fits the LDS of a row workgroup", route_checks)) return -1;
    const size_t lds = (size_t)NC_FIXED_BYTES + NC_PAD_BYTES + (size_t)n * 4;
    if (lds > NC_DEFAULT_LDS_BYTES) {
        static PerDeviceOnce once;
        if (once.first()) {
            DSEG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ncs_pass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               NC_LDS_BYTES));
            DSEG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ncs_result_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               NC_LDS_BYTES));
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
    hipLaunchKernelGGL(ncs_weights_kernel, dim3((unsigned)B), dim3(NC_THREADS), 0, s, degree, n, eps, rr, u);
    DSEG_CHECK_HIP(hipGetLastError());
    for (int t = 0; t < iters; ++t) {
        const int first = t == 0, per = groups + (first ? 0 : 1), o = (t + 1) & 1, h = t & 1;
        hipLaunchKernelGGL(ncs_pass_kernel, dim3((unsigned)((long long)B * per)), dim3(NC_THREADS), lds, s, g64, n, eps, first,
                           first ? z_in : zh[o], first ? nullptr : yh[o], rr, u, zh[h], yh[h], R, groups, per,
                           first ? nullptr : rho + (t - 1), iters);
        DSEG_CHECK_HIP(hipGetLastError());
    }
    const int first = iters == 0, o = (iters + 1) & 1;
    hipLaunchKernelGGL(ncs_result_kernel, dim3((unsigned)B), dim3(NC_THREADS), lds, s, n, first, first ? z_in : zh[o],
                       first ? nullptr : yh[o], rr, u, z_out, first ? nullptr : rho + (iters - 1), iters, fg, eigvec, margin, seed_cell);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
