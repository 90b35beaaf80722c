// The pieces of the normalized cut's passes (the rule: include/dinoseg.h, dinoseg_op_ncut_graph and its addendum), shared by ncut.hip
// (one workgroup per frame runs every pass) and ncut_split.hip (a frame's rows dealt to many workgroups, one launch per pass): ONE
// copy of every order of summation, so the two routes give the same bits in every output.
//
// The family's geometry: a workgroup of 1024 threads = 16 waves.  Thread t owns cells t, t + 1024, ... of a vector: it adds them in
// that order, and every element is read back by the thread that wrote it.  The global sums (||sqrt(d)||^2, <u, z>, ||q||^2, S, the
// mean) are fp64: an xor tree per wave, the 16 waves in wave order (NcBlockSum).  The row sums: rows are dealt to the 16 waves, a
// row's words are wave-uniform (scalar loads), lane l owns keys l, l + 64, ...: per word one conflict-free ds_read_b32 of xv[64 w +
// l], shared by the two rows a wave walks at a time, and one select with the word itself as the lane mask, added in ascending w; the
// 64 lanes meet in an xor tree (nc_row_walk).
//
// The dynamic LDS of a pass or result workgroup: NC_FIXED_BYTES of reduction slots -- [2][16] fp64 sums at 0 (two uses
// alternating), [16] fp32 largest |v| at 256, [16] int32 its cell at 320, [16] fp64 shares of rho at 512 -- then the route's vectors
// of n floats each, then NC_PAD_BYTES: the last word's pad lanes read up to 63 floats past a vector, inside the allocation, never
// selected.
#pragma once
#include "common.h"
#include "pair_common.h"

#include <climits>

namespace dseg {

constexpr int NC_TILE = PAIR_TILE;              // query cells of a graph workgroup
constexpr int NC_THREADS = 1024, NC_WAVES = NC_THREADS / 64;
constexpr int NC_LDS_BYTES = 160 * 1024;        // the CU's whole LDS
constexpr int NC_FIXED_BYTES = 1024;            // the reduction slots
constexpr int NC_SLOT_AMAX = 256, NC_SLOT_AIDX = 320, NC_SLOT_RHO = 512;
constexpr int NC_PAD_BYTES = 256;
constexpr int NC_DEFAULT_LDS_BYTES = 64 * 1024; // beyond it a launch needs the opt-in
constexpr int NC_MAX_ITERS = 4096;
constexpr long long NC_MAX_GRID = 0x7fffffffll;
// the cells whose `vectors` LDS vectors fit one workgroup
constexpr int nc_cell_limit(int vectors) { return (NC_LDS_BYTES - NC_FIXED_BYTES - NC_PAD_BYTES) / (4 * vectors); }

// x where the lane's bit of the wave-uniform word is set, else 0: the word itself is the lane mask of one select
__device__ __forceinline__ float nc_pick(unsigned long long word, float x) {
    float r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(word));
    return r;
}

// the global sum of one value per thread: an xor tree per wave, the waves in wave order; the barrier inside also publishes LDS writes
struct NcBlockSum {
    double* slots;                                                      // [2][16]
    int flip, lane, wave;
    __device__ __forceinline__ double* next() {
        double* s = slots + 16 * flip;
        flip ^= 1;
        return s;
    }
    __device__ __forceinline__ double operator()(double v) {
        double* s = next();
        v = wave_sum_f64(v);
        if (lane == 0) s[wave] = v;
        __syncthreads();
        double t = s[0];
#pragma unroll
        for (int w = 1; w < NC_WAVES; ++w) t += s[w];
        return t;
    }
};

// r = 1 / sqrt(d) and the known top vector u = sqrt(d) / ||sqrt(d)|| from the degree, d = eps (n - c) + c (step 4); rr and u are the
// frame's, in LDS or in global memory
__device__ __forceinline__ void nc_weights(const int32_t* degree, int n, double eps, float* rr, float* u, int tid, NcBlockSum& block_sum) {
    double part = 0.0;
    for (int i = tid; i < n; i += NC_THREADS) {
        const int c = degree[i];
        const float d = (float)(eps * (double)(n - c) + (double)c);
        rr[i] = d > 0.f ? (float)(1.0 / sqrt((double)d)) : 0.f;
        u[i] = d;                                                       // (its own thread reads it back below)
        part += (double)d;
    }
    const double dsum = block_sum(part);
    const double dnorm = sqrt(dsum);
    for (int i = tid; i < n; i += NC_THREADS) u[i] = dnorm > 0.0 ? (float)(sqrt((double)u[i]) / dnorm) : 0.f;
}

// z <- (z - <u, z> u) / || . || on the LDS vector; every element is its thread's own
__device__ __forceinline__ void nc_deflate_normalise(float* z, const float* u, int n, int tid, NcBlockSum& block_sum) {
    double c = 0.0;
    for (int i = tid; i < n; i += NC_THREADS) c = fma((double)u[i], (double)z[i], c);
    c = block_sum(c);
    double ss = 0.0;
    for (int i = tid; i < n; i += NC_THREADS) {
        const float q = (float)((double)z[i] - c * (double)u[i]);
        z[i] = q;
        ss = fma((double)q, (double)q, ss);
    }
    ss = block_sum(ss);
    const double nrm = sqrt(ss);
    for (int i = tid; i < n; i += NC_THREADS) z[i] = nrm > 0.0 ? (float)((double)z[i] / nrm) : 0.f;
}

// The row sums of rows row0 .. row_end - 1 of one frame (rows: its words [n][W], xv in LDS): finish(i, sum over the set bits of row
// i of xv), the xor tree having left the same bits in every lane.  Two rows of the wave at a time, i and i + 16: one read of xv
// serves both, and two streams of words are in flight.
template <class Finish>
__device__ __forceinline__ void nc_row_walk(const unsigned long long* rows, int W, int row0, int row_end, const float* xv, int lane,
                                            int wave, Finish finish) {
    for (int i = row0 + wave; i < row_end; i += 2 * NC_WAVES) {
        const bool two = i + NC_WAVES < row_end;
        const unsigned long long* row_a = rows + (size_t)i * W;
        const unsigned long long* row_b = two ? row_a + (size_t)NC_WAVES * W : row_a;       // (no second row: the first again, unused)
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
                for (int k = 0; k < 8; ++k) x[k] = xv[(w + k) * 64 + lane];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    acc_a += nc_pick(cur_a[k], x[k]);
                    acc_b += nc_pick(cur_b[k], x[k]);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    cur_a[k] = nxt_a[k];
                    cur_b[k] = nxt_b[k];
                }
            }
        }
        for (; w < W; ++w) {
            const float x = xv[w * 64 + lane];
            acc_a += nc_pick(row_a[w], x);
            acc_b += nc_pick(row_b[w], x);
        }
        finish(i, wave_sum(acc_a));
        if (two) finish(i + NC_WAVES, wave_sum(acc_b));
    }
}

// The result (step 7) from the frame's final z in the LDS vector v (overwritten by z r) and its r: z_out, then v = z r, its mean,
// the seed cell (largest |v|, the lowest cell on a tie), the sign, the partition.  lds: the workgroup's slots.  Every pointer but
// seed_cell is the frame's own; z_out may be what z was read from: element i belongs to thread i % 1024, which has read it by now.
__device__ __forceinline__ void nc_result(char* lds, float* v, const float* rr, int n, int tid, NcBlockSum& block_sum, float* z_out,
                                          float* eigvec, uint8_t* fg, float* margin, int32_t* seed_cell) {
    float* amax = reinterpret_cast<float*>(lds + NC_SLOT_AMAX);        // [16] the waves' largest |v|
    int* aidx = reinterpret_cast<int*>(lds + NC_SLOT_AIDX);            // [16] ... and its cell
    double vs = 0.0;
    float ba = -1.f;
    int bi = INT_MAX;
    for (int i = tid; i < n; i += NC_THREADS) {
        const float zi = v[i];
        const float x = zi * rr[i];
        z_out[i] = zi;
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
        if (better(a2, i2, ba, bi)) {
            ba = a2;
            bi = i2;
        }
    }
    if (block_sum.lane == 0) {
        amax[block_sum.wave] = ba;
        aidx[block_sum.wave] = bi;
    }
    const double avg = block_sum(vs) / (double)n;                       // (its barrier publishes v, amax and aidx)
    ba = amax[0];
    bi = aidx[0];
#pragma unroll
    for (int w = 1; w < NC_WAVES; ++w) {
        const float a2 = amax[w];
        const int i2 = aidx[w];
        if (better(a2, i2, ba, bi)) {
            ba = a2;
            bi = i2;
        }
    }
    if (bi == INT_MAX) bi = 0;                                          // (no |v| compared greater than -1: not a finite input)
    const float sigma = (double)v[bi] > avg ? 1.f : -1.f;
    if (tid == 0) *seed_cell = bi;
    for (int i = tid; i < n; i += NC_THREADS) {
        const float x = v[i];
        const float m = (float)((double)sigma * ((double)x - avg));
        eigvec[i] = sigma * x;
        fg[i] = m > 0.f ? 1 : 0;
        if (margin) margin[i] = m;
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool nc_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// B frames of n cells under an entry's cell limit; fits: what the limit leaves room for, in the message's words
inline int nc_cells_check(const char* who, int B, int n, int max_cells, const char* fits) {
    if (B < 1 || n < 1) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive)", who, B, n);
        return -1;
    }
    if (n > max_cells) {
        dinoseg_set_error("%s: n = %d cells exceed the %d whose %s", who, n, max_cells, fits);
        return -1;
    }
    return 0;
}

// what both iterate entries take
struct NcIterateArgs {
    const void* graph;
    const int32_t* degree;
    int B, n;
    double eps;
    const float* z_in;
    int iters;
    float *z_out, *rho;
    uint8_t* fg;
    float *eigvec, *margin;
    int32_t* seed_cell;
};

// The checks of an iterate entry.  scratch: the entry's scratch (has_scratch) or none; route_checks(): the entry's own checks of its
// launch range, in their place between the cell limit and the pass count, 0 or -1 with the error set.
template <class RouteChecks>
int nc_iterate_check(const char* who, const NcIterateArgs& a, bool has_scratch, const void* scratch, int max_cells, const char* fits,
                     RouteChecks route_checks) {
    if (!a.graph || !a.degree || !a.z_in || !a.z_out || !a.fg || !a.eigvec || !a.seed_cell || (has_scratch && !scratch)) {
        dinoseg_set_error("%s: null pointer (only margin, and rho with iters = 0, are optional)", who);
        return -1;
    }
    if (nc_cells_check(who, a.B, a.n, max_cells, fits)) return -1;
    if (route_checks()) return -1;
    if (a.iters < 0 || a.iters > NC_MAX_ITERS) {
        dinoseg_set_error("%s: iters = %d (0 .. %d)", who, a.iters, NC_MAX_ITERS);
        return -1;
    }
    if (a.iters > 0 && !a.rho) {
        dinoseg_set_error("%s: null pointer (rho is required with iters > 0)", who);
        return -1;
    }
    if (!(a.eps >= 0.0 && a.eps < 1.0)) {
        dinoseg_set_error("%s: eps = %g (inside [0, 1))", who, a.eps);
        return -1;
    }
    if (nc_misaligned(a.graph, 7) || nc_misaligned(a.degree, 3) || nc_misaligned(a.z_in, 3) || nc_misaligned(a.z_out, 3) ||
        nc_misaligned(a.rho, 3) || nc_misaligned(a.eigvec, 3) || nc_misaligned(a.margin, 3) || nc_misaligned(a.seed_cell, 3) ||
        (has_scratch && nc_misaligned(scratch, 15))) {
        dinoseg_set_error("%s: the graph must be 8-byte aligned, a 32-bit array 4-byte aligned%s", who,
                          has_scratch ? ", the scratch 16-byte aligned" : "");
        return -1;
    }
    return 0;
}

}  // namespace dseg
