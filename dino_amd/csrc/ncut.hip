// Normalized cut on a 1-bit patch graph (the spectral bipartition of TokenCut / "Deep Spectral Methods") over the unit rows that
// dinoseg_op_normalize_tokens leaves (fp16 hi + lo planes scaled by 2^10), every frame its own graph.  The rule is stated in full in
// include/dinoseg.h (dinoseg_op_ncut_graph); in short bit(i, j) = <x_i, x_j> > tau, W = eps 11^T + (1 - eps) Bits, and a fixed number of
// lazy power iterations on (I + D^-1/2 W D^-1/2) / 2 with the known top vector deflated give the second eigenvector, whose sign
// pattern around its mean is the partition.  No n x n matrix of floats exists anywhere: the graph is n^2 bits.  No atomics; every
// order of summation is a function of n alone.
//
//   ncut_graph_kernel     one workgroup (4 waves) per (frame, tile of 64 query cells).  The frame's own rows are walked as key blocks
//                         of 64 by the family's pair walk (pair_common.h); wave (qh, kh) multiplies queries 32 qh .. by keys 32 kh ..
//                         into THREE accumulators, lo.hi, hi.lo and hi.hi, combined once per block as (lo.hi + hi.lo) + hi.hi: s_ij
//                         and s_ji are the same bits (the cross terms swap roles, fp32 addition commutes), so the graph is symmetric
//                         bit for bit.  A lane owns one key and 16 queries; one ballot per accumulator register turns 64 decisions
//                         into two half words (two queries x 32 keys), the four waves' halves meet in LDS, and 64 threads store the
//                         block's word of their query and add its popcount to the degree they keep in a register.  A query's whole
//                         row belongs to one workgroup: no atomics.
//   ncut_iterate_kernel   one workgroup of 1024 threads per frame runs every pass in one launch.  z, xv = z r, r and u live in LDS;
//                         the frame's graph is read once per pass and stays in L2 / Infinity Cache.  The weights, the deflation, the
//                         row sums, the global sums and the result are the pieces of ncut_common.h, which states their orders of
//                         summation; this kernel's own are rho (a wave chains its rows in order by fp64 fma, the 16 waves in wave
//                         order) and p = (z + y) / 2.
// (ncut_split.hip runs the same passes with a frame's rows dealt to many workgroups, one launch per pass, bit for bit the same.)
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "ncut_common.h"
#include "pair_common.h"

#include <cmath>

namespace dseg {

namespace {

constexpr int NC_VECTORS = 4;                   // z, xv, r, u
constexpr int NC_MAX_CELLS = nc_cell_limit(NC_VECTORS);
static_assert(NC_MAX_CELLS == 10160, "the one-workgroup entries publish this limit");
constexpr const char* NC_FITS = "vectors fit the LDS of one workgroup";

__global__ __launch_bounds__(256) void ncut_graph_kernel(const uint16_t* __restrict__ planes, int n, int D, float tau, int tiles,
                                                         unsigned long long* __restrict__ graph, int32_t* __restrict__ degree) {
    __shared__ __attribute__((aligned(16))) char nc_lds[PAIR_STAGE];
    __shared__ uint32_t halfw[NC_TILE * 2];                             // [query][key half] of the block just finished
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31;
    const int qh = wave >> 1, kh = wave & 1;
    const int b = (int)blockIdx.x / tiles, i0 = ((int)blockIdx.x - b * tiles) * NC_TILE;
    const int nkb = (n + 63) >> 6;
    const uint16_t* fr = planes + (size_t)b * 2 * n * D;                // the frame's hi plane [n][D]; its lo plane follows
    const size_t p_lo = (size_t)n * D;

    // the tile's query rows as the walk stages them (pair_common.h); a row past the last cell re-reads a real one and is never stored,
    // a key row past n re-reads a real one and its decision is forced to 0
    const size_t qrow[2] = {(size_t)min(i0 + pair_stage_row(0), n - 1) * D, (size_t)min(i0 + pair_stage_row(1), n - 1) * D};
    auto key_row = [&](int j) { return (size_t)min(j, n - 1) * D; };
    // lane l < 32 carries the half word of query l of the wave's half: accumulator register my_r of lane half my_h is that query
    const int my_r = (lr & 3) + 4 * (lr >> 3), my_h = (lr >> 2) & 1;

    const int W = nkb;
    const int qi = i0 + tid;                                            // threads 0 .. 63: the query whose words they store
    int cnt = 0;
    auto flush = [&](int kb) {
        if (tid < NC_TILE && qi < n) {
            const unsigned long long word = (unsigned long long)halfw[tid * 2] | ((unsigned long long)halfw[tid * 2 + 1] << 32);
            graph[((size_t)b * n + qi) * W + kb] = word;
            cnt += __popcll(word);
        }
    };

    f32x16 acc_lh, acc_hl, acc_hh;
    // (the walk's first barrier of a block completes halfw of the block before)
    auto flush_previous = [&](int kb) {
        if (kb > 0) flush(kb - 1);
    };
    auto zero = [&]() {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc_lh[r] = 0.f;
            acc_hl[r] = 0.f;
            acc_hh[r] = 0.f;
        }
    };
    auto slice = [&](bf16x8 qhi, bf16x8 qlo, bf16x8 khi, bf16x8 klo) {
        acc_lh = mfma32f<FMT_FP16>(qlo, khi, acc_lh);
        acc_hl = mfma32f<FMT_FP16>(qhi, klo, acc_hl);
        acc_hh = mfma32f<FMT_FP16>(qhi, khi, acc_hh);
    };
    // the block's decisions: register r of this lane is query acc_row(r, lh) of the wave's half, key lr of the wave's half
    auto decide = [&](int kb) {
        const bool kvalid = kb * 64 + kh * 32 + lr < n;                 // (pad bits are zero)
        uint32_t mine = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = ((acc_lh[r] + acc_hl[r]) + acc_hh[r]) * PAIR_UNSCALE + 0.f;    // (+ 0: a negative zero becomes the positive one)
            const unsigned long long m = __ballot(kvalid && s > tau);   // low half: query acc_row(r, 0), high half: acc_row(r, 1)
            if (r == my_r) mine = my_h ? (uint32_t)(m >> 32) : (uint32_t)m;
        }
        if (lane < 32) halfw[(qh * 32 + lane) * 2 + kh] = mine;         // (read after the next barrier, rewritten after the one after it)
    };
    pair_walk(nc_lds, fr, p_lo, qrow, fr, p_lo, nkb, D >> 6, key_row, flush_previous, zero, slice, decide);
    __syncthreads();
    flush(nkb - 1);
    if (tid < NC_TILE && qi < n) degree[(size_t)b * n + qi] = cnt;
}

// z_in may be z_out: element i of both belongs to thread i % 1024, which reads at the start and writes at the end
__global__ __launch_bounds__(NC_THREADS) void ncut_iterate_kernel(const unsigned long long* __restrict__ graph,
                                                                  const int32_t* __restrict__ degree, int n, double eps, const float* z_in,
                                                                  int iters, float* z_out, float* __restrict__ rho,
                                                                  uint8_t* __restrict__ fg, float* __restrict__ eigvec,
                                                                  float* __restrict__ margin, int32_t* __restrict__ seed_cell) {
    extern __shared__ __attribute__((aligned(16))) char nci_lds[];     // the slots (ncut_common.h), then the vectors
    float* z = reinterpret_cast<float*>(nci_lds + NC_FIXED_BYTES);     // [n] the iterate
    float* xv = z + n;                                                  // [n] z r (a word's pad lanes read past it, inside the allocation; never selected)
    float* rr = xv + n;                                                 // [n] r = 1 / sqrt(d)
    float* u = rr + n;                                                  // [n] the known top vector sqrt(d) / ||sqrt(d)||
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, W = (n + 63) >> 6;
    const size_t base = (size_t)b * n;
    NcBlockSum block_sum{reinterpret_cast<double*>(nci_lds), 0, lane, wave};

    for (int i = tid; i < n; i += NC_THREADS) z[i] = z_in[base + i];
    nc_weights(degree + base, n, eps, rr, u, tid, block_sum);
    nc_deflate_normalise(z, u, n, tid, block_sum);
    for (int t = 0; t < iters; ++t) {
        double S = 0.0;
        for (int i = tid; i < n; i += NC_THREADS) {
            const float x = z[i] * rr[i];
            xv[i] = x;
            S += (double)x;
        }
        S = block_sum(S);
        const double epsS = eps * S, om = 1.0 - eps;
        double rp = 0.0;                                                // the wave's share of rho, its rows in order
        nc_row_walk(graph + base * W, W, 0, n, xv, lane, wave, [&](int i, float ti) {
            const float zi = z[i];
            const float y = (float)((double)rr[i] * (epsS + om * (double)ti));
            rp = fma((double)zi, (double)y, rp);
            if (lane == 0) z[i] = 0.5f * (zi + y);
        });
        {                                                               // rho: the waves' shares in wave order
            double* s = block_sum.next();
            if (lane == 0) s[wave] = rp;
            __syncthreads();                                            // ... and the rows' p are visible to their threads
            if (tid == 0) {
                double r = s[0];
#pragma unroll
                for (int w = 1; w < NC_WAVES; ++w) r += s[w];
                rho[(size_t)b * iters + t] = (float)r;
            }
        }
        nc_deflate_normalise(z, u, n, tid, block_sum);
        // the next pass prepares its input as a fresh call would prepare z_out: T chained calls and one call of T passes are the same bits
        if (t + 1 < iters) nc_deflate_normalise(z, u, n, tid, block_sum);
    }
    nc_result(nci_lds, z, rr, n, tid, block_sum, z_out + base, eigvec + base, fg + base, margin ? margin + base : nullptr, seed_cell + b);
}

int nc_grid_check(const char* who, int B, int n) {
    if ((long long)B * ((n + NC_TILE - 1) / NC_TILE) > NC_MAX_GRID) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells exceed the launch range", who, B, n);
        return -1;
    }
    return 0;
}

}  // namespace

int ncut_max_cells() { return NC_MAX_CELLS; }

long long ncut_graph_bytes(int B, int n) {
    if (B < 1 || n < 1 || n > NC_MAX_CELLS || (long long)B * ((n + NC_TILE - 1) / NC_TILE) > NC_MAX_GRID) return -1;
    return 8ll * B * n * ((n + 63) / 64);
}

namespace {

// the graph launch under the cell limit of the entry `who`: the kernel itself has no limit of its own
int nc_launch_graph(const char* who, int max_cells, const void* planes, int B, int n, int D, double tau, void* graph, int32_t* degree,
                    hipStream_t s) {
    if (!planes || !graph || !degree) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (pair_width_check(who, D)) return -1;
    if (nc_cells_check(who, B, n, max_cells, NC_FITS) || nc_grid_check(who, B, n)) return -1;
    if (!std::isfinite(tau) || !(tau > -1.0 && tau < 1.0)) {
        dinoseg_set_error("%s: tau = %g (finite, inside (-1, 1))", who, tau);
        return -1;
    }
    if (nc_misaligned(planes, 15) || nc_misaligned(graph, 7) || nc_misaligned(degree, 3)) {
        dinoseg_set_error("%s: planes must be 16-byte aligned, the graph 8-byte aligned, the degree 4-byte aligned", who);
        return -1;
    }
    const int tiles = (n + NC_TILE - 1) / NC_TILE;
    hipLaunchKernelGGL(ncut_graph_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, s, reinterpret_cast<const uint16_t*>(planes), n, D,
                       (float)tau, tiles, reinterpret_cast<unsigned long long*>(graph), degree);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_ncut_graph(const void* planes, int B, int n, int D, double tau, void* graph, int32_t* degree, hipStream_t s) {
    return nc_launch_graph("dinoseg_op_ncut_graph", NC_MAX_CELLS, planes, B, n, D, tau, graph, degree, s);
}

int launch_ncut_graph_split(const void* planes, int B, int n, int D, double tau, void* graph, int32_t* degree, hipStream_t s) {
    return nc_launch_graph("dinoseg_op_ncut_graph_split", ncut_split_max_cells(), planes, B, n, D, tau, graph, degree, s);
}

int launch_ncut_iterate(const void* graph, const int32_t* degree, int B, int n, double eps, const float* z_in, int iters, float* z_out,
                        float* rho, uint8_t* fg, float* eigvec, float* margin, int32_t* seed_cell, hipStream_t s) {
    const char* who = "dinoseg_op_ncut_iterate";
    const NcIterateArgs args{graph, degree, B, n, eps, z_in, iters, z_out, rho, fg, eigvec, margin, seed_cell};
    if (nc_iterate_check(who, args, false, nullptr, NC_MAX_CELLS, NC_FITS, [&]() { return nc_grid_check(who, B, n); })) return -1;
    const size_t lds = (size_t)NC_FIXED_BYTES + NC_PAD_BYTES + (size_t)n * 4 * NC_VECTORS;
    if (lds > NC_DEFAULT_LDS_BYTES) {
        static PerDeviceOnce once;
        if (once.first()) {
            DSEG_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ncut_iterate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               NC_LDS_BYTES));
            once.mark();
        }
    }
    hipLaunchKernelGGL(ncut_iterate_kernel, dim3((unsigned)B), dim3(NC_THREADS), lds, s, reinterpret_cast<const unsigned long long*>(graph),
                       degree, n, eps, z_in, iters, z_out, rho, fg, eigvec, margin, seed_cell);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
