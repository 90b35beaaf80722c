// Normalized cut on a 1-bit patch graph (the spectral bipartition of TokenCut / "Deep Spectral Methods") over the unit rows that
// dinoseg_op_normalize_tokens leaves (fp16 hi + lo planes scaled by 2^10), every frame its own graph.  The rule is stated in full in
// include/dinoseg.h (dinoseg_op_ncut_graph); in short bit(i, j) = <x_i, x_j> > tau, W = eps 11^T + (1 - eps) Bits, and a fixed number of
// lazy power iterations on (I + D^-1/2 W D^-1/2) / 2 with the known top vector deflated give the second eigenvector, whose sign
// pattern around its mean is the partition.  No n x n matrix of floats exists anywhere: the graph is n^2 bits.  No atomics; every
// order of summation is a function of n alone.
//
//   ncut_graph_kernel     one workgroup (4 waves) per (frame, tile of 64 query cells).  The frame's own rows are walked as key blocks
//                         of 64; per block and 64-wide slice of D the query tile and the key block (hi and lo, 4 x 8 KiB, 128-byte
//                         rows under the library's swizzle) are staged in LDS -- the next slice's global loads are in flight under
//                         the current slice's MFMAs -- and wave (qh, kh) multiplies queries 32 qh .. by keys 32 kh .. on
//                         v_mfma_f32_32x32x16_f16 into THREE accumulators, lo.hi, hi.lo and hi.hi, combined once per block as
//                         (lo.hi + hi.lo) + hi.hi: s_ij and s_ji are the same bits (the cross terms swap roles, fp32 addition
//                         commutes), so the graph is symmetric bit for bit.  A lane owns one key and 16 queries; one ballot per
//                         accumulator register turns 64 decisions into two half words (two queries x 32 keys), the four waves' halves
//                         meet in LDS, and 64 threads store the block's word of their query and add its popcount to the degree they
//                         keep in a register.  A query's whole row belongs to one workgroup: no atomics.
//   ncut_iterate_kernel   one workgroup of 1024 threads per frame runs every pass in one launch.  z, xv = z r, r and u live in LDS.
//                         The row sums: rows are dealt to the 16 waves, a row's words are wave-uniform (scalar loads; the frame's
//                         graph is read once per pass and stays in L2 / Infinity Cache), lane l owns keys l, l + 64, ...: per word one
//                         conflict-free ds_read_b32 of xv[64 w + l] (shared by the two rows a wave walks at a time) and one select on
//                         the word itself as the lane mask, added in ascending w; the 64 lanes meet in an xor tree.  The global sums (S, rho, <u, z>, ||q||^2, the mean) are fp64:
//                         thread t adds its cells t, t + 1024, ... in order, an xor tree per wave, the 16 waves in wave order.
// (ncut_split.hip runs the same passes with a frame's rows dealt to many workgroups, one launch per pass, bit for bit the same.)
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"

#include <climits>
#include <cmath>

namespace dseg {

namespace {

constexpr int NC_TILE = 64;                     // query cells of a graph workgroup
constexpr int NC_STAGE = 32768;                 // Qhi, Qlo, Khi, Klo: 64 rows x 128 B each
constexpr float NC_UNSCALE = 0x1p-20f;          // planes carry 2^10 x: products 2^20 <x_i, x_j>
constexpr int NC_THREADS = 1024, NC_WAVES = NC_THREADS / 64;
constexpr int NC_LDS_BYTES = 160 * 1024;        // the CU's whole LDS
constexpr int NC_FIXED_BYTES = 1024;            // the reduction slots: 2 x 16 fp64, 16 fp32 + 16 int32
constexpr int NC_VECTORS = 4;                   // z, xv, r, u
constexpr int NC_PAD_BYTES = 256;               // the last word's pad lanes read up to 63 floats past a vector: they stay inside
constexpr int NC_MAX_CELLS = (NC_LDS_BYTES - NC_FIXED_BYTES - NC_PAD_BYTES) / (4 * NC_VECTORS);      // 10 160
constexpr int NC_DEFAULT_LDS_BYTES = 64 * 1024; // beyond it a launch needs the opt-in
constexpr int NC_MAX_ITERS = 4096;
constexpr long long NC_MAX_GRID = 0x7fffffffll;

__global__ __launch_bounds__(256) void ncut_graph_kernel(const uint16_t* __restrict__ planes, int n, int D, float tau, int tiles,
                                                         unsigned long long* __restrict__ graph, int32_t* __restrict__ degree) {
    __shared__ __attribute__((aligned(16))) char nc_lds[NC_STAGE];
    __shared__ uint32_t halfw[NC_TILE * 2];                             // [query][key half] of the block just finished
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int qh = wave >> 1, kh = wave & 1;
    const int b = (int)blockIdx.x / tiles, i0 = ((int)blockIdx.x - b * tiles) * NC_TILE;
    const int nkb = (n + 63) >> 6, ndc = D >> 6, total = nkb * ndc;
    const uint16_t* fr = planes + (size_t)b * 2 * n * D;                // the frame's hi plane [n][D]; its lo plane follows
    const size_t p_lo = (size_t)n * D;

    // staging: thread t moves 16 bytes (chunk t & 7) of rows (t >> 3) and (t >> 3) + 32 of each of the four tiles
    const int srow = tid >> 3, schunk = tid & 7;
    size_t qoff[2];
    int soff[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = srow + 32 * h;
        qoff[h] = (size_t)min(i0 + row, n - 1) * D + schunk * 8;        // (a row past the last cell re-reads a real one; never stored)
        soff[h] = tile_off_bytes(row, schunk);
    }
    uint4 g_qh0, g_qh1, g_ql0, g_ql1, g_kh0, g_kh1, g_kl0, g_kl1;         // the slice in flight (named: an array would live in scratch)
    auto ld16 = [](const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); };
    auto fetch = [&](int it) {
        const int kb = it / ndc;
        const size_t dofs = (size_t)(it - kb * ndc) * 64;
        // (a key row past n re-reads a real one; its decision is forced to 0)
        const size_t k0 = (size_t)min(kb * 64 + srow, n - 1) * D + schunk * 8 + dofs;
        const size_t k1 = (size_t)min(kb * 64 + srow + 32, n - 1) * D + schunk * 8 + dofs;
        g_qh0 = ld16(fr + qoff[0] + dofs);
        g_qh1 = ld16(fr + qoff[1] + dofs);
        g_ql0 = ld16(fr + p_lo + qoff[0] + dofs);
        g_ql1 = ld16(fr + p_lo + qoff[1] + dofs);
        g_kh0 = ld16(fr + k0);
        g_kh1 = ld16(fr + k1);
        g_kl0 = ld16(fr + p_lo + k0);
        g_kl1 = ld16(fr + p_lo + k1);
    };

    // fragment addresses: row lr of the wave's half, chunk 2 s + lh of the 128-byte row
    int fq[4], fk[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        fq[s] = tile_off_bytes(qh * 32 + lr, s * 2 + lh);
        fk[s] = 16384 + tile_off_bytes(kh * 32 + lr, s * 2 + lh);
    }
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
    fetch(0);
    for (int it = 0; it < total; ++it) {
        const int kb = it / ndc, dc = it - kb * ndc;
        __syncthreads();                                                // everyone is done reading the previous slice; halfw is complete
        if (dc == 0 && kb > 0) flush(kb - 1);
        *reinterpret_cast<uint4*>(nc_lds + soff[0]) = g_qh0;
        *reinterpret_cast<uint4*>(nc_lds + soff[1]) = g_qh1;
        *reinterpret_cast<uint4*>(nc_lds + 8192 + soff[0]) = g_ql0;
        *reinterpret_cast<uint4*>(nc_lds + 8192 + soff[1]) = g_ql1;
        *reinterpret_cast<uint4*>(nc_lds + 16384 + soff[0]) = g_kh0;
        *reinterpret_cast<uint4*>(nc_lds + 16384 + soff[1]) = g_kh1;
        *reinterpret_cast<uint4*>(nc_lds + 24576 + soff[0]) = g_kl0;
        *reinterpret_cast<uint4*>(nc_lds + 24576 + soff[1]) = g_kl1;
        __syncthreads();
        if (it + 1 < total) fetch(it + 1);
        if (dc == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc_lh[r] = 0.f;
                acc_hl[r] = 0.f;
                acc_hh[r] = 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bf16x8 qhi = lds_frag(nc_lds + fq[s]), qlo = lds_frag(nc_lds + 8192 + fq[s]);
            const bf16x8 khi = lds_frag(nc_lds + fk[s]), klo = lds_frag(nc_lds + 8192 + fk[s]);
            acc_lh = mfma32f<FMT_FP16>(qlo, khi, acc_lh);
            acc_hl = mfma32f<FMT_FP16>(qhi, klo, acc_hl);
            acc_hh = mfma32f<FMT_FP16>(qhi, khi, acc_hh);
        }
        if (dc != ndc - 1) continue;
        // the block's decisions: register r of this lane is query acc_row(r, lh) of the wave's half, key lr of the wave's half
        const bool kvalid = kb * 64 + kh * 32 + lr < n;                 // (pad bits are zero)
        uint32_t mine = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = ((acc_lh[r] + acc_hl[r]) + acc_hh[r]) * NC_UNSCALE + 0.f;      // (+ 0: a negative zero becomes the positive one)
            const unsigned long long m = __ballot(kvalid && s > tau);   // low half: query acc_row(r, 0), high half: acc_row(r, 1)
            if (r == my_r) mine = my_h ? (uint32_t)(m >> 32) : (uint32_t)m;
        }
        if (lane < 32) halfw[(qh * 32 + lane) * 2 + kh] = mine;         // (read after the next barrier, rewritten after the one after it)
    }
    __syncthreads();
    flush(nkb - 1);
    if (tid < NC_TILE && qi < n) degree[(size_t)b * n + qi] = cnt;
}

// x where the lane's bit of the wave-uniform word is set, else 0: the word itself is the lane mask of one select
__device__ __forceinline__ float nc_pick(unsigned long long word, float x) {
    float r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(word));
    return r;
}

__device__ __forceinline__ double nc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);             // (xor tree: every lane holds the same bits)
    return v;
}

// z_in may be z_out: element i of both belongs to thread i % 1024, which reads at the start and writes at the end
__global__ __launch_bounds__(NC_THREADS) void ncut_iterate_kernel(const unsigned long long* __restrict__ graph,
                                                                  const int32_t* __restrict__ degree, int n, double eps, const float* z_in,
                                                                  int iters, float* z_out, float* __restrict__ rho,
                                                                  uint8_t* __restrict__ fg, float* __restrict__ eigvec,
                                                                  float* __restrict__ margin, int32_t* __restrict__ seed_cell) {
    extern __shared__ __attribute__((aligned(16))) char nci_lds[];
    double* slots = reinterpret_cast<double*>(nci_lds);                // [2][16]: the waves' sums, two uses alternating
    float* amax = reinterpret_cast<float*>(nci_lds + 256);             // [16] the waves' largest |v|
    int* aidx = reinterpret_cast<int*>(nci_lds + 320);                 // [16] ... and its cell
    float* z = reinterpret_cast<float*>(nci_lds + NC_FIXED_BYTES);     // [n] the iterate
    float* xv = z + n;                                                  // [n] z r (a word's pad lanes read past it, inside the allocation; never selected)
    float* rr = xv + n;                                                 // [n] r = 1 / sqrt(d)
    float* u = rr + n;                                                  // [n] the known top vector sqrt(d) / ||sqrt(d)||
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, W = (n + 63) >> 6;
    const size_t base = (size_t)b * n;
    int flip = 0;
    // the global sum of one value per thread: xor tree per wave, the waves in wave order; the barrier inside also publishes LDS writes
    auto block_sum = [&](double v) {
        double* s = slots + 16 * flip;
        flip ^= 1;
        v = nc_wave_sum(v);
        if (lane == 0) s[wave] = v;
        __syncthreads();
        double t = s[0];
#pragma unroll
        for (int w = 1; w < NC_WAVES; ++w) t += s[w];
        return t;
    };

    // r, u and the start vector
    double part = 0.0;
    for (int i = tid; i < n; i += NC_THREADS) {
        const int c = degree[base + i];
        const float d = (float)(eps * (double)(n - c) + (double)c);
        rr[i] = d > 0.f ? (float)(1.0 / sqrt((double)d)) : 0.f;
        u[i] = d;
        z[i] = z_in[base + i];
        part += (double)d;
    }
    const double dsum = block_sum(part);
    const double dnorm = sqrt(dsum);
    for (int i = tid; i < n; i += NC_THREADS) u[i] = dnorm > 0.0 ? (float)(sqrt((double)u[i]) / dnorm) : 0.f;

    // z <- (z - <u, z> u) / || . ||; every element is its thread's own
    auto deflate_normalise = [&]() {
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
    };

    deflate_normalise();
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
        auto finish = [&](int i, float ti) {                            // (ti: the xor tree left the same bits in every lane)
            const float zi = z[i];
            const float y = (float)((double)rr[i] * (epsS + om * (double)ti));
            rp = fma((double)zi, (double)y, rp);
            if (lane == 0) z[i] = 0.5f * (zi + y);
        };
        // two rows of the wave at a time, i and i + 16: one read of xv serves both, and two streams of words are in flight
        for (int i = wave; i < n; i += 2 * NC_WAVES) {
            const bool two = i + NC_WAVES < n;
            const unsigned long long* row_a = graph + (base + i) * W;
            const unsigned long long* row_b = two ? row_a + (size_t)NC_WAVES * W : row_a;   // (no second row: the first again, unused)
            float acc_a = 0.f, acc_b = 0.f;
            int w = 0;
            if (W >= 8) {                                               // eight words at a time, the next eight in flight
                unsigned long long cur_a[8], cur_b[8], nxt_a[8], nxt_b[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    cur_a[k] = row_a[k];
                    cur_b[k] = row_b[k];
                }
                for (; w + 8 <= W; w += 8) {
                    const int ahead = w + 16 <= W ? w + 8 : 0;          // (past the last group: re-read the first)
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
        {                                                               // rho: the waves' shares in wave order
            double* s = slots + 16 * flip;
            flip ^= 1;
            if (lane == 0) s[wave] = rp;
            __syncthreads();                                            // ... and the rows' p are visible to their threads
            if (tid == 0) {
                double r = s[0];
#pragma unroll
                for (int w = 1; w < NC_WAVES; ++w) r += s[w];
                rho[(size_t)b * iters + t] = (float)r;
            }
        }
        deflate_normalise();
        // the next pass prepares its input as a fresh call would prepare z_out: T chained calls and one call of T passes are the same bits
        if (t + 1 < iters) deflate_normalise();
    }

    // the result: v = z r, its mean, the seed, the sign, the partition
    double vs = 0.0;
    float ba = -1.f;
    int bi = INT_MAX;
    for (int i = tid; i < n; i += NC_THREADS) {
        const float v = z[i] * rr[i];
        xv[i] = v;
        vs += (double)v;
        const float a = fabsf(v);
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
    const double avg = block_sum(vs) / (double)n;                       // (its barrier publishes xv, amax and aidx)
    ba = amax[0];
    bi = aidx[0];
#pragma unroll
    for (int w = 1; w < NC_WAVES; ++w) {
        const float a2 = amax[w];
        const int i2 = aidx[w];
        if (a2 > ba || (a2 == ba && i2 < bi)) {
            ba = a2;
            bi = i2;
        }
    }
    if (bi == INT_MAX) bi = 0;                                          // (no |v| compared greater than -1: not a finite input)
    const float sigma = (double)xv[bi] > avg ? 1.f : -1.f;
    if (tid == 0) seed_cell[b] = bi;
    for (int i = tid; i < n; i += NC_THREADS) {
        const float v = xv[i];
        const float m = (float)((double)sigma * ((double)v - avg));
        z_out[base + i] = z[i];
        eigvec[base + i] = sigma * v;
        fg[base + i] = m > 0.f ? 1 : 0;
        if (margin) margin[base + i] = m;
    }
}

bool nc_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int nc_shape_check(const char* who, int B, int n, int max_cells = NC_MAX_CELLS) {
    if (B < 1 || n < 1) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive)", who, B, n);
        return -1;
    }
    if (n > max_cells) {
        dinoseg_set_error("%s: n = %d cells exceed the %d whose vectors fit the LDS of one workgroup", who, n, max_cells);
        return -1;
    }
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
    if (D < 64 || D % 64 != 0 || D > 8192) {
        dinoseg_set_error("%s: width D = %d (a multiple of 64 up to 8192)", who, D);
        return -1;
    }
    if (nc_shape_check(who, B, n, max_cells)) return -1;
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
    if (!graph || !degree || !z_in || !z_out || !fg || !eigvec || !seed_cell) {
        dinoseg_set_error("%s: null pointer (only margin, and rho with iters = 0, are optional)", who);
        return -1;
    }
    if (nc_shape_check(who, B, n)) return -1;
    if (iters < 0 || iters > NC_MAX_ITERS) {
        dinoseg_set_error("%s: iters = %d (0 .. %d)", who, iters, NC_MAX_ITERS);
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
    if (nc_misaligned(graph, 7) || nc_misaligned(degree, 3) || nc_misaligned(z_in, 3) || nc_misaligned(z_out, 3) || nc_misaligned(rho, 3) ||
        nc_misaligned(eigvec, 3) || nc_misaligned(margin, 3) || nc_misaligned(seed_cell, 3)) {
        dinoseg_set_error("%s: the graph must be 8-byte aligned, a 32-bit array 4-byte aligned", who);
        return -1;
    }
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
