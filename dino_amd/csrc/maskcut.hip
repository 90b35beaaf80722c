// Multi-object discovery: K rounds of the normalized cut with the found object painted out between rounds (MaskCut; the rule:
// include/dinoseg.h, dinoseg_op_maskcut).  The cut (ncut_split.hip) and the components (components.hip) run unchanged; this file owns
// the glue that makes a round a function of the previous one on the device, ordered by the stream alone: no cooperative launch, no
// grid barrier, no flag, no floating-point atomic, no host synchronisation.
//
//   mc_init_kernel     before round 0: alive = every cell (pad bits zero), score channel 0 = 0.
//   mc_mask_kernel     one wave per row of the graph: row i <- alive_i ? row i & alive : 0 in place, lane l owns words l, l + 64, ..
//                      (one 8-byte load and store per lane and step, 512 contiguous bytes per wave); the popcounts meet in an xor
//                      tree and lane 0 writes degree[i].  A dead row is stored as zeros without being read.
//   mc_round_kernel    one thread per cell: the candidate map fg && alive as int32 for the components, and the round's fg / margin /
//                      eigvec / seed_cell / rho from the entry's working arrays [B][..] into slot t of the caller's [B][K][..].
//   mc_select_kernel   one workgroup of 1024 threads per frame: wave w owns words w, w + 16, .. of the cell bits, lane l cell 64 w + l.
//                      The component of the seed is a ballot per word: cells, the score channel, alive &= ~ballot by lane 0 (the one
//                      writer of the word), the area a popcount; the box is min / max per lane, an xor tree per wave, the 16 waves
//                      through LDS.  Integer and sign operations only.
//   mc_count_kernel    count[b] = the number of rounds with found = 1.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "ncut_common.h"

#include <algorithm>

namespace dseg {

namespace {

constexpr int MC_THREADS = 256, MC_WAVES = MC_THREADS / 64;
constexpr int MC_SEL_THREADS = 1024, MC_SEL_WAVES = MC_SEL_THREADS / 64;
constexpr int MC_MAX_ROUNDS = DINOSEG_MASKCUT_MAX_OBJECTS;

__device__ __forceinline__ int mc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int mc_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int mc_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// per = the workgroups of a frame, over max(n, W) elements
__global__ __launch_bounds__(MC_THREADS) void mc_init_kernel(int n, int W, int K, int per, unsigned long long* __restrict__ alive,
                                                             float* __restrict__ score) {
    const int b = (int)blockIdx.x / per;
    const int e = ((int)blockIdx.x - b * per) * MC_THREADS + (int)threadIdx.x;
    if (e < W) {
        const int left = n - 64 * e;                                    // (>= 1: W = ceil(n / 64))
        alive[(size_t)b * W + e] = left >= 64 ? ~0ull : (1ull << left) - 1ull;
    }
    if (e < n) score[((size_t)b * n + e) * (size_t)(K + 1)] = 0.f;
}

// rows = B n of them, one per wave
__global__ __launch_bounds__(MC_THREADS) void mc_mask_kernel(unsigned long long* __restrict__ graph, int32_t* __restrict__ degree,
                                                             const unsigned long long* __restrict__ alive, int n, int W, long long rows) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * MC_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (int)(row / n), i = (int)(row - (long long)b * n);
    const unsigned long long* al = alive + (size_t)b * W;
    unsigned long long* g = graph + (size_t)row * W;
    const bool on = (al[i >> 6] >> (i & 63)) & 1ull;                    // (wave-uniform)
    int cnt = 0;
    if (on) {
        for (int w = lane; w < W; w += 64) {
            const unsigned long long v = g[w] & al[w];
            g[w] = v;
            cnt += __popcll(v);
        }
        cnt = mc_wave_sum(cnt);
    } else {
        for (int w = lane; w < W; w += 64) g[w] = 0ull;
    }
    if (lane == 0) degree[row] = cnt;
}

// per = the workgroups of a frame, over max(n, iters) elements; the *_w arrays are the round's [B][..], the others the caller's [B][K][..]
__global__ __launch_bounds__(MC_THREADS) void mc_round_kernel(int n, int W, int K, int t, int iters, int per,
                                                              const unsigned long long* __restrict__ alive,
                                                              const uint8_t* __restrict__ fg_w, const float* __restrict__ margin_w,
                                                              const float* __restrict__ eigvec_w, const int32_t* __restrict__ seed_w,
                                                              const float* __restrict__ rho_w, int32_t* __restrict__ cand,
                                                              uint8_t* __restrict__ fg, float* __restrict__ margin,
                                                              float* __restrict__ eigvec, int32_t* __restrict__ seed_cell,
                                                              float* __restrict__ rho) {
    const int b = (int)blockIdx.x / per;
    const int e = ((int)blockIdx.x - b * per) * MC_THREADS + (int)threadIdx.x;
    const size_t slot = (size_t)b * K + t;
    if (e < n) {
        const size_t in = (size_t)b * n + e, out = slot * n + e;
        const uint8_t f = fg_w[in];
        const bool on = (alive[(size_t)b * W + (e >> 6)] >> (e & 63)) & 1ull;
        cand[in] = (f != 0 && on) ? 1 : 0;
        fg[out] = f;
        margin[out] = margin_w[in];
        eigvec[out] = eigvec_w[in];
    }
    if (e < iters) rho[slot * iters + e] = rho_w[(size_t)b * iters + e];
    if (e == 0) seed_cell[slot] = seed_w[b];
}

__global__ __launch_bounds__(MC_SEL_THREADS) void mc_select_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ fg,
                                                                   const float* __restrict__ margin,
                                                                   const int32_t* __restrict__ seed_cell, unsigned long long* alive,
                                                                   int n, int wp, int W, int K, int t, uint8_t* __restrict__ cells,
                                                                   uint8_t* __restrict__ found, int32_t* __restrict__ area,
                                                                   int32_t* __restrict__ box, float* __restrict__ score) {
    __shared__ int red[5][MC_SEL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t base = (size_t)b * n, slot = (size_t)b * K + t;
    unsigned long long* al = alive + (size_t)b * W;
    const int seed = seed_cell[b];
    int k = -1;
    if (seed >= 0 && seed < n && fg[base + seed] != 0 && ((al[seed >> 6] >> (seed & 63)) & 1ull)) k = ids[base + seed];
    __syncthreads();                                                    // (every thread has read the seed's alive bit before a word changes)
    int cnt = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int w = wave; w < W; w += MC_SEL_WAVES) {
        const int i = 64 * w + lane;
        const bool in = i < n;
        const bool c = in && k >= 0 && ids[base + (in ? i : 0)] == k;
        const unsigned long long m = __ballot(c);
        if (in) {
            const float mg = margin[base + i];
            cells[slot * n + i] = c ? 1 : 0;
            score[(base + i) * (size_t)(K + 1) + t + 1] = c ? mg : __uint_as_float(__float_as_uint(mg) | 0x80000000u);
        }
        if (c) {
            const int y = i / wp, x = i - y * wp;
            x0 = min(x0, x);
            y0 = min(y0, y);
            x1 = max(x1, x);
            y1 = max(y1, y);
        }
        if (lane == 0 && m) al[w] &= ~m;                                // (the word's one writer)
        cnt += __popcll(m);                                             // (wave-uniform)
    }
    x0 = mc_wave_min(x0);
    y0 = mc_wave_min(y0);
    x1 = mc_wave_max(x1);
    y1 = mc_wave_max(y1);
    if (lane == 0) {
        red[0][wave] = cnt;
        red[1][wave] = x0;
        red[2][wave] = y0;
        red[3][wave] = x1;
        red[4][wave] = y1;
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0;
#pragma unroll
        for (int w = 0; w < MC_SEL_WAVES; ++w) {
            a += red[0][w];
            x0 = min(x0, red[1][w]);
            y0 = min(y0, red[2][w]);
            x1 = max(x1, red[3][w]);
            y1 = max(y1, red[4][w]);
        }
        const bool hit = k >= 0;                                        // (then the seed itself is one of the cells: a >= 1)
        found[slot] = hit ? 1 : 0;
        area[slot] = hit ? a : 0;
        box[4 * slot + 0] = hit ? x0 : 0;
        box[4 * slot + 1] = hit ? y0 : 0;
        box[4 * slot + 2] = hit ? x1 + 1 : 0;
        box[4 * slot + 3] = hit ? y1 + 1 : 0;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const uint8_t* __restrict__ found, int B, int K, int32_t* __restrict__ count) {
    const int b = (int)blockIdx.x * MC_THREADS + (int)threadIdx.x;
    if (b >= B) return;
    int c = 0;
    for (int t = 0; t < K; ++t) c += found[(size_t)b * K + t] != 0;
    count[b] = c;
}

bool mc_misaligned(const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; }

// B frames of hp x wp cells that both the split cut and the components accept
bool mc_shape_ok(int B, int hp, int wp) {
    return components_scratch_bytes(B, hp, wp) >= 0 && ncut_split_scratch_bytes(B, hp * wp) >= 0;
}

long long mc_up16(long long v) { return (v + 15) & ~15ll; }

// the entry's scratch, every part 16-byte aligned
struct McLayout {
    long long split, cc, small, alive, cand, ids, z, fg, margin, eigvec, seed, rho, bytes;
};
McLayout mc_layout(int B, int hp, int wp) {
    const long long n = (long long)hp * wp, W = (n + 63) / 64, cells = (long long)B * n;
    McLayout L;
    long long at = 0;
    auto take = [&](long long bytes) {
        const long long here = at;
        at = mc_up16(at + bytes);
        return here;
    };
    L.split = take(ncut_split_scratch_bytes(B, (int)n));
    L.cc = take(components_scratch_bytes(B, hp, wp));
    L.small = take(4ll * 9 * B);                                        // count, status, first, label, area [B] and box [B][4] of the components
    L.alive = take(8ll * B * W);
    L.cand = take(4 * cells);
    L.ids = take(4 * cells);
    L.z = take(4 * cells);
    L.fg = take(cells);
    L.margin = take(4 * cells);
    L.eigvec = take(4 * cells);
    L.seed = take(4ll * B);
    L.rho = take(4ll * B * NC_MAX_ITERS);
    L.bytes = at;
    return L;
}

int mc_launch_mask(unsigned long long* graph, int32_t* degree, const unsigned long long* alive, int B, int n, hipStream_t s) {
    const long long rows = (long long)B * n;                            // (< 2^31: the shape checks)
    hipLaunchKernelGGL(mc_mask_kernel, dim3((unsigned)((rows + MC_WAVES - 1) / MC_WAVES)), dim3(MC_THREADS), 0, s, graph, degree, alive, n,
                       (n + 63) >> 6, rows);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int mc_launch_select(const int32_t* ids, const uint8_t* fg, const float* margin, const int32_t* seed_cell, unsigned long long* alive, int B,
                     int n, int wp, int K, int t, uint8_t* cells, uint8_t* found, int32_t* area, int32_t* box, float* score, hipStream_t s) {
    hipLaunchKernelGGL(mc_select_kernel, dim3((unsigned)B), dim3(MC_SEL_THREADS), 0, s, ids, fg, margin, seed_cell, alive, n, wp,
                       (n + 63) >> 6, K, t, cells, found, area, box, score);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

long long maskcut_scratch_bytes(int B, int hp, int wp, int K) {
    if (K < 1 || K > MC_MAX_ROUNDS || !mc_shape_ok(B, hp, wp)) return -1;
    return mc_layout(B, hp, wp).bytes;
}

int launch_ncut_mask(void* graph, int32_t* degree, const void* alive, int B, int n, hipStream_t s) {
    const char* who = "dinoseg_op_ncut_mask";
    if (!graph || !degree || !alive) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (nc_cells_check(who, B, n, ncut_split_max_cells(), "vector fits the LDS of a row workgroup")) return -1;
    if (ncut_split_graph_bytes(B, n) < 0 || (long long)B * n > NC_MAX_GRID) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells exceed the launch range", who, B, n);
        return -1;
    }
    if (mc_misaligned(graph, 7) || mc_misaligned(alive, 7) || mc_misaligned(degree, 3)) {
        dinoseg_set_error("%s: the graph and alive must be 8-byte aligned, degree 4-byte aligned", who);
        return -1;
    }
    return mc_launch_mask(reinterpret_cast<unsigned long long*>(graph), degree, reinterpret_cast<const unsigned long long*>(alive), B, n, s);
}

int launch_maskcut_select(const int32_t* ids, const uint8_t* fg, const float* margin, const int32_t* seed_cell, void* alive, int B, int hp,
                          int wp, int K, int t, uint8_t* cells, uint8_t* found, int32_t* area, int32_t* box, float* score, hipStream_t s) {
    const char* who = "dinoseg_op_maskcut_select";
    if (!ids || !fg || !margin || !seed_cell || !alive || !cells || !found || !area || !box || !score) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (components_scratch_bytes(B, hp, wp) < 0) {
        dinoseg_set_error("%s: B = %d frames of %d x %d cells (each at least 1, sides at most %d, B hp wp below 2^31)", who, B, hp, wp,
                          DINOSEG_COMPONENTS_MAX_SIDE);
        return -1;
    }
    if (K < 1 || K > MC_MAX_ROUNDS) {
        dinoseg_set_error("%s: K = %d rounds (1 .. %d)", who, K, MC_MAX_ROUNDS);
        return -1;
    }
    if (t < 0 || t >= K) {
        dinoseg_set_error("%s: round t = %d (0 .. K - 1 = %d)", who, t, K - 1);
        return -1;
    }
    if (mc_misaligned(ids, 3) || mc_misaligned(margin, 3) || mc_misaligned(seed_cell, 3) || mc_misaligned(alive, 7) ||
        mc_misaligned(area, 3) || mc_misaligned(box, 3) || mc_misaligned(score, 3)) {
        dinoseg_set_error("%s: alive must be 8-byte aligned, a 32-bit array 4-byte aligned", who);
        return -1;
    }
    return mc_launch_select(ids, fg, margin, seed_cell, reinterpret_cast<unsigned long long*>(alive), B, hp * wp, wp, K, t, cells, found,
                            area, box, score, s);
}

int launch_maskcut(void* graph, int32_t* degree, int B, int hp, int wp, double eps, const float* z_start, int iters, int rows_per_group,
                   int connectivity, int K, uint8_t* cells, uint8_t* found, int32_t* area, int32_t* box, float* score, int32_t* count,
                   uint8_t* fg, float* margin, float* eigvec, int32_t* seed_cell, float* rho, void* scratch, hipStream_t s) {
    const char* who = "dinoseg_op_maskcut";
    if (!cells || !found || !area || !box || !score || !count || !margin) {
        dinoseg_set_error("%s: null pointer (only rho with iters = 0 is optional)", who);
        return -1;
    }
    if (components_scratch_bytes(B, hp, wp) < 0) {
        dinoseg_set_error("%s: B = %d frames of %d x %d cells (each at least 1, sides at most %d, B hp wp below 2^31)", who, B, hp, wp,
                          DINOSEG_COMPONENTS_MAX_SIDE);
        return -1;
    }
    const int n = hp * wp;
    // what dinoseg_op_ncut_iterate_split checks, under this entry's name (z_out: the working z of the scratch, as aligned as the scratch)
    const NcIterateArgs args{graph, degree, B, n, eps, z_start, iters, reinterpret_cast<float*>(scratch), rho, fg, eigvec, margin, seed_cell};
    auto route_checks = [&]() {
        if (rows_per_group < 0) {
            dinoseg_set_error("%s: rows_per_group = %d (0 for the library's choice, or at least 1)", who, rows_per_group);
            return -1;
        }
        const int R = rows_per_group == 0 ? 32 : std::min(rows_per_group, n);  // (the library's choice is at least 32 rows)
        if (ncut_split_scratch_bytes(B, n) < 0 || (long long)B * ((n + R - 1) / R + 1) > NC_MAX_GRID) {
            dinoseg_set_error("%s: B = %d frames of n = %d cells in groups of %d rows exceed the launch range", who, B, n, R);
            return -1;
        }
        return 0;
    };
    if (nc_iterate_check(who, args, true, scratch, ncut_split_max_cells(), "vector fits the LDS of a row workgroup", route_checks)) return -1;
    if (connectivity != 4 && connectivity != 8) {
        dinoseg_set_error("%s: connectivity = %d (4 or 8)", who, connectivity);
        return -1;
    }
    if (K < 1 || K > MC_MAX_ROUNDS) {
        dinoseg_set_error("%s: K = %d rounds (1 .. %d)", who, K, MC_MAX_ROUNDS);
        return -1;
    }
    if (mc_misaligned(area, 3) || mc_misaligned(box, 3) || mc_misaligned(score, 3) || mc_misaligned(count, 3)) {
        dinoseg_set_error("%s: a 32-bit array must be 4-byte aligned", who);
        return -1;
    }

    const McLayout L = mc_layout(B, hp, wp);
    char* sc = reinterpret_cast<char*>(scratch);
    int32_t* small = reinterpret_cast<int32_t*>(sc + L.small);
    int32_t *cc_count = small, *cc_status = small + B, *cc_first = small + 2 * B, *cc_label = small + 3 * B, *cc_area = small + 4 * B,
            *cc_box = small + 5 * B;
    unsigned long long* alive = reinterpret_cast<unsigned long long*>(sc + L.alive);
    unsigned long long* g64 = reinterpret_cast<unsigned long long*>(graph);
    int32_t* cand = reinterpret_cast<int32_t*>(sc + L.cand);
    int32_t* ids = reinterpret_cast<int32_t*>(sc + L.ids);
    float* z = reinterpret_cast<float*>(sc + L.z);
    uint8_t* fg_w = reinterpret_cast<uint8_t*>(sc + L.fg);
    float* margin_w = reinterpret_cast<float*>(sc + L.margin);
    float* eigvec_w = reinterpret_cast<float*>(sc + L.eigvec);
    int32_t* seed_w = reinterpret_cast<int32_t*>(sc + L.seed);
    float* rho_w = reinterpret_cast<float*>(sc + L.rho);
    const int W = (n + 63) >> 6;
    const int per_init = (std::max(n, W) + MC_THREADS - 1) / MC_THREADS, per_round = (std::max(n, iters) + MC_THREADS - 1) / MC_THREADS;

    hipLaunchKernelGGL(mc_init_kernel, dim3((unsigned)((long long)B * per_init)), dim3(MC_THREADS), 0, s, n, W, K, per_init, alive, score);
    DSEG_CHECK_HIP(hipGetLastError());
    for (int t = 0; t < K; ++t) {
        if (int rc = mc_launch_mask(g64, degree, alive, B, n, s)) return rc;
        if (int rc = launch_ncut_iterate_split(graph, degree, B, n, eps, z_start, iters, rows_per_group, z, iters ? rho_w : nullptr, fg_w,
                                               eigvec_w, margin_w, seed_w, sc + L.split, s))
            return rc;
        hipLaunchKernelGGL(mc_round_kernel, dim3((unsigned)((long long)B * per_round)), dim3(MC_THREADS), 0, s, n, W, K, t, iters, per_round,
                           alive, fg_w, margin_w, eigvec_w, seed_w, rho_w, cand, fg, margin, eigvec, seed_cell, rho);
        DSEG_CHECK_HIP(hipGetLastError());
        if (int rc = launch_components(cand, B, hp, wp, connectivity, 0, 1, ids, cc_count, cc_first, cc_label, cc_area, cc_box, cc_status,
                                       sc + L.cc, s))
            return rc;
        if (int rc = mc_launch_select(ids, fg_w, margin_w, seed_w, alive, B, n, wp, K, t, cells, found, area, box, score, s)) return rc;
    }
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)((B + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, s, found, B, K, count);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
