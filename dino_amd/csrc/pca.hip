// PCA of patch features: the streaming moments of the patch tokens, the projection onto a basis and the three-colour feature map.
// The rules are stated in full in include/dinoseg.h (dinoseg_op_token_moments, dinoseg_op_pca_project, dinoseg_op_pca_colour).  Every
// product sum here is v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fp32 fmaf chain: lane l holds A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31], so for X^T X over rows both operands of a lane are one coalesced load of X[row k][column i].
//
//   pca_moments_kernel    one wave per (task, range).  A task is a pair of 64-column tiles (dt <= et) -- four 32 x 32 accumulators,
//                         two rows per instruction, the range's rows in order -- or, past the pairs, one 64-column tile of the column
//                         sums (a lane per column, the rows in order) with the range's count of kept rows.  The partials go to the
//                         scratch; a masked row or a row past the range is a row of zeros.
//   pca_moments_finalize  one thread per element d <= e: the ranges' partials added in range order in fp64, the total added once to
//                         outer[d][e] and to its mirror; likewise the sums and the count.
//   pca_project_kernel    one workgroup per 128 token rows, a wave per 32 of them, every component: the centred rows and the basis
//                         staged in LDS 32 columns at a time (stride 33: the operand reads fall on distinct banks).
//   pca_colour_kernel     the family's 64 x 32 output tile (upsample_common.h) over the three scaled components, then the clamp, the
//                         byte and the nearest cell's keep flag.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

namespace {

constexpr long long PCA_MAX_ROWS = (1ll << 31) - 256;
constexpr int PCA_MAX_RANGES = 64;      // ranges of one call
constexpr int PCA_MIN_RANGE = 128;      // rows of a range, unless there are fewer in all
constexpr int PCA_WAVES = 2048;         // (pairs x ranges) aimed at: two waves per SIMD of the 256 compute units
constexpr int PCA_STEPS = 4;            // row pairs loaded ahead of their MFMAs
constexpr int PCA_PROJ_ROWS = 128, PCA_PROJ_CHUNK = 32, PCA_PROJ_STRIDE = PCA_PROJ_CHUNK + 1;

__host__ __device__ inline int pca_pairs(int T) { return T * (T + 1) / 2; }
// the pair (dt, et), dt <= et, in the order (0,0) (0,1) .. (0,T-1) (1,1) ..
__host__ __device__ inline int pca_pair_index(int T, int dt, int et) { return dt * T - dt * (dt - 1) / 2 + (et - dt); }

bool pca_dim_ok(int D) { return D >= 64 && D <= 1024 && (D & 63) == 0; }
bool pca_rows_ok(long long B, long long n) { return B >= 1 && n >= 1 && B * n <= PCA_MAX_ROWS && n <= PCA_MAX_ROWS; }

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(64) void pca_moments_kernel(const float* __restrict__ tokens, const uint8_t* __restrict__ keep, int N, int n,
                                                         int D, const float* __restrict__ shift, int L, int P, float* __restrict__ part_outer,
                                                         float* __restrict__ part_sum, int* __restrict__ part_count) {
    const int lane = threadIdx.x, lr = lane & 31, lh = lane >> 5;
    const int T = D >> 6, range = blockIdx.y;
    const long long first = (long long)range * L;
    const int r0 = (int)(first < N ? first : N), r1 = (int)(first + L < N ? first + L : N);      // the range's rows: r0 .. r1 - 1

    if ((int)blockIdx.x >= P) {
        // column sums of tile t and the count: the lane's column, the rows in order
        const int t = (int)blockIdx.x - P, col = t * 64 + lane;
        const float sh = shift ? shift[col] : 0.f;
        float acc = 0.f;
        int cnt = 0;
        int b = r0 / n, cell = r0 - b * n;
#pragma unroll 8
        for (int row = r0; row < r1; ++row) {
            const bool kept = !keep || keep[row] != 0;
            const float x = tokens[((size_t)row + b + 1) * D + col];
            acc += kept ? __fsub_rn(x, sh) : 0.f;
            cnt += kept ? 1 : 0;
            if (++cell == n) {
                cell = 0;
                ++b;
            }
        }
        part_sum[(size_t)range * D + col] = acc;
        if (t == 0 && lane == 0) part_count[range] = cnt;
        return;
    }

    int dt = 0, et = (int)blockIdx.x;
    while (et >= T - dt) {
        et -= T - dt;
        ++dt;
    }
    et += dt;
    const bool diag = dt == et;
    const int ca = dt * 64 + lr, cb = et * 64 + lr;
    const float sa0 = shift ? shift[ca] : 0.f, sa1 = shift ? shift[ca + 32] : 0.f;
    const float sb0 = shift ? shift[cb] : 0.f, sb1 = shift ? shift[cb + 32] : 0.f;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the lane's row of the first pair: frame b, cell `cell` (rows past the range are never read)
    int row = r0 + lh;
    int b = row / n, cell = row - b * n;
    for (int k = r0; k < r1; k += 2 * PCA_STEPS) {
        float a0[PCA_STEPS], a1[PCA_STEPS], b0[PCA_STEPS], b1[PCA_STEPS];
#pragma unroll
        for (int u = 0; u < PCA_STEPS; ++u) {
            const bool live = row < r1 && (!keep || keep[row] != 0);
            a0[u] = a1[u] = b0[u] = b1[u] = 0.f;
            if (live) {
                const float* px = tokens + ((size_t)row + b + 1) * D;
                a0[u] = __fsub_rn(px[ca], sa0);
                a1[u] = __fsub_rn(px[ca + 32], sa1);
                if (diag) {
                    b0[u] = a0[u];
                    b1[u] = a1[u];
                } else {
                    b0[u] = __fsub_rn(px[cb], sb0);
                    b1[u] = __fsub_rn(px[cb + 32], sb1);
                }
            }
            row += 2;
            cell += 2;
            while (cell >= n) {
                cell -= n;
                ++b;
            }
        }
#pragma unroll
        for (int u = 0; u < PCA_STEPS; ++u) {
            acc[0][0] = mfma_f32(a0[u], b0[u], acc[0][0]);
            acc[0][1] = mfma_f32(a0[u], b1[u], acc[0][1]);
            acc[1][0] = mfma_f32(a1[u], b0[u], acc[1][0]);
            acc[1][1] = mfma_f32(a1[u], b1[u], acc[1][1]);
        }
    }
    float* out = part_outer + ((size_t)range * P + blockIdx.x) * 4096;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[(i * 32 + acc_row(r, lh)) * 64 + j * 32 + lr] = acc[i][j][r];
}

__global__ __launch_bounds__(256) void pca_moments_finalize_kernel(const float* __restrict__ part_outer, const float* __restrict__ part_sum,
                                                                   const int* __restrict__ part_count, int D, int R, double* __restrict__ sum,
                                                                   double* __restrict__ outer, long long* __restrict__ count) {
    // threads 0 .. D - 1: the sums; thread D: the count; with an outer, D D more threads, one per element
    const int idx = (int)(blockIdx.x * 256 + threadIdx.x) - (D + 1);
    const int DD = D * D;
    if (idx >= 0) {
        if (!outer || idx >= DD) return;
        const int d = idx / D, e = idx - d * D;
        if (d > e) return;
        const int T = D >> 6, P = pca_pairs(T), p = pca_pair_index(T, d >> 6, e >> 6);
        const float* src = part_outer + (size_t)p * 4096 + (d & 63) * 64 + (e & 63);
        double total = 0.0;
        for (int r = 0; r < R; ++r) total += (double)src[(size_t)r * P * 4096];
        outer[(size_t)d * D + e] += total;
        if (d != e) outer[(size_t)e * D + d] += total;
    } else if (idx < -1) {
        const int d = idx + D + 1;
        double total = 0.0;
        for (int r = 0; r < R; ++r) total += (double)part_sum[(size_t)r * D + d];
        sum[d] += total;
    } else if (idx == -1) {
        long long total = 0;
        for (int r = 0; r < R; ++r) total += part_count[r];
        *count += total;
    }
}

template <int QB>
__global__ __launch_bounds__(256) void pca_project_kernel(const float* __restrict__ tokens, unsigned Nt, unsigned n1, int D,
                                                          const float* __restrict__ mean, const float* __restrict__ basis,
                                                          const float* __restrict__ scale, int q, float* __restrict__ out) {
    __shared__ float lds_a[4][32 * PCA_PROJ_STRIDE];
    __shared__ float lds_b[QB * 32 * PCA_PROJ_STRIDE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const unsigned row0 = blockIdx.x * (unsigned)PCA_PROJ_ROWS + wave * 32u;      // (Nt + 127 < 2^32)

    f32x16 acc[QB];
#pragma unroll
    for (int jb = 0; jb < QB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jb][r] = 0.f;

    for (int d0 = 0; d0 < D; d0 += PCA_PROJ_CHUNK) {
        if (d0) __syncthreads();
        // the wave's 32 rows, centred (a row past the last one is zeros)
        const float m = mean[d0 + lr];
#pragma unroll 4
        for (int r = lh; r < 32; r += 2) {
            const unsigned t = row0 + r;
            lds_a[wave][r * PCA_PROJ_STRIDE + lr] = t < Nt ? __fsub_rn(tokens[(size_t)t * D + d0 + lr], m) : 0.f;
        }
        // the basis rows (zeros past q)
        for (int i = tid; i < QB * 32 * PCA_PROJ_CHUNK; i += 256) {
            const int j = i >> 5, c = i & 31;
            lds_b[j * PCA_PROJ_STRIDE + c] = j < q ? basis[(size_t)j * D + d0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < PCA_PROJ_CHUNK; k += 2) {
            const float a = lds_a[wave][lr * PCA_PROJ_STRIDE + k + lh];
#pragma unroll
            for (int jb = 0; jb < QB; ++jb) acc[jb] = mfma_f32(a, lds_b[(jb * 32 + lr) * PCA_PROJ_STRIDE + k + lh], acc[jb]);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned t = row0 + acc_row(r, lh);
        if (t >= Nt) continue;
        const bool cls = t % n1 == 0;
#pragma unroll
        for (int jb = 0; jb < QB; ++jb) {
            const int j = jb * 32 + lr;
            if (j >= q) continue;
            float v = acc[jb][r];
            if (scale) v = __fmul_rn(v, scale[j]);
            out[(size_t)t * q + j] = cls ? 0.f : v;
        }
    }
}

__global__ __launch_bounds__(256) void pca_colour_kernel(const float* __restrict__ comps, int hp, int wp, int q, const float* __restrict__ lo,
                                                         const float* __restrict__ inv, const uint8_t* __restrict__ keep, int OH, int OW,
                                                         int tiles_x, int tiles_y, uint8_t* __restrict__ rgb) {
    extern __shared__ float up_lds[];
    const UpTile T = up_tile(tiles_x, tiles_y, OH, OW);
    const UpStrip S = up_strip(T, hp, wp, OH, OW, 3);
    const int n = hp * wp;
    const float lo0 = lo[0], lo1 = lo[1], lo2 = lo[2], in0 = inv[0], in1 = inv[1], in2 = inv[2];
    for (int cell = T.tid; cell < S.ncells; cell += 256) {
        const int r = cell / S.ncols, col = cell - r * S.ncols;
        const float* g = comps + ((size_t)T.b * (n + 1) + 1 + (size_t)(S.fr0 + r) * wp + S.fc0 + col) * q;
        up_lds[cell * 3 + 0] = __fmul_rn(__fsub_rn(g[0], lo0), in0);
        up_lds[cell * 3 + 1] = __fmul_rn(__fsub_rn(g[1], lo1), in1);
        up_lds[cell * 3 + 2] = __fmul_rn(__fsub_rn(g[2], lo2), in2);
    }
    __syncthreads();
    if (!T.active) return;
    uint8_t px[UP_ROWS][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = up_lds + c;
        UpWalk w(p, S.ro0[0], S.ro1[0], S.off0, S.off1, S.lx);
#pragma unroll
        for (int j = 0; j < UP_ROWS; ++j) {
            float v = w.at(p, j > 0 && S.ro0[j] != S.ro0[j - 1], S.ro1[j], S.off0, S.off1, S.lx, S.ly[j]);
            v = fminf(fmaxf(v, 0.f), 1.f);      // (a NaN becomes 0)
            px[j][c] = (uint8_t)rintf(__fmul_rn(255.f, v));
        }
    }
    if (!T.x_ok) return;
    const int cc = (int)(((long long)T.x * wp) / OW);
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        const int y = T.y0 + j;
        if (y >= OH) break;
        const int cr = (int)(((long long)y * hp) / OH);
        const bool kept = !keep || keep[(size_t)T.b * n + (size_t)cr * wp + cc] != 0;
        uint8_t* o = rgb + ((size_t)T.b * T.plane + T.pix0 + (size_t)j * OW) * 3;
        o[0] = kept ? px[j][0] : (uint8_t)0;
        o[1] = kept ? px[j][1] : (uint8_t)0;
        o[2] = kept ? px[j][2] : (uint8_t)0;
    }
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

int pca_ranges(long long N, int D) {
    const int P = pca_pairs(D >> 6);
    long long R = (PCA_WAVES + P - 1) / P;
    const long long by_rows = (N + PCA_MIN_RANGE - 1) / PCA_MIN_RANGE;
    if (by_rows < R) R = by_rows;
    if (R > PCA_MAX_RANGES) R = PCA_MAX_RANGES;
    return R < 1 ? 1 : (int)R;
}

long long pca_scratch_bytes(int B, int n, int D) {
    if (!pca_rows_ok(B, n) || !pca_dim_ok(D)) return -1;
    const long long R = pca_ranges((long long)B * n, D), P = pca_pairs(D >> 6);
    return 4 * R * (P * 4096 + D + 1);
}

int launch_token_moments(const float* tokens, const uint8_t* keep, int B, int n, int D, const float* shift, double* sum, double* outer,
                         long long* count, void* scratch, hipStream_t s) {
    const char* who = "dinoseg_op_token_moments";
    if (!tokens || !sum || !count || !scratch) {
        dinoseg_set_error("%s: null pointer (tokens, sum, count and scratch are required)", who);
        return -1;
    }
    if (!pca_rows_ok(B, n)) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive, B n <= 2^31 - 256)", who, B, n);
        return -1;
    }
    if (!pca_dim_ok(D)) {
        dinoseg_set_error("%s: D = %d (a multiple of 64 in 64 .. 1024)", who, D);
        return -1;
    }
    if (misaligned(tokens, 16) || misaligned(shift, 16) || misaligned(scratch, 16) || misaligned(sum, 8) || misaligned(outer, 8) ||
        misaligned(count, 8)) {
        dinoseg_set_error("%s: tokens, shift and scratch must be 16-byte aligned, sum, outer and count 8-byte aligned", who);
        return -1;
    }
    const int N = B * n, T = D >> 6, P = pca_pairs(T), R = pca_ranges(N, D), L = (int)(((long long)N + R - 1) / R);
    float* part_outer = reinterpret_cast<float*>(scratch);
    float* part_sum = part_outer + (size_t)R * P * 4096;
    int* part_count = reinterpret_cast<int*>(part_sum + (size_t)R * D);
    const int Pl = outer ? P : 0;
    hipLaunchKernelGGL(pca_moments_kernel, dim3((unsigned)(Pl + T), (unsigned)R), dim3(64), 0, s, tokens, keep, N, n, D, shift, L, Pl, part_outer,
                       part_sum, part_count);
    DSEG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pca_moments_finalize_kernel, dim3((unsigned)(((outer ? D * D : 0) + D + 1 + 255) / 256)), dim3(256), 0, s, part_outer, part_sum,
                       part_count, D, R, sum, outer, count);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_pca_project(const float* tokens, int B, int n, int D, const float* mean, const float* basis, const float* scale, int q, float* out,
                       hipStream_t s) {
    const char* who = "dinoseg_op_pca_project";
    if (!tokens || !mean || !basis || !out) {
        dinoseg_set_error("%s: null pointer (tokens, mean, basis and out are required)", who);
        return -1;
    }
    if (!pca_rows_ok(B, n)) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive, B n <= 2^31 - 256)", who, B, n);
        return -1;
    }
    if (!pca_dim_ok(D)) {
        dinoseg_set_error("%s: D = %d (a multiple of 64 in 64 .. 1024)", who, D);
        return -1;
    }
    if (q < 1 || q > DINOSEG_PCA_MAX_Q) {
        dinoseg_set_error("%s: q = %d components (1 .. %d)", who, q, DINOSEG_PCA_MAX_Q);
        return -1;
    }
    if (misaligned(tokens, 16) || misaligned(mean, 16) || misaligned(basis, 16) || misaligned(scale, 4) || misaligned(out, 4)) {
        dinoseg_set_error("%s: tokens, mean and basis must be 16-byte aligned, scale and out 4-byte aligned", who);
        return -1;
    }
    const unsigned n1 = (unsigned)n + 1u, Nt = (unsigned)((long long)B * (n + 1ll));      // (B (n + 1) <= 2 B n < 2^32 - 512)
    const dim3 grid((Nt + PCA_PROJ_ROWS - 1) / PCA_PROJ_ROWS);
    const int QB = (q + 31) / 32;
    if (QB <= 1)
        hipLaunchKernelGGL(pca_project_kernel<1>, grid, dim3(256), 0, s, tokens, Nt, n1, D, mean, basis, scale, q, out);
    else if (QB <= 2)
        hipLaunchKernelGGL(pca_project_kernel<2>, grid, dim3(256), 0, s, tokens, Nt, n1, D, mean, basis, scale, q, out);
    else if (QB <= 4)
        hipLaunchKernelGGL(pca_project_kernel<4>, grid, dim3(256), 0, s, tokens, Nt, n1, D, mean, basis, scale, q, out);
    else
        hipLaunchKernelGGL(pca_project_kernel<8>, grid, dim3(256), 0, s, tokens, Nt, n1, D, mean, basis, scale, q, out);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_pca_colour(const float* comps, int B, int hp, int wp, int q, const float* lo, const float* inv, const uint8_t* keep, int OH,
                      int OW, uint8_t* rgb, hipStream_t s) {
    const char* who = "dinoseg_op_pca_colour";
    if (!comps || !lo || !inv || !rgb) {
        dinoseg_set_error("%s: null pointer (comps, lo, inv and rgb are required)", who);
        return -1;
    }
    if (q < 3 || q > DINOSEG_PCA_MAX_Q) {
        dinoseg_set_error("%s: q = %d components (3 .. %d)", who, q, DINOSEG_PCA_MAX_Q);
        return -1;
    }
    if (upsample_check_shape(who, B, hp, wp, 3, OH, OW)) return -1;
    if (OH > 16384 || OW > 16384 || !pca_rows_ok(B, (long long)hp * wp)) {
        dinoseg_set_error("%s: output %dx%d, B = %d (sides <= 16384, B hp wp <= 2^31 - 256)", who, OH, OW, B);
        return -1;
    }
    if (misaligned(comps, 4) || misaligned(lo, 4) || misaligned(inv, 4)) {
        dinoseg_set_error("%s: comps, lo and inv must be 4-byte aligned", who);
        return -1;
    }
    UpTilePlan pl;
    if (upsample_tile_plan(who, hp, wp, 3, OH, OW, &pl)) return -1;
    if (pl.CC != 3 || pl.stride != 3) {
        dinoseg_set_error("%s: a tile's footprint does not hold three channels in one pass", who);
        return -1;
    }
    hipLaunchKernelGGL(pca_colour_kernel, dim3((unsigned)((long long)pl.tiles_x * pl.tiles_y * B)), dim3(256), pl.lds_bytes, s, comps, hp, wp,
                       q, lo, inv, keep, OH, OW, pl.tiles_x, pl.tiles_y, rgb);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
