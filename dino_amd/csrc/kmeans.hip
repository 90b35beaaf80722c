// Spherical k-means over patch features: Lloyd iterations on the unit rows that dinoseg_op_normalize_tokens leaves (fp16 hi + lo
// planes scaled by 2^10), all B n points of a batch or clip jointly.  The rule is stated in full in include/dinoseg.h
// (dinoseg_op_kmeans_assign); in short a_i = argmax_j <x_i, c_j> (lowest j on an exact tie), c_j = the unit row of the sum of its
// points, an empty cluster keeps its centroid.  No atomics; every order of summation is a function of the shapes and the assignment.
//
//   kmeans_init_kernel        one wave per centroid row: ||row||^2 and the quotient in fp64 (or the row as it is), the fp32 row and
//                             its split 2^10 c = hi + lo into planes [2][K][D].
//   kmeans_assign_kernel      one workgroup (4 waves) per tile of 64 consecutive points.  The centroid planes are walked in blocks of
//                             64 rows by the family's pair walk (pair_common.h); wave (qh, kh) multiplies centroids 32 kh .. by points
//                             32 qh .. with the arithmetic of propagate_scores_kernel: lo.hi + hi.lo + hi.hi into one accumulator.  A
//                             lane owns one point and 16 centroids of the block in ascending order; its running (score, index) pair
//                             stays in registers (a strict > keeps the lower index).  The four pairs of a point meet in LDS under the
//                             total order (score descending, index ascending).  The [N, K] scores are stored only on request.  The
//                             tile's objective share (xor tree over the 64 points) and its count of changed points go to the scratch.
//   kmeans_records_kernel     one workgroup: the tiles' shares in a fixed order -> objective and moved.
//   kmeans_partial_kernel     one workgroup per (range of points, cluster), R = min(ceil(N / 256), 4096 / K clamped to 16 .. 64) ranges
//                             (measured: 64 ranges at K = 256 were 16 384 workgroups with a row or two each and took 86 us): the
//                             range's assignments are scanned in chunks of 1024
//                             (ballots, so the list of members is in index order), the members' rows gathered 16 bytes of each
//                             plane per thread, 4 rows in flight per thread, x = (hi + lo) 2^-10 added in fp32; thread group g of G
//                             = 256 / (threads per row) takes members g, g + G, ... of the chunk's list, the groups are added in
//                             group order.  Output: the range's partial sum [D] and count for the cluster.
//   kmeans_finalize_kernel    one workgroup per cluster: the ranges in range order, ||m||^2 in fp64, the quotient in fp64, the fp32
//                             row and its planes; n_j = 0 or ||m|| = 0 copies the previous row and planes.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "pair_common.h"

#include <climits>

namespace dseg {

namespace {

constexpr int KM_TILE = PAIR_TILE;              // points of an assign workgroup
constexpr int KM_MAX_RANGES = 64;               // point ranges of the update: partial centroid sets in the scratch
constexpr int KM_MIN_RANGES = 16;               // ... the cap at large K
constexpr int KM_RANGE_WGS = 4096;              // ... R K stays near this many workgroups
constexpr int KM_RANGE_MIN = 256;               // a range holds at least this many points (fewer ranges for small N)
constexpr int KM_CHUNK = 1024;                  // assignments scanned per list
constexpr long long KM_MAX_POINTS = (1ll << 31) - 256;

// the fp32 row element and its planes: c = fp32(q), 2^10 c = hi + lo
__device__ __forceinline__ void km_write_unit(double q, float* c, uint16_t* hi, uint16_t* lo) {
    const float c32 = (float)q;
    const UnitSplit v = split_unit((double)c32 * 1024.0);
    *c = c32;
    *hi = v.hi;
    *lo = v.lo;
}

// rows may be the centroids themselves: every element is read and written by the same lane, and the norm is complete before the first write
__global__ __launch_bounds__(256) void kmeans_init_kernel(const float* rows, int K, int D, int normalize, float* centroids,
                                                          uint16_t* __restrict__ planes) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= K) return;                                               // (a whole wave: no barrier follows)
    const float* src = rows + (size_t)row * D;
    double inv = 1.0;
    if (normalize) {
        double ss = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double v = (double)src[d];
            ss = fma(v, v, ss);
        }
        ss = wave_sum_f64(ss);
        inv = 1.0 / fmax(sqrt(ss), 1e-12);
    }
    float* c = centroids + (size_t)row * D;
    uint16_t* hi = planes + (size_t)row * D;
    uint16_t* lo = hi + (size_t)K * D;
    for (int d = lane; d < D; d += 64) km_write_unit((double)src[d] * inv, c + d, hi + d, lo + d);
}

// prev may be assign itself: element i of both belongs to one thread, which reads before it writes
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const uint16_t* __restrict__ points, int N, int n,
                                                            const uint16_t* __restrict__ cplanes, int K, int D, const int32_t* prev,
                                                            int32_t* assign, float* __restrict__ best, float* __restrict__ scores,
                                                            float* __restrict__ tile_obj, int32_t* __restrict__ tile_moved) {
    __shared__ __attribute__((aligned(16))) char km_lds[PAIR_STAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int qh = wave >> 1, kh = wave & 1;
    const int i0 = (int)blockIdx.x * KM_TILE;                           // (N <= 2^31 - 256: i0 + 63 fits)

    // the lane's point in the selection
    const int pi = i0 + qh * 32 + lr;
    const bool pvalid = pi < N;

    // the tile's points as the walk stages them (pair_common.h)
    size_t prow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = min(i0 + pair_stage_row(h), N - 1);               // (a row past the last point re-reads a real one)
        const int b = i / n, c = i - b * n;
        prow[h] = ((size_t)b * 2 * n + c) * D;
    }
    // (a centroid row past K re-reads a real one; never selected)
    auto centroid_row = [&](int j) { return (size_t)min(j, K - 1) * D; };

    float bs = -INFINITY;                                               // the lane's running pair
    int bj = INT_MAX;
    f32x16 acc;
    auto zero = [&]() {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    };
    auto slice = [&](bf16x8 phi, bf16x8 plo, bf16x8 chi, bf16x8 clo) {
        acc = mfma32f<FMT_FP16>(clo, phi, acc);
        acc = mfma32f<FMT_FP16>(chi, plo, acc);
        acc = mfma32f<FMT_FP16>(chi, phi, acc);
    };
    // the block's scores: register r of this lane is centroid acc_row(r, lh) of the wave's half (ascending in r), point lr
    auto select = [&](int kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = kb * 64 + kh * 32 + acc_row(r, lh);
            if (j >= K) continue;
            const float s = acc[r] * PAIR_UNSCALE + 0.f;                // (+ 0: a negative zero becomes the positive one)
            if (scores && pvalid) scores[(size_t)pi * K + j] = s;
            if (s > bs) {                                               // (strict: the lower index keeps an exact tie)
                bs = s;
                bj = j;
            }
        }
    };
    pair_walk(km_lds, points, (size_t)n * D, prow, cplanes, (size_t)K * D, (K + 63) >> 6, D >> 6, centroid_row, [](int) {}, zero, slice,
              select);
    __syncthreads();                                                    // the staging area becomes the four pairs of every point
    float* ms = reinterpret_cast<float*>(km_lds);
    int* mj = reinterpret_cast<int*>(km_lds + 1024);
    ms[tid] = bs;
    mj[tid] = bj;
    __syncthreads();
    if (tid < 64) {                                                     // wave 0: point tid of the tile
        const int t0 = ((tid >> 5) * 2) * 64 + (tid & 31);
        float s = ms[t0];
        int j = mj[t0];
#pragma unroll
        for (int o = 32; o <= 96; o += 32) {
            const float s2 = ms[t0 + o];
            const int j2 = mj[t0 + o];
            if (better(s2, j2, s, j)) { s = s2; j = j2; }
        }
        const int i = i0 + tid;
        float o = 0.f;
        bool mv = false;
        if (i < N) {
            const int a = j == INT_MAX ? 0 : j;                         // (no score compared greater than -inf: not a finite input)
            mv = prev ? prev[i] != a : true;
            assign[i] = a;
            best[i] = s;
            o = s;
        }
        o = wave_sum(o);                                                // (xor tree: a fixed order)
        const int cnt = __popcll(__ballot(mv));
        if (tid == 0) {
            tile_obj[blockIdx.x] = o;
            tile_moved[blockIdx.x] = cnt;
        }
    }
}

__global__ __launch_bounds__(256) void kmeans_records_kernel(const float* __restrict__ tile_obj, const int32_t* __restrict__ tile_moved,
                                                             int ntiles, float* __restrict__ objective, int32_t* __restrict__ moved) {
    __shared__ float so[256];
    __shared__ int sm[256];
    const int tid = threadIdx.x;
    float o = 0.f;
    int m = 0;
    for (int t = tid; t < ntiles; t += 256) {
        o += tile_obj[t];
        m += tile_moved[t];
    }
    so[tid] = o;
    sm[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            so[tid] += so[tid + w];
            sm[tid] += sm[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (objective) *objective = so[0];
        if (moved) *moved = sm[0];
    }
}

__device__ __forceinline__ void km_add_row(float (&acc)[8], uint4 h, uint4 l) {
    const f16x8 hv = __builtin_bit_cast(f16x8, h), lv = __builtin_bit_cast(f16x8, l);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += ((float)hv[e] + (float)lv[e]) * 0x1p-10f;   // x = (hi + lo) 2^-10, exact in fp32
}

__global__ __launch_bounds__(256) void kmeans_partial_kernel(const uint16_t* __restrict__ points, const int32_t* __restrict__ assign,
                                                             int N, int n, int D, int L, int K, int tpr, float* __restrict__ psum,
                                                             int32_t* __restrict__ pcount) {
    __shared__ int list[KM_CHUNK];
    __shared__ int wc[4];
    __shared__ float red[256 * 8];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = blockIdx.x, j = blockIdx.y;
    const long long i0l = (long long)r * L;
    const int i0 = (int)(i0l < N ? i0l : N), i1 = (int)(i0l + L < N ? i0l + L : N);
    const int G = 256 / tpr, g = tid / tpr, c = tid - g * tpr;          // tpr: threads per row, a power of two in 8 .. 256
    const int nchunk = D >> 3;                                          // 16-byte pieces of a plane's row
    const size_t p_lo = (size_t)n * D;
    auto ld16 = [](const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); };
    int count = 0;
    for (int cb = 0; cb < nchunk; cb += tpr) {                          // one pass unless D > 2048
        const bool cvalid = cb + c < nchunk;
        float tot[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        count = 0;
        for (int base = i0; base < i1; base += KM_CHUNK) {
            // the chunk's members in index order: wave w scans entries 256 w .. 256 w + 255
            unsigned long long mk[4];
            int mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int off = wave * 256 + q * 64 + lane;             // (base + off < i1 <= N before it is used)
                const bool match = off < i1 - base && assign[base + off] == j;
                mk[q] = __ballot(match);
                mine += __popcll(mk[q]);
            }
            __syncthreads();                                            // everyone is done with the previous list and wc
            if (lane == 0) wc[wave] = mine;
            __syncthreads();
            int at = 0, cnt = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                at += w < wave ? wc[w] : 0;
                cnt += wc[w];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if ((mk[q] >> lane) & 1ull) list[at + __popcll(mk[q] & ((1ull << lane) - 1ull))] = base + wave * 256 + q * 64 + lane;
                at += __popcll(mk[q]);
            }
            __syncthreads();
            count += cnt;
            // group g adds members g, g + G, ... of the list, four rows in flight
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (cvalid) {
                for (int e = g; e < cnt; e += 4 * G) {
                    uint4 h[4], l[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int ee = e + u * G;
                        h[u] = make_uint4(0, 0, 0, 0);
                        l[u] = make_uint4(0, 0, 0, 0);
                        if (ee < cnt) {
                            const int i = list[ee];
                            const int b = i / n, cell = i - b * n;
                            const uint16_t* p = points + ((size_t)b * 2 * n + cell) * D + (size_t)(cb + c) * 8;
                            h[u] = ld16(p);
                            l[u] = ld16(p + p_lo);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) km_add_row(acc, h[u], l[u]);       // (a row of zeros past the list adds nothing)
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[e];
            __syncthreads();
            if (g == 0) {
                for (int gg = 0; gg < G; ++gg) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) tot[e] += red[(gg * tpr + c) * 8 + e];
                }
            }
        }
        if (g == 0 && cvalid) {
            float* out = psum + ((size_t)r * K + j) * D + (size_t)(cb + c) * 8;
            *reinterpret_cast<float4*>(out) = make_float4(tot[0], tot[1], tot[2], tot[3]);
            *reinterpret_cast<float4*>(out + 4) = make_float4(tot[4], tot[5], tot[6], tot[7]);
        }
    }
    if (tid == 0) pcount[r * K + j] = count;
}

// the new row may be the previous one: a cluster's rows belong to its workgroup alone
__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const float* __restrict__ psum, const int32_t* __restrict__ pcount, int R,
                                                              int K, int D, const float* prev_c, const uint16_t* prev_p,
                                                              float* centroids, uint16_t* planes, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) char kmf_lds[];
    float* m_lds = reinterpret_cast<float*>(kmf_lds);                   // [D] the cluster's sum
    __shared__ double wss[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = blockIdx.x;
    int nj = 0;
#pragma unroll 8
    for (int r = 0; r < R; ++r) nj += pcount[r * K + j];
    double ss = 0.0;
    const size_t rstride = (size_t)K * D;
    for (int d = tid; d < D; d += 256) {
        const float* p = psum + (size_t)j * D + d;
        float m = 0.f;
        int r = 0;
        for (; r + 8 <= R; r += 8) {                                    // ranges in range order, eight loads in flight
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u) * rstride];
#pragma unroll
            for (int u = 0; u < 8; ++u) m += v[u];
        }
        for (; r < R; ++r) m += p[(size_t)r * rstride];
        m_lds[d] = m;
        ss = fma((double)m, (double)m, ss);
    }
    ss = wave_sum_f64(ss);
    if (lane == 0) wss[wave] = ss;
    __syncthreads();
    ss = ((wss[0] + wss[1]) + wss[2]) + wss[3];
    if (tid == 0) counts[j] = nj;
    const size_t row = (size_t)j * D, lo = (size_t)K * D;
    if (nj == 0 || !(ss > 0.0)) {                                       // an empty or cancelled cluster keeps its centroid bit for bit
        if (centroids != prev_c)
            for (int d = tid; d < D; d += 256) centroids[row + d] = prev_c[row + d];
        if (planes != prev_p)
            for (int d = tid; d < D; d += 256) {
                planes[row + d] = prev_p[row + d];
                planes[lo + row + d] = prev_p[lo + row + d];
            }
        return;
    }
    const double inv = 1.0 / sqrt(ss);
    for (int d = tid; d < D; d += 256)                                  // (m_lds[d] is this thread's own store)
        km_write_unit((double)m_lds[d] * inv, centroids + row + d, planes + row + d, planes + lo + row + d);
}

bool km_shape_ok(long long B, long long n, int K, int D) {
    return B >= 1 && n >= 1 && B * n <= KM_MAX_POINTS && B <= KM_MAX_POINTS && n <= KM_MAX_POINTS && K >= 1 && K <= DINOSEG_KMEANS_MAX_K &&
           D >= 64 && D % 64 == 0 && D <= 8192;
}

int km_shape_check(const char* who, int B, int n, int K, int D) {
    if (pair_width_check(who, D)) return -1;
    if (K < 1 || K > DINOSEG_KMEANS_MAX_K) {
        dinoseg_set_error("%s: K = %d centroids (1 <= K <= %d)", who, K, DINOSEG_KMEANS_MAX_K);
        return -1;
    }
    if (B < 1 || n < 1) {
        dinoseg_set_error("%s: B = %d frames of n = %d cells (positive)", who, B, n);
        return -1;
    }
    if ((long long)B * n > KM_MAX_POINTS) {
        dinoseg_set_error("%s: B n = %lld points exceed the launch range (%lld)", who, (long long)B * n, KM_MAX_POINTS);
        return -1;
    }
    return 0;
}

bool km_misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// ranges of the update: at most 64, at most 4096 / K (not below 16: the partial launch stays near 4096 workgroups at large K, where a
// workgroup per (range, cluster) of a finer cut would find a row or two), and no range shorter than 256 points
int km_ranges(long long N, int K) {
    const long long r = (N + KM_RANGE_MIN - 1) / KM_RANGE_MIN;
    int cap = KM_RANGE_WGS / K;
    cap = cap < KM_MIN_RANGES ? KM_MIN_RANGES : cap > KM_MAX_RANGES ? KM_MAX_RANGES : cap;
    return (int)(r < cap ? r : cap);
}

// scratch: [R][K][D] fp32 partial sums, [R][K] int32 partial counts, [tiles] fp32 objective shares, [tiles] int32 moved counts
struct KmScratch {
    float* psum;
    int32_t* pcount;
    float* tile_obj;
    int32_t* tile_moved;
};

KmScratch km_scratch(void* scratch, long long N, int K, int D) {
    const int R = km_ranges(N, K);
    const long long tiles = (N + KM_TILE - 1) / KM_TILE;
    KmScratch s;
    s.psum = reinterpret_cast<float*>(scratch);
    s.pcount = reinterpret_cast<int32_t*>(s.psum + (size_t)R * K * D);
    s.tile_obj = reinterpret_cast<float*>(s.pcount + (size_t)R * K);
    s.tile_moved = reinterpret_cast<int32_t*>(s.tile_obj + tiles);
    return s;
}

}  // namespace

long long kmeans_scratch_bytes(int B, int n, int K, int D) {
    if (!km_shape_ok(B, n, K, D)) return -1;
    const long long N = (long long)B * n;
    return 4ll * km_ranges(N, K) * K * (D + 1) + 8ll * ((N + KM_TILE - 1) / KM_TILE);
}

int launch_kmeans_init(const float* rows, int K, int D, int normalize, float* centroids, void* planes, hipStream_t s) {
    const char* who = "dinoseg_op_kmeans_init";
    if (!rows || !centroids || !planes) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (km_shape_check(who, 1, 1, K, D)) return -1;
    if (km_misaligned(planes, 15) || km_misaligned(rows, 3) || km_misaligned(centroids, 3)) {
        dinoseg_set_error("%s: planes must be 16-byte aligned, the rows 4-byte aligned", who);
        return -1;
    }
    if (normalize != 0 && normalize != 1) {
        dinoseg_set_error("%s: normalize = %d (0 = rows as they are, 1 = unit rows)", who, normalize);
        return -1;
    }
    hipLaunchKernelGGL(kmeans_init_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, s, rows, K, D, normalize, centroids,
                       reinterpret_cast<uint16_t*>(planes));
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_kmeans_assign(const void* points, int B, int n, const void* centroid_planes, int K, int D, const int32_t* prev_assign,
                         int32_t* assign, float* best, float* scores, float* objective, int32_t* moved, void* scratch, hipStream_t s) {
    const char* who = "dinoseg_op_kmeans_assign";
    if (!points || !centroid_planes || !assign || !best || !scratch) {
        dinoseg_set_error("%s: null pointer (points, centroid planes, assign, best and scratch are required)", who);
        return -1;
    }
    if (km_shape_check(who, B, n, K, D)) return -1;
    if (km_misaligned(points, 15) || km_misaligned(centroid_planes, 15) || km_misaligned(scratch, 15)) {
        dinoseg_set_error("%s: points, centroid planes and scratch must be 16-byte aligned", who);
        return -1;
    }
    if (km_misaligned(prev_assign, 3) || km_misaligned(assign, 3) || km_misaligned(best, 3) || km_misaligned(scores, 3) ||
        km_misaligned(objective, 3) || km_misaligned(moved, 3)) {
        dinoseg_set_error("%s: a 32-bit array is not 4-byte aligned", who);
        return -1;
    }
    const long long N = (long long)B * n;
    const int tiles = (int)((N + KM_TILE - 1) / KM_TILE);
    const KmScratch ws = km_scratch(scratch, N, K, D);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)tiles), dim3(256), 0, s, reinterpret_cast<const uint16_t*>(points), (int)N, n,
                       reinterpret_cast<const uint16_t*>(centroid_planes), K, D, prev_assign, assign, best, scores, ws.tile_obj,
                       ws.tile_moved);
    DSEG_CHECK_HIP(hipGetLastError());
    if (objective || moved) {
        hipLaunchKernelGGL(kmeans_records_kernel, dim3(1), dim3(256), 0, s, ws.tile_obj, ws.tile_moved, tiles, objective, moved);
        DSEG_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int launch_kmeans_update(const void* points, int B, int n, const int32_t* assign, const float* prev_centroids, const void* prev_planes,
                         int K, int D, float* centroids, void* planes, int32_t* counts, void* scratch, hipStream_t s) {
    const char* who = "dinoseg_op_kmeans_update";
    if (!points || !assign || !prev_centroids || !prev_planes || !centroids || !planes || !counts || !scratch) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (km_shape_check(who, B, n, K, D)) return -1;
    if (km_misaligned(points, 15) || km_misaligned(prev_planes, 15) || km_misaligned(planes, 15) || km_misaligned(scratch, 15)) {
        dinoseg_set_error("%s: points, both centroid planes and scratch must be 16-byte aligned", who);
        return -1;
    }
    if (km_misaligned(assign, 3) || km_misaligned(prev_centroids, 3) || km_misaligned(centroids, 3) || km_misaligned(counts, 3)) {
        dinoseg_set_error("%s: a 32-bit array is not 4-byte aligned", who);
        return -1;
    }
    const long long N = (long long)B * n;
    const int R = km_ranges(N, K);
    const int L = (int)((N + R - 1) / R);
    int tpr = 8;                                                        // threads per row: the power of two >= D / 8, at most 256
    while (tpr < D / 8 && tpr < 256) tpr *= 2;
    const KmScratch ws = km_scratch(scratch, N, K, D);
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)R, (unsigned)K), dim3(256), 0, s, reinterpret_cast<const uint16_t*>(points),
                       assign, (int)N, n, D, L, K, tpr, ws.psum, ws.pcount);
    DSEG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kmeans_finalize_kernel, dim3((unsigned)K), dim3(256), (size_t)D * 4, s, ws.psum, ws.pcount, R, K, D, prev_centroids,
                       reinterpret_cast<const uint16_t*>(prev_planes), centroids, reinterpret_cast<uint16_t*>(planes), counts);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
