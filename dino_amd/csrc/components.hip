// Connected components of label maps and their object table (the rule: include/dinoseg.h, dinoseg_op_components).  Five plain launches
// behind one 4-byte memset of status, ordered by the stream alone: no cooperative launch, no grid barrier, no flag between workgroups.
//
//   cc_local_kernel    one workgroup per 64 x 32 tile (the tile of upsample_common.h: wave w owns rows 8w .. 8w+7, lane l column l).  The
//                      labels go to LDS (void and out-of-frame pixels as -1); every pixel starts at the first pixel of its horizontal run
//                      (one ballot per row); pixels are united with the row above (and, at connectivity 8, the two diagonals above) by
//                      atomicMin on the LDS parents; every pixel then follows its chain and writes its tile root to parent[] as the
//                      global linear index y W + x (-1 on void pixels).  Raster order inside a tile agrees with the global one.
//   cc_merge_kernel    one thread per pixel on a tile's right or bottom edge: unions across the edge (the straight neighbour; at
//                      connectivity 8 the two diagonal ones, which include both diagonals across every tile corner) by atomicMin on
//                      parent[], read through agent-scope relaxed atomic loads.
//   cc_flatten_kernel  one wave per row segment of 64 pixels: every pixel follows parent[] to its root and writes it to ids[] (the
//                      array read is never the array written); the segment's ballot of roots (root == own index) goes to mask[].
//   cc_scan_kernel     one workgroup per frame: the exclusive prefix sum of the segments' popcounts into off[] (segments are in raster
//                      order, so roots of segment k precede those of k + 1), count[], and the start values of the M table rows.
//   cc_label_kernel    one wave per row segment: a pixel's number is off[segment of its root] + the popcount of that segment's mask
//                      below the root's lane -- no array of numbers, no launch that forms one.  ids[p] is read and written by its own
//                      thread only.  Roots fill first / label / box.y0 of their row; area, box.x0, box.x1 and box.y1 take one integer atomic
//                      per wave and distinct number (the wave is one row segment: the area is a popcount, the x range the mask's first and
//                      last bit), and the three min / max atomics are skipped when a plain read already shows a value at least as good.
//
// Termination (also DESIGN.md).  Invariant: a slot of a parent array only ever receives a SMALLER index than it holds (the initial run
// start is <= the pixel, every later store is an atomicMin), so parent[i] <= i at every moment.  A find chain therefore strictly
// descends and ends after at most H W steps whatever other threads store meanwhile.  A union retries only after its atomicMin found the
// slot already lowered by somebody else (old < a), and continues from old: its upper end strictly descends, so it retries at most H W
// times.  Each loop still carries a step cap of H W (inside a tile: the tile's 2048 pixels, the longest chain its LDS array can hold); an
// overrun sets status[b] = 1 and leaves the loop.
#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"
#include "upsample_common.h"

namespace dseg {

namespace {

constexpr int CC_TW = UP_TW, CC_TH = UP_TH, CC_THREADS = 256, CC_TILE = CC_TW * CC_TH;      // 64 x 32 pixels, 8 per thread
constexpr int CC_MAX_SIDE = 8192, CC_MAX_OBJECTS = 1 << 20;
constexpr int CC_SCAN_THREADS = 1024, CC_SCAN_WAVES = CC_SCAN_THREADS / 64;
static_assert(CC_THREADS == 64 * UP_WAVES, "one wave per 8 rows of the tile");

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- LDS union-find of one tile.  par[i] <= i always; see the termination argument above.
__device__ __forceinline__ int cc_find_lds(volatile int* par, int a, int cap, int* overrun) {
    for (int steps = 0;; ++steps) {
        const int p = par[a];
        if (p == a) return a;
        if (steps >= cap) {
            *overrun = 1;
            return a;
        }
        a = p;
    }
}
__device__ __forceinline__ void cc_union_lds(int* par, int a, int b, int cap, int* overrun) {
    for (int steps = 0;; ++steps) {
        a = cc_find_lds(par, a, cap, overrun);
        b = cc_find_lds(par, b, cap, overrun);
        if (a == b || *overrun) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&par[a], b);                          // a > b: the slot only ever receives a smaller index
        if (old == a) return;                                           // a was a root and now hangs under b
        if (steps >= cap) {
            *overrun = 1;
            return;
        }
        a = old;                                                        // somebody lowered the slot first (old < a): unite old and b
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const int32_t* __restrict__ labels, int H, int W, int tiles_x, int tiles_y,
                                                              int conn8, int ignore, int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ status) {
    __shared__ int lab[CC_TILE];
    __shared__ int par[CC_TILE];
    const UpTile T = up_tile(tiles_x, tiles_y, H, W);
    const int32_t* src = labels + (size_t)T.b * T.plane;
    int overrun = 0;
    // labels -> LDS; every pixel starts at the first pixel of its horizontal run inside the tile
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        const int ly = T.wave * UP_ROWS + j, y = T.y_first + ly, li = ly * CC_TW + T.lane;
        int v = -1;
        if (T.x_ok && y < H) {
            v = src[(size_t)y * W + T.x];
            if (v < 0 || v == ignore) v = -1;
        }
        const int left = __shfl_up(v, 1);
        const bool starts = T.lane == 0 || v < 0 || left != v;
        const unsigned long long m = __ballot(starts) & (~0ull >> (63 - T.lane));      // (bit 0 is always set)
        lab[li] = v;
        par[li] = ly * CC_TW + (63 - __builtin_clzll(m));
    }
    __syncthreads();
    // unions with the row above.  A union is skipped where a neighbour's union implies it.
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        const int ly = T.wave * UP_ROWS + j, li = ly * CC_TW + T.lane;
        const int v = lab[li];
        if (ly == 0 || v < 0) continue;
        const int up = lab[li - CC_TW];
        const int lf = T.lane > 0 ? lab[li - 1] : -1, ul = T.lane > 0 ? lab[li - CC_TW - 1] : -1;
        if (up == v) {
            if (!(lf == v && ul == v)) cc_union_lds(par, li, li - CC_TW, CC_TILE, &overrun);   // (else the left pixel's union covers it)
        } else if (conn8) {
            if (ul == v && lf != v) cc_union_lds(par, li, li - CC_TW - 1, CC_TILE, &overrun);  // (lf == v: left is under ul already)
            if (T.lane < CC_TW - 1 && lab[li - CC_TW + 1] == v) cc_union_lds(par, li, li - CC_TW + 1, CC_TILE, &overrun);
        }
    }
    __syncthreads();
    // tile roots as global linear indices
#pragma unroll
    for (int j = 0; j < UP_ROWS; ++j) {
        const int ly = T.wave * UP_ROWS + j, y = T.y_first + ly, li = ly * CC_TW + T.lane;
        if (!T.x_ok || y >= H) continue;
        int out = -1;
        if (lab[li] >= 0) {
            const int r = cc_find_lds(par, li, CC_TILE, &overrun);
            out = (T.y_first + (r >> 6)) * W + T.x_first + (r & 63);
        }
        parent[(size_t)T.b * T.plane + (size_t)y * W + T.x] = out;
    }
    if (overrun) status[T.b] = 1;
}

// ---- global union-find on parent[] of one frame
__device__ __forceinline__ int cc_find_agent(const int* par, int a, int cap, int* overrun) {
    for (int steps = 0;; ++steps) {
        const int p = cc_load(par + a);
        if (p == a) return a;
        if (steps >= cap) {
            *overrun = 1;
            return a;
        }
        a = p;
    }
}
__device__ __forceinline__ void cc_union_agent(int* par, int a, int b, int cap, int* overrun) {
    for (int steps = 0;; ++steps) {
        a = cc_find_agent(par, a, cap, overrun);
        b = cc_find_agent(par, b, cap, overrun);
        if (a == b || *overrun) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        if (steps >= cap) {
            *overrun = 1;
            return;
        }
        a = old;
    }
}

// A frame's seam pixels: vx seams of H pixels (x = 64 k + 63, x + 1 < W), then hy seams of W pixels (y = 32 k + 31, y + 1 < H).
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const int32_t* __restrict__ labels, int H, int W, int vx, int hy, int per_frame,
                                                              int groups_per_frame, int conn8, int ignore, int cap, int32_t* parent,
                                                              int32_t* __restrict__ status) {
    const int b = (int)blockIdx.x / groups_per_frame;
    const int t = ((int)blockIdx.x - b * groups_per_frame) * CC_THREADS + (int)threadIdx.x;
    if (t >= per_frame) return;
    const size_t plane = (size_t)H * W;
    const int32_t* lab = labels + (size_t)b * plane;
    int* par = parent + (size_t)b * plane;
    auto value = [&](int x, int y) {
        const int v = lab[(size_t)y * W + x];
        return (v < 0 || v == ignore) ? -1 : v;
    };
    int overrun = 0;
    if (t < vx * H) {
        const int k = t / H, y = t - k * H, x = k * CC_TW + CC_TW - 1;
        const int v = value(x, y);
        if (v < 0) return;
        if (value(x + 1, y) == v) {
            // (the pair above, inside the same two tiles and joined to this one in both, is united by its own thread)
            const bool covered = (y % CC_TH) != 0 && value(x, y - 1) == v && value(x + 1, y - 1) == v;
            if (!covered) cc_union_agent(par, y * W + x, y * W + x + 1, cap, &overrun);
        }
        if (conn8) {
            if (y > 0 && value(x + 1, y - 1) == v) cc_union_agent(par, y * W + x, (y - 1) * W + x + 1, cap, &overrun);
            if (y + 1 < H && value(x + 1, y + 1) == v) cc_union_agent(par, y * W + x, (y + 1) * W + x + 1, cap, &overrun);
        }
    } else {
        const int u = t - vx * H;
        const int k = u / W, x = u - k * W, y = k * CC_TH + CC_TH - 1;
        const int v = value(x, y);
        if (v < 0) return;
        if (value(x, y + 1) == v) {
            const bool covered = (x % CC_TW) != 0 && value(x - 1, y) == v && value(x - 1, y + 1) == v;
            if (!covered) cc_union_agent(par, y * W + x, (y + 1) * W + x, cap, &overrun);
        }
        if (conn8) {
            if (x > 0 && value(x - 1, y + 1) == v) cc_union_agent(par, y * W + x, (y + 1) * W + x - 1, cap, &overrun);
            if (x + 1 < W && value(x + 1, y + 1) == v) cc_union_agent(par, y * W + x, (y + 1) * W + x + 1, cap, &overrun);
        }
    }
    if (overrun) status[b] = 1;
}

// one wave per (frame, row, 64 columns); segs = B H cw of them
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int32_t* __restrict__ parent, int H, int W, int cw, int segs, int cap,
                                                                int32_t* __restrict__ ids, unsigned long long* __restrict__ mask,
                                                                int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long long seg64 = (long long)blockIdx.x * (CC_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (seg64 >= segs) return;
    const int seg = (int)seg64;
    const int row = seg / cw, cx = seg - row * cw;                      // row = b H + y
    const int b = row / H, x = cx * 64 + lane;
    const size_t base = (size_t)b * H * W;
    const int own = (row - b * H) * W + x;
    int r = -1, overrun = 0;
    if (x < W) {
        r = parent[base + own];
        if (r >= 0) {
            for (int steps = 0;; ++steps) {
                const int p = parent[base + r];
                if (p == r) break;
                if (steps >= cap) {
                    overrun = 1;
                    break;
                }
                r = p;
            }
        }
        ids[base + own] = r;
    }
    const unsigned long long m = __ballot(x < W && r == own);
    if (lane == 0) mask[seg] = m;
    if (overrun) status[b] = 1;
}

// one workgroup per frame.  Thread t owns the segments [t per, (t + 1) per): their popcounts, then the exclusive prefix.
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_scan_kernel(const unsigned long long* __restrict__ mask, int S, int H, int W, int M,
                                                                  int32_t* __restrict__ off, int32_t* __restrict__ count,
                                                                  int32_t* __restrict__ first, int32_t* __restrict__ label,
                                                                  int32_t* __restrict__ area, int32_t* __restrict__ box) {
    __shared__ int wave_total[CC_SCAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int per = (S + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;
    const int e0 = min(S, tid * per), e1 = min(S, e0 + per);
    const unsigned long long* mk = mask + (size_t)b * S;
    int mine = 0;
    for (int e = e0; e < e1; ++e) mine += __popcll(mk[e]);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < CC_SCAN_WAVES; ++w) {
        const int v = wave_total[w];
        if (w < wave) before += v;
        total += v;
    }
    int run = before + incl - mine;
    for (int e = e0; e < e1; ++e) {
        off[(size_t)b * S + e] = run;
        run += __popcll(mk[e]);
    }
    if (tid == 0) count[b] = total;
    // the table's start values: rows of components wait for the label launch's min / max / add; the others hold the sentinel
    const int live = min(total, M);
    for (int k = tid; k < M; k += CC_SCAN_THREADS) {
        const size_t row = (size_t)b * M + k;
        const bool on = k < live;
        area[row] = 0;
        box[4 * row + 0] = on ? W : 0;
        box[4 * row + 1] = 0;
        box[4 * row + 2] = 0;
        box[4 * row + 3] = 0;
        if (!on) {
            first[row] = -1;
            label[row] = -1;
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_label_kernel(const int32_t* __restrict__ labels, const unsigned long long* __restrict__ mask,
                                                              const int32_t* __restrict__ off, int H, int W, int cw, int segs, int M,
                                                              int32_t* ids, int32_t* __restrict__ first, int32_t* __restrict__ label,
                                                              int32_t* area, int32_t* box) {
    const int lane = threadIdx.x & 63;
    const long long seg64 = (long long)blockIdx.x * (CC_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (seg64 >= segs) return;
    const int seg = (int)seg64;
    const int row = seg / cw, cx = seg - row * cw;
    const int b = row / H, y = row - b * H, x = cx * 64 + lane, S = H * cw;
    const size_t base = (size_t)b * H * W;
    const int own = y * W + x;
    int num = -1;
    if (x < W) {
        const int r = ids[base + own];
        if (r >= 0) {
            const int ry = r / W, rx = r - ry * W;
            const size_t rs = (size_t)b * S + (size_t)ry * cw + (rx >> 6);
            num = off[rs] + __popcll(mask[rs] & ((1ull << (rx & 63)) - 1ull));
            if (r == own && num < M) {                                  // the root: the first pixel of its component
                const size_t trow = (size_t)b * M + num;
                first[trow] = own;
                label[trow] = labels[base + own];
                box[4 * trow + 1] = y;                                  // (nobody else writes y0: the first pixel has the smallest y)
            }
        }
        ids[base + own] = num;
    }
    // one set of atomics per distinct number of the wave
    const bool todo = num >= 0 && num < M;
    unsigned long long pending = __ballot(todo);
    while (pending) {
        const int leader = __builtin_ctzll(pending);
        const int lnum = __shfl(num, leader);
        const unsigned long long m = __ballot(todo && num == lnum);
        if (lane == leader) {
            const size_t trow = (size_t)b * M + lnum;
            const int x0 = cx * 64 + __builtin_ctzll(m), x1 = cx * 64 + 64 - __builtin_clzll(m);
            atomicAdd(&area[trow], __popcll(m));
            // (min / max only ever improve: a read that already shows a value at least as good makes the atomic redundant, however stale)
            if (cc_load(&box[4 * trow + 0]) > x0) atomicMin(&box[4 * trow + 0], x0);
            if (cc_load(&box[4 * trow + 2]) < x1) atomicMax(&box[4 * trow + 2], x1);
            if (cc_load(&box[4 * trow + 3]) < y + 1) atomicMax(&box[4 * trow + 3], y + 1);
        }
        pending &= ~m;
    }
}

bool cc_shape_ok(int B, int H, int W) {
    return B >= 1 && H >= 1 && W >= 1 && H <= CC_MAX_SIDE && W <= CC_MAX_SIDE && (long long)B * H * W < (1ll << 31);
}

struct CcLayout {
    int cw, S;                  // segments per row, per frame
    long long mask, off, parent, bytes;
};
CcLayout cc_layout(int B, int H, int W) {
    CcLayout L;
    L.cw = (W + 63) / 64;
    L.S = H * L.cw;
    L.mask = 0;
    L.off = 8ll * B * L.S;
    L.parent = L.off + 4ll * B * L.S;
    L.bytes = (L.parent + 4ll * B * H * W + 15) & ~15ll;
    return L;
}

}  // namespace

long long components_scratch_bytes(int B, int H, int W) { return cc_shape_ok(B, H, W) ? cc_layout(B, H, W).bytes : -1; }

int launch_components(const int32_t* labels, int B, int H, int W, int connectivity, int ignore, int max_objects, int32_t* ids,
                      int32_t* count, int32_t* first, int32_t* label, int32_t* area, int32_t* box, int32_t* status, void* scratch,
                      hipStream_t s) {
    const char* who = "dinoseg_op_components";
    if (!labels || !ids || !count || !first || !label || !area || !box || !status || !scratch) {
        dinoseg_set_error("%s: null pointer", who);
        return -1;
    }
    if (!cc_shape_ok(B, H, W)) {
        dinoseg_set_error("%s: B = %d frames of %d x %d (each at least 1, sides at most %d, B H W below 2^31)", who, B, H, W, CC_MAX_SIDE);
        return -1;
    }
    if (max_objects < 1 || max_objects > CC_MAX_OBJECTS) {
        dinoseg_set_error("%s: max_objects = %d (1 .. %d)", who, max_objects, CC_MAX_OBJECTS);
        return -1;
    }
    if (connectivity != 4 && connectivity != 8) {
        dinoseg_set_error("%s: connectivity = %d (4 or 8)", who, connectivity);
        return -1;
    }
    auto misaligned = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    if (misaligned(labels, 3) || misaligned(ids, 3) || misaligned(count, 3) || misaligned(first, 3) || misaligned(label, 3) ||
        misaligned(area, 3) || misaligned(box, 3) || misaligned(status, 3) || misaligned(scratch, 15)) {
        dinoseg_set_error("%s: a 32-bit array must be 4-byte aligned, the scratch 16-byte aligned", who);
        return -1;
    }
    const CcLayout L = cc_layout(B, H, W);
    char* sc = reinterpret_cast<char*>(scratch);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(sc + L.mask);
    int32_t* off = reinterpret_cast<int32_t*>(sc + L.off);
    int32_t* parent = reinterpret_cast<int32_t*>(sc + L.parent);
    const int conn8 = connectivity == 8, cap = H * W, M = max_objects;
    const int tiles_x = (W + CC_TW - 1) / CC_TW, tiles_y = (H + CC_TH - 1) / CC_TH;
    const int vx = (W - 1) / CC_TW, hy = (H - 1) / CC_TH;
    const int per_frame = vx * H + hy * W, groups = (per_frame + CC_THREADS - 1) / CC_THREADS;
    const long long segs = (long long)B * L.S;                          // (< 2^31: B H W is)
    const unsigned seg_groups = (unsigned)((segs + CC_THREADS / 64 - 1) / (CC_THREADS / 64));

    DSEG_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)B, s));
    hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)((long long)B * tiles_x * tiles_y)), dim3(CC_THREADS), 0, s, labels, H, W, tiles_x,
                       tiles_y, conn8, ignore, parent, status);
    DSEG_CHECK_HIP(hipGetLastError());
    if (per_frame > 0) {
        hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((long long)B * groups)), dim3(CC_THREADS), 0, s, labels, H, W, vx, hy, per_frame,
                           groups, conn8, ignore, cap, parent, status);
        DSEG_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(seg_groups), dim3(CC_THREADS), 0, s, parent, H, W, L.cw, (int)segs, cap, ids, mask, status);
    DSEG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)B), dim3(CC_SCAN_THREADS), 0, s, mask, L.S, H, W, M, off, count, first, label, area,
                       box);
    DSEG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_label_kernel, dim3(seg_groups), dim3(CC_THREADS), 0, s, labels, mask, off, H, W, L.cw, (int)segs, M, ids, first,
                       label, area, box);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
