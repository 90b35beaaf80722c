// CLS attention maps of the last block at pixel resolution (the reference's visualize_attention.py: attentions[0, :, 0, 1:], enlarged
// by the patch size with nearest-neighbour, optionally thresholded by dt_utils.process_attentions) in ONE launch behind the last
// block's LayerNorm1 + qkv -- without the [B, heads, N, N] matrix of get_last_selfattention, of which this is one row in N.
//
// One workgroup of 1024 threads (16 waves) per (frame, head).  Everything between K and the output lives in LDS (dynamic, ntok + 128
// words):
//   scores   s_n = q_0 . k_n for ALL ntok keys, the CLS query row (token 0, planes summed in fp32) against every key: 8 lanes per key,
//            each one 16-byte load per plane and an 8-term fp32 FMA chain, then the 3-step xor tree over the 8 lanes.  K is read once;
//            a wave instruction reads 1 KiB of consecutive rows and a wave has 8 of them in flight (the loop is bound by the latency
//            of HBM, not by arithmetic).  Rows >= ntok are never read.
//   softmax  over all ntok keys in the log2 domain (Q is pre-scaled by head_dim^-0.5 log2 e): p_n = exp2(s_n - max) * (1 / sum); max
//            and sum are reduced in a fixed order (a thread's keys ascending, the xor tree of a wave, the 16 waves ascending).
//   cut      (keep_out only) the integer rule of include/dinoseg.h: q_j = rint(p_j 2^30) over the patches j = 1 .. ntok-1, T = sum q_j,
//            keep j iff S_le(q_j) 2^24 > (2^24 - t) T.  S_le is monotone, so "keep j" is "q_j >= c" for the smallest value c whose
//            S_le passes the test: 31 bisection steps on the bits of c, each one pass over the patches in LDS and one block sum of
//            32-bit integers (S_le <= T < 2^31).  Integer sums do not depend on their order.  q is monotone in p, so "q_j >= c" is
//            "p_j >= the smallest kept p" (a block minimum): the output pass compares floats.  No atomics.
//   output   attn_out fp32 / keep_out uint8 [B, heads, OH, OW] by nearest neighbour with exact integer coordinates sy = (oy hp) / OH,
//            sx = (ox wp) / OW.  With OW % 4 == 0 and aligned outputs a lane owns 4 consecutive pixels of a row: one 16-byte store of
//            attn and one 4-byte store of keep, consecutive lanes consecutive addresses; otherwise one pixel per lane.  A thread keeps
//            its columns (their sx are formed once) and walks down a band of consecutive rows; sy advances by carry (acc += hp, a
//            step when acc passes OH: the division's own floor), and the values are read from LDS again only when sy moves -- at an
//            8x enlargement one read serves 8 rows.
#include "common.h"
#include "kernels.h"

namespace dseg {

namespace {

constexpr int CLS_THREADS = 1024, CLS_WAVES = CLS_THREADS / 64;
constexpr int CLS_UNROLL = 8;                                           // groups of 8 keys a wave loads before it consumes them
constexpr int CLS_LDS_WORDS = 40960;                                    // the CU's whole 160 KiB
constexpr int CLS_FIXED_WORDS = 128;                                    // the query row [64], the reduction slots [2][16] + [2][16]
constexpr int CLS_ATTN_MAX_TOKENS = CLS_LDS_WORDS - CLS_FIXED_WORDS;    // the scores of one (frame, head) beside the fixed use
constexpr int CLS_DEFAULT_LDS_BYTES = 64 * 1024;                        // beyond it a launch needs the opt-in
constexpr long long CLS_MAX_GRID = 0x7fffffffll;                        // workgroups along grid x

__device__ __forceinline__ uint32_t cls_quant(float p) { return (uint32_t)__builtin_rintf(p * 1073741824.0f); }

// eight consecutive 16-bit elements -> fp32 (+= when ADD)
template <bool ADD>
__device__ __forceinline__ void cls_unpack8(const uint4& h, int fmt, float (&v)[8]) {
    const uint32_t w[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = fmt == FMT_FP16 ? lo_to_f32<FMT_FP16>(w[e]) : bf16_lo_to_f32(w[e]);
        const float b = fmt == FMT_FP16 ? hi_to_f32<FMT_FP16>(w[e]) : bf16_hi_to_f32(w[e]);
        if (ADD) {
            v[2 * e] += a;
            v[2 * e + 1] += b;
        } else {
            v[2 * e] = a;
            v[2 * e + 1] = b;
        }
    }
}

// the nearest gather of one (frame, head): V pixels per lane; a pixel is kept iff its probability is >= pmin
template <int V>
__device__ __forceinline__ void cls_store(const float* __restrict__ pr, int hp, int wp, int OH, int OW, float pmin,
                                          float* __restrict__ attn, uint8_t* __restrict__ keep) {
    const int tid = threadIdx.x;
    const int WV = OW / V;                                              // items of a row (V == 4: OW % 4 == 0)
    const int TX = WV < CLS_THREADS ? WV : CLS_THREADS, TY = CLS_THREADS / TX;      // threads along a row, bands of rows
    const int tx = tid % TX, ty = tid / TX;
    const int R = (OH + TY - 1) / TY;                                   // rows of a band
    const int y0 = ty * R, y1 = y0 + R < OH ? y0 + R : OH;
    if (ty >= TY || y0 >= y1) return;
    for (int xb = tx; xb < WV; xb += TX) {
        int sx[V];
#pragma unroll
        for (int e = 0; e < V; ++e) sx[e] = (int)(((unsigned)(xb * V + e) * (unsigned)wp) / (unsigned)OW);
        const unsigned t0 = (unsigned)y0 * (unsigned)hp;
        int sy = (int)(t0 / (unsigned)OH);
        int acc = (int)(t0 - (unsigned)sy * (unsigned)OH);              // (oy hp) % OH
        float p[V];
        uint32_t kw = 0;
        auto load = [&]() {
            const float* row = pr + sy * wp;
            kw = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                p[e] = row[sx[e]];
                kw |= (p[e] >= pmin ? 1u : 0u) << (8 * e);
            }
        };
        load();
        size_t o = (size_t)y0 * OW + (size_t)xb * V;
        for (int oy = y0; oy < y1; ++oy, o += OW) {
            if (attn) {
                if constexpr (V == 4) *reinterpret_cast<float4*>(attn + o) = make_float4(p[0], p[1], p[2], p[3]);
                else attn[o] = p[0];
            }
            if (keep) {
                if constexpr (V == 4) *reinterpret_cast<uint32_t*>(keep + o) = kw;
                else keep[o] = (uint8_t)kw;
            }
            acc += hp;
            if (acc >= OH) {                                            // (OH >= hp: at most one step a row)
                acc -= OH;
                ++sy;
                if (oy + 1 < y1) load();
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(CLS_THREADS) void cls_attention_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, long plane,
                                                                    int planes, int ntok, int npad, int hp, int wp, int OH, int OW,
                                                                    uint32_t t24, float* __restrict__ attn_out,
                                                                    uint8_t* __restrict__ keep_out, int fmt) {
    extern __shared__ float cls_lds[];
    float* qs = cls_lds;                                                // [64] the CLS query row
    float* redf = cls_lds + 64;                                         // [2][16]: the waves' maxima / minima, the waves' sums
    uint32_t* redu = reinterpret_cast<uint32_t*>(cls_lds + 96);         // [2][16]: the waves' integer sums, two steps alternating
    float* sc = cls_lds + CLS_FIXED_WORDS;                              // [ntok] scores -> exponentials -> probabilities
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bf16_t* Qg = q + (long)pair * npad * 64;
    const bf16_t* Kg = k + (long)pair * npad * 64;
    if (tid < 64) {
        float v = unpack1(Qg[tid], fmt);
        if (planes == 2) v += unpack1(Qg[plane + tid], fmt);
        qs[tid] = v;
    }
    __syncthreads();

    // ---- scores: lane = (key of a group of 8) x (16-byte chunk of the row); CLS_UNROLL groups per wave and pass
    {
        const int sub = lane >> 3, ch = lane & 7;
        float qv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = qs[ch * 8 + e];
        for (int k0 = wv * (8 * CLS_UNROLL); k0 < ntok; k0 += CLS_WAVES * 8 * CLS_UNROLL) {
            uint4 hi[CLS_UNROLL], lo[CLS_UNROLL];
#pragma unroll
            for (int u = 0; u < CLS_UNROLL; ++u) {
                const int key = k0 + u * 8 + sub;
                const int kr = key < ntok ? key : ntok - 1;             // (a lane beyond the last key reads the last key: never a pad row)
                const bf16_t* src = Kg + (long)kr * 64 + ch * 8;
                hi[u] = *reinterpret_cast<const uint4*>(src);
                if (planes == 2) lo[u] = *reinterpret_cast<const uint4*>(src + plane);
            }
#pragma unroll
            for (int u = 0; u < CLS_UNROLL; ++u) {
                const int key = k0 + u * 8 + sub;
                float kv[8];
                cls_unpack8<false>(hi[u], fmt, kv);
                if (planes == 2) cls_unpack8<true>(lo[u], fmt, kv);
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qv[e], kv[e], s);
                s += __shfl_xor(s, 1);
                s += __shfl_xor(s, 2);
                s += __shfl_xor(s, 4);
                if (ch == 0 && key < ntok) sc[key] = s;
            }
        }
    }
    __syncthreads();

    // ---- softmax over all ntok keys
    float mx = -INFINITY;
    for (int n = tid; n < ntok; n += CLS_THREADS) mx = fmaxf(mx, sc[n]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) redf[wv] = mx;
    __syncthreads();
    mx = redf[0];
#pragma unroll
    for (int w = 1; w < CLS_WAVES; ++w) mx = fmaxf(mx, redf[w]);
    float sum = 0.f;
    for (int n = tid; n < ntok; n += CLS_THREADS) {
        const float e = __builtin_amdgcn_exp2f(sc[n] - mx);
        sc[n] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) redf[16 + wv] = sum;
    __syncthreads();
    sum = redf[16];
#pragma unroll
    for (int w = 1; w < CLS_WAVES; ++w) sum += redf[16 + w];
    const float inv = 1.0f / sum;
    for (int n = tid; n < ntok; n += CLS_THREADS) sc[n] *= inv;         // (a thread rewrites its own words: no barrier in between)
    __syncthreads();

    // ---- the cut: the smallest c with S_le(c) 2^24 > (2^24 - t) T; no such c leaves 2^31 - 1, above every q_j <= 2^30
    float pmin = INFINITY;
    if (keep_out) {
        auto block_sum = [&](uint32_t v, int slot) -> uint32_t {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) redu[slot * 16 + wv] = v;
            __syncthreads();
            uint32_t t = 0;
#pragma unroll
            for (int w = 0; w < CLS_WAVES; ++w) t += redu[slot * 16 + w];
            return t;
        };
        uint32_t part = 0;
        for (int n = 1 + tid; n < ntok; n += CLS_THREADS) part += cls_quant(sc[n]);
        const uint64_t T = block_sum(part, 0);
        const uint64_t R = (uint64_t)(16777216u - t24) * T;
        uint32_t cut = 0;
        int slot = 1;
        for (int bit = 30; bit >= 0; --bit, slot ^= 1) {
            const uint32_t trial = cut | (1u << bit);                   // is S_le(trial - 1) still short?  then c >= trial
            part = 0;
            for (int n = 1 + tid; n < ntok; n += CLS_THREADS) {
                const uint32_t qj = cls_quant(sc[n]);
                part += qj < trial ? qj : 0u;
            }
            // (slot alternates: a wave that runs ahead writes the other slot; the one it wrote two steps ago was read by everyone before
            // the barrier of the step in between)
            const uint64_t S = block_sum(part, slot);
            if ((S << 24) <= R) cut = trial;
        }
        // the smallest kept probability (redf's first half was last read before the barriers above)
        for (int n = 1 + tid; n < ntok; n += CLS_THREADS) {
            const float p = sc[n];
            if (cls_quant(p) >= cut) pmin = fminf(pmin, p);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pmin = fminf(pmin, __shfl_xor(pmin, o));
        if (lane == 0) redf[wv] = pmin;
        __syncthreads();
        pmin = redf[0];
#pragma unroll
        for (int w = 1; w < CLS_WAVES; ++w) pmin = fminf(pmin, redf[w]);
    }

    const size_t o = (size_t)pair * OH * OW;
    cls_store<V>(sc + 1, hp, wp, OH, OW, pmin, attn_out ? attn_out + o : nullptr, keep_out ? keep_out + o : nullptr);
}

int allow_large_lds() {
    static PerDeviceOnce once;
    if (!once.first()) return 0;
    const void* fn[2] = {reinterpret_cast<const void*>(&cls_attention_kernel<4>), reinterpret_cast<const void*>(&cls_attention_kernel<1>)};
    for (int i = 0; i < 2; ++i) {
        const hipError_t e = hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, CLS_LDS_WORDS * (int)sizeof(float));
        if (e != hipSuccess) {
            dinoseg_set_error("hipFuncSetAttribute(cls_attention_kernel<%d>, MaxDynamicSharedMemorySize) failed: %s", i ? 1 : 4,
                              hipGetErrorString(e));
            return -2;
        }
    }
    once.mark();
    return 0;
}

}  // namespace

int cls_attention_max_tokens() { return CLS_ATTN_MAX_TOKENS; }

int cls_attention_check(const char* who, int B, int heads, int ntok, int hp, int wp, int OH, int OW, bool want_keep, float threshold) {
    if (B < 1 || heads < 1 || hp < 1 || wp < 1) {
        dinoseg_set_error("%s: bad argument (B=%d heads=%d hp=%d wp=%d; sizes must be positive)", who, B, heads, hp, wp);
        return -1;
    }
    if ((long long)hp * wp + 1 != (long long)ntok) {
        dinoseg_set_error("%s: ntok=%d is not hp*wp + 1 (hp=%d wp=%d)", who, ntok, hp, wp);
        return -1;
    }
    if (OH < hp || OW < wp) {
        dinoseg_set_error("%s: output %dx%d is smaller than the patch grid %dx%d (enlarging and identity only)", who, OH, OW, hp, wp);
        return -1;
    }
    if (want_keep && !(threshold > 0.f && threshold < 1.f)) {
        dinoseg_set_error("%s: threshold=%g must be inside (0, 1)", who, (double)threshold);
        return -1;
    }
    if ((long long)B * heads > CLS_MAX_GRID) {
        dinoseg_set_error("%s: B*heads=%lld workgroups exceed the grid (%lld)", who, (long long)B * heads, CLS_MAX_GRID);
        return -1;
    }
    if (ntok > CLS_ATTN_MAX_TOKENS) {
        dinoseg_set_error("%s: %d tokens exceed the %d whose scores fit the LDS of one workgroup", who, ntok, CLS_ATTN_MAX_TOKENS);
        return -1;
    }
    if ((long long)OH * OW > 0x7fffffffll || (long long)OH * hp > 0x7fffffffll || (long long)OW * wp > 0x7fffffffll) {
        dinoseg_set_error("%s: output %dx%d of a %dx%d grid is too large (32-bit products)", who, OH, OW, hp, wp);
        return -1;
    }
    return 0;
}

int launch_cls_attention(const bf16_t* q, const bf16_t* k, long plane, int planes, int B, int heads, int ntok, int npad, int hp, int wp,
                         int OH, int OW, float threshold, float* attn_out, uint8_t* keep_out, hipStream_t s, int fmt) {
    if (!q || !k || (!attn_out && !keep_out)) {
        dinoseg_set_error("cls_attention: null pointer (q, k, and at least one of attn_out / keep_out, are required)");
        return -1;
    }
    if (cls_attention_check("cls_attention", B, heads, ntok, hp, wp, OH, OW, keep_out != nullptr, threshold)) return -1;
    const size_t lds = (size_t)(CLS_FIXED_WORDS + ntok) * sizeof(float);
    if (lds > CLS_DEFAULT_LDS_BYTES) {
        const int rc = allow_large_lds();
        if (rc) return rc;
    }
    const uint32_t t24 = keep_out ? (uint32_t)__builtin_rint((double)threshold * 16777216.0) : 0u;
    const bool vec = OW % 4 == 0 && (reinterpret_cast<uintptr_t>(attn_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(keep_out) & 3) == 0;
    const dim3 grid((unsigned)(B * heads));
    if (vec)
        hipLaunchKernelGGL(cls_attention_kernel<4>, grid, dim3(CLS_THREADS), lds, s, q, k, plane, planes, ntok, npad, hp, wp, OH, OW, t24, attn_out,
                           keep_out, fmt);
    else
        hipLaunchKernelGGL(cls_attention_kernel<1>, grid, dim3(CLS_THREADS), lds, s, q, k, plane, planes, ntok, npad, hp, wp, OH, OW, t24, attn_out,
                           keep_out, fmt);
    DSEG_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace dseg
