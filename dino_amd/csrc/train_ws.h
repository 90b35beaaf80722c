// Internal: what the two halves of the fine-tune step share -- train_api.hip (the training forward, the dense step, the C entries) and
// backward.hip (the backward): the layout of the training workspace and typed pointers into it, the gradient GEMM helpers the
// backward's stages and the dinoseg_op_* entries both run, and the growth of a library-owned device buffer.
#pragma once
#include <string.h>

#include "forward_steps.h"

constexpr size_t DET_FLOATS = (size_t)1024 * 3 * 1024;      // option deterministic: scratch for per-block partial sums (12 MiB) ...
constexpr size_t DET_TN_FLOATS = (size_t)768 * 3072;        // ... and gemm_tn's per-slice bias partials, one region per stream (2 x 9 MiB)
constexpr int SPLITK_TILES = 768;      // partial 128x128 fp32 tiles of one weight-gradient GEMM (48 MiB): what the workspace holds
static inline int splitk_budget() {
    const int v = dseg::options().splitk_tiles;
    return v < 1 ? 1 : v > SPLITK_TILES ? SPLITK_TILES : v;
}
static inline int pad128(int v) { return (v + 127) / 128 * 128; }

struct TrainLayout {
    int n, ntok, npad, M, Mp, Mpad, Mppad, Cmax;
    // per block (offsets are for block 0; block l adds l * blk_stride)
    size_t Xin, A1, Q, K, V, LSE, CTX, Xmid, A2, HPRE, HB, blk_stride;
    size_t Xfin, PATCH, FEAT, H1, H2, LOGP, DZ;
    size_t dX, dA, dXp, G, dCTX, T1, T2, NLSE, NDEL, DPOS, SINK, ACC, SPLITK, DET;
    size_t zero_begin, zero_end;      // Q/K/V of every block (pad rows must be FINITE, zero is not required: fresh memory is zeroed once)
    size_t total;
    long a_plane, qkv_plane, f_plane, feat_plane, h1_plane, h2_plane, dz_plane, patch_plane, g_plane, t_plane;
    size_t t2_bytes;
};

static inline TrainLayout make_train_layout(const dinoseg_handle* h, int B, int Hf, int Wf) {
    const dinoseg_config& c = h->cfg;
    const int D = c.embed_dim, F = D * c.mlp_ratio, P = h->planes, HP = head_planes();
    TrainLayout L;
    memset(&L, 0, sizeof(L));
    L.n = (Hf / c.patch) * (Wf / c.patch);
    L.ntok = L.n + 1;
    L.npad = (L.ntok + 63) / 64 * 64;
    L.M = B * L.ntok;
    L.Mp = B * L.n;
    L.Mpad = (L.M + 63) / 64 * 64;
    L.Mppad = (L.Mp + 63) / 64 * 64;
    L.Cmax = 3 * D > F ? 3 * D : F;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    L.a_plane = (long)L.M * D;
    L.qkv_plane = (long)B * c.num_heads * L.npad * 64;
    L.f_plane = (long)L.M * F;
    // block 0
    const size_t b0 = off;
    L.Xin = take((size_t)L.M * D * 4);
    L.A1 = take((size_t)P * L.a_plane * 2);
    L.Q = take((size_t)P * L.qkv_plane * 2);
    L.K = take((size_t)P * L.qkv_plane * 2);
    L.V = take((size_t)P * L.qkv_plane * 2);
    L.LSE = take((size_t)B * c.num_heads * L.ntok * 4);
    L.CTX = take((size_t)P * L.a_plane * 2);
    L.Xmid = take((size_t)L.M * D * 4);
    L.A2 = take((size_t)P * L.a_plane * 2);
    L.HPRE = take((size_t)P * L.f_plane * 2);
    L.HB = take((size_t)P * L.f_plane * 2);
    L.blk_stride = off - b0;
    off = b0 + L.blk_stride * (c.n_blocks > 0 ? c.n_blocks : 1);
    L.Xfin = take((size_t)L.M * D * 4);
    L.patch_plane = (long)L.Mp * (3 * c.patch * c.patch);      // the gather matrix: rows 192 wide at patch 8, 768 at patch 16
    L.PATCH = take((size_t)P * L.patch_plane * 2);
    L.feat_plane = (long)L.Mp * D;
    L.FEAT = take((size_t)HP * L.feat_plane * 2);
    L.h1_plane = (long)L.Mp * HEAD_H1_PAD;
    L.H1 = take((size_t)HP * L.h1_plane * 2);
    L.h2_plane = (long)L.Mp * HEAD_H2_PAD;
    L.H2 = take((size_t)HP * L.h2_plane * 2);
    L.LOGP = take((size_t)L.Mp * c.n_classes * 4);
    L.dz_plane = (long)L.Mp * dz_ld(c.n_classes);
    L.DZ = take((size_t)HP * L.dz_plane * 2);
    // backward scratch
    L.dX = take((size_t)L.M * D * 4);
    L.dA = take((size_t)L.M * D * 4);
    L.dXp = take((size_t)2 * L.a_plane * 2);
    L.g_plane = (long)L.M * L.Cmax;
    L.G = take((size_t)2 * L.g_plane * 2);
    {   // d ctx planes [M, D]; also hosts the head's d h1 planes [Mp, 256]
        const size_t e = (size_t)L.a_plane > (size_t)L.h1_plane ? (size_t)L.a_plane : (size_t)L.h1_plane;
        L.dCTX = take(2 * e * 2);
    }
    {   // a transposed plane holds the widest operand of a weight gradient: a block linear (Cmax rows), or the patch matrix, whose
        // round_up(3 p^2, 128) rows exceed Cmax only for a narrow model at patch 16 (768 rows against 512 at embed_dim 128)
        const int patch_rows = pad128(3 * c.patch * c.patch);
        L.t_plane = (long)(L.Cmax > patch_rows ? L.Cmax : patch_rows) * L.Mpad;
    }
    L.T1 = take((size_t)2 * L.t_plane * 2);
    {   // ... T2 also hosts the row pass of the pos-embed gradient, [pos_grid][W/patch][D] floats: a strip a few patches high (8 x 480)
        // has fewer token rows than that (on every frame of at least 7 x 7 patches the planes are the larger)
        const size_t t_bytes = (size_t)2 * L.t_plane * 2, pos_bytes = (size_t)c.pos_grid * (Wf / c.patch) * D * sizeof(float);
        L.T2 = take(t_bytes > pos_bytes ? t_bytes : pos_bytes);
        L.t2_bytes = t_bytes > pos_bytes ? t_bytes : pos_bytes;
    }
    L.NLSE = take((size_t)B * c.num_heads * L.npad * 4);
    L.NDEL = take((size_t)B * c.num_heads * L.npad * 4);
    L.DPOS = take((size_t)L.ntok * D * 4);
    L.SINK = take((size_t)4 * 1024 * 4);
    L.ACC = take(256);        // nll_loss accumulators {sum of -logp[y], valid rows} (the sticky bad-label flag lives in the handle)
    {   // split-K partial tiles of the weight gradients.  gemm_tn writes one partial tile per 128 x 128 tile of dW even unsplit, and the
        // largest block linear has (Cmax / 128) x (D / 128) of them: more than the budget from embed_dim x hidden > 768 x 128 x 128 on
        // (embed_dim 1024 at mlp_ratio 13), where the partials would run into the deterministic scratch behind them
        const size_t lin_tiles = (size_t)(L.Cmax / 128) * (D / 128);
        L.SPLITK = take((lin_tiles > (size_t)SPLITK_TILES ? lin_tiles : (size_t)SPLITK_TILES) * 128 * 128 * 4);
    }
    L.DET = take((size_t)(DET_FLOATS + 2 * DET_TN_FLOATS) * 4);       // option deterministic: per-block partial sums (the largest user: LayerNorm backward, 1024 blocks x 3 x D)
    L.total = off;
    return L;
}

// typed pointers into the training workspace: the saved activations the forward writes and the backward reads
struct BlockWs {
    float *Xin, *Xmid, *LSE;
    bf16_t *A1, *Q, *K, *V, *CTX, *A2, *HPRE, *HB;
};
struct HeadWs {
    float *Xfin, *LOGP;
    bf16_t *FEAT, *H1, *H2;
};
struct TrainWs {
    char* base;
    const TrainLayout& L;
    float* f32(size_t o) const { return reinterpret_cast<float*>(base + o); }
    bf16_t* b16(size_t o) const { return reinterpret_cast<bf16_t*>(base + o); }
    BlockWs block(int l) const {
        const size_t o = l * L.blk_stride;
        return {f32(L.Xin + o), f32(L.Xmid + o), f32(L.LSE + o), b16(L.A1 + o), b16(L.Q + o), b16(L.K + o), b16(L.V + o),
                b16(L.CTX + o), b16(L.A2 + o), b16(L.HPRE + o), b16(L.HB + o)};
    }
    HeadWs head() const { return {f32(L.Xfin), f32(L.LOGP), b16(L.FEAT), b16(L.H1), b16(L.H2)}; }
};

// A library-owned device buffer of at least `need` bytes.  Growing frees the old one behind whatever stream s still runs on it; the
// contents are not kept.  The call site resets what it derives from the contents
static inline int grow_device_buffer(char*& p, size_t& cap, size_t need, hipStream_t s) {
    if (need <= cap) return 0;
    if (p) {
        DSEG_CHECK_HIP(hipStreamSynchronize(s));
        DSEG_CHECK_HIP(hipFree(p));
    }
    p = nullptr;
    cap = 0;
    DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&p), need));
    cap = need;
    return 0;
}

// ------------------------------------------------------------------------------------------------ gradient GEMMs
struct Planes {             // a 16-bit row-major operand: [planes][rows][ld]
    const bf16_t* p;
    long plane;
    int ld;
};

// dX[M, N] = dY[M, K] . W^T[N, K]^T through the 128x128 NT kernel (gemm.hip) with a backward epilogue: EPI_PLAIN -> out_f32,
// EPI_BF16 -> out_bf16, EPI_DRELU / EPI_DGELU -> out_bf16 = (dY . W) * act'(aux)
struct Dgrad {
    Planes dY;
    const bf16_t* Wt; long w_plane;         // the transposed packed weight planes [N_pad][K_pad] (LinearGrad::tw)
    int M, N, K, planes, epi;
    float* out_f32; int ldo_f32;
    bf16_t* out_bf16; long out_plane; int ldo;
    const bf16_t* aux; long aux_plane;      // the saved pre-activation (row stride ldo)
};
static inline int run_dgrad(const Dgrad& a, hipStream_t s) {
    GemmParams g = {};
    g.A = a.dY.p; g.a_plane = a.dY.plane; g.lda = a.dY.ld; g.W = a.Wt; g.w_plane = a.w_plane;
    g.M = a.M; g.N = a.N; g.K = a.K; g.planes = a.planes; g.epi = a.epi;
    g.out_f32 = a.out_f32; g.ldo_f32 = a.ldo_f32;
    g.out_bf16 = a.out_bf16; g.out_plane = a.out_plane; g.ldo = a.ldo; g.aux_in = a.aux; g.aux_plane = a.aux_plane;
    return launch_gemm_small(g, s);
}

// dW[N, k_cols] = dY^T . X straight from the row-major dY [M][N] and layer-input planes X [M][Kc] (gemm_tn.hip: no operand transposes):
// ksplit slices of the batch rows write partial tiles to `part`, one pass sums the slices that own 32-row chunks into dW.
// colsum (optional): the layer's bias gradient = column sums of dY, taken inside the kernel; dW null: the column sums alone.
// Kc >= k_cols: the stored width of X, a multiple of 128 (the classifier's zero-padded hidden activations): the kernel multiplies
// all Kc columns, the reduce writes the first k_cols
struct WgradTn {
    Planes Y, X;
    int M, N, Kc, planes;
    int ksplit;
    float* part;                // [ksplit][round_up(N, 128)][Kc] (the kernel always writes its partial tiles there)
    float* dW; int ldw, k_cols;
    float* colsum;
    int det_region;             // TnParams::det_region
};
static inline int run_wgrad_tn(const WgradTn& a, hipStream_t s) {
    TnParams g = {};
    g.Y = a.Y.p; g.y_plane = a.Y.plane; g.ldy = a.Y.ld; g.X = a.X.p; g.x_plane = a.X.plane; g.ldx = a.X.ld;
    g.M = a.M; g.N = a.N; g.Kc = a.Kc; g.planes = a.planes;
    g.part = a.part; g.ld_part = a.Kc; g.split_stride = (long)pad128(a.N) * a.Kc; g.ksplit = a.ksplit;
    g.colsum = a.colsum;
    g.det_region = a.det_region;
    DSEG_TRY(launch_gemm_tn(g, s));
    if (!a.dW) return 0;
    const int nchunks = (a.M + 31) / 32, per = (nchunks + a.ksplit - 1) / a.ksplit, used = (nchunks + per - 1) / per;
    return launch_splitk_reduce(a.part, used, g.split_stride, a.N, a.Kc, a.dW, a.ldw, a.k_cols, s);
}
// the step's slice count for it: as many as the split-K budget (option splitk_tiles, clamped) allows, at least four chunks each
static inline int tn_slices(int budget, bool plain_grid, int m_rows, int n_rows, int Kc) {
    const int tiles = (pad128(n_rows) / 128) * (Kc / 128), nchunks = (m_rows + 31) / 32;
    int ks = budget / tiles;
    if (ks > nchunks / 4) ks = nchunks / 4;
    if (ks >= 8 && !plain_grid) ks &= ~7;      // a multiple of 8: the kernel's XCD-aware form (gemm_tn.hip); plain_grid = option route_ab & 4
    return ks < 1 ? 1 : ks;
}

// batch slices of the narrow-layer weight gradient below: as many as the budget allows, at least two k-steps each
static inline int wgrad_nt_slices(int budget, int n_rows, int k_pad128, int m_pad) {
    const int tiles = ((n_rows + 127) / 128) * (k_pad128 / 128), nk = m_pad / 64;
    int ks = budget / tiles;
    if (ks > nk / 2) ks = nk / 2;
    return ks < 1 ? 1 : ks;
}

// dW[n_rows, k_cols] += dY^T . X  from transposed planes T_dy [n_pad][m_pad], T_x [k_pad128][m_pad] (NT kernel, the batch rows as
// the contraction).  ks == 1: fp32 atomics straight into dW; ks > 1: slices of the batch write partial tiles to `part` (plain
// stores), one pass sums the slices that own k-steps into dW.
static inline int wgrad_nt(const bf16_t* Tdy, const bf16_t* Tx, long tplane, int m_pad, int n_rows, int k_pad128, int k_cols, int planes,
                           int ks, float* part, float* dW, hipStream_t s) {
    GemmParams g = {};
    g.A = Tdy; g.a_plane = tplane; g.lda = m_pad; g.W = Tx; g.w_plane = tplane;
    g.M = n_rows; g.N = k_pad128; g.K = m_pad; g.planes = planes;
    if (ks == 1) {
        g.epi = EPI_ATOMIC;
        g.out_f32 = dW; g.ldo_f32 = k_cols; g.n_valid = k_cols;
        g.ksplit = 1;
        return launch_gemm_small(g, s);
    }
    const int nk = m_pad / 64, row_tiles = (n_rows + 127) / 128;
    const int per = (nk + ks - 1) / ks, used = (nk + per - 1) / per;       // slices that own k-steps (gemm.hip)
    g.epi = EPI_PLAIN;
    g.out_f32 = part; g.ldo_f32 = k_pad128; g.ksplit = ks;
    g.split_stride = (long)row_tiles * 128 * k_pad128;
    DSEG_TRY(launch_gemm_small(g, s));
    return launch_splitk_reduce(part, used, g.split_stride, n_rows, k_pad128, dW, k_cols, k_cols, s);
}

// backward.hip: the backward of the last training forward, joined with the side stream on every way out
int backward_joined(dinoseg_handle* h, const int64_t* labels, const float* dlogp, float* loss_out, hipStream_t s);
