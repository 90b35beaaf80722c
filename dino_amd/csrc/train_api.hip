// Fine-tune step of the DINOSeg hot path: forward with saved activations, backward, gradients
// written into caller-bound fp32 buffers.  Replaces DINOSeg.training_step + autograd.backward
// (pl_torch_modules.py:261-268) for one data-parallel rank; the cross-rank gradient mean is done by the caller
// (torch.distributed all_reduce over RCCL, dino_amd/parallel.py).  Host code only.
//
// Backward of y = act(x W^T + b), given dY (activation derivative already applied):
//   dX = dY . W          -> gemm.hip NT kernel with the transposed packed weight W^T[K][N] as the "W" operand
//   dW = dY^T . X        -> both operands transposed to [*, rows] planes (transpose_planes_kernel), same NT kernel
//                           with the batch rows as the contraction, split over grid.y, fp32 atomics into dW
//   db = column sums of dY (by-product of the transpose kernel)
#include <string.h>

#include <vector>

#include "forward_steps.h"

namespace {

constexpr size_t DET_FLOATS = (size_t)1024 * 3 * 1024;      // option deterministic: scratch for per-block partial sums (12 MiB) ...
constexpr size_t DET_TN_FLOATS = (size_t)768 * 3072;        // ... and gemm_tn's per-slice bias partials, one region per stream (2 x 9 MiB)
constexpr int SPLITK_TILES = 768;      // partial 128x128 fp32 tiles of one weight-gradient GEMM (48 MiB): what the workspace holds
inline int splitk_budget() {
    const int v = dseg::options().splitk_tiles;
    return v < 1 ? 1 : v > SPLITK_TILES ? SPLITK_TILES : v;
}

struct TrainLayout {
    int n, ntok, npad, M, Mp, Mpad, Mppad, Cmax;
    // per block (offsets are for block 0; block l adds l * blk_stride)
    size_t Xin, A1, Q, K, V, LSE, CTX, Xmid, A2, HPRE, HB, blk_stride;
    size_t Xfin, PATCH, FEAT, H1, H2, LOGP, DZ;
    size_t dX, dA, dXp, G, dCTX, T1, T2, NLSE, NDEL, DPOS, SINK, ACC, SPLITK, DET;
    size_t zero_begin, zero_end;      // Q/K/V of every block (pad rows must be zero)
    size_t total;
    long a_plane, qkv_plane, f_plane, feat_plane, h1_plane, h2_plane, dz_plane, patch_plane, g_plane, t_plane;
    size_t t2_bytes;
};

TrainLayout make_train_layout(const dinoseg_handle* h, int B, int Hf, int Wf) {
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
        const int patch_rows = (3 * c.patch * c.patch + 127) / 128 * 128;
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

// batch slices of the narrow-layer weight gradient below: as many as the split-K budget allows, at least two k-steps each
int wgrad_nt_slices(int n_rows, int k_pad128, int m_pad) {
    const int tiles = ((n_rows + 127) / 128) * (k_pad128 / 128), nk = m_pad / 64;
    int ks = splitk_budget() / tiles;
    if (ks > nk / 2) ks = nk / 2;
    return ks < 1 ? 1 : ks;
}

// dW[n_rows, k_cols] += dY^T . X  from transposed planes T_dy [n_pad][m_pad], T_x [k_pad128][m_pad] (NT kernel, the batch rows as
// the contraction).  ks == 1: fp32 atomics straight into dW; ks > 1: slices of the batch write partial tiles to `part` (plain
// stores), one pass sums the slices that own k-steps into dW.
int wgrad_nt(const bf16_t* Tdy, const bf16_t* Tx, long tplane, int m_pad, int n_rows, int k_pad128, int k_cols, int planes, int ks,
             float* part, float* dW, hipStream_t s) {
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

}  // namespace

int dinoseg_train_release(dinoseg_handle* h) {
    if (h->tws) (void)hipFree(h->tws);
    if (h->twbuf) (void)hipFree(h->twbuf);
    if (h->dws) (void)hipFree(h->dws);
    h->dws = nullptr;
    h->dws_bytes = 0;
    if (h->bad_label_flag) (void)hipFree(h->bad_label_flag);
    h->bad_label_flag = nullptr;
    h->tws = nullptr;
    h->twbuf = nullptr;
    h->tws_bytes = h->twbuf_bytes = 0;
    return 0;
}

extern "C" int dinoseg_bind_grad(dinoseg_handle* h, const char* name, float* dev_ptr) {
    if (!h || !name) {
        dinoseg_set_error("dinoseg_bind_grad: null argument");
        return -1;
    }
    auto it = h->grad_index.find(name);
    if (it == h->grad_index.end()) {
        dinoseg_set_error("dinoseg_bind_grad: unexpected key '%s'", name);
        return -1;
    }
    it->second->ptr = dev_ptr;
    return 0;
}

extern "C" int dinoseg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, int32_t decoupled, int32_t step, float grad_scale, void* stream) {
    if (!p || !g || !m || !v || step < 1) {
        dinoseg_set_error("dinoseg_adam_step: bad argument");
        return -1;
    }
    return launch_adam(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale,
                       reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_adam_step_multi(int32_t count, float* const* p, const float* const* g, float* const* m, float* const* v,
                                       const int64_t* n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                       int32_t decoupled, int32_t step, float grad_scale, void* stream) {
    if (count < 0 || (count > 0 && (!p || !g || !m || !v || !n)) || step < 1) {
        dinoseg_set_error("dinoseg_adam_step_multi: bad argument");
        return -1;
    }
    std::vector<long> nn(count);
    for (int i = 0; i < count; ++i) {
        if (!p[i] || !g[i] || !m[i] || !v[i] || n[i] < 0) {
            dinoseg_set_error("dinoseg_adam_step_multi: null pointer or negative size at tensor %d", i);
            return -1;
        }
        nn[i] = (long)n[i];
    }
    return launch_multi_adam(count, p, g, m, v, nn.data(), lr, beta1, beta2, eps, weight_decay, decoupled, step, grad_scale,
                             reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_attention_bwd(const void* q, const void* k, const void* v, int64_t qkv_plane, const void* dO,
                                        const void* O, int64_t o_plane, const float* lse, float* scratch, void* dqkv,
                                        int64_t dqkv_plane, int32_t B, int32_t heads, int32_t ntok, int32_t npad,
                                        int32_t planes, void* stream) {
    AttnBwdParams a = {};
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.qkv_plane = qkv_plane;
    a.dO = (const bf16_t*)dO; a.O = (const bf16_t*)O; a.dO_plane = o_plane; a.lse = lse;
    a.neg_lse = scratch; a.neg_delta = scratch + (size_t)B * heads * npad;
    a.dqkv = (bf16_t*)dqkv; a.dqkv_plane = dqkv_plane;
    a.B = B; a.heads = heads; a.ntok = ntok; a.npad = npad; a.planes = planes;
    return launch_attention_bwd(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_layernorm_bwd(const float* dy, const float* x, const float* gamma, float eps, int32_t M, int32_t D,
                                        float* dx, int32_t accumulate, float* dgamma, float* dbeta, int32_t drop_cls,
                                        int32_t ntok, void* stream) {
    return launch_layernorm_bwd(dy, x, gamma, eps, M, D, dx, accumulate, dgamma, dbeta, drop_cls, ntok,
                                reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_layernorm_bwd2(const float* dy, const float* x, const float* gamma, float eps, int32_t M, int32_t D, float* dx,
                                         int32_t accumulate, float* dgamma, float* dbeta, int32_t drop_cls, int32_t ntok, void* dxp,
                                         int64_t dxp_plane, int32_t planes, float* colsum, void* stream) {
    if (dxp && planes != 1 && planes != 2) {
        dinoseg_set_error("dinoseg_op_layernorm_bwd2: planes must be 1 or 2 (got %d)", planes);
        return -1;
    }
    return launch_layernorm_bwd(dy, x, gamma, eps, M, D, dx, accumulate, dgamma, dbeta, drop_cls, ntok,
                                reinterpret_cast<hipStream_t>(stream), (bf16_t*)dxp, dxp_plane, planes, colsum);
}

// the step's wgrad_tn with the caller's slice count: gemm_tn, then the reduce over the slices that own batch rows
extern "C" int dinoseg_op_gemm_tn(const void* Y, int64_t y_plane, int32_t ldy, const void* X, int64_t x_plane, int32_t ldx, int32_t M,
                                  int32_t N, int32_t Kc, int32_t planes, int32_t ksplit, float* part, float* dW, int32_t ldw,
                                  int32_t k_cols, float* colsum, void* stream) {
    if (!part) {        // (the kernel always writes its partial tiles there, also when only the column sums are wanted)
        dinoseg_set_error("dinoseg_op_gemm_tn: part is required");
        return -1;
    }
    if (dW && (k_cols < 1 || k_cols > Kc || ldw < k_cols)) {
        dinoseg_set_error("dinoseg_op_gemm_tn: bad output columns (k_cols=%d Kc=%d ldw=%d)", k_cols, Kc, ldw);
        return -1;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TnParams g = {};
    g.Y = (const bf16_t*)Y; g.y_plane = y_plane; g.ldy = ldy; g.X = (const bf16_t*)X; g.x_plane = x_plane; g.ldx = ldx;
    g.M = M; g.N = N; g.Kc = Kc; g.planes = planes;
    g.part = part; g.ld_part = Kc; g.split_stride = (long)((N + 127) / 128) * 128 * Kc; g.ksplit = ksplit;
    g.colsum = colsum;
    DSEG_TRY(launch_gemm_tn(g, s));
    if (!dW) return 0;
    const int nchunks = (M + 31) / 32, per = (nchunks + ksplit - 1) / ksplit, used = (nchunks + per - 1) / per;
    return launch_splitk_reduce(part, used, g.split_stride, N, Kc, dW, ldw, k_cols, s);
}

// the step's dgrad: dX[M, N] = dY[M, K] . W^T[N, K]^T through the 128x128 kernel with a backward epilogue
extern "C" int dinoseg_op_gemm_bwd(const void* A, int64_t a_plane, int32_t lda, const void* Wt, int64_t w_plane, int32_t M, int32_t N,
                                   int32_t K, int32_t planes, int32_t epi, float* out_f32, int32_t ldo_f32, void* out_bf16,
                                   int64_t out_plane, int32_t ldo, const void* aux_in, int64_t aux_plane, void* stream) {
    if (epi != EPI_PLAIN && epi != EPI_BF16 && epi != EPI_DGELU && epi != EPI_DRELU) {
        dinoseg_set_error("dinoseg_op_gemm_bwd: epi %d is not a backward epilogue (0, 6, 8, 9)", epi);
        return -1;
    }
    if ((epi == EPI_DGELU || epi == EPI_DRELU) && !aux_in) {
        dinoseg_set_error("dinoseg_op_gemm_bwd: epi %d needs aux_in", epi);
        return -1;
    }
    GemmParams g = {};
    g.A = (const bf16_t*)A; g.a_plane = a_plane; g.lda = lda; g.W = (const bf16_t*)Wt; g.w_plane = w_plane;
    g.M = M; g.N = N; g.K = K; g.planes = planes; g.epi = epi;
    g.out_f32 = out_f32; g.ldo_f32 = ldo_f32;
    g.out_bf16 = (bf16_t*)out_bf16; g.out_plane = out_plane; g.ldo = ldo; g.aux_in = (const bf16_t*)aux_in; g.aux_plane = aux_plane;
    return launch_gemm_small(g, reinterpret_cast<hipStream_t>(stream));
}

// the step's narrow-layer weight gradient (k_cols % 128 != 0: the patch embedding): dY [M][N] (fp32 rows, or bf16 planes) and X
// planes [M][K] transposed into T1 / T2 (+ the bias column sums of dY, drop_cls), then the NT kernel over the batch rows with ksplit
// slices (1: fp32 atomics into dW; else partial tiles in `part` + the reduce).  dW [N][K], row stride K.
extern "C" int dinoseg_op_wgrad_nt(const float* dy_f32, const void* dy, int64_t dy_plane, int32_t ldy, const void* x, int64_t x_plane,
                                   int32_t ldx, int32_t M, int32_t N, int32_t K, int32_t planes, int32_t drop_cls, int32_t ntok,
                                   int32_t ksplit, void* T1, void* T2, int64_t t_plane, int32_t m_pad, float* part, float* dW,
                                   float* colsum, void* stream) {
    const int n_pad = (N + 127) / 128 * 128, k_pad = (K + 127) / 128 * 128;
    if ((dy_f32 == nullptr) == (dy == nullptr) || ksplit < 1 || M < 1 || (long)n_pad * m_pad > t_plane ||
        (long)k_pad * m_pad > t_plane || (ksplit > 1 && !part)) {
        dinoseg_set_error("dinoseg_op_wgrad_nt: bad argument (M=%d N=%d K=%d m_pad=%d ksplit=%d)", M, N, K, m_pad, ksplit);
        return -1;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bf16_t *t1 = (bf16_t*)T1, *t2 = (bf16_t*)T2;
    DSEG_TRY(launch_transpose_planes(dy_f32, (const bf16_t*)dy, dy_plane, ldy, M, N, t1, t_plane, n_pad, m_pad, nullptr, 0, 0, colsum,
                                     planes, drop_cls, ntok, s));
    DSEG_TRY(launch_transpose_planes(nullptr, (const bf16_t*)x, x_plane, ldx, M, K, t2, t_plane, k_pad, m_pad, nullptr, 0, 0, nullptr,
                                     planes, 0, 0, s));
    if (!dW) return 0;
    return wgrad_nt(t1, t2, t_plane, m_pad, N, k_pad, K, planes, ksplit, part, dW, s);
}

extern "C" int dinoseg_op_nll_loss_grad(const float* logp, const int64_t* labels, const float* dlogp, int32_t M, int32_t C, float* acc,
                                        int32_t* flags, float* loss, void* dz, int64_t dz_plane, int32_t ldz, void* stream) {
    if ((labels == nullptr) == (dlogp == nullptr) || (labels && (!acc || !flags || !loss)) || M < 1 || C < 1 || ldz < C) {
        dinoseg_set_error("dinoseg_op_nll_loss_grad: needs exactly one of labels (+ acc, flags, loss) and dlogp, ldz >= C");
        return -1;
    }
    return launch_nll_loss_grad(logp, labels, dlogp, M, C, acc, flags, loss, (bf16_t*)dz, dz_plane, ldz,
                                reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_pos_resample_bwd_hw(const float* dpos, int32_t g, int32_t D, int32_t oh, int32_t ow, float* dpe, float* scratch,
                                              void* stream) {
    if (g < 1 || D < 1 || oh < 1 || ow < 1) {
        dinoseg_set_error("dinoseg_op_pos_resample_bwd_hw: bad shape g=%d D=%d oh=%d ow=%d", g, D, oh, ow);
        return -1;
    }
    return launch_pos_resample_bwd(dpos, g, D, oh, ow, dpe, scratch, reinterpret_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ the step
// Forward with saved activations (DINOSeg.forward under autograd, pl_torch_modules.py:239-256).  The saved state stays valid
// until the next call; train_backward_impl consumes it.
static int train_forward_impl(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t Hf, int32_t Wf, float* logp_out,
                              hipStream_t s) {
    DSEG_TRY(check_forward_args("dinoseg_train_forward", h, x, x_kind, B, Hf, Wf));
    if (h->fmt != FMT_BF16) {
        dinoseg_set_error("dinoseg_train_forward: precision fp16 is inference-only (fp16 gradients would need loss scaling); use bf16 or bf16x3");
        return -1;
    }
    h->tr_B = -1;       // no valid saved forward until this one has been enqueued completely
    DSEG_TRY(check_stream_device(h, s));
    DSEG_TRY(dinoseg_prepare_resolution_hw(h, Hf, Wf, reinterpret_cast<void*>(s)));
    const dinoseg_config& c = h->cfg;
    const int D = c.embed_dim, F = D * c.mlp_ratio, P = h->planes, H = c.num_heads, C = c.n_classes;
    const int NB = c.n_blocks;
    const TrainLayout L = make_train_layout(h, B, Hf, Wf);
    const ModelRec& m = h->model;

    // ---- workspace
    if (!h->bad_label_flag) {       // (its own allocation: a change of batch shape re-lays the workspace, the latched flag must survive it)
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->bad_label_flag), 256));
        DSEG_CHECK_HIP(hipMemsetAsync(h->bad_label_flag, 0, 256, s));
    }
    if (L.total > h->tws_bytes) {
        if (h->tws) {
            DSEG_CHECK_HIP(hipStreamSynchronize(s));
            DSEG_CHECK_HIP(hipFree(h->tws));
        }
        h->tws = nullptr;
        h->tws_bytes = 0;
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->tws), L.total));
        h->tws_bytes = L.total;
        h->tws_B = -1;
    }
    char* ws = h->tws;
    const TrainWs w = {ws, L};
    if (h->tws_B != B || h->tws_H != Hf || h->tws_W != Wf) {
        for (int l = 0; l < NB; ++l)   // Q/K/V pad rows must be zero (never written afterwards)
            DSEG_CHECK_HIP(hipMemsetAsync(ws + L.Q + l * L.blk_stride, 0, L.LSE - L.Q, s));
        DSEG_CHECK_HIP(hipMemsetAsync(ws + L.ACC, 0, 256, s));
        h->tws_B = B;
        h->tws_H = Hf;
        h->tws_W = Wf;
    }

    // =============================================================== forward (activations kept)
    const StepEnv env = {h, s, false};      // (no profile events: the classes count the inference forward's launches)
    float* X0 = NB > 0 ? w.f32(L.Xin) : w.f32(L.Xfin);
    DSEG_TRY(embed_tokens(env, {x, x_kind, B, Hf, Wf, w.b16(L.PATCH), L.patch_plane, P, FMT_BF16, X0, 0}));

    for (int l = 0; l < NB; ++l) {
        const BlockRec& blk = m.blocks[l];
        const auto [Xin, Xmid, LSE, A1, Q, Kb, V, CTX, A2, HPRE, HB] = w.block(l);
        float* Xout = l + 1 < NB ? w.block(l + 1).Xin : w.f32(L.Xfin);
        const QkvOut qkv = {Q, Kb, V, L.qkv_plane, L.ntok, L.npad, H, D, QK_SCALE};
        const bool fuse_ln = options().gemm_ln != 0 && L.qkv_plane < (1L << 31) && L.f_plane < (1L << 31);
        if (fuse_ln && blk.qkv.slab) {
            // LN1 + qkv in one launch; the normalised planes the weight gradient needs are a by-product (a_out)
            LnGemmParams g = {};
            g.X = Xin; g.ldx = D; g.gamma = blk.norm1_w; g.beta = blk.norm1_b; g.eps = c.ln_eps;
            g.W = blk.qkv.slab; g.bias = blk.qkv.b;
            g.M = L.M; g.N = 3 * D; g.epi = EPI_QKV;
            set_qkv(g, qkv);
            g.a_out = A1; g.a_plane = L.a_plane;
            DSEG_TRY(launch_gemm_ln(g, D, P, s));
        } else {
        DSEG_TRY(launch_layernorm(Xin, blk.norm1_w, blk.norm1_b, c.ln_eps, L.M, D, A1, L.a_plane, P,
                                  nullptr, 0, L.ntok, s));
        {
            GemmParams g = linear_gemm(blk.qkv);
            g.A = A1; g.a_plane = L.a_plane; g.lda = D;
            g.M = L.M; g.epi = EPI_QKV;
            set_qkv(g, qkv);
            DSEG_TRY(launch_gemm(g, s));
        }
        }
        {
            AttnParams a = {};
            a.q = Q; a.k = Kb; a.v = V; a.qkv_plane = L.qkv_plane; a.ctx = CTX; a.ctx_plane = L.a_plane;
            a.lse = LSE;
            a.B = B; a.heads = H; a.ntok = L.ntok; a.npad = L.npad; a.planes = P;
            DSEG_TRY(launch_attention(a, s));
        }
        {
            GemmParams g = resid_gemm(blk.proj, CTX, L.a_plane, L.M, Xmid);
            g.resid = Xin;
            DSEG_TRY(launch_gemm(g, s));
        }
        if (fuse_ln && blk.fc1.slab) {
            LnGemmParams g = {};
            g.X = Xmid; g.ldx = D; g.gamma = blk.norm2_w; g.beta = blk.norm2_b; g.eps = c.ln_eps;
            g.W = blk.fc1.slab; g.bias = blk.fc1.b;
            g.M = L.M; g.N = F; g.epi = EPI_GELU;
            set_hidden_out(g, HB, L.f_plane, F);
            g.a_out = A2; g.a_plane = L.a_plane;
            g.aux_out = HPRE; g.aux_plane = L.f_plane;
            DSEG_TRY(launch_gemm_ln(g, D, P, s));
        } else {
        DSEG_TRY(launch_layernorm(Xmid, blk.norm2_w, blk.norm2_b, c.ln_eps, L.M, D, A2, L.a_plane, P,
                                  nullptr, 0, L.ntok, s));
        {
            GemmParams g = linear_gemm(blk.fc1);
            g.A = A2; g.a_plane = L.a_plane; g.lda = D;
            g.M = L.M; g.epi = EPI_GELU;
            set_hidden_out(g, HB, L.f_plane, F);
            g.aux_out = HPRE; g.aux_plane = L.f_plane;
            DSEG_TRY(launch_gemm(g, s));
        }
        }
        {
            GemmParams g = resid_gemm(blk.fc2, HB, L.f_plane, L.M, Xout);
            g.resid = Xmid;
            DSEG_TRY(launch_gemm(g, s));
        }
    }
    const auto [Xfin, LOGP, FEAT, H1, H2] = w.head();
    DSEG_TRY(run_head(env, {Xfin, L.M, L.Mp, L.ntok, FEAT, H1, H2, L.feat_plane, L.h1_plane, L.h2_plane, FMT_BF16, LOGP, nullptr}));
    if (logp_out) DSEG_CHECK_HIP(hipMemcpyAsync(logp_out, LOGP, (size_t)L.Mp * C * 4, hipMemcpyDeviceToDevice, s));
    h->tr_B = B;
    h->tr_H = Hf;
    h->tr_W = Wf;
    return 0;
}

// Backward of the last train_forward_impl.  Exactly one of (labels, dlogp) is given:
//   labels : loss = F.nll_loss(logp, labels) (mean over the rows whose label is not -100) -> *loss_out, then backward of it
//   dlogp  : fp32 [B*n, C] upstream gradient d L / d logp (torch.autograd path)
// Gradients are written (not accumulated) into the buffers bound with dinoseg_bind_grad.
static int train_backward_impl(dinoseg_handle* h, const int64_t* labels, const float* dlogp, float* loss_out, hipStream_t s) {
    if (!h || (labels == nullptr) == (dlogp == nullptr) || (labels && !loss_out)) {
        dinoseg_set_error("dinoseg_backward: needs exactly one of labels (+ loss_out) and dlogp");
        return -1;
    }
    if (h->tr_B <= 0 || !h->tws) {
        dinoseg_set_error("dinoseg_backward: no saved forward (call dinoseg_train_forward first)");
        return -3;
    }
    if (!h->weights_ready) {
        dinoseg_set_error("dinoseg_backward: weights were re-bound after the forward; run the forward again");
        return -3;
    }
    const int B = h->tr_B, oh = h->tr_H / h->cfg.patch, ow = h->tr_W / h->cfg.patch;
    const dinoseg_config& c = h->cfg;
    const int D = c.embed_dim, F = D * c.mlp_ratio, P = h->planes, HP = head_planes(), H = c.num_heads, C = c.n_classes;
    const int NB = c.n_blocks;
    const bool mlp_head = c.head_kind == DINOSEG_HEAD_MLP;
    const TrainLayout L = make_train_layout(h, B, h->tr_H, h->tr_W);
    const TrainWs w = {h->tws, L};
    const ModelRec& m = h->model;
    GradRec& gr = h->grad;

    // ---- transposed packed weights for dX = dY . W  (weights change every optimiser step: repack)
    {
        std::vector<std::pair<const LinearRec*, LinearGrad*>> lins;      // every linear with an input gradient, in twbuf order
        for (int l = 0; l < NB; ++l) {
            const BlockRec& blk = m.blocks[l];
            BlockGrad& bg = gr.blocks[l];
            lins.insert(lins.end(), {{&blk.qkv, &bg.qkv}, {&blk.proj, &bg.proj}, {&blk.fc1, &bg.fc1}, {&blk.fc2, &bg.fc2}});
        }
        if (mlp_head) lins.insert(lins.end(), {{&m.head[0], &gr.head[0]}, {&m.head[1], &gr.head[1]}});
        lins.push_back({&m.clf, &gr.clf});
        auto bytes = [](const LinearRec& r, const LinearGrad& g) { return align_up((size_t)r.planes * g.t_plane * 2, 256); };
        size_t total = 0;
        for (auto& rg : lins) total += bytes(*rg.first, *rg.second);
        if (total > h->twbuf_bytes) {
            if (h->twbuf) {
                DSEG_CHECK_HIP(hipStreamSynchronize(s));
                DSEG_CHECK_HIP(hipFree(h->twbuf));
            }
            h->twbuf = nullptr;
            DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->twbuf), total));
            h->twbuf_bytes = total;
        }
        size_t off = 0;
        std::vector<dseg::PackJob> jobs;
        for (auto& rg : lins) {
            const LinearRec& r = *rg.first;
            LinearGrad& g = *rg.second;
            g.tw = reinterpret_cast<bf16_t*>(h->twbuf + off);
            off += bytes(r, g);
            // W [N][K] fp32 -> W^T planes [k_pad][n_pad]: "rows" of the source are N, transposed destination rows are K
            jobs.push_back({r.w, g.tw, g.t_plane, r.N, r.K, g.n_pad, g.k_pad, r.planes, 1});
        }
        DSEG_TRY(launch_multi_pack(jobs.data(), (int)jobs.size(), s));
    }

    bool backbone = false;
    {
        std::vector<float*> zp;
        std::vector<long> zn;
        for (auto& kv : h->grad_index) {
            const GradSlot& g = *kv.second;
            if (!g.ptr) continue;
            zp.push_back(g.ptr);
            zn.push_back(g.numel);
            backbone |= g.backbone;
        }
        if (!zp.empty()) DSEG_TRY(launch_multi_zero((int)zp.size(), zp.data(), zn.data(), s));      // one launch instead of ~50 memset nodes
    }
    // option deterministic: the launchers below write per-block partial sums here and add them in a fixed order (train.hip,
    // gemm_tn.hip) instead of fp32 atomics; cleared on every way out
    // The scratch pointer is process-wide state read by the launchers: a second backward entered while it is set (another host thread
    // stepping another handle) would write its partial sums into THIS handle's workspace -- refused instead.
    struct DetGuard {
        bool mine = false;
        ~DetGuard() { if (mine) det_scratch() = DetScratch{nullptr, 0, {nullptr, nullptr}, 0}; }
    } det_guard;
    if (options().deterministic) {
        if (det_scratch().ptr != nullptr) {
            dinoseg_set_error("dinoseg_backward: option deterministic allows one backward at a time per process (another one is being queued)");
            return -1;
        }
        float* det = w.f32(L.DET);
        det_scratch() = DetScratch{det, DET_FLOATS, {det + DET_FLOATS, det + DET_FLOATS + DET_TN_FLOATS}, DET_TN_FLOATS};
        det_guard.mine = true;
    }
    const hipStream_t main_stream = s;
    const auto [Xfin, LOGP, FEAT, H1, H2] = w.head();
    bf16_t *DZ = w.b16(L.DZ), *PATCH = w.b16(L.PATCH);

    // =============================================================== backward
    // stage events: a side stream can start reducing a gradient bucket while the rest of backward still runs
    h->stage_done = 0;
    auto stage_mark_on = [&](int stage, hipStream_t on) -> int {
        while ((int)h->stage_ev.size() <= stage) {
            hipEvent_t ev;
            DSEG_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            h->stage_ev.push_back(ev);
        }
        DSEG_CHECK_HIP(hipEventRecord(h->stage_ev[stage], on));
        h->stage_done = stage + 1;
        return 0;
    };
    auto stage_mark = [&](int stage) -> int { return stage_mark_on(stage, s); };
    // Side stream for the blocks' weight gradients (option train_streams = 2).  dW = dY^T . X reads what the input-gradient chain
    // has already produced and feeds nothing but the optimiser, so it runs beside that chain on the handle's internal stream:
    // the chain's tail rounds and memory-bound kernels (LayerNorm backward, the attention prep) leave CUs idle that the
    // weight-gradient tiles fill.  side_begin(): the side stream waits for everything queued on s so far; side_end() returns an
    // event the caller's stream waits on (side_wait) before it overwrites an operand the side kernels read, and before every
    // gradient-stage event.  Fork and join are events only: the call stays stream-ordered for the caller and capturable.
    // (deterministic mode: the side stream's only partial sums are gemm_tn's bias sums: they have their own part of the scratch area)
    const bool side = options().train_streams >= 2;
    hipStream_t ws_ = s;
    size_t bw_i = 0;
    auto bw_event = [&](hipEvent_t* out) -> int {
        if (bw_i == h->bw_ev.size()) {
            hipEvent_t ev;
            DSEG_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            h->bw_ev.push_back(ev);
        }
        *out = h->bw_ev[bw_i++];
        return 0;
    };
    if (side) {
        DSEG_TRY(ensure_aux_stream(h));
        ws_ = h->aux_stream;
    }
    auto side_begin = [&]() -> int {
        if (!side) return 0;
        hipEvent_t ev;
        DSEG_TRY(bw_event(&ev));
        DSEG_CHECK_HIP(hipEventRecord(ev, s));
        DSEG_CHECK_HIP(hipStreamWaitEvent(ws_, ev, 0));
        return 0;
    };
    auto side_end = [&](hipEvent_t* done) -> int {
        *done = nullptr;
        if (!side) return 0;
        DSEG_TRY(bw_event(done));
        DSEG_CHECK_HIP(hipEventRecord(*done, ws_));
        return 0;
    };
    auto side_wait = [&](hipEvent_t& done) -> int {
        if (done) DSEG_CHECK_HIP(hipStreamWaitEvent(s, done, 0));
        done = nullptr;
        return 0;
    };
    float* sink = w.f32(L.SINK);
    bf16_t *T1 = w.b16(L.T1), *T2 = w.b16(L.T2);

    // dX[M_, Kin] = dY[M_, Ncols] . W   with optional activation-derivative epilogue
    auto dgrad = [&](const bf16_t* dY, long dy_plane, int ld, int M_, int n_contract, const LinearGrad& wt, int k_out, int planes, int epi,
                     float* out_f32, bf16_t* out_bf16, long out_plane, const bf16_t* aux, long aux_plane) -> int {
        GemmParams g = {};
        g.A = dY; g.a_plane = dy_plane; g.lda = ld; g.W = wt.tw; g.w_plane = wt.t_plane;
        g.M = M_; g.N = k_out; g.K = n_contract; g.planes = planes; g.epi = epi;
        g.out_f32 = out_f32; g.ldo_f32 = k_out;
        g.out_bf16 = out_bf16; g.out_plane = out_plane; g.ldo = k_out; g.aux_in = aux; g.aux_plane = aux_plane;
        return launch_gemm_small(g, s);
    };
    // dW[n_rows, k_cols] += dY^T . X  from transposed planes T_dy [n_pad][m_pad], T_x [k_pad128][m_pad]
    auto wgrad = [&](const bf16_t* Tdy, const bf16_t* Tx, long tplane, int m_pad, int n_rows, int k_pad128, int k_cols, int planes,
                     float* dW) -> int {
        if (!dW) return 0;
        return wgrad_nt(Tdy, Tx, tplane, m_pad, n_rows, k_pad128, k_cols, planes, wgrad_nt_slices(n_rows, k_pad128, m_pad),
                        w.f32(L.SPLITK), dW, s);
    };
    auto pad128 = [](int v) { return (v + 127) / 128 * 128; };
    // weight gradient straight from the row-major dY and layer-input planes (gemm_tn.hip): no operand transposes
    // dbias (optional): the layer's bias gradient = column sums of Y, taken inside the weight-gradient kernel.  When the weight is
    // frozen that kernel still runs for the column sums alone if colsum_alone (the head layers); otherwise (the block linears) a
    // pack pass over Y produces them
    // k_pad (optional): the stored width of X when that is a multiple of 128 and k_cols is not (the classifier's zero-padded hidden
    // activations): the kernel multiplies all k_pad columns, the reduce writes the first k_cols
    auto wgrad_tn = [&](const bf16_t* Y, long y_plane, int ldy, const bf16_t* X, long x_plane, int ldx, int m_rows, int n_rows,
                        int k_cols, int planes, float* dW, float* dbias, hipStream_t s, int k_pad, bool colsum_alone) -> int {
        if (!dW && !dbias) return 0;
        if (!dW && !colsum_alone)
            return launch_transpose_planes(nullptr, Y, y_plane, ldy, m_rows, n_rows, nullptr, 0, pad128(n_rows), L.Mpad, nullptr, 0, 0,
                                           dbias, planes, 0, 0, s, s != main_stream);
        const int Kc = k_pad ? k_pad : k_cols;
        TnParams g = {};
        g.Y = Y; g.y_plane = y_plane; g.ldy = ldy; g.X = X; g.x_plane = x_plane; g.ldx = ldx;
        g.M = m_rows; g.N = n_rows; g.Kc = Kc; g.planes = planes;
        const int row_tiles = (n_rows + 127) / 128, tiles = row_tiles * (Kc / 128), nchunks = (m_rows + 31) / 32;
        int ks = splitk_budget() / tiles;
        if (ks > nchunks / 4) ks = nchunks / 4;
        if (ks >= 8 && !(dseg::options().route_ab & 4)) ks &= ~7;      // a multiple of 8: the kernel's XCD-aware form (gemm_tn.hip)
        if (ks < 1) ks = 1;
        const int per = (nchunks + ks - 1) / ks, used = (nchunks + per - 1) / per;
        g.part = w.f32(L.SPLITK); g.ld_part = Kc; g.split_stride = (long)row_tiles * 128 * Kc; g.ksplit = ks;
        g.colsum = dbias;
        g.det_region = s != main_stream;
        DSEG_TRY(launch_gemm_tn(g, s));
        if (!dW) return 0;
        return launch_splitk_reduce(g.part, used, g.split_stride, n_rows, Kc, dW, k_cols, k_cols, s);
    };

    // ---- loss and d logits (pl_torch_modules.py:264-265)
    const int ldz = dz_ld(C);
    DSEG_TRY(launch_nll_loss_grad(LOGP, labels, dlogp, L.Mp, C, w.f32(L.ACC), h->bad_label_flag, loss_out, DZ,
                                  L.dz_plane, ldz, s));
    const long tpl = L.t_plane;
    float* dX = w.f32(L.dX);
    float* dA = w.f32(L.dA);
    bf16_t* G = w.b16(L.G);
    if (mlp_head) {
        // layer_3: z = h2 W3^T + b3      (weight and bias gradients straight from the row-major planes: gemm_tn.hip; h2 / h1 are stored
        // 128 / 256 wide, zero beyond their 100 / 200 columns)
        const LinearGrad &g1 = gr.head[0], &g2 = gr.head[1], &g3 = gr.clf;
        DSEG_TRY(wgrad_tn(DZ, L.dz_plane, ldz, H2, L.h2_plane, HEAD_H2_PAD, L.Mp, C, HEAD_H2, HP, g3.dw.ptr, g3.db.ptr, s, HEAD_H2_PAD, true));
        bf16_t* dH2 = G;                         // [HP][Mp][128]
        const long dh2_plane = (long)L.Mp * HEAD_H2_PAD;
        DSEG_TRY(dgrad(DZ, L.dz_plane, ldz, L.Mp, ldz, g3, HEAD_H2_PAD, HP, EPI_DRELU, nullptr, dH2, dh2_plane, H2, L.h2_plane));
        // layer_2
        DSEG_TRY(wgrad_tn(dH2, dh2_plane, HEAD_H2_PAD, H1, L.h1_plane, HEAD_H1_PAD, L.Mp, HEAD_H2, HEAD_H1, HP, g2.dw.ptr, g2.db.ptr, s, HEAD_H1_PAD, true));
        bf16_t* dH1 = w.b16(L.dCTX);             // [HP][Mp][256] fits: Mp*256 <= M*D
        const long dh1_plane = (long)L.Mp * HEAD_H1_PAD;
        DSEG_TRY(dgrad(dH2, dh2_plane, HEAD_H2_PAD, L.Mp, HEAD_H2_PAD, g2, HEAD_H1_PAD, HP, EPI_DRELU, nullptr, dH1, dh1_plane, H1, L.h1_plane));
        // layer_1
        DSEG_TRY(wgrad_tn(dH1, dh1_plane, HEAD_H1_PAD, FEAT, L.feat_plane, D, L.Mp, HEAD_H1, D, HP, g1.dw.ptr, g1.db.ptr, s, D, true));
        if (backbone)
            DSEG_TRY(dgrad(dH1, dh1_plane, HEAD_H1_PAD, L.Mp, HEAD_H1_PAD, g1, D, HP, EPI_PLAIN, dA, nullptr, 0, nullptr, 0));
    } else {
        DSEG_TRY(wgrad_tn(DZ, L.dz_plane, ldz, FEAT, L.feat_plane, D, L.Mp, C, D, HP, gr.clf.dw.ptr, gr.clf.db.ptr, s, D, true));
        if (backbone)
            DSEG_TRY(dgrad(DZ, L.dz_plane, ldz, L.Mp, ldz, gr.clf, D, HP, EPI_PLAIN, dA, nullptr, 0, nullptr, 0));
    }
    DSEG_TRY(stage_mark(0));
    if (!backbone) return 0;      // frozen backbone (freeze_bb, pl_torch_modules.py:434-436): only the head trains

    // ---- final norm (CLS rows get no gradient from the head)
    auto gsink = [&](const GradSlot& g) { return g.ptr ? g.ptr : sink; };      // (LayerNorm backward always writes its gain / shift sums)
    // (every LayerNorm backward also leaves its dX rows as bf16 planes dXp and their column sums = the bias gradient of the
    //  layer the walk reaches next: mlp.fc2 of the last block here)
    bf16_t* dXp = w.b16(L.dXp);
    DSEG_TRY(launch_layernorm_bwd(dA, Xfin, m.norm_w, c.ln_eps, L.M, D, dX, 0, gsink(gr.norm_w), gsink(gr.norm_b), 1, L.ntok, s, dXp,
                                  L.a_plane, P, NB > 0 ? gr.blocks[NB - 1].fc2.db.ptr : nullptr));

    bf16_t* dCTX = w.b16(L.dCTX);
    hipEvent_t w_fc2 = nullptr, w_fc1 = nullptr, w_proj = nullptr, w_qkv = nullptr;
    for (int l = NB - 1; l >= 0; --l) {
        const BlockRec& blk = m.blocks[l];
        const BlockGrad& bg = gr.blocks[l];
        const auto [Xin, Xmid, LSE, A1, Q, Kb, V, CTX, A2, HPRE, HB] = w.block(l);
        // ---- mlp.fc2 : X_out = X_mid + H W2^T + b
        // (dXp = bf16 planes of dX and the fc2 bias gradient were left by the LayerNorm backward that produced dX; the weight
        //  gradient reads dXp and HB row-major)
        DSEG_TRY(side_begin());
        DSEG_TRY(wgrad_tn(dXp, L.a_plane, D, HB, L.f_plane, F, L.M, D, F, P, bg.fc2.dw.ptr, nullptr, ws_, 0, false));
        DSEG_TRY(side_end(&w_fc2));
        // dHpre = (dX . W2) * gelu'(Hpre)      (writes G: the previous block's qkv weight gradient reads it)
        DSEG_TRY(side_wait(w_qkv));
        DSEG_TRY(dgrad(dXp, L.a_plane, D, L.M, D, bg.fc2, F, P, EPI_DGELU, nullptr, G, (long)L.M * F, HPRE, L.f_plane));
        // ---- mlp.fc1 : Hpre = A2 W1^T + b
        DSEG_TRY(side_begin());
        DSEG_TRY(wgrad_tn(G, (long)L.M * F, F, A2, L.a_plane, D, L.M, F, D, P, bg.fc1.dw.ptr, bg.fc1.db.ptr, ws_, 0, false));
        DSEG_TRY(side_end(&w_fc1));
        DSEG_TRY(dgrad(G, (long)L.M * F, F, L.M, F, bg.fc1, D, P, EPI_PLAIN, dA, nullptr, 0, nullptr, 0));
        // ---- norm2 (input X_mid); the residual branch keeps dX      (rewrites dXp: the fc2 weight gradient reads it)
        DSEG_TRY(side_wait(w_fc2));
        DSEG_TRY(launch_layernorm_bwd(dA, Xmid, blk.norm2_w, c.ln_eps, L.M, D, dX, 1, gsink(bg.norm2_w), gsink(bg.norm2_b), 0, L.ntok, s,
                                      dXp, L.a_plane, P, bg.proj.db.ptr));
        // ---- attn.proj : X_mid = X_in + ctx Wp^T + b
        DSEG_TRY(side_begin());
        DSEG_TRY(wgrad_tn(dXp, L.a_plane, D, CTX, L.a_plane, D, L.M, D, D, P, bg.proj.dw.ptr, nullptr, ws_, 0, false));
        DSEG_TRY(side_end(&w_proj));
        DSEG_TRY(dgrad(dXp, L.a_plane, D, L.M, D, bg.proj, D, P, EPI_BF16, nullptr, dCTX, L.a_plane, nullptr, 0));
        // ---- attention      (writes G: the fc1 weight gradient reads it)
        DSEG_TRY(side_wait(w_fc1));
        {
            AttnBwdParams a = {};
            a.q = Q; a.k = Kb; a.v = V; a.qkv_plane = L.qkv_plane;
            a.dO = dCTX; a.O = CTX; a.dO_plane = L.a_plane; a.lse = LSE;
            a.neg_lse = w.f32(L.NLSE); a.neg_delta = w.f32(L.NDEL);
            a.dqkv = G; a.dqkv_plane = (long)L.M * 3 * D;
            a.B = B; a.heads = H; a.ntok = L.ntok; a.npad = L.npad; a.planes = P;
            DSEG_PROF(DINOSEG_PROF_ATTN_BWD, DSEG_TRY(launch_attention_bwd(a, s)));
        }
        // ---- attn.qkv : qkv = A1 Wqkv^T + b
        DSEG_TRY(side_begin());
        DSEG_TRY(wgrad_tn(G, (long)L.M * 3 * D, 3 * D, A1, L.a_plane, D, L.M, 3 * D, D, P, bg.qkv.dw.ptr,
                          bg.qkv.db.ptr, ws_, 0, false));
        DSEG_TRY(side_end(&w_qkv));
        DSEG_TRY(dgrad(G, (long)L.M * 3 * D, 3 * D, L.M, 3 * D, bg.qkv, D, P, EPI_PLAIN, dA, nullptr, 0, nullptr, 0));
        // ---- norm1 (input X_in)      (rewrites dXp: the proj weight gradient reads it)
        // (by-products for mlp.fc2 of block l-1; the embedding step after block 0 packs dX itself: it drops the CLS rows)
        DSEG_TRY(side_wait(w_proj));
        DSEG_TRY(launch_layernorm_bwd(dA, Xin, blk.norm1_w, c.ln_eps, L.M, D, dX, 1, gsink(bg.norm1_w), gsink(bg.norm1_b), 0, L.ntok, s,
                                      l > 0 ? dXp : nullptr, L.a_plane, P, l > 0 ? gr.blocks[l - 1].fc2.db.ptr : nullptr));
        // this block's gradients are complete once the side stream has finished its qkv weight gradient; the stage event is
        // recorded on the side stream (it has waited for everything the block queued on s up to the qkv weight gradient -- the
        // LayerNorm backward above is covered by the extra fork), so the caller's stream does not stall here
        if (side) {
            DSEG_TRY(side_begin());
            DSEG_TRY(stage_mark_on(1 + (NB - 1 - l), ws_));
            continue;
        }
        DSEG_TRY(stage_mark(1 + (NB - 1 - l)));
    }

    // join: the caller's stream continues (and the call returns) behind everything the side stream did; the embedding step
    // below reuses the split-K workspace
    DSEG_TRY(side_wait(w_qkv));
    // ---- embeddings: tokens = [cls ; conv(patches)] + pos   (vision_transformer.py:224-235)
    float* dpos = w.f32(L.DPOS);
    DSEG_TRY(launch_batch_sum_rows(dX, B, L.ntok, D, dpos, s));
    if (gr.cls_token.ptr)
        DSEG_CHECK_HIP(hipMemcpyAsync(gr.cls_token.ptr, dpos, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
    // (scratch: the T2 transpose buffer, idle until the patch-embed gradient below; make_train_layout sizes it for [pos_grid][W/patch][D] floats)
    if (gr.pos_embed.ptr) {
        if ((size_t)c.pos_grid * ow * D * sizeof(float) > L.t2_bytes) {
            dinoseg_set_error("dinoseg_backward: pos-embed scratch does not fit (pos_grid %d, grid %d x %d)", c.pos_grid, oh, ow);
            return -1;
        }
        DSEG_TRY(launch_pos_resample_bwd(dpos, c.pos_grid, D, oh, ow, gr.pos_embed.ptr, reinterpret_cast<float*>(T2), s));
    }
    DSEG_TRY(launch_transpose_planes(dX, nullptr, 0, D, L.Mp, D, T1, tpl, pad128(D), L.Mppad, nullptr, 0, 0,
                                     gr.patch.db.ptr, P, 1, L.ntok, s));
    if (gr.patch.dw.ptr) {
        const int kp = 3 * c.patch * c.patch;       // 192 columns in 256 transposed rows at patch 8; 768 in 768 at patch 16
        if ((long)pad128(kp) * L.Mppad > tpl) {
            dinoseg_set_error("dinoseg_backward: the transposed patch matrix (%d x %d) does not fit its plane (%ld)", pad128(kp), L.Mppad, tpl);
            return -1;
        }
        DSEG_TRY(launch_transpose_planes(nullptr, PATCH, L.patch_plane, kp, L.Mp, kp, T2, tpl, pad128(kp), L.Mppad, nullptr, 0, 0, nullptr, P, 0, 0, s));
        DSEG_TRY(wgrad(T1, T2, tpl, L.Mppad, D, pad128(kp), kp, P, gr.patch.dw.ptr));
    }
    return stage_mark(NB + 1);
}

extern "C" int dinoseg_train_forward_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W,
                                        float* logp_out, void* stream) {
    DeviceGuard guard(h);
    return train_forward_impl(h, x, x_kind, B, H, W, logp_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_train_forward(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, float* logp_out,
                                     void* stream) {
    return dinoseg_train_forward_hw(h, x, x_kind, B, r, r, logp_out, stream);
}

// The backward forks weight-gradient kernels onto the handle's side stream (option train_streams = 2) and joins them before it
// returns.  An error in between returns early: join here too, so that the caller's stream never runs ahead of side-stream kernels
// that still read / write the gradient buffers, the split-K workspace or the activations (as dinoseg_forward does for its halves).
static int backward_joined(dinoseg_handle* h, const int64_t* labels, const float* dlogp, float* loss_out, hipStream_t s) {
    const int rc = train_backward_impl(h, labels, dlogp, loss_out, s);
    if (rc != 0 && h && h->aux_stream && h->ev_join) {
        (void)hipEventRecord(h->ev_join, h->aux_stream);
        (void)hipStreamWaitEvent(s, h->ev_join, 0);
    }
    return rc;
}

extern "C" int dinoseg_backward(dinoseg_handle* h, const float* dlogp, void* stream) {
    DeviceGuard guard(h);
    return backward_joined(h, nullptr, dlogp, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_train_step_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W,
                                     const int64_t* labels, float* loss_out, float* logp_out, void* stream) {
    if (!labels || !loss_out) {
        dinoseg_set_error("dinoseg_train_step: bad argument");
        return -1;
    }
    DeviceGuard guard(h);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DSEG_TRY(train_forward_impl(h, x, x_kind, B, H, W, logp_out, s));
    return backward_joined(h, labels, nullptr, loss_out, s);
}

extern "C" int64_t dinoseg_op_upsample_nll_scratch_bytes(int32_t B, int32_t hp, int32_t wp, int32_t C, int32_t OH, int32_t OW) {
    return upsample_nll_scratch_bytes(B, hp, wp, C, OH, OW);
}

extern "C" int dinoseg_op_upsample_nll(const float* logp, int32_t B, int32_t hp, int32_t wp, int32_t C, int32_t OH, int32_t OW,
                                       const int64_t* labels, int32_t ignore_index, float* loss_out, float* dlogp_out, float* n_valid_out,
                                       int32_t* flags, void* scratch, void* stream) {
    return launch_upsample_nll(logp, B, hp, wp, C, OH, OW, labels, ignore_index, loss_out, dlogp_out, n_valid_out, flags, scratch,
                               reinterpret_cast<hipStream_t>(stream));
}

// The fine-tune step on pixel labels: the forward with saved activations, the cross-entropy of its log-probs upsampled to OH x OW
// (upsample_loss.hip: loss and d loss / d logp, no [B, C, OH, OW] tensor), then the backward from that d logp.  Everything the loss
// would refuse is refused here, before the forward enqueues anything.
extern "C" int dinoseg_train_step_dense_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t OH,
                                           int32_t OW, const int64_t* labels, int32_t ignore_index, float* loss_out, float* logp_out,
                                           void* stream) {
    if (!h || !x || !labels || !loss_out || B <= 0) {
        dinoseg_set_error("dinoseg_train_step_dense_hw: bad argument (null handle, frames, labels or loss_out, or B=%d)", B);
        return -1;
    }
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    const int hp = H / h->cfg.patch, wp = W / h->cfg.patch, C = h->cfg.n_classes;
    if (upsample_nll_check("dinoseg_train_step_dense_hw", B, hp, wp, C, OH, OW, ignore_index)) return -1;
    DeviceGuard guard(h);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DSEG_TRY(train_forward_impl(h, x, x_kind, B, H, W, logp_out, s));
    const size_t dl_bytes = align_up((size_t)B * hp * wp * C * sizeof(float), 256);
    const size_t need = dl_bytes + (size_t)upsample_nll_scratch_bytes(B, hp, wp, C, OH, OW);
    if (need > h->dws_bytes) {
        if (h->dws) {
            DSEG_CHECK_HIP(hipStreamSynchronize(s));
            DSEG_CHECK_HIP(hipFree(h->dws));
        }
        h->dws = nullptr;
        h->dws_bytes = 0;
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->dws), need));
        h->dws_bytes = need;
    }
    const TrainLayout L = make_train_layout(h, B, H, W);
    float* dlogp = reinterpret_cast<float*>(h->dws);
    DSEG_TRY(launch_upsample_nll(reinterpret_cast<const float*>(h->tws + L.LOGP), B, hp, wp, C, OH, OW, labels, ignore_index, loss_out, dlogp,
                                 nullptr, h->bad_label_flag, h->dws + dl_bytes, s));
    return backward_joined(h, nullptr, dlogp, nullptr, s);
}

extern "C" int dinoseg_train_step(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r,
                                  const int64_t* labels, float* loss_out, float* logp_out, void* stream) {
    return dinoseg_train_step_hw(h, x, x_kind, B, r, r, labels, loss_out, logp_out, stream);
}

extern "C" int dinoseg_grad_stages(const dinoseg_handle* h) { return h ? h->cfg.n_blocks + 2 : -1; }

extern "C" int dinoseg_stream_wait_grad_stage(dinoseg_handle* h, int32_t stage, void* stream) {
    if (!h || stage < 0 || stage >= h->cfg.n_blocks + 2) {
        dinoseg_set_error("dinoseg_stream_wait_grad_stage: stage out of range");
        return -1;
    }
    if (stage >= h->stage_done) {
        dinoseg_set_error("dinoseg_stream_wait_grad_stage: the last backward recorded %d stage(s); stage %d was not reached "
                          "(frozen backbone?)", h->stage_done, stage);
        return -3;
    }
    DeviceGuard guard(h);
    DSEG_CHECK_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), h->stage_ev[stage], 0));
    return 0;
}

extern "C" int dinoseg_train_status(dinoseg_handle* h, int32_t* bad_labels, void* stream) {
    if (!h || !bad_labels) {
        dinoseg_set_error("dinoseg_train_status: null argument");
        return -1;
    }
    *bad_labels = 0;
    if (!h->bad_label_flag) return 0;
    DeviceGuard guard(h);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int flag = 0;
    DSEG_CHECK_HIP(hipMemcpyAsync(&flag, h->bad_label_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    DSEG_CHECK_HIP(hipStreamSynchronize(s));
    if (flag) DSEG_CHECK_HIP(hipMemsetAsync(h->bad_label_flag, 0, sizeof(int), s));
    *bad_labels = flag;
    return 0;
}
