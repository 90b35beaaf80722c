// Fine-tune step of the DINOSeg hot path: forward with saved activations, backward, gradients
// written into caller-bound fp32 buffers.  Replaces DINOSeg.training_step + autograd.backward
// (pl_torch_modules.py:261-268) for one data-parallel rank; the cross-rank gradient mean is done by the caller
// (torch.distributed all_reduce over RCCL, dino_amd/parallel.py).  Host code only: the training forward, the pixel-label step and the
// C entries; the backward is backward.hip, the workspace layout and the gradient GEMM helpers both share are train_ws.h.
#include <vector>

#include "train_ws.h"

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

// the step's weight gradient (train_ws.h: run_wgrad_tn) with the caller's slice count
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
    WgradTn a = {};
    a.Y = {(const bf16_t*)Y, y_plane, ldy}; a.X = {(const bf16_t*)X, x_plane, ldx};
    a.M = M; a.N = N; a.Kc = Kc; a.planes = planes; a.ksplit = ksplit;
    a.part = part; a.dW = dW; a.ldw = ldw; a.k_cols = k_cols; a.colsum = colsum;
    return run_wgrad_tn(a, reinterpret_cast<hipStream_t>(stream));
}

// the step's input gradient (train_ws.h: run_dgrad): dX[M, N] = dY[M, K] . W^T[N, K]^T through the 128x128 kernel with a backward epilogue
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
    Dgrad a = {};
    a.dY = {(const bf16_t*)A, a_plane, lda}; a.Wt = (const bf16_t*)Wt; a.w_plane = w_plane;
    a.M = M; a.N = N; a.K = K; a.planes = planes; a.epi = epi;
    a.out_f32 = out_f32; a.ldo_f32 = ldo_f32;
    a.out_bf16 = (bf16_t*)out_bf16; a.out_plane = out_plane; a.ldo = ldo; a.aux = (const bf16_t*)aux_in; a.aux_plane = aux_plane;
    return run_dgrad(a, reinterpret_cast<hipStream_t>(stream));
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
// the training workspace of B frames of Hf x Wf and the handle's bad-label flag
static int ensure_train_workspace(dinoseg_handle* h, const TrainLayout& L, int B, int Hf, int Wf, hipStream_t s) {
    if (!h->bad_label_flag) {       // (its own allocation: a change of batch shape re-lays the workspace, the latched flag must survive it)
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->bad_label_flag), 256));
        DSEG_CHECK_HIP(hipMemsetAsync(h->bad_label_flag, 0, 256, s));
    }
    const bool grows = L.total > h->tws_bytes;
    DSEG_TRY(grow_device_buffer(h->tws, h->tws_bytes, L.total, s));
    if (grows) h->tws_B = -1;
    if (h->tws_B != B || h->tws_H != Hf || h->tws_W != Wf) {
        // pad rows (include/dinoseg.h, dinoseg_op_attention and dinoseg_op_attention_bwd): rows ntok..npad of q, k and v are read with the
        // 64-row tiles they share with real rows and must hold FINITE values -- any finite values, zero is not required (the forward and
        // the backward mask a pad key and give a pad query probability 0; 0 x finite = 0, 0 x Inf is not).  Fresh memory may hold
        // anything: zero Q/K/V once per layout (never written afterwards).
        for (int l = 0; l < h->cfg.n_blocks; ++l)
            DSEG_CHECK_HIP(hipMemsetAsync(h->tws + L.Q + l * L.blk_stride, 0, L.LSE - L.Q, s));
        DSEG_CHECK_HIP(hipMemsetAsync(h->tws + L.ACC, 0, 256, s));
        h->tws_B = B;
        h->tws_H = Hf;
        h->tws_W = Wf;
    }
    return 0;
}

// qkv / fc1 where the LayerNorm-fused kernel does not run: LayerNorm of X into the planes A, then the regular GEMM on them.  g: the
// linear's GemmParams with the epilogue and its outputs set
static int ln_then_gemm(const dinoseg_handle* h, const TrainLayout& L, const float* X, const float* gamma, const float* beta, bf16_t* A,
                        GemmParams g, hipStream_t s) {
    const int D = h->cfg.embed_dim;
    DSEG_TRY(launch_layernorm(X, gamma, beta, h->cfg.ln_eps, L.M, D, A, L.a_plane, h->planes, nullptr, 0, L.ntok, s));
    g.A = A; g.a_plane = L.a_plane; g.lda = D;
    g.M = L.M;
    return launch_gemm(g, s);
}

// one block of the training forward: every activation the backward reads stays in w (Xout: the next block's Xin, or Xfin)
static int train_block_forward(const dinoseg_handle* h, const TrainLayout& L, const BlockRec& blk, const BlockWs& w, float* Xout, int B,
                               hipStream_t s) {
    const dinoseg_config& c = h->cfg;
    const int D = c.embed_dim, F = D * c.mlp_ratio, P = h->planes, H = c.num_heads;
    const QkvOut qkv = {w.Q, w.K, w.V, L.qkv_plane, L.ntok, L.npad, H, D, QK_SCALE};
    const bool fuse_ln = options().gemm_ln != 0 && L.qkv_plane < (1L << 31) && L.f_plane < (1L << 31);
    if (fuse_ln && blk.qkv.slab) {
        // LN1 + qkv in one launch; the normalised planes the weight gradient needs are a by-product (a_out)
        LnGemmParams g = {};
        g.X = w.Xin; g.ldx = D; g.gamma = blk.norm1_w; g.beta = blk.norm1_b; g.eps = c.ln_eps;
        g.W = blk.qkv.slab; g.bias = blk.qkv.b;
        g.M = L.M; g.N = 3 * D; g.epi = EPI_QKV;
        set_qkv(g, qkv);
        g.a_out = w.A1; g.a_plane = L.a_plane;
        DSEG_TRY(launch_gemm_ln(g, D, P, s));
    } else {
        GemmParams g = linear_gemm(blk.qkv);
        g.epi = EPI_QKV;
        set_qkv(g, qkv);
        DSEG_TRY(ln_then_gemm(h, L, w.Xin, blk.norm1_w, blk.norm1_b, w.A1, g, s));
    }
    {
        AttnParams a = {};
        a.q = w.Q; a.k = w.K; a.v = w.V; a.qkv_plane = L.qkv_plane; a.ctx = w.CTX; a.ctx_plane = L.a_plane;
        a.lse = w.LSE;
        a.B = B; a.heads = H; a.ntok = L.ntok; a.npad = L.npad; a.planes = P;
        DSEG_TRY(launch_attention(a, s));
    }
    {
        GemmParams g = resid_gemm(blk.proj, w.CTX, L.a_plane, L.M, w.Xmid);
        g.resid = w.Xin;
        DSEG_TRY(launch_gemm(g, s));
    }
    if (fuse_ln && blk.fc1.slab) {
        LnGemmParams g = {};
        g.X = w.Xmid; g.ldx = D; g.gamma = blk.norm2_w; g.beta = blk.norm2_b; g.eps = c.ln_eps;
        g.W = blk.fc1.slab; g.bias = blk.fc1.b;
        g.M = L.M; g.N = F; g.epi = EPI_GELU;
        set_hidden_out(g, w.HB, L.f_plane, F);
        g.a_out = w.A2; g.a_plane = L.a_plane;
        g.aux_out = w.HPRE; g.aux_plane = L.f_plane;
        DSEG_TRY(launch_gemm_ln(g, D, P, s));
    } else {
        GemmParams g = linear_gemm(blk.fc1);
        g.epi = EPI_GELU;
        set_hidden_out(g, w.HB, L.f_plane, F);
        g.aux_out = w.HPRE; g.aux_plane = L.f_plane;
        DSEG_TRY(ln_then_gemm(h, L, w.Xmid, blk.norm2_w, blk.norm2_b, w.A2, g, s));
    }
    GemmParams g = resid_gemm(blk.fc2, w.HB, L.f_plane, L.M, Xout);
    g.resid = w.Xmid;
    return launch_gemm(g, s);
}

// Forward with saved activations (DINOSeg.forward under autograd, pl_torch_modules.py:239-256).  The saved state stays valid
// until the next call; the backward (backward.hip) consumes it.
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
    const int NB = h->cfg.n_blocks;
    const TrainLayout L = make_train_layout(h, B, Hf, Wf);
    DSEG_TRY(ensure_train_workspace(h, L, B, Hf, Wf, s));
    const TrainWs w = {h->tws, L};
    const auto [Xfin, LOGP, FEAT, H1, H2] = w.head();

    const StepEnv env = {h, s, false};      // (no profile events: the classes count the inference forward's launches)
    DSEG_TRY(embed_tokens(env, {x, x_kind, B, Hf, Wf, w.b16(L.PATCH), L.patch_plane, h->planes, FMT_BF16, NB > 0 ? w.f32(L.Xin) : Xfin, 0}));
    for (int l = 0; l < NB; ++l)
        DSEG_TRY(train_block_forward(h, L, h->model.blocks[l], w.block(l), l + 1 < NB ? w.block(l + 1).Xin : Xfin, B, s));
    DSEG_TRY(run_head(env, {Xfin, L.M, L.Mp, L.ntok, FEAT, H1, H2, L.feat_plane, L.h1_plane, L.h2_plane, FMT_BF16, LOGP, nullptr}));
    if (logp_out) DSEG_CHECK_HIP(hipMemcpyAsync(logp_out, LOGP, (size_t)L.Mp * h->cfg.n_classes * 4, hipMemcpyDeviceToDevice, s));
    h->tr_B = B;
    h->tr_H = Hf;
    h->tr_W = Wf;
    return 0;
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
    DSEG_TRY(grow_device_buffer(h->dws, h->dws_bytes, need, s));
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
