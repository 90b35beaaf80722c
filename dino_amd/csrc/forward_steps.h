// Internal: what the inference forward (forward.hip) and the training forward (train_api.hip) have in common -- the argument check,
// the parameter fills both write, the patch embedding and the head.  Each takes its buffers, plane strides, planes and format from
// the caller: the two forwards lay their workspaces out differently.
#pragma once
#include "handle.h"

// The refusals of every forward, before anything is enqueued; who = the entry's name in the messages.  -3: the weights are not packed.
static inline int check_forward_args(const char* who, const dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W) {
    if (!h || !x || B <= 0) {
        dinoseg_set_error("%s: bad argument", who);
        return -1;
    }
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    if (x_kind != DINOSEG_INPUT_U8_HWC && x_kind != DINOSEG_INPUT_F32_CHW) {
        dinoseg_set_error("%s: bad x_kind %d", who, x_kind);
        return -1;
    }
    if (!h->weights_ready) {
        dinoseg_set_error("%s: weights not packed (call dinoseg_refresh_weights after binding)", who);
        return -3;
    }
    return 0;
}

constexpr float QK_SCALE = 0.125f * 1.44269504088896340736f;   // head_dim^-0.5 (vision_transformer.py:73) * log2(e)

// ------------------------------------------------------------------------------------------------ parameter fills
// where a qkv epilogue scatters to: Q (pre-scaled), K, V, each [planes][B, heads, npad, 64]
struct QkvOut {
    bf16_t *q, *k, *v;
    long qkv_plane;
    int ntok, npad, heads, dmodel;
    float qscale;
};
template <class P>
static inline void set_qkv_rows(P& g, const QkvOut& o) {
    g.q = o.q; g.k = o.k; g.v = o.v;
    g.ntok = o.ntok; g.npad = o.npad; g.heads = o.heads; g.qscale = o.qscale;
}
template <class P>      // GemmParams / LnGemmParams
static inline void set_qkv(P& g, const QkvOut& o) {
    set_qkv_rows(g, o);
    g.qkv_plane = o.qkv_plane; g.dmodel = o.dmodel;
}
static inline void set_qkv(MlpFused3Params& g, const QkvOut& o) {     // the tail of mlp_fused3.hip: D = 384 is the kernel's own
    set_qkv_rows(g, o);
    g.qkv_plane = o.qkv_plane;
}
static inline void set_qkv(MlpFusedParams& g, const QkvOut& o) { set_qkv_rows(g, o); }     // ... of mlp_fused2.hip: one plane

// fc1: the GELU rows [planes][M][F]
template <class P>      // GemmParams / LnGemmParams
static inline void set_hidden_out(P& g, bf16_t* hb, long hb_plane, int F) {
    g.out_bf16 = hb; g.out_plane = hb_plane; g.ldo = F;
}

// attn.proj / mlp.fc2 with the residual add: X[M, D] (+)= A . W^T + b.  The caller adds dispatch_rows or resid
static inline GemmParams resid_gemm(const LinearRec& l, const bf16_t* A, long a_plane, int M, float* X) {
    GemmParams g = linear_gemm(l);
    g.A = A; g.a_plane = a_plane; g.lda = l.K;
    g.M = M; g.epi = EPI_RESID;
    g.out_f32 = X; g.ldo_f32 = l.N;
    return g;
}

// ------------------------------------------------------------------------------------------------ prepare_tokens
struct EmbedArgs {
    const void* x;
    int x_kind, B, Hf, Wf;
    bf16_t* gather; long gather_plane;     // the patch-gather matrix: planes x [B n, 3 p^2]
    int planes, fmt;
    float* X;                               // token rows out [B (n + 1), D] fp32
    int dispatch_rows;                      // GemmParams::dispatch_rows of the embedding GEMM (0: its own rows)
};
// gather + GEMM (+ bias + position) + cls rows (vision_transformer.py:224-235)
static inline int embed_tokens(const StepEnv& e, const EmbedArgs& a) {
    const dinoseg_handle* h = e.h;
    const dinoseg_config& c = h->cfg;
    const int n = (a.Hf / c.patch) * (a.Wf / c.patch);
    float mean255[3], inv255[3];
    norm_consts(mean255, inv255);
    DSEG_PROF_ENV(e, DINOSEG_PROF_PATCH, DSEG_TRY(launch_patch_gather(a.x, a.x_kind, a.B, a.Hf, a.Wf, mean255, inv255, a.gather, a.gather_plane,
                                                                  a.planes, e.s, a.fmt, c.patch)));
    GemmParams g = linear_gemm(h->model.patch);
    g.A = a.gather; g.a_plane = a.gather_plane; g.lda = 3 * c.patch * c.patch;       // the conv's fan-in: 192 at patch 8, 768 at patch 16
    g.M = a.B * n; g.epi = EPI_PATCH; g.dispatch_rows = a.dispatch_rows;
    g.out_f32 = a.X; g.ldo_f32 = c.embed_dim;
    g.pos = h->pos_cache; g.n_patches = n;
    DSEG_PROF_ENV(e, DINOSEG_PROF_PATCH, DSEG_TRY(launch_gemm(g, e.s)));
    DSEG_PROF_ENV(e, DINOSEG_PROF_PATCH, DSEG_TRY(launch_cls_rows(a.X, h->model.cls_token, h->pos_cache, a.B, n + 1, c.embed_dim, e.s)));
    return 0;
}

// ------------------------------------------------------------------------------------------------ final norm + head
struct HeadArgs {
    const float* X;                         // residual stream [M, D]
    int M, Mp, ntok;                        // token rows, patch rows, tokens per frame
    bf16_t *FEAT, *H1, *H2;                 // final-norm patch rows and the MLP head's hidden rows, hi + lo planes
    long feat_plane, h1_plane, h2_plane;
    int fmt;                                // format of those planes (split_fmt)
    float* logp; int32_t* argmax;           // fp32 [Mp, n_classes]; int32 [Mp] (nullable)
};
// final norm, drop CLS (vision_transformer.py:243; pl_torch_modules.py:243,253), then the segmentation head
// (pl_torch_modules.py:108-138), always in split precision
static inline int run_head(const StepEnv& e, const HeadArgs& a) {
    const dinoseg_config& c = e.h->cfg;
    const ModelRec& m = e.h->model;
    const int D = c.embed_dim;
    DSEG_PROF_ENV(e, DINOSEG_PROF_LN, DSEG_TRY(launch_layernorm(a.X, m.norm_w, m.norm_b, c.ln_eps, a.M, D, a.FEAT, a.feat_plane, head_planes(),
                                                            nullptr, 1, a.ntok, e.s, a.fmt)));
    const bf16_t* in = a.FEAT;
    long in_plane = a.feat_plane;
    int ld = D, K = D;
    if (c.head_kind == DINOSEG_HEAD_MLP) {
        GemmParams g = linear_gemm(m.head[0]);
        g.A = a.FEAT; g.a_plane = a.feat_plane; g.lda = D;
        g.M = a.Mp; g.epi = EPI_RELU;
        g.out_bf16 = a.H1; g.out_plane = a.h1_plane; g.ldo = HEAD_H1_PAD;
        DSEG_PROF_ENV(e, DINOSEG_PROF_HEAD, DSEG_TRY(launch_gemm(g, e.s)));
        g = linear_gemm(m.head[1]);
        g.A = a.H1; g.a_plane = a.h1_plane; g.lda = HEAD_H1_PAD;
        g.M = a.Mp; g.epi = EPI_RELU;
        g.out_bf16 = a.H2; g.out_plane = a.h2_plane; g.ldo = HEAD_H2_PAD;
        DSEG_PROF_ENV(e, DINOSEG_PROF_HEAD, DSEG_TRY(launch_gemm(g, e.s)));
        in = a.H2; in_plane = a.h2_plane; ld = HEAD_H2_PAD; K = HEAD_H2;
    }
    DSEG_PROF_ENV(e, DINOSEG_PROF_HEAD, DSEG_TRY(launch_head_final(in, in_plane, ld, a.Mp, K, m.clf.w, m.clf.b, c.n_classes, a.logp, a.argmax, e.s,
                                                               a.fmt, m.clf.pk.w, m.clf.pk.plane)));
    return 0;
}
