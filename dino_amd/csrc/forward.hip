// The inference forward of the DINOSeg hot path on one MI355X (see include/dinoseg.h): dinoseg_forward*, dinoseg_last_selfattention*,
// dinoseg_cls_attention_hw, dinoseg_forward_mask* and dinoseg_features*.  Host code only: a request (what the call wants back), a
// per-call context (buffers and sizes), the route of each block as a value (plan_block: the one reader of the options in the block
// loop), and the stages that enqueue what the route says.  The handle, the weights, the workspaces and the options live in api.hip.
#include "forward_steps.h"

using namespace dseg;

namespace {

// ------------------------------------------------------------------------------------------------ request
// What a forward call wants back, and with that where the block loop stops.  Filled by the extern "C" entries; every pointer nullable.
struct ForwardRequest {
    float* logp_out = nullptr;          // the head: log-probs [B n, C] (null: they stay in the workspace) ...
    int32_t* argmax_out = nullptr;      // ... and their argmax [B n]
    int32_t tap_block = -1;             // debug tap: the token rows after prepare_tokens (0) or after block tap_block
    float* tap_out = nullptr;
    float* attn_out = nullptr;          // get_last_selfattention: the probabilities of the last block, then stop
    float* cls_attn_out = nullptr;      // dinoseg_cls_attention_hw: the CLS row of those probabilities over the patches, enlarged to
    uint8_t* cls_keep_out = nullptr;    // OH x OW (below), and / or its cumulative-mass threshold at cls_threshold, then stop
    float cls_threshold = 0.f;
    bool wants_cls_attention() const { return cls_attn_out || cls_keep_out; }
    const float* cls_mask = nullptr;    // forward_mask / get_last_selfattention(x, cls_mask): the last block on the CLS token through
    int n_masks = 0;                    // each of n_masks masks; the masked probabilities (mask_attn_out) and / or one embedding
    float* mask_attn_out = nullptr;     // per mask (emb_out), then stop
    float* emb_out = nullptr;
    float* feat_out = nullptr;          // dinoseg_features: final-norm tokens [B, N, D] after feat_blocks blocks (0 = all), then stop
    int feat_blocks = 0;
    int OH = 0, OW = 0;                 // dinoseg_forward_dense_hw: behind the head, the log-probs upsampled to OH x OW on the same
    int32_t* labels = nullptr;          // stream: int32 [B, OH, OW] ...
    float* dense = nullptr;             // ... and / or fp32 [B, n_classes, OH, OW]
    bool wants_dense() const { return labels || dense; }
};
// the request of the second half-batch of a split forward: the outputs of the frames from B0 on (n patches a frame, C classes)
ForwardRequest second_half(const ForwardRequest& rq, int B0, long n, int C) {
    ForwardRequest r = rq;
    const size_t px = (size_t)B0 * rq.OH * rq.OW;
    if (r.logp_out) r.logp_out += (size_t)B0 * n * C;
    if (r.argmax_out) r.argmax_out += (size_t)B0 * n;
    if (r.labels) r.labels += px;
    if (r.dense) r.dense += px * C;
    return r;
}
// which part of a split forward a call is: slot 0 = the caller's stream, 1 = the second half-batch (its own workspace, the handle's
// internal stream); disp_B = the batch of the WHOLE call (0: this call is the whole)
struct SplitPart {
    int slot = 0, disp_B = 0;
};

// ------------------------------------------------------------------------------------------------ context
// One forward call: built once by begin_forward, read by every stage
struct ForwardCtx {
    StepEnv env;                        // the handle, the stream, profiled
    const ForwardRequest* rq;
    const dinoseg_config* cfg;
    const ModelRec* model;
    int B, Hf, Wf;
    WsLayout L;
    char* ws;
    float* X;                           // the residual stream [M, D] fp32
    bf16_t *A, *Q, *K, *V, *CTX, *HB, *FEAT, *H1, *H2;
    // every size-dependent kernel choice is made for the rows of the WHOLE call: the half-batches of a split forward (disp_B = the
    // call's batch) then take the routes -- and the summation order -- the unsplit batch takes, so the split changes no bit
    int disp_B, disp_M, disp_Mp;
    int D, F, P, FM, SF;                // embed_dim, hidden width; operand planes and format of the blocks; format of the head's planes
    float qscale;
    int v_bf16;                         // the qkv epilogue writes V as bf16 hi + lo planes (below)
    QkvOut qkv() const { return {Q, K, V, L.qkv_plane, L.ntok, L.npad, cfg->num_heads, D, qscale}; }
};

int begin_forward(ForwardCtx& c, dinoseg_handle* h, int32_t B, int32_t Hf, int32_t Wf, const ForwardRequest& rq, hipStream_t s,
                  const SplitPart& part) {
    c.env = {h, s, true};
    c.rq = &rq;
    c.cfg = &h->cfg;
    c.model = &h->model;
    c.B = B; c.Hf = Hf; c.Wf = Wf;
    c.L = make_layout(h, B, Hf, Wf);
    DSEG_TRY(ensure_workspace(h, part.slot, c.L, B, Hf, Wf, s));
    const WsLayout& L = c.L;
    c.ws = part.slot ? h->ws2 : h->ws;
    c.X = reinterpret_cast<float*>(c.ws + L.X);
    auto b16 = [&](size_t off) { return reinterpret_cast<bf16_t*>(c.ws + off); };
    c.A = b16(L.A); c.Q = b16(L.Q); c.K = b16(L.K); c.V = b16(L.V); c.CTX = b16(L.CTX); c.HB = b16(L.HB);
    c.FEAT = b16(L.FEAT); c.H1 = b16(L.H1); c.H2 = b16(L.H2);
    c.disp_B = part.disp_B > 0 ? part.disp_B : B;
    c.disp_M = c.disp_B * L.ntok;
    c.disp_Mp = c.disp_B * L.n;
    c.D = h->cfg.embed_dim; c.F = c.D * h->cfg.mlp_ratio; c.P = h->planes; c.FM = h->fmt; c.SF = split_fmt(h);
    c.qscale = QK_SCALE;
    // fp16 hi + lo planes: from two rounds of 256-query workgroups on, the attention is the zero-reference assembly kernel, whose
    // probabilities and V are bf16 hi + lo planes -- the qkv epilogue writes V that way (decided for the batch of the WHOLE call; never
    // on the visualisation paths, whose small kernels read V in the mode's own format)
    c.v_bf16 = (c.P == 2 && c.FM == FMT_FP16 && !rq.attn_out && !rq.cls_mask && attention_x3_za(c.disp_B, h->cfg.num_heads, L.ntok)) ? 1 : 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------ parameter fills
GemmParams qkv_gemm(const ForwardCtx& c, const BlockRec& blk) {       // LayerNorm1's planes A -> Q / K / V
    GemmParams g = linear_gemm(blk.qkv);
    g.A = c.A; g.a_plane = c.L.a_plane; g.lda = c.D;
    g.M = c.L.M; g.epi = EPI_QKV; g.dispatch_rows = c.disp_M;
    g.v_bf16 = c.v_bf16;
    set_qkv(g, c.qkv());
    return g;
}
GemmParams fc1_gemm(const ForwardCtx& c, const BlockRec& blk) {       // LayerNorm2's planes A -> the GELU rows HB
    GemmParams g = linear_gemm(blk.fc1);
    g.A = c.A; g.a_plane = c.L.a_plane; g.lda = c.D;
    g.M = c.L.M; g.epi = EPI_GELU; g.dispatch_rows = c.disp_M;
    set_hidden_out(g, c.HB, c.L.hb_plane, c.F);
    return g;
}
GemmParams proj_gemm(const ForwardCtx& c, const BlockRec& blk) {      // x += proj(ctx) + b
    GemmParams g = resid_gemm(blk.proj, c.CTX, c.L.ctx_plane, c.L.M, c.X);
    g.dispatch_rows = c.disp_M;
    return g;
}
GemmParams fc2_gemm(const ForwardCtx& c, const BlockRec& blk) {       // x += fc2(hb) + b
    GemmParams g = resid_gemm(blk.fc2, c.HB, c.L.hb_plane, c.L.M, c.X);
    g.dispatch_rows = c.disp_M;
    return g;
}
// the same linear through the row-stationary streaming kernels (gemm_rs.hip): its fragment-order copy; a copy that carries the
// LayerNorm in front of qkv / fc1 (gemm_rs_ln at the refresh) runs with the LayerNorm inside -- no LayerNorm launch, no 16-bit A
// round trip -- and only so
GemmParams to_rs(const ForwardCtx& c, GemmParams g, const LinearRec& lin) {
    g.W = lin.rs;
    if (lin.rs_bias) {
        g.ln_x = c.X; g.ln_eps = c.cfg->ln_eps; g.bias = lin.rs_bias;
    }
    return g;
}
// the LayerNorm-fused GEMM (gemm_ln.hip) of qkv / fc1: the fields both share; X rows are normalised in the GEMM's prologue, no
// bf16 A round trip
LnGemmParams ln_gemm(const ForwardCtx& c, const LinearRec& lin, const float* gamma, const float* beta, int epi) {
    LnGemmParams g = {};
    g.X = c.X; g.ldx = c.D; g.gamma = gamma; g.beta = beta; g.eps = c.cfg->ln_eps;
    g.W = lin.slab; g.bias = lin.b;
    g.M = c.L.M; g.N = lin.N; g.epi = epi; g.fmt = c.FM;
    return g;
}
int layernorm_to_A(const ForwardCtx& c, const float* gamma, const float* beta) {
    return launch_layernorm(c.X, gamma, beta, c.cfg->ln_eps, c.L.M, c.D, c.A, c.L.a_plane, c.P, nullptr, 0, c.L.ntok, c.env.s, c.FM);
}

// ------------------------------------------------------------------------------------------------ the route of a block
// LayerNorm + linear (LayerNorm1 + qkv, LayerNorm2 + fc1)
enum LnLinear {
    LNLIN_TAIL,         // qkv only: Q / K / V were written by the fused launch of the block before
    LNLIN_GEMM_LN,      // one launch of gemm_ln.hip
    LNLIN_RS_LN,        // one launch of gemm_rs.hip, the LayerNorm inside
    LNLIN_LN_RS,        // a LayerNorm launch, then gemm_rs.hip
    LNLIN_LN_GEMM,      // a LayerNorm launch, then the regular GEMM
};
enum BlockTail { TAIL_FUSED3, TAIL_FUSED4, TAIL_FUSED2, TAIL_SEPARATE };
struct BlockRoute {
    LnLinear qkv = LNLIN_LN_GEMM;
    // the second half: proj + MLP as one launch of mlp_fused3.hip / mlp_fused4.hip / mlp_fused2.hip, or separate GEMMs
    BlockTail tail = TAIL_SEPARATE;
    bool fuse_proj = false;             // ... with the attention output projection inside (else it runs in front of the launch)
    bool writes_next_qkv = false;       // ... and LayerNorm1 + qkv of the NEXT block at its end: that block's qkv is LNLIN_TAIL
    LnLinear fc1 = LNLIN_LN_GEMM;       // TAIL_SEPARATE: how LayerNorm2 + fc1 run
    bool rs_proj = false, rs_fc2 = false;       // proj (when not fused) / fc2 (TAIL_SEPARATE) through gemm_rs.hip
};

// How block i of this call runs, given the route of the block before it.  The only reader of the options and of the handle's option
// snapshots in the block loop.
BlockRoute plan_block(const ForwardCtx& c, const BlockRec& blk, int i, const BlockRoute& prev) {
    const Options& o = options();
    const dinoseg_handle* h = c.env.h;
    const WsLayout& L = c.L;
    const int P = c.P, disp_M = c.disp_M;
    BlockRoute r;
    // a block linear through the row-stationary streaming kernels: its copy exists (the linear's gemm_rs bit was set at the last
    // refresh), the bit is still set, the batch fills the chip and the kernel takes the parameters.  The LayerNorm-carrying copy
    // never under a cls_mask.  The one predicate for both the LayerNorm launch and the GEMM
    const int rs_bits = disp_M < o.gemm_rs_min_rows ? 0 : (o.gemm_rs & h->gemm_rs_snap);
    auto rs_route = [&](const GemmParams& g, const LinearRec& lin) -> bool {
        if (!lin.rs || !(rs_bits & lin.rs_bit)) return false;
        if (lin.rs_bias && c.rq->cls_mask) return false;
        return gemm_rs_supported(to_rs(c, g, lin));
    };
    auto ln_linear = [&](bool rs, const LinearRec& lin) { return !rs ? LNLIN_LN_GEMM : lin.rs_bias ? LNLIN_RS_LN : LNLIN_LN_RS; };
    // gemm_ln: 0 never fused, 2 always, 1 (default) by measurement (round 4, tools/r4_smallbatch.sh, 1..6 frames @480):
    //  * single plane (bf16 / fp16): fused from 80 row panels of 128 on -- below that its persistent 128 x 384 panels leave most
    //    CUs idle (one frame = 29 panels: qkv 31 against 21 us with LayerNorm + the 128x128 kernel, fc1 40 against 23; the
    //    whole single-frame forward 1.72 -> 1.33 ms at 12 blocks; crossover between 2 and 3 frames);
    //  * hi+lo planes: its 64-row panels run one workgroup per CU, so it wins only while they fill about one round of the chip
    //    (9 600 .. 16 384 rows = 3-4 frames: fc1 1.15 against 1.24 ms; 1 frame 1.01 against 0.48, 6 frames 2.13 against 1.33);
    //    from 512 tiles of 128 x 384 on, LayerNorm + the hi+lo configuration of the persistent GEMM (B = 32: fc1 30 + 534 us
    //    against 670 fused).
    const bool big_x3 = P == 2 && o.gemm_big && (long)((disp_M + 127) / 128) * 3 >= 512;
    const bool ln_small = P == 1 ? (disp_M + 127) / 128 < 80 : (disp_M < 9600 || disp_M > 16384);
    const bool fuse_ln = o.gemm_ln == 2 || (o.gemm_ln == 1 && !big_x3 && !ln_small);
    // (the fused kernel keeps 32-bit output row offsets)
    if (prev.writes_next_qkv) r.qkv = LNLIN_TAIL;
    else if (fuse_ln && blk.qkv.slab && L.qkv_plane < (1L << 31)) r.qkv = LNLIN_GEMM_LN;
    else r.qkv = ln_linear(rs_route(qkv_gemm(c, blk), blk.qkv), blk.qkv);

    // the fused MLP kernels run for this many token rows (options mlp_fused / mlp_fused_min_rows, mlp_fused3_min_rows)
    const bool fuse_mlp3 = P == 2 && blk.mlp3 &&      // hi + lo planes: mlp_fused3.hip
                           (o.mlp_fused == 2 || (o.mlp_fused == 1 && disp_M >= o.mlp_fused3_min_rows));
    const bool fuse_mlp = fuse_mlp3 || (blk.mlp && (o.mlp_fused == 2 || (o.mlp_fused == 1 && disp_M >= o.mlp_fused_min_rows)));
    // (the fused MLP kernels take the attention output projection along: x += proj(ctx) + b, then the MLP, one launch)
    r.fuse_proj = fuse_mlp && o.proj_fused && (fuse_mlp3 || (P == 1 && blk.projf));
    const bool has_next = i + 1 < c.cfg->n_blocks;
    if (fuse_mlp3) {
        r.tail = TAIL_FUSED3;
        r.writes_next_qkv = r.fuse_proj && o.qkv_fused3 && has_next && L.qkv_plane < (1L << 31);
    } else if (fuse_mlp && r.fuse_proj && o.mlp_fused4 && h->mlp_fused4_snap && !o.qkv_fused && blk.mlp4) {
        r.tail = TAIL_FUSED4;
        r.writes_next_qkv = o.qkv_fused4 && has_next;
    } else if (fuse_mlp) {
        r.tail = TAIL_FUSED2;
        r.writes_next_qkv = r.fuse_proj && o.qkv_fused && has_next && c.model->blocks[i + 1].qkvf;
    } else {
        r.tail = TAIL_SEPARATE;
        if (fuse_ln && blk.fc1.slab && L.hb_plane < (1L << 31)) r.fc1 = LNLIN_GEMM_LN;
        else r.fc1 = ln_linear(rs_route(fc1_gemm(c, blk), blk.fc1), blk.fc1);
        r.rs_fc2 = rs_route(fc2_gemm(c, blk), blk.fc2);
    }
    if (!r.fuse_proj) r.rs_proj = rs_route(proj_gemm(c, blk), blk.proj);
    return r;
}

// ------------------------------------------------------------------------------------------------ stages
// prepare_tokens (vision_transformer.py:224-235); the patch-gather matrix is hosted by A
int embed_tokens(const ForwardCtx& c, const void* x, int32_t x_kind) {
    const dinoseg_handle* h = c.env.h;
    const long pg_plane = (long)c.L.Mp * (3 * c.cfg->patch * c.cfg->patch);
    return ::embed_tokens(c.env, {x, x_kind, c.B, c.Hf, c.Wf, c.A, pg_plane, patch_planes(h), patch_fmt(h), c.X, c.disp_Mp});
}

// LayerNorm1 + qkv of a block -> Q / K / V
int run_ln_qkv(const ForwardCtx& c, const BlockRec& blk, LnLinear route) {
    if (route == LNLIN_TAIL) return 0;
    if (route == LNLIN_GEMM_LN) {
        LnGemmParams g = ln_gemm(c, blk.qkv, blk.norm1_w, blk.norm1_b, EPI_QKV);
        set_qkv(g, c.qkv());
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_QKV, DSEG_TRY(launch_gemm_ln(g, c.D, c.P, c.env.s)));
        return 0;
    }
    const GemmParams g = qkv_gemm(c, blk);
    if (route != LNLIN_RS_LN) DSEG_PROF_ENV(c.env, DINOSEG_PROF_LN, DSEG_TRY(layernorm_to_A(c, blk.norm1_w, blk.norm1_b)));
    DSEG_PROF_ENV(c.env, DINOSEG_PROF_QKV, DSEG_TRY(route == LNLIN_LN_GEMM ? launch_gemm(g, c.env.s) : launch_gemm_rs(to_rs(c, g, blk.qkv), c.env.s)));
    return 0;
}

int run_attention(const ForwardCtx& c) {
    AttnParams a = {};
    a.q = c.Q; a.k = c.K; a.v = c.V; a.qkv_plane = c.L.qkv_plane;
    a.ctx = c.CTX; a.ctx_plane = c.L.ctx_plane; a.lse = nullptr;
    a.B = c.B; a.heads = c.cfg->num_heads; a.ntok = c.L.ntok; a.npad = c.L.npad; a.planes = c.P; a.fmt = c.FM;
    a.shared_gpu = c.env.h->in_split ? 1 : 0;
    a.dispatch_B = c.disp_B;
    a.v_bf16 = c.v_bf16;
    DSEG_PROF_ENV(c.env, DINOSEG_PROF_ATTN, DSEG_TRY(launch_attention(a, c.env.s)));
    return 0;
}

// The last block with cls_mask (Block.forward, vision_transformer.py:127-140): the CLS token attends through each mask; its residual
// is repeated once per mask; MLP and the final norm run on those n_masks rows only.  The patch-token rows of X / A / CTX / HB are
// dead from here on and host the n_masks rows (checked: n_masks < ntok).
int run_masked_last_block(const ForwardCtx& c, const BlockRec& blk) {
    const ForwardRequest& rq = *c.rq;
    const WsLayout& L = c.L;
    const hipStream_t s = c.env.s;
    const int Nm = rq.n_masks, D = c.D, P = c.P, FM = c.FM;
    const float eps = c.cfg->ln_eps;
    DSEG_TRY(launch_cls_mask_attn(c.Q, c.K, c.V, L.qkv_plane, P, c.cfg->num_heads, L.ntok, L.npad, rq.cls_mask, Nm, c.CTX, L.ctx_plane,
                                  rq.mask_attn_out, s, FM));
    if (!rq.emb_out) return 0;
    float* Xm = c.X + D;                        // rows 1 .. Nm
    DSEG_TRY(launch_broadcast_row0(c.X, D, Nm, s));
    auto lin = [&](const LinearRec& l, const bf16_t* Ain, long a_plane, int epi, bf16_t* ob, long o_plane) -> int {
        GemmParams g = linear_gemm(l);
        g.A = Ain; g.a_plane = a_plane; g.lda = l.K;
        g.M = Nm; g.epi = epi;
        g.out_f32 = Xm; g.ldo_f32 = D;
        g.out_bf16 = ob; g.out_plane = o_plane; g.ldo = l.N;
        return launch_gemm_small(g, s);
    };
    DSEG_TRY(lin(blk.proj, c.CTX, L.ctx_plane, EPI_RESID, nullptr, 0));
    DSEG_TRY(launch_layernorm(Xm, blk.norm2_w, blk.norm2_b, eps, Nm, D, c.A, L.a_plane, P, nullptr, 0, L.ntok, s, FM));
    DSEG_TRY(lin(blk.fc1, c.A, L.a_plane, EPI_GELU, c.HB, L.hb_plane));
    DSEG_TRY(lin(blk.fc2, c.HB, L.hb_plane, EPI_RESID, nullptr, 0));
    return launch_layernorm(Xm, c.model->norm_w, c.model->norm_b, eps, Nm, D, c.A, L.a_plane, P, rq.emb_out, 0, L.ntok, s, FM);
}

// The second half of block i: x += proj(ctx) + b, x += fc2(gelu(fc1(LayerNorm2(x)))) (+ LayerNorm1 + qkv of block i + 1 where the
// route says so: a tap of this block's output still reads X, which is complete)
int run_block_tail(const ForwardCtx& c, const BlockRec& blk, int i, const BlockRoute& r) {
    const hipStream_t s = c.env.s;
    const WsLayout& L = c.L;
    if (!r.fuse_proj) {
        const GemmParams g = proj_gemm(c, blk);
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_PROJ, DSEG_TRY(r.rs_proj ? launch_gemm_rs(to_rs(c, g, blk.proj), s) : launch_gemm(g, s)));
    }
    if (r.tail == TAIL_FUSED3 || r.tail == TAIL_FUSED4) {
        // projection + LN2 + fc1 + GELU + fc2 + residual in one launch: on hi + lo planes (mlp_fused3.hip), or on one plane with one
        // wave per SIMD (mlp_fused4.hip: no plane strides, V always bf16)
        const bool x3 = r.tail == TAIL_FUSED3;
        MlpFused3Params g = {};
        g.X = c.X; g.eps = c.cfg->ln_eps;
        g.Wp = x3 ? blk.mlp3 : blk.mlp4; g.b2 = blk.fc2.b;
        g.M = L.M; g.fmt = c.FM;
        if (r.fuse_proj) {
            g.ctx = c.CTX; g.bproj = blk.proj.b;
            if (x3) g.ctx_plane = L.ctx_plane;
            if (r.writes_next_qkv) {
                set_qkv(g, c.qkv());
                if (x3) g.v_bf16 = c.v_bf16;
                else g.qkv_plane = 0;
            }
        }
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_FC1, DSEG_TRY(x3 ? launch_mlp_fused3(g, s) : launch_mlp_fused4(g, s)));
    } else if (r.tail == TAIL_FUSED2) {
        // LN2 + fc1 + GELU + fc2 + residual in one launch: the hidden activation never reaches HBM (mlp_fused2.hip)
        MlpFusedParams g = {};
        g.X = c.X; g.ldx = c.D; g.gamma = blk.norm2_w; g.beta = blk.norm2_b; g.eps = c.cfg->ln_eps;
        g.Wp = blk.mlp; g.b1 = blk.fc1.b; g.b2 = blk.fc2.b;
        g.M = L.M; g.fmt = c.FM;
        if (r.fuse_proj) {
            g.ctx = c.CTX; g.Wproj = blk.projf; g.bproj = blk.proj.b;
            if (r.writes_next_qkv) {
                const BlockRec& nb = c.model->blocks[i + 1];
                g.Wqkv = nb.qkvf; g.bqkv = nb.qkv.b;
                g.gamma1 = nb.norm1_w; g.beta1 = nb.norm1_b;
                set_qkv(g, c.qkv());
            }
        }
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_FC1, DSEG_TRY(launch_mlp_fused2(g, s)));
    } else {
        if (r.fc1 == LNLIN_GEMM_LN) {
            LnGemmParams g = ln_gemm(c, blk.fc1, blk.norm2_w, blk.norm2_b, EPI_GELU);
            set_hidden_out(g, c.HB, L.hb_plane, c.F);
            DSEG_PROF_ENV(c.env, DINOSEG_PROF_FC1, DSEG_TRY(launch_gemm_ln(g, c.D, c.P, s)));
        } else {
            const GemmParams g = fc1_gemm(c, blk);
            if (r.fc1 != LNLIN_RS_LN) DSEG_PROF_ENV(c.env, DINOSEG_PROF_LN, DSEG_TRY(layernorm_to_A(c, blk.norm2_w, blk.norm2_b)));
            DSEG_PROF_ENV(c.env, DINOSEG_PROF_FC1, DSEG_TRY(r.fc1 == LNLIN_LN_GEMM ? launch_gemm(g, s) : launch_gemm_rs(to_rs(c, g, blk.fc1), s)));
        }
        const GemmParams g = fc2_gemm(c, blk);
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_FC2, DSEG_TRY(r.rs_fc2 ? launch_gemm_rs(to_rs(c, g, blk.fc2), s) : launch_gemm(g, s)));
    }
    return 0;
}

// every token through the final norm, fp32 (VisionTransformer.forward(x, all=True) / forward(x, intermediate=k))
int final_norm_tokens(const ForwardCtx& c, float* out) {
    return launch_layernorm(c.X, c.model->norm_w, c.model->norm_b, c.cfg->ln_eps, c.L.M, c.D, nullptr, 0, 1, out, 0, c.L.ntok, c.env.s);
}

// final norm + head (+ the dense upsample, timed with the head: its output side)
int run_head(const ForwardCtx& c) {
    const ForwardRequest& rq = *c.rq;
    const WsLayout& L = c.L;
    float* logp = rq.logp_out ? rq.logp_out : reinterpret_cast<float*>(c.ws + L.HB);
    DSEG_TRY(::run_head(c.env, {c.X, L.M, L.Mp, L.ntok, c.FEAT, c.H1, c.H2, L.feat_plane, L.h1_plane, L.h2_plane, c.SF, logp, rq.argmax_out}));
    if (rq.wants_dense())
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_HEAD, DSEG_TRY(launch_upsample_argmax(logp, c.B, c.Hf / c.cfg->patch, c.Wf / c.cfg->patch, c.cfg->n_classes,
                                                                           rq.OH, rq.OW, rq.labels, rq.dense, c.env.s)));
    return 0;
}

// ------------------------------------------------------------------------------------------------ forward
int forward_impl(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t Hf, int32_t Wf, const ForwardRequest& rq,
                 void* stream, const SplitPart& part = {}) {
    DSEG_TRY(check_forward_args("dinoseg_forward", h, x, x_kind, B, Hf, Wf));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard(h);
    DSEG_TRY(check_stream_device(h, s));
    DSEG_TRY(dinoseg_prepare_resolution_hw(h, Hf, Wf, stream));
    ForwardCtx c;
    DSEG_TRY(begin_forward(c, h, B, Hf, Wf, rq, s, part));
    const int NB = h->cfg.n_blocks;
    const size_t xbytes = (size_t)c.L.M * c.D * sizeof(float);
    auto tap = [&](int after) -> int {
        if (rq.tap_block == after && rq.tap_out) DSEG_CHECK_HIP(hipMemcpyAsync(rq.tap_out, c.X, xbytes, hipMemcpyDeviceToDevice, s));
        return 0;
    };

    DSEG_TRY(embed_tokens(c, x, x_kind));
    DSEG_TRY(tap(0));
    // ---- transformer blocks (vision_transformer.py:122-140) ----
    BlockRoute route;
    for (int i = 0; i < NB; ++i) {
        const BlockRec& blk = h->model.blocks[i];
        const bool last = i == NB - 1;
        route = plan_block(c, blk, i, route);
        DSEG_TRY(run_ln_qkv(c, blk, route.qkv));
        if (rq.attn_out && last)        // get_last_selfattention: probabilities of the last block, then stop
            return launch_attn_probs(c.Q, c.K, c.L.qkv_plane, c.P, B, h->cfg.num_heads, c.L.ntok, c.L.npad, rq.attn_out, s, c.FM);
        if (rq.wants_cls_attention() && last) {
            DSEG_PROF_ENV(c.env, DINOSEG_PROF_ATTN, DSEG_TRY(launch_cls_attention(c.Q, c.K, c.L.qkv_plane, c.P, B, h->cfg.num_heads, c.L.ntok, c.L.npad,
                                                                              Hf / h->cfg.patch, Wf / h->cfg.patch, rq.OH, rq.OW,
                                                                              rq.cls_threshold, rq.cls_attn_out, rq.cls_keep_out, s, c.FM)));
            return 0;
        }
        if (rq.cls_mask && last) return run_masked_last_block(c, blk);
        DSEG_TRY(run_attention(c));
        DSEG_TRY(run_block_tail(c, blk, i, route));
        DSEG_TRY(tap(i + 1));
        if (rq.feat_out && rq.feat_blocks == i + 1 && !last) return final_norm_tokens(c, rq.feat_out);
    }
    if (rq.feat_out) return final_norm_tokens(c, rq.feat_out);
    return run_head(c);
}

// Option "streams" = 2: a batch of >= split_min frames runs as two half-batches, the first on the caller's stream, the second on
// the handle's internal stream (forked from and joined to the caller's stream by events, so the call keeps its stream-ordered
// semantics and stays capturable).  Frames are independent (pl_torch_modules.py:253 flattens them); kernels of different
// layers of the two halves overlap: one half's attention fills the CUs the other half's GEMM tail rounds and memory phases
// leave idle (measured: +4.5 % frames/s at B = 32; four quarter-batches: -5 %).  The two workspaces together are the size of one.
int forward_split(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, const ForwardRequest& rq, void* stream) {
    DSEG_TRY(check_forward_args("dinoseg_forward", h, x, x_kind, B, H, W));
    const bool split = options().streams >= 2 && B >= options().split_min && B >= 2 && rq.tap_block < 0 && !rq.tap_out;
    if (!split) return forward_impl(h, x, x_kind, B, H, W, rq, stream);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard(h);
    DSEG_TRY(check_stream_device(h, s));
    DSEG_TRY(ensure_aux_stream(h));
    DSEG_TRY(dinoseg_prepare_resolution_hw(h, H, W, stream));      // the resampled position embedding: before the fork, both halves read it
    const int B0 = (B + 1) / 2, B1 = B - B0;
    const long n = (long)(H / h->cfg.patch) * (W / h->cfg.patch);
    const size_t frame_bytes = x_kind == DINOSEG_INPUT_U8_HWC ? (size_t)H * W * 3 : (size_t)H * W * 3 * sizeof(float);
    const void* x1 = reinterpret_cast<const char*>(x) + (size_t)B0 * frame_bytes;
    DSEG_CHECK_HIP(hipEventRecord(h->ev_fork, s));
    DSEG_CHECK_HIP(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
    h->in_split = true;
    const ForwardRequest rq1 = second_half(rq, B0, n, h->cfg.n_classes);
    const int rc0 = forward_impl(h, x, x_kind, B0, H, W, rq, stream, {0, B});
    const int rc1 = forward_impl(h, x1, x_kind, B1, H, W, rq1, h->aux_stream, {1, B});
    h->in_split = false;
    // join even after an error: the caller's stream must not run ahead of work already queued on the internal one
    DSEG_CHECK_HIP(hipEventRecord(h->ev_join, h->aux_stream));
    DSEG_CHECK_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
    return rc0 ? rc0 : rc1;
}

}  // namespace

extern "C" int dinoseg_forward_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, float* logp_out,
                                  int32_t* argmax_out, int32_t tap_block, float* tap_out, void* stream) {
    ForwardRequest rq;
    rq.logp_out = logp_out; rq.argmax_out = argmax_out; rq.tap_block = tap_block; rq.tap_out = tap_out;
    return forward_split(h, x, x_kind, B, H, W, rq, stream);
}

// The forward, then the bilinear upsample + argmax of its log-probs (upsample.hip) behind the head on the same stream(s).  Everything the
// upsample would refuse is refused here, before the forward enqueues anything.
extern "C" int dinoseg_forward_dense_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t OH,
                                        int32_t OW, float* logp_out, int32_t* argmax_out, int32_t* labels_out, float* dense_out,
                                        void* stream) {
    if (!h || !x || B <= 0) {
        dinoseg_set_error("dinoseg_forward_dense_hw: bad argument (null handle or frames, or B=%d)", B);
        return -1;
    }
    if (!labels_out && !dense_out) {
        dinoseg_set_error("dinoseg_forward_dense_hw: null pointer (at least one of labels_out / dense_out is required)");
        return -1;
    }
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    const int hp = H / h->cfg.patch, wp = W / h->cfg.patch;
    if (upsample_check_shape("dinoseg_forward_dense_hw", B, hp, wp, h->cfg.n_classes, OH, OW)) return -1;
    ForwardRequest rq;
    rq.logp_out = logp_out; rq.argmax_out = argmax_out;
    rq.OH = OH; rq.OW = OW; rq.labels = labels_out; rq.dense = dense_out;
    return forward_split(h, x, x_kind, B, H, W, rq, stream);
}

// The forward into the caller's logp_out, then the two launches of the image-guided upsample (upsample_guided.hip) for the whole batch on
// the caller's stream, behind the join of the two-stream split.  The forward's own code paths are untouched.  Everything the launches
// would refuse is refused here, before the forward enqueues anything.
extern "C" int dinoseg_forward_guided_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W,
                                         const uint8_t* guide, int32_t OH, int32_t OW, int32_t radius, double sigma_spatial,
                                         double sigma_range, float* logp_out, uint32_t* cells_scratch, int32_t* labels_out, float* dense_out,
                                         void* stream) {
    const char* who = "dinoseg_forward_guided_hw";
    if (!h || !x || B <= 0) {
        dinoseg_set_error("%s: bad argument (null handle or frames, or B=%d)", who, B);
        return -1;
    }
    if (!guide || !logp_out || !cells_scratch || (!labels_out && !dense_out)) {
        dinoseg_set_error("%s: null pointer (guide, logp_out, cells_scratch, and at least one of labels_out / dense_out, are required)", who);
        return -1;
    }
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    const int hp = H / h->cfg.patch, wp = W / h->cfg.patch, C = h->cfg.n_classes;
    if (upsample_guided_check(who, B, hp, wp, C, OH, OW, radius, sigma_spatial, sigma_range, nullptr)) return -1;
    if (guide_cells_check(who, B, hp, wp, OH, OW)) return -1;
    ForwardRequest rq;
    rq.logp_out = logp_out;
    DSEG_TRY(forward_split(h, x, x_kind, B, H, W, rq, stream));
    DeviceGuard guard(h);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DSEG_TRY(launch_guide_cells(who, guide, B, OH, OW, hp, wp, cells_scratch, s));
    return launch_upsample_guided(who, logp_out, guide, cells_scratch, B, hp, wp, C, OH, OW, radius, sigma_spatial, sigma_range, labels_out,
                                  dense_out, s);
}

extern "C" int dinoseg_forward_refined_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W,
                                          const uint8_t* guide, int32_t OH, int32_t OW, double gain, const int32_t* dilations, int32_t n_dil,
                                          double sigma, int32_t iters, float* logp_out, void* scratch, int32_t* labels_out, float* dense_out,
                                          void* stream) {
    const char* who = "dinoseg_forward_refined_hw";
    if (!h || !x || B <= 0) {
        dinoseg_set_error("%s: bad argument (null handle or frames, or B=%d)", who, B);
        return -1;
    }
    if (!guide || !logp_out || !scratch || (!labels_out && !dense_out)) {
        dinoseg_set_error("%s: null pointer (guide, logp_out, scratch, and at least one of labels_out / dense_out, are required)", who);
        return -1;
    }
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    const int hp = H / h->cfg.patch, wp = W / h->cfg.patch, C = h->cfg.n_classes;
    if (refine_seed_check(who, REFINE_SEED_SCORES, B, C, OH, OW, hp, wp, gain)) return -1;
    if (refine_iterate_check(who, B, C, OH, OW, dilations, n_dil, sigma, iters, nullptr)) return -1;
    ForwardRequest rq;
    rq.logp_out = logp_out;
    DSEG_TRY(forward_split(h, x, x_kind, B, H, W, rq, stream));
    DeviceGuard guard(h);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DSEG_TRY(launch_refine_seed(who, logp_out, REFINE_SEED_SCORES, B, C, OH, OW, hp, wp, gain, scratch, s));
    return launch_refine_iterate(who, guide, scratch, B, C, OH, OW, dilations, n_dil, sigma, iters, labels_out, dense_out, s);
}

extern "C" int dinoseg_forward(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, float* logp_out,
                               int32_t* argmax_out, int32_t tap_block, float* tap_out, void* stream) {
    return dinoseg_forward_hw(h, x, x_kind, B, r, r, logp_out, argmax_out, tap_block, tap_out, stream);
}

extern "C" int dinoseg_last_selfattention_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W,
                                             float* attn_out, void* stream) {
    if (!attn_out || !h || h->cfg.n_blocks < 1) {
        dinoseg_set_error("dinoseg_last_selfattention: needs an output buffer and at least one block");
        return -1;
    }
    ForwardRequest rq;
    rq.attn_out = attn_out;
    return forward_impl(h, x, x_kind, B, H, W, rq, stream);
}

extern "C" int dinoseg_last_selfattention(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, float* attn_out,
                                          void* stream) {
    return dinoseg_last_selfattention_hw(h, x, x_kind, B, r, r, attn_out, stream);
}

// The forward up to the last block's LayerNorm1 + qkv, then the CLS attention launch (cls_attention.hip).  Everything that launch would
// refuse is refused here, before the forward enqueues anything.
extern "C" int dinoseg_cls_attention_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t OH,
                                        int32_t OW, float threshold, float* attn_out, uint8_t* keep_out, void* stream) {
    const char* who = "dinoseg_cls_attention_hw";
    if (!h || !x || B <= 0 || h->cfg.n_blocks < 1) {
        dinoseg_set_error("%s: bad argument (null handle or frames, B=%d, or a model without blocks)", who, B);
        return -1;
    }
    if (!attn_out && !keep_out) {
        dinoseg_set_error("%s: null pointer (at least one of attn_out / keep_out is required)", who);
        return -1;
    }
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    const int hp = H / h->cfg.patch, wp = W / h->cfg.patch;
    if ((long long)hp * wp + 1 > 0x7fffffffll) {
        dinoseg_set_error("%s: a %dx%d frame has too many tokens", who, H, W);
        return -1;
    }
    if (cls_attention_check(who, B, h->cfg.num_heads, hp * wp + 1, hp, wp, OH, OW, keep_out != nullptr, threshold)) return -1;
    ForwardRequest rq;
    rq.cls_attn_out = attn_out; rq.cls_keep_out = keep_out; rq.cls_threshold = threshold;
    rq.OH = OH; rq.OW = OW;
    return forward_impl(h, x, x_kind, B, H, W, rq, stream);
}

extern "C" int dinoseg_forward_mask_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t H, int32_t W, const float* cls_mask,
                                       int32_t n_masks, float* emb_out, float* attn_out, void* stream) {
    if (!h || h->cfg.n_blocks < 1 || !cls_mask || n_masks < 1 || (!emb_out && !attn_out)) {
        dinoseg_set_error("dinoseg_forward_mask: needs at least one block, n_masks >= 1 masks and one output buffer");
        return -1;
    }
    const int32_t pz = h->cfg.patch;
    if (frame_ok(H, W, pz) && n_masks >= (H / pz) * (W / pz) + 1) {
        dinoseg_set_error("dinoseg_forward_mask: n_masks=%d must be smaller than the token count %d", n_masks, (H / pz) * (W / pz) + 1);
        return -1;
    }
    ForwardRequest rq;
    rq.cls_mask = cls_mask; rq.n_masks = n_masks; rq.emb_out = emb_out; rq.mask_attn_out = attn_out;
    return forward_impl(h, x, x_kind, 1, H, W, rq, stream);
}

extern "C" int dinoseg_forward_mask(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t r, const float* cls_mask,
                                    int32_t n_masks, float* emb_out, float* attn_out, void* stream) {
    return dinoseg_forward_mask_hw(h, x, x_kind, r, r, cls_mask, n_masks, emb_out, attn_out, stream);
}

extern "C" int dinoseg_features_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t n_blocks,
                                   float* tokens_out, void* stream) {
    if (!h || !tokens_out || n_blocks < 0 || n_blocks > h->cfg.n_blocks) {
        dinoseg_set_error("dinoseg_features: needs an output buffer and 0 <= n_blocks <= %d", h ? h->cfg.n_blocks : 0);
        return -1;
    }
    ForwardRequest rq;
    rq.feat_out = tokens_out; rq.feat_blocks = n_blocks;
    return forward_impl(h, x, x_kind, B, H, W, rq, stream);
}

extern "C" int dinoseg_features(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, int32_t n_blocks,
                                float* tokens_out, void* stream) {
    return dinoseg_features_hw(h, x, x_kind, B, r, r, n_blocks, tokens_out, stream);
}
