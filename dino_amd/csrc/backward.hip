// The backward of the fine-tune step (dinoseg_backward, dinoseg_train_step*): gradients of the last training forward (train_api.hip),
// written into the caller-bound fp32 buffers.  Host code only: a per-call context (sizes, scratch pointers and the options, read
// once), the side stream of the blocks' weight gradients with its buffer hazards as a record, and the stages of the walk.
//
// Backward of y = act(x W^T + b), given dY (activation derivative already applied):
//   dX = dY . W          -> gemm.hip NT kernel with the transposed packed weight W^T[K][N] as the "W" operand (run_dgrad)
//   dW = dY^T . X        -> gemm_tn.hip from the row-major operands, the batch rows split into slices (run_wgrad_tn); the patch
//                           embedding (192 columns): both operands transposed to [*, rows] planes, same NT kernel (wgrad_nt)
//   db = column sums of dY (by-product of the weight-gradient kernel, of the LayerNorm backward that produced dY, or of a transpose)
#include <vector>

#include "train_ws.h"

namespace {

// ------------------------------------------------------------------------------------------------ context
// One backward call: built once by begin_backward, read by every stage: no stage reads the options itself
struct BackwardCtx {
    StepEnv env;                        // the handle, the caller's stream, profiled
    const dinoseg_config* cfg;
    const ModelRec* model;
    GradRec* grad;
    const int64_t* labels; const float* dlogp; float* loss_out;       // exactly one of labels (+ loss_out) and dlogp
    int B, oh, ow, D, F, P, HP, H, C, NB, ldz;
    bool mlp_head;
    TrainLayout L;
    char* ws;
    float *dX, *dA, *sink, *SPLITK, *NLSE, *NDEL, *DPOS, *ACC, *DET;
    bf16_t *dXp, *G, *dCTX, *T1, *T2, *DZ, *PATCH;
    // the options the walk depends on
    bool deterministic, two_streams, plain_tn_grid;     // train_streams >= 2; route_ab & 4
    int splitk;                                         // splitk_tiles, clamped to what the workspace holds
    TrainWs saved() const { return {ws, L}; }
    float* gsink(const GradSlot& g) const { return g.ptr ? g.ptr : sink; }      // (LayerNorm backward always writes its gain / shift sums)
};

int begin_backward(dinoseg_handle* h, const int64_t* labels, const float* dlogp, float* loss_out, hipStream_t s, BackwardCtx& c) {
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
    const dinoseg_config& cf = h->cfg;
    c.env = {h, s, true};
    c.cfg = &cf; c.model = &h->model; c.grad = &h->grad;
    c.labels = labels; c.dlogp = dlogp; c.loss_out = loss_out;
    c.B = h->tr_B; c.oh = h->tr_H / cf.patch; c.ow = h->tr_W / cf.patch;
    c.D = cf.embed_dim; c.F = c.D * cf.mlp_ratio; c.P = h->planes; c.HP = head_planes(); c.H = cf.num_heads; c.C = cf.n_classes;
    c.NB = cf.n_blocks; c.ldz = dz_ld(c.C);
    c.mlp_head = cf.head_kind == DINOSEG_HEAD_MLP;
    c.L = make_train_layout(h, c.B, h->tr_H, h->tr_W);
    c.ws = h->tws;
    const TrainLayout& L = c.L;
    const TrainWs w = c.saved();
    c.dX = w.f32(L.dX); c.dA = w.f32(L.dA); c.sink = w.f32(L.SINK); c.SPLITK = w.f32(L.SPLITK);
    c.NLSE = w.f32(L.NLSE); c.NDEL = w.f32(L.NDEL); c.DPOS = w.f32(L.DPOS); c.ACC = w.f32(L.ACC); c.DET = w.f32(L.DET);
    c.dXp = w.b16(L.dXp); c.G = w.b16(L.G); c.dCTX = w.b16(L.dCTX); c.T1 = w.b16(L.T1); c.T2 = w.b16(L.T2);
    c.DZ = w.b16(L.DZ); c.PATCH = w.b16(L.PATCH);
    const Options& o = options();
    c.deterministic = o.deterministic != 0;
    c.two_streams = o.train_streams >= 2;
    c.plain_tn_grid = (o.route_ab & 4) != 0;
    c.splitk = splitk_budget();
    return 0;
}

// ------------------------------------------------------------------------------------------------ process and handle state
// Option deterministic: the launchers write per-block partial sums into a scratch area of the workspace and add them in a fixed
// order (train.hip, gemm_tn.hip) instead of fp32 atomics.  The scratch pointer is process-wide state read by the launchers: a second
// backward entered while it is set (another host thread stepping another handle) would write its partial sums into THIS handle's
// workspace -- refused instead.  Cleared on every way out
struct DetScratchGuard {
    bool mine = false;
    int claim(float* det) {
        if (det_scratch().ptr != nullptr) {
            dinoseg_set_error("dinoseg_backward: option deterministic allows one backward at a time per process (another one is being queued)");
            return -1;
        }
        det_scratch() = DetScratch{det, DET_FLOATS, {det + DET_FLOATS, det + DET_FLOATS + DET_TN_FLOATS}, DET_TN_FLOATS};
        mine = true;
        return 0;
    }
    ~DetScratchGuard() { if (mine) det_scratch() = DetScratch{nullptr, 0, {nullptr, nullptr}, 0}; }
};

// stage events: a side stream can start reducing a gradient bucket while the rest of backward still runs (handle.h: stage_ev)
struct StageEvents {
    dinoseg_handle* h;
    int mark(int stage, hipStream_t on) const {
        while ((int)h->stage_ev.size() <= stage) {
            hipEvent_t ev;
            DSEG_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            h->stage_ev.push_back(ev);
        }
        DSEG_CHECK_HIP(hipEventRecord(h->stage_ev[stage], on));
        h->stage_done = stage + 1;
        return 0;
    }
};

// Side stream for the blocks' weight gradients (option train_streams = 2).  dW = dY^T . X reads what the input-gradient chain
// has already produced and feeds nothing but the optimiser, so it runs beside that chain on the handle's internal stream:
// the chain's tail rounds and memory-bound kernels (LayerNorm backward, the attention prep) leave CUs idle that the
// weight-gradient tiles fill.  fork(): the side stream waits for everything queued on the caller's stream so far; mark() yields an
// event the caller's stream waits on (wait) before it overwrites an operand the side kernels read, and before every
// gradient-stage event.  Fork and join are events only: the call stays stream-ordered for the caller and capturable.  With one
// stream `stream` is the caller's, mark() yields null and wait() of null does nothing.
// (deterministic mode: the side stream's only partial sums are gemm_tn's bias sums: they have their own part of the scratch area)
struct SideStream {
    dinoseg_handle* h;
    hipStream_t caller, stream;       // stream: the handle's internal one, or the caller's again when the option is off
    bool on = false;
    size_t next = 0;        // into the handle's pool of fork / join events (bw_ev), reused from the start by every backward
    int open(dinoseg_handle* h_, hipStream_t s, bool two_streams) {
        h = h_; caller = stream = s; on = two_streams;
        if (on) {
            DSEG_TRY(ensure_aux_stream(h));
            stream = h->aux_stream;
        }
        return 0;
    }
    int event(hipEvent_t* out) {
        if (next == h->bw_ev.size()) {
            hipEvent_t ev;
            DSEG_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            h->bw_ev.push_back(ev);
        }
        *out = h->bw_ev[next++];
        return 0;
    }
    int fork() {
        if (!on) return 0;
        hipEvent_t ev;
        DSEG_TRY(event(&ev));
        DSEG_CHECK_HIP(hipEventRecord(ev, caller));
        DSEG_CHECK_HIP(hipStreamWaitEvent(stream, ev, 0));
        return 0;
    }
    int mark(hipEvent_t* done) {
        *done = nullptr;
        if (!on) return 0;
        DSEG_TRY(event(done));
        DSEG_CHECK_HIP(hipEventRecord(*done, stream));
        return 0;
    }
    int wait(hipEvent_t& done) const {
        if (done) DSEG_CHECK_HIP(hipStreamWaitEvent(caller, done, 0));
        done = nullptr;
        return 0;
    }
};

// What a pending side-stream weight-gradient GEMM still reads, as the event recorded behind that GEMM (null: nothing pending).  The
// caller's stream waits on the field directly in front of the launch that overwrites the buffer:
//   buffer | read by (side stream)     | next writer (caller's stream)
//   dXp    | mlp.fc2 weight gradient   | norm2 backward of the same block
//   G      | mlp.fc1 weight gradient   | attention backward of the same block (d qkv)
//   dXp    | attn.proj weight gradient | norm1 backward of the same block
//   G      | attn.qkv weight gradient  | mlp.fc2 input gradient of the NEXT block of the walk (d Hpre); behind block 0 the join in
//          |                           | front of the embeddings, which also reuse the split-K partial tiles
// One record lives across the block loop: G_read_by_qkv is the only field a block leaves set.
struct SideHazards {
    hipEvent_t dXp_read_by_fc2 = nullptr, G_read_by_fc1 = nullptr, dXp_read_by_proj = nullptr, G_read_by_qkv = nullptr;
};

// ------------------------------------------------------------------------------------------------ gradient GEMMs of the step
// dX[rows, k_out] = dY . W of one linear; the call site adds the epilogue's output (out_f32, or out_bf16 + out_plane [+ aux])
Dgrad dgrad_of(Planes dY, int rows, const LinearGrad& wt, int k_out, int planes, int epi) {
    Dgrad a = {};
    a.dY = dY; a.Wt = wt.tw; a.w_plane = wt.t_plane;
    a.M = rows; a.N = k_out; a.K = dY.ld; a.planes = planes; a.epi = epi;
    a.ldo_f32 = a.ldo = k_out;
    return a;
}
int dgrad_f32(const BackwardCtx& c, Planes dY, int rows, const LinearGrad& wt, int k_out, int planes, float* out) {
    Dgrad a = dgrad_of(dY, rows, wt, k_out, planes, EPI_PLAIN);
    a.out_f32 = out;
    return run_dgrad(a, c.env.s);
}
int dgrad_planes(const BackwardCtx& c, Planes dY, int rows, const LinearGrad& wt, int planes, int epi, Planes out, Planes aux) {
    Dgrad a = dgrad_of(dY, rows, wt, out.ld, planes, epi);
    a.out_bf16 = const_cast<bf16_t*>(out.p); a.out_plane = out.plane;
    a.aux = aux.p; a.aux_plane = aux.plane;
    return run_dgrad(a, c.env.s);
}

// Weight (and, with_bias, bias) gradient of one linear [n_rows][k_cols] on stream `on`, X stored X.ld >= k_cols wide: the step's slice
// count, partial tiles and scratch region.  When the weight is frozen the kernel still runs for the column sums alone if colsum_alone
// (the head layers); otherwise (the block linears) a pack pass over Y produces them
int wgrad_tn(const BackwardCtx& c, Planes Y, Planes X, int m_rows, int n_rows, int k_cols, int planes, const LinearGrad& lg, bool with_bias,
             hipStream_t on, bool colsum_alone) {
    WgradTn a = {};
    a.Y = Y; a.X = X; a.M = m_rows; a.N = n_rows; a.Kc = X.ld; a.planes = planes;
    a.dW = lg.dw.ptr; a.ldw = a.k_cols = k_cols; a.colsum = with_bias ? lg.db.ptr : nullptr;
    a.det_region = on != c.env.s;
    if (!a.dW && !a.colsum) return 0;
    if (!a.dW && !colsum_alone)
        return launch_transpose_planes(nullptr, Y.p, Y.plane, Y.ld, m_rows, n_rows, nullptr, 0, pad128(n_rows), c.L.Mpad, nullptr, 0, 0,
                                       a.colsum, planes, 0, 0, on, a.det_region);
    a.ksplit = tn_slices(c.splitk, c.plain_tn_grid, m_rows, n_rows, a.Kc);
    a.part = c.SPLITK;
    return run_wgrad_tn(a, on);
}
// ... of a block linear beside the input-gradient chain: the side stream forks, runs it and leaves its event in *done
int side_wgrad(const BackwardCtx& c, SideStream& side, Planes Y, Planes X, int n_rows, int k_cols, const LinearGrad& lg, bool with_bias,
               hipEvent_t* done) {
    DSEG_TRY(side.fork());
    DSEG_TRY(wgrad_tn(c, Y, X, c.L.M, n_rows, k_cols, c.P, lg, with_bias, side.stream, false));
    return side.mark(done);
}

// ------------------------------------------------------------------------------------------------ stages
// transposed packed weights for dX = dY . W  (weights change every optimiser step: repack)
int pack_transposed_weights(const BackwardCtx& c) {
    dinoseg_handle* h = c.env.h;
    const ModelRec& m = *c.model;
    GradRec& gr = *c.grad;
    std::vector<std::pair<const LinearRec*, LinearGrad*>> lins;      // every linear with an input gradient, in twbuf order
    for (int l = 0; l < c.NB; ++l) {
        const BlockRec& blk = m.blocks[l];
        BlockGrad& bg = gr.blocks[l];
        lins.insert(lins.end(), {{&blk.qkv, &bg.qkv}, {&blk.proj, &bg.proj}, {&blk.fc1, &bg.fc1}, {&blk.fc2, &bg.fc2}});
    }
    if (c.mlp_head) lins.insert(lins.end(), {{&m.head[0], &gr.head[0]}, {&m.head[1], &gr.head[1]}});
    lins.push_back({&m.clf, &gr.clf});
    auto bytes = [](const LinearRec& r, const LinearGrad& g) { return align_up((size_t)r.planes * g.t_plane * 2, 256); };
    size_t total = 0;
    for (auto& rg : lins) total += bytes(*rg.first, *rg.second);
    DSEG_TRY(grow_device_buffer(h->twbuf, h->twbuf_bytes, total, c.env.s));
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
    return launch_multi_pack(jobs.data(), (int)jobs.size(), c.env.s);
}

// gradients are written, not accumulated: zero every bound buffer (one launch instead of ~50 memset nodes).  *backbone: a dino.*
// gradient is bound
int zero_bound_grads(const BackwardCtx& c, bool* backbone) {
    std::vector<float*> zp;
    std::vector<long> zn;
    *backbone = false;
    for (auto& kv : c.env.h->grad_index) {
        const GradSlot& g = *kv.second;
        if (!g.ptr) continue;
        zp.push_back(g.ptr);
        zn.push_back(g.numel);
        *backbone |= g.backbone;
    }
    return zp.empty() ? 0 : launch_multi_zero((int)zp.size(), zp.data(), zn.data(), c.env.s);
}

// loss and d logits (pl_torch_modules.py:264-265), then the head down to dA = d loss / d final-norm rows (only if the backbone trains);
// stage 0
int head_backward(const BackwardCtx& c, bool backbone, const StageEvents& stages) {
    const TrainLayout& L = c.L;
    const GradRec& gr = *c.grad;
    const hipStream_t s = c.env.s;
    const auto [Xfin, LOGP, FEAT, H1, H2] = c.saved().head();
    const int D = c.D, HP = c.HP, Mp = L.Mp;
    DSEG_TRY(launch_nll_loss_grad(LOGP, c.labels, c.dlogp, Mp, c.C, c.ACC, c.env.h->bad_label_flag, c.loss_out, c.DZ, L.dz_plane, c.ldz, s));
    const Planes dz = {c.DZ, L.dz_plane, c.ldz}, feat = {FEAT, L.feat_plane, D};
    if (!c.mlp_head) {
        DSEG_TRY(wgrad_tn(c, dz, feat, Mp, c.C, D, HP, gr.clf, true, s, true));
        if (backbone) DSEG_TRY(dgrad_f32(c, dz, Mp, gr.clf, D, HP, c.dA));
        return stages.mark(0, s);
    }
    // weight and bias gradients straight from the row-major planes (gemm_tn.hip); h2 / h1 are stored 128 / 256 wide, zero beyond their
    // 100 / 200 columns.  d h2 [HP][Mp][128] lives in G, d h1 [HP][Mp][256] in dCTX (fits: Mp * 256 <= M * D)
    const Planes h1 = {H1, L.h1_plane, HEAD_H1_PAD}, h2 = {H2, L.h2_plane, HEAD_H2_PAD};
    const Planes dh2 = {c.G, (long)Mp * HEAD_H2_PAD, HEAD_H2_PAD}, dh1 = {c.dCTX, (long)Mp * HEAD_H1_PAD, HEAD_H1_PAD};
    // layer_3: z = h2 W3^T + b3
    DSEG_TRY(wgrad_tn(c, dz, h2, Mp, c.C, HEAD_H2, HP, gr.clf, true, s, true));
    DSEG_TRY(dgrad_planes(c, dz, Mp, gr.clf, HP, EPI_DRELU, dh2, h2));
    // layer_2
    DSEG_TRY(wgrad_tn(c, dh2, h1, Mp, HEAD_H2, HEAD_H1, HP, gr.head[1], true, s, true));
    DSEG_TRY(dgrad_planes(c, dh2, Mp, gr.head[1], HP, EPI_DRELU, dh1, h1));
    // layer_1
    DSEG_TRY(wgrad_tn(c, dh1, feat, Mp, HEAD_H1, D, HP, gr.head[0], true, s, true));
    if (backbone) DSEG_TRY(dgrad_f32(c, dh1, Mp, gr.head[0], D, HP, c.dA));
    return stages.mark(0, s);
}

// final norm (CLS rows get no gradient from the head).  Every LayerNorm backward also leaves its dX rows as bf16 planes dXp and their
// column sums = the bias gradient of the layer the walk reaches next: mlp.fc2 of the last block here
int final_norm_backward(const BackwardCtx& c) {
    const GradRec& gr = *c.grad;
    const float* Xfin = c.saved().head().Xfin;
    return launch_layernorm_bwd(c.dA, Xfin, c.model->norm_w, c.cfg->ln_eps, c.L.M, c.D, c.dX, 0, c.gsink(gr.norm_w), c.gsink(gr.norm_b), 1,
                                c.L.ntok, c.env.s, c.dXp, c.L.a_plane, c.P, c.NB > 0 ? gr.blocks[c.NB - 1].fc2.db.ptr : nullptr);
}

// Block l: dX = d loss / d X_out (fp32, kept along the residual branch) and its planes dXp come in, those of X_in go out.  The four
// weight gradients run on the side stream; hz (above) says what they still read
int block_backward(const BackwardCtx& c, SideStream& side, int l, SideHazards& hz) {
    const TrainLayout& L = c.L;
    const BlockRec& blk = c.model->blocks[l];
    const BlockGrad& bg = c.grad->blocks[l];
    const hipStream_t s = c.env.s;
    const auto [Xin, Xmid, LSE, A1, Q, Kb, V, CTX, A2, HPRE, HB] = c.saved().block(l);
    const int D = c.D, F = c.F, P = c.P, M = L.M;
    const Planes dxp = {c.dXp, L.a_plane, D}, dhid = {c.G, (long)M * F, F}, dqkv = {c.G, (long)M * 3 * D, 3 * D}, dctx = {c.dCTX, L.a_plane, D};
    // ---- mlp.fc2 : X_out = X_mid + H W2^T + b      (dXp and the fc2 bias gradient were left by the LayerNorm backward that produced dX)
    DSEG_TRY(side_wgrad(c, side, dxp, {HB, L.f_plane, F}, D, F, bg.fc2, false, &hz.dXp_read_by_fc2));
    // dHpre = (dX . W2) * gelu'(Hpre)
    DSEG_TRY(side.wait(hz.G_read_by_qkv));
    DSEG_TRY(dgrad_planes(c, dxp, M, bg.fc2, P, EPI_DGELU, dhid, {HPRE, L.f_plane, F}));
    // ---- mlp.fc1 : Hpre = A2 W1^T + b
    DSEG_TRY(side_wgrad(c, side, dhid, {A2, L.a_plane, D}, F, D, bg.fc1, true, &hz.G_read_by_fc1));
    DSEG_TRY(dgrad_f32(c, dhid, M, bg.fc1, D, P, c.dA));
    // ---- norm2 (input X_mid); the residual branch keeps dX.  By-products: dXp and the proj bias gradient
    DSEG_TRY(side.wait(hz.dXp_read_by_fc2));
    DSEG_TRY(launch_layernorm_bwd(c.dA, Xmid, blk.norm2_w, c.cfg->ln_eps, M, D, c.dX, 1, c.gsink(bg.norm2_w), c.gsink(bg.norm2_b), 0, L.ntok, s,
                                  c.dXp, L.a_plane, P, bg.proj.db.ptr));
    // ---- attn.proj : X_mid = X_in + ctx Wp^T + b
    DSEG_TRY(side_wgrad(c, side, dxp, {CTX, L.a_plane, D}, D, D, bg.proj, false, &hz.dXp_read_by_proj));
    DSEG_TRY(dgrad_planes(c, dxp, M, bg.proj, P, EPI_BF16, dctx, {nullptr, 0, 0}));
    // ---- attention
    DSEG_TRY(side.wait(hz.G_read_by_fc1));
    {
        AttnBwdParams a = {};
        a.q = Q; a.k = Kb; a.v = V; a.qkv_plane = L.qkv_plane;
        a.dO = c.dCTX; a.O = CTX; a.dO_plane = L.a_plane; a.lse = LSE;
        a.neg_lse = c.NLSE; a.neg_delta = c.NDEL;
        a.dqkv = c.G; a.dqkv_plane = dqkv.plane;
        a.B = c.B; a.heads = c.H; a.ntok = L.ntok; a.npad = L.npad; a.planes = P;
        DSEG_PROF_ENV(c.env, DINOSEG_PROF_ATTN_BWD, DSEG_TRY(launch_attention_bwd(a, s)));
    }
    // ---- attn.qkv : qkv = A1 Wqkv^T + b
    DSEG_TRY(side_wgrad(c, side, dqkv, {A1, L.a_plane, D}, 3 * D, D, bg.qkv, true, &hz.G_read_by_qkv));
    DSEG_TRY(dgrad_f32(c, dqkv, M, bg.qkv, D, P, c.dA));
    // ---- norm1 (input X_in).  By-products for mlp.fc2 of block l-1; the embedding step after block 0 packs dX itself: it drops the CLS rows
    DSEG_TRY(side.wait(hz.dXp_read_by_proj));
    return launch_layernorm_bwd(c.dA, Xin, blk.norm1_w, c.cfg->ln_eps, M, D, c.dX, 1, c.gsink(bg.norm1_w), c.gsink(bg.norm1_b), 0, L.ntok, s,
                                l > 0 ? c.dXp : nullptr, L.a_plane, P, l > 0 ? c.grad->blocks[l - 1].fc2.db.ptr : nullptr);
}

// embeddings: tokens = [cls ; conv(patches)] + pos   (vision_transformer.py:224-235); the last stage
int embed_backward(const BackwardCtx& c, const StageEvents& stages) {
    const TrainLayout& L = c.L;
    const GradRec& gr = *c.grad;
    const dinoseg_config& cf = *c.cfg;
    const hipStream_t s = c.env.s;
    const int D = c.D, P = c.P;
    DSEG_TRY(launch_batch_sum_rows(c.dX, c.B, L.ntok, D, c.DPOS, s));
    if (gr.cls_token.ptr) DSEG_CHECK_HIP(hipMemcpyAsync(gr.cls_token.ptr, c.DPOS, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
    // (scratch: the T2 transpose buffer, idle until the patch-embed gradient below; make_train_layout sizes it for [pos_grid][W/patch][D] floats)
    if (gr.pos_embed.ptr) {
        if ((size_t)cf.pos_grid * c.ow * D * sizeof(float) > L.t2_bytes) {
            dinoseg_set_error("dinoseg_backward: pos-embed scratch does not fit (pos_grid %d, grid %d x %d)", cf.pos_grid, c.oh, c.ow);
            return -1;
        }
        DSEG_TRY(launch_pos_resample_bwd(c.DPOS, cf.pos_grid, D, c.oh, c.ow, gr.pos_embed.ptr, reinterpret_cast<float*>(c.T2), s));
    }
    const long tpl = L.t_plane;
    DSEG_TRY(launch_transpose_planes(c.dX, nullptr, 0, D, L.Mp, D, c.T1, tpl, pad128(D), L.Mppad, nullptr, 0, 0, gr.patch.db.ptr, P, 1, L.ntok, s));
    if (!gr.patch.dw.ptr) return stages.mark(c.NB + 1, s);
    // dW[D, kp] += dY^T . X from the transposed planes T1 (d tokens without the CLS rows) and T2 (the saved patch matrix)
    const int kp = 3 * cf.patch * cf.patch;       // 192 columns in 256 transposed rows at patch 8; 768 in 768 at patch 16
    if ((long)pad128(kp) * L.Mppad > tpl) {
        dinoseg_set_error("dinoseg_backward: the transposed patch matrix (%d x %d) does not fit its plane (%ld)", pad128(kp), L.Mppad, tpl);
        return -1;
    }
    DSEG_TRY(launch_transpose_planes(nullptr, c.PATCH, L.patch_plane, kp, L.Mp, kp, c.T2, tpl, pad128(kp), L.Mppad, nullptr, 0, 0, nullptr, P, 0, 0, s));
    DSEG_TRY(wgrad_nt(c.T1, c.T2, tpl, L.Mppad, D, pad128(kp), kp, P, wgrad_nt_slices(c.splitk, D, pad128(kp), L.Mppad), c.SPLITK, gr.patch.dw.ptr, s));
    return stages.mark(c.NB + 1, s);
}

// Backward of the last train_forward_impl.  Exactly one of (labels, dlogp) is given:
//   labels : loss = F.nll_loss(logp, labels) (mean over the rows whose label is not -100) -> *loss_out, then backward of it
//   dlogp  : fp32 [B*n, C] upstream gradient d L / d logp (torch.autograd path)
// Gradients are written (not accumulated) into the buffers bound with dinoseg_bind_grad.
int train_backward_impl(dinoseg_handle* h, const int64_t* labels, const float* dlogp, float* loss_out, hipStream_t s) {
    BackwardCtx c;
    DSEG_TRY(begin_backward(h, labels, dlogp, loss_out, s, c));
    DSEG_TRY(pack_transposed_weights(c));
    bool backbone = false;
    DSEG_TRY(zero_bound_grads(c, &backbone));
    DetScratchGuard det;
    if (c.deterministic) DSEG_TRY(det.claim(c.DET));
    h->stage_done = 0;
    const StageEvents stages = {h};
    SideStream side;
    DSEG_TRY(side.open(h, s, c.two_streams));
    DSEG_TRY(head_backward(c, backbone, stages));
    if (!backbone) return 0;      // frozen backbone (freeze_bb, pl_torch_modules.py:434-436): only the head trains
    DSEG_TRY(final_norm_backward(c));
    SideHazards hz;     // hz.G_read_by_qkv is carried from block l into block l - 1, and out of block 0 into the join below
    for (int l = c.NB - 1; l >= 0; --l) {
        DSEG_TRY(block_backward(c, side, l, hz));
        // this block's gradients are complete once the side stream has finished its qkv weight gradient; the stage event is
        // recorded on the side stream (it has waited for everything the block queued on s up to the qkv weight gradient -- the
        // LayerNorm backward of norm1 is covered by the extra fork), so the caller's stream does not stall here
        if (side.on) {
            DSEG_TRY(side.fork());
            DSEG_TRY(stages.mark(1 + (c.NB - 1 - l), side.stream));
            continue;
        }
        DSEG_TRY(stages.mark(1 + (c.NB - 1 - l), s));
    }
    // join: the caller's stream continues (and the call returns) behind everything the side stream did
    DSEG_TRY(side.wait(hz.G_read_by_qkv));
    return embed_backward(c, stages);
}

}  // namespace

// The backward forks weight-gradient kernels onto the handle's side stream (option train_streams = 2) and joins them before it
// returns.  An error in between returns early: join here too, so that the caller's stream never runs ahead of side-stream kernels
// that still read / write the gradient buffers, the split-K workspace or the activations (as dinoseg_forward does for its halves).
int backward_joined(dinoseg_handle* h, const int64_t* labels, const float* dlogp, float* loss_out, hipStream_t s) {
    const int rc = train_backward_impl(h, labels, dlogp, loss_out, s);
    if (rc != 0 && h && h->aux_stream && h->ev_join) {
        (void)hipEventRecord(h->ev_join, h->aux_stream);
        (void)hipStreamWaitEvent(s, h->ev_join, 0);
    }
    return rc;
}
