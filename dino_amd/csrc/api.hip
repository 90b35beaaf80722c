// C-ABI of libdinoseg_hip.so (see include/dinoseg.h): handle, weight binding / packing, workspaces, options, profiling and the
// stand-alone ops.  The forward of the DINOSeg hot path is forward.hip, the fine-tune step train_api.hip (its backward: backward.hip).  Host code only; kernels
// live in gemm.hip / attention.hip / elementwise.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "handle.h"

using namespace dseg;

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";

extern "C" void dinoseg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* dinoseg_last_error(void) { return g_err; }
extern "C" int dinoseg_version(void) { return 300; }      // 3.0: fused MLP kernel, two streams by default; the measurement kernel moved to libdinoseg_tools.so

int device_cu_count() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        dinoseg_set_error("hipGetDevice failed");
        return -1;
    }
    if (dev >= 0 && dev < 64 && cache[dev].load() > 0) return cache[dev].load();
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        dinoseg_set_error("hipDeviceGetAttribute(MultiprocessorCount) failed on device %d", dev);
        return -1;
    }
    if (dev >= 0 && dev < 64) cache[dev].store(n);
    return n;
}



static std::string block_prefix(int i) { return "dino.blocks." + std::to_string(i) + "."; }

// every nn.Linear-shaped parameter pair: its names, its logical [N, K] and the padded [n_pad, k_pad] of its operand planes, its record
// in m and its gradient slots in g and, for a block linear, its block and gemm_rs option bit (LinearRec::rs_bit).  The ONE shape
// table of the linears: the bind API's index, the refresh and the transposed copies of the fine-tune step all follow it
struct LinSpec {
    std::string wname, bname;
    int N, K, n_pad, k_pad, planes, fmt;
    LinearRec* rec;
    int block, rs_bit;
    LinearGrad* grad;
    int t_n_pad;        // columns of the transposed copy W^T [k_pad][t_n_pad] (0: none)
    bool pack;          // operand planes in wbuf (the classifier has them only for the wide head kernel)
};

static std::vector<LinSpec> linear_specs(dinoseg_handle* h, ModelRec& m) {
    const dinoseg_config& c = h->cfg;
    const int D = c.embed_dim, F = c.embed_dim * c.mlp_ratio, P = h->planes, FM = h->fmt, HP = head_planes(), SF = split_fmt(h), C = c.n_classes;
    GradRec& g = h->grad;
    std::vector<LinSpec> v;
    // (fp16 mode: the patch embedding runs split like the head -- 0.13 % of the FLOPs, and its operands are raw pixels)
    v.push_back({"dino.patch_embed.proj.weight", "dino.patch_embed.proj.bias", D, 3 * c.patch * c.patch, D, 3 * c.patch * c.patch, patch_planes(h), patch_fmt(h), &m.patch, -1, 0, &g.patch, 0, true});
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string b = block_prefix(i);
        BlockRec& k = m.blocks[i];
        BlockGrad& kg = g.blocks[i];
        v.push_back({b + "attn.qkv.weight", b + "attn.qkv.bias", 3 * D, D, 3 * D, D, P, FM, &k.qkv, i, 2, &kg.qkv, 3 * D, true});
        v.push_back({b + "attn.proj.weight", b + "attn.proj.bias", D, D, D, D, P, FM, &k.proj, i, 4, &kg.proj, D, true});
        v.push_back({b + "mlp.fc1.weight", b + "mlp.fc1.bias", F, D, F, D, P, FM, &k.fc1, i, 1, &kg.fc1, F, true});
        v.push_back({b + "mlp.fc2.weight", b + "mlp.fc2.bias", D, F, D, F, P, FM, &k.fc2, i, 4, &kg.fc2, D, true});
    }
    const bool mlp = c.head_kind == DINOSEG_HEAD_MLP;
    if (mlp) {
        v.push_back({"clf.layer_1.weight", "clf.layer_1.bias", HEAD_H1, D, HEAD_H1_PAD, D, HP, SF, &m.head[0], -1, 0, &g.head[0], HEAD_H1_PAD, true});
        v.push_back({"clf.layer_2.weight", "clf.layer_2.bias", HEAD_H2, HEAD_H1, HEAD_H2_PAD, HEAD_H1_PAD, HP, SF, &m.head[1], -1, 0, &g.head[1], HEAD_H2_PAD, true});
    }
    // the classifier: launch_head_final reads it in fp32; more than 32 classes: also as hi+lo planes [round_up(C, 32)][ld] for the wide
    // kernel (head_wide.hip).  Its transposed copy pads the classes to the width of the d logits planes instead
    v.push_back({mlp ? "clf.layer_3.weight" : "clf.layer_1.weight", mlp ? "clf.layer_3.bias" : "clf.layer_1.bias", C, mlp ? HEAD_H2 : D,
                 (C + 31) / 32 * 32, mlp ? HEAD_H2_PAD : D, HP, SF, &m.clf, -1, 0, &g.clf, dz_ld(C), C > HEAD_FINAL_MAX_C});
    return v;
}

// the bind API's name index, built once: the expected shape of every key and the gradient slot it names
static void index_params(dinoseg_handle* h) {
    const dinoseg_config& c = h->cfg;
    const int64_t D = c.embed_dim, p = c.patch;
    GradRec& g = h->grad;
    g.blocks.resize(c.n_blocks);
    ModelRec unused;        // (the table also names each linear's record: no use for that here)
    unused.blocks.resize(c.n_blocks);
    auto add = [&](const std::string& name, std::vector<int64_t> shape, GradSlot& slot) {
        slot.numel = 1;
        for (int64_t d : shape) slot.numel *= (long)d;
        slot.backbone = name.rfind("dino.", 0) == 0;
        h->expected[name] = std::move(shape);
        h->grad_index[name] = &slot;
    };
    add("dino.cls_token", {1, 1, D}, g.cls_token);
    add("dino.pos_embed", {1, (int64_t)c.pos_grid * c.pos_grid + 1, D}, g.pos_embed);
    add("dino.norm.weight", {D}, g.norm_w);
    add("dino.norm.bias", {D}, g.norm_b);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string b = block_prefix(i);
        add(b + "norm1.weight", {D}, g.blocks[i].norm1_w);
        add(b + "norm1.bias", {D}, g.blocks[i].norm1_b);
        add(b + "norm2.weight", {D}, g.blocks[i].norm2_w);
        add(b + "norm2.bias", {D}, g.blocks[i].norm2_b);
    }
    for (const LinSpec& sp : linear_specs(h, unused)) {
        if (sp.grad == &g.patch) add(sp.wname, {D, 3, p, p}, sp.grad->dw);      // (the one weight that is bound as a convolution's)
        else add(sp.wname, {sp.N, sp.K}, sp.grad->dw);
        add(sp.bname, {sp.N}, sp.grad->db);
        sp.grad->n_pad = sp.t_n_pad;
        sp.grad->k_pad = sp.t_n_pad ? sp.k_pad : 0;
        sp.grad->t_plane = (long)sp.grad->n_pad * sp.grad->k_pad;
    }
}

extern "C" int dinoseg_create(const dinoseg_config* cfg, dinoseg_handle** out) {
    if (!cfg || !out) {
        dinoseg_set_error("dinoseg_create: null argument");
        return -1;
    }
    if (cfg->embed_dim % 128 != 0 || cfg->embed_dim > 1024 || cfg->num_heads * 64 != cfg->embed_dim ||
        (cfg->patch != 8 && cfg->patch != 16) ||
        cfg->n_blocks < 0 || cfg->n_classes < 1 || cfg->n_classes > HEAD_WIDE_MAX_C || cfg->mlp_ratio < 1 || cfg->pos_grid < 1 ||
        (cfg->precision != DINOSEG_BF16 && cfg->precision != DINOSEG_BF16X3 && cfg->precision != DINOSEG_FP16 &&
         cfg->precision != DINOSEG_FP16X3) ||
        (cfg->head_kind != DINOSEG_HEAD_MLP && cfg->head_kind != DINOSEG_HEAD_LINEAR)) {
        dinoseg_set_error("dinoseg_create: unsupported config (embed_dim=%d heads=%d mlp_ratio=%d patch=%d blocks=%d classes=%d; embed_dim must be "
                          "a multiple of 128 up to 1024 with heads = embed_dim / 64, mlp_ratio >= 1, patch 8 or 16, 1..%d classes)",
                          cfg->embed_dim, cfg->num_heads, cfg->mlp_ratio, cfg->patch, cfg->n_blocks, cfg->n_classes, HEAD_WIDE_MAX_C);
        return -1;
    }
    dinoseg_handle* h = new dinoseg_handle();
    h->cfg = *cfg;
    h->planes = (cfg->precision == DINOSEG_BF16X3 || cfg->precision == DINOSEG_FP16X3) ? 2 : 1;
    h->fmt = (cfg->precision == DINOSEG_FP16 || cfg->precision == DINOSEG_FP16X3) ? FMT_FP16 : FMT_BF16;
    index_params(h);
    *out = h;
    return 0;
}

// the inference workspaces and the split-forward stream / events (they live on the handle's device)
static void release_workspaces(dinoseg_handle* h) {
    if (h->ws) (void)hipFree(h->ws);
    if (h->ws2) (void)hipFree(h->ws2);
    if (h->aux_stream) {
        (void)hipStreamSynchronize(h->aux_stream);
        (void)hipStreamDestroy(h->aux_stream);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (auto& e : h->bw_ev) (void)hipEventDestroy(e);
    h->bw_ev.clear();
    h->ws = h->ws2 = nullptr;
    h->ws_bytes = h->ws2_bytes = 0;
    h->ws_B = h->ws_H = h->ws_W = h->ws2_B = h->ws2_H = h->ws2_W = -1;
    h->aux_stream = nullptr;
    h->ev_fork = h->ev_join = nullptr;
}

extern "C" int dinoseg_destroy(dinoseg_handle* h) {
    if (!h) return 0;
    DeviceGuard guard(h);
    if (h->wbuf) (void)hipFree(h->wbuf);
    if (h->pos_cache) (void)hipFree(h->pos_cache);
    release_workspaces(h);
    (void)dinoseg_train_release(h);
    for (auto& r : h->prof_recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto& e : h->prof_pool) (void)hipEventDestroy(e);
    for (auto& e : h->stage_ev) (void)hipEventDestroy(e);
    delete h;
    return 0;
}

// forget every packed copy (they point into wbuf): a refresh lays out only the copies its options ask for
static void clear_packs(dinoseg_handle* h) { h->model = ModelRec(); }

extern "C" int dinoseg_bind_weight(dinoseg_handle* h, const char* name, const void* dev_ptr, const int64_t* shape,
                                   int32_t ndim) {
    if (!h || !name || !dev_ptr || !shape) {
        dinoseg_set_error("dinoseg_bind_weight: null argument");
        return -1;
    }
    auto it = h->expected.find(name);
    if (it == h->expected.end()) {
        dinoseg_set_error("dinoseg_bind_weight: unexpected key '%s'", name);
        return -1;
    }
    const std::vector<int64_t>& want = it->second;
    bool ok = (int)want.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = want[i] == shape[i];
    if (!ok) {
        dinoseg_set_error("dinoseg_bind_weight: shape mismatch for '%s'", name);
        return -1;
    }
    {
        // the device that owns the parameters owns the handle: workspace, packed weights and every launch follow it
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, dev_ptr) != hipSuccess || attr.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            dinoseg_set_error("dinoseg_bind_weight: '%s' is not a device pointer", name);
            return -1;
        }
        if (h->device >= 0 && h->device != attr.device && !h->bound.empty() && h->bound.count(name) == 0) {
            dinoseg_set_error("dinoseg_bind_weight: '%s' lives on device %d, earlier tensors on device %d", name, attr.device, h->device);
            return -1;
        }
        if (h->device != attr.device) {
            if (h->device >= 0) {        // model.to(another device): everything the library allocated is on the old one
                DeviceGuard old(h);
                if (h->wbuf) (void)hipFree(h->wbuf);
                if (h->pos_cache) (void)hipFree(h->pos_cache);
                release_workspaces(h);
                (void)dinoseg_train_release(h);
                // events belong to the device they were created on: the gradient-stage and profiler events too
                for (auto& e : h->stage_ev) (void)hipEventDestroy(e);
                h->stage_ev.clear();
                h->stage_done = 0;
                for (auto& r : h->prof_recs) {
                    (void)hipEventDestroy(r.a);
                    (void)hipEventDestroy(r.b);
                }
                h->prof_recs.clear();
                for (auto& e : h->prof_pool) (void)hipEventDestroy(e);
                h->prof_pool.clear();
                h->wbuf = nullptr; h->pos_cache = nullptr; h->pos_hp = h->pos_wp = -1;
                h->wbuf_bytes = h->pos_cap = 0;
                h->tws_B = h->tws_H = h->tws_W = h->tr_B = -1;
                clear_packs(h);
                h->bound.clear();
                for (auto& kv : h->grad_index) kv.second->ptr = nullptr;
            }
            h->device = attr.device;
        }
    }
    BoundTensor t;
    t.ptr = reinterpret_cast<const float*>(dev_ptr);
    t.shape.assign(shape, shape + ndim);
    h->bound[name] = t;
    h->weights_ready = false;
    h->pos_stale = true;        // (dinoseg_refresh_weights resamples the cached resolution again)
    return 0;
}



// does gemm_rs.hip take this block linear (with the LayerNorm inside: ln)?  gemm_rs_supported on the shape and strides the forward
// fills in; the addresses are placeholders it never reads
static bool rs_shape_supported(const dinoseg_handle* h, const LinSpec& sp, bool ln) {
    static float placeholder[1];
    float* f = placeholder;
    bf16_t* b = reinterpret_cast<bf16_t*>(placeholder);
    GemmParams g = {};
    g.A = b; g.lda = sp.K; g.W = b;
    g.M = 1; g.N = sp.N; g.K = sp.K; g.planes = 1; g.fmt = sp.fmt; g.epi = sp.rs_bit == 1 ? EPI_GELU : sp.rs_bit == 2 ? EPI_QKV : EPI_RESID;
    g.bias = f;
    g.out_f32 = f; g.ldo_f32 = sp.N;        // attn.proj / mlp.fc2: the fp32 residual rows, N = embed_dim wide
    g.out_bf16 = b; g.ldo = sp.N;           // mlp.fc1: the hidden rows
    g.q = g.k = g.v = b; g.heads = h->cfg.num_heads; g.dmodel = h->cfg.embed_dim;
    if (ln) { g.ln_x = f; g.ln_eps = h->cfg.ln_eps; }
    return gemm_rs_supported(g);
}

// the fp32 parameters a fused launch of block b folds into its slot stream (mlp_fused3.hip / mlp_fused4.hip); next = the block
// whose LayerNorm1 + qkv are the tail of that launch (null behind the last block)
static MlpFused3Weights fused_block_weights(const BlockRec& b, const BlockRec* next) {
    MlpFused3Weights w = {};
    w.Wproj = b.proj.w; w.W1 = b.fc1.w; w.b1 = b.fc1.b; w.W2 = b.fc2.w;
    w.gamma2 = b.norm2_w; w.beta2 = b.norm2_b;
    if (next) {
        w.Wqkv_next = next->qkv.w; w.bqkv_next = next->qkv.b;
        w.gamma1_next = next->norm1_w; w.beta1_next = next->norm1_b;
    }
    return w;
}

// Packs every copy the records name (their pointers are set), in stream order: padded biases and slabs, the operand planes of all
// linears as one launch, the row-stationary copies, then the fused launches' streams.  Always here, with the refresh: a forward
// captured in a graph contains no pack kernels, so a deferred pack would let a replay after a fine-tune step read stale fused-kernel
// weights next to fresh ones.
static int pack_copies(dinoseg_handle* h, const std::vector<LinSpec>& specs, hipStream_t s) {
    const int Dm = h->cfg.embed_dim, Fh = h->cfg.embed_dim * h->cfg.mlp_ratio;
    std::vector<BlockRec>& blocks = h->model.blocks;
    std::vector<PackJob> jobs;
    for (const LinSpec& sp : specs) {
        const LinearRec& r = *sp.rec;
        if (!sp.pack) continue;
        jobs.push_back({r.w, r.pk.w, r.pk.plane, sp.N, sp.K, sp.n_pad, sp.k_pad, sp.planes, 0, sp.fmt});
        if (r.pk.bias_pad) {
            DSEG_CHECK_HIP(hipMemsetAsync(r.pk.bias_pad, 0, (size_t)sp.n_pad * sizeof(float), s));
            DSEG_CHECK_HIP(hipMemcpyAsync(r.pk.bias_pad, r.b, (size_t)sp.N * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        if (r.slab) DSEG_TRY(launch_pack_slabs(r.w, sp.N, sp.K, sp.planes, r.slab, s, sp.fmt));
    }
    DSEG_TRY(launch_multi_pack(jobs.data(), (int)jobs.size(), s));
    for (const LinSpec& sp : specs) {
        const LinearRec& r = *sp.rec;
        if (!r.rs) continue;
        if (r.rs_bias) {      // the copy carries the LayerNorm in front of the linear: norm1 for qkv, norm2 for fc1
            const BlockRec& k = blocks[sp.block];
            const bool qkv = sp.rs_bit == 2;
            DSEG_TRY(launch_pack_rs_ln(r.w, qkv ? k.norm1_w : k.norm2_w, qkv ? k.norm1_b : k.norm2_b, r.b, sp.N, sp.K, r.rs, r.rs_bias, s, sp.fmt));
        } else {
            DSEG_TRY(launch_pack_rs(r.w, sp.N, sp.K, sp.rs_bit == 4 ? 1 : 0, r.rs, s, sp.fmt));
        }
    }
    for (const BlockRec& k : blocks) {
        if (k.mlp) DSEG_TRY(launch_pack_mlp(k.fc1.w, k.fc2.w, Dm, Fh, k.mlp, s, h->fmt));
        if (k.projf) DSEG_TRY(launch_pack_proj(k.proj.w, Dm, k.projf, s, h->fmt));
        if (k.qkvf) DSEG_TRY(launch_pack_qkv(k.qkv.w, Dm, k.qkvf, s, h->fmt));
    }
    // (block i's stream ends with the qkv weight of block i + 1: the tail of its fused launch)
    for (size_t i = 0; i < blocks.size(); ++i) {
        const MlpFused3Weights w = fused_block_weights(blocks[i], i + 1 < blocks.size() ? &blocks[i + 1] : nullptr);
        if (blocks[i].mlp4) DSEG_TRY(launch_pack_mlp4(w, Dm, Fh, blocks[i].mlp4, s, h->fmt));
        if (blocks[i].mlp3) DSEG_TRY(launch_pack_mlp3(w, Dm, Fh, blocks[i].mlp3, s, h->fmt));
    }
    return 0;
}

extern "C" int dinoseg_refresh_weights(dinoseg_handle* h, void* stream) {
    if (!h) return -1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard(h);
    DSEG_TRY(check_stream_device(h, s));
    for (auto& kv : h->expected)
        if (!h->bound.count(kv.first)) {
            dinoseg_set_error("dinoseg_refresh_weights: missing key '%s' (strict load)", kv.first.c_str());
            return -3;
        }
    // the process-wide options that decide which copies exist are read ONCE per refresh: the packs below and every forward until the
    // next refresh use these values (a later dinoseg_set_option on a live handle takes effect with the next refresh, never between a
    // pack and its GEMM; mlp_fused4 and gemm_rs can also switch their route off in between: kernels.h Options)
    h->fp16_patch_planes_snap = options().fp16_patch_planes;
    h->mlp_fused4_snap = options().mlp_fused4;
    h->gemm_rs_snap = options().gemm_rs;
    h->gemm_rs_ln_snap = options().gemm_rs_ln;
    // every copy of the previous refresh is dropped: only those these options ask for are laid out again (a copy left over from
    // another layout would be re-packed over, or read from, whatever lives at its old offset now)
    h->weights_ready = false;
    ModelRec& m = h->model;
    m = ModelRec();
    m.blocks.resize(h->cfg.n_blocks);
    m.cls_token = W(h, "dino.cls_token");
    m.pos_embed = W(h, "dino.pos_embed");
    m.norm_w = W(h, "dino.norm.weight");
    m.norm_b = W(h, "dino.norm.bias");
    for (int i = 0; i < h->cfg.n_blocks; ++i) {
        const std::string b = block_prefix(i);
        m.blocks[i].norm1_w = W(h, b + "norm1.weight"); m.blocks[i].norm1_b = W(h, b + "norm1.bias");
        m.blocks[i].norm2_w = W(h, b + "norm2.weight"); m.blocks[i].norm2_b = W(h, b + "norm2.bias");
    }
    // ---- the plan: every copy of this refresh, in wbuf order -- what it is, how long it is, which record pointer it becomes.  Each
    // size and each "does this copy exist" is written here and nowhere else: the buffer's size and every offset follow from this list.
    struct Copy { std::string what; size_t bytes; void** slot; };
    std::vector<Copy> plan;
    auto copy16 = [&](const std::string& what, size_t elems, bf16_t*& slot) { plan.push_back({what, elems * sizeof(bf16_t), reinterpret_cast<void**>(&slot)}); };
    auto copy32 = [&](const std::string& what, size_t elems, float*& slot) { plan.push_back({what, elems * sizeof(float), reinterpret_cast<void**>(&slot)}); };
    const std::vector<LinSpec> specs = linear_specs(h, m);
    const int Dm = h->cfg.embed_dim, Fh = h->cfg.embed_dim * h->cfg.mlp_ratio;
    for (const LinSpec& sp : specs) {
        LinearRec& r = *sp.rec;
        r.w = W(h, sp.wname); r.b = W(h, sp.bname);
        r.N = sp.N; r.K = sp.K; r.planes = sp.planes; r.fmt = sp.fmt; r.rs_bit = sp.rs_bit;
        if (!sp.pack) continue;
        r.pk.plane = (long)sp.n_pad * sp.k_pad; r.pk.n_pad = sp.n_pad; r.pk.k_pad = sp.k_pad;
        copy16(sp.wname, (size_t)sp.planes * sp.n_pad * sp.k_pad, r.pk.w);
        if (sp.n_pad != sp.N) copy32("bias_pad " + sp.bname, sp.n_pad, r.pk.bias_pad);
        // qkv / fc1: also kept slab-major for the LayerNorm-fused kernel (the hi+lo one is bf16 only: gemm_ln.hip)
        if ((sp.rs_bit == 2 || sp.rs_bit == 1) && !(sp.planes == 2 && sp.fmt != FMT_BF16) &&
            gemm_ln_supported(sp.K, sp.N, sp.planes, sp.rs_bit == 2 ? EPI_QKV : EPI_GELU, Dm))
            copy16("slab " + sp.wname, (size_t)gemm_ln_slab_elems(sp.N, sp.K, sp.planes), r.slab);
    }
    // one-plane modes of the wide model: fragment-order copies of the four block linears for the row-stationary GEMMs (gemm_rs.hip),
    // for the linears whose gemm_rs bit is set and whose shape gemm_rs.hip takes.  qkv / fc1 with option gemm_rs_ln: the copy carries
    // the LayerNorm in front of the linear -- norm1 for qkv, norm2 for fc1 -- and a folded bias
    for (const LinSpec& sp : specs) {
        if (h->planes != 1 || Dm != 768 || !(h->gemm_rs_snap & sp.rs_bit)) continue;
        const bool ln = sp.rs_bit != 4 && h->gemm_rs_ln_snap;
        if (!rs_shape_supported(h, sp, ln)) continue;
        copy16("rs " + sp.wname, (size_t)sp.N * sp.K, sp.rec->rs);
        if (ln) copy32("rs_bias " + sp.wname, sp.N, sp.rec->rs_bias);
    }
    if (mlp_fused3_supported(Dm, Fh, h->planes))
        for (int i = 0; i < h->cfg.n_blocks; ++i) copy16("mlp3 " + block_prefix(i), (size_t)mlp_fused3_pack_elems(Dm, Fh), m.blocks[i].mlp3);
    if (h->mlp_fused4_snap && mlp_fused4_supported(Dm, Fh, h->planes))      // (a fine-tune step re-packs what exists)
        for (int i = 0; i < h->cfg.n_blocks; ++i) copy16("mlp4 " + block_prefix(i), (size_t)mlp_fused4_pack_elems(Dm, Fh), m.blocks[i].mlp4);
    if (mlp_fused_supported(Dm, Fh, h->planes)) {
        const long mlp_elems = mlp_fused_pack_elems(Dm, Fh), proj_elems = mlp_fused_proj_pack_elems(Dm), qkv_elems = mlp_fused_qkv_pack_elems(Dm);
        for (int i = 0; i < h->cfg.n_blocks; ++i) {
            const std::string b = block_prefix(i);
            copy16("mlp " + b, mlp_elems, m.blocks[i].mlp);
            if (proj_elems > 0) copy16("proj " + b, proj_elems, m.blocks[i].projf);
            if (i > 0 && qkv_elems > 0) copy16("qkvf " + b, qkv_elems, m.blocks[i].qkvf);      // (block 0's qkv has no fused kernel in front of it)
        }
    }
    // ---- the buffer: each copy 256-byte aligned, in plan order
    std::vector<dinoseg_handle::WbufEntry> layout;
    size_t total = 0;
    for (const Copy& cp : plan) {
        layout.push_back({cp.what, total, cp.bytes});
        total += align_up(cp.bytes, 256);
    }
    if (total > h->wbuf_bytes) {
        ++h->generation;
        if (h->wbuf) DSEG_CHECK_HIP(hipFree(h->wbuf));
        h->wbuf = nullptr;
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->wbuf), total));
        h->wbuf_bytes = total;
    }
    for (size_t i = 0; i < plan.size(); ++i) *plan[i].slot = h->wbuf + layout[i].off;
    // a captured forward bakes in the address and the format of every copy it reads: another layout in the same buffer (a copy
    // that changed size, appeared or left) is a new state generation, like a new buffer; the same layout is not (an in-place weight
    // update replays the captured forward, which reads the re-packed copies)
    if (layout != h->wbuf_layout) ++h->generation;
    h->wbuf_layout = std::move(layout);
    DSEG_TRY(pack_copies(h, specs, s));
    h->weights_ready = true;
    // pos_embed may have changed in place (load_state_dict into the same storage, an optimizer step on an unfrozen backbone).  A
    // captured forward contains no resample launch and never calls dinoseg_prepare_resolution, so "resample on the next forward"
    // (pos_hp = -1 alone) would let a replay read the OLD rows next to freshly packed linears: resample here, in stream order with
    // the packs, into the SAME buffer: like the re-packed linears, the captured pointers stay valid and the replay reads new rows.
    if (h->pos_hp > 0 && h->pos_cache != nullptr) {
        DSEG_TRY(launch_pos_resample(m.pos_embed, h->cfg.pos_grid, h->cfg.embed_dim, h->pos_hp, h->pos_wp, h->pos_cache, s));
    } else {
        h->pos_hp = h->pos_wp = -1;      // (nothing cached: the next forward resamples, and dinoseg_prepare_resolution counts a new generation)
    }
    h->pos_stale = false;
    return 0;
}


extern "C" int dinoseg_prepare_resolution_hw(dinoseg_handle* h, int32_t Hf, int32_t Wf, void* stream) {
    if (!h) return -1;
    if (!frame_ok(Hf, Wf, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    if (!h->bound.count("dino.pos_embed")) {
        dinoseg_set_error("dinoseg_prepare_resolution: dino.pos_embed not bound");
        return -3;
    }
    const int hp = Hf / h->cfg.patch, wp = Wf / h->cfg.patch, D = h->cfg.embed_dim;
    if (h->pos_hp == hp && h->pos_wp == wp && !h->pos_stale) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard guard(h);
    ++h->generation;        // (the cache holds ONE patch grid: a captured forward of another one would read this one's rows)
    const size_t need = ((size_t)hp * wp + 1) * D * sizeof(float);
    if (need > h->pos_cap) {
        if (h->pos_cache) DSEG_CHECK_HIP(hipFree(h->pos_cache));
        h->pos_cache = nullptr;
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&h->pos_cache), need));
        h->pos_cap = need;
    }
    DSEG_TRY(launch_pos_resample(W(h, "dino.pos_embed"), h->cfg.pos_grid, D, hp, wp, h->pos_cache, s));
    h->pos_hp = hp;
    h->pos_wp = wp;
    h->pos_stale = false;
    return 0;
}

extern "C" int dinoseg_prepare_resolution(dinoseg_handle* h, int32_t r, void* stream) {
    return dinoseg_prepare_resolution_hw(h, r, r, stream);
}

// ------------------------------------------------------------------------------------------------ workspace
WsLayout make_layout(const dinoseg_handle* h, int B, int Hf, int Wf) {
    const dinoseg_config& c = h->cfg;
    const int D = c.embed_dim, F = D * c.mlp_ratio, P = h->planes, HP = head_planes();
    WsLayout L;
    L.n = (Hf / c.patch) * (Wf / c.patch);
    L.ntok = L.n + 1;
    L.npad = (L.ntok + 63) / 64 * 64;
    L.M = B * L.ntok;
    L.Mp = B * L.n;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    L.X = take((size_t)L.M * D * 4);
    L.a_plane = (long)L.M * D;                 // LN output; also hosts the patch-gather matrix: patch_planes x [Mp, 3 p^2]
    {
        const size_t ln_bytes = (size_t)P * L.a_plane * 2, pg_bytes = (size_t)patch_planes(h) * L.Mp * (3 * c.patch * c.patch) * 2;
        L.A = take(ln_bytes > pg_bytes ? ln_bytes : pg_bytes);
    }
    L.qkv_plane = (long)B * c.num_heads * L.npad * 64;
    L.Q = take((size_t)P * L.qkv_plane * 2);
    L.K = take((size_t)P * L.qkv_plane * 2);
    L.V = take((size_t)P * L.qkv_plane * 2);
    L.ctx_plane = (long)L.M * D;
    L.CTX = take((size_t)P * L.ctx_plane * 2);
    L.hb_plane = (long)L.M * F;
    {   // HB also hosts the log-probabilities when the caller asks for the argmax only (dinoseg_forward with logp_out == nullptr)
        const size_t hb_bytes = (size_t)P * L.hb_plane * 2, lp_bytes = (size_t)L.Mp * c.n_classes * 4;
        L.HB = take(hb_bytes > lp_bytes ? hb_bytes : lp_bytes);
    }
    L.feat_plane = (long)L.Mp * D;
    L.FEAT = take((size_t)HP * L.feat_plane * 2);
    L.h1_plane = (long)L.Mp * HEAD_H1_PAD;
    L.H1 = take((size_t)HP * L.h1_plane * 2);
    L.h2_plane = (long)L.Mp * HEAD_H2_PAD;
    L.H2 = take((size_t)HP * L.h2_plane * 2);
    L.total = off;
    return L;
}

extern "C" int64_t dinoseg_state_generation(const dinoseg_handle* h) { return h ? h->generation : -1; }

extern "C" int64_t dinoseg_workspace_bytes_hw(const dinoseg_handle* h, int32_t B, int32_t H, int32_t W) {
    if (!h || B <= 0) return -1;
    if (!frame_ok(H, W, h->cfg.patch)) {
        set_resolution_error(h->cfg.patch);
        return -1;
    }
    return (int64_t)(make_layout(h, B, H, W).total + h->wbuf_bytes);
}

extern "C" int64_t dinoseg_workspace_bytes(const dinoseg_handle* h, int32_t B, int32_t r) {
    return dinoseg_workspace_bytes_hw(h, B, r, r);
}

int ensure_workspace(dinoseg_handle* h, int slot, const WsLayout& L, int B, int Hf, int Wf, hipStream_t s) {
    char*& ws = slot ? h->ws2 : h->ws;
    size_t& bytes = slot ? h->ws2_bytes : h->ws_bytes;
    int& wB = slot ? h->ws2_B : h->ws_B;
    int& wH = slot ? h->ws2_H : h->ws_H;
    int& wW = slot ? h->ws2_W : h->ws_W;
    if (L.total > bytes) {
        ++h->generation;
        if (ws) {
            DSEG_CHECK_HIP(hipStreamSynchronize(s));
            DSEG_CHECK_HIP(hipFree(ws));
        }
        ws = nullptr;
        bytes = 0;
        DSEG_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&ws), L.total));
        bytes = L.total;
        wB = -1;
    }
    if (wB != B || wH != Hf || wW != Wf) {
        // pad rows (include/dinoseg.h, dinoseg_op_attention): rows ntok..npad of q, k and v are read with the 64-row tiles they share with
        // real rows and must hold FINITE values -- any finite values, zero is not required (a pad key gets probability 0, 0 x finite = 0;
        // 0 x Inf is not).  Fresh memory may hold anything: zero Q/K/V once per layout (never written afterwards).  A layout change is a
        // new state generation: a forward captured under the OLD layout holds no memset node, and another layout's launches have since
        // written other things (fp32 residual rows ...) where its pad rows live -- the owner of the graph must capture again.
        DSEG_CHECK_HIP(hipMemsetAsync(ws + L.Q, 0, L.CTX - L.Q, s));
        ++h->generation;
        wB = B;
        wH = Hf;
        wW = Wf;
    }
    return 0;
}

int ensure_aux_stream(dinoseg_handle* h) {
    if (!h->aux_stream) {
        DSEG_CHECK_HIP(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
        DSEG_CHECK_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        DSEG_CHECK_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    return 0;
}

extern "C" int dinoseg_op_resize_u8(const uint8_t* src, int32_t sh, int32_t sw, uint8_t* dst, int32_t dh, int32_t dw, void* stream) {
    if (!src || !dst) {
        dinoseg_set_error("dinoseg_op_resize_u8: null pointer");
        return -1;
    }
    return launch_resize_u8(src, sh, sw, dst, dh, dw, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_upsample_argmax(const float* logp, int32_t B, int32_t hp, int32_t wp, int32_t C, int32_t OH, int32_t OW,
                                          int32_t* labels_out, float* dense_out, void* stream) {
    return launch_upsample_argmax(logp, B, hp, wp, C, OH, OW, labels_out, dense_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_guide_cells(const uint8_t* guide, int32_t B, int32_t OH, int32_t OW, int32_t hp, int32_t wp, uint32_t* cells,
                                      void* stream) {
    return launch_guide_cells("dinoseg_op_guide_cells", guide, B, OH, OW, hp, wp, cells, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_upsample_guided(const float* logp, const uint8_t* guide, const uint32_t* cells, int32_t B, int32_t hp, int32_t wp,
                                          int32_t C, int32_t OH, int32_t OW, int32_t radius, double sigma_spatial, double sigma_range,
                                          int32_t* labels_out, float* dense_out, void* stream) {
    return launch_upsample_guided("dinoseg_op_upsample_guided", logp, guide, cells, B, hp, wp, C, OH, OW, radius, sigma_spatial, sigma_range,
                                  labels_out, dense_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_refine_scratch_bytes(int32_t B, int32_t C, int32_t OH, int32_t OW) { return refine_scratch_bytes(B, C, OH, OW); }

extern "C" int dinoseg_op_refine_seed(const void* seed, int32_t kind, int32_t B, int32_t C, int32_t OH, int32_t OW, int32_t hp, int32_t wp,
                                      double gain, void* scratch, void* stream) {
    return launch_refine_seed("dinoseg_op_refine_seed", seed, kind, B, C, OH, OW, hp, wp, gain, scratch, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_refine_iterate(const uint8_t* guide, void* scratch, int32_t B, int32_t C, int32_t OH, int32_t OW,
                                         const int32_t* dilations, int32_t n_dil, double sigma, int32_t iters, int32_t* labels_out,
                                         float* dense_out, void* stream) {
    return launch_refine_iterate("dinoseg_op_refine_iterate", guide, scratch, B, C, OH, OW, dilations, n_dil, sigma, iters, labels_out,
                                 dense_out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_upsample_ensemble_scratch_bytes(int32_t K, int32_t B, int32_t OH, int32_t OW) {
    return upsample_ensemble_scratch_bytes(K, B, OH, OW);
}

extern "C" int dinoseg_op_upsample_ensemble(const float* const* logp, const int32_t* hp, const int32_t* wp, const int32_t* flip, int32_t K,
                                            int32_t B, int32_t C, int32_t OH, int32_t OW, int32_t* labels_out, float* conf_out,
                                            float* probs_out, void* scratch, void* stream) {
    if (K < 1 || K > UPE_MAX_VIEWS) {
        dinoseg_set_error("dinoseg_op_upsample_ensemble: %d views (1 <= K <= %d)", K, UPE_MAX_VIEWS);
        return -1;
    }
    if (!logp || !hp || !wp || !flip) {
        dinoseg_set_error("dinoseg_op_upsample_ensemble: null view table (logp, hp, wp and flip are host arrays of K entries)");
        return -1;
    }
    UpEnsViews views = {};
    for (int k = 0; k < K; ++k) views.v[k] = {logp[k], hp[k], wp[k], flip[k], 0};
    return launch_upsample_ensemble(views, K, B, C, OH, OW, labels_out, conf_out, probs_out, scratch, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_window_origins(int32_t L, int32_t win, int32_t stride, int32_t* out, int32_t cap) {
    return window_origins(L, win, stride, out, cap);
}

extern "C" int dinoseg_op_crop_windows(const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t win_h, int32_t win_w,
                                       int32_t stride_h, int32_t stride_w, int32_t first, int32_t count, void* out, void* stream) {
    return launch_crop_windows(x, x_kind, B, H, W, win_h, win_w, stride_h, stride_w, first, count, out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_window_merge(const float* logp, int32_t B, int32_t H, int32_t W, int32_t patch, int32_t win_h, int32_t win_w,
                                       int32_t stride_h, int32_t stride_w, int32_t C, int32_t* labels_out, float* dense_out, void* stream) {
    return launch_window_merge(logp, B, H, W, patch, win_h, win_w, stride_h, stride_w, C, labels_out, dense_out,
                               reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_augment(const uint8_t* frames, const void* masks, int32_t mask_kind, int32_t B, int32_t H, int32_t W,
                                  const dinoseg_augment_frame* table, int32_t max_radius, int32_t OH, int32_t OW, int32_t out_kind, void* out,
                                  int64_t* pixel_labels, int64_t* patch_labels, int32_t patch, float* scratch, void* stream) {
    return launch_augment(frames, masks, mask_kind, B, H, W, table, max_radius, OH, OW, out_kind, out, pixel_labels, patch_labels, patch,
                          scratch, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_normalize_tokens(const float* tokens, int32_t B, int32_t n, int32_t D, void* planes, void* stream) {
    return launch_normalize_tokens(tokens, B, n, D, planes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_label_cells(const void* labels, int32_t mask_kind, int32_t OH, int32_t OW, int32_t hp, int32_t wp, int32_t C,
                                      float* seg, void* stream) {
    return launch_label_cells(labels, mask_kind, OH, OW, hp, wp, C, seg, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_propagate_scratch_bytes(int32_t hp, int32_t wp, int32_t n_ctx, int32_t k) {
    return propagate_scratch_bytes(hp, wp, n_ctx, k);
}

extern "C" int dinoseg_op_propagate(const void* target_planes, const void* const* ctx_planes, const float* const* ctx_segs, int32_t n_ctx,
                                    int32_t hp, int32_t wp, int32_t D, int32_t C, int32_t radius, int32_t k, double tau, float* seg_out,
                                    int32_t* topk_idx, float* topk_w, void* scratch, void* stream) {
    return launch_propagate(target_planes, ctx_planes, ctx_segs, n_ctx, hp, wp, D, C, radius, k, tau, seg_out, topk_idx, topk_w, scratch,
                            reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_knn_scratch_bytes(int32_t N, int32_t M, int32_t k, int32_t splits) { return knn_scratch_bytes(N, M, k, splits); }

extern "C" int32_t dinoseg_knn_splits(int32_t N, int32_t M, int32_t k) { return knn_splits(N, M, k); }

extern "C" int dinoseg_op_knn_labels(const void* query_planes, int32_t B, int32_t n, const void* bank_planes, int64_t M, int64_t bank_rows,
                                     const void* bank_labels, int32_t label_kind, int32_t D, int32_t C, int32_t k, double tau,
                                     int32_t splits, float* seg_out, int32_t* topk_idx, float* topk_w, void* scratch, void* stream) {
    return launch_knn_labels(query_planes, B, n, bank_planes, M, bank_rows, bank_labels, label_kind, D, C, k, tau, splits, seg_out,
                             topk_idx, topk_w, scratch, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_pca_scratch_bytes(int32_t B, int32_t n, int32_t D) { return pca_scratch_bytes(B, n, D); }

extern "C" int32_t dinoseg_pca_ranges(int64_t rows, int32_t D) {
    return rows >= 1 && rows <= (1ll << 31) - 256 && D >= 64 && D <= 1024 && D % 64 == 0 ? pca_ranges(rows, D) : -1;
}

extern "C" int dinoseg_op_token_moments(const float* tokens, const uint8_t* keep, int32_t B, int32_t n, int32_t D, const float* shift,
                                        double* sum, double* outer, int64_t* count, void* scratch, void* stream) {
    return launch_token_moments(tokens, keep, B, n, D, shift, sum, outer, reinterpret_cast<long long*>(count), scratch,
                                reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_pca_project(const float* tokens, int32_t B, int32_t n, int32_t D, const float* mean, const float* basis,
                                      const float* scale, int32_t q, float* out, void* stream) {
    return launch_pca_project(tokens, B, n, D, mean, basis, scale, q, out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_pca_colour(const float* comps, int32_t B, int32_t hp, int32_t wp, int32_t q, const float* lo, const float* inv,
                                     const uint8_t* keep, int32_t OH, int32_t OW, uint8_t* rgb, void* stream) {
    return launch_pca_colour(comps, B, hp, wp, q, lo, inv, keep, OH, OW, rgb, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_kmeans_scratch_bytes(int32_t B, int32_t n, int32_t K, int32_t D) { return kmeans_scratch_bytes(B, n, K, D); }

extern "C" int dinoseg_op_kmeans_init(const float* rows, int32_t K, int32_t D, int32_t normalize, float* centroids, void* planes,
                                      void* stream) {
    return launch_kmeans_init(rows, K, D, normalize, centroids, planes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_kmeans_assign(const void* points, int32_t B, int32_t n, const void* centroid_planes, int32_t K, int32_t D,
                                        const int32_t* prev_assign, int32_t* assign, float* best, float* scores, float* objective,
                                        int32_t* moved, void* scratch, void* stream) {
    return launch_kmeans_assign(points, B, n, centroid_planes, K, D, prev_assign, assign, best, scores, objective, moved, scratch,
                                reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_kmeans_update(const void* points, int32_t B, int32_t n, const int32_t* assign, const float* prev_centroids,
                                        const void* prev_planes, int32_t K, int32_t D, float* centroids, void* planes, int32_t* counts,
                                        void* scratch, void* stream) {
    return launch_kmeans_update(points, B, n, assign, prev_centroids, prev_planes, K, D, centroids, planes, counts, scratch,
                                reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_ncut_graph_bytes(int32_t B, int32_t n) { return ncut_graph_bytes(B, n); }

extern "C" int32_t dinoseg_ncut_max_cells(void) { return ncut_max_cells(); }

extern "C" int dinoseg_op_ncut_graph(const void* planes, int32_t B, int32_t n, int32_t D, double tau, void* graph, int32_t* degree,
                                     void* stream) {
    return launch_ncut_graph(planes, B, n, D, tau, graph, degree, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_ncut_iterate(const void* graph, const int32_t* degree, int32_t B, int32_t n, double eps, const float* z_in,
                                       int32_t iters, float* z_out, float* rho, uint8_t* fg, float* eigvec, float* margin,
                                       int32_t* seed_cell, void* stream) {
    return launch_ncut_iterate(graph, degree, B, n, eps, z_in, iters, z_out, rho, fg, eigvec, margin, seed_cell,
                               reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t dinoseg_ncut_split_max_cells(void) { return ncut_split_max_cells(); }

extern "C" int64_t dinoseg_ncut_split_graph_bytes(int32_t B, int32_t n) { return ncut_split_graph_bytes(B, n); }

extern "C" int64_t dinoseg_ncut_split_scratch_bytes(int32_t B, int32_t n) { return ncut_split_scratch_bytes(B, n); }

extern "C" int dinoseg_op_ncut_graph_split(const void* planes, int32_t B, int32_t n, int32_t D, double tau, void* graph, int32_t* degree,
                                           void* stream) {
    return launch_ncut_graph_split(planes, B, n, D, tau, graph, degree, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_ncut_iterate_split(const void* graph, const int32_t* degree, int32_t B, int32_t n, double eps, const float* z_in,
                                             int32_t iters, int32_t rows_per_group, float* z_out, float* rho, uint8_t* fg, float* eigvec,
                                             float* margin, int32_t* seed_cell, void* scratch, void* stream) {
    return launch_ncut_iterate_split(graph, degree, B, n, eps, z_in, iters, rows_per_group, z_out, rho, fg, eigvec, margin, seed_cell,
                                     scratch, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_components_scratch_bytes(int32_t B, int32_t H, int32_t W) { return components_scratch_bytes(B, H, W); }

extern "C" int dinoseg_op_components(const int32_t* labels, int32_t B, int32_t H, int32_t W, int32_t connectivity, int32_t ignore,
                                     int32_t max_objects, int32_t* ids, int32_t* count, int32_t* first, int32_t* label, int32_t* area,
                                     int32_t* box, int32_t* status, void* scratch, void* stream) {
    return launch_components(labels, B, H, W, connectivity, ignore, max_objects, ids, count, first, label, area, box, status, scratch,
                             reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_maskcut_scratch_bytes(int32_t B, int32_t hp, int32_t wp, int32_t K) { return maskcut_scratch_bytes(B, hp, wp, K); }

extern "C" int dinoseg_op_ncut_mask(void* graph, int32_t* degree, const void* alive, int32_t B, int32_t n, void* stream) {
    return launch_ncut_mask(graph, degree, alive, B, n, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_maskcut_select(const int32_t* ids, const uint8_t* fg, const float* margin, const int32_t* seed_cell, void* alive,
                                         int32_t B, int32_t hp, int32_t wp, int32_t K, int32_t t, uint8_t* cells, uint8_t* found,
                                         int32_t* area, int32_t* box, float* score, void* stream) {
    return launch_maskcut_select(ids, fg, margin, seed_cell, alive, B, hp, wp, K, t, cells, found, area, box, score,
                                 reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_maskcut(void* graph, int32_t* degree, int32_t B, int32_t hp, int32_t wp, double eps, const float* z_start,
                                  int32_t iters, int32_t rows_per_group, int32_t connectivity, int32_t K, uint8_t* cells, uint8_t* found,
                                  int32_t* area, int32_t* box, float* score, int32_t* count, uint8_t* fg, float* margin, float* eigvec,
                                  int32_t* seed_cell, float* rho, void* scratch, void* stream) {
    return launch_maskcut(graph, degree, B, hp, wp, eps, z_start, iters, rows_per_group, connectivity, K, cells, found, area, box, score,
                          count, fg, margin, eigvec, seed_cell, rho, scratch, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_confusion(const int32_t* pred, const int64_t* gt, int64_t n, int32_t n_classes, int64_t* cm, void* stream) {
    return launch_confusion(pred, gt, n, n_classes, cm, reinterpret_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ options
namespace dseg {
Options& options() {
    static Options o;
    return o;
}
}  // namespace dseg

// what dinoseg_set_option stores for a value: *out, or -1 with the error set
static int opt_value(int32_t v, int* out) { *out = v; return 0; }
static int opt_flag(int32_t v, int* out) { *out = v ? 1 : 0; return 0; }
static int opt_bits3(int32_t v, int* out) { *out = v & 7; return 0; }
static int opt_min2(int32_t v, int* out) { *out = v < 2 ? 2 : v; return 0; }
static int opt_1_or_2(int32_t v, int* out) { *out = v == 1 ? 1 : 2; return 0; }
static int opt_fmt(int32_t v, int* out) {
    if (v != FMT_BF16 && v != FMT_FP16) {
        dinoseg_set_error("dinoseg_set_option: op_fmt must be 0 (bf16) or 1 (fp16)");
        return -1;
    }
    *out = v;
    return 0;
}
// every key of dinoseg_set_option: the member of Options it writes (kernels.h: what each one does) and how the value is normalised
static const struct OptionRow {
    const char* name;
    int Options::*member;       // null: accepted and ignored
    int (*normalise)(int32_t, int*);
} OPTION_TABLE[] = {
    {"gemm_ln", &Options::gemm_ln, opt_value},
    {"gemm_big", &Options::gemm_big, opt_value},
    {"route_ab", &Options::route_ab, opt_value},
    {"fp16_patch_planes", &Options::fp16_patch_planes, opt_1_or_2},
    {"op_v_bf16", &Options::op_v_bf16, opt_flag},        // dinoseg_op_attention with fp16 hi + lo planes: V is given as bf16 hi + lo planes (AttnParams::v_bf16)
    {"op_fmt", &Options::op_fmt, opt_fmt},               // operand format of the single-plane stand-alone ops (dinoseg_op_*): 0 bf16, 1 fp16
    {"streams", &Options::streams, opt_value},
    {"mlp_fused", &Options::mlp_fused, opt_value},
    {"qkv_fused", &Options::qkv_fused, opt_value},
    {"proj_fused", &Options::proj_fused, opt_value},
    {"mlp_stagger", &Options::mlp_stagger, opt_value},
    {"mlp_grid", &Options::mlp_grid, opt_value},
    {"splitk_tiles", &Options::splitk_tiles, opt_value},
    {"deterministic", &Options::deterministic, opt_flag},    // the fine-tune step's reductions in a fixed order (kernels.h Options::deterministic)
    {"train_streams", &Options::train_streams, opt_value},
    {"mlp_variant", nullptr, opt_value},                 // (accepted and ignored: the one-wave-per-SIMD build was removed in round 4)
    {"gemm_rs", &Options::gemm_rs, opt_bits3},
    {"gemm_rs_ln", &Options::gemm_rs_ln, opt_flag},
    {"gemm_rs_min_rows", &Options::gemm_rs_min_rows, opt_value},
    {"qkv_fused3", &Options::qkv_fused3, opt_flag},
    {"qkv_fused4", &Options::qkv_fused4, opt_flag},
    {"mlp_fused4", &Options::mlp_fused4, opt_flag},
    {"mlp_fused3_min_rows", &Options::mlp_fused3_min_rows, opt_value},
    {"mlp_fused_min_rows", &Options::mlp_fused_min_rows, opt_value},
    {"split_min", &Options::split_min, opt_min2},
    {"gemm_dbg", &Options::gemm_dbg, opt_value},
    {"attn_variant", &Options::attn_variant, opt_value},
    {"attn_dbg", &Options::attn_dbg, opt_value},
};

extern "C" int dinoseg_set_option(const char* key, int32_t value) {
    if (!key) return -1;
    for (const OptionRow& row : OPTION_TABLE) {
        if (strcmp(key, row.name) != 0) continue;
        int v = 0;
        DSEG_TRY(row.normalise(value, &v));
        if (row.member) dseg::options().*row.member = v;
        return 0;
    }
    dinoseg_set_error("dinoseg_set_option: unknown key '%s'", key);
    return -1;
}

extern "C" int dinoseg_get_option(const char* key, int32_t* value) {
    if (!key || !value) {
        dinoseg_set_error("dinoseg_get_option: null argument");
        return -1;
    }
    for (const OptionRow& row : OPTION_TABLE) {
        if (strcmp(key, row.name) != 0) continue;
        *value = row.member ? dseg::options().*row.member : 0;
        return 0;
    }
    dinoseg_set_error("dinoseg_get_option: unknown key '%s'", key);
    return -1;
}

extern "C" const char* dinoseg_option_name(int32_t index) {
    const int32_t n = (int32_t)(sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0]));
    return index >= 0 && index < n ? OPTION_TABLE[index].name : nullptr;
}

// ------------------------------------------------------------------------------------------------ profiling
extern "C" int dinoseg_profile(dinoseg_handle* h, int32_t level) {
    if (!h || level < 0 || level > 2) {
        dinoseg_set_error("dinoseg_profile: level must be 0, 1 or 2");
        return -1;
    }
    for (auto& r : h->prof_recs) {
        h->prof_pool.push_back(r.a);
        h->prof_pool.push_back(r.b);
    }
    h->prof_recs.clear();
    h->prof_level = level;
    return 0;
}

extern "C" int dinoseg_profile_read(dinoseg_handle* h, float* ms_sum, int32_t* counts) {
    if (!h || !ms_sum || !counts) {
        dinoseg_set_error("dinoseg_profile_read: null argument");
        return -1;
    }
    for (int c = 0; c < DINOSEG_PROF_COUNT; ++c) {
        ms_sum[c] = 0.f;
        counts[c] = 0;
    }
    for (auto& r : h->prof_recs) {
        DSEG_CHECK_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        DSEG_CHECK_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        ms_sum[r.cat] += ms;
        counts[r.cat] += 1;
        h->prof_pool.push_back(r.a);
        h->prof_pool.push_back(r.b);
    }
    h->prof_recs.clear();
    return 0;
}

// ------------------------------------------------------------------------------------------------ stand-alone ops
extern "C" int dinoseg_op_pack(const float* src, int32_t rows, int32_t cols, void* dst, int64_t plane_stride,
                               int32_t rows_pad, int32_t cols_pad, int32_t planes, void* stream) {
    return launch_pack_planes(src, rows, cols, reinterpret_cast<bf16_t*>(dst), plane_stride, rows_pad, cols_pad, planes,
                              reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_gemm(const void* A, int64_t a_plane, int32_t lda, const void* Wp, int64_t w_plane, int32_t M,
                               int32_t N, int32_t K, int32_t planes, int32_t epi, const float* bias, float* out_f32,
                               void* out_bf16, int64_t out_plane, int32_t ldo, void* stream) {
    if (epi < EPI_PLAIN || epi > EPI_RELU) {
        dinoseg_set_error("dinoseg_op_gemm: epi must be 0..3");
        return -1;
    }
    GemmParams g = {};
    g.A = reinterpret_cast<const bf16_t*>(A); g.a_plane = a_plane; g.lda = lda;
    g.W = reinterpret_cast<const bf16_t*>(Wp); g.w_plane = w_plane;
    g.M = M; g.N = N; g.K = K; g.planes = planes; g.epi = epi; g.bias = bias;
    g.fmt = options().op_fmt;
    g.out_f32 = out_f32; g.ldo_f32 = N;
    g.out_bf16 = reinterpret_cast<bf16_t*>(out_bf16); g.out_plane = out_plane; g.ldo = ldo;
    return launch_gemm(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_qkv_gemm(const void* A, int64_t a_plane, const void* Wp, int64_t w_plane, const float* bias,
                                   int32_t B, int32_t ntok, int32_t npad, int32_t heads, int32_t planes, float qscale,
                                   void* q, void* k, void* v, int64_t qkv_plane, void* stream) {
    GemmParams g = {};
    const int D = heads * 64;
    g.A = reinterpret_cast<const bf16_t*>(A); g.a_plane = a_plane; g.lda = D;
    g.W = reinterpret_cast<const bf16_t*>(Wp); g.w_plane = w_plane;
    g.M = B * ntok; g.N = 3 * D; g.K = D; g.planes = planes; g.epi = EPI_QKV; g.bias = bias;
    g.fmt = options().op_fmt;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v);
    g.qkv_plane = qkv_plane; g.ntok = ntok; g.npad = npad; g.heads = heads; g.dmodel = D; g.qscale = qscale;
    g.v_bf16 = options().op_v_bf16;
    return launch_gemm(g, reinterpret_cast<hipStream_t>(stream));
}

// the shape rules of launch_gemm_small (gemm.hip), for the entries below that name their own refusals
static bool gemm_small_shape_ok(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t planes) {
    return M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 64 == 0 && lda >= K && lda % 8 == 0 && (planes == 1 || planes == 2);
}

extern "C" int dinoseg_op_patch_gemm(const void* A, const void* Wp, const float* bias, const float* pos, int32_t B, int32_t n_patches,
                                     int32_t N, int32_t K, int32_t planes, float* X_out, void* stream) {
    if (!A || !Wp || !bias || !pos || !X_out) {
        dinoseg_set_error("dinoseg_op_patch_gemm: null pointer");
        return -1;
    }
    if (B <= 0 || n_patches <= 0 || (int64_t)B * n_patches > INT32_MAX || !gemm_small_shape_ok(B * n_patches, N, K, K, planes)) {
        dinoseg_set_error("dinoseg_op_patch_gemm: unsupported shape B=%d n_patches=%d N=%d K=%d planes=%d (need N%%128==0, K%%64==0)", B, n_patches,
                          N, K, planes);
        return -1;
    }
    GemmParams g = {};
    g.A = reinterpret_cast<const bf16_t*>(A); g.a_plane = (long)B * n_patches * K; g.lda = K;
    g.W = reinterpret_cast<const bf16_t*>(Wp); g.w_plane = (long)N * K;
    g.M = B * n_patches; g.N = N; g.K = K; g.planes = planes; g.epi = EPI_PATCH; g.bias = bias;
    g.fmt = options().op_fmt;
    g.out_f32 = X_out; g.ldo_f32 = N;
    g.pos = pos; g.n_patches = n_patches;
    return launch_gemm(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_gemm_train(const void* A, int64_t a_plane, int32_t lda, const void* Wp, int64_t w_plane, int32_t M, int32_t N,
                                     int32_t K, int32_t planes, int32_t epi, const float* bias, const float* resid, float* out_f32,
                                     void* out_bf16, int64_t out_plane, int32_t ldo, void* aux_out, int64_t aux_plane, void* stream) {
    if (epi != EPI_RESID && epi != EPI_GELU) {
        dinoseg_set_error("dinoseg_op_gemm_train: epi must be 1 (residual) or 2 (GELU)");
        return -1;
    }
    if (!A || !Wp || (epi == EPI_RESID && (!resid || !out_f32 || resid == out_f32)) || (epi == EPI_GELU && (!out_bf16 || !aux_out))) {
        dinoseg_set_error("dinoseg_op_gemm_train: epi 1 needs resid and out_f32 (two buffers), epi 2 needs out_bf16 and aux_out");
        return -1;
    }
    if (!gemm_small_shape_ok(M, N, K, lda, planes) || (epi == EPI_GELU && (ldo < N || ldo % 8 != 0))) {
        dinoseg_set_error("dinoseg_op_gemm_train: unsupported shape M=%d N=%d K=%d lda=%d ldo=%d planes=%d (need N%%128==0, K%%64==0)", M, N, K, lda,
                          ldo, planes);
        return -1;
    }
    if (epi == EPI_GELU && options().op_fmt != FMT_BF16) {
        dinoseg_set_error("dinoseg_op_gemm_train: the pre-activation planes (aux_out) are bf16 only");
        return -1;
    }
    GemmParams g = {};
    g.A = reinterpret_cast<const bf16_t*>(A); g.a_plane = a_plane; g.lda = lda;
    g.W = reinterpret_cast<const bf16_t*>(Wp); g.w_plane = w_plane;
    g.M = M; g.N = N; g.K = K; g.planes = planes; g.epi = epi; g.bias = bias;
    g.fmt = options().op_fmt;
    if (epi == EPI_RESID) {
        g.resid = resid; g.out_f32 = out_f32; g.ldo_f32 = N;
    } else {
        g.out_bf16 = reinterpret_cast<bf16_t*>(out_bf16); g.out_plane = out_plane; g.ldo = ldo;
        g.aux_out = reinterpret_cast<bf16_t*>(aux_out); g.aux_plane = aux_plane;
    }
    return launch_gemm(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_mlp_fused_pack_elems(int32_t D, int32_t F) { return mlp_fused_pack_elems(D, F); }

extern "C" int dinoseg_op_pack_mlp(const float* W1, const float* W2, int32_t D, int32_t F, void* dst, void* stream) {
    if (!W1 || !W2 || !dst) {
        dinoseg_set_error("dinoseg_op_pack_mlp: null pointer");
        return -1;
    }
    return launch_pack_mlp(W1, W2, D, F, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_mlp_fused(float* X, const float* gamma, const float* beta, float eps, const void* Wp, const float* b1,
                                    const float* b2, int32_t M, int32_t D, int32_t F, void* stream) {
    if (!X || !gamma || !beta || !Wp || !b1 || !b2 || !mlp_fused_supported(D, F, 1)) {
        dinoseg_set_error("dinoseg_op_mlp_fused: null pointer or unsupported shape D=%d F=%d", D, F);
        return -1;
    }
    MlpFusedParams g = {};
    g.X = X; g.ldx = D; g.gamma = gamma; g.beta = beta; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b1 = b1; g.b2 = b2; g.M = M; g.fmt = options().op_fmt;
    return launch_mlp_fused2(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_proj_pack_elems(int32_t D) { return mlp_fused_proj_pack_elems(D); }

extern "C" int dinoseg_op_pack_proj(const float* Wsrc, int32_t D, void* dst, void* stream) {
    if (!Wsrc || !dst || mlp_fused_proj_pack_elems(D) <= 0) {
        dinoseg_set_error("dinoseg_op_pack_proj: null pointer or unsupported width D=%d", D);
        return -1;
    }
    return launch_pack_proj(Wsrc, D, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_proj_mlp_fused(float* X, const void* ctx, const void* Wproj, const float* bproj, const float* gamma,
                                         const float* beta, float eps, const void* Wp, const float* b1, const float* b2, int32_t M,
                                         int32_t D, int32_t F, void* stream) {
    if (!X || !ctx || !Wproj || !bproj || !gamma || !beta || !Wp || !b1 || !b2 || !mlp_fused_supported(D, F, 1) ||
        mlp_fused_proj_pack_elems(D) <= 0) {
        dinoseg_set_error("dinoseg_op_proj_mlp_fused: null pointer or unsupported shape D=%d F=%d", D, F);
        return -1;
    }
    MlpFusedParams g = {};
    g.X = X; g.ldx = D; g.gamma = gamma; g.beta = beta; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b1 = b1; g.b2 = b2; g.M = M;
    g.ctx = reinterpret_cast<const bf16_t*>(ctx); g.Wproj = reinterpret_cast<const bf16_t*>(Wproj); g.bproj = bproj;
    g.fmt = options().op_fmt;
    return launch_mlp_fused2(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_pack_rs(const float* W, int32_t N, int32_t K, int32_t kind, void* dst, void* stream) {
    return launch_pack_rs(W, N, K, kind, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_gemm_rs(const void* A, int32_t lda, const void* Wp, const float* bias, int32_t M, int32_t N, int32_t K, int32_t epi,
                                  float* x_inout, void* out16, int32_t ldo, void* q, void* k, void* v, int32_t ntok, int32_t npad,
                                  int32_t heads, float qscale, void* stream) {
    GemmParams g = {};
    g.A = reinterpret_cast<const bf16_t*>(A); g.lda = lda; g.W = reinterpret_cast<const bf16_t*>(Wp); g.bias = bias;
    g.M = M; g.N = N; g.K = K; g.planes = 1; g.fmt = options().op_fmt; g.epi = epi;
    g.out_f32 = x_inout; g.ldo_f32 = N; g.out_bf16 = reinterpret_cast<bf16_t*>(out16); g.ldo = ldo;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v);
    g.ntok = ntok; g.npad = npad; g.heads = heads; g.dmodel = heads * 64; g.qscale = qscale;
    return launch_gemm_rs(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_pack_rs_ln(const float* W, const float* gamma, const float* beta, const float* bias, int32_t N, int32_t K, void* dst_w,
                                     float* dst_bias, void* stream) {
    return launch_pack_rs_ln(W, gamma, beta, bias, N, K, reinterpret_cast<bf16_t*>(dst_w), dst_bias, reinterpret_cast<hipStream_t>(stream),
                             options().op_fmt);
}

extern "C" int dinoseg_op_ln_gemm_rs(const float* X, float eps, const void* Wp, const float* bias_folded, int32_t M, int32_t N, int32_t K,
                                     int32_t epi, void* out16, int32_t ldo, void* q, void* k, void* v, int32_t ntok, int32_t npad, int32_t heads,
                                     float qscale, void* stream) {
    if (!X) {
        dinoseg_set_error("dinoseg_op_ln_gemm_rs: null rows");
        return -1;
    }
    GemmParams g = {};
    g.ln_x = X; g.ln_eps = eps;
    g.W = reinterpret_cast<const bf16_t*>(Wp); g.bias = bias_folded;
    g.M = M; g.N = N; g.K = K; g.planes = 1; g.fmt = options().op_fmt; g.epi = epi;
    g.out_bf16 = reinterpret_cast<bf16_t*>(out16); g.ldo = ldo;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v);
    g.ntok = ntok; g.npad = npad; g.heads = heads; g.dmodel = heads * 64; g.qscale = qscale;
    return launch_gemm_rs(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_mlp3_pack_elems(int32_t D, int32_t F) { return mlp_fused3_pack_elems(D, F); }

extern "C" int dinoseg_op_pack_mlp3(const float* Wproj, const float* W1, const float* b1, const float* W2, const float* gamma2, const float* beta2,
                                    const float* Wqkv_next, const float* bqkv_next, const float* gamma1_next, const float* beta1_next, int32_t D,
                                    int32_t F, int32_t fmt, void* dst, void* stream) {
    if (fmt != FMT_BF16 && fmt != FMT_FP16) {
        dinoseg_set_error("dinoseg_op_pack_mlp3: bad operand format %d", fmt);
        return -1;
    }
    MlpFused3Weights w = {Wproj, W1, b1, W2, gamma2, beta2, Wqkv_next, bqkv_next, gamma1_next, beta1_next};
    return launch_pack_mlp3(w, D, F, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream), fmt);
}

extern "C" int dinoseg_op_proj_mlp_fused3(float* X, const void* ctx, int64_t ctx_plane, const float* bproj, float eps, const void* Wp, const float* b2,
                                          int32_t M, int32_t D, int32_t F, int32_t fmt, void* stream) {
    if (!mlp_fused3_supported(D, F, 2) || (fmt != FMT_BF16 && fmt != FMT_FP16)) {
        dinoseg_set_error("dinoseg_op_proj_mlp_fused3: unsupported shape D=%d F=%d or format %d", D, F, fmt);
        return -1;
    }
    MlpFused3Params g = {};
    g.X = X; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b2 = b2; g.M = M;
    g.ctx = reinterpret_cast<const bf16_t*>(ctx); g.ctx_plane = ctx_plane; g.bproj = bproj; g.fmt = fmt;
    return launch_mlp_fused3(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_block_tail_fused3(float* X, const void* ctx, int64_t ctx_plane, const float* bproj, float eps, const void* Wp,
                                            const float* b2, void* q, void* k, void* v, int64_t qkv_plane, int32_t B, int32_t ntok, int32_t npad,
                                            int32_t heads, float qscale, int32_t v_bf16, int32_t D, int32_t F, int32_t fmt, void* stream) {
    if (!mlp_fused3_supported(D, F, 2) || (fmt != FMT_BF16 && fmt != FMT_FP16) || !q || B <= 0 || npad % 64 != 0) {
        dinoseg_set_error("dinoseg_op_block_tail_fused3: unsupported shape D=%d F=%d, format %d, or null q", D, F, fmt);
        return -1;
    }
    MlpFused3Params g = {};
    g.X = X; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b2 = b2; g.M = B * ntok;
    g.ctx = reinterpret_cast<const bf16_t*>(ctx); g.ctx_plane = ctx_plane; g.bproj = bproj; g.fmt = fmt;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v); g.qkv_plane = qkv_plane;
    g.ntok = ntok; g.npad = npad; g.heads = heads; g.qscale = qscale; g.v_bf16 = v_bf16;
    return launch_mlp_fused3(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_mlp4_pack_elems(int32_t D, int32_t F) { return mlp_fused4_pack_elems(D, F); }

extern "C" int dinoseg_op_pack_mlp4(const float* Wproj, const float* W1, const float* b1, const float* W2, const float* gamma2, const float* beta2,
                                    const float* Wqkv_next, const float* bqkv_next, const float* gamma1_next, const float* beta1_next, int32_t D,
                                    int32_t F, int32_t fmt, void* dst, void* stream) {
    if (fmt != FMT_BF16 && fmt != FMT_FP16) {
        dinoseg_set_error("dinoseg_op_pack_mlp4: bad operand format %d", fmt);
        return -1;
    }
    MlpFused3Weights w = {Wproj, W1, b1, W2, gamma2, beta2, Wqkv_next, bqkv_next, gamma1_next, beta1_next};
    return launch_pack_mlp4(w, D, F, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream), fmt);
}

extern "C" int dinoseg_op_proj_mlp_fused4(float* X, const void* ctx, const float* bproj, float eps, const void* Wp, const float* b2, int32_t M,
                                          int32_t D, int32_t F, int32_t fmt, void* stream) {
    if (!mlp_fused4_supported(D, F, 1) || (fmt != FMT_BF16 && fmt != FMT_FP16)) {
        dinoseg_set_error("dinoseg_op_proj_mlp_fused4: unsupported shape D=%d F=%d or format %d", D, F, fmt);
        return -1;
    }
    MlpFused3Params g = {};
    g.X = X; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b2 = b2; g.M = M;
    g.ctx = reinterpret_cast<const bf16_t*>(ctx); g.bproj = bproj; g.fmt = fmt;
    return launch_mlp_fused4(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_block_tail_fused4(float* X, const void* ctx, const float* bproj, float eps, const void* Wp, const float* b2, void* q, void* k,
                                            void* v, int32_t B, int32_t ntok, int32_t npad, int32_t heads, float qscale, int32_t D, int32_t F,
                                            int32_t fmt, void* stream) {
    if (!mlp_fused4_supported(D, F, 1) || (fmt != FMT_BF16 && fmt != FMT_FP16) || !q || B <= 0 || npad % 64 != 0) {
        dinoseg_set_error("dinoseg_op_block_tail_fused4: unsupported shape D=%d F=%d, format %d, or null q", D, F, fmt);
        return -1;
    }
    MlpFused3Params g = {};
    g.X = X; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b2 = b2; g.M = B * ntok;
    g.ctx = reinterpret_cast<const bf16_t*>(ctx); g.bproj = bproj; g.fmt = fmt;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v);
    g.ntok = ntok; g.npad = npad; g.heads = heads; g.qscale = qscale;
    return launch_mlp_fused4(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_qkv_pack_elems(int32_t D) { return mlp_fused_qkv_pack_elems(D); }

extern "C" int dinoseg_op_pack_qkv(const float* Wsrc, int32_t D, void* dst, void* stream) {
    if (!Wsrc || !dst || mlp_fused_qkv_pack_elems(D) <= 0) {
        dinoseg_set_error("dinoseg_op_pack_qkv: null pointer or unsupported width D=%d", D);
        return -1;
    }
    return launch_pack_qkv(Wsrc, D, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_block_tail_fused(float* X, const void* ctx, const void* Wproj, const float* bproj, const float* gamma2,
                                           const float* beta2, float eps, const void* Wp, const float* b1, const float* b2,
                                           const void* Wqkv, const float* bqkv, const float* gamma1, const float* beta1, void* q, void* k,
                                           void* v, int32_t B, int32_t ntok, int32_t npad, int32_t heads, float qscale, int32_t D,
                                           int32_t F, void* stream) {
    if (!X || !ctx || !Wproj || !bproj || !gamma2 || !beta2 || !Wp || !b1 || !b2 || !Wqkv || !bqkv || !gamma1 || !beta1 || !q || !k ||
        !v || B <= 0 || ntok <= 0 || npad < ntok || npad % 64 != 0 || heads * 64 != D || !mlp_fused_supported(D, F, 1) ||
        mlp_fused_proj_pack_elems(D) <= 0 || mlp_fused_qkv_pack_elems(D) <= 0) {
        dinoseg_set_error("dinoseg_op_block_tail_fused: null pointer or unsupported shape D=%d F=%d heads=%d", D, F, heads);
        return -1;
    }
    MlpFusedParams g = {};
    g.X = X; g.ldx = D; g.gamma = gamma2; g.beta = beta2; g.eps = eps;
    g.Wp = reinterpret_cast<const bf16_t*>(Wp); g.b1 = b1; g.b2 = b2; g.M = B * ntok;
    g.ctx = reinterpret_cast<const bf16_t*>(ctx); g.Wproj = reinterpret_cast<const bf16_t*>(Wproj); g.bproj = bproj;
    g.Wqkv = reinterpret_cast<const bf16_t*>(Wqkv); g.bqkv = bqkv; g.gamma1 = gamma1; g.beta1 = beta1;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v);
    g.ntok = ntok; g.npad = npad; g.heads = heads; g.qscale = qscale; g.fmt = options().op_fmt;
    return launch_mlp_fused2(g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int64_t dinoseg_op_ln_gemm_slab_elems(int32_t N, int32_t K, int32_t planes) {
    return gemm_ln_supported(K, N, planes, EPI_GELU, 0) ? gemm_ln_slab_elems(N, K, planes) : -1;
}

extern "C" int dinoseg_op_pack_slabs(const float* Wsrc, int32_t N, int32_t K, int32_t planes, void* dst, void* stream) {
    if (!Wsrc || !dst || !gemm_ln_supported(K, N, planes, EPI_GELU, 0)) {
        dinoseg_set_error("dinoseg_op_pack_slabs: unsupported shape N=%d K=%d planes=%d", N, K, planes);
        return -1;
    }
    return launch_pack_slabs(Wsrc, N, K, planes, reinterpret_cast<bf16_t*>(dst), reinterpret_cast<hipStream_t>(stream),
                             planes == 1 ? options().op_fmt : FMT_BF16);
}

extern "C" int dinoseg_op_ln_gemm(const float* X, const float* gamma, const float* beta, float eps, const void* Wp, int64_t w_plane,
                                  const float* bias, int32_t M, int32_t N, int32_t K, int32_t planes, int32_t epi, void* out_bf16,
                                  int64_t out_plane, void* q, void* k, void* v, int64_t qkv_plane, int32_t ntok, int32_t npad,
                                  int32_t heads, float qscale, void* a_out, void* aux_out, void* stream) {
    LnGemmParams g = {};
    g.X = X; g.ldx = K; g.gamma = gamma; g.beta = beta; g.eps = eps;
    g.W = reinterpret_cast<const bf16_t*>(Wp); g.w_plane = w_plane; g.bias = bias;
    g.M = M; g.N = N; g.epi = epi;
    g.out_bf16 = reinterpret_cast<bf16_t*>(out_bf16); g.out_plane = out_plane; g.ldo = N;
    g.q = reinterpret_cast<bf16_t*>(q); g.k = reinterpret_cast<bf16_t*>(k); g.v = reinterpret_cast<bf16_t*>(v);
    g.qkv_plane = qkv_plane; g.ntok = ntok; g.npad = npad; g.heads = heads; g.dmodel = heads * 64; g.qscale = qscale;
    g.a_out = reinterpret_cast<bf16_t*>(a_out); g.a_plane = (long)M * K;
    g.aux_out = reinterpret_cast<bf16_t*>(aux_out); g.aux_plane = out_plane;
    g.fmt = planes == 1 ? options().op_fmt : FMT_BF16;
    return launch_gemm_ln(g, K, planes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_attention(const void* q, const void* k, const void* v, int64_t qkv_plane, void* ctx,
                                    int64_t ctx_plane, float* lse, int32_t B, int32_t heads, int32_t ntok, int32_t npad,
                                    int32_t planes, void* stream) {
    AttnParams a = {};
    a.q = reinterpret_cast<const bf16_t*>(q); a.k = reinterpret_cast<const bf16_t*>(k);
    a.v = reinterpret_cast<const bf16_t*>(v); a.qkv_plane = qkv_plane;
    a.ctx = reinterpret_cast<bf16_t*>(ctx); a.ctx_plane = ctx_plane; a.lse = lse;
    a.B = B; a.heads = heads; a.ntok = ntok; a.npad = npad; a.planes = planes;
    a.fmt = options().op_fmt;
    a.v_bf16 = options().op_v_bf16;
    return launch_attention(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, int32_t M, int32_t D,
                                    void* out_bf16, int64_t out_plane, int32_t planes, float* out_f32, int32_t drop_cls,
                                    int32_t ntok, void* stream) {
    return launch_layernorm(x, gamma, beta, eps, M, D, reinterpret_cast<bf16_t*>(out_bf16), out_plane, planes, out_f32,
                            drop_cls, ntok, reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_pos_resample_hw(const float* pos_embed, int32_t g, int32_t D, int32_t oh, int32_t ow, float* out, void* stream) {
    if (!pos_embed || !out || g <= 0 || D <= 0 || oh <= 0 || ow <= 0) {
        dinoseg_set_error("dinoseg_op_pos_resample: bad argument");
        return -1;
    }
    return launch_pos_resample(pos_embed, g, D, oh, ow, out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_pos_resample(const float* pos_embed, int32_t g, int32_t D, int32_t o, float* out, void* stream) {
    return dinoseg_op_pos_resample_hw(pos_embed, g, D, o, o, out, stream);
}

extern "C" int dinoseg_op_patch_gather_hw(const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, void* out, int64_t out_plane,
                                          int32_t planes, void* stream) {
    if (!frame_ok(H, W)) {
        dinoseg_set_error("Resolution should be a multiple of 8.");
        return -1;
    }
    float mean255[3], inv255[3];
    norm_consts(mean255, inv255);
    return launch_patch_gather(x, x_kind, B, H, W, mean255, inv255, reinterpret_cast<bf16_t*>(out), out_plane, planes,
                               reinterpret_cast<hipStream_t>(stream), planes == 2 ? options().op_fmt : FMT_BF16);
}

// the gather at either patch size (8: the entry above; 16: rows 768 wide); both plane counts in the op_fmt format
extern "C" int dinoseg_op_patch_gather_p(const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t patch, void* out,
                                         int64_t out_plane, int32_t planes, void* stream) {
    if (patch != 8 && patch != 16) {
        dinoseg_set_error("dinoseg_op_patch_gather_p: patch=%d must be 8 or 16", patch);
        return -1;
    }
    if (!frame_ok(H, W, patch)) {
        set_resolution_error(patch);
        return -1;
    }
    if (!x || !out || B <= 0 || (planes != 1 && planes != 2) || (x_kind != DINOSEG_INPUT_U8_HWC && x_kind != DINOSEG_INPUT_F32_CHW) ||
        (planes == 2 && out_plane < (int64_t)B * (H / patch) * (W / patch) * 3 * patch * patch)) {
        dinoseg_set_error("dinoseg_op_patch_gather_p: bad argument");
        return -1;
    }
    float mean255[3], inv255[3];
    norm_consts(mean255, inv255);
    return launch_patch_gather(x, x_kind, B, H, W, mean255, inv255, reinterpret_cast<bf16_t*>(out), out_plane, planes,
                               reinterpret_cast<hipStream_t>(stream), options().op_fmt, patch);
}

extern "C" int dinoseg_op_patch_gather(const void* x, int32_t x_kind, int32_t B, int32_t r, void* out, int64_t out_plane,
                                       int32_t planes, void* stream) {
    return dinoseg_op_patch_gather_hw(x, x_kind, B, r, r, out, out_plane, planes, stream);
}

extern "C" int dinoseg_op_head_final(const void* in, int64_t in_plane, int32_t ld, int32_t M, int32_t K, const float* Wc,
                                     const float* b, int32_t C, float* logp, int32_t* argmax, void* stream) {
    return launch_head_final(reinterpret_cast<const bf16_t*>(in), in_plane, ld, M, K, Wc, b, C, logp, argmax,
                             reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_head_wide(const void* in, int64_t in_plane, int32_t ld, int32_t M, int32_t K, const void* Wp, int64_t w_plane,
                                    const float* b, int32_t C, float* logp, int32_t* argmax, void* stream) {
    return launch_head_wide(reinterpret_cast<const bf16_t*>(in), in_plane, ld, M, K, reinterpret_cast<const bf16_t*>(Wp), w_plane, b, C,
                            logp, argmax, reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

// ---- the helper kernels on their own (tests/test_helper_ops_gpu.py): every entry checks its arguments on the host first ----
extern "C" int dinoseg_op_attn_probs(const void* q, const void* k, int64_t qkv_plane, int32_t planes, int32_t B, int32_t heads, int32_t ntok,
                                     int32_t npad, float* out, void* stream) {
    if (!q || !k || !out) {
        dinoseg_set_error("dinoseg_op_attn_probs: null pointer");
        return -1;
    }
    if ((planes != 1 && planes != 2) || B < 1 || heads < 1 || ntok < 1 || npad < ntok || (int64_t)B * heads > 65535 ||
        (planes == 2 && qkv_plane < (int64_t)B * heads * npad * 64)) {
        dinoseg_set_error("dinoseg_op_attn_probs: bad argument (planes=%d B=%d heads=%d ntok=%d npad=%d qkv_plane=%lld)", planes, B, heads, ntok,
                          npad, (long long)qkv_plane);
        return -1;
    }
    return launch_attn_probs(reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), qkv_plane, planes, B, heads, ntok, npad, out,
                             reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int32_t dinoseg_cls_attention_max_tokens(void) { return cls_attention_max_tokens(); }

extern "C" int dinoseg_op_cls_attention(const void* q, const void* k, int64_t qkv_plane, int32_t planes, int32_t B, int32_t heads, int32_t ntok,
                                        int32_t npad, int32_t hp, int32_t wp, int32_t OH, int32_t OW, float threshold, float* attn_out,
                                        uint8_t* keep_out, void* stream) {
    const char* who = "dinoseg_op_cls_attention";
    if (!q || !k || (!attn_out && !keep_out)) {
        dinoseg_set_error("%s: null pointer (q, k, and at least one of attn_out / keep_out, are required)", who);
        return -1;
    }
    if (planes != 1 && planes != 2) {
        dinoseg_set_error("%s: planes=%d must be 1 or 2", who, planes);
        return -1;
    }
    if (cls_attention_check(who, B, heads, ntok, hp, wp, OH, OW, keep_out != nullptr, threshold)) return -1;
    if (npad < ntok) {
        dinoseg_set_error("%s: npad=%d is smaller than ntok=%d", who, npad, ntok);
        return -1;
    }
    if ((int64_t)B * heads > INT64_MAX / 64 / npad) {
        dinoseg_set_error("%s: B*heads*npad*64 (B=%d heads=%d npad=%d) is too large", who, B, heads, npad);
        return -1;
    }
    if (planes == 2 && (qkv_plane < (int64_t)B * heads * npad * 64 || qkv_plane % 8 != 0)) {
        dinoseg_set_error("%s: qkv_plane=%lld puts the lo plane inside the hi plane of %lld elements, or off a 16-byte boundary", who,
                          (long long)qkv_plane, (long long)B * heads * npad * 64);
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) {
        dinoseg_set_error("%s: q and k must be 16-byte aligned", who);
        return -1;
    }
    return launch_cls_attention(reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), qkv_plane, planes, B, heads, ntok, npad,
                                hp, wp, OH, OW, threshold, attn_out, keep_out, reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_cls_mask_attn(const void* q, const void* k, const void* v, int64_t qkv_plane, int32_t planes, int32_t heads,
                                        int32_t ntok, int32_t npad, const float* mask, int32_t n_masks, void* ctx, int64_t ctx_plane,
                                        float* probs, void* stream) {
    if (!q || !k || !v || !mask || !ctx) {
        dinoseg_set_error("dinoseg_op_cls_mask_attn: null pointer");
        return -1;
    }
    if ((planes != 1 && planes != 2) || heads < 1 || heads > 65535 || ntok < 1 || npad < ntok || n_masks < 1 ||
        (planes == 2 && (qkv_plane < (int64_t)heads * npad * 64 || ctx_plane < (int64_t)n_masks * heads * 64))) {
        dinoseg_set_error("dinoseg_op_cls_mask_attn: bad argument (planes=%d heads=%d ntok=%d npad=%d n_masks=%d qkv_plane=%lld ctx_plane=%lld)",
                          planes, heads, ntok, npad, n_masks, (long long)qkv_plane, (long long)ctx_plane);
        return -1;
    }
    return launch_cls_mask_attn(reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), reinterpret_cast<const bf16_t*>(v),
                                qkv_plane, planes, heads, ntok, npad, mask, n_masks, reinterpret_cast<bf16_t*>(ctx), ctx_plane, probs,
                                reinterpret_cast<hipStream_t>(stream), options().op_fmt);
}

extern "C" int dinoseg_op_cls_rows(float* X, const float* cls, const float* pos, int32_t B, int32_t ntok, int32_t D, void* stream) {
    if (!X || !cls || !pos) {
        dinoseg_set_error("dinoseg_op_cls_rows: null pointer");
        return -1;
    }
    if (B < 1 || ntok < 1 || D < 1 || (int64_t)B * D > INT32_MAX) {
        dinoseg_set_error("dinoseg_op_cls_rows: bad shape B=%d ntok=%d D=%d", B, ntok, D);
        return -1;
    }
    return launch_cls_rows(X, cls, pos, B, ntok, D, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_broadcast_row0(float* X, int32_t D, int32_t n, void* stream) {
    if (!X) {
        dinoseg_set_error("dinoseg_op_broadcast_row0: null pointer");
        return -1;
    }
    if (D < 1 || n < 0) {
        dinoseg_set_error("dinoseg_op_broadcast_row0: bad shape D=%d n=%d", D, n);
        return -1;
    }
    if (n == 0) return 0;
    return launch_broadcast_row0(X, D, n, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_batch_sum_rows(const float* X, int32_t B, int32_t ntok, int32_t D, float* out, void* stream) {
    if (!X || !out) {
        dinoseg_set_error("dinoseg_op_batch_sum_rows: null pointer");
        return -1;
    }
    if (B < 1 || ntok < 1 || D < 1) {
        dinoseg_set_error("dinoseg_op_batch_sum_rows: bad shape B=%d ntok=%d D=%d", B, ntok, D);
        return -1;
    }
    return launch_batch_sum_rows(X, B, ntok, D, out, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_multi_pack(int32_t count, const float* const* src, void* const* dst, const int64_t* plane, const int32_t* rows,
                                     const int32_t* cols, const int32_t* rows_pad, const int32_t* cols_pad, const int32_t* planes,
                                     const int32_t* transposed, const int32_t* fmt, void* stream) {
    if (count < 0 || (count > 0 && (!src || !dst || !plane || !rows || !cols || !rows_pad || !cols_pad || !planes || !transposed || !fmt))) {
        dinoseg_set_error("dinoseg_op_multi_pack: bad argument");
        return -1;
    }
    std::vector<PackJob> jobs(count);
    for (int i = 0; i < count; ++i) {
        const int64_t elems = (int64_t)rows_pad[i] * cols_pad[i];
        if (rows[i] < 0 || cols[i] < 0 || rows_pad[i] < rows[i] || cols_pad[i] < cols[i] || (planes[i] != 1 && planes[i] != 2) ||
            (transposed[i] != 0 && transposed[i] != 1) || (fmt[i] != FMT_BF16 && fmt[i] != FMT_FP16) || (planes[i] == 2 && plane[i] < elems)) {
            dinoseg_set_error("dinoseg_op_multi_pack: bad job %d (rows=%d cols=%d rows_pad=%d cols_pad=%d planes=%d transposed=%d fmt=%d plane=%lld)",
                              i, rows[i], cols[i], rows_pad[i], cols_pad[i], planes[i], transposed[i], fmt[i], (long long)plane[i]);
            return -1;
        }
        if (elems > 0 && (!dst[i] || (!src[i] && (int64_t)rows[i] * cols[i] > 0))) {      // (an empty job may carry null pointers)
            dinoseg_set_error("dinoseg_op_multi_pack: null pointer at job %d", i);
            return -1;
        }
        PackJob& j = jobs[i];
        j.src = src[i]; j.dst = reinterpret_cast<bf16_t*>(dst[i]); j.plane = plane[i];
        j.rows = rows[i]; j.cols = cols[i]; j.rows_pad = rows_pad[i]; j.cols_pad = cols_pad[i];
        j.planes = planes[i]; j.transposed = transposed[i]; j.fmt = fmt[i];
    }
    return launch_multi_pack(jobs.data(), count, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dinoseg_op_multi_zero(int32_t count, float* const* p, const int64_t* n, void* stream) {
    if (count < 0 || (count > 0 && (!p || !n))) {
        dinoseg_set_error("dinoseg_op_multi_zero: bad argument");
        return -1;
    }
    std::vector<long> nn(count);
    for (int i = 0; i < count; ++i) {
        if (!p[i] || n[i] < 0) {
            dinoseg_set_error("dinoseg_op_multi_zero: null pointer or negative size at tensor %d", i);
            return -1;
        }
        nn[i] = (long)n[i];
    }
    return launch_multi_zero(count, p, nn.data(), reinterpret_cast<hipStream_t>(stream));
}
