// Internal: the handle behind the C-ABI (shared by api.hip, forward.hip, train_api.hip and backward.hip).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/dinoseg.h"
#include "common.h"
#include "kernels.h"

using namespace dseg;   // internal header: only included by the API translation units

#define DSEG_TRY(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

// ------------------------------------------------------------------------------------------------ handle
struct BoundTensor {
    const float* ptr = nullptr;
    std::vector<int64_t> shape;
};

struct PackedLinear {       // W[N,K] operand planes of one nn.Linear, padded to the GEMM tile
    bf16_t* w = nullptr;
    long plane = 0;
    int n_pad = 0, k_pad = 0;
    float* bias_pad = nullptr;   // only when N was padded (head layers); else the bound bias is used
};

// The weights as dinoseg_refresh_weights resolved them: the bound fp32 tensors and the library-owned copies (pointers into wbuf;
// null = that copy does not exist under the options of the last refresh).  Filled by the refresh and by nothing else; every
// reader checks weights_ready first, which dinoseg_bind_weight clears, so a record is never read stale.
struct LinearRec {          // one nn.Linear
    const float* w = nullptr;    // bound weight [N, K] and bias [N]
    const float* b = nullptr;
    int N = 0, K = 0, planes = 0, fmt = 0;
    int rs_bit = 0;              // its bit of option gemm_rs (block linears: 1 mlp.fc1, 2 attn.qkv, 4 attn.proj and mlp.fc2; else 0)
    PackedLinear pk;             // operand planes (every linear that feeds gemm.hip)
    bf16_t* slab = nullptr;      // qkv / fc1: slab-major copy for the LayerNorm-fused kernel (gemm_ln.hip), where supported
    bf16_t* rs = nullptr;        // one-plane modes at embed_dim 768: the fragment-order copy gemm_rs.hip streams ...
    float* rs_bias = nullptr;    // ... and, when that copy carries the LayerNorm in front of the linear (gemm_rs_ln_snap), the folded bias
};
struct BlockRec {           // one transformer block
    const float *norm1_w = nullptr, *norm1_b = nullptr, *norm2_w = nullptr, *norm2_b = nullptr;
    LinearRec qkv, proj, fc1, fc2;
    bf16_t* mlp = nullptr;       // fc1 + fc2 in MFMA fragment order (mlp_fused2.hip)
    bf16_t* projf = nullptr;     // attn.proj.weight in the same fragment order (mlp_fused2.hip, PROJ)
    bf16_t* qkvf = nullptr;      // attn.qkv.weight in fragment order (mlp_fused2.hip, QKV tail of the block before; never block 0)
    bf16_t* mlp3 = nullptr;      // hi + lo modes: attn.proj + fc1 + fc2 (+ the next block's qkv) as the slot stream of mlp_fused3.hip
    bf16_t* mlp4 = nullptr;      // one-plane modes, option mlp_fused4: the same as the slot stream of mlp_fused4.hip
};
struct ModelRec {
    LinearRec patch;             // dino.patch_embed.proj
    const float *cls_token = nullptr, *pos_embed = nullptr, *norm_w = nullptr, *norm_b = nullptr;
    std::vector<BlockRec> blocks;
    LinearRec head[2];           // clf.layer_1 / layer_2 of the MLP head
    LinearRec clf;               // the classifier (layer_3 of the MLP head, layer_1 of the linear head): fp32 for launch_head_final;
                                 // pk = its hi+lo planes for the wide head kernel (n_classes > 32), empty below that
};

// The training half, in ModelRec's shape: where dinoseg_bind_grad put each parameter's gradient buffer (null = frozen), and the
// transposed copies of the linears' weights the input-gradient GEMMs multiply by.  Not part of ModelRec: a refresh resets that
// record, the gradient bindings outlive it.  Sized by dinoseg_create and never resized (grad_index points into it).
struct GradSlot {
    float* ptr = nullptr;        // the caller's fp32 buffer
    long numel = 0;
    bool backbone = false;       // a dino.* parameter (as opposed to the head's)
};
struct LinearGrad {
    GradSlot dw, db;
    bf16_t* tw = nullptr;        // W^T planes [k_pad][n_pad] in twbuf, packed at the top of every backward
    long t_plane = 0;
    int n_pad = 0, k_pad = 0;    // (0: no transposed copy -- the patch embedding has no input gradient)
};
struct BlockGrad {
    GradSlot norm1_w, norm1_b, norm2_w, norm2_b;
    LinearGrad qkv, proj, fc1, fc2;
};
struct GradRec {
    LinearGrad patch;
    GradSlot cls_token, pos_embed, norm_w, norm_b;
    std::vector<BlockGrad> blocks;
    LinearGrad head[2], clf;
};

struct dinoseg_handle {
    dinoseg_config cfg;
    int planes;
    int fmt = 0;                // operand format: FMT_BF16 / FMT_FP16 (DINOSEG_FP16: planes = 1, DINOSEG_FP16X3: planes = 2, both fmt = FMT_FP16)
    int device = -1;            // ordinal of the GPU that owns the bound tensors (set by the first dinoseg_bind_weight)
    // the bind API's name index: what each key must look like, what was bound to it, which gradient slot it names.  Readers of the
    // parameters work from the typed records (model, grad), never from these
    std::map<std::string, BoundTensor> bound;
    std::map<std::string, std::vector<int64_t>> expected;
    std::map<std::string, GradSlot*> grad_index;
    // packed weights (library-owned)
    char* wbuf = nullptr;
    size_t wbuf_bytes = 0;
    ModelRec model;             // what the last dinoseg_refresh_weights resolved and packed (valid while weights_ready)
    bool weights_ready = false;
    int fp16_patch_planes_snap = 1;        // option fp16_patch_planes as of the last dinoseg_refresh_weights (what the packs were made for)
    int mlp_fused4_snap = 0;               // ... mlp_fused4, gemm_rs and gemm_rs_ln likewise (kernels.h Options: which of them a forward reads)
    int gemm_rs_snap = 0;
    int gemm_rs_ln_snap = 0;
    struct WbufEntry {                     // one packed copy in wbuf: what it is, where it starts, how long it is
        std::string what;
        size_t off, bytes;
        bool operator==(const WbufEntry& o) const { return what == o.what && off == o.off && bytes == o.bytes; }
    };
    std::vector<WbufEntry> wbuf_layout;    // the copies of the last refresh, in wbuf order (a change of layout is a new generation)
    int64_t generation = 0;     // dinoseg_state_generation: bumped when an address or cached content a captured forward bakes in changes
    // pos-embed cache
    float* pos_cache = nullptr;
    int pos_hp = -1, pos_wp = -1;   // patch grid (rows, columns) the cache holds (-1: nothing)
    bool pos_stale = false;     // dino.pos_embed was (re)bound since the cache was filled
    size_t pos_cap = 0;
    // activation workspace (library-owned)
    char* ws = nullptr;
    size_t ws_bytes = 0;
    int ws_B = -1, ws_H = -1, ws_W = -1;
    // second half-batch of a split forward (option "streams" = 2): its own workspace, an internal stream, fork / join events
    char* ws2 = nullptr;
    size_t ws2_bytes = 0;
    int ws2_B = -1, ws2_H = -1, ws2_W = -1;
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool in_split = false;                 // a split forward is being queued (both halves' launches share the chip)
    // fine-tune step state (train_api.hip, backward.hip; the layout of tws: train_ws.h)
    GradRec grad;                          // bound gradient buffers and the transposed weights
    char* tws = nullptr;                  // training workspace: saved activations + backward scratch
    size_t tws_bytes = 0;
    int tws_B = -1, tws_H = -1, tws_W = -1;
    int tr_B = -1, tr_H = -1, tr_W = -1;   // batch / frame size of the saved forward dinoseg_backward will differentiate
    int* bad_label_flag = nullptr;         // sticky "a label outside [0, C) other than -100 was seen" (device int, owned by the handle:
                                           // it must survive the training workspace being re-laid out for another batch shape)
    // gradient-stage events of the last backward (dinoseg_stream_wait_grad_stage): stage 0 = head, 1 + k = final norm and block
    // n_blocks-1-k, n_blocks + 1 = embeddings; stage_done = number of stages the last backward recorded
    std::vector<hipEvent_t> stage_ev;
    int stage_done = 0;
    // fork / join events of the weight-gradient side stream (option train_streams = 2: backward.hip, SideStream); aux_stream is shared with
    // the split forward
    std::vector<hipEvent_t> bw_ev;
    char* twbuf = nullptr;                 // transposed packed weights for the input-gradient GEMMs
    size_t twbuf_bytes = 0;
    char* dws = nullptr;                   // pixel-label step (dinoseg_train_step_dense_hw): d loss / d logp [B*n, C], then the loss scratch
    size_t dws_bytes = 0;
    // optional per-kernel-class timing with HIP events on the caller's stream (bench.py roofline leg)
    int prof_level = 0;                    // 0 off, 1 attention only, 2 every class
    struct ProfRec { int cat; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
};

// Every entry point that takes a handle runs on the handle's device, whatever the caller's current device is (the reference's
// model.to('cuda:1') pattern leaves the current device at 0): allocations, hipFuncSetAttribute and launches all follow it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const dinoseg_handle* h) {
        if (!h || h->device < 0) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
// a non-default stream must live on the handle's device: a launch on another device's stream with this device's pointers faults
static inline int check_stream_device(const dinoseg_handle* h, hipStream_t s) {
    if (!h || h->device < 0 || s == nullptr) return 0;
    hipDevice_t d = -1;
    if (hipStreamGetDevice(s, &d) != hipSuccess) return 0;      // legacy / per-thread default stream handles
    if ((int)d != h->device) {
        dinoseg_set_error("stream belongs to device %d but the model's tensors live on device %d", (int)d, h->device);
        return -1;
    }
    return 0;
}

// the handle's side stream + its fork / join events (api.hip): created on first use, destroyed with the workspaces
int ensure_aux_stream(dinoseg_handle* h);

// the inference workspace of B frames of Hf x Wf (api.hip): byte offsets of its buffers, the plane strides, the row counts
struct WsLayout {
    size_t X, A, Q, K, V, CTX, HB, FEAT, H1, H2, total;
    long a_plane, qkv_plane, ctx_plane, hb_plane, feat_plane, h1_plane, h2_plane;
    int n, ntok, npad, M, Mp;
};
WsLayout make_layout(const dinoseg_handle* h, int B, int Hf, int Wf);
// slot 0: the caller's stream; slot 1: the second half-batch of a split forward (its own buffer, the handle's internal stream)
int ensure_workspace(dinoseg_handle* h, int slot, const WsLayout& L, int B, int Hf, int Wf, hipStream_t s);

static inline int prof_begin(dinoseg_handle* h, int cat, hipStream_t s) {
    if (h->prof_level == 0 || (h->prof_level == 1 && cat != DINOSEG_PROF_ATTN)) return -1;
    hipEvent_t ev[2];
    for (int i = 0; i < 2; ++i) {
        if (!h->prof_pool.empty()) {
            ev[i] = h->prof_pool.back();
            h->prof_pool.pop_back();
        } else if (hipEventCreate(&ev[i]) != hipSuccess) {
            return -1;
        }
    }
    h->prof_recs.push_back({cat, ev[0], ev[1]});
    (void)hipEventRecord(ev[0], s);
    return (int)h->prof_recs.size() - 1;
}
static inline void prof_end(dinoseg_handle* h, int idx, hipStream_t s) {
    if (idx >= 0) (void)hipEventRecord(h->prof_recs[idx].b, s);
}
// who enqueues: the handle, the stream, and whether the profiler counts the launches (the training forward records no events)
struct StepEnv {
    dinoseg_handle* h;
    hipStream_t s;
    bool profiled;
};
#define DSEG_PROF_ENV(env, cat, stmt)                                                         \
    do {                                                                                   \
        const int _pi = (env).profiled ? prof_begin((env).h, cat, (env).s) : -1;           \
        stmt;                                                                              \
        prof_end((env).h, _pi, (env).s);                                                   \
    } while (0)
// ... with h and s of the enclosing function
#define DSEG_PROF(cat, stmt) DSEG_PROF_ENV((StepEnv{h, s, true}), cat, stmt)

static inline int head_planes() { return 2; }
// the MLP head: embed_dim -> 200 -> 100 -> classes; the hidden activations are stored 256 / 128 wide, zero beyond their columns
constexpr int HEAD_H1 = 200, HEAD_H1_PAD = 256, HEAD_H2 = 100, HEAD_H2_PAD = 128;
// width of the d logits planes DZ: the classes rounded up to the 64-column k-step of the head's dgrad GEMM (launch_gemm_small: K % 64)
static inline int dz_ld(int C) { return (C + 63) / 64 * 64; }
// planes of the patch-embedding GEMM: the mode's own, except that the fp16 mode runs it split like the head (raw pixel operands,
// 0.13 % of the FLOPs)
static inline int patch_planes(const dinoseg_handle* h) { return (h->fmt == FMT_FP16 && h->fp16_patch_planes_snap == 2) ? 2 : h->planes; }
// format of the split (two-plane) operands of the head (and of the patch embedding where it runs split): fp16 only in the fp16 hi+lo
// mode -- the single-plane fp16 mode keeps them bf16 hi+lo (their error is far below that mode's)
static inline int split_fmt(const dinoseg_handle* h) { return h->planes == 2 ? h->fmt : (int)FMT_BF16; }
// format of the patch-embedding operands: the mode's own when it runs on the mode's planes, the split format otherwise
static inline int patch_fmt(const dinoseg_handle* h) { return patch_planes(h) == h->planes ? h->fmt : split_fmt(h); }   // the classifier head always runs in split precision (it is tiny)
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline const float* W(const dinoseg_handle* h, const std::string& k) { return h->bound.at(k).ptr; }
// the GemmParams fields that follow from which linear it is (a padded head layer multiplies its padded shape, with the padded bias);
// the call site adds what is its own: A, the outputs, the epilogue
static inline GemmParams linear_gemm(const LinearRec& l) {
    GemmParams g = {};
    g.W = l.pk.w; g.w_plane = l.pk.plane;
    g.N = l.pk.n_pad; g.K = l.pk.k_pad; g.planes = l.planes; g.fmt = l.fmt;
    g.bias = l.pk.bias_pad ? l.pk.bias_pad : l.b;
    return g;
}
static inline void norm_consts(float mean255[3], float inv255[3]) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c) {
        mean255[c] = mean[c] * 255.0f;          // albumentations: mean * max_pixel_value (fp32)
        inv255[c] = 1.0f / (sd[c] * 255.0f);    // reciprocal of std * max_pixel_value (fp32)
    }
}
// H x W frames: both positive multiples of the patch size, 8 or 16.  The ONE copy of the check and of its two messages (the
// reference's text at patch 8, pl_torch_modules.py:271-272; a patch-16 handle names 16): dino_amd/capi.py maps exactly these
// strings to ValueError.
static inline bool frame_ok(int32_t H, int32_t W, int32_t p = 8) { return H > 0 && W > 0 && H % p == 0 && W % p == 0; }
static inline void set_resolution_error(int32_t p) {
    dinoseg_set_error(p == 16 ? "Resolution should be a multiple of 16." : "Resolution should be a multiple of 8.");
}
static inline int32_t patch_of(const dinoseg_handle* h) { return h ? h->cfg.patch : 8; }
int dinoseg_train_release(dinoseg_handle* h);   // train_api.hip: frees the training workspace
