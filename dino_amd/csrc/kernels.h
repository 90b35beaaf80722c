// Host-side launch interface of the dinoseg HIP kernels (internal; the public C-ABI is include/dinoseg.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct dinoseg_augment_frame;       // include/dinoseg.h: one frame's augmentation parameters (36 words)

namespace dseg {

typedef uint16_t bf16_t;

enum GemmEpilogue {
    EPI_PLAIN = 0,   // out_f32[M,N] = acc (+ bias)
    EPI_RESID = 1,   // out_f32[M,N] += acc + bias            (attn.proj / mlp.fc2 + residual add)
    EPI_GELU = 2,    // out_bf16 planes = gelu_erf(acc + bias) (mlp.fc1)
    EPI_RELU = 3,    // out_bf16 planes = relu(acc + bias)     (head layer_1 / layer_2)
    EPI_QKV = 4,     // scatter to Q (pre-scaled), K, V : each [B,H,Npad,64]
    EPI_PATCH = 5,   // token rows: X[b*(n+1)+1+p, :] = acc + bias + pos[1+p, :]
    // --- backward / training (gemm.hip only) ---
    EPI_BF16 = 6,    // out_bf16 planes = acc (+ bias)
    EPI_ATOMIC = 7,  // out_f32 += acc by fp32 atomics (split-K weight gradients; out must be zeroed)
    EPI_DGELU = 8,   // out_bf16 planes = acc * gelu'(aux_in)   (aux_in = saved fc1 pre-activation planes)
    EPI_DRELU = 9,   // out_bf16 planes = acc * (aux_in > 0)    (aux_in = saved post-ReLU activation planes)
};

// C[M,N] = A[M,K] . W[N,K]^T  (both operands K-contiguous, bf16 hi(/lo) planes, fp32 accumulate)
struct GemmParams {
    const bf16_t* A; long a_plane; int lda;     // [planes][M][lda]
    const bf16_t* W; long w_plane;              // [planes][N][K]
    int M, N, K;
    int n_off;                                  // (gemm_big only) first output column / W row of this launch
    int n_valid;                                // ATOMIC: only columns < n_valid are written (0 = all N)
    int dbg;                                    // timing-only ablations: bit0 skip epilogue stores, bit1 skip steady-state loads
    int planes;                                 // 1: bf16 ; 2: bf16 hi+lo split (3 MFMAs per product)
    int fmt;                                    // operand format: 0 = bf16, 1 = fp16 (FMT_FP16: A, W and the 16-bit outputs of GELU / RELU / QKV).
                                                // One fp16 plane: EPI_QKV still writes V as bf16 (the fast attention's P.V product stays bf16);
                                                // fp16 hi+lo planes (planes == 2): every plane is fp16.  Inference epilogues only
    int epi;
    const float* bias;                          // [N] or null
    float* out_f32; int ldo_f32;                // PLAIN / RESID / PATCH
    bf16_t* out_bf16; long out_plane; int ldo;  // GELU / RELU : [planes][M][ldo]
    bf16_t* q; bf16_t* k; bf16_t* v; long qkv_plane;    // QKV
    int ntok, npad, heads, dmodel; float qscale;
    const float* pos; int n_patches;            // PATCH
    const float* resid;                         // RESID: out = resid + acc + bias (null: in place on out_f32)
    bf16_t* aux_out;                            // GELU: also save the pre-activation planes here (training), ld = ldo
    const bf16_t* aux_in; long aux_plane;       // DGELU / DRELU operand planes [planes][M][ldo]; also plane stride of aux_out
    int v_bf16;                                 // EPI_QKV with fp16 hi + lo planes: write V as bf16 hi + lo planes (AttnParams::v_bf16)
    int dispatch_rows;                          // launch_gemm's kernel choice is made for this many rows instead of M when > 0: the two
                                                // half-batches of a split forward take the route of the whole batch (same summation order)
    int ksplit;                                 // >1: split the K loop over grid.y (EPI_ATOMIC, or EPI_PLAIN partial tiles)
    long split_stride;                          // EPI_PLAIN with ksplit > 1: slice y writes out_f32 + y * split_stride (floats)
    // launch_gemm_rs, EPI_GELU / EPI_QKV only: A = (ln_x - mean) rstd per row, computed in the kernel's prologue (ln_x fp32 [M][K] rows, row stride K;
    // A unused); W / bias = launch_pack_rs_ln's copies, which carry the LayerNorm's weight and bias
    const float* ln_x; float ln_eps;
};
int launch_gemm(const GemmParams& p, hipStream_t s);       // dispatches between the two kernels below
int launch_gemm_small(const GemmParams& p, hipStream_t s); // 128x128 tile, bf16 or bf16x3 (gemm.hip)
bool gemm_big_supported(const GemmParams& p);
int launch_gemm_big(const GemmParams& p, hipStream_t s);   // 256x384 persistent tile, bf16 only (gemm_big.hip)

// Row-stationary streaming GEMMs for the wide model (gemm_rs.hip; one plane, embed_dim 768): p.W = the weight re-packed by launch_pack_rs
// (kind 0 for EPI_GELU / EPI_QKV: K = 768; kind 1 for EPI_RESID: N = 768, in place on out_f32)
bool gemm_rs_supported(const GemmParams& p);
int launch_pack_rs(const float* W, int N, int K, int kind, bf16_t* dst, hipStream_t s, int fmt);
int launch_pack_rs_ln(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, bf16_t* dst_w, float* dst_bias,
                      hipStream_t s, int fmt);
int launch_gemm_rs(const GemmParams& p, hipStream_t s);

// LayerNorm-fused A-stationary GEMM for qkv / fc1 (gemm_ln.hip): X fp32 rows are normalised in the prologue, W streams
struct LnGemmParams {
    const float* X; int ldx;                    // residual stream [M, K] fp32
    const float* gamma; const float* beta; float eps;
    const bf16_t* W; long w_plane;              // slab-major packed copy (launch_pack_slabs); w_plane unused
    const float* bias;                          // [N]
    int M, N;
    int epi;                                    // EPI_QKV or EPI_GELU
    bf16_t* out_bf16; long out_plane; int ldo;  // GELU: [planes][M][ldo]
    bf16_t* q; bf16_t* k; bf16_t* v; long qkv_plane; int ntok, npad, heads, dmodel; float qscale;   // QKV
    bf16_t* a_out; long a_plane;                // optional: the normalised planes [planes][M][K] (training: weight gradients)
    bf16_t* aux_out; long aux_plane;            // optional (GELU): pre-activation planes [planes][M][ldo] (training: gelu')
    int dbg;                                    // timing-only ablations (wrong results): 1 skip epilogue, 2 skip W DMA, 4 skip LN prologue
    int fmt;                                    // operand format (FMT_BF16 / FMT_FP16), as GemmParams::fmt
};
bool gemm_ln_supported(int K, int N, int planes, int epi, int dmodel);
long gemm_ln_slab_elems(int N, int K, int planes);      // bf16 elements of the slab-major copy of W [N][K]
int launch_pack_slabs(const float* src, int N, int K, int planes, bf16_t* dst, hipStream_t s, int fmt = 0);
int launch_gemm_ln(const LnGemmParams& p, int K, int planes, hipStream_t s);

// Fused MLP of one transformer block, single-plane modes, D = 384 (mlp_fused2.hip): X += fc2(gelu(fc1(LayerNorm(X))))   in place
struct MlpFusedParams {
    float* X; int ldx;                          // residual stream [M, 384] fp32
    const float* gamma; const float* beta; float eps;
    const bf16_t* Wp;                           // both weights in MFMA fragment order (launch_pack_mlp)
    const float* b1; const float* b2;           // [1536], [384]
    int M;
    int* queue;                                 // (diagnostic builds: MF2_STAMP buffer)
    int n_long, sleep_max;                      // set by launch_mlp_fused2: start-time spread of the workgroups with one item fewer
    // optional (mlp_fused2 only): the block's attention output projection in the same launch, X += ctx . Wproj^T + bproj first
    const bf16_t* ctx;                          // [M, 384] bf16 attention output (row stride 384), null = MLP only
    const bf16_t* Wproj;                        // launch_pack_proj
    const float* bproj;
    // optional (with ctx): LayerNorm1 + the qkv projection of the NEXT block at the end of the same launch (Q pre-scaled by qscale)
    const bf16_t* Wqkv;                         // launch_pack_qkv: [1152, 384] in fragment order; null = no qkv tail
    const float* bqkv; const float* gamma1; const float* beta1;
    bf16_t* q; bf16_t* k; bf16_t* v;            // each [B, heads, npad, 64] bf16 (rows >= ntok are never written)
    int ntok, npad, heads; float qscale;
    int fmt;                                    // mlp_fused2 only: operand format of ctx, the packed weights and everything in between
                                                // (FMT_BF16 / FMT_FP16); the qkv tail writes V as bf16 either way
};
long mlp_fused_qkv_pack_elems(int D);           // bf16 elements of the packed qkv weight (0: unsupported width)
int launch_pack_qkv(const float* W, int D, bf16_t* dst, hipStream_t s, int fmt = 0);
long mlp_fused_proj_pack_elems(int D);          // bf16 elements of the packed projection weight (0: unsupported width)
int launch_pack_proj(const float* W, int D, bf16_t* dst, hipStream_t s, int fmt = 0);
bool mlp_fused_supported(int D, int F, int planes);
long mlp_fused_pack_elems(int D, int F);        // bf16 elements of the packed copy (0: unsupported shape)
int launch_pack_mlp(const float* W1, const float* W2, int D, int F, bf16_t* dst, hipStream_t s, int fmt = 0);
int launch_mlp_fused2(const MlpFusedParams& p, hipStream_t s);     // role-split wave pairs, two waves per SIMD (mlp_fused2.hip)

// Attention output projection + fused MLP of one block on hi + lo operand planes (mlp_fused3.hip): X += ctx . Wproj^T + bproj (when ctx is
// given), then X += fc2(gelu(fc1(LayerNorm(X)))), in place, one launch, D = 384
struct MlpFused3Params {
    float* X;                                   // residual stream [M, 384] fp32
    float eps;                                  // LayerNorm epsilon (norm2; norm1 of the next block in the qkv tail)
    const bf16_t* Wp;                           // launch_pack_mlp3: proj + fc1 + fc2 as 108 slots of (lo, hi) fragment pairs in stream order (+ the 36
                                                // slots of the next block's Wqkv), then the folded biases -- the LayerNorms' weights and biases ride in it
    const float* b2;                            // [384]
    int M;
    const bf16_t* ctx; long ctx_plane;          // attention output planes [2][M][384] (hi, then lo at + ctx_plane elements); null = MLP only
    const float* bproj;
    int fmt;                                    // operand format of ctx, the packed weights and everything in between (FMT_BF16 / FMT_FP16)
    // optional (with ctx; q != null): LayerNorm1 + the qkv projection of the NEXT block at the end of the same launch (Wp packed with Wqkv_next);
    // Q pre-scaled by qscale
    bf16_t* q; bf16_t* k; bf16_t* v; long qkv_plane;      // each [2][B, heads, npad, 64] (lo plane at + qkv_plane elements; rows >= ntok never written)
    int ntok, npad, heads; float qscale;
    int v_bf16;                                 // fmt == FMT_FP16: V as bf16 hi + lo planes (GemmParams::v_bf16)
};
// what launch_pack_mlp3 reads: the fp32 parameters of a block's second half (and of the next block's first linear)
struct MlpFused3Weights {
    const float* Wproj; const float* W1; const float* b1; const float* W2;
    const float* gamma2; const float* beta2;                                         // norm2 of this block: folded into W1 / b1
    const float* Wqkv_next; const float* bqkv_next; const float* gamma1_next; const float* beta1_next;      // nullable together: the qkv tail
};
bool mlp_fused3_supported(int D, int F, int planes);
long mlp_fused3_pack_elems(int D, int F);       // 16-bit elements of the packed copy, qkv tail slots and folded biases included (0: unsupported shape)
int launch_pack_mlp3(const MlpFused3Weights& w, int D, int F, bf16_t* dst, hipStream_t s, int fmt);
int launch_mlp_fused3(const MlpFused3Params& p, hipStream_t s);
// The same launch on ONE operand plane, one wave per SIMD (mlp_fused4.hip; MlpFused3Params without the plane strides; the qkv tail writes one plane
// each, V as bf16): Wp = launch_pack_mlp4's 54 (+ 18: the next block's Wqkv) slots of 48 fragments (Wproj may be null for an MLP-only copy: its six
// slots are zero and never read), the LayerNorms folded in as in launch_pack_mlp3, then the folded biases
bool mlp_fused4_supported(int D, int F, int planes);
long mlp_fused4_pack_elems(int D, int F);       // 16-bit elements of the packed copy, tail slots and folded biases included (0: unsupported shape)
int launch_pack_mlp4(const MlpFused3Weights& w, int D, int F, bf16_t* dst, hipStream_t s, int fmt);
int launch_mlp_fused4(const MlpFused3Params& p, hipStream_t s);

// tuning knobs (dinoseg_set_option: the table in api.hip).  A handle's forward reads them as it runs (forward.hip: plan_block), except four that decide which packed
// copies dinoseg_refresh_weights lays out (every load_state_dict, in-place weight update and fine-tune step refreshes):
// fp16_patch_planes and gemm_rs_ln are refresh-only, mlp_fused4 and the gemm_rs bits switch-off-only (below).  Every forward
// equals, bit for bit, the same forward of a fresh handle whose first refresh saw fp16_patch_planes and gemm_rs_ln at their values
// of the last refresh, mlp_fused4 and gemm_rs at (value at the last refresh) AND (current value), and every other option at its
// current value (tests/test_refresh_routes_gpu.py).  A refresh that
// changes which copies exist, or their offsets or sizes, bumps dinoseg_state_generation; one that keeps them does not.
struct Options {
    int gemm_ln = 1;         // qkv / fc1 through the LayerNorm-fused kernel (gemm_ln.hip): 0 never, 2 wherever it applies, 1 = by measurement (forward.hip: plan_block)
    int gemm_big = 1;        // use gemm_big.hip where it applies
    int gemm_dbg = 0;        // ablation bits copied into GemmParams::dbg (wrong results; timing only)
    int attn_dbg = 0;        // same for AttnParams::dbg (bits 0-2: attention.hip ablations, wrong results); bit 3: attention_za's one-block body for the
                             // ragged last q-tile OFF (an A/B switch, results unchanged)
    int mlp_fused = 1;       // the MLP half of a block as one launch (mlp_fused2.hip): 0 never, 1 for >= mlp_fused_min_rows rows, 2 wherever supported
    int mlp_fused_min_rows = 12000;      // (4 frames @480: +3 %; 6 frames: +18 % with the projection inside; 2 frames: even)
    int mlp_fused3_min_rows = 10000;     // hi + lo planes (mlp_fused3.hip): 3 frames @480 +10 %, 4: +16 %, 8: +19 %; 2 frames -17 %, 1: -36 % (tools/m3_thresh.sh)
    int mlp_stagger = 0;     // experiment: > 0 = one workgroup per CU, those with one item fewer start up to this many x 3.9 us late
    int mlp_grid = 0;        // workgroups of the fused MLP launch (0 = the fewest that need no extra round: mlp_fused2.hip)
    int qkv_fused = 0;       // 1: ... and LayerNorm1 + qkv of the NEXT block at its end (blocks 1.. then have no LN+qkv launch); measured
                             // +1 % on one stream, +-0 on two: the tail is bound by the same HBM write burst as the launch it replaces
    int mlp_fused4 = 0;      // one-plane modes: 1 = the fused projection + MLP launch with ONE wave per SIMD (mlp_fused4.hip) instead of mlp_fused2.hip's two
                             // (no qkv tail: only while qkv_fused is 0).  The launch 354-360 against 359-371 us, the headline +0.3-0.4 % (profiles/r06_mlp_fused4.md):
                             // inside the boxes' spread, so the older kernel stays the default.
                             // Switch-off-only: read when the weights are packed (dinoseg_refresh_weights: its copies exist only if it was
                             // on then) and at every forward; the route runs while it was on at the last refresh AND is on now -- setting it
                             // between two refreshes can switch the route off, never on
    int qkv_fused4 = 1;      // ... with LayerNorm1 + qkv of the NEXT block at its end (as qkv_fused3 for the hi + lo launch)
    int qkv_fused3 = 1;      // hi + lo planes (mlp_fused3.hip): 1 = LayerNorm1 + qkv of the NEXT block at the end of the fused projection + MLP launch
    int gemm_rs = 3;         // the row-stationary streaming GEMMs (gemm_rs.hip; embed_dim 768, one plane, >= gemm_rs_min_rows rows), a bit per linear:
                             // 1 = mlp.fc1 (its GELU epilogue rides in the MFMA gaps: 329 against gemm_big's 357 us at 57 616 rows), 2 = attn.qkv
                             // (-3 % on the launch), 4 = attn.proj and mlp.fc2 (slower); 0 = never.  configs.vitb on one box: 850 / 865 / 873
                             // frames/s with 0 / 1 / 3 (profiles/r06_gemm_rs.md).  Switch-off-only, bit by bit, like mlp_fused4: a linear gets its
                             // copy at refresh only if its bit is set and gemm_rs.hip takes its shape (else LayerNorm + the regular GEMM), and
                             // runs on it while the bit was set at the last refresh AND is set at the forward
    int gemm_rs_min_rows = 24000;
    int gemm_rs_ln = 1;      // ... with the LayerNorm in front of qkv / fc1 computed in the kernel's prologue (no LayerNorm launch, no 16-bit A round trip).
                             // Refresh-only: the copy carries the LayerNorm or not as this was at the last refresh; setting it in between
                             // changes nothing until the next refresh
    int proj_fused = 1;      // 1: the block's attention output projection runs inside the fused MLP launch
    int streams = 2;         // 2: dinoseg_forward runs a batch of >= split_min frames as two half-batches on two streams (forward.hip)
    int split_min = 8;       // (8 frames @480: +6 %, 12: +16 %, 16: +12 %; 6 frames and fewer: slower split)
    int route_ab = 0;        // A/B switches of dispatch routes that do not change results: bit 0 = 128-row tiles for the residual GEMMs of a small
                             // batch (gemm.hip HALFM off), bit 1 = one wave per row in the LayerNorm backward (train.hip), bit 2 = the weight-
                             // gradient GEMM's split count not rounded to a multiple of 8 (its XCD-aware grid off: train_ws.h tn_slices, gemm_tn.hip)
    int fp16_patch_planes = 1;      // precision fp16: 1 = the patch embedding on one fp16 plane like the rest of the mode (2466 -> 2486 frames/s,
                                    // 0.0263 / 8 flips -> 0.0218 / 5 on the G3 fixture), 2 = on bf16 hi+lo planes (round 4's first build).
                                    // Refresh-only: read when the weights are packed (the next dinoseg_refresh_weights), never in between
    int op_v_bf16 = 0;       // dinoseg_op_attention: AttnParams::v_bf16 (tests)
    int op_fmt = 0;          // operand format (FMT_BF16 / FMT_FP16) of the single-plane stand-alone ops (dinoseg_op_*: tests, tools); a
                             // handle's forward follows its own precision instead
    int deterministic = 0;   // 1: the fine-tune step sums the loss, the bias and the LayerNorm gamma / beta gradients in a FIXED order (per-block
                             // partials into a scratch area + one ordered pass; the side stream's gemm_tn launches have their own region)
                             // instead of fp32 atomics: two runs from the same state are bit-identical (tests/test_train_gpu.py)
    int train_streams = 2;   // 2: backward runs the weight-gradient GEMMs of the blocks on the handle's side stream (backward.hip)
    int splitk_tiles = 512;  // weight-gradient GEMMs: partial 128x128 tiles per launch (<= 768, the workspace holds that many)
    int attn_variant = 11 | 1024 | 65536;
                             // bit 0: overflow check on the row sums instead of a per-tile row maximum; bit 1: idle waves skip the
                             // tile work; bit 2: unused (round 1-3's software-pipelined kernel, removed); bit 3 (bf16 mode):
                             // the zero-reference kernel, four waves per SIMD (attention_z.hip); bit 9: never split the keys of a
                             // q-tile over wave groups (attn_fwd_zs_kernel, the small-grid form: A/B and tests);
                             // bit 10 (round 5, default): grids of four rounds and more run the tile loop as a hand-scheduled assembly
                             // pipeline (attention_za.hip: bit-identical outputs), bit 16: with 64 queries per wave at two waves per
                             // SIMD; bit 11: that kernel at every grid size, bit 12: attention_z.hip's 256-query workgroups at every
                             // grid size (tests); bit 6: never the 256-query workgroups (nor attention_za.hip)
};
Options& options();

// Flash-style fused multi-head attention, head_dim 64.
struct AttnParams {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; long qkv_plane;   // as written by EPI_QKV: [planes][B,H,npad,64]
    bf16_t* ctx; long ctx_plane;       // [planes][B*ntok][heads*64]
    float* lse;                        // optional [B,H,ntok] log2-domain log-sum-exp (for backward), may be null
    int B, heads, ntok, npad, planes;
    int dbg;                           // timing-only ablations: bit0 skip max/exp, bit1 skip steady-state loads, bit2 skip PV
    int shared_gpu;                    // hint: another stream's kernels run beside this launch (the split forward): prefer wide workgroups
    int dispatch_B;                    // > 0: choices that change the arithmetic (the key split of small grids) are made for this batch: the
                                       // half-batches of a split forward run what the whole call would (as GemmParams::dispatch_rows)
    int v_bf16;                        // hi + lo planes with fmt == FMT_FP16: V arrives as bf16 hi + lo planes (GemmParams::v_bf16) -- the
                                       // zero-reference kernels (attention_z.hip / attention_za.hip: probabilities and V bf16, Q / K / ctx
                                       // fp16); 0: every plane fp16, the reference-based kernel of attention.hip
    int fmt;                           // FMT_FP16, one plane (attention_z.hip): Q, K and ctx are fp16, V and the probabilities stay bf16 (2^S against
                                       // the fixed reference 0 needs bf16's exponent range); hi+lo planes (attention.hip): everything fp16, the
                                       // probabilities bounded by the running reference (<= 2^15)
};
int launch_attention(const AttnParams& p, hipStream_t s);
int launch_attention_z(const AttnParams& p, hipStream_t s);    // zero-reference softmax, <= 128 registers: 4 waves per SIMD (attention_z.hip)
int launch_attention_za(const AttnParams& p, hipStream_t s);
// hi + lo planes: does a forward of `batch` frames (the WHOLE call's batch) run the zero-reference assembly kernel (attention_za.hip, X3)?
// The caller of the qkv GEMM asks too: in the fp16 hi + lo mode that kernel wants V as bf16 planes (GemmParams::v_bf16).
bool attention_x3_za(int batch, int heads, int ntok);   // the same arithmetic, tile loop as a hand-scheduled assembly pipeline (attention_za.hip)

// fp32 [rows, cols] -> bf16 planes [planes][rows_pad][cols_pad], zero padded
int launch_pack_planes(const float* src, int rows, int cols, bf16_t* dst, long plane, int rows_pad, int cols_pad,
                       int planes, hipStream_t s, int fmt = 0);

// LayerNorm over the last dim (D % 128 == 0, D <= 1024). rows of x: [M, D] fp32.
// drop_cls != 0: input row m = b*ntok + t is skipped for t == 0 and written to output row b*(ntok-1) + t-1.
int launch_layernorm(const float* x, const float* gamma, const float* beta, float eps, int M, int D,
                     bf16_t* out, long out_plane, int planes, float* out_f32, int drop_cls, int ntok, hipStream_t s, int fmt = 0);

// Patch gather ("im2col") for the 8x8/stride-8 patch embedding. k index = c*64 + ky*8 + kx.
// kind 0: uint8 HWC frames [B,H,W,3] with the ImageNet normalisation fused; kind 1: fp32 CHW [B,3,H,W] as is.  H, W multiples of 8.
// patch = 16: the 16x16/stride-16 embedding, k index = c*256 + ky*16 + kx, rows 768 wide, H, W multiples of 16.
int launch_patch_gather(const void* x, int kind, int B, int H, int W, const float* mean255, const float* inv_std255,
                        bf16_t* out, long out_plane, int planes, hipStream_t s, int fmt = 0, int patch = 8);

// X[b*ntok + 0, :] = cls[:] + pos[0, :]
int launch_cls_rows(float* X, const float* cls, const float* pos, int B, int ntok, int D, hipStream_t s);

// Bicubic (A=-0.75, align_corners=False, scale_factor rule) resample of the g x g patch pos-embed grid to oh x ow (one scale per axis).
int launch_pos_resample(const float* pos_embed, int g, int D, int oh, int ow, float* out, hipStream_t s);

// Final classifier layer + log_softmax + argmax.  in: bf16 hi/lo planes [2][M][ld]; W fp32 [C][K].  C <= 32 runs head_final_kernel;
// 33 <= C <= HEAD_WIDE_MAX_C runs the wide MFMA kernel on Wp, the classifier packed as hi+lo planes [round_up(C, 32)][ld].
constexpr int HEAD_FINAL_MAX_C = 32, HEAD_WIDE_MAX_C = 256;
int launch_head_final(const bf16_t* in, long in_plane, int ld, int M, int K, const float* W, const float* b, int C,
                      float* logp, int32_t* argmax, hipStream_t s, int fmt = 0, const bf16_t* Wp = nullptr, long w_plane = 0);
// the wide kernel alone (head_wide.hip), any 1 <= C <= HEAD_WIDE_MAX_C; needs ld % 32 == 0
int launch_head_wide(const bf16_t* in, long in_plane, int ld, int M, int K, const bf16_t* Wp, long w_plane, const float* b, int C,
                     float* logp, int32_t* argmax, hipStream_t s, int fmt);

// materialised softmax(q k^T) of one block, fp32 [B,H,ntok,ntok] (get_last_selfattention; visualisation only)
int launch_attn_probs(const bf16_t* q, const bf16_t* k, long plane, int planes, int B, int heads, int ntok, int npad, float* out,
                      hipStream_t s, int fmt = 0);
// cm[gt][pred] += 1 over n patches (int64 [C,C], accumulates)
int launch_cls_mask_attn(const bf16_t* q, const bf16_t* k, const bf16_t* v, long plane, int planes, int heads, int ntok, int npad,
                         const float* mask, int n_masks, bf16_t* ctx, long ctx_plane, float* probs, hipStream_t s, int fmt = 0);
// CLS attention maps at pixel resolution (cls_attention.hip; the rule: include/dinoseg.h, dinoseg_op_cls_attention): the CLS query row
// of softmax(q k^T) over all ntok = hp*wp + 1 keys, its patch part enlarged to OH x OW by nearest neighbour -> attn_out fp32 and / or
// keep_out uint8 (the cumulative-mass threshold) [B, heads, OH, OW].  q, k as launch_attn_probs reads them.  One launch, one workgroup
// per (frame, head), no atomics, no scratch.  cls_attention_check: the host-side refusals of the shape alone (-1 and a message
// starting with `who`); cls_attention_max_tokens: the most tokens whose scores fit the LDS of one workgroup.
int cls_attention_max_tokens();
int cls_attention_check(const char* who, int B, int heads, int ntok, int hp, int wp, int OH, int OW, bool want_keep, float threshold);
int launch_cls_attention(const bf16_t* q, const bf16_t* k, long plane, int planes, int B, int heads, int ntok, int npad, int hp, int wp,
                         int OH, int OW, float threshold, float* attn_out, uint8_t* keep_out, hipStream_t s, int fmt = 0);
int launch_broadcast_row0(float* X, int D, int n, hipStream_t s);
int launch_resize_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, hipStream_t s);
int launch_confusion(const int32_t* pred, const int64_t* gt, long n, int C, int64_t* cm, hipStream_t s);
// Bilinear upsample (F.interpolate, align_corners=False, exact integer coordinates) of the head's log-probs logp [B, hp*wp, C] to
// OH x OW (>= hp x wp) fused with the first-maximum argmax (upsample.hip): labels int32 [B, OH, OW] and / or dense fp32 [B, C, OH, OW]
// its shape check alone (-1 and a message starting with `who`): sizes positive, 1 <= C <= 256, OH >= hp, OW >= wp, the integer ranges
int upsample_check_shape(const char* who, int B, int hp, int wp, int C, int OH, int OW);
int launch_upsample_argmax(const float* logp, int B, int hp, int wp, int C, int OH, int OW, int32_t* labels, float* dense, hipStream_t s);
// Image-guided pixel-resolution output (upsample_guided.hip; the rule: include/dinoseg.h, dinoseg_op_upsample_guided): joint bilateral
// upsampling of logp [B, hp*wp, C] to OH x OW guided by the uint8 frame guide [B, OH, OW, 3].  launch_guide_cells: the rounded mean
// colour of every cell's pixels, packed uint32 [B, hp, wp].  launch_upsample_guided: per pixel the weighted mean of the (2 radius + 1)^2
// cells around its own, labels int32 [B, OH, OW] = its first maximum and / or dense fp32 [B, C, OH, OW].  One launch each, no atomics.
// The checks are the host-side refusals alone (-1 and a message starting with `who`, as the launches' own); upsample_guided_check also
// plans the launch.
struct UpGuidedPlan {
    int tiles_x, tiles_y, CC, stride, kw_log2, col_words;
    size_t lds_bytes;
    float a_s, a_r;
};
int guide_cells_check(const char* who, int B, int hp, int wp, int OH, int OW);
int launch_guide_cells(const char* who, const uint8_t* guide, int B, int OH, int OW, int hp, int wp, uint32_t* cells, hipStream_t s);
int upsample_guided_check(const char* who, int B, int hp, int wp, int C, int OH, int OW, int radius, double sigma_spatial, double sigma_range,
                          UpGuidedPlan* plan);
int launch_upsample_guided(const char* who, const float* logp, const uint8_t* guide, const uint32_t* cells, int B, int hp, int wp, int C, int OH, int OW,
                           int radius, double sigma_spatial, double sigma_range, int32_t* labels, float* dense, hipStream_t s);
// Image-guided iterative label refinement (refine.hip; the rule: include/dinoseg.h, dinoseg_op_refine_iterate): PAMR passes over a state
// [B, C, OH, OW] that ping-pongs between the halves of scratch [2][B, C, OH, OW], guided by the uint8 frame guide [B, OH, OW, 3].
// launch_refine_seed writes half 0 from int32 labels [B, OH, OW] (one-hot) or fp32 scores [B, hp*wp, C] (bilinear enlargement, then
// softmax(gain v)); launch_refine_iterate runs `iters` passes, one launch each, and writes labels int32 [B, OH, OW] and / or the final
// state dense fp32 [B, C, OH, OW].  No atomics.  The checks are the host-side refusals alone (-1 and a message starting with `who`);
// refine_iterate_check also plans the launch.
constexpr int REFINE_SEED_LABELS = 0, REFINE_SEED_SCORES = 1;
constexpr int REFINE_MAX_C = 256, REFINE_MAX_DIL = 6, REFINE_MAX_DILATION = 24, REFINE_MAX_ITERS = 64, REFINE_MAX_SIDE = 1 << 14;
struct RefinePlan {
    int tiles_x, tiles_y, CC, plane_words;
    size_t lds_bytes;
    float k;
};
long long refine_scratch_bytes(int B, int C, int OH, int OW);
int refine_seed_check(const char* who, int kind, int B, int C, int OH, int OW, int hp, int wp, double gain);
int launch_refine_seed(const char* who, const void* seed, int kind, int B, int C, int OH, int OW, int hp, int wp, double gain, void* scratch,
                       hipStream_t s);
int refine_iterate_check(const char* who, int B, int C, int OH, int OW, const int32_t* dilations, int n_dil, double sigma, int iters,
                         RefinePlan* plan);
int launch_refine_iterate(const char* who, const uint8_t* guide, void* scratch, int B, int C, int OH, int OW, const int32_t* dilations,
                          int n_dil, double sigma, int iters, int32_t* labels, float* dense, hipStream_t s);
// Pixel-resolution training loss (upsample_loss.hip): loss = F.cross_entropy(that upsample of logp, labels int64 [B, OH, OW]) with the
// mean over the valid pixels (0 <= label < C; ignore_index and -100 skipped, anything else skipped and flags[0] |= 1), and dlogp
// [B, hp*wp, C] = d loss / d logp (nullable: loss only), without a [B, C, OH, OW] tensor.  dlogp is a gather in a fixed order (no
// floating-point atomics); the loss sum uses atomics, or under option deterministic per-tile partials + launch_det_finalize.
// scratch: upsample_nll_scratch_bytes (<= 8 bytes per pixel + 64 KiB).  upsample_nll_check: the host-side refusals alone.
long long upsample_nll_scratch_bytes(int B, int hp, int wp, int C, int OH, int OW);
int upsample_nll_check(const char* who, int B, int hp, int wp, int C, int OH, int OW, int ignore_index);
int launch_upsample_nll(const float* logp, int B, int hp, int wp, int C, int OH, int OW, const int64_t* labels, int ignore_index,
                        float* loss, float* dlogp, float* n_valid, int* flags, void* scratch, hipStream_t s);
// Multi-scale + flip ensemble at pixel resolution (upsample_ensemble.hip): per pixel the mean over K views of softmax_c(that upsample
// of view k's log-probs logp_k [B, hp_k*wp_k, C], the grid mirrored horizontally first when flip_k), in view order in fp32; labels int32
// [B, OH, OW] = its first maximum, conf fp32 [B, OH, OW] = that maximum, probs fp32 [B, C, OH, OW] = the mean itself (each nullable, at
// least one).  One launch, no atomics, no [B, C, OH, OW] transient; scratch: upsample_ensemble_scratch_bytes (4 K bytes per pixel).
// The view table travels to the kernel by value.  upsample_ensemble_check: the host-side refusals alone (1 <= K <= 12, non-null views,
// flip 0 / 1, upsample_check_shape per view, the summed footprints of a tile within the LDS).
constexpr int UPE_MAX_VIEWS = 12;
struct UpEnsView {
    const float* logp;
    int hp, wp, flip, pad_;
};
struct UpEnsViews {
    UpEnsView v[UPE_MAX_VIEWS];
};
long long upsample_ensemble_scratch_bytes(int K, int B, int OH, int OW);
int upsample_ensemble_check(const char* who, const UpEnsViews& views, int K, int B, int C, int OH, int OW);
int launch_upsample_ensemble(const UpEnsViews& views, int K, int B, int C, int OH, int OW, int32_t* labels, float* conf, float* probs,
                             void* scratch, hipStream_t s);

// Sliding-window inference at pixel resolution (windows.hip).  The window rule per axis: g = max(L - w + s - 1, 0) / s + 1 windows at
// o[i] = max(min(i s + w, L) - w, 0); windows of a frame row-major over (gy, gx), of a batch frame-major.
// window_origins: the rule on the host (out == null with cap == 0 asks for g alone); -1 for w > L, s < 1 or too little room.
// launch_crop_windows: windows [first, first + count) of x (kind 0: uint8 [B,H,W,3], 1: fp32 [B,3,H,W]) -> a contiguous batch of the
// same kind ([count, wh, ww, 3] / [count, 3, wh, ww]; ww % 8 == 0, out 16-byte aligned), one launch.
// launch_window_merge: logp fp32 [B gh gw, (wh/patch)(ww/patch), C] -> per pixel the mean over the windows that contain it of the
// bilinear upsample of each window's grid to (wh, ww) (upsample.hip's coordinates and arithmetic), fp32 adds in window order, IEEE
// division by the count: labels int32 [B,H,W] = its first maximum, dense fp32 [B,C,H,W] = the mean (each nullable, at least one).
// One launch, no atomics, no scratch.  window_merge_check: the host-side refusals of the shape alone (C, patch, window / stride
// values, more than 4 windows over a pixel row or column, integer ranges, the LDS plan).
int window_origins(int L, int win, int stride, int32_t* out, int cap);
int launch_crop_windows(const void* x, int kind, int B, int H, int W, int win_h, int win_w, int stride_h, int stride_w, int first,
                        int count, void* out, hipStream_t s);
int window_merge_check(const char* who, int B, int H, int W, int patch, int win_h, int win_w, int stride_h, int stride_w, int C);
int launch_window_merge(const float* logp, int B, int H, int W, int patch, int win_h, int win_w, int stride_h, int stride_w, int C,
                        int32_t* labels, float* dense, hipStream_t s);

// Augmentation of fine-tuning frames and masks (augment.hip; the rule: include/dinoseg.h, dinoseg_op_augment).  frames uint8 [B,H,W,3],
// masks uint8 / int64 [B,H,W] (nullable, with both label outputs), table a DEVICE array of B records -> out in out_kind (uint8
// [B,OH,OW,3] / normalised fp32 [B,3,OH,OW]), int64 pixel labels [B,OH,OW] and patch labels [B,(OH/patch)(OW/patch)] (each nullable).
// max_radius == 0: one launch (warp + colour + labels + conversion); otherwise the warp launch writes the fp32 planar scratch
// [B,3,OH,OW] and the blur launch (tile + halo in LDS, both passes without HBM in between) writes out.  Every refusal is on the host.
int launch_augment(const uint8_t* frames, const void* masks, int mask_kind, int B, int H, int W, const dinoseg_augment_frame* table,
                   int max_radius, int OH, int OW, int out_kind, void* out, int64_t* pixel_labels, int64_t* patch_labels, int patch,
                   float* scratch, hipStream_t s);

// Video label propagation from patch features (propagate.hip; the rule: include/dinoseg.h, dinoseg_op_propagate).
// launch_normalize_tokens: tokens fp32 [B, 1 + n, D] -> unit rows times 2^10 as fp16 hi + lo planes [B][2][n][D], the CLS row skipped.
// launch_label_cells: integer pixel labels [OH, OW] (kind 0 uint8, 1 int64) -> class shares per cell, fp32 [n, C].
// launch_propagate: one target frame from n_ctx <= 16 context frames (host arrays of device pointers, by value to the kernels): the
// scores launch (one workgroup per query tile and context frame, per-query lists of k in LDS) and the merge launch (weights, gathers).
// scratch: propagate_scratch_bytes (8 n_ctx n k; -1 for refusable arguments).  No atomics; every refusal is on the host.
// The top-k selection of both launches -- lists, total order, 4-way merge, wave select, weights, topk outputs, scratch layout, the
// checks of D, C, k and tau -- is select_common.h, one copy for this operator and launch_knn_labels.
int launch_normalize_tokens(const float* tokens, int B, int n, int D, void* planes, hipStream_t s);
int launch_label_cells(const void* labels, int mask_kind, int OH, int OW, int hp, int wp, int C, float* seg, hipStream_t s);
long long propagate_scratch_bytes(int hp, int wp, int n_ctx, int k);
int launch_propagate(const void* target_planes, const void* const* ctx_planes, const float* const* ctx_segs, int n_ctx, int hp, int wp,
                     int D, int C, int radius, int k, double tau, float* seg_out, int32_t* topk_idx, float* topk_w, void* scratch,
                     hipStream_t s);

// Few-shot segmentation: k-NN label retrieval from a flat bank of labelled patch features (knn.hip; the rule: include/dinoseg.h,
// dinoseg_op_knn_labels).  Queries are the planes of launch_normalize_tokens for B frames of n cells; the bank is planes
// [2][bank_rows][D] with M live rows and soft fp32 [bank_rows, C] (kind 0) or hard uint8 [bank_rows] (kind 1) labels.
// launch_knn_labels: the scores launch (one workgroup per 64 queries and bank range, per-query lists of k in LDS) and the merge launch
// (the ranges' lists, weights, gathers), the selection being select_common.h's.  knn_splits: the library's number of ranges;
// knn_scratch_bytes: 8 S N k (splits 0 = the library's choice); both host only, -1 for refusable arguments.  No atomics; every
// refusal is on the host.
int knn_splits(int N, int M, int k);
long long knn_scratch_bytes(int N, int M, int k, int splits);
int launch_knn_labels(const void* query_planes, int B, int n, const void* bank_planes, long long M, long long bank_rows,
                      const void* bank_labels, int label_kind, int D, int C, int k, double tau, int splits, float* seg_out,
                      int32_t* topk_idx, float* topk_w, void* scratch, hipStream_t s);

// PCA of patch features (pca.hip; the rules: include/dinoseg.h, dinoseg_op_token_moments).  Tokens are fp32 [B, 1 + n, D] as
// dinoseg_features_hw writes them, the CLS row skipped.  launch_token_moments: the partials launch (one wave per (tile pair or sum
// tile, range) on the fp32-input MFMA) and the finalising launch (ranges added in order in fp64, the mirror written, the accumulators
// added to).  pca_ranges: R(B n, D); pca_scratch_bytes: 4 R (4096 pairs + D + 1), host only, -1 for refusable arguments.
// launch_pca_project: centred rows times basis^T into the token layout [B, 1 + n, q], the CLS rows zero.  launch_pca_colour: three
// components -> scaled, enlarged with the family's tile walk, clamped, uint8 [B, OH, OW, 3].  No atomics; every refusal is on the host.
int pca_ranges(long long N, int D);
long long pca_scratch_bytes(int B, int n, int D);
int launch_token_moments(const float* tokens, const uint8_t* keep, int B, int n, int D, const float* shift, double* sum, double* outer,
                         long long* count, void* scratch, hipStream_t s);
int launch_pca_project(const float* tokens, int B, int n, int D, const float* mean, const float* basis, const float* scale, int q, float* out,
                       hipStream_t s);
int launch_pca_colour(const float* comps, int B, int hp, int wp, int q, const float* lo, const float* inv, const uint8_t* keep, int OH,
                      int OW, uint8_t* rgb, hipStream_t s);

// Spherical k-means over patch features (kmeans.hip; the rule: include/dinoseg.h, dinoseg_op_kmeans_assign).  Points are the planes of
// launch_normalize_tokens for B frames of n cells, clustered jointly; centroids are fp32 [K, D] rows plus planes [2][K][D].
// launch_kmeans_init: fp32 rows -> (unit) fp32 rows and their planes.  launch_kmeans_assign: the assign launch (scores on MFMAs, the
// running pair in registers, scores [N, K] on request) and, when a record slot is given, the one-workgroup records launch.
// launch_kmeans_update: the partial launch (one workgroup per (range, cluster), members gathered in index order) and the finalize launch
// (ranges in range order, fp64 norm, row and planes).  scratch: kmeans_scratch_bytes (-1 for refusable arguments).  No atomics.
long long kmeans_scratch_bytes(int B, int n, int K, int D);
int launch_kmeans_init(const float* rows, int K, int D, int normalize, float* centroids, void* planes, hipStream_t s);
int launch_kmeans_assign(const void* points, int B, int n, const void* centroid_planes, int K, int D, const int32_t* prev_assign,
                         int32_t* assign, float* best, float* scores, float* objective, int32_t* moved, void* scratch, hipStream_t s);
int launch_kmeans_update(const void* points, int B, int n, const int32_t* assign, const float* prev_centroids, const void* prev_planes,
                         int K, int D, float* centroids, void* planes, int32_t* counts, void* scratch, hipStream_t s);

// Normalized cut on a 1-bit patch graph (ncut.hip; the rule: include/dinoseg.h, dinoseg_op_ncut_graph).  Points are the planes of
// launch_normalize_tokens; every frame is its own graph.  launch_ncut_graph: one workgroup per (frame, 64 queries), three MFMA
// accumulators per tile, ballots -> the row-major bit graph [B][n][ceil(n / 64)] uint64 and the exact degree.  launch_ncut_iterate: one
// workgroup of 1024 threads per frame, every pass in one launch, the vectors in LDS -> z_out, rho [B][iters], fg, eigvec, margin
// (optional), seed_cell.  ncut_graph_bytes: -1 for refusable arguments.  ncut_max_cells: what the vectors leave of the LDS.  No atomics.
long long ncut_graph_bytes(int B, int n);
int ncut_max_cells();
int launch_ncut_graph(const void* planes, int B, int n, int D, double tau, void* graph, int32_t* degree, hipStream_t s);
int launch_ncut_iterate(const void* graph, const int32_t* degree, int B, int n, double eps, const float* z_in, int iters, float* z_out,
                        float* rho, uint8_t* fg, float* eigvec, float* margin, int32_t* seed_cell, hipStream_t s);
// The same rule and the same bits with a frame's rows dealt to many workgroups (ncut_split.hip; the addendum in include/dinoseg.h):
// one launch per pass ordered by the stream alone, xv the only vector in LDS, z / y / r / u in a scratch of ncut_split_scratch_bytes.
// launch_ncut_graph_split (ncut.hip) is launch_ncut_graph's kernel under the split cell limit.
int ncut_split_max_cells();
long long ncut_split_graph_bytes(int B, int n);
long long ncut_split_scratch_bytes(int B, int n);
int launch_ncut_graph_split(const void* planes, int B, int n, int D, double tau, void* graph, int32_t* degree, hipStream_t s);
int launch_ncut_iterate_split(const void* graph, const int32_t* degree, int B, int n, double eps, const float* z_in, int iters,
                              int rows_per_group, float* z_out, float* rho, uint8_t* fg, float* eigvec, float* margin, int32_t* seed_cell,
                              void* scratch, hipStream_t s);

// Connected components of label maps and their object table (components.hip; the rule: include/dinoseg.h, dinoseg_op_components): a
// union-find per 64 x 32 tile in LDS, unions across tile edges by integer atomicMin, roots and per-segment root masks, a prefix sum per
// frame, ids and the table.  Five plain launches ordered by the stream.  components_scratch_bytes: -1 for refusable arguments.
long long components_scratch_bytes(int B, int H, int W);
int launch_components(const int32_t* labels, int B, int H, int W, int connectivity, int ignore, int max_objects, int32_t* ids,
                      int32_t* count, int32_t* first, int32_t* label, int32_t* area, int32_t* box, int32_t* status, void* scratch,
                      hipStream_t s);

// Multi-object discovery: K rounds of the split cut with the found object painted out between rounds (maskcut.hip; the rule:
// include/dinoseg.h, dinoseg_op_maskcut).  launch_ncut_mask: graph &= alive in place and the exact degree, one wave per row.
// launch_maskcut_select: the seed's component -> cells, found, area, box, the score channel t + 1, alive &= ~cells; one workgroup per
// frame.  launch_maskcut: the K rounds -- mask, launch_ncut_iterate_split, candidates, launch_components, select -- on the stream; it
// destroys the graph.  maskcut_scratch_bytes: -1 for refusable arguments.
long long maskcut_scratch_bytes(int B, int hp, int wp, int K);
int launch_ncut_mask(void* graph, int32_t* degree, const void* alive, int B, int n, hipStream_t s);
int launch_maskcut_select(const int32_t* ids, const uint8_t* fg, const float* margin, const int32_t* seed_cell, void* alive, int B, int hp,
                          int wp, int K, int t, uint8_t* cells, uint8_t* found, int32_t* area, int32_t* box, float* score, hipStream_t s);
int launch_maskcut(void* graph, int32_t* degree, int B, int hp, int wp, double eps, const float* z_start, int iters, int rows_per_group,
                   int connectivity, int K, uint8_t* cells, uint8_t* found, int32_t* area, int32_t* box, float* score, int32_t* count,
                   uint8_t* fg, float* margin, float* eigvec, int32_t* seed_cell, float* rho, void* scratch, hipStream_t s);

// ---- fine-tune step (train.hip, attention_bwd.hip) ----
struct AttnBwdParams {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; long qkv_plane;   // forward operands [planes][B,H,npad,64]
    const bf16_t* dO; const bf16_t* O; long dO_plane;                      // d ctx and ctx, [planes][B*ntok][H*64]
    const float* lse;                                                      // forward log2-domain LSE [B,H,ntok]
    float* neg_lse; float* neg_delta;                                      // scratch [B,H,npad] each
    bf16_t* dqkv; long dqkv_plane;                                         // out: [planes][B*ntok][3*H*64]
    int B, heads, ntok, npad, planes;
};
int launch_attention_bwd(const AttnBwdParams& p, hipStream_t s);

int launch_transpose_planes(const float* src_f32, const bf16_t* src_pl, long src_plane, int ld_src, int M, int C,
                            bf16_t* T, long t_plane, int c_pad, int m_pad, bf16_t* Nout, long n_plane, int ldn,
                            float* colsum, int planes, int drop_cls, int ntok, hipStream_t s, int det_region = 0);
                            // det_region (deterministic mode, colsum given): 0 = the caller's stream, 1 = the weight-gradient side stream,
                            // whose partial sums go to its own part of the scratch (as TnParams::det_region)
// labels != null: F.nll_loss (mean over rows whose label is not -100) + d logits; labels == null: d logits from the caller's dlogp
int launch_nll_loss_grad(const float* logp, const int64_t* labels, const float* dlogp, int M, int C, float* acc, int* flags,
                         float* loss, bf16_t* dz, long dz_plane, int ldz, hipStream_t s);
// dxp / colsum (optional): the final dx rows as bf16 planes [planes][M][D] and their column sums (train.hip)
int launch_layernorm_bwd(const float* dy, const float* x, const float* gamma, float eps, int M, int D, float* dx,
                         int accumulate, float* dgamma, float* dbeta, int drop_cls, int ntok, hipStream_t s,
                         bf16_t* dxp = nullptr, long dxp_plane = 0, int planes = 1, float* colsum = nullptr);
// Weight gradient on row-major operands (gemm_tn.hip): part[slice][n][k] = sum over the slice's batch rows of Y[m][n] X[m][k]
struct TnParams {
    const bf16_t* Y; long y_plane; int ldy;     // dY planes [planes][M][ldy], columns n < N (N % 128 == 0 not required: rows guarded)
    const bf16_t* X; long x_plane; int ldx;     // layer input planes [planes][M][ldx], columns k < Kc (Kc % 128 == 0)
    int M, N, Kc, planes;
    float* part; int ld_part; long split_stride; int ksplit;
    float* colsum;                              // optional [N]: += column sums of dY over the M rows (the layer's bias gradient)
    float* det; int det_ld;                     // set by launch_gemm_tn in deterministic mode: per-slice partial sums [ksplit][det_ld]
    int det_region;                             // deterministic mode: 0 = the caller's stream, 1 = the weight-gradient side stream (its own part of the scratch)
};
int launch_gemm_tn(const TnParams& p, hipStream_t s);
// Deterministic mode (Options::deterministic): the scratch area the partial sums of the current backward go to (set by
// dinoseg_backward around its launches; nullptr = atomics) and the ordered pass dst[c] += sum_p part[p * ld + c], p ascending.
struct DetScratch { float* ptr; size_t floats; float* tn[2]; size_t tn_floats; };      // tn[r]: gemm_tn's partials, per stream region
DetScratch& det_scratch();
int launch_det_finalize(const float* part, int nparts, int width, int ld, float* dst, hipStream_t s);
int launch_splitk_reduce(const float* part, int ks, long stride, int rows, int ld_part, float* out, int ldo, int cols, hipStream_t s);
int launch_batch_sum_rows(const float* X, int B, int ntok, int D, float* out, hipStream_t s);
int launch_pos_resample_bwd(const float* dpos, int g, int D, int oh, int ow, float* dpe, float* scratch /* g*ow*D floats */, hipStream_t s);
constexpr int MULTI_MAX = 64;       // tensors per multi-tensor launch (table passed as a kernel argument)
int launch_multi_adam(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n, float lr,
                      float b1, float b2, float eps, float wd, int decoupled, int step, float gscale, hipStream_t s);
int launch_multi_zero(int count, float* const* p, const long* n, hipStream_t s);
int launch_adam(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd,
                int decoupled, int step, float gscale, hipStream_t s);
// several pack_planes jobs in ONE launch, plain or transposed (dst[pl][c][r] = src[r][c], planes [planes][cols_pad][rows_pad]: the W^T
// operands of dgrad).  A weight refresh is ~30 of them, each a few microseconds of work behind a launch: the fine-tune step repacks
// every weight after every optimiser step
struct PackJob {
    const float* src; bf16_t* dst; long plane;
    int rows, cols, rows_pad, cols_pad, planes, transposed;
    int fmt = 0;                    // FMT_BF16 / FMT_FP16
};
int launch_multi_pack(const PackJob* jobs, int count, hipStream_t s);

}  // namespace dseg
