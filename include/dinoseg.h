/* dinoseg.h -- C-ABI of libdinoseg_hip.so: the MI355X (gfx950) DINOSeg hot path.
 *
 * Drop-in boundary for the reference's Python model class (reference = sachaMorin/dino, all
 * citations relative to its root).  The reference has no FFI of its own -- its "operator interface"
 * for this path is the DINOSeg module API -- so each entry point names the Python call it replaces.
 * The host-side mirror (dino_amd/dinoseg.py) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions: extern "C", plain pointers and sizes, no torch / C++ types.  Every function returns
 * 0 on success and a negative code on failure (-1 bad argument, -2 HIP runtime error, -3 state error);
 * dinoseg_last_error() returns the message.  All device pointers are caller-owned (PyTorch-ROCm
 * tensors); the library owns only its packed-weight copies and its activation workspace, released by
 * dinoseg_destroy().  Every call is asynchronous on the caller's `stream` (a hipStream_t passed as
 * void*; pass torch.cuda.current_stream().cuda_stream) and performs no host synchronisation, except
 * the lazy workspace (re)allocation on the first call for a larger (B, r).
 * A handle is not re-entrant: one handle per process per GPU.
 */
#ifndef DINOSEG_H
#define DINOSEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dinoseg_handle dinoseg_handle;

/* Precision of the GEMM / attention operands (accumulation is always fp32):
 *   DINOSEG_BF16   : bf16 operands, 1 MFMA per product  (benchmark mode, BASELINE.json "bf16")
 *   DINOSEG_BF16X3 : bf16 hi+lo operand pairs, 3 MFMAs per product (~16 mantissa bits): the parity mode
 *                    that meets "argmax identical, |dlogp| <= 1e-3" against the fp32 reference.
 *   DINOSEG_FP16   : fp16 operands (11 significand bits), 1 MFMA per product at the bf16 rate: the linears and Q.K^T on
 *                    v_mfma_f32_32x32x16_f16; the probabilities and V (the P.V product) stay bf16 -- 2^S against the fixed
 *                    reference 0 needs bf16's exponent range; the head runs split (bf16 hi+lo).
 *                    ~6x closer to the reference than DINOSEG_BF16 at the same speed; inference only (the fine-tune
 *                    entry points refuse it: fp16 gradients would need loss scaling).
 *   DINOSEG_FP16X3 : fp16 hi+lo operand pairs everywhere (patch embedding and head included), 3 MFMAs per product at the
 *                    bf16x3 rate, ~22 significand bits instead of ~16: the parity mode with margin (2x closer to the reference
 *                    than DINOSEG_BF16X3 on the goldens, ~8x on ill-conditioned weights -- outlier channels, sharp heads);
 *                    values beyond +-65504 saturate; inference only. */
enum { DINOSEG_BF16 = 0, DINOSEG_BF16X3 = 1, DINOSEG_FP16 = 2, DINOSEG_FP16X3 = 3 };
enum { DINOSEG_HEAD_LINEAR = 0, DINOSEG_HEAD_MLP = 1 };
enum { DINOSEG_INPUT_U8_HWC = 0,      /* uint8 [B,r,r,3] frames; ImageNet normalisation fused on device   */
       DINOSEG_INPUT_F32_CHW = 1 };   /* fp32  [B,3,r,r] already-normalised tensor (DINOSeg.forward input) */

/* Architecture = the reference ctor arguments that shape the path.
 * DINOSeg.__init__(head, n_blocks, n_classes, backbone='vit')   dt_segmentation/src/pl_torch_modules.py:144-222
 * vit_small / vit_base(patch_size=8)                             dt_segmentation/src/vision_transformer.py:300-311
 *
 * Patch size.  `patch` is 8 or 16, the published DINO sizes (anything else: dinoseg_create returns -1).  Every comment below
 * is written for patch 8; on a patch-16 handle read `patch` wherever it says 8 in a frame size: H and W must be multiples of
 * 16 (else -1 and "Resolution should be a multiple of 16."; a patch-8 handle keeps "... multiple of 8."), hp = H/16, wp = W/16,
 * masks, labels and outputs have (H/16)*(W/16) rows per frame, dino.patch_embed.proj.weight is [D, 3, 16, 16] and, with
 * pos_grid = 14, dino.pos_embed is [1, 197, D] and is returned unresampled for 224 x 224 frames only.
 * Alignment at patch 16: the gather reads frames with 16-byte loads, so the frame pointer x of every entry that takes frames
 * (dinoseg_forward*, dinoseg_features*, dinoseg_last_selfattention*, dinoseg_forward_mask*, dinoseg_train_forward*,
 * dinoseg_train_step*) must be 16-byte aligned -- W % 16 == 0 keeps every row and frame offset aligned behind it; a whole
 * allocation or a slice of whole frames is.  A misaligned pointer is refused (-1), never read.  (Patch 8 reads uint8 frames with
 * 4-byte loads and fp32 frames with 16-byte loads, as before.) */
typedef struct dinoseg_config {
    int32_t embed_dim;    /* 384 (ViT-S) / 768 (ViT-B); multiple of 128                         */
    int32_t num_heads;    /* embed_dim / 64                                                      */
    int32_t n_blocks;     /* transformer blocks kept (dino.blocks[:n_blocks], :177)              */
    int32_t patch;        /* 8 or 16                                                             */
    int32_t mlp_ratio;    /* 4                                                                   */
    int32_t n_classes;    /* 1 .. 256 (33 and up: the wide MFMA head kernel; above 256: rejected)  */
    int32_t head_kind;    /* DINOSEG_HEAD_*  (pl_torch_modules.py:219-222)                       */
    int32_t pos_grid;     /* 28 (patch 8) / 14 (patch 16): stored pos_embed is [1, g*g+1, D]     */
    float   ln_eps;       /* 1e-6 (vision_transformer.py:303)                                    */
    int32_t precision;    /* DINOSEG_BF16 / DINOSEG_BF16X3 / DINOSEG_FP16 / DINOSEG_FP16X3       */
} dinoseg_config;

const char* dinoseg_last_error(void);
int dinoseg_version(void);

/* Replaces DINOSeg.__init__ (pl_torch_modules.py:144-237) minus the network fetch (dt_utils.py:19-29). */
int dinoseg_create(const dinoseg_config* cfg, dinoseg_handle** out);
int dinoseg_destroy(dinoseg_handle* h);

/* Replaces load_state_dict() inside LightningModule.load_from_checkpoint (call sites README.md:31,
 * visualize.py:23): bind one fp32 device tensor by its state_dict key ("dino.blocks.0.attn.qkv.weight",
 * "clf.layer_1.bias", ...).  The pointer is borrowed and must stay valid; shape is checked. */
int dinoseg_bind_weight(dinoseg_handle* h, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim);

/* (Re)build the library's packed bf16 operand planes from the bound fp32 tensors.  Call after binding
 * and after every optimiser step (the role `.to(device)` / optimizer.step() play for torch, README.md:31). */
int dinoseg_refresh_weights(dinoseg_handle* h, void* stream);

/* Replaces DINOSeg.set_resolution (pl_torch_modules.py:270-274) on the device side: bicubic pos-embed
 * resample for an (r/8)x(r/8) grid (vision_transformer.py:202-222), cached per resolution.  r % 8 != 0 -> -1. */
int dinoseg_prepare_resolution(dinoseg_handle* h, int32_t r, void* stream);

/* ---- non-square frames.  The reference takes H x W inputs: prepare_tokens reads `B, nc, w, h = x.shape`, and
 * interpolate_pos_encoding resamples the g x g grid with one scale per axis, scale_factor = ((H/8 + 0.1)/g, (W/8 + 0.1)/g)
 * (vision_transformer.py:202-233); forward_mask takes (1, 3, H, W) frames and (N, H/8, W/8) masks (:250-265).  Each `_hw`
 * entry below is its `r` sibling with the frame given as H rows x W columns (both multiples of 8, else -1 and
 * "Resolution should be a multiple of 8."), hp = H/8, wp = W/8 patches per column / row, n = hp*wp tokens per frame ordered
 * row-major over (hp, wp) (PatchEmbed's flatten(2).transpose(1, 2), :153-157); the `r` entry is H = W = r.  The stored
 * pos_embed is returned untouched only when H == W and hp == g (:205): a side of g on one axis of a rectangle still
 * resamples that axis at g / (g + 0.1).  The position cache holds one (hp, wp) grid. */
int dinoseg_prepare_resolution_hw(dinoseg_handle* h, int32_t H, int32_t W, void* stream);
/* dinoseg_forward at H x W (vision_transformer.py:224-248): logp_out [B*n, n_classes], argmax_out [B*n], tap_out [B*(n+1), D] */
int dinoseg_forward_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, float* logp_out,
                       int32_t* argmax_out, int32_t tap_block, float* tap_out, void* stream);
/* dinoseg_last_selfattention at H x W (vision_transformer.py:273-280): attn_out [B, heads, n+1, n+1] */
int dinoseg_last_selfattention_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W,
                                  float* attn_out, void* stream);
/* CLS attention maps at pixel resolution: what visualize_attention.py draws (attentions[0, :, 0, 1:] of get_last_selfattention,
 * enlarged by the patch size with nearest-neighbour) and what dt_utils.process_attentions thresholds, for B frames, without the
 * [B, heads, n+1, n+1] matrix.  The forward runs up to the last block's LayerNorm1 + qkv; one more launch (dinoseg_op_cls_attention,
 * where the rule is stated in full) writes
 *   attn_out fp32  [B, heads, OH, OW]: the CLS query's softmax probabilities of the n patch keys (softmax over all n + 1 keys),
 *   keep_out uint8 [B, heads, OH, OW]: 1 where the patch belongs to the top `threshold` share of the patches' attention mass,
 * each nullable, not both; any OH >= hp, OW >= wp (OH = hp, OW = wp: the raw grid; OH = H, OW = W: the script's enlarged maps).
 * threshold is read only with keep_out and must lie inside (0, 1).  x of either kind.  Everything the launch would refuse -- and
 * a frame of more than dinoseg_cls_attention_max_tokens() tokens -- is refused before the forward enqueues anything.  Timed under
 * DINOSEG_PROF_ATTN. */
int dinoseg_cls_attention_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t OH, int32_t OW,
                             float threshold, float* attn_out, uint8_t* keep_out, void* stream);
/* the most tokens (hp*wp + 1) of a frame whose scores fit the LDS of the launch's workgroup */
int32_t dinoseg_cls_attention_max_tokens(void);
/* dinoseg_forward_mask at H x W (vision_transformer.py:250-271): cls_mask [n_masks, hp*wp] (the (N, H/8, W/8) masks, row-major),
 * n_masks <= hp*wp; attn_out [heads, n_masks, n+1] */
int dinoseg_forward_mask_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t H, int32_t W, const float* cls_mask,
                            int32_t n_masks, float* emb_out, float* attn_out, void* stream);
/* dinoseg_features at H x W (vision_transformer.py:237-248): tokens_out [B, n+1, embed_dim] */
int dinoseg_features_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t n_blocks,
                        float* tokens_out, void* stream);

/* Replaces DINOSeg.forward (pl_torch_modules.py:239-256) and the argmax of predict() (:294):
 *   x        : B frames at r x r, layout per x_kind
 *   logp_out : fp32 [B*(r/8)^2, n_classes] log-probabilities (may be NULL)
 *   argmax_out: int32 [B*(r/8)^2] first-maximum class index (may be NULL)
 *   tap_block / tap_out: optional debug tap -- tap_block = 0 copies the token matrix after prepare_tokens,
 *   i > 0 after block i, into tap_out (fp32 [B*((r/8)^2+1), embed_dim]); pass -1 / NULL to disable. */
int dinoseg_forward(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, float* logp_out,
                    int32_t* argmax_out, int32_t tap_block, float* tap_out, void* stream);

/* Replaces VisionTransformer.get_last_selfattention (vision_transformer.py:273-280; caller visualize_attention.py:46):
 * the materialised softmax(q k^T / 8) of the LAST block, attn_out fp32 [B, heads, N, N] with N = (r/8)^2 + 1.
 * Visualisation path, not the inference hot path (which never writes the N x N matrix). */
int dinoseg_last_selfattention(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, float* attn_out,
                               void* stream);

/* Replaces VisionTransformer.forward_mask (vision_transformer.py:250-271) and get_last_selfattention(x, cls_mask)
 * (:273-280) for ONE frame x (kinds as dinoseg_forward): every block but the last runs as usual; in the last block the CLS
 * query attends through each of the n_masks masks (its logits MULTIPLIED by the mask, CLS key by 0; Attention.forward
 * :80-107), the CLS residual is repeated once per mask (Block.forward :127-140), then MLP and the final norm.
 * cls_mask: fp32 [n_masks, (r/8)^2] on device, n_masks <= (r/8)^2.  emb_out: fp32 [n_masks, embed_dim] (nullable);
 * attn_out: fp32 [heads, n_masks, (r/8)^2 + 1] masked attention of the last block (nullable; with emb_out NULL the call
 * stops after the attention, like get_last_selfattention). */
int dinoseg_forward_mask(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t r, const float* cls_mask, int32_t n_masks,
                         float* emb_out, float* attn_out, void* stream);

/* Replaces VisionTransformer.forward(x, all=True, intermediate=k) (vision_transformer.py:237-248), i.e. `model.dino(x)`:
 * tokens through n_blocks blocks (0 = all the handle has) and the final LayerNorm, tokens_out fp32 [B, (r/8)^2 + 1, embed_dim]
 * (row 0 of every frame is the CLS token; DINOSeg.forward takes [:, 1:], pl_torch_modules.py:243). */
int dinoseg_features(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, int32_t n_blocks,
                     float* tokens_out, void* stream);

/* Replaces the Resize(r, r) of get_transforms (pl_torch_modules.py:36-38, applied in predict at :291) for frames that are
 * not already r x r: uint8 HWC [sh, sw, 3] -> [dh, dw, 3] on device, restating cv2.resize(INTER_LINEAR)'s fixed-point
 * arithmetic (albumentations 1.1.0 -> opencv 4.5.5, third-party: parity unpinned) so that predict() keeps
 * the frame on the wire as uint8 and resizes it ahead of the patch-embedding gather. */
int dinoseg_op_resize_u8(const uint8_t* src, int32_t sh, int32_t sw, uint8_t* dst, int32_t dh, int32_t dw, void* stream);

/* Confusion matrix for the validation metrics (validation_epoch_end, pl_torch_modules.py:310-332):
 * cm[gt][pred] += 1 over n patches; cm int64 [n_classes, n_classes] on device (zero it first); 1 <= n_classes <= 256. */
int dinoseg_op_confusion(const int32_t* pred, const int64_t* gt, int64_t n, int32_t n_classes, int64_t* cm, void* stream);

/* ---- pixel-resolution output (no reference counterpart: the reference stops at the patch grid and np.kron's the labels,
 * pl_torch_modules.py:294-298).  What ViT segmenters do instead: interpolate the class scores to the pixel grid, then argmax. ----
 *
 * dinoseg_op_upsample_argmax: F.interpolate(logp.view(B, hp, wp, C).permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear",
 * align_corners=False) and its argmax over classes in one launch, without the [B, C, OH, OW] transient.
 *   logp       : fp32 [B, hp*wp, C], the layout the head writes; 1 <= C <= 256
 *   labels_out : int32 [B, OH, OW], the FIRST maximum over classes (nullable); dinoseg_op_confusion takes it as `pred`
 *   dense_out  : fp32 [B, C, OH, OW], the interpolated log-probs in torch's layout (nullable); at least one output is required
 * Coordinates are exact.  Per axis, with input size i, output size o, output index d:  num = max((2d+1) i - o, 0), den = 2 o in
 * integers;  i0 = min(num / den, i-1), i1 = min(i0+1, i-1);  lambda = float(num % den) / float(den), 0 when num / den >= i-1;  the
 * value is a + (b - a) lambda, along x and then along y, in fp32.  Any OH >= hp and OW >= wp (upsampling and identity); a smaller
 * output, a null input, C outside 1..256 and non-positive sizes are refused on the host (-1) before anything is launched. */
int dinoseg_op_upsample_argmax(const float* logp, int32_t B, int32_t hp, int32_t wp, int32_t C, int32_t OH, int32_t OW,
                               int32_t* labels_out, float* dense_out, void* stream);
/* dinoseg_forward_hw (without the debug tap) followed by dinoseg_op_upsample_argmax of its log-probs to OH x OW on the same stream.
 * logp_out [B*n, n_classes] and argmax_out [B*n] are the optional low-res outputs of dinoseg_forward_hw; with logp_out == NULL the
 * log-probs stay in the workspace (no new memory).  labels_out int32 [B, OH, OW], dense_out fp32 [B, n_classes, OH, OW]: at least
 * one.  OH >= H/patch, OW >= W/patch.  Under the two-stream split each half-batch upsamples on its own stream into its slice of the
 * outputs before the join: stream-ordered, capturable, no host synchronisation. */
int dinoseg_forward_dense_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t OH, int32_t OW,
                             float* logp_out, int32_t* argmax_out, int32_t* labels_out, float* dense_out, void* stream);

/* ---- image-guided pixel-resolution output: joint bilateral upsampling (Kopf et al. 2007) of the log-probs, guided by the frame the
 * caller already holds, so that label boundaries follow the image's edges instead of the crossing point between two patch centres ----
 *
 *   logp   : fp32 [B, hp*wp, C], the head's output, finite; 1 <= C <= 256
 *   guide  : uint8 [B, OH, OW, 3] at the OUTPUT's size, OH >= hp, OW >= wp, OH, OW <= 2^20
 *   radius : R in 0..3;  sigma_spatial in [0.5, 16] (cells);  sigma_range in [1e-3, 1e3] (of the full 0..255 range)
 * The constants a_s = log2(e) / (2 sigma_spatial^2) and a_r = log2(e) / (2 (255 sigma_range)^2) are computed on the host in fp64 and
 * rounded once to fp32; the rule is in terms of the rounded values.  All coordinates are integers.
 *
 * 1. Cell colours (dinoseg_op_guide_cells).  Output pixel (y, x) belongs to cell ((y hp) / OH, (x wp) / OW) -- the nearest rule of
 *    dinoseg_op_cls_attention.  Per cell and channel m = (2 sum + n) / (2 n) in integers, sum = the guide summed over the cell's n
 *    pixels: the rounded mean, 0..255.  cells: uint32 [B, hp, wp] packed R | G << 8 | B << 16.  Integer sums, no atomics.
 * 2. Taps.  For output pixel (oy, ox): r0 = (oy hp) / OH, c0 = (ox wp) / OW; the taps are the cells (r0 + dr, c0 + dc), dr, dc = -R .. R,
 *    that lie inside the grid (the others are skipped), in the order dr ascending, then dc ascending.
 * 3. Spatial term.  my = 2 r OH - ((2 oy + 1) hp - OH) for the tap's row r: an integer, NOT clamped -- the pixel's align_corners=False
 *    coordinate against the cell centre, in units of 1 / (2 OH) cells.  dy = float(my) / float(2 OH) (correctly rounded), dx likewise;
 *    s = dy dy + dx dx, each operation rounded to fp32.
 * 4. Range term.  D = the integer squared RGB distance between guide[b, oy, ox] and the tap's cell colour (<= 195 075); Dmin = the
 *    smallest D over the pixel's taps.
 * 5. Weight.  w = exp2(-(s a_s) - float(D - Dmin) a_r), each operation rounded to fp32, exp2 to one ulp.  Subtracting Dmin cancels
 *    in the quotient below and keeps the largest weight at or above 2^-(a_s 2 (R + 1/2)^2) >= 2^-71: the sum never underflows.
 *    For R = 0 the single tap's weight is exactly 1.
 * 6. Value.  acc_k = sum over taps of w L[tap, k] by fmaf in tap order from 0;  W = sum of w in the same order;  V_k = acc_k (1 / W),
 *    the reciprocal correctly rounded, once per pixel.  dense_out[b, k, oy, ox] = V_k; labels_out = the FIRST maximum of V_k over k.
 * Consequences: R = 0 is the nearest-neighbour enlargement of logp, bit for bit; a constant guide gives a pure Gaussian enlargement;
 * nothing is atomic and two runs agree bit for bit; the labels-only launch writes the labels of the launch with dense_out.
 *
 * dinoseg_op_guide_cells: step 1 alone, one launch.  dinoseg_op_upsample_guided: steps 2-6 in one launch from the cells of step 1 (for
 * the same guide and grid), without the [B, C, OH, OW] transient unless dense_out is given; labels_out int32 [B, OH, OW], dense_out fp32
 * [B, C, OH, OW], at least one.  Refused on the host (-1, a message naming the entry) before anything is launched: null pointers, a
 * radius outside 0..3, sigmas outside their ranges or not finite, every shape dinoseg_op_upsample_argmax refuses, OH or OW above 2^20,
 * and a tile footprint ((64 + 2R) x (32 + 2R) cells at ratio 1) that does not fit the LDS.  Stream-ordered, no host synchronisation. */
int dinoseg_op_guide_cells(const uint8_t* guide, int32_t B, int32_t OH, int32_t OW, int32_t hp, int32_t wp, uint32_t* cells, void* stream);
int dinoseg_op_upsample_guided(const float* logp, const uint8_t* guide, const uint32_t* cells, int32_t B, int32_t hp, int32_t wp, int32_t C,
                               int32_t OH, int32_t OW, int32_t radius, double sigma_spatial, double sigma_range, int32_t* labels_out,
                               float* dense_out, void* stream);
/* dinoseg_forward_hw into the caller's logp_out [B*n, n_classes] (required), then dinoseg_op_guide_cells into cells_scratch (uint32
 * [B, hp, wp], required) and dinoseg_op_upsample_guided for the whole batch on the caller's stream (under the two-stream split: behind
 * the join).  For uint8 frames with OH x OW == H x W, guide may alias x.  Everything the launches would refuse is refused before the
 * forward enqueues anything.  Stream-ordered, capturable, no host synchronisation, no allocation. */
int dinoseg_forward_guided_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, const uint8_t* guide,
                              int32_t OH, int32_t OW, int32_t radius, double sigma_spatial, double sigma_range, float* logp_out,
                              uint32_t* cells_scratch, int32_t* labels_out, float* dense_out, void* stream);

/* ---- image-guided iterative label refinement at pixel resolution: PAMR (pixel-adaptive mask refinement, Araslanov & Roth, CVPR 2020).
 * A state P [B, C, OH, OW] is averaged `iters` times over dilated neighbours whose weights fall with the guide's colour difference in
 * units of the local standard deviation, so mass spreads inside a region and stops at the image's edges.  A pure gather in a fixed tap
 * order: no atomics, nothing that grows as N^2, two runs agree bit for bit ----
 *
 *   guide     : uint8 [B, OH, OW, 3] at the state's size; 1 <= OH, OW <= 2^14
 *   state P   : fp32 [B, C, OH, OW], 1 <= C <= 256, in half 0 of scratch [2][B, C, OH, OW] (dinoseg_refine_scratch_bytes)
 *   dilations : host array d_1 < ... < d_M, 1 <= M <= 6, each in 1..24 (PAMR's: 1, 2, 4, 8, 12, 24)
 *   sigma     : in [1e-3, 1e3] (PAMR's constant: 0.1);  iters in 0..64
 * With S = 9 M, the constant k = log2(e) sqrt(S (S - 1)) / (3 sigma) is computed on the host in fp64 and rounded once to fp32; the rule
 * is in terms of the rounded value.  All coordinates and colour differences are integers.
 *
 * 1. Taps.  Per dilation d the 8 offsets (dy, dx) in {-d, 0, d}^2 without (0, 0); order: dilation ascending, then dy ascending, then dx
 *    ascending; T = 8 M taps.  A tap's coordinates are clamped to the frame (replicate border), so a tap may be the pixel itself.
 * 2. Local deviation.  Per pixel and guide channel, over the S samples -- the 9 clamped positions of every dilation, the centre counting
 *    M times -- the integer sums s1 = sum g, s2 = sum g^2 and Nv = S s2 - s1^2 (exact in int32, <= 1.9e8).  r = 0 when Nv == 0 (every
 *    |difference| of that channel is then 0 too); otherwise r = k / sqrt(float(Nv)): the conversion, the square root and the quotient
 *    each correctly rounded to fp32.  This is log2(e) / (3 sigma std) with the unbiased standard deviation of the samples.
 * 3. Weights.  e_t = -(a_R r_R + a_G r_G + a_B r_B): a_R r_R rounded, then fmaf in channel order, a = the integer absolute difference
 *    between the guide at the pixel and at the tap.  e_max = the maximum over taps; w_t = exp2(e_t - e_max), the difference rounded to
 *    fp32, exp2 to one ulp.  The largest weight is exactly 1, so W = sum of w_t in tap order >= 1.
 * 4. Pass.  acc_k = sum over taps of fmaf(w_t, P_k(q_t), acc) from 0 in tap order;  P'_k = acc_k (1 / W), the reciprocal correctly
 *    rounded, once per pixel.
 * 5. Result.  After the last pass labels = the FIRST maximum of P_k over k; if that maximum is not > 0 the label is -1 (no mass
 *    reached the pixel).  iters = 0 labels the seed.
 * Consequences: a constant guide gives all weights exactly 1 and a pass is plain fp32 additions in tap order times the rounded 1 / T;
 * iters = n in one call equals n calls with iters = 1, each from the state the one before returned, bit for bit; the labels-only call
 * writes the labels of the call that also returns the state.
 *
 * dinoseg_op_refine_seed: one launch that writes half 0 of scratch.
 *   kind 0: seed = int32 labels [B, OH, OW]; the one-hot state of C classes.  A label outside [0, C) (255, -100) gives an all-zero
 *           pixel, which takes what its neighbours give.  hp, wp and gain are ignored.
 *   kind 1: seed = fp32 scores [B, hp*wp, C], OH >= hp, OW >= wp: the bilinear enlargement v of dinoseg_op_upsample_argmax (its dense
 *           values bit for bit), then per pixel g_k = gain v_k (rounded), m = max g_k, x_k = exp(g_k - m) by v_exp_f32 of (g_k - m)
 *           log2(e), s = sum of x_k in class order, P_k = x_k (1 / s) with the reciprocal correctly rounded.  gain > 0 and finite; 1
 *           makes the head's log-probs seed their own probabilities.
 * dinoseg_op_refine_iterate: `iters` passes from half 0, one launch each, ping-pong between the halves; the last pass writes labels_out
 *   int32 [B, OH, OW] and, when given, the final state dense_out fp32 [B, C, OH, OW] (at least one is required; dense_out must not
 *   alias scratch).  Afterwards the scratch's contents are unspecified; half 0 is read, so seed again (or copy a state into half 0)
 *   before the next call.
 * Refused on the host (-1, a message naming the entry) before anything is launched: null pointers; kind outside {0, 1}; B < 1; C, n_dil,
 * a dilation, sigma, gain, iters or sizes out of range; dilations not strictly ascending; every shape dinoseg_op_upsample_argmax
 * refuses (kind 1); a tile footprint (64 + 2 d_M) x (32 + 2 d_M), clamped to the frame, of which two planes do not fit the LDS (no
 * accepted dilation reaches that).  Stream-ordered, no host synchronisation, no allocation. */
int64_t dinoseg_refine_scratch_bytes(int32_t B, int32_t C, int32_t OH, int32_t OW);
int dinoseg_op_refine_seed(const void* seed, int32_t kind, int32_t B, int32_t C, int32_t OH, int32_t OW, int32_t hp, int32_t wp, double gain,
                           void* scratch, void* stream);
int dinoseg_op_refine_iterate(const uint8_t* guide, void* scratch, int32_t B, int32_t C, int32_t OH, int32_t OW, const int32_t* dilations,
                              int32_t n_dil, double sigma, int32_t iters, int32_t* labels_out, float* dense_out, void* stream);
/* dinoseg_forward_hw into the caller's logp_out [B*n, n_classes] (required), then dinoseg_op_refine_seed (kind 1, gain) from it into
 * scratch and dinoseg_op_refine_iterate for the whole batch on the caller's stream (under the two-stream split: behind the join).  For
 * uint8 frames with OH x OW == H x W, guide may alias x.  Everything the launches would refuse is refused before the forward enqueues
 * anything.  Stream-ordered, capturable, no host synchronisation, no allocation. */
int dinoseg_forward_refined_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, const uint8_t* guide,
                               int32_t OH, int32_t OW, double gain, const int32_t* dilations, int32_t n_dil, double sigma, int32_t iters,
                               float* logp_out, void* scratch, int32_t* labels_out, float* dense_out, void* stream);

/* ---- pixel-resolution training loss (what ViT segmenters train on: F.cross_entropy(F.interpolate(scores, size=mask.shape,
 * mode="bilinear", align_corners=False), mask, ignore_index=255)), without the [B, C, OH, OW] transient ----
 *
 * dinoseg_op_upsample_nll: with U = the bilinear upsample of logp (the coordinates and arithmetic of dinoseg_op_upsample_argmax) and
 * n = the number of valid pixels of the batch,
 *   loss  = (1/n) sum over valid pixels of logsumexp_c U[b,c,y,x] - U[b,t,y,x]                  -> *loss_out (device float)
 *   dlogp = d loss / d logp, fp32 [B, hp*wp, C]: what dinoseg_backward takes (nullable: loss only)
 *   logp   : fp32 [B, hp*wp, C];  labels: int64 [B, OH, OW];  1 <= C <= 256;  OH >= hp, OW >= wp
 * A pixel is valid when 0 <= label < C.  ignore_index (outside [0, C), e.g. 255) and -100 are skipped; any other label is skipped
 * too and sets flags[0] |= 1 (device int32, nullable).  n == 0: loss is NaN, dlogp all zeros.  n_valid_out (device float, nullable)
 * receives n.  dlogp is summed in a fixed order without floating-point atomics: bit-identical from run to run; the loss sum uses
 * atomics unless option "deterministic" is 1.  scratch: dinoseg_op_upsample_nll_scratch_bytes(...) bytes of device memory (one fp32
 * per pixel plus reduction partials: at most 8 bytes per pixel + 64 KiB; -1 for a shape the op refuses).  Stream-ordered, no host
 * synchronisation, capturable.  Null logp / labels / loss_out / scratch, a bad shape and an ignore_index inside [0, C) are refused
 * on the host (-1) before anything is launched. */
int64_t dinoseg_op_upsample_nll_scratch_bytes(int32_t B, int32_t hp, int32_t wp, int32_t C, int32_t OH, int32_t OW);
int dinoseg_op_upsample_nll(const float* logp, int32_t B, int32_t hp, int32_t wp, int32_t C, int32_t OH, int32_t OW,
                            const int64_t* labels, int32_t ignore_index, float* loss_out, float* dlogp_out, float* n_valid_out,
                            int32_t* flags, void* scratch, void* stream);

/* ---- multi-scale + flip ensemble at pixel resolution (the standard evaluation protocol of ADE20K / COCO-Stuff / Pascal-Context
 * segmenters: run the frame at several scales, each also mirrored, bring every view's scores to the output size, softmax each view,
 * average, argmax), without any [B, C, OH, OW] transient ----
 *
 * dinoseg_op_upsample_ensemble: sum_k softmax_c(F.interpolate(grid_k, size=(OH, OW), mode="bilinear", align_corners=False)) / K with
 * grid_k = logp[k].view(B, hp[k], wp[k], C).permute(0, 3, 1, 2), flipped along its width first when flip[k] == 1; one launch.
 *   logp, hp, wp, flip : HOST arrays of K entries (as dinoseg_adam_step_multi takes its arrays); logp[k] a device pointer to fp32
 *                        [B, hp[k]*wp[k], C], the layout the head writes; flip[k] 0 or 1; 1 <= K <= 12; 1 <= C <= 256
 *   labels_out : int32 [B, OH, OW], the FIRST maximum over classes of the summed probabilities (nullable)
 *   conf_out   : fp32 [B, OH, OW], that maximum / K: the ensemble's probability of the label (nullable)
 *   probs_out  : fp32 [B, C, OH, OW], the mean probabilities in torch's layout (nullable); at least one output is required
 *   scratch    : dinoseg_op_upsample_ensemble_scratch_bytes(K, B, OH, OW) bytes of device memory = one fp32 per view and pixel
 *                (-1 for K or a size out of range)
 * Per pixel, view k and class c: v_k[c] is the bilinear value with the coordinates and arithmetic of dinoseg_op_upsample_argmax
 * (exact integer coordinates, a + (b - a) lambda along x and then along y); when flip[k] == 1 the two column taps are wp-1-i0 and
 * wp-1-i1, in that order, with the same lambda, so a flipped view fed a mirrored grid is bit-identical to an unflipped view fed the
 * original.  lse_k = m_k + logf(sum_c expf(v_k[c] - m_k)) with m_k the (running) maximum over classes, p_k[c] = expf(v_k[c] - lse_k)
 * (expf of these arguments <= 0 is the hardware's 2^(x log2 e): within 3e-8 absolute of the libm value);
 * s[c] = p_0[c] + p_1[c] + ... in view order in fp32; probs = s / K, conf = max_c s[c] / K.  No atomics: bit-identical from run to
 * run.  Every view needs OH >= hp[k] and OW >= wp[k].  K outside 1..12, a null table or view pointer, a flip other than 0 / 1, all
 * outputs null, a null scratch, a shape dinoseg_op_upsample_argmax refuses, and views whose footprints under one 64 x 32 output tile
 * add up to more cells than the LDS holds (the message names the count) are refused on the host (-1) before anything is launched.
 * Stream-ordered, no host synchronisation. */
int64_t dinoseg_op_upsample_ensemble_scratch_bytes(int32_t K, int32_t B, int32_t OH, int32_t OW);
int dinoseg_op_upsample_ensemble(const float* const* logp, const int32_t* hp, const int32_t* wp, const int32_t* flip, int32_t K, int32_t B,
                                 int32_t C, int32_t OH, int32_t OW, int32_t* labels_out, float* conf_out, float* probs_out, void* scratch,
                                 void* stream);

/* ---- sliding-window inference at pixel resolution (mmsegmentation's mode='slide'; the evaluation protocol of Segmenter, SETR and
 * the DINO-based ADE20K / Pascal-Context segmenters for frames larger than the training size): cut the frame into overlapping
 * windows of the training size, run the model on every window, bring each window's scores to pixel resolution, average them where
 * windows overlap, argmax -- without a [B, C, H, W] accumulator ----
 *
 * The window rule, per axis, with frame side L, window w (1 <= w <= L) and stride s (>= 1), in integers:
 *   g    = max(L - w + s - 1, 0) / s + 1                   windows
 *   o[i] = max(min(i s + w, L) - w, 0),  i = 0 .. g-1      their origins: the last window is shifted back so that it ends at L
 * Windows of a frame are ordered row-major over (gy, gx), windows of a batch frame-major: window (b, gy, gx) has the index
 * (b gh + gy) gw + gx in the flattened list of B gh gw windows.  Origins need not be multiples of the patch, and H, W need not be.
 *
 * dinoseg_window_origins (host only, no device): writes o[0 .. g-1] to out (room for cap entries) and returns g; with out == NULL and
 * cap == 0 it returns g alone.  -1 for w > L, w < 1, s < 1 or cap < g. */
int dinoseg_window_origins(int32_t L, int32_t win, int32_t stride, int32_t* out, int32_t cap);
/* dinoseg_op_crop_windows: windows [first, first + count) of the flattened list, gathered into one contiguous batch that
 * dinoseg_forward_hw takes, in one launch.
 *   x   : the frames, x_kind 0 = uint8 [B, H, W, 3], 1 = fp32 [B, 3, H, W]
 *   out : uint8 [count, win_h, win_w, 3] or fp32 [count, 3, win_h, win_w]; 16-byte aligned (the start of an allocation)
 * win_w is a multiple of 8 (the destination is written with vector stores; the source is read element by element, a window starts
 * at any pixel).  Null pointers, an x_kind other than 0 / 1, non-positive sizes or strides, a window larger than the frame, and
 * first < 0, count < 1 or first + count > B gh gw are refused on the host (-1) before anything is launched. */
int dinoseg_op_crop_windows(const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t win_h, int32_t win_w,
                            int32_t stride_h, int32_t stride_w, int32_t first, int32_t count, void* out, void* stream);
/* dinoseg_op_window_merge: the log-probs of all windows -> pixel-resolution mean and labels, in ONE launch.
 *   logp       : fp32 [B gh gw, (win_h/patch) (win_w/patch), C], the layout the head writes for the window batch in the order above
 *   labels_out : int32 [B, H, W], the FIRST maximum over classes of the mean (nullable)
 *   dense_out  : fp32 [B, C, H, W], the mean log-probs in torch's layout (nullable); at least one output is required
 *   1 <= C <= 256; patch 8 or 16; win_h, win_w multiples of the patch, win_h <= H, win_w <= W; strides >= 1; any H, W
 * Per pixel (y, x) and class c: for every window that contains the pixel, in window order, u_w[c] is the bilinear value of that
 * window's grid at the window's local pixel (y - oy, x - ox), upsampled from (win_h/patch, win_w/patch) to (win_h, win_w) with the
 * coordinates and arithmetic of dinoseg_op_upsample_argmax (exact integer coordinates, a + (b - a) lambda along x and then along
 * y);  m[c] = (u_w0[c] + u_w1[c] + ...) / (float)n with fp32 adds in window order, n the number of windows that contain the pixel,
 * and an IEEE division;  dense = m, label = the first maximum of m.  No atomics and no scratch: bit-identical from run to run; one
 * window equal to the frame gives exactly dinoseg_op_upsample_argmax.
 * Accepted: every frame in which no pixel row lies in more than 4 window rows and no pixel column in more than 4 window columns
 * (at most 16 windows over a pixel); any stride >= ceil(window / 3) qualifies.  Denser coverage is refused with a message that
 * names it.  Also refused on the host (-1) before anything is launched: a null logp, both outputs null, C outside 1..256, a patch
 * other than 8 or 16, window sides that are not patch multiples, a window larger than the frame, non-positive strides or sizes,
 * and sizes beyond the integer ranges of dinoseg_op_upsample_argmax.  Stream-ordered, no host synchronisation. */
int dinoseg_op_window_merge(const float* logp, int32_t B, int32_t H, int32_t W, int32_t patch, int32_t win_h, int32_t win_w,
                            int32_t stride_h, int32_t stride_w, int32_t C, int32_t* labels_out, float* dense_out, void* stream);

/* ---- augmentation of fine-tuning frames and label masks on the device (the reference's get_augmented_transforms(),
 * pl_torch_modules.py:44-57: RandomResizedCrop, ShiftScaleRotate, HorizontalFlip, ColorJitter(brightness), GaussianBlur, Normalize,
 * the mask nearest-resized to the patch grid) as one or two launches.  The device code is a pure function of an explicit per-frame
 * table: no device random numbers, integer (Q16) coordinates, no atomics -- bit-identical from run to run.  The randomness lives in
 * the host function that fills the table (dino_amd.augment.draw_reference_augment). ----
 *
 * One frame's parameters, 36 32-bit words (Python: a row of an int32 [B, 36] tensor, the floats bit-cast). */
typedef struct dinoseg_augment_frame {
    int32_t a[6];        /* inverse affine, OUTPUT pixel (ox, oy) -> source, in Q16 (units of 2^-16 source pixel), evaluated in int64:
                            Ux = a0 ox + a1 oy + a2,  Uy = a3 ox + a4 oy + a5.  U is the continuous source coordinate in edge
                            convention (source pixel i covers [i, i+1)); a2 and a5 already contain the output half-pixel term
                            (a0 + a1) / 2 resp. (a3 + a4) / 2 */
    int32_t border;      /* 0 = reflect-101 (OpenCV's default, what the reference's ShiftScaleRotate uses), 1 = constant; read as
                            border & 1 */
    int32_t void_label;  /* the label written where the nearest source pixel is outside the frame, under border = 1 */
    float fill[3];       /* RGB in 0..255: the value of every bilinear TAP outside the frame under border = 1 (per tap, as
                            cv2.BORDER_CONSTANT and grid_sample(padding_mode="zeros") do) */
    float gain, bias, sat; /* colour: v = fmaf(gain, v, bias) per channel; g = 0.299 r + 0.587 g + 0.114 b of those;
                            v = fmaf(sat, v - g, g); clamp to [0, 255] */
    int32_t radius;      /* Gaussian radius r, 0..20 (kernel size 2r + 1 <= 41); 0 = no blur; clamped to [0, max_radius] on the device */
    float w[21];         /* taps w[|d|], d = -r..r, normalised by the host in fp64; entries past r are ignored */
} dinoseg_augment_frame;
/* The rule, per output pixel (ox, oy) of frame b:
 *   image : Vx = Ux - 32768, x0 = Vx >> 16 (arithmetic), lx = (float)(Vx & 0xFFFF) / 65536.f; the same for y.  The four taps
 *           (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1), every index folded by the border rule: reflect-101 with side n has the
 *           period 2 (n - 1) (.. 2 1 0 1 2 .. n-2 n-1 n-2 ..; a side of 1 always folds to 0); under border = 1 a tap with an index
 *           outside the frame has the value fill[c].  Lerp along x, then y, each fmaf(b - a, l, a) (as dinoseg_op_upsample_argmax).
 *   label : the source mask at (Uy >> 16, Ux >> 16) after folding, or void_label when that is outside under border = 1.
 *   colour: as the struct states (gray = fmaf(0.114, b, fmaf(0.587, g, 0.299 r)) in fp32).
 *   blur  : separable, horizontal then vertical, on the OUTPUT frame after colour: sum over d = -r .. r in that order,
 *           acc = fmaf(w[|d|], v[fold(x + d)], acc) from acc = 0, output coordinates folded by reflect-101 (OH, OW > r); the
 *           intermediate is fp32 and is not rounded or clamped.  A frame with radius 0 skips the blur altogether.
 *   out   : out_kind DINOSEG_INPUT_F32_CHW: fp32 [B, 3, OH, OW] = (v / 255 - mean) / std with the ImageNet constants;
 *           DINOSEG_INPUT_U8_HWC: uint8 [B, OH, OW, 3] = rintf of v clamped to [0, 255].  Both are what dinoseg_forward_hw and the
 *           train-step entries take.
 * dinoseg_op_augment:
 *   frames       : uint8 [B, H, W, 3];  masks: uint8 (mask_kind 0) or int64 (mask_kind 1) [B, H, W], nullable
 *   table        : DEVICE array of B dinoseg_augment_frame;  max_radius: an upper bound (0..20) of the table's radii, known to the host
 *   out          : the image in out_kind, 16-byte aligned
 *   pixel_labels : int64 [B, OH, OW], nullable;  patch_labels: int64 [B, (OH/patch) (OW/patch)], nullable: the pixel label at
 *                  (patch i, patch j), what the reference's Resize(NEAREST) to res // 8 picks
 *   scratch      : fp32 [B, 3, OH, OW] of the caller, required when max_radius > 0 (never touched otherwise)
 * Launch 1 (augment_warp_kernel) does warp, colour and labels per output pixel; with max_radius == 0 it writes the final image and
 * is the only launch.  Launch 2 (augment_blur_kernel, max_radius > 0) stages each 64 x 32 output tile of the scratch with its
 * r-wide folded halo in LDS one channel at a time, keeps the horizontal pass's result in LDS, and writes the final image; frames
 * with radius 0 are converted straight through (bit-identical to the one-launch result).
 * Refused on the host (-1) before anything is launched: null frames, table or out; a mask_kind or out_kind other than 0 / 1;
 * non-positive sizes or sides above 16384; max_radius outside 0..20; OH <= max_radius or OW <= max_radius; a label output
 * without masks; patch_labels with a patch other than 8 or 16 or with OH or OW not a multiple of it; a null scratch when
 * max_radius > 0; out not 16-byte aligned.  Stream-ordered, no host synchronisation. */
int dinoseg_op_augment(const uint8_t* frames, const void* masks, int32_t mask_kind, int32_t B, int32_t H, int32_t W,
                       const dinoseg_augment_frame* table, int32_t max_radius, int32_t OH, int32_t OW, int32_t out_kind, void* out,
                       int64_t* pixel_labels, int64_t* patch_labels, int32_t patch, float* scratch, void* stream);

/* ---- video label propagation from patch features (the semi-supervised video segmentation protocol of the DINO paper: one labelled
 * frame, every later frame takes its labels from the nearest patch features of the frames before it), without the [n_ctx, n, n]
 * affinity.  No reference counterpart: the reference labels one frame at a time.  propagate.hip.
 *
 * Notation: hp x wp the patch grid, n = hp wp cells row-major, D the embedding width (a multiple of 64), C the number of label
 * classes, 1 .. 256, independent of the model's head; R >= 0 the neighbourhood radius in cells, k in 1 .. 16, tau > 0 the temperature.
 * Context list of target frame t >= 1 (the caller's, DINOSeg.propagate): frame 0 first, then the last min(t - 1, n_context) frames
 * before t, oldest first: t = 1 -> [0]; t = 2 -> [0, 1]; t = 9, n_context = 7 -> [0, 2 .. 8].  Frame 0 never enters the queue; at most
 * 1 + n_context <= 16 context frames.
 *
 * 1. Features (dinoseg_op_normalize_tokens).  The patch tokens of dinoseg_features_hw without the CLS row; f^ = f / max(||f||_2, 1e-12).
 *    The operand planes hold 2^10 f^ as fp16 hi + lo (hi = fp16(v), lo = fp16(v - hi), the norm and the quotient in fp64):
 *    [B][2][n][D] 16-bit elements, hi plane then lo plane per frame.
 * 2. Candidates.  The candidates of query cell q = (r, c) are the cells j = (r', c') of every context frame with |r' - r| <= R and
 *    |c' - c| <= R inside the grid (integer test per pair).  Candidate j of the ci-th context frame has the global index g = ci n + j.
 *    Its score s = <f^_t[q], f^_ctx[j]> is accumulated in fp32 from the planes (lo.hi + hi.lo + hi.hi, D in ascending slices of 64) and
 *    is a function of the two rows alone, not of where the pair sits in a tile: bit-equal rows give bit-equal scores.  A score of -0 is
 *    taken as +0.  |s - the fp64 value| <= (D + 16) 2^-24.
 * 3. Selection.  The K' = min(k, #candidates) candidates that come first in the total order (score descending, then g ascending):
 *    rank 0 .. K'-1.  The order is total, so the result does not depend on how the lists are merged.
 * 4. Weights.  w_i = exp2((s_i - s_0) a) in fp32, a = log2(e) / tau computed in fp64 on the host and rounded once to fp32;
 *    W = sum w_i in rank order.
 * 5. Value.  V[c] = (sum_i w_i seg[g_i, c]) (1 / W), by fmaf in rank order from 0, the reciprocal (correctly rounded) taken once;
 *    seg_out[q, :] = V, fp32 [n, C].  This soft map, not its argmax, is what later frames use as context.
 * 6. Pixel labels: dinoseg_op_upsample_argmax applied to seg_out, unchanged.
 *
 * The seed (dinoseg_op_label_cells): integer pixel labels [OH, OW] (OH >= hp, OW >= wp; mask_kind 0 = uint8, 1 = int64, as
 * dinoseg_op_augment) -> seg fp32 [n, C].  Pixel (y, x) belongs to cell ((y hp) / OH, (x wp) / OW), the nearest rule of
 * dinoseg_op_guide_cells; seg[cell, c] = float(count_c) / float(n_cell) with integer counts (no atomics); a pixel whose label is
 * outside [0, C) (255, -100) counts in n_cell and in no class.
 *
 * In exact arithmetic and without ties this is the DINO script's computation (exp(bmm / 0.1) times the neighbourhood mask, topk over
 * all context candidates, renormalise, segs @ aff; defaults n_context 7, R 12, k 5, tau 0.1).  Deviations: exact ties at the cut keep
 * exactly k candidates by index (the script keeps the whole tied group); the script's per-class min-max rescale of the enlarged map is
 * not done; the enlargement uses this library's exact coordinates.
 *
 * dinoseg_op_propagate: steps 2 - 5 for one target frame in two launches (per (8 x 8 query tile, context frame) the scores on MFMAs
 * and a per-query list of k in LDS; then the merge of the context frames' lists, the weights and the k gathers).  ctx_planes /
 * ctx_segs are HOST arrays of n_ctx device pointers (planes of step 1, seg fp32 [n, C]); they travel to the kernels by value.
 * scratch: dinoseg_propagate_scratch_bytes(hp, wp, n_ctx, k) bytes of device memory (8 n_ctx n k; host only, -1 for refusable
 * arguments).  Optional debug outputs: topk_idx int32 [n, k] (g in rank order, -1 beyond K') and topk_w fp32 [n, k] (w_i / W, 0
 * beyond K').  R above the grid's sides is the whole grid.  No atomics, no synchronisation between workgroups; two runs agree bit for
 * bit.  Refused on the host (-1, the message names the entry) before anything is launched: null pointers; C outside 1 .. 256; k
 * outside 1 .. 16; n_ctx outside 1 .. 16; R < 0; tau not finite or not positive; non-positive sizes or grid sides above 4096; D not a
 * multiple of 64 or above 8192; planes not 16-byte aligned.  Stream-ordered, no host synchronisation, no allocation. */
#define DINOSEG_PROPAGATE_MAX_CONTEXT 16
#define DINOSEG_PROPAGATE_MAX_K 16
int dinoseg_op_normalize_tokens(const float* tokens, int32_t B, int32_t n, int32_t D, void* planes, void* stream);
int dinoseg_op_label_cells(const void* labels, int32_t mask_kind, int32_t OH, int32_t OW, int32_t hp, int32_t wp, int32_t C, float* seg,
                           void* stream);
int64_t dinoseg_propagate_scratch_bytes(int32_t hp, int32_t wp, int32_t n_ctx, int32_t k);
int dinoseg_op_propagate(const void* target_planes, const void* const* ctx_planes, const float* const* ctx_segs, int32_t n_ctx,
                         int32_t hp, int32_t wp, int32_t D, int32_t C, int32_t radius, int32_t k, double tau, float* seg_out,
                         int32_t* topk_idx, float* topk_w, void* scratch, void* stream);

/* ---- few-shot segmentation: k-NN label retrieval from a memory bank of labelled patch features (the k-NN evaluation of the DINO paper
 * made dense; the in-context scene understanding protocol of Hummingbird), without the [N, M] score matrix.  No reference counterpart:
 * the reference trains its head.  knn.hip.  The definitions are those of the propagation section above; only what differs is stated.
 *
 * Notation: B query frames of n cells, N = B n queries, query i = frame i / n, cell i % n; a bank of bank_rows rows of which the first
 * M are live (1 <= M <= bank_rows <= 2^24), so that a bank is filled in place up to its capacity; D the embedding width (a multiple
 * of 64 in 64 .. 8192); C classes, 1 .. 256; k in 1 .. 16; tau > 0; E = (D + 16) 2^-24.
 *
 * 1. Rows.  Query planes [B][2][n][D] as dinoseg_op_normalize_tokens writes them.  Bank planes [2][bank_rows][D]: the same format with
 *    one "frame" of bank_rows rows, the lo plane bank_rows D elements after the hi plane.  Rows M .. bank_rows - 1 (planes and labels)
 *    are never read.
 * 2. Labels.  label_kind 0: soft fp32 [bank_rows, C].  label_kind 1: hard uint8 [bank_rows]; a value >= C is void: a void row is a
 *    neighbour like any other (it is selected, its weight counts in W) and adds to no class, the convention of dinoseg_op_label_cells.
 * 3. Candidates.  Every live row g in 0 .. M-1 is a candidate of every query: no neighbourhood test.  The score is step 2 of the
 *    propagation rule exactly (lo.hi + hi.lo + hi.hi in one fp32 chain on v_mfma_f32_32x32x16_f16, D in ascending slices of 64, -0
 *    taken as +0, a function of the two rows alone, |s - the fp64 value| <= E).
 * 4. Selection.  The first K' = min(k, M) candidates in the total order (score descending, then g ascending).
 * 5. Weights and value.  Steps 4 and 5 of the propagation rule: w_i = exp2((s_i - s_0) a), a = log2(e) / tau rounded once on the host,
 *    W = sum w_i in rank order, V[c] = (sum_i w_i labels[g_i, c]) (1 / W) by fmaf in rank order from 0.  Hard labels:
 *    V[c] = (the sum of the w_i with label_i == c, in rank order) (1 / W).  seg_out[i, :] = V, fp32 [N, C].
 * 6. Pixel labels: dinoseg_op_upsample_argmax applied to seg_out, unchanged.
 *
 * dinoseg_op_knn_labels: steps 3 - 5 in two launches.  Scores: the grid is (ceil(N / 64), S); a workgroup takes 64 consecutive queries
 * and one of S contiguous bank ranges, walks it in key blocks of 64 and keeps each query's list of k (score, g) in LDS; its merged
 * list goes to the scratch [S][N][k].  With nblk = ceil(M / 64) key blocks, range s is the blocks floor(s nblk / S) ..
 * floor((s + 1) nblk / S) - 1, i.e. rows 64 floor(s nblk / S) .. min(64 floor((s + 1) nblk / S), M) - 1: whole blocks, never empty,
 * the last one clipped at M.  Merge: one wave per query merges the S lists under the total order (S k <= 256 keys), forms the weights
 * and does the k gathers (soft rows) or k compares per class (hard labels).  No atomics, no synchronisation between workgroups,
 * nothing of size N M is written; two runs agree bit for bit.
 * splits: 0 = the library's choice, dinoseg_knn_splits(N, M, k) = min(cap, max(1, min(ceil(512 / ceil(N / 64)), nblk / 4))) with
 * cap = min(16, 256 / k, nblk): two workgroups for each of the 256 compute units where the query tiles alone give fewer, and ranges of
 * at least 4 key blocks.  Any S in 1 .. cap is accepted.  The order is total, so the outputs are bit-identical for every S.
 * scratch: dinoseg_knn_scratch_bytes(N, M, k, splits) bytes of device memory (8 S N k, S resolved as above; host only, -1 for
 * refusable arguments; dinoseg_knn_splits likewise).  Optional outputs: topk_idx int32 [N, k] (g in rank order, -1 beyond K') and
 * topk_w fp32 [N, k] (w_i / W, 0 beyond K').
 * Refused on the host (-1, the message names the entry) before anything is launched: null pointers (the two optional outputs apart);
 * C outside 1 .. 256; k outside 1 .. 16; splits outside 0 .. cap; a label_kind other than 0 / 1; D not a multiple of 64 or above
 * 8192; M or bank_rows outside 1 <= M <= bank_rows <= 2^24; non-positive B or n, n above 2^24, B n above 2^31 - 256; tau not finite
 * or not positive; planes not 16-byte aligned.  Stream-ordered, no host synchronisation, no allocation. */
#define DINOSEG_KNN_MAX_K 16
int64_t dinoseg_knn_scratch_bytes(int32_t N, int32_t M, int32_t k, int32_t splits);
int32_t dinoseg_knn_splits(int32_t N, int32_t M, int32_t k);
int dinoseg_op_knn_labels(const void* query_planes, int32_t B, int32_t n, const void* bank_planes, int64_t M, int64_t bank_rows,
                          const void* bank_labels, int32_t label_kind, int32_t D, int32_t C, int32_t k, double tau, int32_t splits,
                          float* seg_out, int32_t* topk_idx, float* topk_w, void* scratch, void* stream);

/* ---- PCA of patch features: streaming moments, projection onto a basis and the three-colour feature map (the DINO / DINOv2 figure;
 * the dimensionality reduction STEGO, "Deep ViT Features" and Hummingbird put in front of clustering and retrieval).  No reference
 * counterpart.  pca.hip.  The eigen-decomposition is the host's (dino_amd.pca_solve); these are the three device operators around it.
 *
 * Notation: tokens are fp32 [B][1 + n][D] as dinoseg_features_hw writes them; row 0 of every frame is the CLS row and is skipped, as
 * dinoseg_op_normalize_tokens skips it.  D is a multiple of 64 in 64 .. 1024.  Patch row p = b n + c (frame b, cell c), p in
 * 0 .. N - 1, N = B n.  Every product sum is v_mfma_f32_32x32x2_f32, which is bit for bit the fp32 fmaf chain in k order, so the
 * rules below are exact to restate.
 *
 * dinoseg_op_token_moments: the sufficient statistics of a PCA, added to the caller's accumulators so that a data set is fitted chunk
 * by chunk.
 *   keep  : uint8 [B][n], nullable; a row with keep == 0 does not take part.   shift : fp32 [D], nullable = zeros.
 *   sum   : fp64 [D];   outer : fp64 [D][D], nullable (sums and count only);   count : int64 [1].  All three are ADDED to.
 * 1. The point.  c_p[d] = fp32(x_p[d] - shift[d]): one fp32 subtraction.  A row that is not kept has c_p = +0 in every column.
 * 2. Ranges.  ALL N patch rows, kept or not, are cut by position into R ranges of L = ceil(N / R) consecutive rows: range r is
 *    rows r L .. min((r + 1) L, N) - 1 (trailing ranges may be empty).  R = dinoseg_pca_ranges(N, D) =
 *    max(1, min(64, ceil(N / 128), ceil(2048 / P))) with T = D / 64 column tiles and P = T (T + 1) / 2 tile pairs: a function of N
 *    and D alone, never of the mask, so no compaction pass is needed.
 * 3. Partials.  Per range, part_outer[d][e] = the fp32 chain acc = fmaf(c_p[d], c_p[e], acc) over the range's rows in ascending
 *    order from +0 (rows not kept add +0 products); part_sum[d] = the fp32 chain acc = acc + c_p[d] likewise.  Only tile pairs
 *    with d / 64 <= e / 64 are computed.
 * 4. Totals.  total = the partials added in range order in fp64 from 0; outer[d][e] += total for d <= e, and the SAME total is added
 *    to outer[e][d]: an outer that starts symmetric stays exactly symmetric.  sum[d] += its total.  count += the kept rows (exact).
 * Bounds, per element: |outer's increment - exact sum_p c_p[d] c_p[e]| <= (L + 16) 2^-24 sum_p |c_p[d] c_p[e]|, and
 * |sum's increment - exact| <= (L + 16) 2^-24 sum_p |c_p[d]|.  No atomics, no synchronisation between workgroups beyond the two
 * kernel boundaries; two runs agree bit for bit.  scratch: dinoseg_pca_scratch_bytes(B, n, D) = 4 R (4096 P + D + 1) bytes (host only,
 * -1 for refusable arguments; dinoseg_pca_ranges likewise): the ranges' partials, nothing of size N D.
 *
 * dinoseg_op_pca_project: y[p][j] = the fp32 chain acc = fmaf(fp32(x_p[d] - mean[d]), basis[j][d], acc) over d ascending from +0,
 * multiplied once by scale[j] when scale is given (whitening).
 *   mean : fp32 [D];  basis : fp32 [q][D], q in 1 .. 256;  scale : fp32 [q], nullable;  out : fp32 [B][1 + n][q], the token layout
 * with row 0 of every frame written as zeros, so that dinoseg_op_normalize_tokens(out, B, n, q, ...) takes it unchanged when q is a
 * multiple of 64 and dinoseg_op_pca_colour reads it.  A row's result depends on that row alone: B frames in one call or one by one
 * agree bit for bit.  |y - the fp64 value| <= (D + 16) 2^-24 sum_d |c[d] basis[j][d]|, times |scale[j]| when scale is given.
 *
 * dinoseg_op_pca_colour: components 0 .. 2 of comps (fp32 [B][1 + hp wp][q], q >= 3, as dinoseg_op_pca_project writes them) to
 * rgb uint8 [B][OH][OW][3] in one launch, 3 bytes per pixel written, no [B, 3, OH, OW] fp32 tensor.
 *   lo, inv : fp32 [3] on the device;  keep : uint8 [B][hp wp], nullable.
 * Per cell and channel t = (v - lo_c) inv_c, one subtraction and one multiplication in fp32; t is enlarged bilinearly with the exact
 * integer coordinates and the arithmetic of dinoseg_op_upsample_argmax (a + (b - a) lambda by fmaf along x, then along y); then
 * t = min(max(t, 0), 1) (a NaN becomes 0), byte = (uint8) rintf(255 t) (ties to even).  A pixel whose nearest cell
 * ((oy hp) / OH, (ox wp) / OW), the rule of dinoseg_op_guide_cells, is not kept becomes (0, 0, 0).  OH >= hp, OW >= wp, sides up to
 * 16384.  Two runs agree bit for bit.
 *
 * Refused on the host (-1, the message names the entry) before anything is launched: null required pointers; D not a multiple of 64
 * in 64 .. 1024; q outside 1 .. 256, or below 3 for the colour entry; non-positive sizes; B n above 2^31 - 256; an output smaller
 * than the grid or a side above 16384; tokens, shift, mean, basis or scratch not 16-byte aligned; sum, outer or count not 8-byte
 * aligned; scale, out, comps, lo or inv not 4-byte aligned.  Stream-ordered, no host synchronisation, no allocation. */
#define DINOSEG_PCA_MAX_Q 256
int64_t dinoseg_pca_scratch_bytes(int32_t B, int32_t n, int32_t D);
int32_t dinoseg_pca_ranges(int64_t rows, int32_t D);
int dinoseg_op_token_moments(const float* tokens, const uint8_t* keep, int32_t B, int32_t n, int32_t D, const float* shift, double* sum,
                             double* outer, int64_t* count, void* scratch, void* stream);
int dinoseg_op_pca_project(const float* tokens, int32_t B, int32_t n, int32_t D, const float* mean, const float* basis, const float* scale,
                           int32_t q, float* out, void* stream);
int dinoseg_op_pca_colour(const float* comps, int32_t B, int32_t hp, int32_t wp, int32_t q, const float* lo, const float* inv,
                          const uint8_t* keep, int32_t OH, int32_t OW, uint8_t* rgb, void* stream);

/* ---- unsupervised segmentation: spherical k-means over patch features (the k-means baseline of STEGO and of "Deep ViT Features as
 * Dense Visual Descriptors": cluster the patch tokens of a batch or clip, get segments whose ids mean the same in every frame).  No
 * reference counterpart: the reference trains on hand-labelled frames.  kmeans.hip.
 *
 * Notation: B frames of n cells, N = B n points, point i = frame i / n, cell i % n; D the embedding width (a multiple of 64 in
 * 64 .. 8192); K centroids, 1 .. 256 (the class limit of dinoseg_op_upsample_argmax); E = (D + 16) 2^-24.
 *
 * 1. Points.  The planes of dinoseg_op_normalize_tokens, [B][2][n][D] fp16 hi / lo scaled by 2^10.  The point is DEFINED as
 *    x_i = (hi_i + lo_i) 2^-10, which is exact in fp32: no rounding of the normalisation enters the rule.  All N points are clustered
 *    jointly.
 * 2. Centroids.  K rows, kept as fp32 [K][D] and as planes [2][K][D] in the same format: 2^10 c = hi + lo with hi = fp16(2^10 c),
 *    lo = fp16(2^10 c - hi), the split of the fp32 row.  The assignment reads the planes alone: c_j there is (hi_j + lo_j) 2^-10.
 *    dinoseg_op_kmeans_init writes both from caller rows [K, D]: with normalize = 1 the row is c = fp32(row / max(||row||_2, 1e-12)),
 *    the norm (fma in fp64) and the quotient in fp64 as dinoseg_op_normalize_tokens does them; with normalize = 0 the row is taken as
 *    it is (centroids that an update wrote are unit rows already and keep their bits).  centroids may be rows itself.
 * 3. Assignment (dinoseg_op_kmeans_assign).  s_ij = <x_i, c_j>, accumulated in fp32 from the planes with the arithmetic of
 *    dinoseg_op_propagate (lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16_f16, D in ascending slices of 64): a function of the two rows
 *    alone, |s_ij - the fp64 value| <= E; a score of -0 is taken as +0.  a_i = argmax_j s_ij, the lowest j on an exact tie; best_i =
 *    s_{i, a_i}.  The running (score, index) pair stays in registers; scores fp32 [N, K] is written only when the pointer is given.
 * 4. Records.  *objective = sum_i best_i in fp32 in a fixed order (per tile of 64 points an xor tree, then the tiles strided over 256
 *    threads and a binary tree); *moved = #{i : prev_assign[i] != a_i}, exact, = N when prev_assign is NULL.  Either slot may be NULL.
 *    prev_assign may be assign itself.
 * 5. Update (dinoseg_op_kmeans_update).  m_j = sum over {i : a_i = j} of x_i in fp32, in an order that is a function of the shapes and
 *    the assignment: the points are cut into R = min(ceil(N / 256), Rmax) ranges of ceil(N / R), Rmax = 4096 / K clamped to
 *    16 .. 64; inside a range the members of a cluster
 *    are taken in index order, 1024 assignments at a time, dealt round-robin to G = 256 / T thread groups (T the power of two >= D / 8,
 *    8 .. 256), each group adds its members in order, the groups are added in group order, the ranges in range order.  No
 *    floating-point atomic, no synchronisation between workgroups beyond kernel boundaries; two runs agree bit for bit.
 *    |m_j[d] - the exact sum| <= (n_j + 16) 2^-24 sum_i |x_i[d]|.  c_j = fp32(m_j / ||m_j||), the norm (fma in fp64) and the quotient in
 *    fp64; the row and its planes are written.  n_j = 0 or ||m_j|| = 0: the previous row and planes are copied bit for bit.
 *    counts[j] = n_j.  centroids / planes may be prev_centroids / prev_planes themselves.
 * 6. Pixel labels: dinoseg_op_upsample_argmax applied to scores [B, n, K], unchanged.
 *
 * The loop is the caller's (DINOSeg.cluster): init, then iters times (assign, update) with the record slots objective + t, moved + t of
 * device arrays, then one final assign that writes scores and slot iters.  Nothing stops early and nothing synchronises with the host.
 *
 * Deviations from sklearn's KMeans / the usual script: cosine (spherical) k-means, so the centroid is renormalised and the objective
 * is the sum of cosines (larger is better); seeding is by distinct sampled points (no k-means++); an empty cluster keeps its centroid
 * (sklearn relocates it); a fixed number of iterations, no tolerance test; ties go to the lowest index.
 *
 * scratch: dinoseg_kmeans_scratch_bytes(B, n, K, D) = 4 R K (D + 1) + 8 ceil(N / 64) bytes of device memory, 16-byte aligned, the same
 * buffer for assign and update (R as in step 5, at most 64): R partial centroid sets fp32 [R][K][D], their counts int32 [R][K], and per tile of 64 points one fp32
 * objective share and one int32 moved count.  Nothing of size N K or N D.  Host only; -1 for refusable arguments.
 *
 * Refused on the host (-1, the message names the entry) before anything is launched: null pointers (scores, objective, moved and
 * prev_assign are optional); D not a multiple of 64 in 64 .. 8192; K outside 1 .. 256; B or n below 1; B n above 2^31 - 256; points,
 * planes or scratch not 16-byte aligned, a 32-bit array not 4-byte aligned; normalize outside {0, 1}.  Stream-ordered, no allocation. */
#define DINOSEG_KMEANS_MAX_K 256
int64_t dinoseg_kmeans_scratch_bytes(int32_t B, int32_t n, int32_t K, int32_t D);
int dinoseg_op_kmeans_init(const float* rows, int32_t K, int32_t D, int32_t normalize, float* centroids, void* planes, void* stream);
int dinoseg_op_kmeans_assign(const void* points, int32_t B, int32_t n, const void* centroid_planes, int32_t K, int32_t D,
                             const int32_t* prev_assign, int32_t* assign, float* best, float* scores, float* objective, int32_t* moved,
                             void* scratch, void* stream);
int dinoseg_op_kmeans_update(const void* points, int32_t B, int32_t n, const int32_t* assign, const float* prev_centroids,
                             const void* prev_planes, int32_t K, int32_t D, float* centroids, void* planes, int32_t* counts,
                             void* scratch, void* stream);

/* ---- unsupervised foreground masks: normalized cut on a 1-bit patch graph (the spectral bipartition of TokenCut and of "Deep
 * Spectral Methods": which cells are the object and which the background, in this frame alone, with no label, no head, no k and no
 * other frame).  No reference counterpart.  ncut.hip.  No n x n matrix of floats exists: a frame's graph is n^2 bits.
 *
 * Notation, per frame (frames are independent; every frame is its own graph): n cells, 1 .. dinoseg_ncut_max_cells(); D the embedding
 * width (a multiple of 64 in 64 .. 8192); W = ceil(n / 64) words per row; E = (D + 16) 2^-24.
 *
 * 1. Points.  The planes of dinoseg_op_normalize_tokens, [B][2][n][D] fp16 hi / lo scaled by 2^10; x_i = (hi_i + lo_i) 2^-10 as
 *    dinoseg_op_kmeans_assign defines it.
 * 2. Scores.  s_ij = <x_i, x_j> from the planes on v_mfma_f32_32x32x16_f16, D in ascending slices of 64, fp32 accumulators.  The three
 *    products are kept in THREE accumulators and combined once as (c_lo.hi + c_hi.lo) + c_hi.hi, c_a.b = sum_d a_i[d] b_j[d].  This
 *    deliberately differs from the single chain lo.hi + hi.lo + hi.hi of dinoseg_op_propagate and dinoseg_op_kmeans_assign: with this
 *    grouping s_ij and s_ji are the same bits (the two cross terms swap roles, fp32 addition commutes), so the graph is symmetric bit
 *    for bit.  s_ij is a function of the two rows alone; |s_ij - the fp64 value| <= E; a score of -0 is taken as +0.
 * 3. Graph (dinoseg_op_ncut_graph).  bit(i, j) = s_ij > tau, tau rounded once to fp32 on the host.  graph: [B][n][W] uint64 words, row
 *    major, key j at bit j % 64 of word j / 64; pad bits are zero.  degree[i] = cnt_i = popcount(row i), exact (int32 [B][n]).
 *    This is the only launch that touches the planes.
 * 4. Weights.  W = eps 11^T + (1 - eps) Bits (TokenCut's binary affinity: 1 above tau, eps below).  d_i = fp32(eps (n - cnt_i) + cnt_i),
 *    formed in fp64; r_i = fp32(1 / sqrt(d_i)) (0 where d_i = 0); u_i = fp32(sqrt(d_i) / sqrt(sum_j d_j)), the known top eigenvector of
 *    M = D^-1/2 W D^-1/2 (0 where the sum is 0).  The iteration runs on (I + M) / 2, whose spectrum lies in [0, 1]: a negative
 *    eigenvalue of the non-PSD threshold graph can never win.
 * 5. Deflate and normalise, DN(z): c = <u, z>; q_i = fp32(z_i - c u_i); z_i <- fp32(q_i / ||q||), or 0 everywhere where ||q|| = 0
 *    (one-cell grids and complete graphs fall under this case).
 * 6. One pass (dinoseg_op_ncut_iterate), from a prepared z = DN(.):
 *      xv_j = z_j r_j (fp32);  S = sum_j xv_j;  t_i = the sum of xv_j over the set bits of row i, in fp32 in a fixed order: key j
 *      belongs to lane j % 64, a lane adds its keys in ascending order from 0, the 64 lanes are added in an xor tree (offsets 32, 16, .., 1);
 *      y_i = fp32(r_i (eps S + (1 - eps) t_i));  rho = <z, y>;  p_i = (z_i + y_i) / 2 (fp32);  z' = DN(p).
 *    The global sums S, rho, c, ||q||^2 and the mean of step 7 are fp64 in a fixed order that depends on n only (thread t of 1024 adds
 *    cells t, t + 1024, .. in order -- rho: wave w of 16 adds rows w, w + 16, .. --, an xor tree per wave, the 16 waves in order).
 *    |t_i - the exact sum| <= (cnt_i + 16) 2^-24 sum over the set bits of |xv_j|.
 *    The call: z_0 = DN(z_in); iters passes, rho[b][t] = the pass's Rayleigh record <z, y> = <z, M z> of the unit z it started from;
 *    z_out = the last z'.  Every pass after the first prepares its input once more, DN(z'), exactly as a fresh call would prepare z_out: a call
 *    with iters = T equals T calls with iters = 1 chained through z_out, bit for bit.  iters = 0 does step 7 on z_0.
 * 7. Result.  v_i = z_i r_i (fp32); avg = the mean of v (fp64); seed_cell = argmax |v_i|, the lowest index on a tie; sigma = +1 if
 *    v_seed > avg, else -1; margin_i = fp32(sigma (v_i - avg)); fg_i = margin_i > 0; eigvec = sigma v.  This is TokenCut's
 *    bipartition and seed rule: the side that holds the largest |v| is the foreground.
 * 8. Pixel labels: dinoseg_op_upsample_argmax, unchanged, applied to the two-class map [B, n, 2] = (0, margin_i); the first maximum
 *    makes ties go to background.
 *
 * Deviations from TokenCut: the points are the tokens of dinoseg_features_hw, not last-block keys; a fixed number of lazy power
 * iterations replaces the dense generalized eigh; no connected component around the seed is taken and no box is produced.
 *
 * dinoseg_ncut_graph_bytes(B, n) = 8 B n ceil(n / 64); dinoseg_ncut_max_cells() = what the four vectors z, xv, r, u leave of the 160 KiB
 * of LDS of the one workgroup that iterates a frame (10 160; the 480 x 640 camera at patch 8 has 4800; 960 x 960 at patch 8, 14 400,
 * does not fit).  Host only; the size query answers -1 for refusable arguments.
 *
 * dinoseg_op_ncut_iterate: z_in / z_out fp32 [B][n] (z_out may be z_in); rho fp32 [B][iters] (may be NULL with iters = 0); fg uint8
 * [B][n]; eigvec fp32 [B][n]; margin fp32 [B][n] or NULL; seed_cell int32 [B].  One workgroup of 1024 threads per frame runs every
 * pass in one launch; no synchronisation between workgroups, no scratch, no host synchronisation; bit-identical from run to run.
 *
 * Refused on the host (-1, the message names the entry) before anything is launched: null pointers (margin is optional, rho with
 * iters = 0); D not a multiple of 64 in 64 .. 8192; B or n below 1; n above dinoseg_ncut_max_cells(); tau not finite or outside
 * (-1, 1); eps outside [0, 1); iters outside 0 .. 4096; planes not 16-byte aligned, the graph not 8-byte aligned, a 32-bit array not
 * 4-byte aligned.  Stream-ordered, no allocation. */
int64_t dinoseg_ncut_graph_bytes(int32_t B, int32_t n);
int32_t dinoseg_ncut_max_cells(void);
int dinoseg_op_ncut_graph(const void* planes, int32_t B, int32_t n, int32_t D, double tau, void* graph, int32_t* degree, void* stream);
int dinoseg_op_ncut_iterate(const void* graph, const int32_t* degree, int32_t B, int32_t n, double eps, const float* z_in, int32_t iters,
                            float* z_out, float* rho, uint8_t* fg, float* eigvec, float* margin, int32_t* seed_cell, void* stream);

/* Addendum: the same rule with a frame's rows dealt to many workgroups (ncut_split.hip).  Opt-in; the entries above are unchanged.
 *
 * The rule is steps 1-8 above, word for word, and every order of summation in it is a function of n alone: the split entries give
 * THE SAME BITS as the entries above in every output wherever both accept n.  Only two things differ: which workgroup computes a
 * row's t_i and y_i (t_i depends on the row and on xv alone, so the owner does not matter), and the cell limit.
 *
 * dinoseg_op_ncut_iterate_split issues iters + 2 plain launches on the caller's stream, ordered by the stream alone -- no grid
 * barrier, no cooperative launch, no flag, no atomic, no graph capture, no host synchronisation:
 *   weights    one workgroup per frame: r and u (step 4) into the scratch;
 *   pass t     (iters launches) B x (ceil(n / R) + [t > 0]) workgroups of 1024 threads, R = rows per workgroup.  Every row workgroup
 *              redundantly prepares the pass's input in its own LDS, in the thread-ownership order of step 6, from the previous
 *              launch's z and y in the scratch -- p = (z + y) / 2, DN(p), DN once more (pass 0: DN(z_in)), xv = z r, S -- so all
 *              hold the same bits; it then walks its R rows and writes their y_i, and its rows' z_i, into the OTHER half of the
 *              ping-pong scratch (workgroups of the same launch still read the old half).  The extra workgroup of a frame forms
 *              rho[t - 1], a record that never feeds back, from the previous launch's z and y in the rule's order;
 *   result     one workgroup per frame: the last p, DN(p) (iters = 0: DN(z_in)), rho[iters - 1] and step 7.  z_out may be z_in for
 *              every iters, 0 included: nothing before this launch writes z_out, and here every element is read and written by
 *              one thread.
 *
 * dinoseg_ncut_split_max_cells() = (160 KiB - 1024 bytes of reduction slots - the 256-byte pad that the last word's pad lanes read)
 * / 4 bytes = 40 640: the one fp32 vector a row workgroup keeps in LDS is xv; every other vector element belongs to one thread and
 * lives in the scratch.  960 x 960 at patch 8 has 14 400 cells.  dinoseg_ncut_split_graph_bytes(B, n) = 8 B n ceil(n / 64);
 * dinoseg_ncut_split_scratch_bytes(B, n) = 24 B n: six fp32 vectors per frame, the two halves of z and of y, r and u.  Nothing scales
 * with n^2.  Both answer -1 for B or n below 1, n above the split limit, or B ceil(n / 64) beyond the launch range.  The scratch
 * holds nothing between calls.
 *
 * rows_per_group: 0 = the library's choice, the smallest multiple of 32 (every wave walks whole pairs of rows) at which the B
 * ceil(n / R) row workgroups of a pass are at most 256, one per compute unit: all of them run at once and the redundant preparation
 * is paid once per pass; but never more than 256 rows (measured faster at batch 32 than one round of larger groups).  >= 1 is
 * taken as given (above n: n).  The bits do not depend on it.
 *
 * dinoseg_op_ncut_graph_split runs the graph launch of dinoseg_op_ncut_graph unchanged; only the host's cell limit differs.
 *
 * Refused (-1, the message names the entry, nothing is launched): everything the entries above refuse, with
 * dinoseg_ncut_split_max_cells() as the cell limit; a null scratch or one not 16-byte aligned; rows_per_group below 0; B (ceil(n / R)
 * + 1) beyond the launch range. */
int32_t dinoseg_ncut_split_max_cells(void);
int64_t dinoseg_ncut_split_graph_bytes(int32_t B, int32_t n);
int64_t dinoseg_ncut_split_scratch_bytes(int32_t B, int32_t n);
int dinoseg_op_ncut_graph_split(const void* planes, int32_t B, int32_t n, int32_t D, double tau, void* graph, int32_t* degree,
                                void* stream);
int dinoseg_op_ncut_iterate_split(const void* graph, const int32_t* degree, int32_t B, int32_t n, double eps, const float* z_in,
                                  int32_t iters, int32_t rows_per_group, float* z_out, float* rho, uint8_t* fg, float* eigvec,
                                  float* margin, int32_t* seed_cell, void* scratch, void* stream);

/* ---- connected components of a label map and their object table (what scipy.ndimage.label plus find_objects give on the host: how
 * many objects a label map holds, which pixels each one owns, its area and its box).  No reference counterpart.  components.hip.
 * Everything is an integer; the result is a function of the input alone, bit for bit, from run to run.
 *
 * Input: labels int32 [B][H][W]; connectivity 4 or 8; ignore int32.
 *
 * 1. Void.  A pixel is void when its label is negative or equals `ignore` (ignore = -1: negatives only).
 * 2. Joined.  Two non-void pixels of one frame are joined when they are 4-neighbours ((x +- 1, y) or (x, y +- 1)) and carry the same
 *    label; with connectivity = 8 also when they are diagonal neighbours ((x +- 1, y +- 1)) with the same label.
 * 3. Components are the classes of the transitive closure of "joined".  Frames never interact.
 * 4. The first pixel of a component is its pixel with the smallest linear index y W + x.
 * 5. The components of a frame are numbered 0, 1, .. in ascending order of their first pixels (raster order, the order of
 *    scipy.ndimage.label on a one-class map).
 *
 * Output:
 *   ids     int32 [B][H][W]   the number of the pixel's component, -1 on void pixels;
 *   count   int32 [B]         the true number of components of the frame, however large;
 *   the object table of M = max_objects rows per frame: first int32 [B][M] (the first pixel's linear index), label int32 [B][M]
 *   (the component's label), area int32 [B][M] (its pixel count), box int32 [B][M][4] = (x0, y0, x1, y1), half-open: x0 / y0 the
 *   smallest x / y of any of its pixels, x1 / y1 the largest plus one.  Row k < min(count, M) describes component k; rows from
 *   min(count, M) on hold first = -1, label = -1, area = 0, box = 0.  ids and count do not depend on M;
 *   status  int32 [B]         0.  (1 would say that a loop of the launches below ran into its step cap, which their invariant rules
 *                             out: every parent slot only ever receives a smaller index, so every chain strictly descends.)
 *
 * Launches (five, plain, on the caller's stream behind a memset of status; ordered by the stream alone: no cooperative launch, no grid
 * barrier, no flag between workgroups, no host synchronisation, no allocation): a union-find per 64 x 32 tile in LDS rooted at the
 * tile's smallest index; unions across tile edges by integer atomicMin on the parent array (the fixed point -- every component rooted
 * at its smallest index -- is unique, so the arrival order does not show); every pixel's root and, per row segment of 64 pixels, the
 * bit mask of the pixels that are roots; per frame the prefix sum of the masks' popcounts (segments are in raster order) and count;
 * ids = the prefix of the root's segment + the popcount of its mask below the root, and the table by integer add / min / max, one per
 * wave and distinct component.  No floating-point atomic anywhere.
 *
 * scratch: dinoseg_components_scratch_bytes(B, H, W) = 4 B H W + 12 B H ceil(W / 64) bytes rounded up to 16, 16-byte aligned device
 * memory (the parent array, the masks, the prefixes); it holds nothing between calls.  Host only; -1 for refusable arguments.
 *
 * Refused on the host (-1, the message names the entry) before anything is launched: a null pointer; B, H or W below 1; H or W above
 * 8192; B H W >= 2^31; max_objects outside 1 .. 2^20; connectivity outside {4, 8}; a 32-bit array not 4-byte aligned or the scratch
 * not 16-byte aligned. */
#define DINOSEG_COMPONENTS_MAX_SIDE 8192
#define DINOSEG_COMPONENTS_MAX_OBJECTS (1 << 20)
int64_t dinoseg_components_scratch_bytes(int32_t B, int32_t H, int32_t W);
int dinoseg_op_components(const int32_t* labels, int32_t B, int32_t H, int32_t W, int32_t connectivity, int32_t ignore,
                          int32_t max_objects, int32_t* ids, int32_t* count, int32_t* first, int32_t* label, int32_t* area, int32_t* box,
                          int32_t* status, void* scratch, void* stream);

/* ---- multi-object discovery: recursive normalized cuts (MaskCut, the discovery step of CutLER: cut the graph, keep the connected
 * component around the seed cell, paint its cells out of the graph, cut again).  No reference counterpart.  maskcut.hip.  The cut is
 * dinoseg_op_ncut_iterate_split and the components are dinoseg_op_components, both unchanged; what is new is the glue that makes a
 * round a function of the previous one on the device.  On the 1-bit graph "paint the object out" is graph &= alive and the degree a
 * popcount, so everything new is an integer or a sign operation: the result is a function of the input alone, bit for bit.
 *
 * Per frame (frames are independent): n = hp wp cells, W = ceil(n / 64), K = max_objects rounds t = 0 .. K - 1.  State: alive, one
 * bit per cell, [B][W] uint64 words, cell i at bit i % 64 of word i / 64, pad bits zero.  Before round 0 every cell is alive and
 * score[b][i][0] = 0 is written (once).
 *
 * 1. Mask (dinoseg_op_ncut_mask).  graph[i][w] <- alive_i ? graph[i][w] & alive[w] : 0, in place; degree[i] = popcount of the new row,
 *    exact.  Pad bits stay zero; a symmetric graph stays symmetric.  Bits are only ever cleared, so masking the previous round's
 *    graph with the new alive equals masking the original graph: one graph buffer serves all rounds.  Dead cells stay in the graph
 *    as nodes joined to nothing: every pair with a dead cell weighs eps, which is what MaskCut's feats * (1 - painting) gives under
 *    TokenCut's binary affinity.  Steps 4-7 of dinoseg_op_ncut_graph apply to the masked graph unchanged, with n the FULL cell count.
 * 2. Cut.  dinoseg_op_ncut_iterate_split on the masked graph and degree.  Every round starts from the SAME start vector z_start,
 *    which no round writes.  Its result is fg_t, margin_t, seed_cell_t, eigvec_t, rho_t.
 * 3. Candidates.  cand_i = (fg_t[i] != 0 && alive_i) ? 1 : 0 as int32 [B][hp][wp]; ids = the ids of dinoseg_op_components on it with
 *    ignore = 0 and the connectivity given (its table is not used).
 * 4. Select (dinoseg_op_maskcut_select).  s = seed_cell_t.  k = ids[s] where 0 <= s < n, alive_s and fg_t[s] != 0, else -1;
 *    found_t = k >= 0 (a dead seed or a background seed gives 0).  cells_t[i] = found_t && ids[i] == k.  area_t = the count of cells_t;
 *    box_t = (x0, y0, x1, y1), half-open, in CELLS (x = i % wp, y = i / wp), all four 0 when not found.  alive &= ~cells_t.
 *    score[b][i][t + 1] = cells_t[i] ? margin_t[i] : -|margin_t[i]| (margin_t[i] with the sign bit set: the bits of torch.where(cells,
 *    margin, -margin.abs())).  No other channel of score is touched.  Nothing is summed in floating point; the area and the box are
 *    integer add / min / max in one workgroup per frame.
 * 5. Pixel labels: dinoseg_op_upsample_argmax, unchanged, on score [B, n, K + 1]: 0 is background, t + 1 is object t, ties go to the
 *    lower index.
 * 6. No early stop (there is no host synchronisation).  A round with found_t = 0 leaves alive unchanged, so every later round repeats
 *    it bit for bit.  count[b] = the number of rounds with found = 1.
 *
 * Deviations from MaskCut: the points are the tokens of dinoseg_features_hw, not last-block keys; the lazy power iteration replaces
 * eigh; the three-corner reversal of the partition, the IoU > 0.5 rejection, the 1 % area rejection and the CRF post-processing are
 * not done; a not-found round does not end the loop, it repeats.
 *
 * dinoseg_op_maskcut runs the K rounds on the caller's stream: an init launch; per round the mask launch, the iters + 2 launches of
 * the split cut, one launch that forms cand and copies the round's fg / margin / eigvec / seed_cell / rho into slot t of the
 * caller's arrays, the launches of dinoseg_op_components, the select launch; at the end one launch for count.  Nothing synchronises
 * with the host, nothing allocates, there are no flags and no atomics of its own.  IT DESTROYS THE CALLER'S GRAPH AND DEGREE: after
 * the call they are those of the last round's mask.  Outputs: cells uint8 [B][K][n]; found uint8 [B][K]; area int32 [B][K]; box
 * int32 [B][K][4]; score fp32 [B][n][K + 1]; count int32 [B]; fg uint8 [B][K][n]; margin, eigvec fp32 [B][K][n]; seed_cell int32
 * [B][K]; rho fp32 [B][K][iters] (may be NULL with iters = 0).  z_start fp32 [B][n].
 *
 * dinoseg_maskcut_scratch_bytes(B, hp, wp, K): the split scratch, the components scratch and its one-row table, alive, cand, ids,
 * the working z and the round's working fg / margin / eigvec / seed_cell / rho (rho at the 4096 passes the cut accepts), each part
 * rounded up to 16 bytes; it does not grow with K.  Host only; -1 for refusable arguments.  The scratch holds nothing between calls.
 *
 * Refused (-1, the message names the entry, nothing is launched, the outputs, the scratch and the graph stay untouched): a null
 * pointer (rho with iters = 0 is optional); everything dinoseg_op_ncut_iterate_split refuses about B, n, eps, iters and
 * rows_per_group and dinoseg_op_components about B, hp, wp; K outside 1 .. 16; t outside 0 .. K - 1; connectivity not 4 or 8; the
 * graph or alive not 8-byte aligned, a 32-bit array not 4-byte aligned, the scratch not 16-byte aligned. */
#define DINOSEG_MASKCUT_MAX_OBJECTS 16
int64_t dinoseg_maskcut_scratch_bytes(int32_t B, int32_t hp, int32_t wp, int32_t K);
int dinoseg_op_ncut_mask(void* graph, int32_t* degree, const void* alive, int32_t B, int32_t n, void* stream);
int dinoseg_op_maskcut_select(const int32_t* ids, const uint8_t* fg, const float* margin, const int32_t* seed_cell, void* alive, int32_t B,
                              int32_t hp, int32_t wp, int32_t K, int32_t t, uint8_t* cells, uint8_t* found, int32_t* area, int32_t* box,
                              float* score, void* stream);
int dinoseg_op_maskcut(void* graph, int32_t* degree, int32_t B, int32_t hp, int32_t wp, double eps, const float* z_start, int32_t iters,
                       int32_t rows_per_group, int32_t connectivity, int32_t K, uint8_t* cells, uint8_t* found, int32_t* area,
                       int32_t* box, float* score, int32_t* count, uint8_t* fg, float* margin, float* eigvec, int32_t* seed_cell,
                       float* rho, void* scratch, void* stream);

/* ---- fine-tune step (replaces DINOSeg.training_step + autograd + optimizer.step, pl_torch_modules.py:258-268) ---- */

/* Bind (or, with NULL, unbind) the fp32 gradient buffer of a parameter, same shape as the bound weight.  A parameter
 * without a bound gradient is frozen; with no "dino.*" gradient bound the backward stops at the head
 * (freeze_bb, pl_torch_modules.py:434-436). */
int dinoseg_bind_grad(dinoseg_handle* h, const char* name, float* dev_ptr);

/* One training step on this rank's B frames: forward with saved activations, loss = F.nll_loss(log_probs, labels)
 * (mean over the patches whose label is not -100; labels int64 on device), backward.  Every bound gradient buffer is OVERWRITTEN with
 * d loss / d parameter; *loss_out (device float) receives the loss; logp_out (optional) the log-probabilities.
 * Call dinoseg_refresh_weights() after the optimiser changed the parameters. */
int dinoseg_train_step(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, const int64_t* labels,
                       float* loss_out, float* logp_out, void* stream);

/* The two halves of the step, for callers that own the loss (torch.autograd: `loss = F.nll_loss(model(x), y); loss.backward()`,
 * pl_torch_modules.py:261-266).  dinoseg_train_forward = DINOSeg.forward with the activations kept (logp_out fp32
 * [B*(r/8)^2, n_classes]); dinoseg_backward takes dlogp = d loss / d log-probabilities (same shape, fp32, device) and
 * OVERWRITES every bound gradient buffer with d loss / d parameter.  The saved forward stays valid until the next
 * dinoseg_train_forward / dinoseg_train_step on this handle.  dinoseg_train_step(labels) == train_forward + nll_loss +
 * backward, through the same kernels (same d logits bit for bit). */
int dinoseg_train_forward(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t r, float* logp_out, void* stream);
/* The two at H x W frames (vision_transformer.py:202-233; see dinoseg_prepare_resolution_hw): labels / logp_out have B*(H/8)*(W/8)
 * rows; the pos_embed gradient is the transpose of the two-axis resample. */
int dinoseg_train_step_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, const int64_t* labels,
                          float* loss_out, float* logp_out, void* stream);
int dinoseg_train_forward_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, float* logp_out,
                             void* stream);
int dinoseg_backward(dinoseg_handle* h, const float* dlogp, void* stream);
/* The step on PIXEL labels: dinoseg_train_forward_hw, then dinoseg_op_upsample_nll of its log-probs against labels int64 [B, OH, OW]
 * (OH >= H/patch, OW >= W/patch; ignore_index outside [0, n_classes)), then dinoseg_backward of that d logp -- the same three
 * launches sequences, so the same loss and gradients bit for bit under option "deterministic".  The d logp buffer and the loss
 * scratch live in the handle (sized on first use: warm the handle before capturing); an out-of-range label latches the flag
 * dinoseg_train_status reads.  *loss_out (device float) receives the loss, logp_out (optional) the low-res log-probabilities. */
int dinoseg_train_step_dense_hw(dinoseg_handle* h, const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t OH, int32_t OW,
                                const int64_t* labels, int32_t ignore_index, float* loss_out, float* logp_out, void* stream);

/* Gradient stages of the backward, for overlapping the data-parallel all-reduce with it (no reference
 * counterpart: the reference trains on one GPU).  dinoseg_backward / dinoseg_train_step record an event on their stream when the
 * gradients of a stage are final: stage 0 = head (clf.*), stage 1 + k = dino.norm.* and dino.blocks[n_blocks-1-k].*,
 * stage n_blocks + 1 = embeddings (cls_token, pos_embed, patch_embed).  dinoseg_grad_stages returns n_blocks + 2;
 * dinoseg_stream_wait_grad_stage makes `stream` (e.g. the communication stream) wait for stage `stage` of the LAST backward
 * enqueued on this handle, without blocking the host. */
int dinoseg_grad_stages(const dinoseg_handle* h);
int dinoseg_stream_wait_grad_stage(dinoseg_handle* h, int32_t stage, void* stream);

/* Label check of the training steps since the last call.  F.nll_loss ignores rows labelled -100 (ignore_index; the mean is
 * over the other rows) and raises for any other label outside [0, n_classes): the kernels treat such a row as ignored
 * and latch a flag; *bad_labels receives it (1 = at least one out-of-range label was seen) and the flag is cleared.
 * Synchronises `stream`. */
int dinoseg_train_status(dinoseg_handle* h, int32_t* bad_labels, void* stream);

/* Fused Adam (decoupled = 0: torch.optim.Adam, weight decay added to the gradient) / AdamW (decoupled = 1) update of
 * one tensor; step counts from 1; grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
int dinoseg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int32_t decoupled, int32_t step, float grad_scale, void* stream);

/* The same update for `count` parameters in one launch per 64 tensors (host arrays of device pointers and element counts):
 * what optimizer.step() does for the whole parameter list (pl_torch_modules.py:258-259). */
int dinoseg_adam_step_multi(int32_t count, float* const* p, const float* const* g, float* const* m, float* const* v,
                            const int64_t* n, float lr, float beta1, float beta2, float eps, float weight_decay,
                            int32_t decoupled, int32_t step, float grad_scale, void* stream);

/* Per-kernel-class timing with HIP events recorded on the forward's stream (used by bench.py for the
 * roofline leg).  level 0 = off, 1 = the dominant kernel only (fused attention), 2 = every class.
 * dinoseg_profile_read() waits for the recorded events, writes the summed milliseconds and launch counts
 * per class (arrays of DINOSEG_PROF_COUNT) and clears the records. */
enum { DINOSEG_PROF_PATCH = 0, DINOSEG_PROF_LN = 1, DINOSEG_PROF_QKV = 2, DINOSEG_PROF_ATTN = 3, DINOSEG_PROF_PROJ = 4,
       DINOSEG_PROF_FC1 = 5, DINOSEG_PROF_FC2 = 6, DINOSEG_PROF_HEAD = 7,
       DINOSEG_PROF_ATTN_BWD = 8,      /* the flash-style attention backward of the fine-tune step: prep + dQ + dK,dV kernels */
       DINOSEG_PROF_COUNT = 9 };
int dinoseg_profile(dinoseg_handle* h, int32_t level);
int dinoseg_profile_read(dinoseg_handle* h, float* ms_sum, int32_t* counts);

/* Process-wide switches.  Keys:
 *   "streams"    2 [default] / 1: with 2, dinoseg_forward runs a batch of >= "split_min" (default 8) frames as two half-batches,
 *                the first on the caller's stream, the second on an internal stream forked from / joined to it by events (the
 *                call stays stream-ordered and capturable; outputs bit-identical to the one-stream run in every precision -- each
 *                half takes the kernel routes of the whole batch: tests/test_model_gpu.py::test_two_stream_split_equals_one_stream*;
 *                +6 to +9 % frames/s at B = 32 on MI355X: one half's attention fills the CUs the other half's GEMM tails and
 *                memory phases leave idle); 1 = one stream;
 *   "fp16_patch_planes" 1 [default] / 2: precision fp16 only -- the patch embedding on one fp16 plane, or on bf16 hi+lo planes;
 *   "op_fmt"     0 [default] / 1: operand format of the single-plane stand-alone ops (dinoseg_op_*: tests, tools): bf16 / fp16;
 *   "gemm_big"   1 [default] = the persistent 256x384 (bf16) / 128x384 (bf16x3) GEMM where it applies, 0 = always the 128x128
 *                kernel, 2 = wherever its shape rules allow;
 *   "gemm_ln"    1 [default] = qkv / fc1 through the LayerNorm-fused kernels where measured faster, 0 never, 2 wherever supported;
 *   "mlp_fused"  1 [default] = the MLP half of a block (LayerNorm2, fc1, GELU, fc2, residual) as ONE launch where it applies (bf16
 *                mode, embed_dim 384, batches of >= 4 frames at 480x480), 0 never, 2 wherever the shape allows;
 *   "proj_fused" 1 [default] = where that launch runs, it also carries the block's attention output projection + residual
 *                (x += proj(ctx) + b first: vision_transformer.py:104-105), 0 = the projection stays a GEMM launch of its own;
 *   "qkv_fused"  0 [default] / 1 = ... and LayerNorm1 + qkv of the next block at its end (blocks 1.. have no LN + qkv launch then:
 *                +1 % frames/s on one stream, none on two -- the tail writes Q / K / V in the same HBM burst as the launch it replaces);
 *   "mlp_variant" accepted and ignored (the one-wave-per-SIMD build of the fused MLP kernel was removed in round 4);
 *   "train_streams" 2 [default] = dinoseg_backward / dinoseg_train_step run the blocks' weight-gradient GEMMs on an internal stream
 *                beside the input-gradient chain (forked from / joined to the caller's stream by events: stream-ordered, capturable),
 *                1 = everything on the caller's stream (use it when several processes share one GPU);
 *   "deterministic" 0 [default] / 1: the fine-tune step sums the loss, the bias gradients and the LayerNorm gamma / beta gradients from
 *                per-block partials in a FIXED order instead of fp32 atomics (the side stream's bias sums in their own scratch region):
 *                two runs from the same state are bit-identical, at 4-5 % of the step (SURVEY.md section 8e "fixed reduction tree"; with world_size > 1 the
 *                all-reduce's own order is RCCL's); one training step at a time per process while it is on;
 *   "op_v_bf16"  0 [default] / 1: dinoseg_op_attention with fp16 hi + lo planes takes V as bf16 hi + lo planes (what the forward hands
 *                the zero-reference kernels at large batch: attention_za.hip);
 *   "splitk_tiles" 512 [default]: partial 128x128 tiles of one weight-gradient GEMM (<= 768);
 *   "route_ab"   0 [default]: A/B switches of dispatch routes that do not change results (bit 0: 128-row tiles for the residual GEMMs
 *                of a small batch; bit 1: the one-wave-per-row LayerNorm backward; bit 2: the weight-gradient GEMM's 2-D grid);
 *   "attn_variant", "gemm_dbg", "attn_dbg": kernel A/B and timing-ablation switches (tools/bench_ops.py; attn_variant's bits:
 *                dino_amd/csrc/kernels.h -- default 11 | 1024 | 65536: from four rounds of workgroups on the attention runs its tile loop
 *                as a generated assembly pipeline, attention_za.hip, bit-identical to the compiled kernel);
 *   "mlp_fused_min_rows" 12000 [default], "mlp_fused3_min_rows" 10000 [default]: the fewest token rows at which "mlp_fused" = 1 takes the
 *                fused launch, on one plane / on hi + lo planes;
 *   "qkv_fused3" 1 [default], "qkv_fused4" 1 [default]: "qkv_fused" for the hi + lo launch / for the one-wave-per-SIMD launch;
 *   "mlp_fused4" 0 [default] / 1: one-plane modes -- the fused projection + MLP launch with one wave per SIMD (read at refresh and at
 *                every forward: setting it between two refreshes can switch the route off, never on);
 *   "gemm_rs"    3 [default]: the row-stationary streaming GEMMs (embed_dim 768, one plane, >= "gemm_rs_min_rows" rows, default 24000),
 *                a bit per linear: 1 = mlp.fc1, 2 = attn.qkv, 4 = attn.proj and mlp.fc2 (stored & 7; read like "mlp_fused4");
 *   "gemm_rs_ln" 1 [default] / 0: ... with the LayerNorm in front of qkv / fc1 in the kernel's prologue (read at refresh only);
 *   "mlp_stagger" 0 [default], "mlp_grid" 0 [default]: experiment switches of the fused MLP launch (dino_amd/csrc/kernels.h).
 * A value is stored normalised (a flag as 0 / 1, "gemm_rs" & 7, "split_min" >= 2, "fp16_patch_planes" 1 or 2); a refused one ("op_fmt"
 * outside 0 / 1, an unknown key) returns -1 and stores nothing. */
int dinoseg_set_option(const char* key, int32_t value);
/* Reads the stored (normalised) value of one key of dinoseg_set_option into *value; -1 for an unknown key or a null pointer, *value untouched. */
int dinoseg_get_option(const char* key, int32_t* value);
/* The key in row `index` (0 ..) of the option table, NULL outside it: enumerates the keys of dinoseg_set_option / dinoseg_get_option. */
const char* dinoseg_option_name(int32_t index);

/* Bytes of library-owned device memory a (B, r) forward needs (activations + packed weights). */
int64_t dinoseg_workspace_bytes(const dinoseg_handle* h, int32_t B, int32_t r);
/* ... of a (B, H x W) forward (vision_transformer.py:224-233: hp*wp + 1 tokens per frame) */
int64_t dinoseg_workspace_bytes_hw(const dinoseg_handle* h, int32_t B, int32_t H, int32_t W);
/* Counts the events that invalidate device addresses or cached contents a CAPTURED dinoseg_forward has baked in: a re-allocation of
 * the activation workspace or of the packed weights, a re-computation of the resampled position embedding (another resolution).
 * A caller that replays a HIP graph of the forward compares it with the value read after the capture and re-captures on a change
 * (DINOSeg.predict does: pl_torch_modules.py:276-300 is a single-frame call, launch-bound when issued kernel by kernel). */
int64_t dinoseg_state_generation(const dinoseg_handle* h);

/* ---- stand-alone operators (same kernels the forward uses; exported for unit parity tests) ------------- */

/* fp32 [rows, cols] -> bf16 planes [planes][rows_pad][cols_pad] (zero padded); plane stride in elements */
int dinoseg_op_pack(const float* src, int32_t rows, int32_t cols, void* dst, int64_t plane_stride, int32_t rows_pad,
                    int32_t cols_pad, int32_t planes, void* stream);

/* C[M,N] = A[M,K] . W[N,K]^T on packed planes.  epi: 0 plain(+bias) -> out_f32; 1 residual: out_f32 += acc+bias;
 * 2 GELU(erf) -> out_bf16 planes; 3 ReLU -> out_bf16 planes.  (aten::addmm of vision_transformer.py:60-63,75,105) */
int dinoseg_op_gemm(const void* A, int64_t a_plane, int32_t lda, const void* W, int64_t w_plane, int32_t M, int32_t N,
                    int32_t K, int32_t planes, int32_t epi, const float* bias, float* out_f32, void* out_bf16,
                    int64_t out_plane, int32_t ldo, void* stream);

/* attn.qkv GEMM with the head-scatter epilogue (vision_transformer.py:82): Q (times qscale), K, V, each
 * [planes][B,H,npad,64]; M = B*ntok rows.  With fp16 hi + lo planes (option "op_fmt" 1, planes 2) option "op_v_bf16" 1 writes V as
 * bf16 hi + lo planes, the form dinoseg_op_attention reads under the same option (the forward's default parity mode at large batches). */
int dinoseg_op_qkv_gemm(const void* A, int64_t a_plane, const void* W, int64_t w_plane, const float* bias, int32_t B,
                        int32_t ntok, int32_t npad, int32_t heads, int32_t planes, float qscale, void* q, void* k,
                        void* v, int64_t qkv_plane, void* stream);

/* The patch-embedding GEMM (the conv of vision_transformer.py:153,157 as a GEMM, + bias + position rows, :224-235):
 *     X_out[b (n_patches + 1) + 1 + p, :] = A[b n_patches + p, :] . W^T + bias + pos[1 + p, :]
 * A: planes x [B n_patches][K] (the patch-gather matrix), W: planes x [N][K], both in the format of option "op_fmt"; bias fp32 [N];
 * pos fp32 [n_patches + 1][N]; X_out fp32 [B (n_patches + 1)][N].  The CLS rows b (n_patches + 1) are not written.  N % 128 == 0,
 * K % 64 == 0. */
int dinoseg_op_patch_gemm(const void* A, const void* W, const float* bias, const float* pos, int32_t B, int32_t n_patches, int32_t N,
                          int32_t K, int32_t planes, float* X_out, void* stream);

/* dinoseg_op_gemm as dinoseg_train_forward launches it.  epi 1: out_f32 = resid + A W^T + bias with resid != out_f32 (attn.proj and
 * mlp.fc2 read the residual stream of one buffer and write the next); epi 2: out_bf16 planes = GELU(z), z = A W^T + bias, and
 * aux_out planes [planes][M][ldo] (plane stride aux_plane) = z itself, kept for the backward's gelu' -- bf16 operands only.
 * N % 128 == 0, K % 64 == 0, lda % 8 == 0 (the 128 x 128 kernel). */
int dinoseg_op_gemm_train(const void* A, int64_t a_plane, int32_t lda, const void* W, int64_t w_plane, int32_t M, int32_t N, int32_t K,
                          int32_t planes, int32_t epi, const float* bias, const float* resid, float* out_f32, void* out_bf16,
                          int64_t out_plane, int32_t ldo, void* aux_out, int64_t aux_plane, void* stream);

/* Slab-major bf16 copy of an fp32 weight W [N][K] for dinoseg_op_ln_gemm (dst holds dinoseg_op_ln_gemm_slab_elems(N, K, planes)
 * bf16 elements; -1 = unsupported shape): [column tile][k-step][plane][rows][32 k], pre-swizzled, zero padded. */
int64_t dinoseg_op_ln_gemm_slab_elems(int32_t N, int32_t K, int32_t planes);
int dinoseg_op_pack_slabs(const float* W, int32_t N, int32_t K, int32_t planes, void* dst, void* stream);

/* LayerNorm (eps as given) fused into the GEMM that consumes it: out = epilogue(LN(X) W^T + bias), X fp32 [M, K] (K = 384);
 * Wp = the slab-major copy made by dinoseg_op_pack_slabs (w_plane is ignored).
 * epi 4 (QKV): scatter to q (x qscale), k, v [planes][B*heads][npad][64]; epi 2 (GELU): out_bf16 [planes][M][N].
 * a_out / aux_out (nullable): the normalised planes [planes][M][K] / the pre-GELU planes, kept by training forwards.
 * Replaces nn.LayerNorm + nn.Linear pairs vision_transformer.py:123 -> :75 and :135 -> :60-61. */
int dinoseg_op_ln_gemm(const float* X, const float* gamma, const float* beta, float eps, const void* Wp, int64_t w_plane,
                       const float* bias, int32_t M, int32_t N, int32_t K, int32_t planes, int32_t epi, void* out_bf16,
                       int64_t out_plane, void* q, void* k, void* v, int64_t qkv_plane, int32_t ntok, int32_t npad,
                       int32_t heads, float qscale, void* a_out, void* aux_out, void* stream);

/* The whole MLP half of a block in one launch (bf16 mode, embed_dim 384, hidden 1536):  X += fc2(gelu(fc1(LayerNorm(X)))),
 * X fp32 [M, 384] updated in place.  Replaces Block.forward's `x = x + self.mlp(self.norm2(x))` (vision_transformer.py:135 ->
 * :59-65): LayerNorm2, fc1, exact GELU (fitted form of the bf16 mode), fc2, residual add; the hidden activation stays on chip.
 * Wp = both weights re-packed in MFMA fragment order by dinoseg_op_pack_mlp (dinoseg_op_mlp_fused_pack_elems(D, F) bf16
 * elements; 0 = unsupported shape).
 * Range with fp16 operands (option "op_fmt" 1; the same holds for dinoseg_op_proj_mlp_fused, dinoseg_op_block_tail_fused and the
 * mlp_fused4.hip entries below): the hidden activation is NOT saturated -- a pre-activation beyond 65504 is stored as inf and the row
 * comes back NaN (0 x inf in fc2); up to 65504 it is exact.  b1 reaches the accumulator as three fp16 pieces: |b1| <= 65504, and an
 * |b1| < 0.5 may lose up to 2^-25.  dinoseg_op_gemm's GELU epilogue, dinoseg_op_gemm_rs and the hi + lo entries (mlp_fused3.hip) saturate at
 * +-65504 instead.  Measured and not changed: profiles/fused_gelu_saturation_ab.md; DESIGN.md (precision modes). */
int64_t dinoseg_op_mlp_fused_pack_elems(int32_t D, int32_t F);
int dinoseg_op_pack_mlp(const float* W1, const float* W2, int32_t D, int32_t F, void* dst, void* stream);
int dinoseg_op_mlp_fused(float* X, const float* gamma, const float* beta, float eps, const void* Wp, const float* b1,
                         const float* b2, int32_t M, int32_t D, int32_t F, void* stream);

/* The same launch with the block's attention output projection in front (role-split kernel only):
 *     X += ctx . Wproj^T + bproj;   X += fc2(gelu(fc1(LayerNorm(X))))
 * = Attention.forward's `x = self.proj(x)` + Block.forward's two residual adds (vision_transformer.py:104-105, :123, :135).
 * ctx: bf16 [M, 384] (the attention output, row stride 384); Wproj: the [384, 384] weight re-packed by dinoseg_op_pack_proj
 * (dinoseg_op_proj_pack_elems(D) bf16 elements; 0 = unsupported width).  Library option "proj_fused" (default 1) makes
 * dinoseg_forward use it wherever the fused MLP runs. */
int64_t dinoseg_op_proj_pack_elems(int32_t D);
int dinoseg_op_pack_proj(const float* W, int32_t D, void* dst, void* stream);
int dinoseg_op_proj_mlp_fused(float* X, const void* ctx, const void* Wproj, const float* bproj, const float* gamma,
                              const float* beta, float eps, const void* Wp, const float* b1, const float* b2, int32_t M,
                              int32_t D, int32_t F, void* stream);

/* Row-stationary streaming GEMMs of the wide model (gemm_rs.hip; one operand plane in the format of option "op_fmt", embed_dim 768): what
 * nn.Linear computes in Attention.qkv / Mlp.fc1 (K = 768: epi 4 = the Q / K / V scatter of dinoseg_op_qkv_gemm, epi 2 = GELU into out16 [M][ldo])
 * and in Attention.proj / Mlp.fc2 with the residual add (N = 768, epi 1: x_inout [M][768] += A W^T + bias) -- vision_transformer.py:75, :60-61, :105,
 * :63 + :123 / :135.  Wp: the fp32 weight [N][K] re-packed by dinoseg_op_pack_rs (N * K 16-bit elements; kind 0 for epi 2 / 4, kind 1 for epi 1).
 * dinoseg_forward uses them for ViT-B/8 batches of >= option "gemm_rs_min_rows" rows; option "gemm_rs" is a bit per linear (1 mlp.fc1,
 * 2 attn.qkv, 4 attn.proj + mlp.fc2; default 3: the two that measure faster than the generic kernel). */
int dinoseg_op_pack_rs(const float* W, int32_t N, int32_t K, int32_t kind, void* dst, void* stream);
/* ... with the LayerNorm in front of the linear inside the launch (epi 2 / 4 only): `self.qkv(self.norm1(x))` / `self.fc1(self.norm2(x))`
 * (vision_transformer.py:122 -> :75, :134 -> :60), X fp32 [M][K] rows, K = 768.  The kernel's prologue computes (x - mean) rstd per row; the LayerNorm's
 * weight and bias ride in the packed copy: dinoseg_op_pack_rs_ln writes W . diag(gamma) in fragment order (N * K 16-bit elements) and the folded bias
 * bias + W beta ([N] fp32) -- LayerNorm(x) W^T + b = ((x - mean) rstd) (W diag(gamma))^T + (b + W beta).  Library option "gemm_rs_ln" (default 1, read by
 * dinoseg_refresh_weights). */
int dinoseg_op_pack_rs_ln(const float* W, const float* gamma, const float* beta, const float* bias, int32_t N, int32_t K, void* dst_w,
                          float* dst_bias, void* stream);
int dinoseg_op_ln_gemm_rs(const float* X, float eps, const void* Wp, const float* bias_folded, int32_t M, int32_t N, int32_t K, int32_t epi,
                          void* out16, int32_t ldo, void* q, void* k, void* v, int32_t ntok, int32_t npad, int32_t heads, float qscale,
                          void* stream);
int dinoseg_op_gemm_rs(const void* A, int32_t lda, const void* Wp, const float* bias, int32_t M, int32_t N, int32_t K, int32_t epi,
                       float* x_inout, void* out16, int32_t ldo, void* q, void* k, void* v, int32_t ntok, int32_t npad, int32_t heads,
                       float qscale, void* stream);

/* The same fusion on hi + lo operand planes (the parity modes; mlp_fused3.hip), one launch for
 *     X += ctx . Wproj^T + bproj;   X += fc2(gelu(fc1(LayerNorm(X))))      (vision_transformer.py:104-105, :123, :135 -> :59-65)
 * ctx: the attention output as two planes [2][M][384] (hi, then lo at + ctx_plane elements), or null = the MLP half only (bproj unused).
 * Wp: dinoseg_op_pack_mlp3's copy (dinoseg_op_mlp3_pack_elems(D, F) 16-bit elements; 0 = unsupported shape): Wproj, W1, W2 -- and optionally the NEXT
 * block's Wqkv [1152, 384] -- as hi + lo fragment pairs in the order the kernel walks them, with the LayerNorms folded in: norm2's weight into the columns
 * of W1 and its bias into b1, the next block's norm1 into Wqkv / bqkv (LayerNorm(x) W^T + b = ((x - mean) rstd) (W diag(gamma))^T + (b + W beta)); the kernel
 * computes (x - mean) rstd only.  fmt: 0 = bf16 planes, 1 = fp16 planes.
 * dinoseg_op_block_tail_fused3: ... and LayerNorm1 + the qkv projection of the NEXT block at the end of the same launch
 * (vision_transformer.py:122 -> :75): afterwards X holds the block's output and q / k / v (each two planes [2][B, heads, npad, 64], lo at
 * + qkv_plane elements; q pre-scaled by qscale; rows >= ntok untouched) hold what LayerNorm + the qkv GEMM would have written from it;
 * v_bf16 (fmt 1 only): V as bf16 planes, what the zero-reference hi + lo attention reads.  M = B * ntok rows.  Library option "qkv_fused3"
 * (default 1) makes dinoseg_forward use it wherever the hi + lo fused launch runs. */
int64_t dinoseg_op_mlp3_pack_elems(int32_t D, int32_t F);
int dinoseg_op_pack_mlp3(const float* Wproj, const float* W1, const float* b1, const float* W2, const float* gamma2, const float* beta2,
                         const float* Wqkv_next, const float* bqkv_next, const float* gamma1_next, const float* beta1_next, int32_t D, int32_t F,
                         int32_t fmt, void* dst, void* stream);
int dinoseg_op_proj_mlp_fused3(float* X, const void* ctx, int64_t ctx_plane, const float* bproj, float eps, const void* Wp, const float* b2,
                               int32_t M, int32_t D, int32_t F, int32_t fmt, void* stream);
int dinoseg_op_block_tail_fused3(float* X, const void* ctx, int64_t ctx_plane, const float* bproj, float eps, const void* Wp, const float* b2,
                                 void* q, void* k, void* v, int64_t qkv_plane, int32_t B, int32_t ntok, int32_t npad, int32_t heads, float qscale,
                                 int32_t v_bf16, int32_t D, int32_t F, int32_t fmt, void* stream);

/* The single-plane fusion with ONE wave per SIMD (mlp_fused4.hip): the same result as dinoseg_op_proj_mlp_fused (fp16 / bf16 operands, the
 * logistic GELU of the benchmark modes), the structure of the hi + lo kernel above -- 128-row items, 32 rows per wave held in registers for
 * the whole item, the weights as one linear stream of 48-KiB slots, LayerNorm2's weight folded into W1's columns and its bias into b1 (the kernel
 * computes (x - mean) rstd).  ctx: [M][384] in the operand format, or null = the MLP half only.  Wp: dinoseg_op_pack_mlp4
 * (dinoseg_op_mlp4_pack_elems(D, F) 16-bit elements; Wproj may be null with ctx == null).  Library option "mlp_fused4" (default 0: it measures
 * equal; set before dinoseg_refresh_weights) makes dinoseg_forward use it instead of dinoseg_op_proj_mlp_fused.
 * vision_transformer.py:104-105, :123, :135 -> :59-65. */
int64_t dinoseg_op_mlp4_pack_elems(int32_t D, int32_t F);
int dinoseg_op_pack_mlp4(const float* Wproj, const float* W1, const float* b1, const float* W2, const float* gamma2, const float* beta2,
                         const float* Wqkv_next, const float* bqkv_next, const float* gamma1_next, const float* beta1_next, int32_t D, int32_t F,
                         int32_t fmt, void* dst, void* stream);
int dinoseg_op_proj_mlp_fused4(float* X, const void* ctx, const float* bproj, float eps, const void* Wp, const float* b2, int32_t M, int32_t D,
                               int32_t F, int32_t fmt, void* stream);
/* ... and LayerNorm1 + the qkv projection of the NEXT block at the end of the same launch (Wp packed with Wqkv_next; as
 * dinoseg_op_block_tail_fused3 on one plane: q / k / v [B, heads, npad, 64] in the operand format, V as bf16, q pre-scaled, rows >= ntok untouched).
 * Library option "qkv_fused4" (default 1). */
int dinoseg_op_block_tail_fused4(float* X, const void* ctx, const float* bproj, float eps, const void* Wp, const float* b2, void* q, void* k, void* v,
                                 int32_t B, int32_t ntok, int32_t npad, int32_t heads, float qscale, int32_t D, int32_t F, int32_t fmt,
                                 void* stream);

/* ... and with LayerNorm1 + the qkv projection of the NEXT block at its end (Block.forward of block i from `x = x + attn` on, then
 * block i+1 up to `qkv = self.qkv(self.norm1(x))`: vision_transformer.py:123, :135, :122 -> :75): after the launch X holds block i's
 * output and q / k / v ([B, heads, npad, 64] bf16 each, q pre-scaled by qscale = 64^-0.5 * log2(e), rows >= ntok untouched) hold what
 * dinoseg_op_ln_gemm(EPI_QKV) would have written from it.  M = B * ntok rows.  Wqkv: the [1152, 384] weight re-packed by
 * dinoseg_op_pack_qkv (dinoseg_op_qkv_pack_elems(D) bf16 elements).  Library option "qkv_fused" (default 0: see there). */
int64_t dinoseg_op_qkv_pack_elems(int32_t D);
int dinoseg_op_pack_qkv(const float* W, int32_t D, void* dst, void* stream);
int dinoseg_op_block_tail_fused(float* X, const void* ctx, const void* Wproj, const float* bproj, const float* gamma2,
                                const float* beta2, float eps, const void* Wp, const float* b1, const float* b2, const void* Wqkv,
                                const float* bqkv, const float* gamma1, const float* beta1, void* q, void* k, void* v, int32_t B,
                                int32_t ntok, int32_t npad, int32_t heads, float qscale, int32_t D, int32_t F, void* stream);

/* fused softmax(q k^T) v (vision_transformer.py:85,101,104); q must be pre-scaled by 64^-0.5 * log2(e).
 * q, k, v: [planes][B,heads,npad,64]; ctx: bf16 planes [planes][B*ntok][heads*64]; lse (optional): fp32 [B,heads,ntok], log2 domain.
 * Pad rows: rows ntok..npad of q, k and v are read with the 64-row tiles they share with real rows and must hold FINITE values -- any
 * finite values, zero is not required.  Every kernel masks them: a pad key gets probability 0 and 0 x finite = 0, so they never
 * reach ctx or lse (bit for bit: tests/test_forward_containment_gpu.py); a NaN or Inf there may (0 x Inf).
 * On inputs whose scores are integers, whose values are small integers and whose sums fit 24 bits, every route is exact: where the row
 * sum is a power of two ctx carries the round-to-nearest-even planes of the exact quotient bit for bit, elsewhere each element lies within
 * the store format's half ulp plus 4 * 2^-24 of it (tests/test_attention_probes_gpu.py).  lse lies within 2 fp32 ulps at the magnitude of
 * the hardware log2's result (assumed, not documented) plus one ulp of lse itself, at any integer shift of the scores up to +-200. */
int dinoseg_op_attention(const void* q, const void* k, const void* v, int64_t qkv_plane, void* ctx, int64_t ctx_plane,
                         float* lse, int32_t B, int32_t heads, int32_t ntok, int32_t npad, int32_t planes, void* stream);

/* nn.LayerNorm over the last dim (vision_transformer.py:303).  out_bf16 / out_f32 may each be NULL. */
int dinoseg_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, int32_t M, int32_t D,
                         void* out_bf16, int64_t out_plane, int32_t planes, float* out_f32, int32_t drop_cls,
                         int32_t ntok, void* stream);

/* interpolate_pos_encoding (vision_transformer.py:202-222): pos_embed fp32 [g*g+1, D] -> out fp32 [o*o+1, D] */
int dinoseg_op_pos_resample(const float* pos_embed, int32_t g, int32_t D, int32_t o, float* out, void* stream);
/* interpolate_pos_encoding with one scale per axis (vision_transformer.py:202-233): out fp32 [oh*ow+1, D]; rows at
 * g / (oh + 0.1), columns at g / (ow + 0.1); the copy only when oh == ow == g (:205) */
int dinoseg_op_pos_resample_hw(const float* pos_embed, int32_t g, int32_t D, int32_t oh, int32_t ow, float* out, void* stream);

/* patch gather (+ fused Normalize for uint8 input) -> bf16 planes [planes][B*(r/8)^2][192] */
int dinoseg_op_patch_gather(const void* x, int32_t x_kind, int32_t B, int32_t r, void* out, int64_t out_plane,
                            int32_t planes, void* stream);
/* ... of H x W frames (PatchEmbed, vision_transformer.py:153-157): [planes][B*(H/8)*(W/8)][192], patches row-major */
int dinoseg_op_patch_gather_hw(const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, void* out, int64_t out_plane,
                               int32_t planes, void* stream);
/* ... at either patch size, patch = 8 or 16 (anything else -> -1): [planes][B*(H/patch)*(W/patch)][3*patch*patch], column
 * c*patch*patch + ky*patch + kx.  H and W must be multiples of `patch` (-1, "Resolution should be a multiple of 8." / "... of 16.").
 * One plane is the rounded value, two planes are hi + lo at out and out + out_plane (out_plane >= rows * 3*patch*patch elements);
 * both in the format of option "op_fmt".  At patch 16, x and out must be 16-byte aligned and out_plane a multiple of 8 elements
 * (16-byte loads and stores; else -1).  The two entries above keep their meaning: patch 8. */
int dinoseg_op_patch_gather_p(const void* x, int32_t x_kind, int32_t B, int32_t H, int32_t W, int32_t patch, void* out,
                              int64_t out_plane, int32_t planes, void* stream);

/* last Linear + log_softmax + argmax (pl_torch_modules.py:122-123,:294); in: hi/lo planes [2][M][ld]; C <= 32 */
int dinoseg_op_head_final(const void* in, int64_t in_plane, int32_t ld, int32_t M, int32_t K, const float* W,
                          const float* b, int32_t C, float* logp, int32_t* argmax, void* stream);
/* The same on MFMAs (the kernel the model runs for 33 <= n_classes <= 256), any 1 <= C <= 256: Wp = the classifier as hi/lo planes
 * [2][round_up(C, 32)][ld] (dinoseg_op_pack, zero padded; w_plane = their stride), b fp32 [C]; ld % 32 == 0, K <= ld.
 * Operand format: option op_fmt. */
int dinoseg_op_head_wide(const void* in, int64_t in_plane, int32_t ld, int32_t M, int32_t K, const void* Wp, int64_t w_plane,
                         const float* b, int32_t C, float* logp, int32_t* argmax, void* stream);

/* flash-attention backward: q,k,v as the forward; dO, O: ctx-layout planes [planes][B*ntok][heads*64]; lse from the
 * forward; scratch: 2*B*heads*npad floats; dqkv out: planes [planes][B*ntok][3*heads*64] (gradient of the qkv
 * projection output, Q|K|V columns).  npad % 64 == 0, npad >= ntok, planes 1 or 2 (else -1, nothing is launched).
 * Pad rows: rows ntok..npad of q, k and v are read with the 64-row tiles they share with real rows and must hold FINITE values -- any
 * finite values, zero is not required.  A pad key is masked (dQ) or never stored (dK, dV); a pad query has -lse = -inf, probability 0,
 * and 0 x finite = 0: dqkv carries the bits of the run on zero pad rows (tests/test_backward_containment_gpu.py); a NaN or Inf
 * there may reach it (0 x Inf).  dO and O have no pad rows; no row at or beyond B*ntok is read.
 * scratch needs no initialisation: all 2*B*heads*npad floats are written before they are read (-lse | -inf, then -delta | 0), and
 * nothing outside them.  The plane strides qkv_plane, o_plane (shared by dO and O) and dqkv_plane may exceed the minimum; dqkv rows have
 * no stride of their own (3*heads*64 elements).  Nothing but dqkv[p][row < B*ntok][col] and the scratch is written.
 * Exactness: the kernels compute delta = sum dO O, P = 2^(q.k - lse), dS = P (dO.v - delta), dQ = 0.125 dS.k, dK = ln2 dS^T.q,
 * dV = P^T.dO from their inputs alone.  On inputs whose scores and lse are integers, whose v, dO and O are small integers and whose
 * sums fit 24 bits, dQ and dV carry the round-to-nearest-even planes of 0.125 * sum and of the sum, bit for bit on both planes, with P
 * and dS rounded to the planes (hi = RNE, lo = RNE of the rest) and hi.hi + hi.lo + lo.hi per product.  dK = float32(sum) * float32(ln 2):
 * on one plane the RNE plane of that product, bit for bit; on two planes within the planes' half ulp (2^-17 relative) plus 2^-23 of the
 * exact product -- its lo plane is rounded from the exact product where the compiler contracts the split's multiply and subtract, from
 * the fp32 product where it does not, and either is a correct split.  (tests/test_attention_bwd_probes_gpu.py::test_probe,
 * ::test_probes_on_the_8_wave_dq_route; the construction and what it can see: tests/attention_bwd_probe_util.py,
 * tests/test_attention_bwd_probes_cpu.py.) */
int dinoseg_op_attention_bwd(const void* q, const void* k, const void* v, int64_t qkv_plane, const void* dO, const void* O,
                             int64_t o_plane, const float* lse, float* scratch, void* dqkv, int64_t dqkv_plane, int32_t B,
                             int32_t heads, int32_t ntok, int32_t npad, int32_t planes, void* stream);

/* native_layer_norm_backward: dx (+)= ..., dgamma += ..., dbeta += ... (atomics; zero them first) */
int dinoseg_op_layernorm_bwd(const float* dy, const float* x, const float* gamma, float eps, int32_t M, int32_t D, float* dx,
                             int32_t accumulate, float* dgamma, float* dbeta, int32_t drop_cls, int32_t ntok, void* stream);
/* ... with the by-products the fine-tune step uses: the final dx rows as bf16 planes dxp [planes][M][D] (plane stride dxp_plane; null =
 * none) and colsum[D] += their column sums (null = none) */
int dinoseg_op_layernorm_bwd2(const float* dy, const float* x, const float* gamma, float eps, int32_t M, int32_t D, float* dx,
                              int32_t accumulate, float* dgamma, float* dbeta, int32_t drop_cls, int32_t ntok, void* dxp,
                              int64_t dxp_plane, int32_t planes, float* colsum, void* stream);

/* Weight gradient on row-major planes (the step's route for every layer whose input width is a multiple of 128):
 * dW[n][k] += sum_m Y[m][n] X[m][k] for n < N, k < k_cols; Y planes [planes][M][ldy], X planes [planes][M][ldx], Kc % 128 == 0
 * columns of X multiplied.  ksplit slices of the batch write partial tiles to part (required: ksplit * ceil(N/128)*128 * Kc floats), then
 * the slices that own rows are summed into dW (row stride ldw; dW == null: column sums only).  colsum[N] += the column sums of Y
 * (null = none).  Zero dW and colsum first. */
int dinoseg_op_gemm_tn(const void* Y, int64_t y_plane, int32_t ldy, const void* X, int64_t x_plane, int32_t ldx, int32_t M, int32_t N,
                       int32_t Kc, int32_t planes, int32_t ksplit, float* part, float* dW, int32_t ldw, int32_t k_cols, float* colsum,
                       void* stream);
/* Input gradient of a linear layer: acc[M][N] = A[M][K] . Wt[N][K]^T (bf16 planes, N % 128 == 0, K % 64 == 0) with a backward
 * epilogue: epi 0 = fp32 out_f32[M][ldo_f32] (no bias), 6 = bf16 planes out_bf16 [planes][M][ldo], 8 = acc * gelu'(aux_in),
 * 9 = acc * (aux_in > 0) into out_bf16 (aux_in: planes [planes][M][ldo], plane stride aux_plane) */
int dinoseg_op_gemm_bwd(const void* A, int64_t a_plane, int32_t lda, const void* Wt, int64_t w_plane, int32_t M, int32_t N, int32_t K,
                        int32_t planes, int32_t epi, float* out_f32, int32_t ldo_f32, void* out_bf16, int64_t out_plane, int32_t ldo,
                        const void* aux_in, int64_t aux_plane, void* stream);
/* Weight gradient of a narrow layer (input width not a multiple of 128: the patch embedding): dY (fp32 rows dy_f32 [*][ldy], or bf16
 * planes dy [planes][*][ldy]; drop_cls: logical row j is physical row b*ntok + t + 1) and X planes [planes][M][ldx] are transposed
 * into T1 / T2 ([planes][round_up(., 128)][m_pad] each, plane stride t_plane, m_pad % 64 == 0, >= M), colsum[N] += the column sums
 * of dY; then dW[N][K] += dY^T X over the batch rows: ksplit == 1 by fp32 atomics, else ksplit slices of partial tiles in part
 * (ksplit * ceil(N/128)*128 * round_up(K, 128) floats) and a reduce. */
int dinoseg_op_wgrad_nt(const float* dy_f32, const void* dy, int64_t dy_plane, int32_t ldy, const void* x, int64_t x_plane, int32_t ldx,
                        int32_t M, int32_t N, int32_t K, int32_t planes, int32_t drop_cls, int32_t ntok, int32_t ksplit, void* T1,
                        void* T2, int64_t t_plane, int32_t m_pad, float* part, float* dW, float* colsum, void* stream);
/* F.nll_loss (mean, ignore_index -100) + the backward of log_softmax.  Exactly one of labels [M] and dlogp [M][C] (fp32).  labels:
 * acc (2 floats), *loss = the mean, flags[0] |= 1 on a label outside [0, C) and not -100 (the row is ignored).  dz: d logits as bf16
 * hi + lo planes [2][M][ldz] (plane stride dz_plane), columns >= C zero; C > 32 needs an even ldz. */
int dinoseg_op_nll_loss_grad(const float* logp, const int64_t* labels, const float* dlogp, int32_t M, int32_t C, float* acc,
                             int32_t* flags, float* loss, void* dz, int64_t dz_plane, int32_t ldz, void* stream);
/* Backward of dinoseg_op_pos_resample_hw: dpe [g*g+1][D] += the transpose of the resample applied to dpos [oh*ow+1][D];
 * scratch: g * ow * D floats */
int dinoseg_op_pos_resample_bwd_hw(const float* dpos, int32_t g, int32_t D, int32_t oh, int32_t ow, float* dpe, float* scratch,
                                   void* stream);

/* ---- the helper kernels on their own (tests).  16-bit operands are in the format of option "op_fmt"; every entry refuses null
 * pointers and negative sizes on the host (-1 with a message) before anything is launched. ---- */

/* Materialised softmax(q k^T) of one block (get_last_selfattention, vision_transformer.py:273-280 -> :85, :101): q (pre-scaled by
 * 64^-0.5 * log2(e)) and k as [planes][B, heads, npad, 64] (lo plane at + qkv_plane elements; rows >= ntok are never read),
 * out fp32 [B, heads, ntok, ntok]. */
int dinoseg_op_attn_probs(const void* q, const void* k, int64_t qkv_plane, int32_t planes, int32_t B, int32_t heads, int32_t ntok,
                          int32_t npad, float* out, void* stream);
/* The CLS query row of that softmax at pixel resolution, with dt_utils.process_attentions' cumulative-mass threshold, in one launch
 * (one workgroup per (frame, head); the N x N matrix is never formed).  q, k as dinoseg_op_attn_probs reads them (rows >= ntok are
 * never read; the lo plane at + qkv_plane elements, qkv_plane >= B*heads*npad*64 and a multiple of 8; pointers 16-byte aligned);
 * ntok = hp*wp + 1, at most dinoseg_cls_attention_max_tokens().
 *   Softmax: s_n = q_0 . k_n in fp32 for every key n < ntok (token 0 is the CLS query); p_n = 2^(s_n - max_n s_n) / sum_n 2^(s_n - max)
 *     over ALL ntok keys (q carries head_dim^-0.5 log2 e, so this is softmax(q k^T head_dim^-0.5)); the patches are p_1 .. p_{ntok-1},
 *     patch j - 1 = (row, column) of the hp x wp grid, row-major: get_last_selfattention(x)[b, h, 0, 1:].
 *   Threshold (only with keep_out; threshold inside (0, 1), else -1): q_j = rint(p_j 2^30) as an unsigned 32-bit integer, T = sum_j q_j
 *     over the patches, S_le(v) = the sum of the q_j <= v, t = rint(threshold 2^24) (threshold as the fp32 value passed).  Patch j is
 *     kept iff S_le(q_j) 2^24 > (2^24 - t) T, all in unsigned 64-bit integers (T < 2^31: no overflow).  This is process_attentions'
 *     rule -- sort ascending, normalise by the patches' own sum, keep where the cumulative sum exceeds 1 - threshold -- made exact:
 *     integer sums do not depend on their order, so a host restatement reproduces every decision.  It differs from the fp32 sort /
 *     cumsum in the 2^-30 quantisation and at exact ties: the reference keeps a suffix of a tied group in unspecified sort order, this
 *     rule keeps the whole group.
 *   Output: pixel (oy, ox) of the OH x OW map takes patch (sy, sx) = ((oy hp) / OH, (ox wp) / OW), integer division; for integer
 *     multiples this is F.interpolate(scale_factor=patch, mode="nearest").  Any OH >= hp, OW >= wp.
 * attn_out fp32 [B, heads, OH, OW], keep_out uint8 (0 / 1) [B, heads, OH, OW]; each nullable, not both.  attn_out is the same bits
 * with and without keep_out; two runs give the same bits. */
int dinoseg_op_cls_attention(const void* q, const void* k, int64_t qkv_plane, int32_t planes, int32_t B, int32_t heads, int32_t ntok,
                             int32_t npad, int32_t hp, int32_t wp, int32_t OH, int32_t OW, float threshold, float* attn_out,
                             uint8_t* keep_out, void* stream);
/* Attention.forward(x, cls_mask) for the CLS query of ONE frame (vision_transformer.py:80-107): the CLS row's logits times
 * [0, mask], softmax over all ntok keys, @ V.  q, k, v: [planes][heads, npad, 64] (with one fp16 plane V is bf16, as the fused
 * attention has it); mask fp32 [n_masks][ntok - 1]; ctx: planes [planes][n_masks][heads * 64] (lo at + ctx_plane elements); probs
 * (nullable): fp32 [heads][n_masks][ntok].  More than 15 360 tokens exceed the score buffer (-1). */
int dinoseg_op_cls_mask_attn(const void* q, const void* k, const void* v, int64_t qkv_plane, int32_t planes, int32_t heads, int32_t ntok,
                             int32_t npad, const float* mask, int32_t n_masks, void* ctx, int64_t ctx_plane, float* probs, void* stream);
/* X[b * ntok, :] = cls + pos[0, :] for b < B (prepare_tokens, vision_transformer.py:229-233); X fp32 [B * ntok, D]; other rows untouched */
int dinoseg_op_cls_rows(float* X, const float* cls, const float* pos, int32_t B, int32_t ntok, int32_t D, void* stream);
/* rows 1 .. n of X fp32 [n + 1, D] = row 0 (the CLS residual once per mask, vision_transformer.py:131-135); n == 0 does nothing */
int dinoseg_op_broadcast_row0(float* X, int32_t D, int32_t n, void* stream);
/* out[t, d] = sum over b < B of X[b, t, d] (the pos-embed gradient of a batch); X fp32 [B, ntok, D], out fp32 [ntok, D] */
int dinoseg_op_batch_sum_rows(const float* X, int32_t B, int32_t ntok, int32_t D, float* out, void* stream);
/* `count` weight packs in one launch per 40 jobs, what dinoseg_refresh_weights runs: job i turns src[i] fp32 [rows, cols] into planes
 * [planes][rows_pad][cols_pad] at dst[i] (transposed[i] = 1: [planes][cols_pad][rows_pad], dst[c][r] = src[r][c]), zero padded, the lo
 * plane at + plane[i] elements, fmt[i] 0 = bf16, 1 = fp16.  Host arrays of `count` entries, as dinoseg_adam_step_multi takes them.  A job
 * with rows_pad * cols_pad == 0 is skipped. */
int dinoseg_op_multi_pack(int32_t count, const float* const* src, void* const* dst, const int64_t* plane, const int32_t* rows,
                          const int32_t* cols, const int32_t* rows_pad, const int32_t* cols_pad, const int32_t* planes,
                          const int32_t* transposed, const int32_t* fmt, void* stream);
/* p[i][0 .. n[i]) = 0 for `count` fp32 tensors in one launch per 64 (the gradient reset of a fine-tune step); n[i] == 0 is legal */
int dinoseg_op_multi_zero(int32_t count, float* const* p, const int64_t* n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DINOSEG_H */
