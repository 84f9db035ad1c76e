/*
 * u2tok.h -- C ABI of libu2tok_hip.so, the MI355X (gfx950) implementation of the u2Tokenizer forward path.
 *
 * The reference (Siyou-Li/u2Tokenizer) has no FFI / operator registry: its hot path
 * `u2MetaForCausalLM.prepare_inputs_for_multimodal` (src/model/u2_arch.py:96-117) is a chain of Python
 * nn.Module calls into stock torch ops.  The seam a maintainer would bind is therefore the three module
 * forwards + the embedding splice; each entry point below names the reference code it replaces.
 * The Python host side (u2tokenizer_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions for EVERY function:
 *   - all pointers are DEVICE pointers (HBM) unless the name says `host`; tensors are dense row-major;
 *   - "bf16" = raw bfloat16 bits (uint16_t); parameters are expected in bf16 (model.to(torch.bfloat16));
 *   - work is enqueued on `stream` (a hipStream_t, e.g. torch.cuda.current_stream().cuda_stream);
 *     nothing allocates device memory, nothing synchronises, the caller owns every buffer including the workspace;
 *   - work is launched on the CURRENT HIP device: make the device of the buffers current first (hipSetDevice);
 *   - return value: 0 = success, negative = U2TOK_ERR_* (the Python shim raises RuntimeError).
 */
#ifndef U2TOK_H_
#define U2TOK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define U2TOK_OK 0
#define U2TOK_ERR_ARG (-1)        /* bad dimension / null pointer / unsupported combination */
#define U2TOK_ERR_LAUNCH (-2)     /* a kernel launch failed */
#define U2TOK_ERR_WORKSPACE (-3)  /* workspace too small: call the matching *_workspace_bytes */
#define U2TOK_ERR_DEVICE (-4)     /* current device is not gfx950 */

typedef void* u2tok_stream_t; /* hipStream_t */

/* ---- library identity / gating -------------------------------------------------------------- */
int u2tok_version(void);               /* MAJOR*10000 + MINOR*100 + PATCH */
const char* u2tok_arch(void);          /* "gfx950" */
/* The 16-bit ELEMENT TYPE of this build: "bf16" (libu2tok_hip.so) or "f16" (libu2tok_hip_f16.so -- the same sources compiled
 * with -DU2_ELEM_F16 for checkpoints loaded in float16, evalscipt/ourmodel_amos.py:33,70).  Wherever this header says "bf16"
 * (parameter / activation buffers, function names such as u2tok_gemm_bf16) read "the element type of the build": both
 * libraries export exactly the same symbols, accumulate in fp32 and differ only in the storage format and the MFMA opcode. */
const char* u2tok_elem(void);
int u2tok_device_check(void);          /* 0 if the current HIP device is gfx950, else U2TOK_ERR_DEVICE */
/* ---- execution contexts --------------------------------------------------------------------------------------------
 * Options, the tokenizer's side streams / events (one set per caller stream), split-K scratch registrations and
 * profiling records belong to a CONTEXT.  A host thread works on its current context: the one bound with
 * u2tok_ctx_set_current (thread-local, like hipSetDevice), or the process default context when none is bound.  Give
 * every model -- or every host thread -- its own context and they share no mutable state; a context used from several
 * threads at once is safe for launches as long as its options are not changed concurrently.  A context's side streams
 * are created on the HIP device that is current at their first use: keep one context per device. */
typedef struct u2tok_ctx* u2tok_ctx_t;
int u2tok_ctx_create(u2tok_ctx_t* out);
int u2tok_ctx_destroy(u2tok_ctx_t ctx);      /* no work of this context may still be being enqueued */
int u2tok_ctx_set_current(u2tok_ctx_t ctx);  /* NULL: back to the process default context */
u2tok_ctx_t u2tok_ctx_get_current(void);     /* NULL when the thread uses the default context */

/* Tuning / diagnostics switches of the calling thread's current context; U2TOK_ERR_ARG if unknown / out of range:
    "gemm_tile" {0 heuristic, 64, 128: tile of the small-tile kernel}, "gemm_splitk" {-1 never, 0 heuristic, 2..16 force
    that many K slices where scratch allows}, "gemm_big" {-1 never, 0 heuristic; force a form of the big-tile kernel: 20 / 21 =
    256x256 / 256x192 tiles with two LDS stages, 22 = 256x128 ring (three stages), 24 / 26 = 256x192 / 256x256 with three stages
    for B, 27 = the drain form of 24}, "gemm_big_grid" {persistent workgroups}, "gemm_big_splitk" {K slices of a FORCED big-tile
    launch}, "gemm_big_drain" {1: the heuristic may pick the drain form, 0: never}, "gemm_skinny" {2: 64 < M <= 256 rows against
    2048 .. 4096 columns take the unsplit skinny kernel, 1: its FLAT-encoded form, 0: never}, "kmajor_b" {1: P V and the DiffTS aggregation read V / X in place as
    K-major operands, 0: through transposed copies}, "gemm_tail_fused" {1: <= 16 rows behind a multiple of 256 rows (the ViT's cls
    rows) are computed inside the big-tile launch by the few-rows kernel's arithmetic, 0: a few-rows launch of their own},
    "flash_mode" {0 pick, 1 plain 128-row units, 7 double pipeline (generated asm KV loop)}, "flash_q_prescaled" {1: the q handed to
    u2tok_flash_attention_d64 already carries scale * log2 e}, "vit_flash" {0 unfused attention, 1}, "tta_overlap" {0, 1: side
    stream for the TTA k|v projections},
    "vit_vt_epilogue" {1: the ViT's q|k|v product leaves V^T (the flash kernel's operand) from its own V tiles, 0: a transpose launch},
    "tok_flash" {1: the tokenizer's attention cores run the fused kernel of u2tok_tok_attention, 0: GEMM -> softmax -> GEMM},
    "tok_wide" {1: head dims 256 / 512 (not 384) of that kernel run its 8-wave form (a wave pair per 16-query block, two waves per SIMD),
    0: the 4-wave form},
    "svr_fold" {1: a tokenizer forward that asks for no SVR intermediate uses the fold slots of its weight table (below), 0: never},
    "profile" {0, 1} */
int u2tok_set_option(const char* name, int value);
/* Scratch for split-K partial sums of u2tok_gemm_bf16 calls on `stream` (fp32, slices x M x N), registered on the
 * current context: skinny products (few output tiles, long K) are cut along K when a scratch is registered; NULL / 0
 * removes it.  The module forwards below carve their own from their workspace and do not need this. */
int u2tok_set_gemm_scratch(void* device_ptr, size_t bytes, void* stream);

/* With option "profile" = 1 every launch is bracketed by hipEvents on its stream.  Collect (HOST arrays of ncat <= 6
 * entries; synchronises on the recorded events, then resets): summed milliseconds, algorithmic FLOPs and launch
 * counts per kernel class 0 = MFMA GEMM, 1 = ViT flash attention, 2 = temporal attention, 3 = row ops
 * (LayerNorm / softmax / RoPE / scores / top-k / pooling), 4 = data movement (im2col, transposes, gathers, splice),
 * 5 = fused tokenizer attention (u2tok_tok_attention). */
int u2tok_profile_collect(double* ms_host, double* flops_host, int64_t* count_host, int32_t ncat);
/* Same, plus the summed ALGORITHMIC bytes (every operand read once + every result written once) per class. */
int u2tok_profile_collect2(double* ms_host, double* flops_host, double* bytes_host, int64_t* count_host, int32_t ncat);

/* ---- configuration records -------------------------------------------------------------------- */

/* ViT3DTower (src/model/multimodal_encoder/vit.py:132-164) built on MONAI 1.3.0 PatchEmbeddingBlock
 * (perceptron) + TransformerBlock x depth; hyper-parameters hard-coded at vit.py:33-38,139-146. */
typedef struct {
  int32_t nchunk;          /* B*C: 32-slice chunks in this call (u2_arch.py:105-106) */
  int32_t img[3];          /* config.image_size, e.g. {32,256,256} */
  int32_t patch[3];        /* config.patch_size, e.g. {4,16,16} */
  int32_t hidden;          /* 768 */
  int32_t mlp_dim;         /* 3072 */
  int32_t depth;           /* 12 */
  int32_t heads;           /* 12 (head dim must be 64) */
  int32_t vol_dtype;       /* 0 = fp16, 1 = bf16, 2 = fp32 voxels */
  int32_t keep_cls;        /* 0: select_feature == "patch" (drop cls, vit.py:157-158); 1: "cls_patch" */
  float ln_eps;            /* 1e-5 */
} u2tok_vit_config;

/* ViT weight table: array of (4 + 11*depth + 2) device pointers, all bf16, MONAI state-dict names:
 *   [0] patch_embedding.position_embeddings (1,ntok,hidden)   [1] patch_embedding.patch_embeddings.1.weight
 *   [2] patch_embedding.patch_embeddings.1.bias               [3] cls_token
 *   per block i (base 4 + 11*i): norm1.weight, norm1.bias, attn.qkv.weight, attn.out_proj.weight,
 *       attn.out_proj.bias, norm2.weight, norm2.bias, mlp.linear1.weight, mlp.linear1.bias,
 *       mlp.linear2.weight, mlp.linear2.bias
 *   [4+11*depth] norm.weight   [5+11*depth] norm.bias */
#define U2TOK_VIT_NW(depth) (4 + 11 * (depth) + 2)

/* SpatialPoolingProjector (src/model/multimodal_projector/spatial_pooling_projector.py:7-59). */
typedef struct {
  int32_t nchunk;
  int32_t grid[3];         /* num_patches_pre = image_size / patch_size */
  int32_t pooling_size;    /* 2 */
  int32_t pooling_type;    /* 0 = "spatial" (avg_pool3d), 1 = "sequence" (avg_pool1d over pooling_size^3) */
  int32_t in_dim;          /* 768 */
  int32_t out_dim;         /* E = LLM hidden size */
  int32_t layer_type;      /* 0 = "mlp" (GELU between), 1 = "linear" */
  int32_t layer_num;       /* 2 */
} u2tok_spp_config;
/* SPP weight table: 2*layer_num pointers: projector.{0,2,..}.weight, .bias in order. */

/* u2Tokenizer (src/model/u2tokenizer/u2Tokenizer.py:6-47; builder.py:3-14). */
typedef struct {
  int32_t B;               /* volumes */
  int32_t T;               /* chunks per volume ("frames") */
  int32_t N;               /* projector tokens per chunk */
  int32_t E;               /* embed_size == hidden_size */
  int32_t Lt;              /* text tokens (padded question length) */
  int32_t num_heads;       /* u2t_num_heads */
  int32_t num_layers;      /* u2t_num_layers */
  int32_t top_k;           /* u2t_top_k */
  int32_t num_query;       /* num_3d_query_token */
  int32_t use_multi_scale; /* bool */
  int32_t attn_type;       /* 0 = "rma" (RelativeMultiheadAttention), 1 = "rope", 2 = nn.MultiheadAttention read
                              sequence-first (every other attn_type string, svr.py:16-18): attends across batch entries */
  int32_t enable_diffts;   /* bool: DifferentiableTokenSelection vs TokenSelection */
  int32_t enable_dmtp;     /* bool: DynamicMultiScalePooling */
  int32_t max_seq_len;     /* 512: rma.py:6 / rope.py:19 */
  float diffts_tau;        /* 1.0 (svr.py:94) */
  float ln_eps;            /* 1e-5 */
} u2tok_tokenizer_config;

/* Tokenizer weight table (all bf16), in this order; an attention record "ATT" is
 *   wq.weight, wq.bias, wk.weight, wk.bias, wv.weight, wv.bias, dense.weight, dense.bias, relative_bias
 * (relative_bias = null for MultiHeadCrossAttention and for attn_type rope):
 *   [0] query_tokens
 *   per SVR layer l (base 1 + 18*l):  ATT spatial_attention, ATT temporal_attention
 *   then token_selection.score_net.weight, .bias
 *   then dynamic_pool.gate_fc.weight, .bias   (null when !enable_dmtp)
 *   per TTA layer l (33 pointers): ATT self_attention, ATT visual_cross_attention, ATT text_cross_attention,
 *       norm_self.weight, .bias, norm_cross_v.weight, .bias, norm_cross_t.weight, .bias
 *   then ATT layer_linagg.linear_aggregator (wv/dense present in the state dict but never read: tta.py:47-48,62-65) */
#define U2TOK_TOK_NW(layers) (1 + 18 * (layers) + 4 + 33 * (layers) + 9)
/* FOLD SLOTS: U2TOK_TOK_NFOLD(layers) more pointers behind the U2TOK_TOK_NW(layers) above, a (W', b') pair per SVR attention that
 * has a predecessor.  The SVR stack is a chain of 2 L attentions with nothing between them (svr.py:23-40,50-62: no residual, norm
 * or activation), so the output projection (dense / out_proj) of attention j - 1 is followed directly by the packed q | k | v
 * projection of attention j: with W' = W_qkv W_o (3E, E) and b' = W_qkv b_o + b_qkv (3E) -- u2tok_tokenizer_svr_fold builds both --
 * q | k | v of attention j is context(j - 1) W'^T + b' and the E x E product of attention j - 1 is not run.  Attention j = 2 l is
 * layer l's spatial attention, j = 2 l + 1 its temporal one; the pair of attention j >= 1 is at U2TOK_TOK_NW + 2 (j - 1), + 1:
 *   layer 0 temporal, layer 1 spatial, layer 1 temporal, ..., layer L-1 temporal.
 * A null pointer in a pair means "not folded".  A pair is used when option "svr_fold" is 1, the call asks for no SVR intermediate
 * (svr_out null; no svr_in / svr_out tap) and wq | wk | wv of attention j are packed (back to back, weights and biases); a call
 * that asks for an SVR intermediate is parity instrumentation, runs every projection at the reference's rounding points and DOES
 * NOT READ the slots -- every other call does, so its table must have them (null where there is no fold).  The last attention's
 * output projection always runs.  The folded route rounds W' once to the element type where the unfolded one rounds the projected
 * tokens; (2 L - 1) 3 E^2 elements of device memory, which the caller owns and rebuilds when a weight changes. */
#define U2TOK_TOK_NFOLD(layers) ((layers) > 0 ? 2 * (2 * (layers) - 1) : 0)

/* ---- the hot path ------------------------------------------------------------------------------ */

/* Replaces ViT3DTower.forward (vit.py:148-164): volume (nchunk,1,D,H,W) -> features
 * (nchunk, ntok[+1], hidden) bf16. */
size_t u2tok_vit_workspace_bytes(const u2tok_vit_config* cfg);
int u2tok_vit_forward(const u2tok_vit_config* cfg, const void* const* weights, const void* volume, void* out,
                      void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* Replaces SpatialPoolingProjector.forward (spatial_pooling_projector.py:34-52):
 * (nchunk, g1*g2*g3, in_dim) bf16 -> (nchunk, proj_out_num, out_dim) bf16. */
size_t u2tok_spp_workspace_bytes(const u2tok_spp_config* cfg);
int u2tok_spp_forward(const u2tok_spp_config* cfg, const void* const* weights, const void* x, void* out,
                      void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* Replaces u2Tokenizer.forward (u2Tokenizer.py:40-47): v_token (B,T,N,E), t_token (B,Lt,E) bf16 ->
 * aligned tokens (B,num_query,E) bf16.  topk_idx_out (optional, may be null): (B,top_k) int64 indices chosen by
 * TokenSelection (only written when !enable_diffts) -- the path's integer output.  svr_out (optional, may be null):
 * (B,T*N,E) bf16 copy of the refined tokens the selection stage scores (output of svr.py:166-170), so that a checker
 * can replay the selection on identical inputs.  weights: U2TOK_TOK_NW(L) + U2TOK_TOK_NFOLD(L) pointers (the fold slots are read
 * by a call with svr_out null). */
size_t u2tok_tokenizer_workspace_bytes(const u2tok_tokenizer_config* cfg);
int u2tok_tokenizer_forward(const u2tok_tokenizer_config* cfg, const void* const* weights, const void* v_token,
                            const void* t_token, void* out, int64_t* topk_idx_out, void* svr_out, void* workspace,
                            size_t workspace_bytes, u2tok_stream_t stream);

/* One fold slot of the tokenizer weight table: w_fold (3E, E) = w_qkv (3E, E) w_o (E, E) -- one u2tok_gemm_bf16 product, w_o read
 * K-major as it lies -- and b_fold (3E) = b_o w_qkv^T + b_qkv; fp32 accumulation, one rounding to the element type each.  w_qkv /
 * b_qkv: the packed wq | wk | wv of the attention, w_o / b_o: dense (out_proj) of the attention before it.  All pointers are
 * required and the outputs must not alias the inputs; E a multiple of 8. */
int u2tok_tokenizer_svr_fold(const void* w_qkv, const void* b_qkv, const void* w_o, const void* b_o, void* w_fold, void* b_fold,
                             int32_t E, u2tok_stream_t stream);

/* Same forward with PARITY TAPS (tests): any layer's input can be replaced by a caller buffer ("teacher forcing": each
 * layer of the residual-free SVR stack / of the TTA is then compared on the reference's own fp32 input for that layer) and
 * any layer's output copied out.  Every pointer, and every array entry, may be NULL.  Shapes: svr (B,T,N,E), visual
 * (B,Lv,E) with Lv = top_k (+ top_k/2 + top_k/4 with multi-scale pooling), tta (B,num_query,E); all bf16. */
typedef struct {
  const void* const* svr_in;  /* [num_layers]: replaces the input of SVR layer l (svr.py:23-40) */
  void* const* svr_out;       /* [num_layers]: receives the output of SVR layer l */
  const void* visual_in;      /* replaces the visual tokens the TTA attends to (output of svr.py:171-184) */
  void* visual_out;           /* receives them (before a replacement) */
  const void* const* tta_in;  /* [num_layers]: replaces the query input of TTA layer l (tta.py:93-107) */
  void* const* tta_out;       /* [num_layers]: receives the output of TTA layer l */
} u2tok_tokenizer_taps;
int u2tok_tokenizer_forward_taps(const u2tok_tokenizer_config* cfg, const void* const* weights, const void* v_token,
                                 const void* t_token, void* out, int64_t* topk_idx_out, const u2tok_tokenizer_taps* taps,
                                 void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* Replaces embed_tokens(ids) + the splice of u2_arch.py:109,113-116:
 * out[b][s] = (1 <= s <= nfeat) ? feats[b][s-1] : table[ids[b][s]].  nfeat = 0 / feats = null: plain lookup.
 * An id outside [0, vocab) is clamped to the nearest table row (id < 0 -> row 0, id >= vocab -> row vocab - 1). */
int u2tok_embed_splice(const void* table, const int64_t* ids, const void* feats, void* out, int32_t B, int32_t S,
                       int32_t E, int32_t nfeat, int64_t vocab, u2tok_stream_t stream);

/* ---- producer of the path's input ("next" row of the scope table) ------------------------------------------- */
/* u2Transform.adaptive_resize (src/utils/u2Transform.py:62-122 with the validation transforms of :46-54) on the GPU:
 * ScaleIntensityRangePercentiles(lower_pct, upper_pct, 0, 1, clip) -> CropForeground -> anti-aliased trilinear
 * resize to (int(H r), int(W r), min(D, depth_pad)), r = min(target/H, target/W) -> zero pad to
 * depth_pad x target x target.  vol: fp32 [D][H][W] (the tensor of u2Transform.py:68-69 without the channel axis);
 * out: [depth_pad][target][target] == (depth_pad/32, 32, target, target) of out_dtype (0 fp16, 1 bf16, 2 fp32);
 * info (optional, 12 x int32, device): status (0 ok, 1 no foreground, 2 filter too wide), crop lo[3], hi[3] (d,h,w),
 * resized size[3], then the two percentiles as float. */
size_t u2tok_preprocess_workspace_bytes(int32_t D, int32_t H, int32_t W);
int u2tok_preprocess_volume(const float* vol, void* out, int32_t* info, int32_t D, int32_t H, int32_t W, int32_t target,
                            int32_t depth_pad, float lower_pct, float upper_pct, int32_t out_dtype, void* workspace,
                            size_t workspace_bytes, u2tok_stream_t stream);

/* Same with the training-time branch of u2Transform (u2Transform.py:32-44): between CropForeground and the resize the
 * volume is rotated by rot90_k quarter turns in the (H, W) plane (RandRotate90(spatial_axes=(1,2)), torch.rot90
 * convention), flipped along D / H / W (RandFlip x3), multiplied by (1 + scale_factor) (RandScaleIntensity) and shifted by
 * shift_offset (RandShiftIntensity).  The random draws are the CALLER's (host struct): the library is deterministic. */
typedef struct {
  int32_t rot90_k;       /* 0..3 */
  int32_t flip[3];       /* bool per spatial axis (d, h, w) */
  float scale_factor;    /* RandScaleIntensity factor in [-0.1, 0.1] in the reference; 0 = off */
  float shift_offset;    /* RandShiftIntensity offset in [-0.1, 0.1] in the reference; 0 = off */
} u2tok_augment;
int u2tok_preprocess_volume_aug(const float* vol, void* out, int32_t* info, int32_t D, int32_t H, int32_t W, int32_t target,
                                int32_t depth_pad, float lower_pct, float upper_pct, int32_t out_dtype,
                                const u2tok_augment* aug, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* ---- building blocks (exported for the parity tests; same kernels the pipelines launch) -------- */

/* C[z] = epi(alpha * A[z] B[z]^T): A (M,K) lda, B (N,K) ldb, C (M,N) ldc; z = zb*nbh + zh with element strides.
 * flags: 1 bias[n], 2 bias[m], 4 GELU, 8 + R[m][n], 16 C is fp32 (else bf16), 64 B is K-tile-major [K/64][N][64],
 * 256 B is stored K-major, (K,N) with ldb >= N (C = A B: the input-gradient product dX = dY W without a transposed W),
 * 128 | 256 A is stored K-major too, (K,M) with lda >= M (C = A^T B: the weight-gradient product dW = dY^T X without
 * transposed activations); the K-major dimension (M resp. N) must be a multiple of 8.
 * 512: gate | up pair product of a gated MLP (LlamaMLP / Qwen3MLP: act_fn(gate_proj(x)) * up_proj(x)): B = the gate weight's
 * I rows followed by the up weight's I rows (N = 2 I), C (M, I) bf16 = bf16(silu(bf16(x gate^T))) * bf16(x up^T) -- the values
 * u2tok_gemm_bf16 + u2tok_swiglu_bf16 produce, bit for bit, without the (M, 2 I) intermediate; alone (no other flag, nz = 1),
 * K % 64 == 0, I % 16 == 0, 16-byte aligned operands; U2TOK_ERR_ARG otherwise.
 * GELU (flag 4, and u2tok_gelu_fwd) is not exact erf-GELU: x Phi(x) with Phi a logistic-polynomial approximation, |error| <= 3.3e-6
 * before rounding, evaluated on the pre-activation rounded to the element type (after bias, before the residual). */
int u2tok_gemm_bf16(const void* A, const void* B, void* C, const void* bias, const void* R, int32_t M, int32_t N,
                    int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int32_t nz, int32_t nbh,
                    int64_t sAb, int64_t sAh, int64_t sBb, int64_t sBh, int64_t sCb, int64_t sCh, int64_t sRb,
                    int64_t sRh, float alpha, int32_t flags, u2tok_stream_t stream);
/* u2tok_gemm_bf16 with the column split and the transposed side output of the ViT's q|k|v product:
 *   - nsplit (a multiple of 16, not with flag 512): columns n < nsplit are scaled by alpha_lo instead of alpha, from the fp32
 *     accumulator and before the bias -- once, whatever kernel and however many K slices the product takes;
 *   - vt != NULL: columns n >= vt_n0 of the many-row part of the product are NOT written to C (those elements of C are left
 *     untouched) but, transposed, to vt[m / vt_rows][n - vt_n0][perm16(m % vt_rows)] (bf16; row stride vt_ld keys, chunk stride
 *     vt_bs elements), perm16 = the key order of u2tok_transpose_bf16(..., perm16 = 1): inside every group of 16 keys
 *     [0-3, 8-11, 4-7, 12-15].  Rows past the last multiple of 256 (<= 16: the ViT's cls rows) are written whole to C.
 *     Only the deep 256 x 192 big-tile forms have it: plain bf16 output (flags 0, nz 1), the heuristic route (option gemm_big 0),
 *     vt_n0 and N - vt_n0 multiples of 192, nsplit <= vt_n0, vt_rows a multiple of 256 that divides the many-row part, vt 16-byte
 *     aligned, vt_ld >= vt_rows, vt_bs >= (N - vt_n0) * vt_ld, both multiples of 8; U2TOK_ERR_ARG otherwise, before any launch.
 * With nsplit = 0, alpha_lo = 1 and vt = NULL this is u2tok_gemm_bf16: the same kernels, the same bits. */
int u2tok_gemm_bf16_ex(const void* A, const void* B, void* C, const void* bias, const void* R, int32_t M, int32_t N,
                       int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int32_t nz, int32_t nbh,
                       int64_t sAb, int64_t sAh, int64_t sBb, int64_t sBh, int64_t sCb, int64_t sCh, int64_t sRb,
                       int64_t sRh, float alpha, int32_t flags, int32_t nsplit, float alpha_lo, void* vt, int32_t vt_n0,
                       int32_t vt_rows, int64_t vt_ld, int64_t vt_bs, u2tok_stream_t stream);
int u2tok_layernorm_bf16(const void* x, const void* res, const void* w, const void* b, void* y, int32_t rows,
                         int32_t C, float eps, u2tok_stream_t stream);
/* The strided form: y[b][r] = LN(x[b][r] (+ res[b][r])) w + b for b < nb, r < rows; row r of batch entry b at
 * x + b*x_bs + r*x_ld (elements; res and y alike).  res = null: no residual, res_bs / res_ld unread.  C % 8 == 0, C <= 8192,
 * every stride a multiple of 8 elements, every pointer 16-byte aligned; U2TOK_ERR_ARG otherwise.  Only the C columns of each
 * row are written.  (The ViT's final norm is two such calls: patch rows, then one cls row per batch entry.) */
int u2tok_layernorm_rows(const void* x, const void* res, const void* w, const void* b, void* y, int32_t nb, int32_t rows,
                         int32_t C, int64_t x_bs, int64_t x_ld, int64_t res_bs, int64_t res_ld, int64_t y_bs, int64_t y_ld,
                         float eps, u2tok_stream_t stream);
int u2tok_softmax_rows(const float* S, void* P, int32_t nz, int32_t rows, int32_t n, int64_t lds, int64_t ldp,
                       float scale, const void* rel_bias, int32_t H, int32_t max_len, u2tok_stream_t stream);
/* out[z][c][r] = in[z][r][c], pad columns zeroed.  perm16 != 0 (needs ld_out % 16 == 0): inside each group of 16
 * output columns the order is [0-3, 8-11, 4-7, 12-15] -- the V^T layout u2tok_flash_attention_d64 consumes. */
int u2tok_transpose_bf16(const void* in, void* out, int32_t nz, int32_t R, int32_t C, int64_t ld_in, int64_t ld_out,
                         int64_t in_zs, int64_t out_zs, int32_t perm16, u2tok_stream_t stream);
int u2tok_im2col_patches(const void* vol, int32_t vol_dtype, void* out, int32_t nchunk, int32_t D, int32_t H,
                         int32_t W, int32_t p1, int32_t p2, int32_t p3, u2tok_stream_t stream);
int u2tok_avgpool3d_tokens(const void* x, void* y, int32_t nb, int32_t g1, int32_t g2, int32_t g3, int32_t w1,
                           int32_t w2, int32_t w3, int32_t C, u2tok_stream_t stream);
int u2tok_score_gemv(const void* x, const void* w, const void* bias, float* scores, int32_t rows, int32_t E,
                     u2tok_stream_t stream);
/* idx[b][0..k): the indices of the k largest of scores[b][0..n), n <= 8192, 1 <= k <= n: descending score, ties by ascending
 * index, -0.0 == +0.0, every NaN (either sign bit, any payload) first -- torch.sort(descending=True, stable=True). */
int u2tok_topk_sorted(const float* scores, int64_t* idx, int32_t B, int32_t n, int32_t k, u2tok_stream_t stream);
int u2tok_gather_rows(const void* x, const int64_t* idx, void* out, int32_t B, int32_t n, int32_t k, int32_t E,
                      u2tok_stream_t stream);
/* dst[b * dst_bs + e] = src[e] for b < nb, e < n: one row broadcast into nb slots dst_bs elements apart (dst_bs >= n) */
int u2tok_fill_rows(const void* src, void* dst, int32_t nb, int64_t n, int64_t dst_bs, u2tok_stream_t stream);
/* ws: B*3*16*ceil(E/256) floats (only read/written when gate_w != null) */
int u2tok_multiscale_pool(const void* x, void* out, int32_t B, int32_t k, int32_t E, const void* gate_w,
                          const void* gate_b, float* ws, u2tok_stream_t stream);
/* attention over the chunk axis (svr.py:31-36) of rows in (b t n) order: T <= 16, d = E / H in {64, 128, 256, 384, 512} */
int u2tok_temporal_attention(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t T,
                             int32_t N, int32_t H, int32_t d, int64_t ld_qkv, int64_t ld_out, float scale,
                             const void* rel_bias, int32_t max_len, u2tok_stream_t stream);
/* softmax(q k^T * scale) v for head_dim 64 (MONAI SABlock core, vit.py:100-105) over S main rows per batch plus
 * n_extra (0 / 1) extra row per batch that lives elsewhere (the cls token, kept after all patch rows): row r of batch b
 * at q + b*q_bs + r*ld_qk, head h at column 64 h; vt = V^T of the main rows, [nb][H][64][S_pad] in perm16 order, zero
 * padded; extra row of batch b at qx / kx / vx + b*x_bs, its output at outx + b*ox_bs. */
int u2tok_flash_attention_d64(const void* q, const void* k, const void* vt, void* out, int32_t nb, int32_t S,
                              int32_t H, int64_t ld_qk, int64_t q_bs, int64_t ld_out, int64_t out_bs, int32_t S_pad,
                              float scale, const void* qx, const void* kx, const void* vx, void* outx, int64_t x_bs,
                              int64_t ox_bs, int32_t n_extra, u2tok_stream_t stream);
/* Same, and lse[(b * H + h) * lse_ld + row] = log2 sum_k exp2(q_row . k scale log2 e) for every query row (the extra row at
 * index S; lse_ld >= S + n_extra): the row statistics u2tok_flash_attention_d64_bwd takes instead of rebuilding them. */
int u2tok_flash_attention_d64_lse(const void* q, const void* k, const void* vt, void* out, int32_t nb, int32_t S,
                              int32_t H, int64_t ld_qk, int64_t q_bs, int64_t ld_out, int64_t out_bs, int32_t S_pad,
                              float scale, const void* qx, const void* kx, const void* vx, void* outx, int64_t x_bs,
                              int64_t ox_bs, int32_t n_extra, float* lse, int64_t lse_ld,
                                  u2tok_stream_t stream);
/* Fused attention core of the tokenizer's attention modules -- RelativeMultiheadAttention (rma.py:60-75: + relative_bias
 * [j - i + max_len - 1][h], bf16 (2 max_len - 1, H)), RotaryMultiheadAttention (rope.py:82-86), MultiHeadCrossAttention /
 * LinearAggregation (tta.py:55-61; rel_bias NULL):  out = softmax(q k^T scale + bias) v  per (batch, head), scores and
 * probabilities never in HBM.  Row r of batch b at ptr + b*?_bs + r*ld?, head h at column h*d, d in {64, 96, 128, 256, 384, 512}
 * (384 = E / 8 at E = 3072; it runs the 4-wave kernel whatever "tok_wide" says); q / k / v 16-byte aligned with strides
 * % 8 == 0, out 8-byte aligned with strides % 4 == 0; with rel_bias: Sq, Skv <= max_len.  splits: 0 = heuristic, n > 0 = cut the keys into n ranges (fp32 partial sums in `workspace`:
 * u2tok_tok_attention_workspace_bytes, 16-byte aligned; NULL = unsplit).  U2TOK_ERR_ARG for shapes it does not take. */
size_t u2tok_tok_attention_workspace_bytes(int32_t nb, int32_t H, int32_t Sq, int32_t Skv, int32_t d);
int u2tok_tok_attention(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv, int32_t H,
                        int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs, int64_t v_bs,
                        int64_t o_bs, float scale, const void* rel_bias, int32_t max_len, int32_t splits, void* workspace,
                        size_t workspace_bytes, u2tok_stream_t stream);

/* ---- the consumer of the path's output ("next" row f3): prefill of the stock HF decoder on the spliced embeddings ---------
 * (LlamaForCausalLM / Qwen3ForCausalLM.forward with inputs_embeds, src/model/language_model/u2llama.py:76-87,123-126).  The
 * decoder keeps its HuggingFace module tree, parameters, KV cache and generate loop; u2tokenizer_amd/prefill.py runs each
 * layer of the PREFILL as RMSNorm -> packed q|k|v GEMM -> head norm + rotary -> causal grouped-query attention -> out
 * projection (+ residual) -> RMSNorm -> packed gate|up GEMM -> SiLU(gate) * up -> down projection (+ residual). */
/* softmax(q k^T scale [causal: key j <= query i + Skv - Sq]) v with grouped-query heads: query head h (column h*d of q / out)
 * reads key / value head h / (Hq / Hkv) (column of k / v); d in {64, 96, 128, 256, 384, 512}; layout conventions of
 * u2tok_tok_attention.  (u2tok_attention_gqa_ex / _range with a key range or row statistics, and _band, do not take 384:
 * U2TOK_ERR_ARG.) */
int u2tok_attention_gqa(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv, int32_t Hq,
                        int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs,
                        int64_t v_bs, int64_t o_bs, float scale, int32_t causal, u2tok_stream_t stream);
/* The same without the causal mask and WITH key splits (flash-decoding: partial results per key range in `workspace`, merged in a
 * fixed order): the decode step's attention of a few query rows over a long KV cache -- nb = batch x kv heads entries of
 * (Skv, d) keys, Hq = query heads per kv head, Hkv = 1 (Qwen3 / Llama decode, language_model/u2llama.py:123-126: generate()).
 * workspace: u2tok_tok_attention_workspace_bytes(nb, Hq, Sq, Skv, d) bytes, 16-byte aligned; NULL = unsplit. */
int u2tok_attention_gqa_split(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                              int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                              int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, void* workspace, size_t workspace_bytes,
                              u2tok_stream_t stream);
/* y[r] = bf16(x[r] * rsqrt(mean(x[r]^2) + eps)) * w   (LlamaRMSNorm / Qwen3RMSNorm); C % 8 == 0, C <= 8192 */
int u2tok_rmsnorm_bf16(const void* x, const void* w, void* y, int64_t rows, int32_t C, int64_t ldx, int64_t ldy, float eps,
                       u2tok_stream_t stream);
/* In place on the q and k heads of a packed projection output qkv[rows][(Hq + 2 Hkv) D] (D = 64 / 96 / 128): per-head RMSNorm
 * with weights wq / wk (Qwen3Attention.q_norm / k_norm; both NULL: none, Llama) and x cos + rotate_half(x) sin
 * (apply_rotary_pos_emb) with cos / sin [rows][cs_ld >= D], fp32 (cos_sin_f32 != 0) or bf16. */
int u2tok_qk_norm_rope(void* qkv, const void* wq, const void* wk, const void* cos, const void* sin, int32_t cos_sin_f32,
                       int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t cs_ld, float eps,
                       u2tok_stream_t stream);
/* The same, and the finished k heads and the v heads also written in the KV cache's layout: k_cache / v_cache
 * [rows / S][Hkv][capacity][D] bf16 (HF DynamicLayer: (batch, kv heads, seq, head_dim); row = batch * S + position) at positions
 * s_off .. s_off + S - 1, kv_stride = capacity * D elements between (batch, kv head) entries (0: dense, capacity = S) -- the
 * prefill hands the cache its tensors without a transposing copy, a decode step appends in place
 * (language_model/u2llama.py:123-126: generate()). */
int u2tok_qk_norm_rope_kv(void* qkv, const void* wq, const void* wk, const void* cos, const void* sin, int32_t cos_sin_f32,
                          int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t cs_ld, float eps,
                          void* k_cache, void* v_cache, int32_t S, int64_t kv_stride, int32_t s_off, u2tok_stream_t stream);
/* u2tok_qk_norm_rope_kv on an FP8 (e4m3) KV cache (u2tok_kv_quantize_rows below: the format), in ONE launch: the q and k columns of
 * qkv get the bits u2tok_qk_norm_rope_kv leaves there; the finished k heads and the v heads are written as codes into positions
 * s_off .. s_off + S - 1 of the dense buffers k_codes / v_codes (B = rows / S, Hkv, capacity, D) bytes (16-byte aligned) and their
 * scales into k_scales / v_scales (B, Hkv, capacity) fp32 -- quantised from the values rounded to the element type, so codes and
 * scales have the bits of u2tok_qk_norm_rope_kv into dense 16-bit rows followed by u2tok_kv_quantize_rows of those rows (=
 * ops.quantize_kv_fp8).  No 16-bit K / V row is written.  Everything u2tok_qk_norm_rope_kv refuses, a null or misaligned buffer,
 * S < 1, s_off < 0, s_off + S > capacity, capacity * D >= 2^31: U2TOK_ERR_ARG, nothing launched, nothing written. */
int u2tok_qk_norm_rope_kv8(void* qkv, const void* wq, const void* wk, const void* cos, const void* sin, int32_t cos_sin_f32,
                           int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t cs_ld, float eps, void* k_codes,
                           void* v_codes, float* k_scales, float* v_scales, int32_t S, int32_t capacity, int32_t s_off,
                           u2tok_stream_t stream);
/* out[r][i] = bf16(silu(gate_up[r][i])) * gate_up[r][I + i]   (LlamaMLP / Qwen3MLP with gate | up packed); I % 8 == 0 */
int u2tok_swiglu_bf16(const void* gate_up, void* out, int64_t rows, int32_t I, int64_t ld_in, int64_t ld_out,
                      u2tok_stream_t stream);

/* ---- one decode step of a decoder layer (the step HF generate() repeats per new token: language_model/u2llama.py:123-126,
 * eval/mrg.py:74-77 asks for up to 768) in two calls -- between them the host appends the new k / v to its KV cache.
 *   pre : input RMSNorm -> packed q|k|v projection (few-rows GEMM) -> per-head q / k RMSNorm (NULL weights: none) + rotary;
 *         qkv (B, (Hq + 2 Hkv) D) keeps the finished queries; the step's keys / values go to position s_off of k_cache / v_cache
 *         (B, Hkv, capacity, D; kv_stride = capacity * D, 0: a dense (B, Hkv, 1, D) pair with s_off = 0)
 *   post: attention of the B query rows over the first T positions of K / V (same layout; keys split over workgroups, merged
 *         in a fixed order) -> out projection + residual x -> RMSNorm -> packed gate|up -> SiLU(gate) * up -> down + residual
 *         batched = 0: a launch pair per sequence, kv_start must be NULL.  batched != 0: the batched decode attention
 *         (u2tok_decode_attention: one launch for all B sequences and heads, plus one merge; Hq / Hkv <= 16) with a first visible
 *         cache position per sequence, kv_start (device int32[B]; NULL: all zeros) -- query b attends over positions
 *         kv_start[b] .. T - 1, the cache of a LEFT-padded batch.
 * B <= 64, D in {64, 96, 128}, E % 32 == 0, I % 32 == 0; biases may be NULL; same rounding points as the HF modules in bf16.
 * 16 < B <= 64: the four products are u2tok_gemm_rows' / u2tok_gemm_rows_w8_wide's (below) -- the weights are still streamed once
 * per step, and the products of sequence b have exactly the bits they have in a step of the sequences 16 (b / 16) .. min(B,
 * 16 (b / 16) + 16) - 1 alone (the attention's key splits are a function of (B, Hkv, T), as for every B) --; post then requires batched != 0 (a launch pair per sequence would be 128 launches per layer), kv_start NULL
 * or per sequence as before.  B > 64, and B > 16 with batched = 0: U2TOK_ERR_ARG before anything is launched.
 * A sliding-window layer (Phi-3: the last W positions) passes K / V advanced to its first visible position and T = W.
 * One workspace for both calls: u2tok_decoder_decode_workspace_bytes(cfg, T) bytes.
 * EVERY refusal of pre, of post and of post_kv8 -- the half's own argument checks and everything one of its launches would refuse
 * (the products', the row kernels', the attention's, the adapter groups') -- is evaluated before the call's first launch, as in the
 * whole-stack step below: an error code other than U2TOK_ERR_LAUNCH means nothing was launched and nothing was written.
 * The layer's parameters travel in one descriptor, filled once per layer; the library keeps no pointer to it.  With the four
 * scales NULL the four W* are contiguous (N, K) matrices in the element type.  With all four set the step is weight-only FP8:
 * the W* are OCP e4m3 codes (contiguous (N, K) bytes) with one fp32 scale per weight row, every product is u2tok_gemm_rows_w8's
 * (below), and activations, biases, norms, attention and the KV cache stay in the element type; E, Hq * D and I must then be
 * multiples of 64, the weights 16-byte and the scales 4-byte aligned.  Some but not all scales set, and every other argument the
 * step does not take: U2TOK_ERR_ARG before anything is launched.
 * With cfg->wform = 2 the step is weight-only MXFP4: the W* are e2m1 codes (contiguous (N, K / 2) bytes) and the four scale_*
 * fields point at their e8m0 BLOCK scales (contiguous (N, K / 32) bytes, no alignment asked) instead of fp32 row scales; every
 * product is u2tok_gemm_rows_w4's (below); E, Hq * D and I must then be multiples of 128 and the weights 16-byte aligned.  It runs
 * at B <= 64, batched or not, with kv_start and with adapters as the other two forms do.  (The form is said by the config and the
 * descriptor keeps its 17 pointers, so that a descriptor filled by a caller of an earlier version stays valid as it is.)  Some but
 * not all, or none, of the block scales set, a wform other than 0 or 2, E, Hq * D or I not a multiple of 128: U2TOK_ERR_ARG from
 * pre (q|k|v) or post before anything is launched. */
typedef struct u2tok_decode_config {
  int32_t B, E, Hq, Hkv, D, I; /* new tokens (= batch), hidden size, query / key-value heads, head dim, MLP width */
  float eps, qk_eps, scale;    /* RMSNorm eps, q / k norm eps, softmax scale */
  int32_t wform;               /* what the layer's scale_* are: 0 = fp32 row scales (all NULL: weights in the element type; all set:
                                  e4m3 codes), 2 = e8m0 block-scale bytes (all set: e2m1 codes) */
} u2tok_decode_config;
/* Unmerged adapters (LoRA) of the step, `layer->lora` (NULL: none).  Each of the four products carries the segments of
 * u2tok_lora_rows (below) that are added to it: q|k|v up to 3 (a packed qkv_proj: one), o up to 1, gate|up up to 2 (a packed
 * gate_up_proj: one), down up to 1; n_* = 0 leaves the product alone.  The group product runs after the product it belongs to --
 * q|k|v: before the head norm and the rotary embedding, so the cache receives adapted keys and values; o and down: after the
 * residual epilogue, Y = rnd(float(Y) + scale u B^T) --, on base weights in the element type, in e4m3 or in e2m1 alike.  With a gate or up
 * segment the pair product takes its unfused form (product, group, SiLU(gate) * up).  `scratch` (16-byte aligned) is the branch's
 * own: 24576 bytes for u (64 rows of 192 elements) followed by the largest u2tok_lora_rows_workspace_bytes of the four groups;
 * u2tok_decoder_decode_workspace_bytes keeps its values.  A segment list u2tok_lora_rows refuses, a count outside its range or a
 * short scratch: U2TOK_ERR_ARG / U2TOK_ERR_WORKSPACE from pre (q|k|v) or post (o, gate|up, down) before anything is launched. */
typedef struct u2tok_lora_seg {
  const void *A, *B;     /* A (r, K), B (N, r): contiguous, element type, 16-byte aligned */
  int32_t r, col0, N;    /* rank; the segment's columns [col0, col0 + N) of Y */
  float scale;
} u2tok_lora_seg;
typedef struct u2tok_decode_lora {
  u2tok_lora_seg qkv[3], o[1], gu[2], down[1];
  int32_t n_qkv, n_o, n_gu, n_down;
  void* scratch;
  size_t scratch_bytes;
} u2tok_decode_lora;
typedef struct u2tok_decode_layer {
  const void *w_in_norm, *Wqkv, *bqkv, *wq_norm, *wk_norm;       /* first half */
  const void *Wo, *bo, *w_post_norm, *Wgu, *bgu, *Wdown, *bdown; /* second half */
  const float *scale_qkv, *scale_o, *scale_gu, *scale_down;      /* all NULL: weights in the element type;
                                                                    all set: the four W* are e4m3 codes, a scale per row --
                                                                    cfg->wform = 2: the four W* are e2m1 codes and these
                                                                    are the addresses of their e8m0 block-scale BYTES */
  const u2tok_decode_lora* lora;                                 /* unmerged adapters of the step; NULL: none */
} u2tok_decode_layer;
size_t u2tok_decoder_decode_workspace_bytes(const u2tok_decode_config* cfg, int32_t T);
int u2tok_decoder_decode_pre(const u2tok_decode_config* cfg, const u2tok_decode_layer* layer, const void* x, const void* cos,
                             const void* sin, int32_t cos_sin_f32, int64_t cs_ld, void* qkv, void* k_cache, void* v_cache,
                             int64_t kv_stride, int32_t s_off, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
int u2tok_decoder_decode_post(const u2tok_decode_config* cfg, const u2tok_decode_layer* layer, const void* x, const void* qkv,
                              const void* K, const void* V, int32_t T, int64_t kv_stride, int32_t batched, const int32_t* kv_start,
                              void* out, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* post on an FP8 (e4m3) KV cache (u2tok_kv_quantize_rows below: the format): K / V are replaced by the dense code buffers k_codes /
 * v_codes (B, Hkv, capacity, D) bytes and their scales k_scales / v_scales (B, Hkv, capacity) fp32.  k_new / v_new: the step's
 * 16-bit rows, dense (B, Hkv, 1, D) -- what u2tok_decoder_decode_pre wrote with kv_stride = 0, s_off = 0.  The call quantises them
 * into position s_off of the buffers, then attends over positions k_first .. s_off (a window: k_first > 0) with
 * u2tok_decode_attention_kv8 -- always the batched form: Hq / Hkv <= 16, kv_start (NULL or device int32[B]) counted from k_first
 * --; everything after the attention is u2tok_decoder_decode_post's, all weight forms and adapter groups.  Workspace:
 * u2tok_decoder_decode_workspace_bytes(cfg, s_off - k_first + 1).  Everything either launcher or post refuses, 0 <= k_first <= s_off
 * < capacity violated: U2TOK_ERR_ARG / U2TOK_ERR_WORKSPACE before anything is launched or written. */
int u2tok_decoder_decode_post_kv8(const u2tok_decode_config* cfg, const u2tok_decode_layer* layer, const void* x, const void* qkv,
                                  const void* k_new, const void* v_new, void* k_codes, void* v_codes, float* k_scales, float* v_scales,
                                  int32_t capacity, int32_t k_first, int32_t s_off, const int32_t* kv_start, void* out, void* workspace,
                                  size_t workspace_bytes, u2tok_stream_t stream);
/* ---- one decode step of the WHOLE decoder stack in one call: for each of the n_layers layers exactly the launches of
 * u2tok_decoder_decode_pre followed by u2tok_decoder_decode_post, in their order, on the caller's stream (no graph, nothing
 * captured), so every value has the bits the per-layer calls give it.  Layer l reads the hidden state layer l - 1 wrote (layer 0: x,
 * (B, E) rows) -- it goes through two (B, E) rows of the workspace --; after the last layer the stack's final RMSNorm
 * (w_final_norm, final_eps) writes out (B, E); w_final_norm NULL: out receives the last hidden state as it is.
 * Per layer: its config and descriptor (the weight form may differ from layer to layer; B and E may not), its append-in-place cache
 * buffers k_cache / v_cache (B, Hkv, capacity, D) with kv_stride = capacity * D, the position s_off the step's k / v rows are
 * written at, and the positions k_first .. k_first + T - 1 <= s_off the attention reads (a sliding-window layer: the last min(T, W)).
 * cos / sin / cos_sin_f32 / cs_ld, batched and kv_start: as in the per-layer calls, the same for every layer.
 * EVERY refusal of EVERY layer -- the argument checks of both halves, the weight forms' demands, the adapter groups', the
 * products' and row kernels' own, workspace size, kv_stride -- is evaluated before the first launch: an error code means nothing
 * was launched and no cache row was written.  The library keeps no pointer after the call returns.
 * workspace: u2tok_decoder_decode_stack_workspace_bytes(L, n_layers) bytes (0: descriptors it refuses), 256-byte aligned; its
 * first 4 bytes are the ticket of the tail norms: zeroed ONCE by whoever allocates the workspace, left zero by every call.
 * tail_norm != 0: the three RMSNorms that follow a product with a residual -- o -> the post-attention norm, down of layer l -> the
 * input norm of layer l + 1, the last down -> the final norm -- run in the tail of that product's launch (u2tok_gemm_rows_norm)
 * instead of a launch of their own, with the same bits; a product followed by an adapter group, a product a tile kernel runs and a
 * row wider than 4096 keep the separate launch. */
typedef struct u2tok_decode_stack_layer {
  const u2tok_decode_config* cfg;    /* per layer: wform may differ between layers */
  const u2tok_decode_layer*  layer;
  void *k_cache, *v_cache;           /* the layer's append-in-place buffers (B, Hkv, capacity, D) */
  int64_t kv_stride;
  int32_t s_off;                     /* position the step's k / v rows are written at */
  int32_t k_first, T;                /* attention reads positions k_first .. k_first + T - 1 (window layers: the last min(T, W)) */
} u2tok_decode_stack_layer;
size_t u2tok_decoder_decode_stack_workspace_bytes(const u2tok_decode_stack_layer* L, int32_t n_layers);
int u2tok_decoder_decode_stack(const u2tok_decode_stack_layer* L, int32_t n_layers, const void* x, const void* cos, const void* sin,
                               int32_t cos_sin_f32, int64_t cs_ld, int32_t batched, const int32_t* kv_start,
                               const void* w_final_norm /* NULL: none */, float final_eps, int32_t tail_norm, void* out,
                               void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* ---- the head of a decode step: everything between the last layer and the next token's logits.  For the B <= 64 rows of a step,
 *   xn     = what u2tok_rmsnorm_bf16 makes of the UN-NORMED hidden rows x (B, E; ldx elements between rows) with w_norm and eps;
 *   logits = (B, V) FP32, ld_logits >= V floats between rows: what the few-rows product of the head's weight form makes of xn with
 *            fp32 C (flag 16) -- wform 0: u2tok_gemm_rows on W (V, E) in the element type; 1: u2tok_gemm_rows_w8_wide on e4m3 codes
 *            with scale = fp32 (V); 2: u2tok_gemm_rows_w4 on e2m1 codes with scale = the e8m0 block-scale bytes (V, E / 32)
 * -- bit for bit: the entry adds no kernel, it launches those two.  The logits are not rounded to 16 bits on the way.  Columns of
 * the logits' rows beyond V are neither read nor written.  ldw (elements for wform 0, bytes for codes) and lds (bytes): 0 = dense.
 * U2TOK_ERR_ARG, nothing launched: B outside 1 .. 64, V < 2, a null pointer (scale with wform 1 / 2), an unknown wform, ldx < E,
 * ld_logits < V, a workspace not 16-byte aligned, and everything u2tok_rmsnorm_bf16 (E % 8, E <= 8192, 16-byte aligned x and
 * w_norm) and the product of that form (E % 32 / 64 / 128, 16-byte aligned W, ...) refuse; U2TOK_ERR_WORKSPACE: fewer than
 * u2tok_decode_head_workspace_bytes(B, E) bytes (the normed rows; 0 for B outside 1 .. 64 or E < 1). */
typedef struct u2tok_decode_head_desc {
  const void* w_norm;  /* (E), element type: the stack's final RMSNorm */
  const void* W;       /* (V, E) in wform */
  const void* scale;   /* wform 0: ignored; 1: fp32 (V); 2: e8m0 bytes (V, E / 32) */
  int32_t E, V;
  int32_t wform;       /* 0 = element type, 1 = e4m3 with a scale per row, 2 = e2m1 with e8m0 block scales */
  float eps;
  int64_t ldw, lds;    /* 0: dense */
} u2tok_decode_head_desc;
size_t u2tok_decode_head_workspace_bytes(int32_t B, int32_t E);
int u2tok_decode_head(const u2tok_decode_head_desc* head, const void* x, int64_t ldx, int32_t B, float* logits, int64_t ld_logits,
                      void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* u2tok_decoder_decode_stack (with w_final_norm = NULL: out (B, E) receives the last layer's hidden rows as they are) followed by
 * u2tok_decode_head on out, in ONE call with the bits of the two.  The stack step's rule covers both: every refusal of every layer
 * AND of the head is evaluated before the first launch -- an error code means nothing was launched, no cache row, hidden row or logit
 * was written.  head->E must be the layers' E, B is theirs.  workspace: u2tok_decoder_decode_stack_head_workspace_bytes(L, n_layers,
 * head) bytes (0: descriptors it refuses) -- the stack step's workspace, ticket included, followed by the head's --, 256-byte aligned. */
size_t u2tok_decoder_decode_stack_head_workspace_bytes(const u2tok_decode_stack_layer* L, int32_t n_layers, const u2tok_decode_head_desc* head);
int u2tok_decoder_decode_stack_head(const u2tok_decode_stack_layer* L, int32_t n_layers, const void* x, const void* cos, const void* sin,
                                    int32_t cos_sin_f32, int64_t cs_ld, int32_t batched, const int32_t* kv_start, int32_t tail_norm,
                                    void* out, const u2tok_decode_head_desc* head, float* logits, int64_t ld_logits, void* workspace,
                                    size_t workspace_bytes, u2tok_stream_t stream);
/* ---- the whole-stack step, and the step with the head, on an FP8 (e4m3) KV cache: u2tok_decoder_decode_stack /
 * u2tok_decoder_decode_stack_head with every layer's cache as the dense code buffers k_codes / v_codes (B, Hkv, capacity, D) bytes
 * and scales k_scales / v_scales (B, Hkv, capacity) fp32 of u2tok_decoder_decode_post_kv8.  Per layer the launches are those of
 * u2tok_decoder_decode_pre with u2tok_qk_norm_rope_kv8 in the rotary kernel's place -- the step's k / v rows go to position s_off
 * as codes in that launch, no 16-bit row is written and nothing is quantised afterwards -- followed by those of
 * u2tok_decoder_decode_post_kv8 from u2tok_decode_attention_kv8 on: as many launches as a layer of the 16-bit stack step has, and
 * every value -- hidden rows, codes, scales, logits -- has the bits the per-layer calls on such a cache give it.  The attention is
 * always the batched form (no `batched` argument; Hq / Hkv <= 16) over positions k_first .. s_off, kv_start counted from k_first.
 * All weight forms, adapter groups, tail_norm, w_final_norm and the head: as in the 16-bit entries.  The workspace has their layout
 * and their size on the same (cfg, T): u2tok_decoder_decode_stack_kv8_workspace_bytes / _head_kv8_workspace_bytes (0: descriptors
 * they refuse), 256-byte aligned, the ticket in its first 4 bytes.
 * EVERY refusal of every layer and of the head precedes the first launch -- everything the 16-bit entries refuse, everything
 * u2tok_qk_norm_rope_kv8 and u2tok_decode_attention_kv8 refuse (a null or misaligned code or scale buffer among them), and
 * 0 <= k_first <= s_off < capacity with T == s_off - k_first + 1 violated: U2TOK_ERR_ARG / U2TOK_ERR_WORKSPACE, and no code, scale,
 * hidden row or logit was written. */
typedef struct u2tok_decode_stack_layer_kv8 {
  const u2tok_decode_config* cfg;    /* per layer: wform may differ between layers */
  const u2tok_decode_layer*  layer;
  void *k_codes, *v_codes;           /* (B, Hkv, capacity, D) bytes */
  float *k_scales, *v_scales;        /* (B, Hkv, capacity) fp32 */
  int32_t capacity;
  int32_t s_off;                     /* position the step's k / v rows are written at */
  int32_t k_first, T;                /* attention reads positions k_first .. k_first + T - 1 = s_off */
} u2tok_decode_stack_layer_kv8;
size_t u2tok_decoder_decode_stack_kv8_workspace_bytes(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers);
int u2tok_decoder_decode_stack_kv8(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers, const void* x, const void* cos,
                                   const void* sin, int32_t cos_sin_f32, int64_t cs_ld, const int32_t* kv_start,
                                   const void* w_final_norm /* NULL: none */, float final_eps, int32_t tail_norm, void* out,
                                   void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
size_t u2tok_decoder_decode_stack_head_kv8_workspace_bytes(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers,
                                                           const u2tok_decode_head_desc* head);
int u2tok_decoder_decode_stack_head_kv8(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers, const void* x, const void* cos,
                                        const void* sin, int32_t cos_sin_f32, int64_t cs_ld, const int32_t* kv_start, int32_t tail_norm,
                                        void* out, const u2tok_decode_head_desc* head, float* logits, int64_t ld_logits,
                                        void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* ---- products on FP8 weights (weight-only: OCP e4m3 codes, one fp32 scale per weight row; activations, biases, norms,
 * attention and the KV cache stay in the element type).  A product is exactly x . (scale[n] * e4m3(W8[n][:])) with fp32
 * accumulation -- the codes are widened to the element type in registers, where every e4m3 value is exact --, so all the loss is
 * the quantiser's (u2tokenizer_amd/ops.py: quantize_rows_fp8).  The weight bytes of a step, which bound it, are halved.
 * u2tok_gemm_rows_w8: C (M <= 16, N) = epilogue(scale[n] * sum_k A[m][k] e4m3(W8[n][k])); W8 (N, K) bytes, ldw bytes between rows;
 * flags of u2tok_gemm_bf16: 1 (bias[n]), 8 (+ R, ldr), 16 (fp32 C), or 512 ALONE (W8 = gate rows | up rows, N = 2 I, I % 8 == 0,
 * C (M, I) = bf16(silu(bf16(gate))) * bf16(up): the values of the product followed by u2tok_swiglu_bf16, bit for bit).
 * K % 64 == 0, lda % 8 == 0, ldw % 16 == 0, A and W8 16-byte aligned, scale non-null; U2TOK_ERR_ARG otherwise, nothing launched.
 * Bit-repeatable (partial sums are added in a fixed order).
 * u2tok_gemm_rows_w8_wide: the same product for 1 <= M <= 64, every other argument and refusal as above.  M <= 16: the same launch.
 * 16 < M <= 64: each weight fragment is loaded once and feeds one MFMA per block of 16 rows; row m has exactly the bits it has as
 * row m % 16 of the M <= 16 product on rows 16 (m / 16) .. min(M, 16 (m / 16) + 16) - 1 (same K slices, same accumulator chains,
 * same order of the partial sums, same epilogue).  (u2tok_gemm_rows_w8 itself keeps refusing M > 16, as published.) */
int u2tok_gemm_rows_w8(const void* A, const void* W8, const float* scale, void* C, const void* bias, const void* R, int32_t M,
                       int32_t N, int32_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags,
                       u2tok_stream_t stream);
int u2tok_gemm_rows_w8_wide(const void* A, const void* W8, const float* scale, void* C, const void* bias, const void* R, int32_t M,
                            int32_t N, int32_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags,
                            u2tok_stream_t stream);
/* ---- products on MXFP4 weights (OCP Microscaling FP4, weight-only).  An (N, K) weight is
 *   codes : (N, K / 2) bytes of e2m1 codes (sign, 2 exponent bits, 1 mantissa bit: 0, .5, 1, 1.5, 2, 3, 4, 6 and their negatives), the
 *           code of EVEN k in the LOW nibble of byte k / 2; ldw bytes between rows, ldw % 16 == 0, ldw >= K / 2, base 16-byte aligned;
 *   scales: (N, K / 32) bytes, e8m0: byte e scales the 32 consecutive k = 32 j .. 32 j + 31 of one weight row by 2^(e - 127); lds
 *           bytes between rows, lds >= K / 32;
 *   K % 128 == 0.
 * Activations, biases, norms, attention and the KV cache stay in the element type.  A product is exactly
 * epilogue(sum_k A[m][k] * e2m1(code[n][k]) * 2^(e[n][k / 32] - 127)) with fp32 accumulation: codes are widened WITH their scale to
 * the element type in registers (v_cvt_scalef32_pk_{bf16,f16}_fp4), and every e2m1 * 2^x is exact in bf16 and in fp16 for the
 * scales the quantiser emits (u2tokenizer_amd/ops.py: quantize_blocks_fp4, x = e - 127 in [-23, 13]), so all the loss is the
 * quantiser's.  For a scale byte outside that range the weight is whatever the conversion instruction rounds e2m1 * 2^x to in the
 * element type (fp16: subnormals, zero or infinity; e = 255 is NaN in e8m0 and not interpreted here).
 * u2tok_gemm_rows_w4: C (M, N), 1 <= M <= 64 in this one entry; flags of u2tok_gemm_rows_w8: 1 (bias[n]), 8 (+ R, ldr), 16 (fp32 C),
 * or 512 ALONE (W4 = gate rows | up rows, N = 2 I, I % 8 == 0, C (M, I) = bf16(silu(bf16(gate))) * bf16(up)).  K % 128 != 0, a
 * misaligned A / W4 / C, lda % 8 != 0 or a leading dimension below its row, a null S, M outside 1 .. 64, unknown flags:
 * U2TOK_ERR_ARG, nothing launched.  16 < M <= 64: the block-of-16 contract of u2tok_gemm_rows_w8_wide.  Bit-repeatable. */
int u2tok_gemm_rows_w4(const void* A, const void* W4, const uint8_t* S, void* C, const void* bias, const void* R, int32_t M,
                       int32_t N, int32_t K, int64_t lda, int64_t ldw, int64_t lds, int64_t ldc, int64_t ldr, int32_t flags,
                       u2tok_stream_t stream);
/* The few-rows (weight-streaming) product on weights in the element type, called directly instead of through u2tok_gemm_bf16's
 * plan: C (M, N) = epilogue(sum_k A[m][k] W[n][k]), 1 <= M <= 64, W (N, K) with ldw elements between rows, K % 32 == 0, one batch
 * entry; flags 1 (bias[n]), 8 (+ R, ldr), 16 (fp32 C), or 512 ALONE (W = gate rows | up rows, N = 2 I, I % 8 == 0, C (M, I) =
 * bf16(silu(bf16(gate))) * bf16(up)); lda % 8 == 0, ldw % 8 == 0, A and W 16-byte aligned; U2TOK_ERR_ARG otherwise, nothing
 * launched.  M <= 16: the kernel u2tok_gemm_bf16 picks for such a product, bit for bit.  16 < M <= 64: the block-of-16 contract
 * of u2tok_gemm_rows_w8_wide.  Bit-repeatable. */
int u2tok_gemm_rows(const void* A, const void* W, void* C, const void* bias, const void* R, int32_t M, int32_t N, int32_t K,
                    int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags, u2tok_stream_t stream);
/* The few-rows product with the RMSNorm of its finished rows in the SAME launch: C as u2tok_gemm_rows (wform = 0; scale ignored),
 * u2tok_gemm_rows_w8_wide (wform = 1; scale: fp32 per weight row) or u2tok_gemm_rows_w4 (wform = 2; scale: the e8m0 block-scale
 * bytes, lds bytes between rows) computes it, bit for bit, and Yn (M, N; ldn elements between rows) = what u2tok_rmsnorm_bf16 makes
 * of C with w_norm and eps, bit for bit.  Each workgroup releases its part of C at device scope and draws a ticket with an atomic
 * add; the one that draws the last ticket acquires, norms the M rows (a wave per row) and puts the ticket back to 0 -- nobody
 * waits for another workgroup.  ticket: 4 bytes of device memory, 4-byte aligned, that read 0 before the call (they read 0 again
 * after it); two launches that may overlap must not share one.
 * Only the non-pair form WITH a residual: flags 8, optionally | 1; C in the element type; N % 8 == 0, N <= 4096, ldc % 8 == 0,
 * ldn % 8 == 0, C / w_norm / Yn 16-byte aligned.  The pair flag, fp32 C, no residual, a null w_norm / Yn / ticket, a misaligned
 * ticket, and everything the plain product refuses: U2TOK_ERR_ARG, nothing launched, nothing written. */
int u2tok_gemm_rows_norm(const void* A, const void* W, void* C, const void* bias, const void* R, int32_t M, int32_t N, int32_t K,
                         int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags, int32_t wform, const void* scale,
                         int64_t lds, const void* w_norm, float eps, void* Yn, int64_t ldn, void* ticket, u2tok_stream_t stream);
/* Batched decode attention: out[b] = softmax(q[b] K[b]^T scale over keys kv_start[b] <= j < T) V[b] for B sequences of ONE query
 * row each.  q / out: (B, Hq * D) rows, ldq / ldo elements apart (head h at column h * D); K / V: (B, Hkv, T, D), kv_stride
 * elements between (batch, kv head) entries (0: dense, T * D) -- an append-in-place buffer or the dense cache; D in {64, 96, 128},
 * Hq / Hkv <= 16, B <= 65535.  One workgroup per (sequence, kv head, key split) stages each K / V tile once for the whole group of
 * query heads; the splits are fixed ranges of [0, T) (tiles wholly below kv_start[b] are skipped, a split without a visible key is
 * empty), their fp32 partial results are merged in a fixed order: no atomics, bit-repeatable.  A sequence without a visible key
 * gets zeros.  workspace: u2tok_decode_attention_workspace_bytes(B, Hq, Hkv, T, D) bytes (0: no splits), 16-byte aligned. */
size_t u2tok_decode_attention_workspace_bytes(int32_t B, int32_t Hq, int32_t Hkv, int32_t T, int32_t D);
int u2tok_decode_attention(const void* q, const void* K, const void* V, void* out, int32_t B, int32_t Hq, int32_t Hkv, int32_t T,
                           int32_t D, int64_t ldq, int64_t kv_stride, int64_t ldo, float scale, const int32_t* kv_start,
                           void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* ---- the FP8 (e4m3) KV cache.  One row = the D values of one (sequence, kv head, position), K and V each: scale = amax / 448 in
 * fp32 (an all-zero row: 1.0), code = e4m3fn(clamp(x / scale, +-448)), round to nearest even, IEEE division; the NaN codes never
 * occur; value = code x scale exactly.  Finite inputs only (a non-finite row does not fault; its codes are unspecified).
 * u2tok_kv_quantize_rows: k / v (B, Hkv, n, D) rows in the element type -- unit stride inside a row, *_bs / *_hs / *_rs elements
 * between sequences / heads / positions, multiples of 8, 16-byte aligned -- into positions s_off .. s_off + n - 1 of the dense
 * buffers k_codes / v_codes (B, Hkv, capacity, D) bytes (16-byte aligned) and k_scales / v_scales (B, Hkv, capacity) fp32, K and
 * V in one launch; bit-equal to ops.quantize_kv_fp8.  D in {64, 96, 128}.  A null pointer, a misaligned one, another D,
 * s_off + n > capacity: U2TOK_ERR_ARG, nothing launched, nothing written.
 * u2tok_decode_attention_kv8: u2tok_decode_attention over codes -- the same splits, fp32 partials merged in ascending order, no
 * atomics, bit-repeatable, zeros for a sequence without a visible key.  kv_stride BYTES between (batch, kv head) code entries (0:
 * dense, T * D; a multiple of 16), scale_stride floats between their scale entries (0: T).  Codes are widened to the element type
 * in registers (exact), the MFMAs stay in the element type: s_j = k_scales[j] * sum_d q_d code(K_jd), p_j = exp2(s_j c - m), the
 * row sum takes p_j, the P operand is rnd(p_j * v_scales[j]) (the IEEE-half build: times 2^8, undone where the sum is divided).
 * workspace: u2tok_decode_attention_kv8_workspace_bytes (= u2tok_decode_attention_workspace_bytes).
 * u2tok_attention_kv8_rows: the same attention for Sq >= 1 NEW positions per sequence (a continued prefill on such a cache: a prompt
 * fed in chunks, a second turn, draft verification).  q / out: B * Sq rows, row b * Sq + i at ldq / ldo elements apart (the q
 * columns of packed q|k|v rows; a dense context).  Codes, scales, kv_stride, sc_stride as above, the pointers advanced to the first
 * position read; T counts the positions read, the Sq new ones last.  Row i sees key j iff kv_start[b] <= j <= i + T - Sq and, for
 * window W > 0, j > i + T - Sq - W (window = 0: no lower edge).  The 16 rows of a workgroup's operand are 16 consecutive flat rows
 * i * (Hq / Hkv) + head-in-group of one kv head, so the cache is read once per 16 such rows: the form for few new positions.  A
 * row that sees no key: zeros.  Bit-repeatable; Sq = 1, window = 0 gives the bits of u2tok_decode_attention_kv8.  Everything that
 * entry refuses, Sq < 1, Sq > T, window < 0, B * Sq * Hq >= 2^31: U2TOK_ERR_ARG / U2TOK_ERR_WORKSPACE before anything is launched.
 * workspace: u2tok_attention_kv8_rows_workspace_bytes. */
int u2tok_kv_quantize_rows(const void* k, const void* v, int32_t B, int32_t Hkv, int32_t n, int32_t D, int64_t k_bs, int64_t k_hs,
                           int64_t k_rs, int64_t v_bs, int64_t v_hs, int64_t v_rs, void* k_codes, void* v_codes, float* k_scales,
                           float* v_scales, int32_t capacity, int32_t s_off, u2tok_stream_t stream);
size_t u2tok_decode_attention_kv8_workspace_bytes(int32_t B, int32_t Hq, int32_t Hkv, int32_t T, int32_t D);
int u2tok_decode_attention_kv8(const void* q, const void* k_codes, const void* v_codes, const float* k_scales, const float* v_scales,
                               void* out, int32_t B, int32_t Hq, int32_t Hkv, int32_t T, int32_t D, int64_t ldq, int64_t kv_stride,
                               int64_t scale_stride, int64_t ldo, float scale, const int32_t* kv_start, void* workspace,
                               size_t workspace_bytes, u2tok_stream_t stream);
size_t u2tok_attention_kv8_rows_workspace_bytes(int32_t B, int32_t Sq, int32_t Hq, int32_t Hkv, int32_t T, int32_t D);
int u2tok_attention_kv8_rows(const void* q, const void* k_codes, const void* v_codes, const float* k_scales, const float* v_scales,
                             void* out, int32_t B, int32_t Sq, int32_t Hq, int32_t Hkv, int32_t T, int32_t D, int64_t ldq,
                             int64_t kv_stride, int64_t sc_stride, int64_t ldo, float scale, int32_t window, const int32_t* kv_start,
                             void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* in-place rotate-half RoPE (rope.py:6-13,77-80): rows indexed (outer, s, inner), position = s; inverse != 0 rotates
 * the other way (the backward of the rotation) */
int u2tok_rope_apply(void* x, int64_t n_outer, int32_t S, int32_t n_inner, int32_t H, int32_t d, int64_t ld,
                     int32_t max_len, int32_t inverse, u2tok_stream_t stream);

/* ---- backward-pass building blocks ("next" row f1: training through the path) ---------------------------------------
 * The GEMM-shaped parts of the backward (dX = dY W, dW = dY^T X, dQ / dK / dV / dP of the attention cores) are
 * u2tok_gemm_bf16 calls on (transposed) operands; these are the rest.  The host side (u2tokenizer_amd/autograd.py)
 * sequences them behind torch.autograd.Function so that the drop-in modules train (train_stage1.py:244-251). */
/* y = gelu(z): the approximation of u2tok_gemm_bf16's flag 4 (|y - z Phi(z)| <= 3.3e-6 before rounding to the element type);
 * dz = dy gelu'(z) with gelu' the derivative of EXACT erf-GELU, Phi(z) + z phi(z).  n % 8 == 0, 16-byte aligned buffers. */
int u2tok_gelu_fwd(const void* z, void* y, int64_t n, u2tok_stream_t stream);
int u2tok_gelu_bwd(const void* z, const void* dy, void* dz, int64_t n, u2tok_stream_t stream);
/* out[c] (+)= sum_r x[r][c] (* y[r][c] when y != NULL) in fp32, fixed summation order (bit-repeatable); out (fp32)
 * and / or out_bf16 receive the result; workspace: u2tok_colsum_workspace_bytes. */
size_t u2tok_colsum_workspace_bytes(int32_t rows, int32_t C);
int u2tok_colsum_bf16(const void* x, const void* y, float* out, void* out_bf16, int32_t rows, int32_t C, int64_t ldx,
                      int64_t ldy, void* workspace, int32_t accumulate, u2tok_stream_t stream);
/* Backward of y = LayerNorm(x (+ res)) * w + b (rows x C, dense): dv = gradient w.r.t. x (== w.r.t. res), dw / db:
 * fp32 [C] (overwritten, or added to when accumulate != 0). */
size_t u2tok_layernorm_bwd_workspace_bytes(int32_t rows, int32_t C);
int u2tok_layernorm_bwd(const void* x, const void* res, const void* w, const void* dy, void* dv, float* dw, float* db,
                        int32_t rows, int32_t C, float eps, void* workspace, int32_t accumulate, u2tok_stream_t stream);
/* dS = P * (dP - rowsum(P * dP)) per row; P, dS bf16 [nrows][ldp] (columns >= n of dS zeroed), dP fp32 [nrows][lddp] */
int u2tok_softmax_bwd(const void* P, const float* dP, void* dS, int64_t nrows, int32_t n, int64_t ldp, int64_t lddp,
                      u2tok_stream_t stream);
/* gradient of the relative-bias table (rma.py:64-70): dtable[d + max_len - 1][h] += sum over z % H == h and the
 * diagonal j - i = d of dS[z][i][j];  dS: bf16 [nz][S][ldp];  dtable: fp32 [2 max_len - 1][H] */
int u2tok_relbias_grad(const void* dS, float* dtable, int32_t nz, int32_t S, int32_t H, int64_t ldp, int32_t max_len,
                       u2tok_stream_t stream);
int u2tok_rowdot_bf16(const void* a, const void* b, float* out, int64_t rows, int32_t C, int64_t lda, int64_t ldb,
                      u2tok_stream_t stream);

/* One rank's shard of a ZeRO-1 AdamW step (config/ds_config.json:27-41; u2tokenizer_amd/dp.py): fp32 master weights and
 * moments (n elements each) updated in place from the bf16 gradient piece scaled by grad_scale (1 / world size) and, when
 * grad_coef != NULL, by the device scalar *grad_coef (the clipping coefficient); out_bf16 receives the rounded new master
 * (the piece the all-gather sends).  torch.optim.AdamW arithmetic; step = 1-based step count (bias corrections).  group:
 * optional per-element parameter-group index (uint8) into the host tables lr[ngroups] / weight_decay[ngroups], ngroups <= 8. */
int u2tok_adamw_step(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, const uint8_t* group, void* out_bf16,
                     int64_t n, const float* lr, const float* weight_decay, int32_t ngroups, float beta1, float beta2, float eps,
                     int32_t step, float grad_scale, const float* grad_coef, u2tok_stream_t stream);

/* Fused backward of the ViT attention core (MONAI SABlock, vit.py:100-105; head dim 64, no bias):
 *   out = softmax(q k^T * scale) v   ->   dq, dk, dv   from q, k, v, out and d_out,
 * replacing what torch.autograd does for the reference (softmax / matmul backward through the (S x S) probabilities, 1.6 GB
 * fp32 per layer at S = 2049) by two flash-style kernels that rebuild the probabilities tile by tile.  All S rows of a batch
 * in one row-major bf16 view: q, k, v row r of batch b at + b*bs_qkv + r*ld_qkv, head h at column h*64 (16-byte aligned
 * bases, strides % 8 == 0); out / d_out with ld_o / bs_o; dq, dk, dv with ld_d / bs_d (may be slices of one packed
 * buffer).  lse: the row statistics of u2tok_flash_attention_d64_lse ((nb * H, lse_ld) floats), or NULL -- the backward then
 * rebuilds them in an extra sweep over the keys.  workspace: u2tok_flash_attention_d64_bwd_workspace_bytes(), 256-byte
 * aligned.  No atomics: bit-repeatable. */
size_t u2tok_flash_attention_d64_bwd_workspace_bytes(int32_t nb, int32_t S, int32_t H);
int32_t u2tok_flash_attention_d64_bwd(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t bs_qkv,
                                      const void* out, const void* d_out, int64_t ld_o, int64_t bs_o, void* dq, void* dk,
                                      void* dv, int64_t ld_d, int64_t bs_d, int32_t nb, int32_t S, int32_t H, float scale,
                                      const float* lse, int64_t lse_ld, void* workspace, size_t workspace_bytes,
                                      u2tok_stream_t stream);

/* ---- the decoder's training route (u2tokenizer_amd/decoder_train.py; opt-in): the backward of the decoder layer ------------
 * Causal grouped-query attention with a per-sequence key length: u2tok_attention_gqa's call, plus kv_len (device int32[nb]
 * or NULL: query i of sequence b sees key j iff j <= i + Skv - Sq and j < kv_len[b] -- HF's causal mask of a right-padded
 * 2-D attention mask; kv_len[b] >= 1) and lse (NULL, or (nb * Hq, lse_ld) floats: log2 sum_j exp2(q.k_j scale log2 e) of
 * each query row over its visible keys, for u2tok_attention_gqa_bwd).  Both NULL: exactly u2tok_attention_gqa. */
int u2tok_attention_gqa_ex(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                           int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                           int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, int32_t causal, const int32_t* kv_len,
                           float* lse, int64_t lse_ld, u2tok_stream_t stream);
/* The same with a first visible key per sequence: kv_start (device int32[nb] or NULL) -- key j of sequence b is visible iff
 * kv_start[b] <= j < kv_len[b] (and j <= i + Skv - Sq when causal): HF's mask of a LEFT-padded 2-D attention mask (kv_start) or a
 * right-padded one (kv_len).  A query row that sees no key (a padding position) gets exact zeros, and 0 in lse.  Either pointer may
 * be NULL; all three NULL: exactly u2tok_attention_gqa. */
int u2tok_attention_gqa_range(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                              int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                              int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, int32_t causal, const int32_t* kv_start,
                              const int32_t* kv_len, float* lse, int64_t lse_ld, u2tok_stream_t stream);
/* The same reading K / V where a KV cache keeps them, and with an attention window (the decoder's continued prefill: new positions
 * against a filled cache, a prefill longer than the window of a sliding-window layer).  k_hs / v_hs: elements between the kv heads of
 * one sequence -- d for the column-packed (nb, Skv, Hkv * d) view of the calls above; for the view [:, :, :Skv] of a cache buffer
 * (B, Hkv, capacity, d): ldk = d, k_hs = capacity * d, k_bs = Hkv * capacity * d (multiples of 8; nothing is copied).  window = W > 0
 * (causal only): key j is visible to query i iff i + Skv - Sq - W < j <= i + Skv - Sq -- W keys, the query's own included, HF's
 * sliding-window rule --, intersected with kv_start[b] <= j < kv_len[b] when those are given; 0: no window.  A row that sees no key
 * gets exact zeros (lse 0).  d = 64, 96 or 128.  k_hs = v_hs = d and window = 0: exactly u2tok_attention_gqa_range (all range
 * pointers NULL as well: exactly u2tok_attention_gqa). */
int u2tok_attention_gqa_band(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                             int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                             int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, int32_t causal, const int32_t* kv_start,
                             const int32_t* kv_len, float* lse, int64_t lse_ld, int64_t k_hs, int64_t v_hs, int32_t window,
                             u2tok_stream_t stream);
/* Its backward (causal, Sq = Skv = S, d = 64 or 128): dq, dk, dv from q, k, v, out, d_out and (optional) lse of
 * u2tok_attention_gqa_ex, honouring kv_len.  Layout of u2tok_flash_attention_d64_bwd with Hq query heads (q / dq: head h at
 * column h*d) and Hkv kv heads (k, v / dk, dv: head h at column h*d of their pointers): with q | k | v column views of one
 * packed (rows, (Hq + 2 Hkv) d) buffer, dq | dk | dv land in one packed gradient.  dk / dv of a kv head sum its Hq / Hkv query
 * heads in a fixed order; no atomics: bit-repeatable.  workspace: u2tok_attention_gqa_bwd_workspace_bytes(), 256-byte aligned. */
size_t u2tok_attention_gqa_bwd_workspace_bytes(int32_t nb, int32_t S, int32_t Hq);
int u2tok_attention_gqa_bwd(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t bs_qkv, const void* out,
                            const void* d_out, int64_t ld_o, int64_t bs_o, void* dq, void* dk, void* dv, int64_t ld_d, int64_t bs_d,
                            int32_t nb, int32_t S, int32_t Hq, int32_t Hkv, int32_t d, float scale, const int32_t* kv_len,
                            const float* lse, int64_t lse_ld, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* The same backward at head dim 96 (Phi-3: 32 heads of 96), the argument list of u2tok_attention_gqa_bwd without d: the same
 * launcher, checks, layout and workspace (u2tok_attention_gqa_bwd_workspace_bytes()); u2tok_attention_gqa_bwd itself takes
 * 64 and 128 only. */
int u2tok_attention_gqa_bwd_d96(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t bs_qkv, const void* out,
                                const void* d_out, int64_t ld_o, int64_t bs_o, void* dq, void* dk, void* dv, int64_t ld_d,
                                int64_t bs_d, int32_t nb, int32_t S, int32_t Hq, int32_t Hkv, float scale, const int32_t* kv_len,
                                const float* lse, int64_t lse_ld, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* RMSNorm backward (forward: u2tok_rmsnorm_bf16; x, dy, dres, dx dense (rows, C), C % 8 == 0, C <= 4096):
 *   dx = d/dx + dres (dres: the residual stream's gradient, or NULL);  dw (fp32, C) = sum_rows dy bf16(x rstd), added to dw when
 *   accumulate, in a fixed order.  workspace: u2tok_rmsnorm_bwd_workspace_bytes(). */
size_t u2tok_rmsnorm_bwd_workspace_bytes(int32_t rows, int32_t C);
int u2tok_rmsnorm_bwd(const void* x, const void* w, const void* dy, const void* dres, void* dx, float* dw, int32_t rows, int32_t C,
                      float eps, void* workspace, size_t workspace_bytes, int32_t accumulate, u2tok_stream_t stream);
/* Head norm + rotary backward, in place on the q / k columns of a packed gradient dqkv[rows][(Hq + 2 Hkv) D] (forward:
 * u2tok_qk_norm_rope): the inverse rotation, then (wq / wk given) the per-head RMSNorm backward from the pre-norm q | k heads
 * pre[rows][ld_pre >= (Hq + Hkv) D], dwq / dwk (fp32, D) summed over rows and heads; v columns untouched.
 * workspace: u2tok_qk_norm_rope_bwd_workspace_bytes() (norm only; may be NULL without). */
size_t u2tok_qk_norm_rope_bwd_workspace_bytes(int64_t rows, int32_t D);
int u2tok_qk_norm_rope_bwd(void* dqkv, const void* pre, const void* wq, const void* wk, const void* cos, const void* sin,
                           int32_t cos_sin_f32, int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t ld_pre,
                           int64_t cs_ld, float eps, float* dwq, float* dwk, void* workspace, size_t workspace_bytes,
                           int32_t accumulate, u2tok_stream_t stream);
/* SwiGLU backward (forward: u2tok_swiglu_bf16): from the gate | up pre-activations gu[rows][ld_gu >= 2I] and d(act)
 * dact[rows][ld_da >= I]: dgu[rows][ld_dgu >= 2I] = [d_gate | d_up], the packed gradient of the gate|up product. */
int u2tok_swiglu_bwd(const void* gu, const void* dact, void* dgu, int64_t rows, int32_t I, int64_t ld_gu, int64_t ld_da,
                     int64_t ld_dgu, u2tok_stream_t stream);

/* ---- the loss head (u2tokenizer_amd/loss_head.py; opt-in): lm_head + cross-entropy without the rows x vocab logits ----------
 * Both calls work on a block Z of logits: rows x Vs elements (16-byte aligned, leading dimension ldz >= Vs, ldz % 8 == 0,
 * Vs % 8 == 0) holding the vocabulary columns [v0, v0 + Vs); row offsets are 64-bit.  labels: int64[rows].
 * u2tok_ce_lse_update reads the block once and folds it into the per-row running state (fp32[rows] each): m = running maximum,
 * l = running sum of exp(z - m), zt = the label's logit (written when v0 <= label < v0 + Vs, else left alone).  Before the first
 * slice the caller sets m = -inf, l = 0; after the last, the row's log-sum-exp is m + log(l).  No atomics, fixed summation order:
 * bit-repeatable. */
int u2tok_ce_lse_update(const void* Z, int64_t ldz, int32_t rows, int32_t Vs, int64_t v0, const int64_t* labels, float* m, float* l,
                        float* zt, u2tok_stream_t stream);
/* u2tok_ce_lse_update with further per-row statistics folded into the same single read of the block (each optional; with all four
 * pointers NULL this IS u2tok_ce_lse_update).  m, l, zt carry the same bits as u2tok_ce_lse_update writes, whatever else is asked for.
 *   amax, aidx (fp32[rows], int64[rows]; both or neither): the running maximum logit and the FIRST global column v0 + j that holds
 *     it -- larger value first, then smaller index, so the order in which slices are fed does not matter.  The caller sets
 *     amax = -inf, aidx = INT64_MAX before the first slice; a row of -inf only ends at its first column.
 *   zsum (fp32[rows]): the running sum of the row's logits; the caller sets 0.
 *   l2 (fp32[rows]): the running sum of exp(2 (z - m)) against the same running maximum m; the caller sets 0.  After the last
 *     slice log sum exp(2 z) = 2 m + log(l2).
 * NaN logits are outside the contract.  No atomics, fixed order of every reduction: bit-repeatable. */
int u2tok_ce_stats_update(const void* Z, int64_t ldz, int32_t rows, int32_t Vs, int64_t v0, const int64_t* labels, float* m, float* l,
                          float* zt, float* amax, int64_t* aidx, float* zsum, float* l2, u2tok_stream_t stream);
/* In place:  Z[r][j] <- elem(coef[r] * (exp(float(Z[r][j]) - lse[r]) - [v0 + j == labels[r]])),  lse[r] the NATURAL-log sum of
 * exponentials of the whole row (m + log(l) above), coef[r] the upstream gradient of the row's loss: the element-type rounding
 * of the fp32 gradient of the fp32 logits, which is what F.cross_entropy(logits.float(), ...) hands back to lm_head. */
int u2tok_ce_grad_inplace(void* Z, int64_t ldz, int32_t rows, int32_t Vs, int64_t v0, const int64_t* labels, const float* lse,
                          const float* coef, u2tok_stream_t stream);

/* ---- the sampling warper (u2tokenizer_amd/sampling.py; opt-in): temperature, top-k and top-p in one launch, without a sort -------
 * logits / out: rows x V fp32 (4-byte aligned, leading dimensions ld_in, ld_out >= V, 64-bit row offsets); out may be logits.  The same
 * code in both builds (no 16-bit element is involved).  top_k = 0: no top-k stage; top_p = 1: no top-p stage.  Per row:
 *   1. z = x / temperature, one correctly rounded fp32 division (temperature = 1: z = x);
 *   2. top-k, k = min(max(top_k, min_keep), V): z_i < (k-th largest z) is removed; ties with the k-th value stay; -0.0 = +0.0;
 *      exact (counts only);
 *   3. top-p over the survivors, with softmax probabilities (removed and -inf entries: 0): rank by value, among equal values the
 *      HIGHER INDEX ranks higher (the order of a stable ascending sort, read from its end); token i stays iff the mass of the tokens
 *      ranked strictly above it is < top_p, or fewer than min_keep tokens rank above it (transformers' `cumsum <= 1 - top_p` rule
 *      written from the top);
 *   4. out_i = z_i where kept, -inf elsewhere (-inf inputs stay -inf).
 * The masses are summed as integers (exp(z - max) at 2^-40): the result does not depend on scheduling -- the same input gives the
 * same bits.  A row holding NaN, +inf or nothing but -inf gets unspecified values in all of its V elements; the other rows of the
 * call are not affected.
 * workspace: u2tok_sample_warp_workspace_bytes(rows, V) bytes, 4-byte aligned (0 for rows < 1 or V < 2); afterwards it holds one record of
 * eight uint32 per row: the boundary token's (key << 32 | index) composite (low word, high word), the bit from which it is resolved,
 * the histogram passes taken, the top-k key bound, the number of tokens ranked at or above the boundary, two zeros.
 * U2TOK_ERR_ARG: rows < 1, V < 2, temperature <= 0, top_p outside (0, 1], min_keep < 1, top_k < 0, ld < V, a null or misaligned
 * pointer; U2TOK_ERR_WORKSPACE: workspace_bytes too small. */
size_t u2tok_sample_warp_workspace_bytes(int32_t rows, int32_t V);
int u2tok_sample_warp(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int32_t rows, int32_t V, float temperature,
                      int32_t top_k, float top_p, int32_t min_keep, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);
/* The split-row form, for calls of a few rows: the semantics, arguments, refusals and determinism of u2tok_sample_warp word for word,
 * and `out` BIT-EQUAL to its `out` on the same input, with equal kept counts (record word 5; the other record words need not match).
 * A row is spread over min(16, ceil(V / 8192)) workgroups and every pass of the descent is a launch of its own on the caller's
 * stream: each workgroup adds the non-empty bins of its slice's histogram to a per-row table in the workspace with device-scope
 * integer atomics (counts and 2^-40 masses: no sum depends on an order), the NEXT launch reads the table, and every workgroup takes
 * the bin decision from it again.  The kernel boundary is the only ordering between workgroups: nobody spins, nobody waits.  The number
 * of launches follows from the parameters alone (u2tok_sample_warp_split_launches: 3 + 4 with a top-k stage + 8 with a top-p stage
 * + 8 with top-p and min_keep > 1); a launch whose pass is decided already returns at once.  The call does not depend on what the
 * workspace holds at entry (its first launch zeroes what the others accumulate into).  out may be logits: the last launch is the
 * only writer.  workspace: u2tok_sample_warp_split_workspace_bytes(rows, V) bytes, 4-byte aligned: the records of
 * u2tok_sample_warp, then about 61 KB per row. */
size_t u2tok_sample_warp_split_workspace_bytes(int32_t rows, int32_t V);
int32_t u2tok_sample_warp_split_launches(int32_t V, int32_t top_k, float top_p, int32_t min_keep);
int u2tok_sample_warp_split(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int32_t rows, int32_t V, float temperature,
                            int32_t top_k, float top_p, int32_t min_keep, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* ---- rank-r adapter (LoRA) products of the decoder training route (csrc/lora.hip; u2tokenizer_amd/decoder_train.py: LoraDeltaFn) ----
 * Three bandwidth-bound kernels for r in {16, 32, 64}, outside u2tok_gemm_bf16's plan.  All operands are 16-bit elements of the
 * build's type with unit column stride and a leading dimension in elements (multiples of 8; base pointers 16-byte aligned); the big
 * operand also takes an element offset (a multiple of 8), so that a column segment of a packed q|k|v or gate|up activation or
 * gradient is read and written in place.  fp32 accumulation on v_mfma_f32_16x16x32, alpha applied to the fp32 sum, ONE rounding at the
 * store; no atomics, every sum in a fixed order: two calls give the same bits (u2tok_lora_wgrad: for the same workspace_bytes).
 * U2TOK_ERR_ARG, nothing launched: r outside {16, 32, 64}, a shape outside the contract below, a null or misaligned pointer,
 * a leading dimension shorter than its row.
 *
 * u2tok_lora_down:  U (M, r) = alpha X (M, K) A (r, K)^T, K % 32 == 0.  X = X + x_off, rows ldx apart.
 * u2tok_lora_up:    Y (M, N) = [Y +] alpha U (M, r) W (N, r)^T, N % 16 == 0.  Y = Y + y_off, rows ldy apart; accumulate != 0 reads Y:
 *                   float(Y) + alpha acc in fp32 (one fused multiply-add), rounded once; accumulate == 0 never reads Y.  Columns
 *                   of Y's buffer outside [y_off, y_off + N) are neither read nor written.
 * u2tok_lora_wgrad: G (r, C) = alpha U (M, r)^T X (M, C), the contraction over the M rows, C % 8 == 0.  X = X + x_off.  G: elements
 *                   (out_f32 == 0) or fp32 (out_f32 != 0), rows ldg apart.  workspace (optional, 16-byte aligned): with room for s >= 2
 *                   fp32 (r, C) tiles the rows are cut into up to s fixed ranges across workgroups and a second launch adds the
 *                   ranges' tiles in order; 512 / ceil(C / 64) tiles are as many as are ever used.  Without one, a 64-column strip
 *                   of X is one workgroup's. */
int u2tok_lora_down(const void* X, int64_t x_off, int64_t ldx, const void* A, int64_t lda, void* U, int64_t ldu, int32_t M, int32_t K,
                    int32_t r, float alpha, u2tok_stream_t stream);
int u2tok_lora_up(const void* U, int64_t ldu, const void* W, int64_t ldw, void* Y, int64_t y_off, int64_t ldy, int32_t M, int32_t N,
                  int32_t r, float alpha, int32_t accumulate, u2tok_stream_t stream);
int u2tok_lora_wgrad(const void* U, int64_t ldu, const void* X, int64_t x_off, int64_t ldx, void* G, int64_t ldg, int32_t M, int32_t C,
                     int32_t r, float alpha, int32_t out_f32, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

/* ---- the adapter branch of one packed product for a few rows, as a group (csrc/lora_rows.hip): what a decode step adds for its
 * unmerged adapters, in two launches however many of the product's projections are wrapped.  1 <= n <= 3 segments (u2tok_lora_seg,
 * above) share the input X (M, K), 1 <= M <= 64, K % 32 == 0; r_i in {16, 32, 64} (they may differ), N_i % 16 == 0, col0_i % 16 == 0,
 * column ranges disjoint (gaps allowed).  X, U and Y are row-strided (ldx / ldu / ldy elements, multiples of 8; 16-byte aligned):
 *   u_i = rnd(X A_i^T), stored to U at columns sum_{j<i} r_j (ldu >= sum r_j);
 *   Y[:, col0_i : col0_i + N_i] = rnd(float(Y) + scale_i u_i B_i^T), one fused multiply-add on the fp32 sum, rounded once
 * -- the rounding points of u2tok_lora_down followed by u2tok_lora_up's accumulate form.  Launch 1 cuts K into slices of
 * max(8, ceil(K / 32 / 64)) 32-wide steps -- a function of K alone -- and leaves an fp32 16 x r_i tile per (slice, segment, block of
 * 16 rows) in the workspace; launch 2 adds the tiles in slice order, rounds u and runs the rank-r products onto Y.  No atomics: two
 * calls give the same bits, and a block of 16 rows has exactly the bits it has in a call on those rows alone.  Columns of Y outside
 * the segments and rows >= M of U and Y are neither read nor written.
 * U2TOK_ERR_ARG, nothing launched: M, K, n, a rank, N or col0 outside the contract, overlapping segments, ldy shorter than a segment's
 * end, a null or misaligned pointer (the workspace included); U2TOK_ERR_WORKSPACE: fewer than
 * u2tok_lora_rows_workspace_bytes(M, K, segs, n) = ceil(M / 16) * slices * sum r_i * 64 bytes (0 for arguments the call refuses). */
size_t u2tok_lora_rows_workspace_bytes(int32_t M, int32_t K, const u2tok_lora_seg* segs, int32_t n);
int u2tok_lora_rows(const void* X, int64_t ldx, const u2tok_lora_seg* segs, int32_t n, void* U, int64_t ldu, void* Y, int64_t ldy,
                    int32_t M, int32_t K, void* workspace, size_t workspace_bytes, u2tok_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* U2TOK_H_ */
