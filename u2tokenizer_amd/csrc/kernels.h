// Internal C++ launcher API of the u2tok HIP library.  Every function enqueues work on `stream`,
// never allocates, never synchronises, and returns U2_OK or a negative U2_ERR_* code.
#pragma once
#include <algorithm>
#include "common.h"
#include "ctx.h"

namespace u2 {

// ------------------------------------------------------------------ profiling (ctx.hip)
enum : int { PROF_GEMM = 0, PROF_FLASH = 1, PROF_TEMPORAL = 2, PROF_ROWOP = 3, PROF_MOVE = 4, PROF_TOKATTN = 5, PROF_NCAT = 6 };
void prof_enable(bool on);
bool prof_enabled();
int prof_collect(double* ms, double* flops, double* bytes, int64_t* count, int ncat);  // bytes may be null
struct ProfScope {  // brackets one launch with hipEvents on `st` when the current context profiles; free otherwise
  // flops / bytes: ALGORITHMIC work of the launch (2MNK; operands + results once), for the roofline lines of bench.py
  ProfScope(int cat, double flops, hipStream_t st, double bytes = 0.0);
  ~ProfScope();
  int idx_;
  hipStream_t st_;
  Context* c_;
};

// ------------------------------------------------------------------ GEMM (gemm.hip)
enum : int {
  GEMM_BIAS_N = 1,     // + bias[n]   (nn.Linear bias)
  GEMM_BIAS_M = 2,     // + bias[m]   (operand-swapped products, e.g. DiffTS scores^T)
  GEMM_GELU = 4,       // GELU after bias: gelu_epi (common.h), the logistic-polynomial approximation of erf-GELU (|error| <= 3.3e-6)
                       // on the pre-activation rounded to the element type -- not exact erf
  GEMM_RESIDUAL = 8,   // + R[m][n]   (residual stream / position embedding), after GELU
  GEMM_OUT_F32 = 16,   // C is float32 instead of bf16
  GEMM_VEC_OK = 32,    // internal: vector epilogue legal (set by the launcher)
  GEMM_B_KTILE = 64,   // C-ABI only: B is K-tile-major [K/64][N][64] (pack_ktile_major); K % 64 == 0, nz == 1
  GEMM_A_KMAJOR = 128, // A is stored [K][M] (leading dim lda >= M, M % 8 == 0): C = A^T B^T-form products without a transpose
  GEMM_SWIGLU = 512,   // B = [gate rows | up rows] (N = 2 I): C[m][j] = bf16(silu(gate_j)) * up_j, C is [M][I] bf16; no other epilogue
                       // flag, K % 64 == 0, I % 16 == 0 (the 256 x 192-tile kernel stages gate / up rows pairwise, gemm_bt.hip)
  GEMM_B_KMAJOR = 256, // B is stored [K][N] (leading dim ldb >= N, N % 8 == 0); A K-major requires B K-major too
};

struct GemmDesc {
  const bf16_t* A = nullptr;  // [M][K] row-major, leading dim lda ([K][M] with GEMM_A_KMAJOR)
  const bf16_t* B = nullptr;  // [N][K] row-major, leading dim ldb ([K][N] with GEMM_B_KMAJOR)
  void* C = nullptr;          // [M][N] bf16 or f32, leading dim ldc
  const bf16_t* bias = nullptr;
  const bf16_t* R = nullptr;  // [M][N] bf16, leading dim ldr
  int M = 0, N = 0, K = 0;
  int64_t lda = 0, ldb = 0, ldc = 0, ldr = 0;
  int64_t ldbk = 0;  // 0: B rows are K-contiguous; else B is K-tile-major [K/64][N][64] (ldb = 64, ldbk = N * 64)
  // batch z in [0, nz): zb = z / nbh, zh = z % nbh; element offsets zb*s?b + zh*s?h
  int nz = 1, nbh = 1;
  int64_t sAb = 0, sAh = 0, sBb = 0, sBh = 0, sCb = 0, sCh = 0, sRb = 0, sRh = 0;
  float alpha = 1.f;
  // columns n < nsplit (a multiple of 16) take alpha_lo instead of alpha: the ViT's q|k|v product leaves its q columns
  // multiplied by softmax scale * log2 e, from the fp32 accumulator (what flash_attention_d64(..., q_prescaled = 1) reads)
  int nsplit = 0;
  float alpha_lo = 1.f;
  int flags = 0;
  int tiles_m = 0, tiles_n = 0;  // filled by the launcher
  // split-K (filled by the launcher): K tiles [s * kt_per, (s + 1) * kt_per) go to grid.z slice s, which leaves raw
  // fp32 sums in partial[s][z][m][n] (dense, ld = N); gemm_splitk_reduce_kernel applies the epilogue
  int ksplit = 1, kt_per = 0;
  float* partial = nullptr;
  // transposed side output (gemm_vt_supported() first): columns n >= vt_n0 are NOT written to C but, transposed, to
  // vt[m / vt_rows][n - vt_n0][m % vt_rows] (leading dim vt_ld keys, chunk stride vt_bs) in the flash kernel's key order
  // (perm16 of transpose_bf16) -- the ViT's q|k|v product writes V^T itself.  Rows of a few-rows tail still go to C.
  bf16_t* vt = nullptr;
  int vt_n0 = 0, vt_rows = 0;
  int64_t vt_ld = 0, vt_bs = 0;
  // in-launch tail (filled by the big-tile launcher): rows [M, M + tail_rows) of A / C / R (<= 16: the ViT's cls rows behind the
  // patch rows) are computed inside the same launch by the few-rows arithmetic (rows.h) instead of a launch of their own
  int tail_rows = 0;
  // classic tile kernel (filled by its launcher): 1 = the LDS-DMA pieces leave as buffer_load ... lds (both operands of a batch entry
  // span < 2 GB), 0 = FLAT-encoded global_load_lds (option gemm_mubuf 0, or larger operands)
  int mubuf = 0;
  // big-tile kernels: row tiles per group of the tile walk (pp_tile: ids walk `group_m` row tiles column by column)
  int group_m = 8;
};

// Options (tile, split-K, big-tile selection) and the split-K scratch registration of the launch stream come from the
// calling thread's current Context (ctx.h).  Without a registered scratch, products run unsplit.
int gemm_bf16(GemmDesc d, hipStream_t stream);
bool gemm_vt_supported(const GemmDesc& d, int vt_n0, int vt_rows);  // gemm.hip: may d.vt be set for this product?

// Routing (gemm_plan.hip, host code only): gemm_bf16 = gemm_validate -> gemm_plan -> one launch per step.
enum : int { GK_ROWS16 = 0, GK_TILE = 1, GK_SKINNY = 2, GK_BIG = 3 };
struct GemmStep {  // one kernel instantiation over rows [row0, row0 + rows) of the product
  int kind = GK_TILE;
  int form = 0;  // GK_ROWS16: waves (4 / 8 / 16); GK_TILE: tile (64 / 128); GK_BIG: variant (20 21 22 24 26 27, gemm_plan.hip)
  int row0 = 0, rows = 0;
  bool pair = false, ta = false, tb = false, mubuf = false, gelu = false, vt = false;  // template arguments
  int ksplit = 1, kt_per = 0;  // K slices (> 1: fp32 partial sums in the stream's scratch, then gemm_splitk_reduce_kernel)
  int tail_rows = 0;           // GK_BIG: rows [row0 + rows, + tail_rows) computed in the same launch (rows.h)
  int tiles_m = 0, tiles_n = 0;
  int grid[3] = {1, 1, 1};
};
struct GemmPlan { int nsteps = 0; GemmStep step[2]; };  // main, tail
int gemm_validate(GemmDesc& d);  // U2_ERR_ARG or U2_OK with GEMM_VEC_OK resolved
int gemm_plan(const GemmDesc& d, const Options& o, size_t scratch_bytes, GemmPlan& p);  // d validated; U2_ERR_ARG if no kernel takes it
void gemm_plan_format(const GemmPlan& p, char* buf, size_t n);  // " | <kernel> rows= grid= slices= tail=" per step (the trace)
// the launchers of the steps (descriptor of the step's rows, launcher fields filled)
int gemm_skinny_launch(const GemmDesc& d, const GemmStep& s, hipStream_t stream);  // gemm_skinny.hip
int gemm_bt_launch(const GemmDesc& d, const GemmStep& s, hipStream_t stream);      // gemm_bt.hip

// The form of a weight operand: the element type, e4m3 codes with an fp32 scale per row, e2m1 codes (two per byte, even k in the
// low nibble) with an e8m0 scale byte per block of 32 k.  Decided once at the C boundary (capi.hip), then carried: RowsArgs::form,
// DecodeCfg::form.  What a form asks of a product and of a decode step, and what it reads:
struct WFormFacts {
  int k_mult;        // K (the step's E, Hq D and I) is a multiple of it: the k of one step of the K loop (rows.h)
  int ldw_div;       // a weight row is K / ldw_div units of ldw: bytes with codes, else elements
  int ldw_mult;      // ... and ldw a multiple of it (16-byte aligned rows)
  int scale_align;   // bytes
  double w_bytes;    // per weight (the profiler's byte count)
  int scale_bytes;   // per scale; 0: the form has none
  int scale_k;       // k per scale (lds >= K / scale_k); 0: one per row
};
enum class WForm : int { ELEM = 0, E4M3 = 1, E2M1 = 2 };
constexpr WFormFacts WFORM_FACTS[3] = {{32, 1, 8, 1, 2.0, 0, 0}, {64, 1, 16, 4, 1.0, 4, 0}, {128, 2, 16, 1, 0.5, 1, 32}};
constexpr bool wform_known(WForm f) { return (unsigned)f <= (unsigned)WForm::E2M1; }
constexpr const WFormFacts& wform_facts(WForm f) { return WFORM_FACTS[(int)f]; }

// The few-rows (weight-streaming) product (gemm_rows.hip; arithmetic: rows.h): C = epilogue(A . W^T) for 1 <= M <= 64 rows on
// weights in the element type, C = epilogue(scale[n] * A . e4m3(W)^T) on e4m3 codes, C = epilogue(A . (e2m1(W) 2^(scale - 127))^T)
// on e2m1 codes; 16-byte aligned A / W rows.  Each block of 16 rows has the bits of the M <= 16 product on it.
// The RMSNorm of the finished rows in the tail of the product that wrote them (gemm_rows.hip: the workgroup that draws the last
// ticket norms all M rows of C): Yn = rmsnorm(C) * w over the N columns, bit for bit rmsnorm_bf16's.  Set (w != nullptr) only on
// the non-pair form with a residual and an element-type C, N % 8 == 0, N <= ROWS_NORM_MAX_N; `ticket`: 4 bytes of device memory
// that read 0 before the launch and read 0 again after it.
struct RowsNorm {
  const bf16_t* w = nullptr;     // [N]
  bf16_t* Yn = nullptr;          // [M][N], leading dim ld
  uint32_t* ticket = nullptr;
  int64_t ld = 0;
  float eps = 0.f;
};
constexpr int ROWS_NORM_MAX_N = 4096;  // (the tail holds a row in 8 x 16 bytes per lane: the 64-register instantiations must not spill)
struct RowsEpi {                 // what the epilogue of a lane's 4 columns reads (rows.h: rows_store)
  const bf16_t* bias = nullptr;  // [N] (GEMM_BIAS_N) or [M] (GEMM_BIAS_M)
  int N = 0, flags = 0;
  int nsplit = 0;                // columns n < nsplit take alpha_lo instead of alpha (GemmDesc)
  int64_t ldc = 0, ldr = 0;
  float alpha = 1.f, alpha_lo = 1.f;
  RowsNorm norm;                 // gemm_rows alone (a plan's step leaves it unset)
};
struct RowsArgs : RowsEpi {
  const bf16_t* A = nullptr;     // [M][K] elements, leading dim lda
  const void* W = nullptr;       // [N][K] in `form`, leading dim ldw (WFormFacts)
  const void* scale = nullptr;   // E4M3: [N] fp32; E2M1: [N][K / 32] e8m0 bytes (2^(e - 127)), lds bytes between rows; ELEM: ignored
  void* C = nullptr;             // [M][N] elements or fp32 (GEMM_OUT_F32); [M][N / 2] elements with GEMM_SWIGLU
  const bf16_t* R = nullptr;     // [M][N], leading dim ldr (GEMM_RESIDUAL)
  int M = 0, K = 0;
  int64_t lda = 0, ldw = 0;
  WForm form = WForm::ELEM;      // (the kernels are instantiated per form and do not read it)
  int64_t lds = 0;
};
// gemm_rows: the product outside the plan -- what the decode step calls directly (the plan of an M = 17 .. 64 product is a tile
// kernel's, pinned for the training path): flags GEMM_BIAS_N | GEMM_RESIDUAL | GEMM_OUT_F32 or GEMM_SWIGLU alone, alpha = 1 and no
// column split.  gemm_rows_check: its argument check alone (U2_ERR_ARG, nothing launched).  gemm_rows_launch: the launch alone, for
// a step of the plan (gemm.hip: gemm_step), whose product gemm_validate and rows16_ok have checked and gemm_bf16 brackets.
int gemm_rows_check(const RowsArgs& a);
int gemm_rows(const RowsArgs& a, hipStream_t stream);
int gemm_rows_launch(const RowsArgs& a, hipStream_t stream);

// ------------------------------------------------------------------ row ops (rowops.hip)
// y[b][r][:] = LayerNorm(x[b][r][:] (+ res[b][r][:])) * w + bias   (bf16 in/out, fp32 math)
int layernorm_bf16(const bf16_t* x, const bf16_t* res, const bf16_t* w, const bf16_t* bias, bf16_t* y,
                   int nb, int rows, int C, int64_t x_bs, int64_t x_ld, int64_t res_bs, int64_t res_ld,
                   int64_t y_bs, int64_t y_ld, float eps, hipStream_t stream);

// P[z][r][c] = softmax_c( S[z][r][c] * scale + rel_bias[(c - r) + max_len - 1][z % H] ), bf16 out,
// columns [n, ldp) of P are written as zero.  rel_bias may be null.
int softmax_rows(const float* S, bf16_t* P, int nz, int rows, int n, int64_t lds, int64_t ldp,
                 int64_t s_zs, int64_t p_zs, float scale, const bf16_t* rel_bias, int H, int max_len,
                 hipStream_t stream);

// out[z][c][r] = in[z][r][c]; columns [R, ld_out) of out are zero-filled.  perm16 != 0: inside every group of
// 16 output columns the order is [0-3, 8-11, 4-7, 12-15] (layout the flash-attention kernel expects for V^T).
int transpose_bf16(const bf16_t* in, bf16_t* out, int nz, int R, int C, int64_t ld_in, int64_t ld_out,
                   int64_t in_zs, int64_t out_zs, int perm16, hipStream_t stream);

// ------------------------------------------------------------------ vision (vision.hip)
enum : int { VOL_F16 = 0, VOL_BF16 = 1, VOL_F32 = 2 };
// im2col of reference PatchEmbeddingBlock(perceptron): "b c (h p1) (w p2) (d p3) -> b (h w d) (p1 p2 p3 c)"
// with c == 1.  vol: [nchunk][D][H][W] of vol_dtype; out: [nchunk][nh*nw*nd][p1*p2*p3] bf16.
int im2col_patches(const void* vol, int vol_dtype, bf16_t* out, int nchunk, int D, int H, int W,
                   int p1, int p2, int p3, hipStream_t stream);

// SpatialPoolingProjector pooling: tokens (g1,g2,g3) grid -> avg over ps^3 neighbourhoods.
int avgpool3d_tokens(const bf16_t* x, bf16_t* y, int nb, int g1, int g2, int g3, int w1, int w2, int w3, int C,
                     hipStream_t stream);
// dst[b*dst_bs + e] = src[e] for e < n  (cls token / query token broadcast)
int fill_rows(const bf16_t* src, bf16_t* dst, int nb, int64_t n, int64_t dst_bs, hipStream_t stream);
// in-place rotate-half RoPE on rows indexed (outer, s, inner), position = s, heads = d-wide column slices
int rope_apply(bf16_t* x, int64_t n_outer, int S, int n_inner, int H, int d, int64_t ld, int max_len, int inverse,
               hipStream_t stream);

// out[b][s] = (s == 0 || s > nfeat) ? table[ids[b][s]] : feats[b][s-1]   (embedding lookup + splice)
// feats may be null with nfeat == 0 (plain lookup).
int embed_splice(const bf16_t* table, const int64_t* ids, const bf16_t* feats, bf16_t* out, int B, int S,
                 int E, int nfeat, int64_t vocab, hipStream_t stream);

// ------------------------------------------------------------------ volume preprocessing (preprocess.hip)
// u2Transform.adaptive_resize on the GPU: vol [D][H][W] fp32 (the tensor of u2Transform.py:68-69 without its channel
// axis) -> out [depth_pad][target][target] (== (depth_pad/32, 32, target, target)) in out_dtype (VOL_*).
// info (optional, device, 12 x int32): status, crop box lo[3], hi[3], resized size[3], then a_min, a_max as float.
// aug (may be null): the training-time augmentations of u2Transform.py:37-42 with their random draws made by the caller
struct PreAugment {
  int rot_k = 0;              // RandRotate90(spatial_axes=(1, 2)): quarter turns of the (h, w) plane, torch.rot90 convention
  int flip[3] = {0, 0, 0};    // RandFlip(spatial_axis = 0 / 1 / 2) on the rotated volume
  float mul = 1.f;            // RandScaleIntensity: v * (1 + factor)
  float add = 0.f;            // RandShiftIntensity: v + offset
};
size_t preprocess_workspace_bytes(int D, int H, int W);
int preprocess_volume(const float* vol, void* out, int32_t* info, int D, int H, int W, int target, int depth_pad,
                      float lower_pct, float upper_pct, int out_dtype, const PreAugment* aug, void* ws, size_t ws_bytes,
                      hipStream_t stream);

// ------------------------------------------------------------------ selection / pooling (select.hip)
// scores[b][i] = fp32( sum_e x[b][i][e] * w[e] + bias ), accumulated in fp64.
int score_gemv(const bf16_t* x, const bf16_t* w, const bf16_t* bias, float* scores, int rows, int E,
               hipStream_t stream);
// idx[b][0..k) = indices of the k largest scores[b][0..n), descending, ties -> lower index first.
int topk_sorted(const float* scores, int64_t* idx, int B, int n, int k, hipStream_t stream);
// out[b][i][:] = x[b][idx[b][i]][:]
int gather_rows(const bf16_t* x, const int64_t* idx, bf16_t* out, int B, int n, int k, int E,
                hipStream_t stream);
// Multi-scale pooling {1,2,4} along the token axis (+ optional DMTP gates).  x: [B][k][E];
// out: [B][k + k/2 + k/4][E].  gate_w/gate_b null -> fixed pooling.  ws: >= B*3*16*ceil(E/256) floats.
int multiscale_pool(const bf16_t* x, bf16_t* out, int B, int k, int E, const bf16_t* gate_w,
                    const bf16_t* gate_b, float* ws, hipStream_t stream);

// ------------------------------------------------------------------ backward-pass kernels (backward.hip)
int gelu_fwd(const bf16_t* z, bf16_t* y, int64_t n, hipStream_t stream);                      // y = gelu_fast(z), n % 8 == 0
int gelu_bwd(const bf16_t* z, const bf16_t* dy, bf16_t* dz, int64_t n, hipStream_t stream);  // dz = dy gelu'(z): the derivative of exact erf-GELU
// out[c] (+)= sum_r x[r][c] (* y[r][c] when y != null), fp32, fixed summation order; ws: colsum_workspace_bytes
size_t colsum_workspace_bytes(int rows, int C);
int colsum_bf16(const bf16_t* x, const bf16_t* y, float* out, bf16_t* out_bf16, int rows, int C, int64_t ldx, int64_t ldy,
                float* ws, int accumulate, hipStream_t stream);
// LayerNorm backward of y = LN(x (+ res)) w + b: dv = gradient w.r.t. x (and res), dw / db fp32 [C]
size_t layernorm_bwd_workspace_bytes(int rows, int C);
int layernorm_bwd(const bf16_t* x, const bf16_t* res, const bf16_t* w, const bf16_t* dy, bf16_t* dv, float* dw, float* db,
                  int rows, int C, float eps, float* ws, int accumulate, hipStream_t stream);
// dS = P (dP - rowsum(P dP)); pad columns [n, ldp) zeroed
int softmax_bwd(const bf16_t* P, const float* dP, bf16_t* dS, int64_t nrows, int n, int64_t ldp, int64_t lddp,
                hipStream_t stream);
// dtable[d + max_len - 1][h] += sum over z % H == h and the diagonal j - i = d of dS[z][i][j]   (dS: [nz][S][ldp])
int relbias_grad(const bf16_t* dS, float* dtable, int nz, int S, int H, int64_t ldp, int max_len, hipStream_t stream);
int rowdot_bf16(const bf16_t* a, const bf16_t* b, float* out, int64_t rows, int C, int64_t lda, int64_t ldb,
                hipStream_t stream);
// loss head (loss.hip): online log-sum-exp over one vocabulary slice of the logits, and the cross-entropy gradient written over them
int ce_lse_update(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l, float* zt,
                  hipStream_t stream);
// the same pass with further per-row statistics: (amax, aidx) both or neither, zsum, l2 each or nullptr
int ce_stats_update(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l, float* zt,
                    float* amax, int64_t* aidx, float* zsum, float* l2, hipStream_t stream);
int ce_grad_inplace(bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, const float* lse, const float* coef,
                    hipStream_t stream);
// sampling warper (sample.hip): temperature / top-k / top-p filtering of fp32 logits, one launch, no sort
size_t sample_warp_workspace_bytes(int rows, int V);
// The split-row form (sample.hip): sample_warp's contract and bits of `out`, a row over min(16, ceil(V / SAMPLE_SPLIT_SLICE)) workgroups,
// one launch per pass of the descent (sample_warp_split_launches of them, fixed by the parameters alone)
constexpr int SAMPLE_SPLIT_SLICE = 8192;
size_t sample_warp_split_workspace_bytes(int rows, int V);
int sample_warp_split_launches(int V, int top_k, float top_p, int min_keep);
int sample_warp_split(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int rows, int V, float temperature, int top_k,
                      float top_p, int min_keep, void* ws, size_t ws_bytes, hipStream_t st);
int sample_warp(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int rows, int V, float temperature, int top_k,
                float top_p, int min_keep, void* ws, size_t ws_bytes, hipStream_t stream);
// sharded AdamW step (dp.py): see backward.hip
struct AdamWArgs {
  float lr[8], wd[8];  // per parameter group
  float b1, b2, eps, inv_c1, inv_sqrt_c2, gscale;
  const float* gcoef;  // optional device scalar multiplied into the gradient (clipping coefficient)
};
int adamw_step(float* master, float* m, float* v, const bf16_t* grad, const uint8_t* group, bf16_t* out, int64_t n,
               const AdamWArgs& a, hipStream_t stream);

// ------------------------------------------------------------------ attention (attn.hip)
// Temporal attention of SpatioTemporalAttentionLayer: sequences of length T <= 16 that run ACROSS
// chunks.  q/k/v/out rows are laid out [b][t][n] (leading dim ld), heads are column slices of width d.
int temporal_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int T, int N,
                       int H, int d, int64_t ld_qkv, int64_t ld_out, float scale, const bf16_t* rel_bias,
                       int max_len, hipStream_t stream);

// Flash attention for the ViT blocks (head_dim 64) over S main rows per batch plus n_extra (0 / 1) extra row per
// batch stored elsewhere (the cls token).  q,k: row r of batch b at q + b*q_bs + r*ld_qk, head h at column h*64;
// vt: V^T of the main rows, [nb][H][64][S_pad] (S_pad % 64 == 0, zero padded, perm16 column order); out like q with
// ld_out / out_bs.  Extra row of batch b: qx / kx / vx + b*x_bs, output outx + b*ox_bs (head h at column h*64).
int flash_attention_d64(const bf16_t* q, const bf16_t* k, const bf16_t* vt, bf16_t* out, int nb, int S, int H,
                        int64_t ld_qk, int64_t q_bs, int64_t ld_out, int64_t out_bs, int S_pad, float scale,
                        const bf16_t* qx, const bf16_t* kx, const bf16_t* vx, bf16_t* outx, int64_t x_bs, int64_t ox_bs,
                        int n_extra, float* lse, int64_t lse_ld, hipStream_t stream,  // lse: optional row statistics out
                        int q_prescaled = 0);  // 1: q and qx already carry scale * log2 e (S >= 512: the double pipeline)
// Backward of the same attention: dq / dk / dv of out = softmax(q k^T scale) v for head dim 64, all S rows of a batch in ONE
// row-major view (q, k, v: row r of batch b at + b*bs_qkv + r*ld_qkv, head h at column h*64; o / dout with ld_o / bs_o;
// dq / dk / dv with ld_d / bs_d).  lse: optional row statistics of the forward kernel.  Workspace: the row statistics (lse, D).
// The non-causal, equal-heads instantiation of the one flash backward pair of attn_bwd.hip (bwd_dq_kernel, bwd_dkv_kernel);
// attention_gqa_bwd below is its causal, grouped-query one.  Each entry point keeps its own argument checks.
size_t flash_attention_d64_bwd_workspace_bytes(int nb, int S, int H);
int flash_attention_d64_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                            const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                            int64_t bs_d, int nb, int S, int H, float scale, const float* lse, int64_t lse_ld,
                            void* workspace, size_t workspace_bytes, hipStream_t stream);
// Fused attention forward (tokattn.hip): out = softmax(q k^T scale + bias / masks) v per (batch, head); row r of batch b at
// + b*?_bs + r*ld?, query head h at column h*d of q / out, kv head h / (H / Hkv) of k / v.  One descriptor for every caller: the
// tokenizer's attention modules (rma.py:60-75, tta.py:55-61, rope.py:82-86), the decoder's prefill, decode, training and continued
// prefill routes.  The optional fields' defaults are the plain call; what is set picks the kernel form:
//   plain  d in {64, 96, 128, 256, 384, 512}; rel_bias (not causal) and key splits (not causal) only here
//   range  kv_start / kv_len / lse set: d in {64, 96, 128, 256, 512}
//   band   k_hs / v_hs != d or a window: d in {64, 96, 128}
struct AttnCall {
  const bf16_t *q = nullptr, *k = nullptr, *v = nullptr;
  bf16_t* out = nullptr;
  int nb = 0, Sq = 0, Skv = 0, H = 0, Hkv = 0, d = 0;  // Hkv = H: plain multi-head
  int64_t ldq = 0, ldk = 0, ldv = 0, ldo = 0, q_bs = 0, k_bs = 0, v_bs = 0, o_bs = 0;
  float scale = 1.f;
  const bf16_t* rel_bias = nullptr;  // + rel_bias[j - i + max_len - 1][h]
  int max_len = 0;
  int causal = 0;  // key j visible to query i iff j <= i + Skv - Sq
  // Few (batch, head, 64-query) units -> the key range is cut into splits whose fp32 partial results go through `ws`
  // (tok_attention_workspace_bytes, 16-byte aligned; null: unsplit).  force_splits > 0 overrides the heuristic (tests).
  int force_splits = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // key j of sequence b visible iff kv_start[b] <= j < kv_len[b] (device int (nb) each; null: 0 / Skv); a row that sees no key gets
  // zeros.  lse: row statistics for attention_gqa_bwd, (nb * H, lse_ld) fp32 in log2 units.
  const int *kv_start = nullptr, *kv_len = nullptr;
  float* lse = nullptr;
  int64_t lse_ld = 0;
  int64_t k_hs = 0, v_hs = 0;  // elements between the kv heads of a sequence (0: d, column-packed; capacity * d: a KV cache's (B, Hkv, capacity, d))
  int window = 0;              // W > 0 (causal): ... and only if j > i + Skv - Sq - W
};
int attention(const AttnCall& c, hipStream_t stream);
int attention_check(const AttnCall& c);  // every refusal of attention(c, .), nothing launched
// tok_attention_supported: the plain form takes these shapes / strides (pipeline.hip falls back to the GEMM chain otherwise)
bool tok_attention_supported(const AttnCall& c);
size_t tok_attention_workspace_bytes(int nb, int H, int Sq, int Skv, int d);
// The decoder training route (u2tokenizer_amd/decoder_train.py).  attention_gqa_bwd (attn_bwd.hip, the causal instantiations
// of the pair behind flash_attention_d64_bwd): the flash backward of attention()'s causal GQA call with kv_len and lse, d = 64 / 128,
// Sq = Skv = S, layout of flash_attention_d64_bwd with Hq query and Hkv kv heads.  rmsnorm_bwd,
// qk_norm_rope_bwd, swiglu_bwd (backward.hip): the row operations' backward.
size_t attention_gqa_bwd_workspace_bytes(int nb, int S, int Hq);
int attention_gqa_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                      const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                      int64_t bs_d, int nb, int S, int Hq, int Hkv, int d, float scale, const int* kv_len, const float* lse_in,
                      int64_t lse_ld, void* workspace, size_t workspace_bytes, hipStream_t stream);
// (head dim 96, Phi-3: the <96, true> instantiations through the same launcher and workspace; attention_gqa_bwd refuses 96)
int attention_gqa_bwd_d96(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                          const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                          int64_t bs_d, int nb, int S, int Hq, int Hkv, float scale, const int* kv_len, const float* lse_in,
                          int64_t lse_ld, void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t rmsnorm_bwd_workspace_bytes(int rows, int C);
int rmsnorm_bwd(const bf16_t* x, const bf16_t* w, const bf16_t* dy, const bf16_t* dres, bf16_t* dx, float* dw, int rows, int C,
                float eps, float* ws, size_t ws_bytes, int accumulate, hipStream_t st);
size_t qk_norm_rope_bwd_workspace_bytes(int64_t rows, int D);
int qk_norm_rope_bwd(bf16_t* dqkv, const bf16_t* pre, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp,
                     int cs_is_f32, int64_t rows, int Hq, int Hkv, int D, int64_t ld, int64_t ld_pre, int64_t cs_ld, float eps,
                     float* dwq, float* dwk, float* ws, size_t ws_bytes, int accumulate, hipStream_t st);
int swiglu_bwd(const bf16_t* gu, const bf16_t* dact, bf16_t* dgu, int64_t rows, int I, int64_t ld_gu, int64_t ld_da,
               int64_t ld_dgu, hipStream_t st);
// ------------------------------------------------------------------ decoder prefill row kernels (decoder.hip)
int rmsnorm_bf16(const bf16_t* x, const bf16_t* w, bf16_t* y, int64_t rows, int C, int64_t ldx, int64_t ldy, float eps,
                 hipStream_t stream);
int qk_norm_rope(bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int cs_is_f32,
                 int64_t rows, int Hq, int Hkv, int D, int64_t ld, int64_t cs_ld, float eps, bf16_t* kc, bf16_t* vc, int S,
                 int64_t kv_stride, int s_off, hipStream_t stream);
// (qk_norm_rope on an e4m3 cache: the finished k heads and the v heads as codes and scales at positions s_off .. s_off + S - 1 of
//  the dense buffers -- the bits of qk_norm_rope into 16-bit rows followed by kv_quantize_rows, in one launch)
int qk_norm_rope_kv8(bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int cs_is_f32, int64_t rows, int Hq,
                     int Hkv, int D, int64_t ld, int64_t cs_ld, float eps, uint8_t* kcd, uint8_t* vcd, float* ksc, float* vsc, int S,
                     int capacity, int s_off, hipStream_t stream);
int swiglu_bf16(const bf16_t* gu, bf16_t* out, int64_t rows, int I, int64_t ld_in, int64_t ld_out, hipStream_t stream);
int swiglu_check(const bf16_t* gu, const bf16_t* out, int64_t rows, int I, int64_t ld_in, int64_t ld_out);  // its refusals alone
struct DecodeCfg {  // one decode step of a decoder layer (decoder.hip)
  int B, E, Hq, Hkv, D, I;
  float eps, qk_eps, scale;
  WForm form = WForm::ELEM;  // of the layer's four W*
};
// One segment of a few-rows adapter group (lora_rows.hip; the layout of u2tok_lora_seg): A (r, K) and B (N, r) contiguous, the
// segment's columns [col0, col0 + N) of the product it is added to
struct LoraSeg {
  const bf16_t *A, *B;
  int r, col0, N;
  float scale;
};
size_t lora_rows_workspace_bytes(int M, int K, const LoraSeg* segs, int n);
// check_only: every refusal of the call (U2_ERR_ARG / U2_ERR_WORKSPACE), nothing launched
int lora_rows(const bf16_t* X, int64_t ldx, const LoraSeg* segs, int n, bf16_t* U, int64_t ldu, bf16_t* Y, int64_t ldy, int M, int K,
              void* ws, size_t ws_bytes, bool check_only, hipStream_t st);
// The unmerged adapters of a layer's decode step (the layout of u2tok_decode_lora): the segment lists of the four products (n_* = 0:
// none) and the branch's own scratch -- DECODE_LORA_U_BYTES for u (64 rows x 192 columns), then the group products' workspace
struct DecodeLora {
  LoraSeg qkv[3], o[1], gu[2], down[1];
  int n_qkv, n_o, n_gu, n_down;
  void* scratch;
  size_t scratch_bytes;
};
constexpr size_t DECODE_LORA_U_LD = 192, DECODE_LORA_U_BYTES = 64 * DECODE_LORA_U_LD * sizeof(bf16_t);
// A layer's decode-step parameters, in the form DecodeCfg::form names (capi.hip decodes u2tok_decode_layer into it).  ELEM: the four
// W* are in the element type and the scales are not read.  E4M3: codes with an fp32 scale per weight row.  E2M1: codes with an
// e8m0 scale byte per block of 32 (gemm_rows.hip).  The quantised forms ask E, Hq * D and I multiples of 64 / 128, 16-byte aligned
// weights and all four scales, aligned to their type (WFormFacts): U2_ERR_ARG otherwise, like every other refusal before anything
// is launched.
struct DecodeLayer {
  const void *Wqkv, *Wo, *Wgu, *Wdown;
  const bf16_t *w_in_norm, *bqkv, *wq_norm, *wk_norm;  // first half
  const bf16_t *bo, *w_post_norm, *bgu, *bdown;        // second half
  const void *scale_qkv, *scale_o, *scale_gu, *scale_down;
  const DecodeLora* lora = nullptr;                    // unmerged adapters (NULL: none)
};
size_t decoder_decode_workspace_bytes(const DecodeCfg& c, int T);
int decoder_decode_pre(const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32,
                       int64_t cs_ld, bf16_t* qkv, bf16_t* kc, bf16_t* vc, int64_t kv_stride, int s_off, void* ws, size_t ws_bytes,
                       hipStream_t st);
// batched: the batched decode attention (decode_attn.hip) in place of the per-sequence loop, with kv_start the optional (B) first
// visible cache position per sequence (a left-padded batch); kv_start without batched: U2_ERR_ARG
int decoder_decode_post(const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const bf16_t* qkv, const bf16_t* K, const bf16_t* V,
                        int T, int64_t kv_stride, bool batched, const int* kv_start, bf16_t* out, void* ws, size_t ws_bytes,
                        hipStream_t st);
// One layer of the whole-stack step (capi.hip decodes u2tok_decode_stack_layer into it): the layer's two halves on its
// append-in-place cache buffers kc / vc (B, Hkv, capacity, D; kv_stride = capacity * D).  The step's k / v rows go to position
// s_off, the attention reads positions k_first .. k_first + T - 1 <= s_off.
// kv8 (capi.hip decodes u2tok_decode_stack_layer_kv8 into it): the layer's cache is e4m3 -- the dense code buffers Kc / Vc (B, Hkv,
// capacity, D) bytes and scales Ks / Vs (B, Hkv, capacity) of DecodeKv8 below; the step's rows go to position s_off as codes in the
// first half's rotary launch (qk_norm_rope_kv8), the attention -- batched only -- reads the codes of positions k_first .. s_off, so
// T = s_off - k_first + 1 and s_off < capacity; kc / vc / kv_stride are not read.
struct DecodeStackLayer {
  DecodeCfg cfg;
  DecodeLayer layer;
  bf16_t *kc = nullptr, *vc = nullptr;
  int64_t kv_stride = 0;
  int s_off, k_first, T;
  bool kv8 = false;
  uint8_t *Kc = nullptr, *Vc = nullptr;
  float *Ks = nullptr, *Vs = nullptr;
  int capacity = 0;
};
// Every layer's pre and post in one call, the hidden state through the workspace, the final RMSNorm (w_final: null = the last hidden
// state as it is) into out; every refusal of every layer before the first launch.  tail_norm: gemm_rows' RowsNorm for the norms
// behind the o and down products.  The first 4 bytes of the (256-byte aligned) workspace are the ticket: zero before the call.
size_t decoder_decode_stack_workspace_bytes(const DecodeStackLayer* L, int n);
int decoder_decode_stack(const DecodeStackLayer* L, int n, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32, int64_t cs_ld,
                         bool batched, const int* kv_start, const bf16_t* w_final, float final_eps, bool tail_norm, bf16_t* out, void* ws,
                         size_t ws_bytes, hipStream_t st);
// The head of a decode step (capi.hip decodes u2tok_decode_head_desc into it): the stack's final RMSNorm (w_norm (E), eps), then the
// output matrix W (V, E) in `form` -- ldw elements (ELEM) or bytes (codes) between rows; scale: [V] fp32 (E4M3) or [V][E / 32] e8m0
// bytes with lds bytes between rows (E2M1).
struct DecodeHead {
  const bf16_t* w_norm = nullptr;
  const void *W = nullptr, *scale = nullptr;
  WForm form = WForm::ELEM;
  int E = 0, V = 0;
  float eps = 0.f;
  int64_t ldw = 0, lds = 0;
};
// logits (B <= 64, V; fp32, ldl) = gemm_rows(GEMM_OUT_F32) of rmsnorm_bf16 of x (B, E; ldx), bit for bit; the normed rows live in
// the workspace (16-byte aligned).  decoder_decode_stack_head: decoder_decode_stack with w_final = null into out, then the head on
// out, in one call whose every refusal -- the layers' and the head's -- precedes its first launch; workspace: the stack step's, then
// the head's.
size_t decode_head_workspace_bytes(int B, int E);
int decode_head(const DecodeHead& h, const bf16_t* x, int64_t ldx, int B, float* logits, int64_t ldl, void* ws, size_t ws_bytes,
                hipStream_t st);
size_t decoder_decode_stack_head_workspace_bytes(const DecodeStackLayer* L, int n, const DecodeHead& h);
int decoder_decode_stack_head(const DecodeStackLayer* L, int n, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32,
                              int64_t cs_ld, bool batched, const int* kv_start, bool tail_norm, bf16_t* out, const DecodeHead& h,
                              float* logits, int64_t ldl, void* ws, size_t ws_bytes, hipStream_t st);
// ------------------------------------------------------------------ batched decode attention (decode_attn.hip)
// One query row per sequence over its KV cache, all B sequences and heads in one launch (+ one merge of the key splits):
// q / out (B, Hq * D) rows with ldq / ldo elements between sequences, K / V (B, Hkv, T, D) with kv_stride elements between
// (batch, kv head) entries; key j of sequence b is visible iff j >= kv_start[b] (NULL: all).  check_only: every refusal of the
// call, nothing launched.
size_t decode_attention_workspace_bytes(int B, int Hq, int Hkv, int T, int D);
int decode_attention(const bf16_t* q, const bf16_t* K, const bf16_t* V, bf16_t* out, int B, int Hq, int Hkv, int T, int D,
                     int64_t ldq, int64_t kv_stride, int64_t ldo, float scale, const int* kv_start, void* ws, size_t ws_bytes,
                     bool check_only, hipStream_t stream);
// ---- the FP8 (e4m3) KV cache (decode_attn.hip): codes (B, Hkv, capacity, D) bytes and ONE fp32 scale per cache row, (B, Hkv,
// capacity); value = code x scale.  kv_quantize_rows: the 16-bit rows k / v (B, Hkv, n, D; *_bs / *_hs / *_rs elements between
// sequences / heads / positions, multiples of 8) as codes and scales at positions s_off .. s_off + n - 1 of dense buffers, one
// launch for both.  decode_attention_kv8: decode_attention over codes -- kv_stride BYTES and sc_stride floats between (batch, kv
// head) entries (0: dense, T D and T).  check_only: every refusal of the call, nothing launched.
int kv_quantize_rows(const bf16_t* k, const bf16_t* v, int B, int Hkv, int n, int D, int64_t k_bs, int64_t k_hs, int64_t k_rs, int64_t v_bs,
                     int64_t v_hs, int64_t v_rs, uint8_t* kc, uint8_t* vc, float* ksc, float* vsc, int capacity, int s_off, bool check_only,
                     hipStream_t stream);
size_t decode_attention_kv8_workspace_bytes(int B, int Hq, int Hkv, int T, int D);
int decode_attention_kv8(const bf16_t* q, const uint8_t* Kc, const uint8_t* Vc, const float* Ks, const float* Vs, bf16_t* out, int B, int Hq,
                         int Hkv, int T, int D, int64_t ldq, int64_t kv_stride, int64_t sc_stride, int64_t ldo, float scale,
                         const int* kv_start, void* ws, size_t ws_bytes, bool check_only, hipStream_t stream);
// attention_kv8_rows: Sq >= 1 new positions per sequence over the codes -- q / out are B Sq rows (row b Sq + i, ldq / ldo elements
// apart), T counts the positions read (the new ones last); row i sees key j iff kv_start[b] <= j <= i + T - Sq and, window W > 0,
// j > i + T - Sq - W.  Sq = 1, window = 0: the bits of decode_attention_kv8.
size_t attention_kv8_rows_workspace_bytes(int B, int Sq, int Hq, int Hkv, int T, int D);
int attention_kv8_rows(const bf16_t* q, const uint8_t* Kc, const uint8_t* Vc, const float* Ks, const float* Vs, bf16_t* out, int B, int Sq,
                       int Hq, int Hkv, int T, int D, int64_t ldq, int64_t kv_stride, int64_t sc_stride, int64_t ldo, float scale, int window,
                       const int* kv_start, void* ws, size_t ws_bytes, bool check_only, hipStream_t stream);
// The second half of a layer's decode step on such a cache: the step's new 16-bit rows k_new / v_new (B, Hkv, 1, D; dense: what
// decoder_decode_pre wrote) are quantised into position s_off of the dense buffers (capacity positions per (batch, kv head)
// entry), the attention -- always the batched kernel -- reads positions k_first .. s_off, kv_start counted from k_first.
// (Inside the whole-stack step k_new / v_new are null: the rows are in the buffers already and nothing is quantised.)
struct DecodeKv8 {
  const bf16_t *k_new, *v_new;
  uint8_t *Kc, *Vc;
  float *Ks, *Vs;
  int capacity, k_first, s_off;
};
int decoder_decode_post_kv8(const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const bf16_t* qkv, const DecodeKv8& kv,
                            const int* kv_start, bf16_t* out, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace u2
