// extern "C" surface of libu2tok_hip.so (declared in include/u2tok.h).  Thin: argument marshalling only.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "pipeline.h"

using namespace u2;

static_assert(U2TOK_OK == U2_OK && U2TOK_ERR_ARG == U2_ERR_ARG && U2TOK_ERR_LAUNCH == U2_ERR_LAUNCH &&
                  U2TOK_ERR_WORKSPACE == U2_ERR_WORKSPACE && U2TOK_ERR_DEVICE == U2_ERR_DEVICE,
              "public and internal status codes must agree");

#define BF(p) reinterpret_cast<const bf16_t*>(p)
#define BFW(p) reinterpret_cast<bf16_t*>(p)
#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

int u2tok_version(void) { return 200; /* 0.2.0 */ }
const char* u2tok_arch(void) { return "gfx950"; }
const char* u2tok_elem(void) { return U2_ELEM_ASM; }

int u2tok_device_check(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return U2_ERR_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return U2_ERR_DEVICE;
  return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? U2_OK : U2_ERR_DEVICE;
}

// ---- contexts (ctx.h)
int u2tok_ctx_create(u2tok_ctx_t* out) {
  if (!out) return U2_ERR_ARG;
  *out = reinterpret_cast<u2tok_ctx_t>(new (std::nothrow) Context());
  return *out ? U2_OK : U2_ERR_ARG;
}
int u2tok_ctx_destroy(u2tok_ctx_t c) {
  if (!c) return U2_ERR_ARG;
  Context* cx = reinterpret_cast<Context*>(c);
  if (ctx_bound() == cx) ctx_bind(nullptr);
  delete cx;
  return U2_OK;
}
int u2tok_ctx_set_current(u2tok_ctx_t c) {
  ctx_bind(reinterpret_cast<Context*>(c));
  return U2_OK;
}
u2tok_ctx_t u2tok_ctx_get_current(void) { return reinterpret_cast<u2tok_ctx_t>(ctx_bound()); }

int u2tok_set_option(const char* name, int value) {
  if (!name) return U2_ERR_ARG;
  Options& o = ctx().opt;
  struct Opt { const char* name; int Options::*field; int lo, hi; };
  static const Opt table[] = {
      {"gemm_splitk", &Options::gemm_splitk, -1, 16},   {"gemm_mubuf", &Options::gemm_mubuf, 0, 1}, {"ln_wide", &Options::ln_wide, 0, 1},   {"gemm_big", &Options::gemm_big, -1, 27},
      {"gemm_big_grid", &Options::gemm_big_grid, 1, 4096}, {"gemm_big_splitk", &Options::gemm_big_splitk, 0, 16},
      {"gemm_big_drain", &Options::gemm_big_drain, 0, 1}, {"gemm_skinny", &Options::gemm_skinny, 0, 2},
       {"kmajor_b", &Options::kmajor_b, 0, 1},            {"gemm_tail_fused", &Options::gemm_tail_fused, 0, 1},
      {"flash_mode", &Options::flash_mode, 0, 7},        {"flash_q_prescaled", &Options::flash_q_prescaled, 0, 1},
      {"vit_flash", &Options::vit_flash, 0, 1},         {"tta_overlap", &Options::tta_overlap, 0, 1},
      {"vit_vt_epilogue", &Options::vit_vt_epilogue, 0, 1},
      {"tok_flash", &Options::tok_flash, 0, 1},
      {"tok_wide", &Options::tok_wide, 0, 2},
      {"svr_fold", &Options::svr_fold, 0, 1},
  };
  if (!strcmp(name, "gemm_tile")) {
    if (value != 0 && value != 64 && value != 128) return U2_ERR_ARG;
    o.gemm_tile = value;
    return U2_OK;
  }
  if (!strcmp(name, "profile")) { prof_enable(value != 0); return U2_OK; }
  for (const Opt& t : table)
    if (!strcmp(name, t.name)) {
      if (value < t.lo || value > t.hi) return U2_ERR_ARG;
      if (t.field == &Options::gemm_big && value > 0 && !(value >= 20 && value <= 27 && value != 23 && value != 25)) return U2_ERR_ARG;
      if (t.field == &Options::flash_mode && value != 0 && value != 1 && value != 7) return U2_ERR_ARG;
      o.*(t.field) = value;
      return U2_OK;
    }
  return U2_ERR_ARG;
}

int u2tok_set_gemm_scratch(void* device_ptr, size_t bytes, void* stream) {
  ctx().set_scratch(reinterpret_cast<hipStream_t>(stream), device_ptr, device_ptr ? bytes : 0);
  return U2_OK;
}

int u2tok_profile_collect(double* ms, double* flops, int64_t* count, int32_t ncat) {
  if (!ms || !flops || !count || ncat <= 0 || ncat > PROF_NCAT) return U2_ERR_ARG;
  return prof_collect(ms, flops, nullptr, count, ncat);
}
int u2tok_profile_collect2(double* ms, double* flops, double* bytes, int64_t* count, int32_t ncat) {
  if (!ms || !flops || !bytes || !count || ncat <= 0 || ncat > PROF_NCAT) return U2_ERR_ARG;
  return prof_collect(ms, flops, bytes, count, ncat);
}

size_t u2tok_vit_workspace_bytes(const u2tok_vit_config* cfg) {
  if (!cfg) return 0;
  size_t peak = 0;
  if (vit_forward(*cfg, nullptr, nullptr, nullptr, nullptr, 0, true, &peak, nullptr) != U2_OK) return 0;
  return peak + 256;
}
int u2tok_vit_forward(const u2tok_vit_config* cfg, const void* const* weights, const void* volume, void* out,
                      void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  if (!cfg || !workspace || ((uintptr_t)workspace & 255)) return U2_ERR_ARG;
  return vit_forward(*cfg, weights, volume, BFW(out), workspace, workspace_bytes, false, nullptr, ST(stream));
}

size_t u2tok_spp_workspace_bytes(const u2tok_spp_config* cfg) {
  if (!cfg) return 0;
  size_t peak = 0;
  if (spp_forward(*cfg, nullptr, nullptr, nullptr, nullptr, 0, true, &peak, nullptr) != U2_OK) return 0;
  return peak + 256;
}
int u2tok_spp_forward(const u2tok_spp_config* cfg, const void* const* weights, const void* x, void* out,
                      void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  if (!cfg || !workspace || ((uintptr_t)workspace & 255)) return U2_ERR_ARG;
  return spp_forward(*cfg, weights, BF(x), BFW(out), workspace, workspace_bytes, false, nullptr, ST(stream));
}

size_t u2tok_tokenizer_workspace_bytes(const u2tok_tokenizer_config* cfg) {
  if (!cfg) return 0;
  size_t peak = 0;
  if (tokenizer_forward(*cfg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, true, &peak,
                        nullptr) != U2_OK)
    return 0;
  return peak + 256;
}
int u2tok_tokenizer_forward(const u2tok_tokenizer_config* cfg, const void* const* weights, const void* v_token,
                            const void* t_token, void* out, int64_t* topk_idx_out, void* svr_out, void* workspace,
                            size_t workspace_bytes, u2tok_stream_t stream) {
  if (!cfg || !workspace || ((uintptr_t)workspace & 255)) return U2_ERR_ARG;
  return tokenizer_forward(*cfg, weights, BF(v_token), BF(t_token), BFW(out), topk_idx_out, BFW(svr_out), nullptr, workspace,
                           workspace_bytes, false, nullptr, ST(stream));
}
int u2tok_tokenizer_forward_taps(const u2tok_tokenizer_config* cfg, const void* const* weights, const void* v_token,
                                 const void* t_token, void* out, int64_t* topk_idx_out, const u2tok_tokenizer_taps* taps,
                                 void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  if (!cfg || !taps || !workspace || ((uintptr_t)workspace & 255)) return U2_ERR_ARG;
  return tokenizer_forward(*cfg, weights, BF(v_token), BF(t_token), BFW(out), topk_idx_out, nullptr, taps, workspace,
                           workspace_bytes, false, nullptr, ST(stream));
}

int u2tok_tokenizer_svr_fold(const void* w_qkv, const void* b_qkv, const void* w_o, const void* b_o, void* w_fold, void* b_fold,
                             int32_t E, u2tok_stream_t stream) {
  return svr_fold_build(BF(w_qkv), BF(b_qkv), BF(w_o), BF(b_o), BFW(w_fold), BFW(b_fold), E, ST(stream));
}

size_t u2tok_preprocess_workspace_bytes(int32_t D, int32_t H, int32_t W) { return preprocess_workspace_bytes(D, H, W); }
int u2tok_preprocess_volume(const float* vol, void* out, int32_t* info, int32_t D, int32_t H, int32_t W, int32_t target,
                            int32_t depth_pad, float lower_pct, float upper_pct, int32_t out_dtype, void* workspace,
                            size_t workspace_bytes, u2tok_stream_t stream) {
  return preprocess_volume(vol, out, info, D, H, W, target, depth_pad, lower_pct, upper_pct, out_dtype, nullptr, workspace,
                           workspace_bytes, ST(stream));
}
int u2tok_preprocess_volume_aug(const float* vol, void* out, int32_t* info, int32_t D, int32_t H, int32_t W, int32_t target,
                                int32_t depth_pad, float lower_pct, float upper_pct, int32_t out_dtype,
                                const u2tok_augment* aug, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  if (!aug) return U2_ERR_ARG;
  PreAugment a;
  a.rot_k = aug->rot90_k;
  for (int i = 0; i < 3; ++i) a.flip[i] = aug->flip[i];
  a.mul = 1.0f + aug->scale_factor;
  a.add = aug->shift_offset;
  return preprocess_volume(vol, out, info, D, H, W, target, depth_pad, lower_pct, upper_pct, out_dtype, &a, workspace,
                           workspace_bytes, ST(stream));
}

int u2tok_embed_splice(const void* table, const int64_t* ids, const void* feats, void* out, int32_t B, int32_t S,
                       int32_t E, int32_t nfeat, int64_t vocab, u2tok_stream_t stream) {
  return embed_splice(BF(table), ids, BF(feats), BFW(out), B, S, E, nfeat, vocab, ST(stream));
}

int u2tok_gemm_bf16(const void* A, const void* B, void* C, const void* bias, const void* R, int32_t M, int32_t N,
                    int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int32_t nz, int32_t nbh,
                    int64_t sAb, int64_t sAh, int64_t sBb, int64_t sBh, int64_t sCb, int64_t sCh, int64_t sRb,
                    int64_t sRh, float alpha, int32_t flags, u2tok_stream_t stream) {
  GemmDesc g;
  g.A = BF(A); g.B = BF(B); g.C = C; g.bias = BF(bias); g.R = BF(R);
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldr = ldr;
  g.nz = nz; g.nbh = nbh;
  g.sAb = sAb; g.sAh = sAh; g.sBb = sBb; g.sBh = sBh; g.sCb = sCb; g.sCh = sCh; g.sRb = sRb; g.sRh = sRh;
  g.alpha = alpha;
  g.flags = flags & (GEMM_BIAS_N | GEMM_BIAS_M | GEMM_GELU | GEMM_RESIDUAL | GEMM_OUT_F32 | GEMM_A_KMAJOR | GEMM_B_KMAJOR |
                     GEMM_SWIGLU);
  if (flags & GEMM_B_KTILE) {
    if ((K & 63) || nz != 1) return U2_ERR_ARG;
    g.ldb = 64;
    g.ldbk = (int64_t)N * 64;
  }
  return gemm_bf16(g, ST(stream));
}

// u2tok_gemm_bf16 with the descriptor fields the ViT's q|k|v product sets (pipeline.hip: vit_block): the column split and the
// transposed side output.  Neutral values (nsplit 0, alpha_lo 1, vt NULL) leave the descriptor u2tok_gemm_bf16 builds.
int u2tok_gemm_bf16_ex(const void* A, const void* B, void* C, const void* bias, const void* R, int32_t M, int32_t N,
                       int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldr, int32_t nz, int32_t nbh,
                       int64_t sAb, int64_t sAh, int64_t sBb, int64_t sBh, int64_t sCb, int64_t sCh, int64_t sRb,
                       int64_t sRh, float alpha, int32_t flags, int32_t nsplit, float alpha_lo, void* vt, int32_t vt_n0,
                       int32_t vt_rows, int64_t vt_ld, int64_t vt_bs, u2tok_stream_t stream) {
  GemmDesc g;
  g.A = BF(A); g.B = BF(B); g.C = C; g.bias = BF(bias); g.R = BF(R);
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldr = ldr;
  g.nz = nz; g.nbh = nbh;
  g.sAb = sAb; g.sAh = sAh; g.sBb = sBb; g.sBh = sBh; g.sCb = sCb; g.sCh = sCh; g.sRb = sRb; g.sRh = sRh;
  g.alpha = alpha;
  g.flags = flags & (GEMM_BIAS_N | GEMM_BIAS_M | GEMM_GELU | GEMM_RESIDUAL | GEMM_OUT_F32 | GEMM_A_KMAJOR | GEMM_B_KMAJOR |
                     GEMM_SWIGLU);
  if (flags & GEMM_B_KTILE) {
    if ((K & 63) || nz != 1) return U2_ERR_ARG;
    g.ldb = 64;
    g.ldbk = (int64_t)N * 64;
  }
  g.nsplit = nsplit; g.alpha_lo = alpha_lo;
  if (vt) {
    // 16-byte stores of 8 keys; every chunk of vt_rows keys holds N - vt_n0 rows of vt_ld keys inside its vt_bs elements
    if (vt_n0 <= 0 || vt_n0 >= N || vt_rows <= 0 || ((uintptr_t)vt & 15) || (vt_ld & 7) || (vt_bs & 7) || vt_ld < vt_rows ||
        vt_bs < (int64_t)(N - vt_n0) * vt_ld || !gemm_vt_supported(g, vt_n0, vt_rows))
      return U2_ERR_ARG;
    g.vt = BFW(vt); g.vt_n0 = vt_n0; g.vt_rows = vt_rows; g.vt_ld = vt_ld; g.vt_bs = vt_bs;
  }
  return gemm_bf16(g, ST(stream));
}

int u2tok_layernorm_bf16(const void* x, const void* res, const void* w, const void* b, void* y, int32_t rows,
                         int32_t C, float eps, u2tok_stream_t stream) {
  return layernorm_dense(BF(x), BF(res), BF(w), BF(b), BFW(y), rows, C, eps, ST(stream));
}

int u2tok_layernorm_rows(const void* x, const void* res, const void* w, const void* b, void* y, int32_t nb, int32_t rows,
                         int32_t C, int64_t x_bs, int64_t x_ld, int64_t res_bs, int64_t res_ld, int64_t y_bs, int64_t y_ld,
                         float eps, u2tok_stream_t stream) {
  return layernorm_bf16(BF(x), BF(res), BF(w), BF(b), BFW(y), nb, rows, C, x_bs, x_ld, res_bs, res_ld, y_bs, y_ld, eps,
                        ST(stream));
}

int u2tok_softmax_rows(const float* S, void* P, int32_t nz, int32_t rows, int32_t n, int64_t lds, int64_t ldp,
                       float scale, const void* rel_bias, int32_t H, int32_t max_len, u2tok_stream_t stream) {
  return softmax_rows(S, BFW(P), nz, rows, n, lds, ldp, (int64_t)rows * lds, (int64_t)rows * ldp, scale, BF(rel_bias), H,
                      max_len, ST(stream));
}

int u2tok_transpose_bf16(const void* in, void* out, int32_t nz, int32_t R, int32_t C, int64_t ld_in, int64_t ld_out,
                         int64_t in_zs, int64_t out_zs, int32_t perm16, u2tok_stream_t stream) {
  return transpose_bf16(BF(in), BFW(out), nz, R, C, ld_in, ld_out, in_zs, out_zs, perm16, ST(stream));
}

int u2tok_im2col_patches(const void* vol, int32_t vol_dtype, void* out, int32_t nchunk, int32_t D, int32_t H,
                         int32_t W, int32_t p1, int32_t p2, int32_t p3, u2tok_stream_t stream) {
  return im2col_patches(vol, vol_dtype, BFW(out), nchunk, D, H, W, p1, p2, p3, ST(stream));
}

int u2tok_avgpool3d_tokens(const void* x, void* y, int32_t nb, int32_t g1, int32_t g2, int32_t g3, int32_t w1,
                           int32_t w2, int32_t w3, int32_t C, u2tok_stream_t stream) {
  return avgpool3d_tokens(BF(x), BFW(y), nb, g1, g2, g3, w1, w2, w3, C, ST(stream));
}

int u2tok_score_gemv(const void* x, const void* w, const void* bias, float* scores, int32_t rows, int32_t E,
                     u2tok_stream_t stream) {
  return score_gemv(BF(x), BF(w), BF(bias), scores, rows, E, ST(stream));
}

int u2tok_topk_sorted(const float* scores, int64_t* idx, int32_t B, int32_t n, int32_t k, u2tok_stream_t stream) {
  return topk_sorted(scores, idx, B, n, k, ST(stream));
}

int u2tok_gather_rows(const void* x, const int64_t* idx, void* out, int32_t B, int32_t n, int32_t k, int32_t E,
                      u2tok_stream_t stream) {
  return gather_rows(BF(x), idx, BFW(out), B, n, k, E, ST(stream));
}

int u2tok_fill_rows(const void* src, void* dst, int32_t nb, int64_t n, int64_t dst_bs, u2tok_stream_t stream) {
  return fill_rows(BF(src), BFW(dst), nb, n, dst_bs, ST(stream));
}

int u2tok_multiscale_pool(const void* x, void* out, int32_t B, int32_t k, int32_t E, const void* gate_w,
                          const void* gate_b, float* ws, u2tok_stream_t stream) {
  return multiscale_pool(BF(x), BFW(out), B, k, E, BF(gate_w), BF(gate_b), ws, ST(stream));
}

int u2tok_temporal_attention(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t T,
                             int32_t N, int32_t H, int32_t d, int64_t ld_qkv, int64_t ld_out, float scale,
                             const void* rel_bias, int32_t max_len, u2tok_stream_t stream) {
  return temporal_attention(BF(q), BF(k), BF(v), BFW(out), B, T, N, H, d, ld_qkv, ld_out, scale, BF(rel_bias), max_len,
                            ST(stream));
}

int u2tok_flash_attention_d64(const void* q, const void* k, const void* vt, void* out, int32_t nb, int32_t S,
                              int32_t H, int64_t ld_qk, int64_t q_bs, int64_t ld_out, int64_t out_bs, int32_t S_pad,
                              float scale, const void* qx, const void* kx, const void* vx, void* outx, int64_t x_bs,
                              int64_t ox_bs, int32_t n_extra, u2tok_stream_t stream) {
  return flash_attention_d64(BF(q), BF(k), BF(vt), BFW(out), nb, S, H, ld_qk, q_bs, ld_out, out_bs, S_pad, scale,
                             BF(qx), BF(kx), BF(vx), BFW(outx), x_bs, ox_bs, n_extra, nullptr, 0, ST(stream));
}
int u2tok_flash_attention_d64_lse(const void* q, const void* k, const void* vt, void* out, int32_t nb, int32_t S,
                                  int32_t H, int64_t ld_qk, int64_t q_bs, int64_t ld_out, int64_t out_bs, int32_t S_pad,
                                  float scale, const void* qx, const void* kx, const void* vx, void* outx, int64_t x_bs,
                                  int64_t ox_bs, int32_t n_extra, float* lse, int64_t lse_ld, u2tok_stream_t stream) {
  if (!lse) return U2_ERR_ARG;
  return flash_attention_d64(BF(q), BF(k), BF(vt), BFW(out), nb, S, H, ld_qk, q_bs, ld_out, out_bs, S_pad, scale,
                             BF(qx), BF(kx), BF(vx), BFW(outx), x_bs, ox_bs, n_extra, lse, lse_ld, ST(stream));
}

size_t u2tok_tok_attention_workspace_bytes(int32_t nb, int32_t H, int32_t Sq, int32_t Skv, int32_t d) {
  return tok_attention_workspace_bytes(nb, H, Sq, Skv, d);
}
// the arguments every attention entry point below shares
static AttnCall attn_call(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv, int32_t Hq,
                          int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs,
                          int64_t v_bs, int64_t o_bs, float scale) {
  AttnCall c;
  c.q = BF(q); c.k = BF(k); c.v = BF(v); c.out = BFW(out);
  c.nb = nb; c.Sq = Sq; c.Skv = Skv; c.H = Hq; c.Hkv = Hkv; c.d = d;
  c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.ldo = ldo; c.q_bs = q_bs; c.k_bs = k_bs; c.v_bs = v_bs; c.o_bs = o_bs;
  c.scale = scale;
  return c;
}
int u2tok_tok_attention(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv, int32_t H,
                        int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs, int64_t v_bs,
                        int64_t o_bs, float scale, const void* rel_bias, int32_t max_len, int32_t splits, void* workspace,
                        size_t workspace_bytes, u2tok_stream_t stream) {
  AttnCall c = attn_call(q, k, v, out, nb, Sq, Skv, H, H, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale);
  c.rel_bias = BF(rel_bias); c.max_len = max_len;
  c.force_splits = splits; c.ws = workspace; c.ws_bytes = workspace_bytes;
  return attention(c, ST(stream));
}

int u2tok_attention_gqa(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv, int32_t Hq,
                        int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs, int64_t k_bs,
                        int64_t v_bs, int64_t o_bs, float scale, int32_t causal, u2tok_stream_t stream) {
  AttnCall c = attn_call(q, k, v, out, nb, Sq, Skv, Hq, Hkv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale);
  c.causal = causal;  // (no workspace: no key splits)
  return attention(c, ST(stream));
}
int u2tok_attention_gqa_split(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                              int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                              int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, void* workspace, size_t workspace_bytes,
                              u2tok_stream_t stream) {
  AttnCall c = attn_call(q, k, v, out, nb, Sq, Skv, Hq, Hkv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale);
  c.ws = workspace; c.ws_bytes = workspace_bytes;  // (the heuristic's splits)
  return attention(c, ST(stream));
}
int u2tok_rmsnorm_bf16(const void* x, const void* w, void* y, int64_t rows, int32_t C, int64_t ldx, int64_t ldy, float eps,
                       u2tok_stream_t stream) {
  return rmsnorm_bf16(BF(x), BF(w), BFW(y), rows, C, ldx, ldy, eps, ST(stream));
}
int u2tok_qk_norm_rope(void* qkv, const void* wq, const void* wk, const void* cos, const void* sin, int32_t cos_sin_f32,
                       int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t cs_ld, float eps,
                       u2tok_stream_t stream) {
  return qk_norm_rope(BFW(qkv), BF(wq), BF(wk), cos, sin, cos_sin_f32, rows, Hq, Hkv, D, ld, cs_ld, eps, nullptr, nullptr, 0, 0, 0,
                      ST(stream));
}
int u2tok_qk_norm_rope_kv(void* qkv, const void* wq, const void* wk, const void* cos, const void* sin, int32_t cos_sin_f32,
                          int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t cs_ld, float eps,
                          void* k_cache, void* v_cache, int32_t S, int64_t kv_stride, int32_t s_off, u2tok_stream_t stream) {
  if (!k_cache || !v_cache) return U2_ERR_ARG;
  return qk_norm_rope(BFW(qkv), BF(wq), BF(wk), cos, sin, cos_sin_f32, rows, Hq, Hkv, D, ld, cs_ld, eps, BFW(k_cache),
                      BFW(v_cache), S, kv_stride, s_off, ST(stream));
}
int u2tok_qk_norm_rope_kv8(void* qkv, const void* wq, const void* wk, const void* cos, const void* sin, int32_t cos_sin_f32,
                           int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t cs_ld, float eps, void* k_codes,
                           void* v_codes, float* k_scales, float* v_scales, int32_t S, int32_t capacity, int32_t s_off,
                           u2tok_stream_t stream) {
  return qk_norm_rope_kv8(BFW(qkv), BF(wq), BF(wk), cos, sin, cos_sin_f32, rows, Hq, Hkv, D, ld, cs_ld, eps, reinterpret_cast<uint8_t*>(k_codes),
                          reinterpret_cast<uint8_t*>(v_codes), k_scales, v_scales, S, capacity, s_off, ST(stream));
}
static DecodeCfg dec_cfg(const u2tok_decode_config* c) {
  DecodeCfg d;
  d.B = c->B; d.E = c->E; d.Hq = c->Hq; d.Hkv = c->Hkv; d.D = c->D; d.I = c->I;
  d.eps = c->eps; d.qk_eps = c->qk_eps; d.scale = c->scale;
  return d;
}
static bool dec_ok(const u2tok_decode_config* c) {
  return c && c->B > 0 && c->B <= 64 && c->E > 0 && !(c->E & 31) && c->Hq > 0 && c->Hkv > 0 && c->Hq % c->Hkv == 0 &&
         (c->D == 64 || c->D == 96 || c->D == 128) && c->I > 0 && !(c->I & 31) && (c->wform == 0 || c->wform == 2);
}
size_t u2tok_decoder_decode_workspace_bytes(const u2tok_decode_config* c, int32_t T) {
  return dec_ok(c) && T > 0 ? decoder_decode_workspace_bytes(dec_cfg(c), T) : 0;
}
static_assert(sizeof(u2tok_decode_lora) == sizeof(DecodeLora) && sizeof(u2tok_lora_seg) == sizeof(LoraSeg), "one layout");
// The one place that reads the ABI's spelling of a weight form: wform = 2 with all four scale fields set (the e2m1 codes' block-scale
// bytes) is E2M1; wform = 0 with none set is ELEM, with all four set (fp32 row scales) E4M3; everything else is refused -- some of
// the four set, and wform = 2 with none: a step of codes must not be taken for a 16-bit one, whose weights are four times as long.
static int dec_args(const u2tok_decode_config* c, const u2tok_decode_layer* l, DecodeCfg& cfg, DecodeLayer& d) {
  if (!dec_ok(c) || !l) return U2_ERR_ARG;
  const int set = !!l->scale_qkv + !!l->scale_o + !!l->scale_gu + !!l->scale_down;
  if ((set != 0 && set != 4) || (c->wform == 2 && set == 0)) return U2_ERR_ARG;
  cfg = dec_cfg(c);
  cfg.form = c->wform == 2 ? WForm::E2M1 : set ? WForm::E4M3 : WForm::ELEM;
  d.w_in_norm = BF(l->w_in_norm); d.Wqkv = l->Wqkv; d.bqkv = BF(l->bqkv); d.wq_norm = BF(l->wq_norm); d.wk_norm = BF(l->wk_norm);
  d.Wo = l->Wo; d.bo = BF(l->bo); d.w_post_norm = BF(l->w_post_norm);
  d.Wgu = l->Wgu; d.bgu = BF(l->bgu); d.Wdown = l->Wdown; d.bdown = BF(l->bdown);
  d.scale_qkv = l->scale_qkv; d.scale_o = l->scale_o; d.scale_gu = l->scale_gu; d.scale_down = l->scale_down;
  d.lora = reinterpret_cast<const DecodeLora*>(l->lora);
  return U2_OK;
}
int u2tok_decoder_decode_pre(const u2tok_decode_config* c, const u2tok_decode_layer* l, const void* x, const void* cos, const void* sin,
                             int32_t cos_sin_f32, int64_t cs_ld, void* qkv, void* k_cache, void* v_cache, int64_t kv_stride,
                             int32_t s_off, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  DecodeCfg cfg;
  DecodeLayer d;
  const int e = dec_args(c, l, cfg, d);
  if (e != U2_OK) return e;
  return decoder_decode_pre(cfg, d, BF(x), cos, sin, cos_sin_f32, cs_ld, BFW(qkv), BFW(k_cache), BFW(v_cache), kv_stride, s_off,
                            workspace, workspace_bytes, ST(stream));
}
int u2tok_decoder_decode_post(const u2tok_decode_config* c, const u2tok_decode_layer* l, const void* x, const void* qkv, const void* K,
                              const void* V, int32_t T, int64_t kv_stride, int32_t batched, const int32_t* kv_start, void* out,
                              void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  DecodeCfg cfg;
  DecodeLayer d;
  const int e = dec_args(c, l, cfg, d);
  if (e != U2_OK) return e;
  return decoder_decode_post(cfg, d, BF(x), BF(qkv), BF(K), BF(V), T, kv_stride, batched != 0, kv_start, BFW(out), workspace,
                             workspace_bytes, ST(stream));
}
int u2tok_decoder_decode_post_kv8(const u2tok_decode_config* c, const u2tok_decode_layer* l, const void* x, const void* qkv,
                                  const void* k_new, const void* v_new, void* k_codes, void* v_codes, float* k_scales, float* v_scales,
                                  int32_t capacity, int32_t k_first, int32_t s_off, const int32_t* kv_start, void* out, void* workspace,
                                  size_t workspace_bytes, u2tok_stream_t stream) {
  DecodeCfg cfg;
  DecodeLayer d;
  const int e = dec_args(c, l, cfg, d);
  if (e != U2_OK) return e;
  DecodeKv8 kv;
  kv.k_new = BF(k_new); kv.v_new = BF(v_new);
  kv.Kc = reinterpret_cast<uint8_t*>(k_codes); kv.Vc = reinterpret_cast<uint8_t*>(v_codes);
  kv.Ks = k_scales; kv.Vs = v_scales;
  kv.capacity = capacity; kv.k_first = k_first; kv.s_off = s_off;
  return decoder_decode_post_kv8(cfg, d, BF(x), BF(qkv), kv, kv_start, BFW(out), workspace, workspace_bytes, ST(stream));
}
// ---- the whole-stack step (decoder.hip): the layers' descriptors decoded as the two per-layer entries decode theirs, nothing kept
extern "C++" {
// (the cache of one layer, per kind of descriptor)
static void stack_cache(const u2tok_decode_stack_layer& l, DecodeStackLayer& s) {
  s.kc = BFW(l.k_cache); s.vc = BFW(l.v_cache);
  s.kv_stride = l.kv_stride;
}
static void stack_cache(const u2tok_decode_stack_layer_kv8& l, DecodeStackLayer& s) {
  s.kv8 = true;
  s.Kc = reinterpret_cast<uint8_t*>(l.k_codes); s.Vc = reinterpret_cast<uint8_t*>(l.v_codes);
  s.Ks = l.k_scales; s.Vs = l.v_scales;
  s.capacity = l.capacity;
}
template <typename Layer>  // u2tok_decode_stack_layer or u2tok_decode_stack_layer_kv8
static int stack_args(const Layer* L, int32_t n, std::vector<DecodeStackLayer>& v) {
  if (!L || n <= 0) return U2_ERR_ARG;
  try { v.resize((size_t)n); } catch (const std::bad_alloc&) { return U2_ERR_ARG; }
  for (int32_t i = 0; i < n; ++i) {
    DecodeStackLayer& s = v[(size_t)i];
    const int e = dec_args(L[i].cfg, L[i].layer, s.cfg, s.layer);
    if (e != U2_OK) return e;
    stack_cache(L[i], s);
    s.s_off = L[i].s_off; s.k_first = L[i].k_first; s.T = L[i].T;
  }
  return U2_OK;
}
}  // extern "C++"
size_t u2tok_decoder_decode_stack_workspace_bytes(const u2tok_decode_stack_layer* L, int32_t n_layers) {
  std::vector<DecodeStackLayer> v;
  return stack_args(L, n_layers, v) == U2_OK ? decoder_decode_stack_workspace_bytes(v.data(), n_layers) : 0;
}
int u2tok_decoder_decode_stack(const u2tok_decode_stack_layer* L, int32_t n_layers, const void* x, const void* cos, const void* sin,
                               int32_t cos_sin_f32, int64_t cs_ld, int32_t batched, const int32_t* kv_start, const void* w_final_norm,
                               float final_eps, int32_t tail_norm, void* out, void* workspace, size_t workspace_bytes,
                               u2tok_stream_t stream) {
  std::vector<DecodeStackLayer> v;
  const int e = stack_args(L, n_layers, v);
  if (e != U2_OK) return e;
  return decoder_decode_stack(v.data(), n_layers, BF(x), cos, sin, cos_sin_f32, cs_ld, batched != 0, kv_start, BF(w_final_norm), final_eps,
                              tail_norm != 0, BFW(out), workspace, workspace_bytes, ST(stream));
}
// ---- the head of the step (decoder.hip): wform names the form outright (0 / 1 / 2); a leading dimension of 0 is the dense one
static int head_args(const u2tok_decode_head_desc* h, DecodeHead& d) {
  if (!h || h->wform < 0 || h->wform > 2 || h->E <= 0 || h->ldw < 0 || h->lds < 0) return U2_ERR_ARG;
  d.form = (WForm)h->wform;
  d.w_norm = BF(h->w_norm); d.W = h->W; d.scale = h->scale;
  d.E = h->E; d.V = h->V; d.eps = h->eps;
  d.ldw = h->ldw ? h->ldw : h->E / wform_facts(d.form).ldw_div;
  d.lds = h->lds ? h->lds : h->E >> 5;
  return U2_OK;
}
size_t u2tok_decode_head_workspace_bytes(int32_t B, int32_t E) { return decode_head_workspace_bytes(B, E); }
int u2tok_decode_head(const u2tok_decode_head_desc* head, const void* x, int64_t ldx, int32_t B, float* logits, int64_t ld_logits,
                      void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  DecodeHead d;
  const int e = head_args(head, d);
  if (e != U2_OK) return e;
  return decode_head(d, BF(x), ldx, B, logits, ld_logits, workspace, workspace_bytes, ST(stream));
}
size_t u2tok_decoder_decode_stack_head_workspace_bytes(const u2tok_decode_stack_layer* L, int32_t n_layers, const u2tok_decode_head_desc* head) {
  std::vector<DecodeStackLayer> v;
  DecodeHead d;
  if (stack_args(L, n_layers, v) != U2_OK || head_args(head, d) != U2_OK) return 0;
  return decoder_decode_stack_head_workspace_bytes(v.data(), n_layers, d);
}
int u2tok_decoder_decode_stack_head(const u2tok_decode_stack_layer* L, int32_t n_layers, const void* x, const void* cos, const void* sin,
                                    int32_t cos_sin_f32, int64_t cs_ld, int32_t batched, const int32_t* kv_start, int32_t tail_norm,
                                    void* out, const u2tok_decode_head_desc* head, float* logits, int64_t ld_logits, void* workspace,
                                    size_t workspace_bytes, u2tok_stream_t stream) {
  std::vector<DecodeStackLayer> v;
  DecodeHead d;
  int e = stack_args(L, n_layers, v);
  if (e == U2_OK) e = head_args(head, d);
  if (e != U2_OK) return e;
  return decoder_decode_stack_head(v.data(), n_layers, BF(x), cos, sin, cos_sin_f32, cs_ld, batched != 0, kv_start, tail_norm != 0, BFW(out), d,
                                   logits, ld_logits, workspace, workspace_bytes, ST(stream));
}
// ---- the whole-stack step and the step with the head on an e4m3 KV cache: the same two walks over layers marked kv8, always with
// the batched decode attention
size_t u2tok_decoder_decode_stack_kv8_workspace_bytes(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers) {
  std::vector<DecodeStackLayer> v;
  return stack_args(L, n_layers, v) == U2_OK ? decoder_decode_stack_workspace_bytes(v.data(), n_layers) : 0;
}
int u2tok_decoder_decode_stack_kv8(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers, const void* x, const void* cos, const void* sin,
                                   int32_t cos_sin_f32, int64_t cs_ld, const int32_t* kv_start, const void* w_final_norm, float final_eps,
                                   int32_t tail_norm, void* out, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  std::vector<DecodeStackLayer> v;
  const int e = stack_args(L, n_layers, v);
  if (e != U2_OK) return e;
  return decoder_decode_stack(v.data(), n_layers, BF(x), cos, sin, cos_sin_f32, cs_ld, true, kv_start, BF(w_final_norm), final_eps,
                              tail_norm != 0, BFW(out), workspace, workspace_bytes, ST(stream));
}
size_t u2tok_decoder_decode_stack_head_kv8_workspace_bytes(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers,
                                                           const u2tok_decode_head_desc* head) {
  std::vector<DecodeStackLayer> v;
  DecodeHead d;
  if (stack_args(L, n_layers, v) != U2_OK || head_args(head, d) != U2_OK) return 0;
  return decoder_decode_stack_head_workspace_bytes(v.data(), n_layers, d);
}
int u2tok_decoder_decode_stack_head_kv8(const u2tok_decode_stack_layer_kv8* L, int32_t n_layers, const void* x, const void* cos, const void* sin,
                                        int32_t cos_sin_f32, int64_t cs_ld, const int32_t* kv_start, int32_t tail_norm, void* out,
                                        const u2tok_decode_head_desc* head, float* logits, int64_t ld_logits, void* workspace,
                                        size_t workspace_bytes, u2tok_stream_t stream) {
  std::vector<DecodeStackLayer> v;
  DecodeHead d;
  int e = stack_args(L, n_layers, v);
  if (e == U2_OK) e = head_args(head, d);
  if (e != U2_OK) return e;
  return decoder_decode_stack_head(v.data(), n_layers, BF(x), cos, sin, cos_sin_f32, cs_ld, true, kv_start, tail_norm != 0, BFW(out), d, logits,
                                   ld_logits, workspace, workspace_bytes, ST(stream));
}
// ---- the few-rows product (gemm_rows.hip): one filler for the five exports; a quantised form without its scales is refused here
static int rows(WForm form, const void* A, const void* W, const void* scale, int64_t lds, void* C, const void* bias, const void* R,
                int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags, u2tok_stream_t stream,
                const RowsNorm& norm = RowsNorm{}) {
  if (form != WForm::ELEM && !scale) return U2_ERR_ARG;
  RowsArgs a;
  a.A = BF(A); a.W = W; a.scale = scale; a.form = form; a.C = C; a.bias = BF(bias); a.R = BF(R);
  a.M = M; a.N = N; a.K = K;
  a.lda = lda; a.ldw = ldw; a.lds = lds; a.ldc = ldc; a.ldr = ldr;
  a.flags = flags;
  a.norm = norm;
  return gemm_rows(a, ST(stream));
}
// (with the RMSNorm of the finished rows in the launch's tail; a null norm weight is refused: the plain products are the four below)
int u2tok_gemm_rows_norm(const void* A, const void* W, void* C, const void* bias, const void* R, int32_t M, int32_t N, int32_t K, int64_t lda,
                         int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags, int32_t wform, const void* scale, int64_t lds,
                         const void* w_norm, float eps, void* Yn, int64_t ldn, void* ticket, u2tok_stream_t stream) {
  if (!w_norm || !wform_known((WForm)wform)) return U2_ERR_ARG;
  RowsNorm nm;
  nm.w = BF(w_norm); nm.Yn = BFW(Yn); nm.ticket = reinterpret_cast<uint32_t*>(ticket); nm.ld = ldn; nm.eps = eps;
  return rows((WForm)wform, A, W, scale, lds, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream, nm);
}
int u2tok_gemm_rows_w8(const void* A, const void* W8, const float* scale, void* C, const void* bias, const void* R, int32_t M, int32_t N,
                       int32_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags, u2tok_stream_t stream) {
  if (M > 16) return U2_ERR_ARG;  // (this entry point keeps the range it was published with; 17 .. 64 rows: _wide)
  return rows(WForm::E4M3, A, W8, scale, 0, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream);
}
int u2tok_gemm_rows_w8_wide(const void* A, const void* W8, const float* scale, void* C, const void* bias, const void* R, int32_t M,
                            int32_t N, int32_t K, int64_t lda, int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags,
                            u2tok_stream_t stream) {
  return rows(WForm::E4M3, A, W8, scale, 0, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream);
}
// (e2m1 codes with e8m0 block scales: one entry for 1 .. 64 rows)
int u2tok_gemm_rows_w4(const void* A, const void* W4, const uint8_t* S, void* C, const void* bias, const void* R, int32_t M, int32_t N,
                       int32_t K, int64_t lda, int64_t ldw, int64_t lds, int64_t ldc, int64_t ldr, int32_t flags,
                       u2tok_stream_t stream) {
  return rows(WForm::E2M1, A, W4, S, lds, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream);
}
// (on element-type weights, outside u2tok_gemm_bf16's plan)
int u2tok_gemm_rows(const void* A, const void* W, void* C, const void* bias, const void* R, int32_t M, int32_t N, int32_t K, int64_t lda,
                    int64_t ldw, int64_t ldc, int64_t ldr, int32_t flags, u2tok_stream_t stream) {
  return rows(WForm::ELEM, A, W, nullptr, 0, C, bias, R, M, N, K, lda, ldw, ldc, ldr, flags, stream);
}
int u2tok_kv_quantize_rows(const void* k, const void* v, int32_t B, int32_t Hkv, int32_t n, int32_t D, int64_t k_bs, int64_t k_hs,
                           int64_t k_rs, int64_t v_bs, int64_t v_hs, int64_t v_rs, void* k_codes, void* v_codes, float* k_scales,
                           float* v_scales, int32_t capacity, int32_t s_off, u2tok_stream_t stream) {
  return kv_quantize_rows(BF(k), BF(v), B, Hkv, n, D, k_bs, k_hs, k_rs, v_bs, v_hs, v_rs, reinterpret_cast<uint8_t*>(k_codes),
                          reinterpret_cast<uint8_t*>(v_codes), k_scales, v_scales, capacity, s_off, false, ST(stream));
}
size_t u2tok_decode_attention_kv8_workspace_bytes(int32_t B, int32_t Hq, int32_t Hkv, int32_t T, int32_t D) {
  return decode_attention_kv8_workspace_bytes(B, Hq, Hkv, T, D);
}
int u2tok_decode_attention_kv8(const void* q, const void* k_codes, const void* v_codes, const float* k_scales, const float* v_scales,
                               void* out, int32_t B, int32_t Hq, int32_t Hkv, int32_t T, int32_t D, int64_t ldq, int64_t kv_stride,
                               int64_t scale_stride, int64_t ldo, float scale, const int32_t* kv_start, void* workspace,
                               size_t workspace_bytes, u2tok_stream_t stream) {
  return decode_attention_kv8(BF(q), reinterpret_cast<const uint8_t*>(k_codes), reinterpret_cast<const uint8_t*>(v_codes), k_scales,
                              v_scales, BFW(out), B, Hq, Hkv, T, D, ldq, kv_stride, scale_stride, ldo, scale, kv_start, workspace,
                              workspace_bytes, false, ST(stream));
}
size_t u2tok_attention_kv8_rows_workspace_bytes(int32_t B, int32_t Sq, int32_t Hq, int32_t Hkv, int32_t T, int32_t D) {
  return attention_kv8_rows_workspace_bytes(B, Sq, Hq, Hkv, T, D);
}
int u2tok_attention_kv8_rows(const void* q, const void* k_codes, const void* v_codes, const float* k_scales, const float* v_scales,
                             void* out, int32_t B, int32_t Sq, int32_t Hq, int32_t Hkv, int32_t T, int32_t D, int64_t ldq,
                             int64_t kv_stride, int64_t sc_stride, int64_t ldo, float scale, int32_t window, const int32_t* kv_start,
                             void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return attention_kv8_rows(BF(q), reinterpret_cast<const uint8_t*>(k_codes), reinterpret_cast<const uint8_t*>(v_codes), k_scales, v_scales,
                            BFW(out), B, Sq, Hq, Hkv, T, D, ldq, kv_stride, sc_stride, ldo, scale, window, kv_start, workspace,
                            workspace_bytes, false, ST(stream));
}
size_t u2tok_decode_attention_workspace_bytes(int32_t B, int32_t Hq, int32_t Hkv, int32_t T, int32_t D) {
  return decode_attention_workspace_bytes(B, Hq, Hkv, T, D);
}
int u2tok_decode_attention(const void* q, const void* K, const void* V, void* out, int32_t B, int32_t Hq, int32_t Hkv, int32_t T,
                           int32_t D, int64_t ldq, int64_t kv_stride, int64_t ldo, float scale, const int32_t* kv_start,
                           void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return decode_attention(BF(q), BF(K), BF(V), BFW(out), B, Hq, Hkv, T, D, ldq, kv_stride, ldo, scale, kv_start, workspace,
                          workspace_bytes, false, ST(stream));
}
int u2tok_swiglu_bf16(const void* gate_up, void* out, int64_t rows, int32_t I, int64_t ld_in, int64_t ld_out,
                      u2tok_stream_t stream) {
  return swiglu_bf16(BF(gate_up), BFW(out), rows, I, ld_in, ld_out, ST(stream));
}

int u2tok_rope_apply(void* x, int64_t n_outer, int32_t S, int32_t n_inner, int32_t H, int32_t d, int64_t ld,
                     int32_t max_len, int32_t inverse, u2tok_stream_t stream) {
  return rope_apply(BFW(x), n_outer, S, n_inner, H, d, ld, max_len, inverse, ST(stream));
}

// ---- backward-pass building blocks (backward.hip)
int u2tok_gelu_fwd(const void* z, void* y, int64_t n, u2tok_stream_t stream) { return gelu_fwd(BF(z), BFW(y), n, ST(stream)); }
int u2tok_gelu_bwd(const void* z, const void* dy, void* dz, int64_t n, u2tok_stream_t stream) {
  return gelu_bwd(BF(z), BF(dy), BFW(dz), n, ST(stream));
}
size_t u2tok_colsum_workspace_bytes(int32_t rows, int32_t C) { return colsum_workspace_bytes(rows, C); }
int u2tok_colsum_bf16(const void* x, const void* y, float* out, void* out_bf16, int32_t rows, int32_t C, int64_t ldx,
                      int64_t ldy, void* workspace, int32_t accumulate, u2tok_stream_t stream) {
  return colsum_bf16(BF(x), BF(y), out, BFW(out_bf16), rows, C, ldx, ldy, reinterpret_cast<float*>(workspace), accumulate,
                     ST(stream));
}
size_t u2tok_layernorm_bwd_workspace_bytes(int32_t rows, int32_t C) { return layernorm_bwd_workspace_bytes(rows, C); }
int u2tok_layernorm_bwd(const void* x, const void* res, const void* w, const void* dy, void* dv, float* dw, float* db,
                        int32_t rows, int32_t C, float eps, void* workspace, int32_t accumulate, u2tok_stream_t stream) {
  return layernorm_bwd(BF(x), BF(res), BF(w), BF(dy), BFW(dv), dw, db, rows, C, eps, reinterpret_cast<float*>(workspace),
                       accumulate, ST(stream));
}
int u2tok_softmax_bwd(const void* P, const float* dP, void* dS, int64_t nrows, int32_t n, int64_t ldp, int64_t lddp,
                      u2tok_stream_t stream) {
  return softmax_bwd(BF(P), dP, BFW(dS), nrows, n, ldp, lddp, ST(stream));
}
int u2tok_relbias_grad(const void* dS, float* dtable, int32_t nz, int32_t S, int32_t H, int64_t ldp, int32_t max_len,
                       u2tok_stream_t stream) {
  return relbias_grad(BF(dS), dtable, nz, S, H, ldp, max_len, ST(stream));
}
int u2tok_rowdot_bf16(const void* a, const void* b, float* out, int64_t rows, int32_t C, int64_t lda, int64_t ldb,
                      u2tok_stream_t stream) {
  return rowdot_bf16(BF(a), BF(b), out, rows, C, lda, ldb, ST(stream));
}
int u2tok_ce_lse_update(const void* Z, int64_t ldz, int32_t rows, int32_t Vs, int64_t v0, const int64_t* labels, float* m, float* l,
                        float* zt, u2tok_stream_t stream) {
  return ce_lse_update(BF(Z), ldz, rows, Vs, v0, labels, m, l, zt, ST(stream));
}
int u2tok_ce_stats_update(const void* Z, int64_t ldz, int32_t rows, int32_t Vs, int64_t v0, const int64_t* labels, float* m, float* l,
                          float* zt, float* amax, int64_t* aidx, float* zsum, float* l2, u2tok_stream_t stream) {
  return ce_stats_update(BF(Z), ldz, rows, Vs, v0, labels, m, l, zt, amax, aidx, zsum, l2, ST(stream));
}
int u2tok_ce_grad_inplace(void* Z, int64_t ldz, int32_t rows, int32_t Vs, int64_t v0, const int64_t* labels, const float* lse,
                          const float* coef, u2tok_stream_t stream) {
  return ce_grad_inplace(BFW(Z), ldz, rows, Vs, v0, labels, lse, coef, ST(stream));
}
size_t u2tok_sample_warp_split_workspace_bytes(int32_t rows, int32_t V) { return sample_warp_split_workspace_bytes(rows, V); }
int32_t u2tok_sample_warp_split_launches(int32_t V, int32_t top_k, float top_p, int32_t min_keep) {
  return sample_warp_split_launches(V, top_k, top_p, min_keep);
}
int u2tok_sample_warp_split(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int32_t rows, int32_t V, float temperature,
                            int32_t top_k, float top_p, int32_t min_keep, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return sample_warp_split(logits, ld_in, out, ld_out, rows, V, temperature, top_k, top_p, min_keep, workspace, workspace_bytes, ST(stream));
}
size_t u2tok_sample_warp_workspace_bytes(int32_t rows, int32_t V) { return sample_warp_workspace_bytes(rows, V); }
int u2tok_sample_warp(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int32_t rows, int32_t V, float temperature,
                      int32_t top_k, float top_p, int32_t min_keep, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return sample_warp(logits, ld_in, out, ld_out, rows, V, temperature, top_k, top_p, min_keep, workspace, workspace_bytes, ST(stream));
}
int u2tok_adamw_step(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, const uint8_t* group, void* out_bf16,
                     int64_t n, const float* lr, const float* weight_decay, int32_t ngroups, float beta1, float beta2, float eps,
                     int32_t step, float grad_scale, const float* grad_coef, u2tok_stream_t stream) {
  if (!lr || !weight_decay || ngroups <= 0 || ngroups > 8 || step <= 0 || (ngroups > 1 && !group)) return U2_ERR_ARG;
  AdamWArgs a;
  for (int i = 0; i < 8; ++i) { a.lr[i] = lr[i < ngroups ? i : 0]; a.wd[i] = weight_decay[i < ngroups ? i : 0]; }
  a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  a.inv_c1 = (float)(1.0 / (1.0 - pow((double)beta1, step)));
  a.inv_sqrt_c2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, step)));
  a.gscale = grad_scale; a.gcoef = grad_coef;
  return adamw_step(master, exp_avg, exp_avg_sq, BF(grad), group, BFW(out_bf16), n, a, ST(stream));
}
size_t u2tok_flash_attention_d64_bwd_workspace_bytes(int32_t nb, int32_t S, int32_t H) {
  return flash_attention_d64_bwd_workspace_bytes(nb, S, H);
}
int32_t u2tok_flash_attention_d64_bwd(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t bs_qkv,
                                      const void* out, const void* d_out, int64_t ld_o, int64_t bs_o, void* dq, void* dk,
                                      void* dv, int64_t ld_d, int64_t bs_d, int32_t nb, int32_t S, int32_t H, float scale,
                                      const float* lse, int64_t lse_ld, void* workspace, size_t workspace_bytes,
                                      u2tok_stream_t stream) {
  return flash_attention_d64_bwd(BF(q), BF(k), BF(v), ld_qkv, bs_qkv, BF(out), BF(d_out), ld_o, bs_o, BFW(dq), BFW(dk), BFW(dv),
                                 ld_d, bs_d, nb, S, H, scale, lse, lse_ld, workspace, workspace_bytes, ST(stream));
}

// ---- the decoder's training route
int u2tok_attention_gqa_ex(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                           int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                           int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, int32_t causal, const int32_t* kv_len,
                           float* lse, int64_t lse_ld, u2tok_stream_t stream) {
  return u2tok_attention_gqa_range(q, k, v, out, nb, Sq, Skv, Hq, Hkv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale, causal,
                                   nullptr, kv_len, lse, lse_ld, stream);
}
int u2tok_attention_gqa_range(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                              int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                              int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, int32_t causal, const int32_t* kv_start,
                              const int32_t* kv_len, float* lse, int64_t lse_ld, u2tok_stream_t stream) {
  AttnCall c = attn_call(q, k, v, out, nb, Sq, Skv, Hq, Hkv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale);
  c.causal = causal; c.kv_start = kv_start; c.kv_len = kv_len; c.lse = lse; c.lse_ld = lse_ld;
  return attention(c, ST(stream));
}
int u2tok_attention_gqa_band(const void* q, const void* k, const void* v, void* out, int32_t nb, int32_t Sq, int32_t Skv,
                             int32_t Hq, int32_t Hkv, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bs,
                             int64_t k_bs, int64_t v_bs, int64_t o_bs, float scale, int32_t causal, const int32_t* kv_start,
                             const int32_t* kv_len, float* lse, int64_t lse_ld, int64_t k_hs, int64_t v_hs, int32_t window,
                             u2tok_stream_t stream) {
  if (!k_hs || !v_hs) return U2_ERR_ARG;  // (a caller names its head strides: 0 is the descriptor's own "column-packed")
  AttnCall c = attn_call(q, k, v, out, nb, Sq, Skv, Hq, Hkv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale);
  c.causal = causal; c.kv_start = kv_start; c.kv_len = kv_len; c.lse = lse; c.lse_ld = lse_ld;
  c.k_hs = k_hs; c.v_hs = v_hs; c.window = window;
  return attention(c, ST(stream));
}
size_t u2tok_attention_gqa_bwd_workspace_bytes(int32_t nb, int32_t S, int32_t Hq) {
  return attention_gqa_bwd_workspace_bytes(nb, S, Hq);
}
int u2tok_attention_gqa_bwd(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t bs_qkv, const void* out,
                            const void* d_out, int64_t ld_o, int64_t bs_o, void* dq, void* dk, void* dv, int64_t ld_d, int64_t bs_d,
                            int32_t nb, int32_t S, int32_t Hq, int32_t Hkv, int32_t d, float scale, const int32_t* kv_len,
                            const float* lse, int64_t lse_ld, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return attention_gqa_bwd(BF(q), BF(k), BF(v), ld_qkv, bs_qkv, BF(out), BF(d_out), ld_o, bs_o, BFW(dq), BFW(dk), BFW(dv), ld_d,
                           bs_d, nb, S, Hq, Hkv, d, scale, kv_len, lse, lse_ld, workspace, workspace_bytes, ST(stream));
}
int u2tok_attention_gqa_bwd_d96(const void* q, const void* k, const void* v, int64_t ld_qkv, int64_t bs_qkv, const void* out,
                                const void* d_out, int64_t ld_o, int64_t bs_o, void* dq, void* dk, void* dv, int64_t ld_d,
                                int64_t bs_d, int32_t nb, int32_t S, int32_t Hq, int32_t Hkv, float scale, const int32_t* kv_len,
                                const float* lse, int64_t lse_ld, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return attention_gqa_bwd_d96(BF(q), BF(k), BF(v), ld_qkv, bs_qkv, BF(out), BF(d_out), ld_o, bs_o, BFW(dq), BFW(dk), BFW(dv), ld_d,
                               bs_d, nb, S, Hq, Hkv, scale, kv_len, lse, lse_ld, workspace, workspace_bytes, ST(stream));
}
size_t u2tok_rmsnorm_bwd_workspace_bytes(int32_t rows, int32_t C) { return rmsnorm_bwd_workspace_bytes(rows, C); }
int u2tok_rmsnorm_bwd(const void* x, const void* w, const void* dy, const void* dres, void* dx, float* dw, int32_t rows, int32_t C,
                      float eps, void* workspace, size_t workspace_bytes, int32_t accumulate, u2tok_stream_t stream) {
  return rmsnorm_bwd(BF(x), BF(w), BF(dy), BF(dres), BFW(dx), dw, rows, C, eps, reinterpret_cast<float*>(workspace),
                     workspace_bytes, accumulate, ST(stream));
}
size_t u2tok_qk_norm_rope_bwd_workspace_bytes(int64_t rows, int32_t D) { return qk_norm_rope_bwd_workspace_bytes(rows, D); }
int u2tok_qk_norm_rope_bwd(void* dqkv, const void* pre, const void* wq, const void* wk, const void* cos, const void* sin,
                           int32_t cos_sin_f32, int64_t rows, int32_t Hq, int32_t Hkv, int32_t D, int64_t ld, int64_t ld_pre,
                           int64_t cs_ld, float eps, float* dwq, float* dwk, void* workspace, size_t workspace_bytes,
                           int32_t accumulate, u2tok_stream_t stream) {
  return qk_norm_rope_bwd(BFW(dqkv), BF(pre), BF(wq), BF(wk), cos, sin, cos_sin_f32, rows, Hq, Hkv, D, ld, ld_pre, cs_ld, eps, dwq,
                          dwk, reinterpret_cast<float*>(workspace), workspace_bytes, accumulate, ST(stream));
}
int u2tok_swiglu_bwd(const void* gu, const void* dact, void* dgu, int64_t rows, int32_t I, int64_t ld_gu, int64_t ld_da,
                     int64_t ld_dgu, u2tok_stream_t stream) {
  return swiglu_bwd(BF(gu), BF(dact), BFW(dgu), rows, I, ld_gu, ld_da, ld_dgu, ST(stream));
}

}  // extern "C"
