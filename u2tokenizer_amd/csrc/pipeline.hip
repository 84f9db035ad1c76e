// Launch sequences of the three module forwards of the hot path (reference: u2_arch.py:91-117):
//   ViT3DTower (vit.py:114-126,148-164) -> SpatialPoolingProjector (spatial_pooling_projector.py:34-52)
//   -> u2Tokenizer (u2Tokenizer.py:40-47 = svr.py:166-188 + tta.py:126-140).
// Everything is enqueued from C++ on one HIP stream (no per-op Python/ctypes round trip); intermediate
// tensors live in a caller-provided workspace carved by a bump arena.  Each forward is written once, as stage functions over
// weight records filled from its table in one place, and can run "dry" (no launches) to size that workspace.
#include <vector>
#include "pipeline.h"

namespace u2 {

namespace {

struct Arena {
  char* base;
  size_t cap;
  size_t off = 0, peak = 0;
  bool dry;
  Arena(void* b, size_t c, bool d) : base((char*)b), cap(c), dry(d) {}
  template <typename T>
  T* get(size_t count) {
    const size_t a = (off + 255) & ~(size_t)255;
    off = a + count * sizeof(T);
    if (off > peak) peak = off;
    if (dry) return reinterpret_cast<T*>((uintptr_t)0x1000 + a);  // never dereferenced
    return (off <= cap) ? reinterpret_cast<T*>(base + a) : nullptr;
  }
  bool ok() const { return dry || peak <= cap; }
};

// The split-K scratch registration of `st` for the duration of one module forward, the previous one restored on exit:
// what a forward computes must not depend on a registration some other caller left behind (a direct u2tok_gemm_bf16
// user, the training path) -- the split changes the summation order.  The ViT and the projector run without one.
struct ScratchScope {
  Context& cx;
  hipStream_t st;
  Scratch prev;
  bool on;
  ScratchScope(Context& c, hipStream_t s, void* p, size_t bytes, bool enable) : cx(c), st(s), prev{s, nullptr, 0}, on(enable) {
    if (!on) return;
    prev = cx.scratch_of(st);
    cx.set_scratch(st, p, bytes);
  }
  ~ScratchScope() { if (on) cx.set_scratch(st, prev.p, prev.bytes); }
};

// The run context, `r` wherever it is in scope: the arena, whether this run only sizes it (dry), the stream to enqueue on
struct Run { Arena& ar; bool dry; hipStream_t st; };
// U2_TRY: a helper that works in both modes (sizes in a dry run, launches in a real one).  U2_RUN: a launch, skipped in a dry run.
// U2_CHECK_WS: the requests so far fit the workspace.  Each returns the error from the enclosing function.
#define U2_TRY(expr) do { const int e_ = (expr); if (e_ != U2_OK) return e_; } while (0)
#define U2_RUN(expr) U2_TRY(r.dry ? U2_OK : (expr))
#define U2_CHECK_WS(ar) U2_TRY((ar).ok() ? U2_OK : U2_ERR_WORKSPACE)
inline int hip_status(hipError_t e) { return e == hipSuccess ? U2_OK : U2_ERR_LAUNCH; }
inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// A weight table as the records' fill functions read it; a dry run has none and gets null pointers.
struct Table {
  const void* const* W;
  const bf16_t* operator[](int i) const { return W ? reinterpret_cast<const bf16_t*>(W[i]) : nullptr; }
};
struct Lin { const bf16_t *w, *b; };  // weight and bias of a linear layer or a LayerNorm

// y[rows][ldy] = x[rows][ldx] @ W[out][in]^T + b  (+GELU) (+R)
static GemmDesc linear_desc(const bf16_t* x, int64_t ldx, const bf16_t* w, const bf16_t* b, bf16_t* y, int64_t ldy, int64_t rows,
                            int in, int out, int extra_flags, const bf16_t* R, int64_t ldr, int nsplit = 0, float alpha_lo = 1.f) {
  GemmDesc g;
  g.A = x; g.B = w; g.C = y; g.bias = b; g.R = R;
  g.M = (int)rows; g.N = out; g.K = in;
  g.lda = ldx; g.ldb = in; g.ldc = ldy; g.ldr = ldr;
  g.flags = (b ? GEMM_BIAS_N : 0) | extra_flags | (R ? GEMM_RESIDUAL : 0);
  g.nsplit = nsplit; g.alpha_lo = alpha_lo;  // columns [0, nsplit) scaled by alpha_lo (before the bias)
  return g;
}
// ... of dense x rows (ldx = in), R with y's leading dimension.  Both modes: nothing to size.
int linear(const Run& r, const bf16_t* x, Lin l, bf16_t* y, int64_t ldy, int64_t rows, int in, int out, int flags = 0,
           const bf16_t* R = nullptr) {
  if (r.dry) return U2_OK;
  return gemm_bf16(linear_desc(x, in, l.w, l.b, y, ldy, rows, in, out, flags, R, R ? ldy : 0), r.st);
}
// parity taps and optional outputs: n elements of src copied out (dst null: not asked for)
int tap(const Run& r, void* dst, const bf16_t* src, size_t n) {
  if (r.dry || !dst) return U2_OK;
  return hip_status(hipMemcpyAsync(dst, src, n * sizeof(bf16_t), hipMemcpyDeviceToDevice, r.st));
}
// (b, t, n) <-> (t, b, n) / [cls | patches] gathers: `count` runs of `run` elements, `dld` / `sld` elements apart
int copy_runs(const Run& r, bf16_t* dst, size_t dld, const bf16_t* src, size_t sld, size_t run, size_t count) {
  if (r.dry) return U2_OK;
  return hip_status(hipMemcpy2DAsync(dst, dld * sizeof(bf16_t), src, sld * sizeof(bf16_t), run * sizeof(bf16_t), count,
                                     hipMemcpyDeviceToDevice, r.st));
}

struct Heads { int H, d; float scale; int max_len; };  // of one forward; the bias tables have 2 max_len - 1 rows (rma.py:64-68)
struct AttnCore : AttnCall {   // equal heads, no masks; the key-split scratch (ws) comes from the arena
  bool unfused = false;  // force the GEMM chain (the ViT's debug path)
};

// softmax(Q K^T * scale + bias) V.  Reference: rma.py:60-75 / tta.py:55-61 / rope.py:82-86 (which also materialise the
// probabilities).  Default: the fused kernel of tokattn.hip (scores and probabilities never leave the registers; few
// (batch, head, 64-query) units -> key splits whose fp32 partial sums live in the arena).  Option "tok_flash" = 0, or a shape
// that kernel does not take: two batched MFMA GEMMs around fp32 scores and bf16 probabilities in HBM.
int attention_core(Run& r, const AttnCore& a) {
  Arena& ar = r.ar;
  if (!a.unfused && (r.dry || opts().tok_flash)) {
    const size_t mark = ar.off;
    AttnCall c = a;
    c.Hkv = a.H;
    c.ws_bytes = tok_attention_workspace_bytes(a.nb, a.H, a.Sq, a.Skv, a.d);
    c.ws = c.ws_bytes ? ar.get<char>(c.ws_bytes) : nullptr;
    U2_CHECK_WS(ar);
    // (a dry run sizes the arena for BOTH forms: which one a real call takes depends on pointers it does not have)
    ar.off = mark;
    if (!r.dry && tok_attention_supported(c)) return attention(c, r.st);
  }
  const size_t mark = ar.off;
  const int64_t ldS = round_up(a.Skv, 8), ldp = ldS, nz = (int64_t)a.nb * a.H;
  if (nz > 65535) return U2_ERR_ARG;
  float* S = ar.get<float>((size_t)nz * a.Sq * ldS);
  bf16_t* P = ar.get<bf16_t>((size_t)nz * a.Sq * ldp);
  // P V: V is read in place as a K-major B operand (rows = keys; GEMM_B_KMAJOR, LDS transpose reads) when the key count
  // keeps the 16-byte chunks of P whole; otherwise through a transposed copy
  const bool v_in_place = opts().kmajor_b && !(a.Skv & 7) && !(a.d & 7) && !(a.ldv & 7) && !(a.v_bs & 7) && !((uintptr_t)a.v & 15);
  bf16_t* Vt = v_in_place ? nullptr : ar.get<bf16_t>((size_t)a.nb * a.H * a.d * ldp);
  U2_CHECK_WS(ar);
  {
    GemmDesc g;
    g.A = a.q; g.B = a.k; g.C = S;
    g.M = a.Sq; g.N = a.Skv; g.K = a.d;
    g.lda = a.ldq; g.ldb = a.ldk; g.ldc = ldS;
    g.nz = (int)nz; g.nbh = a.H;
    g.sAb = a.q_bs; g.sAh = a.d; g.sBb = a.k_bs; g.sBh = a.d;
    g.sCb = (int64_t)a.H * a.Sq * ldS; g.sCh = (int64_t)a.Sq * ldS;
    g.flags = GEMM_OUT_F32;
    U2_RUN(gemm_bf16(g, r.st));
  }
  U2_RUN(softmax_rows(S, P, (int)nz, a.Sq, a.Skv, ldS, ldp, (int64_t)a.Sq * ldS, (int64_t)a.Sq * ldp, a.scale,
                      a.rel_bias, a.H, a.max_len, r.st));
  {
    GemmDesc g;
    g.A = P; g.C = a.out;
    g.M = a.Sq; g.N = a.d;
    g.lda = ldp; g.ldc = a.ldo;
    g.nz = (int)nz; g.nbh = a.H;
    g.sAb = (int64_t)a.H * a.Sq * ldp; g.sAh = (int64_t)a.Sq * ldp;
    g.sCb = a.o_bs; g.sCh = a.d;
    if (v_in_place) {
      g.B = a.v; g.K = a.Skv; g.ldb = a.ldv;
      g.sBb = a.v_bs; g.sBh = a.d;
      g.flags = GEMM_B_KMAJOR;
    } else {
      U2_RUN(transpose_bf16(a.v, Vt, a.nb, a.Skv, a.H * a.d, a.ldv, ldp, a.v_bs, (int64_t)a.H * a.d * ldp, 0, r.st));
      g.B = Vt; g.K = (int)ldp; g.ldb = ldp;
      g.sBb = (int64_t)a.H * a.d * ldp; g.sBh = (int64_t)a.d * ldp;
    }
    U2_RUN(gemm_bf16(g, r.st));
  }
  ar.off = mark;
  return U2_OK;
}

// The two call forms of attention_core.  Self: packed q | k | v rows (3 E = 3 H d wide) -> out rows of E; nb sequences of S rows,
// rows `ld` and sequences `bs` elements apart in qkv, a third of either in out.
int self_attention(Run& r, const Heads& hd, const bf16_t* qkv, bf16_t* out, int nb, int S, int64_t ld, int64_t bs,
                   const bf16_t* rel_bias, bool unfused = false) {
  const int E = hd.H * hd.d;
  AttnCore a;
  a.q = qkv; a.k = qkv + E; a.v = qkv + 2 * E; a.out = out;
  a.ldq = a.ldk = a.ldv = ld; a.q_bs = a.k_bs = a.v_bs = bs; a.ldo = ld / 3; a.o_bs = bs / 3;
  a.nb = nb; a.Sq = a.Skv = S; a.H = hd.H; a.d = hd.d; a.scale = hd.scale; a.rel_bias = rel_bias; a.max_len = hd.max_len;
  a.unfused = unfused;
  return attention_core(r, a);
}
// Cross: dense q / out rows of E, nb sequences of Sq; nb sequences of Skv key and value rows of leading dimension ldkv -- the
// halves of a packed k | v buffer (ldkv = 2 E) or two buffers (ldkv = E).  No bias table (tta.py:55-61).
int cross_attention(Run& r, const Heads& hd, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ldkv, bf16_t* out, int nb,
                    int Sq, int Skv) {
  const int E = hd.H * hd.d;
  AttnCore a;
  a.q = q; a.k = k; a.v = v; a.out = out;
  a.ldq = a.ldo = E; a.ldk = a.ldv = ldkv; a.q_bs = a.o_bs = (int64_t)Sq * E; a.k_bs = a.v_bs = (int64_t)Skv * ldkv;
  a.nb = nb; a.Sq = Sq; a.Skv = Skv; a.H = hd.H; a.d = hd.d; a.scale = hd.scale;
  return attention_core(r, a);
}

// attention over the CHUNK axis of rows laid out (b, t, n) [leading dim 3E for q | k | v, E for the output]: Bx * Nx * H
// independent sequences of Tx rows that are Nx rows apart (svr.py:31-36 without its two permute().contiguous() copies).
// Tx <= 16 and a head dim the wave kernel is built for: one launch; otherwise the batched-GEMM core, one batch entry
// at a time (sequence rows are Nx * 3E elements apart, the Nx positions and H heads are the GEMM batch).
int chunk_axis_attention(Run& r, const Heads& hd, const bf16_t* qkv, bf16_t* out, int Bx, int Tx, int Nx, const bf16_t* rel_bias) {
  const int d = hd.d, E = hd.H * d;
  if (Tx <= 16 && (d == 64 || d == 128 || d == 256 || d == 384 || d == 512))
    return r.dry ? U2_OK
                 : temporal_attention(qkv, qkv + E, qkv + 2 * E, out, Bx, Tx, Nx, hd.H, d, 3 * E, E, hd.scale, rel_bias, hd.max_len, r.st);
  for (int b = 0; b < Bx; ++b)
    U2_TRY(self_attention(r, hd, qkv + (int64_t)b * Tx * Nx * 3 * E, out + (int64_t)b * Tx * Nx * E, Nx, Tx, (int64_t)Nx * 3 * E,
                          3 * E, rel_bias));
  return U2_OK;
}

// =========================================================================== ViT3DTower
struct VitBlock { Lin norm1; const bf16_t* wqkv; Lin out, norm2, fc1, fc2; };  // (the SABlock qkv projection has no bias)
struct VitWeights { const bf16_t *pos, *cls; Lin patch, norm; std::vector<VitBlock> blocks; };
// The ViT weight table (include/u2tok.h, "ViT weight table"): read here and nowhere else
VitWeights vit_weights(const VitConfig& c, Table t) {
  VitWeights w{t[0], t[3], {t[1], t[2]}, {t[4 + 11 * c.depth], t[5 + 11 * c.depth]}, {}};
  for (int l = 0, i = 4; l < c.depth; ++l, i += 11)
    w.blocks.push_back({{t[i], t[i + 1]}, t[i + 2], {t[i + 3], t[i + 4]}, {t[i + 5], t[i + 6]}, {t[i + 7], t[i + 8]}, {t[i + 9], t[i + 10]}});
  return w;
}

struct Vit {  // one ViT forward: geometry, buffers and the stages that are not in line in vit_forward
  const VitConfig& c; Run r;
  int nc, ntok, S, S_pad, Hd;
  int64_t prow, rows;  // patch rows; cls row of chunk b is row prow + b
  Heads hd;
  bf16_t *x, *xn, *qkv, *att, *vt, *h1;

  // unfused reference attention (debug option "vit_flash" = 0): gather [cls | patches] per chunk, two GEMMs + softmax
  int unfused_attention() {
    const size_t mark = r.ar.off;
    bf16_t* qc = r.ar.get<bf16_t>((size_t)rows * 3 * Hd);
    bf16_t* ac = r.ar.get<bf16_t>((size_t)rows * Hd);
    U2_CHECK_WS(r.ar);
    const size_t rq = (size_t)3 * Hd;  // a q | k | v row
    U2_TRY(copy_runs(r, qc + rq, S * rq, qkv, ntok * rq, ntok * rq, nc));
    U2_TRY(copy_runs(r, qc, S * rq, qkv + prow * rq, rq, rq, nc));
    U2_TRY(self_attention(r, hd, qc, ac, nc, S, rq, (int64_t)S * rq, nullptr, true));
    U2_TRY(copy_runs(r, att, (size_t)ntok * Hd, ac + Hd, (size_t)S * Hd, (size_t)ntok * Hd, nc));
    U2_TRY(copy_runs(r, att + prow * Hd, Hd, ac, (size_t)S * Hd, Hd, nc));
    r.ar.off = mark;
    return U2_OK;
  }

  // One MONAI TransformerBlock / SABlock on the residual stream x
  int block(const VitBlock& w) {
    // x = x + out_proj(attn(qkv(norm1(x))))
    U2_RUN(layernorm_dense(x, nullptr, w.norm1.w, w.norm1.b, xn, (int)rows, Hd, c.ln_eps, r.st));
    // the double pipeline reads q already multiplied by softmax scale * log2 e: the product scales its q columns from the
    // fp32 accumulator (one rounding, as for the unscaled q of vit.py:100-105; the SABlock qkv projection has no bias)
    const bool q_pre = opts().vit_flash && ntok >= 512 && (opts().flash_mode == 0 || opts().flash_mode == 7);
    // ... and, where the 256 x 192 deep form runs the product (round 5), the V tiles leave V^T for the flash kernel themselves:
    // their K loop runs with the MFMA operands exchanged and the transposed accumulators are stored in that operand's key order
    // (gemm_bt.hip: vt_epilogue) -- no row-major V of the patch rows, no transpose launch (12 per volume).  Same values, bit for bit.
    GemmDesc gq = linear_desc(xn, Hd, w.wqkv, nullptr, qkv, 3 * Hd, rows, Hd, 3 * Hd, 0, nullptr, 0, q_pre ? Hd : 0,
                              hd.scale * 1.44269504088896340736f);
    const bool vt_fused = opts().vit_flash && opts().vit_vt_epilogue && S_pad == ntok && gemm_vt_supported(gq, 2 * Hd, ntok);
    if (vt_fused) {
      gq.vt = vt; gq.vt_n0 = 2 * Hd; gq.vt_rows = ntok; gq.vt_ld = S_pad; gq.vt_bs = (int64_t)Hd * S_pad;
    }
    U2_RUN(gemm_bf16(gq, r.st));
    if (opts().vit_flash) {
      if (!vt_fused)
        U2_RUN(transpose_bf16(qkv + 2 * Hd, vt, nc, ntok, Hd, 3 * Hd, S_pad, (int64_t)ntok * 3 * Hd, (int64_t)Hd * S_pad, 1, r.st));
      const bf16_t* xq = qkv + prow * 3 * Hd;  // q | k | v of the cls rows
      U2_RUN(flash_attention_d64(qkv, qkv + Hd, vt, att, nc, ntok, hd.H, 3 * Hd, (int64_t)ntok * 3 * Hd, Hd,
                                 (int64_t)ntok * Hd, S_pad, hd.scale, xq, xq + Hd, xq + 2 * Hd, att + prow * Hd, 3 * Hd, Hd,
                                 1, nullptr, 0, r.st, q_pre ? 1 : 0));
    } else {
      U2_TRY(unfused_attention());
    }
    U2_TRY(linear(r, att, w.out, x, Hd, rows, Hd, Hd, 0, x));
    // x = x + linear2(gelu(linear1(norm2(x))))
    U2_RUN(layernorm_dense(x, nullptr, w.norm2.w, w.norm2.b, xn, (int)rows, Hd, c.ln_eps, r.st));
    U2_TRY(linear(r, xn, w.fc1, h1, c.mlp_dim, rows, Hd, c.mlp_dim, GEMM_GELU));
    return linear(r, h1, w.fc2, x, Hd, rows, c.mlp_dim, Hd, 0, x);
  }
};

}  // namespace

// Row layout of the residual stream: the nc * ntok PATCH rows first (chunk-major), then the nc cls rows.  The
// reference keeps [cls | patches] per chunk (vit.py:116-118); a transformer is indifferent to the order rows are
// stored in, and this one makes every GEMM see M = nc*ntok (+ nc), the patch rows of a chunk tile exactly into
// 128 / 256-row attention units, and the final "drop the cls token" (vit.py:157-160) a no-op.
int vit_forward(const VitConfig& c, const void* const* W, const void* volume, bf16_t* out, void* ws, size_t ws_bytes,
                bool dry, size_t* peak, hipStream_t st) {
  if (c.nchunk <= 0 || c.depth < 0 || c.heads <= 0 || c.hidden != c.heads * 64) return U2_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if (c.img[i] <= 0 || c.patch[i] <= 0 || c.img[i] % c.patch[i]) return U2_ERR_ARG;
  if (!dry && (!W || !volume || !out)) return U2_ERR_ARG;
  const int nh = c.img[0] / c.patch[0], nw = c.img[1] / c.patch[1], nd = c.img[2] / c.patch[2];
  const int ntok = nh * nw * nd, S = ntok + 1, Hd = c.hidden, Kp = c.patch[0] * c.patch[1] * c.patch[2], nc = c.nchunk;
  const int64_t prow = (int64_t)nc * ntok, rows = prow + nc;
  const VitWeights w = vit_weights(c, Table{dry ? nullptr : W});

  ScratchScope scratch_scope(ctx(), st, nullptr, 0, !dry);
  Arena ar(ws, ws_bytes, dry);
  Vit v{c, Run{ar, dry, st}, nc, ntok, S, (int)round_up(ntok, 64), Hd, prow, rows, Heads{c.heads, 64, 1.0f / sqrtf(64.0f), 0}};
  const Run& r = v.r;
  bf16_t* x = v.x = ar.get<bf16_t>((size_t)rows * Hd);
  v.xn = ar.get<bf16_t>((size_t)rows * Hd);
  v.qkv = ar.get<bf16_t>((size_t)rows * 3 * Hd);
  v.att = ar.get<bf16_t>((size_t)rows * Hd);
  v.vt = ar.get<bf16_t>((size_t)nc * Hd * v.S_pad);
  // patches (only needed for the embedding) and the MLP hidden share one region
  bf16_t* patches = v.h1 = ar.get<bf16_t>(std::max((size_t)nc * ntok * Kp, (size_t)rows * c.mlp_dim));
  U2_CHECK_WS(ar);

  // ---- patch embedding: im2col + Linear + position embedding; cls token rows appended (vit.py:115-118)
  U2_RUN(im2col_patches(volume, c.vol_dtype, patches, nc, c.img[0], c.img[1], c.img[2], c.patch[0], c.patch[1],
                        c.patch[2], st));
  U2_RUN(fill_rows(w.cls, x + prow * Hd, nc, Hd, Hd, st));
  GemmDesc g = linear_desc(patches, Kp, w.patch.w, w.patch.b, x, Hd, ntok, Kp, Hd, 0, w.pos, Hd);  // per chunk: + the same positions
  g.nz = nc; g.sAb = (int64_t)ntok * Kp; g.sCb = (int64_t)ntok * Hd;
  U2_RUN(gemm_bf16(g, st));
  for (const VitBlock& b : w.blocks) U2_TRY(v.block(b));
  // final norm; the cls rows are dropped unless select_feature == "cls_patch" (vit.py:124,157-160), in which case
  // the output goes back to the reference's [cls | patches] order per chunk
  if (c.keep_cls) {
    U2_RUN(layernorm_bf16(x, nullptr, w.norm.w, w.norm.b, out + Hd, nc, ntok, Hd, (int64_t)ntok * Hd, Hd, 0, 0,
                          (int64_t)S * Hd, Hd, c.ln_eps, st));
    U2_RUN(layernorm_bf16(x + prow * Hd, nullptr, w.norm.w, w.norm.b, out, nc, 1, Hd, Hd, Hd, 0, 0, (int64_t)S * Hd, Hd,
                          c.ln_eps, st));
  } else {
    U2_RUN(layernorm_dense(x, nullptr, w.norm.w, w.norm.b, out, (int)prow, Hd, c.ln_eps, st));
  }
  if (peak) *peak = ar.peak;
  U2_CHECK_WS(ar);
  return U2_OK;
}

// =========================================================================== SpatialPoolingProjector
// (weight table: layer l's weight and bias at 2 l, 2 l + 1 -- include/u2tok.h, "SPP weight table")
int spp_forward(const SppConfig& c, const void* const* W, const bf16_t* x, bf16_t* out, void* ws, size_t ws_bytes,
                bool dry, size_t* peak, hipStream_t st) {
  if (c.nchunk <= 0 || c.pooling_size <= 0 || c.layer_num <= 0 || c.in_dim <= 0 || c.out_dim <= 0) return U2_ERR_ARG;
  if (!dry && (!W || !x || !out)) return U2_ERR_ARG;
  const int ps = c.pooling_size;
  int g1 = c.grid[0], g2 = c.grid[1], g3 = c.grid[2], w1 = ps, w2 = ps, w3 = ps;
  if (c.pooling_type == 1) { g3 = g1 * g2 * g3; g1 = g2 = 1; w1 = w2 = 1; w3 = ps * ps * ps; }
  else if (c.pooling_type != 0) return U2_ERR_ARG;
  if (g1 < w1 || g2 < w2 || g3 < w3) return U2_ERR_ARG;
  const int np = (g1 / w1) * (g2 / w2) * (g3 / w3);
  const int64_t rows = (int64_t)c.nchunk * np;
  const Table w{dry ? nullptr : W};
  ScratchScope scratch_scope(ctx(), st, nullptr, 0, !dry);
  Arena ar(ws, ws_bytes, dry);
  const Run r{ar, dry, st};
  bf16_t* pooled = ar.get<bf16_t>((size_t)rows * c.in_dim);
  bf16_t* ha = ar.get<bf16_t>((size_t)rows * c.out_dim);
  bf16_t* hb = ar.get<bf16_t>((size_t)rows * c.out_dim);
  U2_CHECK_WS(ar);
  U2_RUN(avgpool3d_tokens(x, pooled, c.nchunk, g1, g2, g3, w1, w2, w3, c.in_dim, st));
  const bf16_t* cur = pooled;
  int cur_dim = c.in_dim;
  for (int l = 0; l < c.layer_num; ++l) {
    const bool last = (l == c.layer_num - 1);
    bf16_t* dst = last ? out : ((l & 1) ? hb : ha);
    U2_TRY(linear(r, cur, {w[2 * l], w[2 * l + 1]}, dst, c.out_dim, rows, cur_dim, c.out_dim,
                  (!last && c.layer_type == 0) ? GEMM_GELU : 0));
    cur = dst;
    cur_dim = c.out_dim;
  }
  if (peak) *peak = ar.peak;
  return U2_OK;
}

// =========================================================================== u2Tokenizer
namespace {
struct Att { Lin q, k, v, o; const bf16_t* rb; };  // an attention module's projections and its relative-bias table (null: none)
// fold: the packed q | k | v projection applied to the output projection of the attention BEFORE this one (svr_fold_build);
// null: not folded, that output projection runs
struct SvrAtt : Att { Lin fold; };
struct SvrLayer { SvrAtt spatial, temporal; };
struct TtaLayer { Att self, visual, text; Lin norm_self, norm_v, norm_t; };
struct TokWeights {
  const bf16_t* query;
  Lin score, gate;  // token_selection.score_net; dynamic_pool.gate_fc (null when !enable_dmtp)
  Att linagg;       // (wv / dense are in the table but never read: tta.py:47-48,62-65)
  std::vector<SvrLayer> svr;  // per layer
  std::vector<TtaLayer> tta;
};
// n projections of one input lie back to back in HBM, weights and biases (tokenizer.py: pack_weights)
bool packed(const Lin* l, int n, int E) {
  bool p = l[0].w && l[0].b;
  for (int i = 1; i < n; ++i) p = p && l[i].w == l[i - 1].w + (size_t)E * E && l[i].b == l[i - 1].b + E;
  return p;
}
// The tokenizer weight table (include/u2tok.h, "Tokenizer weight table"): read here and nowhere else.  Only the self attentions of
// attn_type rma have a bias table; whatever the table holds in that slot of any other attention is dropped here.  The fold slots
// behind the table are read only when `folds`; a slot is taken when both its pointers are there and its attention's q | k | v is packed.
TokWeights tok_weights(const TokConfig& c, Table t, bool folds) {
  auto att = [&](int i, bool self) {
    return Att{{t[i], t[i + 1]}, {t[i + 2], t[i + 3]}, {t[i + 4], t[i + 5]}, {t[i + 6], t[i + 7]}, self && c.attn_type == 0 ? t[i + 8] : nullptr};
  };
  const int L = c.num_layers, i_sel = 1 + 18 * L, i_tta = i_sel + 4, i_lin = i_tta + 33 * L, i_fold = U2TOK_TOK_NW(L);
  // SVR attention j = 2 l (spatial) / 2 l + 1 (temporal) of the chain; fold slot j - 1 holds its (W', b')
  auto svr_att = [&](int i, int j) {
    SvrAtt a{att(i, true), {nullptr, nullptr}};
    const Lin qkv[3] = {a.q, a.k, a.v};
    if (folds && j > 0 && t[i_fold + 2 * (j - 1)] && t[i_fold + 2 * (j - 1) + 1] && packed(qkv, 3, c.E))
      a.fold = {t[i_fold + 2 * (j - 1)], t[i_fold + 2 * (j - 1) + 1]};
    return a;
  };
  TokWeights w{t[0], {t[i_sel], t[i_sel + 1]}, {nullptr, nullptr}, att(i_lin, false), {}, {}};
  if (c.enable_dmtp) w.gate = {t[i_sel + 2], t[i_sel + 3]};
  for (int l = 0, i = 1; l < L; ++l, i += 18) w.svr.push_back({svr_att(i, 2 * l), svr_att(i + 9, 2 * l + 1)});
  for (int l = 0, i = i_tta; l < L; ++l, i += 33)
    w.tta.push_back({att(i, true), att(i + 9, false), att(i + 18, false), {t[i + 27], t[i + 28]}, {t[i + 29], t[i + 30]}, {t[i + 31], t[i + 32]}});
  return w;
}

// The host module packs wq | wk | wv (and their biases) back to back in HBM (tokenizer.py: pack_weights); when it
// did, the three projections of one input are ONE GEMM with N = 3E (2E for the k | v pair of a cross attention):
// the activation panel is read once and the launch fills the machine 3x better at small M.  (A dry run's nulls are not packed.)
// out[rows][n E] = x W^T + b for the n projections p: {q, k, v} or {k, v} of one attention
int packed_proj(const Run& r, const bf16_t* x, std::initializer_list<Lin> p, bf16_t* out, int64_t rows, int E) {
  const Lin* l = p.begin(); const int n = (int)p.size();
  if (packed(l, n, E)) return linear(r, x, l[0], out, n * E, rows, E, n * E);
  for (int i = 0; i < n; ++i) U2_TRY(linear(r, x, l[i], out + i * E, n * E, rows, E, E));
  return U2_OK;
}
// q and k of packed q | k | v rows indexed (outer, s, inner) rotated in place, position = s
int rope_qk(const Run& r, const Heads& hd, bf16_t* qkv, int64_t n_outer, int S, int n_inner) {
  const int E = hd.H * hd.d;
  U2_RUN(rope_apply(qkv, n_outer, S, n_inner, hd.H, hd.d, 3 * E, hd.max_len, 0, r.st));
  U2_RUN(rope_apply(qkv + E, n_outer, S, n_inner, hd.H, hd.d, 3 * E, hd.max_len, 0, r.st));
  return U2_OK;
}
template <typename P> inline P* slot(P* const* per_layer, int l) { return per_layer ? per_layer[l] : nullptr; }

struct Tok {  // one tokenizer forward: what its stages share, and the stages in the order tokenizer_forward calls them
  const TokConfig& c; Run r; const TokWeights& w;
  TokTaps taps;  // (all null without taps and in a dry run)
  const bf16_t* t_token;
  int B, T, N, E, L, Q, k;
  Heads hd;
  int64_t rows, qrows;                // B * T * N visual rows, B * Q query rows
  bf16_t *xa, *xb, *qkv, *sctx;       // SVR: ping-pong token buffers, packed q | k | v, attention context
  bool x_ctx = false;                 // SVR: x is an attention's context, its output projection folded into the next q | k | v
  const bf16_t* V; int Lv;            // the Lv visual tokens per batch entry the aggregation attends to
  bf16_t *qa, *qb, *qc, *qproj, *qctx, *qo;  // TTA: query ping-pong (+ qc), projections, context, sub-layer output
  // k | v of the two cross attentions of every layer: one buffer each, filled on the side stream (or kv_inline, in line)
  SideStream* side; bool overlap;
  bf16_t *kv_inline, *kv_v[8], *kv_t[8], *k_lin;  // k_lin: key projection of the final linear aggregation

  // attn_type 2 with B > 1, temporal: the sequence is the B*N (batch, token) pairs of one chunk index: gather rows (b, t, n) ->
  // (t, b, n), attend, scatter into actx
  int temporal_across_batch(bf16_t* actx) {
    const size_t mark = r.ar.off;
    bf16_t* g = r.ar.get<bf16_t>((size_t)rows * 3 * E);
    bf16_t* gc = r.ar.get<bf16_t>((size_t)rows * E);
    U2_CHECK_WS(r.ar);
    const size_t S2 = (size_t)B * N;
    for (int b = 0; b < B; ++b)
      U2_TRY(copy_runs(r, g + (size_t)b * N * 3 * E, S2 * 3 * E, qkv + (size_t)b * T * N * 3 * E, (size_t)N * 3 * E, (size_t)N * 3 * E, T));
    U2_TRY(self_attention(r, hd, g, gc, T, (int)S2, 3 * E, (int64_t)S2 * 3 * E, nullptr));
    for (int b = 0; b < B; ++b)
      U2_TRY(copy_runs(r, actx + (size_t)b * T * N * E, (size_t)N * E, gc + (size_t)b * N * E, S2 * E, (size_t)N * E, T));
    r.ar.off = mark;
    return U2_OK;
  }

  // The SVR stack is a chain of 2 L attentions with nothing between them (svr.py:23-40,50-62): the output projection of one is
  // followed directly by the packed q | k | v projection of the next, a Linear applied to a Linear.  Where the next attention has its
  // fold (W' = W_qkv W_o, b' = W_qkv b_o + b_qkv: SvrAtt::fold), the output projection is skipped and x stays that attention's
  // CONTEXT (x_ctx) for the folded projection to read: one E x E product per attention less.  The last attention's always runs.
  // q | k | v of attention a from x
  int svr_qkv(const SvrAtt& a, const bf16_t* x) {
    if (x_ctx) return linear(r, x, a.fold, qkv, 3 * E, rows, E, 3 * E);
    return packed_proj(r, x, {a.q, a.k, a.v}, qkv, rows, E);
  }
  // where attention a's context goes: sctx, or xa when x (which the projection before it reads) is sctx itself
  bf16_t* svr_ctx(const bf16_t* x) const { return x == sctx ? xa : sctx; }
  // x = the output projection of attention a's context actx (into xa / xb, whichever neither x nor actx is), or actx itself when the
  // attention `next` folds the projection
  int svr_project(const SvrAtt& a, const SvrAtt* next, bf16_t* actx, const bf16_t*& x) {
    x_ctx = next && next->fold.w;
    if (x_ctx) { x = actx; return U2_OK; }
    bf16_t* y = (x == xa || actx == xa) ? xb : xa;
    U2_TRY(linear(r, actx, a.o, y, E, rows, E, E));
    x = y;
    return U2_OK;
  }

  // ---------------- SVR layer l (svr.py:23-40,50-62): x = temporal(spatial(x)), no residual / norm.  x: the layer's input, then its
  // output.  attn_type 2 = nn.MultiheadAttention read sequence-first (svr.py:16-18,28-35): attention runs across whatever sits
  // in dim 0, INCLUDING the batch entries: "spatial" = across the B*T (batch, chunk) pairs at a token position,
  // "temporal" = across the B*N (batch, token) pairs of a chunk index.
  int svr_layer(int l, const bf16_t*& x) {
    const SvrLayer& a = w.svr[l];
    if (const void* in = slot(taps.svr_in, l)) x = reinterpret_cast<const bf16_t*>(in);  // (a call with SVR taps has no folds)
    // spatial: sequences of N tokens inside each chunk (svr.py:27-30)
    bf16_t* actx = svr_ctx(x);
    U2_TRY(svr_qkv(a.spatial, x));
    if (c.attn_type == 1) U2_TRY(rope_qk(r, hd, qkv, (int64_t)B * T, N, 1));
    if (c.attn_type == 2)  // sequence = the B*T (batch, chunk) pairs, batch = token position
      U2_TRY(chunk_axis_attention(r, hd, qkv, actx, 1, B * T, N, a.spatial.rb));
    else
      U2_TRY(self_attention(r, hd, qkv, actx, B * T, N, 3 * E, (int64_t)N * 3 * E, a.spatial.rb));
    U2_TRY(svr_project(a.spatial, &a.temporal, actx, x));
    // temporal: sequences of T chunks at each token position (svr.py:32-36); rows stay in (b t n) order
    actx = svr_ctx(x);
    U2_TRY(svr_qkv(a.temporal, x));
    if (c.attn_type == 1) U2_TRY(rope_qk(r, hd, qkv, B, T, N));
    if (c.attn_type == 2 && B == 1)  // sequence = the N tokens of a chunk, batch = chunk
      U2_TRY(self_attention(r, hd, qkv, actx, T, N, 3 * E, (int64_t)N * 3 * E, a.temporal.rb));
    else if (c.attn_type == 2)
      U2_TRY(temporal_across_batch(actx));
    else
      U2_TRY(chunk_axis_attention(r, hd, qkv, actx, B, T, N, a.temporal.rb));
    U2_TRY(svr_project(a.temporal, l + 1 < L ? &w.svr[l + 1].spatial : nullptr, actx, x));
    return tap(r, slot(taps.svr_out, l), x, (size_t)rows * E);
  }

  // ---------------- token selection (svr.py:171): x -> sel (B, k, E)
  // DifferentiableTokenSelection (svr.py:101-117): weights = softmax_tokens(score_net(x)/tau); out = W^T X.
  // Computed operand-swapped so the scores land transposed: scT[r][tok] = score_w[r] . x[tok] + b[r].
  int select_diffts(const bf16_t* x, bf16_t* sel) {
    const int TN = T * N;
    const size_t mark = r.ar.off;
    const int64_t ldS = round_up(TN, 8);
    float* scT = r.ar.get<float>((size_t)B * k * ldS);
    bf16_t* P = r.ar.get<bf16_t>((size_t)B * k * ldS);
    const bool x_in_place = opts().kmajor_b && !(TN & 7);  // the aggregation reads X as a K-major B operand (rows = tokens)
    bf16_t* Xt = x_in_place ? nullptr : r.ar.get<bf16_t>((size_t)B * E * ldS);
    U2_CHECK_WS(r.ar);
    {
      GemmDesc g;
      g.A = w.score.w; g.B = x; g.C = scT; g.bias = w.score.b;
      g.M = k; g.N = TN; g.K = E; g.lda = E; g.ldb = E; g.ldc = ldS;
      g.nz = B; g.sBb = (int64_t)TN * E; g.sCb = (int64_t)k * ldS;
      g.flags = GEMM_BIAS_M | GEMM_OUT_F32;
      U2_RUN(gemm_bf16(g, r.st));
    }
    U2_RUN(softmax_rows(scT, P, B, k, TN, ldS, ldS, (int64_t)k * ldS, (int64_t)k * ldS, 1.0f / c.diffts_tau, nullptr, 1, 0, r.st));
    {
      GemmDesc g;
      g.A = P; g.C = sel;
      g.M = k; g.N = E; g.lda = ldS; g.ldc = E;
      g.nz = B; g.sAb = (int64_t)k * ldS; g.sCb = (int64_t)k * E;
      if (x_in_place) {
        g.B = x; g.K = TN; g.ldb = E; g.sBb = (int64_t)TN * E;
        g.flags = GEMM_B_KMAJOR;
      } else {
        U2_RUN(transpose_bf16(x, Xt, B, TN, E, E, ldS, (int64_t)TN * E, (int64_t)E * ldS, 0, r.st));
        g.B = Xt; g.K = (int)ldS; g.ldb = ldS; g.sBb = (int64_t)E * ldS;
      }
      U2_RUN(gemm_bf16(g, r.st));
    }
    r.ar.off = mark;
    return U2_OK;
  }
  // TokenSelection (svr.py:75-91): hard top-k over the flattened (t n) axis, sorted by score
  int select_topk(const bf16_t* x, bf16_t* sel, int64_t* topk_idx_out) {
    const size_t mark = r.ar.off;
    float* scores = r.ar.get<float>((size_t)rows);
    int64_t* idx = topk_idx_out ? topk_idx_out : r.ar.get<int64_t>((size_t)B * k);
    U2_CHECK_WS(r.ar);
    U2_RUN(score_gemv(x, w.score.w, w.score.b, scores, (int)rows, E, r.st));
    U2_RUN(topk_sorted(scores, idx, B, T * N, k, r.st));
    U2_RUN(gather_rows(x, idx, sel, B, T * N, k, E, r.st));
    r.ar.off = mark;
    return U2_OK;
  }

  // ---------------- multi-scale pooling (svr.py:173-184): sel -> V, Lv
  int multiscale_pooling(const bf16_t* sel) {
    V = sel, Lv = k;
    if (c.use_multi_scale) {
      Lv = k + k / 2 + k / 4;
      bf16_t* pooled = r.ar.get<bf16_t>((size_t)B * Lv * E);
      float* gws = r.ar.get<float>((size_t)B * 3 * 16 * cdiv(E, 256));
      U2_CHECK_WS(r.ar);
      U2_RUN(multiscale_pool(sel, pooled, B, k, E, w.gate.w, w.gate.b, gws, r.st));
      V = pooled;
    }
    // parity taps: the visual tokens the aggregation stage attends to
    U2_TRY(tap(r, taps.visual_out, V, (size_t)B * Lv * E));
    if (taps.visual_in) V = reinterpret_cast<const bf16_t*>(taps.visual_in);
    return U2_OK;
  }

  // ---------------- the TTA's buffers, and the side-stream prefetch of what depends on V and t_token alone: k | v of the two cross
  // attentions of every layer and the aggregation's keys (at most 7 layers: a SideStream has 16 events)
  int tta_prefetch() {
    qa = r.ar.get<bf16_t>((size_t)qrows * E);
    qb = r.ar.get<bf16_t>((size_t)qrows * E);
    qc = r.ar.get<bf16_t>((size_t)qrows * E);
    qproj = r.ar.get<bf16_t>((size_t)qrows * 3 * E);
    qctx = r.ar.get<bf16_t>((size_t)qrows * E);
    qo = r.ar.get<bf16_t>((size_t)qrows * E);
    side = (!r.dry && opts().tta_overlap && L > 0 && L <= 7) ? ctx().side_for(r.st) : nullptr;
    overlap = r.dry ? (L > 0 && L <= 7) : side != nullptr;  // dry: size for the larger (overlapped) layout
    kv_inline = overlap ? nullptr : r.ar.get<bf16_t>((size_t)B * std::max(Lv, c.Lt) * 2 * E);
    if (overlap)
      for (int l = 0; l < L; ++l) {
        kv_v[l] = r.ar.get<bf16_t>((size_t)B * Lv * 2 * E);
        kv_t[l] = r.ar.get<bf16_t>((size_t)B * c.Lt * 2 * E);
      }
    k_lin = r.ar.get<bf16_t>((size_t)B * Lv * E);
    U2_CHECK_WS(r.ar);
    if (!overlap || r.dry) return U2_OK;
    const Run rs{r.ar, false, side->s};
    // fork: everything `st` has enqueued so far (V and t_token are final) precedes the side stream's work
    U2_TRY(hip_status(hipEventRecord(side->fork, r.st)));
    U2_TRY(hip_status(hipStreamWaitEvent(side->s, side->fork, 0)));
    for (int l = 0; l < L; ++l) {
      U2_TRY(packed_proj(rs, V, {w.tta[l].visual.k, w.tta[l].visual.v}, kv_v[l], (int64_t)B * Lv, E));
      U2_TRY(hip_status(hipEventRecord(side->done[2 * l], side->s)));
      U2_TRY(packed_proj(rs, t_token, {w.tta[l].text.k, w.tta[l].text.v}, kv_t[l], (int64_t)B * c.Lt, E));
      U2_TRY(hip_status(hipEventRecord(side->done[2 * l + 1], side->s)));
    }
    U2_TRY(linear(rs, V, w.linagg.k, k_lin, E, (int64_t)B * Lv, E, E));
    return hip_status(hipEventRecord(side->done[2 * L], side->s));
  }

  // MultiHeadCrossAttention.forward (tta.py:42-69), is_compress = False: dst = dense(attn(wq qin, k | v of the Ls rows of src)).
  // Prefetched: k | v are in kv once side-stream event `ready` has fired; otherwise they are computed into kv here.
  int cross(const Att& a, const bf16_t* src, int Ls, const bf16_t* qin, bf16_t* dst, bf16_t* kv, int ready) {
    U2_TRY(linear(r, qin, a.q, qproj, E, qrows, E, E));
    if (overlap)
      U2_RUN(hip_status(hipStreamWaitEvent(r.st, side->done[ready], 0)));
    else
      U2_TRY(packed_proj(r, src, {a.k, a.v}, kv, (int64_t)B * Ls, E));
    U2_TRY(cross_attention(r, hd, qproj, kv, kv + E, 2 * E, qctx, B, Q, Ls));
    return linear(r, qctx, a.o, dst, E, qrows, E, E);
  }

  // ---------------- TTA layer l (tta.py:93-107): three post-LN residual sub-layers on the query tokens.  qcur: input, then output.
  int tta_layer(int l, bf16_t*& qcur) {
    const TtaLayer& a = w.tta[l];
    if (const void* in = slot(taps.tta_in, l)) qcur = (bf16_t*)in;  // (only ever read)
    bf16_t* s1 = (qcur == qa) ? qb : qa;
    // self attention on the query tokens + post-LN residual (tta.py:94-96)
    if (c.attn_type == 2 && B == 1) {
      // (B = 1, Q, E) read sequence-first: every query token is a batch entry with a sequence of ONE key, whose
      // softmax weight is exactly 1 -> the context is the value projection itself (tta.py:84,94)
      U2_TRY(linear(r, qcur, a.self.v, qctx, E, qrows, E, E));
    } else {
      U2_TRY(packed_proj(r, qcur, {a.self.q, a.self.k, a.self.v}, qproj, qrows, E));
      if (c.attn_type == 1) U2_TRY(rope_qk(r, hd, qproj, B, Q, 1));
      if (c.attn_type == 2)  // (B, Q, E) read sequence-first: the sequence is the B batch entries of one query index
        U2_TRY(chunk_axis_attention(r, hd, qproj, qctx, 1, B, Q, a.self.rb));
      else
        U2_TRY(self_attention(r, hd, qproj, qctx, B, Q, 3 * E, (int64_t)Q * 3 * E, a.self.rb));
    }
    U2_TRY(linear(r, qctx, a.self.o, qo, E, qrows, E, E));
    U2_RUN(layernorm_dense(qcur, qo, a.norm_self.w, a.norm_self.b, s1, (int)qrows, E, c.ln_eps, r.st));
    // visual cross attention (tta.py:97-100)
    U2_TRY(cross(a.visual, V, Lv, s1, qo, overlap ? kv_v[l] : kv_inline, 2 * l));
    U2_RUN(layernorm_dense(s1, qo, a.norm_v.w, a.norm_v.b, qc, (int)qrows, E, c.ln_eps, r.st));
    // text cross attention (tta.py:101-103) -- no padding mask in the reference
    U2_TRY(cross(a.text, t_token, c.Lt, qc, qo, overlap ? kv_t[l] : kv_inline, 2 * l + 1));
    U2_RUN(layernorm_dense(qc, qo, a.norm_t.w, a.norm_t.b, s1, (int)qrows, E, c.ln_eps, r.st));
    qcur = s1;
    return tap(r, slot(taps.tta_out, l), qcur, (size_t)qrows * E);
  }

  // ---------------- LinearAggregation (tta.py:109-116): is_compress=True -> V un-projected, no out-proj
  int linear_aggregation(const bf16_t* qcur, bf16_t* out) {
    U2_TRY(linear(r, qcur, w.linagg.q, qproj, E, qrows, E, E));
    if (overlap)
      U2_RUN(hip_status(hipStreamWaitEvent(r.st, side->done[2 * L], 0)));
    else
      U2_TRY(linear(r, V, w.linagg.k, k_lin, E, (int64_t)B * Lv, E, E));
    return cross_attention(r, hd, qproj, k_lin, V, E, out, B, Q, Lv);
  }
};
}  // namespace

int tokenizer_forward(const TokConfig& c, const void* const* W, const bf16_t* v_token, const bf16_t* t_token,
                      bf16_t* out, int64_t* topk_idx_out, bf16_t* svr_out, const TokTaps* taps, void* ws, size_t ws_bytes,
                      bool dry, size_t* peak, hipStream_t st) {
  if (c.B <= 0 || c.T <= 0 || c.N <= 0 || c.E <= 0 || c.Lt <= 0 || c.num_heads <= 0 || c.num_layers < 0) return U2_ERR_ARG;
  if (c.E % c.num_heads || (c.E / c.num_heads) % 8 || c.top_k <= 0 || c.num_query <= 0) return U2_ERR_ARG;
  if (c.attn_type < 0 || c.attn_type > 2) return U2_ERR_ARG;
  if (!dry && (!W || !v_token || !t_token || !out)) return U2_ERR_ARG;
  const int B = c.B, E = c.E, d = E / c.num_heads, L = c.num_layers, k = c.top_k;
  if (!c.enable_diffts && k > c.T * c.N) return U2_ERR_ARG;                     // torch.topk would raise
  if (c.N > c.max_seq_len || c.T > c.max_seq_len || c.num_query > c.max_seq_len) return U2_ERR_ARG;  // rma.py:64-68 index range
  // The SVR folds are for calls that ask for the aligned tokens alone.  A call that asks for an SVR intermediate (the refined tokens,
  // an SVR tap) is parity instrumentation: it runs projection by projection, at the reference's rounding points, and does not read
  // the fold slots at all.  (The TTA / visual taps sit behind the stack and do not look into it.)
  bool folds = !dry && opts().svr_fold && !svr_out;
  for (int l = 0; folds && taps && l < L; ++l) folds = !slot(taps->svr_in, l) && !slot(taps->svr_out, l);
  const TokWeights w = tok_weights(c, Table{dry ? nullptr : W}, folds);

  Arena ar(ws, ws_bytes, dry);
  // split-K scratch for the skinny linear layers of this forward (M = 256 queries against E x E weights); registered
  // for this stream only while the launches below are being enqueued
  // (24 MB covers the E x E products; the TTA self-attention's packed q|k|v product takes the big-tile kernel in 4 K slices:
  //  4 x rows x 3E fp32)
  const size_t kSplitK = std::max<size_t>(24u << 20, (size_t)16 * B * c.num_query * 3 * E);
  char* skw = ar.get<char>(kSplitK);
  U2_CHECK_WS(ar);
  ScratchScope scratch_scope(ctx(), st, skw, kSplitK, !dry);
  Tok t{c, Run{ar, dry, st}, w, (taps && !dry) ? *taps : TokTaps{}, t_token, B, c.T, c.N, E, L, c.num_query, k,
        Heads{c.num_heads, d, 1.0f / sqrtf((float)d), c.max_seq_len}, (int64_t)B * c.T * c.N, (int64_t)B * c.num_query};
  const Run& r = t.r;
  t.xa = ar.get<bf16_t>((size_t)t.rows * E);
  t.xb = ar.get<bf16_t>((size_t)t.rows * E);
  t.qkv = ar.get<bf16_t>((size_t)t.rows * 3 * E);
  t.sctx = ar.get<bf16_t>((size_t)t.rows * E);
  U2_CHECK_WS(ar);

  // The reference's forward (u2Tokenizer.py:40-47): SpatioTemporalSignificanceScoring (svr.py:50-62) ...
  const bf16_t* x = v_token;
  for (int l = 0; l < L; ++l) U2_TRY(t.svr_layer(l, x));
  U2_TRY(tap(r, svr_out, x, (size_t)t.rows * E));  // optional: the refined tokens the selection stage sees (parity tests)
  // ... token selection and pooling (svr.py:171-184) ...
  bf16_t* sel = ar.get<bf16_t>((size_t)B * k * E);
  U2_CHECK_WS(ar);
  U2_TRY(c.enable_diffts ? t.select_diffts(x, sel) : t.select_topk(x, sel, topk_idx_out));
  U2_TRY(t.multiscale_pooling(sel));
  // ... TextConditionTokenAggregatorModel (tta.py:126-140)
  U2_TRY(t.tta_prefetch());
  U2_RUN(fill_rows(w.query, t.qa, B, (int64_t)t.Q * E, (int64_t)t.Q * E, st));  // query_tokens.expand(B,-1,-1)
  bf16_t* qcur = t.qa;
  for (int l = 0; l < L; ++l) U2_TRY(t.tta_layer(l, qcur));
  U2_TRY(t.linear_aggregation(qcur, out));
  if (peak) *peak = ar.peak;
  U2_CHECK_WS(ar);
  return U2_OK;
}

// y = ctx Wo^T + bo, then q | k | v = y Wqkv^T + bqkv  ==  ctx (Wqkv Wo)^T + (bo Wqkv^T + bqkv).  Wo [E_out][E_in] is the K-major B
// operand of the first product as it lies.  No split-K scratch, whatever the caller registered: the same bits for the same weights.
int svr_fold_build(const bf16_t* Wqkv, const bf16_t* bqkv, const bf16_t* Wo, const bf16_t* bo, bf16_t* Wf, bf16_t* bf, int E,
                   hipStream_t st) {
  if (!Wqkv || !bqkv || !Wo || !bo || !Wf || !bf || E <= 0 || (E & 7)) return U2_ERR_ARG;
  if (Wf == Wqkv || Wf == Wo || bf == bqkv || bf == bo) return U2_ERR_ARG;
  ScratchScope scratch_scope(ctx(), st, nullptr, 0, true);
  GemmDesc g;
  g.A = Wqkv; g.B = Wo; g.C = Wf;
  g.M = 3 * E; g.N = E; g.K = E;
  g.lda = E; g.ldb = E; g.ldc = E;
  g.flags = GEMM_B_KMAJOR;
  U2_TRY(gemm_bf16(g, st));
  return gemm_bf16(linear_desc(bo, E, Wqkv, bqkv, bf, 3 * E, 1, E, 3 * E, 0, nullptr, 0), st);
}

}  // namespace u2
