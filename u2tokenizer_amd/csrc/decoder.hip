// Row kernels of the decoder prefill that consumes the path's output (the step AFTER the path --
// LlamaForCausalLM / Qwen3ForCausalLM.forward on the spliced inputs_embeds, src/model/language_model/u2llama.py:76-87,123-126).
// The decoder stays the stock HuggingFace module tree (its parameters, its KV cache, its generate loop); for the PREFILL of
// the S = 1024 spliced embeddings the host side (u2tokenizer_amd/prefill.py) runs each layer as
//   RMSNorm -> packed q|k|v GEMM -> per-head RMSNorm (Qwen3) + rotary embedding -> causal grouped-query attention
//   (tokattn.hip) -> out-projection GEMM (+ residual) -> RMSNorm -> packed gate|up GEMM -> SiLU(gate) * up -> down GEMM (+ residual)
// and these are the HBM-bound pieces between the GEMMs.  All bf16 in / out, fp32 arithmetic, 16-byte accesses.
#include "rows.h"

namespace u2 {

// ------------------------------------------------------------------------------------------------ RMSNorm
// y[r][:] = bf16(x[r][:] * rsqrt(mean(x[r][:]^2) + eps)) * w   (LlamaRMSNorm / Qwen3RMSNorm: the normalised value is rounded
// to the input dtype before the product with w -- the same two rounding points here)
template <int NC>  // 16-byte chunks per lane held in registers: C <= NC * 512
__global__ __launch_bounds__(256) void rmsnorm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                      bf16_t* __restrict__ y, int64_t rows, int C, int64_t ldx, int64_t ldy,
                                                      float eps) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  rmsnorm_row<NC>(x + row * ldx, w, y + row * ldy, C, eps, threadIdx.x & 63);  // (rows.h: the norm in a product's tail runs the same row)
}

// (the refusals alone: the whole-stack step asks them of every layer before its first launch)
static int rmsnorm_check(const bf16_t* x, const bf16_t* w, const bf16_t* y, int64_t rows, int C, int64_t ldx, int64_t ldy) {
  if (!x || !w || !y || rows <= 0 || C <= 0 || (C & 7) || C > 8192 || (ldx & 7) || (ldy & 7)) return U2_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) || cdiv(rows, 4) > 0x7fffffff) return U2_ERR_ARG;
  return U2_OK;
}

int rmsnorm_bf16(const bf16_t* x, const bf16_t* w, bf16_t* y, int64_t rows, int C, int64_t ldx, int64_t ldy, float eps,
                 hipStream_t stream) {
  if (const int e = rmsnorm_check(x, w, y, rows, C, ldx, ldy)) return e;
  ProfScope ps(PROF_ROWOP, 0, stream, (double)rows * C * 4.0);
  dim3 grid((unsigned)cdiv(rows, 4));
#define U2_RN(NC) hipLaunchKernelGGL((rmsnorm_kernel<NC>), grid, dim3(256), 0, stream, x, w, y, rows, C, ldx, ldy, eps)
  if (C <= 1024) U2_RN(2);
  else if (C <= 2048) U2_RN(4);
  else if (C <= 4096) U2_RN(8);
  else U2_RN(16);
#undef U2_RN
  return launch_status();
}

// ------------------------------------------------------------------------------------------------ q / k: head norm + rotary
// In place on the q and k column blocks of the packed projection output qkv[rows][(Hq + 2 Hkv) D]: for every (row, head)
//   x <- RMSNorm_D(x) * w_q|k          (Qwen3Attention.q_norm / k_norm; skipped when the weight pointer is null: Llama)
//   x <- x * cos + rotate_half(x) * sin (apply_rotary_pos_emb; cos / sin: [rows][D] fp32 or bf16 as HF hands them out)
// One wave per (row, head); lane l < D/2 holds the pair (x[l], x[l + D/2]) rotate_half couples.
// kc / vc (optional): the KV cache's own layout, [batch][kv head][S][D] dense (HF DynamicLayer: (B, H_kv, S, D)); the finished
// k heads are written there as well and the v heads copied, so the cache takes the tensors as they are (row = batch * S + s).
template <int D, typename CS>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(bf16_t* __restrict__ qkv, const bf16_t* __restrict__ wq,
                                                           const bf16_t* __restrict__ wk, const CS* __restrict__ cosp,
                                                           const CS* __restrict__ sinp, int64_t rows, int Hq, int Hkv,
                                                           int64_t ld, int64_t cs_ld, float eps, bf16_t* __restrict__ kc,
                                                           bf16_t* __restrict__ vc, int S, int64_t kvs, int s_off) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nh = Hq + Hkv + (kc ? Hkv : 0);
  if (item >= rows * nh) return;
  const int64_t row = item / nh;
  const int hh = (int)(item - row * nh);
  bf16_t* p = qkv + row * ld + (int64_t)hh * D;  // k heads follow the q heads in the packed row, v heads the k heads
  constexpr int HALF = D / 2;
  const bool on = lane < HALF;
  bf16_t* cdst = nullptr;
  if (kc && hh >= Hq) {
    const int64_t bi = row / S, si = row - bi * S;
    const int hk = hh - Hq;
    // (kvs: elements between consecutive (batch, kv head) entries -- S * D dense, or the capacity of an append-in-place cache,
    //  whose next free position is s_off)
    cdst = (hk < Hkv ? kc + (bi * Hkv + hk) * kvs + (int64_t)(s_off + si) * D : vc + (bi * Hkv + (hk - Hkv)) * kvs + (int64_t)(s_off + si) * D);
    if (hk >= Hkv) {  // a v head: copy
      if (on) {
        cdst[lane] = p[lane];
        cdst[lane + HALF] = p[lane + HALF];
      }
      return;
    }
  }
  const bf16_t* w = hh < Hq ? wq : wk;
  float a = 0.f, b = 0.f;
  if (on) {
    a = bf16_to_f32(p[lane]);
    b = bf16_to_f32(p[lane + HALF]);
  }
  if (w) {
    const float rstd = rsqrtf(wave_sum(a * a + b * b) / (float)D + eps);
    if (on) {
      // (the reference rounds the normalised value to bf16 before the weight product: keep that rounding point)
      a = bf16_to_f32(f32_to_bf16(a * rstd)) * bf16_to_f32(w[lane]);
      b = bf16_to_f32(f32_to_bf16(b * rstd)) * bf16_to_f32(w[lane + HALF]);
      a = bf16_to_f32(f32_to_bf16(a));
      b = bf16_to_f32(f32_to_bf16(b));
    }
  }
  if (on) {
    const CS* cr = cosp + row * cs_ld;
    const CS* sr = sinp + row * cs_ld;
    const float c0 = (float)cr[lane], c1 = (float)cr[lane + HALF], s0 = (float)sr[lane], s1 = (float)sr[lane + HALF];
    const bf16_t r0 = f32_to_bf16(a * c0 - b * s0), r1 = f32_to_bf16(b * c1 + a * s1);  // rotate_half(x) = (-x2, x1)
    p[lane] = r0;
    p[lane + HALF] = r1;
    if (cdst) {
      cdst[lane] = r0;
      cdst[lane + HALF] = r1;
    }
  }
}

struct Bf16Val {  // bf16 cos / sin tables
  bf16_t v;
  __device__ explicit operator float() const { return bf16_to_f32(v); }
};

// (the refusals alone, and kv_stride resolved: 0 = dense)
static int qk_norm_rope_check(const bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int64_t rows, int Hq,
                              int Hkv, int D, const bf16_t* kc, const bf16_t* vc, int S, int64_t& kv_stride, int s_off) {
  if (!qkv || !cosp || !sinp || rows <= 0 || Hq <= 0 || Hkv <= 0 || (D != 64 && D != 96 && D != 128) || (!wq) != (!wk)) return U2_ERR_ARG;
  if ((!kc) != (!vc) || (kc && (S <= 0 || rows % S))) return U2_ERR_ARG;
  if (kv_stride == 0) kv_stride = (int64_t)S * D;
  if (kc && (s_off < 0 || kv_stride < (int64_t)(s_off + S) * D)) return U2_ERR_ARG;
  if (cdiv(rows * (Hq + Hkv + (kc ? Hkv : 0)), 4) > 0x7fffffff) return U2_ERR_ARG;
  return U2_OK;
}

int qk_norm_rope(bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int cs_is_f32,
                 int64_t rows, int Hq, int Hkv, int D, int64_t ld, int64_t cs_ld, float eps, bf16_t* kc, bf16_t* vc, int S,
                 int64_t kv_stride, int s_off, hipStream_t stream) {
  if (const int e = qk_norm_rope_check(qkv, wq, wk, cosp, sinp, rows, Hq, Hkv, D, kc, vc, S, kv_stride, s_off)) return e;
  const int64_t items = rows * (Hq + Hkv + (kc ? Hkv : 0));
  ProfScope ps(PROF_ROWOP, 0, stream, (double)items * D * 4.0);
  dim3 grid((unsigned)cdiv(items, 4));
#define U2_QK(D_, T_)                                                                                                     \
  hipLaunchKernelGGL((qk_norm_rope_kernel<D_, T_>), grid, dim3(256), 0, stream, qkv, wq, wk, reinterpret_cast<const T_*>(cosp), \
                     reinterpret_cast<const T_*>(sinp), rows, Hq, Hkv, ld, cs_ld, eps, kc, vc, S, kv_stride, s_off)
  if (D == 128 && cs_is_f32) U2_QK(128, float);
  else if (D == 128) U2_QK(128, Bf16Val);
  else if (D == 96 && cs_is_f32) U2_QK(96, float);   // (lanes 48..63 of each wave idle)
  else if (D == 96) U2_QK(96, Bf16Val);
  else if (cs_is_f32) U2_QK(64, float);
  else U2_QK(64, Bf16Val);
#undef U2_QK
  return launch_status();
}

// ------------------------------------------------------------------------------------------------ q / k: head norm + rotary, k / v: quantising append
// qk_norm_rope_kernel on an FP8 (e4m3) KV cache (decode_attn.hip: the format): the same work split and the same q and k columns of
// qkv, bit for bit; where that kernel writes the finished k head and copies the v head to 16-bit cache rows, this one writes them
// as codes -- D bytes at row (b Hkv + h) cap + s_off + s of kcd / vcd, one fp32 scale at that row of ksc / vsc --, quantised from
// the values ROUNDED to the element type (k: what it has just stored in qkv; v: the row as it stands there).  So codes and scales
// have the bits of kv_quantize_rows_kernel on the 16-bit rows qk_norm_rope_kernel would have written: the row maximum is exact in
// any order (idle lanes hold 0), the two divisions are IEEE fp32.  No 16-bit K / V row is written anywhere.
// Stores: v_cvt_pk_fp8_f32 leaves a lane's codes l and l + D/2 in bytes 0 and 1 of one register, and they go out as two
// global_store_byte, the second after one shift (read in the ISA: one conversion, one v_lshrrev, two byte stores, the scale's
// global_store_dword).  A store's up to 64 bytes are one contiguous run, the same lines dword stores would touch; collecting four
// lanes' codes into a dword first costs cross-lane moves and selects per half and still leaves two store instructions -- it saves
// active lanes only, on one row per (sequence, kv head).
template <int D, typename CS>
__global__ __launch_bounds__(256) void qk_norm_rope_kv8_kernel(bf16_t* __restrict__ qkv, const bf16_t* __restrict__ wq,
                                                               const bf16_t* __restrict__ wk, const CS* __restrict__ cosp,
                                                               const CS* __restrict__ sinp, int64_t rows, int Hq, int Hkv, int64_t ld,
                                                               int64_t cs_ld, float eps, uint8_t* __restrict__ kcd,
                                                               uint8_t* __restrict__ vcd, float* __restrict__ ksc,
                                                               float* __restrict__ vsc, int S, int cap, int s_off) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nh = Hq + 2 * Hkv;
  if (item >= rows * nh) return;
  const int64_t row = item / nh;
  const int hh = (int)(item - row * nh);
  bf16_t* p = qkv + row * ld + (int64_t)hh * D;  // k heads follow the q heads in the packed row, v heads the k heads
  constexpr int HALF = D / 2;
  const bool on = lane < HALF;
  const bool is_v = hh >= Hq + Hkv;
  float a = 0.f, b = 0.f;
  if (on) {
    a = bf16_to_f32(p[lane]);
    b = bf16_to_f32(p[lane + HALF]);
  }
  if (!is_v) {  // a q or k head: qk_norm_rope_kernel's arithmetic and rounding points
    const bf16_t* w = hh < Hq ? wq : wk;
    if (w) {
      const float rstd = rsqrtf(wave_sum(a * a + b * b) / (float)D + eps);
      if (on) {
        a = bf16_to_f32(f32_to_bf16(a * rstd)) * bf16_to_f32(w[lane]);
        b = bf16_to_f32(f32_to_bf16(b * rstd)) * bf16_to_f32(w[lane + HALF]);
        a = bf16_to_f32(f32_to_bf16(a));
        b = bf16_to_f32(f32_to_bf16(b));
      }
    }
    if (on) {
      const CS* cr = cosp + row * cs_ld;
      const CS* sr = sinp + row * cs_ld;
      const float c0 = (float)cr[lane], c1 = (float)cr[lane + HALF], s0 = (float)sr[lane], s1 = (float)sr[lane + HALF];
      const bf16_t r0 = f32_to_bf16(a * c0 - b * s0), r1 = f32_to_bf16(b * c1 + a * s1);  // rotate_half(x) = (-x2, x1)
      p[lane] = r0;
      p[lane + HALF] = r1;
      a = bf16_to_f32(r0);  // (the cache row is quantised from the rounded values)
      b = bf16_to_f32(r1);
    }
    if (hh < Hq) return;
  }
  // the row as codes: kv_quantize_rows_kernel's arithmetic (wave-uniform from here: a k or a v head)
  const float am = wave_max(fmaxf(fabsf(a), fabsf(b)));
  const float scale = am > 0.f ? am / 448.f : 1.f;
#if defined(__HIP_DEVICE_COMPILE__)
  const int c = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(a / scale, -448.f), 448.f), fminf(fmaxf(b / scale, -448.f), 448.f), 0, false);
#else
  const int c = 0;
#endif
  const int hk = hh - Hq - (is_v ? Hkv : 0);
  const int64_t bi = row / S, si = row - bi * S;
  const int64_t pos = (bi * Hkv + hk) * cap + s_off + si;
  if (on) {
    uint8_t* dst = (is_v ? vcd : kcd) + pos * D;
    dst[lane] = (uint8_t)c;
    dst[lane + HALF] = (uint8_t)(c >> 8);
  }
  if (lane == 0) (is_v ? vsc : ksc)[pos] = scale;
}

// (the refusals alone: qk_norm_rope_check's, and of the destination what kv_quantize_rows refuses of its own)
static int qk_norm_rope_kv8_check(const bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int64_t rows, int Hq,
                                  int Hkv, int D, const uint8_t* kcd, const uint8_t* vcd, const float* ksc, const float* vsc, int S, int capacity,
                                  int s_off) {
  if (!kcd || !vcd || !ksc || !vsc || capacity <= 0 || S <= 0 || s_off < 0 || (int64_t)s_off + S > capacity) return U2_ERR_ARG;
  if ((((uintptr_t)kcd | (uintptr_t)vcd) & 15) || (((uintptr_t)ksc | (uintptr_t)vsc) & 3)) return U2_ERR_ARG;
  int64_t kv_stride = (int64_t)capacity * D;  // (rows of D elements: that check's room for s_off + S is the one made above)
  if (const int e = qk_norm_rope_check(qkv, wq, wk, cosp, sinp, rows, Hq, Hkv, D, reinterpret_cast<const bf16_t*>(kcd),
                                       reinterpret_cast<const bf16_t*>(vcd), S, kv_stride, s_off))
    return e;
  return (int64_t)capacity * D >= (1ll << 31) ? U2_ERR_ARG : U2_OK;
}

int qk_norm_rope_kv8(bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int cs_is_f32, int64_t rows, int Hq,
                     int Hkv, int D, int64_t ld, int64_t cs_ld, float eps, uint8_t* kcd, uint8_t* vcd, float* ksc, float* vsc, int S,
                     int capacity, int s_off, hipStream_t stream) {
  if (const int e = qk_norm_rope_kv8_check(qkv, wq, wk, cosp, sinp, rows, Hq, Hkv, D, kcd, vcd, ksc, vsc, S, capacity, s_off)) return e;
  const int64_t items = rows * (Hq + 2 * Hkv);
  ProfScope ps(PROF_ROWOP, 0, stream, (double)items * D * 4.0);
  dim3 grid((unsigned)cdiv(items, 4));
#define U2_QK8(D_, T_)                                                                                                        \
  hipLaunchKernelGGL((qk_norm_rope_kv8_kernel<D_, T_>), grid, dim3(256), 0, stream, qkv, wq, wk, reinterpret_cast<const T_*>(cosp), \
                     reinterpret_cast<const T_*>(sinp), rows, Hq, Hkv, ld, cs_ld, eps, kcd, vcd, ksc, vsc, S, capacity, s_off)
  if (D == 128 && cs_is_f32) U2_QK8(128, float);
  else if (D == 128) U2_QK8(128, Bf16Val);
  else if (D == 96 && cs_is_f32) U2_QK8(96, float);   // (lanes 48..63 of each wave idle)
  else if (D == 96) U2_QK8(96, Bf16Val);
  else if (cs_is_f32) U2_QK8(64, float);
  else U2_QK8(64, Bf16Val);
#undef U2_QK8
  return launch_status();
}

// ------------------------------------------------------------------------------------------------ SwiGLU
// out[r][i] = silu(gu[r][i]) * gu[r][I + i]   (LlamaMLP / Qwen3MLP: down_proj(act_fn(gate_proj(x)) * up_proj(x)) with the
// gate | up projections packed into one GEMM); the reference rounds silu(gate) to bf16 before the product: kept.
__global__ __launch_bounds__(256) void swiglu_kernel(const bf16_t* __restrict__ gu, bf16_t* __restrict__ out, int64_t rows, int I,
                                                     int64_t ld_in, int64_t ld_out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per = I >> 3;
  if (idx >= rows * per) return;
  const int64_t r = idx / per;
  const int c = (int)(idx - r * per) * 8;
  const uint4 g = *reinterpret_cast<const uint4*>(gu + r * ld_in + c);
  const uint4 u = *reinterpret_cast<const uint4*>(gu + r * ld_in + I + c);
  auto f = [](float gate, float up) {
    const float s = gate / (1.0f + __expf(-gate));
    return bf16_to_f32(f32_to_bf16(s)) * up;
  };
  *reinterpret_cast<uint4*>(out + r * ld_out + c) =
      uint4{pack2_bf16(f(bf16lo(g.x), bf16lo(u.x)), f(bf16hi(g.x), bf16hi(u.x))),
            pack2_bf16(f(bf16lo(g.y), bf16lo(u.y)), f(bf16hi(g.y), bf16hi(u.y))),
            pack2_bf16(f(bf16lo(g.z), bf16lo(u.z)), f(bf16hi(g.z), bf16hi(u.z))),
            pack2_bf16(f(bf16lo(g.w), bf16lo(u.w)), f(bf16hi(g.w), bf16hi(u.w)))};
}

int swiglu_check(const bf16_t* gu, const bf16_t* out, int64_t rows, int I, int64_t ld_in, int64_t ld_out) {
  if (!gu || !out || rows <= 0 || I <= 0 || (I & 7) || (ld_in & 7) || (ld_out & 7) || (((uintptr_t)gu | (uintptr_t)out) & 15))
    return U2_ERR_ARG;
  return cdiv(rows * (I >> 3), 256) > 0x7fffffff ? U2_ERR_ARG : U2_OK;
}

int swiglu_bf16(const bf16_t* gu, bf16_t* out, int64_t rows, int I, int64_t ld_in, int64_t ld_out, hipStream_t stream) {
  if (const int e = swiglu_check(gu, out, rows, I, ld_in, ld_out)) return e;
  const int64_t total = rows * (I >> 3);
  ProfScope ps(PROF_ROWOP, 0, stream, (double)rows * I * 6.0);
  hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, gu, out, rows, I, ld_in, ld_out);
  return launch_status();
}

// ------------------------------------------------------------------------------------------------ one decode step of a layer
// The two halves of a decoder layer's decode step (B <= 64 new tokens against the KV cache), each ONE call for the host: the
// step `generate` repeats up to 768 times per report is bound by the host's launch rate when every kernel is its own Python
// call (7.9 ms per step of a 36-layer decoder, ~4 ms of kernels).  Between the halves the host appends k / v to its cache
// (HF DynamicCache: a torch.cat) and hands back the dense (B, H_kv, T, D) tensors.
// Every entry point walks its sequence of launches twice, through one Step: a DEC_CHECK walk, in which each op answers with the
// refusals of its launcher -- the launcher's own code -- and launches nothing, then a DEC_RUN walk, in which each op launches.  The
// sequence is written once, and every refusal of a call, whichever launcher raises it, precedes the call's first launch.
enum : int { DEC_CHECK = 1, DEC_RUN = 2 };

struct Step {
  int mode;
  hipStream_t st;
  bool check() const { return mode == DEC_CHECK; }

  int norm(const bf16_t* x, const bf16_t* w, bf16_t* y, int rows, int C, int64_t ldx, float eps) const {
    return check() ? rmsnorm_check(x, w, y, rows, C, ldx, C) : rmsnorm_bf16(x, w, y, rows, C, ldx, C, eps, st);
  }
  int rows(const RowsArgs& a) const { return check() ? gemm_rows_check(a) : gemm_rows(a, st); }
  int rope(bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int cs_is_f32, int rows, int Hq, int Hkv,
           int D, int64_t cs_ld, float eps, bf16_t* kc, bf16_t* vc, int64_t kv_stride, int s_off) const {
    const int64_t ld = (int64_t)(Hq + 2 * Hkv) * D;
    return check() ? qk_norm_rope_check(qkv, wq, wk, cosp, sinp, rows, Hq, Hkv, D, kc, vc, 1, kv_stride, s_off)
                   : qk_norm_rope(qkv, wq, wk, cosp, sinp, cs_is_f32, rows, Hq, Hkv, D, ld, cs_ld, eps, kc, vc, 1, kv_stride, s_off, st);
  }
  // (the same on an e4m3 cache: the step's k / v rows go to position q8.s_off of its buffers as codes)
  int rope8(bf16_t* qkv, const bf16_t* wq, const bf16_t* wk, const void* cosp, const void* sinp, int cs_is_f32, int rows, int Hq, int Hkv, int D,
            int64_t cs_ld, float eps, const DecodeKv8& q8) const {
    const int64_t ld = (int64_t)(Hq + 2 * Hkv) * D;
    return check() ? qk_norm_rope_kv8_check(qkv, wq, wk, cosp, sinp, rows, Hq, Hkv, D, q8.Kc, q8.Vc, q8.Ks, q8.Vs, 1, q8.capacity, q8.s_off)
                   : qk_norm_rope_kv8(qkv, wq, wk, cosp, sinp, cs_is_f32, rows, Hq, Hkv, D, ld, cs_ld, eps, q8.Kc, q8.Vc, q8.Ks, q8.Vs, 1, q8.capacity,
                                      q8.s_off, st);
  }
  int swiglu(const bf16_t* gu, bf16_t* act, int rows, int I) const {
    return check() ? swiglu_check(gu, act, rows, I, 2 * I, I) : swiglu_bf16(gu, act, rows, I, 2 * I, I, st);
  }
  int attend(const AttnCall& a) const { return check() ? attention_check(a) : attention(a, st); }
  // (decode_attention, decode_attention_kv8, kv_quantize_rows, lora_rows: launchers that take the walk's mode themselves)
};

// One projection of the step on a weight (w, scale) in `form`: the element type's product through the plan, codes (the step's
// DecodeCfg::form) through the few-rows product on 1-byte or 4-bit weights (gemm_rows.hip).  pair: w = gate | up, y (rows, out / 2).
// In a check walk: the product's refusals alone -- gemm_rows_check, or the plan's own verdict.
// norm (w set; the whole-stack step's): the RMSNorm that follows the product, asked for in the product's tail (RowsNorm: the
//   non-pair form with a residual).  *normed says whether the launch carried it: yes where the few-rows kernel runs the product
//   (always on codes and above 16 rows, else when the plan picks it) and takes the norm (gemm_rows_check); no -- and in a check walk
//   always -- the caller's next op is the norm itself.
static int dec_linear(const Step& s, const bf16_t* x, int64_t ldx, const void* w, const void* scale, WForm form, const bf16_t* b, bf16_t* y,
                      int64_t ldy, int rows, int in, int out, const bf16_t* R, int64_t ldr, bool pair, const RowsNorm* norm = nullptr,
                      bool* normed = nullptr) {
  RowsArgs a;
  a.A = x; a.W = w; a.scale = scale; a.form = form; a.C = y; a.bias = b; a.R = R;
  a.M = rows; a.N = out; a.K = in;
  a.lda = ldx; a.ldw = in / wform_facts(form).ldw_div; a.lds = in >> 5; a.ldc = ldy; a.ldr = ldr;
  a.flags = pair ? GEMM_SWIGLU : (b ? GEMM_BIAS_N : 0) | (R ? GEMM_RESIDUAL : 0);
  if (normed) *normed = false;
  bool tail = false;
  if (norm && norm->w) {  // (a norm the tail does not take -- a row wider than it holds -- stays a launch of its own)
    a.norm = *norm;
    tail = gemm_rows_check(a) == U2_OK;
    if (!tail) a.norm = RowsNorm{};
  }
  if (form != WForm::ELEM || rows > 16) {
    const int e = s.rows(a);
    if (normed) *normed = tail && e == U2_OK && !s.check();
    return e;
  }
  GemmDesc g;  // 16-bit weights, M <= 16: the plan (the same kernel, or a tile kernel when rows16_ok says no)
  g.A = x; g.B = reinterpret_cast<const bf16_t*>(w); g.C = y; g.bias = b; g.R = R;
  g.M = rows; g.N = out; g.K = in;
  g.lda = ldx; g.ldb = in; g.ldc = ldy; g.ldr = ldr;
  g.flags = a.flags;
  if (!s.check() && !tail) return gemm_bf16(g, s.st);
  GemmDesc v = g;  // the plan's verdict without a launch
  GemmPlan p;
  const Scratch sc = ctx().scratch_of(s.st);
  int e = gemm_validate(v);
  if (e == U2_OK) e = gemm_plan(v, opts(), sc.p ? sc.bytes : 0, p);
  if (e != U2_OK || s.check()) return e;
  if (p.nsteps != 1 || p.step[0].kind != GK_ROWS16) return gemm_bf16(g, s.st);  // (a tile kernel: no tail to carry the norm)
  e = gemm_rows(a, s.st);  // the kernel the plan launches for this product, bit for bit, with the norm in its tail
  if (normed) *normed = e == U2_OK;
  return e;
}

// The adapter group of one product of the step (DecodeLora; lora_rows.hip): u at the head of the branch's scratch, the group's
// workspace behind it.  No adapters, or none on this product: no op.
static int dec_lora(const Step& s, const DecodeLora* lr, const LoraSeg* segs, int n, int nmax, const bf16_t* x, int64_t ldx, bf16_t* y,
                    int64_t ldy, int rows, int in) {
  if (!lr || n == 0) return U2_OK;
  if (n < 0 || n > nmax || !lr->scratch || ((uintptr_t)lr->scratch & 15)) return U2_ERR_ARG;
  if (lr->scratch_bytes < DECODE_LORA_U_BYTES) return U2_ERR_WORKSPACE;
  return lora_rows(x, ldx, segs, n, reinterpret_cast<bf16_t*>(lr->scratch), DECODE_LORA_U_LD, y, ldy, rows, in,
                   reinterpret_cast<char*>(lr->scratch) + DECODE_LORA_U_BYTES, lr->scratch_bytes - DECODE_LORA_U_BYTES, s.check(), s.st);
}

// What a quantised form asks of a step before anything is launched (WFormFacts): E, Hq D and I multiples of the form's step, and of
// the n products from `first` on (q|k|v, o, gate|up, down: the ones this half runs) 16-byte aligned codes and a scale aligned to
// its type.  The element type's products check themselves.
static bool wform_step_ok(const DecodeCfg& c, const DecodeLayer& l, int first, int n) {
  if (!wform_known(c.form)) return false;
  if (c.form == WForm::ELEM) return true;
  const WFormFacts& f = wform_facts(c.form);
  if (c.E % f.k_mult || (c.Hq * c.D) % f.k_mult || c.I % f.k_mult) return false;
  const void* const w[4] = {l.Wqkv, l.Wo, l.Wgu, l.Wdown};
  const void* const sc[4] = {l.scale_qkv, l.scale_o, l.scale_gu, l.scale_down};
  for (int i = first; i < first + n; ++i)
    if (!w[i] || !sc[i] || ((uintptr_t)w[i] & 15) || (uintptr_t)sc[i] % f.scale_align) return false;
  return true;
}

size_t decoder_decode_workspace_bytes(const DecodeCfg& c, int T) {
  const size_t rows = (size_t)c.B;
  size_t n = rows * ((size_t)3 * c.E + (size_t)c.Hq * c.D + (size_t)3 * c.I) * sizeof(bf16_t);  // xn, h, hn | ctx | gu (2 I), act
  n = (n + 255) & ~(size_t)255;
  // the attention's key-split partials: decoder_decode_post's per-sequence form or its batched kernel
  return n + std::max(tok_attention_workspace_bytes(c.Hkv, c.Hq / c.Hkv, 1, T, c.D), decode_attention_workspace_bytes(c.B, c.Hq, c.Hkv, T, c.D)) +
         256;
}

// The two walks of a per-layer entry (the whole-stack step makes them over all its layers: stack_walk)
template <typename Half>
static int check_then_run(hipStream_t st, const Half& half) {
  const int e = half(Step{DEC_CHECK, st});
  return e != U2_OK ? e : half(Step{DEC_RUN, st});
}

// input RMSNorm -> q|k|v projection -> per-head RMSNorm + rotary; qkv (B, (Hq + 2 Hkv) D) keeps the finished queries, kc / vc
// (B, Hkv, 1, D) receive the new cache entries.  have_xn (the whole-stack step): the norm rode in the tail of the product that wrote x.
// q8 (the whole-stack step on an e4m3 cache): the new entries go to position q8->s_off of its buffers as codes, in the rotary
// kernel's launch (qk_norm_rope_kv8); kc / vc are not read.
static int dec_pre(const Step& s, const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32,
                   int64_t cs_ld, bf16_t* qkv, bf16_t* kc, bf16_t* vc, int64_t kv_stride, int s_off, void* ws, size_t ws_bytes, bool have_xn,
                   const DecodeKv8* q8 = nullptr) {
  if (s.check()) {  // the half's own refusals; everything below is a launcher's
    if (c.B <= 0 || c.B > 64 || c.Hkv <= 0 || c.Hq % c.Hkv || !x || !l.w_in_norm || !l.Wqkv || !qkv || (!q8 && (!kc || !vc)) || !ws) return U2_ERR_ARG;
    if (!wform_step_ok(c, l, 0, 1)) return U2_ERR_ARG;
    if (ws_bytes < (size_t)c.B * c.E * sizeof(bf16_t)) return U2_ERR_WORKSPACE;
  }
  bf16_t* xn = reinterpret_cast<bf16_t*>(ws);
  const int nq = (c.Hq + 2 * c.Hkv) * c.D;
  const DecodeLora* lr = l.lora;
  int e = have_xn ? U2_OK : s.norm(x, l.w_in_norm, xn, c.B, c.E, c.E, c.eps);
  if (e == U2_OK) e = dec_linear(s, xn, c.E, l.Wqkv, l.scale_qkv, c.form, l.bqkv, qkv, nq, c.B, c.E, nq, nullptr, 0, false);
  if (e == U2_OK && lr) e = dec_lora(s, lr, lr->qkv, lr->n_qkv, 3, xn, c.E, qkv, nq, c.B, c.E);  // (before the head norm and the rotary embedding)
  if (e != U2_OK) return e;
  return q8 ? s.rope8(qkv, l.wq_norm, l.wk_norm, cosp, sinp, cs_is_f32, c.B, c.Hq, c.Hkv, c.D, cs_ld, c.qk_eps, *q8)
            : s.rope(qkv, l.wq_norm, l.wk_norm, cosp, sinp, cs_is_f32, c.B, c.Hq, c.Hkv, c.D, cs_ld, c.qk_eps, kc, vc, kv_stride, s_off);
}

int decoder_decode_pre(const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32,
                       int64_t cs_ld, bf16_t* qkv, bf16_t* kc, bf16_t* vc, int64_t kv_stride, int s_off, void* ws, size_t ws_bytes,
                       hipStream_t st) {
  return check_then_run(st, [&](const Step& s) {
    return dec_pre(s, c, l, x, cosp, sinp, cs_is_f32, cs_ld, qkv, kc, vc, kv_stride, s_off, ws, ws_bytes, false);
  });
}

// attention over the cache (keys split over workgroups) -> out projection + residual -> RMSNorm -> gate|up -> SwiGLU -> down
// projection + residual.  K / V: (B, Hkv, T, D) with kv_stride elements between (batch, kv head) entries (0: dense); out (B, E).
// (batched: decode_attn.hip's kernel over all sequences with kv_start, else one attention() launch pair per sequence -- B <= 16
// only: 17 .. 64 sequences take the batched kernel or U2_ERR_ARG.  q8: an e4m3 cache, decoder_decode_post_kv8; with k_new and
// v_new both null -- the whole-stack step, whose rotary kernel has put the step's rows at s_off already -- no quantising launch)
// The whole-stack step's tail norms -- ticket (null: none): the post-attention norm is asked for in the tail of the o product, and
// `after` (w set: the norm that follows this layer -- the next layer's input norm or the stack's final one, into after->Yn) in the
// tail of the down product; *after_done: that launch carried it.  A product followed by an adapter group keeps the norm's own
// launch: the group adds to the product's rows after it.
static int dec_post(const Step& s, const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const bf16_t* qkv, const bf16_t* K, const bf16_t* V,
                    int T, int64_t kv_stride, bool batched, const int* kv_start, bf16_t* out, void* ws, size_t ws_bytes, uint32_t* ticket,
                    const RowsNorm* after, bool* after_done, const DecodeKv8* q8 = nullptr) {
  if (s.check()) {  // the half's own refusals; everything below is a launcher's
    if (c.B <= 0 || c.B > 64 || (c.B > 16 && !batched) || c.Hkv <= 0 || T <= 0 || !x || !qkv || (!q8 && (!K || !V)) || !l.Wo || !l.w_post_norm || !l.Wgu || !l.Wdown || !out ||
        !ws)
      return U2_ERR_ARG;
    if (batched ? c.Hq / c.Hkv > 16 || ((uintptr_t)kv_start & 3) : kv_start != nullptr) return U2_ERR_ARG;
    if (!wform_step_ok(c, l, 1, 3)) return U2_ERR_ARG;
    if (ws_bytes < decoder_decode_workspace_bytes(c, T)) return U2_ERR_WORKSPACE;
    if (q8 && (!batched || q8->k_first < 0 || q8->s_off < q8->k_first || T != q8->s_off - q8->k_first + 1)) return U2_ERR_ARG;
  }
  const int g = c.Hq / c.Hkv, nq = (c.Hq + 2 * c.Hkv) * c.D, qd = c.Hq * c.D;
  bf16_t* p = reinterpret_cast<bf16_t*>(ws);
  bf16_t* h = p + (size_t)c.B * c.E;          // (xn of the first half lives at p)
  bf16_t* hn = h + (size_t)c.B * c.E;
  bf16_t* ctx = hn + (size_t)c.B * c.E;
  bf16_t* gu = ctx + (size_t)c.B * qd;
  bf16_t* act = gu + (size_t)c.B * 2 * c.I;
  size_t used = ((size_t)c.B * ((size_t)3 * c.E + qd + (size_t)3 * c.I) * sizeof(bf16_t) + 255) & ~(size_t)255;
  char* aws = reinterpret_cast<char*>(ws) + used;
  const size_t aws_bytes = ws_bytes - used;
  if (kv_stride == 0) kv_stride = (int64_t)T * c.D;
  const DecodeLora* lr = l.lora;
  int e = U2_OK;
  if (q8) {  // the step's rows into position s_off as codes, then the attention over positions k_first .. s_off
    if (q8->k_new || q8->v_new)
      e = kv_quantize_rows(q8->k_new, q8->v_new, c.B, c.Hkv, 1, c.D, (int64_t)c.Hkv * c.D, c.D, c.D, (int64_t)c.Hkv * c.D, c.D, c.D, q8->Kc, q8->Vc,
                           q8->Ks, q8->Vs, q8->capacity, q8->s_off, s.check(), s.st);
    if (e == U2_OK)
      e = decode_attention_kv8(qkv, q8->Kc + (int64_t)q8->k_first * c.D, q8->Vc + (int64_t)q8->k_first * c.D, q8->Ks + q8->k_first,
                               q8->Vs + q8->k_first, ctx, c.B, c.Hq, c.Hkv, T, c.D, nq, (int64_t)q8->capacity * c.D, q8->capacity, qd, c.scale,
                               kv_start, aws, aws_bytes, s.check(), s.st);
  } else if (batched) {
    e = decode_attention(qkv, K, V, ctx, c.B, c.Hq, c.Hkv, T, c.D, nq, kv_stride, qd, c.scale, kv_start, aws, aws_bytes, s.check(), s.st);
  } else {
    // attention() is every caller's launcher and asks less of a cache than decode_attention: a scale that is not positive, a
    // (batch, kv head) entry shorter than its T rows or past 32-bit offsets stay the step's to refuse, where the whole-stack walk
    // has always refused them, so that a call's status does not depend on the attention it asks for
    if (s.check() && (!(c.scale > 0.f) || kv_stride < (int64_t)T * c.D || (int64_t)T * c.D * 2 >= (1ll << 31))) return U2_ERR_ARG;
    for (int b = 0; b < c.B && e == U2_OK; ++b) {  // entries of one batch element: its kv heads; the g query heads of a group are the "heads"
      AttnCall a;
      a.q = qkv + (size_t)b * nq; a.k = K + (size_t)b * c.Hkv * kv_stride; a.v = V + (size_t)b * c.Hkv * kv_stride;
      a.out = ctx + (size_t)b * qd;
      a.nb = c.Hkv; a.Sq = 1; a.Skv = T; a.H = g; a.Hkv = 1; a.d = c.D;
      a.ldq = a.ldo = a.q_bs = a.o_bs = (int64_t)g * c.D; a.ldk = a.ldv = c.D; a.k_bs = a.v_bs = kv_stride;
      a.scale = c.scale; a.ws = aws; a.ws_bytes = aws_bytes;
      e = s.attend(a);
    }
  }
  if (e != U2_OK) return e;
  RowsNorm o_norm;
  if (ticket && !(lr && lr->n_o != 0)) o_norm.w = l.w_post_norm, o_norm.Yn = hn, o_norm.ld = c.E, o_norm.eps = c.eps, o_norm.ticket = ticket;
  bool normed = false;
  e = dec_linear(s, ctx, qd, l.Wo, l.scale_o, c.form, l.bo, h, c.E, c.B, qd, c.E, x, c.E, false, &o_norm, &normed);
  if (e == U2_OK && lr) e = dec_lora(s, lr, lr->o, lr->n_o, 1, ctx, qd, h, c.E, c.B, qd);   // (after the residual epilogue: the same terms)
  if (e == U2_OK && !normed) e = s.norm(h, l.w_post_norm, hn, c.B, c.E, c.E, c.eps);
  if (e != U2_OK) return e;
  const bool gu_lora = lr && lr->n_gu != 0;   // a gate or up adapter: the pair product in its unfused form, the group before the SiLU
  if (!gu_lora && !l.bgu && !(c.E & 63) && !(c.I & 15)) {  // SiLU(gate) * up in the epilogue of the pair product (gemm_rows16_kernel<., true>)
    e = dec_linear(s, hn, c.E, l.Wgu, l.scale_gu, c.form, nullptr, act, c.I, c.B, c.E, 2 * c.I, nullptr, 0, true);
  } else {
    e = dec_linear(s, hn, c.E, l.Wgu, l.scale_gu, c.form, l.bgu, gu, 2 * c.I, c.B, c.E, 2 * c.I, nullptr, 0, false);
    if (e == U2_OK && gu_lora) e = dec_lora(s, lr, lr->gu, lr->n_gu, 2, hn, c.E, gu, 2 * c.I, c.B, c.E);
    if (e == U2_OK) e = s.swiglu(gu, act, c.B, c.I);
  }
  if (e != U2_OK) return e;
  const bool down_tail = ticket && after && !(lr && lr->n_down != 0);
  e = dec_linear(s, act, c.I, l.Wdown, l.scale_down, c.form, l.bdown, out, c.E, c.B, c.I, c.E, h, c.E, false, down_tail ? after : nullptr, after_done);
  if (e == U2_OK && lr) e = dec_lora(s, lr, lr->down, lr->n_down, 1, act, c.I, out, c.E, c.B, c.I);
  return e;
}

int decoder_decode_post(const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const bf16_t* qkv, const bf16_t* K, const bf16_t* V,
                        int T, int64_t kv_stride, bool batched, const int* kv_start, bf16_t* out, void* ws, size_t ws_bytes,
                        hipStream_t st) {
  return check_then_run(st, [&](const Step& s) {
    return dec_post(s, c, l, x, qkv, K, V, T, kv_stride, batched, kv_start, out, ws, ws_bytes, nullptr, nullptr, nullptr);
  });
}

int decoder_decode_post_kv8(const DecodeCfg& c, const DecodeLayer& l, const bf16_t* x, const bf16_t* qkv, const DecodeKv8& kv,
                            const int* kv_start, bf16_t* out, void* ws, size_t ws_bytes, hipStream_t st) {
  const int64_t T = (int64_t)kv.s_off - kv.k_first + 1;
  if (T <= 0 || T > 0x7fffffff || !kv.k_new || !kv.v_new) return U2_ERR_ARG;  // (this entry always quantises: its rows are the caller's)
  return check_then_run(st, [&](const Step& s) {
    return dec_post(s, c, l, x, qkv, nullptr, nullptr, (int)T, 0, true, kv_start, out, ws, ws_bytes, nullptr, nullptr, nullptr, &kv);
  });
}

// ------------------------------------------------------------------------------------------------ one decode step of the stack
// The whole decoder stack's step in ONE call: per layer exactly the launches of the two halves above, in their order, on the
// caller's stream; the hidden state goes from layer to layer through two (B, E) rows of the workspace, the stack's final RMSNorm
// (w_final: null = none) writes `out`.  The workspace: 256 bytes whose first 4 are the tail norms' ticket (zeroed once by whoever
// owns the workspace; every launch that uses it leaves it zero), the layers' shared per-layer workspace (the largest
// decoder_decode_workspace_bytes of them), the q|k|v rows, the two hidden rows.
// tail_norm: the three norms that follow an o or a down product ride in that product's tail (dec_post).
// A layer on an e4m3 cache (DecodeStackLayer::kv8): the same walk, the same workspace; its first half's rotary kernel writes the
// step's rows as codes (qk_norm_rope_kv8), its second half attends over the codes -- as many launches as a 16-bit layer has.
static size_t stack_layer_ws(const DecodeStackLayer* L, int n) {
  size_t m = 0;
  for (int i = 0; i < n; ++i) m = std::max(m, decoder_decode_workspace_bytes(L[i].cfg, L[i].T));
  return (m + 255) & ~(size_t)255;
}
static size_t stack_qkv_bytes(const DecodeStackLayer* L, int n) {
  size_t m = 0;
  for (int i = 0; i < n; ++i) m = std::max(m, (size_t)L[i].cfg.B * (L[i].cfg.Hq + 2 * L[i].cfg.Hkv) * L[i].cfg.D * sizeof(bf16_t));
  return (m + 255) & ~(size_t)255;
}
static size_t stack_hidden_bytes(const DecodeCfg& c) { return ((size_t)c.B * c.E * sizeof(bf16_t) + 255) & ~(size_t)255; }

size_t decoder_decode_stack_workspace_bytes(const DecodeStackLayer* L, int n) {
  if (!L || n <= 0) return 0;
  for (int i = 0; i < n; ++i)
    if (L[i].T <= 0 || L[i].cfg.B != L[0].cfg.B || L[i].cfg.E != L[0].cfg.E) return 0;
  return 256 + stack_layer_ws(L, n) + stack_qkv_bytes(L, n) + 2 * stack_hidden_bytes(L[0].cfg);
}

// One walk over every half of every layer: the step is the check walk, then the run walk; the step with the head puts its head's
// walks behind each of the two.
static int stack_walk(const Step& s, const DecodeStackLayer* L, int n, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32,
                      int64_t cs_ld, bool batched, const int* kv_start, const bf16_t* w_final, float final_eps, bool tail_norm, bf16_t* out,
                      void* ws, size_t ws_bytes) {
  if (s.check()) {
    if (!L || n <= 0 || !x || !out || !ws || ((uintptr_t)ws & 255)) return U2_ERR_ARG;
    for (int i = 0; i < n; ++i) {
      const DecodeStackLayer& sl = L[i];
      if (sl.cfg.B != L[0].cfg.B || sl.cfg.E != L[0].cfg.E || sl.T <= 0 || sl.k_first < 0 || sl.s_off < 0 ||
          (int64_t)sl.k_first + sl.T > (int64_t)sl.s_off + 1)
        return U2_ERR_ARG;
      // (an e4m3 cache: the attention reads up to the step's own row, 0 <= k_first <= s_off < capacity, and only in its batched form)
      if (sl.kv8 && (!batched || sl.s_off >= sl.capacity || (int64_t)sl.T != (int64_t)sl.s_off - sl.k_first + 1)) return U2_ERR_ARG;
    }
    const size_t need = decoder_decode_stack_workspace_bytes(L, n);
    if (need == 0) return U2_ERR_ARG;
    if (ws_bytes < need) return U2_ERR_WORKSPACE;
  }
  const DecodeCfg& c0 = L[0].cfg;
  char* base = reinterpret_cast<char*>(ws);
  uint32_t* ticket = tail_norm ? reinterpret_cast<uint32_t*>(base) : nullptr;
  void* lws = base + 256;
  const size_t lws_bytes = stack_layer_ws(L, n);
  bf16_t* qkv = reinterpret_cast<bf16_t*>(base + 256 + lws_bytes);
  bf16_t* hid[2];
  hid[0] = reinterpret_cast<bf16_t*>(reinterpret_cast<char*>(qkv) + stack_qkv_bytes(L, n));
  hid[1] = reinterpret_cast<bf16_t*>(reinterpret_cast<char*>(hid[0]) + stack_hidden_bytes(c0));
  bf16_t* xn = reinterpret_cast<bf16_t*>(lws);  // (where every layer's first half keeps its normed input: dec_pre)
  const bf16_t* cur = x;
  bool have_xn = false;
  for (int i = 0; i < n; ++i) {
    const DecodeStackLayer& sl = L[i];
    const bool last = i == n - 1;
    bf16_t* nxt = last && !w_final ? out : hid[i & 1];
    // (an e4m3 cache: the rotary kernel appends the codes, the second half finds the rows in place -- no k_new / v_new)
    const DecodeKv8 q8v{nullptr, nullptr, sl.Kc, sl.Vc, sl.Ks, sl.Vs, sl.capacity, sl.k_first, sl.s_off};
    const DecodeKv8* q8 = sl.kv8 ? &q8v : nullptr;
    int e = dec_pre(s, sl.cfg, sl.layer, cur, cosp, sinp, cs_is_f32, cs_ld, qkv, sl.kc, sl.vc, sl.kv_stride, sl.s_off, lws, lws_bytes, have_xn, q8);
    if (e != U2_OK) return e;   // (a null cache buffer among them: nothing below offsets one)
    RowsNorm after;  // the norm that follows the layer: the next layer's input norm into its xn, or the final norm into out
    if (!last) after.w = L[i + 1].layer.w_in_norm, after.Yn = xn, after.eps = L[i + 1].cfg.eps;
    else if (w_final) after.w = w_final, after.Yn = out, after.eps = final_eps;
    after.ld = c0.E;
    after.ticket = ticket;
    bool done = false;  // the down product's tail carried `after` (never in a check walk: the norm's own refusals are asked for)
    const int64_t first = (int64_t)sl.k_first * sl.cfg.D;
    e = dec_post(s, sl.cfg, sl.layer, cur, qkv, q8 ? nullptr : sl.kc + first, q8 ? nullptr : sl.vc + first, sl.T, sl.kv_stride, batched, kv_start,
                 nxt, lws, lws_bytes, ticket, after.w ? &after : nullptr, &done, q8);
    if (e == U2_OK && last && w_final && !done) e = s.norm(nxt, w_final, out, c0.B, c0.E, c0.E, final_eps);
    if (e != U2_OK) return e;
    have_xn = done && !last;
    cur = nxt;
  }
  return U2_OK;
}

int decoder_decode_stack(const DecodeStackLayer* L, int n, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32, int64_t cs_ld,
                         bool batched, const int* kv_start, const bf16_t* w_final, float final_eps, bool tail_norm, bf16_t* out, void* ws,
                         size_t ws_bytes, hipStream_t st) {
  return check_then_run(st, [&](const Step& s) {
    return stack_walk(s, L, n, x, cosp, sinp, cs_is_f32, cs_ld, batched, kv_start, w_final, final_eps, tail_norm, out, ws, ws_bytes);
  });
}

// ------------------------------------------------------------------------------------------------ the head of a decode step
// Everything between the last layer and the next token's logits, for the B <= 64 rows of a step: the stack's final RMSNorm of the
// un-normed hidden rows x (B, E; ldx) into the workspace, then logits (B, V; fp32, ldl) = normed rows . W^T on the few-rows product
// in the head's weight form.  No kernel of its own: rmsnorm_bf16, then gemm_rows with GEMM_OUT_F32 -- the logits are by definition
// the bits of those two calls.
size_t decode_head_workspace_bytes(int B, int E) {
  return B > 0 && B <= 64 && E > 0 ? ((size_t)B * E * sizeof(bf16_t) + 255) & ~(size_t)255 : 0;
}

static RowsArgs head_rows(const DecodeHead& h, const bf16_t* xn, int B, float* logits, int64_t ldl) {
  RowsArgs a;
  a.A = xn; a.W = h.W; a.scale = h.scale; a.form = h.form; a.C = logits;
  a.M = B; a.N = h.V; a.K = h.E;
  a.lda = h.E; a.ldw = h.ldw; a.lds = h.lds; a.ldc = ldl;
  a.flags = GEMM_OUT_F32;
  return a;
}

// (a check walk: every refusal of the head, nothing launched -- its own, the norm's, the product's)
static int head_walk(const Step& s, const DecodeHead& h, const bf16_t* x, int64_t ldx, int B, float* logits, int64_t ldl, void* ws, size_t ws_bytes) {
  if (s.check()) {
    if (!wform_known(h.form) || B <= 0 || B > 64 || h.E <= 0 || h.V < 2 || !x || !h.w_norm || !h.W || !logits || !ws || ((uintptr_t)ws & 15))
      return U2_ERR_ARG;
    if (h.form != WForm::ELEM && !h.scale) return U2_ERR_ARG;
    if (ldx < h.E || ldl < h.V) return U2_ERR_ARG;
  }
  bf16_t* xn = reinterpret_cast<bf16_t*>(ws);
  int e = s.norm(x, h.w_norm, xn, B, h.E, ldx, h.eps);
  if (e == U2_OK) e = s.rows(head_rows(h, xn, B, logits, ldl));
  // (the workspace's size behind the launchers' refusals: the order in which the head has always answered)
  if (e == U2_OK && s.check() && ws_bytes < decode_head_workspace_bytes(B, h.E)) e = U2_ERR_WORKSPACE;
  return e;
}

int decode_head(const DecodeHead& h, const bf16_t* x, int64_t ldx, int B, float* logits, int64_t ldl, void* ws, size_t ws_bytes,
                hipStream_t st) {
  return check_then_run(st, [&](const Step& s) { return head_walk(s, h, x, ldx, B, logits, ldl, ws, ws_bytes); });
}

// The whole-stack step followed by the head, in one call: out (B, E) receives the last layer's hidden rows as they are (the stack
// step with w_final = null), the head norms them and writes the logits.  The workspace is the stack step's followed by the head's.
// The stack's rule holds for both: the layers' DEC_CHECK walk, then the head's checks, and only then the first launch.
size_t decoder_decode_stack_head_workspace_bytes(const DecodeStackLayer* L, int n, const DecodeHead& h) {
  const size_t s = decoder_decode_stack_workspace_bytes(L, n);
  if (s == 0 || h.E != L[0].cfg.E) return 0;
  const size_t hb = decode_head_workspace_bytes(L[0].cfg.B, h.E);
  return hb ? s + hb : 0;
}

int decoder_decode_stack_head(const DecodeStackLayer* L, int n, const bf16_t* x, const void* cosp, const void* sinp, int cs_is_f32,
                              int64_t cs_ld, bool batched, const int* kv_start, bool tail_norm, bf16_t* out, const DecodeHead& h,
                              float* logits, int64_t ldl, void* ws, size_t ws_bytes, hipStream_t st) {
  const size_t sb = decoder_decode_stack_workspace_bytes(L, n);  // (0: null or no layers, descriptors the step refuses)
  if (sb == 0 || !ws || h.E != L[0].cfg.E) return U2_ERR_ARG;
  if (ws_bytes < sb) return U2_ERR_WORKSPACE;
  const int B = L[0].cfg.B;
  void* hws = reinterpret_cast<char*>(ws) + sb;
  return check_then_run(st, [&](const Step& s) {
    const int e = stack_walk(s, L, n, x, cosp, sinp, cs_is_f32, cs_ld, batched, kv_start, nullptr, 0.f, tail_norm, out, ws, sb);
    return e != U2_OK ? e : head_walk(s, h, out, h.E, B, logits, ldl, hws, ws_bytes - sb);
  });
}

}  // namespace u2
