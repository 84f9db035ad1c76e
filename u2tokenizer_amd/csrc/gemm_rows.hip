// The few-rows (weight-streaming) product: 1 .. 64 rows against N x K weights, in three weight forms (kernels.h: WForm) -- the element
// type, e4m3 codes with one fp32 scale per weight row (the decode step's four products read half the bytes; DESIGN f3: the step is
// bound by them), and OCP MXFP4: e2m1 codes with one e8m0 scale per block of 32 k, a quarter of the bytes, widened with their scale
// by one conversion instruction per pair (DESIGN f11).  Weight-only: activations stay in the element type, the MFMA is the element
// type's v_mfma_f32_16x16x32 on weights widened in registers (rows.h), so a product on codes is exactly x . dequant(W) in fp32
// accumulation.  Who calls it: the plan for M <= 16 (gemm.hip: gemm_step -- the ViT's cls rows, the decode step of up to 16
// sequences), the decode step of 17 .. 64 sequences and on e4m3 / e2m1 weights directly (decoder.hip), u2tok_gemm_rows*.  Arithmetic: rows.h -- every block of 16 rows gets the bits of the M <= 16
// product on those rows, so a sequence's tokens do not depend on how many sequences share the step.
#include "rows.h"

namespace u2 {

// The ViT keeps its 8 cls rows behind the 16384 patch rows (pipeline.hip); the big-tile kernel takes the 64 full 256-row
// tiles and leaves those 8 rows to a second launch -- 36 of them per volume (qkv, out-proj, fc2 of 12 blocks).  On the
// 64 x 64 tile kernel such a product is a chain of K / 64 dependent stage-and-wait steps on a few dozen workgroups:
// ~20 us each, latency-bound.  Here a workgroup owns 16 output columns for all NB = ceil(M / 16) blocks of 16 rows ("rows16": blocks
// of 16 rows); its NW waves split the K steps (W8: double steps) and carry NB accumulators each, fed from ONE weight fragment per
// step: every wave loads its weight fragments (the MFMA A operand: 16 rows x 64 contiguous bytes per instruction) and activation
// fragments straight from memory -- all loads of a wave (of a block of steps in flight, rows.h) are issued before its first MFMA,
// so the whole product costs about one memory latency, and every weight byte is read once per product however many rows share it.
// The NB x NW partial tiles go through LDS once; wave b then adds the NW tiles of row block b in slice order (bit-repeatable) and
// runs that block's epilogue: the row scale (W8), then rows_store (alpha, bias, GELU, residual, element / fp32 out) or the pair
// form.  v_mfma_f32_16x16x32 with the weights as A: a lane ends up with 4 consecutive output columns of one row, as in the tile
// kernels.
// PAIR (GEMM_SWIGLU: W = [gate rows | up rows], N = 2 I, C (M, I) = bf16(silu(gate)) * up -- the form the big-tile kernel has for
// the prefill): the workgroup's 16 weight rows are 8 gate rows and the SAME 8 up rows, so the lanes of column groups 0 / 1 hold
// the gates and those of groups 2 / 3 (32 lanes further) the matching ups; the decode step's SwiGLU launch goes away.
// a.W / a.ldw: bytes with codes (e4m3: one per byte, e2m1: two), else elements of the element type.
// NORM (RowsNorm, non-pair alone): after its rows_store every workgroup goes through rows_norm_tail (rows.h) -- release, ticket, and
// in the workgroup that draws the last one the RMSNorm of the M finished rows.  A template parameter, not a branch on a.norm.w: the
// row function keeps a row's 16-byte chunks and the weight's in registers (NC = 8: about 100 VGPRs), and as a branch that tail set
// the register count -- 4 waves per SIMD instead of 5 .. 8, 144 bytes of scratch in the 64-register instantiations -- of every
// product that never asks for a norm.  The 72 instantiations without it are compiled from the text they had (DESIGN f12).
template <int NW, int NB, bool PAIR, WForm F, bool NORM = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(rows_min_waves(NW, NB, F, NORM)))) void gemm_rows16_kernel(RowsArgs a) {
  static_assert(!(PAIR && NORM), "the norm follows the non-pair epilogue");
  __shared__ float red[NB][NW][64][4];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (scalar: the row block of the epilogue too)
  const int l15 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  constexpr bool W8 = F == WForm::E4M3, W4 = F == WForm::E2M1;
  const int nsteps = W4 ? a.K >> 7 : W8 ? a.K >> 6 : a.K >> 5;  // K % 128 == 0 / K % 64 == 0 / K % 32 == 0 (gemm_rows_check, rows16_ok)
  const int per = (nsteps + NW - 1) / NW, s0 = wv * per, s1 = min(nsteps, s0 + per);
  const int I2 = a.N >> 1;
  // the weight row of column c of the workgroup's 16 (PAIR: gate row 8 blk + c for c < 8, up row I + 8 blk + c - 8)
  auto wrow = [&](int c) {
    if constexpr (PAIR) return min((c < 8 ? 0 : I2) + (int)blockIdx.x * 8 + (c & 7), a.N - 1);
    else return min(n0 + c, a.N - 1);
  };
  constexpr int GE = W4 ? 32 : W8 ? 16 : 8;  // elements of a lane group per step: 16 bytes of the weight row in every form
  const char* wp = reinterpret_cast<const char*>(a.W) + (int64_t)wrow(l15) * a.ldw * (W8 || W4 ? 1 : 2) + g * 16;
  const bf16_t* xp[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) xp[b] = a.A + (int64_t)min(16 * b + l15, a.M - 1) * a.lda + g * GE;
  f32x4 acc[NB];
  if constexpr (W4) rows_slice<NB, F>(wp, xp, s0, s1, acc, reinterpret_cast<const uint8_t*>(a.scale) + (int64_t)wrow(l15) * a.lds + g);
  else rows_slice<NB, F>(wp, xp, s0, s1, acc);
  // lane holds C[m = 16 b + l15][column 4 g + r of the workgroup's 16] of every block b
#pragma unroll
  for (int b = 0; b < NB; ++b) *reinterpret_cast<f32x4*>(red[b][wv][lane]) = acc[b];
  __syncthreads();
  const int rb = wv;                          // (NW >= 4 >= NB: a wave per row block)
  const int mb = min(16, a.M - 16 * rb);      // rows of the block (rb < NB: >= 1, NB = ceil(M / 16))
  const int m = 16 * rb + l15;
  auto tile_sum = [&](float (&v)[4]) {        // the NW partial tiles of the row block, in slice order
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += red[rb][w][lane][r];
  };
  auto store = [&](float (&v)[4]) {           // the non-pair epilogue of the lane's 4 columns of row m
    if constexpr (W8) {  // the scaled sum is an fp32 value of its own before the epilogue sees it (alpha = 1 there)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] *= reinterpret_cast<const float*>(a.scale)[wrow(4 * g + r)];
    }
    RowsEpi e = a;
    if constexpr (W8 || W4 || NB > 1) e.alpha = e.alpha_lo = 1.f, e.nsplit = 0;  // (only a plan's step, 16-bit and M <= 16, sets them: constants here)
    rows_store(e, v, m, n0 + 4 * g, reinterpret_cast<char*>(a.C), a.R);
  };
  if constexpr (NORM) {  // the RMSNorm of the finished rows in this launch's tail: every thread gets there, epilogue or not
    if (rb < NB && l15 < mb) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      tile_sum(v);
      store(v);
    }
    rows_norm_tail(a.norm, reinterpret_cast<const bf16_t*>(a.C), a.ldc, a.M, a.N, NW, reinterpret_cast<uint32_t*>(&red[0][0][0][0]));
    return;
  }
  if (rb >= NB) return;
  if (!PAIR && l15 >= mb) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  tile_sum(v);
  if constexpr (PAIR) {  // (all 64 lanes: lanes of rows >= M carry copies of row M - 1 and write nothing)
    auto mult = [&](int r) {
      const int c = 4 * g + r;  // (wrow(c) written out: through the nested lambda <4, 4, true, true> takes 8 more VGPRs and loses a wave)
      if constexpr (W8) return reinterpret_cast<const float*>(a.scale)[min((c < 8 ? 0 : I2) + (int)blockIdx.x * 8 + (c & 7), a.N - 1)];
      else if constexpr (W4) return 1.f;  // (the block scales went in with the conversion)
      else return a.alpha;
    };
    rows_pair_store(v, mult, g < 2 && l15 < mb, m, (int)blockIdx.x * 8 + 4 * g, I2, reinterpret_cast<bf16_t*>(a.C), a.ldc);
    return;
  }
  store(v);
}

// What gemm_rows accepts: one function for all weight forms, the per-form numbers from WFormFacts (kernels.h).
int gemm_rows_check(const RowsArgs& a) {
  if (!wform_known(a.form)) return U2_ERR_ARG;
  const WFormFacts& f = wform_facts(a.form);
  const bool pair = a.flags & GEMM_SWIGLU;
  if (!a.A || !a.W || !a.C || a.M <= 0 || a.M > 64 || a.N <= 0 || a.K <= 0 || a.K % f.k_mult) return U2_ERR_ARG;
  if (a.flags & ~(GEMM_BIAS_N | GEMM_RESIDUAL | GEMM_OUT_F32 | GEMM_SWIGLU)) return U2_ERR_ARG;
  if (pair && (a.flags != GEMM_SWIGLU || (a.N & 15))) return U2_ERR_ARG;  // gate | up: N = 2 I, I % 8 == 0
  if (((a.flags & GEMM_BIAS_N) && !a.bias) || ((a.flags & GEMM_RESIDUAL) && (!a.R || a.ldr < a.N))) return U2_ERR_ARG;
  if (a.lda < a.K || (a.lda & 7) || a.ldw < a.K / f.ldw_div || a.ldw % f.ldw_mult || a.ldc < (pair ? a.N >> 1 : a.N)) return U2_ERR_ARG;
  if (f.scale_bytes && (!a.scale || (uintptr_t)a.scale % f.scale_align || (f.scale_k && a.lds < a.K / f.scale_k))) return U2_ERR_ARG;
  if ((((uintptr_t)a.A | (uintptr_t)a.W) & 15) || ((uintptr_t)a.C & ((a.flags & GEMM_OUT_F32) ? 3 : 1))) return U2_ERR_ARG;
  if (const RowsNorm& n = a.norm; n.w) {  // the norm in the tail: the non-pair form with a residual on element-type rows rmsnorm_row reads
    if (pair || !(a.flags & GEMM_RESIDUAL) || (a.flags & GEMM_OUT_F32) || !n.Yn || !n.ticket || ((uintptr_t)n.ticket & 3)) return U2_ERR_ARG;
    if ((a.N & 7) || a.N > ROWS_NORM_MAX_N || (a.ldc & 7) || n.ld < a.N || (n.ld & 7) || (((uintptr_t)a.C | (uintptr_t)n.w | (uintptr_t)n.Yn) & 15))
      return U2_ERR_ARG;
  }
  return U2_OK;
}

int gemm_rows_launch(const RowsArgs& a, hipStream_t stream) {
  const bool pair = a.flags & GEMM_SWIGLU;
  const int nb = (a.M + 15) >> 4;
  const int nw = rows16_slices(a.K / wform_facts(a.form).k_mult);  // from the (double, quad) steps alone, whatever M: the contract
  // the 72 instantiations: [WForm][PAIR][NW = 16, 8, 4][NB - 1]
#define ROWS_NB(NW, PAIR, F) \
  {gemm_rows16_kernel<NW, 1, PAIR, F>, gemm_rows16_kernel<NW, 2, PAIR, F>, gemm_rows16_kernel<NW, 3, PAIR, F>, gemm_rows16_kernel<NW, 4, PAIR, F>}
#define ROWS_FORM(F) \
  {{ROWS_NB(16, false, F), ROWS_NB(8, false, F), ROWS_NB(4, false, F)}, {ROWS_NB(16, true, F), ROWS_NB(8, true, F), ROWS_NB(4, true, F)}}
  void (*const k[3][2][3][4])(RowsArgs) = {ROWS_FORM(WForm::ELEM), ROWS_FORM(WForm::E4M3), ROWS_FORM(WForm::E2M1)};
#undef ROWS_FORM
#undef ROWS_NB
  // ... and the 36 with the norm in the tail: [WForm][NW = 16, 8, 4][NB - 1]
#define ROWS_NORM_NB(NW, F)                                                                                                           \
  {gemm_rows16_kernel<NW, 1, false, F, true>, gemm_rows16_kernel<NW, 2, false, F, true>, gemm_rows16_kernel<NW, 3, false, F, true>, \
   gemm_rows16_kernel<NW, 4, false, F, true>}
#define ROWS_NORM_FORM(F) {ROWS_NORM_NB(16, F), ROWS_NORM_NB(8, F), ROWS_NORM_NB(4, F)}
  void (*const kn[3][3][4])(RowsArgs) = {ROWS_NORM_FORM(WForm::ELEM), ROWS_NORM_FORM(WForm::E4M3), ROWS_NORM_FORM(WForm::E2M1)};
#undef ROWS_NORM_FORM
#undef ROWS_NORM_NB
  const dim3 grid((unsigned)(pair ? cdiv(a.N >> 1, 8) : cdiv(a.N, 16)));
  const bool norm = a.norm.w && !pair;  // (gemm_rows_check: never on the pair form)
  hipLaunchKernelGGL(norm ? kn[(int)a.form][2 - nw / 8][nb - 1] : k[(int)a.form][pair][2 - nw / 8][nb - 1], grid, dim3(nw * 64), 0, stream, a);
  return launch_status();
}

int gemm_rows(const RowsArgs& a, hipStream_t stream) {
  const int e = gemm_rows_check(a);
  if (e != U2_OK) return e;
  const WFormFacts& f = wform_facts(a.form);
  const bool pair = a.flags & GEMM_SWIGLU;
  const double out_b = pair ? 2.0 * a.M * (a.N >> 1) : ((a.flags & GEMM_OUT_F32) ? 4.0 : 2.0) * a.M * a.N;
  ProfScope ps(PROF_GEMM, 2.0 * a.M * a.N * a.K, stream,
               2.0 * a.M * a.K + f.w_bytes * a.N * a.K + (double)f.scale_bytes * a.N * (f.scale_k ? a.K / f.scale_k : 1) + out_b +
                   ((a.flags & GEMM_RESIDUAL) ? 2.0 * a.M * a.N : 0.0));
  return gemm_rows_launch(a, stream);
}

}  // namespace u2
