// The arithmetic of the few-rows product (1 .. 64 rows against N x K weights in the element type, as e4m3 codes or as e2m1 codes with
// block scales), shared by
// gemm_rows16_kernel (gemm_rows.hip) and by the big-tile kernel's in-launch tail (gemm_bt.hip, round 5: the ViT's 8 cls rows ride in
// the launch of the 16384 patch rows instead of a launch of their own) -- ONE definition, so that a row's value does not depend on
// which of them computed it, on the weight form's kernel, or on how many row blocks share the pass over K:
//   * K is cut into NW contiguous slices of `per` steps; a slice is ONE accumulator chain of v_mfma_f32_16x16x32 per block of 16
//     rows, in step order (weights as the A operand: a lane ends up with 4 consecutive output columns of one row);
//   * the NW partial 16 x 16 tiles of a row block are added in slice order 0 .. NW - 1, then the epilogue of the product is applied.
// THE CONTRACT for 17 .. 64 rows (NB = 2 .. 4 blocks of 16 rows in ONE pass over K -- a weight fragment is loaded once and feeds NB
// MFMAs, one per row block; the decode step of 17 .. 64 sequences streams its weights once, as the step of 16 does): row m of an M-row
// product has the bits it has as row m % 16 of the M <= 16 product on rows 16 (m / 16) .. min(M, 16 (m / 16) + 16) - 1.  Per
// 16 x 16 tile nothing differs; only the schedule is another (rows_in_flight).
//
// 16-bit weights: a step covers 32 k; lane group g = lane / 16 owns k = 32 s + 8 g .. + 7: one 16-byte load of 8 elements, one MFMA.
//
// OCP e4m3 (1-byte) weights: the same product with the weight operand read as 8-bit codes, widened to the element type in registers
// (every e4m3 value is exact in bf16 and in fp16) and ONE fp32 scale per weight row applied to the cross-wave sum:
// C[m][n] = epilogue(scale[n] * sum_k x[m][k] * e4m3(W8[n][k])), fp32 accumulation.  Nothing in here is lossy beyond the 16-bit
// product's own roundings; the quantiser (ops.quantize_rows_fp8) is.
// THE K MAPPING (weights and activations use the same one, so any k reaches the MFMA on both sides in the same slot):
//   * K is cut into K / 64 DOUBLE STEPS; double step s covers k = 64 s .. 64 s + 63;
//   * lane group g = lane / 16 (0 .. 3) of a double step owns k = 64 s + 16 g .. 64 s + 16 g + 15: ONE 16-byte weight load (16
//     codes) and two 16-byte activation loads;
//   * its first 8 values (k = 64 s + 16 g + 0 .. 7) are the group's 8 K slots of MFMA 1 of the double step, the next 8
//     (k = 64 s + 16 g + 8 .. 15) those of MFMA 2 -- v_mfma_f32_16x16x32 sums its 32 slots, whichever k sits in them.
//   * the double steps are cut into NW contiguous slices (one per wave, `per` double steps each); a slice is one accumulator chain
//     in double-step order, MFMA 1 before MFMA 2; the NW partial tiles are added in slice order 0 .. NW - 1.
//
// OCP MXFP4 (e2m1 codes, two per byte, even k in the low nibble; one e8m0 scale byte per 32 consecutive k of a weight row) weights:
// the same product with the weight operand read as 4-bit codes, widened to the element type in registers WITH the block's scale
// (v_cvt_scalef32_pk_*_fp4: e2m1 x 2^(e - 127) is exact in bf16 and fp16 for every scale the quantiser emits, e - 127 in
// [-23, 13]; outside that range the value is whatever the instruction rounds to).  Nothing is applied after the sum:
// C[m][n] = epilogue(sum_k x[m][k] * e2m1(W4[n][k]) * 2^(S[n][k / 32] - 127)), fp32 accumulation, alpha = 1.
// THE K MAPPING:
//   * K is cut into K / 128 QUAD STEPS; quad step s covers k = 128 s .. 128 s + 127;
//   * lane group g = lane / 16 of a quad step owns k = 128 s + 32 g .. 128 s + 32 g + 31: ONE 16-byte weight load (32 codes) -- exactly
//     one MX block, hence ONE scale byte S[n][4 s + g] per lane and quad step -- and four 16-byte activation loads (64 contiguous
//     bytes of the row);
//   * its values 8 j .. 8 j + 7 (j = 0 .. 3; dword j of the load) are the group's 8 K slots of MFMA j of the quad step;
//   * the scale enters as the conversion's fp32 operand ((uint32)e << 23);
//   * the quad steps are cut into NW contiguous slices (rows16_slices of their number); a slice is one accumulator chain in
//     quad-step order, MFMA 0 .. 3; the NW partial tiles are added in slice order 0 .. NW - 1.
#pragma once
#include <type_traits>
#include "kernels.h"

namespace u2 {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// 8 e4m3 codes (two dwords, ascending k) -> one MFMA fragment of 8 elements: v_cvt_pk_f32_fp8 x 4, the element type's pack x 4
__device__ __forceinline__ bf16x8 w8_widen(uint32_t lo, uint32_t hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  const u32x4 p = {pack2_bf16(a.x, a.y), pack2_bf16(b.x, b.y), pack2_bf16(c.x, c.y), pack2_bf16(d.x, d.y)};
  return __builtin_bit_cast(bf16x8, p);
#else
  (void)lo; (void)hi;
  return bf16x8{};
#endif
}

// 8 e2m1 codes (one dword: ascending k, the even k of a byte in its low nibble) and their block's scale as an fp32 (2^x) -> one MFMA
// fragment of 8 elements: v_cvt_scalef32_pk_{bf16,f16}_fp4 x 4, one per byte -- the instruction emits the low nibble first
__device__ __forceinline__ bf16x8 w4_widen(uint32_t c, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
  const u32x4 p = {__builtin_bit_cast(uint32_t, U2_CVT_SCALE_PK_ELEM_FP4(c, s, 0)), __builtin_bit_cast(uint32_t, U2_CVT_SCALE_PK_ELEM_FP4(c, s, 1)),
                   __builtin_bit_cast(uint32_t, U2_CVT_SCALE_PK_ELEM_FP4(c, s, 2)), __builtin_bit_cast(uint32_t, U2_CVT_SCALE_PK_ELEM_FP4(c, s, 3))};
  return __builtin_bit_cast(bf16x8, p);
#else
  (void)c; (void)s;
  return bf16x8{};
#endif
}

// Steps (W8: double steps) whose loads are in flight before the first MFMA.  One row block: 8 = 16 loads (W8: 8 weight + 16
// activation loads) per lane.  NB > 1: 4 steps = 4 (1 + NB) loads, 2 double steps = 2 weight + 4 NB activation loads, because 8 x
// (1 weight + 4 activation fragments) do not fit the 128 VGPRs a lane of a 16-wave workgroup has.
// e2m1: quad steps of 1 weight + 4 NB activation + 1 scale load: TWO of them for one row block (2 + 8 + 2 loads: 64 .. 76 VGPRs, 6 .. 8
// waves per SIMD; four -- 97 .. 117 VGPRs, 4 waves -- measured 5 to 10 % slower at 16 rows and on the K = 12288 product, equal within
// 2 % elsewhere: DESIGN f11), ONE for NB > 1 (two for NB = 2 measured 5 to 10 % slower at 32 rows).
constexpr int rows_in_flight(int NB, WForm F) {
  return F == WForm::E2M1 ? (NB == 1 ? 2 : 1) : NB == 1 ? 8 : F == WForm::E4M3 ? 2 : 4;
}
// The loop form.  Whole blocks of U steps run without a guard per step (a guarded step lets the compiler sink its loads behind the
// MFMAs before it), then the rest of the slice (< U) is one guarded block; where codes are converted, a scheduling barrier keeps
// every load of a block ahead of its first conversion.  On weights streamed from memory the 16-bit NB > 1 loops are 2 to 11 % faster in
// this form than with every block clamped and guarded (profiles/few_rows_variants.json).  NOT for e4m3 codes with NB > 1
// (rows_guarded): there every block is clamped and guarded and nothing is fenced, because the two-body form with the fence holds
// 2 + 4 NB fragments AND the widened codes at once -- 96 .. 116 VGPRs instead of 42 .. 82, occupancy 4 .. 5 waves per SIMD
// instead of 7 .. 8 in the compiler's resource report; without the fence still 5 .. 6 instead of 7 .. 8.
// e2m1 with NB > 1: one quad step per block, so a block is whole or absent and the two forms are the same loop: the guarded one.
constexpr bool rows_guarded(int NB, WForm F) { return F != WForm::ELEM && NB > 1; }
// The waves per SIMD gemm_rows16_kernel asks the register allocator for.  NW / 4 is what its launch bounds say by themselves (the
// element and e4m3 instantiations compile as without the attribute).  e2m1 with NB > 1 on 4 or 8 waves: 8, the occupancy of the e4m3
// instantiations of the same (NW, NB) -- left alone the allocator keeps all 4 NB activation fragments of a quad step in flight and
// ends at 6 .. 7 waves for NB = 3 / 4; held to 64 registers it still neither spills nor touches scratch (DESIGN f11).
// With the norm in the tail (NORM) the tail sets the register count: what the launch bounds say.
constexpr int rows_min_waves(int NW, int NB, WForm F, bool NORM = false) { return F == WForm::E2M1 && NB > 1 && NW < 16 && !NORM ? 8 : NW / 4; }

// Steps [s0, s1) of one slice for NB row blocks.  wp = the lane's weight row + 16 g bytes (a step is 64 bytes of a weight row in
// every form: 8 elements, 16 or 32 codes per lane group); xp[b] = its activation row of block b + 8 g (e4m3: 16 g, e2m1: 32 g)
// elements; sp (e2m1 alone) = the lane's scale row + g: a step's scale byte is sp[4 step].  A weight
// fragment feeds the NB blocks in block order; a code is widened once for all of them.  The bounds are the same for all lanes of a
// wave; they are moved to scalar registers here, so that the guards below are scalar branches and never EXEC masks around an MFMA
// (MFMA ignores EXEC: as lane values the guards have left a guarded MFMA without its skip-if-EXEC-is-empty branch, a step counted twice).
template <int NB, WForm F>
__device__ __forceinline__ void rows_slice(const char* wp, const bf16_t* const (&xp)[NB], int s0_, int s1_, f32x4 (&acc)[NB],
                                           const uint8_t* sp = nullptr) {
  const int s0 = __builtin_amdgcn_readfirstlane(s0_), s1 = __builtin_amdgcn_readfirstlane(s1_);
  constexpr bool W8 = F == WForm::E4M3, W4 = F == WForm::E2M1;
  constexpr int U = rows_in_flight(NB, F), NX = W4 ? 4 : W8 ? 2 : 1;  // NX: activation fragments (= MFMAs per row block) of a step
  constexpr bool G = rows_guarded(NB, F);
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto block = [&](int sb, auto whole) {
    u32x4 wf[U];
    bf16x8 xf[U][NB][NX];
    uint32_t sf[U];  // (e2m1: the step's scale byte)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int st = decltype(whole)::value ? sb + u : min(sb + u, s1 - 1);
      wf[u] = *reinterpret_cast<const u32x4*>(wp + st * 64);
      if constexpr (W4) sf[u] = sp[4 * st];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int h = 0; h < NX; ++h) xf[u][b][h] = *reinterpret_cast<const bf16x8*>(xp[b] + st * (32 * NX) + 8 * h);
    }
    if constexpr ((W8 || W4) && !G) __builtin_amdgcn_sched_barrier(0);  // every load above is issued before the first conversion / MFMA below
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (decltype(whole)::value || sb + u < s1) {
        bf16x8 w[NX];
        if constexpr (W8) w[0] = w8_widen(wf[u].x, wf[u].y), w[1] = w8_widen(wf[u].z, wf[u].w);
        else if constexpr (W4) {
          const float s = __uint_as_float(sf[u] << 23);
          w[0] = w4_widen(wf[u].x, s), w[1] = w4_widen(wf[u].y, s), w[2] = w4_widen(wf[u].z, s), w[3] = w4_widen(wf[u].w, s);
        } else w[0] = __builtin_bit_cast(bf16x8, wf[u]);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int h = 0; h < NX; ++h) acc[b] = mfma16(w[h], xf[u][b][h], acc[b]);
      }
  };
  int sb = s0;
  if constexpr (G) {
    for (; sb < s1; sb += U) block(sb, std::false_type{});
  } else {
    for (; sb + U <= s1; sb += U) block(sb, std::true_type{});
    if (sb < s1) block(sb, std::false_type{});
  }
}

// epilogue for the lane's 4 columns n = n_first .. n_first + 3 of row m (row index inside C / R / bias_m as handed over)
__device__ __forceinline__ void rows_store(const RowsEpi& e, const float (&v)[4], int m, int n_first, char* C, const bf16_t* R) {
  const bool out_f32 = e.flags & GEMM_OUT_F32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n_first + r;
    if (n >= e.N) break;
    float x = v[r] * (n < e.nsplit ? e.alpha_lo : e.alpha);
    if (e.flags & GEMM_BIAS_M) x += bf16_to_f32(e.bias[m]);
    if (e.flags & GEMM_BIAS_N) x += bf16_to_f32(e.bias[n]);
    if (e.flags & GEMM_GELU) x = gelu_epi(x);
    if (e.flags & GEMM_RESIDUAL) x += bf16_to_f32(R[(int64_t)m * e.ldr + n]);
    if (out_f32) reinterpret_cast<float*>(C)[(int64_t)m * e.ldc + n] = x;
    else reinterpret_cast<bf16_t*>(C)[(int64_t)m * e.ldc + n] = f32_to_bf16(x);
  }
}

// The pair epilogue (GEMM_SWIGLU): C[m][n] = SiLU(gate) * up with the rounding points of swiglu_kernel -- gate and up each rounded
// to the element type, silu rounded before the product, the product rounded on store.  v: the lane's 4 sums; mult(r): the
// multiplier of sum r (alpha, or the weight row's scale), applied before the first rounding.  The lanes of column groups 0 / 1 hold
// the gates of columns n_first .. n_first + 3 < I of row m, those 32 lanes further the matching ups; called by all 64 lanes,
// `writes` picks the gate lanes of real rows.
template <class Mult>
__device__ __forceinline__ void rows_pair_store(const float (&v)[4], Mult mult, bool writes, int m, int n_first, int I, bf16_t* C,
                                                int64_t ldc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float t = v[r] * mult(r);
    const float gate = bf16_to_f32(f32_to_bf16(t));
    const float up = bf16_to_f32(f32_to_bf16(__shfl_xor(t, 32, 64)));  // column group g + 2 of the same row
    const int n = n_first + r;
    if (writes && n < I) {
      const float sg = gate / (1.0f + __expf(-gate));
      C[(int64_t)m * ldc + n] = f32_to_bf16(bf16_to_f32(f32_to_bf16(sg)) * up);
    }
  }
}

// One row of the RMSNorm, by one wave: yp[:] = bf16(xp[:] * rsqrt(mean(xp[:]^2) + eps)) * w (the normalised value is rounded to the
// element type before the product with w).  ONE definition for rmsnorm_kernel (decoder.hip) and for the norm in the tail of the
// few-rows product (rows_norm_tail): lane l holds the 16-byte chunks l, 64 + l, ... of the row (NC of them: C <= NC * 512), adds
// their squares in that order and the wave adds the 64 sums in wave_sum's order -- nothing depends on the block the wave sits in,
// nor on NC beyond the chunks it covers.
template <int NC>
__device__ __forceinline__ void rmsnorm_row(const bf16_t* xp, const bf16_t* w, bf16_t* yp, int C, float eps, int lane) {
  const int nchunk = C >> 3;
  uint4 v[NC];
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = i * 64 + lane;
    v[i] = uint4{0, 0, 0, 0};
    if (c < nchunk) {
      v[i] = *reinterpret_cast<const uint4*>(xp + c * 8);
      const float a0 = bf16lo(v[i].x), a1 = bf16hi(v[i].x), a2 = bf16lo(v[i].y), a3 = bf16hi(v[i].y);
      const float a4 = bf16lo(v[i].z), a5 = bf16hi(v[i].z), a6 = bf16lo(v[i].w), a7 = bf16hi(v[i].w);
      sq += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3 + a4 * a4 + a5 * a5 + a6 * a6 + a7 * a7;
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int c = i * 64 + lane;
    if (c < nchunk) {
      const uint4 uw = *reinterpret_cast<const uint4*>(w + c * 8);
      const uint4 n = uint4{pack2_bf16(bf16lo(v[i].x) * rstd, bf16hi(v[i].x) * rstd), pack2_bf16(bf16lo(v[i].y) * rstd, bf16hi(v[i].y) * rstd),
                            pack2_bf16(bf16lo(v[i].z) * rstd, bf16hi(v[i].z) * rstd), pack2_bf16(bf16lo(v[i].w) * rstd, bf16hi(v[i].w) * rstd)};
      *reinterpret_cast<uint4*>(yp + c * 8) =
          uint4{pack2_bf16(bf16lo(n.x) * bf16lo(uw.x), bf16hi(n.x) * bf16hi(uw.x)), pack2_bf16(bf16lo(n.y) * bf16lo(uw.y), bf16hi(n.y) * bf16hi(uw.y)),
                pack2_bf16(bf16lo(n.z) * bf16lo(uw.z), bf16hi(n.z) * bf16hi(uw.z)), pack2_bf16(bf16lo(n.w) * bf16lo(uw.w), bf16hi(n.w) * bf16hi(uw.w))};
    }
  }
}

// The norm in the tail of the few-rows product (RowsNorm), reached by EVERY thread of the workgroup after its rows_store.  flag: 4
// bytes of LDS nobody reads any more.
//   * every thread fences its stores to C at agent scope (release), the workgroup meets at a barrier, and one thread draws the
//     workgroup's ticket with an atomic add at agent scope: whoever sees that ticket's value sees the workgroup's part of C;
//   * the workgroup whose ticket is the last of the grid (every other part of C has been released before it) fences again (acquire:
//     its loads of C must not be served from lines a compute unit kept from an earlier launch on the same buffer), its NW waves norm
//     the M rows, a wave per row and launch rmsnorm_kernel's row function, and it puts the ticket back to 0 for the next launch
//     (the end of the kernel releases that store; nobody else touches the ticket after the last draw).
// Nobody waits for another workgroup: a workgroup that is not the last leaves.
__device__ __forceinline__ void rows_norm_tail(const RowsNorm& nm, const bf16_t* C, int64_t ldc, int M, int N, int nw, uint32_t* flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();  // (also: the epilogue's reads of the LDS tiles are over before `flag` is written)
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(nm.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *flag = t == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (*flag == 0u) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int lane = threadIdx.x & 63;
  for (int row = threadIdx.x >> 6; row < M; row += nw) {
    const bf16_t* xp = C + (int64_t)row * ldc;
    bf16_t* yp = nm.Yn + (int64_t)row * nm.ld;
    if (N <= 1024) rmsnorm_row<2>(xp, nm.w, yp, N, nm.eps, lane);
    else if (N <= 2048) rmsnorm_row<4>(xp, nm.w, yp, N, nm.eps, lane);
    else rmsnorm_row<8>(xp, nm.w, yp, N, nm.eps, lane);
  }
  if (threadIdx.x == 0) __hip_atomic_store(nm.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  (void)nm; (void)C; (void)ldc; (void)M; (void)N; (void)nw; (void)flag;
#endif
}

__host__ __device__ inline int rows16_slices(int nsteps) { return nsteps >= 64 ? 16 : nsteps >= 16 ? 8 : 4; }  // (the launcher's choice of NW)

// the epilogue fields of a plan's product
__host__ __device__ inline RowsEpi rows_epi(const GemmDesc& d) {
  RowsEpi e;
  e.bias = d.bias; e.N = d.N; e.flags = d.flags; e.nsplit = d.nsplit;
  e.ldc = d.ldc; e.ldr = d.ldr; e.alpha = d.alpha; e.alpha_lo = d.alpha_lo;
  return e;
}

}  // namespace u2
