// The arithmetic of the few-rows product on OCP e4m3 (1-byte) weights: rows16.h's product with the weight operand read as 8-bit
// codes, widened to the element type in registers (every e4m3 value is exact in bf16 and in fp16) and ONE fp32 scale per weight
// row applied to the cross-wave sum:  C[m][n] = epilogue(scale[n] * sum_k x[m][k] * e4m3(W8[n][k])), fp32 accumulation.  Nothing
// in here is lossy beyond rows16.h's own roundings; the quantiser (ops.quantize_rows_fp8) is.
//
// THE K MAPPING (weights and activations use the same one, so any k reaches the MFMA on both sides in the same slot):
//   * K is cut into K / 64 DOUBLE STEPS; double step s covers k = 64 s .. 64 s + 63;
//   * lane group g = lane / 16 (0 .. 3) of a double step owns k = 64 s + 16 g .. 64 s + 16 g + 15: ONE 16-byte weight load (16
//     codes) and two 16-byte activation loads;
//   * its first 8 values (k = 64 s + 16 g + 0 .. 7) are the group's 8 K slots of MFMA 1 of the double step, the next 8
//     (k = 64 s + 16 g + 8 .. 15) those of MFMA 2 -- v_mfma_f32_16x16x32 sums its 32 slots, whichever k sits in them.
//   * the double steps are cut into NW contiguous slices (one per wave, `per` double steps each); a slice is one accumulator chain
//     in double-step order, MFMA 1 before MFMA 2; the NW partial tiles are added in slice order 0 .. NW - 1.
#pragma once
#include <type_traits>
#include "rows16.h"

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

// double steps [s0, s1) of one slice; wp = the lane's weight row + 16 g bytes, xp = its activation row + 16 g elements; 8 double
// steps = 8 weight + 16 activation loads per lane in flight before the first MFMA.  Whole blocks of 8 run without a guard per step
// (a guarded step lets the compiler sink its loads behind the MFMAs before it); the rest of the slice (< 8) is one guarded block.
__device__ __forceinline__ f32x4 rows16_w8_slice(const uint8_t* wp, const bf16_t* xp, int s0, int s1) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = 8;
  auto block = [&](int sb, auto whole) {
    u32x4 wf[U];
    bf16x8 xf[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int st = decltype(whole)::value ? sb + u : min(sb + u, s1 - 1);
      wf[u] = *reinterpret_cast<const u32x4*>(wp + st * 64);
      xf[u][0] = *reinterpret_cast<const bf16x8*>(xp + st * 64);
      xf[u][1] = *reinterpret_cast<const bf16x8*>(xp + st * 64 + 8);
    }
    __builtin_amdgcn_sched_barrier(0);  // every load above is issued before the first conversion / MFMA below
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (decltype(whole)::value || sb + u < s1) {
        acc = mfma16(w8_widen(wf[u].x, wf[u].y), xf[u][0], acc);
        acc = mfma16(w8_widen(wf[u].z, wf[u].w), xf[u][1], acc);
      }
  };
  int sb = s0;
  for (; sb + U <= s1; sb += U) block(sb, std::true_type{});
  if (sb < s1) block(sb, std::false_type{});
  return acc;
}

}  // namespace u2
