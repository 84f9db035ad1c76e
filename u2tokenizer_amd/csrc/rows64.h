// The few-rows product for 17 .. 64 activation rows: rows16.h / rows16_w8.h's arithmetic on NB = 2 .. 4 blocks of 16 rows in ONE
// pass over K -- a weight fragment is loaded once and feeds NB MFMAs, one per row block (the decode step of 17 .. 64 sequences
// streams its weights once, as the step of 16 does).
// THE CONTRACT: row m of an M-row product has the bits it has as row m % 16 of the M <= 16 product on rows 16 (m / 16) ..
// min(M, 16 (m / 16) + 16) - 1.  Per 16 x 16 tile nothing differs from rows16_slice / rows16_w8_slice: the same NW =
// rows16_slices(steps) contiguous K slices of `per` steps, one v_mfma_f32_16x16x32 accumulator chain per slice in step order (e4m3:
// double steps, MFMA 1 before MFMA 2), the partial tiles added in slice order 0 .. NW - 1 by the kernels (gemm_rows64.hip), then
// rows16_store / the pair epilogue / the row scale.  Only the schedule is another: U = 4 steps (2 double steps) in flight instead
// of 8, because 8 x (1 weight + 4 activation fragments) do not fit the 128 VGPRs a lane of a 16-wave workgroup has.
#pragma once
#include "rows16_w8.h"

namespace u2 {

// steps [s0, s1) of one slice for NB row blocks; wp = the lane's weight row + 8 g elements, xp[b] = its activation row of block b
// + 8 g elements; 4 steps = 4 (1 + NB) loads per lane in flight
template <int NB>
__device__ __forceinline__ void rows64_slice(const bf16_t* wp, const bf16_t* const (&xp)[NB], int s0, int s1, f32x4 (&acc)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int U = 4;
  for (int sb = s0; sb < s1; sb += U) {
    bf16x8 wf[U], xf[U][NB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int st = min(sb + u, s1 - 1);
      wf[u] = *reinterpret_cast<const bf16x8*>(wp + st * 32);
#pragma unroll
      for (int b = 0; b < NB; ++b) xf[u][b] = *reinterpret_cast<const bf16x8*>(xp[b] + st * 32);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (sb + u < s1) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = mfma16(wf[u], xf[u][b], acc[b]);
      }
  }
}

// double steps [s0, s1) of one slice on e4m3 weights (rows16_w8.h's K mapping); wp = the lane's weight row + 16 g bytes, xp[b] =
// its activation row of block b + 16 g elements; 2 double steps = 2 weight + 4 NB activation loads per lane in flight; a code is
// widened once for all row blocks
template <int NB>
__device__ __forceinline__ void rows64_w8_slice(const uint8_t* wp, const bf16_t* const (&xp)[NB], int s0, int s1, f32x4 (&acc)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int U = 2;
  for (int sb = s0; sb < s1; sb += U) {
    u32x4 wf[U];
    bf16x8 xf[U][NB][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int st = min(sb + u, s1 - 1);
      wf[u] = *reinterpret_cast<const u32x4*>(wp + st * 64);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        xf[u][b][0] = *reinterpret_cast<const bf16x8*>(xp[b] + st * 64);
        xf[u][b][1] = *reinterpret_cast<const bf16x8*>(xp[b] + st * 64 + 8);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (sb + u < s1) {
        const bf16x8 w0 = w8_widen(wf[u].x, wf[u].y), w1 = w8_widen(wf[u].z, wf[u].w);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          acc[b] = mfma16(w0, xf[u][b][0], acc[b]);
          acc[b] = mfma16(w1, xf[u][b][1], acc[b]);
        }
      }
  }
}

}  // namespace u2
