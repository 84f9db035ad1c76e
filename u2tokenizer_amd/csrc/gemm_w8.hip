// The few-rows product (M <= 16 rows against N x K weights; gemm.hip: gemm_rows16_kernel; 17 .. 64 rows: gemm_rows64.hip) on e4m3 weights with one fp32 scale per
// weight row -- the decode step's four weight-streaming products read half the bytes (DESIGN f3: the step is bound by them).
// Weight-only: activations stay in the element type, the MFMA is the element type's v_mfma_f32_16x16x32 on weights widened in
// registers (rows16_w8.h), so the product is exactly x . dequant(W8) in fp32 accumulation.  A launcher of its own (RowsW8Args),
// outside GemmDesc and the plan.
#include "rows16_w8.h"

namespace u2 {

// A workgroup owns 16 output columns (PAIR: 8 gate rows and the SAME 8 up rows of a packed gate | up weight, as
// gemm_rows16_kernel<., true>); its NW waves split the double steps; partial tiles through LDS in wave order; then the row scale,
// then rows16_store's epilogue (bias_n, residual, element / fp32 out) or SiLU(gate) * up with the rounding points of swiglu_kernel.
template <int NW, bool PAIR>
__global__ __launch_bounds__(NW * 64) void gemm_rows16_w8_kernel(RowsW8Args a) {
  __shared__ float red[NW][64][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nd = a.K >> 6;  // K % 64 == 0 (launcher)
  const int per = (nd + NW - 1) / NW, s0 = wv * per, s1 = min(nd, s0 + per);
  const int I2 = a.N >> 1;
  const int nrow = PAIR ? min((l15 < 8 ? 0 : I2) + (int)blockIdx.x * 8 + (l15 & 7), a.N - 1) : min(n0 + l15, a.N - 1);
  const int mrow = min(l15, a.M - 1);
  const f32x4 acc = rows16_w8_slice(a.W + (int64_t)nrow * a.ldw + g * 16, a.A + (int64_t)mrow * a.lda + g * 16, s0, s1);
  // lane holds C[m = l15][column 4 g + r of the workgroup's 16]
  red[wv][lane][0] = acc[0]; red[wv][lane][1] = acc[1]; red[wv][lane][2] = acc[2]; red[wv][lane][3] = acc[3];
  __syncthreads();
  if (wv != 0 || (!PAIR && l15 >= a.M)) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += red[w][lane][r];
  const int m = l15;
  if constexpr (PAIR) {  // (wave 0, all 64 lanes: lanes of rows >= M carry copies of row M - 1 and write nothing)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 4 * g + r;  // the column's weight row: gate row 8 b + c (c < 8), up row I + 8 b + c - 8
      const float t = v[r] * a.scale[min((c < 8 ? 0 : I2) + (int)blockIdx.x * 8 + (c & 7), a.N - 1)];
      const float gate = bf16_to_f32(f32_to_bf16(t));
      const float up = bf16_to_f32(f32_to_bf16(__shfl_xor(t, 32, 64)));  // column group g + 2 of the same row
      const int n = (int)blockIdx.x * 8 + c;
      if (g < 2 && l15 < a.M && n < I2) {
        const float sg = gate / (1.0f + __expf(-gate));
        reinterpret_cast<bf16_t*>(a.C)[(int64_t)m * a.ldc + n] = f32_to_bf16(bf16_to_f32(f32_to_bf16(sg)) * up);
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] *= a.scale[min(n0 + 4 * g + r, a.N - 1)];
  GemmDesc d;  // (rows16_store reads these fields only)
  d.N = a.N; d.flags = a.flags; d.bias = a.bias; d.ldc = a.ldc; d.ldr = a.ldr;
  rows16_store(d, v, m, n0 + 4 * g, reinterpret_cast<char*>(a.C), a.R);
}

int gemm_rows_w8_check(const RowsW8Args& a) {
  const bool pair = a.flags & GEMM_SWIGLU;
  if (!a.A || !a.W || !a.scale || !a.C || a.M <= 0 || a.M > 64 || a.N <= 0 || a.K <= 0 || (a.K & 63)) return U2_ERR_ARG;
  if (a.flags & ~(GEMM_BIAS_N | GEMM_RESIDUAL | GEMM_OUT_F32 | GEMM_SWIGLU)) return U2_ERR_ARG;
  if (pair && (a.flags != GEMM_SWIGLU || (a.N & 15))) return U2_ERR_ARG;  // gate | up: N = 2 I, I % 8 == 0
  if (((a.flags & GEMM_BIAS_N) && !a.bias) || ((a.flags & GEMM_RESIDUAL) && (!a.R || a.ldr < a.N))) return U2_ERR_ARG;
  if (a.lda < a.K || (a.lda & 7) || a.ldw < a.K || (a.ldw & 15) || a.ldc < (pair ? a.N >> 1 : a.N)) return U2_ERR_ARG;
  if ((((uintptr_t)a.A | (uintptr_t)a.W) & 15) || ((uintptr_t)a.scale & 3) || ((uintptr_t)a.C & ((a.flags & GEMM_OUT_F32) ? 3 : 1)))
    return U2_ERR_ARG;
  return U2_OK;
}

int gemm_rows_w8(const RowsW8Args& a, hipStream_t stream) {
  const int e = gemm_rows_w8_check(a);
  if (e != U2_OK) return e;
  if (a.M > 16) return gemm_rows64_launch(a, true, stream);  // 17 .. 64 rows: the same arithmetic per block of 16 (rows64.h)
  const bool pair = a.flags & GEMM_SWIGLU;
  const int nw = rows16_slices(a.K >> 6);  // from the double steps, as rows16_slices picks it from the steps of the 16-bit product
  const dim3 grid((unsigned)(pair ? cdiv(a.N >> 1, 8) : cdiv(a.N, 16)));
  const double out_b = pair ? 2.0 * a.M * (a.N >> 1) : ((a.flags & GEMM_OUT_F32) ? 4.0 : 2.0) * a.M * a.N;
  ProfScope ps(PROF_GEMM, 2.0 * a.M * a.N * a.K, stream,
               2.0 * a.M * a.K + (double)a.N * a.K + 4.0 * a.N + out_b + ((a.flags & GEMM_RESIDUAL) ? 2.0 * a.M * a.N : 0.0));
  void (*const k[2][3])(RowsW8Args) = {
      {gemm_rows16_w8_kernel<16, true>, gemm_rows16_w8_kernel<8, true>, gemm_rows16_w8_kernel<4, true>},
      {gemm_rows16_w8_kernel<16, false>, gemm_rows16_w8_kernel<8, false>, gemm_rows16_w8_kernel<4, false>}};
  hipLaunchKernelGGL(k[!pair][2 - nw / 8], grid, dim3(nw * 64), 0, stream, a);
  return launch_status();
}

}  // namespace u2
