// The few-rows product for 16 < M <= 64 rows against N x K weights, in both weight forms: element-type weights (what
// gemm_rows16_kernel, gemm.hip, computes for M <= 16) and e4m3 codes with one fp32 scale per weight row (gemm_rows16_w8_kernel,
// gemm_w8.hip).  The decode step of 17 .. 64 sequences (decoder.hip) is what calls it: weight streaming, every weight byte read
// once per step however many sequences share it.  Arithmetic: rows64.h -- every block of 16 rows gets the bits of the M <= 16
// product on those rows, so a sequence's tokens do not depend on how many sequences share the step.
#include "rows64.h"

namespace u2 {

// A workgroup owns 16 output columns (PAIR: 8 gate rows and the SAME 8 up rows of a packed gate | up weight) for all NB =
// ceil(M / 16) row blocks; its NW waves split the K steps (W8: double steps) and carry NB accumulators each, fed from ONE weight
// fragment per step.  The NB x NW partial tiles go through LDS once; wave b then adds the NW tiles of row block b in slice order
// and runs that block's epilogue: the M <= 16 kernels' own (row scale, rows16_store, the pair form's rounding points).
// a.W / a.ldw: bytes and codes with W8, else elements of the element type.
template <int NW, int NB, bool PAIR, bool W8>
__global__ __launch_bounds__(NW * 64) void gemm_rows64_kernel(RowsW8Args a) {
  __shared__ float red[NB][NW][64][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nsteps = W8 ? a.K >> 6 : a.K >> 5;  // K % 64 == 0 / K % 32 == 0 (launchers)
  const int per = (nsteps + NW - 1) / NW, s0 = wv * per, s1 = min(nsteps, s0 + per);
  const int I2 = a.N >> 1;
  const int nrow = PAIR ? min((l15 < 8 ? 0 : I2) + (int)blockIdx.x * 8 + (l15 & 7), a.N - 1) : min(n0 + l15, a.N - 1);
  constexpr int GE = W8 ? 16 : 8;  // elements of a lane group per step
  const bf16_t* xp[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) xp[b] = a.A + (int64_t)min(16 * b + l15, a.M - 1) * a.lda + g * GE;
  f32x4 acc[NB];
  if constexpr (W8) rows64_w8_slice<NB>(a.W + (int64_t)nrow * a.ldw + g * 16, xp, s0, s1, acc);
  else rows64_slice<NB>(reinterpret_cast<const bf16_t*>(a.W) + (int64_t)nrow * a.ldw + g * 8, xp, s0, s1, acc);
  // lane holds C[m = 16 b + l15][column 4 g + r of the workgroup's 16] of every block b
#pragma unroll
  for (int b = 0; b < NB; ++b) *reinterpret_cast<f32x4*>(red[b][wv][lane]) = acc[b];
  __syncthreads();
  const int rb = wv;                          // (NW >= 4 >= NB: a wave per row block)
  if (rb >= NB) return;
  const int mb = min(16, a.M - 16 * rb);      // rows of the block (>= 1: NB = ceil(M / 16))
  if (!PAIR && l15 >= mb) return;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += red[rb][w][lane][r];
  const int m = 16 * rb + l15;
  if constexpr (PAIR) {  // (all 64 lanes: lanes of rows >= M carry copies of row M - 1 and write nothing)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 4 * g + r;  // the column's weight row: gate row 8 b + c (c < 8), up row I + 8 b + c - 8
      float t = v[r];
      if constexpr (W8) t *= a.scale[min((c < 8 ? 0 : I2) + (int)blockIdx.x * 8 + (c & 7), a.N - 1)];
      const float gate = bf16_to_f32(f32_to_bf16(t));
      const float up = bf16_to_f32(f32_to_bf16(__shfl_xor(t, 32, 64)));  // column group g + 2 of the same row
      const int n = (int)blockIdx.x * 8 + c;
      if (g < 2 && l15 < mb && n < I2) {
        const float sg = gate / (1.0f + __expf(-gate));
        reinterpret_cast<bf16_t*>(a.C)[(int64_t)m * a.ldc + n] = f32_to_bf16(bf16_to_f32(f32_to_bf16(sg)) * up);
      }
    }
    return;
  }
  if constexpr (W8) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= a.scale[min(n0 + 4 * g + r, a.N - 1)];
  }
  GemmDesc d;  // (rows16_store reads these fields only; alpha = 1)
  d.N = a.N; d.flags = a.flags; d.bias = a.bias; d.ldc = a.ldc; d.ldr = a.ldr;
  rows16_store(d, v, m, n0 + 4 * g, reinterpret_cast<char*>(a.C), a.R);
}

template <int NW, bool W8>
static void (*rows64_pick(int nb, bool pair))(RowsW8Args) {
  void (*const k[2][3])(RowsW8Args) = {
      {gemm_rows64_kernel<NW, 2, false, W8>, gemm_rows64_kernel<NW, 3, false, W8>, gemm_rows64_kernel<NW, 4, false, W8>},
      {gemm_rows64_kernel<NW, 2, true, W8>, gemm_rows64_kernel<NW, 3, true, W8>, gemm_rows64_kernel<NW, 4, true, W8>}};
  return k[pair][nb - 2];
}

// arguments checked by the callers (gemm.hip: gemm_rows, gemm_w8.hip: gemm_rows_w8); 16 < a.M <= 64
int gemm_rows64_launch(const RowsW8Args& a, bool w8, hipStream_t stream) {
  if (a.M <= 16 || a.M > 64) return U2_ERR_ARG;
  const bool pair = a.flags & GEMM_SWIGLU;
  const int nb = (a.M + 15) >> 4;
  const int nw = rows16_slices(w8 ? a.K >> 6 : a.K >> 5);  // the M <= 16 kernels' choice: the contract
  const dim3 grid((unsigned)(pair ? cdiv(a.N >> 1, 8) : cdiv(a.N, 16)));
  const double out_b = pair ? 2.0 * a.M * (a.N >> 1) : ((a.flags & GEMM_OUT_F32) ? 4.0 : 2.0) * a.M * a.N;
  ProfScope ps(PROF_GEMM, 2.0 * a.M * a.N * a.K, stream,
               2.0 * a.M * a.K + (w8 ? 1.0 : 2.0) * a.N * a.K + (w8 ? 4.0 * a.N : 0.0) + out_b +
                   ((a.flags & GEMM_RESIDUAL) ? 2.0 * a.M * a.N : 0.0));
  void (*k)(RowsW8Args);
  if (w8) k = nw == 16 ? rows64_pick<16, true>(nb, pair) : nw == 8 ? rows64_pick<8, true>(nb, pair) : rows64_pick<4, true>(nb, pair);
  else k = nw == 16 ? rows64_pick<16, false>(nb, pair) : nw == 8 ? rows64_pick<8, false>(nb, pair) : rows64_pick<4, false>(nb, pair);
  hipLaunchKernelGGL(k, grid, dim3(nw * 64), 0, stream, a);
  return launch_status();
}

}  // namespace u2
