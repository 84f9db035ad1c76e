// Rank-r adapter (LoRA) products for the decoder training route: three bandwidth-bound kernels whose small operand has r in
// {16, 32, 64} rows or columns (include/u2tok.h: u2tok_lora_down / u2tok_lora_up / u2tok_lora_wgrad).  They do not go through the
// GEMM plan: a rank-16 panel on a 128 x 128 tile wastes 7/8 of every MFMA, and the K-major forms want dimensions a 16-wide operand
// meets only by accident.  Common rules: 16-bit operands in the build's element type, fp32 accumulation on v_mfma_f32_16x16x32
// (mfma16 of common.h, the fragment maps of rows.h: the small operand is the A operand, so a lane ends up with 4 consecutive
// values of the small dimension or of the output row), ONE rounding at the store, no atomics and a fixed order of every sum (two
// calls give the same bits), row-strided operands with unit column stride, so that a column segment of a packed q|k|v or gate|up
// buffer is read and written in place.
//
//   down   U (M, r) = alpha X (M, K) A (r, K)^T.  One workgroup per 16 rows of X; K is cut into `nw` contiguous slices of 32-wide
//          steps, one wave and one accumulator chain per slice (rows.h with the roles exchanged: U^T = A X^T), 8 / (r / 16) steps
//          of loads in flight per lane; the slices' 16 x r tiles are added through LDS in slice order.  X is read once, 64
//          contiguous bytes per row and step; A (r x K, L2 resident) once per workgroup.
//   up     Y (M, N) = [Y +] alpha U (M, r) W (N, r)^T.  No reduction across waves: a wave owns 16 rows x 64 columns at a time.  The
//          A operand rows of its four MFMAs are the columns n = base + 16 (i / 4) + 4 t + i % 4 (tile t, operand row i), which
//          leaves lane group g with the 16 CONSECUTIVE columns base + 16 g .. + 15 of its row: 32 contiguous bytes per lane, 128
//          per row, both for the read of the accumulate form and for the store.  r = 16 runs the 32-deep MFMA with the upper
//          half of the contraction zero.
//   wgrad  G (r, C) = alpha U (M, r)^T X (M, C), the contraction over the ROWS.  Both operands are strided along the contraction, so
//          a workgroup stages 128 rows x 64 columns of X and 128 x r of U in LDS with 16-byte global loads (the next tile's loads
//          are issued before the current tile's MFMAs) and its lanes gather their 8-row fragments from there; each of the 4 waves
//          takes 32 of the 128 rows, the waves' tiles are added in wave order.  With a workspace the rows are also cut across
//          workgroups (fixed ranges, fp32 partial tiles, a second launch adds them in range order), so that a 64-column strip does
//          not leave most of the chip idle.
#include <algorithm>
#include "../../include/u2tok.h"
#include "common.h"

namespace u2 {
namespace {

__device__ __forceinline__ bf16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

// ------------------------------------------------------------------------------------------------------------------ down
template <int R16>
__global__ __launch_bounds__(1024) void lora_down_kernel(const bf16_t* __restrict__ X, int64_t ldx, const bf16_t* __restrict__ A,
                                                         int64_t lda, bf16_t* __restrict__ U, int64_t ldu, int M, int nsteps, int per,
                                                         float alpha) {
  extern __shared__ f32x4 down_red[];   // [nw][R16][64]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * 16;
  const bf16_t* xp = X + (int64_t)min(m0 + i, M - 1) * ldx + 8 * g;   // (rows past M repeat the last one; never stored)
  const bf16_t* ap = A + (int64_t)i * lda + 8 * g;
  const int s0 = w * per, s1 = min(s0 + per, nsteps);
  f32x4 acc[R16];
#pragma unroll
  for (int t = 0; t < R16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int UN = 8 / R16;
  for (int sb = s0; sb < s1; sb += UN) {
    bf16x8 xf[UN], af[UN][R16];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int st = min(sb + u, s1 - 1);
      xf[u] = ld8(xp + st * 32);
#pragma unroll
      for (int t = 0; t < R16; ++t) af[u][t] = ld8(ap + (int64_t)t * 16 * lda + st * 32);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u)
      if (sb + u < s1) {
#pragma unroll
        for (int t = 0; t < R16; ++t) acc[t] = mfma16(af[u][t], xf[u], acc[t]);
      }
  }
#pragma unroll
  for (int t = 0; t < R16; ++t) down_red[(w * R16 + t) * 64 + lane] = acc[t];
  __syncthreads();
  // D[row = adapter row 16 t + 4 g + reg][col = row m0 + i of X]: the lane's 4 values are consecutive in U's row
  for (int t = w; t < R16; t += nw) {
    f32x4 s = down_red[t * 64 + lane];
    for (int v = 1; v < nw; ++v) s += down_red[(v * R16 + t) * 64 + lane];
    if (m0 + i < M) {
      uint2 o = {pack2_bf16(s[0] * alpha, s[1] * alpha), pack2_bf16(s[2] * alpha, s[3] * alpha)};
      *reinterpret_cast<uint2*>(U + (int64_t)(m0 + i) * ldu + 16 * t + 4 * g) = o;
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------- up
constexpr int UP_WAVES = 4, UP_UNITS = 2;   // a workgroup: 16 rows x 4 waves x 2 units x 64 columns

template <int KS>
__global__ __launch_bounds__(64 * UP_WAVES) void lora_up_kernel(const bf16_t* __restrict__ U, int64_t ldu, const bf16_t* __restrict__ W,
                                                                int64_t ldw, bf16_t* Y, int64_t ldy, int M, int N, int r, float alpha,
                                                                int accumulate) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int m = blockIdx.y * 16 + i;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 uf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int k0 = 32 * ks + 8 * g;
    uf[ks] = k0 < r ? ld8(U + (int64_t)min(m, M - 1) * ldu + k0) : zero;
  }
#pragma unroll
  for (int unit = 0; unit < UP_UNITS; ++unit) {
    const int nbase = ((blockIdx.x * UP_WAVES + w) * UP_UNITS + unit) * 64;
    if (nbase >= N) break;
    const bool live = m < M && nbase + 16 * g < N;   // (N % 16 == 0: a lane's 16 columns are inside or outside together)
    bf16_t* yp = Y + (int64_t)m * ldy + nbase + 16 * g;
    uint4 y0 = {0, 0, 0, 0}, y1 = {0, 0, 0, 0};
    if (live && accumulate) {
      y0 = *reinterpret_cast<const uint4*>(yp);
      y1 = *reinterpret_cast<const uint4*>(yp + 8);
    }
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int n = min(nbase + 16 * (i >> 2) + 4 * t + (i & 3), N - 1);   // (columns past N repeat the last one; never stored)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int k0 = 32 * ks + 8 * g;
        const bf16x8 wf = k0 < r ? ld8(W + (int64_t)n * ldw + k0) : zero;
        acc[t] = mfma16(wf, uf[ks], acc[t]);
      }
    }
    if (live) {
      // acc[t][reg] = column nbase + 16 g + 4 t + reg of row m
      const uint32_t yin[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
      uint32_t o[8];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        o[2 * t] = pack2_bf16(__builtin_fmaf(alpha, acc[t][0], bf16lo(yin[2 * t])), __builtin_fmaf(alpha, acc[t][1], bf16hi(yin[2 * t])));
        o[2 * t + 1] = pack2_bf16(__builtin_fmaf(alpha, acc[t][2], bf16lo(yin[2 * t + 1])),
                                  __builtin_fmaf(alpha, acc[t][3], bf16hi(yin[2 * t + 1])));
      }
      *reinterpret_cast<uint4*>(yp) = uint4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<uint4*>(yp + 8) = uint4{o[4], o[5], o[6], o[7]};
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- wgrad
constexpr int WG_ROWS = 128, WG_COLS = 64, WG_XS = WG_COLS + 4;   // LDS row strides of 8 (mod 16) bytes: 8-byte writes, the four
                                                                  // lane groups' 8-row offsets fall on two bank sets instead of one
template <int R16>
struct WgradSmem {
  static constexpr int US = 16 * R16 + 4;
  static constexpr int stage = WG_ROWS * (WG_XS + US) * 2, red = 3 * R16 * 4 * 64 * 16;
  static constexpr int bytes = stage > red ? stage : red;
};

__device__ __forceinline__ void st_lds8(bf16_t* p, uint4 v) {   // 16 bytes to an 8-byte aligned LDS address
  reinterpret_cast<uint2*>(p)[0] = uint2{v.x, v.y};
  reinterpret_cast<uint2*>(p)[1] = uint2{v.z, v.w};
}

template <int R16>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const bf16_t* __restrict__ U, int64_t ldu, const bf16_t* __restrict__ X,
                                                         int64_t ldx, void* G, int64_t ldg, float* part, int M, int C, int rows_per_split,
                                                         float alpha, int out_f32) {
  constexpr int r = 16 * R16, US = WgradSmem<R16>::US, UCH = r / 8;    // UCH: 16-byte chunks per row of U
  constexpr int XL = WG_ROWS * (WG_COLS / 8) / 256, UL = WG_ROWS * UCH / 256;   // chunks per thread: 4 and 1 / 2 / 4
  __shared__ __attribute__((aligned(16))) unsigned char smem[WgradSmem<R16>::bytes];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);
  bf16_t* us = xs + WG_ROWS * WG_XS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * WG_COLS;
  const int mbeg = blockIdx.y * rows_per_split, mend = min(M, mbeg + rows_per_split);
  const uint4 zero4 = {0, 0, 0, 0};
  uint4 xr[XL], ur[UL];

  auto fetch = [&](int mt) {   // rows mt .. mt + 127 -> registers (zeros past mend / past column C)
#pragma unroll
    for (int p = 0; p < XL; ++p) {
      const int q = tid + 256 * p, row = mt + (q >> 3), c = c0 + 8 * (q & 7);
      xr[p] = row < mend && c < C ? *reinterpret_cast<const uint4*>(X + (int64_t)row * ldx + c) : zero4;
    }
#pragma unroll
    for (int p = 0; p < UL; ++p) {
      const int q = tid + 256 * p, row = mt + q / UCH;
      ur[p] = row < mend ? *reinterpret_cast<const uint4*>(U + (int64_t)row * ldu + 8 * (q % UCH)) : zero4;
    }
  };

  f32x4 acc[R16][4];
#pragma unroll
  for (int t = 0; t < R16; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(mbeg);
  for (int mt = mbeg; mt < mend; mt += WG_ROWS) {
#pragma unroll
    for (int p = 0; p < XL; ++p) {
      const int q = tid + 256 * p;
      st_lds8(xs + (q >> 3) * WG_XS + 8 * (q & 7), xr[p]);
    }
#pragma unroll
    for (int p = 0; p < UL; ++p) {
      const int q = tid + 256 * p;
      st_lds8(us + (q / UCH) * US + 8 * (q % UCH), ur[p]);
    }
    __syncthreads();
    if (mt + WG_ROWS < mend) fetch(mt + WG_ROWS);
    // the wave's 32 rows of the tile: element j of lane group g is row 32 w + 8 g + j for both operands
    const bf16_t* xk = xs + (32 * w + 8 * g) * WG_XS + i;
    const bf16_t* uk = us + (32 * w + 8 * g) * US + i;
    bf16x8 bf[4], af[R16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) bf[ct][j] = (short)xk[j * WG_XS + 16 * ct];
#pragma unroll
      for (int t = 0; t < R16; ++t) af[t][j] = (short)uk[j * US + 16 * t];
    }
#pragma unroll
    for (int t = 0; t < R16; ++t)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[t][ct] = mfma16(af[t], bf[ct], acc[t][ct]);
    __syncthreads();
  }

  // the four waves' tiles, added in wave order by wave 0 (the staging tiles are dead: the last loop iteration ended on a barrier)
  f32x4* red = reinterpret_cast<f32x4*>(smem);
  if (w > 0) {
#pragma unroll
    for (int t = 0; t < R16; ++t)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) red[(((w - 1) * R16 + t) * 4 + ct) * 64 + lane] = acc[t][ct];
  }
  __syncthreads();
  if (w > 0) return;
  const bool direct = part == nullptr;
#pragma unroll
  for (int t = 0; t < R16; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 s = acc[t][ct];
      for (int v = 0; v < 3; ++v) s += red[((v * R16 + t) * 4 + ct) * 64 + lane];
      const int c = c0 + 16 * ct + i;   // D[row = 16 t + 4 g + reg][col = c]
      if (c >= C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * t + 4 * g + e;
        if (!direct) part[((int64_t)blockIdx.y * r + row) * C + c] = s[e];
        else if (out_f32) reinterpret_cast<float*>(G)[(int64_t)row * ldg + c] = s[e] * alpha;
        else reinterpret_cast<bf16_t*>(G)[(int64_t)row * ldg + c] = f32_to_bf16(s[e] * alpha);
      }
    }
}

// the row ranges' partial tiles, added in range order
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ part, void* G, int64_t ldg, int r, int C, int splits,
                                                                float alpha, int out_f32) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)r * C) return;
  float s = part[idx];
  for (int v = 1; v < splits; ++v) s += part[(int64_t)v * r * C + idx];
  const int row = (int)(idx / C), c = (int)(idx % C);
  if (out_f32) reinterpret_cast<float*>(G)[(int64_t)row * ldg + c] = s * alpha;
  else reinterpret_cast<bf16_t*>(G)[(int64_t)row * ldg + c] = f32_to_bf16(s * alpha);
}

inline bool rank_ok(int r) { return r == 16 || r == 32 || r == 64; }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace u2

using namespace u2;

extern "C" {

int u2tok_lora_down(const void* X, int64_t x_off, int64_t ldx, const void* A, int64_t lda, void* U, int64_t ldu, int32_t M, int32_t K,
                    int32_t r, float alpha, u2tok_stream_t stream) {
  if (!X || !A || !U || M < 1 || K < 32 || K % 32 || !rank_ok(r) || x_off < 0 || x_off % 8 || ldx % 8 || lda % 8 || ldu % 8 || ldx < K ||
      lda < K || ldu < r || (int64_t)M > (int64_t)65535 * 16 || !al16(X) || !al16(A) || !al16(U))
    return U2_ERR_ARG;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(X) + x_off;
  const int nsteps = K / 32, R16 = r / 16;
  int nw = nsteps >= 64 ? 16 : nsteps >= 16 ? 8 : nsteps >= 4 ? 4 : 1;
  if (R16 == 4 && nw > 8) nw = 8;   // (the reduction tile: nw x r / 16 KB of LDS)
  const int per = (nsteps + nw - 1) / nw;
  const dim3 grid((unsigned)((M + 15) / 16)), block(64 * nw);
  const size_t lds = (size_t)nw * R16 * 64 * sizeof(f32x4);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bf16_t* a = reinterpret_cast<const bf16_t*>(A);
  bf16_t* u = reinterpret_cast<bf16_t*>(U);
  if (R16 == 1) hipLaunchKernelGGL(lora_down_kernel<1>, grid, block, lds, st, x, ldx, a, lda, u, ldu, M, nsteps, per, alpha);
  else if (R16 == 2) hipLaunchKernelGGL(lora_down_kernel<2>, grid, block, lds, st, x, ldx, a, lda, u, ldu, M, nsteps, per, alpha);
  else hipLaunchKernelGGL(lora_down_kernel<4>, grid, block, lds, st, x, ldx, a, lda, u, ldu, M, nsteps, per, alpha);
  return launch_status();
}

int u2tok_lora_up(const void* U, int64_t ldu, const void* W, int64_t ldw, void* Y, int64_t y_off, int64_t ldy, int32_t M, int32_t N,
                  int32_t r, float alpha, int32_t accumulate, u2tok_stream_t stream) {
  if (!U || !W || !Y || M < 1 || N < 16 || N % 16 || !rank_ok(r) || y_off < 0 || y_off % 8 || ldu % 8 || ldw % 8 || ldy % 8 || ldu < r ||
      ldw < r || ldy < N || (int64_t)M > (int64_t)65535 * 16 || !al16(U) || !al16(W) || !al16(Y))
    return U2_ERR_ARG;
  const dim3 grid((unsigned)((N + 64 * UP_WAVES * UP_UNITS - 1) / (64 * UP_WAVES * UP_UNITS)), (unsigned)((M + 15) / 16)), block(64 * UP_WAVES);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bf16_t* u = reinterpret_cast<const bf16_t*>(U);
  const bf16_t* w = reinterpret_cast<const bf16_t*>(W);
  bf16_t* y = reinterpret_cast<bf16_t*>(Y) + y_off;
  if (r <= 32) hipLaunchKernelGGL(lora_up_kernel<1>, grid, block, 0, st, u, ldu, w, ldw, y, ldy, M, N, r, alpha, accumulate != 0);
  else hipLaunchKernelGGL(lora_up_kernel<2>, grid, block, 0, st, u, ldu, w, ldw, y, ldy, M, N, r, alpha, accumulate != 0);
  return launch_status();
}

int u2tok_lora_wgrad(const void* U, int64_t ldu, const void* X, int64_t x_off, int64_t ldx, void* G, int64_t ldg, int32_t M, int32_t C,
                     int32_t r, float alpha, int32_t out_f32, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  if (!U || !X || !G || M < 1 || C < 8 || C % 8 || !rank_ok(r) || x_off < 0 || x_off % 8 || ldu % 8 || ldx % 8 || ldu < r || ldx < C ||
      ldg < C || !al16(U) || !al16(X) || (reinterpret_cast<uintptr_t>(G) & (out_f32 ? 3 : 1)) || (workspace && !al16(workspace)))
    return U2_ERR_ARG;
  const int strips = (C + WG_COLS - 1) / WG_COLS, tiles = (M + WG_ROWS - 1) / WG_ROWS;
  // row ranges: enough workgroups for ~2 per CU, as far as the workspace (one fp32 (r, C) tile per range) allows
  int64_t splits = std::min<int64_t>(tiles, std::max(1, 512 / strips));
  const int64_t cap = workspace ? (int64_t)(workspace_bytes / ((size_t)r * C * sizeof(float))) : 0;
  splits = std::min(splits, cap);
  int rps = M;
  if (splits > 1) {
    rps = (int)((tiles + splits - 1) / splits) * WG_ROWS;
    splits = (M + rps - 1) / rps;
  }
  float* part = splits > 1 ? reinterpret_cast<float*>(workspace) : nullptr;
  if (splits < 1) splits = 1;
  const dim3 grid((unsigned)strips, (unsigned)splits), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bf16_t* u = reinterpret_cast<const bf16_t*>(U);
  const bf16_t* x = reinterpret_cast<const bf16_t*>(X) + x_off;
  if (r == 16) hipLaunchKernelGGL(lora_wgrad_kernel<1>, grid, block, 0, st, u, ldu, x, ldx, G, ldg, part, M, C, rps, alpha, out_f32 != 0);
  else if (r == 32) hipLaunchKernelGGL(lora_wgrad_kernel<2>, grid, block, 0, st, u, ldu, x, ldx, G, ldg, part, M, C, rps, alpha, out_f32 != 0);
  else hipLaunchKernelGGL(lora_wgrad_kernel<4>, grid, block, 0, st, u, ldu, x, ldx, G, ldg, part, M, C, rps, alpha, out_f32 != 0);
  int status = launch_status();
  if (status != U2_OK || !part) return status;
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)(((int64_t)r * C + 255) / 256)), dim3(256), 0, st, part, G, ldg, r, C,
                     (int)splits, alpha, out_f32 != 0);
  return launch_status();
}

}  // extern "C"
