// The adapter (LoRA) branch of one packed product for a FEW rows (M <= 64: a decode step), as a group, in two launches
// (include/u2tok.h: u2tok_lora_rows).  Up to three segments {A_i (r_i, K), B_i (N_i, r_i), col0_i, scale_i} share the input X (M, K):
//   u_i = rnd16(X A_i^T)                                                        -> U[:, sum_{j<i} r_j ...]
//   Y[:, col0_i : col0_i + N_i] = rnd16(float(Y) + scale_i u_i B_i^T)           (one fused multiply-add per element)
// the rounding points of lora.hip's down / up pair, which at a decode step would be two launches per wrapped projection with ONE
// workgroup walking all of A per 16 rows (down_proj: r x 12288).  Here
//   launch 1  (K slice, segment, block of 16 rows) workgroups of one wave: the slice's accumulator chains (lora_down_kernel's
//             fragments: U^T = A X^T, 8 / (r / 16) steps of loads in flight) end as an fp32 16 x r partial tile in the workspace.
//             The slice count is a function of K alone.
//   launch 2  (segment, 256 columns, block of 16 rows) workgroups of four waves: the slices' tiles are added in slice order, rounded to
//             u (the workgroup of a segment's first columns also stores it to U) and handed through LDS to the waves, each of which
//             runs lora_up_kernel's unit (16 rows x 64 columns, a lane owns 16 consecutive columns = 32 contiguous bytes) onto Y.
// No atomics, every sum in a fixed order: two calls give the same bits, and a block of 16 rows has the bits it has in a call on those
// rows alone (nothing a workgroup computes depends on M beyond which rows it stores; rows past M repeat the last one).
#include "../../include/u2tok.h"
#include "kernels.h"

namespace u2 {
namespace {

__device__ __forceinline__ bf16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

struct RowsSeg {
  const bf16_t *A, *B;
  int r, col0, N, ucol;   // ucol: the segment's first column of U
  int tile0, blk0;        // first 16 x 16 fp32 tile of a slice row in the workspace / first workgroup of launch 2
  float scale;
};
struct LoraRowsArgs {
  RowsSeg s[3];
  int n;
};

constexpr int ROWS_MIN_STEPS = 8, ROWS_MAX_SLICES = 64;
// 32-wide steps per K slice: at least 8 (one batch of loads in flight), at most 64 slices
inline int rows_per_slice(int nsteps) { return std::max(ROWS_MIN_STEPS, (nsteps + ROWS_MAX_SLICES - 1) / ROWS_MAX_SLICES); }

template <int R16>
__device__ __forceinline__ void rows_down_slice(const bf16_t* __restrict__ xp, const bf16_t* __restrict__ ap, int64_t lda, int s0, int s1,
                                                f32x4* __restrict__ out, int lane) {
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
  for (int t = 0; t < R16; ++t) out[t * 64 + lane] = acc[t];
}

__global__ __launch_bounds__(64) void lora_rows_down_kernel(const bf16_t* __restrict__ X, int64_t ldx, LoraRowsArgs a, f32x4* __restrict__ ws,
                                                            int M, int nsteps, int per, int nslices, int rsum16) {
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  const int sl = blockIdx.x, m0 = blockIdx.z * 16;
  const RowsSeg s = a.s[blockIdx.y];
  const int R16 = s.r >> 4;
  const int64_t lda = (int64_t)nsteps * 32;
  const bf16_t* xp = X + (int64_t)min(m0 + i, M - 1) * ldx + 8 * g;   // (rows past M repeat the last one; never stored)
  const bf16_t* ap = s.A + (int64_t)i * lda + 8 * g;
  const int s0 = sl * per, s1 = min(s0 + per, nsteps);
  f32x4* out = ws + ((int64_t)blockIdx.z * nslices * rsum16 + s.tile0 + sl * R16) * 64;
  if (R16 == 1) rows_down_slice<1>(xp, ap, lda, s0, s1, out, lane);
  else if (R16 == 2) rows_down_slice<2>(xp, ap, lda, s0, s1, out, lane);
  else rows_down_slice<4>(xp, ap, lda, s0, s1, out, lane);
}

constexpr int ROWS_UP_WAVES = 4, ROWS_US = 64 + 8;   // u in LDS: 16 rows of 144 bytes (16-byte aligned fragments)

// lora_up_kernel's unit with the accumulate form: 16 rows x 64 columns of Y from nbase on
template <int KS>
__device__ __forceinline__ void rows_up_unit(const bf16_t* us, const bf16_t* __restrict__ W, bf16_t* Y, int64_t ldy, int m, int M, int nbase,
                                             int N, int r, float alpha, int i, int g) {
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 uf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int k0 = 32 * ks + 8 * g;
    uf[ks] = k0 < r ? ld8(us + i * ROWS_US + k0) : zero;
  }
  const bool live = m < M && nbase + 16 * g < N;   // (N % 16 == 0: a lane's 16 columns are inside or outside together)
  bf16_t* yp = Y + (int64_t)m * ldy + nbase + 16 * g;
  uint4 y0 = {0, 0, 0, 0}, y1 = {0, 0, 0, 0};
  if (live) {
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
      const bf16x8 wf = k0 < r ? ld8(W + (int64_t)n * r + k0) : zero;
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

__global__ __launch_bounds__(64 * ROWS_UP_WAVES) void lora_rows_up_kernel(LoraRowsArgs a, const f32x4* __restrict__ ws, bf16_t* __restrict__ U,
                                                                          int64_t ldu, bf16_t* Y, int64_t ldy, int M, int nslices,
                                                                          int rsum16) {
  __shared__ __attribute__((aligned(16))) bf16_t us[16 * ROWS_US];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  int si = 0;
  if (a.n > 1 && (int)blockIdx.x >= a.s[1].blk0) si = 1;
  if (a.n > 2 && (int)blockIdx.x >= a.s[2].blk0) si = 2;
  const RowsSeg s = a.s[si];
  const int lb = blockIdx.x - s.blk0, m0 = blockIdx.y * 16, R16 = s.r >> 4;
  // the slices' tiles in slice order; D[row = adapter row 16 t + 4 g + reg][col = row m0 + i of X]: 4 consecutive values of u's row
  if (tid < R16 * 64) {
    const f32x4* tp = ws + ((int64_t)blockIdx.y * nslices * rsum16 + s.tile0) * 64 + tid;
    const int stride = R16 * 64;
    f32x4 sum = tp[0];
    int v = 1;
    for (; v + 8 <= nslices; v += 8) {   // eight loads in flight, added in slice order
      f32x4 p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = tp[(v + j) * stride];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += p[j];
    }
    for (; v < nslices; ++v) sum += tp[v * stride];
    const uint2 o = {pack2_bf16(sum[0], sum[1]), pack2_bf16(sum[2], sum[3])};
    *reinterpret_cast<uint2*>(us + i * ROWS_US + 16 * w + 4 * g) = o;   // (tid = 64 t + lane: the wave index is the tile)
    if (lb == 0 && m0 + i < M) *reinterpret_cast<uint2*>(U + (int64_t)(m0 + i) * ldu + s.ucol + 16 * w + 4 * g) = o;
  }
  __syncthreads();
  const int nbase = (lb * ROWS_UP_WAVES + w) * 64;
  if (nbase >= s.N) return;
  bf16_t* y = Y + s.col0;
  if (s.r <= 32) rows_up_unit<1>(us, s.B, y, ldy, m0 + i, M, nbase, s.N, s.r, s.scale, i, g);
  else rows_up_unit<2>(us, s.B, y, ldy, m0 + i, M, nbase, s.N, s.r, s.scale, i, g);
}

inline bool rank_ok(int r) { return r == 16 || r == 32 || r == 64; }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// everything the group asks of its shapes (no pointer but the segments' own): -> sum of the ranks, or 0
int rows_shapes_ok(const LoraSeg* segs, int n, int M, int K) {
  if (!segs || n < 1 || n > 3 || M < 1 || M > 64 || K < 32 || K % 32) return 0;
  int rsum = 0;
  for (int i = 0; i < n; ++i) {
    const LoraSeg& s = segs[i];
    if (!s.A || !s.B || !al16(s.A) || !al16(s.B) || !rank_ok(s.r) || s.N < 16 || s.N % 16 || s.col0 < 0 || s.col0 % 16 ||
        (int64_t)s.col0 + s.N > 0x7fffffff || !(s.scale == s.scale))
      return 0;
    for (int j = 0; j < i; ++j)   // disjoint column ranges
      if (s.col0 < segs[j].col0 + segs[j].N && segs[j].col0 < s.col0 + s.N) return 0;
    rsum += s.r;
  }
  return rsum;
}

}  // namespace

size_t lora_rows_workspace_bytes(int M, int K, const LoraSeg* segs, int n) {
  const int rsum = rows_shapes_ok(segs, n, M, K);
  if (!rsum) return 0;
  const int nsteps = K / 32, per = rows_per_slice(nsteps), nslices = (nsteps + per - 1) / per;
  return (size_t)((M + 15) / 16) * nslices * rsum * 16 * sizeof(float);
}

int lora_rows(const bf16_t* X, int64_t ldx, const LoraSeg* segs, int n, bf16_t* U, int64_t ldu, bf16_t* Y, int64_t ldy, int M, int K,
              void* ws, size_t ws_bytes, bool check_only, hipStream_t st) {
  const int rsum = rows_shapes_ok(segs, n, M, K);
  if (!rsum || !X || !U || !Y || !ws || !al16(X) || !al16(U) || !al16(Y) || !al16(ws) || ldx % 8 || ldu % 8 || ldy % 8 || ldx < K || ldu < rsum)
    return U2_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (ldy < (int64_t)segs[i].col0 + segs[i].N) return U2_ERR_ARG;
  if (ws_bytes < lora_rows_workspace_bytes(M, K, segs, n)) return U2_ERR_WORKSPACE;
  if (check_only) return U2_OK;
  const int nsteps = K / 32, per = rows_per_slice(nsteps), nslices = (nsteps + per - 1) / per, mb = (M + 15) / 16;
  LoraRowsArgs a;
  a.n = n;
  int ucol = 0, blk = 0;
  for (int i = 0; i < 3; ++i) {
    const LoraSeg& s = segs[i < n ? i : 0];
    a.s[i] = RowsSeg{s.A, s.B, s.r, s.col0, s.N, ucol, nslices * (ucol / 16), blk, s.scale};
    if (i < n) {
      ucol += s.r;
      blk += (s.N + 64 * ROWS_UP_WAVES - 1) / (64 * ROWS_UP_WAVES);
    }
  }
  f32x4* w4 = reinterpret_cast<f32x4*>(ws);
  hipLaunchKernelGGL(lora_rows_down_kernel, dim3((unsigned)nslices, (unsigned)n, (unsigned)mb), dim3(64), 0, st, X, ldx, a, w4, M, nsteps, per,
                     nslices, rsum / 16);
  int e = launch_status();
  if (e != U2_OK) return e;
  hipLaunchKernelGGL(lora_rows_up_kernel, dim3((unsigned)blk, (unsigned)mb), dim3(64 * ROWS_UP_WAVES), 0, st, a, w4, U, ldu, Y, ldy, M, nslices,
                     rsum / 16);
  return launch_status();
}

}  // namespace u2

using namespace u2;

static_assert(sizeof(u2tok_lora_seg) == sizeof(LoraSeg), "u2tok_lora_seg and LoraSeg are one layout");

extern "C" {

size_t u2tok_lora_rows_workspace_bytes(int32_t M, int32_t K, const u2tok_lora_seg* segs, int32_t n) {
  return lora_rows_workspace_bytes(M, K, reinterpret_cast<const LoraSeg*>(segs), n);
}

int u2tok_lora_rows(const void* X, int64_t ldx, const u2tok_lora_seg* segs, int32_t n, void* U, int64_t ldu, void* Y, int64_t ldy, int32_t M,
                    int32_t K, void* workspace, size_t workspace_bytes, u2tok_stream_t stream) {
  return lora_rows(reinterpret_cast<const bf16_t*>(X), ldx, reinterpret_cast<const LoraSeg*>(segs), n, reinterpret_cast<bf16_t*>(U), ldu,
                   reinterpret_cast<bf16_t*>(Y), ldy, M, K, workspace, workspace_bytes, false, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
