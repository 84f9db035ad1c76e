// Row kernels of the loss head (u2tokenizer_amd/loss_head.py): cross-entropy over lm_head's logits taken one vocabulary slice at a time,
// so that no rows x vocab tensor ever exists.  Z = rows x Vs block of logits (16-bit elements, leading dimension ldz) holding the
// vocabulary columns [v0, v0 + Vs).  Reference: transformers' ForCausalLMLoss = F.cross_entropy(logits.float(), labels), whose
// backward hands lm_head the element-type rounding of the fp32 gradient  g (softmax(z) - onehot(label)).
// HBM-bound: one read of Z (ce_lse_update / ce_stats_update), one read + one write (ce_grad_inplace); 16-byte accesses, fp32 arithmetic, no atomics.
#include "kernels.h"

namespace u2 {

__device__ __forceinline__ void unpack8(const uint4 u, float v[8]) {
  v[0] = bf16lo(u.x); v[1] = bf16hi(u.x); v[2] = bf16lo(u.y); v[3] = bf16hi(u.y);
  v[4] = bf16lo(u.z); v[5] = bf16hi(u.z); v[6] = bf16lo(u.w); v[7] = bf16hi(u.w);
}

// exp(a - b) for the merges of (max, sum) pairs: 1 when the two are the same value (also -inf and -inf: an empty partial), 0 when a = -inf
__device__ __forceinline__ float merge_scale(float a, float b) { return a == b ? 1.f : __expf(a - b); }

// One workgroup per row.  A thread keeps an online (max, sum exp) pair over its chunks of 8 (chunk c of thread t: column 8 (t + 256 c)),
// the pairs meet by wave shuffles, then across the four waves through LDS; thread 0 folds the block's pair into the row's running (m, l)
// and picks up the label's logit when this slice holds it.  Every sum has a fixed order: the same inputs give the same bits.
//
// Compile-time flavours add further per-row statistics to the same pass (u2tok_ce_stats_update); <false, false, false> is
// u2tok_ce_lse_update, and (m, l, zt) come off the one reduction tree in every flavour, so they carry the same bits in all of them.
//   ARG  (amax, aidx): the maximum and the FIRST column that holds it.  The order is lexicographic -- larger value, then smaller
//        index -- at every level: a thread walks its chunks in ascending columns and takes a new index only on a strictly larger
//        chunk maximum (inside a chunk: the lowest j that equals it); across lanes and across waves the value tree is the one of m,
//        and the index is the MINIMUM over the partners whose maximum equals the merged one (the others, and threads without a
//        chunk, offer NOIDX); against the running pair: larger value, or the same value at a smaller global column v0 + j (int64).
//        A row of -inf only therefore ends at its first column, and the order in which slices are fed does not matter.
//   SUM  (zsum): the sum of the logits.  Longest chain of dependent fp32 additions per slice: 3 (the tree over a chunk's 8 values)
//        + ceil(Vs / 2048) (a thread's chunks, in order) + 6 (wave shuffles) + 2 (four waves) = ceil(Vs / 2048) + 11; the addition
//        into the running sum is one more per slice.
//   L2   (l2): sum exp(2 (z - m)) against the SAME running maximum as l: the squares of the very exponentials that go into l, and
//        wherever l is rescaled by a factor (merge_scale's conventions included) l2 is rescaled by its square.
constexpr int NOIDX = 0x7fffffff;

template <bool ARG, bool SUM, bool L2>
__global__ __launch_bounds__(256) void ce_update_kernel(const bf16_t* __restrict__ Z, int64_t ldz, int Vs, int64_t v0,
                                                        const int64_t* __restrict__ labels, float* __restrict__ m_io,
                                                        float* __restrict__ l_io, float* __restrict__ zt, float* __restrict__ amax,
                                                        int64_t* __restrict__ aidx, float* __restrict__ zsum_io,
                                                        float* __restrict__ l2_io) {
  __shared__ float red[4][4];   // max, sum exp, sum exp^2, sum z
  __shared__ int redi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const bf16_t* zp = Z + row * ldz;
  const int nchunk = Vs >> 3;
  float m = -INFINITY, s = 0.f, s2 = 0.f, zs = 0.f;
  int ai = NOIDX;
#pragma unroll 4
  for (int c = tid; c < nchunk; c += 256) {
    float v[8];
    unpack8(*reinterpret_cast<const uint4*>(zp + (int64_t)c * 8), v);
    const float cm = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
    if constexpr (SUM) zs += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    if constexpr (ARG) {
      if (cm > m || ai == NOIDX) {   // strictly larger, or the thread's first chunk (which may be -inf throughout)
        int j = 7;
#pragma unroll
        for (int k = 6; k >= 0; --k) j = v[k] == cm ? k : j;
        ai = c * 8 + j;
      }
    }
    if (cm > m) {   // new running max: rescale what has been summed (rare after the first chunks)
      const float sc = __expf(m - cm);
      s *= sc;
      if constexpr (L2) s2 *= sc * sc;
      m = cm;
    }
    if (m > -INFINITY) {   // (a chunk of -inf only, before any finite value: nothing to add, and -inf - -inf must not be formed)
      float e[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = __expf(v[k] - m);
      s += ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
      if constexpr (L2)
        s2 += ((e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3])) + ((e[4] * e[4] + e[5] * e[5]) + (e[6] * e[6] + e[7] * e[7]));
    }
  }
  const float wm = wave_max(m);
  const float wsc = merge_scale(m, wm);
  s = wave_sum(s * wsc);
  if constexpr (L2) s2 = wave_sum(s2 * (wsc * wsc));
  if constexpr (SUM) zs = wave_sum(zs);
  if constexpr (ARG) {
    ai = m == wm ? ai : NOIDX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ai = min(ai, __shfl_xor(ai, o, 64));
  }
  if (lane == 0) {
    red[0][wave] = wm;
    red[1][wave] = s;
    if constexpr (L2) red[2][wave] = s2;
    if constexpr (SUM) red[3][wave] = zs;
    if constexpr (ARG) redi[wave] = ai;
  }
  __syncthreads();
  if (tid == 0) {
    const float bm = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    const float c0 = merge_scale(red[0][0], bm), c1 = merge_scale(red[0][1], bm), c2 = merge_scale(red[0][2], bm),
                c3 = merge_scale(red[0][3], bm);
    const float bl = (red[1][0] * c0 + red[1][1] * c1) + (red[1][2] * c2 + red[1][3] * c3);
    const float m0 = m_io[row], l0 = l_io[row];   // first slice: (-inf, 0)
    const float mn = fmaxf(m0, bm);
    const float r0 = merge_scale(m0, mn), r1 = merge_scale(bm, mn);
    m_io[row] = mn;
    l_io[row] = l0 * r0 + bl * r1;
    const int64_t li = labels[row] - v0;
    if (li >= 0 && li < Vs) zt[row] = bf16_to_f32(zp[li]);
    if constexpr (L2) {
      const float bl2 = (red[2][0] * (c0 * c0) + red[2][1] * (c1 * c1)) + (red[2][2] * (c2 * c2) + red[2][3] * (c3 * c3));
      l2_io[row] = l2_io[row] * (r0 * r0) + bl2 * (r1 * r1);
    }
    if constexpr (SUM) zsum_io[row] += (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]);
    if constexpr (ARG) {
      int bi = NOIDX;
#pragma unroll
      for (int w = 0; w < 4; ++w) bi = red[0][w] == bm ? min(bi, redi[w]) : bi;
      const int64_t gi = v0 + bi;   // (bi < Vs: the wave that holds the block's maximum holds a column of it)
      const float a0 = amax[row];
      if (bm > a0 || (bm == a0 && gi < aidx[row])) {
        amax[row] = bm;
        aidx[row] = gi;
      }
    }
  }
}

static bool ce_block_ok(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l,
                        float* zt) {
  if (!Z || !labels || !m || !l || !zt || rows < 1 || Vs < 1 || v0 < 0 || ldz < Vs || (ldz & 7) || (Vs & 7)) return false;
  return !(((uintptr_t)Z & 15) || (((uintptr_t)m | (uintptr_t)l | (uintptr_t)zt) & 3) || ((uintptr_t)labels & 7));
}

template <bool ARG, bool SUM, bool L2>
static int ce_update_launch(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l,
                            float* zt, float* amax, int64_t* aidx, float* zsum, float* l2, hipStream_t st) {
  ProfScope ps(PROF_ROWOP, 0, st, (double)rows * Vs * 2.0);
  hipLaunchKernelGGL((ce_update_kernel<ARG, SUM, L2>), dim3((unsigned)rows), dim3(256), 0, st, Z, ldz, Vs, v0, labels, m, l, zt, amax,
                     aidx, zsum, l2);
  return launch_status();
}

int ce_lse_update(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l, float* zt,
                  hipStream_t st) {
  if (!ce_block_ok(Z, ldz, rows, Vs, v0, labels, m, l, zt)) return U2_ERR_ARG;
  return ce_update_launch<false, false, false>(Z, ldz, rows, Vs, v0, labels, m, l, zt, nullptr, nullptr, nullptr, nullptr, st);
}

int ce_stats_update(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l, float* zt,
                    float* amax, int64_t* aidx, float* zsum, float* l2, hipStream_t st) {
  if (!ce_block_ok(Z, ldz, rows, Vs, v0, labels, m, l, zt) || (!amax != !aidx)) return U2_ERR_ARG;
  if ((((uintptr_t)amax | (uintptr_t)zsum | (uintptr_t)l2) & 3) || ((uintptr_t)aidx & 7)) return U2_ERR_ARG;
  if (v0 > INT64_MAX - Vs) return U2_ERR_ARG;
  static constexpr decltype(&ce_update_launch<false, false, false>) flavour[8] = {
      ce_update_launch<false, false, false>, ce_update_launch<true, false, false>, ce_update_launch<false, true, false>,
      ce_update_launch<true, true, false>,   ce_update_launch<false, false, true>, ce_update_launch<true, false, true>,
      ce_update_launch<false, true, true>,   ce_update_launch<true, true, true>};
  return flavour[(amax ? 1 : 0) | (zsum ? 2 : 0) | (l2 ? 4 : 0)](Z, ldz, rows, Vs, v0, labels, m, l, zt, amax, aidx, zsum, l2, st);
}

// Z[r][j] <- elem( coef[r] (exp(Z[r][j] - lse[r]) - [v0 + j == label[r]]) ), lse the NATURAL-log sum of exponentials of the whole row.
// Workgroup (x, y): row x, chunks [1024 y, 1024 y + 1024) of 8 columns, four per thread.
__global__ __launch_bounds__(256) void ce_grad_inplace_kernel(bf16_t* __restrict__ Z, int64_t ldz, int Vs, int64_t v0,
                                                              const int64_t* __restrict__ labels, const float* __restrict__ lse,
                                                              const float* __restrict__ coef) {
  const int64_t row = blockIdx.x;
  bf16_t* zp = Z + row * ldz;
  const int nchunk = Vs >> 3;
  const float ls = lse[row], g = coef[row];
  const int64_t li = labels[row] - v0;   // the label's column in this slice, or outside [0, Vs)
  const int c0 = blockIdx.y * 1024 + threadIdx.x;
  uint4 u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c0 + i * 256 < nchunk) u[i] = *reinterpret_cast<const uint4*>(zp + (int64_t)(c0 + i * 256) * 8);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + i * 256;
    if (c < nchunk) {
      float v[8];
      unpack8(u[i], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = g * (__expf(v[j] - ls) - ((int64_t)c * 8 + j == li ? 1.f : 0.f));
      *reinterpret_cast<uint4*>(zp + (int64_t)c * 8) =
          uint4{pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3]), pack2_bf16(v[4], v[5]), pack2_bf16(v[6], v[7])};
    }
  }
}

int ce_grad_inplace(bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, const float* lse, const float* coef,
                    hipStream_t st) {
  if (!Z || !labels || !lse || !coef || rows < 1 || Vs < 1 || v0 < 0 || ldz < Vs || (ldz & 7) || (Vs & 7)) return U2_ERR_ARG;
  if (((uintptr_t)Z & 15) || (((uintptr_t)lse | (uintptr_t)coef) & 3) || ((uintptr_t)labels & 7)) return U2_ERR_ARG;
  const int64_t ny = cdiv(Vs >> 3, 1024);
  if (ny > 65535) return U2_ERR_ARG;
  ProfScope ps(PROF_ROWOP, 0, st, (double)rows * Vs * 4.0);
  hipLaunchKernelGGL(ce_grad_inplace_kernel, dim3((unsigned)rows, (unsigned)ny), dim3(256), 0, st, Z, ldz, Vs, v0, labels, lse, coef);
  return launch_status();
}

}  // namespace u2
