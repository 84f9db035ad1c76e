// Row kernels of the loss head (u2tokenizer_amd/loss_head.py): cross-entropy over lm_head's logits taken one vocabulary slice at a time,
// so that no rows x vocab tensor ever exists.  Z = rows x Vs block of logits (16-bit elements, leading dimension ldz) holding the
// vocabulary columns [v0, v0 + Vs).  Reference: transformers' ForCausalLMLoss = F.cross_entropy(logits.float(), labels), whose
// backward hands lm_head the element-type rounding of the fp32 gradient  g (softmax(z) - onehot(label)).
// HBM-bound: one read of Z (ce_lse_update), one read + one write (ce_grad_inplace); 16-byte accesses, fp32 arithmetic, no atomics.
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
__global__ __launch_bounds__(256) void ce_lse_update_kernel(const bf16_t* __restrict__ Z, int64_t ldz, int Vs, int64_t v0,
                                                            const int64_t* __restrict__ labels, float* __restrict__ m_io,
                                                            float* __restrict__ l_io, float* __restrict__ zt) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const bf16_t* zp = Z + row * ldz;
  const int nchunk = Vs >> 3;
  float m = -INFINITY, s = 0.f;
#pragma unroll 4
  for (int c = tid; c < nchunk; c += 256) {
    float v[8];
    unpack8(*reinterpret_cast<const uint4*>(zp + (int64_t)c * 8), v);
    const float cm = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
    if (cm > m) {   // new running max: rescale what has been summed (rare after the first chunks)
      s *= __expf(m - cm);
      m = cm;
    }
    if (m > -INFINITY)   // (a chunk of -inf only, before any finite value: nothing to add, and -inf - -inf must not be formed)
      s += ((__expf(v[0] - m) + __expf(v[1] - m)) + (__expf(v[2] - m) + __expf(v[3] - m))) +
           ((__expf(v[4] - m) + __expf(v[5] - m)) + (__expf(v[6] - m) + __expf(v[7] - m)));
  }
  const float wm = wave_max(m);
  s = wave_sum(s * merge_scale(m, wm));
  if (lane == 0) { red[0][wave] = wm; red[1][wave] = s; }
  __syncthreads();
  if (tid == 0) {
    const float bm = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    const float bl = (red[1][0] * merge_scale(red[0][0], bm) + red[1][1] * merge_scale(red[0][1], bm)) +
                     (red[1][2] * merge_scale(red[0][2], bm) + red[1][3] * merge_scale(red[0][3], bm));
    const float m0 = m_io[row], l0 = l_io[row];   // first slice: (-inf, 0)
    const float mn = fmaxf(m0, bm);
    m_io[row] = mn;
    l_io[row] = l0 * merge_scale(m0, mn) + bl * merge_scale(bm, mn);
    const int64_t li = labels[row] - v0;
    if (li >= 0 && li < Vs) zt[row] = bf16_to_f32(zp[li]);
  }
}

int ce_lse_update(const bf16_t* Z, int64_t ldz, int rows, int Vs, int64_t v0, const int64_t* labels, float* m, float* l, float* zt,
                  hipStream_t st) {
  if (!Z || !labels || !m || !l || !zt || rows < 1 || Vs < 1 || v0 < 0 || ldz < Vs || (ldz & 7) || (Vs & 7)) return U2_ERR_ARG;
  if (((uintptr_t)Z & 15) || (((uintptr_t)m | (uintptr_t)l | (uintptr_t)zt) & 3) || ((uintptr_t)labels & 7)) return U2_ERR_ARG;
  ProfScope ps(PROF_ROWOP, 0, st, (double)rows * Vs * 2.0);
  hipLaunchKernelGGL(ce_lse_update_kernel, dim3((unsigned)rows), dim3(256), 0, st, Z, ldz, Vs, v0, labels, m, l, zt);
  return launch_status();
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
