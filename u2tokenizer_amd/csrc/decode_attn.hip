// Batched decode attention: ONE query row per sequence over that sequence's KV cache, for all B sequences and all heads of a
// decode step in one launch (+ one merge of the key splits), with a first visible key per sequence (a left-padded batch).
//
//   out[b][h] = softmax_j(q[b][h] . K[b][h / g][j] scale,  kv_start[b] <= j < T) V[b][h / g]      g = Hq / Hkv <= 16
//
// The per-sequence form this replaces for padded batches (decoder.hip: decode_post's loop) launches tokattn.hip's 64-query-row
// kernel once per sequence with ONE live query row per head, and every query head of a group stages the same K / V tiles again.
// Here the g query heads of a group are the ROWS of one 16-row MFMA operand (unused rows zero), so a K / V tile is staged once for
// the whole group:
//
//   workgroup = (sequence b, kv head, key split), 4 waves; wave w walks the split's 32-key tiles w, w + 4, ... on its own:
//     S^T (16 keys x 16 heads) = K Q^T : v_mfma_f32_16x16x32, A = K fragment (LDS), B = the group's queries (registers, loaded once)
//     O^T (16 d x 16 heads)   += V^T P^T: A = V^T fragment (two ds_read_b64_tr_b16 of the row-major V tile), B = the lane's own
//                                         exp'd scores -- the operand layouts and the LDS swizzles of tok_attn_kernel (tokattn.hip)
//   Each wave keeps its own running (max, sum, O^T) and its own two LDS stages of [K tile | V tile]: no barrier inside the key loop,
//   only the wave's own s_waitcnt on its LDS-DMA (`buffer_load_dwordx4 ... lds`: the MUBUF form stages about three times what the
//   FLAT form does beside MFMA-issuing waves, profiles/r06_stage_bw.log); the next tile is in flight under the current one.
//   The four waves' states meet once, through LDS, in wave order.
//
// Key splits cover FIXED ranges of tiles of [0, T): grid and workspace depend on (B, Hkv, T) only, never on kv_start.  Tiles wholly
// below kv_start[b] are skipped, the partial one is masked; a wave or a split without a visible key leaves (m, l) = (-inf, 0) and
// O = 0, which every merge treats as empty (merge weight of (-inf, -inf) is 1 on a zero term, as loss.hip's merge_scale).  Partials
// are fp32, merged in ascending split order, no atomics: the same call twice gives the same bits.  A sequence without any visible
// key gets zeros.
#include "kernels.h"

namespace u2 {

struct DecAttnArgs {
  const bf16_t *q, *k, *v;
  bf16_t* out;
  const int* kv_start;  // optional (B)
  int64_t ldq, ldo, kv_stride;
  int B, Hq, Hkv, G, T;
  int ns, tps;          // key splits, 32-key tiles per split
  float scale_log2e;
  float* opart;         // ns > 1: [ns][B][Hq][D] fp32, un-normalised
  float* ml;            // ns > 1: [ns][B][Hq][2] = (running max in log2 units, sum)
};

__device__ __forceinline__ float da_merge(float a, float b) { return a == b ? 1.f : __builtin_amdgcn_exp2f(a - b); }

template <int SEG>
__device__ __forceinline__ int da_v_rot(int k) {  // tokattn.hip: tv_rot
  if constexpr (SEG == 16) return 2 * (k & 3) + 8 * ((k >> 2) & 1);
  else return 2 * ((k >> 1) & 1) + 4 * ((k >> 2) & 1);
}
__device__ __forceinline__ int da_pos96(int row, int L) { return L ^ ((row >> 1) & 2); }  // tokattn.hip: t96_pos

typedef short da_v4s_t __attribute__((ext_vector_type(4)));

template <int D>
__global__ __launch_bounds__(256) void decode_attn_kernel(const DecAttnArgs a) {
  constexpr int BK = 32;              // keys per tile
  constexpr int CPR = D / 8;          // 16-byte chunks per tile row
  constexpr int ROWB = D * 2;         // bytes per tile row
  constexpr int TILE = BK * ROWB;     // bytes per K (or V) tile
  constexpr int SEG = CPR >= 16 ? 16 : 8;
  constexpr int NP = BK * CPR / 64;   // DMA pieces per lane per tile (one wave stages its own tile)
  constexpr int KS = D / 32;          // k steps of Q K^T
  constexpr int DB = D / 16;          // 16-wide d blocks of O^T
  static_assert(BK * CPR % 64 == 0, "tile");
  extern __shared__ __attribute__((aligned(16))) char lds[];  // per wave: [stage][K tile | V tile] x 2; then the waves' merge

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  char* const wl = lds + w * 4 * TILE;

  const int sp = blockIdx.x % a.ns;
  const int bh = blockIdx.x / a.ns;
  const int hkv = bh % a.Hkv, b = bh / a.Hkv;
  const int T = a.T, G = a.G;
  const int ntile = (T + BK - 1) / BK;
  const int kvs = a.kv_start ? max(0, min(a.kv_start[b], T)) : 0;
  const int t_lo = max(sp * a.tps, kvs / BK), t_hi = min(ntile, sp * a.tps + a.tps);

  const bf16_t* kb_ = a.k + ((int64_t)b * a.Hkv + hkv) * a.kv_stride;
  const bf16_t* vb_ = a.v + ((int64_t)b * a.Hkv + hkv) * a.kv_stride;

  // ---- LDS-DMA of one tile by one wave: piece i of a lane is LDS chunk c = i * 64 + lane = (row c / CPR, position c % CPR); the swizzle is
  // applied on the per-lane SOURCE address (the DMA destination is lane-linear); rows past the last key read a copy of it (masked below)
  auto dma = [&](const bf16_t* base, bool is_k, int kt, char* dst) {
    const int last = T - 1 - kt * BK;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int c = i * 64 + lane, row = c / CPR, cp = c % CPR;
      const int src_chunk = D == 96 ? da_pos96(row, cp)
                            : is_k  ? cp ^ (row & (SEG - 1))
                                    : (cp & ~(SEG - 1)) | (((cp & (SEG - 1)) - da_v_rot<SEG>(row)) & (SEG - 1));
      lds_dma_mubuf16(base, dst + i * 1024, min(row, last) * ROWB + src_chunk * 16, kt * TILE);
    }
  };

  int kt = t_lo + w;
  if (kt < t_hi) {
    dma(kb_, true, kt, wl);
    dma(vb_, false, kt, wl + TILE);
  }
  // ---- the group's queries (B operand): row l15 = query head hkv * G + l15 (rows >= G: zero), Q[row][32 ks + 8 g .. + 7]
  bf16x8 qf[KS];
  {
    const bf16_t* qp = a.q + (int64_t)b * a.ldq + (int64_t)(hkv * G + min(l15, G - 1)) * D + g * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
      if (l15 >= G) qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  // ---- per-lane fragment offsets (tok_attn_kernel's)
  const int k_row_off = l15 * ROWB;
  const int k_swz = D == 96 ? (l15 >> 1) & 2 : l15 & (SEG - 1);
  const int v_row = 4 * g + (l15 >> 2);
  const int v_rot = da_v_rot<SEG>(v_row);
  const int v_base_off = v_row * ROWB + (l15 & 1) * 8;
  const int v_cc = (l15 & 3) >> 1;

  f32x4 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float c_scale = a.scale_log2e;

  for (int it = 0; kt < t_hi; kt += 4, ++it) {
    const int stage = it & 1;
    const char* const tK = wl + stage * 2 * TILE;
    const char* const tV = tK + TILE;
    if (kt + 4 < t_hi) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of the other stage (the previous tile) have returned
      dma(kb_, true, kt + 4, wl + (stage ^ 1) * 2 * TILE);
      dma(vb_, false, kt + 4, wl + (stage ^ 1) * 2 * TILE + TILE);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");  // tile kt has landed; tile kt + 4 stays in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // ---- S^T = K Q^T: two 16-key blocks, independent accumulator chains
    f32x4 sc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(tK + kb * 16 * ROWB + k_row_off + (((ks * 4 + g) ^ k_swz) << 4));
        if (ks & 1) acc1 = mfma16(kf, qf[ks], acc1);
        else acc0 = mfma16(kf, qf[ks], acc0);
      }
      sc[kb] = acc0 + acc1;
    }
    // ---- online softmax: the lane owns keys kt * 32 + 16 (i >> 2) + 4 g + (i & 3) of head l15
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = sc[i >> 2][i & 3];
    if (kt * BK < kvs || kt * BK + BK > T) {  // (wave-uniform) the partial first / last tile of the visible range
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = kt * BK + (i >> 2) * 16 + 4 * g + (i & 3);
        if (j < kvs || j >= T) x[i] = -INFINITY;
      }
    }
    float mt = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    mt *= c_scale;  // (scale > 0 commutes with the max)
    const float m_new = fmaxf(m_run, mt);
    const float alpha = da_merge(m_run, m_new);          // (-inf, -inf): 1 on a zero state, never -inf - (-inf)
    const float m_sub = m_new == -INFINITY ? 0.f : m_new;  // no visible key so far: every score is -inf, exp2(-inf - 0) = 0
    m_run = m_new;
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      x[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(x[i], c_scale, -m_sub));
      ps += x[i];
    }
    l_run = l_run * alpha + ps;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      o[db][0] *= alpha; o[db][1] *= alpha; o[db][2] *= alpha; o[db][3] *= alpha;
    }
    // P fragment: k-slot (g, e) carries key 16 (e >> 2) + 4 g + (e & 3) -- P never leaves its lane
    union { bf16x8 v; uint32_t u[4]; } pf;
    pf.u[0] = pack2_bf16(x[0], x[1]);
    pf.u[1] = pack2_bf16(x[2], x[3]);
    pf.u[2] = pack2_bf16(x[4], x[5]);
    pf.u[3] = pack2_bf16(x[6], x[7]);
    // ---- O^T += V^T P^T.  The transpose reads go out as asm, two d blocks at a time with their own wait: hipcc puts s_waitcnt vmcnt(0)
    // in front of a ds_read_b64_tr_b16 that follows an LDS-DMA, which would end the overlap with tile kt + 4
    {
      const uint32_t tv = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)const_cast<char*>(tV) + v_base_off;
#pragma unroll
      for (int db = 0; db < DB; db += 2) {
        uint32_t ad[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int cc = 2 * (db + u) + v_cc;
          const int cp = D == 96 ? da_pos96(v_row, cc) : (cc & ~(SEG - 1)) | (((cc & (SEG - 1)) + v_rot) & (SEG - 1));
          ad[u] = tv + cp * 16;
        }
        da_v4s_t lo0, hi0, lo1, hi1;
        asm volatile("ds_read_b64_tr_b16 %0, %4\n\tds_read_b64_tr_b16 %1, %4 offset:%6\n\t"
                     "ds_read_b64_tr_b16 %2, %5\n\tds_read_b64_tr_b16 %3, %5 offset:%6\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(lo0), "=&v"(hi0), "=&v"(lo1), "=&v"(hi1)
                     : "v"(ad[0]), "v"(ad[1]), "n"(16 * ROWB)
                     : "memory");
        o[db] = mfma16(bf16x8{lo0[0], lo0[1], lo0[2], lo0[3], hi0[0], hi0[1], hi0[2], hi0[3]}, pf.v, o[db]);
        o[db + 1] = mfma16(bf16x8{lo1[0], lo1[1], lo1[2], lo1[3], hi1[0], hi1[1], hi1[2], hi1[3]}, pf.v, o[db + 1]);
      }
    }
  }

  // ---- the four waves' states meet in LDS (wave order): lane holds O^T[d = 16 db + 4 g + r][head l15]
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  __syncthreads();  // every wave is done with its tiles: the staging area is free
  float* const so = reinterpret_cast<float*>(lds);  // [4][16][D]
  float* const sml = so + 4 * 16 * D;               // [4][16][2]
  if (l15 < G) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
      *reinterpret_cast<float4*>(so + (w * 16 + l15) * D + 16 * db + 4 * g) = float4{o[db][0], o[db][1], o[db][2], o[db][3]};
    if (g == 0) {
      sml[(w * 16 + l15) * 2] = m_run;
      sml[(w * 16 + l15) * 2 + 1] = l_tot;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < G * (D / 4); idx += 256) {
    const int qh = idx / (D / 4), c4 = (idx - qh * (D / 4)) * 4;
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) m = fmaxf(m, sml[(u * 16 + qh) * 2]);
    float L = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float wgt = da_merge(sml[(u * 16 + qh) * 2], m);
      L += wgt * sml[(u * 16 + qh) * 2 + 1];
      const float4 t = *reinterpret_cast<const float4*>(so + (u * 16 + qh) * D + c4);
      acc[0] += wgt * t.x; acc[1] += wgt * t.y; acc[2] += wgt * t.z; acc[3] += wgt * t.w;
    }
    const int head = hkv * G + qh;
    if (a.ns == 1) {
      const float inv = L > 0.f ? 1.f / L : 0.f;  // no visible key: zeros
      *reinterpret_cast<uint2*>(a.out + (int64_t)b * a.ldo + head * D + c4) =
          uint2{pack2_bf16(acc[0] * inv, acc[1] * inv), pack2_bf16(acc[2] * inv, acc[3] * inv)};
    } else {
      const int64_t e = ((int64_t)sp * a.B + b) * a.Hq + head;
      *reinterpret_cast<float4*>(a.opart + e * D + c4) = float4{acc[0], acc[1], acc[2], acc[3]};
      if (c4 == 0) {
        a.ml[e * 2] = m;
        a.ml[e * 2 + 1] = L;
      }
    }
  }
}

// out[b][head] = sum_s 2^(m_s - m) O_s / sum_s 2^(m_s - m) l_s over the key splits, s in ascending order; an empty split is (-inf, 0)
__global__ __launch_bounds__(256) void decode_attn_merge_kernel(const DecAttnArgs a, int D) {
  const int d4 = D >> 2;
  const int64_t total = (int64_t)a.B * a.Hq * d4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % d4) * 4;
  const int64_t bhq = idx / d4;  // b * Hq + head
  const int64_t step = (int64_t)a.B * a.Hq;
  float m = -INFINITY;
  for (int s = 0; s < a.ns; ++s) m = fmaxf(m, a.ml[(s * step + bhq) * 2]);
  float L = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < a.ns; ++s) {
    const float* mp = a.ml + (s * step + bhq) * 2;
    const float wgt = da_merge(mp[0], m);
    L += wgt * mp[1];
    const float4 t = *reinterpret_cast<const float4*>(a.opart + (s * step + bhq) * D + c4);
    acc[0] += wgt * t.x; acc[1] += wgt * t.y; acc[2] += wgt * t.z; acc[3] += wgt * t.w;
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  const int b = (int)(bhq / a.Hq), head = (int)(bhq % a.Hq);
  *reinterpret_cast<uint2*>(a.out + (int64_t)b * a.ldo + head * D + c4) =
      uint2{pack2_bf16(acc[0] * inv, acc[1] * inv), pack2_bf16(acc[2] * inv, acc[3] * inv)};
}

// Key splits of a call: enough workgroups for the 256 CUs, at least one tile per wave of a split.  A function of (B, Hkv, T) only.
static int dec_attn_splits(int B, int Hkv, int T) {
  const int64_t base = (int64_t)B * Hkv;
  const int ntile = (int)cdiv(T, 32);
  if (ntile < 8) return 1;
  return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(256, base), ntile / 4));
}

size_t decode_attention_workspace_bytes(int B, int Hq, int Hkv, int T, int D) {
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || T <= 0 || D <= 0) return 0;
  const int ns = dec_attn_splits(B, Hkv, T);
  return ns > 1 ? (size_t)ns * B * Hq * ((size_t)D * 4 + 8) : 0;
}

int decode_attention(const bf16_t* q, const bf16_t* K, const bf16_t* V, bf16_t* out, int B, int Hq, int Hkv, int T, int D,
                     int64_t ldq, int64_t kv_stride, int64_t ldo, float scale, const int* kv_start, void* ws, size_t ws_bytes,
                     hipStream_t stream) {
  if (!q || !K || !V || !out || B <= 0 || B > 65535 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || Hq / Hkv > 16) return U2_ERR_ARG;
  if (D != 64 && D != 96 && D != 128) return U2_ERR_ARG;
  if (kv_stride == 0) kv_stride = (int64_t)T * D;
  if (kv_stride < (int64_t)T * D || (kv_stride & 7) || (int64_t)T * D * 2 >= (1ll << 31)) return U2_ERR_ARG;  // (32-bit DMA offsets)
  if (ldq < (int64_t)Hq * D || ldo < (int64_t)Hq * D || (ldq & 7) || (ldo & 3) || !(scale > 0.f)) return U2_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)K | (uintptr_t)V) & 15) || ((uintptr_t)out & 7) || ((uintptr_t)kv_start & 3)) return U2_ERR_ARG;
  DecAttnArgs a;
  a.q = q; a.k = K; a.v = V; a.out = out; a.kv_start = kv_start;
  a.ldq = ldq; a.ldo = ldo; a.kv_stride = kv_stride;
  a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.T = T;
  a.scale_log2e = scale * 1.44269504088896340736f;
  const int ntile = (int)cdiv(T, 32);
  int ns = ws ? dec_attn_splits(B, Hkv, T) : 1;  // (no workspace: unsplit)
  a.tps = (int)cdiv(ntile, ns);
  a.ns = (int)cdiv(ntile, a.tps);  // no split beyond the last tile
  a.opart = nullptr; a.ml = nullptr;
  if (a.ns > 1) {
    if (ws_bytes < (size_t)a.ns * B * Hq * ((size_t)D * 4 + 8)) return U2_ERR_WORKSPACE;
    if ((uintptr_t)ws & 15) return U2_ERR_ARG;
    a.opart = reinterpret_cast<float*>(ws);
    a.ml = a.opart + (size_t)a.ns * B * Hq * D;
  }
  const int64_t grid = (int64_t)B * Hkv * a.ns;
  if (grid > 0x7fffffff) return U2_ERR_ARG;
  ProfScope ps(PROF_TOKATTN, 4.0 * B * Hq * (double)T * D, stream, 2.0 * B * D * (2.0 * Hq + 2.0 * T * Hkv));
#define U2_DA(D_)                                                                                                      \
  do {                                                                                                                 \
    constexpr size_t smem_ = 4 * 4 * 32 * (D_) * 2;  /* 4 waves x 2 stages x (K | V) tile; >= the merge's 4 x 16 x D floats + 512 */ \
    static_assert(smem_ >= 4 * 16 * (D_) * 4 + 512, "merge area");                                                     \
    hipLaunchKernelGGL((decode_attn_kernel<D_>), dim3((unsigned)grid), dim3(256), smem_, stream, a);                   \
  } while (0)
  if (D == 128) U2_DA(128);
  else if (D == 96) U2_DA(96);
  else U2_DA(64);
#undef U2_DA
  if (a.ns > 1) {
    const int64_t total = (int64_t)B * Hq * (D / 4);
    hipLaunchKernelGGL(decode_attn_merge_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, a, D);
  }
  return launch_status();
}

}  // namespace u2
