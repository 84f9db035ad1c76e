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
#include "rows.h"

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
                     bool check_only, hipStream_t stream) {
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
  if (check_only) return U2_OK;
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

// ================================================================================================== the FP8 (e4m3) KV cache
// K and V as OCP e4m3 codes with ONE fp32 scale per cache row -- the D values of one (sequence, kv head, position), K and V each:
//   scale = amax / 448 (an all-zero row: 1), code = e4m3(clamp(x / scale, +-448)) round to nearest even; value = code x scale exactly.
// Codes (B, Hkv, capacity, D) bytes, scales (B, Hkv, capacity) fp32.  Two kernels: the quantising append and the decode attention
// over codes; the 16-bit kernel above is the model of the second.

struct KvQuantArgs {
  const bf16_t *k, *v;
  int64_t k_bs, k_hs, k_rs, v_bs, v_hs, v_rs;  // elements between sequences / kv heads / positions of the source rows
  uint8_t *kc, *vc;
  float *ksc, *vsc;
  int64_t rows;  // B * Hkv * n
  int Hkv, n, D, cap, s_off, nblk;
};

// 16 lanes per row (lane c < D / 8 holds the row's elements 8 c .. 8 c + 7), four rows per wave, 16 per workgroup; workgroups
// [0, nblk) take K, [nblk, 2 nblk) V.  The row maximum is exact in any order; the two divisions are IEEE fp32 (hipcc's default for
// `/`), so codes and scales have the bits of ops.quantize_kv_fp8.  Stores: 8 codes per lane, the scale by the row's first lane.
__global__ __launch_bounds__(256) void kv_quantize_rows_kernel(const KvQuantArgs a) {
  const int sub = threadIdx.x & 15;
  const bool is_v = (int)blockIdx.x >= a.nblk;
  const int64_t row = (int64_t)((int)blockIdx.x - (is_v ? a.nblk : 0)) * 16 + (threadIdx.x >> 4);
  const bool live = row < a.rows && sub < (a.D >> 3);
  const int64_t r = row < a.rows ? row : a.rows - 1;
  const int i = (int)(r % a.n);
  const int64_t bh = r / a.n;
  const int h = (int)(bh % a.Hkv);
  const int64_t b = bh / a.Hkv;
  const bf16_t* src = is_v ? a.v + b * a.v_bs + h * a.v_hs + i * a.v_rs : a.k + b * a.k_bs + h * a.k_hs + i * a.k_rs;
  uint4 u = uint4{0, 0, 0, 0};
  if (live) u = *reinterpret_cast<const uint4*>(src + sub * 8);
  const float x[8] = {bf16lo(u.x), bf16hi(u.x), bf16lo(u.y), bf16hi(u.y), bf16lo(u.z), bf16hi(u.z), bf16lo(u.w), bf16hi(u.w)};
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(x[j]));
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
  const float scale = am > 0.f ? am / 448.f : 1.f;
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = fminf(fmaxf(x[j] / scale, -448.f), 448.f);
#if defined(__HIP_DEVICE_COMPILE__)
  int c0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false), c1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  c0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], c0, true);
  c1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], c1, true);
#else
  int c0 = 0, c1 = 0;
#endif
  if (live) {
    const int64_t pos = bh * a.cap + a.s_off + i;
    *reinterpret_cast<uint2*>((is_v ? a.vc : a.kc) + pos * a.D + sub * 8) = uint2{(uint32_t)c0, (uint32_t)c1};
    if (sub == 0) (is_v ? a.vsc : a.ksc)[pos] = scale;
  }
}

int kv_quantize_rows(const bf16_t* k, const bf16_t* v, int B, int Hkv, int n, int D, int64_t k_bs, int64_t k_hs, int64_t k_rs, int64_t v_bs,
                     int64_t v_hs, int64_t v_rs, uint8_t* kc, uint8_t* vc, float* ksc, float* vsc, int capacity, int s_off, bool check_only,
                     hipStream_t stream) {
  if (!k || !v || !kc || !vc || !ksc || !vsc || B <= 0 || Hkv <= 0 || n <= 0 || capacity <= 0 || s_off < 0) return U2_ERR_ARG;
  if (D != 64 && D != 96 && D != 128) return U2_ERR_ARG;
  if ((int64_t)s_off + n > capacity || (int64_t)capacity * D >= (1ll << 31)) return U2_ERR_ARG;
  if ((((uintptr_t)k | (uintptr_t)v | (uintptr_t)kc | (uintptr_t)vc) & 15) || (((uintptr_t)ksc | (uintptr_t)vsc) & 3)) return U2_ERR_ARG;
  if (((k_bs | k_hs | k_rs | v_bs | v_hs | v_rs) & 7) || k_bs < 0 || k_hs < 0 || k_rs < 0 || v_bs < 0 || v_hs < 0 || v_rs < 0) return U2_ERR_ARG;
  KvQuantArgs a;
  a.k = k; a.v = v; a.k_bs = k_bs; a.k_hs = k_hs; a.k_rs = k_rs; a.v_bs = v_bs; a.v_hs = v_hs; a.v_rs = v_rs;
  a.kc = kc; a.vc = vc; a.ksc = ksc; a.vsc = vsc;
  a.rows = (int64_t)B * Hkv * n;
  a.Hkv = Hkv; a.n = n; a.D = D; a.cap = capacity; a.s_off = s_off;
  const int64_t nblk = cdiv(a.rows, 16);
  if (2 * nblk > 0x7fffffff) return U2_ERR_ARG;
  a.nblk = (int)nblk;
  if (check_only) return U2_OK;
  ProfScope ps(PROF_ROWOP, 0.0, stream, 2.0 * a.rows * (3.0 * D + 4.0));
  hipLaunchKernelGGL(kv_quantize_rows_kernel, dim3((unsigned)(2 * nblk)), dim3(256), 0, stream, a);
  return launch_status();
}

// ---- decode attention over codes.  decode_attn_kernel's structure -- workgroup = (sequence, kv head, key split), four waves with
// their own tiles, two LDS stages and running (max, sum, O^T), the fixed splits, the merges -- on tiles of 64 keys x D BYTES (the
// bytes a wave keeps in flight are those of the 16-bit kernel's 32-key tiles) plus the tile's 64 K scales and 64 V scales:
//   S^T = K Q^T        A = 8 codes of a key (one ds_read_b64) widened to the element type in registers (exact), B = the queries;
//                      s_j = ks[j] * sum_d q_d code(K_jd) in fp32, p_j = exp2(s_j c - m), l += p_j
//   O^T += V^T P^T     B = rnd_elem(p_j vs[j] PRE): the V scale rides on the probability; PRE = 2^8 in the IEEE-half build (vs is
//                      about amax / 448, so p vs alone falls into half's subnormals; 2^8 vs stays finite for every finite half
//                      value), 1 in the bf16 build; undone, exactly, where the sum is divided by l.
//                      A = V^T from `ds_read_b64_tr_b16` over BYTE PAIRS: lane l15 of a 16-lane group receives the pair
//                      (d = 32 blk + 2 l15, + 1) of its 8 keys; the low bytes widen to the fragment of the even d, the high bytes to
//                      that of the odd one -- two MFMAs per read pair, whose accumulator rows 4 g + r are d = 32 blk + 8 g + 2 r
//                      (+ 1): a lane ends up with 8 CONSECUTIVE d per 32-wide block.
// LDS image of a tile (K and V alike): row r at r * D, its 16-byte chunk ch at position ch ^ da8_swz(r) -- both the K row reads
// (a 32-lane half: 16 keys x one chunk) and the transposed V reads (a half: 8 keys x two chunks) are conflict-free for D = 64, 96,
// 128 (tests/test_kv8_host.py enumerates the banks).  Every LDS read of the key loop is inline asm with its own lgkmcnt wait: the
// compiler neither sees them nor puts a vmcnt(0) in front of them, so tile kt + 4 stays in flight under tile kt.
struct DecAttn8Args {
  const bf16_t* q;
  const uint8_t *k, *v;
  const float *ks, *vs;
  bf16_t* out;
  const int* kv_start;
  int64_t ldq, ldo, kv_stride, sc_stride;  // kv_stride: bytes, sc_stride: floats between (batch, kv head) entries
  int B, Hq, Hkv, G, T;
  int ns, tps;  // key splits, 64-key tiles per split
  float scale_log2e;
  float* opart;
  float* ml;
  int Sq, nrb, window;  // the rows form (decode_attn_kv8_kernel<D, true>): new positions per sequence, row blocks per kv head, W (0: none)
};

#if U2_ELEM_IS_F16
#define DA8_PRE 256.f
#define DA8_PRE_INV 0.00390625f
#else
#define DA8_PRE 1.f
#define DA8_PRE_INV 1.f
#endif

template <int D>
__host__ __device__ constexpr int da8_swz(int row) {
  return D == 128 ? (((row >> 1) & 3) << 1) | ((row >> 3) & 1) : D == 64 ? (((row >> 2) & 1) << 1) | ((row >> 3) & 1) : (row >> 3) & 1;
}

__device__ __forceinline__ void lds_dma_mubuf4(const void* base_rsrc_ptr, void* lds_dst, int voffset, int soffset) {  // (common.h: lds_dma_mubuf16)
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base_rsrc_ptr), 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_dst, 4, voffset, soffset, 0, 0);
#else
  (void)base_rsrc_ptr; (void)lds_dst; (void)voffset; (void)soffset;
#endif
}

typedef uint32_t da_u2_t __attribute__((ext_vector_type(2)));

// one 16-key block (K) / one 16-row offset (V) of reads per line; the immediates are 16 rows of D bytes
#define DA8_L2(op, n, off) op " %[" n "0], %[a0]" off "\n\t" op " %[" n "1], %[a1]" off "\n\t"
#define DA8_L3(op, n, off) DA8_L2(op, n, off) op " %[" n "2], %[a2]" off "\n\t"
#define DA8_L4(op, n, off) DA8_L3(op, n, off) op " %[" n "3], %[a3]" off "\n\t"
#define DA8_SCALES                                                                                                            \
  "ds_read_b128 %[s0], %[sa]\n\tds_read_b128 %[s1], %[sa] offset:64\n\tds_read_b128 %[s2], %[sa] offset:128\n\t"             \
  "ds_read_b128 %[s3], %[sa] offset:192\n\tds_read_b128 %[s4], %[sa] offset:256\n\tds_read_b128 %[s5], %[sa] offset:320\n\t" \
  "ds_read_b128 %[s6], %[sa] offset:384\n\tds_read_b128 %[s7], %[sa] offset:448\n\t"
#define DA8_OUT_SC                                                                                                                   \
  [s0] "=&v"(ksc[0]), [s1] "=&v"(ksc[1]), [s2] "=&v"(ksc[2]), [s3] "=&v"(ksc[3]), [s4] "=&v"(vsc[0]), [s5] "=&v"(vsc[1]), [s6] "=&v"(vsc[2]), \
      [s7] "=&v"(vsc[3])
#define DA8_OUT2(n, t) [n##00] "=&v"(t[0][0]), [n##01] "=&v"(t[0][1]), [n##10] "=&v"(t[1][0]), [n##11] "=&v"(t[1][1]), [n##20] "=&v"(t[2][0]), \
                       [n##21] "=&v"(t[2][1]), [n##30] "=&v"(t[3][0]), [n##31] "=&v"(t[3][1])
#define DA8_OUT3(n, t) DA8_OUT2(n, t), [n##02] "=&v"(t[0][2]), [n##12] "=&v"(t[1][2]), [n##22] "=&v"(t[2][2]), [n##32] "=&v"(t[3][2])
#define DA8_OUT4(n, t) DA8_OUT3(n, t), [n##03] "=&v"(t[0][3]), [n##13] "=&v"(t[1][3]), [n##23] "=&v"(t[2][3]), [n##33] "=&v"(t[3][3])

// ROWS (the continued prefill on such a cache, u2tok_attention_kv8_rows): Sq new positions per sequence instead of one.  The 16 rows
// of the B operand are 16 consecutive FLAT rows f = i G + gh of the kv head (i: the new position, gh: the query head inside the
// group; G need not divide 16: a block may straddle positions), workgroup = (sequence, kv head, row block, key split); rows
// f >= Sq G of the last block carry zero queries and are never stored.  With c = T - Sq the lane's row sees key j iff
// kv_start[b] <= j <= i + c and, for a window W > 0, j > i + c - W; a block walks the tiles between its first row's lower edge and
// its last row's diagonal, the masked path on every tile that an edge of one of its rows crosses (wave-uniform).  Partials and
// output are indexed by b' = b Sq + i where the decode form has b: the merge kernel is the same.  Everything else -- the tiles, the
// LDS image, the reads, the counted waits, the waves' merge -- is the code below, shared; ROWS = false compiles to the decode kernel.
template <int D, bool ROWS = false>
__global__ __launch_bounds__(256) void decode_attn_kv8_kernel(const DecAttn8Args a) {
  constexpr int BK = 64;              // keys per tile
  constexpr int CPR = D / 16;         // 16-byte chunks per tile row
  constexpr int ROWB = D;             // bytes per tile row
  constexpr int TILE = BK * ROWB;     // bytes per K (or V) tile
  constexpr int STAGE = 2 * TILE + 512;  // [K tile | V tile | 64 K scales | 64 V scales]
  constexpr int NP = CPR;             // 16-byte DMA pieces per lane per tile
  constexpr int KS = D / 32;          // k steps of Q K^T = 32-wide d blocks of O^T
  extern __shared__ __attribute__((aligned(16))) char lds[];  // per wave: two stages; then the waves' merge

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  char* const wl = lds + w * 2 * STAGE;

  const int sp = blockIdx.x % a.ns;
  const int rb = ROWS ? (blockIdx.x / a.ns) % a.nrb : 0;  // row block
  const int bh = ROWS ? blockIdx.x / a.ns / a.nrb : blockIdx.x / a.ns;
  const int hkv = bh % a.Hkv, b = bh / a.Hkv;
  const int T = a.T, G = a.G;
  const int ntile = (T + BK - 1) / BK;
  const int kvs = a.kv_start ? max(0, min(a.kv_start[b], T)) : 0;
  // ROWS: the block's live rows, the lane's row f = (position r_i, head r_gh) and its visible keys [j_lo, j_hi]; the block's edges:
  // e_hi = the first row's diagonal (a tile reaching beyond it is masked), e_lo = the last row's lower edge (a tile starting below it is)
  // (the decode form reads none of the six: its expressions stand where they stood)
  int nlive = G, r_i = 0, r_gh = min(l15, G - 1), j_lo = 0, j_hi = 0, e_lo = 0, e_hi = 0, t_first = 0, t_end = 0;
  if constexpr (ROWS) {
    const int c = T - a.Sq, W = a.window, f0 = rb * 16;
    nlive = min(16, a.Sq * G - f0);
    const int f = f0 + min(l15, nlive - 1);
    r_i = f / G;
    r_gh = f - r_i * G;
    const int i0 = f0 / G, i1 = (f0 + nlive - 1) / G;
    j_hi = r_i + c;
    j_lo = W > 0 ? max(kvs, r_i + c - W + 1) : kvs;
    e_hi = i0 + c;
    e_lo = W > 0 ? max(kvs, i1 + c - W + 1) : kvs;
    const int k_lo = W > 0 ? max(kvs, i0 + c - W + 1) : kvs;  // the block's keys: k_lo .. i1 + c, every one seen by some row
    t_first = k_lo / BK;
    t_end = k_lo > i1 + c ? t_first : (i1 + c) / BK + 1;      // (kv_start beyond the last row's diagonal: no tile)
  }
  const int t_lo = ROWS ? max(sp * a.tps, t_first) : max(sp * a.tps, kvs / BK);
  const int t_hi = ROWS ? min(t_end, sp * a.tps + a.tps) : min(ntile, sp * a.tps + a.tps);

  const uint8_t* kb_ = a.k + ((int64_t)b * a.Hkv + hkv) * a.kv_stride;
  const uint8_t* vb_ = a.v + ((int64_t)b * a.Hkv + hkv) * a.kv_stride;
  const float* ksb = a.ks + ((int64_t)b * a.Hkv + hkv) * a.sc_stride;
  const float* vsb = a.vs + ((int64_t)b * a.Hkv + hkv) * a.sc_stride;

  // ---- LDS-DMA of one tile by one wave: piece i of a lane is LDS chunk c = i * 64 + lane = (row c / CPR, position c % CPR), which holds
  // the row's chunk position ^ swz(row) (the swizzle on the SOURCE address); the two scale pieces are 4 bytes per lane, lane = key.
  // Rows and scales past the last key read a copy of it (masked below): nothing beyond position T - 1 is touched
  auto dma = [&](int kt, char* dst) {
    const int last = T - 1 - kt * BK;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int c = i * 64 + lane, row = c / CPR, cp = c % CPR;
      const int off = min(row, last) * ROWB + ((cp ^ da8_swz<D>(row)) << 4);
      lds_dma_mubuf16(kb_, dst + i * 1024, off, kt * TILE);
      lds_dma_mubuf16(vb_, dst + TILE + i * 1024, off, kt * TILE);
    }
    lds_dma_mubuf4(ksb, dst + 2 * TILE, min(lane, last) * 4, kt * BK * 4);
    lds_dma_mubuf4(vsb, dst + 2 * TILE + 256, min(lane, last) * 4, kt * BK * 4);
  };

  int kt = t_lo + w;
  if (kt < t_hi) dma(kt, wl);
  // ---- the group's queries (B operand), as decode_attn_kernel has them
  bf16x8 qf[KS];
  {
    const bf16_t* qp = ROWS ? a.q + ((int64_t)b * a.Sq + r_i) * a.ldq + (int64_t)(hkv * G + r_gh) * D + g * 8
                            : a.q + (int64_t)b * a.ldq + (int64_t)(hkv * G + min(l15, G - 1)) * D + g * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
      if (l15 >= nlive) qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  // ---- per-lane byte offsets into a stage.  K: key l15 of a 16-key block, the 8 codes d = 32 ks + 8 g .. + 7.  V: the lane supplies the
  // address of key 4 g + (l15 >> 2) of a 16-key block, bytes 32 blk + 8 (l15 & 3) .. + 7 (four byte pairs)
  const int v_row = 4 * g + (l15 >> 2);
  uint32_t ka[KS], va[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    ka[s] = l15 * ROWB + (((2 * s + (g >> 1)) ^ da8_swz<D>(l15)) << 4) + (g & 1) * 8;
    va[s] = TILE + v_row * ROWB + (((2 * s + ((l15 & 3) >> 1)) ^ da8_swz<D>(v_row)) << 4) + (l15 & 1) * 8;
  }
  const uint32_t sa_off = 2 * TILE + 16 * g;

  f32x4 oe[KS], oo[KS];  // O^T rows of the even / odd d of each 32-wide block
#pragma unroll
  for (int s = 0; s < KS; ++s) oe[s] = oo[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float c_scale = a.scale_log2e;

  for (int it = 0; kt < t_hi; kt += 4, ++it) {
    const int stage = it & 1;
    if (kt + 4 < t_hi) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      dma(kt + 4, wl + (stage ^ 1) * STAGE);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP + 2) : "memory");  // tile kt has landed; tile kt + 4 stays in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const uint32_t st = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(wl + stage * STAGE);
    // ---- the tile's K codes (four 16-key blocks x KS steps) and its scales (the lane's keys 16 kb + 4 g .. + 3 of each block)
    da_u2_t kc[4][KS];
    f32x4 ksc[4], vsc[4];
    {
      const uint32_t sa = st + sa_off;
      uint32_t ad[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) ad[s] = st + ka[s];
      if constexpr (D == 64) {
        asm volatile(DA8_SCALES DA8_L2("ds_read_b64", "k0", "") DA8_L2("ds_read_b64", "k1", " offset:1024") DA8_L2("ds_read_b64", "k2", " offset:2048")
                         DA8_L2("ds_read_b64", "k3", " offset:3072") "s_waitcnt lgkmcnt(0)"
                     : DA8_OUT_SC, DA8_OUT2(k, kc)
                     : [sa] "v"(sa), [a0] "v"(ad[0]), [a1] "v"(ad[1])
                     : "memory");
      } else if constexpr (D == 96) {
        asm volatile(DA8_SCALES DA8_L3("ds_read_b64", "k0", "") DA8_L3("ds_read_b64", "k1", " offset:1536") DA8_L3("ds_read_b64", "k2", " offset:3072")
                         DA8_L3("ds_read_b64", "k3", " offset:4608") "s_waitcnt lgkmcnt(0)"
                     : DA8_OUT_SC, DA8_OUT3(k, kc)
                     : [sa] "v"(sa), [a0] "v"(ad[0]), [a1] "v"(ad[1]), [a2] "v"(ad[2])
                     : "memory");
      } else {
        asm volatile(DA8_SCALES DA8_L4("ds_read_b64", "k0", "") DA8_L4("ds_read_b64", "k1", " offset:2048") DA8_L4("ds_read_b64", "k2", " offset:4096")
                         DA8_L4("ds_read_b64", "k3", " offset:6144") "s_waitcnt lgkmcnt(0)"
                     : DA8_OUT_SC, DA8_OUT4(k, kc)
                     : [sa] "v"(sa), [a0] "v"(ad[0]), [a1] "v"(ad[1]), [a2] "v"(ad[2]), [a3] "v"(ad[3])
                     : "memory");
      }
    }
    // ---- S^T = K Q^T per 16-key block, two accumulator chains; then the keys' scales
    float x[16], pv[16];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kf = w8_widen(kc[kb][ks].x, kc[kb][ks].y);
        if (ks & 1) acc1 = mfma16(kf, qf[ks], acc1);
        else acc0 = mfma16(kf, qf[ks], acc0);
      }
      const f32x4 sc = acc0 + acc1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[4 * kb + r] = sc[r] * ksc[kb][r];
        pv[4 * kb + r] = vsc[kb][r] * DA8_PRE;  // (a power of two: exact)
      }
    }
    // ---- online softmax: the lane owns keys kt * 64 + 16 (i >> 2) + 4 g + (i & 3) of head l15
    // (wave-uniform) the partial first / last tile of the visible range; ROWS: a tile that an edge of one of the block's rows crosses
    if (ROWS ? kt * BK < e_lo || kt * BK + BK - 1 > e_hi : kt * BK < kvs || kt * BK + BK > T) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = kt * BK + (i >> 2) * 16 + 4 * g + (i & 3);
        if (ROWS ? j < j_lo || j > j_hi : j < kvs || j >= T) x[i] = -INFINITY, pv[i] = 0.f;
      }
    }
    float mt = x[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mt = fmaxf(mt, x[i]);
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    mt *= c_scale;
    const float m_new = fmaxf(m_run, mt);
    const float alpha = da_merge(m_run, m_new);
    const float m_sub = m_new == -INFINITY ? 0.f : m_new;
    m_run = m_new;
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(x[i], c_scale, -m_sub));
      ps += x[i];          // (the row sum takes the unscaled p)
      pv[i] *= x[i];       // p_j vs[j] PRE: one fp32 rounding, then the element type's below
    }
    l_run = l_run * alpha + ps;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      oe[s][0] *= alpha; oe[s][1] *= alpha; oe[s][2] *= alpha; oe[s][3] *= alpha;
      oo[s][0] *= alpha; oo[s][1] *= alpha; oo[s][2] *= alpha; oo[s][3] *= alpha;
    }
    // P fragments, one per 32-key half hh: k-slot (g, e) carries key 32 hh + 16 (e >> 2) + 4 g + (e & 3)
    union { bf16x8 v; uint32_t u[4]; } pf[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int j = 0; j < 4; ++j) pf[hh].u[j] = pack2_bf16(pv[8 * hh + 2 * j], pv[8 * hh + 2 * j + 1]);
    // ---- O^T += V^T P^T: per 32-wide d block four transposed reads (keys +0, +16 | +32, +48: the two halves' lo and hi)
    da_u2_t vt[4][KS];
    {
      uint32_t ad[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) ad[s] = st + va[s];
      if constexpr (D == 64) {
        asm volatile(DA8_L2("ds_read_b64_tr_b16", "v0", "") DA8_L2("ds_read_b64_tr_b16", "v1", " offset:1024")
                         DA8_L2("ds_read_b64_tr_b16", "v2", " offset:2048") DA8_L2("ds_read_b64_tr_b16", "v3", " offset:3072") "s_waitcnt lgkmcnt(0)"
                     : DA8_OUT2(v, vt)
                     : [a0] "v"(ad[0]), [a1] "v"(ad[1])
                     : "memory");
      } else if constexpr (D == 96) {
        asm volatile(DA8_L3("ds_read_b64_tr_b16", "v0", "") DA8_L3("ds_read_b64_tr_b16", "v1", " offset:1536")
                         DA8_L3("ds_read_b64_tr_b16", "v2", " offset:3072") DA8_L3("ds_read_b64_tr_b16", "v3", " offset:4608") "s_waitcnt lgkmcnt(0)"
                     : DA8_OUT3(v, vt)
                     : [a0] "v"(ad[0]), [a1] "v"(ad[1]), [a2] "v"(ad[2])
                     : "memory");
      } else {
        asm volatile(DA8_L4("ds_read_b64_tr_b16", "v0", "") DA8_L4("ds_read_b64_tr_b16", "v1", " offset:2048")
                         DA8_L4("ds_read_b64_tr_b16", "v2", " offset:4096") DA8_L4("ds_read_b64_tr_b16", "v3", " offset:6144") "s_waitcnt lgkmcnt(0)"
                     : DA8_OUT4(v, vt)
                     : [a0] "v"(ad[0]), [a1] "v"(ad[1]), [a2] "v"(ad[2]), [a3] "v"(ad[3])
                     : "memory");
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        // a dword = (key 2 t: d even, d odd | key 2 t + 1: d even, d odd); lo = the half's keys 4 g .. + 3, hi = 16 + 4 g .. + 3
        const da_u2_t lo = vt[2 * hh][s], hi = vt[2 * hh + 1][s];
        const f32x2 c0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo.x, false), c1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo.x, true);
        const f32x2 c2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo.y, false), c3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo.y, true);
        const f32x2 c4 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi.x, false), c5 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi.x, true);
        const f32x2 c6 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi.y, false), c7 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi.y, true);
        const u32x4 ev = {pack2_bf16(c0.x, c1.x), pack2_bf16(c2.x, c3.x), pack2_bf16(c4.x, c5.x), pack2_bf16(c6.x, c7.x)};
        const u32x4 od = {pack2_bf16(c0.y, c1.y), pack2_bf16(c2.y, c3.y), pack2_bf16(c4.y, c5.y), pack2_bf16(c6.y, c7.y)};
        oe[s] = mfma16(__builtin_bit_cast(bf16x8, ev), pf[hh].v, oe[s]);
        oo[s] = mfma16(__builtin_bit_cast(bf16x8, od), pf[hh].v, oo[s]);
      }
#endif
  }

  // ---- the four waves' states meet in LDS (wave order): lane holds O^T[d = 32 s + 8 g + 2 r (+ 1)][head l15]
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  __syncthreads();  // every wave is done with its tiles: the staging area is free
  float* const so = reinterpret_cast<float*>(lds);  // [4][16][D]
  float* const sml = so + 4 * 16 * D;               // [4][16][2]
  if (l15 < nlive) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      float* const p = so + (w * 16 + l15) * D + 32 * s + 8 * g;
      *reinterpret_cast<float4*>(p) = float4{oe[s][0], oo[s][0], oe[s][1], oo[s][1]};
      *reinterpret_cast<float4*>(p + 4) = float4{oe[s][2], oo[s][2], oe[s][3], oo[s][3]};
    }
    if (g == 0) {
      sml[(w * 16 + l15) * 2] = m_run;
      sml[(w * 16 + l15) * 2 + 1] = l_tot;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < nlive * (D / 4); idx += 256) {
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
    const int oi = ROWS ? (rb * 16 + qh) / G : 0;                       // ROWS: row qh of the block = (position oi, head)
    const int head = hkv * G + (ROWS ? rb * 16 + qh - oi * G : qh);
    const int64_t ob = ROWS ? (int64_t)b * a.Sq + oi : (int64_t)b;      // the row of out and of the partials
    const int64_t nb = ROWS ? (int64_t)a.B * a.Sq : (int64_t)a.B;
    if (a.ns == 1) {
      const float inv = (L > 0.f ? 1.f / L : 0.f) * DA8_PRE_INV;  // no visible key: zeros
      *reinterpret_cast<uint2*>(a.out + ob * a.ldo + head * D + c4) =
          uint2{pack2_bf16(acc[0] * inv, acc[1] * inv), pack2_bf16(acc[2] * inv, acc[3] * inv)};
    } else {  // (the partials leave without the pre-scale: decode_attn_merge_kernel is the 16-bit kernel's)
      const int64_t e = ((int64_t)sp * nb + ob) * a.Hq + head;
      *reinterpret_cast<float4*>(a.opart + e * D + c4) =
          float4{acc[0] * DA8_PRE_INV, acc[1] * DA8_PRE_INV, acc[2] * DA8_PRE_INV, acc[3] * DA8_PRE_INV};
      if (c4 == 0) {
        a.ml[e * 2] = m;
        a.ml[e * 2 + 1] = L;
      }
    }
  }
}

// The splits are those of the 16-bit kernel on the same (B, Hkv, T), counted in 64-key tiles: never more partials than its
// workspace holds, so decoder_decode_workspace_bytes covers the step on either cache.
size_t decode_attention_kv8_workspace_bytes(int B, int Hq, int Hkv, int T, int D) { return decode_attention_workspace_bytes(B, Hq, Hkv, T, D); }

int decode_attention_kv8(const bf16_t* q, const uint8_t* Kc, const uint8_t* Vc, const float* Ks, const float* Vs, bf16_t* out, int B, int Hq,
                         int Hkv, int T, int D, int64_t ldq, int64_t kv_stride, int64_t sc_stride, int64_t ldo, float scale,
                         const int* kv_start, void* ws, size_t ws_bytes, bool check_only, hipStream_t stream) {
  if (!q || !Kc || !Vc || !Ks || !Vs || !out || B <= 0 || B > 65535 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || Hq / Hkv > 16) return U2_ERR_ARG;
  if (D != 64 && D != 96 && D != 128) return U2_ERR_ARG;
  if (kv_stride == 0) kv_stride = (int64_t)T * D;
  if (sc_stride == 0) sc_stride = T;
  if (kv_stride < (int64_t)T * D || (kv_stride & 15) || sc_stride < T || (int64_t)T * D >= (1ll << 31)) return U2_ERR_ARG;  // (32-bit DMA offsets)
  if (ldq < (int64_t)Hq * D || ldo < (int64_t)Hq * D || (ldq & 7) || (ldo & 3) || !(scale > 0.f)) return U2_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)Kc | (uintptr_t)Vc) & 15) || ((uintptr_t)out & 7) || (((uintptr_t)kv_start | (uintptr_t)Ks | (uintptr_t)Vs) & 3))
    return U2_ERR_ARG;
  DecAttn8Args a;
  a.q = q; a.k = Kc; a.v = Vc; a.ks = Ks; a.vs = Vs; a.out = out; a.kv_start = kv_start;
  a.ldq = ldq; a.ldo = ldo; a.kv_stride = kv_stride; a.sc_stride = sc_stride;
  a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.T = T;
  a.Sq = 1; a.nrb = 1; a.window = 0;  // (read by the rows form only)
  a.scale_log2e = scale * 1.44269504088896340736f;
  const int ntile = (int)cdiv(T, 64);
  int ns = ws ? std::min(dec_attn_splits(B, Hkv, T), ntile) : 1;  // (no workspace: unsplit)
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
  if (check_only) return U2_OK;
  ProfScope ps(PROF_TOKATTN, 4.0 * B * Hq * (double)T * D, stream, 2.0 * B * D * 2.0 * Hq + 2.0 * B * Hkv * (double)T * (D + 4.0));
#define U2_DA8(D_)                                                                                                          \
  do {                                                                                                                      \
    constexpr size_t smem_ = 4 * 2 * (2 * 64 * (D_) + 512);  /* 4 waves x 2 stages; >= the merge's 4 x 16 x D floats + 512 */ \
    static_assert(smem_ >= 4 * 16 * (D_) * 4 + 512, "merge area");                                                          \
    hipLaunchKernelGGL((decode_attn_kv8_kernel<D_>), dim3((unsigned)grid), dim3(256), smem_, stream, a);                    \
  } while (0)
  if (D == 128) U2_DA8(128);
  else if (D == 96) U2_DA8(96);
  else U2_DA8(64);
#undef U2_DA8
  if (a.ns > 1) {
    DecAttnArgs m;
    m.q = nullptr; m.k = nullptr; m.v = nullptr; m.out = out; m.kv_start = nullptr;
    m.ldq = ldq; m.ldo = ldo; m.kv_stride = 0;
    m.B = B; m.Hq = Hq; m.Hkv = Hkv; m.G = a.G; m.T = T; m.ns = a.ns; m.tps = a.tps;
    m.scale_log2e = a.scale_log2e; m.opart = a.opart; m.ml = a.ml;
    const int64_t total = (int64_t)B * Hq * (D / 4);
    hipLaunchKernelGGL(decode_attn_merge_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, m, D);
  }
  return launch_status();
}

// ---- the rows form: Sq new positions per sequence against the codes (the continued prefill on an e4m3 cache).  nrb row blocks of 16
// flat rows per (sequence, kv head); the splits are dec_attn_splits' on B nrb where the decode entry has B, so Sq = 1 has the decode
// entry's grid, splits and bits.  The cache is streamed once per row block: the form for FEW new positions.
static int da8_row_blocks(int Sq, int G) { return (int)cdiv((int64_t)Sq * G, 16); }
static int da8_rows_splits(int B, int Sq, int Hq, int Hkv, int T) {
  const int64_t blocks = (int64_t)B * da8_row_blocks(Sq, Hq / Hkv);
  return std::min(dec_attn_splits((int)std::min<int64_t>(blocks, 1 << 30), Hkv, T), (int)cdiv(T, 64));
}

size_t attention_kv8_rows_workspace_bytes(int B, int Sq, int Hq, int Hkv, int T, int D) {
  if (B <= 0 || Sq <= 0 || Hq <= 0 || Hkv <= 0 || T <= 0 || D <= 0 || Hq % Hkv) return 0;
  const int ns = da8_rows_splits(B, Sq, Hq, Hkv, T);
  return ns > 1 ? (size_t)ns * B * Sq * Hq * ((size_t)D * 4 + 8) : 0;
}

int attention_kv8_rows(const bf16_t* q, const uint8_t* Kc, const uint8_t* Vc, const float* Ks, const float* Vs, bf16_t* out, int B, int Sq,
                       int Hq, int Hkv, int T, int D, int64_t ldq, int64_t kv_stride, int64_t sc_stride, int64_t ldo, float scale, int window,
                       const int* kv_start, void* ws, size_t ws_bytes, bool check_only, hipStream_t stream) {
  if (!q || !Kc || !Vc || !Ks || !Vs || !out || B <= 0 || B > 65535 || T <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || Hq / Hkv > 16) return U2_ERR_ARG;
  if (D != 64 && D != 96 && D != 128) return U2_ERR_ARG;
  if (Sq < 1 || Sq > T || window < 0 || (int64_t)B * Sq > 0x7fffffff / Hq) return U2_ERR_ARG;  // (the merge's 32-bit row and head)
  if (kv_stride == 0) kv_stride = (int64_t)T * D;
  if (sc_stride == 0) sc_stride = T;
  if (kv_stride < (int64_t)T * D || (kv_stride & 15) || sc_stride < T || (int64_t)T * D >= (1ll << 31)) return U2_ERR_ARG;  // (32-bit DMA offsets)
  if (ldq < (int64_t)Hq * D || ldo < (int64_t)Hq * D || (ldq & 7) || (ldo & 3) || !(scale > 0.f)) return U2_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)Kc | (uintptr_t)Vc) & 15) || ((uintptr_t)out & 7) || (((uintptr_t)kv_start | (uintptr_t)Ks | (uintptr_t)Vs) & 3))
    return U2_ERR_ARG;
  DecAttn8Args a;
  a.q = q; a.k = Kc; a.v = Vc; a.ks = Ks; a.vs = Vs; a.out = out; a.kv_start = kv_start;
  a.ldq = ldq; a.ldo = ldo; a.kv_stride = kv_stride; a.sc_stride = sc_stride;
  a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.T = T;
  a.Sq = Sq; a.nrb = da8_row_blocks(Sq, a.G); a.window = window;
  a.scale_log2e = scale * 1.44269504088896340736f;
  const int ntile = (int)cdiv(T, 64);
  const int ns = ws ? da8_rows_splits(B, Sq, Hq, Hkv, T) : 1;  // (no workspace: unsplit)
  a.tps = (int)cdiv(ntile, ns);
  a.ns = (int)cdiv(ntile, a.tps);  // no split beyond the last tile
  a.opart = nullptr; a.ml = nullptr;
  const size_t rows = (size_t)B * Sq;
  if (a.ns > 1) {
    if (ws_bytes < (size_t)a.ns * rows * Hq * ((size_t)D * 4 + 8)) return U2_ERR_WORKSPACE;
    if ((uintptr_t)ws & 15) return U2_ERR_ARG;
    a.opart = reinterpret_cast<float*>(ws);
    a.ml = a.opart + (size_t)a.ns * rows * Hq * D;
  }
  const int64_t grid = (int64_t)B * Hkv * a.nrb * a.ns;
  if (grid > 0x7fffffff) return U2_ERR_ARG;
  if (check_only) return U2_OK;
  ProfScope ps(PROF_TOKATTN, 4.0 * rows * Hq * (double)T * D, stream,
               2.0 * rows * D * 2.0 * Hq + 2.0 * B * Hkv * (double)a.nrb * (double)T * (D + 4.0));
#define U2_DA8R(D_)                                                                                                         \
  do {                                                                                                                      \
    constexpr size_t smem_ = 4 * 2 * (2 * 64 * (D_) + 512);  /* the decode form's: 4 waves x 2 stages; >= the merge area */   \
    static_assert(smem_ >= 4 * 16 * (D_) * 4 + 512, "merge area");                                                          \
    hipLaunchKernelGGL((decode_attn_kv8_kernel<D_, true>), dim3((unsigned)grid), dim3(256), smem_, stream, a);              \
  } while (0)
  if (D == 128) U2_DA8R(128);
  else if (D == 96) U2_DA8R(96);
  else U2_DA8R(64);
#undef U2_DA8R
  if (a.ns > 1) {
    DecAttnArgs m;
    m.q = nullptr; m.k = nullptr; m.v = nullptr; m.out = out; m.kv_start = nullptr;
    m.ldq = ldq; m.ldo = ldo; m.kv_stride = 0;
    m.B = (int)rows; m.Hq = Hq; m.Hkv = Hkv; m.G = a.G; m.T = T; m.ns = a.ns; m.tps = a.tps;
    m.scale_log2e = a.scale_log2e; m.opart = a.opart; m.ml = a.ml;
    const int64_t total = (int64_t)rows * Hq * (D / 4);
    hipLaunchKernelGGL(decode_attn_merge_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, m, D);
  }
  return launch_status();
}
}  // namespace u2
