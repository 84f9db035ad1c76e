// Backward of the decoder's causal grouped-query attention (training route of u2tokenizer_amd/decoder_train.py):
//   out = softmax(q k^T * scale + causal / key-length mask) v   ->   dq, dk, dv   from q, k, v, out, d_out (+ the forward's lse)
// for head dims 64 and 128.  The kernel pair of attn_bwd.hip (the ViT's d = 64, non-causal, equal-heads backward) is the
// template: two kernels, no atomics, bit-repeatable, transposed fragments by ds_read_b64_tr_b16, XCD-aware order.  What
// differs:
//   * the mask: query i of sequence b sees key j iff j <= i and j < kv_len[b] (HF's causal mask built from a right-padded
//     2-D attention mask; kv_len NULL: plain causal).  Work outside the mask is skipped by whole 64-row tiles: the dQ kernel
//     visits keys 0 .. min(last query of its block, kv_len - 1), the dK / dV kernel visits queries from its block's first key
//     on; a dK / dV block whose keys all lie at or beyond kv_len writes zeros.
//   * grouped-query heads: the dQ kernel runs per QUERY head and reads kv head h / G; the dK / dV kernel runs per KV head and
//     sums the contributions of its G query heads in one set of accumulators, heads in ascending order (no atomics).
//   * head dim DH = 64 or 128: tiles of 64 rows x DH, 16-byte chunks XOR-swizzled within each 128-byte half row (the
//     attn_bwd.hip swizzle applied to both halves), DH / 16 k steps, DH / 32 accumulator blocks.
//   * inputs and outputs are strided column views: q, k, v of one packed (rows, (Hq + 2 Hkv) d) buffer (or any other
//     layout with a common leading dim), dq, dk, dv likewise -- the q|k|v product's backward reads one dense gradient.
#include "kernels.h"

namespace u2 {

namespace {

struct GqaBwdArgs {
  const bf16_t *q, *k, *v, *o, *dout;
  bf16_t *dq, *dk, *dv;
  float *lse, *dsum;      // (nb * Hq, S_pad): row statistics handed from the dQ kernel to the dK / dV kernel
  const float* lse_in;    // optional: the forward's (nb * Hq, lse_ld), log2 units
  const int* kv_len;      // optional: (nb) valid keys per sequence
  int64_t lse_ld;
  int S, Hq, Hkv, G, S_pad, nblk, nwg;
  int64_t ld_qkv, bs_qkv, ld_o, bs_o, ld_d, bs_d;
  float scale, scale_log2e;
};

// LDS position of 16-byte chunk `chunk` of row `row` in a [64][DH] tile: the attn_bwd.hip swizzle (chunk ^ rev3((row >> 1) & 7))
// inside each 128-byte half of the row.
template <int DH>
__device__ __forceinline__ uint32_t gtile_off(int row, int chunk) {
  const int p = (row >> 1) & 7;
  const int x = ((p & 1) << 2) | (p & 2) | ((p >> 2) & 1);
  return (uint32_t)(row * (DH * 2) + (((chunk & ~7) | ((chunk & 7) ^ x)) << 4));
}

__device__ __forceinline__ float gdot8(const uint4 a, const uint4 b) {
  float s = 0.f;
  s = __builtin_fmaf(bf16lo(a.x), bf16lo(b.x), s); s = __builtin_fmaf(bf16hi(a.x), bf16hi(b.x), s);
  s = __builtin_fmaf(bf16lo(a.y), bf16lo(b.y), s); s = __builtin_fmaf(bf16hi(a.y), bf16hi(b.y), s);
  s = __builtin_fmaf(bf16lo(a.z), bf16lo(b.z), s); s = __builtin_fmaf(bf16hi(a.z), bf16hi(b.z), s);
  s = __builtin_fmaf(bf16lo(a.w), bf16lo(b.w), s); s = __builtin_fmaf(bf16hi(a.w), bf16hi(b.w), s);
  return s;
}

__device__ __forceinline__ int gxcd_order(int w, int nwg) {
  const int qn = nwg >> 3, rn = nwg & 7;
  const int xcd = w & 7, idx = w >> 3;
  return (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + idx;
}

union GFrag {
  bf16x8 v;
  uint4 q;
  uint32_t u[4];
};

typedef short gv4s_t __attribute__((ext_vector_type(4)));

// A operand "X^T" (32 d rows x 16 k) from a row-major [64][DH] tile, k slots in the order of an accumulator fed back as the
// B operand (attn_bwd.hip: tr_frag): lane (d = 32 nb + (lane & 31), hi = lane >> 5) receives rows r0 + 4 hi + {0..3} and
// r0 + 8 + 4 hi + {0..3} of its column.
template <int DH>
__device__ __forceinline__ bf16x8 gtr_frag(const char* tile, int lane, int nb, int r0) {
  typedef __attribute__((address_space(3))) gv4s_t* lds_v4;
  const int a = lane & 15;
  const int chunk = 4 * nb + 2 * ((lane >> 4) & 1) + ((a & 3) >> 1), sub = (a & 1) * 8;
  const int row1 = r0 + 4 * (lane >> 5) + (a >> 2), row2 = row1 + 8;
  const gv4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(tile + gtile_off<DH>(row1, chunk) + sub));
  const gv4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(tile + gtile_off<DH>(row2, chunk) + sub));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ int kv_len_of(const GqaBwdArgs& a, int b) {
  return a.kv_len ? max(1, min(a.kv_len[b], a.S)) : a.S;
}

// ----------------------------------------------------------------------------------------------------------- dQ
// one workgroup per (batch, query head, 128 query rows); 4 waves x 32 queries; lane = query column, 16 keys per 32-key block
template <int DH, bool HAVE_LSE>
__global__ __launch_bounds__(256, 2) void gqa_bwd_dq_kernel(const GqaBwdArgs a) {
  constexpr int KS = DH / 16, NB = DH / 32, CPR = DH / 8, NLD = 64 * CPR / 256, TILE = 64 * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char glds[];  // [stage][K | V] tiles
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int S = a.S, S_pad = a.S_pad;
  const int vid = gxcd_order(blockIdx.x, a.nwg);
  // causal: the last query blocks of a head have the most keys -- hand those out first
  const int bh = vid / a.nblk, b = bh / a.Hq, h = bh - b * a.Hq;
  const int blk = a.nblk - 1 - (vid - bh * a.nblk);
  const int hkv = h / a.G;
  const float c = a.scale_log2e;
  const int q0 = blk * 128;
  const int wrow0 = q0 + wv * 32;
  const bool wave_active = wrow0 < S;
  const int qrow = min(wrow0 + l31, S - 1);
  const int kvl = kv_len_of(a, b);
  const int64_t ld = a.ld_qkv;
  const bf16_t* kb_ = a.k + (int64_t)b * a.bs_qkv + hkv * DH;
  const bf16_t* vb_ = a.v + (int64_t)b * a.bs_qkv + hkv * DH;

  GFrag qf[KS], dof[KS];
  float dpart = 0.f;
  {
    const bf16_t* qp = a.q + (int64_t)b * a.bs_qkv + (int64_t)qrow * ld + h * DH + hi * 8;
    const bf16_t* op = a.o + (int64_t)b * a.bs_o + (int64_t)qrow * a.ld_o + h * DH + hi * 8;
    const bf16_t* gp = a.dout + (int64_t)b * a.bs_o + (int64_t)qrow * a.ld_o + h * DH + hi * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[ks].q = *reinterpret_cast<const uint4*>(qp + ks * 16);
      dof[ks].q = *reinterpret_cast<const uint4*>(gp + ks * 16);
      const uint4 ov = *reinterpret_cast<const uint4*>(op + ks * 16);
      dpart += gdot8(ov, dof[ks].q);
    }
  }
  const float Dq = dpart + __shfl_xor(dpart, 32, 64);

  int srow[NLD], sch[NLD];
  uint32_t soff[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int cidx = i * 256 + tid;
    srow[i] = cidx / CPR;
    sch[i] = cidx % CPR;
    soff[i] = gtile_off<DH>(srow[i], sch[i]);
  }
  uint4 rk[NLD], rv[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) rv[i] = uint4{0u, 0u, 0u, 0u};
  auto gload = [&](int t, bool full) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int64_t r = (int64_t)min(t * 64 + srow[i], S - 1) * ld + sch[i] * 8;
      rk[i] = *reinterpret_cast<const uint4*>(kb_ + r);
      if (full) rv[i] = *reinterpret_cast<const uint4*>(vb_ + r);
    }
  };
  auto lstore = [&](int st, bool full) {
    char* sK = glds + st * 2 * TILE;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      *reinterpret_cast<uint4*>(sK + soff[i]) = rk[i];
      if (full) *reinterpret_cast<uint4*>(sK + TILE + soff[i]) = rv[i];
    }
  };
  // keys visited: 0 .. min(last query of the block, kv_len - 1)
  const int ntile = (min(min(q0 + 128, S), kvl) + 63) >> 6;
  // masks a tile's scores: key kk invisible to this lane's query (kk > query or kk >= kv_len) -> -inf
  auto mask = [&](f32x16* sc, int t) {
    if (t * 64 + 63 > wrow0 || t * 64 + 64 > kvl) {  // wave-uniform
      const int kvb = t * 64 + 4 * hi;
      const int qi = wrow0 + l31;
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = kvb + kbk * 32 + (r & 3) + 8 * (r >> 2);
          if (kk > qi || kk >= kvl) sc[kbk][r] = -INFINITY;
        }
    }
  };

  float m_run = -INFINITY, l_run = 0.f;
  if constexpr (!HAVE_LSE) {
    gload(0, false);
    lstore(0, false);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks].v), "+v"(dof[ks].v));
    for (int t = 0; t < ntile; ++t) {
      const int st = t & 1;
      if (t + 1 < ntile) gload(t + 1, false);
      if (wave_active) {
        const char* sK = glds + st * 2 * TILE;
        f32x16 sc[2];
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[kbk][r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + gtile_off<DH>(kbk * 32 + l31, ks * 2 + hi));
            sc[kbk] = mfma32(kf, qf[ks].v, sc[kbk]);
          }
        }
        mask(sc, t);
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx[r & 3] = fmaxf(mx[r & 3], sc[kbk][r]);
        float mt = fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3]));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * c;
        const float m_new = fmaxf(m_run, mt);  // finite from tile 0 on: key 0 is visible to every query
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
          for (int r = 0; r < 16; ++r) ps[r & 3] += __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kbk][r], c, -m_new));
        l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + ((ps[0] + ps[1]) + (ps[2] + ps[3]));
        m_run = m_new;
      }
      if (t + 1 < ntile) lstore((t + 1) & 1, false);
      __syncthreads();
    }
  }
  float lse = 0.f;
  if constexpr (HAVE_LSE) {
    lse = a.lse_in[(int64_t)bh * a.lse_ld + qrow];
  } else if (wave_active) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    lse = m_run + __builtin_log2f(l_tot);
  }
  if (wave_active && hi == 0 && wrow0 + l31 < S) {  // for the dK / dV kernel
    a.lse[(int64_t)bh * S_pad + wrow0 + l31] = lse;
    a.dsum[(int64_t)bh * S_pad + wrow0 + l31] = Dq;
  }

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
  gload(0, true);
  lstore(0, true);
  __syncthreads();
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks].v), "+v"(dof[ks].v));
  for (int t = 0; t < ntile; ++t) {
    const int st = t & 1;
    if (t + 1 < ntile) gload(t + 1, true);
    if (wave_active && t * 64 <= wrow0 + 31) {  // (a tile wholly past this wave's diagonal contributes nothing)
      const char* sK = glds + st * 2 * TILE;
      const char* sV = sK + TILE;
      f32x16 sc[2], dp[2];
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc[kbk][r] = 0.f; dp[kbk][r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + gtile_off<DH>(kbk * 32 + l31, ks * 2 + hi));
          sc[kbk] = mfma32(kf, qf[ks].v, sc[kbk]);
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sV + gtile_off<DH>(kbk * 32 + l31, ks * 2 + hi));
          dp[kbk] = mfma32(vf, dof[ks].v, dp[kbk]);
        }
      }
      mask(sc, t);
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kbk][r], c, -lse));
          sc[kbk][r] = p * (dp[kbk][r] - Dq);
        }
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          GFrag pf;
#pragma unroll
          for (int j = 0; j < 4; ++j) pf.u[j] = pack2_bf16(sc[kbk][ks2 * 8 + 2 * j], sc[kbk][ks2 * 8 + 2 * j + 1]);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const bf16x8 tf = gtr_frag<DH>(sK, lane, nb, kbk * 32 + ks2 * 16);
            acc[nb] = mfma32(tf, pf.v, acc[nb]);
          }
        }
    }
    if (t + 1 < ntile) lstore((t + 1) & 1, true);
    __syncthreads();
  }
  if (wave_active && wrow0 + l31 < S) {
    bf16_t* op = a.dq + (int64_t)b * a.bs_d + (int64_t)(wrow0 + l31) * a.ld_d + h * DH;
    const float sc_ = a.scale;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2*>(op + nb * 32 + 8 * g + 4 * hi) =
            uint2{pack2_bf16(acc[nb][4 * g] * sc_, acc[nb][4 * g + 1] * sc_),
                  pack2_bf16(acc[nb][4 * g + 2] * sc_, acc[nb][4 * g + 3] * sc_)};
  }
}

// ----------------------------------------------------------------------------------------------------------- dK, dV
// one workgroup per (batch, kv head, 128 keys); 4 waves x 32 keys; lane = key column, 16 queries per 32-query block; the
// G query heads of the kv head one after the other into the same accumulators
// (d = 128: K, V fragments and the dK, dV accumulators are 192 registers -- one wave per SIMD and the whole register file
// instead of spilling at two)
template <int DH>
__global__ __launch_bounds__(256, DH >= 128 ? 1 : 2) void gqa_bwd_dkv_kernel(const GqaBwdArgs a) {
  constexpr int KS = DH / 16, NB = DH / 32, CPR = DH / 8, NLD = 64 * CPR / 256, TILE = 64 * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char glds[];  // [stage][Q | dO] tiles, then stat[stage][lse | D][64]
  float* const stat = reinterpret_cast<float*>(glds + 4 * TILE);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int S = a.S, S_pad = a.S_pad;
  const int vid = gxcd_order(blockIdx.x, a.nwg);
  const int bh = vid / a.nblk, b = bh / a.Hkv, hkv = bh - b * a.Hkv;
  const int blk = vid - bh * a.nblk;  // (the first key blocks see the most queries and come first)
  const float c = a.scale_log2e;
  const int k0 = blk * 128;
  const int wkey0 = k0 + wv * 32;
  const bool wave_active = wkey0 < S;
  const int kkey = wkey0 + l31;
  const int krow = min(kkey, S - 1);
  const int kvl = kv_len_of(a, b);
  const int64_t ld = a.ld_qkv;

  f32x16 accV[NB], accK[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accV[nb][r] = 0.f; accK[nb][r] = 0.f; }

  const int t0 = k0 >> 6, ntq = (S + 63) >> 6;
  const int nit = k0 < kvl ? a.G * (ntq - t0) : 0;  // (keys all at or beyond kv_len: no query sees them, gradients are 0)
  if (nit > 0) {
    GFrag kf[KS], vf[KS];
    {
      const bf16_t* kp = a.k + (int64_t)b * a.bs_qkv + (int64_t)krow * ld + hkv * DH + hi * 8;
      const bf16_t* vp = a.v + (int64_t)b * a.bs_qkv + (int64_t)krow * ld + hkv * DH + hi * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        kf[ks].q = *reinterpret_cast<const uint4*>(kp + ks * 16);
        vf[ks].q = *reinterpret_cast<const uint4*>(vp + ks * 16);
      }
    }
    int srow[NLD], sch[NLD];
    uint32_t soff[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int cidx = i * 256 + tid;
      srow[i] = cidx / CPR;
      sch[i] = cidx % CPR;
      soff[i] = gtile_off<DH>(srow[i], sch[i]);
    }
    uint4 rq[NLD], rg[NLD];
    float4 rs = {0.f, 0.f, 0.f, 0.f};
    // iteration it = (query head g = it / (ntq - t0), query tile t = t0 + it % (ntq - t0))
    auto gload = [&](int it) {
      const int g = it / (ntq - t0), t = t0 + it % (ntq - t0);
      const int h = hkv * a.G + g;
      const bf16_t* qb_ = a.q + (int64_t)b * a.bs_qkv + h * DH;
      const bf16_t* gb_ = a.dout + (int64_t)b * a.bs_o + h * DH;
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int qr = min(t * 64 + srow[i], S - 1);
        rq[i] = *reinterpret_cast<const uint4*>(qb_ + (int64_t)qr * ld + sch[i] * 8);
        rg[i] = *reinterpret_cast<const uint4*>(gb_ + (int64_t)qr * a.ld_o + sch[i] * 8);
      }
      if (tid < 32) {
        const int64_t bhq = (int64_t)b * a.Hq + h;
        const int qq = t * 64 + (tid & 15) * 4;
        rs = *reinterpret_cast<const float4*>((tid < 16 ? a.lse : a.dsum) + bhq * S_pad + qq);
        const float fill = tid < 16 ? INFINITY : 0.f;  // queries past the end: probabilities exactly 0
        if (qq + 0 >= S) rs.x = fill;
        if (qq + 1 >= S) rs.y = fill;
        if (qq + 2 >= S) rs.z = fill;
        if (qq + 3 >= S) rs.w = fill;
      }
    };
    auto lstore = [&](int st) {
      char* sQ = glds + st * 2 * TILE;
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        *reinterpret_cast<uint4*>(sQ + soff[i]) = rq[i];
        *reinterpret_cast<uint4*>(sQ + TILE + soff[i]) = rg[i];
      }
      if (tid < 32) *reinterpret_cast<float4*>(stat + (st * 2 + (tid >> 4)) * 64 + (tid & 15) * 4) = rs;
    };
    gload(0);
    lstore(0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(kf[ks].v), "+v"(vf[ks].v));
    for (int it = 0; it < nit; ++it) {
      const int st = it & 1;
      const int t = t0 + it % (ntq - t0);
      if (it + 1 < nit) gload(it + 1);
      if (wave_active && t * 64 + 63 >= wkey0 && wkey0 < kvl) {  // (queries of the tile all before this wave's keys: nothing)
        const char* sQ = glds + st * 2 * TILE;
        const char* sG = sQ + TILE;
        const float* sl = stat + st * 2 * 64;
        const bool need_mask = t * 64 < wkey0 + 32 || kvl < wkey0 + 32;  // wave-uniform
#pragma unroll
        for (int qbk = 0; qbk < 2; ++qbk) {
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 qa = *reinterpret_cast<const bf16x8*>(sQ + gtile_off<DH>(qbk * 32 + l31, ks * 2 + hi));
            s = mfma32(qa, kf[ks].v, s);
            const bf16x8 ga = *reinterpret_cast<const bf16x8*>(sG + gtile_off<DH>(qbk * 32 + l31, ks * 2 + hi));
            dp = mfma32(ga, vf[ks].v, dp);
          }
          if (need_mask) {
            const int qb = t * 64 + qbk * 32 + 4 * hi;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int qi = qb + (r & 3) + 8 * (r >> 2);
              if (kkey > qi || kkey >= kvl) s[r] = -INFINITY;
            }
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float4 l4 = *reinterpret_cast<const float4*>(&sl[qbk * 32 + 8 * g + 4 * hi]);
            const float4 d4 = *reinterpret_cast<const float4*>(&sl[64 + qbk * 32 + 8 * g + 4 * hi]);
            const float le[4] = {l4.x, l4.y, l4.z, l4.w}, de[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[4 * g + e], c, -le[e]));
              s[4 * g + e] = p;
              dp[4 * g + e] = p * (dp[4 * g + e] - de[e]);
            }
          }
#pragma unroll
          for (int ks2 = 0; ks2 < 2; ++ks2) {
            GFrag pp, ps;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              pp.u[j] = pack2_bf16(s[ks2 * 8 + 2 * j], s[ks2 * 8 + 2 * j + 1]);
              ps.u[j] = pack2_bf16(dp[ks2 * 8 + 2 * j], dp[ks2 * 8 + 2 * j + 1]);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
              const bf16x8 gt = gtr_frag<DH>(sG, lane, nb, qbk * 32 + ks2 * 16);
              accV[nb] = mfma32(gt, pp.v, accV[nb]);
              const bf16x8 qt = gtr_frag<DH>(sQ, lane, nb, qbk * 32 + ks2 * 16);
              accK[nb] = mfma32(qt, ps.v, accK[nb]);
            }
          }
        }
      }
      if (it + 1 < nit) lstore((it + 1) & 1);
      __syncthreads();
    }
  }
  if (wave_active && kkey < S) {
    bf16_t* kp = a.dk + (int64_t)b * a.bs_d + (int64_t)kkey * a.ld_d + hkv * DH;
    bf16_t* vp = a.dv + (int64_t)b * a.bs_d + (int64_t)kkey * a.ld_d + hkv * DH;
    const float sc_ = a.scale;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = nb * 32 + 8 * g + 4 * hi;
        *reinterpret_cast<uint2*>(kp + d0) = uint2{pack2_bf16(accK[nb][4 * g] * sc_, accK[nb][4 * g + 1] * sc_),
                                                   pack2_bf16(accK[nb][4 * g + 2] * sc_, accK[nb][4 * g + 3] * sc_)};
        *reinterpret_cast<uint2*>(vp + d0) = uint2{pack2_bf16(accV[nb][4 * g], accV[nb][4 * g + 1]),
                                                   pack2_bf16(accV[nb][4 * g + 2], accV[nb][4 * g + 3])};
      }
  }
}

inline size_t galign256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t attention_gqa_bwd_workspace_bytes(int nb, int S, int Hq) {
  if (nb <= 0 || S <= 0 || Hq <= 0) return 0;
  const size_t S_pad = ((size_t)S + 63) & ~(size_t)63;
  return 2 * galign256((size_t)nb * Hq * S_pad * 4);
}

int attention_gqa_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                      const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                      int64_t bs_d, int nb, int S, int Hq, int Hkv, int d, float scale, const int* kv_len, const float* lse_in,
                      int64_t lse_ld, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!q || !k || !v || !o || !dout || !dq || !dk || !dv || !workspace) return U2_ERR_ARG;
  if (d != 64 && d != 128) return U2_ERR_ARG;
  if (nb <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || !(scale > 0.f)) return U2_ERR_ARG;
  if ((int64_t)nb * Hq * ((S + 127) / 128) > 0x7fffffff) return U2_ERR_ARG;
  if ((ld_qkv & 7) || (bs_qkv & 7) || (ld_o & 7) || (bs_o & 7) || (ld_d & 3) || (bs_d & 3)) return U2_ERR_ARG;
  if (ld_qkv < (int64_t)Hq * d || ld_o < (int64_t)Hq * d || ld_d < (int64_t)Hq * d) return U2_ERR_ARG;
  if ((nb > 1 && (bs_qkv < (int64_t)S * ld_qkv || bs_o < (int64_t)S * ld_o || bs_d < (int64_t)S * ld_d))) return U2_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)dout) & 15) ||
      (((uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 7) || ((uintptr_t)workspace & 255) || ((uintptr_t)kv_len & 3))
    return U2_ERR_ARG;
  if (lse_in && (lse_ld < S || ((uintptr_t)lse_in & 3))) return U2_ERR_ARG;
  if (workspace_bytes < attention_gqa_bwd_workspace_bytes(nb, S, Hq)) return U2_ERR_WORKSPACE;
  const int S_pad = (S + 63) & ~63;
  char* w = static_cast<char*>(workspace);
  const size_t sb = galign256((size_t)nb * Hq * S_pad * 4);
  GqaBwdArgs a;
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.lse = reinterpret_cast<float*>(w);
  a.dsum = reinterpret_cast<float*>(w + sb);
  a.lse_in = lse_in; a.lse_ld = lse_ld; a.kv_len = kv_len;
  a.S = S; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.S_pad = S_pad;
  a.ld_qkv = ld_qkv; a.bs_qkv = bs_qkv; a.ld_o = ld_o; a.bs_o = bs_o; a.ld_d = ld_d; a.bs_d = bs_d;
  a.scale = scale;
  a.scale_log2e = scale * 1.44269504088896340736f;
  a.nblk = (S + 127) / 128;
  // (visible pairs of a causal head: ~S^2 / 2; the profile records the flops of the visible pairs)
  const double unit = 2.0 * (double)nb * Hq * (double)S * (S + 1) / 2.0 * d;
  const size_t tile = (size_t)64 * d * 2;
  {
    a.nwg = nb * Hq * a.nblk;
    ProfScope ps(PROF_FLASH, (lse_in ? 3.0 : 4.0) * unit, stream, (double)nb * S * Hq * d * 2.0 * 4.0);
#define U2_GDQ(D_, L_) hipLaunchKernelGGL((gqa_bwd_dq_kernel<D_, L_>), dim3((unsigned)a.nwg), dim3(256), 4 * tile, stream, a)
    if (d == 128) { if (lse_in) U2_GDQ(128, true); else U2_GDQ(128, false); }
    else { if (lse_in) U2_GDQ(64, true); else U2_GDQ(64, false); }
#undef U2_GDQ
  }
  int e = launch_status();
  if (e != U2_OK) return e;
  {
    a.nwg = nb * Hkv * a.nblk;
    ProfScope ps(PROF_FLASH, 4.0 * unit, stream, (double)nb * S * Hq * d * 2.0 * 4.0);
    const size_t smem = 4 * tile + 4 * 64 * sizeof(float);
    if (d == 128) hipLaunchKernelGGL(gqa_bwd_dkv_kernel<128>, dim3((unsigned)a.nwg), dim3(256), smem, stream, a);
    else hipLaunchKernelGGL(gqa_bwd_dkv_kernel<64>, dim3((unsigned)a.nwg), dim3(256), smem, stream, a);
  }
  return launch_status();
}

}  // namespace u2
