// Flash attention backward, one kernel pair for both attentions that train:
//   out = softmax(q k^T * scale [+ mask]) v   ->   dq, dk, dv   from q, k, v, out, d_out (+ optionally the forward's lse)
//   * the ViT blocks' d = 64 self-attention (MONAI SABlock, vit.py:100-105): equal heads, no mask
//     (CAUSAL = false);
//   * the decoder's causal grouped-query attention (training route of u2tokenizer_amd/decoder_train.py), d = 64 / 96 / 128
//     (CAUSAL = true; 96 -- Phi-3's head dim -- through u2tok_attention_gqa_bwd_d96),
// without the (S x S) probability / score-gradient tensors the unfused backward round-trips through HBM (ViT: 1.6 GB fp32 +
// 0.8 GB bf16, several times per layer at S = 2049).  Two kernels, no atomics, bit-repeatable:
//
//   bwd_dq_kernel    one workgroup per (batch, query head, 128 query rows), 4 waves x 32 queries, two sweeps over the keys:
//                    sweep 1 rebuilds the row statistics (lse = log2 sum exp2(s c), c = scale log2 e) -- skipped when the
//                    forward's are given (HAVE_LSE) -- and D = rowsum(d_out * out); sweep 2 computes  S^T = K Q^T,
//                    dP^T = V dO^T,  dS^T = P^T (dP^T - D)  and  dQ^T += K^T dS^T.  A lane owns one QUERY (column of the
//                    32x32 MFMA result) and 16 keys per block, so lse / D are lane scalars and dS^T feeds the next MFMA from
//                    the lane's own registers: its k slots carry the keys of a 16-group in the order
//                    [0-3, 8-11 | 4-7, 12-15] (lane halves), and the K^T fragment of the other operand is gathered in
//                    exactly that order from the row-major K tile by two ds_read_b64_tr_b16 (a 16-lane group reads a
//                    [4 keys][16 d] block; lane a supplies row a >> 2, piece a & 3, receives column a).
//   bwd_dkv_kernel   one workgroup per (batch, kv head, 128 keys), 4 waves x 32 keys, one sweep over the queries in the
//                    other orientation: S = Q K^T, dP = dO V^T with a lane owning one KEY and 16 queries per block;
//                    dV^T += dO^T P,  dK^T += Q^T dS  again from registers, the Q^T / dO^T fragments transpose-read from
//                    the same row-major Q / dO tiles that feed S and dP.  lse / D come from the first kernel through the
//                    workspace.
//
// Head dim DH = 64, 96 or 128: tiles of 64 rows x DH, DH / 16 k steps, DH / 32 accumulator blocks (d = 96: 192-byte rows with a
// tile placement of their own, tile_off<96>, two waves per SIMD without scratch; d = 128: the K, V fragments
// and the dK, dV accumulators are 192 registers -- the dK / dV kernel runs one wave per SIMD with the whole register file
// instead of spilling at two).
// The mask (CAUSAL): query i of sequence b sees key j iff j <= i and j < kv_len[b] (HF's causal mask built from a
// right-padded 2-D attention mask; kv_len NULL: plain causal).  Work outside the mask is skipped by whole 64-row tiles: the
// dQ kernel visits keys 0 .. min(last query of its block, kv_len - 1), the dK / dV kernel visits queries from its block's
// first key on; a dK / dV block whose keys all lie at or beyond kv_len writes zeros.  Without it every key below S is
// visible, every tile is visited and only the ragged last tile is masked; none of the mask arithmetic is compiled in.
// Grouped-query heads (built with CAUSAL only; without it the heads are equal, G = 1): the dQ kernel runs per QUERY head and
// reads kv head h / G; the dK / dV kernel runs per KV head and sums the contributions of its G query heads in one set of
// accumulators, heads in ascending order.
// Inputs and outputs are strided column views: q, k, v of one packed (rows, (Hq + 2 Hkv) d) buffer (or any other layout with
// a common leading dim), dq, dk, dv likewise -- the q|k|v product's backward reads one dense gradient.
//
// Cost: 8 matmul units of 2 S^2 d flop per head, over the visible pairs (the ViT's unfused form has 5 plus ~16 GB of HBM
// traffic per layer); HBM: q, k, v, out, d_out read, dq, dk, dv written, 2 x 4 bytes per (head, row) of statistics -- no
// transposed copies.
#include "kernels.h"

namespace u2 {

namespace {

struct Args {
  const bf16_t *q, *k, *v, *o, *dout;  // row-major views, head h at column h * DH
  bf16_t *dq, *dk, *dv;
  float *lse, *dsum;    // (nb * Hq, S_pad): row statistics handed from the dQ kernel to the dK / dV kernel
  const float* lse_in;  // optional row statistics of the forward kernel, (nb * Hq, lse_ld), log2 units
  const int* kv_len;    // optional (CAUSAL only): (nb) valid keys per sequence
  int64_t lse_ld;
  int S, Hq, Hkv, G, S_pad, nblk, nwg;  // nblk: 128-row blocks per (batch, head); nwg = nb * heads of the kernel * nblk
  int64_t ld_qkv, bs_qkv, ld_o, bs_o, ld_d, bs_d;
  float scale, scale_log2e;
};

// [64][DH] bf16 tiles, 16-byte chunks XOR-swizzled within each 128-byte half row with the BIT-REVERSED row pair index
// rev3((row >> 1) & 7).  Two access patterns share a tile: the 32 x 32 row fragments (ds_read_b128: 16 consecutive rows at
// one chunk -> any bijection of the 8 row pairs onto the 8 slots is conflict-free, as attn.hip's plain (row >> 1) & 7) and
// the transpose reads (4 consecutive rows x 4 consecutive chunks per half wave): rows r and r + 2 must land in different
// 64-byte groups, i.e. their XOR values must differ in bit 2 -- rev3(p) ^ rev3(p + 1) = 4 for even p.  With the plain swizzle
// the transpose reads were 2-way conflicts (15-20 % of the LDS cycles, profiles/r02_kernel_pmc.json).
template <int DH>
__device__ __forceinline__ uint32_t tile_off(int row, int chunk) {
  const int p = (row >> 1) & 7;
  const int x = ((p & 1) << 2) | (p & 2) | ((p >> 2) & 1);
  return (uint32_t)(row * (DH * 2) + (((chunk & ~7) | ((chunk & 7) ^ x)) << 4));
}
// DH = 96: rows of 192 bytes = 12 chunks, which the XOR over 8 chunks would send out of the row (chunks 8-11 ^ 4..7 -> 12-15).
// A 192-byte row starts 12 slots after its predecessor, so chunk c of row r sits in the 16-byte slot
// 4 ((c >> 2) - r mod 4) + (c & 3) of the 256-byte bank row: the group of four chunks picks the 64-byte quarter and rows r,
// r + 4, r + 8, r + 12 meet in one quarter.  XOR of the chunk's low two bits with (row >> 2) & 3 separates those four and stays
// inside the group of four chunks: the 16 rows of a ds_read_b128 lane group at one chunk cover the 16 slots (4 rows mod 4 x 4
// XOR values -- for 16 consecutive rows and for the hardware's groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} alike), and
// a transpose read's 4 aligned rows (one XOR value, four quarters) x 4 chunks of one group cover them too.  Both conflict-free.
template <>
__device__ __forceinline__ uint32_t tile_off<96>(int row, int chunk) {
  return (uint32_t)(row * 192 + ((chunk & ~3) << 4) + (((chunk & 3) ^ ((row >> 2) & 3)) << 4));
}

__device__ __forceinline__ float dot8(const uint4 a, const uint4 b) {
  float s = 0.f;
  s = __builtin_fmaf(bf16lo(a.x), bf16lo(b.x), s); s = __builtin_fmaf(bf16hi(a.x), bf16hi(b.x), s);
  s = __builtin_fmaf(bf16lo(a.y), bf16lo(b.y), s); s = __builtin_fmaf(bf16hi(a.y), bf16hi(b.y), s);
  s = __builtin_fmaf(bf16lo(a.z), bf16lo(b.z), s); s = __builtin_fmaf(bf16hi(a.z), bf16hi(b.z), s);
  s = __builtin_fmaf(bf16lo(a.w), bf16lo(b.w), s); s = __builtin_fmaf(bf16hi(a.w), bf16hi(b.w), s);
  return s;
}

// XCD-aware order (as attn.hip): workgroup w runs on XCD w % 8; every XCD gets a contiguous range of logical ids so that
// the blocks of one (batch, head) share that XCD's L2 copy of the operands they all stream (K, V, K^T resp. Q, dO, Q^T,
// dO^T): with the plain (block, head) grid every head was fetched by all eight L2s -- 0.93 GB of fabric-side reads per
// launch against 0.15 GB of operands (ViT shape, profiles/r02_kernel_pmc.json).
__device__ __forceinline__ int xcd_order(int w, int nwg) {
  const int qn = nwg >> 3, rn = nwg & 7;
  const int xcd = w & 7, idx = w >> 3;
  return (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + idx;
}

union Frag {
  bf16x8 v;
  uint4 q;
  uint32_t u[4];
};

typedef short v4s_t __attribute__((ext_vector_type(4)));

// A operand "X^T" (32 d rows x 16 k) of v_mfma_f32_32x32x16_bf16 from a row-major [64 rows][DH] tile (rows = keys or
// queries = the contraction index), in the k-slot order of an accumulator fed back as the B operand: lane
// (d = 32 nb + (lane & 31), hi = lane >> 5) needs rows r0 + 4 hi + {0..3} and r0 + 8 + 4 hi + {0..3} of column d.  Two
// transpose reads; r0 = 32 blk + 16 ks2 is a compile-time constant.
template <int DH>
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int lane, int nb, int r0) {
  typedef __attribute__((address_space(3))) v4s_t* lds_v4;
  const int a = lane & 15;
  const int chunk = 4 * nb + 2 * ((lane >> 4) & 1) + ((a & 3) >> 1), sub = (a & 1) * 8;
  const int row1 = r0 + 4 * (lane >> 5) + (a >> 2), row2 = row1 + 8;
  const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(tile + tile_off<DH>(row1, chunk) + sub));
  const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(tile + tile_off<DH>(row2, chunk) + sub));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// Staging of a [64][DH] tile, global -> registers (issued a tile ahead, under the MFMAs) -> LDS: the 256 threads carry
// DH / 32 pieces of 16 bytes each, piece i of thread tid = chunk (i * 256 + tid) % (DH / 8) of row (i * 256 + tid) / (DH / 8).
// Rows past the end re-read row S - 1; what they contribute is masked or never written.
// DH = 96 (12 chunks per row, 768 = 3 x 256 pieces): thread tid carries chunks (tid & 3) + {0, 4, 8} of row tid >> 2 -- one
// row, one global and one LDS address per thread with constant offsets between the pieces, where (i * 256 + tid) / 12 costs
// three of each (the registers that decided between two waves per SIMD and scratch in the dK / dV kernel).
// (Functions over array references, not lambdas capturing the arrays: with the lambdas the pieces went through scratch.)
template <int DH>
__device__ __forceinline__ void tile_load(bf16x8 (&r)[DH / 32], const bf16_t* base, int64_t ld, int row0, int S, int tid) {
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    if constexpr (DH == 96) {  // one row address per thread, the pieces 64 bytes apart
      r[i] = *reinterpret_cast<const bf16x8*>(base + (int64_t)min(row0 + (tid >> 2), S - 1) * ld + (4 * i + (tid & 3)) * 8);
    } else {
      const int cidx = i * 256 + tid;
      r[i] = *reinterpret_cast<const bf16x8*>(base + (int64_t)min(row0 + cidx / (DH / 8), S - 1) * ld + cidx % (DH / 8) * 8);
    }
  }
}
template <int DH>
__device__ __forceinline__ void tile_store(char* tile, const bf16x8 (&r)[DH / 32], int tid) {
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    if constexpr (DH == 96) {
      *reinterpret_cast<bf16x8*>(tile + tile_off<DH>(tid >> 2, 4 * i + (tid & 3))) = r[i];
    } else {
      const int cidx = i * 256 + tid;
      *reinterpret_cast<bf16x8*>(tile + tile_off<DH>(cidx / (DH / 8), cidx % (DH / 8))) = r[i];
    }
  }
}

// -inf into the scores of key tile t where the lane's query qi does not see the key: kk >= kvl, and with CAUSAL kk > qi.
// The lane owns keys t*64 + kbk*32 + (r&3) + 8*(r>>2) + 4*hi.  Without CAUSAL kvl = S: only the ragged last tile has any.
template <bool CAUSAL>
__device__ __forceinline__ void mask_keys(f32x16 (&sc)[2], int t, int hi, int qi, int wrow0, int kvl) {
  if ((CAUSAL && t * 64 + 63 > wrow0) || t * 64 + 64 > kvl) {  // wave-uniform
    const int kvb = t * 64 + 4 * hi;
#pragma unroll
    for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = kvb + kbk * 32 + (r & 3) + 8 * (r >> 2);
        if ((CAUSAL && kk > qi) || kk >= kvl) sc[kbk][r] = -INFINITY;  // p = 0
      }
  }
}

// ----------------------------------------------------------------------------------------------------------- dQ
template <int DH, bool CAUSAL, bool HAVE_LSE>  // HAVE_LSE: the forward kernel's row statistics are given, no sweep 1
__global__ __launch_bounds__(256, 2) void bwd_dq_kernel(const Args a) {
  constexpr int KS = DH / 16, NB = DH / 32, NLD = DH / 32, TILE = 64 * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char lds[];  // [stage][K | V] tiles
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int S = a.S, S_pad = a.S_pad;
  const int vid = xcd_order(blockIdx.x, a.nwg);
  const int bh = vid / a.nblk, b = bh / a.Hq, h = bh - b * a.Hq;
  // causal: the last query blocks of a head have the most keys -- hand those out first
  const int blk = CAUSAL ? a.nblk - 1 - (vid - bh * a.nblk) : vid - bh * a.nblk;
  const int hkv = CAUSAL ? h / a.G : h;
  const float c = a.scale_log2e;
  const int q0 = blk * 128;
  const int wrow0 = q0 + wv * 32;
  const bool wave_active = wrow0 < S;
  const int qi = wrow0 + l31;
  const int qrow = min(qi, S - 1);
  const int kvl = CAUSAL ? (a.kv_len ? max(1, min(a.kv_len[b], S)) : S) : S;  // keys at or beyond kvl are invisible
  const int64_t ld = a.ld_qkv;
  const bf16_t* kb_ = a.k + (int64_t)b * a.bs_qkv + hkv * DH;
  const bf16_t* vb_ = a.v + (int64_t)b * a.bs_qkv + hkv * DH;

  // Q / dO fragments (B operands: lane = query column, 8 d values per k16 step) and D = rowsum(dO * O)
  Frag qf[KS], dof[KS];
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
      dpart += dot8(ov, dof[ks].q);
    }
  }
  const float Dq = dpart + __shfl_xor(dpart, 32, 64);

  bf16x8 rk[NLD], rv[NLD];  // the next K / V tile on its way to LDS
  // keys visited: 0 .. min(last query of the block, kv_len - 1) with the mask, all of them without
  const int ntile = ((CAUSAL ? min(min(q0 + 128, S), kvl) : S) + 63) >> 6;

  float m_run = -INFINITY, l_run = 0.f;
  if constexpr (!HAVE_LSE) {
    // ---------------- sweep 1: lse (log2 units) of the lane's query row
    tile_load<DH>(rk, kb_, ld, 0, S, tid);
    tile_store<DH>(lds, rk, tid);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks].v), "+v"(dof[ks].v));  // loads done before the loops
    for (int t = 0; t < ntile; ++t) {
      if (t + 1 < ntile) tile_load<DH>(rk, kb_, ld, (t + 1) * 64, S, tid);
      if (wave_active) {
        const char* sK = lds + (t & 1) * 2 * TILE;
        f32x16 sc[2];
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[kbk][r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + tile_off<DH>(kbk * 32 + l31, ks * 2 + hi));
            sc[kbk] = mfma32(kf, qf[ks].v, sc[kbk]);
          }
        }
        mask_keys<CAUSAL>(sc, t, hi, qi, wrow0, kvl);
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx[r & 3] = fmaxf(mx[r & 3], sc[kbk][r]);
        float mt = fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3]));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * c;  // scale > 0
        const float m_new = fmaxf(m_run, mt);        // finite from tile 0 on: key 0 is visible to every query
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
          for (int r = 0; r < 16; ++r) ps[r & 3] += __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kbk][r], c, -m_new));
        l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + ((ps[0] + ps[1]) + (ps[2] + ps[3]));
        m_run = m_new;
      }
      if (t + 1 < ntile) tile_store<DH>(lds + ((t + 1) & 1) * 2 * TILE, rk, tid);
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
  if (wave_active && hi == 0 && qi < S) {  // for the dK / dV kernel
    a.lse[(int64_t)bh * S_pad + qi] = lse;
    a.dsum[(int64_t)bh * S_pad + qi] = Dq;
  }

  // ---------------- sweep 2: dQ^T
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
  tile_load<DH>(rk, kb_, ld, 0, S, tid);
  tile_load<DH>(rv, vb_, ld, 0, S, tid);
  tile_store<DH>(lds, rk, tid);
  tile_store<DH>(lds + TILE, rv, tid);
  __syncthreads();
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks].v), "+v"(dof[ks].v));  // loads done before the loop
  for (int t = 0; t < ntile; ++t) {
    if (t + 1 < ntile) {
      tile_load<DH>(rk, kb_, ld, (t + 1) * 64, S, tid);
      tile_load<DH>(rv, vb_, ld, (t + 1) * 64, S, tid);
    }
    if (wave_active && (!CAUSAL || t * 64 <= wrow0 + 31)) {  // (a tile wholly past this wave's diagonal contributes nothing)
      const char* sK = lds + (t & 1) * 2 * TILE;
      const char* sV = sK + TILE;
      f32x16 sc[2], dp[2];
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc[kbk][r] = 0.f; dp[kbk][r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + tile_off<DH>(kbk * 32 + l31, ks * 2 + hi));
          sc[kbk] = mfma32(kf, qf[ks].v, sc[kbk]);
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sV + tile_off<DH>(kbk * 32 + l31, ks * 2 + hi));
          dp[kbk] = mfma32(vf, dof[ks].v, dp[kbk]);
        }
      }
      mask_keys<CAUSAL>(sc, t, hi, qi, wrow0, kvl);
      // dS^T = P^T (dP^T - D), unscaled (the scale is applied once in the epilogue)
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kbk][r], c, -lse));
          sc[kbk][r] = p * (dp[kbk][r] - Dq);
        }
      // dQ^T += K^T dS^T: k-slots jj of step (kbk, ks2) carry keys kbk*32 + 16*ks2 + 8*(jj>>2) + 4*hi + (jj&3); the K^T
      // fragment is transpose-read from the row-major K tile in that order
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          Frag pf;
#pragma unroll
          for (int j = 0; j < 4; ++j) pf.u[j] = pack2_bf16(sc[kbk][ks2 * 8 + 2 * j], sc[kbk][ks2 * 8 + 2 * j + 1]);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const bf16x8 tf = tr_frag<DH>(sK, lane, nb, kbk * 32 + ks2 * 16);
            acc[nb] = mfma32(tf, pf.v, acc[nb]);
          }
        }
    }
    if (t + 1 < ntile) {
      tile_store<DH>(lds + ((t + 1) & 1) * 2 * TILE, rk, tid);
      tile_store<DH>(lds + ((t + 1) & 1) * 2 * TILE + TILE, rv, tid);
    }
    __syncthreads();
  }
  // lane: q = lane & 31, d = nb*32 + 8*g + 4*hi + e
  if (wave_active && qi < S) {
    bf16_t* op = a.dq + (int64_t)b * a.bs_d + (int64_t)qi * a.ld_d + h * DH;
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
// lse (threads 0-15) and D (16-31) of 4 queries each of the tile at q0, for stat[stage][lse | D][64]; queries past the end
// get lse = +inf, which makes their probabilities exactly 0
__device__ __forceinline__ void stat_load(float4& rs, const float* lse, const float* dsum, int q0, int S, int tid) {
  if (tid < 32) {
    const int qq = q0 + (tid & 15) * 4;
    rs = *reinterpret_cast<const float4*>((tid < 16 ? lse : dsum) + qq);
    const float fill = tid < 16 ? INFINITY : 0.f;
    if (qq + 0 >= S) rs.x = fill;
    if (qq + 1 >= S) rs.y = fill;
    if (qq + 2 >= S) rs.z = fill;
    if (qq + 3 >= S) rs.w = fill;
  }
}

template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256, DH >= 128 ? 1 : 2) void bwd_dkv_kernel(const Args a) {
  constexpr int KS = DH / 16, NB = DH / 32, NLD = DH / 32, TILE = 64 * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char lds[];  // [stage][Q | dO] tiles, then stat[stage][lse | D][64]
  float* const stat = reinterpret_cast<float*>(lds + 4 * TILE);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int S = a.S, S_pad = a.S_pad;
  const int vid = xcd_order(blockIdx.x, a.nwg);
  const int bh = vid / a.nblk, b = bh / a.Hkv, hkv = bh - b * a.Hkv;
  const int blk = vid - bh * a.nblk;  // (causal: the first key blocks see the most queries and come first)
  const float c = a.scale_log2e;
  const int k0 = blk * 128;
  const int wkey0 = k0 + wv * 32;
  const bool wave_active = wkey0 < S;
  const int kkey = wkey0 + l31;
  const int krow = min(kkey, S - 1);
  const int kvl = CAUSAL ? (a.kv_len ? max(1, min(a.kv_len[b], S)) : S) : S;
  const int64_t ld = a.ld_qkv;

  f32x16 accV[NB], accK[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accV[nb][r] = 0.f; accK[nb][r] = 0.f; }

  // query tiles t0 .. ntq - 1 of each of the G query heads, heads in ascending order: iteration it is
  // (head it / nt, tile t0 + it % nt).  Without the mask: every tile, and one head (so no division in that build).
  const int t0 = CAUSAL ? k0 >> 6 : 0, nt = ((S + 63) >> 6) - t0;
  const int nit = CAUSAL ? a.G * nt : nt;
  // (causal, keys all at or beyond kv_len: no query sees them, the gradients are 0)
  if (!CAUSAL || k0 < kvl) {
    // K / V fragments (B operands: lane = key column)
    Frag kf[KS], vf[KS];
    {
      const bf16_t* kp = a.k + (int64_t)b * a.bs_qkv + (int64_t)krow * ld + hkv * DH + hi * 8;
      const bf16_t* vp = a.v + (int64_t)b * a.bs_qkv + (int64_t)krow * ld + hkv * DH + hi * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        kf[ks].q = *reinterpret_cast<const uint4*>(kp + ks * 16);
        vf[ks].q = *reinterpret_cast<const uint4*>(vp + ks * 16);
      }
    }
    bf16x8 rq[NLD], rg[NLD];  // the next Q / dO tile and its statistics on their way to LDS
    float4 rs = {0.f, 0.f, 0.f, 0.f};
#define U2_DKV_GLOAD(it_)                                                                             \
  do {                                                                                                \
    const int h_ = CAUSAL ? hkv * a.G + (it_) / nt : hkv, q0_ = (t0 + (CAUSAL ? (it_) % nt : (it_))) * 64; \
    tile_load<DH>(rq, a.q + (int64_t)b * a.bs_qkv + h_ * DH, ld, q0_, S, tid);                        \
    tile_load<DH>(rg, a.dout + (int64_t)b * a.bs_o + h_ * DH, a.ld_o, q0_, S, tid);                   \
    const int64_t so_ = ((int64_t)b * a.Hq + h_) * S_pad;                                             \
    stat_load(rs, a.lse + so_, a.dsum + so_, q0_, S, tid);                                            \
  } while (0)
#define U2_DKV_LSTORE(st_)                                                                            \
  do {                                                                                                \
    tile_store<DH>(lds + (st_) * 2 * TILE, rq, tid);                                                  \
    tile_store<DH>(lds + (st_) * 2 * TILE + TILE, rg, tid);                                           \
    if (tid < 32) *reinterpret_cast<float4*>(stat + ((st_) * 2 + (tid >> 4)) * 64 + (tid & 15) * 4) = rs; \
  } while (0)
    U2_DKV_GLOAD(0);
    U2_DKV_LSTORE(0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(kf[ks].v), "+v"(vf[ks].v));
    for (int it = 0; it < nit; ++it) {
      const int st = it & 1;
      const int t = t0 + (CAUSAL ? it % nt : it);
      if (it + 1 < nit) U2_DKV_GLOAD(it + 1);
      // (causal: the queries of the tile all before this wave's keys, or its keys all beyond kv_len: nothing)
      if (wave_active && (!CAUSAL || (t * 64 + 63 >= wkey0 && wkey0 < kvl))) {
        const char* sQ = lds + st * 2 * TILE;
        const char* sG = sQ + TILE;
        const float* sl = stat + st * 2 * 64;
        const bool need_mask = CAUSAL && (t * 64 < wkey0 + 32 || kvl < wkey0 + 32);  // wave-uniform
#pragma unroll
        for (int qbk = 0; qbk < 2; ++qbk) {
          // S = Q K^T, dP = dO V^T: lane = key column, rows = queries qbk*32 + (r&3) + 8*(r>>2) + 4*hi
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 qa = *reinterpret_cast<const bf16x8*>(sQ + tile_off<DH>(qbk * 32 + l31, ks * 2 + hi));
            s = mfma32(qa, kf[ks].v, s);
            const bf16x8 ga = *reinterpret_cast<const bf16x8*>(sG + tile_off<DH>(qbk * 32 + l31, ks * 2 + hi));
            dp = mfma32(ga, vf[ks].v, dp);
          }
          if (need_mask) {  // (keys past S need none: their columns are never written)
            const int qb = t * 64 + qbk * 32 + 4 * hi;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int qq = qb + (r & 3) + 8 * (r >> 2);
              if (kkey > qq || kkey >= kvl) s[r] = -INFINITY;
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
          // dV^T += dO^T P, dK^T += Q^T dS: k-slots jj of step ks2 carry queries qbk*32 + 16*ks2 + 8*(jj>>2) + 4*hi + (jj&3);
          // the dO^T / Q^T fragments are transpose-read from the row-major tiles in that order
#pragma unroll
          for (int ks2 = 0; ks2 < 2; ++ks2) {
            Frag pp, ps;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              pp.u[j] = pack2_bf16(s[ks2 * 8 + 2 * j], s[ks2 * 8 + 2 * j + 1]);
              ps.u[j] = pack2_bf16(dp[ks2 * 8 + 2 * j], dp[ks2 * 8 + 2 * j + 1]);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
              const bf16x8 gt = tr_frag<DH>(sG, lane, nb, qbk * 32 + ks2 * 16);
              accV[nb] = mfma32(gt, pp.v, accV[nb]);
              const bf16x8 qt = tr_frag<DH>(sQ, lane, nb, qbk * 32 + ks2 * 16);
              accK[nb] = mfma32(qt, ps.v, accK[nb]);
            }
          }
        }
      }
      if (it + 1 < nit) U2_DKV_LSTORE((it + 1) & 1);
      __syncthreads();
    }
#undef U2_DKV_GLOAD
#undef U2_DKV_LSTORE
  }
  // lane: key = lane & 31, d = nb*32 + 8*g + 4*hi + e
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

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t workspace_bytes(int nb, int S, int Hq) {
  if (nb <= 0 || S <= 0 || Hq <= 0) return 0;
  const size_t S_pad = ((size_t)S + 63) & ~(size_t)63;
  return 2 * align256((size_t)nb * Hq * S_pad * 4);
}

template <int DH, bool CAUSAL>
void launch_pair(Args& a, int nb, bool have_lse, double unit, double row_bytes, hipStream_t stream, int* status) {
  constexpr size_t tiles = 4 * (size_t)64 * DH * 2;
  {
    a.nwg = nb * a.Hq * a.nblk;
    // (bytes: the ViT's count q, k, v, o, dO, dq resp. those and dk, dv whole; the decoder's count the query-head side only)
    ProfScope ps(PROF_FLASH, (have_lse ? 3.0 : 4.0) * unit, stream, row_bytes * (CAUSAL ? 4.0 : 6.0));
    if (have_lse) hipLaunchKernelGGL((bwd_dq_kernel<DH, CAUSAL, true>), dim3((unsigned)a.nwg), dim3(256), tiles, stream, a);
    else hipLaunchKernelGGL((bwd_dq_kernel<DH, CAUSAL, false>), dim3((unsigned)a.nwg), dim3(256), tiles, stream, a);
  }
  *status = launch_status();
  if (*status != U2_OK) return;
  {
    a.nwg = nb * a.Hkv * a.nblk;
    ProfScope ps(PROF_FLASH, 4.0 * unit, stream, row_bytes * (CAUSAL ? 4.0 : 8.0));
    hipLaunchKernelGGL((bwd_dkv_kernel<DH, CAUSAL>), dim3((unsigned)a.nwg), dim3(256), tiles + 4 * 64 * sizeof(float), stream, a);
  }
  *status = launch_status();
}

// The one launcher: validates what both entry points require, splits the workspace, fills Args, picks the instantiation.
// causal = false is built for d = 64 and equal heads only (the ViT); causal: d = 64 / 96 / 128 (96 through its own entry point).
int attention_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                  const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d, int64_t bs_d,
                  int nb, int S, int Hq, int Hkv, int d, float scale, bool causal, const int* kv_len, const float* lse_in,
                  int64_t lse_ld, void* workspace, size_t ws_bytes, hipStream_t stream) {
  if (!q || !k || !v || !o || !dout || !dq || !dk || !dv || !workspace) return U2_ERR_ARG;
  if (d != 64 && ((d != 96 && d != 128) || !causal)) return U2_ERR_ARG;
  if (nb <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || (!causal && Hq != Hkv) || !(scale > 0.f)) return U2_ERR_ARG;
  if ((int64_t)nb * Hq * ((S + 127) / 128) > 0x7fffffff) return U2_ERR_ARG;
  if ((ld_qkv & 7) || (bs_qkv & 7) || (ld_o & 7) || (bs_o & 7) || (ld_d & 3) || (bs_d & 3)) return U2_ERR_ARG;
  if (ld_qkv < (int64_t)Hq * d || ld_o < (int64_t)Hq * d || ld_d < (int64_t)Hq * d) return U2_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)dout) & 15) ||
      (((uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 7) || ((uintptr_t)workspace & 255) || ((uintptr_t)kv_len & 3))
    return U2_ERR_ARG;
  if (lse_in && (lse_ld < S || ((uintptr_t)lse_in & 3))) return U2_ERR_ARG;
  if (ws_bytes < workspace_bytes(nb, S, Hq)) return U2_ERR_WORKSPACE;
  const int S_pad = (S + 63) & ~63;
  char* w = static_cast<char*>(workspace);
  Args a;
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.lse = reinterpret_cast<float*>(w);
  a.dsum = reinterpret_cast<float*>(w + align256((size_t)nb * Hq * S_pad * 4));
  a.lse_in = lse_in; a.lse_ld = lse_ld; a.kv_len = kv_len;
  a.S = S; a.Hq = Hq; a.Hkv = Hkv; a.G = Hq / Hkv; a.S_pad = S_pad;
  a.ld_qkv = ld_qkv; a.bs_qkv = bs_qkv; a.ld_o = ld_o; a.bs_o = bs_o; a.ld_d = ld_d; a.bs_d = bs_d;
  a.scale = scale;
  a.scale_log2e = scale * 1.44269504088896340736f;
  a.nblk = (S + 127) / 128;
  a.nwg = 0;
  // the profile records the flops of the visible pairs: all S^2 of a head without the mask, ~S^2 / 2 with it
  const double pairs = causal ? (double)S * (S + 1) / 2.0 : (double)S * S;
  const double unit = 2.0 * (double)nb * Hq * pairs * d, row_bytes = (double)nb * S * Hq * d * 2.0;
  int e = U2_OK;
  if (!causal) launch_pair<64, false>(a, nb, lse_in != nullptr, unit, row_bytes, stream, &e);
  else if (d == 64) launch_pair<64, true>(a, nb, lse_in != nullptr, unit, row_bytes, stream, &e);
  else if (d == 96) launch_pair<96, true>(a, nb, lse_in != nullptr, unit, row_bytes, stream, &e);
  else launch_pair<128, true>(a, nb, lse_in != nullptr, unit, row_bytes, stream, &e);
  return e;
}

}  // namespace

size_t flash_attention_d64_bwd_workspace_bytes(int nb, int S, int H) { return workspace_bytes(nb, S, H); }

int flash_attention_d64_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                            const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                            int64_t bs_d, int nb, int S, int H, float scale, const float* lse_in, int64_t lse_ld,
                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if ((int64_t)nb * H > 65535) return U2_ERR_ARG;
  return attention_bwd(q, k, v, ld_qkv, bs_qkv, o, dout, ld_o, bs_o, dq, dk, dv, ld_d, bs_d, nb, S, H, H, 64, scale, false, nullptr,
                       lse_in, lse_ld, workspace, workspace_bytes, stream);
}

size_t attention_gqa_bwd_workspace_bytes(int nb, int S, int Hq) { return workspace_bytes(nb, S, Hq); }

int attention_gqa_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                      const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                      int64_t bs_d, int nb, int S, int Hq, int Hkv, int d, float scale, const int* kv_len, const float* lse_in,
                      int64_t lse_ld, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  // (the batches of one view must not overlap; the ViT's entry point never asked)
  if (nb > 1 && (bs_qkv < (int64_t)S * ld_qkv || bs_o < (int64_t)S * ld_o || bs_d < (int64_t)S * ld_d)) return U2_ERR_ARG;
  if (d != 64 && d != 128) return U2_ERR_ARG;  // (head dim 96 has its own entry point below)
  return attention_bwd(q, k, v, ld_qkv, bs_qkv, o, dout, ld_o, bs_o, dq, dk, dv, ld_d, bs_d, nb, S, Hq, Hkv, d, scale, true, kv_len,
                       lse_in, lse_ld, workspace, workspace_bytes, stream);
}

int attention_gqa_bwd_d96(const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld_qkv, int64_t bs_qkv, const bf16_t* o,
                          const bf16_t* dout, int64_t ld_o, int64_t bs_o, bf16_t* dq, bf16_t* dk, bf16_t* dv, int64_t ld_d,
                          int64_t bs_d, int nb, int S, int Hq, int Hkv, float scale, const int* kv_len, const float* lse_in,
                          int64_t lse_ld, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (nb > 1 && (bs_qkv < (int64_t)S * ld_qkv || bs_o < (int64_t)S * ld_o || bs_d < (int64_t)S * ld_d)) return U2_ERR_ARG;
  return attention_bwd(q, k, v, ld_qkv, bs_qkv, o, dout, ld_o, bs_o, dq, dk, dv, ld_d, bs_d, nb, S, Hq, Hkv, 96, scale, true, kv_len,
                       lse_in, lse_ld, workspace, workspace_bytes, stream);
}

}  // namespace u2
