// bf16 MFMA GEMM for gfx950:  C[z][m][n] = epilogue( alpha * sum_k A[z][m][k] * B[z][n][k] )
//
// Both operands are K-contiguous ("NT" form): A is an activation matrix [M][K], B is a weight in
// nn.Linear layout [N][K] (or K/V^T/... for the attention products).  This is the workhorse of the
// hot path: every nn.Linear of the ViT blocks (reference vit.py:100-105 via MONAI SABlock/MLPBlock),
// the SPP MLP (spatial_pooling_projector.py:22-28), every wq/wk/wv/dense of the tokenizer
// (rma.py:13-16, tta.py:16-19), the DiffTS score/aggregation products (svr.py:105-115) and the
// QK^T / PV products of the tokenizer attention (rma.py:61,73; tta.py:56,59).
//
// Design (CDNA4):
//  * 256 threads = 4 wave64 in a 2x2 arrangement; block tile BMxBNx64, wave tile (BM/2)x(BN/2) built
//    from v_mfma_f32_16x16x32_bf16.  The MFMA is issued with the WEIGHT fragment as the A operand and
//    the ACTIVATION fragment as the B operand, so a lane ends up holding 4 consecutive output columns
//    n of one output row m -> 8-byte bf16 / 16-byte fp32 stores and vector bias/residual loads.
//  * LDS tile = [rows][64 bf16] (128 B per row), 16-byte chunks XOR-swizzled with (row & 7) so the
//    ds_read_b128 fragment reads of a 16-lane group touch 16 distinct 16-B slots (conflict-free).
//  * Two LDS stages; global->LDS by LDS-DMA (global_load_lds_dwordx4, swizzle applied on the per-lane
//    SOURCE address because the DMA destination is lane-linear), issued as one burst ahead of the MFMAs
//    of the current K tile.  (Register staging, DMA pieces spread between the MFMAs and 64-byte rows
//    (BK = 32) were measured 10-25 % slower in round 1 -- profiles/r01_gemm_pp_study.log -- and removed.)
//  * XCD-aware, M-grouped tile order so that the 8 private L2s each see a compact band of tiles.
#include <type_traits>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include "kernels.h"
#include "rows.h"

namespace u2 {

__device__ uint4 g_zero16;  // zero-initialised; K-tail chunks of the LDS-DMA path read from here

// LDS chunk swizzle: XOR value for the 16-byte chunk index of `row` (128-B rows, 8 chunks): row & 7.
template <int BK>
__device__ __forceinline__ int lds_swz(int row) {
  static_assert(BK == 64, "BK");
  return row & 7;
}

// K-major operands (TA / TB; the weight-gradient and input-gradient products of the training path, whose operands would
// otherwise be transposed in HBM first): the operand is stored [K][rows] (row index = k, the M resp. N index contiguous).
// Its LDS tile is [64 k][BX] with 16-byte chunks (8 consecutive m) rotated inside the k row by kmaj_rot(k), and the MFMA
// fragment (8 consecutive k of one m) is gathered by two ds_read_b64_tr_b16: a 16-lane group reads a [4 k][16 m] block --
// lane a supplies the address of row a >> 2, 8-byte piece a & 3 and receives column a of the four rows
// (tools/ubench/tr_read.hip prints the instruction's mapping) -- so a lane ends up with k = 8 (lane >> 4) + {0..7} of column
// lane & 15, the same k-slot order as a K-contiguous fragment (the two forms mix freely as A and B).
// The rotation keeps the 16 chunks that the two 16-lane groups of a half wave touch (rows k..k+3 and k+8..k+11, two chunks
// each) in 16 different 16-byte slots of the 256-byte bank row.
template <int CPRX>  // chunks per k row: 16 (128-wide tile) or 8 (64-wide tile, two k rows per bank row)
__device__ __forceinline__ int kmaj_rot(int k) {
  if constexpr (CPRX == 16) return 2 * (k & 3) + 8 * ((k >> 3) & 1);
  else return 2 * ((k >> 1) & 1) + 4 * ((k >> 3) & 1);
}

typedef short v4s_t __attribute__((ext_vector_type(4)));

template <int BM, int BN, bool TA = false, bool TB = false>
__global__ __launch_bounds__(256, 2) void gemm_bf16_nt_kernel(GemmDesc d) {
  constexpr int BK = 64;
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int MI = WM / 16, NI = WN / 16;
  constexpr int CPR = BK / 8;                              // 16-B chunks per tile row
  constexpr int ROWB = BK * 2;                             // bytes per tile row
  constexpr int CA = BM * CPR / 256, CB = BN * CPR / 256;  // 16-B chunks per thread per tile
  constexpr int KSTEPS = BK / 32;
  constexpr int STAGE = (BM + BN) * ROWB;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- tile order: XCD-contiguous bands, then groups of 8 m-tiles ----
  const int ntiles = d.tiles_m * d.tiles_n;
  int pid = blockIdx.x;
  {
    const int q = ntiles >> 3, r = ntiles & 7;
    const int xcd = pid & 7, idx = pid >> 3;
    pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  constexpr int GROUP_M = 8;
  const int per_group = GROUP_M * d.tiles_n;
  const int group = pid / per_group;
  const int first_m = group * GROUP_M;
  const int gsz = min(d.tiles_m - first_m, GROUP_M);
  const int tm = first_m + (pid % per_group) % gsz;
  const int tn = (pid % per_group) / gsz;
  const int bm0 = tm * BM, bn0 = tn * BN;

  const int z = blockIdx.y;
  const int zb = z / d.nbh, zh = z - zb * d.nbh;
  const bf16_t* __restrict__ A = d.A + zb * d.sAb + zh * d.sAh;
  const bf16_t* __restrict__ B = d.B + zb * d.sBb + zh * d.sBh;

  // ---- per-thread global source pointers (row clamped, swizzled chunk folded in) ----
  // K-contiguous operand: chunk c of the tile = (row c / 8, k chunk c % 8); K-major operand: (k row c / CPRX, slot c % CPRX)
  // holding the 8 columns  ((slot - rot(k)) mod CPRX) * 8.  ka / kb: k offset inside a K tile (tail mask); oka / okb: the
  // chunk exists at all (columns past M / N of a K-major operand read the zero chunk).
  constexpr int CPRA = BM / 8, CPRB = BN / 8;
  const bf16_t* pa[CA];
  const bf16_t* pb[CB];
  int ka[CA], kb[CB];
  bool oka[CA], okb[CB];
  // MUBUF form (d.mubuf; round 6): byte offsets from this batch entry's operand base, one raw descriptor per operand, the K advance in the
  // scalar offset.  (Beside waves that issue MFMAs -- here: the other workgroup of the CU -- the FLAT-encoded global_load_lds stages a
  // third of what buffer_load ... lds does: tools/ubench/stage_bw.hip, profiles/r06_stage_bw.log.)  A chunk that does not exist (K tail,
  // columns past M / N of a K-major operand) takes the lane offset 2^31: past num_records whichever way the range check reads it -> zeros.
  int va[CA], vb[CB];
  const bool mubuf = d.mubuf != 0;
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int c = i * 256 + tid;
    if constexpr (TA) {
      const int krow = c / CPRA, cc = ((c % CPRA) - kmaj_rot<CPRA>(krow)) & (CPRA - 1);
      ka[i] = krow;
      oka[i] = bm0 + cc * 8 < d.M;
      pa[i] = A + (int64_t)krow * d.lda + bm0 + cc * 8;
    } else {
      const int row = c / CPR, gc = (c % CPR) ^ lds_swz<BK>(row);
      const int grow = min(bm0 + row, d.M - 1);
      ka[i] = gc * 8;
      oka[i] = true;
      pa[i] = A + (int64_t)grow * d.lda + gc * 8;
    }
    va[i] = (int)((pa[i] - A) * 2);
  }
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    const int c = i * 256 + tid;
    if constexpr (TB) {
      const int krow = c / CPRB, cc = ((c % CPRB) - kmaj_rot<CPRB>(krow)) & (CPRB - 1);
      kb[i] = krow;
      okb[i] = bn0 + cc * 8 < d.N;
      pb[i] = B + (int64_t)krow * d.ldb + bn0 + cc * 8;
    } else {
      const int row = c / CPR, gc = (c % CPR) ^ lds_swz<BK>(row);
      const int grow = min(bn0 + row, d.N - 1);
      kb[i] = gc * 8;
      okb[i] = true;
      pb[i] = B + (int64_t)grow * d.ldb + gc * 8;
    }
    vb[i] = (int)((pb[i] - B) * 2);
  }

  f32x4 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets: row = base + (lane & 15) with bases multiples of 16, so swz(row) == swz(lane & 15)
  const int frow = (lane & 15) * ROWB;
  int foff[KSTEPS];
#pragma unroll
  for (int kk = 0; kk < KSTEPS; ++kk) foff[kk] = (((kk * 4 + (lane >> 4)) ^ lds_swz<BK>(lane & 15)) << 4);
  // K-major fragments: lane a = lane & 15 of its 16-lane group addresses k row 8 (lane >> 4) + (a >> 2) (+ 4 for the second
  // read, + 32 per k step), 8-byte piece a & 3 of the fragment's two chunks; rot() of that row does not depend on the +4 /
  // +32, so the per-lane part is one offset per fragment.
  int fta[TA ? MI : 1], ftb[TB ? NI : 1];
  {
    const int a = lane & 15, krow = 8 * (lane >> 4) + (a >> 2);
    if constexpr (TA) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int cc = (wm * WM + mi * 16) / 8 + ((a & 3) >> 1);
        fta[mi] = (krow * CPRA + ((cc + kmaj_rot<CPRA>(krow)) & (CPRA - 1))) * 16 + (a & 1) * 8;
      }
    }
    if constexpr (TB) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int cc = (wn * WN + ni * 16) / 8 + ((a & 3) >> 1);
        ftb[ni] = (krow * CPRB + ((cc + kmaj_rot<CPRB>(krow)) & (CPRB - 1))) * 16 + (a & 1) * 8;
      }
    }
  }

  // elements between consecutive K tiles of a B row: BK for row-major weights, N * BK for "K-tile-major" packed ones
  // ([K / 64][N][64]: the 64 x 64 tile a workgroup stages per K step is one contiguous 8 KB block); K-major: BK rows
  [[maybe_unused]] const int64_t kadv_a = BK * d.lda;
  const int64_t kadv_b = TB ? BK * d.ldb : (d.ldbk ? d.ldbk : BK);
  const int nkt_all = (d.K + BK - 1) / BK;
  const int kt0 = (d.ksplit > 1) ? (int)blockIdx.z * d.kt_per : 0;   // split-K: this slice's K tiles
  const int nkt = (d.ksplit > 1) ? min(nkt_all, kt0 + d.kt_per) : nkt_all;
  auto dma = [&](int kt, int buf) {
    const int k0 = kt * BK;
    char* s = lds + buf * STAGE;
    if (mubuf) {
      const int sa = (int)((TA ? (int64_t)kt * kadv_a : (int64_t)k0) * 2), sb = (int)((int64_t)kt * kadv_b * 2);
#pragma unroll
      for (int i = 0; i < CA; ++i) {
        const bool ok = (TA ? oka[i] : true) && k0 + ka[i] < d.K;
        lds_dma_mubuf16(A, s + (i * 256 + wave * 64) * 16, ok ? va[i] : (int)0x80000000, sa);
      }
#pragma unroll
      for (int i = 0; i < CB; ++i) {
        const bool ok = (TB ? okb[i] : true) && k0 + kb[i] < d.K;
        lds_dma_mubuf16(B, s + BM * ROWB + (i * 256 + wave * 64) * 16, ok ? vb[i] : (int)0x80000000, sb);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const void* src;
      if constexpr (TA) src = (oka[i] && k0 + ka[i] < d.K) ? (const void*)(pa[i] + (int64_t)kt * kadv_a) : (const void*)&g_zero16;
      else src = (k0 + ka[i] < d.K) ? (const void*)(pa[i] + k0) : (const void*)&g_zero16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(s + (i * 256 + wave * 64) * 16),
                                       16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      const void* src;
      if constexpr (TB) src = (okb[i] && k0 + kb[i] < d.K) ? (const void*)(pb[i] + (int64_t)kt * kadv_b) : (const void*)&g_zero16;
      else src = (k0 + kb[i] < d.K) ? (const void*)(pb[i] + (int64_t)kt * kadv_b) : (const void*)&g_zero16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(s + BM * ROWB + (i * 256 + wave * 64) * 16),
                                       16, 0, 0);
    }
  };
  auto compute = [&](int buf) {
    const char* tA = lds + buf * STAGE;                    // A tile base ([BM][64] or [64][BM])
    const char* tB = lds + buf * STAGE + BM * ROWB;        // B tile base (both forms are (BM resp. BN) * 128 bytes)
    const char* sA = tA + (wm * WM) * ROWB + frow;
    const char* sB = tB + (wn * WN) * ROWB + frow;
    typedef __attribute__((address_space(3))) v4s_t* lds_v4;
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      bf16x8 xf[MI], wf[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        if constexpr (TA) {
          const char* q = tA + fta[mi] + kk * (32 * CPRA * 16);
          const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)q);
          const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(q + 4 * CPRA * 16));
          xf[mi] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        } else {
          xf[mi] = *reinterpret_cast<const bf16x8*>(sA + mi * 16 * ROWB + foff[kk]);
        }
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        if constexpr (TB) {
          const char* q = tB + ftb[ni] + kk * (32 * CPRB * 16);
          const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)q);
          const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(q + 4 * CPRB * 16));
          wf[ni] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        } else {
          wf[ni] = *reinterpret_cast<const bf16x8*>(sB + ni * 16 * ROWB + foff[kk]);
        }
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = mfma16(wf[ni], xf[mi], acc[mi][ni]);
    }
  };

  dma(kt0, kt0 & 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = kt0; kt < nkt; ++kt) {
    if (kt + 1 < nkt) dma(kt + 1, (kt + 1) & 1);
    compute(kt & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: lane holds C[m][n0..n0+3], m = tile row (lane & 15), n0 = 4 * (lane >> 4) ----
  if (d.ksplit > 1) {  // split-K slice: raw fp32 sums, the reduce kernel does the rest
    float* P = d.partial + ((int64_t)blockIdx.z * d.nz + z) * (int64_t)d.M * d.N;
    const int m_b = bm0 + wm * WM + (lane & 15), n_b = bn0 + wn * WN + (lane >> 4) * 4;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int m = m_b + mi * 16;
      if (m >= d.M) continue;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int n0 = n_b + ni * 16;
        float* pp = P + (int64_t)m * d.N + n0;
        if (n0 + 3 < d.N && (d.N & 3) == 0) {
          *reinterpret_cast<float4*>(pp) = float4{acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]};
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n0 + r < d.N) pp[r] = acc[mi][ni][r];
        }
      }
    }
    return;
  }
  const bool out_f32 = d.flags & GEMM_OUT_F32;
  char* Cz = reinterpret_cast<char*>(d.C) + (zb * d.sCb + zh * d.sCh) * (out_f32 ? 4 : 2);
  const bf16_t* Rz = (d.flags & GEMM_RESIDUAL) ? d.R + zb * d.sRb + zh * d.sRh : nullptr;
  const int m_base = bm0 + wm * WM + (lane & 15);
  const int n_base = bn0 + wn * WN + (lane >> 4) * 4;

  // Fast path: every column group of this block is inside N and all vector accesses are legal.  The flag set is
  // resolved ONCE into compile-time booleans (the common combinations), so the unrolled body is branch-free.
  auto epi_vec = [&](auto BN_, auto GELU_, auto RES_, auto F32_) {
    float4 bn[NI];
    if constexpr (decltype(BN_)::value) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const uint2 b2 = *reinterpret_cast<const uint2*>(d.bias + n_base + ni * 16);
        bn[ni] = float4{bf16lo(b2.x), bf16hi(b2.x), bf16lo(b2.y), bf16hi(b2.y)};
      }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int m = m_base + mi * 16;
      if (m >= d.M) continue;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int n0 = n_base + ni * 16;
        const float al = n0 < d.nsplit ? d.alpha_lo : d.alpha;
        float v0 = acc[mi][ni][0] * al, v1 = acc[mi][ni][1] * al, v2 = acc[mi][ni][2] * al, v3 = acc[mi][ni][3] * al;
        if constexpr (decltype(BN_)::value) { v0 += bn[ni].x; v1 += bn[ni].y; v2 += bn[ni].z; v3 += bn[ni].w; }
        if constexpr (decltype(GELU_)::value) { gelu_epi2(v0, v1); gelu_epi2(v2, v3); }
        if constexpr (decltype(RES_)::value) {
          const uint2 r2 = *reinterpret_cast<const uint2*>(Rz + (int64_t)m * d.ldr + n0);
          v0 += bf16lo(r2.x); v1 += bf16hi(r2.x); v2 += bf16lo(r2.y); v3 += bf16hi(r2.y);
        }
        if constexpr (decltype(F32_)::value)
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(Cz) + (int64_t)m * d.ldc + n0) = float4{v0, v1, v2, v3};
        else
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(Cz) + (int64_t)m * d.ldc + n0) =
              uint2{pack2_bf16(v0, v1), pack2_bf16(v2, v3)};
      }
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  const int ef = d.flags & (GEMM_BIAS_N | GEMM_BIAS_M | GEMM_GELU | GEMM_RESIDUAL | GEMM_OUT_F32);
  if ((d.flags & GEMM_VEC_OK) && bn0 + BN <= d.N && !(ef & GEMM_BIAS_M)) {
    switch (ef) {
      case 0: epi_vec(F_{}, F_{}, F_{}, F_{}); return;
      case GEMM_OUT_F32: epi_vec(F_{}, F_{}, F_{}, T_{}); return;
      case GEMM_BIAS_N: epi_vec(T_{}, F_{}, F_{}, F_{}); return;
      case GEMM_BIAS_N | GEMM_GELU: epi_vec(T_{}, T_{}, F_{}, F_{}); return;
      case GEMM_BIAS_N | GEMM_RESIDUAL: epi_vec(T_{}, F_{}, T_{}, F_{}); return;
      case GEMM_RESIDUAL: epi_vec(F_{}, F_{}, T_{}, F_{}); return;
      default: break;
    }
  }
  // Generic path (tails, unaligned, bias along M, rare flag sets): scalar, fully predicated.  The loops must stay
  // fully unrolled: a runtime index into acc[][] would move the accumulators to scratch memory.
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m_base + mi * 16;
    if (m >= d.M) continue;
    const float bm_v = (d.flags & GEMM_BIAS_M) ? bf16_to_f32(d.bias[m]) : 0.f;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n_base + ni * 16 + r;
        if (n >= d.N) break;
        float x = acc[mi][ni][r] * (n < d.nsplit ? d.alpha_lo : d.alpha) + bm_v;
        if (d.flags & GEMM_BIAS_N) x += bf16_to_f32(d.bias[n]);
        if (d.flags & GEMM_GELU) x = gelu_epi(x);
        if (Rz) x += bf16_to_f32(Rz[(int64_t)m * d.ldr + n]);
        if (out_f32) reinterpret_cast<float*>(Cz)[(int64_t)m * d.ldc + n] = x;
        else reinterpret_cast<bf16_t*>(Cz)[(int64_t)m * d.ldc + n] = f32_to_bf16(x);
      }
    }
  }
}

// out[z][m][n] = epilogue(alpha * sum_s partial[s][z][m][n]); one thread per 4 consecutive n
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(GemmDesc d) {
  const int64_t n4 = (d.N + 3) >> 2;
  const int64_t total = (int64_t)d.nz * d.M * n4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int n0 = (int)(idx % n4) * 4;
  const int64_t zm = idx / n4;
  const int m = (int)(zm % d.M), z = (int)(zm / d.M);
  const int64_t slice = (int64_t)d.nz * d.M * d.N;
  const float* P = d.partial + ((int64_t)z * d.M + m) * d.N + n0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const bool full = (n0 + 3 < d.N) && (d.N & 3) == 0;
  for (int s = 0; s < d.ksplit; ++s) {
    if (full) {
      const float4 t = *reinterpret_cast<const float4*>(P + s * slice);
      v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
    } else {
      for (int r = 0; r < 4; ++r)
        if (n0 + r < d.N) v[r] += P[s * slice + r];
    }
  }
  const int zb = z / d.nbh, zh = z - zb * d.nbh;
  const bool out_f32 = d.flags & GEMM_OUT_F32;
  const float bm_v = (d.flags & GEMM_BIAS_M) ? bf16_to_f32(d.bias[m]) : 0.f;
  const bf16_t* Rz = (d.flags & GEMM_RESIDUAL) ? d.R + zb * d.sRb + zh * d.sRh + (int64_t)m * d.ldr : nullptr;
  char* Cz = reinterpret_cast<char*>(d.C) + (zb * d.sCb + zh * d.sCh + (int64_t)m * d.ldc) * (out_f32 ? 4 : 2);
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + r;
    if (n >= d.N) break;
    float x = v[r] * (n < d.nsplit ? d.alpha_lo : d.alpha) + bm_v;
    if (d.flags & GEMM_BIAS_N) x += bf16_to_f32(d.bias[n]);
    if (d.flags & GEMM_GELU) x = gelu_epi(x);
    if (Rz) x += bf16_to_f32(Rz[n]);
    if (out_f32) reinterpret_cast<float*>(Cz)[n] = x;
    else reinterpret_cast<bf16_t*>(Cz)[n] = f32_to_bf16(x);
  }
}

// One step of a plan (gemm_plan.hip) on the rows it covers; `partial`: the stream's scratch.
static int gemm_step(const GemmDesc& d, const GemmStep& s, void* partial, hipStream_t stream) {
  GemmDesc g = d;
  g.A = d.A + (int64_t)s.row0 * d.lda;
  g.C = reinterpret_cast<char*>(d.C) + (int64_t)s.row0 * d.ldc * ((d.flags & GEMM_OUT_F32) ? 4 : 2);
  if (d.flags & GEMM_RESIDUAL) g.R = d.R + (int64_t)s.row0 * d.ldr;
  g.M = s.rows;
  g.ksplit = s.ksplit, g.kt_per = s.kt_per, g.partial = s.ksplit > 1 ? reinterpret_cast<float*>(partial) : nullptr;
  g.tail_rows = s.tail_rows, g.tiles_m = s.tiles_m, g.tiles_n = s.tiles_n, g.mubuf = s.mubuf;
  const dim3 grid(s.grid[0], s.grid[1], s.grid[2]);
  int e;
  if (s.kind == GK_ROWS16) {  // (gemm_rows.hip)
    RowsArgs a;
    static_cast<RowsEpi&>(a) = rows_epi(g);
    a.A = g.A; a.W = g.B; a.C = g.C; a.R = g.R;
    a.M = g.M; a.K = g.K;
    a.lda = g.lda; a.ldw = g.ldb;
    // the launcher derives waves, pair form and grid from the product; the plan (what gemm_plan_format prints) must say the same
    if (s.form != rows16_slices(g.K >> 5) || s.pair != bool(g.flags & GEMM_SWIGLU) || s.grid[0] != (int)cdiv(s.pair ? g.N >> 1 : g.N, s.pair ? 8 : 16))
      return U2_ERR_ARG;
    e = gemm_rows_launch(a, stream);
  } else if (s.kind == GK_TILE) {
    void (*const k[2][3])(GemmDesc) = {
        {gemm_bf16_nt_kernel<128, 128, true, true>, gemm_bf16_nt_kernel<128, 128, false, true>, gemm_bf16_nt_kernel<128, 128>},
        {gemm_bf16_nt_kernel<64, 64, true, true>, gemm_bf16_nt_kernel<64, 64, false, true>, gemm_bf16_nt_kernel<64, 64>}};
    hipLaunchKernelGGL(k[s.form != 128][s.ta ? 0 : s.tb ? 1 : 2], grid, dim3(256), 2 * (2 * s.form) * 64 * 2, stream, g);
    e = launch_status();
  } else {
    e = s.kind == GK_SKINNY ? gemm_skinny_launch(g, s, stream) : gemm_bt_launch(g, s, stream);
  }
  if (e != U2_OK || s.ksplit == 1) return e;
  // split-K: the epilogue over g.partial[ksplit][nz][M][N]
  hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3((unsigned)cdiv((int64_t)g.nz * g.M * ((g.N + 3) >> 2), 256)), dim3(256), 0, stream, g);
  return launch_status();
}

int gemm_bf16(GemmDesc d, hipStream_t stream) {
  const int flags = d.flags;
  const Scratch sc = ctx().scratch_of(stream);
  GemmPlan p;
  int e = gemm_validate(d);
  if (e == U2_OK) e = gemm_plan(d, opts(), sc.p ? sc.bytes : 0, p);
  static const bool trace = getenv("U2TOK_GEMM_TRACE") != nullptr;  // diagnostics: one line per product and its plan on stderr
  if (trace) {
    char route[512] = " | error";
    if (e == U2_OK) gemm_plan_format(p, route, sizeof(route));
    fprintf(stderr, "gemm M=%d N=%d K=%d nz=%d flags=0x%x lda=%d ldb=%d ldc=%d%s\n", d.M, d.N, d.K, d.nz, flags, (int)d.lda,
            (int)d.ldb, (int)d.ldc, route);
  }
  if (e != U2_OK) return e;
  const bool out_f32 = d.flags & GEMM_OUT_F32;
  const double zA = (d.sAb || d.sAh) ? d.nz : 1, zB = (d.sBb || d.sBh) ? d.nz : 1;  // a batch-shared operand is read once
  ProfScope ps(PROF_GEMM, 2.0 * d.M * d.N * d.K * d.nz, stream,
               (d.flags & GEMM_SWIGLU) ? 2.0 * d.M * d.K + 2.0 * d.N * d.K + 2.0 * d.M * (d.N >> 1)
                                       : 2.0 * d.M * d.K * zA + 2.0 * d.N * d.K * zB +
                                             d.nz * ((out_f32 ? 4.0 : 2.0) * d.M * d.N + ((d.flags & GEMM_RESIDUAL) ? 2.0 * d.M * d.N : 0.0)));
  for (int i = 0; i < p.nsteps && e == U2_OK; ++i) e = gemm_step(d, p.step[i], sc.p, stream);
  return e;
}

bool gemm_vt_supported(const GemmDesc& d, int vt_n0, int vt_rows) {
  GemmDesc v = d;
  v.vt = static_cast<bf16_t*>(v.C);  // (the plan only asks whether a transposed output is requested)
  v.vt_n0 = vt_n0;
  v.vt_rows = vt_rows;
  GemmPlan p;
  return gemm_validate(v) == U2_OK && gemm_plan(v, opts(), 0, p) == U2_OK && p.step[0].kind == GK_BIG && p.step[0].vt;
}

}  // namespace u2
