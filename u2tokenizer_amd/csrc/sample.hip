// Sampling warper (u2tokenizer_amd/sampling.py): temperature, top-k and top-p (nucleus) filtering of fp32 logits in one launch, without a
// sort.  fp32 only: the same code in both element builds.  Per row (include/u2tok.h has the full statement):
//   z = x / T (one correctly rounded division; T = 1: z = x);  top-k keeps z >= the k-th largest z (ties kept, -0 = +0);  top-p ranks the
//   survivors by (value, then index) descending and keeps a token iff the softmax mass ranked strictly above it is < top_p, or fewer than
//   min_keep tokens rank above it;  out = z where kept, -inf elsewhere.
// The kept set is "everything ranked at or above one boundary token", so what the kernel looks for is that token.  Every token gets the
// 64-bit composite  (order-preserving bit pattern of z) << 32 | index,  whose unsigned order IS the rank order, and the boundary is found by
// a radix descent over its eight bytes, most significant first: one pass over the row (it stays in L2 after the first) builds a 256-bin
// histogram of the current byte among the tokens that match the bytes already fixed, a suffix scan from the top picks the bin that holds the
// boundary.  Bytes that are the same in every token (the low 16 bits of bf16-valued logits, the high bytes of the index) cost no pass, and
// the descent stops as soon as the boundary's bin holds one token.  The top-k stage is the same descent on counts over the value bytes.
// DETERMINISM: the masses are exp(z - max) rounded to integers at 2^-40 (2^-(63 - log2 V) for rows longer than 2^23), the histograms are
// integer LDS adds: no sum depends on an order, the same input gives the same bits.
// One workgroup of 16 waves per row; workgroups never wait for each other.  LDS: 16 copies of the (count, mass) histograms (lane & 15 picks
// one: tokens of a wave that fall into one bin -- the few exponent bins of the first pass -- meet 4 to an address, not 64) = 48 KB.
#include "kernels.h"

namespace u2 {
namespace {

constexpr int SW_THREADS = 1024, SW_BINS = 256, SW_COPIES = 16;

struct SwShared {
  uint32_t hc[SW_BINS * SW_COPIES];   // [bin][copy] counts
  uint64_t hm[SW_BINS * SW_COPIES];   // [bin][copy] fixed-point masses
  uint32_t tc[SW_BINS];
  uint64_t tm[SW_BINS];
  float red_f[16];
  uint32_t red_or[16], red_and[16];
  uint64_t target, above_m;
  uint32_t bin, bin_cnt, above_c;
};

// unsigned order of the result = order of the floats; -0.0 and +0.0 get one key (NaNs land at the two ends)
__device__ __forceinline__ uint32_t order_key(float z) {
  uint32_t u = __float_as_uint(z);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SwRow {
  const float* x;
  int V;
  float T;
  bool div;
};

// Every pass walks the row the same way: a thread takes elements tid, tid + 1024, ... (4-byte loads: any V, any alignment of a row) in
// batches of SW_BATCH whose loads are all issued before the first is used.  (Measured: a pass over a 151 936-wide row takes ~45 us with
// the batches and with a plain loop alike -- DESIGN 7 f6 -- so the load latency is not what bounds the one-workgroup form.)
constexpr int SW_BATCH = 16;
template <typename F>
__device__ __forceinline__ void sw_for_each(const SwRow& r, int tid, F f) {
  for (int base = tid; base < r.V; base += SW_THREADS * SW_BATCH) {
    float x[SW_BATCH];
#pragma unroll
    for (int u = 0; u < SW_BATCH; ++u) {
      const int i = base + u * SW_THREADS;
      x[u] = i < r.V ? r.x[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SW_BATCH; ++u) {
      const int i = base + u * SW_THREADS;
      if (i < r.V) f(i, r.div ? x[u] / r.T : x[u]);
    }
  }
}

// The result of a descent: the boundary's composite with the bytes below `shift` unknown (zero) -- a token ranks at or above the boundary
// iff (composite >> shift) >= (prefix >> shift) -- and how many tokens do.
struct SwCut {
  uint64_t prefix;
  int shift;
  uint32_t kept;
};

// MASS: the boundary is the lowest-ranked token whose mass above it is < top_p of the total (target = ceil(top_p * total), set on the first
// histogram, which holds every token >= kmin);  else: the token of rank `count_target` (1 = the largest).  Tokens with key < kmin (removed
// by top-k) take no part.  Bytes lo_byte .. 7 of the composite are resolved; `varying` has a bit per byte that differs between tokens,
// `fixed` the value of the others.
template <bool MASS>
__device__ SwCut sw_descend(SwShared& sh, const SwRow& r, float zmax, float scale, uint32_t kmin, float top_p, uint32_t count_target,
                            int lo_byte, uint32_t varying, uint64_t fixed, uint32_t& passes) {
  const int tid = threadIdx.x, lane = tid & 63, copy = tid & (SW_COPIES - 1);
  uint64_t prefix = 0, above_m = 0;
  uint32_t above_c = 0;
  bool have_target = !MASS;
  for (int b = 7; b >= lo_byte; --b) {
    const int shift = 8 * b;
    if (!((varying >> b) & 1u)) {   // the same byte in every token: nothing to count
      prefix |= fixed & (0xffull << shift);
      continue;
    }
    for (int i = tid; i < SW_BINS * SW_COPIES; i += SW_THREADS) { sh.hc[i] = 0u; sh.hm[i] = 0ull; }
    __syncthreads();
    const uint64_t hi_mask = b == 7 ? 0ull : ~0ull << (shift + 8);
    sw_for_each(r, tid, [&](int i, float z) {
      const uint32_t key = order_key(z);
      const uint64_t comp = ((uint64_t)key << 32) | (uint32_t)i;
      if (key >= kmin && ((comp ^ prefix) & hi_mask) == 0ull) {
        const int slot = (int)((comp >> shift) & 0xffu) * SW_COPIES + copy;
        atomicAdd(&sh.hc[slot], 1u);
        if (MASS) atomicAdd(reinterpret_cast<unsigned long long*>(&sh.hm[slot]), (unsigned long long)__float2ull_rn(__expf(z - zmax) * scale));
      }
    });
    __syncthreads();
    if (tid < SW_BINS) {
      uint32_t c = 0;
      uint64_t m = 0;
#pragma unroll
      for (int j = 0; j < SW_COPIES; ++j) { c += sh.hc[tid * SW_COPIES + j]; m += sh.hm[tid * SW_COPIES + j]; }
      sh.tc[tid] = c;
      sh.tm[tid] = m;
    }
    __syncthreads();
    if (tid < 64) {   // lane l owns bins 4l .. 4l + 3; suffix sums from the top bin down
      uint32_t c[4];
      uint64_t v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = sh.tc[4 * lane + j]; v[j] = MASS ? sh.tm[4 * lane + j] : (uint64_t)c[j]; }
      const uint64_t sv = (v[0] + v[1]) + (v[2] + v[3]);
      const uint32_t sc = (c[0] + c[1]) + (c[2] + c[3]);
      uint64_t iv = sv;
      uint32_t ic = sc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint64_t tv = __shfl_down((unsigned long long)iv, o, 64);
        const uint32_t tcn = __shfl_down(ic, o, 64);
        if (lane + o < 64) { iv += tv; ic += tcn; }
      }
      uint64_t target = have_target ? (MASS ? sh.target : (uint64_t)count_target) : 0ull;
      if (!have_target) {   // ceil(top_p * total) in double: an error of 2^-53 of the total, far inside the masses' own rounding
        const uint64_t total = __shfl((unsigned long long)iv, 0, 64);
        const double t = ceil((double)top_p * (double)total);
        target = t >= 18446744073709551615.0 ? total : (uint64_t)t;
        if (target > total) target = total;
        if (target < 1ull) target = 1ull;
        if (lane == 0) sh.target = target;
      }
      uint64_t av = (MASS ? above_m : (uint64_t)above_c) + (iv - sv);   // what ranks above this lane's bins
      uint32_t ac = above_c + (ic - sc);
      int hit = -1;
      uint64_t hav = 0;
      uint32_t hac = 0;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        // (bin 0 always qualifies: a row of NaNs or infinities, whose sums mean nothing, still ends in some bin)
        if (hit < 0 && (av + v[j] >= target || (lane == 0 && j == 0))) { hit = j; hav = av; hac = ac; }
        av += v[j];
        ac += c[j];
      }
      const uint64_t ball = __ballot(hit >= 0);
      if (lane == 63 - __clzll((long long)ball)) {
        sh.bin = 4 * lane + hit;
        sh.bin_cnt = c[hit];
        sh.above_m = hav;
        sh.above_c = hac;
      }
    }
    __syncthreads();
    have_target = true;
    ++passes;
    prefix |= (uint64_t)sh.bin << shift;
    above_c = sh.above_c;
    if (MASS) above_m = sh.above_m;
    const uint32_t n = sh.bin_cnt;
    __syncthreads();   // (sh.bin .. are rewritten by the next pass)
    if (n <= 1u) return SwCut{prefix, shift, above_c + 1u};   // the boundary token itself: the bytes below cannot matter
  }
  return SwCut{prefix, 8 * lo_byte, above_c + 1u};
}

__global__ __launch_bounds__(SW_THREADS) void sample_warp_kernel(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int V,
                                                                 float T, int top_k, float top_p, int min_keep, float scale,
                                                                 uint32_t* records) {
  __shared__ SwShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const SwRow r{logits + row * ld_in, V, T, T != 1.0f};
  float* o = out + row * ld_out;

  // pass 0: the row's maximum, and which bits of the keys differ between tokens
  float zmax = -INFINITY;
  uint32_t k_or = 0u, k_and = ~0u;
  sw_for_each(r, tid, [&](int, float z) {
    const uint32_t key = order_key(z);
    zmax = fmaxf(zmax, z);
    k_or |= key;
    k_and &= key;
  });
  zmax = wave_max(zmax);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { k_or |= __shfl_xor(k_or, s, 64); k_and &= __shfl_xor(k_and, s, 64); }
  if (lane == 0) { sh.red_f[wave] = zmax; sh.red_or[wave] = k_or; sh.red_and[wave] = k_and; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SW_THREADS / 64; ++w) { zmax = fmaxf(zmax, sh.red_f[w]); k_or |= sh.red_or[w]; k_and &= sh.red_and[w]; }
  __syncthreads();
  const uint32_t k_diff = k_or ^ k_and;
  uint32_t varying = 0u;   // bit b: byte b of the composite (0-3 index, 4-7 key) differs between tokens
  for (int b = 0; b < 4; ++b) {
    if (((uint32_t)(V - 1) >> (8 * b)) != 0u) varying |= 1u << b;
    if ((k_diff >> (8 * b)) & 0xffu) varying |= 1u << (4 + b);
  }
  const uint64_t fixed = (uint64_t)k_or << 32;   // (where the bytes do not vary, or = and = the byte)

  uint32_t passes = 0u, kmin = 0u;
  const int64_t k = top_k > 0 ? (top_k > min_keep ? top_k : min_keep) : 0;
  if (k > 0 && k < V) {   // top-k: the k-th largest key; everything >= it survives, ties included
    const SwCut c = sw_descend<false>(sh, r, zmax, scale, 0u, 1.f, (uint32_t)k, 4, varying, fixed, passes);
    kmin = (uint32_t)(c.prefix >> 32);
  }
  SwCut cut{0ull, 0, 0u};   // top_p = 1: every survivor
  if (top_p < 1.f) {
    cut = sw_descend<true>(sh, r, zmax, scale, kmin, top_p, 0u, 0, varying, fixed, passes);
    const uint32_t need = (uint32_t)(min_keep < V ? min_keep : V);
    if (cut.kept < need)   // min_keep reaches past the nucleus: the boundary is the token of rank min_keep
      cut = sw_descend<false>(sh, r, zmax, scale, kmin, 1.f, need, 0, varying, fixed, passes);
  }
  const uint64_t want = cut.prefix >> cut.shift;
  // (out may be logits: an element is read here for the last time, by the thread that then writes it)
  sw_for_each(r, tid, [&](int i, float z) {
    const uint32_t key = order_key(z);
    const uint64_t comp = ((uint64_t)key << 32) | (uint32_t)i;
    o[i] = (key >= kmin && (comp >> cut.shift) >= want) ? z : -INFINITY;
  });
  if (tid == 0) {   // the row's record: boundary composite (low, high word), resolved-from bit, histogram passes taken
    uint32_t* rec = records + row * 8;
    rec[0] = (uint32_t)cut.prefix; rec[1] = (uint32_t)(cut.prefix >> 32); rec[2] = (uint32_t)cut.shift; rec[3] = passes;
    rec[4] = kmin; rec[5] = cut.kept; rec[6] = 0u; rec[7] = 0u;
  }
}

// ------------------------------------------------------------------------------------------------ the split-row form
// The same descent with a row spread over G workgroups, for calls of a few rows (one workgroup per row walks a 151 936-wide row eight
// times by itself).  Every pass of the descent is a LAUNCH: each workgroup builds the histogram of its slice of the row in LDS as above
// and adds its non-empty bins to the pass's table in the workspace with device-scope INTEGER atomics (counts, 2^-40 masses: no sum
// depends on an order, so the tables, and with them every decision, have the bits of the one-workgroup kernel's LDS histograms).  The
// next launch reads the table -- the kernel boundary on the stream is the only ordering between workgroups; nobody waits for anybody --
// and EVERY workgroup takes the bin decision from it again (sp_decide: sw_descend's suffix scan), so all agree; workgroup 0 of the row
// leaves the resulting state in the workspace for the launch after.  The host fixes the launches from the parameters alone: init
// (zeroes everything the call accumulates into), stats (maximum, varying bits), one launch per byte of each stage that the parameters
// ask for -- top-k: 4, top-p: 8, min_keep > 1 behind top-p: 8 --, final (the last decision, then the only writer of `out`).  A launch
// whose pass is decided already -- a byte equal in all tokens, a stage that ended on a bin of one token, a min_keep stage the nucleus
// made unnecessary -- returns after its decision.
constexpr int SP_MAX_PASS = 20, SP_MAX_G = 16, SP_STATE_BYTES = 64, SP_TABLE_BYTES = SW_BINS * 12;
constexpr size_t SP_ROW_BYTES = 64 + (size_t)(SP_MAX_PASS + 1) * SP_STATE_BYTES + (size_t)SP_MAX_PASS * SP_TABLE_BYTES;
enum : uint32_t { SP_HAVE_TARGET = 1u, SP_DONE = 2u, SP_SKIP2 = 4u };

struct SpState {   // a row's descent between two launches
  uint64_t prefix, above_m, target, cut_prefix;
  uint32_t above_c, kmin, cut_shift, cut_kept, passes, flags, done_shift, pad;
};
static_assert(sizeof(SpState) == SP_STATE_BYTES, "one state slot");

struct SpPlan {    // the call's histogram launches: stage 0 = top-k (counts), 1 = top-p (masses), 2 = min_keep (counts); byte 7 .. lo
  int n;
  int8_t stage[SP_MAX_PASS], byte[SP_MAX_PASS];
};

struct SpArgs {
  const float* logits;
  float* out;
  int64_t ld_in, ld_out;
  int V, G, chunk;       // G workgroups per row, each on `chunk` elements
  float T, top_p, scale;
  uint32_t k, need;      // top-k's count target (0: no top-k stage); min(min_keep, V)
  uint32_t* records;
  char* rows;            // rows x SP_ROW_BYTES, 8-byte aligned
  SpPlan plan;
};

__device__ __forceinline__ uint32_t* sp_hdr(const SpArgs& a, int64_t row) { return reinterpret_cast<uint32_t*>(a.rows + row * SP_ROW_BYTES); }
__device__ __forceinline__ SpState* sp_state(const SpArgs& a, int64_t row, int p) {
  return reinterpret_cast<SpState*>(a.rows + row * SP_ROW_BYTES + 64 + (size_t)p * SP_STATE_BYTES);
}
__device__ __forceinline__ uint32_t* sp_counts(const SpArgs& a, int64_t row, int p) {
  return reinterpret_cast<uint32_t*>(a.rows + row * SP_ROW_BYTES + 64 + (size_t)(SP_MAX_PASS + 1) * SP_STATE_BYTES + (size_t)p * SP_TABLE_BYTES);
}
__device__ __forceinline__ uint64_t* sp_masses(const SpArgs& a, int64_t row, int p) { return reinterpret_cast<uint64_t*>(sp_counts(a, row, p) + SW_BINS); }

__device__ __forceinline__ float key_to_float(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// sw_for_each over the slice [lo, hi) of the row
template <typename F>
__device__ __forceinline__ void sp_for_each(const SwRow& r, int lo, int hi, int tid, F f) {
  for (int64_t base = (int64_t)lo + tid; base < hi; base += SW_THREADS * SW_BATCH) {
    float x[SW_BATCH];
#pragma unroll
    for (int u = 0; u < SW_BATCH; ++u) {
      const int64_t i = base + u * SW_THREADS;
      x[u] = i < hi ? r.x[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SW_BATCH; ++u) {
      const int64_t i = base + u * SW_THREADS;
      if (i < hi) f((int)i, r.div ? x[u] / r.T : x[u]);
    }
  }
}

__global__ __launch_bounds__(256) void sp_init_kernel(SpArgs a, int64_t nrows) {
  uint32_t* w = reinterpret_cast<uint32_t*>(a.rows);
  const int64_t per = (int64_t)(SP_ROW_BYTES / 4), total = nrows * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) w[i] = (i % per) == 2 ? ~0u : 0u;   // (word 2: the AND of the keys)
}

// the row's maximum and the OR / AND of its keys: sample_warp_kernel's pass 0 on a slice, one atomic each per workgroup
__global__ __launch_bounds__(SW_THREADS) void sp_stats_kernel(SpArgs a) {
  __shared__ float red_f[16];
  __shared__ uint32_t red_or[16], red_and[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const SwRow r{a.logits + row * a.ld_in, a.V, a.T, a.T != 1.0f};
  const int64_t chunk = a.chunk;
  const int lo = (int)std::min<int64_t>(a.V, blockIdx.y * chunk), hi = (int)std::min<int64_t>(a.V, lo + chunk);
  float zmax = -INFINITY;
  uint32_t k_or = 0u, k_and = ~0u;
  sp_for_each(r, lo, hi, tid, [&](int, float z) {
    const uint32_t key = order_key(z);
    zmax = fmaxf(zmax, z);
    k_or |= key;
    k_and &= key;
  });
  zmax = wave_max(zmax);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { k_or |= __shfl_xor(k_or, s, 64); k_and &= __shfl_xor(k_and, s, 64); }
  if (lane == 0) { red_f[wave] = zmax; red_or[wave] = k_or; red_and[wave] = k_and; }
  __syncthreads();
  if (tid == 0 && lo < hi) {
    for (int w = 0; w < SW_THREADS / 64; ++w) { zmax = fmaxf(zmax, red_f[w]); k_or |= red_or[w]; k_and &= red_and[w]; }
    uint32_t* hdr = sp_hdr(a, row);
    atomicMax(&hdr[0], order_key(zmax));
    atomicOr(&hdr[1], k_or);
    atomicAnd(&hdr[2], k_and);
  }
}

// What the launch after pass q makes of pass q's table: sw_descend's loop body for (stage, byte b) on the state s, and at the stage's
// last byte the stage's result (kmin, or the cut) and a fresh descent state.  Uniform over the workgroup: every thread returns the same.
__device__ SpState sp_decide(SwShared& sh, SpState s, const uint32_t* tcnt, const uint64_t* tmass, int stage, int b, uint32_t varying,
                             uint64_t fixed, const SpArgs& a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const bool mass = stage == 1, runs = stage != 2 || !(s.flags & SP_SKIP2);
  const int shift = 8 * b, lo_byte = stage == 0 ? 4 : 0;
  if (runs && !(s.flags & SP_DONE)) {
    if (!((varying >> b) & 1u)) {
      s.prefix |= fixed & (0xffull << shift);
    } else {
      if (tid < SW_BINS) { sh.tc[tid] = tcnt[tid]; sh.tm[tid] = mass ? tmass[tid] : 0ull; }
      __syncthreads();
      if (tid < 64) {   // (sw_descend's scan: lane l owns bins 4l .. 4l + 3; suffix sums from the top bin down)
        const bool have_target = !mass || (s.flags & SP_HAVE_TARGET);
        uint32_t c[4];
        uint64_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { c[j] = sh.tc[4 * lane + j]; v[j] = mass ? sh.tm[4 * lane + j] : (uint64_t)c[j]; }
        const uint64_t sv = (v[0] + v[1]) + (v[2] + v[3]);
        const uint32_t sc = (c[0] + c[1]) + (c[2] + c[3]);
        uint64_t iv = sv;
        uint32_t ic = sc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint64_t tv = __shfl_down((unsigned long long)iv, o, 64);
          const uint32_t tcn = __shfl_down(ic, o, 64);
          if (lane + o < 64) { iv += tv; ic += tcn; }
        }
        uint64_t target = mass ? s.target : (uint64_t)(stage == 0 ? a.k : a.need);
        if (!have_target) {
          const uint64_t total = __shfl((unsigned long long)iv, 0, 64);
          const double t = ceil((double)a.top_p * (double)total);
          target = t >= 18446744073709551615.0 ? total : (uint64_t)t;
          if (target > total) target = total;
          if (target < 1ull) target = 1ull;
        }
        if (lane == 0) sh.target = target;
        uint64_t av = (mass ? s.above_m : (uint64_t)s.above_c) + (iv - sv);
        uint32_t ac = s.above_c + (ic - sc);
        int hit = -1;
        uint64_t hav = 0;
        uint32_t hac = 0;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          if (hit < 0 && (av + v[j] >= target || (lane == 0 && j == 0))) { hit = j; hav = av; hac = ac; }
          av += v[j];
          ac += c[j];
        }
        const uint64_t ball = __ballot(hit >= 0);
        if (lane == 63 - __clzll((long long)ball)) {
          sh.bin = 4 * lane + hit;
          sh.bin_cnt = c[hit];
          sh.above_m = hav;
          sh.above_c = hac;
        }
      }
      __syncthreads();
      if (mass) { s.target = sh.target; s.flags |= SP_HAVE_TARGET; }
      ++s.passes;
      s.prefix |= (uint64_t)sh.bin << shift;
      s.above_c = sh.above_c;
      if (mass) s.above_m = sh.above_m;
      const uint32_t n = sh.bin_cnt;
      __syncthreads();
      if (n <= 1u) { s.flags |= SP_DONE; s.done_shift = (uint32_t)shift; }
    }
  }
  if (b == lo_byte) {   // the stage ends: sw_descend's return value, then what the kernel does with it
    if (runs) {
      const uint32_t r_shift = (s.flags & SP_DONE) ? s.done_shift : (uint32_t)(8 * lo_byte), r_kept = s.above_c + 1u;
      if (stage == 0) {
        s.kmin = (uint32_t)(s.prefix >> 32);
      } else {
        s.cut_prefix = s.prefix; s.cut_shift = r_shift; s.cut_kept = r_kept;
        if (stage == 1 && !(r_kept < a.need)) s.flags |= SP_SKIP2;
      }
    }
    s.prefix = 0ull; s.above_m = 0ull; s.target = 0ull; s.above_c = 0u; s.done_shift = 0u;
    s.flags &= SP_SKIP2;
  }
  return s;
}

// the state in front of pass p (p = plan.n: behind the last one), from the state in front of pass p - 1 and that pass's table
__device__ SpState sp_advance(SwShared& sh, const SpArgs& a, int64_t row, int p, uint32_t varying, uint64_t fixed) {
  SpState s{};
  if (p > 0) s = sp_decide(sh, *sp_state(a, row, p - 1), sp_counts(a, row, p - 1), sp_masses(a, row, p - 1), a.plan.stage[p - 1], a.plan.byte[p - 1], varying, fixed, a);
  if (blockIdx.y == 0 && threadIdx.x == 0 && p < a.plan.n) *sp_state(a, row, p) = s;   // (read by the next launch alone)
  return s;
}

__device__ __forceinline__ void sp_header(const SpArgs& a, int64_t row, float& zmax, uint32_t& varying, uint64_t& fixed) {
  const uint32_t* hdr = sp_hdr(a, row);
  zmax = key_to_float(hdr[0]);
  const uint32_t k_or = hdr[1], k_diff = k_or ^ hdr[2];
  varying = 0u;
  for (int b = 0; b < 4; ++b) {
    if (((uint32_t)(a.V - 1) >> (8 * b)) != 0u) varying |= 1u << b;
    if ((k_diff >> (8 * b)) & 0xffu) varying |= 1u << (4 + b);
  }
  fixed = (uint64_t)k_or << 32;
}

__global__ __launch_bounds__(SW_THREADS) void sp_pass_kernel(SpArgs a, int p) {
  __shared__ SwShared sh;
  const int tid = threadIdx.x, copy = tid & (SW_COPIES - 1);
  const int64_t row = blockIdx.x;
  float zmax;
  uint32_t varying;
  uint64_t fixed;
  sp_header(a, row, zmax, varying, fixed);
  const SpState s = sp_advance(sh, a, row, p, varying, fixed);
  const int stage = a.plan.stage[p], b = a.plan.byte[p], shift = 8 * b;
  if ((stage == 2 && (s.flags & SP_SKIP2)) || (s.flags & SP_DONE) || !((varying >> b) & 1u)) return;   // decided already: nothing to count
  const SwRow r{a.logits + row * a.ld_in, a.V, a.T, a.T != 1.0f};
  const int64_t chunk = a.chunk;
  const int lo = (int)std::min<int64_t>(a.V, blockIdx.y * chunk), hi = (int)std::min<int64_t>(a.V, lo + chunk);
  if (lo >= hi) return;
  const bool mass = stage == 1;
  for (int i = tid; i < SW_BINS * SW_COPIES; i += SW_THREADS) { sh.hc[i] = 0u; sh.hm[i] = 0ull; }
  __syncthreads();
  const uint64_t hi_mask = b == 7 ? 0ull : ~0ull << (shift + 8), prefix = s.prefix;
  const uint32_t kmin = s.kmin;
  const float scale = a.scale;
  sp_for_each(r, lo, hi, tid, [&](int i, float z) {
    const uint32_t key = order_key(z);
    const uint64_t comp = ((uint64_t)key << 32) | (uint32_t)i;
    if (key >= kmin && ((comp ^ prefix) & hi_mask) == 0ull) {
      const int slot = (int)((comp >> shift) & 0xffu) * SW_COPIES + copy;
      atomicAdd(&sh.hc[slot], 1u);
      if (mass) atomicAdd(reinterpret_cast<unsigned long long*>(&sh.hm[slot]), (unsigned long long)__float2ull_rn(__expf(z - zmax) * scale));
    }
  });
  __syncthreads();
  if (tid < SW_BINS) {   // this workgroup's non-empty bins into the pass's table
    uint32_t c = 0;
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < SW_COPIES; ++j) { c += sh.hc[tid * SW_COPIES + j]; m += sh.hm[tid * SW_COPIES + j]; }
    if (c) atomicAdd(&sp_counts(a, row, p)[tid], c);
    if (mass && m) atomicAdd(reinterpret_cast<unsigned long long*>(&sp_masses(a, row, p)[tid]), (unsigned long long)m);
  }
}

__global__ __launch_bounds__(SW_THREADS) void sp_final_kernel(SpArgs a) {
  __shared__ SwShared sh;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  float zmax;
  uint32_t varying;
  uint64_t fixed;
  sp_header(a, row, zmax, varying, fixed);
  const SpState s = sp_advance(sh, a, row, a.plan.n, varying, fixed);
  const SwRow r{a.logits + row * a.ld_in, a.V, a.T, a.T != 1.0f};
  float* o = a.out + row * a.ld_out;
  const int64_t chunk = a.chunk;
  const int lo = (int)std::min<int64_t>(a.V, blockIdx.y * chunk), hi = (int)std::min<int64_t>(a.V, lo + chunk);
  const uint32_t kmin = s.kmin, cshift = s.cut_shift;
  const uint64_t want = s.cut_prefix >> cshift;
  // (out may be logits: the only launch that writes, and an element is read for the last time by the thread that then writes it)
  sp_for_each(r, lo, hi, tid, [&](int i, float z) {
    const uint32_t key = order_key(z);
    const uint64_t comp = ((uint64_t)key << 32) | (uint32_t)i;
    o[i] = (key >= kmin && (comp >> cshift) >= want) ? z : -INFINITY;
  });
  if (blockIdx.y == 0 && tid == 0) {
    uint32_t* rec = a.records + row * 8;
    rec[0] = (uint32_t)s.cut_prefix; rec[1] = (uint32_t)(s.cut_prefix >> 32); rec[2] = cshift; rec[3] = s.passes;
    rec[4] = kmin; rec[5] = s.cut_kept; rec[6] = 0u; rec[7] = 0u;
  }
}

}  // namespace

size_t sample_warp_workspace_bytes(int rows, int V) {
  if (rows < 1 || V < 2) return 0;
  return (size_t)cdiv((int64_t)rows * 32, 256) * 256;   // one 32-byte record per row
}

int sample_warp(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int rows, int V, float temperature, int top_k,
                float top_p, int min_keep, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!logits || !out || !ws) return U2_ERR_ARG;
  if (rows < 1 || V < 2 || !(temperature > 0.f) || !(top_p > 0.f && top_p <= 1.f) || min_keep < 1 || top_k < 0 || ld_in < V ||
      ld_out < V)
    return U2_ERR_ARG;
  if ((((uintptr_t)logits | (uintptr_t)out | (uintptr_t)ws) & 3)) return U2_ERR_ARG;
  if (ws_bytes < sample_warp_workspace_bytes(rows, V)) return U2_ERR_WORKSPACE;
  int bits = 0;   // ceil(log2 V): the masses are integers at 2^-min(40, 63 - bits), so that a row's total stays below 2^63
  while (((int64_t)1 << bits) < V) ++bits;
  const int e = 63 - bits < 40 ? 63 - bits : 40;
  ProfScope ps(PROF_ROWOP, 0, st, (double)rows * V * 8.0);
  hipLaunchKernelGGL(sample_warp_kernel, dim3((unsigned)rows), dim3(SW_THREADS), 0, st, logits, ld_in, out, ld_out, V, temperature, top_k,
                     top_p, min_keep, ldexpf(1.f, e), reinterpret_cast<uint32_t*>(ws));
  return launch_status();
}

// ---- the split-row form: the same contract; the workspace also holds, behind the records, a header, the states and the tables per row
static int sp_groups(int V) { return (int)std::min<int64_t>(SP_MAX_G, cdiv((int64_t)V, (int64_t)SAMPLE_SPLIT_SLICE)); }

size_t sample_warp_split_workspace_bytes(int rows, int V) {
  const size_t rec = sample_warp_workspace_bytes(rows, V);
  return rec ? rec + 8 + (size_t)rows * SP_ROW_BYTES : 0;   // (+ 8: the rows' part starts at the next 8-byte boundary)
}

int sample_warp_split_launches(int V, int top_k, float top_p, int min_keep) {
  const int64_t k = top_k > 0 ? (top_k > min_keep ? top_k : min_keep) : 0;
  return 3 + (k > 0 && k < V ? 4 : 0) + (top_p < 1.f ? 8 : 0) + (top_p < 1.f && min_keep > 1 ? 8 : 0);
}

int sample_warp_split(const float* logits, int64_t ld_in, float* out, int64_t ld_out, int rows, int V, float temperature, int top_k,
                      float top_p, int min_keep, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!logits || !out || !ws) return U2_ERR_ARG;
  if (rows < 1 || V < 2 || !(temperature > 0.f) || !(top_p > 0.f && top_p <= 1.f) || min_keep < 1 || top_k < 0 || ld_in < V ||
      ld_out < V)
    return U2_ERR_ARG;
  if ((((uintptr_t)logits | (uintptr_t)out | (uintptr_t)ws) & 3)) return U2_ERR_ARG;
  if (ws_bytes < sample_warp_split_workspace_bytes(rows, V)) return U2_ERR_WORKSPACE;
  int bits = 0;
  while (((int64_t)1 << bits) < V) ++bits;
  const int e = 63 - bits < 40 ? 63 - bits : 40;
  SpArgs a;
  a.logits = logits; a.out = out; a.ld_in = ld_in; a.ld_out = ld_out; a.V = V; a.G = sp_groups(V); a.chunk = (int)cdiv((int64_t)V, (int64_t)a.G);
  a.T = temperature; a.top_p = top_p; a.scale = ldexpf(1.f, e);
  const int64_t k = top_k > 0 ? (top_k > min_keep ? top_k : min_keep) : 0;
  a.k = k > 0 && k < V ? (uint32_t)k : 0u;
  a.need = (uint32_t)(min_keep < V ? min_keep : V);
  a.records = reinterpret_cast<uint32_t*>(ws);
  a.rows = reinterpret_cast<char*>(((uintptr_t)ws + sample_warp_workspace_bytes(rows, V) + 7) & ~(uintptr_t)7);
  a.plan.n = 0;
  auto stage = [&](int s, int lo) { for (int b = 7; b >= lo; --b) { a.plan.stage[a.plan.n] = (int8_t)s; a.plan.byte[a.plan.n++] = (int8_t)b; } };
  if (a.k) stage(0, 4);
  if (top_p < 1.f) stage(1, 0);
  if (top_p < 1.f && min_keep > 1) stage(2, 0);
  ProfScope ps(PROF_ROWOP, 0, st, (double)rows * V * 8.0);
  const dim3 grid((unsigned)rows, (unsigned)a.G);
  const int64_t words = (int64_t)rows * (int64_t)(SP_ROW_BYTES / 4);
  hipLaunchKernelGGL(sp_init_kernel, dim3((unsigned)std::min<int64_t>(4096, cdiv(words, (int64_t)256))), dim3(256), 0, st, a, (int64_t)rows);
  hipLaunchKernelGGL(sp_stats_kernel, grid, dim3(SW_THREADS), 0, st, a);
  for (int p = 0; p < a.plan.n; ++p) hipLaunchKernelGGL(sp_pass_kernel, grid, dim3(SW_THREADS), 0, st, a, p);
  hipLaunchKernelGGL(sp_final_kernel, grid, dim3(SW_THREADS), 0, st, a);
  return launch_status();
}

}  // namespace u2
