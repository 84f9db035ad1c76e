// GEMM routing: which kernel instantiation(s) run a product.  gemm_plan() is a pure function of the validated descriptor, the
// options and the split-K scratch of the launch stream; gemm_bf16 (gemm.hip) executes what it returns.  Host code only
// (tests/test_gemm_plan.py compiles this file with a small driver and checks the routes on the CPU).
#include <cstdio>
#include <algorithm>
#include "rows.h"  // rows16_slices

namespace u2 {

int gemm_validate(GemmDesc& d) {
  if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.nz <= 0 || d.nz > 65535) return U2_ERR_ARG;
  if (!d.A || !d.B || !d.C) return U2_ERR_ARG;
  if (d.nsplit < 0 || (d.nsplit & 15) || (d.nsplit && (d.flags & GEMM_SWIGLU))) return U2_ERR_ARG;
  if (d.nbh <= 0) d.nbh = 1;
  // 16-byte chunked loads along the contiguous dimension of each operand (K, or M / N of a K-major one): that dimension,
  // leading dims and batch strides must keep every chunk aligned
  if (d.flags & GEMM_SWIGLU) {  // gate | up pair product with SiLU(gate) * up in the epilogue: the 256 x 192-tile kernel only
    const int64_t I = d.N >> 1;
    if ((d.flags & ~GEMM_SWIGLU) || d.nz != 1 || d.ldbk || (d.N & 1) || (I & 15) || (d.K & 63) || d.ldc < I || (d.ldc & 7) ||
        (d.lda & 7) || (d.ldb & 7) || (((uintptr_t)d.A | (uintptr_t)d.B | (uintptr_t)d.C) & 15))
      return U2_ERR_ARG;
    return U2_OK;
  }
  const bool ta = d.flags & GEMM_A_KMAJOR, tb = d.flags & GEMM_B_KMAJOR;
  if ((ta && !tb) || (tb && d.ldbk)) return U2_ERR_ARG;
  if ((ta ? d.M : d.K) & 7) return U2_ERR_ARG;
  if ((tb ? d.N : d.K) & 7) return U2_ERR_ARG;
  if ((ta && d.lda < d.M) || (tb && d.ldb < d.N)) return U2_ERR_ARG;
  if ((d.lda & 7) || (d.ldb & 7) || (d.sAb & 7) || (d.sAh & 7) || (d.sBb & 7) || (d.sBh & 7)) return U2_ERR_ARG;
  if (((uintptr_t)d.A & 15) || ((uintptr_t)d.B & 15)) return U2_ERR_ARG;
  if ((d.flags & (GEMM_BIAS_N | GEMM_BIAS_M)) && !d.bias) return U2_ERR_ARG;
  if ((d.flags & GEMM_RESIDUAL) && !d.R) return U2_ERR_ARG;
  const bool out_f32 = d.flags & GEMM_OUT_F32;
  bool vec = (d.ldc % 4 == 0) && (d.sCb % 4 == 0) && (d.sCh % 4 == 0) && (((uintptr_t)d.C & (out_f32 ? 15 : 7)) == 0);
  if (d.flags & GEMM_BIAS_N) vec = vec && (((uintptr_t)d.bias & 7) == 0);
  if (d.flags & GEMM_RESIDUAL)
    vec = vec && (d.ldr % 4 == 0) && (d.sRb % 4 == 0) && (d.sRh % 4 == 0) && (((uintptr_t)d.R & 7) == 0);
  d.flags = vec ? (d.flags | GEMM_VEC_OK) : (d.flags & ~GEMM_VEC_OK);
  return U2_OK;
}

namespace {

void push(GemmPlan& p, const GemmStep& s) { p.step[p.nsteps++] = s; }

// ------------------------------------------------------------------------------------------------ M <= 16 rows (gemm_rows.hip)
// one batch entry, K-contiguous operands, K % 32 == 0
bool rows16_ok(const GemmDesc& d) {
  return d.M <= 16 && d.nz == 1 && !(d.K & 31) && !d.ldbk && !(d.flags & (GEMM_A_KMAJOR | GEMM_B_KMAJOR));
}

GemmStep rows16_step(const GemmDesc& d, int row0) {
  GemmStep s{GK_ROWS16, rows16_slices(d.K >> 5), row0, d.M};  // waves splitting the K / 32 steps
  s.pair = d.flags & GEMM_SWIGLU;
  s.grid[0] = (int)cdiv(d.N, 16);
  return s;
}

// ------------------------------------------------------------------------------------------------ 128^2 / 64^2 tiles (gemm.hip)
GemmStep tile_step(const GemmDesc& d, const Options& o, size_t scratch, int row0) {
  GemmStep s{GK_TILE, 0, row0, d.M};
  int tile = o.gemm_tile;
  // "long K": weight-gradient products of the training path (dW = dY^T X: a small output, K = the 16392 token rows of the
  // ViT).  64 x 64 tiles fill the CUs there but run at ~0.35-0.4 PF/s (197 us for 3072 x 768 x 16392); 128 x 128 tiles with
  // K sliced over 5-8 workgroups keep the better tile and fill the machine.  No inference product has K >= 8192.
  bool longk = false;
  if (tile != 64 && tile != 128) {
    const int64_t big = cdiv(d.M, 128) * cdiv(d.N, 128) * d.nz;
    tile = (big >= 192) ? 128 : 64;  // fill 256 CUs; small-M weight-streaming shapes get 64^2 tiles
    if (tile == 64 && o.gemm_splitk == 0 && d.nz == 1 && d.M >= 512 && d.N >= 512 && d.K >= 8192) {
      tile = 128;
      longk = true;
    }
  }
  // split-K: a product with fewer workgroups than ~2 per CU runs one single-stage-prefetch K loop per CU and is
  // latency-bound (M = 256, N = K = 4096: 36 us, 0.24 PF/s).  Slicing K puts several workgroups on every CU.
  if (o.gemm_splitk >= 0) {
    const int64_t wgs = cdiv(d.M, tile) * cdiv(d.N, tile) * d.nz;
    const int nkt = (int)cdiv(d.K, 64);
    int n = o.gemm_splitk > 1 ? o.gemm_splitk : 0;
    // (128 x 128 tiles: two workgroups per CU are resident -> aim at 512; the decoder prefill's M = 1024 out / down
    //  projections are 256 tiles with K = 4096 / 12288: one K loop per CU with nothing to overlap it otherwise)
    if (n == 0 && d.nz == 1 && (wgs <= 320 || longk) && nkt >= 16)
      n = (int)std::min<int64_t>(8, std::min<int64_t>(nkt / 4, cdiv(longk ? 640 : (tile == 128 ? 512 : 1024), wgs)));
    if (n > 1) {
      const size_t slice = (size_t)d.nz * d.M * d.N * sizeof(float);
      // partial sums cost HBM traffic: capped at 24 MB unless the K loop is long enough to dwarf it
      if (o.gemm_splitk <= 1)
        n = (int)std::min<size_t>(n, (longk ? scratch : std::min<size_t>(scratch, (tile == 128 ? 40u : 24u) << 20)) / slice);
      if (n > 1 && (size_t)n * slice <= scratch) {
        s.kt_per = (int)cdiv(nkt, n);
        s.ksplit = (int)cdiv(nkt, s.kt_per);  // no empty slices
      }
    }
  }
  if (longk && s.ksplit == 1) tile = 64;  // no scratch for the slices: the tile that fills the CUs
  s.form = tile;
  s.ta = d.flags & GEMM_A_KMAJOR;
  s.tb = d.flags & GEMM_B_KMAJOR;
  s.tiles_m = (int)cdiv(d.M, tile);
  s.tiles_n = (int)cdiv(d.N, tile);
  s.grid[0] = s.tiles_m * s.tiles_n;
  s.grid[1] = d.nz;
  s.grid[2] = s.ksplit;
  {  // MUBUF pieces when every byte offset of a batch entry's operands (K tile advance included) stays below 2^31
    const int64_t ktiles = cdiv(d.K, 64) + 1;
    const int64_t ea = (s.ta ? ktiles * 64 * d.lda + d.M : (int64_t)d.M * d.lda + ktiles * 64) * 2;
    const int64_t eb = (s.tb ? ktiles * 64 * d.ldb + d.N : d.ldbk ? ktiles * d.ldbk + (int64_t)d.N * d.ldb : (int64_t)d.N * d.ldb + ktiles * 64) * 2;
    s.mubuf = o.gemm_mubuf && ea < (1ll << 31) - 65536 && eb < (1ll << 31) - 65536;
  }
  return s;
}

void plan_classic(const GemmDesc& d, const Options& o, size_t scratch, int row0, GemmPlan& p) {
  if (o.gemm_tile == 0) {  // (a forced tile keeps the tile kernels: tests of their row tails)
    if (rows16_ok(d)) return push(p, rows16_step(d, row0));
    // <= 16 rows past a multiple of 128 in a many-row product (the ViT's GELU product: M = 16384 + 8 cls rows, 24 column
    // tiles): one more row of 128 x 128 tiles is 24 workgroups that start a SEVENTH round after six full ones (+ 16 %);
    // the few-rows kernel takes them instead
    const int rem = d.M & 127;
    if (d.nz == 1 && d.M >= 2048 && rem != 0 && rem <= 16 && !(d.K & 31) && !d.ldbk &&
        !(d.flags & (GEMM_A_KMAJOR | GEMM_B_KMAJOR | GEMM_BIAS_M))) {
      GemmDesc main = d, tail = d;
      main.M = d.M - rem;
      tail.M = rem;
      push(p, tile_step(main, o, scratch, row0));
      return push(p, rows16_step(tail, row0 + main.M));
    }
  }
  push(p, tile_step(d, o, scratch, row0));
}

// ------------------------------------------------------------------------------------------------ 64 < M <= 256 (gemm_skinny.hip)
// One batch entry, 64 < M <= 256 rows, row-major operands, K a multiple of 128 with >= 16 K tiles of 64, N = 2048 .. 4096 in whole
// 64-column strips (about one workgroup per CU; wider products fill the chip with the big-tile kernel's slices), 16-byte epilogue
// accesses.  Needs no scratch.
// (A batched TTA call, B queries x 256 rows in one product, has M = B 256 > 256 and takes the big-tile or tile kernels instead: its
// results differ from those of B single calls in summation order.)
bool skinny_step(const GemmDesc& d, const Options& o, GemmStep& s) {
  if (!o.gemm_skinny || o.gemm_tile != 0 || o.gemm_big != 0 || o.gemm_splitk != 0) return false;  // (forced choices keep their kernels)
  if (d.nz != 1 || d.M <= 64 || d.M > 256 || (d.N & 63) || (d.K & 127) || d.ldbk) return false;
  if (d.flags & (GEMM_BIAS_M | GEMM_A_KMAJOR | GEMM_B_KMAJOR | GEMM_SWIGLU) || !(d.flags & GEMM_VEC_OK) || d.vt) return false;
  const bool f32 = d.flags & GEMM_OUT_F32;
  if (((uintptr_t)d.C & 15) || (d.ldc & (f32 ? 3 : 7))) return false;
  if ((d.flags & GEMM_BIAS_N) && ((uintptr_t)d.bias & 15)) return false;
  if ((d.flags & GEMM_RESIDUAL) && (((uintptr_t)d.R & 15) || (d.ldr & 7))) return false;
  if ((d.K >> 6) < 16 || d.N < 32 * 64 || d.N > 64 * 64) return false;
  s = GemmStep{GK_SKINNY, 0, 0, d.M};
  s.tiles_m = (d.M + 63) >> 6;
  s.tiles_n = d.N >> 6;  // 64-column strips
  s.grid[0] = s.tiles_m * s.tiles_n;
  // (option gemm_skinny = 1: FLAT-encoded global_load_lds pieces instead of buffer_load ... lds -- A/B)
  s.mubuf = o.gemm_skinny == 2 && (int64_t)d.M * d.lda < (1ll << 29) && (int64_t)d.N * d.ldb < (1ll << 29);
  return true;
}

// ------------------------------------------------------------------------------------------------ big tiles (gemm_bt.hip)
// variants: 20 = 256 x 256, 21 = 256 x 192, 22 = 256 x 128 tiles (ring form); 24 = 256 x 192 with B deep, 26 = 256 x 256 with B deep,
// 27 = 24 as the drain form (tile i's epilogue under tile i + 1's K loop)

// 64-wide K tiles only (at least two); 32-bit byte offsets into A and B (per z)
bool bt_legal(const GemmDesc& d) {
  return !(d.K & 63) && d.K >= 128 && (int64_t)d.M * d.lda < (1ll << 30) && (int64_t)d.N * d.ldb < (1ll << 30);
}

// Which tile (DESIGN.md section 3 has the tables): the kernel runs its K loop at ~50 % of the MFMA peak but nothing overlaps its
// prologue and epilogue, and a product is as slow as its last round of tiles: it is taken when the tiles fill their rounds of 256
// workgroups to >= 70 %, with the tile width that needs the fewest (work-weighted) rounds -- the ViT's N = 2304 / 768 projections are
// exactly 3 / 1 rounds of 192-wide tiles, N = 3072 exactly 3 rounds of 256-wide ones.  GELU products too (packed-math GELU: fc1 of the
// ViT 113 us here against 128 on the 128 x 128 kernel, profiles/r04_bt_gelu_forms.log).
int bt_pick(const GemmDesc& d, const Options& o) {
  if (!bt_legal(d) || d.K < 256) return 0;
  const int gmax = o.gemm_big_grid;
  const int64_t tm = cdiv(d.M, 256) * d.nz;
  const int64_t t4 = tm * cdiv(d.N, 256), t3 = tm * cdiv(d.N, 192);
  const int64_t r4 = cdiv(t4, gmax), r3 = cdiv(t3, gmax);
  const double fill4 = (double)d.M * d.N * d.nz / ((double)r4 * gmax * 65536.0);
  const double fill3 = (double)d.M * d.N * d.nz / ((double)r3 * gmax * 49152.0);
  const double c4 = (double)r4, c3 = 0.9 * (double)r3;  // a 192-wide tile takes ~0.9 of the time of a 256-wide one
  if (c3 < c4) return fill3 >= 0.7 ? 21 : (fill4 >= 0.7 ? 20 : 0);
  return fill4 >= 0.7 ? 20 : (fill3 >= 0.7 ? 21 : 0);
}

// The ring form (256 x 128 tiles, variant 22) for products whose 256- and 192-wide tiles leave the CUs a partial round (bt_pick: fill
// < 70 %) while the 128-wide ones make ONE round that is at least three-quarters full: M = 2048 rows against an E x E weight, 1024
// against 2E x E, 2048 x 4096 x 6144 -- 256 tiles each (profiles/r04_bt_ring_sweep.log, r04_bt_counted_waits_ab.log).
bool bt_ring(const GemmDesc& d, const Options& o) {
  if (d.M < 512 || bt_pick(d, o) != 0 || !bt_legal(d) || d.K < 512) return false;
  const int gmax = o.gemm_big_grid;
  const int64_t t2 = cdiv(d.M, 256) * cdiv(d.N, 128) * d.nz;
  return t2 * 4 >= (int64_t)gmax * 3 && t2 <= gmax;
}

// Products that leave the 256 CUs a partial round of big tiles, sliced along K so that (tiles x slices) fills them -- the cases
// tools/bt_sweep.py measured ahead of the 128 x 128 kernel with its own split-K (profiles/r03_bt_sweep.log): (a) 129..256 rows against
// a wide weight (256 x 12288 x 4096: 256 x 192 tiles, 4 slices), (b) 512..1024 rows, K >= 8192 (256 x 256, 4), (c) 512..1024 rows
// whose 192-wide tiles make exactly half a round (256 x 192, 2).  Returns variant | slices << 8, or 0.
int bt_pick_sliced(const GemmDesc& d) {
  if (!bt_legal(d) || d.nz != 1 || (d.flags & GEMM_GELU)) return 0;
  const int64_t tm = cdiv(d.M, 256);
  if (d.M > 128 && d.M <= 256 && d.N >= 8192 && d.K >= 2048) return 21 | (4 << 8);
  if (d.M >= 512 && d.M <= 1024 && (d.M & 255) == 0) {
    if (d.K >= 8192 && d.N >= 2048 && tm * cdiv(d.N, 256) <= 64) return 20 | (4 << 8);
    const int64_t t3 = tm * (d.N / 192);
    if (d.N % 192 == 0 && d.K >= 4096 && t3 >= 112 && t3 <= 128) return 21 | (2 << 8);
  }
  return 0;
}

// K slices: fill the 256 CUs, keep >= 4 K tiles per slice (and >= 2 in the last one: the K loop's pipeline), within the stream's
// scratch.  Sets s.ksplit / s.kt_per and returns the slice count (1 = unsplit).
int bt_slices(const GemmDesc& d, int want, size_t scratch, GemmStep& s) {
  const int nkt = d.K >> 6;
  if (want <= 1 || d.nz != 1 || nkt < 8) return 1;
  const size_t slice = (size_t)d.M * d.N * sizeof(float);
  if (scratch < 2 * slice) return 1;
  for (int n = (int)std::min<size_t>(std::min(want, nkt / 4), scratch / slice); n > 1; --n) {
    const int per = (int)cdiv(nkt, n), used = (int)cdiv(nkt, per);
    if (nkt - (used - 1) * per >= 2) {  // last slice long enough
      s.ksplit = used;
      s.kt_per = per;
      return used;
    }
  }
  return 1;
}

// May the deep 256 x 192 launch of `d` (many-row part: M a multiple of 256) run as the drain form?
bool bt_drain_ok(const GemmDesc& d, const Options& o) {
  if (!o.gemm_big_drain || d.nz != 1) return false;
  if (d.flags & ~(GEMM_VEC_OK | GEMM_BIAS_N | GEMM_GELU)) return false;
  if (d.K % 384 || d.K < 768 || d.M % 256 || d.N % 192 || d.nsplit % 192) return false;
  if ((d.flags & GEMM_BIAS_N) && d.N > 6144) return false;
  if ((d.flags & GEMM_GELU) && d.vt) return false;
  if (((int64_t)d.M - 1) * d.ldc + d.N >= (1ll << 30)) return false;
  if (d.vt && (int64_t)(d.M / d.vt_rows) * d.vt_bs >= (1ll << 30)) return false;
  const int64_t tiles = (int64_t)(d.M / 256) * (d.N / 192);
  return tiles >= 2 * (int64_t)o.gemm_big_grid;  // every workgroup has a tile to hide the previous one under
}

// Adds the step of variant v over the rows of `d` (s: rows, K slices and in-launch tail already set); U2_ERR_ARG past the grid limit.
int bt_step(const GemmDesc& d, const Options& o, int v, GemmStep& s, GemmPlan& p) {
  s.form = v;
  s.pair = d.flags & GEMM_SWIGLU;
  s.gelu = d.flags & GEMM_GELU;
  s.vt = d.vt != nullptr;
  s.tiles_m = (int)cdiv(d.M, 256);
  s.tiles_n = (int)cdiv(d.N, v == 20 || v == 26 ? 256 : v == 22 ? 128 : 192);
  const int64_t total = (int64_t)s.tiles_m * s.tiles_n * (s.ksplit > 1 ? s.ksplit : d.nz);
  if (total > 0x3fffffff) return U2_ERR_ARG;
  s.grid[0] = (int)std::min<int64_t>(total, o.gemm_big_grid);  // persistent workgroups
  push(p, s);
  return U2_OK;
}

// A transposed side output (GemmDesc::vt) is left by the deep 256 x 192 form and its drain form only, as the heuristic picks them for
// the many-row part of the product (a cls-row tail goes to the few-rows kernel and is written to C as usual): plain bf16 output
// without bias or residual, whole tiles on both sides of vt_n0, and 256-row tiles that do not straddle a chunk of vt_rows keys.
bool vt_ok(const GemmDesc& d, const Options& o, const GemmStep& m) {
  return o.gemm_big == 0 && m.kind == GK_BIG && (m.form == 24 || m.form == 27) && d.nz == 1 && !(d.flags & ~GEMM_VEC_OK) &&
         d.vt_n0 > 0 && d.vt_n0 < d.N && d.vt_n0 % 192 == 0 && (d.N - d.vt_n0) % 192 == 0 && d.nsplit <= d.vt_n0 &&
         d.vt_rows > 0 && d.vt_rows % 256 == 0 && m.rows % d.vt_rows == 0;
}

// 1 = planned, 0 = not this kernel's, < 0 = error.
int plan_big(const GemmDesc& d, const Options& o, size_t scratch, GemmPlan& p) {
  const int mode = o.gemm_big;
  if (mode < 0) return 0;
  if (!(d.flags & GEMM_VEC_OK) || (d.flags & (GEMM_BIAS_M | GEMM_A_KMAJOR | GEMM_B_KMAJOR)) || (d.N & 7)) return 0;
  switch (d.flags & (GEMM_BIAS_N | GEMM_GELU | GEMM_RESIDUAL | GEMM_OUT_F32)) {
    case 0: case GEMM_OUT_F32: case GEMM_BIAS_N: case GEMM_BIAS_N | GEMM_OUT_F32: case GEMM_BIAS_N | GEMM_GELU:
    case GEMM_BIAS_N | GEMM_RESIDUAL: case GEMM_RESIDUAL: break;
    default: return 0;
  }
  // 16-byte epilogue accesses (8 consecutive n per lane)
  const bool f32 = d.flags & GEMM_OUT_F32;
  if (((uintptr_t)d.C & 15) || (d.ldc & (f32 ? 3 : 7)) || (d.sCb & (f32 ? 3 : 7)) || (d.sCh & (f32 ? 3 : 7))) return 0;
  if ((d.flags & GEMM_BIAS_N) && ((uintptr_t)d.bias & 15)) return 0;
  if ((d.flags & GEMM_RESIDUAL) && (((uintptr_t)d.R & 15) || (d.ldr & 7) || (d.sRb & 7) || (d.sRh & 7))) return 0;
  GemmStep s{GK_BIG, mode, 0, d.M};
  if (mode > 0) {  // forced (tests, measurements)
    if (!bt_legal(d) || (mode == 27 && !bt_drain_ok(d, o))) return 0;
    if (mode <= 22) bt_slices(d, o.gemm_big_splitk, scratch, s);
    const int e = bt_step(d, o, mode, s, p);
    return e ? e : 1;
  }
  // A few rows past a multiple of 256 (the ViT's cls rows: M = 2049 per chunk, 8 * 2049 per volume) would cost a whole extra
  // row of tiles: they go through the few-rows / small-tile kernel -- for EVERY form, so that a chunk's rows are computed
  // by the same arithmetic whatever the number of chunks in the call (tests/test_gpu_path.py::test_vit_full_size_properties).
  const int rem = d.M & 255;
  const bool split_tail = d.nz == 1 && rem != 0 && rem <= 64 && d.M > 256;
  GemmDesc main = d;
  if (split_tail) main.M = d.M - rem;
  s.rows = main.M;
  int v = 0;
  if (bt_ring(main, o)) {
    v = 22;  // (ahead of the sliced forms: 192 ring tiles beat 2 x 128 sliced ones)
  } else if (const int sl = split_tail ? 0 : bt_pick_sliced(d)) {
    if (d.vt) return U2_ERR_ARG;  // (no transposed form; refused whatever the scratch, so that gemm_vt_supported needs none)
    if (bt_slices(d, sl >> 8, scratch, s) == (sl >> 8)) {  // (fewer slices than wanted: the small-tile kernel is the better one)
      const int e = bt_step(d, o, sl & 0xff, s, p);
      return e ? e : 1;
    }
    s.ksplit = 1, s.kt_per = 0;
  }
  if (v == 0) {
    if (d.M < 512 || d.N < 256 || d.K < 128) return 0;
    v = bt_pick(main, o);
    if (v == 0) return 0;
    // launched as the deep form of the same tile width with B as the three-stage operand (26 / 24; profiles/r04_bt_deep_*.log);
    // GELU products keep two stages (profiles/r04_bt_gelu_forms.log)
    if (!(d.flags & GEMM_GELU)) v = v == 20 ? 26 : 24;
    // round 6, the drain form: products whose workgroups walk two or more 256 x 192 tiles hide tile i's epilogue under tile i + 1's
    // K loop.  A GELU product prefers it over the 256-wide two-stage form whenever its 192-wide tiles fill their rounds (fc1 of the
    // ViT: four whole rounds instead of three with 256 GELUs per lane exposed in each).
    if (bt_drain_ok(main, o)) {
      const int gmax = o.gemm_big_grid;
      const int64_t t3 = (int64_t)(main.M / 256) * (main.N / 192);
      const double fill3 = (double)t3 / ((double)cdiv(t3, gmax) * gmax);
      if (v == 24 || ((d.flags & GEMM_GELU) && fill3 >= 0.7)) v = 27;
    }
  }
  // <= 16 tail rows ride in the launch of the plain 256 x 256 (20) and deep 256 x 192 (24) forms -- what the ViT's products run
  if (split_tail && rem <= 16 && !(d.K & 31) && (v == 20 || v == 24 || v == 27) && o.gemm_tail_fused) s.tail_rows = rem;
  if (const int e = bt_step(main, o, v, s, p)) return e;
  if (split_tail && !s.tail_rows) {
    GemmDesc tail = d;
    tail.M = rem;
    plan_classic(tail, o, scratch, main.M, p);
  }
  return 1;
}

}  // namespace

int gemm_plan(const GemmDesc& d, const Options& o, size_t scratch, GemmPlan& p) {
  p = GemmPlan{};
  if (d.flags & GEMM_SWIGLU) {  // (validated: alone, N = 2 I)
    // a few rows (decode steps): the few-rows kernel has the pair form too; otherwise only the big-tile kernel has it
    // (256 x 192 tiles = 96 output columns)
    if (d.M <= 16 && o.gemm_tile == 0 && rows16_ok(d)) return push(p, rows16_step(d, 0)), U2_OK;
    if (d.vt || !bt_legal(d)) return U2_ERR_ARG;
    GemmStep s{GK_BIG, 21, 0, d.M};
    return bt_step(d, o, 21, s, p);
  }
  if (d.ldbk == 0) {  // (the 256-wide-tile kernels read row-major B only)
    if (skinny_step(d, o, p.step[0])) return p.nsteps = 1, U2_OK;
    const int big = plan_big(d, o, scratch, p);
    if (big < 0) return big;
    if (big > 0) return d.vt && !vt_ok(d, o, p.step[0]) ? U2_ERR_ARG : U2_OK;
  }
  if (d.vt) return U2_ERR_ARG;  // (a transposed side output only exists in the big-tile kernel: ask gemm_vt_supported first)
  plan_classic(d, o, scratch, 0, p);
  return U2_OK;
}

// " | <kernel instantiation, as the profilers name it> rows= grid= slices= tail=" per step
void gemm_plan_format(const GemmPlan& p, char* buf, size_t n) {
  const char* tf[2] = {"false", "true"};
  size_t k = 0;
  for (int i = 0; i < p.nsteps; ++i) {
    const GemmStep& s = p.step[i];
    char name[64];
    if (s.kind == GK_ROWS16) snprintf(name, sizeof(name), "gemm_rows16_kernel<%d, %s>", s.form, tf[s.pair]);
    else if (s.kind == GK_TILE) snprintf(name, sizeof(name), "gemm_bf16_nt_kernel<%d, %d, %s, %s>", s.form, s.form, tf[s.ta], tf[s.tb]);
    else if (s.kind == GK_SKINNY) snprintf(name, sizeof(name), "gemm_skinny64_kernel<%s>", tf[s.mubuf]);
    else if (s.form == 27) snprintf(name, sizeof(name), "gemm_bt_drain_kernel<%s, %s, %s>", tf[s.gelu], tf[s.vt], tf[s.tail_rows > 0]);
    else snprintf(name, sizeof(name), "gemm_bt_kernel<%d, %s, %s, %d, %s, %s>", s.form == 20 || s.form == 26 ? 4 : s.form == 22 ? 2 : 3,
                  tf[s.pair], tf[s.ksplit > 1], s.form == 24 || s.form == 26 ? 2 : 0, tf[s.vt], tf[s.tail_rows > 0]);
    if (k < n) k += snprintf(buf + k, n - k, " | %s rows=%d+%d grid=%d,%d,%d slices=%d tail=%d%s%s", name, s.row0, s.rows, s.grid[0],
                  s.grid[1], s.grid[2], s.ksplit, s.tail_rows, s.kind == GK_TILE && s.mubuf ? " mubuf" : "", s.ksplit > 1 ? " +reduce" : "");
  }
}

}  // namespace u2
