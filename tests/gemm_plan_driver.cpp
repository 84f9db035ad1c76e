// CPU driver of tests/test_gemm_plan.py: reads one product per line ("key=value ..."), validates and plans it with
// u2tokenizer_amd/csrc/gemm_plan.hip and prints "<status><plan>" (gemm_plan_format).  Pointers are fake addresses: the plan
// reads their alignment only.
//   keys: M N K nz lda ldb ldc ldr sAb sBb sCb nsplit flags (GEMM_* bits) ktile (B K-tile-major) vt=n0,rows
//         a_off c_off bias_off r_off (bytes added to the 4 KB-aligned fake pointers) scratch (bytes) and any Options field below
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sstream>
#include <iostream>
#include "kernels.h"

using namespace u2;

static int parse_case(const std::string& line, GemmDesc& d, Options& o, size_t& scratch) {
  d = GemmDesc{};
  o = Options{};
  scratch = 0;
  d.nz = 1;
  int64_t a_off = 0, c_off = 0, bias_off = 0, r_off = 0, lda = -1, ldb = -1, ldc = -1, ldr = -1;
  int ktile = 0, vt_n0 = 0, vt_rows = 0;
  std::istringstream in(line);
  std::string kv;
  while (in >> kv) {
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return -1;
    const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
    const long long x = strtoll(v.c_str(), nullptr, 0);
    if (k == "M") d.M = (int)x; else if (k == "N") d.N = (int)x; else if (k == "K") d.K = (int)x;
    else if (k == "nz") d.nz = (int)x; else if (k == "nsplit") d.nsplit = (int)x; else if (k == "flags") d.flags = (int)x;
    else if (k == "lda") lda = x; else if (k == "ldb") ldb = x; else if (k == "ldc") ldc = x; else if (k == "ldr") ldr = x;
    else if (k == "sAb") d.sAb = x; else if (k == "sBb") d.sBb = x; else if (k == "sCb") d.sCb = x;
    else if (k == "a_off") a_off = x; else if (k == "c_off") c_off = x; else if (k == "bias_off") bias_off = x; else if (k == "r_off") r_off = x;
    else if (k == "ktile") ktile = (int)x; else if (k == "scratch") scratch = (size_t)x;
    else if (k == "vt") { vt_n0 = (int)x; vt_rows = atoi(v.c_str() + v.find(',') + 1); }
    else if (k == "gemm_tile") o.gemm_tile = (int)x; else if (k == "gemm_mubuf") o.gemm_mubuf = (int)x;
    else if (k == "gemm_splitk") o.gemm_splitk = (int)x; else if (k == "gemm_big") o.gemm_big = (int)x;
    else if (k == "gemm_big_grid") o.gemm_big_grid = (int)x; else if (k == "gemm_big_splitk") o.gemm_big_splitk = (int)x;
    else if (k == "gemm_big_drain") o.gemm_big_drain = (int)x; else if (k == "gemm_skinny") o.gemm_skinny = (int)x;
    else if (k == "gemm_tail_fused") o.gemm_tail_fused = (int)x;
    else return -1;
  }
  const bool ta = d.flags & GEMM_A_KMAJOR, tb = d.flags & GEMM_B_KMAJOR;
  d.lda = lda >= 0 ? lda : ta ? d.M : d.K;
  d.ldb = ldb >= 0 ? ldb : tb ? d.N : d.K;
  d.ldc = ldc >= 0 ? ldc : (d.flags & GEMM_SWIGLU) ? d.N / 2 : d.N;
  d.ldr = ldr >= 0 ? ldr : d.N;
  if (ktile) { d.ldb = 64; d.ldbk = (int64_t)d.N * 64; }
  d.A = reinterpret_cast<const bf16_t*>(0x10000000 + a_off);
  d.B = reinterpret_cast<const bf16_t*>(0x20000000);
  d.C = reinterpret_cast<void*>(0x30000000 + c_off);
  if (d.flags & (GEMM_BIAS_N | GEMM_BIAS_M)) d.bias = reinterpret_cast<const bf16_t*>(0x40000000 + bias_off);
  if (d.flags & GEMM_RESIDUAL) d.R = reinterpret_cast<const bf16_t*>(0x50000000 + r_off);
  if (vt_rows) {
    d.vt = reinterpret_cast<bf16_t*>(0x60000000);
    d.vt_n0 = vt_n0;
    d.vt_rows = vt_rows;
    d.vt_ld = vt_rows;
    d.vt_bs = (int64_t)(d.N - vt_n0) * vt_rows;
  }
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    GemmDesc d;
    Options o;
    size_t scratch;
    if (parse_case(line, d, o, scratch) != 0) {
      printf("bad case: %s\n", line.c_str());
      return 1;
    }
    GemmPlan p;
    int e = gemm_validate(d);
    if (e == U2_OK) e = gemm_plan(d, o, scratch, p);
    char buf[1024] = "";
    if (e == U2_OK) gemm_plan_format(p, buf, sizeof(buf));
    printf("%d%s\n", e, buf);
  }
  return 0;
}
