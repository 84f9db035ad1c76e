// Stand-alone check of the whole-stack decode step's refusal walk (decoder.hip: decoder_decode_stack; capi.hip: the decoding of the
// layer descriptors), meant to be built with the host code under AddressSanitizer and UBSan (make stack_refusal_check) and run on a
// CPU: every call below must return its error code from the walk that precedes the first launch -- without a GPU a launch would not
// return one of these codes -- and must not read or write anything but the descriptors.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../include/u2tok.h"

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }  // (the HIP runtime's own start-up allocations)

static int failures = 0;
static void expect(const char* what, long long got, long long want) {
  if (got != want) {
    std::printf("FAIL %s: got %lld, expected %lld\n", what, got, want);
    ++failures;
  }
}

int main() {
  constexpr int n = 3, B = 2, E = 256, T = 18;
  alignas(256) static char mem[4096];  // addresses the walk may compare and align-check; nothing dereferences them
  void* P = mem;
  u2tok_decode_config cfg[n];
  u2tok_decode_layer lay[n];
  u2tok_decode_stack_layer L[n];
  for (int i = 0; i < n; ++i) {
    cfg[i] = u2tok_decode_config{B, E, 4, 2, 64, 512, 1e-6f, 1e-6f, 0.125f, 0};
    lay[i] = u2tok_decode_layer{P, P, nullptr, nullptr, nullptr, P, nullptr, P, P, nullptr, P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    L[i] = u2tok_decode_stack_layer{&cfg[i], &lay[i], P, P, 256 * 64, T - 1, 0, T};
  }
  const size_t need = u2tok_decoder_decode_stack_workspace_bytes(L, n);
  expect("workspace bytes > per-layer + two hidden rows", need >= u2tok_decoder_decode_workspace_bytes(&cfg[0], T) + 2 * B * E * 2, 1);
  auto call = [&](const u2tok_decode_stack_layer* layers, int count, size_t bytes, int tail) {
    return u2tok_decoder_decode_stack(layers, count, P, P, P, 1, 64, 0, nullptr, P, 1e-6f, tail, P, P, bytes, nullptr);
  };
  for (int tail = 0; tail < 2; ++tail) {
    lay[2].Wdown = nullptr;  // the last layer's second half
    expect("layer 2 Wdown null", call(L, n, need, tail), U2TOK_ERR_ARG);
    lay[2].Wdown = P;
    expect("short workspace", call(L, n, need - 1, tail), U2TOK_ERR_WORKSPACE);
    expect("no layers", call(L, 0, need, tail), U2TOK_ERR_ARG);
    expect("null layers", call(nullptr, n, need, tail), U2TOK_ERR_ARG);
    L[1].layer = nullptr;
    expect("null descriptor", call(L, n, need, tail), U2TOK_ERR_ARG);
    L[1].layer = &lay[1];
    L[1].cfg = nullptr;
    expect("null config", call(L, n, need, tail), U2TOK_ERR_ARG);
    L[1].cfg = &cfg[1];
    L[2].k_cache = nullptr;
    expect("null cache buffer", call(L, n, need, tail), U2TOK_ERR_ARG);
    L[2].k_cache = P;
    L[1].kv_stride = (T - 1) * 64;
    expect("kv_stride without room for the row", call(L, n, need, tail), U2TOK_ERR_ARG);
    L[1].kv_stride = 256 * 64;
    L[0].T = T + 1;
    expect("reads past the step's row", call(L, n, need, tail), U2TOK_ERR_ARG);
    L[0].T = T;
    cfg[2].wform = 2;
    expect("e2m1 without block scales", call(L, n, need, tail), U2TOK_ERR_ARG);
    cfg[2].wform = 0;
    lay[1].scale_gu = reinterpret_cast<const float*>(P);
    expect("some of the four scales", call(L, n, need, tail), U2TOK_ERR_ARG);
    lay[1].scale_gu = nullptr;
    cfg[1].E = 512;
    expect("two hidden sizes", call(L, n, need, tail), U2TOK_ERR_ARG);
    cfg[1].E = E;
    u2tok_decode_lora lr{};
    lr.n_o = 2;  // more segments than the product takes
    lr.scratch = P;
    lr.scratch_bytes = sizeof(mem);
    lay[2].lora = &lr;
    expect("adapter count out of range", call(L, n, need, tail), U2TOK_ERR_ARG);
    lay[2].lora = nullptr;
  }
  expect("workspace bytes of no layers", (long long)u2tok_decoder_decode_stack_workspace_bytes(L, 0), 0);
  expect("workspace bytes of null layers", (long long)u2tok_decoder_decode_stack_workspace_bytes(nullptr, n), 0);
  std::vector<u2tok_decode_stack_layer> many(64, L[0]);
  many[63].layer = nullptr;
  expect("64 layers, the last one bad", call(many.data(), 64, u2tok_decoder_decode_stack_workspace_bytes(L, 1), 0), U2TOK_ERR_ARG);
  if (failures == 0) std::printf("stack_refusal_check: ok\n");
  return failures != 0;
}
