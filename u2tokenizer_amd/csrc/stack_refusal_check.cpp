// Stand-alone check of the whole-stack decode step's refusal walk (decoder.hip: decoder_decode_stack; capi.hip: the decoding of the
// layer descriptors) and of the head's (decode_head, decoder_decode_stack_head; u2tok_decode_head_desc), meant to be built with the host code under AddressSanitizer and UBSan (make stack_refusal_check) and run on a
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
  // ---- faults that only a launcher's own check sees (the step's own refusals pass them): the whole-stack step and the per-layer
  // second half, per sequence and batched, answer from the walk that precedes their first launch.  (Before the per-layer entries
  // walked twice, u2tok_decoder_decode_post answered these from a launch -- run once on that commit, without a GPU: -2, U2TOK_ERR_LAUNCH,
  // for every one of them but the scale of 0 with `batched`, which the batched attention, the first launcher, refused itself.)
  {
    char* Pc = mem;
    const size_t lneed = u2tok_decoder_decode_workspace_bytes(&cfg[0], T);
    auto everywhere = [&](const char* what) {
      expect(what, call(L, n, need, 0), U2TOK_ERR_ARG);
      expect(what, call(L, n, need, 1), U2TOK_ERR_ARG);
      for (int batched = 0; batched < 2; ++batched)
        expect(what, u2tok_decoder_decode_post(&cfg[1], &lay[1], P, P, P, P, T, 256 * 64, batched, nullptr, P, P, lneed, nullptr), U2TOK_ERR_ARG);
    };
    lay[1].Wdown = Pc + 8;
    everywhere("16-bit Wdown 8 bytes off alignment");
    lay[1].Wdown = P;
    lay[1].Wo = Pc + 8;
    everywhere("16-bit Wo 8 bytes off alignment");
    lay[1].Wo = P;
    lay[1].bgu = P;  // a gate|up bias: the product un-paired, SwiGLU a launch of its own, the down product behind it
    lay[1].Wdown = Pc + 8;
    everywhere("un-paired gate|up, Wdown 8 bytes off alignment");
    lay[1].Wdown = P;
    lay[1].bgu = nullptr;
    cfg[1].scale = 0.f;
    everywhere("a scale of 0");
    cfg[1].scale = 0.125f;
  }
  expect("workspace bytes of no layers", (long long)u2tok_decoder_decode_stack_workspace_bytes(L, 0), 0);
  expect("workspace bytes of null layers", (long long)u2tok_decoder_decode_stack_workspace_bytes(nullptr, n), 0);
  std::vector<u2tok_decode_stack_layer> many(64, L[0]);
  many[63].layer = nullptr;
  expect("64 layers, the last one bad", call(many.data(), 64, u2tok_decoder_decode_stack_workspace_bytes(L, 1), 0), U2TOK_ERR_ARG);
  // ---- the head of the step (u2tok_decode_head) and the step with the head (u2tok_decoder_decode_stack_head): the head's refusals
  // come from the check-only pass that follows the layers' walk, so a good stack with a bad head launches nothing either
  constexpr int V = 1000;
  float* LG = reinterpret_cast<float*>(mem);
  const u2tok_decode_head_desc good{P, P, nullptr, E, V, 0, 1e-6f, 0, 0};
  const size_t hneed = u2tok_decode_head_workspace_bytes(B, E);
  expect("head workspace bytes", (long long)hneed, 1024);
  expect("head workspace bytes of no rows", (long long)u2tok_decode_head_workspace_bytes(0, E), 0);
  expect("head workspace bytes of 65 rows", (long long)u2tok_decode_head_workspace_bytes(65, E), 0);
  const size_t sneed = u2tok_decoder_decode_stack_head_workspace_bytes(L, n, &good);
  expect("stack + head workspace bytes", (long long)sneed, (long long)(need + hneed));
  expect("stack + head workspace bytes of a null head", (long long)u2tok_decoder_decode_stack_head_workspace_bytes(L, n, nullptr), 0);
  struct HeadCase { const char* what; u2tok_decode_head_desc h; int64_t ldx, ldl; int rows; void* ws; size_t short_by; int want; };  // (both entries)
  auto with = [&](auto edit) { u2tok_decode_head_desc h = good; edit(h); return h; };
  char* Pc = mem;
  const HeadCase cases[] = {
      {"V = 1", with([](u2tok_decode_head_desc& h) { h.V = 1; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"null W", with([](u2tok_decode_head_desc& h) { h.W = nullptr; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"null norm weight", with([](u2tok_decode_head_desc& h) { h.w_norm = nullptr; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"misaligned W", with([&](u2tok_decode_head_desc& h) { h.W = Pc + 8; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"unknown form", with([](u2tok_decode_head_desc& h) { h.wform = 3; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"e4m3 without scales", with([](u2tok_decode_head_desc& h) { h.wform = 1; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"e2m1 without scales", with([](u2tok_decode_head_desc& h) { h.wform = 2; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"e4m3 with a misaligned scale", with([&](u2tok_decode_head_desc& h) { h.wform = 1; h.scale = Pc + 2; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"e2m1 with a short scale row", with([&](u2tok_decode_head_desc& h) { h.wform = 2; h.scale = Pc; h.lds = E / 32 - 1; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"a weight row shorter than E", with([](u2tok_decode_head_desc& h) { h.ldw = E - 8; }), E, V, B, P, 0, U2TOK_ERR_ARG},
      {"logits rows shorter than V", good, E, V - 1, B, P, 0, U2TOK_ERR_ARG},
      {"misaligned workspace", good, E, V, B, Pc + 8, 0, U2TOK_ERR_ARG},
      {"null workspace", good, E, V, B, nullptr, 0, U2TOK_ERR_ARG},
      {"short workspace", good, E, V, B, P, 1, U2TOK_ERR_WORKSPACE},
  };
  for (const HeadCase& c : cases) {
    expect(c.what, u2tok_decode_head(&c.h, P, c.ldx, c.rows, LG, c.ldl, c.ws, hneed - c.short_by, nullptr), c.want);
    expect(c.what, u2tok_decoder_decode_stack_head(L, n, P, P, P, 1, 64, 0, nullptr, 0, P, &c.h, LG, c.ldl, c.ws, sneed - c.short_by, nullptr),
           c.want);
  }
  // (shapes that are the standalone entry's alone)
  const u2tok_decode_head_desc e192 = with([&](u2tok_decode_head_desc& h) { h.wform = 2; h.scale = Pc; h.E = 192; });
  const u2tok_decode_head_desc e96 = with([&](u2tok_decode_head_desc& h) { h.wform = 1; h.scale = Pc; h.E = 96; });
  const u2tok_decode_head_desc e512 = with([](u2tok_decode_head_desc& h) { h.E = 512; });
  expect("E % 128 != 0 with e2m1", u2tok_decode_head(&e192, P, 192, B, LG, V, P, 4096, nullptr), U2TOK_ERR_ARG);
  expect("E % 64 != 0 with e4m3", u2tok_decode_head(&e96, P, 96, B, LG, V, P, 4096, nullptr), U2TOK_ERR_ARG);
  expect("x rows shorter than E", u2tok_decode_head(&good, P, E - 8, B, LG, V, P, hneed, nullptr), U2TOK_ERR_ARG);
  expect("65 rows", u2tok_decode_head(&good, P, E, 65, LG, V, P, 1 << 20, nullptr), U2TOK_ERR_ARG);
  expect("no rows", u2tok_decode_head(&good, P, E, 0, LG, V, P, hneed, nullptr), U2TOK_ERR_ARG);
  expect("null head", u2tok_decode_head(nullptr, P, E, B, LG, V, P, hneed, nullptr), U2TOK_ERR_ARG);
  expect("null x", u2tok_decode_head(&good, nullptr, E, B, LG, V, P, hneed, nullptr), U2TOK_ERR_ARG);
  expect("null logits", u2tok_decode_head(&good, P, E, B, nullptr, V, P, hneed, nullptr), U2TOK_ERR_ARG);
  // the joint call: the head's hidden size is the layers', a bad layer is still refused, a null head too
  auto joint = [&](const u2tok_decode_head_desc* h, size_t bytes) {
    return u2tok_decoder_decode_stack_head(L, n, P, P, P, 1, 64, 0, nullptr, 0, P, h, LG, V, P, bytes, nullptr);
  };
  expect("joint: null head", joint(nullptr, sneed), U2TOK_ERR_ARG);
  expect("joint: another hidden size", joint(&e512, sneed), U2TOK_ERR_ARG);
  expect("joint: room for the stack but not for the head", joint(&good, need), U2TOK_ERR_WORKSPACE);
  expect("joint: no room for the stack", joint(&good, need - 1), U2TOK_ERR_WORKSPACE);
  lay[2].Wdown = nullptr;
  expect("joint: layer 2 Wdown null", joint(&good, sneed), U2TOK_ERR_ARG);
  lay[2].Wdown = P;
  lay[0].w_in_norm = nullptr;
  expect("joint: layer 0 input norm null", joint(&good, sneed), U2TOK_ERR_ARG);
  lay[0].w_in_norm = P;
  // ---- the same two entries on an e4m3 KV cache (u2tok_decoder_decode_stack_kv8, u2tok_decoder_decode_stack_head_kv8): the walk
  // is the 16-bit one over layers whose first half appends codes (u2tok_qk_norm_rope_kv8's refusals) and whose second half attends
  // over them (u2tok_decode_attention_kv8's); every refusal below comes from the check walk, with and without the head behind it
  {
    constexpr int n8 = 2, CAP = 256;
    float* F = reinterpret_cast<float*>(mem);
    u2tok_decode_stack_layer_kv8 L8[n8];
    for (int i = 0; i < n8; ++i) L8[i] = u2tok_decode_stack_layer_kv8{&cfg[i], &lay[i], P, P, F, F, CAP, T - 1, 0, T};
    const size_t need8 = u2tok_decoder_decode_stack_kv8_workspace_bytes(L8, n8);
    expect("kv8: workspace bytes are the 16-bit step's", (long long)need8, (long long)u2tok_decoder_decode_stack_workspace_bytes(L, n8));
    const size_t sneed8 = u2tok_decoder_decode_stack_head_kv8_workspace_bytes(L8, n8, &good);
    expect("kv8: stack + head workspace bytes", (long long)sneed8, (long long)(need8 + hneed));
    expect("kv8: workspace bytes of no layers", (long long)u2tok_decoder_decode_stack_kv8_workspace_bytes(L8, 0), 0);
    expect("kv8: workspace bytes of null layers", (long long)u2tok_decoder_decode_stack_kv8_workspace_bytes(nullptr, n8), 0);
    expect("kv8: stack + head workspace bytes of a null head", (long long)u2tok_decoder_decode_stack_head_kv8_workspace_bytes(L8, n8, nullptr), 0);
    auto both = [&](const char* what, int want, size_t cut = 0) {
      for (int tail = 0; tail < 2; ++tail) {
        expect(what, u2tok_decoder_decode_stack_kv8(L8, n8, P, P, P, 1, 64, nullptr, P, 1e-6f, tail, P, P, need8 - cut, nullptr), want);
        expect(what, u2tok_decoder_decode_stack_head_kv8(L8, n8, P, P, P, 1, 64, nullptr, tail, P, &good, LG, V, P, sneed8 - cut, nullptr), want);
      }
    };
    L8[1].k_scales = nullptr;
    both("kv8: layer 1 with a null scale buffer", U2TOK_ERR_ARG);
    L8[1].k_scales = F;
    L8[1].v_codes = nullptr;
    both("kv8: layer 1 with a null code buffer", U2TOK_ERR_ARG);
    L8[1].v_codes = P;
    L8[1].k_codes = Pc + 8;
    both("kv8: codes 8 bytes off alignment", U2TOK_ERR_ARG);
    L8[1].k_codes = P;
    L8[1].v_scales = reinterpret_cast<float*>(Pc + 2);
    both("kv8: scales 2 bytes off alignment", U2TOK_ERR_ARG);
    L8[1].v_scales = F;
    L8[1].capacity = T - 1;
    both("kv8: s_off == capacity", U2TOK_ERR_ARG);
    L8[1].capacity = 1 << 25;
    both("kv8: capacity * D >= 2^31", U2TOK_ERR_ARG);
    L8[1].capacity = CAP;
    L8[1].k_first = 1;
    both("kv8: T != s_off - k_first + 1", U2TOK_ERR_ARG);
    L8[1].k_first = -1;
    both("kv8: a negative first position", U2TOK_ERR_ARG);
    L8[1].k_first = 0;
    lay[1].Wo = Pc + 8;
    both("kv8: 16-bit Wo 8 bytes off alignment behind a good layer 1 of 2", U2TOK_ERR_ARG);
    lay[1].Wo = P;
    cfg[1].Hq = 34;
    expect("kv8: 17 query heads per kv head",
           u2tok_decoder_decode_stack_kv8(L8, n8, P, P, P, 1, 64, nullptr, P, 1e-6f, 0, P, P, (size_t)1 << 30, nullptr), U2TOK_ERR_ARG);
    cfg[1].Hq = 4;
    both("kv8: short workspace", U2TOK_ERR_WORKSPACE, 1);
    expect("kv8: null layers", u2tok_decoder_decode_stack_kv8(nullptr, n8, P, P, P, 1, 64, nullptr, P, 1e-6f, 0, P, P, need8, nullptr), U2TOK_ERR_ARG);
    expect("kv8: joint with a null head",
           u2tok_decoder_decode_stack_head_kv8(L8, n8, P, P, P, 1, 64, nullptr, 0, P, nullptr, LG, V, P, sneed8, nullptr), U2TOK_ERR_ARG);
    expect("kv8: joint with room for the stack but not for the head",
           u2tok_decoder_decode_stack_head_kv8(L8, n8, P, P, P, 1, 64, nullptr, 0, P, &good, LG, V, P, need8, nullptr), U2TOK_ERR_WORKSPACE);
    // the rotary entry with the quantising append, by itself
    auto rope8 = [&](void* kc, float* ks, int S, int cap, int s_off) {
      return u2tok_qk_norm_rope_kv8(P, nullptr, nullptr, P, P, 1, 6, 4, 2, 64, 512, 64, 1e-6f, kc, P, ks, F, S, cap, s_off, nullptr);
    };
    expect("rope kv8: null codes", rope8(nullptr, F, 3, 16, 0), U2TOK_ERR_ARG);
    expect("rope kv8: null scales", rope8(P, nullptr, 3, 16, 0), U2TOK_ERR_ARG);
    expect("rope kv8: misaligned codes", rope8(Pc + 8, F, 3, 16, 0), U2TOK_ERR_ARG);
    expect("rope kv8: s_off + S > capacity", rope8(P, F, 3, 16, 14), U2TOK_ERR_ARG);
    expect("rope kv8: s_off + S overflows", rope8(P, F, 3, 16, 0x7fffffff), U2TOK_ERR_ARG);
    expect("rope kv8: rows not a multiple of S", rope8(P, F, 4, 16, 0), U2TOK_ERR_ARG);
    // the per-layer second half keeps its quantising launch: no rows, no call
    expect("post_kv8: null new rows",
           u2tok_decoder_decode_post_kv8(&cfg[0], &lay[0], P, P, nullptr, nullptr, P, P, F, F, CAP, 0, T - 1, nullptr, P, P,
                                         u2tok_decoder_decode_workspace_bytes(&cfg[0], T), nullptr),
           U2TOK_ERR_ARG);
  }
  if (failures == 0) std::printf("stack_refusal_check: ok\n");
  return failures != 0;
}
