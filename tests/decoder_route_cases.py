"""The cases of tests/test_gpu_decoder_route_bits.py: every host route of the decoder layers (prefill, continued prefill, decode
step, training; u2tokenizer_amd/prefill.py) on two-layer decoders, pinned BIT FOR BIT in tests/golden/decoder_route_bits.json
(the e2m1 decode step's in tests/golden/decoder_route_bits_fp4.json; the routes over the kinds of cache layer -- FP8 KV cache,
whole-stack step, head -- in tests/golden/decoder_route_bits_cache.json): per
case the SHA-256 of each call's last hidden state, of every layer's cached keys and values, of the training cases' gradients, and
the deltas of the route counters -- the route taken as well as the numbers.  Importable without a GPU (the host half of the test
checks the case list and the inputs).

Only the public surface is used -- the keywords of `enable_fused_prefill`, the counter dicts, u2tokenizer_amd.lora, transformers --
so that the same file runs against the commit that recorded the fixture and against every later one.

Models (2 layers each): Q = Qwen3, hidden 256, inter 512, 4 query / 2 kv heads of 64; L = Llama, hidden 256, inter 512, 2 / 1 heads
of 128 with attention and MLP biases (no head norm, the unfused gate|up branch); P = Phi-3, hidden 384, inter 512, 4 / 4 heads of
96, sliding_window 16.  A prefill has 70 positions (two 64-key tiles, the second ragged), a continuation 9, then 3 decode steps;
all inputs are seeded `inputs_embeds`, the decode steps (B, 1, E), so that lm_head stays out.

`python tests/decoder_route_cases.py --record --commit HASH [--fp4 | --cache] [--out FILE]` runs every case of one fixture on the GPU and writes the fixture; the test
itself only ever reads it."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch

FIXTURE = Path(__file__).resolve().parent / "golden" / "decoder_route_bits.json"
S0, CHUNK, STEPS, WINDOW = 70, 9, 3, 16
bf, f16 = torch.bfloat16, torch.float16
LORA_TARGETS = ("q_proj", "v_proj", "o_proj", "gate_proj", "down_proj")


def _case(model, B=2, dtype=bf, flags=None, cache="dynamic", S=S0, chunk=0, steps=0, left=None, right=None, lora=None, off=None,
          train=False, expect=()):
    """model: Q / L / P.  cache: None, "dynamic" (an empty DynamicCache: the fused prefill puts its append-in-place layers there),
    "config" (DynamicCache(config=...): sliding layers for P) or "stock" (a DynamicCache the STOCK forward filled with the prefill:
    DynamicLayer, the dense `update` path).  left / right: pads per sequence.  lora: the wrapped projections' names; off: {name:
    flag} wrappers that get `merged` / `disable_adapters` set.  expect: counters that must have moved (the host half reads them
    off the fixture)."""
    return dict(model=model, B=B, dtype=dtype, flags=flags or {}, cache=cache, S=S, chunk=chunk, steps=steps, left=left, right=right,
                lora=lora, off=off or {}, train=train, expect=tuple(expect))


CASES = {
    # a / b / c: Qwen3 prefill without a cache, into an append-in-place cache + decode, decode on a stock-filled cache
    "a-Q-prefill": _case("Q", cache=None, expect=("stats.prefill",)),
    "b-Q-prefill-decode": _case("Q", steps=STEPS, expect=("stats.prefill", "stats.decode")),
    "c-Q-decode-stock-cache": _case("Q", cache="stock", steps=STEPS, expect=("stats.decode",)),
    "d-L-prefill": _case("L", cache=None, expect=("stats.prefill",)),
    "d-L-prefill-decode": _case("L", steps=STEPS, expect=("stats.prefill", "stats.decode")),
    "e-Q-f16": _case("Q", dtype=f16, steps=STEPS, expect=("stats.prefill", "stats.decode")),
    "f-Q-left-padded": _case("Q", flags=dict(padded=True), left=(0, 5), steps=STEPS, expect=("stats.padded_prefill", "stats.padded_decode")),
    "f-Q-right-padded-prefill": _case("Q", flags=dict(padded=True), right=(0, 5), expect=("stats.padded_prefill",)),
    "g-Q-continued-append": _case("Q", flags=dict(continued=True), chunk=CHUNK, expect=("stats.prefill", "extend_stats.extend")),
    "g-Q-continued-stock-cache": _case("Q", flags=dict(continued=True), cache="stock", chunk=CHUNK, expect=("extend_stats.extend",)),
    "g-Q-continued-left-padded": _case("Q", flags=dict(continued=True, padded=True), left=(0, 5), chunk=CHUNK,
                                       expect=("stats.padded_prefill", "extend_stats.padded_extend")),
    "h-P-prefill-12": _case("P", S=12, cache=None, expect=("stats.prefill",)),
    "i-P-prefill-24-band": _case("P", S=24, flags=dict(continued=True), cache=None, expect=("extend_stats.extend",)),
    "j-P-decode-sliding": _case("P", S=12, cache="config", steps=STEPS, expect=("stats.prefill", "stats.decode")),
    "j-P-decode-append": _case("P", S=12, steps=STEPS, expect=("stats.prefill", "stats.decode")),
    # (... and with the window binding: 24 positions cached, the step attends over the last 16)
    "j-P-decode-sliding-past-window": _case("P", S=24, flags=dict(continued=True), cache="config", steps=STEPS,
                                            expect=("extend_stats.extend", "stats.decode")),
    "j-P-decode-append-past-window": _case("P", S=24, flags=dict(continued=True), steps=STEPS,
                                           expect=("extend_stats.extend", "stats.decode")),
    "k-P-continued-append": _case("P", S=24, flags=dict(continued=True), chunk=CHUNK, expect=("extend_stats.extend",)),
    "k-P-continued-sliding": _case("P", S=24, flags=dict(continued=True), cache="config", chunk=CHUNK, expect=("extend_stats.extend",)),
    "l-Q-fp8-decode": _case("Q", flags=dict(fp8_decode=True), steps=STEPS, expect=("stats.prefill", "w8_stats.decode")),
    "m-Q-wide": _case("Q", B=17, flags=dict(wide_decode=True), steps=2, expect=("stats.prefill", "wide_stats.decode")),
    "m-Q-wide-left-padded": _case("Q", B=17, flags=dict(wide_decode=True, padded=True), left=tuple((3 * b) % 7 for b in range(17)),
                                  steps=2, expect=("stats.padded_prefill", "wide_stats.padded_decode")),
    "n-Q-lora": _case("Q", flags=dict(lora=True, continued=True), lora=LORA_TARGETS, chunk=CHUNK, steps=STEPS,
                      expect=("lora_stats.prefill", "lora_stats.extend", "lora_stats.decode", "lora_stats.adapters")),
    "o-Q-lora-fp8": _case("Q", flags=dict(lora=True, fp8_decode=True), lora=LORA_TARGETS, steps=STEPS,
                          expect=("lora_stats.prefill", "lora_stats.decode", "w8_stats.decode")),
    "p-P-lora-packed-qkv": _case("P", S=12, flags=dict(lora=True, continued=True), lora=("qkv_proj",), chunk=CHUNK, steps=STEPS,
                                 expect=("lora_stats.prefill", "lora_stats.extend", "lora_stats.decode")),
    "q-Q-lora-merged-and-disabled": _case("Q", flags=dict(lora=True), lora=LORA_TARGETS, off={"q_proj": "merged", "o_proj": "disable_adapters"},
                                          steps=STEPS, expect=("lora_stats.prefill", "lora_stats.decode")),
    "r-Q-train": _case("Q", flags=dict(train=True), right=(0, 9), cache=None, train=True, expect=("train.stats.layers",)),
    "s-P-train-phi3": _case("P", S=12, flags=dict(train=True, train_phi3=True), cache=None, train=True, expect=("train.stats.layers",)),
    "t-Q-train-lora": _case("Q", flags=dict(train_lora=True), lora=LORA_TARGETS, cache=None, train=True,
                            expect=("train.stats.layers", "train.lora_stats.adapters")),
}
# The e2m1 decode step (fp4_decode), in a fixture of its own (recorded at the commit that brought the form).  `counters`: the exact
# deltas of w4_stats / w8_stats (layer calls: layers in that form x steps).  M = the three-layer stack of build_model.
FP4_CASES = {
    "u-Q-fp4-decode-B1": _case("Q", B=1, flags=dict(fp4_decode=True), steps=STEPS, expect=("stats.prefill", "w4_stats.decode")),
    "u-Q-fp4-decode-left-padded": _case("Q", flags=dict(fp4_decode=True, padded=True), left=(0, 5), steps=STEPS,
                                        expect=("stats.padded_prefill", "w4_stats.padded_decode")),
    "u-Q-fp4-wide": _case("Q", B=17, flags=dict(fp4_decode=True, wide_decode=True), steps=2,
                          expect=("stats.prefill", "w4_stats.decode", "wide_stats.decode")),
    "u-Q-fp4-lora": _case("Q", flags=dict(fp4_decode=True, lora=True), lora=LORA_TARGETS, steps=STEPS,
                          expect=("lora_stats.prefill", "lora_stats.decode", "w4_stats.decode")),
    "u-M-fp4-fp8-mixed-stack": _case("M", flags=dict(fp4_decode=True, fp8_decode=True), steps=STEPS,
                                     expect=("stats.prefill", "w4_stats.decode", "w8_stats.decode")),
}
FP4_COUNTERS = {
    "u-Q-fp4-decode-B1": {"w4_stats.decode": 2 * STEPS},
    "u-Q-fp4-decode-left-padded": {"w4_stats.padded_decode": 2 * STEPS},
    "u-Q-fp4-wide": {"w4_stats.decode": 2 * 2},
    "u-Q-fp4-lora": {"w4_stats.decode": 2 * STEPS},
    "u-M-fp4-fp8-mixed-stack": {"w4_stats.decode": STEPS, "w8_stats.decode": STEPS},   # one layer each; the third keeps 16 bits
}
MIXED_INTER = (256, 320, 288)   # model M: a multiple of 128 (e2m1), of 64 only (e4m3), of 32 only (the element type)
FIXTURE_FP4 = FIXTURE.with_name("decoder_route_bits_fp4.json")
# The routes over the kinds of cache layer -- the decode step and the continued prefill on an e4m3 cache (kv8, kv8_continued), the
# whole-stack step on either kind (stack_decode, stack_kv8) and the head -- in a third fixture, recorded before those routes were
# folded onto one cache-kind rule.  A `Kv8Layer`'s digests are of its codes and scales.  U = Q's sizes as a u2Qwen3ForCausalLM:
# the switches come from its config, every call goes through the causal LM and the digests are of its `logits`.
# mixed: after the prefill layer 1 of the cache is replaced by an append-in-place layer holding the same (dequantised) positions.
KV8, KV8X, STACK, STACK8 = dict(kv8=True), dict(kv8_continued=True), dict(stack_decode=True), dict(stack_kv8=True)
CACHE_CASES = {
    "v-Q-kv8-decode": _case("Q", flags=KV8, steps=STEPS, expect=("stats.prefill", "kv8_stats.decode")),
    "v-Q-kv8-decode-left-padded": _case("Q", flags=dict(KV8, padded=True), left=(0, 5), steps=STEPS,
                                        expect=("stats.padded_prefill", "kv8_stats.padded_decode")),
    "v-P-kv8-decode-past-window": _case("P", S=24, flags=dict(KV8, continued=True), steps=STEPS,
                                        expect=("extend_stats.extend", "kv8_stats.decode")),
    "v-Q-kv8-wide": _case("Q", B=17, flags=dict(KV8, wide_decode=True), steps=2, expect=("kv8_stats.decode", "wide_stats.decode")),
    "w-Q-kv8-continued": _case("Q", flags=KV8X, chunk=CHUNK, steps=STEPS,
                               expect=("stats.prefill", "kv8_extend_stats.extend", "kv8_stats.decode")),
    "w-Q-kv8-continued-left-padded": _case("Q", flags=dict(KV8X, padded=True), left=(0, 5), chunk=CHUNK, steps=STEPS,
                                           expect=("kv8_extend_stats.padded_extend", "kv8_stats.padded_decode")),
    "w-P-kv8-continued-window": _case("P", S=24, flags=KV8X, chunk=CHUNK, expect=("extend_stats.extend", "kv8_extend_stats.extend")),
    "x-Q-stack": _case("Q", flags=STACK, steps=STEPS, expect=("stack_stats.decode", "stats.decode")),
    "x-Q-stack-left-padded": _case("Q", flags=dict(STACK, padded=True), left=(0, 5), steps=STEPS,
                                   expect=("stack_stats.padded_decode", "stats.padded_decode")),
    "x-P-stack-past-window": _case("P", S=24, flags=dict(STACK, continued=True), steps=STEPS, expect=("stack_stats.decode",)),
    "x-Q-stack-fp8-lora": _case("Q", flags=dict(STACK, fp8_decode=True, lora=True), lora=LORA_TARGETS, steps=STEPS,
                                expect=("stack_stats.decode", "w8_stats.decode", "lora_stats.decode")),
    "x-M-stack-fp4-fp8": _case("M", flags=dict(STACK, fp4_decode=True, fp8_decode=True), steps=STEPS,
                               expect=("stack_stats.decode", "w4_stats.decode", "w8_stats.decode")),
    "y-Q-stack-kv8": _case("Q", flags=STACK8, steps=STEPS, expect=("stack_kv8_stats.decode", "stack_stats.decode", "kv8_stats.decode")),
    "y-Q-stack-kv8-left-padded": _case("Q", flags=dict(STACK8, padded=True), left=(0, 5), steps=STEPS,
                                       expect=("stack_kv8_stats.padded_decode", "kv8_stats.padded_decode")),
    "y-P-stack-kv8-past-window": _case("P", S=24, flags=dict(STACK8, continued=True), steps=STEPS,
                                       expect=("stack_kv8_stats.decode", "kv8_stats.decode")),
    "y-Q-stack-kv8-mixed-cache": dict(_case("Q", flags=STACK8, steps=STEPS, expect=("stats.decode", "kv8_stats.decode")), mixed=True),
    "z-U-head-elem": dict(_case("U", flags=dict(head=True), steps=STEPS, expect=("head_stats.head", "stack_stats.decode")), head_form="elem"),
    "z-U-head-fp8": dict(_case("U", flags=dict(head=True), steps=STEPS, expect=("head_stats.head", "stack_stats.decode")), head_form="fp8"),
    "z-U-head-elem-stack-kv8": dict(_case("U", flags=dict(STACK8, head=True), steps=STEPS,
                                          expect=("head_stats.head", "stack_kv8_stats.decode")), head_form="elem"),
}
# exact deltas: the mixed cache ran layer by layer (no whole-stack call: one e4m3 and one 16-bit layer per step); the head cases
# took the head at every step and the stock head for the prefill alone
CACHE_COUNTERS = {
    "y-Q-stack-kv8-mixed-cache": {"stats.prefill": 2, "stats.decode": 2 * STEPS, "kv8_stats.decode": STEPS},
    "y-Q-stack-kv8": {"stats.prefill": 2, "stats.decode": 2 * STEPS, "kv8_stats.decode": 2 * STEPS, "stack_stats.decode": STEPS,
                      "stack_kv8_stats.decode": STEPS},
    "z-U-head-elem": {"stats.prefill": 2, "stats.decode": 2 * STEPS, "stack_stats.decode": STEPS, "head_stats.head": STEPS,
                      "head_stats.fallback": 1},
}
FIXTURE_CACHE = FIXTURE.with_name("decoder_route_bits_cache.json")
FIXTURES = {FIXTURE: CASES, FIXTURE_FP4: FP4_CASES, FIXTURE_CACHE: CACHE_CASES}
ALL_CASES = {**CASES, **FP4_CASES, **CACHE_CASES}
# the test functions (a few seconds each): the cases by what they exercise
GROUPS = {
    "plain": ("a-Q-prefill", "b-Q-prefill-decode", "c-Q-decode-stock-cache", "d-L-prefill", "d-L-prefill-decode", "e-Q-f16"),
    "padded-continued": ("f-Q-left-padded", "f-Q-right-padded-prefill", "g-Q-continued-append", "g-Q-continued-stock-cache",
                         "g-Q-continued-left-padded"),
    "phi3": ("h-P-prefill-12", "i-P-prefill-24-band", "j-P-decode-sliding", "j-P-decode-append", "j-P-decode-sliding-past-window",
             "j-P-decode-append-past-window", "k-P-continued-append", "k-P-continued-sliding"),
    "fp8-wide": ("l-Q-fp8-decode", "m-Q-wide", "m-Q-wide-left-padded"),
    "lora": ("n-Q-lora", "o-Q-lora-fp8", "p-P-lora-packed-qkv", "q-Q-lora-merged-and-disabled"),
    "train": ("r-Q-train", "s-P-train-phi3", "t-Q-train-lora"),
}
FP4_GROUPS = {"fp4": tuple(FP4_CASES)}
CACHE_GROUPS = {name: tuple(c for c in CACHE_CASES if c[0] == letter)
                for name, letter in (("kv8", "v"), ("kv8-continued", "w"), ("stack", "x"), ("stack-kv8", "y"), ("head", "z"))}


def case_ids(fixture=FIXTURE):
    return list(FIXTURES[fixture])


# ------------------------------------------------------------------------------------------------------------------ the inputs
def build_model(kind):
    """The fp32 model on the CPU with seeded weights."""
    from transformers import LlamaConfig, LlamaForCausalLM, Phi3Config, Phi3ForCausalLM, Qwen3Config, Qwen3ForCausalLM
    from u2tokenizer_amd import synth
    common = dict(vocab_size=256, num_hidden_layers=2, intermediate_size=512, max_position_embeddings=512, tie_word_embeddings=False,
                  pad_token_id=0, bos_token_id=1, eos_token_id=2)
    if kind == "M":   # Qwen3 as Q with three layers whose MLPs have the inner sizes of MIXED_INTER: a stack of three weight forms
        from transformers.models.qwen3.modeling_qwen3 import Qwen3MLP
        cfg = Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, **{**common, "num_hidden_layers": 3})
        m = Qwen3ForCausalLM(cfg)
        for layer, inter in zip(m.model.layers, MIXED_INTER):
            layer.mlp = Qwen3MLP(Qwen3Config(**{**cfg.to_dict(), "intermediate_size": inter}))
    elif kind == "U":   # Q's sizes as the project's causal LM (the head route lives in its forward)
        from u2tokenizer_amd import language_model as LM
        m = LM.u2Qwen3ForCausalLM(LM.u2Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, **common))
    elif kind == "Q":
        m = Qwen3ForCausalLM(Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, **common))
    elif kind == "L":
        m = LlamaForCausalLM(LlamaConfig(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                                         attention_bias=True, mlp_bias=True, **common))
    else:
        m = Phi3ForCausalLM(Phi3Config(hidden_size=384, num_attention_heads=4, num_key_value_heads=4, sliding_window=WINDOW, **common))
    synth.fill_module_(m, seed=29, prefix="decoder.")
    return m.eval()


def wrap(m, c):
    """The case's adapters: rank 16, fp32 A / B, no dropout, seeded and non-zero; then the `off` flags."""
    from u2tokenizer_amd import synth
    from u2tokenizer_amd.lora import LoRALinear, add_lora
    add_lora(m, r=16, alpha=32, dropout=0.0, target_modules=c["lora"], adapter_dtype=torch.float32)
    for name, mod in m.named_modules():
        if isinstance(mod, LoRALinear):
            A, B = mod.lora_A["default"].weight, mod.lora_B["default"].weight
            with torch.no_grad():
                A.copy_(synth.synth_tensor(name + ".lora_A.weight", A.shape, 31).to(A.device))
                B.copy_(0.3 * synth.synth_tensor(name + ".lora_B.weight", B.shape, 31).to(B.device))
            flag = c["off"].get(name.rsplit(".", 1)[-1])
            if flag:
                setattr(mod, flag, True)
    return m


def embeds(c, name, n):
    """Seeded (B, n, E) inputs of one call."""
    from u2tokenizer_amd import synth
    E = 384 if c["model"] == "P" else 256
    return 0.5 * synth.synth_tensor(name, (c["B"], n, E), 37)


def mask(c, n):
    """The 2-D attention mask of a call that sees n keys in all (None: no padding in the case)."""
    if c["left"] is None and c["right"] is None:
        return None
    m = torch.ones(c["B"], n, dtype=torch.int64)
    for b in range(c["B"]):
        if c["left"] is not None:
            m[b, :c["left"][b]] = 0
        else:
            m[b, c["S"] - c["right"][b]:c["S"]] = 0
    return m


# ------------------------------------------------------------------------------------------------------------------ running a case
def _sha(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.uint8:   # (the codes of a `Kv8Layer`)
        return hashlib.sha256(t.numpy().tobytes()).hexdigest()
    return hashlib.sha256(t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().tobytes()).hexdigest()


def _counters():
    from u2tokenizer_amd import decoder_train, prefill
    dicts = {"stats": prefill.stats, "extend_stats": prefill.extend_stats, "w8_stats": prefill.w8_stats, "w4_stats": prefill.w4_stats,
             "wide_stats": prefill.wide_stats, "stack_stats": prefill.stack_stats, "head_stats": prefill.head_stats,
             "kv8_stats": prefill.kv8_stats, "kv8_extend_stats": prefill.kv8_extend_stats, "stack_kv8_stats": prefill.stack_kv8_stats,
             "lora_stats": prefill.lora_stats, "train.stats": decoder_train.stats, "train.lora_stats": decoder_train.lora_stats}
    return {f"{n}.{k}": v for n, d in dicts.items() for k, v in d.items()}


def run_case(cid):
    """One case on the GPU -> {"digests": {what: SHA-256}, "stats": {counter: delta}}"""
    from transformers.cache_utils import DynamicCache
    from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill
    c = ALL_CASES[cid]
    dev = "cuda"
    m = build_model(c["model"]).to(c["dtype"]).to(dev)
    if c["lora"]:
        wrap(m, c)
    dig = {}
    before = _counters()
    kw = lambda n: {} if mask(c, n) is None else {"attention_mask": mask(c, n).to(dev)}   # noqa: E731
    if c["train"]:
        m.train()
        enable_fused_prefill(m, **c["flags"])
        x = embeds(c, "x_train", c["S"]).to(c["dtype"]).to(dev).requires_grad_(True)
        with torch.enable_grad():
            out = m.model(inputs_embeds=x, use_cache=False, **kw(c["S"])).last_hidden_state
            out.backward(embeds(c, "cotangent", c["S"]).to(c["dtype"]).to(dev))
        dig["out"] = _sha(out)
        dig["grad.x"] = _sha(x.grad)
        for name, p in m.model.named_parameters():
            if p.grad is not None and (name.startswith("layers.0.") or ".lora_" in name):
                dig["grad." + name] = _sha(p.grad)
    else:
        S, B = c["S"], c["B"]
        cache = None if c["cache"] is None else DynamicCache(config=m.config) if c["cache"] == "config" else DynamicCache()
        x = embeds(c, "x_prefill", S).to(c["dtype"]).to(dev)
        call = lambda **k: m.model(**k).last_hidden_state   # noqa: E731
        if c["model"] == "U":   # (the causal LM sets the switches from its config at its first call)
            from u2tokenizer_amd.prefill import SWITCHES
            for s in SWITCHES:
                if c["flags"].get(s.kw):
                    setattr(m.config, s.config, True)
            m.config.u2_fused_head_form = c["head_form"]
            call = lambda **k: m(**k).logits   # noqa: E731
        with torch.no_grad():
            if c["model"] == "U":
                dig["prefill"] = _sha(call(inputs_embeds=x, past_key_values=cache, use_cache=True, **kw(S)))
            elif c["cache"] == "stock":   # (the stock layers fill the cache; its bits are not what the fixture is about)
                m.model(inputs_embeds=x, past_key_values=cache, use_cache=True, **kw(S))
                enable_fused_prefill(m, **c["flags"])
            else:
                enable_fused_prefill(m, **c["flags"])
                dig["prefill"] = _sha(m.model(inputs_embeds=x, past_key_values=cache, use_cache=cache is not None, **kw(S)).last_hidden_state)
            T = S
            if c.get("mixed"):
                from u2tokenizer_amd import prefill
                lay = prefill._append_layer_class()()
                lay.update(cache.layers[1].keys, cache.layers[1].values)
                cache.layers[1] = lay
            if c["chunk"]:
                xc = embeds(c, "x_chunk", c["chunk"]).to(c["dtype"]).to(dev)
                T += c["chunk"]
                dig["chunk"] = _sha(call(inputs_embeds=xc, past_key_values=cache, use_cache=True, **kw(T)))
            for t in range(c["steps"]):
                xs = embeds(c, f"x_step{t}", 1).to(c["dtype"]).to(dev)
                T += 1
                dig[f"step{t}"] = _sha(call(inputs_embeds=xs, past_key_values=cache, use_cache=True, **kw(T)))
            if cache is not None:
                for i, lay in enumerate(cache.layers):
                    codes = lay.codes() if hasattr(lay, "codes") else None
                    if codes is not None:   # a `Kv8Layer`: what it holds -- K codes, V codes, K scales, V scales
                        assert codes[0].shape[0] == B and codes[0].shape[2] == cache.get_seq_length(i) == T, (cid, i, T)
                        dig[f"keys{i}"], dig[f"values{i}"], dig[f"key_scales{i}"], dig[f"value_scales{i}"] = map(_sha, codes)
                        continue
                    assert lay.keys.shape[0] == B and cache.get_seq_length(i) == T, (cid, i, T)
                    dig[f"keys{i}"], dig[f"values{i}"] = _sha(lay.keys), _sha(lay.values)
    torch.cuda.synchronize()
    disable_fused_prefill(m)
    after = _counters()
    return {"digests": dig, "stats": {k: after[k] - before[k] for k in after if after[k] != before[k]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="run every case on the GPU and write the fixture")
    ap.add_argument("--commit", default="", help="the commit whose Python is recorded (written into the file)")
    ap.add_argument("--fp4", action="store_true", help="the cases of decoder_route_bits_fp4.json instead")
    ap.add_argument("--cache", action="store_true", help="the cases of decoder_route_bits_cache.json instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fixture = FIXTURE_CACHE if a.cache else FIXTURE_FP4 if a.fp4 else FIXTURE
    a.out = a.out or str(fixture)
    if not a.record:
        print(f"{len(FIXTURES[fixture])} cases; --record writes their digests")
        return 0
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from u2tokenizer_amd import ops
    ops.device_check()
    cases = {}
    for cid in FIXTURES[fixture]:
        cases[cid] = run_case(cid)
        print(cid, cases[cid]["stats"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"recorded_at_commit": a.commit, "cases": cases}, indent=0, sort_keys=True) + "\n")
    print(f"wrote {len(cases)} cases to {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
