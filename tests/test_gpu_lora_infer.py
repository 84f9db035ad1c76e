"""GPU: LoRA-wrapped decoder layers on the no-grad routes (enable_fused_prefill(lora=True)): the prefill, the continued prefill and
the decode step with the adapters UNMERGED -- small Llama, Qwen3 and Phi-3 decoders (E = 512 / 768, two layers, every projection
wrapped with r = 16 and non-zero B, eval mode) against the same wrapped model in fp32 on the CPU, under the gate of
tests/test_gpu_prefill.py: no further from the fp32 model than 1.5 x the stock wrapped run of the element type is, + its EPS.  Each
case: prefill logits, the first and last layers' cached keys and values, four teacher-forced decode steps; the routes taken and the
adapters computed by counter; not the stock run's bits; and the adapters matter -- the same fused run with the adapters switched off
lies at least 10 x the gate from the reference.  Then what must give the bits of the unwrapped model's fused routes (disabled and
merged wrappers), the refresh of the cached 16-bit copies, and what must keep the stock forward bit for bit."""
import pytest
import torch

from test_gpu_lora_train import _wrap
from test_gpu_prefill import _err, _small
from test_gpu_w8 import _phi3
from u2tokenizer_amd import synth
from u2tokenizer_amd.lora import LoRALinear

pytestmark = pytest.mark.gpu
bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
D = "cuda"
EPS = {bf: 1e-3, f16: 1.5e-4}      # tests/test_gpu_prefill.py / tests/test_gpu_f16.py
NL, STEPS = 2, 4
BUILDS = {"llama": lambda: _small("llama", NL), "qwen3": lambda: _small("qwen3", NL), "phi3": lambda: _phi3(NL, 32)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    return _ops


def _wrapped(m, adapter_dtype=None, targets=None):
    """tests/test_gpu_lora_train.py's adapters (every projection, r = 16, B of the size of 0.7 x the base weight) with the wrapper's
    own nn.Dropout(0.05), in eval mode; targets: the others are unwrapped again, so the kept adapters have the values they have in
    the fully wrapped model"""
    _wrap(m, adapter_dtype=adapter_dtype, dropout=None)
    if targets is not None:
        for parent in list(m.modules()):
            for name, child in list(parent.named_children()):
                if isinstance(child, LoRALinear) and name not in targets:
                    setattr(parent, name, child.base_layer)
    return m.eval()


def _pair(kind, dt, adapter_dtype=None, targets=None, snap=False):
    """the fp32 wrapped model on the CPU and its copy in `dt` on the GPU (snap: decoder weights the e4m3 quantiser keeps exactly)"""
    m32, mg = BUILDS[kind](), BUILDS[kind]()
    if snap:
        from u2tokenizer_amd import ops as _ops
        _ops.snap_fp8_(m32.model.layers)
        mg.load_state_dict(m32.state_dict())
    mg = mg.to(dt).to(D)
    return _wrapped(m32, None, targets), _wrapped(mg, adapter_dtype, targets)


def _adapters(m, **attrs):
    n = 0
    for mod in m.modules():
        if isinstance(mod, LoRALinear):
            n += 1
            for k, v in attrs.items():
                setattr(mod, k, v)
    return n


def _run(m, x, xs, pads=None, chunk=0):
    """a prefill of x (chunk: its last `chunk` positions as a second call against the filled cache) and one decode step per position
    of xs, on the cache `generate` builds for the config; pads: left pads per sequence -> 2-D masks.  -> (logits per call -- the
    prefill's: last position --, [(keys, values) of the first and last layer after the prompt])"""
    from transformers.cache_utils import DynamicCache
    dev = x.device
    cache = DynamicCache(config=m.config)
    B, S, _ = x.shape
    mask = None
    if pads is not None:
        mask = torch.ones(B, S, dtype=torch.int64, device=dev)
        for b, p in enumerate(pads):
            mask[b, :p] = 0
    kw = lambda n: {} if mask is None else {"attention_mask": torch.cat([mask, torch.ones(B, n - S, dtype=torch.int64, device=dev)], 1)[:, :n]}  # noqa: E731
    with torch.no_grad():
        if chunk:
            m(inputs_embeds=x[:, :S - chunk], past_key_values=cache, use_cache=True, **kw(S - chunk))
            out = [m(inputs_embeds=x[:, S - chunk:], past_key_values=cache, use_cache=True, **kw(S)).logits[:, -1]]
        else:
            out = [m(inputs_embeds=x, past_key_values=cache, use_cache=True, **kw(S)).logits[:, -1]]
        kv = [(cache.layers[i].keys.clone(), cache.layers[i].values.clone()) for i in (0, NL - 1)]
        for t in range(xs.shape[1]):
            out.append(m(inputs_embeds=xs[:, t:t + 1], past_key_values=cache, use_cache=True, **kw(S + t + 1)).logits[:, -1])
    return out, kv


def _valid(t, pads):
    """cached keys / values (B, H, T, d) without the padded positions (whose values no route defines)"""
    if pads is None:
        return t.float().cpu().flatten()
    return torch.cat([t[b, :, p:].float().cpu().flatten() for b, p in enumerate(pads)])


def _gates(what, fused, stock, ref, pads, eps, base=None):
    """every call's logits and the prompt's keys / values of the first and last layer under the gate; returns the worst
    (base-only error) / gate over the logits when the base-only run is handed in"""
    (lf, kf), (ls, ks), (lr, kr) = fused, stock, ref
    worst_ratio = float("inf")
    for i, (a, s, r) in enumerate(zip(lf, ls, lr)):
        ef, es = _err(a.float().cpu(), r), _err(s.float().cpu(), r)
        print(f"{what}, call {i}: route {ef:.3e} stock {es:.3e}")
        assert torch.isfinite(a).all() and ef <= 1.5 * es + eps, (what, i, ef, es)
        assert not torch.equal(a, s), (what, i, "the stock run's bits")
        if base is not None:
            eb = _err(base[0][i].float().cpu(), r)
            worst_ratio = min(worst_ratio, eb / (1.5 * es + eps))
    for li in range(2):
        for j, name in enumerate(("keys", "values")):
            r = _valid(kr[li][j], pads)
            ef, es = _err(_valid(kf[li][j], pads), r), _err(_valid(ks[li][j], pads), r)
            assert ef <= 1.5 * es + eps, (what, name, li, ef, es)
    return worst_ratio


CASES = {
    # kind, B, S, element type, adapter dtype, targets, flags, pads, chunk
    "llama, B = 1": ("llama", 1, 37, bf, None, None, {}, None, 0),
    "qwen3, B = 3": ("qwen3", 3, 37, bf, None, None, {}, None, 0),
    "qwen3, B = 3, left-padded": ("qwen3", 3, 37, bf, None, None, dict(padded=True), (0, 7, 19), 0),
    "llama, B = 17, wide_decode": ("llama", 17, 21, bf, None, None, dict(wide_decode=True), None, 0),
    "qwen3, B = 2, fp8_decode": ("qwen3", 2, 37, bf, None, None, dict(fp8_decode=True), None, 0),
    "llama, B = 2, continued": ("llama", 2, 37, bf, None, None, dict(continued=True), None, 6),
    "phi3 with its window": ("phi3", 2, 30, bf, None, None, {}, None, 0),
    "llama, q_proj and v_proj only": ("llama", 2, 37, bf, None, ("q_proj", "v_proj"), {}, None, 0),
    "qwen3, fp32 adapters": ("qwen3", 2, 37, bf, f32, None, {}, None, 0),
    "llama, f16 build": ("llama", 1, 37, f16, f32, None, {}, None, 0),     # (fp32 adapters: lora.adapter_of takes bf16 or fp32, as peft
    #                                                                          keeps the adapters of an fp16 base in fp32)
}


@pytest.mark.parametrize("case", list(CASES))
def test_unmerged_adapters_on_the_fused_routes(ops, case):
    from u2tokenizer_amd import prefill
    kind, B, S, dt, adt, targets, flags, pads, chunk = CASES[case]
    snap = bool(flags.get("fp8_decode"))
    m32, mg = _pair(kind, dt, adt, targets, snap)
    E = m32.config.hidden_size
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), 7)
    xs = 0.5 * synth.synth_tensor("inputs_embeds", (B, STEPS, E), 8)
    xd, xsd = x.to(dt).to(D), xs.to(dt).to(D)
    ref = _run(m32, x, xs, pads, chunk)
    stock = _run(mg, xd, xsd, pads, chunk)
    per_layer = _adapters(mg) // NL
    assert per_layer == (2 if targets else 4 if kind == "phi3" else 7)
    assert prefill.enable_fused_prefill(mg, lora=True, **flags) == NL
    n0, s0, e0, w0, wd0 = (dict(d) for d in (prefill.lora_stats, prefill.stats, prefill.extend_stats, prefill.w8_stats, prefill.wide_stats))
    fused = _run(mg, xd, xsd, pads, chunk)
    dl = {k: prefill.lora_stats[k] - n0[k] for k in n0}
    calls = 1 + STEPS + (1 if chunk else 0)
    assert dl == {"prefill": NL, "extend": NL if chunk else 0, "decode": NL * STEPS, "adapters": NL * per_layer * calls}, dl
    p, d = ("padded_prefill", "padded_decode") if pads else ("prefill", "decode")
    assert prefill.stats[p] - s0[p] == NL and prefill.stats[d] - s0[d] == NL * STEPS
    assert prefill.extend_stats["extend"] - e0["extend"] == (NL if chunk else 0)
    assert prefill.w8_stats["decode"] - w0["decode"] == (NL * STEPS if snap else 0)
    assert prefill.wide_stats["decode"] - wd0["decode"] == (NL * STEPS if B > 16 else 0)
    # the same fused run with the adapters ignored: the base layers alone
    _adapters(mg, disable_adapters=True)
    base = _run(mg, xd, xsd, pads, chunk)
    _adapters(mg, disable_adapters=False)
    assert prefill.lora_stats["adapters"] - n0["adapters"] == NL * per_layer * calls      # (nothing computed for disabled wrappers)
    prefill.disable_fused_prefill(mg)
    ratio = _gates(case, fused, stock, ref, pads, EPS[dt], base)
    print(f"{case}: base-only error / gate >= {ratio:.1f}")
    assert ratio >= 10, (case, ratio)


@pytest.mark.parametrize("flag", ["disable_adapters", "merged"])
@pytest.mark.parametrize("kind", ["qwen3", "phi3"])
def test_switched_off_wrappers_give_the_bits_of_the_unwrapped_model(ops, kind, flag):
    """DPO's null-reference pass (`disable_adapters`) and a merged model that kept its wrappers: the fused routes on the base layers,
    bit for bit what the unwrapped model's fused routes give -- prefill, cached keys / values, decode steps"""
    from u2tokenizer_amd import prefill
    plain = BUILDS[kind]().to(bf).to(D)
    mg = _wrapped(BUILDS[kind]().to(bf).to(D))
    E = plain.config.hidden_size
    xd = (0.5 * synth.synth_tensor("inputs_embeds", (2, 30, E), 7)).to(bf).to(D)
    xsd = (0.5 * synth.synth_tensor("inputs_embeds", (2, STEPS, E), 8)).to(bf).to(D)
    prefill.enable_fused_prefill(plain)
    want = _run(plain, xd, xsd)
    _adapters(mg, **{flag: True})
    mg.train()                                           # (the dropout does not matter: the branch is not computed)
    prefill.enable_fused_prefill(mg, lora=True)
    n0, s0 = dict(prefill.lora_stats), dict(prefill.stats)
    got = _run(mg, xd, xsd)
    assert prefill.lora_stats == n0 and prefill.stats["prefill"] - s0["prefill"] == NL and prefill.stats["decode"] - s0["decode"] == NL * STEPS
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    for (ka, va), (kb, vb) in zip(got[1], want[1]):
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    prefill.disable_fused_prefill(mg), prefill.disable_fused_prefill(plain)


def test_cached_adapter_copies_refresh(ops):
    """fp32 adapters are computed from 16-bit copies kept in the layer's patch state: B.weight.mul_(2) between two calls moves the
    output to the new reference under the gate (and away from the old one), without a rebuild in between"""
    from u2tokenizer_amd import prefill
    m32, mg = _pair("llama", bf, f32)
    x = 0.5 * synth.synth_tensor("inputs_embeds", (2, 37, 512), 7)
    xs = 0.5 * synth.synth_tensor("inputs_embeds", (2, STEPS, 512), 8)
    xd, xsd = x.to(bf).to(D), xs.to(bf).to(D)
    prefill.enable_fused_prefill(mg, lora=True)
    b0 = prefill.lora_state_builds[0]
    first = _run(mg, xd, xsd)
    assert prefill.lora_state_builds[0] - b0 == NL       # once per layer, not per call
    old = _run(m32, x, xs)
    with torch.no_grad():
        for m in (m32, mg):
            for mod in m.modules():
                if isinstance(mod, LoRALinear):
                    mod.lora_B["default"].weight.mul_(2)
    ref = _run(m32, x, xs)
    got = _run(mg, xd, xsd)
    assert prefill.lora_state_builds[0] - b0 == 2 * NL
    prefill.disable_fused_prefill(mg)
    stock = _run(mg, xd, xsd)
    _gates("doubled B", got, stock, ref, None, EPS[bf])
    for a, b, r in zip(got[0], first[0], old[0]):
        assert _err(a.float().cpu(), r) > 10 * (_err(b.float().cpu(), r) + EPS[bf])


@pytest.mark.parametrize("how", ["active dropout", "switch off", "train_lora alone"])
def test_what_keeps_the_stock_forward_bit_for_bit(ops, how):
    """model.train() with p = 0.05 under no_grad (peft applies the dropout), the switch off, and train_lora alone: the wrapped layers
    run their own forward -- the unpatched model's bits under one seed, no fused call counted"""
    from u2tokenizer_amd import prefill
    mg = _wrapped(BUILDS["qwen3"]().to(bf).to(D))
    if how == "active dropout":
        mg.train()
    xd = (0.5 * synth.synth_tensor("inputs_embeds", (2, 30, 512), 7)).to(bf).to(D)
    xsd = (0.5 * synth.synth_tensor("inputs_embeds", (2, 2, 512), 8)).to(bf).to(D)
    torch.manual_seed(5)
    want = _run(mg, xd, xsd)
    prefill.enable_fused_prefill(mg, **({"lora": True} if how == "active dropout" else {"train_lora": True} if how == "train_lora alone" else {}))
    n0, s0 = dict(prefill.lora_stats), dict(prefill.stats)
    torch.manual_seed(5)
    got = _run(mg, xd, xsd)
    prefill.disable_fused_prefill(mg)
    assert prefill.lora_stats == n0 and prefill.stats == s0
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    if how == "active dropout":                          # (the dropout is live: another seed, other bits)
        torch.manual_seed(6)
        assert not torch.equal(_run(mg, xd, xsd)[0][0], want[0][0])
