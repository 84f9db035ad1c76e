"""GPU: LoRA-wrapped decoder layers on the training route (enable_fused_prefill(train_lora=True); decoder_train.LoraDeltaFn over the
rank-r kernels of csrc/lora.hip) -- small Llama, Qwen3 and Phi-3 decoders with every projection wrapped (r = 16), against the same
wrapped model in fp32 under the project's gate "no further from the fp32 model than 1.5 x the stock bf16 run is, + 1e-3", with bf16
and with fp32 adapter weights, checkpointing off and on; real nn.Dropout masks against the stock wrapped layers' under one seed;
zero B against the route without adapters; and what must keep the stock forward, by counter."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from test_gpu_decoder_train import _batch, _err, _small, ops  # noqa: F401
from test_gpu_phi3_train import _phi3
from test_lora_host import NOT_RUNNABLE, REFUSALS
from u2tokenizer_amd.lora import LoRALinear, add_lora

pytestmark = pytest.mark.gpu
bf, f32 = torch.bfloat16, torch.float32
D = "cuda"
BUILDS = {"llama": lambda: _small("llama"), "qwen3": lambda: _small("qwen3"), "phi3": _phi3}
NL, BATCH, S, LENS = 2, 2, 96, (96, 57)


class FixedMaskDropout(nn.Module):
    """inverted dropout with p = 0.25 whose mask depends on (seed, shape) alone: the fp32, stock bf16 and route runs, and a checkpoint
    recompute, see the same masks"""

    def __init__(self, seed: int, p: float = 0.25):
        super().__init__()
        self.seed, self.p, self.masks = seed, p, {}

    def forward(self, x):
        key = tuple(x.shape)
        if key not in self.masks:
            g = torch.Generator().manual_seed(self.seed)
            self.masks[key] = (torch.rand(key, generator=g) >= self.p).to(x.device)
        return x * self.masks[key].to(x.dtype) / (1.0 - self.p)


def _wrap(m, adapter_dtype=None, dropout="fixed", zero_b=False):
    """every projection wrapped, r = 16; A Kaiming-uniform and B normal from a seeded CPU generator, B scaled so that scaling * B A
    is of the size of 0.7 x the base weight"""
    n = add_lora(m, adapter_dtype=adapter_dtype)
    g = torch.Generator().manual_seed(23)
    for i, w in enumerate(mod for mod in m.modules() if isinstance(mod, LoRALinear)):
        A, B = w.lora_A["default"].weight, w.lora_B["default"].weight
        K = A.shape[1]
        A.data.copy_((torch.rand(A.shape, generator=g) * 2 - 1) * K ** -0.5)
        std = float(f"{w.weight.float().std().item():.2g}")     # (two digits: the same number for the fp32 and the bf16 weights)
        sigma = 0.7 * std * (3 * K) ** 0.5 / (w.scaling["default"] * 16 ** 0.5)
        B.data.copy_(torch.zeros(B.shape) if zero_b else torch.randn(B.shape, generator=g) * sigma)
        if dropout == "fixed":
            w.lora_dropout["default"] = FixedMaskDropout(1000 + i)
    return n


def _run(m, x, mask, labels, dtype, ckpt):
    """test_gpu_decoder_train._run for a model with frozen parameters: gradients of the trainable ones, names of the others' non-None"""
    m.train()
    if ckpt:
        m.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})
    else:
        m.gradient_checkpointing_disable()
    m.zero_grad(set_to_none=True)
    xe = x.to(D, dtype).requires_grad_(True)
    with torch.enable_grad():
        h = m.model(inputs_embeds=xe, attention_mask=mask.to(D), use_cache=False).last_hidden_state
        logits = m.lm_head(h).float()
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1).to(D), ignore_index=-100)
        loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.model.layers.named_parameters() if p.requires_grad}
    leaked = [n for n, p in m.named_parameters() if not p.requires_grad and p.grad is not None]
    return loss.detach(), h.detach(), grads, xe.grad.detach(), leaked


_REF = {}


def _reference(kind, ckpt):
    """the batch, the fp32 wrapped run and (once per build) the fp32 last hidden states without adapters"""
    if (kind, ckpt) not in _REF:
        m32 = BUILDS[kind]().to(D)
        batch = _batch(BATCH, S, LENS, m32.config.hidden_size, m32.config.vocab_size)
        if kind not in _REF:
            m32.train()
            with torch.no_grad():
                _REF[kind] = m32.model(inputs_embeds=batch[0].to(D), attention_mask=batch[1].to(D), use_cache=False).last_hidden_state
        _wrap(m32)
        _REF[kind, ckpt] = (batch, _run(m32, *batch, f32, ckpt))
    return _REF[kind, ckpt] + (_REF[kind],)


@pytest.mark.parametrize("adapter_dtype", [bf, f32], ids=["bf16 adapters", "fp32 adapters"])
@pytest.mark.parametrize("ckpt", [False, True], ids=["", "checkpointing"])
@pytest.mark.parametrize("kind", list(BUILDS))
def test_lora_training_route_matches_the_wrapped_decoder(ops, kind, ckpt, adapter_dtype):
    """Loss, last hidden states, d inputs_embeds and every adapter gradient of a right-padded batch of two: no further from the fp32
    wrapped model than 1.5 x the stock bf16 wrapped run is (+ 1e-3).  The adapters matter: in fp32 they move the last hidden states
    by at least 20 x the stock bf16 run's own error, so a route that ignored them could not pass.  Every frozen base weight's .grad
    stays None; the route ran in every layer (twice with checkpointing), all of its adapters on the rank-r kernels."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import enable_fused_prefill
    batch, ref, h_plain = _reference(kind, ckpt)
    mg = BUILDS[kind]().to(bf).to(D)
    per_layer = _wrap(mg, adapter_dtype=adapter_dtype) // NL
    assert per_layer == (4 if kind == "phi3" else 7)
    stock = _run(mg, *batch, bf, ckpt)
    assert enable_fused_prefill(mg, train_lora=True, train_phi3=kind == "phi3") == NL
    n0, l0 = decoder_train.stats["layers"], dict(decoder_train.lora_stats)
    fused = _run(mg, *batch, bf, ckpt)
    times = NL * (2 if ckpt else 1)
    assert decoder_train.stats["layers"] - n0 == times
    assert decoder_train.lora_stats["layers"] - l0["layers"] == times
    assert decoder_train.lora_stats["adapters"] - l0["adapters"] == times * per_layer
    assert not torch.equal(fused[1], stock[1])
    moved, own = _err(ref[1], h_plain), _err(stock[1], ref[1])
    print(f"{kind}: the adapters move the fp32 hidden states by {moved:.3f}, the stock bf16 run errs by {own:.5f}")
    assert moved >= 20 * own, (moved, own)
    for i, name in ((0, "loss"), (1, "hidden"), (3, "d inputs_embeds")):
        es, ef = _err(stock[i], ref[i]), _err(fused[i], ref[i])
        print(f"{name}: route {ef:.5f}, stock {es:.5f}")
        assert ef <= 1.5 * es + 1e-3, (name, ef, es)
    assert fused[2].keys() == ref[2].keys() == stock[2].keys() and len(fused[2]) == 2 * NL * per_layer
    for n in ref[2]:
        assert ".lora_A." in n or ".lora_B." in n
        assert fused[2][n].dtype == adapter_dtype and fused[2][n].shape == ref[2][n].shape
        es, ef = _err(stock[2][n], ref[2][n]), _err(fused[2][n], ref[2][n])
        assert ef <= 1.5 * es + 1e-3, (n, ef, es)
    assert not fused[4] and not stock[4], fused[4]          # frozen parameters: .grad is None


@pytest.mark.parametrize("adapter_dtype", [bf, f32], ids=["bf16 adapters", "fp32 adapters"])
def test_real_dropout_draws_the_stock_layers_masks(ops, adapter_dtype):
    """nn.Dropout(0.05) under one seed: the route calls each adapter's own dropout module on the stock shape, in the stock order (q,
    k, v, o, gate, up, down) and in the adapter dtype, so every module drops the elements it drops in the stock wrapped layer."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import enable_fused_prefill
    mg = _small("llama").to(bf).to(D)
    _wrap(mg, adapter_dtype=adapter_dtype, dropout="real")
    drops = [(n, mod) for n, mod in mg.named_modules() if type(mod) is nn.Dropout and ".lora_dropout." in n]
    assert len(drops) == 7 * NL and all(mod.p == 0.05 for _, mod in drops)
    seen = {}
    hooks = [mod.register_forward_hook(lambda _m, inp, out, n=n: seen.setdefault(n, []).append(((out == 0).cpu(), (inp[0] != 0).cpu())))
             for n, mod in drops]
    batch = _batch(BATCH, S, LENS, mg.config.hidden_size, mg.config.vocab_size)
    torch.manual_seed(77)
    stock = _run(mg, *batch, bf, False)
    masks_stock, seen = seen, {}
    assert enable_fused_prefill(mg, train_lora=True) == NL
    l0 = decoder_train.lora_stats["layers"]
    torch.manual_seed(77)
    fused = _run(mg, *batch, bf, False)
    assert decoder_train.lora_stats["layers"] - l0 == NL    # (hooks on the dropout modules do not send the layer to the stock forward)
    for h in hooks:
        h.remove()
    assert masks_stock.keys() == seen.keys() and len(seen) == 7 * NL
    for n in seen:
        assert len(seen[n]) == len(masks_stock[n]) == 1
        (a, nza), (b, nzb) = masks_stock[n][0], seen[n][0]
        live = nza & nzb                                    # (a residual sum that is exactly 0 in one run says nothing about its mask)
        assert a.shape == b.shape and live.float().mean().item() > 0.99 and 0.03 < a[live].float().mean().item() < 0.07, n
        assert torch.equal(a[live], b[live]), n
    assert _err(fused[1], stock[1]) < 0.05                  # same masks: the two runs differ by bf16 rounding only


def test_zero_b_is_the_route_without_adapters(ops):
    """B = 0: float(y) + s * 0 rounds back to y, so the wrapped route's hidden states are those of the plain training route"""
    from u2tokenizer_amd.prefill import enable_fused_prefill
    batch = _batch(BATCH, S, LENS, 512, 512)
    plain = _small("llama").to(bf).to(D)
    for p in plain.parameters():
        p.requires_grad_(False)
    enable_fused_prefill(plain, train=True)
    h0 = _run_hidden(plain, batch)
    mg = _small("llama").to(bf).to(D)
    _wrap(mg, zero_b=True)
    enable_fused_prefill(mg, train_lora=True)
    assert torch.equal(_run_hidden(mg, batch), h0)


def _run_hidden(m, batch, B=None):
    m.train()
    x, mask = batch[0], batch[1]
    if B is not None:
        x, mask = x[:B], mask[:B]
    with torch.enable_grad():
        return m.model(inputs_embeds=x.to(D, bf).requires_grad_(True), attention_mask=mask.to(D), use_cache=False).last_hidden_state.detach()


def test_lora_route_stays_stock(ops):
    """By the counters: with train=True alone, or without a switch, a wrapped layer keeps the stock forward; with train_lora each
    refusal of lora.adapter_of (the table of tests/test_lora_host.py, on layer 1's q_proj) sends that layer, and only it, to the stock
    forward; without grad a wrapped layer never takes a HIP route."""
    from u2tokenizer_amd import decoder_train, prefill
    from u2tokenizer_amd.prefill import enable_fused_prefill
    st, ls = decoder_train.stats, decoder_train.lora_stats
    mg = _small("llama").to(bf).to(D)
    _wrap(mg)
    batch = _batch(BATCH, 32, (32, 20), 512, 512)

    def ran():
        n0, l0 = st["layers"], ls["layers"]
        _run_hidden(mg, batch)
        return st["layers"] - n0, ls["layers"] - l0

    assert ran() == (0, 0)
    enable_fused_prefill(mg, train=True)
    assert ran() == (0, 0)                                  # train alone: wrapped projections keep the stock forward
    enable_fused_prefill(mg, train_lora=True)
    assert ran() == (NL, NL)
    p0 = dict(prefill.stats)
    with torch.no_grad():
        mg.model(inputs_embeds=batch[0].to(D, bf), attention_mask=None, use_cache=False)
    assert dict(prefill.stats) == p0                        # no grad: unmerged adapters never take the prefill route
    att = mg.model.layers[1].self_attn
    good = att.q_proj
    for name, change in REFUSALS.items():
        if name in NOT_RUNNABLE:
            continue
        q = copy.deepcopy(good)
        change(q)
        att.q_proj = q.to(D)
        assert ran() == (1, 1), name
    att.q_proj = good
    assert ran() == (NL, NL)
