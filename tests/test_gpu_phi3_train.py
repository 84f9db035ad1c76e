"""GPU: Phi-3 decoder layers (packed qkv_proj / gate_up_proj, head dim 96) and head dim 96 on the decoder's training route --
`enable_fused_prefill(model, train=True, train_phi3=True)` -- as tests/test_gpu_decoder_train.py holds the Llama / Qwen3 route: whole
small decoders against the fp32 stock model under the project's gate (no further from fp32 than 1.5 x the stock bf16 run + 1e-3),
with and without non-reentrant gradient checkpointing, one layer at the Phi-3-mini width, and the calls that keep the stock layers,
by the route's own counter."""
import pytest
import torch

from test_gpu_decoder_train import _batch, _err, _run, ops  # noqa: F401
from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"


def _phi3(layers=2, E=384, H=4, Hkv=4, inter=768, window=2047, vocab=512):
    from transformers import Phi3Config, Phi3ForCausalLM
    m = Phi3ForCausalLM(Phi3Config(vocab_size=vocab, hidden_size=E, intermediate_size=inter, num_hidden_layers=layers,
                                   num_attention_heads=H, num_key_value_heads=Hkv, max_position_embeddings=512, sliding_window=window,
                                   tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m


def _llama96(layers=2):
    from transformers import LlamaConfig, LlamaForCausalLM
    m = LlamaForCausalLM(LlamaConfig(vocab_size=512, hidden_size=384, intermediate_size=768, num_hidden_layers=layers,
                                     num_attention_heads=4, num_key_value_heads=2, head_dim=96, max_position_embeddings=512,
                                     tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2))
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m


BUILDS = {"phi3": _phi3, "phi3 grouped": lambda: _phi3(Hkv=2), "llama 96": _llama96}
_REF = {}


def _reference(kind, ckpt):
    """the fp32 stock run and the batch, once per (build, checkpointing)"""
    if (kind, ckpt) not in _REF:
        m32 = BUILDS[kind]().to(D)
        batch = _batch(2, 96, (96, 57), m32.config.hidden_size, m32.config.vocab_size)
        _REF[kind, ckpt] = (batch, _run(m32, *batch, torch.float32, ckpt))
    return _REF[kind, ckpt]


@pytest.mark.parametrize("kind,ckpt", [("phi3", False), ("phi3", True), ("phi3 grouped", False), ("phi3 grouped", True),
                                       ("llama 96", False)])
def test_phi3_training_route_matches_the_stock_decoder(ops, kind, ckpt):
    """Loss, last hidden states (pad rows included), every layer parameter's gradient -- qkv_proj.weight and gate_up_proj.weight as
    whole tensors -- and d inputs_embeds of a right-padded batch of two (96, 57 of 96 positions): no further from the fp32 stock
    model than 1.5 x the stock bf16 run is (+ 1e-3); the route ran in every layer (twice with checkpointing: forward + recompute),
    and not with the bits of the stock layers."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill
    nl = 2
    (x, mask, labels), ref = _reference(kind, ckpt)
    mg = BUILDS[kind]().to(bf).to(D)
    stock = _run(mg, x, mask, labels, bf, ckpt)
    assert enable_fused_prefill(mg, train=True, train_phi3=True) == nl
    n0 = decoder_train.stats["layers"]
    fused = _run(mg, x, mask, labels, bf, ckpt)
    assert decoder_train.stats["layers"] - n0 == nl * (2 if ckpt else 1)
    assert not torch.equal(fused[1], stock[1])
    for i, name in ((0, "loss"), (1, "hidden"), (3, "d inputs_embeds")):
        es, ef = _err(stock[i], ref[i]), _err(fused[i], ref[i])
        print(f"{kind} ckpt={ckpt} {name}: fused {ef:.3e} stock {es:.3e}")
        assert ef <= 1.5 * es + 1e-3, (name, ef, es)
    assert fused[2].keys() == ref[2].keys()
    if kind.startswith("phi3"):
        assert any(n.endswith("qkv_proj.weight") for n in ref[2]) and any(n.endswith("gate_up_proj.weight") for n in ref[2])
    for n in ref[2]:
        assert fused[2][n].shape == ref[2][n].shape
        es, ef = _err(stock[2][n], ref[2][n]), _err(fused[2][n], ref[2][n])
        assert ef <= 1.5 * es + 1e-3, (n, ef, es)
    # switching the option off, and disabling, restore the stock bits
    enable_fused_prefill(mg, train=True)
    n0 = decoder_train.stats["layers"]
    again = _run(mg, x, mask, labels, bf, ckpt)
    assert decoder_train.stats["layers"] == n0 and torch.equal(again[1], stock[1])
    disable_fused_prefill(mg)


def test_one_layer_at_the_phi3_mini_width(ops):
    """E 3072, 32 heads of 96, I 8192, W 2047; B = 1, S = 128, forward + backward: the output, d input and the four weight gradients
    under the same gate."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import enable_fused_prefill
    kw = dict(layers=1, E=3072, H=32, Hkv=32, inter=8192, vocab=64)
    S = 128
    x = 0.5 * synth.synth_tensor("inputs_embeds", (1, S, 3072), 7)
    g = synth.synth_tensor("d_hidden", (1, S, 3072), 8)

    def run(m, dtype):
        m.train()
        m.zero_grad(set_to_none=True)
        xe = x.to(D, dtype).requires_grad_(True)
        with torch.enable_grad():
            h = m.model(inputs_embeds=xe, use_cache=False).last_hidden_state
            (h.float() * g.to(D)).sum().backward()
        grads = {n: p.grad.detach().clone() for n, p in m.model.layers[0].named_parameters() if n.endswith("proj.weight")}
        return {"output": h.detach(), "d input": xe.grad.detach(), **grads}

    ref = run(_phi3(**kw).to(D), torch.float32)
    assert sorted(n for n in ref if n.endswith("weight")) == ["mlp.down_proj.weight", "mlp.gate_up_proj.weight",
                                                              "self_attn.o_proj.weight", "self_attn.qkv_proj.weight"]
    mg = _phi3(**kw).to(bf).to(D)
    stock = run(mg, bf)
    assert enable_fused_prefill(mg, train=True, train_phi3=True) == 1
    n0 = decoder_train.stats["layers"]
    fused = run(mg, bf)
    assert decoder_train.stats["layers"] - n0 == 1
    assert not torch.equal(fused["output"], stock["output"])
    for n in ref:
        es, ef = _err(stock[n], ref[n]), _err(fused[n], ref[n])
        print(f"phi3-mini layer {n}: fused {ef:.3e} stock {es:.3e}")
        assert ef <= 1.5 * es + 1e-3, (n, ef, es)


def test_phi3_training_route_stays_stock(ops):
    """By the route's counter: without the new switch a Phi-3 never enters the route; with it a call longer than the attention window
    and a left-padded batch keep the stock layers, a call as long as the window trains."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import enable_fused_prefill
    st = decoder_train.stats

    def layers_run(m, S, mask=None):
        n0 = st["layers"]
        x, m2, lab = _batch(2, S, (S, S), m.config.hidden_size, m.config.vocab_size)
        _run(m, x, m2 if mask is None else mask, lab, bf, False)
        return st["layers"] - n0

    mg = _phi3().to(bf).to(D)
    assert layers_run(mg, 96) == 0                               # not patched
    enable_fused_prefill(mg, train=True)
    assert layers_run(mg, 96) == 0                               # the training route without the new switch
    enable_fused_prefill(mg, train_phi3=True)
    assert layers_run(mg, 96) == 0                               # the new switch without the training route
    enable_fused_prefill(mg, train=True, train_phi3=True)
    assert layers_run(mg, 96) == 2
    left = torch.ones((2, 96), dtype=torch.int64)
    left[1, :9] = 0
    assert layers_run(mg, 96, mask=left) == 0                    # left padding
    mw = _phi3(window=64).to(bf).to(D)
    enable_fused_prefill(mw, train=True, train_phi3=True)
    assert layers_run(mw, 96) == 0                               # S = 96 > W = 64: the band is not in the backward kernels
    assert layers_run(mw, 64) == 2                               # S = W
