"""CPU: when a u2 causal LM patches its decoder layers for the HIP routes (language_model.py: on its forward) -- per grad mode,
per config switch (`u2_fused_prefill`, `u2_fused_decoder_training`), per device and dtype of the decoder, for either call
order -- and with which switches.  `prefill.enable_fused_prefill` is replaced by a recorder; the decoder's first parameter
reports `is_cuda` as asked, the layers themselves run stock on the CPU."""
import itertools

import pytest
import torch

from u2tokenizer_amd import language_model as LM, prefill

bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32


class _FakeCuda(torch.Tensor):
    @property
    def is_cuda(self):
        return True


def _expected(order, prefill_on, train_on, dtype, cuda):
    """Without grad: patched once, when `u2_fused_prefill` is on and the decoder is bf16 / fp16 on the GPU; with grad: once,
    when `u2_fused_decoder_training` is on and the decoder is bf16 on the GPU.  Either way with both switches as configured."""
    calls, done = [], set()
    for grad in order:
        if grad in done or not (train_on if grad else prefill_on):
            continue
        if cuda and dtype in ((bf,) if grad else (bf, f16)):
            calls.append((True, False, train_on, prefill_on))
            done.add(grad)
    return calls


@pytest.mark.parametrize("prefill_on,train_on,dtype,cuda,order", list(itertools.product(
    (True, False), (True, False), (bf, f16, f32), (True, False), ((False, True, False, True), (True, False, True, False)))))
def test_lm_patches_its_decoder_once_per_grad_mode(monkeypatch, prefill_on, train_on, dtype, cuda, order):
    calls = []

    def record(model, decode=True, strict=True, train=False, prefill=True):
        calls.append((decode, strict, train, prefill))
        return 0

    monkeypatch.setattr(prefill, "enable_fused_prefill", record)
    cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=16)
    cfg.u2_fused_prefill, cfg.u2_fused_decoder_training = prefill_on, train_on
    m = LM.u2Qwen3ForCausalLM(cfg).to(dtype).eval()
    if cuda:
        layer = m.model.layers[0]
        p0 = next(layer.parameters())
        layer.parameters = lambda *a, **k: iter([p0.detach().as_subclass(_FakeCuda)])
    for grad in order:
        with torch.set_grad_enabled(grad):
            m(inputs_embeds=torch.zeros(1, 3, 64, dtype=dtype))
    assert calls == _expected(order, prefill_on, train_on, dtype, cuda)
