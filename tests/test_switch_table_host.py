"""CPU: prefill.SWITCHES, the one table behind `enable_fused_prefill`'s keywords, the stack state's fields and the config
attributes `language_model._maybe_fuse` reads.  For every switch: the keyword alone sets its field and what it implies and nothing
else; the config attribute of a u2 causal LM alone does the same (plus what the switch needs to act); a second call without the
keyword clears it and frees what it kept per layer; and the signature's defaults are the table's.  The stub models and the
fake-`is_cuda` tensor are those of tests/test_decoder_route_host.py."""
import inspect

import pytest
import torch

from test_decoder_route_host import _FakeCuda, _model
from u2tokenizer_amd import language_model as LM
from u2tokenizer_amd import prefill

bf = torch.bfloat16
BY_KW = {s.kw: s for s in prefill.SWITCHES}
FIELDS = {s.kw: s.field for s in prefill.SWITCHES if s.field is not None}
IDS = [s.kw for s in prefill.SWITCHES]


def _fields(stack):
    return {kw: getattr(stack, f) for kw, f in FIELDS.items()}


def _expected(on):
    """the stack's fields when exactly the keywords `on` differ from their defaults"""
    want = {kw: BY_KW[kw].default for kw in FIELDS}
    for kw in on:
        if kw in FIELDS:
            want[kw] = not BY_KW[kw].default
    return want


def test_the_table_and_the_signature_agree():
    params = inspect.signature(prefill.enable_fused_prefill).parameters
    assert list(params) == ["model"] + IDS
    for s in prefill.SWITCHES:
        assert params[s.kw].default is s.default and isinstance(s.doc, str) and s.doc
        assert all(k in BY_KW for k in s.implies + s.needs)
        assert all(f in prefill._LayerState.__dataclass_fields__ for f in s.frees)
    assert sorted(FIELDS.values()) == sorted(f for f in prefill._StackState.__dataclass_fields__
                                             if f not in ("hook", "pad", "pad_shape", "scratch"))
    assert [s.kw for s in prefill.SWITCHES if s.config is None] == ["decode", "strict"]
    assert BY_KW["train_lora"].implies == ("train",) and BY_KW["train_phi3"].needs == ("train",)
    assert BY_KW["fp8_decode"].frees == ("w8",) and set(BY_KW["lora"].frees) == {"lora", "ads"}


@pytest.mark.parametrize("kw", IDS)
def test_keyword_alone_sets_its_field_and_what_it_implies(kw):
    s = BY_KW[kw]
    m = _model()
    prefill.enable_fused_prefill(m, **{kw: not s.default})
    want = _expected((kw,) + (s.implies if not s.default else ()))
    assert _fields(m.model._u2_stack) == want
    # ... and a second call without it sets every switch anew and frees what this one kept per layer
    st = m.model.layers[0]._u2_prefill
    for f in s.frees:
        setattr(st, f, ("kept",))
    st.variants[(0, False)] = "kept"
    prefill.enable_fused_prefill(m)
    assert _fields(m.model._u2_stack) == _expected(())
    for f in s.frees:
        assert getattr(st, f) is None
    assert not s.frees or st.variants == {}            # (the descriptors built from it go with it)
    prefill.disable_fused_prefill(m)


def test_strict_refuses_a_foreign_layer_and_its_absence_skips_it():
    m = _model()
    m.model.layers.append(torch.nn.Linear(4, 4))
    with pytest.raises(RuntimeError, match="unsupported decoder layer"):
        prefill.enable_fused_prefill(m)
    assert prefill.enable_fused_prefill(m, strict=False) == 1


@pytest.mark.parametrize("kw", [s.kw for s in prefill.SWITCHES if s.config])
@pytest.mark.parametrize("grad", [False, True])
def test_config_attribute_alone_does_the_same(kw, grad):
    s = BY_KW[kw]
    cfg = LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=16)
    setattr(cfg, s.config, not s.default)
    m = LM.u2Qwen3ForCausalLM(cfg).to(bf).eval()
    layer = m.model.layers[0]
    p0 = next(layer.parameters())
    layer.parameters = lambda *a, **k: iter([p0.detach().as_subclass(_FakeCuda)])
    with torch.set_grad_enabled(grad):
        m(inputs_embeds=torch.zeros(1, 3, 64, dtype=bf))
    want = _expected((kw,) + ((s.implies + s.needs) if not s.default else ()))
    if not want["train" if grad else "prefill"]:      # nothing asks for this grad mode's route: the layers are not patched
        assert "_u2_stack" not in m.model.__dict__ and not prefill.is_patched(layer)
        return
    assert prefill.is_patched(layer) and _fields(m.model._u2_stack) == want
