"""CPU: the route of a patched decoder layer with the Phi-3 training switch -- `enable_fused_prefill(model, train=True,
train_phi3=True)`, `config.u2_fused_phi3_training` -- pinned as a table, with the recorders of tests/test_decoder_route_host.py
(nothing is launched: the training route ends in a recorder in place of `decoder_train.layer_forward_train`).

The switch adds head dim 96 (either layout) and the packed Phi-3 layout (head dims 64 / 96 / 128) to the training route; every other
condition of the route holds as before, a layer with an attention window W trains while S <= W, and without `train` the switch
does nothing.  The table of that module (switch off) stays as it is."""
import types

import pytest
import torch

import test_decoder_route_host as R
from u2tokenizer_amd import language_model as LM, prefill

recorder = R.recorder
bf, f16 = R.bf, R.f16
PHI3 = dict(kind="phi3", hidden=192, head_dim=96)


def _patch(m, calls, **flags):
    for layer in m.model.layers:
        layer._calls = calls
        layer.forward = types.MethodType(R._stock, layer)
    prefill.enable_fused_prefill(m, **{"train": True, "train_phi3": True, **flags})


# (model kwargs, enable flags, call kwargs, expected route with grad enabled)
TRAIN_PHI3 = {
    "phi3 layout, head dim 96": (PHI3, {}, {}, "train"),
    "phi3 layout, head dim 64": (dict(kind="phi3", hidden=128, head_dim=64), {}, {}, "train"),
    "phi3 layout, head dim 128": (dict(kind="phi3", hidden=256, head_dim=128), {}, {}, "train"),
    "qwen3, head dim 96": (dict(head_dim=96), {}, {}, "train"),
    "llama, head dim 96": (dict(kind="llama", head_dim=96), {}, {}, "train"),
    "qwen3, head dim 64": ({}, {}, {}, "train"),
    "head dim 256": (dict(head_dim=256), {}, {}, "stock"),
    "fp16": (dict(dtype=f16, **PHI3), {}, {}, "stock"),
    "fp16, qwen3 at 96": (dict(dtype=f16, head_dim=96), {}, {}, "stock"),
    "fp32": (dict(dtype=torch.float32, **PHI3), {}, {}, "stock"),
    "empty cache": (PHI3, {}, dict(cache="plain"), "stock"),
    "filled cache": (PHI3, {}, dict(cache="plain full"), "stock"),
    "right-padded layer mask": (PHI3, {}, dict(B=2, S=8, mask=R._right_padded(2, 8, 5)), "train"),
    "left-padded layer mask": (PHI3, {}, dict(B=2, S=8, mask=R._left_padded(2, 8)), "stock"),
    "left-padded layer mask, llama at 96": (dict(kind="llama", head_dim=96), {}, dict(B=2, S=8, mask=R._left_padded(2, 8)), "stock"),
    "intermediate % 8 != 0": (dict(inter=260, **PHI3), {}, {}, "stock"),
    "output_attentions": (PHI3, {}, dict(output_attentions=True), "stock"),
    "no position embeddings": (PHI3, {}, dict(pe=False), "stock"),
    "window W, S < W": (dict(window=32, **PHI3), {}, dict(S=24), "train"),
    "window W, S = W": (dict(window=32, **PHI3), {}, dict(S=32), "train"),
    "window W, S > W": (dict(window=32, **PHI3), {}, dict(S=40), "stock"),
    "window W, S > W, head dim 64": (dict(kind="phi3", hidden=128, head_dim=64, window=32), {}, dict(S=33), "stock"),
    "train_phi3 without train": (PHI3, dict(train=False), {}, "stock"),
    "train_phi3 without train, llama at 96": (dict(kind="llama", head_dim=96), dict(train=False), {}, "stock"),
    "prefill off": (PHI3, dict(prefill=False), {}, "train"),
}


@pytest.mark.parametrize("name", list(TRAIN_PHI3))
def test_training_route_with_the_phi3_switch(recorder, name):
    mk, flags, call, want = TRAIN_PHI3[name]
    m = R._model(**mk)
    _patch(m, recorder, **flags)
    assert R._route(m, recorder, grad=True, **call) == want


@pytest.mark.parametrize("name", ["phi3 layout, head dim 96", "window W, S > W", "train_phi3 without train"])
def test_the_switch_leaves_the_no_grad_routes_alone(recorder, name):
    mk, flags, call, _ = TRAIN_PHI3[name]
    m = R._model(**mk)
    _patch(m, recorder, **flags)
    assert R._route(m, recorder, grad=False, **call) == ("stock" if call.get("S", 8) > 32 else "prefill")


@pytest.mark.parametrize("change", ["not linear", "hook", "residual dropout, training mode", "no dropout, training mode",
                                    "attention dropout, training mode"])
def test_modified_phi3_layers_keep_the_stock_forward(recorder, change):
    m = R._model(resid_pdrop=0.1 if change.startswith("residual") else 0.0, **PHI3)
    _patch(m, recorder)
    layer = m.model.layers[0]
    want = "stock"
    if change == "not linear":
        old = layer.self_attn.qkv_proj
        layer.self_attn.qkv_proj = R._NotLinear(old.in_features, old.out_features, bias=False, dtype=old.weight.dtype)
    elif change == "hook":
        layer.mlp.gate_up_proj.register_forward_hook(lambda *a: None)
    else:
        m.train()
        if change.startswith("attention"):
            layer.self_attn.attention_dropout = 0.1
        elif change.startswith("no dropout"):
            want = "train"
    assert R._route(m, recorder, grad=True) == want


def test_switching_the_option_off_restores_the_present_routes(recorder):
    m = R._model(**PHI3)
    _patch(m, recorder)
    assert R._route(m, recorder, grad=True) == "train"
    prefill.enable_fused_prefill(m, train=True)                  # (every switch is set anew by every call)
    assert R._route(m, recorder, grad=True) == "stock"
    prefill.enable_fused_prefill(m, train=True, train_phi3=True)
    assert R._route(m, recorder, grad=True) == "train"
    prefill.disable_fused_prefill(m)
    assert not prefill.is_patched(m.model.layers[0])
    assert R._route(m, recorder, grad=True) == "stock"


def test_the_layout_accessors_name_the_parameters_that_own_the_packed_rows():
    m = R._model(**PHI3)
    layer = m.model.layers[0]
    lo = prefill._layout_of(layer)
    assert lo is prefill._PackedLayout and not lo.TRAINS and prefill.TRAIN_HEAD_DIMS == (64, 128)
    pr = lo.projections(layer)
    assert lo.product(pr, 0)[0] == (layer.self_attn.qkv_proj,) and lo.product(pr, 2)[0] == (layer.mlp.gate_up_proj,)
    assert lo.product(pr, 2)[1].shape[0] // 2 == lo.product(pr, 3)[1].shape[1] == 256     # I, from gate|up and from down
    assert lo.product(pr, 0)[1] is layer.self_attn.qkv_proj.weight
    q = R._model()
    layer = q.model.layers[0]
    lo = prefill._layout_of(layer)
    att, mlp = layer.self_attn, layer.mlp
    pr = lo.projections(layer)
    assert lo is prefill._SplitLayout and lo.product(pr, 2)[1].shape[0] // 2 == lo.product(pr, 3)[1].shape[1] == 256
    assert lo.product(pr, 0)[0] == (att.q_proj, att.k_proj, att.v_proj) and lo.product(pr, 2)[0] == (mlp.gate_proj, mlp.up_proj)


@pytest.mark.parametrize("phi3_on,train_on", [(True, False), (True, True), (False, True), (False, False)])
def test_config_switch_patches_the_u2_phi3_layers_for_the_route(recorder, phi3_on, train_on):
    """`config.u2_fused_phi3_training` implies the training route and reaches enable_fused_prefill as `train_phi3` (off: not passed)."""
    cfg = LM.u2Phi3Config(vocab_size=64, hidden_size=192, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                          num_key_value_heads=2, max_position_embeddings=256, sliding_window=2047, pad_token_id=0, bos_token_id=1,
                          eos_token_id=2)
    cfg.u2_fused_prefill, cfg.u2_fused_decoder_training, cfg.u2_fused_phi3_training = False, train_on, phi3_on
    torch.manual_seed(0)
    m = LM.u2Phi3ForCausalLM(cfg).to(bf).eval()
    layer = m.model.layers[0]
    p0 = next(layer.parameters())
    real = layer.parameters
    layer.parameters = lambda *a, **k: iter([p0.detach().as_subclass(R._FakeCuda)])
    seen = []
    enable = prefill.enable_fused_prefill
    prefill.enable_fused_prefill = lambda model, **kw: (seen.append(kw), enable(model, **kw))[1]
    try:
        with torch.enable_grad():
            m(inputs_embeds=torch.zeros(1, 3, 192, dtype=bf))
    finally:
        prefill.enable_fused_prefill = enable
        layer.parameters = real
    if not (phi3_on or train_on):
        assert seen == [] and not prefill.is_patched(layer)
        return
    assert len(seen) == 1 and seen[0]["train"] is True and seen[0].get("train_phi3", False) is phi3_on
    assert ("train_phi3" in seen[0]) == phi3_on
    assert prefill.is_patched(layer) and layer._u2_prefill.stack.train_phi3 is phi3_on
    layer._calls = recorder
    layer._u2_prefill.orig = types.MethodType(R._stock, layer)
    assert R._route(m, recorder, grad=True) == ("train" if phi3_on else "stock")
