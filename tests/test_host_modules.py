"""CPU: host-side mirror of the reference interface -- state-dict contract, builders, error behaviour, and that
the product path refuses to run without the HIP library / a GPU (no silent fallback)."""
import json
from pathlib import Path
from types import SimpleNamespace as NS

import pytest
import torch

import u2tokenizer_amd as U
from u2tokenizer_amd import language_model as LM

GOLDEN = Path(__file__).resolve().parent / "golden"


def _cfg(**kw):
    base = dict(vision_tower="vit3d", image_channel=1, image_size=[32, 64, 64], patch_size=[4, 16, 16],
                vision_select_layer=-1, vision_select_feature="patch", mm_projector_type="spp", proj_layer_type="mlp",
                proj_layer_num=2, proj_pooling_type="spatial", proj_pooling_size=2, mm_hidden_size=768,
                hidden_size=512, enable_u2tokenizer=True, u2t_num_heads=8, u2t_num_layers=1, u2t_top_k=16,
                use_multi_scale=True, num_3d_query_token=16, attn_type="rma", enable_diffts=True, enable_dmtp=True)
    base.update(kw)
    return NS(**base)


def test_state_dict_keys_match_reference_contract():
    """Key names and shapes recorded from the REFERENCE modules (tests/golden/state_dict_keys.json)."""
    ref = json.loads((GOLDEN / "state_dict_keys.json").read_text())
    c = _cfg()
    got = {}
    for prefix, m in (("vision_tower.", U.build_vision_tower(c)), ("mm_projector.", U.build_mm_projector(c)),
                      ("u2tokenizer.", U.build_u2tokenizer_tower(c))):
        got.update({prefix + k: list(v.shape) for k, v in m.state_dict().items()})
    assert got == ref["mu2_small"]
    c2 = _cfg(attn_type="rope", enable_diffts=False, enable_dmtp=False)
    got = {"u2tokenizer." + k: list(v.shape) for k, v in U.build_u2tokenizer_tower(c2).state_dict().items()}
    assert got == ref["rope_hard_small"]
    # attn_type outside {rma, rope}: stock nn.MultiheadAttention parameters (in_proj_weight / out_proj), svr.py:16-18
    c3 = _cfg(attn_type="linvt")
    got = {"u2tokenizer." + k: list(v.shape) for k, v in U.build_u2tokenizer_tower(c3).state_dict().items()}
    assert got == ref["linvt_small"]


def test_shipped_config_flag_enable_rpe_selects_the_attention_type():
    """base_model_tokenizers/Llama-3.2-1B-Instruct/config.json:21 + u2Tokenizer.py:86-93,422: the shipped code generation
    spells the choice as a boolean; src/model/u2tokenizer/builder.py:12 as `attn_type`."""
    ref = json.loads((GOLDEN / "state_dict_keys.json").read_text())
    keys = lambda c: {"u2tokenizer." + k: list(v.shape) for k, v in U.build_u2tokenizer_tower(c).state_dict().items()}
    on, off = _cfg(enable_rpe=True), _cfg(enable_rpe=False)
    del on.attn_type, off.attn_type
    assert keys(on) == {k: v for k, v in ref["mu2_small"].items() if k.startswith("u2tokenizer.")}
    assert keys(off) == ref["linvt_small"]
    assert keys(_cfg(attn_type="rope", enable_rpe=False, enable_diffts=False, enable_dmtp=False)) == ref["rope_hard_small"]


def test_vit_strict_load_tolerates_the_unused_monai_cls_token():
    """u2_arch.py:64-66 loads M3D-CLIP's pretrained_ViT.bin with strict=True; MONAI <= 1.3.x checkpoints carry an unread
    `patch_embedding.cls_token`.  Both generations load, and what was loaded is what is saved."""
    tower = U.build_vision_tower(_cfg()).vision_tower
    sd = {k: v.clone() for k, v in tower.state_dict().items()}
    assert "patch_embedding.cls_token" not in sd
    tower.load_state_dict(sd, strict=True)                                 # newer MONAI: no such key
    old = dict(sd)
    old["patch_embedding.cls_token"] = torch.full((1, 1, 768), 0.25)
    fresh = U.build_vision_tower(_cfg()).vision_tower
    fresh.load_state_dict(old, strict=True)                                # older MONAI: adopted, never read
    back = fresh.state_dict()
    assert set(back) == set(old) and torch.equal(back["patch_embedding.cls_token"], old["patch_embedding.cls_token"])
    assert not fresh.patch_embedding.cls_token.requires_grad
    assert len(fresh._weights()) == len(tower._weights())                  # the launch table does not see it


def test_fused_prefill_refuses_the_older_decoder_layer_protocol():
    """transformers 4.46 (the reference's pin) .. 4.5x: decoder layers take `past_key_value` and return tuples.  The fused
    layer forward is written for the `past_key_values` / tensor-return protocol; patching the older one would skip every
    cache update.  Such layers stay stock (with one warning)."""
    from u2tokenizer_amd import prefill

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = self.k_proj = self.v_proj = self.o_proj = torch.nn.Linear(8, 8)
            self.head_dim, self.scaling = 8, 1.0

    class Mlp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj = self.up_proj = self.down_proj = torch.nn.Linear(8, 8)

    class OldLayer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn, self.mlp = Attn(), Mlp()
            self.input_layernorm = self.post_attention_layernorm = torch.nn.LayerNorm(8)

        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, use_cache=False,
                    position_embeddings=None, **kwargs):
            return (hidden_states,)

    class NewLayer(OldLayer):
        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                    position_embeddings=None, **kwargs) -> torch.Tensor:
            return hidden_states

    class Base(torch.nn.Module):
        def __init__(self, cls):
            super().__init__()
            self.layers = torch.nn.ModuleList([cls(), cls()])

    prefill._warned_protocol[0] = False
    with pytest.warns(UserWarning, match="decoder layer protocol"):
        assert prefill.enable_fused_prefill(Base(OldLayer)) == 0
    new = Base(NewLayer)
    assert prefill.enable_fused_prefill(new) == 2
    # a patched layer still hands anything it does not take (CPU tensors here) to its own forward
    assert new.layers[0](torch.zeros(1, 2, 8)) is not None
    prefill.disable_fused_prefill(new)


def test_float16_parameters_select_the_half_build():
    """evalscipt/ourmodel_amos.py:33 loads the model in float16.  The path modules then run the IEEE-half build of the library
    (libu2tok_hip_f16.so: same sources, same C ABI, u2tok_elem() == "f16") on the fp16 parameters themselves -- no bf16 copy of
    the weights (round 4 kept one: VERDICT r4 #2).  On the host: both builds load side by side and say what they are, the
    element type of an op follows its tensors / the module's parameters, nothing falls back to the CPU, training in fp16 is
    refused."""
    from u2tokenizer_amd import _lib, ops
    hb, hh = _lib.load_library("bf16"), _lib.load_library("f16")
    assert hb.u2tok_elem() == b"bf16" and hh.u2tok_elem() == b"f16" and hb is not hh
    assert _lib.load_library() is hb                                   # outside an op: bf16
    prev = _lib.set_thread_elem("f16")
    try:
        assert _lib.load_library() is hh and ops.elem_dtype() == torch.float16
    finally:
        _lib.set_thread_elem(prev)
    assert ops.elem_dtype() == torch.bfloat16
    tok = U.build_u2tokenizer_tower(_cfg()).half().eval()
    assert not hasattr(tok, "_fp16_twin") and all(p.dtype == torch.float16 for p in tok.parameters())
    tok.requires_grad_(False)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU tensor"):   # no CPU fallback, whatever the element type
        tok(v_token=torch.zeros(1, 2, 16, 512, dtype=torch.float16), t_token=torch.zeros(1, 8, 512, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="inference only"):
        ops.training_needs_bf16(torch.float16, "u2Tokenizer")
    ops.training_needs_bf16(torch.bfloat16, "u2Tokenizer")


def test_builders_raise_like_the_reference():
    with pytest.raises(ValueError, match="Unknown vision tower"):
        U.build_vision_tower(_cfg(vision_tower="resnet"))
    with pytest.raises(ValueError, match="Unknown projector type"):
        U.build_mm_projector(_cfg(mm_projector_type="qformer"))
    with pytest.raises(AssertionError):
        U.build_u2tokenizer_tower(_cfg(hidden_size=100, u2t_num_heads=8))
    assert U.build_mm_projector(_cfg()).proj_out_num == 16
    assert U.build_vision_tower(_cfg()).hidden_size == 768


def test_no_cpu_fallback():
    tok = U.build_u2tokenizer_tower(_cfg()).bfloat16()
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU tensor"):
        tok(v_token=torch.zeros(1, 2, 16, 512, dtype=torch.bfloat16), t_token=torch.zeros(1, 8, 512, dtype=torch.bfloat16))
    with torch.enable_grad(), pytest.raises(RuntimeError, match="GPU tensor"):  # the training path has no CPU fallback either
        tok(v_token=torch.zeros(1, 2, 16, 512, dtype=torch.bfloat16), t_token=torch.zeros(1, 8, 512, dtype=torch.bfloat16))


def test_product_never_imports_the_oracle():
    import re
    root = Path(U.__file__).resolve().parent
    for f in list(root.rglob("*.py")) + list(root.rglob("*.hip")) + list(root.rglob("*.h")):
        assert not re.search(r"^\s*(from|import)\s+oracle|u2_oracle", f.read_text(), flags=re.M), f


def test_hf_surface_and_early_outs():
    from cases import FULL_CASES
    c = FULL_CASES["cfg1"]
    cfg = LM.u2Config(**c["llama"])
    for k, v in c["mm"].items():
        setattr(cfg, k, v)
    m = LM.u2LlamaForCausalLM(cfg).eval()
    assert m.get_model().get_u2tokenizer() is not None and m.get_vision_tower() is not None
    ids = torch.randint(0, cfg.vocab_size, (1, 12))
    # no images -> plain LM path on CPU (u2_arch.py:101-102), same return contract
    r = m.prepare_inputs_for_multimodal(ids, None, None, None, None, None, None)
    assert r[0] is ids and r[4] is None
    r = m.prepare_inputs_for_multimodal(ids[:, :1], None, None, None, None, torch.zeros(1), None)
    assert r[0].shape[1] == 1 and r[4] is None
    with torch.no_grad():
        out = m(input_ids=ids)
    assert out.logits.shape == (1, 12, cfg.vocab_size)
    with pytest.raises(NotImplementedError):
        m.generate(None, ids, inputs_embeds=torch.zeros(1, 2, 512))
    from transformers import AutoConfig
    assert isinstance(AutoConfig.for_model("u2llama"), LM.u2Config)
    q = LM.u2Qwen3ForCausalLM(LM.u2Qwen3Config(vocab_size=64, hidden_size=64, intermediate_size=128,
                                               num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                               head_dim=16))
    assert q.get_vision_tower() is None
    # the third surface of the reference (language_model/u2phi3.py:25-140, train_stage1.py:290-296)
    pc = LM.u2Phi3Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                         num_key_value_heads=2, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    for k, v in c["mm"].items():
        if k != "hidden_size":
            setattr(pc, k, v)
    ph = LM.u2Phi3ForCausalLM(pc).eval()
    assert isinstance(AutoConfig.for_model("u2phi3"), LM.u2Phi3Config) and ph.get_model() is ph.model
    with torch.no_grad():
        assert ph(input_ids=ids % 64).logits.shape == (1, 12, 64)
    r = ph.prepare_inputs_for_multimodal(ids, None, None, None, None, None, None)
    assert r[0] is ids and r[4] is None
    # its decoder layers have another layout (qkv_proj / gate_up_proj): the fused prefill declines them instead of raising
    from u2tokenizer_amd.prefill import enable_fused_prefill
    assert enable_fused_prefill(ph, strict=False) == 0
    with pytest.raises(RuntimeError, match="unsupported decoder layer"):
        enable_fused_prefill(ph)


def test_packed_weight_alias_is_a_view_and_routes_gradients():
    """autograd._cat_rows: parameters that lie back to back in one storage (pack_weights) are stacked WITHOUT a copy and the
    gradient of the stacked matrix is handed back row block by row block; anything else falls back to torch.cat."""
    from u2tokenizer_amd import autograd as AG
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    try:
        buf = torch.arange(3 * 4 * 6, dtype=torch.float32).view(12, 6).clone()
        parts = [torch.nn.Parameter(torch.empty(0)) for _ in range(3)]
        for i, p in enumerate(parts):
            p.data = buf[4 * i:4 * (i + 1)]
        W = AG._cat_rows(parts)
        assert W.shape == (12, 6) and W.data_ptr() == buf.data_ptr(), "adjacent parameters must alias, not copy"
        assert torch.equal(W.detach(), buf)
        G = torch.randn(12, 6)
        (W * G).sum().backward()
        for i, p in enumerate(parts):
            assert torch.equal(p.grad, G[4 * i:4 * (i + 1)])
        # a gap between the parts, or separate storages: plain torch.cat (a copy) with the same values and gradients
        loose = [torch.nn.Parameter(torch.randn(4, 6)) for _ in range(3)]
        W2 = AG._cat_rows(loose)
        assert W2.data_ptr() not in [p.data_ptr() for p in loose]
        assert torch.equal(W2.detach(), torch.cat([p.detach() for p in loose], 0))
        gap = [torch.nn.Parameter(torch.empty(0)) for _ in range(2)]
        gap[0].data, gap[1].data = buf[0:4], buf[8:12]
        assert AG._cat_rows(gap).data_ptr() != buf.data_ptr()
        # in-place optimiser updates stay visible through the alias
        with torch.no_grad():
            parts[1].add_(1.0)
        assert torch.equal(AG._cat_rows(parts).detach()[4:8], parts[1].detach())
    finally:
        torch.set_grad_enabled(prev)


def test_fused_prefill_patch_is_inert_off_the_gpu_and_packs_losslessly():
    """u2tokenizer_amd/prefill.py on the host: patched decoder layers take their stock forward (CPU tensors), packing q|k|v and
    gate|up into one buffer keeps every parameter's value / name / shape (the stock modules keep working on the views), and
    disable_fused_prefill restores the original methods."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from u2tokenizer_amd import prefill as P
    torch.manual_seed(0)
    cfg = Qwen3Config(vocab_size=128, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=64, max_position_embeddings=64)
    m = Qwen3ForCausalLM(cfg).eval()
    x = torch.randn(1, 9, 128)
    with torch.no_grad():
        ref = m(inputs_embeds=x).logits
        assert P.enable_fused_prefill(m) == 2 and P.enable_fused_prefill(m) == 0      # idempotent
        assert torch.equal(m(inputs_embeds=x).logits, ref)                            # CPU: the stock layers ran
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        att = m.model.layers[0].self_attn
        W, b = P._pack((att.q_proj, att.k_proj, att.v_proj))
        assert b is None and W.shape == (128 + 64 + 64, 128)
        assert att.k_proj.weight.data_ptr() == att.q_proj.weight.data_ptr() + att.q_proj.weight.numel() * 4
        assert torch.equal(W[:128], sd["model.layers.0.self_attn.q_proj.weight"])
        assert torch.equal(W[192:], sd["model.layers.0.self_attn.v_proj.weight"])
        W2, _ = P._pack((att.q_proj, att.k_proj, att.v_proj))                         # already packed: the same buffer
        assert W2.data_ptr() == W.data_ptr()
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k
        assert torch.equal(m(inputs_embeds=x).logits, ref)
        P.disable_fused_prefill(m)
        assert not P.is_patched(m.model.layers[0]) and torch.equal(m(inputs_embeds=x).logits, ref)


def test_frozen_tower_feature_sharing_logic():
    """ViT3DTower's opt-in cache of the last features (the DPO step's second pass over the same images with a
    frozen tower): host logic only -- the tower's compute is stubbed.  Byte-identical input + unchanged frozen weights -> the
    cached features; a trainable tower, another image or an in-place weight update -> computed again."""
    tower = U.build_vision_tower(_cfg())
    calls = []

    def fake(x, keep_cls):
        calls.append(keep_cls)
        return x.float().sum().reshape(1) + tower.vision_tower.norm.weight.sum()

    tower.vision_tower.forward_features = fake
    img = torch.rand(2, 1, 32, 64, 64)
    tower.share_frozen_features = True
    a, b = tower(img), tower(img.clone())
    assert len(calls) == 2                                  # trainable tower: never cached
    tower.requires_grad_(False)
    a, b = tower(img), tower(img.clone())
    assert len(calls) == 3 and torch.equal(b, a) and b is not a     # (a copy: in-place ops downstream cannot reach the cache)
    b.add_(1.0)
    assert torch.equal(tower(img), a) and len(calls) == 3
    c = tower(img + 1)
    assert len(calls) == 4 and not torch.equal(c, a)
    with torch.no_grad():
        tower.vision_tower.norm.weight.add_(1.0)
    d = tower(img + 1)
    assert len(calls) == 5 and not torch.equal(d, c)
    # a write through .data does not bump the version counter (an optimiser's copy-out): the whole-model paths that do such
    # writes drop the cache, anything else calls invalidate_feature_cache()
    tower.vision_tower.norm.weight.data.add_(1.0)
    assert torch.equal(tower(img + 1), d) and len(calls) == 5         # (undetectable, documented)
    tower.invalidate_feature_cache()
    e = tower(img + 1)
    assert len(calls) == 6 and not torch.equal(e, d)
    tower.load_state_dict(tower.state_dict())
    tower(img + 1)
    tower.double()
    tower(img + 1)
    assert len(calls) == 8
    calls.clear(); calls.extend([0] * 5)
    tower.share_frozen_features = False
    tower(img + 1)
    assert len(calls) == 6


def test_append_in_place_cache_layer_behaves_like_dynamic_layer():
    """prefill._append_layer_class(): the KV-cache layer the fused prefill installs in a plain DynamicCache -- appends in place into
    doubling buffers; every observable (returned keys / values, lengths, crop, batch selection followed by further updates) equals
    HF's DynamicLayer, whose `update` is a torch.cat."""
    from transformers.cache_utils import DynamicLayer
    from u2tokenizer_amd.prefill import _append_layer_class
    a, d = _append_layer_class()(), DynamicLayer()
    g = torch.Generator().manual_seed(0)

    def step(B, n):
        k, v = torch.randn(B, 3, n, 8, generator=g), torch.randn(B, 3, n, 8, generator=g)
        (ka, va), (kd, vd) = a.update(k, v), d.update(k, v)
        assert torch.equal(ka, kd) and torch.equal(va, vd) and a.get_seq_length() == d.get_seq_length()

    for n in (5, 1, 1, 300, 1, 1):
        step(2, n)
    assert a._kb.shape[2] >= 309 and a.keys.data_ptr() == a._kb.data_ptr()      # in place: a view of the buffer
    a.crop(-2), d.crop(-2)
    step(2, 1)
    a.batch_select_indices(torch.tensor([1])), d.batch_select_indices(torch.tensor([1]))
    step(1, 2)
    a.batch_repeat_interleave(3), d.batch_repeat_interleave(3)
    step(3, 1)



def test_gelu_logistic_polynomial_accuracy_over_all_bf16_inputs():
    """csrc/common.h: gelu_fast = x / (1 + 2^(x P(x^2))), P of degree 4 (round 6: 12 instructions per pair of values instead of the 20 of
    the Abramowitz & Stegun 7.1.28 form).  Its arithmetic restated in numpy float32 (fma = one rounding of the float64 result; exp2 / rcp
    correctly rounded here, one ulp on the hardware), over EVERY finite bf16 input with |x| <= 30, against float64 x Phi(x): the table
    the header quotes.  The GPU side of the same check is tests/test_gpu_ops.py::test_gelu_fwd_over_all_bf16_inputs."""
    import numpy as np
    from scipy.special import ndtr
    f32 = np.float32
    bits = np.arange(65536, dtype=np.uint32)
    x = (bits << np.uint32(16)).view(f32)
    x = x[np.isfinite(x) & (np.abs(x) <= 30)]

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(f32)

    x2 = (x * x).astype(f32)
    p = np.full_like(x, f32(-3.2607881621515844e-06))
    for c in (8.898991654859856e-05, 0.0003546576772350818, -0.10521142929792404, -2.3020575046539307):
        p = fma(p, x2, f32(c))
    with np.errstate(over="ignore"):
        e = np.exp2((p * x).astype(f32).astype(np.float64)).astype(f32)
        y = (x * (f32(1) / (f32(1) + e).astype(f32)).astype(f32)).astype(f32)
    ref = x.astype(np.float64) * ndtr(x.astype(np.float64))
    assert np.abs(y - ref).max() <= 4e-6
    to_bf = lambda v: torch.from_numpy(v.astype(f32)).bfloat16().float().numpy()   # noqa: E731
    big = np.abs(ref) >= 1e-2
    yb, rb = to_bf(y), to_bf(ref.astype(f32))
    ulp = 2.0 ** (np.floor(np.log2(np.abs(rb[big]))) - 7)
    assert (np.abs(yb[big] - rb[big]) <= ulp).all()                                   # never more than one ulp
    assert (yb[big] != rb[big]).mean() <= 2e-3                                          # ... and for 0.09 % of the inputs
    yh, rh = y.astype(np.float16), ref.astype(f32).astype(np.float16)
    assert (yh[big] != rh[big]).mean() <= 1.5e-2                                        # fp16 outputs: 1.0 %
    # saturation: exact identity / exact zero for large |x|, no NaN from the overflowing exponent
    big_x = np.array([40.0, 1e4, 3e38, -40.0, -1e4, -3e38], dtype=f32)
    x2 = (big_x * big_x).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.full_like(big_x, f32(-3.2607881621515844e-06))
        for c in (8.898991654859856e-05, 0.0003546576772350818, -0.10521142929792404, -2.3020575046539307):
            p = fma(p, x2, f32(c))
        e = np.exp2(np.clip((p * big_x).astype(np.float64), -1e4, 1e4)).astype(f32)
        y = big_x * (f32(1) / (f32(1) + e))
    assert (y[:3] == big_x[:3]).all() and (y[3:] == 0).all()
