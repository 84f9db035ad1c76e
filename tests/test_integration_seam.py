"""INTEGRATION.md section A, checked mechanically (VERDICT r5 missing #7): the reference's `u2_arch.py` drives this package's
factories (`u2_arch.py:6-8`), and `u2MetaModel.__init__` (`u2_arch.py:10-19`), `initialize_vision_modules` (`:29-78`) and
`u2LlamaForCausalLM` (`language_model/u2llama.py:19-38`) construct the path -- here through this package's drop-ins of those
three (`u2tokenizer_amd/arch.py`, `u2tokenizer_amd/language_model.py`).  The reference side is RECORDED in
tests/golden/integration_seam.json (tests/golden/make_integration_seam.py runs the unswapped reference from the same
arguments): the state dict of the model it builds, its module classes, the two properties it reads off the modules
(`vision_tower.hidden_size`, `u2_arch.py:68`; `mm_projector.proj_out_num`, `train_stage1.py:369`) and its builders' errors.
Asserted: the modules built are this package's and carry the reference's class names, a checkpoint of the reference's layout
loads with strict=True (key for key, shape for shape), the `pretrain_vision_model` / `pretrain_mm_mlp_adapter` branches
(`u2_arch.py:64-66,74-78`) load strictly, and the properties have the reference's values.

CPU only.  No forward is run (the product has no CPU path)."""
import json
import re
from pathlib import Path
from types import SimpleNamespace as NS

import pytest
import torch

from u2tokenizer_amd import language_model as LM

FIXTURE = Path(__file__).resolve().parent / "golden" / "integration_seam.json"

MODEL_ARGS = dict(image_channel=1, image_size=[32, 64, 64], patch_size=[4, 16, 16], vision_tower="vit3d", vision_select_layer=-1,
                  vision_select_feature="patch", mm_projector_type="spp", proj_layer_type="mlp", proj_layer_num=2,
                  proj_pooling_type="spatial", proj_pooling_size=2, enable_u2tokenizer=True, u2t_num_heads=4, u2t_num_layers=2,
                  u2t_top_k=16, use_multi_scale=True, num_3d_query_token=16, attn_type="rma", enable_diffts=True, enable_dmtp=True,
                  freeze_vision_tower=False, pretrain_vision_model=None, pretrain_mm_mlp_adapter=None)
LLAMA = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4,
             num_key_value_heads=2, max_position_embeddings=256, pad_token_id=0, bos_token_id=1, eos_token_id=2)


@pytest.fixture(scope="module")
def ref():
    """What the unswapped reference built from MODEL_ARGS / LLAMA (tests/golden/make_integration_seam.py)."""
    rec = json.loads(FIXTURE.read_text())
    assert rec["model_args"] == MODEL_ARGS and rec["llama"] == LLAMA, "stale fixture: rerun tests/golden/make_integration_seam.py"
    return rec


def _construct(args):
    cfg = LM.u2Config(**LLAMA)
    torch.manual_seed(0)
    m = LM.u2LlamaForCausalLM(cfg)
    assert m.get_model().get_vision_tower() is None    # (a bare Llama config: u2_arch.py:16 finds no `vision_tower`)
    m.get_model().initialize_vision_modules(NS(**args))
    return m


def _reference_state_dict(ref):
    """A checkpoint of the reference's layout: the recorded keys and shapes, seeded values."""
    g = torch.Generator().manual_seed(0)
    return {k: torch.randn(shape, generator=g) for k, shape in sorted(ref["state_dict"].items())}


def test_arch_constructs_the_reference_checkpoint_layout(ref, tmp_path):
    m = _construct(MODEL_ARGS)
    mm = m.get_model()
    for name in ("vision_tower", "mm_projector", "u2tokenizer"):
        mod = getattr(mm, name)
        assert type(mod).__module__.startswith("u2tokenizer_amd."), (name, type(mod))
        assert type(mod).__name__ == ref["classes"][name]
    # the reference's checkpoint, key for key and shape for shape
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["state_dict"]
    sd_ref = _reference_state_dict(ref)
    sd_ref = {k: v.to(m.state_dict()[k].dtype) for k, v in sd_ref.items()}
    missing, unexpected = m.load_state_dict(sd_ref, strict=True)
    assert not missing and not unexpected
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd_ref[k]), k
    # what the reference reads off the modules
    assert mm.vision_tower.hidden_size == ref["vision_hidden_size"] == 768 == mm.config.mm_hidden_size == ref["mm_hidden_size"]
    assert mm.mm_projector.proj_out_num == ref["proj_out_num"] == 2 * 2 * 4
    assert m.get_u2tokenizer() is mm.u2tokenizer and m.get_vision_tower() is mm.vision_tower
    # a config that already names a vision tower takes the constructor route (u2_arch.py:16-18) -- what from_pretrained does
    cfg2 = LM.u2Config(**LLAMA)
    for k, v in MODEL_ARGS.items():
        setattr(cfg2, k, v)
    cfg2.mm_hidden_size = 768
    m2 = LM.u2LlamaForCausalLM(cfg2)
    assert type(m2.get_model().vision_tower).__module__.startswith("u2tokenizer_amd.")
    assert type(m2.get_model().mm_projector).__module__.startswith("u2tokenizer_amd.")

    # pretrain_vision_model / pretrain_mm_mlp_adapter (u2_arch.py:64-66,74-78): files in the layout the REFERENCE's modules save
    vit_prefix, proj_prefix = "model.vision_tower.vision_tower.", "model.mm_projector."
    vit_sd = {k[len(vit_prefix):]: v + 1.0 for k, v in sd_ref.items() if k.startswith(vit_prefix)}
    proj_sd = {k: v + 2.0 for k, v in sd_ref.items() if k.startswith(proj_prefix)}
    assert vit_sd and proj_sd
    vit_file, proj_file = tmp_path / "pretrained_ViT.bin", tmp_path / "mm_projector.bin"
    torch.save(vit_sd, vit_file)
    torch.save(proj_sd, proj_file)
    m3 = _construct(dict(MODEL_ARGS, pretrain_vision_model=str(vit_file), pretrain_mm_mlp_adapter=str(proj_file)))
    got = m3.get_model().vision_tower.vision_tower.state_dict()
    assert sorted(got) == sorted(vit_sd)
    for k, v in got.items():
        assert torch.equal(v, vit_sd[k]), k
    got = m3.get_model().mm_projector.state_dict()
    assert sorted(got) == sorted(k[len(proj_prefix):] for k in proj_sd)
    for k, v in got.items():
        assert torch.equal(v, proj_sd[proj_prefix + k]), k


def test_arch_error_behaviour_like_the_reference(ref):
    """Unknown tower / projector names raise the reference's ValueError (builder.py of both packages)."""
    with pytest.raises(ValueError, match="^" + re.escape(ref["errors"]["vision_tower"]) + "$"):
        _construct(dict(MODEL_ARGS, vision_tower="resnet"))
    with pytest.raises(ValueError, match="^" + re.escape(ref["errors"]["mm_projector"]) + "$"):
        _construct(dict(MODEL_ARGS, mm_projector_type="qformer"))
