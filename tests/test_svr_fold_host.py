"""CPU: the SVR folds (include/u2tok.h, "FOLD SLOTS") as algebra and as host plumbing.

In float64, with the oracle: the SVR stack evaluated with (W', b') in place of every q | k | v projection behind the first -- and no
output projection in front of it -- equals st_attention_layer chained, which pins WHICH projection folds into which, biases included.
On the module: the folds are plain attributes (state_dict() keys unchanged), in the order the stack runs its attentions."""
import json
from pathlib import Path

import pytest
import torch

from oracle import u2_oracle as O
from helpers import tok_cfg
from svr_fold_cases import _attention_names, case, folded_state_dict, make

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("attn", ["rma", "rope", "mha"])
def test_folded_stack_equals_the_chained_layers_in_float64(attn, L):
    c = case(attn, L, B=2)
    _, sd = make(c, torch.float64)
    folded = folded_state_dict(sd, L)
    names = _attention_names(L)
    changed = sorted(k for k in sd if not torch.equal(sd[k], folded[k]))
    assert len(changed) == (2 * L - 1) * (4 if attn == "mha" else 8), changed   # every fold replaced its q | k | v and the o before it
    assert not any(k.startswith(names[0] + ".w") or k.startswith(names[0] + ".in_proj") for k in changed)   # the first q | k | v stays
    assert not any(k.startswith(names[-1] + ".dense") or k.startswith(names[-1] + ".out_proj") for k in changed)  # and the last o
    x = torch.randn((c["B"], c["T"], c["N"], c["E"]), generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    cfg = tok_cfg(c)

    def stack(s):
        y = x
        for l in range(L):
            y = O.st_attention_layer(s, f"u2tokenizer.svt_module.attention_network.layers.{l}", y, cfg)
        return y

    want, got = stack(sd), stack(folded)
    assert want.pow(2).mean().sqrt() > 1e-3                              # (a live stack: nothing collapsed to zero)
    rel = ((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()
    print(f"{attn} L={L}: folded vs chained, relative RMS {rel:.3e}")
    assert rel <= 1e-10, rel


@pytest.mark.parametrize("attn", ["rma", "mha"])
def test_module_runs_its_attentions_in_fold_order(attn):
    m, _ = make(case(attn, 3))
    names = {id(mod): "u2tokenizer." + n for n, mod in m.named_modules()}
    assert [names[id(a)] for a in m._svr_chain()] == _attention_names(3)
    assert m._fold_slots() == [None] * (2 * 5)                           # no folds on the host: every slot null, two per fold


def test_folds_are_plain_attributes():
    """state_dict() keys after pack_weights() are those of tests/golden/state_dict_keys.json; a fold, once there, is neither a
    parameter nor a buffer, and .to() drops it."""
    from test_checkpoint import _modules
    m = _modules()
    want = json.loads((GOLDEN / "state_dict_keys.json").read_text())["mu2_small"]
    tok = m.u2tokenizer
    tok._packed_key = None
    tok.pack_weights()
    assert tok._folds is None                                            # host parameters: packed, never folded
    E, n = tok.embed_size, 2 * tok.num_layers - 1
    tok._folds = [(torch.zeros(3 * E, E), torch.zeros(3 * E)) for _ in range(n)]
    tok._fold_key = tok._fold_versions()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == want
    assert len(tok._fold_slots()) == 2 * n and all(t is not None for t in tok._fold_slots())
    assert not any("fold" in k for k, _ in list(tok.named_parameters()) + list(tok.named_buffers()))
    before = tok._fold_versions()
    with torch.no_grad():
        tok.svt_module.attention_network.layers[0].spatial_attention.dense.weight.mul_(2.0)
    assert tok._fold_versions() != before                                # an in-place write is seen
    m.to(torch.float64)
    assert tok._folds is None and tok._fold_slots() == [None] * (2 * n)
