"""The head-dim-96 cases of the flash attention backward (u2tok_attention_gqa_bwd_d96) and their float64 models, shared by the host
and the GPU tests: each model is computed once per process (tests/test_decoder_train_bounds_host.py: attn_bwd_model, the
first-order bounds written out there) and never modified."""
import functools

import test_decoder_train_bounds_host as B

# nb, S, Hq, Hkv, d, key lengths (as passed: values above S are the kernel's to clamp): S on and next to the 32-row wave, 64-row
# tile and 128-row block edges, groups of 1, 2 and 8 query heads, lengths of 1, inside a tile, on its edge and beyond S
D96_CASES = [(3, 1, 2, 1, 96, (1, 6, 1)), (3, 33, 8, 1, 96, (1, 33, 38)), (3, 64, 2, 2, 96, (63, 64, 65)),
             (3, 65, 4, 2, 96, (64, 65, 1)), (3, 129, 2, 1, 96, (128, 129, 64)), (3, 257, 4, 2, 96, (262, 64, 63)),
             (1, 129, 3, 3, 96, None), (2, 257, 2, 1, 96, None)]


def case_id(c):
    return "-".join(str(x).replace(" ", "") for x in c)


@functools.lru_cache(maxsize=None)
def inputs(case):
    nb, S, Hq, Hkv, d, _ = case
    return B.attn_inputs(nb, S, Hq, Hkv, d)


@functools.lru_cache(maxsize=None)
def model(case, lse_given=False):
    nb, S, Hq, Hkv, d, lens = case
    inp = inputs(case)
    return B.attn_bwd_model(inp["qkv"], inp["dout"], Hq, Hkv, d, d ** -0.5, lens, lse_given=lse_given)
