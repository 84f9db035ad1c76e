"""The cases of tests/test_svr_fold_host.py and tests/test_gpu_svr_fold.py: small tokenizers (E = 256, 4 heads, T = 3, N = 24,
Lt = 16, Q = 16, the shipped flavour: DiffTS, gated multi-scale pooling) with "lively" weights, and the SVR folds of their weights
written down independently of the library: W' = W_qkv W_o, b' = W_qkv b_o + b_qkv for every SVR attention behind the first, the
output projection being that of the attention BEFORE it in the order the stack runs them (include/u2tok.h, "FOLD SLOTS")."""
import torch

from u2tokenizer_amd import synth

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
ATTN = {"rma": "rma", "rope": "rope", "mha": "linvt"}   # (every name but rma / rope builds nn.MultiheadAttention)


def case(attn, L, B=1):
    return dict(heads=4, E=256, layers=L, B=B, T=3, N=24, Lt=16, Q=16, top_k=24, use_multi_scale=True, attn_type=ATTN[attn],
                enable_diffts=True, enable_dmtp=True, max_seq_len=512, seed=71 + L, lively=True)


def make(c, dtype=torch.float32):
    """The host module of case c with its name-seeded lively weights, and its state dict under the oracle's prefix"""
    from u2tokenizer_amd.tokenizer import u2Tokenizer
    m = u2Tokenizer(embed_size=c["E"], num_heads=c["heads"], num_layers=c["layers"], top_k=c["top_k"],
                    use_multi_scale=c["use_multi_scale"], num_3d_query_token=c["Q"], hidden_size=c["E"],
                    attn_type=c["attn_type"], enable_diffts=c["enable_diffts"], enable_dmtp=c["enable_dmtp"])
    synth.fill_module_(m, seed=c["seed"], prefix="u2tokenizer.", lively=True)
    m = m.to(dtype)
    return m, {"u2tokenizer." + k: v.detach().clone() for k, v in m.state_dict().items()}


def _attention_names(L):
    """SVR attentions in the order the stack runs them"""
    return [f"u2tokenizer.svt_module.attention_network.layers.{l}.{w}_attention" for l in range(L) for w in ("spatial", "temporal")]


def _qkv_o(sd, p):
    if p + ".in_proj_weight" in sd:
        return sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"], sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"]
    return (torch.cat([sd[f"{p}.{n}.weight"] for n in ("wq", "wk", "wv")]), torch.cat([sd[f"{p}.{n}.bias"] for n in ("wq", "wk", "wv")]),
            sd[p + ".dense.weight"], sd[p + ".dense.bias"])


def folded_state_dict(sd, L):
    """sd with every SVR fold applied IN the weights: attention j >= 1 gets W' / b' as its q | k | v projection, and the attention
    before it the identity as its output projection -- the oracle run on it evaluates the folded stack."""
    out = dict(sd)
    names = _attention_names(L)
    E = sd["u2tokenizer.query_tokens"].shape[-1]
    for j in range(1, len(names)):
        w_qkv, b_qkv = _qkv_o(sd, names[j])[:2]
        w_o, b_o = _qkv_o(sd, names[j - 1])[2:]
        wf, bf = w_qkv @ w_o, w_qkv @ b_o + b_qkv
        if names[j] + ".in_proj_weight" in sd:
            out[names[j] + ".in_proj_weight"], out[names[j] + ".in_proj_bias"] = wf, bf
        else:
            for i, n in enumerate(("wq", "wk", "wv")):
                out[f"{names[j]}.{n}.weight"], out[f"{names[j]}.{n}.bias"] = wf[i * E:(i + 1) * E], bf[i * E:(i + 1) * E]
        o = "out_proj" if names[j - 1] + ".in_proj_weight" in sd else "dense"
        out[f"{names[j - 1]}.{o}.weight"], out[f"{names[j - 1]}.{o}.bias"] = torch.eye(E, dtype=w_o.dtype), torch.zeros_like(b_o)
    return out
