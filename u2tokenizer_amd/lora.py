"""LoRA adapters on the decoder's projections, without peft.

The reference fine-tunes the decoder with peft's LoRA (train_stage1.py: r = 16, alpha = 32, dropout = 0.05, bias "none", every
nn.Linear of the LLM backbone) and saves the wrapped model's state dict.  `LoRALinear` has the attribute layout and the
state-dict keys of peft's `lora.Linear` (`base_layer`, `lora_A` / `lora_B` / `lora_dropout` module dicts keyed by adapter name,
`scaling` / `r` / `lora_alpha` dicts, `active_adapters`, `merged`, `disable_adapters`), so that such a file loads into a model
wrapped by `add_lora` and the training route (decoder_train.LoraDeltaFn; `adapter_of` below is its admission test) treats both
alike.  The layout was taken from peft's published source and is not verified against an installed peft.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import torch
from torch import nn

RANKS = (16, 32, 64)                     # what the adapter kernels compute (csrc/lora.hip)
ADAPTER_DTYPES = (torch.bfloat16, torch.float32)
_HOOK_TABLES = ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks")
# per-adapter variants of peft's lora.Linear that change what forward computes: set or non-empty for the adapter = not computed here
_VARIANTS = ("use_dora", "lora_variant", "lora_bias", "fan_in_fan_out", "lora_magnitude_vector", "lora_embedding_A")
PEFT_PREFIX = "base_model.model."


class LoRALinear(nn.Module):
    """base(x) + lora_B(lora_A(dropout(x))) * scaling, the branch in the adapter weights' dtype (peft's lora.Linear.forward)."""

    def __init__(self, base_layer: nn.Linear, r: int = 16, lora_alpha: float = 32, lora_dropout: float = 0.05,
                 adapter_name: str = "default", adapter_dtype: Optional[torch.dtype] = None):
        super().__init__()
        if type(base_layer) is not nn.Linear:
            raise TypeError(f"LoRALinear wraps torch.nn.Linear, got {type(base_layer).__name__}")
        if r < 1:
            raise ValueError("r must be positive")
        self.base_layer = base_layer
        self.in_features, self.out_features = base_layer.in_features, base_layer.out_features
        w = base_layer.weight
        dt = adapter_dtype or w.dtype
        self.lora_A = nn.ModuleDict({adapter_name: nn.Linear(self.in_features, r, bias=False, device=w.device, dtype=dt)})
        self.lora_B = nn.ModuleDict({adapter_name: nn.Linear(r, self.out_features, bias=False, device=w.device, dtype=dt)})
        self.lora_dropout = nn.ModuleDict({adapter_name: nn.Dropout(p=lora_dropout) if lora_dropout > 0 else nn.Identity()})
        self.r = {adapter_name: r}
        self.lora_alpha = {adapter_name: lora_alpha}
        self.scaling = {adapter_name: lora_alpha / r}
        self.active_adapters = [adapter_name]
        self.merged = False
        self.disable_adapters = False
        nn.init.kaiming_uniform_(self.lora_A[adapter_name].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B[adapter_name].weight)

    @property
    def weight(self):
        return self.base_layer.weight

    @property
    def bias(self):
        return self.base_layer.bias

    def forward(self, x):
        result = self.base_layer(x)
        if self.disable_adapters or self.merged:
            return result
        out_dtype = result.dtype
        for name in self.active_adapters:
            if name not in self.lora_A:
                continue
            A, B = self.lora_A[name], self.lora_B[name]
            xa = x.to(A.weight.dtype)
            result = result + B(A(self.lora_dropout[name](xa))) * self.scaling[name]
        return result.to(out_dtype)

    def delta_weight(self, name: str) -> torch.Tensor:
        """scaling * B A in fp32 (out_features, in_features)."""
        return (self.lora_B[name].weight.float() @ self.lora_A[name].weight.float()) * self.scaling[name]


def _decoder_layers(model):
    base = model.get_model() if hasattr(model, "get_model") else getattr(model, "model", model)
    layers = getattr(base, "layers", None)
    if layers is None:
        raise RuntimeError("no decoder layers found (expected an HF Llama / Qwen3 / Phi-3 model)")
    return layers


def add_lora(model, r: int = 16, alpha: float = 32, dropout: float = 0.05, target_modules: Optional[Iterable[str]] = None,
             adapter_dtype: Optional[torch.dtype] = None) -> int:
    """Wrap the nn.Linear modules inside the decoder layers (all of them, or those whose attribute name is in `target_modules`,
    e.g. ("q_proj", "v_proj")) in LoRALinear -- A Kaiming-uniform, B zero: the wrapped model computes what it did --, freeze
    every parameter of `model` that is not an adapter's, and return the number of modules wrapped.  adapter_dtype: the dtype of A
    and B (default: the base weight's)."""
    targets = None if target_modules is None else set(target_modules)
    todo = []
    for layer in _decoder_layers(model):
        inside = {id(s) for w in layer.modules() if isinstance(w, LoRALinear) for s in w.modules()}   # (already wrapped)
        for parent in layer.modules():
            if id(parent) in inside:
                continue
            for name, child in parent.named_children():
                if type(child) is nn.Linear and (targets is None or name in targets):
                    todo.append((parent, name, child))
    for parent, name, child in todo:
        setattr(parent, name, LoRALinear(child, r=r, lora_alpha=alpha, lora_dropout=dropout, adapter_dtype=adapter_dtype))
    for n, p in model.named_parameters():
        p.requires_grad_(".lora_A." in n or ".lora_B." in n)
    return len(todo)


def merge_lora(model) -> int:
    """Fold scaling * B A of every active adapter into its base weight (in place, so weights that are views of the packed q|k|v and
    gate|up buffers of prefill._pack stay views of them) and put the plain nn.Linear back; returns the number of modules unwrapped."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if not isinstance(child, LoRALinear):
                continue
            base = child.base_layer
            if not child.merged and not child.disable_adapters:
                with torch.no_grad():
                    w = base.weight.data
                    total = w.float()
                    for a in child.active_adapters:
                        if a in child.lora_A:
                            total = total + child.delta_weight(a).to(w.device)
                    w.copy_(total.to(w.dtype))
            setattr(parent, name, base)
            n += 1
    return n


def load_lora_state_dict(model, sd, strict: bool = True):
    """Load a state dict with peft's key names (`...q_proj.base_layer.weight`, `...q_proj.lora_A.default.weight`), with or without
    peft's `base_model.model.` prefix, into a model wrapped by `add_lora`.  strict: every adapter key of the file and of the
    model must find its partner (base weights may be absent: peft's adapter-only files)."""
    clean = {(k[len(PEFT_PREFIX):] if k.startswith(PEFT_PREFIX) else k): v for k, v in sd.items()}
    res = model.load_state_dict(clean, strict=False)
    if strict:
        bad = [k for k in res.unexpected_keys] + [k for k in res.missing_keys if ".lora_A." in k or ".lora_B." in k]
        if bad:
            raise RuntimeError(f"load_lora_state_dict: keys without a partner: {bad[:8]}{' ...' if len(bad) > 8 else ''}")
    return res


# ------------------------------------------------------------------------------------------------ the route's admission test
class Adapter:
    """One projection's adapter as the training route computes it."""
    __slots__ = ("base", "A", "B", "dropout", "scaling", "r")

    def __init__(self, base, A, B, dropout, scaling, r):
        self.base, self.A, self.B, self.dropout, self.scaling, self.r = base, A, B, dropout, scaling, r


def _present(m, attr: str) -> bool:
    return attr in m.__dict__ or attr in m._modules or attr in m._parameters or attr in m._buffers or hasattr(type(m), attr)


def _set_for(v, name: str) -> bool:
    """Whether a variant attribute is set for adapter `name`: a mapping (dict, ModuleDict, ParameterDict) by its entry, anything
    else by its truth value."""
    if v is None:
        return False
    if hasattr(v, "keys") and hasattr(v, "__getitem__"):
        if name not in v:
            return False
        e = v[name]
        return True if isinstance(e, (nn.Module, torch.Tensor)) else bool(e)
    return bool(v)


def adapter_of(m) -> Optional[Adapter]:
    """`m` as an adapter the training route computes, duck-typed on the layout of peft's lora.Linear (no import of peft), else None:
    one active adapter, not merged, not disabled; base exactly nn.Linear; lora_A / lora_B exactly bias-free nn.Linear of one dtype,
    bf16 or fp32, in the shapes (r, in) / (out, r); r in RANKS; in and out features multiples of 32 (the kernels' contraction
    steps); a dropout module that does not work in place (the route calls it as the stock forward does, so any module is
    computed as itself); no hooks on the wrapper, the base layer, A or B; none of
    _VARIANTS set for the adapter.  Any attribute that cannot be read as expected gives None: a layout that is not understood is
    never computed as if it were."""
    return _read(m, off=False)


def base_only_of(m) -> Optional[nn.Linear]:
    """The base layer of a wrapper that computes its base layer ALONE -- `merged` or `disable_adapters` set (peft's forward returns
    base_layer(x) then: the null-reference pass of DPO, a merged model that kept its wrappers) -- and that satisfies every other rule
    of `adapter_of` (same base type, same hook rules, same _VARIANTS rules, a readable single active adapter), else None.  The no-grad
    routes of prefill.py count such a projection as its base nn.Linear."""
    a = _read(m, off=True)
    return None if a is None else a.base


def dropout_inactive(drop) -> bool:
    """Whether an adapter's dropout module is the identity in this call: nn.Identity, p == 0, or not in training mode (peft applies
    dropout in train mode even under no_grad; the no-grad routes leave such a call to the stock forward)."""
    if type(drop) is nn.Identity:
        return True
    if type(drop) is nn.Dropout:
        return drop.p == 0 or not drop.training
    return False


def _read(m, off: bool) -> Optional[Adapter]:
    """adapter_of's reading of the layout; off: the wrapper must be merged or disabled (base_only_of) instead of neither."""
    try:
        base = m.base_layer
        if type(base) is not nn.Linear:
            return None
        act = m.active_adapters
        if not isinstance(act, (list, tuple)) or len(act) != 1:
            return None
        name = act[0]
        if (bool(m.merged) or bool(m.disable_adapters)) != off:
            return None
        if set(m.lora_A.keys()) != set(m.lora_B.keys()) or name not in m.lora_A:
            return None
        A, B, drop = m.lora_A[name], m.lora_B[name], m.lora_dropout[name]
        if type(A) is not nn.Linear or type(B) is not nn.Linear or A.bias is not None or B.bias is not None:
            return None
        if A.weight.dtype not in ADAPTER_DTYPES or B.weight.dtype != A.weight.dtype:
            return None
        r = int(m.r[name])
        K, N = base.in_features, base.out_features
        if r not in RANKS or tuple(A.weight.shape) != (r, K) or tuple(B.weight.shape) != (N, r) or K % 32 or N % 32:
            return None
        if tuple(base.weight.shape) != (N, K):
            return None
        if not isinstance(drop, nn.Module) or getattr(drop, "inplace", False):   # (the route CALLS it, whatever module it is)
            return None
        scaling = float(m.scaling[name])
        if not math.isfinite(scaling):
            return None
        for mod in (m, base, A, B):
            for t in _HOOK_TABLES:
                if getattr(mod, t, None):
                    return None
        for attr in _VARIANTS:
            if _present(m, attr) and _set_for(getattr(m, attr), name):
                return None
        return Adapter(base, A, B, drop, scaling, r)
    except Exception:   # (an attribute of the layout is missing or unreadable)
        return None
