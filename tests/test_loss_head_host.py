"""CPU: the host side of the loss head (u2tokenizer_amd/loss_head.py) -- the vocabulary slice plan, the argument checks of its two
C entry points on both builds, which calls of a u2 causal LM take the head and which keep lm_head + ForCausalLMLoss, and the label
shift / row compaction bookkeeping against ForCausalLMLoss's own label handling."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from u2tokenizer_amd import _lib, language_model as LM, loss_head

ERR_ARG = -1


# ------------------------------------------------------------------------------------------------ slice plan
@pytest.mark.parametrize("V", [151936, 128256, 32064, 256, 8])
@pytest.mark.parametrize("R", [1, 1024, 8192, 65536])
@pytest.mark.parametrize("budget", [loss_head.DEFAULT_SLICE_BYTES, 1 << 20, 1])
def test_plan_slices_tiles_the_vocabulary_within_the_budget(V, R, budget):
    plan = loss_head.plan_slices(R, V, budget)
    assert plan[0][0] == 0 and plan[-1][0] + plan[-1][1] == V
    for (a, na), (b, _) in zip(plan, plan[1:]):
        assert a + na == b                                   # no gap, no overlap
    for v0, vs in plan:
        assert vs >= 1
    for v0, vs in plan[:-1]:
        assert vs % 256 == 0
    widest = max(vs for _, vs in plan)
    assert R * widest * 2 <= budget or widest <= 256         # (Vs = 256 when even 256 columns do not fit)
    if len(plan) > 1:
        assert plan[-1][1] <= plan[0][1] and len({vs for _, vs in plan[:-1]}) == 1


def test_plan_slices_default_budget_examples():
    assert loss_head.plan_slices(1024, 151936) == [(0, 76032), (76032, 75904)]       # 256 MiB / (1024 x 2 B) = 131 072 columns
    assert loss_head.plan_slices(77, 32064) == [(0, 32064)]
    assert len(loss_head.plan_slices(8192, 151936)) == 10                            # 16 384 columns at most -> 15 360 each
    with pytest.raises(ValueError):
        loss_head.plan_slices(0, 8)


# ------------------------------------------------------------------------------------------------ C entry points
@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib(request):
    if not all(p.exists() for p in _lib._LIBS.values()):
        _lib.build()
    return _lib.load_library(request.param)


def test_ce_entry_points_reject_bad_arguments_before_any_launch(lib):
    P = 1 << 20   # a 256-byte aligned address that is never dereferenced
    # Z, ldz, rows, Vs, v0, labels, m | lse, l | coef, (zt,) stream
    lse_args = [P, 512, 4, 512, 0, P, P, P, P, None]
    grad_args = [P, 512, 4, 512, 0, P, P, P, None]
    for fn, args, ptrs in ((lib.u2tok_ce_lse_update, lse_args, (0, 5, 6, 7, 8)), (lib.u2tok_ce_grad_inplace, grad_args, (0, 5, 6, 7))):
        def call(**kw):
            a = list(args)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return fn(*a)

        for i in ptrs:
            assert call(**{f"a{i}": None}) == ERR_ARG, (fn.__name__, i)
        assert call(a2=0) == ERR_ARG and call(a2=-3) == ERR_ARG        # rows < 1
        assert call(a3=0) == ERR_ARG and call(a3=-8) == ERR_ARG        # Vs < 1
        assert call(a1=504) == ERR_ARG                                 # ldz < Vs
        assert call(a1=516) == ERR_ARG                                 # ldz not a multiple of 8
        assert call(a3=508) == ERR_ARG                                 # Vs not a multiple of 8
        assert call(a0=P + 8) == ERR_ARG                               # Z not 16-byte aligned
        assert call(a4=-256) == ERR_ARG                                # negative first column


def test_ce_entry_points_are_declared_and_bound():
    for name in ("u2tok_ce_lse_update", "u2tok_ce_grad_inplace"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and args[1] is C.c_int64              # 64-bit leading dimension: rows x ldz passes 2^31


# ------------------------------------------------------------------------------------------------ which calls take the head
class _SubLinear(nn.Linear):
    pass


def _tiny(switch=None, dtype=torch.float32):
    cfg = LM.u2Config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=16)
    if switch is not None:
        cfg.u2_fused_loss_head = switch
    return LM.u2LlamaForCausalLM(cfg).to(dtype).eval()


def _loss(m, dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 64, (2, 9), generator=g)
    labels = ids.clone()
    labels[:, :4] = -100
    n0 = dict(loss_head.stats)
    out = m(input_ids=ids, labels=labels)
    assert loss_head.stats == n0                                       # the head did not run
    assert isinstance(out, LM.CausalLMOutputWithPast) and out.logits is not None and out.logits.shape == (2, 9, 64)
    assert torch.isfinite(out.loss)
    return out.loss


def test_switch_absent_or_off_keeps_the_stock_head():
    assert not _tiny()._loss_head_ok({}) and not _tiny(False)._loss_head_ok({})
    a, b = _loss(_tiny()), _loss(_tiny(False))
    assert type(a) is type(b) is torch.Tensor


@pytest.mark.parametrize("case", ["cpu_bf16", "fp32", "bias", "hook", "subclass", "logits_to_keep", "tuple"])
def test_switch_on_but_head_does_not_qualify_keeps_the_stock_head(case):
    torch.manual_seed(0)
    m = _tiny(True, torch.bfloat16 if case == "cpu_bf16" else torch.float32)
    kwargs = {}
    if case == "bias":
        m.lm_head = nn.Linear(64, 64, bias=True)
    elif case == "hook":
        m.lm_head.register_forward_hook(lambda *a: None)
    elif case == "subclass":
        m.lm_head = _SubLinear(64, 64, bias=False)
    elif case == "logits_to_keep":
        kwargs = {"logits_to_keep": 2}
    elif case == "tuple":
        kwargs = {"return_dict": False}
    assert not m._loss_head_ok(kwargs)
    if not kwargs:
        ref = _tiny(False, m.lm_head.weight.dtype)
        ref.load_state_dict(m.state_dict(), strict=False)
        if case == "bias":
            ref.lm_head = m.lm_head
        a, b = _loss(m), _loss(ref)
        assert type(a) is type(b) and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="token_logprobs"):          # the DPO entry has no fallback: it says so
        m.token_logprobs(None, torch.ones(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64))


def test_head_qualifies_by_type_shape_and_device():
    class _Cuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    m = _tiny(True, torch.bfloat16)
    assert not m._plain_lm_head()
    m.lm_head.weight = nn.Parameter(m.lm_head.weight.detach().as_subclass(_Cuda), requires_grad=False)
    assert m._plain_lm_head() and m._loss_head_ok({}) and not m._loss_head_ok({"logits_to_keep": 1})
    m.config.u2_fused_loss_head = False
    assert m._plain_lm_head() and not m._loss_head_ok({})
    assert loss_head.supported(4096, 151936, torch.bfloat16) and loss_head.supported(2048, 128256, torch.bfloat16)
    assert not loss_head.supported(4096, 151936, torch.float16)        # training is bf16
    assert not loss_head.supported(4096, 32001, torch.bfloat16) and not loss_head.supported(96, 512, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ label bookkeeping
def test_shift_and_compaction_match_the_stock_label_handling():
    from transformers.loss.loss_utils import ForCausalLMLoss
    g = torch.Generator().manual_seed(5)
    B, S, V = 3, 11, 32
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[0, :6] = -100            # masked prompt
    labels[1, 8:] = -100            # right padding
    labels[2] = -100                # a sequence without any label
    logits = torch.randn(B, S, V, generator=g, dtype=torch.float64)
    sl = loss_head.shift_labels(labels)
    assert sl.shape == labels.shape and torch.equal(sl[:, :-1], labels[:, 1:]) and (sl[:, -1] == -100).all()
    idx, lab = loss_head.compact_rows(sl.reshape(-1), V)
    assert torch.equal(idx, torch.nonzero(sl.reshape(-1) != -100).squeeze(1)) and torch.equal(lab, sl.reshape(-1)[idx])
    # the head's arithmetic on those rows only, in torch: the same numbers as ForCausalLMLoss on all rows
    rows = logits.reshape(-1, V)[idx]
    nll = torch.logsumexp(rows, -1) - rows.gather(1, lab[:, None])[:, 0]
    tol = dict(rtol=2e-6, atol=0)   # (ForCausalLMLoss computes in fp32 whatever it is handed)
    assert torch.allclose(nll.sum() / idx.numel(), ForCausalLMLoss(logits, labels, V).double(), **tol)
    assert torch.allclose(nll.sum() / 7, ForCausalLMLoss(logits, labels, V, num_items_in_batch=7).double(), **tol)
    assert torch.allclose(nll.sum() / idx.numel(), ForCausalLMLoss(logits, None, V, shift_labels=sl).double(), **tol)
    per_token = F.cross_entropy(rows, lab, reduction="none")
    assert torch.allclose(nll, per_token, rtol=1e-12, atol=1e-12)


def test_compaction_validates_the_labels_it_keeps():
    ok = torch.tensor([-100, 0, 31, -100, 5])
    idx, lab = loss_head.compact_rows(ok, 32)
    assert idx.tolist() == [1, 2, 4] and lab.tolist() == [0, 31, 5]
    for bad in (32, -1, -99):
        with pytest.raises(ValueError):
            loss_head.compact_rows(torch.tensor([-100, bad, 3]), 32)
    idx, lab = loss_head.compact_rows(torch.full((4,), -100), 32)
    assert idx.numel() == 0 and lab.numel() == 0
    idx, _ = loss_head.compact_rows(torch.tensor([7, -1, -1]), 32, ignore_index=-1)
    assert idx.tolist() == [0]
    with pytest.raises(ValueError):                                   # another ignore_index: -100 is a bad label then
        loss_head.compact_rows(torch.tensor([7, -100, -1]), 32, ignore_index=-1)


def test_function_refuses_what_it_does_not_compute():
    h, w = torch.zeros(4, 64, dtype=torch.float16), torch.zeros(64, 64, dtype=torch.float16)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="float16"):
        loss_head.TokenNLLFn.apply(h, w, lab, -100, 1 << 20)
    with pytest.raises(RuntimeError):
        loss_head.TokenNLLFn.apply(h.to(torch.bfloat16), torch.zeros(63, 64, dtype=torch.bfloat16), lab, -100, 1 << 20)
    with pytest.raises(RuntimeError, match="do not match"):
        loss_head.token_nll(torch.zeros(2, 3, 64, dtype=torch.bfloat16), w.to(torch.bfloat16), torch.zeros(2, 4, dtype=torch.int64))
