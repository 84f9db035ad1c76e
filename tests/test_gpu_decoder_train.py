"""GPU: the decoder's opt-in training route (u2tokenizer_amd/decoder_train.py) -- the causal GQA forward with key lengths and
row statistics, its flash backward, the row kernels' backward against float64 autograd (torch's own bf16 autograd of the same
expression as the yardstick), whole small decoders trained through the route against the fp32 stock model, the gradient-
checkpoint recompute, and the cases that must keep the stock layers."""
import pytest
import torch
import torch.nn.functional as F

from u2tokenizer_amd import synth

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"
ULP = 2.0 ** -8


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from u2tokenizer_amd import ops as _ops
    _ops.device_check()
    return _ops


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(bf)


def rms(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


def check_grad(got, bf_ref, ref, name=""):
    """got / bf_ref (torch's bf16 autograd) against the float64 reference: got's rms error <= 1.5 x torch's + 1 bf16 ulp of
    the gradient's max."""
    ref = ref.double()
    assert torch.isfinite(got.float()).all(), name
    e_got, e_bf = rms(got, ref), rms(bf_ref, ref)
    floor = ULP * ref.abs().max().item()
    assert e_got <= 1.5 * e_bf + floor, (name, e_got, e_bf, floor)


# ------------------------------------------------------------------------------------------------ attention
ATT = [(1, 1024, 32, 8, 128, None), (1, 1024, 32, 8, 64, None), (2, 77, 8, 4, 64, (77, 40)), (1, 130, 4, 4, 128, None),
       (2, 200, 8, 2, 128, (200, 113))]


def _qkv(nb, S, Hq, Hkv, d, seed):
    return rnd(nb, S, (Hq + 2 * Hkv) * d, seed=seed).to(D)


def _attn_ref(qkv, nb, S, Hq, Hkv, d, scale, lens):
    """softmax(q k^T scale, causal AND key < length) v in the precision of qkv -> (out (nb, S, Hq d), lse (nb * Hq, S) natural log)."""
    x = qkv.view(nb, S, Hq + 2 * Hkv, d)
    G = Hq // Hkv
    q = x[:, :, :Hq].permute(0, 2, 1, 3)
    k = x[:, :, Hq:Hq + Hkv].permute(0, 2, 1, 3).repeat_interleave(G, 1)
    v = x[:, :, Hq + Hkv:].permute(0, 2, 1, 3).repeat_interleave(G, 1)
    s = (q @ k.transpose(-1, -2)) * scale
    pos = torch.arange(S, device=qkv.device)
    ln = torch.tensor(lens if lens is not None else [S] * nb, device=qkv.device)
    vis = (pos[None, :] <= pos[:, None])[None] & (pos[None, None, :] < ln[:, None, None])
    s = s.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(s.double(), -1)
    out = torch.softmax(s, -1) @ v
    return out.permute(0, 2, 1, 3).reshape(nb, S, Hq * d), lse.reshape(nb * Hq, S)


@pytest.mark.parametrize("nb,S,Hq,Hkv,d,lens", ATT)
def test_attention_gqa_ex_forward(ops, nb, S, Hq, Hkv, d, lens):
    qkv = _qkv(nb, S, Hq, Hkv, d, 1)
    scale = d ** -0.5
    q, k, v = qkv[..., :Hq * d], qkv[..., Hq * d:(Hq + Hkv) * d], qkv[..., (Hq + Hkv) * d:]
    kv = torch.tensor(lens, dtype=torch.int32, device=D) if lens is not None else None
    with torch.no_grad():
        out, lse = ops.attention_gqa_ex(q, k, v, Hq, Hkv, scale, kv_len=kv, with_lse=True)
        ref, ref_lse = _attn_ref(qkv.double(), nb, S, Hq, Hkv, d, scale, lens)
        tol = 2 * ULP * ref.abs() + ULP * ref.abs().max()
        assert ((out.double() - ref).abs() <= tol).all(), (out.double() - ref).abs().max().item()
        got_lse = lse.double() * 0.6931471805599453   # (log2 units)
        assert (got_lse - ref_lse).abs().max().item() < 1e-3 * max(1.0, ref_lse.abs().max().item())
        # NULL key lengths and statistics: exactly u2tok_attention_gqa
        plain, none = ops.attention_gqa_ex(q, k, v, Hq, Hkv, scale)
        assert none is None and torch.equal(plain, ops.attention_gqa(q, k, v, Hq, Hkv, scale, causal=True))
        if lens is None:   # (all keys: the variant computes the same numbers)
            assert torch.equal(out, plain)


@pytest.mark.parametrize("nb,S,Hq,Hkv,d,lens", ATT)
def test_attention_gqa_bwd(ops, nb, S, Hq, Hkv, d, lens):
    qkv = _qkv(nb, S, Hq, Hkv, d, 2)
    dout = rnd(nb, S, Hq * d, seed=3).to(D)
    scale = d ** -0.5
    kv = torch.tensor(lens, dtype=torch.int32, device=D) if lens is not None else None
    W = (Hq + 2 * Hkv) * d
    with torch.no_grad():
        out, lse = ops.attention_gqa_ex(qkv[..., :Hq * d], qkv[..., Hq * d:(Hq + Hkv) * d], qkv[..., (Hq + Hkv) * d:], Hq, Hkv,
                                        scale, kv_len=kv, with_lse=True)
        got = ops.attention_gqa_bwd(qkv, out, dout, Hq, Hkv, scale, kv_len=kv, lse=lse)
        again = ops.attention_gqa_bwd(qkv, out, dout, Hq, Hkv, scale, kv_len=kv, lse=lse)
        assert torch.equal(got, again)                   # no atomics: bit-repeatable
        nolse = ops.attention_gqa_bwd(qkv, out, dout, Hq, Hkv, scale, kv_len=kv)   # statistics rebuilt by the kernel
    grads = {}
    with torch.enable_grad():
        for dt in (torch.float64, bf):
            x = qkv.to(dt).requires_grad_(True)
            o, _ = _attn_ref(x, nb, S, Hq, Hkv, d, scale, lens)
            o.backward(dout.to(dt))
            grads[dt] = x.grad.view(nb, S, W)
    for name, sl in (("dq", slice(0, Hq * d)), ("dk", slice(Hq * d, (Hq + Hkv) * d)), ("dv", slice((Hq + Hkv) * d, W))):
        check_grad(got[..., sl], grads[bf][..., sl], grads[torch.float64][..., sl], name)
        check_grad(nolse[..., sl], grads[bf][..., sl], grads[torch.float64][..., sl], name + " (no lse)")


# ------------------------------------------------------------------------------------------------ row kernels
def _rmsnorm_hf(x, w, eps=1e-6):
    xf = x.to(torch.float32 if x.dtype == bf else x.dtype)
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)


@pytest.mark.parametrize("rows,C", [(1024, 4096), (77, 2048), (5, 512), (300, 4096)])
def test_rmsnorm_bwd(ops, rows, C):
    x, w = rnd(rows, C, seed=1), (1 + 0.1 * rnd(C, seed=2).float()).to(bf)
    dy = rnd(rows, C, seed=3)
    res = rnd(rows, C, seed=4)
    with torch.no_grad():
        dx, dw = ops.rmsnorm_bwd(x.to(D), w.to(D), dy.to(D), 1e-6)
        dx2, _ = ops.rmsnorm_bwd(x.to(D), w.to(D), dy.to(D), 1e-6, d_res=res.to(D))
    ref = {}
    for dt in (torch.float64, bf):
        xx, ww = x.to(D, dt).requires_grad_(True), w.to(D, dt).requires_grad_(True)
        with torch.enable_grad():
            _rmsnorm_hf(xx, ww).backward(dy.to(D, dt))
        ref[dt] = (xx.grad, ww.grad)
    check_grad(dx, ref[bf][0], ref[torch.float64][0], "dx")
    check_grad(dw, ref[bf][1], ref[torch.float64][1], "dw")
    check_grad(dx2, ref[bf][0] + res.to(D), ref[torch.float64][0] + res.to(D, torch.float64), "dx + d_res")


def _qk_ref(qkv, wq, wk, cos, sin, Hq, Hkv, d, norm):
    rows = qkv.shape[0]
    x = qkv.view(rows, Hq + 2 * Hkv, d)
    parts = []
    for lo, hi, w in ((0, Hq, wq), (Hq, Hq + Hkv, wk)):
        h = x[:, lo:hi]
        if norm:
            h = _rmsnorm_hf(h, w)
        rot = torch.cat((-h[..., d // 2:], h[..., :d // 2]), -1)
        parts.append(h * cos[:, None] + rot * sin[:, None])
    parts.append(x[:, Hq + Hkv:])
    return torch.cat(parts, 1).reshape(rows, -1)


@pytest.mark.parametrize("rows,Hq,Hkv,d,norm,f32", [(1024, 32, 8, 128, True, False), (70, 8, 4, 64, False, True),
                                                     (33, 4, 4, 128, True, True), (9, 32, 8, 64, False, False)])
def test_qk_norm_rope_bwd(ops, rows, Hq, Hkv, d, norm, f32):
    qkv = rnd(rows, (Hq + 2 * Hkv) * d, seed=3)
    wq, wk = (1 + 0.1 * rnd(d, seed=4).float()).to(bf), (1 + 0.1 * rnd(d, seed=5).float()).to(bf)
    pos = torch.arange(rows, dtype=torch.float32)
    inv = 1.0 / (1e6 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.cat([pos[:, None] * inv[None]] * 2, -1)
    cos, sin = fr.cos(), fr.sin()
    if not f32:
        cos, sin = cos.to(bf), sin.to(bf)
    dy = rnd(rows, (Hq + 2 * Hkv) * d, seed=6)
    with torch.no_grad():
        g = dy.to(D)
        _, dwq, dwk = ops.qk_norm_rope_bwd(g, qkv.to(D), wq.to(D) if norm else None, wk.to(D) if norm else None, cos.to(D),
                                           sin.to(D), Hq, Hkv, d, 1e-6)
    assert torch.equal(g[:, (Hq + Hkv) * d:].cpu(), dy[:, (Hq + Hkv) * d:])   # v columns untouched
    ref = {}
    for dt in (torch.float64, bf):
        x = qkv.to(D, dt).requires_grad_(True)
        a, b = wq.to(D, dt).requires_grad_(True), wk.to(D, dt).requires_grad_(True)
        with torch.enable_grad():
            _qk_ref(x, a, b, cos.to(D, dt), sin.to(D, dt), Hq, Hkv, d, norm).backward(dy.to(D, dt))
        ref[dt] = (x.grad, a.grad, b.grad)
    n = (Hq + Hkv) * d
    check_grad(g[:, :n], ref[bf][0][:, :n], ref[torch.float64][0][:, :n], "dq|dk")
    if norm:
        check_grad(dwq, ref[bf][1], ref[torch.float64][1], "dwq")
        check_grad(dwk, ref[bf][2], ref[torch.float64][2], "dwk")


@pytest.mark.parametrize("rows,I", [(300, 1536), (1024, 12288), (7, 16)])
def test_swiglu_bwd(ops, rows, I):
    gu = rnd(rows, 2 * I, scale=2.0, seed=6)
    da = rnd(rows, I, seed=7)
    with torch.no_grad():
        got = ops.swiglu_bwd(gu.to(D), da.to(D))
    ref = {}
    for dt in (torch.float64, bf):
        x = gu.to(D, dt).requires_grad_(True)
        with torch.enable_grad():
            (F.silu(x[:, :I]) * x[:, I:]).backward(da.to(D, dt))
        ref[dt] = x.grad
    check_grad(got[:, :I], ref[bf][:, :I], ref[torch.float64][:, :I], "d_gate")
    check_grad(got[:, I:], ref[bf][:, I:], ref[torch.float64][:, I:], "d_up")


# ------------------------------------------------------------------------------------------------ whole decoders
def _small(kind, layers=2):
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen3Config, Qwen3ForCausalLM
    if kind == "qwen3":   # q / k norms, head dim 128, GQA
        cfg = Qwen3Config(vocab_size=512, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=4, num_key_value_heads=2, head_dim=128, max_position_embeddings=512,
                          tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2)
        m = Qwen3ForCausalLM(cfg)
    else:                 # Llama-3.2-1B's head dim 64, GQA
        cfg = LlamaConfig(vocab_size=512, hidden_size=512, intermediate_size=1024, num_hidden_layers=layers,
                          num_attention_heads=8, num_key_value_heads=2, head_dim=64, max_position_embeddings=512,
                          tie_word_embeddings=False, pad_token_id=0, bos_token_id=1, eos_token_id=2, rope_theta=500000.0)
        m = LlamaForCausalLM(cfg)
    synth.fill_module_(m, seed=17, prefix="decoder.")
    return m


def _batch(B, S, lens, E, vocab, seed=3):
    x = 0.5 * synth.synth_tensor("inputs_embeds", (B, S, E), seed)
    mask = torch.zeros((B, S), dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(3, vocab, (B, S), generator=g)
    labels[mask == 0] = -100
    return x, mask, labels


def _run(m, x, mask, labels, dtype, ckpt):
    m.train()
    if ckpt:
        m.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})
    else:
        m.gradient_checkpointing_disable()
    m.zero_grad(set_to_none=True)
    xe = x.to(D, dtype).requires_grad_(True)
    with torch.enable_grad():
        # (the last hidden states straight from the decoder stack: output_hidden_states would make HF hang its recording hooks
        #  on the layers' submodules, and a hooked layer keeps its stock forward)
        h = m.model(inputs_embeds=xe, attention_mask=mask.to(D), use_cache=False).last_hidden_state
        logits = m.lm_head(h).float()
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1).to(D), ignore_index=-100)
        loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.model.layers.named_parameters()}
    return loss.detach(), h.detach(), grads, xe.grad.detach()


def _err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30)).item()


@pytest.mark.parametrize("kind", ["qwen3", "llama"])
@pytest.mark.parametrize("ckpt", [False, True])
def test_decoder_training_route_matches_the_stock_decoder(ops, kind, ckpt):
    """Loss, last hidden states (pad rows included), every decoder parameter's gradient and d inputs_embeds of a right-padded
    batch of two: no further from the fp32 stock model than 1.5 x the stock bf16 run is (+ 1e-3); the route ran in every layer."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import enable_fused_prefill
    nl, B, S = 2, 2, 96
    m32 = _small(kind, nl).to(D)
    x, mask, labels = _batch(B, S, (96, 57), m32.config.hidden_size, m32.config.vocab_size)
    ref = _run(m32, x, mask, labels, torch.float32, ckpt)
    mg = _small(kind, nl).to(bf).to(D)
    stock = _run(mg, x, mask, labels, bf, ckpt)
    assert enable_fused_prefill(mg, train=True) == nl
    n0 = decoder_train.stats["layers"]
    fused = _run(mg, x, mask, labels, bf, ckpt)
    assert decoder_train.stats["layers"] - n0 == nl * (2 if ckpt else 1)   # (checkpointing: forward + recompute)
    assert not torch.equal(fused[1], stock[1])
    for i, name in ((0, "loss"), (1, "hidden"), (3, "d inputs_embeds")):
        es, ef = _err(stock[i], ref[i]), _err(fused[i], ref[i])
        assert ef <= 1.5 * es + 1e-3, (name, ef, es)
    assert fused[2].keys() == ref[2].keys()
    for n in ref[2]:
        es, ef = _err(stock[2][n], ref[2][n]), _err(fused[2][n], ref[2][n])
        assert ef <= 1.5 * es + 1e-3, (n, ef, es)


def test_checkpoint_recompute_uses_its_own_forwards_padding(ops):
    """Checkpointing on: forward A (one padding), a no_grad forward B with another padding, then A's backward -- the recompute
    must use A's key lengths: gradients equal to those of A alone."""
    from u2tokenizer_amd.prefill import enable_fused_prefill
    mg = _small("qwen3").to(bf).to(D)
    enable_fused_prefill(mg, train=True)
    E, V = mg.config.hidden_size, mg.config.vocab_size
    xa, ma, la = _batch(2, 80, (80, 41), E, V, seed=5)
    xb, mb, _ = _batch(2, 80, (23, 80), E, V, seed=6)
    mg.train()
    mg.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})

    def grads(with_b):
        mg.zero_grad(set_to_none=True)
        with torch.enable_grad():
            loss = mg(inputs_embeds=xa.to(D, bf), attention_mask=ma.to(D), labels=la.to(D), use_cache=False).loss
            if with_b:
                with torch.no_grad():
                    mg(inputs_embeds=xb.to(D, bf), attention_mask=mb.to(D), use_cache=False)
            loss.backward()
        return {n: p.grad.clone() for n, p in mg.model.layers.named_parameters()}

    alone, mixed = grads(False), grads(True)
    for n in alone:
        assert torch.equal(alone[n], mixed[n]), n


def test_training_route_stays_stock(ops):
    """Default settings never enter the route; with train=True each of these keeps the stock forward: a LoRA-like wrapped
    projection, a hook, attention dropout > 0, a left-padded mask, fp16 parameters, head dim 96."""
    from u2tokenizer_amd import decoder_train
    from u2tokenizer_amd.prefill import disable_fused_prefill, enable_fused_prefill
    from test_gpu_prefill import _LoraLikeLinear
    st = decoder_train.stats

    def layers_run(m, mask=None, dtype=bf):
        n0 = st["layers"]
        x, m2, lab = _batch(2, 64, (64, 64), m.config.hidden_size, m.config.vocab_size)
        if mask is not None:
            m2 = mask
        _run(m, x, m2, lab, dtype, False)
        return st["layers"] - n0

    mg = _small("llama").to(bf).to(D)
    assert layers_run(mg) == 0                         # not patched
    enable_fused_prefill(mg)
    assert layers_run(mg) == 0                         # patched for inference only (the default)
    enable_fused_prefill(mg, train=True)
    assert layers_run(mg) == 2
    left = torch.ones((2, 64), dtype=torch.int64)
    left[1, :9] = 0
    assert layers_run(mg, mask=left) == 0              # left padding
    lay = mg.model.layers[1]
    lay.self_attn.q_proj = _LoraLikeLinear(lay.self_attn.q_proj).to(D)
    assert layers_run(mg) == 1                         # the wrapped layer is stock
    lay.self_attn.q_proj = lay.self_attn.q_proj.base_layer
    h = mg.model.layers[0].mlp.register_forward_hook(lambda *a: None)
    assert layers_run(mg) == 1                         # the hooked layer is stock
    h.remove()
    for layer in mg.model.layers:
        layer.self_attn.attention_dropout = 0.1
    assert layers_run(mg) == 0                         # dropout in training mode
    for layer in mg.model.layers:
        layer.self_attn.attention_dropout = 0.0
    disable_fused_prefill(mg)
    mh = _small("llama").to(torch.float16).to(D)
    enable_fused_prefill(mh, train=True)
    assert layers_run(mh, dtype=torch.float16) == 0    # fp16
    from transformers import LlamaConfig, LlamaForCausalLM
    m96 = LlamaForCausalLM(LlamaConfig(vocab_size=512, hidden_size=384, intermediate_size=768, num_hidden_layers=2,
                                       num_attention_heads=4, num_key_value_heads=2, head_dim=96,
                                       max_position_embeddings=512)).to(bf).to(D)
    enable_fused_prefill(m96, train=True)
    assert layers_run(m96) == 0                        # head dim 96: no backward kernel
