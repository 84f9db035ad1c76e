"""Host: the per-element error bounds that tests/test_gpu_decoder_train_ops.py holds the decoder training kernels to
(u2tok_rmsnorm_bwd, u2tok_qk_norm_rope_bwd, u2tok_swiglu_bwd, u2tok_attention_gqa_ex, u2tok_attention_gqa_bwd and the non-causal
u2tok_flash_attention_d64_bwd), as pure functions of the bf16 inputs, next to a torch emulation of each kernel's documented
rounding points.  The tests here run the emulation on every case of the GPU module's case tables (imported, not copied) and
assert that it stays inside the bound: a bound that its own model of the kernel breaks would prove nothing on the GPU.

Conventions.  U = 2^-8 is the unit roundoff the bounds charge per bf16 rounding (round-to-nearest errs by at most half of that,
2^-9 relative, at the top of a binade and by all of it never: the factor between the two is the bounds' only slack), u = 2^-24
that of fp32.  Every *_model function computes the float64 reference and the bound from the same inputs; every *_emulate function
repeats the kernel's arithmetic with `rbf` (-> fp32 -> bf16 -> float64) where the kernel rounds: in float64 (`work`) for the bound
proper, in float32 for the near-tie allowance of the weight gradients.

Near ties.  dw sums dy n with n = bf16(xhat), and the reference rounds its own float64 xhat: where that value lies within 2^-20
(relative) of a rounding boundary of bf16, the kernel's fp32 xhat may round to the other neighbour, and the bound allows |dy| times
one bf16 ulp of n for that element.  Fewer than 1 % of a case's elements may be near ties (random data: ~0.04 %)."""
import math

import pytest
import torch

bf = torch.bfloat16
u, U = 2.0 ** -24, 2.0 ** -8
NEAR = 2.0 ** -20
f64 = torch.float64


def rbf(t):
    """the kernels' bf16 rounding of an fp32 value, back in float64"""
    return t.float().to(bf).double()


def bf16_ulp(t):
    """the spacing of bf16 at |t| (2^(e - 7) for 2^e <= |t| < 2^(e + 1))"""
    _, e = torch.frexp(t.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(t), e - 8)


def near_tie(t):
    """float64 t within 2^-20 |t| of a midpoint between two adjacent bf16 values"""
    a = t.abs().clamp_min(2.0 ** -120)
    q = a / bf16_ulp(a)                       # in [128, 256)
    return ((q - torch.floor(q) - 0.5).abs() <= NEAR * q) & (t != 0)


def worst(err, bound):
    """max of err / bound over the elements (0 / 0 counts as 0)"""
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return r.max().item() if r.numel() else 0.0


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _rn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(bf)


# ---------------------------------------------------------------------------------------------------------------- RMSNorm
def rms_inputs(rows, C, with_dres):
    g = _gen(1, rows, C)
    x, dy = _rn(g, rows, C, scale=1.5), _rn(g, rows, C)
    w = (1.0 + 0.5 * torch.randn(C, generator=g)).to(bf)
    dres = _rn(g, rows, C, scale=0.7) if with_dres else None
    prefill = torch.randn(C, generator=g) * 8
    return dict(x=x, w=w, dy=dy, dres=dres, prefill=prefill, eps=1e-6)


def _norm_bwd_model(x, g, eps):
    """RMSNorm backward over the last dim of x (float64) for the upstream gradient g = dy w (float64) -> (core, bound, rstd, xh):
    core = rstd (g - xh mean(g xh)); bound = the rounding of g to bf16 carried through that expression,
    rstd U (|g| + |xh| mean(|g| |xh|)), plus the fp32 evaluation: the sum of C squares is off by at most C u of itself, so rstd
    (rsqrt, the division by C) and xh = x rstd relatively by e_r = (C / 2 + 2) u; s2 = mean(g xh) by (C u + e_r + 2 u) mean|g xh|;
    the final expression by (e_r + 3 u) |core| + rstd |xh| (C u + 2 e_r + 4 u) mean|g xh|."""
    C = x.shape[-1]
    rstd = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = x * rstd
    core = rstd * (g - xh * (g * xh).mean(-1, keepdim=True))
    mabs = (g * xh).abs().mean(-1, keepdim=True)
    e_r = (C / 2 + 2) * u
    bound = rstd * U * (g.abs() + xh.abs() * mabs) + (e_r + 3 * u) * core.abs() + rstd * xh.abs() * (C * u + 2 * e_r + 4 * u) * mabs
    return core, bound, rstd, xh


def rms_model(x, w, dy, dres, eps, **_):
    """float64 dx = rstd (g - xhat mean_c(g xhat)) (+ dres), g = dy w, and dw = sum_r dy bf16(xhat), with their bounds:
    dx: U |dx| (the output rounding) + _norm_bwd_model's terms + u |dx| (the fp32 addition of dres);
    dw: rows u sum_r |dy n| (rows products, exact in fp32, summed in any order) + the near-tie allowance."""
    x, w, dy = x.double(), w.double(), dy.double()
    rows = x.shape[0]
    core, nb_, _, xh = _norm_bwd_model(x, dy * w, eps)
    dx = core + (dres.double() if dres is not None else 0)
    n = rbf(xh)
    near = near_tie(xh)
    dw_mag = (dy * n).abs().sum(0)
    return dict(dx=dx, dx_bound=U * dx.abs() + nb_ + u * dx.abs(), dw=(dy * n).sum(0), dw_mag=dw_mag,
                dw_bound=rows * u * dw_mag + (near * dy.abs() * bf16_ulp(n)).sum(0), near_frac=near.double().mean().item())


def rms_emulate(x, w, dy, dres, eps, work=f64, **_):
    """the kernel: xhat = x rstd in `work`; n = bf16(xhat) feeds dw; g = bf16(dy w); dx = bf16(rstd (g - xhat mean(g xhat)) + dres)"""
    x, w, dy = x.to(work), w.to(work), dy.to(work)
    rstd = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = x * rstd
    n = rbf(xh)
    g = rbf(dy * w).to(work)
    dx = rstd * (g - xh * (g * xh).mean(-1, keepdim=True)) + (dres.to(work) if dres is not None else 0)
    return rbf(dx), (dy.double() * n).sum(0)


# ------------------------------------------------------------------------------------------------------- head norm + rotary
def qk_inputs(rows, Hq, Hkv, D, norm, f32):
    """dy (rows, (Hq + 2 Hkv) D), pre (rows, (Hq + Hkv) D), wq / wk (D), cos / sin (rows, D) of a rotary table (theta 1e4,
    positions 0 .. rows - 1; row rows // 2 overwritten with the identity cos = 1, sin = 0)"""
    g = _gen(2, rows, Hq, Hkv, D)
    dy = _rn(g, rows, (Hq + 2 * Hkv) * D)
    pre = _rn(g, rows, (Hq + Hkv) * D, scale=1.5)
    wq, wk = (1.0 + 0.3 * torch.randn(D, generator=g)).to(bf), (1.0 + 0.3 * torch.randn(D, generator=g)).to(bf)
    inv = 1.0 / (1e4 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None]
    fr = torch.cat([fr, fr], -1)
    cos, sin = fr.cos(), fr.sin()
    cos[rows // 2], sin[rows // 2] = 1.0, 0.0
    if not f32:
        cos, sin = cos.to(bf), sin.to(bf)
    return dict(dy=dy, pre=pre, wq=wq if norm else None, wk=wk if norm else None, cos=cos, sin=sin, eps=1e-6,
                prefill_q=torch.randn(D, generator=g) * 8, prefill_k=torch.randn(D, generator=g) * 8)


def _unrotate(dy, cos, sin, H, D, work):
    """da = ya c_a + yb s_b, db = yb c_b - ya s_a per head (pair a = l, b = l + D/2) -> (d, mag) (rows, H, D); mag: |ya c| + |yb s|"""
    rows, hf = dy.shape[0], D // 2
    y = dy[:, :H * D].to(work).view(rows, H, D)
    ya, yb = y[..., :hf], y[..., hf:]
    c, s = cos.to(work)[:, None], sin.to(work)[:, None]
    c0, c1, s0, s1 = c[..., :hf], c[..., hf:], s[..., :hf], s[..., hf:]
    d = torch.cat([ya * c0 + yb * s1, yb * c1 - ya * s0], -1)
    mag = torch.cat([(ya * c0).abs() + (yb * s1).abs(), (yb * c1).abs() + (ya * s0).abs()], -1)
    return d, mag


def qk_model(dy, pre, wq, wk, cos, sin, eps, Hq, Hkv, D, **_):
    """float64 result of the q | k columns (rows, (Hq + Hkv) D) and of dwq / dwk, with bounds.
    Rotation only: U |ref| + 2 u (|ya c| + |yb s|) (two fp32 products and their sum).
    With norm: the RMSNorm model over the D columns of a head with g = d w (d: the un-rotated gradient, kept in fp32 by the kernel),
    plus d's fp32 error 2 u mag carried through it as a perturbation of g: rstd (dg + |h| mean(dg |h|)), dg = 2 u mag |w|.  (No
    near-tie allowance for g: a rounding of g that falls to the other side errs by half an ulp plus dg, both already charged.)
    dwq / dwk = sum over rows and the group's heads of d n, n = bf16(h): N terms -> (N + 1) u sum |d n| + 3 u sum mag |n| + the
    near-tie allowance sum near(h) |d| ulp(n)."""
    rows, H = dy.shape[0], Hq + Hkv
    d, mag = _unrotate(dy, cos, sin, H, D, f64)
    if wq is None:
        return dict(out=d.reshape(rows, H * D), out_bound=(U * d.abs() + 2 * u * mag).reshape(rows, H * D), near_frac=0.0)
    w = torch.cat([wq.double().expand(Hq, D), wk.double().expand(Hkv, D)])[None]
    x = pre[:, :H * D].double().view(rows, H, D)
    core, nb_, rstd, h = _norm_bwd_model(x, d * w, eps)
    dg = 2 * u * mag * w.abs()
    bound = U * core.abs() + nb_ + rstd * (dg + h.abs() * (dg * h.abs()).mean(-1, keepdim=True))
    n = rbf(h)
    near = near_tie(h)
    res = dict(out=core.reshape(rows, H * D), out_bound=bound.reshape(rows, H * D), near_frac=near.double().mean().item())
    for name, sl in (("dwq", slice(0, Hq)), ("dwk", slice(Hq, H))):
        t = (d * n)[:, sl]
        N = rows * (sl.stop - sl.start)
        res[name] = t.sum((0, 1))
        res[name + "_mag"] = t.abs().sum((0, 1))
        res[name + "_bound"] = ((N + 1) * u * t.abs().sum((0, 1)) + 3 * u * (mag * n.abs())[:, sl].sum((0, 1))
                                + (near * d.abs() * bf16_ulp(n))[:, sl].sum((0, 1)))
    return res


def qk_emulate(dy, pre, wq, wk, cos, sin, eps, Hq, Hkv, D, work=f64, **_):
    rows, H = dy.shape[0], Hq + Hkv
    d, _ = _unrotate(dy, cos, sin, H, D, work)
    if wq is None:
        return rbf(d).reshape(rows, H * D), None, None
    w = torch.cat([wq.to(work).expand(Hq, D), wk.to(work).expand(Hkv, D)])[None]
    x = pre[:, :H * D].to(work).view(rows, H, D)
    rstd = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    h = x * rstd
    n = rbf(h)
    g = rbf(d * w).to(work)
    out = rbf(rstd * (g - h * (g * h).mean(-1, keepdim=True)))
    t = d.double() * n
    return out.reshape(rows, H * D), t[:, :Hq].sum((0, 1)), t[:, Hq:].sum((0, 1))


# ------------------------------------------------------------------------------------------------------------------ SwiGLU
def swiglu_inputs(rows, I):
    """gate | up (rows, 2 I) and dact (rows, I); the gate mixes N(0, 2) with a ramp over [-30, 30] (sigma saturated at both ends)"""
    g = _gen(3, rows, I)
    gate = torch.randn(rows, I, generator=g) * 2
    ramp = torch.linspace(-30, 30, rows * I).view(rows, I)
    gate = torch.where(torch.rand(rows, I, generator=g) < 0.5, gate, ramp[:, torch.randperm(I, generator=g)])
    return dict(gu=torch.cat([gate, torch.randn(rows, I, generator=g) * 1.5], 1).to(bf), dact=_rn(g, rows, I))


def swiglu_model(gu, dact, **_):
    """d_up = dact silu(g), d_gate = dact u silu'(g), silu'(g) = sg (1 + g (1 - sg)), sg = sigma(g).
    d_up: U |ref| + U |dact| |silu(g)| (silu rounded to bf16) + (4 + 2 |g|) u |ref| (fp32: exp(-g) through exp2(-g log2 e) errs
    relatively by up to ~1.5 |g| u -- the rounded product and the rounded constant -- then the quotient and two products);
    d_gate: U |ref| + U |dact u| |silu'(g)| (dact u rounded) + (6 + 2 |g|) u |dact u| sg (1 + |g| (1 - sg)) (fp32 silu', the terms
    of its cancelling sum taken by magnitude: relative to silu' itself that error is unbounded at its zero near g = -1.28)."""
    I = dact.shape[1]
    g, up, d = gu[:, :I].double(), gu[:, I:].double(), dact.double()
    sg = torch.sigmoid(g)
    silu, dsilu = g * sg, sg * (1 + g * (1 - sg))
    d_up, d_gate = d * silu, d * up * dsilu
    return dict(d_up=d_up, d_up_bound=U * d_up.abs() + U * d.abs() * silu.abs() + (4 + 2 * g.abs()) * u * d_up.abs(),
                d_gate=d_gate, d_gate_bound=U * d_gate.abs() + U * (d * up).abs() * dsilu.abs()
                + (6 + 2 * g.abs()) * u * (d * up).abs() * sg * (1 + g.abs() * (1 - sg)))


def swiglu_emulate(gu, dact, **_):
    I = dact.shape[1]
    g, up, d = gu[:, :I].double(), gu[:, I:].double(), dact.double()
    sg = torch.sigmoid(g)
    return rbf(rbf(d * up) * sg * (1 + g * (1 - sg))), rbf(d * rbf(g * sg))


# --------------------------------------------------------------------------------------------------------------- attention
def attn_inputs(nb, S, Hq, Hkv, d, Skv=None):
    """packed q | k | v (nb, S, (Hq + 2 Hkv) d) and d_out (nb, S, Hq d), N(0, 1); Skv given (forward only): q (nb, S, Hq d) and
    k | v (nb, Skv, 2 Hkv d) under the keys "q" and "kv"."""
    g = _gen(4, nb, S, Hq, Hkv, d, Skv or 0)
    if Skv is None:
        return dict(qkv=_rn(g, nb, S, (Hq + 2 * Hkv) * d), dout=_rn(g, nb, S, Hq * d))
    return dict(q=_rn(g, nb, S, Hq * d), kv=_rn(g, nb, Skv, 2 * Hkv * d))


def other_tail(t, lens, seed):
    """a copy of t (nb, S, ...) whose rows at or beyond lens[b] hold other finite data, magnitudes up to 64"""
    t = t.clone()
    g = _gen(5, seed)
    for b, n in enumerate(lens):
        if n < t.shape[1]:
            t[b, n:] = ((torch.rand(t[b, n:].shape, generator=g) * 2 - 1) * 64).to(bf)
    return t


def heads(t, H, d):
    """(nb, S, H d) -> float64 (nb, H, S, d)"""
    return t.double().view(t.shape[0], t.shape[1], H, d).permute(0, 2, 1, 3)


def rows_of(t):
    """(nb, H, S, d) -> (nb, S, H d)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


def visible(nb, Sq, Skv, lens, causal=True):
    """(nb, Sq, Skv): query i sees key j iff j <= i + Skv - Sq (causal) and j < clamp(lens[b], 1, Skv)"""
    i, j = torch.arange(Sq)[:, None], torch.arange(Skv)[None, :]
    vis = (j <= i + Skv - Sq) if causal else torch.ones(Sq, Skv, dtype=torch.bool)
    ln = torch.tensor([Skv] * nb if lens is None else [max(1, min(int(n), Skv)) for n in lens])
    return vis[None] & (j[None] < ln[:, None, None])


def _probs(q, k, scale, vis):
    G = q.shape[1] // k.shape[1]
    s = (q @ k.repeat_interleave(G, 1).transpose(-1, -2)) * scale
    s = s.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    return s, lse, torch.exp(s - lse[..., None])


def attn_fwd_model(q, k, v, scale, vis):
    """q (nb, Hq, Sq, d), k / v (nb, Hkv, Skv, d) float64 -> out (nb, Hq, Sq, d), lse (nb, Hq, Sq) (natural log) and their bounds.
    out: two roundings -- the result is rounded to bf16, U |out|, and the probabilities enter the P V product as bf16, each p_j
    off by U p_j: U sum_j P_j |v_j| -- plus the fp32 accumulation (Skv + d) u sum_j P_j |v_j|.  Where a row's terms do not cancel
    this is the two-rounding bound 2 U |out|; where they do, |out| says nothing about the error of the sum, and 2 U |out| with a
    floor of U 2^-6 max|out| is broken 6-fold by the emulation below (S = 33, G = 8), so the second rounding is charged on the
    magnitudes it acts on and no floor is needed.
    lse: 1e-5 max(1, |lse|) (an fp32 sum of at most Skv positive terms and a d-term fp32 dot product under it)."""
    s, lse, P = _probs(q, k, scale, vis)
    G = q.shape[1] // k.shape[1]
    vv = v.repeat_interleave(G, 1)
    out = P @ vv
    bound = U * out.abs() + (U + (k.shape[2] + q.shape[3]) * u) * (P @ vv.abs())
    return dict(out=out, out_bound=bound, lse=lse, lse_tol=1e-5 * lse.abs().clamp_min(1.0), P=P, s=s)


def attn_fwd_emulate(q, k, v, scale, vis):
    """the kernel: p = exp(s - rowmax) rounded to bf16 for the P V product, the row sum of the unrounded p divides, one output rounding"""
    s, _, _ = _probs(q, k, scale, vis)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    G = q.shape[1] // k.shape[1]
    return rbf((rbf(p) @ v.repeat_interleave(G, 1)) / p.sum(-1, keepdim=True))


def attn_bwd_model(qkv, dout, Hq, Hkv, d, scale, lens, causal=True, lse_given=False):
    """float64 dq (nb, S, Hq d), dk, dv (nb, S, Hkv d) of out = softmax(q k^T scale + mask) v for the upstream dout, the forward's
    out (nb, S, Hq d) and lse, and the bounds.  The kernel is handed out rounded to bf16 (`out_b`).
    With dP = dO V^T, D = rowsum(dO out), dS = P (dP - D):  dD = U rowsum(|dO| |out|) (out is bf16),  ddS = U |dS| + P dD (dS a bf16
    MFMA operand, D's error under it);  dq: U |dq| + scale ddS |K|;  dk: U |dk| + scale ddS^T |Q| summed over the group's heads;
    dv: U |dv| + U P^T |dO| (P a bf16 operand) summed likewise.
    fp32 on top: the scores are d-term fp32 dot products and lse an fp32 sum (or the forward's, held to lse_tol): P errs relatively
    by eP = scale d u |Q| |K|^T + (S + 8) u (+ lse_tol);  dP and D are d-term sums: fdS = eP |dS| + P d u (|dO| |V|^T + rowsum(|dO|
    |out|));  the accumulations over n = S keys (dq) or G S queries (dk, dv) add n u sum |terms|."""
    nb, S, _ = qkv.shape
    G = Hq // Hkv
    q, k, v = heads(qkv[..., :Hq * d], Hq, d), heads(qkv[..., Hq * d:(Hq + Hkv) * d], Hkv, d), heads(qkv[..., (Hq + Hkv) * d:], Hkv, d)
    dO = heads(dout, Hq, d)
    f = attn_fwd_model(q, k, v, scale, visible(nb, S, S, lens, causal))
    P, out = f["P"], f["out"]
    kk, vv = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    Dm = (dO.abs() * out.abs()).sum(-1, keepdim=True)
    dS = P * (dO @ vv.transpose(-1, -2) - (dO * out).sum(-1, keepdim=True))
    eP = scale * d * u * (q.abs() @ kk.abs().transpose(-1, -2)) + (S + 8) * u + (f["lse_tol"][..., None] if lse_given else 0)
    fdS = eP * dS.abs() + P * d * u * (dO.abs() @ vv.abs().transpose(-1, -2) + Dm)
    ddS = U * dS.abs() + P * (U * Dm) + fdS

    def group(t):
        return t.view(nb, Hkv, G, S, d).sum(2)

    dq, dk, dv = scale * (dS @ kk), group(scale * (dS.transpose(-1, -2) @ q)), group(P.transpose(-1, -2) @ dO)
    dq_b = U * dq.abs() + scale * ((ddS + S * u * dS.abs()) @ kk.abs())
    dk_b = U * dk.abs() + group(scale * ((ddS + G * S * u * dS.abs()).transpose(-1, -2) @ q.abs()))
    dv_b = U * dv.abs() + group(((U + eP + G * S * u) * P).transpose(-1, -2) @ dO.abs())
    res = dict(dq=dq, dk=dk, dv=dv, dq_bound=dq_b, dk_bound=dk_b, dv_bound=dv_b)
    res = {n: rows_of(t) for n, t in res.items()}
    res.update(out=rows_of(out), out_b=rows_of(out).float().to(bf), lse=f["lse"].reshape(nb * Hq, S))
    return res


def attn_bwd_emulate(qkv, dout, Hq, Hkv, d, scale, lens, causal=True):
    """the kernel: D = rowsum(dO bf16(out)); P and dS = P (dP - D) rounded to bf16 for the products; one output rounding"""
    nb, S, _ = qkv.shape
    G = Hq // Hkv
    q, k, v = heads(qkv[..., :Hq * d], Hq, d), heads(qkv[..., Hq * d:(Hq + Hkv) * d], Hkv, d), heads(qkv[..., (Hq + Hkv) * d:], Hkv, d)
    dO = heads(dout, Hq, d)
    _, _, P = _probs(q, k, scale, visible(nb, S, S, lens, causal))
    kk, vv = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    out_b = rbf(P @ vv)
    dS = rbf(P * (dO @ vv.transpose(-1, -2) - (dO * out_b).sum(-1, keepdim=True)))

    def group(t):
        return t.view(nb, Hkv, G, S, d).sum(2)

    return tuple(rows_of(rbf(t)) for t in (scale * (dS @ kk), group(scale * (dS.transpose(-1, -2) @ q)),
                                           group(rbf(P).transpose(-1, -2) @ dO)))


# ------------------------------------------------------------------------------------------------------------------- tests
_TABLES = {"rms_case": "RMS_CASES", "qk_case": "QK_CASES", "swiglu_case": "SWIGLU_CASES", "attn_case": "ATTN_CASES",
           "fwd_case": "FWD_UNEQUAL_CASES", "d64_case": "D64_CASES"}


def pytest_generate_tests(metafunc):
    """the cases are the GPU module's tables (imported here, at collection: that module imports this one at its top)"""
    import test_gpu_decoder_train_ops as gpu
    for arg, table in _TABLES.items():
        if arg in metafunc.fixturenames:
            metafunc.parametrize(arg, getattr(gpu, table), ids=lambda c: "-".join(str(x).replace(" ", "") for x in c))


def _report(name, ratio):
    print(f"emulated error / bound, {name}: {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def test_near_tie_and_ulp_helpers():
    x = torch.tensor([1.0, 1.0078125, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 3.0 + 2.0 ** -7, -0.75 - 2.0 ** -9, 0.0], dtype=f64)
    assert near_tie(x).tolist() == [False, False, True, True, True, True, False]
    assert bf16_ulp(torch.tensor([1.0, 1.99, 2.0, 0.3], dtype=f64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -9]
    frac = near_tie(torch.randn(1 << 20, generator=_gen(9), dtype=f64)).double().mean().item()
    assert 1e-4 < frac < 1e-3, frac


def test_rmsnorm_emulation_inside_bound(rms_case):
    rows, C, with_dres = rms_case
    inp = rms_inputs(rows, C, with_dres)
    m = rms_model(**inp)
    assert m["near_frac"] < 0.01, m["near_frac"]
    dx, dw = rms_emulate(**inp)
    _report("rmsnorm dx", worst((dx - m["dx"]).abs(), m["dx_bound"]))
    assert torch.equal(dw, m["dw"])                                   # float64 xhat rounds as the reference's
    dx32, dw32 = rms_emulate(work=torch.float32, **inp)               # fp32 xhat: near ties may fall to the other side
    _report("rmsnorm dx (fp32 statistics)", worst((dx32 - m["dx"]).abs(), m["dx_bound"]))
    _report("rmsnorm dw (fp32 statistics)", worst((dw32 - m["dw"]).abs(), m["dw_bound"]))


def test_qk_norm_rope_emulation_inside_bound(qk_case):
    rows, Hq, Hkv, D, norm, f32, _ = qk_case
    inp = dict(qk_inputs(rows, Hq, Hkv, D, norm, f32), Hq=Hq, Hkv=Hkv, D=D)
    m = qk_model(**inp)
    assert m["near_frac"] < 0.01, m["near_frac"]
    for work in (f64, torch.float32):
        out, dwq, dwk = qk_emulate(work=work, **inp)
        _report(f"qk_norm_rope dq|dk ({work})", worst((out - m["out"]).abs(), m["out_bound"]))
        if norm:
            _report(f"qk_norm_rope dwq ({work})", worst((dwq - m["dwq"]).abs(), m["dwq_bound"]))
            _report(f"qk_norm_rope dwk ({work})", worst((dwk - m["dwk"]).abs(), m["dwk_bound"]))
    if not norm:   # the identity row passes through bit for bit
        r = rows // 2
        assert torch.equal(out[r], inp["dy"][r, :(Hq + Hkv) * D].double())


def test_swiglu_emulation_inside_bound(swiglu_case):
    rows, I = swiglu_case[:2]
    inp = swiglu_inputs(rows, I)
    g = inp["gu"][:, :I].float()
    assert rows * I < 64 or (g.max() > 20 and g.min() < -20)
    m = swiglu_model(**inp)
    d_gate, d_up = swiglu_emulate(**inp)
    _report("swiglu d_gate", worst((d_gate - m["d_gate"]).abs(), m["d_gate_bound"]))
    _report("swiglu d_up", worst((d_up - m["d_up"]).abs(), m["d_up_bound"]))


def _fwd_ratio(q, k, v, scale, vis):
    f = attn_fwd_model(q, k, v, scale, vis)
    return worst((attn_fwd_emulate(q, k, v, scale, vis) - f["out"]).abs(), f["out_bound"])


def test_attention_emulation_inside_bound(attn_case):
    nb, S, Hq, Hkv, d, lens = attn_case
    inp = attn_inputs(nb, S, Hq, Hkv, d)
    scale = d ** -0.5
    m = attn_bwd_model(inp["qkv"], inp["dout"], Hq, Hkv, d, scale, lens)
    for name, e in zip(("dq", "dk", "dv"), attn_bwd_emulate(inp["qkv"], inp["dout"], Hq, Hkv, d, scale, lens)):
        _report("flash backward " + name, worst((e - m[name]).abs(), m[name + "_bound"]))
    x = inp["qkv"]
    _report("attention forward out", _fwd_ratio(heads(x[..., :Hq * d], Hq, d), heads(x[..., Hq * d:(Hq + Hkv) * d], Hkv, d),
                                                heads(x[..., (Hq + Hkv) * d:], Hkv, d), scale, visible(nb, S, S, lens)))
    if lens is not None:   # keys at or beyond the length get exactly zero
        for b, n in enumerate(lens):
            assert (m["dk"][b, n:] == 0).all() and (m["dv"][b, n:] == 0).all()


def test_attention_forward_unequal_lengths_inside_bound(fwd_case):
    nb, Sq, Skv, Hq, Hkv, d, lens = fwd_case
    inp = attn_inputs(nb, Sq, Hq, Hkv, d, Skv=Skv)
    kv = inp["kv"]
    _report("attention forward out (Sq < Skv)", _fwd_ratio(heads(inp["q"], Hq, d), heads(kv[..., :Hkv * d], Hkv, d),
                                                           heads(kv[..., Hkv * d:], Hkv, d), d ** -0.5, visible(nb, Sq, Skv, lens)))


def test_flash_d64_emulation_inside_bound(d64_case):
    S, H = d64_case
    inp = attn_inputs(2, S, H, H, 64)
    m = attn_bwd_model(inp["qkv"], inp["dout"], H, H, 64, 0.125, None, causal=False)
    for name, e in zip(("dq", "dk", "dv"), attn_bwd_emulate(inp["qkv"], inp["dout"], H, H, 64, 0.125, None, causal=False)):
        _report("flash d64 backward " + name, worst((e - m[name]).abs(), m[name + "_bound"]))


def test_bounds_are_tight_enough_to_see_one_wrong_tile():
    """the reason for per-element bounds: dropping one query head of a group from dk, or letting key kv_len be seen, breaks the bound
    on the elements concerned by an order of magnitude, where a whole-tensor rms moves by a few per cent"""
    nb, S, Hq, Hkv, d = 1, 129, 2, 1, 64
    inp = attn_inputs(nb, S, Hq, Hkv, d)
    m = attn_bwd_model(inp["qkv"], inp["dout"], Hq, Hkv, d, 0.125, (65,))
    one_more = attn_bwd_model(inp["qkv"], inp["dout"], Hq, Hkv, d, 0.125, (66,))
    assert worst((one_more["dq"] - m["dq"]).abs(), m["dq_bound"]) > 10
    assert worst((one_more["dk"] - m["dk"]).abs()[:, 65:], m["dk_bound"][:, 65:] + 1e-300) > 10
    assert math.isfinite(m["dq_bound"].max().item())
