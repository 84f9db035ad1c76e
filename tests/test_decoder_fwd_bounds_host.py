"""Host: the per-element error bounds that tests/test_gpu_decoder_fwd_bounds.py holds the decoder's forward row kernels to --
u2tok_rmsnorm_bf16 (rmsnorm_row<NC>, csrc/rows.h), u2tok_qk_norm_rope / u2tok_qk_norm_rope_kv (qk_norm_rope_kernel<D, CS>) and
u2tok_swiglu_bf16 (csrc/decoder.hip) -- as pure functions of the rounded inputs, next to a torch fp32 emulation of each kernel's
arithmetic and rounding points.  These three kernels are what "bit-equal to" means in most of the decoder's other tests (the norm in
a product's tail, the decode head, the quantising append, the GEMM pair forms, the whole-stack step), so they are held here to
float64 themselves.  The pattern, `Elem` (U, tiny, rnd, ulp), `rounding`, `stored`, `ratio` and `midpoint_within` are those of
tests/test_row_fwd_bounds_host.py; u = 2^-24 is the unit roundoff of fp32, U that of the element type.  Every bound is first order
and without a fitted factor: one U per rounding to the element type, charged on the value that is rounded, and n u sum |terms| for
an fp32 sum of n terms in any order.

RMSNorm.  y = rnd(rnd(x rstd) w), rstd = rsqrt(mean(x^2) + eps).  With n = x rstd and e_r = (C / 2 + 3) u (the C-term sum of exact
squares, halved by the root; the division, the addition of eps, rsqrtf): the inner rounding rounding(|n| (1 + e_r)) |w|, the fp32
terms (e_r + u) |y|, and the store rounding of |y| plus both.  Both rounding points are visible, so there is a sharper second
assertion (`norm_points`, `points_hold`): every element equals rnd(rnd(n) w) evaluated in float64, bit for bit (the second product
is exact in fp32), except where n lies within e_r |n| of a midpoint of the element type; there it must be rnd(n_below w) or
rnd(n_above w).  At most NEAR_TIE_CAP = 10 % of a case's elements may be excused, asserted on the reference alone.

q | k head norm + rotary.  h = x, or the RMSNorm of the head's D columns with wq / wk, which the kernel rounds to the element type
(the norm's two roundings, charged as above with C = D); r0 = a c0 - b s0, r1 = b c1 + a s1 with a, b the halves of h and c0, s0,
c1, s1 read from the first and the second half of the table row.  Bound: the norm's bound carried through the rotation,
da |c| + db |s|, plus 2 u (|a c| + |b s|) for two fp32 products and their sum, plus the store rounding.  Without the norm and with
a 16-bit table both products are exact in fp32 (8 x 8 or 11 x 11 mantissa bits) and their sum is rounded once to fp32 and once to
the element type, with or without an fma: every element then equals the float64 expression rounded through fp32 and the element
type, bit for bit (`exact`).  At least half of the tables have independent halves (an angle per element): a HuggingFace table
repeats its half and cannot see a kernel that reads the wrong one.

SwiGLU.  out = rnd(rnd(silu(g)) up), silu evaluated as g / (1 + __expf(-g)): (4 + 2 |g|) u |silu| for the fp32 evaluation (as
swiglu_model of tests/test_decoder_train_bounds_host.py charges it), the rounding of silu times |up|, the store rounding.  One
derived allowance: for g <= -87, 1 + e^-g may overflow fp32 to +inf (from g = -88.73 down), and the kernel then returns -+0 where
the true |silu| = |g| e^-|g| is still a normal number of bf16 (2e-37 at g = -89); the bound adds |g| e^-|g| |up| there.  Benign: an
absolute error below 2e-36 |up| on a value the next product cannot tell from zero.

Emulated error / bound over the tables: rmsnorm 0.55 to 0.95, qk_norm_rope 0.65 to 0.99, swiglu 0.70 to 0.93 -- a correct rounding
of a value just above a power of two errs by U |value|, so 1.0 is a correctly rounded result on the worst-placed element and 2.0 one
a whole ulp off; with two roundings in a row both have to be worst-placed at once.  Largest near-tie share: 8.3 % (C = 8192, 37
rows, where e_r is 2^-12; none at C = 8); 331 emulated elements over the table differ from rnd(rnd(n) w), every one of them at a
near tie and equal to a candidate (all on the eps-dominated row: 1000 x falls on exact midpoints of bf16).  Every one of the 11
planted faults leaves the bound on at least one case of its table (asserted)."""
import math

import torch

from test_row_fwd_bounds_host import BF16, F16, _gen, f32, f64, midpoint_within, ratio, rounding, stored, u

EPS = 1e-6
NEAR_TIE_CAP = 0.10


def to_el(t, el):
    """float64 -> the element type, through fp32 (exact for every value rounded here but a float64 within 2^-29 of a midpoint)"""
    return t.float().to(el.dtype)


def neighbours(t, el):
    """the two adjacent values of the element type that bracket float64 t: (towards zero, away from zero)"""
    a = t.abs().clamp_min(2.0 ** -120)
    ulp = el.ulp(a)
    lo = torch.floor(a / ulp) * ulp
    return torch.sign(t) * lo, torch.sign(t) * (lo + ulp)


def rnd64(t, el):
    """float64 t rounded to the element type in ONE step (nearest, ties to even), as float64: el.rnd goes through fp32 and so
    rounds a value within 2^-29 of a midpoint twice"""
    lo, hi = neighbours(t, el)
    a, mid = t.abs(), (lo.abs() + hi.abs()) / 2
    even = torch.floor(lo.abs() / el.ulp(a.clamp_min(2.0 ** -120))) % 2 == 0
    return torch.where((a < mid) | ((a == mid) & even), lo, hi)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- RMSNorm
def _norm_model(x, w, eps, el):
    """RMSNorm over the last dim of x (float64) with weights w (float64, broadcastable) -> (n = x rstd, y = n w, what y is off by
    before its store rounding, e_r).  See the module docstring."""
    C = x.shape[-1]
    eps = float(torch.tensor(eps, dtype=f32))
    n = x * (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    e_r = (C / 2 + 3) * u
    y = n * w
    return n, y, rounding(n.abs() * (1 + e_r), el) * w.abs() + (e_r + u) * y.abs(), e_r


def norm_points(n, w, e_r, el):
    """the rounding points of the norm as bits of the element type: want = rnd(rnd(n) w); where n is within e_r |n| of a midpoint
    (tie) the kernel's fp32 n may round to the other neighbour: below = rnd(n_below w), above = rnd(n_above w)"""
    lo, hi = neighbours(n, el)
    tie = midpoint_within(n, e_r * n.abs(), el)
    return dict(want=to_el(rnd64(n, el) * w, el), below=to_el(lo * w, el), above=to_el(hi * w, el), tie=tie,
                share=tie.double().mean().item())


def points_hold(got, p, sel=slice(None)):
    """-> (every element of got[sel] has the bits of want, or of a candidate where excused; the number of excused mismatches)"""
    g = _bits(got.detach().cpu()[sel])
    same = g == _bits(p["want"][sel])
    alt = p["tie"][sel] & ((g == _bits(p["below"][sel])) | (g == _bits(p["above"][sel])))
    return bool((same | alt).all()), int((~same & alt).sum())


def rms_inputs(rows, C, el=BF16):
    """x = 1.5 N(0, 1) (rows, C), w = 1 + 0.5 N(0, 1).  From rows = 5 up: row 1 scaled by 2^-40 (f16: 2^-14, which its subnormals
    survive) so that eps dominates the mean square; row 2 scaled by 2^30 (f16: 2^4: the squares stay finite in fp32 either way);
    row 3 zero except for one element; row 4 all zero."""
    g = _gen(21, rows, C)
    x = torch.randn(rows, C, generator=g) * 1.5
    w = 1.0 + 0.5 * torch.randn(C, generator=g)
    if rows >= 5:
        x[1] *= 2.0 ** (-40 if el is BF16 else -14)
        x[2] *= 2.0 ** (30 if el is BF16 else 4)
        one = x[3, (C * 2) // 3].item()
        x[3] = 0.0
        x[3, (C * 2) // 3] = one
        x[4] = 0.0
    return dict(x=x.to(el.dtype), w=w.to(el.dtype), eps=EPS)


def rms_model(x, w, eps, el=BF16):
    """y = x rstd w in float64, its bound and the rounding points"""
    n, y, pre, e_r = _norm_model(x.double(), w.double(), eps, el)
    return dict(y=y, bound=stored(y, pre, el), points=norm_points(n, w.double(), e_r, el))


RMS_FAULTS = ("no_eps", "mean_over_tier", "short_sum", "w_chunk_off")


def _tier_columns(C):
    """NC 512 of the instantiation the launcher picks"""
    return 512 * (2 if C <= 1024 else 4 if C <= 2048 else 8 if C <= 4096 else 16)


def rms_emulate(x, w, eps, el=BF16, fault=None):
    """the kernel in torch fp32: the sum of squares, / C, + eps, rsqrt; rnd(x rstd); rnd(n w).  Faults: eps dropped; the mean over
    NC 512 columns; the last partly filled set of 64 chunks left out of the sum of squares; w read one 8-element chunk off."""
    v = x.float()
    C = v.shape[-1]
    sq = v * v
    if fault == "short_sum" and C % 512:
        sq = sq[..., :C - C % 512]
    s = sq.sum(-1, keepdim=True) if sq.shape[-1] else torch.zeros_like(v[..., :1])
    rstd = torch.rsqrt(s / float(_tier_columns(C) if fault == "mean_over_tier" else C) + (0.0 if fault == "no_eps" else eps))
    ww = w.float().roll(-8) if fault == "w_chunk_off" else w.float()
    return to_el(el.rnd(v * rstd).float() * ww, el)


# ------------------------------------------------------------------------------------------------------- head norm + rotary
def qk_inputs(rows, Hq, Hkv, D, norm, tbl_f32, table, el=BF16):
    """qkv (rows, (Hq + 2 Hkv) D) = 1.5 N(0, 1), wq / wk = 1 + 0.3 N(0, 1) (norm), cos / sin (rows, D) fp32 or of the element type.
    table "free": an independent angle per element, uniform over the circle (cos^2 + sin^2 = 1 element-wise, the two halves
    unrelated); otherwise a real rotary table of that theta ("1e4", "1e6") at positions 1003 .. 1002 + rows, its half repeated.
    From rows = 5 up, row rows // 2 of the table is the identity cos = 1, sin = 0."""
    g = _gen(22, rows, Hq, Hkv, D, int(norm), int(tbl_f32))
    qkv = (torch.randn(rows, (Hq + 2 * Hkv) * D, generator=g) * 1.5).to(el.dtype)
    wq, wk = ((1.0 + 0.3 * torch.randn(D, generator=g)).to(el.dtype) for _ in range(2))
    if table == "free":
        ang = torch.rand(rows, D, generator=g, dtype=f64) * (2 * math.pi)
    else:
        inv = 1.0 / (float(table) ** (torch.arange(0, D, 2, dtype=f64) / D))
        ang = (1003 + torch.arange(rows, dtype=f64))[:, None] * inv[None]
        ang = torch.cat([ang, ang], -1)
    cos, sin = ang.cos().float(), ang.sin().float()
    if rows >= 5:
        cos[rows // 2], sin[rows // 2] = 1.0, 0.0
    if not tbl_f32:
        cos, sin = cos.to(el.dtype), sin.to(el.dtype)
    return dict(qkv=qkv, wq=wq if norm else None, wk=wk if norm else None, cos=cos, sin=sin, eps=EPS)


def _halves(t, hf):
    return t[..., :hf], t[..., hf:]


def qk_model(qkv, wq, wk, cos, sin, eps, Hq, Hkv, D, el=BF16):
    """the q | k columns (rows, (Hq + Hkv) D) in float64 and their bound; with norm the rounding points of the head norm
    ((rows, Hq + Hkv, D): what the identity row must come back as); without norm and with a 16-bit table `exact`, the bits every
    element must have"""
    rows, H, hf = qkv.shape[0], Hq + Hkv, D // 2
    x = qkv[:, :H * D].double().view(rows, H, D)
    res = {}
    if wq is not None:
        w = torch.cat([wq.double().expand(Hq, D), wk.double().expand(Hkv, D)])[None]
        n, h, pre, e_r = _norm_model(x, w, eps, el)
        dh = stored(h, pre, el)
        res["points"] = norm_points(n, w.expand_as(n), e_r, el)
    else:
        h, dh = x, torch.zeros_like(x)
    (a, b), (da, db) = _halves(h, hf), _halves(dh, hf)
    (c0, c1), (s0, s1) = _halves(cos.double()[:, None], hf), _halves(sin.double()[:, None], hf)
    r = torch.cat([a * c0 - b * s0, b * c1 + a * s1], -1)
    mag = torch.cat([(a * c0).abs() + (b * s0).abs(), (b * c1).abs() + (a * s1).abs()], -1)
    carried = torch.cat([da * c0.abs() + db * s0.abs(), db * c1.abs() + da * s1.abs()], -1)
    res.update(out=r.reshape(rows, H * D), bound=stored(r, carried + 2 * u * mag, el).reshape(rows, H * D))
    if wq is None and cos.dtype != f32:
        res["exact"] = to_el(r, el).reshape(rows, H * D)
    return res


QK_FAULTS = ("rotate_sign", "first_half_table", "d96_over_128", "k_with_wq", "position_in_sequence")


def qk_emulate(qkv, wq, wk, cos, sin, eps, Hq, Hkv, D, el=BF16, fault=None, S=None):
    """the kernel in torch fp32.  Faults: the sign of rotate_half; c0 / s0 for both halves; the mean of a D = 96 head over 128; the k
    heads normed with wq; the table row taken at the position within the sequence (row % S)."""
    rows, H, hf = qkv.shape[0], Hq + Hkv, D // 2
    h = qkv[:, :H * D].float().view(rows, H, D)
    if wq is not None:
        w = torch.cat([wq.float().expand(Hq, D), (wq if fault == "k_with_wq" else wk).float().expand(Hkv, D)])[None]
        den = 128.0 if (fault == "d96_over_128" and D == 96) else float(D)
        rstd = torch.rsqrt((h * h).sum(-1, keepdim=True) / den + eps)
        h = el.rnd(el.rnd(h * rstd).float() * w).float()
    idx = torch.arange(rows)
    if fault == "position_in_sequence" and S:
        idx = idx % S
    a, b = _halves(h, hf)
    (c0, c1), (s0, s1) = _halves(cos.float()[idx][:, None], hf), _halves(sin.float()[idx][:, None], hf)
    if fault == "first_half_table":
        c1, s1 = c0, s0
    sg = -1.0 if fault == "rotate_sign" else 1.0
    return to_el(torch.cat([a * c0 - sg * (b * s0), b * c1 + sg * (a * s1)], -1), el).reshape(rows, H * D)


# ------------------------------------------------------------------------------------------------------------------ SwiGLU
SWIGLU_EDGES = (-89.0, 89.0, -88.0, 1e4, -87.0, -1e4, 88.0, -104.0, -0.0, 0.0, 1e-30, -1e-30, 20.0, -20.0, 30.0, -30.0, 60.0, -60.0,
                87.0, 100.0, -100.0, 104.0, -1.2785, 2.0 ** -126)


def swiglu_inputs(rows, I, el=BF16):
    """gate | up (rows, 2 I): the gate is 2 N(0, 1) with SWIGLU_EDGES, in that order and repeated, at a random quarter of the
    positions (at least half of them up to 24: the smallest case holds the first four); up = 1.5 N(0, 1), clamped to +-4 where
    |gate| >= 20 so that the product stays finite in f16"""
    g = _gen(23, rows, I)
    total = rows * I
    gate = torch.randn(total, generator=g) * 2
    k = max(total // 4, min(total // 2, len(SWIGLU_EDGES)))
    gate[torch.randperm(total, generator=g)[:k]] = torch.tensor(SWIGLU_EDGES)[torch.arange(k) % len(SWIGLU_EDGES)]
    gate = gate.view(rows, I)
    up = torch.randn(rows, I, generator=g) * 1.5
    up = torch.where(gate.abs() >= 20, up.clamp(-4, 4), up)
    return dict(gu=torch.cat([gate, up], 1).to(el.dtype))


def swiglu_model(gu, el=BF16, overflow_allowance=True):
    """silu(g) up in float64 and its bound: ds = the fp32 evaluation (4 + 2 |g|) u |silu| and the rounding of silu on top of it;
    ds |up| (the product of two element-type values is exact in fp32); the store rounding; for g <= -87 the overflow allowance
    |g| e^-|g| |up| (module docstring)"""
    I = gu.shape[1] // 2
    g, up = gu[:, :I].double(), gu[:, I:].double()
    silu = g * torch.sigmoid(g)
    pre = stored(silu, (4 + 2 * g.abs()) * u * silu.abs(), el) * up.abs()
    if overflow_allowance:
        pre = pre + torch.where(g <= -87, g.abs() * torch.exp(-g.abs()) * up.abs(), torch.zeros_like(g))
    out = silu * up
    return dict(out=out, bound=stored(out, pre, el))


SWIGLU_FAULTS = ("swapped", "up_is_gate_column")


def swiglu_emulate(gu, el=BF16, fault=None):
    """the kernel in torch fp32: g / (1 + exp(-g)), rounded; times up, rounded.  Faults: gate and up swapped; up read at column c in
    place of I + c."""
    I = gu.shape[1] // 2
    g, up = gu[:, :I].float(), gu[:, I:].float()
    if fault == "swapped":
        g, up = up, g
    if fault == "up_is_gate_column":
        up = g
    return to_el(el.rnd(g / (1.0 + torch.exp(-g))).float() * up, el)


# ------------------------------------------------------------------------------------------------------------------- tests
_WORST = {}


def _report(name, r):
    _WORST[name] = max(_WORST.get(name, 0.0), r)
    print(f"emulated error / bound, {name}: {r:.3f} (worst so far {_WORST[name]:.3f})")
    assert r <= 1.0, (name, r)


def _gpu():
    import test_gpu_decoder_fwd_bounds as G       # at call time: that module imports this one at its top
    return G


def _elems(i):
    """the first case of every table runs in both element types"""
    return (BF16, F16) if i == 0 else (BF16,)


def _share(name, case, p):
    print(f"{name} {case}: near ties {p['share']:.4f}")
    assert p["share"] <= NEAR_TIE_CAP, (name, case, p["share"])


def test_helpers():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, -1.3, 3.0 + 2.0 ** -7 + 2.0 ** -20, 0.0], dtype=f64)
    lo, hi = neighbours(t, BF16)
    assert lo.tolist() == [1.0, 1.0, -1.296875, 3.0, 0.0] and hi.tolist()[:4] == [1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, -1.3046875, 3.015625]
    lo, hi = neighbours(torch.tensor([1.0 + 2.0 ** -11], dtype=f64), F16)
    assert (lo.item(), hi.item()) == (1.0, 1.0 + 2.0 ** -10)
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -8, -1.3, 0.0, 2.5], dtype=f64)
    assert rnd64(t, BF16).tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -1.296875, 0.0, 2.5]
    x = torch.randn(4096, generator=_gen(20), dtype=f64)
    for el in (BF16, F16):       # the two-step rounding differs from it only next to a midpoint (f16: one element of these, and wrongly)
        clear = ~midpoint_within(x, u * x.abs(), el)
        assert torch.equal(rnd64(x, el)[clear], el.rnd(x)[clear]) and clear.sum() > 4000
        assert ((rnd64(x, el) - x).abs() <= (el.rnd(x) - x).abs()).all()
    # a mismatch is excused only at a near tie, and only towards a candidate
    n, w = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.3], dtype=f64), torch.tensor([3.0, 3.0], dtype=f64)
    p = norm_points(n, w, 8 * u, BF16)
    assert p["tie"].tolist() == [True, False] and p["want"].tolist() == [3.03125, 3.890625] and p["below"].tolist()[0] == 3.0
    assert points_hold(p["want"], p) == (True, 0) and points_hold(torch.tensor([3.0, 3.890625]).to(torch.bfloat16), p) == (True, 1)
    assert not points_hold(torch.tensor([3.03125, 3.875]).to(torch.bfloat16), p)[0]
    assert not points_hold(torch.tensor([3.046875, 3.890625]).to(torch.bfloat16), p)[0]
    assert _tier_columns(8) == 1024 and _tier_columns(1032) == 2048 and _tier_columns(4096) == 4096 and _tier_columns(4104) == 8192


def test_rmsnorm_emulation_inside_bound_and_faults_outside():
    broke = dict.fromkeys(RMS_FAULTS, 0)
    worst_share = excused = 0
    for i, (C, rows) in enumerate(dict.fromkeys((C, rows) for C, rows, _ in _gpu().RMS_CASES)):       # (padded: the same values)
        for el in _elems(i):
            inp = rms_inputs(rows, C, el)
            m = rms_model(**inp, el=el)
            _share("rmsnorm", (C, rows, el.name), m["points"])
            worst_share = max(worst_share, m["points"]["share"])
            got = rms_emulate(**inp, el=el)
            _report("rmsnorm", ratio(got, m["y"], m["bound"]))
            ok, n_alt = points_hold(got, m["points"])
            assert ok, ("an emulated mismatch with rnd(rnd(n) w) that no near tie explains", C, rows, el.name)
            excused += n_alt
            if rows >= 5:
                assert (got[4] == 0).all(), "the all-zero row"
            for f in RMS_FAULTS:
                broke[f] += ratio(rms_emulate(**inp, el=el, fault=f), m["y"], m["bound"]) > 1.0
    print(f"largest near-tie share {worst_share:.4f}; {excused} emulated elements took the other candidate")
    print("cases on which each fault leaves the bound:", broke)
    assert all(broke.values()), broke


def test_qk_norm_rope_emulation_inside_bound_and_faults_outside():
    G = _gpu()
    broke = dict.fromkeys(QK_FAULTS, 0)
    cases = [(rows, Hq, Hkv, D, norm, tf, table, None) for rows, Hq, Hkv, D, norm, tf, _, table in G.QK_CASES] + \
            [(nb * S, Hq, Hkv, D, norm, tf, table, S) for nb, S, Hq, Hkv, D, norm, tf, table, _, _ in G.QK_KV_CASES]
    assert 2 * sum(c[6] == "free" for c in cases) >= len(cases), "at least half of the tables have independent halves"
    assert {(c[3], c[4], c[5]) for c in cases[:len(G.QK_CASES)]} == {(D, n, t) for D in (64, 96, 128) for n in (0, 1) for t in (0, 1)}
    for i, (rows, Hq, Hkv, D, norm, tf, table, S) in enumerate(cases):
        for el in _elems(i):
            inp = dict(qk_inputs(rows, Hq, Hkv, D, norm, tf, table, el), Hq=Hq, Hkv=Hkv, D=D)
            m = qk_model(**inp, el=el)
            got = qk_emulate(**inp, el=el)
            _report("qk_norm_rope", ratio(got, m["out"], m["bound"]))
            if norm:
                _share("qk_norm_rope", (rows, Hq, Hkv, D, el.name), m["points"])
            if "exact" in m:
                assert torch.equal(_bits(got), _bits(m["exact"])), "the exact case"
            if rows >= 5:       # the identity row: the input's bits, or the norm's rounding points
                r = rows // 2
                if norm:
                    assert points_hold(got.view(rows, Hq + Hkv, D), m["points"], r)[0], "identity row"
                else:
                    assert torch.equal(_bits(got[r]), _bits(inp["qkv"][r, :(Hq + Hkv) * D])), "identity row"
            for f in QK_FAULTS:
                broke[f] += ratio(qk_emulate(**inp, el=el, fault=f, S=S), m["out"], m["bound"]) > 1.0
    print("cases on which each fault leaves the bound:", broke)
    assert all(broke.values()), broke


def test_swiglu_emulation_inside_bound_and_faults_outside():
    broke = dict.fromkeys(SWIGLU_FAULTS, 0)
    seen = set()
    for i, (rows, I) in enumerate(dict.fromkeys((rows, I) for rows, I, _, _ in _gpu().SWIGLU_CASES)):
        for el in _elems(i):
            inp = swiglu_inputs(rows, I, el)
            g, up = inp["gu"][:, :I].double(), inp["gu"][:, I:].double()
            seen |= set(g.flatten().tolist()) if el is BF16 else set()
            assert (up.abs()[g.abs() >= 20] <= 4).all()
            m = swiglu_model(**inp, el=el)
            got = swiglu_emulate(**inp, el=el)
            assert torch.isfinite(got.float()).all()
            _report("swiglu", ratio(got, m["out"], m["bound"]))
            for f in SWIGLU_FAULTS:
                broke[f] += ratio(swiglu_emulate(**inp, el=el, fault=f), m["out"], m["bound"]) > 1.0
    assert {float(torch.tensor(e).to(torch.bfloat16)) for e in SWIGLU_EDGES} <= seen, "every edge gate is in some case"
    print("cases on which each fault leaves the bound:", broke)
    assert all(broke.values()), broke


def test_swiglu_overflow_allowance_is_what_the_denominator_loses():
    """g = -89: 1 + e^89 is +inf in fp32 and the emulation returns -0 where silu = -89 e^-89 = -2e-37 is a normal number of bf16; the
    bound without the allowance is broken there, the bound with it is not.  g = -88 (e^88 = 1.65e38, finite) needs none."""
    gu = torch.tensor([[-89.0, -88.0] + [0.0] * 6 + [3.0, 3.0] + [1.0] * 6]).to(torch.bfloat16)
    got = swiglu_emulate(gu)
    assert got[0, 0].item() == 0 and got[0, 1].item() != 0
    tight, m = swiglu_model(gu, overflow_allowance=False), swiglu_model(gu)
    err = (got.double() - m["out"]).abs()
    assert err[0, 0] > tight["bound"][0, 0] and err[0, 0] <= m["bound"][0, 0] and err[0, 1] <= tight["bound"][0, 1]
    assert m["out"][0, 0].abs() > 2.0 ** -126
