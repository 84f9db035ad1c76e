"""Host: the references, bounds and emulations that tests/test_gpu_front_end_bounds.py holds the front end and token selection
kernels to -- im2col_patches, fill_rows (csrc/vision.hip), score_gemv, topk_sorted, gather_rows, multiscale_pool with
dmtp_gate_partial (csrc/select.hip) -- on the pattern of tests/test_row_fwd_bounds_host.py, whose conventions (`Elem`, U, u, `stored`,
`ratio`) and helpers are imported, not copied.  The case tables and input generators are tests/front_end_cases.py.

Exact kernels (im2col, fill_rows, gather_rows, topk_sorted, pooling of small integers) have a *_reference in plain torch and a
*_restate at index level (the arithmetic a kernel has to do: decode a flat item index, clamp, build a 64-bit key), with `fault=` for a
kernel that is wrong in one named way.  Bounded kernels (score_gemv, pooling of N(0, 1) data with and without gates) have a *_model
(float64 reference and a first-order bound per element without a fitted factor) and an *_emulate in torch fp32 that rounds where the
kernel rounds.  The tests run every restatement and emulation over the same tables as the GPU module, assert equality or the bound,
and assert that each of the 22 planted faults (3 of them on score_gemv, beyond the ones asked for) leaves it on at least one case.

The canonical top-k order (oracle.canonical_topk, torch.sort(descending=True, stable=True)): descending score, -0.0 == +0.0, ties by
ascending index; every NaN -- either sign bit, any payload -- ranks first, above +inf, ties among NaNs by ascending index as well.

score_gemv.  The kernel sums the E exact products in fp64 in an order of its own and rounds once to fp32.  Any fp64 order is within
d = E 2^-53 sum|terms| of the exact sum (first order), so the score is within half an fp32 ulp + d of math.fsum's, and bit-equal to
its rounding unless that exact sum lies within d of a midpoint between two fp32 values (`near_tie32`).  On dyadic data (m 2^-6,
|m| <= 255) every partial sum is an integer multiple of 2^-12 below 2^28: exact in any order, the reference is integer arithmetic.
The same argument makes d = 0 on any row whose terms share a grain g (the lowest bit set in any term) with sum|terms| < 2^52 g:
every narrow case and most wide ones (score_model).  The cancelling rows are scaled with E so that d stays about 2^-8 of an ulp of
the result: at most 1 % of the hard scores may be excused as near a boundary; on the N(0, 1) cases none is (asserted here for the
seeds in use).

Gated pooling (`multiscale_gate_model`).  logit_s = sum_e colmean_s[e] gate_w[e] + gate_b, colmean_s the mean of the first
floor(k / s) s tokens.  In fp32: the token sums per column, any order, k u sum_t |x|; the division and the product, 2 u; the column
dot, any order inside a group of 256 columns and then over the 16 slabs x ceil(E / 256) groups of partial logits that the workspace
holds (include/u2tok.h), (256 + 16 ceil(E / 256)) u sum|terms|, where sum|terms| <= A_s = sum_e mean_t|x| |gate_w| whatever the slabs are;
the bias, u.  The softmax over the scales present is test_row_fwd_bounds_host._softmax_err (the argument's error times the result
for __expf, 3 u |a - m| + 2 u for the instruction, the quotient (n + 4) u).  An output element is (sum of s tokens) (gate_s / s):
(s - 1) u mean|x| gate_s for the sum, u for the product, one U for the store (`stored`).  The fp32 gates of the emulation sum to 1
within 3 u per batch element (the kernel does not export its gates; through the bf16 output they are visible to U only).

Preprocessing (`preprocess_model`).  The float64 reference follows u2Transform.adaptive_resize step by step: np.percentile on the
fp32 voxels, the box by nonzero, the geometry by the Python expressions of u2Transform.py:75-98, MONAI's erf taps in float32 (their
definition), the zero-padded separable convolution and the align-corners interpolation in double with the source index in float32
as torch computes it.  Bound: u |y| for the one fp32 rounding of the scaled value, carried through filter and interpolation;
(2 tail + 1) u sum|tap x| per filtered axis; 7 u times the interpolated magnitude; one rounding of the output type.  Status, box,
output size and both percentiles (as float32) are exact.

Worst emulated error / bound over the tables: score_gemv 1.00 (an exact sum that is a midpoint between two fp32 values: half an ulp
is the whole bound), pooling 1.00 fixed and 0.84 gated, preprocessing 0.99 (into a 16-bit type)."""
import math

import numpy as np
import pytest
import torch

import front_end_cases as K
from oracle import u2_oracle as O
from test_decoder_train_bounds_host import _gen, bf16_ulp, near_tie, rbf, worst  # noqa: F401  (the shared helpers)
from test_row_fwd_bounds_host import BF16, ELEMS, F16, Elem, _softmax_err, f32, f64, ratio, stored, u  # noqa: F401

SENTINEL = -0x5A5A5A5A5A5A5A5B        # what the int64 index buffers are pre-filled with
EXCUSED_SHARE = 0.01


# ------------------------------------------------------------------------------------------------------------------ im2col
def im2col_reference(vol, patch, el=BF16):
    """Rearrange("b c (h p1) (w p2) (d p3) -> b (h w d) (p1 p2 p3 c)") (vit.py:90-99, c = 1) of vol (n, D, H, W), rounded to the
    element type by torch"""
    n, D, H, W = vol.shape
    p1, p2, p3 = patch
    x = vol.reshape(n, D // p1, p1, H // p2, p2, W // p3, p3).permute(0, 1, 3, 5, 2, 4, 6)
    return x.reshape(n, -1, p1 * p2 * p3).to(el.dtype)


IM2COL_FAULTS = ("p23_swapped", "hw_swapped")


def im2col_restate(vol, patch, el=BF16, fault=None):
    """out[chunk][(h_i nw + w_i) nd + d_i][(p1i p2 + p2i) p3 + p3i] = vol[chunk][h_i p1 + p1i][w_i p2 + p2i][d_i p3 + p3i] by flat index
    arithmetic.  Faults: the feature index decoded with p2 and p3 exchanged; the row stride of the volume taken from H instead of W
    (flat offsets wrap inside the chunk, as a read that stays in bounds would)."""
    n, D, H, W = vol.shape
    p1, p2, p3 = patch
    nw, nd = H // p2, W // p3
    tok, f = torch.arange((D // p1) * nw * nd)[:, None], torch.arange(p1 * p2 * p3)[None, :]
    d_i, w_i, h_i = tok % nd, (tok // nd) % nw, tok // (nd * nw)
    if fault == "p23_swapped":
        p3i, p2i, p1i = f % p2, (f // p2) % p3, f // (p2 * p3)
    else:
        p3i, p2i, p1i = f % p3, (f // p3) % p2, f // (p2 * p3)
    Hs, Ws = (W, H) if fault == "hw_swapped" else (H, W)
    off = (((h_i * p1 + p1i) * Hs + (w_i * p2 + p2i)) * Ws + (d_i * p3 + p3i)) % (D * H * W)
    return vol.reshape(n, -1)[:, off].to(el.dtype)


# ------------------------------------------------------------------------------------------------------- gather, fill_rows
def gather_reference(x, idx):
    """x[b][clamp(idx[b][j], 0, n - 1)] (include/u2tok.h: never read outside the batch entry)"""
    return x[torch.arange(x.shape[0])[:, None], idx.clamp(0, x.shape[1] - 1)]


GATHER_FAULTS = ("no_clamp",)


def gather_restate(x, idx, fault=None):
    """item i -> (bk, e8) -> row b n + src of the flattened source.  Fault: src unclamped (the row index wraps inside the storage)."""
    B, n, E = x.shape
    b = torch.arange(B)[:, None]
    src = idx if fault == "no_clamp" else torch.where(idx < 0, 0, torch.where(idx >= n, n - 1, idx))
    return x.reshape(B * n, E)[(b * n + src) % (B * n)]


def fill_reference(src, nb, n, dst_bs, fill):
    """the storage of (nb - 1) dst_bs + n elements pre-filled with `fill` after dst[b dst_bs + e] = src[e]"""
    st = fill.clone()
    for b in range(nb):
        st[b * dst_bs:b * dst_bs + n] = src
    return st


def fill_restate(src, nb, n, dst_bs, fill):
    st = fill.clone()
    i = torch.arange(nb * n)
    st[(i // n) * dst_bs + i % n] = src[i % n]
    return st


# ------------------------------------------------------------------------------------------------------------------- score
def ulp32(t):
    """the spacing of fp32 at |t| (float64 in, float64 out): 2^(e - 23) for 2^e <= |t| < 2^(e + 1), 2^-149 in the subnormal range"""
    _, e = torch.frexp(t.abs().clamp_min(2.0 ** -160))
    return torch.ldexp(torch.ones_like(t), (e - 24).clamp_min(-149))


def near_tie32(t, delta):
    """float64 t within delta of a midpoint between two adjacent fp32 values (`near_tie` of the bf16 modules, for fp32)"""
    ulp = ulp32(t)
    q = t.abs() / ulp
    return (q - torch.floor(q) - 0.5).abs() * ulp <= delta


def _low_bit(t):
    """the value of the lowest set bit of the float t != 0"""
    m, e = math.frexp(abs(t))
    M = int(m * 2 ** 53)
    return math.ldexp(M & -M, e - 53)


def score_model(x, w, bias, ints=None, **_):
    """ref = the exact sum of the exact products and the bias (math.fsum; integer arithmetic for dyadic data), mag = sum|terms|,
    delta = E 2^-53 mag, want = ref rounded once to fp32, bound = ulp32 / 2 + delta, near = near_tie32(ref, delta).  delta is 0 where
    the row is provably exact in ANY fp64 order, as dyadic data is: every term is a multiple of `grain` (the lowest bit set in any
    term) and mag < 2^52 grain, so every partial sum of every order is a multiple of grain below 2^53 grain, a value fp64 holds
    exactly.  That matters: a sum of products of 8-bit significands has so few bits that 2 to 3 % of N(0, 1) scores ARE midpoints
    between two fp32 values; with delta = 0 they are not excused but held to the one correct rounding (ties to even)."""
    rows, E = x.shape
    if ints is not None:
        mx, mw, mb = ints
        S = (mx * mw).sum(-1) + (0 if mb is None else mb * 64)
        assert int(S.abs().max()) < 2 ** 28
        ref = S.double() / 4096
        delta = torch.zeros_like(ref)
    else:
        wl, b = w.double().tolist(), 0.0 if bias is None else float(bias.double())
        ref, mag, grain = [], [], []
        for row in x.double().tolist():
            terms = [a * c for a, c in zip(row, wl)] + [b]
            ref.append(math.fsum(terms))
            mag.append(math.fsum(abs(t) for t in terms))
            grain.append(min([_low_bit(t) for t in terms if t] or [1.0]))
        ref, mag, grain = torch.tensor(ref, dtype=f64), torch.tensor(mag, dtype=f64), torch.tensor(grain, dtype=f64)
        delta = torch.where(mag < grain * 2.0 ** 52, 0.0, E * 2.0 ** -53 * mag)
    return dict(ref=ref, want=ref.float(), delta=delta, mag=mag if ints is None else None, bound=0.5 * ulp32(ref.abs() + delta) + delta,
                near=near_tie32(ref, delta) & (delta > 0))


def score_check(got, m):
    """got (fp32) against score_model's m: every score inside the bound, bit-equal wherever the reference is not near a boundary;
    -> (worst error / bound, number of scores excused)"""
    got = got.reshape(-1).cpu()
    r = ratio(got, m["ref"], m["bound"])
    assert r <= 1.0, f"score outside half an ulp + E 2^-53 sum|terms|: ratio {r}"
    same = got.view(torch.int32) == m["want"].view(torch.int32)
    assert bool((same | m["near"]).all()), "a score differs from the rounded exact sum away from every rounding boundary"
    return r, int(m["near"].sum())


SCORE_FAULTS = ("fp32_sum", "tail_dropped", "bias_dropped")


def score_emulate(x, w, bias, fault=None, **_):
    """the kernel in torch: fp64 products, torch's fp64 sum, the bias, one rounding to fp32.  Faults: the sum kept in fp32; the columns
    past the last full 512 (one trip of all 64 lanes) left out; the bias left out."""
    E = x.shape[-1]
    t = x.double() * w.double()
    if fault == "tail_dropped" and E % 512:
        t = t[:, :E - E % 512]
    s = t.float().sum(-1).double() if fault == "fp32_sum" else t.sum(-1)
    if bias is not None and fault != "bias_dropped":
        s = s + bias.double()
    return s.float()


# ------------------------------------------------------------------------------------------------------------------- top-k
TOPK_FAULTS = ("ties_descending", "neg_zero_below", "pad_is_zero_key", "neg_nan_last")


def topk_restate(scores, k, fault=None):
    """the kernel's keys in numpy: (orderable score bits << 32) | ~index, -0 folded into +0, every NaN mapped to the top key, the row
    padded to a power of two with keys of 0, sorted descending.  Faults: the index not complemented; -0 left below +0; the padding
    given the key of a score of 0.0; NaNs left where their bits put them (a sign-bit NaN then sorts below -inf)."""
    B, n = scores.shape
    np2 = 2
    while np2 < n:
        np2 *= 2
    s = scores.numpy().copy()
    if fault != "neg_zero_below":
        s[s == 0] = 0.0
    bits = s.view(np.uint32).astype(np.uint64)
    key = np.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)
    if fault != "neg_nan_last":
        key = np.where(np.isnan(s), np.uint64(0xFFFFFFFF), key)
    i = np.arange(np2, dtype=np.uint64)
    low = i if fault == "ties_descending" else np.uint64(0xFFFFFFFF) - i
    keys = np.zeros((B, np2), dtype=np.uint64)
    if fault == "pad_is_zero_key":
        keys[:] = (np.uint64(0x80000000) << np.uint64(32)) | low
    keys[:, :n] = (key << np.uint64(32)) | low[:n]
    top = np.sort(keys, axis=1)[:, ::-1]
    low_out = (top[:, :k] & np.uint64(0xFFFFFFFF))
    idx = low_out if fault == "ties_descending" else np.uint64(0xFFFFFFFF) - low_out
    return torch.from_numpy(idx.astype(np.int64))


# ----------------------------------------------------------------------------------------------------------------- pooling
def _sd(gate_w, gate_b):
    return {"g.gate_fc.weight": gate_w.double().view(1, -1), "g.gate_fc.bias": gate_b.double().view(1)}


def pool_reference(x, gate_w=None, gate_b=None):
    """oracle.multi_scale_pool in double: rows [scale 1 | scale 2 | scale 4], gated by the softmax over the scales present"""
    if gate_w is None:
        return O.multi_scale_pool(None, None, x.double())
    return O.multi_scale_pool(_sd(gate_w, gate_b), "g", x.double())


def multiscale_gate_model(x, gate_w, gate_b, el=BF16):
    """float64 output, its bound per element (the module docstring derives the terms), the float64 gates (B, scales present)"""
    B, k, E = x.shape
    x64 = x.double()
    scales = [s for s in (1, 2, 4) if k >= s]
    ncg = -(-E // 256)
    pooled = [x64[:, :k // s * s].view(B, k // s, s, E).mean(2) for s in scales]
    pabs = [x64[:, :k // s * s].abs().view(B, k // s, s, E).mean(2) for s in scales]
    if gate_w is None:
        w = torch.ones(B, len(scales), dtype=f64)
        ew = torch.zeros_like(w)
    else:
        gw = gate_w.double()
        dot = torch.stack([pl.mean(1) @ gw for pl in pooled], 1)                              # (B, ns)
        A = torch.stack([pa.mean(1) @ gw.abs() for pa in pabs], 1)
        w, ew = _softmax_err(dot + gate_b.double(), dot, len(scales), (k + 2 + 256 + 16 * ncg) * u * A)
    out = torch.cat([pl * w[:, i, None, None] for i, pl in enumerate(pooled)], 1)
    pre = torch.cat([(s - 1) * u * pa * w[:, i, None, None] + pl.abs() * w[:, i, None, None] * (ew[:, i, None, None] + u)
                     for i, (s, pl, pa) in enumerate(zip(scales, pooled, pabs))], 1)
    return dict(out=out, bound=stored(out, pre, el), gates=w)


POOL_FAULTS = ("tail_dropped", "tail_pair_missing")
GATE_FAULTS = ("mean_over_k", "three_gates", "tail_in_every_slab")


def multiscale_gate_emulate(x, gate_w, gate_b, el=BF16, fault=None):
    """the two kernels in torch fp32 -> (output rounded once, fp32 gates or None).  Column sums over the first floor(k / s) s tokens,
    divided, times gate_w, summed; + gate_b; exp(l - max) / sum over the scales present; rows (sum of s tokens) (gate / s).
    Faults: the rows of the tokens past the last group of four left unwritten (NaN); of those only the scale-2 row of a trailing pair;
    the column sums divided by k; the softmax over three logits when a scale is absent (its logit is the bias); the (<= 3) tokens
    past the last group of four added by all 16 token slabs instead of by slab 0."""
    B, k, E = x.shape
    xf = x.float()
    lim = {1: k, 2: k // 2 * 2, 4: k // 4 * 4}
    scales = [s for s in (1, 2, 4) if k >= s]
    gates = None
    if gate_w is not None:
        logits = []
        for s in (1, 2, 4):
            if k < s and fault != "three_gates":
                continue
            c = xf[:, :lim[s]].sum(1)
            if fault == "tail_in_every_slab" and s < 4:
                c = c + 15 * xf[:, lim[4]:lim[s]].sum(1)
            div = float(k if fault == "mean_over_k" else max(lim[s], 1))
            logits.append((c / div * gate_w.float()).sum(-1) + gate_b.float())
        a = torch.stack(logits, 1)
        p = torch.exp(a - a.max(1, keepdim=True).values)
        gates = (p / p.sum(1, keepdim=True))[:, :len(scales)]
    rows = []
    for i, s in enumerate(scales):
        f = (gates[:, i, None, None] if gates is not None else 1.0) / float(s)
        rows.append(xf[:, :lim[s]].view(B, k // s, s, E).sum(2) * f)
    out = el.rnd(torch.cat(rows, 1))
    g4 = k // 4
    if fault == "tail_dropped":
        out[:, 4 * g4:k] = math.nan
    if fault in ("tail_dropped", "tail_pair_missing") and k // 2 > 2 * g4:
        out[:, k + 2 * g4] = math.nan
    return out, gates


# ------------------------------------------------------------------------------------------------------------ preprocessing
PRE_FAULTS = ("rank_off_by_one", "lerp_wrong_end", "box_upper_inclusive", "round_not_int", "taps_normalised", "align_corners_false",
              "filter_skipped")
OUT_ELEMS = {torch.float32: Elem("f32", f32, u, 2.0 ** -150, lambda t: t.float().double(), None), torch.bfloat16: BF16, torch.float16: F16}
PP_MAX_TAIL = 16


def percentile_restate(values, q, fault=None):
    """np.percentile(method="linear") at index level: virtual index q / 100 (n - 1), neighbours floor and floor + 1 (clamped),
    numpy's lerp (from the far end for t >= 0.5).  Faults: both ranks one too high; the interpolation weight taken from the wrong end."""
    s = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    n = s.size
    pos = q / 100.0 * (n - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, n - 1)
    t = pos - lo
    if fault == "rank_off_by_one":
        lo, hi = min(lo + 1, n - 1), min(hi + 1, n - 1)
    if fault == "lerp_wrong_end":
        t = 1.0 - t
    a, b = s[lo], s[hi]
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def _taps(sigma, fault=None):
    """MONAI's gaussian_1d(sigma, truncated=4, approx="erf", normalize=False) in float32, which is its definition; sigma = 0 gives
    {0, 1, 0} (t = inf)"""
    if not math.isfinite(float(sigma)):                  # an output extent of 0 (only a faulted geometry gets there)
        return PP_MAX_TAIL + 1, None
    tail = int(max(float(sigma) * 4.0, 0.5) + 0.5)
    x = torch.arange(-tail, tail + 1, dtype=f32)
    t = torch.tensor(0.70710678, dtype=f32) / sigma.abs()
    k = (0.5 * (torch.erf(t * (x + 0.5)) - torch.erf(t * (x - 0.5)))).clamp_min(0)
    if fault == "taps_normalised":
        k = k / k.sum()
    return tail, k


def _conv_axis(x, k, tail, ax):
    """zero-padded correlation of x with the 2 tail + 1 taps k along axis ax, in x's dtype, tap by tap"""
    out = torch.zeros_like(x)
    n = x.shape[ax]
    for j in range(-tail, tail + 1):
        lo, hi = max(0, -j), min(n, n - j)
        if lo < hi:
            out.narrow(ax, lo, hi - lo).add_(k[j + tail].to(x.dtype) * x.narrow(ax, lo + j, hi - lo))
    return out


def _lerp_axis(xs, n_in, n_out, ax, fault=None):
    """align_corners linear interpolation of every tensor of xs along ax: the source index in float32 as torch computes it (step
    (in - 1) / (out - 1) in float32, 0 for out = 1), the weights in the tensors' dtype"""
    o = torch.arange(n_out, dtype=f32)
    if fault == "align_corners_false":
        src = ((o + 0.5) * (torch.tensor(float(n_in), dtype=f32) / torch.tensor(float(n_out), dtype=f32)) - 0.5).clamp_min(0)
    else:
        step = torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(n_out - 1), dtype=f32) if n_out > 1 else torch.tensor(0.0)
        src = step * o
    i0 = src.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(f32)
    shape = [1, 1, 1]
    shape[ax] = n_out
    outs = []
    for x in xs:
        w1 = l1.to(x.dtype).view(shape)
        outs.append((1 - w1) * x.index_select(ax, i0) + w1 * x.index_select(ax, i1))
    return outs


def _preprocess(vol_hwd, T, pad, rot90_k=0, work=f64, fault=None):
    """u2Transform.adaptive_resize on the (H, W, D) array in the working layout [d][h][w] -> dict(status, lo, hi, out_size, a_min,
    a_max, out (pad, T, T) in `work`, err, crop).  work = float64: the reference, with `err` the bound in front of the store;
    work = float32: the emulation (every product and sum rounded to fp32).  Percentiles by np.percentile on the fp32 voxels, the box
    by nonzero, the geometry by the Python expressions of u2Transform.py:75-98, the taps in float32, the zero-padded separable
    convolution and the interpolation in `work`."""
    v = np.ascontiguousarray(np.asarray(vol_hwd, dtype=np.float64).transpose(2, 0, 1))
    if fault in ("rank_off_by_one", "lerp_wrong_end"):
        a_min, a_max = percentile_restate(v, 0.5, fault), percentile_restate(v, 99.5, fault)
    else:
        a_min, a_max = float(np.percentile(v, 0.5)), float(np.percentile(v, 99.5))
    y = v - a_min if a_max - a_min == 0.0 else np.clip((v - a_min) / (a_max - a_min), 0.0, 1.0)
    res = dict(status=0, a_min=np.float32(a_min), a_max=np.float32(a_max), lo=None, hi=None, out_size=None,
               out=torch.zeros(pad, T, T, dtype=work), err=torch.zeros(pad, T, T, dtype=f64), crop=None)
    y32 = y.astype(np.float32)                              # MONAI returns float32; the foreground is decided on it
    nz = np.nonzero(y32 > 0)
    if nz[0].size == 0:
        res["status"] = 1
        return res
    lo = [int(i.min()) for i in nz]
    hi = [int(i.max()) + (0 if fault == "box_upper_inclusive" else 1) for i in nz]
    res["lo"], res["hi"] = lo, hi
    if min(h - l for l, h in zip(lo, hi)) <= 0:
        res["status"] = 1
        return res
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    crop64 = np.ascontiguousarray(np.rot90(y[sl], rot90_k, axes=(1, 2)))
    crop32 = np.ascontiguousarray(np.rot90(y32[sl], rot90_k, axes=(1, 2)))
    x = torch.from_numpy(crop64 if work == f64 else crop32.copy()).to(work)
    a = x.abs().double()                                     # magnitudes carried along for the bound
    e = u * a                                                # one fp32 rounding of the scaled value
    d, h, w = x.shape
    ratio = min([T / (h, w)[i] for i in range(2)])
    conv = round if fault == "round_not_int" else int
    out_sz = [d if pad >= d else pad, conv(h * ratio), conv(w * ratio)]
    res["out_size"], res["crop"] = out_sz, x.clone()
    in_sz = [d, h, w]
    if any(o < i for o, i in zip(out_sz, in_sz)):
        factors = torch.tensor([float(i) for i in in_sz], dtype=f32) / torch.tensor([float(o) for o in out_sz], dtype=f32)
        sigmas = torch.maximum(torch.zeros(3), (factors - 1) / 2)
        filt = []
        for ax in range(3):
            tail, k = _taps(sigmas[ax], fault)
            if tail > PP_MAX_TAIL:
                res["status"] = 2
                return res
            filt.append((tail, k))
        skipped = False
        for ax in (2, 1, 0):
            tail, k = filt[ax]
            if fault == "filter_skipped" and float(sigmas[ax]) > 0 and not skipped:
                skipped = True
                continue
            k64 = k.double()
            e = _conv_axis(e, k64, tail, ax) + (2 * tail + 1) * u * _conv_axis(a, k64, tail, ax)
            a = _conv_axis(a, k64, tail, ax)
            x = _conv_axis(x, k, tail, ax)
    for ax in (2, 1, 0):
        x, = _lerp_axis([x], in_sz[ax], out_sz[ax], ax, fault)
        a, e = _lerp_axis([a, e], in_sz[ax], out_sz[ax], ax, fault)
    e = e + 7 * u * a
    od, oh, ow = [min(o, lim) for o, lim in zip(out_sz, (pad, T, T))]
    res["out"][:od, :oh, :ow] = x[:od, :oh, :ow]
    res["err"][:od, :oh, :ow] = e[:od, :oh, :ow]
    return res


def preprocess_reference(vol_hwd, T, pad, rot90_k=0):
    return _preprocess(vol_hwd, T, pad, rot90_k, f64)


def preprocess_model(vol_hwd, T, pad, rot90_k=0, out_dtype=torch.float32):
    """the float64 reference with its bound per voxel: u |y| for the one fp32 rounding of the scaled value, carried through the
    filter and the interpolation (their weights are non-negative); (2 tail + 1) u sum|tap x| per filtered axis; 7 u times the
    interpolated magnitude for the seven roundings of the interpolation; one rounding of the output type (`stored`).  Outside
    the resized block reference and bound are exactly 0."""
    r = preprocess_reference(vol_hwd, T, pad, rot90_k)
    el = OUT_ELEMS[out_dtype]
    pre = r["err"]
    bound = torch.where(r["out"] != 0, stored(r["out"], pre, el), pre) if r["status"] == 0 else pre
    r["bound"] = bound if r["status"] == 0 else torch.zeros_like(pre)
    return r


def preprocess_emulate(vol_hwd, T, pad, rot90_k=0, out_dtype=torch.float32, fault=None):
    """the ten kernels in torch fp32 (percentiles and scaling in double, as the kernels do), rounded once to the output type"""
    r = _preprocess(vol_hwd, T, pad, rot90_k, f32, fault)
    r["out"] = r["out"].to(out_dtype)
    return r


def preprocess_info_equal(got, want):
    """status, box, output size and both percentiles (as float32) are exact; without a foreground only status and percentiles exist"""
    if got["status"] != want["status"] or got["a_min"] != want["a_min"] or got["a_max"] != want["a_max"]:
        return False
    if want["status"] == 1:
        return True
    return got["lo"] == want["lo"] and got["hi"] == want["hi"] and got["out_size"] == want["out_size"]


# ===================================================================================================================== tests
@pytest.mark.parametrize("case", K.IM2COL_CASES)
def test_im2col_restatement_is_the_einops_permutation(case):
    nchunk, dims, patch = case
    for el in (BF16, F16):
        for dt in K.VOXEL_DTYPES:
            for fill in ("code", "mod"):
                vol = K.im2col_voxels(nchunk, dims, dt, fill)
                want = im2col_reference(vol, patch, el)
                assert want.shape == (nchunk, math.prod(dims) // math.prod(patch), math.prod(patch))
                assert torch.equal(im2col_restate(vol, patch, el), want)
    vol = K.im2col_voxels(nchunk, dims, torch.float32, "code")           # the code names the voxel: token 1, feature 0 is (0, 0, 0, p3)
    assert im2col_reference(vol, patch, Elem("f32", f32, 0, 0, None, None))[0, 1, 0].item() == 1 + patch[2]


@pytest.mark.parametrize("fault", IM2COL_FAULTS)
def test_im2col_faults_are_seen(fault):
    seen = []
    for nchunk, dims, patch in K.IM2COL_CASES:
        for fill in ("code", "mod"):
            vol = K.im2col_voxels(nchunk, dims, torch.bfloat16, fill)
            seen.append(not torch.equal(im2col_restate(vol, patch, fault=fault), im2col_reference(vol, patch)))
    assert any(seen), fault
    if fault == "p23_swapped":       # the production patch alone (p2 = p3 = 16) cannot see it: what the old single shape missed
        assert not seen[2] and not seen[3]


@pytest.mark.parametrize("B,n,k,E", K.GATHER_CASES + [K.GATHER_BIG])
def test_gather_restatement_clamps(B, n, k, E):
    if (B, n, k, E) == K.GATHER_BIG:
        assert 1.0 < B * k * E // 8 / (8192 * 256) < 1.01           # a second trip for the first 2048 threads only
        E = 8                         # the same indices, narrow rows: the host side of the big case is its index arithmetic
    x, idx = K.gather_inputs(B, n, k, E)
    assert int(idx.min()) < 0 and int(idx.max()) >= n
    assert torch.equal(gather_restate(x, idx), gather_reference(x, idx))
    assert not torch.equal(gather_restate(x, idx, "no_clamp"), gather_reference(x, idx))


@pytest.mark.parametrize("nb,n,dst_bs", K.FILL_CASES + [K.FILL_BIG])
def test_fill_rows_restatement(nb, n, dst_bs):
    if (nb, n, dst_bs) == K.FILL_BIG:
        assert nb * n > 4096 * 256 >= nb * n - 256
    src = torch.arange(1, n + 1, dtype=torch.int32).to(torch.int16)
    fill = torch.full(((nb - 1) * dst_bs + n + 64,), 0x7FC1, dtype=torch.int16)
    want = fill_reference(src, nb, n, dst_bs, fill)
    assert torch.equal(fill_restate(src, nb, n, dst_bs, fill), want)
    assert int((want == 0x7FC1).sum()) >= 64 + (nb - 1) * (dst_bs - n)


def _score_tables(el):
    for rows, E, with_bias in K.SCORE_CASES:
        for kind in K.SCORE_KINDS:
            yield (rows, E, with_bias, kind), K.score_inputs(rows, E, with_bias, kind, el.dtype)


@pytest.mark.parametrize("el", [BF16, F16], ids=["bf16", "f16"])
def test_score_emulation_is_exact_or_inside_the_bound(el):
    """dyadic: bit-equal to integer arithmetic and to math.fsum; hard data: inside the bound, bit-equal away from boundaries, at most
    1 % excused; the N(0, 1) cases excuse none"""
    worst_r, n_hard, excused = 0.0, 0, {"normal": 0, "cancel": 0}
    for (rows, E, with_bias, kind), inp in _score_tables(el):
        m = score_model(**inp)
        got = score_emulate(**inp)
        if kind == "dyadic":
            assert torch.equal(got.view(torch.int32), m["want"].view(torch.int32))
            assert torch.equal(m["want"], score_model(inp["x"], inp["w"], inp["bias"])["want"]), "integer arithmetic against fsum"
            continue
        r, ex = score_check(got, m)
        worst_r, n_hard = max(worst_r, r), n_hard + rows
        excused[kind] += ex
        if kind == "cancel" and E >= 504:
            assert float((m["ref"].abs() / m["mag"]).max()) < 2.0 ** -4, "the rows cancel"
    assert excused["normal"] == 0, excused
    assert excused["cancel"] <= EXCUSED_SHARE * n_hard, (excused, n_hard)
    assert 0.25 < worst_r <= 1.0
    print(f"score_gemv {el.name}: emulated error / bound {worst_r:.3f}, excused {excused} of {n_hard}")


@pytest.mark.parametrize("fault", SCORE_FAULTS)
def test_score_faults_are_seen(fault):
    seen = False
    for (rows, E, with_bias, kind), inp in _score_tables(BF16):
        m = score_model(**inp)
        got = score_emulate(**inp, fault=fault)
        try:
            score_check(got, m)
        except AssertionError:
            seen = True
            break
    assert seen, fault


@pytest.mark.parametrize("n", K.TOPK_NS)
def test_topk_restatement_is_the_canonical_order(n):
    for mix in range(len(K.TOPK_MIXES)):
        s = K.topk_scores(n, mix)
        for k in K.ks_of(n):
            want = O.canonical_topk(s, k)
            assert want.shape == (K.TOPK_B, k)
            assert torch.equal(topk_restate(s, k), want), (n, mix, k)
    s = K.topk_scores(n, 2)                        # the canonical rule on the NaN row, spelled out
    nan = torch.isnan(s[2]).nonzero().flatten()
    assert torch.equal(O.canonical_topk(s, n)[2, :nan.numel()], nan), "every NaN first, by ascending index"
    if n >= 63:
        bits = s[2].view(torch.int32)
        assert (bits[nan] < 0).any() and (bits[nan] > 0).any(), "NaNs of both signs"


@pytest.mark.parametrize("fault", TOPK_FAULTS)
def test_topk_faults_are_seen(fault):
    seen = {}
    for n in K.TOPK_NS:
        for mix, kinds in enumerate(K.TOPK_MIXES):
            s = K.topk_scores(n, mix)
            got, want = topk_restate(s, n, fault), O.canonical_topk(s, n)
            for r, kind in enumerate(kinds):
                if not torch.equal(got[r], want[r]):
                    seen[kind] = seen.get(kind, 0) + 1
    assert seen, fault
    expect = {"ties_descending": "equal", "neg_zero_below": "zeros", "pad_is_zero_key": "negative", "neg_nan_last": "nan"}[fault]
    assert expect in seen, (fault, seen)
    if fault in ("neg_zero_below", "neg_nan_last"):
        assert set(seen) <= {"zeros", "denormal", "nan"}, seen


def test_chain_is_decided_and_restated():
    """score -> top-k -> gather on the chain case equals oracle.token_selection, and its order is decided: no two of the exact
    scores that meet inside the top k or at the cut come within two fp32 ulps of each other (sums of 520 products of 8-bit significands
    have so few bits that about 2 % of them ARE midpoints between two fp32 values; score_model excuses those)"""
    c = K.CHAIN
    x, w, b = K.chain_inputs()
    sd = {"s.score_net.weight": w.double(), "s.score_net.bias": b.double()}
    tok, idx = O.token_selection(sd, "s", x.double(), c["k"])
    flat = x.reshape(c["B"], c["T"] * c["N"], c["E"])
    m = score_model(flat.reshape(-1, c["E"]), w.reshape(-1), b)
    s = score_emulate(flat.reshape(-1, c["E"]), w.reshape(-1), b).view(c["B"], -1)
    assert torch.equal(s, m["want"].view(c["B"], -1))
    got_idx = topk_restate(s, c["k"])
    assert torch.equal(got_idx, idx)
    assert torch.equal(gather_restate(flat, got_idx).double(), tok)
    top = torch.sort(s, 1, descending=True).values[:, :c["k"] + 1]
    gap = (top[:, :-1].double() - top[:, 1:].double())
    assert (gap > 2 * ulp32(top[:, :-1].double())).all(), "neighbours in the top k + 1 are more than two ulps apart: no rounding moves a token"


def _fixed_cases():
    return K.POOL_FIXED_CASES + [K.POOL_TAIL_BIG]


@pytest.mark.parametrize("el", [BF16, F16], ids=["bf16", "f16"])
def test_fixed_pooling_of_small_integers_is_exact(el):
    for B, k, E in _fixed_cases():
        inp = K.pool_inputs(B, k, E, True, dtype=el.dtype)
        want = pool_reference(inp["x"])
        assert want.shape == (B, k + k // 2 + k // 4, E)
        assert torch.equal(el.rnd(want), want), "every mean of 1, 2 or 4 integers up to 15 is exact in the element type"
        got, _ = multiscale_gate_emulate(inp["x"], None, None, el)
        assert torch.equal(got, want), (B, k, E)


def test_pooling_loops_take_their_second_trip():
    B, k, E = K.POOL_TAIL_BIG
    blocks = -(-max(k // 4, 1) * (E // 8) // 256)                       # the grid follows the groups of four tokens
    assert (k % 4 + (k // 2 - 2 * (k // 4))) * (E // 8) > blocks * 256   # 4 tail rows x 1024 column groups on 4 workgroups
    B, k, E = K.POOL_MAIN_BIG
    assert (k // 4) * (E // 8) > 2048 * 256 and k % 4 == 0


def _pool_ratio(case, gated, el, fault=None):
    B, k, E = case
    inp = K.pool_inputs(B, k, E, False, gated, el.dtype)
    m = multiscale_gate_model(inp["x"], inp["gate_w"], inp["gate_b"], el)
    ref = pool_reference(inp["x"], inp["gate_w"], inp["gate_b"])
    assert torch.allclose(m["out"], ref, rtol=1e-12, atol=1e-300), "the model's reference is the oracle in double"
    got, gates = multiscale_gate_emulate(inp["x"], inp["gate_w"], inp["gate_b"], el, fault)
    if gates is not None and fault is None:
        assert gates.shape[1] == 1 + (k >= 2) + (k >= 4)
        assert ((gates.double().sum(1) - 1).abs() <= 3 * u).all(), "the gates of a batch element sum to 1 within 3 u"
    return ratio(got, m["out"], m["bound"])


@pytest.mark.parametrize("el", [BF16, F16], ids=["bf16", "f16"])
def test_pooling_emulation_stays_inside_the_model(el):
    fixed = max(_pool_ratio(c, False, el) for c in _fixed_cases())
    gated = max(_pool_ratio(c, True, el) for c in K.POOL_GATED_CASES)
    print(f"multiscale_pool {el.name}: emulated error / bound {fixed:.3f} fixed, {gated:.3f} gated")
    assert 0.5 < fixed <= 1.0 and 0.5 < gated <= 1.0, (fixed, gated)


@pytest.mark.parametrize("fault", POOL_FAULTS + GATE_FAULTS)
def test_pooling_faults_are_seen(fault):
    gated = fault in GATE_FAULTS
    cases = [c for c in (K.POOL_GATED_CASES if gated else K.POOL_FIXED_CASES) if c[2] <= 512]
    seen = [c for c in cases if _pool_ratio(c, gated, BF16, fault) > 1.0]
    assert seen, fault
    ks = {c[1] for c in seen}
    if fault == "three_gates":
        assert ks <= {1, 2, 3}, ks
    if fault in ("tail_dropped", "tail_in_every_slab"):
        assert all(k % 4 for k in ks), ks
    if fault == "tail_pair_missing":
        assert all(k % 4 >= 2 for k in ks), ks
    if fault == "mean_over_k":
        assert all(k % 2 or k % 4 for k in ks), ks


# ------------------------------------------------------------------------------------------------------------ preprocessing
def _pre_args(c):
    return c["vol"], c["T"], c["pad"], c["rot90_k"]


@pytest.mark.parametrize("name", sorted(K.PREPROCESS_CASES))
def test_preprocess_emulation_stays_inside_the_model(name):
    c = K.PREPROCESS_CASES[name]
    for dt in c["dtypes"]:
        m = preprocess_model(*_pre_args(c), dt)
        got = preprocess_emulate(*_pre_args(c), dt)
        assert preprocess_info_equal(got, m), name
        assert ratio(got["out"], m["out"], m["bound"]) <= 1.0, name
        if m["status"] == 0:
            od, oh, ow = m["out_size"]
            blk = torch.zeros_like(m["out"], dtype=torch.bool)
            blk[:od, :oh, :ow] = True
            assert (m["out"][~blk] == 0).all() and (m["bound"][~blk] == 0).all()
    for q in (0.5, 99.5):
        assert percentile_restate(c["vol"], q) == np.percentile(c["vol"], q), "the restated ranks and lerp are numpy's"


def test_preprocess_cases_reach_what_they_are_named_for():
    R = {n: preprocess_reference(*_pre_args(c)) for n, c in K.PREPROCESS_CASES.items()}
    assert R["pct_n1"]["status"] == 1 and R["box_empty"]["status"] == 1 and R["geo_too_wide"]["status"] == 2
    assert all(r["status"] == 0 for n, r in R.items() if n not in ("pct_n1", "box_empty", "geo_too_wide"))
    assert list(R["pct_n2"]["crop"].shape) == [1, 1, 1] and R["pct_n2"]["out_size"] == [1, 8, 8]
    low = K.PREPROCESS_CASES["pct_low10"]["vol"].astype(np.float32).view(np.uint32)
    assert len(set((low >> 10).reshape(-1).tolist())) == 1 and len(set(low.reshape(-1).tolist())) == 1000
    s = np.sort(K.PREPROCESS_CASES["pct_dup90"]["vol"].reshape(-1))
    assert s[int(0.995 * 4095) - 1] == s[int(0.995 * 4095) + 2] == 12 and s[int(0.005 * 4095) - 1] == s[int(0.005 * 4095) + 2] == -3
    z = K.PREPROCESS_CASES["pct_zeros"]["vol"]
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any() and (z < 0).any()
    for n, pos in (("box_first", [0, 0, 0]), ("box_last", [4, 5, 8]), ("box_inside", [3, 2, 5])):
        assert R[n]["lo"] == pos and R[n]["hi"] == [p + 1 for p in pos] and R[n]["a_min"] == R[n]["a_max"]
    assert R["box_faces"]["lo"] == [0, 0, 0] and R["box_faces"]["hi"] == [5, 6, 9]
    g = R["geo_exact"]
    assert list(g["crop"].shape) == [3, 8, 8] and g["out_size"] == [3, 8, 8]
    assert torch.equal(g["out"][:3], g["crop"]), "a crop of the target size passes through unchanged"
    for dt in (torch.bfloat16, torch.float16):          # and its two roundings (fp32, then the output type) equal the one
        assert torch.equal(g["crop"].float().to(dt), g["crop"].to(dt))
    assert R["geo_depth1"]["crop"].shape[0] == 1 and 1 in R["geo_plane1"]["crop"].shape[1:]
    assert R["geo_tall_rot1"]["out_size"] == R["geo_tall_rot3"]["out_size"] != R["geo_wide_rot1"]["out_size"]
    assert R["geo_depth_pad"]["out_size"][0] == 32 == R["geo_depth_pad"]["crop"].shape[0]
    assert R["geo_depth_pad1"]["out_size"][0] == 32 and R["geo_depth_pad1"]["crop"].shape[0] == 33
    assert R["geo_depth_pad1"]["out_size"][1] > R["geo_depth_pad1"]["crop"].shape[1], "an upsampled axis next to the downsampled depth"
    assert 28 / 3 > 9.25 and list(R["geo_too_wide"]["crop"].shape)[1] == 28


@pytest.mark.parametrize("fault", PRE_FAULTS)
def test_preprocess_faults_are_seen(fault):
    seen = []
    for name, c in K.PREPROCESS_CASES.items():
        m = preprocess_model(*_pre_args(c))
        got = preprocess_emulate(*_pre_args(c), fault=fault)
        if not preprocess_info_equal(got, m) or ratio(got["out"], m["out"], m["bound"]) > 1.0:
            seen.append(name)
    assert seen, fault
    print(fault, "seen by", seen)
