"""Case tables and input generators of the front end and token selection kernels (csrc/vision.hip: im2col_patches, fill_rows;
csrc/select.hip: score_gemv, topk_sorted, gather_rows, multiscale_pool with dmtp_gate_partial; csrc/preprocess.hip), shared by
tests/test_front_end_bounds_host.py (emulations, bounds, planted faults) and tests/test_gpu_front_end_bounds.py (the kernels).
Every input is generated on the CPU from a fixed seed; nothing here touches a GPU."""
import numpy as np
import torch

from test_decoder_train_bounds_host import _gen

# ---- im2col: chunks, (D, H, W), patch (p1, p2, p3); all extents and all patch sizes distinct
IM2COL_CASES = [(2, (8, 6, 16), (4, 3, 8)),          # distinct everything, small: 4 cells of 12 rows x 2 groups
                (1, (8, 32, 48), (4, 16, 16)),       # the production patch: 384 row groups per cell (two trips of the staging loop)
                (3, (4, 2, 264), (2, 1, 8))]         # 33 groups per row, one row per patch plane, 66 groups per cell (< 256)
VOXEL_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
VOL_CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}

# ---- gather_rows: B, n, k, E; the last has 2 x 1025 x 1024 = 1.0005 x 8192 x 256 work items
GATHER_CASES = [(3, 7, k, E) for E in (8, 264, 4096) for k in (1, 7, 20)]
GATHER_BIG = (2, 7, 1025, 8192)

# ---- fill_rows: nb, n, dst_bs; the last has 3 x 349531 = 1048593 elements, 17 more than 4096 x 256
FILL_CASES = [(nb, n, n + gap) for nb in (1, 3) for n in (1, 7, 4096) for gap in (0, 5)]
FILL_BIG = (3, 349531, 349536)

# ---- score_gemv: rows, E, with bias
SCORE_CASES = [(rows, E, bias) for rows in (1, 3, 4, 5, 9) for E in (8, 504, 512, 520, 4096) for bias in (True, False)]
SCORE_KINDS = ("dyadic", "normal", "cancel")

# ---- topk_sorted: B = 3 rows per mix, three mixes of row kinds per n
TOPK_B = 3
TOPK_NS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4097, 8191, 8192)
TOPK_MIXES = (("equal", "four", "ascending"), ("descending", "zeros", "inf"), ("denormal", "negative", "nan"))
CHAIN = dict(B=2, T=8, N=33, E=520, k=100)

# ---- multiscale_pool: fixed (no gates) B, k, E; gated B, k, E
POOL_KS = tuple(range(1, 10)) + (15, 16, 17, 30, 31, 64)
POOL_FIXED_CASES = [(2, k, E) for E in (8, 264, 512) for k in POOL_KS]
POOL_TAIL_BIG = (2, 3, 8192)            # 3 x 1024 tail items: a second trip of the tail loop (its grid is one workgroup)
POOL_MAIN_BIG = (1, 4100, 4096)         # 1025 x 512 items = 1.001 x 2048 x 256: a second trip of the main loop
POOL_GATED_KS = (1, 2, 3, 4, 5, 7, 17, 64, 130, 260)
POOL_GATED_CASES = [(2, k, E) for E in (264, 512, 8192) for k in POOL_GATED_KS]


def ks_of(n):
    return sorted({1, max(1, n // 2), n})


# ------------------------------------------------------------------------------------------------------------------ im2col
def im2col_voxels(nchunk, dims, dtype, fill):
    """(nchunk, D, H, W) voxels of `dtype`.  fill "code": the integer 1 + ((chunk D + d) H + h) W + w, which names the voxel
    (rounded to a 16-bit voxel type by torch: exact below 257 / 2049, order-preserving above); fill "mod": that integer mod 509
    (a prime) minus 254, exact in every type here, so that a voxel moved by anything but a multiple of 509 shows in every bit."""
    D, H, W = dims
    lin = torch.arange(nchunk * D * H * W, dtype=torch.int64).view(nchunk, D, H, W)
    v = (lin + 1) if fill == "code" else (lin % 509 - 254)
    return v.to(torch.float32).to(dtype)


# ------------------------------------------------------------------------------------------------------------------ gather
def gather_inputs(B, n, k, E, dtype=torch.bfloat16):
    """x (B, n, E) N(0, 1); idx (B, k) int64 in [0, n) with duplicates (k = 20 > n forces them), and out of range: -1, n, 2^40, -2^40
    spread over the batch (k = 1 has room for one per batch entry)."""
    g = _gen(31, B, n, k, E)
    x = torch.randn(B, n, E, generator=g).to(dtype)
    idx = torch.randint(0, n, (B, k), generator=g)
    wild = [-1, n, 2 ** 40, -2 ** 40]
    flat = idx.view(-1)
    for j, w in enumerate(wild):
        flat[(j * 5) % flat.numel()] = w
    if k > 2:
        idx[:, k - 1] = idx[:, 0].clamp(0, n - 1)     # one certain duplicate per batch entry
    return x, idx


# ------------------------------------------------------------------------------------------------------------------- score
def score_inputs(rows, E, with_bias, kind, dtype=torch.bfloat16):
    """x (rows, E), w (E), bias (1) or None.
    dyadic: m 2^-6 with integer |m| <= 255 (8 significant bits: exact in bf16 and f16); also returns the integers.
    normal: N(0, 1) x, N(0, 1 / E) w.
    cancel: w[2 i] = w[2 i + 1]; x[2 i + 1] = -x[2 i] = N(0, 1) min(2^7, 2^23 / E^2) on all but the last 8 columns, which hold N(0, 1):
    the sum of the terms is about E 2^-20 of the sum of their magnitudes without a bias (2^-11 at E = 512, 2^-8 at E = 4096), which keeps the
    first-order error of an fp64 sum, E 2^-53 sum|terms|, near 2^-8 of an fp32 ulp of the score."""
    g = _gen(32, rows, E, int(with_bias), SCORE_KINDS.index(kind))
    if kind == "dyadic":
        mx = torch.randint(-255, 256, (rows, E), generator=g)
        mw = torch.randint(-255, 256, (E,), generator=g)
        mb = torch.randint(-255, 256, (1,), generator=g) if with_bias else None
        f = lambda m: None if m is None else (m.double() / 64).to(dtype)
        return dict(x=f(mx), w=f(mw), bias=f(mb), ints=(mx, mw, mb))
    if kind == "normal":
        x = torch.randn(rows, E, generator=g)
        w = torch.randn(E, generator=g) / E ** 0.5
    else:
        half = torch.randn(rows, E // 2, generator=g) * min(128.0, 2.0 ** 23 / E ** 2)
        x = torch.stack([half, -half], -1).reshape(rows, E)
        x[:, E - 8:] = torch.randn(rows, 8, generator=g)
        w = torch.randn(E // 2, generator=g).repeat_interleave(2) / E ** 0.5
    bias = (torch.randn(1, generator=g) * 0.5).to(dtype) if with_bias else None
    return dict(x=x.to(dtype), w=w.to(dtype), bias=bias, ints=None)


# ------------------------------------------------------------------------------------------------------------------- top-k
def _f32_bits(v):
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v], dtype=torch.int32).view(torch.float32)[0]


POS_NAN, NEG_NAN, NEG_NAN_PAYLOAD = _f32_bits(0x7FC00000), _f32_bits(0xFFC00000), _f32_bits(0xFFFFFFFF)


def topk_row(kind, n, g):
    """one row of n fp32 scores of the named kind"""
    if kind == "equal":
        return torch.full((n,), 1.5)
    if kind == "four":
        return torch.tensor([-2.0, 0.5, 0.5 + 2.0 ** -23, 3.0])[torch.randint(0, 4, (n,), generator=g)]
    if kind == "ascending":
        return torch.arange(n, dtype=torch.float32) * 0.25 - 100
    if kind == "descending":
        return 100 - torch.arange(n, dtype=torch.float32) * 0.25
    if kind == "zeros":           # +0 and -0 tie (ascending index decides), between a few -1 and +1
        r = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        r[torch.rand(n, generator=g) < 0.1] = 1.0
        r[torch.rand(n, generator=g) < 0.1] = -1.0
        return r
    if kind == "inf":
        r = torch.randn(n, generator=g) * 1e30
        r[torch.rand(n, generator=g) < 0.1] = float("inf")
        r[torch.rand(n, generator=g) < 0.1] = -float("inf")
        return r
    if kind == "denormal":        # multiples of 2^-149 of both signs, with ties and zeros of both signs
        m = torch.randint(-40, 41, (n,), generator=g)
        r = (m.double() * 2.0 ** -149).float()
        r[m == 0] = torch.where(torch.rand(int((m == 0).sum()), generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        return r
    if kind == "negative":        # every score far below the key of 0.0; -inf among them
        r = -1e30 * (1 + torch.rand(n, generator=g))
        r[torch.rand(n, generator=g) < 0.05] = -float("inf")
        r[torch.rand(n, generator=g) < 0.05] = -3.4028234663852886e38
        return r
    assert kind == "nan"
    r = torch.randn(n, generator=g)
    u = torch.rand(n, generator=g)
    r[u < 0.06] = POS_NAN
    r[(u >= 0.06) & (u < 0.12)] = NEG_NAN
    r[(u >= 0.12) & (u < 0.15)] = NEG_NAN_PAYLOAD
    r[(u >= 0.15) & (u < 0.2)] = float("inf")
    if n >= 3:
        r[n - 1], r[n // 2] = NEG_NAN, POS_NAN
    return r


def topk_scores(n, mix):
    """(TOPK_B, n) fp32: one row per kind of TOPK_MIXES[mix]"""
    g = _gen(33, n, mix)
    return torch.stack([topk_row(kind, n, g) for kind in TOPK_MIXES[mix]])


def chain_inputs(dtype=torch.bfloat16):
    c = CHAIN
    g = _gen(34, c["B"], c["T"], c["N"], c["E"])
    x = torch.randn(c["B"], c["T"], c["N"], c["E"], generator=g).to(dtype)
    w = (torch.randn(1, c["E"], generator=g) / c["E"] ** 0.5).to(dtype)
    b = (torch.randn(1, generator=g) * 0.5).to(dtype)
    return x, w, b


# ----------------------------------------------------------------------------------------------------------------- pooling
def pool_inputs(B, k, E, integer, gated=False, dtype=torch.bfloat16):
    """x (B, k, E): integers in [-15, 15], or N(0, 1) with a mean of 0.5 on the even batch entries (the token means, and with them the
    gate logits, then differ between the scales by more than rounding noise only through the tokens each scale leaves out);
    gated: gate_w (E) N(0, 4 / E), gate_b (1)."""
    g = _gen(35, B, k, E, int(integer), int(gated))
    if integer:
        x = torch.randint(-15, 16, (B, k, E), generator=g).float()
    else:
        x = torch.randn(B, k, E, generator=g)
        x[0::2] += 0.5
        if k >= 2:
            x[:, k - 1] += 2.0          # the last token: outside scale 2 for odd k, outside scale 4 for k % 4 != 0
    out = dict(x=x.to(dtype), gate_w=None, gate_b=None)
    if gated:
        out["gate_w"] = (torch.randn(E, generator=g) * 2 / E ** 0.5).to(dtype)
        out["gate_b"] = (torch.randn(1, generator=g) * 0.5).to(dtype)
    return out


# ------------------------------------------------------------------------------------------------------------ preprocessing
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _boxed(shape, box, seed, lo=-1000.0):
    """(H, W, D) of fp32 values: background `lo` (the minimum: it scales to exactly 0), the box (h0, h1, w0, w1, d0, d1) filled with
    N(40, 250) rounded to integers, all above the background"""
    rng = np.random.default_rng(seed)
    v = np.full(shape, lo)
    h0, h1, w0, w1, d0, d1 = box
    v[h0:h1, w0:w1, d0:d1] = np.maximum(rng.normal(40, 250, size=(h1 - h0, w1 - w0, d1 - d0)).round(), lo + 1)
    return _f32(v)


def _one_voxel(pos, shape=(6, 9, 5)):
    v = np.full(shape, -5.0)
    v[pos] = 10.0
    return v


def preprocess_cases():
    """name -> dict(vol (H, W, D) float64 of fp32 values, T, pad, rot90_k, dtypes): every volume has at most 32^3 voxels"""
    rng = np.random.default_rng(41)
    low = 1.0 + np.arange(1000) * 2.0 ** -23
    rng.shuffle(low)
    pick = rng.random(4096)
    dup = _f32(np.where(pick < 0.45, -3.0, np.where(pick < 0.9, 12.0, rng.normal(5, 2, 4096).clip(-2, 11))))     # 45 % at each end
    zeros = np.where(rng.random(2048) < 0.5, 0.0, -0.0)
    neg = rng.random(2048) < 0.4
    zeros[neg] = _f32(-rng.random(int(neg.sum())) - 0.25)
    faces = np.full((6, 9, 5), -5.0)
    for h, w, d in [(0, 4, 2), (5, 3, 1), (2, 0, 2), (3, 8, 3), (2, 4, 0), (4, 5, 4)]:
        faces[h, w, d] = 10.0 + h
    f32 = (torch.float32,)
    every = (torch.float32, torch.bfloat16, torch.float16)
    c = {
        # ---- percentiles (radix select)
        "pct_n1": dict(vol=np.full((1, 1, 1), 3.25)),                                # one voxel: degenerate, no foreground
        "pct_n2": dict(vol=np.array([-2.0, 5.5]).reshape(1, 2, 1)),                  # two: a one-voxel crop, in_sz = 1 on every axis
        "pct_n201": dict(vol=_f32(rng.normal(0, 100, 201)).reshape(3, 1, 67)),       # 0.5 / 100 * 200 is 1 up to rounding
        "pct_low10": dict(vol=low.reshape(10, 10, 10)),                              # only pass 2 of the select separates the values
        "pct_dup90": dict(vol=dup.reshape(16, 16, 16)),                              # both neighbours of a rank are the same value
        "pct_zeros": dict(vol=zeros.reshape(16, 16, 8)),                             # +0 / -0 mixed with negatives
        # ---- box
        "box_first": dict(vol=_one_voxel((0, 0, 0))),                                # one voxel above a constant: a_max == a_min,
        "box_last": dict(vol=_one_voxel((5, 8, 4))),                                 # the degenerate branch (x - a_min, unclipped)
        "box_inside": dict(vol=_one_voxel((2, 5, 3))),
        "box_faces": dict(vol=faces),                                                # touches all six faces; in-plane downsampling
        "box_empty": dict(vol=np.full((4, 4, 4), 7.0)),                              # status 1
        # ---- geometry
        "geo_exact": dict(vol=_boxed((10, 11, 5), (1, 9, 2, 10, 1, 4), 51), dtypes=every),          # the crop is T x T, depth 3
        "geo_depth1": dict(vol=_boxed((12, 10, 3), (3, 9, 2, 7, 1, 2), 52)),                        # in_sz = 1 on depth
        "geo_plane1": dict(vol=_boxed((5, 10, 6), (2, 3, 1, 7, 1, 5), 53)),                         # in_sz = 1 on an in-plane axis
        "geo_tall_rot1": dict(vol=_boxed((16, 11, 5), (1, 15, 1, 10, 1, 4), 54), rot90_k=1),        # H > W
        "geo_tall_rot3": dict(vol=_boxed((16, 11, 5), (1, 15, 1, 10, 1, 4), 54), rot90_k=3),
        "geo_wide_rot1": dict(vol=_boxed((11, 16, 5), (1, 10, 1, 15, 1, 4), 55), rot90_k=1),        # W > H
        "geo_wide_rot3": dict(vol=_boxed((11, 16, 5), (1, 10, 1, 15, 1, 4), 55), rot90_k=3),
        "geo_depth_pad": dict(vol=_boxed((5, 6, 32), (0, 5, 0, 6, 0, 32), 56), dtypes=every),       # depth == pad: no filter
        "geo_depth_pad1": dict(vol=_boxed((5, 6, 33), (0, 5, 0, 6, 0, 33), 57), dtypes=every),      # depth 33 -> 32 next to 5 x 6 -> 6 x 8
        "geo_too_wide": dict(vol=_boxed((30, 4, 6), (1, 29, 1, 3, 1, 5), 58), T=3),                 # 28 / 3 > 9.25: status 2
    }
    for v in c.values():
        v.setdefault("T", 8)
        v.setdefault("pad", 32)
        v.setdefault("rot90_k", 0)
        v.setdefault("dtypes", f32)
        assert v["vol"].size <= 32 ** 3 and (v["vol"] == _f32(v["vol"])).all()
    return c


PREPROCESS_CASES = preprocess_cases()
