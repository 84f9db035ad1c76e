"""The forward GEMM gate's tables, data and bound: shared by tests/test_gemm_bounds_host.py (CPU: the bound holds an emulation and
rejects 13 planted faults), tests/test_gemm_plan.py (CPU: every descriptor's route is pinned) and tests/test_gpu_gemm_bounds.py (the
kernels of gemm.hip, gemm_bt.hip, gemm_skinny.hip, gemm_rows.hip and the split-K reduce on the MI355X).  A GEMM kernel that is
added or changed adds its products HERE: a descriptor per shape and option set that reaches it, its form's kernel in FORM_KERNEL,
and the route the driver prints for it in tests/test_gemm_plan.py (GEMM_BOUND_ROUTES).

A case is (form, descriptor, data sets).  The descriptor is the "key=value" line of tests/gemm_plan_driver.cpp with three
differences, as tests/test_gpu_ops.py::GEMM_WRITE_CASES has them: c_off counts ELEMENTS of C, `alpha=` may appear (a float; the plan
does not read it), and `nsplit=` implies alpha_lo = ALPHA_LO.  plan_descriptor() gives the driver's form.  Every C has ldc > N, a
nonzero c_off and, for nz = 2, gaps between the batch entries of A, B and C.

Data sets (operands drawn in float32 from a generator seeded by the case, rounded ONCE to the element type):
  ints      integers in [-3, 3], bias and residual too: every product and every fp32 partial sum is an integer below 2^24, so an
            fp32 output must equal the float64 product bit for bit, an element-type output that value rounded once
  normal    A ~ N(0, 1), B ~ N(0, 1) K^-1/2, bias and residual ~ N(0, 1)
  cancel_k  normal, then A[:, h:2h] = A[:, :h] and B[:, h:2h] = -B[:, :h] + N(0, 2^-6) K^-1/2, h = K // 2: the two halves of the K
            sum cancel to about 2^-6 of either, so what is lost in a half (a partial sum rounded to the element type, a K tile read
            twice) is 64 times larger against the result
  cancel_r  normal, then R = -elem(alpha A B^T + bias) + N(0, 2^-6): the residual addition cancels, so a rounding of the
            accumulator before it is 64 times larger against the result

Bound (per element, against the float64 value of the same epilogue on the same rounded operands; U = the element type's unit
roundoff 2^-8 / 2^-11, u = 2^-24, S = |alpha| sum_k |a_k b_k| with alpha_lo in alpha's place below nsplit):
  plain / bias / residual   U |ref| + (K + 8) u S + 4 u (|bias| + |R|);  an fp32 output drops U |ref|
  GELU                      |gelu'(p)| (U |p| + (K + 8) u S) + 3.3e-6 + U |ref|, p the pre-activation, ref = gelu(p) (+ R)
  SwiGLU pair               U |ref| + U |silu(g)| |up| + U (|silu'(g)| |g| |up| + |silu(g)| |up|)
                            + (K + 8) u (|silu'(g)| |up| S_g + |silu(g)| S_up)
(K + 8) u is the first-order worst case of ANY order of K round-to-nearest fp32 additions of exact products (K - 1 additions, each
relative error u on a partial sum bounded by S) plus the epilogue's operations; nothing is fitted.  The third SwiGLU term is what the
pair epilogue's documented contract adds to `elem(silu(gate)) * up`: include/u2tok.h and rows.h (rows_pair_store) round gate AND up
to the element type before silu and the product -- "the values u2tok_gemm_bf16 + u2tok_swiglu_bf16 produce, bit for bit" -- which
moves the result by |d ref / d g| U |g| + |d ref / d up| U |up| to first order.  The two roundings of the pair form are charged at
least what the formats underflow by (integer data put gates at -100): the rounding of silu(g) max(U |silu(g)|, t) with t = 2^-25 for
f16, half the spacing of its subnormals, and 2^-121 for bf16 -- for g < -88.7 e^-g overflows fp32 and silu evaluates to 0, where
|silu(g)| < 89 e^-88.7 < 2^-121; the store max(U |ref|, tiny) with Elem's tiny (2^-25 / 2^-126)."""
import math

import torch

from test_row_fwd_bounds_host import BF16, ELEMS, F16, ratio, worst  # noqa: F401  (the element types of the row kernels' gate)

u = 2.0 ** -24
BIAS_N, BIAS_M, GELU, RES, OUT_F32, B_KTILE, A_KMAJOR, B_KMAJOR, SWIGLU = 1, 2, 4, 8, 16, 64, 128, 256, 512
ALPHA_LO = 0.125 * 1.4426950408889634          # the ViT's softmax scale (head dim 64) times log2 e
GELU_EPS = 3.3e-6                              # kernels.h, GEMM_GELU: |gelu_epi - erf-GELU| before rounding
OPTION_DEFAULTS = dict(gemm_tile=0, gemm_mubuf=1, gemm_splitk=0, gemm_big=0, gemm_big_grid=256, gemm_big_splitk=0,
                       gemm_big_drain=1, gemm_skinny=2, gemm_tail_fused=1)
SCRATCH = 16 << 20                             # split-K scratch of the sliced cases (>= 3 slices of the largest product)
NOT_PLANNED = ("alpha", "nbh", "sAh", "sBh", "sCh")


def parse(desc):
    p = {}
    for kv in desc.split():
        k, v = kv.split("=")
        p[k] = tuple(int(x) for x in v.split(",")) if k == "vt" else float(v) if k == "alpha" else int(v, 0)
    return p


def plan_descriptor(desc):
    """the product as tests/gemm_plan_driver.cpp reads it: c_off in bytes, what the plan does not read dropped"""
    p = parse(desc)
    out = []
    for kv in desc.split():
        k, v = kv.split("=")
        if k in NOT_PLANNED:
            continue
        out.append(f"c_off={int(v) * (4 if p.get('flags', 0) & OUT_F32 else 2)}" if k == "c_off" else kv)
    return " ".join(out)


def options(p):
    return {k: v for k, v in p.items() if k.startswith("gemm_")}


def desc(M, N, K, flags=0, nz=1, **kw):
    """descriptor of a product whose C has ldc > N and c_off > 0 -- 16-byte aligned rows where N allows the vector epilogue, odd ones
    where it does not -- and whose batch entries (nz = 2) lie apart in A, B and C"""
    f32, pair = bool(flags & OUT_F32), bool(flags & SWIGLU)
    Nc = N // 2 if pair else N
    vec = Nc % 8 == 0
    ldc, c_off = (Nc + 8, 8) if vec else (Nc + 5, 3 if not f32 else 4)
    parts = [f"M={M} N={N} K={K}"]
    ta, tb = bool(flags & A_KMAJOR), bool(flags & B_KMAJOR)
    lda, ldb = (M if ta else K), (N if tb else K)
    if nz > 1:
        parts.append(f"nz={nz}")
    parts.append(f"ldc={ldc}")
    if nz > 1:
        parts.append(f"sAb={(K if ta else M) * lda + 16} sBb={(K if tb else N) * ldb + 24} sCb={M * ldc + (40 if vec else 37)}")
    parts.append(f"c_off={c_off}")
    if flags:
        parts.append(f"flags={flags:#x}")
    parts += [f"{k}={v}" for k, v in kw.items()]
    return " ".join(parts)


# ---------------------------------------------------------------------------------------------------------------- the tables
# (form, descriptor, data sets); the FIRST case of a form also runs on the f16 build.  K is swept, M and N cycle through their edges.
def _data(flags, K, staged=True):
    d = ["ints", "normal"]
    if staged and K >= 64 and not flags & SWIGLU:
        d.append("cancel_k")
    if flags & RES and not flags & GELU:
        d.append("cancel_r")
    return tuple(d)


TILE_MN = [(1, 8), (63, 136), (64, 200), (65, 203), (77, 136), (130, 203), (130, 8), (1, 203)]
TILE_K = (8, 56, 64, 72, 128, 136, 192, 200)
TILE_EPI = (0, BIAS_N, OUT_F32, BIAS_N | RES, BIAS_N | GELU, BIAS_N | GELU | RES, BIAS_M | OUT_F32, RES)


def _tile_cases():
    out = []
    for tile in (64, 128):
        for i, K in enumerate(TILE_K):
            M, N = TILE_MN[(i + (3 if tile == 128 else 0)) % 8]
            f = TILE_EPI[i]
            kw = {"alpha": 0.5} if f == BIAS_N else {}      # (a power of two: the integer data stay exact)
            out.append((f"tile{tile}", desc(M, N, K, f, nz=2 if i % 3 == 1 else 1, **kw, gemm_tile=tile), _data(f, K)))
        # B K-major (K % 8 == 0, N % 8 == 0), A | B K-major (M, N % 8 == 0, any K), B K-tile-major (K % 64 == 0)
        out.append((f"tile{tile}_bk", desc(77, 136, 64, B_KMAJOR, alpha=0.5, gemm_tile=tile), _data(0, 64)))
        out.append((f"tile{tile}_bk", desc(130, 200, 136, B_KMAJOR | OUT_F32, nz=2, gemm_tile=tile), _data(0, 136)))
        for j, K in enumerate((64, 77, 131)):
            out.append((f"tile{tile}_abk", desc((64, 136, 200)[j], (200, 8, 136)[j], K, A_KMAJOR | B_KMAJOR | (OUT_F32 if j == 1 else 0),
                                                nz=2 if j == 2 else 1, gemm_tile=tile), _data(0, K)))
        for j, K in enumerate((64, 128, 192)):
            out.append((f"tile{tile}_ktile", desc((65, 130, 77)[j], (136, 200, 8)[j], K, (0, BIAS_N | GELU, BIAS_N | RES)[j], ktile=1,
                                                  gemm_tile=tile), _data((0, 5, 9)[j], K)))
    return out


SPLITK_EPI = (0, BIAS_N, BIAS_N | RES, BIAS_N | GELU, OUT_F32, BIAS_M | RES)


def _splitk_cases():
    out = []
    for tile, (M, N) in ((128, (130, 136)), (64, (77, 520))):
        for n in (2, 3):
            for f in SPLITK_EPI:
                out.append((f"tile{tile}_splitk", desc(M, N, 1160, f, gemm_tile=tile, gemm_splitk=n, scratch=SCRATCH), _data(f, 1160)))
    return out


def _rows_cases():
    out = []
    MN = [(1, 8), (5, 40), (16, 203), (16, 8), (1, 203), (5, 203), (16, 40)]
    epi = (0, BIAS_N | RES, BIAS_N | GELU, OUT_F32 | BIAS_N, RES, BIAS_M, BIAS_N)
    for i, K in enumerate((32, 64, 96, 768, 2048, 768, 2048)):
        M, N = MN[i]
        out.append(("rows16", desc(M, N, K, epi[i]), _data(epi[i], K)))
    for M, I, K in ((5, 16, 64), (16, 48, 768), (1, 16, 2048)):
        out.append(("rows16_pair", desc(M, 2 * I, K, SWIGLU), ("ints", "normal")))
    return out


def _skinny_cases():
    out = []
    epi = (0, BIAS_N, BIAS_N | GELU, OUT_F32 | BIAS_N)
    for i, K in enumerate((1024, 1152, 1280, 1408)):
        for sk in (2, 1):
            out.append(("skinny", desc((65, 200, 256, 200)[i], 2048, K, epi[i], **({} if sk == 2 else {"gemm_skinny": 1})), _data(epi[i], K)))
    out.append(("skinny", desc(256, 2048, 1408, BIAS_N | RES), ("normal", "cancel_r")))
    return out


BIG_FORCED = (20, 21, 22, 24, 26)
BIG_EPI = (0, OUT_F32, BIAS_N, BIAS_N | OUT_F32, BIAS_N | GELU, BIAS_N | RES, RES)


def _big_cases():
    out = []
    for v in BIG_FORCED:
        for K in range(128, 833, 64):        # 2 .. 13 K tiles: every entry and exit of the two- and three-stage loops, chained
            out.append((f"big{v}", desc(512, 384, K, 0, gemm_big=v, gemm_big_grid=2), ("ints",)))
        for K in (192, 448, 832):
            for f in BIG_EPI:
                data = ("normal", "cancel_r") if f & RES else ("normal",)
                out.append((f"big{v}", desc(300, 200, K, f, gemm_big=v, gemm_big_grid=2), data))
        out.append((f"big{v}", desc(300, 200, 448, BIAS_N, nz=2, gemm_big=v, gemm_big_grid=2), ("ints", "normal")))
    for v in (20, 21, 22):
        for n in (2, 3):
            for M, N in ((300, 200), (256, 384)):
                out.append((f"big{v}_sliced", desc(M, N, 832, BIAS_N | RES if n == 3 else 0, gemm_big=v, gemm_big_splitk=n, gemm_big_grid=2,
                                                   scratch=SCRATCH), ("ints", "cancel_k")))
    return out


DRAIN_K = (768, 1152, 1536)


def _drain_cases():
    out = []
    for K in DRAIN_K:
        for f, kw in ((0, {}), (BIAS_N, {}), (0, {"alpha": 0.5}), (BIAS_N | GELU, {})):
            out.append(("drain27", desc(512, 384, K, f, gemm_big=27, gemm_big_grid=2, **kw), ("ints", "normal", "cancel_k")))
    # the heuristic routes with 2 cls rows behind the tiles, in the launch (gemm_tail_fused 1) and in one of their own (0)
    for tf in (1, 0):
        kw = {} if tf else {"gemm_tail_fused": 0}
        out.append(("heuristic_tail", desc(514, 576, 768, 0, gemm_big_grid=2, **kw), ("ints", "normal", "cancel_k")))
        out.append(("heuristic_tail", desc(514, 1152, 768, BIAS_N | GELU, gemm_big_grid=2, **kw), ("ints", "normal")))
    return out


def _pair_cases():
    return [("big21_pair", desc(300, 2 * I, K, SWIGLU), ("ints", "normal")) for K in (128, 192) for I in (16, 112)]


# the column split (u2tok_gemm_bf16_ex) on every form; with vt=n0,rows the V^T side output as the ViT's q|k|v product asks for it
def _split_cases():
    out = []
    vt = dict(nsplit=192, vt="384,256", gemm_big_grid=2)
    for K in (768, 1152):
        out.append(("qkv_drain_tail", desc(514, 576, K, 0, **vt), ("ints", "normal")))
    out.append(("qkv_drain", desc(512, 576, 768, 0, **vt), ("ints", "normal")))
    for K in (256, 512):
        out.append(("qkv_deep_tail", desc(514, 576, K, 0, **vt), ("ints", "normal")))
    out.append(("qkv_nodrain", desc(514, 576, 768, 0, gemm_big_drain=0, **vt), ("ints", "normal")))
    out.append(("qkv_tail_unfused", desc(514, 576, 768, 0, gemm_tail_fused=0, **vt), ("ints", "normal")))
    out.append(("split_tile64", desc(514, 576, 768, 0, nsplit=192, gemm_tile=64), ("ints", "normal")))
    out.append(("split_skinny", desc(200, 2048, 1024, BIAS_N, nsplit=64), ("ints", "normal")))
    out.append(("split_rows16", desc(16, 576, 768, BIAS_N, nsplit=192), ("ints", "normal")))
    out.append(("split_tile_splitk", desc(77, 520, 1160, 0, nsplit=192, gemm_splitk=3, scratch=SCRATCH), ("ints", "normal")))
    out.append(("split_big_sliced", desc(256, 384, 832, 0, nsplit=192, gemm_big=21, gemm_big_splitk=3, gemm_big_grid=2, scratch=SCRATCH),
                ("ints", "normal")))
    return out


BOUND_CASES = _tile_cases() + _splitk_cases() + _rows_cases() + _skinny_cases() + _big_cases() + _drain_cases() + _pair_cases()
SPLIT_CASES = _split_cases()
ALL_CASES = BOUND_CASES + SPLIT_CASES
FORMS = list(dict.fromkeys(f for f, _, _ in ALL_CASES))

# the kernel instantiation each form was written for: the first step of its pinned route (tests/test_gemm_plan.py)
FORM_KERNEL = {
    "tile64": "gemm_bf16_nt_kernel<64, 64, false, false>", "tile128": "gemm_bf16_nt_kernel<128, 128, false, false>",
    "tile64_bk": "gemm_bf16_nt_kernel<64, 64, false, true>", "tile128_bk": "gemm_bf16_nt_kernel<128, 128, false, true>",
    "tile64_abk": "gemm_bf16_nt_kernel<64, 64, true, true>", "tile128_abk": "gemm_bf16_nt_kernel<128, 128, true, true>",
    "tile64_ktile": "gemm_bf16_nt_kernel<64, 64, false, false>", "tile128_ktile": "gemm_bf16_nt_kernel<128, 128, false, false>",
    "tile64_splitk": "gemm_bf16_nt_kernel<64, 64, false, false>", "tile128_splitk": "gemm_bf16_nt_kernel<128, 128, false, false>",
    "rows16": "gemm_rows16_kernel<", "rows16_pair": "gemm_rows16_kernel<", "skinny": "gemm_skinny64_kernel<",
    "big20": "gemm_bt_kernel<4, false, false, 0, false, false>", "big21": "gemm_bt_kernel<3, false, false, 0, false, false>",
    "big22": "gemm_bt_kernel<2, false, false, 0, false, false>", "big24": "gemm_bt_kernel<3, false, false, 2, false, false>",
    "big26": "gemm_bt_kernel<4, false, false, 2, false, false>",
    "big20_sliced": "gemm_bt_kernel<4, false, true, 0, false, false>", "big21_sliced": "gemm_bt_kernel<3, false, true, 0, false, false>",
    "big22_sliced": "gemm_bt_kernel<2, false, true, 0, false, false>",
    "drain27": "gemm_bt_drain_kernel<", "heuristic_tail": "gemm_bt_drain_kernel<",
    "big21_pair": "gemm_bt_kernel<3, true, false, 0, false, false>",
    "qkv_drain_tail": "gemm_bt_drain_kernel<false, true, true>", "qkv_drain": "gemm_bt_drain_kernel<false, true, false>",
    "qkv_deep_tail": "gemm_bt_kernel<3, false, false, 2, true, true>", "qkv_nodrain": "gemm_bt_kernel<3, false, false, 2, true, true>",
    "qkv_tail_unfused": "gemm_bt_drain_kernel<false, true, false>",
    "split_tile64": "gemm_bf16_nt_kernel<64, 64, false, false>", "split_skinny": "gemm_skinny64_kernel<true>",
    "split_rows16": "gemm_rows16_kernel<8, false>", "split_tile_splitk": "gemm_bf16_nt_kernel<64, 64, false, false>",
    "split_big_sliced": "gemm_bt_kernel<3, false, true, 0, false, false>",
}
# a sliced or sub-form case additionally shows these in its route
FORM_ROUTE_HAS = {"tile64_splitk": "+reduce", "tile128_splitk": "+reduce", "big20_sliced": "+reduce", "big21_sliced": "+reduce",
                  "big22_sliced": "+reduce", "split_tile_splitk": "slices=3", "split_big_sliced": "slices=3",
                  "qkv_tail_unfused": "gemm_rows16_kernel<8, false> rows=512+2"}


def k_slices(p):
    """[k0, k1) of every K slice the launchers of gemm_plan.hip cut for the case's split option: whole 64-wide K tiles, cdiv(tiles,
    wanted) per slice, no empty slice"""
    want = p.get("gemm_splitk", 0) if "gemm_splitk" in p else p.get("gemm_big_splitk", 0)
    K = p["K"]
    if want <= 1:
        return [(0, K)]
    nkt = -(-K // 64)
    per = -(-nkt // want)
    return [(s * per * 64, min(K, (s + 1) * per * 64)) for s in range(-(-nkt // per))]


# ---------------------------------------------------------------------------------------------------------------- data
def _seed(form, p, data):
    return (sum(map(ord, form)) * 131 + p["M"] * 7 + p["N"] * 3 + p["K"] + p.get("flags", 0) * 17 + len(data)) & 0x7FFFFFFF


def gelu64(x):
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def silu64(x):
    return x * torch.sigmoid(x)


def silu_grad64(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def alpha_cols(p):
    """alpha per column (float64, as the kernels hold it: fp32)"""
    a = torch.full((p["N"],), float(torch.tensor(p.get("alpha", 1.0), dtype=torch.float32)), dtype=torch.float64)
    a[:p.get("nsplit", 0)] = float(torch.tensor(ALPHA_LO, dtype=torch.float32))
    return a


def inputs(form, p, data, el=BF16):
    """A (nz, M, K), B (nz, N, K), bias (N or M) or None, R (nz, M, N) or None in the element type -- the LOGICAL operands; K-major and
    K-tile-major storage is the GPU module's business"""
    M, N, K, nz, flags = p["M"], p["N"], p["K"], p.get("nz", 1), p.get("flags", 0)
    g = torch.Generator().manual_seed(_seed(form, p, data))
    nb = M if flags & BIAS_M else N
    if data == "ints":
        A, B = (torch.randint(-3, 4, s, generator=g).float() for s in ((nz, M, K), (nz, N, K)))
        bias, R = torch.randint(-3, 4, (nb,), generator=g).float(), torch.randint(-3, 4, (nz, M, N), generator=g).float()
    else:
        A, B = torch.randn(nz, M, K, generator=g), torch.randn(nz, N, K, generator=g) * K ** -0.5
        bias, R = torch.randn(nb, generator=g), torch.randn(nz, M, N, generator=g)
        if data == "cancel_k":
            h = K // 2
            A[:, :, h:2 * h] = A[:, :, :h]
            B[:, :, h:2 * h] = -B[:, :, :h] + torch.randn(nz, N, h, generator=g) * 2.0 ** -6 * K ** -0.5
    A, B = A.to(el.dtype), B.to(el.dtype)
    bias = bias.to(el.dtype) if flags & (BIAS_N | BIAS_M) else None
    if not flags & RES:
        R = None
    elif data == "cancel_r":
        lin = A.double() @ B.double().transpose(1, 2) * alpha_cols(p) + _bias_term(bias, flags)
        R = (-lin.float().to(el.dtype).float() + torch.randn(nz, M, N, generator=g) * 2.0 ** -6).to(el.dtype)
    else:
        R = R.to(el.dtype)
    return dict(A=A, B=B, bias=bias, R=R)


def _bias_term(bias, flags):
    if bias is None:
        return 0.0
    return bias.double()[:, None] if flags & BIAS_M else bias.double()[None, :]


def model(p, A, B, bias, R, el=BF16):
    """-> dict(ref, bound, exact): the float64 value of the epilogue on the rounded operands, the bound of the module docstring, and
    the columns in which the data make every fp32 operation exact (small integers, alpha a power of two, no GELU / SiLU), or False"""
    K, flags = p["K"], p.get("flags", 0)
    A64, B64 = A.double(), B.double()
    al = alpha_cols(p)
    if flags & SWIGLU:
        I = p["N"] // 2
        prod, S = A64 @ B64.transpose(1, 2), A64.abs() @ B64.abs().transpose(1, 2)
        g, up, Sg, Sup = prod[..., :I], prod[..., I:], S[..., :I], S[..., I:]
        sg, dsg = silu64(g), silu_grad64(g).abs()
        ref = sg * up
        t_silu = max(el.tiny, 2.0 ** -121)
        bound = ((el.U * ref.abs()).clamp_min(el.tiny) + (el.U * sg.abs()).clamp_min(t_silu) * up.abs()
                 + el.U * (dsg * g.abs() * up.abs() + sg.abs() * up.abs()) + (K + 8) * u * (dsg * up.abs() * Sg + sg.abs() * Sup))
        return dict(ref=ref, bound=bound, exact=False)
    lin = A64 @ B64.transpose(1, 2) * al + _bias_term(bias, flags)
    S = A64.abs() @ B64.abs().transpose(1, 2) * al.abs()
    babs = 0.0 if bias is None else _bias_term(bias, flags).abs()
    rabs = 0.0 if R is None else R.double().abs()
    if flags & GELU:
        ref = gelu64(lin) + (0.0 if R is None else R.double())
        bound = gelu_grad64(lin).abs() * (el.U * lin.abs() + (K + 8) * u * S) + GELU_EPS + el.U * ref.abs()
        return dict(ref=ref, bound=bound, exact=False)
    ref = lin + (0.0 if R is None else R.double())
    bound = (K + 8) * u * S + 4 * u * (babs + rabs) + (0.0 if flags & OUT_F32 else el.U * ref.abs())
    ints = bool((A64 == A64.round()).all() and (B64 == B64.round()).all())
    return dict(ref=ref, bound=bound, exact=((al == 0.5) | (al == 1.0)) if ints else False)


def round_once(ref, flags, el=BF16):
    """the float64 value as an exact kernel stores it"""
    return ref.float() if flags & OUT_F32 else ref.float().to(el.dtype)


def perm16(n):
    """position of key k in the flash kernel's V^T: inside every group of 16 keys [0-3, 8-11, 4-7, 12-15]"""
    k = torch.arange(n)
    j = k % 16
    return k - j + torch.where((j >= 4) & (j < 8), j + 4, torch.where((j >= 8) & (j < 12), j - 4, j))
