"""Tensor-level wrappers over the C ABI (include/u2tok.h).  PyTorch supplies device memory and the HIP
stream only; every computation below happens in libu2tok_hip.so."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import threading
from typing import Optional

import torch

from . import _lib

GEMM_BIAS_N, GEMM_BIAS_M, GEMM_GELU, GEMM_RESIDUAL, GEMM_OUT_F32 = 1, 2, 4, 8, 16
_VOL_DTYPE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


# ---------------------------------------------------------------------------------- contexts / device guard
class Context:
    """One execution context of the library (include/u2tok.h, "execution contexts"): its own option set, tokenizer side
    streams + events, split-K scratch table and profiling records.  Every GPU gets a default context on first use;
    `with ops.Context() as c:` runs the enclosed calls of this thread on a private one (e.g. a second model with other
    options, or a worker thread).  The bf16 and the f16 build of the library (_lib.load_library) each keep their own native
    context behind this object, created on first use; options set here reach both."""

    def __init__(self):
        self._handles = {}     # element type -> native handle
        self._options = {}
        self._scratch = {}     # (device index, stream) -> (pointer, bytes): split-K scratch registrations, replayed on every build
        self._lock = threading.Lock()
        self.handle_for("bf16")

    def handle_for(self, elem: str):
        with self._lock:
            hd = self._handles.get(elem)
            if hd is None:
                h = _lib.load_library(elem)
                hd = C.c_void_p()
                _lib.check(h.u2tok_ctx_create(C.byref(hd)), "u2tok_ctx_create")
                self._handles[elem] = hd
                for name, value in self._options.items():
                    self._set(h, hd, name, value)
                for (dev, stream), (ptr, nbytes) in self._scratch.items():
                    self._register_scratch(h, hd, dev, stream, ptr, nbytes)
            return hd

    @staticmethod
    def _register_scratch(h, hd, dev, stream, ptr, nbytes):
        prev = h.u2tok_ctx_get_current()
        with torch.cuda.device(dev):
            h.u2tok_ctx_set_current(hd)
            try:
                _lib.check(h.u2tok_set_gemm_scratch(ptr, nbytes, stream), "u2tok_set_gemm_scratch")
            finally:
                h.u2tok_ctx_set_current(prev)

    def set_gemm_scratch(self, dev, stream, ptr, nbytes) -> None:
        """split-K scratch of `stream` on device index `dev` (ptr None removes it): registered with every build of the library this
        context has a native handle for, and replayed on the ones created later (a bf16 path and an fp16 decoder share it)."""
        with self._lock:
            if ptr is None:
                self._scratch.pop((dev, stream), None)
            else:
                self._scratch[(dev, stream)] = (ptr, nbytes)
            handles = list(self._handles.items())
        for elem, hd in handles:
            self._register_scratch(_lib.load_library(elem), hd, dev, stream, ptr, 0 if ptr is None else nbytes)

    @property
    def handle(self):
        return self.handle_for(_lib.thread_elem())

    def close(self) -> None:
        with self._lock:
            handles, self._handles = self._handles, {}
        for elem, hd in handles.items():
            _lib.load_library(elem).u2tok_ctx_destroy(hd)

    @staticmethod
    def _set(h, hd, name, value):
        prev = h.u2tok_ctx_get_current()
        h.u2tok_ctx_set_current(hd)
        try:
            _lib.check(h.u2tok_set_option(name.encode(), int(value)), f"u2tok_set_option({name})")
        finally:
            h.u2tok_ctx_set_current(prev)

    def set_option(self, name: str, value: int) -> None:
        with self._lock:       # recorded first: a build whose native context is created meanwhile replays it (handle_for)
            self._options[name] = int(value)
            handles = list(self._handles.items())
        for elem, hd in handles:
            self._set(_lib.load_library(elem), hd, name, value)

    def __enter__(self):
        stack = getattr(_tls, "stack", None)
        if stack is None:
            stack = _tls.stack = []
        stack.append(self)
        return self

    def __exit__(self, *exc):
        _tls.stack.pop()
        return False


_tls = threading.local()
_default_ctx = {}  # device index -> Context
_default_lock = threading.Lock()


def active_context(device=None) -> Context:
    """Innermost `with Context()` of the calling thread, else the default context of `device` (current device if None)."""
    stack = getattr(_tls, "stack", None)
    if stack:
        return stack[-1]
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    with _default_lock:
        c = _default_ctx.get(idx)
        if c is None:
            c = _default_ctx[idx] = Context()
    return c


ELEM_OF = {torch.bfloat16: "bf16", torch.float16: "f16"}
ELEM_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}


def elem_dtype() -> torch.dtype:
    """The 16-bit element type of the op the calling thread is inside (bf16 outside one): what its buffers must be."""
    return ELEM_DTYPE[_lib.thread_elem()]


@contextlib.contextmanager
def on_device(t: torch.Tensor, elem=None):
    """Entry guard of every wrapper: makes the tensor's GPU the current HIP device (the library launches on the current
    device; a model on cuda:1 must not launch on cuda:0), picks the library build by ELEMENT TYPE -- `elem` (a dtype: what the
    module's parameters are), else t's dtype if it is bf16 / fp16, else what an enclosing guard chose -- binds the active
    context and yields (library handle, the current torch stream OF THAT DEVICE)."""
    if not t.is_cuda:
        raise RuntimeError("expected a GPU tensor (the u2tok HIP path has no CPU fallback)")
    dt = elem if elem is not None else t.dtype
    name = ELEM_OF.get(dt)
    if name is None and elem is not None:
        raise RuntimeError(f"the u2tok HIP path computes on bfloat16 or float16 parameters, got {elem}")
    prev = _lib.set_thread_elem(name) if name is not None else None
    try:
        h = _lib.load_library()
        with torch.cuda.device(t.device):
            h.u2tok_ctx_set_current(active_context(t.device).handle)
            yield h, torch.cuda.current_stream(t.device).cuda_stream
    finally:
        if name is not None:
            _lib.set_thread_elem(prev)


def _guarded(fn=None, *, infer=True):
    """Runs a building-block wrapper under on_device(first tensor argument); _stream() is that device's stream.  Element type
    of the op = the keyword `elem` (a dtype) if the caller names one, else the first bf16 / fp16 tensor argument's; wrappers
    whose 16-bit operand is not an argument (infer=False: im2col's voxels may be fp16 under a bf16 model, softmax_rows takes fp32
    scores) default to bf16."""
    if fn is None:
        return functools.partial(_guarded, infer=infer)

    @functools.wraps(fn)
    def wrapper(*args, elem=None, **kwargs):
        ts = [a for a in list(args) + list(kwargs.values()) if torch.is_tensor(a)]
        t = ts[0] if ts else None
        if t is None or not t.is_cuda:
            raise RuntimeError(f"{fn.__name__}: expected GPU tensors (the u2tok HIP path has no CPU fallback)")
        if elem is None:
            elem = next((a.dtype for a in ts if a.dtype in ELEM_OF), None) if infer else torch.bfloat16
        with on_device(t, elem) as (_, st):
            prev = getattr(_tls, "stream", None)
            _tls.stream = st
            try:
                return fn(*args, **kwargs)
            finally:
                _tls.stream = prev

    return wrapper


def _stream() -> int:
    st = getattr(_tls, "stream", None)
    return st if st is not None else torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


ELEM = "element type of the running op"   # _need(t, ELEM, ...): bf16 in the bf16 build's ops, fp16 in the f16 build's


def _need(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the u2tok HIP path has no CPU fallback)")
    if dtype is ELEM:
        dtype = elem_dtype()
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


def training_needs_bf16(dtype, who: str) -> None:
    if dtype != torch.bfloat16:
        raise RuntimeError(f"{who}: float16 parameters are supported for inference only (train in bf16, as train_stage1.py / "
                           "config/ds_config.json do)")


def set_option(name: str, value: int) -> None:
    """Option of the active context (the current device's default context unless inside `with Context()`)."""
    active_context().set_option(name, value)


def device_check() -> None:
    _lib.check(_lib.load_library().u2tok_device_check(), "u2tok_device_check")


def vol_dtype_code(dtype) -> int:
    if dtype not in _VOL_DTYPE:
        raise RuntimeError(f"unsupported voxel dtype {dtype} (fp16 / bf16 / fp32)")
    return _VOL_DTYPE[dtype]


GEMM_B_KTILE = 64
GEMM_A_KMAJOR, GEMM_B_KMAJOR = 128, 256


def pack_ktile_major(w: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight (N, K) -> K-tile-major (K/64, N, 64): the 64 x 64 tile a workgroup stages per K step becomes one
    contiguous 8 KB block (cold weights stream from HBM in long bursts instead of 128-byte pieces 2 K bytes apart)."""
    N, K = w.shape
    assert K % 64 == 0
    return w.view(N, K // 64, 64).permute(1, 0, 2).contiguous()


@_guarded
def gemm(a: torch.Tensor, b: torch.Tensor, *, bias=None, residual=None, bias_m=False, gelu=False, out_f32=False,
         alpha=1.0, out: Optional[torch.Tensor] = None, b_ktile: bool = False) -> torch.Tensor:
    """C = epi(alpha * A B^T) for A (..., M, K), B (N, K) or batched (Z, N, K); b_ktile: B = pack_ktile_major(weight)."""
    if b_ktile:
        kt, n_, _ = b.shape
        h = _lib.load_library()
        a2 = _need(a, ELEM, "A").reshape(-1, a.shape[-1]).contiguous()
        M, K = a2.shape
        assert kt * 64 == K
        if out is None:
            out = torch.empty((M, n_), dtype=torch.float32 if out_f32 else elem_dtype(), device=a.device)
        flags = GEMM_B_KTILE | (GEMM_OUT_F32 if out_f32 else 0) | (GEMM_GELU if gelu else 0)
        if bias is not None:
            flags |= GEMM_BIAS_M if bias_m else GEMM_BIAS_N
        if residual is not None:
            flags |= GEMM_RESIDUAL
            residual = residual.contiguous()
        st = h.u2tok_gemm_bf16(_ptr(a2), _ptr(b), _ptr(out), _ptr(bias), _ptr(residual), M, n_, K, K, 64, n_, n_, 1, 1,
                               0, 0, 0, 0, 0, 0, 0, 0, float(alpha), flags, _stream())
        _lib.check(st, "u2tok_gemm_bf16")
        return out
    h = _lib.load_library()
    _need(a, ELEM, "A"), _need(b, ELEM, "B")
    a3 = a.reshape(-1, a.shape[-2], a.shape[-1]) if b.dim() == 3 else a.reshape(1, -1, a.shape[-1])
    a3 = a3.contiguous()
    b = b.contiguous()
    Z, M, K = a3.shape
    N = b.shape[-2]
    assert b.shape[-1] == K
    if out is None:
        out = torch.empty((Z, M, N), dtype=torch.float32 if out_f32 else elem_dtype(), device=a.device)
    flags = (GEMM_OUT_F32 if out_f32 else 0) | (GEMM_GELU if gelu else 0)
    if bias is not None:
        flags |= GEMM_BIAS_M if bias_m else GEMM_BIAS_N
    if residual is not None:
        flags |= GEMM_RESIDUAL
        residual = residual.contiguous()
    sB = N * K if b.dim() == 3 else 0
    st = h.u2tok_gemm_bf16(_ptr(a3), _ptr(b), _ptr(out), _ptr(bias), _ptr(residual), M, N, K, K, K, N, N, Z, 1,
                           M * K, 0, sB, 0, M * N, 0, M * N if residual is not None else 0, 0, float(alpha), flags,
                           _stream())
    _lib.check(st, "u2tok_gemm_bf16")
    return out.reshape(*a.shape[:-1], N) if b.dim() == 2 else out


GEMM_SWIGLU = 512


def gemm_swiglu_supported(rows: int, K: int, I: int) -> bool:
    """Shapes the gate | up pair form of u2tok_gemm_bf16 (flag 512) takes."""
    return rows >= 1 and K % 64 == 0 and K >= 128 and I % 16 == 0 and rows * K < (1 << 30) and 2 * I * K < (1 << 30)


@_guarded
def gemm_swiglu(a: torch.Tensor, w_gate_up: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, I) = bf16(silu(a @ gate^T)) * (a @ up^T) for w_gate_up (2 I, K) = gate rows then up rows: the values of
    `swiglu(gemm(a, w_gate_up))` bit for bit, the (rows, 2 I) intermediate never written (LlamaMLP / Qwen3MLP)."""
    h = _lib.load_library()
    _need(a, ELEM, "A"), _need(w_gate_up, ELEM, "W")
    a2 = a.reshape(-1, a.shape[-1]).contiguous()
    w = w_gate_up.contiguous()
    M, K = a2.shape
    N = w.shape[0]
    I = N // 2
    if w.shape[1] != K or N % 2 or not gemm_swiglu_supported(M, K, I):
        raise RuntimeError(f"gemm_swiglu: unsupported shape rows {M}, K {K}, 2I {N}")
    if out is None:
        out = torch.empty((M, I), dtype=elem_dtype(), device=a.device)
    st = h.u2tok_gemm_bf16(_ptr(a2), _ptr(w), _ptr(out), None, None, M, N, K, K, K, out.stride(0), 0, 1, 1,
                           0, 0, 0, 0, 0, 0, 0, 0, 1.0, GEMM_SWIGLU, _stream())
    _lib.check(st, "u2tok_gemm_bf16 (swiglu pair)")
    return out.reshape(*a.shape[:-1], I)


@_guarded
def gemm_kmajor(a: torch.Tensor, b: torch.Tensor, *, a_kmajor: bool, alpha=1.0, out_f32=False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Products with K-major operands (no transposes in HBM; u2tok_gemm_bf16 flags 128 / 256):
         a_kmajor = False:  C (M, N) = A (M, K) @ B (K, N)          -- dX = dY W
         a_kmajor = True:   C (M, N) = A (K, M)^T @ B (K, N)        -- dW = dY^T X
    Dense 2-D bf16 operands; the K-major dimensions (N, and M when a_kmajor) must be multiples of 8.  out: a dense (M, N) tensor
    of the result's type to write into (e.g. a block of rows of a larger gradient)."""
    h = _lib.load_library()
    a = _need(a, ELEM, "A").contiguous()
    b = _need(b, ELEM, "B").contiguous()
    K, N = b.shape
    M = a.shape[1] if a_kmajor else a.shape[0]
    if (a.shape[0] if a_kmajor else a.shape[1]) != K:
        raise RuntimeError(f"gemm_kmajor: contraction sizes differ ({tuple(a.shape)}, {tuple(b.shape)}, a_kmajor={a_kmajor})")
    dtype = torch.float32 if out_f32 else elem_dtype()
    if out is None:
        out = torch.empty((M, N), dtype=dtype, device=a.device)
    elif out.shape != (M, N) or out.dtype != dtype or not out.is_contiguous() or out.device != a.device:
        raise RuntimeError(f"gemm_kmajor: out must be a dense ({M}, {N}) {dtype} tensor on {a.device}")
    flags = GEMM_B_KMAJOR | (GEMM_A_KMAJOR if a_kmajor else 0) | (GEMM_OUT_F32 if out_f32 else 0)
    st = h.u2tok_gemm_bf16(_ptr(a), _ptr(b), _ptr(out), None, None, M, N, K, a.shape[1], N, N, N, 1, 1,
                           0, 0, 0, 0, 0, 0, 0, 0, float(alpha), flags, _stream())
    _lib.check(st, "u2tok_gemm_bf16")
    return out


def set_gemm_scratch(buf: Optional[torch.Tensor]) -> None:
    """Registers `buf` (any dtype, on the GPU) as split-K scratch for gemm() calls on the current stream; None removes
    it.  The caller keeps the tensor alive while products may be in flight."""
    dev = buf.device if buf is not None else torch.device("cuda", torch.cuda.current_device())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
    active_context(dev).set_gemm_scratch(idx, stream, _ptr(buf), 0 if buf is None else buf.numel() * buf.element_size())


@_guarded
def layernorm(x, w, b, residual=None, eps=1e-5):
    h = _lib.load_library()
    x = _need(x, ELEM, "x").contiguous()
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    if residual is not None:
        residual = residual.contiguous()
    _lib.check(h.u2tok_layernorm_bf16(_ptr(x), _ptr(residual), _ptr(w), _ptr(b), _ptr(y), rows, x.shape[-1],
                                      float(eps), _stream()), "u2tok_layernorm_bf16")
    return y


@_guarded(infer=False)
def softmax_rows(s: torch.Tensor, scale=1.0, rel_bias=None, heads=1, max_len=0, ldp=None):
    """s: (Z, R, n) fp32 -> (Z, R, ldp) elements (bf16, or `elem=torch.float16`; columns >= n are zero); rel_bias in that type."""
    h = _lib.load_library()
    s = _need(s, torch.float32, "S").contiguous()
    Z, R, n = s.shape
    ldp = ldp or (n + 7) // 8 * 8
    p = torch.empty((Z, R, ldp), dtype=elem_dtype(), device=s.device)
    _lib.check(h.u2tok_softmax_rows(_ptr(s), _ptr(p), Z, R, n, n, ldp, float(scale), _ptr(rel_bias), heads, max_len,
                                    _stream()), "u2tok_softmax_rows")
    return p


@_guarded
def transpose(x: torch.Tensor, ld_out=None, perm16=False):
    """x: (Z, R, C) bf16 -> (Z, C, ld_out) with zero padding."""
    h = _lib.load_library()
    x = _need(x, ELEM, "x").contiguous()
    Z, R, Cc = x.shape
    ld_out = ld_out or R
    y = torch.empty((Z, Cc, ld_out), dtype=elem_dtype(), device=x.device)
    _lib.check(h.u2tok_transpose_bf16(_ptr(x), _ptr(y), Z, R, Cc, Cc, ld_out, R * Cc, Cc * ld_out, int(perm16),
                                      _stream()), "u2tok_transpose_bf16")
    return y


@_guarded(infer=False)
def im2col(vol: torch.Tensor, patch):
    """voxels (fp16 / bf16 / fp32) -> patch rows in the element type (bf16, or `elem=torch.float16`)."""
    h = _lib.load_library()
    vol = vol.contiguous()
    nchunk = vol.shape[0]
    D, H, W = vol.shape[-3:]
    p1, p2, p3 = patch
    ntok = (D // p1) * (H // p2) * (W // p3)
    out = torch.empty((nchunk, ntok, p1 * p2 * p3), dtype=elem_dtype(), device=vol.device)
    _lib.check(h.u2tok_im2col_patches(_ptr(vol), vol_dtype_code(vol.dtype), _ptr(out), nchunk, D, H, W, p1, p2, p3,
                                      _stream()), "u2tok_im2col_patches")
    return out


@_guarded
def avgpool3d_tokens(x: torch.Tensor, grid, window):
    h = _lib.load_library()
    x = _need(x, ELEM, "x").contiguous()
    nb, _, Cc = x.shape
    g1, g2, g3 = grid
    w1, w2, w3 = window
    y = torch.empty((nb, (g1 // w1) * (g2 // w2) * (g3 // w3), Cc), dtype=elem_dtype(), device=x.device)
    _lib.check(h.u2tok_avgpool3d_tokens(_ptr(x), _ptr(y), nb, g1, g2, g3, w1, w2, w3, Cc, _stream()),
               "u2tok_avgpool3d_tokens")
    return y


@_guarded
def embed_splice(table: torch.Tensor, ids: torch.Tensor, feats: Optional[torch.Tensor] = None):
    """embed_tokens(ids) with feats (B, nfeat, E) spliced over positions 1..nfeat (u2_arch.py:109,113-116)."""
    h = _lib.load_library()
    table = _need(table, ELEM, "embed_tokens.weight")
    if not table.is_contiguous():
        raise RuntimeError("embed_tokens.weight must be contiguous")
    ids = _need(ids, torch.int64, "ids").contiguous()
    B, S = ids.shape
    E = table.shape[1]
    nfeat = 0
    if feats is not None:
        feats = _need(feats, ELEM, "feats").contiguous()
        nfeat = feats.shape[1]
    out = torch.empty((B, S, E), dtype=elem_dtype(), device=table.device)
    _lib.check(h.u2tok_embed_splice(_ptr(table), _ptr(ids), _ptr(feats), _ptr(out), B, S, E, nfeat, table.shape[0],
                                    _stream()), "u2tok_embed_splice")
    return out


@_guarded
def score_gemv(x, w, bias):
    h = _lib.load_library()
    x = _need(x, ELEM, "x").contiguous()
    rows = x.numel() // x.shape[-1]
    s = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _lib.check(h.u2tok_score_gemv(_ptr(x), _ptr(w), _ptr(bias), _ptr(s), rows, x.shape[-1], _stream()),
               "u2tok_score_gemv")
    return s


@_guarded
def topk_sorted(scores: torch.Tensor, k: int):
    h = _lib.load_library()
    scores = _need(scores, torch.float32, "scores").contiguous()
    B, n = scores.shape
    idx = torch.empty((B, k), dtype=torch.int64, device=scores.device)
    _lib.check(h.u2tok_topk_sorted(_ptr(scores), _ptr(idx), B, n, k, _stream()), "u2tok_topk_sorted")
    return idx


@_guarded
def gather_rows(x, idx):
    h = _lib.load_library()
    x = _need(x, ELEM, "x").contiguous()
    B, n, E = x.shape
    k = idx.shape[1]
    out = torch.empty((B, k, E), dtype=elem_dtype(), device=x.device)
    _lib.check(h.u2tok_gather_rows(_ptr(x), _ptr(idx.contiguous()), _ptr(out), B, n, k, E, _stream()),
               "u2tok_gather_rows")
    return out


@_guarded
def multiscale_pool(x, gate_w=None, gate_b=None):
    h = _lib.load_library()
    x = _need(x, ELEM, "x").contiguous()
    B, k, E = x.shape
    out = torch.empty((B, k + k // 2 + k // 4, E), dtype=elem_dtype(), device=x.device)
    ws = torch.empty((B * 3 * 16 * ((E + 255) // 256),), dtype=torch.float32, device=x.device)
    _lib.check(h.u2tok_multiscale_pool(_ptr(x), _ptr(out), B, k, E, _ptr(gate_w), _ptr(gate_b), _ptr(ws), _stream()),
               "u2tok_multiscale_pool")
    return out


@_guarded
def temporal_attention(q, k, v, B, T, N, H, scale, rel_bias=None, max_len=512):
    """q/k/v: (B*T*N, E) rows in (b t n) order; T <= 16, head dim E / H in {64, 128, 256, 384, 512}."""
    h = _lib.load_library()
    E = q.shape[-1]
    out = torch.empty((B * T * N, E), dtype=elem_dtype(), device=q.device)
    _lib.check(h.u2tok_temporal_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, T, N, H, E // H, q.stride(0),
                                          E, float(scale), _ptr(rel_bias), max_len, _stream()),
               "u2tok_temporal_attention")
    return out


@_guarded
def flash_attention_d64(qkv: torch.Tensor, heads: int, scale: float, extra_last: bool = False, return_lse: bool = False):
    """qkv: (nb, S, 3*heads*64) bf16 in MONAI SABlock column order (q | k | v).  extra_last=True runs the last row of
    every batch through the kernel's "extra row" path (how the ViT tower feeds its cls token); same result.
    return_lse: also the row statistics (nb * heads, S rounded up to 64) fp32 that flash_attention_d64_bwd takes."""
    h = _lib.load_library()
    qkv = _need(qkv, ELEM, "qkv").contiguous()
    nb, S, three = qkv.shape
    Hd = three // 3
    Sm = S - 1 if extra_last else S
    if Sm < 1:
        raise RuntimeError("flash_attention_d64: at least one main row is required")
    S_pad = (Sm + 63) // 64 * 64
    vt = torch.empty((nb, Hd, S_pad), dtype=elem_dtype(), device=qkv.device)
    v_view = qkv[:, :, 2 * Hd:]
    _lib.check(h.u2tok_transpose_bf16(v_view.data_ptr(), _ptr(vt), nb, Sm, Hd, 3 * Hd, S_pad, S * 3 * Hd, Hd * S_pad,
                                      1, _stream()), "u2tok_transpose_bf16")
    out = torch.empty((nb, S, Hd), dtype=elem_dtype(), device=qkv.device)
    es = qkv.element_size()
    x0 = qkv.data_ptr() + (S - 1) * 3 * Hd * es
    args = (qkv.data_ptr(), qkv.data_ptr() + Hd * es, _ptr(vt), _ptr(out), nb, Sm, heads, 3 * Hd, S * 3 * Hd, Hd, S * Hd,
            S_pad, float(scale), x0 if extra_last else None, x0 + Hd * es if extra_last else None,
            x0 + 2 * Hd * es if extra_last else None, out.data_ptr() + (S - 1) * Hd * es if extra_last else None,
            S * 3 * Hd, S * Hd, 1 if extra_last else 0)
    if return_lse:
        lse_ld = (S + 63) // 64 * 64
        lse = torch.empty((nb * heads, lse_ld), dtype=torch.float32, device=qkv.device)
        _lib.check(h.u2tok_flash_attention_d64_lse(*args, _ptr(lse), lse_ld, _stream()), "u2tok_flash_attention_d64_lse")
        return out, lse
    _lib.check(h.u2tok_flash_attention_d64(*args, _stream()), "u2tok_flash_attention_d64")
    return out


@_guarded
def flash_attention_d64_bwd(qkv: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, heads: int, scale: float,
                            lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of flash_attention_d64 w.r.t. its packed input: qkv (nb, S, 3*heads*64), out / d_out (nb, S, heads*64), all
    bf16 -> d_qkv like qkv (u2tok_flash_attention_d64_bwd: two flash-style kernels, no (S x S) tensor in HBM).  lse: the
    forward's row statistics (flash_attention_d64(..., return_lse=True)); without them the backward rebuilds them."""
    h = _lib.load_library()
    qkv = _need(qkv, ELEM, "qkv").contiguous()
    out = _need(out, ELEM, "out").contiguous()
    d_out = _need(d_out, ELEM, "d_out").contiguous()
    nb, S, three = qkv.shape
    Hd = three // 3
    if Hd != heads * 64 or out.shape != (nb, S, Hd) or d_out.shape != out.shape:
        raise RuntimeError("flash_attention_d64_bwd: head dim 64 and out / d_out of shape (nb, S, heads * 64) required")
    if lse is not None:
        lse = _need(lse, torch.float32, "lse").contiguous()
        if lse.dim() != 2 or lse.shape[0] != nb * heads or lse.shape[1] < S:
            raise RuntimeError("flash_attention_d64_bwd: lse must be (nb * heads, >= S) fp32")
    dqkv = torch.empty_like(qkv)
    nbytes = h.u2tok_flash_attention_d64_bwd_workspace_bytes(nb, S, heads)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
    es = qkv.element_size()
    _lib.check(h.u2tok_flash_attention_d64_bwd(qkv.data_ptr(), qkv.data_ptr() + Hd * es, qkv.data_ptr() + 2 * Hd * es,
                                               3 * Hd, S * 3 * Hd, _ptr(out), _ptr(d_out), Hd, S * Hd,
                                               dqkv.data_ptr(), dqkv.data_ptr() + Hd * es, dqkv.data_ptr() + 2 * Hd * es,
                                               3 * Hd, S * 3 * Hd, nb, S, heads, float(scale), _ptr(lse),
                                               0 if lse is None else lse.shape[-1], _ptr(ws), nbytes, _stream()),
               "u2tok_flash_attention_d64_bwd")
    return dqkv


def _kv_len_arg(kv_len, nb: int, device):
    if kv_len is None:
        return None
    if kv_len.dtype != torch.int32 or kv_len.device != device or kv_len.shape != (nb,) or not kv_len.is_contiguous():
        raise RuntimeError(f"kv_len must be a contiguous int32 ({nb},) tensor on {device}")
    return kv_len


def _attn_call(who: str, q, k, v, heads: int, kv_heads, scale: float, kv_start=None, kv_len=None, cache=None):
    """What the attention wrappers below share: the checks of q (nb, Sq, heads * d), k / v (nb, Skv, kv_heads * d) -- kv_heads
    None: tok_attention's equal heads -- and of the key range tensors, the output, and the arguments every C entry point begins
    with (q ... o_bs, scale) -> (out, args).  cache: attention_gqa_band's 4-D k / v, checked there, as (Skv, ldk, k_bs)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _need(t, ELEM, n)
        if (t is q or cache is None) and (t.dim() != 3 or t.stride(2) != 1):
            raise RuntimeError(f"{who}: {n} must be (nb, S, H * d) with a contiguous last dim")
    nb, Sq, Eq = q.shape
    d = Eq // heads
    hk = heads if kv_heads is None else kv_heads
    Skv, ldk, kbs = cache or (k.shape[1], k.stride(1), k.stride(0))
    ldv, vbs = (ldk, kbs) if cache else (v.stride(1), v.stride(0))
    if Eq % heads or k.shape != ((nb, hk, Skv, d) if cache else (nb, Skv, hk * d)) or v.shape != k.shape or heads % hk:
        raise RuntimeError(f"{who}: shapes {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}, heads {heads}/{hk}")
    for t in (kv_start, kv_len):
        _kv_len_arg(t, nb, q.device)
    out = torch.empty((nb, Sq, Eq), dtype=elem_dtype(), device=q.device)
    args = [_ptr(q), _ptr(k), _ptr(v), _ptr(out), nb, Sq, Skv, heads] + ([] if kv_heads is None else [kv_heads]) + \
           [d, q.stride(1), ldk, ldv, Eq, q.stride(0), kbs, vbs, Sq * Eq, float(scale)]
    return out, args


@_guarded
def tok_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float, rel_bias=None, max_len=512,
                  splits: int = 0) -> torch.Tensor:
    """Fused attention core of the tokenizer's attention modules (u2tok_tok_attention; rma.py:60-75, tta.py:55-61):
    q (nb, Sq, E), k / v (nb, Skv, E) bf16 -- any views whose last dim is contiguous (e.g. column slices of a packed q|k|v
    buffer) -> softmax(q k^T scale + rel_bias[j - i + max_len - 1][h]) v as (nb, Sq, E).  splits: 0 = heuristic key split.
    Head dim E / heads in {64, 96, 128, 256, 384, 512}."""
    h = _lib.load_library()
    out, args = _attn_call("tok_attention", q, k, v, heads, None, scale)
    nb, Sq, E = out.shape
    nbytes = h.u2tok_tok_attention_workspace_bytes(nb, heads, Sq, k.shape[1], E // heads)
    if splits > 1:
        nbytes = max(nbytes, splits * nb * Sq * (E * 4 + heads * 8))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    _lib.check(h.u2tok_tok_attention(*args, _ptr(rel_bias), max_len, int(splits), _ptr(ws), ws.numel(), _stream()),
               "u2tok_tok_attention")
    return out


# ---------------------------------------------------------------------------------- decoder prefill blocks (prefill.py)
@_guarded
def attention_gqa(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, kv_heads: int, scale: float,
                  causal: bool = True, split_keys: bool = False) -> torch.Tensor:
    """softmax(q k^T scale [+ causal mask]) v with grouped-query heads (u2tok_attention_gqa): q (nb, Sq, heads * d),
    k / v (nb, Skv, kv_heads * d) -- views with a contiguous last dim -> (nb, Sq, heads * d); d in {64, 96, 128, 256, 384, 512}.
    split_keys (not causal): key ranges on separate workgroups, merged in a fixed order (u2tok_attention_gqa_split) -- few
    query rows over a long KV cache (decode steps)."""
    h = _lib.load_library()
    out, args = _attn_call("attention_gqa", q, k, v, heads, kv_heads, scale)
    if split_keys and not causal:
        nb, Sq, Eq = out.shape
        nbytes = h.u2tok_tok_attention_workspace_bytes(nb, heads, Sq, k.shape[1], Eq // heads)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
        _lib.check(h.u2tok_attention_gqa_split(*args, _ptr(ws) if nbytes else None, nbytes, _stream()), "u2tok_attention_gqa_split")
        return out
    _lib.check(h.u2tok_attention_gqa(*args, int(bool(causal)), _stream()), "u2tok_attention_gqa")
    return out


@_guarded
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """LlamaRMSNorm / Qwen3RMSNorm over the last dim of x (rows, C) bf16."""
    h = _lib.load_library()
    x = _need(x, ELEM, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise RuntimeError("rmsnorm: x must be (rows, C) with a contiguous last dim")
    y = torch.empty((x.shape[0], x.shape[1]), dtype=elem_dtype(), device=x.device)
    _lib.check(h.u2tok_rmsnorm_bf16(_ptr(x), _ptr(_need(w, ELEM, "w")), _ptr(y), x.shape[0], x.shape[1], x.stride(0),
                                    x.shape[1], float(eps), _stream()), "u2tok_rmsnorm_bf16")
    return y


@_guarded
def qk_norm_rope(qkv: torch.Tensor, q_norm_w, k_norm_w, cos: torch.Tensor, sin: torch.Tensor, heads: int, kv_heads: int,
                 head_dim: int, eps: float = 1e-6, kv_cache_seq: int = 0, kv_out=None, kv_pos: int = 0):
    """In place on the q and k heads of qkv (rows, (heads + 2 kv_heads) * head_dim): per-head RMSNorm (weights may both be
    None: Llama) then rotary embedding with cos / sin (rows, head_dim), fp32 or bf16 (u2tok_qk_norm_rope); head_dim 64 / 96 / 128.
    kv_cache_seq = S > 0 (rows = batch * S): also returns the finished keys and the values as fresh dense
    (batch, kv_heads, S, head_dim) tensors -- the KV cache's layout (u2tok_qk_norm_rope_kv): (qkv, k_cache, v_cache).
    kv_out = (k_buf, v_buf): write them instead at positions kv_pos .. kv_pos + S - 1 of (batch, kv_heads, capacity, head_dim)
    buffers (an append-in-place cache)."""
    h = _lib.load_library()
    _need(qkv, ELEM, "qkv")
    rows = qkv.shape[0]
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] != (heads + 2 * kv_heads) * head_dim:
        raise RuntimeError("qk_norm_rope: qkv must be (rows, (heads + 2 kv_heads) * head_dim)")
    if cos.dtype != sin.dtype or cos.dtype not in (torch.float32, elem_dtype()) or cos.shape != (rows, head_dim) \
            or sin.shape != cos.shape or cos.stride(1) != 1 or sin.stride(1) != 1 or cos.stride(0) != sin.stride(0):
        raise RuntimeError("qk_norm_rope: cos / sin must be (rows, head_dim) fp32 or bf16 with equal strides")
    if kv_cache_seq:
        S = int(kv_cache_seq)
        if S <= 0 or rows % S:
            raise RuntimeError("qk_norm_rope: rows must be batch * kv_cache_seq")
        kvs, pos = 0, 0
        if kv_out is not None:
            kc, vc = kv_out
            for t in (kc, vc):
                _need(t, ELEM, "kv_out")
                if t.dim() != 4 or t.shape[0] != rows // S or t.shape[1] != kv_heads or t.shape[3] != head_dim or t.stride(3) != 1 \
                        or t.stride(2) != head_dim or t.stride(0) != kv_heads * t.stride(1) or kv_pos + S > t.shape[2]:
                    raise RuntimeError("qk_norm_rope: kv_out must be (batch, kv_heads, capacity, head_dim) buffers with room")
            if kc.stride(1) != vc.stride(1):
                raise RuntimeError("qk_norm_rope: the two kv_out buffers must have the same capacity")
            kvs, pos = kc.stride(1), int(kv_pos)
        else:
            kc = torch.empty((rows // S, kv_heads, S, head_dim), dtype=elem_dtype(), device=qkv.device)
            vc = torch.empty_like(kc)
        _lib.check(h.u2tok_qk_norm_rope_kv(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(cos), _ptr(sin),
                                           int(cos.dtype == torch.float32), rows, heads, kv_heads, head_dim, qkv.stride(0),
                                           cos.stride(0), float(eps), _ptr(kc), _ptr(vc), S, kvs, pos, _stream()),
                   "u2tok_qk_norm_rope_kv")
        return qkv, kc, vc
    _lib.check(h.u2tok_qk_norm_rope(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(cos), _ptr(sin),
                                    int(cos.dtype == torch.float32), rows, heads, kv_heads, head_dim, qkv.stride(0),
                                    cos.stride(0), float(eps), _stream()), "u2tok_qk_norm_rope")
    return qkv


@_guarded
def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """(rows, 2 I) packed gate | up -> silu(gate) * up (rows, I)  (u2tok_swiglu_bf16)."""
    h = _lib.load_library()
    _need(gate_up, ELEM, "gate_up")
    rows, two_i = gate_up.shape
    out = torch.empty((rows, two_i // 2), dtype=elem_dtype(), device=gate_up.device)
    _lib.check(h.u2tok_swiglu_bf16(_ptr(gate_up), _ptr(out), rows, two_i // 2, gate_up.stride(0), two_i // 2, _stream()),
               "u2tok_swiglu_bf16")
    return out


# ---------------------------------------------------------------------------------- FP8 (e4m3) weight-only products
FP8_MAX = 448.0   # largest finite e4m3 (OCP, torch.float8_e4m3fn); the codes 0x7F / 0xFF are NaN


def quantize_rows_fp8(w: torch.Tensor):
    """Per-row e4m3 quantisation of a 2-D weight (N, K) in bf16 / fp16 / fp32 -> (W8 (N, K) torch.float8_e4m3fn, contiguous,
    scale (N,) fp32) with scale[n] = amax_n / 448 (1.0 for an all-zero row) and W8 = clamp(W / scale, +-448) rounded to e4m3.
    The clamp is what keeps the NaN codes out: torch converts |v| > 448 to NaN, and W / scale can exceed 448 by a rounding.
    Plain torch, any device; not a hot path (the decode route quantises a layer once, prefill.py)."""
    if w.dim() != 2 or w.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise RuntimeError(f"quantize_rows_fp8: expected a 2-D bf16 / fp16 / fp32 weight, got {tuple(w.shape)} {w.dtype}")
    wf = w.detach().float()
    amax = wf.abs().amax(1)
    if not bool(torch.isfinite(amax).all()):
        raise RuntimeError("quantize_rows_fp8: the weight holds inf / nan")
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    w8 = (wf / scale[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).contiguous()
    return w8, scale


def dequantize_rows_fp8(w8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 (N, K) = e4m3(W8) * scale[n]: what the e4m3 products multiply by, exactly."""
    return w8.float() * scale.float()[:, None]


def snap_fp8_(module):
    """In place, for every nn.Linear weight in `module` (or a 2-D tensor): move each row onto values the row quantiser keeps
    EXACTLY -- the row's scale becomes a power of two (the smallest one >= amax / 448), its values e4m3 multiples of it, and the
    largest element is forced to +-448 scale, so that quantize_rows_fp8 finds that same scale.  Then
    dequantize_rows_fp8(*quantize_rows_fp8(w)) == w bit for bit, and w is exact in bf16 (fp16 while 2^-9 scale >= 2^-24): a
    model with snapped weights and its e4m3 decode step compute the same function.  For tests and the A/B tool."""
    ws = [module] if torch.is_tensor(module) else [m.weight.data for m in module.modules() if isinstance(m, torch.nn.Linear)]
    for w in ws:
        wf = w.detach().float()
        amax = wf.abs().amax(1)
        live = amax > 0
        sc = torch.where(live, torch.exp2(torch.ceil(torch.log2(torch.where(live, amax, torch.ones_like(amax)) / FP8_MAX))),
                         torch.ones_like(amax))
        q = (wf / sc[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).float()
        top = wf.abs().argmax(1, keepdim=True)
        sign = torch.where(wf.gather(1, top) < 0, -1.0, 1.0)
        q.scatter_(1, top, torch.where(live[:, None], sign * FP8_MAX, torch.zeros_like(sign)))
        w.copy_((q * sc[:, None]).to(w.dtype))
    return module


# ------------------------------------------------------------------- MXFP4 (e2m1 codes, e8m0 block scales) weight-only products
FP4_BLOCK = 32                       # consecutive k of one weight row that share a scale (OCP Microscaling)
FP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # |e2m1| by code & 7; bit 3 is the sign
FP4_X_MIN, FP4_X_MAX = -23, 13       # block exponents the quantiser emits: every e2m1 * 2^x in it is exact in fp16 AND in bf16


def _fp4_blocks(who, w):
    if not torch.is_tensor(w) or w.dim() != 2 or w.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise RuntimeError(f"{who}: expected a 2-D bf16 / fp16 / fp32 weight")
    N, K = w.shape
    if K % 128:
        raise RuntimeError(f"{who}: K = {K} is not a multiple of 128")
    wf = w.detach().float().reshape(N, K // FP4_BLOCK, FP4_BLOCK)
    amax = wf.abs().amax(2)
    if not bool(torch.isfinite(amax).all()):
        raise RuntimeError(f"{who}: the weight holds inf / nan")
    if bool((amax >= 2.0 ** 16).any()):
        raise RuntimeError(f"{who}: a block's largest magnitude is 2^16 or more")
    # floor(log2(amax)) exactly: amax = m 2^e with m in [0.5, 1)
    x = torch.where(amax > 0, torch.frexp(amax).exponent - 3, torch.zeros_like(amax, dtype=torch.int32)).clamp_(FP4_X_MIN, FP4_X_MAX)
    return wf, x


def _fp4_round(v):
    """|v| (fp32, >= 0) to the nearest e2m1 magnitude, ties to the even code, saturating at 6 -> twice that magnitude (0 .. 12)"""
    v = v.clamp(max=6.0)
    return torch.where(v < 2.0, torch.round(v * 2.0), torch.where(v < 4.0, torch.round(v) * 2.0, torch.round(v * 0.5) * 4.0))


def quantize_blocks_fp4(w: torch.Tensor):
    """OCP MXFP4 quantisation of a 2-D weight (N, K) in bf16 / fp16 / fp32, K % 128 == 0 -> (codes uint8 (N, K / 2): e2m1, the
    code of even k in the low nibble; scales uint8 (N, K / 32): e8m0, 2^(e - 127) for 32 consecutive k of a row).  The OCP MX
    rule: per block x = floor(log2(amax)) - 2 (0 for an all-zero block), clamped to [-23, 13] -- where every e2m1 * 2^x is exact
    in fp16 and bf16 alike, so the codes do not depend on the build --, elements w / 2^x rounded to nearest-even on the e2m1 grid
    {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6.  RuntimeError for inf / nan, a block with amax >= 2^16, a weight that is not
    2-D, K % 128 != 0.  Plain torch, any device; not a hot path (the decode route quantises a layer once, prefill.py)."""
    wf, x = _fp4_blocks("quantize_blocks_fp4", w)
    N, nb, _ = wf.shape
    v = torch.ldexp(wf, -x[:, :, None])                     # (exact: a power of two)
    twice = _fp4_round(v.abs()).to(torch.int64)             # 0, 1, 2, 3, 4, 6, 8, 12
    lut = torch.tensor([0, 1, 2, 3, 4, 0, 5, 0, 6, 0, 0, 0, 7], dtype=torch.uint8, device=w.device)
    code = lut[twice]
    code = torch.where((v < 0) & (code != 0), code | 8, code).reshape(N, nb * FP4_BLOCK)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return codes, (x + 127).to(torch.uint8).contiguous()


def dequantize_blocks_fp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 (N, K) = e2m1(code[n][k]) * 2^(scale[n][k / 32] - 127): what the e2m1 products multiply by, exactly."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2 or \
            codes.shape[0] != scales.shape[0] or codes.shape[1] * 2 != scales.shape[1] * FP4_BLOCK:
        raise RuntimeError(f"dequantize_blocks_fp4: expected uint8 codes (N, K / 2) and scales (N, K / 32), got "
                           f"{tuple(codes.shape)} {codes.dtype}, {tuple(scales.shape)} {scales.dtype}")
    N = codes.shape[0]
    code = torch.stack((codes & 15, codes >> 4), 2).reshape(N, -1).to(torch.int64)
    grid = torch.tensor(FP4_GRID + tuple(-g for g in FP4_GRID), dtype=torch.float32, device=codes.device)
    x = (scales.to(torch.int32) - 127).repeat_interleave(FP4_BLOCK, 1)
    return torch.ldexp(grid[code], x)


def snap_fp4_(module):
    """In place, for every nn.Linear weight in `module` with in_features % 128 == 0 (or a 2-D tensor): move each block of 32 onto
    values the block quantiser keeps EXACTLY -- e2m1 multiples of the block's 2^x, the block's largest element at +-6 2^x or +-4 2^x
    (where rounding with saturation puts it: amax / 2^x lies in [4, 8) unless x was clamped from below), so that quantize_blocks_fp4 finds that same x.  Then
    dequantize_blocks_fp4(*quantize_blocks_fp4(w)) == w bit for bit, and w is exact in bf16 and in fp16: a model with snapped
    weights and its e2m1 decode step compute the same function.  Other weights stay as they are.  For tests and the A/B tool."""
    ws = [module] if torch.is_tensor(module) else [m.weight.data for m in module.modules() if isinstance(m, torch.nn.Linear)]
    for w in ws:
        if w.dim() != 2 or w.shape[1] % 128:
            continue
        wf, x = _fp4_blocks("snap_fp4_", w)
        v = torch.ldexp(wf, -x[:, :, None])
        q = torch.copysign(_fp4_round(v.abs()) * 0.5, v)
        # the largest element: rounding with saturation puts it at 4 or 6 already, except in a block whose x was clamped from below
        top = v.abs().argmax(2, keepdim=True)
        vt = v.gather(2, top)
        q.scatter_(2, top, torch.where(vt == 0, vt, torch.copysign(torch.where(vt.abs() > 5.0, 6.0, 4.0), vt)))
        w.copy_(torch.ldexp(q, x[:, :, None]).reshape(w.shape).to(w.dtype))
    return module


def _rows_call(export, a, w_ops, ldw, N, bias, residual, out_f32, swiglu, out):
    """What gemm_rows, gemm_rows_w8 and gemm_rows_w4 share: A as (M, K) rows with unit column stride, `out`, the flags, the residual
    and its row stride, then the call of `export` (a u2tok_gemm_rows* name, or a function of M that gives one) for a weight of N
    rows with the form's operands `w_ops` (the weight, then its scales) and leading dimensions `ldw` (ldw, then lds) in their
    places, and its status -> out"""
    who = (export if isinstance(export, str) else export(1))[len("u2tok_"):]   # (the wrapper's name, for its messages)
    h = _lib.load_library()
    _need(a, ELEM, "A")
    a2 = a.reshape(-1, a.shape[-1])
    if a2.stride(1) != 1:
        a2 = a2.contiguous()
    (M, K), cols = a2.shape, N // 2 if swiglu else N
    if out is None:
        out = torch.empty((M, cols), dtype=torch.float32 if out_f32 else elem_dtype(), device=a.device)
    if out.shape != (M, cols) or out.stride(1) != 1 or out.dtype != (torch.float32 if out_f32 else elem_dtype()):
        raise RuntimeError(f"{who}: out must be (M, columns) with unit column stride in the output type")
    flags = GEMM_SWIGLU if swiglu else (GEMM_OUT_F32 if out_f32 else 0)
    ldr = 0
    if bias is not None:
        flags |= GEMM_BIAS_N
        bias = _need(bias, ELEM, "bias").contiguous()
    if residual is not None:
        flags |= GEMM_RESIDUAL
        _need(residual, ELEM, "residual")
        if residual.shape != (M, N) or residual.stride(1) != 1:
            raise RuntimeError(f"{who}: residual must be (M, N) with unit column stride")
        ldr = residual.stride(0)
    name = export if isinstance(export, str) else export(M)
    st = getattr(h, name)(_ptr(a2), *map(_ptr, w_ops), _ptr(out), _ptr(bias), _ptr(residual), M, N, K, a2.stride(0), *ldw,
                          out.stride(0), ldr, flags, _stream())
    _lib.check(st, name)
    return out


@_guarded
def gemm_rows_w8(a: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor, *, bias=None, residual=None, out_f32=False,
                 swiglu=False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(M <= 64, N) = epilogue(scale[n] * a @ e4m3(w8)^T) for w8 (N, K) torch.float8_e4m3fn and scale (N,) fp32
    (u2tok_gemm_rows_w8, for M > 16 u2tok_gemm_rows_w8_wide: the decode step's weight-streaming product on 1-byte weights, fp32
    accumulation; each block of 16 rows has the bits of the M <= 16 product on it).  swiglu: w8 = gate
    rows | up rows -> (M, N / 2) = silu(gate) * up.  `out` / `residual` may be row-strided views (unit column stride)."""
    if w8.dtype != torch.float8_e4m3fn or scale.dtype != torch.float32 or not w8.is_cuda or not scale.is_cuda:
        raise RuntimeError("gemm_rows_w8: expected float8_e4m3fn weights and fp32 scales on the GPU")
    w8, scale = w8.contiguous(), scale.contiguous()
    N, K = w8.shape[0], a.shape[-1]
    if w8.shape[1] != K or scale.numel() != N:
        raise RuntimeError(f"gemm_rows_w8: shapes A {tuple(a.reshape(-1, K).shape)}, W8 {tuple(w8.shape)}, "
                           f"scale {tuple(scale.shape)}")
    return _rows_call(lambda M: "u2tok_gemm_rows_w8_wide" if M > 16 else "u2tok_gemm_rows_w8", a, (w8, scale), (K,), N, bias,
                      residual, out_f32, swiglu, out)


@_guarded
def gemm_rows_w4(a: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, *, bias=None, residual=None, out_f32=False,
                 swiglu=False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(M <= 64, N) = epilogue(a @ dequantize_blocks_fp4(codes, scales)^T) for MXFP4 weights -- codes (N, K / 2) uint8, scales
    (N, K / 32) uint8, K % 128 == 0 (u2tok_gemm_rows_w4: the decode step's weight-streaming product on 4-bit weights, fp32
    accumulation; each block of 16 rows has the bits of the M <= 16 product on it).  swiglu: codes = gate rows | up rows ->
    (M, N / 2) = silu(gate) * up.  `out` / `residual` may be row-strided views (unit column stride)."""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or not codes.is_cuda or not scales.is_cuda:
        raise RuntimeError("gemm_rows_w4: expected uint8 codes and uint8 block scales on the GPU")
    codes, scales = codes.contiguous(), scales.contiguous()
    N, K = codes.shape[0], a.shape[-1]
    if codes.dim() != 2 or scales.shape != (N, K // 32) or codes.shape[1] * 2 != K:
        raise RuntimeError(f"gemm_rows_w4: shapes A {tuple(a.reshape(-1, K).shape)}, codes {tuple(codes.shape)}, "
                           f"scales {tuple(scales.shape)}")
    return _rows_call("u2tok_gemm_rows_w4", a, (codes, scales), (K // 2, K // 32), N, bias, residual, out_f32, swiglu, out)


@_guarded
def gemm_rows(a: torch.Tensor, w: torch.Tensor, *, bias=None, residual=None, out_f32=False, swiglu=False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(M <= 64, N) = epilogue(a @ w^T) for w (N, K) in the element type through the few-rows (weight-streaming) kernels, called
    directly (u2tok_gemm_rows) instead of through the plan of `gemm`: M <= 16 the kernel the plan picks, 16 < M <= 64 the
    multi-block kernel whose every block of 16 rows has the bits of the M <= 16 product on it.  K % 32 == 0.  swiglu: w = gate
    rows | up rows -> (M, N / 2) = silu(gate) * up.  `w`, `out` and `residual` may be row-strided views (unit column stride)."""
    _need(w, ELEM, "W")
    if w.dim() != 2 or w.stride(1) != 1:
        w = w.contiguous()
    if w.shape[1] != a.shape[-1]:
        raise RuntimeError(f"gemm_rows: shapes A {tuple(a.reshape(-1, a.shape[-1]).shape)}, W {tuple(w.shape)}")
    return _rows_call("u2tok_gemm_rows", a, (w,), (w.stride(0),), w.shape[0], bias, residual, out_f32, swiglu, out)


@_guarded
def gemm_rows_norm(a: torch.Tensor, w: torch.Tensor, norm_weight: torch.Tensor, eps: float, ticket: torch.Tensor, *, residual,
                   scale: Optional[torch.Tensor] = None, bias=None, out: Optional[torch.Tensor] = None,
                   out_norm: Optional[torch.Tensor] = None, flags: Optional[int] = None):
    """(Y, Yn): the few-rows product with a residual, Y (M <= 64, N) = a @ W^T (+ bias) + residual, and in the SAME launch Yn =
    rmsnorm(Y, norm_weight, eps) (u2tok_gemm_rows_norm: the workgroup that finishes last norms the rows).  W: (N, K) in the element
    type (scale None), float8_e4m3fn with `scale` (N,) fp32, or uint8 e2m1 codes (N, K / 2) with `scale` (N, K / 32) uint8 block
    scales.  Y has the bits of gemm_rows / gemm_rows_w8 / gemm_rows_w4, Yn those of `rmsnorm(Y)`.  ticket: an int32 / uint32 tensor
    of one element on the GPU that holds 0; it holds 0 again afterwards.  N % 8 == 0, N <= 4096.  flags (tests): the raw epilogue
    flags instead of those the arguments imply."""
    h = _lib.load_library()
    _need(a, ELEM, "A")
    a2 = a.reshape(-1, a.shape[-1])
    if a2.stride(1) != 1:
        a2 = a2.contiguous()
    M, K = a2.shape
    if scale is None:
        _need(w, ELEM, "W")
        wform, ldw, lds = 0, w.stride(0), 0
    elif w.dtype == torch.float8_e4m3fn:
        wform, ldw, lds = 1, K, 0
    else:
        wform, ldw, lds = 2, K // 2, K // 32
    if wform and not (w.is_contiguous() and scale.is_contiguous() and w.is_cuda and scale.is_cuda):
        raise RuntimeError("gemm_rows_norm: codes and scales must be contiguous GPU tensors")
    N = w.shape[0]
    dt = elem_dtype()
    out = torch.empty((M, N), dtype=dt, device=a.device) if out is None else out
    out_norm = torch.empty((M, N), dtype=dt, device=a.device) if out_norm is None else out_norm
    for t, name in ((out, "out"), (out_norm, "out_norm")):
        if t.shape != (M, N) or t.stride(1) != 1 or t.dtype != dt:
            raise RuntimeError(f"gemm_rows_norm: {name} must be (M, N) with unit column stride in the element type")
    if bias is not None:
        bias = _need(bias, ELEM, "bias").contiguous()
    norm_weight = _need(norm_weight, ELEM, "norm_weight").contiguous()
    if flags is None:
        flags = (GEMM_RESIDUAL if residual is not None else 0) | (GEMM_BIAS_N if bias is not None else 0)
    st = h.u2tok_gemm_rows_norm(_ptr(a2), _ptr(w), _ptr(out), _ptr(bias), _ptr(residual), M, N, K, a2.stride(0), ldw, out.stride(0),
                                residual.stride(0) if residual is not None else 0, flags, wform, _ptr(scale), lds, _ptr(norm_weight),
                                float(eps), _ptr(out_norm), out_norm.stride(0), _ptr(ticket), _stream())
    _lib.check(st, "u2tok_gemm_rows_norm")
    return out, out_norm


def head_desc(norm_weight: torch.Tensor, eps: float, w: torch.Tensor, scale: Optional[torch.Tensor] = None):
    """The u2tok_decode_head_desc of a final RMSNorm weight (E,) and an output matrix: w (V, E) in the element type (scale None; it
    may be a row-strided view), float8_e4m3fn with `scale` (V,) fp32, or uint8 e2m1 codes (V, E / 2) with `scale` (V, E / 32) uint8
    block scales -- the operands of gemm_rows, gemm_rows_w8 and gemm_rows_w4.  Holds raw addresses: the caller keeps the tensors."""
    E = norm_weight.numel()
    if scale is None:
        wform, cols, ldw, lds = 0, E, w.stride(0), 0
    elif w.dtype == torch.float8_e4m3fn:
        wform, cols, ldw, lds = 1, E, E, 0
    else:
        wform, cols, ldw, lds = 2, E // 2, E // 2, E // 32
    if w.dim() != 2 or w.shape[1] != cols or w.stride(1) != 1 or not w.is_cuda or not norm_weight.is_contiguous() or (
            wform and not (w.is_contiguous() and scale.is_contiguous() and scale.is_cuda)):
        raise RuntimeError(f"head_desc: expected a (V, E = {E}) output matrix on the GPU -- elements, or contiguous codes and scales --, "
                           f"got {tuple(w.shape)} {w.dtype}")
    return _lib.DecodeHead(w_norm=_ptr(norm_weight), W=_ptr(w), scale=_ptr(scale), E=E, V=w.shape[0], wform=wform, eps=float(eps),
                           ldw=ldw, lds=lds)


@_guarded
def decode_head(x: torch.Tensor, norm_weight: torch.Tensor, eps: float, w: torch.Tensor, scale: Optional[torch.Tensor] = None, *,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The head of a decode step (u2tok_decode_head): fp32 logits (B <= 64, V) = the few-rows product of the head's weight form,
    with fp32 C, on rmsnorm(x, norm_weight, eps) of the UN-NORMED hidden rows x (B, E) -- the bits of `rmsnorm` followed by
    gemm_rows / gemm_rows_w8 / gemm_rows_w4 (..., out_f32=True), in one library call.  w / scale: as `head_desc` takes them.
    `out`: an fp32 (B, V) view with unit column stride (a row-strided one keeps its other columns)."""
    h = _lib.load_library()
    _need(x, ELEM, "x"), _need(norm_weight, ELEM, "norm_weight")
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] != norm_weight.numel():
        raise RuntimeError("decode_head: x must be (B, E) with a contiguous last dim")
    if scale is None:
        _need(w, ELEM, "W")
    desc = head_desc(norm_weight, eps, w, scale)
    B, V = x.shape[0], desc.V
    if out is None:
        out = torch.empty((B, V), dtype=torch.float32, device=x.device)
    if out.shape != (B, V) or out.stride(1) != 1 or out.dtype != torch.float32 or not out.is_cuda:
        raise RuntimeError("decode_head: out must be fp32 (B, V) with unit column stride on the GPU")
    need = h.u2tok_decode_head_workspace_bytes(B, desc.E)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    _lib.check(h.u2tok_decode_head(C.addressof(desc), _ptr(x), x.stride(0), B, _ptr(out), out.stride(0), _ptr(ws), need, _stream()),
               "u2tok_decode_head")
    return out


# ---------------------------------------------------------------------------------- rank-r adapter (LoRA) products
def _segment(t: torch.Tensor, name: str):
    """A 2-D view with unit column stride -> (tensor, element offset 0, row stride): the kernels take a column segment of a packed
    buffer as the view's own address and the buffer's row stride."""
    _need(t, ELEM, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError(f"{name}: expected a 2-D tensor with unit column stride, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


@_guarded
def lora_down(x: torch.Tensor, a: torch.Tensor, alpha: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """U (M, r) = alpha x (M, K) a (r, K)^T (u2tok_lora_down): r in {16, 32, 64}, K % 32 == 0.  x may be a column segment of a wider
    buffer (a row-strided view); a and out likewise row-strided.  Anything the kernel does not take raises."""
    h = _lib.load_library()
    x, a = _segment(x, "x"), _segment(a, "a")
    M, K = x.shape
    r = a.shape[0]
    if a.shape[1] != K:
        raise RuntimeError(f"lora_down: shapes x {tuple(x.shape)}, a {tuple(a.shape)}")
    if out is None:
        out = torch.empty((M, r), dtype=elem_dtype(), device=x.device)
    _segment(out, "out")
    if out.shape != (M, r):
        raise RuntimeError("lora_down: out must be (M, r)")
    st = h.u2tok_lora_down(_ptr(x), 0, x.stride(0), _ptr(a), a.stride(0), _ptr(out), out.stride(0), M, K, r, float(alpha), _stream())
    _lib.check(st, "u2tok_lora_down")
    return out


@_guarded
def lora_up(u: torch.Tensor, w: torch.Tensor, y: Optional[torch.Tensor] = None, alpha: float = 1.0,
            accumulate: bool = False) -> torch.Tensor:
    """y (M, N) = [y +] alpha u (M, r) w (N, r)^T (u2tok_lora_up), in place on `y` -- which may be a column segment of a wider buffer,
    whose other columns are not touched; accumulate: float(y) + the product, rounded once.  y None (accumulate False): a new
    tensor.  r in {16, 32, 64}, N % 16 == 0."""
    h = _lib.load_library()
    u, w = _segment(u, "u"), _segment(w, "w")
    M, r = u.shape
    N = w.shape[0]
    if w.shape[1] != r:
        raise RuntimeError(f"lora_up: shapes u {tuple(u.shape)}, w {tuple(w.shape)}")
    if y is None:
        if accumulate:
            raise RuntimeError("lora_up: accumulate needs y")
        y = torch.empty((M, N), dtype=elem_dtype(), device=u.device)
    _segment(y, "y")
    if y.shape != (M, N):
        raise RuntimeError("lora_up: y must be (M, N)")
    st = h.u2tok_lora_up(_ptr(u), u.stride(0), _ptr(w), w.stride(0), _ptr(y), 0, y.stride(0), M, N, r, float(alpha), int(accumulate),
                         _stream())
    _lib.check(st, "u2tok_lora_up")
    return y


def lora_wgrad_workspace_bytes(M: int, C: int, r: int) -> int:
    """The most u2tok_lora_wgrad uses: one fp32 (r, C) tile per row range, min(ceil(M / 128), 512 // ceil(C / 64)) ranges (0: one)."""
    s = min(-(-M // 128), max(1, 512 // -(-C // 64)))
    return s * r * C * 4 if s > 1 else 0


@_guarded
def lora_wgrad(u: torch.Tensor, x: torch.Tensor, alpha: float = 1.0, out_f32: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """G (r, C) = alpha u (M, r)^T x (M, C), the contraction over the rows (u2tok_lora_wgrad); G in the element type or fp32.  x may
    be a column segment of a wider buffer.  r in {16, 32, 64}, C % 8 == 0."""
    h = _lib.load_library()
    u, x = _segment(u, "u"), _segment(x, "x")
    M, r = u.shape
    C = x.shape[1]
    if x.shape[0] != M:
        raise RuntimeError(f"lora_wgrad: shapes u {tuple(u.shape)}, x {tuple(x.shape)}")
    dt = torch.float32 if out_f32 else elem_dtype()
    if out is None:
        out = torch.empty((r, C), dtype=dt, device=u.device)
    if out.shape != (r, C) or out.stride(1) != 1 or out.dtype != dt:
        raise RuntimeError("lora_wgrad: out must be (r, C) with unit column stride in the output type")
    nb = lora_wgrad_workspace_bytes(M, C, r)
    ws = torch.empty(nb, dtype=torch.uint8, device=u.device) if nb else None
    st = h.u2tok_lora_wgrad(_ptr(u), u.stride(0), _ptr(x), 0, x.stride(0), _ptr(out), out.stride(0), M, C, r, float(alpha),
                            int(out_f32), _ptr(ws), nb, _stream())
    _lib.check(st, "u2tok_lora_wgrad")
    return out


def lora_segs(segs):
    """(A (r, K), B (N, r), col0, scale) tuples -> a ctypes array of u2tok_lora_seg (raw addresses: the caller keeps the tensors)."""
    arr = (_lib.LoraSeg * len(segs))()
    for e, (a, b, col0, scale) in zip(arr, segs):
        if not (a.is_contiguous() and b.is_contiguous()) or a.dim() != 2 or b.dim() != 2 or b.shape[1] != a.shape[0]:
            raise RuntimeError(f"lora_rows: a segment needs contiguous A (r, K) and B (N, r), got {tuple(a.shape)}, {tuple(b.shape)}")
        e.A, e.B, e.r, e.col0, e.N, e.scale = a.data_ptr(), b.data_ptr(), a.shape[0], int(col0), b.shape[0], float(scale)
    return arr


def lora_rows_workspace_bytes(M: int, K: int, segs) -> int:
    """u2tok_lora_rows_workspace_bytes for (A, B, col0, scale) tuples; 0 for a group the call refuses.  No GPU needed."""
    arr = segs if isinstance(segs, C.Array) else lora_segs(segs)
    return int(_lib.load_library().u2tok_lora_rows_workspace_bytes(M, K, C.addressof(arr), len(arr)))


@_guarded
def lora_rows(x: torch.Tensor, segs, y: torch.Tensor, u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The adapter branch of one packed product for M <= 64 rows as a group (u2tok_lora_rows, two launches): for each segment
    (A (r, K), B (N, r), col0, scale) of `segs` (1 .. 3, disjoint columns), u_i = rnd(x A_i^T) and y[:, col0:col0 + N] = rnd(float(y)
    + scale u_i B_i^T) in place.  x (M, K) and y may be row-strided views; returns u (M, sum r_i)."""
    h = _lib.load_library()
    x, y = _segment(x, "x"), _segment(y, "y")
    M, K = x.shape
    for a, b, _, _ in segs:
        _need(a, ELEM, "A"), _need(b, ELEM, "B")
        if a.dim() != 2 or a.shape[1] != K:
            raise RuntimeError(f"lora_rows: shapes x {tuple(x.shape)}, A {tuple(a.shape)}")
    arr = lora_segs(segs)
    rsum = sum(a.shape[0] for a, _, _, _ in segs)
    if u is None:
        u = torch.empty((M, rsum), dtype=elem_dtype(), device=x.device)
    _segment(u, "u")
    if y.shape[0] != M or u.shape != (M, rsum):
        raise RuntimeError("lora_rows: y must have M rows and u be (M, sum r)")
    nb = int(h.u2tok_lora_rows_workspace_bytes(M, K, C.addressof(arr), len(arr)))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=x.device)
    st = h.u2tok_lora_rows(_ptr(x), x.stride(0), C.addressof(arr), len(arr), _ptr(u), u.stride(0), _ptr(y), y.stride(0), M, K, _ptr(ws), nb,
                           _stream())
    _lib.check(st, "u2tok_lora_rows")
    return u


@_guarded
def rope_apply(x: torch.Tensor, n_outer, S, n_inner, H, d, max_len=512, inverse=False):
    h = _lib.load_library()
    _lib.check(h.u2tok_rope_apply(_ptr(x), n_outer, S, n_inner, H, d, x.stride(-2), max_len, int(inverse), _stream()),
               "u2tok_rope_apply")
    return x


# ---------------------------------------------------------------------------------- strided GEMM / backward blocks
@_guarded
def gemm_strided(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, M, N, K, lda, ldb, ldc, nz=1, nbh=1,
                 sAb=0, sAh=0, sBb=0, sBh=0, sCb=0, sCh=0, alpha=1.0, out_f32=False, bias=None, bias_m=False,
                 a_off=0, b_off=0, c_off=0, a_kmajor=False, b_kmajor=False) -> torch.Tensor:
    """C[z] = alpha * A[z] B[z]^T with explicit element strides (z = zb * nbh + zh): the descriptor of u2tok_gemm_bf16.
    a / b / out are the STORAGES (any shape); *_off are element offsets into them.  b_kmajor: B[z] is stored (K, N) with
    row stride ldb; a_kmajor (with b_kmajor): A[z] is stored (K, M) with row stride lda."""
    h = _lib.load_library()
    _need(a, ELEM, "A"), _need(b, ELEM, "B")
    flags = (GEMM_OUT_F32 if out_f32 else 0) | (GEMM_A_KMAJOR if a_kmajor else 0) | (GEMM_B_KMAJOR if b_kmajor else 0)
    if bias is not None:
        flags |= GEMM_BIAS_M if bias_m else GEMM_BIAS_N
    st = h.u2tok_gemm_bf16(a.data_ptr() + 2 * a_off, b.data_ptr() + 2 * b_off,
                           out.data_ptr() + (4 if out_f32 else 2) * c_off, _ptr(bias), None, M, N, K, lda, ldb, ldc, 0,
                           nz, nbh, sAb, sAh, sBb, sBh, sCb, sCh, 0, 0, float(alpha), flags, _stream())
    _lib.check(st, "u2tok_gemm_bf16")
    return out


@_guarded
def gemm_ex(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, M, N, K, lda, ldb, ldc, ldr=0, nz=1, nbh=1, sAb=0, sAh=0,
            sBb=0, sBh=0, sCb=0, sCh=0, sRb=0, sRh=0, alpha=1.0, flags=0, bias=None, residual=None, a_off=0, b_off=0, c_off=0,
            r_off=0, nsplit=0, alpha_lo=1.0, vt: Optional[torch.Tensor] = None, vt_n0=0, vt_rows=0, vt_ld=0, vt_bs=0,
            vt_off=0) -> torch.Tensor:
    """The whole descriptor of u2tok_gemm_bf16_ex on STORAGES (any shape; *_off are element offsets into them): `flags` as the
    header numbers them (bias and residual must come with their flag), columns n < nsplit scaled by alpha_lo instead of alpha,
    and with `vt` the columns n >= vt_n0 of the many-row part written transposed to vt[m // vt_rows][n - vt_n0][perm16(m % vt_rows)]
    instead of C (include/u2tok.h has the conditions; anything else raises).  The neutral values give u2tok_gemm_bf16's bits."""
    h = _lib.load_library()
    _need(a, ELEM, "A"), _need(b, ELEM, "B")
    if vt is not None:
        _need(vt, ELEM, "vt")
    if (bias is not None) != bool(flags & (GEMM_BIAS_N | GEMM_BIAS_M)) or (residual is not None) != bool(flags & GEMM_RESIDUAL):
        raise RuntimeError("gemm_ex: bias / residual and their flags do not agree")
    es = a.element_size()
    st = h.u2tok_gemm_bf16_ex(a.data_ptr() + es * a_off, b.data_ptr() + es * b_off, out.data_ptr() + out.element_size() * c_off,
                              _ptr(bias), None if residual is None else residual.data_ptr() + es * r_off, M, N, K, lda, ldb, ldc,
                              ldr, nz, nbh, sAb, sAh, sBb, sBh, sCb, sCh, sRb, sRh, float(alpha), int(flags), int(nsplit),
                              float(alpha_lo), None if vt is None else vt.data_ptr() + es * vt_off, vt_n0, vt_rows, vt_ld, vt_bs,
                              _stream())
    _lib.check(st, "u2tok_gemm_bf16_ex")
    return out


@_guarded
def transpose_ex(x: torch.Tensor, nz: int, R: int, Cc: int, ld_in: int, in_zs: int, ld_out: int = None,
                 x_off: int = 0) -> torch.Tensor:
    """out[z][c][r] = x[z][r][c] for a strided source (row stride ld_in, batch stride in_zs, elements); out is dense
    (nz, Cc, ld_out) with ld_out = R rounded up to 8, padding zeroed."""
    h = _lib.load_library()
    ld_out = ld_out or (R + 7) // 8 * 8
    y = torch.empty((nz, Cc, ld_out), dtype=elem_dtype(), device=x.device)
    _lib.check(h.u2tok_transpose_bf16(x.data_ptr() + 2 * x_off, _ptr(y), nz, R, Cc, ld_in, ld_out, in_zs, Cc * ld_out, 0,
                                      _stream()), "u2tok_transpose_bf16")
    return y


@_guarded
def gelu_fwd(z: torch.Tensor) -> torch.Tensor:
    h = _lib.load_library()
    z = _need(z, ELEM, "z").contiguous()
    y = torch.empty_like(z)
    _lib.check(h.u2tok_gelu_fwd(_ptr(z), _ptr(y), z.numel(), _stream()), "u2tok_gelu_fwd")
    return y


@_guarded
def gelu_bwd(z: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    h = _lib.load_library()
    z, dy = _need(z, ELEM, "z").contiguous(), _need(dy, ELEM, "dy").contiguous()
    dz = torch.empty_like(z)
    _lib.check(h.u2tok_gelu_bwd(_ptr(z), _ptr(dy), _ptr(dz), z.numel(), _stream()), "u2tok_gelu_bwd")
    return dz


@_guarded
def colsum(x: torch.Tensor, y: Optional[torch.Tensor] = None, out_dtype=None) -> torch.Tensor:
    """sum over rows of x (* y): x (rows, C) 16-bit elements -> (C,) in out_dtype (the element type of the guarded call by default,
    or fp32); fp32 accumulation, fixed order."""
    h = _lib.load_library()
    out_dtype = out_dtype or elem_dtype()   # (resolved per call: the f16 build writes IEEE-half bits -- ADVICE r5)
    x = _need(x, ELEM, "x").contiguous()
    rows, Cc = x.shape
    if y is not None:
        y = _need(y, ELEM, "y").contiguous()
    ws = torch.empty(h.u2tok_colsum_workspace_bytes(rows, Cc), dtype=torch.uint8, device=x.device)
    out = torch.empty(Cc, dtype=out_dtype, device=x.device)
    f32 = out_dtype == torch.float32
    _lib.check(h.u2tok_colsum_bf16(_ptr(x), _ptr(y), _ptr(out) if f32 else None, None if f32 else _ptr(out), rows, Cc, Cc,
                                   Cc, _ptr(ws), 0, _stream()), "u2tok_colsum_bf16")
    return out


@_guarded
def layernorm_bwd(x: torch.Tensor, residual: Optional[torch.Tensor], w: torch.Tensor, dy: torch.Tensor, eps=1e-5):
    """-> (dv bf16 like x, dw fp32 (C,), db fp32 (C,)) for y = LN(x (+ residual)) * w + b."""
    h = _lib.load_library()
    x, dy = _need(x, ELEM, "x").contiguous(), _need(dy, ELEM, "dy").contiguous()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    if residual is not None:
        residual = residual.contiguous()
    dv = torch.empty_like(x)
    dw = torch.empty(Cc, dtype=torch.float32, device=x.device)
    db = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = torch.empty(h.u2tok_layernorm_bwd_workspace_bytes(rows, Cc), dtype=torch.uint8, device=x.device)
    _lib.check(h.u2tok_layernorm_bwd(_ptr(x), _ptr(residual), _ptr(w), _ptr(dy), _ptr(dv), _ptr(dw), _ptr(db), rows, Cc,
                                     float(eps), _ptr(ws), 0, _stream()), "u2tok_layernorm_bwd")
    return dv, dw, db


@_guarded
def softmax_bwd(p: torch.Tensor, dp: torch.Tensor, n: int) -> torch.Tensor:
    """p: (..., ldp) bf16 probabilities (pad columns >= n), dp: (..., lddp) fp32 -> dS (..., ldp) bf16."""
    h = _lib.load_library()
    p, dp = _need(p, ELEM, "P").contiguous(), _need(dp, torch.float32, "dP").contiguous()
    ldp, lddp = p.shape[-1], dp.shape[-1]
    ds = torch.empty_like(p)
    _lib.check(h.u2tok_softmax_bwd(_ptr(p), _ptr(dp), _ptr(ds), p.numel() // ldp, n, ldp, lddp, _stream()),
               "u2tok_softmax_bwd")
    return ds


@_guarded
def relbias_grad(ds: torch.Tensor, dtable: torch.Tensor, S: int, H: int, max_len: int) -> None:
    """ds: (nz, S, ldp) bf16; dtable: (2 * max_len - 1, H) fp32, accumulated into."""
    h = _lib.load_library()
    ds = _need(ds, ELEM, "dS").contiguous()
    _need(dtable, torch.float32, "dtable")
    nz = ds.numel() // (S * ds.shape[-1])
    _lib.check(h.u2tok_relbias_grad(_ptr(ds), _ptr(dtable), nz, S, H, ds.shape[-1], max_len, _stream()),
               "u2tok_relbias_grad")


@_guarded
def adamw_step(master: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, grad: torch.Tensor, out_bf16: torch.Tensor,
               step: int, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, grad_coef: Optional[torch.Tensor] = None,
               group: Optional[torch.Tensor] = None) -> None:
    """One rank's shard of a ZeRO-1 AdamW step in ONE kernel (u2tok_adamw_step): fp32 master / moments in place, bf16 gradient
    piece in, bf16 parameter piece out.  lr / weight_decay: floats, or per-group sequences with `group` (uint8 per element)."""
    h = _lib.load_library()
    n = master.numel()
    for t, dt, name in ((master, torch.float32, "master"), (exp_avg, torch.float32, "exp_avg"),
                        (exp_avg_sq, torch.float32, "exp_avg_sq"), (grad, torch.bfloat16, "grad"), (out_bf16, torch.bfloat16, "out")):
        _need(t, dt, name)
        if t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"adamw_step: {name} must be contiguous with {n} elements")
    lrs = [float(x) for x in (lr if isinstance(lr, (list, tuple)) else [lr])]
    wds = [float(x) for x in (weight_decay if isinstance(weight_decay, (list, tuple)) else [weight_decay])]
    if len(lrs) != len(wds) or len(lrs) > 8:
        raise RuntimeError("adamw_step: lr / weight_decay must list the same <= 8 parameter groups")
    if group is not None:
        _need(group, torch.uint8, "group")
    _lib.check(h.u2tok_adamw_step(_ptr(master), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(grad), _ptr(group), _ptr(out_bf16), n,
                                  (C.c_float * len(lrs))(*lrs), (C.c_float * len(wds))(*wds), len(lrs), float(betas[0]),
                                  float(betas[1]), float(eps), int(step), float(grad_scale), _ptr(grad_coef), _stream()),
               "u2tok_adamw_step")


# ---------------------------------------------------------------------------------- pipelines
class _Workspace:
    """Grow-only uint8 HBM scratch owned by the calling module: one buffer per (module instance, HIP stream), so
    calls issued on different streams (two volumes in flight on one GPU) never share scratch."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


def weight_table(tensors) -> "C.Array":
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        if t is None:
            arr[i] = None
            continue
        if not t.is_cuda or t.dtype != elem_dtype() or not t.is_contiguous():
            raise RuntimeError(f"u2tok HIP path needs contiguous {elem_dtype()} parameters on the GPU, all of one 16-bit type "
                               f"(got {t.dtype} on {t.device}); call model.to(torch.bfloat16).cuda() or model.half().cuda()")
        arr[i] = t.data_ptr()
    return arr


# ---------------------------------------------------------------------------------- decoder training route (decoder_train.py)
@_guarded
def attention_gqa_ex(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, kv_heads: int, scale: float,
                     kv_len: Optional[torch.Tensor] = None, with_lse: bool = False, causal: bool = True):
    """attention_gqa with per-sequence key lengths (u2tok_attention_gqa_ex): key j of sequence b is visible only if
    j < kv_len[b] (int32 (nb,) on the GPU, >= 1; None: all).  with_lse: also returns the row statistics the backward reuses,
    (nb * heads, Sq) fp32 in log2 units -> (out, lse | None)."""
    h = _lib.load_library()
    out, args = _attn_call("attention_gqa_ex", q, k, v, heads, kv_heads, scale, kv_len=kv_len)
    nb, Sq, _ = out.shape
    lse = torch.empty((nb * heads, Sq), dtype=torch.float32, device=q.device) if with_lse else None
    _lib.check(h.u2tok_attention_gqa_ex(*args, int(bool(causal)), _ptr(kv_len), _ptr(lse), Sq if with_lse else 0, _stream()),
               "u2tok_attention_gqa_ex")
    return out, lse


@_guarded
def attention_gqa_range(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, kv_heads: int, scale: float,
                        kv_start: Optional[torch.Tensor] = None, kv_len: Optional[torch.Tensor] = None,
                        causal: bool = True) -> torch.Tensor:
    """attention_gqa with a key range per sequence (u2tok_attention_gqa_range): key j of sequence b is visible iff
    kv_start[b] <= j < kv_len[b] (int32 (nb,) on the GPU each; None: 0 / all keys) and, when causal, j <= i + Skv - Sq -- the mask
    of a left-padded (kv_start) or right-padded (kv_len) batch.  A query row that sees no key gets zeros.  Both None: the
    kernel, and the bits, of attention_gqa."""
    h = _lib.load_library()
    out, args = _attn_call("attention_gqa_range", q, k, v, heads, kv_heads, scale, kv_start, kv_len)
    _lib.check(h.u2tok_attention_gqa_range(*args, int(bool(causal)), _ptr(kv_start), _ptr(kv_len), None, 0, _stream()),
               "u2tok_attention_gqa_range")
    return out


@_guarded
def attention_gqa_band(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, kv_heads: int, scale: float,
                       window: Optional[int] = None, kv_start: Optional[torch.Tensor] = None,
                       kv_len: Optional[torch.Tensor] = None, causal: bool = True) -> torch.Tensor:
    """attention_gqa_range reading K / V where a KV cache keeps them, with an attention window (u2tok_attention_gqa_band).
    k / v: (nb, Skv, kv_heads * d) views as there, or 4-D (B, kv_heads, T, d) cache views -- dense, or [:, :, :T] of larger
    (B, kv_heads, cap, d) buffers: stride(3) == 1, stride(2) == d, stride(0) == kv_heads * stride(1), equal strides for both;
    nothing is copied.  window = W (causal only; None / 0: none): key j is visible to query i iff
    i + Skv - Sq - W < j <= i + Skv - Sq -- W keys, the query's own included --, intersected with the key range.  A query row that
    sees no key gets zeros.  d in {64, 96, 128} for a window or a 4-D view.  No window, 3-D views: the kernel, and the bits, of
    attention_gqa_range (no range either: of attention_gqa)."""
    h = _lib.load_library()
    d = q.shape[-1] // heads
    cache, khs = None, d
    if k.dim() == 4:
        if v.shape != k.shape or v.stride() != k.stride() or k.stride(3) != 1 or k.stride(2) != d \
                or k.stride(0) != kv_heads * k.stride(1):
            raise RuntimeError(f"attention_gqa_band: k / v {tuple(k.shape)} strides {k.stride()}, {v.stride()} must be equal "
                               "(B, kv_heads, T, d) views of (B, kv_heads, cap, d) buffers")
        cache, khs = (k.shape[2], d, k.stride(0)), k.stride(1)
    W = int(window or 0)
    if W < 0 or (W and not causal):
        raise RuntimeError(f"attention_gqa_band: window {window}" + ("" if causal else " without the causal mask"))
    out, args = _attn_call("attention_gqa_band", q, k, v, heads, kv_heads, scale, kv_start, kv_len, cache)
    _lib.check(h.u2tok_attention_gqa_band(*args, int(bool(causal)), _ptr(kv_start), _ptr(kv_len), None, 0, khs, khs, W, _stream()),
               "u2tok_attention_gqa_band")
    return out


@_guarded
def decode_attention(q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, heads: int, kv_heads: int, scale: float,
                     kv_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decode step's attention for a whole batch in one launch (u2tok_decode_attention): q (B, heads * d) rows (unit
    stride inside a row), K / V (B, kv_heads, T, d) -- dense, or views [:, :, :T] of larger (B, kv_heads, cap, d) buffers --,
    kv_start int32 (B,) on the GPU or None: query b attends over keys kv_start[b] .. T - 1.  d in {64, 96, 128},
    heads / kv_heads <= 16.  -> (B, heads * d)."""
    h = _lib.load_library()
    for t, n in ((q, "q"), (K, "K"), (V, "V")):
        _need(t, ELEM, n)
    if q.dim() != 2 or q.stride(1) != 1 or K.dim() != 4 or V.shape != K.shape or V.stride() != K.stride():
        raise RuntimeError(f"decode_attention: q {tuple(q.shape)} must be (B, heads * d) rows, K / V equal (B, kv_heads, T, d) views")
    B, Eq = q.shape
    d = Eq // heads
    T = K.shape[2]
    kvs = K.stride(1) if kv_heads > 1 else K.stride(0) if B > 1 else T * d      # elements between (batch, kv head) entries
    if Eq % heads or heads % kv_heads or K.shape != (B, kv_heads, T, d) or K.stride(3) != 1 or K.stride(2) != d \
            or (B > 1 and K.stride(0) != kv_heads * kvs):
        raise RuntimeError(f"decode_attention: shapes {tuple(q.shape)}, {tuple(K.shape)} / strides {K.stride()}, heads {heads}/{kv_heads}")
    kv_start = _kv_len_arg(kv_start, B, q.device)
    out = torch.empty((B, Eq), dtype=elem_dtype(), device=q.device)
    nbytes = h.u2tok_decode_attention_workspace_bytes(B, heads, kv_heads, T, d)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    _lib.check(h.u2tok_decode_attention(_ptr(q), _ptr(K), _ptr(V), _ptr(out), B, heads, kv_heads, T, d, q.stride(0),
                                        kvs, Eq, float(scale), _ptr(kv_start),
                                        _ptr(ws) if nbytes else None, nbytes, _stream()), "u2tok_decode_attention")
    return out


# ---------------------------------------------------------------------------------------------- FP8 (e4m3) KV cache
def quantize_kv_fp8(x: torch.Tensor):
    """The KV cache's e4m3 form, the reference (plain torch, any device): x (..., D) keys or values in bf16 / fp16 / fp32 ->
    (codes (..., D) torch.float8_e4m3fn, scales (...) fp32).  One row = the last dimension (the D values of one (sequence, kv head,
    position)): scale = amax / 448 in fp32 (1.0 for an all-zero row), codes = e4m3(clamp(x_fp32 / scale, +-448)), round to nearest
    even -- `quantize_rows_fp8`'s rule per cache row; the NaN codes never occur.  Finite inputs only: a non-finite row gives
    unspecified codes (nothing is checked: no synchronisation)."""
    xf = x.detach().float()
    amax = xf.abs().amax(-1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    codes = (xf / scale[..., None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return codes, scale


def dequantize_kv_fp8(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """code x scale -- exact in fp32 and fp64 (a 4-bit significand times a 24-bit one), rounded once for a 16-bit `dtype`.  codes:
    torch.float8_e4m3fn or the same bytes as uint8."""
    if codes.dtype == torch.uint8:
        codes = codes.view(torch.float8_e4m3fn)
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    return (codes.to(wide) * scales.to(wide)[..., None]).to(dtype)


def _kv8_buffers(who: str, kc, vc, ks, vs):
    B, Hkv, cap, D = kc.shape
    for t, dt, shape in ((kc, torch.uint8, (B, Hkv, cap, D)), (vc, torch.uint8, (B, Hkv, cap, D)), (ks, torch.float32, (B, Hkv, cap)),
                         (vs, torch.float32, (B, Hkv, cap))):
        if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{who}: code buffers (B, Hkv, capacity, D) uint8 and scale buffers (B, Hkv, capacity) fp32, dense, on "
                               f"the GPU; got {tuple(t.shape)} {t.dtype}")
    return B, Hkv, cap, D


@_guarded
def kv_quantize_rows(k: torch.Tensor, v: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor,
                     s_off: int) -> None:
    """The quantising append (u2tok_kv_quantize_rows): k / v (B, Hkv, n, D) in the element type, unit stride inside a row, any
    other strides that are multiples of 8 -> codes and scales at positions s_off .. s_off + n - 1 of the dense buffers, with the
    bits of `quantize_kv_fp8`."""
    h = _lib.load_library()
    _need(k, ELEM, "k"), _need(v, ELEM, "v")
    B, Hkv, cap, D = _kv8_buffers("kv_quantize_rows", kc, vc, ks, vs)
    if k.dim() != 4 or k.shape != v.shape or tuple(k.shape[:2]) != (B, Hkv) or k.shape[3] != D or k.stride(3) != 1 or v.stride(3) != 1:
        raise RuntimeError(f"kv_quantize_rows: k / v {tuple(k.shape)} / {tuple(v.shape)} against buffers {tuple(kc.shape)}")
    _lib.check(h.u2tok_kv_quantize_rows(_ptr(k), _ptr(v), B, Hkv, k.shape[2], D, k.stride(0), k.stride(1), k.stride(2), v.stride(0),
                                        v.stride(1), v.stride(2), _ptr(kc), _ptr(vc), _ptr(ks), _ptr(vs), cap, int(s_off), _stream()),
               "u2tok_kv_quantize_rows")


@_guarded
def qk_norm_rope_kv8(qkv: torch.Tensor, q_norm_w, k_norm_w, cos: torch.Tensor, sin: torch.Tensor, heads: int, kv_heads: int,
                     head_dim: int, eps: float, kc: torch.Tensor, vc: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor, S: int,
                     s_off: int) -> torch.Tensor:
    """`qk_norm_rope` with the quantising append in the same launch (u2tok_qk_norm_rope_kv8): in place on the q and k heads of qkv
    (B S, (heads + 2 kv_heads) * head_dim); the finished k heads and the v heads go to positions s_off .. s_off + S - 1 of the dense
    buffers as codes and scales, with the bits of `qk_norm_rope(..., kv_cache_seq=S)` followed by `kv_quantize_rows`.  Room in the
    buffers is the library's to refuse."""
    h = _lib.load_library()
    _need(qkv, ELEM, "qkv")
    B, Hkv, cap, D = _kv8_buffers("qk_norm_rope_kv8", kc, vc, ks, vs)
    rows = qkv.shape[0]
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] != (heads + 2 * kv_heads) * head_dim or (Hkv, D) != (kv_heads, head_dim) \
            or S <= 0 or rows != B * S:
        raise RuntimeError(f"qk_norm_rope_kv8: qkv {tuple(qkv.shape)} against buffers {tuple(kc.shape)}, S {S}")
    if cos.dtype != sin.dtype or cos.dtype not in (torch.float32, elem_dtype()) or cos.shape != (rows, head_dim) \
            or sin.shape != cos.shape or cos.stride(1) != 1 or sin.stride(1) != 1 or cos.stride(0) != sin.stride(0):
        raise RuntimeError("qk_norm_rope_kv8: cos / sin must be (rows, head_dim) fp32 or bf16 with equal strides")
    _lib.check(h.u2tok_qk_norm_rope_kv8(_ptr(qkv), _ptr(q_norm_w), _ptr(k_norm_w), _ptr(cos), _ptr(sin), int(cos.dtype == torch.float32),
                                        rows, heads, kv_heads, head_dim, qkv.stride(0), cos.stride(0), float(eps), _ptr(kc), _ptr(vc),
                                        _ptr(ks), _ptr(vs), int(S), cap, int(s_off), _stream()), "u2tok_qk_norm_rope_kv8")
    return qkv


@_guarded
def decode_attention_kv8(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor, T: int, heads: int,
                         scale: float, kv_start: Optional[torch.Tensor] = None, k_first: int = 0) -> torch.Tensor:
    """`decode_attention` over an e4m3 cache (u2tok_decode_attention_kv8): q (B, heads * d) rows in the element type; kc / vc
    (B, kv_heads, capacity, d) uint8 codes and ks / vs (B, kv_heads, capacity) fp32 scales, dense buffers of which positions k_first
    .. k_first + T - 1 are attended over (kv_start int32 (B,) counts from k_first).  -> (B, heads * d)."""
    h = _lib.load_library()
    _need(q, ELEM, "q")
    B, Hkv, cap, d = _kv8_buffers("decode_attention_kv8", kc, vc, ks, vs)
    if q.dim() != 2 or q.stride(1) != 1 or q.shape != (B, heads * d) or heads % Hkv or k_first < 0 or T < 1 or k_first + T > cap:
        raise RuntimeError(f"decode_attention_kv8: q {tuple(q.shape)}, buffers {tuple(kc.shape)}, heads {heads}, T {T}, k_first {k_first}")
    kv_start = _kv_len_arg(kv_start, B, q.device)
    out = torch.empty((B, heads * d), dtype=elem_dtype(), device=q.device)
    nbytes = h.u2tok_decode_attention_kv8_workspace_bytes(B, heads, Hkv, T, d)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    _lib.check(h.u2tok_decode_attention_kv8(_ptr(q), _ptr(kc) + k_first * d, _ptr(vc) + k_first * d, _ptr(ks) + 4 * k_first,
                                            _ptr(vs) + 4 * k_first, _ptr(out), B, heads, Hkv, T, d, q.stride(0), cap * d, cap,
                                            heads * d, float(scale), _ptr(kv_start), _ptr(ws) if nbytes else None, nbytes, _stream()),
               "u2tok_decode_attention_kv8")
    return out


@_guarded
def attention_kv8_rows(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, ks: torch.Tensor, vs: torch.Tensor, T: int, heads: int,
                       scale: float, window: Optional[int] = None, kv_start: Optional[torch.Tensor] = None,
                       k_first: int = 0) -> torch.Tensor:
    """`decode_attention_kv8` for Sq >= 1 new positions per sequence (u2tok_attention_kv8_rows: the continued prefill on an e4m3
    cache): q (B, Sq, heads * d) in the element type -- unit stride inside a row, one stride between the B Sq rows (the q columns
    of packed q|k|v rows qualify) --, buffers as there, of which positions k_first .. k_first + T - 1 are attended over, the Sq new
    ones last: row i sees key j (counted from k_first) iff kv_start[b] <= j <= i + T - Sq and, with a window W, j > i + T - Sq - W.
    -> (B, Sq, heads * d), dense."""
    h = _lib.load_library()
    _need(q, ELEM, "q")
    B, Hkv, cap, d = _kv8_buffers("attention_kv8_rows", kc, vc, ks, vs)
    W = int(window or 0)
    if q.dim() != 3 or q.stride(2) != 1 or tuple(q.shape[::2]) != (B, heads * d) or heads % Hkv or k_first < 0 or q.shape[1] < 1 \
            or T < q.shape[1] or k_first + T > cap or W < 0 or (B > 1 and q.shape[1] > 1 and q.stride(0) != q.shape[1] * q.stride(1)):
        raise RuntimeError(f"attention_kv8_rows: q {tuple(q.shape)} / strides {q.stride()}, buffers {tuple(kc.shape)}, heads {heads}, T {T}, "
                           f"k_first {k_first}, window {window}")
    Sq = q.shape[1]
    kv_start = _kv_len_arg(kv_start, B, q.device)
    out = torch.empty((B, Sq, heads * d), dtype=elem_dtype(), device=q.device)
    nbytes = h.u2tok_attention_kv8_rows_workspace_bytes(B, Sq, heads, Hkv, T, d)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    _lib.check(h.u2tok_attention_kv8_rows(_ptr(q), _ptr(kc) + k_first * d, _ptr(vc) + k_first * d, _ptr(ks) + 4 * k_first,
                                          _ptr(vs) + 4 * k_first, _ptr(out), B, Sq, heads, Hkv, T, d,
                                          q.stride(1) if Sq > 1 else q.stride(0) if B > 1 else heads * d, cap * d, cap, heads * d,
                                          float(scale), W, _ptr(kv_start), _ptr(ws) if nbytes else None, nbytes, _stream()),
               "u2tok_attention_kv8_rows")
    return out


@_guarded
def attention_gqa_bwd(qkv: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, heads: int, kv_heads: int, scale: float,
                      kv_len: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                      d_qkv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal GQA flash backward (u2tok_attention_gqa_bwd): qkv (nb, S, (heads + 2 kv_heads) d) packed q | k | v (after the
    rotary embedding), out / d_out (nb, S, heads * d) -> the packed gradient d_qkv (nb, S, (heads + 2 kv_heads) d): dq | dk | dv
    (written into `d_qkv` if given).  d = 64 or 128, and 96 through u2tok_attention_gqa_bwd_d96; kv_len / lse as
    attention_gqa_ex."""
    h = _lib.load_library()
    _need(qkv, ELEM, "qkv")
    nb, S, W = qkv.shape
    d = W // (heads + 2 * kv_heads)
    if W != (heads + 2 * kv_heads) * d or heads % kv_heads or qkv.stride(2) != 1 or qkv.stride(0) != S * qkv.stride(1):
        raise RuntimeError(f"attention_gqa_bwd: qkv {tuple(qkv.shape)} is not a packed (nb, S, (heads + 2 kv_heads) d) buffer")
    out = _need(out, ELEM, "out").contiguous()
    d_out = _need(d_out, ELEM, "d_out").contiguous()
    if out.shape != (nb, S, heads * d) or d_out.shape != out.shape:
        raise RuntimeError(f"attention_gqa_bwd: out / d_out must be (nb, S, heads * d), got {tuple(out.shape)}, {tuple(d_out.shape)}")
    kv_len = _kv_len_arg(kv_len, nb, qkv.device)
    if lse is not None and (lse.dtype != torch.float32 or lse.shape != (nb * heads, S) or not lse.is_contiguous()):
        raise RuntimeError("attention_gqa_bwd: lse must be the (nb * heads, S) fp32 statistics of attention_gqa_ex")
    if d_qkv is None:
        d_qkv = torch.empty((nb, S, W), dtype=elem_dtype(), device=qkv.device)
    elif d_qkv.shape != (nb, S, W) or not d_qkv.is_contiguous() or d_qkv.dtype != elem_dtype():
        raise RuntimeError("attention_gqa_bwd: d_qkv must be a contiguous tensor shaped like qkv")
    nbytes = h.u2tok_attention_gqa_bwd_workspace_bytes(nb, S, heads)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
    ld, ldo = qkv.stride(1), heads * d
    qp, dp = qkv.data_ptr(), d_qkv.data_ptr()
    es = qkv.element_size()
    views = (qp, qp + heads * d * es, qp + (heads + kv_heads) * d * es, ld, S * ld, _ptr(out), _ptr(d_out), ldo, S * ldo,
             dp, dp + heads * d * es, dp + (heads + kv_heads) * d * es, W, S * W, nb, S, heads, kv_heads)
    rest = (float(scale), _ptr(kv_len), _ptr(lse), S if lse is not None else 0, _ptr(ws), nbytes, _stream())
    if d == 96:
        _lib.check(h.u2tok_attention_gqa_bwd_d96(*views, *rest), "u2tok_attention_gqa_bwd_d96")
    else:
        _lib.check(h.u2tok_attention_gqa_bwd(*views, d, *rest), "u2tok_attention_gqa_bwd")
    return d_qkv


@_guarded
def rmsnorm_bwd(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor, eps: float = 1e-6, d_res: Optional[torch.Tensor] = None):
    """Backward of rmsnorm (u2tok_rmsnorm_bwd): x, dy (rows, C) -> (dx (+ d_res), dw fp32 (C,))."""
    h = _lib.load_library()
    x, dy = _need(x, ELEM, "x").contiguous(), _need(dy, ELEM, "dy").contiguous()
    rows, Cc = x.shape
    if dy.shape != x.shape or (d_res is not None and d_res.shape != x.shape):
        raise RuntimeError("rmsnorm_bwd: x, dy (and d_res) must have the same (rows, C) shape")
    if d_res is not None:
        d_res = _need(d_res, ELEM, "d_res").contiguous()
    dx = torch.empty_like(x)
    dw = torch.empty(Cc, dtype=torch.float32, device=x.device)
    nbytes = h.u2tok_rmsnorm_bwd_workspace_bytes(rows, Cc)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    _lib.check(h.u2tok_rmsnorm_bwd(_ptr(x), _ptr(_need(w, ELEM, "w")), _ptr(dy), _ptr(d_res), _ptr(dx), _ptr(dw), rows, Cc,
                                   float(eps), _ptr(ws), nbytes, 0, _stream()), "u2tok_rmsnorm_bwd")
    return dx, dw


@_guarded
def qk_norm_rope_bwd(d_qkv: torch.Tensor, pre: Optional[torch.Tensor], q_norm_w, k_norm_w, cos: torch.Tensor, sin: torch.Tensor,
                     heads: int, kv_heads: int, head_dim: int, eps: float = 1e-6):
    """Backward of qk_norm_rope, in place on the q / k columns of d_qkv (rows, (heads + 2 kv_heads) head_dim)
    (u2tok_qk_norm_rope_bwd).  pre: the q | k columns before the head norm (rows, >= (heads + kv_heads) head_dim view with a
    contiguous last dim), needed with norm weights.  -> (d_qkv, dwq fp32 | None, dwk fp32 | None)."""
    h = _lib.load_library()
    _need(d_qkv, ELEM, "d_qkv")
    rows = d_qkv.shape[0]
    if d_qkv.dim() != 2 or d_qkv.stride(1) != 1 or d_qkv.shape[1] != (heads + 2 * kv_heads) * head_dim:
        raise RuntimeError("qk_norm_rope_bwd: d_qkv must be (rows, (heads + 2 kv_heads) * head_dim)")
    if cos.dtype != sin.dtype or cos.dtype not in (torch.float32, elem_dtype()) or cos.shape != (rows, head_dim) \
            or sin.shape != cos.shape or cos.stride(1) != 1 or sin.stride(1) != 1 or cos.stride(0) != sin.stride(0):
        raise RuntimeError("qk_norm_rope_bwd: cos / sin must be (rows, head_dim) fp32 or bf16 with equal strides")
    norm = q_norm_w is not None
    dwq = dwk = ws = None
    nbytes = 0
    if norm:
        _need(pre, ELEM, "pre")
        if pre.dim() != 2 or pre.shape[0] != rows or pre.shape[1] < (heads + kv_heads) * head_dim or pre.stride(1) != 1:
            raise RuntimeError("qk_norm_rope_bwd: pre must be (rows, >= (heads + kv_heads) head_dim)")
        dwq = torch.empty(head_dim, dtype=torch.float32, device=d_qkv.device)
        dwk = torch.empty(head_dim, dtype=torch.float32, device=d_qkv.device)
        nbytes = h.u2tok_qk_norm_rope_bwd_workspace_bytes(rows, head_dim)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d_qkv.device)
    _lib.check(h.u2tok_qk_norm_rope_bwd(_ptr(d_qkv), _ptr(pre) if norm else None, _ptr(q_norm_w), _ptr(k_norm_w), _ptr(cos),
                                        _ptr(sin), int(cos.dtype == torch.float32), rows, heads, kv_heads, head_dim,
                                        d_qkv.stride(0), pre.stride(0) if norm else 0, cos.stride(0), float(eps), _ptr(dwq),
                                        _ptr(dwk), _ptr(ws), nbytes, 0, _stream()), "u2tok_qk_norm_rope_bwd")
    return d_qkv, dwq, dwk


@_guarded
def swiglu_bwd(gate_up: torch.Tensor, d_act: torch.Tensor) -> torch.Tensor:
    """Backward of swiglu (u2tok_swiglu_bwd): gate_up (rows, 2 I) pre-activations, d_act (rows, I) -> packed (rows, 2 I)
    [d_gate | d_up]."""
    h = _lib.load_library()
    _need(gate_up, ELEM, "gate_up")
    d_act = _need(d_act, ELEM, "d_act").contiguous()
    rows, two_i = gate_up.shape
    if gate_up.stride(1) != 1 or d_act.shape != (rows, two_i // 2):
        raise RuntimeError("swiglu_bwd: gate_up (rows, 2 I) with a contiguous last dim and d_act (rows, I)")
    dgu = torch.empty((rows, two_i), dtype=elem_dtype(), device=gate_up.device)
    _lib.check(h.u2tok_swiglu_bwd(_ptr(gate_up), _ptr(d_act), _ptr(dgu), rows, two_i // 2, gate_up.stride(0), two_i // 2, two_i,
                                  _stream()), "u2tok_swiglu_bwd")
    return dgu


def _ce_block(z: torch.Tensor, labels: torch.Tensor, who: str):
    _need(z, ELEM, "z")
    if z.dim() != 2 or z.stride(1) != 1:
        raise RuntimeError(f"{who}: z (rows, Vs) with a contiguous last dim")
    if labels.dtype != torch.int64 or labels.shape != (z.shape[0],) or not labels.is_contiguous():
        raise RuntimeError(f"{who}: labels must be a dense int64 (rows,) tensor")
    return z.shape[0], z.shape[1], z.stride(0)


def _ce_f32(t: torch.Tensor, rows: int, name: str) -> torch.Tensor:
    _need(t, torch.float32, name)
    if t.shape != (rows,) or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a dense fp32 ({rows},) tensor")
    return t


@_guarded
def ce_lse_update(z: torch.Tensor, v0: int, labels: torch.Tensor, m: torch.Tensor, l: torch.Tensor, zt: torch.Tensor) -> None:
    """One vocabulary slice of the loss head (u2tok_ce_lse_update): z (rows, Vs) logits of the columns [v0, v0 + Vs) folded into the
    rows' running (m, l) = (max, sum exp(z - m)), updated in place -- m = -inf, l = 0 before the first slice -- and zt = the label's
    logit where this slice holds it.  The row's natural-log sum of exponentials is m + log(l) after the last slice."""
    h = _lib.load_library()
    rows, Vs, ldz = _ce_block(z, labels, "ce_lse_update")
    _lib.check(h.u2tok_ce_lse_update(_ptr(z), ldz, rows, Vs, int(v0), _ptr(labels), _ptr(_ce_f32(m, rows, "m")),
                                     _ptr(_ce_f32(l, rows, "l")), _ptr(_ce_f32(zt, rows, "zt")), _stream()), "u2tok_ce_lse_update")


@_guarded
def ce_stats_update(z: torch.Tensor, v0: int, labels: torch.Tensor, m: torch.Tensor, l: torch.Tensor, zt: torch.Tensor,
                    amax: Optional[torch.Tensor] = None, aidx: Optional[torch.Tensor] = None, zsum: Optional[torch.Tensor] = None,
                    l2: Optional[torch.Tensor] = None) -> None:
    """ce_lse_update with further per-row running statistics folded into the same read of the slice (u2tok_ce_stats_update), each
    optional: (amax, aidx) fp32 / int64 (rows,), together -- the maximum logit and the first global column that holds it, -inf and
    INT64_MAX before the first slice; zsum -- the sum of the logits, 0 before; l2 -- sum exp(2 (z - m)) against the same running
    maximum, 0 before (log sum exp(2 z) = 2 m + log(l2) after the last slice).  m, l, zt come out bit-equal to ce_lse_update's."""
    h = _lib.load_library()
    rows, Vs, ldz = _ce_block(z, labels, "ce_stats_update")
    if (amax is None) != (aidx is None):
        raise RuntimeError("ce_stats_update: amax and aidx go together")
    if aidx is not None:
        _need(aidx, torch.int64, "aidx")
        if aidx.shape != (rows,) or not aidx.is_contiguous():
            raise RuntimeError(f"aidx: expected a dense int64 ({rows},) tensor")
    opt = [None if t is None else _ptr(_ce_f32(t, rows, name)) for t, name in ((amax, "amax"), (zsum, "zsum"), (l2, "l2"))]
    _lib.check(h.u2tok_ce_stats_update(_ptr(z), ldz, rows, Vs, int(v0), _ptr(labels), _ptr(_ce_f32(m, rows, "m")),
                                       _ptr(_ce_f32(l, rows, "l")), _ptr(_ce_f32(zt, rows, "zt")), opt[0],
                                       None if aidx is None else _ptr(aidx), opt[1], opt[2], _stream()), "u2tok_ce_stats_update")


@_guarded
def ce_grad_inplace(z: torch.Tensor, v0: int, labels: torch.Tensor, lse: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """z[r][j] <- coef[r] (exp(z[r][j] - lse[r]) - [v0 + j == labels[r]]) rounded to the element type, in place
    (u2tok_ce_grad_inplace; lse: natural log).  Returns z."""
    h = _lib.load_library()
    rows, Vs, ldz = _ce_block(z, labels, "ce_grad_inplace")
    _lib.check(h.u2tok_ce_grad_inplace(_ptr(z), ldz, rows, Vs, int(v0), _ptr(labels), _ptr(_ce_f32(lse, rows, "lse")),
                                       _ptr(_ce_f32(coef, rows, "coef")), _stream()), "u2tok_ce_grad_inplace")
    return z


@_guarded(infer=False)
def sample_warp(scores: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, min_keep: int = 1,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Temperature, top-k and top-p filtering of fp32 logits in one launch (u2tok_sample_warp; include/u2tok.h states the
    semantics): scores (rows, V) fp32 with unit stride in the last dimension, V >= 2; top_k = 0 / top_p = 1 switch that stage
    off.  -> out (rows, V) fp32: scores / temperature where kept, -inf elsewhere; `out` may be `scores` itself."""
    h = _lib.load_library()
    _need(scores, torch.float32, "scores")
    if scores.dim() != 2 or scores.stride(1) != 1 or scores.shape[0] < 1 or scores.shape[1] < 2:
        raise RuntimeError(f"sample_warp: scores must be (rows >= 1, V >= 2) with a contiguous last dim, got {tuple(scores.shape)}")
    rows, V = scores.shape
    if out is None:
        out = torch.empty((rows, V), dtype=torch.float32, device=scores.device)
    else:
        _need(out, torch.float32, "out")
        if out.shape != scores.shape or out.stride(1) != 1 or out.device != scores.device:
            raise RuntimeError("sample_warp: out must be an fp32 (rows, V) tensor on the scores' device with a contiguous last dim")
    nbytes = h.u2tok_sample_warp_workspace_bytes(rows, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
    _lib.check(h.u2tok_sample_warp(_ptr(scores), scores.stride(0) if rows > 1 else V, _ptr(out), out.stride(0) if rows > 1 else V,
                                   rows, V, float(temperature), int(top_k), float(top_p), int(min_keep), _ptr(ws), nbytes,
                                   _stream()), "u2tok_sample_warp")
    return out


@_guarded(infer=False)
def sample_warp_split(scores: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, min_keep: int = 1,
                      out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`sample_warp` with every row spread over several workgroups and one launch per pass of the descent (u2tok_sample_warp_split):
    the same arguments, `out` bit-equal to sample_warp's; for calls of a few rows.  workspace: a uint8 tensor of at least
    u2tok_sample_warp_split_workspace_bytes(rows, V) bytes to use instead of a fresh one (its contents do not matter; afterwards
    its first 32 bytes per row are the row's record)."""
    h = _lib.load_library()
    _need(scores, torch.float32, "scores")
    if scores.dim() != 2 or scores.stride(1) != 1 or scores.shape[0] < 1 or scores.shape[1] < 2:
        raise RuntimeError(f"sample_warp_split: scores must be (rows >= 1, V >= 2) with a contiguous last dim, got {tuple(scores.shape)}")
    rows, V = scores.shape
    if out is None:
        out = torch.empty((rows, V), dtype=torch.float32, device=scores.device)
    else:
        _need(out, torch.float32, "out")
        if out.shape != scores.shape or out.stride(1) != 1 or out.device != scores.device:
            raise RuntimeError("sample_warp_split: out must be an fp32 (rows, V) tensor on the scores' device with a contiguous last dim")
    nbytes = h.u2tok_sample_warp_split_workspace_bytes(rows, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device) if workspace is None else workspace
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != scores.device or ws.numel() < nbytes:
        raise RuntimeError(f"sample_warp_split: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on the scores' device")
    _lib.check(h.u2tok_sample_warp_split(_ptr(scores), scores.stride(0) if rows > 1 else V, _ptr(out), out.stride(0) if rows > 1 else V,
                                         rows, V, float(temperature), int(top_k), float(top_p), int(min_keep), _ptr(ws), ws.numel(),
                                         _stream()), "u2tok_sample_warp_split")
    return out
