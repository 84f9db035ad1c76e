"""GPU: the few-rows adapter group product (u2tok_lora_rows; csrc/lora_rows.hip) element by element against float64 under the
bounds of tests/test_lora_rows_host.py (which shows on the host that an emulation of the kernels' slice-ordered sums stays inside them
on exactly these cases and inputs): u under U |ref| + K u sum |x a|, then y under the up bound evaluated on the GPU's own u.  Row
counts 1 .. 64 on and next to the 16-row block, contractions of one step, of uneven slices (33 steps) and of 16 slices, all three
ranks and a group of mixed ranks, column counts that leave a half-filled 64-column unit, groups of one to three segments with and
without gaps, padded row strides.  Every element of U and Y that the call may not write -- columns outside the segments, pads, rows
>= M, guard tails -- holds a NaN canary that is compared as integers afterwards.  Repeats are bit-equal, and a block of 16 rows has the
bits of a call on those rows alone.  The worst error / bound ratios go to the parity record under "lora_rows_error_over_bound"."""
import itertools
import time

import pytest
import torch

import test_lora_rows_host as H
from suite_budget import record
from test_decoder_train_bounds_host import worst
from test_gpu_backward_ops import NAN16, call, guard_intact, ops, workspace  # noqa: F401

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
D = "cuda"

# a group: (r, col0, N) per segment
GROUPS = {
    "r16": ((16, 0, 32),),
    "r32 x 2": ((32, 0, 96), (32, 96, 544)),
    "r64, columns before it": ((64, 16, 544),),
    "mixed ranks": ((16, 0, 96), (64, 96, 32), (32, 128, 544)),
    "two with a gap": ((16, 0, 32), (32, 64, 96)),
    "r64 x 3, a gap": ((64, 0, 32), (64, 32, 96), (64, 160, 32)),
}
_MS, _KS = (1, 5, 16, 17, 48, 64), (32, 96, 1056, 4096)
# M = 1 and M = 64 take every (K, group); the others walk the diagonals
CASES = [(m, k, g) for m in (1, 64) for k, g in itertools.product(_KS, GROUPS)] + \
        [(m, _KS[i % 4], list(GROUPS)[(2 * i + 1) % 6]) for i, m in enumerate((5, 16, 17, 48))] + \
        [(5, 4096, "mixed ranks"), (17, 1056, "r64 x 3, a gap"), (48, 1056, "mixed ranks")]
F16_CASE = (17, 1056, "mixed ranks")
PAD_ROWS = 3        # canary rows behind the M rows of U and Y

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.monotonic()
    yield
    print(f"\ntests/test_gpu_lora_rows.py: {time.monotonic() - t:.1f} s; error / bound: {_RATIOS}")


def hold(name, got, ref, bound):
    """every element of got within bound of ref; the worst ratio is printed and recorded before it is asserted"""
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(err).all(), f"{name}: non-finite elements (left unwritten?)"
    r = worst(err, bound)
    _RATIOS[name] = round(max(_RATIOS.get(name, 0.0), r), 4)
    record("lora_rows_error_over_bound", _RATIOS)
    print(f"{name}: error / bound = {r:.3f}")
    assert r <= 1.0, f"{name}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound, worst ratio {r:.3f}"


def fill16(n, dtype=bf):
    return torch.full((n,), NAN16, dtype=torch.int16, device=D).view(dtype)


def bits(t):
    return t.contiguous().view(torch.int16)


class Run:
    """one call on the inputs of H.rows_inputs: X as columns [8, 8 + K) of a padded buffer, Y (M + PAD_ROWS, ldy > the last segment's
    end) and U (M + PAD_ROWS, sum r + 8) NaN-filled with guard tails, the segments of Y's first M rows holding y"""

    def __init__(self, ops, inp, M=None, row0=0, dtype=bf):
        self.ops, self.inp, self.dtype = ops, inp, dtype
        self.row0, self.M = row0, inp["x"].shape[0] - row0 if M is None else M
        M, K = self.M, inp["x"].shape[1]
        self.ldx = K + 24
        self.x = fill16((M + 1) * self.ldx, dtype)
        self.xv = self.x[:M * self.ldx].view(M, self.ldx)[:, 8:8 + K]
        self.xv.copy_(inp["x"][row0:row0 + M].to(D))
        self.width = max(c + n for _, _, c, n, _ in inp["segs"])
        self.ldy, self.rsum = self.width + 40, sum(a.shape[0] for a, *_ in inp["segs"])
        self.ldu = self.rsum + 8
        self.segs = [(a.to(D), b.to(D), c, s) for a, b, c, _, s in inp["segs"]]

    def __call__(self):
        M, inp = self.M, self.inp
        rows = M + PAD_ROWS
        self.y = fill16(rows * self.ldy + 64, self.dtype)
        self.u = fill16(rows * self.ldu + 64, self.dtype)
        yv = self.y[:rows * self.ldy].view(rows, self.ldy)
        for _, _, c, n, _ in inp["segs"]:
            yv[:M, c:c + n] = inp["y"][self.row0:self.row0 + M, c:c + n].to(D)
        self.before = bits(self.y).clone()
        uv = self.u[:rows * self.ldu].view(rows, self.ldu)
        with torch.no_grad():
            self.ops.lora_rows(self.xv, self.segs, yv[:M, :self.width], u=uv[:M, :self.rsum])
        torch.cuda.synchronize()
        # what the call may not touch: Y outside the segments (bit for bit what it held), U outside (M, sum r)
        mask = torch.ones(rows, self.ldy, dtype=torch.bool, device=D)
        for _, _, c, n, _ in inp["segs"]:
            mask[:M, c:c + n] = False
        after, before = bits(self.y), self.before
        assert torch.equal(after[:rows * self.ldy].view(rows, self.ldy)[mask], before[:rows * self.ldy].view(rows, self.ldy)[mask])
        assert torch.equal(after[rows * self.ldy:], before[rows * self.ldy:])
        ub = bits(self.u)
        assert (ub[:rows * self.ldu].view(rows, self.ldu)[:M, self.rsum:] == NAN16).all()
        assert (ub[:rows * self.ldu].view(rows, self.ldu)[M:] == NAN16).all() and (ub[rows * self.ldu:] == NAN16).all()
        return uv[:M, :self.rsum].clone(), yv[:M, :self.width].clone()


def check(name, inp, u, y, U=H.U):
    """u and y of rows [0, M) against the float64 models"""
    o = 0
    for a, b, c, n, s in inp["segs"]:
        r = a.shape[0]
        md = H.down_model(inp["x"], a, 1.0, U=U)
        hold(f"{name} u", u[:, o:o + r], md["out"], md["bound"])
        mu = H.up_model(u[:, o:o + r].cpu(), b, inp["y"][:, c:c + n], s, True, U=U)
        hold(f"{name} y", y[:, c:c + n], mu["out"], mu["bound"])
        o += r


@pytest.mark.parametrize("M,K,group", CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_lora_rows_bounds(ops, M, K, group):
    inp = H.rows_inputs(M, K, GROUPS[group])
    run = Run(ops, inp)
    u, y = run()
    check("lora_rows", inp, u, y)
    u2, y2 = run()
    assert torch.equal(bits(u), bits(u2)) and torch.equal(bits(y), bits(y2))


@pytest.mark.parametrize("K,group", [(1056, "mixed ranks"), (4096, "r32 x 2"), (96, "r64 x 3, a gap")])
def test_a_block_of_16_rows_has_the_bits_of_a_call_of_its_own(ops, K, group):
    """rows 16 - 31 and 32 - 47 of an M = 48 call against M = 16 calls on those rows; an M = 5 call against the first five rows of
    an M = 16 call"""
    inp = H.rows_inputs(48, K, GROUPS[group])
    u48, y48 = Run(ops, inp)()
    cols = torch.zeros(y48.shape[1], dtype=torch.bool, device=D)
    for _, _, c, n, _ in inp["segs"]:
        cols[c:c + n] = True
    for row0 in (0, 16, 32):
        u16, y16 = Run(ops, inp, M=16, row0=row0)()
        assert torch.equal(bits(u16), bits(u48[row0:row0 + 16])), row0
        assert torch.equal(bits(y16[:, cols]), bits(y48[row0:row0 + 16][:, cols])), row0
    u5, y5 = Run(ops, inp, M=5)()
    assert torch.equal(bits(u5), bits(u48[:5])) and torch.equal(bits(y5[:, cols]), bits(y48[:5][:, cols]))


def test_c_abi_with_a_guarded_workspace(ops):
    """the entry point itself: the workspace is exactly u2tok_lora_rows_workspace_bytes, the guard behind it stays intact, and the
    result has the wrapper's bits; one byte less is U2TOK_ERR_WORKSPACE and writes nothing"""
    M, K = 17, 1056
    inp = H.rows_inputs(M, K, GROUPS["mixed ranks"])
    run = Run(ops, inp)
    u, y = run()
    segs = ops.lora_segs(run.segs)
    import ctypes as C
    nb = ops.lora_rows_workspace_bytes(M, K, segs)
    assert nb == 2 * 5 * 112 * 64
    ws = workspace(nb)
    width, rsum = run.width, run.rsum
    yb = fill16(M * width)
    yv = yb.view(M, width)
    for _, _, c, n, _ in inp["segs"]:
        yv[:, c:c + n] = inp["y"][:, c:c + n].to(D)
    ub = fill16(M * rsum)
    call(ops, "u2tok_lora_rows", run.xv.data_ptr(), run.ldx, C.addressof(segs), 3, ub.data_ptr(), rsum, yb.data_ptr(), width, M, K,
         ws.data_ptr(), nb)
    assert guard_intact(ws, nb)
    assert torch.equal(bits(ub.view(M, rsum)), bits(u))
    for _, _, c, n, _ in inp["segs"]:
        assert torch.equal(bits(yv[:, c:c + n]), bits(y[:, c:c + n]))
    keep = bits(yb).clone()
    call(ops, "u2tok_lora_rows", run.xv.data_ptr(), run.ldx, C.addressof(segs), 3, ub.data_ptr(), rsum, yb.data_ptr(), width, M, K,
         ws.data_ptr(), nb - 1, status=-3)
    assert torch.equal(bits(yb), keep)


def test_f16_build(ops):
    """one case on the IEEE-half build (the wrapper picks the build by the tensors' dtype): the same models with U = 2^-11"""
    M, K, group = F16_CASE
    inp = H.rows_inputs(M, K, GROUPS[group], dtype=torch.float16)
    u, y = Run(ops, inp, dtype=torch.float16)()
    check("lora_rows f16", inp, u, y, U=H.U16)
