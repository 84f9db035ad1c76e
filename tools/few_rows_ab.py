#!/usr/bin/env python
"""A/B of the few-rows (weight-streaming) product between two builds of the library, on one GPU: the three C entry points
(u2tok_gemm_rows, u2tok_gemm_rows_w8, u2tok_gemm_rows_w8_wide) at the Qwen3-8B layer shapes

    q|k|v (N 6144, K 4096)   out (4096, 4096)   gate|up, pair form (24576, 4096)   down (4096, 12288)

for M = 1, 16, 17, 64 rows and both weight forms on the bf16 build, M = 1 and 64 on the f16 build.  Both libraries are loaded into
the same child process and timed in alternation: per cell a warm-up of each, then --rounds rounds of --launches launches of A and
of B between device events; us per launch, medians over the rounds; "spread" = the largest deviation of a round's B - A from the
median B - A.  --cold: the launches rotate through copies of the weight (512 MB of them), so that every launch streams its weights from
memory as a decode step's products do, instead of finding them in the caches as repeated launches on one weight do.

    python tools/few_rows_ab.py --a DIR_A --b DIR_B [--cold] [--elems bf16] [--yardstick AA.json] [--out profiles/few_rows_ab.json]

DIR_*: folders holding libu2tok_hip.so and libu2tok_hip_f16.so.  The yardstick is A against itself: run the tool with --b DIR_A
first; given that file, every cell gets `yardstick_us` = the larger of the A/A run's |median B - A| and its spread, and `pass` =
|median B - A| <= yardstick_us.

The parent process never opens the GPU: each element type is a child process of its own under its own time limit, started only
if the one before it ended clean; nothing is tried twice."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SHAPES = (("qkv", 6144, 4096, False), ("out", 4096, 4096, False), ("gate_up", 24576, 4096, True), ("down", 4096, 12288, False))
ROWS = {"bf16": (1, 16, 17, 64), "f16": (1, 64)}
LIBS = {"bf16": "libu2tok_hip.so", "f16": "libu2tok_hip_f16.so"}
ENTRY = ("u2tok_gemm_rows", "u2tok_gemm_rows_w8", "u2tok_gemm_rows_w8_wide")


def _load(folder, elem):
    from u2tokenizer_amd import _lib
    h = C.CDLL(str(Path(folder).resolve() / LIBS[elem]))
    for name in ENTRY + ("u2tok_elem",):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert h.u2tok_elem() == elem.encode()
    return h


def child(a):
    import torch
    elem = a.child
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[elem]
    libs = [_load(a.a, elem), _load(a.b, elem)]
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    g = torch.Generator(device=dev).manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for name, N, K, pair in SHAPES:
        w = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5)
        copies = lambda t: [t] + [t.clone() for _ in range(-(-(512 << 20) // (t.numel() * t.element_size())) - 1 if a.cold else 0)]   # noqa: E731
        w16 = copies(w.to(dt))
        w8 = copies((w * 64).clamp_(-448, 448).to(torch.float8_e4m3fn))
        sc = torch.full((N,), 1 / 64, dtype=torch.float32, device=dev)
        del w
        for M in ROWS[elem]:
            x = torch.randn(M, K, device=dev, generator=g).to(dt)
            out = torch.empty(M, N // 2 if pair else N, dtype=dt, device=dev)
            flags, ldc = (512, N // 2) if pair else (0, N)
            for form in ("elem", "e4m3"):
                if form == "elem":
                    entry = "u2tok_gemm_rows"
                    args = [(x.data_ptr(), w.data_ptr(), out.data_ptr(), None, None, M, N, K, K, K, ldc, 0, flags, stream) for w in w16]
                else:
                    entry = "u2tok_gemm_rows_w8_wide" if M > 16 else "u2tok_gemm_rows_w8"
                    args = [(x.data_ptr(), w.data_ptr(), sc.data_ptr(), out.data_ptr(), None, None, M, N, K, K, K, ldc, 0, flags, stream)
                            for w in w8]

                def timed(h, n):
                    fn = getattr(h, entry)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for i in range(n):
                        st = fn(*args[i % len(args)])
                    t1.record()
                    torch.cuda.synchronize()
                    assert st == 0, (entry, st)
                    return t0.elapsed_time(t1) * 1e3 / n

                for h in libs:
                    timed(h, a.launches)
                t = [[], []]
                for _ in range(a.rounds):
                    for i, h in enumerate(libs):
                        t[i].append(timed(h, a.launches))
                diff = [y - x_ for x_, y in zip(*t)]
                md = statistics.median(diff)
                res.append({"elem": elem, "cold": a.cold, "product": name, "N": N, "K": K, "M": M, "weights": form, "entry": entry,
                            "a_us": round(statistics.median(t[0]), 3), "b_us": round(statistics.median(t[1]), 3),
                            "b_minus_a_us": round(md, 3), "spread_us": round(max(abs(d - md) for d in diff), 3)})
                print(json.dumps(res[-1]), flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def _run(cmd, limit):
    """one child under its own time limit; -> its stdout, or SystemExit (nothing further is started)"""
    print("+", " ".join(cmd), flush=True)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"few_rows_ab: timed out after {limit} s: {' '.join(cmd)} -- stopping here")
    if r.returncode != 0:
        raise SystemExit(f"few_rows_ab: exit status {r.returncode}: {' '.join(cmd)}\n{r.stdout[-2000:]}{r.stderr[-2000:]} -- stopping here")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="folder of library A (the parent's build)")
    ap.add_argument("--b", required=True, help="folder of library B")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--cold", action="store_true", help="rotate through 512 MB of weight copies: every launch reads its weights from memory")
    ap.add_argument("--elems", default="bf16,f16")
    ap.add_argument("--yardstick", default=None, help="the JSON of an A-against-A run of this tool")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=list(LIBS))
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = [sys.executable, str(Path(__file__).resolve()), "--a", a.a, "--b", a.b, "--rounds", str(a.rounds), "--launches",
          str(a.launches)] + (["--cold"] if a.cold else [])
    res = {"what": "few-rows product, library B against library A in one process: us per launch of the C entry point, medians over "
                   "interleaved rounds; spread = largest deviation of a round's B - A from the median B - A; yardstick = A against "
                   "A (the larger of its |median B - A| and its spread); pass = |B - A| <= yardstick",
           "rounds": a.rounds, "launches": a.launches, "cold": a.cold, "rows": []}
    for elem in a.elems.split(","):
        out = _run(me + ["--child", elem], 240)
        res["rows"] += json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
    if a.yardstick:
        key = lambda r: (r["elem"], r["product"], r["M"], r["weights"])   # noqa: E731
        aa = {key(r): r for r in json.loads(Path(a.yardstick).read_text())["rows"]}
        for r in res["rows"]:
            y = aa[key(r)]
            r["yardstick_us"] = round(max(abs(y["b_minus_a_us"]), y["spread_us"]), 3)
            r["pass"] = abs(r["b_minus_a_us"]) <= r["yardstick_us"]
    for r in res["rows"]:
        print(json.dumps(r), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
