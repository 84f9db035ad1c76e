#!/usr/bin/env python
"""A/B of the HOST cost of the module forwards of csrc/pipeline.hip between two trees (each with its own build of the library): ms per
forward at shapes whose kernels are too small to hide the host -- TOKENIZER_CASES["hard_1l"] and the ViT tower of VIT_CASES["c64"]
(tests/cases.py), bf16, weights from synth.fill_module_.

    python tools/pipeline_host_ab.py --a DIR_A --b DIR_B [--yardstick AA.json] [--out FILE.json] [--pairs 3] [--rounds 5] [--calls 200]

The pairing and the yardstick are tools/decoder_routes_ab.py's (run_pairs, compare): one child per tree in alternation, each under its
own time limit, the next started only if the last ended clean; the yardstick is the same run with tree a on both sides, and a cell
passes when b is faster or |median(b - a)| is within the larger of the yardstick's |median difference| and its spread.  A child
imports the package and the cases of ITS tree and times, per cell, --rounds rounds of --calls forwards after a warm-up round
(device events around the calls: the host time between launches counts); its figure per cell is the median round."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from decoder_routes_ab import compare, run_pairs  # noqa: E402

CELLS = ("tokenizer_hard_1l", "vit_c64")


def child(a):
    sys.path.insert(0, str(Path.cwd() / "tests"))   # (cwd and PYTHONPATH are the child's tree)
    from types import SimpleNamespace as NS
    import torch
    from cases import TOKENIZER_CASES, VIT_CASES, tokenizer_inputs
    from u2tokenizer_amd import ops, synth
    from u2tokenizer_amd.tokenizer import u2Tokenizer
    from u2tokenizer_amd.vit import ViT3DTower
    ops.device_check()
    torch.set_grad_enabled(False)
    bf = torch.bfloat16

    def timed(call):
        ms = []
        for _ in range(a.rounds + 1):           # (the first round is the warm-up)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / a.calls)
        return statistics.median(ms[1:])

    c = TOKENIZER_CASES["hard_1l"]
    tok = u2Tokenizer(embed_size=c["E"], num_heads=c["heads"], num_layers=c["layers"], top_k=c["top_k"], use_multi_scale=c["use_multi_scale"],
                      num_3d_query_token=c["Q"], hidden_size=c["E"], attn_type=c["attn_type"], enable_diffts=c["enable_diffts"],
                      enable_dmtp=c["enable_dmtp"])
    synth.fill_module_(tok, seed=c["seed"], prefix="u2tokenizer.")
    tok = tok.to(bf).to("cuda")
    v, t = (x.to(bf).to("cuda") for x in tokenizer_inputs(c))
    out = {CELLS[0]: timed(lambda: tok(v_token=v, t_token=t))}
    c = VIT_CASES["c64"]
    vit = ViT3DTower(NS(vision_select_layer=-1, vision_select_feature=c["select_feature"], image_channel=1, image_size=c["image_size"],
                        patch_size=c["patch_size"]))
    synth.fill_module_(vit, seed=c["seed"], prefix="vision_tower.")
    vit = vit.to(bf).to("cuda")
    vol = synth.synth_volume(1, c["nchunk"], c["image_size"], seed=c["seed"], dtype=torch.float16).view(c["nchunk"], 1, *c["image_size"]).to("cuda")
    out[CELLS[1]] = timed(lambda: vit(vol))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--yardstick", default=None, help="the JSON of the same run with --b DIR_A")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--limit", type=int, default=180, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.a or not a.b:
        ap.error("--a and --b are required")
    trees = {"a": Path(a.a).resolve(), "b": Path(a.b).resolve()}
    runs = run_pairs(trees, ["--rounds", str(a.rounds), "--calls", str(a.calls)], a.pairs, a.limit, script=__file__)
    yard = json.loads(Path(a.yardstick).read_text())["cells"] if a.yardstick else None
    cells, failed = compare(runs, yard, lambda cell: "ms per forward")
    res = {"what": "host cost of the module forwards, tree b against tree a: ms per forward (device events around the calls, host time "
                   "between launches included); one child per tree in alternation; margin = the larger of |median difference| and spread "
                   "of the yardstick run (tree a on both sides)",
           "a": str(a.a), "b": str(a.b), "same_tree": trees["a"] == trees["b"], "pairs": a.pairs, "rounds": a.rounds, "calls": a.calls,
           "cells": cells}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if failed:
        print("slower beyond the yardstick's margin:", failed, flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
