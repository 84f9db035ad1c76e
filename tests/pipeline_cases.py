"""The cases of tests/test_gpu_pipeline_bits.py and tests/test_pipeline_workspace_host.py: what the three module forwards of
csrc/pipeline.hip (ViT tower, pooling projector, u2Tokenizer) COMPUTE and LAUNCH, and what their dry runs ANSWER, pinned with the
library of the commit named inside the fixtures -- before the forwards were split into stage functions over named weight records.

tests/golden/pipeline_bits.json (GPU): per case the SHA-256 of every output's bytes and, from a second run under option
"profile" = 1, the launch records of u2tok_profile_collect2 (count, flops and bytes per category: how many launches of which size
each category made).  Cases, on both builds (bf16, f16), weights from synth.fill_module_:
  * the ten TOKENIZER_CASES of tests/cases.py (out, last_topk_indices where hard top-k is on, last_svr_tokens);
  * forward_with_taps on hard_2l_live (rma) and linvt_b2_live with svr_in, visual_in and tta_in all supplied (out and every tap);
  * options tok_flash = 0, kmajor_b = 0, tta_overlap = 0, each on mu2_2l, rope_fix, linvt_b2_live;
  * d40_1l: E = 320 with 8 heads, head dim 40, which the fused attention kernels do not take -- the GEMM chain by shape;
  * e256_8l / e256_7l: 8 layers switch the side-stream k|v prefetch off (the L <= 7 rule), 7 layers keep it;
  * direct_unpacked: u2tok_tokenizer_forward on a hand-built weight table whose wq / wk / wv (and biases) are separately allocated,
    so the three-launch q|k|v and the two-launch k|v projections run;
  * the ViT tower of VIT_CASES["c64"] with select_feature "patch" and "cls_patch", at defaults, vit_flash = 0, vit_vt_epilogue = 0;
  * both SPP_CASES.

tests/golden/pipeline_workspace.json (host, no GPU): the answers of u2tok_tokenizer_workspace_bytes, u2tok_vit_workspace_bytes and
u2tok_spp_workspace_bytes for both builds, at default options and with kmajor_b = 0, over WORKSPACE_CONFIGS (accepted and refused).

`python tests/pipeline_cases.py --record --commit HASH [--out FILE]` runs the GPU cases and writes the first fixture,
`python tests/pipeline_cases.py --record-workspace --commit HASH [--out FILE]` the second (no GPU); the tests only ever read them."""
import argparse
import ctypes as C
import functools
import hashlib
import json
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import torch

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from cases import SPP_CASES, TOKENIZER_CASES, VIT_CASES, spp_inputs, tokenizer_inputs  # noqa: E402
from u2tokenizer_amd import synth  # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "pipeline_bits.json"
WS_FIXTURE = FIXTURE.with_name("pipeline_workspace.json")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
OPTION_DEFAULTS = {"tok_flash": 1, "kmajor_b": 1, "tta_overlap": 1, "vit_flash": 1, "vit_vt_epilogue": 1}
NCAT = 6   # the categories of u2tok_profile_collect2

_LIVE = dict(max_seq_len=512, use_multi_scale=True, attn_type="rma", enable_diffts=True, enable_dmtp=True, lively=True)
TOK_CONFIGS = dict(
    TOKENIZER_CASES,
    d40_1l=dict(_LIVE, heads=8, E=320, layers=1, B=2, T=3, N=24, Lt=20, Q=16, top_k=24, seed=61),
    e256_8l=dict(_LIVE, heads=4, E=256, layers=8, B=1, T=2, N=16, Lt=16, Q=16, top_k=16, seed=62),
    e256_7l=dict(_LIVE, heads=4, E=256, layers=7, B=1, T=2, N=16, Lt=16, Q=16, top_k=16, seed=62),
)
TAP_CASES = ("hard_2l_live", "linvt_b2_live")
OPTION_CASES = tuple((o, n) for o in ("tok_flash", "kmajor_b", "tta_overlap") for n in ("mu2_2l", "rope_fix", "linvt_b2_live"))
DIRECT_CASE = "hard_2l_live"
VIT_SELECT = ("patch", "cls_patch")
VIT_OPTIONS = ({}, {"vit_flash": 0}, {"vit_vt_epilogue": 0})


def _opt_tag(options):
    return "-".join(f"{k}{v}" for k, v in options.items()) or "default"


def specs():
    """{case id (without the build): (kind, config name, options)}"""
    out = {f"tok-{n}": ("tok", n, {}) for n in TOK_CONFIGS}
    out.update({f"taps-{n}": ("taps", n, {}) for n in TAP_CASES})
    out.update({f"tok-{n}-{o}0": ("tok", n, {o: 0}) for o, n in OPTION_CASES})
    out["direct_unpacked-" + DIRECT_CASE] = ("direct", DIRECT_CASE, {})
    for sel in VIT_SELECT:
        for options in VIT_OPTIONS:
            out[f"vit-c64-{sel}-{_opt_tag(options)}"] = ("vit", sel, options)
    out.update({f"spp-{n}": ("spp", n, {}) for n in SPP_CASES})
    return out


def case_ids():
    return [f"{elem}-{cid}" for elem in DTYPES for cid in specs()]


def swapped_rows(c):
    """Two rows of v_token that differ in chunk AND in token position (exchanging them is no symmetry of any attention type)"""
    return (0, 0, 1), (0, c["T"] - 1, c["N"] - 2)


# ------------------------------------------------------------------------------------------------------------- GPU: running a case
def _mk_tok(c):
    from u2tokenizer_amd.tokenizer import u2Tokenizer
    m = u2Tokenizer(embed_size=c["E"], num_heads=c["heads"], num_layers=c["layers"], top_k=c["top_k"],
                    use_multi_scale=c["use_multi_scale"], num_3d_query_token=c["Q"], hidden_size=c["E"],
                    attn_type=c["attn_type"], enable_diffts=c["enable_diffts"], enable_dmtp=c["enable_dmtp"])
    synth.fill_module_(m, seed=c["seed"], prefix="u2tokenizer.", lively=c.get("lively", False))
    return m


@functools.lru_cache(maxsize=None)
def _tok_model(name, elem):
    return _mk_tok(TOK_CONFIGS[name]).to(DTYPES[elem]).to("cuda")


@functools.lru_cache(maxsize=None)
def _vit_model(select, elem):
    from u2tokenizer_amd.vit import ViT3DTower
    c = VIT_CASES["c64"]
    m = ViT3DTower(NS(vision_select_layer=-1, vision_select_feature=select, image_channel=1, image_size=c["image_size"],
                      patch_size=c["patch_size"]))
    synth.fill_module_(m, seed=c["seed"], prefix="vision_tower.")
    return m.to(DTYPES[elem]).to("cuda")


@functools.lru_cache(maxsize=None)
def _spp_model(name, elem):
    from u2tokenizer_amd.projector import SpatialPoolingProjector
    c = SPP_CASES[name]
    m = SpatialPoolingProjector(c["image_size"], c["patch_size"], c["in_dim"], c["E"], c["layer_type"], c["layer_num"],
                                c["pooling_type"], c["pooling_size"])
    synth.fill_module_(m, seed=c["seed"], prefix="mm_projector.")
    return m.to(DTYPES[elem]).to("cuda")


def _tok_inputs(name, elem):
    v, t = tokenizer_inputs(TOK_CONFIGS[name])
    return v.to(DTYPES[elem]).to("cuda"), t.to(DTYPES[elem]).to("cuda")


def _run_tok(name, elem):
    m = _tok_model(name, elem)
    m.capture_svr_tokens = True
    v, t = _tok_inputs(name, elem)
    out = {"out": m(v_token=v, t_token=t), "last_svr_tokens": m.last_svr_tokens}
    if not TOK_CONFIGS[name]["enable_diffts"]:
        out["last_topk_indices"] = m.last_topk_indices
    return out


def _run_taps(name, elem):
    c, dt = TOK_CONFIGS[name], DTYPES[elem]
    m = _tok_model(name, elem)
    v, t = _tok_inputs(name, elem)
    Lv = c["top_k"] + (c["top_k"] // 2 + c["top_k"] // 4 if c["use_multi_scale"] else 0)
    given = lambda what, shape: (0.5 * synth.synth_tensor(what, shape, c["seed"])).to(dt).to("cuda")   # noqa: E731
    svr_in = [given(f"svr_in{l}", (c["B"], c["T"], c["N"], c["E"])) for l in range(c["layers"])]
    tta_in = [given(f"tta_in{l}", (c["B"], c["Q"], c["E"])) for l in range(c["layers"])]
    out, taps = m.forward_with_taps(v, t, svr_in=svr_in, visual_in=given("visual_in", (c["B"], Lv, c["E"])), tta_in=tta_in)
    res = {"out": out, "visual_out": taps["visual_out"]}
    for key in ("svr_out", "tta_out"):
        res.update({f"{key}{l}": x for l, x in enumerate(taps[key])})
    if not c["enable_diffts"]:
        res["last_topk_indices"] = m.last_topk_indices
    return res


def _run_direct(name, elem):
    """u2tok_tokenizer_forward on a weight table of separately allocated tensors, each with 64 spare elements behind it: no wk
    starts where its wq ends, so nothing is taken for packed"""
    from u2tokenizer_amd import _lib, ops
    c, dt = TOK_CONFIGS[name], DTYPES[elem]
    m = _tok_model(name, elem)
    v, t = _tok_inputs(name, elem)
    B, T, N, E = v.shape
    with ops.on_device(v, elem=dt) as (h, stream):
        bufs = []

        def own(p):
            if p is None:
                return None
            bufs.append(torch.empty(p.numel() + 64, dtype=dt, device="cuda"))
            return bufs[-1][:p.numel()].view(p.shape).copy_(p.detach())

        table = ops.weight_table([own(p) for p in m._weights()])
        cfg = m._config(B, T, N, E, t.shape[1])
        nbytes = h.u2tok_tokenizer_workspace_bytes(C.byref(cfg))
        assert nbytes
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty((B, c["Q"], E), dtype=dt, device="cuda")
        idx = None if c["enable_diffts"] else torch.empty((B, c["top_k"]), dtype=torch.int64, device="cuda")
        svr = torch.empty((B, T * N, E), dtype=dt, device="cuda")
        _lib.check(h.u2tok_tokenizer_forward(C.byref(cfg), table, v.data_ptr(), t.data_ptr(), out.data_ptr(),
                                             None if idx is None else idx.data_ptr(), svr.data_ptr(), ws.data_ptr(), ws.numel(),
                                             stream), "u2tok_tokenizer_forward")
        torch.cuda.synchronize()
    res = {"out": out, "last_svr_tokens": svr}
    if idx is not None:
        res["last_topk_indices"] = idx
    return res


def _run_vit(select, elem):
    c = VIT_CASES["c64"]
    vol = synth.synth_volume(1, c["nchunk"], c["image_size"], seed=c["seed"], dtype=torch.float16)
    return {"out": _vit_model(select, elem)(vol.view(c["nchunk"], 1, *c["image_size"]).to("cuda"))}


def _run_spp(name, elem):
    return {"out": _spp_model(name, elem)(spp_inputs(SPP_CASES[name]).to(DTYPES[elem]).to("cuda"))}


RUNNERS = {"tok": _run_tok, "taps": _run_taps, "direct": _run_direct, "vit": _run_vit, "spp": _run_spp}


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(ops, elem, cid):
    """{"sha": {output: SHA-256}, "profile": {"count" | "flops" | "bytes": one number per category}} of one case on the GPU: the
    digests from a run at the case's options, the records from a second run under "profile" = 1 (whose digests must agree)"""
    from u2tokenizer_amd import _lib
    kind, name, options = specs()[cid]

    def run():
        res = RUNNERS[kind](name, elem)
        torch.cuda.synchronize()
        return {k: _sha(v) for k, v in res.items()}

    try:
        for k, v in options.items():
            ops.set_option(k, v)
        sha = run()
        ops.set_option("profile", 1)
        try:
            again = run()
            cx, h = ops.active_context(torch.device("cuda", torch.cuda.current_device())), _lib.load_library(elem)
            prev = h.u2tok_ctx_get_current()
            h.u2tok_ctx_set_current(cx.handle_for(elem))
            ms, fl, by, cnt = (C.c_double * NCAT)(), (C.c_double * NCAT)(), (C.c_double * NCAT)(), (C.c_int64 * NCAT)()
            try:
                _lib.check(h.u2tok_profile_collect2(ms, fl, by, cnt, NCAT), "u2tok_profile_collect2")
            finally:
                h.u2tok_ctx_set_current(prev)
        finally:
            ops.set_option("profile", 0)
    finally:
        for k in options:
            ops.set_option(k, OPTION_DEFAULTS[k])
    assert again == sha, (elem, cid, "two runs in one process gave different bits")
    return {"sha": sha, "profile": {"count": list(cnt), "flops": list(fl), "bytes": list(by)}}


# ------------------------------------------------------------------------------------------------------------- host: workspace sizes
def _tok_ws(name=None, **kw):
    """The named arguments of a u2tok_tokenizer_config: a TOK_CONFIGS entry (default: the shipped flavour, tiny) with `kw` over it"""
    c = TOK_CONFIGS[name] if name else dict(B=1, T=4, N=32, E=512, Lt=24, heads=8, layers=2, top_k=32, Q=16, use_multi_scale=True,
                                            attn_type="rma", enable_diffts=True, enable_dmtp=True, max_seq_len=512)
    a = dict(B=c["B"], T=c["T"], N=c["N"], E=c["E"], Lt=c["Lt"], num_heads=c["heads"], num_layers=c["layers"], top_k=c["top_k"],
             num_query=c["Q"], use_multi_scale=int(c["use_multi_scale"]), attn_type={"rma": 0, "rope": 1}.get(c["attn_type"], 2),
             enable_diffts=int(c["enable_diffts"]), enable_dmtp=int(c["enable_dmtp"]), max_seq_len=c["max_seq_len"],
             diffts_tau=1.0, ln_eps=1e-5)
    a.update(kw)
    return a


def _vit_ws(**kw):
    c = VIT_CASES["c64"]
    a = dict(nchunk=c["nchunk"], img=c["image_size"], patch=c["patch_size"], hidden=768, mlp_dim=3072, depth=12, heads=12,
             vol_dtype=0, keep_cls=0, ln_eps=1e-5)
    a.update(kw)
    return a


def _spp_ws(name, **kw):
    c = SPP_CASES[name]
    a = dict(nchunk=c["nchunk"], grid=[i // p for i, p in zip(c["image_size"], c["patch_size"])], pooling_size=c["pooling_size"],
             pooling_type=0 if c["pooling_type"] == "spatial" else 1, in_dim=c["in_dim"], out_dim=c["E"],
             layer_type=0 if c["layer_type"] == "mlp" else 1, layer_num=c["layer_num"])
    a.update(kw)
    return a


def workspace_configs():
    """{config id: (export, named arguments of its config struct)}"""
    out = {}
    for n in TOK_CONFIGS:                                  # every tokenizer config of the GPU cases
        out[f"tok-{n}"] = ("tokenizer", _tok_ws(n))
    # BASELINE configs[1] and [2] at the size the benchmark runs: E = 4096, 8 chunks
    full = dict(E=4096, T=8, num_layers=4, num_query=256, top_k=1024, Lt=1024)
    out["tok-config2-E4096"] = ("tokenizer", _tok_ws(B=4, N=64, **full))       # 128^3 volumes: 64 projector tokens per chunk
    out["tok-config3-E4096"] = ("tokenizer", _tok_ws(B=1, N=256, **full))      # 256^3 volumes: 256
    for flag in ("use_multi_scale", "enable_diffts", "enable_dmtp"):           # each boolean flipped from the shipped flavour
        out[f"tok-{flag}0"] = ("tokenizer", _tok_ws(**{flag: 0}))
    for L in (0, 1, 7, 8):
        out[f"tok-layers{L}"] = ("tokenizer", _tok_ws(num_layers=L))
    for at in (0, 1, 2):
        for B in (1, 2):
            out[f"tok-attn{at}-B{B}"] = ("tokenizer", _tok_ws(attn_type=at, B=B))
    # refused by the argument checks
    out["tok-refused-topk-above-TN"] = ("tokenizer", _tok_ws(enable_diffts=0, top_k=4 * 32 + 1))
    out["tok-topk-above-TN-diffts"] = ("tokenizer", _tok_ws(top_k=4 * 32 + 1))          # (accepted: DiffTS has no such limit)
    out["tok-refused-N-above-max"] = ("tokenizer", _tok_ws(N=513))
    out["tok-refused-T-above-max"] = ("tokenizer", _tok_ws(T=513, N=2))
    out["tok-refused-Q-above-max"] = ("tokenizer", _tok_ws(num_query=513))
    out["tok-refused-head-dim-36"] = ("tokenizer", _tok_ws(E=288))
    out["tok-refused-attn3"] = ("tokenizer", _tok_ws(attn_type=3))
    for depth in (0, 1, 12):
        for keep in (0, 1):
            out[f"vit-c64-depth{depth}-keep{keep}"] = ("vit", _vit_ws(depth=depth, keep_cls=keep))
            out[f"vit-256cube-depth{depth}-keep{keep}"] = ("vit", _vit_ws(nchunk=8, img=[32, 256, 256], depth=depth, keep_cls=keep))
    out["vit-refused-image-not-divisible"] = ("vit", _vit_ws(img=[32, 64, 60]))
    out["vit-refused-hidden-not-heads-x-64"] = ("vit", _vit_ws(hidden=760))
    for n in SPP_CASES:
        out[f"spp-{n}"] = ("spp", _spp_ws(n))
    out["spp-refused-pooling-type-2"] = ("spp", _spp_ws("mlp2", pooling_type=2))
    out["spp-refused-grid-below-window"] = ("spp", _spp_ws("mlp2", grid=[1, 4, 4]))
    return out


WS_OPTIONS = ({}, {"kmajor_b": 0})


def workspace_ids():
    return [f"{elem}-{_opt_tag(o)}-{cid}" for elem in DTYPES for o in WS_OPTIONS for cid in workspace_configs()]


def workspace_answers():
    """{id: bytes} from the libraries' dry runs; no device is touched.  The options are set on a context of their own."""
    from u2tokenizer_amd import _lib
    out = {}
    for elem in DTYPES:
        h = _lib.load_library(elem)
        structs = {"tokenizer": (_lib.TokConfig, h.u2tok_tokenizer_workspace_bytes), "vit": (_lib.VitConfig, h.u2tok_vit_workspace_bytes),
                   "spp": (_lib.SppConfig, h.u2tok_spp_workspace_bytes)}
        for options in WS_OPTIONS:
            cx, prev = C.c_void_p(), h.u2tok_ctx_get_current()
            _lib.check(h.u2tok_ctx_create(C.byref(cx)), "u2tok_ctx_create")
            h.u2tok_ctx_set_current(cx)
            try:
                for k, v in options.items():
                    _lib.check(h.u2tok_set_option(k.encode(), v), k)
                for cid, (export, a) in workspace_configs().items():
                    struct, fn = structs[export]
                    a = {k: (C.c_int32 * 3)(*v) if isinstance(v, list) else v for k, v in a.items()}
                    out[f"{elem}-{_opt_tag(options)}-{cid}"] = int(fn(C.byref(struct(**a))))
            finally:
                h.u2tok_ctx_set_current(prev)
                h.u2tok_ctx_destroy(cx)
    return out


# ------------------------------------------------------------------------------------------------------------- recording
def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="run every GPU case and write the digests and launch records")
    ap.add_argument("--record-workspace", action="store_true", help="write the dry runs' answers (no GPU)")
    ap.add_argument("--commit", default="", help="the commit whose library is recorded (written into the file)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.record_workspace:
        answers = workspace_answers()
        out = Path(a.out or WS_FIXTURE)
        out.write_text(json.dumps({"recorded_at_commit": a.commit, "bytes": answers}, indent=0, sort_keys=True) + "\n")
        print(f"wrote {len(answers)} answers to {out}: {sum(v == 0 for v in answers.values())} refused")
        return 0
    if not a.record:
        print(f"{len(case_ids())} GPU cases, {len(workspace_ids())} workspace answers; --record / --record-workspace write them")
        return 0
    from u2tokenizer_amd import ops
    ops.device_check()
    torch.set_grad_enabled(False)
    cases = {}
    for elem in DTYPES:
        for cid in specs():
            cases[f"{elem}-{cid}"] = run_case(ops, elem, cid)
            print(f"{elem}-{cid}", cases[f"{elem}-{cid}"]["profile"]["count"], flush=True)
    assert sorted(cases) == sorted(case_ids())
    out = Path(a.out or FIXTURE)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"recorded_at_commit": a.commit, "cases": cases}, indent=0, sort_keys=True) + "\n")
    print(f"wrote {len(cases)} cases to {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
