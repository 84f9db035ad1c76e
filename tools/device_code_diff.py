#!/usr/bin/env python
"""Per-kernel diff of the gfx950 device code of two builds of the same sources: for each object file given as OLD NEW, the device
code object is unbundled, disassembled, and the instruction text of every kernel symbol compared (addresses and encodings
dropped, so that a kernel that merely moved compares equal).  No GPU is needed.

    python tools/device_code_diff.py OLD.o NEW.o [OLD2.o NEW2.o ...] [--show 40]

Prints, per pair, the number of kernels, the ones that differ and their differing lines; exit status 1 when any kernel differs
or the sets of symbols are not the same."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"


def kernels(obj):
    """{demangled kernel symbol: [instruction text]} of the gfx950 code object bundled in a host object"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = Path(tmp) / "fat.bin", Path(tmp) / "dev.co"      # (as tools/kernel_regs.py)
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                        f"--output={co}", "--unbundle"], check=True)
        text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", str(co)], check=True,
                              capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            ins = re.sub(r"^\s*[0-9a-f]+:\s*", "", line)          # (objdump without encodings: "addr: text" or plain text)
            ins = re.sub(r"\s*//\s*[0-9A-F]+:.*$", "", ins).strip()
            ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<L>", ins)     # branch targets as symbol + offset
            cur.append(ins)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("objs", nargs="+")
    ap.add_argument("--show", type=int, default=40, help="differing lines printed per kernel")
    a = ap.parse_args()
    if len(a.objs) % 2:
        ap.error("object files come in OLD NEW pairs")
    bad = 0
    for old, new in zip(a.objs[0::2], a.objs[1::2]):
        ko, kn = kernels(old), kernels(new)
        differ = [k for k in ko if k in kn and ko[k] != kn[k]]
        only = sorted(set(ko) ^ set(kn))
        print(f"{old} -> {new}: {len(ko)} symbols, {len(differ)} differ, {len(only)} in one build only")
        for k in only:
            print("  only in one:", k)
        for k in differ:
            d = [ln for ln in difflib.unified_diff(ko[k], kn[k], lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
            print(f"  {k}: {len(ko[k])} -> {len(kn[k])} instructions, {len(d)} differing lines")
            for ln in d[:a.show]:
                print("    " + ln)
        bad += len(differ) + len(only)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
