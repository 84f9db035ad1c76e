#!/usr/bin/env python
"""Do two runs launch the same kernels in the same order?  From the rocprofv3 --kernel-trace csv of each run, the sequence of
(kernel name, grid, workgroup size) per stream, streams numbered in the order they first launch:

    python tools/trace_launch_order.py <dir of run A> <dir of run B>

prints the launches per stream and "identical", or the first difference of the first stream that differs (exit status 1)."""
import csv
import sys
from pathlib import Path


def sequences(d):
    """[launch sequence of stream 0, of stream 1, ...] -- streams in order of first launch, launches in dispatch order"""
    rows = [r for f in sorted(Path(d).rglob("*kernel_trace.csv")) for r in csv.DictReader(open(f))]
    assert rows, f"no kernel trace under {d}"
    key = "Stream_Id" if "Stream_Id" in rows[0] else "Queue_Id"
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    streams = {}
    for r in rows:
        dims = tuple(r.get(f"{what}_{ax}", "") for what in ("Grid_Size", "Workgroup_Size") for ax in "XYZ")
        streams.setdefault((r.get("Agent_Id"), r[key]), []).append((r["Kernel_Name"],) + dims)
    return list(streams.values())


def main():
    a, b = sequences(sys.argv[1]), sequences(sys.argv[2])
    print(f"streams: {len(a)} / {len(b)}; launches per stream: {[len(s) for s in a]} / {[len(s) for s in b]}")
    if a == b:
        print("identical: the same (kernel, grid, workgroup size) sequence on every stream")
        return 0
    for i, (sa, sb) in enumerate(zip(a, b)):
        for j, (x, y) in enumerate(zip(sa, sb)):
            if x != y:
                print(f"first difference: stream {i}, launch {j}:\n  A {x}\n  B {y}")
                return 1
        if len(sa) != len(sb):
            print(f"first difference: stream {i} has {len(sa)} launches in A and {len(sb)} in B; the common prefix agrees")
            return 1
    print(f"first difference: {len(a)} streams in A, {len(b)} in B; the common ones agree")
    return 1


if __name__ == "__main__":
    sys.exit(main())
