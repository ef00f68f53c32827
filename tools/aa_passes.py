"""Per-pass times of the anti-aliasing trace kernels from a kernel trace of `tools/aa_timing.py --ab`
(rocprofv3 --kernel-trace --output-format csv ... -- python tools/aa_timing.py --ab ...).

A pass of level L launches the trace kernel L times (one launch per subdivision depth, k_aa.hip rt_antialias),
so the dispatches of a trace kernel, in start order, repeat with period L.  Prints, per kernel name (the generic
aa_trace_kernel instantiation, the specialised rt_spec_aa) and pass index, the median duration and the count.
usage: python tools/aa_passes.py KERNEL_TRACE_CSV [--level 3]"""
import argparse
import csv
import re
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--level", type=int, default=3)
    a = ap.parse_args()
    rows = {}
    with open(a.csv, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("kernel_name") or ""
            if "aa_trace_kernel" not in name and "rt_spec_aa" not in name:
                continue
            t0 = int(r.get("Start_Timestamp") or r.get("start_timestamp"))
            t1 = int(r.get("End_Timestamp") or r.get("end_timestamp"))
            m = re.search(r"aa_trace_kernel<[^>]*>|rt_spec_aa", name)     # the instantiation, without its argument list
            rows.setdefault(m.group(0), []).append((t0, t1 - t0))
    if not rows:
        sys.exit("no anti-aliasing trace dispatches in " + a.csv)
    for name, v in sorted(rows.items()):
        v.sort()
        if len(v) % a.level:
            print(f"{name}: {len(v)} dispatches are no multiple of level {a.level}; pass indices may be off")
        for p in range(a.level):
            d = [ns for i, (_, ns) in enumerate(v) if i % a.level == p]
            print(f"{name}  pass {p + 1}: median {statistics.median(d) / 1e6:.4f} ms over {len(d)} dispatches")
        per = [sum(ns for _, ns in v[i:i + a.level]) for i in range(0, len(v) - a.level + 1, a.level)]
        print(f"{name}  all {a.level} passes: median {statistics.median(per) / 1e6:.4f} ms")


if __name__ == "__main__":
    main()
