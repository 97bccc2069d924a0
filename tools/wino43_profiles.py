#!/usr/bin/env python
"""The two rocprofv3 summaries of profiles/wino_f43_trace.txt from CSV output (--output-format csv):
    python tools/wino43_profiles.py trace  <parent t_kernel_trace.csv> <change t_kernel_trace.csv>
    python tools/wino43_profiles.py pmc    <parent c_counter_collection.csv> <change c_counter_collection.csv>
trace: per kernel and grid size (the shape), calls and average microseconds, the 3x3 layers' kernels first.
pmc:   every collected counter (SQ_VALU_MFMA_BUSY_CYCLES first) summed over the dispatches of one forward (forwards = max-pool dispatches)."""
import collections
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_names  # noqa: E402


def label(name):
    if "wino43_input" in name:
        return "wino43_input (B^T d B, once per layer)"
    if "wino43_output" in name:
        return "wino43_output (A^T M A + affine + ReLU)"
    if "ws1x1f_kernel" in name and re.search(r"ws1x1f_kernel<\d+, \d+, false, false, false, true>", name):
        return "ws1x1f batched K=%s (wino_f43: the 36 products)" % name.split("ws1x1f_kernel<")[1].split(",")[0]
    if "ws1x1f_kernel" in name:
        return "ws1x1f K=%s (streaming 1x1)" % name.split("ws1x1f_kernel<")[1].split(",")[0]
    if "conv_gemm_kernel" in name or "wino_f23" in name:
        return kernel_names.label(name)
    return name.split("(")[0][:60]


def trace(path):
    rows = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        k = (label(r["Kernel_Name"]), int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])))
        a = rows.setdefault(k, [0, 0.0, 1e30, 0.0])
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        a[0] += 1
        a[1] += us
        a[2] = min(a[2], us)
        a[3] = max(a[3], us)
    return rows


def show_trace(tag, rows):
    tot = sum(a[1] for a in rows.values())
    print("## %s: %.1f us of kernels over %d dispatches" % (tag, tot, sum(a[0] for a in rows.values())))
    print("%-66s %10s %6s %9s %8s %8s %6s" % ("kernel", "workgroups", "calls", "total_us", "avg_us", "min_us", "pct"))
    wino = lambda k: "wino" in k[0] or "batched" in k[0]  # noqa: E731
    for k, a in sorted(rows.items(), key=lambda kv: (not wino(kv[0]), -kv[1][1])):
        if a[1] / tot < 0.004 and not wino(k):
            continue
        print("%-66s %10d %6d %9.1f %8.2f %8.2f %6.2f" % (k[0][:66], k[1], a[0], a[1], a[1] / a[0], a[2], 100 * a[1] / tot))


def pmc(path):
    sums = collections.Counter()
    pools = set()
    for r in csv.DictReader(open(path)):
        sums[r["Counter_Name"]] += float(r["Counter_Value"])
        if "maxpool" in r["Kernel_Name"]:
            pools.add(r["Dispatch_Id"])
    return sums, max(1, len(pools))


if __name__ == "__main__":
    what, parent, change = sys.argv[1:4]
    if what == "trace":
        for tag, p in (("parent", parent), ("change", change)):
            show_trace(tag, trace(p))
    else:
        for tag, p in (("parent", parent), ("change", change)):
            s, n = pmc(p)
            print("%s: %d forwards; per forward %s" % (tag, n, ", ".join("%s %.4g" % (c, s[c] / n) for c in sorted(s, key=lambda c: (c != "SQ_VALU_MFMA_BUSY_CYCLES", c)))))
