#!/usr/bin/env python
"""The float32 Winograd launches of a rocprofv3 --kernel-trace result, per kernel AND grid: the kernel name alone does not tell the res5
launches (768 workgroups on 4 x 8-tile blocks, 512 on 5 x 6) from the res2 / res3 ones.  Per group: dispatches, average / median / min / max
and the standard deviation of the per-dispatch durations (the spread a faster launch has to clear).
    python tools/wino_trace_by_grid.py x_results.db [first dispatches to skip per group, default 0]"""
import collections
import os
import sqlite3
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_names  # noqa: E402


def main(path, skip=0):
    c = sqlite3.connect(path)
    # the rocpd `kernels` view of rocprofv3: grid_x/y/z count work-ITEMS, workgroup_x/y/z the items of a workgroup
    cols = [d[1] for d in c.execute("pragma table_info('kernels')")]
    assert all(k in cols for k in ("name", "start", "end", "grid_x", "workgroup_x")), cols
    groups = collections.OrderedDict()
    for name, g, w, s, e in c.execute("select name, grid_x * grid_y * grid_z, workgroup_x * workgroup_y * workgroup_z, start, end from kernels order by start"):
        if "wino_f23_kernel" in name:
            groups.setdefault((kernel_names.label(name), g // w), []).append((e - s) / 1e3)
    print("# %s: float32 Winograd dispatches by kernel and workgroups (durations in us%s)" % (os.path.basename(path), ", first %d of each group skipped" % skip if skip else ""))
    print("%-64s %6s %6s %8s %8s %8s %8s %8s" % ("kernel", "wgs", "n", "avg", "median", "min", "max", "stdev"))
    for (label, wgs), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
        d = d[skip:] or d
        print("%-64s %6d %6d %8.2f %8.2f %8.2f %8.2f %8.2f" % (label[:64], wgs, len(d), sum(d) / len(d), statistics.median(d), min(d), max(d), statistics.pstdev(d)))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)
