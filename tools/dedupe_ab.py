#!/usr/bin/env python3
"""What duplicate suppression costs (stage E of the people assembly: dedupe_kernel in csrc/people.hip).  In ONE process,
after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at least 0.5 s with the
windows listed, the variants of a group alternated in the same windows (the protocol of tools/track_ab.py and tools/complete_ab.py):

  1. a 544x736 float32 net holding one forward of a noise image, max_det 16, max_people 32 — the call of tools/complete_ab.py:
     `assemble_people` with dedupe off and on (max_dist 0: the launch runs and suppresses nobody; and a max_dist that merges about a
     third of the pairs), and the same with completion on at fill_radius 2, which is where the stage is meant to run;
  2. the stand-alone call `caffe.dedupe_people` at n = P = 256, J = 14, on host arrays — upload, launch, download and wait: nobody
     similar (every pair is compared, everybody survives) and everybody similar to the best-scored person (one survivor; absorb on).

Information only: no threshold hangs on these figures.

    python tools/dedupe_ab.py [--out profiles/dedupe_ab.txt]"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python"), os.path.join(ROOT, "tools"),
          os.path.join(ROOT, "tests")):  # tests: the float64 restatement lists the distances a max_dist is chosen among
    sys.path.insert(0, p)
import numpy as np

import dedupe_ref as E
from track_ab import windows

H, W = 544, 736


def crowd(similar):
    """256 people of 14 joints: on a grid of 1024 px (nobody similar), or all within a pixel of the first (everybody similar)."""
    sk = np.array([[8.0 * j, 40.0 * (j % 2)] for j in range(14)])
    ppl = np.zeros((1, 256, 14, 3))
    for q in range(256):
        off = [q / 256.0, 0.0] if similar else [1024.0 * (q % 16), 1024.0 * (q // 16)]
        ppl[0, q, :, :2] = sk + off
        ppl[0, q, :, 2] = 1.0 - q / 512.0
    return ppl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import caffe
    from deepcut_tools import deepercut_prototxt, synth_weights, write_caffemodel

    caffe.set_mode_gpu()
    caffe.set_device(0)
    path = os.path.join(tempfile.mkdtemp(), "synth152.caffemodel")
    write_caffemodel(path, "ResNet-152", synth_weights(152, seed=0))
    proto = deepercut_prototxt(152, H, W, 1)
    edges = np.array([(i, j) for i in range(14) for j in range(14) if i != j], np.int32)
    rs = np.random.RandomState(5)
    mean, std = rs.randn(182, 2) * 15, rs.uniform(4, 30, (182, 2))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731

    def report(title, calls, off):
        for call in calls.values():
            for _ in range(20):
                call()
        per = windows(calls)
        base = statistics.median(per[off])
        say(title)
        for k, v in per.items():
            say("  %s: %s ms per call%s; windows %s" % (k, spread(v), "" if k == off else " (%+.4f ms on %s)" % (statistics.median(v) - base, off), fmt(v)))

    say("# duplicate suppression (stage E), synthetic ResNet-152 %dx%d float32 batch 1; ms per synchronous call by the host clock, median "
        "of 5 windows >= 0.5 s [spread], calls alternated" % (H, W))
    net = caffe.Net(proto, path, caffe.TEST, from_text=True)
    net.forward_images(np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8), 1.0, want=(), pose=False)
    kw = dict(scale=1.0, threshold=0.5, radius=1, max_det=16, edges=edges, mean=mean, std=std, max_cost=30.0, seed_threshold=0.6, max_people=32)
    fill = dict(fill_threshold=0.25, fill_radius=2, min_support=2)
    for title, extra in (("completion off", {}), ("completion on, fill_radius 2", dict(complete=fill))):
        q = dict(kw, **extra)
        base = net.assemble_people(**q)[0]["people"]
        Ds = E.all_distances(base, 3, 32.0)
        merge = dict(max_dist=Ds[len(Ds) // 3] if Ds else 0.0, min_common=3, min_size=32.0)
        nobody = dict(max_dist=0.0, min_common=3, min_size=32.0)
        left = len(net.assemble_people(dedupe=merge, **q)[0]["people"])
        assert len(net.assemble_people(dedupe=nobody, **q)[0]["people"]) == len(base)
        report("held forward of a noise image, max_det 16 max_people 32, %s (%d people; %d pairs with 3 joints in common; %d people left "
               "at max_dist %.4g)" % (title, len(base), len(Ds), left, merge["max_dist"]),
               {"assemble_people, dedupe off": lambda q=q: net.assemble_people(**q),
                "assemble_people, dedupe on, max_dist 0": lambda q=q: net.assemble_people(dedupe=nobody, **q),
                "assemble_people, dedupe on, max_dist %.4g" % merge["max_dist"]: lambda q=q: net.assemble_people(dedupe=merge, **q)},
               "assemble_people, dedupe off")
    del net

    n = np.array([256], np.int32)
    dd = dict(max_dist=0.5, min_common=3, min_size=32.0, absorb=True)
    apart, together = crowd(False), crowd(True)
    assert len(caffe.dedupe_people(apart, n, dedupe=dd)[0]["people"]) == 256 and len(caffe.dedupe_people(together, n, dedupe=dd)[0]["people"]) == 1
    one = crowd(False)[:, :1]
    report("stand-alone dedupe_people on host arrays, J = 14 (upload, one launch, downloads, wait)",
           {"n = P = 1": lambda: caffe.dedupe_people(one, n[:1] * 0 + 1, dedupe=dd),
            "n = P = 256, nobody similar": lambda: caffe.dedupe_people(apart, n, dedupe=dd),
            "n = P = 256, everybody similar": lambda: caffe.dedupe_people(together, n, dedupe=dd)}, "n = P = 1")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
