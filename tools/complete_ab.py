#!/usr/bin/env python3
"""What the completion pass costs (stage D of the people assembly: complete_kernel in csrc/people.hip).  In ONE process,
after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at least 0.5 s with the
windows listed, the variants of a group alternated in the same windows (the protocol of tools/track_ab.py):

  1. a 544x736 float32 net holding one forward of a noise image, max_det 16, max_people 32 — the call of tools/track_ab.py, whose
     `Net.assemble_people` figure in profiles/track_ab.txt is the one to compare with: `assemble_people` with completion off, with
     completion on at fill_radius 2 and 16 (the people of a noise image lack most of their joints), and `track_people` without
     completion, for the tracker's own added launch in the same run;
  2. a planted scene on a DC_OPT_FUSE 0 net of the same size: 32 people of 14 joints, two score peaks of each below the assembly's
     threshold, so that each person lacks exactly two joints and stage D fills both (checked).  32 people of one joint each need 32
     candidates per joint, so this scene runs at max_det 32: completion off, on at fill_radius 2 and at 16.  (At fill_radius 16 a
     window reaches the neighbours' dim peaks, which have the same score, and the tie goes to the lower cell: what is checked is the
     number of fills, which is what the time depends on.)

    python tools/complete_ab.py [--out profiles/complete_ab.txt]"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np

from track_ab import windows

H, W = 544, 736
LOWERED = (3, 9)


def planted(h, w, edges, mean, std):
    """32 people on an 8 x 4 grid of the 68 x 92 map, joint j of a person on a cell of its own (14 rows, two columns), every held cell
    predicting the person's other joints on every edge; the peaks of joints 3 and 9 at 0.3125, the others at 0.875."""
    from oracle import multiperson as M

    prob = np.zeros((14, h, w), np.float32)
    loc = np.zeros((28, h, w), np.float32)
    nxt = np.zeros((2 * len(edges), h, w), np.float32)
    for q in range(32):
        r0, c0 = 2 + 16 * (q // 8), 3 + 11 * (q % 8)
        cells = [(r0 + j, c0 + 2 * (j % 2)) for j in range(14)]
        pts = [np.array([c * 8.0 + 4.0, r * 8.0 + 4.0]) for r, c in cells]
        for j, (r, c) in enumerate(cells):
            prob[j, r, c] = 0.3125 if j in LOWERED else 0.875
        for l, (a, c) in enumerate(edges):
            _, nt = M.encode_targets(pts[a], pts[c], cells[a], 1.0, mean[l], std[l])
            nxt[2 * l:2 * l + 2, cells[a][0], cells[a][1]] = nt
    return prob, loc, nxt


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
    fills = {2: dict(fill_threshold=0.25, fill_radius=2, min_support=2), 16: dict(fill_threshold=0.25, fill_radius=16, min_support=2)}
    say("# completion pass, synthetic ResNet-152 %dx%d float32 batch 1; ms per synchronous call by the host clock, median of 5 windows "
        ">= 0.5 s [spread], calls alternated" % (H, W))

    def group(title, net, kw, tracker=None):
        calls = {"off": lambda: net.assemble_people(**kw)}
        for r, f in fills.items():
            calls["on, fill_radius %d" % r] = lambda f=f: net.assemble_people(complete=f, **kw)
        if tracker is not None:
            calls["track_people, off"] = lambda: net.track_people(tracker, **kw)
        for call in calls.values():
            for _ in range(20):
                call()
        found = len(calls["off"]()[0]["people"])
        filled = {r: int(net.assemble_people(complete=f, **kw)[0]["filled"].sum()) for r, f in fills.items()}
        per = windows(calls)
        off = statistics.median(per["off"])
        say("%s (%d people found; joints filled at fill_radius 2 / 16: %d / %d)" % (title, found, filled[2], filled[16]))
        for k, v in per.items():
            say("  %s%s: %s ms per call%s; windows %s" % ("" if k.startswith("track_people") else "assemble_people ", k, spread(v), "" if k == "off" else " (%+.4f ms on off)" % (statistics.median(v) - off), fmt(v)))
        return found, filled

    net = caffe.Net(proto, path, caffe.TEST, from_text=True)
    net.forward_images(np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8), 1.0, want=(), pose=False)
    kw = dict(scale=1.0, threshold=0.5, radius=1, max_det=16, edges=edges, mean=mean, std=std, max_cost=30.0, seed_threshold=0.6, max_people=32)
    group("held forward of a noise image, max_det 16 max_people 32", net, kw, caffe.Tracker(n_joints=14, slots=1, max_tracks=64))
    del net

    net = caffe.Net(proto, path, caffe.TEST, from_text=True, fuse=0)
    net.forward_batch(np.zeros((1, 3, H, W), np.float32), want=())
    h, w = net.blobs["prob"].shape[2:]
    net.blobs["prob"].data[0], net.blobs["loc_pred"].data[0], net.blobs["next_pred"].data[0] = planted(h, w, edges, mean, std)
    kw = dict(kw, max_det=32, max_cost=20.0, min_joints=2)
    found, filled = group("planted scene, 32 people lacking joints %d and %d each, max_det 32 max_people 32" % LOWERED, net, kw)
    assert found == 32 and filled == {2: 64, 16: 64}, (found, filled)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
