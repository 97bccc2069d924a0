#!/usr/bin/env python3
"""Bottom-up people at 544x736, batch 1, with the dense pairwise head and with the sparse one (DC_OPT_SPARSE_PAIRWISE, csrc/sparse_head.hip,
DESIGN §4.2): float32 and float16, max_det 16 and 64.  In ONE process, after warm-up, the two routes alternate: the dense route is
`forward_images` with all outputs + `assemble_people`, the sparse route `forward_images` with loc_pred and prob only + `assemble_people`
with the option set.  Per route the median of five windows of at least 0.5 s.
    python tools/sparse_pairwise_ab.py [--out profiles/sparse_pairwise_ab.txt]
    python tools/sparse_pairwise_ab.py --trace sparse --dtype f32 --max-det 16    # 50 calls of one route, for rocprofv3 --kernel-trace --stats"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python")):
    sys.path.insert(0, p)
import numpy as np

H, W = 544, 736


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", default="", help="dense | sparse: run 50 calls of that route only")
    ap.add_argument("--dtype", default="")
    ap.add_argument("--max-det", type=int, default=0)
    a = ap.parse_args()
    import caffe
    from deepcut_tools import deepercut_prototxt, synth_weights, write_caffemodel

    caffe.set_mode_gpu()
    caffe.set_device(0)
    path = os.path.join(tempfile.mkdtemp(), "synth152.caffemodel")
    write_caffemodel(path, "ResNet-152", synth_weights(152, seed=0))
    proto = deepercut_prototxt(152, H, W, 1)
    img = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    edges = np.array([(i, j) for i in range(14) for j in range(14) if i != j], np.int32)
    rs = np.random.RandomState(5)
    mean, std = rs.randn(182, 2) * 15, rs.uniform(4, 30, (182, 2))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# bottom-up people, %dx%d batch 1, synthetic ResNet-152: forward_images + assemble_people per call; median of 5 windows >= 0.5 s, routes alternated" % (H, W))
    for dtype in ([a.dtype] if a.dtype else ["f32", "f16"]):
        dense = caffe.Net(proto, path, caffe.TEST, from_text=True, dtype=dtype)
        sparse = caffe.Net(proto, path, caffe.TEST, from_text=True, dtype=dtype, want=["loc_pred", "prob"], sparse_pairwise=True)
        for md in ([a.max_det] if a.max_det else [16, 64]):
            kw = dict(scale=1.0, threshold=0.5, radius=1, max_det=md, edges=edges, mean=mean, std=std, max_cost=30.0, seed_threshold=0.6)

            def call(net):
                net.forward_images(img, 1.0, want=(), pose=False)
                return net.assemble_people(**kw)

            routes = {"dense": dense, "sparse": sparse}
            if a.trace:
                for _ in range(50):
                    call(routes[a.trace])
                continue
            for net in routes.values():
                for _ in range(5):
                    call(net)
            counts, _ = sparse.detect_parts(1.0, 0.5, 1, md)
            per = {k: [] for k in routes}
            for _ in range(5):
                for k, net in routes.items():
                    n, t0 = 0, time.perf_counter()
                    while True:
                        call(net)
                        n += 1
                        dt = time.perf_counter() - t0
                        if dt >= 0.5:
                            break
                    per[k].append(dt / n * 1e3)
            d, s = statistics.median(per["dense"]), statistics.median(per["sparse"])
            say("%s max_det %2d: %4d candidate cells; dense route %.3f ms, sparse route %.3f ms per call (%+.1f %%); windows dense %s sparse %s"
                % (dtype, md, int(counts.sum()), d, s, (s / d - 1) * 100, " ".join("%.3f" % v for v in per["dense"]), " ".join("%.3f" % v for v in per["sparse"])))
    if a.out and not a.trace:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
