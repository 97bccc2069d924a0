#!/usr/bin/env python3
"""DC_DEBUG_TIMING phase stamps of ONE float32 Winograd launch on a 3x3 shape of the 544x736 batch-1 forward, with the layer put on a given
form by set_tile (graph off, autotuning off): what a workgroup of that form spends in front of its K loop, in it and behind it.

    python tools/wino_f32_stamps.py [--shapes res4,res3] [--tiles wino_f23,wino_f23_mix]

A library that does not know a tile name (an older commit) skips it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python")):
    sys.path.insert(0, p)
import numpy as np

SHAPES = {"res4": (256, 256, 34, 46, 1), "res3": (128, 128, 68, 92, 1), "res2": (64, 64, 136, 184, 1), "res5": (512, 512, 34, 46, 2)}


def net_text(cin, cout, h, w, dil):
    L = ['name: "w"', 'input: "data"'] + ["input_dim: %d" % d for d in (1, cin, h, w)]
    L.append('layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: %d kernel_size: 3 '
             'pad: %d dilation: %d bias_term: false } }' % (cout, dil, dil))
    L.append('layer { name: "relu" type: "ReLU" bottom: "c" top: "c" }')
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="res4,res3")
    ap.add_argument("--tiles", default="wino_f23,wino_f23_w16,wino_f23_mix,wino_f23_mix_w16")
    a = ap.parse_args()
    os.environ["DC_AUTOTUNE"] = "0"
    os.environ.pop("DC_WINOGRAD", None)
    os.environ.setdefault("DC_DEBUG_TIMING", "0")  # (read once, at the first launch: every forward below reports launch 0, three runs each, the last one warm)
    import caffe

    caffe.set_mode_gpu()
    caffe.set_device(0)
    rs = np.random.RandomState(0)
    for name in a.shapes.split(","):
        cin, cout, h, w, dil = SHAPES[name]
        net = caffe.Net(net_text(cin, cout, h, w, dil), caffe.TEST, from_text=True, hipgraph=0)
        net.params["c"][0].data[...] = (rs.randn(cout, cin, 3, 3) / np.sqrt(9.0 * cin)).astype(np.float32)
        x = rs.randn(1, cin, h, w).astype(np.float32)
        net.blobs["data"].data[...] = x
        print("## %s: the lowering's tile" % name, file=sys.stderr, flush=True)
        net.forward()
        sig = [r["signature"] for r in net.tune_report() if "/3x3/" in r["signature"]][0]
        for tile in a.tiles.split(","):
            try:
                net.set_tile(sig, tile)
            except Exception as e:  # noqa: BLE001
                print("## %s %s: skipped (%s)" % (name, tile, e), flush=True)
                continue
            net.blobs["data"].data[...] = x
            print("## %s %s" % (name, tile), file=sys.stderr, flush=True)
            net.forward()


if __name__ == "__main__":
    main()
