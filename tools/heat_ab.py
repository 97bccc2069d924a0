#!/usr/bin/env python3
"""What blending a net's score maps into a frame costs (dc_net_draw_heatmap: csrc/heat.cpp and heat_kernel in csrc/heat.hip, DESIGN
§4.5).  In ONE process, after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at
least 0.5 s with the windows listed, the routes of a group alternated in the same windows (the protocol of tools/track_ab.py).

Scene: the `prob` (14 joints) of ONE forward of the synthetic float32 ResNet-152 on a noise image, held; frames of the image's size,
544x736 and 1080x1920, in NV12 and in BGR24; both modes ("max" through caffe.HEAT_LUT with alpha x score, "joints" with the joint
colours), min_score 0.1.  Three routes to a picture of the maps:

  1. a DEVICE frame through `Net.draw_heatmap`: the tables and colours built on the host, one upload, one launch, the wait;
  2. a HOST frame through `Net.draw_heatmap`: the same plus the planes staged up and copied back;
  3. what a caller had before the entry existed, for a frame that lives on the device: `net.blobs["prob"].data` (the map downloaded, at
     fuse >= 2 through a layout pass), the planes downloaded, `Frame.to_bgr` (NV12), a float numpy bilinear upsampling of the 14 maps and
     a float blend on the host BGR image, the image uploaded.  The NV12 route leaves out the conversion back to NV12 that a caller
     feeding an encoder would also pay.  (Its picture is not byte-equal to the device's: it is the straightforward float version.)

Information only: no threshold hangs on these figures.

    python tools/heat_ab.py [--out profiles/heat_ab.txt]"""
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


def numpy_overlay(img, prob, scale, mode, lut, colors, alpha, min_score):
    """The float route: prob [J, Hm, Wm] upsampled bilinearly onto img's grid (uint8 [H, W, 3] BGR, in place) and blended."""
    h, w = img.shape[:2]
    hm, wm = prob.shape[1:]
    u = np.clip(((np.arange(w) + 0.5) * scale - 4.0) / 8.0, 0, wm - 1)
    v = np.clip(((np.arange(h) + 0.5) * scale - 4.0) / 8.0, 0, hm - 1)
    i0, j0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    i1, j1 = np.minimum(i0 + 1, wm - 1), np.minimum(j0 + 1, hm - 1)
    fx, fy = (u - i0).astype(np.float32)[None, :], (v - j0).astype(np.float32)[:, None]
    p = np.clip(prob, 0.0, 1.0)

    def up(c):
        top = c[j0][:, i0] * (1 - fx) + c[j0][:, i1] * fx
        bot = c[j1][:, i0] * (1 - fx) + c[j1][:, i1] * fx
        return top * (1 - fy) + bot * fy

    out = img.astype(np.float32)
    if mode == "max":
        s = up(p[0])
        for c in p[1:]:
            np.maximum(s, up(c), out=s)
        a = np.where(s >= min_score, s * (alpha / 256.0), 0.0)[:, :, None]
        col = lut[np.minimum(255, (s * 256.0).astype(np.int64))][:, :, ::-1].astype(np.float32)
        out = col * a + out * (1 - a)
    else:
        for k, c in enumerate(p):
            s = up(c)
            a = np.where(s >= min_score, s * (alpha / 256.0), 0.0)[:, :, None]
            out = np.asarray(colors[k % len(colors)][::-1], np.float32) * a + out * (1 - a)
    img[...] = np.rint(out).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import caffe
    import torch
    from deepcut_tools import deepercut_prototxt, synth_weights, write_caffemodel

    caffe.set_mode_gpu()
    caffe.set_device(0)
    path = os.path.join(tempfile.mkdtemp(), "synth152.caffemodel")
    write_caffemodel(path, "ResNet-152", synth_weights(152, seed=0))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    say("# blending prob (14 joints) of one held float32 forward into one frame at scale 1, alpha 192 x score, min_score 0.1; ms per synchronous "
        "call by the host clock, median of 5 windows >= 0.5 s [spread], routes alternated")
    lut = np.asarray(caffe.HEAT_LUT, np.uint8)
    for h, w in ((544, 736), (1080, 1920)):
        net = caffe.Net(deepercut_prototxt(152, h, w, 1), path, caffe.TEST, from_text=True)
        rs = np.random.RandomState(1)
        net.forward_images(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), 1.0, want=(), pose=False)
        shape = tuple(net.blobs["prob"].shape)
        for kind in ("nv12", "bgr24"):
            if kind == "nv12":
                planes = [rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, ((h + 1) // 2, (w + 1) // 2, 2)).astype(np.uint8)]
                host = caffe.Frame.nv12(*planes)
                dev = [torch.from_numpy(p).cuda() for p in planes]
                frame = caffe.Frame.nv12_device(dev[0].data_ptr(), dev[1].data_ptr(), h, w, w, 2 * ((w + 1) // 2))
            else:
                planes = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8)]
                host = caffe.Frame.bgr(planes[0])
                dev = [torch.from_numpy(planes[0]).cuda()]
                frame = caffe.Frame.bgr_device(dev[0].data_ptr(), h, w, 3 * w)
            torch.cuda.synchronize()
            image = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
            for mode in ("max", "joints"):
                style = dict(mode=mode, alpha=192, alpha_mode="score", min_score=0.1)

                def before():
                    prob = np.array(net.blobs["prob"].data[0], np.float32)
                    down = [t.cpu().numpy() for t in dev]
                    bgr = caffe.Frame.nv12(*down).to_bgr() if kind == "nv12" else down[0]
                    numpy_overlay(bgr, prob, 1.0, mode, lut, caffe.DRAW_JOINT_COLORS, 192, 0.1)
                    image.copy_(torch.from_numpy(bgr))
                    torch.cuda.synchronize()

                calls = {"device frame, Net.draw_heatmap": lambda: net.draw_heatmap(frame, 1.0, **style),
                         "host frame, Net.draw_heatmap": lambda: net.draw_heatmap(host, 1.0, **style),
                         "blobs[prob].data, planes down, to_bgr, numpy bilinear + blend, upload": before}
                for name, call in calls.items():
                    for _ in range(1 if name.startswith("blobs") else 5):
                        call()
                per = windows(calls)
                base = statistics.median(per["device frame, Net.draw_heatmap"])
                say("%d x %d %s, prob %s, mode %s" % (h, w, kind, "x".join(str(d) for d in shape), mode))
                for k, v in per.items():
                    say("  %s: %s ms per call%s; windows %s" % (k, spread(v), "" if k.startswith("device") else " (%.1fx the device frame's)" % (
                        statistics.median(v) / base), fmt(v)))
        del net
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
