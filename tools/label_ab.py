#!/usr/bin/env python3
"""What labelling people in a frame costs (dc_label_people: csrc/label.cpp and label_kernel in csrc/label.hip).  In ONE
process, after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at least 0.5 s
with the windows listed, the routes of a group alternated in the same windows (the protocol of tools/draw_ab.py).

Scene: the 32 people of tools/draw_ab.py with ids 100 .. 131, scale 2, the other LABEL_DEFAULTS, at 544x736 and 1080x1920, in NV12 and
in BGR24.  Three routes:

  1. a DEVICE frame through `caffe.label_people`: the labels made and binned on the host, one upload, one launch, the wait;
  2. a HOST frame through `caffe.label_people`: the same plus the planes staged up and copied back;
  3. what a caller has without the entry, for a frame that lives on the device: download the planes, `Frame.to_bgr` (NV12), the numpy
     restatement of the rule (tests/label_ref.py) on the host BGR image, upload the image.  The project has no other text renderer; the
     NV12 route leaves out the conversion back to NV12 that a caller feeding an encoder would also pay.

Information only: no threshold hangs on these figures.

    python tools/label_ab.py [--out profiles/label_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python"), os.path.join(ROOT, "tools"),
          os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np

from draw_ab import scene
from track_ab import windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import caffe
    import label_ref
    import torch

    caffe.set_mode_gpu()
    caffe.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    say("# labelling 32 people (ids 100 .. 131, three digits) in one frame, scale 2, gap 2, alpha_text 256, alpha_plate 160, plate by id; "
        "ms per synchronous call by the host clock, median of 5 windows >= 0.5 s [spread], routes alternated")
    ids = 100 + np.arange(32, dtype=np.int64)
    style = dict(caffe.LABEL_DEFAULTS, palette=caffe.DRAW_ID_COLORS)
    for h, w in ((544, 736), (1080, 1920)):
        people = scene(h, w)
        rs = np.random.RandomState(1)
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

            def before():
                down = [t.cpu().numpy() for t in dev]
                bgr = caffe.Frame.nv12(*down).to_bgr() if kind == "nv12" else down[0]
                label_ref.label_bgr(bgr, label_ref.labels(people, h, w, ids=ids, **style))
                image.copy_(torch.from_numpy(bgr))
                torch.cuda.synchronize()

            calls = {"device frame, label_people": lambda: caffe.label_people(frame, people, ids=ids, **style),
                     "host frame, label_people": lambda: caffe.label_people(host, people, ids=ids, **style),
                     "download, to_bgr, numpy restatement, upload": before}
            for call in calls.values():
                for _ in range(2):
                    call()
            per = windows(calls)
            base = statistics.median(per["device frame, label_people"])
            say("%d x %d %s" % (h, w, kind))
            for k, v in per.items():
                say("  %s: %s ms per call%s; windows %s" % (k, spread(v), "" if k.startswith("device") else " (%.1fx the device frame's)" % (
                    statistics.median(v) / base), fmt(v)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
