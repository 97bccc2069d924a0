#!/usr/bin/env python3
"""What redacting people in a frame costs (dc_redact_people: csrc/redact.cpp and redact_kernel in csrc/redact.hip).  In ONE
process, after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at least 0.5 s
with the windows listed, the routes of a group alternated in the same windows (the protocol of tools/draw_ab.py, whose scene this is).

Scene: 32 people of 14 joints (tools/draw_ab.py's), spread over the frame, at 544x736 and 1080x1920, in NV12 and in BGR24; region "head"
and region "body" (pose.HEAD_MPII14, pose.SKELETON_MPII14, the binding's placeholder radii), mosaic blocks of 8 and of 32.  Three routes:

  1. a DEVICE frame through `caffe.redact_people`: the primitives built and binned on the host, one upload, one launch, the wait;
  2. a HOST frame through `caffe.redact_people`: the same plus the planes staged up and copied back;
  3. what a caller had before the entry existed, for a frame that lives on the device: download the planes, `Frame.to_bgr` (NV12), a
     numpy mosaic on the host BGR image (discs and capsules masked inside their bounding boxes, the block means by reshaping), upload the
     image.  The NV12 route leaves out the conversion back to NV12 that a caller feeding an encoder would also pay.

Information only: no threshold hangs on these figures.

    python tools/redact_ab.py [--out profiles/redact_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np

from draw_ab import scene
from track_ab import windows


def numpy_mosaic(img, people, region, head, edges, geometry, block):
    """A mosaic of the region into a host BGR image with numpy: float coverage masked inside each primitive's bounding box, then the means
    of the blocks that hold a covered pixel.  Not the rule's bytes (no fixed point): the cost of the obvious host code."""
    h, w = img.shape[:2]
    covered = np.zeros((h, w), bool)

    def box(x0, y0, x1, y1, r):
        return max(0, int(x0 - r)), max(0, int(y0 - r)), min(w, int(x1 + r) + 2), min(h, int(y1 + r) + 2)

    def capsule(ax, ay, bx, by, r):
        x0, y0, x1, y1 = box(min(ax, bx), min(ay, by), max(ax, bx), max(ay, by), r)
        if x0 >= x1 or y0 >= y1:
            return
        yy, xx = np.ogrid[y0:y1, x0:x1]
        dx, dy = bx - ax, by - ay
        t = np.clip(((xx - ax) * dx + (yy - ay) * dy) / max(dx * dx + dy * dy, 1e-9), 0.0, 1.0)
        covered[y0:y1, x0:x1] |= (xx - ax - t * dx) ** 2 + (yy - ay - t * dy) ** 2 <= r * r

    lo, hi = geometry["min_radius"], geometry["max_radius"]
    for person in people:
        a, b = person[head[0], :2], person[head[1], :2]
        c = (a + b) / 2.0
        capsule(c[0], c[1], c[0], c[1], min(max(geometry["head_scale"] * float(np.hypot(*(b - a))), lo), hi))
        if region == "body":
            r = min(max(geometry["body_scale"] * float(np.ptp(person[:, :2], axis=0).max()), lo), 64.0)
            for i, j in edges:
                capsule(person[i, 0], person[i, 1], person[j, 0], person[j, 1], r)
    hb, wb = -(-h // block), -(-w // block)
    full = np.zeros((hb * block, wb * block), bool)
    full[:h, :w] = covered
    chosen = full.reshape(hb, block, wb, block).any(axis=(1, 3))
    for by, bx in zip(*np.nonzero(chosen)):
        v = img[by * block:(by + 1) * block, bx * block:(bx + 1) * block]
        v[...] = (v.reshape(-1, 3).sum(axis=0) + v.shape[0] * v.shape[1] // 2) // (v.shape[0] * v.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import caffe
    import torch
    from pose import HEAD_MPII14, SKELETON_MPII14

    caffe.set_mode_gpu()
    caffe.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    tw, th, chunk = caffe.draw_limits()
    geometry = dict(caffe.REDACT_DEFAULTS)
    say("# redacting 32 people (head pair %s, the limbs of SKELETON_MPII14, %s) in one frame, effect mosaic; tiles %d x %d, chunk %d; ms per "
        "synchronous call by the host clock, median of 5 windows >= 0.5 s [spread], routes alternated" % (
            HEAD_MPII14, ", ".join("%s %g" % kv for kv in sorted(geometry.items())), tw, th, chunk))
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
            for region in ("head", "body"):
                for block in (8, 32):
                    style = dict(region=region, head=HEAD_MPII14, edges=SKELETON_MPII14, block=block, **geometry)

                    def before():
                        down = [t.cpu().numpy() for t in dev]
                        bgr = caffe.Frame.nv12(*down).to_bgr() if kind == "nv12" else down[0]
                        numpy_mosaic(bgr, people, region, HEAD_MPII14, SKELETON_MPII14, geometry, block)
                        image.copy_(torch.from_numpy(bgr))
                        torch.cuda.synchronize()

                    calls = {"device frame, redact_people": lambda: caffe.redact_people(frame, people, **style),
                             "host frame, redact_people": lambda: caffe.redact_people(host, people, **style),
                             "download, to_bgr, numpy mosaic, upload": before}
                    for call in calls.values():
                        for _ in range(3):
                            call()
                    per = windows(calls)
                    base = statistics.median(per["device frame, redact_people"])
                    say("%d x %d %s, region %s, block %d" % (h, w, kind, region, block))
                    for k, v in per.items():
                        say("  %s: %s ms per call%s; windows %s" % (k, spread(v), "" if k.startswith("device") else " (%.1fx the device frame's)" % (
                            statistics.median(v) / base), fmt(v)))
            # the frames were redacted with every style in turn, by both entries alike: they hold one picture
            for got, want in zip(dev, planes):
                assert np.array_equal(got.cpu().numpy(), want), "the device frame and the host frame differ"
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
