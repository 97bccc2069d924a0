#!/usr/bin/env python3
"""What drawing people into a frame costs (dc_draw_people: csrc/draw.cpp and draw_kernel in csrc/draw.hip).  In ONE process,
after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at least 0.5 s with the
windows listed, the routes of a group alternated in the same windows (the protocol of tools/track_ab.py).

Scene: 32 people of 14 joints with pose.SKELETON_MPII14 (448 limbs and 448 joints), spread over the frame, at 544x736 and 1080x1920, in
NV12 and in BGR24.  Three routes to the same picture:

  1. a DEVICE frame through `caffe.draw_people`: the primitive list built and binned on the host, one upload, one launch, the wait;
  2. a HOST frame through `caffe.draw_people`: the same plus the planes staged up and copied back;
  3. what a caller had before the entry existed, for a frame that lives on the device: download the planes, `Frame.to_bgr` (NV12), numpy
     discs and capsules on the host BGR image, upload the image.  The numpy drawing here masks only each primitive's bounding box — a
     kinder baseline than the demo's `draw_disc`, which masks the whole image per joint — and the NV12 route leaves out the conversion
     back to NV12 that a caller feeding an encoder would also pay.

Information only: no threshold hangs on these figures.

    python tools/draw_ab.py [--out profiles/draw_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np

from track_ab import windows

# one standing person in a unit box (x in 0..1, y in 0..1), MPII order: r ankle, knee, hip; l hip, knee, ankle; r wrist, elbow,
# shoulder; l shoulder, elbow, wrist; upper neck; head top
PERSON = np.array([(0.35, 1.0), (0.36, 0.78), (0.38, 0.55), (0.62, 0.55), (0.64, 0.78), (0.65, 1.0), (0.15, 0.5), (0.2, 0.36), (0.3, 0.2), (0.7, 0.2),
                   (0.8, 0.36), (0.85, 0.5), (0.5, 0.17), (0.5, 0.0)])


def scene(h, w, people=32):
    rs = np.random.RandomState(3)
    out = np.ones((people, 14, 3))
    size = h / 3.0
    for q in range(people):
        at = (rs.uniform(0, w - size * 0.5), rs.uniform(0, h - size))
        out[q, :, :2] = PERSON * (size * 0.5, size) + at + rs.uniform(-2, 2, (14, 2))
    return out


def numpy_overlay(img, people, edges, rj, rl, colors):
    """Discs and capsules into a host BGR image with numpy, each masked inside its own bounding box."""
    h, w = img.shape[:2]

    def box(x0, y0, x1, y1, r):
        return max(0, int(x0 - r)), max(0, int(y0 - r)), min(w, int(x1 + r) + 2), min(h, int(y1 + r) + 2)

    for q, person in enumerate(people):
        c = colors[q % len(colors)][::-1]
        for a, b in edges:
            (ax, ay), (bx, by) = person[a, :2], person[b, :2]
            x0, y0, x1, y1 = box(min(ax, bx), min(ay, by), max(ax, bx), max(ay, by), rl)
            if x0 >= x1 or y0 >= y1:
                continue
            yy, xx = np.ogrid[y0:y1, x0:x1]
            dx, dy = bx - ax, by - ay
            t = np.clip(((xx - ax) * dx + (yy - ay) * dy) / max(dx * dx + dy * dy, 1e-9), 0.0, 1.0)
            img[y0:y1, x0:x1][(xx - ax - t * dx) ** 2 + (yy - ay - t * dy) ** 2 <= rl * rl] = c
        for j in range(person.shape[0]):
            cx, cy = person[j, :2]
            x0, y0, x1, y1 = box(cx, cy, cx, cy, rj)
            if x0 >= x1 or y0 >= y1:
                continue
            yy, xx = np.ogrid[y0:y1, x0:x1]
            img[y0:y1, x0:x1][(xx - cx) ** 2 + (yy - cy) ** 2 <= rj * rj] = c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import caffe
    import torch
    from pose import SKELETON_MPII14

    caffe.set_mode_gpu()
    caffe.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    tw, th, chunk = caffe.draw_limits()
    say("# drawing 32 people x (14 joints + 14 limbs of SKELETON_MPII14) into one frame, joint_radius 4 limb_radius 2 alpha 256; tiles %d x %d, "
        "chunk %d; ms per synchronous call by the host clock, median of 5 windows >= 0.5 s [spread], routes alternated" % (tw, th, chunk))
    style = dict(edges=SKELETON_MPII14, joint_radius=4.0, limb_radius=2.0, palette=caffe.DRAW_ID_COLORS)
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
                numpy_overlay(bgr, people, SKELETON_MPII14, 4.0, 2.0, caffe.DRAW_ID_COLORS)
                image.copy_(torch.from_numpy(bgr))
                torch.cuda.synchronize()

            calls = {"device frame, draw_people": lambda: caffe.draw_people(frame, people, **style),
                     "host frame, draw_people": lambda: caffe.draw_people(host, people, **style),
                     "download, to_bgr, numpy overlay, upload": before}
            for call in calls.values():
                for _ in range(3):
                    call()
            # opaque primitives: drawing again changes nothing, so after the warm-up both frames hold the one picture
            for got, want in zip(dev, planes):
                assert np.array_equal(got.cpu().numpy(), want), "the device frame and the host frame differ"
            per = windows(calls)
            base = statistics.median(per["device frame, draw_people"])
            say("%d x %d %s" % (h, w, kind))
            for k, v in per.items():
                say("  %s: %s ms per call%s; windows %s" % (k, spread(v), "" if k.startswith("device") else " (%.1fx the device frame's)" % (
                    statistics.median(v) / base), fmt(v)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
