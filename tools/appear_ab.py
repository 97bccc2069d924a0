#!/usr/bin/env python3
"""What the appearance descriptor and the tracker's appearance steps cost (csrc/appearance.hip, csrc/track.hip).  In ONE
process, after warm-up, every figure a host clock around a synchronous call, ms per call, the median of five windows of at least 0.5 s
with their spread, the calls of a group alternated in the same windows:
  `describe_people` for 32 people (the MPII torso, the placeholder style) at 544x736 and at 1080x1920, NV12 and BGR24, on device frames
  and on host frames (which are staged up on every call);
  the stand-alone `Tracker.update` at T 64, P = n = 32 and at T = P = n = 256, everybody near their own track, on a tracker with
  appearance off and on one with it on and fed descriptors (every update then updates n models; nobody is born, so step 7' idles).
    python tools/appear_ab.py [--out profiles/appear_ab.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python")):
    sys.path.insert(0, p)
import numpy as np

TORSO = ((8, 2), (9, 3), (8, 9), (2, 3))


def windows(calls, n_windows=5, seconds=0.5):
    """calls: {name: callable}, alternated -> {name: [ms per call of every window]}"""
    per = {k: [] for k in calls}
    for _ in range(n_windows):
        for k, call in calls.items():
            n, t0 = 0, time.perf_counter()
            while True:
                call()
                n += 1
                dt = time.perf_counter() - t0
                if dt >= seconds:
                    break
            per[k].append(dt / n * 1e3)
    return per


def torsos(n, h, w):
    """n people on a grid over the frame, torsos of about a sixth of the frame's height"""
    r = np.random.RandomState(3)
    side = int(np.ceil(np.sqrt(n)))
    out = np.zeros((n, 14, 3), np.float64)
    th, tw = h / 6.0, h / 12.0
    for q in range(n):
        cx, cy = (q % side + 0.5) * w / side, (q // side + 0.5) * h / side
        for j, (sx, sy) in ((8, (-1, -1)), (9, (1, -1)), (2, (-1, 1)), (3, (1, 1))):
            out[q, j] = (cx + sx * tw / 2 + r.uniform(-4, 4), cy + sy * th / 2 + r.uniform(-4, 4), 0.8)
    return out


def near(n):
    """n people on a 400-pixel grid, then the same people moved by up to 3 pixels a joint, in another order (tools/track_ab.py's)"""
    r = np.random.RandomState(1)
    out = np.zeros((1, n, 14, 3), np.float64)
    side = int(np.ceil(np.sqrt(n)))
    for q in range(n):
        out[0, q, :, :2] = (400.0 * (q % side), 400.0 * (q // side)) + r.uniform(-40, 40, (14, 2))
        out[0, q, :, 2] = 0.5
    nxt = out.copy()
    nxt[0, :, :, :2] += r.uniform(-3, 3, (n, 14, 2))
    order = r.permutation(n)
    return out, nxt[:, order], order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import caffe

    caffe.set_mode_gpu()
    caffe.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    say("# appearance: ms per synchronous call by the host clock, median [min - max] of 5 windows >= 0.5 s, calls alternated")
    rs = np.random.RandomState(0)
    for h, w in ((544, 736), (1080, 1920)):
        people = torsos(32, h, w)
        bgr = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        y, uv = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)
        d_bgr, d_y, d_uv = (torch.from_numpy(x).cuda() for x in (bgr, y, uv))
        torch.cuda.synchronize()
        frames = {"BGR24 host": caffe.Frame.bgr(bgr), "BGR24 device": caffe.Frame.bgr_device(d_bgr.data_ptr(), h, w, 3 * w),
                  "NV12 host": caffe.Frame.nv12(y, uv), "NV12 device": caffe.Frame.nv12_device(d_y.data_ptr(), d_uv.data_ptr(), h, w, w, w)}
        calls = {k: (lambda f=f: caffe.describe_people(f, people, edges=TORSO)) for k, f in frames.items()}
        pixels = {k: int(call()[:, 0].sum()) for k, call in calls.items()}
        for call in calls.values():
            for _ in range(20):
                call()
        per = windows(calls)
        for k, v in per.items():
            say("describe_people %dx%d %s, 32 people (%d region pixels): %s ms per call" % (h, w, k, pixels[k], spread(v)))
    for name, T, n in (("T 64, P = n = 32", 64, 32), ("T = P = n = 256", 256, 256)):
        first, second, order = near(n)
        hist = np.zeros((n, 3, 16), np.int32)
        for q in range(n):
            hist[q] = np.stack([np.bincount(rs.randint(q % 8, q % 8 + 8, 500), minlength=16) for _ in range(3)])
        desc = (hist[None], hist[order][None])
        calls = {}
        for mode in ("off", "on"):
            trk = caffe.Tracker(n_joints=14, slots=1, max_tracks=T, max_misses=1000, appearance=(mode == "on") or None)
            kw = [dict(desc=d) for d in desc] if mode == "on" else [dict(), dict()]
            ids0, ids1 = trk.update(first, **kw[0])[0], trk.update(second, **kw[1])[0]
            assert sorted(ids0[0].tolist()) == list(range(n)) and sorted(ids1[0].tolist()) == list(range(n)), (name, mode)  # all born, all matched
            state = {"k": 1}

            def call(trk=trk, frames=(first, second), kw=kw, state=state):
                state["k"] ^= 1
                trk.update(frames[state["k"]], **kw[state["k"]])

            for _ in range(10):
                call()
            calls[mode] = call
        per = windows(calls)
        off, on = statistics.median(per["off"]), statistics.median(per["on"])
        say("Tracker.update %s, everybody near their own track: appearance off %s ms, on %s ms per call (%+.4f ms, x %.2f)"
            % (name, spread(per["off"]), spread(per["on"]), on - off, on / off))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
