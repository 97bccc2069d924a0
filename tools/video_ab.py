#!/usr/bin/env python3
"""What the video path delivers end to end (deepcut_tools.VideoPipeline over dc_net_track_frames_async).  In ONE process
on synthetic ResNet-152 weights at 544x736, host NV12 frames in pinned memory, max_det 16 and max_people 32, tracked people per frame:
 (a) the baseline: `forward_images` + `Net.track_people`, one frame per synchronous call;
 (b) `VideoPipeline` float32 at depth 1, 2, 3, 4, batch 1;
 (c) `VideoPipeline` float16 at depth 1 and 2, batch 1, 4 and 8;
 (d) `Tracker.update` of 8 frames of P = n = 32 into ONE slot as one call (slot map) against 8 calls.
Every figure of (a)-(c) is frames per second by the host clock over a window in which frames are submitted without pause and then
drained; (d) is ms per 8 frames.  The variants are alternated; the median of five windows of at least 0.5 s, with the windows listed.
    python tools/video_ab.py [--out profiles/video_ab.txt]
With --overlay: `VideoPipeline` with draw + redact at depth 1, 2, 3, float32 and float16, on host NV12 frames in pinned
memory and on device NV12 frames — the host route (in_chain=False: the synchronous redact_people / draw_people when a request is
collected), in_chain=True (the overlays enqueued with the request) and no overlay at all (the ceiling) alternated in the same windows.
    python tools/video_ab.py --overlay [--out profiles/video_overlay_ab.txt]
With --overlay --labels: the same, with the label overlay (ids as text, LABEL_DEFAULTS) added to the skeleton and the mosaic.
    python tools/video_ab.py --overlay --labels [--out profiles/video_overlay_labels_ab.txt]"""
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


def windows(runs, n_windows=5, seconds=0.5):
    """runs: {name: callable(seconds) -> (units done, seconds taken)}, alternated -> {name: [units per second of every window]}"""
    per = {k: [] for k in runs}
    for _ in range(n_windows):
        for k, run in runs.items():
            n, dt = run(seconds)
            per[k].append(n / dt)
    return per


def overlay(caffe, VideoPipeline, nets, host_frames, stats, akw, say, fmt, labels=False):
    """The overlay routes of VideoPipeline: frames/s with no overlay, with draw + redact on the host route, and with them in the chain."""
    import torch

    tensors = [(torch.from_numpy(np.array(f._keep[0])).cuda(), torch.from_numpy(np.array(f._keep[1])).cuda()) for f in host_frames]
    torch.cuda.synchronize()
    device_frames = [caffe.Frame.nv12_device(y.data_ptr(), uv.data_ptr(), H, W, W, W) for y, uv in tensors]
    sources = {"host NV12 (pinned)": host_frames, "device NV12": device_frames}
    styles = dict(draw=dict(alpha=160), redact=dict(region="head_or_body", block=8))
    if labels:
        styles["labels"] = True
    routes = {"no overlay": dict(), "host route": dict(styles), "in_chain": dict(styles, in_chain=True)}
    people = {}

    def pipeline(dtype, depth, frames, route):
        pipe = VideoPipeline(nets[dtype], caffe.Tracker(n_joints=14, slots=1, max_tracks=64), depth=depth, batch=1, stats=stats, scale=1.0,
                             **dict(akw, **routes[route]))

        def run(seconds):
            n, got, t0 = 0, 0, time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                pipe.submit(frames[n % len(frames)])
                n += 1
                while pipe._done:
                    people[route] = len(pipe.wait_one()[1])
                    got += 1
            got += len(pipe.drain())
            assert got == n
            return n, time.perf_counter() - t0

        return run

    say("# overlays in the video path: draw (MPII skeleton, alpha 160) + redact (head_or_body, mosaic, block 8)" +
        (" + labels (ids, LABEL_DEFAULTS: scale 2)" if labels else "") + " on every frame; frames are "
        "overwritten again and again (a mosaic of a mosaic costs what a mosaic costs)")
    for dtype in ("f32", "f16"):
        for where, frames in sources.items():
            for depth in (1, 2, 3):
                runs = {route: pipeline(dtype, depth, frames, route) for route in routes}
                for run in runs.values():
                    run(0.2)
                per = windows(runs)
                med = {k: statistics.median(v) for k, v in per.items()}
                say("%s, %s, depth %d: " % (dtype, where, depth) + "; ".join(
                    "%s %.1f frames/s [%.1f - %.1f]" % (k, med[k], min(per[k]), max(per[k])) for k in routes) +
                    "; in_chain / host route %.3f, in_chain / no overlay %.3f" % (med["in_chain"] / med["host route"], med["in_chain"] / med["no overlay"]))
                for k in routes:
                    say("    windows %s: %s" % (k, fmt(per[k])))
    say("# people in the last frame collected: %r" % (people,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--overlay", action="store_true", help="the overlay routes of VideoPipeline instead of (a)-(d)")
    ap.add_argument("--labels", action="store_true", help="with --overlay: the label overlay added to the skeleton and the mosaic")
    a = ap.parse_args()
    import caffe
    from deepcut_tools import VideoPipeline, deepercut_prototxt, synth_weights, write_caffemodel

    caffe.set_mode_gpu()
    caffe.set_device(0)
    path = os.path.join(tempfile.mkdtemp(), "synth152.caffemodel")
    write_caffemodel(path, "ResNet-152", synth_weights(152, seed=0))
    nets = {"f32": caffe.Net(deepercut_prototxt(152, H, W, 1), path, caffe.TEST, from_text=True),
            "f16": caffe.Net(deepercut_prototxt(152, H, W, 1), path, caffe.TEST, from_text=True, dtype="f16")}
    rs = np.random.RandomState(0)
    frames = []
    for _ in range(16):  # pinned planes: the DMA engines take them where they are
        y, uv = caffe.pinned_empty((H, W), np.uint8), caffe.pinned_empty((H // 2, W // 2, 2), np.uint8)
        y[...], uv[...] = rs.randint(0, 256, (H, W)), rs.randint(0, 256, (H // 2, W // 2, 2))
        frames.append(caffe.Frame.nv12(y, uv))
    edges = np.array([(i, j) for i in range(14) for j in range(14) if i != j], np.int32)
    rs = np.random.RandomState(5)
    mean, std = rs.randn(182, 2) * 15, rs.uniform(4, 30, (182, 2))
    akw = dict(threshold=0.5, radius=1, max_det=16, max_cost=30.0, seed_threshold=0.6, max_people=32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.1f" % x for x in v)  # noqa: E731
    say("# video path, synthetic ResNet-152 %dx%d, host NV12 frames in pinned memory, max_det 16 max_people 32, tracker T 64; tracked "
        "people per frame, frames/s by the host clock, median of 5 windows >= 0.5 s, variants alternated" % (H, W))

    if a.overlay:
        overlay(caffe, VideoPipeline, nets, frames, (edges, mean, std), akw, say, fmt, labels=a.labels)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    base_tracker = caffe.Tracker(n_joints=14, slots=1, max_tracks=64)
    found = {}

    def baseline(seconds):
        n, t0 = 0, time.perf_counter()
        while True:
            nets["f32"].forward_images(frames[n % len(frames)], 1.0, want=(), pose=False)
            found["a"] = len(nets["f32"].track_people(base_tracker, scale=1.0, edges=edges, mean=mean, std=std, **akw)[0]["people"])
            n += 1
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return n, dt

    def pipeline(dtype, depth, batch):
        pipe = VideoPipeline(nets[dtype], caffe.Tracker(n_joints=14, slots=1, max_tracks=64), depth=depth, batch=batch,
                             stats=(edges, mean, std), scale=1.0, **akw)

        def run(seconds):
            n, got, t0 = 0, 0, time.perf_counter()
            while time.perf_counter() - t0 < seconds or n % batch:
                pipe.submit(frames[n % len(frames)])
                n += 1
                while pipe._done:
                    pipe.wait_one()
                    got += 1
            got += len(pipe.drain())
            assert got == n
            return n, time.perf_counter() - t0

        return run

    runs = {"(a) forward_images + Net.track_people, f32, one frame per call": baseline}
    for depth in (1, 2, 3, 4):
        runs["(b) VideoPipeline f32 depth %d batch 1" % depth] = pipeline("f32", depth, 1)
    for depth in (1, 2):
        for batch in (1, 4, 8):
            runs["(c) VideoPipeline f16 depth %d batch %d" % (depth, batch)] = pipeline("f16", depth, batch)
    for run in runs.values():  # warm-up: every shape lowered, tuned, its streams chosen
        run(0.2)
    per = windows(runs)
    base = statistics.median(per[list(runs)[0]])
    for k, v in per.items():
        m = statistics.median(v)
        say("%s: %.1f frames/s (%.2fx of (a)); windows %s" % (k, m, m / base, fmt(v)))
    say("# (a) found %d people in its last frame" % found.get("a", -1))

    # (d) the slot map alone: 8 frames of 32 people into one slot
    def world(k):
        r = np.random.RandomState(1)
        out = np.zeros((32, 14, 3), np.float64)
        for q in range(32):
            out[q, :, :2] = (400.0 * (q % 6), 400.0 * (q // 6)) + r.uniform(-40, 40, (14, 2))
            out[q, :, 2] = 0.5
        out[:, :, :2] += 2.0 * k
        return out

    eight = np.stack([world(k % 2) for k in range(8)])
    one_call, eight_calls = caffe.Tracker(n_joints=14, slots=1, max_tracks=64), caffe.Tracker(n_joints=14, slots=1, max_tracks=64)

    def mapped(seconds):
        n, t0 = 0, time.perf_counter()
        while True:
            one_call.update(eight, slot_of=[0] * 8)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return n, dt

    def singly(seconds):
        n, t0 = 0, time.perf_counter()
        while True:
            for b in range(8):
                eight_calls.update(eight[b:b + 1])
            n += 1
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return n, dt

    mapped(0.1), singly(0.1)
    a_ids, b_ids = one_call.update(eight, slot_of=[0] * 8)[0], np.concatenate([eight_calls.update(eight[b:b + 1])[0] for b in range(8)])
    assert (a_ids >= 0).all() and (b_ids >= 0).all()  # every person tracked on both sides
    per = windows({"one": mapped, "eight": singly})
    ms = {k: [1e3 / x for x in v] for k, v in per.items()}
    fmt4 = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    say("(d) Tracker.update, 8 frames of P = n = 32 into one slot, T 64: one call with a slot map %.4f ms, eight calls %.4f ms per 8 frames; "
        "windows one call %s eight calls %s" % (statistics.median(ms["one"]), statistics.median(ms["eight"]), fmt4(ms["one"]), fmt4(ms["eight"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
