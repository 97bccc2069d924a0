#!/usr/bin/env python3
"""What the tracker costs (csrc/track.hip).  In ONE process on a 544x736 float32 net holding one forward, after warm-up, at
max_det 16 and max_people 32, alternating: `Net.track_people` (assembly + the tracker's launch behind it) and `Net.assemble_people` (the
assembly alone, unchanged code).  Then the stand-alone `Tracker.update` — host poses up, one launch, ids back — at T = 64, P = n = 32
and at the entry limits T = P = n = 256, there on people who each stay near their own track (a round of the matching re-derives hardly
any row minimum) and on a planted worst case in which every open track is nearest to the same person in every round (every round
re-derives the row minima of all tracks that are still open), beside `Net.assemble_people` at max_det 64 and max_people 256.  Every figure is a host clock around a synchronous call, ms per call, the median
of five windows of at least 0.5 s with the windows listed.
    python tools/track_ab.py [--out profiles/track_ab.txt]
--assign both measures the matching rules against each other instead (DC_TRACK_OPT_ASSIGN: step 4, greedy, and step 4', the optimal
assignment): the same calls, every one on a greedy and on an optimal tracker, the two alternated in the same windows — `Net.track_people`
and the stand-alone updates above —, with the number of inner trips step 4' takes on each case, counted by its restatement
(tests/assign_ref.py) on the device's own distances.
    python tools/track_ab.py --assign both [--out profiles/track_assign_ab.txt]
--smooth measures step 8 (smoothed poses, `Tracker.smoothing`) the same way: every call on a tracker without smoothing and on one with
it (the placeholder parameters), the two alternated in the same windows — `Net.track_people` on the held forward, the stand-alone update
at 32 people and at T = P = n = 256.  The smoothing-off figures are the ones to hold against this tool's default run on the commit before.
    python tools/track_ab.py --smooth [--out profiles/track_smooth_ab.txt]"""
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


def near(n):
    """n people on a 400-pixel grid, then the same people moved by up to 3 pixels a joint, in another order"""
    r = np.random.RandomState(1)
    out = np.zeros((1, n, 14, 3), np.float64)
    side = int(np.ceil(np.sqrt(n)))
    for q in range(n):
        out[0, q, :, :2] = (400.0 * (q % side), 400.0 * (q // side)) + r.uniform(-40, 40, (14, 2))
        out[0, q, :, 2] = 0.5
    nxt = out.copy()
    nxt[0, :, :, :2] += r.uniform(-3, 3, (n, 14, 2))
    return out, nxt[:, r.permutation(n)]


def contended(n):
    """one rigid pose at x = q, then at x = 1000 + 10 q: every track's nearest open person is the SAME one in every round (the
    leftmost of the second frame, the rightmost of the first on the way back), so every round re-derives the rows of all open tracks"""
    r = np.random.RandomState(2)
    body = r.uniform(-40, 40, (14, 2))
    a, b = np.zeros((1, n, 14, 3), np.float64), np.zeros((1, n, 14, 3), np.float64)
    for q in range(n):
        a[0, q, :, :2], b[0, q, :, :2] = body + (q, 0), body + (1000 + 10 * q, 0)
    a[..., 2] = b[..., 2] = 0.5
    return a, b


CASES = [("T 64, P = n = 32, everybody near their own track", 64, 32, near, 0.25),
         ("T = P = n = 256, everybody near their own track", 256, 256, near, 0.25),
         ("T = P = n = 256, motion 0, every open track nearest to the same person in every round", 256, 256, contended, 1e9)]


def assign_ab(caffe, net, kw, say, fmt):
    """Greedy against optimal, alternated in the same windows: Net.track_people on the held forward, then every stand-alone case."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import assign_ref

    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    rules = ("greedy", "optimal")
    trackers = {r: caffe.Tracker(n_joints=14, slots=1, max_tracks=64, assign=r) for r in rules}
    calls = {"track_people " + r: (lambda t=trackers[r]: net.track_people(t, **kw)) for r in rules}
    calls["assemble_people"] = lambda: net.assemble_people(**kw)
    for call in calls.values():
        for _ in range(20):
            call()
    found = len(net.assemble_people(**kw)[0]["people"])
    per = windows(calls)
    s = statistics.median(per["assemble_people"])
    say("max_det 16 max_people 32 (%d people found), T 64: Net.assemble_people %s ms per call" % (found, spread(per["assemble_people"])))
    # what step 4' had to do there: the assembled people fed to a stand-alone optimal tracker as often as the chained one saw them (the
    # chained entry is Tracker.update bit for bit), the last update's distances handed to the restatement
    people = net.assemble_people(**kw)[0]["people"]
    again = caffe.Tracker(n_joints=14, slots=1, max_tracks=64, assign="optimal")
    for _ in range(40):
        again.update([people])
    live = again.state()["ids"] >= 0
    _, _, dist = again.update([people], return_dist=True)
    count = {}
    assign_ref.assign(dist[0], live.tolist(), len(people), 0.25, count)  # 0.25: caffe.Tracker's default max_dist
    say("  the same frame again and again: %d live tracks against %d people, %d inner trips of step 4' per update" % (int(live.sum()), len(people), count["trips"]))
    for r in rules:
        v = per["track_people " + r]
        say("  Net.track_people, %s: %s ms per call (%+.4f ms on assemble_people); windows %s" % (r, spread(v), statistics.median(v) - s, fmt(v)))
    for name, T, n, make, max_dist in CASES:
        first, second = make(n)
        calls, trips = {}, None
        for r in rules:
            trk = caffe.Tracker(n_joints=14, slots=1, max_tracks=T, max_dist=max_dist, max_misses=1000, motion=0 if make is contended else 1, assign=r)
            ids0, _ = trk.update(first)
            live = trk.state()["ids"] >= 0
            ids1, _, dist = trk.update(second, return_dist=True)
            assert sorted(ids0[0].tolist()) == list(range(n)) and sorted(ids1[0].tolist()) == list(range(n)), (name, r)  # all born, all matched
            if r == "optimal":
                count = {}
                assign_ref.assign(dist[0], live.tolist(), n, max_dist, count)
                trips = count["trips"]
            state = {"k": 1}

            def call(trk=trk, frames=(first, second), state=state):
                state["k"] ^= 1
                trk.update(frames[state["k"]])

            for _ in range(4):
                call()
            calls[r] = call
        per = windows(calls)
        g, o = statistics.median(per["greedy"]), statistics.median(per["optimal"])
        say("Tracker.update %s: greedy %s ms, optimal %s ms per call (%+.4f ms, x %.2f), %d inner trips of step 4'; windows greedy %s optimal %s"
            % (name, spread(per["greedy"]), spread(per["optimal"]), o - g, o / g, trips, fmt(per["greedy"]), fmt(per["optimal"])))


def smooth_ab(caffe, net, kw, say, fmt):
    """Smoothing off against on, alternated in the same windows: Net.track_people on the held forward, then the stand-alone updates."""
    spread = lambda v: "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))  # noqa: E731
    modes = {"off": None, "on": True}
    trackers = {m: caffe.Tracker(n_joints=14, slots=1, max_tracks=64, smooth=v) for m, v in modes.items()}
    calls = {"track_people " + m: (lambda t=trackers[m]: net.track_people(t, **kw)) for m in modes}
    calls["assemble_people"] = lambda: net.assemble_people(**kw)
    for call in calls.values():
        for _ in range(20):
            call()
    found = len(net.assemble_people(**kw)[0]["people"])
    per = windows(calls)
    s = statistics.median(per["assemble_people"])
    say("max_det 16 max_people 32 (%d people found), T 64: Net.assemble_people %s ms per call" % (found, spread(per["assemble_people"])))
    for m in modes:
        v = per["track_people " + m]
        say("  Net.track_people, smoothing %s: %s ms per call (%+.4f ms on assemble_people); windows %s" % (m, spread(v), statistics.median(v) - s, fmt(v)))
    for name, T, n, make, max_dist in CASES[:2]:
        first, second = make(n)
        calls = {}
        for m, v in modes.items():
            trk = caffe.Tracker(n_joints=14, slots=1, max_tracks=T, max_dist=max_dist, max_misses=1000, smooth=v)
            ids0, _ = trk.update(first)
            ids1, _ = trk.update(second)
            assert sorted(ids0[0].tolist()) == list(range(n)) and sorted(ids1[0].tolist()) == list(range(n)), (name, m)  # all born, all matched
            state = {"k": 1}

            def call(trk=trk, frames=(first, second), state=state, smoothed=v is not None):
                state["k"] ^= 1
                trk.update(frames[state["k"]], return_smooth=smoothed)  # on: the smoothed poses and src come back as well

            for _ in range(10):
                call()
            calls[m] = call
        per = windows(calls)
        off, on = statistics.median(per["off"]), statistics.median(per["on"])
        say("Tracker.update %s: smoothing off %s ms, on %s ms per call (%+.4f ms, x %.2f); windows off %s on %s"
            % (name, spread(per["off"]), spread(per["on"]), on - off, on / off, fmt(per["off"]), fmt(per["on"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--smooth", action="store_true", help="smoothing off against on (step 8), alternated")
    ap.add_argument("--assign", default="greedy", choices=["greedy", "both"], help="both: greedy against optimal, alternated")
    a = ap.parse_args()
    import caffe
    from deepcut_tools import deepercut_prototxt, synth_weights, write_caffemodel

    caffe.set_mode_gpu()
    caffe.set_device(0)
    path = os.path.join(tempfile.mkdtemp(), "synth152.caffemodel")
    write_caffemodel(path, "ResNet-152", synth_weights(152, seed=0))
    net = caffe.Net(deepercut_prototxt(152, H, W, 1), path, caffe.TEST, from_text=True)
    img = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    edges = np.array([(i, j) for i in range(14) for j in range(14) if i != j], np.int32)
    rs = np.random.RandomState(5)
    mean, std = rs.randn(182, 2) * 15, rs.uniform(4, 30, (182, 2))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: " ".join("%.4f" % x for x in v)  # noqa: E731
    say("# tracker, synthetic ResNet-152 %dx%d float32 batch 1, one forward held; ms per synchronous call by the host clock, median of 5 "
        "windows >= 0.5 s, calls alternated" % (H, W))
    net.forward_images(img, 1.0, want=(), pose=False)
    kw = dict(scale=1.0, threshold=0.5, radius=1, max_det=16, edges=edges, mean=mean, std=std, max_cost=30.0, seed_threshold=0.6, max_people=32)
    if a.smooth or a.assign == "both":
        (smooth_ab if a.smooth else assign_ab)(caffe, net, kw, say, fmt)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    tracker = caffe.Tracker(n_joints=14, slots=1, max_tracks=64)
    calls = {"track_people": lambda: net.track_people(tracker, **kw), "assemble_people": lambda: net.assemble_people(**kw)}
    for call in calls.values():
        for _ in range(20):
            call()
    found = len(net.assemble_people(**kw)[0]["people"])
    per = windows(calls)
    t, s = statistics.median(per["track_people"]), statistics.median(per["assemble_people"])
    say("max_det 16 max_people 32 (%d people found), T 64: Net.track_people %.4f ms, Net.assemble_people %.4f ms per call (%+.4f ms, %+.1f %%); "
        "windows track_people %s assemble_people %s" % (found, t, s, t - s, (t / s - 1) * 100, fmt(per["track_people"]), fmt(per["assemble_people"])))
    kw256 = dict(kw, max_det=64, max_people=256, threshold=0.2, seed_threshold=0.2)
    wide = lambda: net.assemble_people(**kw256)  # noqa: E731
    for _ in range(10):
        wide()
    found256 = len(wide()[0]["people"])

    standalone = {"assemble_people max_det 64 max_people 256 (%d found)" % found256: wide}
    for name, T, n, make, max_dist in CASES:
        trk = caffe.Tracker(n_joints=14, slots=1, max_tracks=T, max_dist=max_dist, max_misses=1000, motion=0 if make is contended else 1)
        first, second = make(n)
        ids0, _ = trk.update(first)
        ids1, _ = trk.update(second)
        assert sorted(ids0[0].tolist()) == list(range(n)) and sorted(ids1[0].tolist()) == list(range(n)), name  # all born, then all matched
        # alternating the two frames keeps every update a full matching of n people against n live tracks
        state = {"k": 0}

        def call(trk=trk, frames=(first, second), state=state):
            state["k"] ^= 1
            trk.update(frames[state["k"]])

        for _ in range(10):
            call()
        standalone["Tracker.update " + name] = call
    per = windows(standalone)
    for k, v in per.items():
        say("%s: %.4f ms per call; windows %s" % (k, statistics.median(v), fmt(v)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
