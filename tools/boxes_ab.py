"""A/B of the box entry against host-cut crops on one box: every leg in a fresh process, the legs alternated `--reps` times.

    python tools/boxes_ab.py [--reps 3] [--steps 10] [--out profiles/boxes_ab.txt]

Workload: configs[4] from one image: a 1080 x 1920 BGR image, 32 person boxes of 336 x 256, 4 pyramid scales (0.5, 0.75, 1.0,
1.25), ResNet-152 float32 (hipGraph), poses decoded on the device, no maps downloaded.
Legs: `boxes` = NetGroup.forward_boxes(image, boxes, scales) (the image crosses PCIe once, one pre-processing launch per member);
`crops` = the flow a caller writes today: cut the 32 crops on the host, stack them, NetGroup.forward_images (each member uploads
the stack and pre-processes it), then shift every pose by its box corner on the host.  Both legs run the same grouped forward on
the same canvases.  Each leg tunes into one shared tune cache (the first child tunes, the later ones read it).  One JSON line per
leg and repetition, then the medians; a child that fails ends the run.  Each child runs under its own `timeout -k 10`."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("boxes", "crops")
PYRAMID = [0.5, 0.75, 1.0, 1.25]


def _boxes():
    return [(8 + 236 * (i % 8), 12 + 240 * (i // 8), 8 + 236 * (i % 8) + 256, 12 + 240 * (i // 8) + 336) for i in range(32)]


def child(leg, steps):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python")]
    import numpy as np

    import caffe
    from deepcut_tools import deepercut_prototxt

    caffe.set_mode_gpu()
    caffe.set_device(0)
    net = caffe.Net(deepercut_prototxt(152, 336, 256), caffe.TEST, from_text=True, hipgraph=1)
    rs = np.random.RandomState(0)
    for name in net.params:  # weights of the net's own magnitude (values do not steer the timing)
        for b in net.params[name]:
            b.data[...] = rs.randn(*b.data.shape).astype(np.float32) * 0.02
    grp = caffe.NetGroup([net] + [net.clone() for _ in PYRAMID[1:]])
    img = rs.randint(0, 256, (1080, 1920, 3)).astype(np.uint8)
    boxes = _boxes()
    corner = np.array([[x0, y0, 0, 0, 0] for x0, y0, _, _ in boxes], np.float64)[:, :, None]

    if leg == "boxes":
        def step():
            return [o["pose"] for o in grp.forward_boxes(img, boxes, PYRAMID, want=(), pose=True)]
    else:
        def step():
            crops = np.stack([img[y0:y1, x0:x1] for x0, y0, x1, y1 in boxes])
            return [o["pose"] + corner for o in grp.forward_images(crops, PYRAMID, want=(), pose=True)]
    for _ in range(3):  # lower, tune, capture
        poses = step()
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        best = min(best, (time.perf_counter() - t0) / steps)
    # (equal canvases, equal forward: the two legs decode the same poses)
    print(json.dumps({"leg": leg, "ms_per_call": best * 1e3, "boxes_per_s": 32 / best,
                      "pose_checksum": float(sum(np.nansum(p[:, :3]) for p in poses))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", metavar="LEG")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child process")
    ap.add_argument("--cache", default="", help="the shared tune cache (default: boxes_ab_tune.txt beside --out, else here)")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps)
    cache = a.cache or os.path.join(os.path.dirname(os.path.abspath(a.out)) if a.out else ".", "boxes_ab_tune.txt")
    rows = []
    for rep in range(a.reps):
        for leg in LEGS:
            env = dict(os.environ, DC_TUNE_CACHE=cache)
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                raise SystemExit("leg %s failed with status %d: stopping" % (leg, p.returncode))
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            r["rep"] = rep
            rows.append(r)
            print(json.dumps(r), flush=True)
    summary = {}
    for leg in LEGS:
        v = sorted(r["ms_per_call"] for r in rows if r["leg"] == leg)
        summary[leg] = {"median_ms_per_call": v[len(v) // 2], "min": v[0], "max": v[-1]}
    summary["boxes_vs_crops"] = summary["boxes"]["median_ms_per_call"] / summary["crops"]["median_ms_per_call"] - 1.0
    print(json.dumps({"summary": summary}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/boxes_ab.py --reps %d --steps %d on one MI355X: each leg a fresh process, legs alternated; ms per call = one\n"
                    "# 1080x1920 image, 32 boxes of 336x256 x 4 scales (0.5-1.25), ResNet-152 float32, poses only (best of 3 x %d calls)\n"
                    % (a.reps, a.steps, a.steps))
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps({"summary": summary}, indent=1) + "\n")


if __name__ == "__main__":
    main()
