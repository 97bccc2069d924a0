"""A/B of the bfloat16 mode against float16 on one box: every leg in a fresh process, the legs alternated `--reps` times.

    python tools/bf16_ab.py [--reps 3] [--steps 20] [--out FILE] [--legs f16,bf16,bf16-forms] [--parent DIR]

Legs: f16 (default forms: wino_h23 / ws1x1 / stem7x7 where the tuner takes them), f16-direct (DC_WINOGRAD=0 DC_STREAM1X1=0 DC_STEM=0:
the gather-GEMM tiles only, what bf16 runs on by default), bf16 (its switches unset: tiles only) and bf16-forms (DC_STREAM1X1_BF16=-1
DC_STEM_BF16=-1: bs1x1 / bs7x7 where the tuner takes them).  --parent DIR adds the leg bf16-parent: the bf16 leg of another built checkout
(its own tools/bf16_ab.py), for a comparison across commits.  Workloads: the batch-8 544x736 forward one at a time (device-resident,
hipGraph) and the 4-scale pyramid (batch 8 x 272x368 .. 680x920) as one NetGroup.  Each leg tunes its tiles in its own process
(a tune cache per leg, under --cache-dir: the first repetition tunes, the later ones read it).  One JSON line per leg and
repetition, then the medians; a child that fails ends the run.  Each child runs under its own `timeout -k 10`."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"f16": ("f16", {}), "f16-direct": ("f16", {"DC_WINOGRAD": "0", "DC_STREAM1X1": "0", "DC_STEM": "0"}), "bf16": ("bf16", {}),
        "bf16-forms": ("bf16", {"DC_STREAM1X1_BF16": "-1", "DC_STEM_BF16": "-1"})}
PARENT_LEG = "bf16-parent"
SHAPES = [(272, 368), (408, 552), (544, 736), (680, 920)]


def child(leg, work, steps):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "deepcut-cnn_amd"), os.path.join(ROOT, "deepcut-cnn_amd", "python")]
    import torch

    import caffe
    from deepcut_tools import deepercut_prototxt

    caffe.set_mode_gpu()
    caffe.set_device(0)
    dt = LEGS[leg][0]
    dev = torch.device("cuda", 0)
    net = caffe.Net(deepercut_prototxt(152, 544, 736, 8), caffe.TEST, from_text=True, hipgraph=1, dtype=dt)
    rs = torch.Generator(device="cpu").manual_seed(0)
    for name in net.params:  # weights of the net's own magnitude (values do not steer the timing)
        for b in net.params[name]:
            b.data[...] = (torch.randn(*b.data.shape, generator=rs) * 0.02).numpy()
    stream = torch.cuda.Stream(dev)
    if work == "b8":
        h, w = 544, 736
        x = torch.randn(8, 3, h, w, generator=rs).mul_(50).to(dev)
        outs = [torch.empty(8, c, h // 8, w // 8, device=dev) for c in (14, 28, 364)]

        def step():
            net.forward_device(x.data_ptr(), 8, h, w, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), stream.cuda_stream)
        images = 8
    else:
        members = [net.clone() for _ in SHAPES]
        for m, s in zip(members, SHAPES):
            m.reserve(8, *s)
        grp = caffe.NetGroup(members)
        xs = [torch.randn(8, 3, h, w, generator=rs).mul_(50).to(dev) for h, w in SHAPES]
        os_ = [[torch.empty(8, c, h // 8, w // 8, device=dev) for c in (14, 28, 364)] for h, w in SHAPES]
        gshapes = [(8, h, w) for h, w in SHAPES]

        def step():
            grp.forward_device([x.data_ptr() for x in xs], gshapes, [o[0].data_ptr() for o in os_], [o[1].data_ptr() for o in os_],
                               [o[2].data_ptr() for o in os_], stream=stream.cuda_stream)
        images = 8  # one step = 8 image pyramids
    for _ in range(3):  # lower, tune, capture
        step()
    torch.cuda.synchronize(dev)
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize(dev)
        best = min(best, (time.perf_counter() - t0) / steps)
    print(json.dumps({"leg": leg, "work": work, "ms_per_step": best * 1e3, "images_per_s": images / best}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", nargs=2, metavar=("LEG", "WORK"))
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child process")
    ap.add_argument("--cache-dir", default="", help="directory of the per-leg tune caches (default: beside --out, else the working directory)")
    ap.add_argument("--legs", default="", help="comma-separated subset of the legs (default: all)")
    ap.add_argument("--parent", default="", help="another built checkout of this repository: adds the leg bf16-parent")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps)
    legs = [leg for leg in a.legs.split(",") if leg] or list(LEGS)
    if any(leg not in LEGS for leg in legs):
        raise SystemExit("legs: " + ", ".join(LEGS))
    if a.parent:
        legs.insert(0, PARENT_LEG)
    rows = []
    for rep in range(a.reps):
        for work in ("b8", "pyramid"):
            for leg in legs:
                for k in ("DC_STREAM1X1_BF16", "DC_STEM_BF16"):  # the legs set their own
                    os.environ.pop(k, None)
                env = dict(os.environ, **(LEGS[leg][1] if leg in LEGS else {}))
                script = os.path.join(os.path.abspath(a.parent), "tools", "bf16_ab.py") if leg == PARENT_LEG else os.path.abspath(__file__)
                cdir = a.cache_dir or (os.path.dirname(os.path.abspath(a.out)) if a.out else ".")
                env["DC_TUNE_CACHE"] = os.path.join(cdir, "bf16_ab_tune_%s.txt" % leg)
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, script, "--child", "bf16" if leg == PARENT_LEG else leg, work, "--steps", str(a.steps)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-3000:])
                    raise SystemExit("leg %s / %s failed with status %d: stopping" % (leg, work, p.returncode))
                r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                r["rep"], r["leg"] = rep, leg
                rows.append(r)
                print(json.dumps(r), flush=True)
    summary = {}
    for work in ("b8", "pyramid"):
        for leg in legs:
            v = sorted(r["images_per_s"] for r in rows if r["leg"] == leg and r["work"] == work)
            summary["%s/%s" % (work, leg)] = {"median_images_per_s": v[len(v) // 2], "min": v[0], "max": v[-1]}
        for x, y in (("bf16", "f16-direct"), ("bf16", "f16"), ("bf16-forms", "bf16"), ("bf16-forms", "f16"), ("bf16", PARENT_LEG)):
            if x in legs and y in legs:
                summary["%s/%s_vs_%s" % (work, x.replace("-", "_"), y.replace("-", "_"))] = summary["%s/%s" % (work, x)]["median_images_per_s"] / summary["%s/%s" % (work, y)]["median_images_per_s"] - 1.0
    print(json.dumps({"summary": summary}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps({"summary": summary}, indent=1) + "\n")


if __name__ == "__main__":
    main()
