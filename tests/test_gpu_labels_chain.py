"""GPU: the labels inside the asynchronous video chain — `Net.track_frames_async(draw=, redact=, labels=)`
(dc_net_track_frames_async_styles) and `VideoPipeline(labels=, in_chain=True)` — on the net, the frames and the parameters of
tests/test_gpu_video.py and the helpers of tests/test_gpu_overlay_chain.py.  The results of a request are those of the same request
without `labels`, BIT FOR BIT, and its frames are a copy of the clean frames put through the synchronous `caffe.redact_people`,
`caffe.draw_people` and `caffe.label_people`, in that order, with those results, BYTE FOR BYTE.  There is no tolerance anywhere.

PARITY UNPINNED BY THE REFERENCE, which stops at the maps; assembly, tracking, drawing, redaction and label rules are this project's own."""
import numpy as np
import pytest

from test_gpu_overlay_chain import DRAW, ID_COLORS, KEYS, REDACT, _host_route, _make, _planes_equal, _same
from test_gpu_smooth import SKW, _seeded
from test_gpu_video import AKW, CHAIN, EDGES, FRAMES, MEAN, STD, TKW, J, _net
from test_gpu_video import cost_model_tiles  # noqa: F401  (autouse here too: DC_AUTOTUNE=0 for every forward of the module)

pytestmark = pytest.mark.gpu

LABELS = dict(scale=2, gap=1, anchor=13, prefix="ID", alpha_text=240, alpha_plate=150, palette=ID_COLORS)


def _three(caffe, clean, d, labels=LABELS, draw=DRAW, redact=REDACT):
    """Copies of the clean planes through the three synchronous entries with a request's results -> (planes, redacted)."""
    planes, red = _host_route(caffe, clean, d, draw=draw, redact=redact)
    frame = planes[0] if len(planes) == 1 else caffe.Frame.nv12(*planes)
    caffe.label_people(frame, d["people"], ids=d.get("ids"), **labels)
    return planes, red


@pytest.mark.parametrize("with_tracker", [True, False], ids=["tracker", "no-tracker"])
@pytest.mark.parametrize("source", ["bgr", "nv12", "nv12_device"])
def test_async_entry_with_labels(gpu_caffe, synth152, source, with_tracker):
    net = _net("f32", gpu_caffe, synth152[0])
    keep, total, labelled = [], 0, 0
    trackers = [gpu_caffe.Tracker(n_joints=J, **TKW) if with_tracker else None for _ in range(3)]
    for k in range(2):
        frame, read, clean = _make(gpu_caffe, source, k, keep)
        plain = net.track_frames_async(frame, trackers[0], 1.0, draw=DRAW, redact=REDACT, **CHAIN).result()[0]
        without, red0 = _host_route(gpu_caffe, clean, plain)
        assert _planes_equal(read(), without)  # without labels: the bytes of the older route
        frame, read, clean = _make(gpu_caffe, source, k, keep)
        got = net.track_frames_async(frame, trackers[1], 1.0, draw=DRAW, redact=REDACT, labels=LABELS, **CHAIN).result()[0]
        assert set(got) == set(plain) and _same(got, plain, KEYS + ("redacted",)), k
        want, red = _three(gpu_caffe, clean, plain)
        for i, (g, w) in enumerate(zip(read(), want)):
            assert np.array_equal(g, w), "frame %d plane %d: %d bytes differ" % (k, i, int((g != w).sum()))
        assert np.array_equal(got["redacted"], red) and np.array_equal(red, red0)
        labelled += int(not _planes_equal(want, without))
        # labels alone
        frame, read, clean = _make(gpu_caffe, source, k, keep)
        only = net.track_frames_async(frame, trackers[2], 1.0, labels=dict(LABELS, anchor=None, color="text"), **CHAIN).result()[0]
        assert _same(only, plain) and "redacted" not in only
        want, _ = _three(gpu_caffe, clean, plain, labels=dict(LABELS, anchor=None, color="text"), draw=None, redact=None)
        assert _planes_equal(read(), want), k
        total += len(plain["people"])
    if with_tracker:
        a, b = trackers[1].state(), trackers[0].state()
        assert all(np.array_equal(a[k], b[k]) for k in a)
    assert total > 0 and labelled > 0


def test_smoothed_people_are_labelled_where_the_request_returns_them(gpu_caffe, synth152):
    net = _net("f32", gpu_caffe, synth152[0])
    keep = []
    frame, read, clean = _make(gpu_caffe, "nv12", 0, keep)
    net.forward_images(frame, 1.0, want=(), pose=False)
    assembled = net.assemble_people(scale=1.0, **CHAIN)[0]
    plain_t, q, j = _seeded(gpu_caffe, assembled["people"], SKW)
    chain_t, _, _ = _seeded(gpu_caffe, assembled["people"], SKW)
    plain = net.track_frames_async(frame, plain_t, 1.0, **CHAIN).result()[0]
    got = net.track_frames_async(frame, chain_t, 1.0, draw=DRAW, redact=REDACT, labels=LABELS, **CHAIN).result()[0]
    assert _same(got, plain, KEYS + ("bridged",)) and got["bridged"][q, j]
    want, red = _three(gpu_caffe, clean, plain)
    assert _planes_equal(read(), want) and np.array_equal(got["redacted"], red)
    a, b = chain_t.smooth_state(), plain_t.smooth_state()
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_pipeline_in_chain_equals_the_host_route(gpu_caffe, synth152, source):
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    with pytest.raises(ValueError, match="texts"):
        VideoPipeline(net, None, depth=1, stats=(EDGES, MEAN, STD), in_chain=True, labels=dict(texts=[["a"]]), **AKW)
    with pytest.raises(ValueError, match="stream"):
        VideoPipeline(net, None, depth=1, stats=(EDGES, MEAN, STD), in_chain=True, labels=dict(stream=0), **AKW)
    keep, runs = [], {}
    for in_chain in (False, True):
        made = [_make(gpu_caffe, source, k, keep) for k in range(5)]
        tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
        pipe = VideoPipeline(net, tracker, depth=2, batch=1, stats=(EDGES, MEAN, STD), choose_streams=False, in_chain=in_chain,
                             draw={k: v for k, v in DRAW.items() if k != "edges"}, redact=dict(region="head_or_body", block=8),
                             labels=dict(LABELS, scale=1), **AKW)
        for k, (frame, _, _) in enumerate(made):
            pipe.submit(frame, tag=k)
        out = pipe.drain()
        runs[in_chain] = (out, [read() for _, read, _ in made], tracker.state(), [clean for _, _, clean in made])
    (host, host_frames, host_state, clean), (chain, chain_frames, chain_state, _) = runs[False], runs[True]
    assert [t for t, _, _ in host] == [t for t, _, _ in chain] == list(range(5))
    for (_, p0, i0), (_, p1, i1) in zip(host, chain):
        assert np.array_equal(p0, p1) and np.array_equal(i0, i1)
    for k, (a, b) in enumerate(zip(host_frames, chain_frames)):
        assert _planes_equal(a, b), k
    assert all(np.array_equal(host_state[k], chain_state[k]) for k in host_state)
    assert sum(len(p) for _, p, _ in chain) > 0 and sum(int(not _planes_equal(a, c)) for a, c in zip(chain_frames, clean)) >= 3


def test_labelled_pipelines_leave_no_device_memory_behind(gpu_caffe, synth152):
    import gc

    import torch
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    dev = torch.device("cuda", 0)
    free = []
    for _ in range(4):  # the first cycle is the warm-up, three are measured
        tracker = gpu_caffe.Tracker(n_joints=J, slots=2, max_tracks=256, **TKW)
        pipe = VideoPipeline(net, tracker, depth=3, batch=2, stats=(EDGES, MEAN, STD), choose_streams=False, in_chain=True, draw=True,
                             redact=dict(region="body"), labels=True, **AKW)
        for k, f in enumerate(FRAMES[:6]):
            pipe.submit(f.copy(), tag=k, slot=k % 2)
        assert len(pipe.drain()) == 6
        del pipe, tracker
        gc.collect()
        torch.cuda.synchronize(dev)
        free.append(torch.cuda.mem_get_info(dev)[0] / 2 ** 20)
    print("free device memory after each labelled in-chain cycle, MiB: %r" % (free,))
    assert free[1] - free[-1] <= 2.0, free
