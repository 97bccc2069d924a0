"""GPU: the overlays inside the asynchronous video chain — `Net.track_frames_async(draw=, redact=)` (dc_net_track_frames_async_overlay) and
`VideoPipeline(in_chain=True)` — on the 200 x 264 net, the frames and the parameters of tests/test_gpu_video.py.  The results of a request
(people, cand, ids, place) are those of the same request without overlays, BIT FOR BIT, and its frames are a copy of the clean frames put
through the synchronous `caffe.redact_people` then `caffe.draw_people` with those results, BYTE FOR BYTE.  There is no tolerance anywhere.

PARITY UNPINNED BY THE REFERENCE, which stops at the maps; assembly, tracking, drawing and redaction rules are this project's own."""
import numpy as np
import pytest

from test_gpu_smooth import SKW, _seeded
from test_gpu_video import AKW, CHAIN, EDGES, FRAMES, IMG, MEAN, STD, TKW, J, _net, _nv12_planes
from test_gpu_video import cost_model_tiles  # noqa: F401  (autouse here too: DC_AUTOTUNE=0 for every forward of the module)

pytestmark = pytest.mark.gpu

SKELETON = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7), (7, 8), (8, 12), (12, 9), (9, 10), (10, 11), (12, 13), (2, 8), (3, 9))
ID_COLORS = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48))
DRAW = dict(edges=SKELETON, alpha=160, alpha_filled=60, joint_radius=3.0, limb_radius=1.5, palette=ID_COLORS)
REDACT = dict(region="head_or_body", head=(12, 13), edges=SKELETON, block=8, head_scale=0.75, body_scale=0.06, min_radius=4.0, max_radius=256.0)
KEYS = ("people", "cand", "ids", "place")


def _make(caffe, source, k, keep):
    """Frame k of the sequence -> (what the net takes, read() -> its planes as they are now, clean copies of the planes)."""
    if source == "bgr":
        img = FRAMES[k].copy()
        return img, (lambda: [img]), [FRAMES[k].copy()]
    y, uv = _nv12_planes(0)
    y, uv = np.ascontiguousarray(np.roll(y, 8 * k, axis=1)), np.ascontiguousarray(np.roll(uv, 4 * k, axis=1))
    clean = [y.copy(), uv.copy()]
    if source == "nv12":
        return caffe.Frame.nv12(y, uv), (lambda: [y, uv]), clean
    import torch

    ty, tuv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    torch.cuda.synchronize()
    keep.append((ty, tuv))
    frame = caffe.Frame.nv12_device(ty.data_ptr(), tuv.data_ptr(), y.shape[0], y.shape[1], y.shape[1], uv.shape[1] * 2)
    return frame, (lambda: [ty.cpu().numpy(), tuv.cpu().numpy()]), clean


def _host_route(caffe, clean, d, draw=DRAW, redact=REDACT):
    """Copies of the clean planes through the synchronous entries with a request's results -> (planes, redacted)."""
    planes = [c.copy() for c in clean]
    frame = planes[0] if len(planes) == 1 else caffe.Frame.nv12(*planes)
    red = None
    if redact is not None:
        red = caffe.redact_people(frame, d["people"], ids=d.get("ids"), **redact)
    if draw is not None:
        caffe.draw_people(frame, d["people"], ids=d.get("ids"), cand=d["cand"], **draw)
    return planes, red


def _planes_equal(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def _same(got, want, keys=KEYS):
    return all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in keys if k in want)


def _run_sequence(caffe, net, source, n_frames, tracker_kw=TKW, extra=None, with_tracker=True):
    """n_frames of one sequence, every request collected before the next: once without overlays, once with both, on fresh trackers."""
    extra = extra or {}
    keep, total, changed = [], 0, 0
    plain_t = caffe.Tracker(n_joints=J, **tracker_kw) if with_tracker else None
    chain_t = caffe.Tracker(n_joints=J, **tracker_kw) if with_tracker else None
    for k in range(n_frames):
        frame, read, clean = _make(caffe, source, k, keep)
        plain = net.track_frames_async(frame, plain_t, 1.0, **dict(CHAIN, **extra)).result()[0]
        assert _planes_equal(read(), clean)  # a request without overlays leaves the frame alone
        got = net.track_frames_async(frame, chain_t, 1.0, draw=DRAW, redact=REDACT, **dict(CHAIN, **extra)).result()[0]
        assert set(got) == set(plain) | {"redacted"} and _same(got, plain), k
        want, red = _host_route(caffe, clean, plain)
        now = read()
        for i, (g, w) in enumerate(zip(now, want)):
            assert np.array_equal(g, w), "frame %d plane %d: %d bytes differ" % (k, i, int((g != w).sum()))
        assert got["redacted"].dtype == np.int32 and np.array_equal(got["redacted"], red)
        total += len(plain["people"])
        changed += int(not _planes_equal(now, clean))
    if with_tracker:
        a, b = chain_t.state(), plain_t.state()
        assert all(np.array_equal(a[k], b[k]) for k in a)
    assert total > 0 and changed > 0
    return total


@pytest.mark.parametrize("stages", [dict(), dict(complete=True, dedupe=True)], ids=["plain", "complete-dedupe"])
@pytest.mark.parametrize("source", ["bgr", "nv12", "nv12_device"])
def test_async_entry_with_overlays(gpu_caffe, synth152, source, stages):
    net = _net("f32", gpu_caffe, synth152[0])
    total = _run_sequence(gpu_caffe, net, source, 3, extra=stages)
    print("overlays in the chain (%s, %s): %d people over 3 frames" % (source, sorted(stages), total))


@pytest.mark.parametrize("source", ["bgr", "nv12", "nv12_device"])
def test_async_entry_with_overlays_without_a_tracker(gpu_caffe, synth152, source):
    """No tracker: no ids, the person's index chooses the colour."""
    net = _net("f32", gpu_caffe, synth152[0])
    _run_sequence(gpu_caffe, net, source, 2, with_tracker=False)


def test_async_entry_with_overlays_on_the_sparse_pairwise_net(gpu_caffe, synth152):
    net = _net("sparse", gpu_caffe, synth152[0])
    _run_sequence(gpu_caffe, net, "bgr", 2)


@pytest.mark.parametrize("source", ["bgr", "nv12", "nv12_device"])
def test_smoothed_people_are_drawn_with_bridged_joints_at_alpha_filled(gpu_caffe, synth152, source):
    """Two identically seeded smoothing trackers (tests/test_gpu_smooth.py): the request returns the smoothed poses with one joint bridged,
    and the overlays are made from exactly those — the bridged joint and its limbs at alpha_filled."""
    net = _net("f32", gpu_caffe, synth152[0])
    keep = []
    frame, read, clean = _make(gpu_caffe, source, 0, keep)
    net.forward_images(frame, 1.0, want=(), pose=False)
    assembled = net.assemble_people(scale=1.0, **CHAIN)[0]
    plain_t, q, j = _seeded(gpu_caffe, assembled["people"], SKW)
    chain_t, _, _ = _seeded(gpu_caffe, assembled["people"], SKW)
    plain = net.track_frames_async(frame, plain_t, 1.0, **CHAIN).result()[0]
    got = net.track_frames_async(frame, chain_t, 1.0, draw=DRAW, redact=REDACT, **CHAIN).result()[0]
    assert _same(got, plain, KEYS + ("bridged",)) and got["bridged"][q, j] and got["cand"][q, j] == -3
    want, red = _host_route(gpu_caffe, clean, plain)
    assert _planes_equal(read(), want) and np.array_equal(got["redacted"], red)
    # the bridged joint shows: with alpha_filled = alpha the bytes differ
    other, _ = _host_route(gpu_caffe, clean, plain, draw=dict(DRAW, alpha_filled=DRAW["alpha"]))
    assert not _planes_equal(other, want)
    a, b = chain_t.smooth_state(), plain_t.smooth_state()
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_three_frames_of_one_slot_in_one_request(gpu_caffe, synth152):
    """A batch of 3 packed BGR frames with slot_of = [0, 0, 0]: the stacked images are written in place, image by image."""
    net = _net("f32", gpu_caffe, synth152[0])
    clean = np.stack(FRAMES[:3])
    plain = net.track_frames_async(clean.copy(), gpu_caffe.Tracker(n_joints=J, **TKW), 1.0, slot_of=[0, 0, 0], **CHAIN).result()
    stack = clean.copy()
    got = net.track_frames_async(stack, gpu_caffe.Tracker(n_joints=J, **TKW), 1.0, slot_of=[0, 0, 0], draw=DRAW, redact=REDACT, **CHAIN).result()
    assert len(got) == len(plain) == 3 and sum(len(d["people"]) for d in plain) > 0
    for b in range(3):
        assert _same(got[b], plain[b])
        (want,), red = _host_route(gpu_caffe, [clean[b]], plain[b])
        assert np.array_equal(stack[b], want) and np.array_equal(got[b]["redacted"], red), b
    assert len(set(plain[0]["ids"].tolist()) & set(plain[2]["ids"].tolist())) > 0 and not np.array_equal(stack, clean)
    # only_ids / keep_ids choose by the tracker's ids: the request's own results say whom
    first = int(plain[0]["ids"][0])
    stack = clean.copy()
    got = net.track_frames_async(stack, gpu_caffe.Tracker(n_joints=J, **TKW), 1.0, slot_of=[0, 0, 0], redact=dict(REDACT, only_ids=[first]),
                                 **CHAIN).result()
    for b in range(3):
        (want,), red = _host_route(gpu_caffe, [clean[b]], plain[b], draw=None, redact=dict(REDACT, only_ids=[first]))
        assert np.array_equal(stack[b], want) and np.array_equal(got[b]["redacted"], red) and red.sum() <= 1, b


@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_pipeline_in_chain_equals_the_host_route(gpu_caffe, synth152, source):
    """VideoPipeline(depth=3, batch=2) over 9 frames, in_chain=True against in_chain=False on copies: the same (tag, people, ids), the same
    bytes in every frame, the same tracker state.  The builders read the tracker's shared scratch with three executors in flight."""
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    keep, runs = [], {}
    for in_chain in (False, True):
        made = [_make(gpu_caffe, source, k, keep) for k in range(9)]
        tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
        pipe = VideoPipeline(net, tracker, depth=3, batch=2, stats=(EDGES, MEAN, STD), choose_streams=False, in_chain=in_chain,
                             draw={k: v for k, v in DRAW.items() if k != "edges"}, redact=dict(region="head_or_body", block=8), **AKW)
        for k, (frame, _, _) in enumerate(made):
            pipe.submit(frame, tag=k)
        out = pipe.drain()
        runs[in_chain] = (out, [read() for _, read, _ in made], tracker.state(), [clean for _, _, clean in made])
    (host, host_frames, host_state, clean), (chain, chain_frames, chain_state, _) = runs[False], runs[True]
    assert [t for t, _, _ in host] == [t for t, _, _ in chain] == list(range(9))
    for (_, p0, i0), (_, p1, i1) in zip(host, chain):
        assert np.array_equal(p0, p1) and np.array_equal(i0, i1) and i1.dtype == np.int64
    for k, (a, b) in enumerate(zip(host_frames, chain_frames)):
        assert _planes_equal(a, b), k
    assert all(np.array_equal(host_state[k], chain_state[k]) for k in host_state)
    assert sum(len(p) for _, p, _ in chain) > 0 and sum(int(not _planes_equal(a, c)) for a, c in zip(chain_frames, clean)) >= 5


def test_pose_track_people_in_chain(gpu_caffe, synth152):
    """pose.track_people(in_chain=True) yields what the host route yields and writes the same bytes — at depth 1, batch 1 against the
    synchronous default, and at depth 2, batch 2 (a batch forward has bits of its own) against the host route of the same flight."""
    from pose import track_people

    net = _net("f32", gpu_caffe, synth152[0])
    stats = (EDGES, MEAN, STD)
    style = dict(alpha=160, joint_radius=3.0, limb_radius=1.5, palette=ID_COLORS)
    for flight in (dict(), dict(depth=2, batch=2)):
        runs = []
        for kw in (flight, dict(flight, in_chain=True)):
            frames = [f.copy() for f in FRAMES[:4]]
            out = list(track_people(frames, None, None, stats, tracker=gpu_caffe.Tracker(n_joints=J, **TKW), net=net, redact=dict(region="head"),
                                    draw=style, **dict(AKW, **kw)))
            runs.append((out, frames))
        (host, host_frames), (chain, chain_frames) = runs
        assert len(host) == len(chain) == 4 and sum(len(p) for p, _ in chain) > 0
        for (p0, i0), (p1, i1) in zip(host, chain):
            assert np.array_equal(p0, p1) and np.array_equal(i0, i1), flight
        assert all(np.array_equal(a, b) for a, b in zip(host_frames, chain_frames)), flight
        assert any(not np.array_equal(a, b) for a, b in zip(chain_frames, FRAMES[:4])), flight


def test_in_chain_pipelines_leave_no_device_memory_behind(gpu_caffe, synth152):
    """Create / submit / drain / destroy cycles of an in-chain pipeline, as test_pipelines_and_trackers_leave_no_device_memory_behind runs
    them: the executors' overlay blocks go with the clones, the free device memory stays where it was."""
    import gc

    import torch
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    dev = torch.device("cuda", 0)
    free = []
    for _ in range(4):  # the first cycle is the warm-up, three are measured
        tracker = gpu_caffe.Tracker(n_joints=J, slots=2, max_tracks=256, **TKW)
        pipe = VideoPipeline(net, tracker, depth=3, batch=2, stats=(EDGES, MEAN, STD), choose_streams=False, in_chain=True, draw=True,
                             redact=dict(region="body"), **AKW)
        for k, f in enumerate(FRAMES[:6]):
            pipe.submit(f.copy(), tag=k, slot=k % 2)
        assert len(pipe.drain()) == 6
        del pipe, tracker
        gc.collect()
        torch.cuda.synchronize(dev)
        free.append(torch.cuda.mem_get_info(dev)[0] / 2 ** 20)
    print("free device memory after each in-chain cycle, MiB: %r" % (free,))
    assert free[1] - free[-1] <= 2.0, free
    assert IMG.shape == FRAMES[0].shape
