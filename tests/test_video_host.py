"""CPU: the host side of the video path — the slot map of dc_tracker_update_slots / dc_net_track_people_slots /
dc_group_track_people_slots and the asynchronous dc_net_track_frames_async: every new symbol is exported, the new refusals fire before
any device work (so they fire without a device) and name the parameter, the refusals of the synchronous entries arrive in the same
order through the asynchronous one; and the bookkeeping of deepcut_tools.VideoPipeline on a fake net object.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker; what is pinned here is this project's own
interface (include/deepcut_hip.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import people_ref as R

EINVAL, ESHAPE, ENOCPU = -1, -3, -6  # include/deepcut_hip.h
NEW = ["dc_tracker_update_slots", "dc_net_track_people_slots", "dc_group_track_people_slots", "dc_net_track_frames_async"]
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "deepcut_hip.h")


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_new_symbols_are_declared_and_exported():
    import caffe.pycaffe as pc

    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert getattr(pc._lib, name) is not None, name
    import caffe
    import deepcut_tools

    assert hasattr(caffe.Net, "track_frames_async") and hasattr(deepcut_tools, "VideoPipeline")


@pytest.fixture(scope="module")
def cpu():
    """CPU mode for the module: a batch-2 net, a group of it, trackers of two slots."""
    import caffe
    import caffe.pycaffe as pc
    from deepcut_tools import deepercut_prototxt

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    net = caffe.Net(deepercut_prototxt(152, 64, 64, 2), caffe.TEST, from_text=True)
    grp = caffe.NetGroup([net, net.clone()])
    yield dict(caffe=caffe, pc=pc, lib=pc._lib, net=net, grp=grp, two=caffe.Tracker(n_joints=14, slots=2),
               other_j=caffe.Tracker(n_joints=13, slots=2))
    pc._lib.dc_set_mode(mode)


def _err(lib):
    return (lib.dc_last_error() or b"").decode()


def test_tracker_update_slots_refusals(cpu):
    caffe, lib, t = cpu["caffe"], cpu["lib"], cpu["two"]
    people, ids = np.zeros((65, 4, 14, 3)), np.zeros((65, 4), np.int64)

    def update(nb, slot_of, n=None):
        m = np.ascontiguousarray(slot_of, np.int32)
        n = np.ones(max(nb, 1), np.int32) if n is None else np.ascontiguousarray(n, np.int32)
        return lib.dc_tracker_update_slots(t._h, nb, 4, _vp(m), _vp(n), _vp(people), _vp(ids), None, None), _err(lib)

    for bad, b in (([0, 2, 1], 1), ([-1, 0, 0], 0), ([1, 1, 64], 2)):  # a slot outside [0, S)
        rc, msg = update(3, bad)
        assert rc == EINVAL and "slot_of[%d]" % b in msg and "slots = 2" in msg, msg
    for nb in (0, 65, -3):  # nb outside [1, 64] with a map
        rc, msg = update(nb, [0] * 65)
        assert rc == EINVAL and "nb" in msg and "[1, 64]" in msg, msg
    rc, msg = update(3, [0, 0, 1], [1, 5, 1])  # the refusals of dc_tracker_update behind them
    assert rc == EINVAL and "n_people[1]" in msg
    # more images than slots is what the map is for: good arguments reach the mode check, with 64 images too
    for nb, m in ((3, [1, 1, 0]), (64, [1] * 64)):
        rc, msg = update(nb, m)
        assert rc == ENOCPU and "CPU mode" in msg, msg
    # NULL map: dc_tracker_update's rule, nb <= slots
    n3 = np.ones(3, np.int32)
    assert lib.dc_tracker_update_slots(t._h, 3, 4, None, _vp(n3), _vp(people), _vp(ids), None, None) == EINVAL and "slots" in _err(lib)
    assert lib.dc_tracker_update_slots(t._h, 2, 4, None, _vp(n3), _vp(people), _vp(ids), None, None) == ENOCPU
    # through Python
    with pytest.raises(caffe.DeepcutError) as ei:
        t.update(people[:3], slot_of=[0, 1, 2])
    assert ei.value.code == EINVAL and "slot_of[2]" in str(ei.value)
    with pytest.raises(caffe.DeepcutError) as ei:
        t.update(people, slot_of=[0] * 65)
    assert ei.value.code == EINVAL and "nb" in str(ei.value)
    with pytest.raises(ValueError):
        t.update(people[:3], slot_of=[0, 1])  # one slot per image
    with pytest.raises(caffe.DeepcutError) as ei:
        t.update(people[:3], slot_of=[0, 0, 1])
    assert ei.value.code == ENOCPU
    assert t.state(0)["ids"].tolist() == [-1] * 64  # nothing happened


def test_chained_slots_entries_refuse_before_any_device_work(cpu):
    caffe, net, grp, two, other_j = cpu["caffe"], cpu["net"], cpu["grp"], cpu["two"], cpu["other_j"]
    kw = dict(edges=R.all_pairs_edges(), max_cost=20.0, seed_threshold=0.5)
    calls = {"net": lambda t, **k: net.track_people(t, **dict(kw, **k)), "group": lambda t, **k: grp.track_people(t, [1.0, 0.5], 0, **dict(kw, **k))}
    for who, call in calls.items():
        with pytest.raises(caffe.DeepcutError) as ei:
            call(two, slot_of=[0, 2])
        assert ei.value.code == EINVAL and "slot_of[1]" in str(ei.value), who
        with pytest.raises(caffe.DeepcutError) as ei:
            call(other_j, slot_of=[0, 0])
        assert ei.value.code == ESHAPE and "13 joints" in str(ei.value), who
        with pytest.raises(ValueError):
            call(two, slot_of=[0])  # one slot per image of the batch
        with pytest.raises(ValueError):
            call(two, slot_of=[0, 0], max_people=257)  # the assembly's own checks first
        with pytest.raises(caffe.DeepcutError) as ei:
            call(two, slot_of=[1, 1])  # both images into one slot: good, and there is no CPU path
        assert ei.value.code == ENOCPU, who
        one = caffe.Tracker(n_joints=14, slots=1)
        with pytest.raises(caffe.DeepcutError) as ei:
            call(one, slot_of=[0, 0])  # two images, ONE slot: the map allows it
        assert ei.value.code == ENOCPU, who
        with pytest.raises(caffe.DeepcutError) as ei:
            call(one)
        assert ei.value.code == EINVAL and "slots" in str(ei.value), who


def _async_args(pc, n, max_people=8):
    e = np.ascontiguousarray(R.all_pairs_edges())
    q = pc.AssembleParams(1.0, 0.5, 1, 8, 20.0, 0.5, max_people, 1)
    count, people = np.zeros(n, np.int32), np.zeros((n, max(max_people, 1), 14, 3))
    ids = np.zeros((n, max(max_people, 1)), np.int64)
    return e, q, count, people, ids


def test_async_entry_refusals_arrive_in_the_synchronous_order(cpu):
    """dc_net_track_frames_async without a device: the frame entry's refusals first, then the assembly's, then the tracker's and the new
    ones; good arguments reach the mode check (DC_ENOCPU)."""
    caffe, pc, lib, net, two, other_j = cpu["caffe"], cpu["pc"], cpu["lib"], cpu["net"], cpu["two"], cpu["other_j"]
    H, W = 37, 53
    y = np.random.RandomState(1).randint(0, 256, (H, W)).astype(np.uint8)
    uv = np.random.RandomState(2).randint(0, 256, (19, 27, 2)).astype(np.uint8)
    img = np.zeros((2, H, W, 3), np.uint8)
    frame = caffe.Frame.nv12(y, uv)

    def call(tracker=two, frames="good", images=None, n=2, h=H, w=W, scale=1.0, slot_of=None, max_people=8, ids="own", edges="own", bad_frame=None):
        e, q, count, people, own_ids = _async_args(pc, max(n, 1), max_people)
        arr = None
        if frames == "good":
            arr = (pc.DcFrame * 2)(frame.c_frame(), frame.c_frame())
            if bad_frame:
                bad_frame(arr)
        m = None if slot_of is None else np.ascontiguousarray(slot_of, np.int32)
        rc = lib.dc_net_track_frames_async(net._h, None if tracker is None else tracker._h, arr, _vp(images), n, h, w, scale, 0, _vp(m),
                                           C.byref(q), 182, _vp(e) if edges == "own" else edges, None, None, None, _vp(count), _vp(people),
                                           None, _vp(own_ids) if ids == "own" else ids, None)
        return rc, _err(lib)

    def no_plane(arr):
        arr[1].plane[1] = None

    # the new refusals, each naming the parameter
    rc, msg = call(slot_of=[0, 2])
    assert rc == EINVAL and "slot_of[1]" in msg, msg
    rc, msg = call(slot_of=[0, -1])
    assert rc == EINVAL and "slot_of[1]" in msg, msg
    rc, msg = call(tracker=None, ids="own")
    assert rc == EINVAL and "ids" in msg and "tracker" in msg, msg
    # nb = 0 and nb = 65 with a map: nb is the frame count, which the frame entry refuses at 0; 65 frames reach the tracker's check
    rc, msg = call(n=0, slot_of=[0, 0])
    assert rc == EINVAL and "n, height and width" in msg, msg
    e65 = (pc.DcFrame * 65)(*[frame.c_frame()] * 65)
    e, q, count, people, ids = _async_args(pc, 65)
    m = np.zeros(65, np.int32)
    rc = lib.dc_net_track_frames_async(net._h, two._h, e65, None, 65, H, W, 1.0, 0, _vp(m), C.byref(q), 182, _vp(e), None, None, None,
                                       _vp(count), _vp(people), None, _vp(ids), None)
    assert rc == EINVAL and "nb" in _err(lib) and "[1, 64]" in _err(lib), _err(lib)
    # the order of the synchronous entries: the frame entry's refusals ...
    assert call(frames=None, images=None)[0] == EINVAL
    rc, msg = call(scale=0.0, slot_of=[0, 2], max_people=257)
    assert rc == EINVAL and "scale" in msg, msg
    rc, msg = call(bad_frame=no_plane, slot_of=[0, 2], max_people=257)
    assert rc == EINVAL and "frame 1" in msg and "plane[1]" in msg, msg
    # ... then the assembly's ...
    rc, msg = call(slot_of=[0, 2], max_people=257)
    assert rc == EINVAL and "max_people" in msg, msg
    rc, msg = call(slot_of=[0, 2], edges=None)
    assert rc == EINVAL and "edges" in msg, msg
    # ... then the tracker's
    rc, msg = call(tracker=other_j, slot_of=[0, 0])
    assert rc == ESHAPE and "13 joints" in msg, msg
    one = caffe.Tracker(n_joints=14, slots=1)
    rc, msg = call(tracker=one)  # NULL map: nb <= slots
    assert rc == EINVAL and "slots" in msg, msg
    # good arguments, every form of the input: there is no CPU path
    for kw in (dict(), dict(slot_of=[1, 1]), dict(tracker=one, slot_of=[0, 0]), dict(tracker=None, ids=None), dict(ids=None),
               dict(frames=None, images=img)):
        rc, msg = call(**kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, msg)
    # through Python
    kw = dict(edges=R.all_pairs_edges(), max_cost=20.0, seed_threshold=0.5)
    with pytest.raises(caffe.DeepcutError) as ei:
        net.track_frames_async([frame, frame], two, slot_of=[0, 2], **kw)
    assert ei.value.code == EINVAL and "slot_of[1]" in str(ei.value)
    with pytest.raises(caffe.DeepcutError) as ei:
        net.track_frames_async(img, two, **kw)
    assert ei.value.code == ENOCPU
    with pytest.raises(TypeError):
        net.track_frames_async(img, "not a tracker", **kw)
    with pytest.raises(ValueError):
        net.track_frames_async(img, two)  # no edges


# ---- VideoPipeline's bookkeeping on a fake net: no device ---------------------------------------------------------------------------
class FakeHandle(object):
    def __init__(self, net, serial, frames, slot_of):
        self.net, self.serial, self.frames, self.slot_of = net, serial, frames, slot_of

    def done(self):
        return self.serial in self.net.world["finished"]

    def result(self):
        w = self.net.world
        if self.serial not in w["finished"]:
            w["waits"].append(self.serial)
            w["finished"].add(self.serial)
        return [{"people": np.full((1, 1, 3), f[0, 0, 0], np.float64), "ids": np.array([self.serial], np.int64)} for f in self.frames]


class FakeNet(object):
    """What VideoPipeline asks of a net: clone() and track_frames_async() -> a handle with done() / result().  A request finishes when
    the test says so (world["finished"]) or when somebody waits for it (world["waits"] records that)."""

    def __init__(self, world=None, name=0):
        self.world = world if world is not None else dict(finished=set(), waits=[], calls=[], clones=0)
        self.name = name

    def clone(self):
        self.world["clones"] += 1
        return FakeNet(self.world, self.world["clones"])

    def track_frames_async(self, frames, tracker, scale, slot_of=None, **kw):
        frames = frames[None] if getattr(frames, "ndim", 0) == 3 else frames
        serial = len(self.world["calls"])
        self.world["calls"].append(dict(net=self.name, n=len(frames), slot_of=slot_of, scale=scale, kw=kw, tracker=tracker))
        return FakeHandle(self, serial, frames, slot_of)


def _frame(v, h=4, w=6):
    return np.full((h, w, 3), v, np.uint8)


STATS = ("edges", "mean", "std")


def test_pipeline_refuses_depth_outside_1_to_4():
    from deepcut_tools import VideoPipeline

    for depth in (0, 5, -1):
        net = FakeNet()
        with pytest.raises(ValueError) as ei:
            VideoPipeline(net, "tracker", depth=depth, stats=STATS)
        assert "depth" in str(ei.value) and net.world["clones"] == 0
    for batch in (0, 65):
        with pytest.raises(ValueError) as ei:
            VideoPipeline(FakeNet(), "tracker", depth=2, batch=batch, stats=STATS)
        assert "batch" in str(ei.value)
    for depth in (1, 4):
        net = FakeNet()
        assert VideoPipeline(net, "tracker", depth=depth, stats=STATS, choose_streams=False).depth == depth and net.world["clones"] == depth - 1


def test_pipeline_results_in_submission_order_when_executors_finish_out_of_order():
    from deepcut_tools import VideoPipeline

    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=3, stats=STATS, scale=0.5, choose_streams=False, max_det=7)
    for k in range(3):
        pipe.submit(_frame(k), tag="t%d" % k, slot=k % 2)
    w = net.world
    assert [c["net"] for c in w["calls"]] == [0, 1, 2] and not w["waits"]  # three executors, nobody waited
    assert [c["slot_of"] for c in w["calls"]] == [[0], [1], [0]] and all(c["scale"] == 0.5 and c["kw"]["max_det"] == 7 for c in w["calls"])
    assert all(c["kw"]["edges"] == "edges" and c["tracker"] == "tracker" for c in w["calls"])
    w["finished"].update([2, 1])  # the youngest requests finish first
    tag, people, ids = pipe.wait_one()
    assert tag == "t0" and people[0, 0, 0] == 0 and ids.tolist() == [0] and w["waits"] == [0]  # the oldest was waited for and came first
    pipe.submit(_frame(3), tag="t3")  # goes to an executor that is free, without a wait
    assert w["waits"] == [0] and len(w["calls"]) == 4
    out = pipe.drain()
    assert [t for t, _, _ in out] == ["t1", "t2", "t3"] and [int(p[0, 0, 0]) for _, p, _ in out] == [1, 2, 3]
    with pytest.raises(RuntimeError):
        pipe.wait_one()


def test_pipeline_blocks_only_when_every_executor_is_busy():
    from deepcut_tools import VideoPipeline

    for depth in (1, 2, 4):
        net = FakeNet()
        pipe = VideoPipeline(net, None, depth=depth, stats=STATS, choose_streams=False)
        for k in range(depth):
            pipe.submit(_frame(k), tag=k)
            assert not net.world["waits"], depth
        pipe.submit(_frame(depth), tag=depth)  # request depth + 1: the oldest is waited for, nothing else
        assert net.world["waits"] == [0], depth
        assert net.world["calls"][-1]["net"] == net.world["calls"][0]["net"]  # ... and its executor takes the new one
        assert net.world["calls"][-1]["slot_of"] is None  # no tracker: no slot map
        assert [t for t, _, _ in pipe.drain()] == list(range(depth + 1))


def test_pipeline_gathers_batches_and_flushes_a_partial_one():
    from deepcut_tools import VideoPipeline

    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, batch=3, stats=STATS, choose_streams=False)
    for k in range(2):
        pipe.submit(_frame(k), tag=k, slot=1)
    assert not net.world["calls"]  # held
    pipe.submit(_frame(2), tag=2, slot=0)
    assert len(net.world["calls"]) == 1 and net.world["calls"][0]["n"] == 3 and net.world["calls"][0]["slot_of"] == [1, 1, 0]
    pipe.submit(_frame(3), tag=3)
    pipe.submit(_frame(4, h=8), tag=4)  # another shape: what is held goes out first, alone
    assert [c["n"] for c in net.world["calls"]] == [3, 1]
    pipe.flush()
    assert [c["n"] for c in net.world["calls"]] == [3, 1, 1] and net.world["waits"] == [0]  # two executors: the third call waited for the first
    pipe.submit(_frame(5), tag=5)
    pipe.submit(_frame(6), tag=6)
    out = pipe.drain()  # sends the partial batch of two
    assert [c["n"] for c in net.world["calls"]] == [3, 1, 1, 2]
    assert [t for t, _, _ in out] == list(range(7)) and [int(p[0, 0, 0]) for _, p, _ in out] == list(range(7))
    with pytest.raises(ValueError):
        pipe.submit(np.zeros((4, 6), np.uint8))
