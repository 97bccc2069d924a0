"""CPU: the host side of the overlays made from people in device memory (include/deepcut_hip.h: dc_overlay_people_device,
dc_net_track_frames_async_overlay) — the two symbols and their ctypes signatures, every refusal without a device (each before DC_ENOCPU,
worded like dc_draw_people's and dc_redact_people's), and `in_chain=True` of VideoPipeline / track_people on a fake net: the styles travel
with the request and neither `draw_people` nor `redact_people` is called.

PARITY UNPINNED BY THE REFERENCE, which draws with matplotlib on the host and redacts nothing; the rules are this project's own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import people_ref as R
from test_video_host import STATS, FakeNet, _frame

EINVAL, ENOCPU = -1, -6  # include/deepcut_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dc_overlay_people_device": 19, "dc_net_track_frames_async_overlay": 28}  # the entries and how many arguments they take


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_symbols_are_declared_exported_and_bound():
    import caffe
    import caffe.pycaffe as pc

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepcut_hip.h")).read(), flags=re.S)
    lib = C.CDLL(caffe.lib_path())
    for name, n_args in NEW.items():
        decl = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert hasattr(lib, name) and name in pc.EXPORTED_SYMBOLS
        fn = getattr(pc._lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
        assert C.POINTER(pc.DrawStyle) in fn.argtypes and C.POINTER(pc.RedactStyle) in fn.argtypes
    # the chain entry is dc_net_track_frames_async's arguments and then the overlay's
    old, new = pc._lib.dc_net_track_frames_async.argtypes, pc._lib.dc_net_track_frames_async_overlay.argtypes
    assert list(new[:len(old)]) == list(old) and list(new[len(old):]) == list(pc._lib.dc_overlay_people_device.argtypes[11:18])
    assert hasattr(caffe, "overlay_people_device")


@pytest.fixture(scope="module")
def cpu():
    import caffe
    import caffe.pycaffe as pc
    from deepcut_tools import deepercut_prototxt

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    net = caffe.Net(deepercut_prototxt(152, 64, 64, 2), caffe.TEST, from_text=True)
    yield dict(caffe=caffe, pc=pc, lib=pc._lib, net=net, two=caffe.Tracker(n_joints=14, slots=2))
    pc._lib.dc_set_mode(mode)


def _err(lib):
    return (lib.dc_last_error() or b"").decode()


# ---- the styles, good except what a case overrides ---------------------------------------------------------------------------------------
def _styles(pc, keep, draw=None, redact=None):
    """-> (DrawStyle, RedactStyle); draw / redact: the fields a case sets (edges / palette: a list, or None for a null pointer)."""
    d, r = pc.DrawStyle(), pc.RedactStyle()
    edges = np.ascontiguousarray([(0, 1), (1, 2)], np.int32)
    palette = np.ascontiguousarray([(255, 0, 0), (0, 255, 0)], np.uint8)
    keep += [edges, palette]
    d.n_edges, d.edges, d.joint_radius, d.limb_radius, d.alpha, d.alpha_filled, d.min_score = 2, edges.ctypes.data, 4.0, 2.0, 256, 128, 0.0
    d.color_mode, d.palette, d.n_palette = 0, palette.ctypes.data, 2
    r.region, r.head_a, r.head_b = 0, 0, 1
    r.head_scale, r.body_scale, r.min_radius, r.max_radius, r.min_score = 0.75, 0.06, 4.0, 256.0, 0.0
    r.n_edges, r.edges, r.effect, r.block = 2, edges.ctypes.data, 0, 8
    for st, fields in ((d, draw or {}), (r, redact or {})):
        for k, v in fields.items():
            if k in ("edges", "palette") and v is not None:
                a = np.ascontiguousarray(v, np.uint8 if k == "palette" else np.int32)
                keep.append(a)
                v = a.ctypes.data
                if k == "edges" and "n_edges" not in fields:
                    st.n_edges = a.shape[0]
            setattr(st, k, v)
    return d, r


STYLE_CASES = [
    # what dc_draw_people refuses of its style ...
    (dict(draw=dict(n_edges=-1)), ("n_edges",)), (dict(draw=dict(n_edges=129)), ("n_edges",)), (dict(draw=dict(edges=None)), ("edges",)),
    (dict(draw=dict(edges=[(0, 1), (3, 14)])), ("edges[1]", "14")),
    (dict(draw=dict(joint_radius=64.5)), ("joint_radius",)), (dict(draw=dict(limb_radius=float("nan"))), ("limb_radius",)),
    (dict(draw=dict(alpha=257)), ("alpha",)), (dict(draw=dict(alpha_filled=-1)), ("alpha_filled",)),
    (dict(draw=dict(min_score=-0.1)), ("min_score",)), (dict(draw=dict(color_mode=2)), ("color_mode",)),
    (dict(draw=dict(palette=None)), ("palette",)), (dict(draw=dict(n_palette=0)), ("n_palette",)), (dict(draw=dict(n_palette=257)), ("n_palette",)),
    # ... what dc_redact_people refuses of its style ...
    (dict(redact=dict(region=3)), ("region",)), (dict(redact=dict(effect=2)), ("effect",)), (dict(redact=dict(block=6)), ("block",)),
    (dict(redact=dict(head_a=14)), ("head_a", "14")), (dict(redact=dict(head_b=-1)), ("head_b",)),
    (dict(redact=dict(head_a=5, head_b=5)), ("head_a", "head_b")),
    (dict(redact=dict(head_scale=-0.5)), ("head_scale",)), (dict(redact=dict(body_scale=float("inf"))), ("body_scale",)),
    (dict(redact=dict(min_radius=-1.0)), ("min_radius",)), (dict(redact=dict(max_radius=1024.5)), ("max_radius",)),
    (dict(redact=dict(min_radius=8.0, max_radius=7.5)), ("min_radius", "max_radius")), (dict(redact=dict(min_score=float("nan"))), ("min_score",)),
    (dict(redact=dict(edges=[(-1, 1)])), ("edges[0]", "-1")), (dict(redact=dict(n_edges=129)), ("n_edges",)),
    # ... and the new ones
    (dict(no_draw=True, no_redact=True), ("style",)),
    (dict(n_only=257), ("only_ids", "256")), (dict(n_keep=300), ("keep_ids", "256")),
    (dict(n_only=2, null_only=True), ("only_ids",)), (dict(n_keep=1, null_keep=True), ("keep_ids",)),
    (dict(n_only=1, no_ids=True), ("ids is needed",)), (dict(n_keep=0, no_ids=True), ("ids is needed",)),
    (dict(n_only=1, no_redact=True), ("only_ids", "redact style")),
]
GOOD = [dict(), dict(no_draw=True), dict(no_redact=True), dict(n_only=0), dict(n_only=256, n_keep=256), dict(n_keep=3),
        dict(draw=dict(n_edges=0, joint_radius=0.0, limb_radius=0.0)), dict(redact=dict(region=2, effect=1, block=32, n_edges=0))]


def _overlay_tail(pc, keep, kw):
    """The overlay's arguments of both entries except `redacted`: draw, redact, only_ids, n_only, keep_ids, n_keep."""
    d, r = _styles(pc, keep, kw.get("draw"), kw.get("redact"))
    lists = np.arange(300, dtype=np.int64)
    keep += [d, r, lists]
    n_only, n_keep = kw.get("n_only", -1), kw.get("n_keep", -1)
    return (None if kw.get("no_draw") else C.byref(d), None if kw.get("no_redact") else C.byref(r), None if kw.get("null_only") else _vp(lists), n_only,
            None if kw.get("null_keep") else _vp(lists), n_keep)


def _device_entry(pc, H=20, W=30, fmt=1, nb=2, P=4, J=14, frames=None, **kw):
    """dc_overlay_people_device through ctypes in CPU mode: nothing is read through the people's pointers -> (rc, message)."""
    keep = []
    y, uv, bgr = np.zeros((H, W), np.uint8), np.zeros(((H + 1) // 2, (W + 1) // 2, 2), np.uint8), np.zeros((H, W, 3), np.uint8)
    arr = (pc.DcFrame * max(nb, 1))()
    for f in arr:
        if fmt == 0:
            f.plane[0], f.pitch[0] = bgr.ctypes.data, 3 * W
        else:
            f.plane[0], f.plane[1], f.pitch[0], f.pitch[1] = y.ctypes.data, uv.ctypes.data, W, 2 * ((W + 1) // 2)
        f.format = fmt
    if frames:
        frames(arr)
    some = np.zeros(8, np.int64)  # stands for device memory: refused or ENOCPU before anything is read
    rc = pc._lib.dc_overlay_people_device(arr, nb, H, W, 0, P, J, _vp(some), _vp(some), None, None if kw.get("no_ids") else _vp(some),
                                          *(_overlay_tail(pc, keep, kw) + (None, None)))
    return rc, _err(pc._lib)


def test_device_entry_refuses_like_the_synchronous_entries_before_enocpu(cpu):
    pc = cpu["pc"]

    def frame1(field, value, k=None):
        def change(arr):
            if k is None:
                setattr(arr[1], field, value)
            else:
                getattr(arr[1], field)[k] = value
        return change

    cases = [
        (dict(frames=frame1("plane", None, 1)), ("frame 1", "plane[1]")), (dict(frames=frame1("pitch", 29, 0)), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("format", 7)), ("frame 1", "format")), (dict(frames=frame1("matrix", 1)), ("frame 1", "matrix", "differs")),
        (dict(nb=0), ("nb",)), (dict(nb=65), ("nb",)), (dict(P=0), ("P",)), (dict(P=257), ("P",)), (dict(J=0), ("J",)), (dict(J=33), ("J",)),
        (dict(W=16385), ("width",)), (dict(H=16385, W=1), ("height",)),
        (dict(draw=dict(edges=[(0, 1), (2, 3)]), J=3), ("edges[1]",)), (dict(redact=dict(head_a=12, head_b=13), J=13), ("head_b",)),
    ] + STYLE_CASES
    for kw, words in cases:
        rc, msg = _device_entry(pc, **kw)
        assert rc == EINVAL and "overlay_people_device" in msg and all(w in msg for w in words), (kw, rc, msg)
    for kw in GOOD + [dict(fmt=0), dict(nb=64, P=256, J=32)]:
        rc, msg = _device_entry(pc, **kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, rc, msg)
    assert pc._lib.dc_overlay_people_device(None, 1, 4, 4, 0, 1, 2, None, None, None, None, None, None, None, -1, None, -1, None, None) == EINVAL


def test_chain_entry_refuses_what_both_refuse_before_enocpu(cpu):
    """dc_net_track_frames_async_overlay without a device: what dc_net_track_frames_async refuses first, then the overlay's refusals in
    the words of the synchronous entries; good arguments reach the mode check; with no style it is dc_net_track_frames_async."""
    caffe, pc, lib, net, two = cpu["caffe"], cpu["pc"], cpu["lib"], cpu["net"], cpu["two"]
    H, W = 37, 53
    y, uv = np.zeros((H, W), np.uint8), np.zeros((19, 27, 2), np.uint8)
    frame = caffe.Frame.nv12(y, uv)
    img = np.zeros((2, H, W, 3), np.uint8)
    e = np.ascontiguousarray(R.all_pairs_edges())

    def call(tracker=two, images=None, slot_of=None, max_people=8, **kw):
        keep = []
        q = pc.AssembleParams(1.0, 0.5, 1, 8, 20.0, 0.5, max_people, 1)
        count, people = np.zeros(2, np.int32), np.zeros((2, max(max_people, 1), 14, 3))
        ids, red = np.zeros((2, max(max_people, 1)), np.int64), np.full((2, max(max_people, 1)), -7, np.int32)
        arr = None if images is not None else (pc.DcFrame * 2)(frame.c_frame(), frame.c_frame())
        m = None if slot_of is None else np.ascontiguousarray(slot_of, np.int32)
        rc = lib.dc_net_track_frames_async_overlay(net._h, None if tracker is None else tracker._h, arr, _vp(images), 2, H, W, 1.0, 0, _vp(m),
                                                   C.byref(q), 182, _vp(e), None, None, None, _vp(count), _vp(people), None,
                                                   None if tracker is None else _vp(ids), None, *(_overlay_tail(pc, keep, kw) + (_vp(red),)))
        assert (red == -7).all()
        return rc, _err(lib)

    # the chain's own refusals come first ...
    rc, msg = call(slot_of=[0, 2], draw=dict(alpha=300))
    assert rc == EINVAL and "slot_of[1]" in msg, msg
    rc, msg = call(max_people=257, draw=dict(alpha=300))
    assert rc == EINVAL and "max_people" in msg, msg
    # ... then every refusal of the styles and the lists
    for kw, words in STYLE_CASES:
        if kw.get("no_draw") and kw.get("no_redact"):
            continue  # no style at all: the plain chain, below
        if kw.get("no_ids"):
            kw = dict({k: v for k, v in kw.items() if k != "no_ids"}, tracker=None)  # in the chain the ids are the tracker's
        rc, msg = call(**kw)
        assert rc == EINVAL and "track_frames_async" in msg and all(w in msg for w in words), (kw, rc, msg)
    for kw in GOOD + [dict(images=img), dict(tracker=None), dict(no_draw=True, no_redact=True)]:
        rc, msg = call(**kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, rc, msg)
    # through Python
    kw = dict(edges=R.all_pairs_edges(), max_cost=20.0, seed_threshold=0.5)
    with pytest.raises(caffe.DeepcutError) as ei:
        net.track_frames_async(img, two, draw=dict(alpha=300), **kw)
    assert ei.value.code == EINVAL and "alpha" in str(ei.value)
    with pytest.raises(caffe.DeepcutError) as ei:
        net.track_frames_async(img, two, draw=dict(edges=[(0, 1)]), redact=dict(head=(12, 13), only_ids=[3]), **kw)
    assert ei.value.code == ENOCPU
    with pytest.raises(ValueError, match="select"):
        net.track_frames_async(img, two, redact=dict(head=(12, 13), select=np.ones((2, 8))), **kw)
    with pytest.raises(ValueError, match="ids is needed"):
        net.track_frames_async(img, None, redact=dict(head=(12, 13), keep_ids=[1]), **kw)
    with pytest.raises(ValueError, match="head"):
        net.track_frames_async(img, two, redact=dict(), **kw)  # the library knows no skeleton
    frozen = img.copy()
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="writable"):
        net.track_frames_async(frozen, two, draw=dict(), **kw)
    with pytest.raises(ValueError, match="writable"):
        net.track_frames_async(caffe.Frame.bgr(frozen[0]), two, draw=dict(), **kw)
    assert not img.any()


def test_python_device_entry_refusals(cpu):
    caffe = cpu["caffe"]

    class Tensor(object):  # what the binding asks of a device tensor
        def __init__(self, shape, dtype, ptr=4096):
            self.shape, self.dtype, self.ptr = shape, dtype, ptr

        def data_ptr(self):
            return self.ptr

    img = np.zeros((20, 30, 3), np.uint8)
    people, n = Tensor((1, 4, 14, 3), "torch.float64"), Tensor((1,), "torch.int32")
    with pytest.raises(ValueError, match="draw=, redact= or both"):
        caffe.overlay_people_device(img, people, n)
    with pytest.raises(ValueError, match="people"):
        caffe.overlay_people_device(img, Tensor((2, 4, 14, 3), "torch.float64"), n, draw={})
    with pytest.raises(ValueError, match="float64"):
        caffe.overlay_people_device(img, Tensor((1, 4, 14, 3), "torch.float32"), n, draw={})
    with pytest.raises(ValueError, match="n_people"):
        caffe.overlay_people_device(img, people, np.ones(1, np.int32), draw={})
    with pytest.raises(ValueError, match="ids"):
        caffe.overlay_people_device(img, people, n, ids=Tensor((1, 5), "torch.int64"), draw={})
    with pytest.raises(ValueError, match="select"):
        caffe.overlay_people_device(img, people, n, redact=dict(head=(12, 13), select=[1, 0, 1, 1]))
    with pytest.raises(ValueError, match="ids is needed"):
        caffe.overlay_people_device(img, people, n, redact=dict(head=(12, 13), only_ids=[3]))
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.overlay_people_device(img, people, n, redact=dict(head=(12, 14)))
    assert ei.value.code == EINVAL and "head_b" in str(ei.value)
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.overlay_people_device(img, people, n, ids=Tensor((1, 4), "torch.int64"), draw=dict(edges=[(0, 1)]),
                                    redact=dict(head=(12, 13), keep_ids=[3]), redacted=Tensor((1, 4), "torch.int32"))
    assert ei.value.code == ENOCPU and not img.any()


# ---- in_chain= of the pipeline and of track_people on a fake net -----------------------------------------------------------------------
def test_in_chain_sends_the_styles_with_the_request_and_calls_neither_entry(monkeypatch):
    import caffe
    import caffe.pycaffe as pc
    import pose
    import pose.people as pp
    from deepcut_tools import VideoPipeline

    for mod in (caffe, pc, pose, pp):  # with the synchronous entries REMOVED nothing can call them
        monkeypatch.delattr(mod, "redact_people")
        monkeypatch.delattr(mod, "draw_people")
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, batch=2, stats=STATS, choose_streams=False, in_chain=True, redact=dict(block=16, only_ids=[3]),
                         draw=dict(alpha=96))
    frames = [_frame(k) for k in range(5)]
    for k, f in enumerate(frames):
        pipe.submit(f, tag=k)
    out = pipe.drain()
    assert [t for t, _, _ in out] == list(range(5)) and [int(p[0, 0, 0]) for _, p, _ in out] == list(range(5))
    calls = net.world["calls"]
    assert [c["n"] for c in calls] == [2, 2, 1]
    for c in calls:  # the styles travel with every request, with what pose.draw_people / pose.redact_people fill in on the host route
        assert c["kw"]["draw"] == dict(alpha=96, edges=pp.SKELETON_MPII14)
        assert c["kw"]["redact"] == dict(block=16, only_ids=[3], head=pp.HEAD_MPII14, edges=pp.SKELETON_MPII14)
    # the default stays the host route: nothing about the styles reaches the net
    monkeypatch.setattr(pp, "redact_people", lambda *a, **k: None, raising=False)
    monkeypatch.setattr(pp, "draw_people", lambda *a, **k: None, raising=False)
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", stats=STATS, choose_streams=False, redact=dict(block=16), draw=True)
    pipe.submit(frames[0])
    pipe.drain()
    assert all("draw" not in c["kw"] and "redact" not in c["kw"] for c in net.world["calls"])
    # in_chain without a style adds nothing either
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", stats=STATS, choose_streams=False, in_chain=True)
    pipe.submit(frames[0])
    pipe.drain()
    assert all("draw" not in c["kw"] and "redact" not in c["kw"] for c in net.world["calls"])


def test_in_chain_refusals():
    import pose.people as pp
    from deepcut_tools import VideoPipeline

    with pytest.raises(ValueError, match="select"):
        VideoPipeline(FakeNet(), "tracker", stats=STATS, in_chain=True, redact=dict(select=[1, 0]))
    VideoPipeline(FakeNet(), "tracker", stats=STATS, in_chain=False, redact=dict(select=[1, 0]))  # the host route takes a mask
    with pytest.raises(ValueError, match="ids is needed"):
        VideoPipeline(FakeNet(), None, stats=STATS, in_chain=True, redact=dict(keep_ids=[4]))
    with pytest.raises(ValueError, match="stream"):
        VideoPipeline(FakeNet(), "tracker", stats=STATS, in_chain=True, draw=dict(stream=5))
    with pytest.raises(ValueError, match="select"):
        list(pp.track_people([_frame(0)], None, None, STATS, tracker="tracker", net=FakeNet(), in_chain=True, redact=dict(select=[1])))


def test_track_people_in_chain_goes_through_the_pipeline_at_depth_one():
    import pose.people as pp

    net = FakeNet()
    frames = [_frame(k) for k in range(3)]
    out = list(pp.track_people(frames, None, None, STATS, tracker="tracker", net=net, in_chain=True, redact=dict(region="body"), draw=True))
    assert [int(p[0, 0, 0]) for p, _ in out] == [0, 1, 2]
    assert all(c["kw"]["redact"]["region"] == "body" and c["kw"]["draw"] == dict(edges=pp.SKELETON_MPII14) for c in net.world["calls"])
    plain = list(pp.track_people([_frame(k) for k in range(3)], None, None, STATS, tracker="tracker", depth=1, batch=2, net=FakeNet()))
    for (p0, i0), (p1, i1) in zip(plain, out):
        assert np.array_equal(p0, p1)
