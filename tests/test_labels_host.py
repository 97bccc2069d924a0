"""CPU: the host side of the label overlay (include/deepcut_hip.h: dc_label_people, dc_label_font, dc_overlay_styles) — every refusal
without a device, each before DC_ENOCPU and naming its field; the font against its golden fixture; the geometry of the rule on the
restatement (tests/label_ref.py) alone; the binding's ValueErrors; the `size` of the styles block.

PARITY UNPINNED BY THE REFERENCE: its demo draws with matplotlib and labels nothing; the rule is this project's own."""
import ctypes as C
import os

import numpy as np
import pytest

import label_ref as LR

EINVAL, ENOCPU = -1, -6  # include/deepcut_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ #-.:/%+_?"


@pytest.fixture(scope="module")
def cpu():
    import caffe
    import caffe.pycaffe as pc

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    yield dict(caffe=caffe, pc=pc, lib=pc._lib)
    pc._lib.dc_set_mode(mode)


def _err(lib):
    return (lib.dc_last_error() or b"").decode()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _style(pc, keep, **fields):
    st = pc.LabelStyle()
    pal = np.ascontiguousarray([(255, 0, 0), (0, 255, 0)], np.uint8)
    keep.append(pal)
    st.scale, st.gap, st.anchor_joint, st.alpha_text, st.alpha_plate, st.min_score = 2, 2, -1, 256, 160, 0.0
    st.color_mode, st.palette, st.n_palette = 0, pal.ctypes.data, 2
    st.prefix = b"ID"
    for k, v in fields.items():
        setattr(st, k, v)
    return st


def _call(cpu, nb=1, h=48, w=64, P=3, J=14, n_people=None, texts=None, no_style=False, frame=None, ids=True, **fields):
    pc, lib = cpu["pc"], cpu["lib"]
    keep = []
    img = np.zeros((nb, h, w, 3), np.uint8)
    frames = (pc.DcFrame * nb)()
    for b in range(nb):
        frames[b].plane[0], frames[b].pitch[0], frames[b].format = img[b].ctypes.data, 3 * w, 0
        for k, v in (frame or {}).items():
            setattr(frames[b], k, v) if not isinstance(v, tuple) else getattr(frames[b], k).__setitem__(v[0], v[1])
    n = np.ascontiguousarray([P] * nb if n_people is None else n_people, np.int32)
    ppl = np.ones((nb, P, J, 3), np.float64)
    idv = np.arange(nb * P, dtype=np.int64).reshape(nb, P) if ids else None
    st = _style(pc, keep, **fields)
    rc = lib.dc_label_people(frames, nb, h, w, 0, P, J, _vp(n), _vp(ppl), _vp(idv), _vp(texts), None if no_style else C.byref(st), None)
    return rc, _err(lib)


def _texts(nb, P, rows):
    t = np.zeros((nb, P, 24), np.uint8)
    for (b, p), v in rows.items():
        t[b, p, :len(v)] = np.frombuffer(v, np.uint8)
    return t


REFUSALS = [
    # what dc_draw_people refuses of the frames, the dimensions and n_people
    (dict(nb=65), ("nb",)), (dict(h=16385), ("height",)), (dict(w=0), ("width",)), (dict(P=257), ("P",)), (dict(J=33), ("J",)), (dict(J=0), ("J",)),
    (dict(frame=dict(format=7)), ("format",)), (dict(frame=dict(pitch=(0, 5))), ("pitch",)), (dict(frame=dict(plane=(0, None))), ("plane",)),
    (dict(n_people=[4]), ("n_people[0]", "4")), (dict(nb=2, n_people=[1, -1]), ("n_people[1]", "-1")),
    # the style
    (dict(no_style=True), ("style",)), (dict(palette=None), ("palette",)),
    (dict(scale=0), ("scale",)), (dict(scale=9), ("scale",)), (dict(gap=-1), ("gap",)), (dict(gap=65), ("gap",)),
    (dict(anchor_joint=-2), ("anchor_joint",)), (dict(anchor_joint=14), ("anchor_joint", "14")),
    (dict(alpha_text=257), ("alpha_text",)), (dict(alpha_text=-1), ("alpha_text",)), (dict(alpha_plate=257), ("alpha_plate",)),
    (dict(alpha_plate=-1), ("alpha_plate",)),
    (dict(min_score=float("nan")), ("min_score",)), (dict(min_score=-0.5), ("min_score",)), (dict(min_score=float("inf")), ("min_score",)),
    (dict(color_mode=2), ("color_mode",)), (dict(n_palette=0), ("n_palette",)), (dict(n_palette=257), ("n_palette",)),
    (dict(prefix=b"ABCDE"), ("prefix", "4")), (dict(prefix=b"A!"), ("prefix[1]", "0x21")), (dict(prefix=b"\xe9"), ("prefix[0]", "0xE9")),
    # the texts
    (dict(texts=_texts(1, 3, {(0, 2): b"OK*"})), ("texts[0][2]", "[2]", "0x2A")),
    (dict(texts=_texts(1, 3, {(0, 1): b"X" * 24})), ("texts[0][1]", "NUL")),
    (dict(nb=2, texts=_texts(2, 3, {(1, 0): b"a~"})), ("texts[1][0]", "0x7E")),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_name_the_field_before_a_device_is_needed(cpu, case):
    kw, words = REFUSALS[case]
    rc, msg = _call(cpu, **kw)
    assert rc == EINVAL, (kw, rc, msg)
    for word in words:
        assert word in msg, (kw, msg)


def test_good_arguments_reach_enocpu_at_the_limits(cpu):
    for kw in (dict(), dict(nb=64, P=256, J=32, scale=8, anchor_joint=31, gap=64, texts=_texts(64, 256, {(63, 255): b"abcdefghijklmnopqrstuvw"})),
               dict(ids=False, prefix=b"ab_?", color_mode=1, alpha_text=0, alpha_plate=0, n_palette=1),
               dict(texts=_texts(1, 3, {(0, 0): CHARS[:23].encode(), (0, 1): CHARS[23:].encode()})),
               dict(n_people=[1], texts=_texts(1, 3, {(0, 2): b"!!"}))):  # rows of people beyond n_people are not read
        rc, msg = _call(cpu, **kw)
        assert rc == ENOCPU, (kw, rc, msg)
        assert "CPU mode" in msg


# ---- the font ----------------------------------------------------------------------------------------------------------------------------
def _golden():
    font, name = {}, None
    for line in open(os.path.join(ROOT, "tests", "golden", "label_font_5x7.txt")).read().splitlines():
        if line.startswith("= "):
            name = " " if line[2:] == "space" else line[2:]
            font[name] = []
        elif line:
            assert len(line) == 5 and set(line) <= set(".#"), line
            font[name].append(int(line.replace(".", "0").replace("#", "1"), 2))
    return font


def test_font_equals_the_golden_fixture(cpu):
    caffe, lib = cpu["caffe"], cpu["lib"]
    gold = _golden()
    assert "".join(gold) == CHARS == caffe.LABEL_CHARS and all(len(v) == 7 for v in gold.values())
    assert caffe.LABEL_FONT == {ch: tuple(rows) for ch, rows in gold.items()}
    assert all(rows == (0,) * 7 if ch == " " else any(rows) for ch, rows in caffe.LABEL_FONT.items())
    assert all(0 <= r < 32 for rows in caffe.LABEL_FONT.values() for r in rows)
    assert len(set(caffe.LABEL_FONT.values())) == 46
    rows = (C.c_ubyte * 7)()
    for ch in range(256):
        rc = lib.dc_label_font(ch, C.byref(rows))
        up = chr(ch).upper() if ch < 128 else None
        if up in gold and (chr(ch) in gold or chr(ch).islower()):
            assert rc == 0 and tuple(rows) == tuple(gold[up]), ch  # lower case folds to upper case
        else:
            assert rc == EINVAL and str(ch) in _err(lib), ch
    assert lib.dc_label_font(-1, C.byref(rows)) == EINVAL and lib.dc_label_font(256 + ord("A"), C.byref(rows)) == EINVAL


# ---- the geometry, on the restatement alone ----------------------------------------------------------------------------------------------
def _person(*joints, J=4):
    p = np.zeros((1, J, 3))
    for j, (x, y) in enumerate(joints):
        p[0, j] = (x, y, 1.0)
    return p


def test_geometry_of_the_rule():
    H, W = 70, 101
    one = lambda ppl, **kw: LR.labels(ppl, H, W, **kw)  # noqa: E731
    # n = 1 at scale 2: tw = 10, th = 14, pw = 14, ph = 18; the box corner (40.5, 50.25) -> X = 40, Y = 50 - 2 - 18
    (a,) = one(_person((40.5, 50.25), (60, 64)), ids=[7])
    assert (a["X"], a["Y"], a["pw"], a["ph"], a["text"]) == (40, 30, 14, 18, "7")
    # the anchor centres the label: X = 60 - 7, Y = 64 - 2 - 18
    (a,) = one(_person((40.5, 50.25), (60, 64)), ids=[7], anchor=1)
    assert (a["X"], a["Y"]) == (53, 44)
    # an anchor that is not held falls back to the box
    (a,) = one(_person((40.5, 50.25), (60, 64)), ids=[7], anchor=3)
    assert (a["X"], a["Y"]) == (40, 30)
    # the four clamps
    assert [(v["X"], v["Y"]) for v in one(_person((-30, 40)), ids=[7])] == [(0, 20)]
    assert [(v["X"], v["Y"]) for v in one(_person((40, 5)), ids=[7])] == [(40, 0)]
    assert [(v["X"], v["Y"]) for v in one(_person((99, 40)), ids=[7])] == [(W - 14, 20)]
    assert [(v["X"], v["Y"]) for v in one(_person((40, 500)), ids=[7])] == [(40, H - 18)]
    # wider than the frame: X = 0, cut on the right
    (a,) = one(_person((50, 60)), ids=[2 ** 63 - 1], prefix="ID:#")
    assert a["text"] == "ID:#9223372036854775807" and len(a["text"]) == 23 and a["pw"] == 2 * (6 * 23 + 1) > W and a["X"] == 0
    masks = LR.layers(a, H, W)
    assert masks[0][0][a["Y"], W - 1] and masks[0][0].shape == (H, W)
    (a,) = one(_person((50, 60)), ids=[2 ** 63 - 1], scale=1)
    assert len(a["text"]) == 19 and a["pw"] == 6 * 19 + 1
    # no label: key -1, no held joint, both alphas 0; a text of its own labels an untracked person
    assert one(_person((50, 60)), ids=[-1]) == []
    assert one(np.full((1, 4, 3), np.nan), ids=[3]) == [] and one(_person((50, 60)), ids=[3], min_score=1.0) == []
    assert one(_person((50, 60)), ids=[3], alpha_text=0, alpha_plate=0) == []
    assert [v["text"] for v in one(_person((50, 60)), ids=[-1], texts=["who?"])] == ["WHO?"]
    assert [v["text"] for v in one(_person((50, 60)), ids=[5], texts=[""])] == ["5"]
    # the layers: one alpha 0 leaves the other
    (a,) = one(_person((50, 60)), ids=[3], alpha_plate=0)
    assert len(LR.layers(a, H, W)) == 1
    # the text layer of "1" at scale 1 is the glyph, one pixel inside the plate
    (a,) = one(_person((50, 60)), ids=[1], scale=1, alpha_plate=0)
    (m, _, _), = LR.layers(a, H, W)
    got = [int("".join("1" if v else "0" for v in m[a["Y"] + 1 + r, a["X"] + 1:a["X"] + 6]), 2) for r in range(7)]
    assert tuple(got) == LR.font()["1"] and m.sum() == sum(bin(r).count("1") for r in LR.font()["1"])


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_python_value_errors(cpu):
    caffe = cpu["caffe"]
    img = np.zeros((32, 32, 3), np.uint8)
    ppl = np.ones((2, 14, 3))
    with pytest.raises(ValueError, match="texts.0..1.*'~'"):
        caffe.label_people(img, ppl, texts=["ok", "a~"])
    with pytest.raises(ValueError, match="24 characters"):
        caffe.label_people(img, ppl, texts=["x" * 24])
    with pytest.raises(ValueError, match="prefix.*5 characters"):
        caffe.label_people(img, ppl, prefix="ABCDE")
    with pytest.raises(ValueError, match="prefix.*'!'"):
        caffe.label_people(img, ppl, prefix="A!")
    with pytest.raises(ValueError, match="color"):
        caffe.label_people(img, ppl, color="rainbow")
    with pytest.raises(ValueError, match="3 texts for 2 people"):
        caffe.label_people(img, ppl, texts=["a", "b", "c"])
    with pytest.raises(ValueError, match="ids"):
        caffe.label_people(img, ppl, ids=[1, 2, 3])
    for bad in (dict(texts=[["a"]]), dict(stream=1)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            caffe.pycaffe._label_overlay_struct(bad)
    # good arguments go to the library, which has no CPU path; lower case is folded by the binding
    with pytest.raises(caffe.DeepcutError, match="CPU mode"):
        caffe.label_people(img, ppl, ids=[3, -1], texts=["abc xyz", None], prefix="id:", anchor=13, color="text")
    assert set(caffe.LABEL_DEFAULTS) == {"scale", "gap", "anchor", "prefix", "alpha_text", "alpha_plate", "min_score", "color", "palette", "text_color",
                                         "plate_color"}


# ---- the styles block ----------------------------------------------------------------------------------------------------------------------
def _device_call(cpu, size=None, draw=False, labels=True, old=False, **fields):
    pc, lib = cpu["pc"], cpu["lib"]
    keep = []
    nb, h, w, P, J = 1, 48, 64, 3, 14
    img = np.zeros((nb, h, w, 3), np.uint8)
    frames = (pc.DcFrame * nb)()
    frames[0].plane[0], frames[0].pitch[0], frames[0].format = img[0].ctypes.data, 3 * w, 0
    n, ppl = np.ascontiguousarray([P], np.int32), np.ones((nb, P, J, 3), np.float64)  # never read: the call ends before a device is needed
    if old:
        return lib.dc_overlay_people_device(frames, nb, h, w, 0, P, J, _vp(n), _vp(ppl), None, None, None, None, None, -1, None, -1, None, None), _err(lib)
    st = pc.OverlayStyles()
    st.size = C.sizeof(pc.OverlayStyles) if size is None else size
    lab = _style(pc, keep, **fields)
    if labels:
        st.labels = C.pointer(lab)
    st.n_only = st.n_keep = -1
    return lib.dc_overlay_people_device_styles(frames, nb, h, w, 0, P, J, _vp(n), _vp(ppl), None, None, C.byref(st), None, None), _err(lib)


def test_styles_block_size_and_label_style(cpu):
    pc = cpu["pc"]
    full = C.sizeof(pc.OverlayStyles)
    assert _device_call(cpu)[0] == ENOCPU  # labels alone are an overlay
    for size in (0, 8, pc.OverlayStyles.redact.offset + 7, full + 1, full + 64):
        rc, msg = _device_call(cpu, size=size)
        assert rc == EINVAL and "size" in msg and str(size) in msg, (size, msg)
    # a caller compiled before `labels` existed: the field is not read, and nothing is left to do
    rc, msg = _device_call(cpu, size=pc.OverlayStyles.labels.offset)
    assert rc == EINVAL and "style" in msg, msg
    rc, msg = _device_call(cpu, labels=False)
    assert rc == EINVAL and "style" in msg, msg
    # the label style is refused in dc_label_people's words
    for fields, word in ((dict(scale=9), "scale"), (dict(anchor_joint=14), "anchor_joint"), (dict(prefix=b"a,"), "prefix[1]"), (dict(palette=None), "palette")):
        rc, msg = _device_call(cpu, **fields)
        assert rc == EINVAL and word in msg and "overlay_people_device" in msg, (fields, msg)


def test_old_entries_still_refuse_both_styles_null(cpu):
    rc, msg = _device_call(cpu, old=True)
    assert rc == EINVAL and "null argument: style (a draw style, a redact style or both)" in msg, msg
    caffe = cpu["caffe"]
    class Shaped(object):  # the styles are looked at before the tensors
        shape = (1, 3, 14, 3)

    with pytest.raises(ValueError, match="draw=, redact= or both"):
        caffe.overlay_people_device(np.zeros((8, 8, 3), np.uint8), Shaped(), None)


def test_chain_styles_entry_checks_size_and_label_style(cpu):
    """dc_net_track_frames_async_styles without a device: the block's `size`, then the label style in dc_label_people's words; good
    arguments reach the mode check; with no style at all it is dc_net_track_frames_async."""
    import people_ref as R
    from deepcut_tools import deepercut_prototxt

    caffe, pc, lib = cpu["caffe"], cpu["pc"], cpu["lib"]
    net = caffe.Net(deepercut_prototxt(152, 64, 64, 2), caffe.TEST, from_text=True)
    tracker = caffe.Tracker(n_joints=14, slots=2)
    H, W = 37, 53
    img = np.zeros((2, H, W, 3), np.uint8)
    e = np.ascontiguousarray(R.all_pairs_edges())
    full = C.sizeof(pc.OverlayStyles)

    def call(size=full, labels=True, with_tracker=True, **fields):
        keep = []
        q = pc.AssembleParams(1.0, 0.5, 1, 8, 20.0, 0.5, 8, 1)
        count, people, ids = np.zeros(2, np.int32), np.zeros((2, 8, 14, 3)), np.zeros((2, 8), np.int64)
        st = pc.OverlayStyles()
        st.size, st.n_only, st.n_keep = size, -1, -1
        lab = _style(pc, keep, **fields)
        if labels:
            st.labels = C.pointer(lab)
        rc = lib.dc_net_track_frames_async_styles(net._h, tracker._h if with_tracker else None, None, _vp(img), 2, H, W, 1.0, 0, None, C.byref(q), 182,
                                                  _vp(e), None, None, None, _vp(count), _vp(people), None, _vp(ids) if with_tracker else None, None,
                                                  C.byref(st), None)
        return rc, _err(lib)

    for size in (0, 8, pc.OverlayStyles.redact.offset + 7, full + 1):
        rc, msg = call(size=size)
        assert rc == EINVAL and "track_frames_async" in msg and "size" in msg and str(size) in msg, (size, msg)
    for fields, word in ((dict(scale=0), "scale"), (dict(gap=65), "gap"), (dict(anchor_joint=14), "anchor_joint"), (dict(prefix=b"a;"), "prefix[1]")):
        rc, msg = call(**fields)
        assert rc == EINVAL and word in msg and "track_frames_async" in msg, (fields, msg)
    for kw in (dict(), dict(with_tracker=False), dict(labels=False), dict(size=pc.OverlayStyles.labels.offset, scale=0)):  # the last two: the plain chain
        rc, msg = call(**kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, msg)
    # through Python: the label style's names are checked by the binding, its values by the library
    kw = dict(edges=R.all_pairs_edges(), max_cost=20.0, seed_threshold=0.5)
    with pytest.raises(ValueError, match="texts"):
        net.track_frames_async(img, tracker, labels=dict(texts=[["a"]]), **kw)
    with pytest.raises(ValueError, match="stream"):
        net.track_frames_async(img, tracker, labels=dict(stream=3), **kw)
    with pytest.raises(caffe.DeepcutError) as ei:
        net.track_frames_async(img, tracker, labels=dict(scale=9), **kw)
    assert ei.value.code == EINVAL and "scale" in str(ei.value)
    with pytest.raises(caffe.DeepcutError) as ei:
        net.track_frames_async(img, None, labels=True, **kw)
    assert ei.value.code == ENOCPU and not img.any()


# ---- labels= of the pipeline, of track_people and of the demo, on a fake net -------------------------------------------------------------
def test_labels_travel_with_the_request_in_chain_and_are_written_on_the_host_route(monkeypatch):
    import pose.people as pp
    from deepcut_tools import VideoPipeline
    from test_video_host import STATS, FakeNet, _frame

    written = []
    monkeypatch.setattr(pp, "label_people", lambda frame, people, ids=None, **style: written.append((int(frame[0, 0, 0]), style)))
    frames = [_frame(k) for k in range(3)]
    # in the chain: the style goes with every request and nothing is called when a request is collected
    net = FakeNet()
    out = list(pp.track_people(frames, None, None, STATS, tracker="tracker", net=net, in_chain=True, labels=dict(scale=3, prefix="id")))
    assert [int(p[0, 0, 0]) for p, _ in out] == [0, 1, 2] and not written
    assert all(c["kw"]["labels"] == dict(scale=3, prefix="id") and c["kw"].get("draw") is None for c in net.world["calls"])
    # the host route, in flight: label_people per frame, nothing about the style reaches the net
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, stats=STATS, choose_streams=False, labels=True)
    for f in frames:
        pipe.submit(f)
    assert len(pipe.drain()) == 3 and [v for v, _ in written] == [0, 1, 2] and all(style == {} for _, style in written)
    assert all("labels" not in c["kw"] for c in net.world["calls"])
    # off: nothing is added
    written[:] = []
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", stats=STATS, choose_streams=False, in_chain=True, labels=None)
    pipe.submit(frames[0])
    pipe.drain()
    assert not written and all("labels" not in c["kw"] for c in net.world["calls"])
    # refusals: texts and stream cannot go into the chain; the host route takes texts
    for bad in (dict(texts=[["a"]]), dict(stream=5)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            list(pp.track_people(frames, None, None, STATS, tracker="tracker", net=FakeNet(), in_chain=True, labels=bad))
    VideoPipeline(FakeNet(), "tracker", stats=STATS, in_chain=False, labels=dict(texts=[["a"]]))
    with pytest.raises(ValueError, match="labels must be"):
        list(pp.track_people(frames, None, None, STATS, tracker="tracker", net=FakeNet(), labels="yes"))


def test_demo_has_a_labels_flag():
    from pose.pose_demo import predict_pose_from

    flag = [p for p in predict_pose_from.params if p.name == "labels"]
    assert len(flag) == 1 and flag[0].is_flag and flag[0].default is False and "--labels" in flag[0].opts
