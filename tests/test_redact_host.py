"""CPU: the host side of the redaction (include/deepcut_hip.h, dc_redact_people) — the symbol, every refusal of the entry without a device
(each before DC_ENOCPU, naming the field), properties of the numpy restatement itself (tests/redact_ref.py: the mosaic is idempotent, the
result does not depend on the order of people, only bytes of selected blocks change), only_ids / keep_ids -> select, and the `redact=`
switch of VideoPipeline / track_people on a fake net.

PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind; the rule is this project's own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import redact_ref as RR
from test_video_host import STATS, FakeNet, _frame

EINVAL, ENOCPU = -1, -6  # include/deepcut_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKELETON = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7), (7, 8), (8, 12), (12, 9), (9, 10), (10, 11), (12, 13), (2, 8), (3, 9))


def test_symbol_is_declared_exported_and_bound():
    import caffe
    import caffe.pycaffe as pc

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepcut_hip.h")).read(), flags=re.S)
    assert re.search(r"\bdc_redact_people\s*\(", text) and "typedef struct dc_redact_style" in text
    for name, value in (("DC_REDACT_HEAD", 0), ("DC_REDACT_BODY", 1), ("DC_REDACT_HEAD_OR_BODY", 2), ("DC_REDACT_MOSAIC", 0), ("DC_REDACT_FILL", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert hasattr(C.CDLL(caffe.lib_path()), "dc_redact_people") and "dc_redact_people" in pc.EXPORTED_SYMBOLS
    # the ctypes struct has the header's fields in the header's order
    body = re.search(r"typedef struct dc_redact_style \{(.*?)\} dc_redact_style;", text, flags=re.S).group(1)
    names = [n for n in re.findall(r"[A-Za-z_]\w*", body) if n not in ("int", "double", "const", "unsigned", "char")]
    assert names == [f[0] for f in pc.RedactStyle._fields_], names


# ---- the entry's refusals, without a device --------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_mode():
    import caffe
    import caffe.pycaffe as pc

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    yield caffe, pc
    pc._lib.dc_set_mode(mode)


def _raw(pc, H=20, W=30, fmt=1, nb=2, P=4, J=14, frames=None, n_people=None, null_style=False, **style):
    """dc_redact_people through ctypes with good arguments except what the caller overrides -> (rc, message, redacted)."""
    y, uv = np.zeros((H, W), np.uint8), np.zeros(((H + 1) // 2, (W + 1) // 2, 2), np.uint8)
    bgr = np.zeros((H, W, 3), np.uint8)
    arr = (pc.DcFrame * max(nb, 1))()
    for f in arr:
        if fmt == 0:
            f.plane[0], f.pitch[0] = bgr.ctypes.data, 3 * W
        else:
            f.plane[0], f.plane[1], f.pitch[0], f.pitch[1] = y.ctypes.data, uv.ctypes.data, W, 2 * ((W + 1) // 2)
        f.format = fmt
    if frames:
        frames(arr)
    n = np.ascontiguousarray([1] * max(nb, 1) if n_people is None else n_people, np.int32)
    people = np.ones((max(nb, 1), max(P, 1), max(J, 1), 3))
    given = style.pop("edges", [(0, 1), (1, 2)])
    edges = np.ascontiguousarray([] if given is None else given, np.int32).reshape(-1, 2)
    st = pc.RedactStyle()
    st.region, st.head_a, st.head_b = 0, 0, 1
    st.head_scale, st.body_scale, st.min_radius, st.max_radius, st.min_score = 0.75, 0.06, 4.0, 256.0, 0.0
    st.n_edges, st.edges = style.pop("n_edges", edges.shape[0]), None if given is None else edges.ctypes.data
    st.effect, st.block = 0, 8
    for k, v in style.items():
        setattr(st, k, v)
    redacted = np.full((max(nb, 1), max(P, 1)), -7, np.int32)
    rc = pc._lib.dc_redact_people(arr, nb, H, W, 0, P, J, n.ctypes.data_as(C.c_void_p), people.ctypes.data_as(C.c_void_p), None,
                                  None if null_style else C.byref(st), redacted.ctypes.data_as(C.c_void_p), None)
    return rc, (pc._lib.dc_last_error() or b"").decode(), redacted


def test_every_argument_error_is_einval_naming_the_field_before_enocpu(cpu_mode):
    _caffe, pc = cpu_mode

    def frame1(field, value, k=None):
        def change(arr):
            if k is None:
                setattr(arr[1], field, value)
            else:
                getattr(arr[1], field)[k] = value
        return change

    nan, inf = float("nan"), float("inf")
    cases = [
        # what dc_draw_people refuses of frames, nb, height, width, P, J, n_people and edges
        (dict(frames=frame1("plane", None, 1)), ("frame 1", "plane[1]")),
        (dict(frames=frame1("plane", None, 0), fmt=0), ("frame 1", "plane[0]")),
        (dict(frames=frame1("pitch", 29, 0)), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("pitch", 28, 1)), ("frame 1", "pitch[1]")),
        (dict(frames=frame1("pitch", 89, 0), fmt=0), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("format", 7)), ("frame 1", "format")),
        (dict(frames=frame1("matrix", 2)), ("frame 1", "matrix")),
        (dict(frames=frame1("range", -1)), ("frame 1", "range")),
        (dict(frames=frame1("format", 0)), ("frame 1", "format", "differs")),
        (dict(frames=frame1("matrix", 1)), ("frame 1", "matrix", "differs")),
        (dict(frames=frame1("range", 1)), ("frame 1", "range", "differs")),
        (dict(nb=0), ("nb",)), (dict(nb=65), ("nb",)),
        (dict(P=0), ("P",)), (dict(P=257), ("P",)), (dict(J=0), ("J",)), (dict(J=33), ("J",)),
        (dict(W=16385), ("width",)), (dict(H=16385, W=1), ("height",)),
        (dict(n_edges=-1), ("n_edges",)), (dict(n_edges=129), ("n_edges",)), (dict(edges=None, n_edges=2), ("edges",)),
        (dict(edges=[(0, 1), (3, 14)]), ("edges[1]", "14")), (dict(edges=[(-1, 1)]), ("edges[0]", "-1")), (dict(edges=[(0, 1), (2, 3)], J=3), ("edges[1]",)),
        (dict(n_people=[1, 5]), ("n_people[1]",)), (dict(n_people=[-1, 0]), ("n_people[0]",)),
        # the redaction's own
        (dict(null_style=True), ("style",)),
        (dict(region=3), ("region",)), (dict(region=-1), ("region",)),
        (dict(effect=2), ("effect",)), (dict(effect=-1), ("effect",)),
        (dict(block=0), ("block",)), (dict(block=1), ("block",)), (dict(block=6), ("block",)), (dict(block=64), ("block",)), (dict(block=-8), ("block",)),
        (dict(head_a=-1), ("head_a", "-1")), (dict(head_a=14), ("head_a", "14")), (dict(head_b=-1), ("head_b",)), (dict(head_b=14), ("head_b", "14")),
        (dict(head_a=5, head_b=5), ("head_a", "head_b")),
        (dict(head_a=12, head_b=13, region=1, J=13), ("head_b",)),  # checked for the body region too
        (dict(head_scale=-0.5), ("head_scale",)), (dict(head_scale=nan), ("head_scale",)), (dict(head_scale=inf), ("head_scale",)),
        (dict(body_scale=-0.5), ("body_scale",)), (dict(body_scale=nan), ("body_scale",)), (dict(body_scale=inf), ("body_scale",)),
        (dict(min_radius=-1.0), ("min_radius",)), (dict(min_radius=nan), ("min_radius",)), (dict(min_radius=1025.0, max_radius=1025.0), ("min_radius",)),
        (dict(max_radius=1024.5), ("max_radius",)), (dict(max_radius=nan), ("max_radius",)), (dict(max_radius=inf), ("max_radius",)),
        (dict(min_radius=8.0, max_radius=7.5), ("min_radius", "max_radius")),
        (dict(min_score=-0.1), ("min_score",)), (dict(min_score=nan), ("min_score",)), (dict(min_score=inf), ("min_score",)),
    ]
    for kw, words in cases:
        rc, msg, red = _raw(pc, **kw)
        assert rc == EINVAL and "redact_people" in msg and all(w in msg for w in words), (kw, rc, msg)
        assert (red == -7).all(), kw  # refused before anything was written
    # good arguments, both formats, every region, effect and block, the limits themselves: there is no CPU path
    good = [dict(), dict(fmt=0), dict(n_edges=0), dict(nb=64, P=256, J=32), dict(n_people=[0, 0]), dict(effect=1),
            dict(min_radius=0.0, max_radius=0.0, head_scale=0.0, body_scale=0.0), dict(min_radius=1024.0, max_radius=1024.0)]
    good += [dict(region=r) for r in (0, 1, 2)] + [dict(block=b) for b in (2, 4, 8, 16, 32)]
    for kw in good:
        rc, msg, _red = _raw(pc, **kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, rc, msg)
    # NULL arguments
    assert pc._lib.dc_redact_people(None, 1, 4, 4, 0, 1, 2, None, None, None, None, None, None) == EINVAL


def test_python_entry_refusals(cpu_mode):
    caffe, _pc = cpu_mode
    import pose

    people = np.ones((2, 14, 3))
    img = np.zeros((20, 30, 3), np.uint8)
    frozen = img.copy()
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="writable"):
        caffe.redact_people(frozen, people, head=(12, 13))
    with pytest.raises(ValueError, match="frames"):
        caffe.redact_people("picture", people, head=(12, 13))
    with pytest.raises(ValueError, match="head"):
        caffe.redact_people(img, people)  # the library knows no skeleton: the pair is the caller's (pose.redact_people has MPII's)
    with pytest.raises(ValueError, match="region"):
        caffe.redact_people(img, people, head=(12, 13), region="face")
    with pytest.raises(ValueError, match="effect"):
        caffe.redact_people(img, people, head=(12, 13), effect="blur")
    with pytest.raises(ValueError, match="one entry per frame"):
        caffe.redact_people(img, np.ones((2, 3, 14, 3)), head=(12, 13))
    with pytest.raises(ValueError, match="ids"):
        caffe.redact_people(img, people, head=(12, 13), ids=[1, 2, 3])
    with pytest.raises(ValueError, match="select"):
        caffe.redact_people(img, people, head=(12, 13), select=[1, 0, 1])
    with pytest.raises(ValueError, match="ids is needed"):
        caffe.redact_people(img, people, head=(12, 13), only_ids=[3])
    for kw, word in ((dict(block=7), "block"), (dict(head=(12, 14)), "head_b"), (dict(head=(3, 3)), "head_a"), (dict(head_scale=-1.0), "head_scale"),
                     (dict(min_radius=9.0, max_radius=8.0), "max_radius"), (dict(edges=[(0, 14)]), "edges[0]")):
        with pytest.raises(caffe.DeepcutError) as ei:
            caffe.redact_people(img, people, **dict(dict(head=(12, 13)), **kw))
        assert ei.value.code == EINVAL and word in str(ei.value), kw
    for call in (lambda: caffe.redact_people(img, people, head=(12, 13), ids=[3, -1], keep_ids=[3]),
                 lambda: caffe.redact_people([caffe.Frame.bgr(img), caffe.Frame.bgr(img.copy())], [people, people[:0]], head=(0, 1), region="body"),
                 lambda: pose.redact_people(img, people, ids=np.array([0, 1]), region="head_or_body", effect="fill", fill=(1, 2, 3))):
        with pytest.raises(caffe.DeepcutError) as ei:
            call()
        assert ei.value.code == ENOCPU
    assert not img.any()
    assert pose.HEAD_MPII14 == (12, 13) and (12, 13) in pose.SKELETON_MPII14
    assert set(caffe.REDACT_DEFAULTS) == {"head_scale", "body_scale", "min_radius", "max_radius"}
    assert 0.0 <= caffe.REDACT_DEFAULTS["min_radius"] <= caffe.REDACT_DEFAULTS["max_radius"] <= 1024.0


def test_only_ids_and_keep_ids_become_select():
    import caffe

    ids = np.array([[4, 9, -1, 4], [7, 7, 2, 0]], np.int64)
    assert caffe.redact_select(ids) is None and caffe.redact_select(None) is None
    assert caffe.redact_select(ids, only_ids=[4, 2]).tolist() == [[1, 0, 0, 1], [0, 0, 1, 0]]
    assert caffe.redact_select(ids, keep_ids=[7, -1]).tolist() == [[1, 1, 0, 1], [0, 0, 1, 1]]
    assert caffe.redact_select(ids, only_ids=[4, 7], keep_ids=[7]).tolist() == [[1, 0, 0, 1], [0, 0, 0, 0]]
    mask = np.array([[0, 5, 1, 1], [1, 0, 1, 1]])
    assert caffe.redact_select(ids, select=mask).tolist() == [[0, 1, 1, 1], [1, 0, 1, 1]]
    got = caffe.redact_select(ids, only_ids=(4, 7), select=mask)
    assert got.dtype == np.uint8 and got.tolist() == [[0, 0, 0, 1], [1, 0, 0, 0]]
    assert caffe.redact_select(ids, only_ids=[]).tolist() == [[0] * 4] * 2 and caffe.redact_select(ids, keep_ids=[]).tolist() == [[1] * 4] * 2
    with pytest.raises(ValueError, match="ids is needed"):
        caffe.redact_select(None, keep_ids=[1])
    with pytest.raises(ValueError, match="select"):
        caffe.redact_select(ids, only_ids=[1], select=np.ones((2, 3)))


# ---- properties of the restatement itself ----------------------------------------------------------------------------------------------
def _people(seed=3, count=4, h=71, w=93):
    rs = np.random.RandomState(seed)
    p = np.zeros((count, 14, 3))
    centre = np.stack([rs.uniform(5, w - 5, count), rs.uniform(5, h - 5, count)], 1)
    p[:, :, :2] = centre[:, None, :] + rs.uniform(-18, 18, (count, 14, 2))
    p[:, :, :2] = np.round(p[:, :, :2] * 32) / 32  # 1/32 px: ties of the 1/16 grid among them
    p[:, :, 2] = rs.uniform(0.2, 1.0, (count, 14))
    p[1, 13] = 0.0  # no head top
    return p


def _bgr(seed=5, h=71, w=93):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _nv12(seed=6, h=71, w=93):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, ((h + 1) // 2, (w + 1) // 2, 2)).astype(np.uint8)


@pytest.mark.parametrize("region", ["head", "body", "head_or_body"])
@pytest.mark.parametrize("block", [2, 8, 32])
def test_restatement_mosaic_is_idempotent_order_free_and_local(region, block):
    people = _people()
    kw = dict(region=region, edges=SKELETON, min_radius=2.0)
    prims, redacted = RR.primitives(people, **kw)
    assert redacted.tolist() == ([1, 0, 1, 1] if region == "head" else [1, 1, 1, 1])
    clean, (y0, uv0) = _bgr(), _nv12()
    img, y, uv = clean.copy(), y0.copy(), uv0.copy()
    blocks = RR.redact_bgr(img, prims, "mosaic", block)
    assert RR.redact_nv12(y, uv, prims, "bt601", "limited", "mosaic", block) == blocks and blocks
    # only bytes of selected blocks differ from the input — luma / BGR pixels and the chroma samples whose pixel (2 cx, 2 cy) is in one
    sel = np.zeros(clean.shape[:2], bool)
    for by, bx in blocks:
        sel[by * block:(by + 1) * block, bx * block:(bx + 1) * block] = True
    assert np.array_equal(img[~sel], clean[~sel]) and np.array_equal(y[~sel], y0[~sel]) and (img[sel] != clean[sel]).any()
    csel = sel[::2, ::2]
    assert csel.shape == uv.shape[:2] and np.array_equal(uv[~csel], uv0[~csel])
    assert (uv[csel] != uv0[csel]).any() == (block > 2)  # B = 2: one chroma sample per block, which is its own mean
    # every selected block is flat
    for by, bx in blocks:
        v = img[by * block:(by + 1) * block, bx * block:(bx + 1) * block].reshape(-1, 3)
        assert (v == v[0]).all()
    # idempotent: the same call on its own output changes no byte
    again, y2, uv2 = img.copy(), y.copy(), uv.copy()
    RR.redact_bgr(again, prims, "mosaic", block)
    RR.redact_nv12(y2, uv2, prims, "bt601", "limited", "mosaic", block)
    assert np.array_equal(again, img) and np.array_equal(y2, y) and np.array_equal(uv2, uv)
    # the order of people does not matter
    perm = [2, 0, 3, 1]
    prims_p, redacted_p = RR.primitives(people[perm], **kw)
    other = clean.copy()
    RR.redact_bgr(other, prims_p, "mosaic", block)
    assert np.array_equal(other, img) and redacted_p.tolist() == redacted[perm].tolist()


def test_restatement_radii_and_selection_rules():
    one = np.zeros((1, 14, 3))
    one[0, 12], one[0, 13] = (40.0, 50.0, 1.0), (40.0, 20.0, 1.0)  # neck, head top: 30 px apart
    (head,), red = RR.primitives(one, head_scale=0.5, min_radius=1.0, max_radius=100.0)
    assert head == dict(a=(640, 560), b=(640, 560), r16=240, capsule=False) and red.tolist() == [1]
    assert RR.primitives(one, head_scale=0.5, min_radius=20.0)[0][0]["r16"] == 320  # min_radius wins
    assert RR.primitives(one, head_scale=0.5, max_radius=10.0, min_radius=1.0)[0][0]["r16"] == 160  # max_radius wins
    none, red0 = RR.primitives(one, head_scale=0.0, min_radius=0.0)  # a radius of 0: no primitive is made
    assert none == [] and red0.tolist() == [0]
    # rint, ties to even: 32 px = 512 units apart, head_scale k / 1024 (exact): 240.5 -> 240, 241.5 -> 242
    tie = one.copy()
    tie[0, 13, 1] = 18.0
    assert RR.primitives(tie, head_scale=481.0 / 1024.0, min_radius=0.0)[0][0]["r16"] == 240
    assert RR.primitives(tie, head_scale=483.0 / 1024.0, min_radius=0.0)[0][0]["r16"] == 242
    # body: the bounding box's larger side is 30 px = 480 units; the cap of 64 px wins over min_radius
    body, _ = RR.primitives(one, region="body", edges=((12, 13),), body_scale=0.1, min_radius=1.0)
    assert [(p["capsule"], p["r16"]) for p in body] == [(False, 360), (True, 48), (False, 48), (False, 48)]
    assert RR.primitives(one, region="body", body_scale=10.0, min_radius=100.0, max_radius=200.0)[0][1]["r16"] == 1024
    # a single held joint: s16 = 0, the radius is min_radius; no head disc, and "head" makes nothing of the person
    lone = np.zeros((1, 14, 3))
    lone[0, 4] = (10.0, 10.0, 0.9)
    made, red1 = RR.primitives(lone, region="head_or_body", min_radius=3.0)
    assert made == [dict(a=(160, 160), b=(160, 160), r16=48, capsule=False)] and red1.tolist() == [1]
    assert RR.primitives(lone, region="head")[1].tolist() == [0]
    # select and n_people
    two = np.concatenate([one, one + (30.0, 0.0, 0.0)])
    assert RR.primitives(two, select=[0, 1])[1].tolist() == [0, 1] and RR.primitives(two, n_people=1)[1].tolist() == [1, 0]
    # the negative midpoint floors (arithmetic shift)
    neg = np.zeros((1, 14, 3))
    neg[0, 12], neg[0, 13] = (-1.0, -1.0, 1.0), (-1.0625, -1.1875, 1.0)
    assert RR.primitives(neg)[0][0]["a"] == ((-16 - 17) >> 1, (-16 - 19) >> 1) == (-17, -18)
    # FILL through the forward colour rule
    assert RR.forward_colour((255, 255, 255), "bt601", "limited") == (235, 128, 128) and RR.forward_colour((0, 0, 0), "bt709", "full") == (0, 128, 128)


# ---- redact= of the pipeline and of track_people on a fake net -------------------------------------------------------------------------
def test_redact_none_never_touches_the_redact_entry(monkeypatch):
    """With the entry REMOVED from every module that offers it, the default runs as before: no attribute access, no call."""
    import caffe
    import caffe.pycaffe as pc
    import pose
    import pose.people as pp
    from deepcut_tools import VideoPipeline

    for mod in (caffe, pc, pose, pp):
        monkeypatch.delattr(mod, "redact_people")
    monkeypatch.delattr(pp, "_redact_style")
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, batch=2, stats=STATS, choose_streams=False)
    for k in range(5):
        pipe.submit(_frame(k), tag=k)
    assert [t for t, _, _ in pipe.drain()] == list(range(5))
    net = FakeNet()
    out = list(pose.track_people([_frame(k) for k in range(3)], None, None, STATS, tracker="tracker", depth=1, batch=2, net=net))
    assert [int(p[0, 0, 0]) for p, _ in out] == [0, 1, 2] and all("redact" not in c["kw"] for c in net.world["calls"])


def test_redact_runs_before_draw_on_the_frame_of_the_request(monkeypatch):
    import pose.people as pp
    from deepcut_tools import VideoPipeline

    log = []
    monkeypatch.setattr(pp, "redact_people", lambda frame, people, ids=None, **style: log.append(("redact", frame, people, ids, style)))
    monkeypatch.setattr(pp, "draw_people", lambda frame, people, ids=None, **style: log.append(("draw", frame, people, ids, style)))
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, batch=2, stats=STATS, choose_streams=False, redact=dict(block=16), draw=dict(alpha=96))
    frames = [_frame(k) for k in range(5)]
    for k, f in enumerate(frames):
        pipe.submit(f, tag=k)
    assert all("redact" not in c["kw"] and "draw" not in c["kw"] for c in net.world["calls"])  # the styles stay with the pipeline
    out = pipe.drain()
    assert [e[0] for e in log] == ["redact", "draw"] * 5
    for k, (tag, people, ids) in enumerate(out):
        r, d = log[2 * k], log[2 * k + 1]
        assert r[1] is frames[k] and d[1] is frames[k] and r[2] is people and r[3] is ids and r[4] == dict(block=16) and d[4] == dict(alpha=96, cand=None)
    # redact alone keeps the frames too; anything but None / True / a dict is refused
    log[:] = []
    pipe = VideoPipeline(FakeNet(), "tracker", stats=STATS, choose_streams=False, redact=True)
    pipe.submit(frames[0])
    pipe.drain()
    assert [(e[0], e[4]) for e in log] == [("redact", {})] and log[0][1] is frames[0]
    with pytest.raises(ValueError, match="redact"):
        VideoPipeline(FakeNet(), "tracker", stats=STATS, redact="yes")
    # track_people hands the style on, (people, ids) are what they are without it
    log[:] = []
    plain = list(pp.track_people([_frame(k) for k in range(3)], None, None, STATS, tracker="tracker", depth=1, batch=2, net=FakeNet()))
    frames = [_frame(k) for k in range(3)]
    with_it = list(pp.track_people(frames, None, None, STATS, tracker="tracker", depth=1, batch=2, net=FakeNet(), redact=dict(region="body"), draw=True))
    assert [e[0] for e in log] == ["redact", "draw"] * 3 and all(e[1] is frames[i // 2] for i, e in enumerate(log))
    assert all(e[4] == dict(region="body") for e in log[::2])
    for (p0, i0), (p1, i1) in zip(plain, with_it):
        assert np.array_equal(p0, p1) and np.array_equal(i0, i1)
