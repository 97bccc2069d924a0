"""CPU: the host side of the appearance descriptor and of the tracker's appearance steps (include/deepcut_hip.h, dc_describe_people and
dc_tracker_update_appearance) — the symbols and structs, every refusal without a device (each DC_EINVAL naming the field, before
DC_ENOCPU), the Python refusals, properties of the numpy restatement itself (tests/appear_ref.py) and scripted sequences on it.

PARITY UNPINNED BY THE REFERENCE, which stops at the maps; both rules are this project's own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import appear_ref as AR
import track_ref as TR

EINVAL, ENOCPU = -1, -6  # include/deepcut_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORSO = ((8, 2), (9, 3), (8, 9), (2, 3))
NEW = ("dc_describe_people", "dc_tracker_set_appearance", "dc_tracker_get_appearance", "dc_tracker_update_appearance",
       "dc_tracker_appearance_state")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepcut_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    import caffe
    import caffe.pycaffe as pc

    text, lib = _header(), C.CDLL(caffe.lib_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in pc.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+DC_APPEARANCE_BINS\s+16\b", text) and re.search(r"#define\s+DC_TRACK_GALLERY\s+64\b", text)
    assert caffe.APPEARANCE_BINS == 16 and caffe.TRACK_GALLERY == 64
    # the ctypes structs have the header's fields in the header's order
    for struct, cls in (("dc_appearance_style", pc.AppearanceStyle), ("dc_track_appearance_params", pc.TrackAppearanceParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        names = [n for n in re.findall(r"[A-Za-z_]\w*", body) if n not in ("int", "double", "const", "size_t")]
        assert names == [f[0] for f in cls._fields_], names
    import pose

    assert pose.TORSO_MPII14 == TORSO
    assert set(caffe.APPEARANCE_DEFAULTS) == {"scale", "min_radius", "min_score", "min_pixels", "alpha256", "reid_max", "max_age", "min_hits"}


# ---- the entries' refusals, without a device -------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_mode():
    import caffe
    import caffe.pycaffe as pc

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    yield caffe, pc
    pc._lib.dc_set_mode(mode)


def _raw(pc, H=20, W=30, fmt=1, nb=2, P=4, J=14, frames=None, n_people=None, null_style=False, **style):
    """dc_describe_people through ctypes with good arguments except what the caller overrides -> (rc, message, desc)."""
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
    st = pc.AppearanceStyle()
    st.size, st.scale, st.min_radius, st.min_score = C.sizeof(pc.AppearanceStyle), 0.04, 2.0, 0.0
    st.n_edges, st.edges = style.pop("n_edges", edges.shape[0]), None if given is None else edges.ctypes.data
    for k, v in style.items():
        setattr(st, k, v)
    desc = np.full((max(nb, 1), max(P, 1), 3, 16), -7, np.int32)
    rc = pc._lib.dc_describe_people(arr, nb, H, W, 0, P, J, n.ctypes.data_as(C.c_void_p), people.ctypes.data_as(C.c_void_p),
                                    None if null_style else C.byref(st), desc.ctypes.data_as(C.c_void_p), None)
    return rc, (pc._lib.dc_last_error() or b"").decode(), desc


def test_every_argument_error_of_describe_people_is_einval_naming_the_field_before_enocpu(cpu_mode):
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
        # what dc_redact_people refuses of frames, nb, height, width, P, J, n_people and edges
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
        # the descriptor's own
        (dict(null_style=True), ("style",)),
        (dict(size=0), ("size",)), (dict(size=C.sizeof(pc.AppearanceStyle) - 1), ("size",)),
        (dict(scale=-0.5), ("scale",)), (dict(scale=nan), ("scale",)), (dict(scale=inf), ("scale",)),
        (dict(min_radius=-1.0), ("min_radius",)), (dict(min_radius=nan), ("min_radius",)), (dict(min_radius=64.5), ("min_radius",)),
        (dict(min_score=-0.1), ("min_score",)), (dict(min_score=nan), ("min_score",)), (dict(min_score=inf), ("min_score",)),
    ]
    for kw, words in cases:
        rc, msg, desc = _raw(pc, **kw)
        assert rc == EINVAL, (kw, rc, msg)
        assert msg.startswith("describe_people: ") and all(w in msg for w in words), (kw, msg)
        assert (desc == -7).all(), kw  # nothing was written
    # good arguments — the limits included — reach the mode check: there is no CPU path
    for kw in (dict(), dict(fmt=0), dict(edges=None, n_edges=0), dict(scale=0.0, min_radius=0.0), dict(min_radius=64.0), dict(nb=64, n_people=[0] * 64),
               dict(size=C.sizeof(pc.AppearanceStyle) + 64)):
        rc, msg, _ = _raw(pc, **kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, rc, msg)


def test_tracker_appearance_parameters_set_get_and_refusals_without_a_device(cpu_mode):
    caffe, pc = cpu_mode
    t = caffe.Tracker(n_joints=3, max_tracks=4)
    assert t.appearance is None
    t.appearance = True
    assert t.appearance == {k: caffe.APPEARANCE_DEFAULTS[k] for k in ("min_pixels", "alpha256", "reid_max", "max_age", "min_hits")}
    t.appearance = dict(min_pixels=1, alpha256=0, reid_max=0, max_age=0, min_hits=1)  # the lower limits
    t.appearance = dict(alpha256=256, reid_max=12288, max_age=100000)  # the upper ones
    assert t.appearance["alpha256"] == 256 and t.appearance["min_pixels"] == caffe.APPEARANCE_DEFAULTS["min_pixels"]
    for bad, word in ((dict(min_pixels=0), "min_pixels"), (dict(alpha256=-1), "alpha256"), (dict(alpha256=257), "alpha256"),
                      (dict(reid_max=-1), "reid_max"), (dict(reid_max=12289), "reid_max"), (dict(max_age=-1), "max_age"),
                      (dict(max_age=100001), "max_age"), (dict(min_hits=0), "min_hits")):
        with pytest.raises(caffe.DeepcutError) as e:
            t.appearance = bad
        assert e.value.code == EINVAL and word in str(e.value), (bad, str(e.value))
        assert t.appearance["alpha256"] == 256  # a refused value changes nothing
    q = pc.TrackAppearanceParams(2, 1, 1, 1, 1, 1)
    assert pc._lib.dc_tracker_set_appearance(t._h, C.byref(q)) == EINVAL and b"enabled" in pc._lib.dc_last_error()
    with pytest.raises(ValueError, match="bogus"):
        t.appearance = dict(bogus=1)
    with pytest.raises(ValueError, match="bogus"):
        caffe.Tracker(n_joints=3, appearance=dict(bogus=1))
    with pytest.raises(TypeError):
        t.appearance = 3
    # the state before any update: nothing valid, an empty gallery — with appearance on and off
    for _ in range(2):
        st = t.appearance_state(0)
        assert not st["track_valid"].any() and not st["track_model"].any() and (st["gallery_ids"] == -1).all() and (st["gallery_age"] == -1).all()
        assert st["track_model"].shape == (4, 3, 16) and st["gallery_model"].shape == (64, 3, 16)
        t.appearance = None
    assert t.appearance is None
    # the update entry: its refusals come before DC_ENOCPU, appearance off among them
    people, desc = np.ones((1, 2, 3, 3)), np.ones((1, 2, 3, 16), np.int32)
    with pytest.raises(caffe.DeepcutError) as e:
        t.update(people, desc=desc)
    assert e.value.code == EINVAL and "appearance is off" in str(e.value)
    t.appearance = True
    with pytest.raises(caffe.DeepcutError) as e:
        t.update(people, desc=desc, return_smooth=True)
    assert e.value.code == EINVAL and "smoothing is off" in str(e.value)
    with pytest.raises(caffe.DeepcutError) as e:
        t.update(people, n_people=[3], desc=desc)
    assert e.value.code == EINVAL and "n_people[0]" in str(e.value)
    with pytest.raises(ValueError, match="desc must be"):
        t.update(people, desc=desc[:, :1])
    with pytest.raises(caffe.DeepcutError) as e:
        t.update(people, desc=desc, return_reid=True)
    assert e.value.code == ENOCPU
    with pytest.raises(caffe.DeepcutError) as e:
        t.appearance_state(1)
    assert e.value.code == EINVAL and "slot" in str(e.value)


def test_track_people_refuses_appearance_off_the_synchronous_route_and_unknown_keys():
    import pose

    frames = [np.zeros((16, 16, 3), np.uint8)]
    for kw in (dict(depth=2), dict(batch=2), dict(in_chain=True, draw=True)):
        with pytest.raises(ValueError, match="appearance"):
            next(pose.track_people(frames, "no.prototxt", "no.caffemodel", None, appearance=True, **kw))
    with pytest.raises(ValueError, match="bogus"):
        next(pose.track_people(frames, "no.prototxt", "no.caffemodel", None, appearance=dict(bogus=1)))
    with pytest.raises(TypeError):
        next(pose.track_people(frames, "no.prototxt", "no.caffemodel", None, appearance=3))


# ---- properties of the descriptor's restatement ----------------------------------------------------------------------------------------
STYLE = dict(edges=TORSO, scale=0.1, min_radius=1.5, min_score=0.1)


def _torso(cx, cy, half_w=6.0, half_h=8.0):
    p = np.zeros((14, 3))
    p[8], p[9] = (cx - half_w, cy - half_h, 0.9), (cx + half_w, cy - half_h, 0.9)
    p[2], p[3] = (cx - half_w + 1.5, cy + half_h, 0.9), (cx + half_w - 1.25, cy + half_h, 0.9)
    return p


def _image(seed=5, h=48, w=64):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_restatement_channels_sum_to_the_region_and_a_pixel_counts_once_per_person():
    img = _image()
    people = np.stack([_torso(20.0, 20.5), _torso(40.25, 24.0), _torso(200.0, 20.0)])
    desc = AR.describe_bgr(img, people, **STYLE)
    for p in range(3):
        caps = AR.capsules(people[p], **STYLE)
        n = int(AR.region(48, 64, caps).sum())
        assert desc[p].sum(axis=1).tolist() == [n] * 3
        # the capsules of one person overlap at the corners of the torso: the pixels under two of them count once
        if n:
            assert sum(int(AR.region(48, 64, [c]).sum()) for c in caps) > n
    assert desc[0].any() and desc[1].any() and not desc[2].any()
    # a radius of 0 makes no primitive; no held limb: zeros
    assert not AR.describe_bgr(img, people[:1], **dict(STYLE, scale=0.0, min_radius=0.0)).any()
    assert not AR.describe_bgr(img, people[:1], **dict(STYLE, min_score=0.95)).any()


def test_restatement_does_not_depend_on_the_order_of_people_and_reads_nv12_chroma_at_half_resolution():
    img = _image()
    people = np.stack([_torso(20.0, 20.5), _torso(26.0, 24.0), _torso(40.25, 24.0)])
    desc = AR.describe_bgr(img, people, **STYLE)
    order = [2, 0, 1]
    assert np.array_equal(AR.describe_bgr(img, people[order], **STYLE), desc[order])
    y, uv = img[:, :, 0].copy(), img[:24, :32, 1:].copy()
    d = AR.describe_nv12(y, uv, people, **STYLE)
    assert np.array_equal(d[:, 0], AR.describe_bgr(np.repeat(y[:, :, None], 3, 2), people, **STYLE)[:, 0])
    full = np.repeat(np.repeat(uv, 2, 0), 2, 1)  # every pixel's chroma sample
    assert np.array_equal(d[:, 1:], AR.describe_bgr(np.concatenate([y[:, :, None], full], 2), people, **STYLE)[:, 1:])


def test_a_descriptor_is_close_to_itself_and_far_from_another_colour():
    rs = np.random.RandomState(2)
    for _ in range(50):
        n = int(rs.randint(1, 4000))
        h = np.stack([np.bincount(rs.randint(0, 16, n), minlength=16) for _ in range(3)])
        q = AR.quantise(h, 1)
        assert all(abs(sum(q[16 * c:16 * c + 16]) - 4096) <= 8 for c in range(3))
        assert -24 <= AR.dissimilarity(q, q) <= 24
        assert AR.blend(q, q, 77) == q
    red, blue = np.zeros((3, 16), int), np.zeros((3, 16), int)
    red[:, 2], blue[:, 13] = 100, 100
    assert AR.dissimilarity(AR.quantise(red, 1), AR.quantise(blue, 1)) == 12288
    assert AR.quantise(red, 101) is None and AR.quantise(np.zeros((3, 16), int), 1) is None
    assert AR.blend([0, 4096], [4096, 0], 256) == [4096, 0] and AR.blend([0, 4096], [4096, 0], 0) == [0, 4096]
    assert AR.blend([10], [0], 64) == [10 + ((-10 * 64 + 128) >> 8)] == [8]  # the shift is arithmetic: floor, not truncation


# ---- scripted sequences on the tracker's restatement -----------------------------------------------------------------------------------
J = 3
PRM = TR.params(J, max_misses=2, min_common=1, max_dist=0.5, min_size=16.0, motion=0)
AP = AR.appearance_params(min_pixels=10, alpha256=64, reid_max=3000, max_age=12, min_hits=2)


def _pose(x, y):
    return np.array([[x, y, 0.9], [x + 8.0, y, 0.9], [x + 4.0, y + 16.0, 0.9]])


def _colour(bin_, n=200):
    h = np.zeros((3, 16), np.int32)
    h[:, bin_], h[:, (bin_ + 1) % 16] = n - n // 4, n // 4
    return h


def _run(frames, ap=AP, with_desc=True, T=4, P=4):
    """frames: per frame a list of (x, y, colour bin) -> per frame (ids [m], reid [m]); the slot and the appearance state."""
    slot, app, out = TR.Slot(T, J), AR.Appearance(T), []
    for people in frames:
        ppl, desc = np.zeros((P, J, 3)), np.zeros((P, 3, 16), np.int32)
        for k, (x, y, c) in enumerate(people):
            ppl[k], desc[k] = _pose(x, y), _colour(c)
        ids, _place, reid, _D = AR.update(slot, app, ppl, len(people), P, PRM, ap, desc if with_desc else None)
        out.append((ids[:len(people)].tolist(), reid[:len(people)].tolist()))
    return out, slot, app


def test_a_person_who_leaves_and_comes_back_elsewhere_takes_the_old_id():
    away = PRM["max_misses"] + 3
    frames = [[(10.0, 10.0, 2), (100.0, 10.0, 9)]] * 3 + [[(100.0, 10.0, 9)]] * away + [[(100.0, 10.0, 9), (60.0, 90.0, 2)]] * 2
    out, slot, app = _run(frames)
    assert out[0] == ([0, 1], [0, 0]) and out[2] == ([0, 1], [0, 0])
    assert out[3 + away] == ([1, 0], [0, 1])  # the old id, far from where the track was lost
    assert out[-1] == ([1, 0], [0, 0]) and slot.next_id == 2 and all(e is None for e in app.gallery)
    # the plain tracker gives a new id, and so does appearance on without descriptors
    slot2 = TR.Slot(4, J)
    plain = []
    for people in frames:
        ppl = np.zeros((4, J, 3))
        for k, (x, y, _c) in enumerate(people):
            ppl[k] = _pose(x, y)
        plain.append(TR.update(slot2, ppl, len(people), 4, PRM)[0][:len(people)].tolist())
    assert plain[3 + away] == [1, 2]
    blind, slot3, _ = _run(frames, with_desc=False)
    assert [ids for ids, _ in blind] == plain and not any(any(r) for _, r in blind) and slot3.next_id == slot2.next_id


def test_a_differently_coloured_person_does_not_take_the_id_and_an_old_entry_is_gone():
    away = PRM["max_misses"] + 3
    frames = [[(10.0, 10.0, 2)]] * 3 + [[]] * away + [[(60.0, 90.0, 11)]]
    out, _slot, app = _run(frames)
    assert out[-1] == ([1], [0]) and [e[0] for e in app.gallery if e is not None] == [0]  # id 0 still waits
    # the same colour, but later than max_age: the entry is gone (freed at misses = 3, i.e. in the third empty frame; it ages from then on)
    for extra, want in ((AP["max_age"] - 1, ([0], [1])), (AP["max_age"], ([1], [0]))):
        frames = [[(10.0, 10.0, 2)]] * 3 + [[]] * (PRM["max_misses"] + 1 + extra) + [[(60.0, 90.0, 2)]]
        out, _slot, app = _run(frames)
        assert out[-1] == want, (extra, out[-1])
        assert all(e is None for e in app.gallery)
    # a track with fewer than min_hits hits does not enter the gallery
    frames = [[(10.0, 10.0, 2)]] + [[]] * away + [[(60.0, 90.0, 2)]]
    assert _run(frames)[0][-1] == ([1], [0])
    # too few pixels: not valid, so nothing to re-identify with
    frames = [[(10.0, 10.0, 2)]] * 3 + [[]] * away + [[(60.0, 90.0, 2)]]
    assert _run(frames, ap=dict(AP, min_pixels=201))[0][-1] == ([1], [0])


def test_the_gallery_replaces_its_oldest_entry_when_it_is_full():
    T = P = 128
    slot, app = TR.Slot(T, J), AR.Appearance(T)
    ap = dict(AP, min_hits=1)

    def crowd(first, count, halves=False):
        """halves: two bins five apart, half the pixels each — at least 3072 away from every `_colour`, so beyond reid_max"""
        ppl, desc = np.zeros((P, J, 3)), np.zeros((P, 3, 16), np.int32)
        for k in range(count):
            ppl[k], desc[k] = _pose(64.0 * ((first + k) % 16), 64.0 * ((first + k) // 16)), _colour((first + k) % 16, 100 + first + k)
            if halves:
                desc[k] = 0
                desc[k][:, (first + k) % 16], desc[k][:, (first + k + 5) % 16] = 50, 50
        return ppl, desc

    ppl, desc = crowd(0, 30)
    AR.update(slot, app, ppl, 30, P, PRM, ap, desc)
    for _ in range(PRM["max_misses"] + 1):
        AR.update(slot, app, np.zeros((P, J, 3)), 0, P, PRM, ap, None)
    assert sorted(e[0] for e in app.gallery if e is not None) == list(range(30))
    ppl, desc = crowd(30, 70, halves=True)
    ids, _place, reid, _D = AR.update(slot, app, ppl, 70, P, PRM, ap, desc)
    assert ids[:70].tolist() == list(range(30, 100)) and not reid.any()
    for _ in range(PRM["max_misses"] + 1):
        AR.update(slot, app, np.zeros((P, J, 3)), 0, P, PRM, ap, None)
    got = [e[0] for e in app.gallery]
    # 70 freed at once into 34 free entries; the other 36 replace the oldest: the 30 first (entries 0 .. 29, ascending), then — every
    # entry has age 0 now — entry 0 again and again
    assert got[30:] == list(range(30, 64)) and got[1:30] == list(range(65, 94)) and got[0] == 99
