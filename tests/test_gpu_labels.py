"""GPU: `caffe.label_people` (dc_label_people) against the numpy restatement of its rule in tests/label_ref.py, BYTE FOR BYTE, the pitch
padding (pre-filled with a sentinel) included — the rule is integer only, so there is no tolerance.

PARITY UNPINNED BY THE REFERENCE: its demo draws with matplotlib and labels nothing; the rule is this project's own.

Shapes: 70 x 101 (3 x 4 tiles of 32 x 32, the last ones partial; an odd width: chroma blocks of one column) and 33 x 35 (odd both ways,
one pixel row and three pixel columns in the last tiles)."""
import numpy as np
import pytest

import label_ref as LR
from test_gpu_draw import _same, _surface

pytestmark = pytest.mark.gpu

PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48))
CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ #-.:/%+_?"
FORMATS = [("bgr", None), ("nv12", ("bt601", "limited")), ("nv12", ("bt709", "full"))]


def _surf(fmt, h, w, seed=3):
    return _surface(fmt[0], h, w, seed, fmt[1] or ("bt601", "limited"))


def _reference(surfaces, people, n_people=None, ids=None, texts=None, **style):
    want = [s.copy() for s in surfaces]
    for b, s in enumerate(want):
        labs = LR.labels(people[b], s.h, s.w, None if n_people is None else n_people[b], None if ids is None else ids[b],
                         None if texts is None else texts[b], **style)
        if len(s.bufs) == 1:
            LR.label_bgr(s.views()[0], labs)
        else:
            LR.label_nv12(*s.views(), labs, s.matrix, s.range)
    return want


def _on_host(caffe, surfaces, people, **kw):
    got = [s.copy() for s in surfaces]
    caffe.label_people([s.host_frame(caffe) for s in got], people, **kw)
    return got


def _on_device(caffe, surfaces, people, **kw):
    import torch

    tensors = [[torch.from_numpy(b).cuda() for b in s.bufs] for s in surfaces]
    torch.cuda.synchronize()
    caffe.label_people([s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)], people, **kw)
    got = [s.copy() for s in surfaces]
    for g, t in zip(got, tensors):
        g.bufs = [x.cpu().numpy() for x in t]
    return got


def _check(caffe, surfaces, people, where=("host", "device"), **kw):
    """Host and device frames against the restatement; -> the restatement's surfaces."""
    kw.setdefault("palette", PALETTE)
    want = _reference(surfaces, people, **kw)
    for place in where:
        got = (_on_host if place == "host" else _on_device)(caffe, surfaces, people, **kw)
        for b, (g, w_) in enumerate(zip(got, want)):
            for k, (x, y) in enumerate(zip(g.bufs, w_.bufs)):
                bad = np.argwhere(x != y)
                assert bad.size == 0, "%s frame %d plane %d: %d bytes differ, first at %s: got %d, want %d" % (
                    place, b, k, len(bad), tuple(bad[0]), x[tuple(bad[0])], y[tuple(bad[0])])
    return want


def _people(spots, J=3):
    """One person per (x, y): joint 0 there, joint 1 a little down and right, joint 2 not held."""
    p = np.zeros((1, len(spots), J, 3))
    for k, (x, y) in enumerate(spots):
        p[0, k, 0] = (x, y, 0.9)
        p[0, k, 1] = (x + 6.3, y + 9.6, 0.8)
        p[0, k, 2] = (np.nan, 1.0, 0.9)
    return p


# seams of the 32-pixel tiles in x and in y, the four clamps, a person without a held joint (index 6), the middle
SPOTS = [(30.4, 45.5), (60.2, 33.0), (-20.0, 50.0), (50.0, 3.0), (200.0, 50.0), (50.0, 400.0), (40.0, 40.0), (12.7, 64.2)]


def _scene(h, w):
    ppl = _people(SPOTS)
    ppl[0, 6, :, 2] = 0.0  # no held joint: no label
    ids = np.array([[3, 17, 0, 1234, 5, -1, 8, 2 ** 40 + 7]], np.int64)
    return ppl, ids


@pytest.mark.parametrize("fmt", FORMATS, ids=["bgr", "nv12-601l", "nv12-709f"])
@pytest.mark.parametrize("size", [(70, 101), (33, 35)], ids=["70x101", "33x35"])
def test_labels_equal_the_restatement(gpu_caffe, fmt, size):
    h, w = size
    ppl, ids = _scene(h, w)
    surfaces = [_surf(fmt, h, w)]
    base = _check(gpu_caffe, surfaces, ppl, ids=ids, prefix="#")
    assert not _same(base, surfaces)  # something was written
    for scale in (1, 3, 8):  # at 8 in 33 x 35 every label is larger than the frame: X = Y = 0, cut right and below
        _check(gpu_caffe, surfaces, ppl, ids=ids, scale=scale, gap=scale, where=("device",))
    _check(gpu_caffe, surfaces, ppl, ids=ids, anchor=0, where=("device",))  # held: centred on the joint
    _check(gpu_caffe, surfaces, ppl, ids=ids, anchor=2, gap=0, where=("device",))  # not held: the box's corner
    for kw in (dict(alpha_plate=256), dict(alpha_plate=128, alpha_text=128), dict(alpha_plate=0), dict(alpha_text=0, alpha_plate=77),
               dict(color="text", plate_color=(10, 200, 30), alpha_plate=200), dict(color="plate", text_color=(0, 0, 0), min_score=0.85)):
        _check(gpu_caffe, surfaces, ppl, ids=ids, where=("device",), **kw)
    _check(gpu_caffe, surfaces, ppl, where=("device",))  # ids NULL: the person's index
    _check(gpu_caffe, surfaces, ppl, n_people=[3], ids=ids, where=("host",))


@pytest.mark.parametrize("fmt", FORMATS[:2], ids=["bgr", "nv12"])
def test_nothing_to_label_writes_nothing(gpu_caffe, fmt):
    ppl, ids = _scene(70, 101)
    surfaces = [_surf(fmt, 70, 101, seed=4), _surf(fmt, 70, 101, seed=5)]
    two = np.concatenate([ppl, ppl])
    for kw in (dict(n_people=[0, 0]), dict(alpha_text=0, alpha_plate=0), dict(ids=np.full((2, 8), -1, np.int64)), dict(min_score=2.0)):
        assert _same(_check(gpu_caffe, surfaces, two, **kw), surfaces)
    # a frame nothing is labelled in stays as it is beside one that is written
    want = _check(gpu_caffe, surfaces, two, n_people=[0, 8], ids=np.concatenate([ids, ids]))
    assert _same(want[:1], surfaces[:1]) and not _same(want[1:], surfaces[1:])


@pytest.mark.parametrize("fmt", FORMATS[:2], ids=["bgr", "nv12"])
def test_texts_use_every_glyph_and_the_longest_key(gpu_caffe, fmt):
    h, w = 70, 101
    rows = [CHARS[0:12], CHARS[12:24], CHARS[24:36].lower(), CHARS[36:46], "", None]
    ppl = _people([(3.0, 12.0 + 11.0 * k) for k in range(6)])
    ids = np.array([[1, 2, 3, -1, 2 ** 63 - 1, 6]], np.int64)  # a text of its own labels an untracked person; "" and None: the made text
    labs = LR.labels(ppl[0], h, w, ids=ids[0], texts=rows, scale=1, prefix="ID:#")
    assert [v["text"] for v in labs] == [CHARS[0:12], CHARS[12:24], CHARS[24:36], CHARS[36:46], "ID:#9223372036854775807", "ID:#6"]
    assert set("".join(v["text"] for v in labs)) == set(CHARS)
    _check(gpu_caffe, [_surf(fmt, h, w)], ppl, ids=ids, texts=[rows], scale=1, gap=0, prefix="ID:#")
    _check(gpu_caffe, [_surf(fmt, h, w)], ppl, ids=ids, texts=[rows], scale=2, gap=1, alpha_plate=100, color="text", where=("device",))


@pytest.mark.parametrize("fmt", FORMATS[:2], ids=["bgr", "nv12"])
def test_overlapping_labels_keep_their_order(gpu_caffe, fmt):
    h, w = 33, 35
    ppl = _people([(8.0, 28.0), (11.0, 31.0)])
    surfaces = [_surf(fmt, h, w)]
    kw = dict(ids=np.array([[1, 2]], np.int64), alpha_plate=128, alpha_text=200, gap=0)
    ab = _check(gpu_caffe, surfaces, ppl, **kw)
    ba = _check(gpu_caffe, surfaces, ppl[:, ::-1].copy(), where=("device",), **dict(kw, ids=np.array([[2, 1]], np.int64)))
    assert not _same(ab, ba)  # the order is visible


@pytest.mark.parametrize("fmt", FORMATS[:2], ids=["bgr", "nv12"])
def test_256_labels_on_one_tile_take_the_walk_past_its_first_trip(gpu_caffe, fmt):
    h, w = 70, 101
    rs = np.random.RandomState(11)
    # every plate (19 x 9 at scale 1 with three characters) holds pixel (40, 40) of tile (1, 1); half of them reach tile (0, 1) too
    spots = [(24.0 + rs.randint(0, 16), 42.0 + rs.randint(0, 8)) for _ in range(256)]
    ppl = _people(spots)
    ids = (100 + np.arange(256, dtype=np.int64))[None]
    labs = LR.labels(ppl[0], h, w, ids=ids[0], scale=1, gap=0)
    assert len(labs) == 256 and all(v["X"] <= 40 < v["X"] + v["pw"] and v["Y"] <= 40 < v["Y"] + v["ph"] for v in labs)
    _check(gpu_caffe, [_surf(fmt, h, w)], ppl, ids=ids, scale=1, gap=0, alpha_plate=90, alpha_text=180)
