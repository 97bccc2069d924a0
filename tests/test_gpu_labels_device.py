"""GPU: `caffe.overlay_people_device(..., labels=)` (dc_overlay_people_device_styles) — the labels made on the device from people that
torch uploaded.  Every comparison is BYTE FOR BYTE, whole buffers (pitch padding and a guard row behind each plane included): against
the numpy restatements (tests/redact_ref.py, tests/draw_ref.py, tests/label_ref.py, in that order) AND against the synchronous
`caffe.redact_people`, `caffe.draw_people`, `caffe.label_people` on a copy of the frame.

PARITY UNPINNED BY THE REFERENCE, which draws with matplotlib on the host and labels nothing; the rules are this project's own.

Shapes: the 67 x 101 frames of tests/test_gpu_overlay_device.py, nb = 3 with frame 1 holding nobody."""
import numpy as np
import pytest

import label_ref as LR
from test_gpu_overlay_device import FORMATS, GEOMETRY, SEVEN, SKELETON, _assert_same, _download, _restated, _same, _surfaces, _upload

pytestmark = pytest.mark.gpu

LABELS = dict(scale=1, gap=1, anchor=13, prefix="P", alpha_text=230, alpha_plate=140, palette=SEVEN)


def _crowd(people=5, seed=5, h=67, w=101):
    rs = np.random.RandomState(seed)
    p = np.zeros((3, people, 14, 3))
    p[..., 0] = np.round(rs.uniform(-10, w + 10, (3, people, 14)) * 16) / 16
    p[..., 1] = np.round(rs.uniform(-10, h + 10, (3, people, 14)) * 16) / 16
    p[..., 2] = rs.uniform(0.2, 1.0, (3, people, 14))
    p[0, 1, 13, 2] = 0.0  # the anchor not held: the box's corner
    p[2, 0, :, 0] = np.nan  # nobody to label
    ids = rs.permutation(3 * people * 40)[:3 * people].reshape(3, people).astype(np.int64)
    ids[0, 2] = -1
    ids[2, 3] = 2 ** 63 - 1
    return p, ids


def _with_labels(want, people, n, ids, labels):
    for b, s in enumerate(want):
        labs = LR.labels(people[b], s.h, s.w, int(n[b]), None if ids is None else ids[b], **labels)
        v = s.views()
        if s.fmt == "bgr":
            LR.label_bgr(v[0], labs)
        else:
            LR.label_nv12(v[0], v[1], labs, s.matrix, s.range)
    return want


def _overlay(caffe, surfaces, people, n, cand, ids, draw, redact, labels, where="device", stream=None):
    import torch

    dev = lambda a, t: None if a is None else torch.from_numpy(np.array(a, t)).cuda()  # noqa: E731
    t_people, t_n, t_cand, t_ids = dev(people, np.float64), dev(n, np.int32), dev(cand, np.int32), dev(ids, np.int64)
    t_red = None if redact is None else torch.full(people.shape[:2], -7, dtype=torch.int32, device="cuda")
    if where == "device":
        tensors = _upload(surfaces)
        frames = [s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)]
    else:
        got = [s.copy() for s in surfaces]
        frames = [s.host_frame(caffe) for s in got]
    torch.cuda.synchronize()
    caffe.overlay_people_device(frames, t_people, t_n, cand=t_cand, ids=t_ids, draw=draw, redact=redact, redacted=t_red, labels=labels,
                                stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    if where == "device":
        got = _download(surfaces, tensors)
    return got, None if t_red is None else t_red.cpu().numpy()


def _check(caffe, surfaces, people, n=None, cand=None, ids=None, draw=None, redact=None, labels=None, where=("device", "host")):
    import torch

    n = np.full(people.shape[0], people.shape[1], np.int32) if n is None else np.asarray(n, np.int32)
    clamped = np.clip(n, 0, people.shape[1])
    want, red = _restated(surfaces, people, clamped, cand, ids, draw, redact)
    want = _with_labels(want, people, clamped, ids, labels)
    # the three synchronous entries in the rule's order, on one device copy
    tensors = _upload(surfaces)
    torch.cuda.synchronize()
    frames = [s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)]
    if redact is not None:
        caffe.redact_people(frames, people, n_people=clamped, ids=ids, **redact)
    if draw is not None:
        caffe.draw_people(frames, people, n_people=clamped, ids=ids, cand=cand, **draw)
    caffe.label_people(frames, people, n_people=clamped, ids=ids, **labels)
    _assert_same("synchronous entries against the restatement", _download(surfaces, tensors), want)
    for place in where:
        got, r = _overlay(caffe, surfaces, people, n, cand, ids, draw, redact, labels, place)
        _assert_same("overlay on %s frames" % place, got, want)
        if redact is not None:
            assert r.dtype == np.int32 and np.array_equal(r, red), (place, r, red)
    return want, red


@pytest.mark.parametrize("fmt", FORMATS)
def test_labels_alone_equal_label_people(gpu_caffe, fmt):
    people, ids = _crowd()
    surfaces = _surfaces(fmt)
    want, _ = _check(gpu_caffe, surfaces, people, n=[5, 0, 5], ids=ids, labels=LABELS)
    assert not _same(want[:1], surfaces[:1]) and _same(want[1:2], surfaces[1:2])
    _check(gpu_caffe, surfaces, people, n=[5, 0, 4], labels=dict(LABELS, scale=3, anchor=None, color="text"), where=("device",))  # no ids: indices
    _check(gpu_caffe, surfaces, people, n=[5, 0, 5], ids=ids, labels=dict(LABELS, scale=8, alpha_plate=0, prefix=""), where=("device",))
    none, _ = _check(gpu_caffe, surfaces, people, n=[5, 0, 5], ids=ids, labels=dict(LABELS, alpha_plate=0, alpha_text=0), where=("device",))
    assert _same(none, surfaces)


@pytest.mark.parametrize("fmt", FORMATS)
def test_redact_draw_and_labels_together_keep_their_order(gpu_caffe, fmt):
    import torch

    people, ids = _crowd()
    cand = np.where(np.random.RandomState(2).rand(3, 5, 14) < 0.2, -2, 0).astype(np.int32)
    draw = dict(edges=SKELETON, joint_radius=3.0, limb_radius=1.5, alpha=200, alpha_filled=90, palette=SEVEN)
    redact = dict(GEOMETRY, region="head_or_body", effect="mosaic", block=8, only_ids=[int(v) for v in ids[0, :3]] + [int(ids[2, 1])])
    surfaces = _surfaces(fmt)
    want, red = _check(gpu_caffe, surfaces, people, n=[5, 0, 5], cand=cand, ids=ids, draw=draw, redact=redact, labels=LABELS)
    # `redacted` is what the route without labels reports, and without labels the bytes are the older route's
    plain_want, plain_red = _restated(surfaces, people, np.array([5, 0, 5]), cand, ids, draw, redact)
    got, r = _overlay(gpu_caffe, surfaces, people, np.array([5, 0, 5], np.int32), cand, ids, draw, redact, None)
    _assert_same("labels=None", got, plain_want)
    assert np.array_equal(r, plain_red) and np.array_equal(red, plain_red) and not _same(want, plain_want)
    # a caller's stream with device frames: asynchronous, the same bytes
    got, _ = _overlay(gpu_caffe, surfaces, people, np.array([5, 0, 5], np.int32), cand, ids, draw, redact, LABELS, stream=torch.cuda.Stream())
    _assert_same("on a stream", got, want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_256_people_on_one_tile_and_counts_read_as_clamped(gpu_caffe, fmt):
    rs = np.random.RandomState(11)
    people = np.zeros((3, 256, 14, 3))
    # every plate (at scale 1 with "P" and three digits: 25 x 9) holds pixel (40, 40) of tile (1, 1): the self-binning walk takes two passes
    people[:, :, 13, 0] = 34.0 + rs.randint(0, 14, (3, 256))
    people[:, :, 13, 1] = 42.0 + rs.randint(0, 8, (3, 256))
    people[:, :, 13, 2] = 0.9
    ids = (100 + rs.permutation(3 * 256).reshape(3, 256) % 900).astype(np.int64)
    surfaces = _surfaces(fmt)
    labels = dict(LABELS, gap=0, alpha_plate=90, alpha_text=180)
    for b in (0, 2):
        labs = LR.labels(people[b], 67, 101, ids=ids[b], **labels)
        assert len(labs) == 256 and all(v["X"] <= 40 < v["X"] + v["pw"] and v["Y"] <= 40 < v["Y"] + v["ph"] for v in labs)
    _check(gpu_caffe, surfaces, people, n=[256, -3, 300], ids=ids, labels=labels, where=("device",))  # -3 reads as 0, 300 as 256
