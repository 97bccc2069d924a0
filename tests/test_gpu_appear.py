"""GPU: `caffe.describe_people` (dc_describe_people) against the numpy restatement of its rule in tests/appear_ref.py, EXACTLY — the rule
is integer only, so there is no tolerance —, on host and on device frames; and every frame byte, the pitch padding (pre-filled with a
sentinel) included, is what it was: the call only reads frames.

PARITY UNPINNED BY THE REFERENCE, which stops at the maps; the rule is this project's own.

Shapes: a BGR24 frame 70 x 90 with pitch padding and an NV12 frame 71 x 93 (odd both ways: chroma blocks of 2 and 1 pixels, 3 x 3 tiles of
32 x 32 with partial ones), and 160 primitives in one tile (beyond the chunk of 64)."""
import functools

import numpy as np
import pytest

import appear_ref as AR
from test_gpu_draw import _surface

pytestmark = pytest.mark.gpu

SIDES = {"bgr": (70, 90), "nv12": (71, 93)}
TORSO = ((8, 2), (9, 3), (8, 9), (2, 3))  # MPII: right shoulder - right hip, left shoulder - left hip, the shoulders, the hips
STYLE = dict(edges=TORSO, scale=0.1, min_radius=1.5, min_score=0.1)


def _surfaces(fmt, count=1):
    h, w = SIDES[fmt]
    return [_surface(fmt, h, w, seed=3 + k) for k in range(count)]


def _torso(cx, cy, half_w, half_h, score=0.9):
    """A person [14, 3] whose shoulders and hips stand around (cx, cy); every other joint is missing."""
    p = np.zeros((14, 3))
    p[8], p[9] = (cx - half_w, cy - half_h, score), (cx + half_w, cy - half_h, score)
    p[2], p[3] = (cx - half_w + 1.5, cy + half_h, score), (cx + half_w - 1.25, cy + half_h, score)
    return p


def _reference(surfaces, people, n_people, **style):
    out = []
    for b, s in enumerate(surfaces):
        v = s.views()
        n = None if n_people is None else n_people[b]
        out.append(AR.describe_bgr(v[0], people[b], n, **style) if len(v) == 1 else AR.describe_nv12(v[0], v[1], people[b], n, **style))
    return np.stack(out)


def _unchanged(place, got, surfaces):
    for b, (g, s) in enumerate(zip(got, surfaces)):
        for k, (x, y) in enumerate(zip(g, s.bufs)):
            assert np.array_equal(x, y), "%s frame %d plane %d: the call changed %d bytes" % (place, b, k, int((x != y).sum()))


def _check(caffe, surfaces, people, n_people=None, **style):
    """Host frames (read-only arrays) and device frames against the restatement -> the descriptors [nb, P, 3, 16]."""
    import torch

    style = dict(STYLE, **style)
    people = np.asarray(people, np.float64)
    want = _reference(surfaces, people, n_people, **style)
    # host: the arrays are read-only — a store by the library's host half would fault, one by the device cannot reach them
    host = [s.copy() for s in surfaces]
    for s in host:
        for buf in s.bufs:
            buf.setflags(write=False)
    got = caffe.describe_people([s.host_frame(caffe) for s in host], people, n_people, **style)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), ("host", np.argwhere(got != want)[:5].tolist())
    _unchanged("host", [s.bufs for s in host], surfaces)
    # device
    tensors = [[torch.from_numpy(b.copy()).cuda() for b in s.bufs] for s in surfaces]
    torch.cuda.synchronize()
    got = caffe.describe_people([s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)], people, n_people, **style)
    assert np.array_equal(got, want), ("device", np.argwhere(got != want)[:5].tolist())
    _unchanged("device", [[x.cpu().numpy() for x in t] for t in tensors], surfaces)
    return want


@functools.lru_cache(maxsize=None)
def _scene():
    """Six people: across the corner (32, 32) of four tiles; partly outside the frame's right and bottom edge; wholly outside; two that
    overlap; one without a held torso joint (its arms are there, so it has a size).  Coordinates at odd sixteenths and ties."""
    lost = np.zeros((14, 3))
    lost[6], lost[7], lost[10] = (20.0, 50.0, 0.8), (24.0, 58.0, 0.8), (30.0, 52.0, 0.8)
    lost[8] = (22.0, 44.0, 0.05)  # a shoulder below min_score
    p = np.stack([_torso(32.03125, 32.21875, 9.5, 11.0), _torso(84.5, 62.5, 9.0, 12.0), _torso(300.0, 200.0, 8.0, 10.0),
                  _torso(60.0, 20.0, 7.0, 8.0), _torso(64.5, 24.25, 7.0, 8.0), lost])
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_regions_on_tile_corners_edges_and_overlaps(gpu_caffe, fmt):
    s = _surfaces(fmt)
    want = _check(gpu_caffe, s, _scene()[None])
    n = want[0].sum(axis=2)  # [P, 3]: each channel's counts sum to the region's pixels
    assert (n == n[:, :1]).all()
    assert n[0, 0] > 0 and n[1, 0] > 0 and n[3, 0] > 0 and n[4, 0] > 0
    assert n[2, 0] == 0 and n[5, 0] == 0  # wholly outside; no held torso limb
    h, w = SIDES[fmt]
    # person 0 reaches all four tiles around (32, 32); person 1 is cut by the frame: fewer pixels than the same torso well inside
    ys, xs = np.nonzero(AR.region(h, w, AR.capsules(_scene()[0], **STYLE)))
    assert ys.min() < 32 <= ys.max() and xs.min() < 32 <= xs.max()
    inside = AR.region(200, 200, AR.capsules(_scene()[1], **STYLE)).sum()
    assert 0 < n[1, 0] < inside
    # the two overlapping people share pixels, and each counts them
    a, b = (AR.region(h, w, AR.capsules(_scene()[k], **STYLE)) for k in (3, 4))
    assert (a & b).any() and n[3, 0] == a.sum() and n[4, 0] == b.sum()


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_three_frames_with_different_people_counts(gpu_caffe, fmt):
    """nb = 3: n_people 6, 0 and 2 of P = 6 — desc is zeros beyond n_people, and a frame without people is not read."""
    people = np.stack([_scene(), _scene()[::-1], _scene()[[3, 0, 1, 2, 4, 5]]])
    want = _check(gpu_caffe, _surfaces(fmt, 3), people, n_people=[6, 0, 2])
    assert want[0].any() and not want[1].any() and want[2, :2].any() and not want[2, 2:].any()


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_forty_people_on_one_spot_walk_the_chunks(gpu_caffe, fmt):
    """40 people of 4 limbs stacked inside tile (1, 1) behind one of 2 limbs: 160 + 2 primitives in one tile, past the chunk of 64, so
    the chunk loop runs three times.  Runs of 4 alone would end exactly on the chunk boundaries (64 = 16 x 4); behind the run of 2 the
    runs of person 16 (primitives 62 .. 65) and person 32 (126 .. 129) straddle them."""
    people = np.stack([_torso(47.0 + (k % 5) * 0.4375, 47.5 + (k // 5) * 0.3125, 5.0 + (k % 3) * 0.5, 6.0 + (k % 4) * 0.25) for k in range(41)])
    people[0, 3] = 0.0  # person 0 loses a hip: 2 limbs
    caps = [AR.capsules(p, **STYLE) for p in people]
    assert [len(c) for c in caps] == [2] + [4] * 40
    h, w = SIDES[fmt]
    for c in caps:
        ys, xs = np.nonzero(AR.region(h, w, c))
        assert 32 <= ys.min() and ys.max() < 64 and 32 <= xs.min() and xs.max() < 64  # one tile
    want = _check(gpu_caffe, _surfaces(fmt), people[None])
    assert (want[0].sum(axis=2) > 0).all() and len({w_.tobytes() for w_ in want[0]}) > 20  # the people differ


def test_no_region_reaches_a_frame_and_single_frame_shapes(gpu_caffe):
    """Nothing to launch: all zeros; a [m, J, 3] array for one frame gives [m, 3, 16]; a plain BGR array is taken like `Frame.bgr`."""
    s = _surfaces("bgr")[0]
    img = np.ascontiguousarray(s.views()[0])
    img.setflags(write=False)
    far = np.stack([_torso(300.0, 200.0, 8.0, 10.0), _torso(-90.0, -40.0, 8.0, 10.0)])
    got = gpu_caffe.describe_people(img, far, **STYLE)
    assert got.shape == (2, 3, 16) and got.dtype == np.int32 and not got.any()
    import pose

    near = _scene()[:2]
    got = pose.describe_people(img, near, scale=STYLE["scale"], min_radius=STYLE["min_radius"], min_score=STYLE["min_score"])
    assert pose.TORSO_MPII14 == TORSO and np.array_equal(got, AR.describe_bgr(img, near, **STYLE))
