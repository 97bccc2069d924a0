"""GPU: `caffe.overlay_people_device` (dc_overlay_people_device) — the device half of the in-chain overlays alone, on crafted people that
are uploaded with torch.  Every comparison is BYTE FOR BYTE, whole buffers (pitch padding and a guard row behind each plane, pre-filled
with a sentinel, included): against the numpy restatements tests/redact_ref.py then tests/draw_ref.py, AND against the synchronous
`caffe.redact_people` then `caffe.draw_people` on a copy of the frame.  The rules are integer only, so there is no tolerance.

PARITY UNPINNED BY THE REFERENCE, which draws with matplotlib on the host and redacts nothing; the rules are this project's own.

Shapes: 67 x 101 frames — odd both ways, so NV12 has chroma blocks of 2 and 1 pixels, and 3 x 4 tiles of 32 x 32 with partial ones —, NV12
and BGR24, nb = 3 with frame 1 holding nobody."""
import functools

import numpy as np
import pytest

import draw_ref as DR
import redact_ref as RR

pytestmark = pytest.mark.gpu

SENT = 0xA5
H, W = 67, 101
SKELETON = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7), (7, 8), (8, 12), (12, 9), (9, 10), (10, 11), (12, 13), (2, 8), (3, 9))
JOINT_COLORS = tuple([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 245, 255), (255, 131, 250), (255, 255, 0)] * 2 + [(0, 0, 0), (255, 255, 255)])
SEVEN = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240))
GEOMETRY = dict(head=(12, 13), edges=SKELETON, head_scale=0.75, body_scale=0.06, min_radius=2.0, max_radius=256.0)
FORMATS = ["bgr", "nv12"]


# ---- pitched surfaces: every pitch padded by 13 bytes, a guard row behind each plane -----------------------------------------------------
class Surface(object):
    def __init__(self, fmt, h=H, w=W, seed=3, matrix="bt601", range_="limited"):
        self.fmt, self.h, self.w, self.matrix, self.range = fmt, h, w, matrix, range_
        rows, self.pitch = ([h], [3 * w + 13]) if fmt == "bgr" else ([h, (h + 1) // 2], [w + 13, 2 * ((w + 1) // 2) + 13])
        self.bufs = [np.full((r + 1, p), SENT, np.uint8) for r, p in zip(rows, self.pitch)]
        rs = np.random.RandomState(seed)
        for v in self.views():
            v[...] = rs.randint(0, 256, v.shape)

    def views(self):
        strided = np.lib.stride_tricks.as_strided
        if self.fmt == "bgr":
            return [strided(self.bufs[0], (self.h, self.w, 3), (self.pitch[0], 3, 1))]
        return [self.bufs[0][:self.h, :self.w], strided(self.bufs[1], ((self.h + 1) // 2, (self.w + 1) // 2, 2), (self.pitch[1], 2, 1))]

    def copy(self):
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__)
        c.bufs = [b.copy() for b in self.bufs]
        return c

    def host_frame(self, caffe):
        v = self.views()
        return caffe.Frame.bgr(v[0]) if self.fmt == "bgr" else caffe.Frame.nv12(v[0], v[1], matrix=self.matrix, range=self.range)

    def device_frame(self, caffe, tensors):
        if self.fmt == "bgr":
            return caffe.Frame.bgr_device(tensors[0].data_ptr(), self.h, self.w, self.pitch[0])
        return caffe.Frame.nv12_device(tensors[0].data_ptr(), tensors[1].data_ptr(), self.h, self.w, self.pitch[0], self.pitch[1],
                                       matrix=self.matrix, range=self.range)


def _surfaces(fmt, nb=3, **kw):
    return [Surface(fmt, seed=3 + b, **kw) for b in range(nb)]


def _assert_same(place, got, want):
    for b, (g, w_) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g.bufs, w_.bufs)):
            bad = np.argwhere(x != y)
            assert bad.size == 0, "%s frame %d plane %d: %d bytes differ, first at %s: got %d, want %d" % (
                place, b, k, len(bad), tuple(bad[0]), x[tuple(bad[0])], y[tuple(bad[0])])


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s.bufs, t.bufs))


# ---- the three routes ------------------------------------------------------------------------------------------------------------------
def _select(ids, redact):
    """only_ids / keep_ids of a redact dict -> the restatement's select [nb, P] (None: everyone)."""
    only, keep = redact.get("only_ids"), redact.get("keep_ids")
    if only is None and keep is None:
        return None
    sel = np.ones(ids.shape, bool)
    if only is not None:
        sel &= np.isin(ids, np.asarray(list(only), np.int64))
    if keep is not None:
        sel &= ~np.isin(ids, np.asarray(list(keep), np.int64))
    return sel


def _restated(surfaces, people, n, cand, ids, draw, redact):
    """tests/redact_ref.py then tests/draw_ref.py -> (surfaces, redacted [nb, P] or None)."""
    want, red = [s.copy() for s in surfaces], []
    for b, s in enumerate(want):
        v = s.views()
        if redact is not None:
            sel = _select(ids, redact)
            style = {k: x for k, x in redact.items() if k not in ("only_ids", "keep_ids")}
            prims, r = RR.primitives(people[b], n[b], None if sel is None else sel[b], **style)
            effect = (style.get("effect", "mosaic"), style.get("block", 8), style.get("fill", (0, 0, 0)))
            if s.fmt == "bgr":
                RR.redact_bgr(v[0], prims, *effect)
            else:
                RR.redact_nv12(v[0], v[1], prims, s.matrix, s.range, *effect)
            red.append(r)
        if draw is not None:
            prims = DR.primitives(people[b], n[b], None if cand is None else cand[b], None if ids is None else ids[b], **draw)
            if s.fmt == "bgr":
                DR.draw_bgr(v[0], prims)
            else:
                DR.draw_nv12(v[0], v[1], prims, s.matrix, s.range)
    return want, np.stack(red) if red else None


def _upload(surfaces):
    import torch

    return [[torch.from_numpy(b).cuda() for b in s.bufs] for s in surfaces]


def _download(surfaces, tensors):
    got = [s.copy() for s in surfaces]
    for g, t in zip(got, tensors):
        g.bufs = [x.cpu().numpy() for x in t]
    return got


def _synchronous(caffe, surfaces, people, n, cand, ids, draw, redact):
    """`caffe.redact_people` then `caffe.draw_people` on device copies -> (surfaces, redacted)."""
    import torch

    tensors = _upload(surfaces)
    torch.cuda.synchronize()
    frames = [s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)]
    red = None
    if redact is not None:
        red = caffe.redact_people(frames, people, n_people=n, ids=ids, **redact)
    if draw is not None:
        caffe.draw_people(frames, people, n_people=n, ids=ids, cand=cand, **draw)
    return _download(surfaces, tensors), red


def _overlay(caffe, surfaces, people, n, cand, ids, draw, redact, where="device", calls=1, stream=None):
    """`caffe.overlay_people_device` with everything about the people in device memory -> (surfaces, redacted)."""
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
    for _ in range(calls):
        caffe.overlay_people_device(frames, t_people, t_n, cand=t_cand, ids=t_ids, draw=draw, redact=redact, redacted=t_red,
                                    stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    if where == "device":
        got = _download(surfaces, tensors)
    return got, None if t_red is None else t_red.cpu().numpy()


def _check(caffe, surfaces, people, n=None, cand=None, ids=None, draw=None, redact=None, where=("device", "host")):
    """The overlay on device and on host frames against the restatement and against the synchronous calls; -> (want, redacted)."""
    n = np.full(people.shape[0], people.shape[1], np.int32) if n is None else np.asarray(n, np.int32)
    want, red = _restated(surfaces, people, n, cand, ids, draw, redact)
    sync, sync_red = _synchronous(caffe, surfaces, people, n, cand, ids, draw, redact)
    _assert_same("synchronous entries against the restatement", sync, want)
    for place in where:
        got, r = _overlay(caffe, surfaces, people, n, cand, ids, draw, redact, place)
        _assert_same("overlay on %s frames" % place, got, want)
        if redact is not None:
            assert r.dtype == np.int32 and np.array_equal(r, red) and np.array_equal(r, sync_red), (place, r, red, sync_red)
    return want, red


# ---- 1. order under load ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forty(x0, y0):
    """40 people of the MPII skeleton with every joint inside the 28 x 28 pixels at (x0, y0), at 1/32 pixel."""
    rs = np.random.RandomState(11)
    p = np.zeros((40, 14, 3))
    p[:, :, 0] = x0 + np.round(rs.uniform(0, 28, (40, 14)) * 32) / 32
    p[:, :, 1] = y0 + np.round(rs.uniform(0, 28, (40, 14)) * 32) / 32
    p[:, :, 2] = rs.uniform(0.3, 1.0, (40, 14))
    return p


@pytest.mark.parametrize("fmt", FORMATS)
def test_order_is_kept_over_more_than_four_passes_in_one_tile_and_across_a_tile_corner(gpu_caffe, fmt):
    """Frame 0: all 1 120 primitives inside tile (1, 1); frame 1: nobody; frame 2: the same scene astride the corner of four tiles.  Half
    opaque and coloured by joint: any change of order changes bytes."""
    _tw, _th, chunk = gpu_caffe.draw_limits()
    people = np.stack([_forty(34.0, 34.0), np.zeros((40, 14, 3)), _forty(18.0, 18.0)])
    draw = dict(edges=SKELETON, joint_radius=2.5, limb_radius=1.25, alpha=128, color="joint", palette=JOINT_COLORS)
    n_prims = len(DR.primitives(people[0], **draw))
    assert n_prims == 40 * 28 > 4 * 256 and n_prims > chunk
    assert all(32 <= v < 64 for v in (people[0, :, :, :2].min(), people[0, :, :, :2].max())) and people[2, :, :, 0].min() < 32 < people[2, :, :, 0].max()
    surfaces = _surfaces(fmt)
    want, _ = _check(gpu_caffe, surfaces, people, n=[40, 0, 40], draw=draw)
    assert _same(want[1:2], surfaces[1:2]) and not _same(want[:1], surfaces[:1]) and not _same(want[2:], surfaces[2:])
    # the order is visible: the same people the other way round give other bytes
    other, _ = _restated(surfaces, people[:, ::-1], [40, 0, 40], None, None, draw, None)
    assert not _same(other, want)


# ---- 2. the rule's edges ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_people():
    """nb = 3, P = 6.  Frame 0: the joints the rule drops and keeps; frame 1: nobody; frame 2: a long thin limb, and people beyond the frame."""
    p = np.zeros((3, 6, 14, 3))
    a = p[0]
    a[0, :6] = [(12.0, 9.0, 0.9), (np.nan, 20.0, 0.9), (30.0, np.inf, 0.9), (40.5, 12.25, np.nan), (52.03125, 30.0, 0.25), (60.0, 31.96875, 0.2500001)]
    a[1, :6] = [(-3.0, 5.0, 0.8), (4.0, -2.5, 0.8), (W + 1.5, 20.0, 0.8), (W + 40.0, 30.0, 0.8), (50.0, H + 2.0, 0.8), (50.0, H + 70.0, 0.8)]
    a[2, 6:14] = [(20.0 + 7 * k, 40.0 + 3 * (k % 3), 0.7) for k in range(8)]   # cand marks some of them filled / bridged
    a[3, 6:14] = [(18.0 + 9 * k, 50.5 + 2 * (k % 2), 0.6) for k in range(8)]
    a[4, 12], a[4, 13] = (70.0, 20.0, 0.9), (74.0, 8.0, 0.9)
    c = p[2]
    c[0, 0], c[0, 1] = (4.0, 4.0, 0.9), (97.0, 62.0, 0.9)      # from tile (0, 0) to tile (3, 1): its box's other corners hold nothing of it
    c[1, :3] = [(-500.0, -500.0, 0.9), (-400.0, -450.0, 0.9), (-40000.0, 10.0, 0.9)]  # dropped, and clamped to -32768
    c[2, :2] = [(5000.0, 30.0, 0.9), (40000.0, 30.0, 0.9)]
    c[3, 12], c[3, 13] = (33.0, 33.0, 0.9), (31.0, 29.0, 0.9)  # a head astride the corner of four tiles
    p.setflags(write=False)
    return p


def _edge_cand():
    cand = np.zeros((3, 6, 14), np.int32)
    cand[0, 2, 7], cand[0, 2, 9], cand[0, 3, 12], cand[0, 0, 0] = -2, -3, -3, -1
    cand[2, 0, 1] = -2
    return cand


EDGE_IDS = np.array([[-1, 0, (1 << 40) + 3, 5, 6, 7], [1, 2, 3, 4, 5, 6], [(1 << 40) + 3, -1, 0, 13, 1, 2]], np.int64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_drawing_rule_edges(gpu_caffe, fmt):
    people, cand = _edge_people(), _edge_cand()
    n = [5, 0, 4]
    surfaces = _surfaces(fmt)
    draw = dict(edges=SKELETON, joint_radius=3.0, limb_radius=1.0, alpha=200, alpha_filled=64, min_score=0.25, color="id", palette=SEVEN,
                untracked=(9, 200, 77))
    prims = DR.primitives(people[0], 5, cand[0], EDGE_IDS[0], **draw)
    assert {64, 200} == {q["alpha"] for q in prims} and (9, 200, 77) in {q["rgb"] for q in prims}
    assert not any(q["a"] == (832, 480) for q in prims)  # score == min_score: not drawn
    assert SEVEN[((1 << 40) + 3) % 7] in {q["rgb"] for q in prims}
    want, _ = _check(gpu_caffe, surfaces, people, n=n, cand=cand, ids=EDGE_IDS, draw=draw)
    assert _same(want[1:2], surfaces[1:2]) and not _same(want[2:], surfaces[2:])
    # the long limb leaves the tiles at its box's other two corners as they are
    before, after = surfaces[2].views()[0], want[2].views()[0]
    assert np.array_equal(before[:32, 64:96], after[:32, 64:96]) and np.array_equal(before[40:64, :32], after[40:64, :32])
    # ids null: the person's index chooses the colour; cand null: alpha everywhere; either radius 0: that kind is not drawn
    plain, _ = _check(gpu_caffe, surfaces, people, n=n, draw=draw, where=("device",))
    assert not _same(plain, want)
    _check(gpu_caffe, surfaces, people, n=n, cand=cand, ids=EDGE_IDS, draw=dict(draw, joint_radius=0.0), where=("device",))
    _check(gpu_caffe, surfaces, people, n=n, cand=cand, ids=EDGE_IDS, draw=dict(draw, limb_radius=0.0, color="joint"), where=("device",))
    none, _ = _check(gpu_caffe, surfaces, people, n=n, draw=dict(draw, limb_radius=0.0, joint_radius=0.0), where=("device",))
    assert _same(none, surfaces)


# ---- 3. the limits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_limits_256_people_32_joints_128_edges(gpu_caffe, fmt):
    """P = n_people = 256, J = 32, 128 edges, tiny radii, one frame; five held joints a person keep the restatement quick."""
    rs = np.random.RandomState(21)
    people = np.zeros((1, 256, 32, 3))
    for p in range(256):
        for j in rs.choice(32, 5, replace=False):
            people[0, p, j] = (np.round(rs.uniform(-4, W + 4) * 16) / 16, np.round(rs.uniform(-4, H + 4) * 16) / 16, rs.uniform(0.3, 1.0))
    edges = [(int(a), int(c)) for a, c in rs.randint(0, 32, (128, 2))]
    ids = rs.randint(-1, 1000, (1, 256)).astype(np.int64)
    cand = rs.randint(-3, 4, (1, 256, 32)).astype(np.int32)
    draw = dict(edges=edges, joint_radius=0.75, limb_radius=0.5, alpha=150, alpha_filled=90, color="id", palette=SEVEN)
    redact = dict(region="head_or_body", head=(30, 31), edges=edges, head_scale=0.1, body_scale=0.01, min_radius=0.5, max_radius=3.0, block=2)
    surfaces = _surfaces(fmt, nb=1)
    want, red = _check(gpu_caffe, surfaces, people, cand=cand, ids=ids, draw=draw, redact=redact, where=("device",))
    assert red.all() and not _same(want, surfaces)


# ---- 4. the redaction ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crowd(seed=3, count=5):
    """People scattered over the frame, joints within 16 px of the person's centre; joints missing here and there; person 1 has no head top."""
    rs = np.random.RandomState(seed)
    p = np.zeros((count, 14, 3))
    centre = np.stack([rs.uniform(0, W, count), rs.uniform(0, H, count)], 1)
    p[:, :, :2] = np.round((centre[:, None, :] + rs.uniform(-16, 16, (count, 14, 2))) * 32) / 32
    p[:, :, 2] = rs.uniform(0.2, 1.0, (count, 14))
    p[rs.rand(count, 14) < 0.15] = 0.0
    p[1, 13] = 0.0
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("block", [2, 8, 32])
@pytest.mark.parametrize("region", ["head", "body", "head_or_body"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_redaction_regions_and_blocks(gpu_caffe, fmt, region, block):
    people = np.stack([_crowd(3), _crowd(4), _crowd(5)])
    effect = dict(effect="fill", fill=(200, 30, 90)) if block == 8 else dict(effect="mosaic")
    redact = dict(GEOMETRY, region=region, block=block, **effect)
    surfaces = _surfaces(fmt, matrix="bt709", range_="full")
    want, red = _check(gpu_caffe, surfaces, people, n=[5, 0, 4], redact=redact)
    assert red[0, 1] == (0 if region == "head" else 1) and not red[1].any() and not red[2, 4] and red[2, :4].any()
    assert _same(want[1:2], surfaces[1:2]) and not _same(want[:1], surfaces[:1])
    if effect["effect"] == "mosaic":  # applied twice, the mosaic changes nothing
        twice, _ = _overlay(gpu_caffe, surfaces, people, np.array([5, 0, 4], np.int32), None, None, None, redact, calls=2)
        _assert_same("the mosaic twice", twice, want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_redaction_by_only_ids_and_keep_ids(gpu_caffe, fmt):
    people = np.stack([_crowd(3), _crowd(4), _crowd(5)])
    ids = np.array([[4, 9, -1, 4, (1 << 40) + 3], [7, 7, 2, 0, 1], [20, 21, 22, 23, 24]], np.int64)
    surfaces = _surfaces(fmt)
    base = dict(GEOMETRY, region="head_or_body", block=4)
    everyone, _ = _check(gpu_caffe, surfaces, people, n=[5, 0, 5], ids=ids, redact=base, where=("device",))
    seen = []
    for lists in (dict(only_ids=[4, 22, (1 << 40) + 3]), dict(keep_ids=[9, -1, 20, 21]), dict(only_ids=[4, 9, 21], keep_ids=[9]), dict(only_ids=[])):
        want, red = _check(gpu_caffe, surfaces, people, n=[5, 0, 5], ids=ids, redact=dict(base, **lists), where=("device",))
        seen.append(red.tolist())
        assert not _same(want, everyone)
    assert seen[0] == [[1, 0, 0, 1, 1], [0] * 5, [0, 0, 1, 0, 0]] and seen[1] == [[1, 0, 0, 1, 1], [0] * 5, [0, 0, 1, 1, 1]]
    assert seen[2] == [[1, 0, 0, 1, 0], [0] * 5, [0, 1, 0, 0, 0]] and not np.any(seen[3])


# ---- 5. both styles in one call, and a caller's stream ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_both_styles_in_one_call_are_redact_then_draw(gpu_caffe, fmt):
    import torch

    people = np.stack([_crowd(3), _crowd(4), _crowd(5)])
    ids = np.arange(15, dtype=np.int64).reshape(3, 5) - 1
    cand = np.random.RandomState(2).randint(-3, 3, (3, 5, 14)).astype(np.int32)
    draw = dict(edges=SKELETON, joint_radius=3.0, limb_radius=1.5, alpha=160, alpha_filled=70, color="id", palette=SEVEN)
    redact = dict(GEOMETRY, region="body", block=8)
    surfaces = _surfaces(fmt)
    n = np.array([5, 0, 3], np.int32)
    want, _ = _check(gpu_caffe, surfaces, people, n=n, cand=cand, ids=ids, draw=draw, redact=redact)
    only_redacted, _ = _restated(surfaces, people, n, cand, ids, None, redact)
    only_drawn, _ = _restated(surfaces, people, n, cand, ids, draw, None)
    assert not _same(want, only_redacted) and not _same(want, only_drawn)
    # on a caller's stream the call is asynchronous; the bytes are the same once that stream has run
    got, _ = _overlay(gpu_caffe, surfaces, people, n, cand, ids, draw, redact, stream=torch.cuda.Stream())
    _assert_same("on a caller's stream", got, want)
