"""GPU: `caffe.draw_people` (dc_draw_people) against the numpy restatement of its rule in tests/draw_ref.py, BYTE FOR BYTE, the pitch
padding (pre-filled with a sentinel) included — the rule is integer only, so there is no tolerance.

PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host; the rule is this project's own.

Shapes: 71 x 93 frames (odd both ways: chroma blocks of 2 and 1 pixels exist; 3 x 3 tiles of 32 x 32, the last ones partial) and a
64 x 256 frame for the limbs that run tens of thousands of pixels out of it."""
import functools

import numpy as np
import pytest

import draw_ref as DR
import nv12_ref as NR

pytestmark = pytest.mark.gpu

SENT = 0xA5
H, W = 71, 93
SKELETON = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7), (7, 8), (8, 12), (12, 9), (9, 10), (10, 11), (12, 13), (2, 8), (3, 9))
ID_COLORS = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48))
JOINT_COLORS = tuple([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 245, 255), (255, 131, 250), (255, 255, 0)] * 2 + [(0, 0, 0), (255, 255, 255)])
PAIRS = [(m, r) for m in NR.MATRICES for r in NR.RANGES]


# ---- pitched surfaces ------------------------------------------------------------------------------------------------------------------
class Bgr(object):
    def __init__(self, h, w, pitch, seed):
        self.h, self.w, self.pitch = h, w, pitch
        self.bufs = [np.full((h, pitch), SENT, np.uint8)]
        self.views()[0][...] = np.random.RandomState(seed).randint(0, 256, (h, w, 3))

    def views(self):
        return [np.lib.stride_tricks.as_strided(self.bufs[0], (self.h, self.w, 3), (self.pitch, 3, 1))]

    def copy(self):
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__)
        c.bufs = [b.copy() for b in self.bufs]
        return c

    def host_frame(self, caffe):
        return caffe.Frame.bgr(self.views()[0])

    def device_frame(self, caffe, tensors):
        return caffe.Frame.bgr_device(tensors[0].data_ptr(), self.h, self.w, self.pitch)

    def reference(self, prims, stats=None):
        DR.draw_bgr(self.views()[0], prims, stats)


class Nv12(Bgr):
    def __init__(self, h, w, py, puv, seed, matrix="bt601", range_="limited"):
        self.h, self.w, self.py, self.puv, self.matrix, self.range = h, w, py, puv, matrix, range_
        ch, cw = (h + 1) // 2, (w + 1) // 2
        self.bufs = [np.full((h, py), SENT, np.uint8), np.full((ch, puv), SENT, np.uint8)]
        rs = np.random.RandomState(seed)
        y, uv = self.views()
        y[...] = rs.randint(0, 256, (h, w))
        uv[...] = rs.randint(0, 256, (ch, cw, 2))

    def views(self):
        ch, cw = (self.h + 1) // 2, (self.w + 1) // 2
        return [self.bufs[0][:, :self.w], np.lib.stride_tricks.as_strided(self.bufs[1], (ch, cw, 2), (self.puv, 2, 1))]

    def host_frame(self, caffe):
        y, uv = self.views()
        return caffe.Frame.nv12(y, uv, matrix=self.matrix, range=self.range)

    def device_frame(self, caffe, tensors):
        return caffe.Frame.nv12_device(tensors[0].data_ptr(), tensors[1].data_ptr(), self.h, self.w, self.py, self.puv, matrix=self.matrix,
                                       range=self.range)

    def reference(self, prims, stats=None):
        y, uv = self.views()
        DR.draw_nv12(y, uv, prims, self.matrix, self.range, stats)


def _surface(fmt, h=H, w=W, seed=3, pair=("bt601", "limited")):
    if fmt == "bgr":
        return Bgr(h, w, 3 * w + 13, seed)
    return Nv12(h, w, w + 7, 2 * ((w + 1) // 2) + 10, seed, *pair)


def _on_host(caffe, surfaces, people, **kw):
    got = [s.copy() for s in surfaces]
    caffe.draw_people([s.host_frame(caffe) for s in got], people, **kw)
    return got


def _on_device(caffe, surfaces, people, **kw):
    import torch

    tensors = [[torch.from_numpy(b).cuda() for b in s.bufs] for s in surfaces]
    torch.cuda.synchronize()
    caffe.draw_people([s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)], people, **kw)
    got = [s.copy() for s in surfaces]
    for g, t in zip(got, tensors):
        g.bufs = [x.cpu().numpy() for x in t]
    return got


def _reference(surfaces, people, n_people=None, cand=None, ids=None, stats=None, **style):
    want = [s.copy() for s in surfaces]
    for b, s in enumerate(want):
        prims = DR.primitives(people[b], None if n_people is None else n_people[b], None if cand is None else cand[b],
                              None if ids is None else ids[b], **style)
        s.reference(prims, stats)
    return want


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s.bufs, t.bufs))


def _ref_style(kw):
    """The call's keyword arguments as the restatement takes them (the palette always explicit)."""
    return {k: v for k, v in kw.items() if k not in ("n_people", "cand", "ids")}


def _check(caffe, surfaces, people, where=("host", "device"), stats=None, **kw):
    """Host and device frames against the restatement; -> the restatement's surfaces."""
    want = _reference(surfaces, people, kw.get("n_people"), kw.get("cand"), kw.get("ids"), stats, **_ref_style(kw))
    for place in where:
        got = (_on_host if place == "host" else _on_device)(caffe, surfaces, people, **kw)
        for b, (g, w_) in enumerate(zip(got, want)):
            for k, (x, y) in enumerate(zip(g.bufs, w_.bufs)):
                bad = np.argwhere(x != y)
                assert bad.size == 0, "%s frame %d plane %d: %d bytes differ, first at %s: got %d, want %d" % (
                    place, b, k, len(bad), tuple(bad[0]), x[tuple(bad[0])], y[tuple(bad[0])])
    return want


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crowd(seed=7, people=5, h=H, w=W):
    """A handful of people whose limbs cross the frame and its tile borders; joints missing here and there; the last person half outside
    the frame; coordinates at odd sixteenths and on rounding ties."""
    rs = np.random.RandomState(seed)
    p = np.zeros((people, 14, 3))
    p[:, :, 0] = np.round(rs.uniform(-6, w + 6, (people, 14)) * 32) / 32  # 1/32 px: half of them ties of the 1/16 grid
    p[:, :, 1] = np.round(rs.uniform(-6, h + 6, (people, 14)) * 32) / 32
    p[:, :, 2] = rs.uniform(0.2, 1.0, (people, 14))
    p[rs.rand(people, 14) < 0.15] = 0.0  # (0, 0, 0): a joint the person does not have
    p[-1, :, 0] += w * 0.6
    p[0, 3] = (np.nan, 10.0, 0.9)  # never drawn
    p[0, 4] = (10.0, 10.0, np.inf)
    p.setflags(write=False)
    return p


STYLE = dict(edges=SKELETON, joint_radius=3.0, limb_radius=1.5, alpha=200, alpha_filled=90, palette=ID_COLORS, color="id")


def test_bgr24_pitched(gpu_caffe):
    s = _surface("bgr")
    want = _check(gpu_caffe, [s], _crowd()[None], **STYLE)
    changed = want[0].bufs[0] != s.bufs[0]
    assert changed.any() and not changed[:, 3 * W:].any()  # something was drawn, the padding is the sentinel still


@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_nv12_odd_frame_every_matrix_and_range(gpu_caffe, pair):
    s = _surface("nv12", pair=pair)
    want = _check(gpu_caffe, [s], _crowd()[None], **STYLE)
    assert (want[0].bufs[0] != s.bufs[0]).any() and (want[0].bufs[1] != s.bufs[1]).any()
    # the frame's last chroma row and column belong to blocks of 2 and 1 pixels: they were drawn into
    uv0, uv1 = s.views()[1], want[0].views()[1]
    assert (uv0[-1] != uv1[-1]).any() and (uv0[:, -1] != uv1[:, -1]).any()


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_order_is_kept_where_alpha_shows_it(gpu_caffe, fmt):
    """Three people on top of each other at alpha = 96: reversing them changes the bytes, in the restatement and on the device alike."""
    one = np.zeros((14, 3))
    one[:, 0], one[:, 1], one[:, 2] = np.linspace(8, 84, 14), np.linspace(60, 9, 14), 1.0
    people = np.stack([one, one + (1.25, 0.5, 0), one + (2.5, 1.0, 0)])[None]
    kw = dict(STYLE, alpha=96, joint_radius=5.0, limb_radius=3.0)
    s = _surface(fmt)
    a = _check(gpu_caffe, [s], people, **kw)
    b = _check(gpu_caffe, [s], people[:, ::-1], **kw)
    assert not _same(a, b)
    assert not _same(_on_device(gpu_caffe, [s], people, **kw), _on_device(gpu_caffe, [s], people[:, ::-1], **kw))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_limbs_far_out_of_the_frame_take_the_clamp_and_the_guard(gpu_caffe, fmt):
    """64 x 256: one limb whose ends lie about 30 000 px outside on either side, one with an end beyond the clamp at 32 768 px."""
    h, w = 64, 256
    people = np.zeros((1, 2, 4, 3))
    people[0, 0] = [(-29950.3, -7311.7, 1), (30211.9, 7402.2, 1), (20.0, -31000.0, 1), (31.0, 52000.0, 1)]
    people[0, 1] = [(-50000.0, 12.5, 1), (200.0, 40.0, 1), (1e12, -1e12, 1), (90.0, 33.0, 1)]
    stats = {}
    s = _surface(fmt, h, w)
    want = _check(gpu_caffe, [s], people, stats=stats, edges=((0, 1), (2, 3)), joint_radius=2.0, limb_radius=2.5, alpha=256, palette=ID_COLORS)
    print("%d pixel tests of the restatement took the guard" % stats["guard"])
    assert stats["guard"] > 0 and (want[0].bufs[0] != s.bufs[0]).any()
    assert DR.snap(1e12) == 1 << 19 and DR.snap(-50000.0) == -(1 << 19)


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_more_primitives_over_one_tile_than_a_chunk(gpu_caffe, fmt):
    """People stacked inside ONE tile until people x (J + n_edges) > 2 chunks; only the last of them is opaque."""
    tile_w, tile_h, chunk = gpu_caffe.draw_limits()
    assert (tile_w, tile_h) == (32, 32), "the scene below is laid out for 32 x 32 tiles"
    count = 2 * chunk // (14 + len(SKELETON)) + 1
    assert count * (14 + len(SKELETON)) > 2 * chunk
    rs = np.random.RandomState(9)
    people = np.ones((1, count, 14, 3))
    people[0, :, :, 0] = rs.uniform(tile_w + 4, 2 * tile_w - 4, (count, 14))  # tile (1, 1), radii included
    people[0, :, :, 1] = rs.uniform(tile_h + 4, 2 * tile_h - 4, (count, 14))
    cand = np.full((1, count, 14), -2, np.int32)
    cand[0, -1] = 0
    s = _surface(fmt)
    want = _check(gpu_caffe, [s], people, cand=cand, **dict(STYLE, alpha=256, alpha_filled=70))
    lo, hi = want[0].copy(), s.copy()
    for v, u in zip(lo.views(), hi.views()):  # nothing outside tile (1, 1) changed
        sel = np.ones(v.shape[:2], bool)
        if v.shape[:2] == (H, W):
            sel[tile_h:2 * tile_h, tile_w:2 * tile_w] = False
        else:
            sel[tile_h // 2:tile_h, tile_w // 2:tile_w] = False
        assert np.array_equal(v[sel], u[sel])


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("color", ["id", "joint"])
def test_three_frames_with_ids_and_cand(gpu_caffe, fmt, color):
    """nb = 3 with n_people = (2, 0, 5): ids with -1 (the untracked colour), cand with -2 and -3 (alpha_filled), both colour modes."""
    people = np.stack([_crowd(21), _crowd(22), _crowd(23)])
    n = np.array([2, 0, 5], np.int32)
    ids = np.array([[7, -1, 0, 0, 0], [1, 2, 3, 4, 5], [12, 3, -1, 40000000000, 6]], np.int64)
    cand = np.random.RandomState(4).randint(-3, 4, (3, 5, 14)).astype(np.int32)
    assert (cand == -2).any() and (cand == -3).any()
    surfaces = [_surface(fmt, seed=30 + b, pair=("bt709", "full")) for b in range(3)]
    kw = dict(STYLE, color=color, palette=ID_COLORS if color == "id" else JOINT_COLORS, untracked=(9, 200, 120), min_score=0.3)
    want = _check(gpu_caffe, surfaces, people, n_people=n, ids=ids, cand=cand, **kw)
    assert not _same(want[:1], surfaces[:1]) and _same(want[1:2], surfaces[1:2]) and not _same(want[2:], surfaces[2:])


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_nobody_to_draw_leaves_every_byte(gpu_caffe, fmt):
    surfaces = [_surface(fmt, seed=40), _surface(fmt, seed=41)]
    people = np.stack([_crowd(21), _crowd(22)])
    for where in (_on_host, _on_device):
        assert _same(where(gpu_caffe, surfaces, people, n_people=[0, 0], **STYLE), surfaces)
        # people there, nothing to draw of them: both radii 0, every score at or below min_score, everybody outside the frame
        assert _same(where(gpu_caffe, surfaces, people, **dict(STYLE, joint_radius=0.0, limb_radius=0.0)), surfaces)
        assert _same(where(gpu_caffe, surfaces, people, **dict(STYLE, min_score=1.0)), surfaces)
        assert _same(where(gpu_caffe, surfaces, people + (5000.0, 0.0, 0.0), **STYLE), surfaces)


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_host_and_device_frames_agree_and_runs_repeat(gpu_caffe, fmt):
    s = _surface(fmt, seed=50)
    people = _crowd(24, 8)[None]
    host, dev = _on_host(gpu_caffe, [s], people, **STYLE), _on_device(gpu_caffe, [s], people, **STYLE)
    assert _same(host, dev) and not _same(host, [s])
    assert _same(_on_device(gpu_caffe, [s], people, **STYLE), dev) and _same(_on_host(gpu_caffe, [s], people, **STYLE), host)
    # a bare array is wrapped like Frame.bgr and drawn in place; a caller's stream is taken
    if fmt == "bgr":
        import torch

        img = np.ascontiguousarray(s.views()[0])
        gpu_caffe.draw_people(img, people[0], **STYLE)
        assert np.array_equal(img, host[0].views()[0])
        t = [torch.from_numpy(b).cuda() for b in s.bufs]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        gpu_caffe.draw_people(s.device_frame(gpu_caffe, t), people[0], stream=st.cuda_stream, **STYLE)
        assert np.array_equal(t[0].cpu().numpy(), dev[0].bufs[0])


# ---- pose.track_people(draw=) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flight", [dict(), dict(depth=2, batch=2)], ids=["synchronous", "depth2-batch2"])
def test_track_people_draws_what_it_yields(gpu_caffe, synth152, flight):
    """Three synthetic frames: (people, ids) are what they are without `draw`, and every frame is the restatement applied to the people
    that were yielded for it (the assembly alone fills and bridges nothing, so every primitive is at `alpha`)."""
    import os

    import people_ref as R
    from deepcut_tools import deepercut_prototxt
    from pose import track_people

    old = os.environ.get("DC_AUTOTUNE")
    os.environ["DC_AUTOTUNE"] = "0"  # the cost model's tiles: nothing is timed
    try:
        h, w = 200, 264
        rs = np.random.RandomState(5)
        stats = (R.all_pairs_edges(), rs.randn(182, 2) * 15, rs.uniform(4, 30, (182, 2)))
        akw = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
        tkw = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1)
        img = np.random.RandomState(4).randint(0, 256, (h - 3, w - 5, 3)).astype(np.uint8)
        clean = [np.ascontiguousarray(np.roll(img, 8 * k, axis=1)) for k in range(3)]
        net = gpu_caffe.Net(deepercut_prototxt(152, h, w), synth152[0], gpu_caffe.TEST, from_text=True)
        style = dict(alpha=160, joint_radius=3.0, limb_radius=1.5, palette=ID_COLORS)
        plain = list(track_people([f.copy() for f in clean], None, None, stats, tracker=gpu_caffe.Tracker(n_joints=14, **tkw), net=net,
                                  **dict(akw, **flight)))
        frames = [f.copy() for f in clean]
        drawn = list(track_people(frames, None, None, stats, tracker=gpu_caffe.Tracker(n_joints=14, **tkw), net=net, draw=style,
                                  **dict(akw, **flight)))
    finally:
        if old is None:
            del os.environ["DC_AUTOTUNE"]
        else:
            os.environ["DC_AUTOTUNE"] = old
    assert len(plain) == len(drawn) == 3 and sum(len(p) for p, _ in drawn) > 0
    for k, ((p0, i0), (p1, i1)) in enumerate(zip(plain, drawn)):
        assert np.array_equal(p0, p1) and np.array_equal(i0, i1), k
        want = clean[k].copy()
        DR.draw_bgr(want, DR.primitives(p1, ids=i1, edges=SKELETON, color="id", **style))
        assert np.array_equal(frames[k], want), k
        assert len(p1) == 0 or not np.array_equal(want, clean[k]), k


# ---- pose_demo.py --skeleton -------------------------------------------------------------------------------------------------------------
def test_demo_skeleton_overlay_is_the_restatement(synth152, tmp_path):
    """The demo's command line with --skeleton: the PNG it writes is the restatement applied to the pose it saved, by-joint colours."""
    import os
    import subprocess
    import sys

    from PIL import Image

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "deepcut-cnn_amd", "python", "pose", "pose_demo.py")
    rgb = np.random.RandomState(8).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(str(tmp_path / "img.png"))
    out = str(tmp_path / "pose.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "deepcut-cnn_amd", "python"), root]))
    r = subprocess.run([sys.executable, demo, str(tmp_path / "img.png"), "--model_bin", synth152[0], "--out_name", out, "--skeleton"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    pose = np.load(out, allow_pickle=True)["pose"].astype(np.float64)
    want = np.ascontiguousarray(rgb[:, :, ::-1])
    DR.draw_bgr(want, DR.primitives(pose[:3].T[None], edges=SKELETON, color="joint", palette=JOINT_COLORS, joint_radius=8.0, limb_radius=3.0,
                                    alpha=256))
    got = np.asarray(Image.open(out + "_vis.png"))
    assert np.array_equal(got[:, :, ::-1], want) and not np.array_equal(got, rgb)
