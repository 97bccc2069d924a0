"""GPU: `caffe.redact_people` (dc_redact_people) against the numpy restatement of its rule in tests/redact_ref.py, BYTE FOR BYTE, the pitch
padding (pre-filled with a sentinel) included — the rule is integer only, so there is no tolerance.  Host frames and device frames are
both compared whole-buffer, and `redacted` with them.

PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind; the rule is this project's own.

Shapes: 71 x 93 frames (odd both ways: partial tiles, partial blocks at every block size, chroma blocks of 2 and 1 pixels), a 150 x 170
frame for a head disc of 90 pixels radius (beyond the drawing rule's 64), a 40 x 40 frame with 71 primitives over one tile."""
import functools

import numpy as np
import pytest

import draw_ref as DR
import redact_ref as RR
from test_gpu_draw import ID_COLORS, PAIRS, SKELETON, _surface

pytestmark = pytest.mark.gpu

H, W = 71, 93
BLOCKS = (2, 4, 8, 16, 32)
HEAD = (12, 13)
GEOMETRY = dict(head=HEAD, edges=SKELETON, head_scale=0.75, body_scale=0.06, min_radius=4.0, max_radius=256.0)


# ---- the call on host and on device frames, and the restatement ------------------------------------------------------------------------
def _on_host(caffe, surfaces, people, calls=1, **kw):
    got = [s.copy() for s in surfaces]
    frames = [s.host_frame(caffe) for s in got]
    red = [caffe.redact_people(frames, people, **kw) for _ in range(calls)]
    return got, red[-1]


def _on_device(caffe, surfaces, people, calls=1, **kw):
    import torch

    tensors = [[torch.from_numpy(b).cuda() for b in s.bufs] for s in surfaces]
    torch.cuda.synchronize()
    frames = [s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)]
    red = [caffe.redact_people(frames, people, **kw) for _ in range(calls)]
    got = [s.copy() for s in surfaces]
    for g, t in zip(got, tensors):
        g.bufs = [x.cpu().numpy() for x in t]
    return got, red[-1]


def _apply(surface, prims, effect="mosaic", block=8, fill=(0, 0, 0)):
    """The restatement on one surface, in place -> the selected blocks."""
    v = surface.views()
    if len(v) == 1:
        return RR.redact_bgr(v[0], prims, effect, block, fill)
    return RR.redact_nv12(v[0], v[1], prims, surface.matrix, surface.range, effect, block, fill)


def _reference(surfaces, people, n_people=None, select=None, effect="mosaic", block=8, fill=(0, 0, 0), **geometry):
    """-> (the restatement's surfaces, redacted [nb, P], the blocks selected per frame)."""
    want, red, blocks = [s.copy() for s in surfaces], [], []
    for b, s in enumerate(want):
        prims, r = RR.primitives(people[b], None if n_people is None else n_people[b], None if select is None else select[b], **geometry)
        blocks.append(_apply(s, prims, effect, block, fill))
        red.append(r)
    return want, np.stack(red), blocks


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s.bufs, t.bufs))


def _assert_same(place, got, want):
    for b, (g, w_) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g.bufs, w_.bufs)):
            bad = np.argwhere(x != y)
            assert bad.size == 0, "%s frame %d plane %d: %d bytes differ, first at %s: got %d, want %d" % (
                place, b, k, len(bad), tuple(bad[0]), x[tuple(bad[0])], y[tuple(bad[0])])


def _check(caffe, surfaces, people, **kw):
    """Host and device frames, and `redacted`, against the restatement; -> (the restatement's surfaces, redacted, blocks)."""
    want, red, blocks = _reference(surfaces, people, **kw)
    for place, run in (("host", _on_host), ("device", _on_device)):
        got, r = run(caffe, surfaces, people, **kw)
        _assert_same(place, got, want)
        assert r.dtype == np.int32 and np.array_equal(r, red), (place, r, red)
    return want, red, blocks


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _person(neck=None, top=None, **joints):
    p = np.zeros((14, 3))
    if neck is not None:
        p[12] = (neck[0], neck[1], 0.9)
    if top is not None:
        p[13] = (top[0], top[1], 0.8)
    for j, v in joints.items():
        p[int(j[1:])] = (v[0], v[1], 0.7)
    return p


@functools.lru_cache(maxsize=None)
def _three_heads():
    """A head that straddles the right and the bottom edge (and the tile border at y = 64), one wholly outside, one without its head top;
    coordinates at odd sixteenths and on ties of the 1/16 grid."""
    p = np.stack([_person((84.28125, 69.09375), (91.71875, 61.40625)), _person((200.0, 180.0), (204.0, 170.0)), _person((30.0, 30.0), None)])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _crowd(seed=3, count=4, h=H, w=W, spread=18.0):
    """People scattered over the frame, joints within `spread` px of the person's centre; joints missing here and there."""
    rs = np.random.RandomState(seed)
    p = np.zeros((count, 14, 3))
    centre = np.stack([rs.uniform(0, w, count), rs.uniform(0, h, count)], 1)
    p[:, :, :2] = np.round((centre[:, None, :] + rs.uniform(-spread, spread, (count, 14, 2))) * 32) / 32
    p[:, :, 2] = rs.uniform(0.2, 1.0, (count, 14))
    p[rs.rand(count, 14) < 0.15] = 0.0
    p.setflags(write=False)
    return p


# ---- 1. the base grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_heads_mosaic_on_an_odd_frame_at_every_block_size(gpu_caffe, fmt, block):
    s = _surface(fmt)
    want, red, blocks = _check(gpu_caffe, [s], _three_heads()[None], region="head", block=block, **dict(GEOMETRY, head_scale=1.5))
    assert red.tolist() == [[1, 1, 0]]  # made though wholly outside; no head top: not redacted, and the caller can see it
    # the blocks reach the frame's last (partial) block row and column, and both sides of the tile border at y = 64
    by, bx = zip(*blocks[0])
    assert max(by) == (H - 1) // block and max(bx) == (W - 1) // block and min(by) * block < 64
    assert not _same(want, [s])
    if fmt == "nv12" and block > 2:
        uv0, uv1 = s.views()[1], want[0].views()[1]
        assert (uv0[-1] != uv1[-1]).any() and (uv0[:, -1] != uv1[:, -1]).any()  # chroma blocks of 2 and 1 pixels were averaged


# ---- 2. fill ---------------------------------------------------------------------------------------------------------------------------
def test_fill_bgr24(gpu_caffe):
    s = _surface("bgr")
    want, _red, blocks = _check(gpu_caffe, [s], _crowd()[None], region="head", effect="fill", fill=(200, 30, 90), block=8, **GEOMETRY)
    by, bx = sorted(blocks[0])[0]
    assert want[0].views()[0][by * 8, bx * 8].tolist() == [90, 30, 200]


@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_fill_nv12_every_matrix_and_range(gpu_caffe, pair):
    s = _surface("nv12", pair=pair)
    want, _red, blocks = _check(gpu_caffe, [s], _crowd()[None], region="head", effect="fill", fill=(200, 30, 90), block=8, **GEOMETRY)
    by, bx = sorted(blocks[0])[0]
    y, uv = want[0].views()
    assert (int(y[by * 8, bx * 8]),) + tuple(int(v) for v in uv[by * 4, bx * 4]) == RR.forward_colour((200, 30, 90), *pair)


# ---- 3. body and head_or_body ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", ["body", "head_or_body"])
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_body_regions_with_the_mpii_skeleton(gpu_caffe, fmt, region):
    """Four people and a fifth with a single held joint (s16 = 0: its radius is min_radius)."""
    people = np.concatenate([_crowd(), _person(j4=(47.5, 8.25))[None]])[None]
    s = _surface(fmt)
    want, red, _blocks = _check(gpu_caffe, [s], people, region=region, block=4, **dict(GEOMETRY, body_scale=0.11, min_radius=2.5))
    assert red.tolist() == [[1] * 5] and not _same(want, [s])
    lone, _ = RR.primitives(people[0, 4:], region=region, **dict(GEOMETRY, min_radius=2.5))
    assert lone == [dict(a=(760, 132), b=(760, 132), r16=40, capsule=False)]
    # the two regions differ where a person has a head pair
    other, _, _ = _reference([s], people, region="body" if region == "head_or_body" else "head_or_body", block=4,
                             **dict(GEOMETRY, body_scale=0.11, min_radius=2.5))
    assert not _same(other, want)


# ---- 4. a head disc larger than the drawing rule's radii -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_head_disc_of_ninety_pixels(gpu_caffe, fmt):
    h, w = 150, 170
    people = _person((85.0, 149.5), (85.0, -0.5))[None, None]  # 150 px apart
    (disc,), _ = RR.primitives(people[0], region="head", **dict(GEOMETRY, head_scale=0.6))
    assert disc["r16"] == 90 * 16 > 1024
    s = _surface(fmt, h, w)
    want, red, blocks = _check(gpu_caffe, [s], people, region="head", block=8, **dict(GEOMETRY, head_scale=0.6))
    assert red.tolist() == [[1]]
    # the disc reaches the top and the bottom edge, not the corners
    assert (0, 10) in blocks[0] and ((h - 1) // 8, 10) in blocks[0] and (0, 0) not in blocks[0] and ((h - 1) // 8, (w - 1) // 8) not in blocks[0]


# ---- 5. the staging loop's second trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_more_primitives_over_one_tile_than_a_chunk(gpu_caffe, fmt):
    """40 x 40: 70 small heads stacked in the top left corner and one in the bottom right of the SAME tile, the 71st primitive — its blocks
    are covered by nothing of the first chunk."""
    tile_w, tile_h, chunk = gpu_caffe.draw_limits()
    assert (tile_w, tile_h) == (32, 32) and 70 >= chunk, "the scene below is laid out for 32 x 32 tiles and a chunk of at most 70"
    rs = np.random.RandomState(12)
    people = np.stack([_person(tuple(rs.uniform(3, 9, 2)), None) for _ in range(71)])
    people[:, 13] = people[:, 12] + (0.0, -3.0, 0.0)
    people[70, 12], people[70, 13] = (27.0, 28.5, 1.0), (27.0, 25.5, 1.0)
    kw = dict(region="head", block=4, **dict(GEOMETRY, head_scale=1.0, min_radius=1.0))
    s = _surface(fmt, 40, 40)
    want, red, blocks = _check(gpu_caffe, [s], people[None], **kw)
    assert red.tolist() == [[1] * 71]
    _, _, first = _reference([s], people[None, :70], **kw)
    late = blocks[0] - first[0]
    assert late and all(4 * by >= 20 and 4 * bx >= 20 and 4 * by + 3 < tile_h and 4 * bx + 3 < tile_w for by, bx in late)


# ---- 6. a batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_three_frames_with_a_select_mask(gpu_caffe, fmt):
    """nb = 3 with n_people = (0, 1, 5), P = 6 > max(n_people), a mask that drops some of them."""
    people = np.stack([_crowd(21, 6), _crowd(22, 6), _crowd(23, 6)])
    n = np.array([0, 1, 5], np.int32)
    select = np.array([[1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0], [0, 1, 1, 0, 1, 1]], np.uint8)
    surfaces = [_surface(fmt, seed=30 + b, pair=("bt709", "full")) for b in range(3)]
    want, red, _blocks = _check(gpu_caffe, surfaces, people, n_people=n, select=select, region="head_or_body", block=16, **GEOMETRY)
    assert red.tolist() == [[0] * 6, [1, 0, 0, 0, 0, 0], [0, 1, 1, 0, 1, 0]]
    assert _same(want[:1], surfaces[:1]) and not _same(want[1:2], surfaces[1:2]) and not _same(want[2:], surfaces[2:])
    # only_ids / keep_ids give the same mask from ids
    ids = np.array([[0, 1, 2, 3, 4, 5], [7, 8, 9, 10, 11, 12], [20, 21, 22, 23, 24, 25]], np.int64)
    for kw in (dict(only_ids=[7, 21, 22, 24, 25, 99]), dict(keep_ids=[0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 20, 23])):
        got, r = _on_device(gpu_caffe, surfaces, people, n_people=n, ids=ids, region="head_or_body", block=16, **dict(GEOMETRY, **kw))
        _assert_same("device, %s" % sorted(kw), got, want)
        assert np.array_equal(r, red)


# ---- 7. nothing selected ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_nothing_selected_leaves_every_byte(gpu_caffe, fmt):
    surfaces = [_surface(fmt, seed=40), _surface(fmt, seed=41)]
    people = np.stack([_crowd(21), _crowd(22)])
    kw = dict(region="body", block=8, **GEOMETRY)
    for where in (_on_host, _on_device):
        got, red = where(gpu_caffe, surfaces, people, select=np.zeros((2, 4), np.uint8), **kw)
        assert _same(got, surfaces) and not red.any()
        got, red = where(gpu_caffe, surfaces, people, n_people=[0, 0], **kw)
        assert _same(got, surfaces) and not red.any()
        got, red = where(gpu_caffe, surfaces, people + (5000.0, 0.0, 0.0), **kw)  # everybody outside the frame: made, and nothing to do
        assert _same(got, surfaces) and red.all()
        got, red = where(gpu_caffe, surfaces, people, **dict(kw, min_score=1.0))
        assert _same(got, surfaces) and not red.any()


# ---- 8. idempotence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [2, 32])
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_second_mosaic_call_changes_no_byte(gpu_caffe, fmt, block):
    s = _surface(fmt, seed=50)
    people = _crowd(24, 6)[None]
    kw = dict(region="body", block=block, **GEOMETRY)
    for where in (_on_host, _on_device):
        once, _ = where(gpu_caffe, [s], people, **kw)
        twice, _ = where(gpu_caffe, [s], people, calls=2, **kw)
        assert _same(once, twice) and not _same(once, [s])
    # a bare array is wrapped like Frame.bgr and redacted in place; one frame's [m, J, 3] gives redacted [m]; a caller's stream is taken
    if fmt == "bgr":
        import torch

        img = np.ascontiguousarray(s.views()[0])
        red = gpu_caffe.redact_people(img, people[0], **kw)
        assert red.shape == (6,) and np.array_equal(img, once[0].views()[0])
        t = [torch.from_numpy(b).cuda() for b in s.bufs]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        gpu_caffe.redact_people(s.device_frame(gpu_caffe, t), people[0], stream=st.cuda_stream, **kw)
        assert np.array_equal(t[0].cpu().numpy(), once[0].bufs[0])


# ---- pose_demo.py --redact -------------------------------------------------------------------------------------------------------------
def test_demo_redact_under_the_skeleton_is_the_restatement(synth152, tmp_path):
    """The demo's command line with --redact head --skeleton: the PNG it writes is the restatement of the redaction (the binding's
    defaults, the MPII head pair) and then of the overlay, applied to the pose it saved."""
    import os
    import subprocess
    import sys

    from PIL import Image

    from test_gpu_draw import JOINT_COLORS

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "deepcut-cnn_amd", "python", "pose", "pose_demo.py")
    rgb = np.random.RandomState(8).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(str(tmp_path / "img.png"))
    out = str(tmp_path / "pose.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "deepcut-cnn_amd", "python"), root]))
    r = subprocess.run([sys.executable, demo, str(tmp_path / "img.png"), "--model_bin", synth152[0], "--out_name", out, "--skeleton", "--redact",
                        "head"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    pose = np.load(out, allow_pickle=True)["pose"].astype(np.float64)
    want = np.ascontiguousarray(rgb[:, :, ::-1])
    prims, red = RR.primitives(pose[:3].T[None], region="head", **GEOMETRY)
    RR.redact_bgr(want, prims, "mosaic", 8)
    redacted = want.copy()
    DR.draw_bgr(want, DR.primitives(pose[:3].T[None], edges=SKELETON, color="joint", palette=JOINT_COLORS, joint_radius=8.0, limb_radius=3.0,
                                    alpha=256))
    got = np.asarray(Image.open(out + "_vis.png"))
    assert np.array_equal(got[:, :, ::-1], want)
    assert red.tolist() == [1] and not np.array_equal(redacted[:, :, ::-1], rgb)


# ---- 9. pose.track_people(redact=, draw=) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flight", [dict(), dict(depth=2, batch=2)], ids=["synchronous", "depth2-batch2"])
def test_track_people_redacts_and_then_draws_what_it_yields(gpu_caffe, synth152, flight):
    """Three synthetic frames: (people, ids) are what they are without `redact`, and every frame is the restatement of the redaction and
    then the restatement of the drawing, in that order, applied to the people that were yielded for it."""
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
        geometry = dict(head_scale=0.75, body_scale=0.06, min_radius=4.0, max_radius=256.0)
        redact = dict(region="head_or_body", block=8, **geometry)
        plain = list(track_people([f.copy() for f in clean], None, None, stats, tracker=gpu_caffe.Tracker(n_joints=14, **tkw), net=net,
                                  **dict(akw, **flight)))
        frames = [f.copy() for f in clean]
        both = list(track_people(frames, None, None, stats, tracker=gpu_caffe.Tracker(n_joints=14, **tkw), net=net, redact=redact, draw=style,
                                 **dict(akw, **flight)))
    finally:
        if old is None:
            del os.environ["DC_AUTOTUNE"]
        else:
            os.environ["DC_AUTOTUNE"] = old
    assert len(plain) == len(both) == 3 and sum(len(p) for p, _ in both) > 0
    for k, ((p0, i0), (p1, i1)) in enumerate(zip(plain, both)):
        assert np.array_equal(p0, p1) and np.array_equal(i0, i1), k
        want = clean[k].copy()
        prims, red = RR.primitives(p1, region="head_or_body", head=HEAD, edges=SKELETON, **geometry)
        RR.redact_bgr(want, prims, "mosaic", 8)
        redacted = want.copy()
        DR.draw_bgr(want, DR.primitives(p1, ids=i1, edges=SKELETON, color="id", **style))
        assert np.array_equal(frames[k], want), k
        assert len(p1) == 0 or (red.all() and not np.array_equal(redacted, clean[k]) and not np.array_equal(want, redacted)), k
