"""CPU: the per-(member, image) reflected column of dc_group_decode_boxes as restated in tests/boxfuse_ref.py (its properties), and the
host side of dc_group_decode_pose, dc_group_forward_boxes_mirrored, dc_group_decode_boxes and of estimate_pose / estimate_poses
(fuse=True, flip=True): what they refuse before any device work.  The device side is tests/test_gpu_boxfuse.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn keeps the best single scale (estimate_pose.py:119-126), fuses no maps and mirrors
nothing; the rule is this project's own (include/deepcut_hip.h)."""
import ctypes as C

import numpy as np
import pytest

import boxfuse_ref as BF
import caffe
import caffe.pycaffe as pc
import flip_ref as FL
from deepcut_tools import deepercut_prototxt

EINVAL, ESHAPE, ENOCPU = -1, -3, -6  # include/deepcut_hip.h
PI = FL.MIRROR_MPII14


def _random_maps(rs, nb, shapes):
    return [(rs.rand(nb, 14, h, w), rs.randn(nb, 28, h, w)) for h, w in shapes]


def test_every_box_of_one_width_is_the_image_rule():
    """ws the same for every image of a member, (image_width - 1) * the member's scale: flip_ref.fuse at that image_width, exactly."""
    rs = np.random.RandomState(3)
    scales, mirror, width = (1.0, 0.7, 1.0, 0.7), (0, 0, 1, 1), 117
    maps = _random_maps(rs, 3, [(11, 15), (8, 11), (11, 15), (8, 11)])
    ws = [[float(width - 1) * s] * 3 for s in scales]
    for base in (0, 1):
        got, a = BF.fuse(maps, scales, base, mirror, ws, PI)
        want, wa = FL.fuse([m + (None,) for m in maps], scales, base, mirror, width, PI)
        for k in range(2):
            assert np.array_equal(got[k], want[k]) and np.array_equal(a[k], wa[k])
    # and ws is read per image: another width for image 1 alone changes image 1 alone
    ws2 = [list(r) for r in ws]
    ws2[2][1], ws2[3][1] = 90.0 * 1.0, 90.0 * 0.7
    other, _ = BF.fuse(maps, scales, 0, mirror, ws2, PI)
    ref, _ = BF.fuse(maps, scales, 0, mirror, ws, PI)
    assert np.array_equal(other[0][[0, 2]], ref[0][[0, 2]]) and not np.array_equal(other[0][1], ref[0][1])
    assert np.array_equal(other[1][[0, 2]], ref[1][[0, 2]]) and not np.array_equal(other[1][1], ref[1][1])


def test_a_single_unmirrored_member_fuses_to_itself():
    rs = np.random.RandomState(4)
    maps = _random_maps(rs, 2, [(9, 13)])
    got, a = BF.fuse(maps, (0.8,), 0, (0,), [[0.0, 0.0]], PI)
    for k in range(2):
        assert np.array_equal(got[k], maps[0][k]) and np.array_equal(a[k], np.abs(maps[0][k]))


@pytest.mark.parametrize("scales,mirror", [((1.0, 1.0), (0, 1)), ((1.0, 0.5, 1.0, 0.5), (0, 0, 1, 1))])
def test_a_linear_field_and_its_hand_flipped_copy_fuse_to_the_plain_field(scales, mirror):
    """A field linear in the image point, rendered into every member at its own scale; a mirrored member holds it hand-flipped about
    every box's OWN width (three odd, different widths, so no reflected column is cell-aligned), relabelled by pi and with the x
    components negated.  Wherever no member's sample is clamped, the fusion returns the base member's own field: the bilinear sample of
    a linear field is exact, and the reflection of the reflection is the identity only if ws is the box's own."""
    rs = np.random.RandomState(6)
    widths = (61, 91, 31)
    nb, nj = len(widths), 14
    shapes = {1.0: (12, 14), 0.5: (6, 7)}
    p0, px, py = rs.rand(nj), rs.randn(nj) * 1e-3, rs.randn(nj) * 1e-3
    l0, lx, ly = rs.randn(2 * nj), rs.randn(2 * nj) * 1e-2, rs.randn(2 * nj) * 1e-2
    pi = np.asarray(PI)
    src_loc = 2 * pi[np.arange(2 * nj) // 2] + np.arange(2 * nj) % 2
    maps = []
    for s, flipped in zip(scales, mirror):
        h, w = shapes[s]
        y = ((8.0 * np.arange(h) + 4.0) / s)[None, None, :, None]
        prob, loc = np.zeros((nb, nj, h, w)), np.zeros((nb, 2 * nj, h, w))
        for b, cw in enumerate(widths):
            x = (8.0 * np.arange(w) + 4.0) / s
            if flipped:
                x = (cw - 1) - x  # the crop's own point behind column c of the flipped crop
            x = x[None, None, None, :]
            pr = (p0[None, :, None, None] + px[None, :, None, None] * x + py[None, :, None, None] * y)[0]
            lo = ((l0[None, :, None, None] + lx[None, :, None, None] * x + ly[None, :, None, None] * y) * s)[0]  # loc_pred is in the member's units
            if flipped:
                pr, lo = pr[pi], lo[src_loc]  # (pi is an involution: channel j of the mirror holds joint pi[j] of the scene)
                lo[0::2] = -lo[0::2]
            prob[b], loc[b] = pr, lo
        maps.append((prob, loc))
    ws = [[float(cw - 1) * s for cw in widths] for s in scales]
    fused, a = BF.fuse(maps, scales, 0, mirror, ws, PI)
    hb, wb = shapes[1.0]
    for b, cw in enumerate(widths):
        ok = np.ones(wb, bool)
        for m, s in enumerate(scales):
            q, c = s / scales[0], np.arange(wb)
            u = (((ws[m][b] - (8.0 * c + 4.0) * q) - 4.0) / 8.0) if mirror[m] else (((8.0 * c + 4.0) * q - 4.0) / 8.0)
            ok &= (u >= 0) & (u <= shapes[s][1] - 1)
        rows = slice(1, hb - 2)  # (the half-scale member's rows clamp at both ends)
        assert ok.sum() >= 2, (cw, ok)
        for k in range(2):
            err = np.abs(fused[k][b][:, rows][:, :, ok] - maps[0][k][b][:, rows][:, :, ok]).max()
            assert err <= 1e-11 * max(1.0, np.abs(maps[0][k]).max()), (cw, k, err)
    # the widths matter: every box reflected about box 0's width fuses to something else
    wrong, _ = BF.fuse(maps, scales, 0, mirror, [[r[0]] * nb for r in ws], PI)
    assert np.abs(wrong[1][1] - fused[1][1]).max() > 1e-2


def test_box_ws_is_the_crop_width_and_the_scale_the_member_ran_the_box_at():
    ws = BF.box_ws([(3, 5, 64, 90), (40, 0, 131, 96)], [1.0, 0.8], (1.0, 0.7))
    assert ws.shape == (2, 2) and ws[0, 0] == 60.0 and ws[1, 1] == 90.0 * (0.8 * 0.7) and ws[0, 1] == 90.0 * (0.8 * 1.0)


# ---- the entry points without a device ------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _err():
    return (pc._lib.dc_last_error() or b"").decode()


class _Calls(object):
    """The new entry points on one group of four through the raw C ABI, with arguments that are right unless a test replaces one."""

    def __init__(self):
        a = caffe.Net(deepercut_prototxt(101, 64, 64), caffe.TEST, from_text=True)
        self.g = g = caffe.NetGroup([a] + [a.clone() for _ in range(3)])
        n, j = g.nets[0].blobs["prob"].shape[:2]
        self.pose = np.zeros((n, 5, j))
        self.sc = np.ascontiguousarray([0.7, 1.0, 0.7, 1.0], np.float64)

    def mirror(self, flags=(0, 0, 1, 1), width=64, pi=PI):
        self.keep = (None if flags is None else np.ascontiguousarray(flags, np.int32), None if pi is None else np.ascontiguousarray(pi, np.int32))
        return pc.FuseMirror(None if self.keep[0] is None else self.keep[0].ctypes.data, width,
                             None if self.keep[1] is None else self.keep[1].ctypes.data, 0, None)

    def decode_pose(self, fm, base=1, scales="own", pose="own"):
        return pc._lib.dc_group_decode_pose(self.g._h, _vp(self.sc) if isinstance(scales, str) else scales, base, None if fm is None else C.byref(fm),
                                            _vp(self.pose) if isinstance(pose, str) else pose, 0, None)

    def decode_boxes(self, fm, base=1, scales="own"):
        return pc._lib.dc_group_decode_boxes(self.g._h, _vp(self.sc) if isinstance(scales, str) else scales, base, None if fm is None else C.byref(fm),
                                             None, None, _vp(self.pose), 0, None)


def test_decode_pose_refuses_what_detect_parts_refuses_before_any_device_work():
    caffe.set_mode_cpu()
    k = _Calls()
    swapped, far = list(PI), list(PI)
    swapped[0], swapped[1] = 4, 4
    far[3] = 14
    call = k.decode_pose
    assert call(k.mirror()) == ENOCPU and "CPU mode" in _err()
    assert call(k.mirror(), pose=None) == EINVAL and "pose" in _err()
    assert call(k.mirror(), scales=None) == EINVAL and "null scales" in _err()
    bad = np.ascontiguousarray([0.7, -1.0, 0.7, 1.0])
    assert call(k.mirror(), scales=_vp(bad)) == EINVAL and "scale of member 1" in _err()
    assert call(k.mirror(), base=4) == EINVAL and "base 4 is outside" in _err()
    assert call(k.mirror(width=0)) == EINVAL and "image_width" in _err()
    assert call(k.mirror(pi=None)) == EINVAL and "joint_mirror" in _err()
    assert call(k.mirror(pi=far)) == EINVAL and "joint_mirror[3]" in _err()
    assert call(k.mirror(pi=swapped)) == EINVAL and "involution" in _err()
    assert call(k.mirror(flags=(0, 1, 1, 0))) == EINVAL and "base" in _err() and "mirrored" in _err()
    # the order is detect_parts' own: the scales before the table
    assert call(k.mirror(width=0), base=4) == EINVAL and "base 4 is outside" in _err()
    # no mirrored member, or no table: nothing of it is read
    assert call(k.mirror(flags=(0, 0, 0, 0), width=0, pi=None)) == ENOCPU
    assert call(k.mirror(flags=None, width=0, pi=None)) == ENOCPU
    assert call(None) == ENOCPU and "decode_pose" in _err()


def test_decode_boxes_refuses_before_any_device_work():
    caffe.set_mode_cpu()
    k = _Calls()
    swapped, far = list(PI), list(PI)
    swapped[0], swapped[1] = 4, 4
    far[3] = 14
    call = k.decode_boxes
    assert call(None, scales=None) == EINVAL and "null scales" in _err()
    assert call(None, base=-1) == EINVAL and "base -1 is outside" in _err()
    assert call(k.mirror(pi=None)) == EINVAL and "joint_mirror" in _err()
    assert call(k.mirror(pi=far)) == EINVAL and "joint_mirror[3]" in _err()
    assert call(k.mirror(pi=swapped)) == EINVAL and "involution" in _err()
    assert call(k.mirror(flags=(0, 1, 1, 0))) == EINVAL and "base" in _err() and "mirrored" in _err()
    # image_width is not read: a table that is right otherwise gets as far as the members' own record of their last box batch
    for width in (0, -3, 64):
        assert call(k.mirror(width=width)) == EINVAL and "member 2" in _err() and "last box batch was not mirrored" in _err(), width
    # nobody marked: the members hold no boxes yet
    for fm in (None, k.mirror(flags=(0, 0, 0, 0), pi=None), k.mirror(flags=None, pi=None)):
        assert call(fm) == EINVAL and "no boxes" in _err() and "forward_boxes" in _err()


def test_forward_boxes_mirrored_checks_the_boxes_of_every_member_first():
    caffe.set_mode_cpu()
    k = _Calls()
    img = np.zeros((96, 131, 3), np.uint8)
    pyr = (C.c_double * 4)(1.0, 0.7, 1.0, 0.7)
    flags = np.ascontiguousarray([0, 0, 1, 1], np.int32)

    def call(boxes, canvas=(96, 96), mirror=flags, n=None):
        b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
        s = np.ones(b.shape[0])
        return pc._lib.dc_group_forward_boxes_mirrored(k.g._h, _vp(img), 96, 131, 0, _vp(b), _vp(s), b.shape[0] if n is None else n, pyr, canvas[0],
                                                       canvas[1], _vp(mirror), None, None, None, None)

    good = [(3, 5, 64, 90), (70, 20, 101, 77)]
    assert call(good) == ENOCPU and "CPU mode" in _err()
    assert call(good, mirror=None) == ENOCPU
    assert call(good, n=0) == 0
    assert call([(3, 5, 64, 90), (9, 9, 9, 20)]) == EINVAL and "box 1" in _err() and "empty" in _err()
    assert call([(120, 0, 132, 10)]) == EINVAL and "outside" in _err()
    assert call(good, canvas=(96, 60)) == EINVAL and "multiple of 8" in _err()
    assert call([(0, 0, 131, 96)], canvas=(64, 64)) == EINVAL and "needs a" in _err() and "group member 0" in _err()


def test_the_python_methods_check_the_lengths():
    caffe.set_mode_cpu()
    k = _Calls()
    g, sc = k.g, [0.7, 1.0, 0.7, 1.0]
    img = np.zeros((96, 131, 3), np.uint8)
    with pytest.raises(ValueError):
        g.decode_pose(sc[:3], 1)
    with pytest.raises(ValueError):
        g.decode_pose(sc, 1, mirror=[0, 0, 1])
    with pytest.raises(ValueError):
        g.decode_pose(sc, 1, mirror=[0, 0, 1, 1], image_width=64, joint_mirror=PI[:-1])
    with pytest.raises(ValueError):
        g.decode_boxes(sc, 1, mirror=[0, 1])
    with pytest.raises(ValueError):
        g.forward_boxes(img, [(3, 5, 64, 90)], sc, mirror=[0, 1])
    with pytest.raises(caffe.DeepcutError) as e:
        g.decode_pose(sc, 1, mirror=[0, 0, 1, 1], image_width=64, joint_mirror=PI)
    assert e.value.code == ENOCPU
    with pytest.raises(caffe.DeepcutError) as e:
        g.decode_pose(sc, 1)
    assert e.value.code == ENOCPU
    with pytest.raises(caffe.DeepcutError) as e:
        g.decode_boxes(sc, 1, mirror=[0, 0, 1, 1], joint_mirror=PI)
    assert e.value.code == EINVAL and "member 2" in str(e.value)
    for kw in (dict(mirror=[0, 0, 1, 1]), dict(mirror=[0, 0, 0, 0]), dict()):
        with pytest.raises(caffe.DeepcutError) as e:
            g.forward_boxes(img, [(3, 5, 64, 90)], sc, **kw)
        assert e.value.code == ENOCPU


class _NoNet(object):
    """A net that must not be touched: every attribute access fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the net was touched (%s) before the arguments were checked" % name)


def test_estimate_pose_and_estimate_poses_check_the_fusion_arguments_without_a_net():
    from pose.estimate_pose import estimate_pose, estimate_poses

    img = np.zeros((64, 64, 3), np.uint8)
    net = _NoNet()
    for kw in (dict(fuse=True), dict(flip=True)):
        for bad in (dict(tiling="exact"), dict(on_device=False), dict(grouped=False)):
            with pytest.raises(ValueError) as e:
                estimate_pose(img, None, None, scales=[0.7, 1.0], net=net, **dict(kw, **bad))
            assert "fuse" in str(e.value), (kw, bad)
    swapped = list(PI)
    swapped[0], swapped[1] = 4, 4
    for fn, args in ((estimate_pose, (img, None, None)), (estimate_poses, (img, [(3, 5, 60, 60)], None, None))):
        with pytest.raises(ValueError) as e:
            fn(*args, scales=[0.7, 1.0], net=net, flip=True, joint_mirror=swapped)
        assert "involution" in str(e.value)
        with pytest.raises(ValueError) as e:
            fn(*args, scales=[0.7, 1.0], net=net, flip=True, joint_mirror=None)
        assert "joint_mirror" in str(e.value)
        with pytest.raises(ValueError) as e:
            fn(*args, scales=[0.7, 1.0], net=net, flip=True, base=2)  # member 2 is the mirror of member 0
        assert "plain" in str(e.value)
        with pytest.raises(ValueError) as e:
            fn(*args, scales=[0.7, 1.0], net=net, fuse=True, base=2)
        assert "base" in str(e.value)
        with pytest.raises(ValueError) as e:
            fn(*args, scales=[], net=net, fuse=True)
        assert "scales" in str(e.value)
