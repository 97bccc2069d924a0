"""CPU: the mirrored fusion rule of dc_group_fuse_maps_mirrored as restated in tests/flip_ref.py (its properties, and the planted
mirrored pyramid through the restated people assembly), and the host side of the dc_group_*_mirrored entries and of
estimate_people(flip=True): what they refuse before any device work.  The device side is tests/test_gpu_flip.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and mirrors nothing on the pose path; the rule is
this project's own (include/deepcut_hip.h)."""
import ctypes as C

import numpy as np
import pytest

import caffe
import caffe.pycaffe as pc
import flip_ref as FL
import fuse_ref as F
import people_ref as R
from deepcut_tools import deepercut_prototxt
from fuse_ref import MEAN, STD, match_people

EINVAL, ESHAPE, ENOCPU = -1, -3, -6  # include/deepcut_hip.h


def test_the_joint_table_of_the_package_is_the_restated_one():
    import pose

    assert tuple(pose.MIRROR_MPII14) == FL.MIRROR_MPII14 == (5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13)
    assert all(FL.MIRROR_MPII14[FL.MIRROR_MPII14[j]] == j for j in range(14))


def test_mirrored_edges_take_the_lowest_index():
    pi = (1, 0, 2)
    assert list(FL.mirrored_edges(R.all_pairs_edges(3), pi)) == [2, 3, 0, 1, 5, 4]  # (0,1)->(1,0), (0,2)->(1,2), (1,0)->(0,1), ...
    twice = np.concatenate([R.all_pairs_edges(3), R.all_pairs_edges(3)])
    assert list(FL.mirrored_edges(twice, pi)) == [2, 3, 0, 1, 5, 4] * 2  # the duplicates in the second half are never chosen


def _linear_scene(shapes, scales, mirror, width, pi, edges, mean, std, slope):
    """Three joints and a `prob` that is linear in the image point, correctly encoded on every cell of every member; a mirrored member
    holds the encoding of the reflected, relabelled scene."""
    joints = np.array([[101.3, 77.9], [140.0, 31.5], [60.2, 120.4]])
    nj = len(joints)
    maps = []
    for (h, w), s, flipped in zip(shapes, scales, mirror):
        seen = joints.copy()
        if flipped:
            seen[list(pi)] = joints
            seen[:, 0] = (width - 1) - seen[:, 0]
        prob, loc, nxt = np.zeros((1, nj, h, w)), np.zeros((1, 2 * nj, h, w)), np.zeros((1, 2 * len(edges), h, w))
        for r in range(h):
            for c in range(w):
                x, y = (8.0 * c + 4.0) / s, (8.0 * r + 4.0) / s
                for j in range(nj):  # joint j of what this member sees is joint pi[j] of the scene, at the reflected column
                    jj, xx = (pi[j], (width - 1) - x) if flipped else (j, x)
                    prob[0, j, r, c] = 0.1 * (jj + 1) + slope[0] * xx + slope[1] * y
                    loc[0, 2 * j:2 * j + 2, r, c] = F.M.encode_targets(seen[j], seen[j], (r, c), s, (0, 0), (1, 1))[0]
                for l, (a, b) in enumerate(edges):
                    nxt[0, 2 * l:2 * l + 2, r, c] = F.M.encode_targets(seen[a], seen[b], (r, c), s, mean[l], std[l])[1]
        maps.append((prob, loc, nxt))
    return maps


def test_plain_and_mirrored_renderings_of_one_scene_fuse_to_the_plain_maps():
    """{plain, mirrored} at one scale and at two: the fused maps are the base member's own wherever no sample is clamped.  The statistics
    are powers of two and small integers, asymmetric between an edge and its mirror, and rho is 1 or 2: every gain and bias is
    exact as a float, so what is left is float64 rounding."""
    pi, edges, width = (1, 0, 2), R.all_pairs_edges(3), 187
    mean = np.array([[3, -5], [7, 2], [-4, 6], [1, 1], [0, -8], [9, 4]], np.float64)
    std = np.array([[2, 4], [8, 16], [4, 2], [16, 32], [2, 8], [32, 4]], np.float64)
    shapes = {0.5: (12, 12), 1.0: (23, 24)}  # canvases 96x96 and 184x192 of a 184 x 187 image
    for scales, mirror in (((1.0, 1.0), (0, 1)), ((1.0, 0.5, 1.0, 0.5), (0, 0, 1, 1))):
        maps = _linear_scene([shapes[s] for s in scales], scales, mirror, width, pi, edges, mean, std, (1e-3, 2e-3))
        fused, a = FL.fuse(maps, scales, 0, mirror, width, pi, edges, mean, std)
        h, w = shapes[1.0]
        # unclamped: the reflected sample of column c lies inside every mirrored member's map, and the plain one's too
        inner = (slice(None), slice(None), slice(1, h - 2), slice(2, w - 3))
        for k in range(3):
            err = np.abs(fused[k][inner] - maps[0][k][inner]).max()
            print("%d members, %s: max |fused - plain| = %.3e" % (len(scales), F.NAMES[k], err))
            assert err <= 1e-11 * max(1.0, np.abs(maps[0][k]).max())
        # and the mirrored members matter: with their flags dropped the same maps fuse to something else
        wrong, _ = F.fuse(maps, scales, 0, mean, std)
        assert np.abs(wrong[1][inner] - maps[0][1][inner]).max() > 1e-2


def test_the_identity_permutation_on_a_symmetric_scene():
    """pi = identity and (w - 1) s = 8 W_m: the reflection maps cell c onto cell W_m - 1 - c exactly.  A scene that is its own mirror
    image (prob and the y components symmetric, the decoded x components antisymmetric) then fuses with its mirrored copy to itself."""
    rs = np.random.RandomState(2)
    nb, nj, h, w = 2, 3, 7, 11
    edges = R.all_pairs_edges(nj)
    mean = np.array([[3, -5], [7, 2], [-4, 6], [1, 1], [0, -8], [9, 4]], np.float64)
    std = np.array([[2, 4], [8, 16], [4, 2], [16, 32], [2, 8], [32, 4]], np.float64)
    sym = lambda a: a + a[..., ::-1]  # noqa: E731
    anti = lambda a: a - a[..., ::-1]  # noqa: E731
    prob = sym(rs.rand(nb, nj, h, w))
    loc = np.zeros((nb, 2 * nj, h, w))
    loc[:, 0::2], loc[:, 1::2] = anti(rs.randn(nb, nj, h, w)), sym(rs.randn(nb, nj, h, w))
    nxt = np.zeros((nb, 2 * len(edges), h, w))
    nxt[:, 0::2] = (anti(rs.randn(nb, len(edges), h, w)) * 16 - mean[None, :, 0, None, None]) / std[None, :, 0, None, None]
    nxt[:, 1::2] = sym(rs.randn(nb, len(edges), h, w))
    maps = (prob, loc, nxt)
    width = 8 * w + 1
    i0, i1, f = FL.sample_axis_mirrored(w, w, 1.0, float(width - 1))
    assert np.array_equal(i0, np.arange(w)[::-1]) and (f == 0).all()
    fused, a = FL.fuse([maps, maps], (1.0, 1.0), 0, (0, 1), width, (0, 1, 2), edges, mean, std)
    for k in range(3):
        assert np.abs(fused[k] - maps[k]).max() <= 1e-12 * max(1.0, np.abs(maps[k]).max()), F.NAMES[k]
        assert (a[k] >= np.abs(fused[k]) - 1e-12).all()
    # with left and right swapped in the table the same maps are no longer their own mirror image
    other, _ = FL.fuse([maps, maps], (1.0, 1.0), 0, (0, 1), width, (1, 0, 2), edges, mean, std)
    assert np.abs(other[0] - prob).max() > 1e-2


def test_gain_and_bias_reduce_to_the_unmirrored_ones():
    """l' = l, pi the identity and the sign dropped: (rho, (rho - 1) mean / std) — to one float32 ulp, the two being different
    double expressions of the same number."""
    edges = R.all_pairs_edges()
    ident, same = np.arange(14), np.arange(len(edges))
    assert np.array_equal(FL.mirrored_edges(edges, ident), same)
    for rho in (1.0, 0.7 / 1.3, 1.3):
        for k, ch in ((0, 14), (1, 28), (2, 364)):
            g0, b0 = F.gain_bias(k, ch, rho, MEAN, STD)
            g1, b1, src = FL.mirror_gain_bias(k, ch, rho, ident, same, MEAN, STD, sign=1.0)
            assert np.array_equal(src, np.arange(ch))
            assert np.allclose(g1, g0, rtol=2.0 ** -23, atol=0) and np.allclose(b1, b0, rtol=2.0 ** -23, atol=1e-30)
    # the rule itself: the x components change sign, the edge's statistics are those of the mirrored edge
    lp = FL.mirrored_edges(edges, FL.MIRROR_MPII14)
    g, b, src = FL.mirror_gain_bias(2, 364, 0.5, FL.MIRROR_MPII14, lp, MEAN, STD)
    l = 17
    assert tuple(edges[lp[l]]) == (FL.MIRROR_MPII14[edges[l][0]], FL.MIRROR_MPII14[edges[l][1]]) and lp[l] != l
    assert src[2 * l] == 2 * lp[l] and src[2 * l + 1] == 2 * lp[l] + 1
    assert g[2 * l] == np.float32(-0.5 * STD[lp[l], 0] / STD[l, 0]) and g[2 * l + 1] == np.float32(0.5 * STD[lp[l], 1] / STD[l, 1])
    assert b[2 * l] == np.float32(-(0.5 * MEAN[lp[l], 0] + MEAN[l, 0]) / STD[l, 0])
    assert b[2 * l + 1] == np.float32((0.5 * MEAN[lp[l], 1] - MEAN[l, 1]) / STD[l, 1])


@pytest.mark.parametrize("sixteen_bit", [False, True])
def test_planted_mirrored_pyramid_returns_the_three_people(sixteen_bit):
    sc = FL.planted(sixteen_bit)
    gaps = {}
    counts, dets, cost, people, cand = F.assemble_fused([a[0] for a in sc["fused"]], R.all_pairs_edges(), FL.SCALES[FL.BASE], MEAN, STD, gaps=gaps)
    print("planted mirrored pyramid (%s): gap between a chosen link and the best it rules out >= %.6g, gap to max_cost >= %.6g network pixels"
          % ("16-bit values" if sixteen_bit else "float32 values", gaps["choice"], gaps["max_cost"]))
    assert gaps["choice"] >= 1e-6 and gaps["max_cost"] >= 1e-6
    assert (counts == 3).all() and people.shape == (3, 14, 3) and (cand >= 0).all()
    who = match_people(people, sc["joints"])
    assert sorted(who) == [0, 1, 2]
    assert np.allclose(people[:, :, :2], sc["joints"][who], rtol=0, atol=1e-9)
    assert np.abs(people[:, :, :2] - sc["truth"][who]).max() <= (1.0 if sixteen_bit else 1e-4)
    # the mirrored members are really mirrored: fused as if they were plain, the same maps do not decode to the planted joints
    wrong, _ = F.fuse(sc["maps"], FL.SCALES, FL.BASE, MEAN, STD)
    r, c = sc["cells"][0][0]
    assert wrong[0][0][0, r, c] < 0.75 * sc["fused"][0][0][0, r, c]


# ---- the entry points without a device ------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Calls(object):
    """The three mirrored entry points on one group of four through the raw C ABI, with arguments that are right unless a test replaces one."""

    def __init__(self):
        a = caffe.Net(deepercut_prototxt(101, 64, 64), caffe.TEST, from_text=True)
        self.g = g = caffe.NetGroup([a] + [a.clone() for _ in range(3)])
        n, j = g.nets[0].blobs["prob"].shape[:2]
        self.j, self.e = j, g.nets[0].blobs["next_pred"].shape[1] // 2
        self.edges = np.ascontiguousarray(R.all_pairs_edges(j)[:self.e], np.int32)
        h, w = g.nets[0].blobs["prob"].shape[2:]
        self.out = [np.zeros((n, c, h, w), np.float32) for c in (j, 2 * j, 2 * self.e)]
        self.counts, self.dets = np.zeros((n, j), np.int32), np.zeros((n, j, 8, 5))
        self.n_people, self.people = np.zeros(n, np.int32), np.zeros((n, 32, j, 3))
        self.q = pc.AssembleParams(-5.0, 0.5, 1, 8, 20.0, 0.5, 32, 1)
        self.sc = np.ascontiguousarray([0.7, 1.0, 0.7, 1.0], np.float64)

    def mirror(self, flags=(0, 0, 1, 1), width=64, pi=FL.MIRROR_MPII14, n_edges=None, edges="own"):
        self.keep = (None if flags is None else np.ascontiguousarray(flags, np.int32), None if pi is None else np.ascontiguousarray(pi, np.int32),
                     self.edges if isinstance(edges, str) else edges)
        fm = pc.FuseMirror(*[None if a is None else a.ctypes.data for a in self.keep[:2]][:1], width,
                           None if self.keep[1] is None else self.keep[1].ctypes.data, self.e if n_edges is None else n_edges,
                           None if self.keep[2] is None else self.keep[2].ctypes.data)
        return fm

    def fuse(self, fm, base=1, want=(True, True, True)):
        o = [_vp(a) if w else None for a, w in zip(self.out, want)]
        return pc._lib.dc_group_fuse_maps_mirrored(self.g._h, _vp(self.sc), base, None if fm is None else C.byref(fm), self.e, None, None, o[0], o[1],
                                                   o[2], 0, None)

    def detect(self, fm, base=1, **_):
        return pc._lib.dc_group_detect_parts_mirrored(self.g._h, _vp(self.sc), base, None if fm is None else C.byref(fm), 0.5, 1, 8, _vp(self.counts),
                                                      _vp(self.dets))

    def assemble(self, fm, base=1, **_):
        return pc._lib.dc_group_assemble_people_mirrored(self.g._h, _vp(self.sc), base, None if fm is None else C.byref(fm), C.byref(self.q), self.e,
                                                         _vp(self.edges), None, None, None, _vp(self.n_people), _vp(self.people), None, None)


def _err():
    return (pc._lib.dc_last_error() or b"").decode()


def test_the_mirrored_entry_points_refuse_bad_arguments_before_any_device_work():
    caffe.set_mode_cpu()
    k = _Calls()
    assert k.j == 14
    swapped = list(FL.MIRROR_MPII14)
    swapped[0], swapped[1] = 4, 4  # 0 -> 4 -> 1: no involution
    far = list(FL.MIRROR_MPII14)
    far[3] = 14
    pairs_only = np.ascontiguousarray(R.one_direction_edges(14)[:k.e], np.int32)  # a -> c with a < c only: (0, 1) has no mirrored (5, 4)
    for name, call in (("fuse_maps", k.fuse), ("detect_parts", k.detect), ("assemble_people", k.assemble)):
        # right arguments get as far as the device: CPU mode is what is refused
        assert call(k.mirror()) == ENOCPU and "CPU mode" in _err(), name
        assert call(k.mirror(width=0)) == EINVAL and "image_width" in _err(), name
        assert call(k.mirror(width=-3)) == EINVAL and "image_width" in _err(), name
        assert call(k.mirror(pi=None)) == EINVAL and "joint_mirror" in _err(), name
        assert call(k.mirror(pi=far)) == EINVAL and "joint_mirror[3]" in _err(), name
        assert call(k.mirror(pi=swapped)) == EINVAL and "involution" in _err(), name
        assert call(k.mirror(flags=(0, 1, 1, 0))) == EINVAL and "base" in _err() and "mirrored" in _err(), name
        # what the unmirrored calls refuse is refused in the same way, first
        assert call(k.mirror(), base=4) == EINVAL and "base 4 is outside" in _err(), name
        if name != "detect_parts":  # (it fuses prob and loc_pred only: the edges are not read)
            assert call(k.mirror(n_edges=k.e - 1)) == EINVAL and "edges" in _err(), name
            assert call(k.mirror(edges=None)) == EINVAL and "null edges" in _err(), name
            if name == "fuse_maps":  # (assemble_people takes its own `edges`, which this group's full list is)
                assert call(k.mirror(edges=pairs_only)) == EINVAL and "no mirrored edge" in _err(), name
        # no mirrored member, or no table at all: nothing of it is read, the unmirrored path answers
        assert call(k.mirror(flags=(0, 0, 0, 0), width=0, pi=None, n_edges=3, edges=None)) == ENOCPU, name
        assert call(k.mirror(flags=None, width=0, pi=None)) == ENOCPU, name
        assert call(None) == ENOCPU, name
    # without next_pred the edges are not read
    assert k.fuse(k.mirror(n_edges=5, edges=None), want=(True, True, False)) == ENOCPU
    # the forward entry: a null member image is refused with or without a mirror table, then CPU mode
    img = np.zeros((1, 64, 64, 3), np.uint8)
    ptrs = (C.c_void_p * 4)(*[img.ctypes.data] * 4)
    ints = lambda v: (C.c_int * 4)(*v)  # noqa: E731
    args = (ints([1] * 4), ints([64] * 4), ints([64] * 4), (C.c_double * 4)(0.7, 1.0, 0.7, 1.0))
    flags = np.ascontiguousarray([0, 0, 1, 1], np.int32)
    assert pc._lib.dc_group_forward_images_mirrored(k.g._h, ptrs, *args, _vp(flags), 0, None, None, None, None) == ENOCPU
    assert pc._lib.dc_group_forward_images_mirrored(k.g._h, ptrs, *args, None, 0, None, None, None, None) == ENOCPU
    ptrs[2] = None
    assert pc._lib.dc_group_forward_images_mirrored(k.g._h, ptrs, *args, _vp(flags), 0, None, None, None, None) == EINVAL and "member 2" in _err()


def test_the_python_methods_check_the_lengths():
    caffe.set_mode_cpu()
    k = _Calls()
    g, sc = k.g, [0.7, 1.0, 0.7, 1.0]
    with pytest.raises(ValueError):
        g.fuse_maps(sc, 1, mirror=[0, 0, 1])  # one flag per member
    with pytest.raises(ValueError):
        g.fuse_maps(sc, 1, mirror=[0, 0, 1, 1], image_width=64, joint_mirror=FL.MIRROR_MPII14[:-1], edges=k.edges)
    with pytest.raises(ValueError):
        g.forward_images(np.zeros((64, 64, 3), np.uint8), sc, pose=True, mirror=[0, 0, 1, 1])  # no pose from a mirrored member
    with pytest.raises(ValueError):
        g.forward_images(np.zeros((64, 64, 3), np.uint8), sc, pose=False, mirror=[0, 1])
    # right lengths: the library answers (CPU mode), through the mirrored entries and — mirror=None — through today's
    for kw in (dict(mirror=[0, 0, 1, 1], image_width=64, joint_mirror=FL.MIRROR_MPII14), dict()):
        with pytest.raises(caffe.DeepcutError) as e:
            g.fuse_maps(sc, 1, edges=k.edges, **kw) if kw else g.fuse_maps(sc, 1)
        assert e.value.code == ENOCPU
        with pytest.raises(caffe.DeepcutError) as e:
            g.detect_parts(sc, 1, **kw)
        assert e.value.code == ENOCPU
        with pytest.raises(caffe.DeepcutError) as e:
            g.assemble_people(sc, 1, edges=k.edges, max_cost=20.0, **kw)
        assert e.value.code == ENOCPU
    with pytest.raises(caffe.DeepcutError) as e:
        g.fuse_maps(sc, 2, mirror=[0, 0, 1, 1], image_width=64, joint_mirror=FL.MIRROR_MPII14, edges=k.edges)
    assert e.value.code == EINVAL and "mirrored" in str(e.value)


def test_estimate_people_checks_the_flip_arguments_without_a_device():
    from pose import estimate_people

    img = np.zeros((64, 64, 3), np.uint8)
    stats = (R.all_pairs_edges(), None, None)
    bad = list(FL.MIRROR_MPII14)
    bad[0], bad[1] = 4, 4
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, stats, flip=True, joint_mirror=bad)
    assert "involution" in str(e.value)
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, stats, flip=True, joint_mirror=None)
    assert "joint_mirror" in str(e.value)
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, stats, flip=True, joint_mirror=list(range(13)) + [14])
    assert "outside" in str(e.value)
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, stats, scales=[0.7, 1.0], base=2, flip=True)  # member 2 is the mirror of member 0
    assert "plain" in str(e.value)
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, stats, scale=0.8, base=1, flip=True)
    assert "plain" in str(e.value)
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, stats, scale=0.5, scales=[0.5, 1.0], flip=True)
    assert "scales" in str(e.value)
