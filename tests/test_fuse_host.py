"""CPU: the multi-scale fusion rule of dc_group_fuse_maps as restated in tests/fuse_ref.py (its properties, and the planted pyramid
through the restated people assembly), and the host side of dc_group_fuse_maps / dc_group_detect_parts / dc_group_assemble_people:
what they refuse before any device work.  The device side is tests/test_gpu_fuse.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps; the fusion rule is this project's own
(include/deepcut_hip.h)."""
import ctypes as C

import numpy as np
import pytest

import caffe
import caffe.pycaffe as pc
import fuse_ref as F
import people_ref as R
from deepcut_tools import deepercut_prototxt

from fuse_ref import MEAN, SCALES, STD, match_people, planted

EINVAL, ESHAPE, ENOCPU = -1, -3, -6  # include/deepcut_hip.h


def _random_maps(shapes, nb=2, joints=3, edges=4, seed=3):
    rs = np.random.RandomState(seed)
    return [(rs.rand(nb, joints, h, w).astype(np.float32), rs.randn(nb, 2 * joints, h, w).astype(np.float32),
             rs.randn(nb, 2 * edges, h, w).astype(np.float32)) for h, w in shapes]


def zeroed_others(maps, base):
    return [t if m == base else tuple(np.zeros_like(a) for a in t) for m, t in enumerate(maps)]


def test_one_member_is_the_identity():
    maps = _random_maps([(7, 9)])
    fused, a = F.fuse(maps, [0.8], 0, np.ones((4, 2)), np.full((4, 2), 2.0))
    for k in range(3):
        assert np.array_equal(fused[k], maps[0][k].astype(np.float64))
        assert np.array_equal(a[k], np.abs(maps[0][k]).astype(np.float64))


def test_the_base_member_contributes_its_own_cells():
    """Replacing the base member's maps by zero changes the fused maps by exactly (base cell * its gain 1 + its bias 0) / M."""
    shapes = [(8, 11), (11, 15), (15, 20)]
    maps = _random_maps(shapes)
    mean, std = np.arange(8.0).reshape(4, 2), np.full((4, 2), 3.0)
    for base in (0, 1, 2):
        for axis, n in ((0, shapes[base][0]), (1, shapes[base][1])):
            i0, i1, f = F.sample_axis(n, n, 1.0)
            assert np.array_equal(i0, np.arange(n)) and (f == 0).all()
        zeroed = [tuple(np.zeros_like(a) for a in t) if m == base else t for m, t in enumerate(maps)]
        full, _ = F.fuse(maps, SCALES, base, mean, std)
        rest, _ = F.fuse(zeroed, SCALES, base, mean, std)
        third = float(np.float32(1.0) / np.float32(3.0))
        for k in range(3):
            assert np.allclose(full[k] - rest[k], maps[base][k].astype(np.float64) * third, rtol=0, atol=1e-12)
        # the base member alone (the others hold zeros; no statistics, so no bias): weight 1 on its own cell and nothing else, i.e.
        # exactly its own maps times the float32 1/3 — not a bit of interpolation
        alone, mag = F.fuse(zeroed_others(maps, base), SCALES, base)
        for k in range(3):
            assert np.array_equal(alone[k], maps[base][k].astype(np.float64) * third)
            assert np.array_equal(mag[k], np.abs(maps[base][k]).astype(np.float64) * third)


def test_a_linear_field_is_interpolated_without_error():
    """loc_pred and next_pred of one joint, correctly encoded on every cell of every member: the fused values are the base member's
    own encoding wherever no sample is clamped (here: away from the last rows and columns)."""
    shapes = [(18, 24), (25, 33), (33, 43)]
    joint, nxt_joint, mean, std = np.array([101.3, 77.9]), np.array([140.0, 31.5]), np.array([[7.0, -3.0]]), np.array([[11.0, 5.0]])
    maps = []
    for (h, w), s in zip(shapes, SCALES):
        loc, nxt = np.zeros((1, 2, h, w)), np.zeros((1, 2, h, w))
        for r in range(h):
            for c in range(w):
                loc[0, :, r, c], nxt[0, :, r, c] = F.M.encode_targets(joint, nxt_joint, (r, c), s, mean[0], std[0])
        maps.append((None, loc, nxt))
    for base in (0, 1, 2):
        fused, a = F.fuse(maps, SCALES, base, mean, std)
        h, w = shapes[base]
        inner = (slice(None), slice(None), slice(1, h - 2), slice(1, w - 2))
        for k in (1, 2):
            # (gain and bias are carried as float32: one rounding each, relative to their terms of A)
            assert (np.abs(fused[k][inner] - maps[base][k][inner]) <= 2 * 2.0 ** -24 * a[k][inner]).all()


@pytest.mark.parametrize("sixteen_bit", [False, True])
def test_planted_pyramid_returns_the_three_people(sixteen_bit):
    sc = planted(sixteen_bit)
    gaps = {}
    counts, dets, cost, people, cand = F.assemble_fused([a[0] for a in sc["fused"]], R.all_pairs_edges(), SCALES[1], MEAN, STD, gaps=gaps)
    print("planted pyramid (%s): gap between a chosen link and the best it rules out >= %.6g, gap to max_cost >= %.6g network pixels"
          % ("16-bit values" if sixteen_bit else "float32 values", gaps["choice"], gaps["max_cost"]))
    assert gaps["choice"] >= 1e-6 and gaps["max_cost"] >= 1e-6
    assert (counts == 3).all() and people.shape == (3, 14, 3) and (cand >= 0).all()
    who = match_people(people, sc["joints"])
    assert sorted(who) == [0, 1, 2]
    assert np.allclose(people[:, :, :2], sc["joints"][who], rtol=0, atol=1e-9)
    assert np.abs(people[:, :, :2] - sc["truth"][who]).max() <= (1.0 if sixteen_bit else 1e-4)


# ---- the three entry points without a device --------------------------------------------------------------------------------------
def _group(n=3, h=64, w=64):
    a = caffe.Net(deepercut_prototxt(101, h, w), caffe.TEST, from_text=True)
    return caffe.NetGroup([a] + [a.clone() for _ in range(n - 1)])


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Calls(object):
    """The three entry points on one group through the raw C ABI, with arguments that are right unless a test replaces one."""

    def __init__(self, g):
        self.g = g
        n, j = g.nets[0].blobs["prob"].shape[:2]
        self.e = g.nets[0].blobs["next_pred"].shape[1] // 2
        self.edges = np.ascontiguousarray(R.all_pairs_edges(j)[:self.e], np.int32)
        h, w = g.nets[0].blobs["prob"].shape[2:]
        self.out = [np.zeros((n, c, h, w), np.float32) for c in (j, 2 * j, 2 * self.e)]
        self.counts, self.dets = np.zeros((n, j), np.int32), np.zeros((n, j, 8, 5))
        self.n_people, self.people = np.zeros(n, np.int32), np.zeros((n, 32, j, 3))
        self.q = pc.AssembleParams(-5.0, 0.5, 1, 8, 20.0, 0.5, 32, 1)  # (scale is not read)

    def fuse(self, scales, base=0, n_edges=None, mean=None, std=None, want=(True, True, True)):
        sc = None if scales is None else np.ascontiguousarray(scales, np.float64)
        o = [_vp(a) if w else None for a, w in zip(self.out, want)]
        return pc._lib.dc_group_fuse_maps(self.g._h, _vp(sc), base, self.e if n_edges is None else n_edges, _vp(mean), _vp(std), o[0], o[1], o[2], 0,
                                          None)

    def detect(self, scales, base=0, **_):
        sc = None if scales is None else np.ascontiguousarray(scales, np.float64)
        return pc._lib.dc_group_detect_parts(self.g._h, _vp(sc), base, 0.5, 1, 8, _vp(self.counts), _vp(self.dets))

    def assemble(self, scales, base=0, n_edges=None, mean=None, std=None, **_):
        sc = None if scales is None else np.ascontiguousarray(scales, np.float64)
        ne = self.e if n_edges is None else n_edges
        edges = self.edges if ne <= self.e else np.ascontiguousarray(np.concatenate([self.edges, self.edges])[:ne])
        return pc._lib.dc_group_assemble_people(self.g._h, _vp(sc), base, C.byref(self.q), ne, _vp(edges), _vp(mean), _vp(std), None,
                                                _vp(self.n_people), _vp(self.people), None, None)


def _err():
    return (pc._lib.dc_last_error() or b"").decode()


def test_the_entry_points_refuse_bad_arguments_before_any_device_work():
    caffe.set_mode_cpu()
    g = _group()
    k = _Calls(g)
    good = [0.7, 1.0, 1.3]
    nan_mean, neg_std, inf_std = np.zeros((k.e, 2)), np.ones((k.e, 2)), np.ones((k.e, 2))
    nan_mean[3, 1], neg_std[2, 0], inf_std[5, 1] = np.nan, -1.0, np.inf
    for name, call in (("fuse_maps", k.fuse), ("detect_parts", k.detect), ("assemble_people", k.assemble)):
        assert call(None) == EINVAL and "scales" in _err(), name
        for bad in ([0.7, 0.0, 1.3], [0.7, 1.0, -1.3], [np.nan, 1.0, 1.3], [0.7, np.inf, 1.3]):
            assert call(bad) == EINVAL and "scale of member" in _err(), (name, bad)
        for base in (-1, 3):
            assert call(good, base=base) == EINVAL and "base" in _err(), (name, base)
        if name == "detect_parts":
            continue  # (it fuses prob and loc_pred only: no statistics, no edges)
        assert call(good, mean=nan_mean) == EINVAL and "mean of edge 3" in _err(), name
        assert call(good, std=neg_std) == EINVAL and "std of edge 2" in _err(), name
        assert call(good, std=inf_std) == EINVAL and "std of edge 5" in _err(), name
        assert call(good, n_edges=k.e - 1) == ESHAPE and "edges" in _err(), name
        assert call(good, n_edges=k.e + 1) == ESHAPE and "edges" in _err(), name
    # without next_pred neither the statistics nor n_edges are read
    assert k.fuse(good, n_edges=5, mean=nan_mean, want=(True, True, False)) == ENOCPU
    # members whose maps differ in batch size
    g.nets[1].blobs["data"].reshape(2, 3, 64, 64)
    g.nets[1].reshape()
    for name, call in (("fuse_maps", k.fuse), ("detect_parts", k.detect), ("assemble_people", k.assemble)):
        assert call(good) == ESHAPE and "member 1" in _err() and "2 images" in _err(), name


def test_then_cpu_mode_is_refused():
    caffe.set_mode_cpu()
    g = _group()
    k = _Calls(g)
    single = pc._lib.dc_net_detect_parts(g.nets[0]._h, 1.0, 0.5, 1, 8, _vp(k.counts), _vp(k.dets))  # the single-net entry's own answer
    assert single == ENOCPU
    for name, call in (("fuse_maps", k.fuse), ("detect_parts", k.detect), ("assemble_people", k.assemble)):
        assert call([0.7, 1.0, 1.3], base=1) == single and "CPU mode" in _err(), name
    # through the Python methods: the same answers as exceptions
    with pytest.raises(caffe.DeepcutError) as e:
        g.fuse_maps([0.7, 1.0, 1.3])
    assert e.value.code == single
    with pytest.raises(caffe.DeepcutError) as e:
        g.detect_parts([0.7, 1.0, 1.3], base=1)
    assert e.value.code == single
    with pytest.raises(caffe.DeepcutError) as e:
        g.assemble_people([0.7, 1.0, 1.3], base=1, edges=k.edges, max_cost=20.0)
    assert e.value.code == single
    with pytest.raises(caffe.DeepcutError) as e:
        g.fuse_maps([0.7, -1.0, 1.3])
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        g.fuse_maps([0.7, 1.0])  # one scale per member
    with pytest.raises(ValueError):
        g.assemble_people([0.7, 1.0, 1.3], edges=k.edges[:-1])


def test_estimate_people_refuses_scale_together_with_scales():
    from pose import estimate_people

    img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError) as e:
        estimate_people(img, None, None, (R.all_pairs_edges(), None, None), scale=0.5, scales=[0.5, 1.0])
    assert "scales" in str(e.value)
