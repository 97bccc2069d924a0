"""-m gpu: mirror test-time augmentation of the bottom-up entry — dc_group_forward_images_mirrored (the flip inside the device
pre-processing) and dc_group_fuse_maps_mirrored / dc_group_detect_parts_mirrored / dc_group_assemble_people_mirrored (mirrored members
fused on the device) — against the host-flipped image, the restatement in tests/flip_ref.py and, behind it, tests/people_ref.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and mirrors nothing on the pose path, so there is no
reference output to hold the rule to.  The rule is this project's own (include/deepcut_hip.h); what is proven here is that the flipped
pre-processing is bit for bit the unflipped one of the flipped image, and that the device fuses what its restatement fuses, within
the float32 bound the restatement derives (16 * 2^-24 * A: a mirrored member costs the roundings an unmirrored one does)."""
import ctypes as C

import numpy as np
import pytest

import flip_ref as FL
import fuse_ref as F
import people_ref as R
from fuse_ref import MEAN, STD, match_people

pytestmark = pytest.mark.gpu

# 88 x 117: the width is no multiple of 8, so (w - 1) s is not cell-aligned and both edges clamp.  Canvases 88x120 and 64x88: maps 11x15, 8x11
IMG = np.random.RandomState(37).randint(0, 256, (2, 88, 117, 3)).astype(np.uint8)
SCALES = (1.0, 0.7, 1.0, 0.7)  # scale 1.0 takes the no-resample branch of the pre-processing, 0.7 both resample passes
MIRROR = (0, 0, 1, 1)
ALL = ("prob", "loc_pred", "next_pred")
PI = FL.MIRROR_MPII14
EDGES = R.all_pairs_edges()
MKW = dict(mirror=MIRROR, image_width=IMG.shape[2], joint_mirror=PI)


def _group(caffe, path, image_hw, scales, n=1, **kw):
    from deepcut_tools import deepercut_prototxt

    shapes = [(n,) + tuple(caffe.canvas_size(image_hw[0], image_hw[1], s)) for s in scales]
    net = caffe.Net(deepercut_prototxt(152, shapes[0][1], shapes[0][2], n), path, caffe.TEST, from_text=True, **kw)
    return caffe.NetGroup.for_shapes(net, shapes)


KINDS = {"f32": dict(), "f16": dict(dtype="f16"), "bf16": dict(dtype="bf16"), "fuse0": dict(fuse=0)}


_made = {}


def _forwarded(kind, gpu_caffe, synth152):
    """Per kind of member, once per module: the group, what ONE grouped forward of [IMG, IMG, host-flipped IMG, host-flipped IMG] left in
    the members (inputs and maps), and then the same after ONE grouped forward of IMG with the last two members mirrored on the device —
    whose maps the members still hold.  Never written to, and no test forwards these groups again."""
    if kind not in _made:
        grp = _group(gpu_caffe, synth152[0], IMG.shape[1:3], SCALES, n=2, **KINDS[kind])
        flipped = np.ascontiguousarray(IMG[:, :, ::-1])
        state = []
        for images, kw in (([IMG, IMG, flipped, flipped], dict()), (IMG, dict(mirror=MIRROR))):
            outs = grp.forward_images(images, SCALES, want=ALL, pose=False, **kw)
            state.append(([net.blobs["data"].data.copy() for net in grp.nets], [tuple(o[k].copy() for k in ALL) for o in outs]))
        _made[kind] = (kind, grp, state[0], state[1])
    return _made[kind]


@pytest.fixture(scope="module", params=list(KINDS))
def forwarded(request, gpu_caffe, synth152):
    return _forwarded(request.param, gpu_caffe, synth152)


@pytest.fixture(scope="module")
def forwarded_f32(gpu_caffe, synth152):
    """The float32 group alone, for what does not depend on the members' element type (the unmirrored path, the chain on the float32
    fused buffer, the host-side refusals)."""
    yield _forwarded("f32", gpu_caffe, synth152)
    _made.clear()


def test_mirrored_preprocessing_is_the_plain_one_of_the_flipped_image(forwarded):
    """The network input of a mirrored member, and with it all three maps, bit for bit — with a horizontal resample pass (0.7) and
    without one (1.0), for float32, float16 and bfloat16 inputs."""
    kind, grp, (host_data, host_maps), (dev_data, dev_maps) = forwarded
    assert [m[0].shape[2:] for m in dev_maps] == [(11, 15), (8, 11), (11, 15), (8, 11)]
    for m in range(4):
        assert host_data[m].shape == dev_data[m].shape and np.array_equal(host_data[m], dev_data[m]), (kind, "data", m)
        for k, name in enumerate(ALL):
            assert np.array_equal(host_maps[m][k], dev_maps[m][k]), (kind, name, m)
    # and the flip is a flip: the mirrored member's input is not the plain member's (nor are its maps)
    assert not np.array_equal(dev_data[0], dev_data[2]) and not np.array_equal(dev_maps[1][0], dev_maps[3][0])
    assert np.array_equal(dev_data[0][:, :, :, :117], dev_data[2][:, :, :, 116::-1])  # scale 1.0: the pixels themselves, reversed


def test_fused_maps_of_a_real_mirrored_forward_match_the_restatement(forwarded):
    """M = 4 (two scales, each plain and mirrored), batch 2, the full 14 / 28 / 364 heads, MIRROR_MPII14, all-pairs edges, base = either
    plain member; float32, float16, bfloat16 and DC_OPT_FUSE 0 members (separate map tensors, not channel views)."""
    kind, grp, _, (_, maps) = forwarded
    for base in (0, 1):
        ref, a = FL.fuse(maps, SCALES, base, MIRROR, IMG.shape[2], PI, EDGES, MEAN, STD)
        got = grp.fuse_maps(SCALES, base, MEAN, STD, edges=EDGES, **MKW)
        again = grp.fuse_maps(SCALES, base, MEAN, STD, edges=EDGES, **MKW)
        for k, name in enumerate(ALL):
            assert got[name].dtype == np.float32 and got[name].shape == ref[k].shape
            ratio = FL.worst_ratio(got[name], ref[k], a[k])
            print("%s, base %d, %s: worst |device - restatement| / (16 * 2^-24 * A) = %.4f" % (kind, base, name, ratio))
            assert ratio <= 1.0
            assert np.array_equal(got[name], again[name])
        # the flags matter: the same maps fused as if nobody were mirrored are something else
        plain = grp.fuse_maps(SCALES, base, MEAN, STD)
        assert not np.array_equal(plain["loc_pred"], got["loc_pred"])
    # a subset of the maps: the same numbers, and the edges are not needed
    part = grp.fuse_maps(SCALES, 1, want=("prob", "loc_pred"), **MKW)
    full = grp.fuse_maps(SCALES, 1, MEAN, STD, edges=EDGES, **MKW)
    assert sorted(part) == ["loc_pred", "prob"] and all(np.array_equal(part[k], full[k]) for k in part)
    # one map alone: its rows of the table start at channel 0; next_pred alone counts the joints from the base member's prob
    for name in ALL:
        one = grp.fuse_maps(SCALES, 1, MEAN, STD, want=(name,), edges=EDGES, **MKW)
        assert list(one) == [name] and np.array_equal(one[name], full[name]), name


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _same(a, b):
    return all(np.array_equal(x["people"], y["people"]) and np.array_equal(x["cand"], y["cand"]) and np.array_equal(x["cost"], y["cost"])
               for x, y in zip(a, b))


def test_no_mirrored_member_is_todays_result_bit_for_bit(forwarded_f32):
    """mirror all zero, and a NULL table through the C ABI: fuse_maps, detect_parts and assemble_people of the unmirrored entries."""
    import caffe.pycaffe as pc

    kind, grp, _, _ = forwarded_f32
    none = dict(mirror=(0, 0, 0, 0), image_width=None, joint_mirror=None)
    want = grp.fuse_maps(SCALES, 1, MEAN, STD)
    got = grp.fuse_maps(SCALES, 1, MEAN, STD, **none)
    assert all(np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)) for k in ALL)
    out = {k: np.full_like(want[k], np.nan) for k in ALL}
    sc = np.ascontiguousarray(SCALES, np.float64)
    rc = pc._lib.dc_group_fuse_maps_mirrored(grp._h, _vp(sc), 1, None, 182, _vp(np.ascontiguousarray(MEAN)), _vp(np.ascontiguousarray(STD)),
                                             _vp(out["prob"]), _vp(out["loc_pred"]), _vp(out["next_pred"]), 0, None)
    assert rc == 0, pc._lib.dc_last_error()
    assert all(np.array_equal(want[k].view(np.uint32), out[k].view(np.uint32)) for k in ALL)
    kw = dict(threshold=0.5, radius=1, max_det=8, edges=EDGES, mean=MEAN, std=STD, max_cost=40.0, seed_threshold=0.55, max_people=32, min_joints=1,
              return_cost=True)
    assert _same(grp.assemble_people(SCALES, 1, **kw), grp.assemble_people(SCALES, 1, **dict(kw, **none)))
    a, b = grp.detect_parts(SCALES, 1, 0.5, 1, 8), grp.detect_parts(SCALES, 1, 0.5, 1, 8, **none)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_chain_on_the_devices_own_mirrored_fusion(forwarded_f32):
    """detect_parts and assemble_people with mirrored members against the oracle's candidates and the restated costs and assembly run on
    the maps fuse_maps returned: the standard tests/test_gpu_fuse.py holds the unmirrored chain to."""
    kind, grp, _, _ = forwarded_f32
    base = 1
    fused = grp.fuse_maps(SCALES, base, MEAN, STD, edges=EDGES, **MKW)
    thr, radius, md, max_cost, seed = 0.5, 1, 8, 40.0, 0.55
    kw = dict(threshold=thr, radius=radius, max_det=md, edges=EDGES, mean=MEAN, std=STD, max_cost=max_cost, seed_threshold=seed, max_people=32,
              min_joints=1)
    runs = [grp.assemble_people(SCALES, base, return_cost=True, **dict(kw, **MKW)) for _ in range(2)]
    assert _same(runs[0], runs[1])
    counts, dets = grp.detect_parts(SCALES, base, thr, radius, md, **MKW)
    total = finite = 0
    for b in range(2):
        ref_counts, ref_dets = R.M.nms_candidates(fused["prob"][b], fused["loc_pred"][b], SCALES[base], thr, radius, md)
        assert np.array_equal(counts[b], ref_counts) and np.array_equal(dets[b][:, :, 2:], ref_dets[:, :, 2:])
        assert np.allclose(dets[b][:, :, :2], ref_dets[:, :, :2], rtol=0, atol=1e-9)
        ref_cost = R.pair_costs_from_candidates(ref_counts, ref_dets, fused["next_pred"][b], EDGES, SCALES[base], MEAN, STD)
        got = runs[0][b]["cost"]
        assert np.array_equal(np.isposinf(got), np.isposinf(ref_cost)) and not np.isnan(got).any()
        fin = np.isfinite(ref_cost)
        err = float(np.abs(got[fin] - ref_cost[fin]).max()) if fin.any() else 0.0
        print("mirrored chain, image %d: %d candidates, %d finite costs, max |device - restatement| = %.3e" % (b, counts[b].sum(), fin.sum(), err))
        assert err <= 1e-9
        people, cand = R.assemble(counts[b], dets[b], got, max_cost, seed, 32, 1)
        assert np.array_equal(runs[0][b]["cand"], cand) and np.array_equal(runs[0][b]["people"], people)
        total += len(cand)
        finite += int(fin.sum())
    assert total > 0 and finite > 0


@pytest.mark.parametrize("dtype,sixteen_bit", [("f32", False), ("bf16", True)])
def test_planted_mirrored_pyramid_whole_chain(gpu_caffe, synth152, dtype, sixteen_bit):
    """Three planted people rendered into every member's maps — for the mirrored members as the mirror image shows them — and written
    through `.data`.  The restatement decides from the maps alone, with room to spare (tests/test_flip_host.py asserts the gaps), which
    candidates there are and how they group; the device returns exactly that, and every joint within sqrt(53) / s_b times the float32
    bound of the fused loc_pred."""
    sc = FL.planted(sixteen_bit)
    grp = _group(gpu_caffe, synth152[0], FL.IMAGE_HW, FL.SCALES, fuse=0, dtype=dtype)
    img = np.random.RandomState(8).randint(0, 256, FL.IMAGE_HW + (3,)).astype(np.uint8)
    grp.forward_images(img, FL.SCALES, want=(), pose=False, mirror=FL.MIRROR)
    assert grp.nets[0].dtype == dtype
    for net, maps in zip(grp.nets, sc["maps"]):
        for k, name in enumerate(ALL):
            assert net.blobs[name].shape[2:] == maps[k].shape[2:]
            net.blobs[name].data[...] = maps[k]
    mkw = dict(mirror=FL.MIRROR, image_width=FL.IMAGE_HW[1], joint_mirror=PI)
    fused = [a[0] for a in sc["fused"]]
    s_b = FL.SCALES[FL.BASE]
    counts, dets, cost, people, cand = F.assemble_fused(fused, EDGES, s_b, MEAN, STD)
    dev_counts, dev_dets = grp.detect_parts(FL.SCALES, FL.BASE, F.THRESHOLD, 1, 8, **mkw)
    assert np.array_equal(dev_counts[0], counts) and (counts == 3).all() and np.array_equal(dev_dets[0][:, :, 3:], dets[:, :, 3:])
    got = grp.assemble_people(FL.SCALES, FL.BASE, threshold=F.THRESHOLD, radius=1, max_det=8, edges=EDGES, mean=MEAN, std=STD, max_cost=20.0,
                              seed_threshold=0.5, min_joints=2, **mkw)[0]
    assert np.array_equal(got["cand"], cand) and (cand >= 0).all() and cand.shape == (3, 14)
    who = match_people(got["people"], sc["joints"])
    assert sorted(who) == [0, 1, 2]
    worst = 0.0
    for p, q in enumerate(who):
        for j in range(14):
            r, c = sc["cells"][q][j]
            for k in range(2):
                lim = R.M.LOCREF / s_b * F.BOUND * sc["A"][1][0, 2 * j + k, r, c] + 1e-12  # (+ the double arithmetic of the decode)
                err = abs(got["people"][p, j, k] - sc["joints"][q, j, k])
                worst = max(worst, err / lim)
                assert err <= lim, (q, j, k, err, lim)
    print("planted mirrored pyramid (%s): worst joint error / bound = %.4f" % (dtype, worst))
    dev = grp.fuse_maps(FL.SCALES, FL.BASE, MEAN, STD, edges=EDGES, **mkw)
    for k, name in enumerate(ALL):
        assert FL.worst_ratio(dev[name], sc["fused"][k], sc["A"][k]) <= 1.0, name


def test_estimate_people_with_flip(gpu_caffe, synth152):
    """estimate_people(flip=True) = one mirrored grouped forward + one NetGroup.assemble_people by hand: a single scale as a group of two,
    a pyramid of k scales as a group of 2k (the plain members, then their mirrors; base: the plain scale nearest 1.0); flip=False is what
    it was."""
    from deepcut_tools import deepercut_prototxt
    from pose import MIRROR_MPII14, estimate_people
    from pose.estimate_pose import _scale_group

    net = gpu_caffe.Net(deepercut_prototxt(152, 88, 120), synth152[0], gpu_caffe.TEST, from_text=True)
    img = np.random.RandomState(4).randint(0, 256, (85, 115, 3)).astype(np.uint8)
    kw = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
    stats = (EDGES, MEAN, STD)

    def by_hand(scales, base):
        k = len(scales)
        grp = _scale_group(net, 2 * k)
        flags = [0] * k + [1] * k
        grp.forward_images(img, scales * 2, want=(), pose=False, mirror=flags)
        return grp.assemble_people(scales * 2, base, edges=EDGES, mean=MEAN, std=STD, mirror=flags, image_width=115, joint_mirror=MIRROR_MPII14,
                                   **kw)[0]["people"]

    got = estimate_people(img, None, None, stats, net=net, scales=[1.3, 1.0], flip=True, **kw)
    want = by_hand([1.3, 1.0], 1)
    assert got.shape == want.shape and got.shape[1:] == (14, 3) and np.array_equal(got, want)
    assert np.array_equal(estimate_people(img, None, None, stats, net=net, scales=[1.3, 1.0], base=0, flip=True, **kw), by_hand([1.3, 1.0], 0))
    one = estimate_people(img, None, None, stats, net=net, scale=0.8, flip=True, **kw)
    assert np.array_equal(one, by_hand([0.8], 0))
    # without the flip: the unmirrored entries, as before
    plain = estimate_people(img, None, None, stats, net=net, scales=[1.3, 1.0], **kw)
    grp = _scale_group(net, 2)
    grp.forward_images(img, [1.3, 1.0], want=(), pose=False)
    assert np.array_equal(plain, grp.assemble_people([1.3, 1.0], 1, edges=EDGES, mean=MEAN, std=STD, **kw)[0]["people"])


def test_errors_leave_the_group_usable(forwarded_f32, gpu_caffe):
    """Every refusal of the mirrored entries, on a group that holds a forward: DC_EINVAL naming what is wrong, nothing launched, and the
    next good call gives what it gave before."""
    kind, grp, _, _ = forwarded_f32
    before = grp.fuse_maps(SCALES, 1, MEAN, STD, edges=EDGES, **MKW)
    swapped, far = list(PI), list(PI)
    swapped[0], swapped[1] = 4, 4
    far[3] = 14
    one_way = R.one_direction_edges(14)  # a -> c with a < c only: (0, 1) has no mirrored edge (5, 4)
    bad = [
        (dict(MKW, image_width=0), "image_width"),
        (dict(MKW, image_width=-117), "image_width"),
        (dict(MKW, joint_mirror=None), "joint_mirror"),
        (dict(MKW, joint_mirror=far), "joint_mirror[3]"),
        (dict(MKW, joint_mirror=swapped), "involution"),
        (dict(MKW, mirror=(0, 1, 1, 0)), "mirrored"),  # base 1 is mirrored
    ]
    calls = {
        "fuse_maps": lambda kw, **e: grp.fuse_maps(SCALES, 1, MEAN, STD, **dict(dict(edges=EDGES, **kw), **e)),
        "detect_parts": lambda kw, **e: grp.detect_parts(SCALES, 1, 0.5, 1, 8, **kw),
        "assemble_people": lambda kw, **e: grp.assemble_people(SCALES, 1, **dict(dict(edges=EDGES, mean=MEAN, std=STD, max_cost=40.0, **kw), **e)),
    }
    for name, call in calls.items():
        for kw, word in bad:
            with pytest.raises(gpu_caffe.DeepcutError) as ei:
                call(kw)
            assert ei.value.code == -1 and word in str(ei.value), (name, word, str(ei.value))
    # the edges: a mirrored edge that is missing, another count than the call's, none at all
    for e, word in ((one_way, "no mirrored edge"), (EDGES[:-1], "181 edges"), (None, "0 edges")):
        with pytest.raises(gpu_caffe.DeepcutError) as ei:
            calls["fuse_maps"](MKW, edges=e)
        assert ei.value.code == -1 and word in str(ei.value), (word, str(ei.value))
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        calls["assemble_people"](MKW, edges=one_way)
    assert ei.value.code == -1 and "no mirrored edge" in str(ei.value)
    # what the unmirrored call refuses is refused in the same way
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        grp.fuse_maps((1.0, -0.7, 1.0, 0.7), 1, MEAN, STD, edges=EDGES, **MKW)
    assert ei.value.code == -1 and "scale of member 1" in str(ei.value)
    after = grp.fuse_maps(SCALES, 1, MEAN, STD, edges=EDGES, **MKW)
    assert all(np.array_equal(before[k], after[k]) for k in ALL)
