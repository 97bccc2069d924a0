"""-m gpu: fused multi-scale and mirrored poses for the single-person entry and the box entry — dc_group_decode_pose,
dc_group_forward_boxes_mirrored (the flip inside the box pre-processing) and dc_group_decode_boxes (every box's own reflected column in
the fusion kernel, then the restricted decode on the fused maps) — against the host-flipped image, the restatement in
tests/boxfuse_ref.py and `pose.estimate_pose`'s own decoders.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn keeps the best single scale (estimate_pose.py:119-126), fuses no maps and mirrors
nothing, so there is no reference output to hold the rule to.  The rule is this project's own (include/deepcut_hip.h); what is proven
here is that the flipped box pre-processing is bit for bit the unflipped one of the flipped image with reflected boxes, that the device
fuses what its restatement fuses within the float32 bound the restatement derives (16 * 2^-24 * A), and that the poses are the
decoders' own on the device's fused maps."""
import ctypes as C

import numpy as np
import pytest

import boxfuse_ref as BF
import flip_ref as FL
from pose import estimate_pose as ep

pytestmark = pytest.mark.gpu

PI = FL.MIRROR_MPII14
MAPS = ("prob", "loc_pred")

# ---- the box entry: one 96 x 131 image, three boxes of odd, different widths (61, 91, 31: ws is never cell-aligned and differs per box);
# box 1 touches three image edges.  Pyramid (1.0, 0.7): the pre-processing takes both resample passes and the no-resample branch.
IMG = np.random.RandomState(41).randint(0, 256, (96, 131, 3)).astype(np.uint8)
BOXES = [(3, 5, 64, 90), (40, 0, 131, 96), (70, 20, 101, 77)]
BSCALES = [1.0, 0.8, 1.3]
PYR = (1.0, 0.7, 1.0, 0.7)
MIRROR = (0, 0, 1, 1)
W = IMG.shape[1]
REFLECTED = [(W - x1, y0, W - x0, y1) for x0, y0, x1, y1 in BOXES]
KINDS = {"f32": dict(), "f16": dict(dtype="f16"), "bf16": dict(dtype="bf16")}

_boxed = {}


def _boxes_forwarded(kind, gpu_caffe, synth152):
    """Per kind of member, once per module: a group of four, what ONE grouped forward_boxes of the host-flipped image with reflected
    boxes left in the members (inputs and maps), and then the same after ONE grouped forward_boxes of IMG with the last two members
    mirrored on the device — whose maps the members still hold.  Never written to."""
    if kind not in _boxed:
        from deepcut_tools import deepercut_prototxt

        net = gpu_caffe.Net(deepercut_prototxt(152, 88, 80, 3), synth152[0], gpu_caffe.TEST, from_text=True, **KINDS[kind])
        grp = gpu_caffe.NetGroup([net] + [net.clone() for _ in range(3)])
        flipped = np.ascontiguousarray(IMG[:, ::-1])
        state = []
        for image, boxes, kw in ((flipped, REFLECTED, dict()), (IMG, BOXES, dict(mirror=MIRROR))):
            outs = grp.forward_boxes(image, boxes, PYR, BSCALES, want=MAPS, pose=True, **kw)
            state.append(([m.blobs["data"].data.copy() for m in grp.nets], [tuple(o[k].copy() for k in MAPS) for o in outs], outs))
        _boxed[kind] = (kind, grp, state[0], state[1])
    return _boxed[kind]


@pytest.fixture(scope="module", params=list(KINDS))
def boxed(request, gpu_caffe, synth152):
    return _boxes_forwarded(request.param, gpu_caffe, synth152)


@pytest.fixture(scope="module", params=["f32", "bf16"])
def boxed_f32_bf16(request, gpu_caffe, synth152):
    return _boxes_forwarded(request.param, gpu_caffe, synth152)


@pytest.fixture(scope="module")
def boxed_f32(gpu_caffe, synth152):
    yield _boxes_forwarded("f32", gpu_caffe, synth152)
    _boxed.clear()


def test_mirrored_box_preprocessing_is_the_plain_one_of_the_flipped_image(boxed):
    """A mirrored member's `data` blob and maps, bit for bit, for float32, float16 and bfloat16 members, with both resample passes
    (0.7, and box scales 0.8 and 1.3 at 1.0) and without one (box 0 at 1.0)."""
    kind, grp, (host_data, host_maps, host_outs), (dev_data, dev_maps, dev_outs) = boxed
    assert [m[0].shape for m in dev_maps] == [(3, 14, 11, 10), (3, 14, 8, 7)] * 2
    for m in (2, 3):
        assert host_data[m].shape == dev_data[m].shape and np.array_equal(host_data[m], dev_data[m]), (kind, "data", m)
        for k, name in enumerate(MAPS):
            assert np.array_equal(host_maps[m][k], dev_maps[m][k]), (kind, name, m)
    # the flip is a flip: box 0 at scale 1.0 is the crop's own pixels reversed, and the mirrored member's input is not the plain one's
    assert np.array_equal(dev_data[0][0][:, :85, :61], dev_data[2][0][:, :85, 60::-1])
    assert not np.array_equal(dev_data[1], dev_data[3]) and not np.array_equal(dev_maps[0][0], dev_maps[2][0])
    # "pose" is absent when a member is mirrored, present otherwise
    assert all("pose" not in o for o in dev_outs) and all("pose" in o for o in host_outs)


def test_fused_box_maps_match_the_restatement(boxed_f32_bf16):
    """decode_boxes' fused prob / loc_pred against boxfuse_ref on the members' own returned maps: both plain bases, float32 and bfloat16
    members; a repeat call returns the same bits; and every box has its own reflected column."""
    kind, grp, _, (_, maps, _) = boxed_f32_bf16
    ws = BF.box_ws(BOXES, BSCALES, PYR)
    for base in (0, 1):
        ref, a = BF.fuse(maps, PYR, base, MIRROR, ws, PI)
        got = grp.decode_boxes(PYR, base, mirror=MIRROR, joint_mirror=PI, want=MAPS)
        again = grp.decode_boxes(PYR, base, mirror=MIRROR, joint_mirror=PI, want=MAPS)
        wrong, wa = BF.fuse(maps, PYR, base, MIRROR, [[r[0]] * len(BOXES) for r in ws], PI)
        for k, name in enumerate(MAPS):
            assert got[name].dtype == np.float32 and got[name].shape == ref[k].shape
            ratio = BF.worst_ratio(got[name], ref[k], a[k])
            print("%s, base %d, %s: worst |device - restatement| / (16 * 2^-24 * A) = %.4f" % (kind, base, name, ratio))
            assert ratio <= 1.0
            assert np.array_equal(got[name].view(np.uint32), again[name].view(np.uint32))
            assert BF.worst_ratio(got[name], wrong[k], wa[k]) > 1.0, "fused with every ws set to box 0's is something else"
            assert BF.worst_ratio(got[name][0], wrong[k][0], wa[k][0]) <= 1.0  # (box 0 itself is reflected about its own width either way)
        assert np.array_equal(got["pose"], again["pose"])


def test_box_poses_are_the_restricted_decode_of_the_devices_own_fused_maps(boxed_f32_bf16):
    """The bar tests/test_gpu_boxes.py holds the unfused entry to: box_pose_from_maps at scales[i] * pyramid[base], atol 1e-9."""
    kind, grp, _, _ = boxed_f32_bf16
    for base in (0, 1):
        got = grp.decode_boxes(PYR, base, mirror=MIRROR, joint_mirror=PI, want=MAPS)
        want = BF.box_poses(got["prob"], got["loc_pred"], BOXES, BSCALES, PYR[base])
        assert got["pose"].shape == want.shape == (3, 5, 14)
        err = float(np.abs(got["pose"] - want).max())
        print("%s, base %d: max |device pose - box_pose_from_maps of the fused maps| = %.3e" % (kind, base, err))
        assert np.allclose(got["pose"], want, rtol=0, atol=1e-9)
        # pose alone, or one map alone: the same numbers
        assert np.array_equal(grp.decode_boxes(PYR, base, mirror=MIRROR, joint_mirror=PI)["pose"], got["pose"])
        one = grp.decode_boxes(PYR, base, mirror=MIRROR, joint_mirror=PI, want=("loc_pred",))
        assert sorted(one) == ["loc_pred", "pose"] and np.array_equal(one["loc_pred"], got["loc_pred"])


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_no_mirrored_member_is_todays_box_entry_bit_for_bit(boxed_f32, gpu_caffe):
    """forward_boxes(mirror = all zero) and the raw dc_group_forward_boxes_mirrored with zero flags and with NULL: the members' inputs,
    maps and poses of forward_boxes; a group of one member decodes to that member's own forward_boxes pose."""
    import caffe.pycaffe as pc

    kind, grp, _, _ = boxed_f32
    pair = gpu_caffe.NetGroup(grp.nets[:2])
    pyr = PYR[:2]
    want = pair.forward_boxes(IMG, BOXES, pyr, BSCALES, want=MAPS, pose=True)
    want = [{k: v.copy() for k, v in o.items()} for o in want]
    want_data = [m.blobs["data"].data.copy() for m in pair.nets]
    got = pair.forward_boxes(IMG, BOXES, pyr, BSCALES, want=MAPS, pose=True, mirror=(0, 0))
    for m in range(2):
        assert np.array_equal(pair.nets[m].blobs["data"].data, want_data[m])
        assert sorted(got[m]) == ["loc_pred", "pose", "prob"] and all(np.array_equal(got[m][k], want[m][k]) for k in want[m])
    b, sc, cv = gpu_caffe.check_boxes(IMG.shape, BOXES, BSCALES)
    for flags in (np.zeros(2, np.int32), None):
        outs = [{k: np.full_like(want[m][k], np.nan) for k in MAPS} for m in range(2)]
        col = lambda k: (C.c_void_p * 2)(*[o[k].ctypes.data for o in outs])  # noqa: E731
        rc = pc._lib.dc_group_forward_boxes_mirrored(pair._h, _vp(IMG), IMG.shape[0], IMG.shape[1], 0, _vp(b), _vp(sc), len(BOXES),
                                                     (C.c_double * 2)(*pyr), cv[0], cv[1], _vp(flags), col("prob"), col("loc_pred"), None, None)
        assert rc == 0, pc._lib.dc_last_error()
        for m in range(2):
            assert np.array_equal(pair.nets[m].blobs["data"].data, want_data[m])
            assert all(np.array_equal(outs[m][k].view(np.uint32), want[m][k].view(np.uint32)) for k in MAPS)
    # fm NULL and all-zero flags: the unmirrored fusion, the same bits
    plain = pair.decode_boxes(pyr, 0, want=MAPS)
    zero = pair.decode_boxes(pyr, 0, mirror=(0, 0), want=MAPS)
    assert all(np.array_equal(plain[k], zero[k]) for k in plain)
    assert np.allclose(plain["pose"], BF.box_poses(plain["prob"], plain["loc_pred"], BOXES, BSCALES, pyr[0]), rtol=0, atol=1e-9)
    # a group of one: the member's own maps widened to float32, and its own pose
    solo = gpu_caffe.NetGroup([grp.nets[1]])
    own = solo.forward_boxes(IMG, BOXES, (0.7,), BSCALES, want=MAPS, pose=True)[0]
    own = {k: v.copy() for k, v in own.items()}
    dec = solo.decode_boxes((0.7,), 0, want=MAPS)
    assert np.array_equal(dec["prob"], own["prob"]) and np.array_equal(dec["loc_pred"], own["loc_pred"])
    assert np.array_equal(dec["pose"], own["pose"])
    # (the four members of the module's group hold the mirrored forward again for the tests that follow)
    grp.forward_boxes(IMG, BOXES, PYR, BSCALES, want=(), pose=False, mirror=MIRROR)


def test_box_refusals_leave_the_group_usable(boxed_f32, gpu_caffe):
    kind, grp, _, _ = boxed_f32
    kw = dict(mirror=MIRROR, joint_mirror=PI)
    before = grp.decode_boxes(PYR, 1, want=MAPS, **kw)
    swapped, far = list(PI), list(PI)
    swapped[0], swapped[1] = 4, 4
    far[3] = 14
    bad = [
        (dict(kw, joint_mirror=None), "joint_mirror"),
        (dict(kw, joint_mirror=far), "joint_mirror[3]"),
        (dict(kw, joint_mirror=swapped), "involution"),
        (dict(kw, mirror=(0, 1, 1, 0)), "base member 1 is mirrored"),
        (dict(kw, mirror=None), "member 2 is not marked as mirrored"),
        (dict(kw, mirror=(0, 0, 0, 1)), "member 2 is not marked as mirrored"),
        (dict(kw, mirror=(1, 0, 1, 1)), "member 0 is marked as mirrored"),
    ]
    for args, word in bad:
        with pytest.raises(gpu_caffe.DeepcutError) as ei:
            grp.decode_boxes(PYR, 1, **args)
        assert ei.value.code == -1 and word in str(ei.value), (word, str(ei.value))
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        grp.decode_boxes((1.0, -0.7, 1.0, 0.7), 1, **kw)
    assert ei.value.code == -1 and "scale of member 1" in str(ei.value)
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        grp.decode_boxes(PYR, 4, **kw)
    assert ei.value.code == -1 and "base 4 is outside" in str(ei.value)
    after = grp.decode_boxes(PYR, 1, want=MAPS, **kw)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a member that holds other boxes than the rest is named; the group's next forward and decode are what they were
    b, sc, cv = gpu_caffe.check_boxes(IMG.shape, BOXES, BSCALES)
    grp.nets[1].forward_boxes(IMG, BOXES[:2], np.asarray(BSCALES[:2]) * 0.7, canvas=(gpu_caffe.member_canvas(cv[0], 0.7), gpu_caffe.member_canvas(cv[1], 0.7)),
                              want=(), pose=False)
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        grp.decode_boxes(PYR, 1, **kw)
    assert ei.value.code == -1 and "member 1 holds 2 boxes" in str(ei.value), str(ei.value)
    grp.forward_boxes(IMG, BOXES, PYR, BSCALES, want=(), pose=False, mirror=MIRROR)
    again = grp.decode_boxes(PYR, 1, want=MAPS, **kw)
    for k in MAPS:  # (the member re-lowered its own plan in between: the group's merged launches may sum in another tile order)
        assert float(np.abs(again[k] - before[k]).max()) <= 1e-4 * max(1.0, float(np.abs(before[k]).max())), k


# ---- the image entry: 88 x 117 images, batch 2, as tests/test_gpu_flip.py ---------------------------------------------------------------
IMGS = np.random.RandomState(37).randint(0, 256, (2, 88, 117, 3)).astype(np.uint8)
ISCALES = (1.0, 0.7, 1.0, 0.7)
IKW = dict(mirror=MIRROR, image_width=IMGS.shape[2], joint_mirror=PI)


def _image_group(caffe, path, image_hw, scales, n=1, **kw):
    from deepcut_tools import deepercut_prototxt

    shapes = [(n,) + tuple(caffe.canvas_size(image_hw[0], image_hw[1], s)) for s in scales]
    net = caffe.Net(deepercut_prototxt(152, shapes[0][1], shapes[0][2], n), path, caffe.TEST, from_text=True, **kw)
    return caffe.NetGroup.for_shapes(net, shapes)


@pytest.fixture(scope="module")
def image_group(gpu_caffe, synth152):
    """DC_OPT_FUSE 0 members (separate map tensors, writable through `.data`), float32."""
    return _image_group(gpu_caffe, synth152[0], IMGS.shape[1:3], ISCALES, n=2, fuse=0)


def test_decode_pose_is_pose_from_maps_of_the_fused_maps(image_group, gpu_caffe):
    grp = image_group
    outs = grp.forward_images(IMGS, ISCALES, want=MAPS, pose=False, mirror=MIRROR)
    maps = [tuple(o[k].copy() for k in MAPS) for o in outs]
    for base in (0, 1):
        for kw in (IKW, dict()):
            fused = grp.fuse_maps(ISCALES, base, want=MAPS, **kw)
            pose = grp.decode_pose(ISCALES, base, **kw)
            assert pose.shape == (2, 5, 14)
            for b in range(2):
                want = ep.pose_from_maps(fused["prob"][b], fused["loc_pred"][b], ISCALES[base])
                assert np.allclose(pose[b], want, rtol=0, atol=1e-9), (base, bool(kw), b)
            assert np.array_equal(pose, grp.decode_pose(ISCALES, base, **kw))
    assert not np.array_equal(grp.decode_pose(ISCALES, 0, **IKW), grp.decode_pose(ISCALES, 0))
    # the per-image flip record leaves fuse_maps(mirror=...) what it was: within the bound of flip_ref ...
    fused = grp.fuse_maps(ISCALES, 0, want=MAPS, **IKW)
    ref, a = FL.fuse([m + (None,) for m in maps], ISCALES, 0, MIRROR, IMGS.shape[2], PI)
    for k, name in enumerate(MAPS):
        ratio = FL.worst_ratio(fused[name], ref[k], a[k])
        print("image entry, %s: worst |device - restatement| / (16 * 2^-24 * A) = %.4f" % (name, ratio))
        assert ratio <= 1.0
    # ... and entry 0 of the batch of two is, bit for bit, a batch of one holding the same maps
    before = grp.decode_pose(ISCALES, 0, **IKW)
    swapped = list(PI)
    swapped[0], swapped[1] = 4, 4
    for kw, word in ((dict(IKW, image_width=0), "image_width"), (dict(IKW, joint_mirror=swapped), "involution"), (dict(IKW, mirror=(1, 0, 1, 1)), "mirrored")):
        with pytest.raises(gpu_caffe.DeepcutError) as ei:
            grp.decode_pose(ISCALES, 0, **kw)
        assert ei.value.code == -1 and word in str(ei.value)
    assert np.array_equal(before, grp.decode_pose(ISCALES, 0, **IKW))
    grp.forward_images(IMGS[:1], ISCALES, want=(), pose=False, mirror=MIRROR)
    for net, mm in zip(grp.nets, maps):
        for k, name in enumerate(MAPS):
            assert net.blobs[name].shape[0] == 1
            net.blobs[name].data[...] = mm[k][:1]
    single = grp.fuse_maps(ISCALES, 0, want=MAPS, **IKW)
    for name in MAPS:
        assert np.array_equal(single[name].view(np.uint32), fused[name][:1].view(np.uint32)), name
    assert np.array_equal(grp.decode_pose(ISCALES, 0, **IKW)[0], before[0])


def test_decode_pose_on_members_narrowed_to_prob_and_loc_pred(gpu_caffe, synth152):
    grp = _image_group(gpu_caffe, synth152[0], IMGS.shape[1:3], ISCALES, n=2)
    for net in grp.nets:
        net.set_outputs(["loc_pred", "prob"])
    grp.forward_images(IMGS, ISCALES, want=(), pose=False, mirror=MIRROR)
    assert all("next_pred" not in net.wanted_outputs for net in grp.nets)
    fused = grp.fuse_maps(ISCALES, 0, want=MAPS, **IKW)
    pose = grp.decode_pose(ISCALES, 0, **IKW)
    for b in range(2):
        assert np.allclose(pose[b], ep.pose_from_maps(fused["prob"][b], fused["loc_pred"][b], ISCALES[0]), rtol=0, atol=1e-9)


@pytest.mark.parametrize("dtype,sixteen_bit", [("f32", False), ("bf16", True)])
def test_planted_mirrored_pyramid_decodes_to_the_highest_person(gpu_caffe, synth152, dtype, sixteen_bit):
    """flip_ref.planted(...) written into the members.  On the restatement alone: every joint's global maximum of the fused `prob` is a
    planted cell — that of the person whose fused peak is the highest for this joint — by at least 1e-3 over every other cell.  (Which
    person that is differs per joint: the three peaks are 0.9, 0.85 and 0.8, and the bilinear samples of the 0.7 and mirrored members take
    up to 0.06 off a peak depending on where it falls between their cells; person 0 is on top for no joint of this scene.)  decode_pose
    then returns that person's planted joints."""
    sc = FL.planted(sixteen_bit)
    fp = sc["fused"][0][0]
    who = []
    for j in range(14):
        q = int(np.argmax([fp[j][sc["cells"][p][j]] for p in range(3)]))
        r, c = sc["cells"][q][j]
        rest = fp[j].copy()
        rest[r, c] = -np.inf
        assert fp[j, r, c] - rest.max() >= 1e-3, (j, q, fp[j, r, c], rest.max())
        who.append(q)
    assert len(set(who)) > 1  # (the answer is not one person's pose: the fused maps decide joint by joint)
    grp = _image_group(gpu_caffe, synth152[0], FL.IMAGE_HW, FL.SCALES, fuse=0, dtype=dtype)
    img = np.random.RandomState(8).randint(0, 256, FL.IMAGE_HW + (3,)).astype(np.uint8)
    grp.forward_images(img, FL.SCALES, want=(), pose=False, mirror=FL.MIRROR)
    assert grp.nets[0].dtype == dtype
    for net, maps in zip(grp.nets, sc["maps"]):
        for k, name in enumerate(("prob", "loc_pred", "next_pred")):
            assert net.blobs[name].shape[2:] == maps[k].shape[2:]
            net.blobs[name].data[...] = maps[k]
    pose = grp.decode_pose(FL.SCALES, FL.BASE, mirror=FL.MIRROR, image_width=FL.IMAGE_HW[1], joint_mirror=PI)[0]
    truth = np.array([sc["truth"][who[j]][j] for j in range(14)])
    err = float(np.abs(pose[:2].T - truth).max())
    print("planted mirrored pyramid (%s): max |decoded joint - planted joint| = %.3e px" % (dtype, err))
    assert err <= (1.0 if sixteen_bit else 1e-4)
    rows, cols = ep.pose_cells(pose, FL.SCALES[FL.BASE])
    assert [(int(r), int(c)) for r, c in zip(rows, cols)] == [tuple(sc["cells"][who[j]][j]) for j in range(14)]
    assert np.allclose(pose[2], [fp[j][sc["cells"][who[j]][j]] for j in range(14)], rtol=0, atol=1e-5)


def test_estimate_pose_and_estimate_poses_fused_and_flipped(gpu_caffe, synth152):
    """fuse=True, flip=True = the by-hand sequence of group calls (plain members, then their mirrors; base: the plain scale nearest 1.0);
    the defaults return what they returned."""
    from deepcut_tools import deepercut_prototxt
    from pose import MIRROR_MPII14
    from pose.estimate_pose import _scale_group, estimate_pose, estimate_poses

    net = gpu_caffe.Net(deepercut_prototxt(152, 96, 136), synth152[0], gpu_caffe.TEST, from_text=True)
    scales, four, flags = [0.7, 1.0], [0.7, 1.0, 0.7, 1.0], [0, 0, 1, 1]
    got = estimate_pose(IMG, None, None, scales=scales, net=net, fuse=True, flip=True)
    grp = _scale_group(net, 4)
    grp.forward_images(IMG, four, want=(), pose=False, mirror=flags)
    want = grp.decode_pose(four, 1, mirror=flags, image_width=W, joint_mirror=MIRROR_MPII14)[0]
    assert got.shape == (5, 14) and np.array_equal(got, want)
    assert np.array_equal(estimate_pose(IMG, None, None, scales=scales, net=net, flip=True, base=0),
                          grp.decode_pose(four, 0, mirror=flags, image_width=W, joint_mirror=MIRROR_MPII14)[0])
    fused_only = estimate_pose(IMG, None, None, scales=scales, net=net, fuse=True)
    two = _scale_group(net, 2)
    two.forward_images(IMG, scales, want=(), pose=False)
    assert np.array_equal(fused_only, two.decode_pose(scales, 1)[0]) and not np.array_equal(fused_only, got)
    # the default: select_best over the per-scale poses, as before
    plain = estimate_pose(IMG, None, None, scales=scales, net=net)
    outs = two.forward_images(IMG, scales, want=(), pose=True)
    best = ep.select_best([o["pose"][0] for o in outs])
    assert (plain is None) == (best is None) and (plain is None or np.array_equal(plain, best))
    # the box entry
    poses = estimate_poses(IMG, BOXES, None, None, scales=scales, net=net, fuse=True, flip=True)
    b, _, cv = gpu_caffe.check_boxes(IMG.shape, BOXES, 1.0)
    grp.forward_boxes(IMG, b, four, canvas=cv, want=(), pose=False, mirror=flags)
    by_hand = grp.decode_boxes(four, 1, mirror=flags, joint_mirror=MIRROR_MPII14)["pose"]
    assert len(poses) == 3 and all(np.array_equal(p, q) for p, q in zip(poses, by_hand))
    plain = estimate_poses(IMG, BOXES, None, None, scales=scales, net=net)
    outs = two.forward_boxes(IMG, b, scales, canvas=cv, want=(), pose=True)
    for i in range(3):
        best = ep.select_best([o["pose"][i] for o in outs])
        assert (plain[i] is None) == (best is None) and (best is None or np.array_equal(plain[i], best))
