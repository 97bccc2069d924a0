"""-m gpu: the box entry (dc_net_forward_boxes / dc_group_forward_boxes) — top-down poses for the person boxes of one image.

Pinned semantics (tests/test_boxes_host.py builds them on the host): the `data` blob holds, bit for bit, the demo's
pre-processing of every host-cut crop on a common zero canvas (`estimate_pose.box_canvases`); the maps are `net.forward()` of that
batch; pose i is `pose_from_maps` on the crop's own cells, shifted by the box corner (`estimate_pose.box_pose_from_maps`)."""
import ctypes as C
import os

import numpy as np
import pytest

from pose import estimate_pose as ep
from test_gpu_tiling import _fill, local_fcn_prototxt

pytestmark = pytest.mark.gpu
DC_EINVAL = -1

IMG = np.random.RandomState(17).randint(0, 256, (120, 160, 3)).astype(np.uint8)
IMG[:40, 100:] = 250  # flat patches: clipping at 255 and exact replicas in the resample
IMG[80:, :30] = 3
BOXES = [(0, 0, 160, 120), (0, 0, 37, 53), (101, 77, 160, 120), (50, 60, 51, 61), (10, 119, 150, 120), (159, 0, 160, 120),
         (20, 30, 90, 100), (33, 7, 70, 31)]
SCALES = [0.5, 1.0, 1.3, 1.0, 0.8, 1.1, 1.7, 0.61]


def _net(caffe, dtype="f32"):
    net = caffe.Net(local_fcn_prototxt(64, 64), caffe.TEST, from_text=True, dtype=dtype)
    _fill(net, 5)
    return net


@pytest.fixture(scope="module")
def nets(gpu_caffe):
    return {d: _net(gpu_caffe, d) for d in ("f32", "f16", "bf16")}


def _as_elem(x, dtype):
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        import torch

        return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    return x


def _host_batch(boxes, scales, canvas):
    return ep.box_canvases(IMG, boxes, scales, canvas).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_data_blob_is_the_host_construction_bit_for_bit(gpu_caffe, nets, dtype):
    net = nets[dtype]
    b, sc, cv = gpu_caffe.check_boxes(IMG.shape, BOXES, SCALES)
    net.forward_boxes(IMG, BOXES, SCALES, want=(), pose=False)
    got = net.blobs["data"].data
    want = _as_elem(np.ascontiguousarray(_host_batch(b, sc, cv)), dtype)
    assert got.shape == want.shape == (len(BOXES), 3) + cv
    for i in range(len(BOXES)):
        assert np.array_equal(got[i], want[i]), "box %d" % i
    # a larger canvas than needed: the same crops, more zeros
    net.forward_boxes(IMG, BOXES[1:4], SCALES[1:4], canvas=(cv[0] + 16, cv[1] + 8), want=(), pose=False)
    assert np.array_equal(net.blobs["data"].data, _as_elem(_host_batch(b[1:4], sc[1:4], (cv[0] + 16, cv[1] + 8)), dtype))


def test_maps_and_poses_equal_the_classic_entry_on_the_host_batch(gpu_caffe, nets):
    net = nets["f32"]
    b, sc, cv = gpu_caffe.check_boxes(IMG.shape, BOXES, SCALES)
    out = net.forward_boxes(IMG, BOXES, SCALES, want=("prob", "loc_pred"), pose=True)
    assert out["prob"].shape == (len(BOXES), 14, cv[0] // 8, cv[1] // 8) and out["pose"].shape == (len(BOXES), 5, 14)
    net.blobs["data"].reshape(*((len(BOXES), 3) + cv))
    net.blobs["data"].data[...] = _host_batch(b, sc, cv)
    net.forward()  # same net, same shape, same plan
    prob, loc = net.blobs["prob"].data.copy(), net.blobs["loc_pred"].data.copy()
    assert np.array_equal(out["prob"], prob) and np.array_equal(out["loc_pred"], loc)
    for i in range(len(BOXES)):
        want = ep.box_pose_from_maps(prob[i], loc[i], b[i], sc[i])
        assert np.allclose(out["pose"][i], want, rtol=0, atol=1e-9), i


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_16bit_poses_follow_their_own_maps(nets, dtype):
    out = nets[dtype].forward_boxes(IMG, BOXES, SCALES, want=("prob", "loc_pred"), pose=True)
    for i in range(len(BOXES)):
        want = ep.box_pose_from_maps(out["prob"][i], out["loc_pred"][i], BOXES[i], SCALES[i])
        assert np.allclose(out["pose"][i], want, rtol=0, atol=1e-9), i


def test_small_box_never_decodes_outside_its_own_cells(nets):
    # a 1 x 1 box (one 8 x 8 canvas: one map cell) beside the whole image: its row of the batch covers a 15 x 20 map, whose
    # unrestricted arg-max lies elsewhere for most joints; the decode must still return the one cell the crop has
    net = nets["f32"]
    boxes, scales = [(0, 0, 160, 120), (50, 60, 51, 61), (3, 5, 20, 14)], [1.0, 1.0, 1.0]
    out = net.forward_boxes(IMG, boxes, scales, want=("prob", "loc_pred"), pose=True)
    prob, loc = out["prob"], out["loc_pred"]
    assert prob.shape[2:] == (15, 20)
    for i, (rows_own, cols_own) in ((1, (1, 1)), (2, (2, 3))):
        free = ep.pose_from_maps(prob[i], loc[i], 1.0)
        fr, fc = ep.pose_cells(free, 1.0)
        assert ((fr >= rows_own) | (fc >= cols_own)).sum() >= 4, "the case must put unrestricted maxima outside"
        pose = out["pose"][i]
        rr, cc = ep.pose_cells(pose - np.array([[boxes[i][0]], [boxes[i][1]], [0], [0], [0]]), 1.0)
        assert (rr >= 0).all() and (rr < rows_own).all() and (cc >= 0).all() and (cc < cols_own).all()
        assert np.allclose(pose, ep.box_pose_from_maps(prob[i], loc[i], boxes[i], 1.0), rtol=0, atol=1e-9)
        assert not np.allclose(pose[0] - boxes[i][0], free[0])


def test_device_pointer_form_equals_host_form(gpu_caffe, nets):
    import torch

    net = nets["f32"]
    host = net.forward_boxes(IMG, BOXES, SCALES, want=("prob", "loc_pred"), pose=True)
    _, _, cv = gpu_caffe.check_boxes(IMG.shape, BOXES, SCALES)
    img = torch.from_numpy(IMG).cuda()
    prob = torch.empty(host["prob"].shape, dtype=torch.float32, device="cuda")
    loc = torch.empty(host["loc_pred"].shape, dtype=torch.float32, device="cuda")
    pose = torch.empty(host["pose"].shape, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    net.forward_boxes_device(img.data_ptr(), IMG.shape[0], IMG.shape[1], BOXES, SCALES, cv, prob.data_ptr(), loc.data_ptr(), None,
                             pose.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(prob.cpu().numpy(), host["prob"]) and np.array_equal(loc.cpu().numpy(), host["loc_pred"])
    assert np.array_equal(pose.cpu().numpy(), host["pose"])


def test_group_over_four_scales_equals_four_single_calls(gpu_caffe, nets):
    from pose.estimate_pose import _scale_group

    net = nets["f32"]
    pyramid = [0.5, 0.75, 1.0, 1.25]
    b, sc, cv = gpu_caffe.check_boxes(IMG.shape, BOXES[1:], 1.0)
    grp = _scale_group(net, 4)
    outs = grp.forward_boxes(IMG, BOXES[1:], pyramid, want=("prob", "loc_pred"), pose=True)
    datas = [m.blobs["data"].data.copy() for m in grp.nets]
    for c, p in enumerate(pyramid):
        mc = (gpu_caffe.member_canvas(cv[0], p), gpu_caffe.member_canvas(cv[1], p))
        one = net.forward_boxes(IMG, BOXES[1:], sc * p, canvas=mc, want=("prob", "loc_pred"), pose=True)
        assert np.array_equal(datas[c], net.blobs["data"].data), c  # the member's canvases are the single call's, bit for bit
        assert outs[c]["prob"].shape == one["prob"].shape
        # the group's merged launches may sum in another tile order than the single net's
        assert float(np.abs(outs[c]["prob"] - one["prob"]).max()) <= 1e-4
        assert float(np.abs(outs[c]["loc_pred"] - one["loc_pred"]).max()) <= 1e-4 * max(1.0, float(np.abs(one["loc_pred"]).max()))
        for i in range(len(b)):
            g, s = outs[c]["pose"][i], one["pose"][i]
            assert np.allclose(g, ep.box_pose_from_maps(outs[c]["prob"][i], outs[c]["loc_pred"][i], b[i], sc[i] * p), rtol=0, atol=1e-9)
            assert np.allclose(g[2], s[2], rtol=0, atol=1e-4)
            # a joint whose cell moved must have moved to a cell that ties with the single call's maximum to that tolerance
            shift = np.array([[b[i][0]], [b[i][1]], [0], [0], [0]])
            gr, gc = ep.pose_cells(g - shift, sc[i] * p)
            sr, scl = ep.pose_cells(s - shift, sc[i] * p)
            jj = np.arange(14)
            assert (one["prob"][i][jj, gr, gc] >= one["prob"][i][jj, sr, scl] - 1e-4).all()
            same = (gr == sr) & (gc == scl)
            assert np.abs(g[:, same] - s[:, same]).max(initial=0.0) <= 1e-2


def _c_forward(caffe, net, boxes, scales, canvas):
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, np.float64), (b.shape[0],)))
    return caffe.pycaffe._lib.dc_net_forward_boxes(net._h, IMG.ctypes.data_as(C.c_void_p), IMG.shape[0], IMG.shape[1], 0,
                                                   b.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), b.shape[0], canvas[0],
                                                   canvas[1], None, None, None, None, None)


@pytest.mark.parametrize("boxes,canvas,msg", [
    ([(0, 0, 8, 8), (9, 9, 9, 20)], (64, 64), "box 1 .* is empty"),
    ([(0, 0, 8, 8), (150, 0, 161, 10)], (64, 64), "box 1 .* outside"),
    ([(0, -2, 8, 8)], (64, 64), "box 0 .* outside"),
    ([(0, 0, 8, 8), (0, 0, 100, 20)], (64, 64), "box 1 .* needs a 24x104 canvas"),
    ([(0, 0, 8, 8)], (64, 60), "not a positive multiple of 8"),
])
def test_errors_name_the_box_before_any_device_work(gpu_caffe, nets, boxes, canvas, msg):
    import re

    net = nets["f32"]
    net.forward_boxes(IMG, [(0, 0, 16, 16)], 1.0, want=(), pose=False)
    before = net.blobs["data"].data.copy()
    assert _c_forward(gpu_caffe, net, boxes, 1.0, canvas) == DC_EINVAL
    assert re.search(msg, gpu_caffe.pycaffe._lib.dc_last_error().decode())
    with pytest.raises(ValueError, match=msg):
        net.forward_boxes(IMG, boxes, 1.0, canvas=canvas)
    assert np.array_equal(net.blobs["data"].data, before)  # nothing was reshaped or written
    grp = ep._scale_group(net, 2)
    with pytest.raises(ValueError):
        grp.forward_boxes(IMG, boxes, [1.0, 0.5], canvas=canvas)
    pyr = (C.c_double * 2)(1.0, 0.5)
    b = np.ascontiguousarray(np.asarray(boxes, np.int32))
    s = np.ones(len(boxes))
    rc = gpu_caffe.pycaffe._lib.dc_group_forward_boxes(grp._h, IMG.ctypes.data_as(C.c_void_p), IMG.shape[0], IMG.shape[1], 0,
                                                       b.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), len(boxes), pyr,
                                                       canvas[0], canvas[1], None, None, None, None, None)
    assert rc == DC_EINVAL and re.search(msg, gpu_caffe.pycaffe._lib.dc_last_error().decode())


def test_no_boxes_is_a_no_op(gpu_caffe, nets):
    net = nets["f32"]
    assert _c_forward(gpu_caffe, net, np.zeros((0, 4)), 1.0, (0, 0)) == 0
    assert net.forward_boxes(IMG, np.zeros((0, 4), int))["pose"].shape == (0, 5, 14)


def test_config4_shaped_crowd_32_boxes_4_scales_with_pairwise_maps(gpu_caffe, synth152):
    """configs[4] as ONE call: 32 person boxes of 336 x 256 in a 1080 x 1920 image, 4 pyramid scales, next_pred on."""
    from deepcut_tools import deepercut_prototxt
    from oracle import oracle as O

    path, layers = synth152
    rs = np.random.RandomState(4)
    img = rs.randint(0, 256, (1080, 1920, 3)).astype(np.uint8)
    boxes = [(8 + 236 * (i % 8), 10 + 264 * (i // 8) - (i % 3) * 5, 8 + 236 * (i % 8) + 256, 10 + 264 * (i // 8) - (i % 3) * 5 + 336)
             for i in range(32)]
    boxes = [(x0, max(y0, 0), x1, min(y1, 1080)) for x0, y0, x1, y1 in boxes]
    net = gpu_caffe.Net(deepercut_prototxt(152, 336, 256), path, gpu_caffe.TEST, from_text=True)
    assert "next_pred" in net.wanted_outputs
    pyramid = [0.5, 0.75, 1.0, 1.25]
    grp = ep._scale_group(net, 4)
    outs = grp.forward_boxes(img, boxes, pyramid, want=("prob", "loc_pred", "next_pred"), pose=True)
    b, _, cv = gpu_caffe.check_boxes(img.shape, boxes)
    assert cv == (336, 256)
    for c, p in enumerate(pyramid):
        o = outs[c]
        h8, w8 = gpu_caffe.member_canvas(cv[0], p) // 8, gpu_caffe.member_canvas(cv[1], p) // 8
        assert o["prob"].shape == (32, 14, h8, w8) and o["next_pred"].shape == (32, 364, h8, w8)
        assert all(np.isfinite(v).all() for v in o.values())
        assert (o["prob"] > 0).all() and (o["prob"] < 1).all()
        for i in range(32):
            assert np.allclose(o["pose"][i], ep.box_pose_from_maps(o["prob"][i], o["loc_pred"][i], b[i], p), rtol=0, atol=1e-9)
    # member 2 (scale 1): box 9's canvas is the host construction, and its maps the CPU oracle's forward of that canvas
    m = grp.nets[2]
    x = ep.box_canvases(img, b[9:10], [1.0], cv).transpose(0, 3, 1, 2)
    assert np.array_equal(m.blobs["data"].data[9:10], x)
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(deepercut_prototxt(152, *cv), layers).forward(data=np.ascontiguousarray(x))
    for k in ("prob", "loc_pred", "next_pred"):
        assert float(np.abs(outs[2][k][9] - ref[k][0]).max()) <= 1e-3, k
    # estimate_poses: the best scale per box over the same grouped call; the caller's net keeps its output selection
    poses = ep.estimate_poses(img, boxes[:6], None, None, scales=pyramid, net=net)
    assert "next_pred" in net.wanted_outputs
    small = grp.forward_boxes(img, boxes[:6], pyramid, want=(), pose=True)
    for i in range(6):
        want = ep.select_best([o["pose"][i] for o in small])
        assert (poses[i] is None) == (want is None)
        if want is not None:
            assert np.array_equal(poses[i], want)
