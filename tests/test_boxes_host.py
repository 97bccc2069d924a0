"""CPU: the box entry's host side — argument checks (Python and C ABI) that fire before any device work, the smallest-canvas
rule, and the semantics the device route is pinned to (tests/test_gpu_boxes.py), built here from `preprocess` + Pillow:
canvas i = the demo's pre-processing of the host-cut crop at the top-left of a zero canvas, pose i = `pose_from_maps` on the
crop's own cells plus the box corner."""
import ctypes as C

import numpy as np
import pytest

import caffe
from oracle import preprocess as OP
from pose import estimate_pose as ep
from test_gpu_tiling import local_fcn_prototxt

DC_EINVAL, DC_ENOCPU = -1, -6
IMG = np.random.RandomState(5).randint(0, 256, (61, 83, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def cpu_net():
    mode = caffe.pycaffe._lib.dc_get_mode()
    caffe.set_mode_cpu()
    yield caffe.Net(local_fcn_prototxt(64, 64), caffe.TEST, from_text=True)
    caffe.pycaffe._lib.dc_set_mode(mode)


BAD = [
    ([(10, 10, 10, 20)], 1.0, None, "box 0 .* is empty"),
    ([(0, 0, 8, 8), (5, 9, 30, 9)], 1.0, None, "box 1 .* is empty"),
    ([(-1, 0, 8, 8)], 1.0, None, "box 0 .* outside"),
    ([(0, 0, 84, 8)], 1.0, None, "box 0 .* outside"),
    ([(0, 0, 8, 62)], 1.0, None, "box 0 .* outside"),
    ([(0, 0, 8, 8)], 0.0, None, "box 0 .*scale .* is not positive"),
    ([(0, 0, 8, 8)], 1.0, (12, 16), "canvas 12x16 is not a positive multiple of 8"),
    ([(0, 0, 8, 8), (0, 0, 40, 20)], 1.0, (16, 48), "box 1 .* needs a 24x40 canvas"),
    ([(0, 0, 8, 8), (0, 0, 40, 20)], [1.0, 0.5], (16, 16), "box 1 .* needs a 16x24 canvas"),
]


@pytest.mark.parametrize("boxes,scales,canvas,msg", BAD)
def test_python_checks_refuse_before_the_library(cpu_net, boxes, scales, canvas, msg):
    with pytest.raises(ValueError, match=msg):
        caffe.check_boxes(IMG.shape, boxes, scales, canvas)
    # the net's entry raises the same ValueError in CPU mode: nothing reached the library (which would say DC_ENOCPU)
    with pytest.raises(ValueError, match=msg):
        cpu_net.forward_boxes(IMG, boxes, scales, canvas=canvas)


def _c_call(net, boxes, scales, canvas):
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, np.float64), (b.shape[0],)))
    return caffe.pycaffe._lib.dc_net_forward_boxes(net._h, IMG.ctypes.data_as(C.c_void_p), IMG.shape[0], IMG.shape[1], 0,
                                                   b.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), b.shape[0], canvas[0],
                                                   canvas[1], None, None, None, None, None)


@pytest.mark.parametrize("boxes,scales,canvas,msg", BAD)
def test_c_abi_checks_name_the_box(cpu_net, boxes, scales, canvas, msg):
    import re

    rc = _c_call(cpu_net, boxes, scales, canvas or (64, 64))
    assert rc == DC_EINVAL
    assert re.search(msg, caffe.pycaffe._lib.dc_last_error().decode())


def test_c_abi_valid_boxes_reach_the_mode_check_and_n0_is_a_noop(cpu_net):
    assert _c_call(cpu_net, [(0, 0, 8, 8)], 1.0, (8, 8)) == DC_ENOCPU  # every check passed; CPU mode has no forward
    assert _c_call(cpu_net, np.zeros((0, 4)), 1.0, (0, 0)) == 0
    assert cpu_net.forward_boxes(IMG, np.zeros((0, 4), int))["pose"].shape == (0, 5, 14)


def test_none_canvas_is_the_smallest_that_fits():
    boxes = [(0, 0, 83, 61), (3, 4, 4, 5), (10, 0, 30, 1), (0, 20, 50, 41)]
    for scales in (1.0, [0.5, 2.0, 1.7, 0.9], [1.3, 1.0, 3.0, 0.61]):
        b, sc, cv = caffe.check_boxes(IMG.shape, boxes, scales)
        own = [ep.crop_canvas_size(y1 - y0, x1 - x0, s) for (x0, y0, x1, y1), s in zip(b, sc)]
        assert own == [caffe.canvas_size(y1 - y0, x1 - x0, s) for (x0, y0, x1, y1), s in zip(b, sc)]
        assert cv == (max(o[0] for o in own), max(o[1] for o in own))
        caffe.check_boxes(IMG.shape, boxes, scales, cv)
        for smaller in ((cv[0] - 8, cv[1]), (cv[0], cv[1] - 8)):
            if min(smaller) >= 8:
                with pytest.raises(ValueError, match="canvas"):
                    caffe.check_boxes(IMG.shape, boxes, scales, smaller)


ODD = [(0, 0, 83, 61),  # the whole image: touches every edge
       (0, 0, 17, 9), (70, 50, 83, 61), (0, 40, 12, 61), (60, 0, 83, 25),  # each corner
       (40, 30, 41, 31),  # 1 x 1
       (5, 12, 77, 13),  # one row
       (33, 2, 34, 60)]  # one column
SCALES = [1.0, 0.5, 1.7, 0.61, 2.3, 1.0, 0.83, 1.25]


def test_box_canvases_are_the_crops_own_preprocessing():
    b, sc, cv = caffe.check_boxes(IMG.shape, ODD, SCALES)
    got = ep.box_canvases(IMG, b, sc, cv)
    assert got.shape == (len(ODD),) + cv + (3,)
    for i, (x0, y0, x1, y1) in enumerate(ODD):
        crop = np.ascontiguousarray(IMG[y0:y1, x0:x1])
        want = OP.preprocess(crop, sc[i])  # the pure-NumPy restatement of Pillow, not the Pillow route box_canvases takes
        h, w = want.shape[:2]
        assert (h, w) == ep.crop_canvas_size(y1 - y0, x1 - x0, sc[i])
        assert np.array_equal(got[i, :h, :w], want), i
        assert not got[i, h:].any() and not got[i, :, w:].any()


def test_padding_repeats_the_crops_edge_not_the_images():
    # at scale 1 the canvas is the crop itself, then its last row / column repeated up to the stride
    x0, y0, x1, y1 = 20, 10, 33, 27  # 17 x 13: canvas 24 x 16
    c = ep.box_canvases(IMG, [(x0, y0, x1, y1)], [1.0], (24, 16))[0]
    crop = IMG[y0:y1, x0:x1].astype(np.float32) - ep.MEAN_BGR.astype(np.float32)
    assert np.array_equal(c[:17, :13], crop)
    assert np.array_equal(c[17:24, :13], np.repeat(crop[-1:], 7, axis=0))  # the crop's last row, not image row 27..
    assert np.array_equal(c[:17, 13:16], np.repeat(crop[:, -1:], 3, axis=1))
    assert not np.array_equal(IMG[y1, x0:x1], IMG[y1 - 1, x0:x1])  # (so the image's own next row would differ)
    one = ep.box_canvases(IMG, [(40, 30, 41, 31)], [1.0], (8, 8))[0]
    assert np.array_equal(one, np.broadcast_to(IMG[30, 40].astype(np.float32) - ep.MEAN_BGR.astype(np.float32), (8, 8, 3)))


def test_box_pose_is_restricted_to_the_crops_cells_and_shifted():
    rs = np.random.RandomState(2)
    box, s = (30, 20, 61, 45), 0.83  # crop 25 x 31 at 0.83: canvas 24 x 32, i.e. 3 x 4 cells of a 6 x 7 map
    oh, ow = ep.crop_canvas_size(25, 31, s)
    assert (oh, ow) == (24, 32)
    prob = rs.uniform(0, 0.5, (14, 6, 7)).astype(np.float32)
    loc = rs.randn(28, 6, 7).astype(np.float32)
    prob[:, 5, 6] = 0.99  # the unrestricted maximum lies outside the crop's own cells
    prob[3, 2, 3] = 0.9  # joint 3: the restricted maximum at the region's last cell
    pose = ep.box_pose_from_maps(prob, loc, box, s)
    ref = ep.pose_from_maps(prob[:, :3, :4], loc[:, :3, :4], s)
    assert np.array_equal(pose[2:], ref[2:])
    assert np.array_equal(pose[0], ref[0] + 30) and np.array_equal(pose[1], ref[1] + 20)
    rows, cols = ep.pose_cells(ref, s)
    assert (rows < 3).all() and (cols < 4).all() and rows[3] == 2 and cols[3] == 3
    assert not np.allclose(pose, ep.pose_from_maps(prob, loc, s))
