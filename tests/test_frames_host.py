"""CPU: the host side of the frame entries (dc_net_forward_frames, dc_net_forward_boxes_frame, dc_group_forward_frames,
dc_group_forward_boxes_frame) — the refusals fire before any device work, so they fire without a device: DC_EINVAL naming the field
and the frame index; frames that pass reach the mode check (DC_ENOCPU), and n = 0 boxes do nothing."""
import ctypes as C

import numpy as np
import pytest

import caffe
import caffe.pycaffe as pc
from test_gpu_tiling import local_fcn_prototxt

DC_EINVAL, DC_ENOCPU = -1, -6
H, W = 37, 53
Y = np.random.RandomState(1).randint(0, 256, (H, W)).astype(np.uint8)
UV = np.random.RandomState(2).randint(0, 256, (19, 27, 2)).astype(np.uint8)
BOXES = np.array([(0, 0, 30, 20), (5, 7, 40, 33)], np.int32)
BOX_SCALES = np.array([1.0, 1.0], np.float64)


@pytest.fixture(scope="module")
def cpu_nets():
    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    net = caffe.Net(local_fcn_prototxt(64, 64), caffe.TEST, from_text=True)
    yield net, caffe.NetGroup([net, net.clone()])
    pc._lib.dc_set_mode(mode)


def _err():
    return (pc._lib.dc_last_error() or b"").decode()


def _pair():
    f = caffe.Frame.nv12(Y, UV).c_frame()
    return (pc.DcFrame * 2)(f, f)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _set(field, k, v):
    def change(a):
        if k is None:
            setattr(a[1], field, v)
        else:
            getattr(a[1], field)[k] = v
    return change


CASES = [(_set("plane", 0, None), "plane[0]"), (_set("plane", 1, None), "plane[1]"), (_set("pitch", 0, W - 1), "pitch[0]"),
         (_set("pitch", 1, 53), "pitch[1]"), (_set("format", None, 2), "unknown format"), (_set("matrix", None, 2), "unknown matrix"),
         (_set("range", None, 2), "unknown range"), (_set("format", None, 0), "format 0 differs"), (_set("matrix", None, 1), "matrix 1 differs"),
         (_set("range", None, 1), "range 1 differs")]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_image_entries_name_the_field_and_the_frame(cpu_nets, case):
    net, grp = cpu_nets
    change, word = CASES[case]
    a = _pair()
    change(a)
    assert pc._lib.dc_net_forward_frames(net._h, a, 2, H, W, 1.0, 0, None, None, None, None, None) == DC_EINVAL
    assert word in _err() and "frame 1" in _err(), _err()
    good = _pair()
    rc = pc._lib.dc_group_forward_frames(grp._h, (C.c_void_p * 2)(C.addressof(good), C.addressof(a)), (C.c_int * 2)(2, 2), (C.c_int * 2)(H, H),
                                         (C.c_int * 2)(W, W), (C.c_double * 2)(1.0, 0.5), None, 0, None, None, None, None, None)
    assert rc == DC_EINVAL and word in _err() and "frame 1" in _err() and "member 1" in _err(), _err()


def test_minimum_pitches_and_a_bgr_frame_without_a_second_plane_pass(cpu_nets):
    net, grp = cpu_nets
    a = _pair()
    for f in a:
        f.pitch[0], f.pitch[1] = W, 54
    assert pc._lib.dc_net_forward_frames(net._h, a, 2, H, W, 1.0, 0, None, None, None, None, None) == DC_ENOCPU, _err()
    bgr = caffe.Frame.bgr(np.zeros((H, W, 3), np.uint8)).c_frame()
    assert bgr.plane[1] is None and bgr.pitch[0] == 3 * W
    assert pc._lib.dc_net_forward_frames(net._h, C.byref(bgr), 1, H, W, 1.0, 0, None, None, None, None, None) == DC_ENOCPU, _err()
    bgr.pitch[0] = 3 * W - 1
    assert pc._lib.dc_net_forward_frames(net._h, C.byref(bgr), 1, H, W, 1.0, 0, None, None, None, None, None) == DC_EINVAL
    assert "pitch[0]" in _err() and "frame 0" in _err()
    # null arguments and sizes, as the packed entry refuses them
    assert pc._lib.dc_net_forward_frames(net._h, None, 1, H, W, 1.0, 0, None, None, None, None, None) == DC_EINVAL
    assert pc._lib.dc_net_forward_frames(net._h, a, 0, H, W, 1.0, 0, None, None, None, None, None) == DC_EINVAL
    assert pc._lib.dc_net_forward_frames(net._h, a, 2, H, W, 0.0, 0, None, None, None, None, None) == DC_EINVAL


def test_box_entries(cpu_nets):
    net, grp = cpu_nets
    f = caffe.Frame.nv12(Y, UV).c_frame()
    pyr = (C.c_double * 2)(1.0, 0.7)

    def one(fr, n=2, canvas=(40, 40)):
        return pc._lib.dc_net_forward_boxes_frame(net._h, fr, H, W, 0, _vp(BOXES), _vp(BOX_SCALES), n, canvas[0], canvas[1], None, None, None,
                                                  None, None)

    def group(fr, n=2, canvas=(40, 40)):
        return pc._lib.dc_group_forward_boxes_frame(grp._h, fr, H, W, 0, _vp(BOXES), _vp(BOX_SCALES), n, pyr, canvas[0], canvas[1], None, None,
                                                    None, None, None, None)

    for call in (one, group):
        assert call(C.byref(f)) == DC_ENOCPU, _err()
        assert call(C.byref(f), n=0) == 0 and call(None, n=0) == 0
        assert call(None) == DC_EINVAL
        assert call(C.byref(f), canvas=(12, 16)) == DC_EINVAL and "canvas 12x16" in _err()  # the boxes are checked as in the packed entry
        bad = caffe.Frame.nv12(Y, UV).c_frame()
        bad.pitch[1] = 10
        assert call(C.byref(bad)) == DC_EINVAL and "pitch[1]" in _err() and "frame 0" in _err(), _err()
        bad = caffe.Frame.nv12(Y, UV).c_frame()
        bad.plane[1] = None
        assert call(C.byref(bad)) == DC_EINVAL and "plane[1]" in _err(), _err()


def test_python_entries_refuse_mixed_batches_before_the_library(cpu_nets):
    net, _ = cpu_nets
    f = caffe.Frame.nv12(Y, UV)
    with pytest.raises(ValueError, match="one size"):
        net.forward_images([f, caffe.Frame.nv12(Y[:36], UV[:18])], 1.0)
    with pytest.raises(ValueError, match="both host or both device"):
        net.forward_images([f, caffe.Frame.nv12_device(4096, 8192, H, W, 64, 64)], 1.0)
    with pytest.raises(ValueError, match="maps only"):
        net.forward_boxes(caffe.Frame.nv12_device(4096, 8192, H, W, 64, 64), BOXES, 1.0)
    with pytest.raises(caffe.DeepcutError) as e:  # a host frame passes every check and reaches the mode check
        net.forward_images(f, 1.0)
    assert e.value.code == DC_ENOCPU
    with pytest.raises(caffe.DeepcutError) as e:
        net.forward_boxes(f, BOXES, 1.0)
    assert e.value.code == DC_ENOCPU
