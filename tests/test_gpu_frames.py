"""-m gpu: the frame entries (dc_net_forward_frames, dc_net_forward_boxes_frame, dc_group_forward_frames, dc_group_forward_boxes_frame) —
NV12 and pitched BGR video frames read where the pre-processing fetches a pixel.

The reference of EVERY case is the existing entry run on the frame converted on the host by the restatement of the rule in
tests/nv12_ref.py (no product code), and equality is bit for bit: the conversion yields 8-bit channels, and everything behind the
fetch — replicate padding, mirror, both resample passes, the direct branch, mean, canvas — is integer arithmetic on those.

Frames are 37 x 53 and 38 x 54 (odd and even: the last row and column own a chroma sample of their own, and the replicate padding
crosses it) in buffers with pitch_y = W + 11 and pitch_uv = 2 ((W + 1) // 2) + 6 whose padding bytes are 0xFF, so a read through the
wrong pitch changes the result; the planes are random bytes with a block of all 125 combinations of the extremes 0, 16, 235, 240, 255."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nv12_ref as NR

pytestmark = pytest.mark.gpu
DC_EINVAL = -1
MEAN = np.array([104.0, 117.0, 123.0], np.float32)
EXTREMES = list(itertools.product((0, 16, 235, 240, 255), repeat=3))
SIZES = [(37, 53), (38, 54)]
SCALES = [1.0, 0.5, 1.3]  # the direct-fetch branch, multi-tap, upsample
CSC = {(37, 53): ("bt601", "limited"), (38, 54): ("bt709", "full")}


# ---- small nets, as tests/test_gpu_preprocess.py and tests/test_gpu_boxes.py build theirs (tests/test_gpu_tiling.py) ------------------
def _conv(name, bottom, top, nout, k, pad=0, stride=1, dilation=1, bias=False, typ="Convolution"):
    p = "num_output: %d kernel_size: %d pad: %d stride: %d" % (nout, k, pad, stride)
    if dilation != 1:
        p += " dilation: %d" % dilation
    if not bias:
        p += " bias_term: false"
    return 'layer { name: "%s" type: "%s" bottom: "%s" top: "%s" convolution_param { %s } }' % (name, typ, bottom, top, p)


def _bn_relu(suffix, blob):
    return ['layer { name: "bn%s" type: "BatchNorm" bottom: "%s" top: "%s" batch_norm_param { use_global_stats: true } }' % (suffix, blob, blob),
            'layer { name: "scale%s" type: "Scale" bottom: "%s" top: "%s" scale_param { bias_term: true } }' % (suffix, blob, blob),
            'layer { name: "relu%s" type: "ReLU" bottom: "%s" top: "%s" }' % (suffix, blob, blob)]


def _fcn_prototxt(h, w):
    L = ['name: "local_fcn"', 'input: "data"'] + ["input_dim: %d" % d for d in (1, 3, h, w)]
    L.append(_conv("conv1", "data", "conv1", 16, 7, pad=3, stride=2))
    L += _bn_relu("_conv1", "conv1")
    L.append('layer { name: "pool1" type: "Pooling" bottom: "conv1" top: "pool1" pooling_param { pool: MAX kernel_size: 3 stride: 2 } }')
    L.append(_conv("c2", "pool1", "c2", 32, 3, pad=1))
    L += _bn_relu("_c2", "c2")
    L.append(_conv("c3", "c2", "c3", 32, 1, stride=2))
    L += _bn_relu("_c3", "c3")
    L.append(_conv("c4", "c3", "c4", 64, 1, stride=2))
    L += _bn_relu("_c4", "c4")
    L.append(_conv("c5", "c4", "c5", 64, 3, pad=2, dilation=2))
    L += _bn_relu("_c5", "c5")
    for suffix, nout, out in (("pose", 14, "fc_pose"), ("locref", 28, "loc_pred")):
        L.append(_conv("up_" + suffix, "c5", "up_" + suffix, nout, 3, stride=2, bias=True, typ="Deconvolution"))
        L.append(_conv("skip_" + suffix, "c3", "skip_" + suffix, nout, 1, bias=True))
        L.append('layer { name: "crop_%s" type: "Crop" bottom: "up_%s" bottom: "skip_%s" top: "crop_%s" }' % (suffix, suffix, suffix, suffix))
        L.append('layer { name: "%s" type: "Eltwise" bottom: "skip_%s" bottom: "crop_%s" top: "%s" }' % (out, suffix, suffix, out))
    L.append('layer { name: "prob" type: "Sigmoid" bottom: "fc_pose" top: "prob" }')
    return "\n".join(L) + "\n"


def _fill(net, seed):
    rs = np.random.RandomState(seed)
    for name, blobs in net.params.items():
        if name.startswith("bn"):
            blobs[0].data[...] = rs.randn(*blobs[0].data.shape) * 0.1
            blobs[1].data[...] = rs.uniform(0.5, 1.5, blobs[1].data.shape)
            blobs[2].data[...] = 1.0
        elif name.startswith("scale"):
            blobs[0].data[...] = rs.uniform(0.5, 1.5, blobs[0].data.shape)
            blobs[1].data[...] = rs.randn(*blobs[1].data.shape) * 0.1
        else:
            w = blobs[0].data
            fan = float(np.prod(w.shape[1:])) if not name.startswith("up_") else float(w.shape[0] * 9 / 4.0)
            w[...] = rs.randn(*w.shape) / np.sqrt(fan)
            if len(blobs) > 1:
                blobs[1].data[...] = rs.randn(*blobs[1].data.shape) * 0.1


@pytest.fixture(scope="module")
def nets(gpu_caffe):
    out = {}
    for d in ("f32", "f16", "bf16"):
        out[d] = gpu_caffe.Net(_fcn_prototxt(64, 64), gpu_caffe.TEST, from_text=True, dtype=d)
        _fill(out[d], 5)
    return out


# ---- source frames ---------------------------------------------------------------------------------------------------------
class Src(object):
    """One NV12 frame: pitched buffers (padding 0xFF), the views a host Frame takes, and the restatement's BGR image."""

    def __init__(self, hw, seed, extremes_at=0):
        h, w = hw
        rs = np.random.RandomState(seed)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        self.h, self.w, self.py, self.puv = h, w, w + 11, 2 * cw + 6
        self.matrix, self.range = CSC.get(hw, ("bt601", "limited"))
        self.ybuf, self.uvbuf = np.full((h, self.py), 0xFF, np.uint8), np.full((ch, self.puv), 0xFF, np.uint8)
        self.y = self.ybuf[:, :w]
        self.uv = np.lib.stride_tricks.as_strided(self.uvbuf, (ch, cw, 2), (self.puv, 2, 1))
        self.y[...] = rs.randint(0, 256, (h, w))
        self.uv[...] = rs.randint(0, 256, (ch, cw, 2))
        for k, (yy, cb, cr) in enumerate(EXTREMES):  # chroma cell k + extremes_at, and the top-left pixel of that cell
            r, c = divmod(k + extremes_at, cw)
            self.uv[r, c] = (cb, cr)
            self.y[2 * r, 2 * c] = yy
        self.bgr = NR.to_bgr(self.y, self.uv, self.matrix, self.range, h, w)
        self._dev = None

    def host(self, caffe):
        return caffe.Frame.nv12(self.y, self.uv, matrix=self.matrix, range=self.range)

    def device(self, caffe):
        import torch

        if self._dev is None:  # an allocation of its own per plane, padding and all
            self._dev = (torch.from_numpy(self.ybuf).cuda(), torch.from_numpy(self.uvbuf).cuda())
            torch.cuda.synchronize()
        return caffe.Frame.nv12_device(self._dev[0].data_ptr(), self._dev[1].data_ptr(), self.h, self.w, self.py, self.puv, matrix=self.matrix,
                                       range=self.range)

    def frame(self, caffe, where):
        return self.host(caffe) if where == "host" else self.device(caffe)


_srcs = {}


def srcs(hw):
    """Three frames of one size in separate allocations; never written to after construction."""
    if hw not in _srcs:
        _srcs[hw] = [Src(hw, 100 * hw[0] + k, extremes_at=7 * k) for k in range(3)]
    return _srcs[hw]


def test_the_extremes_hit_both_clips_of_every_channel():
    for hw in SIZES:
        s = srcs(hw)[0]
        r, g, b = NR.convert(*np.array(EXTREMES).T, s.matrix, s.range)
        ky, rv, bu, gu, gv = NR.coefficients(s.matrix, s.range)
        Y, Cb, Cr = (np.array(EXTREMES).T.astype(np.int64) - np.array([[NR.scales(s.range)[0]], [128], [128]]))
        raw = [(ky * Y + rv * Cr + 32768) >> 16, (ky * Y + gu * Cb + gv * Cr + 32768) >> 16, (ky * Y + bu * Cb + 32768) >> 16]
        for v in raw:
            assert (v < 0).any() and (v > 255).any()
        assert all(((0 <= v) & (v <= 255)).all() for v in (r, g, b))


def _data(net):
    return net.blobs["data"].data.copy()


_ref = {}


def _reference(caffe, nets, dtype, hw, scale):
    """The existing entries on the converted images, once per (dtype, size, scale): data of n = 1, of n = 3, and of a two-member group
    (plain, mirrored) of image 0."""
    from pose.estimate_pose import _scale_group

    key = (dtype, hw, scale)
    if key not in _ref:
        net, ss = nets[dtype], srcs(hw)
        net.forward_images(ss[0].bgr, scale, want=(), pose=False)
        one = _data(net)
        net.forward_images(np.stack([s.bgr for s in ss]), scale, want=(), pose=False)
        three = _data(net)
        grp = _scale_group(net, 2)
        grp.forward_images(ss[0].bgr, [scale, scale], want=(), pose=False, mirror=[0, 1])
        _ref[key] = (one, three, [_data(m) for m in grp.nets])
    return _ref[key]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_network_input_equals_the_existing_entry_on_the_converted_image(gpu_caffe, nets, dtype, where):
    from pose.estimate_pose import _scale_group

    net = nets[dtype]
    for hw in SIZES:
        ss = srcs(hw)
        for scale in SCALES:
            one, three, pair = _reference(gpu_caffe, nets, dtype, hw, scale)
            what = (dtype, where, hw, scale)
            net.forward_images(ss[0].frame(gpu_caffe, where), scale, want=(), pose=False)
            assert one.shape[0] == 1 and np.array_equal(_data(net), one), what
            net.forward_images([s.frame(gpu_caffe, where) for s in ss], scale, want=(), pose=False)  # three separate surfaces
            assert three.shape[0] == 3 and np.array_equal(_data(net), three), what
            grp = _scale_group(net, 2)
            grp.forward_images(ss[0].frame(gpu_caffe, where), [scale, scale], want=(), pose=False, mirror=[0, 1])
            for m in range(2):
                assert np.array_equal(_data(grp.nets[m]), pair[m]), what + ("mirror", m)
            assert not np.array_equal(pair[0], pair[1])
    assert _reference(gpu_caffe, nets, dtype, (37, 53), 1.0)[0].shape == (1, 3, 40, 56)  # several workgroups, the last partly filled


@pytest.mark.parametrize("matrix", NR.MATRICES)
@pytest.mark.parametrize("range_", NR.RANGES)
def test_scale_one_gives_back_the_conversion_itself(gpu_caffe, nets, matrix, range_):
    """128 x 144: 4608 chroma cells, every one with a pixel of its own: 4483 independent random triples and the 125 extremes."""
    h, w = 128, 144
    s = Src((h, w), 9)
    s.matrix, s.range = matrix, range_
    want = NR.to_bgr(s.y, s.uv, matrix, range_, h, w)
    for where in ("host", "device"):
        nets["f32"].forward_images(s.frame(gpu_caffe, where), 1.0, want=(), pose=False)
        got = nets["f32"].blobs["data"].data[0].transpose(1, 2, 0) + MEAN
        assert got.shape == (h, w, 3) and np.array_equal(got, want.astype(np.float32)), (matrix, range_, where)


@pytest.mark.parametrize("where", ["host", "device"])
def test_maps_and_pose_equal_those_of_the_converted_array(gpu_caffe, nets, where):
    net = nets["f32"]
    for hw, scale in (((37, 53), 1.0), ((38, 54), 0.5), ((37, 53), 1.3)):
        ss = srcs(hw)
        want = net.forward_images(np.stack([s.bgr for s in ss]), scale, want=("prob", "loc_pred"), pose=True)
        want = {k: v.copy() for k, v in want.items()}
        got = net.forward_images([s.frame(gpu_caffe, where) for s in ss], scale, want=("prob", "loc_pred"), pose=True)
        assert sorted(got) == sorted(want) == ["loc_pred", "pose", "prob"]
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (where, hw, scale, k)


# one box with an odd origin (it pairs chroma by its place in the image, not in the crop), one reaching the last row and column
BOXES = [(0, 0, 30, 20), (5, 7, 40, 33), (21, 9, 53, 37)]
BOX_SCALES = [1.0, 1.3, 0.6]


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_boxes_equal_the_existing_entry_on_the_converted_image(gpu_caffe, nets, dtype):
    net, s = nets[dtype], srcs((37, 53))[0]
    want = {k: v.copy() for k, v in net.forward_boxes(s.bgr, BOXES, BOX_SCALES, want=("prob", "loc_pred"), pose=True).items()}
    want_data = _data(net)
    got = net.forward_boxes(s.host(gpu_caffe), BOXES, BOX_SCALES, want=("prob", "loc_pred"), pose=True)
    assert np.array_equal(_data(net), want_data) and want_data.shape[0] == 3
    for k in ("prob", "loc_pred", "pose"):
        assert np.array_equal(got[k], want[k]), (dtype, k)
    # a device frame: the maps (this method copies no device pose to the host)
    got = net.forward_boxes(s.device(gpu_caffe), BOXES, BOX_SCALES, want=("prob", "loc_pred"), pose=False)
    assert np.array_equal(_data(net), want_data)
    assert np.array_equal(got["prob"], want["prob"]) and np.array_equal(got["loc_pred"], want["loc_pred"])
    # the odd-origin box is NOT the host-cut crop of the planes: its chroma pairs by image position
    x0, y0, x1, y1 = BOXES[1]
    cut = NR.to_bgr(s.y[y0:y1, x0:x1], s.uv[(y0 + 1) // 2:, (x0 + 1) // 2:], s.matrix, s.range, y1 - y0, x1 - x0)
    assert not np.array_equal(cut, s.bgr[y0:y1, x0:x1])


def test_grouped_boxes_two_scales_and_mirrored(gpu_caffe, nets):
    from pose import MIRROR_MPII14
    from pose.estimate_pose import _scale_group

    net, s = nets["f32"], srcs((37, 53))[0]
    pyr = [1.0, 0.7]
    grp = _scale_group(net, 2)
    want = grp.forward_boxes(s.bgr, BOXES, pyr, BOX_SCALES, want=("prob", "loc_pred"), pose=True)
    want = [{k: v.copy() for k, v in o.items()} for o in want]
    want_data = [_data(m) for m in grp.nets]
    for where in ("host", "device"):
        got = grp.forward_boxes(s.frame(gpu_caffe, where), BOXES, pyr, BOX_SCALES, want=("prob", "loc_pred"), pose=where == "host")
        for m in range(2):
            assert np.array_equal(_data(grp.nets[m]), want_data[m]), (where, m)
            for k in got[m]:
                assert np.array_equal(got[m][k], want[m][k]), (where, m, k)
            assert ("pose" in got[m]) == (where == "host")
    # the mirrored form, then the fused decode
    grp4, flags = _scale_group(net, 4), [0, 0, 1, 1]
    grp4.forward_boxes(s.bgr, BOXES, pyr * 2, BOX_SCALES, want=(), pose=False, mirror=flags)
    want_data = [_data(m) for m in grp4.nets]
    want = {k: v.copy() for k, v in grp4.decode_boxes(pyr * 2, 0, mirror=flags, joint_mirror=MIRROR_MPII14, want=("prob", "loc_pred")).items()}
    grp4.forward_boxes(s.host(gpu_caffe), BOXES, pyr * 2, BOX_SCALES, want=(), pose=False, mirror=flags)
    for m in range(4):
        assert np.array_equal(_data(grp4.nets[m]), want_data[m]), m
    got = grp4.decode_boxes(pyr * 2, 0, mirror=flags, joint_mirror=MIRROR_MPII14, want=("prob", "loc_pred"))
    assert sorted(got) == sorted(want) and "pose" in got
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(want_data[0], want_data[2])


def test_pyramid_people_and_fused_pose(gpu_caffe, nets, synth152):
    import people_ref as R
    from deepcut_tools import deepercut_prototxt
    from fuse_ref import MEAN as PAIR_MEAN, STD as PAIR_STD
    from pose import estimate_people
    from pose.estimate_pose import estimate_pose

    s = srcs((37, 53))[0]
    frame = s.host(gpu_caffe)
    assert np.array_equal(frame.to_bgr(), s.bgr)
    net = gpu_caffe.Net(deepercut_prototxt(152, 40, 56), synth152[0], gpu_caffe.TEST, from_text=True)
    stats = (R.all_pairs_edges(), PAIR_MEAN, PAIR_STD)
    kw = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
    want = estimate_people(frame.to_bgr(), None, None, stats, net=net, scales=[0.7, 1.0], flip=True, **kw)
    got = estimate_people(frame, None, None, stats, net=net, scales=[0.7, 1.0], flip=True, **kw)
    assert got.shape == want.shape and got.shape[1:] == (14, 3) and np.array_equal(got, want)
    small = nets["f32"]
    want = estimate_pose(frame.to_bgr(), None, None, scales=[0.7, 1.0], net=small, fuse=True, flip=True, all_outputs=True)
    got = estimate_pose(frame, None, None, scales=[0.7, 1.0], net=small, fuse=True, flip=True, all_outputs=True)
    assert got.shape == (5, 14) and np.array_equal(got, want)
    # the per-scale route, and the host route through Frame.to_bgr()
    assert np.array_equal(estimate_pose(frame, None, None, scales=[0.7, 1.0], net=small, all_outputs=True),
                          estimate_pose(s.bgr, None, None, scales=[0.7, 1.0], net=small, all_outputs=True))
    assert np.array_equal(estimate_pose(frame, None, None, scales=[1.0], net=small, on_device=False, all_outputs=True),
                          estimate_pose(s.bgr, None, None, scales=[1.0], net=small, on_device=False, all_outputs=True))


def test_pitched_bgr_frame_equals_the_packed_entry(gpu_caffe, nets):
    import torch

    net, (h, w) = nets["f32"], (37, 53)
    buf = np.full((h, 3 * w + 5), 0xFF, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (3 * w + 5, 3, 1))
    view[...] = np.random.RandomState(12).randint(0, 256, (h, w, 3))
    packed = np.ascontiguousarray(view)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    frames = {"host": gpu_caffe.Frame.bgr(view), "device": gpu_caffe.Frame.bgr_device(dev.data_ptr(), h, w, 3 * w + 5)}
    for scale in SCALES:
        net.forward_images(packed, scale, want=(), pose=False)
        want = _data(net)
        for where, f in frames.items():
            net.forward_images(f, scale, want=(), pose=False)
            assert np.array_equal(_data(net), want), (where, scale)
    net.forward_boxes(packed, BOXES, BOX_SCALES, want=(), pose=False)
    want = _data(net)
    net.forward_boxes(frames["host"], BOXES, BOX_SCALES, want=(), pose=False)
    assert np.array_equal(_data(net), want)


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_wrong_pitch_changes_the_result(gpu_caffe, nets, where):
    """The padding is there to be seen: the same planes described with a smaller pitch (still at least a row, so every read stays
    inside the buffers) give another network input — the equalities above are not blind to the pitch."""
    net, s = nets["f32"], srcs((37, 53))[0]
    net.forward_images(s.bgr, 1.0, want=(), pose=False)
    want = _data(net)
    f = s.frame(gpu_caffe, where)
    for k in range(2):
        g = gpu_caffe.Frame(f.format, f.planes, [p - (1, 2)[j] * (j == k) for j, p in enumerate(f.pitches)], s.h, s.w, s.matrix, s.range,
                            f.is_device, f._keep)
        net.forward_images(g, 1.0, want=(), pose=False)
        assert not np.array_equal(_data(net), want), (where, k)
    net.forward_images(f, 1.0, want=(), pose=False)
    assert np.array_equal(_data(net), want)


def _err():
    import caffe.pycaffe as pc

    return (pc._lib.dc_last_error() or b"").decode()


def test_refusals_name_the_field_and_leave_the_input_alone(gpu_caffe, nets):
    import caffe.pycaffe as pc
    from pose.estimate_pose import _scale_group

    net, ss = nets["f32"], srcs((37, 53))
    net.forward_images(ss[0].bgr, 1.0, want=(), pose=False)
    before = _data(net)
    h, w = 37, 53

    def pair():
        return (pc.DcFrame * 2)(ss[0].host(gpu_caffe).c_frame(), ss[1].host(gpu_caffe).c_frame())

    def null_chroma(a):
        a[1].plane[1] = None

    def null_luma(a):
        a[1].plane[0] = None

    def set_(field, k, v):
        def f(a):
            if k is None:
                setattr(a[1], field, v)
            else:
                getattr(a[1], field)[k] = v
        return f

    cases = [(null_chroma, "plane[1]"), (null_luma, "plane[0]"), (set_("pitch", 0, w - 1), "pitch[0]"), (set_("pitch", 1, 2 * 27 - 1), "pitch[1]"),
             (set_("format", None, 7), "format"), (set_("matrix", None, 2), "matrix"), (set_("range", None, -1), "range"),
             # frames of one call that differ
             (set_("format", None, 0), "format"), (set_("matrix", None, 1), "matrix"), (set_("range", None, 1), "range")]
    for change, field in cases:
        a = pair()
        change(a)
        rc = pc._lib.dc_net_forward_frames(net._h, a, 2, h, w, 1.0, 0, None, None, None, None, None)
        assert rc == DC_EINVAL and field in _err() and "frame 1" in _err(), (field, _err())
        assert np.array_equal(_data(net), before), field
    # the box entry and the two group entries refuse the same, before any device work
    b = np.array(BOXES, np.int32)
    sc = np.array(BOX_SCALES, np.float64)
    bad = ss[0].host(gpu_caffe).c_frame()
    bad.pitch[1] = 10
    rc = pc._lib.dc_net_forward_boxes_frame(net._h, C.byref(bad), h, w, 0, b.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), 3, 48, 56,
                                            None, None, None, None, None)
    assert rc == DC_EINVAL and "pitch[1]" in _err() and "frame 0" in _err(), _err()
    grp = _scale_group(net, 2)
    rc = pc._lib.dc_group_forward_boxes_frame(grp._h, C.byref(bad), h, w, 0, b.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), 3,
                                              (C.c_double * 2)(1.0, 0.7), 48, 56, None, None, None, None, None, None)
    assert rc == DC_EINVAL and "pitch[1]" in _err(), _err()
    good, a = pair(), pair()
    a[1].plane[1] = None
    rc = pc._lib.dc_group_forward_frames(grp._h, (C.c_void_p * 2)(C.addressof(good), C.addressof(a)), (C.c_int * 2)(2, 2), (C.c_int * 2)(h, h),
                                         (C.c_int * 2)(w, w), (C.c_double * 2)(1.0, 0.5), None, 0, None, None, None, None, None)
    assert rc == DC_EINVAL and "plane[1]" in _err() and "frame 1" in _err() and "member 1" in _err(), _err()
    assert np.array_equal(_data(net), before)
    # and the Python layer: frames of two sizes, host and device frames mixed
    with pytest.raises(ValueError, match="one size"):
        net.forward_images([ss[0].host(gpu_caffe), srcs((38, 54))[0].host(gpu_caffe)], 1.0)
    with pytest.raises(ValueError, match="both host or both device"):
        net.forward_images([ss[0].host(gpu_caffe), ss[1].device(gpu_caffe)], 1.0)
    assert np.array_equal(_data(net), before)
