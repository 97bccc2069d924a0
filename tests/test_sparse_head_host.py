"""No GPU: the restatement of the sparse pairwise head (tests/sparse_head_ref.py) against oracle.OracleNet, the filter image of
dc_sparse_head_pack against NumPy, DC_OPT_SPARSE_PAIRWISE on CPU-mode nets, and the arguments estimate_people refuses."""
import numpy as np
import pytest

import caffe
import sparse_head_ref as SR


def _weights(rs, k5, k3, joints, bias, integers=True):
    pairs = joints * (joints - 1)
    out = []
    draw = (lambda *s: rs.randint(-4, 5, s).astype(np.float32)) if integers else (lambda *s: rs.randn(*s).astype(np.float32))
    for suffix, nout in (("pose", joints), ("locref", 2 * joints), ("next", 2 * pairs)):
        out.append(("x5_up_" + suffix, "Deconvolution", [draw(k5, nout, 3, 3)] + ([draw(nout)] if bias else [])))
        out.append(("x3_" + suffix, "Convolution", [draw(nout, k3, 1, 1)] + ([draw(nout)] if bias else [])))
    return out


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("h5,w5,h,w,oh,ow", [(3, 4, 6, 8, 0, 0), (3, 4, 5, 7, 0, 0), (3, 4, 5, 7, 1, 1), (3, 4, 5, 7, 1, 0), (3, 4, 5, 7, 0, 1)])
def test_restatement_equals_the_oracle_on_head_only_nets(h5, w5, h, w, oh, ow, bias):
    """next_pred of the oracle (double accumulation) against the nine masked matmuls, <= 1e-12 x range.  The oracle returns float32, so
    operands are small integers: every product and sum is exact in both, and any difference is a tap, an offset or a border that the
    restatement gets wrong, not rounding.  Usual size (x3 = 2 x5) and an odd one, every crop offset the Crop layer admits there (it needs its bottom strictly larger), with
    and without bias."""
    from oracle import oracle as O

    rs = np.random.RandomState(h * 100 + w * 10 + oh * 2 + ow)
    k5, k3, joints, n = 8, 4, 2, 2
    text = SR.head_prototxt(n, k5, k3, h5, w5, h, w, joints, bias=bias, oh=oh, ow=ow)
    weights = _weights(rs, k5, k3, joints, bias)
    x5 = rs.randint(-4, 5, (n, k5, h5, w5)).astype(np.float32)
    x3 = rs.randint(-4, 5, (n, k3, h, w)).astype(np.float32)
    O.set_double_acc(True)
    try:
        blobs = O.OracleNet(text, weights).forward(x5=x5, x3=x3)
    finally:
        O.set_double_acc(False)
    W = {name: b for name, _t, b in weights}
    ref, s = SR.sparse_head_ref(x3, x5, W["x3_next"][0], W["x5_up_next"][0], W["x3_next"][1] if bias else None,
                                W["x5_up_next"][1] if bias else None, oh, ow)
    got = blobs["next_pred"].astype(np.float64)
    assert got.shape == ref.shape == (n, 4, h, w)
    rng = np.abs(ref).max()
    assert rng > 10 and np.abs(got - ref).max() <= 1e-12 * rng
    assert (s >= np.abs(ref)).all()


def _expect_image(ws, wd):
    cout, k3 = ws.shape
    k5 = wd.shape[0]
    nq, n5, n3 = (cout + 31) // 32, (k5 + 7) // 8, (k3 + 7) // 8
    taps = np.zeros((9, nq, n5, 64, 4), np.float32)
    skip = np.zeros((nq, n3, 64, 4), np.float32)
    for q in range(nq):
        for l in range(64):
            n = 32 * q + l % 32
            if n >= cout:
                continue
            for m in range(4):
                for j in range(n5):
                    k = 8 * j + 4 * (l // 32) + m
                    if k < k5:
                        taps[:, q, j, l, m] = wd[k, n].reshape(9)
                for j in range(n3):
                    k = 8 * j + 4 * (l // 32) + m
                    if k < k3:
                        skip[q, j, l, m] = ws[n, k]
    return taps, skip


@pytest.mark.parametrize("cout,k3,k5", [(4, 4, 8), (40, 12, 21), (64, 16, 32)])
def test_filter_image_against_numpy(cout, k3, k5):
    """Every filter at its place in the fragment order, zeros in the padding of K and Cout; sizes that are no multiple of 8 / 32 included."""
    rs = np.random.RandomState(cout)
    ws, wd = rs.randn(cout, k3).astype(np.float32), rs.randn(k5, cout, 3, 3).astype(np.float32)
    taps, skip = caffe.sparse_head_pack(ws, wd)
    et, es = _expect_image(ws, wd)
    assert np.array_equal(taps, et) and np.array_equal(skip, es)


def test_option_set_get_and_clone_on_a_cpu_mode_net():
    caffe.set_mode_cpu()
    net = caffe.Net(SR.head_prototxt(1, 8, 4, 3, 4, 6, 8), caffe.TEST, from_text=True)
    assert net.get_option(5) == 0 and net.sparse_pairwise is False and net.clone().sparse_pairwise is False
    net.sparse_pairwise = True
    assert net.get_option(5) == 1 and net.sparse_pairwise is True
    assert net.clone().sparse_pairwise is True
    net.sparse_pairwise = False
    assert net.get_option(5) == 0
    with pytest.raises(caffe.DeepcutError) as e:
        net.set_option(5, 2)
    assert e.value.code == -1
    made = caffe.Net(SR.head_prototxt(1, 8, 4, 3, 4, 6, 8), caffe.TEST, from_text=True, want=["loc_pred", "prob"], sparse_pairwise=True)
    assert made.sparse_pairwise is True and made.wanted_outputs == ["loc_pred", "prob"]
    assert "sparse_packs" in net.stats() and net.stats()["sparse_packs"] == 0


_NOT_HEADS = {
    "a convolution writes next_pred": ('input: "x3"\ninput_shape { dim: 1 dim: 4 dim: 6 dim: 8 }\n'
                                       'layer { name: "direct" type: "Convolution" bottom: "x3" top: "next_pred" convolution_param { num_output: 4 kernel_size: 1 } }\n',
                                       "direct"),
    "the sum of two convolutions": ('input: "x3"\ninput_shape { dim: 1 dim: 4 dim: 6 dim: 8 }\n'
                                    'layer { name: "a" type: "Convolution" bottom: "x3" top: "a" convolution_param { num_output: 4 kernel_size: 1 } }\n'
                                    'layer { name: "second" type: "Convolution" bottom: "x3" top: "b" convolution_param { num_output: 4 kernel_size: 1 } }\n'
                                    'layer { name: "next_pred" type: "Eltwise" bottom: "a" bottom: "b" top: "next_pred" }\n', "second"),
    "a 3x3 skip": (SR.head_prototxt(1, 8, 4, 3, 4, 6, 8).replace(
        'name: "x3_next" type: "Convolution" bottom: "x3" top: "x3_next" convolution_param { num_output: 4 kernel_size: 1 pad: 0',
        'name: "x3_next" type: "Convolution" bottom: "x3" top: "x3_next" convolution_param { num_output: 4 kernel_size: 3 pad: 1'), "x3_next"),
    "a relu between the skip and the sum": (SR.head_prototxt(1, 8, 4, 3, 4, 6, 8).replace(
        'layer { name: "crop_next"', 'layer { name: "skip_relu" type: "ReLU" bottom: "x3_next" top: "x3_next" }\nlayer { name: "crop_next"'), "skip_relu"),
}


@pytest.mark.parametrize("what", sorted(_NOT_HEADS))
def test_option_refused_where_next_pred_is_no_such_head(what):
    text, layer = _NOT_HEADS[what]
    caffe.set_mode_cpu()
    net = caffe.Net(text, caffe.TEST, from_text=True)
    with pytest.raises(caffe.DeepcutError) as e:
        net.sparse_pairwise = True
    assert e.value.code == -4 and "'%s'" % layer in str(e.value)  # DC_EUNSUP naming the layer
    assert net.get_option(5) == 0


def test_a_net_without_next_pred_is_refused():
    caffe.set_mode_cpu()
    net = caffe.Net('input: "x3"\ninput_shape { dim: 1 dim: 4 dim: 6 dim: 8 }\n'
                    'layer { name: "c" type: "Convolution" bottom: "x3" top: "c" convolution_param { num_output: 4 kernel_size: 1 } }\n', caffe.TEST, from_text=True)
    with pytest.raises(caffe.DeepcutError) as e:
        net.sparse_pairwise = True
    assert e.value.code == -4


def test_pairwise_at_refuses_cells_outside_the_map_before_any_device_work():
    caffe.set_mode_cpu()
    net = caffe.Net(SR.head_prototxt(2, 8, 4, 3, 4, 6, 8), caffe.TEST, from_text=True)
    for bad in ([2, 0, 0], [0, 6, 0], [0, 0, 8], [-1, 0, 0], [0, -1, 0]):
        with pytest.raises(caffe.DeepcutError) as e:
            net.pairwise_at([[0, 0, 0], bad])
        assert e.value.code == -1 and "detection 1" in str(e.value)  # DC_EINVAL, not the CPU-mode refusal


def test_estimate_people_refuses_sparse_with_a_pyramid_or_a_flip():
    from pose import estimate_people

    img = np.zeros((32, 32, 3), np.uint8)
    stats = (np.zeros((0, 2), np.int32), np.zeros((0, 2)), np.zeros((0, 2)))
    with pytest.raises(ValueError, match="sparse"):
        estimate_people(img, "no.prototxt", "no.caffemodel", stats, sparse=True, scales=[1.0, 0.5])
    with pytest.raises(ValueError, match="sparse"):
        estimate_people(img, "no.prototxt", "no.caffemodel", stats, sparse=True, flip=True)
