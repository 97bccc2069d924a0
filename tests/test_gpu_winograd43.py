"""-m gpu: the unfused Winograd F(4x4,3x3) form of the float32 3x3 layers (csrc/wino43_f32.hip, tile `wino_f43`: input transform, 36 batched
ws1x1f products, inverse transform), put in place with set_tile on single layers and on every 3x3 layer of a small whole net.  Against the CPU
oracle at the bound tests/test_gpu_winograd.py holds single layers to, 1e-4 x max(1, max|reference|) (measured here 7e-6 .. 3.8e-5 absolute on
ranges of 4 .. 7), and at the error of the form's own float32 emulation with sequential sums (tests/f32_ref.py wino43_f32, which measures 1.0e-5 x
range on a res4 layer): at most 3 x its maximum and 2 x its RMS error against a float64 reference; measured, worst over the cases: 1.24 and 0.87.
Whole nets at the path's 1e-3.

Shapes: the smallest that reach each path of the three kernels.  A step of the multiply is 16 tiles, a tile 4 x 4 pixels:
  5 x 9, 6 x 7      2 x 3 / 2 x 2 tiles, partial in both directions, one partial step
  18 x 22           30 tiles: a full step and a partial one, two pixel ranges
  34 x 46, Cin 64   108 tiles: 7 steps in 7 ranges (36 slices x 7 = 252 workgroups over the eight XCDs)
  2 x 6 x 7         the tiles of two images in one step
  9 x 11, d = 2     four phase images of 5 x 6, 5 x 5, 4 x 6 and 4 x 5 pixels on one 2 x 2 tile grid
"""
import os

import numpy as np
import pytest

import f32_ref as F
from conftest import rand_image
from test_gpu_winograd import wino_case

pytestmark = pytest.mark.gpu
LABEL = "wino_f43+ws1x1f<16xN>"


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DC_AUTOTUNE", "0")     # the form is put in place by set_tile
    monkeypatch.setenv("DC_WINOGRAD43", "-1")  # its filter image is packed, nothing is forced
    monkeypatch.delenv("DC_WINOGRAD", raising=False)
    monkeypatch.delenv("DC_TUNE_CACHE", raising=False)
    monkeypatch.delenv("DC_WSF43_SLOTS", raising=False)


def _conv_net(n, cin, cout, h, w, dil, relu, resid=False, stride=1):
    L = ['name: "w"', 'input: "data"'] + ["input_dim: %d" % d for d in (n, cin, h, w)]
    L.append('layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: %d kernel_size: 3 '
             'pad: %d dilation: %d stride: %d bias_term: false } }' % (cout, dil, dil, stride))
    L.append('layer { name: "bn" type: "BatchNorm" bottom: "c" top: "c" batch_norm_param { use_global_stats: true } }')
    L.append('layer { name: "sc" type: "Scale" bottom: "c" top: "c" scale_param { bias_term: true } }')
    out = "c"
    if resid:
        L.append('layer { name: "sum" type: "Eltwise" bottom: "data" bottom: "c" top: "sum" }')
        out = "sum"
    if relu:
        L.append('layer { name: "relu" type: "ReLU" bottom: "%s" top: "%s" }' % (out, out))
    return "\n".join(L) + "\n", out


CASES = [  # n, cin, cout, h, w, dilation, relu
    (1, 64, 64, 5, 9, 1, True),
    (1, 64, 64, 6, 7, 1, False),
    (1, 64, 64, 18, 22, 1, True),
    (1, 64, 64, 34, 46, 1, False),
    (2, 64, 64, 6, 7, 1, True),
    (1, 64, 64, 9, 11, 2, True),
    # every K of the multiply x one and two channel slices
    (1, 64, 128, 6, 7, 1, True), (1, 128, 64, 6, 7, 1, False), (1, 128, 128, 6, 7, 1, True), (1, 256, 64, 6, 7, 1, True),
    (1, 256, 128, 6, 7, 1, False), (1, 512, 64, 6, 7, 1, True), (1, 512, 128, 6, 7, 1, False),
]
_reference = {}  # case -> (prototxt, output blob, weights, input, oracle output): made once, left unchanged


def _case_data(case, resid=False, stride=1):
    key = case + (resid, stride)
    if key not in _reference:
        from oracle import oracle as O

        n, cin, cout, h, w, dil, relu = case
        proto, out = _conv_net(n, cin, cout, h, w, dil, relu, resid, stride)
        rs = np.random.RandomState(cin + cout + h)
        # a folded affine that is neither 1 nor 0: BatchNorm mean / variance and Scale gain / bias
        weights = [("c", "Convolution", [(rs.randn(cout, cin, 3, 3) / np.sqrt(9.0 * cin)).astype(np.float32)]),
                   ("bn", "BatchNorm", [rs.randn(cout).astype(np.float32) * 0.1, rs.uniform(0.5, 1.5, cout).astype(np.float32),
                                        np.array([1.0], np.float32)]),
                   ("sc", "Scale", [rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.randn(cout).astype(np.float32) * 0.1])]
        x = rs.randn(n, cin, h, w).astype(np.float32)
        O.set_threads(min(16, os.cpu_count() or 1))
        ref = O.OracleNet(proto, weights).forward(data=x)[out]
        ref.setflags(write=False)
        x.setflags(write=False)
        _reference[key] = (proto, out, weights, x, ref)
    return _reference[key]


def _net(gpu_caffe, proto, weights):
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True)
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    return net


def _signature(net):
    sigs = [r["signature"] for r in net.tune_report() if "/3x3/" in r["signature"]]
    assert len(sigs) == 1, sigs
    return sigs[0]


def _on_the_form(net, x):
    """the first forward lowers the shape; the form is then put in place on its plan"""
    net.blobs["data"].data[...] = x
    net.forward()
    net.set_tile(_signature(net), "wino_f43")
    assert LABEL in net.plan_text()


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d_%dx%d_d%d%s" % (c[:6] + ("_relu" if c[6] else "",)) for c in CASES])
def test_single_layers_match_the_oracle_twice_with_the_same_bits(gpu_caffe, case):
    proto, out, weights, x, ref = _case_data(case)
    net = _net(gpu_caffe, proto, weights)
    _on_the_form(net, x)
    runs = []
    for _ in range(2):
        net.blobs["data"].data[...] = x
        net.forward()
        runs.append(net.blobs[out].data.copy())
    assert runs[0].shape == ref.shape
    err = float(np.abs(runs[0] - ref).max())
    bound = 1e-4 * max(1.0, float(np.abs(ref).max()))
    print("wino_f43 %s: max|hip - oracle| = %.3e (bound %.3e)" % (case, err, bound))
    assert err <= bound, (err, bound)
    ref64, model, pixels = wino_case(case, weights, x, "wino43")
    F.assert_f32_tight(runs[0], ref64, model, "wino_f43: %s" % (case,), pixels)
    assert np.array_equal(runs[0], runs[1]), "two runs differ"


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_pixel_reaches_its_neighbourhood_and_stays_in_its_tiles(gpu_caffe, bad):
    """Input pixel (7, 9) of channel 3 is NaN / inf (inf - inf in the input transform: NaN).  The 3 x 3 outputs that read it are not finite in
    every channel; so may be the rest of the tiles whose 6 x 6 patch holds it, and nothing else: every other output has the clean input's value."""
    case = (1, 64, 64, 18, 22, 1, False)
    proto, out, weights, x, ref = _case_data(case)
    net = _net(gpu_caffe, proto, weights)
    _on_the_form(net, x)
    xb = x.copy()
    py, px = 7, 9
    xb[0, 3, py, px] = bad
    net.blobs["data"].data[...] = xb
    net.forward()
    got = net.blobs[out].data.copy()
    assert not np.isfinite(got[0, :, py - 1:py + 2, px - 1:px + 2]).any()
    touched = np.zeros(got.shape[2:], bool)
    for ty in range(5):
        for tx in range(6):
            if 4 * ty - 1 <= py <= 4 * ty + 4 and 4 * tx - 1 <= px <= 4 * tx + 4:
                touched[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = True
    assert touched.sum() == 2 * 16  # (row 7 sits in the patches of tile rows 1 and 2, column 9 in tile column 2's only)
    clean = ~touched
    assert np.isfinite(got[0][:, clean]).all()
    assert float(np.abs(got[0][:, clean] - ref[0][:, clean]).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


def test_refused_layers_keep_their_tiles(gpu_caffe, monkeypatch):
    """DC_WINOGRAD43=1 forces the form wherever it is eligible: a stride-2 layer and a layer with a shortcut are not, run on what they ran on
    before and match the oracle; set_tile refuses the form for them."""
    monkeypatch.setenv("DC_WINOGRAD43", "1")
    for resid, stride in ((False, 2), (True, 1)):
        proto, out, weights, x, ref = _case_data((1, 64, 64, 18, 22, 1, True), resid, stride)
        net = _net(gpu_caffe, proto, weights)
        net.blobs["data"].data[...] = x
        net.forward()
        assert "wino_f43" not in net.plan_text()
        with pytest.raises(gpu_caffe.DeepcutError):
            net.set_tile(_signature(net), "wino_f43")
        net.blobs["data"].data[...] = x
        net.forward()
        assert float(np.abs(net.blobs[out].data - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    # ... and the switch itself: an eligible layer is lowered onto the form, with DC_WINOGRAD43=0 the form does not exist for it
    proto, out, weights, x, ref = _case_data((1, 64, 64, 18, 22, 1, True))
    assert LABEL in _net(gpu_caffe, proto, weights).plan_text()
    monkeypatch.setenv("DC_WINOGRAD43", "0")
    net = _net(gpu_caffe, proto, weights)
    net.blobs["data"].data[...] = x
    net.forward()
    assert "wino_f43" not in net.plan_text()
    with pytest.raises(gpu_caffe.DeepcutError):
        net.set_tile(_signature(net), "wino_f43")


# ---- whole nets: 96 x 128, ResNet-152 with synthetic weights, every 3x3 layer on the form (tile grids 6 x 8, 3 x 4, 2 x 2 and, per phase image of
# the dilated res5 layers, 1 x 1)
H, W = 96, 128
_whole = {}


def _whole_ref(synth152, seed):
    if seed not in _whole:
        from deepcut_tools import deepercut_prototxt
        from oracle import oracle as O

        _path, layers = synth152
        img = rand_image(seed, H, W)
        O.set_threads(min(16, os.cpu_count() or 1))
        ref = O.OracleNet(deepercut_prototxt(152, H, W), layers).forward(data=img)
        _whole[seed] = (img, {k: ref[k].copy() for k in ("prob", "loc_pred", "next_pred")})
    return _whole[seed]


def _whole_net(gpu_caffe, synth152, img, **kw):
    from deepcut_tools import deepercut_prototxt

    path, _layers = synth152
    net = gpu_caffe.Net(deepercut_prototxt(152, H, W), path, gpu_caffe.TEST, from_text=True, **kw)
    net.blobs["data"].data[...] = img
    net.forward()
    _all_on_the_form(net)
    return net


def _all_on_the_form(net):
    sigs = [r["signature"] for r in net.tune_report() if "/3x3/" in r["signature"] and r["signature"].endswith("+w")]
    assert sigs
    for s in sigs:
        net.set_tile(s, "wino_f43")
    assert sum(LABEL in ln for ln in net.plan_text().splitlines()) == 50  # 47 plain + 3 dilated 3x3 layers


@pytest.mark.parametrize("hipgraph", [0, 1], ids=["launches", "hipgraph"])
def test_a_whole_net_with_every_3x3_layer_on_the_form(gpu_caffe, synth152, hipgraph):
    """Measured on MI355X (launches and hipGraph alike, capture and replay alike): max|hip - oracle| prob 4.5e-07, loc_pred 2.5e-06, next_pred 2.8e-06
    (bound 1e-3)."""
    img, ref = _whole_ref(synth152, 3)
    net = _whole_net(gpu_caffe, synth152, img, hipgraph=hipgraph)
    for _ in range(2):  # (with hipgraph: the capture, then a replay)
        net.blobs["data"].data[...] = img
        net.forward()
        for k in ref:
            err = float(np.abs(net.blobs[k].data - ref[k]).max())
            print("whole net on wino_f43, hipgraph %d, %s: max|hip - oracle| = %.3e" % (hipgraph, k, err))
            assert err <= 1e-3, (k, err)


def test_two_clones_back_to_back_keep_their_own_transforms(gpu_caffe, synth152):
    """A net and its clone, each with its own image, enqueued on their own streams without a wait in between, three times over: each against its
    own reference.  V and M are per executor; shared between the two, one forward's products would be read by the other's inverse transform."""
    refs = [_whole_ref(synth152, 3), _whole_ref(synth152, 4)]
    net = _whole_net(gpu_caffe, synth152, refs[0][0])
    clone = net.clone()
    clone.blobs["data"].data[...] = refs[1][0]
    clone.forward()
    _all_on_the_form(clone)
    nets = [net, clone]
    outs = [{k: np.empty(refs[i][1][k].shape, np.float32) for k in refs[i][1]} for i in range(2)]
    for _ in range(3):
        for i in range(2):
            nets[i].forward_host_async(refs[i][0], outs[i]["prob"], outs[i]["loc_pred"], outs[i]["next_pred"])
    for n in nets:
        n.synchronize()
    for i in range(2):
        for k in outs[i]:
            assert float(np.abs(outs[i][k] - refs[i][1][k]).max()) <= 1e-3, (i, k)
