"""-m gpu: the 5 x 6-tile block forms of the float32 Winograd kernel (wino_f32.hip, WinoGeom<5, 3, side by side>; tiles wino_f23_5x6 and
wino_f23_5x6_w16), put in place with set_tile on single 3x3 layers and on the res5 layers of the full net.  Against the CPU oracle at the
suite's bound (<= 1e-3 max-abs) and, single layers, at the error of the form's float32 emulation with sequential sums (tests/f32_ref.py:
3 x its maximum, 2 x its RMS error against a float64 reference), and bit for bit against the 4 x 8 form of the same wave count: a tile's arithmetic (channel order, order
of the partial sums in the epilogue) does not depend on the block slot it sits in."""
import os

import numpy as np
import pytest

import f32_ref as F
from conftest import rand_image
from test_gpu_winograd import wino_case

pytestmark = pytest.mark.gpu

FORMS = [("wino_f23_5x6", "wino_f23", "wino_f23<5x6x16>"), ("wino_f23_5x6_w16", "wino_f23_w16", "wino_f23<5x6x16_w16>")]


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv("DC_AUTOTUNE", "0")  # the forms are put in place by set_tile
    monkeypatch.delenv("DC_WINOGRAD", raising=False)
    monkeypatch.delenv("DC_TUNE_CACHE", raising=False)


def _oracle(proto, layers, img):
    from oracle import oracle as O

    O.set_threads(min(16, os.cpu_count() or 1))
    return O.OracleNet(proto, layers).forward(data=img)


def _conv_net(n, cin, cout, h, w, dil, relu, resid):
    L = ['name: "w"', 'input: "data"'] + ["input_dim: %d" % d for d in (n, cin, h, w)]
    L.append('layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: %d kernel_size: 3 '
             'pad: %d dilation: %d bias_term: false } }' % (cout, dil, dil))
    L.append('layer { name: "bn" type: "BatchNorm" bottom: "c" top: "c" batch_norm_param { use_global_stats: true } }')
    L.append('layer { name: "sc" type: "Scale" bottom: "c" top: "c" scale_param { bias_term: true } }')
    out = "c"
    if resid:
        L.append('layer { name: "sum" type: "Eltwise" bottom: "data" bottom: "c" top: "sum" }')
        out = "sum"
    if relu:
        L.append('layer { name: "relu" type: "ReLU" bottom: "%s" top: "%s" }' % (out, out))
    return "\n".join(L) + "\n", out


CASES = [  # n, cin, cout, h, w, dilation, relu, shortcut          tile grid per phase image
    (1, 512, 512, 34, 46, 2, True, False),   # the res5 shape of the benchmark: 9 x 12 tiles = 2 x 2 blocks
    (1, 64, 64, 31, 45, 1, True, False),     # 16 x 23 tiles, odd pixel sizes: ragged last block row / column and last tile
    (2, 128, 128, 17, 9, 1, False, False),   # batch 2, 9 x 5 tiles: narrower than a block
    (1, 32, 16, 2, 37, 1, True, False),      # one tile high, 19 wide
    (1, 32, 32, 27, 1, 1, False, False),     # one tile (one pixel) wide, 14 high
    (1, 32, 16, 1, 1, 1, True, False),       # a single pixel
    (3, 64, 96, 13, 21, 2, False, False),    # dilation 2, odd sizes, batch 3: 4 x 6 tiles
    (1, 64, 64, 20, 28, 1, True, True),      # shortcut + ReLU, 10 x 14 tiles: full blocks in y, ragged in x
    (2, 64, 64, 22, 26, 1, False, True),     # batch 2, shortcut without ReLU, 11 x 13 tiles
    (1, 96, 48, 11, 50, 3, False, False),    # dilation 3: 2 x 9 tiles
    (1, 64, 64, 23, 37, 4, True, True),      # dilation 4, shortcut + ReLU: 3 x 5 tiles
]


def _signature(net):
    sigs = [r["signature"] for r in net.tune_report() if "/3x3/" in r["signature"]]
    assert len(sigs) == 1, sigs
    return sigs[0]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("case", CASES)
def test_single_layers_match_the_oracle_and_the_4x8_form(gpu_caffe, case, form):
    tile, tile48, label = form
    n, cin, cout, h, w, dil, relu, resid = case
    proto, out = _conv_net(n, cin, cout, h, w, dil, relu, resid)
    rs = np.random.RandomState(cin + h)
    weights = [("c", "Convolution", [(rs.randn(cout, cin, 3, 3) / np.sqrt(9.0 * cin)).astype(np.float32)]),
               ("bn", "BatchNorm", [rs.randn(cout).astype(np.float32) * 0.1, rs.uniform(0.5, 1.5, cout).astype(np.float32),
                                    np.array([1.0], np.float32)]),
               ("sc", "Scale", [rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.randn(cout).astype(np.float32) * 0.1])]
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True)
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    x = rs.randn(n, cin, h, w).astype(np.float32)
    got = {}
    for t in (None, tile48, tile):  # (the first forward lowers the shape; the tiles are then put in place on its plan)
        if t:
            net.set_tile(_signature(net), t)
        net.blobs["data"].data[...] = x
        net.forward()
        got[t] = net.blobs[out].data.copy()
        if t:  # the comparison below is between the two Winograd forms, not with a direct tile
            assert (label if t == tile else label.replace("5x6", "4x8")) in net.plan_text(), "the layer does not run on " + t
    ref = _oracle(proto, weights, x)[out]
    assert got[tile].shape == ref.shape
    err = float(np.abs(got[tile] - ref).max())
    print("%s %s: max|hip - oracle| = %.3e, differing elements against %s: %d" % (tile, case, err, tile48, int((got[tile] != got[tile48]).sum())))
    assert err <= 1e-3, err
    ref64, model, pixels = wino_case(case, weights, x)
    F.assert_f32_tight(got[tile], ref64, model, "wino_f23_5x6: %s %s" % (tile, case), pixels)
    assert np.array_equal(got[tile], got[tile48]), "not bit-identical to the 4 x 8 form"


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_full_net_at_the_bench_shape_with_res5_on_the_5x6_form(gpu_caffe, synth152, form):
    from deepcut_tools import deepercut_prototxt

    tile, _tile48, label = form
    path, layers = synth152
    h, w = 544, 736
    proto = deepercut_prototxt(152, h, w)
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True)
    img = rand_image(3, h, w)
    net.blobs["data"].data[...] = img
    net.forward()
    res5 = [r for r in net.tune_report() if "/3x3/" in r["signature"] and r["signature"].split("/")[1] == "512"]
    assert len(res5) == 1 and res5[0]["launches"] == 3, res5
    net.set_tile(res5[0]["signature"], tile)
    net.blobs["data"].data[...] = img
    net.forward()
    assert sum(label in ln for ln in net.plan_text().splitlines()) == 3
    ref = _oracle(proto, layers, img)
    for k in ("prob", "loc_pred", "next_pred"):
        err = float(np.abs(net.blobs[k].data - ref[k]).max())
        print("%s %-9s max|hip - oracle| = %.3e" % (tile, k, err))
        assert err <= 1e-3, (k, err)


def test_the_autotuner_is_offered_the_5x6_forms_for_res5_only_and_takes_one(gpu_caffe, synth152, monkeypatch):
    """At 544x736 the dilated res5 layers (9 x 12 tiles per phase image) are the only Winograd layers that need fewer 5 x 6 blocks than 4 x 8
    ones: their signature is timed on all four forms, every other one on the two 4 x 8 forms only.  A fresh tuning takes a 5 x 6 form for it
    (timed alone 45 against 67 us: two thirds of the workgroups)."""
    from deepcut_tools import deepercut_prototxt

    monkeypatch.setenv("DC_AUTOTUNE", "1")
    path, _ = synth152
    net = gpu_caffe.Net(deepercut_prototxt(152, 544, 736), path, gpu_caffe.TEST, from_text=True)
    net.blobs["data"].data[...] = rand_image(3, 544, 736)
    net.forward()
    new = {"wino_f23_5x6", "wino_f23_5x6_w16"}
    for r in net.tune_report():
        timed = set(t for t, _ in r["timed"])
        if "/3x3/" in r["signature"] and r["signature"].split("/")[1] == "512":
            print("res5 3x3:", r["tile"], r["timed"])
            assert new <= timed and {"wino_f23", "wino_f23_w16"} <= timed
            assert r["tile"] in new, r
        else:
            assert not (new & timed), r
