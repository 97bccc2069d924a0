"""-m gpu: the mixed-block forms of the float32 Winograd kernel (wino_f32.hip, WinoGMix; tiles wino_f23_mix and wino_f23_mix_w16): one
launch whose workgroups run 4 x 8-tile blocks in front of a straight cut of the tile grid and 5 x 6-tile blocks behind it.  Put in place
with set_tile on single 3x3 layers and on every 3x3 layer of a small whole net.  Bit for bit against the 4 x 8 form of the same wave count
(a tile's arithmetic does not depend on the block slot it sits in; the 8- and the 16-wave forms differ from each other by float32 rounding,
tests/test_gpu_winograd.py, so each is compared with its own), and against the CPU oracle at the bound tests/test_gpu_winograd.py holds
single layers to: 1e-4 * max(1, max|reference|), and the error of the form's float32 emulation with sequential sums (tests/f32_ref.py)."""
import os

import numpy as np
import pytest

import f32_ref as F
from conftest import rand_image
from test_gpu_winograd import wino_case

pytestmark = pytest.mark.gpu

FORMS = [("wino_f23_mix", "wino_f23", "wino_f23<4x8+5x6x16>", "wino_f23<4x8x16>"),
         ("wino_f23_mix_w16", "wino_f23_w16", "wino_f23<4x8+5x6x16_w16>", "wino_f23<4x8x16_w16>")]


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv("DC_AUTOTUNE", "0")  # the forms are put in place by set_tile
    monkeypatch.delenv("DC_WINOGRAD", raising=False)
    monkeypatch.delenv("DC_TUNE_CACHE", raising=False)


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


# Cin = 128: four 32-channel steps, one past the ring of three (the dilated case: 64, two).  Cout = 32: two 16-channel slices; the cases with a
# shortcut add the layer's input, so they have Cout = Cin = 128 (eight slices).
CASES = [  # n, cin, cout, h, w, dilation, relu, shortcut     tiles per phase image, (vertical cut, blocks of 4 x 8, of 5 x 6)
    ((1, 128, 32, 34, 46, 1, False, False), (17, 23), (0, 9, 4)),    # the res4 grid of the benchmark: a horizontal cut
    ((1, 128, 128, 34, 46, 1, True, True), (17, 23), (0, 9, 4)),     # ... with shortcut + ReLU
    ((1, 128, 32, 33, 45, 1, True, False), (17, 23), (0, 9, 4)),     # odd sizes: the last tile row and column half outside the image
    ((2, 128, 128, 33, 45, 1, True, True), (17, 23), (0, 9, 4)),     # ... batch 2, shortcut + ReLU
    ((1, 128, 32, 18, 26, 1, True, False), (9, 13), (1, 3, 2)),      # the smallest vertical cut (tests/test_wino_cover.py): 5 blocks against 6 / 6
    ((2, 128, 128, 40, 28, 1, False, True), (20, 14), (1, 5, 4)),    # a vertical cut, 9 blocks against 10 / 12: batch 2, shortcut without ReLU
    ((1, 128, 32, 27, 54, 1, False, False), (14, 27), (1, 8, 6)),    # a vertical cut with two block columns on either side, odd height
    ((1, 64, 32, 68, 92, 2, True, False), (17, 23), (0, 9, 4)),      # dilation 2: four phase images of 17 x 23 tiles
    ((1, 128, 32, 18, 24, 1, True, False), (9, 12), (0, 0, 4)),      # not offered: the planner's cover is the pure 5 x 6 one, set_tile still runs it
]
_reference = {}  # case -> (prototxt, output blob, weights, input, oracle output): made once, shared by the two forms


def _case_data(case):
    if case not in _reference:
        from oracle import oracle as O

        n, cin, cout, h, w, dil, relu, resid = case
        proto, out = _conv_net(n, cin, cout, h, w, dil, relu, resid)
        rs = np.random.RandomState(cin + h)
        weights = [("c", "Convolution", [(rs.randn(cout, cin, 3, 3) / np.sqrt(9.0 * cin)).astype(np.float32)]),
                   ("bn", "BatchNorm", [rs.randn(cout).astype(np.float32) * 0.1, rs.uniform(0.5, 1.5, cout).astype(np.float32),
                                        np.array([1.0], np.float32)]),
                   ("sc", "Scale", [rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.randn(cout).astype(np.float32) * 0.1])]
        x = rs.randn(n, cin, h, w).astype(np.float32)
        O.set_threads(min(16, os.cpu_count() or 1))
        ref = O.OracleNet(proto, weights).forward(data=x)[out]
        ref.setflags(write=False)
        _reference[case] = (proto, out, weights, x, ref)
    return _reference[case]


def _signature(net):
    sigs = [r["signature"] for r in net.tune_report() if "/3x3/" in r["signature"]]
    assert len(sigs) == 1, sigs
    return sigs[0]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("case,tiles,cover", CASES, ids=["%dx%dx%d_%dx%d_d%d%s%s" % (c[0][:6] + ("_relu" if c[0][6] else "", "_sum" if c[0][7] else "")) for c in CASES])
def test_single_layers_match_the_4x8_form_and_the_oracle(gpu_caffe, case, tiles, cover, form):
    tile, tile48, label, label48 = form
    c = gpu_caffe.wino_cover(*tiles)
    assert (c["vertical"] if c["na"] and c["nb"] else 0, c["na"], c["nb"]) == cover, c  # the case runs the cover it is here for
    proto, out, weights, x, ref = _case_data(case)
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True)
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    got = {}
    for t in (None, tile48, tile):  # (the first forward lowers the shape; the tiles are then put in place on its plan)
        if t:
            net.set_tile(_signature(net), t)
        net.blobs["data"].data[...] = x
        net.forward()
        got[t] = net.blobs[out].data.copy()
        if t:
            assert (label if t == tile else label48) in net.plan_text(), "the layer does not run on " + t
    assert got[tile].shape == ref.shape
    err = float(np.abs(got[tile] - ref).max())
    bound = 1e-4 * max(1.0, float(np.abs(ref).max()))
    print("%s %s: max|hip - oracle| = %.3e (bound %.3e), differing elements against %s: %d" % (tile, case, err, bound, tile48, int((got[tile] != got[tile48]).sum())))
    assert err <= bound, (err, bound)
    ref64, model, pixels = wino_case(case, weights, x)
    F.assert_f32_tight(got[tile], ref64, model, "wino_f23_mix: %s %s" % (tile, case), pixels)
    assert np.array_equal(got[tile], got[tile48]), "not bit-identical to the 4 x 8 form"


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_a_whole_net_with_every_3x3_layer_on_the_mixed_form(gpu_caffe, synth152, form):
    """240 x 320: tile grids of 30 x 40 (res2), 15 x 20 (res3), 8 x 10 (res4) and, per phase image of the dilated res5 layers, 4 x 5 tiles —
    covers with and without a cut.  Every map has the bits it has with those layers on the 4 x 8 Winograd form."""
    from deepcut_tools import deepercut_prototxt

    tile, tile48, label, label48 = form
    path, _layers = synth152
    h, w = 240, 320
    net = gpu_caffe.Net(deepercut_prototxt(152, h, w), path, gpu_caffe.TEST, from_text=True)
    img = rand_image(3, h, w)
    maps = {}
    for t, lab in ((None, None), (tile48, label48), (tile, label)):
        if t:
            sigs = [r["signature"] for r in net.tune_report() if "/3x3/" in r["signature"] and r["signature"].endswith("+w")]
            assert sigs
            for s in sigs:
                net.set_tile(s, t)
        net.blobs["data"].data[...] = img
        net.forward()
        if t:
            assert sum(lab in ln for ln in net.plan_text().splitlines()) == 50  # 47 plain + 3 dilated 3x3 layers
            maps[t] = {k: net.blobs[k].data.copy() for k in ("prob", "loc_pred", "next_pred")}
    for k in maps[tile]:
        assert np.isfinite(maps[tile][k]).all() and float(np.abs(maps[tile][k]).max()) > 0, k
        assert np.array_equal(maps[tile][k], maps[tile48][k]), k
