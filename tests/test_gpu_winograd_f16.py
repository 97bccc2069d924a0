"""-m gpu: the float16 Winograd F(2x2,3x3) form of the stride-1 3x3 convolutions (csrc/wino_f16.hip, tile name wino_h23: fp16
operands, fp32 accumulate, fp32 epilogue), forced with DC_WINOGRAD=1; by default it is used only where the per-shape timing
finds it faster.  Reference arithmetic: conv_layer.cpp:25-40, base_conv_layer.cpp:257-280 (the CPU oracle restates them).

Winograd changes the rounding, not the mathematics: the transformed patch B^T d B is formed by packed float16 adds (two roundings
per value) from pixels pre-multiplied by 1/4, the transformed filters are rounded to float16 under a per-channel power of two, the
products accumulate in float32.  What is held:
  * on float16-valued operands, six of CASES against a numpy model of exactly that arithmetic (_wino_model) and against the float64
    convolution — test_single_layers_match_a_model_of_the_forms_arithmetic:
      (a) |got - ref64| <= ulp_f16(ref64) + 2 x max|model - ref64|     (the form's intrinsic error, taken from the model, never the kernel)
      (b) |got - model| <= ulp_f16(model) + 1e-6 x range               (one rounding of the output: the kernel rounds WHAT the model rounds)
  * on operands that are not float16 values, all of CASES (the two large ones only here) within the float16 path's older figure,
    2e-3 x output range; full nets: prob <= 2.5e-3, loc_pred / next_pred <= 4e-3 x range (tests/test_gpu_fp16.py).
Measured on an MI355X over the six model cases: worst |got - ref64| / bound (a) 0.494, worst |got - model| / bound (b) 0.499 (the kernel
rounds what the model rounds: 0.5 is the output's rounding); max|model - ref64| / range = 5.06e-4, 5.35e-4, 2.92e-4, 4.57e-4, 5.87e-4,
5.91e-4 in the order of MODEL_CASES — the form's intrinsic error, about 0.3 of the 2e-3 x range figure."""
import os

import numpy as np
import pytest

from conftest import rand_image
from oracle import oracle as O
from test_gpu_fp16 import _check_maps, _large_activation_weights, f16_operands, f16_round, f16_ulp
from test_gpu_winograd import _conv_net

pytestmark = pytest.mark.gpu
LABEL = "wino_h23<"


@pytest.fixture(autouse=True)
def _force(monkeypatch):
    monkeypatch.setenv("DC_WINOGRAD", "1")
    monkeypatch.setenv("DC_AUTOTUNE", "0")


CASES = [  # n, cin, cout, h, w, dilation, relu
    (8, 256, 256, 34, 46, 1, True),    # the res4 shape of configs[2]'s 544x736 member: two 128-channel blocks
    (1, 64, 64, 31, 45, 1, True),      # odd sizes (ragged last tile row / column), one 64-channel block (NF = 1)
    (2, 128, 128, 17, 9, 1, False),    # batch 2, narrower than one tile block, no ReLU
    (1, 64, 64, 5, 3, 1, True),        # smaller than a tile block in both directions, two staged steps (the least a float16 layer has)
    (1, 192, 192, 12, 20, 1, True),    # six staged steps (the ring wraps twice), 192 = 3 x 64 channels
    (2, 512, 512, 34, 46, 2, True),    # res5: dilation 2 = four interleaved phase images
    (3, 64, 128, 13, 21, 2, False),    # dilation 2, odd sizes, batch 3
    (1, 128, 64, 11, 50, 3, False),    # dilation 3
]


def _weights(rs, cin, cout):
    return [("c", "Convolution", [(rs.randn(cout, cin, 3, 3) / np.sqrt(9.0 * cin)).astype(np.float32)]),
            ("bn", "BatchNorm", [rs.randn(cout).astype(np.float32) * 0.1, rs.uniform(0.5, 1.5, cout).astype(np.float32),
                                 np.array([1.0], np.float32)]),
            ("sc", "Scale", [rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.randn(cout).astype(np.float32) * 0.1])]


@pytest.mark.parametrize("case", CASES)
def test_single_layers_match_oracle(gpu_caffe, case):
    n, cin, cout, h, w, dil, relu = case
    proto, out = _conv_net(n, cin, cout, h, w, dil, relu, False)
    rs = np.random.RandomState(cin + h)
    weights = _weights(rs, cin, cout)
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="f16")
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    x = rs.randn(n, cin, h, w).astype(np.float32)
    net.blobs["data"].data[...] = x
    net.forward()
    assert LABEL in net.plan_text(), "the layer was not lowered to the float16 Winograd kernel"
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, weights).forward(data=x)[out]
    got = net.blobs[out].data
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print("wino_h23 %s: max|hip - oracle| = %.3e (range %.2f)" % (case, err, float(np.abs(ref).max())))
    assert err <= 2e-3 * max(1.0, float(np.abs(ref).max())), err
    assert err > 1e-6, "suspiciously exact: is the float16 kernel really running?"


# ---- a model of the form's own arithmetic ---------------------------------------------------------------------------------------
_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def _bt(d, axis):
    """One pass of B^T along `axis` (length 4) in the array's own precision: one add per value — t0 = d0 - d2, t1 = d1 + d2,
    t2 = d2 - d1, t3 = d1 - d3 (wino_f16.hip: RA / RB / SB of a wave's row, XA / XB of its positions)."""
    d0, d1, d2, d3 = (np.take(d, i, axis=axis) for i in range(4))
    return np.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], axis=axis)


def _fold(weights):
    """BatchNorm (global statistics) and Scale folded as net_lower.cpp folds them, in double: y = a x conv + b."""
    (mean, var, sf), (gamma, beta) = [[np.asarray(v, np.float64) for v in blobs] for _n, _t, blobs in weights[1:]]
    s = 1.0 / np.sqrt(var / sf[0] + 1e-5)
    return gamma * s, beta - mean / sf[0] * s * gamma


def _ref64(x, w, a, b, relu, d):
    n, c, H, W = x.shape
    xp = np.zeros((n, c, H + 2 * d, W + 2 * d))
    xp[:, :, d:d + H, d:d + W] = x
    y = np.zeros((n, w.shape[0], H, W))
    for i in range(3):
        for j in range(3):
            y += np.einsum("ncyx,oc->noyx", xp[:, :, i * d:i * d + H, j * d:j * d + W], w[:, :, i, j].astype(np.float64))
    y = y * a[None, :, None, None] + b[None, :, None, None]
    return np.maximum(y, 0.0) if relu else y


def _wino_model(x, w, a, b, relu, d):
    """wino_h23 in numpy, float16 where the kernel rounds to float16 and float64 where it computes in float32:
      * the pixels are multiplied by 1/4 in float16 when they are staged (sstore);
      * B^T d B by float16 adds, first along the patch rows (stage1), then along its columns (stage2): two roundings per value;
      * U = G g G^T in double, times the power of two that brings the output channel's largest |U| into [2^13, 2^14), to float and
        then to float16 at the upload (wino_half_pack_filters);
      * products, the sum over the input channels and A^T M A in float32 — float64 here;
      * y = A^T M A x float(a x 4 x row scale) + float(b), ReLU; the kernel then rounds ONCE to float16 — the model is returned unrounded.
    Dilation d: d x d phase images, each a pad-1 problem of its own; tiles start at even phase-grid positions, zeros beyond the image."""
    n, c, H, W = x.shape
    co = w.shape[0]
    U = np.einsum("ai,ocij,bj->ocab", _G, w.astype(np.float64), _G)
    mx = np.abs(U).reshape(co, -1).max(axis=1)
    f = np.ldexp(1.0, 13 - (np.frexp(mx)[1] - 1))
    U16 = (U * f[:, None, None, None]).astype(np.float32).astype(np.float16).astype(np.float64)
    scale = (a * 4.0 * (1.0 / f).astype(np.float32)).astype(np.float32).astype(np.float64)
    shift = b.astype(np.float32).astype(np.float64)
    y = np.zeros((n, co, H, W))
    for phy in range(d):
        for phx in range(d):
            ph = x[:, :, phy::d, phx::d]
            Hp, Wp = ph.shape[2:]
            if Hp == 0 or Wp == 0:
                continue
            TY, TX = (Hp + 1) // 2, (Wp + 1) // 2
            xp = np.zeros((n, c, 2 * TY + 2, 2 * TX + 2), np.float16)
            xp[:, :, 1:Hp + 1, 1:Wp + 1] = ph.astype(np.float16) * np.float16(0.25)
            iy = (2 * np.arange(TY))[:, None] + np.arange(4)[None]
            ix = (2 * np.arange(TX))[:, None] + np.arange(4)[None]
            patch = xp[:, :, iy[:, None, :, None], ix[None, :, None, :]]  # n, c, TY, TX, 4 rows, 4 columns: float16
            v = _bt(_bt(patch, 4), 5)
            assert v.dtype == np.float16
            m = np.einsum("ncyxab,ocab->noyxab", v.astype(np.float64), U16)
            t = np.einsum("pa,noyxab,qb->noypxq", _AT, m, _AT).reshape(n, co, 2 * TY, 2 * TX)[:, :, :Hp, :Wp]
            y[:, :, phy::d, phx::d] = t
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    return np.maximum(y, 0.0) if relu else y


MODEL_CASES = [(1, 64, 64, 31, 45, 1), (2, 128, 128, 17, 9, 1), (1, 64, 64, 5, 3, 1), (1, 192, 192, 12, 20, 1), (3, 64, 128, 13, 21, 2), (1, 128, 64, 11, 50, 3)]
assert set(MODEL_CASES) <= set(c[:6] for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c[:6] in MODEL_CASES])
def test_single_layers_match_a_model_of_the_forms_arithmetic(gpu_caffe, case):
    n, cin, cout, h, w, dil, relu = case
    proto, out = _conv_net(n, cin, cout, h, w, dil, relu, False)
    rs = np.random.RandomState(cin + h)
    weights = _weights(rs, cin, cout)
    weights[0] = (weights[0][0], weights[0][1], [f16_operands(weights[0][2][0])])
    x = f16_operands(rs.randn(n, cin, h, w))
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="f16")
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    net.blobs["data"].data[...] = x
    net.forward()
    assert LABEL in net.plan_text(), "the layer was not lowered to the float16 Winograd kernel"
    got = net.blobs[out].data.copy()
    a, b = _fold(weights)
    ref = _ref64(x, weights[0][2][0], a, b, relu, dil)
    model = _wino_model(x, weights[0][2][0], a, b, relu, dil)
    assert got.shape == ref.shape and np.array_equal(got, f16_round(got))
    rng = float(np.abs(ref).max())
    intrinsic = float(np.abs(model - ref).max())
    err_a, bound_a = np.abs(got - ref), f16_ulp(ref) + 2.0 * intrinsic
    err_b, bound_b = np.abs(got - model), f16_ulp(model) + 1e-6 * rng
    at = np.unravel_index(int(np.argmax(err_b / bound_b)), err_b.shape)
    print("wino_h23 %s: max|model - ref64| = %.3e = %.3e x range (%.3g); worst |got - ref64| / bound (a) %.3f; worst |got - model| / bound (b) "
          "%.3f at %s (got %r, model %r, ref64 %r)" % (case, intrinsic, intrinsic / rng, rng, float((err_a / bound_a).max()),
                                                          float((err_b / bound_b).max()), at, float(got[at]), float(model[at]), float(ref[at])))
    assert 1e-5 * rng < intrinsic <= 2e-3 * rng, "the model's distance from the convolution is the form's intrinsic error"
    assert float((err_a - bound_a).max()) <= 0, "(a): worst excess %g" % float((err_a - bound_a).max())
    assert float((err_b - bound_b).max()) <= 0, "(b): worst excess %g at %s" % (float((err_b - bound_b).max()), at)


def test_a_shortcut_operand_keeps_the_direct_kernel(gpu_caffe):
    """the kernel has no shortcut operand (no 3x3 layer of the path has one): such a launch stays a gather-GEMM"""
    proto, out = _conv_net(1, 64, 64, 20, 28, 1, True, True)
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="f16")
    assert "wino" not in net.plan_text()


@pytest.mark.parametrize("hw,n", [((104, 136), 2), ((240, 320), 1)])
def test_full_net_with_every_eligible_layer_in_winograd_form(gpu_caffe, synth152, hw, n):
    from deepcut_tools import deepercut_prototxt

    path, layers = synth152
    h, w = hw
    proto = deepercut_prototxt(152, h, w, n)
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16")
    img = rand_image(3, h, w, n=n)
    out = net.forward_batch(img)
    assert sum(LABEL in ln for ln in net.plan_text().splitlines()) == 50  # 47 plain + 3 dilated 3x3 layers
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, layers).forward(data=img)
    _check_maps(out, ref)


@pytest.mark.parametrize("gain", [32.0, 1024.0])
def test_trained_weight_like_magnitudes(gpu_caffe, synth152, tmp_path, gain):
    """As tests/test_gpu_fp16.py::test_fp16_on_trained_weight_like_magnitudes, every 3x3 layer in the Winograd form: with the trunk at
    up to 70 % of float16's largest finite value the transformed patches (sums of four pixels) must not overflow — the kernel
    stages the pixels pre-multiplied by 1/4 — and the transformed filters keep their precision through their own row scale."""
    from deepcut_tools import deepercut_prototxt, write_caffemodel

    _, layers = synth152
    big = _large_activation_weights(layers, gain)
    path = str(tmp_path / "big.caffemodel")
    write_caffemodel(path, "ResNet-152", big)
    h, w = 104, 136
    proto = deepercut_prototxt(152, h, w, 1)
    img = rand_image(33, h, w)
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, big).forward(data=img)
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16", fuse=0)
    net.blobs["data"].data[...] = img
    out = net.forward()
    assert sum(LABEL in ln for ln in net.plan_text().splitlines()) == 50
    for k in ("prob", "loc_pred", "next_pred"):
        assert np.isfinite(out[k]).all(), k
    _check_maps(out, ref)
    for name in ("res4b35", "res5c"):
        r = ref[name]
        got = net.blobs[name].data
        assert np.isfinite(got).all(), name
        assert float(np.abs(got - r).max()) <= 1e-2 * float(np.abs(r).max()), name


def test_autotuner_times_the_form_and_set_tile_takes_it(gpu_caffe, monkeypatch):
    """unset DC_WINOGRAD: the form competes with the direct tiles per shape (the tune report lists its timing), and
    set_tile / the tune-cache name `wino_h23` select it"""
    monkeypatch.delenv("DC_WINOGRAD")
    monkeypatch.delenv("DC_AUTOTUNE")
    proto, out = _conv_net(8, 256, 256, 34, 46, 1, True, False)
    net = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="f16")
    rs = np.random.RandomState(1)
    for name, _t, blobs in _weights(rs, 256, 256):
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    x = rs.randn(8, 256, 34, 46).astype(np.float32)
    net.blobs["data"].data[...] = x
    net.forward()
    a = net.blobs[out].data.copy()
    (ent,) = [e for e in net.tune_report() if "+w" in e["signature"]]
    assert any(t[0] == "wino_h23" for t in ent["timed"]), ent
    other = "wino_h23" if ent["tile"] != "wino_h23" else [t[0] for t in ent["timed"] if t[0] != "wino_h23"][0]
    net.set_tile(ent["signature"], other)
    net.blobs["data"].data[...] = x
    net.forward()
    b = net.blobs[out].data
    assert ("wino_h23<" in net.plan_text()) == (other == "wino_h23")
    assert float(np.abs(a - b).max()) <= 4e-3 * max(1.0, float(np.abs(a).max()))
