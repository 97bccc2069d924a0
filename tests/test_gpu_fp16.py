"""-m gpu: the float16 path (DC_OPT_DTYPE 1, BASELINE configs[2]: fp16 operands in HBM, v_mfma_f32_32x32x16_f16
with float32 accumulation and float32 epilogue) against the CPU oracle.

Single layers on float16-representable operands (f16_operands below) are held to ONE rounding of the output: the oracle accumulates
in double and |got - ref| <= ulp_f16(ref) + 1e-6 x range — the 26 convolution / deconvolution configurations of the net
(test_fp16_conv_deconv_configs), every h... / d... tile (test_gpu_tile_shapes.py), the streaming and stem forms
(test_gpu_fp16_forms.py, + 1e-5 x max(1, range) as their bfloat16 twins), the per-row filter scaling
(test_fp16_row_scaling_keeps_small_filter_rows, range taken per output channel).  The filter upload and the input conversion round to
nearest even bit for bit; max-pool, crop and eltwise are exact against the oracle rounded to float16.  wino_h23 rounds differently
by design and is held to a model of its own arithmetic (test_gpu_winograd_f16.py).

The older figure, 2e-3 x max(1, range) per layer (one rounding of inputs, weights and output), still applies where the operands are
NOT float16 values (test_fp16_single_layers, and the forms' own files), to the two large Winograd cases, and — as the larger figures
below — to full nets, whose activations are rounded to 11 significant bits after each of 152 layers:
  prob      <= 2.5e-3 max-abs          (measured ~9e-4 at 240x320; the sigmoid compresses the error)
  loc_pred, next_pred <= 4e-3 x max(1, range of the map)   (measured ~1.4e-3 x range)

Worst |got - bound's reference| / bound measured on an MI355X, per group (0.5 is the one rounding itself; no row needed more than the
1e-6 x range accumulation term):
  the 26 T2 rows 0.499 | every float16 tile on the small nets 0.499 | ws1x1 0.491 | stem7x7 0.490 | row scaling 0.498 (small rows 0.492)
  wino_h23 (a) 0.494, (b) 0.499, with max|model - ref64| / range = 5.06e-4, 5.35e-4, 2.92e-4, 4.57e-4, 5.87e-4, 5.91e-4 on its six cases"""
import os
import zlib

import numpy as np
import pytest

from conftest import rand_image
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def f16_round(a):
    """float32 -> the nearest float16 (ties to even), as float32."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def f16_ulp(a):
    """2^(floor(log2(max(|a|, 2^-14))) - 10): the spacing of float16 at a (any real a, float64 inside); below the smallest normal
    number it stays at the subnormal spacing 2^-24.  (frexp, not log2: log2 of the float just below a power of two rounds up.)"""
    m = np.maximum(np.abs(np.asarray(a, np.float64)), 2.0 ** -14)
    return np.ldexp(1.0, np.frexp(m)[1] - 1 - 10)


def f16_operands(a):
    """f16_round, then every value with |v| < 2^-14 set to 0: operands a float16 kernel reads exactly and that are never subnormal.
    How the matrix unit treats float16 SUBNORMAL inputs (kept or flushed) has not been established here, and the one-ulp bounds
    of the tight tests must not rest on it: subnormal operands are out of their scope."""
    r = f16_round(a)
    return np.where(np.abs(r) < 2.0 ** -14, np.float32(0), r)


def _check_maps(out, ref):
    assert float(np.abs(out["prob"] - ref["prob"]).max()) <= 2.5e-3
    for k in ("loc_pred", "next_pred"):
        rng = max(1.0, float(np.abs(ref[k]).max()))
        err = float(np.abs(out[k] - ref[k]).max())
        assert err <= 4e-3 * rng, (k, err, rng)
        assert err > 1e-5, "suspiciously exact: is the fp16 path really running?"


@pytest.mark.parametrize("fuse", [0, 2])
@pytest.mark.parametrize("hw", [(64, 64), (104, 136)])
def test_fp16_full_net_matches_oracle(gpu_caffe, synth152, hw, fuse):
    from deepcut_tools import deepercut_prototxt

    path, layers = synth152
    h, w = hw
    proto = deepercut_prototxt(152, h, w, 2)
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16", fuse=fuse)
    assert "dtype=f16" in net.plan_text() and "conv_gemm<h" in net.plan_text()
    img = rand_image(31, h, w, n=2)
    net.blobs["data"].data[...] = img
    out = net.forward()
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, layers).forward(data=img)
    _check_maps(out, ref)
    if fuse == 0:  # intermediate blobs too, relative to their range
        for name in ("conv1", "pool1", "res2c", "res3b7", "res4b35", "res5c"):
            r = ref[name]
            assert float(np.abs(net.blobs[name].data - r).max()) <= 1e-2 * max(1.0, float(np.abs(r).max())), name


def test_fp16_pyramid_scale_batch8(gpu_caffe, synth152):
    """BASELINE configs[2]: batch of 8 at the 0.5 scale of 736x544 (272x368), fp16 MFMA with fp32 accumulate."""
    from deepcut_tools import deepercut_prototxt

    path, layers = synth152
    h, w = 272, 368
    proto = deepercut_prototxt(152, h, w, 8)
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16")
    imgs = rand_image(10, h, w, n=8)
    out = net.forward_batch(imgs)
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, layers).forward(data=imgs)
    _check_maps(out, ref)
    pose = net.decode_pose(0.5)  # the device decode reads the half maps
    assert pose.shape == (8, 5, 14) and np.isfinite(pose).all()


def test_switching_dtype_on_a_live_net(gpu_caffe, synth152):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    net = gpu_caffe.Net(deepercut_prototxt(152, 64, 64), path, gpu_caffe.TEST, from_text=True)
    img = rand_image(32, 64, 64)
    net.blobs["data"].data[...] = img
    a = {k: v.copy() for k, v in net.forward().items()}
    net.set_option(3, 1)
    net.blobs["data"].data[...] = img
    b = {k: v.copy() for k, v in net.forward().items()}
    net.set_option(3, 0)
    net.blobs["data"].data[...] = img
    c = net.forward()
    for k in a:
        assert np.array_equal(a[k], c[k]), k              # float32 is reproduced bit for bit
        d = float(np.abs(a[k] - b[k]).max())
        assert 1e-6 < d < 2e-2, (k, d)                    # float16 differs, slightly


@pytest.mark.parametrize("cfg", [("conv", 7, 2, 3, 1, 3, 64, 41, 54), ("conv", 3, 1, 1, 1, 64, 64, 13, 17),
                                 ("conv", 1, 2, 0, 1, 256, 128, 14, 18), ("conv", 3, 1, 2, 2, 512, 512, 7, 9),
                                 ("conv", 1, 1, 0, 1, 2048, 512, 5, 6), ("deconv", 3, 2, 0, 1, 2048, 28, 4, 5)])
def test_fp16_single_layers(gpu_caffe, cfg):
    kind, k, s, p, d, cin, cout, h, w = cfg
    rs = np.random.RandomState(zlib.crc32(repr(cfg).encode()) & 0x7fffffff)  # (hash() of a tuple holding a str moves with PYTHONHASHSEED)
    typ = "Convolution" if kind == "conv" else "Deconvolution"
    text = ('input: "x" input_dim: 2 input_dim: %d input_dim: %d input_dim: %d\n' % (cin, h, w) +
            'layer { name: "l" type: "%s" bottom: "x" top: "y" convolution_param { num_output: %d kernel_size: %d '
            "stride: %d pad: %d dilation: %d } }" % (typ, cout, k, s, p, d))
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    x = rs.randn(2, cin, h, w).astype(np.float32)
    wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    wt = (rs.randn(*wshape) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    net.params["l"][0].data[...] = wt
    net.params["l"][1].data[...] = b
    net.blobs["x"].data[...] = x
    got = net.forward()["y"]
    ref = (O.conv_forward if kind == "conv" else O.deconv_forward)(x, wt, b, s, p, d)
    assert got.shape == ref.shape
    assert float(np.abs(got - ref).max()) <= 2e-3 * max(1.0, float(np.abs(ref).max()))


# ---- single layers on float16 operands: one rounding ------------------------------------------------------------------------------
from test_gpu_layers import T2, _inp  # noqa: E402  (the 26 convolution / deconvolution configurations of the net)


@pytest.mark.parametrize("cfg", T2, ids=lambda c: "%s_k%ds%dp%dd%d_%dto%d" % (c[0], c[1], c[2], c[3], c[4], c[6], c[7]))
def test_fp16_conv_deconv_configs(gpu_caffe, cfg, monkeypatch):
    """As test_bf16_conv_deconv_configs: operands that are float16 values, the oracle accumulating in double, one rounding of the
    output.  The Winograd form is off (it rounds its transformed patches: test_gpu_winograd_f16.py holds it to its own model); the
    streaming and stem forms stay at their defaults — they claim the tiles' arithmetic."""
    monkeypatch.setenv("DC_WINOGRAD", "0")
    kind, k, s, p, d, bias, cin, cout, h, w = cfg
    rs = np.random.RandomState(zlib.crc32(repr(cfg).encode()) & 0x7fffffff)
    typ = "Convolution" if kind == "conv" else "Deconvolution"
    text = _inp("x", (2, cin, h, w)) + (
        'layer { name: "l" type: "%s" bottom: "x" top: "y" convolution_param { num_output: %d kernel_size: %d '
        "stride: %d pad: %d dilation: %d bias_term: %s } }" % (typ, cout, k, s, p, d, "true" if bias else "false"))
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    x = f16_operands(rs.randn(2, cin, h, w))
    wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    wt = f16_operands(rs.randn(*wshape) / np.sqrt(cin * k * k))
    b = rs.randn(cout).astype(np.float32) if bias else None
    net.params["l"][0].data[...] = wt
    if bias:
        net.params["l"][1].data[...] = b
    net.blobs["x"].data[...] = x
    got = net.forward()["y"]
    O.set_double_acc(True)
    try:
        ref = (O.conv_forward if kind == "conv" else O.deconv_forward)(x, wt, b, s, p, d)
    finally:
        O.set_double_acc(False)
    assert got.shape == ref.shape
    assert np.array_equal(got, f16_round(got)), "outputs are float16 values"
    rng = float(np.abs(ref).max())
    bound = f16_ulp(ref) + 1e-6 * rng
    err = np.abs(got.astype(np.float64) - ref)
    at = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    tiles = sorted(set(ln.split("\t")[1] for ln in net.plan_text().splitlines() if not ln.startswith("#") and "\t" in ln))
    print("f16 %s: worst |got - ref| / bound = %.3f at %s (got %r, ref %r, range %.3g) on %s" % (
        cfg, float((err / bound).max()), at, float(got[at]), float(ref[at]), rng, tiles))
    assert float((err - bound).max()) <= 0, "worst excess %g (range %g)" % (float((err - bound).max()), rng)


def _one_hot_layer(gpu_caffe, cin, cout, wt, bias=None):
    """A 1x1 layer over `cin` one-hot pixels: y[co, j] = w[co, j] (+ bias[co]) — every converted weight read back."""
    text = _inp("x", (1, cin, 1, cin)) + ('layer { name: "l" type: "Convolution" bottom: "x" top: "y" '
                                          "convolution_param { num_output: %d kernel_size: 1 bias_term: %s } }" % (cout, "true" if bias is not None else "false"))
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    net.params["l"][0].data[...] = wt
    if bias is not None:
        net.params["l"][1].data[...] = bias
    x = np.zeros((1, cin, 1, cin), np.float32)
    x[0, np.arange(cin), 0, np.arange(cin)] = 1.0  # pixel j holds e_j
    net.blobs["x"].data[...] = x
    return net.forward()["y"][0, :, 0, :].copy()


def _ties(a, idx):
    """The float32 values a[idx] moved onto exact float16 ties: the low 13 mantissa bits become 0x1000."""
    u = a.view(np.uint32)
    u[idx] = (u[idx] & np.uint32(0xFFFFE000)) | np.uint32(0x1000)


def test_fp16_filter_upload_rounds_to_nearest_even(gpu_caffe):
    """Weights that are NOT float16 values (N(0,1), eight exact ties, the smallest normal binade, all |w| >= 2^-14): the upload scales
    every filter row by a power of two (DevVec::row_scale) and converts it on the device; what comes back through the epilogue's
    inverse scale must be numpy's round-to-nearest-even of the weight, bit for bit — the row scale changes no rounding."""
    cin, cout = 64, 64
    rs = np.random.RandomState(5)
    wt = rs.randn(cout, cin, 1, 1).astype(np.float32)
    wt[1, :4, 0, 0] = [2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -11), 1.3e-4, -7e-5]  # the bottom of the normal range (a tie among them)
    small = np.abs(wt) < 2.0 ** -14
    wt[small] = np.float32(0.37)
    _ties(wt[0, :, 0, 0], slice(0, 8))
    assert (np.abs(wt) >= 2.0 ** -14).all()
    assert int((f16_round(wt) != wt).sum()) > 4000 and (wt.view(np.uint32)[0, :8, 0, 0] & 0x1FFF == 0x1000).all()
    y = _one_hot_layer(gpu_caffe, cin, cout, wt)
    assert np.array_equal(y, f16_round(wt[:, :, 0, 0]))


def test_fp16_input_conversion_rounds_to_nearest_even(gpu_caffe):
    """The same layer with identity filters: y is the converted input, which must be f16_round(x) for an x that is not float16
    values — ties, values up to the thousands and down to the smallest normal binade included."""
    c, npix = 64, 96
    rs = np.random.RandomState(6)
    x = (rs.randn(1, c, 1, npix) * np.exp2(rs.randint(-10, 11, (1, c, 1, npix)))).astype(np.float32)
    x[np.abs(x) < 2.0 ** -14] = np.float32(2.0 ** -14 * 1.5)
    _ties(x[0, :, 0, 0], slice(0, 8))
    _ties(x[0, 5, 0, :], slice(8, 16))
    assert int((f16_round(x) != x).sum()) > 5000
    text = _inp("x", (1, c, 1, npix)) + ('layer { name: "l" type: "Convolution" bottom: "x" top: "y" '
                                         "convolution_param { num_output: %d kernel_size: 1 bias_term: false } }" % c)
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    net.params["l"][0].data[...] = np.eye(c, dtype=np.float32).reshape(c, c, 1, 1)
    net.blobs["x"].data[...] = x
    assert np.array_equal(net.forward()["y"], f16_round(x))


def _row_scaled_f16(w):
    """The filter rows as the lowering stores them (net_lower.cpp, half_row_scale): k = 13 - floor(log2(max|row|)) brings the row's
    largest magnitude into [2^13, 2^14), w' = f16_round(w x 2^k) / 2^k; an all-zero row stays as it is.  -> float64"""
    w = np.asarray(w, np.float32)
    mx = np.abs(w).max(axis=1)
    k = np.where(mx > 0, 13 - (np.frexp(np.where(mx > 0, mx, 1.0))[1] - 1), 0)
    f = np.ldexp(1.0, k)[:, None]
    return f16_round(w.astype(np.float64) * f).astype(np.float64) / f


def test_fp16_row_scaling_keeps_small_filter_rows(gpu_caffe):
    """What DevVec::row_scale is for: filter rows of magnitude 1e-5, 1e-6 and 1e-7, of which plain float16 (smallest normal 6.1e-5,
    subnormal spacing 6e-8) would keep a few bits or none, over activations of magnitude ~100.  The reference is float64 over the
    weights rounded as the lowering rounds them; the bound is one rounding of the output, ulp_f16(ref) + 1e-6 x range, the range taken
    PER OUTPUT CHANNEL (the rows differ by seven orders of magnitude: the layer's range would excuse the small rows entirely; float32
    accumulation over K = 64 and the bias add are relative to the row's own sums).  One row is all zero (its output is exactly the
    bias), one has a largest weight that is exactly a power of two (the edge of ilogb)."""
    cin, cout, n, h, w = 64, 64, 2, 5, 7
    rs = np.random.RandomState(7)
    wt = (rs.randn(cout, cin) / 8).astype(np.float32)
    for r, mag in ((3, 1e-5), (4, 1e-6), (5, 1e-7), (40, 1e-5), (41, 1e-7)):
        wt[r] = (mag * rs.uniform(0.25, 1.0, cin) * rs.choice([-1.0, 1.0], cin)).astype(np.float32)
    wt[7] = 0.0
    wt[9] = (rs.uniform(0.01, 0.1, cin) * rs.choice([-1.0, 1.0], cin)).astype(np.float32)
    wt[9, 11] = 0.125  # the row's largest weight: exactly 2^-3
    bias = f16_round(rs.randn(cout))
    bias[[3, 4, 5]] = 0.0  # the small rows' outputs stand alone here; rows 40, 41 add them to an O(1) bias
    x = f16_operands(rs.randn(n, cin, h, w) * 100.0)
    text = _inp("x", (n, cin, h, w)) + ('layer { name: "l" type: "Convolution" bottom: "x" top: "y" '
                                        "convolution_param { num_output: %d kernel_size: 1 bias_term: true } }" % cout)
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    net.params["l"][0].data[...] = wt.reshape(cout, cin, 1, 1)
    net.params["l"][1].data[...] = bias
    net.blobs["x"].data[...] = x
    got = net.forward()["y"]
    ref = np.einsum("oc,nchw->nohw", _row_scaled_f16(wt), x.astype(np.float64)) + bias.astype(np.float64)[None, :, None, None]
    exact = np.einsum("oc,nchw->nohw", wt.astype(np.float64), x.astype(np.float64)) + bias.astype(np.float64)[None, :, None, None]
    rng = np.abs(ref).max(axis=(0, 2, 3), keepdims=True)
    ratio = np.abs(got.astype(np.float64) - ref) / (f16_ulp(ref) + 1e-6 * rng)
    print("row scaling: worst |got - ref| / bound per row group: small rows %.3f, zero row %.3f, power-of-two row %.3f, others %.3f" % (
        float(ratio[:, [3, 4, 5, 40, 41]].max()), float(ratio[:, 7].max()), float(ratio[:, 9].max()),
        float(np.delete(ratio, [3, 4, 5, 7, 9, 40, 41], axis=1).max())))
    assert np.array_equal(got, f16_round(got))
    assert float(ratio.max()) <= 1.0, float(ratio.max())
    assert np.array_equal(got[:, 7], np.broadcast_to(bias[7], got[:, 7].shape)), "the all-zero row returns the bias"
    # the small rows keep their precision against the EXACT weights: every weight is within 2^-11 of itself (relative), then the bound above
    slack = 2.0 ** -11 * np.einsum("oc,nchw->nohw", np.abs(wt).astype(np.float64), np.abs(x).astype(np.float64))
    for r in (3, 4, 5):
        over = np.abs(got[:, r] - exact[:, r]) - (slack[:, r] + f16_ulp(exact[:, r]) + 1e-6 * float(np.abs(exact[:, r]).max()))
        assert float(over.max()) <= 0, (r, float(over.max()))


@pytest.mark.parametrize("hw", [(3, 5), (15, 20), (33, 47)])
def test_fp16_maxpool_is_exact(gpu_caffe, hw):
    text = _inp("x", (2, 64) + hw) + 'layer { name: "p" type: "Pooling" bottom: "x" top: "y" pooling_param { pool: MAX kernel_size: 3 stride: 2 } }'
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    x = f16_round(np.random.RandomState(1).randn(2, 64, *hw) * 1e3)
    net.blobs["x"].data[...] = x
    assert np.array_equal(net.forward()["y"], O.maxpool_forward(x, 3, 2))


def test_fp16_eltwise_crop_are_exact(gpu_caffe):
    text = (_inp("a", (2, 14, 9, 11)) + _inp("b", (2, 14, 8, 10)) +
            'layer { name: "c" type: "Crop" bottom: "a" bottom: "b" top: "ac" }'
            'layer { name: "e" type: "Eltwise" bottom: "b" bottom: "ac" top: "s" }')
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="f16")
    rs = np.random.RandomState(3)
    a, b = f16_round(rs.randn(2, 14, 9, 11)), f16_round(rs.randn(2, 14, 8, 10))
    net.blobs["a"].data[...] = a
    net.blobs["b"].data[...] = b
    net.forward()
    ac = O.crop_forward(a, b)
    assert np.array_equal(net.blobs["ac"].data, ac)
    assert np.array_equal(net.blobs["s"].data, f16_round(b + ac))  # (a + b in float32 is exact for two float16 values)


def _large_activation_weights(layers, gain):
    """Synthetic weights whose trunk activations are `gain` times larger — what the un-normalised blocks of a trained
    ResNet look like — with the head filters divided by `gain` so that the output maps stay O(1): conv1's Scale (gamma,
    beta) is multiplied (the global-statistics BatchNorm layers do not re-normalise, ReLU is positively homogeneous), the
    six head convolutions / deconvolutions (not their biases) are divided."""
    out = []
    for name, t, blobs in layers:
        blobs = [b.copy() for b in blobs]
        if name == "scale_conv1":
            blobs = [b * np.float32(gain) for b in blobs]
        if name.startswith("res5c_up_") or name.startswith("res3d_"):
            blobs[0] = blobs[0] / np.float32(gain)
        out.append((name, t, blobs))
    return out


@pytest.mark.parametrize("gain", [32.0, 256.0, 1024.0])
def test_fp16_on_trained_weight_like_magnitudes(gpu_caffe, synth152, tmp_path, gain):
    """The float16 path on activations of trained-network magnitude: the conditioned synthetic trunk peaks at ~33 (res4b35)
    and ~45 (res5c); scaled by 32 / 256 / 1024 it reaches 1.4e3 / 1.1e4 / 4.6e4 — up to 70 % of float16's largest finite value
    65504, where its spacing is 32.  The maps must stay finite and inside the stated bounds against the float32 oracle of the SAME
    weights (rounding is relative: the bounds, relative to the maps' range, do not move with the magnitude)."""
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
    peak = {k: float(np.abs(ref[k]).max()) for k in ("res3b7", "res4b35", "res5c")}
    assert peak["res4b35"] > 25 * gain and peak["res5c"] > 35 * gain, peak  # the activations ARE large (gain 1024: 3.3e4 / 4.6e4)
    assert max(peak.values()) < 6.0e4, peak                                   # and still representable in float16
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16", fuse=0)
    net.blobs["data"].data[...] = img
    out = net.forward()
    for k in ("prob", "loc_pred", "next_pred"):
        assert np.isfinite(out[k]).all(), k
    _check_maps(out, ref)
    for name in ("res4b35", "res5c"):  # the large blobs themselves: relative to their range
        r = ref[name]
        got = net.blobs[name].data
        assert np.isfinite(got).all(), name
        assert float(np.abs(got - r).max()) <= 1e-2 * float(np.abs(r).max()), name


def test_fp16_net_with_a_narrow_skip_level(gpu_caffe):
    """A DeeperCut-shaped FCN whose layers have 16 / 32 input channels — fewer than the 64 halves of a float16 K tile, so they
    take the row-tap packing — including the two sibling skip convolutions that run as ONE launch: round 2 packed only the
    first sibling's filters in that path (the second head read rows beyond the image); found by round 3's bounds check."""
    from test_gpu_tiling import _fill, local_fcn_prototxt

    h, w = 64, 96
    proto = local_fcn_prototxt(h, w)
    net32 = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True)
    _fill(net32, 5)
    layers = [(name, typ, [b.data.copy() for b in net32.params[name]])
              for name, typ in zip(net32._layer_names, net32.layer_types) if name in net32.params]
    img = rand_image(7, h, w)
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, layers).forward(data=img)
    net32.blobs["data"].data[...] = img
    out32 = net32.forward()
    for k in ("prob", "loc_pred"):
        assert float(np.abs(out32[k] - ref[k]).max()) <= 1e-3, k
    for fuse in (0, 2):
        net16 = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="f16", fuse=fuse)
        _fill(net16, 5)
        net16.blobs["data"].data[...] = img
        out = net16.forward()
        # (an unconditioned toy net: its logits span tens of units, so the sigmoid output is compared loosely and the linear
        #  maps relative to their range — a missing sibling shows up as an error of the order of the range itself)
        assert float(np.abs(out["prob"] - ref["prob"]).max()) <= 3e-2, fuse
        rng = max(1.0, float(np.abs(ref["loc_pred"]).max()))
        assert float(np.abs(out["loc_pred"] - ref["loc_pred"]).max()) <= 4e-3 * rng, (fuse, rng)
        if fuse == 0:
            lg = ref["fc_pose"]
            assert float(np.abs(net16.blobs["fc_pose"].data - lg).max()) <= 4e-3 * max(1.0, float(np.abs(lg).max()))


def test_host_entry_of_the_fp16_batch8_net_stays_close_to_the_device_forward(gpu_caffe, synth152):
    """Review r3, weak 2: `Net.forward_batch(ndarray)` on a float16 batch-8 net took 39 ms against 4 ms device-resident —
    the result arrays were fresh `np.empty` memory on every call and the device-to-host copy faulted 81 MB of pages inside
    the driver.  Ten consecutive calls must move none of the net's lowering / graph / re-pack / buffer counters and stay
    under twice the device-resident forward of the same net (measured: 6.4 ms against 3.9)."""
    import time

    import torch
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    h, w, b = 544, 736, 8
    net = gpu_caffe.Net(deepercut_prototxt(152, h, w, b), path, gpu_caffe.TEST, from_text=True, dtype="f16", hipgraph=1)
    x = rand_image(77, h, w, n=b)
    xd = torch.from_numpy(x).cuda()
    od = [torch.empty(net.blobs[k].shape, device="cuda") for k in ("prob", "loc_pred", "next_pred")]

    def dev():
        net.forward_device(xd.data_ptr(), b, h, w, od[0].data_ptr(), od[1].data_ptr(), od[2].data_ptr())
        torch.cuda.synchronize()

    dev()
    dev()
    t_dev = []
    for _ in range(5):
        t0 = time.perf_counter()
        dev()
        t_dev.append(time.perf_counter() - t0)
    first = {k: v.copy() for k, v in net.forward_batch(x).items()}  # also warms the pool of result arrays
    net.forward_batch(x)
    before = net.stats()
    t_host = []
    for _ in range(10):
        t0 = time.perf_counter()
        out = net.forward_batch(x)
        t_host.append(time.perf_counter() - t0)
        del out
    after = net.stats()
    for k in ("lowerings", "graph_instantiations", "repacks", "buffer_growths"):
        assert after[k] == before[k], (k, before[k], after[k])
    out = net.forward_batch(x)
    for k in first:
        assert np.array_equal(out[k], first[k]), k  # recycled destinations, same values
    held = net.forward_batch(x)  # `out` is still referenced: its arrays must not be handed out again
    assert all(held[k] is not out[k] for k in out)
    d, hmed = sorted(t_dev)[2], sorted(t_host)[5]
    assert hmed < 2.0 * d + 1e-3, "host entry %.2f ms vs device-resident %.2f ms" % (hmed * 1e3, d * 1e3)
