"""-m gpu: the float16 streaming 1x1 form ("ws1x1", csrc/stream1x1.hip) and stem form ("stem7x7", csrc/stem_f16.hip) against the
REFERENCE to one rounding — their own files (test_gpu_stream1x1.py, test_gpu_stem.py) hold them bit for bit / within 1e-3 x range to a
gather-GEMM tile and, on operands that are not float16 values, to the oracle within 2e-3 x range; an error the form shared with that
tile would pass both.

Here inputs, shortcut and filters are float16 values (f16_operands of test_gpu_fp16.py: none subnormal), the oracle accumulates in
double and applies the BatchNorm / Scale / shortcut / ReLU chain to that sum, so the output's rounding is the only one:
|got - ref| <= ulp_f16(ref) + 1e-5 x max(1, range) — the slack of the forms' bfloat16 twins (test_gpu_bf16_stream.py,
test_gpu_bf16_stem.py).  The cases and net builders are the forms' own: for ws1x1 the single pixel, 25 pixels, 189 pixels without
the affine, one case per K (64, 128, 256, 512) and the 2070-pixel walk; for stem7x7 the pixel-like input scale (randn x 50) on the
1 x 1, 9 x 11, 33 x 129 and 131 x 77 images, which reach every tile edge.  Worst |got - ref| / bound measured on an MI355X: ws1x1 0.491, stem7x7 0.490."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_fp16 import f16_operands, f16_round, f16_ulp
from test_gpu_stem import CASES as STEM_ALL
from test_gpu_stem import _net_text as stem_net_text
from test_gpu_stream1x1 import CASES as STREAM_ALL
from test_gpu_stream1x1 import _net_text as stream_net_text
from test_gpu_stream1x1 import _weights as stream_weights

pytestmark = pytest.mark.gpu

STREAM_CASES = [
    (1, 64, 256, 1, 1, False, True, False),     # a single pixel, no affine (K = 64)
    (1, 256, 512, 5, 5, True, False, True),     # 25 pixels: less than one step
    (3, 128, 256, 7, 9, True, True, False),     # 189 pixels, no affine
    (2, 64, 256, 40, 56, True, True, True),     # K = 64
    (2, 128, 512, 33, 19, True, True, True),    # K = 128
    (1, 512, 256, 16, 16, True, True, True),    # K = 512
    (1, 256, 1024, 45, 46, True, True, True),   # K = 256: the 2070-pixel walk
]
STEM_CASES = [(1, 1, 1, True, False), (3, 9, 11, False, True), (2, 33, 129, False, False), (2, 131, 77, True, True)]
assert set(STREAM_CASES) <= set(STREAM_ALL) and set(STEM_CASES) <= set(STEM_ALL)  # the forms' own cases, not new ones


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DC_AUTOTUNE", "0")
    for k in ("DC_TUNE_CACHE", "DC_CONV_VARIANT", "DC_STREAM1X1", "DC_STEM", "DC_WINOGRAD"):
        monkeypatch.delenv(k, raising=False)


def _reference(proto, weights, **inputs):
    O.set_threads(min(16, os.cpu_count() or 1))
    O.set_double_acc(True)
    try:
        return O.OracleNet(proto, weights).forward(**inputs)
    finally:
        O.set_double_acc(False)


def _run(caffe, proto, weights, inputs, out):
    net = caffe.Net(proto, caffe.TEST, from_text=True, dtype="f16")
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    for k, v in inputs.items():
        net.blobs[k].data[...] = v
    net.forward()
    return net.blobs[out].data.copy(), net.plan_text()


def _hold(got, ref, what):
    assert got.shape == ref.shape
    assert np.array_equal(got, f16_round(got)), "outputs are float16 values"
    bound = f16_ulp(ref) + 1e-5 * max(1.0, float(np.abs(ref).max()))
    err = np.abs(got.astype(np.float64) - ref)
    at = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    print("%s: worst |got - ref| / bound = %.3f at %s (got %r, ref %r, range %.3g)" % (
        what, float((err / bound).max()), at, float(got[at]), float(ref[at]), float(np.abs(ref).max())))
    assert float((err - bound).max()) <= 0, "%s: worst excess %g" % (what, float((err - bound).max()))


@pytest.mark.parametrize("case", STREAM_CASES)
def test_ws1x1_is_one_rounding_from_the_reference(gpu_caffe, case, monkeypatch):
    n, cin, cout, h, w, shortcut, relu, affine = case
    proto, out = stream_net_text(n, cin, cout, h, w, shortcut, relu, affine)
    rs = np.random.RandomState(cin + cout + h)
    weights = stream_weights(rs, cin, cout, affine)
    weights[0] = (weights[0][0], weights[0][1], [f16_operands(weights[0][2][0])])
    inputs = {"data": f16_operands(rs.randn(n, cin, h, w))}
    if shortcut:
        inputs["sc"] = f16_operands(rs.randn(n, cout, h, w))
    monkeypatch.setenv("DC_STREAM1X1", "1")
    got, plan = _run(gpu_caffe, proto, weights, inputs, out)
    assert "ws1x1" in plan, plan
    _hold(got, _reference(proto, weights, **inputs)[out], "ws1x1 %s" % (case,))


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem7x7_is_one_rounding_from_the_reference(gpu_caffe, case, monkeypatch):
    n, h, w, relu, affine = case
    proto = stem_net_text(n, h, w, relu, affine)
    rs = np.random.RandomState(h + w)
    weights = [("conv1", "Convolution", [f16_operands(rs.randn(64, 3, 7, 7) / np.sqrt(147.0))])]
    if affine:
        weights.append(("bn", "BatchNorm", [rs.randn(64).astype(np.float32) * 0.1, rs.uniform(0.5, 1.5, 64).astype(np.float32), np.array([1.0], np.float32)]))
        weights.append(("scale", "Scale", [rs.uniform(0.5, 1.5, 64).astype(np.float32), rs.randn(64).astype(np.float32) * 0.1]))
    x = f16_operands(rs.randn(n, 3, h, w) * 50.0)  # mean-subtracted pixel values
    monkeypatch.setenv("DC_STEM", "1")
    got, plan = _run(gpu_caffe, proto, weights, {"data": x}, "conv1")
    assert "stem7x7" in plan, plan
    _hold(got, _reference(proto, weights, data=x)["conv1"], "stem7x7 %s" % (case,))
