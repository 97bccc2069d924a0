"""-m gpu: "bs7x7", the 7x7 / stride-2 stem of a bfloat16 net (csrc/stem_f16.hip, T = __bf16), forced with DC_STEM_BF16=1 — opt-in:
unset means 0.  Pixels (randn x 50) and filters are bf16 values, so the output's rounding is the only one: against the oracle
|got - ref| <= ulp_bf16(ref) + 1e-5 x max(1, range), and against the row-tap gather-GEMM launch of the same layer the same bound
around that launch's values (another grouping of the float32 sum: at most one rounding flips).  Odd and tiny images, batches, with and
without the affine / the ReLU; the geometries the form does not take; the image entry bit for bit against the host-canvas route."""
import os

import numpy as np
import pytest

from test_gpu_bf16 import bf16_round, bf16_ulp
from test_gpu_stem import _net_text

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DC_AUTOTUNE", "0")
    for k in ("DC_TUNE_CACHE", "DC_CONV_VARIANT", "DC_CONV_VARIANT_BF16", "DC_STREAM1X1_BF16", "DC_STEM_BF16", "DC_STREAM1X1", "DC_STEM", "DC_WINOGRAD"):
        monkeypatch.delenv(k, raising=False)


def _oracle(proto, layers, **inputs):
    from oracle import oracle as O

    O.set_threads(min(16, os.cpu_count() or 1))
    return O.OracleNet(proto, layers).forward(**inputs)


CASES = [  # n, h, w, relu, affine
    (2, 131, 77, True, True),    # odd sizes: tiles hang over both edges, batch 2
    (3, 9, 11, False, True),     # 5 x 6 outputs: less than one tile
    (1, 1, 1, True, False),      # a single pixel: every tap but the centre in the padding; no affine
    (1, 64, 200, True, False),
    (2, 33, 129, False, False),  # 65 output columns: one column into the second tile
]


def _run(caffe, proto, weights, x, mode, monkeypatch):
    monkeypatch.setenv("DC_STEM_BF16", mode)
    net = caffe.Net(proto, caffe.TEST, from_text=True, dtype="bf16")
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    net.blobs["data"].data[...] = x
    net.forward()
    return net.blobs["conv1"].data.copy(), net.plan_text()


@pytest.mark.parametrize("case", CASES)
def test_stem_matches_the_oracle_and_the_row_tap_launch(gpu_caffe, case, monkeypatch):
    n, h, w, relu, affine = case
    proto = _net_text(n, h, w, relu, affine)
    rs = np.random.RandomState(h + w)
    weights = [("conv1", "Convolution", [bf16_round(rs.randn(64, 3, 7, 7) / np.sqrt(147.0))])]
    if affine:
        weights.append(("bn", "BatchNorm", [rs.randn(64).astype(np.float32) * 0.1, rs.uniform(0.5, 1.5, 64).astype(np.float32), np.array([1.0], np.float32)]))
        weights.append(("scale", "Scale", [rs.uniform(0.5, 1.5, 64).astype(np.float32), rs.randn(64).astype(np.float32) * 0.1]))
    x = bf16_round(rs.randn(n, 3, h, w) * 50.0)
    got, plan = _run(gpu_caffe, proto, weights, x, "1", monkeypatch)
    assert "bs7x7" in plan, plan
    direct, plan0 = _run(gpu_caffe, proto, weights, x, "0", monkeypatch)
    assert "bs7x7" not in plan0 and "conv_gemm<b" in plan0
    ref = _oracle(proto, weights, data=x)["conv1"]
    assert got.shape == ref.shape
    assert np.array_equal(got, bf16_round(got)), "outputs are bf16 values"
    rng = max(1.0, float(np.abs(ref).max()))
    e_ref = float((np.abs(got - ref) - (bf16_ulp(ref) + 1e-5 * rng)).max())
    e_dir = float((np.abs(got - direct) - (bf16_ulp(direct) + 1e-5 * rng)).max())
    print("worst excess over the bound: against the oracle %g, against the row-tap launch %g" % (e_ref, e_dir))
    assert e_ref <= 0
    assert e_dir <= 0


def test_only_the_stem_geometry_takes_it(gpu_caffe, monkeypatch):
    monkeypatch.setenv("DC_STEM_BF16", "1")
    base = ['name: "s"', 'input: "data"'] + ["input_dim: %d" % d for d in (1, 3, 32, 32)]
    for conv in ("num_output: 64 kernel_size: 7 pad: 3 stride: 1", "num_output: 64 kernel_size: 5 pad: 2 stride: 2"):
        proto = "\n".join(base + ['layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { %s bias_term: false } }' % conv]) + "\n"
        text = gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="bf16").plan_text()
        assert "bs7x7" not in text and "conv_gemm<b" in text, conv
    proto = "\n".join(base + ['layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: 64 kernel_size: 7 pad: 3 stride: 2 bias_term: false } }']) + "\n"
    assert "bs7x7<" in gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="bf16").plan_text()
    for dt in ("f16", "f32"):
        assert "bs7x7" not in gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype=dt).plan_text()
    monkeypatch.setenv("DC_STEM_BF16", "0")
    assert "bs7x7" not in gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="bf16").plan_text()


def test_image_entry_equals_the_host_canvas_route_on_the_forms(gpu_caffe, synth152, monkeypatch):
    from oracle import preprocess as OP
    from deepcut_tools import deepercut_prototxt
    from pose.estimate_pose import forward_maps

    path, _ = synth152
    monkeypatch.setenv("DC_STEM_BF16", "1")
    monkeypatch.setenv("DC_STREAM1X1_BF16", "1")
    net = gpu_caffe.Net(deepercut_prototxt(152, 64, 64), path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    img = np.random.RandomState(21).randint(0, 256, (150, 210, 3)).astype(np.uint8)
    scale = 0.75
    out = net.forward_images(img, scale, want=("prob", "loc_pred"))
    text = net.plan_text()
    assert "bs7x7<" in text and "bs1x1<" in text
    canvas = OP.preprocess(img, scale)
    assert np.array_equal(net.blobs["data"].data[0].transpose(1, 2, 0), canvas)  # integers in [-123, 151]: exact in bf16
    prob, loc = forward_maps(net, canvas)  # host canvas -> net.forward()
    assert "bs7x7<" in net.plan_text()
    assert np.array_equal(out["prob"][0], prob) and np.array_equal(out["loc_pred"][0], loc)
