"""-m gpu: "bs1x1", the streaming form of the dense 1x1 layers of a bfloat16 net (csrc/stream1x1.hip, T = __bf16), forced with
DC_STREAM1X1_BF16=1 — the form is opt-in: unset means 0.

Single layers: inputs, shortcut and weights are bf16 values, so the output's rounding is the only one.  The form must equal a bf16
LDS-DMA tile without in-workgroup split-K BIT FOR BIT (the same matrix instruction on the same operands in the same K order, the
bfloat16 gather-GEMM's epilogue), produce bf16 values, and lie within one rounding of the oracle:
|got - ref| <= ulp_bf16(ref) + 1e-5 x max(1, max|ref|)  (float32 accumulation over K <= 512).
The cases are those of tests/test_gpu_stream1x1.py: every K, both wave counts, ragged and tiny M, the peeled / steady / tail steps, every
epilogue combination.  Then the layers the form does not take, the full net, a NetGroup (ONE launch per layer over the members'
tensors), determinism, a tune-cache file that names the form, and the large-activation weights the bfloat16 mode exists for."""
import os

import numpy as np
import pytest

from conftest import rand_image
from test_gpu_bf16 import MAP_TOL, PROB_TOL, _large_activation_weights, bf16_round, bf16_ulp
from test_gpu_stream1x1 import CASES, _net_text, _weights

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


def _direct_tile(caffe):
    """(index, name) of a bf16 LDS-DMA tile whose waves do not split K — the counterpart of float16's d128x64x64_w221_s2 — looked up by name."""
    names = caffe.conv_variants_bf16()
    if "bd128x64x64_w221_s2" in names:
        return names.index("bd128x64x64_w221_s2"), "bd128x64x64_w221_s2"
    for i, n in enumerate(names):
        parts = n.split("_")
        if n.startswith("bd") and len(parts) == 3 and parts[1].startswith("w") and parts[1].endswith("1"):
            return i, n
    raise AssertionError(names)


def _bf16_weights(rs, cin, cout, affine):
    w = _weights(rs, cin, cout, affine)
    w[0] = (w[0][0], w[0][1], [bf16_round(w[0][2][0])])
    return w


def _case_data(case):
    n, cin, cout, h, w, shortcut, relu, affine = case
    proto, out = _net_text(n, cin, cout, h, w, shortcut, relu, affine)
    rs = np.random.RandomState(cin + cout + h)
    weights = _bf16_weights(rs, cin, cout, affine)
    inputs = {"data": bf16_round(rs.randn(n, cin, h, w))}
    if shortcut:
        inputs["sc"] = bf16_round(rs.randn(n, cout, h, w))
    return proto, out, weights, inputs


def _run(caffe, proto, weights, inputs, out, mode, monkeypatch):
    monkeypatch.setenv("DC_STREAM1X1_BF16", mode)
    if mode == "0":
        monkeypatch.setenv("DC_CONV_VARIANT_BF16", str(_direct_tile(caffe)[0]))
    else:
        monkeypatch.delenv("DC_CONV_VARIANT_BF16", raising=False)
    net = caffe.Net(proto, caffe.TEST, from_text=True, dtype="bf16")
    for name, _t, blobs in weights:
        for p, b in zip(net.params[name], blobs):
            p.data[...] = b
    for k, v in inputs.items():
        net.blobs[k].data[...] = v
    net.forward()
    return net.blobs[out].data.copy(), net.plan_text()


@pytest.mark.parametrize("case", CASES)
def test_single_layers_equal_the_tile_bit_for_bit_and_the_oracle_to_one_rounding(gpu_caffe, case, monkeypatch):
    proto, out, weights, inputs = _case_data(case)
    got, plan = _run(gpu_caffe, proto, weights, inputs, out, "1", monkeypatch)
    assert "bs1x1" in plan, plan
    direct, plan0 = _run(gpu_caffe, proto, weights, inputs, out, "0", monkeypatch)
    assert "bs1x1" not in plan0 and _direct_tile(gpu_caffe)[1] in plan0, plan0
    ref = _oracle(proto, weights, **inputs)[out]
    assert got.shape == ref.shape
    bound = bf16_ulp(ref) + 1e-5 * max(1.0, float(np.abs(ref).max()))
    print("worst excess over the bound: form %g, tile %g; form == tile: %s" % (
        float((np.abs(got - ref) - bound).max()), float((np.abs(direct - ref) - bound).max()), np.array_equal(got, direct)))
    assert np.array_equal(got, direct), float(np.abs(got - direct).max())
    assert np.array_equal(got, bf16_round(got)), "outputs are bf16 values"
    assert float((np.abs(got - ref) - bound).max()) <= 0


def test_layers_the_form_does_not_take_keep_their_tiles(gpu_caffe, monkeypatch):
    """Stride 2, 3x3, a channel count that is not a whole slice, K = 1024: lowered onto the bf16 tiles even when the form is forced;
    float16 and float32 nets never see it."""
    monkeypatch.setenv("DC_STREAM1X1_BF16", "1")
    def proto_of(cin, conv):
        base = ['name: "s"', 'input: "data"'] + ["input_dim: %d" % d for d in (1, cin, 16, 16)]
        return "\n".join(base + ['layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { %s bias_term: false } }' % conv]) + "\n"
    for cin, conv in ((64, "num_output: 256 kernel_size: 1 stride: 2"), (64, "num_output: 256 kernel_size: 3 pad: 1"), (64, "num_output: 192 kernel_size: 1"),
                      (1024, "num_output: 256 kernel_size: 1")):
        text = gpu_caffe.Net(proto_of(cin, conv), gpu_caffe.TEST, from_text=True, dtype="bf16").plan_text()
        assert "bs1x1" not in text and "conv_gemm<b" in text, (conv, text)
    proto = proto_of(64, "num_output: 256 kernel_size: 1")
    assert "bs1x1<" in gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype="bf16").plan_text()
    for dt in ("f16", "f32"):
        assert "bs1x1" not in gpu_caffe.Net(proto, gpu_caffe.TEST, from_text=True, dtype=dt).plan_text()


def test_the_form_is_deterministic(gpu_caffe, monkeypatch):
    proto, out, weights, inputs = _case_data(CASES[0])
    a, _ = _run(gpu_caffe, proto, weights, inputs, out, "1", monkeypatch)
    b, _ = _run(gpu_caffe, proto, weights, inputs, out, "1", monkeypatch)
    assert np.array_equal(a, b)


def _maps_within(out, ref):
    assert float(np.abs(out["prob"] - ref["prob"]).max()) <= PROB_TOL
    for k in ("loc_pred", "next_pred"):
        assert float(np.abs(out[k] - ref[k]).max()) <= MAP_TOL * max(1.0, float(np.abs(ref[k]).max())), k


def test_full_net_with_every_eligible_layer_on_the_form(gpu_caffe, synth152, monkeypatch):
    from deepcut_tools import deepercut_prototxt

    path, layers = synth152
    h, w, n = 104, 136, 2
    proto = deepercut_prototxt(152, h, w, n)
    img = rand_image(11, h, w, n=n)
    monkeypatch.setenv("DC_STREAM1X1_BF16", "1")
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    net.blobs["data"].data[...] = img
    on = {k: v.copy() for k, v in net.forward().items()}
    assert sum("bs1x1" in ln for ln in net.plan_text().splitlines()) == 51
    _maps_within(on, _oracle(proto, layers, data=img))
    monkeypatch.setenv("DC_STREAM1X1_BF16", "0")
    off = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    off.blobs["data"].data[...] = img
    ref = off.forward()
    assert "bs1x1" not in off.plan_text()
    _maps_within(on, ref)  # (the tiles the cost model picks may split K inside the workgroup: not bit equality)


def test_group_launches_walk_the_members_tensors_in_one_launch(gpu_caffe, synth152, monkeypatch):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    shapes = [(2, 40, 56), (2, 64, 64), (2, 72, 104), (2, 104, 136)]
    imgs = [rand_image(60 + i, h, w, n=n) for i, (n, h, w) in enumerate(shapes)]
    monkeypatch.setenv("DC_STREAM1X1_BF16", "1")
    n, h, w = shapes[0]
    net = gpu_caffe.Net(deepercut_prototxt(152, h, w, n), path, gpu_caffe.TEST, from_text=True, dtype="bf16", hipgraph=1)
    grp = gpu_caffe.NetGroup.for_shapes(net, shapes, lanes=1)
    outs = grp.forward_batch(imgs)
    text = grp.plan_text()
    assert sum("conv_gemm_mp<bs1x1>" in ln for ln in text.splitlines()) == 51, text[:600]
    monkeypatch.setenv("DC_STREAM1X1_BF16", "0")
    for (n, h, w), img, o in zip(shapes, imgs, outs):
        ref = gpu_caffe.Net(deepercut_prototxt(152, h, w, n), path, gpu_caffe.TEST, from_text=True, dtype="bf16")
        ref.blobs["data"].data[...] = img
        r = ref.forward()
        assert "bs1x1" not in ref.plan_text()
        _maps_within(o, r)


def test_a_tune_cache_names_the_form_for_bf16_signatures_only(gpu_caffe, synth152, tmp_path, monkeypatch):
    """A cache line "<bf16 signature> bs1x1" is applied by the next net's device run (switch at -1: the form is a candidate); the same name
    under the float16 signature of the same shape is ignored and the float16 plan is what it is without the file."""
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    proto = deepercut_prototxt(152, 64, 64)
    img = rand_image(4, 64, 64)
    monkeypatch.setenv("DC_STREAM1X1_BF16", "-1")
    probe = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    probe.plan_text()
    rep_b = probe.tune_report()
    assert "bs1x1" not in probe.plan_text()
    marked = [r["signature"] for r in rep_b if r["signature"].endswith("+w")]
    assert sum(r["launches"] for r in rep_b if r["signature"] in marked) == 51
    f16 = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16")
    f16.blobs["data"].data[...] = img
    f16.forward()
    f16_plan = f16.plan_text()
    rep_h = f16.tune_report()
    cache = tmp_path / "tune.txt"
    h_marked = set("h" + m[1:] for m in marked)  # the float16 signatures of the same shapes
    assert len(h_marked & set(r["signature"] for r in rep_h)) == len(marked)
    lines = ["%s %s" % (r["signature"], "bs1x1" if r["signature"] in marked else r["tile"]) for r in rep_b]
    lines += ["%s %s" % (r["signature"], "bs1x1" if r["signature"] in h_marked else r["tile"]) for r in rep_h]
    cache.write_text("\n".join(lines) + "\n")
    monkeypatch.setenv("DC_TUNE_CACHE", str(cache))
    monkeypatch.setenv("DC_AUTOTUNE", "1")  # (the file holds every signature: nothing is timed)
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    net.blobs["data"].data[...] = img
    out = {k: v.copy() for k, v in net.forward().items()}
    assert sum("bs1x1<" in ln for ln in net.plan_text().splitlines()) == 51 and net.stats()["autotune_runs"] == 0
    again = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16")
    again.blobs["data"].data[...] = img
    again.forward()
    assert "bs1x1" not in again.plan_text() and again.plan_text() == f16_plan
    monkeypatch.setenv("DC_AUTOTUNE", "0")
    monkeypatch.delenv("DC_TUNE_CACHE")
    monkeypatch.setenv("DC_STREAM1X1_BF16", "0")
    off = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    off.blobs["data"].data[...] = img
    _maps_within(out, off.forward())


def test_the_forms_hold_activations_float16_cannot(gpu_caffe, synth152, tmp_path, monkeypatch):
    """Both bf16 forms on the gain-4096 weights of tests/test_gpu_bf16.py: a float16 intermediate anywhere in them would overflow."""
    from deepcut_tools import deepercut_prototxt, write_caffemodel

    _, layers = synth152
    big = _large_activation_weights(layers, 4096.0)
    path = str(tmp_path / "big.caffemodel")
    write_caffemodel(path, "ResNet-152", big)
    h, w = 104, 136
    proto = deepercut_prototxt(152, h, w, 1)
    img = rand_image(33, h, w)
    ref = _oracle(proto, big, data=img)
    assert min(float(np.abs(ref[k]).max()) for k in ("res4b35", "res5c")) > 65504.0
    monkeypatch.setenv("DC_STREAM1X1_BF16", "1")
    monkeypatch.setenv("DC_STEM_BF16", "1")
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="bf16")
    net.blobs["data"].data[...] = img
    out = net.forward()
    text = net.plan_text()
    assert sum("bs1x1<" in ln for ln in text.splitlines()) == 51 and sum("bs7x7<" in ln for ln in text.splitlines()) == 1
    for k in ("prob", "loc_pred", "next_pred"):
        assert np.isfinite(out[k]).all(), k
    _maps_within(out, ref)
