"""-m gpu: the bfloat16 path (DC_OPT_DTYPE 2: bf16 operands in HBM, v_mfma_f32_32x32x16_bf16 with float32 accumulation and a
float32 epilogue) against the CPU oracle.

Single layers are checked tightly: inputs and weights are made bf16-representable in numpy, the oracle accumulates in double, and
the one rounding of the output allows |got - ref| <= ulp_bf16(|ref|) + 1e-6 x range.  Max-pool, crop and eltwise are bit-exact
against the oracle rounded to bf16.

Full net (synthetic ResNet-152, batch 2, fuse 0 and 2; every bf16 tile forced at 72x104; the large-activation weights) against the
float32 oracle — measured on an MI355X, bounds at about twice the largest measured error:
  prob                 measured <= 6.7e-3          bound 1.4e-2
  loc_pred, next_pred  measured <= 1.31e-2 x range  bound 2.7e-2 x max(1, range of the map)
Activations are rounded to 8 significant bits after each of 152 layers: ~7-9x the float16 figures (~9e-4, ~1.4e-3 x range)."""
import os
import zlib

import numpy as np
import pytest

from conftest import rand_image
from oracle import oracle as O

pytestmark = pytest.mark.gpu
PROB_TOL, MAP_TOL = 1.4e-2, 2.7e-2


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32: bit arithmetic, NaN kept."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    r = np.where(np.isnan(a), u.astype(np.uint32) | 0x00400000, r)
    return r.view(np.float32).reshape(a.shape)


def bf16_ulp(a):
    e = np.floor(np.log2(np.maximum(np.abs(a), np.float32(2.0 ** -126))))
    return np.exp2(e - 7)


def _check_maps(out, ref, prob_tol=PROB_TOL, map_tol=MAP_TOL, floor=True):
    errs = {}
    errs["prob"] = float(np.abs(out["prob"] - ref["prob"]).max())
    assert errs["prob"] <= prob_tol, errs
    for k in ("loc_pred", "next_pred"):
        rng = max(1.0, float(np.abs(ref[k]).max()))
        errs[k] = float(np.abs(out[k] - ref[k]).max()) / rng
        assert errs[k] <= map_tol, (k, errs)
        if floor:
            assert errs[k] > 1e-5, "suspiciously exact: is the bf16 path really running?"
    print("bf16 errors (prob abs, maps / range):", errs)
    return errs


def _net(caffe, proto, path=None, **kw):
    args = (proto, path) if path else (proto,)
    return caffe.Net(*args, caffe.TEST, from_text=True, dtype="bf16", **kw)


# ---- single layers -----------------------------------------------------------------------------------------------------------
from test_gpu_layers import T2, _inp  # noqa: E402  (the 26 convolution / deconvolution configurations of the net)


@pytest.mark.parametrize("cfg", T2, ids=lambda c: "%s_k%ds%dp%dd%d_%dto%d" % (c[0], c[1], c[2], c[3], c[4], c[6], c[7]))
def test_bf16_conv_deconv_configs(gpu_caffe, cfg):
    kind, k, s, p, d, bias, cin, cout, h, w = cfg
    rs = np.random.RandomState(zlib.crc32(repr(cfg).encode()) & 0x7fffffff)
    typ = "Convolution" if kind == "conv" else "Deconvolution"
    text = _inp("x", (2, cin, h, w)) + (
        'layer { name: "l" type: "%s" bottom: "x" top: "y" convolution_param { num_output: %d kernel_size: %d '
        "stride: %d pad: %d dilation: %d bias_term: %s } }" % (typ, cout, k, s, p, d, "true" if bias else "false"))
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="bf16")
    x = bf16_round(rs.randn(2, cin, h, w))
    wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    wt = bf16_round(rs.randn(*wshape) / np.sqrt(cin * k * k))
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
    assert np.array_equal(got, bf16_round(got)), "outputs are bf16 values"
    rng = float(np.abs(ref).max())
    excess = np.abs(got - ref) - (bf16_ulp(ref) + 1e-6 * rng)
    assert float(excess.max()) <= 0, "worst excess %g (range %g)" % (float(excess.max()), rng)


def test_bf16_filter_upload_rounds_to_nearest_even(gpu_caffe):
    """Weights that are NOT bf16 values: the upload converts them on the device; a 1x1 layer over one-hot inputs reads every
    converted weight back, which must be numpy's round-to-nearest-even of it (ties included)."""
    cin, cout = 64, 64
    rs = np.random.RandomState(5)
    wt = rs.randn(cout, cin, 1, 1).astype(np.float32)
    wt.view(np.uint32)[0, :8, 0, 0] = (wt.view(np.uint32)[0, :8, 0, 0] & 0xFFFF0000) | 0x8000  # exact ties
    text = _inp("x", (1, cin, 1, cin)) + ('layer { name: "l" type: "Convolution" bottom: "x" top: "y" '
                                          "convolution_param { num_output: %d kernel_size: 1 bias_term: false } }" % cout)
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="bf16")
    net.params["l"][0].data[...] = wt
    x = np.zeros((1, cin, 1, cin), np.float32)
    x[0, np.arange(cin), 0, np.arange(cin)] = 1.0  # pixel j holds e_j
    net.blobs["x"].data[...] = x
    y = net.forward()["y"][0, :, 0, :]  # y[co, j] = w[co, j]
    assert np.array_equal(y, bf16_round(wt[:, :, 0, 0]))


@pytest.mark.parametrize("hw", [(3, 5), (15, 20), (33, 47)])
def test_bf16_maxpool_is_exact(gpu_caffe, hw):
    text = _inp("x", (2, 64) + hw) + 'layer { name: "p" type: "Pooling" bottom: "x" top: "y" pooling_param { pool: MAX kernel_size: 3 stride: 2 } }'
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="bf16")
    x = bf16_round(np.random.RandomState(1).randn(2, 64, *hw) * 1e3)
    net.blobs["x"].data[...] = x
    assert np.array_equal(net.forward()["y"], O.maxpool_forward(x, 3, 2))


def test_bf16_eltwise_crop_are_exact(gpu_caffe):
    text = (_inp("a", (2, 14, 9, 11)) + _inp("b", (2, 14, 8, 10)) +
            'layer { name: "c" type: "Crop" bottom: "a" bottom: "b" top: "ac" }'
            'layer { name: "e" type: "Eltwise" bottom: "b" bottom: "ac" top: "s" }')
    net = gpu_caffe.Net(text, gpu_caffe.TEST, from_text=True, fuse=0, dtype="bf16")
    rs = np.random.RandomState(3)
    a, b = bf16_round(rs.randn(2, 14, 9, 11)), bf16_round(rs.randn(2, 14, 8, 10))
    net.blobs["a"].data[...] = a
    net.blobs["b"].data[...] = b
    net.forward()
    ac = O.crop_forward(a, b)
    assert np.array_equal(net.blobs["ac"].data, ac)
    assert np.array_equal(net.blobs["s"].data, bf16_round(O.eltwise_sum(b, ac)))


# ---- the full net --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [0, 2])
@pytest.mark.parametrize("hw", [(64, 64), (104, 136)])
def test_bf16_full_net_matches_oracle(gpu_caffe, synth152, hw, fuse):
    from deepcut_tools import deepercut_prototxt

    path, layers = synth152
    h, w = hw
    proto = deepercut_prototxt(152, h, w, 2)
    net = _net(gpu_caffe, proto, path, fuse=fuse)
    text = net.plan_text()
    assert "dtype=bf16" in text and "conv_gemm<b" in text
    img = rand_image(31, h, w, n=2)
    net.blobs["data"].data[...] = img
    out = net.forward()
    O.set_threads(min(16, os.cpu_count() or 1))
    ref = O.OracleNet(proto, layers).forward(data=img)
    _check_maps(out, ref)
    if fuse == 0:
        for name in ("conv1", "pool1", "res2c", "res3b7", "res4b35", "res5c"):
            r = ref[name]
            assert float(np.abs(net.blobs[name].data - r).max()) <= MAP_TOL * max(1.0, float(np.abs(r).max())), name


def _large_activation_weights(layers, gain):
    """The synthetic weights with a trunk `gain` times larger (conv1's Scale multiplied: the global-statistics BatchNorm layers do
    not re-normalise and ReLU is positively homogeneous) and the six head filters divided by `gain`, so that the maps stay O(1)."""
    out = []
    for name, t, blobs in layers:
        blobs = [b.copy() for b in blobs]
        if name == "scale_conv1":
            blobs = [b * np.float32(gain) for b in blobs]
        if name.startswith("res5c_up_") or name.startswith("res3d_"):
            blobs[0] = blobs[0] / np.float32(gain)
        out.append((name, t, blobs))
    return out


@pytest.mark.parametrize("gain", [4096.0, 16384.0])
def test_bf16_holds_activations_float16_cannot(gpu_caffe, synth152, tmp_path, gain):
    """The case the mode exists for: a trunk whose activations lie beyond float16's largest finite value (65504)."""
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
    peak = {k: float(np.abs(ref[k]).max()) for k in ("res4b35", "res5c")}
    assert min(peak.values()) > 65504.0, peak  # outside float16
    net = _net(gpu_caffe, proto, path, fuse=0)
    net.blobs["data"].data[...] = img
    out = net.forward()
    for k in ("prob", "loc_pred", "next_pred"):
        assert np.isfinite(out[k]).all(), k
    _check_maps(out, ref)
    for name in ("res4b35", "res5c"):
        r, got = ref[name], net.blobs[name].data
        assert np.isfinite(got).all(), name
        assert float(np.abs(got - r).max()) <= 3e-2 * float(np.abs(r).max()), name
    f16 = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype="f16", fuse=0)
    f16.blobs["data"].data[...] = img
    o16 = f16.forward()
    print("gain %g: trunk peak %s; float16 maps finite: %s" % (gain, peak, {k: bool(np.isfinite(v).all()) for k, v in o16.items()}))


# ---- every bf16 tile -----------------------------------------------------------------------------------------------------
H, W = 72, 104
MAX_BF16_VARIANTS = 40


@pytest.fixture(scope="module")
def reference72(synth152):
    from deepcut_tools import deepercut_prototxt

    _, layers = synth152
    O.set_threads(min(16, os.cpu_count() or 1))
    img = rand_image(9, H, W)
    return img, O.OracleNet(deepercut_prototxt(152, H, W), layers).forward(data=img)


def _run_forced(gpu_caffe, synth152, v, img, monkeypatch):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    monkeypatch.setenv("DC_CONV_VARIANT_BF16", str(v))
    net = _net(gpu_caffe, deepercut_prototxt(152, H, W), path)
    net.blobs["data"].data[...] = img
    out = {k: v.copy() for k, v in net.forward().items()}
    used = set(ln.split("\t")[1] for ln in net.plan_text().splitlines() if "conv_gemm<" in ln)
    return out, used


@pytest.mark.parametrize("v", range(MAX_BF16_VARIANTS))
def test_forced_bf16_variant_matches_oracle(gpu_caffe, synth152, reference72, monkeypatch, v):
    table = gpu_caffe.conv_variants_bf16()
    if v >= len(table):
        pytest.skip("the bf16 table has %d entries" % len(table))
    img, ref = reference72
    out, used = _run_forced(gpu_caffe, synth152, v, img, monkeypatch)
    assert "conv_gemm<%s>" % table[v] in used, (table[v], sorted(used))
    assert len(used) <= 4, sorted(used)
    _check_maps(out, ref)


def test_bf16_variant_table_is_covered(gpu_caffe, synth152, reference72, monkeypatch):
    table = gpu_caffe.conv_variants_bf16()
    assert 0 < len(table) <= MAX_BF16_VARIANTS, "raise MAX_BF16_VARIANTS"
    img, _ = reference72
    monkeypatch.setenv("DC_AUTOTUNE", "0")
    _, base = _run_forced(gpu_caffe, synth152, -1, img, monkeypatch)
    _, beyond = _run_forced(gpu_caffe, synth152, len(table), img, monkeypatch)  # out of range: nothing is forced
    assert beyond == base


def test_hand_edited_tune_cache_gives_a_bf16_launch_no_f16_tile(gpu_caffe, synth152, tmp_path, monkeypatch):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    proto = deepercut_prototxt(152, 64, 64)
    probe = _net(gpu_caffe, proto, path)
    probe.plan_text()
    keys = [r["signature"] for r in probe.tune_report()]
    cache = tmp_path / "tune.txt"
    cache.write_text("".join("%s d128x128x64_w221_s2\n%s wino_h23\n" % (k, "h" + k[1:]) for k in keys[::2]) +
                     "".join("%s ws1x1\n" % k for k in keys[1::2]))
    monkeypatch.setenv("DC_TUNE_CACHE", str(cache))
    net = _net(gpu_caffe, proto, path)
    net.blobs["data"].data[...] = rand_image(4, 64, 64)
    net.forward()
    names = set(gpu_caffe.conv_variants_bf16())
    tiles = [ln.split("\t")[1] for ln in net.plan_text().splitlines() if not ln.startswith("#") and "maxpool" not in ln]
    assert all(t.startswith("conv_gemm<") and t[10:-1] in names for t in tiles), sorted(set(tiles))


# ---- device pre-processing and decoding -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net200(gpu_caffe, synth152):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    n = _net(gpu_caffe, deepercut_prototxt(152, 200, 264), path)
    n.forward_batch(rand_image(12, 200, 264, n=2), want=())
    return n


def test_bf16_image_entry_equals_classic_entry(gpu_caffe, synth152):
    from oracle import preprocess as OP
    from deepcut_tools import deepercut_prototxt
    from pose.estimate_pose import forward_maps, pose_from_maps

    path, _ = synth152
    net = _net(gpu_caffe, deepercut_prototxt(152, 64, 64), path)
    img = np.random.RandomState(21).randint(0, 256, (150, 210, 3)).astype(np.uint8)
    for scale in (1.0, 0.75):
        out = net.forward_images(img, scale, want=("prob", "loc_pred"), pose=True)
        canvas = OP.preprocess(img, scale)
        assert np.array_equal(net.blobs["data"].data[0].transpose(1, 2, 0), canvas)  # integers in [-123, 151]: exact in bf16
        prob, loc = forward_maps(net, canvas)  # host canvas -> net.forward()
        assert np.array_equal(out["prob"][0], prob) and np.array_equal(out["loc_pred"][0], loc)
        assert np.allclose(out["pose"][0], pose_from_maps(prob, loc, scale), rtol=0, atol=1e-9)
        assert np.allclose(net.decode_pose(scale)[0], pose_from_maps(prob, loc, scale), rtol=0, atol=1e-9)


def test_bf16_multiperson_decode_matches_oracle(net200):
    from oracle import multiperson as M

    prob, loc, nxt = net200.blobs["prob"].data, net200.blobs["loc_pred"].data, net200.blobs["next_pred"].data
    counts, dets = net200.detect_parts(1.0, 0.5, 1, 16)
    for b in range(prob.shape[0]):
        ref_counts, ref = M.nms_candidates(prob[b], loc[b], 1.0, 0.5, 1, 16)
        assert np.array_equal(counts[b], ref_counts)
        assert np.array_equal(dets[b][:, :, 2:], ref[:, :, 2:])
        assert np.allclose(dets[b][:, :, :2], ref[:, :, :2], rtol=0, atol=1e-9)
    rs = np.random.RandomState(0)
    h, w = nxt.shape[2:]
    cells = [(int(rs.randint(0, 2)), int(rs.randint(0, h)), int(rs.randint(0, w))) for _ in range(20)]
    got = net200.decode_pairwise(np.array(cells), 1.3)
    for b in (0, 1):
        idx = [i for i, c in enumerate(cells) if c[0] == b]
        ref = M.pairwise_positions(nxt[b], [cells[i][1:] for i in idx], 1.3, None, None)
        assert np.allclose(got[idx], ref, rtol=0, atol=1e-9)


# ---- groups, executors, outputs ---------------------------------------------------------------------------------------------
def test_bf16_pyramid_group_equals_members(gpu_caffe, synth152):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    shapes = [(1, 64, 80), (1, 96, 120), (1, 128, 160), (1, 160, 200)]
    net = _net(gpu_caffe, deepercut_prototxt(152, 64, 80), path)
    grp = gpu_caffe.NetGroup.for_shapes(net, shapes, lanes=1)
    imgs = [rand_image(40 + i, h, w, n=n) for i, (n, h, w) in enumerate(shapes)]
    g = grp.forward_batch(imgs)
    assert grp.stats()["multi_launches"] > 100 and "dtype=bf16" in grp.plan_text()
    for i, m in enumerate(grp.nets):
        alone = m.forward_batch(imgs[i])
        for k in ("prob", "loc_pred", "next_pred"):
            rng = 1.0 if k == "prob" else max(1.0, float(np.abs(alone[k]).max()))
            assert float(np.abs(g[i][k] - alone[k]).max()) <= (PROB_TOL if k == "prob" else MAP_TOL * rng), (i, k)


def test_groups_never_mix_element_kinds(gpu_caffe):
    from deepcut_tools import deepercut_prototxt

    a = gpu_caffe.Net(deepercut_prototxt(101, 64, 64), gpu_caffe.TEST, from_text=True, dtype="bf16")
    for other in ("f32", "f16"):
        b = a.clone()
        b.set_option(3, {"f32": 0, "f16": 1}[other])
        with pytest.raises(gpu_caffe.DeepcutError):
            gpu_caffe.NetGroup([a, b])


def test_bf16_clone_pipeline_and_emit_maps(gpu_caffe, synth152):
    import torch
    from deepcut_tools import Pipeline, deepercut_prototxt

    path, _ = synth152
    net = _net(gpu_caffe, deepercut_prototxt(152, 64, 80), path)
    x = rand_image(3, 64, 80)
    ref = {k: v.copy() for k, v in net.forward_batch(x).items()}
    c = net.clone()
    assert c.dtype == "bf16"
    out_c = c.forward_batch(x)
    for k in ref:
        assert out_c[k].dtype == np.float32 and np.array_equal(out_c[k], ref[k]), k
    # emit_maps with element size 2: the bf16 values as they are, widened in numpy == the float32 emit
    bufs = {k: torch.empty(ref[k].shape, dtype=torch.bfloat16, device="cuda") for k in ref}
    net.forward_batch(x)
    net.emit_maps_device(bufs["prob"].data_ptr(), bufs["loc_pred"].data_ptr(), bufs["next_pred"].data_ptr(), half=True)
    torch.cuda.synchronize()
    for k in ref:
        assert np.array_equal(bufs[k].float().cpu().numpy(), ref[k]), k
    f32 = gpu_caffe.Net(deepercut_prototxt(152, 64, 80), path, gpu_caffe.TEST, from_text=True)
    f32.forward_batch(x)
    with pytest.raises(gpu_caffe.DeepcutError):
        f32.emit_maps_device(bufs["prob"].data_ptr(), half=True)
    pipe = Pipeline(c, depth=2, coalesce=1)
    xp = gpu_caffe.pinned_empty((1, 3, 64, 80))
    xp[...] = x
    outs = [gpu_caffe.pinned_empty(ref[k].shape) for k in ("prob", "loc_pred", "next_pred")]
    pipe.submit_host(xp, *outs, tag=0)
    pipe.drain()
    for o, k in zip(outs, ("prob", "loc_pred", "next_pred")):
        assert float(np.abs(o - ref[k]).max()) <= (PROB_TOL if k == "prob" else MAP_TOL * max(1.0, float(np.abs(ref[k]).max()))), k
    del pipe


def test_switching_between_three_dtypes(gpu_caffe, synth152, monkeypatch):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    monkeypatch.setenv("DC_AUTOTUNE", "0")  # the cost model's tiles: the same in every net, so the maps are comparable bit for bit
    proto = deepercut_prototxt(152, 64, 64)
    img = rand_image(32, 64, 64)
    own = {}
    for dt in ("f32", "bf16", "f16"):
        n = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True, dtype=dt)
        n.blobs["data"].data[...] = img
        own[dt] = {k: v.copy() for k, v in n.forward().items()}
    net = gpu_caffe.Net(proto, path, gpu_caffe.TEST, from_text=True)
    for dt, code in (("f32", 0), ("bf16", 2), ("f16", 1), ("f32", 0)):
        net.set_option(3, code)
        net.blobs["data"].data[...] = img
        out = net.forward()
        for k in out:
            assert np.array_equal(out[k], own[dt][k]), (dt, k)
    d = float(np.abs(own["bf16"]["prob"] - own["f32"]["prob"]).max())
    assert 1e-6 < d <= PROB_TOL, d


def test_bf16_nets_leave_no_device_memory_behind(gpu_caffe, synth152):
    import gc

    import torch
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    dev = torch.device("cuda", 0)
    x = rand_image(5, 64, 64)
    free = []
    for _ in range(4):
        n = _net(gpu_caffe, deepercut_prototxt(152, 64, 64), path)
        n.forward_batch(x)
        del n
        gc.collect()
        torch.cuda.synchronize(dev)
        free.append(torch.cuda.mem_get_info(dev)[0] / 2 ** 20)
    assert free[1] - free[-1] <= 2.0, free
