"""CPU: the host side of the two bfloat16 forms — "bs1x1" (the streaming kernel of the dense 1x1 layers, csrc/stream1x1.hip) and "bs7x7"
(the stem, csrc/stem_f16.hip).  Lowering only, like tests/test_bf16_host.py: the forms are OPT-IN (DC_STREAM1X1_BF16 / DC_STEM_BF16, unset
means 0), the float16 switches keep doing nothing for a bfloat16 net, the names are known to set_tile, and the filter image the forms read
loses nothing.  The forward, and a tune-cache file naming the forms (a cache is applied where the device run tunes), are
tests/test_gpu_bf16_stream.py and tests/test_gpu_bf16_stem.py."""
import numpy as np
import pytest

import caffe
from deepcut_tools import deepercut_prototxt
from test_gpu_bf16 import bf16_round

BF16_SWITCHES = ("DC_STREAM1X1_BF16", "DC_STEM_BF16")
F16_SWITCHES = ("DC_WINOGRAD", "DC_STREAM1X1", "DC_STEM")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in BF16_SWITCHES + F16_SWITCHES + ("DC_TUNE_CACHE", "DC_CONV_VARIANT", "DC_CONV_VARIANT_BF16", "DC_AUTOTUNE"):
        monkeypatch.delenv(k, raising=False)


def _net(dtype, h=240, w=320):
    return caffe.Net(deepercut_prototxt(152, h, w), caffe.TEST, from_text=True, dtype=dtype)


def _lines(net):
    return [l for l in net.plan_text().splitlines() if not l.startswith("#")]


def _signatures(net):
    net.plan_text()
    return [r["signature"] for r in net.tune_report()]


def _is_bf16_tile(line):
    return "conv_gemm<" in line and line.split("conv_gemm<")[1].split(">")[0] in set(caffe.conv_variants_bf16())


def test_default_environment_offers_a_bf16_net_no_form():
    nb = _net("bf16")
    lines = _lines(nb)
    assert len(lines) == 158
    assert not any("bs1x1" in l or "bs7x7" in l for l in lines)
    assert not any("+w" in k for k in _signatures(nb))
    # the float16 net of the same shape keeps its forms: before the device run times them a default plan NAMES no form (the lowering puts
    # the cost model's tiles in), it marks the launches a form competes for — 51 ws1x1, conv1 and the 50 stride-1 3x3 layers
    nh = _net("f16")
    nh.plan_text()
    assert sum(r["launches"] for r in nh.tune_report() if r["signature"].endswith("+w")) == 102


def test_forms_forced(monkeypatch):
    base = _net("bf16")
    base_lines, base_flops, base_keys = _lines(base), base.flops(), _signatures(base)
    f16_base = _net("f16").plan_text()
    for k in BF16_SWITCHES:
        monkeypatch.setenv(k, "1")
    monkeypatch.setenv("DC_AUTOTUNE", "0")
    net = _net("bf16")
    lines = _lines(net)
    assert len(lines) == 158 and net.flops() == base_flops
    stream = [i for i, l in enumerate(lines) if "bs1x1<" in l]
    stem = [i for i, l in enumerate(lines) if "bs7x7<" in l]
    assert len(stream) == 51 and len(stem) == 1  # 3 + 8 + 36 + 3 expansions and res2a_branch1; conv1
    assert all("branch2c" in lines[i] or "res2a_branch1" in lines[i] for i in stream) and "conv1" in lines[stem[0]]
    rest = [l for i, l in enumerate(lines) if i not in stream + stem and "\tmaxpool" not in l]
    assert len(rest) == 158 - 52 - 1 and all(_is_bf16_tile(l) for l in rest), [l for l in rest if not _is_bf16_tile(l)][:3]
    # the signatures of exactly those 52 launches say that a form competes for the layer
    launches = [l for l in base_lines if "\tmaxpool" not in l]
    assert len(launches) == 157
    report = {r["signature"]: r for r in net.tune_report()}
    marked = [k for k in report if k.endswith("+w")]
    assert sum(report[k]["launches"] for k in marked) == 52 and all(report[k]["tile"] in ("bs1x1", "bs7x7") for k in marked)
    assert not any("+w" in k for k in report if k not in marked)
    assert sorted(k.replace("+w", "") for k in report) == sorted(base_keys)
    # the two switches are bfloat16 switches
    assert _net("f16").plan_text() == f16_base


def test_float16_switches_do_nothing_for_a_bf16_net(monkeypatch):
    for k in F16_SWITCHES:
        monkeypatch.setenv(k, "1")
    net = _net("bf16")
    lines = [l for l in _lines(net) if "\tmaxpool" not in l]
    assert all(_is_bf16_tile(l) for l in lines)
    assert not any("+w" in k for k in _signatures(net))
    text = _net("f16").plan_text()  # the same switches do give a float16 net its forms, by name
    assert all(f in text for f in ("ws1x1", "stem7x7", "wino_h23"))


def _stream_key(keys, prefix):
    for k in keys:  # <M>/<Cout>/<Ktot>/<klen>/<taps>/<sy>,<sx>/...
        f = k[len(prefix):].split("/")
        if k.startswith(prefix) and f[4] == "1x1" and int(f[2]) <= 512 and f[5].split(",")[0] == "1" and int(f[1]) % 256 == 0 and int(f[2]) in (64, 128, 256, 512):
            return k
    raise AssertionError(keys)


def test_set_tile_takes_the_form_for_bf16_signatures_only(monkeypatch):
    monkeypatch.setenv("DC_STREAM1X1_BF16", "-1")
    monkeypatch.setenv("DC_STEM_BF16", "-1")
    nb, nh = _net("bf16", 64, 64), _net("f16", 64, 64)
    kb, kh = _signatures(nb), _signatures(nh)
    assert "bs1x1" not in nb.plan_text() and "bs7x7" not in nb.plan_text()  # -1: a candidate of the timing, not the lowering's choice
    key_b, key_h = _stream_key(kb, "b"), _stream_key(kh, "h")
    assert key_b.endswith("+w") and key_b[1:] == key_h[1:]
    nb.set_tile(key_b, "bs1x1")
    assert "bs1x1<" in nb.plan_text()
    with pytest.raises(caffe.DeepcutError) as e:
        nh.set_tile(key_h, "bs1x1")
    assert "cannot take" in str(e.value)
    key_3x3 = next(k for k in kb if "/3x3/" in k)
    with pytest.raises(caffe.DeepcutError):
        nb.set_tile(key_3x3, "bs1x1")
    with pytest.raises(caffe.DeepcutError):
        nb.set_tile(key_b, "bs7x7")
    with pytest.raises(caffe.DeepcutError):
        nb.set_tile(key_b, "ws1x1")
    stem_key = next(k for k in kb if "/7x1/" in k)
    nb.set_tile(stem_key, "bs7x7")
    assert "bs7x7<" in nb.plan_text()
    with pytest.raises(caffe.DeepcutError):
        nh.set_tile(next(k for k in kh if "/7x1/" in k), "bs7x7")


def test_set_tile_refuses_the_forms_while_their_switches_are_unset():
    nb = _net("bf16", 64, 64)
    kb = _signatures(nb)
    with pytest.raises(caffe.DeepcutError):
        nb.set_tile(_stream_key(kb, "b"), "bs1x1")
    with pytest.raises(caffe.DeepcutError):
        nb.set_tile(next(k for k in kb if "/7x1/" in k), "bs7x7")


@pytest.mark.parametrize("cout,k", [(256, 64), (512, 128), (64, 512)])
def test_the_filter_image_is_a_permutation_of_the_weights(cout, k):
    """The bf16 forms read dc_stream1x1_pack's image (no row scale, no pre-scale): bf16-representable weights come out as they went in."""
    rs = np.random.RandomState(cout + k)
    g = bf16_round(rs.randn(cout, k, 1, 1))
    g.reshape(-1)[:] += bf16_round(np.arange(cout * k) % 251 * 2.0 ** -3)  # (fewer repeated values)
    g = bf16_round(g)
    img = np.asarray(caffe.stream1x1_pack(g))
    assert img.size == g.size
    assert np.array_equal(np.sort(img.reshape(-1)), np.sort(g.reshape(-1)))
    assert np.array_equal(img, bf16_round(img))
    # fragment order [Cout/32][K/16][64 lanes][8]: lane = 32 ((k % 16) / 8) + co % 32, element k % 8
    flat = img.reshape(-1)
    for co, kk in ((0, 0), (33, 9), (cout - 1, k - 1)):
        assert flat[(((co // 32) * (k // 16) + kk // 16) * 64 + ((kk % 16) // 8) * 32 + co % 32) * 8 + kk % 8] == g[co, kk, 0, 0]
