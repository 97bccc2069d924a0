"""CPU: the host side of the bfloat16 mode (DC_OPT_DTYPE 2) — option handling, the lowering of the full net onto the bfloat16
tile table, and the tile choices a tune cache / set_tile may hand a bf16 launch.  The forward itself is tests/test_gpu_bf16.py."""
import pytest

import caffe
from deepcut_tools import deepercut_prototxt

F16_ONLY_FORMS = ("wino_h23", "ws1x1", "stem7x7")


def _plan_lines(net):
    text = net.plan_text()
    return text.splitlines()[0], [l for l in text.splitlines() if not l.startswith("#")]


def _tile(line):
    return line.split("conv_gemm<")[1].split(">")[0]


def test_dtype_option_accepts_bfloat16():
    net = caffe.Net(deepercut_prototxt(101, 64, 64), caffe.TEST, from_text=True)
    net.set_option(3, 2)
    assert net.get_option(3) == 2 and net.dtype == "bf16"
    for bad in (3, -1):
        with pytest.raises(caffe.DeepcutError):
            net.set_option(3, bad)
    assert net.get_option(3) == 2
    for spelling in ("bf16", "bfloat16"):
        assert caffe.Net(deepercut_prototxt(101, 64, 64), caffe.TEST, from_text=True, dtype=spelling).dtype == "bf16"


def test_bf16_tile_table():
    names = caffe.conv_variants_bf16()
    assert len(names) > 0 and len(set(names)) == len(names), "tile names are tune-cache keys: unique"
    assert not set(names) & set(n for n, _ in caffe.conv_variants()), "disjoint from the float32 / float16 table"
    assert all(n.startswith("b") for n in names)
    assert len(caffe.conv_variants()) == 55  # the existing table keeps its indices (DC_CONV_VARIANT)


@pytest.mark.parametrize("forms_on", [False, True])
def test_bf16_lowering_on_the_host(monkeypatch, forms_on):
    if forms_on:  # forcing the float16-only forms on must not offer them to a bfloat16 layer
        for k in ("DC_WINOGRAD", "DC_STREAM1X1", "DC_STEM"):
            monkeypatch.setenv(k, "1")
    net = caffe.Net(deepercut_prototxt(152, 240, 320), caffe.TEST, from_text=True, dtype="bf16")
    head, lines = _plan_lines(net)
    assert "dtype=bf16" in head and len(lines) == 158
    names = set(caffe.conv_variants_bf16())
    convs = [l for l in lines if "\tmaxpool" not in l]
    assert all("conv_gemm<" in l and _tile(l) in names for l in convs), [l for l in convs if "conv_gemm<" not in l][:3]
    assert not any(f in l for l in lines for f in F16_ONLY_FORMS)
    assert "K=448 taps=7" in lines[0]  # the stem on the row-tap packing: 7 rows of 8 pixels x 8 channels
    assert abs(net.flops() / 1e9 - 46.24) < 0.01
    if forms_on:  # the same switches do give a float16 net its forms
        f16 = caffe.Net(deepercut_prototxt(152, 240, 320), caffe.TEST, from_text=True, dtype="f16")
        text = f16.plan_text()
        assert all(f in text for f in F16_ONLY_FORMS)


def test_forcing_a_bf16_tile(monkeypatch):
    names = caffe.conv_variants_bf16()
    i = names.index(next(n for n in names if n.startswith("bd")))
    monkeypatch.setenv("DC_CONV_VARIANT_BF16", str(i))
    net = caffe.Net(deepercut_prototxt(152, 72, 104), caffe.TEST, from_text=True, dtype="bf16")
    _, lines = _plan_lines(net)
    used = set(_tile(l) for l in lines if "conv_gemm<" in l)
    assert names[i] in used and len(used) <= 4
    # DC_CONV_VARIANT_BF16 is a bf16 switch: a float16 net is lowered as without it
    monkeypatch.delenv("DC_CONV_VARIANT_BF16")
    base = _plan_lines(caffe.Net(deepercut_prototxt(152, 72, 104), caffe.TEST, from_text=True, dtype="f16"))
    monkeypatch.setenv("DC_CONV_VARIANT_BF16", str(i))
    assert _plan_lines(caffe.Net(deepercut_prototxt(152, 72, 104), caffe.TEST, from_text=True, dtype="f16")) == base


def _signatures(net):
    net.plan_text()  # lowers the current shape
    return [r["signature"] for r in net.tune_report()]


def test_set_tile_refuses_the_other_16_bit_kind():
    proto = deepercut_prototxt(152, 64, 64)
    nb = caffe.Net(proto, caffe.TEST, from_text=True, dtype="bf16")
    nh = caffe.Net(proto, caffe.TEST, from_text=True, dtype="f16")
    kb, kh = _signatures(nb), _signatures(nh)
    assert all(k.startswith("b") for k in kb) and all(k.startswith("h") for k in kh)
    f16_tile = next(n for n, es in caffe.conv_variants() if n.startswith("d128x128x64"))
    bf16_tile = next(n for n in caffe.conv_variants_bf16() if n.startswith("bd128x128x64"))
    key_b = next(k for k in kb if "/1x1/" in k)
    key_h = next(k for k in kh if "/1x1/" in k)
    with pytest.raises(caffe.DeepcutError) as e:
        nb.set_tile(key_b, f16_tile)
    assert "cannot take" in str(e.value)
    with pytest.raises(caffe.DeepcutError):
        nh.set_tile(key_h, bf16_tile)
    with pytest.raises(caffe.DeepcutError):
        nb.set_tile(key_b, "ws1x1")
    nb.set_tile(key_b, bf16_tile)  # its own kind: accepted
    assert "conv_gemm<%s>" % bf16_tile in nb.plan_text()


def test_a_shared_tune_cache_gives_a_bf16_net_no_f16_choice(tmp_path, monkeypatch):
    """One DC_TUNE_CACHE file for float16 and bfloat16 nets: the bf16 signatures carry a prefix of their own ("b"; float16 "h"),
    so the float16 lines of the same shapes never name a bf16 launch's tile.  set_tile reads the file and writes the union back:
    the float16 lines survive, the bf16 net's plan takes no float16 tile.  (A float16 tile written under a bf16 signature by
    hand is refused where the device run applies the file: tests/test_gpu_bf16.py.)"""
    proto = deepercut_prototxt(152, 64, 64)
    nh = caffe.Net(proto, caffe.TEST, from_text=True, dtype="f16")
    kh = _signatures(nh)
    f16_tile = "d128x128x64_w221_s2"
    cache = tmp_path / "tune.txt"
    cache.write_text("".join("%s %s\n" % (k, f16_tile) for k in kh))
    monkeypatch.setenv("DC_TUNE_CACHE", str(cache))
    nb = caffe.Net(proto, caffe.TEST, from_text=True, dtype="bf16")
    kb = _signatures(nb)
    assert not set(kb) & set(kh) and [k[1:] for k in kb] == [k[1:].replace("+w", "") for k in kh]  # same shapes, other prefix, no forms
    bf16_tile = "bd128x128x64_w221_s2"
    nb.set_tile(kb[1], bf16_tile)
    text = nb.plan_text()
    assert "conv_gemm<%s>" % f16_tile not in text and "conv_gemm<%s>" % bf16_tile in text
    assert all(_tile(l) in set(caffe.conv_variants_bf16()) for l in text.splitlines() if "conv_gemm<" in l)
    rows = dict(ln.rsplit(" ", 1) for ln in cache.read_text().splitlines() if ln.strip())
    assert rows[kb[1]] == bf16_tile and all(rows[k] == f16_tile for k in kh)
