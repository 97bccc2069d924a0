"""CPU: a row-tap launch (one tap per kernel row over several adjacent pixels: inputs narrower than a K tile) takes only tiles whose
K tile is the whole tap.  The kernel checks a lane's tap validity at its column in the tap's first K tile; on a later K tile of the
same tap the lanes past the row end would read the next row's pixels in place of the zero padding — and, on the last row, memory
past the tensor.  A float32 3x3 layer over 16 channels (taps of 64 elements) offers 32-element K tiles that would do exactly that."""
import pytest

import caffe

H, W = 64, 96


def _narrow_net(dtype="f32"):
    from test_gpu_tiling import local_fcn_prototxt

    net = caffe.Net(local_fcn_prototxt(H, W), caffe.TEST, from_text=True, dtype=dtype)
    net.plan_text()
    return net


def _row_tap_key(net):
    rows = [r for r in net.tune_report() if "/3x1/" in r["signature"]]  # c2: 3 row taps of 4 pixels x 16 channels
    assert len(rows) == 1, net.tune_report()
    return rows[0]["signature"]


def test_row_tap_launch_refuses_a_tile_shorter_than_its_tap():
    net = _narrow_net()
    key = _row_tap_key(net)
    assert key.split("/")[3] == "64"  # K per tap
    short = [n for n, es in caffe.conv_variants() if es == 4 and n.split("x")[2].split("_")[0] == "32"]
    whole = [n for n, es in caffe.conv_variants() if es == 4 and n.split("x")[2].split("_")[0] == "64"]
    assert short and whole
    for t in short:
        with pytest.raises(caffe.DeepcutError) as e:
            net.set_tile(key, t)
        assert "cannot take" in str(e.value)
    net.set_tile(key, whole[0])
    assert "conv_gemm<%s>" % whole[0] in net.plan_text()


def test_forcing_a_short_tile_leaves_the_row_tap_launch_on_a_whole_tap_tile(monkeypatch):
    names = [n for n, _ in caffe.conv_variants()]
    i = names.index("32x64x32_w122_p4")
    monkeypatch.setenv("DC_CONV_VARIANT", str(i))
    net = _narrow_net()
    line = [ln for ln in net.plan_text().splitlines() if "taps=3" in ln and "K=192" in ln]
    assert len(line) == 1 and "x64_" in line[0].split("conv_gemm<")[1].split(">")[0], line
